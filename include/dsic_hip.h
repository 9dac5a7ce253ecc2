/* dsic_hip.h — C ABI of libdsic_hip.so, the MI355X (gfx950) hot path of the
 * modelv2 Student-t hyperprior codec.
 *
 * The reference (Dimitrinov74/Domain-Specific-Image-Compression) has no FFI
 * layer: its seam is the Python module API of code/modelv2.  Each entry point
 * below replaces the torch op sequence of the cited reference lines; the
 * ctypes binding a maintainer would add is shown in INTEGRATION.md and lives
 * in domain-specific-image-compression_amd/lib.py.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  All
 *     device work of a call, every launch of a call that makes several, is
 *     enqueued on `stream`, in order: it starts after what the caller enqueued
 *     there before the call and is complete before what the caller enqueues
 *     there after it.  The call returns without waiting for the device, so a
 *     result is read behind `stream` like any other work on it;
 *   - the library allocates nothing and keeps no state; callers own all
 *     buffers including workspaces.  Calls on different streams whose
 *     buffers (workspaces and the Winograd ticket included) are disjoint do
 *     not affect each other, at whatever time they run;
 *     (tests/test_gpu_stream_order.py holds every export to these three)
 *   - activations are NHWC float32 with a channel count that is a multiple
 *     of 8; image tensors at the boundary are NCHW float32 like the
 *     reference's (eval_selfcontained.py:58-59);
 *   - return value: 0 = ok, DSIC_EINVAL = bad argument, DSIC_EHIP = a HIP
 *     runtime error (hipGetLastError text via dsic_last_error()).
 */
#ifndef DSIC_HIP_H
#define DSIC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSIC_OK 0
#define DSIC_EINVAL 1
#define DSIC_EHIP 2

/* activation fused into the conv epilogue */
#define DSIC_ACT_NONE 0
#define DSIC_ACT_GDN 1   /* x / sqrt(beta + gamma*x^2)   layers.py:19-27 */
#define DSIC_ACT_IGDN 2  /* x * sqrt(beta + gamma*x^2)   layers.py:24-25 */
#define DSIC_ACT_RELU 3  /* nn.ReLU                      layers.py:108-111 */
/* Activation layout flag, OR-ed into the s2d_in / s2d_out arguments of dsic_conv3x3_wino_bf16_nhwc and the s2d
 * argument of dsic_conv_first_*: the tensor is chunk-major (CM16) [B][C/16][H][W][16] fp32 instead of NHWC, on the
 * same channel axis (C = 4*Cs in the space-to-depth order for a space-to-depth map).  A 16-channel chunk's window row
 * is then contiguous.  Only layers that dsic_wino_bf16_m64 assigns to the 64-tile kernel read or write it (anything
 * else returns DSIC_EINVAL); Cout a multiple of 16 on the output side. */
#define DSIC_LAYOUT_CM16 2

const char* dsic_last_error(void);
int dsic_abi_version(void);

/* The arithmetic variant of every contraction of the library, one run-time switch (the reference has no such
 * notion: it is torch's fp32 conv, model.py:27-35; both variants are held to its outputs):
 * 1 = operands split into two bf16 planes, bf16 MFMAs, fp32 accumulation (default); 0 = fp32-input MFMAs.
 * The environment variable DSIC_WINO_BF16=0 sets the initial value to 0.  Weights packed for one variant must be
 * re-packed after a switch (the Python layers key their caches on it). */
int dsic_split_bf16(void);
int dsic_set_split_bf16(int on);

/* ---- weight re-layout (once per checkpoint load) ------------------------ */

/* nn.Conv2d weight [Cout,Cin,k,k] (layers.py:29-31) -> packed
 * [k*k][CinP/8][CoutP][8], CinP = ceil8(Cin), CoutP = ceil32(Cout), zero
 * padded.  dst must hold dsic_packed_conv_weight_floats() floats. */
int64_t dsic_packed_conv_weight_floats(int Cout, int Cin, int k);
int dsic_pack_conv_weight(const float* w_oihw, float* dst, int Cout, int Cin,
                          int k, void* stream);

/* nn.ConvTranspose2d(Cin,Cout,5,2,2,output_padding=1) weight [Cin,Cout,5,5]
 * (layers.py:83,89,93,123,124) -> the four sub-pixel phase kernels
 * (3x3,3x2,2x3,2x2 taps = all 25 taps) packed [25][Cin/8][CoutP][8], zero
 * padded: phase py*2+px owns (3-py)(3-px) taps (ty,tx), tx fastest; tap (ty,tx)
 * of output (2i+py,2j+px) reads input (i-1+ty+py, j-1+tx+px) through
 * w[py+4-2(ty+py)][px+4-2(tx+px)].  Cin % 8 == 0; dst holds
 * dsic_packed_conv_weight_floats(Cout, Cin, 5) floats. */
int dsic_pack_convT_weight(const float* w_iohw, float* dst, int Cin, int Cout,
                           void* stream);

/* Last synthesis layer ConvTranspose2d(Cin,Cimg,5,2,2,1) (layers.py:97):
 * the four phases become the 4*Cimg <= 16 output columns of ONE 3x3 stride-1
 * contraction over the input grid; packed [9][Cin/16][16][16] fp32, followed
 * by the same values as two bf16 planes [Cin/16][9][hi,mid][half][16][8]
 * (the B operands of the split-bf16 kernel) = together
 * dsic_convT_image_weight_floats(Cin) floats.  Column ph*Cimg+c is phase
 * ph = py*2+px of image channel c; columns >= 4*Cimg are zero; hi = bf16(v) and
 * mid = bf16(v - hi), both round-to-nearest-even.  Cin % 16 == 0, Cimg in [1,4]. */
int64_t dsic_convT_image_weight_floats(int Cin);
int dsic_pack_convT_image_weight(const float* w_iohw, float* dst, int Cin,
                                 int Cimg, void* stream);

/* ---- layout helpers ------------------------------------------------------ */

/* NCHW image [B,C,H,W] -> NHWC with C padded to 8 (zeros). */
int dsic_image_to_nhwc8(const float* x_nchw, float* dst_nhwc8, int B, int C,
                        int H, int W, void* stream);
/* NHWC [B,H,W,C] -> NCHW [B,C,H,W] */
int dsic_nhwc_to_nchw(const float* src, float* dst, int B, int H, int W, int C,
                      void* stream);
/* NCHW [B,C,H,W] -> NHWC [B,H,W,C] */
int dsic_nchw_to_nhwc(const float* src, float* dst, int B, int C, int H, int W,
                      void* stream);

/* F.pad(x,(0,pad_w,0,pad_h),mode="reflect") on [planes,H,W] (modelseval.py:57-64:
 * pad bottom/right to a multiple of 16).  dst: [planes,H+pad_h,W+pad_w]. */
int dsic_reflect_pad_br(const float* src, float* dst, int planes, int H, int W,
                        int pad_h, int pad_w, void* stream);

/* Band preparation of code/combinebandsall.py:7-12,35-36 for stacked Sentinel-2 bands:
 * per plane b -= min(b); b /= max(b) (if non-zero).  bands/out01: [planes][HW] float32
 * (planes = images x bands); out_u8 (may be NULL): uint8(b*255) as written to PNG. */
int dsic_normalize_bands(const float* bands, float* out01, uint8_t* out_u8,
                         int planes, int HW, void* stream);

/* ---- convolutions (fp32 MFMA implicit GEMM, fused bias + activation) ----- */

/* conv() + optional GDN/ReLU: nn.Conv2d(Cin,Cout,k,stride,padding=(k-1)/2)
 * (layers.py:29-31, 51-72, 86-94, 108-112).  k in {3,5}; (k,stride) in
 * {(3,1),(5,2)}.  in: NHWC [B,H,W,CinP]; out: NHWC [B,Ho,Wo,Cout],
 * Ho = ceil(H/stride).  beta/gamma are the EFFECTIVE per-channel values
 * (param^2 - 2^-18, layers.py:20-21); ignored unless act is GDN/IGDN. */
int dsic_conv2d_nhwc(const float* in, const float* w_packed, const float* bias,
                     const float* beta, const float* gamma, float* out, int B,
                     int H, int W, int CinP, int Cout, int k, int stride,
                     int act, void* stream);

/* 3x3 stride-1 conv() + optional GDN/IGDN/ReLU by Winograd F(2x2,3x3) on the
 * fp32 MFMA (layers.py:56,62,67,86,90,94,108,109): 2.25x fewer multiplies than
 * dsic_conv2d_nhwc, same fp32 operands.  u_packed from dsic_pack_wino_weight
 * (G g G^T per (cout,cin), [16 positions xi*4+nu][CinP/8][CoutP][8], CinP = ceil8(Cin),
 * CoutP = ceil32(Cout), zero padded, dsic_wino_weight_floats() floats; the packer takes
 * any Cin, the kernels below do not).  Cin % 32 == 0, Cout % 4 == 0,
 * Cout <= 128.  in NHWC [B,H,W,Cin] -> out NHWC [B,H,W,Cout].  ticket: 16 bytes of device
 * memory zeroed ONCE by the caller (dynamic tile hand-out of the persistent kernel; each launch
 * leaves it zeroed again; launches sharing a ticket must be ordered on one stream). */
int64_t dsic_wino_weight_floats(int Cout, int Cin);
int dsic_pack_wino_weight(const float* w_oihw, float* dst, int Cout, int Cin,
                          void* stream);
int dsic_conv3x3_wino_nhwc(const float* in, const float* u_packed,
                           const float* bias, const float* beta,
                           const float* gamma, float* out, int B, int H, int W,
                           int Cin, int Cout, int act, int s2d_out, int s2d_in,
                           void* ticket, void* stream);
/* conv(Cs,Cout,5,2) (layers.py:54,60,65) as a 3x3 stride-1 Winograd conv over the
 * space-to-depth input [B,H/2,W/2,4*Cs] (channel (a*2+b)*Cs+c = x[2i+a][2j+b][c],
 * written by the producing layer when its s2d_out flag is set): 16 instead of
 * 25 multiplies per output and channel pair.  Pack the reference [Cout,Cs,5,5]
 * weight with dsic_pack_wino_s2_weight and call dsic_conv3x3_wino_nhwc with
 * Cin = 4*Cs on the half-resolution grid and s2d_in = 1 (lets the kernel skip the
 * Winograd positions that are structurally zero for the phases lacking a tap row/column). */
int dsic_pack_wino_s2_weight(const float* w_oihw5, float* dst, int Cout, int Cs,
                             void* stream);
/* ConvTranspose2d(Cin,Cout,5,2,2,output_padding=1) + optional IGDN/ReLU
 * (layers.py:83,89,93,123,124) by Winograd: each sub-pixel phase (py,px) is a 3x3
 * stride-1 conv over the input grid with taps g[wr][wc] = w[py+4-2wr][px+4-2wc]
 * (zero for wr < py or wc < px), so all four share the transformed input.  dst/u_packed4:
 * 4 * dsic_wino_weight_floats(Cout, Cin) floats.  in NHWC [B,H,W,Cin] -> out NHWC
 * [B,2H,2W,Cout].  Cin % 32 == 0, Cout % 4 == 0, Cout <= 128. */
int dsic_pack_wino_convT_weight(const float* w_iohw5, float* dst, int Cin,
                                int Cout, void* stream);
int dsic_conv_transpose2d_wino_nhwc(const float* in, const float* u_packed4,
                                    const float* bias, const float* beta,
                                    const float* gamma, float* out, int B,
                                    int H, int W, int Cin, int Cout, int act,
                                    void* ticket, void* stream);

/* Winograd layers on the bf16 MFMA path with fp32-class results (csrc/conv_wino_bf16.hip): the
 * fp32 operands are split into bf16 planes (x = hi + mid [+ lo]) and the cross products are
 * accumulated in fp32.  dsic_wino_bf16_planes(): planes the library was built with (2: products
 * hh, hm, mh; 3: + mm, hl, lh).  u_f32: transformed weights as written by dsic_pack_wino_weight /
 * dsic_pack_wino_s2_weight (nphase 1) or dsic_pack_wino_convT_weight (nphase 4); dst:
 * nphase * dsic_wino_bf16_weight_bytes(Cout, Cin) bytes, [phase][16][Cin/16][planes][CoutP][16] bf16;
 * plane q = bf16(rem_q) round-to-nearest-even, rem_0 = u, rem_q+1 = rem_q - plane_q.  Cin % 32 == 0.
 * The two conv entry points mirror dsic_conv3x3_wino_nhwc / dsic_conv_transpose2d_wino_nhwc
 * (same layers of code/modelv2/layers.py:54-72, 83-97, 108-124; Cin a multiple of 32, >= 64).
 * out_cstride / out_coff (floats; 0 / 0 = a dense [B,H,W,Cout] output): the Cout <= 128 channels of this
 * call are a slice of a wider NHWC tensor - conv(128,192,5,2) (layers.py:72) runs as a 128- and a
 * 64-channel call into one [B,H,W,192] tensor. */
int dsic_wino_bf16_planes(void);
int64_t dsic_wino_bf16_weight_bytes(int Cout, int Cin);
int dsic_split_wino_weight_bf16(const float* u_f32, void* dst, int Cout, int Cin,
                                int nphase, void* stream);
int dsic_conv3x3_wino_bf16_nhwc(const float* in, const void* u_planes,
                                const float* bias, const float* beta,
                                const float* gamma, float* out, int B, int H, int W,
                                int Cin, int Cout, int act, int s2d_out, int s2d_in,
                                int out_cstride, int out_coff, void* ticket, void* stream);
/* Split-K for layers whose images hold fewer than four 16x8-pixel tiles (g_a.10/12/14, h_a.*: layers.py:66-72,
 * 108-112 on 16x16 .. 4x4 latents), where a workgroup would otherwise walk all Cin/16 chunks of a tile alone:
 * dsic_wino_bf16_ksplit(H, W, Cin) -> S (a function of the layer geometry only, 1 = do not split);
 * dsic_conv3x3_wino_bf16_splitk_nhwc = dsic_conv3x3_wino_bf16_nhwc with the input channels of every tile
 * shared by S work items, whose partial sums (partials: S buffers of the size of `out`, caller-owned) are
 * added in fixed order, biased and activated by a second launch. */
int dsic_wino_bf16_ksplit(int H, int W, int Cin);
/* 1 when dsic_conv3x3_wino_bf16_nhwc / dsic_conv_transpose2d_wino_bf16_nhwc run the layer with the 64-tile,
 * two-pass kernel (csrc/conv_wino_bf16m.hip: H and W multiples of 16, at least 4 work items per image; nphase = 4
 * for ConvTranspose2d, 1 otherwise) - a function of the layer geometry only, like the split-K rule. */
int dsic_wino_bf16_m64(int H, int W, int Cin, int nphase);
/* The 64-tile kernel runs two pass-B chunks whose Winograd row xi = 3 (5x5/s2 over space-to-depth) or xi = 0
 * (ConvTranspose2d phases 2, 3) is structurally zero as one chunk-pass; results are bit-identical either way.
 * dsic_wino_pair_chunks(on): 1 / 0 switches that on / off for later launches (default on; DSIC_WINO_PAIR=0 in the
 * environment: off), a negative value only asks; returns the previous setting.
 * dsic_wino_pair_schedule: host restatement of a tile's pass B from the kernel's own tables - the (chunk, position
 * xi*4 + nu) pairs that accumulator acc (0..3) of wave half pq (0, 1) receives, in order, in the paired (1) or
 * unpaired (0) schedule of mode 0 (3x3) / 1 (space-to-depth) / 2 (ConvTranspose2d item of `phase`) with nchunks =
 * Cin/16; writes up to cap pairs of ints to out and returns their number (negative: bad arguments or a table
 * that contradicts itself). */
int dsic_wino_pair_chunks(int on);
/* The Winograd kernels are persistent: a launch has one workgroup per compute unit of the device (DSIC_WINO_GRID =
 * 1..1024 in the environment: that many), at most one per work item, and each takes work items from the ticket
 * until none is left; an output element is the work of one item, so results are bit-identical at every grid.
 * dsic_wino_grid(n): n = 1..1024 caps the grid of later launches at n workgroups on every device (tests walk a
 * workgroup through many items at small shapes), 0 returns to the default, a negative value only asks, a value
 * above 1024 changes nothing and returns -1; otherwise returns the previous cap (0: none). */
int dsic_wino_grid(int n);
int dsic_wino_pair_schedule(int mode, int nchunks, int phase, int paired, int pq, int acc, int* out, int cap);
int dsic_conv3x3_wino_bf16_splitk_nhwc(const float* in, const void* u_planes,
                                       const float* bias, const float* beta,
                                       const float* gamma, float* out, int B, int H, int W,
                                       int Cin, int Cout, int act, int s2d_out, int s2d_in,
                                       int out_cstride, int out_coff, int ksplit,
                                       float* partials, void* ticket, void* stream);
int dsic_conv_transpose2d_wino_bf16_nhwc(const float* in, const void* u_planes4,
                                         const float* bias, const float* beta,
                                         const float* gamma, float* out, int B,
                                         int H, int W, int Cin, int Cout, int act,
                                         void* ticket, void* stream);
/* The same with the input / output layout chosen: layout_in, layout_out 0 (NHWC) or DSIC_LAYOUT_CM16. */
int dsic_conv_transpose2d_wino_bf16_layout(const float* in, const void* u_planes4,
                                           const float* bias, const float* beta,
                                           const float* gamma, float* out, int B,
                                           int H, int W, int Cin, int Cout, int act,
                                           int layout_in, int layout_out, void* ticket,
                                           void* stream);

/* First analysis layer conv(Cimg,Cout,3,1) + optional GDN/ReLU (layers.py:51)
 * read straight from the NCHW image [B,Cimg,H,W] (Cimg 3 or 4) with K = 9*Cimg;
 * w_oihw is the reference weight [Cout,Cimg,3,3] unpacked; out NHWC [B,H,W,Cout],
 * Cout a multiple of 4, <= 128.  s2d_out: store space-to-depth
 * [B,H/2,W/2,4*Cout] for a following 5x5/s2 layer run by Winograd; | DSIC_LAYOUT_CM16: store
 * chunk-major [B,C/16,H',W',16] (Cout a multiple of 16). */
int dsic_conv_first_nchw(const float* x_nchw, const float* w_oihw,
                         const float* bias, const float* beta,
                         const float* gamma, float* out_nhwc, int B, int Cimg,
                         int H, int W, int Cout, int act, int s2d_out,
                         void* stream);
/* The same layer from the decoded image bytes: x_u8_nhwc [B][H][W][Cimg] uint8 (PIL / numpy layout);
 * to_tensor (code/modelv2/modelseval.py:66-67, eval_selfcontained.py:58-59: float(v)/255) is fused
 * into the kernel's window staging. */
int dsic_conv_first_u8hwc(const unsigned char* x_u8_nhwc, const float* w_oihw,
                          const float* bias, const float* beta, const float* gamma,
                          float* out_nhwc, int B, int Cimg, int H, int W, int Cout,
                          int act, int s2d, void* stream);
/* to_tensor alone: uint8 [B][H][W][C] -> float32 [B][C][H][W] in [0,1] (the x of the metrics). */
int dsic_image_u8hwc_to_f32nchw(const unsigned char* x_u8_nhwc, float* out_nchw,
                                int B, int C, int H, int W, void* stream);


/* ConvTranspose2d(Cin,Cout,5,2,2,output_padding=1) + optional IGDN/ReLU.
 * in NHWC [B,H,W,Cin] -> out NHWC [B,2H,2W,Cout]. */
int dsic_conv_transpose2d_nhwc(const float* in, const float* w_packed,
                               const float* bias, const float* beta,
                               const float* gamma, float* out, int B, int H,
                               int W, int Cin, int Cout, int act, void* stream);

/* Last synthesis layer: in NHWC [B,H,W,Cin] -> x_hat NCHW [B,Cimg,2H,2W]. */
int dsic_conv_transpose2d_image(const float* in, const float* w_packed,
                                const float* bias, float* out_nchw, int B,
                                int H, int W, int Cin, int Cimg, void* stream);

/* ---- hyper-synthesis heads, quantisation, rate --------------------------- */

/* AdaptiveAvgPool2d(1) -> mlp_sigma / mlp_nu (1x1 conv, ReLU, 1x1 conv)
 * (layers.py:131-139,147-151), then sigma = exp(log_sigma),
 * nu = clamp(exp(log_nu), min_nu, max_nu) (model.py:54-55; the spatial mean
 * of a spatially constant tensor is the tensor).  t: NHWC [B,HW,N] = ReLU
 * output of h_s.  1x1 weights are passed INPUT-major: w1 [N][N], w2 [N][M]
 * (= reference weight[o,i,0,0] transposed).  Outputs [B,M]. */
int dsic_hyper_params(const float* t_nhwc, const float* w1_sigma,
                      const float* b1_sigma, const float* w2_sigma,
                      const float* b2_sigma, const float* w1_nu,
                      const float* b1_nu, const float* w2_nu,
                      const float* b2_nu, float* log_sigma, float* log_nu,
                      float* sigma, float* nu, int B, int HW, int N, int M,
                      float min_nu, float max_nu, void* stream);

/* quantize("round") (model.py:27-35, 44-45, 62), StudentT.neg_log2_prob
 * (distributions.py:20-31), FactorizedGaussian.neg_log2_prob
 * (distributions.py:39-46) and the per-image sums behind model.py:76.
 * y NHWC [B,HWy,M], z NHWC [B,HWz,N]; sigma, nu [B,M]; z_log_sigma [N].
 * per_element: sigma, nu are NCHW [B,M,HWy] (spatial_params=True) instead of [B,M].
 * y_noisy/z_noisy (NHWC, may be NULL): when given they ARE y_tilde/z_tilde
 * (quant_mode="noise"), otherwise y_tilde = round(y).  Outputs: y_hat NHWC
 * (= round(y), the synthesis input), y_tilde/z_tilde/nll_y/nll_z in the
 * reference's NCHW, sums[B][2] = {sum nll_y, sum nll_z} as fp64 (each image is
 * summed by 16 workgroups whose partial sums are added in a fixed order).
 * work: dsic_rate_workspace_doubles(B) doubles of device scratch. */
int64_t dsic_rate_workspace_doubles(int B);
int dsic_rate(const float* y_nhwc, const float* z_nhwc,
              const float* y_noisy_nhwc, const float* z_noisy_nhwc,
              const float* sigma, const float* nu, const float* z_log_sigma,
              float* y_hat_nhwc, float* y_tilde_nchw, float* z_tilde_nchw,
              float* nll_y_nchw, float* nll_z_nchw, double* sums, double* work,
              int B, int HWy, int M, int HWz, int N, int per_element, void* stream);

/* spatial_params=True branch of model.py:49-51: the two 3x3 heads' NHWC outputs
 * [B,HW,M] -> sigma = exp(log_sigma), nu = clamp(exp(log_nu), min_nu, max_nu) as
 * NCHW [B,M,HW]; dsic_rate / dsic_cdf_tables_student then take per_element = 1. */
int dsic_sigma_nu_spatial(const float* log_sigma_nhwc, const float* log_nu_nhwc,
                          float* sigma_nchw, float* nu_nchw, int B, int HW, int M,
                          float min_nu, float max_nu, void* stream);

/* StudentT.neg_log2_prob (distributions.py:20-31) elementwise on NCHW x[n].
 * per_channel=1: sigma/nu are [B*C] (spatially constant, HW elements each);
 * per_channel=0: sigma/nu are full tensors of n elements. */
int dsic_student_t_bits(const float* x, const float* sigma, const float* nu,
                        float* out, int64_t n, int HW, int per_channel,
                        void* stream);
/* FactorizedGaussian.neg_log2_prob (distributions.py:39-46), x NCHW. */
int dsic_gaussian_bits(const float* x, const float* log_sigma, float* out,
                       int B, int C, int HW, void* stream);

/* torch.round (half to even) elementwise: quantize(x,"round"), model.py:32-33 */
int dsic_round(const float* x, float* out, int64_t n, void* stream);

/* Stand-alone GDN (inverse=0) / IGDN (inverse=1) on NCHW (layers.py:19-27);
 * beta/gamma are the effective per-channel values. */
int dsic_gdn_nchw(const float* x, const float* beta, const float* gamma,
                  float* out, int B, int C, int HW, int inverse, void* stream);

/* ---- distortion metrics -------------------------------------------------- */

/* One MS-SSIM level (pytorch-msssim 1.0.0 semantics, called at
 * modelseval.py:78-88, eval_selfcontained_entropy.py:154): 11-tap Gaussian
 * "valid" filtering, cs/ssim maps, spatial means.  X,Y: [planes,H,W] (planes =
 * B*C of an NCHW tensor); partial: workspace of dsic_ssim_partial_doubles()
 * doubles; means: [planes][2] = (mean cs, mean ssim).  clamp_x clamps X to
 * [0,1] on load (modelseval.py:178). */
int64_t dsic_ssim_partial_doubles(int planes, int H, int W);
int dsic_ssim_level(const float* X, const float* Y, double* partial,
                    double* means, int planes, int H, int W, float C1, float C2,
                    int clamp_x, void* stream);
/* The same level plus the inputs of the next one: Xn, Yn [planes,Hn,Wn] =
 * F.avg_pool2d(kernel=2, padding=size%2) of (clamped) X and of Y
 * (pytorch-msssim's downsampling between levels, modelseval.py:80-85), Hn =
 * (H + 2*(H%2) - 2)/2 + 1.  For even H and W % 4 == 0
 * (dsic_ssim_level_pool_fused) the pool comes out of the pass that reads the
 * level; other shapes run dsic_ssim_level + 2 x dsic_avgpool2. */
int dsic_ssim_level_pool_fused(int H, int W);
int dsic_ssim_level_pool(const float* X, const float* Y, double* partial,
                         double* means, float* Xn, float* Yn, int planes, int H,
                         int W, float C1, float C2, int clamp_x, void* stream);
/* F.avg_pool2d(kernel=2, padding=size%2) between MS-SSIM levels. */
int dsic_avgpool2(const float* src, float* dst, int planes, int H, int W,
                  int clamp, void* stream);
/* out[b] = mean_c prod_l relu(v_l)^w_l from means [levels][B*C][2]. */
int dsic_msssim_finalize(const double* means, const float* weights, float* out,
                         int levels, int B, int C, int relu_last, void* stream);
/* out[b] = sum (a-b)^2 over one image (F.mse_loss numerator,
 * modelseval.py:69-76); clamp_a clamps a to [0,1] first. */
int dsic_sqerr_per_image(const float* a, const float* b, double* out, int B,
                         int64_t n_per_image, int clamp_a, void* stream);

/* ---- per-patch entropy coding ------------------------------------------- */
/* Restates custom_compress / custom_decompress of
 * code/modelv2/eval_selfcontained_entropy.py:26-123 and the torchac 0.9.3
 * calls inside them (third-party; :48,62,96,116).  The script cannot execute
 * as written; the frozen interpretation is in DESIGN.md.
 * err: device int, OR-ed with 1 (a support with L < 1 or L > Lmax), 2 (symbol
 * outside its support), 4 (output capacity exceeded); callers zero it first. */

/* :39-41,52-54: meta[b] = {floor(min(y))-tail, Ly, floor(min(z))-tail, Lz},
 * L = ceil(max)-floor(min)+2*tail+1, tail >= 0.
 * y_nchw/z_nchw: float latents (y_tilde, z_tilde: integer-valued), n_* >= 1 per image.
 * Only |v| < 1e9 is admitted: a NaN, an infinity or a larger magnitude anywhere in y (z)
 * of an image sets that half of meta[b] to (0, 0), which every consumer refuses with err
 * bit 1; the other half and the other images are unaffected. */
int dsic_latent_support(const float* y_nchw, const float* z_nchw, int* meta,
                        int B, int64_t n_y, int64_t n_z, int tail, void* stream);

/* :43-47 gaussian PMF -> pmf_to_uint16_cdf (:17-23) -> spread table.
 * sigma_z [N] = exp(z_prior.log_sigma) (:32, no clamp); tables [B][N][Lmax]
 * uint16, entry k = c[k] for k < L_b (c[L_b] = 65536 implicit).
 * Both table calls: any sigma >= 0 is accepted, 0 and inf included (NaN is undefined),
 * and any nu > 0; nothing is clamped.  Exactly the entries [0, L_b) of a row are written;
 * an image whose support has L_b < 1 or L_b > Lmax raises err bit 1 and none of its rows
 * is touched, while the other images of the call get their tables.  1 <= Lmax <= 1000. */
int dsic_cdf_tables_gauss(const float* sigma_z, const int* meta,
                          uint16_t* tables, int B, int N, int Lmax, int* err,
                          void* stream);
/* :55-61 Student-t PMF tables; sigma, nu [B][rows]: rows = M for spatially constant
 * parameters (spatial_params=False), rows = M*Hy*Wy (NCHW order = symbol order)
 * for per-element parameters (spatial_params=True, layers.py:127-129). */
int dsic_cdf_tables_student(const float* sigma, const float* nu,
                            const int* meta, uint16_t* tables, int B, int rows,
                            int Lmax, int* err, void* stream);

/* torchac.encode_float_cdf call sites :48,62: per image the z string then the
 * y string.  per_element_y: tab_y has one row per y symbol ([B][M*HWy][Lmax])
 * instead of one per channel.  out: [B][cap_z + cap_y] bytes, ZERO-INITIALISED by the caller (bits
 * are OR-ed in; z at offset 0, y at cap_z),
 * lengths [B][2] = {len_z, len_y}.  Symbol order C,H,W of the NCHW latents. */
int dsic_range_encode(const float* y_nchw, const float* z_nchw, const int* meta,
                      const uint16_t* tab_y, const uint16_t* tab_z, int Lmax,
                      int B, int M, int HWy, int N, int HWz, uint8_t* out,
                      int64_t cap_y, int64_t cap_z, int* lengths, int* err,
                      int streams_per_wg, int per_element_y, void* stream);

/* dsic_range_encode in three launches on `stream` (pack: every symbol's interval; chain: the serial interval
 * recurrence, one small wave per string; place: bit offsets and bits in parallel).  Same arguments and the same
 * out, lengths and err, without streams_per_wg; `workspace` is device memory of at least
 * dsic_range_encode_workspace_size(B, M, HWy, N, HWz) bytes, private to this call until the stream passes it.
 * The workspace size is -1 for a bad shape. */
int64_t dsic_range_encode_workspace_size(int B, int M, int HWy, int N, int HWz);
int dsic_range_encode_ws(const float* y_nchw, const float* z_nchw, const int* meta,
                         const uint16_t* tab_y, const uint16_t* tab_z, int Lmax,
                         int B, int M, int HWy, int N, int HWz, uint8_t* out,
                         int64_t cap_y, int64_t cap_z, int* lengths, int* err,
                         int per_element_y, void* workspace, int64_t workspace_bytes, void* stream);

/* Segmented y strings: the y string of an image is coded as segs (1, 2, 4, 8 or 16, dividing M) independent
 * range-coder strings, segment k = channels [k*M/segs, (k+1)*M/segs) (a contiguous symbol range and a contiguous
 * block of table rows), all with the image's one support.  Arguments as dsic_range_encode_ws, with cap_seg (a multiple
 * of 4, >= 8) the capacity of one segment: out [B][cap_z + segs*cap_seg] zero-initialised, the z string at 0,
 * segment k at cap_z + k*cap_seg; lengths [B][1 + segs] = {len_z, len_y0 .. len_y(segs-1)}.  segs = 1 is
 * dsic_range_encode_ws.  The z string is never segmented. */
int64_t dsic_range_encode_seg_workspace_size(int B, int M, int HWy, int N, int HWz, int segs);
int dsic_range_encode_seg_ws(const float* y_nchw, const float* z_nchw, const int* meta,
                             const uint16_t* tab_y, const uint16_t* tab_z, int Lmax,
                             int B, int M, int HWy, int N, int HWz, uint8_t* out,
                             int64_t cap_seg, int64_t cap_z, int* lengths, int* err,
                             int per_element_y, int segs, void* workspace, int64_t workspace_bytes,
                             void* stream);

/* torchac.decode_float_cdf call sites :96,116: string b starts at
 * in + b*stride and has lengths[b*lstride + loff] bytes; meta_off 0 = y, 2 = z.
 * out: NCHW float latents [B][C][HW] (symbol + min).
 * The bytes at and behind lengths[...] (zeros stand in for them) and the table entries k >= L_b of a
 * row (c[L_b] = 65536 is implicit) are never interpreted: both may hold anything.  Any bytes decode
 * to symbols inside the support.  An image whose L_b is < 1 or > Lmax raises err bit 1 and keeps its
 * part of out untouched; the other images decode. */
int dsic_range_decode(const uint8_t* in, int64_t stride, const int* lengths,
                      int lstride, int loff, const int* meta, int meta_off,
                      const uint16_t* tables, int Lmax, int B, int C, int HW,
                      int per_element, float* out_nchw, int* err, void* stream);

/* dsic_range_decode of segmented strings, one wave per (string, segment): the segs segments of string b lie back
 * to back from in + b*stride (4-byte aligned), segment k at byte sum_{j<k} seg_lengths[b*segs + j] with
 * seg_lengths[b*segs + k] bytes, at any alignment.  Starts and lengths are cut to what is left of
 * lengths[b*lstride + loff]: a forged length reads zeros, never past the string.  Segment k decodes channels
 * [k*C/segs, (k+1)*C/segs) with the rows of `tables` that belong to them. */
int dsic_range_decode_seg(const uint8_t* in, int64_t stride, const int* lengths, int lstride,
                          int loff, const int* seg_lengths, int segs, const int* meta,
                          int meta_off, const uint16_t* tables, int Lmax, int B, int C, int HW,
                          int per_element, float* out_nchw, int* err, void* stream);

/* ---- whole-image codec (codec.py; no reference counterpart: its driver codes one
 * image of sizes that are multiples of 16 in one pass, eval_selfcontained_entropy.py:126-159) --
 * Tile grid of an H x W image and tiles th x tw (multiples of 16, >= 32, at most the padded
 * size): Hp = ceil16(H), tiles_y = ceil(Hp/th), origin of tile row i = min(i*th, Hp-th), tile
 * row i owns padded rows [i*th, min((i+1)*th, Hp)); columns likewise; tiles numbered row-major.
 * Padding to Hp x Wp reflects bottom/right as dsic_reflect_pad_br does (Hp-H < H, Wp-W < W).
 * Every call that takes a tile grid (gather, stitch, blend, the mask and validity calls, the
 * residual calls) refuses an image with a side over 2^30 pixels or whose padded size holds over
 * 2^31 - 1 blocks of 16 x 16 pixels (about 2^39 pixels): row, column and tile numbers are ints.
 * Below that, offsets into the image are 64-bit.
 * The calls handle tiles [first_tile, first_tile+n_tiles) of the grid.
 * gather: img uint8 [H][W][C] (C 3 or 4) -> tiles uint8 [n][th][tw][C], or img float32
 *   [C][H][W] -> tiles float32 [n][C][th][tw]; tiles 16-byte aligned.
 * stitch: decoded tiles float32 [n][C][th][tw] -> the pixels they own, cropped to H x W, into
 *   img float32 [C][H][W] as clamp(x,0,1), or img uint8 [H][W][C] as (uint8)(clamp(x,0,1)*255)
 *   (truncating, = torch x.clamp(0,1).mul(255).to(uint8)); img 16-byte aligned. */
int dsic_tile_gather_u8(const uint8_t* img_hwc, uint8_t* tiles, int H, int W, int C,
                        int th, int tw, int first_tile, int n_tiles, void* stream);
int dsic_tile_gather_f32(const float* img_chw, float* tiles, int H, int W, int C,
                         int th, int tw, int first_tile, int n_tiles, void* stream);
int dsic_tile_stitch_f32(const float* tiles, float* img_chw, int H, int W, int C,
                         int th, int tw, int first_tile, int n_tiles, void* stream);
int dsic_tile_stitch_u8(const float* tiles, uint8_t* img_hwc, int H, int W, int C,
                        int th, int tw, int first_tile, int n_tiles, void* stream);

/* The DSIC2 container of entropy.pack_container, written on the device from the outputs of
 * dsic_range_encode (bytes [B][cap_z+cap_y], lengths [B][2], meta [B][4] of
 * dsic_latent_support; err may be NULL): magic "DSIC2\0" | tag u32 | B,My,Hy,Wy,Nz,Hz,Wz u32 |
 * B x (min_y,max_y,min_z,max_z i32, len_z,len_y u32) | B x (z string, y string).
 * out holds at least 38 + 24*B + B*(cap_z+cap_y) bytes.  workspace: 2*B+3 int64; on
 * completion workspace[0] = container bytes, workspace[1] = *err (0 without err),
 * workspace[2..2+2B] = offsets of the strings after the records (exclusive scan). */
int dsic_container_pack(const uint8_t* bytes, int64_t cap_z, int64_t cap_y, const int* lengths,
                        const int* meta, const int* err, int B, uint32_t tag, int My, int Hy,
                        int Wy, int Nz, int Hz, int Wz, int64_t* workspace, uint8_t* out,
                        void* stream);
/* The DSIC3 container of segmented y strings, from the outputs of dsic_range_encode_seg_ws (bytes
 * [B][cap_z + segs*cap_seg], lengths [B][1 + segs]; segs 2, 4, 8 or 16): magic "DSIC3\0" | the DSIC2 fields |
 * segs u32 | B x the DSIC2 record (len_y = the sum of its segments) | B x segs u32 segment lengths |
 * B x (z string, segment 0 .. segs-1).  out holds at least 42 + (24 + 4*segs)*B + B*(cap_z + segs*cap_seg)
 * bytes; workspace: B*(1+segs)+3 int64, [0] and [1] as dsic_container_pack. */
int dsic_container_pack_seg(const uint8_t* bytes, int64_t cap_z, int64_t cap_seg, int segs,
                            const int* lengths, const int* meta, const int* err, int B,
                            uint32_t tag, int My, int Hy, int Wy, int Nz, int Hz, int Wz,
                            int64_t* workspace, uint8_t* out, void* stream);
/* Inverse for the decoder: a DSIC2 container of B images (blob_bytes bytes on the device) ->
 * z strings at zbuf + b*zstride, y strings at ybuf + b*ystride, lengths [B][2] (z, y) and
 * meta [B][4] (ymin, Ly, zmin, Lz) as dsic_range_decode takes them (lstride 2).  The caller has
 * checked the records on the host (max_len = the longest string, <= both strides); bytes past
 * a string's length in zbuf / ybuf are left as they are.  workspace: 2*B+3 int64. */
int dsic_container_scatter(const uint8_t* blob, int64_t blob_bytes, int B, int64_t max_len,
                           uint8_t* zbuf, int64_t zstride, uint8_t* ybuf, int64_t ystride,
                           int* lengths, int* meta, int64_t* workspace, void* stream);

/* ---- region decode (codec.decompress_region): a window of an image from only its tiles ----
 * The strings of n tiles picked from any containers of a stream, for one decode batch.  blob
 * (on the device, 16-byte aligned, its allocation a whole number of 16-byte chunks) holds the
 * selected byte spans back to back; desc is device int64 [n][4]: z offset, z length, y offset,
 * y length inside blob (any alignment).  String i goes to zbuf + i*zstride / ybuf + i*ystride
 * and lengths [n][2] (z, y) is written as dsic_range_decode takes it (lstride 2).  A length is
 * cut to its stride and to blob_bytes, and an offset outside the blob moves nothing, so a
 * forged descriptor cannot move a copy out of bounds.  max_len = the longest string;
 * n in 1..32767.  meta [n][4] comes from the host, which has the records. */
int dsic_strings_scatter_select(const uint8_t* blob, int64_t blob_bytes, const int64_t* desc,
                                int n, int64_t max_len, uint8_t* zbuf, int64_t zstride,
                                uint8_t* ybuf, int64_t ystride, int* lengths, void* stream);
/* Stitch into a window image.  tiles float32 [n][C][th][tw]; tile_ids device int32 [n], the
 * grid number of each (H, W, th, tw as for the calls above).  out is the window rows
 * [wy0, wy0+wh) x columns [wx0, wx0+ww) of the image as an image of its own: float32
 * [C][wh][ww] (C in 1..8) or uint8 [wh][ww][C] (C 3 or 4), 16-byte aligned.  Tile t writes the
 * pixels it owns that lie in the window, with the values of the whole-image stitch calls bit
 * for bit; every window pixel is written once when tile_ids holds every tile that meets the
 * window.  A number outside the grid, or a tile that does not meet the window, writes
 * nothing.  n in 1..65535. */
int dsic_tile_stitch_window_f32(const float* tiles, const int* tile_ids, int n, float* out,
                                int H, int W, int C, int th, int tw, int wy0, int wx0, int wh,
                                int ww, void* stream);
int dsic_tile_stitch_window_u8(const float* tiles, const int* tile_ids, int n, uint8_t* out,
                               int H, int W, int C, int th, int tw, int wy0, int wx0, int wh,
                               int ww, void* stream);

/* Overlapped tiles with blended seams (codec.tile_grid with overlap = O, a multiple of 16 with
 * O <= min(th, tw) / 2; O = 0 is the grid above).  On an axis of more than one tile the stride
 * is s = t - O, tiles = ceil((P - O) / s), nominal origin a(i) = i*s, real origin
 * min(i*s, P - t).  Tile i's support is [a(i), a(i+1) + O), the last one's [a(n-1), P); its
 * weight is (2k+1)/(2O) over the first O positions of the support (i > 0, k counted from a(i)),
 * (2(O-1-k)+1)/(2O) over [a(i+1), a(i+1) + O) (k counted from a(i+1)), 1 elsewhere in the
 * support and 0 outside it, so at most two tiles per axis weigh on a position and their
 * weights sum to 1.
 * gather_*_ov: the gather calls above on this grid; overlap = 0 gives their tiles bit for bit.
 * blend_window_f32: adds one decoded batch (tiles float32 [n][C][th][tw]; tile_ids device int32
 *   [n], strictly ascending, n in 1..64) into canvas, the float32 [C][wh][ww] image of the
 *   window rows [wy0, wy0+wh) x columns [wx0, wx0+ww), 16-byte aligned and zeroed by the caller
 *   before the first batch.  All float32, unfused: rcp = 1.0f / (float)(2 O), a ramp weight
 *   (float)(2k+1) * rcp, the weight of a tile w = wy * wx, its contribution w * clamp(x,0,1),
 *   and a pixel the left fold ((0 + c_a) + c_b) + ... over its contributing tiles in ascending
 *   number.  No atomics: a pixel is read, added to and stored by one thread per call, that of
 *   the lowest-numbered contributing tile in the call, and the partial sum travels in the
 *   canvas, so batches that arrive in ascending tile order give the same bits however the tiles
 *   are cut into batches.  A number outside the grid, or a tile that misses the window, adds
 *   nothing.
 * blend_finish_f32: canvas = min(canvas, 1) in place (the float32 weights of a pixel can sum to
 *   1 + 2 ulp).  blend_finish_u8: out uint8 [h][w][C] = (uint8)(min(canvas, 1) * 255),
 *   truncating, C 3 or 4, out 16-byte aligned. */
int dsic_tile_gather_u8_ov(const uint8_t* img_hwc, uint8_t* tiles, int H, int W, int C, int th,
                           int tw, int overlap, int first_tile, int n_tiles, void* stream);
int dsic_tile_gather_f32_ov(const float* img_chw, float* tiles, int H, int W, int C, int th,
                            int tw, int overlap, int first_tile, int n_tiles, void* stream);
int dsic_tile_blend_window_f32(const float* tiles, const int* tile_ids, int n, float* canvas,
                               int H, int W, int C, int th, int tw, int overlap, int wy0,
                               int wx0, int wh, int ww, void* stream);
int dsic_tile_blend_finish_f32(float* canvas, int C, int h, int w, void* stream);
int dsic_tile_blend_finish_u8(const float* canvas, uint8_t* out_hwc, int C, int h, int w,
                              void* stream);

/* ---- near-lossless residual layer (codec.compress_image with max_error = tau, 0..127) ----
 * Per tile, with x the gathered uint8 tile [th][tw][C] (C 3 or 4) and x_hat the encoder's
 * forward reconstruction float32 [C][th][tw]:
 *   p = (uint8)(clamp(x_hat,0,1)*255)  (float32, truncating: the uint8 stitch's value),
 *   r = x - p, s = 2 tau + 1, q = sign(r) * floor((|r| + tau) / s), |q| <= Q = (255 + tau) / s,
 *   q = 0 outside the rectangle the tile owns; the decoder writes clamp(p + q s, 0, 255), which
 *   lies within tau of x.  All integer.
 * residual_quantize_u8: tiles uint8 [n][th][tw][C], x_hat float32 [n][C][th][tw], own int32
 *   [n][4] = the owned rows [y0, y1) and columns [x0, x1) in tile coordinates -> q float32
 *   [n][C][th][tw] and hist int32 [n][C][512], to which the count of every pixel of the tile is
 *   ADDED at bin q + Q (the caller zeroes it).  tiles, x_hat, q 16-byte aligned; th, tw
 *   multiples of 16; n in 1..3000.
 * residual_tables: hist -> meta int32 [n][4] = (smin, L, 0, 1): the support [smin, smin + L) =
 *   min .. max of q over all channels of the tile in the y slots of the coder's meta, and the
 *   support of a one-symbol dummy string in the z slots; per (tile, channel) the table
 *   c[k] = floor(cum[k] * (65536 - L) / (th*tw)) + k, k < L (64-bit integers, cum the exclusive
 *   prefix sum of the channel's histogram over the support; c[L] = 65536 is implicit), entries
 *   k >= L written as 0, as compact uint16 [n][C][Lmax] and replicated to the 16 row bands of
 *   the channel in coder uint16 [n][C*16][Lmax]; both 16-byte aligned.  Lmax = ceil8(2 Q + 1).
 *   The q planes are coded by dsic_range_encode_seg_ws as its y family: M = C*16 channels of
 *   HWy = (th/16)*tw symbols, 16 segments, with a dummy z family of one symbol 0 (N = HWz = 1,
 *   a one-entry table 0) whose string is dropped.
 * residual_pack: the residual block of a batch from that call's outputs (bytes
 *   [n][cap_z + 16*cap_seg], lengths [n][17]; err may be NULL): "DSICR\0" | n, C, th, tw, tau,
 *   16 u32 | n x (smin i32, L u32, span_bytes u32) | n x 16 u32 segment lengths | per tile its
 *   span: C x L uint16 table entries, then the 16 segment strings.  out holds at least
 *   30 + 76*n + n*(2*C*Lmax + 16*cap_seg) bytes; workspace: (C+16)*n + 3 int64, [0] = block
 *   bytes, [1] = *err.
 * tile_stitch_window_u8_res: dsic_tile_stitch_window_u8 with q float32 [n][C][th][tw] (the decoded
 *   residual steps) added: a pixel is clamp(p + (int)q * (2 tau + 1), 0, 255). */
int dsic_residual_quantize_u8(const uint8_t* tiles, const float* x_hat, const int* own, int n,
                              int C, int th, int tw, int tau, float* q, int* hist, void* stream);
int dsic_residual_tables(const int* hist, int n, int C, int th, int tw, int tau, int Lmax,
                         int* meta, uint16_t* compact, uint16_t* coder, void* stream);
int dsic_residual_pack(const uint8_t* bytes, int64_t cap_z, int64_t cap_seg, const int* lengths,
                       const int* meta, const uint16_t* compact, const int* err, int n, int C,
                       int th, int tw, int tau, int Lmax, int64_t* workspace, uint8_t* out,
                       void* stream);
int dsic_tile_stitch_window_u8_res(const float* tiles, const float* q, int tau,
                                   const int* tile_ids, int n, uint8_t* out, int H, int W, int C,
                                   int th, int tw, int wy0, int wx0, int wh, int ww, void* stream);

/* ---- bounded-error residual layer for uint16 images (codec.compress_image with tolerance = tau,
 * 0..32767; stream version 9).  max_error above stays the uint8 mode; this is its uint16 sibling.
 * Per tile, with x the uint16 image [H][W][C] (C 1..4, any 2-byte alignment), the scale lohi (host,
 * 2*C words) and x_hat the encoder's forward reconstruction float32 [C][th][tw]:
 *   p = denorm(x_hat) = lo + (uint32)(clamp(x_hat,0,1)*(float)R + 0.5f)  (the uint16 stitch's value),
 *   r = x - p, s = 2 tau + 1, q = sign(r) * floor((|r| + tau) / s), |q| <= Q16 = (65535 + tau) / s,
 *   q = 0 outside the rectangle the tile owns; the decoder writes clamp(p + q s, 0, 65535), within
 *   tau of x.  Per tile q is split with m = max |q| and k the least shift with m <= 255 << k (0..9):
 *   hi = q >> k (arithmetic) in [-255, 255], lo = q & (2^k - 1).  hi is coded as the uint8 layer's q
 *   at tau = 0 (bin hi + 255 of 512, Lmax = 512, 16 row bands as 16 segments); lo travels raw as k
 *   bit planes of C*th*tw/8 bytes: bit b of byte i of plane j is bit j of lo of sample 8 i + b in
 *   [C][th][tw] order.  All integer.
 * residual_quantize_u16: tiles first_tile .. first_tile + n_tiles - 1 of the grid (H, W, th, tw),
 *   x_hat float32 [n][C][th][tw] -> q int32 [n][C][th][tw] and maxabs int32 [n], to which max |q| is
 *   applied by an integer atomic max (the caller zeroes it).  Only owned pixels are read.  x_hat, q
 *   16-byte aligned; n_tiles in 1..3000.
 * residual_split_u16: q, maxabs -> k int32 [n], hi float32 [n][C][th][tw] (clamped to +-255), hist
 *   int32 [n][C][512] (ADDED at bin hi + 255; the caller zeroes it) and planes uint64
 *   [n][9][C*th*tw/64], of which the first k[t] of tile t are written: word w of plane j is the
 *   64-bit ballot of bit j of lo over samples 64 w .. 64 w + 63.
 * residual_tables_u16: dsic_residual_tables at Q = 255 and Lmax = 512 for C 1..4: meta int32 [n][4]
 *   = (smin, L, 0, 1), compact uint16 [n][C][512], coder uint16 [n][C*16][512].
 * residual_pack_u16: the wide residual block of a batch: "DSICW\0" | n, C, th, tw, tau, 16 u32 |
 *   n x (smin i32, L u32, k u32, span_bytes u32) | n x 16 u32 segment lengths | per tile its span:
 *   C x L uint16 table entries, k planes, then the 16 segment strings (bytes, lengths, cap_z,
 *   cap_seg as dsic_residual_pack takes them).  out holds at least 30 + 80*n + n*(2*C*512 +
 *   9*C*th*tw/8 + 16*cap_seg) bytes; workspace: (C+17)*n + 3 int64, [0] = block bytes, [1] = *err.
 * residual_join_u16: hi float32 [n][C][th][tw] (decoded), blob the uploaded bytes (`total` of
 *   them) in which tile t's k[t] planes lie back to back from byte plane_off[t] (int64, any
 *   alignment; planes that would leave the blob read as 0; k clamped to 0..9) -> q float32
 *   [n][C][th][tw] = hi * 2^k + lo, clamped to +-Q16.  hi, q 16-byte aligned.
 * tile_stitch_window_u16_res: dsic_tile_stitch_window_u16 with q added: a value is
 *   clamp(denorm(x_hat) + (int)q * (2 tau + 1), 0, 65535).
 * DSIC_EINVAL: null pointers, C outside 1..4, tau outside 0..32767, n outside 1..3000, tile sides
 * that are no multiples of 16, misaligned buffers, a bad scale or grid. */
int dsic_residual_quantize_u16(const uint16_t* img_hwc, const float* x_hat, int H, int W, int C,
                               int th, int tw, const uint32_t* lohi, int tau, int first_tile,
                               int n_tiles, int* q, int* maxabs, void* stream);
int dsic_residual_split_u16(const int* q, const int* maxabs, int n, int C, int th, int tw,
                            float* hi, int* hist, int* k, uint64_t* planes, void* stream);
int dsic_residual_tables_u16(const int* hist, int n, int C, int th, int tw, int* meta,
                             uint16_t* compact, uint16_t* coder, void* stream);
int dsic_residual_pack_u16(const uint8_t* bytes, int64_t cap_z, int64_t cap_seg, const int* lengths,
                           const int* meta, const int* k, const uint16_t* compact,
                           const uint64_t* planes, const int* err, int n, int C, int th, int tw,
                           int tau, int64_t* workspace, uint8_t* out, void* stream);
int dsic_residual_join_u16(const float* hi, const uint8_t* blob, int64_t total,
                           const int64_t* plane_off, const int* k, int n, int C, int th, int tw,
                           int tau, float* q, void* stream);
int dsic_tile_stitch_window_u16_res(const float* tiles, const float* q, int tau,
                                    const int* tile_ids, int n_tiles, uint16_t* out, int H, int W,
                                    int C, int th, int tw, int wy0, int wx0, int wh, int ww,
                                    const uint32_t* lohi, void* stream);

/* ---- image overviews (codec.build_overviews, compress_image with overviews = n) ----
 * One level of the pyramid from the one before it: dst is H2 x W2, H2 = ceil(H/2), W2 = ceil(W/2),
 * and output pixel (y, x) is taken from source rows 2y and min(2y+1, H-1) and columns 2x and
 * min(2x+1, W-1): on an odd side the last row or column counts twice, and nothing outside
 * H x W is read.  With a = top-left, b = top-right, c = bottom-left, d = bottom-right:
 * halve_u8: uint8 [H][W][C] -> uint8 [H2][W2][C], (a + b + c + d + 2) >> 2 per channel.
 * halve_f32: float32 [C][H][W] -> float32 [C][H2][W2], ((a + b) + (c + d)) * 0.25f, unfused.
 * C, H, W >= 1; src and dst at any (element) alignment, and they must not overlap. */
int dsic_image_halve_u8(const uint8_t* src_hwc, uint8_t* dst_hwc, int H, int W, int C,
                        void* stream);
int dsic_image_halve_f32(const float* src_chw, float* dst_chw, int C, int H, int W,
                         void* stream);

/* ---- nodata masks (codec.compress_image with nodata = v, 0..255; stream version 5) ----
 * A pixel of a uint8 [H][W][C] image (C 3 or 4) is nodata iff all its C channels equal v.  Per
 * tile of the grid (th, tw multiples of 16, no overlap) the mask m is a bit plane in tile
 * coordinates: th*tw bits, row-major, bit y*tw + x in byte (y*tw + x) / 8, LSB first, held as
 * uint32 [th*tw/32]; the bit is 1 iff the pixel is owned by the tile, inside H x W and nodata.
 * The delta plane is d[y][x] = m[y][x] ^ m[y-1][x], m[-1] = 0.  A payload is d in one of two
 * modes: 0 = the plane, th*tw/8 bytes; 1 = the positions y*tw + x of its set bits, ascending,
 * u16 little endian if th*tw <= 65536, else u32; mode 1 iff it is strictly shorter.
 * mask_classify_u8: counts int32 [n_tiles], to which the number of nodata pixels among the
 *   owned pixels inside H x W of tiles first_tile .. first_tile + n_tiles - 1 is ADDED (the
 *   caller zeroes it); n_tiles <= 65535 per call.  The image at any alignment.
 * mask_delta_planes_u8: tile_ids int32 [n] -> planes uint32 [n][th*tw/32] = the tiles' d
 *   planes, and popcounts int32 [n], to which their set bits are ADDED.  A number outside the
 *   grid gives the empty plane.
 * mask_pack: planes, popcounts, tile_ids [n] -> out = n x (tile u32, mode u32, bytes u32), then
 *   the n payloads back to back; out holds at least n * (12 + th*tw/8) bytes, 4-byte aligned.
 *   workspace: n + 2 int64, [0] = bytes written, [1] = 0.
 * mask_unpack: blob (the payloads, anywhere in it and at any alignment; readable in whole
 *   dwords) and desc int32 [n][3] = (mode, offset in blob, bytes) -> planes uint32
 *   [n][th*tw/32] = the m planes, 16-byte aligned.  Positions must ascend (the host checks);
 *   a payload that leaves the blob, or whose mode or length no tile can have, gives the empty
 *   plane, and a position >= th*tw sets nothing.
 * mask_apply_u8 / mask_apply_f32: desc int32 [n][2] = (tile, index into planes or -1 for "all
 *   set") -> v (uint8 [wh][ww][C]) or (float)v / 255.0f (float32 [C][wh][ww]) at those pixels
 *   of the window rows [wy0, wy0+wh) x columns [wx0, wx0+ww) that the tile owns and whose bit is
 *   set; nothing else is written, so set bits outside a tile's owned rectangle are harmless.
 *   A tile outside the grid, or a plane index >= n_planes, writes nothing.  out 16-byte aligned. */
int dsic_mask_classify_u8(const uint8_t* img_hwc, int H, int W, int C, int th, int tw, int nodata,
                          int first_tile, int n_tiles, int* counts, void* stream);
int dsic_mask_delta_planes_u8(const uint8_t* img_hwc, int H, int W, int C, int th, int tw,
                              int nodata, const int* tile_ids, int n, uint32_t* planes,
                              int* popcounts, void* stream);
int dsic_mask_pack(const uint32_t* planes, const int* popcounts, const int* tile_ids, int n,
                   int th, int tw, int64_t* workspace, uint8_t* out, void* stream);
int dsic_mask_unpack(const uint8_t* blob, int64_t blob_bytes, const int* desc, int n, int th,
                     int tw, uint32_t* planes, void* stream);
int dsic_mask_apply_u8(const uint32_t* planes, int n_planes, const int* desc, int n, int nodata,
                       uint8_t* out, int H, int W, int C, int th, int tw, int wy0, int wx0,
                       int wh, int ww, void* stream);
int dsic_mask_apply_f32(const uint32_t* planes, int n_planes, const int* desc, int n, int nodata,
                        float* out, int H, int W, int C, int th, int tw, int wy0, int wx0, int wh,
                        int ww, void* stream);

/* ---- 16-bit imagery (codec.compress_image of a uint16 [H][W][C] image; stream version 6) ----
 * Per band c the scale is a pair of integers lo_c <= hi_c in 0..65535, R = hi - lo.  Every call
 * that takes one reads it from the HOST pointer lohi: 2*C uint32 (lo0, hi0, lo1, hi1, ...),
 * copied by value into the kernel's arguments, hence 1 <= C <= 4.
 *   norm(v)   = R == 0 ? 0.0f : (float)(min(max(v, lo), hi) - lo) / (float)R   (one IEEE division)
 *   denorm(x) = lo + (uint32)(clamp(x, 0, 1) * (float)R + 0.5f)               (unfused; NaN -> lo)
 * denorm(norm(v)) == v for lo <= v <= hi, also with norm(v) one ulp off either way.
 * Images are uint16 at any 2-byte alignment; a row of W*C*2 bytes must not exceed 2^31 - 1.
 * band_range_u16: out_lohi_dev (DEVICE, uint32 [2*C]) = per band the minimum and maximum of the
 *   whole image; the call initialises it, and the result does not depend on the launch shape.
 * tile_gather_u16 / _ov: uint16 [H][W][C] -> float32 tiles [n][C][th][tw] = norm of the
 *   reflect-padded tiles, grid, padding and (first_tile, n_tiles) as tile_gather_f32 / _ov; the
 *   result is tile_gather_f32 of the float32 [C][H][W] image norm(img), bit for bit.
 * tile_stitch_window_u16: tiles float32 [n][C][th][tw] + tile_ids -> denorm into the uint16
 *   [wh][ww][C] window image, owned rectangles and window as tile_stitch_window_u8.
 * tile_blend_finish_u16: canvas float32 [C][h][w] (tile_blend_window_f32) -> denorm(min(v, 1))
 *   into uint16 [h][w][C].
 * image_halve_u16: uint16 [H][W][C] -> [ceil(H/2)][ceil(W/2)][C], (a + b + c + d + 2) >> 2 in 32
 *   bits, the last row or column of an odd side counted twice; src and dst must not overlap. */
int dsic_band_range_u16(const uint16_t* img_hwc, int H, int W, int C, uint32_t* out_lohi_dev,
                        void* stream);
int dsic_tile_gather_u16(const uint16_t* img_hwc, float* tiles, int H, int W, int C, int th,
                         int tw, const uint32_t* lohi, int first_tile, int n_tiles, void* stream);
int dsic_tile_gather_u16_ov(const uint16_t* img_hwc, float* tiles, int H, int W, int C, int th,
                            int tw, int overlap, const uint32_t* lohi, int first_tile, int n_tiles,
                            void* stream);
int dsic_tile_stitch_window_u16(const float* tiles, const int* tile_ids, int n_tiles,
                                uint16_t* out, int H, int W, int C, int th, int tw, int wy0,
                                int wx0, int wh, int ww, const uint32_t* lohi, void* stream);
int dsic_tile_blend_finish_u16(const float* canvas, uint16_t* out_hwc, int C, int h, int w,
                               const uint32_t* lohi, void* stream);
int dsic_image_halve_u16(const uint16_t* src_hwc, uint16_t* dst_hwc, int H, int W, int C,
                         void* stream);

/* ---- resampled reads (codec.ImageReader.read with size = (oh, ow)) ----
 * The level-0 region rows [y0, y0+h) x columns [x0, x0+w), resampled to oh x ow from a window of
 * overview level `shift` (0 = the image itself): src holds sh x sw pixels of that level, its first
 * pixel being the level's pixel (sy0, sx0), and must contain the region's covering window, rows
 * y0 >> shift ... (y0+h-1) >> shift and the columns likewise (codec.level_window).  src and dst
 * are uint8 / uint16 [.][.][C] or float32 [C][.][.].  All geometry is integer: on the row axis,
 * scaled by oh, output row i covers [i h, (i+1) h) and level row Y covers
 * [(Y << shift) oh - y0 oh, ((Y+1) << shift) oh - y0 oh); wy(i, Y) is the length they share
 * (summed over Y: h); columns likewise with ow, x0, w.
 * mode 0, average.  u8 / u16: S = sum wy wx v, T = sum wy wx in 64 bits, output
 *   (2 S + T) / (2 T), the exact weighted mean rounded half up.  f32: the float32 left fold over
 *   Y ascending, then X ascending, of (float)(wy wx) * v, unfused, divided by (float)T.
 *   nodata (u8 / u16: a pixel value, -1 = none; f32: the value, used if has_nodata != 0): a source
 *   pixel whose C channels all equal it stays out of S and T; T = 0 gives it in every channel.
 * mode 1, nearest: level row (y0 + (2 i + 1) h / (2 oh)) >> shift, columns likewise; copied, and
 *   nodata has no effect.
 * DSIC_EINVAL: null pointers; C outside 3..4 (u8), 1..4 (u16), 1..8 (f32); shift outside 0..15;
 * a region whose covering window leaves the source window; h w > 2^46; sizes under 1 or origins
 * under 0; u16 / f32 pointers not aligned to their element; src and dst overlapping. */
int dsic_window_resample_u8(const uint8_t* src_hwc, int sh, int sw, int sy0, int sx0, int C,
                            int shift, int y0, int x0, int h, int w, uint8_t* dst_hwc, int oh,
                            int ow, int mode, int nodata, void* stream);
int dsic_window_resample_u16(const uint16_t* src_hwc, int sh, int sw, int sy0, int sx0, int C,
                             int shift, int y0, int x0, int h, int w, uint16_t* dst_hwc, int oh,
                             int ow, int mode, int nodata, void* stream);
int dsic_window_resample_f32(const float* src_chw, int sh, int sw, int sy0, int sx0, int C,
                             int shift, int y0, int x0, int h, int w, float* dst_chw, int oh,
                             int ow, int mode, float nodata, int has_nodata, void* stream);

/* ---- validity masks (codec.compress_image with valid = mask, stream version 8) ----
 * A validity image is uint8 [H][W] at any address, 0 = invalid: a one-channel image whose "nodata
 * value" is 0.  The mask block, the planes, pack and unpack are those of the nodata masks above; a
 * set plane bit means the pixel is owned, inside the image and invalid.
 * dsic_valid_classify / dsic_valid_delta_planes: dsic_mask_classify_u8 / dsic_mask_delta_planes_u8
 *   on the validity image: per tile the invalid pixels among its owned pixels (counts is added
 *   to: zero it first), and the d planes and popcounts of the listed tiles, same grid, ownership
 *   and plane layout.
 * dsic_mask_apply_u16: dsic_mask_apply_u8 for a uint16 [wh][ww][C] window at any 2-byte alignment,
 *   C 1..4, fill 0..65535: fill at the set bits of the listed tiles (plane -1: over the whole
 *   owned rectangle) inside the window, nothing else.
 * dsic_mask_window_u8: the validity of a window, uint8 [wh][ww] at any address: every owned pixel
 *   of the listed tiles (desc as for apply) inside the window gets 0 where its bit is set and 1
 *   elsewhere; pixels of tiles that are not listed (full tiles) keep what the caller put there.
 * dsic_image_halve_valid_u8 / _u16: one overview level of a masked image, C 1..4.  The four taps
 *   of dsic_image_halve_u8 (a repeated tap counts twice); k = the valid taps, S = their sum per
 *   channel: the output is (2 S + k) / (2 k) (k = 4: (a + b + c + d + 2) >> 2) and is valid iff
 *   k > 0; for k = 0 it is the unmasked mean of the four taps.  dst_valid is uint8 [H2][W2] of 0
 *   and 1.  Outputs at any element alignment; src, src_valid, dst and dst_valid must not overlap.
 * dsic_band_range_valid_u16: dsic_band_range_u16 over the pixels whose validity byte is not 0; a
 *   band without a valid pixel gives (0, 0).  Atomic min and max: no dependence on any order.
 * dsic_window_resample_valid_u8 / _u16: dsic_window_resample_u8 / _u16 with a validity window
 *   src_valid [sh][sw] beside the source and an optional output validity dst_valid [oh][ow] (NULL:
 *   none).  A source pixel stays out of S and T iff its validity byte is 0 (no value is compared);
 *   T = 0 writes fill in every channel and validity 0, else validity 1.  Nearest copies the pixel
 *   and its validity (as 0 or 1).  Geometry, reduced weights and (2 S + T) / (2 T) are unchanged.
 * DSIC_EINVAL: as their siblings' (null pointers, C, the grid, more than 65535 tiles per call, a
 *   window outside the image, misaligned pointers, overlapping buffers) and a fill beyond the
 *   element type. */
int dsic_valid_classify(const uint8_t* valid_hw, int H, int W, int th, int tw, int first_tile,
                        int n_tiles, int* counts, void* stream);
int dsic_valid_delta_planes(const uint8_t* valid_hw, int H, int W, int th, int tw,
                            const int* tile_ids, int n_tiles, uint32_t* planes, int* popcounts,
                            void* stream);
int dsic_mask_apply_u16(const uint32_t* planes, int n_planes, const int* desc, int n, int fill,
                        uint16_t* out, int H, int W, int C, int th, int tw, int wy0, int wx0,
                        int wh, int ww, void* stream);
int dsic_mask_window_u8(const uint32_t* planes, int n_planes, const int* desc, int n,
                        uint8_t* out_hw, int H, int W, int th, int tw, int wy0, int wx0, int wh,
                        int ww, void* stream);
int dsic_image_halve_valid_u8(const uint8_t* src_hwc, const uint8_t* src_valid, uint8_t* dst_hwc,
                              uint8_t* dst_valid, int H, int W, int C, void* stream);
int dsic_image_halve_valid_u16(const uint16_t* src_hwc, const uint8_t* src_valid,
                               uint16_t* dst_hwc, uint8_t* dst_valid, int H, int W, int C,
                               void* stream);
int dsic_band_range_valid_u16(const uint16_t* img_hwc, const uint8_t* valid_hw, int H, int W,
                              int C, uint32_t* out_lohi_dev, void* stream);
int dsic_window_resample_valid_u8(const uint8_t* src_hwc, const uint8_t* src_valid, int sh, int sw,
                                  int sy0, int sx0, int C, int shift, int y0, int x0, int h,
                                  int w, uint8_t* dst_hwc, uint8_t* dst_valid, int oh, int ow,
                                  int mode, int fill, void* stream);
int dsic_window_resample_valid_u16(const uint16_t* src_hwc, const uint8_t* src_valid, int sh,
                                   int sw, int sy0, int sx0, int C, int shift, int y0, int x0,
                                   int h, int w, uint16_t* dst_hwc, uint8_t* dst_valid, int oh,
                                   int ow, int mode, int fill, void* stream);

/* ---- rendered views (codec.ImageReader.render, .histogram) ----
 * dsic_window_render_u8 / _u16: a display image of a resampled window in one launch.  Per output
 *   pixel first exactly what dsic_window_resample_u8 / _u16 compute for it (src_valid = NULL;
 *   nodata as there, -1 = none) or, with a validity window src_valid [sh][sw], what
 *   dsic_window_resample_valid_u8 / _u16 compute (nodata is ignored): same geometry, reduced
 *   weights, (2 S + T) / (2 T) and nearest rule; the resampled sample m stays in registers.
 *   Output band b then takes channel bands[b] of it, stretched with the pair (lo, hi) =
 *   lohi[2 bands[b]], lohi[2 bands[b] + 1]: R = hi - lo, d = min(max(m, lo), hi) - lo, the byte is
 *   R == 0 ? 0 : (510 d + R) / (2 R), which is 255 d / R rounded half up.  dst is uint8
 *   [oh][ow][nb + alpha].  With src_valid an output pixel with nothing valid under it (nearest:
 *   whose source pixel is invalid) gets background in every band and, for alpha = 1, alpha 0;
 *   every other pixel gets alpha 255.  Without src_valid every pixel is valid, and a nodata result
 *   (T = 0) is stretched like any value.  bands (nb ints) and lohi (2 C words) are host arrays,
 *   read before the call returns.
 *   DSIC_EINVAL, nothing written: what the resample calls refuse, with C 1..4 for both kinds; nb
 *   other than 1 or 3; a band outside 0..C-1; a pair that is not lo <= hi <= 255 (65535); alpha
 *   outside 0..1; background outside 0..255; dst overlapping src or src_valid.
 * dsic_band_histogram_u8 / _u16: hist [C][256] ([C][65536]) uint32 on the device; hist[c][v] += the
 *   number of counted pixels of img [H][W][C] whose channel c equals v.  valid_hw (NULL: none),
 *   uint8 [H][W], leaves out its zeros; nodata (-1: none) leaves out the pixels whose C channels
 *   all equal it.  The caller zeroes hist; several calls sum into it.  Integer atomic adds: no
 *   dependence on any order.  img at any element alignment, hist 4-byte aligned.
 *   DSIC_EINVAL: null img or hist; C outside 1..4; H or W under 1 or H W >= 2^32; nodata beyond the
 *   element type; hist overlapping img or valid_hw. */
int dsic_window_render_u8(const uint8_t* src_hwc, const uint8_t* src_valid, int sh, int sw, int sy0,
                          int sx0, int C, int shift, int y0, int x0, int h, int w,
                          const int* bands, int nb, const uint32_t* lohi, uint8_t* dst, int oh,
                          int ow, int mode, int nodata, int alpha, int background, void* stream);
int dsic_window_render_u16(const uint16_t* src_hwc, const uint8_t* src_valid, int sh, int sw,
                           int sy0, int sx0, int C, int shift, int y0, int x0, int h, int w,
                           const int* bands, int nb, const uint32_t* lohi, uint8_t* dst, int oh,
                           int ow, int mode, int nodata, int alpha, int background, void* stream);
int dsic_band_histogram_u8(const uint8_t* img_hwc, const uint8_t* valid_hw, int H, int W, int C,
                           int nodata, uint32_t* hist, void* stream);
int dsic_band_histogram_u16(const uint16_t* img_hwc, const uint8_t* valid_hw, int H, int W, int C,
                            int nodata, uint32_t* hist, void* stream);

/* ---- warped reads (codec.ImageReader.read_warped, .render_warped) ----
 * An affine view of level 0 (H x W), sampled from a window of overview level `shift` (LH x LW, LH =
 * ceil(H / 2^shift)): src holds sh x sw pixels of that level from its pixel (sy0, sx0), src_valid
 * (NULL: none) their validity bytes.  m: six int64 on the host, the 2 x 3 matrix in (row, column)
 * order in Q16, level-0 pixels per output pixel, read before the call returns.  All geometry is
 * integer: output pixel (i, j) of oh x ow samples the level-0 position P / 2^17,
 *   Py = m[0] (2 i + 1) + m[1] (2 j + 1) + 2 m[2],  Px = m[3] (2 i + 1) + m[4] (2 j + 1) + 2 m[5],
 * and is inside iff 0 <= Py < H 2^17 and 0 <= Px < W 2^17; an outside pixel is fill in every
 * channel and validity 0.  With q = P - 2^(16+shift), Y0 = q >> (17 + shift) and the phase p =
 * (q >> (10 + shift)) & 127, tap indices clamped to the level:
 * mode 1, nearest: pixel (min(Py >> (17 + shift), LH - 1), ...), a copy of pixel and validity.
 * mode 0, bilinear: taps Y0, Y0 + 1 with weights (128 - p, p) per axis; S = sum wy wx v and T =
 *   sum wy wx over the taps that count; (2 S + T) / (2 T); T = 0 gives fill and validity 0.
 * mode 2, cubic: Keys a = -1/2, taps Y0 - 1 ... Y0 + 2, per-axis weights scaled by 2^22:
 *   -p^3 + 256 p^2 - 16384 p, 3 p^3 - 640 p^2 + 2^22, -3 p^3 + 512 p^2 + 16384 p, p^3 - 128 p^2.
 *   If all 16 clamped taps count: clamp((S + 2^43) >> 44, 0, 255 or 65535), S in int64;
 *   otherwise the bilinear pixel.
 * A tap counts iff its validity byte is not 0 (src_valid; nodata is then ignored), else iff its C
 * channels do not all equal nodata (-1: none), else always.  dst_valid (NULL: none) is uint8
 * [oh][ow] of 0 and 1.
 * dsic_window_warp_render_u8 / _u16: the same sample, never stored, through the band choice,
 *   stretch, alpha and background of dsic_window_render_u8 / _u16; a pixel whose validity would
 *   be 0 gets background in every band and alpha 0.
 * DSIC_EINVAL, nothing written: null pointers; C outside 3..4 (u8), 1..4 (u16; render: 1..4 for
 *   both); mode outside 0..2; shift outside 0..15; LH or LW that is not the level's size; a source
 *   window outside the level; oh or ow outside 1..2^20; |m[0]|, |m[1]|, |m[3]|, |m[4]| over 2^26 or
 *   |m[2]|, |m[5]| >= 2^47; a source window that does not contain every tap of every inside sample
 *   (the range is exact at the four corner pixels, widened by the mode's taps and clamped to the
 *   level); nodata or fill beyond the element type; misaligned pointers; overlapping buffers; and
 *   what dsic_window_render_u8 refuses of its display arguments, in the same words and the same
 *   order (one check serves both, csrc/render.h). */
int dsic_window_warp_u8(const uint8_t* src_hwc, const uint8_t* src_valid, int sh, int sw, int sy0,
                        int sx0, int C, int shift, int LH, int LW, int H, int W, const int64_t* m,
                        uint8_t* dst_hwc, uint8_t* dst_valid, int oh, int ow, int mode, int nodata,
                        int fill, void* stream);
int dsic_window_warp_u16(const uint16_t* src_hwc, const uint8_t* src_valid, int sh, int sw,
                         int sy0, int sx0, int C, int shift, int LH, int LW, int H, int W,
                         const int64_t* m, uint16_t* dst_hwc, uint8_t* dst_valid, int oh, int ow,
                         int mode, int nodata, int fill, void* stream);
int dsic_window_warp_render_u8(const uint8_t* src_hwc, const uint8_t* src_valid, int sh, int sw,
                               int sy0, int sx0, int C, int shift, int LH, int LW, int H, int W,
                               const int64_t* m, const int* bands, int nb, const uint32_t* lohi,
                               uint8_t* dst, int oh, int ow, int mode, int nodata, int alpha,
                               int background, void* stream);
int dsic_window_warp_render_u16(const uint16_t* src_hwc, const uint8_t* src_valid, int sh, int sw,
                                int sy0, int sx0, int C, int shift, int LH, int LW, int H, int W,
                                const int64_t* m, const int* bands, int nb, const uint32_t* lohi,
                                uint8_t* dst, int oh, int ow, int mode, int nodata, int alpha,
                                int background, void* stream);

/* ---- index views (codec.ImageReader.render_index, .render_index_warped, .index_histogram) ----
 * An index is (kind, a, b): a and b are band numbers of the stream, b is ignored for a band.  It is
 * taken from the sample that the resample or warp call would write for the same request: resample
 * first, index after, as the render calls stretch that sample.  top is 255 or 65535, A the sample
 * of band a, B the sample of band b, s = A + B.  The index value v is kept as the unsigned
 * u = v - vmin:
 *
 *   kind                      u                       v = u + vmin              vmin .. vmax      defined
 *   DSIC_INDEX_BAND           A                       the sample itself         0 .. top          always
 *   DSIC_INDEX_DIFFERENCE     A - B + top             A - B                     -top .. top       always
 *   DSIC_INDEX_ND             (40000 A + s) / (2 s)   10000 (A - B) / (A + B)   -10000 .. 10000   s != 0
 *                             (unsigned 32-bit)       rounded half up
 *
 * 40000 * 65535 + 131070 < 2^32, so the normalised difference is one 32-bit unsigned division per
 * pixel; the scale 10000 is the customary integer NDVI.  A normalised difference with s = 0 is
 * invalid, exactly as a pixel with nothing valid under it: background, alpha 0, not counted.
 * The stretch pair (lo, hi) is given in v units, vmin <= lo <= hi <= vmax; the byte is k = the
 * stretch of the render calls applied to (u, lo - vmin, hi - vmin): 510 * 131070 + 131070 < 2^32.
 * Colour map: cmap_dev is uint8 [256][3] on the device and the output bands are cmap[k][0..2].
 * dst is uint8 [oh][ow][3 + alpha]; an invalid pixel gets background in the three bands and, for
 * alpha = 1, alpha 0; every other pixel gets alpha 255.
 * dsic_window_index_render_u8 / _u16: the geometry, src_valid, mode and nodata of
 *   dsic_window_render_u8 / _u16.  dsic_window_warp_index_render_u8 / _u16: those of
 *   dsic_window_warp_render_u8 / _u16.
 *   DSIC_EINVAL, nothing written: what the sibling refuses of geometry, pointers, overlap and
 *   alignment; kind outside the three; a band outside 0..C-1; a pair that is not vmin <= lo <= hi
 *   <= vmax; a null cmap_dev; cmap overlapping dst; alpha outside 0..1; background outside 0..255.
 * dsic_index_histogram_u8 / _u16: hist[u] += the number of counted pixels of img [H][W][C] whose
 *   index is u: 20001 uint32 on the device for DSIC_INDEX_ND, 2 top + 1 (511 or 131071) for
 *   DSIC_INDEX_DIFFERENCE.  Counted is what dsic_band_histogram_u8 / _u16 count, less the pixels of
 *   a normalised difference with s = 0.  The caller zeroes hist; several calls sum into it;
 *   integer atomic adds: no dependence on any order.
 *   DSIC_EINVAL: what dsic_band_histogram_u8 refuses; a band outside 0..C-1; a kind other than
 *   these two (DSIC_INDEX_BAND: dsic_band_histogram_u8 / _u16 count a band). */
#define DSIC_INDEX_BAND 0
#define DSIC_INDEX_DIFFERENCE 1
#define DSIC_INDEX_ND 2
int dsic_window_index_render_u8(const uint8_t* src_hwc, const uint8_t* src_valid, int sh, int sw,
                                int sy0, int sx0, int C, int shift, int y0, int x0, int h, int w,
                                int kind, int band_a, int band_b, int lo, int hi,
                                const uint8_t* cmap_dev, uint8_t* dst, int oh, int ow, int mode,
                                int nodata, int alpha, int background, void* stream);
int dsic_window_index_render_u16(const uint16_t* src_hwc, const uint8_t* src_valid, int sh, int sw,
                                 int sy0, int sx0, int C, int shift, int y0, int x0, int h, int w,
                                 int kind, int band_a, int band_b, int lo, int hi,
                                 const uint8_t* cmap_dev, uint8_t* dst, int oh, int ow, int mode,
                                 int nodata, int alpha, int background, void* stream);
int dsic_window_warp_index_render_u8(const uint8_t* src_hwc, const uint8_t* src_valid, int sh,
                                     int sw, int sy0, int sx0, int C, int shift, int LH, int LW,
                                     int H, int W, const int64_t* m, int kind, int band_a,
                                     int band_b, int lo, int hi, const uint8_t* cmap_dev,
                                     uint8_t* dst, int oh, int ow, int mode, int nodata, int alpha,
                                     int background, void* stream);
int dsic_window_warp_index_render_u16(const uint16_t* src_hwc, const uint8_t* src_valid, int sh,
                                      int sw, int sy0, int sx0, int C, int shift, int LH, int LW,
                                      int H, int W, const int64_t* m, int kind, int band_a,
                                      int band_b, int lo, int hi, const uint8_t* cmap_dev,
                                      uint8_t* dst, int oh, int ow, int mode, int nodata, int alpha,
                                      int background, void* stream);
int dsic_index_histogram_u8(const uint8_t* img_hwc, const uint8_t* valid_hw, int H, int W, int C,
                            int nodata, int kind, int band_a, int band_b, uint32_t* hist,
                            void* stream);
int dsic_index_histogram_u16(const uint16_t* img_hwc, const uint8_t* valid_hw, int H, int W, int C,
                             int nodata, int kind, int band_a, int band_b, uint32_t* hist,
                             void* stream);

/* ---- gridded reads (codec.ImageReader.read_gridded, .render_gridded, .render_index_gridded) ----
 * A reprojected view: the warp calls with the rule "where does output pixel (i, j) sample" given
 * by a coordinate mesh instead of a matrix.  step = S = 2^s is 16, 32 or 64; nh = ceil(oh / S), nw
 * = ceil(ow / S).  The mesh G is int64 [nh + 1][nw + 1][2]: node (a, b) holds the level-0 position
 * (y, x) in Q16 of the output corner (a S, b S), in the frame of the warp calls' matrix (pixel
 * (i, j) has its centre at (i + 1/2, j + 1/2)).  Every entry is under 2^48 in size, or a node has
 * DSIC_GRID_NONE = -2^63 in its y entry: no position here (its x entry is then not looked at).
 * With a = i >> s, b = j >> s, fu = 2 (i - a S) + 1, fv = 2 (j - b S) + 1, per axis
 *   P = ((2S - fu) (2S - fv) G[a][b] + (2S - fu) fv G[a][b+1] + fu (2S - fv) G[a+1][b]
 *        + fu fv G[a+1][b+1]) >> (2 s + 1)
 * (an arithmetic shift: a floor; the weights sum to 2^(2s+2) <= 2^14, the sum stays under 2^62) is
 * the position in Q17, and everything after it - the inside test, the level, the taps, the
 * weights, the masks, fill and validity - is what the warp calls state for their P.  Every pixel
 * of a cell with a none node is fill, validity 0.  For G[a][b] = m0 a S + m1 b S + m2 per axis, P
 * = m0 (2 i + 1) + m1 (2 j + 1) + 2 m2: on an affine mesh the result is the warp call's, bit for
 * bit, for every step and mode.
 * The mesh is given twice and the library still allocates nothing: mesh_host is what the call
 * checks before it returns, mesh_dev (the same values, uploaded by the caller, 8-byte aligned) is
 * what the kernel reads.  Taps are clamped to the source window as well as to the level, so a
 * device copy that differs cannot make the kernel read outside the source allocation.
 * The other arguments, the three kinds of call and their outputs are those of
 * dsic_window_warp_u8 / _u16, dsic_window_warp_render_u8 / _u16 and
 * dsic_window_warp_index_render_u8 / _u16.
 * DSIC_EINVAL, nothing written: what the warp sibling refuses, less its matrix; a step other than
 *   16, 32, 64; more than 2^22 nodes; an entry of 2^48 or more in size; a none mark in an x entry
 *   whose y entry holds a position; a source window that does not contain every tap the mesh can
 *   ask for: per axis the positions of a cell lie between the smallest and largest of its four
 *   nodes, so the box is the minimum and maximum over the nodes of all cells without a none node,
 *   doubled to Q17, cut to the image, widened by the mode's taps and clamped to the level (no such
 *   cell, or a box beside the image: any window will do); a mesh_dev that is misaligned or
 *   overlaps an output. */
#define DSIC_GRID_NONE INT64_MIN
int dsic_window_grid_u8(const uint8_t* src_hwc, const uint8_t* src_valid, int sh, int sw, int sy0,
                        int sx0, int C, int shift, int LH, int LW, int H, int W,
                        const int64_t* mesh_host, const int64_t* mesh_dev, int step,
                        uint8_t* dst_hwc, uint8_t* dst_valid, int oh, int ow, int mode, int nodata,
                        int fill, void* stream);
int dsic_window_grid_u16(const uint16_t* src_hwc, const uint8_t* src_valid, int sh, int sw,
                         int sy0, int sx0, int C, int shift, int LH, int LW, int H, int W,
                         const int64_t* mesh_host, const int64_t* mesh_dev, int step,
                         uint16_t* dst_hwc, uint8_t* dst_valid, int oh, int ow, int mode,
                         int nodata, int fill, void* stream);
int dsic_window_grid_render_u8(const uint8_t* src_hwc, const uint8_t* src_valid, int sh, int sw,
                               int sy0, int sx0, int C, int shift, int LH, int LW, int H, int W,
                               const int64_t* mesh_host, const int64_t* mesh_dev, int step,
                               const int* bands, int nb, const uint32_t* lohi, uint8_t* dst, int oh,
                               int ow, int mode, int nodata, int alpha, int background,
                               void* stream);
int dsic_window_grid_render_u16(const uint16_t* src_hwc, const uint8_t* src_valid, int sh, int sw,
                                int sy0, int sx0, int C, int shift, int LH, int LW, int H, int W,
                                const int64_t* mesh_host, const int64_t* mesh_dev, int step,
                                const int* bands, int nb, const uint32_t* lohi, uint8_t* dst,
                                int oh, int ow, int mode, int nodata, int alpha, int background,
                                void* stream);
int dsic_window_grid_index_render_u8(const uint8_t* src_hwc, const uint8_t* src_valid, int sh,
                                     int sw, int sy0, int sx0, int C, int shift, int LH, int LW,
                                     int H, int W, const int64_t* mesh_host,
                                     const int64_t* mesh_dev, int step, int kind, int band_a,
                                     int band_b, int lo, int hi, const uint8_t* cmap_dev,
                                     uint8_t* dst, int oh, int ow, int mode, int nodata, int alpha,
                                     int background, void* stream);
int dsic_window_grid_index_render_u16(const uint16_t* src_hwc, const uint8_t* src_valid, int sh,
                                      int sw, int sy0, int sx0, int C, int shift, int LH, int LW,
                                      int H, int W, const int64_t* mesh_host,
                                      const int64_t* mesh_dev, int step, int kind, int band_a,
                                      int band_b, int lo, int hi, const uint8_t* cmap_dev,
                                      uint8_t* dst, int oh, int ow, int mode, int nodata, int alpha,
                                      int background, void* stream);

/* ---- scene stacks (codec.SceneStack.read, .render): n placed windows into one ----
 * dsic_window_composite_u8 / _u16: a mosaic or a per-pixel composite of n source windows in one
 *   launch, without a workspace.  src, src_valid, rect and nodata are host arrays of n entries,
 *   read before the call returns.  src[i] is a dense device window [h_i][w_i][C]; src_valid[i] is
 *   NULL or uint8 [h_i][w_i], 0 = invalid; rect[4 i .. 4 i + 3] = (dy, dx, h, w) is where source i
 *   lies inside the oh x ow output: sources may overlap and may leave holes; nodata[i] is -1 for
 *   none, or a pixel value: a pixel of source i whose C channels all equal it is invalid.
 *   The candidates of output pixel p are the sources i, in list order, whose rect contains p,
 *   whose src_valid, if given, is not zero at p, and in which p is not nodata; k is their number.
 *
 *   mode                        result, all integer
 *   DSIC_COMPOSITE_FIRST   0    the pixel of the first candidate
 *   DSIC_COMPOSITE_LAST    1    the pixel of the last candidate
 *   DSIC_COMPOSITE_MEAN    2    per band (2 S + k) / (2 k), S the sum over the candidates: S / k
 *                               rounded half up; 2 * 16 * 65535 + 16 < 2^32
 *   DSIC_COMPOSITE_MEDIAN  3    per band, the bands on their own: of the candidates' values sorted
 *                               as v[0 .. k-1], v[(k - 1) / 2] for odd k and
 *                               (v[k / 2 - 1] + v[k / 2] + 1) >> 1 for even k
 *
 *   k = 0 gives fill in every band.  dst_hwc is [oh][ow][C]; dst_valid (NULL: not wanted), uint8
 *   [oh][ow], receives k > 0 as 1 or 0; dst_count (NULL: not wanted), uint8 [oh][ow], receives k.
 *   All buffers at any element alignment.  first and last read validity bytes (of a source with a
 *   nodata value: its pixels) up to the winner and the winner's pixel, and with dst_count the
 *   validity of the whole list; mean and median read every candidate's pixel.
 *   DSIC_EINVAL, nothing written: n outside 1..16; C outside 1..4; oh or ow under 1 or
 *   oh ow >= 2^31; a null array, a null src[i] or a null dst_hwc; a rect with h or w under 1 or not
 *   inside the output; mode outside 0..3; fill or a nodata[i] beyond the element type; an output
 *   overlapping an input or another output. */
#define DSIC_COMPOSITE_FIRST 0
#define DSIC_COMPOSITE_LAST 1
#define DSIC_COMPOSITE_MEAN 2
#define DSIC_COMPOSITE_MEDIAN 3
int dsic_window_composite_u8(const uint8_t* const* src, const uint8_t* const* src_valid,
                             const int* rect, const int* nodata, int n, int C, uint8_t* dst_hwc,
                             uint8_t* dst_valid, uint8_t* dst_count, int oh, int ow, int mode,
                             int fill, void* stream);
int dsic_window_composite_u16(const uint16_t* const* src, const uint8_t* const* src_valid,
                              const int* rect, const int* nodata, int n, int C, uint16_t* dst_hwc,
                              uint8_t* dst_valid, uint8_t* dst_count, int oh, int ow, int mode,
                              int fill, void* stream);

/* ---- best-pixel composites (codec.SceneStack.read with a ranked reduce, with_source=) ----
 * dsic_window_composite_pick_u8 / _u16: the whole pixel of one candidate per output pixel, and
 *   which source it came from.  src, src_valid, rect, nodata, n, C, dst_hwc, dst_valid, dst_count,
 *   oh, ow and fill are those of dsic_window_composite_u8 / _u16, and so are the candidates: the
 *   sources i, in list order, whose rect contains p, whose src_valid, if given, is not zero at p,
 *   and in which p is not nodata.  (kind, a, b) is an index of the table of the index views above,
 *   with top = 255 or 65535: u = its unsigned value of the candidate's samples A of band a and B
 *   of band b.  For the two ranked modes a candidate must also have a defined index: a
 *   DSIC_INDEX_ND candidate with A + B = 0 is not a candidate.  k is the number of candidates.
 *
 *   mode                        result: all C bands of one candidate
 *   DSIC_COMPOSITE_FIRST   0    the first candidate
 *   DSIC_COMPOSITE_LAST    1    the last candidate
 *   DSIC_COMPOSITE_MAX     4    the candidate with the largest u
 *   DSIC_COMPOSITE_MIN     5    the candidate with the smallest u
 *                               ties, in both: the candidate that comes first in list order
 *
 *   k = 0 gives fill in every band.  dst_valid receives k > 0, dst_count k, as above.  dst_source
 *   (NULL: not wanted), uint8 [oh][ow], receives the id of the winning source and 255 where k = 0.
 *   id is NULL, then the id of source i is i, or a host array of n values in 0..254, read before
 *   the call returns.  kind, a and b are ignored for first and last.  Everything is integer: u is
 *   at most 131070, the ranking is one unsigned comparison per candidate, nothing is divided
 *   beyond the one division of a normalised difference.  One launch, no workspace; all buffers at
 *   any element alignment.  max and min read every source's validity and bands a and b of every
 *   candidate, and the winner's pixel.  first and last without id and dst_source write the bytes
 *   of dsic_window_composite_u8 / _u16.
 *   DSIC_EINVAL, nothing written: what dsic_window_composite_u8 / _u16 refuse, with mode outside
 *   {0, 1, 4, 5}; for max and min a kind outside the three or a band outside 0..C-1; an id outside
 *   0..254; dst_source overlapping an input or another output. */
#define DSIC_COMPOSITE_MAX 4
#define DSIC_COMPOSITE_MIN 5
int dsic_window_composite_pick_u8(const uint8_t* const* src, const uint8_t* const* src_valid,
                                  const int* rect, const int* nodata, const int* id, int n, int C,
                                  uint8_t* dst_hwc, uint8_t* dst_valid, uint8_t* dst_count,
                                  uint8_t* dst_source, int oh, int ow, int mode, int kind, int a,
                                  int b, int fill, void* stream);
int dsic_window_composite_pick_u16(const uint16_t* const* src, const uint8_t* const* src_valid,
                                   const int* rect, const int* nodata, const int* id, int n, int C,
                                   uint16_t* dst_hwc, uint8_t* dst_valid, uint8_t* dst_count,
                                   uint8_t* dst_source, int oh, int ow, int mode, int kind, int a,
                                   int b, int fill, void* stream);

/* ---- warped scene stacks (codec.SceneStack.read_warped, .render_warped, .render_index_warped) ----
 * dsic_window_warp_composite_u8 / _u16: n scenes, 1..16, each under its own affine, sampled and
 *   combined per output pixel in one launch, without a workspace and without an intermediate in
 *   memory.  sources is a host array of n dsic_warp_source structs, read before the call returns
 *   (one struct per source rather than parallel arrays: one ctypes.Structure on the Python side).
 *   A source carries what dsic_window_warp_u8 / _u16 take for one scene: src (a device window
 *   [sh][sw][C] of the export's element type), src_valid (NULL: none), sh, sw, sy0, sx0, shift, LH,
 *   LW, H, W and its own Q16 matrix m[6] (output pixel -> that scene's level-0 position); nodata
 *   (-1: none); the id (0..254) that dst_source names it by; reserved is 0.  Shared: C, oh, ow,
 *   fill, sample_mode (0 bilinear, 1 nearest, 2 cubic, as the warp calls number their mode),
 *   reduce_mode (DSIC_COMPOSITE_FIRST, _LAST, _MEAN, _MEDIAN, _MAX or _MIN) and (kind, a, b), the
 *   index of the two ranked modes (ignored for the others).  Outputs: dst_hwc [oh][ow][C] and the
 *   optional uint8 planes dst_valid, dst_count and dst_source [oh][ow] (NULL: not wanted).
 *
 *   The result is defined as the chain of the exports above, bit for bit:
 *   1. for each source i, dsic_window_warp_u8 / _u16 with that source's arguments, mode =
 *      sample_mode, any fill and a dst_valid gives an oh x ow image S_i and its validity V_i;
 *   2. dsic_window_composite_u8 / _u16 (first, last, mean, median) or
 *      dsic_window_composite_pick_u8 / _u16 (max, min, and any call with dst_source) over the n
 *      pairs (S_i, V_i), each with the rect (0, 0, oh, ow), nodata[i] and id[i], with mode =
 *      reduce_mode, (kind, a, b) and fill, gives dst_hwc, dst_valid, dst_count and dst_source.
 *   So a source with src_valid ignores its nodata value under the taps, as step 1 does, and a
 *   sampled pixel whose C channels all equal nodata is no candidate, as step 2 has it.  The
 *   candidate rule, the rounding of mean, the median of an even count, the index and its defined
 *   values, the first of ties, fill and source 255 where k = 0 are those stated for the composite
 *   and pick calls above.  All buffers at any element alignment.
 *   DSIC_EINVAL, nothing written, in the words of the calls of the chain where one applies: n
 *   outside 1..16; a null sources or dst_hwc; C outside 3..4 (u8), 1..4 (u16); sample_mode outside
 *   0..2; oh or ow outside 1..2^20 or oh ow >= 2^31; reduce_mode outside 0..5; for max and min a
 *   kind outside the three or a band outside 0..C-1; dst_source with mean or median; fill beyond
 *   the element type; misaligned dst_hwc; outputs that overlap; then per source, named by its
 *   number: a null src; what the warp calls refuse of shift, H, W, LH, LW, the source window, the
 *   matrix and the taps; a nodata beyond the element type; an id outside 0..254; a misaligned src;
 *   a src or src_valid overlapping an output. */
typedef struct dsic_warp_source {
  const void* src;
  const uint8_t* src_valid;
  int sh, sw, sy0, sx0, shift, LH, LW, H, W;
  int nodata, id, reserved;
  int64_t m[6];
} dsic_warp_source;
int dsic_window_warp_composite_u8(const dsic_warp_source* sources, int n, int C, uint8_t* dst_hwc,
                                  uint8_t* dst_valid, uint8_t* dst_count, uint8_t* dst_source,
                                  int oh, int ow, int sample_mode, int reduce_mode, int kind, int a,
                                  int b, int fill, void* stream);
int dsic_window_warp_composite_u16(const dsic_warp_source* sources, int n, int C, uint16_t* dst_hwc,
                                   uint8_t* dst_valid, uint8_t* dst_count, uint8_t* dst_source,
                                   int oh, int ow, int sample_mode, int reduce_mode, int kind,
                                   int a, int b, int fill, void* stream);

/* ---- zonal statistics (codec.ImageReader.zonal_stats, codec.SceneStack.zonal_stats) ----
 * Per zone of a zone raster, the moments and extremes of the bands or of an index.  Integer and
 * bit for bit.  img [H][W][C] is uint8 or uint16, C in 1..4; valid_hw (NULL: none), uint8 [H][W],
 * leaves out its zeros; nodata (-1: none) leaves out the pixels whose C channels all equal it, as
 * dsic_band_histogram_u8 / _u16 count.  zones_hw is uint16 [H][W] and Z, 1..65535, the number of
 * zones: pixel p belongs to zone z = zones[p] iff z < Z.  Every other id belongs to no zone and is
 * ignored, 65535 being the customary "none"; an id at or above Z never produces a write.
 * what says which values v a pixel has:
 *   DSIC_ZONAL_BANDS (-1): every band, K = C values, v = px[k], u = v; band_a, band_b are ignored.
 *   DSIC_INDEX_BAND / _DIFFERENCE / _ND of bands a, b: K = 1 value, v = u + vmin with u and vmin
 *     of the index table above: px[a], px[a] - px[b], or the normalised difference in units of
 *     1 / 10000 rounded half up.  A pixel whose index is not defined (A + B = 0) is left out, as
 *     dsic_index_histogram_u8 / _u16 leave it out.
 * stats is [Z][K][5] 64-bit words on the device, and the call accumulates into it, per zone z and
 * value k over the counted pixels of the zone:
 *   [0] += their number (unsigned)          [3] = min([3], their least v)    (signed)
 *   [1] += the sum of v (signed)            [4] = max([4], their largest v)  (signed)
 *   [2] += the sum of v^2 (unsigned; |v| <= 65535 and H W < 2^32, so it fits: the moments are
 *          taken of v, not of u)
 *   The caller sets words 0..2 to 0, word 3 to INT64_MAX and word 4 to INT64_MIN before the first
 *   call; several calls (the strips of a window) accumulate into one table on the device.  Integer
 *   atomic adds, minima and maxima: no dependence on any order.  A zone without a counted pixel
 *   keeps its words.
 * hist (NULL: none) is uint32 [Z][K][256] on the device, zeroed by the caller, and lohi, given
 *   exactly when hist is, 2 K words on the host read before the call returns: per value k the pair
 *   (lo, hi) in u units.  hist[z][k][stretch(u, lo, hi)] += 1 per counted pixel, stretch the byte
 *   of the render calls (255 (clamp(u) - lo) / (hi - lo) rounded half up).  A uint8 band with
 *   (0, 255) has its exact per-zone histogram; anything wider has 256 equal steps from lo to hi.
 * A table of at most DSIC_ZONAL_LDS_BYTES (Z K 40 bytes) is gathered in LDS per workgroup and
 *   flushed once; a larger one takes the 64-bit atomics in global memory.  Same results.
 * DSIC_EINVAL, nothing written: a null img, zones or stats; C outside 1..4; H or W under 1 or
 *   H W >= 2^32; Z outside 1..65535; what outside -1..2; a band outside 0..C-1; nodata beyond
 *   the element type; img not aligned to its element, zones to 2, stats to 8, hist or lohi to 4
 *   bytes; lohi without hist or hist without lohi; a pair that is not 0 <= lo <= hi <= vmax -
 *   vmin (top for the bands); stats or hist overlapping img, valid_hw or zones_hw, or each
 *   other. */
#define DSIC_ZONAL_BANDS (-1)
#define DSIC_ZONAL_LDS_BYTES 40960
int dsic_zonal_stats_u8(const uint8_t* img_hwc, const uint8_t* valid_hw, const uint16_t* zones_hw,
                        int H, int W, int C, int nodata, int what, int band_a, int band_b, int Z,
                        uint64_t* stats, const uint32_t* lohi, uint32_t* hist, void* stream);
int dsic_zonal_stats_u16(const uint16_t* img_hwc, const uint8_t* valid_hw,
                         const uint16_t* zones_hw, int H, int W, int C, int nodata, int what,
                         int band_a, int band_b, int Z, uint64_t* stats, const uint32_t* lohi,
                         uint32_t* hist, void* stream);

/* HIP stream limited to the CUs whose bit is set in mask_host[words] (bit i of
 * word i/32 = CU i).  Used to give the range coder its own few CUs beside the
 * conv kernels; there is no reference counterpart (the reference is
 * single-stream).  The caller destroys the stream. */
int dsic_stream_create_masked(const uint32_t* mask_host, int words,
                              void** stream_out);
int dsic_stream_destroy(void* stream);

/* The table math evaluated on the HOST (no GPU needed): lets CPU-only tests
 * compare it bit for bit with the oracle and with the reference-generated
 * fixture tests/golden/entropy_ref.npz.
 * dsic_host_gaussian_cdf_f32: eval_selfcontained_entropy.py:14-15 in float32.
 * dsic_host_pmf_to_uint16_cdf: :17-23; pmf_host [L][C] float32 (support axis
 *   first), out_host [L+1][C] uint16.
 * dsic_host_cdf_table: one coder table (:41-47 or :54-61 + spreading);
 *   out_host: L uint16; raw_host: NULL or L+1 uint16 = the pre-spreading cdf of :22. */
double dsic_host_normal_cdf(double x);
double dsic_host_student_t_cdf(double t, double nu);
float dsic_host_gaussian_cdf_f32(float x);
/* sigma_z = exp(z_prior.log_sigma) (:32) as float32(exp64(x)): one value for encoder and
 * decoder on any machine (torch's expf differs between its CPU and GPU builds). */
float dsic_host_exp_f32(float x);
int dsic_host_pmf_to_uint16_cdf(const float* pmf_host, int L, int C,
                                uint16_t* out_host);
int dsic_host_cdf_table(int student, float sigma, float nu, int smin, int L,
                        uint16_t* out_host, uint16_t* raw_host);

#ifdef __cplusplus
}
#endif
#endif /* DSIC_HIP_H */
