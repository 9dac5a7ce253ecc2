// Near-lossless residual layer of the whole-image codec (codec.py, max_error = tau): per tile, the integer
// difference between the gathered uint8 tile x and the uint8 image p of the encoder's own x_hat, quantized with step
// s = 2 tau + 1, coded with one static table per (tile, colour channel) by the range coder of entropy.hip.
//
//   p = (uint8)(clamp(x_hat, 0, 1) * 255)      float32, truncating: what stitch_hwc_kernel writes
//   r = x - p,  q = sign(r) * floor((|r| + tau) / s),  |q| <= Q = floor((255 + tau) / s)
//   q = 0 at every pixel the tile does not own (the decoder never writes it)
//   decoder: x' = clamp(p + q s, 0, 255), |x' - x| <= tau           (image_codec.hip stitch_hwc_kernel<uint8_t, true>)
//
// The q plane of a tile, float32 [C][th][tw], is read by the coder as the latent [C 16][(th / 16) tw]: 16 row bands
// per colour plane, coded as 16 segments.  Everything here is integer arithmetic or byte movement; the kernels are
// memory-bound and move 16 bytes per lane where the layout allows.
#include "residual_block.h"

namespace dsic {

constexpr int kResRows = 16;     // rows of one tile per quantize workgroup (th is a multiple of 16)
constexpr int kResBins = 512;    // histogram bins per (tile, channel): bin q + Q, 2 Q + 1 <= 511 of them used

__host__ __device__ inline int res_Q(int tau) { return (255 + tau) / (2 * tau + 1); }
__host__ __device__ inline int res_lmax(int tau) { return (2 * res_Q(tau) + 1 + 7) / 8 * 8; }

// one of the 4 pixels of a lane: r = x - p -> q
__device__ __forceinline__ int quantize_one(int x, float x_hat, int tau, int s) {
  const int p = (int)(uint8_t)(clamp01(x_hat) * 255.0f);
  const int r = x - p, a = r < 0 ? -r : r;
  const int qa = (a + tau) / s;
  return r < 0 ? -qa : qa;
}

// tiles uint8 [n][th][tw][C], x_hat float32 [n][C][th][tw], own int32 [n][4] = rows [y0, y1) x columns [x0, x1) of
// the tile that it owns inside the image -> q float32 [n][C][th][tw], hist int32 [n][C][512] (+= at bin q + Q; every
// pixel of the tile is counted, the ones it does not own as q = 0).  A lane takes 4 pixels of a row: 4 C bytes of x
// (one dwordx4 for C = 4, three dwords for C = 3), a float4 of x_hat and of q per channel.  The histogram is kept in
// LDS per workgroup and flushed with one global atomic per non-empty bin: integer sums, so no order shows.
template <int C>
__global__ __launch_bounds__(256) void residual_quantize_kernel(const uint8_t* __restrict__ tiles,
                                                                const float* __restrict__ x_hat,
                                                                const int* __restrict__ own, int th, int tw, int tau,
                                                                float* __restrict__ q, int* __restrict__ hist) {
  __shared__ int lh[C * kResBins];
  const int t = blockIdx.y, r0 = blockIdx.x * kResRows;
  for (int i = threadIdx.x; i < C * kResBins; i += blockDim.x) lh[i] = 0;
  __syncthreads();
  const int s = 2 * tau + 1, Q = res_Q(tau);
  const int oy0 = own[4 * t], oy1 = own[4 * t + 1], ox0 = own[4 * t + 2], ox1 = own[4 * t + 3];
  const size_t cplane = (size_t)th * tw;
  const uint8_t* xt = tiles + (size_t)t * cplane * C;
  const float* ht = x_hat + (size_t)t * C * cplane;
  float* qt = q + (size_t)t * C * cplane;
  const int cpr = tw >> 2;  // 4-pixel chunks per row
  for (int i = threadIdx.x; i < kResRows * cpr; i += blockDim.x) {
    const int r = i / cpr, x0 = (i - r * cpr) << 2;
    const int y = r0 + r;
    const size_t e = (size_t)y * tw + x0;
    uint32_t xw[4] = {0u, 0u, 0u, 0u};  // the 4 C bytes of x, pixel-major
    if constexpr (C == 4) {
      const uint4 v = *(const uint4*)(xt + e * 4);
      xw[0] = v.x, xw[1] = v.y, xw[2] = v.z, xw[3] = v.w;
    } else {
      const uint32_t* w = (const uint32_t*)(xt + e * 3);
      xw[0] = w[0], xw[1] = w[1], xw[2] = w[2];
    }
    const bool row_owned = y >= oy0 && y < oy1;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float4 h = *(const float4*)(ht + c * cplane + e);
      const float hv[4] = {h.x, h.y, h.z, h.w};
      int qv[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int byte = k * C + c;
        const int x = (int)((xw[byte >> 2] >> (8 * (byte & 3))) & 0xFFu);
        const bool owned = row_owned && x0 + k >= ox0 && x0 + k < ox1;
        qv[k] = owned ? quantize_one(x, hv[k], tau, s) : 0;
      }
      *(float4*)(qt + c * cplane + e) = make_float4((float)qv[0], (float)qv[1], (float)qv[2], (float)qv[3]);
      // equal neighbours (flat areas, the pixels outside the owned rectangle) share one LDS atomic
      int run = 1;
#pragma unroll
      for (int k = 1; k <= 4; ++k) {
        if (k < 4 && qv[k] == qv[k - 1]) {
          ++run;
        } else {
          atomicAdd(&lh[c * kResBins + qv[k - 1] + Q], run);
          run = 1;
        }
      }
    }
  }
  __syncthreads();
  int* ghist = hist + (size_t)t * C * kResBins;
  for (int i = threadIdx.x; i < C * kResBins; i += blockDim.x) {
    const int v = lh[i];
    if (v) atomicAdd(ghist + i, v);
  }
}

// One wave per (tile, channel): blockIdx.x = channel, blockIdx.y = tile.  hist [n][C][512] -> the tile's support
// [smin, smin + L) = min .. max of q over all its channels, meta [n][4] = (smin, L, 0, 1) (the residual in the y
// slots; the z slots describe the one-symbol dummy string of the encode call), and the channel's table
//   c[k] = floor(cum[k] (65536 - L) / npix) + k,  k < L     (64-bit; cum the exclusive prefix sum of the histogram)
// as compact uint16 [n][C][Lmax] for the stream and replicated to the channel's 16 band rows of the coder table
// [n][C 16][Lmax].  Entries k >= L are written as 0.  Lane l holds entries 8 l .. 8 l + 7: one 16-byte store a row.
__global__ __launch_bounds__(64) void residual_tables_kernel(const int* __restrict__ hist, int C, int npix, int tau,
                                                             int Lmax, int* __restrict__ meta,
                                                             uint16_t* __restrict__ compact,
                                                             uint16_t* __restrict__ coder) {
  const int lane = threadIdx.x, c = blockIdx.x, t = blockIdx.y;
  const int Q = res_Q(tau);
  const int* th = hist + (size_t)t * C * kResBins;
  int lo = kResBins, hi = -1;
  for (int i = lane; i < C * kResBins; i += 64) {
    if (th[i] != 0) {
      const int bin = i & (kResBins - 1);
      lo = min(lo, bin), hi = max(hi, bin);
    }
  }
  lo = wave_min(lo), hi = wave_max(hi);
  if (hi < lo) lo = hi = Q;       // an empty histogram (never from the quantize kernel): the one symbol 0
  hi = min(hi, lo + Lmax - 1);    // a histogram from elsewhere cannot widen the table past its row
  const int L = hi - lo + 1;
  if (c == 0 && lane == 0) {
    meta[4 * t] = lo - Q, meta[4 * t + 1] = L, meta[4 * t + 2] = 0, meta[4 * t + 3] = 1;
  }
  const int* ch = th + c * kResBins;
  int v[8], sum = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = 8 * lane + j;
    v[j] = k < L ? ch[lo + k] : 0;
    sum += v[j];
  }
  int incl = sum;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  long long cum = incl - sum;
  uint16_t e[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = 8 * lane + j;
    e[j] = k < L ? (uint16_t)(cum * (long long)(65536 - L) / (long long)npix + k) : (uint16_t)0;
    cum += v[j];
  }
  if (8 * lane < Lmax) {
    uint4 w;
    __builtin_memcpy(&w, e, 16);
    *(uint4*)(compact + ((size_t)t * C + c) * Lmax + 8 * lane) = w;
    uint16_t* rows = coder + ((size_t)t * C + c) * kResBands * Lmax + 8 * lane;
#pragma unroll
    for (int b = 0; b < kResBands; ++b) *(uint4*)(rows + (size_t)b * Lmax) = w;
  }
}

}  // namespace dsic

using namespace dsic;

#define DSIC_RES_SHAPE(what)                                                                                    \
  DSIC_REQUIRE(C == 3 || C == 4, what ": C=%d must be 3 or 4", C);                                              \
  DSIC_REQUIRE(tau >= 0 && tau <= 127, what ": tau=%d must be in 0..127", tau);                                 \
  DSIC_REQUIRE(n >= 1 && n <= 3000, what ": n=%d tiles per call (1..3000)", n)

extern "C" int dsic_residual_quantize_u8(const uint8_t* tiles, const float* x_hat, const int* own, int n, int C, int th,
                                         int tw, int tau, float* q, int* hist, void* stream) {
  DSIC_REQUIRE(tiles && x_hat && own && q && hist, "residual_quantize_u8: null pointer");
  DSIC_RES_SHAPE("residual_quantize_u8");
  DSIC_REQUIRE(th >= 16 && tw >= 16 && th % 16 == 0 && tw % 16 == 0,
               "residual_quantize_u8: tile %dx%d: sides must be multiples of 16 (th %% 16, tw %% 16)", th, tw);
  DSIC_REQUIRE((((uintptr_t)tiles | (uintptr_t)x_hat | (uintptr_t)q) & 15) == 0,
               "residual_quantize_u8: tiles, x_hat and q must be 16-byte aligned");
  const dim3 grid(th / kResRows, n);
  if (C == 3)
    hipLaunchKernelGGL(residual_quantize_kernel<3>, grid, dim3(256), 0, (hipStream_t)stream, tiles, x_hat, own, th, tw,
                       tau, q, hist);
  else
    hipLaunchKernelGGL(residual_quantize_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, tiles, x_hat, own, th, tw,
                       tau, q, hist);
  return check_launch("residual_quantize_u8");
}

extern "C" int dsic_residual_tables(const int* hist, int n, int C, int th, int tw, int tau, int Lmax, int* meta,
                                    uint16_t* compact, uint16_t* coder, void* stream) {
  DSIC_REQUIRE(hist && meta && compact && coder, "residual_tables: null pointer");
  DSIC_RES_SHAPE("residual_tables");
  DSIC_REQUIRE(th >= 16 && tw >= 16 && th % 16 == 0 && tw % 16 == 0 && (int64_t)th * tw < ((int64_t)1 << 30),
               "residual_tables: tile %dx%d: sides must be multiples of 16 (th %% 16)", th, tw);
  DSIC_REQUIRE(Lmax == res_lmax(tau), "residual_tables: Lmax=%d must be %d for tau=%d", Lmax, res_lmax(tau), tau);
  DSIC_REQUIRE((((uintptr_t)compact | (uintptr_t)coder) & 15) == 0,
               "residual_tables: compact and coder must be 16-byte aligned");
  hipLaunchKernelGGL(residual_tables_kernel, dim3(C, n), dim3(64), 0, (hipStream_t)stream, hist, C, th * tw, tau, Lmax,
                     meta, compact, coder);
  return check_launch("residual_tables");
}

// The tables of the wide residual's high part (residual_u16.hip): the same kernel at Q = 255, rows of res_lmax(0) =
// 512, for the 1 to 4 bands of a uint16 image.
extern "C" int dsic_residual_tables_u16(const int* hist, int n, int C, int th, int tw, int* meta, uint16_t* compact,
                                        uint16_t* coder, void* stream) {
  DSIC_REQUIRE(hist && meta && compact && coder, "residual_tables_u16: null pointer");
  DSIC_REQUIRE(C >= 1 && C <= 4, "residual_tables_u16: C=%d must be in 1..4", C);
  DSIC_REQUIRE(n >= 1 && n <= 3000, "residual_tables_u16: n=%d tiles per call (1..3000)", n);
  DSIC_REQUIRE(th >= 16 && tw >= 16 && th % 16 == 0 && tw % 16 == 0 && (int64_t)th * tw < ((int64_t)1 << 30),
               "residual_tables_u16: tile %dx%d: sides must be multiples of 16 (th %% 16)", th, tw);
  DSIC_REQUIRE(((uintptr_t)hist & 3) == 0 && ((uintptr_t)meta & 3) == 0 &&
                   (((uintptr_t)compact | (uintptr_t)coder) & 15) == 0,
               "residual_tables_u16: hist and meta must be 4-byte, compact and coder 16-byte aligned");
  hipLaunchKernelGGL(residual_tables_kernel, dim3(C, n), dim3(64), 0, (hipStream_t)stream, hist, C, th * tw, 0,
                     res_lmax(0), meta, compact, coder);
  return check_launch("residual_tables_u16");
}

extern "C" int dsic_residual_pack(const uint8_t* bytes, int64_t cap_z, int64_t cap_seg, const int* lengths,
                                  const int* meta, const uint16_t* compact, const int* err, int n, int C, int th, int tw,
                                  int tau, int Lmax, int64_t* workspace, uint8_t* out, void* stream) {
  DSIC_REQUIRE(bytes && lengths && meta && compact && workspace && out, "residual_pack: null pointer");
  DSIC_RES_SHAPE("residual_pack");
  DSIC_REQUIRE(th >= 16 && tw >= 16 && th % 16 == 0 && tw % 16 == 0,
               "residual_pack: tile %dx%d: sides must be multiples of 16 (th %% 16)", th, tw);
  DSIC_REQUIRE(Lmax == res_lmax(tau), "residual_pack: Lmax=%d must be %d for tau=%d", Lmax, res_lmax(tau), tau);
  DSIC_REQUIRE(cap_z > 0 && cap_seg > 0 && cap_z % 4 == 0 && cap_seg % 4 == 0,
               "residual_pack: bad capacities (cap_z=%lld cap_seg=%lld)", (long long)cap_z, (long long)cap_seg);
  DSIC_REQUIRE(((uintptr_t)bytes & 3) == 0 && ((uintptr_t)compact & 3) == 0,
               "residual_pack: bytes and compact must be 4-byte aligned");
  return launch_pack<NarrowBlock>("residual_pack(head)", "residual_pack(pieces)", bytes, cap_z, cap_seg, lengths, meta,
                                  nullptr, compact, nullptr, err, n, C, th, tw, tau, Lmax, cap_seg, workspace, out,
                                  (hipStream_t)stream);
}
