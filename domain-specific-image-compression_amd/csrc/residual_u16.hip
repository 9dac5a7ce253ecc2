// Bounded-error residual layer for uint16 imagery (codec.py, tolerance = tau, stream version 9): per tile, the integer
// difference between the uint16 image x and the uint16 image p of the encoder's own x_hat, quantized with step
// s = 2 tau + 1.
//
//   p = denorm(x_hat) = lo + (uint32)(clamp(x_hat, 0, 1) * (float)R + 0.5f)      what stitch_hwc_kernel writes
//   r = x - p,  q = sign(r) * floor((|r| + tau) / s),  |q| <= Q16 = floor((65535 + tau) / s)
//   q = 0 at every pixel the tile does not own
//   decoder: x' = clamp(p + q s, 0, 65535), |x' - x| <= tau                       (image_codec.hip stitch_hwc_kernel<uint16_t, true>)
//
// q has up to 131 071 values, far past the 511 symbols of the 16-bit coder tables, so it is split per tile: with
// m = max |q| over the tile and k the least shift with m <= 255 << k (0 .. 9),
//   hi = q >> k (arithmetic, floor) in [-255, 255],  lo = q & (2^k - 1),  q = hi 2^k + lo.
// hi goes through the uint8 layer's path as it is (residual.hip: histogram at bin hi + 255 of 512, one table per
// (tile, band), 16 row bands as 16 segments); lo travels raw as k bit planes of C th tw / 8 bytes, bit b of byte i of
// plane j being bit j of lo of sample 8 i + b in [C][th][tw] order: the 64-bit ballot of 64 consecutive samples,
// little endian.  Everything here is integer arithmetic or byte movement and memory-bound.
#include "residual_block.h"
#include "tile_grid.h"
#include "u16_scale.h"

namespace dsic {

constexpr int kW16Rows = 16;    // rows of one tile per workgroup (th is a multiple of 16)
constexpr int kW16Bins = 512;   // histogram bins per (tile, band): bin hi + 255
constexpr int kW16Top = 255;    // |hi| <= 255
constexpr int kW16Planes = WideBlock::slots;  // the largest shift: Q16(0) = 65535 <= 255 << 9

__host__ __device__ inline int w16_Q(int tau) { return (65535 + tau) / (2 * tau + 1); }
__host__ __device__ inline int w16_shift(int m) {
  int k = 0;
  while (k < kW16Planes && m > (kW16Top << k)) ++k;
  return k;
}
// img uint16 [H][W][C] at any 2-byte alignment, x_hat float32 [n][C][th][tw] of tiles first .. first + n - 1 of the
// grid -> q int32 [n][C][th][tw] and maxabs int32 [n] (max= |q|: an integer maximum, so no order shows; the caller
// zeroes it).  A lane takes 4 pixels of a tile row as the gather does, but reads only pixels the tile owns, which lie
// inside the image: a run of 4 owned pixels is one load_run, a run cut by the owned rectangle goes value by value,
// and a run outside it reads nothing and writes q = 0.
template <int C>
__global__ __launch_bounds__(256) void quantize_u16_kernel(const uint16_t* __restrict__ img,
                                                           const float* __restrict__ x_hat, Grid g, int first, Scale sc,
                                                           int tau, int* __restrict__ q, int* __restrict__ maxabs) {
  const Owned o = owned(g, first + blockIdx.y);
  const int r0 = blockIdx.x * kW16Rows, vpr = g.tw >> 2;
  const size_t cplane = (size_t)g.th * g.tw;
  const float* ht = x_hat + (size_t)blockIdx.y * C * cplane;
  int* qt = q + (size_t)blockIdx.y * C * cplane;
  const uint32_t s = 2 * tau + 1;
  int m = 0;
  for (int i = threadIdx.x; i < kW16Rows * vpr; i += blockDim.x) {
    const int r = i / vpr, j0 = (i - r * vpr) << 2;
    const int y = o.oy + r0 + r, x0 = o.ox + j0;
    const size_t e = (size_t)(r0 + r) * g.tw + j0;
    const int xa = max(x0, o.x0), xb = min(x0 + 4, o.x1);  // the owned columns of the run
    const bool any = y >= o.y0 && y < o.y1 && xa < xb;
    uint16_t v[4 * C];
#pragma unroll
    for (int k = 0; k < 4 * C; ++k) v[k] = 0;
    if (any) {
      const uint16_t* src = img + ((size_t)y * g.W + x0) * C;
      if (xb - xa == 4) {
        load_run<2 * C>(src, v);
      } else {
#pragma unroll
        for (int p = 0; p < 4; ++p)
          if (x0 + p >= xa && x0 + p < xb) {
#pragma unroll
            for (int c = 0; c < C; ++c) v[p * C + c] = src[p * C + c];
          }
      }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
      int qv[4] = {0, 0, 0, 0};
      if (any) {
        const float4 h = *(const float4*)(ht + c * cplane + e);
        const float hv[4] = {h.x, h.y, h.z, h.w};
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          if (x0 + p >= xa && x0 + p < xb) {
            const int d = (int)v[p * C + c] - (int)denorm_u16(hv[p], sc.lo[c], sc.R[c]);
            const int qa = (int)(((uint32_t)(d < 0 ? -d : d) + (uint32_t)tau) / s);
            qv[p] = d < 0 ? -qa : qa;
            m = max(m, qa);
          }
        }
      }
      *(int4*)(qt + c * cplane + e) = make_int4(qv[0], qv[1], qv[2], qv[3]);
    }
  }
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0 && m > 0) atomicMax(maxabs + blockIdx.y, m);
}

// q int32 [n][C][th][tw], maxabs int32 [n] -> kout int32 [n] = the tile's shift k = w16_shift(maxabs), hi float32
// [n][C][th][tw] (the coder's input; clamped to +-255, which changes nothing for an honest maxabs), hist int32
// [n][C][512] += at bin hi + 255 (LDS histogram, one global atomic per non-empty bin; the zeros of a wave, the
// common value and all there is outside the owned rectangle, are counted by one ballot), and the k low planes
// uint64 [n][9][C th tw / 64]: word w of plane j is the ballot of bit j of lo over samples 64 w .. 64 w + 63.  The
// ballot layout makes a lane one sample, so loads and stores are dwords here, consecutive over the wave; a workgroup
// takes 16 rows of every band, 16 tw samples that start at a multiple of 256, so every wave is whole.
__global__ __launch_bounds__(256) void split_u16_kernel(const int* __restrict__ q, const int* __restrict__ maxabs, int C,
                                                        int th, int tw, float* __restrict__ hi, int* __restrict__ hist,
                                                        int* __restrict__ kout,
                                                        unsigned long long* __restrict__ planes) {
  __shared__ int lh[4 * kW16Bins];
  const int t = blockIdx.y, r0 = blockIdx.x * kW16Rows, lane = threadIdx.x & 63;
  for (int i = threadIdx.x; i < C * kW16Bins; i += blockDim.x) lh[i] = 0;
  __syncthreads();
  const int k = w16_shift(maxabs[t]);
  if (blockIdx.x == 0 && threadIdx.x == 0) kout[t] = k;
  const size_t cplane = (size_t)th * tw, per = (size_t)C * cplane, wpp = per >> 6;
  const int* qt = q + (size_t)t * per;
  float* ht = hi + (size_t)t * per;
  unsigned long long* pt = planes + (size_t)t * kW16Planes * wpp;
  const int span = kW16Rows * tw, low = (1 << k) - 1;
  for (int c = 0; c < C; ++c) {
    const size_t base = c * cplane + (size_t)r0 * tw;
    for (int i = threadIdx.x; i < span; i += blockDim.x) {
      const size_t s = base + i;
      const int v = qt[s];
      const int h = min(max(v >> k, -kW16Top), kW16Top), lo = v & low;
      ht[s] = (float)h;
      const unsigned long long zeros = __ballot(h == 0);
      if (h != 0) atomicAdd(&lh[c * kW16Bins + h + kW16Top], 1);
      if (lane == 0 && zeros) atomicAdd(&lh[c * kW16Bins + kW16Top], __popcll(zeros));
      unsigned long long mine = 0;
      for (int j = 0; j < k; ++j) {
        const unsigned long long b = __ballot((lo >> j) & 1);
        if (lane == j) mine = b;
      }
      if (lane < k) pt[(size_t)lane * wpp + (s >> 6)] = mine;
    }
  }
  __syncthreads();
  int* ghist = hist + (size_t)t * C * kW16Bins;
  for (int i = threadIdx.x; i < C * kW16Bins; i += blockDim.x) {
    const int v = lh[i];
    if (v) atomicAdd(ghist + i, v);
  }
}

// hi float32 [n][C][th][tw] (the decoded high parts), the uploaded stream bytes `blob` of `total` bytes in which tile
// t's k[t] planes lie back to back from byte plane_off[t] (any alignment: read in place, a byte per lane and plane) ->
// q float32 [n][C][th][tw] = hi 2^k + lo, exact since |q| < 2^24, clamped to +-Q16: a forged record can join to 131 071,
// an encoder's own never passes Q16.  A lane takes 8 consecutive samples: two float4 in, one byte of each plane, two
// float4 out.  Planes that would leave the blob are read as 0.
__global__ __launch_bounds__(256) void join_u16_kernel(const float* __restrict__ hi, const uint8_t* __restrict__ blob,
                                                       int64_t total, const long long* __restrict__ plane_off,
                                                       const int* __restrict__ kk, int64_t pb, int Q16,
                                                       float* __restrict__ q) {
  const int t = blockIdx.y;
  const int k = tile_planes<WideBlock>(kk, t);
  const long long off = plane_off[t];
  const bool inside = off >= 0 && off + (long long)k * pb <= total;
  const float* ht = hi + (size_t)t * pb * 8;
  float* qt = q + (size_t)t * pb * 8;
  for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < pb; u += (int64_t)gridDim.x * blockDim.x) {
    const float4 a = *(const float4*)(ht + 8 * u), b = *(const float4*)(ht + 8 * u + 4);
    const float h[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    uint32_t lo[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (inside) {
      for (int j = 0; j < k; ++j) {
        const uint32_t byte = blob[off + (long long)j * pb + u];
#pragma unroll
        for (int e = 0; e < 8; ++e) lo[e] |= ((byte >> e) & 1u) << j;
      }
    }
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int hv = min(max((int)h[e], -kW16Top), kW16Top);
      const int v = hv * (1 << k) + (int)lo[e];
      o[e] = (float)min(max(v, -Q16), Q16);
    }
    *(float4*)(qt + 8 * u) = make_float4(o[0], o[1], o[2], o[3]);
    *(float4*)(qt + 8 * u + 4) = make_float4(o[4], o[5], o[6], o[7]);
  }
}

}  // namespace dsic

using namespace dsic;

#define DSIC_W16_SHAPE(what)                                                                                    \
  DSIC_REQUIRE(C >= 1 && C <= 4, what ": C=%d must be in 1..4", C);                                             \
  DSIC_REQUIRE(n >= 1 && n <= 3000, what ": n=%d tiles per call (1..3000)", n);                                 \
  DSIC_REQUIRE(th >= 16 && tw >= 16 && th % 16 == 0 && tw % 16 == 0 && (int64_t)th * tw < ((int64_t)1 << 26),   \
               what ": tile %dx%d: sides must be multiples of 16 (th %% 16, tw %% 16)", th, tw)
#define DSIC_W16_TAU(what) DSIC_REQUIRE(tau >= 0 && tau <= 32767, what ": tau=%d must be in 0..32767", tau)

extern "C" int dsic_residual_quantize_u16(const uint16_t* img_hwc, const float* x_hat, int H, int W, int C, int th,
                                          int tw, const uint32_t* lohi, int tau, int first_tile, int n_tiles, int* q,
                                          int* maxabs, void* stream) {
  DSIC_REQUIRE(img_hwc && x_hat && lohi && q && maxabs, "residual_quantize_u16: null pointer");
  DSIC_U16_COMMON("residual_quantize_u16", img_hwc);
  DSIC_W16_TAU("residual_quantize_u16");
  DSIC_U16_SCALE("residual_quantize_u16");
  DSIC_TILE_ARGS("residual_quantize_u16");
  DSIC_REQUIRE(n_tiles <= 3000, "residual_quantize_u16: n=%d tiles per call (1..3000)", n_tiles);
  DSIC_U16_ROW("residual_quantize_u16", W);
  DSIC_REQUIRE((((uintptr_t)x_hat | (uintptr_t)q) & 15) == 0 && ((uintptr_t)maxabs & 3) == 0,
               "residual_quantize_u16: x_hat and q must be 16-byte, maxabs 4-byte aligned");
  DSIC_U16_BY_C(quantize_u16_kernel, grid, dim3(256), 0, (hipStream_t)stream, img_hwc, x_hat, g, first_tile, sc, tau, q,
                maxabs);
  return check_launch("residual_quantize_u16");
}

extern "C" int dsic_residual_split_u16(const int* q, const int* maxabs, int n, int C, int th, int tw, float* hi,
                                       int* hist, int* k, uint64_t* planes, void* stream) {
  DSIC_REQUIRE(q && maxabs && hi && hist && k && planes, "residual_split_u16: null pointer");
  DSIC_W16_SHAPE("residual_split_u16");
  DSIC_REQUIRE((((uintptr_t)q | (uintptr_t)maxabs | (uintptr_t)hi | (uintptr_t)hist | (uintptr_t)k) & 3) == 0 &&
                   ((uintptr_t)planes & 7) == 0,
               "residual_split_u16: q, maxabs, hi, hist and k must be 4-byte, planes 8-byte aligned");
  hipLaunchKernelGGL(split_u16_kernel, dim3(th / kW16Rows, n), dim3(256), 0, (hipStream_t)stream, q, maxabs, C, th, tw,
                     hi, hist, k, (unsigned long long*)planes);
  return check_launch("residual_split_u16");
}

extern "C" int dsic_residual_pack_u16(const uint8_t* bytes, int64_t cap_z, int64_t cap_seg, const int* lengths,
                                      const int* meta, const int* k, const uint16_t* compact, const uint64_t* planes,
                                      const int* err, int n, int C, int th, int tw, int tau, int64_t* workspace,
                                      uint8_t* out, void* stream) {
  DSIC_REQUIRE(bytes && lengths && meta && k && compact && planes && workspace && out,
               "residual_pack_u16: null pointer");
  DSIC_W16_SHAPE("residual_pack_u16");
  DSIC_W16_TAU("residual_pack_u16");
  DSIC_REQUIRE(cap_z > 0 && cap_seg > 0 && cap_z % 4 == 0 && cap_seg % 4 == 0,
               "residual_pack_u16: bad capacities (cap_z=%lld cap_seg=%lld)", (long long)cap_z, (long long)cap_seg);
  DSIC_REQUIRE(((uintptr_t)bytes & 3) == 0 && ((uintptr_t)compact & 3) == 0 && ((uintptr_t)planes & 7) == 0 &&
                   ((uintptr_t)workspace & 7) == 0,
               "residual_pack_u16: bytes and compact must be 4-byte, planes and workspace 8-byte aligned");
  const int64_t longest = (int64_t)WideBlock::slots * C * th * tw / 8;
  return launch_pack<WideBlock>("residual_pack_u16(head)", "residual_pack_u16(pieces)", bytes, cap_z, cap_seg, lengths,
                                meta, k, compact, (const uint8_t*)planes, err, n, C, th, tw, tau, WideBlock::lmax,
                                cap_seg > longest ? cap_seg : longest, workspace, out, (hipStream_t)stream);
}

extern "C" int dsic_residual_join_u16(const float* hi, const uint8_t* blob, int64_t total, const int64_t* plane_off,
                                      const int* k, int n, int C, int th, int tw, int tau, float* q, void* stream) {
  DSIC_REQUIRE(hi && blob && plane_off && k && q, "residual_join_u16: null pointer");
  DSIC_W16_SHAPE("residual_join_u16");
  DSIC_W16_TAU("residual_join_u16");
  DSIC_REQUIRE(total >= 0, "residual_join_u16: total=%lld bytes", (long long)total);
  DSIC_REQUIRE((((uintptr_t)hi | (uintptr_t)q) & 15) == 0 && ((uintptr_t)plane_off & 7) == 0 && ((uintptr_t)k & 3) == 0,
               "residual_join_u16: hi and q must be 16-byte, plane_off 8-byte, k 4-byte aligned");
  const int64_t pb = (int64_t)C * th * tw / 8;
  const int64_t blocks = (pb + 255) / 256;
  hipLaunchKernelGGL(join_u16_kernel, dim3((unsigned)(blocks > 64 ? 64 : blocks), n), dim3(256), 0, (hipStream_t)stream,
                     hi, blob, total, (const long long*)plane_off, k, pb, w16_Q(tau), q);
  return check_launch("residual_join_u16");
}
