// Validity masks beside the image (codec.compress_image with valid = mask, stream version 8): the masked halving that
// the overview levels of a masked scene are defined by, and the band range over valid pixels only.  A validity image
// is uint8 [H][W], 0 = invalid.
//
// Masked halving.  dst is H2 x W2 with H2 = ceil(H/2), W2 = ceil(W/2); an output pixel takes the four taps of
// pyramid.hip: rows 2y and min(2y+1, H-1), columns 2x and min(2x+1, W-1), a repeated tap counting twice.  With k the
// number of valid taps and S the sum over them per channel the output is (2 S + k) / (2 k), the mean over the valid
// taps rounded half up ((a + b + c + d + 2) >> 2 for k = 4), and the output pixel is valid iff k > 0; for k = 0 the
// output is the unmasked mean of the four taps.  All in integers: nothing depends on any order.
//
// Byte movers as pyramid.hip's and image_u16.hip's.  Both outputs are flat arrays at any element alignment: a thread
// owns one aligned 16-byte chunk of the image or of the validity and stores it as a dwordx4; the ragged chunks at the
// ends are element stores.  A chunk that lies in one output row away from a repeated last column, and whose loads stay
// inside the source, reads its two source rows as three 16-byte loads each and their validity as two (load16_any: the
// sources are aligned as they happen to be); every other chunk goes element by element.
#include <limits.h>

#include "byte_movers.h"

namespace dsic {

struct HalveV {
  int H, W, H2, W2;
  __device__ __forceinline__ int below(int y) const { return min(2 * y + 1, H - 1); }
  __device__ __forceinline__ int right(int x) const { return min(2 * x + 1, W - 1); }
};

// the four taps' pixel numbers of output pixel (y, x)
__device__ __forceinline__ void halve_taps(const HalveV& g, int y, int x, int64_t* p) {
  const int64_t r0 = (int64_t)(2 * y) * g.W, r1 = (int64_t)g.below(y) * g.W;
  const int xa = 2 * x, xb = g.right(x);
  p[0] = r0 + xa, p[1] = r0 + xb, p[2] = r1 + xa, p[3] = r1 + xb;
}

template <typename T>
__device__ __forceinline__ T halve_valid_value(const T* __restrict__ src, const uint8_t* __restrict__ val,
                                               const HalveV& g, int C, int y, int x, int c) {
  int64_t p[4];
  halve_taps(g, y, x, p);
  uint32_t S = 0, A = 0, k = 0;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const uint32_t v = src[p[t] * C + c];
    const bool ok = val[p[t]] != 0;
    A += v;
    S += ok ? v : 0u;
    k += ok;
  }
  return (T)(k ? (2 * S + k) / (2 * k) : (A + 2u) >> 2);
}

__device__ __forceinline__ uint8_t halve_valid_flag(const uint8_t* __restrict__ val, const HalveV& g, int y, int x) {
  int64_t p[4];
  halve_taps(g, y, x, p);
  return (uint8_t)((val[p[0]] | val[p[1]] | val[p[2]] | val[p[3]]) != 0);
}

// E outputs that begin at channel PH of an output pixel, from the 48 bytes of each source row that begin at that
// pixel's left source pixel (halve_window of pyramid.hip, halve16_window of image_u16.hip) and the 32 validity bytes
// of each row from the same pixel: output e is channel (PH + e) % C of pixel j = (PH + e) / C, whose taps are values
// 2jC + c and 2jC + c + C of the two windows and validity bytes 2j and 2j + 1.
template <typename T, int C, int PH>
__device__ __forceinline__ uint4 halve_valid_window(const T* __restrict__ top, const T* __restrict__ bot,
                                                    const uint8_t* __restrict__ vtop, const uint8_t* __restrict__ vbot) {
  constexpr int E = 16 / (int)sizeof(T), NV = 48 / (int)sizeof(T);
  const uint8_t* tp = (const uint8_t*)top;
  const uint8_t* bp = (const uint8_t*)bot;
  const uint4 tv[3] = {load16_any(tp), load16_any(tp + 16), load16_any(tp + 32)};
  const uint4 bv[3] = {load16_any(bp), load16_any(bp + 16), load16_any(bp + 32)};
  const uint4 av[2] = {load16_any(vtop), load16_any(vtop + 16)};
  const uint4 cv[2] = {load16_any(vbot), load16_any(vbot + 16)};
  T t[NV], u[NV], o[E];
  uint8_t a[32], b[32];
  __builtin_memcpy(t, tv, 48);
  __builtin_memcpy(u, bv, 48);
  __builtin_memcpy(a, av, 32);
  __builtin_memcpy(b, cv, 32);
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int j = (PH + e) / C, c = (PH + e) % C, s = 2 * j * C + c;
    const uint32_t v[4] = {t[s], t[s + C], u[s], u[s + C]};
    const bool ok[4] = {a[2 * j] != 0, a[2 * j + 1] != 0, b[2 * j] != 0, b[2 * j + 1] != 0};
    uint32_t S = 0, A = 0, k = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) A += v[i], S += ok[i] ? v[i] : 0u, k += ok[i];
    o[e] = (T)(k ? (2 * S + k) / (2 * k) : (A + 2u) >> 2);
  }
  uint4 r;
  __builtin_memcpy(&r, o, 16);
  return r;
}

template <typename T, int C>
__device__ __forceinline__ uint4 halve_valid_window_at(int ph, const T* __restrict__ top, const T* __restrict__ bot,
                                                       const uint8_t* __restrict__ vtop,
                                                       const uint8_t* __restrict__ vbot) {
  switch (ph) {
    case 0: return halve_valid_window<T, C, 0>(top, bot, vtop, vbot);
    case 1: return halve_valid_window<T, C, (C > 1 ? 1 : 0)>(top, bot, vtop, vbot);
    case 2: return halve_valid_window<T, C, (C > 2 ? 2 : 0)>(top, bot, vtop, vbot);
    default: return halve_valid_window<T, C, C - 1>(top, bot, vtop, vbot);
  }
}

// Units [0, nq) are the 16-byte chunks of the output image, units [nq, nq + mq) those of the output validity.  mis
// and vmis: the outputs' offsets behind a 16-byte boundary, in elements.
template <typename T, int C>
__global__ __launch_bounds__(256) void halve_valid_kernel(const T* __restrict__ src, const uint8_t* __restrict__ sval,
                                                          T* __restrict__ dst, uint8_t* __restrict__ dval, HalveV g,
                                                          int mis, int vmis) {
  constexpr int E = 16 / (int)sizeof(T), NV = 48 / (int)sizeof(T);
  const int rb = g.W2 * C;  // elements of an output row
  const int64_t spix = (int64_t)g.H * g.W;
  const int64_t n = (int64_t)g.H2 * g.W2 * C + mis, nq = (n + E - 1) / E;
  const int64_t m = (int64_t)g.H2 * g.W2 + vmis, mq = (m + 15) >> 4;
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq + mq; q += step) {
    if (q < nq) {
      const int64_t q0 = q * E, lo = max(q0, (int64_t)mis), hi = min(q0 + E, n);
      const int64_t px = (lo - mis) / C;
      int c = (int)((lo - mis) - px * C), y = (int)(px / g.W2), x = (int)(px - (int64_t)y * g.W2);
      if (lo == q0 && hi == q0 + E) {  // a whole chunk: the window path where its loads stay inside the source
        const int b0 = x * C + c, xl = (b0 + E - 1) / C;
        const int64_t pt = (int64_t)(2 * y) * g.W + 2 * x, pb = (int64_t)g.below(y) * g.W + 2 * x;
        if (b0 + E <= rb && 2 * xl + 1 < g.W && pb * C + NV <= spix * C && pb + 32 <= spix) {
          *(uint4*)(dst + (q0 - mis)) = halve_valid_window_at<T, C>(c, src + pt * C, src + pb * C, sval + pt, sval + pb);
          continue;
        }
      }
      T b[E];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        b[e] = 0;
        if (q0 + e >= lo && q0 + e < hi) {
          b[e] = halve_valid_value<T>(src, sval, g, C, y, x, c);
          if (++c == C) {
            c = 0;
            if (++x == g.W2) x = 0, ++y;
          }
        }
      }
      if (lo == q0 && hi == q0 + E) {
        uint4 v;
        __builtin_memcpy(&v, b, 16);
        *(uint4*)(dst + (q0 - mis)) = v;
      } else {
        for (int64_t e = lo; e < hi; ++e) dst[e - mis] = b[e - q0];
      }
    } else {
      const int64_t q0 = (q - nq) << 4, lo = max(q0, (int64_t)vmis), hi = min(q0 + 16, m);
      int y = (int)((lo - vmis) / g.W2), x = (int)((lo - vmis) - (int64_t)y * g.W2);
      uint8_t b[16];
      const int64_t pt = (int64_t)(2 * y) * g.W + 2 * x, pb = (int64_t)g.below(y) * g.W + 2 * x;
      if (lo == q0 && hi == q0 + 16 && x + 16 <= g.W2 && 2 * (x + 15) + 1 < g.W && pb + 32 <= spix) {
        const uint4 av[2] = {load16_any(sval + pt), load16_any(sval + pt + 16)};
        const uint4 cv[2] = {load16_any(sval + pb), load16_any(sval + pb + 16)};
        uint8_t a[32], d[32];
        __builtin_memcpy(a, av, 32);
        __builtin_memcpy(d, cv, 32);
#pragma unroll
        for (int e = 0; e < 16; ++e) b[e] = (uint8_t)((a[2 * e] | a[2 * e + 1] | d[2 * e] | d[2 * e + 1]) != 0);
        uint4 v;
        __builtin_memcpy(&v, b, 16);
        *(uint4*)(dval + (q0 - vmis)) = v;
        continue;
      }
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        b[e] = 0;
        if (q0 + e >= lo && q0 + e < hi) {
          b[e] = halve_valid_flag(sval, g, y, x);
          if (++x == g.W2) x = 0, ++y;
        }
      }
      if (lo == q0 && hi == q0 + 16) {
        uint4 v;
        __builtin_memcpy(&v, b, 16);
        *(uint4*)(dval + (q0 - vmis)) = v;
      } else {
        for (int64_t e = lo; e < hi; ++e) dval[e - vmis] = b[e - q0];
      }
    }
  }
}

// ---- band range over the valid pixels -------------------------------------------------------------------------------

__global__ void band_range_valid_init_kernel(uint32_t* __restrict__ out, int C) {
  if ((int)threadIdx.x < 2 * C) out[threadIdx.x] = (threadIdx.x & 1) ? 0u : 0xFFFFFFFFu;
}

// a band that met no valid pixel still holds the start values: it becomes (0, 0)
__global__ void band_range_valid_finish_kernel(uint32_t* __restrict__ out, int C) {
  if ((int)threadIdx.x < C && out[2 * threadIdx.x] > out[2 * threadIdx.x + 1]) out[2 * threadIdx.x] = 0u;
}

// band_range_kernel of image_u16.hip with a validity byte per pixel: a unit is 8 pixels, C 16-byte loads that begin
// at a pixel and their 8 validity bytes; a value of an invalid pixel joins neither the minimum nor the maximum.  Wave
// reduction, workgroup reduction through LDS, then one atomic min and max per workgroup and band.
template <int C>
__global__ __launch_bounds__(256) void band_range_valid_kernel(const uint16_t* __restrict__ img,
                                                               const uint8_t* __restrict__ val, int64_t npix,
                                                               uint32_t* __restrict__ out) {
  __shared__ uint32_t red[2][4][4];
  uint32_t mn[C], mx[C];
#pragma unroll
  for (int c = 0; c < C; ++c) mn[c] = 0xFFFFFFFFu, mx[c] = 0u;
  const int64_t units = npix >> 3, step = (int64_t)gridDim.x * blockDim.x;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t u = tid; u < units; u += step) {
    uint4 q[C];
    uint16_t v[8 * C];
    uint8_t ok[8];
#pragma unroll
    for (int k = 0; k < C; ++k) q[k] = load16_any((const uint8_t*)(img + u * 8 * C) + 16 * k);
    __builtin_memcpy(v, q, 16 * C);
#pragma unroll
    for (int k = 0; k < 8; ++k) ok[k] = val[u * 8 + k];
#pragma unroll
    for (int k = 0; k < 8 * C; ++k) {
      if (ok[k / C]) {
        mn[k % C] = min(mn[k % C], (uint32_t)v[k]);
        mx[k % C] = max(mx[k % C], (uint32_t)v[k]);
      }
    }
  }
  if (tid < (npix & 7) && val[(units << 3) + tid]) {
    const uint16_t* p = img + ((units << 3) + tid) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) mn[c] = min(mn[c], (uint32_t)p[c]), mx[c] = max(mx[c], (uint32_t)p[c]);
  }
#pragma unroll
  for (int c = 0; c < C; ++c) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      mn[c] = min(mn[c], (uint32_t)__shfl_down(mn[c], o, 64));
      mx[c] = max(mx[c], (uint32_t)__shfl_down(mx[c], o, 64));
    }
    if ((threadIdx.x & 63) == 0) red[0][c][threadIdx.x >> 6] = mn[c], red[1][c][threadIdx.x >> 6] = mx[c];
  }
  __syncthreads();
  if ((int)threadIdx.x < C) {
    const int c = threadIdx.x;
    atomicMin(out + 2 * c, min(min(red[0][c][0], red[0][c][1]), min(red[0][c][2], red[0][c][3])));
    atomicMax(out + 2 * c + 1, max(max(red[1][c][0], red[1][c][1]), max(red[1][c][2], red[1][c][3])));
  }
}

static bool valid_apart(const void* a, int64_t a_bytes, const void* b, int64_t b_bytes) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa + (uintptr_t)a_bytes <= pb || pb + (uintptr_t)b_bytes <= pa;
}

static int valid_blocks(int64_t units) {
  const int64_t b = (units + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}

template <typename T>
static int halve_valid(const char* what, const T* src, const uint8_t* sval, T* dst, uint8_t* dval, int H, int W, int C,
                       int cmin, void* stream) {
  DSIC_REQUIRE(src && sval && dst && dval, "%s: null pointer", what);
  DSIC_REQUIRE(C >= cmin && C <= 4, "%s: C=%d must be in %d..4", what, C, cmin);
  DSIC_REQUIRE(H >= 1 && W >= 1, "%s: H=%d W=%d must both be at least 1", what, H, W);
  DSIC_REQUIRE((int64_t)W * C * (int64_t)sizeof(T) <= INT_MAX, "%s: a row of W=%d pixels of C=%d is over 2^31 - 1 bytes",
               what, W, C);
  DSIC_REQUIRE((((uintptr_t)src | (uintptr_t)dst) & (sizeof(T) - 1)) == 0, "%s: src and dst must be %d-byte aligned", what,
               (int)sizeof(T));
  const HalveV g = {H, W, H / 2 + (H & 1), W / 2 + (W & 1)};
  const int64_t sb = (int64_t)sizeof(T) * H * W * C, db = (int64_t)sizeof(T) * g.H2 * g.W2 * C;
  const int64_t svb = (int64_t)H * W, dvb = (int64_t)g.H2 * g.W2;
  DSIC_REQUIRE(valid_apart(src, sb, dst, db) && valid_apart(sval, svb, dval, dvb) && valid_apart(src, sb, dval, dvb) &&
                   valid_apart(sval, svb, dst, db) && valid_apart(dst, db, dval, dvb),
               "%s: src and dst overlap", what);
  const int mis = (int)(((uintptr_t)dst & 15) / sizeof(T)), vmis = (int)((uintptr_t)dval & 15);
  const int64_t units = (db / (int64_t)sizeof(T) + mis) / (16 / (int64_t)sizeof(T)) + (dvb + vmis) / 16 + 2;
  const dim3 grid(valid_blocks(units));
  hipStream_t st = (hipStream_t)stream;
  switch (C) {
    case 1: hipLaunchKernelGGL((halve_valid_kernel<T, 1>), grid, dim3(256), 0, st, src, sval, dst, dval, g, mis, vmis); break;
    case 2: hipLaunchKernelGGL((halve_valid_kernel<T, 2>), grid, dim3(256), 0, st, src, sval, dst, dval, g, mis, vmis); break;
    case 3: hipLaunchKernelGGL((halve_valid_kernel<T, 3>), grid, dim3(256), 0, st, src, sval, dst, dval, g, mis, vmis); break;
    default: hipLaunchKernelGGL((halve_valid_kernel<T, 4>), grid, dim3(256), 0, st, src, sval, dst, dval, g, mis, vmis); break;
  }
  return check_launch(what);
}

}  // namespace dsic

using namespace dsic;

extern "C" int dsic_image_halve_valid_u8(const uint8_t* src_hwc, const uint8_t* src_valid, uint8_t* dst_hwc,
                                         uint8_t* dst_valid, int H, int W, int C, void* stream) {
  return halve_valid<uint8_t>("image_halve_valid_u8", src_hwc, src_valid, dst_hwc, dst_valid, H, W, C, 1, stream);
}

extern "C" int dsic_image_halve_valid_u16(const uint16_t* src_hwc, const uint8_t* src_valid, uint16_t* dst_hwc,
                                          uint8_t* dst_valid, int H, int W, int C, void* stream) {
  return halve_valid<uint16_t>("image_halve_valid_u16", src_hwc, src_valid, dst_hwc, dst_valid, H, W, C, 1, stream);
}

extern "C" int dsic_band_range_valid_u16(const uint16_t* img_hwc, const uint8_t* valid_hw, int H, int W, int C,
                                         uint32_t* out_lohi_dev, void* stream) {
  DSIC_REQUIRE(img_hwc && valid_hw && out_lohi_dev, "band_range_valid_u16: null pointer");
  DSIC_REQUIRE(C >= 1 && C <= 4, "band_range_valid_u16: C=%d must be in 1..4", C);
  DSIC_REQUIRE(((uintptr_t)img_hwc & 1) == 0, "band_range_valid_u16: the uint16 image must be 2-byte aligned");
  DSIC_REQUIRE(H >= 1 && W >= 1, "band_range_valid_u16: empty image %dx%d", H, W);
  DSIC_REQUIRE((int64_t)W * C * 2 <= INT_MAX, "band_range_valid_u16: a row of W=%d pixels of C=%d uint16 is over 2^31 - 1 bytes",
               W, C);
  DSIC_REQUIRE(((uintptr_t)out_lohi_dev & 3) == 0, "band_range_valid_u16: out must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(band_range_valid_init_kernel, dim3(1), dim3(64), 0, st, out_lohi_dev, C);
  int rc = check_launch("band_range_valid_u16(init)");
  if (rc) return rc;
  const int64_t npix = (int64_t)H * W;
  int64_t blocks = ((npix >> 3) + 4 * 256 - 1) / (4 * 256);  // about four units per lane
  blocks = blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);
  switch (C) {
    case 1: hipLaunchKernelGGL(band_range_valid_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, st, img_hwc, valid_hw, npix, out_lohi_dev); break;
    case 2: hipLaunchKernelGGL(band_range_valid_kernel<2>, dim3((unsigned)blocks), dim3(256), 0, st, img_hwc, valid_hw, npix, out_lohi_dev); break;
    case 3: hipLaunchKernelGGL(band_range_valid_kernel<3>, dim3((unsigned)blocks), dim3(256), 0, st, img_hwc, valid_hw, npix, out_lohi_dev); break;
    default: hipLaunchKernelGGL(band_range_valid_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, st, img_hwc, valid_hw, npix, out_lohi_dev); break;
  }
  rc = check_launch("band_range_valid_u16");
  if (rc) return rc;
  hipLaunchKernelGGL(band_range_valid_finish_kernel, dim3(1), dim3(64), 0, st, out_lohi_dev, C);
  return check_launch("band_range_valid_u16(finish)");
}
