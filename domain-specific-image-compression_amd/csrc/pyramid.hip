// Image overviews (codec.build_overviews): one level of the pyramid from the one before it, one launch per level.
// dst is H2 x W2 with H2 = ceil(H/2), W2 = ceil(W/2); output pixel (y, x) is taken from source rows 2y and
// min(2y+1, H-1) and columns 2x and min(2x+1, W-1), so on an odd side the last row or column counts twice and nothing
// outside H x W is read.  uint8 HWC: (a + b + c + d + 2) >> 2 per channel; float32 CHW: ((a + b) + (c + d)) * 0.25f,
// a = top-left, b = top-right, c = bottom-left, d = bottom-right (built with -ffp-contract=off: NumPy gives the same
// bits).
//
// Byte movers as image_codec.hip's.  An output row is W2*C bytes or W2 floats, no multiple of 16 bytes in general, so
// the output is one flat array: a thread owns one of its aligned 16-byte chunks and stores it as a dwordx4; the ragged
// head and tail of the array are byte (dword) stores.  A chunk that lies in one output row away from a repeated last
// column reads its two source rows as 16-byte loads (load16_any: the source is aligned as it happens to be); a chunk
// that crosses a row end, meets the repeated column, or whose loads would pass the end of the image goes element by
// element.
#include <limits.h>

#include "byte_movers.h"

namespace dsic {

struct Halve {
  int H, W, H2, W2;
  __device__ __forceinline__ int below(int y) const { return min(2 * y + 1, H - 1); }
  __device__ __forceinline__ int right(int x) const { return min(2 * x + 1, W - 1); }
};

// elements [i0, i0 + n), n <= 16, of the flat uint8 output -> b[0 .. n)
__device__ __forceinline__ void halve_bytes(const uint8_t* __restrict__ src, const Halve& g, int C, int64_t i0, int n,
                                            uint8_t* b) {
  const int64_t p = i0 / C;
  int c = (int)(i0 - p * C), y = (int)(p / g.W2), x = (int)(p - (int64_t)y * g.W2);
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    b[e] = 0;
    if (e < n) {
      const uint8_t* top = src + (int64_t)(2 * y) * g.W * C + c;
      const uint8_t* bot = src + (int64_t)g.below(y) * g.W * C + c;
      const int64_t xa = (int64_t)(2 * x) * C, xb = (int64_t)g.right(x) * C;
      b[e] = (uint8_t)(((int)top[xa] + (int)top[xb] + (int)bot[xa] + (int)bot[xb] + 2) >> 2);
      if (++c == C) {
        c = 0;
        if (++x == g.W2) x = 0, ++y;
      }
    }
  }
}

// 16 output bytes that begin at channel PH of an output pixel, from the 48 bytes of each source row that begin at
// that pixel's left source pixel: output byte e is channel (PH + e) % C of pixel j = (PH + e) / C, whose sources are
// bytes 2jC + c and 2jC + c + C of the two windows (at most byte 39).
template <int C, int PH>
__device__ __forceinline__ uint4 halve_window(const uint8_t* __restrict__ top, const uint8_t* __restrict__ bot) {
  const uint4 tv[3] = {load16_any(top), load16_any(top + 16), load16_any(top + 32)};
  const uint4 bv[3] = {load16_any(bot), load16_any(bot + 16), load16_any(bot + 32)};
  uint8_t t[48], u[48], o[16];
  __builtin_memcpy(t, tv, 48);
  __builtin_memcpy(u, bv, 48);
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int j = (PH + e) / C, c = (PH + e) % C, a = 2 * j * C + c;
    o[e] = (uint8_t)(((int)t[a] + (int)t[a + C] + (int)u[a] + (int)u[a + C] + 2) >> 2);
  }
  uint4 v;
  __builtin_memcpy(&v, o, 16);
  return v;
}

template <int C>
__device__ __forceinline__ uint4 halve_window_at(int ph, const uint8_t* __restrict__ top,
                                                 const uint8_t* __restrict__ bot) {
  switch (ph) {
    case 0: return halve_window<C, 0>(top, bot);
    case 1: return halve_window<C, 1>(top, bot);
    case 2: return halve_window<C, 2>(top, bot);
    default: return halve_window<C, C - 1>(top, bot);
  }
}

// uint8 [H][W][C] -> uint8 [H2][W2][C], n bytes: `head` bytes up to dst's first aligned chunk, nfull chunks, a tail.
// CT = C for 3 and 4 channels, the sizes with a window path; 0 = any C, element by element.
template <int CT>
__global__ __launch_bounds__(256) void halve_u8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                       Halve g, int C, int64_t n, int head, int64_t nfull) {
  const int rb = g.W2 * C;  // bytes of an output row
  const int64_t total = (int64_t)g.H * g.W * C;
  if (blockIdx.x == 0 && threadIdx.x < 2) {  // the ragged ends: under 16 bytes each
    const int64_t lo = threadIdx.x ? head + 16 * nfull : 0, hi = threadIdx.x ? n : head;
    uint8_t b[16];
    halve_bytes(src, g, C, lo, (int)(hi - lo), b);
#pragma unroll
    for (int e = 0; e < 16; ++e)
      if (e < hi - lo) dst[lo + e] = b[e];
  }
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nfull; q += step) {
    const int64_t q0 = head + 16 * q;
    uint4 v;
    bool done = false;
    if (CT) {
      const int y = (int)(q0 / rb), b0 = (int)(q0 - (int64_t)y * rb);
      const int xf = b0 / CT, xl = (b0 + 15) / CT;
      const int64_t st = ((int64_t)(2 * y) * g.W + 2 * xf) * CT, sb = ((int64_t)g.below(y) * g.W + 2 * xf) * CT;
      if (b0 + 16 <= rb && 2 * xl + 1 < g.W && sb + 48 <= total) {
        v = halve_window_at<CT ? CT : 3>(b0 - xf * CT, src + st, src + sb);
        done = true;
      }
    }
    if (!done) {
      uint8_t b[16];
      halve_bytes(src, g, C, q0, 16, b);
      __builtin_memcpy(&v, b, 16);
    }
    *(uint4*)(dst + q0) = v;
  }
}

__device__ __forceinline__ float halve4(float a, float b, float c, float d) { return ((a + b) + (c + d)) * 0.25f; }

// element i of the flat float32 output
__device__ __forceinline__ float halve_float(const float* __restrict__ src, const Halve& g, int64_t i) {
  const int64_t r = i / g.W2;  // output row, counted through the planes
  const int x = (int)(i - r * g.W2);
  const int64_t c = r / g.H2;
  const int y = (int)(r - c * g.H2);
  const float* top = src + (c * g.H + 2 * y) * g.W;
  const float* bot = src + (c * g.H + g.below(y)) * g.W;
  return halve4(top[2 * x], top[g.right(x)], bot[2 * x], bot[g.right(x)]);
}

__device__ __forceinline__ float4 load_float4_any(const float* p) {
  const uint4 v = load16_any((const uint8_t*)p);
  return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}

// float32 [C][H][W] -> float32 [C][H2][W2], n floats: `head` floats up to dst's first aligned chunk, nfull chunks of 4
__global__ __launch_bounds__(256) void halve_f32_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                        Halve g, int64_t n, int head, int64_t nfull) {
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (tid < head) dst[tid] = halve_float(src, g, tid);
  for (int64_t e = head + 4 * nfull + tid; e < n; e += step) dst[e] = halve_float(src, g, e);
  for (int64_t q = tid; q < nfull; q += step) {
    const int64_t q0 = head + 4 * q;
    const int64_t r = q0 / g.W2;
    const int x = (int)(q0 - r * g.W2);
    float4 v;
    if (x + 4 <= g.W2 && 2 * (x + 3) + 1 < g.W) {  // 8 floats of each source row, all inside it
      const int64_t c = r / g.H2;
      const int y = (int)(r - c * g.H2);
      const float* top = src + (c * g.H + 2 * y) * g.W + 2 * x;
      const float* bot = src + (c * g.H + g.below(y)) * g.W + 2 * x;
      const float4 t0 = load_float4_any(top), t1 = load_float4_any(top + 4);
      const float4 b0 = load_float4_any(bot), b1 = load_float4_any(bot + 4);
      v = make_float4(halve4(t0.x, t0.y, b0.x, b0.y), halve4(t0.z, t0.w, b0.z, b0.w), halve4(t1.x, t1.y, b1.x, b1.y),
                      halve4(t1.z, t1.w, b1.z, b1.w));
    } else {
      v = make_float4(halve_float(src, g, q0), halve_float(src, g, q0 + 1), halve_float(src, g, q0 + 2),
                      halve_float(src, g, q0 + 3));
    }
    *(float4*)(dst + q0) = v;
  }
}

static int halve_blocks(int64_t chunks) {
  const int64_t b = (chunks + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}

static bool apart(const void* a, int64_t a_bytes, const void* b, int64_t b_bytes) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa + (uintptr_t)a_bytes <= pb || pb + (uintptr_t)b_bytes <= pa;
}

}  // namespace dsic

using namespace dsic;

extern "C" int dsic_image_halve_u8(const uint8_t* src_hwc, uint8_t* dst_hwc, int H, int W, int C, void* stream) {
  DSIC_REQUIRE(src_hwc && dst_hwc, "image_halve_u8: null pointer");
  DSIC_REQUIRE(C >= 1 && H >= 1 && W >= 1, "image_halve_u8: H=%d W=%d C=%d must all be at least 1", H, W, C);
  DSIC_REQUIRE((int64_t)W * C <= INT_MAX, "image_halve_u8: a row of W=%d pixels of C=%d bytes is over 2^31 - 1 bytes", W,
               C);
  const Halve g = {H, W, H / 2 + (H & 1), W / 2 + (W & 1)};
  const int64_t n = (int64_t)g.H2 * g.W2 * C;
  DSIC_REQUIRE(apart(src_hwc, (int64_t)H * W * C, dst_hwc, n), "image_halve_u8: src and dst overlap");
  int64_t head = (16 - ((uintptr_t)dst_hwc & 15)) & 15;
  if (head > n) head = n;
  const int64_t nfull = (n - head) >> 4;
  const dim3 grid(halve_blocks(nfull));
  hipStream_t st = (hipStream_t)stream;
  if (C == 3) hipLaunchKernelGGL(halve_u8_kernel<3>, grid, dim3(256), 0, st, src_hwc, dst_hwc, g, C, n, (int)head, nfull);
  else if (C == 4)
    hipLaunchKernelGGL(halve_u8_kernel<4>, grid, dim3(256), 0, st, src_hwc, dst_hwc, g, C, n, (int)head, nfull);
  else hipLaunchKernelGGL(halve_u8_kernel<0>, grid, dim3(256), 0, st, src_hwc, dst_hwc, g, C, n, (int)head, nfull);
  return check_launch("image_halve_u8");
}

extern "C" int dsic_image_halve_f32(const float* src_chw, float* dst_chw, int C, int H, int W, void* stream) {
  DSIC_REQUIRE(src_chw && dst_chw, "image_halve_f32: null pointer");
  DSIC_REQUIRE(C >= 1 && H >= 1 && W >= 1, "image_halve_f32: C=%d H=%d W=%d must all be at least 1", C, H, W);
  DSIC_REQUIRE((((uintptr_t)src_chw | (uintptr_t)dst_chw) & 3) == 0, "image_halve_f32: src and dst must be 4-byte aligned");
  const Halve g = {H, W, H / 2 + (H & 1), W / 2 + (W & 1)};
  const int64_t n = (int64_t)C * g.H2 * g.W2;
  DSIC_REQUIRE(apart(src_chw, 4 * (int64_t)C * H * W, dst_chw, 4 * n), "image_halve_f32: src and dst overlap");
  int64_t head = ((16 - ((uintptr_t)dst_chw & 15)) & 15) >> 2;
  if (head > n) head = n;
  const int64_t nfull = (n - head) >> 2;
  hipLaunchKernelGGL(halve_f32_kernel, dim3(halve_blocks(nfull)), dim3(256), 0, (hipStream_t)stream, src_chw, dst_chw, g,
                     n, (int)head, nfull);
  return check_launch("image_halve_f32");
}
