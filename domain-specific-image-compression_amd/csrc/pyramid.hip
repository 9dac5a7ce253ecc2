// Image overviews (codec.build_overviews): one level of the pyramid from the one before it, one launch per level.
// dst is H2 x W2 with H2 = ceil(H/2), W2 = ceil(W/2); output pixel (y, x) is taken from source rows 2y and
// min(2y+1, H-1) and columns 2x and min(2x+1, W-1), so on an odd side the last row or column counts twice and nothing
// outside H x W is read.  uint8 HWC: (a + b + c + d + 2) >> 2 per channel, over the taps, the value and the window of
// halve.h, which states them once for both widths and for masked scenes (3, 4 and over 4 channels: halve_u8_kernel
// below; 1 and 2 channels: halve.h's halve_kernel); float32 CHW: ((a + b) + (c + d)) * 0.25f, a = top-left,
// b = top-right, c = bottom-left, d = bottom-right (built with -ffp-contract=off: NumPy gives the same bits).
//
// Byte movers as image_codec.hip's.  An output row is W2*C bytes or W2 floats, no multiple of 16 bytes in general, so
// the output is one flat array: a thread owns one of its aligned 16-byte chunks and stores it as a dwordx4 (uint8: the
// cursor of hwc_chunks.h; both: the ragged head and tail of the array are element stores).  A float32 chunk that
// lies in one output row away from a repeated last column reads its two source rows as 16-byte loads (load16_any: the
// source is aligned as it happens to be); one that crosses a row end or meets the repeated column goes element by
// element.
#include <limits.h>

#include "halve.h"

namespace dsic {

// elements [i0, i0 + n), n <= 16, of the flat uint8 output -> b[0 .. n), tap by tap
__device__ __forceinline__ void halve_run(const uint8_t* __restrict__ src, const Halve& g, int C, int64_t i0, int n,
                                          uint8_t* b) {
  HwcCursorYX u = hwc_cursor_yx(i0, C, g.W2);
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    b[e] = 0;
    if (e < n) {
      b[e] = halve_at<uint8_t, false>(src, nullptr, g, C, u.y, u.x, u.c);
      u.step(C, g.W2);
    }
  }
}

// uint8 [H][W][C] -> uint8 [H2][W2][C], n bytes, for 3, 4 and (CT = 0, C = Crt, tap by tap) any other number of
// channels.  The taps, the value and the window are halve.h's, the cursor hwc_chunks.h's.  The kernel is its own for
// what the shared halve_kernel does otherwise and what that costs here (profiles/pixel_movers_ab.json, the 4096 x 4096
// x 3 level, each against the earlier kernel in the same job): the flat output is split into `head` bytes up to dst's
// first aligned chunk, nfull whole chunks and a tail, the two ragged ends, under 16 bytes each, go to threads 0 and 1 of
// workgroup 0 and the loop meets whole chunks only; and every phase of the window packs its 16 bytes before the phases
// meet (halve_window_packed_at).  As it stands the level takes 27.17 us against 27.09 us; through halve_kernel it took
// 27.80 us against 27.05 us, and with this split but the window packed behind the phases 28.22 us against 27.09 us.
template <int CT>
__global__ __launch_bounds__(256) void halve_u8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                       Halve g, int Crt, int64_t n, int head, int64_t nfull) {
  const int C = CT ? CT : Crt;
  const int rb = g.W2 * C;  // bytes of an output row
  const int64_t total = (int64_t)g.H * g.W * C;
  if (blockIdx.x == 0 && threadIdx.x < 2) {
    const int64_t lo = threadIdx.x ? head + 16 * nfull : 0, hi = threadIdx.x ? n : head;
    uint8_t b[16];
    halve_run(src, g, C, lo, (int)(hi - lo), b);
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
      const int xf = b0 / C, xl = (b0 + 15) / C;
      const int64_t st = ((int64_t)(2 * y) * g.W + 2 * xf) * C, sb = ((int64_t)g.below(y) * g.W + 2 * xf) * C;
      if (b0 + 16 <= rb && 2 * xl + 1 < g.W && sb + 48 <= total) {
        v = halve_window_packed_at<uint8_t, (CT ? CT : 1), false>(b0 - xf * C, src + st, src + sb, nullptr, nullptr);
        done = true;
      }
    }
    if (!done) {
      uint8_t b[16];
      halve_run(src, g, C, q0, 16, b);
      __builtin_memcpy(&v, b, 16);
    }
    *(uint4*)(dst + q0) = v;  // a whole chunk, 16-byte aligned
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

}  // namespace dsic

using namespace dsic;

extern "C" int dsic_image_halve_u8(const uint8_t* src_hwc, uint8_t* dst_hwc, int H, int W, int C, void* stream) {
  DSIC_REQUIRE(src_hwc && dst_hwc, "image_halve_u8: null pointer");
  DSIC_REQUIRE(C >= 1 && H >= 1 && W >= 1, "image_halve_u8: H=%d W=%d C=%d must all be at least 1", H, W, C);
  DSIC_REQUIRE((int64_t)W * C <= INT_MAX, "image_halve_u8: a row of W=%d pixels of C=%d bytes is over 2^31 - 1 bytes",
               W, C);
  const Halve g = make_halve(H, W);
  DSIC_REQUIRE(buffers_apart(src_hwc, (int64_t)H * W * C, dst_hwc, (int64_t)g.H2 * g.W2 * C),
               "image_halve_u8: src and dst overlap");
  const int64_t n = (int64_t)g.H2 * g.W2 * C;
  int64_t head = (16 - ((uintptr_t)dst_hwc & 15)) & 15;
  if (head > n) head = n;
  const int64_t nfull = (n - head) >> 4;
  const dim3 grid(flat_blocks(nfull));
  hipStream_t st = (hipStream_t)stream;
  if (C == 1 || C == 2) {  // the window instantiations the earlier code did not have: the shared kernel
    launch_halve<uint8_t, false, 2>(src_hwc, dst_hwc, g, C, {}, st);
  } else if (C == 3) {
    hipLaunchKernelGGL(halve_u8_kernel<3>, grid, dim3(256), 0, st, src_hwc, dst_hwc, g, C, n, (int)head, nfull);
  } else if (C == 4) {
    hipLaunchKernelGGL(halve_u8_kernel<4>, grid, dim3(256), 0, st, src_hwc, dst_hwc, g, C, n, (int)head, nfull);
  } else {
    hipLaunchKernelGGL(halve_u8_kernel<0>, grid, dim3(256), 0, st, src_hwc, dst_hwc, g, C, n, (int)head, nfull);
  }
  return check_launch("image_halve_u8");
}

extern "C" int dsic_image_halve_f32(const float* src_chw, float* dst_chw, int C, int H, int W, void* stream) {
  DSIC_REQUIRE(src_chw && dst_chw, "image_halve_f32: null pointer");
  DSIC_REQUIRE(C >= 1 && H >= 1 && W >= 1, "image_halve_f32: C=%d H=%d W=%d must all be at least 1", C, H, W);
  DSIC_REQUIRE((((uintptr_t)src_chw | (uintptr_t)dst_chw) & 3) == 0,
               "image_halve_f32: src and dst must be 4-byte aligned");
  const Halve g = make_halve(H, W);
  const int64_t n = (int64_t)C * g.H2 * g.W2;
  DSIC_REQUIRE(buffers_apart(src_chw, 4 * (int64_t)C * H * W, dst_chw, 4 * n), "image_halve_f32: src and dst overlap");
  int64_t head = ((16 - ((uintptr_t)dst_chw & 15)) & 15) >> 2;
  if (head > n) head = n;
  const int64_t nfull = (n - head) >> 2;
  hipLaunchKernelGGL(halve_f32_kernel, dim3(flat_blocks(nfull)), dim3(256), 0, (hipStream_t)stream, src_chw, dst_chw, g,
                     n, (int)head, nfull);
  return check_launch("image_halve_f32");
}
