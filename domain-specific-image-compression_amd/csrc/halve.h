// The 2 x 2 halving of an HWC image (uint8 or uint16), with or without a validity image beside it: the one statement
// behind dsic_image_halve_u8 (pyramid.hip), dsic_image_halve_u16 (image_u16.hip) and dsic_image_halve_valid_u8 / _u16
// (valid.hip).  dst is H2 x W2 with H2 = ceil(H/2), W2 = ceil(W/2); output pixel (y, x) takes four taps, rows 2y and
// min(2y+1, H-1), columns 2x and min(2x+1, W-1), a repeated tap counting twice.  Per channel, with A the sum of the
// taps: (A + 2) >> 2.  With validity (V), k the number of valid taps and S the sum over them: (2 S + k) / (2 k), the
// mean over the valid taps rounded half up, and (A + 2) >> 2 for k = 0; the output pixel is valid iff k > 0.  All in
// integers: nothing depends on any order.
//
// The outputs are flat arrays at any element alignment, walked by hwc_chunks.h: a thread owns one aligned 16-byte
// chunk of the image or, with V, of the validity.  A whole chunk that lies in one output row away from a repeated last
// column, and whose loads stay inside the source, takes the window path: three 16-byte loads of each source row, with
// V two of each validity row (load16_any: the sources are aligned as they happen to be).  Every other chunk goes tap
// by tap.
#pragma once
#include <algorithm>

#include "byte_movers.h"
#include "hwc_chunks.h"

namespace dsic {

struct Halve {
  int H, W, H2, W2;
  __device__ __forceinline__ int below(int y) const { return min(2 * y + 1, H - 1); }
  __device__ __forceinline__ int right(int x) const { return min(2 * x + 1, W - 1); }
};
static inline Halve make_halve(int H, int W) { return {H, W, H / 2 + (H & 1), W / 2 + (W & 1)}; }

// the validity image of a masked halving and its output, vmis bytes behind a 16-byte boundary; nothing without V
template <bool V>
struct HalveValid {};
template <>
struct HalveValid<true> {
  const uint8_t* src;
  uint8_t* dst;
  int vmis;
};

// the four taps' pixel numbers of output pixel (y, x)
__device__ __forceinline__ void halve_taps(const Halve& g, int y, int x, int64_t* p) {
  const int64_t r0 = (int64_t)(2 * y) * g.W, r1 = (int64_t)g.below(y) * g.W;
  const int xa = 2 * x, xb = g.right(x);
  p[0] = r0 + xa, p[1] = r0 + xb, p[2] = r1 + xa, p[3] = r1 + xb;
}

// the output value of four taps; ok is read with V only.  S is summed with a mask of the tap's validity, not a select:
// the same sum, and the masked uint8 kernels stay within 64 VGPRs with it
template <typename T, bool V>
__device__ __forceinline__ T halve_value(const uint32_t (&v)[4], const bool (&ok)[4]) {
  uint32_t S = 0, A = 0, k = 0;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    A += v[t];
    if constexpr (V) S += v[t] & (0u - (uint32_t)ok[t]), k += ok[t];
  }
  if constexpr (V) return (T)(k ? (2 * S + k) / (2 * k) : (A + 2u) >> 2);
  return (T)((A + 2u) >> 2);
}

// channel c of output pixel (y, x), tap by tap
template <typename T, bool V>
__device__ __forceinline__ T halve_at(const T* __restrict__ src, const uint8_t* __restrict__ val, const Halve& g, int C,
                                      int y, int x, int c) {
  int64_t p[4];
  halve_taps(g, y, x, p);
  uint32_t v[4];
  bool ok[4] = {true, true, true, true};
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    v[t] = src[p[t] * C + c];
    if constexpr (V) ok[t] = val[p[t]] != 0;
  }
  return halve_value<T, V>(v, ok);
}

__device__ __forceinline__ uint8_t halve_flag(const uint8_t* __restrict__ val, const Halve& g, int y, int x) {
  int64_t p[4];
  halve_taps(g, y, x, p);
  return (uint8_t)((val[p[0]] | val[p[1]] | val[p[2]] | val[p[3]]) != 0);
}

// E outputs that begin at channel PH of an output pixel, from the 48 bytes of each source row that begin at that
// pixel's left source pixel and, with V, the 32 validity bytes of each row from the same pixel: output e is channel
// (PH + e) % C of pixel j = (PH + e) / C, whose taps are values 2jC + c and 2jC + c + C of the two windows (at most
// value 39 of 48 for uint8, 22 of 24 for uint16) and validity bytes 2j and 2j + 1.
template <typename T, int C, int PH, bool V>
__device__ __forceinline__ void halve_window(const T* __restrict__ top, const T* __restrict__ bot,
                                             const uint8_t* __restrict__ vtop, const uint8_t* __restrict__ vbot, T* o) {
  constexpr int E = 16 / (int)sizeof(T), NV = 48 / (int)sizeof(T);
  const uint8_t* tp = (const uint8_t*)top;
  const uint8_t* bp = (const uint8_t*)bot;
  uint8_t a[32], b[32];
  if constexpr (V) {
    const uint4 av[2] = {load16_any(vtop), load16_any(vtop + 16)};
    const uint4 cv[2] = {load16_any(vbot), load16_any(vbot + 16)};
    __builtin_memcpy(a, av, 32);
    __builtin_memcpy(b, cv, 32);
  }
  const uint4 tv[3] = {load16_any(tp), load16_any(tp + 16), load16_any(tp + 32)};
  const uint4 bv[3] = {load16_any(bp), load16_any(bp + 16), load16_any(bp + 32)};
  T t[NV], u[NV];
  __builtin_memcpy(t, tv, 48);
  __builtin_memcpy(u, bv, 48);
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int j = (PH + e) / C, c = (PH + e) % C, s = 2 * j * C + c;
    const uint32_t v[4] = {t[s], t[s + C], u[s], u[s + C]};
    bool ok[4] = {true, true, true, true};
    if constexpr (V) ok[0] = a[2 * j] != 0, ok[1] = a[2 * j + 1] != 0, ok[2] = b[2 * j] != 0, ok[3] = b[2 * j + 1] != 0;
    o[e] = halve_value<T, V>(v, ok);
  }
}

template <typename T, int C, bool V>
__device__ __forceinline__ void halve_window_at(int ph, const T* __restrict__ top, const T* __restrict__ bot,
                                                const uint8_t* __restrict__ vtop, const uint8_t* __restrict__ vbot,
                                                T* o) {
  switch (ph) {
    case 0: return halve_window<T, C, 0, V>(top, bot, vtop, vbot, o);
    case 1: return halve_window<T, C, (C > 1 ? 1 : 0), V>(top, bot, vtop, vbot, o);
    case 2: return halve_window<T, C, (C > 2 ? 2 : 0), V>(top, bot, vtop, vbot, o);
    default: return halve_window<T, C, C - 1, V>(top, bot, vtop, vbot, o);
  }
}

// The same with every phase packing its 16 bytes before the phases meet again, for halve_u8_kernel of pyramid.hip:
// behind the switch above the E outputs are E separate values, packed once; here they are one uint4 per phase.  The
// compiler then keeps more of the window's loads in flight, at 87 - 97 VGPRs where the masked and the uint16
// kernels are held to 64, so those take the form above (profiles/pixel_movers_ab.json has both measured for uint8).
template <typename T, int C, int PH, bool V>
__device__ __forceinline__ uint4 halve_window_packed(const T* __restrict__ top, const T* __restrict__ bot,
                                                     const uint8_t* __restrict__ vtop,
                                                     const uint8_t* __restrict__ vbot) {
  T o[16 / sizeof(T)];
  halve_window<T, C, PH, V>(top, bot, vtop, vbot, o);
  uint4 r;
  __builtin_memcpy(&r, o, 16);
  return r;
}

template <typename T, int C, bool V>
__device__ __forceinline__ uint4 halve_window_packed_at(int ph, const T* __restrict__ top, const T* __restrict__ bot,
                                                        const uint8_t* __restrict__ vtop,
                                                        const uint8_t* __restrict__ vbot) {
  switch (ph) {
    case 0: return halve_window_packed<T, C, 0, V>(top, bot, vtop, vbot);
    case 1: return halve_window_packed<T, C, (C > 1 ? 1 : 0), V>(top, bot, vtop, vbot);
    case 2: return halve_window_packed<T, C, (C > 2 ? 2 : 0), V>(top, bot, vtop, vbot);
    default: return halve_window_packed<T, C, C - 1, V>(top, bot, vtop, vbot);
  }
}

// chunk q of the output validity: a pixel is valid iff one of its four taps is
__device__ __forceinline__ void halve_valid_chunk(const HalveValid<true>& val, const Halve& g, int64_t q) {
  const uint8_t* __restrict__ sval = val.src;
  const int64_t spix = (int64_t)g.H * g.W, dpix = (int64_t)g.H2 * g.W2;
  Chunk ch;
  flat_chunk<uint8_t>(val.vmis, dpix, q, &ch);
  HwcCursorYX u = hwc_cursor_yx(ch.lo() - val.vmis, 1, g.W2);
  const int64_t pt = (int64_t)(2 * u.y) * g.W + 2 * u.x, pb = (int64_t)g.below(u.y) * g.W + 2 * u.x;
  uint8_t b[16];
  if (ch.first == 0 && ch.end == 16 && u.x + 16 <= g.W2 && 2 * (u.x + 15) + 1 < g.W && pb + 32 <= spix) {
    const uint4 av[2] = {load16_any(sval + pt), load16_any(sval + pt + 16)};
    const uint4 cv[2] = {load16_any(sval + pb), load16_any(sval + pb + 16)};
    uint8_t a[32], d[32];
    __builtin_memcpy(a, av, 32);
    __builtin_memcpy(d, cv, 32);
#pragma unroll
    for (int e = 0; e < 16; ++e) b[e] = (uint8_t)((a[2 * e] | a[2 * e + 1] | d[2 * e] | d[2 * e + 1]) != 0);
  } else {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      b[e] = 0;
      if (ch.has(e)) {
        b[e] = halve_flag(sval, g, u.y, u.x);
        u.step(1, g.W2);
      }
    }
  }
  store_chunk<uint8_t>(val.dst, val.vmis, ch.q0, ch.lo(), ch.hi(), b);
}

// T [H][W][C] -> T [H2][W2][C], C in 1 .. 4, the output mis elements behind a 16-byte boundary.  Units [0, nq) are the
// chunks of the output image; with V units [nq, nq + mq) are those of the output validity.
template <typename T, int C, bool V>
__global__ __launch_bounds__(256) void halve_kernel(const T* __restrict__ src, T* __restrict__ dst, Halve g, int mis,
                                                    HalveValid<V> val) {
  constexpr int E = 16 / (int)sizeof(T), NV = 48 / (int)sizeof(T);
  const int rb = g.W2 * C;  // elements of an output row
  const int64_t spix = (int64_t)g.H * g.W, dpix = (int64_t)g.H2 * g.W2;
  const int64_t nq = flat_chunks<T>(mis, dpix * C);
  const uint8_t* sval = nullptr;
  if constexpr (V) sval = val.src;
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t mq = 0;
  if constexpr (V) mq = flat_chunks<uint8_t>(val.vmis, dpix);
  for (int64_t q = tid; q < nq + mq; q += step) {
    Chunk ch;
    if (q >= nq) {
      if constexpr (V) halve_valid_chunk(val, g, q - nq);
      continue;
    }
    flat_chunk<T>(mis, dpix * C, q, &ch);
    HwcCursorYX u = hwc_cursor_yx(ch.lo() - mis, C, g.W2);
    T b[E];
    if (ch.first == 0 && ch.end == E) {  // a whole chunk: the window path where its loads stay inside the source
      const int b0 = u.x * C + u.c, xl = (b0 + E - 1) / C;
      const int64_t pt = (int64_t)(2 * u.y) * g.W + 2 * u.x, pb = (int64_t)g.below(u.y) * g.W + 2 * u.x;
      if (b0 + E <= rb && 2 * xl + 1 < g.W && pb * C + NV <= spix * C && (!V || pb + 32 <= spix)) {
        halve_window_at<T, C, V>(u.c, src + pt * C, src + pb * C, V ? sval + pt : nullptr, V ? sval + pb : nullptr, b);
        store_chunk<T>(dst, mis, ch.q0, ch.lo(), ch.hi(), b);
        continue;
      }
    }
#pragma unroll
    for (int e = 0; e < E; ++e) {
      b[e] = 0;
      if (ch.has(e)) {
        b[e] = halve_at<T, V>(src, sval, g, C, u.y, u.x, u.c);
        u.step(C, g.W2);
      }
    }
    store_chunk<T>(dst, mis, ch.q0, ch.lo(), ch.hi(), b);
  }
}

// The launch of one halving, after the export's own checks, which hold C to 1 .. CMAX.
template <typename T, bool V, int CMAX = 4>
static void launch_halve(const T* src, T* dst, const Halve& g, int C, HalveValid<V> val, hipStream_t st) {
  const int mis = (int)(((uintptr_t)dst & 15) / sizeof(T));
  int64_t units = flat_chunks<T>(mis, (int64_t)g.H2 * g.W2 * C);
  if constexpr (V) units += flat_chunks<uint8_t>(val.vmis, (int64_t)g.H2 * g.W2);
  const dim3 grid(flat_blocks(units));
  if (C == 1) hipLaunchKernelGGL((halve_kernel<T, 1, V>), grid, dim3(256), 0, st, src, dst, g, mis, val);
  if (C == 2) hipLaunchKernelGGL((halve_kernel<T, 2, V>), grid, dim3(256), 0, st, src, dst, g, mis, val);
  if constexpr (CMAX >= 3) {
    if (C == 3) hipLaunchKernelGGL((halve_kernel<T, 3, V>), grid, dim3(256), 0, st, src, dst, g, mis, val);
    if (C == 4) hipLaunchKernelGGL((halve_kernel<T, 4, V>), grid, dim3(256), 0, st, src, dst, g, mis, val);
  }
}

}  // namespace dsic
