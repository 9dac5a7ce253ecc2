// The chunk walk of the HWC byte movers (image_codec.hip, image_u16.hip, mask.hip, halve.h), stated once over the
// element type T (uint8_t or uint16_t; float for the one-channel rows of mask.hip's float32 window, whose base is
// 16-byte aligned, mis = 0).  An output is written as aligned 16-byte chunks of E = 16 / sizeof(T) elements,
// one thread per chunk.  The output may begin `mis` elements behind a 16-byte boundary: positions then count elements
// shifted by mis, so that position q0, a multiple of E, is an aligned 16 bytes of memory at img + (q0 - mis).  A chunk
// that lies whole inside its row segment (or flat array) is one dwordx4 store; a ragged chunk at either end is element
// stores of its own elements only, as its neighbours belong to another thread, another tile or a guard.
#pragma once
#include "common.h"

namespace dsic {

// chunk [q0, q0 + E) and the part [lo, hi) of it that lies inside the segment; the part is kept as the elements
// [first, end) of the chunk, 0 <= first < end <= E
struct Chunk {
  int64_t q0;
  int first, end;
  __host__ __device__ int64_t lo() const { return q0 + first; }
  __host__ __device__ int64_t hi() const { return q0 + end; }
  __host__ __device__ bool has(int e) const { return e >= first && e < end; }  // element q0 + e
};

// Chunk k of the row segment of `seg` elements whose first element is b0 (shifted by mis already); false where the
// segment has no such chunk.  A segment touches at most seg / E + 2 chunks.
template <typename T>
__host__ __device__ inline bool row_chunk(int64_t b0, int64_t seg, int64_t k, Chunk* ch) {
  constexpr int E = 16 / (int)sizeof(T);
  const int64_t q0 = (b0 / E + k) * E, b1 = b0 + seg;
  ch->q0 = q0, ch->first = q0 > b0 ? 0 : (int)(b0 - q0), ch->end = q0 + E < b1 ? E : (int)(b1 - q0);
  return q0 < b1;
}

// chunk q of a flat array of n elements that begins mis < E elements behind a 16-byte boundary
template <typename T>
__host__ __device__ inline bool flat_chunk(int mis, int64_t n, int64_t q, Chunk* ch) {
  return row_chunk<T>(mis, n, q, ch);
}
template <typename T>
__host__ __device__ inline int64_t flat_chunks(int mis, int64_t n) {
  constexpr int E = 16 / (int)sizeof(T);
  return (n + mis + E - 1) / E;
}

// (pixel, channel) of element e of a run of C-channel pixels, and the step to the next element
struct HwcCursor {
  int64_t px;
  int c;
  __host__ __device__ void step(int C) {
    if (++c == C) c = 0, ++px;
  }
};
__host__ __device__ inline HwcCursor hwc_cursor(int64_t e, int C) {
  const int64_t px = e / C;
  return {px, (int)(e - px * C)};
}

// the same for a flat image of W-pixel rows: the pixel as (y, x), the step carries from x into y
struct HwcCursorYX {
  int y, x, c;
  __host__ __device__ void step(int C, int W) {
    if (++c == C) {
      c = 0;
      if (++x == W) x = 0, ++y;
    }
  }
};
__host__ __device__ inline HwcCursorYX hwc_cursor_yx(int64_t e, int C, int W) {
  const int rb = W * C;  // elements of a row, under 2^31: one 64-bit division, the rest in 32 bits
  const int y = (int)(e / rb), r = (int)(e - (int64_t)y * rb), x = r / C;
  return {y, x, r - x * C};
}

// elements [lo, hi) of chunk q0 from b[0 .. E): b[e - q0] is element e
template <typename T>
__device__ __forceinline__ void store_chunk(T* __restrict__ img, int mis, int64_t q0, int64_t lo, int64_t hi,
                                            const T* b) {
  constexpr int E = 16 / (int)sizeof(T);
  if (lo == q0 && hi == q0 + E) {
    uint4 v;
    __builtin_memcpy(&v, b, 16);
    *(uint4*)(img + (q0 - mis)) = v;
  } else {
    for (int64_t e = lo; e < hi; ++e) img[e - mis] = b[e - q0];
  }
}

}  // namespace dsic
