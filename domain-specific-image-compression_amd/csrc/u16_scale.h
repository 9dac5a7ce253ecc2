// The per-band scale of a uint16 image (codec.py, kind 2) as the kernels of image_u16.hip and residual_u16.hip see
// it: the pairs (lo, R = hi - lo) by value, norm and denorm, the run loader for uint16 at any 2-byte alignment, and
// the argument checks the uint16 exports share.
#pragma once
#include <limits.h>

#include "common.h"

namespace dsic {

struct Scale {
  uint32_t lo[4], R[4];
};

__device__ __forceinline__ uint32_t pick(const uint32_t (&a)[4], int c) {
  return c == 0 ? a[0] : (c == 1 ? a[1] : (c == 2 ? a[2] : a[3]));
}

__device__ __forceinline__ float norm_u16(uint32_t v, uint32_t lo, uint32_t R) {
  v = min(max(v, lo), lo + R) - lo;
  return R ? __fdiv_rn((float)v, (float)R) : 0.f;
}

__device__ __forceinline__ uint16_t denorm_u16(float x, uint32_t lo, uint32_t R) {
  x = x > 0.f ? (x > 1.f ? 1.f : x) : 0.f;  // clamp(x, 0, 1); a NaN becomes 0
  return (uint16_t)(lo + (uint32_t)__fadd_rn(__fmul_rn(x, (float)R), 0.5f));
}

// 2 ND uint16 from any 2-byte aligned address.  Off a dword boundary the dwords read are those that hold the run's
// first and last value, so no dword outside the allocation is touched.
template <int ND>
__device__ __forceinline__ void load_run(const uint16_t* p, uint16_t* out) {
  uint32_t d[ND];
  const uintptr_t a = (uintptr_t)p;
  if ((a & 3) == 0) {
    if (ND % 4 == 0 && (a & 15) == 0) {
#pragma unroll
      for (int k = 0; k < ND / 4; ++k) {
        const uint4 v = ((const uint4*)p)[k];
        d[4 * k] = v.x, d[4 * k + 1] = v.y, d[4 * k + 2] = v.z, d[4 * k + 3] = v.w;
      }
    } else if ((a & 7) == 0) {  // ND is even
#pragma unroll
      for (int k = 0; k < ND / 2; ++k) {
        const uint2 v = ((const uint2*)p)[k];
        d[2 * k] = v.x, d[2 * k + 1] = v.y;
      }
    } else {
#pragma unroll
      for (int k = 0; k < ND; ++k) d[k] = ((const uint32_t*)p)[k];
    }
  } else {
    const uint32_t* w = (const uint32_t*)(a - 2);
    uint32_t prev = w[0];
#pragma unroll
    for (int k = 0; k < ND; ++k) {
      const uint32_t next = w[k + 1];
      d[k] = __builtin_amdgcn_alignbyte(next, prev, 2);
      prev = next;
    }
  }
  __builtin_memcpy(out, d, 4 * ND);
}

// the host's 2 C words (lo0, hi0, ...) as the kernels take them; nullptr where they are no scale
static const char* scale_error(const uint32_t* lohi, int C, Scale* s) {
  for (int c = 0; c < 4; ++c) s->lo[c] = s->R[c] = 0;
  for (int c = 0; c < C; ++c) {
    if (lohi[2 * c + 1] > 65535u) return "hi must be at most 65535";
    if (lohi[2 * c] > lohi[2 * c + 1]) return "lo must not exceed hi";
    s->lo[c] = lohi[2 * c], s->R[c] = lohi[2 * c + 1] - lohi[2 * c];
  }
  return nullptr;
}

}  // namespace dsic

// `what` is a string, not only a literal
#define DSIC_U16_COMMON(what, img)                                                                                  \
  DSIC_REQUIRE(C >= 1 && C <= 4, "%s: C=%d must be in 1..4", what, C);                                              \
  DSIC_REQUIRE(((uintptr_t)(img) & 1) == 0, "%s: the uint16 image must be 2-byte aligned", what)
#define DSIC_U16_SCALE(what)                                                          \
  Scale sc;                                                                           \
  const char* se = scale_error(lohi, C, &sc);                                         \
  DSIC_REQUIRE(!se, "%s: scale: %s", what, se ? se : "")
#define DSIC_U16_ROW(what, W)                                                                                         \
  DSIC_REQUIRE((int64_t)(W) * C * 2 <= INT_MAX, "%s: a row of W=%d pixels of C=%d uint16 is over 2^31 - 1 bytes", \
               what, (W), C)
#define DSIC_U16_BY_C(kernel, ...)                                                    \
  switch (C) {                                                                        \
    case 1: hipLaunchKernelGGL(kernel<1>, __VA_ARGS__); break;                        \
    case 2: hipLaunchKernelGGL(kernel<2>, __VA_ARGS__); break;                        \
    case 3: hipLaunchKernelGGL(kernel<3>, __VA_ARGS__); break;                        \
    default: hipLaunchKernelGGL(kernel<4>, __VA_ARGS__); break;                       \
  }
