// What the render kernels of view.hip and warp.hip share: the display options of one launch and the stretch of a sample
// to a byte.  Output band b takes channel band[b] of the resampled pixel, stretched between lo[b] and hi[b]; a thread
// packs its nb + alpha bytes into one word.
#pragma once
#include "common.h"

namespace dsic {

struct Render {
  int nb, alpha, background, need;
  int band[3];
  uint32_t lo[3], hi[3];
};

__device__ __forceinline__ uint32_t stretch_byte(uint32_t m, uint32_t lo, uint32_t hi) {
  const uint32_t R = hi - lo, d = min(max(m, lo), hi) - lo;
  return R ? (510u * d + R) / (2u * R) : 0u;  // 255 d / R rounded half up; 510 * 65535 + 65535 < 2^32
}

}  // namespace dsic
