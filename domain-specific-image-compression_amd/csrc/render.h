// What view.hip (resampled windows) and warp.hip (affine views) share; geometry, samplers and kernels stay in those files.
//   device: the display options of a launch (Render) and the stretch of a sample to a byte.  Both render kernels hold
//     the same display tail, written out: output band b takes channel band[b] of the sampled pixel, stretched between
//     lo[b] and hi[b]; an invalid pixel is background; alpha follows the validity; a thread packs its nb + alpha bytes
//     into one word.  As a shared function it costs render_kernel 0.7 to 1 % on a whole level ("Viewing path").
//   host: the display check in two parts (display_options before the geometry check, display_of after it), pixel_value
//     (the range of nodata and fill), windows_apart (overlap, over the optional validity buffers) and launch_grid.
#pragma once
#include "common.h"

namespace dsic {

struct Render {
  int nb, alpha, background, need;  // need: bit c set = channel c of the sampled pixel is used
  int band[3];
  uint32_t lo[3], hi[3];
};

__device__ __forceinline__ uint32_t stretch_byte(uint32_t m, uint32_t lo, uint32_t hi) {
  const uint32_t R = hi - lo, d = min(max(m, lo), hi) - lo;
  return R ? (510u * d + R) / (2u * R) : 0u;  // 255 d / R rounded half up; 510 * 65535 + 65535 < 2^32
}

inline dim3 launch_grid(int64_t nblocks) { return dim3((unsigned)(nblocks > (1 << 20) ? (1 << 20) : nblocks)); }

// whether v is a pixel value of T, or, with lowest = -1, the -1 that stands for none
template <typename T>
inline bool pixel_value(int v, int lowest) { return v >= lowest && v <= (int)(T)~(T)0; }

// whether the outputs dst and oval lie apart from the inputs src and sval and from each other; sval and oval may be null
inline bool windows_apart(const void* src, int64_t sb, const void* sval, int64_t svb, const void* dst, int64_t db,
                          const void* oval, int64_t ovb) {
  const auto apart = [](const void* a, int64_t ab, const void* b, int64_t bb) {
    return !a || !b || buffers_apart(a, ab, b, bb);
  };
  return apart(src, sb, dst, db) && apart(sval, svb, dst, db) && apart(oval, ovb, src, sb) &&
         apart(oval, ovb, sval, svb) && apart(oval, ovb, dst, db);
}

// The display check, first part: what is refused before the geometry is looked at.
inline int display_options(const char* what, int nb, int alpha, int background) {
  DSIC_REQUIRE(nb == 1 || nb == 3, "%s: nb=%d output bands (1 or 3)", what, nb);
  DSIC_REQUIRE(alpha == 0 || alpha == 1, "%s: alpha=%d (0 or 1)", what, alpha);
  DSIC_REQUIRE(background >= 0 && background <= 255, "%s: background=%d must be in 0..255", what, background);
  return DSIC_OK;
}

// The display check, second part, after the geometry check (C is in 1..4): the options of a launch over elements of T.
template <typename T>
inline int display_of(const char* what, int C, const int* bands, int nb, const uint32_t* lohi, int nodata, int alpha,
                      int background, Render* r) {
  DSIC_REQUIRE(bands && lohi, "%s: null pointer", what);
  const int top = (int)(T)~(T)0;
  DSIC_REQUIRE(pixel_value<T>(nodata, -1), "%s: nodata=%d (-1 for none, or a pixel value)", what, nodata);
  for (int c = 0; c < C; ++c)
    DSIC_REQUIRE(lohi[2 * c] <= lohi[2 * c + 1] && lohi[2 * c + 1] <= (uint32_t)top,
                 "%s: stretch pair (%u, %u) of band %d must have 0 <= lo <= hi <= %d", what, lohi[2 * c], lohi[2 * c + 1], c,
                 top);
  *r = {nb, alpha, background, 0, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  for (int b = 0; b < nb; ++b) {
    DSIC_REQUIRE(bands[b] >= 0 && bands[b] < C, "%s: band %d is outside 0..%d", what, bands[b], C - 1);
    r->band[b] = bands[b], r->lo[b] = lohi[2 * bands[b]], r->hi[b] = lohi[2 * bands[b] + 1];
    r->need |= 1 << bands[b];
  }
  return DSIC_OK;
}

}  // namespace dsic
