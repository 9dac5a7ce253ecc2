// What view.hip (resampled windows) and warp.hip (affine views) share; geometry, samplers and kernels stay in those files.
//   device: the display options of a launch (Render) and the stretch of a sample to a byte.  Both render kernels hold
//     the same display tail, written out: output band b takes channel band[b] of the sampled pixel, stretched between
//     lo[b] and hi[b]; an invalid pixel is background; alpha follows the validity; a thread packs its nb + alpha bytes
//     into one word.  As a shared function it costs render_kernel 0.7 to 1 % on a whole level ("Viewing path").
//   device, index views: the index of a sampled pixel (index_value: band, difference, normalised difference, as the
//     unsigned u = v - vmin; include/dsic_hip.h has the table), the colour map staged in LDS (index_stage) and the index
//     tail (index_tail: u stretched to a byte k, the output bands cmap[k], background and alpha as above).  Only the index
//     kernels of view.hip and warp.hip hold it; histogram.hip counts index_value.
//   host: the display check in two parts (display_options before the geometry check, display_of after it), likewise the
//     index check (index_options, index_of), pixel_value (the range of nodata and fill), windows_apart (overlap, over the
//     optional validity buffers) and launch_grid.
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

// ---- index views ----
constexpr int INDEX_BAND = 0, INDEX_DIFFERENCE = 1, INDEX_ND = 2;  // DSIC_INDEX_* of include/dsic_hip.h
constexpr int INDEX_SCALE = 10000, INDEX_ND_BINS = 2 * INDEX_SCALE + 1;

struct IndexRender {
  int kind, a, b, alpha, background, need;  // b = a for a band; need as Render's
  uint32_t top, lo, hi;                     // the stretch pair in u units: lo - vmin, hi - vmin
};

// the index of a pixel with the samples A and B as u = v - vmin, and whether it is defined
__device__ __forceinline__ bool index_value(int kind, uint32_t A, uint32_t B, uint32_t top, uint32_t* u) {
  if (kind == INDEX_ND) {
    const uint32_t s = A + B;
    *u = s ? (40000u * A + s) / (2u * s) : 0u;  // 10000 (A - B) / s + 10000 rounded half up; 40000 * 65535 + 131070 < 2^32
    return s != 0;
  }
  *u = kind == INDEX_DIFFERENCE ? A - B + top : A;
  return true;
}

// the colour map uint8 [256][3] into cm[256], one packed word per entry; t: the thread's number in a workgroup of 256
__device__ __forceinline__ void index_stage(const uint8_t* __restrict__ cmap, uint32_t* cm, int t) {
  cm[t] = (uint32_t)cmap[3 * t] | (uint32_t)cmap[3 * t + 1] << 8 | (uint32_t)cmap[3 * t + 2] << 16;
  __syncthreads();
}

// The index tail: the sampled pixel m (valid: ok) to its 3 + alpha bytes at o.  510 * 131070 + 131070 < 2^32.
__device__ __forceinline__ void index_tail(const IndexRender& r, const uint32_t* cm, bool ok, const uint32_t m[4],
                                           uint8_t* o, bool dwords) {
  const uint32_t A = r.a == 0 ? m[0] : r.a == 1 ? m[1] : r.a == 2 ? m[2] : m[3];
  const uint32_t B = r.b == 0 ? m[0] : r.b == 1 ? m[1] : r.b == 2 ? m[2] : m[3];
  uint32_t u;
  ok = index_value(r.kind, A, B, r.top, &u) && ok;
  uint32_t word = ok ? cm[stretch_byte(u, r.lo, r.hi)] : (uint32_t)r.background * 0x010101u;
  if (r.alpha && ok) word |= 0xFF000000u;
  if (dwords) {
    *(uint32_t*)o = word;
  } else {
    for (int b = 0; b < 3 + r.alpha; ++b) o[b] = (uint8_t)(word >> (8 * b));
  }
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

// The index check, first part: what is refused before the geometry is looked at.
inline int index_options(const char* what, int kind, int alpha, int background) {
  DSIC_REQUIRE(kind >= INDEX_BAND && kind <= INDEX_ND, "%s: kind=%d (0 band, 1 difference, 2 nd)", what, kind);
  DSIC_REQUIRE(alpha == 0 || alpha == 1, "%s: alpha=%d (0 or 1)", what, alpha);
  DSIC_REQUIRE(background >= 0 && background <= 255, "%s: background=%d must be in 0..255", what, background);
  return DSIC_OK;
}

// the least and the largest index value v of a kind over elements with the largest value top
inline void index_range(int kind, int top, int* vmin, int* vmax) {
  *vmin = kind == INDEX_BAND ? 0 : kind == INDEX_DIFFERENCE ? -top : -INDEX_SCALE;
  *vmax = kind == INDEX_ND ? INDEX_SCALE : top;
}

// The bands of an index over C channels (C is in 1..4): b is ignored for a band.
inline int index_bands(const char* what, int C, int kind, int a, int b) {
  DSIC_REQUIRE(a >= 0 && a < C, "%s: band %d is outside 0..%d", what, a, C - 1);
  DSIC_REQUIRE(kind == INDEX_BAND || (b >= 0 && b < C), "%s: band %d is outside 0..%d", what, b, C - 1);
  return DSIC_OK;
}

// The index check, second part, after the geometry check: the options of a launch over elements of T that writes
// dbytes bytes at dst.
template <typename T>
inline int index_of(const char* what, int C, int kind, int a, int b, int lo, int hi, const uint8_t* cmap, int nodata,
                    int alpha, int background, const void* dst, int64_t dbytes, IndexRender* r) {
  DSIC_REQUIRE(cmap, "%s: null pointer", what);
  const int top = (int)(T)~(T)0;
  DSIC_REQUIRE(pixel_value<T>(nodata, -1), "%s: nodata=%d (-1 for none, or a pixel value)", what, nodata);
  const int status = index_bands(what, C, kind, a, b);
  if (status != DSIC_OK) return status;
  int vmin, vmax;
  index_range(kind, top, &vmin, &vmax);
  DSIC_REQUIRE(vmin <= lo && lo <= hi && hi <= vmax, "%s: stretch pair (%d, %d) must have %d <= lo <= hi <= %d", what, lo, hi,
               vmin, vmax);
  DSIC_REQUIRE(buffers_apart(cmap, 768, dst, dbytes), "%s: cmap and dst overlap", what);
  if (kind == INDEX_BAND) b = a;
  *r = {kind, a, b, alpha, background, (1 << a) | (1 << b), (uint32_t)top, (uint32_t)(lo - vmin), (uint32_t)(hi - vmin)};
  return DSIC_OK;
}

}  // namespace dsic
