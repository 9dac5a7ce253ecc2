// Resampled reads (codec.ImageReader.read with size=(oh, ow)): a region of level 0, given through a window of overview
// level l that covers it, resampled to oh x ow.  One launch; a thread owns one output pixel with all its channels.
//
// The geometry is integer.  On the row axis, scaled by oh, output row i covers [i h, (i+1) h) of the region and source
// row Y (a row of level l, counted in that level's own grid) covers [(Y << l) oh - y0 oh, ((Y+1) << l) oh - y0 oh);
// wy(i, Y) is the length of their intersection, which over Y sums to h.  The rows with wy > 0 are
// (y0 + i h / oh) >> l ... (y0 + ((i+1) h - 1) / oh) >> l (floor divisions), all inside the covering window
// codec.level_window(l, y0, x0, h, w).  Columns likewise with ow, x0 and w.
//
// average, uint8 / uint16 [sh][sw][C]: per channel S = sum wy wx v and T = sum wy wx in 64 bits, output
// (2 S + T) / (2 T): the weighted mean rounded half up, exact.  h w <= 2^46 keeps 2 S + T under 2^64.
// average, float32 [C][sh][sw]: acc = the float32 left fold over Y ascending, then X ascending, of
// float32(wy wx) * v (built with -ffp-contract=off: NumPy folds to the same bits), output acc / float32(T).
// nodata: a source pixel whose C channels all equal the value stays out of S (acc) and T; T = 0 gives the value.
// validity (the _valid exports, a stream with a validity mask): a byte window [sh][sw] beside the source says which
// pixels stay out of S and T (0 = invalid; no value is compared), T = 0 gives the fill and validity 0 in the optional
// output validity [oh][ow], and nearest copies pixel and validity.
// nearest: source row (y0 2 oh + (2 i + 1) h) / (2 oh) >> l = (y0 + (2 i + 1) h / (2 oh)) >> l, columns likewise; a copy.
// render (codec.ImageReader.render, the _render exports): the same pixel, of which chosen channels are stretched to
// bytes between two values per channel, with the validity as alpha; the resampled samples never reach memory.
// index views (codec.ImageReader.render_index, the _index_render exports): the same pixel again, of which one or two
// channels become an index (a band, a difference, a normalised difference) that is stretched to a byte and sent through
// a colour map of 256 entries.
//
// A wave covers 64 consecutive pixels of an output row, so its loads walk the source rows in step and its stores are
// one run of 64 C elements; each source pixel is needed by at most two output rows and two output columns when the
// level fits the scale (codec.view_level), which the caches absorb.
//
// Here: the geometry (View, view_check), the samplers and the kernels.  In render.h, shared with warp.hip: Render and
// stretch_byte, the display check (display_options, display_of), the index tail and its check (index_value, index_stage,
// index_tail, index_options, index_of) and the small host checks.
#include <limits.h>

#include "common.h"
#include "render.h"

namespace dsic {

struct View {
  int sh, sw, sy0, sx0, shift, y0, x0, h, w, oh, ow;
  int hn, hd, wn, wd;  // h / oh and w / ow in lowest terms: the integer kinds' weights (view_reduce)
};

struct Span {
  int a, b;
};

// output index i of n over the region [o, o + len): the first and last source index of level `shift` that it meets
__device__ __forceinline__ Span axis_span(int i, int len, int n, int o, int shift) {
  const int64_t lo = (int64_t)i * len / n, hi = ((int64_t)(i + 1) * len - 1) / n;
  return {(int)((o + lo) >> shift), (int)((o + hi) >> shift)};
}

// the length, scaled by n, that output index i and source index Y share: positive for Y inside axis_span
__device__ __forceinline__ int64_t axis_weight(int i, int len, int n, int o, int shift, int Y) {
  const int64_t a = ((int64_t)Y << shift) * n - (int64_t)o * n, b = a + ((int64_t)n << shift);
  return min(b, (int64_t)(i + 1) * len) - max(a, (int64_t)i * len);
}

__device__ __forceinline__ int axis_nearest(int i, int len, int n, int o, int shift) {
  return (int)((o + (2 * (int64_t)i + 1) * len / (2 * (int64_t)n)) >> shift);
}

constexpr int VIEW_BX = 64, VIEW_BY = 4;  // output pixels of a workgroup: 4 rows of 64

// One output pixel (i, j) of the integer kinds: its C resampled samples into m, and whether anything counted under it.
// T = uint8_t or uint16_t, [.][.][C] with C <= 4; nodata < 0 = none.  The weights are taken with h / oh and w / ow in
// lowest terms: every interval end is a multiple of gcd(h, oh), so this divides all wy by it, S and T alike, and
// (2 S + T) / (2 T) is the same integer while S and T stay small (halving: T = 4).
// V: the validity window sval [sh][sw] (0 = invalid) decides what stays out of S and T instead of a comparison with
// nodata, and the result says whether the pixel is valid (nearest: its source pixel's validity); T = 0 gives nodata
// (the fill) in every channel.  Without V the result is true.
// need: bit c set = channel c is wanted; the others' divisions are skipped and their m is not defined.
template <typename T, bool V>
__device__ __forceinline__ bool resample_pixel(const T* __restrict__ src, const uint8_t* __restrict__ sval, const View& v,
                                               int C, int mode, int nodata, int i, int j, int need, uint32_t m[4]) {
  if (mode == 1) {
    const int Y = axis_nearest(i, v.hn, v.hd, v.y0, v.shift), X = axis_nearest(j, v.wn, v.wd, v.x0, v.shift);
    const T* p = src + ((int64_t)(Y - v.sy0) * v.sw + (X - v.sx0)) * C;
#pragma unroll
    for (int c = 0; c < 4; ++c) m[c] = c < C ? (uint32_t)p[c] : 0u;
    return V ? sval[(int64_t)(Y - v.sy0) * v.sw + (X - v.sx0)] != 0 : true;
  }
  const Span ry = axis_span(i, v.hn, v.hd, v.y0, v.shift), rx = axis_span(j, v.wn, v.wd, v.x0, v.shift);
  uint64_t S[4] = {0, 0, 0, 0}, Tw = 0;
  for (int Y = ry.a; Y <= ry.b; ++Y) {
    const uint64_t wy = (uint64_t)axis_weight(i, v.hn, v.hd, v.y0, v.shift, Y);
    const T* row = src + (int64_t)(Y - v.sy0) * v.sw * C;
    for (int X = rx.a; X <= rx.b; ++X) {
      const uint64_t wgt = wy * (uint64_t)axis_weight(j, v.wn, v.wd, v.x0, v.shift, X);
      const T* p = row + (int64_t)(X - v.sx0) * C;
      uint32_t val[4];
      bool nd = V ? sval[(int64_t)(Y - v.sy0) * v.sw + (X - v.sx0)] == 0 : nodata >= 0;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        val[c] = c < C ? (uint32_t)p[c] : 0u;
        if (!V && c < C) nd = nd && val[c] == (uint32_t)nodata;
      }
      if (nd) continue;
      Tw += wgt;
#pragma unroll
      for (int c = 0; c < 4; ++c) S[c] += wgt * val[c];
    }
  }
  // (2 S + T) / (2 T): in 32 bits where both fit, which reduced weights nearly always allow
  const bool narrow = ((2 * (S[0] | S[1] | S[2] | S[3]) + Tw) >> 32) == 0 && (Tw >> 31) == 0;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    if (c >= C || !((need >> c) & 1)) continue;
    const uint64_t num = 2 * S[c] + Tw, den = 2 * Tw;
    m[c] = !Tw ? (uint32_t)(T)nodata : narrow ? (uint32_t)num / (uint32_t)den : (uint32_t)(num / den);
  }
  return V ? Tw != 0 : true;
}

// The resampled window itself: dst [oh][ow][C] and, with V and oval not null, oval [oh][ow] = 1 or 0.
template <typename T, bool V>
__global__ __launch_bounds__(VIEW_BX * VIEW_BY) void resample_int_kernel(const T* __restrict__ src,
                                                                         T* __restrict__ dst, View v, int C, int mode,
                                                                         int nodata, int bx, int64_t nblocks,
                                                                         const uint8_t* __restrict__ sval,
                                                                         uint8_t* __restrict__ oval) {
  for (int64_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
    const int64_t by = blk / bx;
    const int j = (int)(blk - by * bx) * VIEW_BX + threadIdx.x;
    const int64_t i64 = by * VIEW_BY + threadIdx.y;
    if (i64 >= v.oh || j >= v.ow) continue;
    const int i = (int)i64;
    T* o = dst + ((int64_t)i * v.ow + j) * C;
    uint32_t m[4];
    const bool ok = resample_pixel<T, V>(src, sval, v, C, mode, nodata, i, j, 15, m);
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < C) o[c] = (T)m[c];
    if (V && oval) oval[(int64_t)i * v.ow + j] = (uint8_t)ok;
  }
}

// The rendered window (dsic_window_render_u8 / _u16): resample_pixel, then output band b = channel r.band[b] of it
// stretched to a byte with r.lo[b], r.hi[b], then alpha.  A thread packs its nb + alpha bytes into one word: a wave
// stores one run of 64 (nb + alpha) bytes, a dword per lane where that is 4 bytes at an aligned address.
// Render and stretch_byte: render.h, shared with warp.hip.
template <typename T, bool V>
__global__ __launch_bounds__(VIEW_BX * VIEW_BY) void render_kernel(const T* __restrict__ src,
                                                                   const uint8_t* __restrict__ sval,
                                                                   uint8_t* __restrict__ dst, View v, int C, int mode,
                                                                   int nodata, Render r, int bx, int64_t nblocks) {
  const int n = r.nb + r.alpha;
  const bool dwords = n == 4 && ((uintptr_t)dst & 3) == 0;
  for (int64_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
    const int64_t by = blk / bx;
    const int j = (int)(blk - by * bx) * VIEW_BX + threadIdx.x;
    const int64_t i64 = by * VIEW_BY + threadIdx.y;
    if (i64 >= v.oh || j >= v.ow) continue;
    const int i = (int)i64;
    uint32_t m[4] = {0u, 0u, 0u, 0u};
    const bool ok = resample_pixel<T, V>(src, sval, v, C, mode, nodata, i, j, r.need, m);
    uint32_t word = 0;
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      if (b >= r.nb) continue;
      const int k = r.band[b];
      const uint32_t s = k == 0 ? m[0] : k == 1 ? m[1] : k == 2 ? m[2] : m[3];
      word |= (ok ? stretch_byte(s, r.lo[b], r.hi[b]) : (uint32_t)r.background) << (8 * b);
    }
    if (r.alpha) word |= (ok ? 255u : 0u) << (8 * r.nb);
    uint8_t* o = dst + ((int64_t)i * v.ow + j) * n;
    if (dwords) {
      *(uint32_t*)o = word;
    } else {
      for (int b = 0; b < n; ++b) o[b] = (uint8_t)(word >> (8 * b));
    }
  }
}

// The index view of the window (dsic_window_index_render_u8 / _u16): resample_pixel for the one or two bands of the
// index, then render.h's index tail: the index of the resampled samples, stretched to a byte k, through the colour map
// cm[k], which the workgroup stages in LDS once.  3 + alpha bytes per pixel, stored as render_kernel stores them.
template <typename T, bool V>
__global__ __launch_bounds__(VIEW_BX * VIEW_BY) void index_render_kernel(const T* __restrict__ src,
                                                                         const uint8_t* __restrict__ sval,
                                                                         uint8_t* __restrict__ dst, View v, int C, int mode,
                                                                         int nodata, IndexRender r,
                                                                         const uint8_t* __restrict__ cmap, int bx,
                                                                         int64_t nblocks) {
  __shared__ uint32_t cm[VIEW_BX * VIEW_BY];
  static_assert(VIEW_BX * VIEW_BY == 256, "one colour map entry per thread");
  index_stage(cmap, cm, threadIdx.y * VIEW_BX + threadIdx.x);
  const int n = 3 + r.alpha;
  const bool dwords = n == 4 && ((uintptr_t)dst & 3) == 0;
  for (int64_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
    const int64_t by = blk / bx;
    const int j = (int)(blk - by * bx) * VIEW_BX + threadIdx.x;
    const int64_t i64 = by * VIEW_BY + threadIdx.y;
    if (i64 >= v.oh || j >= v.ow) continue;
    const int i = (int)i64;
    uint32_t m[4] = {0u, 0u, 0u, 0u};
    const bool ok = resample_pixel<T, V>(src, sval, v, C, mode, nodata, i, j, r.need, m);
    index_tail(r, cm, ok, m, dst + ((int64_t)i * v.ow + j) * n, dwords);
  }
}

// float32 [C][.][.], C <= 8
__global__ __launch_bounds__(VIEW_BX * VIEW_BY) void resample_f32_kernel(const float* __restrict__ src,
                                                                         float* __restrict__ dst, View v, int C,
                                                                         int mode, float nodata, int has_nodata, int bx,
                                                                         int64_t nblocks) {
  const int64_t splane = (int64_t)v.sh * v.sw, dplane = (int64_t)v.oh * v.ow;
  for (int64_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
    const int64_t by = blk / bx;
    const int j = (int)(blk - by * bx) * VIEW_BX + threadIdx.x;
    const int64_t i64 = by * VIEW_BY + threadIdx.y;
    if (i64 >= v.oh || j >= v.ow) continue;
    const int i = (int)i64;
    float* o = dst + (int64_t)i * v.ow + j;
    if (mode == 1) {
      const int Y = axis_nearest(i, v.h, v.oh, v.y0, v.shift), X = axis_nearest(j, v.w, v.ow, v.x0, v.shift);
      const float* p = src + (int64_t)(Y - v.sy0) * v.sw + (X - v.sx0);
      for (int c = 0; c < C; ++c) o[c * dplane] = p[c * splane];
      continue;
    }
    const Span ry = axis_span(i, v.h, v.oh, v.y0, v.shift), rx = axis_span(j, v.w, v.ow, v.x0, v.shift);
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int64_t Tw = 0;
    for (int Y = ry.a; Y <= ry.b; ++Y) {
      const int64_t wy = axis_weight(i, v.h, v.oh, v.y0, v.shift, Y);
      const float* row = src + (int64_t)(Y - v.sy0) * v.sw;
      for (int X = rx.a; X <= rx.b; ++X) {
        const int64_t wgt = wy * axis_weight(j, v.w, v.ow, v.x0, v.shift, X);
        const float* p = row + (X - v.sx0);
        float val[8];
        bool nd = has_nodata != 0;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          val[c] = c < C ? p[c * splane] : 0.f;
          if (c < C) nd = nd && val[c] == nodata;
        }
        if (nd) continue;
        Tw += wgt;
        const float wf = (float)wgt;
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[c] = acc[c] + wf * val[c];
      }
    }
    const float tf = (float)Tw;
#pragma unroll
    for (int c = 0; c < 8; ++c)
      if (c < C) o[c * dplane] = Tw ? acc[c] / tf : nodata;
  }
}

// the checks every kind shares; on success the launch shape.  dst holds dch elements of delem bytes per output pixel
static int view_check(const char* what, const void* src, const void* dst, const View& v, int C, int cmin, int cmax,
                      int elem, int delem, int dch, int mode, int* bx, int64_t* nblocks) {
  DSIC_REQUIRE(src && dst, "%s: null pointer", what);
  DSIC_REQUIRE(C >= cmin && C <= cmax, "%s: C=%d must be in %d..%d", what, C, cmin, cmax);
  DSIC_REQUIRE(mode == 0 || mode == 1, "%s: mode=%d (0 average, 1 nearest)", what, mode);
  DSIC_REQUIRE(v.shift >= 0 && v.shift <= 15, "%s: shift=%d must be in 0..15", what, v.shift);
  DSIC_REQUIRE(v.sh >= 1 && v.sw >= 1 && v.sy0 >= 0 && v.sx0 >= 0, "%s: source window %dx%d at (%d, %d)", what, v.sh, v.sw,
               v.sy0, v.sx0);
  DSIC_REQUIRE(v.h >= 1 && v.w >= 1 && v.y0 >= 0 && v.x0 >= 0 && (int64_t)v.y0 + v.h <= INT_MAX &&
                   (int64_t)v.x0 + v.w <= INT_MAX,
               "%s: region %dx%d at (%d, %d)", what, v.h, v.w, v.y0, v.x0);
  DSIC_REQUIRE(v.oh >= 1 && v.ow >= 1, "%s: output %dx%d must be at least 1x1", what, v.oh, v.ow);
  DSIC_REQUIRE((int64_t)v.sh * v.sw <= ((int64_t)1 << 48) && (int64_t)v.oh * v.ow <= ((int64_t)1 << 48),
               "%s: a source window of %dx%d or an output of %dx%d pixels is over 2^48", what, v.sh, v.sw, v.oh, v.ow);
  DSIC_REQUIRE((int64_t)v.h * v.w <= ((int64_t)1 << 46), "%s: a region of %dx%d pixels is over 2^46", what, v.h, v.w);
  const int64_t ya = v.y0 >> v.shift, yb = ((int64_t)v.y0 + v.h - 1) >> v.shift;
  const int64_t xa = v.x0 >> v.shift, xb = ((int64_t)v.x0 + v.w - 1) >> v.shift;
  DSIC_REQUIRE(ya >= v.sy0 && yb < (int64_t)v.sy0 + v.sh && xa >= v.sx0 && xb < (int64_t)v.sx0 + v.sw,
               "%s: the region %dx%d at (%d, %d) covers rows %lld..%lld, columns %lld..%lld of level %d, outside the "
               "source window %dx%d at (%d, %d)",
               what, v.h, v.w, v.y0, v.x0, (long long)ya, (long long)yb, (long long)xa, (long long)xb, v.shift, v.sh,
               v.sw, v.sy0, v.sx0);
  DSIC_REQUIRE(((uintptr_t)src & (uintptr_t)(elem - 1)) == 0 && ((uintptr_t)dst & (uintptr_t)(delem - 1)) == 0,
               "%s: src must be %d-byte aligned and dst %d-byte aligned", what, elem, delem);
  DSIC_REQUIRE(buffers_apart(src, (int64_t)elem * C * v.sh * v.sw, dst, (int64_t)delem * dch * v.oh * v.ow),
               "%s: src and dst overlap", what);
  *bx = (v.ow + VIEW_BX - 1) / VIEW_BX;
  *nblocks = (int64_t)*bx * ((v.oh + VIEW_BY - 1) / VIEW_BY);
  return DSIC_OK;
}

static int view_gcd(int a, int b) {
  while (b) {
    const int t = a % b;
    a = b;
    b = t;
  }
  return a;
}

static View view_of(int sh, int sw, int sy0, int sx0, int shift, int y0, int x0, int h, int w, int oh, int ow) {
  View v = {sh, sw, sy0, sx0, shift, y0, x0, h, w, oh, ow, h, oh, w, ow};
  if (h >= 1 && oh >= 1 && w >= 1 && ow >= 1) {
    const int gy = view_gcd(h, oh), gx = view_gcd(w, ow);
    v.hn = h / gy, v.hd = oh / gy, v.wn = w / gx, v.wd = ow / gx;
  }
  return v;
}

// V: with a validity window; value is then the fill, else nodata (-1 for none)
template <typename T, bool V>
static int resample_int(const char* what, const T* src, const uint8_t* sval, const View& v, int C, int cmin, T* dst,
                        uint8_t* oval, int mode, int value, void* stream) {
  int bx;
  int64_t nblocks;
  const int status = view_check(what, src, dst, v, C, cmin, 4, (int)sizeof(T), (int)sizeof(T), C, mode, &bx, &nblocks);
  if (status != DSIC_OK) return status;
  if (!V) DSIC_REQUIRE(pixel_value<T>(value, -1), "%s: nodata=%d (-1 for none, or a pixel value)", what, value);
  if (V) DSIC_REQUIRE(sval, "%s: null pointer", what);
  if (V) DSIC_REQUIRE(pixel_value<T>(value, 0), "%s: fill=%d must be a pixel value", what, value);
  const int64_t spix = (int64_t)v.sh * v.sw, opix = (int64_t)v.oh * v.ow, px = (int64_t)sizeof(T) * C;
  DSIC_REQUIRE(windows_apart(src, px * spix, sval, spix, dst, px * opix, oval, opix), "%s: src and dst overlap", what);
  hipLaunchKernelGGL((resample_int_kernel<T, V>), launch_grid(nblocks), dim3(VIEW_BX, VIEW_BY), 0, (hipStream_t)stream, src,
                     dst, v, C, mode, value, bx, nblocks, sval, oval);
  return check_launch(what);
}

template <typename T>
static int render(const char* what, const T* src, const uint8_t* sval, const View& v, int C, const int* bands, int nb,
                  const uint32_t* lohi, uint8_t* dst, int mode, int nodata, int alpha, int background, void* stream) {
  int bx;
  int64_t nblocks;
  Render r;
  const int n = nb + alpha;
  int status = display_options(what, nb, alpha, background);
  if (status == DSIC_OK) status = view_check(what, src, dst, v, C, 1, 4, (int)sizeof(T), 1, n, mode, &bx, &nblocks);
  if (status == DSIC_OK) status = display_of<T>(what, C, bands, nb, lohi, nodata, alpha, background, &r);
  if (status != DSIC_OK) return status;
  const int64_t spix = (int64_t)v.sh * v.sw, opix = (int64_t)v.oh * v.ow;
  DSIC_REQUIRE(windows_apart(src, (int64_t)sizeof(T) * C * spix, sval, spix, dst, n * opix, nullptr, 0),
               "%s: src and dst overlap", what);
  if (sval)
    hipLaunchKernelGGL((render_kernel<T, true>), launch_grid(nblocks), dim3(VIEW_BX, VIEW_BY), 0, (hipStream_t)stream, src,
                       sval, dst, v, C, mode, 0, r, bx, nblocks);
  else
    hipLaunchKernelGGL((render_kernel<T, false>), launch_grid(nblocks), dim3(VIEW_BX, VIEW_BY), 0, (hipStream_t)stream, src,
                       sval, dst, v, C, mode, nodata, r, bx, nblocks);
  return check_launch(what);
}

template <typename T>
static int index_render(const char* what, const T* src, const uint8_t* sval, const View& v, int C, int kind, int a, int b,
                        int lo, int hi, const uint8_t* cmap, uint8_t* dst, int mode, int nodata, int alpha, int background,
                        void* stream) {
  int bx;
  int64_t nblocks;
  IndexRender r;
  const int n = 3 + alpha;
  const int64_t spix = (int64_t)v.sh * v.sw, opix = (int64_t)v.oh * v.ow;
  int status = index_options(what, kind, alpha, background);
  if (status == DSIC_OK) status = view_check(what, src, dst, v, C, 1, 4, (int)sizeof(T), 1, n, mode, &bx, &nblocks);
  if (status == DSIC_OK)
    status = index_of<T>(what, C, kind, a, b, lo, hi, cmap, nodata, alpha, background, dst, n * opix, &r);
  if (status != DSIC_OK) return status;
  DSIC_REQUIRE(windows_apart(src, (int64_t)sizeof(T) * C * spix, sval, spix, dst, n * opix, nullptr, 0),
               "%s: src and dst overlap", what);
  if (sval)
    hipLaunchKernelGGL((index_render_kernel<T, true>), launch_grid(nblocks), dim3(VIEW_BX, VIEW_BY), 0, (hipStream_t)stream,
                       src, sval, dst, v, C, mode, 0, r, cmap, bx, nblocks);
  else
    hipLaunchKernelGGL((index_render_kernel<T, false>), launch_grid(nblocks), dim3(VIEW_BX, VIEW_BY), 0, (hipStream_t)stream,
                       src, sval, dst, v, C, mode, nodata, r, cmap, bx, nblocks);
  return check_launch(what);
}

}  // namespace dsic

using namespace dsic;

extern "C" int dsic_window_resample_u8(const uint8_t* src_hwc, int sh, int sw, int sy0, int sx0, int C, int shift, int y0,
                                       int x0, int h, int w, uint8_t* dst_hwc, int oh, int ow, int mode, int nodata,
                                       void* stream) {
  const View v = view_of(sh, sw, sy0, sx0, shift, y0, x0, h, w, oh, ow);
  return resample_int<uint8_t, false>("window_resample_u8", src_hwc, nullptr, v, C, 3, dst_hwc, nullptr, mode, nodata, stream);
}

extern "C" int dsic_window_resample_u16(const uint16_t* src_hwc, int sh, int sw, int sy0, int sx0, int C, int shift,
                                        int y0, int x0, int h, int w, uint16_t* dst_hwc, int oh, int ow, int mode,
                                        int nodata, void* stream) {
  const View v = view_of(sh, sw, sy0, sx0, shift, y0, x0, h, w, oh, ow);
  return resample_int<uint16_t, false>("window_resample_u16", src_hwc, nullptr, v, C, 1, dst_hwc, nullptr, mode, nodata,
                                       stream);
}

extern "C" int dsic_window_resample_f32(const float* src_chw, int sh, int sw, int sy0, int sx0, int C, int shift, int y0,
                                        int x0, int h, int w, float* dst_chw, int oh, int ow, int mode, float nodata,
                                        int has_nodata, void* stream) {
  const View v = view_of(sh, sw, sy0, sx0, shift, y0, x0, h, w, oh, ow);
  int bx;
  int64_t nblocks;
  const int status = view_check("window_resample_f32", src_chw, dst_chw, v, C, 1, 8, 4, 4, C, mode, &bx, &nblocks);
  if (status != DSIC_OK) return status;
  hipLaunchKernelGGL(resample_f32_kernel, launch_grid(nblocks), dim3(VIEW_BX, VIEW_BY), 0, (hipStream_t)stream, src_chw,
                     dst_chw, v, C, mode, nodata, has_nodata, bx, nblocks);
  return check_launch("window_resample_f32");
}

extern "C" int dsic_window_resample_valid_u8(const uint8_t* src_hwc, const uint8_t* src_valid, int sh, int sw, int sy0,
                                             int sx0, int C, int shift, int y0, int x0, int h, int w, uint8_t* dst_hwc,
                                             uint8_t* dst_valid, int oh, int ow, int mode, int fill, void* stream) {
  const View v = view_of(sh, sw, sy0, sx0, shift, y0, x0, h, w, oh, ow);
  return resample_int<uint8_t, true>("window_resample_valid_u8", src_hwc, src_valid, v, C, 3, dst_hwc, dst_valid, mode,
                                     fill, stream);
}

extern "C" int dsic_window_resample_valid_u16(const uint16_t* src_hwc, const uint8_t* src_valid, int sh, int sw, int sy0,
                                              int sx0, int C, int shift, int y0, int x0, int h, int w, uint16_t* dst_hwc,
                                              uint8_t* dst_valid, int oh, int ow, int mode, int fill, void* stream) {
  const View v = view_of(sh, sw, sy0, sx0, shift, y0, x0, h, w, oh, ow);
  return resample_int<uint16_t, true>("window_resample_valid_u16", src_hwc, src_valid, v, C, 1, dst_hwc, dst_valid, mode,
                                      fill, stream);
}

extern "C" int dsic_window_render_u8(const uint8_t* src_hwc, const uint8_t* src_valid, int sh, int sw, int sy0, int sx0,
                                     int C, int shift, int y0, int x0, int h, int w, const int* bands, int nb,
                                     const uint32_t* lohi, uint8_t* dst, int oh, int ow, int mode, int nodata, int alpha,
                                     int background, void* stream) {
  const View v = view_of(sh, sw, sy0, sx0, shift, y0, x0, h, w, oh, ow);
  return render<uint8_t>("window_render_u8", src_hwc, src_valid, v, C, bands, nb, lohi, dst, mode, nodata, alpha,
                         background, stream);
}

extern "C" int dsic_window_render_u16(const uint16_t* src_hwc, const uint8_t* src_valid, int sh, int sw, int sy0, int sx0,
                                      int C, int shift, int y0, int x0, int h, int w, const int* bands, int nb,
                                      const uint32_t* lohi, uint8_t* dst, int oh, int ow, int mode, int nodata, int alpha,
                                      int background, void* stream) {
  const View v = view_of(sh, sw, sy0, sx0, shift, y0, x0, h, w, oh, ow);
  return render<uint16_t>("window_render_u16", src_hwc, src_valid, v, C, bands, nb, lohi, dst, mode, nodata, alpha,
                          background, stream);
}

extern "C" int dsic_window_index_render_u8(const uint8_t* src_hwc, const uint8_t* src_valid, int sh, int sw, int sy0,
                                           int sx0, int C, int shift, int y0, int x0, int h, int w, int kind, int band_a,
                                           int band_b, int lo, int hi, const uint8_t* cmap_dev, uint8_t* dst, int oh, int ow,
                                           int mode, int nodata, int alpha, int background, void* stream) {
  const View v = view_of(sh, sw, sy0, sx0, shift, y0, x0, h, w, oh, ow);
  return index_render<uint8_t>("window_index_render_u8", src_hwc, src_valid, v, C, kind, band_a, band_b, lo, hi, cmap_dev,
                               dst, mode, nodata, alpha, background, stream);
}

extern "C" int dsic_window_index_render_u16(const uint16_t* src_hwc, const uint8_t* src_valid, int sh, int sw, int sy0,
                                            int sx0, int C, int shift, int y0, int x0, int h, int w, int kind, int band_a,
                                            int band_b, int lo, int hi, const uint8_t* cmap_dev, uint8_t* dst, int oh,
                                            int ow, int mode, int nodata, int alpha, int background, void* stream) {
  const View v = view_of(sh, sw, sy0, sx0, shift, y0, x0, h, w, oh, ow);
  return index_render<uint16_t>("window_index_render_u16", src_hwc, src_valid, v, C, kind, band_a, band_b, lo, hi, cmap_dev,
                                dst, mode, nodata, alpha, background, stream);
}
