// Warped reads (codec.ImageReader.read_warped / render_warped): an affine view of level 0, sampled from a window of
// overview level l with nearest, bilinear or Keys cubic interpolation.  One launch; a thread owns one output pixel with
// all its channels.  warp_sample.h states the integer geometry and holds the sampler, which warp_composite.hip shares.
//
// A workgroup is 16 x 16 output pixels and each of its four waves owns an 8 x 8 patch: whatever the angle, the patch's
// taps lie in a box of about 12 x 12 level pixels, a dozen cache lines, where 64 pixels of one output row walk up to 45
// source rows at 45 degrees, one line each (DESIGN.md section 3 has the count).  A lane row of the patch stores 8 C
// contiguous elements.  Taps are also clamped to the source window, so a wrong plan cannot read outside the allocation.
//
// Here: the kernels and the check of a launch (warp_check).  In warp_sample.h: the geometry (Warp, warp_geometry,
// warp_axis) and the sampler.  In render.h, shared with view.hip: Render and stretch_byte, the display check
// (display_options, display_of), the index tail and its check (index_value, index_stage, index_tail, index_options,
// index_of) and the small host checks.
#include "common.h"
#include "render.h"
#include "warp_sample.h"

namespace dsic {

// The warped window itself: dst [oh][ow][C] and, with oval not null, oval [oh][ow] = 1 or 0.
template <typename T, bool V>
__global__ __launch_bounds__(WARP_TILE * WARP_TILE) void warp_kernel(const T* __restrict__ src,
                                                                     const uint8_t* __restrict__ sval, T* __restrict__ dst,
                                                                     uint8_t* __restrict__ oval, Warp g, int C, int mode,
                                                                     int nodata, int fill, int bx, int64_t nblocks) {
  for (int64_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
    int i, j;
    if (!warp_where(g, blk, bx, &i, &j)) continue;
    uint32_t m[4];
    const bool ok = warp_pixel<T, V>(src, sval, g, C, mode, nodata, (uint32_t)fill, i, j, m);
    T* o = dst + ((int64_t)i * g.ow + j) * C;
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < C) o[c] = (T)m[c];
    if (oval) oval[(int64_t)i * g.ow + j] = (uint8_t)ok;
  }
}

// The rendered warped window: warp_pixel, then the band choice, stretch, alpha and background of view.hip's
// render_kernel; an invalid pixel (outside the image, or nothing counting under it) is background with alpha 0.
template <typename T, bool V>
__global__ __launch_bounds__(WARP_TILE * WARP_TILE) void warp_render_kernel(const T* __restrict__ src,
                                                                            const uint8_t* __restrict__ sval,
                                                                            uint8_t* __restrict__ dst, Warp g, int C,
                                                                            int mode, int nodata, Render r, int bx,
                                                                            int64_t nblocks) {
  const int n = r.nb + r.alpha;
  const bool dwords = n == 4 && ((uintptr_t)dst & 3) == 0;
  for (int64_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
    int i, j;
    if (!warp_where(g, blk, bx, &i, &j)) continue;
    uint32_t m[4];
    const bool ok = warp_pixel<T, V>(src, sval, g, C, mode, nodata, 0u, i, j, m);
    uint32_t word = 0;
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      if (b >= r.nb) continue;
      const int k = r.band[b];
      const uint32_t s = k == 0 ? m[0] : k == 1 ? m[1] : k == 2 ? m[2] : m[3];
      word |= (ok ? stretch_byte(s, r.lo[b], r.hi[b]) : (uint32_t)r.background) << (8 * b);
    }
    if (r.alpha) word |= (ok ? 255u : 0u) << (8 * r.nb);
    uint8_t* o = dst + ((int64_t)i * g.ow + j) * n;
    if (dwords) {
      *(uint32_t*)o = word;
    } else {
      for (int b = 0; b < n; ++b) o[b] = (uint8_t)(word >> (8 * b));
    }
  }
}

// The index view of the warped window (dsic_window_warp_index_render_u8 / _u16): warp_pixel, then render.h's index
// tail with the colour map staged in LDS, as view.hip's index_render_kernel.
template <typename T, bool V>
__global__ __launch_bounds__(WARP_TILE * WARP_TILE) void warp_index_render_kernel(const T* __restrict__ src,
                                                                                  const uint8_t* __restrict__ sval,
                                                                                  uint8_t* __restrict__ dst, Warp g, int C,
                                                                                  int mode, int nodata, IndexRender r,
                                                                                  const uint8_t* __restrict__ cmap, int bx,
                                                                                  int64_t nblocks) {
  __shared__ uint32_t cm[WARP_TILE * WARP_TILE];
  static_assert(WARP_TILE * WARP_TILE == 256, "one colour map entry per thread");
  index_stage(cmap, cm, threadIdx.x);
  const int n = 3 + r.alpha;
  const bool dwords = n == 4 && ((uintptr_t)dst & 3) == 0;
  for (int64_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
    int i, j;
    if (!warp_where(g, blk, bx, &i, &j)) continue;
    uint32_t m[4];
    const bool ok = warp_pixel<T, V>(src, sval, g, C, mode, nodata, 0u, i, j, m);
    index_tail(r, cm, ok, m, dst + ((int64_t)i * g.ow + j) * n, dwords);
  }
}

// the checks both kinds share; on success the launch shape.  dst holds dch elements of delem bytes per output pixel
static int warp_check(const char* what, const void* src, const uint8_t* sval, const void* dst, const uint8_t* oval,
                      const Warp& g, int H, int W, const int64_t* m, int C, int cmin, int elem, int delem, int dch,
                      int mode, int* bx, int64_t* nblocks) {
  DSIC_REQUIRE(src && dst && m, "%s: null pointer", what);
  DSIC_REQUIRE(C >= cmin && C <= 4, "%s: C=%d must be in %d..4", what, C, cmin);
  DSIC_REQUIRE(mode >= 0 && mode <= 2, "%s: mode=%d (0 bilinear, 1 nearest, 2 cubic)", what, mode);
  const int status = warp_geometry(what, g, H, W, m, mode);
  if (status != DSIC_OK) return status;
  DSIC_REQUIRE(((uintptr_t)src & (uintptr_t)(elem - 1)) == 0 && ((uintptr_t)dst & (uintptr_t)(delem - 1)) == 0,
               "%s: src must be %d-byte aligned and dst %d-byte aligned", what, elem, delem);
  const int64_t spix = (int64_t)g.sh * g.sw, opix = (int64_t)g.oh * g.ow;
  DSIC_REQUIRE(windows_apart(src, elem * C * spix, sval, spix, dst, delem * dch * opix, oval, opix),
               "%s: src and dst overlap", what);
  *bx = (g.ow + WARP_TILE - 1) / WARP_TILE;
  *nblocks = (int64_t)*bx * ((g.oh + WARP_TILE - 1) / WARP_TILE);
  return DSIC_OK;
}

template <typename T>
static int warp(const char* what, const T* src, const uint8_t* sval, const Warp& g, int H, int W, const int64_t* m, int C,
                int cmin, T* dst, uint8_t* oval, int mode, int nodata, int fill, void* stream) {
  int bx;
  int64_t nblocks;
  const int status = warp_check(what, src, sval, dst, oval, g, H, W, m, C, cmin, (int)sizeof(T), (int)sizeof(T), C, mode,
                                &bx, &nblocks);
  if (status != DSIC_OK) return status;
  DSIC_REQUIRE(pixel_value<T>(nodata, -1), "%s: nodata=%d (-1 for none, or a pixel value)", what, nodata);
  DSIC_REQUIRE(pixel_value<T>(fill, 0), "%s: fill=%d must be a pixel value", what, fill);
  if (sval)
    hipLaunchKernelGGL((warp_kernel<T, true>), launch_grid(nblocks), dim3(WARP_TILE * WARP_TILE), 0, (hipStream_t)stream, src,
                       sval, dst, oval, g, C, mode, -1, fill, bx, nblocks);
  else
    hipLaunchKernelGGL((warp_kernel<T, false>), launch_grid(nblocks), dim3(WARP_TILE * WARP_TILE), 0, (hipStream_t)stream, src,
                       sval, dst, oval, g, C, mode, nodata, fill, bx, nblocks);
  return check_launch(what);
}

template <typename T>
static int warp_render(const char* what, const T* src, const uint8_t* sval, const Warp& g, int H, int W, const int64_t* m,
                       int C, const int* bands, int nb, const uint32_t* lohi, uint8_t* dst, int mode, int nodata, int alpha,
                       int background, void* stream) {
  int bx;
  int64_t nblocks;
  Render r;
  int status = display_options(what, nb, alpha, background);
  if (status == DSIC_OK)
    status = warp_check(what, src, sval, dst, nullptr, g, H, W, m, C, 1, (int)sizeof(T), 1, nb + alpha, mode, &bx, &nblocks);
  if (status == DSIC_OK) status = display_of<T>(what, C, bands, nb, lohi, nodata, alpha, background, &r);
  if (status != DSIC_OK) return status;
  if (sval)
    hipLaunchKernelGGL((warp_render_kernel<T, true>), launch_grid(nblocks), dim3(WARP_TILE * WARP_TILE), 0,
                       (hipStream_t)stream, src, sval, dst, g, C, mode, -1, r, bx, nblocks);
  else
    hipLaunchKernelGGL((warp_render_kernel<T, false>), launch_grid(nblocks), dim3(WARP_TILE * WARP_TILE), 0,
                       (hipStream_t)stream, src, sval, dst, g, C, mode, nodata, r, bx, nblocks);
  return check_launch(what);
}

template <typename T>
static int warp_index_render(const char* what, const T* src, const uint8_t* sval, const Warp& g, int H, int W,
                             const int64_t* m, int C, int kind, int a, int b, int lo, int hi, const uint8_t* cmap,
                             uint8_t* dst, int mode, int nodata, int alpha, int background, void* stream) {
  int bx;
  int64_t nblocks;
  IndexRender r;
  const int n = 3 + alpha;
  int status = index_options(what, kind, alpha, background);
  if (status == DSIC_OK)
    status = warp_check(what, src, sval, dst, nullptr, g, H, W, m, C, 1, (int)sizeof(T), 1, n, mode, &bx, &nblocks);
  if (status == DSIC_OK)
    status = index_of<T>(what, C, kind, a, b, lo, hi, cmap, nodata, alpha, background, dst, (int64_t)n * g.oh * g.ow, &r);
  if (status != DSIC_OK) return status;
  if (sval)
    hipLaunchKernelGGL((warp_index_render_kernel<T, true>), launch_grid(nblocks), dim3(WARP_TILE * WARP_TILE), 0,
                       (hipStream_t)stream, src, sval, dst, g, C, mode, -1, r, cmap, bx, nblocks);
  else
    hipLaunchKernelGGL((warp_index_render_kernel<T, false>), launch_grid(nblocks), dim3(WARP_TILE * WARP_TILE), 0,
                       (hipStream_t)stream, src, sval, dst, g, C, mode, nodata, r, cmap, bx, nblocks);
  return check_launch(what);
}

}  // namespace dsic

using namespace dsic;

extern "C" int dsic_window_warp_u8(const uint8_t* src_hwc, const uint8_t* src_valid, int sh, int sw, int sy0, int sx0,
                                   int C, int shift, int LH, int LW, int H, int W, const int64_t* m, uint8_t* dst_hwc,
                                   uint8_t* dst_valid, int oh, int ow, int mode, int nodata, int fill, void* stream) {
  const Warp g = warp_of(sh, sw, sy0, sx0, shift, LH, LW, H, W, m, oh, ow);
  return warp<uint8_t>("window_warp_u8", src_hwc, src_valid, g, H, W, m, C, 3, dst_hwc, dst_valid, mode, nodata, fill,
                       stream);
}

extern "C" int dsic_window_warp_u16(const uint16_t* src_hwc, const uint8_t* src_valid, int sh, int sw, int sy0, int sx0,
                                    int C, int shift, int LH, int LW, int H, int W, const int64_t* m, uint16_t* dst_hwc,
                                    uint8_t* dst_valid, int oh, int ow, int mode, int nodata, int fill, void* stream) {
  const Warp g = warp_of(sh, sw, sy0, sx0, shift, LH, LW, H, W, m, oh, ow);
  return warp<uint16_t>("window_warp_u16", src_hwc, src_valid, g, H, W, m, C, 1, dst_hwc, dst_valid, mode, nodata, fill,
                        stream);
}

extern "C" int dsic_window_warp_render_u8(const uint8_t* src_hwc, const uint8_t* src_valid, int sh, int sw, int sy0,
                                          int sx0, int C, int shift, int LH, int LW, int H, int W, const int64_t* m,
                                          const int* bands, int nb, const uint32_t* lohi, uint8_t* dst, int oh, int ow,
                                          int mode, int nodata, int alpha, int background, void* stream) {
  const Warp g = warp_of(sh, sw, sy0, sx0, shift, LH, LW, H, W, m, oh, ow);
  return warp_render<uint8_t>("window_warp_render_u8", src_hwc, src_valid, g, H, W, m, C, bands, nb, lohi, dst, mode, nodata,
                              alpha, background, stream);
}

extern "C" int dsic_window_warp_render_u16(const uint16_t* src_hwc, const uint8_t* src_valid, int sh, int sw, int sy0,
                                           int sx0, int C, int shift, int LH, int LW, int H, int W, const int64_t* m,
                                           const int* bands, int nb, const uint32_t* lohi, uint8_t* dst, int oh, int ow,
                                           int mode, int nodata, int alpha, int background, void* stream) {
  const Warp g = warp_of(sh, sw, sy0, sx0, shift, LH, LW, H, W, m, oh, ow);
  return warp_render<uint16_t>("window_warp_render_u16", src_hwc, src_valid, g, H, W, m, C, bands, nb, lohi, dst, mode,
                               nodata, alpha, background, stream);
}

extern "C" int dsic_window_warp_index_render_u8(const uint8_t* src_hwc, const uint8_t* src_valid, int sh, int sw, int sy0,
                                                int sx0, int C, int shift, int LH, int LW, int H, int W, const int64_t* m,
                                                int kind, int band_a, int band_b, int lo, int hi, const uint8_t* cmap_dev,
                                                uint8_t* dst, int oh, int ow, int mode, int nodata, int alpha,
                                                int background, void* stream) {
  const Warp g = warp_of(sh, sw, sy0, sx0, shift, LH, LW, H, W, m, oh, ow);
  return warp_index_render<uint8_t>("window_warp_index_render_u8", src_hwc, src_valid, g, H, W, m, C, kind, band_a, band_b,
                                    lo, hi, cmap_dev, dst, mode, nodata, alpha, background, stream);
}

extern "C" int dsic_window_warp_index_render_u16(const uint16_t* src_hwc, const uint8_t* src_valid, int sh, int sw, int sy0,
                                                 int sx0, int C, int shift, int LH, int LW, int H, int W, const int64_t* m,
                                                 int kind, int band_a, int band_b, int lo, int hi, const uint8_t* cmap_dev,
                                                 uint8_t* dst, int oh, int ow, int mode, int nodata, int alpha,
                                                 int background, void* stream) {
  const Warp g = warp_of(sh, sw, sy0, sx0, shift, LH, LW, H, W, m, oh, ow);
  return warp_index_render<uint16_t>("window_warp_index_render_u16", src_hwc, src_valid, g, H, W, m, C, kind, band_a, band_b,
                                     lo, hi, cmap_dev, dst, mode, nodata, alpha, background, stream);
}
