// Warped reads (codec.ImageReader.read_warped / render_warped): an affine view of level 0, sampled from a window of
// overview level l with nearest, bilinear or Keys cubic interpolation.  One launch; a thread owns one output pixel with
// all its channels.
//
// The geometry is integer.  m[6] is the 2 x 3 matrix in (row, column) order in Q16, level-0 pixels per output pixel.
// Output pixel (i, j) samples the level-0 position P / 2^17 with
//   Py = m00 (2 i + 1) + m01 (2 j + 1) + 2 m02,   Px = m10 (2 i + 1) + m11 (2 j + 1) + 2 m12
// and is inside iff 0 <= Py < H 2^17 and 0 <= Px < W 2^17; an outside pixel is fill and invalid.  At level l (LH x LW):
//   nearest (mode 1): pixel (min(Py >> (17 + l), LH - 1), min(Px >> (17 + l), LW - 1)), a copy of pixel and validity.
//   q = P - 2^(16+l) (centre-aligned), Y0 = q >> (17 + l), phase p = (q >> (10 + l)) & 127, taps clamped to the level.
//   bilinear (mode 0): taps Y0, Y0 + 1 with weights (128 - p, p) per axis; S = sum wy wx v and T = sum wy wx over the
//     taps that count, output (2 S + T) / (2 T); T = 0 gives fill and invalid.  T <= 2^14: 32 bits hold 2 S + T.
//   cubic (mode 2): Keys a = -1/2, taps Y0 - 1 ... Y0 + 2, integer weights scaled by 2^22 per axis (cubic_weights; they
//     sum to 2^22).  If all 16 clamped taps count the output is clamp((S + 2^43) >> 44, 0, top) with S in int64
//     (sum |wy wx| <= 1.5625 2^44, so |S| < 2^61); otherwise the pixel is the bilinear one.
// A tap counts iff its validity byte is not 0 (src_valid), else iff its channels do not all equal nodata (nodata >= 0),
// else always.
//
// A workgroup is 16 x 16 output pixels and each of its four waves owns an 8 x 8 patch: whatever the angle, the patch's
// taps lie in a box of about 12 x 12 level pixels, a dozen cache lines, where 64 pixels of one output row walk up to 45
// source rows at 45 degrees, one line each (DESIGN.md section 3 has the count).  A lane row of the patch stores 8 C
// contiguous elements.  Taps are also clamped to the source window, so a wrong plan cannot read outside the allocation.
//
// Here: the geometry (Warp, warp_check, warp_axis), the sampler and the kernels.  In render.h, shared with view.hip:
// Render and stretch_byte, the display check (display_options, display_of), the index tail and its check (index_value,
// index_stage, index_tail, index_options, index_of) and the small host checks.
#include <limits.h>

#include "common.h"
#include "render.h"

namespace dsic {

struct Warp {
  int sh, sw, sy0, sx0, shift, LH, LW, oh, ow;
  int64_t HP, WP;  // H 2^17 and W 2^17: the inside test
  int64_t m[6];
};

constexpr int WARP_TILE = 16, WARP_PATCH = 8;  // output pixels of a workgroup (16 x 16) and of a wave (8 x 8)
constexpr int64_t WARP_COEF = (int64_t)1 << 26, WARP_SHIFT = (int64_t)1 << 47;
constexpr int WARP_SIDE = 1 << 20;

// the index inside the source window of level index Y, clamped to the level and then to the window
__device__ __forceinline__ int warp_tap(int Y, int L, int s0, int sn) { return min(max(min(max(Y, 0), L - 1) - s0, 0), sn - 1); }

// Keys a = -1/2 at phase p / 128, scaled by 2 * 128^3 = 2^22
__device__ __forceinline__ void cubic_weights(int p, int w[4]) {
  const int p2 = p * p, p3 = p2 * p;
  w[0] = -p3 + 256 * p2 - 16384 * p;
  w[1] = 3 * p3 - 640 * p2 + (1 << 22);
  w[2] = -3 * p3 + 512 * p2 + 16384 * p;
  w[3] = p3 - 128 * p2;
}

// the tap at (yw, xw) of the window: its channels into v, and whether it counts
template <typename T, bool V>
__device__ __forceinline__ bool warp_load(const T* __restrict__ src, const uint8_t* __restrict__ sval, const Warp& g, int C,
                                          int nodata, int yw, int xw, uint32_t v[4]) {
  const int64_t at = (int64_t)yw * g.sw + xw;
  const T* p = src + at * C;
#pragma unroll
  for (int c = 0; c < 4; ++c) v[c] = c < C ? (uint32_t)p[c] : 0u;
  if (V) return sval[at] != 0;
  bool nd = nodata >= 0;
#pragma unroll
  for (int c = 0; c < 4; ++c)
    if (c < C) nd = nd && v[c] == (uint32_t)nodata;
  return !nd;
}

// One output pixel (i, j): its C samples into out (channels from C on: 0), and whether it is valid.  T = uint8_t or
// uint16_t, [.][.][C] with C <= 4; V: a validity window beside the source; nodata < 0 = none.
template <typename T, bool V>
__device__ __forceinline__ bool warp_pixel(const T* __restrict__ src, const uint8_t* __restrict__ sval, const Warp& g, int C,
                                           int mode, int nodata, uint32_t fill, int i, int j, uint32_t out[4]) {
  const int64_t Py = g.m[0] * (2 * i + 1) + g.m[1] * (2 * j + 1) + 2 * g.m[2];
  const int64_t Px = g.m[3] * (2 * i + 1) + g.m[4] * (2 * j + 1) + 2 * g.m[5];
#pragma unroll
  for (int c = 0; c < 4; ++c) out[c] = c < C ? fill : 0u;
  if (Py < 0 || Py >= g.HP || Px < 0 || Px >= g.WP) return false;
  const int l = g.shift;
  if (mode == 1) {
    const int yw = warp_tap((int)(Py >> (17 + l)), g.LH, g.sy0, g.sh), xw = warp_tap((int)(Px >> (17 + l)), g.LW, g.sx0, g.sw);
    const T* p = src + ((int64_t)yw * g.sw + xw) * C;
#pragma unroll
    for (int c = 0; c < 4; ++c) out[c] = c < C ? (uint32_t)p[c] : 0u;
    return V ? sval[(int64_t)yw * g.sw + xw] != 0 : true;
  }
  const int64_t qy = Py - ((int64_t)1 << (16 + l)), qx = Px - ((int64_t)1 << (16 + l));
  const int Y0 = (int)(qy >> (17 + l)), X0 = (int)(qx >> (17 + l));
  const int py = (int)(qy >> (10 + l)) & 127, px = (int)(qx >> (10 + l)) & 127;
  uint32_t Sb[4] = {0u, 0u, 0u, 0u}, Tb = 0u;  // the bilinear sums over the taps that count
  const uint32_t by[2] = {128u - (uint32_t)py, (uint32_t)py}, bx[2] = {128u - (uint32_t)px, (uint32_t)px};
  if (mode == 0) {
    const int xw[2] = {warp_tap(X0, g.LW, g.sx0, g.sw), warp_tap(X0 + 1, g.LW, g.sx0, g.sw)};
#pragma unroll
    for (int ky = 0; ky < 2; ++ky) {
      const int yw = warp_tap(Y0 + ky, g.LH, g.sy0, g.sh);
#pragma unroll
      for (int kx = 0; kx < 2; ++kx) {
        uint32_t v[4];
        if (!warp_load<T, V>(src, sval, g, C, nodata, yw, xw[kx], v)) continue;
        const uint32_t wgt = by[ky] * bx[kx];
        Tb += wgt;
#pragma unroll
        for (int c = 0; c < 4; ++c) Sb[c] += wgt * v[c];
      }
    }
  } else {
    int wy[4], wx[4], xw[4];
    cubic_weights(py, wy);
    cubic_weights(px, wx);
#pragma unroll
    for (int k = 0; k < 4; ++k) xw[k] = warp_tap(X0 - 1 + k, g.LW, g.sx0, g.sw);
    int64_t S[4] = {0, 0, 0, 0};
    bool all = true;
#pragma unroll
    for (int ky = 0; ky < 4; ++ky) {
      const int yw = warp_tap(Y0 - 1 + ky, g.LH, g.sy0, g.sh);
      int64_t row[4] = {0, 0, 0, 0};
#pragma unroll
      for (int kx = 0; kx < 4; ++kx) {
        uint32_t v[4];
        const bool counts = warp_load<T, V>(src, sval, g, C, nodata, yw, xw[kx], v);
        all = all && counts;
#pragma unroll
        for (int c = 0; c < 4; ++c) row[c] += (int64_t)wx[kx] * (int64_t)(int)v[c];
        if (ky >= 1 && ky <= 2 && kx >= 1 && kx <= 2 && counts) {  // the bilinear taps among the sixteen
          const uint32_t wgt = by[ky - 1] * bx[kx - 1];
          Tb += wgt;
#pragma unroll
          for (int c = 0; c < 4; ++c) Sb[c] += wgt * v[c];
        }
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) S[c] += (int64_t)wy[ky] * row[c];
    }
    if (all) {
      const int64_t top = (int64_t)(T)~(T)0;
#pragma unroll
      for (int c = 0; c < 4; ++c)
        out[c] = c < C ? (uint32_t)min(max((S[c] + ((int64_t)1 << 43)) >> 44, (int64_t)0), top) : 0u;
      return true;
    }
  }
  if (!Tb) return false;
#pragma unroll
  for (int c = 0; c < 4; ++c) out[c] = c < C ? (2u * Sb[c] + Tb) / (2u * Tb) : 0u;
  return true;
}

// output pixel of thread t of block blk: wave t / 64 owns patch (t / 128, (t / 64) % 2), lane t % 64 its pixel
// ((t % 64) / 8, t % 8)
__device__ __forceinline__ bool warp_where(const Warp& g, int64_t blk, int bx, int* i, int* j) {
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int64_t by = blk / bx;
  const int64_t i64 = by * WARP_TILE + (wave >> 1) * WARP_PATCH + (lane >> 3);
  const int64_t j64 = (blk - by * bx) * WARP_TILE + (wave & 1) * WARP_PATCH + (lane & 7);
  *i = (int)i64, *j = (int)j64;
  return i64 < g.oh && j64 < g.ow;
}

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

// One axis of the host check: the level indices that the taps of all inside samples can take, from the positions of the
// four corner pixels (P is affine in (i, j), the floor monotone).  false: no sample is inside on this axis.
static bool warp_axis(const int64_t* m, int oh, int ow, int64_t NP, int L, int l, int mode, int64_t* a, int64_t* b) {
  int64_t lo = INT64_MAX, hi = INT64_MIN;
  for (int k = 0; k < 4; ++k) {
    const int64_t i = (k & 1) ? oh - 1 : 0, j = (k & 2) ? ow - 1 : 0;
    const int64_t P = m[0] * (2 * i + 1) + m[1] * (2 * j + 1) + 2 * m[2];
    lo = P < lo ? P : lo, hi = P > hi ? P : hi;
  }
  if (hi < 0 || lo >= NP) return false;
  lo = lo < 0 ? 0 : lo, hi = hi >= NP ? NP - 1 : hi;
  if (mode == 1) {
    *a = lo >> (17 + l), *b = hi >> (17 + l);  // arithmetic shifts: floors
  } else {
    const int64_t half = (int64_t)1 << (16 + l);
    const int before = mode == 2 ? 1 : 0, after = mode == 2 ? 2 : 1;
    *a = ((lo - half) >> (17 + l)) - before, *b = ((hi - half) >> (17 + l)) + after;
  }
  *a = *a < 0 ? 0 : *a > L - 1 ? L - 1 : *a;
  *b = *b < 0 ? 0 : *b > L - 1 ? L - 1 : *b;
  return true;
}

// the checks both kinds share; on success the launch shape.  dst holds dch elements of delem bytes per output pixel
static int warp_check(const char* what, const void* src, const uint8_t* sval, const void* dst, const uint8_t* oval,
                      const Warp& g, int H, int W, const int64_t* m, int C, int cmin, int elem, int delem, int dch,
                      int mode, int* bx, int64_t* nblocks) {
  DSIC_REQUIRE(src && dst && m, "%s: null pointer", what);
  DSIC_REQUIRE(C >= cmin && C <= 4, "%s: C=%d must be in %d..4", what, C, cmin);
  DSIC_REQUIRE(mode >= 0 && mode <= 2, "%s: mode=%d (0 bilinear, 1 nearest, 2 cubic)", what, mode);
  DSIC_REQUIRE(g.shift >= 0 && g.shift <= 15, "%s: shift=%d must be in 0..15", what, g.shift);
  DSIC_REQUIRE(H >= 1 && W >= 1 && H <= (1 << 30) && W <= (1 << 30), "%s: image %dx%d", what, H, W);
  DSIC_REQUIRE(g.LH == (int)(((int64_t)H + ((int64_t)1 << g.shift) - 1) >> g.shift) &&
                   g.LW == (int)(((int64_t)W + ((int64_t)1 << g.shift) - 1) >> g.shift),
               "%s: level %d of a %dx%d image is not %dx%d", what, g.shift, H, W, g.LH, g.LW);
  DSIC_REQUIRE(g.sh >= 1 && g.sw >= 1 && g.sy0 >= 0 && g.sx0 >= 0 && (int64_t)g.sy0 + g.sh <= g.LH &&
                   (int64_t)g.sx0 + g.sw <= g.LW,
               "%s: source window %dx%d at (%d, %d) of a %dx%d level", what, g.sh, g.sw, g.sy0, g.sx0, g.LH, g.LW);
  DSIC_REQUIRE(g.oh >= 1 && g.ow >= 1 && g.oh <= WARP_SIDE && g.ow <= WARP_SIDE, "%s: output %dx%d must be 1x1 .. 2^20x2^20",
               what, g.oh, g.ow);
  for (int k = 0; k < 6; ++k) {
    const int64_t bound = k % 3 == 2 ? WARP_SHIFT - 1 : WARP_COEF;
    DSIC_REQUIRE(m[k] >= -bound && m[k] <= bound, "%s: matrix entry %d = %lld is outside +-%lld (Q16)", what, k,
                 (long long)m[k], (long long)bound);
  }
  int64_t ya = 0, yb = 0, xa = 0, xb = 0;
  if (warp_axis(m, g.oh, g.ow, g.HP, g.LH, g.shift, mode, &ya, &yb) &&
      warp_axis(m + 3, g.oh, g.ow, g.WP, g.LW, g.shift, mode, &xa, &xb))
    DSIC_REQUIRE(ya >= g.sy0 && yb < (int64_t)g.sy0 + g.sh && xa >= g.sx0 && xb < (int64_t)g.sx0 + g.sw,
                 "%s: the view's taps cover rows %lld..%lld, columns %lld..%lld of level %d, outside the source window "
                 "%dx%d at (%d, %d)",
                 what, (long long)ya, (long long)yb, (long long)xa, (long long)xb, g.shift, g.sh, g.sw, g.sy0, g.sx0);
  DSIC_REQUIRE(((uintptr_t)src & (uintptr_t)(elem - 1)) == 0 && ((uintptr_t)dst & (uintptr_t)(delem - 1)) == 0,
               "%s: src must be %d-byte aligned and dst %d-byte aligned", what, elem, delem);
  const int64_t spix = (int64_t)g.sh * g.sw, opix = (int64_t)g.oh * g.ow;
  DSIC_REQUIRE(windows_apart(src, elem * C * spix, sval, spix, dst, delem * dch * opix, oval, opix),
               "%s: src and dst overlap", what);
  *bx = (g.ow + WARP_TILE - 1) / WARP_TILE;
  *nblocks = (int64_t)*bx * ((g.oh + WARP_TILE - 1) / WARP_TILE);
  return DSIC_OK;
}

static Warp warp_of(int sh, int sw, int sy0, int sx0, int shift, int LH, int LW, int H, int W, const int64_t* m, int oh,
                    int ow) {
  Warp g = {sh, sw, sy0, sx0, shift, LH, LW, oh, ow, (int64_t)H * 131072, (int64_t)W * 131072, {0, 0, 0, 0, 0, 0}};
  for (int k = 0; m && k < 6; ++k) g.m[k] = m[k];
  return g;
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
