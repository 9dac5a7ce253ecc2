// The affine sampler, shared by warp.hip (one scene per launch), warp_composite.hip (up to 16 scenes per launch) and
// grid.hip (one scene under a coordinate mesh).
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
// else always.  Taps are also clamped to the source window, so a wrong plan cannot read outside the allocation.
//
// Here: the geometry (Warp, warp_of), the sampler (warp_tap, cubic_weights, warp_load, warp_sample_at: the sample at a
// position; warp_pixel: the affine position of (i, j), then that sample), the work split (warp_where) and the part of
// the host check that looks at one scene's geometry (warp_frame, warp_axis_taps, warp_axis, warp_holds, warp_geometry).
// grid.hip samples the same way at positions interpolated from a mesh.
#pragma once
#include <limits.h>

#include "common.h"

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

// The sample at the level-0 position (Py, Px) / 2^17: its C values into out (channels from C on: 0), and whether it is
// valid.  T = uint8_t or uint16_t, [.][.][C] with C <= 4; V: a validity window beside the source; nodata < 0 = none.
// Whoever states where output pixel (i, j) samples calls it: warp_pixel below (an affine), grid.hip (a mesh).
template <typename T, bool V>
__device__ __forceinline__ bool warp_sample_at(const T* __restrict__ src, const uint8_t* __restrict__ sval, const Warp& g,
                                               int C, int mode, int nodata, uint32_t fill, int64_t Py, int64_t Px,
                                               uint32_t out[4]) {
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

// One output pixel (i, j) of the affine view g.m: its position, then the sample there.
template <typename T, bool V>
__device__ __forceinline__ bool warp_pixel(const T* __restrict__ src, const uint8_t* __restrict__ sval, const Warp& g, int C,
                                           int mode, int nodata, uint32_t fill, int i, int j, uint32_t out[4]) {
  const int64_t Py = g.m[0] * (2 * i + 1) + g.m[1] * (2 * j + 1) + 2 * g.m[2];
  const int64_t Px = g.m[3] * (2 * i + 1) + g.m[4] * (2 * j + 1) + 2 * g.m[5];
  return warp_sample_at<T, V>(src, sval, g, C, mode, nodata, fill, Py, Px, out);
}

// output pixel of thread t of block blk of an oh x ow output: wave t / 64 owns patch (t / 128, (t / 64) % 2), lane
// t % 64 its pixel ((t % 64) / 8, t % 8)
__device__ __forceinline__ bool warp_where(int oh, int ow, int64_t blk, int bx, int* i, int* j) {
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int64_t by = blk / bx;
  const int64_t i64 = by * WARP_TILE + (wave >> 1) * WARP_PATCH + (lane >> 3);
  const int64_t j64 = (blk - by * bx) * WARP_TILE + (wave & 1) * WARP_PATCH + (lane & 7);
  *i = (int)i64, *j = (int)j64;
  return i64 < oh && j64 < ow;
}

__device__ __forceinline__ bool warp_where(const Warp& g, int64_t blk, int bx, int* i, int* j) {
  return warp_where(g.oh, g.ow, blk, bx, i, j);
}

// One axis of the host check: the level indices a .. b that the taps of all inside samples can take when the positions
// (Q17) lie in lo .. hi: cut to the image, widened by the mode's taps, clamped to the level.  false: no sample is inside
// on this axis.  warp_axis (an affine) and grid.hip (a mesh) find lo and hi.
static bool warp_axis_taps(int64_t lo, int64_t hi, int64_t NP, int L, int l, int mode, int64_t* a, int64_t* b) {
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

// The same from the positions of the four corner pixels of an affine view: P is affine in (i, j), the floor monotone.
static bool warp_axis(const int64_t* m, int oh, int ow, int64_t NP, int L, int l, int mode, int64_t* a, int64_t* b) {
  int64_t lo = INT64_MAX, hi = INT64_MIN;
  for (int k = 0; k < 4; ++k) {
    const int64_t i = (k & 1) ? oh - 1 : 0, j = (k & 2) ? ow - 1 : 0;
    const int64_t P = m[0] * (2 * i + 1) + m[1] * (2 * j + 1) + 2 * m[2];
    lo = P < lo ? P : lo, hi = P > hi ? P : hi;
  }
  return warp_axis_taps(lo, hi, NP, L, l, mode, a, b);
}

// The frame of one scene under a view of g.oh x g.ow pixels: the level, the source window and the output size.
static int warp_frame(const char* what, const Warp& g, int H, int W) {
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
  return DSIC_OK;
}

// The words for a source window that does not hold the taps ya .. yb, xa .. xb.
static int warp_holds(const char* what, const Warp& g, int64_t ya, int64_t yb, int64_t xa, int64_t xb) {
  DSIC_REQUIRE(ya >= g.sy0 && yb < (int64_t)g.sy0 + g.sh && xa >= g.sx0 && xb < (int64_t)g.sx0 + g.sw,
               "%s: the view's taps cover rows %lld..%lld, columns %lld..%lld of level %d, outside the source window "
               "%dx%d at (%d, %d)",
               what, (long long)ya, (long long)yb, (long long)xa, (long long)xb, g.shift, g.sh, g.sw, g.sy0, g.sx0);
  return DSIC_OK;
}

// The geometry of one scene under an affine view sampled with `mode` (in 0..2): the frame, the matrix, and that the
// window holds every tap.  warp_check and the composite's per-source check both run it, so both refuse the same things
// in the same words.
static int warp_geometry(const char* what, const Warp& g, int H, int W, const int64_t* m, int mode) {
  const int status = warp_frame(what, g, H, W);
  if (status != DSIC_OK) return status;
  for (int k = 0; k < 6; ++k) {
    const int64_t bound = k % 3 == 2 ? WARP_SHIFT - 1 : WARP_COEF;
    DSIC_REQUIRE(m[k] >= -bound && m[k] <= bound, "%s: matrix entry %d = %lld is outside +-%lld (Q16)", what, k,
                 (long long)m[k], (long long)bound);
  }
  int64_t ya = 0, yb = 0, xa = 0, xb = 0;
  if (warp_axis(m, g.oh, g.ow, g.HP, g.LH, g.shift, mode, &ya, &yb) &&
      warp_axis(m + 3, g.oh, g.ow, g.WP, g.LW, g.shift, mode, &xa, &xb))
    return warp_holds(what, g, ya, yb, xa, xb);
  return DSIC_OK;
}

static Warp warp_of(int sh, int sw, int sy0, int sx0, int shift, int LH, int LW, int H, int W, const int64_t* m, int oh,
                    int ow) {
  Warp g = {sh, sw, sy0, sx0, shift, LH, LW, oh, ow, (int64_t)H * 131072, (int64_t)W * 131072, {0, 0, 0, 0, 0, 0}};
  for (int k = 0; m && k < 6; ++k) g.m[k] = m[k];
  return g;
}

}  // namespace dsic
