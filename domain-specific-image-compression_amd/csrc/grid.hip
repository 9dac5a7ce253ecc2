// Gridded reads (codec.ImageReader.read_gridded / render_gridded / render_index_gridded): a view of level 0 whose sample
// positions come from a coordinate mesh, the way raster tools reproject: the exact transform at the nodes of a coarse
// mesh of output positions, bilinear interpolation between them, then warp.hip's sampler at the interpolated position.
//
// The mesh G is int64 [nh + 1][nw + 1][2], nh = ceil(oh / S), nw = ceil(ow / S), S = 2^s in {16, 32, 64}: node (a, b)
// holds the level-0 position (y, x) in Q16 of the output corner (a S, b S), |value| < 2^48, or GRID_NONE = -2^63 in its y
// entry: no position here.  Output pixel (i, j) lies in cell (a, b) = (i >> s, j >> s) at the odd offsets
// fu = 2 (i - a S) + 1, fv = 2 (j - b S) + 1 of 2 S, and per axis its position in Q17 is
//   P = ((2S - fu)(2S - fv) G[a][b] + (2S - fu) fv G[a][b+1] + fu (2S - fv) G[a+1][b] + fu fv G[a+1][b+1]) >> (2 s + 1),
// an arithmetic shift.  The weights sum to 2^(2s+2) <= 2^14, so the sum stays under 2^62.  Rearranged,
//   4 S^2 G00 + 2S fu (G10 - G00) + 2S fv (G01 - G00) + fu fv (G00 - G10 - G01 + G11)
// is the same integer; its terms can pass 2^63, so it is formed in uint64_t, where they wrap and the sum does not.  For
// G[a][b] = m0 a S + m1 b S + m2 it is m0 (2 i + 1) + m1 (2 j + 1) + 2 m2: an affine mesh gives warp.hip's position and
// hence its pixel, bit for bit.  A cell with a GRID_NONE node is fill and invalid throughout.  Everything after P - the
// inside test, the level, the taps, the masks, the fill - is warp_sample.h's warp_sample_at.
//
// The work split is warp.hip's (warp_where): a workgroup is 16 x 16 output pixels, and S is a multiple of 16, so a
// workgroup lies inside one cell.  Its four nodes, the none test and the cell's coefficients are therefore the same for
// every thread: the nodes come by scalar loads straight from the mesh (no LDS staging), and with fu = fu0 + tu,
// fv = fv0 + tv (fu0, fv0 the workgroup's, tu and tv twice the thread's row and column in it) the sum is
//   K0 + tu K1 + tv K2 + tu tv K3
// with four coefficients per axis formed once per block iteration in scalar registers (grid_cell).  A thread pays three
// multiplies of a 64-bit coefficient by a number under 1024 per axis, where the affine kernel pays two by 2 i + 1.
//
// Here: the cell's coefficients, the three kernels (mirrors of warp.hip's) and the check of a call (grid_check).  The
// host copy of the mesh is what the check reads; the kernels read the device copy.  Taps are clamped to the source
// window, so a device copy that differs cannot make a kernel read outside the allocation.
#include "common.h"
#include "render.h"
#include "warp_sample.h"

namespace dsic {

constexpr int64_t GRID_NONE = INT64_MIN, GRID_BOUND = (int64_t)1 << 48, GRID_NODES = (int64_t)1 << 22;

struct Mesh {
  int nw1, s;  // nodes per mesh row, log2 of the step
};

// The coefficients of the cell that block `blk` lies in, k[axis][0..3] (axis 0: y); false if one of its nodes is none.
// Everything here depends on the block alone.
__device__ __forceinline__ bool grid_cell(const int64_t* __restrict__ nodes, const Mesh& q, int64_t blk, int bx,
                                          uint64_t k[2][4]) {
  const int64_t by = blk / bx;
  const int64_t i0 = by * WARP_TILE, j0 = (blk - by * bx) * WARP_TILE;
  const int64_t a = i0 >> q.s, b = j0 >> q.s;
  const int64_t* __restrict__ n0 = nodes + (a * q.nw1 + b) * 2;
  const int64_t* __restrict__ n1 = n0 + (int64_t)q.nw1 * 2;
  // all eight entries first, two runs of 32 contiguous bytes, and a test without short circuits: one wait for the
  // scalar loads per block, where a test that loads as it goes waits for up to four in a row
  const int64_t g0[4] = {n0[0], n0[1], n0[2], n0[3]}, g1[4] = {n1[0], n1[1], n1[2], n1[3]};
  const bool none = (g0[0] == GRID_NONE) | (g0[2] == GRID_NONE) | (g1[0] == GRID_NONE) | (g1[2] == GRID_NONE);
  const uint64_t fu = (uint64_t)(2 * (i0 - (a << q.s)) + 1), fv = (uint64_t)(2 * (j0 - (b << q.s)) + 1);
#pragma unroll
  for (int x = 0; x < 2; ++x) {
    const uint64_t G00 = (uint64_t)g0[x], G01 = (uint64_t)g0[2 + x], G10 = (uint64_t)g1[x], G11 = (uint64_t)g1[2 + x];
    const uint64_t B = (G10 - G00) << (q.s + 1), Cc = (G01 - G00) << (q.s + 1), D = G00 - G10 - G01 + G11;
    k[x][0] = (G00 << (2 * q.s + 2)) + B * fu + Cc * fv + D * fu * fv;
    k[x][1] = B + D * fv;
    k[x][2] = Cc + D * fu;
    k[x][3] = D;
  }
  return !none;
}

// the position (Q17) on one axis of the thread at row tu / 2, column tv / 2 of its workgroup
__device__ __forceinline__ int64_t grid_position(const uint64_t k[4], uint32_t tu, uint32_t tv, int s) {
  return (int64_t)(k[0] + tu * k[1] + tv * k[2] + (uint64_t)(tu * tv) * k[3]) >> (2 * s + 1);
}

// One output pixel (i, j) of a block whose cell is whole (k) or not: as warp_pixel.
template <typename T, bool V>
__device__ __forceinline__ bool grid_pixel(const T* __restrict__ src, const uint8_t* __restrict__ sval, const Warp& g, int C,
                                           int mode, int nodata, uint32_t fill, bool whole, const uint64_t k[2][4], int s,
                                           int i, int j, uint32_t out[4]) {
  if (!whole) {
#pragma unroll
    for (int c = 0; c < 4; ++c) out[c] = c < C ? fill : 0u;
    return false;
  }
  const uint32_t tu = 2u * (uint32_t)(i & (WARP_TILE - 1)), tv = 2u * (uint32_t)(j & (WARP_TILE - 1));
  return warp_sample_at<T, V>(src, sval, g, C, mode, nodata, fill, grid_position(k[0], tu, tv, s),
                              grid_position(k[1], tu, tv, s), out);
}

// The gridded window itself: dst [oh][ow][C] and, with oval not null, oval [oh][ow] = 1 or 0.
template <typename T, bool V>
__global__ __launch_bounds__(WARP_TILE * WARP_TILE) void grid_kernel(const T* __restrict__ src,
                                                                     const uint8_t* __restrict__ sval, T* __restrict__ dst,
                                                                     uint8_t* __restrict__ oval, Warp g,
    const int64_t* __restrict__ nodes, Mesh q, int C,
                                                                     int mode, int nodata, int fill, int bx,
                                                                     int64_t nblocks) {
  for (int64_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
    uint64_t k[2][4];
    const bool whole = grid_cell(nodes, q, blk, bx, k);
    int i, j;
    if (!warp_where(g, blk, bx, &i, &j)) continue;
    uint32_t m[4];
    const bool ok = grid_pixel<T, V>(src, sval, g, C, mode, nodata, (uint32_t)fill, whole, k, q.s, i, j, m);
    T* o = dst + ((int64_t)i * g.ow + j) * C;
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < C) o[c] = (T)m[c];
    if (oval) oval[(int64_t)i * g.ow + j] = (uint8_t)ok;
  }
}

// The rendered gridded window: grid_pixel, then the display tail of warp.hip's warp_render_kernel, written out as there.
template <typename T, bool V>
__global__ __launch_bounds__(WARP_TILE * WARP_TILE) void grid_render_kernel(const T* __restrict__ src,
                                                                            const uint8_t* __restrict__ sval,
                                                                            uint8_t* __restrict__ dst, Warp g,
    const int64_t* __restrict__ nodes, Mesh q, int C,
                                                                            int mode, int nodata, Render r, int bx,
                                                                            int64_t nblocks) {
  const int n = r.nb + r.alpha;
  const bool dwords = n == 4 && ((uintptr_t)dst & 3) == 0;
  for (int64_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
    uint64_t k[2][4];
    const bool whole = grid_cell(nodes, q, blk, bx, k);
    int i, j;
    if (!warp_where(g, blk, bx, &i, &j)) continue;
    uint32_t m[4];
    const bool ok = grid_pixel<T, V>(src, sval, g, C, mode, nodata, 0u, whole, k, q.s, i, j, m);
    uint32_t word = 0;
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      if (b >= r.nb) continue;
      const int ch = r.band[b];
      const uint32_t s = ch == 0 ? m[0] : ch == 1 ? m[1] : ch == 2 ? m[2] : m[3];
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

// The index view of the gridded window: grid_pixel, then render.h's index tail with the colour map staged in LDS.
template <typename T, bool V>
__global__ __launch_bounds__(WARP_TILE * WARP_TILE) void grid_index_render_kernel(const T* __restrict__ src,
                                                                                  const uint8_t* __restrict__ sval,
                                                                                  uint8_t* __restrict__ dst, Warp g,
    const int64_t* __restrict__ nodes, Mesh q,
                                                                                  int C, int mode, int nodata, IndexRender r,
                                                                                  const uint8_t* __restrict__ cmap, int bx,
                                                                                  int64_t nblocks) {
  __shared__ uint32_t cm[WARP_TILE * WARP_TILE];
  static_assert(WARP_TILE * WARP_TILE == 256, "one colour map entry per thread");
  index_stage(cmap, cm, threadIdx.x);
  const int n = 3 + r.alpha;
  const bool dwords = n == 4 && ((uintptr_t)dst & 3) == 0;
  for (int64_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
    uint64_t k[2][4];
    const bool whole = grid_cell(nodes, q, blk, bx, k);
    int i, j;
    if (!warp_where(g, blk, bx, &i, &j)) continue;
    uint32_t m[4];
    const bool ok = grid_pixel<T, V>(src, sval, g, C, mode, nodata, 0u, whole, k, q.s, i, j, m);
    index_tail(r, cm, ok, m, dst + ((int64_t)i * g.ow + j) * n, dwords);
  }
}

// The mesh of a call, from its host copy: the step, the node count, every node within bounds with the none mark in its
// y entry alone, and that the source window holds every tap.  Per axis the bilinear combination of a cell lies between
// the smallest and the largest of its four node values, so the positions lie in 2 min .. 2 max (Q17) over the nodes of
// the cells without a none node, and warp_axis_taps does the rest as for an affine view.
static int grid_mesh(const char* what, const Warp& g, const int64_t* mesh, int step, int mode, int* s) {
  DSIC_REQUIRE(step == 16 || step == 32 || step == 64, "%s: step=%d must be 16, 32 or 64", what, step);
  *s = step == 16 ? 4 : step == 32 ? 5 : 6;
  const int64_t nh = (g.oh + step - 1) / step, nw = (g.ow + step - 1) / step, nw1 = nw + 1;
  DSIC_REQUIRE((nh + 1) * nw1 <= GRID_NODES, "%s: output %dx%d at step %d takes a mesh of %lldx%lld nodes, over 2^22", what,
               g.oh, g.ow, step, (long long)(nh + 1), (long long)nw1);
  for (int64_t a = 0; a <= nh; ++a)
    for (int64_t b = 0; b <= nw; ++b) {
      const int64_t y = mesh[(a * nw1 + b) * 2], x = mesh[(a * nw1 + b) * 2 + 1];
      if (y == GRID_NONE) continue;  // no position here; the x entry is not looked at
      DSIC_REQUIRE(x != GRID_NONE, "%s: mesh node (%lld, %lld) has the none mark in its x entry; it belongs in y", what,
                   (long long)a, (long long)b);
      DSIC_REQUIRE(y > -GRID_BOUND && y < GRID_BOUND && x > -GRID_BOUND && x < GRID_BOUND,
                   "%s: mesh node (%lld, %lld) = (%lld, %lld) is outside +-2^48 (Q16)", what, (long long)a, (long long)b,
                   (long long)y, (long long)x);
    }
  int64_t lo[2] = {INT64_MAX, INT64_MAX}, hi[2] = {INT64_MIN, INT64_MIN};
  for (int64_t a = 0; a < nh; ++a)
    for (int64_t b = 0; b < nw; ++b) {
      const int64_t* n[4] = {mesh + (a * nw1 + b) * 2, mesh + (a * nw1 + b + 1) * 2, mesh + ((a + 1) * nw1 + b) * 2,
                             mesh + ((a + 1) * nw1 + b + 1) * 2};
      if (n[0][0] == GRID_NONE || n[1][0] == GRID_NONE || n[2][0] == GRID_NONE || n[3][0] == GRID_NONE) continue;
      for (int c = 0; c < 4; ++c)
        for (int x = 0; x < 2; ++x) lo[x] = n[c][x] < lo[x] ? n[c][x] : lo[x], hi[x] = n[c][x] > hi[x] ? n[c][x] : hi[x];
    }
  int64_t ya = 0, yb = 0, xa = 0, xb = 0;
  if (lo[0] <= hi[0] && warp_axis_taps(2 * lo[0], 2 * hi[0], g.HP, g.LH, g.shift, mode, &ya, &yb) &&
      warp_axis_taps(2 * lo[1], 2 * hi[1], g.WP, g.LW, g.shift, mode, &xa, &xb))
    return warp_holds(what, g, ya, yb, xa, xb);
  return DSIC_OK;
}

// the checks all three kinds share, in warp_check's order and words; on success the device mesh and the launch shape
static int grid_check(const char* what, const void* src, const uint8_t* sval, const void* dst, const uint8_t* oval,
                      const Warp& g, int H, int W, const int64_t* mesh_host, const int64_t* mesh_dev, int step, int C,
                      int cmin, int elem, int delem, int dch, int mode, Mesh* q, int* bx, int64_t* nblocks) {
  DSIC_REQUIRE(src && dst && mesh_host && mesh_dev, "%s: null pointer", what);
  DSIC_REQUIRE(C >= cmin && C <= 4, "%s: C=%d must be in %d..4", what, C, cmin);
  DSIC_REQUIRE(mode >= 0 && mode <= 2, "%s: mode=%d (0 bilinear, 1 nearest, 2 cubic)", what, mode);
  int status = warp_frame(what, g, H, W), s = 0;
  if (status == DSIC_OK) status = grid_mesh(what, g, mesh_host, step, mode, &s);
  if (status != DSIC_OK) return status;
  DSIC_REQUIRE(((uintptr_t)src & (uintptr_t)(elem - 1)) == 0 && ((uintptr_t)dst & (uintptr_t)(delem - 1)) == 0 &&
                   ((uintptr_t)mesh_dev & 7) == 0,
               "%s: src must be %d-byte aligned, dst %d-byte aligned and the mesh 8-byte aligned", what, elem, delem);
  const int64_t spix = (int64_t)g.sh * g.sw, opix = (int64_t)g.oh * g.ow;
  const int nw1 = (g.ow + step - 1) / step + 1;
  const int64_t mbytes = 16 * (int64_t)nw1 * ((g.oh + step - 1) / step + 1);
  DSIC_REQUIRE(windows_apart(src, elem * C * spix, sval, spix, dst, delem * dch * opix, oval, opix),
               "%s: src and dst overlap", what);
  DSIC_REQUIRE(windows_apart(mesh_dev, mbytes, nullptr, 0, dst, delem * dch * opix, oval, opix),
               "%s: the device mesh and dst overlap", what);
  *q = {nw1, s};
  *bx = (g.ow + WARP_TILE - 1) / WARP_TILE;
  *nblocks = (int64_t)*bx * ((g.oh + WARP_TILE - 1) / WARP_TILE);
  return DSIC_OK;
}

template <typename T>
static int grid(const char* what, const T* src, const uint8_t* sval, const Warp& g, int H, int W, const int64_t* mesh_host,
                const int64_t* mesh_dev, int step, int C, int cmin, T* dst, uint8_t* oval, int mode, int nodata, int fill,
                void* stream) {
  int bx;
  int64_t nblocks;
  Mesh q;
  const int status = grid_check(what, src, sval, dst, oval, g, H, W, mesh_host, mesh_dev, step, C, cmin, (int)sizeof(T),
                                (int)sizeof(T), C, mode, &q, &bx, &nblocks);
  if (status != DSIC_OK) return status;
  DSIC_REQUIRE(pixel_value<T>(nodata, -1), "%s: nodata=%d (-1 for none, or a pixel value)", what, nodata);
  DSIC_REQUIRE(pixel_value<T>(fill, 0), "%s: fill=%d must be a pixel value", what, fill);
  if (sval)
    hipLaunchKernelGGL((grid_kernel<T, true>), launch_grid(nblocks), dim3(WARP_TILE * WARP_TILE), 0, (hipStream_t)stream, src,
                       sval, dst, oval, g, mesh_dev, q, C, mode, -1, fill, bx, nblocks);
  else
    hipLaunchKernelGGL((grid_kernel<T, false>), launch_grid(nblocks), dim3(WARP_TILE * WARP_TILE), 0, (hipStream_t)stream, src,
                       sval, dst, oval, g, mesh_dev, q, C, mode, nodata, fill, bx, nblocks);
  return check_launch(what);
}

template <typename T>
static int grid_render(const char* what, const T* src, const uint8_t* sval, const Warp& g, int H, int W,
                       const int64_t* mesh_host, const int64_t* mesh_dev, int step, int C, const int* bands, int nb,
                       const uint32_t* lohi, uint8_t* dst, int mode, int nodata, int alpha, int background, void* stream) {
  int bx;
  int64_t nblocks;
  Mesh q;
  Render r;
  int status = display_options(what, nb, alpha, background);
  if (status == DSIC_OK)
    status = grid_check(what, src, sval, dst, nullptr, g, H, W, mesh_host, mesh_dev, step, C, 1, (int)sizeof(T), 1, nb + alpha,
                        mode, &q, &bx, &nblocks);
  if (status == DSIC_OK) status = display_of<T>(what, C, bands, nb, lohi, nodata, alpha, background, &r);
  if (status != DSIC_OK) return status;
  if (sval)
    hipLaunchKernelGGL((grid_render_kernel<T, true>), launch_grid(nblocks), dim3(WARP_TILE * WARP_TILE), 0,
                       (hipStream_t)stream, src, sval, dst, g, mesh_dev, q, C, mode, -1, r, bx, nblocks);
  else
    hipLaunchKernelGGL((grid_render_kernel<T, false>), launch_grid(nblocks), dim3(WARP_TILE * WARP_TILE), 0,
                       (hipStream_t)stream, src, sval, dst, g, mesh_dev, q, C, mode, nodata, r, bx, nblocks);
  return check_launch(what);
}

template <typename T>
static int grid_index_render(const char* what, const T* src, const uint8_t* sval, const Warp& g, int H, int W,
                             const int64_t* mesh_host, const int64_t* mesh_dev, int step, int C, int kind, int a, int b,
                             int lo, int hi, const uint8_t* cmap, uint8_t* dst, int mode, int nodata, int alpha,
                             int background, void* stream) {
  int bx;
  int64_t nblocks;
  Mesh q;
  IndexRender r;
  const int n = 3 + alpha;
  int status = index_options(what, kind, alpha, background);
  if (status == DSIC_OK)
    status = grid_check(what, src, sval, dst, nullptr, g, H, W, mesh_host, mesh_dev, step, C, 1, (int)sizeof(T), 1, n, mode, &q,
                        &bx, &nblocks);
  if (status == DSIC_OK)
    status = index_of<T>(what, C, kind, a, b, lo, hi, cmap, nodata, alpha, background, dst, (int64_t)n * g.oh * g.ow, &r);
  if (status != DSIC_OK) return status;
  if (sval)
    hipLaunchKernelGGL((grid_index_render_kernel<T, true>), launch_grid(nblocks), dim3(WARP_TILE * WARP_TILE), 0,
                       (hipStream_t)stream, src, sval, dst, g, mesh_dev, q, C, mode, -1, r, cmap, bx, nblocks);
  else
    hipLaunchKernelGGL((grid_index_render_kernel<T, false>), launch_grid(nblocks), dim3(WARP_TILE * WARP_TILE), 0,
                       (hipStream_t)stream, src, sval, dst, g, mesh_dev, q, C, mode, nodata, r, cmap, bx, nblocks);
  return check_launch(what);
}

}  // namespace dsic

using namespace dsic;

extern "C" int dsic_window_grid_u8(const uint8_t* src_hwc, const uint8_t* src_valid, int sh, int sw, int sy0, int sx0,
                                   int C, int shift, int LH, int LW, int H, int W, const int64_t* mesh_host,
                                   const int64_t* mesh_dev, int step, uint8_t* dst_hwc, uint8_t* dst_valid, int oh, int ow,
                                   int mode, int nodata, int fill, void* stream) {
  const Warp g = warp_of(sh, sw, sy0, sx0, shift, LH, LW, H, W, nullptr, oh, ow);
  return grid<uint8_t>("window_grid_u8", src_hwc, src_valid, g, H, W, mesh_host, mesh_dev, step, C, 3, dst_hwc, dst_valid,
                       mode, nodata, fill, stream);
}

extern "C" int dsic_window_grid_u16(const uint16_t* src_hwc, const uint8_t* src_valid, int sh, int sw, int sy0, int sx0,
                                    int C, int shift, int LH, int LW, int H, int W, const int64_t* mesh_host,
                                    const int64_t* mesh_dev, int step, uint16_t* dst_hwc, uint8_t* dst_valid, int oh,
                                    int ow, int mode, int nodata, int fill, void* stream) {
  const Warp g = warp_of(sh, sw, sy0, sx0, shift, LH, LW, H, W, nullptr, oh, ow);
  return grid<uint16_t>("window_grid_u16", src_hwc, src_valid, g, H, W, mesh_host, mesh_dev, step, C, 1, dst_hwc, dst_valid,
                        mode, nodata, fill, stream);
}

extern "C" int dsic_window_grid_render_u8(const uint8_t* src_hwc, const uint8_t* src_valid, int sh, int sw, int sy0,
                                          int sx0, int C, int shift, int LH, int LW, int H, int W,
                                          const int64_t* mesh_host, const int64_t* mesh_dev, int step, const int* bands,
                                          int nb, const uint32_t* lohi, uint8_t* dst, int oh, int ow, int mode, int nodata,
                                          int alpha, int background, void* stream) {
  const Warp g = warp_of(sh, sw, sy0, sx0, shift, LH, LW, H, W, nullptr, oh, ow);
  return grid_render<uint8_t>("window_grid_render_u8", src_hwc, src_valid, g, H, W, mesh_host, mesh_dev, step, C, bands, nb,
                              lohi, dst, mode, nodata, alpha, background, stream);
}

extern "C" int dsic_window_grid_render_u16(const uint16_t* src_hwc, const uint8_t* src_valid, int sh, int sw, int sy0,
                                           int sx0, int C, int shift, int LH, int LW, int H, int W,
                                           const int64_t* mesh_host, const int64_t* mesh_dev, int step, const int* bands,
                                           int nb, const uint32_t* lohi, uint8_t* dst, int oh, int ow, int mode, int nodata,
                                           int alpha, int background, void* stream) {
  const Warp g = warp_of(sh, sw, sy0, sx0, shift, LH, LW, H, W, nullptr, oh, ow);
  return grid_render<uint16_t>("window_grid_render_u16", src_hwc, src_valid, g, H, W, mesh_host, mesh_dev, step, C, bands, nb,
                               lohi, dst, mode, nodata, alpha, background, stream);
}

extern "C" int dsic_window_grid_index_render_u8(const uint8_t* src_hwc, const uint8_t* src_valid, int sh, int sw, int sy0,
                                                int sx0, int C, int shift, int LH, int LW, int H, int W,
                                                const int64_t* mesh_host, const int64_t* mesh_dev, int step, int kind,
                                                int band_a, int band_b, int lo, int hi, const uint8_t* cmap_dev,
                                                uint8_t* dst, int oh, int ow, int mode, int nodata, int alpha,
                                                int background, void* stream) {
  const Warp g = warp_of(sh, sw, sy0, sx0, shift, LH, LW, H, W, nullptr, oh, ow);
  return grid_index_render<uint8_t>("window_grid_index_render_u8", src_hwc, src_valid, g, H, W, mesh_host, mesh_dev, step, C,
                                    kind, band_a, band_b, lo, hi, cmap_dev, dst, mode, nodata, alpha, background, stream);
}

extern "C" int dsic_window_grid_index_render_u16(const uint16_t* src_hwc, const uint8_t* src_valid, int sh, int sw, int sy0,
                                                 int sx0, int C, int shift, int LH, int LW, int H, int W,
                                                 const int64_t* mesh_host, const int64_t* mesh_dev, int step, int kind,
                                                 int band_a, int band_b, int lo, int hi, const uint8_t* cmap_dev,
                                                 uint8_t* dst, int oh, int ow, int mode, int nodata, int alpha,
                                                 int background, void* stream) {
  const Warp g = warp_of(sh, sw, sy0, sx0, shift, LH, LW, H, W, nullptr, oh, ow);
  return grid_index_render<uint16_t>("window_grid_index_render_u16", src_hwc, src_valid, g, H, W, mesh_host, mesh_dev, step,
                                     C, kind, band_a, band_b, lo, hi, cmap_dev, dst, mode, nodata, alpha, background, stream);
}
