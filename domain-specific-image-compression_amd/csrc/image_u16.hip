// 16-bit imagery for the whole-image codec (codec.py, stream version 6): uint16 [H][W][C] scenes with a per-band
// scale (lo, hi), R = hi - lo, that travels in the stream.  The normalisation of code/combinebandsall.py:7-12 is
// fused into the tile gather and its inverse into the stitch and the blend finish:
//   norm(v)   = R == 0 ? 0.0f : (float)(min(max(v, lo), hi) - lo) / (float)R      one IEEE division
//   denorm(x) = lo + (uint32)(clamp(x, 0, 1) * (float)R + 0.5f)                   unfused, rounds to nearest
// so that the gather's tiles are those tile_gather_f32 cuts from the float32 image norm(img), bit for bit, and
// denorm(norm(v)) == v inside [lo, hi].  The scale is at most 4 pairs, passed by value in the kernel arguments.
//
// Byte movers as image_codec.hip's and pyramid.hip's.  Images are uint16 at any 2-byte alignment: loads are dwordx4 /
// dwordx2 where the address allows and alignbyte funnels of dword loads where it does not; outputs are written as
// aligned 16-byte chunks (8 pixels' values) with element stores only at the ragged ends.  The gather reads the image
// once: a lane takes 4 consecutive pixels of a row (8 C bytes), consecutive lanes consecutive runs, and stores one
// float4 per plane.
#include "byte_movers.h"
#include "tile_grid.h"
#include "u16_scale.h"

namespace dsic {

// ---- band range -------------------------------------------------------------------------------------------

__global__ void band_range_init_kernel(uint32_t* __restrict__ out, int C) {
  if ((int)threadIdx.x < 2 * C) out[threadIdx.x] = (threadIdx.x & 1) ? 0u : 0xFFFFFFFFu;
}

// Per band the minimum and maximum of npix pixels.  A unit is 8 pixels, C 16-byte loads that begin at a pixel, so a
// value's band is known at compile time; the units are dealt out grid-stride, the pixels behind the last whole unit go
// to the first lanes of workgroup 0.  Wave reduction, workgroup reduction through LDS, then one atomic min and max per
// workgroup and band: min and max do not depend on the order, so neither does the result.
template <int C>
__global__ __launch_bounds__(256) void band_range_kernel(const uint16_t* __restrict__ img, int64_t npix,
                                                         uint32_t* __restrict__ out) {
  __shared__ uint32_t red[2][4][4];
  uint32_t mn[C], mx[C];
#pragma unroll
  for (int c = 0; c < C; ++c) mn[c] = 0xFFFFFFFFu, mx[c] = 0u;
  const int64_t units = npix >> 3, step = (int64_t)gridDim.x * blockDim.x;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t u = tid; u < units; u += step) {
    uint4 q[C];
    uint16_t v[8 * C];
#pragma unroll
    for (int k = 0; k < C; ++k) q[k] = load16_any((const uint8_t*)(img + u * 8 * C) + 16 * k);
    __builtin_memcpy(v, q, 16 * C);
#pragma unroll
    for (int k = 0; k < 8 * C; ++k) {
      mn[k % C] = min(mn[k % C], (uint32_t)v[k]);
      mx[k % C] = max(mx[k % C], (uint32_t)v[k]);
    }
  }
  if (tid < (npix & 7)) {
    const uint16_t* p = img + ((units << 3) + tid) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) mn[c] = min(mn[c], (uint32_t)p[c]), mx[c] = max(mx[c], (uint32_t)p[c]);
  }
#pragma unroll
  for (int c = 0; c < C; ++c) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      mn[c] = min(mn[c], (uint32_t)__shfl_down(mn[c], o, 64));
      mx[c] = max(mx[c], (uint32_t)__shfl_down(mx[c], o, 64));
    }
    if ((threadIdx.x & 63) == 0) red[0][c][threadIdx.x >> 6] = mn[c], red[1][c][threadIdx.x >> 6] = mx[c];
  }
  __syncthreads();
  if ((int)threadIdx.x < C) {
    const int c = threadIdx.x;
    atomicMin(out + 2 * c, min(min(red[0][c][0], red[0][c][1]), min(red[0][c][2], red[0][c][3])));
    atomicMax(out + 2 * c + 1, max(max(red[1][c][0], red[1][c][1]), max(red[1][c][2], red[1][c][3])));
  }
}

// ---- tile gather ------------------------------------------------------------------------------------------

// uint16 HWC image -> float32 tiles [n][C][th][tw], normalised; the grid and the padding of gather_f32_kernel
template <int C>
__global__ __launch_bounds__(256) void gather_u16_kernel(const uint16_t* __restrict__ img, float* __restrict__ tiles,
                                                         Grid g, int first, Scale s) {
  const int t = first + blockIdx.y;
  const int oy = g.oy(t / g.nx), ox = g.ox(t % g.nx);
  const int vpr = g.tw >> 2;
  const int r0 = blockIdx.x * kTileRows;
  const size_t cplane = (size_t)g.th * g.tw;
  float* dst = tiles + (size_t)blockIdx.y * C * cplane + (size_t)r0 * g.tw;
  for (int i = threadIdx.x; i < kTileRows * vpr; i += blockDim.x) {
    const int r = i / vpr, j0 = (i - r * vpr) << 2;
    const uint16_t* src_row = img + (size_t)reflect(oy + r0 + r, g.H) * g.W * C;
    const int x0 = ox + j0;
    uint16_t v[4 * C];
    if (x0 + 3 < g.W) {
      load_run<2 * C>(src_row + (size_t)x0 * C, v);
    } else {  // the run reaches the reflected columns
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const uint16_t* px = src_row + (size_t)reflect(x0 + p, g.W) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) v[p * C + c] = px[c];
      }
    }
#pragma unroll
    for (int c = 0; c < C; ++c)
      *(float4*)(dst + c * cplane + (size_t)r * g.tw + j0) =
          make_float4(norm_u16(v[c], s.lo[c], s.R[c]), norm_u16(v[C + c], s.lo[c], s.R[c]),
                      norm_u16(v[2 * C + c], s.lo[c], s.R[c]), norm_u16(v[3 * C + c], s.lo[c], s.R[c]));
  }
}

// ---- tile stitch and blend finish --------------------------------------------------------------------------

// tiles [n][C][th][tw] -> denorm into the uint16 HWC window image; the rectangles of stitch_u8_kernel.  Positions
// count uint16 elements; `mis` is the window image's offset behind a 16-byte boundary in elements, so that chunk q0
// (in elements shifted by mis) is an aligned 16 bytes of memory.
// RES (codec.py, tolerance = tau): the decoded residual steps q float32 [n][C][th][tw] (residual_u16.hip) are added,
// a value is clamp(denorm(x_hat) + (int)q * step, 0, 65535) with step = 2 tau + 1; |q| <= (65535 + tau) / step as the
// join kernel leaves it, so the sum stays inside int32.
template <bool RES>
__global__ __launch_bounds__(256) void stitch_u16_kernel(const float* __restrict__ tiles, const float* __restrict__ qres,
                                                         int step, uint16_t* __restrict__ img, Grid g, int C,
                                                         const int* __restrict__ ids, Clip w, Scale s, int mis) {
  Owned o;
  if (!stitch_rect(g, ids, 0, w, &o)) return;
  const int ya = o.y0 + blockIdx.x * kTileRows;
  const int rows = min(kTileRows, o.y1 - ya);
  if (rows <= 0) return;
  const size_t cplane = (size_t)g.th * g.tw;
  const float* src = tiles + (size_t)blockIdx.y * C * cplane;
  const float* qsrc = RES ? qres + (size_t)blockIdx.y * C * cplane : nullptr;
  const int wW = w.x1 - w.x0;
  const int seg = (o.x1 - o.x0) * C;
  const int cpr = seg / 8 + 2;  // 16-byte chunks a row segment can touch
  for (int i = threadIdx.x; i < rows * cpr; i += blockDim.x) {
    const int r = i / cpr, k = i - r * cpr;
    const int y = ya + r;
    const int64_t b0 = ((int64_t)(y - w.y0) * wW + (o.x0 - w.x0)) * C + mis, b1 = b0 + seg;
    const int64_t q0 = ((b0 >> 3) + k) << 3;
    if (q0 >= b1) continue;
    const int64_t lo = max(q0, b0), hi = min(q0 + 8, b1);
    const float* srow = src + (size_t)(y - o.oy) * g.tw;
    int px = (int)((lo - b0) / C), c = (int)((lo - b0) - (int64_t)px * C);
    px += o.x0 - o.ox;  // column within the tile
    uint16_t b[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      b[e] = 0;
      if (q0 + e >= lo && q0 + e < hi) {
        b[e] = denorm_u16(srow[c * cplane + px], pick(s.lo, c), pick(s.R, c));
        if constexpr (RES) {
          const int v = (int)b[e] + (int)qsrc[(size_t)(y - o.oy) * g.tw + c * cplane + px] * step;
          b[e] = (uint16_t)(v < 0 ? 0 : (v > 65535 ? 65535 : v));
        }
        if (++c == C) c = 0, ++px;
      }
    }
    if (lo == q0 && hi == q0 + 8) {
      uint4 v;
      __builtin_memcpy(&v, b, 16);
      *(uint4*)(img + (q0 - mis)) = v;
    } else {
      for (int64_t e = lo; e < hi; ++e) img[e - mis] = b[e - q0];
    }
  }
}

// canvas float32 [C][hw] -> denorm(min(v, 1)) into the uint16 [hw][C] image, 16 bytes per lane
__global__ __launch_bounds__(256) void blend_finish_u16_kernel(const float* __restrict__ canvas,
                                                               uint16_t* __restrict__ out, int C, int64_t hw, Scale s,
                                                               int mis) {
  const int64_t n = hw * C + mis, nq = (n + 7) >> 3, step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += step) {
    const int64_t q0 = q << 3, lo = max(q0, (int64_t)mis), hi = min(q0 + 8, n);
    int64_t px = (lo - mis) / C;
    int c = (int)((lo - mis) - px * C);
    uint16_t b[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      b[e] = 0;
      if (q0 + e >= lo && q0 + e < hi) {
        b[e] = denorm_u16(canvas[c * hw + px], pick(s.lo, c), pick(s.R, c));  // the clamp of denorm is min(v, 1)
        if (++c == C) c = 0, ++px;
      }
    }
    if (lo == q0 && hi == q0 + 8) {
      uint4 v;
      __builtin_memcpy(&v, b, 16);
      *(uint4*)(out + (q0 - mis)) = v;
    } else {
      for (int64_t e = lo; e < hi; ++e) out[e - mis] = b[e - q0];
    }
  }
}

// ---- halving (overviews) -----------------------------------------------------------------------------------

struct Halve16 {
  int H, W, H2, W2;
  __device__ __forceinline__ int below(int y) const { return min(2 * y + 1, H - 1); }
  __device__ __forceinline__ int right(int x) const { return min(2 * x + 1, W - 1); }
};

// elements [i0, i0 + n), n <= 8, of the flat uint16 output -> b[0 .. n)
__device__ __forceinline__ void halve_elems(const uint16_t* __restrict__ src, const Halve16& g, int C, int64_t i0,
                                            int n, uint16_t* b) {
  const int64_t p = i0 / C;
  int c = (int)(i0 - p * C), y = (int)(p / g.W2), x = (int)(p - (int64_t)y * g.W2);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    b[e] = 0;
    if (e < n) {
      const uint16_t* top = src + (int64_t)(2 * y) * g.W * C + c;
      const uint16_t* bot = src + (int64_t)g.below(y) * g.W * C + c;
      const int64_t xa = (int64_t)(2 * x) * C, xb = (int64_t)g.right(x) * C;
      b[e] = (uint16_t)(((uint32_t)top[xa] + (uint32_t)top[xb] + (uint32_t)bot[xa] + (uint32_t)bot[xb] + 2u) >> 2);
      if (++c == C) {
        c = 0;
        if (++x == g.W2) x = 0, ++y;
      }
    }
  }
}

// 8 output values that begin at channel PH of an output pixel, from the 24 values (48 bytes) of each source row
// that begin at that pixel's left source pixel: output e is channel (PH + e) % C of pixel j = (PH + e) / C, whose
// sources are values 2jC + c and 2jC + c + C of the two windows (at most value 22).
template <int C, int PH>
__device__ __forceinline__ uint4 halve16_window(const uint16_t* __restrict__ top, const uint16_t* __restrict__ bot) {
  uint16_t t[24], u[24], o[8];
  load_run<12>(top, t);
  load_run<12>(bot, u);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int j = (PH + e) / C, c = (PH + e) % C, a = 2 * j * C + c;
    o[e] = (uint16_t)(((uint32_t)t[a] + (uint32_t)t[a + C] + (uint32_t)u[a] + (uint32_t)u[a + C] + 2u) >> 2);
  }
  uint4 v;
  __builtin_memcpy(&v, o, 16);
  return v;
}

template <int C>
__device__ __forceinline__ uint4 halve16_window_at(int ph, const uint16_t* __restrict__ top,
                                                   const uint16_t* __restrict__ bot) {
  switch (ph) {
    case 0: return halve16_window<C, 0>(top, bot);
    case 1: return halve16_window<C, (C > 1 ? 1 : 0)>(top, bot);
    case 2: return halve16_window<C, (C > 2 ? 2 : 0)>(top, bot);
    default: return halve16_window<C, C - 1>(top, bot);
  }
}

// uint16 [H][W][C] -> uint16 [H2][W2][C], n values: `head` values up to dst's first aligned chunk, nfull chunks of 8,
// a tail.  A chunk inside one output row, away from a repeated last column and with both 48-byte windows inside the
// image takes the window path; every other goes value by value.
template <int C>
__global__ __launch_bounds__(256) void halve_u16_kernel(const uint16_t* __restrict__ src, uint16_t* __restrict__ dst,
                                                        Halve16 g, int64_t n, int head, int64_t nfull) {
  const int rb = g.W2 * C;  // values of an output row
  const int64_t total = (int64_t)g.H * g.W * C;
  if (blockIdx.x == 0 && threadIdx.x < 2) {  // the ragged ends: under 8 values each
    const int64_t lo = threadIdx.x ? head + 8 * nfull : 0, hi = threadIdx.x ? n : head;
    uint16_t b[8];
    halve_elems(src, g, C, lo, (int)(hi - lo), b);
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (e < hi - lo) dst[lo + e] = b[e];
  }
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nfull; q += step) {
    const int64_t q0 = head + 8 * q;
    const int y = (int)(q0 / rb), b0 = (int)(q0 - (int64_t)y * rb);
    const int xf = b0 / C, xl = (b0 + 7) / C;
    const int64_t st = ((int64_t)(2 * y) * g.W + 2 * xf) * C, sb = ((int64_t)g.below(y) * g.W + 2 * xf) * C;
    uint4 v;
    if (b0 + 8 <= rb && 2 * xl + 1 < g.W && sb + 24 <= total) {
      v = halve16_window_at<C>(b0 - xf * C, src + st, src + sb);
    } else {
      uint16_t b[8];
      halve_elems(src, g, C, q0, 8, b);
      __builtin_memcpy(&v, b, 16);
    }
    *(uint4*)(dst + q0) = v;
  }
}

static bool apart16(const void* a, int64_t a_bytes, const void* b, int64_t b_bytes) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa + (uintptr_t)a_bytes <= pb || pb + (uintptr_t)b_bytes <= pa;
}

}  // namespace dsic

using namespace dsic;

extern "C" int dsic_band_range_u16(const uint16_t* img_hwc, int H, int W, int C, uint32_t* out_lohi_dev,
                                   void* stream) {
  DSIC_REQUIRE(img_hwc && out_lohi_dev, "band_range_u16: null pointer");
  DSIC_U16_COMMON("band_range_u16", img_hwc);
  DSIC_REQUIRE(H >= 1 && W >= 1, "band_range_u16: empty image %dx%d", H, W);
  DSIC_U16_ROW("band_range_u16", W);
  DSIC_REQUIRE(((uintptr_t)out_lohi_dev & 3) == 0, "band_range_u16: out must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(band_range_init_kernel, dim3(1), dim3(64), 0, st, out_lohi_dev, C);
  const int rc = check_launch("band_range_u16(init)");
  if (rc) return rc;
  const int64_t npix = (int64_t)H * W;
  int64_t blocks = ((npix >> 3) + 4 * 256 - 1) / (4 * 256);  // about four units per lane
  blocks = blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);
  DSIC_U16_BY_C(band_range_kernel, dim3((unsigned)blocks), dim3(256), 0, st, img_hwc, npix, out_lohi_dev);
  return check_launch("band_range_u16");
}

#define DSIC_GATHER_U16(what)                                                                                     \
  DSIC_REQUIRE(img_hwc && tiles && lohi, what ": null pointer");                                                  \
  DSIC_U16_COMMON(what, img_hwc);                                                                                 \
  DSIC_U16_SCALE(what);                                                                                           \
  DSIC_TILE_ARGS_OV(what, overlap);                                                                               \
  DSIC_U16_ROW(what, W);                                                                                          \
  DSIC_REQUIRE(((uintptr_t)tiles & 15) == 0, what ": tiles must be 16-byte aligned");                             \
  DSIC_U16_BY_C(gather_u16_kernel, grid, dim3(256), 0, (hipStream_t)stream, img_hwc, tiles, g, first_tile, sc);   \
  return check_launch(what)

extern "C" int dsic_tile_gather_u16_ov(const uint16_t* img_hwc, float* tiles, int H, int W, int C, int th, int tw,
                                       int overlap, const uint32_t* lohi, int first_tile, int n_tiles, void* stream) {
  DSIC_GATHER_U16("tile_gather_u16_ov");
}

extern "C" int dsic_tile_gather_u16(const uint16_t* img_hwc, float* tiles, int H, int W, int C, int th, int tw,
                                    const uint32_t* lohi, int first_tile, int n_tiles, void* stream) {
  const int overlap = 0;
  DSIC_GATHER_U16("tile_gather_u16");
}

extern "C" int dsic_tile_stitch_window_u16(const float* tiles, const int* tile_ids, int n_tiles, uint16_t* out, int H,
                                           int W, int C, int th, int tw, int wy0, int wx0, int wh, int ww,
                                           const uint32_t* lohi, void* stream) {
  DSIC_REQUIRE(tiles && tile_ids && out && lohi, "tile_stitch_window_u16: null pointer");
  DSIC_U16_COMMON("tile_stitch_window_u16", out);
  DSIC_U16_SCALE("tile_stitch_window_u16");
  DSIC_WINDOW_ARGS("tile_stitch_window_u16");
  DSIC_U16_ROW("tile_stitch_window_u16", ww);
  hipLaunchKernelGGL(stitch_u16_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, tiles, (const float*)nullptr, 0,
                     out, g, C, tile_ids, clip, sc, (int)(((uintptr_t)out & 15) >> 1));
  return check_launch("tile_stitch_window_u16");
}

extern "C" int dsic_tile_stitch_window_u16_res(const float* tiles, const float* q, int tau, const int* tile_ids,
                                               int n_tiles, uint16_t* out, int H, int W, int C, int th, int tw, int wy0,
                                               int wx0, int wh, int ww, const uint32_t* lohi, void* stream) {
  DSIC_REQUIRE(tiles && q && tile_ids && out && lohi, "tile_stitch_window_u16_res: null pointer");
  DSIC_U16_COMMON("tile_stitch_window_u16_res", out);
  DSIC_REQUIRE(tau >= 0 && tau <= 32767, "tile_stitch_window_u16_res: tau=%d must be in 0..32767", tau);
  DSIC_U16_SCALE("tile_stitch_window_u16_res");
  DSIC_WINDOW_ARGS("tile_stitch_window_u16_res");
  DSIC_U16_ROW("tile_stitch_window_u16_res", ww);
  hipLaunchKernelGGL(stitch_u16_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, tiles, q, 2 * tau + 1, out, g, C,
                     tile_ids, clip, sc, (int)(((uintptr_t)out & 15) >> 1));
  return check_launch("tile_stitch_window_u16_res");
}

extern "C" int dsic_tile_blend_finish_u16(const float* canvas, uint16_t* out_hwc, int C, int h, int w,
                                          const uint32_t* lohi, void* stream) {
  DSIC_REQUIRE(canvas && out_hwc && lohi, "tile_blend_finish_u16: null pointer");
  DSIC_U16_COMMON("tile_blend_finish_u16", out_hwc);
  DSIC_U16_SCALE("tile_blend_finish_u16");
  DSIC_REQUIRE(h >= 1 && w >= 1, "tile_blend_finish_u16: empty window %dx%d", h, w);
  DSIC_U16_ROW("tile_blend_finish_u16", w);
  const int64_t hw = (int64_t)h * w;
  hipLaunchKernelGGL(blend_finish_u16_kernel, dim3(finish_blocks((hw * C + 15) >> 3)), dim3(256), 0,
                     (hipStream_t)stream, canvas, out_hwc, C, hw, sc, (int)(((uintptr_t)out_hwc & 15) >> 1));
  return check_launch("tile_blend_finish_u16");
}

extern "C" int dsic_image_halve_u16(const uint16_t* src_hwc, uint16_t* dst_hwc, int H, int W, int C, void* stream) {
  DSIC_REQUIRE(src_hwc && dst_hwc, "image_halve_u16: null pointer");
  DSIC_U16_COMMON("image_halve_u16", (uintptr_t)src_hwc | (uintptr_t)dst_hwc);
  DSIC_REQUIRE(H >= 1 && W >= 1, "image_halve_u16: H=%d W=%d must both be at least 1", H, W);
  DSIC_U16_ROW("image_halve_u16", W);
  const Halve16 g = {H, W, H / 2 + (H & 1), W / 2 + (W & 1)};
  const int64_t n = (int64_t)g.H2 * g.W2 * C;
  DSIC_REQUIRE(apart16(src_hwc, 2 * (int64_t)H * W * C, dst_hwc, 2 * n), "image_halve_u16: src and dst overlap");
  int64_t head = ((16 - ((uintptr_t)dst_hwc & 15)) & 15) >> 1;
  if (head > n) head = n;
  const int64_t nfull = (n - head) >> 3;
  DSIC_U16_BY_C(halve_u16_kernel, dim3(finish_blocks(nfull)), dim3(256), 0, (hipStream_t)stream, src_hwc, dst_hwc, g,
                n, (int)head, nfull);
  return check_launch("image_halve_u16");
}
