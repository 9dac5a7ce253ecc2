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
// aligned 16-byte chunks (8 values) with element stores only at the ragged ends (hwc_chunks.h).  The gather reads the
// image once: a lane takes 4 consecutive pixels of a row (8 C bytes), consecutive lanes consecutive runs, and stores
// one float4 per plane.  The stitch and the blend finish are image_codec.hip's stitch_hwc_kernel<uint16_t, RES> and
// blend_finish_hwc_kernel<uint16_t>, the halving is halve.h's halve_kernel<uint16_t, C, false>; here stand the band
// range (with and without a validity image), the gather, and the exports.
#include "halve.h"
#include "hwc_launch.h"

namespace dsic {

// ---- band range -------------------------------------------------------------------------------------------

__global__ void band_range_init_kernel(uint32_t* __restrict__ out, int C) {
  if ((int)threadIdx.x < 2 * C) out[threadIdx.x] = (threadIdx.x & 1) ? 0u : 0xFFFFFFFFu;
}

// V: a band that met no valid pixel still holds the start values: it becomes (0, 0)
__global__ void band_range_finish_kernel(uint32_t* __restrict__ out, int C) {
  if ((int)threadIdx.x < C && out[2 * threadIdx.x] > out[2 * threadIdx.x + 1]) out[2 * threadIdx.x] = 0u;
}

// Per band the minimum and maximum of npix pixels; with V (a validity byte per pixel, 0 = invalid) of the valid ones
// only.  A unit is 8 pixels, C 16-byte loads that begin at a pixel and with V their 8 validity bytes, so a value's band
// is known at compile time; the units are dealt out grid-stride, the pixels behind the last whole unit go to the first
// lanes of workgroup 0.  Wave reduction, workgroup reduction through LDS, then one atomic min and max per workgroup and
// band: min and max do not depend on the order, so neither does the result.
template <int C, bool V>
__global__ __launch_bounds__(256) void band_range_kernel(const uint16_t* __restrict__ img,
                                                         const uint8_t* __restrict__ val, int64_t npix,
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
    uint8_t ok[8];
#pragma unroll
    for (int k = 0; k < C; ++k) q[k] = load16_any((const uint8_t*)(img + u * 8 * C) + 16 * k);
    __builtin_memcpy(v, q, 16 * C);
#pragma unroll
    for (int k = 0; k < 8; ++k) ok[k] = V ? val[u * 8 + k] : 1;
#pragma unroll
    for (int k = 0; k < 8 * C; ++k) {
      if (ok[k / C]) {
        mn[k % C] = min(mn[k % C], (uint32_t)v[k]);
        mx[k % C] = max(mx[k % C], (uint32_t)v[k]);
      }
    }
  }
  if (tid < (npix & 7) && (!V || val[(units << 3) + tid])) {
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

template <bool V>
static void launch_band_range(int C, dim3 grid, hipStream_t st, const uint16_t* img, const uint8_t* val, int64_t npix,
                              uint32_t* out) {
  switch (C) {
    case 1: hipLaunchKernelGGL((band_range_kernel<1, V>), grid, dim3(256), 0, st, img, val, npix, out); break;
    case 2: hipLaunchKernelGGL((band_range_kernel<2, V>), grid, dim3(256), 0, st, img, val, npix, out); break;
    case 3: hipLaunchKernelGGL((band_range_kernel<3, V>), grid, dim3(256), 0, st, img, val, npix, out); break;
    default: hipLaunchKernelGGL((band_range_kernel<4, V>), grid, dim3(256), 0, st, img, val, npix, out); break;
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

// ---- exports ----------------------------------------------------------------------------------------------
// `what` is the export's name in its messages; valid_hw == nullptr is refused where `valid` asks for it.
static int band_range(const char* what, bool valid, const uint16_t* img_hwc, const uint8_t* valid_hw, int H, int W,
                      int C, uint32_t* out_lohi_dev, void* stream) {
  DSIC_REQUIRE(img_hwc && (valid_hw || !valid) && out_lohi_dev, "%s: null pointer", what);
  DSIC_U16_COMMON(what, img_hwc);
  DSIC_REQUIRE(H >= 1 && W >= 1, "%s: empty image %dx%d", what, H, W);
  DSIC_U16_ROW(what, W);
  DSIC_REQUIRE(((uintptr_t)out_lohi_dev & 3) == 0, "%s: out must be 4-byte aligned", what);
  char step[64];
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(band_range_init_kernel, dim3(1), dim3(64), 0, st, out_lohi_dev, C);
  snprintf(step, sizeof step, "%s(init)", what);
  int rc = check_launch(step);
  if (rc) return rc;
  const int64_t npix = (int64_t)H * W;
  int64_t blocks = ((npix >> 3) + 4 * 256 - 1) / (4 * 256);  // about four units per lane
  blocks = blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);
  if (valid) launch_band_range<true>(C, dim3((unsigned)blocks), st, img_hwc, valid_hw, npix, out_lohi_dev);
  else launch_band_range<false>(C, dim3((unsigned)blocks), st, img_hwc, valid_hw, npix, out_lohi_dev);
  rc = check_launch(what);
  if (rc || !valid) return rc;
  hipLaunchKernelGGL(band_range_finish_kernel, dim3(1), dim3(64), 0, st, out_lohi_dev, C);
  snprintf(step, sizeof step, "%s(finish)", what);
  return check_launch(step);
}

static int gather_u16(const char* what, const uint16_t* img_hwc, float* tiles, int H, int W, int C, int th, int tw,
                      int overlap, const uint32_t* lohi, int first_tile, int n_tiles, void* stream) {
  DSIC_REQUIRE(img_hwc && tiles && lohi, "%s: null pointer", what);
  DSIC_U16_COMMON(what, img_hwc);
  DSIC_U16_SCALE(what);
  DSIC_TILE_ARGS_OV(what, overlap);
  DSIC_U16_ROW(what, W);
  DSIC_REQUIRE(((uintptr_t)tiles & 15) == 0, "%s: tiles must be 16-byte aligned", what);
  DSIC_U16_BY_C(gather_u16_kernel, grid, dim3(256), 0, (hipStream_t)stream, img_hwc, tiles, g, first_tile, sc);
  return check_launch(what);
}

// q == nullptr stands for "no residual" only where res is false
static int stitch_window_u16(const char* what, bool res, const float* tiles, const float* q, int tau,
                             const int* tile_ids, int n_tiles, uint16_t* out, int H, int W, int C, int th, int tw,
                             int wy0, int wx0, int wh, int ww, const uint32_t* lohi, void* stream) {
  DSIC_REQUIRE(tiles && (q || !res) && tile_ids && out && lohi, "%s: null pointer", what);
  DSIC_U16_COMMON(what, out);
  DSIC_REQUIRE(!res || (tau >= 0 && tau <= 32767), "%s: tau=%d must be in 0..32767", what, tau);
  DSIC_U16_SCALE(what);
  DSIC_WINDOW_ARGS(what);
  DSIC_U16_ROW(what, ww);
  launch_stitch_u16(res, grid, (hipStream_t)stream, tiles, q, res ? 2 * tau + 1 : 0, out, g, C, tile_ids, clip, sc);
  return check_launch(what);
}

}  // namespace dsic

using namespace dsic;

extern "C" int dsic_band_range_u16(const uint16_t* img_hwc, int H, int W, int C, uint32_t* out_lohi_dev,
                                   void* stream) {
  return band_range("band_range_u16", false, img_hwc, nullptr, H, W, C, out_lohi_dev, stream);
}

extern "C" int dsic_band_range_valid_u16(const uint16_t* img_hwc, const uint8_t* valid_hw, int H, int W, int C,
                                         uint32_t* out_lohi_dev, void* stream) {
  return band_range("band_range_valid_u16", true, img_hwc, valid_hw, H, W, C, out_lohi_dev, stream);
}

extern "C" int dsic_tile_gather_u16_ov(const uint16_t* img_hwc, float* tiles, int H, int W, int C, int th, int tw,
                                       int overlap, const uint32_t* lohi, int first_tile, int n_tiles, void* stream) {
  return gather_u16("tile_gather_u16_ov", img_hwc, tiles, H, W, C, th, tw, overlap, lohi, first_tile, n_tiles, stream);
}

extern "C" int dsic_tile_gather_u16(const uint16_t* img_hwc, float* tiles, int H, int W, int C, int th, int tw,
                                    const uint32_t* lohi, int first_tile, int n_tiles, void* stream) {
  return gather_u16("tile_gather_u16", img_hwc, tiles, H, W, C, th, tw, 0, lohi, first_tile, n_tiles, stream);
}

extern "C" int dsic_tile_stitch_window_u16(const float* tiles, const int* tile_ids, int n_tiles, uint16_t* out, int H,
                                           int W, int C, int th, int tw, int wy0, int wx0, int wh, int ww,
                                           const uint32_t* lohi, void* stream) {
  return stitch_window_u16("tile_stitch_window_u16", false, tiles, nullptr, 0, tile_ids, n_tiles, out, H, W, C, th, tw,
                           wy0, wx0, wh, ww, lohi, stream);
}

extern "C" int dsic_tile_stitch_window_u16_res(const float* tiles, const float* q, int tau, const int* tile_ids,
                                               int n_tiles, uint16_t* out, int H, int W, int C, int th, int tw, int wy0,
                                               int wx0, int wh, int ww, const uint32_t* lohi, void* stream) {
  return stitch_window_u16("tile_stitch_window_u16_res", true, tiles, q, tau, tile_ids, n_tiles, out, H, W, C, th, tw,
                           wy0, wx0, wh, ww, lohi, stream);
}

extern "C" int dsic_tile_blend_finish_u16(const float* canvas, uint16_t* out_hwc, int C, int h, int w,
                                          const uint32_t* lohi, void* stream) {
  DSIC_REQUIRE(canvas && out_hwc && lohi, "tile_blend_finish_u16: null pointer");
  DSIC_U16_COMMON("tile_blend_finish_u16", out_hwc);
  DSIC_U16_SCALE("tile_blend_finish_u16");
  DSIC_REQUIRE(h >= 1 && w >= 1, "tile_blend_finish_u16: empty window %dx%d", h, w);
  DSIC_U16_ROW("tile_blend_finish_u16", w);
  launch_blend_finish_u16((hipStream_t)stream, canvas, out_hwc, C, (int64_t)h * w, sc);
  return check_launch("tile_blend_finish_u16");
}

extern "C" int dsic_image_halve_u16(const uint16_t* src_hwc, uint16_t* dst_hwc, int H, int W, int C, void* stream) {
  DSIC_REQUIRE(src_hwc && dst_hwc, "image_halve_u16: null pointer");
  DSIC_U16_COMMON("image_halve_u16", (uintptr_t)src_hwc | (uintptr_t)dst_hwc);
  DSIC_REQUIRE(H >= 1 && W >= 1, "image_halve_u16: H=%d W=%d must both be at least 1", H, W);
  DSIC_U16_ROW("image_halve_u16", W);
  const Halve g = make_halve(H, W);
  DSIC_REQUIRE(buffers_apart(src_hwc, 2 * (int64_t)H * W * C, dst_hwc, 2 * (int64_t)g.H2 * g.W2 * C),
               "image_halve_u16: src and dst overlap");
  launch_halve<uint16_t, false>(src_hwc, dst_hwc, g, C, {}, (hipStream_t)stream);
  return check_launch("image_halve_u16");
}
