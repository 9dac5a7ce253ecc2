// Nodata masks of the whole-image codec (codec.compress_image with nodata = v, stream version 5).  A pixel of a uint8
// HWC image is nodata iff all its C channels equal v.  Per tile, over the pixels it owns inside H x W (tile_grid.h
// owned()), the mask m is a bit plane in tile coordinates: th*tw bits, row-major, bit y*tw + x in byte (y*tw + x) / 8,
// LSB first; 1 iff the pixel is owned, inside the image and nodata.  What travels is the vertical delta plane
// d[y][x] = m[y][x] ^ m[y-1][x] (m[-1] = 0), raw (mode 0, th*tw/8 bytes) or as the ascending positions of its set
// bits (mode 1; u16 if th*tw <= 65536, else u32), whichever is shorter, raw on a tie.
//
// Byte movers as image_codec.hip's.  The image is read 16 pixels per lane, C 16-byte loads (load16_any: the image
// is aligned as it happens to be) that become one 16-bit half of a plane dword; a run of 16 pixels that the tile does
// not own whole goes pixel by pixel.  tw is a multiple of 16, not of 32, so a plane row is a whole number of halves and
// a dword may hold the end of one row and the start of the next.
//
//   classify      image -> per tile the count of nodata pixels among its owned pixels: one read of the image
//   delta planes  image, tile ids -> d planes as dwords [th*tw/32] and their popcounts: the tiles' pixels read twice
//                 (a half needs its row and the row above), the second time from cache
//   pack          planes, popcounts -> records (tile, mode, bytes) and the payloads back to back in one buffer;
//                 mode 1 is an ordered compaction (workgroup scan over the dwords' popcounts)
//   unpack        payloads, (mode, offset, bytes) per tile -> m planes: every dword gathers the positions of its 32
//                 bits from the ascending list by bisection (no atomics, the result does not depend on any order), or
//                 copies its raw bytes; then the XOR prefix down every 16-bit column strip
//   apply         m planes, (tile, plane or -1 = all set) per tile -> v (uint8 or uint16 HWC, one kernel over the
//                 element type) or v / 255.0f (float32 CHW) at the tile's owned pixels inside the window whose bit is
//                 set; nothing else is written.  All three window writers (and the validity window) open with
//                 window_rows and walk their rows in the chunks of hwc_chunks.h.
//
// What this file shares is stated elsewhere: the grid, its argument checks, kTileRows and a tile's part of a window in
// tile_grid.h; the offsets scan of the pack head in byte_movers.h.  The nodata exports (C = 3, 4) and the validity
// exports (C = 1) are one launcher each, at the end of the file.
#include <limits.h>

#include "byte_movers.h"
#include "hwc_chunks.h"
#include "tile_grid.h"

namespace dsic {

// bit e = pixel e of the 16 at p is nodata; all 16 C bytes are read
template <int C>
__device__ __forceinline__ uint32_t nodata16_full(const uint8_t* __restrict__ p, uint32_t v) {
  uint32_t m = 0;
  if (C == 1) {  // a validity image (csrc/mask.hip, the valid exports): one load gives the 16 plane bits
    const uint4 q = load16_any(p);
    uint8_t b[16];
    __builtin_memcpy(b, &q, 16);
#pragma unroll
    for (int e = 0; e < 16; ++e) m |= (uint32_t)(b[e] == v) << e;
  } else if (C == 4) {
    const uint32_t vv = v * 0x01010101u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint4 q = load16_any(p + 16 * k);
      m |= ((uint32_t)(q.x == vv) | ((uint32_t)(q.y == vv) << 1) | ((uint32_t)(q.z == vv) << 2) |
            ((uint32_t)(q.w == vv) << 3))
           << (4 * k);
    }
  } else {
    const uint4 q[3] = {load16_any(p), load16_any(p + 16), load16_any(p + 32)};
    uint8_t b[48];
    __builtin_memcpy(b, q, 48);
#pragma unroll
    for (int e = 0; e < 16; ++e)
      m |= (uint32_t)(b[3 * e] == v && b[3 * e + 1] == v && b[3 * e + 2] == v) << e;
  }
  return m;
}

// The 16 mask bits of row y, columns [16 s, 16 s + 16) of the tile that owns `o`, in tile coordinates: a bit is set
// iff the pixel is owned, inside H x W (o is cut to it) and nodata.
template <int C>
__device__ __forceinline__ uint32_t mask16(const uint8_t* __restrict__ img, int W, const Owned& o, uint32_t v, int y,
                                           int s) {
  const int iy = o.oy + y, ix0 = o.ox + 16 * s;
  if (iy < o.y0 || iy >= o.y1) return 0;
  const int lo = max(o.x0, ix0), hi = min(o.x1, ix0 + 16);
  if (lo >= hi) return 0;
  const uint8_t* row = img + ((int64_t)iy * W + ix0) * C;
  if (hi - lo == 16) return nodata16_full<C>(row, v);
  uint32_t m = 0;
  for (int x = lo; x < hi; ++x) {
    const uint8_t* p = row + (x - ix0) * C;
    bool e = true;
#pragma unroll
    for (int c = 0; c < C; ++c) e = e && p[c] == v;
    m |= (uint32_t)e << (x - ix0);
  }
  return m;
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;  // in lane 0
}

// blockIdx.y = tile first + blockIdx.y, blockIdx.x = a block of kTileRows of its rows; counts[blockIdx.y] += nodata
template <int C>
__global__ __launch_bounds__(256) void mask_classify_kernel(const uint8_t* __restrict__ img, Grid g, uint32_t v,
                                                            int first, int* __restrict__ counts) {
  const Owned o = owned(g, first + blockIdx.y);
  const int S = g.tw >> 4, r0 = blockIdx.x * kTileRows;
  int cnt = 0;
  for (int i = threadIdx.x; i < kTileRows * S; i += blockDim.x) {
    const int r = i / S;
    cnt += __popc(mask16<C>(img, g.W, o, v, r0 + r, i - r * S));
  }
  cnt = wave_sum(cnt);
  if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(counts + blockIdx.y, cnt);
}

// blockIdx.y = tile ids[blockIdx.y]; a thread makes one dword of its d plane: halves 2w and 2w + 1, half h = row
// h / S, strip h % S (S = tw / 16)
template <int C>
__global__ __launch_bounds__(256) void mask_delta_kernel(const uint8_t* __restrict__ img, Grid g, uint32_t v,
                                                         const int* __restrict__ ids, uint32_t* __restrict__ planes,
                                                         int* __restrict__ pop) {
  const int t = ids[blockIdx.y];
  const int D = (g.th * g.tw) >> 5, S = g.tw >> 4;
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t d = 0;
  if (w < D && t >= 0 && t < g.ny * g.nx) {
    const Owned o = owned(g, t);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int h = 2 * w + k, y = h / S, s = h - y * S;
      const uint32_t m = mask16<C>(img, g.W, o, v, y, s) ^ (y ? mask16<C>(img, g.W, o, v, y - 1, s) : 0u);
      d |= m << (16 * k);
    }
  }
  if (w < D) planes[(size_t)blockIdx.y * D + w] = d;
  const int cnt = wave_sum(__popc(d));
  if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(pop + blockIdx.y, cnt);
}

// ---- pack: records and payloads of the mixed tiles in one buffer ----------------------------------------------------
// out: n x (tile u32, mode u32, bytes u32) | the n payloads back to back.  ws[0] = bytes of all that, ws[1] = 0,
// ws[2 + t] = offset of payload t behind the records.
constexpr int kMaskRec = 12;
__host__ __device__ inline int pos_bytes(int64_t bits) { return bits <= 65536 ? 2 : 4; }
__device__ __forceinline__ int64_t list_bytes(const int* pop, int t, int64_t bits) {
  const int64_t p = pop[t] < 0 ? 0 : (pop[t] > bits ? bits : pop[t]);
  return p * pos_bytes(bits);
}
__device__ __forceinline__ int64_t payload_bytes(const int* pop, int t, int64_t bits, int* mode) {
  const int64_t raw = bits >> 3, list = list_bytes(pop, t, bits);
  *mode = list < raw;
  return *mode ? list : raw;
}

__global__ __launch_bounds__(256) void mask_pack_head_kernel(const int* __restrict__ pop, const int* __restrict__ ids,
                                                             int n, int64_t bits, long long* __restrict__ ws,
                                                             uint8_t* __restrict__ out) {
  __shared__ long long lds4[4];
  const int tid = threadIdx.x;
  for (int i = tid; i < kMaskRec * n; i += blockDim.x) {
    const int t = i / kMaskRec, k = i - t * kMaskRec;
    int mode;
    const int64_t bytes = payload_bytes(pop, t, bits, &mode);
    const uint32_t f[3] = {(uint32_t)ids[t], (uint32_t)mode, (uint32_t)bytes};
    put_u32(out + i, k & 3, f[k >> 2]);
  }
  const long long total = scan_offsets(
      n,
      [&](int t) {
        int mode;
        return payload_bytes(pop, t, bits, &mode);
      },
      lds4, ws + 2);
  if (tid == 0) ws[0] = (long long)kMaskRec * n + total, ws[1] = 0;
}

// blockIdx.y = tile, blockIdx.x = slice of a raw plane; a list is written by slice 0 alone, in order: the scan gives
// every dword the rank of its first set bit
__global__ __launch_bounds__(256) void mask_pack_payload_kernel(const uint32_t* __restrict__ planes,
                                                                const int* __restrict__ pop, int n, int64_t bits,
                                                                const long long* __restrict__ ws,
                                                                uint8_t* __restrict__ out) {
  __shared__ long long lds4[4];
  const int t = blockIdx.y, D = (int)(bits >> 5);
  int mode;
  const int64_t bytes = payload_bytes(pop, t, bits, &mode);
  const uint32_t* plane = planes + (size_t)t * D;
  uint8_t* dst = out + (int64_t)kMaskRec * n + ws[2 + t];
  if (!mode) {
    copy_bytes(dst, (const uint8_t*)plane, bytes, blockIdx.x, gridDim.x);
    return;
  }
  if (blockIdx.x) return;
  const int ps = pos_bytes(bits);
  const long long count = bytes / ps;
  long long carry = 0;
  for (int w0 = 0; w0 < D; w0 += blockDim.x) {
    const int w = w0 + threadIdx.x;
    uint32_t v = w < D ? plane[w] : 0u;
    long long tot;
    long long idx = carry + block_exclusive_scan(__popc(v), lds4, &tot);
    carry += tot;
    for (; v && idx < count; v &= v - 1, ++idx) {  // payload offsets are multiples of the position size
      const uint32_t pos = 32u * (uint32_t)w + (uint32_t)(__ffs((int)v) - 1);
      if (ps == 2) *(uint16_t*)(dst + 2 * idx) = (uint16_t)pos;
      else *(uint32_t*)(dst + 4 * idx) = pos;
    }
  }
}

// ---- unpack: payloads -> m planes ---------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t get_pos(const uint8_t* p, int ps) {
  uint32_t v = (uint32_t)p[0] | ((uint32_t)p[1] << 8);
  if (ps == 4) v |= ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
  return v;
}

// One workgroup per tile.  desc [n][3] = (mode, offset of the payload in blob, its bytes).  A payload that cannot be
// a tile's (the host has checked: a bad mode or length, or one that leaves the blob) gives the empty plane, and a
// position outside the plane sets nothing.
__global__ __launch_bounds__(256) void mask_unpack_kernel(const uint8_t* __restrict__ blob, int64_t blob_bytes,
                                                          const int* __restrict__ desc, int th, int tw,
                                                          uint32_t* __restrict__ planes) {
  __shared__ uint16_t part[256];
  const int t = blockIdx.x, tid = threadIdx.x;
  const int64_t bits = (int64_t)th * tw, raw = bits >> 3;
  const int D = (int)(bits >> 5), S = tw >> 4, ps = pos_bytes(bits);
  const int mode = desc[3 * t];
  const int64_t off = desc[3 * t + 1], bytes = desc[3 * t + 2];
  const bool in_blob = off >= 0 && bytes >= 0 && off + bytes <= blob_bytes;
  uint32_t* plane = planes + (size_t)t * D;
  const uint8_t* src = blob + off;
  if (in_blob && mode == 0 && bytes == raw) {
    copy_bytes((uint8_t*)plane, src, raw, 0, 1);
  } else {
    const int count = in_blob && mode == 1 && bytes % ps == 0 && bytes < raw ? (int)(bytes / ps) : 0;
    for (int w = tid; w < D; w += blockDim.x) {
      int lo = 0, hi = count;  // the first position that is not below 32 w
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (get_pos(src + (int64_t)mid * ps, ps) < 32u * (uint32_t)w) lo = mid + 1;
        else hi = mid;
      }
      uint32_t v = 0;
      for (int k = 0; k < 32 && lo < count; ++k, ++lo) {
        const uint32_t pos = get_pos(src + (int64_t)lo * ps, ps);
        if (pos >= 32u * (uint32_t)w + 32u) break;
        v |= 1u << (pos & 31);
      }
      plane[w] = v;
    }
  }
  __syncthreads();
  // m[y] = m[y-1] ^ d[y] down every strip of 16 columns: thread (r, s) folds the rows of group r of strip s, the
  // groups' folds meet in LDS, and the second pass writes m over d
  uint16_t* h = (uint16_t*)plane;
  const int G = min(256 / S, th), R = (th + G - 1) / G;
  const int s = tid % S, r = tid / S;
  const int ya = min(r * R, th), yb = r < G ? min(ya + R, th) : ya;
  uint16_t x = 0;
  for (int y = ya; y < yb; ++y) x ^= h[(size_t)y * S + s];
  part[tid] = x;
  __syncthreads();
  uint16_t acc = 0;
  for (int k = 0; k < r && k < G; ++k) acc ^= part[k * S + s];
  for (int y = ya; y < yb; ++y) {
    acc ^= h[(size_t)y * S + s];
    h[(size_t)y * S + s] = acc;
  }
}

// ---- apply: v at the pixels whose bit is set ------------------------------------------------------------------------
// desc [n][2] = (tile, plane index or -1 for "all set").  What workgroup (blockIdx.x, blockIdx.y) of a window writer
// works on: o, the part of tile desc[blockIdx.y][0] the call writes (owned_in_window of tile_grid.h); its rows
// [ya, ya + rows) of that part; the tile's m plane, null for "all set"; and wW, the window's width in pixels.  False
// where there is nothing to write: a tile outside the grid, a plane index >= n_planes, an empty part, no rows.
struct WindowRows {
  Owned o;
  int ya, rows, wW;
  const uint32_t* plane;
};
__device__ __forceinline__ bool window_rows(const uint32_t* planes, const int* desc, int n_planes, const Grid& g,
                                            const Clip& w, WindowRows* r) {
  const int pi = desc[2 * blockIdx.y + 1];
  if (pi >= n_planes || !owned_in_window(g, desc[2 * blockIdx.y], w, &r->o)) return false;
  r->ya = r->o.y0 + blockIdx.x * kTileRows;
  r->rows = min(kTileRows, r->o.y1 - r->ya);
  r->wW = w.x1 - w.x0;
  r->plane = pi < 0 ? nullptr : planes + (size_t)pi * ((g.th * g.tw) >> 5);
  return r->rows > 0;
}

__device__ __forceinline__ bool mask_bit(const uint32_t* plane, int idx) {
  return !plane || ((plane[idx >> 5] >> (idx & 31)) & 1u);
}

// HWC window of T (uint8_t or uint16_t) at any element alignment: `mis` is the window image's offset behind a 16-byte
// boundary in elements (hwc_chunks.h).  A chunk whose every element is selected is one dwordx4 store of v, any other
// stores v at its selected elements.
template <typename T>
__global__ __launch_bounds__(256) void mask_apply_hwc_kernel(const uint32_t* __restrict__ planes,
                                                             const int* __restrict__ desc, int n_planes, Grid g, int C,
                                                             Clip w, T* __restrict__ img, uint32_t v, int mis) {
  constexpr int E = 16 / (int)sizeof(T);
  WindowRows R;
  if (!window_rows(planes, desc, n_planes, g, w, &R)) return;
  const Owned& o = R.o;
  const int seg = (o.x1 - o.x0) * C;
  const int cpr = seg / E + 2;  // 16-byte chunks a row segment can touch
  const uint32_t vv = v * (sizeof(T) == 1 ? 0x01010101u : 0x00010001u);
  for (int i = threadIdx.x; i < R.rows * cpr; i += blockDim.x) {
    const int r = i / cpr, k = i - r * cpr;
    const int y = R.ya + r;
    const int64_t b0 = ((int64_t)(y - w.y0) * R.wW + (o.x0 - w.x0)) * C + mis;
    Chunk ch;
    if (!row_chunk<T>(b0, seg, k, &ch)) continue;
    HwcCursor u = hwc_cursor(ch.lo() - b0, C);
    u.px += o.x0 - o.ox;  // column within the tile
    const int row_bit = (y - o.oy) * g.tw;
    uint32_t sel = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      if (ch.has(e)) {
        sel |= (uint32_t)mask_bit(R.plane, row_bit + (int)u.px) << e;
        u.step(C);
      }
    }
    if (sel == (1u << E) - 1u) {
      *(uint4*)(img + (ch.q0 - mis)) = make_uint4(vv, vv, vv, vv);
    } else {
#pragma unroll
      for (int e = 0; e < E; ++e)
        if ((sel >> e) & 1u) img[ch.q0 + e - mis] = (T)v;
    }
  }
}

// float32 CHW window; blockIdx.z = channel
__global__ __launch_bounds__(256) void mask_apply_f32_kernel(const uint32_t* __restrict__ planes,
                                                             const int* __restrict__ desc, int n_planes, Grid g,
                                                             Clip w, float* __restrict__ img, float fv) {
  WindowRows R;
  if (!window_rows(planes, desc, n_planes, g, w, &R)) return;
  const Owned& o = R.o;
  const int64_t cplane = (int64_t)blockIdx.z * (w.y1 - w.y0) * R.wW;
  const int seg = o.x1 - o.x0;
  const int cpr = seg / 4 + 2;  // 4-float chunks a row segment can touch; the window is 16-byte aligned, mis = 0
  for (int i = threadIdx.x; i < R.rows * cpr; i += blockDim.x) {
    const int r = i / cpr, k = i - r * cpr;
    const int y = R.ya + r;
    const int64_t b0 = cplane + (int64_t)(y - w.y0) * R.wW + (o.x0 - w.x0);
    Chunk ch;
    if (!row_chunk<float>(b0, seg, k, &ch)) continue;
    const int bit0 = (y - o.oy) * g.tw + (o.x0 - o.ox) + (int)(ch.lo() - b0);
    uint32_t sel = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (ch.has(e)) sel |= (uint32_t)mask_bit(R.plane, bit0 + e - ch.first) << e;
    if (sel == 0xFu) {
      *(float4*)(img + ch.q0) = make_float4(fv, fv, fv, fv);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if ((sel >> e) & 1u) img[ch.q0 + e] = fv;
    }
  }
}

// The validity window, uint8 [h][w] at any alignment (`mis` in bytes): every owned pixel of the listed tiles inside
// the window gets 0 where its bit is set (or the plane is -1, all set) and 1 elsewhere; no other byte is written.
__global__ __launch_bounds__(256) void mask_window_u8_kernel(const uint32_t* __restrict__ planes,
                                                             const int* __restrict__ desc, int n_planes, Grid g, Clip w,
                                                             uint8_t* __restrict__ out, int mis) {
  WindowRows R;
  if (!window_rows(planes, desc, n_planes, g, w, &R)) return;
  const Owned& o = R.o;
  const int seg = o.x1 - o.x0;
  const int cpr = seg / 16 + 2;  // 16-byte chunks a row segment can touch
  for (int i = threadIdx.x; i < R.rows * cpr; i += blockDim.x) {
    const int r = i / cpr, k = i - r * cpr;
    const int y = R.ya + r;
    const int64_t b0 = (int64_t)(y - w.y0) * R.wW + (o.x0 - w.x0) + mis;
    Chunk ch;
    if (!row_chunk<uint8_t>(b0, seg, k, &ch)) continue;
    const int bit0 = (y - o.oy) * g.tw + (o.x0 - o.ox) + (int)(ch.lo() - b0);
    uint8_t b[16];
#pragma unroll
    for (int e = 0; e < 16; ++e)
      b[e] = ch.has(e) ? (uint8_t)!mask_bit(R.plane, bit0 + e - ch.first) : (uint8_t)0;
    store_chunk<uint8_t>(out, mis, ch.q0, ch.lo(), ch.hi(), b);
  }
}

}  // namespace dsic

// ---- exports --------------------------------------------------------------------------------------------------------
// The grid, tile-range and window checks are tile_grid.h's (DSIC_GRID, DSIC_TILE_ARGS, DSIC_WINDOW_ARGS).  What is the
// mask calls' alone stands here once: a tile's bit positions are ints, so a tile has at most 2^30 pixels, and a window
// writer takes n_planes >= 0 planes, at a non-null pointer unless there are none.
namespace dsic {

static int tile_pixels_ok(const char* what, int th, int tw) {
  DSIC_REQUIRE((int64_t)th * tw <= INT_MAX / 2, "%s: a tile of %dx%d has over 2^30 pixels", what, th, tw);
  return DSIC_OK;
}

static int window_planes_ok(const char* what, int th, int tw, const uint32_t* planes, int n_planes) {
  DSIC_REQUIRE(n_planes >= 0 && (planes || n_planes == 0), "%s: %d planes at a null pointer", what, n_planes);
  return tile_pixels_ok(what, th, tw);
}

// classify and delta planes of a C-channel image (C = 3, 4: a uint8 HWC image and its nodata value v; C = 1: a validity
// image, v = 0): every check the nodata and the validity exports share, and the one dispatch on C
static int classify(const char* what, const uint8_t* img, int H, int W, int C, int th, int tw, uint32_t v,
                    int first_tile, int n_tiles, int* counts, void* stream) {
  DSIC_REQUIRE(img && counts, "%s: null pointer", what);
  DSIC_TILE_ARGS(what);
  if (const int rc = tile_pixels_ok(what, th, tw)) return rc;
  DSIC_REQUIRE(((uintptr_t)counts & 3) == 0, "%s: counts must be 4-byte aligned", what);
  const auto kernel = C == 1 ? mask_classify_kernel<1> : (C == 3 ? mask_classify_kernel<3> : mask_classify_kernel<4>);
  hipLaunchKernelGGL(kernel, grid, dim3(256), 0, (hipStream_t)stream, img, g, v, first_tile, counts);
  return check_launch(what);
}

static int delta_planes(const char* what, const uint8_t* img, int H, int W, int C, int th, int tw, uint32_t v,
                        const int* tile_ids, int n_tiles, uint32_t* planes, int* popcounts, void* stream) {
  DSIC_REQUIRE(img && tile_ids && planes && popcounts, "%s: null pointer", what);
  DSIC_GRID(what);
  if (const int rc = tile_pixels_ok(what, th, tw)) return rc;
  DSIC_REQUIRE(n_tiles >= 1 && n_tiles <= 65535, "%s: n=%d tiles per call (1..65535)", what, n_tiles);
  DSIC_REQUIRE((((uintptr_t)planes | (uintptr_t)popcounts | (uintptr_t)tile_ids) & 3) == 0,
               "%s: planes, popcounts and tile ids must be 4-byte aligned", what);
  const auto kernel = C == 1 ? mask_delta_kernel<1> : (C == 3 ? mask_delta_kernel<3> : mask_delta_kernel<4>);
  hipLaunchKernelGGL(kernel, dim3(ceil_div((g.th * g.tw) >> 5, 256), n_tiles), dim3(256), 0, (hipStream_t)stream, img,
                     g, v, tile_ids, planes, popcounts);
  return check_launch(what);
}

}  // namespace dsic

using namespace dsic;

extern "C" int dsic_mask_classify_u8(const uint8_t* img_hwc, int H, int W, int C, int th, int tw, int nodata,
                                     int first_tile, int n_tiles, int* counts, void* stream) {
  DSIC_REQUIRE(C == 3 || C == 4, "mask_classify_u8: C=%d must be 3 or 4", C);
  DSIC_REQUIRE(nodata >= 0 && nodata <= 255, "mask_classify_u8: nodata=%d must be in 0..255", nodata);
  return classify("mask_classify_u8", img_hwc, H, W, C, th, tw, (uint32_t)nodata, first_tile, n_tiles, counts, stream);
}

extern "C" int dsic_mask_delta_planes_u8(const uint8_t* img_hwc, int H, int W, int C, int th, int tw, int nodata,
                                         const int* tile_ids, int n_tiles, uint32_t* planes, int* popcounts,
                                         void* stream) {
  DSIC_REQUIRE(C == 3 || C == 4, "mask_delta_planes_u8: C=%d must be 3 or 4", C);
  DSIC_REQUIRE(nodata >= 0 && nodata <= 255, "mask_delta_planes_u8: nodata=%d must be in 0..255", nodata);
  return delta_planes("mask_delta_planes_u8", img_hwc, H, W, C, th, tw, (uint32_t)nodata, tile_ids, n_tiles, planes,
                      popcounts, stream);
}

// Validity masks (codec.compress_image with valid = mask, stream version 8).  The mask travels as a uint8 [H][W] image,
// 0 = invalid: a one-channel image whose "nodata value" is 0, so classify and the d planes are the C = 1 instantiation
// of the kernels above, with their grid, ownership and plane layout.
extern "C" int dsic_valid_classify(const uint8_t* valid_hw, int H, int W, int th, int tw, int first_tile, int n_tiles,
                                   int* counts, void* stream) {
  return classify("valid_classify", valid_hw, H, W, 1, th, tw, 0u, first_tile, n_tiles, counts, stream);
}

extern "C" int dsic_valid_delta_planes(const uint8_t* valid_hw, int H, int W, int th, int tw, const int* tile_ids,
                                       int n_tiles, uint32_t* planes, int* popcounts, void* stream) {
  return delta_planes("valid_delta_planes", valid_hw, H, W, 1, th, tw, 0u, tile_ids, n_tiles, planes, popcounts,
                      stream);
}

#define DSIC_MASK_TILE(what)                                                                                     \
  DSIC_REQUIRE(th >= 32 && tw >= 32 && th % 16 == 0 && tw % 16 == 0 && tw <= 4096 &&                             \
                   (int64_t)th * tw <= INT_MAX / 2,                                                              \
               what ": tile %dx%d: sides must be multiples of 16 from 32, tw at most 4096, under 2^30 pixels", th, \
               tw);                                                                                              \
  DSIC_REQUIRE(n_tiles >= 1 && n_tiles <= 65535, what ": n=%d tiles per call (1..65535)", n_tiles)

extern "C" int dsic_mask_pack(const uint32_t* planes, const int* popcounts, const int* tile_ids, int n_tiles, int th,
                              int tw, int64_t* workspace, uint8_t* out, void* stream) {
  DSIC_REQUIRE(planes && popcounts && tile_ids && workspace && out, "mask_pack: null pointer");
  DSIC_MASK_TILE("mask_pack");
  DSIC_REQUIRE((((uintptr_t)planes | (uintptr_t)out) & 3) == 0, "mask_pack: planes and out must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  long long* ws = (long long*)workspace;
  const int64_t bits = (int64_t)th * tw;
  hipLaunchKernelGGL(mask_pack_head_kernel, dim3(1), dim3(256), 0, st, popcounts, tile_ids, n_tiles, bits, ws, out);
  const int rc = check_launch("mask_pack(head)");
  if (rc) return rc;
  hipLaunchKernelGGL(mask_pack_payload_kernel, dim3(string_parts(bits >> 3), n_tiles), dim3(256), 0, st, planes,
                     popcounts, n_tiles, bits, (const long long*)ws, out);
  return check_launch("mask_pack(payloads)");
}

extern "C" int dsic_mask_unpack(const uint8_t* blob, int64_t blob_bytes, const int* desc, int n_tiles, int th, int tw,
                                uint32_t* planes, void* stream) {
  DSIC_REQUIRE(blob && desc && planes, "mask_unpack: null pointer");
  DSIC_MASK_TILE("mask_unpack");
  DSIC_REQUIRE(blob_bytes >= 0, "mask_unpack: negative size");
  DSIC_REQUIRE(((uintptr_t)planes & 15) == 0, "mask_unpack: planes must be 16-byte aligned");
  hipLaunchKernelGGL(mask_unpack_kernel, dim3(n_tiles), dim3(256), 0, (hipStream_t)stream, blob, blob_bytes, desc, th,
                     tw, planes);
  return check_launch("mask_unpack");
}

// The window writers: the range of the fill value and of C, the window (leaving g, clip and grid), the planes, then the
// alignments each writer needs.
extern "C" int dsic_mask_apply_u8(const uint32_t* planes, int n_planes, const int* desc, int n_tiles, int nodata,
                                  uint8_t* out, int H, int W, int C, int th, int tw, int wy0, int wx0, int wh, int ww,
                                  void* stream) {
  DSIC_REQUIRE(desc && out, "mask_apply_u8: null pointer");
  DSIC_REQUIRE(C == 3 || C == 4, "mask_apply_u8: C=%d must be 3 or 4", C);
  DSIC_REQUIRE(nodata >= 0 && nodata <= 255, "mask_apply_u8: nodata=%d must be in 0..255", nodata);
  DSIC_WINDOW_ARGS("mask_apply_u8");
  if (const int rc = window_planes_ok("mask_apply_u8", th, tw, planes, n_planes)) return rc;
  DSIC_REQUIRE(((uintptr_t)out & 15) == 0, "mask_apply_u8: out must be 16-byte aligned");
  hipLaunchKernelGGL(mask_apply_hwc_kernel<uint8_t>, grid, dim3(256), 0, (hipStream_t)stream, planes, desc, n_planes,
                     g, C, clip, out, (uint32_t)nodata, 0);
  return check_launch("mask_apply_u8");
}

extern "C" int dsic_mask_apply_f32(const uint32_t* planes, int n_planes, const int* desc, int n_tiles, int nodata,
                                   float* out, int H, int W, int C, int th, int tw, int wy0, int wx0, int wh, int ww,
                                   void* stream) {
  DSIC_REQUIRE(desc && out, "mask_apply_f32: null pointer");
  DSIC_REQUIRE(C >= 1 && C <= 8, "mask_apply_f32: C=%d must be in 1..8", C);
  DSIC_REQUIRE(nodata >= 0 && nodata <= 255, "mask_apply_f32: nodata=%d must be in 0..255", nodata);
  DSIC_WINDOW_ARGS("mask_apply_f32");
  if (const int rc = window_planes_ok("mask_apply_f32", th, tw, planes, n_planes)) return rc;
  DSIC_REQUIRE(((uintptr_t)out & 15) == 0, "mask_apply_f32: out must be 16-byte aligned");
  const float fv = (float)nodata / 255.0f;  // on the host, correctly rounded: NumPy's float32(v) / float32(255)
  hipLaunchKernelGGL(mask_apply_f32_kernel, dim3(grid.x, grid.y, C), dim3(256), 0, (hipStream_t)stream, planes, desc,
                     n_planes, g, clip, out, fv);
  return check_launch("mask_apply_f32");
}

extern "C" int dsic_mask_apply_u16(const uint32_t* planes, int n_planes, const int* desc, int n_tiles, int fill,
                                   uint16_t* out, int H, int W, int C, int th, int tw, int wy0, int wx0, int wh, int ww,
                                   void* stream) {
  DSIC_REQUIRE(desc && out, "mask_apply_u16: null pointer");
  DSIC_REQUIRE(C >= 1 && C <= 4, "mask_apply_u16: C=%d must be in 1..4", C);
  DSIC_REQUIRE(fill >= 0 && fill <= 65535, "mask_apply_u16: fill=%d must be in 0..65535", fill);
  DSIC_REQUIRE(((uintptr_t)out & 1) == 0, "mask_apply_u16: the uint16 window must be 2-byte aligned");
  DSIC_WINDOW_ARGS("mask_apply_u16");
  if (const int rc = window_planes_ok("mask_apply_u16", th, tw, planes, n_planes)) return rc;
  DSIC_REQUIRE((((uintptr_t)planes | (uintptr_t)desc) & 3) == 0,
               "mask_apply_u16: planes and desc must be 4-byte aligned");
  DSIC_REQUIRE((int64_t)ww * C * 2 <= INT_MAX, "mask_apply_u16: a row of ww=%d pixels of C=%d uint16 is over 2^31 - 1 bytes",
               ww, C);
  hipLaunchKernelGGL(mask_apply_hwc_kernel<uint16_t>, grid, dim3(256), 0, (hipStream_t)stream, planes, desc, n_planes,
                     g, C, clip, out, (uint32_t)fill, (int)(((uintptr_t)out & 15) >> 1));
  return check_launch("mask_apply_u16");
}

extern "C" int dsic_mask_window_u8(const uint32_t* planes, int n_planes, const int* desc, int n_tiles, uint8_t* out_hw,
                                   int H, int W, int th, int tw, int wy0, int wx0, int wh, int ww, void* stream) {
  DSIC_REQUIRE(desc && out_hw, "mask_window_u8: null pointer");
  DSIC_WINDOW_ARGS("mask_window_u8");
  if (const int rc = window_planes_ok("mask_window_u8", th, tw, planes, n_planes)) return rc;
  DSIC_REQUIRE((((uintptr_t)planes | (uintptr_t)desc) & 3) == 0,
               "mask_window_u8: planes and desc must be 4-byte aligned");
  hipLaunchKernelGGL(mask_window_u8_kernel, grid, dim3(256), 0, (hipStream_t)stream, planes, desc, n_planes, g, clip,
                     out_hw, (int)((uintptr_t)out_hw & 15));
  return check_launch("mask_window_u8");
}
