// Whole-image codec glue (codec.py): an image of any size to tiles of the model's patch size and back, and a
// batch of coder outputs to one DSIC2 container and back.  All of it is byte movement: every kernel is
// memory-bound and works in 16-byte units (dwordx4 loads where the source is aligned, alignbyte funnels of
// dword loads where it is not, dwordx4 stores on aligned destination chunks, byte stores only at the ragged
// ends of a segment).  One workgroup covers a block of rows of one tile, or a slice of one string.  The stitch and
// the blend finish into an HWC image stand here once for uint8 and uint16 (stitch_hwc_kernel, blend_finish_hwc_kernel
// over the chunk walk of hwc_chunks.h and a value policy per width); image_u16.hip's exports launch them.
//
// Tile geometry (codec.tile_grid): Hp = ceil16(H), tiles_y = ceil(Hp / th), origin of tile row i =
// min(i*th, Hp - th); tile row i owns padded rows [i*th, min((i+1)*th, Hp)) (the last row of tiles shifts
// inward and its overlap rows belong to the earlier tile).  Columns likewise; tiles are numbered row-major.
//
// Overlapped tiles (overlap = O, a multiple of 16 with O <= min(th, tw) / 2): on an axis of more than one tile the
// stride is s = t - O, tiles = ceil((P - O) / s), nominal origin a(i) = i*s, real origin min(i*s, P - t); tile i's
// support is [a(i), a(i+1) + O), the last one's [a(n-1), P).  Over the first O positions of a support (i > 0) the
// tile's weight ramps up as (2k+1)/(2O), over [a(i+1), a(i+1) + O) it ramps down as (2(O-1-k)+1)/(2O), elsewhere in
// the support it is 1: at every position the weights of at most two tiles per axis sum to 1.  O = 0 is the grid above.
#include "byte_movers.h"
#include "hwc_chunks.h"
#include "hwc_launch.h"

namespace dsic {

// ---- tile gather ------------------------------------------------------------------------------------------

// uint8 HWC image -> tiles [n][th][tw][C].  A tile row is tw*C bytes, a multiple of 16.
__global__ __launch_bounds__(256) void gather_u8_kernel(const uint8_t* __restrict__ img, uint8_t* __restrict__ tiles,
                                                        Grid g, int C, int first) {
  const int t = first + blockIdx.y;
  const int oy = g.oy(t / g.nx), ox = g.ox(t % g.nx);
  const int row_bytes = g.tw * C, vpr = row_bytes >> 4;
  const int r0 = blockIdx.x * kTileRows;
  uint8_t* dst = tiles + ((size_t)blockIdx.y * g.th + r0) * row_bytes;
  for (int i = threadIdx.x; i < kTileRows * vpr; i += blockDim.x) {
    const int r = i / vpr, j0 = (i - r * vpr) << 4;
    const uint8_t* src_row = img + (size_t)reflect(oy + r0 + r, g.H) * g.W * C;
    uint4 v;
    if (ox + (j0 + 15) / C < g.W) {
      v = load16_any(src_row + (size_t)ox * C + j0);
    } else {  // the run reaches the reflected columns
      uint8_t b[16];
      int px = j0 / C, c = j0 - px * C;
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        b[k] = src_row[(size_t)reflect(ox + px, g.W) * C + c];
        if (++c == C) c = 0, ++px;
      }
      __builtin_memcpy(&v, b, 16);
    }
    *(uint4*)(dst + (size_t)r * row_bytes + j0) = v;
  }
}

// float32 CHW image -> tiles [n][C][th][tw]; blockIdx.z = channel
__global__ __launch_bounds__(256) void gather_f32_kernel(const float* __restrict__ img, float* __restrict__ tiles,
                                                         Grid g, int first) {
  const int t = first + blockIdx.y, c = blockIdx.z, C = gridDim.z;
  const int oy = g.oy(t / g.nx), ox = g.ox(t % g.nx);
  const int vpr = g.tw >> 2;
  const int r0 = blockIdx.x * kTileRows;
  float* dst = tiles + (((size_t)blockIdx.y * C + c) * g.th + r0) * g.tw;
  for (int i = threadIdx.x; i < kTileRows * vpr; i += blockDim.x) {
    const int r = i / vpr, j0 = (i - r * vpr) << 2;
    const float* src_row = img + ((size_t)c * g.H + reflect(oy + r0 + r, g.H)) * g.W;
    const int x0 = ox + j0;
    float4 v;
    if (x0 + 3 < g.W && (((uintptr_t)(src_row + x0)) & 15) == 0) {
      v = *(const float4*)(src_row + x0);
    } else {
      v = make_float4(src_row[reflect(x0, g.W)], src_row[reflect(x0 + 1, g.W)], src_row[reflect(x0 + 2, g.W)],
                      src_row[reflect(x0 + 3, g.W)]);
    }
    *(float4*)(dst + (size_t)r * g.tw + j0) = v;
  }
}

// ---- tile stitch ------------------------------------------------------------------------------------------

// tiles [n][C][th][tw] -> clamp(0,1) into the float32 CHW window image; blockIdx.z = channel
__global__ __launch_bounds__(256) void stitch_f32_kernel(const float* __restrict__ tiles, float* __restrict__ img,
                                                         Grid g, int first, const int* __restrict__ ids, Clip w) {
  const int c = blockIdx.z, C = gridDim.z;
  Owned o;
  if (!stitch_rect(g, ids, first, w, &o)) return;
  const int ya = o.y0 + blockIdx.x * kTileRows;
  const int rows = min(kTileRows, o.y1 - ya);
  if (rows <= 0) return;
  const float* src = tiles + ((size_t)blockIdx.y * C + c) * g.th * g.tw;
  // 4-float chunks aligned in the image (its base is 16-byte aligned): chunk q covers elements [4q, 4q+4)
  const int wW = w.x1 - w.x0;
  const int64_t plane = (int64_t)c * (w.y1 - w.y0) * wW;
  const int cpr = (o.x1 - o.x0) / 4 + 2;  // chunks a row segment can touch
  for (int i = threadIdx.x; i < rows * cpr; i += blockDim.x) {
    const int r = i / cpr, k = i - r * cpr;
    const int y = ya + r;
    const int64_t e0 = plane + (int64_t)(y - w.y0) * wW + (o.x0 - w.x0), e1 = e0 + (o.x1 - o.x0);
    const int64_t q0 = ((e0 >> 2) + k) << 2;
    if (q0 >= e1) continue;
    const float* srow = src + (size_t)(y - o.oy) * g.tw + (o.x0 - o.ox);  // element e of the image: srow[e - e0]
    if (q0 >= e0 && q0 + 4 <= e1) {
      const float* s = srow + (q0 - e0);
      *(float4*)(img + q0) = make_float4(clamp01(s[0]), clamp01(s[1]), clamp01(s[2]), clamp01(s[3]));
    } else {
      for (int64_t e = max(q0, e0); e < min(q0 + 4, e1); ++e) img[e] = clamp01(srow[e - e0]);
    }
  }
}

__device__ __forceinline__ float min1(float v) { return v > 1.f ? 1.f : v; }

// What the width of an HWC output decides: the value of a decoded sample x of channel c (stitch), that of a blended
// canvas sum v (finish), and the range a value with its residual is clamped to.  Passed to the kernels by value.
template <typename T>
struct HwcValue;
template <>
struct HwcValue<uint8_t> {  // p = (uint8)(clamp(x, 0, 1) * 255)
  static constexpr int kMax = 255;
  __device__ __forceinline__ uint8_t stitch(float x, int) const { return (uint8_t)(clamp01(x) * 255.0f); }
  __device__ __forceinline__ uint8_t finish(float v, int) const { return (uint8_t)(min1(v) * 255.0f); }
};
template <>
struct HwcValue<uint16_t> {  // denorm of u16_scale.h with the band's (lo, R); its clamp is the min(v, 1) of the finish
  static constexpr int kMax = 65535;
  Scale s;
  __device__ __forceinline__ uint16_t stitch(float x, int c) const {
    return denorm_u16(x, pick(s.lo, c), pick(s.R, c));
  }
  __device__ __forceinline__ uint16_t finish(float v, int c) const {
    return denorm_u16(v, pick(s.lo, c), pick(s.R, c));
  }
};

// tiles [n][C][th][tw] -> val.stitch(x) into the HWC window image of T, which lies mis elements behind a 16-byte
// boundary (hwc_chunks.h).  RES (near-lossless streams, residual.hip and residual_u16.hip): q [n][C][th][tw] holds the
// tile's integer residual steps and the value is clamp(p + (int)q * step, 0, kMax), step = 2 tau + 1; |q| is at most
// (kMax + tau) / step as the join kernels leave it, so the sum stays inside int32.
template <typename T, bool RES>
__global__ __launch_bounds__(256) void stitch_hwc_kernel(const float* __restrict__ tiles, const float* __restrict__ q,
                                                         int step, T* __restrict__ img, Grid g, int C, int first,
                                                         const int* __restrict__ ids, Clip w, HwcValue<T> val,
                                                         int mis) {
  constexpr int E = 16 / (int)sizeof(T);
  Owned o;
  if (!stitch_rect(g, ids, first, w, &o)) return;
  const int ya = o.y0 + blockIdx.x * kTileRows;
  const int rows = min(kTileRows, o.y1 - ya);
  if (rows <= 0) return;
  const size_t cplane = (size_t)g.th * g.tw;
  const float* src = tiles + (size_t)blockIdx.y * C * cplane;
  const float* qsrc = RES ? q + (size_t)blockIdx.y * C * cplane : nullptr;
  const int wW = w.x1 - w.x0;
  const int seg = (o.x1 - o.x0) * C;
  const int cpr = seg / E + 2;  // 16-byte chunks a row segment can touch
  for (int i = threadIdx.x; i < rows * cpr; i += blockDim.x) {
    const int r = i / cpr, k = i - r * cpr;
    const int y = ya + r;
    const int64_t b0 = ((int64_t)(y - w.y0) * wW + (o.x0 - w.x0)) * C + mis;
    Chunk ch;
    if (!row_chunk<T>(b0, seg, k, &ch)) continue;
    const size_t row = (size_t)(y - o.oy) * g.tw;
    HwcCursor u = hwc_cursor(ch.lo() - b0, C);
    u.px += o.x0 - o.ox;  // column within the tile
    T b[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      b[e] = 0;
      if (ch.has(e)) {
        const size_t at = u.c * cplane + row + u.px;
        b[e] = val.stitch(src[at], u.c);
        if constexpr (RES) {
          const int v = (int)b[e] + (int)qsrc[at] * step;
          b[e] = (T)(v < 0 ? 0 : (v > val.kMax ? val.kMax : v));
        }
        u.step(C);
      }
    }
    store_chunk<T>(img, mis, ch.q0, ch.lo(), ch.hi(), b);
  }
}

// ---- tile blend (overlapped tiles) -------------------------------------------------------------------------
// A pixel's value is the left fold ((0 + c_a) + c_b) + ... over its contributing tiles in ascending tile number,
// c = (wy * wx) * clamp01(x_tile), all float32 and unfused.  The partial sum travels in the canvas: a call adds the
// contributions of the tiles it holds, and one thread per pixel does so, that of the lowest-numbered contributor
// present.  Calls arrive with ascending tiles, so the order of the additions is the same however the tiles are cut
// into calls.

constexpr int kBlendIds = 64;  // tiles per blend call: the id list is searched in LDS

// The tiles that weigh on padded position p of one axis: lo <= hi (equal outside the ramps), with their weights.
struct Contrib {
  int lo, hi;
  float wlo, whi;
};
__device__ __forceinline__ Contrib contrib(int p, int s, int n, int O, float rcp) {
  const int j = min(p / s, n - 1), k = p - j * s;
  if (j > 0 && k < O) return {j - 1, j, (float)(2 * (O - 1 - k) + 1) * rcp, (float)(2 * k + 1) * rcp};
  return {j, j, 1.f, 1.f};
}

// tiles [n][C][th][tw], ids ascending -> accumulated into the float32 [C][wh][ww] canvas; blockIdx.z = channel
__global__ __launch_bounds__(256) void blend_f32_kernel(const float* __restrict__ tiles, const int* __restrict__ ids,
                                                        int n, float* __restrict__ canvas, Grid g, Clip w, float rcp) {
  __shared__ int s_ids[kBlendIds];
  __shared__ int s_slot[9];  // where the tiles (i-1..i+1, j-1..j+1) lie in this call, -1 = not in it
  const int c = blockIdx.z, C = gridDim.z;
  if ((int)threadIdx.x < n) s_ids[threadIdx.x] = ids[threadIdx.x];
  __syncthreads();
  const int t = s_ids[blockIdx.y];
  if (t < 0 || t >= g.ny * g.nx) return;
  const int i = t / g.nx, j = t % g.nx;
  if (threadIdx.x < 9) {
    const int ii = i + (int)threadIdx.x / 3 - 1, jj = j + (int)threadIdx.x % 3 - 1;
    int slot = -1;
    if (ii >= 0 && ii < g.ny && jj >= 0 && jj < g.nx) {
      const int want = ii * g.nx + jj;
      int lo = 0, hi = n;  // the first entry that is not below want
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s_ids[mid] < want) lo = mid + 1;
        else hi = mid;
      }
      if (lo < n && s_ids[lo] == want) slot = lo;
    }
    s_slot[threadIdx.x] = slot;
  }
  __syncthreads();
  if (s_slot[4] != (int)blockIdx.y) return;  // a tile named twice is blended once, by its first entry
  // the support of tile t, cut to the image and the window
  const int sy0 = max(i * g.sy, w.y0), sy1 = min(min(i < g.ny - 1 ? (i + 1) * g.sy + g.O : g.Hp, g.H), w.y1);
  const int sx0 = max(j * g.sx, w.x0), sx1 = min(min(j < g.nx - 1 ? (j + 1) * g.sx + g.O : g.Wp, g.W), w.x1);
  if (sx0 >= sx1) return;
  const int ya = sy0 + blockIdx.x * kTileRows;
  const int rows = min(kTileRows, sy1 - ya);
  if (rows <= 0) return;
  const size_t cplane = (size_t)g.th * g.tw;
  const float* src = tiles + (size_t)c * cplane;

  // v + the contributions to pixel (y, x) of the tiles of this call, if tile t is the lowest of them
  auto pixel = [&](const Contrib& ay, int y, int x, float* v) -> bool {
    const Contrib ax = contrib(x, g.sx, g.nx, g.O, rcp);
    bool mine = false;
    float acc = *v;
    for (int a = ay.lo == ay.hi ? 1 : 0; a < 2; ++a) {
      const int iy = a ? ay.hi : ay.lo;
      const float wy = a ? ay.whi : ay.wlo;
      for (int b = ax.lo == ax.hi ? 1 : 0; b < 2; ++b) {
        const int ix = b ? ax.hi : ax.lo;
        const int slot = s_slot[(iy - i + 1) * 3 + (ix - j + 1)];
        if (slot < 0) continue;
        if (!mine) {
          if (iy != i || ix != j) return false;
          mine = true;
        }
        const float wgt = wy * (b ? ax.whi : ax.wlo);
        const float x_hat = src[(size_t)slot * C * cplane + (size_t)(y - g.oy(iy)) * g.tw + (x - g.ox(ix))];
        acc = acc + wgt * clamp01(x_hat);
      }
    }
    *v = acc;
    return mine;
  };

  const int wW = w.x1 - w.x0;
  const int64_t plane = (int64_t)c * (w.y1 - w.y0) * wW;
  const int cpr = (sx1 - sx0) / 4 + 2;  // 4-float chunks a row segment can touch
  for (int idx = threadIdx.x; idx < rows * cpr; idx += blockDim.x) {
    const int r = idx / cpr, k = idx - r * cpr;
    const int y = ya + r;
    const int64_t e0 = plane + (int64_t)(y - w.y0) * wW + (sx0 - w.x0), e1 = e0 + (sx1 - sx0);
    const int64_t q0 = ((e0 >> 2) + k) << 2;
    if (q0 >= e1) continue;
    const Contrib ay = contrib(y, g.sy, g.ny, g.O, rcp);
    const int xq = sx0 + (int)(q0 - e0);  // the image column of element q0
    if (q0 >= e0 && q0 + 4 <= e1) {
      float4 v = *(const float4*)(canvas + q0);
      const bool m0 = pixel(ay, y, xq, &v.x), m1 = pixel(ay, y, xq + 1, &v.y), m2 = pixel(ay, y, xq + 2, &v.z),
                 m3 = pixel(ay, y, xq + 3, &v.w);
      if (m0 && m1 && m2 && m3) {
        *(float4*)(canvas + q0) = v;
      } else {  // a ramp begins or ends inside the chunk: the other elements belong to another tile's thread
        if (m0) canvas[q0] = v.x;
        if (m1) canvas[q0 + 1] = v.y;
        if (m2) canvas[q0 + 2] = v.z;
        if (m3) canvas[q0 + 3] = v.w;
      }
    } else {
      for (int64_t e = max(q0, e0); e < min(q0 + 4, e1); ++e) {
        float v = canvas[e];
        if (pixel(ay, y, sx0 + (int)(e - e0), &v)) canvas[e] = v;
      }
    }
  }
}

// min(v, 1) in place: in float32 the four weights of a pixel can sum to 1 + 2 ulp
__global__ __launch_bounds__(256) void blend_finish_f32_kernel(float* __restrict__ canvas, int64_t n) {
  const int64_t n4 = n >> 2, step = (int64_t)gridDim.x * blockDim.x;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t q = tid; q < n4; q += step) {
    float4 v = ((const float4*)canvas)[q];
    v.x = min1(v.x), v.y = min1(v.y), v.z = min1(v.z), v.w = min1(v.w);
    ((float4*)canvas)[q] = v;
  }
  for (int64_t e = 4 * n4 + tid; e < n; e += step) canvas[e] = min1(canvas[e]);
}

// canvas float32 [C][hw] -> val.finish(v) into the [hw][C] image of T, mis elements behind a 16-byte boundary
template <typename T>
__global__ __launch_bounds__(256) void blend_finish_hwc_kernel(const float* __restrict__ canvas, T* __restrict__ out,
                                                               int C, int64_t hw, HwcValue<T> val, int mis) {
  constexpr int E = 16 / (int)sizeof(T);
  const int64_t n = hw * C, nq = flat_chunks<T>(mis, n), step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += step) {
    Chunk ch;
    flat_chunk<T>(mis, n, q, &ch);
    HwcCursor u = hwc_cursor(ch.lo() - mis, C);
    T b[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      b[e] = 0;
      if (ch.has(e)) {
        b[e] = val.finish(canvas[u.c * hw + u.px], u.c);
        u.step(C);
      }
    }
    store_chunk<T>(out, mis, ch.q0, ch.lo(), ch.hi(), b);
  }
}

// The launches of the two kernels above, after the export's own checks; mis follows from the output's address.
template <typename T>
static void launch_stitch(bool res, dim3 grid, hipStream_t st, const float* tiles, const float* q, int step, T* out,
                          const Grid& g, int C, int first, const int* ids, const Clip& clip, HwcValue<T> val) {
  const int mis = (int)(((uintptr_t)out & 15) / sizeof(T));
  if (res)
    hipLaunchKernelGGL((stitch_hwc_kernel<T, true>), grid, dim3(256), 0, st, tiles, q, step, out, g, C, first, ids,
                       clip, val, mis);
  else
    hipLaunchKernelGGL((stitch_hwc_kernel<T, false>), grid, dim3(256), 0, st, tiles, q, step, out, g, C, first, ids,
                       clip, val, mis);
}

template <typename T>
static void launch_blend_finish(hipStream_t st, const float* canvas, T* out, int C, int64_t hw, HwcValue<T> val) {
  const int mis = (int)(((uintptr_t)out & 15) / sizeof(T));
  hipLaunchKernelGGL(blend_finish_hwc_kernel<T>, dim3(flat_blocks(flat_chunks<T>(mis, hw * C))), dim3(256), 0, st,
                     canvas, out, C, hw, val, mis);
}

// for image_u16.hip's exports (declared in hwc_launch.h)
void launch_stitch_u16(bool res, dim3 grid, hipStream_t st, const float* tiles, const float* q, int step, uint16_t* out,
                       const Grid& g, int C, const int* ids, const Clip& clip, const Scale& sc) {
  launch_stitch<uint16_t>(res, grid, st, tiles, q, step, out, g, C, 0, ids, clip, {sc});
}
void launch_blend_finish_u16(hipStream_t st, const float* canvas, uint16_t* out, int C, int64_t hw, const Scale& sc) {
  launch_blend_finish<uint16_t>(st, canvas, out, C, hw, {sc});
}

// ---- DSIC2 container --------------------------------------------------------------------------------------
// magic(6) | tag u32 | B,My,Hy,Wy,Nz,Hz,Wz u32 | B x (min_y,max_y,min_z,max_z i32, len_z,len_y u32) | strings
// DSIC3 (K > 1 segments per y string): magic "DSIC3\0" | the same fields | segs u32 | the same records (len_y = the sum
// of the segments) | B x K u32 segment lengths | per image the z string, then the K segments
constexpr int kHeadBytes = 38, kRecBytes = 24;
__host__ __device__ inline int head_bytes(int K) { return K > 1 ? kHeadBytes + 4 : kHeadBytes; }
__host__ __device__ inline int64_t body_offset(int B, int K) {
  return head_bytes(K) + (int64_t)kRecBytes * B + (K > 1 ? (int64_t)4 * B * K : 0);
}

// one workgroup: header, records, exclusive scan of the B (1 + K) string lengths (z0, y0 segments, z1, ...) into
// ws[2..2+B(1+K)]; ws[0] = container bytes, ws[1] = the coder's error word.  lengths [B][1 + K], cap_y the capacity of
// one y segment; K = 1 writes DSIC2.
__global__ __launch_bounds__(256) void pack_head_kernel(const int* __restrict__ lengths, const int* __restrict__ meta,
                                                        const int* __restrict__ err, int B, int K, int64_t cap_z,
                                                        int64_t cap_y, uint32_t tag, int My, int Hy, int Wy, int Nz,
                                                        int Hz, int Wz, long long* __restrict__ ws,
                                                        uint8_t* __restrict__ out) {
  __shared__ long long lds4[4];
  const int tid = threadIdx.x;
  const int hb = head_bytes(K), S = 1 + K;
  if (tid < hb) {
    const char magic[6] = {'D', 'S', 'I', 'C', K > 1 ? '3' : '2', 0};
    const uint32_t f[9] = {tag, (uint32_t)B, (uint32_t)My, (uint32_t)Hy, (uint32_t)Wy, (uint32_t)Nz, (uint32_t)Hz,
                           (uint32_t)Wz, (uint32_t)K};
    if (tid < 6) out[tid] = (uint8_t)magic[tid];
    else put_u32(out + tid, (tid - 6) & 3, f[(tid - 6) >> 2]);
  }
  for (int i = tid; i < kRecBytes * B; i += blockDim.x) {
    const int b = i / kRecBytes, k = i - b * kRecBytes;
    const int* m = meta + 4 * b;
    uint32_t v;
    switch (k >> 2) {
      case 0: v = (uint32_t)m[0]; break;
      case 1: v = (uint32_t)(m[0] + m[1] - 1); break;
      case 2: v = (uint32_t)m[2]; break;
      case 3: v = (uint32_t)(m[2] + m[3] - 1); break;
      case 4: v = (uint32_t)clamp_len(lengths[S * b], cap_z); break;
      default:
        v = 0;
        for (int j = 1; j <= K; ++j) v += (uint32_t)clamp_len(lengths[S * b + j], cap_y);
        break;
    }
    put_u32(out + hb + i, k & 3, v);
  }
  if (K > 1) {
    for (int i = tid; i < 4 * B * K; i += blockDim.x) {
      const int e = i >> 2, b = e / K, j = e - b * K;
      put_u32(out + hb + (int64_t)kRecBytes * B + i, i & 3, (uint32_t)clamp_len(lengths[S * b + 1 + j], cap_y));
    }
  }
  const long long total =
      scan_offsets(S * B, [&](int s) { return clamp_len(lengths[s], (s % S) ? cap_y : cap_z); }, lds4, ws + 2);
  if (tid == 0) {
    ws[2 + S * B] = total;
    ws[0] = body_offset(B, K) + total;
    ws[1] = err ? *err : 0;
  }
}

// blockIdx.y = string s (image s / (1 + K); the z string, then the K segments); blockIdx.x = slice of it
__global__ __launch_bounds__(256) void pack_strings_kernel(const uint8_t* __restrict__ bytes,
                                                           const int* __restrict__ lengths, int B, int K,
                                                           int64_t cap_z, int64_t cap_y,
                                                           const long long* __restrict__ ws,
                                                           uint8_t* __restrict__ out) {
  const int s = blockIdx.y, b = s / (1 + K), j = s - b * (1 + K);
  const uint8_t* src = bytes + (size_t)b * (cap_z + K * cap_y) + (j ? cap_z + (int64_t)(j - 1) * cap_y : 0);
  const int64_t n = clamp_len(lengths[s], j ? cap_y : cap_z);
  copy_bytes(out + body_offset(B, K) + ws[2 + s], src, n, blockIdx.x, gridDim.x);
}

__device__ __forceinline__ uint32_t get_u32(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// one workgroup: records -> meta [B,4] (ymin, Ly, zmin, Lz), lengths [B,2] (z, y), string offsets ws[2..2+2B]
__global__ __launch_bounds__(256) void scatter_head_kernel(const uint8_t* __restrict__ blob, int B,
                                                           int* __restrict__ lengths, int* __restrict__ meta,
                                                           long long* __restrict__ ws) {
  __shared__ long long lds4[4];
  const int tid = threadIdx.x;
  for (int b = tid; b < B; b += blockDim.x) {
    const uint8_t* rec = blob + kHeadBytes + (size_t)kRecBytes * b;
    const int min_y = (int)get_u32(rec), max_y = (int)get_u32(rec + 4);
    const int min_z = (int)get_u32(rec + 8), max_z = (int)get_u32(rec + 12);
    meta[4 * b] = min_y, meta[4 * b + 1] = max_y - min_y + 1;
    meta[4 * b + 2] = min_z, meta[4 * b + 3] = max_z - min_z + 1;
  }
  const long long total = scan_offsets(  // a length is stored as it is read: the thread of string s keeps lengths[s]
      2 * B,
      [&](int s) {
        const uint32_t len = get_u32(blob + kHeadBytes + (size_t)kRecBytes * (s >> 1) + 16 + 4 * (s & 1));
        lengths[s] = (int)len;
        return len;
      },
      lds4, ws + 2);
  if (tid == 0) ws[2 + 2 * B] = total, ws[0] = kHeadBytes + (long long)kRecBytes * B + total, ws[1] = 0;
}

__global__ __launch_bounds__(256) void scatter_strings_kernel(const uint8_t* __restrict__ blob, int64_t blob_bytes,
                                                              int B, uint8_t* __restrict__ zbuf, int64_t zstride,
                                                              uint8_t* __restrict__ ybuf, int64_t ystride,
                                                              const int* __restrict__ lengths,
                                                              const long long* __restrict__ ws) {
  const int s = blockIdx.y, b = s >> 1, which = s & 1;
  const int64_t stride = which ? ystride : zstride;
  const int64_t off = kHeadBytes + (int64_t)kRecBytes * B + ws[2 + s];
  int64_t n = clamp_len(lengths[s], stride);  // the host checked the records; a bad blob still stays in bounds
  if (off + n > blob_bytes) n = blob_bytes - off;
  copy_bytes((which ? ybuf : zbuf) + (size_t)b * stride, blob + off, n, blockIdx.x, gridDim.x);
}

// The same for strings picked from several containers: blob holds the selected byte spans back to back, desc
// [n][4] = (z offset, z length, y offset, y length) inside it.  blockIdx.y = string s (tile s/2 of the batch, z if
// even, y if odd).  A descriptor that points outside the blob or past the row moves fewer bytes, never other ones.
__global__ __launch_bounds__(256) void scatter_select_kernel(const uint8_t* __restrict__ blob, int64_t blob_bytes,
                                                             const long long* __restrict__ desc,
                                                             uint8_t* __restrict__ zbuf, int64_t zstride,
                                                             uint8_t* __restrict__ ybuf, int64_t ystride,
                                                             int* __restrict__ lengths) {
  const int s = blockIdx.y, b = s >> 1, which = s & 1;
  const int64_t stride = which ? ystride : zstride;
  const int64_t off = desc[4 * b + 2 * which], len = desc[4 * b + 2 * which + 1];
  int64_t n = len < 0 ? 0 : (len > stride ? stride : len);
  if (off < 0 || off > blob_bytes) n = 0;
  else if (n > blob_bytes - off) n = blob_bytes - off;
  if (blockIdx.x == 0 && threadIdx.x == 0) lengths[s] = (int)n;
  copy_bytes((which ? ybuf : zbuf) + (size_t)b * stride, blob + off, n, blockIdx.x, gridDim.x);
}

}  // namespace dsic

// ---- exports ----------------------------------------------------------------------------------------------
// An export with and without _ov, or with and without _res, is one body; `what` is the export's name in its messages.
namespace dsic {

static int gather_u8(const char* what, const uint8_t* img_hwc, uint8_t* tiles, int H, int W, int C, int th, int tw,
                     int overlap, int first_tile, int n_tiles, void* stream) {
  DSIC_REQUIRE(img_hwc && tiles, "%s: null pointer", what);
  DSIC_REQUIRE(C == 3 || C == 4, "%s: C=%d must be 3 or 4", what, C);
  DSIC_TILE_ARGS_OV(what, overlap);
  DSIC_REQUIRE(((uintptr_t)tiles & 15) == 0, "%s: tiles must be 16-byte aligned", what);
  hipLaunchKernelGGL(gather_u8_kernel, grid, dim3(256), 0, (hipStream_t)stream, img_hwc, tiles, g, C, first_tile);
  return check_launch(what);
}

static int gather_f32(const char* what, const float* img_chw, float* tiles, int H, int W, int C, int th, int tw,
                      int overlap, int first_tile, int n_tiles, void* stream) {
  DSIC_REQUIRE(img_chw && tiles, "%s: null pointer", what);
  DSIC_REQUIRE(C >= 1 && C <= 8, "%s: C=%d must be in 1..8", what, C);
  DSIC_TILE_ARGS_OV(what, overlap);
  DSIC_REQUIRE(((uintptr_t)tiles & 15) == 0, "%s: tiles must be 16-byte aligned", what);
  hipLaunchKernelGGL(gather_f32_kernel, dim3(grid.x, grid.y, C), dim3(256), 0, (hipStream_t)stream, img_chw, tiles,
                     g, first_tile);
  return check_launch(what);
}

// q == nullptr stands for "no residual" only where res is false
static int stitch_window_u8(const char* what, bool res, const float* tiles, const float* q, int tau,
                            const int* tile_ids, int n_tiles, uint8_t* out, int H, int W, int C, int th, int tw,
                            int wy0, int wx0, int wh, int ww, void* stream) {
  DSIC_REQUIRE(tiles && (q || !res) && tile_ids && out, "%s: null pointer", what);
  DSIC_REQUIRE(C == 3 || C == 4, "%s: C=%d must be 3 or 4", what, C);
  DSIC_REQUIRE(!res || (tau >= 0 && tau <= 127), "%s: tau=%d must be in 0..127", what, tau);
  DSIC_WINDOW_ARGS(what);
  DSIC_REQUIRE(((uintptr_t)out & 15) == 0, "%s: out must be 16-byte aligned", what);
  launch_stitch<uint8_t>(res, grid, (hipStream_t)stream, tiles, q, 2 * tau + 1, out, g, C, 0, tile_ids, clip, {});
  return check_launch(what);
}

}  // namespace dsic

using namespace dsic;

extern "C" int dsic_tile_gather_u8_ov(const uint8_t* img_hwc, uint8_t* tiles, int H, int W, int C, int th, int tw,
                                      int overlap, int first_tile, int n_tiles, void* stream) {
  return gather_u8("tile_gather_u8_ov", img_hwc, tiles, H, W, C, th, tw, overlap, first_tile, n_tiles, stream);
}

extern "C" int dsic_tile_gather_f32_ov(const float* img_chw, float* tiles, int H, int W, int C, int th, int tw,
                                       int overlap, int first_tile, int n_tiles, void* stream) {
  return gather_f32("tile_gather_f32_ov", img_chw, tiles, H, W, C, th, tw, overlap, first_tile, n_tiles, stream);
}

extern "C" int dsic_tile_gather_u8(const uint8_t* img_hwc, uint8_t* tiles, int H, int W, int C, int th, int tw,
                                   int first_tile, int n_tiles, void* stream) {
  return gather_u8("tile_gather_u8", img_hwc, tiles, H, W, C, th, tw, 0, first_tile, n_tiles, stream);
}

extern "C" int dsic_tile_gather_f32(const float* img_chw, float* tiles, int H, int W, int C, int th, int tw,
                                    int first_tile, int n_tiles, void* stream) {
  return gather_f32("tile_gather_f32", img_chw, tiles, H, W, C, th, tw, 0, first_tile, n_tiles, stream);
}

extern "C" int dsic_tile_stitch_f32(const float* tiles, float* img_chw, int H, int W, int C, int th, int tw,
                                    int first_tile, int n_tiles, void* stream) {
  DSIC_REQUIRE(tiles && img_chw, "tile_stitch_f32: null pointer");
  DSIC_REQUIRE(C >= 1 && C <= 8, "tile_stitch_f32: C=%d must be in 1..8", C);
  DSIC_TILE_ARGS("tile_stitch_f32");
  DSIC_REQUIRE(((uintptr_t)img_chw & 15) == 0, "tile_stitch_f32: image must be 16-byte aligned");
  hipLaunchKernelGGL(stitch_f32_kernel, dim3(grid.x, grid.y, C), dim3(256), 0, (hipStream_t)stream, tiles, img_chw,
                     g, first_tile, (const int*)nullptr, Clip{0, H, 0, W});
  return check_launch("tile_stitch_f32");
}

extern "C" int dsic_tile_stitch_u8(const float* tiles, uint8_t* img_hwc, int H, int W, int C, int th, int tw,
                                   int first_tile, int n_tiles, void* stream) {
  DSIC_REQUIRE(tiles && img_hwc, "tile_stitch_u8: null pointer");
  DSIC_REQUIRE(C == 3 || C == 4, "tile_stitch_u8: C=%d must be 3 or 4", C);
  DSIC_TILE_ARGS("tile_stitch_u8");
  DSIC_REQUIRE(((uintptr_t)img_hwc & 15) == 0, "tile_stitch_u8: image must be 16-byte aligned");
  launch_stitch<uint8_t>(false, grid, (hipStream_t)stream, tiles, nullptr, 1, img_hwc, g, C, first_tile, nullptr,
                         Clip{0, H, 0, W}, {});
  return check_launch("tile_stitch_u8");
}

extern "C" int dsic_tile_stitch_window_f32(const float* tiles, const int* tile_ids, int n_tiles, float* out, int H,
                                           int W, int C, int th, int tw, int wy0, int wx0, int wh, int ww,
                                           void* stream) {
  DSIC_REQUIRE(tiles && tile_ids && out, "tile_stitch_window_f32: null pointer");
  DSIC_REQUIRE(C >= 1 && C <= 8, "tile_stitch_window_f32: C=%d must be in 1..8", C);
  DSIC_WINDOW_ARGS("tile_stitch_window_f32");
  DSIC_REQUIRE(((uintptr_t)out & 15) == 0, "tile_stitch_window_f32: out must be 16-byte aligned");
  hipLaunchKernelGGL(stitch_f32_kernel, dim3(grid.x, grid.y, C), dim3(256), 0, (hipStream_t)stream, tiles, out, g, 0,
                     tile_ids, clip);
  return check_launch("tile_stitch_window_f32");
}

extern "C" int dsic_tile_stitch_window_u8(const float* tiles, const int* tile_ids, int n_tiles, uint8_t* out, int H,
                                          int W, int C, int th, int tw, int wy0, int wx0, int wh, int ww,
                                          void* stream) {
  return stitch_window_u8("tile_stitch_window_u8", false, tiles, nullptr, 0, tile_ids, n_tiles, out, H, W, C, th, tw,
                          wy0, wx0, wh, ww, stream);
}

extern "C" int dsic_tile_stitch_window_u8_res(const float* tiles, const float* q, int tau, const int* tile_ids,
                                              int n_tiles, uint8_t* out, int H, int W, int C, int th, int tw, int wy0,
                                              int wx0, int wh, int ww, void* stream) {
  return stitch_window_u8("tile_stitch_window_u8_res", true, tiles, q, tau, tile_ids, n_tiles, out, H, W, C, th, tw,
                          wy0, wx0, wh, ww, stream);
}

extern "C" int dsic_tile_blend_window_f32(const float* tiles, const int* tile_ids, int n_tiles, float* canvas, int H,
                                          int W, int C, int th, int tw, int overlap, int wy0, int wx0, int wh, int ww,
                                          void* stream) {
  DSIC_REQUIRE(tiles && tile_ids && canvas, "tile_blend_window_f32: null pointer");
  DSIC_REQUIRE(C >= 1 && C <= 8, "tile_blend_window_f32: C=%d must be in 1..8", C);
  DSIC_GRID_OV("tile_blend_window_f32", overlap);
  DSIC_REQUIRE(wy0 >= 0 && wx0 >= 0 && wh >= 1 && ww >= 1 && (int64_t)wy0 + wh <= H && (int64_t)wx0 + ww <= W,
               "tile_blend_window_f32: window %dx%d at (%d, %d) outside the %dx%d image", wh, ww, wy0, wx0, H, W);
  DSIC_REQUIRE(n_tiles >= 1 && n_tiles <= kBlendIds, "tile_blend_window_f32: n=%d tiles per call (1..%d)", n_tiles,
               kBlendIds);
  DSIC_REQUIRE(((uintptr_t)canvas & 15) == 0, "tile_blend_window_f32: canvas must be 16-byte aligned");
  const float rcp = overlap ? 1.0f / (float)(2 * overlap) : 0.f;
  hipLaunchKernelGGL(blend_f32_kernel, dim3(g.th / kTileRows, n_tiles, C), dim3(256), 0, (hipStream_t)stream, tiles,
                     tile_ids, n_tiles, canvas, g, Clip{wy0, wy0 + wh, wx0, wx0 + ww}, rcp);
  return check_launch("tile_blend_window_f32");
}

extern "C" int dsic_tile_blend_finish_f32(float* canvas, int C, int h, int w, void* stream) {
  DSIC_REQUIRE(canvas, "tile_blend_finish_f32: null pointer");
  DSIC_REQUIRE(C >= 1 && C <= 8, "tile_blend_finish_f32: C=%d must be in 1..8", C);
  DSIC_REQUIRE(h >= 1 && w >= 1, "tile_blend_finish_f32: empty window %dx%d", h, w);
  DSIC_REQUIRE(((uintptr_t)canvas & 15) == 0, "tile_blend_finish_f32: canvas must be 16-byte aligned");
  const int64_t n = (int64_t)C * h * w;
  hipLaunchKernelGGL(blend_finish_f32_kernel, dim3(flat_blocks(n >> 2)), dim3(256), 0, (hipStream_t)stream, canvas,
                     n);
  return check_launch("tile_blend_finish_f32");
}

extern "C" int dsic_tile_blend_finish_u8(const float* canvas, uint8_t* out_hwc, int C, int h, int w, void* stream) {
  DSIC_REQUIRE(canvas && out_hwc, "tile_blend_finish_u8: null pointer");
  DSIC_REQUIRE(C == 3 || C == 4, "tile_blend_finish_u8: C=%d must be 3 or 4", C);
  DSIC_REQUIRE(h >= 1 && w >= 1, "tile_blend_finish_u8: empty window %dx%d", h, w);
  DSIC_REQUIRE(((uintptr_t)out_hwc & 15) == 0, "tile_blend_finish_u8: out must be 16-byte aligned");
  launch_blend_finish<uint8_t>((hipStream_t)stream, canvas, out_hwc, C, (int64_t)h * w, {});
  return check_launch("tile_blend_finish_u8");
}

extern "C" int dsic_container_pack(const uint8_t* bytes, int64_t cap_z, int64_t cap_y, const int* lengths,
                                   const int* meta, const int* err, int B, uint32_t tag, int My, int Hy, int Wy,
                                   int Nz, int Hz, int Wz, int64_t* workspace, uint8_t* out, void* stream) {
  DSIC_REQUIRE(bytes && lengths && meta && workspace && out, "container_pack: null pointer");
  DSIC_REQUIRE(B > 0 && cap_z > 0 && cap_y > 0 && cap_z % 4 == 0 && cap_y % 4 == 0,
               "container_pack: bad shape (B=%d cap_z=%lld cap_y=%lld)", B, (long long)cap_z, (long long)cap_y);
  DSIC_REQUIRE(((uintptr_t)bytes & 3) == 0, "container_pack: bytes must be 4-byte aligned");
  DSIC_REQUIRE(B <= 32767, "container_pack: at most 32767 images per container");
  hipStream_t st = (hipStream_t)stream;
  long long* ws = (long long*)workspace;
  hipLaunchKernelGGL(pack_head_kernel, dim3(1), dim3(256), 0, st, lengths, meta, err, B, 1, cap_z, cap_y, tag, My, Hy,
                     Wy, Nz, Hz, Wz, ws, out);
  const int rc = check_launch("container_pack(head)");
  if (rc) return rc;
  hipLaunchKernelGGL(pack_strings_kernel, dim3(string_parts(cap_z > cap_y ? cap_z : cap_y), 2 * B), dim3(256), 0,
                     st, bytes, lengths, B, 1, cap_z, cap_y, (const long long*)ws, out);
  return check_launch("container_pack(strings)");
}

extern "C" int dsic_container_pack_seg(const uint8_t* bytes, int64_t cap_z, int64_t cap_seg, int segs,
                                       const int* lengths, const int* meta, const int* err, int B, uint32_t tag,
                                       int My, int Hy, int Wy, int Nz, int Hz, int Wz, int64_t* workspace,
                                       uint8_t* out, void* stream) {
  DSIC_REQUIRE(bytes && lengths && meta && workspace && out, "container_pack_seg: null pointer");
  DSIC_REQUIRE(B > 0 && cap_z > 0 && cap_seg > 0 && cap_z % 4 == 0 && cap_seg % 4 == 0,
               "container_pack_seg: bad shape (B=%d cap_z=%lld cap_seg=%lld)", B, (long long)cap_z, (long long)cap_seg);
  DSIC_REQUIRE((segs == 2 || segs == 4 || segs == 8 || segs == 16) && My > 0 && My % segs == 0,
               "container_pack_seg: segments=%d must be 2, 4, 8 or 16 and divide My=%d", segs, My);
  DSIC_REQUIRE(((uintptr_t)bytes & 3) == 0, "container_pack_seg: bytes must be 4-byte aligned");
  DSIC_REQUIRE((int64_t)B * (1 + segs) <= 65535, "container_pack_seg: at most 65535 strings per container");
  hipStream_t st = (hipStream_t)stream;
  long long* ws = (long long*)workspace;
  hipLaunchKernelGGL(pack_head_kernel, dim3(1), dim3(256), 0, st, lengths, meta, err, B, segs, cap_z, cap_seg, tag, My,
                     Hy, Wy, Nz, Hz, Wz, ws, out);
  const int rc = check_launch("container_pack_seg(head)");
  if (rc) return rc;
  hipLaunchKernelGGL(pack_strings_kernel, dim3(string_parts(cap_z > cap_seg ? cap_z : cap_seg), (1 + segs) * B),
                     dim3(256), 0, st, bytes, lengths, B, segs, cap_z, cap_seg, (const long long*)ws, out);
  return check_launch("container_pack_seg(strings)");
}

extern "C" int dsic_container_scatter(const uint8_t* blob, int64_t blob_bytes, int B, int64_t max_len, uint8_t* zbuf,
                                      int64_t zstride, uint8_t* ybuf, int64_t ystride, int* lengths, int* meta,
                                      int64_t* workspace, void* stream) {
  DSIC_REQUIRE(blob && zbuf && ybuf && lengths && meta && workspace, "container_scatter: null pointer");
  DSIC_REQUIRE(B > 0 && blob_bytes >= kHeadBytes + (int64_t)kRecBytes * B, "container_scatter: blob too short for B=%d",
               B);
  DSIC_REQUIRE(zstride > 0 && ystride > 0 && zstride % 4 == 0 && ystride % 4 == 0,
               "container_scatter: strides must be positive multiples of 4");
  DSIC_REQUIRE(B <= 32767, "container_scatter: at most 32767 images per container");
  hipStream_t st = (hipStream_t)stream;
  long long* ws = (long long*)workspace;
  hipLaunchKernelGGL(scatter_head_kernel, dim3(1), dim3(256), 0, st, blob, B, lengths, meta, ws);
  const int rc = check_launch("container_scatter(head)");
  if (rc) return rc;
  hipLaunchKernelGGL(scatter_strings_kernel, dim3(string_parts(max_len), 2 * B), dim3(256), 0, st, blob, blob_bytes,
                     B, zbuf, zstride, ybuf, ystride, (const int*)lengths, (const long long*)ws);
  return check_launch("container_scatter(strings)");
}

extern "C" int dsic_strings_scatter_select(const uint8_t* blob, int64_t blob_bytes, const int64_t* desc, int n,
                                           int64_t max_len, uint8_t* zbuf, int64_t zstride, uint8_t* ybuf,
                                           int64_t ystride, int* lengths, void* stream) {
  DSIC_REQUIRE(blob && desc && zbuf && ybuf && lengths, "strings_scatter_select: null pointer");
  DSIC_REQUIRE(n >= 1 && n <= 32767, "strings_scatter_select: n=%d tiles per call (1..32767)", n);
  DSIC_REQUIRE(blob_bytes >= 0 && max_len >= 0, "strings_scatter_select: negative size");
  DSIC_REQUIRE(zstride > 0 && ystride > 0 && zstride % 4 == 0 && ystride % 4 == 0,
               "strings_scatter_select: strides must be positive multiples of 4");
  DSIC_REQUIRE(((uintptr_t)blob & 15) == 0, "strings_scatter_select: blob must be 16-byte aligned");
  hipLaunchKernelGGL(scatter_select_kernel, dim3(string_parts(max_len), 2 * n), dim3(256), 0, (hipStream_t)stream,
                     blob, blob_bytes, (const long long*)desc, zbuf, zstride, ybuf, ystride, lengths);
  return check_launch("strings_scatter_select");
}
