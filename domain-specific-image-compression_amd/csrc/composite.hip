// Scene stacks (codec.SceneStack.read): n placed windows into one, per output pixel.  include/dsic_hip.h has the
// definition; in short, the candidates of an output pixel are the sources, in list order, whose rect holds it, whose
// validity byte (if the source has a validity window) is not zero there and whose pixel is not the source's nodata
// value in all channels; k is their number.  first / last: the pixel of the first / last candidate.  mean: per band
// (2 S + k) / (2 k), S the sum over the candidates.  median: per band (v[(k - 1) / 2] + v[k / 2] + 1) >> 1 of the
// candidates' sorted values, which for odd k is the middle one.  k = 0: fill.
//
// One launch, no workspace.  The source table (16 entries of two pointers, a rect and a nodata value) travels by value
// in the kernel arguments, so the loop over the sources reads it with scalar loads and is the same in every lane; a
// workgroup owns 4 rows of 64 output pixels and consecutive lanes take consecutive x, so each source row is read as one
// run of validity bytes and one run of pixels, and each output row is stored as one run.
//   pick (first, last): walks the list from its front or its back, reads validity bytes (of a source with a nodata
//     value: its pixel) until a lane has its winner, leaves the loop once every lane of the wave has one, and loads the
//     winner's pixel alone.  With dst_count the walk goes on to the end of the list, still reading no pixel it does not
//     need.
//   mean: one pass, the sums in registers.
//   median: instantiated for lists of up to 4, 8 and 16 sources.  The loop over the sources is unrolled, every slot a
//     register: a candidate's pixel as 16-bit fields, two bands to a word, any other slot all ones (a value no smaller
//     than any sample, so the k candidates sort to the front).  The slots go through Batcher's odd-even merge network
//     with packed 16-bit minima and maxima, two bands at a time, and the two middle slots are picked by compares against
//     constants: no array is indexed by a variable, nothing goes to scratch.
//   rank (max, min; dsic_window_composite_pick_u8 / _u16 alone): a candidate must also have a defined index
//     (render.h's index_value of its bands a and b); the whole pixel of the candidate with the largest or smallest u,
//     the first of equals.  Instantiated and unrolled as the median, every slot a register, in two passes: the
//     validity bytes of the whole list, all in flight together, then per source that passed bands a and b (all bands
//     of one with a nodata value) and the ranking, one unsigned compare, strict, walking front to back.  The winner's
//     pixel is loaded alone.
//   The source plane (dst_source of the pick exports): the id of the winner, 255 for k = 0.  The id of a source rides
//     in the table entry (its last field, unused before); pick is instantiated a second time with the store.
#include "common.h"
#include "render.h"

namespace dsic {

constexpr int COMPOSITE_MAX = 16;
constexpr int COMPOSITE_FIRST = 0, COMPOSITE_LAST = 1, COMPOSITE_MEAN = 2, COMPOSITE_MEDIAN = 3;  // DSIC_COMPOSITE_*
constexpr int COMPOSITE_RANK_MAX = 4, COMPOSITE_RANK_MIN = 5;  // DSIC_COMPOSITE_MAX, _MIN: the pick exports alone
constexpr int COMPOSITE_NO_SOURCE = 255;                       // the source plane where k = 0
constexpr int COMPOSITE_BX = 64, COMPOSITE_BY = 4;  // output pixels of a workgroup: 4 rows of 64

struct CompositeSource {
  const void* px;        // [h][w][C]
  const uint8_t* valid;  // null, or [h][w]
  int dy, dx, h, w, nodata, id;  // id: what the source plane names the source by
};

struct CompositeTable {
  CompositeSource s[COMPOSITE_MAX];
};

typedef unsigned short composite_u16x2 __attribute__((ext_vector_type(2)));

// Whether source e has a candidate at output pixel (i, j); q: that pixel's number inside the source.
// The nodata comparison loads the pixel, the validity byte is looked at first.
template <typename T, int C>
__device__ __forceinline__ bool composite_candidate(const CompositeSource& e, int i, int j, int64_t* q) {
  const int yy = i - e.dy, xx = j - e.dx;
  if ((unsigned)yy >= (unsigned)e.h || (unsigned)xx >= (unsigned)e.w) return false;
  *q = (int64_t)yy * e.w + xx;
  if (e.valid && e.valid[*q] == 0) return false;
  if (e.nodata < 0) return true;
  const T* p = (const T*)e.px + *q * C;
  bool nd = true;
#pragma unroll
  for (int c = 0; c < C; ++c) nd = nd && (int)p[c] == e.nodata;
  return !nd;
}

// the outputs of one pixel: m (or fill, for k = 0), k > 0, k
template <typename T, int C>
__device__ __forceinline__ void composite_store(const uint32_t m[4], int k, int fill, int64_t at, T* __restrict__ dst,
                                                uint8_t* __restrict__ dval, uint8_t* __restrict__ dcnt) {
#pragma unroll
  for (int c = 0; c < C; ++c) dst[at * C + c] = (T)(k ? m[c] : (uint32_t)fill);
  if (dval) dval[at] = (uint8_t)(k > 0);
  if (dcnt) dcnt[at] = (uint8_t)k;
}

#define COMPOSITE_PIXEL_LOOP                                                  \
  for (int64_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {           \
    const int64_t by = blk / bx;                                              \
    const int j = (int)(blk - by * bx) * COMPOSITE_BX + threadIdx.x;          \
    const int64_t i64 = by * COMPOSITE_BY + threadIdx.y;                      \
    const bool live = i64 < oh && j < ow;                                     \
    const int i = (int)i64;                                                   \
    const int64_t at = (int64_t)i * ow + j;

// SRC: with the source plane dsrc (not null then)
template <typename T, int C, bool SRC>
__global__ __launch_bounds__(COMPOSITE_BX* COMPOSITE_BY) void composite_pick_kernel(
    CompositeTable tab, int n, int last, T* __restrict__ dst, uint8_t* __restrict__ dval, uint8_t* __restrict__ dcnt,
    uint8_t* __restrict__ dsrc, int oh, int ow, int fill, int bx, int64_t nblocks) {
  COMPOSITE_PIXEL_LOOP
    const T* win = nullptr;
    int k = 0, wid = COMPOSITE_NO_SOURCE;
    for (int t = 0; t < n; ++t) {
      const CompositeSource& e = tab.s[last ? n - 1 - t : t];
      int64_t q;
      if (live && (dcnt || !win) && composite_candidate<T, C>(e, i, j, &q)) {
        ++k;
        if (!win) {
          win = (const T*)e.px + q * C;
          if constexpr (SRC) wid = e.id;
        }
      }
      if (!dcnt && !__builtin_amdgcn_ballot_w64(live && !win)) break;  // every lane of the wave has its winner
    }
    if (!live) continue;
    uint32_t m[4] = {0u, 0u, 0u, 0u};
    if (win) {
#pragma unroll
      for (int c = 0; c < C; ++c) m[c] = (uint32_t)win[c];
    }
    composite_store<T, C>(m, k, fill, at, dst, dval, dcnt);
    if constexpr (SRC) dsrc[at] = (uint8_t)wid;
  }
}

template <typename T, int C>
__global__ __launch_bounds__(COMPOSITE_BX* COMPOSITE_BY) void composite_mean_kernel(
    CompositeTable tab, int n, T* __restrict__ dst, uint8_t* __restrict__ dval, uint8_t* __restrict__ dcnt, int oh,
    int ow, int fill, int bx, int64_t nblocks) {
  COMPOSITE_PIXEL_LOOP
    if (!live) continue;
    uint32_t S[4] = {0u, 0u, 0u, 0u};
    int k = 0;
    for (int t = 0; t < n; ++t) {
      const CompositeSource& e = tab.s[t];
      int64_t q;
      if (composite_candidate<T, C>(e, i, j, &q)) {
        const T* p = (const T*)e.px + q * C;
        ++k;
#pragma unroll
        for (int c = 0; c < C; ++c) S[c] += (uint32_t)p[c];
      }
    }
    uint32_t m[4] = {0u, 0u, 0u, 0u};
    if (k) {
#pragma unroll
      for (int c = 0; c < C; ++c) m[c] = (2u * S[c] + (uint32_t)k) / (2u * (uint32_t)k);  // 2 * 16 * 65535 + 16 < 2^32
    }
    composite_store<T, C>(m, k, fill, at, dst, dval, dcnt);
  }
}

// Batcher's odd-even merge sort of N = 2^m slots as a list of compare-exchanges (lo, hi), made at compile time
// (N = 4: 5 pairs, 8: 19, 16: 63)
template <int N>
struct CompositeNetwork {
  int count;
  unsigned char lo[N * N / 2], hi[N * N / 2];
};

template <int N>
constexpr CompositeNetwork<N> composite_network() {
  CompositeNetwork<N> net = {};
  for (int p = 1; p < N; p *= 2)
    for (int k = p; k >= 1; k /= 2)
      for (int j = k % p; j + k < N; j += 2 * k)
        for (int i = 0; i < k && i + j + k < N; ++i)
          if ((i + j) / (2 * p) == (i + j + k) / (2 * p)) {
            net.lo[net.count] = (unsigned char)(i + j);
            net.hi[net.count] = (unsigned char)(i + j + k);
            ++net.count;
          }
  return net;
}

// ascending, both 16-bit halves of every slot on their own; step T of the network and those after it, every slot
// number a constant
template <int N, int T = 0>
__device__ __forceinline__ void composite_sort(composite_u16x2 (&v)[N]) {
  constexpr CompositeNetwork<N> net = composite_network<N>();
  if constexpr (T < net.count) {
    constexpr int lo = net.lo[T], hi = net.hi[T];
    const composite_u16x2 a = v[lo], b = v[hi];
    v[lo] = __builtin_elementwise_min(a, b);
    v[hi] = __builtin_elementwise_max(a, b);
    composite_sort<N, T + 1>(v);
  }
}

// slot `at` of the sorted slots, `at` a lane's own number: every slot is read, by its constant number, and the one
// wanted is kept (a chain of selects between loads is rewritten by the compiler into a load at a variable index)
template <int N>
__device__ __forceinline__ composite_u16x2 composite_slot(const composite_u16x2 (&v)[N], int at) {
  uint32_t r = 0u;
#pragma unroll
  for (int s = 0; s < N; ++s) r |= at == s ? __builtin_bit_cast(uint32_t, v[s]) : 0u;
  return __builtin_bit_cast(composite_u16x2, r);
}

template <typename T, int C, int N>
__global__ __launch_bounds__(COMPOSITE_BX* COMPOSITE_BY) void composite_median_kernel(
    CompositeTable tab, int n, T* __restrict__ dst, uint8_t* __restrict__ dval, uint8_t* __restrict__ dcnt, int oh,
    int ow, int fill, int bx) {
  // one workgroup per launch block and no loop around it: the table's scalar loads then stay beside their uses, and
  // the unrolled list does not hold 16 entries in scalar registers at once
  {
    const int64_t blk = blockIdx.x, by = blk / bx;
    const int j = (int)(blk - by * bx) * COMPOSITE_BX + threadIdx.x;
    const int64_t i64 = by * COMPOSITE_BY + threadIdx.y;
    if (i64 >= oh || j >= ow) return;
    const int i = (int)i64;
    const int64_t at = (int64_t)i * ow + j;
    composite_u16x2 a[N], b[N];  // bands 0 and 1, bands 2 and 3
    int k = 0;
#pragma unroll
    for (int t = 0; t < N; ++t) {
      a[t] = b[t] = composite_u16x2{0xFFFF, 0xFFFF};
      if (t < n) {
        const CompositeSource& e = tab.s[t];
        int64_t q;
        if (composite_candidate<T, C>(e, i, j, &q)) {
          const T* p = (const T*)e.px + q * C;
          ++k;
          a[t] = composite_u16x2{(unsigned short)p[0], C > 1 ? (unsigned short)p[C > 1 ? 1 : 0] : (unsigned short)0};
          if (C > 2) b[t] = composite_u16x2{(unsigned short)p[C > 2 ? 2 : 0], C > 3 ? (unsigned short)p[C > 3 ? 3 : 0] : (unsigned short)0};
        }
      }
    }
    uint32_t m[4] = {0u, 0u, 0u, 0u};
    if (k) {
      const int lo = (k - 1) >> 1, hi = k >> 1;  // equal for odd k: (v + v + 1) >> 1 = v
      composite_sort<N>(a);
      const composite_u16x2 al = composite_slot<N>(a, lo), ah = composite_slot<N>(a, hi);
      m[0] = ((uint32_t)al[0] + ah[0] + 1u) >> 1;
      m[1] = ((uint32_t)al[1] + ah[1] + 1u) >> 1;
      if (C > 2) {
        composite_sort<N>(b);
        const composite_u16x2 bl = composite_slot<N>(b, lo), bh = composite_slot<N>(b, hi);
        m[2] = ((uint32_t)bl[0] + bh[0] + 1u) >> 1;
        m[3] = ((uint32_t)bl[1] + bh[1] + 1u) >> 1;
      }
    }
    composite_store<T, C>(m, k, fill, at, dst, dval, dcnt);
  }
}

// max and min of the pick exports.  kind, a, b: the index (b = a for a band); smallest: min.  One workgroup per launch
// block, as the median.
template <typename T, int C, int N>
__global__ __launch_bounds__(COMPOSITE_BX* COMPOSITE_BY) void composite_rank_kernel(
    CompositeTable tab, int n, T* __restrict__ dst, uint8_t* __restrict__ dval, uint8_t* __restrict__ dcnt,
    uint8_t* __restrict__ dsrc, int oh, int ow, int fill, int bx, int kind, int a, int b, int smallest) {
  const int64_t blk = blockIdx.x, by = blk / bx;
  const int j = (int)(blk - by * bx) * COMPOSITE_BX + threadIdx.x;
  const int64_t i64 = by * COMPOSITE_BY + threadIdx.y;
  if (i64 >= oh || j >= ow) return;
  const int i = (int)i64;
  const int64_t at = (int64_t)i * ow + j;
  uint32_t ok[N];  // the lane's validity byte in source t, 0 outside its rect
  // the validity bytes of the whole list, all in flight together
#pragma unroll
  for (int t = 0; t < N; ++t) {
    ok[t] = 0u;
    if (t < n) {
      const CompositeSource& e = tab.s[t];
      const int yy = i - e.dy, xx = j - e.dx;
      if ((unsigned)yy < (unsigned)e.h && (unsigned)xx < (unsigned)e.w)
        ok[t] = e.valid ? (uint32_t)e.valid[(int64_t)yy * e.w + xx] : 1u;
    }
  }
  // bands a and b of every source that passed (of one with a nodata value all bands) and the ranking: r = u + 1 (max)
  // or ~u (min) is at least 1 (u <= 131070), 0 stands for no candidate yet, and the strict compare keeps the first of
  // equals
  const uint32_t top = (uint32_t)(T)~(T)0;
  const T* win = nullptr;
  uint32_t best = 0u;
  int k = 0, wid = COMPOSITE_NO_SOURCE;
#pragma unroll
  for (int t = 0; t < N; ++t) {
    if (t < n && ok[t]) {
      const CompositeSource& e = tab.s[t];
      const T* p = (const T*)e.px + ((int64_t)(i - e.dy) * e.w + (j - e.dx)) * C;
      const uint32_t A = (uint32_t)p[a], B = (uint32_t)p[b];
      bool nd = e.nodata >= 0;
      if (nd) {
#pragma unroll
        for (int c = 0; c < C; ++c) nd = nd && (int)p[c] == e.nodata;
      }
      uint32_t u;
      if (!nd && index_value(kind, A, B, top, &u)) {
        ++k;
        const uint32_t r = smallest ? ~u : u + 1u;
        if (r > best) best = r, win = p, wid = e.id;
      }
    }
  }
  uint32_t m[4] = {0u, 0u, 0u, 0u};
  if (win) {
#pragma unroll
    for (int c = 0; c < C; ++c) m[c] = (uint32_t)win[c];
  }
  composite_store<T, C>(m, k, fill, at, dst, dval, dcnt);
  if (dsrc) dsrc[at] = (uint8_t)wid;
}

#undef COMPOSITE_PIXEL_LOOP

// The index of a ranked launch (kind, a, b: b = a for a band; nothing is read of it for the other modes).
struct CompositeIndex {
  int kind, a, b;
};

template <typename T, int C>
static void composite_launch(const CompositeTable& tab, int n, T* dst, uint8_t* dval, uint8_t* dcnt, uint8_t* dsrc, int oh,
                             int ow, int mode, const CompositeIndex& ix, int fill, hipStream_t stream) {
  const int bx = (ow + COMPOSITE_BX - 1) / COMPOSITE_BX;
  const int64_t nblocks = (int64_t)bx * ((oh + COMPOSITE_BY - 1) / COMPOSITE_BY);
  // oh ow < 2^31: fewer than 2^31 workgroups of 4 rows of 64
  const dim3 grid = launch_grid(nblocks), every((unsigned)nblocks), block(COMPOSITE_BX, COMPOSITE_BY);
  const int smallest = mode == COMPOSITE_RANK_MIN;
  if ((mode == COMPOSITE_FIRST || mode == COMPOSITE_LAST) && dsrc)
    hipLaunchKernelGGL((composite_pick_kernel<T, C, true>), grid, block, 0, stream, tab, n, (int)(mode == COMPOSITE_LAST),
                       dst, dval, dcnt, dsrc, oh, ow, fill, bx, nblocks);
  else if (mode == COMPOSITE_FIRST || mode == COMPOSITE_LAST)
    hipLaunchKernelGGL((composite_pick_kernel<T, C, false>), grid, block, 0, stream, tab, n, (int)(mode == COMPOSITE_LAST),
                       dst, dval, dcnt, dsrc, oh, ow, fill, bx, nblocks);
  else if (mode == COMPOSITE_MEAN)
    hipLaunchKernelGGL((composite_mean_kernel<T, C>), grid, block, 0, stream, tab, n, dst, dval, dcnt, oh, ow, fill, bx,
                       nblocks);
  else if (mode == COMPOSITE_MEDIAN && n <= 4)
    hipLaunchKernelGGL((composite_median_kernel<T, C, 4>), every, block, 0, stream, tab, n, dst, dval, dcnt, oh, ow, fill,
                       bx);
  else if (mode == COMPOSITE_MEDIAN && n <= 8)
    hipLaunchKernelGGL((composite_median_kernel<T, C, 8>), every, block, 0, stream, tab, n, dst, dval, dcnt, oh, ow, fill,
                       bx);
  else if (mode == COMPOSITE_MEDIAN)
    hipLaunchKernelGGL((composite_median_kernel<T, C, 16>), every, block, 0, stream, tab, n, dst, dval, dcnt, oh, ow,
                       fill, bx);
  else if (n <= 4)
    hipLaunchKernelGGL((composite_rank_kernel<T, C, 4>), every, block, 0, stream, tab, n, dst, dval, dcnt, dsrc, oh, ow,
                       fill, bx, ix.kind, ix.a, ix.b, smallest);
  else if (n <= 8)
    hipLaunchKernelGGL((composite_rank_kernel<T, C, 8>), every, block, 0, stream, tab, n, dst, dval, dcnt, dsrc, oh, ow,
                       fill, bx, ix.kind, ix.a, ix.b, smallest);
  else
    hipLaunchKernelGGL((composite_rank_kernel<T, C, 16>), every, block, 0, stream, tab, n, dst, dval, dcnt, dsrc, oh, ow,
                       fill, bx, ix.kind, ix.a, ix.b, smallest);
}

// Both families of exports.  pick: dsic_window_composite_pick_u8 / _u16, whose modes are first, last, max and min and
// which take id, dsrc and the index; the other two pass null, null and nothing to read.
template <typename T>
static int composite(const char* what, bool pick, const T* const* src, const uint8_t* const* src_valid, const int* rect,
                     const int* nodata, const int* id, int n, int C, T* dst, uint8_t* dval, uint8_t* dcnt, uint8_t* dsrc,
                     int oh, int ow, int mode, CompositeIndex ix, int fill, void* stream) {
  DSIC_REQUIRE(n >= 1 && n <= COMPOSITE_MAX, "%s: n=%d sources (1..%d)", what, n, COMPOSITE_MAX);
  DSIC_REQUIRE(C >= 1 && C <= 4, "%s: C=%d must be in 1..4", what, C);
  DSIC_REQUIRE(oh >= 1 && ow >= 1 && (int64_t)oh * ow < ((int64_t)1 << 31),
               "%s: output %dx%d must be at least 1x1 and under 2^31 pixels", what, oh, ow);
  DSIC_REQUIRE(src && src_valid && rect && nodata && dst, "%s: null pointer", what);
  if (pick) {
    const bool ranked = mode == COMPOSITE_RANK_MAX || mode == COMPOSITE_RANK_MIN;
    DSIC_REQUIRE(mode == COMPOSITE_FIRST || mode == COMPOSITE_LAST || ranked, "%s: mode=%d (0 first, 1 last, 4 max, 5 min)",
                 what, mode);
    if (ranked) {
      DSIC_REQUIRE(ix.kind >= INDEX_BAND && ix.kind <= INDEX_ND, "%s: kind=%d (0 band, 1 difference, 2 nd)", what, ix.kind);
      const int status = index_bands(what, C, ix.kind, ix.a, ix.b);
      if (status != DSIC_OK) return status;
      if (ix.kind == INDEX_BAND) ix.b = ix.a;
    }
  } else {
    DSIC_REQUIRE(mode >= COMPOSITE_FIRST && mode <= COMPOSITE_MEDIAN, "%s: mode=%d (0 first, 1 last, 2 mean, 3 median)", what,
                 mode);
  }
  DSIC_REQUIRE(pixel_value<T>(fill, 0), "%s: fill=%d must be a pixel value", what, fill);
  const int64_t px = (int64_t)sizeof(T) * C, opix = (int64_t)oh * ow;
  DSIC_REQUIRE(((uintptr_t)dst & (sizeof(T) - 1)) == 0, "%s: dst must be %d-byte aligned", what, (int)sizeof(T));
  const void* outs[4] = {dst, dval, dcnt, dsrc};
  const int64_t obytes[4] = {px * opix, opix, opix, opix};
  for (int a = 0; a < 4; ++a)
    for (int b = a + 1; b < 4; ++b)
      DSIC_REQUIRE(!outs[a] || !outs[b] || buffers_apart(outs[a], obytes[a], outs[b], obytes[b]), "%s: the outputs overlap",
                   what);
  CompositeTable tab = {};
  for (int i = 0; i < n; ++i) {
    const int dy = rect[4 * i], dx = rect[4 * i + 1], h = rect[4 * i + 2], w = rect[4 * i + 3];
    DSIC_REQUIRE(src[i], "%s: source %d: null pointer", what, i);
    DSIC_REQUIRE(h >= 1 && w >= 1, "%s: source %d: rect %dx%d must be at least 1x1", what, i, h, w);
    DSIC_REQUIRE(dy >= 0 && dx >= 0 && (int64_t)dy + h <= oh && (int64_t)dx + w <= ow,
                 "%s: source %d: rect %dx%d at (%d, %d) is not inside the output %dx%d", what, i, h, w, dy, dx, oh, ow);
    DSIC_REQUIRE(pixel_value<T>(nodata[i], -1), "%s: source %d: nodata=%d (-1 for none, or a pixel value)", what, i, nodata[i]);
    DSIC_REQUIRE(!id || (id[i] >= 0 && id[i] < COMPOSITE_NO_SOURCE), "%s: source %d: id=%d must be in 0..%d", what, i,
                 id ? id[i] : 0, COMPOSITE_NO_SOURCE - 1);
    DSIC_REQUIRE(((uintptr_t)src[i] & (sizeof(T) - 1)) == 0, "%s: source %d must be %d-byte aligned", what, i, (int)sizeof(T));
    const int64_t spix = (int64_t)h * w;
    for (int a = 0; a < 4; ++a)
      DSIC_REQUIRE(!outs[a] || (buffers_apart(src[i], px * spix, outs[a], obytes[a]) &&
                                (!src_valid[i] || buffers_apart(src_valid[i], spix, outs[a], obytes[a]))),
                   "%s: source %d and an output overlap", what, i);
    tab.s[i] = {src[i], src_valid[i], dy, dx, h, w, nodata[i], id ? id[i] : i};
  }
  const hipStream_t s = (hipStream_t)stream;
  switch (C) {
    case 1: composite_launch<T, 1>(tab, n, dst, dval, dcnt, dsrc, oh, ow, mode, ix, fill, s); break;
    case 2: composite_launch<T, 2>(tab, n, dst, dval, dcnt, dsrc, oh, ow, mode, ix, fill, s); break;
    case 3: composite_launch<T, 3>(tab, n, dst, dval, dcnt, dsrc, oh, ow, mode, ix, fill, s); break;
    default: composite_launch<T, 4>(tab, n, dst, dval, dcnt, dsrc, oh, ow, mode, ix, fill, s); break;
  }
  return check_launch(what);
}

}  // namespace dsic

using namespace dsic;

extern "C" int dsic_window_composite_u8(const uint8_t* const* src, const uint8_t* const* src_valid, const int* rect,
                                        const int* nodata, int n, int C, uint8_t* dst_hwc, uint8_t* dst_valid,
                                        uint8_t* dst_count, int oh, int ow, int mode, int fill, void* stream) {
  return composite<uint8_t>("window_composite_u8", false, src, src_valid, rect, nodata, nullptr, n, C, dst_hwc, dst_valid,
                            dst_count, nullptr, oh, ow, mode, {0, 0, 0}, fill, stream);
}

extern "C" int dsic_window_composite_u16(const uint16_t* const* src, const uint8_t* const* src_valid, const int* rect,
                                         const int* nodata, int n, int C, uint16_t* dst_hwc, uint8_t* dst_valid,
                                         uint8_t* dst_count, int oh, int ow, int mode, int fill, void* stream) {
  return composite<uint16_t>("window_composite_u16", false, src, src_valid, rect, nodata, nullptr, n, C, dst_hwc, dst_valid,
                             dst_count, nullptr, oh, ow, mode, {0, 0, 0}, fill, stream);
}

extern "C" int dsic_window_composite_pick_u8(const uint8_t* const* src, const uint8_t* const* src_valid, const int* rect,
                                             const int* nodata, const int* id, int n, int C, uint8_t* dst_hwc,
                                             uint8_t* dst_valid, uint8_t* dst_count, uint8_t* dst_source, int oh, int ow,
                                             int mode, int kind, int a, int b, int fill, void* stream) {
  return composite<uint8_t>("window_composite_pick_u8", true, src, src_valid, rect, nodata, id, n, C, dst_hwc, dst_valid,
                            dst_count, dst_source, oh, ow, mode, {kind, a, b}, fill, stream);
}

extern "C" int dsic_window_composite_pick_u16(const uint16_t* const* src, const uint8_t* const* src_valid, const int* rect,
                                              const int* nodata, const int* id, int n, int C, uint16_t* dst_hwc,
                                              uint8_t* dst_valid, uint8_t* dst_count, uint8_t* dst_source, int oh, int ow,
                                              int mode, int kind, int a, int b, int fill, void* stream) {
  return composite<uint16_t>("window_composite_pick_u16", true, src, src_valid, rect, nodata, id, n, C, dst_hwc, dst_valid,
                             dst_count, dst_source, oh, ow, mode, {kind, a, b}, fill, stream);
}
