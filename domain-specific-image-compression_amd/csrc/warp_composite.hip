// Warped scene stacks (codec.SceneStack.read_warped): n scenes, each under its own affine, sampled and combined per
// output pixel in one launch.  include/dsic_hip.h defines the result as the chain of dsic_window_warp_u8 / _u16 per source
// and dsic_window_composite(_pick)_u8 / _u16 over the n sampled images; here the sampled pixel of a source lives in
// registers between the two steps and never reaches memory.
//
// The sampler is warp_sample.h's warp_pixel, the one warp.hip launches, so step 1 is the same arithmetic; a source's
// sampled pixel is a candidate iff warp_pixel calls it valid and, for a source with a nodata value, its channels do not
// all equal it (step 2's rule on the sampled image; for the ranked modes the index must be defined as well).
//
// Work split: warp.hip's.  A workgroup is 16 x 16 output pixels, a wave owns an 8 x 8 patch, so under any one source
// the wave's taps lie within a dozen cache lines; blocks are walked by a grid-stride loop in int64.  The source table
// (16 entries of two pointers, a Warp, a nodata value and an id: 128 bytes each, 2 KB) travels by value in the kernel
// arguments and the loop over the sources reads the entry it is at with scalar loads.  Whether a source has a validity
// window is a wave-uniform branch per source.  A source is skipped when no lane of the wave that still wants it lies
// inside it (one ballot over the inside test on Py, Px), and first / last without a count plane leave the loop once
// every lane of the wave has its winner.  For last the host lays the table out back to front.
//   first, last: the first candidate met, its pixel and id in registers.
//   mean: per-band uint32 sums and k; (2 S + k) / (2 k).
//   max, min: r = u + 1 or ~u compared strictly, the winner's pixel and id in registers.
//   median: instantiated for lists of up to 4, 8 and 16 sources.  The candidates' values are kept as a sorted list in
//     N registers per band pair (16-bit fields, two bands to a word, unused slots all ones): a new value is inserted by
//     a fully unrolled chain of packed minima and maxima over the slots, and the two middle slots are picked by compares
//     against constants, as composite.hip does: no array is indexed by a variable, nothing goes to scratch.
#include <stdio.h>

#include "common.h"
#include "render.h"
#include "warp_sample.h"

namespace dsic {

constexpr int WARP_COMPOSITE_MAX = 16;
// DSIC_COMPOSITE_* of include/dsic_hip.h
constexpr int WC_FIRST = 0, WC_LAST = 1, WC_MEAN = 2, WC_MEDIAN = 3, WC_RANK_MAX = 4, WC_RANK_MIN = 5;
constexpr int WC_NO_SOURCE = 255;                        // the source plane where k = 0
constexpr int WC_PICK = 0, WC_SUM = 1, WC_SORT = 2, WC_RANK = 3;  // the kernel's per-pixel state

struct WarpCompositeSource {
  const void* px;        // [sh][sw][C]
  const uint8_t* valid;  // null, or [sh][sw]
  Warp g;
  int nodata, id;
};
static_assert(sizeof(WarpCompositeSource) == 128, "the source table is 2 KB of kernel arguments");

struct WarpCompositeTable {
  WarpCompositeSource s[WARP_COMPOSITE_MAX];
};

struct WarpCompositeOptions {
  int oh, ow, C, sample, fill;
  int kind, a, b, smallest;  // max / min: the index (b = a for a band) and which end wins
};

typedef unsigned short warp_composite_u16x2 __attribute__((ext_vector_type(2)));

// whether output pixel (i, j) samples a position inside the scene: warp_pixel's own test
__device__ __forceinline__ bool warp_composite_inside(const Warp& g, int i, int j) {
  const int64_t Py = g.m[0] * (2 * i + 1) + g.m[1] * (2 * j + 1) + 2 * g.m[2];
  const int64_t Px = g.m[3] * (2 * i + 1) + g.m[4] * (2 * j + 1) + 2 * g.m[5];
  return Py >= 0 && Py < g.HP && Px >= 0 && Px < g.WP;
}

// the sampled pixel of source e at output pixel (i, j) into v, and whether it is a candidate
template <typename T>
__device__ __forceinline__ bool warp_composite_sample(const WarpCompositeSource& e, int C, int sample, int i, int j,
                                                      uint32_t v[4]) {
  bool ok;
  if (e.valid)  // the same in every lane
    ok = warp_pixel<T, true>((const T*)e.px, e.valid, e.g, C, sample, -1, 0u, i, j, v);
  else
    ok = warp_pixel<T, false>((const T*)e.px, nullptr, e.g, C, sample, e.nodata, 0u, i, j, v);
  if (ok && e.nodata >= 0) {
    bool nd = true;
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < C) nd = nd && v[c] == (uint32_t)e.nodata;
    ok = !nd;
  }
  return ok;
}

// x into the ascending list v, both 16-bit halves on their own; the largest value falls off the end (all ones, while
// fewer than N values are in)
template <int N>
__device__ __forceinline__ void warp_composite_insert(warp_composite_u16x2 (&v)[N], warp_composite_u16x2 x) {
#pragma unroll
  for (int s = 0; s < N; ++s) {
    const warp_composite_u16x2 lo = __builtin_elementwise_min(v[s], x);
    x = __builtin_elementwise_max(v[s], x);
    v[s] = lo;
  }
}

// slot `at` of the list, `at` a lane's own number: every slot is read by its constant number and the one wanted is kept
template <int N>
__device__ __forceinline__ warp_composite_u16x2 warp_composite_slot(const warp_composite_u16x2 (&v)[N], int at) {
  uint32_t r = 0u;
#pragma unroll
  for (int s = 0; s < N; ++s) r |= at == s ? __builtin_bit_cast(uint32_t, v[s]) : 0u;
  return __builtin_bit_cast(warp_composite_u16x2, r);
}

// R: the state a pixel keeps over the list (WC_PICK first and last, WC_SUM mean, WC_SORT median, WC_RANK max and min);
// N: the slots of the median's list, 1 otherwise
template <typename T, int R, int N>
__global__ __launch_bounds__(WARP_TILE * WARP_TILE) void warp_composite_kernel(WarpCompositeTable tab, int n,
                                                                               T* __restrict__ dst,
                                                                               uint8_t* __restrict__ dval,
                                                                               uint8_t* __restrict__ dcnt,
                                                                               uint8_t* __restrict__ dsrc,
                                                                               WarpCompositeOptions o, int bx,
                                                                               int64_t nblocks) {
  const int C = o.C;
  const uint32_t top = (uint32_t)(T)~(T)0;
  for (int64_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
    int i, j;
    const bool live = warp_where(o.oh, o.ow, blk, bx, &i, &j);
    uint32_t m[4] = {0u, 0u, 0u, 0u};  // pick, rank: the winner's pixel; sum: the sums
    uint32_t best = 0u;                // rank: 0 stands for no candidate yet, r >= 1
    int k = 0, wid = WC_NO_SOURCE;
    warp_composite_u16x2 lo01[N], lo23[N];  // sort: bands 0 and 1, bands 2 and 3
#pragma unroll
    for (int s = 0; s < N; ++s) lo01[s] = lo23[s] = warp_composite_u16x2{0xFFFF, 0xFFFF};
    for (int t = 0; t < n; ++t) {
      const bool open = live && (R != WC_PICK || dcnt || !k);  // whether this lane still looks at sources
      if (R == WC_PICK && !__builtin_amdgcn_ballot_w64(open)) break;  // every lane of the wave has its winner
      const WarpCompositeSource& e = tab.s[t];
      const bool under = open && warp_composite_inside(e.g, i, j);
      if (!__builtin_amdgcn_ballot_w64(under)) continue;  // no lane of the wave lies inside this source
      uint32_t v[4];
      if (!under || !warp_composite_sample<T>(e, C, o.sample, i, j, v)) {
        // not a candidate of this lane
      } else if constexpr (R == WC_PICK) {
        if (!k) {
#pragma unroll
          for (int c = 0; c < 4; ++c) m[c] = v[c];
          wid = e.id;
        }
        ++k;
      } else if constexpr (R == WC_SUM) {
#pragma unroll
        for (int c = 0; c < 4; ++c) m[c] += v[c];
        ++k;
      } else if constexpr (R == WC_SORT) {
        warp_composite_insert<N>(lo01, warp_composite_u16x2{(unsigned short)v[0], (unsigned short)v[1]});
        if (C > 2) warp_composite_insert<N>(lo23, warp_composite_u16x2{(unsigned short)v[2], (unsigned short)v[3]});
        ++k;
      } else {
        // bands a and b by two shifts of the pixel as 16-bit fields: a chain of selects holds six masks in scalar registers
        const uint64_t px = (uint64_t)(v[0] | v[1] << 16) | (uint64_t)(v[2] | v[3] << 16) << 32;
        const uint32_t A = (uint32_t)(px >> (16 * o.a)) & 0xFFFFu, B = (uint32_t)(px >> (16 * o.b)) & 0xFFFFu;
        uint32_t u;
        if (index_value(o.kind, A, B, top, &u)) {
          ++k;
          const uint32_t r = o.smallest ? ~u : u + 1u;  // u <= 131070; the strict compare keeps the first of equals
          if (r > best) {
            best = r, wid = e.id;
#pragma unroll
            for (int c = 0; c < 4; ++c) m[c] = v[c];
          }
        }
      }
    }
    if (!live) continue;
    if (k) {
      if constexpr (R == WC_SUM) {
#pragma unroll
        for (int c = 0; c < 4; ++c) m[c] = (2u * m[c] + (uint32_t)k) / (2u * (uint32_t)k);  // 2 * 16 * 65535 + 16 < 2^32
      } else if constexpr (R == WC_SORT) {
        const int lo = (k - 1) >> 1, hi = k >> 1;  // equal for odd k: (v + v + 1) >> 1 = v
        const warp_composite_u16x2 al = warp_composite_slot<N>(lo01, lo), ah = warp_composite_slot<N>(lo01, hi);
        m[0] = ((uint32_t)al[0] + ah[0] + 1u) >> 1;
        m[1] = ((uint32_t)al[1] + ah[1] + 1u) >> 1;
        if (C > 2) {
          const warp_composite_u16x2 bl = warp_composite_slot<N>(lo23, lo), bh = warp_composite_slot<N>(lo23, hi);
          m[2] = ((uint32_t)bl[0] + bh[0] + 1u) >> 1;
          m[3] = ((uint32_t)bl[1] + bh[1] + 1u) >> 1;
        }
      }
    }
    const int64_t at = (int64_t)i * o.ow + j;
    T* out = dst + at * C;
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < C) out[c] = (T)(k ? m[c] : (uint32_t)o.fill);
    if (dval) dval[at] = (uint8_t)(k > 0);
    if (dcnt) dcnt[at] = (uint8_t)k;
    if (dsrc) dsrc[at] = (uint8_t)wid;
  }
}

template <typename T, int R, int N>
static void warp_composite_launch(const WarpCompositeTable& tab, int n, T* dst, uint8_t* dval, uint8_t* dcnt, uint8_t* dsrc,
                                  const WarpCompositeOptions& o, hipStream_t stream) {
  const int bx = (o.ow + WARP_TILE - 1) / WARP_TILE;
  const int64_t nblocks = (int64_t)bx * ((o.oh + WARP_TILE - 1) / WARP_TILE);
  hipLaunchKernelGGL((warp_composite_kernel<T, R, N>), launch_grid(nblocks), dim3(WARP_TILE * WARP_TILE), 0, stream, tab, n,
                     dst, dval, dcnt, dsrc, o, bx, nblocks);
}

// The checks, all before the launch, in the words of warp_check and of composite.hip's check where one applies.
template <typename T>
static int warp_composite(const char* what, const dsic_warp_source* src, int n, int C, int cmin, T* dst, uint8_t* dval,
                          uint8_t* dcnt, uint8_t* dsrc, int oh, int ow, int sample, int reduce, int kind, int a, int b,
                          int fill, void* stream) {
  DSIC_REQUIRE(n >= 1 && n <= WARP_COMPOSITE_MAX, "%s: n=%d sources (1..%d)", what, n, WARP_COMPOSITE_MAX);
  DSIC_REQUIRE(src && dst, "%s: null pointer", what);
  DSIC_REQUIRE(C >= cmin && C <= 4, "%s: C=%d must be in %d..4", what, C, cmin);
  DSIC_REQUIRE(sample >= 0 && sample <= 2, "%s: mode=%d (0 bilinear, 1 nearest, 2 cubic)", what, sample);
  DSIC_REQUIRE(oh >= 1 && ow >= 1 && oh <= WARP_SIDE && ow <= WARP_SIDE, "%s: output %dx%d must be 1x1 .. 2^20x2^20", what, oh,
               ow);
  DSIC_REQUIRE((int64_t)oh * ow < ((int64_t)1 << 31), "%s: output %dx%d must be at least 1x1 and under 2^31 pixels", what, oh,
               ow);
  DSIC_REQUIRE(reduce >= WC_FIRST && reduce <= WC_RANK_MIN,
               "%s: reduce mode=%d (0 first, 1 last, 2 mean, 3 median, 4 max, 5 min)", what, reduce);
  const bool ranked = reduce == WC_RANK_MAX || reduce == WC_RANK_MIN;
  if (ranked) {
    DSIC_REQUIRE(kind >= INDEX_BAND && kind <= INDEX_ND, "%s: kind=%d (0 band, 1 difference, 2 nd)", what, kind);
    const int status = index_bands(what, C, kind, a, b);
    if (status != DSIC_OK) return status;
    if (kind == INDEX_BAND) b = a;
  } else {
    kind = a = b = 0;
  }
  DSIC_REQUIRE(!dsrc || (reduce != WC_MEAN && reduce != WC_MEDIAN),
               "%s: dst_source goes with first, last, max and min; reduce mode=%d mixes sources", what, reduce);
  DSIC_REQUIRE(pixel_value<T>(fill, 0), "%s: fill=%d must be a pixel value", what, fill);
  const int64_t px = (int64_t)sizeof(T) * C, opix = (int64_t)oh * ow;
  DSIC_REQUIRE(((uintptr_t)dst & (sizeof(T) - 1)) == 0, "%s: dst must be %d-byte aligned", what, (int)sizeof(T));
  const void* outs[4] = {dst, dval, dcnt, dsrc};
  const int64_t obytes[4] = {px * opix, opix, opix, opix};
  for (int p = 0; p < 4; ++p)
    for (int q = p + 1; q < 4; ++q)
      DSIC_REQUIRE(!outs[p] || !outs[q] || buffers_apart(outs[p], obytes[p], outs[q], obytes[q]), "%s: the outputs overlap",
                   what);
  WarpCompositeTable tab = {};
  for (int i = 0; i < n; ++i) {
    const dsic_warp_source& s = src[i];
    char who[96];
    snprintf(who, sizeof who, "%s: source %d", what, i);
    DSIC_REQUIRE(s.src, "%s: null pointer", who);
    const Warp g = warp_of(s.sh, s.sw, s.sy0, s.sx0, s.shift, s.LH, s.LW, s.H, s.W, s.m, oh, ow);
    const int status = warp_geometry(who, g, s.H, s.W, s.m, sample);
    if (status != DSIC_OK) return status;
    DSIC_REQUIRE(pixel_value<T>(s.nodata, -1), "%s: nodata=%d (-1 for none, or a pixel value)", who, s.nodata);
    DSIC_REQUIRE(s.id >= 0 && s.id < WC_NO_SOURCE, "%s: id=%d must be in 0..%d", who, s.id, WC_NO_SOURCE - 1);
    DSIC_REQUIRE(((uintptr_t)s.src & (sizeof(T) - 1)) == 0, "%s must be %d-byte aligned", who, (int)sizeof(T));
    const int64_t spix = (int64_t)s.sh * s.sw;
    for (int p = 0; p < 4; ++p)
      DSIC_REQUIRE(!outs[p] || (buffers_apart(s.src, px * spix, outs[p], obytes[p]) &&
                                (!s.src_valid || buffers_apart(s.src_valid, spix, outs[p], obytes[p]))),
                   "%s and an output overlap", who);
    tab.s[reduce == WC_LAST ? n - 1 - i : i] = {s.src, s.src_valid, g, s.nodata, s.id};  // last: the list from its back
  }
  const WarpCompositeOptions o = {oh, ow, C, sample, fill, kind, a, b, (int)(reduce == WC_RANK_MIN)};
  const hipStream_t q = (hipStream_t)stream;
  if (reduce == WC_FIRST || reduce == WC_LAST)
    warp_composite_launch<T, WC_PICK, 1>(tab, n, dst, dval, dcnt, dsrc, o, q);
  else if (reduce == WC_MEAN)
    warp_composite_launch<T, WC_SUM, 1>(tab, n, dst, dval, dcnt, dsrc, o, q);
  else if (ranked)
    warp_composite_launch<T, WC_RANK, 1>(tab, n, dst, dval, dcnt, dsrc, o, q);
  else if (n <= 4)
    warp_composite_launch<T, WC_SORT, 4>(tab, n, dst, dval, dcnt, dsrc, o, q);
  else if (n <= 8)
    warp_composite_launch<T, WC_SORT, 8>(tab, n, dst, dval, dcnt, dsrc, o, q);
  else
    warp_composite_launch<T, WC_SORT, 16>(tab, n, dst, dval, dcnt, dsrc, o, q);
  return check_launch(what);
}

}  // namespace dsic

using namespace dsic;

extern "C" int dsic_window_warp_composite_u8(const dsic_warp_source* sources, int n, int C, uint8_t* dst_hwc,
                                             uint8_t* dst_valid, uint8_t* dst_count, uint8_t* dst_source, int oh, int ow,
                                             int sample_mode, int reduce_mode, int kind, int a, int b, int fill,
                                             void* stream) {
  return warp_composite<uint8_t>("window_warp_composite_u8", sources, n, C, 3, dst_hwc, dst_valid, dst_count, dst_source, oh,
                                 ow, sample_mode, reduce_mode, kind, a, b, fill, stream);
}

extern "C" int dsic_window_warp_composite_u16(const dsic_warp_source* sources, int n, int C, uint16_t* dst_hwc,
                                              uint8_t* dst_valid, uint8_t* dst_count, uint8_t* dst_source, int oh, int ow,
                                              int sample_mode, int reduce_mode, int kind, int a, int b, int fill,
                                              void* stream) {
  return warp_composite<uint16_t>("window_warp_composite_u16", sources, n, C, 1, dst_hwc, dst_valid, dst_count, dst_source,
                                  oh, ow, sample_mode, reduce_mode, kind, a, b, fill, stream);
}
