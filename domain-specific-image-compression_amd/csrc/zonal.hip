// Zonal statistics (codec.ImageReader.zonal_stats, codec.SceneStack.zonal_stats): per zone z of a uint16 zone raster and
// per value k of a pixel, stats[z][k] accumulates the count, the sum, the sum of squares, the minimum and the maximum of
// the counted pixels' values; include/dsic_hip.h states the rule.  Integer sums, minima and maxima: no order shows.
//
// A lane takes one pixel of 64 consecutive ones per step, as in histogram.hip, so a wave's loads are one run.  A lane's key
// is its pixel's zone id (a lane past the image holds a key no zone has).  Equal keys on neighbouring lanes are one run,
// found with one ballot; a pixel that is not counted (invalid, nodata, an undefined index) stays in its run and brings
// the neutral element, so validity does not cut runs.  Count, sum, sum of squares, minimum and maximum are reduced within
// each run by a segmented wave reduction of log2(64) shuffle steps: lane i takes lane i + d's partial result iff d is at
// most the number of lanes that continue i's run.  The lane at the head of a run carries (zone, accumulators) on to the
// next step, adds to them while the zone stays, and spills them when it changes.  A scene that is one zone costs 5 K
// atomics per wave for the whole loop; blocks of 64 x 64 pixels cost them once per 64 steps of a wave's lane.
// A key at or above Z belongs to no zone: its run's head does nothing, so such an id never produces a write.
//
// Spills go to a table in LDS when Z * K * 40 bytes fit ZONAL_LDS_BYTES = 40960 (DSIC_ZONAL_LDS_BYTES of the header:
// Z * K <= 1024, 256 zones of four bands, 1024 zones of an index): 40 KB of the CU's 160 KB, so four workgroups of 256
// threads, 16 waves, per CU, which the kernel's registers allow as well (DESIGN.md section 3 has the figures).  The
// workgroup then flushes the zones it touched (count != 0) with one global 64-bit atomic per word.  A larger table takes
// the spills directly, with global 64-bit atomics (add, signed min, signed max).
// The optional per-zone histogram counts stretch_byte(u) into hist[z][k][256] in global memory with 32-bit atomic adds,
// run-carried on (zone, k, bin) exactly as histogram.hip carries (value, count); it is compiled into kernels of its own.
#include "common.h"
#include "render.h"

namespace dsic {

constexpr int ZONAL_THREADS = 256, ZONAL_MAX_BLOCKS = 2048;
constexpr int ZONAL_BANDS = -1;                 // DSIC_ZONAL_BANDS
constexpr int ZONAL_LDS_BYTES = 40960;          // DSIC_ZONAL_LDS_BYTES
constexpr int ZONAL_WORDS = 5;                  // count, sum, sum of squares, min, max
constexpr uint32_t ZONAL_NO_KEY = 0xFFFFFFFFu;  // past the image, and "nothing carried"

struct ZonalPairs {
  uint32_t lo[4], hi[4];  // the histogram's stretch pair per value, in u units
};

// one zone's K records of five words into a table in LDS (workgroup scope) or in global memory (device scope)
template <bool LDS>
__device__ __forceinline__ void zonal_spill(uint64_t* rec, uint64_t cnt, int64_t sum, uint64_t sq, int64_t lo, int64_t hi) {
  constexpr int scope = LDS ? __HIP_MEMORY_SCOPE_WORKGROUP : __HIP_MEMORY_SCOPE_AGENT;
  __hip_atomic_fetch_add(rec + 0, cnt, __ATOMIC_RELAXED, scope);
  __hip_atomic_fetch_add(rec + 1, (uint64_t)sum, __ATOMIC_RELAXED, scope);  // two's complement: the signed sum's bits
  __hip_atomic_fetch_add(rec + 2, sq, __ATOMIC_RELAXED, scope);
  __hip_atomic_fetch_min((int64_t*)rec + 3, lo, __ATOMIC_RELAXED, scope);
  __hip_atomic_fetch_max((int64_t*)rec + 4, hi, __ATOMIC_RELAXED, scope);
}

// KM: 1 or 4, the most values a pixel has in this instantiation (K <= KM)
template <typename T, int KM, bool LDS, bool HIST>
__global__ __launch_bounds__(ZONAL_THREADS) void zonal_kernel(const T* __restrict__ img, const uint8_t* __restrict__ valid,
                                                              const uint16_t* __restrict__ zones, uint64_t n, int C,
                                                              int nodata, int what, int a, int b, int vmin, uint32_t Z, int K,
                                                              uint64_t* __restrict__ stats, ZonalPairs pairs,
                                                              uint32_t* __restrict__ hist) {
  __shared__ uint64_t lt[LDS ? ZONAL_LDS_BYTES / 8 : 1];
  const int records = (int)Z * K;
  if (LDS) {
    for (int i = threadIdx.x; i < records; i += ZONAL_THREADS) {
      uint64_t* rec = lt + i * ZONAL_WORDS;
      rec[0] = rec[1] = rec[2] = 0;
      rec[3] = (uint64_t)INT64_MAX;
      rec[4] = (uint64_t)INT64_MIN;
    }
    __syncthreads();
  }
  uint64_t* table = LDS ? lt : stats;
  const int lane = threadIdx.x & 63;
  const uint32_t top = (uint32_t)(T)~(T)0;
  // the run a head lane carries
  uint32_t held = ZONAL_NO_KEY, hcnt = 0;
  int64_t hsum[KM];
  uint64_t hsq[KM];
  int32_t hmin[KM], hmax[KM];
  uint32_t bkey[KM], bcnt[KM];  // the histogram's own runs: (zone * K + k) * 256 + bin, and its count
#pragma unroll
  for (int k = 0; k < KM; ++k) hsum[k] = 0, hsq[k] = 0, hmin[k] = INT32_MAX, hmax[k] = INT32_MIN, bkey[k] = 0, bcnt[k] = 0;

  // every lane of a wave takes every step (base is the same for all of them): the shuffles and ballots see all 64, and
  // nothing leaves the loop body before the last of them
  for (uint64_t base = (uint64_t)blockIdx.x * ZONAL_THREADS; base < n; base += (uint64_t)gridDim.x * ZONAL_THREADS) {
    const uint64_t p = base + threadIdx.x;
    uint32_t key = ZONAL_NO_KEY, u[KM];
    bool counted = false;
#pragma unroll
    for (int k = 0; k < KM; ++k) u[k] = 0;
    if (p < n) {
      key = zones[p];
      const T* px = img + p * C;
      uint32_t m[4] = {0, 0, 0, 0};
      bool nd = nodata >= 0;
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (c < C) {
          m[c] = (uint32_t)px[c];
          nd = nd && m[c] == (uint32_t)nodata;
        }
      counted = key < Z && !nd && (!valid || valid[p] != 0);
      if (what == ZONAL_BANDS) {
#pragma unroll
        for (int k = 0; k < KM; ++k) u[k] = m[k];
      } else {
        const uint32_t A = a == 0 ? m[0] : a == 1 ? m[1] : a == 2 ? m[2] : m[3];
        const uint32_t B = b == 0 ? m[0] : b == 1 ? m[1] : b == 2 ? m[2] : m[3];
        counted = index_value(what, A, B, top, &u[0]) && counted;
      }
    }
    // the runs of equal keys, and how many lanes after this one continue its run
    const uint32_t left = (uint32_t)__shfl_up((int)key, 1, 64);
    const uint64_t on = __ballot(lane > 0 && left == key);
    const uint64_t after = lane == 63 ? 0 : on >> (lane + 1);
    const int rem = __builtin_ctzll(~after);  // bit 63 of after is 0: ~after is never 0
    // the segmented reduction: the neutral element where the pixel is not counted
    uint32_t cnt = counted ? 1u : 0u;
    int32_t sum[KM], lo[KM], hi[KM];  // 64 values of at most 17 bits: the sum of a step fits 32 bits
    uint64_t sq[KM];
#pragma unroll
    for (int k = 0; k < KM; ++k) {
      const int32_t v = (int32_t)u[k] + vmin;
      sum[k] = counted ? v : 0;
      sq[k] = counted ? (uint64_t)((int64_t)v * v) : 0;
      lo[k] = counted ? v : INT32_MAX;
      hi[k] = counted ? v : INT32_MIN;
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const bool take = d <= rem;
      const uint32_t c2 = (uint32_t)__shfl_down((int)cnt, d, 64);
      cnt += take ? c2 : 0u;
#pragma unroll
      for (int k = 0; k < KM; ++k) {
        if (k >= K) continue;  // K is the same for every lane
        const int32_t s2 = __shfl_down(sum[k], d, 64), l2 = __shfl_down(lo[k], d, 64), h2 = __shfl_down(hi[k], d, 64);
        const uint64_t q2 = (uint64_t)__shfl_down((unsigned long long)sq[k], d, 64);
        if (take) sum[k] += s2, sq[k] += q2, lo[k] = min(lo[k], l2), hi[k] = max(hi[k], h2);
      }
    }
    // the histogram's runs, with every lane in its shuffles and ballots too
    uint64_t bon[KM];
    uint32_t bin[KM];
    if (HIST) {
      const bool before = __shfl_up((int)counted, 1, 64) != 0 && lane > 0;
#pragma unroll
      for (int k = 0; k < KM; ++k) {
        bin[k] = (key * (uint32_t)K + k) * 256u + stretch_byte(u[k], pairs.lo[k], pairs.hi[k]);
        const uint32_t bleft = (uint32_t)__shfl_up((int)bin[k], 1, 64);
        bon[k] = __ballot(counted && before && bleft == bin[k]);
      }
    }
    // from here on the lanes part ways
    if (!((on >> lane) & 1) && key < Z) {  // the head of a run of a zone
      if (held != key) {
        if (hcnt) {
#pragma unroll
          for (int k = 0; k < KM; ++k)
            if (k < K)
              zonal_spill<LDS>(table + ((uint64_t)held * K + k) * ZONAL_WORDS, hcnt, hsum[k], hsq[k], hmin[k], hmax[k]);
        }
        hcnt = 0;
#pragma unroll
        for (int k = 0; k < KM; ++k) hsum[k] = 0, hsq[k] = 0, hmin[k] = INT32_MAX, hmax[k] = INT32_MIN;
        held = key;
      }
      hcnt += cnt;
#pragma unroll
      for (int k = 0; k < KM; ++k) hsum[k] += sum[k], hsq[k] += sq[k], hmin[k] = min(hmin[k], lo[k]), hmax[k] = max(hmax[k], hi[k]);
    }
    if (HIST) {
#pragma unroll
      for (int k = 0; k < KM; ++k) {
        if (k >= K || !counted || ((bon[k] >> lane) & 1)) continue;
        const uint64_t bafter = lane == 63 ? 0 : bon[k] >> (lane + 1);
        const uint32_t run = 1u + (uint32_t)__builtin_ctzll(~bafter);
        if (bcnt[k] && bkey[k] != bin[k]) {
          atomicAdd(hist + bkey[k], bcnt[k]);
          bcnt[k] = 0;
        }
        bkey[k] = bin[k];
        bcnt[k] += run;
      }
    }
  }
  if (hcnt) {
#pragma unroll
    for (int k = 0; k < KM; ++k)
      if (k < K) zonal_spill<LDS>(table + ((uint64_t)held * K + k) * ZONAL_WORDS, hcnt, hsum[k], hsq[k], hmin[k], hmax[k]);
  }
  if (HIST) {
#pragma unroll
    for (int k = 0; k < KM; ++k)
      if (k < K && bcnt[k]) atomicAdd(hist + bkey[k], bcnt[k]);
  }
  if (LDS) {
    __syncthreads();
    for (int i = threadIdx.x; i < records; i += ZONAL_THREADS) {
      const uint64_t* rec = lt + i * ZONAL_WORDS;
      if (rec[0]) zonal_spill<false>(stats + (uint64_t)i * ZONAL_WORDS, rec[0], (int64_t)rec[1], rec[2], (int64_t)rec[3], (int64_t)rec[4]);
    }
  }
}

template <typename T, int KM, bool LDS>
static void zonal_launch(bool with_hist, dim3 grid, hipStream_t stream, const T* img, const uint8_t* valid,
                         const uint16_t* zones, uint64_t n, int C, int nodata, int what, int a, int b, int vmin, uint32_t Z, int K,
                         uint64_t* stats, const ZonalPairs& pairs, uint32_t* hist) {
  if (with_hist)
    hipLaunchKernelGGL((zonal_kernel<T, KM, LDS, true>), grid, dim3(ZONAL_THREADS), 0, stream, img, valid, zones, n, C, nodata,
                       what, a, b, vmin, Z, K, stats, pairs, hist);
  else
    hipLaunchKernelGGL((zonal_kernel<T, KM, LDS, false>), grid, dim3(ZONAL_THREADS), 0, stream, img, valid, zones, n, C, nodata,
                       what, a, b, vmin, Z, K, stats, pairs, hist);
}

template <typename T>
static int zonal_stats(const char* name, const T* img, const uint8_t* valid, const uint16_t* zones, int H, int W, int C,
                       int nodata, int what, int a, int b, int Z, uint64_t* stats, const uint32_t* lohi, uint32_t* hist,
                       void* stream) {
  constexpr int top = (int)(T)~(T)0;
  DSIC_REQUIRE(img && zones && stats, "%s: null pointer", name);
  DSIC_REQUIRE(C >= 1 && C <= 4, "%s: C=%d must be in 1..4", name, C);
  DSIC_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W < ((int64_t)1 << 32), "%s: image %dx%d (at least 1x1, under 2^32 pixels)",
               name, H, W);
  DSIC_REQUIRE(Z >= 1 && Z <= 65535, "%s: Z=%d zones (1..65535)", name, Z);
  DSIC_REQUIRE(what >= ZONAL_BANDS && what <= INDEX_ND, "%s: what=%d (-1 every band, 0 band, 1 difference, 2 nd)", name, what);
  if (what != ZONAL_BANDS) {
    const int status = index_bands(name, C, what, a, b);
    if (status != DSIC_OK) return status;
    if (what == INDEX_BAND) b = a;
  }
  DSIC_REQUIRE(pixel_value<T>(nodata, -1), "%s: nodata=%d (-1 for none, or a pixel value)", name, nodata);
  DSIC_REQUIRE(((uintptr_t)img & (sizeof(T) - 1)) == 0 && ((uintptr_t)zones & 1) == 0 && ((uintptr_t)stats & 7) == 0 &&
                   ((uintptr_t)hist & 3) == 0 && ((uintptr_t)lohi & 3) == 0,
               "%s: img must be %d-byte, zones 2-byte, stats 8-byte, hist and lohi 4-byte aligned", name, (int)sizeof(T));
  DSIC_REQUIRE((hist != nullptr) == (lohi != nullptr), "%s: lohi goes with hist, and hist with lohi", name);
  const int K = what == ZONAL_BANDS ? C : 1;
  int vmin = 0, vmax = top;
  if (what != ZONAL_BANDS) index_range(what, top, &vmin, &vmax);
  ZonalPairs pairs = {{0, 0, 0, 0}, {0, 0, 0, 0}};
  if (hist)
    for (int k = 0; k < K; ++k) {
      DSIC_REQUIRE(lohi[2 * k] <= lohi[2 * k + 1] && lohi[2 * k + 1] <= (uint32_t)(vmax - vmin),
                   "%s: histogram pair (%u, %u) of value %d must have 0 <= lo <= hi <= %d", name, lohi[2 * k], lohi[2 * k + 1], k,
                   vmax - vmin);
      pairs.lo[k] = lohi[2 * k], pairs.hi[k] = lohi[2 * k + 1];
    }
  const int64_t n = (int64_t)H * W, ib = n * C * (int64_t)sizeof(T), zb = 2 * n, sb = (int64_t)Z * K * ZONAL_WORDS * 8,
                hb = (int64_t)Z * K * 1024;
  const auto apart = [&](const void* out, int64_t ob) {
    return buffers_apart(out, ob, img, ib) && buffers_apart(out, ob, zones, zb) && (!valid || buffers_apart(out, ob, valid, n));
  };
  DSIC_REQUIRE(apart(stats, sb), "%s: stats overlaps the image, its validity or the zones", name);
  DSIC_REQUIRE(!hist || apart(hist, hb), "%s: hist overlaps the image, its validity or the zones", name);
  DSIC_REQUIRE(!hist || buffers_apart(hist, hb, stats, sb), "%s: hist overlaps stats", name);
  const int64_t blocks = (n + ZONAL_THREADS - 1) / ZONAL_THREADS;
  const dim3 grid((unsigned)(blocks > ZONAL_MAX_BLOCKS ? ZONAL_MAX_BLOCKS : blocks));
  const bool lds = sb <= ZONAL_LDS_BYTES;
#define ZONAL_GO(KM, LDS) \
  zonal_launch<T, KM, LDS>(hist != nullptr, grid, (hipStream_t)stream, img, valid, zones, (uint64_t)n, C, nodata, what, a, b, vmin, \
                           (uint32_t)Z, K, stats, pairs, hist)
  if (K == 1) {
    if (lds) ZONAL_GO(1, true); else ZONAL_GO(1, false);
  } else {
    if (lds) ZONAL_GO(4, true); else ZONAL_GO(4, false);
  }
#undef ZONAL_GO
  return check_launch(name);
}

}  // namespace dsic

using namespace dsic;

extern "C" int dsic_zonal_stats_u8(const uint8_t* img_hwc, const uint8_t* valid_hw, const uint16_t* zones_hw, int H, int W, int C,
                                   int nodata, int what, int band_a, int band_b, int Z, uint64_t* stats, const uint32_t* lohi,
                                   uint32_t* hist, void* stream) {
  return zonal_stats<uint8_t>("zonal_stats_u8", img_hwc, valid_hw, zones_hw, H, W, C, nodata, what, band_a, band_b, Z, stats, lohi,
                              hist, stream);
}

extern "C" int dsic_zonal_stats_u16(const uint16_t* img_hwc, const uint8_t* valid_hw, const uint16_t* zones_hw, int H, int W, int C,
                                    int nodata, int what, int band_a, int band_b, int Z, uint64_t* stats, const uint32_t* lohi,
                                    uint32_t* hist, void* stream) {
  return zonal_stats<uint16_t>("zonal_stats_u16", img_hwc, valid_hw, zones_hw, H, W, C, nodata, what, band_a, band_b, Z, stats, lohi,
                               hist, stream);
}
