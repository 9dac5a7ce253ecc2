// Band histograms of an image (codec.ImageReader.histogram; the percentile stretch of a rendered view is read off them):
// hist[c][v] += the pixels of img [H][W][C] whose channel c equals v, a validity plane leaving out its zeros and a
// nodata value the pixels whose C channels all equal it.  Integer sums: no order shows.
//
// A lane takes one pixel of 64 consecutive ones per step, so a wave's loads are one run.  Per channel, equal values on
// neighbouring lanes are one run: the lane at its head learns the run's length from one ballot and carries (value,
// count) on to the next step, adding to it while the value stays and spilling it into the histogram when it changes.
// Smooth imagery makes few, long runs, and a constant image makes one add per wave and channel instead of one per
// pixel on a single address.
// uint8: the bins are C x 256 counters in LDS per workgroup, flushed with one global atomic per non-empty bin.
// uint16: C x 65536 counters do not fit LDS; the runs go to the global histogram directly.
#include "common.h"
#include "render.h"

namespace dsic {

constexpr int HIST_THREADS = 256, HIST_MAX_BLOCKS = 2048;

template <typename T, bool LDS>
__global__ __launch_bounds__(HIST_THREADS) void band_histogram_kernel(const T* __restrict__ img,
                                                                      const uint8_t* __restrict__ valid, uint64_t n, int C,
                                                                      int nodata, uint32_t* __restrict__ hist) {
  constexpr int BINS = 1 << (8 * sizeof(T));
  __shared__ uint32_t lh[LDS ? 4 * BINS : 1];
  uint32_t* bins = LDS ? lh : hist;
  if (LDS) {
    for (int i = threadIdx.x; i < C * BINS; i += HIST_THREADS) lh[i] = 0;
    __syncthreads();
  }
  const int lane = threadIdx.x & 63;
  uint32_t held[4] = {0, 0, 0, 0}, count[4] = {0, 0, 0, 0};  // the run a lane carries, per channel
  // every lane of a wave takes every step (base is the same for all of them): the shuffles and ballots see all 64
  for (uint64_t base = (uint64_t)blockIdx.x * HIST_THREADS; base < n; base += (uint64_t)gridDim.x * HIST_THREADS) {
    const uint64_t p = base + threadIdx.x;
    bool counted = p < n;
    uint32_t val[4] = {0, 0, 0, 0};
    if (counted) {
      const T* px = img + p * C;
      bool nd = nodata >= 0;
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (c < C) {
          val[c] = (uint32_t)px[c];
          nd = nd && val[c] == (uint32_t)nodata;
        }
      counted = !nd && (!valid || valid[p] != 0);
    }
    const bool before = __shfl_up((int)counted, 1, 64) != 0 && lane > 0;
    // first the shuffles and ballots of all channels, with every lane in them; then the lanes part ways
    uint64_t on[4] = {0, 0, 0, 0};  // per channel, the lanes that continue the run of the lane before
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const uint32_t left = (uint32_t)__shfl_up((int)val[c], 1, 64);
      on[c] = __ballot(counted && before && left == val[c]);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c >= C || !counted || ((on[c] >> lane) & 1)) continue;
      const uint64_t after = lane == 63 ? 0 : on[c] >> (lane + 1);
      const uint32_t run = 1u + (uint32_t)__builtin_ctzll(~after);  // bit 63 of after is 0: ~after is never 0
      if (count[c] && held[c] != val[c]) {
        atomicAdd(bins + c * BINS + held[c], count[c]);
        count[c] = 0;
      }
      held[c] = val[c];
      count[c] += run;
    }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c)
    if (c < C && count[c]) atomicAdd(bins + c * BINS + held[c], count[c]);
  if (LDS) {
    __syncthreads();
    for (int i = threadIdx.x; i < C * BINS; i += HIST_THREADS) {
      const uint32_t k = lh[i];
      if (k) atomicAdd(hist + i, k);
    }
  }
}

template <typename T, bool LDS>
static int band_histogram(const char* what, const T* img, const uint8_t* valid, int H, int W, int C, int nodata,
                          uint32_t* hist, void* stream) {
  constexpr int BINS = 1 << (8 * sizeof(T));
  DSIC_REQUIRE(img && hist, "%s: null pointer", what);
  DSIC_REQUIRE(C >= 1 && C <= 4, "%s: C=%d must be in 1..4", what, C);
  DSIC_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W < ((int64_t)1 << 32), "%s: image %dx%d (at least 1x1, under 2^32 pixels)",
               what, H, W);
  DSIC_REQUIRE(nodata >= -1 && nodata < BINS, "%s: nodata=%d (-1 for none, or a pixel value)", what, nodata);
  DSIC_REQUIRE(((uintptr_t)img & (sizeof(T) - 1)) == 0 && ((uintptr_t)hist & 3) == 0,
               "%s: img must be %d-byte and hist 4-byte aligned", what, (int)sizeof(T));
  const int64_t n = (int64_t)H * W, hb = (int64_t)4 * C * BINS;
  DSIC_REQUIRE(buffers_apart(hist, hb, img, n * C * (int64_t)sizeof(T)) && (!valid || buffers_apart(hist, hb, valid, n)),
               "%s: hist overlaps the image or its validity", what);
  const int64_t blocks = (n + HIST_THREADS - 1) / HIST_THREADS;
  hipLaunchKernelGGL((band_histogram_kernel<T, LDS>), dim3((unsigned)(blocks > HIST_MAX_BLOCKS ? HIST_MAX_BLOCKS : blocks)),
                     dim3(HIST_THREADS), 0, (hipStream_t)stream, img, valid, (uint64_t)n, C, nodata, hist);
  return check_launch(what);
}

// The histogram of an index (codec.ImageReader.index_histogram): hist[u] += the counted pixels whose index, render.h's
// index_value of bands a and b, is u; a normalised difference with A + B = 0 is not counted.  The run-carrying scheme
// above with one value per pixel.  LDS: the 511 counters of a uint8 difference sit in LDS; the 20001 of a normalised
// difference (80 KB of dynamic LDS: two workgroups per CU, each flushing 20001 words) and the 131071 of a uint16
// difference go to the global histogram directly, nearly one global atomic per pixel on a scene as for the uint16 band
// histogram above: 1.75 ms for 4096 x 4096 pixels against 0.06 ms in LDS, beside the 50 ms that decoding that level
// takes, once per reader (DESIGN.md section 3 has the measurements).
constexpr int INDEX_LDS_BINS = 511;

template <typename T, bool LDS>
__global__ __launch_bounds__(HIST_THREADS) void index_histogram_kernel(const T* __restrict__ img,
                                                                       const uint8_t* __restrict__ valid, uint64_t n, int C,
                                                                       int nodata, int kind, int a, int b,
                                                                       uint32_t* __restrict__ hist) {
  __shared__ uint32_t lh[LDS ? INDEX_LDS_BINS : 1];
  uint32_t* bins = LDS ? lh : hist;
  if (LDS) {
    for (int i = threadIdx.x; i < INDEX_LDS_BINS; i += HIST_THREADS) lh[i] = 0;
    __syncthreads();
  }
  const int lane = threadIdx.x & 63;
  const uint32_t top = (uint32_t)(T)~(T)0;
  uint32_t held = 0, count = 0;  // the run a lane carries
  // every lane of a wave takes every step, as above
  for (uint64_t base = (uint64_t)blockIdx.x * HIST_THREADS; base < n; base += (uint64_t)gridDim.x * HIST_THREADS) {
    const uint64_t p = base + threadIdx.x;
    bool counted = p < n;
    uint32_t u = 0;
    if (counted) {
      const T* px = img + p * C;
      bool nd = nodata >= 0;
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (c < C) nd = nd && (uint32_t)px[c] == (uint32_t)nodata;
      counted = index_value(kind, (uint32_t)px[a], (uint32_t)px[b], top, &u) && !nd && (!valid || valid[p] != 0);
    }
    const bool before = __shfl_up((int)counted, 1, 64) != 0 && lane > 0;
    const uint32_t left = (uint32_t)__shfl_up((int)u, 1, 64);
    const uint64_t on = __ballot(counted && before && left == u);  // the lanes that continue the run of the lane before
    if (counted && !((on >> lane) & 1)) {  // the head of a run
      const uint64_t after = lane == 63 ? 0 : on >> (lane + 1);
      const uint32_t run = 1u + (uint32_t)__builtin_ctzll(~after);  // bit 63 of after is 0: ~after is never 0
      if (count && held != u) {
        atomicAdd(bins + held, count);
        count = 0;
      }
      held = u;
      count += run;
    }
  }
  if (count) atomicAdd(bins + held, count);
  if (LDS) {
    __syncthreads();
    for (int i = threadIdx.x; i < INDEX_LDS_BINS; i += HIST_THREADS) {
      const uint32_t k = lh[i];
      if (k) atomicAdd(hist + i, k);
    }
  }
}

template <typename T>
static int index_histogram(const char* what, const T* img, const uint8_t* valid, int H, int W, int C, int nodata, int kind,
                           int a, int b, uint32_t* hist, void* stream) {
  constexpr int top = (int)(T)~(T)0;
  DSIC_REQUIRE(img && hist, "%s: null pointer", what);
  DSIC_REQUIRE(C >= 1 && C <= 4, "%s: C=%d must be in 1..4", what, C);
  DSIC_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W < ((int64_t)1 << 32), "%s: image %dx%d (at least 1x1, under 2^32 pixels)",
               what, H, W);
  DSIC_REQUIRE(nodata >= -1 && nodata <= top, "%s: nodata=%d (-1 for none, or a pixel value)", what, nodata);
  DSIC_REQUIRE(kind == INDEX_DIFFERENCE || kind == INDEX_ND,
               "%s: kind=%d (1 difference, 2 nd; a band is counted by the band histogram)", what, kind);
  const int status = index_bands(what, C, kind, a, b);
  if (status != DSIC_OK) return status;
  DSIC_REQUIRE(((uintptr_t)img & (sizeof(T) - 1)) == 0 && ((uintptr_t)hist & 3) == 0,
               "%s: img must be %d-byte and hist 4-byte aligned", what, (int)sizeof(T));
  const int64_t n = (int64_t)H * W, hb = (int64_t)4 * (kind == INDEX_ND ? INDEX_ND_BINS : 2 * top + 1);
  DSIC_REQUIRE(buffers_apart(hist, hb, img, n * C * (int64_t)sizeof(T)) && (!valid || buffers_apart(hist, hb, valid, n)),
               "%s: hist overlaps the image or its validity", what);
  const int64_t blocks = (n + HIST_THREADS - 1) / HIST_THREADS;
  const dim3 grid((unsigned)(blocks > HIST_MAX_BLOCKS ? HIST_MAX_BLOCKS : blocks));
  if (kind == INDEX_DIFFERENCE && 2 * top + 1 <= INDEX_LDS_BINS)
    hipLaunchKernelGGL((index_histogram_kernel<T, true>), grid, dim3(HIST_THREADS), 0, (hipStream_t)stream, img, valid,
                       (uint64_t)n, C, nodata, kind, a, b, hist);
  else
    hipLaunchKernelGGL((index_histogram_kernel<T, false>), grid, dim3(HIST_THREADS), 0, (hipStream_t)stream, img, valid,
                       (uint64_t)n, C, nodata, kind, a, b, hist);
  return check_launch(what);
}

}  // namespace dsic

using namespace dsic;

extern "C" int dsic_band_histogram_u8(const uint8_t* img_hwc, const uint8_t* valid_hw, int H, int W, int C, int nodata,
                                      uint32_t* hist, void* stream) {
  return band_histogram<uint8_t, true>("band_histogram_u8", img_hwc, valid_hw, H, W, C, nodata, hist, stream);
}

extern "C" int dsic_band_histogram_u16(const uint16_t* img_hwc, const uint8_t* valid_hw, int H, int W, int C, int nodata,
                                       uint32_t* hist, void* stream) {
  return band_histogram<uint16_t, false>("band_histogram_u16", img_hwc, valid_hw, H, W, C, nodata, hist, stream);
}

extern "C" int dsic_index_histogram_u8(const uint8_t* img_hwc, const uint8_t* valid_hw, int H, int W, int C, int nodata,
                                       int kind, int band_a, int band_b, uint32_t* hist, void* stream) {
  return index_histogram<uint8_t>("index_histogram_u8", img_hwc, valid_hw, H, W, C, nodata, kind, band_a, band_b, hist,
                                  stream);
}

extern "C" int dsic_index_histogram_u16(const uint16_t* img_hwc, const uint8_t* valid_hw, int H, int W, int C, int nodata,
                                        int kind, int band_a, int band_b, uint32_t* hist, void* stream) {
  return index_histogram<uint16_t>("index_histogram_u16", img_hwc, valid_hw, H, W, C, nodata, kind, band_a, band_b, hist,
                                   stream);
}
