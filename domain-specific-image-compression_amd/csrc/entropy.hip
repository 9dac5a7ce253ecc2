// Per-patch entropy coding on the GPU: support scan, CDF tables, range
// encoder / decoder.  Restates the intent of
// code/modelv2/eval_selfcontained_entropy.py:14-23 (gaussian_cdf,
// pmf_to_uint16_cdf), :36-62 (per-image support, PMFs, z-then-y strings) and
// :86-116 (decode), with the torchac 0.9.3 coder it calls (:48,62,96,116;
// third-party: 32-bit low/high, 16-bit precision, pending-bit carry
// resolution).  Interpretation choices are frozen in DESIGN.md "Entropy path".
//
// Parallel structure: tables are embarrassingly parallel (one wave per
// (image, channel) table: the 64 lanes evaluate the boundary CDFs and finish the
// table an entry each; its two order-sensitive sums keep the reference's serial
// order, finish_table_wave).  The coder's interval
// update is a serial dependency chain per string, so one wave per string runs it
// on wave-uniform values (the scalar unit): the 64 lanes translate 64 symbols to
// packed (c_low, c_high - 1) pairs in parallel, the chain reads them lane by lane
// (v_readlane) and records per symbol only the interval before renormalisation.
// Which bits a symbol emits, what is owed in front of them and where they go are
// prefix sums over those records, 64 lanes at a time, ORed into the zero-filled
// output.  Matching leading bits and pending (E3) runs are shifted out in bulk
// with clz instead of bit by bit; the emitted bytes are identical to the
// bit-serial reference loop.  The interval step (IntervalStep), the bit
// bookkeeping (place_group), the bit placement (put_group, put_flush) and the
// symbol lookup (pair_of) are each stated once: the split encoder runs them in
// separate launches, the single kernel in one wave, the decoder's fast path
// shares the interval step.
// Integer work only after the tables: results are bit-exact by construction.
#include "common.h"
#include "dsic_math.h"

#include <climits>

namespace dsic {

// meta[b] = {ymin - tail, Ly, zmin - tail, Lz}: :39-41, :52-54 (the model's values are
// integers already, so floor/ceil are the identity).
__global__ __launch_bounds__(256) void support_kernel(const float* __restrict__ y,
                                                      const float* __restrict__ z,
                                                      int* __restrict__ meta, int64_t ny, int64_t nz,
                                                      int tail) {
  __shared__ float red[2][4];
  __shared__ int bad_any;
  const int b = blockIdx.x;
  for (int which = 0; which < 2; ++which) {
    const float* p = which ? z + (size_t)b * nz : y + (size_t)b * ny;
    const int64_t n = which ? nz : ny;
    float mn = p[0], mx = p[0];
    bool bad = false;  // NaN, infinity or a magnitude no int support can hold
    for (int64_t i = threadIdx.x; i < n; i += 256) {
      const float v = p[i];
      bad |= !(fabsf(v) < 1.0e9f);
      mn = fminf(mn, v);
      mx = fmaxf(mx, v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      mn = fminf(mn, __shfl_down(mn, o, 64));
      mx = fmaxf(mx, __shfl_down(mx, o, 64));
    }
    if (threadIdx.x == 0) bad_any = 0;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
      red[0][threadIdx.x >> 6] = mn;
      red[1][threadIdx.x >> 6] = mx;
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(&bad_any, 1);
    __syncthreads();
    if (threadIdx.x == 0) {
      mn = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
      mx = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
      if (bad_any) {
        // non-finite latents have no support: width 0 makes every consumer of `meta` raise err bit 1
        meta[4 * b + 2 * which] = 0;
        meta[4 * b + 2 * which + 1] = 0;
      } else {
        const int lo = (int)floorf(mn) - tail, hi = (int)ceilf(mx) + tail;
        meta[4 * b + 2 * which] = lo;
        meta[4 * b + 2 * which + 1] = hi - lo + 1;
      }
    }
    __syncthreads();
  }
}

// dm::finish_table with the 64 lanes of a wave: everything that is element-wise (pmf, clamp, divide, scaling,
// truncation, spreading) runs one entry per lane; the two order-sensitive reductions keep the serial order of the
// host function - the float32 sum (torch's cascade) is evaluated by every lane alike, the float64 running sum walks
// the entries through v_readlane.  Same operations on the same operands: the tables are bit-identical to
// dm::finish_table (tests/test_gpu_entropy.py compares them with the host entry point, tests/test_gpu_table_elements.py
// with the oracle over the whole parameter domain).  F[0..L] is overwritten with the rounded prefixes; the last one
// (and with it the `c < 1.0f` select) feeds only raw[L] of the host function: out[k] reads prefix k - 1.
__device__ __forceinline__ void finish_table_wave(float* F, int L, uint16_t* out, float* pmf, int lane) {
  for (int k = lane; k < L; k += 64) {
    float p = F[k + 1] - F[k];
    if (p < 1e-12f) p = 1e-12f;
    pmf[k] = p;
  }
  __builtin_amdgcn_s_waitcnt(0xc07f);
  __builtin_amdgcn_wave_barrier();
  const float total = dm::sum_f32_torch(pmf, L);
  double cum = 0.0;
  for (int base = 0; base < L; base += 64) {
    const int k = base + lane;
    const float q = k < L ? pmf[k] / total : 0.0f;
    const int n = L - base < 64 ? L - base : 64;
    float mine = 0.0f;
    for (int j = 0; j < n; ++j) {
      const float qj = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, q), j));
      cum = cum + (double)qj;
      float c = (float)cum;
      if (base + j == L - 1 && c < 1.0f) c = 1.0f;
      if (j == lane) mine = c;
    }
    if (k < L) F[k] = mine;       // prefix that includes entry k
  }
  __builtin_amdgcn_s_waitcnt(0xc07f);
  __builtin_amdgcn_wave_barrier();
  for (int k = lane; k < L; k += 64) {
    uint32_t u16 = 0;
    if (k > 0) {
      float sc = F[k - 1] * 65535.0f;
      if (sc < 0.0f) sc = 0.0f;
      if (sc > 65535.0f) sc = 65535.0f;
      u16 = (uint32_t)sc;
    }
    out[k] = (uint16_t)((u16 * (uint32_t)(65536 - L)) / 65535u + (uint32_t)k);   // < 2^32: one 32-bit division
  }
}

// One wave per table.  sigma/nu indexed [b*sb + c] (sb = 0 for the image-independent z prior).
// Student-t: F at the boundaries b and -b comes from one evaluation of the tail, which depends on t^2 only (IEEE
// division and squaring are sign-symmetric): on a support that straddles 0 the lanes walk the distinct |b| and each
// writes F at both signs.  The boundary of u = smin + k is float(u) - 0.5f; |b| = float(w) - 0.5f with w = u for
// u >= 1, w = 1 - u for u <= 0 (exact: a straddling support has |u| <= Lmax + 1).  Elsewhere every k is its own.
template <bool STUDENT>
__global__ __launch_bounds__(256) void tables_kernel(const float* __restrict__ sigma,
                                                     const float* __restrict__ nu, int sb,
                                                     const int* __restrict__ meta, int meta_off,
                                                     uint16_t* __restrict__ tables, int C, int Lmax,
                                                     int ntables, int* __restrict__ err) {
  extern __shared__ float shm[];  // per wave: F[Lmax+1], pmf[Lmax]
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int tid = blockIdx.x * 4 + wave;
  if (tid >= ntables) return;
  const int b = tid / C, c = tid % C;
  const int smin = meta[4 * b + meta_off], L = meta[4 * b + meta_off + 1];
  if (L > Lmax || L < 1) {
    if (lane == 0) atomicOr(err, 1);
    return;
  }
  float* F = shm + (size_t)wave * (2 * Lmax + 1);
  float* pmf = F + Lmax + 1;
  const float sg = sigma[(size_t)b * sb + c];
  const float nv = STUDENT ? nu[(size_t)b * sb + c] : 0.0f;
  if (STUDENT && smin <= 0 && smin + L >= 1) {
    const int whi = smin + L > 1 - smin ? smin + L : 1 - smin;   // w = 1 .. whi
    for (int w = 1 + lane; w <= whi; w += 64) {
      const double tail = dm::student_t_tail((double)((float)w - 0.5f) / (double)sg, (double)nv);
      if (w <= smin + L) F[w - smin] = (float)(1.0 - tail);   // u = w
      if (1 - w >= smin) F[1 - w - smin] = (float)tail;       // u = 1 - w
    }
  } else {
    for (int k = lane; k <= L; k += 64)
      F[k] = STUDENT ? dm::table_cdf_student(smin, k, sg, nv) : dm::table_cdf_gauss(smin, k, sg);
  }
  __builtin_amdgcn_s_waitcnt(0xc07f);
  __builtin_amdgcn_wave_barrier();
  finish_table_wave(F, L, tables + ((size_t)b * C + c) * Lmax, pmf, lane);
}

// z tables: sigma is per channel (the same for every image) and a boundary's value depends on u = smin + k only,
// so the tables of one channel evaluate the same CDF values for every image.  One workgroup per (channel, ZT_IMGS
// images): the 256 threads evaluate the channel's CDF once over the union of those images' supports, then each wave
// finishes the tables of ZT_IMGS / 4 images from their slices of that row.  A union wider than `rowmax` boundaries
// (supports far apart) evaluates each table's own boundaries, as tables_kernel<false>.
constexpr int ZT_IMGS = 16;

__global__ __launch_bounds__(256) void gauss_tables_kernel(const float* __restrict__ sigma,
                                                           const int* __restrict__ meta,
                                                           uint16_t* __restrict__ tables, int B, int C, int Lmax,
                                                           int rowmax, int* __restrict__ err) {
  extern __shared__ float shm[];  // row[rowmax], then per wave F[Lmax+1], pmf[Lmax]
  __shared__ int ulo, uhi;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int c = blockIdx.x, b0 = blockIdx.y * ZT_IMGS;
  const int b1 = B - b0 < ZT_IMGS ? B : b0 + ZT_IMGS;
  const float sg = sigma[c];
  if (wave == 0) {   // union [lo, hi] of the valid supports' u = smin .. smin + L
    int lo = INT_MAX, hi = INT_MIN;
    if (b0 + lane < b1 && lane < ZT_IMGS) {
      const int smin = meta[4 * (b0 + lane) + 2], L = meta[4 * (b0 + lane) + 3];
      if (L >= 1 && L <= Lmax) {
        lo = smin;
        hi = smin + L;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      lo = min(lo, __shfl_xor(lo, o, 64));
      hi = max(hi, __shfl_xor(hi, o, 64));
    }
    if (lane == 0) {
      ulo = lo;
      uhi = hi;
    }
  }
  __syncthreads();
  const int lo = ulo, hi = uhi;
  const bool shared_row = hi >= lo && (int64_t)hi - lo < (int64_t)rowmax;
  float* row = shm;
  if (shared_row)
    for (int u = lo + (int)threadIdx.x; u <= hi; u += 256) row[u - lo] = dm::table_cdf_gauss(u, 0, sg);
  __syncthreads();
  float* F = shm + rowmax + (size_t)wave * (2 * Lmax + 1);
  float* pmf = F + Lmax + 1;
  for (int b = b0 + wave; b < b1; b += 4) {
    const int smin = meta[4 * b + 2], L = meta[4 * b + 3];
    if (L > Lmax || L < 1) {
      if (lane == 0) atomicOr(err, 1);
      continue;
    }
    for (int k = lane; k <= L; k += 64) F[k] = shared_row ? row[smin + k - lo] : dm::table_cdf_gauss(smin, k, sg);
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
    finish_table_wave(F, L, tables + ((size_t)b * C + c) * Lmax, pmf, lane);
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
  }
}

// ---- range encoder ----------------------------------------------------------------------------------------------
// The coder is split along its only true dependency.  (1) The interval recurrence is a serial chain per string: it
// runs branch-free on wave-uniform values (scalar unit), reading the (c_low, c_high - 1) pair of symbol j with
// v_readlane from a register the 64 lanes filled in parallel, and records per symbol only (low1, high1), the interval
// BEFORE renormalisation (v_writelane).  (2) WHAT a symbol emits - the leading bits of low1 that became final (E1/E2)
// and the inverse bits owed from the E3 runs since the last such symbol - is recomputed from the records by the 64
// lanes in parallel (place_group), and WHERE those bits go is a prefix sum of their counts (put_group).  Bytes are
// identical to the bit-serial reference loop (torchac): E1/E2 shifts = clz(low ^ high) at once, E3 run = leading
// ones of (low << 1) & ~(high << 1).
//
// Interval state (low, span, lowm1): span = high - low + 1 kept mod 2^32 (0 means 2^32), lowm1 = low - 1.  Bounds
// (cl, ch) = (c_low << 16, c_high << 16), so floor(span c / 2^16) is ONE mul_hi; ch = 0 means c_high = 65536, whose
// product is span itself, and span = 0 selects (2^32 c) >> 16 = c << 16 (a select: 4 % faster than a branch per
// symbol).
struct IntervalStep {
  uint32_t low1, high1, span1;   // the symbol's interval before renormalisation; span1 >= 2^14 - 1
  // nb: leading bits now final (E1/E2); m: (1, 0) bit pairs below the split bit (E3)
  __device__ __forceinline__ void shifts(int& nb, int& m) const {
    nb = __builtin_clz(low1 ^ high1);
    const uint32_t q2 = (high1 | ~low1) << 1;   // 0 where (low, high) = (1, 0)
    m = __builtin_clz(q2 << nb);                // != 0: an all-E3 tail would need span1 == 2
  }
  // after both renormalisation shifts at once (sh = nb + m <= 18, as span1 << sh <= 2^32)
  __device__ __forceinline__ uint32_t low(int sh) const { return (low1 << sh) & 0x7FFFFFFFu; }
  __device__ __forceinline__ uint32_t span(int sh) const { return span1 << sh; }   // exactly 2^32 -> 0
};

// One symbol in two halves, so that an encoder records (low1, high1) between them.  The chain span -> span of the next
// symbol is ~9 dependent scalar operations (mul_hi, select, sub/add, xor | orn2, flbit | shift, shift, flbit, add,
// shift); low - 1 and the record sit beside it.  TOP: ch = 0 (c_high = 65536) may occur.
template <bool TOP>
__device__ __forceinline__ IntervalStep interval_narrow(uint32_t low, uint32_t lowm1, uint32_t span, uint32_t cl,
                                                        uint32_t ch) {
  const uint32_t ml = __umulhi(span, cl), mh = __umulhi(span, ch);
  const uint32_t lo_add = span ? ml : cl;
  const uint32_t hi_add = TOP && !ch ? span : (span ? mh : ch);
  return IntervalStep{low + lo_add, lowm1 + hi_add, hi_add - lo_add};   // low - 1 + floor(span c_high / 2^16)
}

__device__ __forceinline__ void interval_renorm(const IntervalStep& s, uint32_t& low, uint32_t& lowm1,
                                                uint32_t& span) {
  int nb, m;
  s.shifts(nb, m);
  span = s.span(nb + m);
  low = s.low(nb + m);
  lowm1 = low - 1u;
}

template <int J>
__device__ __forceinline__ void wlane(uint32_t& rec, uint32_t v) {
  asm volatile("v_writelane_b32 %0, %1, %2" : "+v"(rec) : "s"(v), "n"(J));
}

template <int J>
__device__ __forceinline__ uint32_t rlane(uint32_t v) {
  uint32_t r;
  asm volatile("v_readlane_b32 %0, %1, %2" : "=s"(r) : "v"(v), "n"(J));
  return r;
}

// Where the steps of a full group of 64 take their bounds from: the only thing in which the two encoders' 64-step
// blocks differ.
//  PackedPairs: one register of packed pairs, unpacked by scalar operations; c_high = 65536 allowed.  One v_readlane
//               per symbol and a register less: the chain kernel (8 VGPRs).
//  LaneBounds:  (c_low << 16, c_high << 16) in two registers, every c_high < 65536.  Two v_readlane per symbol, no
//               unpacking and no select on ch: 3 % faster where registers are free (the single kernel).
struct PackedPairs {
  static constexpr bool TOP = true;
  template <int J>
  static __device__ __forceinline__ void fetch(uint32_t pv, uint32_t, uint32_t& p, uint32_t&) { p = rlane<J>(pv); }
  static __device__ __forceinline__ void bounds(uint32_t p, uint32_t, uint32_t& cl, uint32_t& ch) {
    cl = p << 16;
    ch = (p & 0xFFFF0000u) + 0x10000u;
  }
};
struct LaneBounds {
  static constexpr bool TOP = false;
  template <int J>
  static __device__ __forceinline__ void fetch(uint32_t clo16, uint32_t chi16, uint32_t& l, uint32_t& h) {
    l = rlane<J>(clo16);
    h = rlane<J>(chi16);
  }
  static __device__ __forceinline__ void bounds(uint32_t l, uint32_t h, uint32_t& cl, uint32_t& ch) {
    cl = l;
    ch = h;
  }
};

// Symbol J of a full group, unrolled with immediate lane selects (no M0 / wait-state padding).  (cl, ch): the bounds
// of symbol J, fetched one step earlier; the step first reads those of symbol J + 1, so the VALU -> SGPR latency of
// v_readlane never sits on the serial chain.  ~22 scalar instructions per symbol.
template <class Src, int J>
__device__ __forceinline__ void chain_step(uint32_t& low, uint32_t& lowm1, uint32_t& span, uint32_t& cl, uint32_t& ch,
                                           uint32_t v0, uint32_t v1, uint32_t& rec_low, uint32_t& rec_high) {
  uint32_t n0 = 0u, n1 = 0u;
  if (J < 63) Src::template fetch<(J < 63 ? J + 1 : 63)>(v0, v1, n0, n1);
  const IntervalStep s = interval_narrow<Src::TOP>(low, lowm1, span, cl, ch);
  wlane<J>(rec_low, s.low1);
  wlane<J>(rec_high, s.high1);
  interval_renorm(s, low, lowm1, span);
  Src::bounds(n0, n1, cl, ch);
}

template <class Src, int J0>
__device__ __forceinline__ void chain_steps8(uint32_t& low, uint32_t& lowm1, uint32_t& span, uint32_t& cl,
                                             uint32_t& ch, uint32_t v0, uint32_t v1, uint32_t& rl, uint32_t& rh) {
  chain_step<Src, J0 + 0>(low, lowm1, span, cl, ch, v0, v1, rl, rh);
  chain_step<Src, J0 + 1>(low, lowm1, span, cl, ch, v0, v1, rl, rh);
  chain_step<Src, J0 + 2>(low, lowm1, span, cl, ch, v0, v1, rl, rh);
  chain_step<Src, J0 + 3>(low, lowm1, span, cl, ch, v0, v1, rl, rh);
  chain_step<Src, J0 + 4>(low, lowm1, span, cl, ch, v0, v1, rl, rh);
  chain_step<Src, J0 + 5>(low, lowm1, span, cl, ch, v0, v1, rl, rh);
  chain_step<Src, J0 + 6>(low, lowm1, span, cl, ch, v0, v1, rl, rh);
  chain_step<Src, J0 + 7>(low, lowm1, span, cl, ch, v0, v1, rl, rh);
}

// a full group: the records of its 64 symbols in (rl, rh)
template <class Src>
__device__ __forceinline__ void chain_group(uint32_t v0, uint32_t v1, uint32_t& low, uint32_t& lowm1, uint32_t& span,
                                            uint32_t& rl, uint32_t& rh) {
  uint32_t n0 = 0u, n1 = 0u, cl, ch;
  Src::template fetch<0>(v0, v1, n0, n1);
  Src::bounds(n0, n1, cl, ch);
  chain_steps8<Src, 0>(low, lowm1, span, cl, ch, v0, v1, rl, rh);
  chain_steps8<Src, 8>(low, lowm1, span, cl, ch, v0, v1, rl, rh);
  chain_steps8<Src, 16>(low, lowm1, span, cl, ch, v0, v1, rl, rh);
  chain_steps8<Src, 24>(low, lowm1, span, cl, ch, v0, v1, rl, rh);
  chain_steps8<Src, 32>(low, lowm1, span, cl, ch, v0, v1, rl, rh);
  chain_steps8<Src, 40>(low, lowm1, span, cl, ch, v0, v1, rl, rh);
  chain_steps8<Src, 48>(low, lowm1, span, cl, ch, v0, v1, rl, rh);
  chain_steps8<Src, 56>(low, lowm1, span, cl, ch, v0, v1, rl, rh);
}

// cnt (1..64) symbols of a group of packed pairs, any c_high: the same step in a loop; lanes cnt.. of (rl, rh) are left as they were.
// v_writelane has no clang builtin on this toolchain.  The lane select goes through M0 (an SGPR value plus an SGPR
// lane select would exceed the constant-bus limit); s_nop 3: an SALU result needs 4 wait states before it is used as
// a lane select, and hipcc pads nothing inside asm.  The encoders use no GWS or movrel, so M0 is otherwise unused.
__device__ __forceinline__ void chain_tail(uint32_t pv, int cnt, uint32_t& low, uint32_t& lowm1, uint32_t& span,
                                           uint32_t& rl, uint32_t& rh) {
  for (int j = 0; j < cnt; ++j) {
    const uint32_t pr = __builtin_amdgcn_readlane(pv, j);
    const IntervalStep s = interval_narrow<true>(low, lowm1, span, pr << 16, (pr & 0xFFFF0000u) + 0x10000u);
    asm volatile("s_mov_b32 m0, %4\n\ts_nop 3\n\tv_writelane_b32 %0, %2, m0\n\tv_writelane_b32 %1, %3, m0"
                 : "+v"(rl), "+v"(rh)
                 : "s"(s.low1), "s"(s.high1), "s"(j));
    interval_renorm(s, low, lowm1, span);
  }
}

// One group of 64 records; lane j: symbol j of the group, lanes past the end hold (0, ~0): no bit, no E3 run.
// Per lane the number of final bits of the symbol (nbv, the top bits of lo) and the inverse bits owed behind the first
// of them (pendv, 0 unless nbv > 0); `pending` (wave-uniform) goes from the count owed in front of the group to the
// count owed behind it.
__device__ __forceinline__ void place_group(uint32_t lo, uint32_t hi, int lane, uint32_t& pending, uint32_t& nbv,
                                            uint32_t& pendv) {
  nbv = (uint32_t)__builtin_clz(lo ^ hi);
  const uint32_t mv = (uint32_t)__builtin_clz((((hi | ~lo) << nbv) << 1) | 1u);
  // pending count in front of symbol j = sum of the E3 runs since the last symbol that emitted bits (its own run
  // included), or since the carry-in: a segmented prefix sum
  uint32_t T = mv;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t up = __shfl_up(T, o, 64);
    if (lane >= o) T += up;
  }
  const uint32_t Tex = T - mv;
  const uint64_t heads = __ballot(nbv > 0);
  const uint64_t before = heads & ((1ull << lane) - 1ull);
  const int hb = 63 - __builtin_clzll(before | 1ull);
  const uint32_t Tex_h = __shfl(Tex, hb, 64);
  const uint32_t pend_in = before ? Tex - Tex_h : pending + Tex;
  pendv = nbv ? pend_in : 0u;
  const int hl = 63 - __builtin_clzll(heads | 1ull);
  const uint32_t T63 = __builtin_amdgcn_readlane(T, 63);
  const uint32_t Tex_hl = __builtin_amdgcn_readlane(Tex, hl);
  pending = heads ? T63 - Tex_hl : pending + T63;
}

// ---- bit placement ----------------------------------------------------------------------------------------------
// A string's bits are ORed into its zero-initialised capacity as big-endian 32-bit words, in pieces of at most 32
// bits at any bit offset, by any lane in any order.  WIN: the words wbase .. wbase + PLACE_WIN - 1 are ORed in an LDS
// window (which its owner adds to the output later, one global atomic per word instead of one per piece), the rest
// straight into the output; !WIN: every word goes straight to the output.  A piece that would end behind the capacity
// is dropped whole and *overflow set (error bit 4).
constexpr int PLACE_WIN = 512;
struct BitSink {
  uint32_t* out32;    // the string's capacity
  int64_t cap_bits;
  uint32_t* win;      // WIN only
  int64_t wbase;
};

template <bool WIN>
__device__ __forceinline__ void or_word(const BitSink& S, int64_t w, uint32_t v) {
  const int64_t i = w - S.wbase;
  if (WIN && i >= 0 && i < PLACE_WIN) atomicOr(S.win + i, v);
  else atomicOr(S.out32 + w, v);
}

// append the low `len` (1..32) bits of v at bit offset `off`, MSB first
template <bool WIN>
__device__ __forceinline__ void put_bits(const BitSink& S, int64_t off, uint32_t v, int len, int* overflow) {
  if (off + len > S.cap_bits) {
    *overflow = 1;
    return;
  }
  const int64_t w = off >> 5;
  const int s = (int)(off & 31), space = 32 - s;
  if (len <= space) {
    or_word<WIN>(S, w, __builtin_bswap32(v << (space - len)));
  } else {
    const int rest = len - space;
    or_word<WIN>(S, w, __builtin_bswap32(v >> rest));
    or_word<WIN>(S, w + 1, __builtin_bswap32(v << (32 - rest)));
  }
}

template <bool WIN>
__device__ __forceinline__ void put_ones(const BitSink& S, int64_t off, uint32_t count, int* overflow) {
  while (count > 0) {
    const int len = count > 32 ? 32 : (int)count;
    put_bits<WIN>(S, off, len == 32 ? 0xFFFFFFFFu : ((1u << len) - 1u), len, overflow);
    off += len;
    count -= len;
  }
}

// a first bit and the `pend` inverse bits behind it: a run of ones after a 0; after a 1 the run is zeros, which are
// there already but count against the capacity all the same
template <bool WIN>
__device__ __forceinline__ void put_resolved(const BitSink& S, int64_t off, uint32_t first, uint32_t pend,
                                             int* overflow) {
  put_bits<WIN>(S, off, first, 1, overflow);
  if (!first) put_ones<WIN>(S, off + 1, pend, overflow);
  else if (off + 1 + (int64_t)pend > S.cap_bits) *overflow = 1;
}

// The bits of one group (place_group's nbv, pendv; lo: the records' low1) from bit offset `off` on: lane j places
// the pieces of symbol j behind those of the lanes before it - all its bits at once, or its first bit, the inverse
// bits owed, the rest.  Returns the group's bit count.
template <bool WIN>
__device__ __forceinline__ uint32_t put_group(const BitSink& S, int64_t off, uint32_t lo, uint32_t nbv, uint32_t pendv,
                                              int lane, int* overflow) {
  const uint32_t len = nbv + pendv;
  uint32_t incl = len;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  const int64_t o = off + (int64_t)(incl - len);
  if (nbv > 0) {
    const uint32_t bitsv = lo >> (32u - nbv);
    if (pendv == 0) {
      put_bits<WIN>(S, o, bitsv, (int)nbv, overflow);
    } else {
      put_resolved<WIN>(S, o, bitsv >> (nbv - 1), pendv, overflow);
      if (nbv > 1) put_bits<WIN>(S, o + 1 + pendv, bitsv & ((1u << (nbv - 1)) - 1u), (int)nbv - 1, overflow);
    }
  }
  return (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
}

// The end of a string of `total` bits (torchac's flush), by one lane and straight into the output: one more pending
// bit, then the deciding bit and the pending run; the zero padding is there already.  Returns the length in bytes.
__device__ __forceinline__ int put_flush(const BitSink& S, int64_t total, uint32_t pending, uint32_t low,
                                         int* overflow) {
  const uint32_t pend = pending + 1u;
  put_resolved<false>(S, total, low < 0x40000000u ? 0u : 1u, pend, overflow);
  return (int)((total + 1 + (int64_t)pend + 7) >> 3);
}

// ---- strings and symbols ----------------------------------------------------------------------------------------
// Stream ids: s < B is the y string of image s (which = 1), B + b the z string of image b (which = 0).
// Segments (dsic_range_encode_seg_ws): the y string of an image is coded as K = 2^lk independent strings, segment k =
// its symbols [k ns, (k + 1) ns) with ns = ny / K (M / K channels), so the pairs and records of the B K segment
// strings lie back to back: string s < B K is segment s & (K - 1) of image s >> lk at symbol s * ns, string B K + b
// the z string b at B ny + b nz.  K = 1 is the unsegmented coder.
struct SplitGeom {
  int B, M, HWy, N, HWz, Lmax, per_element_y;
  int K, lk;    // y segments per image and log2 of it
  int64_t ny, nz;
  int64_t ns;   // symbols of one y segment
  int gy, gz;   // place: 64-symbol groups per slice of a y segment / z string (place_slicing)
  int ky, kz;   // place: slices per y segment / z string
  // the whole strings of an image, as the symbols are looked up: s < B is y string s, B + b the z string b
  __device__ __forceinline__ void image(int s, int& which, int& b, int64_t& n, int64_t& base) const {
    which = s < B ? 1 : 0;
    b = which ? s : s - B;
    n = which ? ny : nz;
    base = which ? (int64_t)b * ny : (int64_t)B * ny + (int64_t)b * nz;
  }
  __device__ __forceinline__ void stream(int s, int& which, int& b, int64_t& n, int64_t& base) const {
    const int BK = B << lk;
    which = s < BK ? 1 : 0;
    b = which ? s >> lk : s - BK;
    n = which ? ns : nz;
    base = which ? (int64_t)s * ns : (int64_t)B * ny + (int64_t)b * nz;
  }
  __device__ __forceinline__ int nslices() const { return (B << lk) * ky + B * kz; }
  // place slice q (0 .. nslices() - 1; y segments first) -> string s, slice k of the string, its slice count and
  // the index of the string's first slice record
  __device__ __forceinline__ void slice(int q, int& s, int& k, int& ks, int& gs, int& q0) const {
    const int BK = B << lk;
    const int qz = q - BK * ky;
    const bool y = qz < 0;
    ks = y ? ky : kz;
    gs = y ? gy : gz;
    s = y ? q / ky : BK + qz / kz;
    k = y ? q % ky : qz % kz;
    q0 = q - k;
  }
};

// Groups of 64 symbols per place slice: at least 8 (one slice = one wave's short walk), more for long strings so
// that a string has at most 256 slices (the records a wave composes before it emits).
static inline void place_slicing(int64_t n, int& groups, int& slices) {
  const int64_t ng = (n + 63) / 64;
  const int64_t g = (ng + 255) / 256 > 8 ? (ng + 255) / 256 : 8;
  groups = (int)g;
  slices = (int)((ng + g - 1) / g);
}

// table row t, symbol sc of a support of L -> c_low | (c_high - 1) << 16.  A symbol outside the support (cannot happen
// when meta came from dsic_latent_support on the same latents) raises error bit 2 and is coded as symbol 0.
__device__ __forceinline__ uint32_t pair_of(const uint16_t* t, int sc, int L, int* err) {
  if (sc < 0 || sc >= L) {
    atomicOr(err, 2);
    sc = 0;
  }
  const uint32_t c_low = t[sc];
  const uint32_t c_high = (sc == L - 1) ? 0x10000u : (uint32_t)t[sc + 1];
  return c_low | ((c_high - 1u) << 16);
}

// ---- single-kernel encoder (dsic_range_encode) --------------------------------------------------------------------
// The split encoder's functions in one wave per (image, string): stream ids 0..B-1 = y strings, B..2B-1 = z strings;
// several strings (one per SIMD) may share a workgroup.  Per group of 64 symbols: pair_of by the lanes, chain_group
// (chain_tail for a partial group or one that holds the top symbol, c_high = 65536) on the scalar unit, place_group
// and put_group by the lanes.  It has registers to spare, so its 64-step block takes LaneBounds.
__global__ __launch_bounds__(1024) void range_encode_kernel(
    const float* __restrict__ y, const float* __restrict__ z, const int* __restrict__ meta,
    const uint16_t* __restrict__ tab_y, const uint16_t* __restrict__ tab_z, int Lmax, int M, int HWy,
    int N, int HWz, uint8_t* __restrict__ out, int64_t cap_y, int64_t cap_z,
    int* __restrict__ lengths, int* __restrict__ err, int nstreams, int per_element_y) {
  const int lane = threadIdx.x & 63;
  const int sid = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
  if (sid >= nstreams) return;
  // streams 0..B-1 are the long y strings, B..2B-1 the short z strings: the y waves share as few
  // workgroups (= CUs, which a persistent conv workgroup cannot use meanwhile) as possible
  const int nimg = nstreams >> 1;
  const int which = sid < nimg ? 1 : 0, b = which ? sid : sid - nimg;
  const int C = which ? M : N, HW = which ? HWy : HWz;
  const int64_t n = (int64_t)C * HW;
  const float* sym = which ? y + (size_t)b * n : z + (size_t)b * n;
  const bool per_element = which && per_element_y;  // spatial_params: one table row per y symbol
  const uint16_t* tab = (which ? tab_y + (size_t)b * (per_element ? (size_t)M * HWy : (size_t)M) * Lmax
                               : tab_z + (size_t)b * N * Lmax);
  const int smin = meta[4 * b + (which ? 0 : 2)], L = meta[4 * b + (which ? 1 : 3)];
  const int64_t stride = cap_z + cap_y;  // per image: [z bytes | y bytes], zero-initialised by the caller
  const BitSink sink{(uint32_t*)(out + (size_t)b * stride + (which ? cap_z : 0)), (which ? cap_y : cap_z) * 8,
                     nullptr, 0};
  if (L > Lmax || L < 1) {
    if (lane == 0) {
      atomicOr(err, 1);
      lengths[2 * b + which] = 0;
    }
    return;
  }

  // Two-deep software pipeline for the operand gather: symbols are loaded two groups ahead,
  // their table entries one group ahead, so neither dependent load round sits on the serial
  // chain even when L2 latency is several microseconds under a co-running conv kernel.
  auto sym_of = [&](int64_t g) -> float { return g < n ? sym[g] : 0.f; };
  auto pair_at = [&](float v, int64_t g) -> uint32_t {
    if (g >= n) return 0u;
    const int c = (int)(g / HW);
    return pair_of(tab + (size_t)(per_element ? g : (int64_t)c) * Lmax, (int)v - smin, L, err);
  };

  uint32_t low = 0, span = 0, lowm1 = 0xFFFFFFFFu;   // span 0 = 2^32
  uint32_t pending = 0;
  int64_t base_bits = 0;  // bits emitted so far (wave-uniform)
  int overflow = 0;

  uint32_t cur = pair_at(sym_of(lane), lane);
  float sym1 = sym_of(64 + lane);
  for (int64_t base = 0; base < n; base += 64) {
    const float sym2 = sym_of(base + 128 + lane);
    const uint32_t nxt = pair_at(sym1, base + 64 + lane);
    const int cnt = (int)((n - base) < 64 ? (n - base) : 64);
    uint32_t rl = 0, rh = ~0u;   // lanes past cnt: no bit, no E3 run
    // a full group without the top symbol: bounds in two registers (LaneBounds); else the loop
    const uint32_t chv = (cur >> 16) + 1u;
    if (cnt == 64 && !__any(chv == 0x10000u)) chain_group<LaneBounds>(cur << 16, chv << 16, low, lowm1, span, rl, rh);
    else chain_tail(cur, cnt, low, lowm1, span, rl, rh);
    uint32_t nbv, pendv;
    place_group(rl, rh, lane, pending, nbv, pendv);
    base_bits += (int64_t)put_group<false>(sink, base_bits, rl, nbv, pendv, lane, &overflow);
    cur = nxt;
    sym1 = sym2;
  }
  if (lane == 0) lengths[2 * b + which] = put_flush(sink, base_bits, pending, low, &overflow);
  if (__any(overflow) && lane == 0) atomicOr(err, 4);
}

// ---- split encoder: pack -> chain -> place (dsic_range_encode_ws) -----------------------------------
// The same coder in three launches on the coder's stream, so that the only long-running one is a wave small
// enough to share a CU with a persistent conv workgroup (3 x 168 of a SIMD's 512 VGPRs leave 8).
//  pack  (whole chip, short): every symbol's (c_low, c_high-1) pair, error bits 1 and 2.
//  chain (one wave per string, <= 8 VGPRs, no LDS): chain_group on scalar registers, 64 pairs per global load
//        (two groups ahead); per symbol the interval before renormalisation (low1, high1) leaves through two
//        vector stores per 64 symbols; the final low per string.
//  place (two whole-chip launches of short waves, one slice of a string each): per symbol the E1/E2 bits and the
//        E3 run from (low1, high1); summarize writes each slice's carry map and bit count, emit composes the records
//        in front of its slice and places the slice's bits; the string's last slice writes the flush and the length.
// Workspace: pairs, rec_low, rec_high [B (M HWy + N HWz)] uint32, then final low [B (K + 1)], then (8-byte aligned)
// the slice records [B (K ky + kz)] uint2.
__global__ __launch_bounds__(256) void enc_pack_kernel(const float* __restrict__ y, const float* __restrict__ z,
                                                       const int* __restrict__ meta, const uint16_t* __restrict__ tab_y,
                                                       const uint16_t* __restrict__ tab_z, SplitGeom G,
                                                       uint32_t* __restrict__ pairs, int* __restrict__ err) {
  int which, b;
  int64_t n, base;
  G.image(blockIdx.y, which, b, n, base);
  const int HW = which ? G.HWy : G.HWz, Lmax = G.Lmax;
  const bool per_element = which && G.per_element_y;
  const float* sym = which ? y + (size_t)b * n : z + (size_t)b * n;
  const uint16_t* tab = (which ? tab_y + (size_t)b * (per_element ? (size_t)G.M * G.HWy : (size_t)G.M) * Lmax
                               : tab_z + (size_t)b * G.N * Lmax);
  const int smin = meta[4 * b + (which ? 0 : 2)], L = meta[4 * b + (which ? 1 : 3)];
  if (L > Lmax || L < 1) return;   // the place kernels report it
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n; g += (int64_t)gridDim.x * 256) {
    const int c = (int)(g / HW);
    pairs[base + g] = pair_of(tab + (size_t)(per_element ? g : (int64_t)c) * Lmax, (int)sym[g] - smin, L, err);
  }
}

__global__ __launch_bounds__(64) __attribute__((amdgpu_num_vgpr(8))) void enc_chain_kernel(
    const uint32_t* __restrict__ pairs, const int* __restrict__ meta, SplitGeom G, uint32_t* __restrict__ rec_low,
    uint32_t* __restrict__ rec_high, uint32_t* __restrict__ final_low) {
  const int s = blockIdx.x;
  int which, b;
  int64_t n, base;
  G.stream(s, which, b, n, base);
  const int L = meta[4 * b + (which ? 1 : 3)];
  if (L > G.Lmax || L < 1) return;
  // Buffer accesses: the string's base and size in an SGPR resource, one lane-offset VGPR, the group in the scalar
  // offset.  Past the string end (n * 4 bytes, < 2 GiB: checked by the host) loads return 0 and stores are dropped.
  const uint32_t voff = threadIdx.x * 4u;
  const uint32_t nbytes = (uint32_t)n * 4u;
  const __amdgpu_buffer_rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc((void*)(pairs + base), 0, nbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rlo = __builtin_amdgcn_make_buffer_rsrc((void*)(rec_low + base), 0, nbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rhi = __builtin_amdgcn_make_buffer_rsrc((void*)(rec_high + base), 0, nbytes, 0x00020000);
  auto ld = [&](uint32_t g) -> uint32_t { return __builtin_amdgcn_raw_buffer_load_b32(rp, voff, g * 4u, 0); };
  uint32_t low = 0, span = 0, lowm1 = 0xFFFFFFFFu;   // span 0 = 2^32
  uint32_t cur = ld(0), n1 = ld(64);
  const uint32_t nfull = (uint32_t)n & ~63u;   // 32-bit scalar loop counter (n < 2^29)
  uint32_t g = 0;
  for (; g < nfull; g += 64) {
    const uint32_t n2 = ld(g + 128);
    uint32_t rl = 0, rh = 0;
    chain_group<PackedPairs>(cur, 0u, low, lowm1, span, rl, rh);
    __builtin_amdgcn_raw_buffer_store_b32(rl, rlo, voff, g * 4u, 0);
    __builtin_amdgcn_raw_buffer_store_b32(rh, rhi, voff, g * 4u, 0);
    cur = n1;
    n1 = n2;
  }
  const int cnt = (int)((uint32_t)n - g);   // 0..63 symbols left
  if (cnt > 0) {
    uint32_t rl = 0, rh = 0;
    chain_tail(cur, cnt, low, lowm1, span, rl, rh);
    __builtin_amdgcn_raw_buffer_store_b32(rl, rlo, voff, g * 4u, 0);   // lanes >= cnt: out of range
    __builtin_amdgcn_raw_buffer_store_b32(rh, rhi, voff, g * 4u, 0);
  }
  if (threadIdx.x == 0) final_low[s] = low;
}

// ---- place: summarize -> emit ----------------------------------------------------------------------------------
// A string is cut into slices of `gs` groups of 64 symbols (place_slicing); a wave walks one slice, and a 256-thread
// workgroup holds four such waves that never wait for each other (no barrier; emit gives each wave an LDS window of
// its own), so every workgroup lives for a few microseconds and none keeps a CU from the next conv launch for long.
//  summarize: the slice's carry map of the pending count, c -> (a ? c : 0) + t (a = 1: no symbol of the slice emits
//             a bit), and its bit count with carry-in 0; one record per slice.
//  emit:      the records of the slices in front of it give the slice's carry-in and its bit offset; then put_group
//             per group through the wave's LDS window, and the string's last slice writes the flush and the length.
//             Every record is written by the first launch before the second reads one: no wave waits for another,
//             and the workspace may hold anything when the call starts.
// Composition: (a1, t1) then (a2, t2) = (a1 & a2, (a2 ? t1 : 0) + t2).  A record is (t, len | head << 31), head = !a.
#ifndef PLACE_WAVES
#define PLACE_WAVES 4
#endif
constexpr int PLACE_CHUNK = 8;   // groups whose records one wave loads at once (a slice is >= 8 groups)

// records of the groups c0, c0 + 64, ... (PLACE_CHUNK of them) in one round of loads; past j1: (0, ~0)
__device__ __forceinline__ void place_load(const uint32_t* __restrict__ rlo, const uint32_t* __restrict__ rhi,
                                           int64_t c0, int64_t j1, int lane, uint32_t (&lo)[PLACE_CHUNK],
                                           uint32_t (&hi)[PLACE_CHUNK]) {
#pragma unroll
  for (int i = 0; i < PLACE_CHUNK; ++i) {
    const int64_t j = c0 + i * 64 + lane;
    lo[i] = j < j1 ? rlo[j] : 0u;
    hi[i] = j < j1 ? rhi[j] : ~0u;
  }
}

__global__ __launch_bounds__(64 * PLACE_WAVES) void enc_place_sum_kernel(const int* __restrict__ meta, SplitGeom G,
                                                                         const uint32_t* __restrict__ rec_low,
                                                                         const uint32_t* __restrict__ rec_high,
                                                                         uint2* __restrict__ slices) {
  const int lane = threadIdx.x & 63;
  const int q = __builtin_amdgcn_readfirstlane(blockIdx.x * PLACE_WAVES + (threadIdx.x >> 6));
  if (q >= G.nslices()) return;
  int s, k, ks, gs, q0;
  G.slice(q, s, k, ks, gs, q0);
  int which, b;
  int64_t n, base;
  G.stream(s, which, b, n, base);
  const int L = meta[4 * b + (which ? 1 : 3)];
  if (L > G.Lmax || L < 1) return;   // emit reports it; the chain wrote no records
  const uint32_t* rlo = rec_low + base;
  const uint32_t* rhi = rec_high + base;
  const int64_t j0 = (int64_t)k * gs * 64;
  const int64_t j1 = j0 + (int64_t)gs * 64 < n ? j0 + (int64_t)gs * 64 : n;
  uint32_t pending = 0, bits = 0, head = 0;   // a slice emits < 2^27 bits besides its carry-in
  for (int64_t c0 = j0; c0 < j1; c0 += PLACE_CHUNK * 64) {
    uint32_t lo[PLACE_CHUNK], hi[PLACE_CHUNK];
    place_load(rlo, rhi, c0, j1, lane, lo, hi);
#pragma unroll
    for (int i = 0; i < PLACE_CHUNK; ++i) {
      if (c0 + i * 64 >= j1) break;
      uint32_t nbv, pendv;
      place_group(lo[i], hi[i], lane, pending, nbv, pendv);
      head |= __ballot(nbv > 0) ? 1u : 0u;
      uint32_t len = nbv + pendv;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) len += __shfl_xor(len, o, 64);
      bits += len;
    }
  }
  if (lane == 0) slices[q] = make_uint2(pending, bits | (head << 31));
}

__global__ __launch_bounds__(64 * PLACE_WAVES) void enc_place_emit_kernel(
    const int* __restrict__ meta, SplitGeom G, const uint32_t* __restrict__ rec_low,
    const uint32_t* __restrict__ rec_high, const uint2* __restrict__ slices, const uint32_t* __restrict__ final_low,
    uint8_t* __restrict__ out, int64_t cap_y, int64_t cap_z, int* __restrict__ lengths, int* __restrict__ err) {
  // cap_y: the capacity of one y segment; out [B][cap_z + K cap_y], lengths [B][1 + K] = {z, segment 0 .. K - 1}
  const int lane = threadIdx.x & 63;
  const int q = __builtin_amdgcn_readfirstlane(blockIdx.x * PLACE_WAVES + (threadIdx.x >> 6));
  if (q >= G.nslices()) return;
  int s, k, ks, gs, q0;
  G.slice(q, s, k, ks, gs, q0);
  int which, b;
  int64_t n, base;
  G.stream(s, which, b, n, base);
  const int seg = which ? s & (G.K - 1) : 0;
  int* const length = lengths + (size_t)(1 + G.K) * b + (which ? 1 + seg : 0);
  const int L = meta[4 * b + (which ? 1 : 3)];
  if (L > G.Lmax || L < 1) {
    if (k == 0 && lane == 0) {
      atomicOr(err, 1);
      *length = 0;
    }
    return;
  }
  const uint32_t* rlo = rec_low + base;
  const uint32_t* rhi = rec_high + base;
  const int64_t j0 = (int64_t)k * gs * 64;
  const int64_t j1 = j0 + (int64_t)gs * 64 < n ? j0 + (int64_t)gs * 64 : n;
  uint32_t lo[PLACE_CHUNK], hi[PLACE_CHUNK];   // the first chunk's records travel while the slices are composed
  place_load(rlo, rhi, j0, j1, lane, lo, hi);
  // carry-in and bit offset of slice k: the maps of slices 0..k-1 composed, 64 records per step
  uint32_t pending = 0;
  uint64_t off = 0;
  for (int i0 = 0; i0 < k; i0 += 64) {
    const int i = i0 + lane;
    uint32_t a = 1u, t = 0u, len = 0u;   // past k: the identity map, no bits
    if (i < k) {
      const uint2 r = slices[q0 + i];
      t = r.x;
      len = r.y & 0x7FFFFFFFu;
      a = (r.y >> 31) ? 0u : 1u;
    }
    uint32_t A = a, Tm = t;   // slices i0..i composed
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t pa = __shfl_up(A, o, 64), pt = __shfl_up(Tm, o, 64);
      if (lane >= o) {   // (pa, pt) then (A, Tm)
        Tm = (A ? pt : 0u) + Tm;
        A = pa & A;
      }
    }
    uint32_t Ae = __shfl_up(A, 1, 64), Te = __shfl_up(Tm, 1, 64);
    if (lane == 0) {
      Ae = 1u;
      Te = 0u;
    }
    const uint32_t cin = (Ae ? pending : 0u) + Te;   // owed at the start of slice i
    uint64_t bits = (uint64_t)len + (a ? 0u : cin);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bits += __shfl_xor(bits, o, 64);
    off += bits;
    const uint32_t A63 = __builtin_amdgcn_readlane(A, 63), T63 = __builtin_amdgcn_readlane(Tm, 63);
    pending = (A63 ? pending : 0u) + T63;
  }

  const int64_t stride = cap_z + (int64_t)G.K * cap_y;
  uint32_t* dst32 = (uint32_t*)(out + (size_t)b * stride + (which ? cap_z + (int64_t)seg * cap_y : 0));
  int overflow = 0;
  // the slice's bits are ORed into an LDS window first: one global atomic per output word instead of one per piece
  __shared__ uint32_t win_all[PLACE_WAVES][PLACE_WIN];
  uint32_t* win = win_all[threadIdx.x >> 6];
#pragma unroll
  for (int i = lane; i < PLACE_WIN; i += 64) win[i] = 0u;
  const BitSink sink{dst32, (which ? cap_y : cap_z) * 8, win, (int64_t)(off >> 5)};
  for (int64_t c0 = j0; c0 < j1; c0 += PLACE_CHUNK * 64) {
    if (c0 != j0) place_load(rlo, rhi, c0, j1, lane, lo, hi);
#pragma unroll
    for (int i = 0; i < PLACE_CHUNK; ++i) {
      if (c0 + i * 64 >= j1) break;
      uint32_t nbv, pendv;
      place_group(lo[i], hi[i], lane, pending, nbv, pendv);
      off += put_group<true>(sink, (int64_t)off, lo[i], nbv, pendv, lane, &overflow);
    }
  }
  // the window's words that received bits (all inside the capacity: put_bits checked each piece)
  const int64_t wend = (int64_t)((off + 31) >> 5) - sink.wbase;
  const int nw = wend < PLACE_WIN ? (int)wend : PLACE_WIN;
  __builtin_amdgcn_s_waitcnt(0xc07f);
  __builtin_amdgcn_wave_barrier();
  for (int i = lane; i < nw; i += 64) {
    const uint32_t v = win[i];
    if (v) atomicOr(dst32 + sink.wbase + i, v);
  }
  if (k == ks - 1 && lane == 0) *length = put_flush(sink, (int64_t)off, pending, final_low[s], &overflow);
  if (__any(overflow) && lane == 0) atomicOr(err, 4);
}

// Range decoder, one wave per stream (torchac decode_float_cdf, call sites :96,116).
//
// The reference computes count = ((value-low+1)*2^16 - 1) / span and searches the table for
// c[s] <= count < c[s+1].  For integers that is exactly  floor(span*c[s] / 2^16) <= value-low
// (no division), and the predicate is monotone in s, so all 64 lanes test one table entry each
// and a ballot + popcount gives s.  The interval update and renormalisation mirror the
// encoder (bulk shifts by clz); `value` takes the same shifts with fresh stream bits, and the
// m-step E3 correction  v <- 2(v - 2^30) + bit  collapses to flipping the top bit.  Stream
// bytes are fetched 256 at a time by the wave (zero past the end, like torchac's reader).
//
// SEG (dsic_range_decode_seg): one wave per (string, segment).  The 2^lk segments of string b lie back to back from
// in + b * stride, segment k at byte sum_{j<k} seg_lengths[b][j] (any alignment: the window's big-endian words are
// funnelled from aligned dwords), and decode C / 2^lk channels each with the string's one support: table rows, symbols
// and output from k C / 2^lk.  A segment's start and length are cut to what is left of lengths[b], so a forged
// length reads zeros, never past the string.
template <bool SEG>
__global__ __launch_bounds__(256) void range_decode_kernel(const uint8_t* __restrict__ in,
                                                           int64_t stride,
                                                           const int* __restrict__ lengths, int lstride,
                                                           int loff, const int* __restrict__ meta,
                                                           int meta_off,
                                                           const uint16_t* __restrict__ tables, int Lmax,
                                                           int C, int HW, float* __restrict__ out,
                                                           int* __restrict__ err, int B,
                                                           int per_element, const int* __restrict__ seg_lengths,
                                                           int lk) {
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
  const int b = SEG ? wid >> lk : wid;
  if (b >= B) return;
  const int smin = meta[4 * b + meta_off], L = meta[4 * b + meta_off + 1];
  if (L > Lmax || L < 1) {
    if (lane == 0 && (!SEG || (wid & ((1 << lk) - 1)) == 0)) atomicOr(err, 1);
    return;
  }
  const uint16_t* gt = tables + (size_t)b * (per_element ? (size_t)C * HW : (size_t)C) * Lmax;
  const uint32_t* src32 = (const uint32_t*)(in + (size_t)b * stride);  // stride is a multiple of 4
  int nbytes = lengths[b * lstride + loff];
  float* dst = out + (size_t)b * C * HW;
  int sh8 = 0, ndw_all = 0;   // SEG: 8 x the segment's byte offset inside its first dword; dwords of the whole string
  if (SEG) {
    const int k = wid & ((1 << lk) - 1);
    const uint32_t total = nbytes < 0 ? 0u : (uint32_t)nbytes;
    uint32_t soff = 0;
    for (int j = 0; j < k; ++j) {
      const int lj = seg_lengths[((size_t)b << lk) + j];
      const uint32_t left = total - soff;
      soff += lj < 0 ? 0u : ((uint32_t)lj < left ? (uint32_t)lj : left);
    }
    const int lkk = seg_lengths[((size_t)b << lk) + k];
    const uint32_t left = total - soff;
    nbytes = (int)(lkk < 0 ? 0u : ((uint32_t)lkk < left ? (uint32_t)lkk : left));
    ndw_all = (int)((total + 3u) >> 2);
    src32 += soff >> 2;
    ndw_all -= (int)(soff >> 2);
    sh8 = (int)(soff & 3u) * 8;
    C >>= lk;
    gt += (size_t)k * (per_element ? (size_t)C * HW : (size_t)C) * Lmax;
    dst += (size_t)k * C * HW;
  }
  const int ndw = (nbytes + 3) >> 2;
  const int64_t n = (int64_t)C * HW;

  // 64-dword window of the stream, big-endian words, bytes >= nbytes read as zero
  auto load_window = [&](int w0) -> uint32_t {
    const int k = w0 + lane;
    uint32_t v = 0;
    if (k < ndw) {
      v = __builtin_bswap32(src32[k]);
      if (SEG && sh8) {   // word k of the segment straddles dwords k and k + 1 of the string
        const uint32_t nx = k + 1 < ndw_all ? __builtin_bswap32(src32[k + 1]) : 0u;
        v = (v << sh8) | (nx >> (32 - sh8));
      }
      const int valid = nbytes - 4 * k;  // 1..4 valid bytes in the last dword
      if (valid < 4) v &= 0xFFFFFFFFu << (8 * (4 - valid));
    }
    return v;
  };
  uint32_t win = load_window(0), win_next = load_window(64);
  int wi = 0;  // next dword to feed into the bit buffer
  auto next_dword = [&]() -> uint32_t {
    const uint32_t d = __builtin_amdgcn_readlane(win, wi & 63);
    ++wi;
    if ((wi & 63) == 0) {
      win = win_next;
      win_next = load_window(wi + 64);
    }
    return d;
  };
  uint64_t bitbuf = ((uint64_t)next_dword() << 32);
  bitbuf |= (uint64_t)next_dword();
  int avail = 64;
  auto take = [&](int k) -> uint32_t {  // next k (0..31) bits of the stream
    const uint32_t v = k ? (uint32_t)(bitbuf >> (64 - k)) : 0u;
    bitbuf <<= k;
    avail -= k;
    if (avail <= 32) {
      bitbuf |= (uint64_t)next_dword() << (32 - avail);
      avail += 32;
    }
    return v;
  };

  uint32_t low = 0, high = 0xFFFFFFFFu;
  uint32_t value = take(16);
  value = (value << 16) | take(16);

  const int nseg = (L + 63) >> 6;  // table entries per row, 64 per register
  if (nseg == 1 && !per_element) {
    // ---- fast path: the whole table row in one register, rows per channel ---------------------------------
    // The encoder's IntervalStep, shorter chain (round 3: 371 -> 188 ns per symbol at the bench shape): the state is
    // (low, span, lowm1) and the lanes hold c << 16, so floor(span c / 2^16) is ONE v_mul_hi_u32 per lane for the
    // search, and the decoded symbol's bounds are two of those products (the general path multiplies in 64 bits);
    // c_high = 65536 (last symbol) is hi_add = span.  The two renormalisation shifts
    // (E1/E2 by nb, E3 by m) are applied together and their stream bits taken together when nb + m < 32.  Decoded
    // symbols collect in a register (lane g & 63) and leave as one coalesced 256-byte store per 64 symbols
    // instead of a 4-byte store per symbol.  (Stream bits cut out of two window lanes by absolute bit position,
    // without the 64-bit buffer: +24 ns per symbol - two more v_readlane with an SGPR lane select.)
    const uint64_t valid = L >= 64 ? ~0ull : ((1ull << L) - 1ull);
    auto load_row16 = [&](int64_t rw) -> uint32_t {
      return lane < L ? ((uint32_t)gt[(size_t)rw * Lmax + lane]) << 16 : 0u;
    };
    uint32_t ck16 = load_row16(0), ck16_next = C > 1 ? load_row16(1) : 0u;
    uint32_t span = 0u, lowm1 = 0xFFFFFFFFu;   // low = 0
    int outv = 0;   // symbols (integers) of the current group of 64, one per lane
    int in_r = 0;
    int64_t rw = 0;
    for (int64_t g = 0; g < n; ++g) {
      const uint32_t d = value - low;
      const uint32_t bound = span ? __umulhi(span, ck16) : ck16;
      const int hits = __popcll(__ballot(bound <= d) & valid);   // >= 1: c[0] = 0
      // the decoded symbol's own bounds are two of the products the lanes just formed
      const uint32_t lo_add = __builtin_amdgcn_readlane(bound, hits - 1);
      const uint32_t hi_mul = __builtin_amdgcn_readlane(bound, hits & 63);
      const uint32_t hi_add = hits == L ? span : hi_mul;          // c_high = 65536: floor(span 2^16 / 2^16)
      {  // symbol g -> lane g & 63 of outv
        const int sv = hits - 1 + smin;
        const int ln = (int)(g & 63);
        asm volatile("s_mov_b32 m0, %2\n\ts_nop 3\n\tv_writelane_b32 %0, %1, m0" : "+v"(outv) : "s"(sv), "s"(ln));
        if (ln == 63) dst[g - 63 + lane] = (float)outv;
      }
      const IntervalStep st{low + lo_add, lowm1 + hi_add, hi_add - lo_add};
      int nb, m;
      st.shifts(nb, m);
      const int sh = nb + m;
      if (__builtin_expect(sh < 32, 1)) {
        span = st.span(sh);
        low = st.low(sh);
        const uint32_t v2 = sh ? ((value << sh) | take(sh)) : value;
        value = m ? (v2 ^ 0x80000000u) : v2;
      } else {  // a long E3 run: the two shifts one after the other, as the general path
        uint32_t lo2 = st.low1 << nb, hi2 = (st.high1 << nb) | ((1u << nb) - 1u);
        value = nb ? ((value << nb) | take(nb)) : value;
        lo2 = (lo2 << m) & 0x7FFFFFFFu;
        hi2 = (hi2 << m) | 0x80000000u | ((1u << m) - 1u);
        value = ((value << m) | take(m)) ^ 0x80000000u;
        low = lo2;
        span = hi2 - lo2 + 1u;
      }
      lowm1 = low - 1u;
      if (++in_r == HW) {
        in_r = 0;
        rw += 1;
        ck16 = ck16_next;
        if (rw + 1 < C) ck16_next = load_row16(rw + 1);
      }
    }
    if (n & 63) {
      const int64_t g0 = n & ~(int64_t)63;
      if (lane < (int)(n & 63)) dst[g0 + lane] = (float)outv;
    }
    return;
  }
  // ---- general path: rows wider than 64 entries, or a row per symbol -------------------------------------------
  // Kept apart from IntervalStep on purpose: a step searches up to Lmax / 64 registers of table entries, so its bounds
  // are plain 17-bit values (c_high up to 65536) multiplied in 64 bits against (low, high), not the c << 16 operands
  // of the one-register paths; it shares no operand form with them.
  // Table row of the current symbol: per channel (row changes every HW symbols) or per element
  // (spatial_params: a row per symbol).  Segment 0 of the NEXT row is prefetched while the
  // current symbol is decoded, so the row load never sits on the serial chain.
  // row index of symbol g, tracked incrementally (no 64-bit division on the serial chain)
  int64_t row = 0;   // row of the current symbol
  int in_row = 0;    // symbols already decoded from the current per-channel row
  auto load_seg = [&](const uint16_t* t, int seg) -> uint32_t {
    const int k = seg * 64 + lane;
    return k < L ? (uint32_t)t[k] : 0x10000u;  // entries past L act as c[L] = 65536
  };
  uint32_t ck0 = load_seg(gt, 0);
  for (int64_t g = 0; g < n; ++g) {
    {
      const uint16_t* t = gt + (size_t)row * Lmax;
      const bool new_row = per_element || in_row + 1 == HW;
      uint32_t ck0_next = ck0;
      if (new_row && g + 1 < n) ck0_next = load_seg(gt + (size_t)(row + 1) * Lmax, 0);
      const uint32_t d = value - low;
      const uint32_t r = high - low;  // span - 1
      // s = (number of k in [0,L) with floor(span*c[k]/2^16) <= d) - 1
      int cnt = 0;
      uint32_t c_low = 0, c_high = 0x10000u, carry_low = 0;
      bool carry = false;  // the previous 64-entry segment was entirely <= count
      for (int seg = 0; seg < nseg; ++seg) {
        const int k = seg * 64 + lane;
        const uint32_t ck = seg == 0 ? ck0 : load_seg(t, seg);
        const uint32_t bound = (uint32_t)(((uint64_t)r * ck + ck) >> 16);
        const int hits = __popcll(__ballot(k < L && bound <= d));
        if (hits == 0) {  // only after a full segment (c[0] = 0 always hits)
          if (carry) {
            c_low = carry_low;
            c_high = __builtin_amdgcn_readlane(ck, 0);
          }
          break;
        }
        cnt += hits;
        if (hits < 64) {
          c_low = __builtin_amdgcn_readlane(ck, hits - 1);
          c_high = __builtin_amdgcn_readlane(ck, hits);
          break;
        }
        carry = true;
        carry_low = __builtin_amdgcn_readlane(ck, 63);
        if (seg + 1 == nseg) {
          c_low = carry_low;
          c_high = 0x10000u;
        }
      }
      ck0 = ck0_next;
      if (new_row) {
        row += 1;
        in_row = 0;
      } else {
        in_row += 1;
      }
      const int sidx = cnt - 1;
      if (lane == 0) dst[g] = (float)(sidx + smin);
      // interval update + renormalisation, E1/E2 then E3, on (low, high)
      const uint32_t hi_add = (uint32_t)(((uint64_t)r * c_high + c_high) >> 16);
      const uint32_t lo_add = (uint32_t)(((uint64_t)r * c_low + c_low) >> 16);
      high = (low - 1u) + hi_add;
      low = low + lo_add;
      const int nb = __builtin_clz(low ^ high);
      low <<= nb;
      high = (high << nb) | ((1u << nb) - 1u);
      value = nb ? ((value << nb) | take(nb)) : value;
      const uint32_t e3 = (low << 1) & ~(high << 1);
      const int m = __builtin_clz(~e3);
      low = (low << m) & 0x7FFFFFFFu;
      high = (high << m) | 0x80000000u | ((1u << m) - 1u);
      value = m ? (((value << m) | take(m)) ^ 0x80000000u) : value;
    }
  }
}

}  // namespace dsic

using namespace dsic;

// ENC_ABL (diagnostic builds only, wrong results): skip the launches of 1 support, 2 tables, 4 pack, 8 place (both
// launches), 16 chain; error bits then go to a sink of their own, so that a run is not stopped by them.
#ifndef ENC_ABL
#define ENC_ABL 0
#endif
#if ENC_ABL
__device__ int enc_abl_err_sink;
static int* abl_err(int* err) {
  void* p = nullptr;
  return hipGetSymbolAddress(&p, HIP_SYMBOL(enc_abl_err_sink)) == hipSuccess ? (int*)p : err;
}
#else
static int* abl_err(int* err) { return err; }
#endif


extern "C" int dsic_latent_support(const float* y_nchw, const float* z_nchw, int* meta, int B,
                                   int64_t n_y, int64_t n_z, int tail, void* stream) {
  DSIC_REQUIRE(y_nchw && z_nchw && meta, "latent_support: null pointer");
  DSIC_REQUIRE(B > 0 && n_y > 0 && n_z > 0 && tail >= 0, "latent_support: bad argument");
  if (ENC_ABL & 1) return DSIC_OK;
  hipLaunchKernelGGL(support_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, y_nchw, z_nchw, meta,
                     n_y, n_z, tail);
  return check_launch("latent_support");
}

// C counts table rows per image: channels, or channels*HW in per-element mode (sigma/nu then
// hold one value per latent element, NCHW order = symbol order).
static int tables_launch(bool student, const float* sigma, const float* nu, int per_image,
                         const int* meta, int meta_off, uint16_t* tables, int B, int C, int Lmax,
                         int* err, hipStream_t st) {
  DSIC_REQUIRE(sigma && meta && tables && err && (!student || nu), "cdf_tables: null pointer");
  DSIC_REQUIRE(B > 0 && C > 0 && Lmax >= 1 && Lmax <= 1000, "cdf_tables: Lmax=%d must be in [1,1000]", Lmax);
  if (ENC_ABL & 2) return DSIC_OK;
  err = abl_err(err);
  const int ntables = B * C;
  const size_t shm = (size_t)4 * (2 * Lmax + 1) * sizeof(float);
  const int sb = per_image ? C : 0;
  if (student) {
    hipLaunchKernelGGL(tables_kernel<true>, dim3(ceil_div(ntables, 4)), dim3(256), shm, st, sigma, nu, sb,
                       meta, meta_off, tables, C, Lmax, ntables, err);
  } else if (sb == 0) {
    const int rowmax = 4 * Lmax;
    hipLaunchKernelGGL(gauss_tables_kernel, dim3(C, ceil_div(B, ZT_IMGS)), dim3(256), shm + rowmax * sizeof(float),
                       st, sigma, meta, tables, B, C, Lmax, rowmax, err);
  } else {
    hipLaunchKernelGGL(tables_kernel<false>, dim3(ceil_div(ntables, 4)), dim3(256), shm, st, sigma, nu, sb,
                       meta, meta_off, tables, C, Lmax, ntables, err);
  }
  return check_launch("cdf_tables");
}

extern "C" int dsic_cdf_tables_gauss(const float* sigma_z, const int* meta, uint16_t* tables, int B,
                                     int N, int Lmax, int* err, void* stream) {
  return tables_launch(false, sigma_z, nullptr, 0, meta, 2, tables, B, N, Lmax, err, (hipStream_t)stream);
}

extern "C" int dsic_cdf_tables_student(const float* sigma, const float* nu, const int* meta,
                                       uint16_t* tables, int B, int rows, int Lmax, int* err,
                                       void* stream) {
  return tables_launch(true, sigma, nu, 1, meta, 0, tables, B, rows, Lmax, err, (hipStream_t)stream);
}

extern "C" int dsic_range_encode(const float* y_nchw, const float* z_nchw, const int* meta,
                                 const uint16_t* tab_y, const uint16_t* tab_z, int Lmax, int B, int M,
                                 int HWy, int N, int HWz, uint8_t* out, int64_t cap_y, int64_t cap_z,
                                 int* lengths, int* err, int streams_per_wg, int per_element_y,
                                 void* stream) {
  DSIC_REQUIRE(y_nchw && z_nchw && meta && tab_y && tab_z && out && lengths && err,
               "range_encode: null pointer");
  DSIC_REQUIRE(B > 0 && M > 0 && N > 0 && HWy > 0 && HWz > 0, "range_encode: empty latent");
  DSIC_REQUIRE(cap_y % 4 == 0 && cap_z % 4 == 0 && cap_y >= 8 && cap_z >= 8,
               "range_encode: capacities must be multiples of 4 and >= 8");
  DSIC_REQUIRE(streams_per_wg >= 1 && streams_per_wg <= 16, "range_encode: streams_per_wg must be in [1,16]");
  hipLaunchKernelGGL(range_encode_kernel, dim3(ceil_div(2 * B, streams_per_wg)), dim3(64 * streams_per_wg), 0,
                     (hipStream_t)stream,
                     y_nchw, z_nchw, meta, tab_y, tab_z, Lmax, M, HWy, N, HWz, out, cap_y, cap_z, lengths,
                     err, 2 * B, per_element_y ? 1 : 0);
  return check_launch("range_encode");
}

// Split encoder (pack -> chain -> place): the same bytes, lengths and error bits as dsic_range_encode.
static int64_t place_records(int B, int64_t ns, int64_t nz, int segs) {
  int gy, ky, gz, kz;
  place_slicing(ns, gy, ky);
  place_slicing(nz, gz, kz);
  return (int64_t)B * ((int64_t)segs * ky + kz);
}

// y segments per image: a power of two up to 16 that divides the channels
static bool segs_ok(int segs, int M) {
  return (segs == 1 || segs == 2 || segs == 4 || segs == 8 || segs == 16) && M % segs == 0;
}

extern "C" int64_t dsic_range_encode_seg_workspace_size(int B, int M, int HWy, int N, int HWz, int segs) {
  if (B <= 0 || M <= 0 || HWy <= 0 || N <= 0 || HWz <= 0 || !segs_ok(segs, M)) return -1;
  const int64_t ny = (int64_t)M * HWy, nz = (int64_t)N * HWz;
  const int64_t total = (int64_t)B * (ny + nz);
  // pairs, rec_low, rec_high: 4 B per symbol each; final low per string; 8-byte slice records (+ alignment)
  return 12 * total + 4 * (int64_t)B * (segs + 1) + 8 + 8 * place_records(B, ny / segs, nz, segs);
}

extern "C" int64_t dsic_range_encode_workspace_size(int B, int M, int HWy, int N, int HWz) {
  return dsic_range_encode_seg_workspace_size(B, M, HWy, N, HWz, 1);
}

// cap_y: the capacity of one y segment (of the y string for segs = 1)
extern "C" int dsic_range_encode_seg_ws(const float* y_nchw, const float* z_nchw, const int* meta,
                                        const uint16_t* tab_y, const uint16_t* tab_z, int Lmax, int B, int M,
                                        int HWy, int N, int HWz, uint8_t* out, int64_t cap_seg, int64_t cap_z,
                                        int* lengths, int* err, int per_element_y, int segs, void* workspace,
                                        int64_t workspace_bytes, void* stream) {
  const int64_t cap_y = cap_seg;
  DSIC_REQUIRE(y_nchw && z_nchw && meta && tab_y && tab_z && out && lengths && err && workspace,
               "range_encode_ws: null pointer");
  DSIC_REQUIRE(B > 0 && M > 0 && N > 0 && HWy > 0 && HWz > 0, "range_encode_ws: empty latent");
  DSIC_REQUIRE(segs_ok(segs, M), "range_encode_ws: segments=%d must be 1, 2, 4, 8 or 16 and divide M=%d", segs, M);
  DSIC_REQUIRE(cap_y % 4 == 0 && cap_z % 4 == 0 && cap_y >= 8 && cap_z >= 8,
               "range_encode_ws: capacities must be multiples of 4 and >= 8");
  DSIC_REQUIRE(workspace_bytes >= dsic_range_encode_seg_workspace_size(B, M, HWy, N, HWz, segs),
               "range_encode_ws: workspace too small");
  err = abl_err(err);
  SplitGeom G;
  G.B = B; G.M = M; G.HWy = HWy; G.N = N; G.HWz = HWz; G.Lmax = Lmax; G.per_element_y = per_element_y ? 1 : 0;
  G.K = segs;
  G.lk = __builtin_ctz((unsigned)segs);
  G.ny = (int64_t)M * HWy;
  G.nz = (int64_t)N * HWz;
  G.ns = G.ny / segs;
  DSIC_REQUIRE(G.ny < ((int64_t)1 << 29) && G.nz < ((int64_t)1 << 29), "range_encode_ws: string too long");
  place_slicing(G.ns, G.gy, G.ky);
  place_slicing(G.nz, G.gz, G.kz);
  const int64_t nstrings = (int64_t)B * (segs + 1);
  const int64_t nslices = (int64_t)B * ((int64_t)segs * G.ky + G.kz);
  DSIC_REQUIRE(nslices < ((int64_t)1 << 30) && nstrings < ((int64_t)1 << 30), "range_encode_ws: too many strings");
  const int64_t total = (int64_t)B * (G.ny + G.nz);
  uint32_t* pairs = (uint32_t*)workspace;
  uint32_t* rec_low = pairs + total;
  uint32_t* rec_high = rec_low + total;
  uint32_t* final_low = rec_high + total;
  uint2* slices = (uint2*)(((uintptr_t)(final_low + nstrings) + 7) & ~(uintptr_t)7);
  hipStream_t st = (hipStream_t)stream;
  int rc = DSIC_OK;
  if (!(ENC_ABL & 4)) {
    const int64_t nmax = G.ny > G.nz ? G.ny : G.nz;
    const int gx = (int)((nmax + 255) / 256 < 256 ? (nmax + 255) / 256 : 256);
    hipLaunchKernelGGL(enc_pack_kernel, dim3(gx, 2 * B), dim3(256), 0, st, y_nchw, z_nchw, meta, tab_y, tab_z, G,
                       pairs, err);
    rc = check_launch("range_encode_ws: pack");
    if (rc != DSIC_OK) return rc;
  }
  if (!(ENC_ABL & 16)) {
    // the y strings (the long ones) first; one wave per workgroup
    hipLaunchKernelGGL(enc_chain_kernel, dim3((unsigned)nstrings), dim3(64), 0, st, pairs, meta, G, rec_low, rec_high, final_low);
    rc = check_launch("range_encode_ws: chain");
    if (rc != DSIC_OK) return rc;
  }
  if (!(ENC_ABL & 8)) {
    const int nwg = (int)((nslices + PLACE_WAVES - 1) / PLACE_WAVES);
    hipLaunchKernelGGL(enc_place_sum_kernel, dim3(nwg), dim3(64 * PLACE_WAVES), 0, st, meta, G, rec_low, rec_high,
                       slices);
    rc = check_launch("range_encode_ws: place summarize");
    if (rc != DSIC_OK) return rc;
    hipLaunchKernelGGL(enc_place_emit_kernel, dim3(nwg), dim3(64 * PLACE_WAVES), 0, st, meta, G, rec_low, rec_high,
                       slices, final_low, out, cap_y, cap_z, lengths, err);
    rc = check_launch("range_encode_ws: place emit");
  }
  return rc;
}

extern "C" int dsic_range_encode_ws(const float* y_nchw, const float* z_nchw, const int* meta,
                                    const uint16_t* tab_y, const uint16_t* tab_z, int Lmax, int B, int M,
                                    int HWy, int N, int HWz, uint8_t* out, int64_t cap_y, int64_t cap_z,
                                    int* lengths, int* err, int per_element_y, void* workspace,
                                    int64_t workspace_bytes, void* stream) {
  return dsic_range_encode_seg_ws(y_nchw, z_nchw, meta, tab_y, tab_z, Lmax, B, M, HWy, N, HWz, out, cap_y, cap_z,
                                  lengths, err, per_element_y, 1, workspace, workspace_bytes, stream);
}

extern "C" int dsic_range_decode(const uint8_t* in, int64_t stride, const int* lengths, int lstride,
                                 int loff, const int* meta, int meta_off, const uint16_t* tables,
                                 int Lmax, int B, int C, int HW, int per_element, float* out_nchw,
                                 int* err, void* stream) {
  DSIC_REQUIRE(in && lengths && meta && tables && out_nchw && err, "range_decode: null pointer");
  DSIC_REQUIRE(B > 0 && C > 0 && HW > 0 && Lmax >= 1, "range_decode: bad argument");
  DSIC_REQUIRE(meta_off == 0 || meta_off == 2, "range_decode: meta_off must be 0 (y) or 2 (z)");
  DSIC_REQUIRE(stride % 4 == 0, "range_decode: stride must be a multiple of 4");
  // one wave per workgroup: a decoder wave has its CU's scalar unit to itself (as the encoder's waves)
  hipLaunchKernelGGL(range_decode_kernel<false>, dim3(B), dim3(64), 0, (hipStream_t)stream, in, stride,
                     lengths, lstride, loff, meta, meta_off, tables, Lmax, C, HW, out_nchw, err, B, per_element ? 1 : 0,
                     (const int*)nullptr, 0);
  return check_launch("range_decode");
}

extern "C" int dsic_range_decode_seg(const uint8_t* in, int64_t stride, const int* lengths, int lstride, int loff,
                                     const int* seg_lengths, int segs, const int* meta, int meta_off,
                                     const uint16_t* tables, int Lmax, int B, int C, int HW, int per_element,
                                     float* out_nchw, int* err, void* stream) {
  DSIC_REQUIRE(in && lengths && seg_lengths && meta && tables && out_nchw && err, "range_decode_seg: null pointer");
  DSIC_REQUIRE(B > 0 && C > 0 && HW > 0 && Lmax >= 1, "range_decode_seg: bad argument");
  DSIC_REQUIRE(segs_ok(segs, C), "range_decode_seg: segments=%d must be 1, 2, 4, 8 or 16 and divide C=%d", segs, C);
  DSIC_REQUIRE((int64_t)B * segs < ((int64_t)1 << 30), "range_decode_seg: too many strings");
  DSIC_REQUIRE(meta_off == 0 || meta_off == 2, "range_decode_seg: meta_off must be 0 (y) or 2 (z)");
  DSIC_REQUIRE(stride % 4 == 0 && ((uintptr_t)in & 3) == 0, "range_decode_seg: in and stride must be multiples of 4");
  // one wave per workgroup and per (string, segment)
  hipLaunchKernelGGL(range_decode_kernel<true>, dim3(B * segs), dim3(64), 0, (hipStream_t)stream, in, stride, lengths,
                     lstride, loff, meta, meta_off, tables, Lmax, C, HW, out_nchw, err, B, per_element ? 1 : 0,
                     seg_lengths, __builtin_ctz((unsigned)segs));
  return check_launch("range_decode_seg");
}

// A HIP stream restricted to a subset of the compute units (mask bit i = CU i
// enabled).  Lets the serial range coder own a few CUs while the conv kernels
// of the next batch run on the others.  The caller destroys it.
extern "C" int dsic_stream_create_masked(const uint32_t* mask_host, int words, void** stream_out) {
  DSIC_REQUIRE(mask_host && stream_out && words >= 1, "stream_create_masked: bad argument");
  hipStream_t st = nullptr;
  hipError_t e = hipExtStreamCreateWithCUMask(&st, (uint32_t)words, mask_host);
  if (e != hipSuccess) {
    set_error("hipExtStreamCreateWithCUMask: %s", hipGetErrorString(e));
    return DSIC_EHIP;
  }
  *stream_out = (void*)st;
  return DSIC_OK;
}
extern "C" int dsic_stream_destroy(void* stream) {
  hipError_t e = hipStreamDestroy((hipStream_t)stream);
  if (e != hipSuccess) {
    set_error("hipStreamDestroy: %s", hipGetErrorString(e));
    return DSIC_EHIP;
  }
  return DSIC_OK;
}

// Host-side evaluation of the same table math (CPU tests compare it with the
// oracle without a GPU; the device kernels are compared on the GPU box).
extern "C" double dsic_host_normal_cdf(double x) { return dm::normal_cdf(x); }
extern "C" double dsic_host_student_t_cdf(double t, double nu) { return dm::student_t_cdf(t, nu); }
extern "C" float dsic_host_gaussian_cdf_f32(float x) { return dm::gaussian_cdf_f32(x); }
extern "C" float dsic_host_exp_f32(float x) { return (float)dm::exp((double)x); }
extern "C" int dsic_host_pmf_to_uint16_cdf(const float* pmf_host, int L, int C, uint16_t* out_host) {
  // :17-23 on a host pmf [L][C] (support axis first, like the reference) -> out [L+1][C]
  DSIC_REQUIRE(pmf_host && out_host && L >= 1 && C >= 1, "host_pmf_to_uint16_cdf: bad argument");
  for (int c = 0; c < C; ++c) {
    double cum = 0.0;
    out_host[c] = 0;
    for (int k = 0; k < L; ++k) {
      cum = cum + (double)pmf_host[(size_t)k * C + c];
      float v = (float)cum;
      if (k == L - 1 && v < 1.0f) v = 1.0f;
      float sc = v * 65535.0f;
      if (sc < 0.0f) sc = 0.0f;
      if (sc > 65535.0f) sc = 65535.0f;
      out_host[(size_t)(k + 1) * C + c] = (uint16_t)sc;
    }
  }
  return DSIC_OK;
}
extern "C" int dsic_host_cdf_table(int student, float sigma, float nu, int smin, int L,
                                   uint16_t* out_host, uint16_t* raw_host) {
  DSIC_REQUIRE(out_host && L >= 1 && L <= 4096, "host_cdf_table: bad argument");
  float F[4097], pmf[4096];
  for (int k = 0; k <= L; ++k)
    F[k] = student ? dm::table_cdf_student(smin, k, sigma, nu) : dm::table_cdf_gauss(smin, k, sigma);
  dm::finish_table(F, L, out_host, pmf, raw_host);
  return DSIC_OK;
}
