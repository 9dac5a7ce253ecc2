// Device helpers shared by the byte movers of image_codec.hip, residual_block.h and mask.hip: 16-byte loads from any
// address, a string copy split over workgroups, the workgroup prefix sum and the one loop over it that turns n string
// lengths into offsets (scan_offsets), and the little-endian field writers of the container heads; and the workgroup
// counts of their launches.  The chunk walk of
// the HWC outputs is hwc_chunks.h.  Whether two buffers meet is buffers_apart of common.h.
#pragma once
#include "common.h"

namespace dsic {

// 16 bytes from any address: aligned dword loads funnelled by __builtin_amdgcn_alignbyte.  The dwords read
// start at the aligned-down address of p and end at the dword holding p[15], so no byte outside the
// allocation's dwords is touched.
__device__ __forceinline__ uint4 load16_any(const uint8_t* p) {
  const uintptr_t a = (uintptr_t)p;
  if ((a & 15) == 0) return *(const uint4*)p;
  const int sh = a & 3;
  const uint32_t* w = (const uint32_t*)(a - sh);
  const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3];
  if (sh == 0) return make_uint4(w0, w1, w2, w3);
  const uint32_t w4 = w[4];
  return make_uint4(__builtin_amdgcn_alignbyte(w1, w0, sh), __builtin_amdgcn_alignbyte(w2, w1, sh),
                    __builtin_amdgcn_alignbyte(w3, w2, sh), __builtin_amdgcn_alignbyte(w4, w3, sh));
}

// n bytes src -> dst (any alignments), split over `parts` workgroups of blockDim.x threads: the destination's
// aligned 16-byte chunks are whole dwordx4 stores, the ragged head and tail are byte stores (their neighbours
// belong to another string or to the header and are written by another workgroup).
__device__ inline void copy_bytes(uint8_t* dst, const uint8_t* src, int64_t n, int part, int parts) {
  if (n <= 0) return;
  int64_t head = (16 - ((uintptr_t)dst & 15)) & 15;
  if (head > n) head = n;
  const int64_t nfull = (n - head) >> 4;
  const int64_t tail = head + 16 * nfull;
  if (part == 0) {
    for (int64_t i = threadIdx.x; i < head; i += blockDim.x) dst[i] = src[i];
    for (int64_t i = tail + threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i];
  }
  for (int64_t c = (int64_t)part * blockDim.x + threadIdx.x; c < nfull; c += (int64_t)parts * blockDim.x)
    *(uint4*)(dst + head + 16 * c) = load16_any(src + head + 16 * c);
}

// exclusive prefix sum over a 256-thread workgroup; *total = sum of all v
__device__ inline long long block_exclusive_scan(long long v, long long* lds4, long long* total) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  long long s = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const long long t = __shfl_up(s, o, 64);
    if (lane >= o) s += t;
  }
  if (lane == 63) lds4[wid] = s;
  __syncthreads();
  long long base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    base += w < wid ? lds4[w] : 0;
    tot += lds4[w];
  }
  __syncthreads();
  *total = tot;
  return base + s - v;
}

// n lengths -> offsets, by one 256-thread workgroup: out[s] = len(0) + ... + len(s - 1) for s < n, 256 lengths per pass
// with the carry of the passes before; returns the sum of all n (in every thread).  len(s) is called once, by the
// thread that writes out[s].  The head kernels of the container, the residual block and the mask records use it.
template <class F>
__device__ inline long long scan_offsets(int n, F len, long long* lds4, long long* out) {
  long long carry = 0;
  for (int s0 = 0; s0 < n; s0 += blockDim.x) {
    const int s = s0 + threadIdx.x;
    long long tot;
    const long long ex = block_exclusive_scan(s < n ? (long long)len(s) : 0, lds4, &tot);
    if (s < n) out[s] = carry + ex;
    carry += tot;
  }
  return carry;
}

__device__ __forceinline__ float clamp01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }  // torch clamp(0,1)

__device__ __forceinline__ void put_u32(uint8_t* p, int byte, uint32_t v) { *p = (uint8_t)(v >> (8 * byte)); }
__device__ __forceinline__ int64_t clamp_len(int v, int64_t cap) { return v < 0 ? 0 : (v > cap ? cap : v); }

// workgroups per string of a string mover: 4 KiB per workgroup pass, at most 8
static inline int string_parts(int64_t max_len) {
  const int64_t p = (max_len + 16 * 256 - 1) / (16 * 256);
  return (int)(p < 1 ? 1 : (p > 8 ? 8 : p));
}

// workgroups of a flat grid-stride pass over `units` 16-byte units, one unit per thread and pass
static inline int flat_blocks(int64_t units) {
  const int64_t b = (units + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}

}  // namespace dsic
