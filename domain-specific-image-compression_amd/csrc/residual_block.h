// The residual block of a batch, written on the device once for its two widths: the uint8 layer's "DSICR" block
// (residual.hip) and the uint16 layer's "DSICW" block (residual_u16.hip), which adds a shift k to every record and k raw
// bit planes to every span (little endian):
//
//   "DSIC" tag "\0" | n, C, th, tw, tau, bands u32 | n x (smin i32, L u32, [k u32,] span_bytes u32) |
//   n x 16 u32 segment lengths | per tile its span: C x L uint16 tables | [k planes of pb = C th tw / 8 bytes] |
//   the 16 segment strings
//
// A tile's span is P = C + (1) + 16 pieces: table row c (2 L bytes of compact row c), the planes (k pb bytes: the first k
// of the tile's plane slots, which lie back to back), then segment j (lengths[t][1 + j] bytes at bytes + t (cap_z +
// 16 cap_seg) + cap_z + j cap_seg: the output of dsic_range_encode_seg_ws, whose z string is the dummy and is dropped).
// What differs is a compile-time shape, so each instantiation is straight-line code for its own block.
#pragma once
#include "byte_movers.h"

namespace dsic {

constexpr int kResBands = 16;  // row bands per colour plane = segments per tile
constexpr int kResHead = 30;   // magic | n, C, th, tw, tau, bands u32

// tag: the magic's fifth letter; rec: bytes of a record; planes: 1 if a record carries k and a span its planes; slots:
// plane slots per tile in the encoder's buffer; lmax: the row length of the compact tables, 0 = the launch gives it
struct NarrowBlock {
  static constexpr char tag = 'R';
  static constexpr int rec = 12, planes = 0, slots = 0, lmax = 0;
};
struct WideBlock {
  static constexpr char tag = 'W';
  static constexpr int rec = 16, planes = 1, slots = 9, lmax = 512;
};

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

template <class S>
__device__ __forceinline__ int64_t piece_len(int j, int C, int L, int k, int64_t pb, const int* lengths_t,
                                             int64_t cap_seg) {
  if (j < C) return 2 * (int64_t)L;
  if constexpr (S::planes) {
    if (j == C) return k * pb;
  }
  return clamp_len(lengths_t[1 + j - C - S::planes], cap_seg);
}
template <class S>
__device__ __forceinline__ int table_width(const int* meta, int t, int Lmax) {
  const int L = meta[4 * t + 1], top = S::lmax ? S::lmax : Lmax;
  return L < 1 ? 0 : (L > top ? top : L);
}
template <class S>
__device__ __forceinline__ int tile_planes(const int* kk, int t) {
  if constexpr (S::planes) {
    const int k = kk[t];
    return k < 0 ? 0 : (k > S::slots ? S::slots : k);
  }
  return 0;
}
template <class S>
__host__ __device__ inline int64_t body_offset(int n) {
  return kResHead + (int64_t)S::rec * n + (int64_t)4 * kResBands * n;
}

// one workgroup: head, records, segment lengths, and the exclusive scan of the n P piece lengths into ws[2 ..];
// ws[0] = block bytes, ws[1] = the coder's error word.  kk is read only by a block with planes.
template <class S>
__global__ __launch_bounds__(256) void residual_pack_head_kernel(const int* __restrict__ lengths,
                                                                 const int* __restrict__ meta,
                                                                 const int* __restrict__ kk,
                                                                 const int* __restrict__ err, int n, int C, int th,
                                                                 int tw, int tau, int Lmax, int64_t cap_seg,
                                                                 long long* __restrict__ ws,
                                                                 uint8_t* __restrict__ out) {
  __shared__ long long lds4[4];
  const int tid = threadIdx.x;
  const int P = C + S::planes + kResBands, Sl = 1 + kResBands;
  const int64_t pb = S::planes ? (int64_t)C * th * tw / 8 : 0;
  if (tid < kResHead) {
    const char magic[6] = {'D', 'S', 'I', 'C', S::tag, 0};
    const uint32_t f[6] = {(uint32_t)n, (uint32_t)C, (uint32_t)th, (uint32_t)tw, (uint32_t)tau, (uint32_t)kResBands};
    if (tid < 6) out[tid] = (uint8_t)magic[tid];
    else put_u32(out + tid, (tid - 6) & 3, f[(tid - 6) >> 2]);
  }
  for (int i = tid; i < S::rec * n; i += blockDim.x) {
    const int t = i / S::rec, b = i - t * S::rec;
    const int L = table_width<S>(meta, t, Lmax), k = tile_planes<S>(kk, t);
    uint32_t v;
    switch (b >> 2) {
      case 0: v = (uint32_t)meta[4 * t]; break;
      case 1: v = (uint32_t)L; break;
      case S::rec / 4 - 1:  // span_bytes, a record's last word
        v = 0;
        for (int j = 0; j < P; ++j) v += (uint32_t)piece_len<S>(j, C, L, k, pb, lengths + Sl * t, cap_seg);
        break;
      default: v = (uint32_t)k; break;
    }
    put_u32(out + kResHead + i, b & 3, v);
  }
  for (int i = tid; i < 4 * kResBands * n; i += blockDim.x) {
    const int e = i >> 2, t = e / kResBands, j = e - t * kResBands;
    put_u32(out + kResHead + (int64_t)S::rec * n + i, i & 3, (uint32_t)clamp_len(lengths[Sl * t + 1 + j], cap_seg));
  }
  const long long total = scan_offsets(
      P * n,
      [&](int s) {
        const int t = s / P;
        return piece_len<S>(s - t * P, C, table_width<S>(meta, t, Lmax), tile_planes<S>(kk, t), pb, lengths + Sl * t,
                            cap_seg);
      },
      lds4, ws + 2);
  if (tid == 0) {
    ws[2 + P * n] = total;
    ws[0] = body_offset<S>(n) + total;
    ws[1] = err ? *err : 0;
  }
}

// blockIdx.y = piece (tile s / P), blockIdx.x = slice of it.  kk, planes, th and tw are read only by a block with planes.
template <class S>
__global__ __launch_bounds__(256) void residual_pack_pieces_kernel(const uint8_t* __restrict__ bytes,
                                                                   const int* __restrict__ lengths,
                                                                   const int* __restrict__ meta,
                                                                   const int* __restrict__ kk,
                                                                   const uint16_t* __restrict__ compact,
                                                                   const uint8_t* __restrict__ planes, int n, int C,
                                                                   int th, int tw, int Lmax, int64_t cap_z,
                                                                   int64_t cap_seg, const long long* __restrict__ ws,
                                                                   uint8_t* __restrict__ out) {
  const int P = C + S::planes + kResBands, Sl = 1 + kResBands;
  const int s = blockIdx.y, t = s / P, j = s - t * P;
  const int64_t pb = S::planes ? (int64_t)C * th * tw / 8 : 0;
  const int row = S::lmax ? S::lmax : Lmax;
  const uint8_t* src;
  if (j < C) src = (const uint8_t*)(compact + ((size_t)t * C + j) * row);
  else if (S::planes && j == C) src = planes + (size_t)t * S::slots * pb;
  else src = bytes + (size_t)t * (cap_z + kResBands * cap_seg) + cap_z + (int64_t)(j - C - S::planes) * cap_seg;
  copy_bytes(out + body_offset<S>(n) + ws[2 + s], src,
             piece_len<S>(j, C, table_width<S>(meta, t, Lmax), tile_planes<S>(kk, t), pb, lengths + Sl * t, cap_seg),
             blockIdx.x, gridDim.x);
}

// the two launches of dsic_residual_pack / dsic_residual_pack_u16, after their argument checks; longest: the longest
// piece a tile can have, which sizes the copy grid
template <class S>
int launch_pack(const char* head_what, const char* pieces_what, const uint8_t* bytes, int64_t cap_z, int64_t cap_seg,
                const int* lengths, const int* meta, const int* kk, const uint16_t* compact, const uint8_t* planes,
                const int* err, int n, int C, int th, int tw, int tau, int Lmax, int64_t longest, int64_t* workspace,
                uint8_t* out, hipStream_t st) {
  long long* ws = (long long*)workspace;
  hipLaunchKernelGGL(residual_pack_head_kernel<S>, dim3(1), dim3(256), 0, st, lengths, meta, kk, err, n, C, th, tw, tau,
                     Lmax, cap_seg, ws, out);
  const int rc = check_launch(head_what);
  if (rc) return rc;
  hipLaunchKernelGGL(residual_pack_pieces_kernel<S>, dim3(string_parts(longest), (C + S::planes + kResBands) * n),
                     dim3(256), 0, st, bytes, lengths, meta, kk, compact, planes, n, C, th, tw, Lmax, cap_z, cap_seg,
                     (const long long*)ws, out);
  return check_launch(pieces_what);
}

}  // namespace dsic
