// Device side of the Winograd translation units (conv_wino.hip, conv_wino_bf16.hip, conv_wino_bf16m.hip): the tile
// hand-out of a persistent workgroup, the fused bias + activation epilogue and the packed subtraction, each stated
// once.  The counterpart of wino_host.h: no host code.
#pragma once
#include <type_traits>

#include "common.h"

namespace dsic {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef float floatx2 __attribute__((ext_vector_type(2)));
typedef int intx4 __attribute__((ext_vector_type(4)));
typedef unsigned uintx4 __attribute__((ext_vector_type(4)));
typedef unsigned uintx2 __attribute__((ext_vector_type(2)));

namespace wino {

// ---- tile hand-out ----------------------------------------------------------------------------------------------
// Tiles are handed out dynamically (first round = blockIdx.x, then a global ticket): a CU that is slowed down - e.g.
// by co-resident waves of another stream - simply takes fewer tiles.  Helper thread 0 fetches the ticket one tile
// ahead, splits it into (tx, ty, n) (the only integer divisions of the kernel) and posts the descriptor in a 3-slot
// LDS ring: slot k % 3 = the k-th tile of this workgroup.  A slot is written before a workgroup barrier and read
// after it; an item >= ntiles ends the loop of every wave.
// The ticket is two counters: [0] tiles handed out beyond the first round, [1] finished workgroups.  The caller
// zeroes them once; the last workgroup of a launch zeroes them again, for the next launch on the stream.
struct Tile {
  int item, tx, ty, n;  // work item (tile * nphase + phase) and its tile coordinates
  int ks;               // split-K: which run of chunks (else 0)
};

// slot s of the ring, as wave-uniform values.  SPLITK: ty and ks share a word, ty | ks << 16
template <bool SPLITK>
__device__ __forceinline__ Tile read_tile(const float* slots, int s) {
  const intx4 v = *(const intx4*)(slots + 4 * s);
  Tile t;
  t.item = __builtin_amdgcn_readfirstlane(v[0]);
  t.tx = __builtin_amdgcn_readfirstlane(v[1]);
  t.ty = SPLITK ? __builtin_amdgcn_readfirstlane(v[2]) & 0xFFFF : __builtin_amdgcn_readfirstlane(v[2]);
  t.ks = SPLITK ? __builtin_amdgcn_readfirstlane(v[2]) >> 16 : 0;
  t.n = __builtin_amdgcn_readfirstlane(v[3]);
  return t;
}

// helper thread 0 only: work item `item` (run ks of its chunks; 0 without split-K) into slot s
__device__ __forceinline__ void post_tile(float* slots, int s, int item, int ks, int pshift, int tiles_x, int tiles_y) {
  const int tile = item >> pshift;
  const int row = tile / tiles_x;
  const intx4 v = {item, tile - row * tiles_x, (row % tiles_y) | (ks << 16), row / tiles_y};
  *(intx4*)(slots + 4 * s) = v;
}

__device__ __forceinline__ int take_ticket(unsigned long long* ticket) {
  return (int)(atomicAdd(ticket, 1ULL) + gridDim.x);
}

// helper thread 0 of a workgroup that has finished: the last one out re-arms the ticket
__device__ __forceinline__ void rearm_ticket(unsigned long long* ticket) {
  const unsigned long long done = atomicAdd(ticket + 1, 1ULL);
  if (done == (unsigned long long)gridDim.x - 1) {
    ticket[0] = 0ULL;
    ticket[1] = 0ULL;
  }
}

// Ring 0, 1, 2 at the end of a tile.  Helper side: the next tile's slot becomes the current one, the slot written
// during this tile the next, and the slot of the finished tile becomes writable.  MFMA side: one slot on.
__device__ __forceinline__ void rotate_ring(int& s_nxt, int& s_wr) {
  const int s_old = s_nxt;
  s_nxt = s_wr;
  s_wr = s_old == 0 ? 2 : s_old - 1;
}
__device__ __forceinline__ int step_ring(int s_nxt) { return s_nxt == 2 ? 0 : s_nxt + 1; }

// ---- epilogue ---------------------------------------------------------------------------------------------------
// bias, then GDN / IGDN / ReLU, on two values of one output channel
template <int ACT>
__device__ __forceinline__ floatx2 bias_act(floatx2 v, float bias, float beta, float gamma) {
  v = v + floatx2{bias, bias};
  if (ACT == DSIC_ACT_GDN || ACT == DSIC_ACT_IGDN) {
    v = gdn_pair<ACT == DSIC_ACT_IGDN>(v, floatx2{beta, beta}, floatx2{gamma, gamma});
  } else if (ACT == DSIC_ACT_RELU) {
    v[0] = v[0] > 0.f ? v[0] : 0.f;
    v[1] = v[1] > 0.f ? v[1] : 0.f;
  }
  return v;
}

// f(std::integral_constant<int, act>{}): the epilogue is compiled once per activation, the branch is uniform
template <class F>
__device__ __forceinline__ void for_act(int act, F&& f) {
  if (act == DSIC_ACT_GDN)
    f(std::integral_constant<int, DSIC_ACT_GDN>{});
  else if (act == DSIC_ACT_IGDN)
    f(std::integral_constant<int, DSIC_ACT_IGDN>{});
  else if (act == DSIC_ACT_RELU)
    f(std::integral_constant<int, DSIC_ACT_RELU>{});
  else
    f(std::integral_constant<int, DSIC_ACT_NONE>{});
}

// ---- packed subtraction -----------------------------------------------------------------------------------------
// a - b on two / four / sixteen floats with packed fp32 instructions.  The compiler packs fp32 additions
// (v_pk_add_f32) but leaves subtractions scalar (there is no v_pk_sub_f32); the negation is an operand modifier of
// the same instruction, so a - b costs the same single issue slot.  Every VALU issue slot matters here: a SIMD cannot
// issue VALU work of any wave while an MFMA is waiting for the matrix pipe (tools/coissue3.hip).
__device__ __forceinline__ floatx2 pk_sub(floatx2 a, floatx2 b) {
  floatx2 r;
  asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ floatx4 sub4(floatx4 a, floatx4 b) {
  const floatx2 lo = pk_sub(__builtin_shufflevector(a, a, 0, 1), __builtin_shufflevector(b, b, 0, 1));
  const floatx2 hi = pk_sub(__builtin_shufflevector(a, a, 2, 3), __builtin_shufflevector(b, b, 2, 3));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3);
}
__device__ __forceinline__ floatx16 sub16(floatx16 a, floatx16 b) {
  floatx16 r;
#pragma unroll
  for (int i = 0; i < 16; i += 2) {
    const floatx2 x = {a[i], a[i + 1]}, y = {b[i], b[i + 1]};
    const floatx2 d = pk_sub(x, y);
    r[i] = d[0];
    r[i + 1] = d[1];
  }
  return r;
}

}  // namespace wino
}  // namespace dsic
