// Step, slot and chunk-pass tables of the 64-tile split-bf16 Winograd kernel (conv_wino_bf16m.hip), as constexpr
// functions of host and device: the kernel's helper and MFMA waves read the schedule of a tile from here, and so
// does dsic_wino_pair_schedule (the host restatement that tests/test_pair_chunks_cpu.py compares for both
// schedules).
//
// Pass B of a tile walks the Winograd rows xi = 0 (wave half PQ 0) and xi = 3 (PQ 1).  Where one of them is
// structurally zero (MODE 1: xi = 3 in the space-to-depth blocks blk >> 1 == 1, i.e. the upper half of the chunks;
// MODE 2: xi = 0 for the ConvTranspose phases phase >> 1 == 1, the whole pass), two consecutive chunks c, c + 1 run
// as ONE chunk-pass: the live row of c in its own four V slots, the live row of c + 1 in the four slots of the dead
// row, and the wave that owns the live row runs eight steps into the same four positions - chunk c's, then chunk
// c + 1's, so every accumulator receives the same products in the same order as in the unpaired schedule.
#pragma once

#if defined(__HIPCC__)
#define WBM_HD __host__ __device__ __forceinline__
#else
#define WBM_HD inline
#endif

namespace dsic {
namespace wbm {

// Steps of a chunk for wave half PQ in pass PASS: 4 bits per step s, global position xi*4 + nu.  Positions that can
// be structurally zero come last (MODE 1: xi = 3 / nu = 3; MODE 2: xi = 0 / nu = 0), so the two fragments
// prefetched across a chunk boundary are live in (almost) every chunk.
template <int MODE, int PASS, int PQ>
struct Steps {
  // pass A: row xi = 1 + PQ; pass B: row xi = 0 (PQ 0) / 3 (PQ 1); nu ascending (MODE 2: descending, nu = 0 can vanish)
  static constexpr unsigned value =
      PASS == 0 ? (PQ == 0 ? (MODE == 2 ? 0x4567u : 0x7654u) : (MODE == 2 ? 0x89ABu : 0xBA98u))
                : (PQ == 0 ? (MODE == 2 ? 0x0123u : 0x3210u) : (MODE == 2 ? 0xCDEFu : 0xFEDCu));
};
template <int MODE, int PASS, int PQ>
WBM_HD constexpr int gpos(int s) {
  return (int)((Steps<MODE, PASS, PQ>::value >> (4 * s)) & 15u);
}
// index of a global position inside the V buffer of its pass (8 positions: the pass's two xi rows x 4 nu)
template <int PASS>
WBM_HD constexpr int lpos_of(int g) {
  return PASS == 0 ? ((g >> 2) - 1) * 4 + (g & 3) : ((g >> 2) == 3 ? 4 : 0) + (g & 3);
}
// step that holds global position g
template <int MODE, int PASS, int PQ>
WBM_HD constexpr int step_of(int g) {
  for (int s = 0; s < 4; ++s)
    if (gpos<MODE, PASS, PQ>(s) == g) return s;
  return -1;
}

// ---- pass B with paired chunks ----------------------------------------------------------------------------------
// The structurally zero Winograd row of a mode's half-empty chunks, the row that is live there, and the wave half
// that owns the live row in pass B.
WBM_HD constexpr int pair_dead_xi(int mode) { return mode == 2 ? 0 : 3; }
WBM_HD constexpr int pair_live_xi(int mode) { return mode == 2 ? 3 : 0; }
WBM_HD constexpr int pair_owner(int mode) { return mode == 2 ? 1 : 0; }
// First chunk of pass B that runs paired (nchunks: none).  MODE 1: the chunks of the blocks 2 and 3, when the block
// boundaries fall on multiples of 4 chunks (a pair never straddles a block, and the pass keeps an even number of
// chunk-passes: the V buffers alternate through the tile boundary).  MODE 2: the whole pass of a phase 2 / 3 item,
// when that leaves an even number of chunk-passes.
WBM_HD constexpr int pair_first(int mode, int nchunks, int phase, bool on) {
  if (!on) return nchunks;
  if (mode == 1) return nchunks % 8 == 0 ? nchunks / 2 : nchunks;
  if (mode == 2) return ((phase >> 1) & 1) && nchunks % 4 == 0 ? 0 : nchunks;
  return nchunks;
}
// chunk-passes of pass B, and the first chunk of its chunk-pass j (paired from chunk-pass pfirst on)
WBM_HD constexpr int pass_b_len(int nchunks, int pfirst) { return pfirst + (nchunks - pfirst) / 2; }
WBM_HD constexpr int pass_b_chunk(int j, int pfirst) { return j < pfirst ? j : pfirst + 2 * (j - pfirst); }
// The structurally zero row / column of chunk k (4 = none).  MODE 1: the space-to-depth block of chunk k is
// blk = k / (nchunks / 4) (nchunks is a multiple of 4 there), row 3 vanishes for blk >> 1, column 3 for blk & 1 -
// stated as comparisons: the kernel asks per chunk-pass, and an integer division is dozens of instructions.
WBM_HD constexpr unsigned zero_xi_of(int mode, int nchunks, int phase, int k) {
  return mode == 1 ? (k >= 2 * (nchunks >> 2) ? 3u : 4u) : mode == 2 ? (((phase >> 1) & 1) ? 0u : 4u) : 4u;
}
WBM_HD constexpr unsigned zero_nu_of(int mode, int nchunks, int phase, int k) {
  return mode == 1 ? (((k >= (nchunks >> 2) && k < 2 * (nchunks >> 2)) || k >= 3 * (nchunks >> 2)) ? 3u : 4u)
                   : mode == 2 ? ((phase & 1) ? 0u : 4u) : 4u;
}
// Step s < 8 of a paired chunk-pass, for the wave that owns the live row: chunk c + pair_half(s), the position and
// the accumulator of step s & 3, and the V slot - the position's own for chunk c, the dead row's for chunk c + 1.
WBM_HD constexpr int pair_half(int s) { return s >> 2; }
WBM_HD constexpr int pair_acc(int s) { return s & 3; }
template <int MODE, int PQ>
WBM_HD constexpr int pair_gpos(int s) {
  return gpos<MODE, 1, PQ>(s & 3);
}
template <int MODE, int PQ>
WBM_HD constexpr int pair_vslot(int s) {
  return lpos_of<1>(pair_gpos<MODE, PQ>(s)) ^ (pair_half(s) << 2);
}
// V slot into which the helpers commit position (live row, nu) of chunk c + half
WBM_HD constexpr int pair_commit_slot(int mode, int half, int nu) {
  return ((pair_live_xi(mode) == 3 ? 4 : 0) ^ (half << 2)) + nu;
}
// A paired window holds, per chunk, only the nine window rows its live row reads (patch rows 0, 2 for xi = 0: the
// even rows; 1, 3 for xi = 3: the odd rows): window row of stored row r
WBM_HD constexpr int pair_window_row(int mode, int r) { return 2 * r + (pair_live_xi(mode) == 3 ? 1 : 0); }

}  // namespace wbm
}  // namespace dsic
