// Split-bf16 Winograd F(2x2,3x3) for the LARGE layers: 64 Winograd tiles (16x16 output pixels) per workgroup,
// the 16 positions processed as TWO PASSES of 8 (code/modelv2/layers.py:54-72, 86-97: every conv(.,.,3,1),
// conv(C,C,5,2) over space-to-depth and ConvTranspose2d(.,.,5,2,2,1) whose H and W are multiples of 16).
//
// Why: conv_wino_bf16.hip (32 tiles x 16 positions x 128 channels in the accumulators) uses every fragment of the
// transformed weights U for ONE 32-tile MFMA operand: 128 KB of U per 16-channel chunk against 1536 cycles of MFMA
// issue per SIMD = 85 B/clk/CU from L2 - more than the vector-memory path delivers (64 B/clk/CU), and measured:
// with twice the MFMAs per fetched fragment (-DWB_ABL=128) that kernel takes 1.27-1.36x the time for 2x the matrix
// work.  Here a wave owns 4 positions x 2 M tiles x 32 channels (the same 128 accumulator registers) and uses every
// U fragment for both M tiles: half the U bytes per MFMA, and a fragment requested two steps ahead has 2 x 6 MFMAs
// to arrive instead of 2 x 3.
//
// Two passes.  Pass A accumulates the positions of the Winograd rows xi = 1, 2 over all input channels, pass B the
// rows xi = 0, 3.  Y = A^T M A with A^T = [[1,1,1,0],[0,1,-1,-1]]: row xi = 0 feeds only the output row i = 0, row
// xi = 3 only i = 1 (negated).  So the contribution P[i][j] of pass A is folded INTO pass B's accumulators before
// pass B starts - corner positions M[0][0] += P[0][0], M[0][3] -= P[0][1], M[3][0] -= P[1][0], M[3][3] += P[1][1] -
// and the fold after pass B yields the complete outputs: no partial sums leave the registers except the one
// exchange between the two waves of a channel group (LDS, 64 KB per tile at the pass boundary, 128 KB at the end).
//   pass A: wave (nt, pq) owns row xi = 1 + pq (4 positions); C[0] = M0+M1+M2, C[1] = M1-M2-M3 per row;
//           P[0][j] = C1[j] + C2[j], P[1][j] = C1[j] - C2[j]: pq 0 keeps column j = 0 (needs C2[0]), pq 1 column 1.
//   pass B: pq 0 owns (0,0) (0,1) (3,0) (3,1), pq 1 owns (0,2) (0,3) (3,2) (3,3); pq 0 finishes the outputs (i, 0),
//           pq 1 the outputs (i, 1), each with two accumulators of the other.
// The finished outputs (bias + GDN/IGDN/ReLU in registers, as in conv_wino_bf16.hip) leave as global_store_dword
// straight from the accumulator layout: lane = output channel, so 32 lanes write one pixel's 128 contiguous bytes.
// No output staging in LDS, no copy-out by the helper waves (they are the longer pole of a phase here).
//
// Half-empty chunk-passes.  Where one of pass B's two rows is structurally zero (xi = 3 in the space-to-depth blocks 2
// and 3, xi = 0 for the ConvTranspose phases 2 and 3) one wave half issues alone and is held by its U fetches; two such
// chunks run as one chunk-pass (conv_wino_pair.h: tables, V slots, the shorter pass B), bit-identical to one each.
//
// Helper waves, window staging, U stream layout and the V layout in LDS are those of conv_wino_bf16.hip with
// 64 tiles x 8 positions in place of 32 x 16; the same packed weights serve both kernels.  Tile hand-out, epilogue
// and packed subtraction: wino_device.h.
#include "conv_wino_bf16.h"
#include "conv_wino_pair.h"
#include "wino_host.h"

#ifndef WBM_STAMP
#define WBM_STAMP 0   // diagnostic: cycle stamps of the MFMA waves 0 (PQ 0) and 4 (PQ 1) and of helper wave 8 (tools/wbm_stamps.py)
#endif
#ifndef WBM_STAMP_C0
#define WBM_STAMP_C0 0   // first chunk-pass of the tile that gets stamps (32 chunk-passes fit)
#endif
#ifndef WBM_ABL
#define WBM_ABL 0   // diagnostic, wrong results: 1 every window load from tile (0,0) of image 0 (cache hits), 2 no window loads
#endif

namespace dsic {
namespace wbm {

using wb::Args;
using wb::bf16_hi;
using wb::bf16_lo;
using wb::bf16x8;
using wb::cvt_pk_bf16;
using wino::sub4;
using wino::Tile;

constexpr int P = 2;                            // bf16 planes
constexpr int CK = 16;                          // channels per chunk = one MFMA k-step
constexpr int NTILE = 64;                       // Winograd tiles per workgroup tile (8 x 8 = 16 x 16 pixels)
constexpr int ROWB = CK * 2;                    // bytes per (pos, tile) row of a plane
constexpr int POSB = NTILE * ROWB;              // 2048
constexpr int PLANEB = 8 * POSB;                // 8 positions per pass: 16384
constexpr int VBUFB = P * PLANEB;               // 32768
constexpr int XOFF = 2 * VBUFB;                 // exchange region A (region B is V buffer 1, idle during a fold)
constexpr int XBYTES = 8 * 4096;                // one floatx16 per MFMA wave
constexpr int SLOTOFF = XOFF + XBYTES;
constexpr int WINW = 18, WINH = 18;             // input window of a 16x16-pixel tile (halo 1)
constexpr int WINITEMS = WINW * WINH * 4;       // float4 items of one chunk: 1296
constexpr int WINB = WINITEMS * 16;             // 20736 bytes
constexpr int NLOAD = (WINITEMS + 255) / 256;   // 6 window loads per helper thread
constexpr int STAGEOFF = SLOTOFF + 64;
constexpr int NWIN = 3;                          // window buffers: one being transformed, two in flight (LDS-DMA)
constexpr int STAMPOFF = STAGEOFF + NWIN * WINB;
constexpr int PARAMOFF = STAMPOFF + (WBM_STAMP ? 1536 : 0);   // bias, beta, gamma: [3][128] floats
constexpr int LDS_TOTAL = PARAMOFF + 3 * 128 * 4;
constexpr int THREADS = 768;
constexpr int RING = 2;
// a paired window: nine rows of each of two chunks, the second chunk's behind the first's
constexpr int PAIRITEMS = 9 * WINW * 4;          // float4 items of one chunk's half: 648
constexpr int PAIRHALFB = PAIRITEMS * 16;        // 10368 bytes

static_assert(LDS_TOTAL <= 160 * 1024, "LDS budget");
static_assert(2 * PAIRITEMS == WINITEMS, "a paired window fills one window buffer, piece for piece");

#if WBM_STAMP
// per workgroup 384 stamps: [0, 128) MFMA wave 0, [128, 256) helper wave 8, [256, 384) MFMA wave 4.  An MFMA wave
// has 3 stamps per chunk-pass at 3 (sigma - C0), its folds at 120..126 and the tile's item at 127; the helper 4 per
// chunk-pass at 4 (sigma - C0).  Low 32 bits of s_memtime (the LDS copy is 4 bytes per stamp).
static __device__ long long wbm_stamps[256 * 384];
#define MSTAMP(w, i)                                                                                   \
  do {                                                                                                 \
    __builtin_amdgcn_sched_barrier(0);                                                                 \
    if (lane == 0 && wave == (w) && tile_count == 3 && (i) >= 0 && (i) < 128)                          \
      ((unsigned*)(lds_raw + STAMPOFF))[((w) == 0 ? 0 : (w) == 8 ? 128 : 256) + (i)] = (unsigned)__builtin_amdgcn_s_memtime();   \
    __builtin_amdgcn_sched_barrier(0);                                                                 \
  } while (0)
// stamp k of chunk-pass sigma, PER stamps per chunk-pass, inside the window of 32 chunk-passes from WBM_STAMP_C0
#define MSTAMPC(w, sigma, k, PER)                                                                      \
  do {                                                                                                 \
    if ((sigma) >= WBM_STAMP_C0 && (sigma) < WBM_STAMP_C0 + 32) MSTAMP(w, (PER) * ((sigma) - WBM_STAMP_C0) + (k)); \
  } while (0)
#else
#define MSTAMP(w, i)
#define MSTAMPC(w, sigma, k, PER)
#endif

// The lane id, recomputed where it is used: volatile, so it is neither hoisted out of the tile loop nor kept in a
// register through the MFMA loops (which have 16 registers to spare beside accumulators, ring and V fragments).
__device__ __forceinline__ int lane_now() {
  int l;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
  return l;
}

template <int MODE, bool NT_OUT>
__global__ __launch_bounds__(THREADS) void conv_wino_bf16m_kernel(const Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  float* const slots = (float*)(lds_raw + SLOTOFF);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  auto read_slot = [&](int s) { return wino::read_tile<false>(slots, s); };
  const int pshift = a.nphase == 4 ? 2 : 0;
  const int nchunks = a.Cin / CK;   // even, >= 4 (host)
  // Chunk-passes of a tile: sigma < nchunks is pass A, the rest pass B, whose chunks run paired from chunk
  // pfirst on (conv_wino_pair.h; a.pair_b = 0: never).  Helper and MFMA waves derive pfirst, and from it the length
  // nchunks + pass_b_len of the tile, from the same slot record.
  constexpr bool PAIR = MODE != 0;
  auto pfirst_of = [&](const Tile& t) { return PAIR ? pair_first(MODE, nchunks, t.item & 3, a.pair_b != 0) : nchunks; };
  int tile_count = 0;
  (void)tile_count;
  // per-channel epilogue parameters live in LDS: the MFMA waves read them at the fold (an LDS read is not ordered
  // behind their global stores, a register would be one of the 16 they have to spare)
  if (tid < 128) {
    float* const prm = (float*)(lds_raw + PARAMOFF);
    const bool cv = tid < a.Cout, gd = cv && (a.act == DSIC_ACT_GDN || a.act == DSIC_ACT_IGDN);
    prm[tid] = cv ? a.bias[tid] : 0.f;
    prm[128 + tid] = gd ? a.beta[tid] : 1.f;
    prm[256 + tid] = gd ? a.gamma[tid] : 0.f;
  }

  if (wave >= 8) {
    // =================================== helper waves ===========================================
    // thread = (Winograd tile pt of 64, channel quad pq of the 16-channel chunk): the 8 positions of the pass
    __builtin_amdgcn_s_setprio(3);
    const int ht = tid - 512;
    const int Cin = a.Cin;
    const int pt = ht >> 2, pq = ht & 3;
    const int ptx = pt & 7, pty = pt >> 3;
    const int vwrite = pt * ROWB + ((((pq >> 1) ^ ((pt >> 3) & 1))) << 4) + ((pq & 1) << 3);
    unsigned char* const vmine = lds_raw + vwrite;
    auto post = [&](int s, int item) { wino::post_tile(slots, s, item, 0, pshift, a.tiles_x, a.tiles_y); };
    // Input side.  The 18x18-pixel window of the tile (halo 1; 16 channels of the chunk, fp32) goes from global
    // memory straight into one of three LDS window buffers (buffer_load_dwordx4 ... lds: no registers, no staging
    // stores): item i = (pixel i >> 2, channel quad i & 3) lies at byte 16 i of the buffer, i.e. the 64 lanes of a
    // wave-instruction fill 1 KB at M0 + 16 lane.  Helper wave hw issues the items hw*64 + 256 j + lane (j < 6; the
    // last, partial piece belongs to the lanes 0..15 of wave 0).  The loads are inline asm: the compiler does not see
    // them (it would drain an LDS-DMA in front of every barrier), so the waits are counted here:
    //   phase sg: issue the window of chunk-pass sg + 3; transform sg + 1; wait for the window of sg + 2 (all but
    //             this wave's newest NDMA loads); barrier.
    // A window has two phases to arrive; an out-of-image pixel is an out-of-range offset (the DMA writes zeros).
    // Chunk-major input (a.cm_in, [B][Cin/16][H][W][16]): a pixel's 16 channels of the chunk are 64 contiguous bytes
    // and the chunk is a plane of H*W pixels, so a window row is 18 x 64 contiguous bytes and every line a window
    // fetches belongs to its own chunk (NHWC: 64-byte pieces Cin*4 bytes apart, two chunks per 128-byte line).  Only
    // the pixel stride and the chunk stride differ; the LDS window is the same.
    const int pix_f = a.cm_in ? CK : Cin;                                        // floats per pixel of the input
    const unsigned chunk_in_b = a.cm_in ? (unsigned)(a.H * a.W * CK * 4) : (unsigned)(CK * 4);   // bytes per chunk
    struct WinAim {
      unsigned off[NLOAD];
      uintx4 rsrc;
    };
    WinAim am;
    unsigned off2[NLOAD];   // a paired window's offsets (PAIR only); the descriptor is am's
    const int hw = wave - 8;
    const unsigned lds_base = (unsigned)(unsigned long long)(__attribute__((address_space(3))) unsigned char*)lds_raw;
    auto aim = [&](WinAim& m, const Tile& t0) {
      Tile t = t0;
      if (WBM_ABL & 1) { t.n = 0; t.tx = 0; t.ty = 0; }
      const unsigned long long base = (unsigned long long)(a.in + (size_t)t.n * a.H * a.W * Cin);
      m.rsrc = uintx4{(unsigned)base, (unsigned)(base >> 32) & 0xFFFFu, (unsigned)(a.H * a.W * Cin * 4), 0x00020000u};
#pragma unroll
      for (int j = 0; j < NLOAD; ++j) {
        const int i = ht + 256 * j;
        const int pix = i >> 2, q = i & 3;
        const int wy = pix / WINW, wx = pix - wy * WINW;
        const int gy = t.ty * 16 - 1 + wy, gx = t.tx * 16 - 1 + wx;
        const bool ok = i < WINITEMS && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W && !(WBM_ABL & 2);
        m.off[j] = ok ? (unsigned)(((gy * a.W + gx) * pix_f + 4 * q) * 4) : 0x80000000u;
      }
    };
    auto aim_nowhere = [&](WinAim& m) {
#pragma unroll
      for (int j = 0; j < NLOAD; ++j) m.off[j] = 0x80000000u;
    };
    // A paired window (chunks c, c + 1 of pass B with the same dead row): item i < 648 is (stored row r = pixel / 18
    // of 9, channel quad) of chunk c, item 648 + i the same of chunk c + 1; stored row r is the window row
    // pair_window_row(r), the only rows the live Winograd row reads.  Same items per thread and per wave as a whole
    // window, so the same count of loads; the second chunk is part of the vector offset (the halves do not split on
    // a wave boundary).  Aimed only for a tile that has pairs; never used for a load past the tile's last chunk-pass.
    auto aim2 = [&](const Tile& t0) {
      Tile t = t0;
      if (WBM_ABL & 1) { t.n = 0; t.tx = 0; t.ty = 0; }
#pragma unroll
      for (int j = 0; j < NLOAD; ++j) {
        const int i = ht + 256 * j;
        const int half = i >= PAIRITEMS ? 1 : 0;
        const int ii = i - half * PAIRITEMS;
        const int pix = ii >> 2, q = ii & 3;
        const int r = pix / WINW, wx = pix - r * WINW;
        const int gy = t.ty * 16 - 1 + pair_window_row(MODE, r), gx = t.tx * 16 - 1 + wx;
        const bool ok = i < WINITEMS && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W && !(WBM_ABL & 2);
        off2[j] = ok ? (unsigned)(((gy * a.W + gx) * pix_f + 4 * q) * 4) + (unsigned)half * chunk_in_b : 0x80000000u;
      }
    };
    auto dma = [&](int wbuf, int chunk, const unsigned (&off)[NLOAD]) {
      const uintx4 rs = {(unsigned)__builtin_amdgcn_readfirstlane((int)am.rsrc[0]), (unsigned)__builtin_amdgcn_readfirstlane((int)am.rsrc[1]),
                         (unsigned)__builtin_amdgcn_readfirstlane((int)am.rsrc[2]), (unsigned)__builtin_amdgcn_readfirstlane((int)am.rsrc[3])};
      const unsigned soff = (unsigned)chunk * chunk_in_b;
#pragma unroll
      for (int j = 0; j < NLOAD; ++j) {
        const unsigned m0v = lds_base + (unsigned)(STAGEOFF + wbuf * WINB + 16 * (hw * 64 + 256 * j));
        if (j < NLOAD - 1 || ht < WINITEMS - 256 * (NLOAD - 1))   // the last piece: lanes 0..15 of helper wave 0
          asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds"
                       :: "s"(m0v), "v"(off[j]), "s"(rs), "s"(soff) : "memory");
      }
    };
    // number of loads one dma() adds to this wave's vector-memory counter
    const bool last_piece = hw == 0;   // wave-uniform
    auto wait_all_but_newest = [&](int groups) {   // groups = 0, 1 or 2 windows may stay in flight
      if (groups == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      else if (groups == 1) { if (last_piece) asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); }
      else { if (last_piece) asm volatile("s_waitcnt vmcnt(12)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(10)" ::: "memory"); }
    };
    // A paired window is the same 1296 items in the same order (2 x 648), so it adds the same 6 (5) loads per wave.
    static_assert(NLOAD == 6 && 2 * PAIRITEMS == WINITEMS, "the vmcnt immediates above count 6 (5) loads per window, whole or paired");
    // this thread's 4x4 patch inside a staged window: rows 2*pty .. +3, columns 2*ptx .. +3, quad pq
    const int patch0 = ((2 * pty) * WINW + 2 * ptx) * (CK * 4) + pq * 16;
    // Every subtraction of the transform is packed (wino::sub4, wino::pk_sub): 36 issue slots per pass instead of 72.
    auto split_store = [&](floatx4 v, unsigned char* dst) {
      const unsigned h0 = cvt_pk_bf16(v[0], v[1]), h1 = cvt_pk_bf16(v[2], v[3]);
      *(uintx2*)dst = uintx2{h0, h1};
      const floatx2 r01 = wino::pk_sub(floatx2{v[0], v[1]}, floatx2{bf16_lo(h0), bf16_hi(h0)});
      const floatx2 r23 = wino::pk_sub(floatx2{v[2], v[3]}, floatx2{bf16_lo(h1), bf16_hi(h1)});
      *(uintx2*)(dst + PLANEB) = uintx2{cvt_pk_bf16(r01[0], r01[1]), cvt_pk_bf16(r23[0], r23[1])};
    };
    // B^T d B for the two xi rows of a pass: window buffer wbuf -> V buffer vb.  pass A: xi 1 = r1 + r2, xi 2 = r2 - r1
    // (patch rows 1, 2 only); pass B: xi 0 = r0 - r2, xi 3 = r1 - r3.  zxi / znu: the structurally zero Winograd
    // row / column of this chunk (4 = none): never read by the MFMA waves, so neither transformed nor stored.
    auto commit = [&](int wbuf, int vb, bool passB, unsigned zxi, unsigned znu) {
      const unsigned char* src = lds_raw + STAGEOFF + wbuf * WINB + patch0;
      unsigned char* dst = vmine + vb * VBUFB;
      floatx4 xa[4], xb[4];
      bool a_live = true, b_live = true;
      if (!passB) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const floatx4 r1 = *(const floatx4*)(src + (1 * WINW + k) * (CK * 4));
          const floatx4 r2 = *(const floatx4*)(src + (2 * WINW + k) * (CK * 4));
          xa[k] = r1 + r2;
          xb[k] = sub4(r2, r1);
        }
      } else {
        // a dead row (wave-uniform) is neither read nor differenced: all reads of the live rows first
        a_live = zxi != 0u;
        b_live = zxi != 3u;
        floatx4 r0[4], r1[4], r2[4], r3[4];
        if (a_live) {
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            r0[k] = *(const floatx4*)(src + (0 * WINW + k) * (CK * 4));
            r2[k] = *(const floatx4*)(src + (2 * WINW + k) * (CK * 4));
          }
        }
        if (b_live) {
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            r1[k] = *(const floatx4*)(src + (1 * WINW + k) * (CK * 4));
            r3[k] = *(const floatx4*)(src + (3 * WINW + k) * (CK * 4));
          }
        }
        if (a_live) {
#pragma unroll
          for (int k = 0; k < 4; ++k) xa[k] = sub4(r0[k], r2[k]);
        }
        if (b_live) {
#pragma unroll
          for (int k = 0; k < 4; ++k) xb[k] = sub4(r1[k], r3[k]);
        }
      }
      // columns: nu 0: x0-x2, 1: x1+x2, 2: x2-x1, 3: x1-x3
      if (a_live) {
        if (znu != 0) split_store(sub4(xa[0], xa[2]), dst + 0 * POSB);
        split_store(xa[1] + xa[2], dst + 1 * POSB);
        split_store(sub4(xa[2], xa[1]), dst + 2 * POSB);
        if (znu != 3) split_store(sub4(xa[1], xa[3]), dst + 3 * POSB);
      }
      if (b_live) {
        if (znu != 0) split_store(sub4(xb[0], xb[2]), dst + 4 * POSB);
        split_store(xb[1] + xb[2], dst + 5 * POSB);
        split_store(sub4(xb[2], xb[1]), dst + 6 * POSB);
        if (znu != 3) split_store(sub4(xb[1], xb[3]), dst + 7 * POSB);
      }
    };
    auto zero_of = [&](const Tile& t, int k, unsigned& zxi, unsigned& znu) {
      zxi = zero_xi_of(MODE, nchunks, t.item & 3, k);
      znu = zero_nu_of(MODE, nchunks, t.item & 3, k);
    };
    // The live row of the chunks c and c + 1 of pass B from one paired window (aim2): stored rows pty, pty + 1 of
    // each half are the two patch rows the live row reads (xi 0 = r0 - r2, xi 3 = r1 - r3, as in commit); chunk c
    // goes to the row's own V slots, chunk c + 1 to the dead row's (pair_commit_slot).
    auto commit_pair = [&](int wbuf, int vb, const Tile& t, int c) {
      const unsigned char* src = lds_raw + STAGEOFF + wbuf * WINB + (pty * WINW + 2 * ptx) * (CK * 4) + pq * 16;
      unsigned char* dst = vmine + vb * VBUFB;
      floatx4 ra[2][4], rb[2][4];
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          ra[hf][k] = *(const floatx4*)(src + hf * PAIRHALFB + k * (CK * 4));
          rb[hf][k] = *(const floatx4*)(src + hf * PAIRHALFB + (WINW + k) * (CK * 4));
        }
      }
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
        unsigned zxi, znu;
        zero_of(t, c + hf, zxi, znu);
        floatx4 x[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = sub4(ra[hf][k], rb[hf][k]);
        if (znu != 0) split_store(sub4(x[0], x[2]), dst + pair_commit_slot(MODE, hf, 0) * POSB);
        split_store(x[1] + x[2], dst + pair_commit_slot(MODE, hf, 1) * POSB);
        split_store(sub4(x[2], x[1]), dst + pair_commit_slot(MODE, hf, 2) * POSB);
        if (znu != 3) split_store(sub4(x[1], x[3]), dst + pair_commit_slot(MODE, hf, 3) * POSB);
      }
    };
    auto next_ticket = [&]() { return wino::take_ticket(a.ticket); };

    if (ht == 0) {
      post(0, (int)blockIdx.x);
      post(1, next_ticket());
    }
    __syncthreads();  // P0
    Tile cur = read_slot(0);
    int ticket_pre = a.ntiles;
    aim(am, cur);
    const bool pair_on = PAIR && a.pair_b != 0;
    if (pair_on && pfirst_of(cur) < nchunks) aim2(cur);
    dma(0, 0, am.off);
    dma(1, 1, am.off);
    dma(2, 2, am.off);
    if (ht == 0 && read_slot(1).item < a.ntiles) ticket_pre = next_ticket();
    wait_all_but_newest(2);
    __syncthreads();  // P1: the window of chunk 0 has landed (every helper wave has waited for its pieces)
    {
      unsigned zxi, znu;
      zero_of(cur, 0, zxi, znu);
      commit(0, 0, false, zxi, znu);    // V[0] = (cur, pass A, chunk 0)
    }
    wait_all_but_newest(1);             // window of chunk 1
    __syncthreads();  // P
    int wq = 1;                         // window buffer of the chunk-pass transformed in the coming phase
    int s_nxt = 1, s_wr = 2;
    while (cur.item < a.ntiles) {
      const Tile nxt = read_slot(s_nxt);
      const bool more = nxt.item < a.ntiles;
      tile_count++;
      // chunk-passes of this tile: pass A, then pass B with its chunks paired from chunk pfirst on (L is even: the
      // V buffers alternate through the tile boundary, and the loop below runs two phases per turn)
      const int pfirst = pfirst_of(cur);
      const int L = nchunks + pass_b_len(nchunks, pfirst);
      // One phase (chunk-pass sg of this tile; targets past the last one belong to the next tile, whose first three
      // chunk-passes are of its pass A).  Every phase issues the same memory operations whatever the tile: with no
      // next tile the aim points nowhere; a paired window is as many loads as a whole one.
      auto phase = [&](int sg) {
        MSTAMPC(8, sg, 0, 4);
        {
          const int k3 = sg + 3;                                         // window of chunk-pass sg + 3
          if (k3 == L) {   // from here on every load is for the next tile
            if (more) aim(am, nxt); else aim_nowhere(am);
            if (pair_on && more && pfirst_of(nxt) < nchunks) aim2(nxt);
          }
          const int wb3 = wq >= 1 ? wq - 1 : 2;                          // buffer (wq + 2) % 3
          const int jb = k3 - nchunks;                                   // chunk-pass of pass B, if 0 <= jb, k3 < L
          if (PAIR && k3 < L && jb >= pfirst)
            dma(wb3, pass_b_chunk(jb, pfirst), off2);
          else
            dma(wb3, k3 < nchunks ? k3 : k3 < L ? jb : k3 - L, am.off);
        }
        MSTAMPC(8, sg, 1, 4);
        {
          unsigned zxi, znu;                                             // target sg + 1
          const int tg = sg + 1;
          const bool passB = tg >= nchunks && tg < L;
          if (PAIR && passB && tg - nchunks >= pfirst) {
            commit_pair(wq, tg & 1, cur, pass_b_chunk(tg - nchunks, pfirst));
          } else {
            if (tg < L) zero_of(cur, passB ? tg - nchunks : tg, zxi, znu); else zero_of(nxt, 0, zxi, znu);
            commit(wq, tg & 1, passB, zxi, znu);
          }
        }
        wq = wq == 2 ? 0 : wq + 1;
        wait_all_but_newest(1);                                          // window of chunk-pass sg + 2
        MSTAMPC(8, sg, 2, 4);
        __syncthreads();  // B_sg
        MSTAMPC(8, sg, 3, 4);
      };
      if (ht == 0 && more) post(s_wr, ticket_pre);
      for (int sg = 0; sg < L; sg += 2) {
        phase(sg);
        phase(sg + 1);
        if (sg + 2 == nchunks) {   // the MFMA waves fold pass A into pass B's accumulators (exchange through LDS,
          // region B = V buffer 1: not to be written before M4)
          __syncthreads();  // M1
          __syncthreads();  // M2
          __syncthreads();  // M3
          __syncthreads();  // M4
        }
      }
      if (ht == 0 && more && read_slot(s_wr).item < a.ntiles) ticket_pre = next_ticket();
      cur = nxt;
      wino::rotate_ring(s_nxt, s_wr);
    }
#if WBM_STAMP
    if (wave == 8) {
      wbm_stamps[blockIdx.x * 384 + 128 + lane] = (long long)((unsigned*)(lds_raw + STAMPOFF))[128 + lane];
      wbm_stamps[blockIdx.x * 384 + 192 + lane] = (long long)((unsigned*)(lds_raw + STAMPOFF))[192 + lane];
    }
#endif
    if (ht == 0) wino::rearm_ticket(a.ticket);
    return;
  }

  // ===================================== MFMA waves ==============================================
  const int h = lane >> 5, l31 = lane & 31;
  const int nt = wave & 3, pqw = wave >> 2;
  const bool nvalid = nt * 32 < a.CoutP;
  constexpr bool ZSKIP = MODE != 0;
  // U stream: [phase][pos 16][chunk][plane][CoutP][16 bf16]; a fragment = 64 lanes x 16 bytes
  const unsigned plane_b = (unsigned)a.CoutP * 32u;
  const unsigned chunk_b = plane_b * (unsigned)P;
  const unsigned pos_b = chunk_b * (unsigned)nchunks;
  const unsigned ulane = (unsigned)((((nvalid ? nt : 0) * 32 + l31) * 2 + h) * 16);
  // V reads: row l31 (+ 32 m) of a position, k-block h (swizzled)
  const int aread = l31 * ROWB + ((h ^ ((l31 >> 3) & 1)) << 4);
  // exchange slots: [region][wave][quarter 4][lane][4 floats].  Addresses are rebuilt where they are used (from a
  // laundered lane id: the compiler would otherwise keep half a dozen tile-invariant address registers alive
  // through the MFMA loops, which have 16 registers to spare).
  auto xaddr = [&](bool region_b, bool partner) {
    const int ln = lane_now();
    return lds_raw + (region_b ? VBUFB : XOFF) + ((partner ? wave ^ 4 : wave) * 4096) + ln * 16;
  };
#define xa_mine xaddr(false, false)
#define xa_part xaddr(false, true)
#define xb_mine xaddr(true, false)
#define xb_part xaddr(true, true)
  auto xwrite = [&](unsigned char* p, const floatx16& v) {
#pragma unroll
    for (int q = 0; q < 4; ++q) *(floatx4*)(p + q * 1024) = floatx4{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
  };
  auto xread = [&](const unsigned char* p) {
    floatx16 v;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const floatx4 x = *(const floatx4*)(p + q * 1024);
      v[4 * q] = x[0]; v[4 * q + 1] = x[1]; v[4 * q + 2] = x[2]; v[4 * q + 3] = x[3];
    }
    return v;
  };
  // output addressing (bytes): pixel of Winograd tile (ty, tx) of the workgroup tile, output (i, j) of that tile
  //   = tbase + ty*SY + tx*SX + i*SI + j*SJ + channel offset (NHWC: channel*4)
  // Chunk-major output (a.cm_out, [B][C/16][OH][OW][16]): a pixel is 64 bytes of its chunk's plane, the channel
  // offset is (channel/16)*plane + (channel%16)*4, and the space-to-depth block (j, i) is a channel offset of
  // Cout/16 (2 Cout/16) planes.
  const int OHW = a.nphase == 4 ? 4 * a.H * a.W : a.s2d ? (a.H >> 1) * (a.W >> 1) : a.H * a.W;   // output pixels
  const int PB = a.cm_out ? CK * 4 : a.ostride * 4;                    // bytes per output pixel (of a chunk's plane)
  int SJ, SI;
  if (a.nphase == 4) {
    SJ = 2 * PB;
    SI = 2 * (2 * a.W) * PB;
  } else if (a.s2d) {
    SJ = a.cm_out ? (a.Cout / CK) * OHW * (CK * 4) : a.Cout * 4;
    SI = 2 * SJ;
  } else {
    SJ = PB;
    SI = a.W * PB;
  }
  const int SX = a.nphase == 4 ? 2 * SJ : a.s2d ? (a.cm_out ? PB : 4 * a.Cout * 4) : 2 * SJ;
  const int SY = a.nphase == 4 ? 2 * SI : a.s2d ? (a.W >> 1) * SX : 2 * SI;

  auto mfma_waves = [&](auto pq_tag) {
  constexpr int PQ = decltype(pq_tag)::value;
  floatx16 acc[8];   // [step 4][m 2]
  bf16x8 Bq[RING][P];
  __syncthreads();  // P0
  __syncthreads();  // P1
  __syncthreads();  // P
  Tile cur = read_slot(0);
  const __amdgpu_buffer_rsrc_t urs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)a.u, 0, (int)(16u * pos_b * (unsigned)a.nphase), 0x00020000);
  auto soff_item = [&](const Tile& t) { return wb::soff_item(t, a.nphase, a.u_phase_bytes, nchunks, chunk_b); };
  unsigned soff_phase = soff_item(cur);
  auto fetch = [&](bf16x8 (&dst)[P], unsigned so) { wb::fetch_u(dst, urs, ulane, so, plane_b); };
#pragma unroll
  for (int f = 0; f < RING; ++f) fetch(Bq[f], soff_phase + (unsigned)gpos<MODE, 0, PQ>(f) * pos_b);
  int s_nxt = 1;
  while (cur.item < a.ntiles) {
    tile_count++;
#if WBM_STAMP
    if (lane == 0 && wave == 4 * PQ && tile_count == 3) ((unsigned*)(lds_raw + STAMPOFF))[(PQ ? 256 : 0) + 127] = (unsigned)cur.item;
#endif
    const Tile nxt = read_slot(s_nxt);
    const unsigned soff_phase_nxt = soff_item(nxt.item < a.ntiles ? nxt : cur);
    // MODE 2: the phase's zero row / column, for the whole tile.  zero_xi_of / zero_nu_of (conv_wino_pair.h), kept
    // local: read from there, the MFMA schedule of the MODE 2 instances and operand orders in the others move.
    unsigned tzero_xi = 4, tzero_nu = 4;
    if (MODE == 2) {
      const int phase = cur.item & 3;
      if (phase >> 1) tzero_xi = 0;
      if (phase & 1) tzero_nu = 0;
    }
    // one chunk of one pass: 4 steps x (U fragment pair from the ring; per M tile: V pair from LDS, 3 MFMAs)
    auto chunk_body = [&](auto pass_tag, auto first_tag, int chunk) {
      constexpr int PASS = decltype(pass_tag)::value;
      constexpr bool FIRST = decltype(first_tag)::value;
      const bool last = chunk + 1 == nchunks;
      MSTAMPC(4 * PQ, PASS * nchunks + chunk, 0, 3);
      unsigned zero_xi = tzero_xi, zero_nu = tzero_nu;
      if (MODE == 1) {
        zero_xi = zero_xi_of(MODE, nchunks, 0, chunk);
        zero_nu = zero_nu_of(MODE, nchunks, 0, chunk);
      }
      auto is_zero = [&](int s) {
        const int g = gpos<MODE, PASS, PQ>(s);
        return (unsigned)(g >> 2) == zero_xi || (unsigned)(g & 3) == zero_nu;
      };
      const unsigned char* vb = lds_raw + ((PASS * nchunks + chunk) & 1) * VBUFB + aread;
      auto vaddr = [&](int sub, int q) {   // sub = 2*s + m
        return vb + lpos_of<PASS>(gpos<MODE, PASS, PQ>(sub >> 1)) * POSB + (sub & 1) * (32 * ROWB) + q * PLANEB;
      };
      bf16x8 Aq[P];
#pragma unroll
      for (int q = 0; q < P; ++q) Aq[q] = *(const bf16x8*)vaddr(0, q);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const bool live = !ZSKIP || !is_zero(s);  // wave-uniform
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          const int sub = 2 * s + m;
          if (live) {
            const floatx16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            floatx16 c = FIRST ? zero : acc[sub];
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Aq[0], Bq[s % RING][1], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Aq[1], Bq[s % RING][0], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Aq[0], Bq[s % RING][0], c, 0, 0, 0);
            acc[sub] = c;
          } else if (FIRST) {
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[sub][e] = 0.f;
          }
          // V of the next sub-step, issued right behind the MFMAs that read the current one
          if (sub + 1 < 8) {
#pragma unroll
            for (int q = 0; q < P; ++q) Aq[q] = *(const bf16x8*)vaddr(sub + 1, q);
          }
        }
        {
          // refill this ring slot with the fragments of step s + RING (the next chunk's first steps past 3).  Not
          // across a fold: the ring is refilled behind it, so that its 16 registers are free for the fold
          const int f = s + RING;
          const unsigned so = f < 4 ? soff_phase + (unsigned)gpos<MODE, PASS, PQ>(f) * pos_b + (unsigned)chunk * chunk_b
                                    : soff_phase + (unsigned)gpos<MODE, PASS, PQ>(f - 4) * pos_b + (unsigned)(chunk + 1) * chunk_b;
          if (f < 4 ? !(ZSKIP && is_zero(f)) : !last) fetch(Bq[s % RING], so);
        }
      }
      MSTAMPC(4 * PQ, PASS * nchunks + chunk, 1, 3);
      __syncthreads();  // B_sigma
      MSTAMPC(4 * PQ, PASS * nchunks + chunk, 2, 3);
    };
    // One paired chunk-pass of pass B (chunk-pass j: the chunks chunk, chunk + 1), for the wave half that owns the
    // live row: eight steps into the four positions of the row - chunk's four, then those of chunk + 1, whose V
    // lies in the dead row's slots (conv_wino_pair.h).  The ring runs on through both chunks and into the next pair.
    auto pair_body = [&](int j, int chunk) {
      const bool last = chunk + 2 == nchunks;
      MSTAMPC(4 * PQ, nchunks + j, 0, 3);
      auto is_zero = [&](int s) {   // the owner's row is live: the chunk's zero column only
        return (unsigned)(pair_gpos<MODE, PQ>(s) & 3) == zero_nu_of(MODE, nchunks, cur.item & 3, chunk + pair_half(s));
      };
      const unsigned char* vb = lds_raw + (j & 1) * VBUFB + aread;
      auto vaddr = [&](int sub, int q) {   // sub = 2*s + m
        return vb + pair_vslot<MODE, PQ>(sub >> 1) * POSB + (sub & 1) * (32 * ROWB) + q * PLANEB;
      };
      bf16x8 Aq[P];
#pragma unroll
      for (int q = 0; q < P; ++q) Aq[q] = *(const bf16x8*)vaddr(0, q);
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const bool live = !is_zero(s);  // wave-uniform
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          const int sub = 2 * s + m, ai = 2 * pair_acc(s) + m;
          if (live) {
            floatx16 c = acc[ai];
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Aq[0], Bq[s % RING][1], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Aq[1], Bq[s % RING][0], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Aq[0], Bq[s % RING][0], c, 0, 0, 0);
            acc[ai] = c;
          }
          if (sub + 1 < 16) {
#pragma unroll
            for (int q = 0; q < P; ++q) Aq[q] = *(const bf16x8*)vaddr(sub + 1, q);
          }
        }
        {
          const int f = s + RING;   // steps 8, 9: the first two of the next pair
          const unsigned so = soff_phase + (unsigned)pair_gpos<MODE, PQ>(f & 7) * pos_b +
                              (unsigned)(chunk + (f < 8 ? pair_half(f) : 2)) * chunk_b;
          if (f < 8 ? !is_zero(f) : !last) fetch(Bq[s % RING], so);
        }
      }
      MSTAMPC(4 * PQ, nchunks + j, 1, 3);
      __syncthreads();  // B_sigma
      MSTAMPC(4 * PQ, nchunks + j, 2, 3);
    };

    // ---------------------------------- pass A ------------------------------------------------
    chunk_body(std::integral_constant<int, 0>{}, std::true_type{}, 0);
    for (int chunk = 1; chunk < nchunks; ++chunk) chunk_body(std::integral_constant<int, 0>{}, std::false_type{}, chunk);
    // ---- fold pass A into the corner positions of pass B ---------------------------------------
    {
      // own row xi = 1 + PQ: M[nu][m] = acc[2 * step(nu) + m]; C[0] = M0 + M1 + M2, C[1] = M1 - M2 - M3
      constexpr int XI = 1 + PQ;
      constexpr int s0 = step_of<MODE, 0, PQ>(XI * 4 + 0), s1 = step_of<MODE, 0, PQ>(XI * 4 + 1);
      constexpr int s2 = step_of<MODE, 0, PQ>(XI * 4 + 2), s3 = step_of<MODE, 0, PQ>(XI * 4 + 3);
      floatx16 c0[2], c1[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        c0[m] = (acc[2 * s0 + m] + acc[2 * s1 + m]) + acc[2 * s2 + m];
        c1[m] = (acc[2 * s1 + m] - acc[2 * s2 + m]) - acc[2 * s3 + m];
      }
      // pass B: this wave owns row xi = 0 (PQ 0) or 3 (PQ 1); its corner positions nu = 0, 3 start from
      //   (0,0) = P[0][0] = C1[0] + C2[0]    (0,3) = -P[0][1] = -(C1[1] + C2[1])
      //   (3,0) = -P[1][0] = C2[0] - C1[0]   (3,3) = P[1][1] = C1[1] - C2[1]          (C1: row 1 = PQ 0, C2: row 2 = PQ 1)
      constexpr int XB = PQ == 0 ? 0 : 3;
      constexpr int t0 = step_of<MODE, 1, PQ>(XB * 4 + 0), t1 = step_of<MODE, 1, PQ>(XB * 4 + 1);
      constexpr int t2 = step_of<MODE, 1, PQ>(XB * 4 + 2), t3 = step_of<MODE, 1, PQ>(XB * 4 + 3);
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        xwrite(xa_mine, c0[m]);
        xwrite(xb_mine, c1[m]);
        MSTAMP(4 * PQ, 122 + 2 * m);
        __syncthreads();  // M1 / M3
        MSTAMP(4 * PQ, 123 + 2 * m);
        const floatx16 g0 = xread(xa_part), g1 = xread(xb_part);
        if (PQ == 0) {
          acc[2 * t0 + m] = c0[m] + g0;
          acc[2 * t3 + m] = -(c1[m] + g1);
        } else {
          acc[2 * t0 + m] = c0[m] - g0;
          acc[2 * t3 + m] = g1 - c1[m];
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          acc[2 * t1 + m][e] = 0.f;
          acc[2 * t2 + m][e] = 0.f;
        }
        __syncthreads();  // M2 / M4: both regions have been read (M4: V buffer 1 belongs to the helpers again)
      }
      MSTAMP(4 * PQ, 126);
    }
#pragma unroll
    for (int f = 0; f < RING; ++f) fetch(Bq[f], soff_phase + (unsigned)gpos<MODE, 1, PQ>(f) * pos_b);
    // ---------------------------------- pass B ------------------------------------------------
    // single chunks up to pfirst, then pairs: the wave half that owns the dead row only joins their barriers
    const int pfirst = pfirst_of(cur);
    for (int chunk = 0; chunk < pfirst; ++chunk) chunk_body(std::integral_constant<int, 1>{}, std::false_type{}, chunk);
    if constexpr (PAIR) {
      for (int j = pfirst; j < pass_b_len(nchunks, pfirst); ++j) {
        if constexpr (PQ == pair_owner(MODE)) {
          pair_body(j, pass_b_chunk(j, pfirst));
        } else {
          MSTAMPC(4 * PQ, nchunks + j, 0, 3);
          MSTAMPC(4 * PQ, nchunks + j, 1, 3);
          __syncthreads();  // B_sigma
          MSTAMPC(4 * PQ, nchunks + j, 2, 3);
        }
      }
    }
    soff_phase = soff_phase_nxt;

    // ---- final fold: output row i = PQ from the wave's own row; bias + activation; stores --------
    // Y[0][0] = M00 + M01 + M02, Y[0][1] = M01 - M02 - M03 (row 0); Y[1][j] = -(the same of row 3).  No exchange and
    // no barrier: every wave transposes its outputs through its own 4 KB of region A (lane = channel -> lane = channel
    // quad of a tile) and stores 16 bytes per lane, 8 pixels x 128 bytes per instruction.
    MSTAMP(4 * PQ, 120);
    {
      const int phase = cur.item & (a.nphase - 1);
      const int ppy = phase >> 1, ppx = phase & 1;
      const int OH = a.nphase == 4 ? 2 * a.H : a.H, OW = a.nphase == 4 ? 2 * a.W : a.W;
      const __amdgpu_buffer_rsrc_t ors = __builtin_amdgcn_make_buffer_rsrc(
          (void*)(a.out + (size_t)cur.n * OH * OW * a.ostride + a.ooff), 0, (OH * OW * a.ostride - a.ooff) * 4, 0x00020000);
      const unsigned tbase =
          a.nphase == 4 ? (unsigned)(((32 * cur.ty + ppy) * OW + 32 * cur.tx + ppx) * PB)
          : a.s2d       ? (unsigned)(((8 * cur.ty) * (a.W >> 1) + 8 * cur.tx) * SX)
                        : (unsigned)((16 * cur.ty * a.W + 16 * cur.tx) * PB);
      constexpr int XB = PQ == 0 ? 0 : 3;
      constexpr int t0 = step_of<MODE, 1, PQ>(XB * 4 + 0), t1 = step_of<MODE, 1, PQ>(XB * 4 + 1);
      constexpr int t2 = step_of<MODE, 1, PQ>(XB * 4 + 2), t3 = step_of<MODE, 1, PQ>(XB * 4 + 3);
      // transposition area of this wave: [tile row 32][32 channels] floats
      const int ln = lane_now();   // (see xaddr)
      float* const tw = (float*)(lds_raw + XOFF + wave * 4096) + ln + 96 * (ln >> 5);   // lane (h, l31) -> row 4 h, channel l31: 128 h + l31; + row(e) * 32
      const float* const tr = (const float*)(lds_raw + XOFF + wave * 4096) + ln * 4;   // row lane >> 3, quad lane & 7: 32 (lane >> 3) + 4 (lane & 7) = 4 lane; + k * 256
      const float* const prm = (const float*)(lds_raw + PARAMOFF) + nt * 32 + (ln & 31);
      const float pbias = prm[0], pbeta = prm[128], pgamma = prm[256];
      const int cq = nt * 32 + (ln & 7) * 4;     // first channel of this lane's quad
      const int cqoff = a.cm_out ? (cq >> 4) * OHW * (CK * 4) + (cq & 15) * 4 : cq * 4;
      const unsigned svoff = cq < a.Cout ? (unsigned)((ln >> 3) * SX + cqoff) : 0x80000000u;
      auto emit = [&](auto act_tag, int m, int j, floatx16 y) {
        constexpr int ACT = decltype(act_tag)::value;
#pragma unroll
        for (int e = 0; e < 16; e += 2) {
          const floatx2 v = wino::bias_act<ACT>(floatx2{y[e], y[e + 1]}, pbias, pbeta, pgamma);
          const float v0 = v[0], v1 = v[1];
          tw[((e & 3) + 8 * (e >> 2)) * 32] = v0;
          tw[(((e + 1) & 3) + 8 * ((e + 1) >> 2)) * 32] = v1;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the reads below must see this wave's writes
        // tile rows 8k .. 8k+7 = Winograd tiles (ty = 4 m + k, tx = lane >> 3).  All four reads first, into registers
        // of their own; the address goes into the vector offset (no SGPR offset) and the stores are followed by wait
        // states: on this hardware a 16-byte buffer store with an SGPR offset reads its data registers tens of cycles
        // after it has issued, and neither the hardware nor the compiler (which knows the hazard for immediate offsets
        // only) keeps the next instructions from overwriting them - measured: the first registers of the last store of
        // an emit took the next emit's first products in a quarter of the lanes, under load only.
        floatx4 o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = *(const floatx4*)(tr + k * 256);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const unsigned so = tbase + (unsigned)((4 * m + k) * SY + PQ * SI + j * SJ);
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(uintx4, o[k]), ors, svoff + so, 0, NT_OUT ? 2 : 0);
        }
        asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15" ::: "memory");
      };
      auto emit_act = [&](int m, int j, const floatx16& y) {
        wino::for_act(a.act, [&](auto act_tag) { emit(act_tag, m, j, y); });
      };
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const floatx16 y0 = (acc[2 * t0 + m] + acc[2 * t1 + m]) + acc[2 * t2 + m];
        const floatx16 y1 = (acc[2 * t1 + m] - acc[2 * t2 + m]) - acc[2 * t3 + m];
        emit_act(m, 0, PQ == 0 ? y0 : -y0);
        emit_act(m, 1, PQ == 0 ? y1 : -y1);
      }
    }
    MSTAMP(4 * PQ, 121);
#pragma unroll
    for (int f = 0; f < RING; ++f) fetch(Bq[f], soff_phase + (unsigned)gpos<MODE, 0, PQ>(f) * pos_b);
    cur = nxt;
    s_nxt = wino::step_ring(s_nxt);
  }
#if WBM_STAMP
  if (wave == 0 || wave == 4) {   // slot 127: the item of the stamped tile
    unsigned* const st = (unsigned*)(lds_raw + STAMPOFF) + (wave == 0 ? 0 : 256);
    wbm_stamps[blockIdx.x * 384 + (wave == 0 ? 0 : 256) + lane] = (long long)st[lane];
    wbm_stamps[blockIdx.x * 384 + (wave == 0 ? 0 : 256) + 64 + lane] = (long long)st[64 + lane];
  }
#endif
  };
  if (pqw == 0)
    mfma_waves(std::integral_constant<int, 0>{});
  else
    mfma_waves(std::integral_constant<int, 1>{});
}

#undef xa_mine
#undef xa_part
#undef xb_mine
#undef xb_part

}  // namespace wbm
}  // namespace dsic

using namespace dsic;

// Which layers take this kernel: a function of the layer geometry only (never of the batch size: a patch's bits
// must not depend on the batch it is in).  H and W multiples of 16 (no ragged tiles: the stores are unmasked) and
// at least 4 work items per image (32x32 outputs; ConvTranspose2d: 16x16 inputs).
extern "C" int dsic_wino_bf16_m64(int H, int W, int Cin, int nphase) {
  static int mode = -1;   // DSIC_WINO_M64=0: never (A/B runs)
  if (mode < 0) {
    const char* e = getenv("DSIC_WINO_M64");
    mode = e ? atoi(e) : 1;
  }
  if (!mode) return 0;
  if (H <= 0 || W <= 0 || H % 16 || W % 16 || Cin < 64 || Cin % 32) return 0;
  const int min_items = mode > 1 ? mode : 4;
  return (H / 16) * (W / 16) * nphase >= min_items;
}

// Pairing of the half-empty pass-B chunks (conv_wino_pair.h): on unless DSIC_WINO_PAIR=0 (read once; A/B runs), or
// switched by dsic_wino_pair_chunks (tests compare the two schedules in one process).
static int wbm_pair_mode() {
  static int mode = -1;
  if (mode < 0) {
    const char* e = getenv("DSIC_WINO_PAIR");
    mode = e ? (atoi(e) != 0) : 1;
  }
  return mode;
}
static int wbm_pair_override = -1;
extern "C" int dsic_wino_pair_chunks(int on) {
  const int was = wbm_pair_override >= 0 ? wbm_pair_override : wbm_pair_mode();
  if (on >= 0) wbm_pair_override = on != 0;
  return was;
}

// Host restatement of a tile's schedule from the same tables the kernel reads: the (chunk, position xi*4 + nu)
// pairs that accumulator acc (0..3) of wave half pq receives in pass B, in order, for the paired or the unpaired
// schedule.  out: up to cap pairs of ints; returns their number (-1: bad arguments).
namespace {
template <int MODE, int PQ>
int pass_b_sequence(int nchunks, int phase, bool paired, int acc, int* out, int cap) {
  using namespace dsic::wbm;
  int n = 0;
  auto put = [&](int chunk, int g) {
    if (n < cap) {
      out[2 * n] = chunk;
      out[2 * n + 1] = g;
    }
    ++n;
  };
  auto live = [&](int chunk, int g) {
    return (unsigned)(g >> 2) != zero_xi_of(MODE, nchunks, phase, chunk) && (unsigned)(g & 3) != zero_nu_of(MODE, nchunks, phase, chunk);
  };
  const int pfirst = MODE == 0 ? nchunks : pair_first(MODE, nchunks, phase, paired);
  for (int j = 0; j < pass_b_len(nchunks, pfirst); ++j) {
    const int c = pass_b_chunk(j, pfirst);
    if (j < pfirst) {
      for (int s = 0; s < 4; ++s)
        if (s == acc && live(c, gpos<MODE, 1, PQ>(s))) put(c, gpos<MODE, 1, PQ>(s));
    } else if (PQ == pair_owner(MODE)) {
      for (int s = 0; s < 8; ++s) {
        const int g = pair_gpos<MODE, PQ>(s), cc = c + pair_half(s);
        // the V slot the MFMA wave reads is the one the helpers commit this (chunk, position) to
        if (pair_vslot<MODE, PQ>(s) != pair_commit_slot(MODE, pair_half(s), g & 3) || (g >> 2) != pair_live_xi(MODE)) return -2;
        if (pair_acc(s) == acc && live(cc, g)) put(cc, g);
      }
    } else {
      // the other half issues nothing in a paired chunk-pass: its row must be dead in both chunks
      for (int h = 0; h < 2; ++h)
        for (int s = 0; s < 4; ++s)
          if (live(c + h, gpos<MODE, 1, PQ>(s))) return -3;
    }
  }
  return n;
}
}  // namespace
extern "C" int dsic_wino_pair_schedule(int mode, int nchunks, int phase, int paired, int pq, int acc, int* out, int cap) {
  if (mode < 0 || mode > 2 || nchunks < 4 || nchunks % 2 || phase < 0 || phase > 3 || pq < 0 || pq > 1 || acc < 0 || acc > 3 ||
      (cap > 0 && !out))
    return -1;
#define WBM_SEQ(M, Q) pass_b_sequence<M, Q>(nchunks, phase, paired != 0, acc, out, cap)
  switch (mode * 2 + pq) {
    case 0: return WBM_SEQ(0, 0);
    case 1: return WBM_SEQ(0, 1);
    case 2: return WBM_SEQ(1, 0);
    case 3: return WBM_SEQ(1, 1);
    case 4: return WBM_SEQ(2, 0);
    default: return WBM_SEQ(2, 1);
  }
#undef WBM_SEQ
}

// wb_launch (conv_wino_bf16.hip) has checked the layer and chosen this kernel for it; what is left is the 64-tile
// kernel's own: 16x16-pixel tiles, the pass-B pairing, its instances and its launch.
int dsic_wbm_launch(wb::Args& a, hipStream_t st) {
  a.tiles_x = a.W / 16;
  a.tiles_y = a.H / 16;
  a.ntiles = a.tiles_x * a.tiles_y * a.B * a.nphase;   // no more than the 16x8-pixel tiles wb_launch has counted
  a.pair_b = dsic_wino_pair_chunks(-1);
  using wbm::conv_wino_bf16m_kernel;
  static wino_host::Family<6> family = {
      "conv_wino_bf16m", wbm::THREADS, wbm::LDS_TOTAL,   // MODE + 3 * NT_OUT
      {(const void*)conv_wino_bf16m_kernel<0, false>, (const void*)conv_wino_bf16m_kernel<1, false>,
       (const void*)conv_wino_bf16m_kernel<2, false>, (const void*)conv_wino_bf16m_kernel<0, true>,
       (const void*)conv_wino_bf16m_kernel<1, true>, (const void*)conv_wino_bf16m_kernel<2, true>}};
  return wino_host::launch(family, 3 * a.nt_out + (a.s2d_in ? 1 : a.nphase == 4 ? 2 : 0), a.ntiles, a, st);
}

#if WBM_STAMP
extern "C" int dsic_debug_wbm_stamps(long long* host_out) {   // [256 workgroups][384]
  return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(wbm::wbm_stamps), sizeof(long long) * 256 * 384) == hipSuccess ? 0 : 2;
}
#endif
