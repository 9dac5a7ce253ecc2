// Winograd F(2x2,3x3) fp32 convolution for the 3x3 stride-1 layers
// (conv(N,N,3,1) at code/modelv2/layers.py:56,62,67,86,90,94,108,109) with the
// same fused bias + GDN/IGDN/ReLU epilogue as conv_igemm.hip.
//
// Y = A^T [ sum_c (G g G^T) o (B^T d B) ] A needs 16 multiplies per 2x2 output
// tile and channel pair instead of 36: 2.25x fewer MFMA flops for the layers
// that hold 35 % of the model's MACs, at fp32 accuracy (the transforms only add,
// subtract and halve).  It is the same exact-fp32 MFMA instruction; only the
// summation order differs from a direct convolution.
//
// Persistent workgroups (one per CU) of 768 threads over output tiles of 16x8 pixels (= 8x4
// Winograd tiles = the 32 rows of one MFMA M tile).  The 16 Winograd positions are 16 independent
// GEMMs  D_p[32 tiles][Cout] += V_p[32][Cin] U_p[Cin][Cout].
//   waves 0..7  (MFMA waves): wave w owns column tile nt = w&3 (32 output channels) and positions
//               8*(w>>2) .. +7: 8 accumulators of 32x32 = 128 VGPRs, two such waves per SIMD.  Their
//               loop reads V from LDS and U (transformed weights, packed [pos][Cin/8][CoutP][8], L2)
//               and issues MFMAs, nothing else.
//   waves 8..11 (helpers, one per SIMD): load the NHWC input (16 float4 per thread and 32-channel
//               chunk, one chunk ahead), apply B^T d B and write V into the double-buffered LDS image
//               [pos][tile][36]; after a tile they copy the finished 2x2 outputs (folded and activated
//               by the MFMA waves inside the V buffer that has just been consumed) to HBM, 16 bytes
//               per lane.
// See DESIGN.md section 3 for the reasons (in-order vmcnt, VALU issue under MFMA) and the numbers.
#include <stdlib.h>

#include "wino_device.h"
#include "wino_host.h"

#ifndef WINO_STAMP
#define WINO_STAMP 0
#endif
#ifndef WINO_ABL
#define WINO_ABL 0  // diagnostic ablations (wrong results): 1 no epilogue call, 2 no transform/V stores, 4 no input loads, 8 no fold
#endif
#ifndef WINO_STAMP_CHUNK0
#define WINO_STAMP_CHUNK0 0  // first of the four chunks whose MFMA phases are stamped
#endif
#ifndef WINO_STAMP_TILE
#define WINO_STAMP_TILE 16  // which tile of a workgroup is stamped
#endif

namespace dsic {

using wino::sub16;
using wino::sub4;
using wino::Tile;  // a work item (tile*nphase + phase) and its 16x8-pixel tile coordinates

struct WinoArgs {
  const float* in;
  const float* u;  // [16][Cin/8][CoutP][8]
  const float* bias;
  const float* beta;
  const float* gamma;
  float* out;
  int B, H, W, Cin, Cout, CoutP;
  int act;
  unsigned long long* ticket;  // two counters, zeroed once by the caller (wino_device.h)
  int nphase;  // 1, or 4: ConvTranspose2d(5,2,2,1) as four 3x3 sub-pixel phase convs sharing the input;
               // work item w = spatial tile*4 + phase, U of phase p at u + p*u_phase_stride, output pixel
               // (2*oy+py, 2*ox+px) of a [B,2H,2W,Cout] tensor
  int64_t u_phase_stride;
  int s2d_in;  // input is the space-to-depth image of a 5x5/s2 layer: Cin = 4*Cs, channel block (a,b)
  int s2d;  // store space-to-depth: [B,H/2,W/2,4*Cout] (feeds a 5x5/s2 layer run as 3x3 over 4*C)
  int tiles_x, tiles_y, ntiles;  // 16x8-pixel output tiles
  int nt_out;  // stream the output past the caches (set by the host for outputs beyond the MALL's size)
};

#if WINO_STAMP
__device__ long long wino_stamps[256 * 32];
// cycle stamps go to LDS (a global store would sit in the wave's in-order vmcnt queue and perturb
// what is measured) and are copied out when the workgroup ends
#define STAMP_AT(w, i)                                                                            \
  do {                                                                                            \
    __builtin_amdgcn_sched_barrier(0); /* s_memtime does not depend on the MFMAs around it */   \
    if (WINO_STAMP && lane == 0 && wave == (w) && tile_count == WINO_STAMP_TILE)                  \
      ((long long*)(lds + 2 * WBUF + 16))[i] = __builtin_amdgcn_s_memtime();                      \
    __builtin_amdgcn_sched_barrier(0);                                                            \
  } while (0)
#define STAMP(i) STAMP_AT(0, i)
#else
#define STAMP(i)
#endif

constexpr int WCK = 32;                    // channels per chunk
constexpr int WP = WCK + 4;                // LDS floats per (pos, tile) row
constexpr int WBUF = 16 * 32 * WP;         // floats per V buffer
constexpr int WLDS_BYTES = 2 * WBUF * 4;   // 147456
constexpr int WLDS_TOTAL = WLDS_BYTES + 64 + (WINO_STAMP ? 256 : 0);  // + three tile-descriptor slots (+ 32 stamps)
constexpr int WTHREADS = 768;              // 8 MFMA waves + 4 helper waves
#ifndef WINO_RING
#define WINO_RING 4                        // U fragments in flight per MFMA wave (2 or 4)
#endif
#ifndef WINO_CPRIO
#define WINO_CPRIO 1                       // wave priority of an MFMA wave inside an MFMA cluster
#endif
#ifndef WINO_HPRIO
#define WINO_HPRIO 0                       // wave priority of the helper waves
#endif

__device__ __forceinline__ void wg_barrier() { __syncthreads(); }

// MODE 0: plain 3x3 layer.  MODE 1 (space-to-depth input) and MODE 2 (ConvTranspose2d phases) have
// structurally zero Winograd positions whose MFMA clusters are skipped; MODE 0 carries no test in
// the loop.  Steps run position-major (all four 8-channel groups of a position, then the next
// position), MODE 2 from position 7 down: the positions that can be zero then sit mostly at the
// end of a chunk, where the operand prefetch of the skipped steps runs into the chunk barrier
// instead of stalling the next live step (a skipped step takes no time, so the U fragments of the
// steps behind it have had no time to arrive).
//
// Wave specialisation.  Waves 0..7 ("MFMA waves") only read operands and issue MFMAs; waves 8..11
// ("helpers", one per SIMD) load the NHWC input, apply B^T d B and fill the other LDS buffer.
// vmcnt retires in order, so a wave that mixes HBM-latency input loads with the L2-latency U
// stream stalls its MFMAs behind the slowest input load; separate waves have separate counters.
// 12 waves = 3 per SIMD: the kernel must fit 168 VGPRs (128 of them accumulators).
// The MFMA waves fold their accumulators into the 2x2 outputs inside the free V buffer (bias and
// activation fused into the fold's second half) and go on to the next tile; the helpers copy the
// finished outputs to HBM from there, behind the next chunk's input loads.
// Every wave executes the same barrier sequence: P0, P, then per tile B_0..B_{n-1}, E1, E2.
//
// Tiles are handed out dynamically through a 3-slot LDS ring: wino_device.h.
template <int MODE>
__global__ __launch_bounds__(WTHREADS) void conv_wino_kernel(const WinoArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  float* slots = lds + 2 * WBUF;  // written before a workgroup barrier, read after it
  auto read_slot = [&](int s) { return wino::read_tile<false>(slots, s); };
  const int pshift = a.nphase == 4 ? 2 : 0;

  if (wave >= 8) {
    // =================================== helper waves ===========================================
    // thread = (Winograd tile pt, channel quad pq): the whole 4x4 pixel patch, 16 float4 loads
    // (8 adjacent lanes = 128 contiguous bytes), all 16 positions.
    __builtin_amdgcn_s_setprio(WINO_HPRIO);
    const int ht = tid - 512;
    const int Cin = a.Cin;
    const int nchunks = Cin / WCK;
    const int pt = ht >> 3, pq = ht & 7;
    const int ptx = pt & 7, pty = pt >> 3;
    const int vwrite = pt * WP + 4 * pq;  // + pos*32*WP
    auto post = [&](int s, int item) { wino::post_tile(slots, s, item, 0, pshift, a.tiles_x, a.tiles_y); };
    // Input side, in three steps so that the loads of the next chunk can be put in flight before
    // the helper waits at a barrier (a helper only gets issue slots while the MFMA waves idle: the
    // SIMD issues one VALU-class instruction at a time and a pending MFMA holds the port):
    //   aim(tile)    per-thread byte offsets of the 16 patch pixels inside the image, once per tile
    //   issue(chunk) 16 float4 loads of the aimed tile's chunk
    //   commit(vbuf) B^T d B and the 16 stores into the V buffer
    // Input loads are raw buffer loads: descriptor (image base, image bytes) + one 32-bit byte offset
    // per patch pixel + the chunk as scalar offset, i.e. no address arithmetic per load, and a pixel
    // outside the image gets an offset beyond the descriptor's range, which the hardware reads as 0.
    struct Aim {
      unsigned off[16];  // byte offsets of the 16 patch pixels inside the image (+ this thread's channel quad)
      __amdgpu_buffer_rsrc_t rsrc;  // uniform
    };
    auto aim = [&](Aim& m, const Tile& t) {
      const int gy0 = t.ty * 8 + 2 * pty - 1, gx0 = t.tx * 16 + 2 * ptx - 1;
      m.rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(a.in + (size_t)t.n * a.H * a.W * Cin), 0,
                                                 a.H * a.W * Cin * 4, 0x00020000);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int gy = gy0 + i;
        const bool yok = gy >= 0 && gy < a.H;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int gx = gx0 + k;
          const bool ok = yok && gx >= 0 && gx < a.W;
          m.off[i * 4 + k] = ok ? (unsigned)(((gy * a.W + gx) * Cin + 4 * pq) * 4) : 0x80000000u;
        }
      }
    };
    auto issue = [&](floatx4 (&d)[16], const Aim& m, int chunk) {
      if (WINO_ABL & 4) return;
#pragma unroll
      for (int p = 0; p < 16; ++p)
        d[p] = __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(m.rsrc, m.off[p], chunk * (WCK * 4), 0));
    };
    auto commit = [&](floatx4 (&d)[16], const Aim& m, float* vbuf) {
      if (WINO_ABL & 2) return;
      // columns, in place: (w0,w1,w2,w3) = (d0-d2, d1+d2, d2-d1, d1-d3)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const floatx4 d0 = d[i * 4 + 0], d1 = d[i * 4 + 1], d2 = d[i * 4 + 2], d3 = d[i * 4 + 3];
        d[i * 4 + 0] = sub4(d0, d2);
        d[i * 4 + 1] = d1 + d2;
        d[i * 4 + 2] = sub4(d2, d1);
        d[i * 4 + 3] = sub4(d1, d3);
      }
      // rows, straight to LDS: xi0 = r0-r2, xi1 = r1+r2, xi2 = r2-r1, xi3 = r1-r3
      float* dst = vbuf + vwrite;
#pragma unroll
      for (int nu = 0; nu < 4; ++nu) {
        const floatx4 r0 = d[0 * 4 + nu], r1 = d[1 * 4 + nu], r2 = d[2 * 4 + nu], r3 = d[3 * 4 + nu];
        *(floatx4*)(dst + (0 * 4 + nu) * 32 * WP) = sub4(r0, r2);
        *(floatx4*)(dst + (1 * 4 + nu) * 32 * WP) = r1 + r2;
        *(floatx4*)(dst + (2 * 4 + nu) * 32 * WP) = sub4(r2, r1);
        *(floatx4*)(dst + (3 * 4 + nu) * 32 * WP) = sub4(r1, r3);
      }
    };
    // Finished outputs of a tile (bias and activation already applied by the MFMA waves): LDS slots
    // -> global memory, 16 bytes per lane.  The V plane layout of Y (plane p = 4*(2i+j) + g holds,
    // for output pixel (i,j) of every Winograd tile, channels 32g..32g+31) means a helper thread
    // reads exactly the 16 float4 slots it will overwrite with the next V.
    // Two steps: aim_out(tile) computes, while the MFMA waves fold, a buffer descriptor of the output
    // image and one byte offset per output pixel (out of range for a pixel beyond the image: the
    // hardware drops that store); store_outputs() is then nothing but 16 LDS reads and 16 buffer
    // stores - no VALU work, so the copy runs beside the next tile's MFMAs.
    struct OutAim {
      unsigned po[4];
      __amdgpu_buffer_rsrc_t rs;
    };
    auto next_ticket = [&]() { return wino::take_ticket(a.ticket); };
    auto aim_out = [&](OutAim& o, const Tile& t) {
      const int phase = t.item & (a.nphase - 1);
      const int ppy = phase >> 1, ppx = phase & 1;  // sub-pixel phase placement (ConvTranspose2d)
      const int OH = a.nphase == 4 ? 2 * a.H : a.H, OW = a.nphase == 4 ? 2 * a.W : a.W;
      o.rs = __builtin_amdgcn_make_buffer_rsrc((void*)(a.out + (size_t)t.n * OH * OW * a.Cout), 0,
                                               OH * OW * a.Cout * 4, 0x00020000);  // host checks < 2 GiB
#pragma unroll
      for (int ij = 0; ij < 4; ++ij) {
        const int oy = t.ty * 8 + 2 * pty + (ij >> 1);
        const int ox = t.tx * 16 + 2 * ptx + (ij & 1);
        const unsigned po =
            (unsigned)(a.nphase == 4 ? ((2 * oy + ppy) * OW + (2 * ox + ppx)) * a.Cout
                       : a.s2d       ? ((oy >> 1) * (a.W >> 1) + (ox >> 1)) * (4 * a.Cout) + ((oy & 1) * 2 + (ox & 1)) * a.Cout
                                     : (oy * a.W + ox) * a.Cout) * 4u + 16u * pq;
        o.po[ij] = oy < a.H && ox < a.W ? po : 0x80000000u;
      }
    };
    auto store_outputs = [&](const OutAim& o, const float* yreg) {
      const float* src = yreg + vwrite;
      const int ngroups = (a.Cout + 31) >> 5;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        if (g >= ngroups) break;                                      // uniform
        if (g == ngroups - 1 && g * 32 + 4 * pq >= a.Cout) continue;  // partial last group (Cout % 32 != 0)
#pragma unroll
        for (int ij = 0; ij < 4; ++ij) {
          const floatx4 v = *(const floatx4*)(src + (ij * 4 + g) * 32 * WP);
          if (a.nt_out)  // uniform
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(uintx4, v), o.rs, o.po[ij], g * 128, 2);
          else
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(uintx4, v), o.rs, o.po[ij], g * 128, 0);
        }
      }
    };
    int tile_count = 0;
    (void)tile_count;
    if (ht == 0) {
      post(0, (int)blockIdx.x);  // grid <= ntiles
      post(1, next_ticket());
    }
    wg_barrier();  // P0: the first two descriptors are posted
    Tile cur = read_slot(0);
    // The patch in flight and its aim live across tiles: the aim moves on to the next tile two
    // chunks before the current one ends, and (layers with more than one chunk) the loads of the next
    // tile's target 0 are issued before the fold barriers of the current one, so their latency and
    // that of the ticket fetch pass while the MFMA waves fold.
    Aim m;
    floatx4 d[16];
    int ticket_pre = a.ntiles;  // ticket for the descriptor posted in the coming tile's chunk 0 (thread 0)
    aim(m, cur);
    issue(d, m, 0);
    commit(d, m, lds);
    if (nchunks > 1) {
      if (ht == 0 && read_slot(1).item < a.ntiles) ticket_pre = next_ticket();
      issue(d, m, 1);  // target 0 of the first tile
    }
    wg_barrier();  // P
    int buf = 0, s_nxt = 1, s_wr = 2;
    OutAim oa;
    oa.rs = m.rsrc;  // (defined on every path; aimed before the first fold)
#pragma unroll
    for (int ij = 0; ij < 4; ++ij) oa.po[ij] = 0x80000000u;
    bool have_y = false;  // finished outputs of the previous tile wait in V[buf^1], aimed by oa
    while (cur.item < a.ntiles) {
      const Tile nxt = read_slot(s_nxt);
      const bool more = nxt.item < a.ntiles;
      tile_count++;
      // chunk c: the MFMA waves consume V[buf]; the helpers fill V[buf^1] with target c =
      // (cur, c+1), or (nxt, 0) for the last chunk.  Re-aiming is VALU work and happens before the
      // barrier; the 16 buffer loads need no VALU and are issued right behind the barrier, where
      // they fly during the MFMA phase.
      auto pre_aim = [&](int chunk) {
        if (chunk + 2 == nchunks && more) aim(m, nxt);
      };
      auto post_issue = [&](int chunk) {
        if (chunk + 2 < nchunks)
          issue(d, m, chunk + 2);
        else if (chunk + 2 == nchunks && more)
          issue(d, m, 0);
      };
      {  // chunk 0
        float* vnext = lds + (buf ^ 1) * WBUF;
        const bool tgt0 = nchunks > 1 || more;
        int ticket = ticket_pre;
        if (nchunks == 1) {
          // single-chunk layer: target 0 is (nxt, 0).  Ticket first (its return is then the oldest
          // entry of this wave's in-order vmcnt queue), then the input loads, then the output copy:
          // the loads' latency passes during the copy and no load waits behind a store.
          if (ht == 0 && more) ticket = next_ticket();
          aim(m, more ? nxt : cur);
          issue(d, m, 0);
        }
        if (have_y && !(WINO_ABL & 1)) store_outputs(oa, vnext);
        if (tgt0) commit(d, m, vnext);
        if (ht == 0 && more) post(s_wr, ticket);
        pre_aim(0);
        wg_barrier();  // B_0
        post_issue(0);
        buf ^= 1;
      }
      for (int chunk = 1; chunk < nchunks; ++chunk) {
        float* vnext = lds + (buf ^ 1) * WBUF;
        if (chunk + 1 < nchunks || more) commit(d, m, vnext);
        pre_aim(chunk);
        wg_barrier();  // B_chunk
        post_issue(chunk);
        buf ^= 1;
      }
      if (nchunks > 1 && more) {
        // next tile's target 0 = (nxt, 1) (the aim is on nxt since chunk nchunks-2) and the ticket
        // for the descriptor it will post: both in flight across the fold barriers
        if (ht == 0 && read_slot(s_wr).item < a.ntiles) ticket_pre = next_ticket();
        issue(d, m, 1);
      }
      aim_out(oa, cur);  // VALU work, done while the MFMA waves fold
      wg_barrier();  // E1
      wg_barrier();  // E2: the finished outputs of this tile lie in V[buf^1]
      have_y = true;
      cur = nxt;
      // wino::rotate_ring, kept local: through the shared one this kernel's SGPR allocation and spill code move
      const int s_old = s_nxt;
      s_nxt = s_wr;
      s_wr = s_old == 0 ? 2 : s_old - 1;
    }
    if (have_y) store_outputs(oa, lds + (buf ^ 1) * WBUF);  // outputs of the last tile
#if WINO_STAMP
    if (wave == 8 && lane < 32) wino_stamps[blockIdx.x * 32 + lane] = ((long long*)(lds + 2 * WBUF + 16))[lane];
#endif
    if (ht == 0) wino::rearm_ticket(a.ticket);
    return;
  }

  // ===================================== MFMA waves ==============================================
  // Wave w owns column tile nt = w&3 (32 output channels) and positions 8*(w>>2) .. +7.
  const int h = lane >> 5, l31 = lane & 31;
  const int nt = wave & 3, ph = wave >> 2;
  const bool nvalid = nt * 32 < a.CoutP;
  const int nchunks = a.Cin / WCK;
  constexpr bool ZSKIP = MODE != 0;
  constexpr int PDIR = MODE == 2 ? -1 : 1;  // step it = pi*4 + sub works on position p = (PDIR > 0 ? pi : 7 - pi)
  // U stream: packed [pos][Cin/8][CoutP][8] floats; the fetch position advances by one 8-channel
  // group (step_s bytes) per fragment, after four of them to the next position, after 32 to the
  // first position of the next chunk.  Kept as one 32-bit lane offset against a uniform 64-bit
  // base, so no per-fragment address is hoisted.
  const unsigned step_s = (unsigned)a.CoutP * 32u;             // bytes per 8-channel group
  const unsigned step_p = (unsigned)(a.Cin >> 3) * step_s;    // bytes per position
  const unsigned step_pos = (unsigned)PDIR * step_p - 3u * step_s;    // (p, sub 3) -> (p + PDIR, sub 0)
  const unsigned step_chunk = step_s - 7u * (unsigned)PDIR * step_p;  // (last p, sub 3) -> (first p, next chunk)
  // The lane part of the address never changes; the stream position is a scalar (buffer load with
  // SGPR offset), so the MFMA loop spends no VALU instruction on addressing.
  const unsigned ulane = (unsigned)((((nvalid ? nt : 0) * 32 + l31) * 8 + 4 * h) * 4);
  const unsigned soff0 = (unsigned)(ph * 8 + (PDIR > 0 ? 0 : 7)) * step_p;  // first fragment of a tile
  const int aread = ((ph * 8) * 32 + l31) * WP + 4 * h;  // + p*32*WP + sub*8
  auto pos_of = [](int it) { return PDIR > 0 ? it >> 2 : 7 - (it >> 2); };
  // epilogue parameters of this lane's output channel
  float pbias = 0.f, pbeta = 1.f, pgamma = 0.f;
  {
    const int col = nt * 32 + l31;
    if (col < a.Cout) {
      pbias = a.bias[col];
      if (a.act == DSIC_ACT_GDN || a.act == DSIC_ACT_IGDN) {
        pbeta = a.beta[col];
        pgamma = a.gamma[col];
      }
    }
  }
  const int stamp_wave = 0;
  int tile_count = 0;
  (void)stamp_wave; (void)tile_count;
  constexpr int R = WINO_RING;
  static_assert(R == 2 || R == 4, "ring depth must divide the 32 steps of a chunk");

  floatx16 acc[8];
  floatx4 Bq[R];
  wg_barrier();  // P0
  wg_barrier();  // P
  Tile cur = read_slot(0);
  const __amdgpu_buffer_rsrc_t urs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)a.u, 0, (int)(16u * step_p * (unsigned)a.nphase), 0x00020000);  // all phases' U (host checks < 2 GiB)
  const unsigned phase_bytes = (unsigned)a.u_phase_stride * 4u;
  unsigned soff = soff0 + (unsigned)(cur.item & (a.nphase - 1)) * phase_bytes;  // fetch stream position
  // skip: the step is a structurally zero position of this chunk - its MFMAs will not run, so the
  // load is pointed at the tile's first fragment (an L1/L2 hit) instead of pulling a line of zeros
  // through L2; the stream position advances all the same.
  auto fetch = [&](int f, bool skip = false) {  // fragment of step f (mod 32) of the stream
    const unsigned so = skip ? soff0 : soff;
    const floatx4 v = __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(urs, ulane, so, 0));
    soff += (f & 31) == 31 ? step_chunk : ((f & 3) == 3 ? step_pos : step_s);
    return v;
  };
#pragma unroll
  for (int f = 0; f < R - 1; ++f) Bq[f] = fetch(f);
  int buf = 0, s_nxt = 1;
  while (cur.item < a.ntiles) {
    const Tile nxt = read_slot(s_nxt);
    const unsigned soff_nxt = soff0 + (unsigned)((nxt.item < a.ntiles ? nxt.item : cur.item) & (a.nphase - 1)) * phase_bytes;
    tile_count++;
    // FIRST: chunk 0 of a tile starts every accumulator from a zero C operand (inline constant), so
    // the 128 accumulator registers are never cleared by VALU moves
    auto chunk_body = [&](auto first_tag, int chunk) {
      constexpr bool FIRST = decltype(first_tag)::value;
      if (chunk >= WINO_STAMP_CHUNK0 && chunk < WINO_STAMP_CHUNK0 + 4) STAMP((chunk - WINO_STAMP_CHUNK0) * 4 + 0);
      const bool last = chunk + 1 == nchunks;
      // Structurally zero Winograd positions: a 3-tap filter with a zero end tap has a zero
      // transform component (G (g0,g1,0)^T)[3] = 0, (G (0,g1,g2)^T)[0] = 0.  For the space-to-depth
      // form of a 5x5/s2 kernel the phases a=1 / b=1 lack the last row / column (xi=3 / nu=3
      // vanish); for a ConvTranspose2d phase py=1 / px=1 lacks the first row / column (xi=0 /
      // nu=0 vanish).  Those MFMA clusters are skipped: 49 instead of 64 position-phase GEMMs.
      unsigned zero_xi = 4, zero_nu = 4;  // 4 = none
      if (MODE == 1) {
        const int blk = chunk / (nchunks >> 2);  // channel block (a,b) = (blk>>1, blk&1)
        if (blk >> 1) zero_xi = 3;
        if (blk & 1) zero_nu = 3;
      } else if (MODE == 2) {
        const int phase = cur.item & 3;
        if (phase >> 1) zero_xi = 0;
        if (phase & 1) zero_nu = 0;
      }
      auto is_zero = [&](int it) {
        const int p = pos_of(it);
        const unsigned xi = (unsigned)(ph * 2 + (p >> 2)), nu = (unsigned)(p & 3);
        return xi == zero_xi || nu == zero_nu;
      };
      const float* vb = lds + buf * WBUF + aread;
      floatx4 Aq[2];
      Aq[0] = *(const floatx4*)(vb + pos_of(0) * 32 * WP);
#pragma unroll
      for (int it = 0; it < 32; ++it) {  // it = pi*4 + sub
        {
          const int f = it + R - 1;  // U fragment to fetch now (continuous across chunks and tiles)
          if (f == 32 && last) soff = soff_nxt;  // the stream moves on to the next tile: its phase's U, first group
          // (the first R-1 steps of the next chunk are never zero positions: position 0, or 7 in MODE 2)
          Bq[f % R] = fetch(f, ZSKIP && f < 32 && is_zero(f));
        }
        if (it + 1 < 32) {
          const int p1 = pos_of(it + 1), s1 = (it + 1) & 3;
          Aq[(it + 1) & 1] = *(const floatx4*)(vb + p1 * 32 * WP + s1 * 8);
        }
        const int p0 = pos_of(it);
        if (!ZSKIP || !is_zero(it)) {  // wave-uniform
          if (WINO_CPRIO) __builtin_amdgcn_s_setprio(WINO_CPRIO);
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            const floatx16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            acc[p0] = __builtin_amdgcn_mfma_f32_32x32x2f32(Aq[it & 1][s], Bq[it % R][s],
                                                           FIRST && (it & 3) == 0 && s == 0 ? zero : acc[p0], 0, 0, 0);
          }
          if (WINO_CPRIO) __builtin_amdgcn_s_setprio(0);
        } else if (FIRST && (it & 3) == 0) {  // a skipped position still has to read as zero in the fold
#pragma unroll
          for (int e = 0; e < 16; ++e) acc[p0][e] = 0.f;
        }
      }
      if (chunk >= WINO_STAMP_CHUNK0 && chunk < WINO_STAMP_CHUNK0 + 4) STAMP((chunk - WINO_STAMP_CHUNK0) * 4 + 1);
      if (chunk >= WINO_STAMP_CHUNK0 && chunk < WINO_STAMP_CHUNK0 + 4) STAMP((chunk - WINO_STAMP_CHUNK0) * 4 + 2);
      wg_barrier();  // B_chunk
      if (chunk >= WINO_STAMP_CHUNK0 && chunk < WINO_STAMP_CHUNK0 + 4) STAMP((chunk - WINO_STAMP_CHUNK0) * 4 + 3);
      buf ^= 1;
    };
    chunk_body(std::true_type{}, 0);
    for (int chunk = 1; chunk < nchunks; ++chunk) chunk_body(std::false_type{}, chunk);


    // ---- inverse transform ------------------------------------------------------------------
    // Wave (nt, ph) holds M[xi][nu] for xi in {2ph, 2ph+1}.  N[xi][j] = (M A)[xi][j]:
    //   N[.][0] = M0 + M1 + M2,  N[.][1] = M1 - M2 - M3.
    // Y[i][j] = (A^T N)[i][j]:  Y[0] = N0 + N1 + N2,  Y[1] = N1 - N2 - N3.
    //   ph=0: own = N0 + N1 (row 0), sends N1 to row 1;   ph=1: own = -(N2 + N3) (row 1), sends N2 to row 0.
    // Each wave stores its own row's partial sum into the Y planes of the free V buffer, and after
    // a barrier adds the term it owes to the other row in place (read, add, write: after the
    // barrier exactly one lane touches each element): Y = own + received.
    STAMP(24);
    if (WINO_ABL & 8) {
      wg_barrier();
    } else {
      float* yreg = lds + (buf ^ 1) * WBUF;
      // element e of this lane: Winograd tile (e&3) + 8*(e>>2) + 4h, channel 32nt + l31
      float* yown = yreg + ((4 * (2 * ph) + nt) * 32 + 4 * h) * WP + l31;
      float* yoth = yreg + ((4 * (2 * (ph ^ 1)) + nt) * 32 + 4 * h) * WP + l31;
      floatx16 send[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const floatx16 na = j == 0 ? (acc[0] + acc[1]) + acc[2] : sub16(sub16(acc[1], acc[2]), acc[3]);  // local xi 0
        const floatx16 nb = j == 0 ? (acc[4] + acc[5]) + acc[6] : sub16(sub16(acc[5], acc[6]), acc[7]);  // local xi 1
        const floatx16 own = ph == 0 ? na + nb : -(na + nb);
        send[j] = ph == 0 ? nb : na;
#pragma unroll
        for (int e = 0; e < 16; ++e) yown[(4 * j * 32 + (e & 3) + 8 * (e >> 2)) * WP] = own[e];
      }
      wg_barrier();  // E1
      STAMP(25);
      // The wave that adds the second term holds the finished sum in registers, so bias and
      // activation are applied right here (this lane = one output channel: its three parameters
      // live in registers) and the helpers only copy the result out.
      wino::for_act(a.act, [&](auto act_tag) {
        constexpr int ACT = decltype(act_tag)::value;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          floatx16 got;
#pragma unroll
          for (int e = 0; e < 16; ++e) got[e] = yoth[(4 * j * 32 + (e & 3) + 8 * (e >> 2)) * WP];
#pragma unroll
          for (int e = 0; e < 16; e += 2) {
            floatx2 v = {got[e], got[e + 1]};
            v = wino::bias_act<ACT>(v + floatx2{send[j][e], send[j][e + 1]}, pbias, pbeta, pgamma);
            yoth[(4 * j * 32 + (e & 3) + 8 * (e >> 2)) * WP] = v[0];
            yoth[(4 * j * 32 + ((e + 1) & 3) + 8 * ((e + 1) >> 2)) * WP] = v[1];
          }
        }
      });
    }
    STAMP(26);
    wg_barrier();  // E2: the helpers copy the finished outputs from here and refill the buffer
    STAMP(27);
    cur = nxt;
    s_nxt = wino::step_ring(s_nxt);
  }
}

// U_p = G g G^T per (cout, cin), packed [16][Cin/8][CoutP][8].
// s2 = 0: g is the 3x3 kernel of a stride-1 conv, w [Cout][Cin][3][3].
// s2 = 1: w [Cout][Cs][5][5] is a 5x5 stride-2 pad-2 kernel; over the space-to-depth input
//         (channel c' = (a*2+b)*Cs + c holds x[2i+a][2j+b][c]) it is the 3x3 stride-1 kernel
//         g_ab[u][v] = w[2u+a][2v+b] (zero where 2u+a or 2v+b exceeds 4): Cin = 4*Cs.
__global__ void pack_wino_weight_kernel(const float* __restrict__ w, float* __restrict__ dst, int Cout,
                                        int Cin, int Cin8, int CoutP, int s2, int64_t total) {
  // s2 = 2..5: phase (s2-2) = py*2+px of ConvTranspose2d(5,2,2,1), w [Cin][Cout][5][5]:
  //   g[wr][wc] = w[c][n][py+4-2wr][px+4-2wc] for wr >= py, wc >= px, else 0
  //   (output (2i+py, 2j+px) reads input (i-1+wr, j-1+wc); from oy = 2*iy - 2 + ky).
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int j = i & 7;
  int64_t r = i >> 3;
  const int n = r % CoutP;
  r /= CoutP;
  const int c8 = r % Cin8;
  const int p = r / Cin8;
  const int xi = p >> 2, nu = p & 3;
  const int c = c8 * 8 + j;
  float v = 0.f;
  if (n < Cout && c < Cin) {
    float g[9];
    if (s2 >= 2) {
      const int py = (s2 - 2) >> 1, px = (s2 - 2) & 1;
      const float* gp = w + ((size_t)c * Cout + n) * 25;
#pragma unroll
      for (int wr = 0; wr < 3; ++wr)
#pragma unroll
        for (int wc = 0; wc < 3; ++wc)
          g[wr * 3 + wc] = (wr >= py && wc >= px) ? gp[(py + 4 - 2 * wr) * 5 + (px + 4 - 2 * wc)] : 0.f;
    } else if (!s2) {
      const float* gp = w + ((size_t)n * Cin + c) * 9;
#pragma unroll
      for (int t = 0; t < 9; ++t) g[t] = gp[t];
    } else {
      const int Cs = Cin >> 2, ab = c / Cs, cs = c % Cs;
      const int pa = ab >> 1, pb = ab & 1;
      const float* gp = w + ((size_t)n * Cs + cs) * 25;
#pragma unroll
      for (int u = 0; u < 3; ++u)
#pragma unroll
        for (int v = 0; v < 3; ++v) {
          const int ky = 2 * u + pa, kx = 2 * v + pb;
          g[u * 3 + v] = (ky < 5 && kx < 5) ? gp[ky * 5 + kx] : 0.f;
        }
    }
    // row combination (G g)[xi][kx], then column combination with G^T
    float row[3];
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const float g0 = g[0 * 3 + kx], g1 = g[1 * 3 + kx], g2 = g[2 * 3 + kx];
      row[kx] = xi == 0 ? g0 : (xi == 1 ? 0.5f * ((g0 + g1) + g2) : (xi == 2 ? 0.5f * ((g0 - g1) + g2) : g2));
    }
    v = nu == 0 ? row[0]
                : (nu == 1 ? 0.5f * ((row[0] + row[1]) + row[2])
                           : (nu == 2 ? 0.5f * ((row[0] - row[1]) + row[2]) : row[2]));
  }
  dst[i] = v;
}

}  // namespace dsic

using namespace dsic;

#if WINO_STAMP
extern "C" int dsic_debug_wino_stamps(long long* host_out) {
  return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(wino_stamps), sizeof(long long) * 256 * 32) == hipSuccess ? 0 : 2;
}
#endif

extern "C" int64_t dsic_wino_weight_floats(int Cout, int Cin) {
  return (int64_t)16 * (round_up(Cin, 8) / 8) * round_up(Cout, 32) * 8;
}

extern "C" int dsic_pack_wino_weight(const float* w_oihw, float* dst, int Cout, int Cin, void* stream) {
  DSIC_REQUIRE(w_oihw && dst && Cout > 0 && Cin > 0, "pack_wino_weight: bad argument");
  const int Cin8 = round_up(Cin, 8) / 8, CoutP = round_up(Cout, 32);
  const int64_t total = dsic_wino_weight_floats(Cout, Cin);
  hipLaunchKernelGGL(pack_wino_weight_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, w_oihw, dst, Cout, Cin, Cin8, CoutP, 0, total);
  return check_launch("pack_wino_weight");
}

extern "C" int dsic_pack_wino_s2_weight(const float* w_oihw5, float* dst, int Cout, int Cs, void* stream) {
  DSIC_REQUIRE(w_oihw5 && dst && Cout > 0 && Cs > 0 && Cs % 8 == 0, "pack_wino_s2_weight: bad argument");
  const int Cin = 4 * Cs, Cin8 = Cin / 8, CoutP = round_up(Cout, 32);
  const int64_t total = dsic_wino_weight_floats(Cout, Cin);
  hipLaunchKernelGGL(pack_wino_weight_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, w_oihw5, dst, Cout, Cin, Cin8, CoutP, 1, total);
  return check_launch("pack_wino_s2_weight");
}

extern "C" int dsic_pack_wino_convT_weight(const float* w_iohw5, float* dst, int Cin, int Cout, void* stream) {
  DSIC_REQUIRE(w_iohw5 && dst && Cout > 0 && Cin > 0 && Cin % 8 == 0, "pack_wino_convT_weight: bad argument");
  const int Cin8 = Cin / 8, CoutP = round_up(Cout, 32);
  const int64_t total = dsic_wino_weight_floats(Cout, Cin);
  for (int phase = 0; phase < 4; ++phase) {
    hipLaunchKernelGGL(pack_wino_weight_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, w_iohw5, dst + (size_t)phase * total, Cout, Cin, Cin8, CoutP, 2 + phase,
                       total);
  }
  return check_launch("pack_wino_convT_weight");
}

// One launch of the fp32 kernel: a 3x3 layer (nphase 1) or the four phases of a transposed one.  what, gdn: the
// export's message prefix and its name for the activation.
static int wino_launch(const char* what, const char* gdn, const wino_host::Layer& l, int nphase, void* stream) {
  if (const int rc = wino_host::check_layer(what, gdn, 32, l)) return rc;
  WinoArgs a{};
  a.in = l.in; a.u = (const float*)l.u; a.bias = l.bias; a.beta = l.beta; a.gamma = l.gamma; a.out = l.out;
  a.B = l.B; a.H = l.H; a.W = l.W; a.Cin = l.Cin; a.Cout = l.Cout; a.CoutP = round_up(l.Cout, 32); a.act = l.act;
  a.ticket = (unsigned long long*)l.ticket;
  a.s2d = l.s2d_out; a.s2d_in = l.s2d_in;
  a.nphase = nphase; a.u_phase_stride = nphase == 4 ? dsic_wino_weight_floats(l.Cout, l.Cin) : 0;
  a.tiles_x = ceil_div(a.W, 16); a.tiles_y = ceil_div(a.H, 8);
  const int64_t nt = (int64_t)a.tiles_x * a.tiles_y * a.B * nphase;
  if (const int rc = wino_host::check_limits("conv3x3_wino", nt, a.H, a.W, a.Cin, (int64_t)a.Cout * (nphase == 4 ? 4 : 1),
                                             (int64_t)16 * (a.Cin / 8) * a.CoutP * 8 * 4 * nphase))
    return rc;
  a.ntiles = (int)nt;
  a.nt_out = wino_host::streams_output(a.B, a.H, a.W, a.Cout, nphase);
  static wino_host::Family<3> family = {"conv3x3_wino", WTHREADS, WLDS_TOTAL,   // by MODE
                                        {(const void*)conv_wino_kernel<0>, (const void*)conv_wino_kernel<1>,
                                         (const void*)conv_wino_kernel<2>}};
  return wino_host::launch(family, a.s2d_in ? 1 : nphase == 4 ? 2 : 0, nt, a, (hipStream_t)stream);
}

// The cap of every Winograd kernel's persistent grid (wino_host::persistent_grid), for all three translation units.
extern "C" int dsic_wino_grid(int n) { return wino_host::set_grid_override(n); }

extern "C" int dsic_conv_transpose2d_wino_nhwc(const float* in, const float* u_packed4, const float* bias,
                                               const float* beta, const float* gamma, float* out, int B,
                                               int H, int W, int Cin, int Cout, int act, void* ticket,
                                               void* stream) {
  return wino_launch("convT_wino", "IGDN", {in, u_packed4, bias, beta, gamma, out, ticket, B, H, W, Cin, Cout, act, 0, 0},
                     4, stream);
}

extern "C" int dsic_conv3x3_wino_nhwc(const float* in, const float* u_packed, const float* bias,
                                      const float* beta, const float* gamma, float* out, int B, int H,
                                      int W, int Cin, int Cout, int act, int s2d_out, int s2d_in,
                                      void* ticket, void* stream) {
  DSIC_REQUIRE(!((s2d_out | s2d_in) & DSIC_LAYOUT_CM16), "conv3x3_wino: chunk-major activations are not supported");
  return wino_launch("conv3x3_wino", "GDN",
                     {in, u_packed, bias, beta, gamma, out, ticket, B, H, W, Cin, Cout, act, s2d_out, s2d_in ? 1 : 0}, 1,
                     stream);
}
