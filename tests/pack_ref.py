"""NumPy restatements of the weight packers (csrc/layout.hip, conv_wino.hip, conv_wino_bf16.hip, convT_image.hip): for
every export the exact buffer it must write, padding included, and the size functions.

A helper for tests/test_pack_ref_cpu.py (which ties every restated buffer to the convolution it stands for, and shows
that the named mutants differ) and tests/test_gpu_weight_packers.py (which holds the kernels to it bit by bit).  The
buffers are built from the layouts as include/dsic_hip.h and the kernels' comments state them, by reshaping arrays that
carry one axis per index of the layout; the kernels go the other way, from a flat index to its source element.  The
views of g (space-to-depth, transposed phases) and the matrix G are conv_ref's.  NumPy only; torch is touched through
conv_ref's two pure index helpers.

Layouts (CoutP = round_up(Cout, 32); a channel axis of 8 or 16 is innermost; every padding element is +0.0):
  conv        [k*k taps, ky-major][ceil(Cin/8)][CoutP][8]                                    fp32
  convT       [25 taps][Cin/8][CoutP][8]: phases (py,px) = (0,0),(0,1),(1,0),(1,1) own 9, 6, 6, 4 taps (ty,tx), tx
              fastest, with ky = py+4-2(ty+py), kx = px+4-2(tx+px)                            fp32
  Winograd    [16 positions xi*4+nu][ceil(Cin/8)][CoutP][8], U = G g G^T; transposed: four such blocks, py*2+px
  bf16 split  per phase [16][Cin/16][P planes][CoutP][16]                                     bf16
  image       [9 taps wr*3+wc][Cin/16][16 columns ph*Cimg+c][16] fp32, then
              [Cin/16][9][hi, mid][half][16 columns][8] bf16
"""
from __future__ import annotations

import zlib

import numpy as np
import torch

import conv_ref

F32 = np.float32


def round_up(a, b):
    return (a + b - 1) // b * b


# ---------------------------------------------------------------------------------------------------- sizes

def packed_conv_weight_floats(Cout, Cin, k):
    return k * k * (round_up(Cin, 8) // 8) * round_up(Cout, 32) * 8


def packed_convT_weight_floats(Cout, Cin):
    return packed_conv_weight_floats(Cout, Cin, 5)


def wino_weight_floats(Cout, Cin):
    return 16 * (round_up(Cin, 8) // 8) * round_up(Cout, 32) * 8


def wino_bf16_weight_bytes(Cout, Cin, P):
    """One phase: 16 positions x Cin channels x CoutP columns x P planes of 2 bytes."""
    return 16 * (Cin // 16) * P * round_up(Cout, 32) * 16 * 2


def convT_image_weight_floats(Cin):
    """9 taps x Cin x 16 columns as fp32, and as many bytes again for the two bf16 planes."""
    return 2 * 9 * Cin * 16


# ---------------------------------------------------------------------------------------------------- bf16

def bf16_rne(x):
    """float32 -> bf16 bits (uint16), round to nearest, ties to even.  Finite values inside the bf16 range only."""
    b = np.ascontiguousarray(x, dtype=F32).view(np.uint32)
    return ((b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def bf16_trunc(x):
    return (np.ascontiguousarray(x, dtype=F32).view(np.uint32) >> np.uint32(16)).astype(np.uint16)


def bf16_value(bits):
    """bf16 bits -> the float32 of the same value (exact)."""
    return (np.asarray(bits).astype(np.uint32) << np.uint32(16)).view(F32)


def planes(v, P, mutant=None):
    """[P, *v.shape] bf16 bits: plane q = RNE(rem_q), rem_0 = v, rem_{q+1} = rem_q - plane_q (exact in fp32).
    mutants: truncate (planes by truncation), mid_from_v (every plane taken from v, not from the remainder)."""
    cvt = bf16_trunc if mutant == "truncate" else bf16_rne
    rem, out = np.asarray(v, dtype=F32), []
    for _ in range(P):
        p = cvt(rem)
        out.append(p)
        if mutant != "mid_from_v":
            rem = rem - bf16_value(p)
    return np.stack(out)


# ---------------------------------------------------------------------------------------------------- igemm forms

def _tap_cin8_cout(g, pad=0.0):
    """g [T][Cout][Cin] -> [T][ceil(Cin/8)][CoutP][8], flat, in g's dtype; pad: what the padding holds."""
    T, Cout, Cin = g.shape
    C8, CoutP = round_up(Cin, 8) // 8, round_up(Cout, 32)
    full = np.full((T, CoutP, C8 * 8), pad, dtype=g.dtype)
    full[:, :Cout, :Cin] = g
    return np.ascontiguousarray(full.reshape(T, CoutP, C8, 8).transpose(0, 2, 1, 3)).reshape(-1)


def pack_conv_weight(w, k, mutant=None):
    """w [Cout][Cin][k][k] -> tap ky*k+kx holds w[:, :, ky, kx].  mutant: padding (padding left non-zero)."""
    w = np.asarray(w, dtype=F32)
    Cout, Cin = w.shape[:2]
    assert w.shape[2:] == (k, k)
    g = w.transpose(2, 3, 0, 1).reshape(k * k, Cout, Cin)
    return _tap_cin8_cout(g, pad=1.0 if mutant == "padding" else 0.0)


PHASES = ((0, 0), (0, 1), (1, 0), (1, 1))


def convT_taps(order=PHASES, reverse=True):
    """[(py, px, ty, tx, ky, kx)] of the 25 taps in buffer order: phase (py,px) has (3-py)(3-px) local taps (ty,tx);
    output (2i+py, 2j+px) reads input (i-1+ty+py, j-1+tx+px) through kernel element (ky,kx).  reverse=False: the
    kernel walked forwards (ky = 2(ty+py)-py), which is the correlation, not the transposed convolution."""
    taps = []
    for py, px in order:
        for ty in range(3 - py):
            for tx in range(3 - px):
                ky, kx = py + 4 - 2 * (ty + py), px + 4 - 2 * (tx + px)
                taps.append((py, px, ty, tx, ky, kx) if reverse else (py, px, ty, tx, 4 - ky, 4 - kx))
    return taps


def pack_convT_weight(w, mutant=None):
    """w [Cin][Cout][5][5] (nn.ConvTranspose2d).  mutants: swap (w read as [Cout][Cin]), phases (another phase order),
    forward (tap reversal dropped), padding."""
    w = np.asarray(w, dtype=F32)
    Cin, Cout = w.shape[:2]
    assert w.shape[2:] == (5, 5)
    w_oc = w.reshape(Cout, Cin, 5, 5) if mutant == "swap" else w.transpose(1, 0, 2, 3)
    order = (PHASES[0], PHASES[2], PHASES[1], PHASES[3]) if mutant == "phases" else PHASES
    g = np.stack([w_oc[:, :, ky, kx] for *_, ky, kx in convT_taps(order, reverse=mutant != "forward")])
    return _tap_cin8_cout(g, pad=1.0 if mutant == "padding" else 0.0)


# ---------------------------------------------------------------------------------------------------- Winograd forms

def _combine(a, b, c):
    """The four rows of G applied to (a, b, c) in the kernel's stated order: a, 0.5 ((a + b) + c), 0.5 ((a - b) + c),
    c.  In float32 every step is one rounding (x 0.5 is exact), and there is no product to contract into an add."""
    half = a.dtype.type(0.5)
    return [a, half * ((a + b) + c), half * ((a - b) + c), c]


def ggt32(g):
    """g [...,3,3] float32 -> U [...,4,4] float32: rows first ((G g)[xi][kx]), then the columns."""
    g = np.asarray(g, dtype=F32)
    rows = np.stack(_combine(g[..., 0, :], g[..., 1, :], g[..., 2, :]), axis=-2)          # [...,4,3]
    return np.stack(_combine(rows[..., 0], rows[..., 1], rows[..., 2]), axis=-1)          # [...,4,4]


def ggt64(g, absolute=False):
    G = np.array(conv_ref._G, dtype=np.float64)
    g = np.asarray(g, dtype=np.float64)
    if absolute:
        G, g = np.abs(G), np.abs(g)
    return np.einsum("ij,...jk,lk->...il", G, g, G)


def _wino_block(g, pad=0.0):
    """g [Cout][Cin][3][3] float32 -> (U, U64, A), each one [16][ceil(Cin/8)][CoutP][8] block."""
    Cout, Cin = g.shape[:2]
    out = []
    for U in (ggt32(g), ggt64(g), ggt64(g, absolute=True)):
        out.append(_tap_cin8_cout(U.reshape(Cout, Cin, 16).transpose(2, 0, 1), pad))
    return tuple(out)


def pack_wino_weight(w, mutant=None):
    """w [Cout][Cin][3][3] -> (U float32, U64 float64, A = |G||g||G^T| float64) in the packed layout."""
    w = np.asarray(w, dtype=F32)
    assert w.shape[2:] == (3, 3)
    return _wino_block(w, pad=1.0 if mutant == "padding" else 0.0)


def s2d_g(w5):
    """[Cout][Cs][5][5] -> the 3x3 kernels over the 4*Cs space-to-depth channels c' = (2a+b)*Cs + c:
    g_ab[u][v] = w[2u+a][2v+b], zero where the index exceeds 4 (conv_ref.s2d_operands)."""
    _, g = conv_ref.s2d_operands(torch.zeros(1, 1, 2, 2), torch.from_numpy(np.ascontiguousarray(w5, dtype=F32)))
    return g.numpy()


def pack_wino_s2_weight(w5, mutant=None):
    w5 = np.asarray(w5, dtype=F32)
    assert w5.shape[2:] == (5, 5)
    return _wino_block(s2d_g(w5), pad=1.0 if mutant == "padding" else 0.0)


def convT_phase_g(w5):
    """[Cin][Cout][5][5] -> {(py,px): [Cout][Cin][3][3]}, g[wr][wc] = w[py+4-2wr][px+4-2wc], zero for wr < py or
    wc < px (conv_ref.convT_phase_weights)."""
    ph = conv_ref.convT_phase_weights(torch.from_numpy(np.ascontiguousarray(w5, dtype=F32)))
    return {k: v.numpy() for k, v in ph.items()}


def pack_wino_convT_weight(w5, mutant=None):
    """w [Cin][Cout][5][5] -> the four phase blocks, py*2+px.  mutants: swap, phases, forward, padding (as
    pack_convT_weight)."""
    w5 = np.asarray(w5, dtype=F32)
    Cin, Cout = w5.shape[:2]
    assert w5.shape[2:] == (5, 5)
    if mutant == "swap":
        w5 = np.ascontiguousarray(w5.reshape(Cout, Cin, 5, 5).transpose(1, 0, 2, 3))
    if mutant == "forward":
        w5 = w5[:, :, ::-1, ::-1]
    g = convT_phase_g(w5)
    order = (PHASES[0], PHASES[2], PHASES[1], PHASES[3]) if mutant == "phases" else PHASES
    blocks = [_wino_block(g[p], pad=1.0 if mutant == "padding" else 0.0) for p in order]
    return tuple(np.concatenate([b[i] for b in blocks]) for i in range(3))


def unpack_wino(u, Cout, Cin, nphase=1):
    """The packed layout read back: [nphase][16][CoutP][CinP] (any dtype)."""
    C8, CoutP = round_up(Cin, 8) // 8, round_up(Cout, 32)
    return np.asarray(u).reshape(nphase, 16, C8, CoutP, 8).transpose(0, 1, 3, 2, 4).reshape(nphase, 16, CoutP, C8 * 8)


def split_bf16(u32, Cout, Cin, nphase, P, mutant=None):
    """u32: nphase Winograd blocks as the packers write them -> bf16 bits, per phase [16][Cin/16][P][CoutP][16].
    mutants: truncate, mid_from_v (planes())."""
    assert Cin % 16 == 0
    CoutP = round_up(Cout, 32)
    v = unpack_wino(np.asarray(u32, dtype=F32), Cout, Cin, nphase)                         # [ph][16][CoutP][Cin]
    pl = planes(v, P, mutant).reshape(P, nphase, 16, CoutP, Cin // 16, 16)
    return np.ascontiguousarray(pl.transpose(1, 2, 4, 0, 3, 5)).reshape(-1)


def unsplit_bf16(bits, Cout, Cin, nphase, P):
    """The planes of split_bf16 read back as float32 values: [P][nphase][16][CoutP][Cin]."""
    CoutP = round_up(Cout, 32)
    pl = bf16_value(np.asarray(bits).reshape(nphase, 16, Cin // 16, P, CoutP, 16))
    return pl.transpose(3, 0, 1, 4, 2, 5).reshape(P, nphase, 16, CoutP, Cin)


# ---------------------------------------------------------------------------------------------------- image form

def image_g(w, Cin, Cimg):
    """w [Cin][Cimg][5][5] -> [9 taps wr*3+wc][16 columns][Cin]: column ph*Cimg + c is phase ph = py*2+px of image
    channel c; columns >= 4*Cimg are zero."""
    w = np.asarray(w, dtype=F32)
    assert w.shape == (Cin, Cimg, 5, 5) and Cin % 16 == 0 and 1 <= Cimg <= 4
    g = convT_phase_g(w)
    cols = np.zeros((16, Cin, 3, 3), dtype=F32)
    for ph, p in enumerate(PHASES):
        cols[ph * Cimg:(ph + 1) * Cimg] = g[p]
    return cols.reshape(16, Cin, 9).transpose(2, 0, 1)


def pack_convT_image_weight(w, Cin, Cimg, mutant=None):
    """-> (fp32 [9][Cin/16][16 columns][16 channels], bf16 bits [Cin/16][9][hi, mid][half][16 columns][8]), flat; the
    second lies behind the first in the device buffer.  mutants: truncate, mid_from_v, half_col (half and column
    swapped in the planes), padding (columns >= 4*Cimg left non-zero), swap, phases, forward (as pack_convT_weight)."""
    w = np.asarray(w, dtype=F32)
    if mutant == "swap":
        w = np.ascontiguousarray(w.reshape(Cimg, Cin, 5, 5).transpose(1, 0, 2, 3))
    if mutant == "forward":
        w = w[:, :, ::-1, ::-1]
    v = image_g(w, Cin, Cimg)                                                              # [9][16][Cin]
    if mutant == "phases":
        v = v.copy()
        v[:, Cimg:3 * Cimg] = np.concatenate([v[:, 2 * Cimg:3 * Cimg], v[:, Cimg:2 * Cimg]], axis=1)
    if mutant == "padding":
        v = v.copy()
        v[:, 4 * Cimg:] = 1.0
    C16 = Cin // 16
    first = np.ascontiguousarray(v.reshape(9, 16, C16, 16).transpose(0, 2, 1, 3)).reshape(-1)
    pl = planes(v, 2, mutant).reshape(2, 9, 16, C16, 2, 8)                                 # [plane][t][col][c16][half][e]
    axes = (3, 1, 0, 2, 4, 5) if mutant == "half_col" else (3, 1, 0, 4, 2, 5)
    return first, np.ascontiguousarray(pl.transpose(axes)).reshape(-1)


# ---------------------------------------------------------------------------------------------------- shapes, inputs

# the smallest shapes that reach every branch of a packer: channel counts below, at and above the padding steps (8
# input channels, 32 columns), one and several 256-thread blocks, every kernel size, every phase block
CONV_SHAPES = [(k, Cout, Cin) for k in (1, 3, 5) for Cout, Cin in ((4, 3), (33, 12), (64, 8))]
CONVT_SHAPES = [(8, 4), (16, 33)]                      # (Cin, Cout)
WINO_SHAPES = [(4, 3), (36, 32), (64, 64)]             # (Cout, Cin)
WINO_S2_SHAPES = [(36, 8), (64, 16)]                   # (Cout, Cs)
WINO_CONVT_SHAPES = [(8, 36), (32, 64)]                # (Cin, Cout)
SPLIT_SHAPES = [(36, 32, 1), (64, 64, 1), (36, 32, 4)]  # (Cout, Cin, nphase)
IMAGE_SHAPES = [(Cin, Cimg) for Cin in (16, 48) for Cimg in (1, 3, 4)]


def make_weights(shape, seed):
    """[C0][C1][k][k] float32: zero-mean noise, and in every (c0, c1) kernel two planted values that no other kernel
    holds (exact, of either sign, at taps that move with c0 and c1), so that no exchange of indices maps the tensor
    onto itself and no two kernels cancel."""
    C0, C1, k, _ = shape
    rng = np.random.default_rng(seed)
    w = ((rng.random(shape) * 2.0 - 1.0) * 0.25).astype(F32)
    flat = w.reshape(C0, C1, k * k)
    c0, c1 = np.meshgrid(np.arange(C0), np.arange(C1), indexing="ij")
    ident = (1 + c0 * C1 + c1).astype(F32)
    flat[c0, c1, (c0 + 2 * c1) % (k * k)] = ident * F32(2.0 ** -12)
    flat[c0, c1, (3 * c0 + c1 + 1) % (k * k)] = -(ident * F32(2.0 ** -12) + F32(0.5))
    return w


def _f32_bits(*bits):
    return np.array(bits, dtype=np.uint32).view(F32)


def handmade_values():
    """What a bf16 split can get wrong, as float32 values (fp32 denormals and values that round past the bf16 range
    are left out: nothing here relies on what the conversion does with them):
      +0 and -0; exact bf16 values (mid must be 0); exact ties between two bf16 neighbours with an even and an odd
      upper half, of both signs; values whose REMAINDER ties (hi = 1: v - hi = 2^-10 (1 + 1/256), down to even, and
      2^-10 (1 + 3/256), up to even), of both signs; random significands at every magnitude 2^-20 .. 2^10."""
    zeros = _f32_bits(0x00000000, 0x80000000)
    exact = np.array([1.0, -1.5, 2.0 ** -20, -2.0 ** -20, 2.0 ** 10, -2.0 ** 10, 0.0234375, 255.0], dtype=F32)
    ties = _f32_bits(0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x42FE8000, 0x42FF8000, 0x35808000, 0xB5818000)
    rem = np.array([1.0 + 2.0 ** -10 + 2.0 ** -18, 1.0 + 2.0 ** -10 + 3 * 2.0 ** -18], dtype=np.float64)
    rem_ties = np.concatenate([rem, -rem, 64.0 * rem, -rem / 1024.0]).astype(F32)
    assert np.all(rem_ties.astype(np.float64) == np.concatenate([rem, -rem, 64.0 * rem, -rem / 1024.0]))
    rng = np.random.default_rng(2024)
    e = np.repeat(np.arange(-20, 11), 4)
    mags = ((1.0 + rng.random(e.size)) * np.exp2(e) * np.where(rng.random(e.size) < 0.5, -1.0, 1.0)).astype(F32)
    return np.concatenate([zeros, exact, ties, rem_ties, mags])


def handmade_u(Cout, Cin, nphase):
    """nphase Winograd blocks whose real elements cycle through handmade_values(); the padding is +0.0, as the
    packers leave it."""
    vals = handmade_values()
    n = nphase * 16 * Cout * Cin
    # a stride coprime to the number of values: every value meets every plane position
    real = vals[(np.arange(n) * 7) % vals.size].reshape(nphase, 16, Cout, Cin)
    return np.concatenate([_tap_cin8_cout(real[p]) for p in range(nphase)])


EXPORTS = {    # export -> (its shapes, the weight tensor of a shape)
    "conv": (CONV_SHAPES, lambda k, Cout, Cin: (Cout, Cin, k, k)),
    "convT": (CONVT_SHAPES, lambda Cin, Cout: (Cin, Cout, 5, 5)),
    "wino": (WINO_SHAPES, lambda Cout, Cin: (Cout, Cin, 3, 3)),
    "wino_s2": (WINO_S2_SHAPES, lambda Cout, Cs: (Cout, Cs, 5, 5)),
    "wino_convT": (WINO_CONVT_SHAPES, lambda Cin, Cout: (Cin, Cout, 5, 5)),
    "image": (IMAGE_SHAPES, lambda Cin, Cimg: (Cin, Cimg, 5, 5)),
}


def weights(export, shape):
    """The weights both test files pack for `shape` of `export`: the same array on every call."""
    wshape = EXPORTS[export][1](*shape)
    return make_weights(wshape, zlib.crc32(repr((export, tuple(shape))).encode()))


def restate(export, shape, w, mutant=None):
    """The float32 buffer (image: the pair of buffers) of `export` for weights w."""
    if export == "conv":
        return pack_conv_weight(w, shape[0], mutant)
    if export == "convT":
        return pack_convT_weight(w, mutant)
    if export == "image":
        return pack_convT_image_weight(w, *shape, mutant)
    return {"wino": pack_wino_weight, "wino_s2": pack_wino_s2_weight, "wino_convT": pack_wino_convT_weight}[export](
        w, mutant)[0]


def split_inputs(Cout, Cin, nphase):
    """{name: U float32} the split is fed for a shape: a packer's output (3x3 for Cin 32, space-to-depth for Cin 64,
    transposed for four phases) and the hand-made block."""
    if nphase == 4:
        u = pack_wino_convT_weight(weights("wino_convT", (Cin, Cout)))[0]
    elif Cin == 64:
        u = pack_wino_s2_weight(weights("wino_s2", (Cout, Cin // 4)))[0]
    else:
        u = pack_wino_weight(weights("wino", (Cout, Cin)))[0]
    return {"packed": u, "handmade": handmade_u(Cout, Cin, nphase)}
