"""Float64 references of the convolution kernels (csrc/conv_wino*.hip, conv_igemm.hip, conv_first.hip,
convT_image.hip), the per-element envelopes an fp32 / split-bf16 evaluation is entitled to, CPU emulations of both
contractions, the inputs and the case lists.

A helper for tests/test_conv_ref_cpu.py (which anchors it: independent float64 evaluations, the measured peaks behind
the bars R, the derived ceilings, mutant emulations that must fail) and tests/test_gpu_conv_elements.py (which holds
every kernel instance to it element by element).  It restates conv() / ConvTranspose2d(5,2,2,1) / GDN of
layers.py:19-31,83 in torch float64 and the F(2x2,3x3) Winograd mappings of DESIGN.md section 3; it shares no code
with the oracle, the tools or the product package.

Envelopes (float64, per output element, "the quantity a forward error is proportional to"):
  E_dir = |x| (*) |w| + |b|                      direct kernels: the same geometry on absolute values
  E_win = abs-Winograd + |b|                     B^T, G, A^T, data and weights replaced by their absolute values: the
                                                 transforms mix a 4x4 window, so an output's error is relative to its
                                                 tile, not to itself
  E_out = L * bar * E_in + 2^-21 |f(v)|          through the activation f: L = sup |f'| over [v - bar E_in, v + bar E_in]
A device result is judged by |got - ref64| <= bar * E with bar = min(K_GPU * R, ceiling): R is the peak of the CPU
emulation of the same contraction over the test's own inputs (recorded below, re-measured by test_conv_ref_cpu.py),
K_GPU = 2 pays for the MFMA's accumulation order, the ceilings are derived from the number formats.
"""
from __future__ import annotations

import functools
import math
import zlib
from collections import namedtuple

import torch
import torch.nn.functional as F

from rate_ref import f64, gdn64

U32 = 2.0 ** -24
K_GPU = 2.0
ACT_EPS = 2.0 ** -21            # twice the 2^-22 of the v_rsq_f32 epilogue (csrc/common.h:38)

KINDS = ("uniform", "positive", "range", "image")

# Peaks of the CPU emulations, log2 of max |emulation - ref64| / E over every case and kind of the family below: the
# values test_conv_ref_cpu.py measures, as measured (it holds them to +-0.05; the order of every fp32 sum is fixed,
# _mm32, so they do not move with the host's BLAS or thread count).
R_LOG2 = {
    ("first", "fp32", "image"):     -23.335,
    ("first", "fp32", "positive"):  -22.276,
    ("first", "fp32", "range"):     -22.074,
    ("first", "fp32", "uniform"):   -22.910,
    ("first", "split", "image"):    -17.040,
    ("first", "split", "positive"): -17.585,
    ("first", "split", "range"):    -16.601,
    ("first", "split", "uniform"):  -17.385,
    ("igemm", "fp32", "positive"):  -20.244,
    ("igemm", "fp32", "range"):     -21.042,
    ("igemm", "fp32", "uniform"):   -22.385,
    ("image", "fp32", "positive"):  -20.082,
    ("image", "fp32", "range"):     -21.544,
    ("image", "fp32", "uniform"):   -22.569,
    ("image", "split", "positive"): -18.480,
    ("image", "split", "range"):    -17.158,
    ("image", "split", "uniform"):  -18.242,
    ("wino", "fp32", "positive"):   -22.754,
    ("wino", "fp32", "range"):      -23.280,
    ("wino", "fp32", "uniform"):    -25.172,
    ("wino", "split", "positive"):  -20.566,
    ("wino", "split", "range"):     -17.352,
    ("wino", "split", "uniform"):   -20.776,
}


def R(family, contraction, kind):
    return 2.0 ** R_LOG2[(family, contraction, kind)]


def ceiling(contraction, n):
    """What any evaluation of an n-term sum in the format may cost, relative to E: (n + 16) 2^-24 in fp32 (n
    products and additions, 16 for transforms, bias and input conversion); two bf16 planes leave a residual of 2^-17
    per operand and drop mid*mid <= 2^-18: 1.25 * 2^-16 on top."""
    c = (n + 16) * U32
    return c + 1.25 * 2.0 ** -16 if contraction == "split" else c


def bar(family, contraction, kind, n):
    return min(K_GPU * R(family, contraction, kind), ceiling(contraction, n))


# ---------------------------------------------------------------------------------------------------- values

def conv64(x, w, b, k, stride):
    assert k in (3, 5) and stride in (1, 2) and w.shape[-1] == k
    return F.conv2d(f64(x), f64(w), f64(b), stride=stride, padding=(k - 1) // 2)


def convT64(x, w, b):
    return F.conv_transpose2d(f64(x), f64(w), f64(b), stride=2, padding=2, output_padding=1)


def act64(v, act, beta=None, gamma=None):
    """v [B,C,...] float64 -> f(v); act in none / relu / gdn / igdn."""
    if act == "none":
        return v
    if act == "relu":
        return v.clamp(min=0.0)
    return gdn64(v, beta, gamma, act == "igdn")


def act_envelope(v, e_in, act, beta=None, gamma=None):
    """E_out for an input error bound e_in (already bar * E_in) at v: L * e_in + 2^-21 |f(v)|."""
    v, e_in = f64(v), f64(e_in)
    fv = act64(v, act, beta, gamma)
    if act in ("none", "relu"):
        L = torch.ones_like(v)
    else:
        shape = (1, -1) + (1,) * (v.dim() - 2)
        be, ga = f64(beta).view(shape), f64(gamma).view(shape)
        if act == "gdn":        # f' = beta (beta + gamma v^2)^-3/2, decreasing in |v|: the interval's point nearest 0
            a = (v.abs() - e_in).clamp(min=0.0)
            L = be * (be + ga * a * a) ** -1.5
        else:                   # f' = (beta + 2 gamma v^2) / sqrt(beta + gamma v^2), increasing in |v|
            a = v.abs() + e_in
            L = (be + 2.0 * ga * a * a) / torch.sqrt(be + ga * a * a)
    return L * e_in + ACT_EPS * fv.abs()


# ---------------------------------------------------------------------------------------------------- Winograd

_BT = [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]]
_G = [[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]]
_AT = [[1, 1, 1, 0], [0, 1, -1, -1]]


def _planes(t):
    hi = t.bfloat16().float()
    return hi, (t - hi).bfloat16().float()


KB = 4      # fp32 products are accumulated KB terms at a time (an fp32 MFMA takes 2 or 4)


def _mm32(V, U):
    """V @ U in float32 with the sum over n in a fixed order: blocks of KB terms, added one after the other as an
    MFMA chain does.  One torch.bmm over the whole of n would leave the order to the host BLAS, and the measured peaks
    would move with its version and thread count."""
    acc = torch.bmm(V[:, :, :KB], U[:, :KB])
    for k in range(KB, V.shape[2], KB):
        acc = acc + torch.bmm(V[:, :, k:k + KB], U[:, k:k + KB])
    return acc


def pos_gemm(V, U, mode):
    """V [P,T,n] x U [P,n,Co] -> [P,T,Co].  f64 / fp32: one product in the operands' type.  split: hi = bf16(v),
    mid = bf16(v - hi), (hi*mid + mid*hi) + hi*hi, fp32 sums of exact products.  The rest are mutants of split that
    the bar must catch (test_conv_ref_cpu.py): drop_mh5 / drop_hm0 lose one cross product at one Winograd position,
    mid16 loses the activations' mid plane of the first 16 input channels, bf16 keeps one plane."""
    if mode == "f64":
        return torch.bmm(V, U)
    if mode == "fp32":
        return _mm32(V, U)
    (vh, vm), (uh, um) = _planes(V), _planes(U)
    if mode == "bf16":
        return _mm32(vh, uh)
    if mode == "mid16":
        vm = vm.clone()
        vm[:, :, :16] = 0.0
    hm, mh = _mm32(vh, um), _mm32(vm, uh)
    if mode == "drop_mh5":
        mh[5 % V.shape[0]] = 0.0
    elif mode == "drop_hm0":
        hm[0] = 0.0
    else:
        assert mode in ("split", "mid16"), mode
    return (hm + mh) + _mm32(vh, uh)


MUTANTS = ("drop_mh5", "drop_hm0", "mid16", "bf16")


def wino3x3(x, w, mode, absolute=False):
    """3x3 stride-1 'same' correlation by F(2x2,3x3), without bias: x [B,Ci,H,W], w [Co,Ci,3,3].  mode f64 works in
    float64, every other mode in float32 (transforms included, as the kernels and the weight packing do).  absolute:
    the abs-Winograd evaluation behind E_win."""
    dt = torch.float64 if mode == "f64" else torch.float32
    BT, G, AT = (torch.tensor(m, dtype=dt) for m in (_BT, _G, _AT))
    x, w = x.to(dt), w.to(dt)
    if absolute:
        BT, G, AT, x, w = BT.abs(), G.abs(), AT.abs(), x.abs(), w.abs()
    B, Ci, H, W = x.shape
    Co = w.shape[0]
    He, We = H + (H & 1), W + (W & 1)
    th, tw = He // 2, We // 2
    d = F.unfold(F.pad(x, (1, 1 + We - W, 1, 1 + He - H)), kernel_size=4, stride=2).view(B, Ci, 4, 4, th * tw)
    V = torch.einsum("ij,bcjkt,lk->ilbtc", BT, d, BT).reshape(16, B * th * tw, Ci).contiguous()
    U = torch.einsum("ij,ocjk,lk->iloc", G, w, G).reshape(16, Co, Ci).transpose(1, 2).contiguous()
    M = pos_gemm(V, U, mode).view(4, 4, B, th, tw, Co)
    Y = torch.einsum("ij,jkbhwo,lk->bohiwl", AT, M, AT).reshape(B, Co, He, We)
    return Y[:, :, :H, :W]


def s2d_operands(x, w5):
    """conv(Cs,Co,5,2) on even H, W == 3x3 stride-1 over the space-to-depth input: X[(a,b,c)][p,q] = x[c][2p+a][2q+b],
    g[(a,b,c)][u][v] = w6[c][2u+a][2v+b] with the 5x5 weight zero-padded to 6x6 and split in four."""
    X = torch.cat([x[:, :, a::2, b::2] for a in (0, 1) for b in (0, 1)], dim=1)
    w6 = F.pad(w5, (0, 1, 0, 1))
    g = torch.cat([w6[:, :, a::2, b::2] for a in (0, 1) for b in (0, 1)], dim=1)
    return X, g


def convT_phase_weights(w5):
    """ConvTranspose2d(5,2,2,1), w5 [Ci,Co,5,5]: output phase (py,px) is a 3x3 stride-1 conv over the input grid with
    taps g[r][c] = w7[py+4-2r][px+4-2c] (w7: taps 5, 6 zero) -> {(py,px): [Co,Ci,3,3]}."""
    w7 = F.pad(w5, (0, 2, 0, 2))
    out = {}
    for py in (0, 1):
        for px in (0, 1):
            rows, cols = [py + 4 - 2 * r for r in range(3)], [px + 4 - 2 * c for c in range(3)]
            out[(py, px)] = w7[:, :, rows][:, :, :, cols].permute(1, 0, 2, 3).contiguous()
    return out


def _im2col_conv(x, w, k, stride, mode):
    """Direct conv as ONE contraction over n = Ci k^2 (the im2col GEMM), without bias, in float32 under `mode`."""
    B, Ci, H, W = x.shape
    Co = w.shape[0]
    cols = F.unfold(x.float(), kernel_size=k, padding=(k - 1) // 2, stride=stride)          # [B, n, T]
    V = cols.permute(0, 2, 1).reshape(1, -1, Ci * k * k).contiguous()
    U = w.float().reshape(1, Co, Ci * k * k).transpose(1, 2).contiguous()
    Ho, Wo = -(-H // stride), -(-W // stride)
    return pos_gemm(V, U, mode).view(B, Ho, Wo, Co).permute(0, 3, 1, 2)


def evaluate(op, x, w, b, mode, wino, absolute=False):
    """One layer without activation under `mode`, as a Winograd evaluation (wino) or a direct one.
    op: c3 (3x3/s1), c5 (5x5/s2; Winograd: over space-to-depth, even sizes), ct (ConvTranspose2d).
    absolute + mode f64: the envelope (E_win or E_dir) of the same evaluation."""
    dt = torch.float64 if mode == "f64" else torch.float32
    x, w, b = x.to(dt), w.to(dt), b.to(dt)
    if absolute:
        assert mode == "f64"
        b = b.abs()
    if wino:
        if op == "c3":
            y = wino3x3(x, w, mode, absolute)
        elif op == "c5":
            y = wino3x3(*s2d_operands(x, w), mode, absolute)
        else:
            B, _, H, W = x.shape
            y = x.new_zeros(B, w.shape[1], 2 * H, 2 * W)
            for (py, px), g in convT_phase_weights(w).items():
                y[:, :, py::2, px::2] = wino3x3(x, g, mode, absolute)
    elif mode == "f64":
        if absolute:
            x, w = x.abs(), w.abs()
        if op == "ct":
            y = F.conv_transpose2d(x, w, None, stride=2, padding=2, output_padding=1)
        else:
            k = w.shape[-1]
            y = F.conv2d(x, w, None, stride=1 if op == "c3" else 2, padding=(k - 1) // 2)
    else:
        if op == "ct":
            B, _, H, W = x.shape
            y = x.new_zeros(B, w.shape[1], 2 * H, 2 * W)
            for (py, px), g in convT_phase_weights(w).items():
                y[:, :, py::2, px::2] = _im2col_conv(x, g, 3, 1, mode)
        else:
            y = _im2col_conv(x, w, w.shape[-1], 1 if op == "c3" else 2, mode)
    return y + b.view(1, -1, 1, 1)


# ---------------------------------------------------------------------------------------------------- cases

# fam: wino32 (conv_wino.hip / conv_wino_bf16.hip, both variants), wino64 (conv_wino_bf16m.hip), igemm, first, image
# op: c3 / c5 / ct.  H, W: the grid the kernel works on (wino c5: the space-to-depth grid, the image is 2H x 2W;
# igemm c5: the input).  Cin: the kernel's channel count (wino c5: 4 * Cs).  opt: a tuple of flags
#   s2d_out, cm_in, cm_out, u8 (first layer from bytes), splitk, ("slice", coff, cstride), ("B", n, judged...)
Case = namedtuple("Case", "fam op H W Cin Cout act opt")


def _c(fam, op, H, W, Cin, Cout, act, *opt):
    return Case(fam, op, H, W, Cin, Cout, act, tuple(opt))


WINO32_CASES = [
    # 3x3: every H x W, Cin (4, 6, 8, 12 chunks) and Cout once, the four activations.  The two copy-out schedules of
    # the loop (nchunks >= 8, < 8) carry outputs only where a workgroup takes a second item: at the device's grid
    # every workgroup takes one of these cases' <= 27 items, its in-loop stores are dropped offsets and the judged
    # outputs leave through the epilogue.  test_winograd_elements_through_the_ticket_loop caps the grid at 1, 2, 3.
    _c("wino32", "c3", 1, 1, 64, 4, "none"),
    _c("wino32", "c3", 2, 3, 96, 36, "relu"),
    _c("wino32", "c3", 8, 16, 128, 100, "gdn"),
    _c("wino32", "c3", 9, 17, 192, 36, "igdn"),
    _c("wino32", "c3", 7, 15, 64, 128, "gdn"),
    _c("wino32", "c3", 24, 48, 128, 128, "none"),
    # space-to-depth input (MODE 1: zero rows / columns skipped)
    _c("wino32", "c5", 4, 6, 128, 36, "gdn"),
    _c("wino32", "c5", 9, 17, 512, 128, "none"),
    _c("wino32", "c5", 4, 6, 512, 4, "relu"),
    # ConvTranspose2d (MODE 2)
    _c("wino32", "ct", 1, 1, 64, 36, "igdn"),
    _c("wino32", "ct", 5, 7, 192, 128, "relu"),
    _c("wino32", "ct", 9, 17, 64, 128, "none"),
    _c("wino32", "ct", 9, 17, 192, 36, "igdn"),
    # space-to-depth store
    _c("wino32", "c3", 8, 16, 64, 36, "gdn", "s2d_out"),
    _c("wino32", "c3", 10, 18, 128, 128, "relu", "s2d_out"),
    # a channel slice of a wider tensor (split kernel only)
    _c("wino32", "c3", 9, 17, 64, 36, "none", ("slice", 4, 48)),
    # split-K (split kernel only): S = 4, 2, 2
    _c("wino32", "c5", 8, 16, 512, 36, "none", "splitk"),
    _c("wino32", "c3", 16, 16, 128, 128, "gdn", "splitk", "s2d_out"),
    _c("wino32", "c3", 6, 10, 192, 36, "igdn", "splitk", ("slice", 4, 48)),
]

WINO64_CASES = [
    _c("wino64", "c3", 16, 64, 64, 4, "none"),
    _c("wino64", "c3", 64, 16, 96, 36, "gdn"),
    _c("wino64", "c3", 32, 32, 192, 128, "relu", "s2d_out"),
    _c("wino64", "c5", 32, 32, 512, 128, "gdn"),
    _c("wino64", "ct", 16, 16, 128, 36, "igdn"),
    _c("wino64", "ct", 16, 32, 64, 128, "relu"),
    _c("wino64", "c3", 32, 32, 128, 16, "relu", "cm_in", "cm_out"),
    _c("wino64", "c3", 16, 64, 64, 128, "gdn", "cm_out"),
    _c("wino64", "ct", 16, 16, 64, 16, "none", "cm_in", "cm_out"),
    _c("wino64", "c3", 32, 32, 128, 64, "none", ("slice", 64, 192)),
]

# ("inst", template arguments): the conv_igemm_kernel instance the case is meant for (asserted by the GPU test);
# ("B", batch, judged image): the batches to run; every image but the judged one is NaN
IGEMM_CASES = [
    # 3x3 / s1: 16x8x1 with CK 8 in one chunk and NARROW; 8x8x2 with five CK 8 chunks and a ragged batch; 4x4x8 with
    # CK 32; column blocks; 520 workgroups for two column tiles per wave
    _c("igemm", "c3", 17, 13, 8, 24, "gdn", ("inst", "<3,1,16,8,1,8,1,1>")),
    _c("igemm", "c3", 9, 7, 40, 40, "relu", ("inst", "<3,1,8,8,2,8,1,0>"), ("B", 3, 1), ("B", 4, 2)),
    _c("igemm", "c3", 5, 3, 32, 128, "none", ("inst", "<3,1,4,4,8,32,1,0>"), ("B", 9, 1), ("B", 9, 4), ("B", 10, 8)),
    _c("igemm", "c3", 21, 35, 32, 192, "igdn", ("inst", "<3,1,16,8,1,32,1,0>")),
    _c("igemm", "c3", 63, 65, 8, 160, "none", ("inst", "<3,1,16,8,1,8,2,0>"), ("B", 13, 6)),
    # 5x5 / s2: Wo 18 (16x8x1, CK 8); Wo 7 (8x8x2, three CK 8 chunks, NARROW); Wo 4 (4x4x8, CK 8 forced); CK 16 with
    # column blocks; 520 workgroups
    _c("igemm", "c5", 21, 35, 8, 40, "none", ("inst", "<5,2,16,8,1,8,1,0>")),
    _c("igemm", "c5", 17, 13, 24, 24, "gdn", ("inst", "<5,2,8,8,2,8,1,1>"), ("B", 3, 1), ("B", 4, 2)),
    _c("igemm", "c5", 9, 7, 16, 128, "relu", ("inst", "<5,2,4,4,8,8,1,0>"), ("B", 9, 2), ("B", 9, 5), ("B", 10, 8)),
    _c("igemm", "c5", 21, 35, 16, 192, "igdn", ("inst", "<5,2,16,8,1,16,1,0>")),
    _c("igemm", "c5", 127, 129, 8, 160, "none", ("inst", "<5,2,16,8,1,8,2,0>"), ("B", 13, 6)),
    # transposed (the 3x3 / s1 instances with four phases); the last has 528 workgroups
    _c("igemm", "ct", 9, 17, 8, 24, "igdn", ("inst", "<3,1,16,8,1,8,1,1>")),
    _c("igemm", "ct", 9, 7, 40, 40, "relu", ("inst", "<3,1,8,8,2,8,1,0>"), ("B", 3, 1), ("B", 4, 2)),
    _c("igemm", "ct", 3, 4, 32, 128, "none", ("inst", "<3,1,4,4,8,32,1,0>"), ("B", 9, 3), ("B", 9, 6), ("B", 9, 7),
       ("B", 10, 8)),
    _c("igemm", "ct", 7, 9, 32, 192, "igdn", ("inst", "<3,1,16,8,1,32,1,0>")),
    _c("igemm", "ct", 31, 33, 8, 160, "none", ("inst", "<3,1,16,8,1,8,2,0>"), ("B", 11, 5)),
]

FIRST_CASES = [
    _c("first", "c3", 1, 1, 3, 4, "none"),
    _c("first", "c3", 8, 16, 4, 36, "gdn", "u8"),
    _c("first", "c3", 9, 17, 3, 128, "relu"),
    _c("first", "c3", 2, 2, 4, 4, "none", "s2d_out", "u8"),
    _c("first", "c3", 16, 34, 3, 36, "gdn", "s2d_out"),
    _c("first", "c3", 9, 17, 4, 16, "relu", "cm_out", "u8"),
    _c("first", "c3", 16, 34, 3, 16, "none", "cm_out", "s2d_out"),
    _c("first", "c3", 9, 17, 3, 36, "gdn", "u8"),
]

IMAGE_CASES = [      # Cout = Cimg; one tile is IT_H x IT_W = 16 x 32 input pixels
    _c("image", "ct", 1, 1, 16, 1, "none"),
    _c("image", "ct", 16, 32, 48, 3, "none"),
    _c("image", "ct", 17, 33, 128, 4, "none"),
    _c("image", "ct", 17, 33, 16, 3, "none"),
]

ALL_CASES = WINO32_CASES + WINO64_CASES + IGEMM_CASES + FIRST_CASES + IMAGE_CASES


def case_id(c):
    opt = "-".join(o if isinstance(o, str) else "".join(str(v) for v in o) for o in c.opt
                   if isinstance(o, str) or o[0] != "inst")
    return f"{c.fam}-{c.op}-{c.H}x{c.W}-{c.Cin}to{c.Cout}-{c.act}" + ("-" + opt if opt else "")


def slice_of(c):
    for o in c.opt:
        if not isinstance(o, str) and o[0] == "slice":
            return o[1], o[2]
    return None


def instance_of(c):
    return next(o[1] for o in c.opt if not isinstance(o, str) and o[0] == "inst")


def batches_of(c):
    b = [(o[1], o[2]) for o in c.opt if not isinstance(o, str) and o[0] == "B"]
    return b or [(3, 1)]


def is_wino(c):
    return c.fam.startswith("wino")


def family(c):
    return "wino" if is_wino(c) else c.fam


def contractions(c):
    """The arithmetic variants a case runs: fp32 and split, where the kernel family has both."""
    if c.fam == "igemm":
        return ("fp32",)
    if c.fam == "wino64" or slice_of(c) or "splitk" in c.opt:
        return ("split",)
    return ("fp32", "split")


def contraction_length(c):
    if is_wino(c):
        return c.Cin
    return c.Cin * (25 if c.op == "c5" else 9)


def image_shape(c):
    """(channels, H, W) of the NCHW tensor the reference convolves."""
    if is_wino(c) and c.op == "c5":
        return c.Cin // 4, 2 * c.H, 2 * c.W
    return c.Cin, c.H, c.W


def kinds_of(c):
    if "u8" in c.opt:
        return ("image",)
    _, H, W = image_shape(c)
    many_blocks = (-(-H // 8)) * (-(-W // 8)) >= 2
    return ("uniform", "positive", "range") if many_blocks else ("uniform", "positive")


def judged_pairs(cases=None):
    """Every (case, kind, contraction) the GPU test judges."""
    return [(c, k, v) for c in (cases or ALL_CASES) for k in kinds_of(c) for v in contractions(c)]


# ---------------------------------------------------------------------------------------------------- inputs

def case_seed(c, kind):
    """From what defines the data (not from the expected instance, which is a note on the case)."""
    opt = tuple(o for o in c.opt if isinstance(o, str) or o[0] != "inst")
    return zlib.crc32(repr((tuple(c._replace(opt=opt)), kind)).encode())


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _sign(shape, g):
    return torch.randint(0, 2, shape, generator=g).float() * 2.0 - 1.0


def make_x(kind, C, H, W, seed):
    """[1,C,H,W] float32, or for kind image [1,H,W,C] uint8."""
    g = _gen(seed)
    if kind == "uniform":
        return (torch.rand((1, C, H, W), generator=g) * 2 - 1) * 2.0
    if kind == "positive":
        return 0.25 + torch.rand((1, C, H, W), generator=g)
    if kind == "range":
        # 2^(e_block + e_channel) with a random significand and sign: e_block spans [-12, 4] over the 8x8 blocks in
        # equal steps (randomly placed, so that two blocks already differ by 2^16), e_channel uniform in [-3, 3]
        nby, nbx = -(-H // 8), -(-W // 8)
        nb = nby * nbx
        eb = torch.linspace(-12.0, 4.0, nb) if nb > 1 else torch.tensor([-4.0])
        eb = eb[torch.randperm(nb, generator=g)].view(nby, nbx)
        eb = eb.repeat_interleave(8, 0).repeat_interleave(8, 1)[:H, :W]
        ec = torch.rand(C, generator=g) * 6.0 - 3.0
        mag = torch.exp2(eb.view(1, 1, H, W) + ec.view(1, C, 1, 1)) * (1.0 + torch.rand((1, C, H, W), generator=g))
        return _sign((1, C, H, W), g) * mag
    if kind == "image":
        x = torch.randint(0, 256, (1, H, W, C), generator=g, dtype=torch.int64)
        col = torch.arange(W).view(1, 1, W, 1).expand(1, H, W, C)
        x = torch.where(3 * col < W, torch.zeros_like(x), x)           # flat at 0
        x = torch.where(3 * col >= 2 * W, torch.full_like(x, 255), x)  # flat at 255
        return x.to(torch.uint8)
    raise ValueError(kind)


def make_w(kind, shape, cin_axis, K, seed):
    g = _gen(seed)
    if kind in ("uniform", "image"):
        return (torch.rand(shape, generator=g) * 2 - 1) * (2.0 * K ** -0.5)
    if kind == "positive":
        return (0.25 + torch.rand(shape, generator=g)) * K ** -0.5
    view = [1] * len(shape)
    view[cin_axis] = shape[cin_axis]
    ec = (torch.rand(shape[cin_axis], generator=g) * 6.0 - 3.0).view(view)
    return _sign(shape, g) * torch.exp2(ec) * (1.0 + torch.rand(shape, generator=g)) * K ** -0.5


def make_bias(kind, Cout, seed):
    g = _gen(seed)
    if kind == "positive":
        return 0.05 + 0.45 * torch.rand(Cout, generator=g)
    b = (torch.rand(Cout, generator=g) - 0.5)
    b = torch.where(b.abs() < 1e-3, torch.full_like(b, 0.25), b)       # E > 0 wherever the data are all zero
    return b * 2.0 ** -12 if kind == "range" else b


def make_inputs(c, kind):
    """x (float32 [1,C,H,W]; kind image: uint8 [1,H,W,C]), w (the reference's layout), b, beta, gamma (effective)."""
    C, H, W = image_shape(c)
    s = case_seed(c, kind)
    k = 5 if c.op in ("c5", "ct") else 3
    if c.op == "ct":
        wshape, cin_axis, K = (C, c.Cout, 5, 5), 0, C * 6.25
    else:
        wshape, cin_axis, K = (c.Cout, C, k, k), 1, C * k * k
    g = _gen(s + 4)
    return {"x": make_x(kind, C, H, W, s), "w": make_w(kind, wshape, cin_axis, K, s + 1),
            "b": make_bias(kind, c.Cout, s + 2),
            "beta": 0.5 + torch.rand(c.Cout, generator=g), "gamma": 0.02 + 0.28 * torch.rand(c.Cout, generator=g)}


def x_as_float64(x):
    """Exact widening; image bytes are x / 255 in float64 (to_tensor)."""
    if x.dtype == torch.uint8:
        return x.permute(0, 3, 1, 2).to(torch.float64) / 255.0
    return x.to(torch.float64)


def x_as_float32(x):
    """What an fp32 evaluation starts from: the bytes' float(v) / 255 rounded to float32."""
    if x.dtype == torch.uint8:
        return x.permute(0, 3, 1, 2).float() / 255.0
    return x


@functools.lru_cache(maxsize=None)
def reference(c, kind):
    """Inputs, the float64 layer output before the activation (v) and its envelope (E), [1,Cout,Ho,Wo]: computed
    once per (case, kind), never modified."""
    inp = make_inputs(c, kind)
    x = x_as_float64(inp["x"])
    if c.op == "ct":
        v = convT64(x, inp["w"], inp["b"])
    else:
        k = inp["w"].shape[-1]
        v = conv64(x, inp["w"], inp["b"], k, 1 if k == 3 else 2)
    E = evaluate(c.op, x, inp["w"], inp["b"], "f64", is_wino(c), absolute=True)
    assert v.shape == E.shape
    return inp, v, E


def emulate(c, kind, mode):
    """The CPU emulation of the case's contraction under `mode` (fp32, split or a mutant), float32, no activation."""
    inp = make_inputs(c, kind)
    return evaluate(c.op, x_as_float32(inp["x"]), inp["w"], inp["b"], mode, is_wino(c))


def old_bar_factor(c, v, E, new_bar):
    """How far the global-maximum bar of test_gpu_conv.py sits above the per-element one: its tolerance
    2e-6 |ref|max max(1, sqrt(K)/8) * f (f = 6 Winograd fp32, 24 split; 4 / 16 direct) over the median new one."""
    K = contraction_length(c) * (9 if is_wino(c) else 1)
    tol = 2e-6 * float(v.abs().max()) * max(1.0, math.sqrt(K) / 8.0)
    return tol / float((new_bar * E).median())
