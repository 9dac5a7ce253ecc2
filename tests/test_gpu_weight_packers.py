"""The weight packers and the packed-weight cache, held to tests/pack_ref.py.

The seven exports that turn a checkpoint's weights into the forms the conv kernels read (dsic_pack_conv_weight,
dsic_pack_convT_weight, dsic_pack_wino_weight, dsic_pack_wino_s2_weight, dsic_pack_wino_convT_weight,
dsic_split_wino_weight_bf16, dsic_pack_convT_image_weight) are called through lib.load() on the current stream, with a
destination of exactly the size the library states, NaN (bf16: 0xFFFF) between sentinel guards, and a source between
NaN guards.  Asserted: the guards are intact, no element is left unwritten, every padding element is +0.0, the whole
buffer is bit-equal to the NumPy restatement (which tests/test_pack_ref_cpu.py ties to the convolution itself), a
second call gives the same bits, and ops.pack_* / ops.split_wino_weight_bf16 return those bits too (which holds the
sizes their wrappers allocate).  The three Winograd packers are also held to |U - U64| <= 5 * 2^-24 A element-wise
(four roundings and their second-order terms; A = |G||g||G^T|).  Every number is derived; none is a measurement.

One level up, layers._ConvBase._cached, Conv2d.packed_wino_slices and GDN.effective decide which packed form a launch
sees.  One small layer per Kernel value that packs: after a parameter is rewritten (load_state_dict, bias.copy_,
beta.copy_, a bias tensor replaced), the module moved, or the arithmetic variant switched, its output bits are those of
a freshly built module in the same state; and the packers run once per weight version and variant, not per forward.
"""
import ctypes
from collections import namedtuple

import numpy as np
import pytest
import torch

import pack_ref as P

pytestmark = pytest.mark.gpu

GUARD_BYTES, GUARD = 4096, 0xA5


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from dsic_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def L():
    from dsic_amd import lib
    return lib.load()


@pytest.fixture(autouse=True)
def _split_variant():
    """Every case starts on the split-bf16 variant (the default) and leaves the process's variant as it found it."""
    from dsic_amd import layers
    was = layers.wino_bf16()
    layers.set_wino_bf16(True)
    yield
    layers.set_wino_bf16(was)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Dest:
    """n_f32 floats, all NaN, followed by n_bf16 bf16 values, all 0xFFFF, between two guards of GUARD bytes."""

    def __init__(self, n_f32, n_bf16=0):
        self.n_f32, self.nbytes = n_f32, 4 * n_f32 + 2 * n_bf16
        self.flat = torch.full((2 * GUARD_BYTES + self.nbytes,), GUARD, dtype=torch.uint8, device="cuda")
        inner = self.flat[GUARD_BYTES:GUARD_BYTES + self.nbytes]
        inner[:4 * n_f32].view(torch.float32).fill_(float("nan"))
        inner[4 * n_f32:].fill_(0xFF)
        assert inner.data_ptr() % 256 == 0
        self.ptr = ctypes.c_void_p(inner.data_ptr())

    def take(self, what):
        """(float32 part, bf16 part as uint16) on the host; fails on a touched guard."""
        host = self.flat.cpu().numpy()
        g, n = GUARD_BYTES, self.nbytes
        assert np.all(host[:g] == GUARD) and np.all(host[g + n:] == GUARD), f"{what}: a store outside the stated size"
        inner = host[g:g + n]
        return inner[:4 * self.n_f32].view(np.float32), inner[4 * self.n_f32:].view(np.uint16)


def _src(a):
    """A device copy of the float32 array between NaN guards; keep the returned tensor alive during the call."""
    a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
    flat = torch.full((a.size + 2048,), float("nan"), dtype=torch.float32, device="cuda")
    t = flat[1024:1024 + a.size]
    t.copy_(torch.from_numpy(a))
    return t


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint16)


def _equal_parts(what, got, want, pads):
    """got, want, pads: (float32 part, uint16 part); pads: boolean masks of the padding elements."""
    for part, g, w, pad in zip(("fp32", "bf16"), got, want, pads):
        assert g.size == w.size, f"{what} {part}: {g.size} elements, the restatement has {w.size}"
        if not g.size:
            continue
        unwritten = np.isnan(g) if g.dtype == np.float32 else (g == 0xFFFF)
        assert not unwritten.any(), f"{what} {part}: {int(unwritten.sum())} of {g.size} elements never written, " \
                                    f"first at {int(np.flatnonzero(unwritten)[0])}"
        bad = _bits(g)[pad] != 0
        assert not bad.any(), f"{what} {part}: {int(bad.sum())} of {int(pad.sum())} padding elements are not +0.0"
        diff = np.flatnonzero(_bits(g) != _bits(w))
        assert diff.size == 0, f"{what} {part}: {diff.size} of {g.size} elements differ from the restatement, first " \
                               f"at flat index {int(diff[0])}: got {g[diff[0]]!r}, restated {w[diff[0]]!r}"


def _hold(what, L, call, dst, want, pads, via_ops):
    """call(pointer) -> status, twice into the same guarded destination; via_ops() -> the ops wrapper's tensor."""
    for attempt in ("first call", "second call"):
        rc = call(dst.ptr)
        assert rc == 0, f"{what}: {L.dsic_last_error().decode(errors='replace')}"
        got = dst.take(what)
        _equal_parts(f"{what} ({attempt})", got, want, pads)
    t = via_ops()
    assert t.is_cuda and t.is_contiguous()
    raw = t.view(torch.uint8).cpu().numpy()
    want_raw = np.concatenate([want[0].view(np.uint8), want[1].view(np.uint8)])
    assert raw.size == want_raw.size, f"{what}: the ops wrapper allocates {raw.size} bytes, the layout has {want_raw.size}"
    assert np.array_equal(raw, want_raw), f"{what}: the ops wrapper returns other bits than the export"
    return got


NONE16 = np.zeros(0, dtype=np.uint16)
NOPAD16 = np.zeros(0, dtype=bool)


def _pad_mask(T, Cout, Cin):
    """The padding elements of [T][ceil(Cin/8)][CoutP][8]."""
    return P._tap_cin8_cout(np.ones((T, Cout, Cin), dtype=np.float32)) == 0


def _w_cuda(w):
    return torch.from_numpy(w).cuda()


# ---------------------------------------------------------------------------------------------------- the packers

@pytest.mark.parametrize("k,Cout,Cin", P.CONV_SHAPES)
def test_pack_conv_weight(L, ops, k, Cout, Cin):
    w = P.weights("conv", (k, Cout, Cin))
    n = int(L.dsic_packed_conv_weight_floats(Cout, Cin, k))
    src = _src(w)
    _hold(f"pack_conv_weight k={k} {Cin}->{Cout}", L,
          lambda d: L.dsic_pack_conv_weight(_ptr(src), d, Cout, Cin, k, _stream()), Dest(n),
          (P.pack_conv_weight(w, k), NONE16), (_pad_mask(k * k, Cout, Cin), NOPAD16),
          lambda: ops.pack_conv_weight(_w_cuda(w)))


@pytest.mark.parametrize("Cin,Cout", P.CONVT_SHAPES)
def test_pack_convT_weight(L, ops, Cin, Cout):
    w = P.weights("convT", (Cin, Cout))
    n = int(L.dsic_packed_conv_weight_floats(Cout, Cin, 5))          # 25 taps
    src = _src(w)
    _hold(f"pack_convT_weight {Cin}->{Cout}", L,
          lambda d: L.dsic_pack_convT_weight(_ptr(src), d, Cin, Cout, _stream()), Dest(n),
          (P.pack_convT_weight(w), NONE16), (_pad_mask(25, Cout, Cin), NOPAD16),
          lambda: ops.pack_convT_weight(_w_cuda(w)))


def _hold_wino(what, L, call, nphase, Cout, Cin, bufs, via_ops):
    u32, u64, A = bufs
    n = nphase * int(L.dsic_wino_weight_floats(Cout, Cin))
    pad = np.tile(_pad_mask(16, Cout, Cin), nphase)
    got, _ = _hold(what, L, call, Dest(n), (u32, NONE16), (pad, NOPAD16), via_ops)
    err = np.abs(got.astype(np.float64) - u64)
    bound = 5 * 2.0 ** -24 * A
    assert np.all(err <= bound), f"{what}: {int((err > bound).sum())} elements outside 5 * 2^-24 A of the float64 U"


@pytest.mark.parametrize("Cout,Cin", P.WINO_SHAPES)
def test_pack_wino_weight(L, ops, Cout, Cin):
    w = P.weights("wino", (Cout, Cin))
    src = _src(w)
    _hold_wino(f"pack_wino_weight {Cin}->{Cout}", L,
               lambda d: L.dsic_pack_wino_weight(_ptr(src), d, Cout, Cin, _stream()), 1, Cout, Cin,
               P.pack_wino_weight(w), lambda: ops.pack_wino_weight(_w_cuda(w)))


@pytest.mark.parametrize("Cout,Cs", P.WINO_S2_SHAPES)
def test_pack_wino_s2_weight(L, ops, Cout, Cs):
    w = P.weights("wino_s2", (Cout, Cs))
    src = _src(w)
    _hold_wino(f"pack_wino_s2_weight {Cs}->{Cout}", L,
               lambda d: L.dsic_pack_wino_s2_weight(_ptr(src), d, Cout, Cs, _stream()), 1, Cout, 4 * Cs,
               P.pack_wino_s2_weight(w), lambda: ops.pack_wino_s2_weight(_w_cuda(w)))


@pytest.mark.parametrize("Cin,Cout", P.WINO_CONVT_SHAPES)
def test_pack_wino_convT_weight(L, ops, Cin, Cout):
    w = P.weights("wino_convT", (Cin, Cout))
    src = _src(w)
    bufs = P.pack_wino_convT_weight(w)
    per = P.wino_weight_floats(Cout, Cin)
    assert all(np.any(bufs[0][p * per:(p + 1) * per] != 0) for p in range(4)), "all four phase blocks carry weights"
    _hold_wino(f"pack_wino_convT_weight {Cin}->{Cout}", L,
               lambda d: L.dsic_pack_wino_convT_weight(_ptr(src), d, Cin, Cout, _stream()), 4, Cout, Cin,
               bufs, lambda: ops.pack_wino_convT_weight(_w_cuda(w)))


@pytest.mark.parametrize("Cout,Cin,nphase", P.SPLIT_SHAPES)
def test_split_wino_weight_bf16(L, ops, Cout, Cin, nphase):
    """Fed a packer's output and a hand-made U: +-0, exact bf16 values (mid = 0), exact ties of both parities, values
    whose remainder ties, negative values, magnitudes 2^-20 .. 2^10.  fp32 denormals and values that round past the
    bf16 range are left out: what the conversion does with them is not something this project relies on.  Checked at
    the plane count the library was built with (dsic_wino_bf16_planes); the other WB_PLANES value is restated and
    checked on the host only (test_pack_ref_cpu.py)."""
    Pn = int(L.dsic_wino_bf16_planes())
    assert Pn in (2, 3)
    nbytes = nphase * int(L.dsic_wino_bf16_weight_bytes(Cout, Cin))
    CoutP = P.round_up(Cout, 32)
    pad = np.zeros((nphase, 16, Cin // 16, Pn, CoutP, 16), dtype=bool)
    pad[..., Cout:, :] = True
    for name, u in P.split_inputs(Cout, Cin, nphase).items():
        src = _src(u)
        _hold(f"split_wino_weight_bf16 {Cin}->{Cout} x{nphase} P={Pn} ({name} U)", L,
              lambda d: L.dsic_split_wino_weight_bf16(_ptr(src), d, Cout, Cin, nphase, _stream()), Dest(0, nbytes // 2),
              (np.zeros(0, dtype=np.float32), P.split_bf16(u, Cout, Cin, nphase, Pn)), (NOPAD16, pad.reshape(-1)),
              lambda: ops.split_wino_weight_bf16(_w_cuda(u), Cout, Cin, nphase))


@pytest.mark.parametrize("Cin,Cimg", P.IMAGE_SHAPES)
def test_pack_convT_image_weight(L, ops, Cin, Cimg):
    w = P.weights("image", (Cin, Cimg))
    n = int(L.dsic_convT_image_weight_floats(Cin))
    assert n % 2 == 0
    first, second = P.pack_convT_image_weight(w, Cin, Cimg)
    pad1 = np.zeros((9, Cin // 16, 16, 16), dtype=bool)
    pad1[:, :, 4 * Cimg:] = True
    pad2 = np.zeros((Cin // 16, 9, 2, 2, 16, 8), dtype=bool)
    pad2[:, :, :, :, 4 * Cimg:] = True
    src = _src(w)
    _hold(f"pack_convT_image_weight {Cin}->{Cimg}", L,
          lambda d: L.dsic_pack_convT_image_weight(_ptr(src), d, Cin, Cimg, _stream()), Dest(n // 2, n),
          (first, second), (pad1.reshape(-1), pad2.reshape(-1)), lambda: ops.pack_convT_image_weight(_w_cuda(w)))


def test_every_refusal_is_returned_and_touches_nothing(L):
    """Each DSIC_REQUIRE of the seven exports: DSIC_EINVAL, its message, a NaN destination left as it was.  Error
    returns only: nothing here reaches a launch."""
    from dsic_amd import lib
    dst = Dest(1 << 16)
    src = _src(np.ones(1 << 14, dtype=np.float32))
    s, d, st = _ptr(src), dst.ptr, _stream()
    null, arg = "null pointer", "bad argument"
    image = "must be a multiple of 16 and Cimg="
    cases = [
        ("conv null w", lambda: L.dsic_pack_conv_weight(None, d, 4, 3, 3, st), "pack_conv_weight: " + null),
        ("conv null dst", lambda: L.dsic_pack_conv_weight(s, None, 4, 3, 3, st), "pack_conv_weight: " + null),
        ("conv k=2", lambda: L.dsic_pack_conv_weight(s, d, 4, 3, 2, st), "pack_conv_weight: bad shape"),
        ("convT null w", lambda: L.dsic_pack_convT_weight(None, d, 8, 4, st), "pack_convT_weight: " + null),
        ("convT null dst", lambda: L.dsic_pack_convT_weight(s, None, 8, 4, st), "pack_convT_weight: " + null),
        ("convT Cin=12", lambda: L.dsic_pack_convT_weight(s, d, 12, 4, st), "pack_convT_weight: Cin must be a multiple of 8"),
        ("wino null w", lambda: L.dsic_pack_wino_weight(None, d, 4, 3, st), "pack_wino_weight: " + arg),
        ("wino null dst", lambda: L.dsic_pack_wino_weight(s, None, 4, 3, st), "pack_wino_weight: " + arg),
        ("wino_s2 null w", lambda: L.dsic_pack_wino_s2_weight(None, d, 36, 8, st), "pack_wino_s2_weight: " + arg),
        ("wino_s2 null dst", lambda: L.dsic_pack_wino_s2_weight(s, None, 36, 8, st), "pack_wino_s2_weight: " + arg),
        ("wino_s2 Cs=12", lambda: L.dsic_pack_wino_s2_weight(s, d, 36, 12, st), "pack_wino_s2_weight: " + arg),
        ("wino_convT null w", lambda: L.dsic_pack_wino_convT_weight(None, d, 8, 36, st), "pack_wino_convT_weight: " + arg),
        ("wino_convT null dst", lambda: L.dsic_pack_wino_convT_weight(s, None, 8, 36, st), "pack_wino_convT_weight: " + arg),
        ("wino_convT Cin=12", lambda: L.dsic_pack_wino_convT_weight(s, d, 12, 36, st), "pack_wino_convT_weight: " + arg),
        ("split null u", lambda: L.dsic_split_wino_weight_bf16(None, d, 36, 32, 1, st), "split_wino_weight_bf16: " + arg),
        ("split null dst", lambda: L.dsic_split_wino_weight_bf16(s, None, 36, 32, 1, st), "split_wino_weight_bf16: " + arg),
        ("split Cin=48", lambda: L.dsic_split_wino_weight_bf16(s, d, 36, 48, 1, st), "split_wino_weight_bf16: " + arg),
        ("split Cin=16", lambda: L.dsic_split_wino_weight_bf16(s, d, 36, 16, 1, st), "split_wino_weight_bf16: " + arg),
        ("split nphase=0", lambda: L.dsic_split_wino_weight_bf16(s, d, 36, 32, 0, st), "split_wino_weight_bf16: " + arg),
        ("split nphase=2", lambda: L.dsic_split_wino_weight_bf16(s, d, 36, 32, 2, st), "split_wino_weight_bf16: " + arg),
        ("image null w", lambda: L.dsic_pack_convT_image_weight(None, d, 16, 3, st), "pack_convT_image_weight: " + null),
        ("image null dst", lambda: L.dsic_pack_convT_image_weight(s, None, 16, 3, st), "pack_convT_image_weight: " + null),
        ("image Cimg=0", lambda: L.dsic_pack_convT_image_weight(s, d, 16, 0, st), image + "0 in [1,4]"),
        ("image Cimg=5", lambda: L.dsic_pack_convT_image_weight(s, d, 16, 5, st), image + "5 in [1,4]"),
        ("image Cin=24", lambda: L.dsic_pack_convT_image_weight(s, d, 24, 3, st), "Cin=24 " + image),
    ]
    for what, call, fragment in cases:
        rc = call()
        msg = L.dsic_last_error().decode(errors="replace")
        assert rc == lib.DSIC_EINVAL, f"{what}: status {rc}, not DSIC_EINVAL ({msg!r})"
        assert fragment in msg, f"{what}: message {msg!r} lacks {fragment!r}"
    torch.cuda.synchronize()
    got, _ = dst.take("refusals")
    assert np.isnan(got).all(), "a refused call wrote to its destination"
    assert bool((src == 1).all())


# ---------------------------------------------------------------------------------------------------- the cache

# One layer per Kernel value that packs, and the transposed forms.  Channel counts and sizes are conv_ref's cases of
# the family (WINO_F32 under the split variant needs Cin < 64: 32 -> 64); the 64-tile layers get the smallest grid the
# kernel takes (four 16x16 work items: 16x64, transposed 16x16 with its four phases).  gdn: a GDN fused behind the layer.
CacheCase = namedtuple("CacheCase", "name kind cin cout k H W kernel gdn s2d packs")
CACHE_CASES = [
    CacheCase("direct", "conv", 8, 24, 3, 17, 13, "DIRECT", False, False, {"pack_conv_weight": 1}),
    CacheCase("wino_f32", "conv", 32, 64, 3, 7, 15, "WINO_F32", False, False, {"pack_wino_weight": 1}),
    CacheCase("bf16_32", "conv", 64, 128, 3, 7, 15, "BF16_32", True, False,
              {"pack_wino_weight": 1, "split_wino_weight_bf16": 1}),
    CacheCase("bf16_64", "conv", 64, 128, 3, 16, 64, "BF16_64", False, False,
              {"pack_wino_weight": 1, "split_wino_weight_bf16": 1}),
    # Cout = 192 as slices of 128 and 64 over the space-to-depth input [1,4,6,4*32]
    CacheCase("slices", "conv", 32, 192, 5, 4, 6, "BF16_32", True, True,
              {"pack_wino_s2_weight": 2, "split_wino_weight_bf16": 2}),
    CacheCase("image", "convT", 48, 3, 5, 3, 5, "IMAGE", False, False, {"pack_convT_image_weight": 1}),
    CacheCase("directT", "convT", 8, 24, 5, 3, 4, "DIRECT", False, False, {"pack_convT_weight": 1}),
    CacheCase("wino_f32T", "convT", 32, 64, 5, 5, 7, "WINO_F32", False, False, {"pack_wino_convT_weight": 1}),
    CacheCase("bf16_32T", "convT", 64, 128, 5, 5, 7, "BF16_32", False, False,
              {"pack_wino_convT_weight": 1, "split_wino_weight_bf16": 1}),
    CacheCase("bf16_64T", "convT", 64, 128, 5, 16, 16, "BF16_64", False, False,
              {"pack_wino_convT_weight": 1, "split_wino_weight_bf16": 1}),
]
PACKERS = ("pack_conv_weight", "pack_convT_weight", "pack_convT_image_weight", "pack_wino_weight",
           "pack_wino_s2_weight", "pack_wino_convT_weight", "split_wino_weight_bf16")
_cache_ids = [c.name for c in CACHE_CASES]


def _state(c, seed):
    """Parameters of the case's layer (and GDN) as a CPU state dict: {"conv.weight", "conv.bias", "gdn.*"}."""
    g = torch.Generator().manual_seed(1000 * seed + len(c.name))
    shape = (c.cout, c.cin, c.k, c.k) if c.kind == "conv" else (c.cin, c.cout, 5, 5)
    K = c.cin * (c.k * c.k if c.kind == "conv" else 6.25)
    sd = {"conv.weight": (torch.rand(shape, generator=g) * 2 - 1) * 2.0 * K ** -0.5,
          "conv.bias": torch.rand(c.cout, generator=g) - 0.5}
    if c.gdn:
        off = 2.0 ** -18
        sd["gdn.beta"] = torch.sqrt(0.5 + torch.rand(c.cout, generator=g) + off)
        gam = torch.sqrt(0.02 + 0.28 * torch.rand(c.cout, generator=g) + off)
        sd["gdn.gamma"] = torch.sqrt(torch.diag(gam ** 2 - off) + off)
        sd["gdn.gamma_conv.weight"] = gam.view(c.cout, 1, 1, 1)
    return sd


def _build(c, sd):
    from dsic_amd import layers
    m = torch.nn.Module()
    m.conv = layers.Conv2d(c.cin, c.cout, c.k, 2 if c.k == 5 else 1) if c.kind == "conv" \
        else layers.ConvTranspose2d(c.cin, c.cout, 5, 2, 2, output_padding=1)
    if c.gdn:
        m.gdn = layers.GDN(c.cout)
    m.load_state_dict(sd, strict=True)
    return m.cuda()


def _x(c):
    g = torch.Generator().manual_seed(77 + len(c.name))
    C = 4 * c.cin if c.s2d else c.cin
    return ((torch.rand((1, c.H, c.W, C), generator=g) * 2 - 1) * 2.0).cuda()


def _forward(c, m, x, expect_kernel=True):
    """The layer's output for x, on the host.  The slice form reads the space-to-depth input while the layer asks for
    it (use_winograd_s2) and the same image in NHWC otherwise, as a chain would hand it over."""
    from dsic_amd import layers, ops
    gdn = m.gdn if c.gdn else None
    act = ops.ACT_GDN if c.gdn else ops.ACT_NONE
    with torch.no_grad():
        if c.s2d and m.conv.use_winograd_s2:
            choice = m.conv.kernel(c.H, c.W, layers.Layout(s2d=True))
            y = m.conv.run_nhwc(x, act, gdn, x_is_s2d=True)
        elif c.s2d:
            choice = None
            y = m.conv.run_nhwc(ops.depth_to_space(x), act, gdn)
        else:
            choice = m.conv.kernel(c.H, c.W)
            y = m.conv.run_nhwc(x, act, gdn)
    if expect_kernel:
        assert choice is not None and choice.kernel is layers.Kernel[c.kernel], (c.name, choice)
    y = y.cpu()
    assert bool(torch.isfinite(y).all()), c.name
    return y


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_the_64_tile_cases_sit_on_the_threshold(L):
    """half the grid is no longer the 64-tile kernel's: the cases use the smallest it takes"""
    assert L.dsic_wino_bf16_m64(16, 64, 64, 1) and not L.dsic_wino_bf16_m64(16, 32, 64, 1)
    assert L.dsic_wino_bf16_m64(16, 16, 64, 4) and not L.dsic_wino_bf16_m64(8, 16, 64, 4)


@pytest.mark.parametrize("c", CACHE_CASES, ids=_cache_ids)
def test_rewritten_weights_reach_the_next_forward(ops, c):
    A, B = _state(c, 1), _state(c, 2)
    x = _x(c)
    m = _build(c, A)
    first = _forward(c, m, x)
    m.load_state_dict(B)
    second = _forward(c, m, x)
    assert not _same(first, second), "the two weight sets must give different outputs"
    assert _same(second, _forward(c, _build(c, B), x)), "after load_state_dict the forward still sees the old weights"
    m.load_state_dict(A)
    assert _same(_forward(c, m, x), first), "loading the first weights back does not give the first bits"


@pytest.mark.parametrize("c", CACHE_CASES, ids=_cache_ids)
def test_a_single_rewritten_parameter_reaches_the_next_forward(ops, c):
    """bias.copy_ alone, beta.copy_ alone, gamma_conv.weight.copy_ alone, and a bias tensor replaced (what
    load_state_dict(assign=True) does to one parameter): the slice form holds bias slices in its cache."""
    A, B = _state(c, 1), _state(c, 2)
    x = _x(c)
    m = _build(c, A)
    last = _forward(c, m, x)
    state = dict(A)
    steps = [("conv.bias", "copy"), ("conv.bias", "replace")]
    if c.gdn:
        steps += [("gdn.beta", "copy"), ("gdn.gamma_conv.weight", "copy")]
    for i, (name, how) in enumerate(steps):
        new = B[name] if i != 1 else B[name] * 0.5 + 0.125
        mod, attr = m.get_submodule(name.rsplit(".", 1)[0]), name.rsplit(".", 1)[1]
        with torch.no_grad():
            if how == "copy":
                getattr(mod, attr).copy_(new.cuda())
            else:
                getattr(mod, attr).data = new.cuda()
        state[name] = new
        got = _forward(c, m, x)
        assert not _same(got, last), f"{name} ({how}): the new value must change the output"
        assert _same(got, _forward(c, _build(c, state), x)), f"{name} ({how}): the forward still sees the old value"
        last = got


@pytest.mark.parametrize("c", CACHE_CASES, ids=_cache_ids)
def test_a_moved_module_gives_the_same_bits(ops, c):
    x = _x(c)
    m = _build(c, _state(c, 1))
    first = _forward(c, m, x)
    m = m.cpu().cuda()
    assert _same(_forward(c, m, x), first)
    # and a rewrite after the move is seen (the caches are keyed on the tensors the module holds now)
    B = _state(c, 2)
    m.load_state_dict(B)
    assert _same(_forward(c, m, x), _forward(c, _build(c, B), x))


@pytest.mark.parametrize("c", CACHE_CASES, ids=_cache_ids)
def test_every_packed_form_follows_the_variant_switch(ops, c):
    from dsic_amd import layers
    A = _state(c, 1)
    x = _x(c)
    m = _build(c, A)
    first = _forward(c, m, x)
    try:
        layers.set_wino_bf16(False)
        off = _forward(c, m, x, expect_kernel=False)
        assert _same(off, _forward(c, _build(c, A), x, expect_kernel=False)), \
            "after the switch the layer does not run what a layer built under the fp32 variant runs"
        if "split_wino_weight_bf16" in c.packs and not c.s2d:
            assert m.conv.kernel(c.H, c.W).kernel is layers.Kernel.WINO_F32
            u = m.conv.packed_wino() if c.kind == "conv" else m.conv.packed()
            assert u.dtype == torch.float32, "the fp32 variant must see fp32 U, not the cached bf16 planes"
            assert not _same(off, first), "the two variants' arithmetic differs"
        if c.s2d:
            assert not m.conv.use_winograd_s2, "only the split kernel stores a Cout slice"
        layers.set_wino_bf16(True)
        assert _same(_forward(c, m, x), first), "back on the split variant the first bits do not return"
        if "split_wino_weight_bf16" in c.packs and not c.s2d:
            u = m.conv.packed_wino() if c.kind == "conv" else m.conv.packed()
            assert u.dtype == torch.uint8
    finally:
        layers.set_wino_bf16(True)


@pytest.mark.parametrize("c", CACHE_CASES, ids=_cache_ids)
def test_packing_happens_once_per_weight_version_and_variant(ops, c, monkeypatch):
    from dsic_amd import layers
    calls = {}

    def counted(name, fn):
        def wrapper(*a, **k):
            calls[name] = calls.get(name, 0) + 1
            return fn(*a, **k)
        return wrapper
    for name in PACKERS:
        monkeypatch.setattr(ops, name, counted(name, getattr(ops, name)))
    x = _x(c)
    m = _build(c, _state(c, 1))
    _forward(c, m, x)
    assert calls == c.packs, "what the first forward packs"
    for _ in range(2):
        _forward(c, m, x)
    assert calls == c.packs, "a later forward packed again"
    if c.gdn:
        assert m.gdn.effective()[0] is m.gdn.effective()[0]
    m.load_state_dict(_state(c, 2))
    for _ in range(2):
        _forward(c, m, x)
    assert calls == {k: 2 * v for k, v in c.packs.items()}, "once more for the new weights, and only once"
    try:
        layers.set_wino_bf16(False)
        before = dict(calls)
        _forward(c, m, x, expect_kernel=False)
        after = dict(calls)
        assert after != before, "the variant is part of the key: the forms are made again"
        _forward(c, m, x, expect_kernel=False)
        assert calls == after, "a later forward under the fp32 variant packed again"
    finally:
        layers.set_wino_bf16(True)
