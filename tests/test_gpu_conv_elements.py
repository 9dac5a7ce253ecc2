"""Every conv kernel instance, export by export, against the float64 reference of tests/conv_ref.py.

tests/test_gpu_conv.py holds these kernels to one number per case (the largest error against the tensor's largest
value, on zero-mean noise, in outputs from torch.empty).  Here every output ELEMENT is held to its own envelope,
|device - float64| <= bar * E through the activation (conv_ref.py; the bars are the measured peaks of CPU emulations of
the same contraction, test_conv_ref_cpu.py), on zero-mean, all-positive and wide-range inputs and on image bytes, at one
shape per branch of the dispatch.  Every buffer the kernel sees sits between guards: outputs start as NaN between
sentinels (an element never written or a store outside the tensor fails), inputs, weights, bias, beta and gamma sit
between NaN guards (a read past a tensor poisons the result), and the judged image is the only finite image of its
batch (a read from a neighbouring image poisons it).  A second call and the judged image alone (B = 1) give the same
bits; after each Winograd call the ticket is zero.  The Winograd cases run once more with the persistent grid capped
at 1, 2 and 3 workgroups (dsic_wino_grid), where a workgroup takes item after item and the outputs of one tile leave
during the next one's phases: the bits must be those of the device's grid.
"""
import contextlib
import math

import pytest
import torch

import conv_ref as R

pytestmark = pytest.mark.gpu

SENTINEL, OUTSIDE = -777.0, -7.0
ACT = {"none": 0, "gdn": 1, "igdn": 2, "relu": 3}
_worst = {}          # (family, contraction, kind) -> largest |device - float64| / E over the cases without GDN / IGDN
_seen = set()        # kernel instances run


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from dsic_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def L():
    from dsic_amd import lib
    return lib.load()


def _guard_len(W, C):
    return (max(4096, 16 * W * C) + 15) // 16 * 16


class Guarded:
    """A tensor of `shape` between two guards of `glen` elements (a multiple of 16 floats: the 16-byte alignment of
    the interior is the allocation's)."""

    def __init__(self, shape, glen, inner, guard, dtype=torch.float32):
        self.shape, self.n, self.g, self.guard = tuple(shape), math.prod(shape), glen, guard
        self.flat = torch.empty(self.n + 2 * glen, dtype=dtype, device="cuda")
        self.flat[:glen] = guard
        self.flat[glen + self.n:] = guard
        self.t = self.flat[glen:glen + self.n].view(self.shape)
        if isinstance(inner, torch.Tensor):
            self.t.copy_(inner.reshape(self.shape))
        else:
            self.t.fill_(inner)
        assert self.t.data_ptr() % 16 == 0

    def take(self, what):
        """The interior on the host; fails on a touched guard."""
        host = self.flat.cpu()
        assert bool((host[:self.g] == self.guard).all()) and bool((host[self.g + self.n:] == self.guard).all()), \
            f"{what}: a store outside the tensor"
        return host[self.g:self.g + self.n].view(self.shape)

    def untouched(self):
        host = self.flat.cpu()
        return bool((host[:self.g] == self.guard).all()) and bool((host[self.g + self.n:] == self.guard).all()) \
            and bool(torch.isnan(host[self.g:self.g + self.n]).all())


def _out(shape, W, cstride):
    return Guarded(shape, _guard_len(W, cstride), float("nan"), SENTINEL)


def _in(t, W=1, C=1):
    """A device copy of t between NaN guards (bytes: 0xFF, a NaN where two of them are read as bf16)."""
    if t is None:
        return None
    if t.dtype == torch.uint8:
        return Guarded(t.shape, 4 * _guard_len(W, C), t, 255, torch.uint8).t
    return Guarded(t.shape, _guard_len(W, C), t, float("nan")).t


def _batch(img, B, j):
    """[B, *img.shape]: image j = img, every other image NaN (bytes: 255)."""
    if img.dtype == torch.uint8:
        x = torch.full((B,) + tuple(img.shape), 255, dtype=torch.uint8)
    else:
        x = torch.full((B,) + tuple(img.shape), float("nan"))
    x[j] = img
    return x


def _s2d(hwc):
    H2, W2, C = hwc.shape
    return hwc.view(H2 // 2, 2, W2 // 2, 2, C).permute(0, 2, 1, 3, 4).reshape(H2 // 2, W2 // 2, 4 * C)


def _d2s(hwc4):
    H, W, C4 = hwc4.shape
    return hwc4.view(H, W, 2, 2, C4 // 4).permute(0, 2, 1, 3, 4).reshape(2 * H, 2 * W, C4 // 4)


def _cm(hwc):
    H, W, C = hwc.shape
    return hwc.view(H, W, C // 16, 16).permute(2, 0, 1, 3).contiguous()


def _uncm(chw16):
    CC, H, W, _ = chw16.shape
    return chw16.permute(1, 2, 0, 3).reshape(H, W, 16 * CC)


def _out_shape(c, B, Ho, Wo):
    """The output tensor of a case and its width and channel stride for the guards."""
    s2d, cm, sl = "s2d_out" in c.opt, "cm_out" in c.opt, R.slice_of(c)
    H, W, C = (Ho // 2, Wo // 2, 4 * c.Cout) if s2d else (Ho, Wo, c.Cout)
    if sl:
        C = sl[1]
    return ((B, C // 16, H, W, 16) if cm else (B, H, W, C)), W, C


def _judged_chw(c, host, j):
    """Image j of the output tensor as [Cout,Ho,Wo], and what lies outside a channel slice."""
    img, outside = host[j], None
    if "cm_out" in c.opt:
        img = _uncm(img)
    sl = R.slice_of(c)
    if sl:
        outside = torch.cat([img[..., :sl[0]], img[..., sl[0] + c.Cout:]], dim=-1)
        img = img[..., sl[0]:sl[0] + c.Cout]
    if "s2d_out" in c.opt:
        img = _d2s(img.contiguous())
    return img.permute(2, 0, 1).contiguous(), outside


def _judge(c, kind, contraction, got, what):
    """Every element of got [Cout,Ho,Wo] inside its envelope; notes the worst error in units of E."""
    inp, v, E = R.reference(c, kind)
    assert got.shape == v.shape[1:], (what, got.shape, v.shape)
    bad = torch.isnan(got).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.shape[0]} of {got.numel()} elements never written or poisoned by a read " \
                             f"outside the image, first at (channel, row, col) {tuple(bad[0].tolist())}"
    b = R.bar(R.family(c), contraction, kind, R.contraction_length(c))
    want = R.act64(v, c.act, inp["beta"], inp["gamma"])[0]
    env = R.act_envelope(v, b * E, c.act, inp["beta"], inp["gamma"])[0]
    err = (got.double() - want).abs()
    ratio = err / env
    worst = float(ratio.max())
    key = (R.family(c), contraction, kind)
    # for the report: the error in units of E with nothing granted to the activation, so that it compares with the
    # emulation's peak as it is; taken where the output is the contraction's own (no activation or ReLU: behind a
    # GDN the rounding of f(v) itself is no part of it)
    if c.act in ("none", "relu"):
        _worst[key] = max(_worst.get(key, 0.0), float((err / E[0]).max()))
    print(f"{what}: worst |device - float64| / envelope {worst:.3f} (bar 2^{math.log2(b):.2f} of E)")
    at = tuple((ratio == ratio.max()).nonzero()[0].tolist())
    assert worst <= 1.0, f"{what}: {int((ratio > 1).sum())} elements outside the envelope, worst {worst:.2f}x at " \
                         f"(channel, row, col) {at}: got {float(got[at])!r}, float64 {float(want[at])!r}"


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _act_args(c, inp):
    if c.act in ("gdn", "igdn"):
        return ACT[c.act], _in(inp["beta"]), _in(inp["gamma"])
    return ACT[c.act], None, None


def _check_run(c, kind, contraction, what, run, batches):
    """run(B, j) -> (Guarded output after one call, a function that calls again on the same buffers).  Judges image j
    of every batch, the second call and the image alone."""
    first = None
    for B, j in batches:
        out, launch = run(B, j)
        got, outside = _judged_chw(c, out.take(what), j)
        _judge(c, kind, contraction, got, f"{what} B={B} image {j}")
        if outside is not None:
            assert bool((outside == OUTSIDE).all()), f"{what}: a store outside the channel slice"
        launch()
        again, _ = _judged_chw(c, out.take(what), j)
        assert _same_bits(again, got), f"{what}: a second call on the same buffers gives other bits"
        if first is None:
            first = got
        else:
            assert _same_bits(got, first), f"{what}: the bits depend on the image's place in the batch (B={B}, {j})"
    solo, _ = _judged_chw(c, run(1, 0)[0].take(what), 0)
    assert _same_bits(solo, first), f"{what}: the image alone gives other bits than in the batch"


# ---------------------------------------------------------------------------------------------------- Winograd

def _wino_run(ops, L, c, kind, contraction):
    inp, v, _ = R.reference(c, kind)
    split = contraction == "split"
    x = inp["x"][0].permute(1, 2, 0).contiguous()                       # [Hx,Wx,C]
    if c.op == "c5":
        x = _s2d(x)
    assert x.shape == (c.H, c.W, c.Cin)
    if "cm_in" in c.opt:
        x = _cm(x)
    w = inp["w"].cuda()
    nphase = 4 if c.op == "ct" else 1
    u = {"c3": ops.pack_wino_weight, "c5": ops.pack_wino_s2_weight, "ct": ops.pack_wino_convT_weight}[c.op](w)
    if split:
        u = ops.split_wino_weight_bf16(u, c.Cout, c.Cin, nphase)
    u = _in(u.cpu())
    bias = _in(inp["b"])
    act, beta, gamma = _act_args(c, inp)
    Ho, Wo = v.shape[2:]
    sl = R.slice_of(c)
    # the instance this case is meant for
    m64 = bool(L.dsic_wino_bf16_m64(c.H, c.W, c.Cin, nphase)) and split
    S = L.dsic_wino_bf16_ksplit(c.H, c.W, c.Cin) if "splitk" in c.opt else 1
    assert m64 == (c.fam == "wino64"), (c, m64)
    if "splitk" in c.opt:
        assert split and c.op != "ct" and S == {512: 4, 128: 2, 192: 2}[c.Cin] and ops.WINO_SPLITK, (c, S)
    mode = {"c3": 0, "c5": 1, "ct": 2}[c.op]
    _seen.add((f"conv_wino_bf16{'m' if m64 else ''}_kernel<{mode}>" if split else f"conv_wino_kernel<{mode}>")
              + (f" split-K {S}" if S > 1 else "") + f" {c.Cin // 16} chunks")

    def run(B, j):
        xd = _in(_batch(x, B, j), c.W, c.Cin)
        shape, W, C = _out_shape(c, B, Ho, Wo)
        out = _out(shape, W, C)
        if sl:
            out.t[..., :sl[0]] = OUTSIDE
            out.t[..., sl[0] + c.Cout:] = OUTSIDE
        cm = dict(cm_in="cm_in" in c.opt, cm_out="cm_out" in c.opt)

        def launch():
            if c.op == "ct":
                ops.conv_transpose2d_wino_nhwc(xd, u, bias, c.Cout, act, beta, gamma, out=out.t, **cm)
            else:
                ops.conv3x3_wino_nhwc(xd, u, bias, c.Cout, act, beta, gamma, out=out.t, s2d_out="s2d_out" in c.opt,
                                      s2d_in=c.op == "c5", out_coff=sl[0] if sl else 0, split_k="splitk" in c.opt,
                                      **cm)
            torch.cuda.synchronize()
            assert not bool(ops._ticket(xd.device).any()), "the ticket is not zero after the call"
        launch()
        return out, launch
    return run


@pytest.mark.parametrize("c", R.WINO32_CASES + R.WINO64_CASES, ids=R.case_id)
def test_winograd_elements(ops, L, c):
    for kind in R.kinds_of(c):
        for contraction in R.contractions(c):
            what = f"{R.case_id(c)} {kind} {contraction}"
            _check_run(c, kind, contraction, what, _wino_run(ops, L, c, kind, contraction), R.batches_of(c))


@pytest.fixture
def wino_grid(L):
    """dsic_wino_grid, with the cap that was set before the test back in place afterwards (after a failure too)."""
    was = L.dsic_wino_grid(-1)
    yield L.dsic_wino_grid
    L.dsic_wino_grid(was)


def _wino_items(L, c, B):
    """Work items of a launch over B images, as the launch code counts them (wino_launch in conv_wino.hip and
    wb_launch in conv_wino_bf16.hip: 16x8-pixel tiles, times the split-K factor; dsic_wbm_launch in
    conv_wino_bf16m.hip: 16x16-pixel tiles; a transposed layer has four phase items per tile)."""
    nphase = 4 if c.op == "ct" else 1
    if c.fam == "wino64":
        assert c.H % 16 == 0 and c.W % 16 == 0
        return (c.H // 16) * (c.W // 16) * B * nphase
    S = L.dsic_wino_bf16_ksplit(c.H, c.W, c.Cin) if "splitk" in c.opt else 1
    return -(-c.H // 8) * (-(-c.W // 16)) * B * nphase * S


# test_winograd_elements runs every case at the device's grid, min(items, CUs): with at most 27 items each workgroup
# takes one, copies nothing out inside its loop and leaves through the epilogue behind a prologue that no item
# precedes.  Here the grid is capped at 1, 2 and 3 workgroups, so that a workgroup walks from item to item: the judged
# image is the first item a workgroup ever takes (7, 0: the prologue, then its outputs leave during a NaN successor's
# phases), the last (7, 6: a NaN predecessor, the epilogue) and one in the middle (3, 1).  An output element is the
# work of one item (of S partial sums added in fixed order by the second launch), so the bits are those of the
# default grid, which are judged against float64 once.
@pytest.mark.parametrize("grid", [1, 2, 3])
@pytest.mark.parametrize("c", R.WINO32_CASES + R.WINO64_CASES, ids=R.case_id)
def test_winograd_elements_through_the_ticket_loop(ops, L, wino_grid, c, grid):
    items = _wino_items(L, c, 7)                                         # of the batches (7, 0) and (7, 6)
    assert items >= 2 * grid + 1, f"{items} items on {grid} workgroups: none takes a third item"
    for kind in R.kinds_of(c):
        for contraction in R.contractions(c):
            what = f"{R.case_id(c)} {kind} {contraction}"
            run = _wino_run(ops, L, c, kind, contraction)
            wino_grid(0)
            ref, _ = _judged_chw(c, run(3, 1)[0].take(what), 1)
            _judge(c, kind, contraction, ref, f"{what} default grid")
            assert wino_grid(grid) == 0 and wino_grid(-1) == grid
            for B, j in ((3, 1), (7, 0), (7, 6)):
                where = f"{what} grid {grid} B={B} image {j}"
                out, launch = run(B, j)                                  # the launch checks the ticket
                got, outside = _judged_chw(c, out.take(where), j)         # take checks the guards
                if outside is not None:
                    assert bool((outside == OUTSIDE).all()), f"{where}: a store outside the channel slice"
                bad = torch.isnan(got).nonzero()
                assert bad.numel() == 0, f"{where}: {bad.shape[0]} of {got.numel()} elements never written or " \
                                         f"poisoned, first at (channel, row, col) {tuple(bad[0].tolist())}"
                diff = (got.view(torch.int32) != ref.view(torch.int32)).nonzero()
                assert _same_bits(got, ref), f"{where}: {diff.shape[0]} of {got.numel()} elements differ from the " \
                                             f"default grid's, first at (channel, row, col) {tuple(diff[0].tolist())}"
                launch()
                again, outside = _judged_chw(c, out.take(where), j)
                assert _same_bits(again, got), f"{where}: a second call on the same buffers gives other bits"
                if outside is not None:
                    assert bool((outside == OUTSIDE).all()), f"{where}: a store outside the channel slice"


# ---------------------------------------------------------------------------------------------------- implicit GEMM

_tile_places = {}   # tile shape -> places of the judged image inside a tile group, over all cases


@pytest.mark.parametrize("c", R.IGEMM_CASES, ids=R.case_id)
def test_implicit_gemm_elements(ops, c):
    instance = R.instance_of(c)
    k, stride = (5, 2) if c.op == "c5" else (3, 1)
    for kind in R.kinds_of(c):
        inp, v, _ = R.reference(c, kind)
        x = inp["x"][0].permute(1, 2, 0).contiguous()
        w = inp["w"].cuda()
        wp = _in((ops.pack_convT_weight(w) if c.op == "ct" else ops.pack_conv_weight(w)).cpu())
        bias = _in(inp["b"])
        act, beta, gamma = _act_args(c, inp)
        Ho, Wo = v.shape[2:]
        Wg, Hg = (c.W, c.H) if c.op == "ct" else (Wo, Ho)               # the grid the tiles cover
        tn = 1 if Wg > 8 else (2 if Wg > 4 else 8)

        def run(B, j):
            if B > 1:
                name = ops._conv_kernel_name(3 if c.op == "ct" else k, stride if c.op != "ct" else 1, Wg, c.Cin,
                                             ops.round_up(c.Cout, 32), Hg, B, 4 if c.op == "ct" else 1)
                assert name == "conv_igemm_kernel" + instance, (name, instance)
                _seen.add(name + (" transposed" if c.op == "ct" else ""))
                _tile_places.setdefault(tn, set()).add(j % tn)
            xd = _in(_batch(x, B, j), c.W, c.Cin)
            out = _out((B, Ho, Wo, c.Cout), Wo, c.Cout)

            def launch():
                if c.op == "ct":
                    ops.conv_transpose2d_nhwc(xd, wp, bias, c.Cout, act, beta, gamma, out=out.t)
                else:
                    ops.conv2d_nhwc(xd, wp, bias, c.Cout, k, stride, act, beta, gamma, out=out.t)
                torch.cuda.synchronize()
            launch()
            return out, launch
        _check_run(c, kind, "fp32", f"{R.case_id(c)} {kind}", run, R.batches_of(c))


def test_implicit_gemm_tile_places():
    """Over all cases the judged image stood at every place of a tile group (8x8x2: 2 places, 4x4x8: 8).  Reads what
    test_implicit_gemm_elements noted: run the module whole, in file order, in one process."""
    assert _tile_places.get(2) == {0, 1} and _tile_places.get(8) == set(range(8)), _tile_places


# ---------------------------------------------------------------------------------------------------- first layer

@contextlib.contextmanager
def _variant(contraction):
    """The library's arithmetic variant for the first and the image layer, restored on the way out."""
    from dsic_amd import layers
    before = layers.wino_bf16()
    try:
        layers.set_wino_bf16(contraction == "split")
        assert layers.WINO_BF16 == (contraction == "split")
        yield
    finally:
        layers.set_wino_bf16(before)


@pytest.mark.parametrize("c", R.FIRST_CASES, ids=R.case_id)
def test_first_layer_elements(ops, L, c):
    from dsic_amd import lib
    flag = int("s2d_out" in c.opt) | (ops.LAYOUT_CM16 if "cm_out" in c.opt else 0)
    fn = L.dsic_conv_first_u8hwc if "u8" in c.opt else L.dsic_conv_first_nchw
    for contraction in R.contractions(c):
        for kind in R.kinds_of(c):
            inp, v, _ = R.reference(c, kind)
            x = inp["x"][0]                                              # float [C,H,W] or bytes [H,W,C]
            assert (x.dtype == torch.uint8) == ("u8" in c.opt)
            w, bias = _in(inp["w"]), _in(inp["b"])
            act, beta, gamma = _act_args(c, inp)
            _seen.add(f"conv_first_kernel<{c.Cin}> {contraction}" + (" bytes" if "u8" in c.opt else ""))

            def run(B, j):
                xd = _in(_batch(x, B, j), c.W, c.Cin)
                shape, W, C = _out_shape(c, B, c.H, c.W)
                out = _out(shape, W, C)

                def launch():
                    lib.check(fn(ops._p(xd), ops._p(w), ops._p(bias), ops._p(beta), ops._p(gamma), ops._p(out.t), B,
                                 c.Cin, c.H, c.W, c.Cout, act, flag, ops._stream()), "conv_first")
                    torch.cuda.synchronize()
                launch()
                return out, launch
            with _variant(contraction):
                _check_run(c, kind, contraction, f"{R.case_id(c)} {kind} {contraction}", run, R.batches_of(c))


# ---------------------------------------------------------------------------------------------------- image layer

@pytest.mark.parametrize("c", R.IMAGE_CASES, ids=R.case_id)
def test_image_layer_elements(ops, c):
    for contraction in R.contractions(c):
        for kind in R.kinds_of(c):
            inp, v, _ = R.reference(c, kind)
            x = inp["x"][0].permute(1, 2, 0).contiguous()
            wp = _in(ops.pack_convT_image_weight(inp["w"].cuda()).cpu())
            bias = _in(inp["b"])
            _seen.add(f"convT_image_kernel {contraction} Cin {c.Cin}")
            what = f"{R.case_id(c)} {kind} {contraction}"

            def run(B, j):
                xd = _in(_batch(x, B, j), c.W, c.Cin)
                out = _out((B, c.Cout, 2 * c.H, 2 * c.W), 2 * c.W, c.Cout)

                def launch():
                    ops.conv_transpose2d_image(xd, wp, bias, c.Cout, out=out.t)
                    torch.cuda.synchronize()
                    return out.take(what)[j]
                return launch
            with _variant(contraction):
                launch = run(3, 1)
                got = launch()
                _judge(c, kind, contraction, got, what)
                assert _same_bits(launch(), got), f"{what}: a second call on the same buffers gives other bits"
                assert _same_bits(run(1, 0)(), got), f"{what}: the image alone gives other bits than in the batch"


# ---------------------------------------------------------------------------------------------------- refusals

def test_refusals_leave_the_output_untouched(ops, L):
    """Each documented requirement of the Winograd and first-layer exports that no other test triggers: ValueError,
    nothing stored."""
    dummy_f = torch.zeros(1 << 20, device="cuda")
    dummy_u = torch.zeros(1 << 22, dtype=torch.uint8, device="cuda")
    b = torch.zeros(256, device="cuda")

    def refused(match, fn, x_shape, out_shape, *args, **kw):
        x = torch.zeros(x_shape, device="cuda")
        out = _out(out_shape, out_shape[-2], out_shape[-1])
        with pytest.raises(ValueError, match=match):
            fn(x, *args, out=out.t, **kw)
        torch.cuda.synchronize()
        assert out.untouched(), match
        assert not bool(ops._ticket(x.device).any())

    for u in (dummy_f, dummy_u):
        refused("multiple of 4", ops.conv3x3_wino_nhwc, (1, 8, 16, 64), (1, 8, 16, 6), u, b, 6, split_k=False)
        refused("multiple of 4", ops.conv3x3_wino_nhwc, (1, 8, 16, 64), (1, 8, 16, 132), u, b, 132, split_k=False)
        refused("multiple of 4", ops.conv_transpose2d_wino_nhwc, (1, 8, 16, 64), (1, 16, 32, 6), u, b, 6)
        refused("multiple of 4", ops.conv_transpose2d_wino_nhwc, (1, 8, 16, 64), (1, 16, 32, 132), u, b, 132)
        refused("even H and W", ops.conv3x3_wino_nhwc, (1, 9, 16, 64), (1, 4, 8, 4 * 32), u, b, 32, s2d_out=True,
                split_k=False)
    # split kernels only
    refused("multiple of 32, >= 64", ops.conv3x3_wino_nhwc, (1, 8, 16, 48), (1, 8, 16, 32), dummy_u, b, 32)
    refused("multiple of 32, >= 64", ops.conv_transpose2d_wino_nhwc, (1, 8, 16, 48), (1, 16, 32, 32), dummy_u, b, 32)
    refused("64-tile kernel only", ops.conv3x3_wino_nhwc, (1, 8, 16, 64), (1, 2, 8, 16, 16), dummy_u, b, 32,
            cm_out=True, split_k=False)
    refused("does not fit a pixel stride", ops.conv3x3_wino_nhwc, (1, 8, 16, 64), (1, 8, 16, 48), dummy_u, b, 36,
            out_coff=16, split_k=False)
    refused("does not fit a pixel stride", ops.conv3x3_wino_nhwc, (1, 8, 16, 512), (1, 8, 16, 48), dummy_u, b, 36,
            out_coff=16)                                              # the same through split-K
    # even H with a space-to-depth store through split-K
    refused("even H and W", ops.conv3x3_wino_nhwc, (1, 7, 16, 512), (1, 3, 8, 4 * 32), dummy_u, b, 32, s2d_out=True)
    # the first layer, from floats and from bytes: Cout % 4, Cout > 128, odd H with a space-to-depth store
    from dsic_amd import lib
    w, xf, xb = torch.zeros(132 * 3 * 9, device="cuda"), torch.zeros((1, 3, 9, 16), device="cuda"), \
        torch.zeros((1, 9, 16, 3), dtype=torch.uint8, device="cuda")
    for fn, x in ((L.dsic_conv_first_nchw, xf), (L.dsic_conv_first_u8hwc, xb)):
        for match, H, Cout, flag in (("multiple of 4", 8, 6, 0), ("multiple of 4", 8, 132, 0),
                                     ("even H and W", 9, 32, 1)):
            out = _out((1, 9, 16, 132), 16, 132)
            rc = fn(ops._p(x), ops._p(w), ops._p(b), None, None, ops._p(out.t), 1, 3, H, 16, Cout, 0, flag,
                    ops._stream())
            assert rc == lib.DSIC_EINVAL
            with pytest.raises(ValueError, match=match):
                lib.check(rc, "conv_first")
            torch.cuda.synchronize()
            assert out.untouched(), match


# ---------------------------------------------------------------------------------------------------- streamed stores

def test_streamed_output_of_the_32_tile_kernel_equals_the_cached_one(ops):
    """Outputs above 300 MiB leave the 32-tile split-bf16 kernel through its streaming-store instance (NT_OUT), which
    only a layer the 64-tile kernel does not take can reach: 280 is no multiple of 16, and 8 x 280 x 280 x 128 floats
    are 321 MB.  The same images four at a time are 160 MB per call and take the cached-store instance; a patch's
    bits do not depend on its batch, so all 8 images agree bit for bit."""
    B, H, W, Cin, Cout = 8, 280, 280, 64, 128
    g = torch.Generator(device="cuda").manual_seed(280)
    x = torch.randn((B, H, W, Cin), device="cuda", generator=g)
    w = torch.randn((Cout, Cin, 3, 3), device="cuda", generator=g) / 24
    bias = torch.randn(Cout, device="cuda", generator=g)
    u = ops.split_wino_weight_bf16(ops.pack_wino_weight(w), Cout, Cin)
    whole = ops.conv3x3_wino_nhwc(x, u, bias, Cout, split_k=False)
    assert 4 * whole.numel() > 300 << 20 > 2 * whole.numel() and tuple(whole.shape) == (B, H, W, Cout)
    halves = [ops.conv3x3_wino_nhwc(x[i:i + 4], u, bias, Cout, split_k=False) for i in (0, 4)]
    torch.cuda.synchronize()
    _seen.add("conv_wino_bf16_kernel<0> split-bf16 streamed stores")
    assert not bool(ops._ticket(x.device).any())
    assert bool(torch.isfinite(whole).all()) and float(whole.abs().max()) > 1.0
    for b in range(B):
        assert torch.equal(whole[b].view(torch.int32), halves[b // 4][b % 4].view(torch.int32)), \
            f"image {b}: the streamed and the cached stores give other bits"


# ---------------------------------------------------------------------------------------------------- the report

def test_worst_ratios_reported():
    """Prints, per (family, contraction, kind), the largest device error in units of E beside the CPU emulation's peak
    R (run the module whole, in file order, in one process); a device error above K_GPU * R has failed its case
    above."""
    for key in sorted(_worst):
        r = _worst[key]
        print(f"{key}: device worst 2^{math.log2(max(r, 1e-300)):.2f} of E, measured emulation peak R "
              f"2^{R.R_LOG2[key]:.2f}, device / R {r / R.R(*key):.2f}")
    for name in sorted(_seen):
        print("ran", name)
    assert _worst, "run the whole module"
