"""Index views on the GPU.  The index render, warped index render and index histogram kernels alone, bit for bit against
the NumPy restatement of tests/index_ref.py (composed with view_ref, valid_ref and warp_ref), outputs between guards and
inputs inside a larger allocation as in test_gpu_render.py; then codec.ImageReader.render_index / render_index_warped /
render_many / index_histogram / index_stretch on the 150 x 200 scenes of test_gpu_render.py: an index view is the
restated index, stretch and colour map of what read or read_warped returns for the same request, for every kind of
stream; and the command-line tool."""
import ctypes
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import index_ref as X
import index_stream_cases  # noqa: F401  (its recipes join the table that test_gpu_stream_order.py runs)
import render_ref as R
import view_ref as V
import warp_ref as W
from dsic_amd import codec, lib
from dsic_amd.ops import _p, _stream
from test_gpu_render import (_CACHE, BATCH, H0, REQUESTS, STREAMS, U16_PAIRS, W0, _contents, _model, _np, _pairs, _read,
                             _reader, _stream_of)
from test_gpu_valid import U8_FILL, Out, _inside, _same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOP = {"u8": 255, "u16": 65535}
MODES = {"average": 0, "nearest": 1}
KINDS = [("u8", 3), ("u8", 4), ("u16", 1), ("u16", 2), ("u16", 4)]
_CMAPS = {}


def _cmap(seed=0):
    """a random colour map on the host and the device: a wrong entry cannot pass"""
    if seed not in _CMAPS:
        host = np.random.default_rng(1000 + seed).integers(0, 256, size=(256, 3)).astype(np.uint8)
        _CMAPS[seed] = (host, torch.from_numpy(host).cuda())
    return _CMAPS[seed]


def _pair(name, top, which):
    """lo == hi, the whole range, a narrow pair with values on both sides: in index units"""
    vmin, vmax = X.value_range(name, top)
    if name == "nd":
        return [(2000, 2000), (vmin, vmax), (-1500, 2500)][which]
    if name == "difference":
        return [(-(top // 5), -(top // 5)), (vmin, vmax), (-(top // 8), top // 6)][which]
    return [(top // 3, top // 3), (vmin, vmax), (3 * (top // 8), 5 * (top // 8))][which]


def _blocks(img):
    """a block of 0 in all bands, so that A + B = 0 lies under whole outputs and under parts of outputs, and a block of
    the largest value in all bands: the bottom-left and bottom-right thirds (kernel_image has its nodata block top left)"""
    h, w = img.shape[:2]
    if h >= 3 and w >= 3:
        img[-(h // 3):, :w // 3] = 0
        img[-(h // 3):, -(w // 3):] = TOP["u8" if img.dtype == np.uint8 else "u16"]
    elif h * w > 1:
        img[-1, 0] = 0
    return img


def _args(index):
    """(kind, a, b) as the exports take them; a kind given as a number goes through as it is"""
    if isinstance(index[0], int):
        return index
    name, a, b = X.parse(index)
    return X.KINDS[name], a, b


# ---- the index render kernels ---------------------------------------------------------------------------------------
def _render(kind, src, sval, c, C, index, pair, cmap, dst, mode, nodata, alpha, background):
    y0, x0, h, w = c["region"]
    oh, ow = c["size"]
    return getattr(lib.load(), "dsic_window_index_render_" + kind)(
        _p(src), None if sval is None else _p(sval), c["sh"], c["sw"], c["sy0"], c["sx0"], C, c["shift"], y0, x0, h, w,
        *_args(index), pair[0], pair[1], None if cmap is None else _p(cmap), _p(dst), oh, ow, mode,
        -1 if nodata is None else nodata, alpha, background, _stream())


def _sweep(si, ki, kind, C, shift):
    """The thinned product: per (size, shift, kind) one (mode, mask) whose resample is restated once, and under it
    every index kind with its bands, alpha, background, stretch pair and the output's alignment taking turns; bands
    a == b once per kind."""
    turn = si * len(V.SHIFTS) + shift + ki
    masks = ["none", "valid", "nodata"] if kind == "u8" else ["none", "valid"]
    mode, mask = ("average", "nearest")[turn % 2], masks[(turn // 2) % len(masks)]
    shows = []
    for n, name in enumerate(["band"] if C == 1 else ["nd", "difference", "band"]):
        t = turn + n
        a = t % C
        b = a if C == 1 or (si, shift) == (3, 1) else (a + 1 + (t // 2) % (C - 1)) % C
        index = ("band", a) if name == "band" else (name, a, b)
        shows.append((index, (turn // 3 + n) % 2, (0, 200)[(turn // 5 + n) % 2], (turn // 2 + 2 * n) % 3, t))
    return mode, mask, shows


def test_the_sweep_takes_every_value_of_every_axis():
    for ki, (kind, C) in enumerate(KINDS):
        seen = set()
        for si in range(len(V.SIZES)):
            for shift in V.SHIFTS:
                mode, mask, shows = _sweep(si, ki, kind, C, shift)
                seen |= {mode, mask, (mode, mask)}
                for index, alpha, background, which, turn in shows:
                    seen |= {("alpha", alpha), ("bg", background), ("pair", index[0], which), ("index", index[0]),
                             ("offset", alpha, min(turn % 4, 1))}
                    if index[0] != "band":
                        seen.add(("a == b", index[1] == index[2]))
                    assert all(0 <= v < C for v in index[1:])
        masks = ["none", "valid"] + (["nodata"] if kind == "u8" else [])
        names = ["band"] if C == 1 else ["nd", "difference", "band"]
        assert {(m, k) for m in ("average", "nearest") for k in masks} <= seen, (kind, C)
        assert {("alpha", 0), ("alpha", 1), ("bg", 0), ("bg", 200)} <= seen, (kind, C)
        assert {("offset", 1, 0), ("offset", 1, 1), ("offset", 0, 0), ("offset", 0, 1)} <= seen, (kind, C)   # dwords and bytes
        assert {("index", n) for n in names} | {("pair", n, w) for n in names for w in range(3)} <= seen, (kind, C)
        assert C == 1 or {("a == b", True), ("a == b", False)} <= seen, (kind, C)


@pytest.mark.parametrize("si", range(len(V.SIZES)))
@pytest.mark.parametrize("ki", range(len(KINDS)))
def test_index_render_kernels_equal_the_restatement(si, ki):
    (src_size, out_size), (kind, C) = V.SIZES[si], KINDS[ki]
    cmap, d_cmap = _cmap(si + ki)
    for shift in V.SHIFTS:
        if src_size[1] > 1000 and shift != ki % len(V.SHIFTS):              # the long rows: one shift per kind
            continue
        c = V.kernel_case(src_size, out_size, shift)
        mode, mask, shows = _sweep(si, ki, kind, C, shift)
        img = _blocks(V.kernel_image(kind, C, c["sh"], c["sw"]))
        rng = np.random.default_rng(c["sh"] * 13 + c["sw"] + C)
        valid = None
        if mask == "valid":
            valid = rng.random((c["sh"], c["sw"])) < 0.7
            valid[:max(1, c["sh"] // 2), :max(1, c["sw"] // 2)] = False     # a quadrant wholly invalid
            valid = valid.astype(np.uint8) * rng.integers(1, 256, size=valid.shape).astype(np.uint8)
        nodata = V.NODATA[kind] if mask == "nodata" else None
        elem = img.dtype.itemsize
        d_src, d_val = _inside(img, elem * (1 + shift)), None if valid is None else _inside(valid, 3)
        geo = (c["sy0"], c["sx0"], shift, c["region"], c["size"])
        if valid is None:
            res, ok = V.resample(img, *geo, mode, nodata if mode == "average" else None), None
        else:
            res, ok = R.valid_ref.resample(img, valid, *geo, mode, 0)
        for index, alpha, background, which, turn in shows:
            pair = _pair(index[0], TOP[kind], which)
            what = (f"window_index_render_{kind} {src_size}->{out_size} C={C} shift={shift} {mode} {mask} index={index} "
                    f"pair={pair} alpha={alpha} background={background}")
            want = X.display_index(res, ok, index, pair, cmap, alpha, background)
            for offset in {0, turn % 4}:                                     # 4 bytes per pixel: the dword stores and not
                out = Out(want.size, offset=offset)
                lib.check(_render(kind, d_src, d_val, c, C, index, pair, d_cmap, out.view, MODES[mode], nodata, alpha,
                                  background), what)
                _same(out.host(what), want, what)
            assert want.shape == out_size + (3 + alpha,)


def test_zero_sums_lie_under_whole_outputs_and_under_parts_of_outputs():
    """the sweep's zero block does what it is there for, and the top block reaches the ends of every kind"""
    c = V.kernel_case((17, 33), (5, 7), 0)
    img = _blocks(V.kernel_image("u16", 2, c["sh"], c["sw"]))
    res = V.resample(img, c["sy0"], c["sx0"], 0, c["region"], c["size"])
    s = res.astype(np.int64).sum(axis=2)
    whole = V.resample((img.astype(np.int64).sum(axis=2, keepdims=True) > 0).astype(np.uint16) * 65535, c["sy0"], c["sx0"], 0,
                       c["region"], c["size"])[:, :, 0]
    assert (s == 0).any() and ((whole > 0) & (whole < 65535)).any() and (res == 65535).all(axis=2).any()
    cmap, d_cmap = _cmap(99)
    want = X.display_index(res, None, ("nd", 0, 1), (-10000, 10000), cmap, True, 9)
    assert (want[s == 0] == [9, 9, 9, 0]).all() and (want[..., 3] == 255).any()
    out = Out(want.size)
    lib.check(_render("u16", _inside(img, 2), None, c, 2, ("nd", 0, 1), (-10000, 10000), d_cmap, out.view, 0, None, 1, 9), "nd")
    _same(out.host("nd"), want, "nd over the zero block")


@pytest.mark.parametrize("name", list(codec.COLORMAPS))
def test_each_named_map_through_the_kernel(name):
    c = V.kernel_case((33, 35), (16, 17), 1)
    img = _blocks(V.kernel_image("u16", 4, c["sh"], c["sw"]))
    cmap = codec.COLORMAPS[name]
    res = V.resample(img, c["sy0"], c["sx0"], 1, c["region"], c["size"])
    want = X.display_index(res, None, ("nd", 3, 0), (-10000, 10000), cmap, False, 0)
    out = Out(want.size, offset=1)
    lib.check(_render("u16", _inside(img, 2), None, c, 4, ("nd", 3, 0), (-10000, 10000), torch.from_numpy(cmap).cuda(),
                      out.view, 0, None, 0, 0), name)
    _same(out.host(name), want, name)
    assert len(np.unique(want.reshape(-1, 3), axis=0)) > 8                   # the view shows the map, not one colour


# ---- the warped index render kernels --------------------------------------------------------------------------------
# every source size and every output size of warp_ref at least once, the four matrices, the three masks
WARPS = [((17, 33), (16, 16), 0, "rot30", "valid"), ((40, 68), (70, 130), 1, "minify2.5", "none"),
         ((5, 7), (17, 33), 2, "magnify3", "nodata"), ((40, 68), (7, 9), 0, "rot30", "valid"),
         ((2, 2), (1, 1), 0, "identity", "none"), ((1, 1), (7, 9), 1, "magnify3", "valid"),
         ((17, 33), (17, 33), 1, "identity", "nodata"), ((5, 7), (16, 16), 0, "minify2.5", "none")]


def _warp_render(kind, src, sval, c, C, index, pair, cmap, dst, mode, nodata, alpha, background):
    return getattr(lib.load(), "dsic_window_warp_index_render_" + kind)(
        _p(src), None if sval is None else _p(sval), c["sh"], c["sw"], c["sy0"], c["sx0"], C, c["shift"], c["LH"], c["LW"],
        c["H"], c["W"], (ctypes.c_int64 * 6)(*c["m"]), *_args(index), pair[0], pair[1], None if cmap is None else _p(cmap),
        _p(dst), *c["size"], mode, -1 if nodata is None else nodata, alpha, background, _stream())


def _cut(a, c):
    return np.ascontiguousarray(a[c["sy0"]:c["sy0"] + c["sh"], c["sx0"]:c["sx0"] + c["sw"]])


def test_the_warp_cases_take_every_size_matrix_and_mask():
    assert {w[0] for w in WARPS} == set(W.SRC_SIZES) and {w[1] for w in WARPS} == set(W.OUT_SIZES)
    assert {w[2] for w in WARPS} == set(W.SHIFTS) and {w[3] for w in WARPS} == {"identity", "rot30", "magnify3", "minify2.5"}
    assert {w[4] for w in WARPS} == {"none", "valid", "nodata"}


@pytest.mark.parametrize("kind,C", KINDS)
def test_warp_index_render_kernels_equal_the_restated_display(kind, C):
    top = TOP[kind]
    inside_some = undefined_some = 0
    for n, (src_size, out_size, l, name, mask) in enumerate(WARPS):
        img = _blocks(W.level_image(kind, C, *src_size))
        val = W.validity(*src_size, seed=n) if mask == "valid" else None
        nodata = W.NODATA[kind] if mask == "nodata" else None
        cmap, d_cmap = _cmap(n)
        for mode in (0, 1, 2):
            c = W.kernel_case(src_size, out_size, l, name, mode, n % 2)
            res, ok = W.run_case(img, val, c, mode, nodata, 0)
            src = _inside(_cut(img, c), (1 + mode) * img.dtype.itemsize)
            sval = None if val is None else _inside(_cut(val, c), 3)
            names = ["band"] if C == 1 else ["nd", "difference", "band"]
            for k, iname in enumerate(names):
                t = n + mode + k
                a = t % C
                b = a if C == 1 or (n, mode) == (0, 0) else (a + 1 + t % (C - 1)) % C
                index = ("band", a) if iname == "band" else (iname, a, b)
                pair = _pair(iname, top, (n + k + mode) % 3)
                alpha, background = (t // 2) % 2, (200, 0)[t % 2]
                want = X.display_index(res, ok, index, pair, cmap, alpha, background)
                for offset in {0, 1 + mode}:
                    out = Out(want.size, offset=offset)
                    what = (f"window_warp_index_render_{kind} {src_size}->{out_size} C={C} shift={l} {name} mode={mode} "
                            f"{mask} index={index} pair={pair} alpha={alpha} background={background} offset={offset}")
                    lib.check(_warp_render(kind, src, sval, c, C, index, pair, d_cmap, out.view, mode, nodata, alpha,
                                           background), what)
                    _same(out.host(what), want, what)
                if iname == "nd":
                    undefined_some += int((ok & (res[..., a].astype(np.int64) + res[..., b] == 0)).any())
            inside_some += int(ok.any())
    assert inside_some >= 2 * len(WARPS)                                     # not a sweep of empty views,
    assert C == 1 or undefined_some > 0                                      # and the zero block is met


# ---- the index histogram kernels ------------------------------------------------------------------------------------
def _histogram(kind, img, valid, nodata, index, hist):
    H, W_, C = img.shape
    fn = getattr(lib.load(), "dsic_index_histogram_" + kind)
    d_img, d_valid = _inside(img, 2 if kind == "u16" else 1), None if valid is None else _inside(valid, 3)
    status = fn(_p(d_img), None if d_valid is None else _p(d_valid), H, W_, C, -1 if nodata is None else nodata,
                *_args(index), _p(hist), _stream())
    torch.cuda.synchronize()                                                 # the inputs live until the kernel has read them
    return status


@pytest.mark.parametrize("H,W_", [(1, 1), (3, 5), (70, 1030), (257, 263)])
@pytest.mark.parametrize("kind,C", [("u16", 2), ("u16", 4), ("u8", 3), ("u8", 4)])
def test_index_histogram_kernels_equal_the_restatement(H, W_, kind, C):
    rng = np.random.default_rng(H * 1009 + W_ * 7 + C)
    speckle = (rng.random((H, W_)) < 0.7).astype(np.uint8) * rng.integers(1, 256, size=(H, W_)).astype(np.uint8)
    masks = [("none", None), ("speckle", speckle), ("all invalid", np.zeros((H, W_), dtype=np.uint8))]
    for w, what in enumerate(("random", "constant", "smooth")):
        img = _contents(kind, H, W_, C, what, rng)
        if H * W_ > 1:
            img[:max(1, H // 4), -max(1, W_ // 4):] = 0                      # A + B = 0: not counted by nd
        cases = [(name, valid, None) for name, valid in masks]
        if kind == "u8":
            nd = int(img[H // 2, W_ // 2, 0])
            img[H // 2:, W_ // 2:] = nd                                      # a block of nodata pixels, and
            img[0, 0, C - 1] = nd ^ 1                                        # a pixel that a single channel keeps in
            cases.append(("nodata", None, nd))
        # 20001 bins (both widths), 511 (uint8 difference, counted in LDS), 131071 (uint16 difference)
        for index in (("nd", C - 1, 0), ("difference", w % C, (w + 1) % C), ("nd", 1, 1)):
            bins = 20001 if index[0] == "nd" else 2 * TOP[kind] + 1
            for name, valid, nodata in cases:
                label = f"index_histogram_{kind} {H}x{W_}x{C} {what} {name} {index}"
                hist = Out(4 * bins, fill=0)
                want = X.histogram(img, valid, nodata, index)
                assert want.shape == (bins,)
                lib.check(_histogram(kind, img, valid, nodata, index, hist.view), label)
                got = hist.host(label).view(np.uint32)
                assert np.array_equal(got, want), label
                assert name != "all invalid" or not got.any()
                if name == "speckle":                                        # a second call adds to the first
                    lib.check(_histogram(kind, img, None, nodata, index, hist.view), label)
                    got = hist.host(label).view(np.uint32)
                    assert np.array_equal(got, want + X.histogram(img, None, nodata, index)), label + " twice"
                if name == "none" and index[0] == "nd" and H * W_ > 1:
                    assert got.sum() < H * W_                                # the zero block stayed out


# ---- refusals -------------------------------------------------------------------------------------------------------
def test_the_calls_refuse_through_their_error_return_and_write_nothing():
    src = torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda")
    out, hist = Out(4 * 4 * 4 + 768), Out(4 * 20001)
    dst, over = out.view[:64], out.view[32:32 + 768]                         # a colour map that overlaps the output
    cmap = _cmap(0)[1]
    view = {"sh": 8, "sw": 8, "sy0": 0, "sx0": 0, "shift": 0, "region": (0, 0, 8, 8), "size": (4, 4)}
    warp = {"sh": 8, "sw": 8, "sy0": 0, "sx0": 0, "shift": 0, "LH": 8, "LW": 8, "H": 8, "W": 8,
            "m": (2 * 65536, 0, 0, 0, 2 * 65536, 0), "size": (4, 4)}
    args = dict(C=3, index=("nd", 0, 1), pair=(-10000, 10000), cmap=cmap, mode=0, nodata=None, alpha=1, background=0)
    err = lib.load().dsic_last_error
    for call, c in ((_render, view), (_warp_render, warp)):
        for change, word in (({"index": ("nd", 0, 3)}, "band 3"), ({"index": ("difference", -1, 0)}, "band -1"),
                             ({"pair": (-10001, 0)}, "(-10001, 0)"), ({"pair": (0, 10001)}, "(0, 10001)"),
                             ({"pair": (9, 8)}, "(9, 8)"), ({"index": ("difference", 0, 1), "pair": (-256, 0)}, "(-256, 0)"),
                             ({"index": ("band", 0), "pair": (0, 256)}, "(0, 256)"), ({"cmap": None}, "null"),
                             ({"cmap": over}, "cmap and dst overlap"), ({"alpha": 2}, "alpha=2"),
                             ({"background": 256}, "background"), ({"background": -1}, "background"), ({"C": 5}, "C=5"),
                             ({"mode": 3}, "mode=3"), ({"nodata": 256}, "nodata=256")):
            p = dict(args, **change)
            assert call("u8", src, None, c, p["C"], p["index"], p["pair"], p["cmap"], dst, p["mode"], p["nodata"], p["alpha"],
                        p["background"]) == lib.DSIC_EINVAL, (call.__name__, change)
            assert word.encode() in err(), (word, err())
        for kind in (-1, 3):                                                 # a kind outside the three
            assert call("u8", src, None, c, 3, (kind, 0, 1), (0, 0), cmap, dst, 0, None, 1, 0) == lib.DSIC_EINVAL
            assert f"kind={kind}".encode() in err()
        assert call("u8", src, out.view[:64], c, 3, ("nd", 0, 1), (0, 0), cmap, dst, 0, None, 1, 0) == lib.DSIC_EINVAL
        assert b"overlap" in err()                                           # dst over the validity window
    assert _render("u8", src, None, dict(view, region=(0, 0, 9, 8)), 3, ("nd", 0, 1), (0, 0), cmap, dst, 0, None, 1,
                   0) == lib.DSIC_EINVAL and b"outside the source window" in err()
    assert _warp_render("u8", src, None, dict(warp, sh=7), 3, ("nd", 0, 1), (0, 0), cmap, dst, 0, None, 1,
                        0) == lib.DSIC_EINVAL and b"outside the source window" in err()
    L = lib.load()
    for a in ((4, 4, 5, -1, 2, 0, 1), (0, 4, 3, -1, 2, 0, 1), (4, 4, 3, 256, 2, 0, 1), (4, 4, 3, -1, 0, 0, 1), (4, 4, 3, -1, 3, 0, 1),
              (4, 4, 3, -1, 2, 3, 1), (4, 4, 3, -1, 1, 0, -1)):
        assert L.dsic_index_histogram_u8(_p(src), None, *a, _p(hist.view), _stream()) == lib.DSIC_EINVAL, a
    assert L.dsic_index_histogram_u8(_p(src), None, 4, 4, 3, -1, 2, 0, 1, _p(hist.view[1:]), _stream()) == lib.DSIC_EINVAL
    assert L.dsic_index_histogram_u8(_p(src), None, 4, 4, 3, -1, 2, 0, 1, None, _stream()) == lib.DSIC_EINVAL
    torch.cuda.synchronize()
    assert (out.host("refused calls") == U8_FILL).all() and (hist.host("refused calls") == U8_FILL).all()
    assert not bool(src.any())


# ---- the reader -----------------------------------------------------------------------------------------------------
def _index_of(C, k):
    return [("nd", C - 1, 0), ("difference", 0, C - 1), ("band", 1), ("nd", 1, 2)][k % 4]


def _colormap(k):
    """a named map, the random map as a tensor on the device, the random map as a NumPy array -> (argument, host table)"""
    names = list(codec.COLORMAPS)
    if k % 3 == 0:
        return names[(k // 3) % 4], codec.COLORMAPS[names[(k // 3) % 4]]
    host, dev = _cmap(7)
    return (dev, host) if k % 3 == 1 else (host, host)


@pytest.mark.parametrize("name", list(STREAMS))
def test_an_index_view_is_the_restated_index_of_the_read(name):
    kind, C, kw = STREAMS[name]
    top = 65535 if kind == "u16" else 255
    masked, pyramid = "valid" in kw, "overviews" in kw
    with _reader(name) as r, _reader(name) as plain:
        for k, (win, size, level) in enumerate(REQUESTS):
            for resampling in ("average", "nearest") if size is not None else ("average",):
                st = {}
                index = _index_of(C, k)
                pair = _pair(index[0], top, (k + 1) % 3) if index[0] != "difference" or top == 255 else (-3000, 2000)
                arg, table = _colormap(k)
                alpha, background = bool(k % 2) and "nodata" not in kw, (0, 200)[(k // 2) % 2]
                got = r.render_index(*win, index, size=size, level=level, stretch=pair, colormap=arg, alpha=alpha,
                                     background=background, resampling=resampling, stats=st)
                img, valid = _read(plain, name, win, size, level, resampling)
                want = X.display_index(img, valid, index, pair, table, alpha, background)
                assert got.is_cuda and got.dtype == torch.uint8 and got.is_contiguous()
                assert got.shape == want.shape and np.array_equal(_np(got), want), (name, win, size, resampling, index)
                if size == (37, 50):
                    assert st["level"] == (2 if pyramid else 0)
                if masked and size is not None and win[0] == 0:
                    assert not valid.all() and valid.any() and (_np(got)[~valid][:, :3] == background).all()
        if pyramid:                                                          # a level's own window, as it is
            got = r.render_index(3, 5, 60, 80, ("nd", 0, 2), level=1, colormap="ndvi", alpha=masked, background=50)
            img, valid = _read(plain, name, (3, 5, 60, 80), None, 1, "average")
            assert np.array_equal(_np(got), X.display_index(img, valid, ("nd", 0, 2), (-10000, 10000), codec.COLORMAPS["ndvi"],
                                                            masked, 50))
        # the tie to the old tail: a band through "grey" with the band's pair is render's grey, three times
        pairs = U16_PAIRS if kind == "u16" else _pairs("u8", C, 1)
        a = 1 if kind == "u16" else 2                                        # a pair with lo < hi
        for size in ((45, 52), None):
            tied = r.render_index(40, 40, 60, 70, ("band", a), size=size, stretch=pairs[a], colormap="grey", alpha=masked,
                                  background=77)
            assert torch.equal(tied, r.render(40, 40, 60, 70, size=size, bands=(a, a, a), stretch=pairs, alpha=masked,
                                              background=77))


def _views():
    """(matrix, size, level, resampling): turned, minified onto an overview, overhanging, beside nothing"""
    return [(codec.rotation_affine(75, 100, 30, 1.25, 64, 80), (64, 80), None, "bilinear"),
            (codec.window_affine(3, 5, 140, 190, 35, 47), (35, 47), None, "cubic"),
            (codec.rotation_affine(140, 190, -20, 0.4, 50, 70), (50, 70), None, "cubic"),
            ([[-1, 0, 120], [0, 1, 100.5]], (64, 64), 0, "nearest")]


@pytest.mark.parametrize("name", list(STREAMS))
def test_a_warped_index_view_is_the_restated_index_of_the_warped_read(name):
    kind, C, kw = STREAMS[name]
    top = 65535 if kind == "u16" else 255
    out = "u8" if kind == "f32" else None
    with _reader(name) as r, _reader(name) as plain:
        for k, (matrix, size, level, resampling) in enumerate(_views()):
            index = _index_of(C, k + 1)
            pair = _pair(index[0], top, k % 3) if index[0] != "difference" or top == 255 else (-3000, 2000)
            arg, table = _colormap(k + 1)
            alpha, background = bool(k % 2) and "nodata" not in kw, (0, 200)[(k // 2) % 2]
            st = {}
            got = r.render_index_warped(matrix, size, index, level=level, stretch=pair, colormap=arg, alpha=alpha,
                                        background=background, resampling=resampling, stats=st)
            img, valid = plain.read_warped(matrix, size, level=level, resampling=resampling, out=out, with_valid=True)
            want = X.display_index(_np(img), _np(valid), index, pair, table, alpha, background)
            assert got.dtype == torch.uint8 and got.is_contiguous() and np.array_equal(_np(got), want), (name, k)
            assert st["matrix_q16"] == codec.affine_q16(matrix)
        before, st = r.stats, {}                                             # beside the image: nothing decoded or launched
        shown = r.render_index_warped([[1, 0, 0], [0, 1, -900]], (20, 30), ("nd", 0, 1), alpha="nodata" not in kw,
                                      background=31, stats=st)
        assert st["tiles"] == [] and st["level_window"] is None and r.stats["decoded"] == before["decoded"]
        assert np.array_equal(_np(shown)[..., :3], np.full((20, 30, 3), 31))
        assert "nodata" in kw or not bool(shown[..., 3].any())


def test_render_many_mixes_plain_and_index_requests_and_shares_the_decode_batches():
    for name in ("u8_valid", "u16"):
        C = STREAMS[name][1]
        top = 65535 if name == "u16" else 255
        pairs = U16_PAIRS if name == "u16" else _pairs("u8", C, 2)
        reqs = []
        for k, (win, size, level) in enumerate(REQUESTS):
            q = {"window": win, "size": size, "level": level}
            if k % 2:
                q.update(stretch=pairs, bands=[(0, 1, 2), (C - 1, 0, 0)][k // 2 % 2])
            else:
                index = _index_of(C, k // 2)
                q.update(index=index, colormap=_colormap(k // 2)[0])
                if k:
                    q.update(stretch=_pair(index[0], top, 1))
            reqs.append(q)
        reqs.append({"window": (5, 7, 40, 50), "index": ("band", 0), "stretch": (0, top)})

        def single(reader, q):
            common = dict(size=q.get("size"), level=q.get("level"), stretch=q.get("stretch"), alpha=True, background=31)
            if "index" in q:
                return reader.render_index(*q["window"], q["index"], colormap=q.get("colormap", "grey"), **common)
            return reader.render(*q["window"], bands=q.get("bands"), **common)

        with _reader(name) as one:
            want = [single(one, q) for q in reqs]
        assert all(w.shape[2] == (4 if "index" in q or len(q["bands"]) == 3 else 2) for w, q in zip(want, reqs))
        with _reader(name) as r, _reader(name) as reads:
            st, st_reads = {}, {}
            got = r.render_many(reqs, alpha=True, background=31, stats=st)
            reads.read_many([{k: v for k, v in q.items() if k in ("window", "size", "level")} for q in reqs], stats=st_reads)
            assert len(got) == len(want) and all(torch.equal(g, w) for g, w in zip(got, want))
            assert st["decode_batches"] <= st_reads["decode_batches"] and st["decoded"] == st_reads["decoded"] > 0
            assert sorted(st["tiles"]) == sorted(st_reads["tiles"]) and len(set(st["tiles"])) == len(st["tiles"])
            again = {}
            assert all(torch.equal(g, w) for g, w in zip(r.render_many(reqs, alpha=True, background=31, stats=again), want))
            assert (again["decoded"], again["decode_batches"]) == (0, 0)
        with _reader(name, cache_bytes=3 * 4 * C * 64 * 64) as r:            # the union does not fit: one by one
            assert all(torch.equal(g, w) for g, w in zip(r.render_many(reqs, alpha=True, background=31), want))


@pytest.mark.parametrize("name", list(STREAMS))
def test_the_index_histogram_counts_the_levels_pixels_once_and_the_stretches_follow(name):
    kind, C, kw = STREAMS[name]
    top = 65535 if kind == "u16" else 255
    with _reader(name) as r, _reader(name) as plain:
        n = len(r.levels)
        for level in [None] + list(range(n))[:2]:
            h, w = r.levels[n - 1 if level is None else level]
            img, valid = _read(plain, name, (0, 0, h, w), None, n - 1 if level is None else level, "average")
            for index in (("nd", C - 1, 0), ("difference", 0, 1)):
                vmin, vmax = X.value_range(index[0], top)
                got = r.index_histogram(index, level)
                want = X.histogram(img, None if "nodata" in kw else valid, kw.get("nodata"), index)
                assert got.dtype == np.int64 and got.shape == (vmax - vmin + 1,) and np.array_equal(got, want), (name, level)
                assert 0 < got.sum() <= h * w
                before = r.stats
                assert np.array_equal(r.index_histogram(index, level), got)
                assert r.stats["decoded"] == before["decoded"] and r.stats["bytes_read"] == before["bytes_read"]
                for percent in ((2, 98), (0, 100)):
                    assert r.index_stretch(index, percent, level) == X.index_stretch(want, index, top, percent)
            assert np.array_equal(r.index_histogram(("band", 1), level), r.histogram(level)[1])
            assert r.index_stretch(("band", 1), (2, 98), level) == r.stretch((2, 98), level)[1]
        # the default stretches
        win, size = (40, 40, 60, 70), (45, 52)
        assert torch.equal(r.render_index(*win, ("nd", 0, 1), size=size),
                           r.render_index(*win, ("nd", 0, 1), size=size, stretch=(-10000, 10000)))
        band = r.stretch()[2] if kind == "u16" else (0, 255)                # what render uses for the band
        assert torch.equal(r.render_index(*win, ("band", 2), size=size), r.render_index(*win, ("band", 2), size=size, stretch=band))
        auto = r.index_stretch(("difference", 0, 1))
        assert auto == X.index_stretch(r.index_histogram(("difference", 0, 1)), ("difference", 0, 1), top) and auto[0] < auto[1]
        assert torch.equal(r.render_index(*win, ("difference", 0, 1), size=size, colormap="diverging"),
                           r.render_index(*win, ("difference", 0, 1), size=size, colormap="diverging", stretch=auto))
        eye = codec.window_affine(40, 40, 60, 70, 45, 52)
        assert torch.equal(r.render_index_warped(eye, size, ("difference", 0, 1)),
                           r.render_index_warped(eye, size, ("difference", 0, 1), stretch=auto))
    with _reader(name) as r:                                                 # the first use counts the coarsest level
        st = {}
        r.render_index(5, 7, 40, 50, ("difference", 0, 1), size=(40, 50), stats=st)
        assert {l for l, _ in st["tiles"]} == {0, len(r.levels) - 1}
        assert 0 < st["decoded"] == r.stats["decoded"] <= len(set(st["tiles"]))     # each missing tile once


def test_the_readers_refusals_come_before_anything_is_decoded():
    with _reader("u16") as r:
        for level in range(len(r.levels)):                                   # every level's heads are read; no tile is
            r.index(level)
        before = r.stats
        eye = [[1, 0, 0], [0, 1, 0]]
        for kw, word in (({"index": ("nd", 0)}, "index="), ({"index": ("nd", 0, 4)}, "index="), ({"index": ("ndvi", 0, 1)}, "index="),
                         ({"stretch": (-10001, 0)}, "stretch"), ({"stretch": (9, 8)}, "stretch"), ({"stretch": [(0, 1)] * 4}, "stretch"),
                         ({"colormap": "viridis"}, "colormap"), ({"colormap": np.zeros((256, 4), np.uint8)}, "colormap"),
                         ({"background": 256}, "background"), ({"background": -1}, "background"), ({"level": 3}, "levels 0 .. 2")):
            p = dict({"index": ("nd", 0, 1)}, **kw)
            with pytest.raises(ValueError, match=word):
                r.render_index(0, 0, 64, 64, p.pop("index"), size=(16, 16), **p)
            p = dict({"index": ("nd", 0, 1)}, **kw)
            with pytest.raises(ValueError, match=word):
                r.render_index_warped(eye, (16, 16), p.pop("index"), **p)
            if "level" not in kw and "background" not in kw:
                with pytest.raises(ValueError, match=word):
                    r.render_many([dict({"window": (0, 0, 64, 64), "index": ("nd", 0, 1)}, **kw), {"window": (0, 0, 64, 64)}])
        with pytest.raises(ValueError, match="resampling"):
            r.render_index(0, 0, 64, 64, ("nd", 0, 1), resampling="cubic")
        with pytest.raises(ValueError, match="window"):
            r.render_index(0, 0, H0 + 1, 8, ("nd", 0, 1), size=(4, 4))
        with pytest.raises(ValueError, match="index="):
            r.index_histogram(("nd", 0, 4))
        with pytest.raises(ValueError, match="levels 0 .. 2"):
            r.index_histogram(("nd", 0, 1), 3)
        with pytest.raises(ValueError, match="percent"):
            r.index_stretch(("nd", 0, 1), (98, 2))
        with pytest.raises(ValueError, match="index="):
            r.index_stretch(("band", 4))
        assert r.stats["decoded"] == 0 and r.stats["bytes_read"] == before["bytes_read"]
    with _reader("u8_nodata") as r:
        with pytest.raises(ValueError, match="valid="):
            r.render_index(0, 0, 64, 64, ("nd", 0, 1), size=(16, 16), alpha=True)
        with pytest.raises(ValueError, match="valid="):
            r.render_index_warped([[1, 0, 0], [0, 1, 0]], (16, 16), ("nd", 0, 1), alpha=True)
        assert r.stats["decoded"] == 0
    r = _reader("u8")
    r.close()
    with pytest.raises(ValueError, match="closed"):
        r.render_index(0, 0, 8, 8, ("nd", 0, 1))
    with pytest.raises(ValueError, match="closed"):
        r.index_histogram(("nd", 0, 1))


# ---- the tool -------------------------------------------------------------------------------------------------------
def test_the_tool_renders_index_views_into_npy_and_ppm(tmp_path):
    model, stream = _model(4), _stream_of("u16_valid")
    sd = _CACHE[("model", 4)][1]
    torch.save({"model": {k: torch.from_numpy(v) for k, v in sd.items()}}, tmp_path / "ckpt.pt")
    (tmp_path / "s.dsic").write_bytes(stream)
    tool = os.path.join(ROOT, "tools", "dsic_image.py")
    head = [sys.executable, tool, "render", str(tmp_path / "s.dsic")]
    tail = ["--weights", str(tmp_path / "ckpt.pt"), "--batch", str(BATCH)]
    # a window to .npy with the percentile pair and alpha; a turned view to .ppm with a pair of its own
    runs = [(["--region", "0,0,150,200", "--size", "37,50", "--index", "nd:3,0", "--colormap", "ndvi", "--percent", "1,99",
              "--alpha", "--background", "60"], "a.npy"),
            (["--rotate", "30", "--center", "75,100", "--scale", "1.5", "--size", "64,100", "--index", "nd:3,0", "--colormap",
              "ndvi", "--index-stretch=-2000,6000", "--resampling", "cubic"], "b.ppm")]
    outs = []
    for extra, dst in runs:
        p = subprocess.run(head + [str(tmp_path / dst)] + extra + tail, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stdout + p.stderr
        outs.append(p.stdout)
    with codec.ImageReader(model, io.BytesIO(stream), batch=BATCH) as r:
        auto = r.index_stretch(("nd", 3, 0), (1, 99))
        a = _np(r.render_index(0, 0, H0, W0, ("nd", 3, 0), size=(37, 50), stretch=auto, colormap="ndvi", alpha=True,
                               background=60))
        b = _np(r.render_index_warped(codec.rotation_affine(75, 100, 30, 1.5, 64, 100), (64, 100), ("nd", 3, 0),
                                      stretch=(-2000, 6000), colormap="ndvi", resampling="cubic"))
    assert -10000 <= auto[0] < auto[1] <= 10000
    assert np.array_equal(np.load(tmp_path / "a.npy"), a) and a.shape == (37, 50, 4) and (a[..., 3] == 0).any()
    assert (tmp_path / "b.ppm").read_bytes() == b"P6\n100 64\n255\n" + b.tobytes() and b.shape == (64, 100, 3)
    assert "index nd:3,0" in outs[0] and "colormap ndvi + alpha" in outs[0] and "level 2" in outs[0] and "37x50" in outs[0]
    assert f"stretch ({auto[0]}, {auto[1]})" in outs[0] and "stretch (-2000, 6000)" in outs[1] and "64x100" in outs[1]
