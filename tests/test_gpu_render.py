"""Rendered views on the GPU.  The histogram and render kernels alone, bit for bit against the NumPy restatement of
tests/render_ref.py, outputs between guards and inputs inside a larger allocation as in test_gpu_valid.py; then
codec.ImageReader.render / render_many / histogram / stretch on 150 x 200 scenes (tile 64, batch 4, the synthetic
N = 128 / M = 192 model): a render is the restated stretch of what read returns for the same request, for every kind of
stream; and the command-line tool."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import render_ref as R
import view_ref as V
from dsic_amd import codec, lib
from dsic_amd import synthetic as S
from dsic_amd.model import CompressionModel
from dsic_amd.ops import _p, _stream
from test_gpu_valid import U8_FILL, Out, _inside, _same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}
TOP = {"u8": 255, "u16": 65535}
MODES = {"average": 0, "nearest": 1}
KINDS = [k for k in V.KINDS if k[0] != "f32"] + [("u8", 1)]


def _c_int(values):
    import ctypes
    return (ctypes.c_int * len(values))(*values)


# ---- the histogram kernels ------------------------------------------------------------------------------------------
def _histogram(kind, img, valid, nodata, hist):
    """uint16 images at an address that is 2-byte but not 4-byte aligned, uint8 ones at an odd address"""
    H, W, C = img.shape
    fn = getattr(lib.load(), "dsic_band_histogram_" + kind)
    d_img, d_valid = _inside(img, 2 if kind == "u16" else 1), None if valid is None else _inside(valid, 3)
    status = fn(_p(d_img), None if d_valid is None else _p(d_valid), H, W, C, -1 if nodata is None else nodata, _p(hist),
                _stream())
    torch.cuda.synchronize()                                                 # the inputs live until the kernel has read them
    return status


def _contents(kind, H, W, C, what, rng):
    top, dtype = TOP[kind], V.DTYPES[kind]
    if what == "constant":
        return np.full((H, W, C), top // 3, dtype=dtype)
    if what == "smooth":                                                     # long runs along a row, few values
        img = (np.arange(W)[None, :, None] // 97 + np.arange(H)[:, None, None] // 50 + np.arange(C)[None, None, :])
        return (img * (top // 40)).astype(dtype)
    img = rng.integers(0, top + 1, size=(H, W, C)).astype(dtype)
    img.reshape(-1)[0], img.reshape(-1)[-1] = 0, top
    return img


@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (70, 1030), (257, 263)])
@pytest.mark.parametrize("kind,C", [("u16", 1), ("u16", 2), ("u16", 3), ("u16", 4), ("u8", 3), ("u8", 4)])
def test_histogram_kernels_equal_bincount(H, W, kind, C):
    rng = np.random.default_rng(H * 1009 + W * 7 + C)
    bins = TOP[kind] + 1
    speckle = (rng.random((H, W)) < 0.7).astype(np.uint8) * rng.integers(1, 256, size=(H, W)).astype(np.uint8)
    masks = [("none", None), ("speckle", speckle), ("all invalid", np.zeros((H, W), dtype=np.uint8))]
    for what in ("random", "constant", "smooth"):
        img = _contents(kind, H, W, C, what, rng)
        cases = [(name, valid, None) for name, valid in masks]
        if kind == "u8":
            nd = int(img[H // 2, W // 2, 0])
            img[H // 2:, W // 2:] = nd                                       # a block of nodata pixels, and
            img[0, 0, C - 1] = nd ^ 1                                        # a pixel that a single channel keeps in
            cases.append(("nodata", None, nd))
        for name, valid, nodata in cases:
            label = f"band_histogram_{kind} {H}x{W}x{C} {what} {name}"
            hist = Out(4 * C * bins, fill=0)
            want = R.histogram(img, valid, nodata)
            lib.check(_histogram(kind, img, valid, nodata, hist.view), label)
            got = hist.host(label).view(np.uint32).reshape(C, bins)
            assert np.array_equal(got, want), label
            assert name != "all invalid" or not got.any()
            if name == "speckle":                                            # a second call adds to the first
                lib.check(_histogram(kind, img, None, nodata, hist.view), label)
                got = hist.host(label).view(np.uint32).reshape(C, bins)
                assert np.array_equal(got, want + R.histogram(img, None, nodata)), label + " twice"


def test_histogram_calls_refuse_and_write_nothing():
    img = torch.zeros((4, 4, 3), dtype=torch.uint8, device="cuda")
    hist = Out(4 * 3 * 256)
    L = lib.load()
    for args in ((4, 4, 5, -1), (0, 4, 3, -1), (4, 4, 3, 256)):
        assert L.dsic_band_histogram_u8(_p(img), None, *args, _p(hist.view), _stream()) == lib.DSIC_EINVAL
    assert L.dsic_band_histogram_u8(_p(img), None, 4, 4, 3, -1, _p(hist.view[1:]), _stream()) == lib.DSIC_EINVAL
    assert (hist.host("refused calls") == U8_FILL).all()


# ---- the render kernels ---------------------------------------------------------------------------------------------
def _pairs(kind, C, turn):
    """lo == hi, the whole range, a narrow pair with samples on either side, a wide one: one per band, rotated"""
    top = TOP[kind]
    kinds = [(top // 3, top // 3), (0, top), (3 * (top // 8), 5 * (top // 8)), (top // 10, top - top // 10)]
    return [kinds[(c + turn) % 4] for c in range(C)]


def _render(kind, src, sval, c, C, bands, pairs, dst, mode, nodata, alpha, background):
    y0, x0, h, w = c["region"]
    oh, ow = c["size"]
    return getattr(lib.load(), "dsic_window_render_" + kind)(
        _p(src), None if sval is None else _p(sval), c["sh"], c["sw"], c["sy0"], c["sx0"], C, c["shift"], y0, x0, h, w,
        _c_int(bands), len(bands), codec._lohi(pairs), _p(dst), oh, ow, mode, -1 if nodata is None else nodata, alpha,
        background, _stream())


def _sweep(si, ki, kind, C, shift):
    """The thinned product: per (size, shift, kind) one (mode, mask) whose resample is restated once, and under it
    every band choice with alpha, background, stretch and the output's alignment taking turns."""
    turn = si * len(V.SHIFTS) + shift + ki
    masks = ["none", "valid", "nodata"] if kind == "u8" else ["none", "valid"]
    mode, mask = ("average", "nearest")[turn % 2], masks[(turn // 2) % len(masks)]
    shows = [((0,), turn % 2, (0, 200)[(turn // 2) % 2], turn), ((C - 1, 0, 0), (turn + 1) % 2, (200, 0)[(turn // 2) % 2],
                                                                  turn + 1)]
    if C >= 3:
        shows.append(((0, 1, 2), (turn // 3) % 2, 200 * ((turn // 5) % 2), turn + 2))
    return mode, mask, shows


def test_the_sweep_takes_every_value_of_every_axis():
    for ki, (kind, C) in enumerate(KINDS):
        seen = set()
        for si in range(len(V.SIZES)):
            for shift in V.SHIFTS:
                mode, mask, shows = _sweep(si, ki, kind, C, shift)
                seen |= {mode, mask, (mode, mask)} | {("alpha", a) for _, a, _, _ in shows}
                seen |= {("bg", b) for _, _, b, _ in shows} | {("bands", len(b), a) for b, a, _, _ in shows}
        masks = ["none", "valid"] + (["nodata"] if kind == "u8" else [])
        assert {(m, k) for m in ("average", "nearest") for k in masks} <= seen, (kind, C)
        assert {("alpha", 0), ("alpha", 1), ("bg", 0), ("bg", 200), ("bands", 3, 1), ("bands", 3, 0), ("bands", 1, 1),
                ("bands", 1, 0)} <= seen, (kind, C)


@pytest.mark.parametrize("si", range(len(V.SIZES)))
@pytest.mark.parametrize("ki", range(len(KINDS)))
def test_render_kernels_equal_the_restatement(si, ki):
    (src_size, out_size), (kind, C) = V.SIZES[si], KINDS[ki]
    for shift in V.SHIFTS:
        if src_size[1] > 1000 and shift != ki % len(V.SHIFTS):              # the long rows: one shift per kind
            continue
        c = V.kernel_case(src_size, out_size, shift)
        mode, mask, shows = _sweep(si, ki, kind, C, shift)
        img = V.kernel_image(kind, C, c["sh"], c["sw"])
        rng = np.random.default_rng(c["sh"] * 13 + c["sw"] + C)
        valid = None
        if mask == "valid":
            valid = rng.random((c["sh"], c["sw"])) < 0.7
            valid[:max(1, c["sh"] // 2), :max(1, c["sw"] // 2)] = False     # nothing valid under some outputs
            valid = valid.astype(np.uint8) * rng.integers(1, 256, size=valid.shape).astype(np.uint8)
        nodata = V.NODATA[kind] if mask == "nodata" else None
        elem = img.dtype.itemsize
        d_src, d_val = _inside(img, elem * (1 + shift)), None if valid is None else _inside(valid, 3)
        geo = (c["sy0"], c["sx0"], shift, c["region"], c["size"])
        if valid is None:
            res, ok = V.resample(img, *geo, mode, nodata if mode == "average" else None), None
        else:
            res, ok = R.valid_ref.resample(img, valid, *geo, mode, 0)
        for bands, alpha, background, turn in shows:
            pairs = _pairs(kind, C, turn)
            n = len(bands) + alpha
            what = (f"window_render_{kind} {src_size}->{out_size} C={C} shift={shift} {mode} {mask} bands={bands} "
                    f"alpha={alpha} background={background} {pairs}")
            want = R.display(res, ok, bands, pairs, alpha, background)
            for offset in {0, turn % 4}:                                     # 4 bytes per pixel: the dword stores and not
                out = Out(want.size, offset=offset)
                lib.check(_render(kind, d_src, d_val, c, C, bands, pairs, out.view, MODES[mode], nodata, alpha, background),
                          what)
                _same(out.host(what), want, what)
            assert want.shape == out_size + (n,)


def test_a_render_is_the_restated_render_of_the_source():
    """once through render_ref.render itself, so that its own composition of resample and display is held too"""
    c = V.kernel_case((17, 33), (5, 7), 1)
    for kind, C in (("u8", 4), ("u16", 2)):
        img = V.kernel_image(kind, C, c["sh"], c["sw"])
        valid = (np.random.default_rng(3).random((c["sh"], c["sw"])) < 0.5).astype(np.uint8)
        pairs = _pairs(kind, C, 1)
        for sval, nodata in ((None, None), (None, V.NODATA[kind]), (valid, None)):
            for mode in ("average", "nearest"):
                want = R.render(img, sval, c["sy0"], c["sx0"], 1, c["region"], c["size"], (C - 1, 0, 0), pairs, mode, nodata,
                                True, 77)
                out = Out(want.size)
                lib.check(_render(kind, _inside(img, 2), None if sval is None else _inside(sval, 1), c, C, (C - 1, 0, 0), pairs,
                                  out.view, MODES[mode], nodata, 1, 77), kind)
                _same(out.host(kind), want, f"{kind} {mode} nodata={nodata} valid={sval is not None}")


def test_render_calls_refuse_through_their_error_return_and_write_nothing():
    src = torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda")
    out = Out(4 * 4 * 4)
    ok = {"sh": 8, "sw": 8, "sy0": 0, "sx0": 0, "shift": 0, "region": (0, 0, 8, 8), "size": (4, 4)}
    full = [(0, 255)] * 3
    args = dict(bands=(0, 1, 2), pairs=full, mode=0, nodata=None, alpha=1, background=0)
    for change, word in (({"bands": (0, 1)}, "nb=2"), ({"bands": (0, 1, 3)}, "band 3"), ({"pairs": [(9, 8)] * 3}, "(9, 8)"),
                         ({"pairs": [(0, 256)] * 3}, "(0, 256)"), ({"alpha": 2}, "alpha=2"), ({"background": 256}, "background"),
                         ({"mode": 3}, "mode=3"), ({"nodata": 256}, "nodata=256")):
        p = dict(args, **change)
        assert _render("u8", src, None, ok, 3, p["bands"], p["pairs"], out.view, p["mode"], p["nodata"], p["alpha"],
                       p["background"]) == lib.DSIC_EINVAL
        assert word.encode() in lib.load().dsic_last_error(), word
    for change, word in (({"region": (0, 0, 9, 8)}, "outside the source window"), ({"shift": 16}, "shift=16"),
                         ({"size": (0, 4)}, "output")):
        assert _render("u8", src, None, dict(ok, **change), 3, (0, 1, 2), full, out.view, 0, None, 1, 0) == lib.DSIC_EINVAL
        assert word.encode() in lib.load().dsic_last_error()
    assert _render("u8", src, None, ok, 5, (0, 1, 2), full, out.view, 0, None, 1, 0) == lib.DSIC_EINVAL
    assert _render("u8", src, out.view[:64], ok, 3, (0, 1, 2), full, out.view, 0, None, 1, 0) == lib.DSIC_EINVAL
    assert b"overlap" in lib.load().dsic_last_error()                        # dst over the validity window
    assert (out.host("refused calls") == U8_FILL).all() and not bool(src.any())


# ---- the reader -----------------------------------------------------------------------------------------------------
H0, W0, TILE, BATCH, NODATA, FILL = 150, 200, 64, 4, 7, 9
ARGS = {"tile": TILE, "batch": BATCH}
SCALE = [(0, 12000), (100, 11000), (0, 65535), (500, 9000)]
STREAMS = {"u8": ("u8", 3, {}), "f32": ("f32", 3, {}), "u8_nodata": ("u8", 3, {"nodata": NODATA}),
           "u8_valid": ("u8", 3, {"valid": True, "fill": FILL, "overviews": 2}),
           "u16": ("u16", 4, {"scale": SCALE, "overviews": 2}),
           "u16_valid": ("u16", 4, {"scale": SCALE, "valid": True, "fill": 0, "overviews": 2}),
           "u16_tol": ("u16", 4, {"scale": SCALE, "tolerance": 8})}


def _model(in_ch):
    if ("model", in_ch) not in _CACHE:
        sd = S.make_state_dict(seed=1, N=128, M=192, in_ch=in_ch, spatial_params=False)
        m = CompressionModel(N=128, M=192, spatial_params=False, min_nu=2, max_nu=100.0, in_ch=in_ch)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        _CACHE[("model", in_ch)] = (m.cuda().eval(), sd)
    return _CACHE[("model", in_ch)][0]


def _valid():
    """a wedge that empties the first tiles, and a speckled block"""
    yy, xx = np.mgrid[:H0, :W0]
    valid = ~(2 * yy + xx < 200)
    valid[100:140, 120:180] &= ~(np.random.default_rng(5).random((40, 60)) < 0.5)
    return valid


def _stream_of(name):
    if ("stream", name) not in _CACHE:
        kind, in_ch, kw = STREAMS[name]
        kw = dict(kw)
        x = S.make_patches(21, 1, H0, W0, in_ch)[0].astype(np.float32)
        if kind == "f32":
            img = np.ascontiguousarray(x)
        elif kind == "u8":
            img = np.ascontiguousarray((x * 255 + 0.5).astype(np.uint8).transpose(1, 2, 0))
        else:
            img = np.ascontiguousarray((x * 10000 + 0.5).astype(np.uint16).transpose(1, 2, 0))
            img[20:24, 30:34] = 65535                                        # the hot pixels a percentile stretch ignores
        if "nodata" in kw:
            img[~_valid()] = NODATA
        if kw.pop("valid", False):
            kw["valid"] = torch.from_numpy(_valid()).cuda()
        _CACHE[("stream", name)] = codec.compress_image(_model(in_ch), torch.from_numpy(img).cuda(), **ARGS, **kw)
    return _CACHE[("stream", name)]


def _reader(name, **kw):
    return codec.ImageReader(_model(STREAMS[name][1]), _stream_of(name), batch=BATCH, **kw)


def _np(t):
    return t.cpu().numpy()


def _read(r, name, win, size, level, resampling):
    """what read gives for the request, as (image, validity or None): through out="u8" for a float32-kind stream, with
    the validity wherever read can give it"""
    out = "u8" if STREAMS[name][0] == "f32" else None
    if "nodata" in STREAMS[name][2]:                                         # its mask is by value
        return _np(r.read(*win, size=size, level=level, out=out, resampling=resampling)), None
    img, valid = r.read(*win, size=size, level=level, out=out, resampling=resampling, with_valid=True)
    return _np(img), _np(valid)


# inside one tile; across four tiles; the whole image at a quarter of its size; magnified; and windows as they are
U16_PAIRS = [(300, 9000), (0, 65535), (4000, 4000), (0, 12000)]         # the scene's values lie in 0 .. 10000
REQUESTS = [((5, 7, 40, 50), (20, 25), None), ((40, 40, 60, 70), (45, 52), None), ((0, 0, H0, W0), (37, 50), None),
            ((100, 150, 10, 12), (25, 31), None), ((30, 50, 50, 60), None, None), ((90, 100, 21, 33), (21, 33), 0)]


@pytest.mark.parametrize("name", list(STREAMS))
def test_a_render_is_the_stretch_of_the_read(name):
    kind, C, kw = STREAMS[name]
    top = 65535 if kind == "u16" else 255
    pairs = U16_PAIRS if kind == "u16" else _pairs("u8", C, 1)
    masked, pyramid = "valid" in kw, "overviews" in kw
    with _reader(name) as r, _reader(name) as plain:
        assert len(r.levels) == (3 if pyramid else 1)
        for k, (win, size, level) in enumerate(REQUESTS):
            for resampling in ("average", "nearest") if size is not None else ("average",):
                st = {}
                bands = [(0, 1, 2), (C - 1, 0, 0), (1,)][k % 3]
                alpha, background = bool(k % 2) and "nodata" not in kw, (0, 200)[(k // 2) % 2]
                got = r.render(*win, size=size, level=level, bands=bands, stretch=pairs, alpha=alpha, background=background,
                               resampling=resampling, stats=st)
                img, valid = _read(plain, name, win, size, level, resampling)
                assert img.dtype == (np.uint16 if top == 65535 else np.uint8)
                want = R.display(img, valid, bands, pairs, alpha, background)
                assert got.is_cuda and got.dtype == torch.uint8 and got.is_contiguous()
                assert got.shape == want.shape and np.array_equal(_np(got), want), (name, win, size, resampling)
                if size == (37, 50):
                    assert st["level"] == (2 if pyramid else 0)
                if masked and size is not None and win[0] == 0:
                    assert not valid.all() and valid.any()
                    assert (_np(got)[~valid][:, :len(bands)] == background).all()
        if pyramid:                                                          # a level's own window, as it is
            got = r.render(3, 5, 60, 80, level=1, stretch=pairs, alpha=masked, background=50)
            img, valid = _read(plain, name, (3, 5, 60, 80), None, 1, "average")
            assert np.array_equal(_np(got), R.display(img, valid, (0, 1, 2), pairs, masked, 50))
        defaults = r.render(40, 40, 60, 70, size=(45, 52))                   # bands and stretch by default
        img, valid = _read(plain, name, (40, 40, 60, 70), (45, 52), None, "average")
        if kind == "u16":
            auto = r.stretch()
            assert auto == codec.stretch_from_histogram(r.histogram(), (2, 98)) and all(hi < 65535 for _, hi in auto)
            assert np.array_equal(_np(defaults), R.display(img, valid, (0, 1, 2), auto))
            assert np.array_equal(_np(defaults), _np(r.render(40, 40, 60, 70, size=(45, 52), stretch=auto)))
        else:
            assert np.array_equal(_np(defaults)[valid if valid is not None else ...],
                                  img[valid if valid is not None else ...][..., :3])     # (0, 255): the bytes themselves


@pytest.mark.parametrize("name", list(STREAMS))
def test_the_histogram_counts_the_levels_valid_pixels_once(name):
    kind, C, kw = STREAMS[name]
    with _reader(name) as r, _reader(name) as plain:
        n = len(r.levels)
        for level in [None] + list(range(n)):
            h, w = r.levels[n - 1 if level is None else level]
            before = r.stats
            got = r.histogram(level)
            first = r.stats["decoded"] - before["decoded"]
            img, valid = _read(plain, name, (0, 0, h, w), None, n - 1 if level is None else level, "average")
            want = R.histogram(img, None if "nodata" in kw else valid, kw.get("nodata"))
            assert got.dtype == np.int64 and got.shape == (C, 65536 if kind == "u16" else 256)
            assert np.array_equal(got, want), (name, level)
            if "valid" in kw or "nodata" in kw:
                assert 0 < got[0].sum() < h * w
            before = r.stats
            assert np.array_equal(r.histogram(level), got)
            assert r.stats["decoded"] == before["decoded"] and r.stats["bytes_read"] == before["bytes_read"]
            assert (first > 0) == (level is None or level != n - 1)         # the default is the coarsest level
        assert r.stretch((0, 100)) == R.percentile_stretch(r.histogram(), (0, 100))
        level0 = r.histogram(0)
    with _reader(name, cache_bytes=0) as r:                                  # strips beside the cache: the same counts
        assert np.array_equal(r.histogram(0), level0)


def test_render_many_is_the_list_of_renders_and_shares_the_decode_batches():
    for name in ("u8_valid", "u16"):
        C = STREAMS[name][1]
        pairs = U16_PAIRS if name == "u16" else _pairs("u8", C, 2)
        reqs = [{"window": win, "size": size, "level": level, "stretch": pairs, "bands": [(0, 1, 2), (C - 1, 0, 0), (1,)][k % 3]}
                for k, (win, size, level) in enumerate(REQUESTS)] + [{"window": (5, 7, 40, 50), "stretch": pairs}]
        with _reader(name) as one:
            want = [one.render(*q["window"], size=q.get("size"), level=q.get("level"), bands=q.get("bands"),
                               stretch=q["stretch"], alpha=True, background=31) for q in reqs]
        with _reader(name) as r, _reader(name) as reads:
            st, st_reads = {}, {}
            got = r.render_many(reqs, alpha=True, background=31, stats=st)
            reads.read_many([{k: v for k, v in q.items() if k in ("window", "size", "level")} for q in reqs], stats=st_reads)
            assert len(got) == len(want) and all(torch.equal(g, w) for g, w in zip(got, want))
            assert st["decode_batches"] <= st_reads["decode_batches"] and st["decoded"] == st_reads["decoded"] > 0
            assert sorted(st["tiles"]) == sorted(st_reads["tiles"])
            again = {}
            assert all(torch.equal(g, w) for g, w in zip(r.render_many(reqs, alpha=True, background=31, stats=again), want))
            assert (again["decoded"], again["decode_batches"]) == (0, 0)
        with _reader(name, cache_bytes=3 * 4 * C * TILE * TILE) as r:      # the union does not fit: one by one
            assert all(torch.equal(g, w) for g, w in zip(r.render_many(reqs, alpha=True, background=31), want))
    with _reader("u16") as r:                                                # no stretch given: the reader's own,
        st = {}                                                              # and its histogram's tiles are counted
        got = r.render_many([{"window": (5, 7, 40, 50), "size": (40, 50)}], stats=st)[0]
        assert {l for l, _ in st["tiles"]} == {0, 2} and st["decoded"] == r.stats["decoded"] == len(st["tiles"])
        assert st["bytes_read"] > 0 and st["decode_batches"] == 2
        auto, again = r.stretch(), {}
        assert torch.equal(got, r.render(5, 7, 40, 50, size=(40, 50), stretch=auto))
        assert torch.equal(got, r.render(5, 7, 40, 50, size=(40, 50), stats=again)) and again["decoded"] == 0


def test_the_readers_refusals():
    with _reader("u16") as r:
        full = [(0, 65535)] * 4
        for kw, word in (({"bands": (0, 1)}, "bands"), ({"bands": (4,)}, "bands"), ({"stretch": full[:3]}, "stretch"),
                         ({"stretch": [(0, 65536)] * 4}, "stretch"), ({"stretch": [(9, 8)] * 4}, "stretch"),
                         ({"background": 256}, "background"), ({"background": -1}, "background"),
                         ({"resampling": "cubic"}, "resampling"), ({"level": 3}, "levels 0 .. 2")):
            before = r.stats
            with pytest.raises(ValueError, match=word):
                r.render(0, 0, 64, 64, size=(16, 16), **dict({"stretch": full}, **kw))
            assert r.stats["decoded"] == before["decoded"]
        with pytest.raises(ValueError, match="window"):
            r.render(0, 0, H0 + 1, 8, size=(4, 4), stretch=full)
        with pytest.raises(ValueError, match="levels 0 .. 2"):
            r.histogram(3)
        with pytest.raises(ValueError, match="percent"):
            r.stretch((98, 2))
        assert r.stats["decoded"] == 0
    with _reader("u8") as r:
        with pytest.raises(ValueError, match="stretch"):
            r.render(0, 0, 8, 8, stretch=[(0, 256)] * 3)
    with _reader("u8_nodata") as r:
        with pytest.raises(ValueError, match="valid="):
            r.render(0, 0, 64, 64, size=(16, 16), alpha=True)
        assert r.stats["decoded"] == 0
    r = _reader("u8")
    r.close()
    with pytest.raises(ValueError, match="closed"):
        r.render(0, 0, 8, 8)
    with pytest.raises(ValueError, match="closed"):
        r.histogram()


def test_the_tool_renders_into_npy_and_ppm(tmp_path):
    model, stream = _model(4), _stream_of("u16_valid")
    sd = _CACHE[("model", 4)][1]
    torch.save({"model": {k: torch.from_numpy(v) for k, v in sd.items()}}, tmp_path / "ckpt.pt")
    (tmp_path / "s.dsic").write_bytes(stream)
    tool = os.path.join(ROOT, "tools", "dsic_image.py")
    head = [sys.executable, tool, "render", str(tmp_path / "s.dsic")]
    tail = ["--weights", str(tmp_path / "ckpt.pt"), "--batch", str(BATCH)]
    runs = [(["--region", "0,0,150,200", "--size", "37,50", "--bands", "3,0,1", "--alpha", "--background", "60"], "a.npy"),
            (["--size", "75,100", "--percent", "0,100", "--resampling", "nearest"], "b.ppm")]
    outs = []
    for extra, dst in runs:
        p = subprocess.run(head + [str(tmp_path / dst)] + extra + tail, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stdout + p.stderr
        outs.append(p.stdout)
    with codec.ImageReader(model, io.BytesIO(stream), batch=BATCH) as r:
        auto, whole = r.stretch(), r.stretch((0, 100))
        a = _np(r.render(0, 0, H0, W0, size=(37, 50), bands=(3, 0, 1), stretch=auto, alpha=True, background=60))
        b = _np(r.render(0, 0, H0, W0, size=(75, 100), stretch=whole, resampling="nearest"))
    assert np.array_equal(np.load(tmp_path / "a.npy"), a) and a.shape == (37, 50, 4) and (a[..., 3] == 0).any()
    assert (tmp_path / "b.ppm").read_bytes() == b"P6\n100 75\n255\n" + b.tobytes()
    assert "level 2" in outs[0] and "37x50" in outs[0] and "bands 3,0,1 + alpha" in outs[0]
    assert "stretch " + ", ".join(f"({lo}, {hi})" for lo, hi in auto) in outs[0]
    assert "level 1" in outs[1] and "stretch " + ", ".join(f"({lo}, {hi})" for lo, hi in whole) in outs[1]
