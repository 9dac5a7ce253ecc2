"""Warped reads on the GPU.  The warp and warp-render kernels alone, bit for bit against the restatement of
tests/warp_ref.py, outputs between guards and inputs inside a larger allocation as in test_gpu_pyramid.py; then
codec.ImageReader.read_warped / render_warped on the 330 x 530 scene of that file and of test_gpu_valid.py: a warped
read is the restatement applied to decompress_region's output of the planned window, for every kind of stream; and the
command-line tool."""
import ctypes
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import render_ref as D
import warp_ref as R
from dsic_amd import codec, lib
from dsic_amd.ops import _p, _stream
from test_gpu_pyramid import _CACHE as _PCACHE
from test_gpu_pyramid import BATCH, H0, W0, Out, _alone, _inside, _model, _same
from test_gpu_valid import _model as _valid_model
from test_gpu_valid import _pyramid as _valid_pyramid
from test_gpu_view import _stream_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = 65536
MASKS = ("none", "valid", "nodata")


# ---- the kernels ----------------------------------------------------------------------------------------------------
def _head(src, sval, c, C):
    return (_p(src), None if sval is None else _p(sval), c["sh"], c["sw"], c["sy0"], c["sx0"], C, c["shift"], c["LH"],
            c["LW"], c["H"], c["W"], (ctypes.c_int64 * 6)(*c["m"]))


def _warp(kind, src, sval, c, C, dst, oval, mode, nodata, fill):
    return getattr(lib.load(), "dsic_window_warp_" + kind)(
        *_head(src, sval, c, C), _p(dst), None if oval is None else _p(oval), *c["size"], mode,
        -1 if nodata is None else nodata, fill, _stream())


def _warp_render(kind, src, sval, c, C, bands, pairs, dst, mode, nodata, alpha, background):
    return getattr(lib.load(), "dsic_window_warp_render_" + kind)(
        *_head(src, sval, c, C), (ctypes.c_int * len(bands))(*bands), len(bands), codec._lohi(pairs), _p(dst), *c["size"],
        mode, -1 if nodata is None else nodata, alpha, background, _stream())


def _cut(a, c):
    return np.ascontiguousarray(a[c["sy0"]:c["sy0"] + c["sh"], c["sx0"]:c["sx0"] + c["sw"]])


def _sweep(si, ki, k):
    """The thinned product: per (source size, kind, matrix) one shift, output size, mask and window margin; all three
    modes run under it."""
    turn = si + ki + k
    return R.SHIFTS[turn % 3], R.OUT_SIZES[(2 * si + ki + k) % 5], MASKS[(si + ki // 3 + k // 3 + k) % 3], (turn // 2) % 2


def test_the_sweep_takes_every_value_of_every_axis():
    for ki in range(len(R.KINDS)):
        seen = set()
        for si in range(len(R.SRC_SIZES)):
            for k, name in enumerate(R.MATRICES):
                l, out_size, mask, margin = _sweep(si, ki, k)
                seen |= {("shift", l), ("out", out_size), ("mask", mask), ("margin", margin), (name, mask), (name, l),
                         (R.SRC_SIZES[si], l), (R.SRC_SIZES[si], mask)}
        assert {("shift", l) for l in R.SHIFTS} | {("out", s) for s in R.OUT_SIZES} | {("mask", m) for m in MASKS} <= seen
        assert {(s, l) for s in R.SRC_SIZES for l in R.SHIFTS} | {(s, m) for s in R.SRC_SIZES for m in MASKS} <= seen
        assert {("margin", 0), ("margin", 1)} <= seen
    pairs = {(name, _sweep(si, ki, k)[2]) for ki in range(len(R.KINDS)) for si in range(len(R.SRC_SIZES))
             for k, name in enumerate(R.MATRICES)}
    assert pairs == {(name, m) for name in R.MATRICES for m in MASKS}


@pytest.mark.parametrize("si", range(len(R.SRC_SIZES)))
@pytest.mark.parametrize("ki", range(len(R.KINDS)))
def test_warp_kernels_equal_the_restatement(si, ki):
    src_size, (kind, C) = R.SRC_SIZES[si], R.KINDS[ki]
    img, fill = R.level_image(kind, C, *src_size), R.FILL[kind]
    inside_some = 0
    for k, name in enumerate(R.MATRICES):
        l, out_size, mask, margin = _sweep(si, ki, k)
        val = R.validity(*src_size, seed=k) if mask == "valid" else None
        nodata = R.NODATA[kind] if mask == "nodata" else None
        for mode in (0, 1, 2):
            c = R.kernel_case(src_size, out_size, l, name, mode, margin)
            want, ok = R.run_case(img, val, c, mode, nodata, fill)
            src = _inside(_cut(img, c), (k + mode) % 4)                      # the input at several element offsets
            sval = None if val is None else _inside(_cut(val, c), (k + 2 * mode) % 4)
            out, oval = Out(want.size, img.dtype, (0, 1, 3, 2)[(k + mode) % 4]), Out(ok.size, np.uint8, (k + mode) % 3)
            what = f"window_warp_{kind} {src_size}->{out_size} C={C} shift={l} {name} mode={mode} {mask} margin={margin}"
            lib.check(_warp(kind, src, sval, c, C, out.view, oval.view, mode, nodata, fill), what)
            _same(out.host(what), want, what)
            _same(oval.host(what), ok.astype(np.uint8), what + " validity")
            inside_some += int(ok.any())
            if mode == 2 and k % 4 == 0:                                     # and without an output validity
                alone = Out(want.size, img.dtype, 1)
                lib.check(_warp(kind, src, sval, c, C, alone.view, None, mode, nodata, fill), what)
                _same(alone.host(what), want, what + " image alone")
    assert inside_some >= len(R.MATRICES)                                    # the sweep is not a sweep of empty views


def test_identity_rotation_and_halving_on_the_device():
    for kind, C in (("u8", 3), ("u16", 2)):
        img = R.level_image(kind, C, 40, 68)
        dev = torch.from_numpy(img).cuda()
        y0, x0, h, w = 5, 9, 23, 37
        base = {"sh": 40, "sw": 68, "sy0": 0, "sx0": 0, "LH": 40, "LW": 68}
        for mode in (0, 1, 2):
            for m, size, want in (((Q, 0, y0 * Q, 0, Q, x0 * Q), (h, w), img[y0:y0 + h, x0:x0 + w]),
                                  ((0, Q, y0 * Q, -Q, 0, (x0 + w) * Q), (w, h), np.rot90(img[y0:y0 + h, x0:x0 + w]))):
                out = Out(h * w * C, img.dtype)
                c = dict(base, H=40, W=68, shift=0, m=m, size=size)
                lib.check(_warp(kind, dev, None, c, C, out.view, None, mode, None, 0), kind)
                _same(out.host(kind), want, f"{kind} mode {mode} {m}")
            out = Out(img.size, img.dtype)
            c = dict(base, H=80, W=136, shift=1, m=(2 * Q, 0, 0, 0, 2 * Q, 0), size=(40, 68))
            lib.check(_warp(kind, dev, None, c, C, out.view, None, mode, None, 0), kind)
            _same(out.host(kind), img, f"{kind} mode {mode} halving")


# ---- the render exports ---------------------------------------------------------------------------------------------
RENDERS = [((17, 33), (16, 16), 0, "rot30", "valid"), ((40, 68), (70, 130), 1, "overhang", "none"),
           ((5, 7), (17, 33), 2, "magnify3", "nodata"), ((40, 68), (7, 9), 0, "shear", "valid"),
           ((2, 2), (1, 1), 0, "identity", "none")]


@pytest.mark.parametrize("kind,C", R.KINDS + [("u8", 1)])
def test_warp_render_kernels_equal_the_restated_display(kind, C):
    top = 255 if kind == "u8" else 65535
    for n, (src_size, out_size, l, name, mask) in enumerate(RENDERS):
        img = R.level_image(kind, C, *src_size)
        val = R.validity(*src_size, seed=n) if mask == "valid" else None
        nodata = R.NODATA[kind] if mask == "nodata" else None
        pairs = [[(top // 3, top // 3), (0, top), (3 * (top // 8), 5 * (top // 8)), (top // 10, top - top // 10)][(c + n) % 4]
                 for c in range(C)]
        for mode in (0, 1, 2):
            c = R.kernel_case(src_size, out_size, l, name, mode, n % 2)
            res, ok = R.run_case(img, val, c, mode, nodata, 0)
            src = _inside(_cut(img, c), 1 + mode)
            sval = None if val is None else _inside(_cut(val, c), 3)
            # 4 bytes per pixel at an aligned and at an odd address (the dword stores and not), and 1, 2 and 3 bytes
            shows = [((C - 1, 0, 0), 1, 200, 0), ((C - 1, 0, 0), 1, 0, 1 + mode), ((0,), 0, 77, 0), ((C - 1,), 1, 9, 2)]
            if C >= 3:
                shows.append(((0, 1, 2), 0, 200, mode))
            for bands, alpha, background, offset in shows:
                want = D.display(res, ok, bands, pairs, alpha, background)
                out = Out(want.size, np.uint8, offset)
                what = (f"window_warp_render_{kind} {src_size}->{out_size} C={C} shift={l} {name} mode={mode} {mask} "
                        f"bands={bands} alpha={alpha} background={background} offset={offset}")
                lib.check(_warp_render(kind, src, sval, c, C, bands, pairs, out.view, mode, nodata, alpha, background), what)
                _same(out.host(what), want, what)
            if name == "overhang":
                assert not ok.all() and ok.any()


# ---- refusals -------------------------------------------------------------------------------------------------------
def test_the_calls_refuse_through_their_error_return_and_write_nothing():
    src = torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda")
    out, oval = Out(8 * 8 * 4, np.uint8), Out(64, np.uint8)
    ok = {"sh": 8, "sw": 8, "sy0": 0, "sx0": 0, "shift": 0, "LH": 8, "LW": 8, "H": 8, "W": 8, "m": (Q, 0, 0, 0, Q, 0),
          "size": (8, 8)}
    full = [(0, 255)] * 3
    for change, C, mode, word in (({"sh": 7}, 3, 0, "outside the source window"), ({}, 3, 3, "mode=3"),
                                  ({"m": ((1 << 26) + 1, 0, 0, 0, Q, 0)}, 3, 0, "matrix entry 0"), ({}, 2, 0, "C=2"),
                                  ({}, 5, 0, "C=5"), ({"size": (8, (1 << 20) + 1)}, 3, 0, "output")):
        c = dict(ok, **change)
        assert _warp("u8", src, None, c, C, out.view, oval.view, mode, None, 0) == lib.DSIC_EINVAL
        assert word.encode() in lib.load().dsic_last_error(), word
        if C != 2:
            assert _warp_render("u8", src, None, c, C, (0, 1, 2), full, out.view, mode, None, 1, 0) == lib.DSIC_EINVAL
            assert word.encode() in lib.load().dsic_last_error(), word
    assert _warp("u8", src, None, ok, 3, out.view, out.view[100:], 0, None, 0) == lib.DSIC_EINVAL
    assert b"overlap" in lib.load().dsic_last_error()                        # the output validity inside the output
    assert _warp("u8", src, out.view[:64], ok, 3, out.view, None, 0, None, 0) == lib.DSIC_EINVAL
    assert b"overlap" in lib.load().dsic_last_error()                        # dst over the validity window
    assert _warp_render("u8", src, out.view[:64], ok, 3, (0, 1, 2), full, out.view, 0, None, 1, 0) == lib.DSIC_EINVAL
    assert _warp("u8", src, None, ok, 3, src, None, 0, None, 0) == lib.DSIC_EINVAL
    with pytest.raises(ValueError, match="band 3"):
        lib.check(_warp_render("u8", src, None, ok, 3, (0, 1, 3), full, out.view, 0, None, 1, 0), "window_warp_render_u8")
    assert (out.host("refused calls") == 0x5A).all() and (oval.host("refused calls") == 0x5A).all() and not bool(src.any())


# ---- the reader -----------------------------------------------------------------------------------------------------
STREAMS = ["plain", "segments", "overlap", "max_error", "nodata", "u16", "masked u8", "masked u16", "pyramid"]


def _open(name):
    """(model, stream) of a stream kind"""
    if name.startswith("masked"):
        config = name.split()[1]
        return _valid_model(4 if config == "u16" else 3), _valid_pyramid(config)
    return _model(), _stream_of(name)


def _views():
    """(matrix, size, level, resampling): turned, magnified, minified onto an overview, overhanging, mirrored"""
    return [(codec.rotation_affine(160, 260, 30, 1.25, 96, 120), (96, 120), None, "bilinear"),
            (codec.rotation_affine(300, 500, -20, 0.3, 50, 70), (50, 70), None, "cubic"),
            (codec.window_affine(3, 5, 320, 512, 80, 128), (80, 128), None, "cubic"),
            (codec.rotation_affine(165, 265, 90, 2.5, 200, 150), (200, 150), None, "bilinear"),
            ([[-1, 0, 200], [0, 1, 100.5]], (64, 64), 0, "nearest"),
            (codec.window_affine(250, 380, 70, 90, 50, 60), (50, 60), None, "bilinear")]


def _restated(model, stream, st, size, resampling, ix0):
    """the restatement applied to decompress_region of the planned window"""
    level, lw, m = st["level"], st["level_window"], st["matrix_q16"]
    ix = codec.stream_index(stream, level=level)
    masked = "fill" in ix
    src = codec.decompress_region(model, stream, *lw, batch=BATCH, level=level, with_valid=masked)
    src, sval = (src[0].cpu().numpy(), src[1].cpu().numpy().astype(np.uint8)) if masked else (src.cpu().numpy(), None)
    fill = ix.get("fill", ix.get("nodata", 0))
    return R.warp(src, sval, lw[0], lw[1], level, ix["H"], ix["W"], ix0["H"], ix0["W"], m, size, R.MODES[resampling],
                  ix.get("nodata"), fill)


@pytest.mark.parametrize("name", STREAMS)
def test_a_warped_read_is_the_restatement_of_the_planned_window(name):
    model, stream = _open(name)
    ix0 = codec.stream_index(stream)
    levels = len(ix0.get("levels", [0]))
    with codec.ImageReader(model, stream, batch=BATCH) as r:
        for matrix, size, level, resampling in _views():
            st, again = {}, {}
            got, valid = r.read_warped(matrix, size, level=level, resampling=resampling, stats=st, with_valid=True)
            m = codec.affine_q16(matrix)
            assert st["matrix_q16"] == m and st["level"] == (codec.warp_level(levels, m) if level is None else level)
            lw = st["level_window"]
            LH, LW = r.levels[st["level"]]
            assert lw == codec.warp_window(st["level"], LH, LW, H0, W0, m, *size, R.MODES[resampling])
            want, ok = _restated(model, stream, st, size, resampling, ix0)
            assert got.is_cuda and got.is_contiguous() and tuple(got.shape) == size + (ix0["C"],)
            _same(got.cpu().numpy().ravel(), want, f"{name} {matrix} {resampling}")
            assert valid.dtype == torch.bool and np.array_equal(valid.cpu().numpy(), ok), (name, matrix)
            ix = codec.stream_index(stream, level=st["level"])
            assert st["tiles"] == [(st["level"], t) for t in codec.window_tiles(ix, *lw)]
            same = r.read_warped(matrix, size, level=level, resampling=resampling, stats=again)
            assert again["decoded"] == 0 and again["hits"] == len(codec._coded_tiles(ix, [t for _, t in again["tiles"]]))
            assert torch.equal(same.view(torch.uint8), got.view(torch.uint8))
        if name.startswith("masked"):
            assert not ok.all() and ok.any()                                 # the last view meets the speckled block
        if levels > 1:
            assert {1, 0} <= {codec.warp_level(levels, codec.affine_q16(v[0])) for v in _views()}


@pytest.mark.parametrize("name", ["plain", "u16", "pyramid", "masked u8"])
def test_identity_halving_and_views_beside_the_image(name):
    model, stream = _open(name)
    with codec.ImageReader(model, stream, batch=BATCH) as r:
        C = r.shape[2]
        for resampling in ("bilinear", "cubic", "nearest"):
            st = {}
            got = r.read_warped(codec.window_affine(40, 50, 33, 35, 33, 35), (33, 35), resampling=resampling, stats=st)
            want = r.read(40, 50, 33, 35)
            assert st["level"] == 0 and np.array_equal(got.cpu().numpy(), want.cpu().numpy()), (name, resampling)
            if len(r.levels) > 1:                                            # the halving view takes level 1 as it is
                # the last row and column of level 1 have their centres on the image's edge: outside
                got = r.read_warped([[2, 0, 0], [0, 2, 0]], (165, 265), resampling=resampling, stats=st)
                assert st["level"] == 1 and st["level_window"] == (0, 0, 165, 265)
                assert np.array_equal(got.cpu().numpy(), r.read(0, 0, 165, 265, level=1).cpu().numpy()), (name, resampling)
        before, st = r.stats, {}
        fill = r.index(0).get("fill", 0)
        got, valid = r.read_warped([[1, 0, 400], [0, 1, 0]], (20, 30), stats=st, with_valid=True)
        assert st["level_window"] is None and st["tiles"] == [] and r.stats["decoded"] == before["decoded"]
        assert tuple(got.shape) == (20, 30, C) and bool((got.cpu().numpy() == fill).all()) and not bool(valid.any())
        shown = r.render_warped([[1, 0, 0], [0, 1, -900]], (20, 30), alpha=name != "nodata", background=31, stats=st)
        assert st["tiles"] == [] and r.stats["decoded"] == before["decoded"]
        assert np.array_equal(shown.cpu().numpy()[..., :3], np.full((20, 30, 3), 31)) and not bool(shown[..., 3].any())


@pytest.mark.parametrize("name", ["plain", "nodata", "u16", "masked u8", "masked u16", "pyramid"])
def test_a_warped_render_is_the_stretch_of_the_warped_read(name):
    model, stream = _open(name)
    with codec.ImageReader(model, stream, batch=BATCH) as r, codec.ImageReader(model, stream, batch=BATCH) as plain:
        C, top = r.shape[2], 65535 if r.kind == codec.KIND_U16_HWC else 255
        pairs = [[(top // 10, top - top // 10), (0, top), (top // 4, top // 2), (top // 3, top // 3)][c] for c in range(C)]
        for k, (matrix, size, level, resampling) in enumerate(_views()):
            bands = [(0, 1, 2), (C - 1, 0, 0), (1,)][k % 3]
            alpha, background = bool(k % 2) and name != "nodata", (0, 200)[(k // 2) % 2]
            got = r.render_warped(matrix, size, level=level, bands=bands, stretch=pairs, alpha=alpha, background=background,
                                  resampling=resampling)
            img, valid = plain.read_warped(matrix, size, level=level, resampling=resampling, with_valid=True)
            want = D.display(img.cpu().numpy(), valid.cpu().numpy(), bands, pairs, alpha, background)
            assert got.dtype == torch.uint8 and got.is_contiguous() and np.array_equal(got.cpu().numpy(), want), (name, k)
        inside = codec.window_affine(100, 200, 40, 60, 100, 150)             # inside the image: the stretch throughout
        if not name.startswith("masked"):
            got = r.render_warped(inside, (100, 150), stretch=pairs)
            img = plain.read_warped(inside, (100, 150)).cpu().numpy()
            assert np.array_equal(got.cpu().numpy(), D.display(img, None, (0, 1, 2), pairs))
        if top == 65535:                                                     # the default stretch is render's
            auto = r.stretch()
            assert torch.equal(r.render_warped(inside, (100, 150)), r.render_warped(inside, (100, 150), stretch=auto))


def test_the_readers_refusals():
    with codec.ImageReader(_model(), _stream_of("pyramid"), batch=BATCH) as r:
        eye = [[1, 0, 0], [0, 1, 0]]
        for kw, word in (({"out": "f32"}, "float32"), ({"out": "u4"}, "out="), ({"out": "u16"}, "u16"),
                         ({"resampling": "average"}, "resampling"), ({"level": 4}, "levels 0 .. 3"),
                         ({"size": (0, 4)}, "size"), ({"size": (4,)}, "size"), ({"size": (4, (1 << 20) + 1)}, "size"),
                         ({"matrix": [[2000, 0, 0], [0, 1, 0]]}, "1024"), ({"matrix": [[1, 0], [0, 1]]}, "matrix")):
            args = dict({"matrix": eye, "size": (8, 8)}, **kw)
            with pytest.raises(ValueError, match=word):
                r.read_warped(**args)
        for kw, word in (({"bands": (0, 1)}, "bands"), ({"stretch": [(9, 8)] * 3}, "stretch"), ({"background": 256}, "background"),
                         ({"resampling": "average"}, "resampling")):
            with pytest.raises(ValueError, match=word):
                r.render_warped(eye, (8, 8), **kw)
        assert r.stats["decoded"] == 0
    f32 = _alone("f32", 0)                                                   # the float32-kind stream of the scene
    assert codec.stream_index(f32)["kind"] == codec.KIND_F32_CHW
    with codec.ImageReader(_model(), f32, batch=BATCH) as r:
        with pytest.raises(ValueError, match="float32"):
            r.read_warped([[1, 0, 0], [0, 1, 0]], (8, 8))                    # a float32-kind stream with out=None
        got = r.read_warped([[1, 0, 10], [0, 1, 20]], (8, 8), out="u8")
        assert np.array_equal(got.cpu().numpy(), r.read(10, 20, 8, 8, out="u8").cpu().numpy())
        shown = r.render_warped([[1, 0, 10], [0, 1, 20]], (8, 8))            # rendered from its out="u8" form
        assert np.array_equal(shown.cpu().numpy(), got.cpu().numpy())


# ---- the tool -------------------------------------------------------------------------------------------------------
def test_the_tool_renders_a_turned_view(tmp_path):
    model, stream = _model(), _stream_of("pyramid")
    sd = _PCACHE[("model", 3, 128, 192)][1]
    torch.save({"model": {k: torch.from_numpy(v) for k, v in sd.items()}}, tmp_path / "ckpt.pt")
    (tmp_path / "s.dsic").write_bytes(stream)
    tool = os.path.join(ROOT, "tools", "dsic_image.py")
    p = subprocess.run([sys.executable, tool, "render", str(tmp_path / "s.dsic"), str(tmp_path / "view.npy"), "--weights",
                        str(tmp_path / "ckpt.pt"), "--batch", str(BATCH), "--rotate", "30", "--center", "160,260", "--scale",
                        "2.5", "--size", "64,100", "--resampling", "cubic", "--alpha"], cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    with codec.ImageReader(model, io.BytesIO(stream), batch=BATCH) as reader:
        want = reader.render_warped(codec.rotation_affine(160, 260, 30, 2.5, 64, 100), (64, 100), resampling="cubic",
                                    alpha=True)
    assert np.array_equal(np.load(tmp_path / "view.npy"), want.cpu().numpy()) and want.shape == (64, 100, 4)
    assert "64x100" in p.stdout and "level 1" in p.stdout
