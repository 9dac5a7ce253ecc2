"""Scene stacks on the GPU.  The composite kernels alone, bit for bit against the NumPy restatement of
tests/composite_ref.py, outputs between guards and inputs inside larger allocations at odd and 2-byte alignments as in
test_gpu_render.py; then codec.SceneStack on the 150 x 200 scenes of test_gpu_render.py and three more of other seeds: a
read is the restated composite of what the readers themselves return for the scenes' parts, for a uint16 mosaic over
three levels and a uint8 temporal stack; render; the refusals; and the command-line tool."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import composite_ref as X
import composite_stream_cases  # noqa: F401  (its recipes join the table that test_gpu_stream_order.py runs)
import render_ref as R
from dsic_amd import codec, lib
from dsic_amd import synthetic as S
from dsic_amd.ops import _p, _stream
from test_gpu_render import _CACHE, ARGS, BATCH, H0, SCALE, STREAMS, U16_PAIRS, W0, _model, _np, _reader, _stream_of
from test_gpu_valid import U8_FILL, Out, _inside, _same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STACK = codec.SceneStack                         # the feature under test: without it nothing in this file is held


# ---- the kernels ----------------------------------------------------------------------------------------------------
def _composite(kind, srcs, masks, rects, nodata, C, dst, dval, dcnt, oh, ow, mode, fill):
    """uint16 sources at addresses that are 2-byte but not 4-byte aligned, uint8 ones and the validity at odd addresses;
    the device copies live until the kernel has run"""
    n, elem = len(srcs), srcs[0].dtype.itemsize
    d_src = [_inside(s, elem * (1 + 2 * (i % 2))) for i, s in enumerate(srcs)]
    d_val = [None if m is None else _inside(m, 1 + 2 * (i % 3)) for i, m in enumerate(masks)]
    status = getattr(lib.load(), "dsic_window_composite_" + kind)(
        (ctypes.c_void_p * n)(*[_p(t) for t in d_src]), (ctypes.c_void_p * n)(*[None if t is None else _p(t) for t in d_val]),
        (ctypes.c_int * (4 * n))(*[v for r in rects for v in r]), (ctypes.c_int * n)(*nodata), n, C, _p(dst),
        None if dval is None else _p(dval), None if dcnt is None else _p(dcnt), oh, ow, mode, fill, _stream())
    torch.cuda.synchronize()
    return status


def test_the_sweep_takes_every_value_of_every_axis():
    for ki, (kind, C) in enumerate(X.KINDS):
        seen = set()
        for si in range(len(X.SIZES)):
            for c in X.sweep(ki, si):
                seen |= {("n", c["n"]), ("mode", c["mode"]), ("layout", c["layout"]), ("validity", c["validity"]),
                         ("fill", c["fill"] > 0), ("valid", c["want_valid"]), ("count", c["want_count"]),
                         ("mode, n", c["mode"], c["n"])}
        assert {("n", n) for n in X.NS} | {("mode", m) for m in range(4)} | {("layout", l) for l in X.LAYOUTS} <= seen
        assert {("validity", v) for v in X.VALIDITY} | {("fill", f) for f in (False, True)} <= seen
        assert {(o, b) for o in ("valid", "count") for b in (False, True)} <= seen
        assert {("mode, n", m, n) for m in range(4) for n in X.NS} <= seen, (kind, C)


@pytest.mark.parametrize("si", range(len(X.SIZES)))
@pytest.mark.parametrize("ki", range(len(X.KINDS)))
def test_composite_kernels_equal_the_restatement(si, ki):
    (oh, ow), (kind, C) = X.SIZES[si], X.KINDS[ki]
    elem = X.DTYPES[kind]().itemsize
    for case in X.sweep(ki, si):
        n, mode, fill = case["n"], case["mode"], case["fill"]
        srcs, masks, rects, nodata = X.case_inputs(kind, C, oh, ow, case)
        what = f"window_composite_{kind} {oh}x{ow}x{C} {case}"
        want, want_valid, want_count = X.composite(srcs, masks, rects, nodata, C, oh, ow, mode, fill)
        if case["validity"] == "ladder" and oh * ow >= 33 * 130:            # no source dropped, none taken twice
            assert set(want_count.ravel().tolist()) == set(range(n + 1)), what
        dst = Out(want.nbytes, offset=elem * case["offset"])
        dval = Out(oh * ow, offset=1 + case["offset"]) if case["want_valid"] else None
        dcnt = Out(oh * ow, offset=3 - case["offset"]) if case["want_count"] else None
        lib.check(_composite(kind, srcs, masks, rects, nodata, C, dst.view, dval and dval.view, dcnt and dcnt.view, oh, ow,
                             mode, fill), what)
        _same(dst.host(what), want, what)
        if dval is not None:
            _same(dval.host(what), want_valid, what + ": valid")
        if dcnt is not None:
            _same(dcnt.host(what), want_count, what + ": count")


def test_every_mode_of_one_input_with_and_without_the_optional_outputs():
    """the four modes side by side on one staggered, randomly valid input, each with every choice of the two optional
    outputs: the image does not depend on which of them is asked for (first and last stop early only without a count)"""
    oh, ow, n, C = 33, 130, 9, 3
    for kind in ("u8", "u16"):
        case = dict(n=n, mode=0, layout="staggered", validity="random")
        srcs, masks, rects, nodata = X.case_inputs(kind, C, oh, ow, case)
        nodata[2] = int(srcs[2][3, 3, 0])
        srcs[2][3:9, 3:40] = nodata[2]                                       # validity and nodata on one source
        for mode in range(4):
            want, want_valid, want_count = X.composite(srcs, masks, rects, nodata, C, oh, ow, mode, 5)
            for with_valid in (False, True):
                for with_count in (False, True):
                    what = f"window_composite_{kind} mode {mode} valid {with_valid} count {with_count}"
                    dst, dval, dcnt = Out(want.nbytes), Out(oh * ow) if with_valid else None, Out(oh * ow) if with_count else None
                    lib.check(_composite(kind, srcs, masks, rects, nodata, C, dst.view, dval and dval.view,
                                         dcnt and dcnt.view, oh, ow, mode, 5), what)
                    _same(dst.host(what), want, what)
                    assert dval is None or np.array_equal(dval.host(what).reshape(oh, ow), want_valid), what
                    assert dcnt is None or np.array_equal(dcnt.host(what).reshape(oh, ow), want_count), what


def test_composite_calls_refuse_through_their_error_return_and_write_nothing():
    src = torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda")
    out, cnt = Out(8 * 8 * 3), Out(64)

    def call(rect=(0, 0, 8, 8), n=1, C=3, dst=None, mode=0, fill=0, nodata=-1):
        return lib.load().dsic_window_composite_u8(
            (ctypes.c_void_p * 1)(_p(src)), (ctypes.c_void_p * 1)(None), (ctypes.c_int * 4)(*rect), (ctypes.c_int * 1)(nodata), n, C,
            _p(out.view) if dst is None else dst, None, _p(cnt.view), 8, 8, mode, fill, _stream())

    for kw, word in (({"n": 0}, "n=0"), ({"C": 5}, "C=5"), ({"rect": (1, 0, 8, 8)}, "not inside"), ({"mode": 4}, "mode=4"),
                     ({"fill": 256}, "fill=256"), ({"nodata": 256}, "nodata=256"), ({"dst": _p(src)}, "overlap"),
                     ({"dst": _p(cnt.view)}, "outputs overlap")):
        assert call(**kw) == lib.DSIC_EINVAL and word.encode() in lib.load().dsic_last_error(), word
    torch.cuda.synchronize()
    assert (out.host("refused calls") == U8_FILL).all() and (cnt.host("refused calls") == U8_FILL).all() and not bool(src.any())
    assert call() == lib.DSIC_OK
    assert not out.host("a legal call").any() and (cnt.host("a legal call") == 1).all()


# ---- the stack ------------------------------------------------------------------------------------------------------
MODES = ("first", "last", "mean", "median")


def _extra(kind, seed):
    """one more 150 x 200 scene of another seed, compressed once per session; seed 22 with two overviews"""
    if ("extra", kind, seed) not in _CACHE:
        in_ch = 4 if kind == "u16" else 3
        x = S.make_patches(seed, 1, H0, W0, in_ch)[0].astype(np.float32)
        kw = {"overviews": 2} if seed == 22 else {}
        if kind == "u16":
            img = np.ascontiguousarray((x * 10000 + 0.5).astype(np.uint16).transpose(1, 2, 0))
            kw["scale"] = SCALE
        else:
            img = np.ascontiguousarray((x * 255 + 0.5).astype(np.uint8).transpose(1, 2, 0))
        _CACHE[("extra", kind, seed)] = codec.compress_image(_model(in_ch), torch.from_numpy(img).cuda(), **ARGS, **kw)
    return _CACHE[("extra", kind, seed)]


def _extra_reader(kind, seed):
    return codec.ImageReader(_model(4 if kind == "u16" else 3), _extra(kind, seed), batch=BATCH)


def _restated(stack, readers, window, level, mode, fill):
    """composite_ref over what the readers themselves return for the parts of the window"""
    srcs, masks, rects, nodata = [], [], [], []
    scenes = [(o, r.levels) for o, r in zip(stack.offsets, readers)]
    for s, part, rect in codec.stack_parts(level, scenes, window):
        img, valid = readers[s].read(*part, level=level, with_valid=True)
        srcs.append(_np(img))
        masks.append(_np(valid).astype(np.uint8))
        rects.append(rect)
        nodata.append(readers[s].index(level).get("nodata", -1))
    C = stack.shape[2]
    if not srcs:
        dtype = np.uint16 if stack.kind == codec.KIND_U16_HWC else np.uint8
        return np.full(window[2:] + (C,), fill, dtype=dtype), np.zeros(window[2:], np.uint8), np.zeros(window[2:], np.uint8), 0
    return X.composite(srcs, masks, rects, nodata, C, window[2], window[3], X.MODES[mode], fill) + (len(srcs),)


def _check_read(stack, plain, window, level, mode, fill=0):
    st = {}
    img, valid, count = stack.read(*window, level=level, reduce=mode, fill=fill, with_valid=True, with_count=True, stats=st)
    want, want_valid, want_count, parts = _restated(stack, plain, window, level, mode, fill)
    what = (window, level, mode)
    assert img.is_cuda and img.is_contiguous() and valid.dtype == torch.bool and count.dtype == torch.uint8
    assert _np(img).dtype == want.dtype and np.array_equal(_np(img), want), what
    assert np.array_equal(_np(valid), want_valid != 0) and np.array_equal(_np(count), want_count), what
    assert st["parts"] == parts, what
    alone = stack.read(*window, level=level, reduce=mode, fill=fill)
    assert np.array_equal(_np(alone), want), what
    return want, want_valid, want_count


def test_a_stack_of_one_reader_is_the_reader():
    for name in ("u8", "u8_nodata", "u16_valid"):
        with _reader(name) as r, _reader(name) as plain:
            stack = codec.SceneStack([r])
            assert stack.levels == r.levels and stack.shape == r.shape
            for level, window in [(0, (30, 50, 100, 120))] + ([(2, (3, 5, 30, 40))] if len(r.levels) == 3 else []):
                want, want_valid = plain.read(*window, level=level, with_valid=True)
                by_value = _np(want) == 7 if name == "u8_nodata" else None
                for mode in MODES:
                    img, valid = stack.read(*window, level=level, reduce=mode, fill=STREAMS[name][2].get("fill", 7),
                                            with_valid=True)
                    assert np.array_equal(_np(img), _np(want)), (name, level, mode)
                    if by_value is None:
                        assert np.array_equal(_np(valid), _np(want_valid)), (name, level, mode)
                        assert name != "u16_valid" or (not _np(valid).all() and _np(valid).any())
                    else:                                                    # a nodata stream's validity is by value
                        assert np.array_equal(_np(valid), ~by_value.all(axis=2)) and not _np(valid).all()


def test_a_uint16_mosaic_over_three_levels():
    offsets = [(0, 0), (40, 60), (100, 0)]
    with _reader("u16") as a, _reader("u16_valid") as b, _extra_reader("u16", 22) as c, _reader("u16") as pa, \
            _reader("u16_valid") as pb, _extra_reader("u16", 22) as pc:
        stack = codec.SceneStack([a, b, c], offsets)
        assert stack.levels == [(250, 260), (125, 130), (63, 65)] and stack.shape == (250, 260, 4)
        assert len(codec.SceneStack([a, b, c], [(0, 0), (40, 62), (100, 0)]).levels) == 2
        # inside one scene, across seams, through a hole (above the second scene, right of the first), the whole grid
        windows = {0: [(5, 7, 30, 40), (30, 50, 100, 120), (0, 190, 60, 70), (0, 0, 250, 260)],
                   2: [(1, 1, 8, 12), (5, 10, 40, 40), (0, 45, 20, 20), (0, 0, 63, 65)]}
        for level, wins in windows.items():
            for k, window in enumerate(wins):
                for mode in MODES:
                    want, want_valid, want_count = _check_read(stack, [pa, pb, pc], window, level, mode, fill=(0, 65535)[k % 2])
                if k == 0:
                    assert want_count.max() == 1
                if k == 2:
                    assert not want_valid.all() and want_valid.any()
                if k == 3:
                    assert want_count.max() == 3 and want_count.min() == 0
        assert np.array_equal(_np(stack.read(0, 210, 30, 40, fill=123)), np.full((30, 40, 4), 123, np.uint16))   # no scene
        st = {}
        img, valid, count = stack.read(0, 210, 30, 40, with_valid=True, with_count=True, stats=st)
        assert st["parts"] == 0 and st["decoded"] == 0 and not bool(valid.any()) and not bool(count.any())
        st = {}
        stack.read(30, 50, 100, 120, stats=st)
        assert st["parts"] == 3 and st["decoded"] == 0 and st["hits"] > 0 and {t[0] for t in st["tiles"]} == {0, 1, 2}   # cached


def test_a_uint8_temporal_stack():
    with _reader("u8") as a, _reader("u8_nodata") as b, _reader("u8_valid") as c, _extra_reader("u8", 22) as d, \
            _extra_reader("u8", 23) as e, _reader("u8") as pa, _reader("u8_nodata") as pb, _reader("u8_valid") as pc, \
            _extra_reader("u8", 22) as pd, _extra_reader("u8", 23) as pe:
        stack = codec.SceneStack([a, b, c, d, e])
        assert stack.levels == [(H0, W0)] and len(d.levels) == 3
        got = {}
        for mode in MODES:
            for window in ((0, 0, H0, W0), (20, 30, 70, 90)):
                got[mode, window[0]] = _check_read(stack, [pa, pb, pc, pd, pe], window, 0, mode, fill=9)
        median, _, count = got["median", 0]
        assert (median != got["mean", 0][0]).any() and (median != got["first", 0][0]).any()
        assert count.max() == 5 and count[0, 0] < 5 and count[-1, -1] == 5   # the wedge of the nodata and masked scenes
        assert (got["first", 0][0] != got["last", 0][0]).any()


def test_a_render_is_the_restated_display_of_the_composite():
    with _reader("u16") as a, _reader("u16_valid") as b, _extra_reader("u16", 22) as c:
        stack = codec.SceneStack([a, b, c], [(0, 0), (40, 60), (100, 0)])
        for k, (level, window) in enumerate(((0, (0, 150, 120, 110)), (2, (0, 0, 63, 65)), (0, (30, 50, 100, 120)))):
            for mode in ("median", "first"):
                bands, alpha, background = [(0, 1, 2), (3, 0, 0), (1,)][k], bool((k + 1) % 2), (0, 200)[k % 2]
                img, valid = stack.read(*window, level=level, reduce=mode, with_valid=True)
                got = stack.render(*window, level=level, reduce=mode, bands=bands, stretch=U16_PAIRS, alpha=alpha,
                                   background=background)
                want = R.display(_np(img), _np(valid), bands, U16_PAIRS, alpha, background)
                assert got.dtype == torch.uint8 and got.shape == want.shape and np.array_equal(_np(got), want), (level, window)
                if k < 2:
                    assert not _np(valid).all() and (_np(got)[~_np(valid)][:, :len(bands)] == background).all()
        with pytest.raises(ValueError, match="stretch"):
            stack.render(0, 0, 8, 8)
        with pytest.raises(ValueError, match="bands"):
            stack.render(0, 0, 8, 8, bands=(4,), stretch=U16_PAIRS)
    with _reader("u8") as a, _reader("u8_valid") as b:                        # uint8: (0, 255) by default, the bytes themselves
        stack = codec.SceneStack([b, a])
        img, valid = stack.read(0, 0, 60, 80, reduce="mean", with_valid=True)
        got = stack.render(0, 0, 60, 80, reduce="mean", alpha=True)
        assert np.array_equal(_np(got), R.display(_np(img), _np(valid), (0, 1, 2), [(0, 255)] * 3, True, 0))
        assert np.array_equal(_np(got)[..., :3], _np(img)) and (_np(got)[..., 3] == 255).all()


def test_the_stacks_refusals():
    with _reader("u8") as u8, _reader("u16") as u16, _reader("f32") as f32, _reader("u8_valid") as u8v, \
            _extra_reader("u8", 22) as one:
        for readers, kw, word in (([u8, u16], {}, "one kind"), ([u8, one, f32], {}, "float32"), ([], {}, "0 readers"),
                                  ([u8] * 17, {}, "17 readers"), ([u8, one], {"offsets": [(0, 0)]}, "offsets"),
                                  ([u8, one], {"offsets": [(0, 0), (0, -8)]}, "offsets"),
                                  ([u8, one], {"offsets": [(0, 0), (8, 8)], "shape": (150, 208)}, "outside the 150x208 grid")):
            with pytest.raises(ValueError, match=word):
                codec.SceneStack(readers, **kw)
        with _reader("u16_valid") as four, _extra_reader("u16", 22) as also_four:
            codec.SceneStack([four, also_four])
        with codec.ImageReader(_model(4), _four_band_u8(), batch=BATCH) as four_bands:
            with pytest.raises(ValueError, match="band count"):
                codec.SceneStack([u8, four_bands])
        stack = codec.SceneStack([u8v, one])
        assert len(stack.levels) == 3
        before = one.stats["decoded"]
        for args, kw, word in (((0, 0, H0 + 1, 8), {}, "outside"), ((0, 0, 0, 8), {}, "empty"), ((-1, 0, 8, 8), {}, "outside"),
                               ((0, 0, 39, 8), {"level": 2}, "outside the 38x50 level 2"), ((0, 0, 8, 8), {"level": 3}, "levels 0 .. 2"),
                               ((0, 0, 8, 8), {"level": -1}, "levels 0 .. 2"), ((0, 0, 8, 8), {"reduce": "mode"}, "reduce"),
                               ((0, 0, 8, 8), {"fill": 256}, "fill"), ((0, 0, 8, 8.5), {}, "integers")):
            with pytest.raises(ValueError, match=word):
                stack.read(*args, **kw)
        assert one.stats["decoded"] == before
        closed = _reader("u8")
        stack = codec.SceneStack([u8, closed])
        closed.close()
        with pytest.raises(ValueError, match="closed"):
            stack.read(0, 0, 8, 8)
        with pytest.raises(ValueError, match="closed"):
            codec.SceneStack([u8, closed])


def _four_band_u8():
    if ("extra", "u8", "four bands") not in _CACHE:
        x = S.make_patches(24, 1, H0, W0, 4)[0].astype(np.float32)
        img = np.ascontiguousarray((x * 255 + 0.5).astype(np.uint8).transpose(1, 2, 0))
        _CACHE[("extra", "u8", "four bands")] = codec.compress_image(_model(4), torch.from_numpy(img).cuda(), **ARGS)
    return _CACHE[("extra", "u8", "four bands")]


def test_the_tool_composites_two_stream_files(tmp_path):
    model = _model(4)
    sd = _CACHE[("model", 4)][1]
    torch.save({"model": {k: torch.from_numpy(v) for k, v in sd.items()}}, tmp_path / "ckpt.pt")
    (tmp_path / "a.dsic").write_bytes(_stream_of("u16_valid"))
    (tmp_path / "b.dsic").write_bytes(_extra("u16", 22))
    tool = os.path.join(ROOT, "tools", "dsic_image.py")
    cmd = [sys.executable, tool, "composite", str(tmp_path / "out.npy"), "--scene", str(tmp_path / "a.dsic"), "--scene",
           str(tmp_path / "b.dsic") + "@40,60", "--reduce", "median", "--level", "1", "--region", "10,20,70,90", "--fill", "77",
           "--count-out", str(tmp_path / "count.npy"), "--valid-out", str(tmp_path / "valid.npy"), "--weights",
           str(tmp_path / "ckpt.pt"), "--batch", str(BATCH)]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    with _reader("u16_valid") as a, _extra_reader("u16", 22) as b:
        stack = codec.SceneStack([a, b], [(0, 0), (40, 60)])
        img, valid, count = stack.read(10, 20, 70, 90, level=1, reduce="median", fill=77, with_valid=True, with_count=True)
    assert np.array_equal(np.load(tmp_path / "out.npy"), _np(img)) and img.shape == (70, 90, 4)
    assert np.array_equal(np.load(tmp_path / "count.npy"), _np(count)) and _np(count).max() == 2
    assert np.array_equal(np.load(tmp_path / "valid.npy"), _np(valid)) and not _np(valid).all()
    assert "median of 2 scene(s) on a 190x260 grid, 3 level(s)" in p.stdout and "of level 1" in p.stdout
    p = subprocess.run(cmd[:4] + ["--weights", str(tmp_path / "ckpt.pt")], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode != 0 and "--scene" in p.stderr
