"""Best-pixel composites on the GPU.  The pick exports alone, bit for bit against the NumPy restatement of
tests/best_pixel_ref.py, outputs between guards and inputs inside larger allocations at odd and 2-byte alignments as in
test_gpu_composite.py; then codec.SceneStack on that file's streams: ranked reads and the source plane against the
restatement of what the readers return, render_index against index_ref, the refusals, and the command-line tool."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import best_pixel_ref as BP
import best_pixel_stream_cases  # noqa: F401  (its recipes join the table that test_gpu_stream_order.py runs)
import composite_ref as X
import index_ref
from dsic_amd import codec, lib
from dsic_amd.ops import _p, _stream
from test_gpu_composite import _composite, _extra, _extra_reader
from test_gpu_render import _CACHE, BATCH, H0, U16_PAIRS, W0, _model, _np, _reader, _stream_of
from test_gpu_valid import U8_FILL, Out, _inside, _same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REDUCE = codec.stack_reduce                      # the feature under test: without it nothing in this file is held
NDVI = ("nd", 3, 0)


# ---- the kernels ----------------------------------------------------------------------------------------------------
def _pick(kind, srcs, masks, rects, nodata, ids, C, dst, dval, dcnt, dsrc, oh, ow, mode, index, fill):
    """test_gpu_composite._composite's placement: uint16 sources at addresses that are 2-byte but not 4-byte aligned,
    uint8 ones and the validity at odd addresses; the device copies live until the kernel has run"""
    n, elem = len(srcs), srcs[0].dtype.itemsize
    d_src = [_inside(s, elem * (1 + 2 * (i % 2))) for i, s in enumerate(srcs)]
    d_val = [None if m is None else _inside(m, 1 + 2 * (i % 3)) for i, m in enumerate(masks)]
    opt = lambda t: None if t is None else _p(t)
    status = getattr(lib.load(), "dsic_window_composite_pick_" + kind)(
        (ctypes.c_void_p * n)(*[_p(t) for t in d_src]), (ctypes.c_void_p * n)(*[opt(t) for t in d_val]),
        (ctypes.c_int * (4 * n))(*[v for r in rects for v in r]), (ctypes.c_int * n)(*nodata),
        None if ids is None else (ctypes.c_int * n)(*ids), n, C, _p(dst), opt(dval), opt(dcnt), opt(dsrc), oh, ow, mode,
        index_ref.KINDS[index[0]], index[1], index[-1], fill, _stream())
    torch.cuda.synchronize()
    return status


@pytest.mark.parametrize("si", range(len(BP.SIZES)))
@pytest.mark.parametrize("ki", range(len(BP.KINDS)))
def test_pick_kernels_equal_the_restatement(si, ki):
    (oh, ow), (kind, C) = BP.SIZES[si], BP.KINDS[ki]
    elem = X.DTYPES[kind]().itemsize
    for case in BP.sweep(ki, si):
        srcs, masks, rects, nodata, ids = BP.case_inputs(kind, C, oh, ow, case)
        what = f"window_composite_pick_{kind} {oh}x{ow}x{C} {case}"
        want, want_valid, want_count, want_source = BP.pick(srcs, masks, rects, nodata, ids, C, oh, ow, case["mode"],
                                                            case["index"], case["fill"])
        dst = Out(want.nbytes, offset=elem * case["offset"])
        dval = Out(oh * ow, offset=1 + case["offset"]) if case["want_valid"] else None
        dcnt = Out(oh * ow, offset=3 - case["offset"]) if case["want_count"] else None
        dsrc = Out(oh * ow, offset=2 + case["offset"]) if case["want_source"] else None
        lib.check(_pick(kind, srcs, masks, rects, nodata, ids, C, dst.view, dval and dval.view, dcnt and dcnt.view,
                        dsrc and dsrc.view, oh, ow, case["mode"], case["index"], case["fill"]), what)
        _same(dst.host(what), want, what)
        for out, plane, name in ((dval, want_valid, "valid"), (dcnt, want_count, "count"), (dsrc, want_source, "source")):
            if out is not None:
                _same(out.host(what), plane, what + ": " + name)


def _one_input(kind):
    """test_gpu_composite's: nine staggered, randomly valid sources, validity and nodata on one of them, and a block without a
    normalised difference"""
    oh, ow, n, C = 33, 130, 9, 3
    srcs, masks, rects, nodata = X.case_inputs(kind, C, oh, ow, dict(n=n, mode=0, layout="staggered", validity="random"))
    nodata[2] = int(srcs[2][3, 3, 0])
    srcs[2][3:9, 3:40] = nodata[2]
    srcs[4][10:20, 30:90, :2] = 0                                            # a normalised difference without a value
    return oh, ow, n, C, srcs, masks, rects, nodata


def test_every_mode_of_one_input_with_every_choice_of_the_optional_outputs():
    """the image does not depend on which of the three optional outputs are asked for, nor does any of them on the
    others"""
    for kind in ("u8", "u16"):
        oh, ow, n, C, srcs, masks, rects, nodata = _one_input(kind)
        for mode, index in ((BP.FIRST, ("band", 0)), (BP.LAST, ("band", 0)), (BP.MAX, ("nd", 1, 0)), (BP.MIN, ("difference", 0, 2))):
            wants = BP.pick(srcs, masks, rects, nodata, None, C, oh, ow, mode, index, 5)
            assert len(set(wants[3].ravel().tolist())) == n + 1             # every source wins somewhere, and none
            for choice in range(8):
                what = f"window_composite_pick_{kind} mode {mode} outputs {choice:03b}"
                outs = [Out(wants[0].nbytes)] + [Out(oh * ow) if choice >> b & 1 else None for b in range(3)]
                lib.check(_pick(kind, srcs, masks, rects, nodata, None, C, *[o and o.view for o in outs], oh, ow, mode, index, 5),
                          what)
                for out, want in zip(outs, wants):
                    if out is not None:
                        _same(out.host(what), want, what)


def test_first_and_last_without_ids_and_source_write_the_old_exports_bytes():
    for kind in ("u8", "u16"):
        oh, ow, n, C, srcs, masks, rects, nodata = _one_input(kind)
        nbytes = oh * ow * C * srcs[0].dtype.itemsize
        for mode in (BP.FIRST, BP.LAST):
            for with_count in (False, True):                                 # with a count the walk goes to the end
                what = f"{kind} mode {mode} count {with_count}"
                old = [Out(nbytes), Out(oh * ow), Out(oh * ow) if with_count else None]
                new = [Out(nbytes), Out(oh * ow), Out(oh * ow) if with_count else None]
                lib.check(_composite(kind, srcs, masks, rects, nodata, C, *[o and o.view for o in old], oh, ow, mode, 5), what)
                lib.check(_pick(kind, srcs, masks, rects, nodata, None, C, *[o and o.view for o in new], None, oh, ow, mode,
                                ("band", 0), 5), what)
                for o, m in zip(old, new):
                    if o is not None:
                        _same(m.host(what), o.host(what), what)


def test_pick_calls_refuse_through_their_error_return_and_write_nothing():
    src = torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda")
    out, cnt, sou = Out(8 * 8 * 3), Out(64), Out(64)

    def call(rect=(0, 0, 8, 8), n=1, C=3, dst=None, ds=None, mode=4, kind=2, a=1, b=0, fill=0, nodata=-1, ids=None):
        return lib.load().dsic_window_composite_pick_u8(
            (ctypes.c_void_p * 1)(_p(src)), (ctypes.c_void_p * 1)(None), (ctypes.c_int * 4)(*rect), (ctypes.c_int * 1)(nodata),
            None if ids is None else (ctypes.c_int * 1)(*ids), n, C, _p(out.view) if dst is None else dst, None, _p(cnt.view),
            _p(sou.view) if ds is None else ds, 8, 8, mode, kind, a, b, fill, _stream())

    for kw, word in (({"n": 0}, "n=0"), ({"C": 5}, "C=5"), ({"rect": (1, 0, 8, 8)}, "not inside"), ({"mode": 2}, "mode=2"),
                     ({"mode": 3}, "mode=3"), ({"mode": 6}, "mode=6"), ({"kind": 3}, "kind=3"), ({"a": 3}, "band 3"),
                     ({"b": -1}, "band -1"), ({"mode": 5, "kind": 0, "a": 4}, "band 4"), ({"ids": (255,)}, "id=255"),
                     ({"ids": (-1,)}, "id=-1"), ({"fill": 256}, "fill=256"), ({"nodata": 256}, "nodata=256"),
                     ({"dst": _p(src)}, "overlap"), ({"ds": _p(src)}, "overlap"), ({"ds": _p(cnt.view)}, "outputs overlap"),
                     ({"ds": _p(out.view)}, "outputs overlap")):
        assert call(**kw) == lib.DSIC_EINVAL and word.encode() in lib.load().dsic_last_error(), word
    torch.cuda.synchronize()
    for o in (out, cnt, sou):
        assert (o.host("refused calls") == U8_FILL).all()
    assert not bool(src.any())
    assert call(ids=(254,)) == lib.DSIC_OK                                   # all zeros: no normalised difference anywhere
    assert (out.host("a legal call") == 0).all() and (cnt.host("a legal call") == 0).all()
    assert (sou.host("a legal call") == 255).all()
    assert call(ids=(254,), kind=1) == lib.DSIC_OK
    assert (cnt.host("a legal call") == 1).all() and (sou.host("a legal call") == 254).all()
    assert call(mode=0, kind=9, a=-1, b=77) == lib.DSIC_OK                   # first and last do not look at the index
    assert (sou.host("a legal call") == 0).all()


# ---- the stack ------------------------------------------------------------------------------------------------------
def _restated(stack, readers, window, level, reduce, fill):
    """best_pixel_ref over what the readers themselves return for the parts of the window, scene numbers as ids"""
    srcs, masks, rects, nodata, ids = [], [], [], [], []
    scenes = [(o, r.levels) for o, r in zip(stack.offsets, readers)]
    for s, part, rect in codec.stack_parts(level, scenes, window):
        img, valid = readers[s].read(*part, level=level, with_valid=True)
        srcs.append(_np(img))
        masks.append(_np(valid).astype(np.uint8))
        rects.append(rect)
        nodata.append(readers[s].index(level).get("nodata", -1))
        ids.append(s)
    C, (h, w) = stack.shape[2], window[2:]
    if not srcs:
        dtype = np.uint16 if stack.kind == codec.KIND_U16_HWC else np.uint8
        return np.full((h, w, C), fill, dtype=dtype), np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8)
    mode, index = (BP.MODES[reduce], ("band", 0)) if isinstance(reduce, str) else (BP.MODES[reduce[0]], reduce[1])
    return BP.pick(srcs, masks, rects, nodata, ids, C, h, w, mode, index, fill)


def _check_read(stack, plain, window, level, reduce, fill=0):
    img, valid, count, source = stack.read(*window, level=level, reduce=reduce, fill=fill, with_valid=True, with_count=True,
                                           with_source=True)
    want, want_valid, want_count, want_source = _restated(stack, plain, window, level, reduce, fill)
    what = (window, level, reduce)
    assert img.is_cuda and img.is_contiguous() and valid.dtype == torch.bool and source.dtype == torch.uint8
    assert source.shape == (window[2], window[3]) and count.dtype == torch.uint8
    assert _np(img).dtype == want.dtype and np.array_equal(_np(img), want), what
    assert np.array_equal(_np(valid), want_valid != 0) and np.array_equal(_np(count), want_count), what
    assert np.array_equal(_np(source), want_source), what
    assert np.array_equal(_np(stack.read(*window, level=level, reduce=reduce, fill=fill)), want), what
    img2, source2 = stack.read(*window, level=level, reduce=reduce, fill=fill, with_source=True)
    assert np.array_equal(_np(img2), want) and np.array_equal(_np(source2), want_source), what
    return want, want_valid, want_count, want_source


def test_a_ranked_uint16_mosaic_over_three_levels():
    offsets = [(0, 0), (40, 60), (100, 0)]
    with _reader("u16") as a, _reader("u16_valid") as b, _extra_reader("u16", 22) as c, _reader("u16") as pa, \
            _reader("u16_valid") as pb, _extra_reader("u16", 22) as pc:
        stack = codec.SceneStack([a, b, c], offsets)
        # inside one scene, across seams, through a hole (above the second scene, right of the first), the whole grid
        windows = {0: [(5, 7, 30, 40), (30, 50, 100, 120), (0, 190, 60, 70), (0, 0, 250, 260)],
                   2: [(1, 1, 8, 12), (5, 10, 40, 40), (0, 45, 20, 20), (0, 0, 63, 65)]}
        for level, wins in windows.items():
            for k, window in enumerate(wins):
                for reduce in (("max", NDVI), ("min", ("band", 2)), ("max", ("difference", 1, 2)), "first", "last"):
                    _, want_valid, want_count, want_source = _check_read(stack, [pa, pb, pc], window, level, reduce,
                                                                         fill=(0, 65535)[k % 2])
                    if k == 0:
                        assert want_count.max() == 1 and {0} <= set(want_source.ravel().tolist()) <= {0, 255}
                    if k == 2:
                        assert not want_valid.all() and want_valid.any() and 255 in want_source
                    if k == 3:
                        assert want_count.max() == 3 and set(want_source.ravel().tolist()) == {0, 1, 2, 255}
        # a window that scene 0 does not meet: the plane holds scene numbers, not positions in the launch's list
        st = {}
        img, source = stack.read(160, 70, 60, 100, reduce=("max", NDVI), with_source=True, stats=st)
        assert st["parts"] == 2 and set(_np(source).ravel().tolist()) <= {1, 2, 255} and {1, 2} <= set(_np(source).ravel().tolist())
        _check_read(stack, [pa, pb, pc], (160, 70, 60, 100), 0, "last")
        # no scene: nothing is launched
        st = {}
        img, valid, source = stack.read(0, 210, 30, 40, reduce=("max", NDVI), fill=123, with_valid=True, with_source=True, stats=st)
        assert st["parts"] == 0 and st["decoded"] == 0 and (_np(img) == 123).all() and not bool(valid.any())
        assert source.dtype == torch.uint8 and (_np(source) == 255).all()
        # cached second reads decode nothing
        st = {}
        stack.read(30, 50, 100, 120, reduce=("max", NDVI), with_source=True, stats=st)
        assert st["parts"] == 3 and st["decoded"] == 0 and st["hits"] > 0 and {t[0] for t in st["tiles"]} == {0, 1, 2}


def test_a_ranked_uint8_temporal_stack():
    with _reader("u8") as a, _reader("u8_nodata") as b, _reader("u8_valid") as c, _extra_reader("u8", 22) as d, \
            _extra_reader("u8", 23) as e, _reader("u8") as pa, _reader("u8_nodata") as pb, _reader("u8_valid") as pc, \
            _extra_reader("u8", 22) as pd, _extra_reader("u8", 23) as pe:
        stack, plain = codec.SceneStack([a, b, c, d, e]), [pa, pb, pc, pd, pe]
        got = {}
        for reduce in (("max", ("nd", 0, 2)), ("min", ("nd", 0, 2)), ("max", ("band", 1)), ("min", ("difference", 2, 1)), "first"):
            for window in ((0, 0, H0, W0), (20, 30, 70, 90)):
                got[reduce, window[0]] = _check_read(stack, plain, window, 0, reduce, fill=9)
        best, _, count, source = got[("max", ("nd", 0, 2)), 0]
        assert (best != got["first", 0][0]).any() and (best != got[("min", ("nd", 0, 2)), 0][0]).any()
        assert (best != _np(stack.read(0, 0, H0, W0, reduce="median", fill=9))).any()
        assert count.max() == 5 and count[0, 0] < 5 and set(source.ravel().tolist()) >= {0, 1, 3, 4}
        # every pixel is, in all bands, the pixel of the scene its source plane names
        scenes = [_np(r.read(0, 0, H0, W0)) for r in plain]
        # scene 2 is scene 0 under a mask, and scene 0 is valid everywhere: where the two agree the tie goes to scene 0
        assert not (source == 2)[(scenes[0][..., [0, 2]] == scenes[2][..., [0, 2]]).all(axis=2)].any()
        for s, scene in enumerate(scenes):
            assert np.array_equal(best[source == s], scene[source == s]), s
        assert (best[source == 255] == 9).all()
        st = {}
        stack.read(0, 0, H0, W0, reduce=("max", ("nd", 0, 2)), stats=st)
        assert st["parts"] == 5 and st["decoded"] == 0 and st["hits"] > 0
        for kw, word in (({"reduce": "mean", "with_source": True}, "with_source"), ({"reduce": "median", "with_source": True}, "with_source"),
                         ({"reduce": "max"}, "'max', index"), ({"reduce": ("max", ("nd", 3, 0))}, "bands in 0 .. 2"),
                         ({"reduce": ("most", ("nd", 1, 0))}, "reduce"), ({"reduce": ("max", NDVI[:2])}, "reduce")):
            with pytest.raises(ValueError, match=word):
                stack.read(0, 0, 8, 8, **kw)


def test_a_render_index_is_the_restated_index_view_of_the_composite():
    with _reader("u16") as a, _reader("u16_valid") as b, _extra_reader("u16", 22) as c:
        stack = codec.SceneStack([a, b, c], [(0, 0), (40, 60), (100, 0)])
        for k, (level, window) in enumerate(((0, (0, 150, 120, 110)), (2, (0, 0, 63, 65)), (0, (30, 50, 100, 120)))):
            for reduce in (("max", NDVI), "median"):
                index, pair, cmap = [(NDVI, None, "ndvi"), (("difference", 1, 2), (-3000, 4000), "diverging"),
                                     (("band", 3), (200, 9000), "heat")][k]
                alpha, background = bool((k + 1) % 2), (0, 200)[k % 2]
                img, valid = stack.read(*window, level=level, reduce=reduce, with_valid=True)
                got = stack.render_index(*window, index, level=level, reduce=reduce, stretch=pair, colormap=cmap, alpha=alpha,
                                         background=background)
                want = index_ref.display_index(_np(img), _np(valid), index, pair or (-10000, 10000), codec.COLORMAPS[cmap],
                                               alpha, background)
                assert got.dtype == torch.uint8 and got.shape == want.shape and np.array_equal(_np(got), want), (level, window)
                if k < 2:
                    assert not _np(valid).all() and (_np(got)[~_np(valid)][:, :3] == background).all()
                also = stack.render(*window, level=level, reduce=reduce, bands=(3, 0, 1), stretch=U16_PAIRS)
                assert also.shape == (window[2], window[3], 3)               # render takes the ranked reduces as they come
        own = np.ascontiguousarray(codec.COLORMAPS["heat"][::-1])
        got = stack.render_index(30, 50, 100, 120, NDVI, reduce=("min", NDVI), colormap=own)
        img, valid = stack.read(30, 50, 100, 120, reduce=("min", NDVI), with_valid=True)
        assert np.array_equal(_np(got), index_ref.display_index(_np(img), _np(valid), NDVI, (-10000, 10000), own))
        for index, kw, word in ((("band", 0), {}, "stretch"), (("difference", 0, 1), {}, "stretch"), (("nd", 4, 0), {}, "bands in 0 .. 3"),
                                (NDVI, {"stretch": (-10001, 0)}, "stretch pair"), (NDVI, {"colormap": "rainbow"}, "colormap"),
                                (NDVI, {"background": 256}, "background"), (NDVI, {"reduce": "mode"}, "reduce"),
                                (NDVI, {"level": 3}, "levels 0 .. 2")):
            with pytest.raises(ValueError, match=word):
                stack.render_index(0, 0, 8, 8, index, **kw)
        with pytest.raises(ValueError, match="needs stretch=") as err:
            stack.render(0, 0, 8, 8)
        with pytest.raises(ValueError, match="needs stretch=") as err2:
            stack.render_index(0, 0, 8, 8, ("band", 0))
        assert str(err.value).partition(": ")[2] == str(err2.value).partition(": ")[2]
    with _reader("u8") as a, _reader("u8_valid") as b:                        # uint8: the index's full range by default
        stack = codec.SceneStack([b, a])
        for index in (("band", 1), ("difference", 0, 2), ("nd", 0, 2)):
            reduce = ("max", index)
            img, valid = stack.read(0, 0, 60, 80, reduce=reduce, with_valid=True)
            got = stack.render_index(0, 0, 60, 80, index, reduce=reduce, alpha=True)
            pair = index_ref.value_range(index[0], 255)
            assert np.array_equal(_np(got), index_ref.display_index(_np(img), _np(valid), index, pair, codec.COLORMAPS["grey"], True, 0))


def test_the_tool_writes_a_maximum_ndvi_composite_and_its_source_plane(tmp_path):
    _model(4)
    sd = _CACHE[("model", 4)][1]
    torch.save({"model": {k: torch.from_numpy(v) for k, v in sd.items()}}, tmp_path / "ckpt.pt")
    (tmp_path / "a.dsic").write_bytes(_stream_of("u16_valid"))
    (tmp_path / "b.dsic").write_bytes(_extra("u16", 22))
    tool = os.path.join(ROOT, "tools", "dsic_image.py")
    cmd = [sys.executable, tool, "composite", str(tmp_path / "out.npy"), "--scene", str(tmp_path / "a.dsic"), "--scene",
           str(tmp_path / "b.dsic") + "@40,60", "--weights", str(tmp_path / "ckpt.pt"), "--batch", str(BATCH), "--level", "1",
           "--region", "10,20,70,90", "--fill", "77", "--reduce", "max"]
    more = ["--index", "nd:3,0", "--source-out", str(tmp_path / "source.npy"), "--count-out", str(tmp_path / "count.npy")]
    p = subprocess.run(cmd + more, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    with _reader("u16_valid") as a, _extra_reader("u16", 22) as b:
        stack = codec.SceneStack([a, b], [(0, 0), (40, 60)])
        img, count, source = stack.read(10, 20, 70, 90, level=1, reduce=("max", NDVI), fill=77, with_count=True, with_source=True)
    assert np.array_equal(np.load(tmp_path / "out.npy"), _np(img)) and img.shape == (70, 90, 4)
    assert np.array_equal(np.load(tmp_path / "count.npy"), _np(count)) and _np(count).max() == 2
    assert np.array_equal(np.load(tmp_path / "source.npy"), _np(source)) and set(_np(source).ravel().tolist()) == {0, 1, 255}
    assert "max of nd:3,0 of 2 scene(s) on a 190x260 grid, 3 level(s)" in p.stdout and "of level 1" in p.stdout
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 2 and "--index" in p.stderr
