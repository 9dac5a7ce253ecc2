"""Warped scene stacks on the GPU.  The exports dsic_window_warp_composite_u8 / _u16 alone, bit for bit against the
NumPy restatement of tests/warp_stack_ref.py (the chain of warp_ref and composite_ref / best_pixel_ref), outputs between
guards and inputs inside larger allocations at odd and 2-byte alignments; the fused call against the chain of the older
exports run on the GPU; then codec.SceneStack.read_warped, render_warped and render_index_warped on the coded streams of
test_gpu_composite.py / test_gpu_render.py, and the command-line tool."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import best_pixel_ref as BP
import composite_ref as X
import index_ref
import render_ref
import warp_stack_ref as WS
import warp_stack_stream_cases  # noqa: F401  (its recipes join the table of tests/stream_cases.py)
from dsic_amd import codec, lib
from dsic_amd.ops import _p, _stream
from test_gpu_best_pixel import _pick
from test_gpu_composite import _composite, _extra, _extra_reader
from test_gpu_render import _CACHE, ARGS, BATCH, H0, SCALE, U16_PAIRS, W0, _model, _np, _reader, _stream_of
from test_gpu_valid import U8_FILL, Out, _inside, _same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READ_WARPED = codec.SceneStack.read_warped       # the feature under test: without it nothing in this file is held
NDVI = ("nd", 3, 0)
BIG = WS.SIZES[-1]


# ---- the kernels ----------------------------------------------------------------------------------------------------
def _table(srcs, ids):
    """the sources on the device: uint16 windows at addresses that are 2-byte but not 4-byte aligned, uint8 ones and the
    validity at odd addresses -> (the host table, the device copies, to be kept until the kernel has run)"""
    elem = srcs[0]["src"].dtype.itemsize
    table, keep = (lib.WarpSource * len(srcs))(), []
    for i, s in enumerate(srcs):
        d_src = _inside(s["src"], elem * (1 + 2 * (i % 2)))
        d_val = None if s["val"] is None else _inside(s["val"], 1 + 2 * (i % 3))
        keep += [d_src, d_val]
        table[i] = lib.WarpSource(_p(d_src), None if d_val is None else _p(d_val), s["sh"], s["sw"], s["sy0"], s["sx0"], s["shift"],
                                  s["LH"], s["LW"], s["H"], s["W"], s["nodata"], i if ids is None else ids[i], 0,
                                  (ctypes.c_int64 * 6)(*s["m"]))
    return table, keep


def _fused(kind, srcs, ids, C, outs, size, sample, reduce, index, fill):
    table, keep = _table(srcs, ids)
    status = getattr(lib.load(), "dsic_window_warp_composite_" + kind)(
        table, len(srcs), C, *[None if o is None else _p(o.view) for o in outs], size[0], size[1], sample, reduce,
        index_ref.KINDS[index[0]], index[1], index[-1], fill, _stream())
    torch.cuda.synchronize()
    return status


def _check_outs(outs, wants, what):
    for out, want, name in zip(outs, wants, ("image", "valid", "count", "source")):
        if out is not None:
            _same(out.host(what), want, what + ": " + name)


@pytest.mark.parametrize("si", range(len(WS.SIZES)))
@pytest.mark.parametrize("ki", range(len(WS.KINDS)))
def test_kernels_equal_the_restatement(si, ki):
    size, (kind, C) = WS.SIZES[si], WS.KINDS[ki]
    oh, ow = size
    elem = X.DTYPES[kind]().itemsize
    for case in WS.sweep(ki, si):
        srcs = WS.case_sources(kind, C, size, case)
        wants = WS.restate(kind, C, size, case, srcs)
        what = f"window_warp_composite_{kind} {oh}x{ow}x{C} {case}"
        outs = [Out(wants[0].nbytes, offset=elem * case["offset"]),
                Out(oh * ow, offset=1 + case["offset"]) if case["want_valid"] else None,
                Out(oh * ow, offset=3 - case["offset"]) if case["want_count"] else None,
                Out(oh * ow, offset=2 + case["offset"]) if case["want_source"] else None]
        lib.check(_fused(kind, srcs, WS.case_ids(case["n"]) if case["ids"] else None, C, outs, size, case["sample"],
                         case["reduce"], case["index"], case["fill"]), what)
        _check_outs(outs, wants, what)


def _one_input(kind, sample):
    C = 3 if kind == "u8" else 4
    return C, WS.sources(kind, C, BIG, 16, sample)


def test_the_largest_list_lets_every_source_win_and_leaves_a_hole():
    """a condition on the inputs, held by the restatement alone: on 33 x 130 with 16 sources every source that meets the
    output wins somewhere under first and under max, and some pixel has no candidate"""
    for kind in ("u8", "u16"):
        for sample in range(3):
            C, srcs = _one_input(kind, sample)
            meets = {i for i, s in enumerate(srcs) if s["meets"]}
            assert len(meets) == 15 and 2 not in meets
            for reduce in (WS.FIRST, WS.MAX):
                source = WS.warp_composite(srcs, C, BIG, sample, reduce, ("nd", 0, C - 1), 0, None)[3]
                assert set(source.ravel().tolist()) == meets | {255}, (kind, sample, reduce)


@pytest.mark.parametrize("kind", ["u8", "u16"])
def test_the_fused_call_equals_the_chain_of_the_older_exports(kind):
    """n launches of dsic_window_warp_* and one of dsic_window_composite(_pick)_*, all on the GPU, against the one launch:
    image and planes, every reduce under every sample mode"""
    oh, ow = BIG
    L = lib.load()
    for sample in range(3):
        C, srcs = _one_input(kind, sample)
        elem = srcs[0]["src"].dtype.itemsize
        table, keep = _table(srcs, None)
        imgs = [torch.empty((oh, ow, C), dtype=torch.uint8 if kind == "u8" else torch.uint16, device="cuda") for _ in srcs]
        vals = [torch.empty((oh, ow), dtype=torch.uint8, device="cuda") for _ in srcs]
        for i, s in enumerate(srcs):
            lib.check(getattr(L, "dsic_window_warp_" + kind)(
                table[i].src, table[i].src_valid, s["sh"], s["sw"], s["sy0"], s["sx0"], C, s["shift"], s["LH"], s["LW"], s["H"],
                s["W"], (ctypes.c_int64 * 6)(*s["m"]), _p(imgs[i]), _p(vals[i]), oh, ow, sample, s["nodata"], (i * 37) % 250,
                _stream()), "window_warp")
        torch.cuda.synchronize()
        h_imgs, h_vals = [_np(t) for t in imgs], [_np(t) for t in vals]
        rects, nodata = [(0, 0, oh, ow)] * len(srcs), [s["nodata"] for s in srcs]
        for reduce in range(6):
            what = f"{kind} sample {sample} reduce {reduce}"
            index = ("nd", 0, C - 1)
            ranked_or_source = reduce not in (WS.MEAN, WS.MEDIAN)
            chain = [Out(oh * ow * C * elem), Out(oh * ow), Out(oh * ow), Out(oh * ow) if ranked_or_source else None]
            if ranked_or_source:
                lib.check(_pick(kind, h_imgs, h_vals, rects, nodata, None, C, *[o.view for o in chain], oh, ow, reduce, index, 5),
                          what)
            else:
                lib.check(_composite(kind, h_imgs, h_vals, rects, nodata, C, *[o.view for o in chain[:3]], oh, ow, reduce, 5), what)
            fused = [Out(oh * ow * C * elem), Out(oh * ow), Out(oh * ow), Out(oh * ow) if ranked_or_source else None]
            lib.check(_fused(kind, srcs, None, C, fused, BIG, sample, reduce, index, 5), what)
            for f, c, name in zip(fused, chain, ("image", "valid", "count", "source")):
                if f is not None:
                    _same(f.host(what), c.host(what), what + ": " + name)


def test_every_reduce_of_one_input_with_every_choice_of_the_optional_outputs():
    """the image does not depend on which of the three optional outputs are asked for, nor does any of them on the
    others"""
    oh, ow = BIG
    for kind in ("u8", "u16"):
        C, srcs = _one_input(kind, 0)
        for reduce, index in ((WS.FIRST, ("band", 0)), (WS.LAST, ("band", 0)), (WS.MEAN, ("band", 0)), (WS.MEDIAN, ("band", 0)),
                              (WS.MAX, ("nd", 1, 0)), (WS.MIN, ("difference", 0, 2))):
            wants = WS.warp_composite(srcs, C, BIG, 0, reduce, index, 5, None)
            for choice in range(8):
                if wants[3] is None and choice & 4:
                    continue                                                 # mean, median: no source plane (refused)
                what = f"window_warp_composite_{kind} reduce {reduce} outputs {choice:03b}"
                outs = [Out(wants[0].nbytes)] + [Out(oh * ow) if choice >> b & 1 else None for b in range(3)]
                lib.check(_fused(kind, srcs, None, C, outs, BIG, 0, reduce, index, 5), what)
                _check_outs(outs, wants, what)


def test_calls_refuse_through_their_error_return_and_write_nothing():
    src = torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda")
    out, cnt, sou = Out(8 * 8 * 3), Out(64), Out(64)
    ident = (65536, 0, 0, 0, 65536, 0)

    def call(n=1, C=3, dst=None, ds=None, sample=1, reduce=4, kind=2, a=1, b=0, fill=0, nodata=-1, id=0, m=ident, sh=8, shift=0):
        table = (lib.WarpSource * 1)(lib.WarpSource(_p(src), None, sh, 8, 0, 0, shift, 8, 8, 8, 8, nodata, id, 0,
                                                    (ctypes.c_int64 * 6)(*m)))
        return lib.load().dsic_window_warp_composite_u8(table, n, C, _p(out.view) if dst is None else dst, None, _p(cnt.view),
                                                        _p(sou.view) if ds is None else ds, 8, 8, sample, reduce, kind, a, b,
                                                        fill, _stream())

    for kw, word in (({"n": 0}, "n=0"), ({"C": 5}, "C=5"), ({"C": 2}, "C=2"), ({"sample": 3}, "mode=3"), ({"reduce": 6}, "mode=6"),
                     ({"kind": 3}, "kind=3"), ({"a": 3}, "band 3"), ({"b": -1}, "band -1"), ({"id": 255}, "id=255"),
                     ({"fill": 256}, "fill=256"), ({"nodata": 256}, "nodata=256"), ({"reduce": 2}, "dst_source"),
                     ({"sh": 9}, "source window"), ({"shift": 1}, "level 1"), ({"m": (1 << 27, 0, 0, 0, 65536, 0)}, "matrix entry 0"),
                     ({"sh": 4}, "taps cover"), ({"dst": _p(src)}, "overlap"), ({"ds": _p(src)}, "overlap"),
                     ({"ds": _p(cnt.view)}, "outputs overlap")):
        assert call(**kw) == lib.DSIC_EINVAL and word.encode() in lib.load().dsic_last_error(), word
    torch.cuda.synchronize()
    for o in (out, cnt, sou):
        assert (o.host("refused calls") == U8_FILL).all()
    assert call(id=254) == lib.DSIC_OK                                       # all zeros: no normalised difference anywhere
    torch.cuda.synchronize()
    assert (out.host("a legal call") == 0).all() and (cnt.host("a legal call") == 0).all()
    assert (sou.host("a legal call") == 255).all()
    assert call(id=254, kind=1) == lib.DSIC_OK
    torch.cuda.synchronize()
    assert (cnt.host("a legal call") == 1).all() and (sou.host("a legal call") == 254).all()
    assert call(reduce=0, kind=9, a=-1, b=77) == lib.DSIC_OK                 # the unranked reduces do not look at the index
    torch.cuda.synchronize()
    assert (sou.host("a legal call") == 0).all()


# ---- the stack ------------------------------------------------------------------------------------------------------
def _restated(scenes, plain, view_q16, size, resampling, reduce, fill):
    """the definition over what each reader's own read_warped returns for the composed matrix: the chain's first step
    through the single-scene export, its second through composite_ref / best_pixel_ref with full rects"""
    oh, ow = size
    imgs, vals, nodata, ids = [], [], [], []
    for s, m, level, lw in codec.stack_warp_parts(scenes, view_q16, size, resampling):
        matrix = [[v / 65536 for v in m[:3]], [v / 65536 for v in m[3:]]]    # exact: affine_q16 gives m back
        assert codec.affine_q16(matrix) == m
        st = {}
        img, valid = plain[s].read_warped(matrix, size, resampling=resampling, with_valid=True, stats=st)
        assert st["level"] == level and st["level_window"] == lw
        imgs.append(_np(img))
        vals.append(_np(valid).astype(np.uint8))
        nodata.append(plain[s].index(level).get("nodata", -1))
        ids.append(s)
    C = plain[0].shape[2]
    if not imgs:
        return (np.full((oh, ow, C), fill, dtype=_np(plain[0].read(0, 0, 1, 1)).dtype), np.zeros(size, np.uint8),
                np.zeros(size, np.uint8), np.full(size, 255, np.uint8))
    rects = [(0, 0, oh, ow)] * len(imgs)
    if reduce in ("mean", "median"):
        return tuple(X.composite(imgs, vals, rects, nodata, C, oh, ow, X.MODES[reduce], fill)) + (None,)
    mode, index = (BP.MODES[reduce], ("band", 0)) if isinstance(reduce, str) else (BP.MODES[reduce[0]], reduce[1])
    return BP.pick(imgs, vals, rects, nodata, ids, C, oh, ow, mode, index, fill)


def _check_read(stack, plain, matrix, size, resampling, reduce, fill=0):
    with_source = reduce not in ("mean", "median")
    got = stack.read_warped(matrix, size, reduce=reduce, resampling=resampling, fill=fill, with_valid=True, with_count=True,
                            with_source=with_source)
    want = _restated(stack._warp_scenes, plain, codec.affine_q16(matrix), size, resampling, reduce, fill)
    what = (matrix, size, resampling, reduce)
    assert got[0].is_cuda and got[0].is_contiguous() and got[1].dtype == torch.bool and got[2].dtype == torch.uint8
    assert _np(got[0]).dtype == want[0].dtype and np.array_equal(_np(got[0]), want[0]), what
    assert np.array_equal(_np(got[1]), want[1] != 0) and np.array_equal(_np(got[2]), want[2]), what
    if with_source:
        assert got[3].dtype == torch.uint8 and np.array_equal(_np(got[3]), want[3]), what
    assert np.array_equal(_np(stack.read_warped(matrix, size, reduce=reduce, resampling=resampling, fill=fill)), want[0]), what
    return want


REDUCES = ["first", "last", "mean", "median", ("max", NDVI), ("min", ("band", 2))]


def test_a_turned_uint16_mosaic_is_the_restated_chain_over_the_readers_own_warped_reads():
    offsets = [(0, 0), (40, 60), (100, 0)]
    with _reader("u16") as a, _reader("u16_valid") as b, _extra_reader("u16", 22) as c, _reader("u16") as pa, \
            _reader("u16_valid") as pb, _extra_reader("u16", 22) as pc:
        stack, plain = codec.SceneStack([a, b, c], offsets), [pa, pb, pc]
        H, W = stack.levels[0]
        views = [(codec.rotation_affine(H / 2, W / 2, 30, 3.0, 60, 90), (60, 90)),          # turned, across all three and holes
                 (codec.rotation_affine(120, 100, -75, 0.4, 33, 50), (33, 50)),              # magnified
                 (codec.rotation_affine(H / 2, W / 2, 10, 4.2, 41, 37), (41, 37)),           # minified: level 2 of each scene
                 ([[1.7, 0.2, -20.25], [-0.1, 2.3, 15.5]], (70, 64))]                        # sheared, overhanging the grid
        for k, (matrix, size) in enumerate(views):
            for r, reduce in enumerate(REDUCES):
                resampling = ("bilinear", "cubic", "nearest")[(k + r) % 3]
                want = _check_read(stack, plain, matrix, size, resampling, reduce, fill=(0, 65535)[k % 2])
                if k == 0 and reduce == "first":
                    assert set(want[3].ravel().tolist()) == {0, 1, 2, 255} and want[2].max() >= 2
        st = {}
        stack.read_warped(views[2][0], views[2][1], stats=st)
        assert st["parts"] == 3 and st["scenes"] == [0, 1, 2] and st["levels"] == [2, 2, 2] and len(st["matrix_q16"]) == 3
        assert st["view_q16"] == codec.affine_q16(views[2][0]) and len(st["level_windows"]) == 3
        assert st["matrix_q16"][1] == codec.compose_q16(stack._warp_scenes[1][0], st["view_q16"])
        assert st["decoded"] == 0 and st["hits"] > 0 and {t[0] for t in st["tiles"]} == {0, 1, 2}
        # a view beside every scene: nothing is decoded, nothing is launched
        st = {}
        img, valid, count, source = stack.read_warped([[1, 0, 0], [0, 1, 400]], (20, 30), fill=123, with_valid=True,
                                                      with_count=True, with_source=True, stats=st)
        assert st["parts"] == 0 and st["decoded"] == 0 and st["tiles"] == [] and (_np(img) == 123).all()
        assert not bool(valid.any()) and not bool(count.any()) and (_np(source) == 255).all() and img.dtype == torch.uint16
        # a view that the first scene does not meet: the plane holds scene numbers
        st = {}
        _, source = stack.read_warped(codec.window_affine(160, 70, 60, 100, 30, 50), (30, 50), with_source=True, stats=st)
        assert st["scenes"] == [1, 2] and {1, 2} <= set(_np(source).ravel().tolist()) <= {1, 2, 255}
        for kw, word in (({"reduce": "mean", "with_source": True}, "with_source"), ({"reduce": "mode"}, "reduce"),
                         ({"resampling": "average"}, "resampling"), ({"fill": 65536}, "fill"), ({"size": (0, 4)}, "size"),
                         ({"size": (1 << 16, 1 << 15)}, "2\\^31"), ({"matrix": [[2000, 0, 0], [0, 1, 0]]}, "coefficient"),
                         ({"matrix": [[1, 0], [0, 1]]}, "matrix")):
            args = dict({"matrix": [[1, 0, 0], [0, 1, 0]], "size": (8, 8)}, **kw)
            with pytest.raises(ValueError, match=word):
                stack.read_warped(**args)


def test_the_identity_view_is_read_under_every_resampling():
    with _reader("u8") as a, _reader("u8_nodata") as b, _reader("u8_valid") as c, _extra_reader("u8", 22) as d:
        stack = codec.SceneStack([a, b, c, d], [(0, 0), (10, 30), (0, 0), (60, 20)])
        for window in ((0, 0) + tuple(stack.levels[0]), (20, 30, 70, 90), (100, 5, 33, 17)):
            y0, x0, h, w = window
            for reduce in REDUCES[:4] + [("max", ("nd", 0, 2)), ("min", ("band", 1))]:
                with_source = reduce not in ("mean", "median")
                want = stack.read(*window, reduce=reduce, fill=9, with_valid=True, with_count=True, with_source=with_source)
                for resampling in ("nearest", "bilinear", "cubic"):      # cubic: test_warp_stack_cpu.py recorded that it holds
                    got = stack.read_warped(codec.window_affine(y0, x0, h, w, h, w), (h, w), reduce=reduce, resampling=resampling,
                                            fill=9, with_valid=True, with_count=True, with_source=with_source)
                    for g, x in zip(got, want):
                        assert g.dtype == x.dtype and np.array_equal(_np(g), _np(x)), (window, reduce, resampling)


def _halved_stream():
    """level 1 of the u16 scene as a stream of its own"""
    if ("warp stack", "halved") not in _CACHE:
        with _reader("u16") as r:
            half = r.read(0, 0, *r.levels[1], level=1)
        _CACHE[("warp stack", "halved")] = codec.compress_image(_model(4), half, **ARGS, scale=SCALE)
    return _CACHE[("warp stack", "halved")]


def test_a_scene_and_its_halved_copy_placed_at_half_scale():
    half = lambda: codec.ImageReader(_model(4), _halved_stream(), batch=BATCH)
    placements = [[[0.5, 0, 0], [0, 0.5, 0]], [[1, 0, 0], [0, 1, 0]]]
    with half() as a, _reader("u16_valid") as b, half() as pa, _reader("u16_valid") as pb:
        stack = codec.SceneStack([a, b], shape=(H0, W0), placements=placements)
        assert stack.levels == [(H0, W0)] and stack.shape == (H0, W0, 4) and stack.offsets is None
        assert stack.placements == [codec.affine_q16(m) for m in placements]
        for k, (matrix, size) in enumerate(((codec.window_affine(0, 0, H0, W0, 75, 100), (75, 100)),
                                            (codec.rotation_affine(70, 90, 45, 0.7, 48, 52), (48, 52)))):
            for r, reduce in enumerate(REDUCES):
                want = _check_read(stack, [pa, pb], matrix, size, ("bilinear", "nearest", "cubic")[(k + r) % 3], reduce)
            assert want[2].max() == 2
        st = {}
        stack.read_warped(codec.window_affine(0, 0, H0, W0, 75, 100), (75, 100), stats=st)
        assert st["levels"] == [0, 1]                                        # the halved copy is sampled at its own level 0
        for call in (lambda: stack.read(0, 0, 8, 8), lambda: stack.render(0, 0, 8, 8, stretch=U16_PAIRS),
                     lambda: stack.render_index(0, 0, 8, 8, NDVI)):
            with pytest.raises(ValueError, match="read_warped"):
                call()


def test_the_rendered_views_are_the_restated_display_of_read_warped():
    with _reader("u16") as a, _reader("u16_valid") as b, _extra_reader("u16", 22) as c:
        stack = codec.SceneStack([a, b, c], [(0, 0), (40, 60), (100, 0)])
        matrix, size = codec.rotation_affine(125, 130, 30, 3.0, 60, 90), (60, 90)
        for k, reduce in enumerate(("first", "median", ("max", NDVI))):
            resampling = ("bilinear", "cubic", "nearest")[k]
            alpha, background = bool(k % 2), (0, 200, 17)[k]
            img, valid = stack.read_warped(matrix, size, reduce=reduce, resampling=resampling, with_valid=True)
            assert not _np(valid).all() and _np(valid).any()
            got = stack.render_warped(matrix, size, reduce=reduce, bands=(3, 0, 1), stretch=U16_PAIRS, alpha=alpha,
                                      background=background, resampling=resampling)
            want = render_ref.display(_np(img), _np(valid), (3, 0, 1), U16_PAIRS, alpha, background)
            assert got.dtype == torch.uint8 and got.shape == want.shape and np.array_equal(_np(got), want), reduce
            index, pair, cmap = [(NDVI, None, "ndvi"), (("difference", 1, 2), (-3000, 4000), "diverging"),
                                 (("band", 3), (200, 9000), "heat")][k]
            got = stack.render_index_warped(matrix, size, index, reduce=reduce, stretch=pair, colormap=cmap, alpha=alpha,
                                            background=background, resampling=resampling)
            want = index_ref.display_index(_np(img), _np(valid), index, pair or (-10000, 10000), codec.COLORMAPS[cmap], alpha,
                                           background)
            assert got.dtype == torch.uint8 and got.shape == want.shape and np.array_equal(_np(got), want), reduce
        with pytest.raises(ValueError, match="needs stretch=") as err:
            stack.render_warped(matrix, size)
        with pytest.raises(ValueError, match="needs stretch=") as err2:
            stack.render(0, 0, 8, 8)
        assert str(err.value).partition(": ")[2] == str(err2.value).partition(": ")[2]
        for kw, word in (({"index": ("nd", 4, 0)}, "bands in 0 .. 3"), ({"stretch": (-10001, 0)}, "stretch pair"),
                         ({"colormap": "rainbow"}, "colormap"), ({"background": 256}, "background"), ({"reduce": "mode"}, "reduce"),
                         ({"resampling": "average"}, "resampling")):
            with pytest.raises(ValueError, match=word):
                stack.render_index_warped(matrix, size, **dict({"index": NDVI}, **kw))


def test_a_pan_decodes_only_the_tiles_that_enter():
    with _reader("u16") as a, _extra_reader("u16", 22) as b:
        stack = codec.SceneStack([a, b], [(0, 0), (40, 60)])
        first, second, third = {}, {}, {}
        view = lambda dy, dx: codec.rotation_affine(50 + dy, 60 + dx, 20, 1.0, 40, 50)
        stack.read_warped(view(0, 0), (40, 50), reduce="median", stats=first)
        stack.read_warped(view(45, 70), (40, 50), reduce="median", stats=second)
        stack.read_warped(view(45, 70), (40, 50), reduce="median", stats=third)
        assert first["decoded"] == len(set(first["tiles"])) > 0 and first["hits"] == 0
        entered = set(second["tiles"]) - set(first["tiles"])
        assert 0 < len(entered) < len(set(second["tiles"])) and second["decoded"] == len(entered)
        assert second["hits"] == len(set(second["tiles"])) - len(entered)
        assert third["decoded"] == 0 and third["tiles"] == second["tiles"]


def test_the_tool_writes_a_turned_composite_and_a_placed_one(tmp_path):
    _model(4)
    sd = _CACHE[("model", 4)][1]
    torch.save({"model": {k: torch.from_numpy(v) for k, v in sd.items()}}, tmp_path / "ckpt.pt")
    (tmp_path / "a.dsic").write_bytes(_stream_of("u16_valid"))
    (tmp_path / "b.dsic").write_bytes(_extra("u16", 22))
    (tmp_path / "h.dsic").write_bytes(_halved_stream())
    tool = os.path.join(ROOT, "tools", "dsic_image.py")
    head = [sys.executable, tool, "composite", str(tmp_path / "out.npy"), "--weights", str(tmp_path / "ckpt.pt"), "--batch",
            str(BATCH), "--fill", "77"]
    cmd = head + ["--scene", str(tmp_path / "a.dsic"), "--scene", str(tmp_path / "b.dsic") + "@40,60", "--reduce", "max",
                  "--index", "nd:3,0", "--rotate", "30", "--center", "95,130", "--scale", "1.5", "--size", "60,90",
                  "--resampling", "cubic", "--source-out", str(tmp_path / "source.npy"), "--count-out", str(tmp_path / "count.npy")]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    with _reader("u16_valid") as a, _extra_reader("u16", 22) as b:
        stack = codec.SceneStack([a, b], [(0, 0), (40, 60)])
        img, count, source = stack.read_warped(codec.rotation_affine(95, 130, 30, 1.5, 60, 90), (60, 90), reduce=("max", NDVI),
                                               resampling="cubic", fill=77, with_count=True, with_source=True)
    assert np.array_equal(np.load(tmp_path / "out.npy"), _np(img)) and img.shape == (60, 90, 4)
    assert np.array_equal(np.load(tmp_path / "count.npy"), _np(count)) and _np(count).max() == 2
    assert np.array_equal(np.load(tmp_path / "source.npy"), _np(source)) and set(_np(source).ravel().tolist()) == {0, 1, 255}
    assert "warped view 60x90" in p.stdout and "cubic" in p.stdout
    cmd = head + ["--scene", str(tmp_path / "h.dsic") + "@0.5,0,0,0,0.5,0", "--scene", str(tmp_path / "a.dsic"), "--reduce", "mean",
                  "--affine", "2,0,0,0,2,0", "--size", "75,100"]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    with codec.ImageReader(_model(4), _halved_stream(), batch=BATCH) as a, _reader("u16_valid") as b:
        stack = codec.SceneStack([a, b], shape=(75, 100), placements=[[[0.5, 0, 0], [0, 0.5, 0]], [[1, 0, 0], [0, 1, 0]]])
        img = stack.read_warped([[2, 0, 0], [0, 2, 0]], (75, 100), reduce="mean", fill=77)
    assert np.array_equal(np.load(tmp_path / "out.npy"), _np(img))
    p = subprocess.run(head + ["--scene", str(tmp_path / "a.dsic"), "--rotate", "30"], cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 2 and "--size" in p.stderr
