"""The index views without a GPU: the restatement of tests/index_ref.py against exact rationals (the normalised
difference is 10000 (A - B) / (A + B) rounded half up, for every pair of bytes and a grid of 16-bit pairs) and against
its own properties (the 32-bit bounds, the ends of difference and band, the stretch of u, the colour maps);
codec.colormap_from_anchors and codec.COLORMAPS against it; the six entry points' declarations and refusals (which need
the library, not a device); the reader's and the tool's argument errors."""
import ctypes
import importlib.util
import os
import re
import types
from fractions import Fraction

import numpy as np
import pytest

import index_ref as X
import index_stream_cases as ISC
import render_ref as R
import stream_cases as SC
from dsic_amd import codec, lib, view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"dsic_window_index_render_u8": 26, "dsic_window_index_render_u16": 26, "dsic_window_warp_index_render_u8": 27,
       "dsic_window_warp_index_render_u16": 27, "dsic_index_histogram_u8": 11, "dsic_index_histogram_u16": 11}
BAND, DIFFERENCE, ND = 0, 1, 2


def _half_up(f):
    """a Fraction rounded half up, as an int"""
    return (2 * f.numerator + f.denominator) // (2 * f.denominator)


# ---- the arithmetic -------------------------------------------------------------------------------------------------
def _nd_exact(pairs):
    return [None if A + B == 0 else _half_up(Fraction(10000 * (A - B), A + B)) for A, B in pairs]


def test_nd_is_the_exact_quotient_rounded_half_up_for_every_pair_of_bytes():
    A, B = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    img = np.stack([A, B], axis=-1).astype(np.uint8)
    u, defined = X.index_value(img, "nd", 0, 1)
    assert u.dtype == np.int64 and defined.dtype == bool
    assert not defined[0, 0] and defined.sum() == 65535 and u[0, 0] == 0
    want = _nd_exact([(a, b) for a in range(256) for b in range(256)])
    got = [None if not d else int(v) - 10000 for v, d in zip(u.ravel(), defined.ravel())]
    assert got == want
    assert u.min() == 0 and u.max() == 20000
    assert (u[defined & (A == B)] == 10000).all() and (u[1:, 0] == 20000).all() and (u[0, 1:] == 0).all()
    assert np.array_equal(X.index_value(img, "nd", 1, 0)[1], defined)


def test_nd_on_the_16_bit_grid_and_random_pairs():
    grid = [0, 1, 2, 255, 256, 32767, 32768, 65534, 65535]
    rng = np.random.default_rng(7)
    pairs = [(a, b) for a in grid for b in grid] + [tuple(int(v) for v in p) for p in rng.integers(0, 65536, size=(10000, 2))]
    img = np.array(pairs, dtype=np.uint16)[None]
    u, defined = X.index_value(img, "nd", 0, 1)
    want = _nd_exact(pairs)
    got = [None if not d else int(v) - 10000 for v, d in zip(u[0], defined[0])]
    assert got == want and defined[0].sum() == len(pairs) - 1
    assert u.min() >= 0 and u.max() <= 20000
    # the half: (A - B) / (A + B) = 1 / 20000 exactly is 0.5 in units of 1 / 10000 and goes up
    assert int(X.index_value(np.array([[[20001, 19999]]], dtype=np.uint16), "nd", 0, 1)[0][0, 0]) - 10000 == 1
    assert int(X.index_value(np.array([[[19999, 20001]]], dtype=np.uint16), "nd", 0, 1)[0][0, 0]) - 10000 == 0     # -0.5 -> 0


def test_the_32_bit_bounds_hold_at_their_extreme_arguments():
    assert 40000 * 65535 + 131070 < 2 ** 32                                 # nd's numerator at A = B = 65535
    assert 40000 * 65535 + 65535 < 2 ** 32                                  # and at A = 65535, B = 0
    assert 510 * 131070 + 131070 < 2 ** 32                                  # the stretch of a uint16 difference's whole range
    assert 2 * 131070 < 2 ** 32 and 2 * 131070 > 0
    top = np.array([[[65535, 65535], [65535, 0], [0, 65535]]], dtype=np.uint16)
    u, defined = X.index_value(top, "nd", 0, 1)
    assert u[0].tolist() == [10000, 20000, 0] and defined.all()
    as32 = (np.uint64(40000) * top[..., 0].astype(np.uint64) + top.astype(np.uint64).sum(axis=-1))
    assert (as32 < 2 ** 32).all()


def test_difference_and_band_at_their_ends():
    for dtype, top in ((np.uint8, 255), (np.uint16, 65535)):
        img = np.array([[[0, top, 5], [top, 0, 5], [7, 7, 5], [0, 0, 5], [top, top, 5]]], dtype=dtype)
        u, defined = X.index_value(img, "difference", 0, 1)
        assert u[0].tolist() == [0, 2 * top, top, top, top] and defined.all()
        assert X.value_range("difference", top) == (-top, top) and X.value_range("band", top) == (0, top)
        assert X.value_range("nd", top) == (-10000, 10000)
        u, defined = X.index_value(img, "band", 1, 1)
        assert u[0].tolist() == [top, 0, 7, 0, top] and defined.all()
        u, _ = X.index_value(img, "difference", 2, 2)                       # a == b: zero everywhere
        assert (u == top).all()
        assert view.index_range("difference", top) == (-top, top) and view.index_range("nd", top) == (-10000, 10000)
        assert view.index_range("band", top) == (0, top)


@pytest.mark.parametrize("lo,hi", [(0, 20000), (5000, 15000), (9999, 10001), (0, 131070), (65535, 65536), (0, 510),
                                   (100000, 131070), (300, 300)])
def test_the_stretch_of_u_is_monotone_from_0_at_lo_to_255_at_hi(lo, hi):
    u = np.arange(0, 131071, dtype=np.int64)
    k = X.stretch(u, lo, hi)
    assert k.dtype == np.uint8 and (np.diff(k.astype(np.int64)) >= 0).all()
    assert k[lo] == 0 and (k[:lo + 1] == 0).all()
    if lo == hi:
        assert not k.any()
        return
    assert k[hi] == 255 and (k[hi:] == 255).all()
    R_ = hi - lo
    for d in sorted({0, 1, R_ // 2, R_ // 2 + 1, R_ - 1, R_, R_ // 3}):
        assert int(k[lo + d]) == _half_up(Fraction(255 * d, R_)), (lo, hi, d)
    if hi <= 65535:
        assert np.array_equal(k[:65536], R.stretch(u[:65536], lo, hi))


def test_display_index_marks_invalid_and_undefined_pixels():
    res = np.array([[[10, 10, 0], [0, 0, 9], [30, 10, 0]], [[0, 40, 0], [5, 0, 1], [1, 1, 1]]], dtype=np.uint8)
    ok = np.array([[1, 1, 0], [1, 1, 1]], dtype=bool)
    cmap = np.random.default_rng(1).integers(0, 256, size=(256, 3)).astype(np.uint8)
    out = X.display_index(res, ok, ("nd", 0, 1), (-10000, 10000), cmap, alpha=True, background=200)
    assert out.shape == (2, 3, 4) and out.dtype == np.uint8
    assert out[0, 1].tolist() == [200, 200, 200, 0]                          # A + B = 0
    assert out[0, 2].tolist() == [200, 200, 200, 0]                          # invalid
    assert out[0, 0].tolist() == cmap[128].tolist() + [255]                  # v = 0 -> u = 10000 -> k = 127.5 -> 128
    assert out[1, 0].tolist() == cmap[0].tolist() + [255] and out[1, 1].tolist() == cmap[255].tolist() + [255]
    plain = X.display_index(res, None, ("band", 1), (0, 255), codec.COLORMAPS["grey"])
    assert plain.shape == (2, 3, 3) and np.array_equal(plain, np.repeat(res[:, :, 1:2], 3, axis=2))
    assert np.array_equal(plain, R.display(res, None, (1, 1, 1), [(0, 255)] * 3))


def test_the_index_histogram_counts_defined_pixels_that_count():
    img = np.array([[[3, 1], [0, 0]], [[7, 7], [1, 3]]], dtype=np.uint8)
    h = X.histogram(img, None, None, ("nd", 0, 1))
    assert h.shape == (20001,) and h.dtype == np.int64 and h.sum() == 3 and h[15000] == 1 and h[10000] == 1 and h[5000] == 1
    assert X.histogram(img, None, 7, ("nd", 0, 1)).sum() == 2
    assert X.histogram(img, np.array([[0, 1], [1, 1]]), None, ("nd", 0, 1)).sum() == 2
    d = X.histogram(img, None, None, ("difference", 0, 1))
    assert d.shape == (511,) and d.sum() == 4 and d[255] == 2 and d[257] == 1 and d[253] == 1
    assert X.histogram(img.astype(np.uint16), None, None, ("difference", 1, 0)).shape == (131071,)
    assert np.array_equal(X.histogram(img, None, 7, ("band", 1)), R.histogram(img, None, 7)[1])
    assert X.index_stretch(d, ("difference", 0, 1), 255, (0, 100)) == (-2, 2)
    assert X.index_stretch(np.zeros(511, dtype=np.int64), ("difference", 0, 1), 255) == (-255, -255)


# ---- colour maps ----------------------------------------------------------------------------------------------------
def test_colormap_from_anchors_passes_through_its_anchors_and_is_monotone_between_them():
    anchors = [(0, (10, 200, 0)), (1, (11, 190, 0)), (100, (250, 20, 0)), (254, (250, 20, 255)), (255, (0, 0, 0))]
    cmap = codec.colormap_from_anchors(anchors)
    assert cmap.dtype == np.uint8 and cmap.shape == (256, 3) and np.array_equal(cmap, X.colormap_from_anchors(anchors))
    for p, c in anchors:
        assert tuple(cmap[p]) == c
    for (p0, c0), (p1, c1) in zip(anchors, anchors[1:]):
        seg = cmap[p0:p1 + 1].astype(np.int64)
        for ch in range(3):
            step = np.diff(seg[:, ch])
            assert (step >= 0).all() if c1[ch] >= c0[ch] else (step <= 0).all()
            for i in range(p0, p1 + 1):                                      # the line, rounded half up, as a fraction
                assert int(cmap[i, ch]) == _half_up(Fraction(c0[ch] * (p1 - i) + c1[ch] * (i - p0), p1 - p0))
    assert codec.colormap_from_anchors is view.colormap_from_anchors


def test_the_named_colormaps():
    assert set(codec.COLORMAPS) == {"grey", "ndvi", "diverging", "heat"}
    for name, cmap in codec.COLORMAPS.items():
        assert cmap.dtype == np.uint8 and cmap.shape == (256, 3), name
    grey = codec.COLORMAPS["grey"]
    assert all(tuple(grey[k]) == (k, k, k) for k in range(256))
    assert tuple(codec.COLORMAPS["diverging"][128]) == (255, 255, 255)
    d = codec.COLORMAPS["diverging"].astype(int)
    assert d[0, 2] > d[0, 0] and d[255, 0] > d[255, 2]                       # blue end, red end
    h = codec.COLORMAPS["heat"].astype(int)
    assert tuple(h[0]) == (0, 0, 0) and tuple(h[255]) == (255, 255, 255) and (np.diff(h.sum(axis=1)) >= 0).all()
    n = codec.COLORMAPS["ndvi"].astype(int)
    assert n[0, 0] > n[0, 1] > n[0, 2] and n[255, 1] > n[255, 0] and n[255, 1] > n[255, 2]   # brown ... dark green
    assert n[128].min() >= 180                                               # pale in the middle


def test_colormap_from_anchors_refuses():
    good = [(0, (0, 0, 0)), (255, (255, 255, 255))]
    for bad in ([(1, (0, 0, 0)), (255, (1, 1, 1))], [(0, (0, 0, 0)), (254, (1, 1, 1))], [(0, (0, 0, 0))], [],
                [(0, (0, 0, 0)), (9, (1, 1, 1)), (9, (2, 2, 2)), (255, (3, 3, 3))],
                [(0, (0, 0, 0)), (20, (1, 1, 1)), (10, (2, 2, 2)), (255, (3, 3, 3))], [(0, (0, 0)), (255, (1, 1, 1))],
                [(0, (0, 0, 256)), (255, (1, 1, 1))], [(0, (0, -1, 0)), (255, (1, 1, 1))], [(0, (0.5, 0, 0)), (255, (1, 1, 1))],
                [(0.0, (0, 0, 0)), (255, (1, 1, 1))], 7, [7, 8], None):
        with pytest.raises(ValueError, match="colormap_from_anchors"):
            codec.colormap_from_anchors(bad)
    assert np.array_equal(codec.colormap_from_anchors(good), codec.COLORMAPS["grey"])


# ---- the exports ----------------------------------------------------------------------------------------------------
def test_the_new_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "dsic_hip.h")).read()
    for name, nargs in NEW.items():
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert decl, name
        assert len(decl.group(1).split(",")) == nargs
        res, args = lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs and getattr(lib.load(), name) is not None
    for word in ("DSIC_INDEX_BAND 0", "DSIC_INDEX_DIFFERENCE 1", "DSIC_INDEX_ND 2", "(40000 A + s) / (2 s)", "A - B + top",
                 "40000 * 65535 + 131070 < 2^32", "510 * 131070 + 131070 < 2^32"):
        assert word in header, word
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for word in ("(40000·A + s) / (2·s)", "A − B + top", "−10000 … 10000"):
        assert word in design, word
    assert view.INDEX_KINDS == {"band": BAND, "difference": DIFFERENCE, "nd": ND}


def test_the_six_exports_have_stream_recipes_in_the_table():
    """tests/index_stream_cases.py registers them in tests/stream_cases.py's table on import: test_stream_cases_cpu.py
    and test_gpu_stream_order.py, collected after this file, then hold them as they hold every other export"""
    L = lib.load()
    assert len(ISC.NAMES) == len(set(ISC.NAMES)) == 12 and set(ISC.NAMES) <= set(SC.names())
    assert {e for n in ISC.NAMES for e in SC.build(n, L).exports} == set(NEW)
    assert all(SC.family(n) == "views" for n in ISC.NAMES)
    for n in ISC.NAMES:
        c = SC.build(n, L)
        assert c.judged() and c.inputs("A").keys() == c.inputs("B").keys()


def test_the_index_render_calls_check_their_arguments_without_a_gpu():
    L = lib.load()
    E, err = lib.DSIC_EINVAL, L.dsic_last_error
    a, b, m, cm = 1 << 20, 1 << 24, 1 << 22, 1 << 26           # non-null, aligned, far apart: every call is refused
    ok = dict(src=a, val=None, sh=8, sw=8, sy0=0, sx0=0, C=3, shift=0, y0=0, x0=0, h=8, w=8, kind=ND, ba=0, bb=1, lo=-10000,
              hi=10000, cmap=cm, dst=b, oh=4, ow=4, mode=0, nodata=-1, alpha=0, background=0)
    eye = (ctypes.c_int64 * 6)(65536, 0, 0, 0, 65536, 0)

    def call(export, name, **kw):
        p = dict(ok, **kw)
        tail = (p["kind"], p["ba"], p["bb"], p["lo"], p["hi"], p["cmap"], p["dst"], p["oh"], p["ow"], p["mode"], p["nodata"],
                p["alpha"], p["background"], None)
        head = (p["src"], p["val"], p["sh"], p["sw"], p["sy0"], p["sx0"], p["C"], p["shift"])
        if export == "window_index_render_":
            return getattr(L, "dsic_" + export + name)(*head, p["y0"], p["x0"], p["h"], p["w"], *tail)
        return getattr(L, "dsic_" + export + name)(*head, p["sh"], p["sw"], p["sh"], p["sw"], eye, *tail)

    for name, top in (("u8", 255), ("u16", 65535)):
        for export in ("window_index_render_", "window_warp_index_render_"):
            assert call(export, name, src=None) == E and b"null" in err()
            assert err().decode().partition(": ")[0] == export + name
            assert call(export, name, dst=None) == E and b"null" in err()
            assert call(export, name, cmap=None) == E and b"null" in err()
            for kind in (-1, 3):
                assert call(export, name, kind=kind) == E and f"kind={kind}".encode() in err()
            for C in (0, 5):
                assert call(export, name, C=C) == E and f"C={C}".encode() in err()
            assert call(export, name, ba=3) == E and b"band 3" in err()
            assert call(export, name, bb=-1) == E and b"band -1" in err()
            assert call(export, name, C=1, bb=1) == E and b"band 1" in err()
            # b is ignored for a band: the next fault is reported
            assert call(export, name, C=1, kind=BAND, bb=9, lo=0, hi=top + 1) == E and b"stretch pair" in err()
            assert call(export, name, alpha=2) == E and b"alpha=2" in err()
            assert call(export, name, alpha=-1) == E and b"alpha" in err()
            assert call(export, name, background=256) == E and b"background=256" in err()
            assert call(export, name, background=-1) == E and b"background" in err()
            for kind, lo, hi in ((ND, -10001, 0), (ND, 0, 10001), (ND, 5, 4), (DIFFERENCE, -top - 1, 0), (DIFFERENCE, 0, top + 1),
                                 (DIFFERENCE, 1, 0), (BAND, -1, 5), (BAND, 0, top + 1), (BAND, 9, 8)):
                assert call(export, name, kind=kind, lo=lo, hi=hi) == E and f"stretch pair ({lo}, {hi})".encode() in err()
            assert call(export, name, nodata=top + 1) == E and f"nodata={top + 1}".encode() in err()
            assert call(export, name, nodata=-2) == E and b"nodata" in err()
            assert call(export, name, shift=16) == E and b"shift=16" in err()
            assert call(export, name, mode=3) == E and b"mode=3" in err()
            assert call(export, name, oh=0) == E and b"output" in err()
            assert call(export, name, dst=a + 16) == E and b"overlap" in err()
            assert call(export, name, val=m, dst=m + 32) == E and b"overlap" in err()      # the validity window is 64 bytes
            assert call(export, name, cmap=b + 40) == E and b"cmap and dst overlap" in err()   # dst is 4 * 4 * 3 = 48 bytes
            assert call(export, name, cmap=b - 767) == E and b"cmap and dst overlap" in err()
            assert call(export, name, cmap=b + 48, alpha=1) == E and b"cmap and dst overlap" in err()   # with alpha: 64
        assert call("window_index_render_", name, h=9) == E and b"outside the source window" in err()
        assert call("window_index_render_", name, mode=2) == E and b"mode=2" in err()
    assert call("window_index_render_", "u16", src=a + 1) == E and b"2-byte aligned" in err()


def test_the_index_histogram_calls_check_their_arguments_without_a_gpu():
    L = lib.load()
    E, err = lib.DSIC_EINVAL, L.dsic_last_error
    a, b, m = 1 << 20, 1 << 24, 1 << 22
    for name, top, elem in (("u8", 255, 1), ("u16", 65535, 2)):
        fn = getattr(L, "dsic_index_histogram_" + name)
        assert fn(None, None, 4, 4, 3, -1, ND, 0, 1, b, None) == E and b"null" in err()
        assert fn(a, None, 4, 4, 3, -1, ND, 0, 1, None, None) == E and b"null" in err()
        for C in (0, 5):
            assert fn(a, None, 4, 4, C, -1, ND, 0, 0, b, None) == E and f"C={C}".encode() in err()
        assert fn(a, None, 0, 4, 3, -1, ND, 0, 1, b, None) == E and b"image" in err()
        assert fn(a, None, 65536, 65536, 1, -1, ND, 0, 0, 1 << 44, None) == E and b"2^32" in err()
        assert fn(a, None, 4, 4, 3, top + 1, ND, 0, 1, b, None) == E and f"nodata={top + 1}".encode() in err()
        for kind in (BAND, -1, 3):                                           # a band is the band histogram's
            assert fn(a, None, 4, 4, 3, -1, kind, 0, 1, b, None) == E and f"kind={kind}".encode() in err()
        assert fn(a, None, 4, 4, 3, -1, ND, 3, 1, b, None) == E and b"band 3" in err()
        assert fn(a, None, 4, 4, 3, -1, DIFFERENCE, 0, -1, b, None) == E and b"band -1" in err()
        assert fn(a, None, 4, 4, 3, -1, ND, 0, 1, b + 2, None) == E and b"aligned" in err()
        assert fn(a, None, 4, 4, 3, -1, ND, 0, 1, a + 16 * 3 * elem - 4, None) == E and b"overlap" in err()
        assert fn(a, None, 4, 4, 3, -1, ND, 0, 1, a - 4 * 20001 + 4, None) == E and b"overlap" in err()
        assert fn(a, None, 4, 4, 3, -1, DIFFERENCE, 0, 1, a - 4 * (2 * top + 1) + 4, None) == E and b"overlap" in err()
        assert fn(a, m, 4, 4, 3, -1, ND, 0, 1, m + 12, None) == E and b"overlap" in err()
    assert L.dsic_index_histogram_u16(a + 1, None, 4, 4, 3, -1, ND, 0, 1, b, None) == E and b"aligned" in err()


# ---- the reader's and the tool's argument errors ----------------------------------------------------------------------
def _reader(C, kind, **extra):
    """A reader over nothing, one level open: every refusal below comes before the first read of a tile"""
    r = object.__new__(codec.ImageReader)
    r._closed, r._dir, r._source = False, None, types.SimpleNamespace(bytes_read=0)
    r._open = {0: (None, dict({"C": C, "kind": kind, "H": 64, "W": 64, "version": 1}, **extra), 0)}
    return r


def test_the_index_views_refuse_before_any_launch():
    u8, u16 = _reader(3, codec.KIND_U8_HWC), _reader(4, codec.KIND_U16_HWC, scale=[(0, 65535)] * 4, version=6)
    win = (0, 0, 8, 8)
    eye = [[1, 0, 0], [0, 1, 0]]
    for r, C, top in ((u8, 3, 255), (u16, 4, 65535)):
        calls = [lambda **kw: r.render_index(*win, **kw), lambda **kw: r.render_index_warped(eye, (8, 8), **kw),
                 lambda **kw: r.render_many([dict({"window": win}, **kw)])]
        for call in calls:
            for index in (("nd", 0), ("nd", 0, 1, 2), ("band", 0, 1), ("ndvi", 0, 1), ("nd", 0, C), ("nd", -1, 0), ("band", C),
                          ("nd", 0.5, 1), (), 7, "nd", (0, 1, 2)):
                with pytest.raises(ValueError, match="index="):
                    call(index=index, stretch=(0, 1))
            for index, stretch in ((("nd", 0, 1), (-10001, 0)), (("nd", 0, 1), (0, 10001)), (("nd", 0, 1), (5, 4)),
                                   (("difference", 0, 1), (-top - 1, 0)), (("difference", 0, 1), (0, top + 1)),
                                   (("band", 0), (-1, 4)), (("band", 0), (0, top + 1)), (("nd", 0, 1), (0, 1, 2)),
                                   (("nd", 0, 1), (0.5, 3)), (("nd", 0, 1), 7), (("nd", 0, 1), [(0, 1)] * C)):
                with pytest.raises(ValueError, match="stretch"):
                    call(index=index, stretch=stretch)
            for colormap in ("viridis", np.zeros((256, 4), np.uint8), np.zeros((255, 3), np.uint8), np.zeros((256, 3), np.int32),
                             7, None, [[0, 0, 0]] * 256):
                with pytest.raises(ValueError, match="colormap"):
                    call(index=("nd", 0, 1), stretch=(0, 1), colormap=colormap)
        for call in calls[:2]:
            for background in (-1, 256, 0.5, None):
                with pytest.raises(ValueError, match="background"):
                    call(index=("nd", 0, 1), stretch=(0, 1), background=background)
        with pytest.raises(ValueError, match="resampling"):
            r.render_index(*win, ("nd", 0, 1), resampling="cubic")
        with pytest.raises(ValueError, match="resampling"):
            r.render_index_warped(eye, (8, 8), ("nd", 0, 1), resampling="average")
        with pytest.raises(ValueError, match="size"):
            r.render_index(*win, ("nd", 0, 1), size=(0, 4))
        for index in (("nd", 0), ("band", C), 7):
            with pytest.raises(ValueError, match="index="):
                r.index_histogram(index, level=0)
            with pytest.raises(ValueError, match="index="):
                r.index_stretch(index, level=0)
        with pytest.raises(ValueError, match="percent"):
            r.index_stretch(("nd", 0, 1), (98, 2), level=0)
    nodata = _reader(3, codec.KIND_U8_HWC, nodata=7, version=5)
    with pytest.raises(ValueError, match="valid="):
        nodata.render_index(*win, ("nd", 0, 1), alpha=True)
    with pytest.raises(ValueError, match="valid="):
        nodata.render_index_warped(eye, (8, 8), ("nd", 0, 1), alpha=True)
    with pytest.raises(ValueError, match="valid="):
        nodata.render_many([{"window": win, "index": ("nd", 0, 1)}], alpha=True)
    assert {"render_index", "render_index_warped", "index_histogram", "index_stretch"} <= set(dir(codec.ImageReader))


def _tool():
    spec = importlib.util.spec_from_file_location("_dsic_image_tool", os.path.join(ROOT, "tools", "dsic_image.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_the_tools_argument_errors(capsys):
    tool = _tool()
    base = ["render", "a.dsic", "b.npy", "--weights", "w.pt"]
    for extra, word in ((["--index", "nd"], "--index"), (["--index", "nd:0"], "--index"), (["--index", "band:0,1"], "--index"),
                        (["--index", "ndvi:0,1"], "--index"), (["--index", "nd:a,b"], "--index"),
                        (["--index", "nd:0,1", "--bands", "0"], "--index"), (["--index", "nd:0,1", "--stretch", "0,9"], "--index"),
                        (["--index", "nd:0,1", "--colormap", "viridis"], "--colormap"),
                        (["--index", "nd:0,1", "--index-stretch", "5"], "--index-stretch"),
                        (["--index", "nd:0,1", "--index-stretch", "a,b"], "--index-stretch"),
                        (["--index", "nd:0,1", "--index-stretch", "0,9", "--percent", "2,98"], "exclude"),
                        (["--colormap", "ndvi"], "go with --index"), (["--index-stretch", "0,9"], "go with --index")):
        with pytest.raises(SystemExit) as e:
            tool.main(base + extra)
        assert e.value.code == 2 and word in capsys.readouterr().err, extra
    for extra in (["--index", "nd:0,1"], ["--colormap", "ndvi"], ["--index-stretch", "0,9"]):
        with pytest.raises(SystemExit) as e:                               # render's options are render's alone
            tool.main(["decompress", "a.dsic", "b.npy", "--weights", "w.pt"] + extra)
        assert e.value.code == 2 and "go with render" in capsys.readouterr().err
