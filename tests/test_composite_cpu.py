"""Scene stacks without a GPU: the restatement of tests/composite_ref.py anchored (the median against np.median and the
floor + half-up rule, the mean against exact rationals, first and last on hand-made cases, the ladder's counts), the two
exports' declarations and refusals (which need the library, not a device), the planning functions codec.stack_levels and
codec.stack_parts, and the sweep of test_gpu_composite.py."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import composite_ref as X
import composite_stream_cases as CSC
import stream_cases as SC
from dsic_amd import codec, lib, view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"dsic_window_composite_u8": 14, "dsic_window_composite_u16": 14}
STACK = codec.SceneStack                         # the feature under test: without it nothing in this file is held


def _stack(values, dtype=np.uint8):
    """n sources of one pixel and one band, all covering a 1 x 1 output"""
    return [np.array([[[v]]], dtype=dtype) for v in values]


def _one(values, valid, mode, dtype=np.uint8, fill=99):
    n = len(values)
    masks = [np.array([[v]], dtype=np.uint8) for v in valid]
    dst, ok, k = X.composite(_stack(values, dtype), masks, [(0, 0, 1, 1)] * n, [-1] * n, 1, 1, 1, mode, fill)
    return int(dst[0, 0, 0]), int(ok[0, 0]), int(k[0, 0])


# ---- the restatement ------------------------------------------------------------------------------------------------
def test_the_median_is_numpys_for_odd_counts_and_floor_plus_half_up_for_even_ones():
    rng = np.random.default_rng(3)
    for dtype, top in ((np.uint8, 255), (np.uint16, 65535)):
        for n in range(1, 17):
            for _ in range(40):
                values = rng.integers(0, top + 1, size=n)
                if rng.random() < 0.3:
                    values[: n // 2] = top                                   # ties, at the top value
                valid = rng.random(n) < 0.7
                got, ok, k = _one(values, valid, X.MEDIAN, dtype)
                kept = np.sort(values[valid].astype(np.int64))
                assert k == len(kept) and ok == (k > 0)
                if k == 0:
                    assert got == 99
                elif k % 2:
                    assert got == int(np.median(kept)) == kept[(k - 1) // 2]
                else:
                    a, b = int(kept[k // 2 - 1]), int(kept[k // 2])
                    assert got == (a + b + 1) >> 1 == int(np.floor(np.median(kept) + 0.5))
    assert _one([1, 2], [1, 1], X.MEDIAN)[0] == 2 and _one([0, 255, 7, 9], [1, 1, 1, 1], X.MEDIAN)[0] == 8
    assert _one([65535, 65535], [1, 1], X.MEDIAN, np.uint16)[0] == 65535


def test_the_bands_of_a_median_are_independent():
    srcs = [np.array([[[1, 9]]], np.uint8), np.array([[[5, 2]]], np.uint8), np.array([[[3, 4]]], np.uint8)]
    dst, _, _ = X.composite(srcs, [None] * 3, [(0, 0, 1, 1)] * 3, [-1] * 3, 2, 1, 1, X.MEDIAN, 0)
    assert dst[0, 0].tolist() == [3, 4]                                      # from the third source and the third source
    srcs[2][0, 0] = (3, 200)
    assert X.composite(srcs, [None] * 3, [(0, 0, 1, 1)] * 3, [-1] * 3, 2, 1, 1, X.MEDIAN, 0)[0][0, 0].tolist() == [3, 9]


def test_the_mean_is_the_exact_quotient_rounded_half_up():
    assert 2 * 16 * 65535 + 16 < 2 ** 32
    rng = np.random.default_rng(4)
    for dtype, top in ((np.uint8, 255), (np.uint16, 65535)):
        for n in list(range(1, 17)) * 10:
            values = rng.integers(0, top + 1, size=n)
            valid = rng.random(n) < 0.8
            got, ok, k = _one(values, valid, X.MEAN, dtype)
            if k == 0:
                assert got == 99 and not ok
                continue
            f = Fraction(int(values[valid].sum()), k)
            assert got == (2 * f.numerator + f.denominator) // (2 * f.denominator)
    assert _one([1, 2], [1, 1], X.MEAN)[0] == 2 and _one([1, 1, 2], [1, 1, 1], X.MEAN)[0] == 1       # 1.5 up, 1.33 down
    assert _one([65535] * 16, [1] * 16, X.MEAN, np.uint16)[0] == 65535


def test_first_and_last_on_hand_made_cases_with_nodata_by_value():
    a = np.array([[[1, 1], [7, 7]], [[3, 3], [7, 8]]], dtype=np.uint8)       # nodata 7: (0, 1) is out, (1, 1) stays
    b = np.array([[[10, 10], [20, 20]], [[30, 30], [40, 40]]], dtype=np.uint8)
    vb = np.array([[1, 1], [0, 5]], dtype=np.uint8)
    args = ([a, b], [None, vb], [(0, 0, 2, 2)] * 2, [7, -1], 2, 2, 2)
    dst, ok, k = X.composite(*args, X.FIRST, 0)
    assert dst[..., 0].tolist() == [[1, 20], [3, 7]] and dst[1, 1].tolist() == [7, 8]
    assert ok.tolist() == [[1, 1], [1, 1]] and k.tolist() == [[2, 1], [1, 2]]
    dst, _, _ = X.composite(*args, X.LAST, 0)
    assert dst[..., 0].tolist() == [[10, 20], [3, 40]]
    # a hole: b alone, smaller, inside a 2 x 3 output, invalid at one of its pixels
    dst, ok, k = X.composite([b[:, :1]], [vb[:, :1]], [(0, 2, 2, 1)], [-1], 2, 2, 3, X.FIRST, 200)
    assert dst[..., 0].tolist() == [[200, 200, 10], [200, 200, 200]] and ok.tolist() == [[0, 0, 1], [0, 0, 0]]
    assert k.dtype == np.uint8 and ok.dtype == np.uint8 and dst.dtype == np.uint8
    # validity and nodata hold together: a pixel must pass both
    dst, _, k = X.composite([b], [vb], [(0, 0, 2, 2)], [40], 2, 2, 2, X.LAST, 0)
    assert k.tolist() == [[1, 1], [0, 0]]


def test_the_ladder_yields_every_count():
    for n in (1, 2, 3, 5, 16):
        oh, ow = 1, (n + 1) * n
        masks = X.ladder_validity(n, oh, ow)
        k = sum((m != 0).astype(int) for m in masks)
        assert sorted(set(k.ravel().tolist())) == list(range(n + 1))
        assert (k.ravel() == np.arange(oh * ow) % (n + 1)).all()
        assert all((m != 0).any() and (m == 0).any() for m in masks)        # every source is in some counts and out of some
    for n in X.NS:
        for oh, ow in X.SIZES[2:]:
            k = sum((m != 0).astype(int) for m in X.ladder_validity(n, oh, ow))
            assert set(k.ravel().tolist()) == set(range(n + 1))


def test_the_layouts_lie_inside_the_output():
    for name in X.LAYOUTS:
        for n in X.NS:
            for oh, ow in X.SIZES:
                rects = X.layout(name, n, oh, ow)
                assert len(rects) == n
                for dy, dx, h, w in rects:
                    assert h >= 1 and w >= 1 and dy >= 0 and dx >= 0 and dy + h <= oh and dx + w <= ow, (name, n, oh, ow)
    cover = np.zeros((33, 130), dtype=int)
    for dy, dx, h, w in X.layout("disjoint", 9, 33, 130):
        cover[dy:dy + h, dx:dx + w] += 1
    assert cover.max() == 1 and (cover == 0).any()                           # disjoint, with holes
    cover[:] = 0
    for dy, dx, h, w in X.layout("staggered", 5, 33, 130):
        cover[dy:dy + h, dx:dx + w] += 1
    assert cover.max() == 5 and cover.min() == 0 and set(range(1, 6)) <= set(cover.ravel().tolist())
    edges = X.layout("flush", 4, 33, 130)
    assert {(r[0] == 0, r[1] == 0, r[0] + r[2] == 33, r[1] + r[3] == 130) for r in edges} == {
        (True, True, False, True), (False, True, True, True), (True, True, True, False), (True, False, True, True)}
    assert X.layout("one_pixel", 3, 33, 130)[0][2:] == (1, 1)


def test_the_sweep_takes_every_value_of_every_axis():
    every = set()
    for ki, (kind, C) in enumerate(X.KINDS):
        seen = set()
        for si in range(len(X.SIZES)):
            for c in X.sweep(ki, si):
                seen |= {("n", c["n"]), ("mode", c["mode"]), ("layout", c["layout"]), ("validity", c["validity"]),
                         ("fill", c["fill"]), ("valid", c["want_valid"]), ("count", c["want_count"]), ("offset", c["offset"]),
                         ("mode, n", c["mode"], c["n"]), ("mode, validity", c["mode"], c["validity"]),
                         ("mode, layout", c["mode"], c["layout"]), ("size, mode", si, c["mode"])}
                assert c["validity"] != "ladder" or (c["layout"] == "full" and c["want_count"])
        want = ({("n", n) for n in X.NS} | {("mode", m) for m in range(4)} | {("layout", l) for l in X.LAYOUTS}
                | {("validity", v) for v in X.VALIDITY} | {("fill", 0), ("fill", X.TOP[kind])}
                | {(o, b) for o in ("valid", "count") for b in (False, True)} | {("offset", 0), ("offset", 1)}
                | {("mode, n", m, n) for m in range(4) for n in X.NS}       # the median on both sides of each bucket edge
                | {("mode, validity", m, v) for m in range(4) for v in X.VALIDITY}
                | {("size, mode", s, m) for s in range(len(X.SIZES)) for m in range(4)})
        assert want <= seen, (kind, C, sorted(want - seen, key=str))
        every |= seen
    assert {("mode, layout", m, l) for m in range(4) for l in X.LAYOUTS} <= every


# ---- the exports ----------------------------------------------------------------------------------------------------
def test_the_two_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "dsic_hip.h")).read()
    for name, nargs in NEW.items():
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert decl, name
        assert len(decl.group(1).split(",")) == nargs and decl.group(1).split(",")[-1].strip() == "void* stream"
        res, args = lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs and getattr(lib.load(), name) is not None
    for word in ("#define DSIC_COMPOSITE_FIRST 0", "#define DSIC_COMPOSITE_LAST 1", "#define DSIC_COMPOSITE_MEAN 2",
                 "#define DSIC_COMPOSITE_MEDIAN 3", "(2 S + k) / (2 k)", "2 * 16 * 65535 + 16 < 2^32"):
        assert word in header, word
    assert view.REDUCE == X.MODES == {"first": 0, "last": 1, "mean": 2, "median": 3}
    assert lib.load().dsic_abi_version() == 4


def test_the_two_exports_have_stream_recipes_in_the_table():
    """tests/composite_stream_cases.py registers them in tests/stream_cases.py's table on import: test_stream_cases_cpu.py
    and test_gpu_stream_order.py, collected after this file, then hold them as they hold every other export"""
    L = lib.load()
    assert len(CSC.NAMES) == len(set(CSC.NAMES)) == 4 and set(CSC.NAMES) <= set(SC.names())
    assert {e for n in CSC.NAMES for e in SC.build(n, L).exports} == set(NEW)
    assert all(SC.family(n) == "views" for n in CSC.NAMES)
    for n in CSC.NAMES:
        c = SC.build(n, L)
        a, b = c.inputs("A"), c.inputs("B")
        assert c.judged() == ["dst", "dv", "dn"] and a.keys() == b.keys()
        assert c.restate(a) != c.restate(b)
        k = np.frombuffer(c.restate(a), np.uint8)[-CSC.OH * CSC.OW:]
        assert k.max() == 3 and k.min() == 0                                 # all three overlap somewhere, a hole elsewhere


def test_the_composite_calls_check_their_arguments_without_a_gpu():
    L = lib.load()
    E, err = lib.DSIC_EINVAL, L.dsic_last_error
    a, b, m, d, v, c = 1 << 20, 1 << 21, 1 << 22, 1 << 24, 1 << 25, 1 << 26    # non-null, aligned, far apart

    def call(name, src=(a, b), val=(None, m), rect=((0, 0, 8, 8), (2, 2, 6, 6)), nodata=(-1, -1), n=None, C=3, dst=d, dv=v,
             dn=c, oh=8, ow=8, mode=3, fill=0, arrays=(True, True, True, True)):
        k = len(src)
        host = [(ctypes.c_void_p * k)(*src), (ctypes.c_void_p * k)(*val), (ctypes.c_int * (4 * k))(*[x for r in rect for x in r]),
                (ctypes.c_int * k)(*nodata)]
        host = [h if keep else None for h, keep in zip(host, arrays)]
        return getattr(L, "dsic_window_composite_" + name)(*host, k if n is None else n, C, dst, dv, dn, oh, ow, mode, fill, None)

    for name, top, elem in (("u8", 255, 1), ("u16", 65535, 2)):
        assert call(name, n=0) == E and b"n=0" in err()
        assert err().decode().partition(": ")[0] == "window_composite_" + name
        assert call(name, src=(a,) * 17, val=(None,) * 17, rect=((0, 0, 8, 8),) * 17, nodata=(-1,) * 17) == E and b"n=17" in err()
        for C in (0, 5):
            assert call(name, C=C) == E and f"C={C}".encode() in err()
        assert call(name, oh=0) == E and b"output" in err()
        assert call(name, ow=-1) == E and b"output" in err()
        assert call(name, oh=1 << 16, ow=1 << 15, dst=1 << 40, dv=1 << 44, dn=1 << 45) == E and b"2^31" in err()
        for i in range(4):
            assert call(name, arrays=tuple(j != i for j in range(4))) == E and b"null" in err()
        assert call(name, src=(a, None)) == E and b"source 1" in err() and b"null" in err()
        assert call(name, dst=None) == E and b"null" in err()
        assert call(name, rect=((0, 0, 8, 8), (2, 2, 0, 6))) == E and b"rect 0x6" in err()
        assert call(name, rect=((0, 0, 8, 8), (2, 2, 6, -1))) == E and b"at least 1x1" in err()
        for rect in ((2, 2, 7, 6), (2, 3, 6, 6), (-1, 0, 4, 4), (0, -1, 4, 4), (8, 0, 1, 1)):
            assert call(name, rect=((0, 0, 8, 8), rect)) == E and b"not inside the output" in err(), rect
        for mode in (-1, 4):
            assert call(name, mode=mode) == E and f"mode={mode}".encode() in err()
        assert call(name, fill=top + 1) == E and f"fill={top + 1}".encode() in err()
        assert call(name, fill=-1) == E and b"fill=-1" in err()
        assert call(name, nodata=(-1, top + 1)) == E and f"nodata={top + 1}".encode() in err()
        assert call(name, nodata=(-2, -1)) == E and b"nodata=-2" in err()
        # overlaps: an output over a source, over a validity window, over another output
        assert call(name, dst=a + 8 * 8 * 3 * elem - elem) == E and b"overlap" in err()
        assert call(name, dst=b - 8 * 8 * 3 * elem + elem) == E and b"overlap" in err()
        assert call(name, dst=m + 2 * elem) == E and b"overlap" in err()     # the validity window of source 1 is 36 bytes
        assert call(name, dv=a + 16) == E and b"overlap" in err()
        assert call(name, dn=m + 35) == E and b"overlap" in err()
        assert call(name, dv=d + 8 * 8 * 3 * elem - 1) == E and b"outputs overlap" in err()
        assert call(name, dn=v + 63) == E and b"outputs overlap" in err()
        assert call(name, dn=d) == E and b"outputs overlap" in err()
    assert call("u16", src=(a + 1, b)) == E and b"2-byte aligned" in err()
    assert call("u16", dst=d + 1) == E and b"2-byte aligned" in err()


# ---- the planning ---------------------------------------------------------------------------------------------------
THREE = [(150, 200), (75, 100), (38, 50)]


def test_stack_levels():
    assert codec.stack_levels([THREE, THREE], [(0, 0), (40, 60)]) == [(190, 260), (95, 130), (48, 65)]
    assert codec.stack_levels([THREE, THREE], [(0, 0), (40, 62)]) == [(190, 262), (95, 131)]
    assert codec.stack_levels([THREE, THREE], [(0, 0), (41, 60)]) == [(191, 260)]
    assert codec.stack_levels([THREE, THREE[:1]], [(0, 0), (40, 60)]) == [(190, 260)]
    assert codec.stack_levels([THREE, THREE[:2]], [(0, 0), (40, 60)]) == [(190, 260), (95, 130)]
    assert codec.stack_levels([THREE] * 5) == THREE                          # a temporal stack: the scenes' own levels
    assert codec.stack_levels([THREE], [(8, 16)], (400, 300)) == [(400, 300), (200, 150), (100, 75)]
    for lists, offsets, shape, word in (([], None, None, "0 scenes"), ([THREE] * 17, None, None, "17 scenes"),
                                        ([THREE], [(0, 0), (1, 1)], None, "offsets"), ([THREE], [(-4, 0)], None, "offsets"),
                                        ([THREE], [(0.5, 0)], None, "offsets"), ([THREE, THREE], [(0, 0), (40, 60)], (190, 259),
                                                                                  "outside the 190x259 grid"),
                                        ([THREE], None, (0, 5), "size")):
        with pytest.raises(ValueError, match=word):
            codec.stack_levels(lists, offsets, shape)


def test_a_scene_fits_its_stack_level():
    """scene s lies at (oy >> l, ox >> l) with its own level-l size: inside the stack's level l for every legal offset"""
    for h, w, oy, ox in ((151, 203, 44, 64), (150, 200, 4, 8), (97, 101, 12, 0), (149, 199, 100, 100)):
        own = codec.overview_shapes(h, w, 2)
        levels = codec.stack_levels([own, THREE], [(oy, ox), (0, 0)])
        assert len(levels) == 3
        for l, (H, W) in enumerate(levels):
            assert (oy >> l) + own[l][0] <= H and (ox >> l) + own[l][1] <= W


def test_stack_parts():
    odd = codec.overview_shapes(151, 203, 2)                                 # (151, 203), (76, 102), (38, 51)
    scenes = [((0, 0), THREE), ((40, 60), odd)]
    P = codec.stack_parts
    # level 0: no scene (right of the first, above the second), one, two
    assert P(0, scenes, (0, 210, 30, 40)) == []
    assert P(0, scenes, (5, 7, 30, 40)) == [(0, (5, 7, 30, 40), (0, 0, 30, 40))]
    assert P(0, scenes, (160, 100, 20, 50)) == [(1, (120, 40, 20, 50), (0, 0, 20, 50))]
    assert P(0, scenes, (30, 50, 100, 120)) == [(0, (30, 50, 100, 120), (0, 0, 100, 120)),
                                               (1, (0, 0, 90, 110), (10, 10, 90, 110))]
    assert P(0, scenes, (100, 150, 91, 113)) == [(0, (100, 150, 50, 50), (0, 0, 50, 50)),
                                                (1, (60, 90, 91, 113), (0, 0, 91, 113))]   # to the second's last pixel
    # level 2: the second scene lies at (10, 15) with 38 x 51 pixels
    assert P(2, scenes, (0, 55, 8, 10)) == []
    assert P(2, scenes, (0, 0, 9, 14)) == [(0, (0, 0, 9, 14), (0, 0, 9, 14))]
    assert P(2, scenes, (40, 10, 8, 56)) == [(1, (30, 0, 8, 51), (0, 5, 8, 51))]
    assert P(2, scenes, (5, 10, 40, 50)) == [(0, (5, 10, 33, 40), (0, 0, 33, 40)), (1, (0, 0, 35, 45), (5, 5, 35, 45))]
    whole = P(2, scenes, (0, 0, 48, 66))
    assert whole == [(0, (0, 0, 38, 50), (0, 0, 38, 50)), (1, (0, 0, 38, 51), (10, 15, 38, 51))]
    for s, part, rect in whole:                                              # a part is as large as its rect, inside its scene
        assert part[2:] == rect[2:] and part[0] + part[2] <= scenes[s][1][2][0] and part[1] + part[3] <= scenes[s][1][2][1]


def test_the_stack_is_exported_beside_the_reader():
    assert codec.SceneStack is view.SceneStack and codec.stack_levels is view.stack_levels
    assert codec.stack_parts is view.stack_parts and view.MAX_SCENES == 16
    for word in ("not the halving of the level-0", "median and halving do not commute"):
        assert word in " ".join(view.SceneStack.read.__doc__.split())
