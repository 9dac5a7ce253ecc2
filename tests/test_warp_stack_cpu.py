"""Warped scene stacks without a GPU: codec.compose_q16 against exact fractions, codec.stack_warp_parts against
warp_ref.brute_window, the identity claim on the restatement of tests/warp_stack_ref.py (integer offsets under a window's
own view are composite_ref / best_pixel_ref on the cropped windows), conditions on the kernel test's inputs, the two
exports' declarations and refusals (which need the library, not a device), and the ValueErrors of SceneStack that need no
device."""
import ctypes
import os
import re
import types
from fractions import Fraction

import numpy as np
import pytest

import best_pixel_ref as BP
import composite_ref as X
import stream_cases as SC
import warp_ref as R
import warp_stack_ref as WS
import warp_stack_stream_cases as WSC
from dsic_amd import codec, lib, view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"dsic_window_warp_composite_u8": 16, "dsic_window_warp_composite_u16": 16}
COMPOSE = codec.compose_q16                      # the feature under test: without it nothing in this file is held


# ---- compose_q16 ----------------------------------------------------------------------------------------------------
def _half_up(x):
    return int((x + Fraction(1, 2)).__floor__())


def test_compose_q16_is_the_exact_product_rounded_half_up():
    assert codec.compose_q16 is view.compose_q16 and codec.stack_warp_parts is view.stack_warp_parts
    rng = np.random.default_rng(5)
    for k in range(400):
        big = 1 << (4 + k % 17)                                          # products stay within check_q16
        A = [int(v) for v in rng.integers(-big, big + 1, 6)]
        V = [int(v) for v in rng.integers(-big, big + 1, 6)]
        A[2], A[5], V[2], V[5] = (int(v) for v in rng.integers(-(1 << 30), 1 << 30, 4))
        want = []
        for r in (0, 3):
            for c in range(3):
                x = Fraction(A[r] * V[c] + A[r + 1] * V[3 + c], 65536)
                want.append(_half_up(x) + (A[r + 2] if c == 2 else 0))
        assert COMPOSE(A, V) == tuple(want), (A, V)
    ident = (65536, 0, 0, 0, 65536, 0)
    m = (12345, -777, 1 << 40, 99, -65536, -(1 << 33))
    assert COMPOSE(ident, m) == m and COMPOSE(m, ident) == m
    for oy, ox in ((0, 0), (3, 5), (1000, 7), (1 << 20, 12)):
        off = (65536, 0, -oy * 65536, 0, 65536, -ox * 65536)
        assert COMPOSE(off, m) == (m[0], m[1], m[2] - oy * 65536, m[3], m[4], m[5] - ox * 65536)
    # -0.5 rounds up to 0, 0.5 to 1
    assert COMPOSE((1, 0, 0, 0, 1, 0), (32768, -32768, 32768, 32767, -32769, 0)) == (1, 0, 1, 0, -1, 0)
    big = (1 << 26, 1 << 26, 0, 0, 65536, 0)
    with pytest.raises(ValueError, match="coefficient"):
        COMPOSE(big, big)
    with pytest.raises(ValueError, match="offset"):
        COMPOSE((1 << 26, 0, (1 << 47) - 1, 0, 65536, 0), (65536, 0, 1 << 40, 0, 65536, 0))
    for bad in ((1, 2, 3), (1 << 27, 0, 0, 0, 1, 0), (0.5, 0, 0, 0, 1, 0)):
        with pytest.raises(ValueError):
            COMPOSE(bad, ident)
        with pytest.raises(ValueError):
            COMPOSE(ident, bad)


# ---- stack_warp_parts -----------------------------------------------------------------------------------------------
def _levels(H, W, n):
    return [(R.level_size(H, l), R.level_size(W, l)) for l in range(n)]


def test_stack_warp_parts_plans_each_scene_as_the_brute_window_says():
    scenes = [(view.affine_q16([[1, 0, 0], [0, 1, 0]]), _levels(40, 60, 3)),
              (view.affine_q16([[1, 0, -20], [0, 1, -30]]), _levels(33, 47, 1)),         # an integer offset, one level
              (view.affine_q16([[0.5, 0, -3.25], [0, 0.5, 2.5]]), _levels(30, 30, 2)),    # a 2x coarser scene, a fraction off
              (view.affine_q16([[0.8, 0.6, -10], [-0.6, 0.8, 25]]), _levels(50, 50, 4)),  # a turned scene
              (view.affine_q16([[1, 0, -500], [0, 1, 0]]), _levels(20, 20, 2))]           # wholly beside every view below
    views = [([[1, 0, 0], [0, 1, 0]], (24, 31)), ([[2.6, 0, 1.5], [0, 2.6, 0.25]], (17, 20)), ([[0.3, 0.1, 12], [-0.1, 0.3, 20]], (25, 19)),
             ([[4.1, 0, 0], [0, 4.1, 0]], (12, 14)), ([[9, 0, -3], [0, 9, -3]], (7, 9))]
    seen_levels = set()
    for matrix, size in views:
        v = view.affine_q16(matrix)
        for mode_name, mode in R.MODES.items():
            parts = codec.stack_warp_parts(scenes, v, size, mode)
            assert parts == codec.stack_warp_parts(scenes, v, size, mode_name)
            assert [p[0] for p in parts] == sorted(p[0] for p in parts) and 4 not in [p[0] for p in parts]
            met = {}
            for s, m, level, lw in parts:
                A, levels = scenes[s]
                assert m == COMPOSE(A, v) and level == R.warp_level(len(levels), m)
                assert lw == R.warp_window(level, *levels[level], *levels[0], m, *size, mode)
                met[s] = (m, level, lw)
                seen_levels.add((s, level))
            for s, (A, levels) in enumerate(scenes):
                m = COMPOSE(A, v)
                level = R.warp_level(len(levels), m)
                brute = R.brute_window(level, *levels[level], *levels[0], m, *size, mode)
                if s not in met:
                    assert brute is None, (s, matrix)
                elif brute is not None:                                      # the corner rule holds every tap
                    y0, x0, h, w = met[s][2]
                    assert y0 <= brute[0] and x0 <= brute[1] and brute[0] + brute[2] <= y0 + h and brute[1] + brute[3] <= x0 + w
    assert {l for s, l in seen_levels if s == 0} == {0, 1, 2} and {l for s, l in seen_levels if s == 1} == {0}
    assert {l for s, l in seen_levels if s == 3} >= {0, 2}
    with pytest.raises(ValueError, match="size"):
        codec.stack_warp_parts(scenes, view.affine_q16(views[0][0]), (0, 3), 0)


# ---- the identity claim, on the restatement -------------------------------------------------------------------------
def _as_sources(srcs, masks, rects, nodata, window, sample):
    y0, x0, h, w = window
    v = view.affine_q16(view.window_affine(y0, x0, h, w, h, w))
    out = []
    for img, mask, (dy, dx, sh, sw), nd in zip(srcs, masks, rects, nodata):
        m = COMPOSE((65536, 0, -dy * 65536, 0, 65536, -dx * 65536), v)
        out.append(dict(src=img, val=mask, sy0=0, sx0=0, sh=sh, sw=sw, shift=0, LH=sh, LW=sw, H=sh, W=sw, m=m, nodata=nd))
    return out


def _cropped(srcs, masks, rects, nodata, window):
    scenes = [((dy, dx), [(h, w)]) for dy, dx, h, w in rects]
    parts = view.stack_parts(0, scenes, window)
    pick = lambda a, p: None if a is None else np.ascontiguousarray(a[p[0]:p[0] + p[2], p[1]:p[1] + p[3]])
    return ([pick(srcs[s], p) for s, p, _ in parts], [pick(masks[s], p) for s, p, _ in parts], [r for _, _, r in parts],
            [nodata[s] for s, _, _ in parts], [s for s, _, _ in parts])


HOLDS_FOR_CUBIC = True       # recorded: at phase 0 the cubic weights are (0, 2^22, 0, 0), and a pixel with a tap that does
#                              not count is the bilinear one, whose phase-0 weights are (128, 0)


def test_integer_offsets_under_a_windows_own_view_are_the_composite_of_the_cropped_windows():
    held = 0
    for kind, C in (("u8", 3), ("u16", 1), ("u16", 4)):
        for n, layout, validity in ((1, "full", "random"), (4, "staggered", "random"), (5, "flush", "nodata"),
                                    (9, "disjoint", "none"), (16, "staggered", "random")):
            oh, ow = 23, 37
            case = dict(n=n, mode=0, layout=layout, validity=validity)
            srcs, masks, rects, nodata = X.case_inputs(kind, C, oh, ow, case)
            if n > 1:
                srcs[1][2:6, 3:9] = 0                                        # A + B = 0
            for window in ((0, 0, oh, ow), (5, 7, 11, 20), (oh - 3, ow - 4, 3, 4)):
                c_srcs, c_masks, c_rects, c_nodata, c_ids = _cropped(srcs, masks, rects, nodata, window)
                h, w = window[2:]
                for sample in (1, 0, 2):
                    if sample == 2 and not HOLDS_FOR_CUBIC:
                        continue
                    sources = _as_sources(srcs, masks, rects, nodata, window, sample)
                    for reduce in range(6):
                        index = ("nd", 0, C - 1) if C > 1 else ("band", 0)
                        got = WS.warp_composite(sources, C, (h, w), sample, reduce, index, 9, None, warp_fill=3)
                        if not c_srcs:
                            want = (np.full((h, w, C), 9, srcs[0].dtype), np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8),
                                    np.full((h, w), 255, np.uint8))
                        elif reduce in (WS.MEAN, WS.MEDIAN):
                            want = tuple(X.composite(c_srcs, c_masks, c_rects, c_nodata, C, h, w, reduce, 9)) + (None,)
                        else:
                            want = BP.pick(c_srcs, c_masks, c_rects, c_nodata, c_ids, C, h, w, reduce, index, 9)
                        for g, x, name in zip(got, want, ("image", "valid", "count", "source")):
                            if g is not None and x is not None:
                                assert g.dtype == x.dtype and np.array_equal(g, x), (kind, C, n, window, sample, reduce, name)
                        held += 1
    assert held > 700


# ---- conditions on the kernel test's inputs -------------------------------------------------------------------------
def test_the_sweep_meets_every_reduce_under_every_sample_mode_for_every_list_length():
    seen, outputs = set(), set()
    for ki in range(len(WS.KINDS)):
        for si in range(len(WS.SIZES)):
            for c in WS.sweep(ki, si):
                seen.add((c["n"], c["reduce"], c["sample"]))
                outputs.add((c["want_valid"], c["want_count"], c["want_source"]))
                assert not (c["want_source"] and c["reduce"] in (WS.MEAN, WS.MEDIAN))
                a, b = c["index"][1], c["index"][-1]
                assert 0 <= a < WS.KINDS[ki][1] and 0 <= b < WS.KINDS[ki][1]
    assert seen == {(n, r, s) for n in WS.NS for r in range(6) for s in range(3)}
    assert len(outputs) == 8
    assert WS.NS == [1, 4, 5, 8, 9, 16] and WS.SIZES == [(1, 1), (7, 9), (17, 33), (33, 130)]
    assert {v for v, _, _ in WS.LIST} == {"rot30", "mirror", "magnify3", "minify2.5", "overhang", "beside", "patch"}
    assert {m for _, m, _ in WS.LIST[:4]} | {m for _, m, _ in WS.LIST[4:]} == {"valid", "nodata", "none"}
    assert {l for _, _, l in WS.LIST[:4]} == {0, 1, 2}


def test_the_largest_list_lets_every_source_win_leaves_a_hole_and_holds_an_undefined_index():
    size = WS.SIZES[-1]
    for kind, C in (("u8", 3), ("u16", 4), ("u16", 2)):
        for sample in range(3):
            srcs = WS.sources(kind, C, size, 16, sample)
            meets = {i for i, s in enumerate(srcs) if s["meets"]}
            assert meets == set(range(16)) - {2}
            index = ("nd", 0, C - 1)
            first = WS.warp_composite(srcs, C, size, sample, WS.FIRST, index, 0, None)
            best = WS.warp_composite(srcs, C, size, sample, WS.MAX, index, 0, None)
            assert set(first[3].ravel().tolist()) == meets | {255} and set(best[3].ravel().tolist()) == meets | {255}
            assert first[2].max() > 8 and (best[2] < first[2]).any()        # a list longer than 8, and A + B = 0 somewhere
            other = WS.warp_composite(srcs, C, size, sample, WS.MAX, index, 0, None, warp_fill=201)
            assert all(np.array_equal(a, b) for a, b in zip(best, other))   # `any fill` in the chain's first step


# ---- the exports ----------------------------------------------------------------------------------------------------
def test_the_two_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "dsic_hip.h")).read()
    for name, nargs in NEW.items():
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert decl, name
        params = [p.strip() for p in decl.group(1).split(",")]
        assert len(params) == nargs and params[-1] == "void* stream"
        res, args = lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs and getattr(lib.load(), name) is not None
        for p, t in zip(params, args):                                       # pointer for pointer, int for int
            assert ("*" in p) == (t is ctypes.c_void_p) and (t is ctypes.c_void_p or t is ctypes.c_int), (name, p)
        assert [p.split()[-1].lstrip("*") for p in params[:3] + params[6:]] == [
            "sources", "n", "C", "dst_source", "oh", "ow", "sample_mode", "reduce_mode", "kind", "a", "b", "fill", "stream"]
    struct = re.search(r"typedef struct dsic_warp_source \{(.*?)\} dsic_warp_source;", header, flags=re.S).group(1)
    fields = [f.strip().lstrip("*") for line in struct.split(";") for f in line.split(",") if f.strip()]
    names = [f.split()[-1].lstrip("*").partition("[")[0] for f in fields]
    assert names == [n for n, _ in lib.WarpSource._fields_] and ctypes.sizeof(lib.WarpSource) == 112
    for word in ("defined as the chain of the exports above, bit for bit", "dsic_window_warp_u8 / _u16 with that source's arguments",
                 "dst_source with mean or median"):
        assert word in header, word


def test_the_two_exports_have_stream_recipes_in_the_table():
    L = lib.load()
    assert len(WSC.NAMES) == len(set(WSC.NAMES)) == 4 and set(WSC.NAMES) <= set(SC.names())
    assert {e for n in WSC.NAMES for e in SC.build(n, L).exports} == set(NEW)
    assert all(SC.family(n) == "views" for n in WSC.NAMES)
    for n in WSC.NAMES:
        c = SC.build(n, L)
        a, b = c.inputs("A"), c.inputs("B")
        assert a.keys() == b.keys() and c.restate(a) != c.restate(b)
        plane = WSC.OH * WSC.OW
        out = np.frombuffer(c.restate(a), np.uint8)
        if n.endswith("max"):
            assert c.judged() == ["dst", "dv", "dn", "ds"] and set(out[-plane:].tolist()) == set(WSC.IDS) | {255}
            assert out[-2 * plane:-plane].max() == 3
        else:
            assert c.judged() == ["dst", "dv", "dn"] and out[-plane:].max() == 3 and out[-plane:].min() == 0


def test_the_calls_check_their_arguments_without_a_gpu():
    L = lib.load()
    E, err = lib.DSIC_EINVAL, L.dsic_last_error
    a, b, m, d, v, c, s = 1 << 20, 1 << 21, 1 << 22, 1 << 24, 1 << 25, 1 << 26, 1 << 27   # non-null, aligned, far apart
    ident = (65536, 0, 0, 0, 65536, 0)
    ok = dict(src=a, val=None, sh=8, sw=8, sy0=0, sx0=0, shift=0, LH=8, LW=8, H=8, W=8, nodata=-1, id=0, m=ident)

    def call(name, sources=({}, {"src": b, "val": m, "id": 7}), n=None, C=3, dst=d, dv=v, dn=c, ds=s, oh=8, ow=8, sample=0,
             reduce=4, kind=2, ba=2, bb=0, fill=0, table=True):
        rows = [dict(ok, **kw) for kw in sources]
        host = (lib.WarpSource * max(1, len(rows)))(*[
            lib.WarpSource(r["src"], r["val"], r["sh"], r["sw"], r["sy0"], r["sx0"], r["shift"], r["LH"], r["LW"], r["H"], r["W"],
                           r["nodata"], r["id"], 0, (ctypes.c_int64 * 6)(*r["m"])) for r in rows])
        return getattr(L, "dsic_window_warp_composite_" + name)(host if table else None, len(rows) if n is None else n, C, dst, dv,
                                                                 dn, ds, oh, ow, sample, reduce, kind, ba, bb, fill, None)

    for name, top, elem, cmin in (("u8", 255, 1, 3), ("u16", 65535, 2, 1)):
        assert call(name, n=0) == E and b"n=0" in err()
        assert err().decode().partition(": ")[0] == "window_warp_composite_" + name
        assert call(name, sources=({},) * 17) == E and b"n=17" in err()
        assert call(name, table=False) == E and b"null" in err()
        assert call(name, dst=None) == E and b"null" in err()
        for C in (cmin - 1, 5):
            assert call(name, C=C) == E and f"C={C} must be in {cmin}..4".encode() in err()
        for sample in (-1, 3):
            assert call(name, sample=sample) == E and f"mode={sample} (0 bilinear, 1 nearest, 2 cubic)".encode() in err()
        assert call(name, oh=0) == E and b"must be 1x1 .. 2^20x2^20" in err()
        assert call(name, ow=(1 << 20) + 1) == E and b"must be 1x1 .. 2^20x2^20" in err()
        assert call(name, oh=1 << 16, ow=1 << 15, dst=1 << 40, dv=1 << 44, dn=1 << 45, ds=1 << 46) == E and b"under 2^31" in err()
        for reduce in (-1, 6):
            assert call(name, reduce=reduce) == E and f"mode={reduce}".encode() in err() and b"4 max, 5 min" in err()
        for reduce in (4, 5):
            for kind in (-1, 3):
                assert call(name, reduce=reduce, kind=kind) == E and f"kind={kind} (0 band, 1 difference, 2 nd)".encode() in err()
            assert call(name, reduce=reduce, ba=3) == E and b"band 3 is outside 0..2" in err()
            assert call(name, reduce=reduce, bb=-1) == E and b"band -1 is outside 0..2" in err()
            assert call(name, reduce=reduce, kind=0, ba=3, bb=0) == E and b"band 3" in err()
        for reduce in (2, 3):
            assert call(name, reduce=reduce) == E and b"dst_source goes with first, last, max and min" in err()
            assert call(name, reduce=reduce, ds=None, kind=9, ba=-1, bb=9, dst=a) == E and b"overlap" in err()   # not the index
        assert call(name, fill=top + 1) == E and f"fill={top + 1} must be a pixel value".encode() in err()
        assert call(name, dn=v + 63) == E and b"outputs overlap" in err()
        assert call(name, ds=d + 8 * 8 * 3 * elem - 1) == E and b"outputs overlap" in err()
        # per source, in warp_check's words behind the source's number
        head = f"window_warp_composite_{name}: source 1: ".encode()
        two = lambda **kw: call(name, sources=({}, dict({"src": b, "val": m, "id": 7}, **kw)))
        assert two(src=None) == E and head + b"null pointer" in err()
        assert two(shift=16) == E and head + b"shift=16 must be in 0..15" in err()
        assert two(H=0) == E and head + b"image 0x8" in err()
        assert two(LH=7) == E and head + b"level 0 of a 8x8 image is not 7x8" in err()
        assert two(sy0=1) == E and head + b"source window 8x8 at (1, 0) of a 8x8 level" in err()
        assert two(m=(1 << 27, 0, 0, 0, 65536, 0)) == E and head + b"matrix entry 0 = 134217728 is outside" in err()
        assert two(m=(65536, 0, 1 << 47, 0, 65536, 0)) == E and head + b"matrix entry 2" in err()
        assert two(sh=7) == E and head + b"the view's taps cover rows 0..7, columns 0..7 of level 0, outside the source window 7x8" in err()
        assert two(nodata=top + 1) == E and head + f"nodata={top + 1}".encode() in err()
        assert two(id=255) == E and head + b"id=255 must be in 0..254" in err()
        assert two(id=-1) == E and b"id=-1" in err()
        assert two(src=d + 8 * 8 * 3 * elem - elem) == E and b"source 1 and an output overlap" in err()
        assert two(val=s + 63) == E and b"source 1 and an output overlap" in err()
        assert call(name, dv=a + 16) == E and b"source 0 and an output overlap" in err()
    assert call("u16", sources=({"src": a + 1},)) == E and b"source 0 must be 2-byte aligned" in err()
    assert call("u16", dst=d + 1) == E and b"dst must be 2-byte aligned" in err()


# ---- SceneStack without a device ------------------------------------------------------------------------------------
def _fake(kind=codec.KIND_U16_HWC, C=4, H=40, W=60, levels=2):
    return types.SimpleNamespace(kind=kind, shape=(H, W, C), levels=_levels(H, W, levels), _dev="cpu")


def test_the_constructor_and_the_methods_raise_what_needs_no_device():
    readers = [_fake(), _fake(H=20, W=30)]
    ident, half = [[1, 0, 0], [0, 1, 0]], [[0.5, 0, 0], [0, 0.5, 0]]
    stack = codec.SceneStack(readers, shape=(40, 60), placements=[ident, half])
    assert stack.levels == [(40, 60)] and stack.shape == (40, 60, 4) and stack.offsets is None
    assert stack.placements == [view.affine_q16(ident), view.affine_q16(half)]
    plain = codec.SceneStack(readers, [(0, 0), (8, 12)])
    assert plain.placements is None and plain.offsets == [(0, 0), (8, 12)] and len(plain.levels) == 2
    assert plain._warp_scenes[1][0] == (65536, 0, -8 * 65536, 0, 65536, -12 * 65536)
    for kw, word in (({"offsets": [(0, 0), (0, 0)], "shape": (40, 60), "placements": [ident, half]}, "exclude"),
                     ({"placements": [ident, half]}, "shape"), ({"shape": (40, 60), "placements": [ident]}, "1 placements for 2"),
                     ({"shape": (40, 60), "placements": [ident, [[1, 0], [0, 1]]]}, "affine_q16"),
                     ({"shape": (40, 60), "placements": [ident, [[2000, 0, 0], [0, 1, 0]]]}, "coefficient"),
                     ({"shape": (0, 60), "placements": [ident, half]}, "SceneStack")):
        with pytest.raises(ValueError, match=word):
            codec.SceneStack(readers, **kw)
    for call in (lambda: stack.read(0, 0, 8, 8), lambda: stack.render(0, 0, 8, 8), lambda: stack.render_index(0, 0, 8, 8, ("nd", 3, 0))):
        with pytest.raises(ValueError, match="read_warped"):
            call()
    for st in (stack, plain):
        for kw, word in (({"resampling": "average"}, "resampling='average' \\(bilinear, nearest, cubic\\)"),
                         ({"matrix": [[1, 0], [0, 1]]}, "affine_q16"), ({"matrix": [[2000, 0, 0], [0, 1, 0]]}, "coefficient"),
                         ({"size": (0, 4)}, "size"), ({"size": ((1 << 20) + 1, 1)}, "2\\^20"), ({"size": (1 << 16, 1 << 15)}, "2\\^31"),
                         ({"reduce": "mode"}, "SceneStack.read_warped: reduce="), ({"reduce": ("max", ("nd", 4, 0))}, "bands in 0 .. 3"),
                         ({"reduce": "median", "with_source": True}, "with_source"), ({"fill": 65536}, "fill=65536"),
                         ({"fill": 1.5}, "fill")):
            with pytest.raises(ValueError, match=word):
                st.read_warped(**dict({"matrix": ident, "size": (8, 8)}, **kw))
        with pytest.raises(ValueError, match="SceneStack.render_warped: a uint16 stack needs stretch="):
            st.render_warped(ident, (8, 8))
        with pytest.raises(ValueError, match="SceneStack.render_index_warped"):
            st.render_index_warped(ident, (8, 8), ("band", 0))
        with pytest.raises(ValueError, match="resampling"):
            st.render_index_warped(ident, (8, 8), ("nd", 3, 0), resampling="average")
