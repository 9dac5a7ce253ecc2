"""Best-pixel composites without a GPU: the restatement of tests/best_pixel_ref.py against a plain per-pixel loop and
against composite_ref for first and last, conditions on the sweep's inputs (every axis value taken, every source wins
somewhere, three mutants of the definition differ on them), codec.stack_reduce, and the two exports' declarations,
recipes and refusals (which need the library, not a device)."""
import ctypes
import os
import re

import numpy as np
import pytest

import best_pixel_ref as BP
import best_pixel_stream_cases as BSC
import composite_ref as X
import index_ref
import stream_cases as SC
from dsic_amd import codec, lib, view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"dsic_window_composite_pick_u8": 19, "dsic_window_composite_pick_u16": 19}
REDUCE = codec.stack_reduce                      # the feature under test: without it nothing in this file is held


def _cases(sizes=range(len(BP.SIZES))):
    for ki, (kind, C) in enumerate(BP.KINDS):
        for si in sizes:
            for case in BP.sweep(ki, si):
                yield kind, C, BP.SIZES[si], case


def _restated(kind, C, size, case, **mutant):
    srcs, masks, rects, nodata, ids = BP.case_inputs(kind, C, *size, case)
    return BP._pick(srcs, masks, rects, nodata, ids, C, *size, case["mode"], case["index"], case["fill"], **mutant)


# ---- the restatement ------------------------------------------------------------------------------------------------
def _by_loop(srcs, masks, rects, nodata, ids, C, oh, ow, mode, index, fill):
    """the definition, pixel by pixel and source by source, in Python integers"""
    kind, a, b = index_ref.parse(index)
    top = X.TOP["u8" if srcs[0].dtype == np.uint8 else "u16"]
    dst = np.full((oh, ow, C), fill, dtype=srcs[0].dtype)
    valid, count, source = (np.zeros((oh, ow), np.uint8), np.zeros((oh, ow), np.uint8), np.full((oh, ow), 255, np.uint8))
    for y in range(oh):
        for x in range(ow):
            cands = []                                                       # (position, u or None)
            for i, (dy, dx, h, w) in enumerate(rects):
                if not (dy <= y < dy + h and dx <= x < dx + w):
                    continue
                if masks[i] is not None and masks[i][y - dy, x - dx] == 0:
                    continue
                px = [int(v) for v in srcs[i][y - dy, x - dx]]
                if nodata[i] >= 0 and all(v == nodata[i] for v in px):
                    continue
                A, B = px[a], px[b]
                if kind == "nd":
                    u = None if A + B == 0 else (40000 * A + (A + B)) // (2 * (A + B))
                else:
                    u = A - B + top if kind == "difference" else A
                if mode in (BP.FIRST, BP.LAST) or u is not None:
                    cands.append((i, u))
            if not cands:
                continue
            if mode == BP.FIRST:
                win = cands[0][0]
            elif mode == BP.LAST:
                win = cands[-1][0]
            else:
                best = (max if mode == BP.MAX else min)(u for _, u in cands)
                win = next(i for i, u in cands if u == best)                 # the first of equals
            dy, dx = rects[win][:2]
            dst[y, x] = srcs[win][y - dy, x - dx]
            valid[y, x], count[y, x], source[y, x] = 1, len(cands), win if ids is None else ids[win]
    return dst, valid, count, source


def test_the_restatement_is_a_plain_loop_on_the_two_smallest_sizes():
    seen = set()
    for kind, C, (oh, ow), case in _cases(sizes=(0, 1)):
        srcs, masks, rects, nodata, ids = BP.case_inputs(kind, C, oh, ow, case)
        args = (srcs, masks, rects, nodata, ids, C, oh, ow, case["mode"], case["index"], case["fill"])
        for got, want, name in zip(BP.pick(*args), _by_loop(*args), ("dst", "valid", "count", "source")):
            assert got.dtype == want.dtype and np.array_equal(got, want), (kind, C, oh, ow, case, name)
        seen.add((case["mode"], case["index"][0]))
    assert {(m, k) for m in (BP.MAX, BP.MIN) for k in BP.INDEX_KINDS} <= seen
    # by hand: one pixel, three sources of two bands; nd = 10000 (A - B) / (A + B) is 0, undefined, 3333, 3333
    srcs = [np.array([[[v, w]]], np.uint8) for v, w in ((5, 5), (0, 0), (2, 1), (4, 2))]
    one = lambda mode, index, ids=None: [int(o.ravel()[0]) for o in BP.pick(srcs, [None] * 4, [(0, 0, 1, 1)] * 4, [-1] * 4,
                                                                             ids, 2, 1, 1, mode, index, 77)[::3]]
    assert one(BP.MAX, ("nd", 0, 1)) == [2, 2] and one(BP.MIN, ("nd", 0, 1)) == [5, 0]       # the tie goes to the first
    assert one(BP.MIN, ("band", 0)) == [0, 1] and one(BP.MIN, ("difference", 0, 1)) == [5, 0]
    assert one(BP.MAX, ("difference", 0, 1), [9, 8, 7, 6]) == [4, 6] and one(BP.LAST, ("nd", 0, 1), [9, 8, 7, 6]) == [4, 6]
    count = BP.pick(srcs, [None] * 4, [(0, 0, 1, 1)] * 4, [-1] * 4, None, 2, 1, 1, BP.MAX, ("nd", 0, 1), 77)[2]
    assert int(count[0, 0]) == 3                                             # the undefined one does not count
    none = BP.pick(srcs[1:2], [None], [(0, 0, 1, 1)], [-1], None, 2, 1, 1, BP.MIN, ("nd", 0, 1), 77)
    assert [int(o.ravel()[0]) for o in none] == [77, 0, 0, 255]


def test_first_and_last_are_composite_refs_and_name_the_first_or_last_candidate():
    held = 0
    for kind, C, (oh, ow), case in _cases():
        if case["mode"] not in (BP.FIRST, BP.LAST) or (oh, ow) == BP.SIZES[3] and case["n"] > 8:
            continue
        srcs, masks, rects, nodata, ids = BP.case_inputs(kind, C, oh, ow, case)
        dst, valid, count, source = BP.pick(srcs, masks, rects, nodata, ids, C, oh, ow, case["mode"], case["index"], case["fill"])
        want = X.composite(srcs, masks, rects, nodata, C, oh, ow, case["mode"], case["fill"])
        assert all(np.array_equal(g, w) and g.dtype == w.dtype for g, w in zip((dst, valid, count), want)), (kind, C, case)
        _, cand = BP.candidates(srcs, masks, rects, nodata, C, oh, ow)
        ids = list(range(case["n"])) if ids is None else ids
        for i in range(case["n"]):
            others = cand[:i] if case["mode"] == BP.FIRST else cand[i + 1:]
            assert np.array_equal(source == ids[i], cand[i] & ~others.any(axis=0)), (kind, C, case, i)
        assert np.array_equal(source == 255, ~cand.any(axis=0))
        held += 1
    assert held > 60


# ---- conditions on the inputs ---------------------------------------------------------------------------------------
def test_the_sweep_takes_every_value_of_every_axis():
    every = set()
    for ki, (kind, C) in enumerate(BP.KINDS):
        seen = set()
        for si in range(len(BP.SIZES)):
            for c in BP.sweep(ki, si):
                ranked = c["mode"] in (BP.MAX, BP.MIN)
                seen |= {("n", c["n"]), ("mode", c["mode"]), ("layout", c["layout"]), ("validity", c["validity"]),
                         ("fill", c["fill"]), ("valid", c["want_valid"]), ("count", c["want_count"]),
                         ("source", c["want_source"]), ("ids", c["ids"]), ("offset", c["offset"]),
                         ("mode, n", c["mode"], c["n"]), ("mode, validity", c["mode"], c["validity"]),
                         ("size, mode", si, c["mode"]), ("mode, source, ids", c["mode"], c["want_source"], c["ids"]),
                         ("outputs", c["want_valid"], c["want_count"], c["want_source"])}
                if ranked:
                    seen |= {("index", c["index"][0]), ("mode, index", c["mode"], c["index"][0]), ("low", c["low"])}
                every |= {("mode, layout", c["mode"], c["layout"]), ("size, index", si, c["index"][0]) if ranked else None}
                assert c["validity"] != "ladder" or (c["layout"] == "full" and c["want_count"])
                a, b = c["index"][1], c["index"][-1]
                assert 0 <= a < C and 0 <= b < C and (C == 1 or c["index"][0] == "band" or a != b)
        modes = (BP.FIRST, BP.LAST, BP.MAX, BP.MIN)
        want = ({("n", n) for n in BP.NS} | {("mode", m) for m in modes} | {("layout", l) for l in BP.LAYOUTS}
                | {("validity", v) for v in BP.VALIDITY} | {("fill", 0), ("fill", X.TOP[kind])}
                | {(o, b) for o in ("valid", "count", "source", "ids") for b in (False, True)} | {("offset", 0), ("offset", 1)}
                | {("mode, n", m, n) for m in modes for n in BP.NS}      # the ranked kernels on both sides of 4, 8, 16
                | {("mode, validity", m, v) for m in modes for v in BP.VALIDITY}
                | {("size, mode", s, m) for s in range(len(BP.SIZES)) for m in modes}
                | {("mode, source, ids", m, s, i) for m in modes for s in (False, True) for i in (False, True)}
                | {("outputs", v, c, s) for v in (False, True) for c in (False, True) for s in (False, True)}
                | {("index", k) for k in BP.INDEX_KINDS} | {("mode, index", m, k) for m in (BP.MAX, BP.MIN) for k in BP.INDEX_KINDS}
                | {("low", kind == "u8"), ("low", False)})
        assert want <= seen, (kind, C, sorted(want - seen, key=str))
    assert {("mode, layout", m, l) for m in (BP.FIRST, BP.LAST, BP.MAX, BP.MIN) for l in BP.LAYOUTS} <= every
    assert {("size, index", s, k) for s in range(len(BP.SIZES)) for k in BP.INDEX_KINDS} <= every
    for n in BP.NS:
        ids = BP.case_ids(n)
        assert len(set(ids)) == n and 254 in ids and min(ids) >= 0 and max(ids) <= 254


def test_every_source_wins_somewhere_and_the_definitions_mutants_differ():
    """at the two larger sizes: every position of the longest list wins in some ranked case and 255 occurs; and per
    kind ties, A + B = 0 and undefined candidates are there, since the mutants that treat them otherwise give other
    results"""
    for si in (2, 3):
        oh, ow = BP.SIZES[si]
        winners = set()
        for ki, (kind, C) in enumerate(BP.KINDS):
            differ = {"ties": 0, "rank": 0, "undefined": 0}
            for case in BP.sweep(ki, si):
                if case["mode"] not in (BP.MAX, BP.MIN):
                    continue
                plain = _restated(kind, C, (oh, ow), case)
                ids = BP.case_ids(case["n"]) if case["ids"] else list(range(case["n"]))
                winners |= {255 if v == 255 else ids.index(v) for v in set(plain[3].ravel().tolist())}
                same = lambda other: all(np.array_equal(g, w) for g, w in zip(plain, other))
                differ["ties"] += not same(_restated(kind, C, (oh, ow), case, ties_to_last=True))
                if case["index"][0] == "nd":
                    differ["rank"] += not same(_restated(kind, C, (oh, ow), case, rank=lambda A, B: A - B + 65535))
                    differ["undefined"] += not same(_restated(kind, C, (oh, ow), case, keep_undefined=True))
            # one band: a = b, every defined nd is 0 and every A - B too, so the two rankings are the same one
            assert all(v for key, v in differ.items() if C > 1 or key != "rank"), (kind, C, si, differ)
        assert winners == set(range(max(BP.NS))) | {255}, (si, sorted(winners))


# ---- codec.stack_reduce ---------------------------------------------------------------------------------------------
def test_stack_reduce_names_the_accepted_forms():
    assert codec.stack_reduce is view.stack_reduce
    assert [REDUCE(name, 3) for name in ("first", "last", "mean", "median")] == [(0, 0, 0, 0), (1, 0, 0, 0), (2, 0, 0, 0), (3, 0, 0, 0)]
    assert REDUCE(("max", ("nd", 3, 0)), 4) == (4, 2, 3, 0) and REDUCE(("min", ("nd", 0, 3)), 4) == (5, 2, 0, 3)
    assert REDUCE(("max", ("difference", 1, 2)), 3) == (4, 1, 1, 2) and REDUCE(("min", ("band", 2)), 3) == (5, 0, 2, 2)
    assert REDUCE(["max", ["band", 0]], 1) == (4, 0, 0, 0)
    assert view.REDUCE == X.MODES and view.RANKED == {"max": BP.MAX, "min": BP.MIN} and view.NO_SOURCE == BP.NO_SOURCE
    assert {k: v for k, v in BP.MODES.items() if k in view.RANKED} == view.RANKED
    for bad in ("mode", "max", "min", ("max",), ("max", ("nd", 3, 0), 1), ("mean", ("nd", 3, 0)), ("first", ("band", 0)),
                ("max", "nd"), ("max", ("nd", 3)), ("max", ("band", 0, 1)), ("max", ("ndvi", 3, 0)), ("max", ("nd", 4, 0)),
                ("max", ("nd", 0, -1)), ("min", ("band", 4)), ("max", ("nd", 0.5, 1)), ("max", 5), (4, ("nd", 3, 0)), None, 4):
        with pytest.raises(ValueError) as err:
            REDUCE(bad, 4)
        text = str(err.value)
        assert all(w in text for w in ("first, last, mean, median", "('max', index)", "('min', index)", "('nd', a, b)",
                                       "('difference', a, b)", "('band', a)")), (bad, text)
    with pytest.raises(ValueError, match="bands in 0 .. 2"):
        REDUCE(("max", ("nd", 3, 0)), 3)
    with pytest.raises(ValueError, match="SceneStack.read: reduce="):
        REDUCE("mode", 3, "SceneStack.read")


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
        assert [p.split()[-1].lstrip("*") for p in params[4:5] + params[10:11] + params[13:18]] == [
            "id", "dst_source", "mode", "kind", "a", "b", "fill"]
    for word in ("#define DSIC_COMPOSITE_MAX 4", "#define DSIC_COMPOSITE_MIN 5", "A + B = 0 is not a candidate",
                 "the candidate that comes first in list order", "255 where k = 0"):
        assert word in header, word


def test_the_two_exports_have_stream_recipes_in_the_table():
    L = lib.load()
    assert len(BSC.NAMES) == len(set(BSC.NAMES)) == 4 and set(BSC.NAMES) <= set(SC.names())
    assert {e for n in BSC.NAMES for e in SC.build(n, L).exports} == set(NEW)
    assert all(SC.family(n) == "views" for n in BSC.NAMES)
    for n in BSC.NAMES:
        c = SC.build(n, L)
        a, b = c.inputs("A"), c.inputs("B")
        assert c.judged() == ["dst", "dv", "dn", "ds"] and a.keys() == b.keys()
        assert c.restate(a) != c.restate(b)
        plane = BSC.OH * BSC.OW
        out = np.frombuffer(c.restate(a), np.uint8)
        k, source = out[-2 * plane:-plane], out[-plane:]
        assert k.max() == 3 and k.min() == 0 and set(source.tolist()) == set(BSC.IDS) | {255}


def test_the_pick_calls_check_their_arguments_without_a_gpu():
    L = lib.load()
    E, err = lib.DSIC_EINVAL, L.dsic_last_error
    a, b, m, d, v, c, s = 1 << 20, 1 << 21, 1 << 22, 1 << 24, 1 << 25, 1 << 26, 1 << 27   # non-null, aligned, far apart

    def call(name, src=(a, b), val=(None, m), rect=((0, 0, 8, 8), (2, 2, 6, 6)), nodata=(-1, -1), ids=None, n=None, C=3, dst=d,
             dv=v, dn=c, ds=s, oh=8, ow=8, mode=4, kind=2, ba=2, bb=0, fill=0, arrays=(True, True, True, True)):
        k = len(src)
        host = [(ctypes.c_void_p * k)(*src), (ctypes.c_void_p * k)(*val), (ctypes.c_int * (4 * k))(*[x for r in rect for x in r]),
                (ctypes.c_int * k)(*nodata)]
        host = [h if keep else None for h, keep in zip(host, arrays)]
        return getattr(L, "dsic_window_composite_pick_" + name)(
            *host, None if ids is None else (ctypes.c_int * k)(*ids), k if n is None else n, C, dst, dv, dn, ds, oh, ow, mode,
            kind, ba, bb, fill, None)

    for name, top, elem in (("u8", 255, 1), ("u16", 65535, 2)):
        # what the composite calls refuse
        assert call(name, n=0) == E and b"n=0" in err()
        assert err().decode().partition(": ")[0] == "window_composite_pick_" + name
        assert call(name, src=(a,) * 17, val=(None,) * 17, rect=((0, 0, 8, 8),) * 17, nodata=(-1,) * 17) == E and b"n=17" in err()
        for C in (0, 5):
            assert call(name, C=C) == E and f"C={C}".encode() in err()
        assert call(name, oh=0) == E and b"output" in err()
        assert call(name, oh=1 << 16, ow=1 << 15, dst=1 << 40, dv=1 << 44, dn=1 << 45, ds=1 << 46) == E and b"2^31" in err()
        for i in range(4):
            assert call(name, arrays=tuple(j != i for j in range(4))) == E and b"null" in err()
        assert call(name, src=(a, None)) == E and b"source 1" in err() and b"null" in err()
        assert call(name, dst=None) == E and b"null" in err()
        assert call(name, rect=((0, 0, 8, 8), (2, 2, 0, 6))) == E and b"rect 0x6" in err()
        assert call(name, rect=((0, 0, 8, 8), (2, 3, 6, 6))) == E and b"not inside the output" in err()
        assert call(name, fill=top + 1) == E and f"fill={top + 1}".encode() in err()
        assert call(name, nodata=(-1, top + 1)) == E and f"nodata={top + 1}".encode() in err()
        assert call(name, dst=a + 8 * 8 * 3 * elem - elem) == E and b"overlap" in err()
        assert call(name, dv=a + 16) == E and b"overlap" in err()
        assert call(name, dn=v + 63) == E and b"outputs overlap" in err()
        # and the refusals of their own: the mode, the index, the ids, the source plane
        for mode in (-1, 2, 3, 6):
            assert call(name, mode=mode) == E and f"mode={mode}".encode() in err() and b"4 max, 5 min" in err()
        for mode in (4, 5):
            for kind in (-1, 3):
                assert call(name, mode=mode, kind=kind) == E and f"kind={kind}".encode() in err()
            assert call(name, mode=mode, ba=3) == E and b"band 3 is outside 0..2" in err()
            assert call(name, mode=mode, bb=-1) == E and b"band -1 is outside 0..2" in err()
            assert call(name, mode=mode, kind=1, bb=3) == E and b"band 3" in err()
            assert call(name, mode=mode, kind=0, ba=3, bb=0) == E and b"band 3" in err()
        assert call(name, ids=(0, 255)) == E and b"source 1" in err() and b"id=255" in err()
        assert call(name, ids=(-1, 3)) == E and b"id=-1" in err()
        assert call(name, ds=a + 8 * 8 * 3 * elem - 1) == E and b"source 0 and an output overlap" in err()
        assert call(name, ds=m + 35) == E and b"source 1 and an output overlap" in err()
        assert call(name, ds=d + 8 * 8 * 3 * elem - 1) == E and b"outputs overlap" in err()
        assert call(name, ds=v + 63) == E and b"outputs overlap" in err()
        assert call(name, ds=c - 63) == E and b"outputs overlap" in err()
    assert call("u16", src=(a + 1, b)) == E and b"2-byte aligned" in err()
    assert call("u16", dst=d + 1) == E and b"2-byte aligned" in err()
    # the old exports keep their modes: 4 is refused there
    host = [(ctypes.c_void_p * 1)(a), (ctypes.c_void_p * 1)(None), (ctypes.c_int * 4)(0, 0, 8, 8), (ctypes.c_int * 1)(-1)]
    assert L.dsic_window_composite_u8(*host, 1, 3, d, v, c, 8, 8, 4, 0, None) == E and b"mode=4 (0 first, 1 last, 2 mean, 3 median)" in err()
