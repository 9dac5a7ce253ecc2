"""The NumPy restatement of dsic_window_composite_pick_u8 / _u16 (include/dsic_hip.h), written from the definition, and
the sweep test_gpu_best_pixel.py runs (kept here so that a test without a GPU can hold it).

The candidates of an output pixel are composite_ref's: the sources, in list order, whose rect holds the pixel, whose
validity byte is not 0 there and whose pixel is not all-nodata.  For max and min a candidate must also have a defined
index: u = index_ref.index_value of its bands a and b, and an nd candidate with A + B = 0 is not a candidate.  With k
candidates: max / min = the whole pixel of the candidate with the largest / smallest u, among equals the first in list
order; first / last = the whole pixel of the first / last candidate; k = 0 = fill.  Beside the image: valid (k > 0),
count (k) and source, the id of the winning source (its position where no ids are given) and 255 where k = 0."""
import numpy as np

import composite_ref as X
import index_ref

FIRST, LAST, MAX, MIN = 0, 1, 4, 5
MODES = {"first": FIRST, "last": LAST, "max": MAX, "min": MIN}
NO_SOURCE = 255


def candidates(srcs, valids, rects, nodata, C, oh, ow):
    """composite_ref's candidate rule -> (vals int64 [n][oh][ow][C], cand bool [n][oh][ow])"""
    n = len(srcs)
    assert n == len(valids) == len(rects) == len(nodata) and n >= 1
    vals = np.zeros((n, oh, ow, C), dtype=np.int64)
    cand = np.zeros((n, oh, ow), dtype=bool)
    for i in range(n):
        dy, dx, h, w = rects[i]
        assert h >= 1 and w >= 1 and dy >= 0 and dx >= 0 and dy + h <= oh and dx + w <= ow
        px = np.asarray(srcs[i]).reshape(h, w, C).astype(np.int64)
        ok = np.ones((h, w), dtype=bool) if valids[i] is None else np.asarray(valids[i]).reshape(h, w) != 0
        if nodata[i] >= 0:
            ok = ok & ~(px == nodata[i]).all(axis=2)
        vals[i, dy:dy + h, dx:dx + w] = px
        cand[i, dy:dy + h, dx:dx + w] = ok
    return vals, cand


def _pick(srcs, valids, rects, nodata, ids, C, oh, ow, mode, index, fill, ties_to_last=False, rank=None, keep_undefined=False):
    """pick, and its mutants for test_best_pixel_cpu.py: ties_to_last breaks ties towards the last candidate, rank
    replaces the index (a function of the samples A and B), keep_undefined keeps candidates whose index is not defined"""
    n, dtype = len(srcs), np.asarray(srcs[0]).dtype
    vals, cand = candidates(srcs, valids, rects, nodata, C, oh, ow)
    if mode in (MAX, MIN):
        kind, a, b = index_ref.parse(index)
        u, defined = index_ref.index_value(vals.astype(dtype), kind, a, b)
        if rank is not None:
            u = rank(vals[..., a], vals[..., b])
        if not keep_undefined:
            cand = cand & defined
        key = np.where(cand, u if mode == MAX else -u, np.iinfo(np.int64).min)      # the winner has the largest key
    else:
        assert mode in (FIRST, LAST)
        t = np.arange(n, dtype=np.int64)[:, None, None]
        key = np.where(cand, -t if mode == FIRST else t, np.iinfo(np.int64).min)
    winner = n - 1 - np.argmax(key[::-1], axis=0) if ties_to_last else np.argmax(key, axis=0)   # argmax: the first of equals
    k = cand.sum(axis=0)
    ids = np.arange(n) if ids is None else np.asarray(ids)
    assert ids.shape == (n,) and ids.min() >= 0 and ids.max() < NO_SOURCE
    dst = np.where(k[..., None] > 0, np.take_along_axis(vals, winner[None, ..., None], axis=0)[0], fill)
    source = np.where(k > 0, ids[winner], NO_SOURCE)
    return dst.astype(dtype), (k > 0).astype(np.uint8), k.astype(np.uint8), source.astype(np.uint8)


def pick(srcs, valids, rects, nodata, ids, C, oh, ow, mode, index, fill):
    """srcs, valids, rects, nodata as composite_ref.composite takes them; ids: None or n values in 0 .. 254; mode: FIRST,
    LAST, MAX or MIN; index: ("nd", a, b), ("difference", a, b) or ("band", a), not looked at for FIRST and LAST
    -> (dst [oh][ow][C] of the sources' dtype, valid uint8 [oh][ow], count uint8 [oh][ow], source uint8 [oh][ow])"""
    return _pick(srcs, valids, rects, nodata, ids, C, oh, ow, mode, index, fill)


# ---- the sweep of the kernel test, over composite_ref's axes --------------------------------------------------------
KINDS, NS, LAYOUTS, VALIDITY, SIZES = X.KINDS, X.NS, X.LAYOUTS, X.VALIDITY, X.SIZES
assert SIZES == [(1, 1), (3, 5), (33, 130), (70, 1030)]    # one pixel, less than a wave, a ragged last workgroup in
MODE_TURNS = (MAX, FIRST, MIN, LAST)                       # both directions, more than one block row
INDEX_KINDS = ("nd", "difference", "band")


def case_ids(n):
    """n distinct ids, 254 and 0 among them once n >= 2, none equal to its position"""
    ids = [254] + [(37 * i + 11) % 254 for i in range(1, n - 1)] + [0] * (n > 1)
    assert len(set(ids)) == n and all(v != i for i, v in enumerate(ids))
    return ids


def sweep(ki, si):
    """The cases of (kind, size): one per n, with mode, index, layout, validity, fill, the three optional outputs and
    the ids taking turns.  The ladder goes with the full layout and a count, as in composite_ref.sweep.  low: uint8
    samples drawn from 0 .. 7, so that equal indices and A + B = 0 are frequent."""
    kind, C = KINDS[ki]
    cases = []
    for ni, n in enumerate(NS):
        t = (ki * len(SIZES) + si) * len(NS) + ni
        validity = VALIDITY[(ki + 2 * si + ni) % 4]
        ladder = validity == "ladder"
        a = t % C
        b = (a + 1 + (t // C) % max(1, C - 1)) % C
        ikind = INDEX_KINDS[(2 * ni + si + ki) % 3]
        wants = (ni + 3 * si + 5 * ki) % 8
        cases.append(dict(n=n, mode=MODE_TURNS[(ni + si + ki) % 4], index=(ikind, a) if ikind == "band" else (ikind, a, b),
                          layout="full" if ladder else LAYOUTS[(ki + 2 * si + ni) % 5], validity=validity,
                          fill=X.TOP[kind] * ((t // 2 + ni) % 2), want_valid=bool(wants & 1), want_count=ladder or bool(wants & 2),
                          want_source=bool(wants & 4), ids=bool((ni // 2 + si + ki) % 2), offset=(t // 3) % 2,
                          low=kind == "u8" and t % 3 != 1))
    return cases


def case_inputs(kind, C, oh, ow, case):
    """(srcs, valids, rects, nodata, ids) of a sweep case: composite_ref.case_inputs', a low case folded into 0 .. 7
    (composite_ref's uint8 nodata value is 7: a nodata pixel stays one), and in the second source a block of zeros"""
    srcs, masks, rects, nodata = X.case_inputs(kind, C, oh, ow, dict(case, mode=MODE_TURNS.index(case["mode"])))
    if case["low"]:
        srcs = [s & np.uint8(7) for s in srcs]
    if case["n"] > 1:
        h, w = rects[1][2:]
        srcs[1][h // 3:h // 3 + max(1, h // 4), w // 3:w // 3 + max(1, w // 4)] = 0
    return srcs, masks, rects, nodata, case_ids(case["n"]) if case["ids"] else None
