"""The NumPy restatement of dsic_window_warp_composite_u8 / _u16 (include/dsic_hip.h) and the cases
test_gpu_warp_stack.py runs (kept here so that a test without a GPU can hold them).

The export is defined as a chain of older exports, and the restatement is literally that chain over their restatements:
warp_ref.warp per source, which gives an image S_i and a validity V_i of the output's size, then composite_ref.composite
(first, last, mean, median) or best_pixel_ref.pick (max, min, and whenever a source plane is asked for) over the pairs
(S_i, V_i), each with the full rect (0, 0, oh, ow), the source's nodata value and the ids."""
import numpy as np

import best_pixel_ref as BP
import composite_ref as X
import warp_ref as R

FIRST, LAST, MEAN, MEDIAN, MAX, MIN = 0, 1, 2, 3, 4, 5
REDUCES = {"first": FIRST, "last": LAST, "mean": MEAN, "median": MEDIAN, "max": MAX, "min": MIN}


def warp_composite(sources, C, size, sample_mode, reduce, index, fill, ids, warp_fill=0):
    """sources: dicts with src (the window [sh][sw][C] of level `shift` from its pixel (sy0, sx0)), val (None or its
    validity bytes), sy0, sx0, shift, LH, LW, H, W, m (Q16) and nodata (-1: none); reduce: 0 .. 5 as DSIC_COMPOSITE_*;
    index: as best_pixel_ref.pick takes it (looked at for max and min); ids: None or one per source.  warp_fill is the
    `any fill` of step 1: the result must not depend on it.
    -> (dst [oh][ow][C], valid uint8, count uint8, source uint8 or, for mean and median, None)"""
    oh, ow = size
    imgs, vals = [], []
    for s in sources:
        tap_nodata = None if s["val"] is not None or s["nodata"] < 0 else s["nodata"]      # src_valid: nodata ignored there
        img, ok = R.warp(s["src"], s["val"], s["sy0"], s["sx0"], s["shift"], s["LH"], s["LW"], s["H"], s["W"], s["m"], size,
                         sample_mode, tap_nodata, warp_fill)
        imgs.append(img)
        vals.append(ok.astype(np.uint8))
    rects, nodata = [(0, 0, oh, ow)] * len(sources), [s["nodata"] for s in sources]
    if reduce in (MEAN, MEDIAN):
        return tuple(X.composite(imgs, vals, rects, nodata, C, oh, ow, reduce, fill)) + (None,)
    return BP.pick(imgs, vals, rects, nodata, ids, C, oh, ow, reduce, index, fill)


# ---- the cases ------------------------------------------------------------------------------------------------------
KINDS = R.KINDS                                                  # u8 with C = 3, 4 and u16 with C = 1 .. 4
SIZES = [(1, 1), (7, 9), (17, 33), (33, 130)]    # one pixel, inside one patch, partial patches and a second workgroup, more
NS = [1, 4, 5, 8, 9, 16]                                         # both sides of the median's lists of 4, 8 and 16
INDEX_KINDS = BP.INDEX_KINDS
NODATA = {"u8": 7, "u16": 300}
# (view, what marks a pixel invalid, shift): the five named views of warp_ref.MATRICES, a source entirely beside the
# output, and small patches in the lower half for the sources that are valid wherever they are inside
LIST = [("rot30", "valid", 0), ("mirror", "nodata", 1), ("beside", "none", 2), ("magnify3", "valid", 1),
        ("minify2.5", "nodata", 2), ("overhang", "valid", 0), ("patch", "none", 1), ("rot30", "nodata", 2),
        ("mirror", "valid", 0), ("patch", "none", 2), ("magnify3", "nodata", 1), ("overhang", "nodata", 0),
        ("patch", "none", 0), ("minify2.5", "valid", 2), ("magnify3", "valid", 1), ("mirror", "nodata", 0)]
assert len(LIST) == max(NS)


def _matrix(view, i, H, W, oh, ow):
    if view == "beside":                                         # every position above the image
        return R.q16([[1, 0, -(oh + 10)], [0, 1, 0.25]])
    if view == "patch":                                          # the whole image on 6 x 12 output pixels, a place per source
        a, b, y, x = H / 6, W / 12, min(oh // 2 + 2 * (i % 4), max(0, oh - 6)), (10 + 17 * i) % max(1, ow - 12)
        return R.q16([[a, 0, -a * y], [0, b, -b * x]])
    return R.matrix(view, H, W, oh, ow)


def _owned(i, n, y, x, oh, ow):
    """where source i of n is meant to count, in output coordinates: everywhere in the top quarter, with its two
    neighbours-to-be in the second quarter of its stripe, alone in the lower half of its stripe"""
    stripe = np.floor(x * n / ow).astype(np.int64)
    mine = stripe == i
    shared = (stripe == (i + 1) % n) | (stripe == (i + 3) % n) | mine
    return (y < oh / 4) | (shared & (y < oh / 2)) | mine


def sources(kind, C, size, n, sample_mode, seed=0):
    """The first n entries of LIST as sources of a size[0] x size[1] output: random pixels; per source a validity
    window, a nodata value or neither; the planned source window, a level pixel wider for every other source; in the
    first source a block of zeros that counts (A + B = 0 for a normalised difference)."""
    oh, ow = size
    dtype, top = X.DTYPES[kind], X.TOP[kind]
    out = []
    for i, (view, marks, l) in enumerate(LIST[:n]):
        rng = np.random.default_rng(1000 * seed + 16 * len(out) + 7 * C + (kind == "u16"))
        LH, LW = (5 + i % 3, 7 + i % 2) if view == "patch" else (24 + i, 40 + 2 * i)
        H, W = R.image_size(LH, l), R.image_size(LW, l)
        m = _matrix(view, i, H, W, oh, ow)
        img = rng.integers(0, top + 1, (LH, LW, C)).astype(dtype)
        # the output position of every level pixel's centre, through the inverse of the matrix in floating point: the
        # inputs may be made by any means
        a = np.array([[m[0], m[1]], [m[3], m[4]]], dtype=np.float64) / 65536
        inv = np.linalg.inv(a)
        py = (np.arange(LH) + 0.5)[:, None] * (1 << l) - m[2] / 65536
        px = (np.arange(LW) + 0.5)[None, :] * (1 << l) - m[5] / 65536
        y, x = inv[0, 0] * py + inv[0, 1] * px, inv[1, 0] * py + inv[1, 1] * px
        own = _owned(i, n, y, x, oh, ow)
        if i == 0:
            zero = (y >= oh / 8) & (y < oh / 4) & (x >= ow / 4) & (x < ow / 2)
            img[zero] = 0
        val, nodata = None, -1
        if marks == "valid":
            val = own.astype(np.uint8) * rng.integers(1, 256, (LH, LW)).astype(np.uint8)
        elif marks == "nodata":
            nodata = NODATA[kind]
            img[~own] = nodata
        win = R.warp_window(l, LH, LW, H, W, m, oh, ow, sample_mode) or (0, 0, 1, 1)
        margin = i % 2
        ya, xa = max(win[0] - margin, 0), max(win[1] - margin, 0)
        yb, xb = min(win[0] + win[2] + margin, LH), min(win[1] + win[3] + margin, LW)
        out.append({"src": np.ascontiguousarray(img[ya:yb, xa:xb]), "val": None if val is None else np.ascontiguousarray(val[ya:yb, xa:xb]),
                    "sy0": ya, "sx0": xa, "sh": yb - ya, "sw": xb - xa, "shift": l, "LH": LH, "LW": LW, "H": H, "W": W, "m": m,
                    "nodata": nodata, "meets": R.warp_window(l, LH, LW, H, W, m, oh, ow, sample_mode) is not None})
    return out


def case_ids(n):
    return BP.case_ids(n)


def sweep(ki, si):
    """The cases of (kind, size), one per n: sample mode, reduce, index, fill, the three optional outputs and the ids take
    turns so that over the kinds and sizes every n meets every reduce under every sample mode."""
    kind, C = KINDS[ki]
    q = ki * len(SIZES) + si
    cases = []
    for ni, n in enumerate(NS):
        t = q * len(NS) + ni
        a = t % C
        b = (a + 1 + (t // C) % max(1, C - 1)) % C
        ikind = INDEX_KINDS[(2 * ni + si + ki) % 3]
        reduce = (q + ni) % 6
        wants = (ni + 3 * si + 5 * ki) % 8
        cases.append(dict(n=n, sample=(q + 2 * ni + q // 6) % 3, reduce=reduce,
                          index=(ikind, a) if ikind == "band" else (ikind, a, b), fill=X.TOP[kind] * ((t // 2 + ni) % 2),
                          want_valid=bool(wants & 1), want_count=bool(wants & 2),
                          want_source=bool(wants & 4) and reduce not in (MEAN, MEDIAN), ids=bool((ni // 2 + si + ki) % 2),
                          offset=(t // 3) % 2))
    return cases


def case_sources(kind, C, size, case):
    return sources(kind, C, size, case["n"], case["sample"])


def restate(kind, C, size, case, srcs=None):
    srcs = case_sources(kind, C, size, case) if srcs is None else srcs
    ids = case_ids(case["n"]) if case["ids"] else None
    return warp_composite(srcs, C, size, case["sample"], case["reduce"], case["index"], case["fill"], ids)
