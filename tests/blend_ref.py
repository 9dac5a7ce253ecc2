"""Restatements of the overlapped tile grid and its seam blend, for the overlap tests (no tests here).

Geometry (per axis, L pixels, Lp = ceil16(L), t = min(tile, Lp), overlap O): one tile when Lp <= t; otherwise stride
s = t - O, n = ceil((Lp - O) / s) tiles, nominal origins a(i) = i*s, real origins o(i) = min(i*s, Lp - t), supports
[a(i), a(i+1) + O) and [a(n-1), Lp) for the last.  Weight of tile i at p: (2k+1)/(2O), k = p - a(i), over the first
O positions of the support when i > 0; (2(O-1-k)+1)/(2O), k = p - a(i+1), over [a(i+1), a(i+1)+O) when i < n-1; 1
elsewhere in the support; 0 outside it.

Blend arithmetic (float32, no fused multiply-add): rcp = 1.0f / (float)(2 O); a ramp weight is (float)(2k+1) * rcp; a
tile's weight w = wy * wx (a weight-1 axis contributes exactly 1.0f); its contribution w * clamp01(x); a pixel is the
left fold ((0 + c_a) + c_b) + ... over its contributing tiles in ascending tile number; the finish takes min(v, 1),
and uint8 output is (uint8)(v * 255.0f), truncating.

Error of the float32 fold against the exact value, u = 2^-24.  A term w*|x| carries these relative roundings: rcp
(once, but it enters wy and wx, so twice), the ramp multiply of each axis (two), the product wy * wx (one) and the
product with clamp01(x) (one): six.  The fold starts from 0, so 0 + c_a is exact and at most three additions follow;
the first term passes through all three.  Every term therefore carries at most nine factors (1 + d), |d| <= u, and
|float32 - exact| <= g9 * sum(w |x|) with g9 = 9u / (1 - 9u) (Higham's gamma_9).  That is below the 12 u the
feature's description allows for; BOUND_ROUNDINGS = 9 is what the tests assert.  The float64 evaluation that stands
for the exact value adds at most 2^-50 * sum(w |x|) of its own.
"""
from fractions import Fraction

import numpy as np

BOUND_ROUNDINGS = 9

# (tile, overlap, H, W): the cases of the GPU kernel test, each named for the way the kernel can go wrong
CASES = {
    "ramps_back_to_back": (32, 16, 70, 90),
    "last_row_shifted_last_column_not": (64, 16, 120, 200),
    "single_tile_column": (64, 32, 130, 64),
    "single_tile_row": (64, 16, 64, 300),
    "four_full_size_tiles": (256, 32, 300, 300),
}


def ceil16(n):
    return (n + 15) // 16 * 16


def valid_overlaps(tile):
    return list(range(16, tile // 2 + 1, 16))


def axis(L, tile, O):
    """One axis: dict Lp, t, s, n, a (nominal origins), o (real origins), sup (supports)."""
    Lp = ceil16(L)
    t = min(tile, Lp)
    if Lp <= t:
        return {"Lp": Lp, "t": t, "s": t, "n": 1, "a": [0], "o": [0], "sup": [(0, Lp)]}
    s = t - O
    n = -(-(Lp - O) // s)
    a = [i * s for i in range(n)]
    return {"Lp": Lp, "t": t, "s": s, "n": n, "a": a, "o": [min(v, Lp - t) for v in a],
            "sup": [(a[i], a[i + 1] + O) if i < n - 1 else (a[i], Lp) for i in range(n)]}


def _ramps(ax, O, up, down, one, zero, only=None):
    """[n][Lp] weights; up(k) / down(k) give the ramp values.  only: the tiles whose rows are wanted; the others' rows
    are left empty (an axis of thousands of tiles)."""
    out = []
    for i in range(ax["n"]):
        if only is not None and i not in only:
            out.append(None)
            continue
        lo, hi = ax["sup"][i]
        w = [zero] * ax["Lp"]
        for p in range(lo, hi):
            if i > 0 and p - ax["a"][i] < O:
                w[p] = up(p - ax["a"][i])
            elif i < ax["n"] - 1 and p >= ax["a"][i + 1]:
                w[p] = down(p - ax["a"][i + 1])
            else:
                w[p] = one
        out.append(w)
    return out


def weights_exact(ax, O):
    """[n][Lp] Fractions."""
    return _ramps(ax, O, lambda k: Fraction(2 * k + 1, 2 * O), lambda k: Fraction(2 * (O - 1 - k) + 1, 2 * O),
                  Fraction(1), Fraction(0))


def weights_f32(ax, O, only=None):
    """[n][Lp] float32, as the kernel computes them; with `only`, a dict of the rows of those tiles."""
    rcp = np.float32(1.0) / np.float32(2 * O) if O else np.float32(0)
    rows = _ramps(ax, O, lambda k: np.float32(2 * k + 1) * rcp, lambda k: np.float32(2 * (O - 1 - k) + 1) * rcp,
                  np.float32(1), np.float32(0), only)
    if only is not None:
        return {i: np.array(r, dtype=np.float32) for i, r in enumerate(rows) if r is not None}
    return np.array(rows, dtype=np.float32)


def weights_f64(ax, O):
    return np.array([[float(v) for v in row] for row in weights_exact(ax, O)], dtype=np.float64)


def grid(H, W, th, tw, O):
    """The two axes of an image whose tiles are th x tw (th = min(tile, ceil16(H)), likewise tw)."""
    ay, ax = axis(H, th, O), axis(W, tw, O)
    assert ay["t"] == th and ax["t"] == tw
    return ay, ax


def contributing(H, W, th, tw, O, y0, x0, h, w):
    """Brute force: the tiles with a non-zero weight on some pixel of the window, ascending."""
    ay, ax = grid(H, W, th, tw, O)
    rows = [i for i, (a, b) in enumerate(ay["sup"]) if any(y0 <= p < y0 + h for p in range(a, min(b, H)))]
    cols = [j for j, (a, b) in enumerate(ax["sup"]) if any(x0 <= p < x0 + w for p in range(a, min(b, W)))]
    return [i * ax["n"] + j for i in rows for j in cols]


def make_tiles(case, C, seed=0):
    """The GPU test's inputs: random tiles in [-0.2, 1.2], float32 [n][C][th][tw] (both clamps act)."""
    tile, O, H, W = CASES[case]
    ay, ax = axis(H, tile, O), axis(W, tile, O)
    rng = np.random.default_rng(1000 + seed + 7 * sorted(CASES).index(case))
    return rng.uniform(-0.2, 1.2, size=(ay["n"] * ax["n"], C, ay["t"], ax["t"])).astype(np.float32)


def _blend(batches, H, W, C, th, tw, O, wfun, dtype, rows=None):
    """rows = (y0, y1): only the rows [y0, y1) of the canvas, as [C][y1 - y0][W]; the weights of the listed tiles only"""
    ay, ax = grid(H, W, th, tw, O)
    y0, y1 = (0, H) if rows is None else rows
    if rows is None:
        wy, wx = wfun(ay, O), wfun(ax, O)
    else:
        ids = [t for batch in batches for t, _ in batch]
        wy, wx = wfun(ay, O, {t // ax["n"] for t in ids}), wfun(ax, O, {t % ax["n"] for t in ids})
    canvas = np.zeros((C, y1 - y0, W), dtype=dtype)
    mass = np.zeros((C, y1 - y0, W), dtype=dtype)
    last = -1
    for batch in batches:
        for t, x in batch:
            assert t > last, "tiles must arrive in ascending order"
            last = t
            i, j = divmod(t, ax["n"])
            (ya, yb), (xa, xb) = ay["sup"][i], ax["sup"][j]
            ya, yb, xb = max(ya, y0), min(yb, H, y1), min(xb, W)
            if ya >= yb:
                continue
            oy, ox = ay["o"][i], ax["o"][j]
            wgt = (wy[i][ya:yb, None] * wx[j][None, xa:xb]).astype(dtype)
            v = np.clip(np.asarray(x, dtype=np.float32)[:, ya - oy:yb - oy, xa - ox:xb - ox], 0, 1).astype(dtype)
            c = (wgt[None] * v).astype(dtype)
            canvas[:, ya - y0:yb - y0, xa:xb] = canvas[:, ya - y0:yb - y0, xa:xb] + c
            mass[:, ya - y0:yb - y0, xa:xb] += np.abs(c)
    return canvas, mass


def blend_f32(batches, H, W, C, th, tw, O, rows=None):
    """The float32 fold over batches (lists of (tile id, float32 [C][th][tw])), ascending: the unfinished canvas
    [C][H][W], or its rows [y0, y1) for rows = (y0, y1).  How the tiles are cut into batches does not enter: the fold
    runs in tile order."""
    return _blend(batches, H, W, C, th, tw, O, weights_f32, np.float32, rows)[0]


def blend_f64(batches, H, W, C, th, tw, O):
    """The same blend in float64 with exact-ratio weights -> (canvas, sum of w |x| per pixel)."""
    return _blend(batches, H, W, C, th, tw, O, weights_f64, np.float64)


def finish_f32(canvas):
    return np.minimum(canvas, np.float32(1)).astype(np.float32)


def finish_u8(canvas):
    """uint8 [H][W][C], truncating."""
    return (finish_f32(canvas) * np.float32(255.0)).astype(np.uint8).transpose(1, 2, 0).copy()


def error_bound(mass):
    u = 2.0 ** -24
    return (BOUND_ROUNDINGS * u / (1 - BOUND_ROUNDINGS * u) + 2.0 ** -50) * mass
