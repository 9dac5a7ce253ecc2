"""NumPy / pure-integer restatement of the gridded reads (csrc/grid.hip, codec.ImageReader.read_gridded, view.grid_level,
view.grid_window).  No tests here; test_grid_cpu.py holds the restatement to its own properties and to warp_ref on affine
meshes, test_gpu_grid.py holds the kernels and the reader to it.

A view of oh x ow pixels with the step S = 2^s carries a mesh G, int64 [nh + 1][nw + 1][2], nh = ceil(oh / S): node
(a, b) is the level-0 position (y, x) in Q16 of the output corner (a S, b S), or NONE in its y entry.  Pixel (i, j) lies
in cell (a, b) = (i >> s, j >> s) at fu = 2 (i - a S) + 1, fv = 2 (j - b S) + 1 and samples, per axis, the Q17 position
  P = ((2S - fu)(2S - fv) G[a][b] + (2S - fu) fv G[a][b+1] + fu (2S - fv) G[a+1][b] + fu fv G[a+1][b+1]) >> (2 s + 1);
a cell with a none node is fill and invalid.  After P everything is warp_ref's: `position` is the rule for one pixel in
Python's integers, `positions` the same over a view in int64, `sample` warp_ref.warp's sampler at given positions."""
from fractions import Fraction

import numpy as np

import warp_ref as R

NONE = -(1 << 63)
STEPS = (16, 32, 64)
MASKS = ("none", "valid", "nodata")


def shape(size, S):
    return -(-size[0] // S) + 1, -(-size[1] // S) + 1, 2


def position(G, S, i, j):
    """(Py, Px) of output pixel (i, j) in Python's integers, or None in a cell with a none node; also the largest
    |four-weight sum| met, for the bound"""
    s = S.bit_length() - 1
    a, b = i >> s, j >> s
    fu, fv = 2 * (i - a * S) + 1, 2 * (j - b * S) + 1
    nodes = [[int(v) for v in G[a + da, b + db]] for da in (0, 1) for db in (0, 1)]
    if any(n[0] == NONE for n in nodes):
        return None, 0
    w = [(2 * S - fu) * (2 * S - fv), (2 * S - fu) * fv, fu * (2 * S - fv), fu * fv]
    assert sum(w) == 1 << (2 * s + 2)
    sums = [sum(wk * n[x] for wk, n in zip(w, nodes)) for x in (0, 1)]
    return tuple(v >> (2 * s + 1) for v in sums), max(abs(v) for v in sums)


def rearranged_u64(G, S, i, j, x):
    """the rearranged form of one axis in arithmetic modulo 2^64, then the arithmetic shift of the wrapped sum"""
    s, M = S.bit_length() - 1, (1 << 64) - 1
    a, b = i >> s, j >> s
    fu, fv = 2 * (i - a * S) + 1, 2 * (j - b * S) + 1
    G00, G01, G10, G11 = (int(G[a + da, b + db, x]) & M for da in (0, 1) for db in (0, 1))
    total = ((4 * S * S * G00 & M) + (2 * S * fu * ((G10 - G00) & M) & M) + (2 * S * fv * ((G01 - G00) & M) & M)
             + (fu * fv * ((G00 - G10 - G01 + G11) & M) & M)) & M
    return (total - (1 << 64) if total >> 63 else total) >> (2 * s + 1)


def positions(G, S, size):
    """(Py, Px, whole) over the view in int64: whole is False in the cells with a none node (their P is 0)"""
    s = S.bit_length() - 1
    i = np.arange(size[0], dtype=np.int64)[:, None]
    j = np.arange(size[1], dtype=np.int64)[None, :]
    a, b = i >> s, j >> s
    fu, fv = 2 * (i - a * S) + 1, 2 * (j - b * S) + 1
    some = G[..., 0] != NONE
    whole = some[a, b] & some[a, b + 1] & some[a + 1, b] & some[a + 1, b + 1]
    Z = np.where(some[..., None], G, 0)
    out = []
    for x in (0, 1):
        total = ((2 * S - fu) * (2 * S - fv) * Z[a, b, x] + (2 * S - fu) * fv * Z[a, b + 1, x]
                 + fu * (2 * S - fv) * Z[a + 1, b, x] + fu * fv * Z[a + 1, b + 1, x])
        out.append(np.where(whole, total >> (2 * s + 1), 0))
    return out[0], out[1], whole


def sample(src, sval, sy0, sx0, l, LH, LW, H, W, Py, Px, whole, mode, nodata=None, fill=0):
    """warp_ref.warp's sampler at the positions (Py, Px) [oh][ow] (Q17) where `whole`: src uint8 / uint16 [sh][sw][C], the
    window of level l from its pixel (sy0, sx0); sval None or its validity bytes -> (image, valid bool).  Every tap of an
    inside pixel must lie inside the window."""
    oh, ow = Py.shape
    sh, sw, C = src.shape
    top = R.TOP[src.dtype]
    inside = whole & (Py >= 0) & (Py < H << 17) & (Px >= 0) & (Px < W << 17)
    out = np.full((oh, ow, C), fill, dtype=src.dtype)
    if not inside.any():
        return out, np.zeros((oh, ow), dtype=bool)
    if sval is not None:
        counts = np.asarray(sval) != 0
    elif nodata is not None:
        counts = ~(src == nodata).all(axis=2)
    else:
        counts = np.ones((sh, sw), dtype=bool)

    def window(idx, L, s0, sn):
        idx = np.clip(idx, 0, L - 1) - s0
        assert (idx[inside] >= 0).all() and (idx[inside] < sn).all(), "a tap outside the source window"
        return np.where(inside, idx, 0)

    if mode == 1:
        Y, X = window(Py >> (17 + l), LH, sy0, sh), window(Px >> (17 + l), LW, sx0, sw)
        out[inside] = src[Y, X][inside]
        return out, inside & (np.asarray(sval)[Y, X] != 0 if sval is not None else True)
    qy, qx = Py - (1 << (16 + l)), Px - (1 << (16 + l))
    Y0, X0 = qy >> (17 + l), qx >> (17 + l)
    py, px = (qy >> (10 + l)) & 127, (qx >> (10 + l)) & 127
    v = src.astype(np.int64)
    S, T = np.zeros((oh, ow, C), dtype=np.int64), np.zeros((oh, ow), dtype=np.int64)
    for ky, wy in enumerate((128 - py, py)):
        Y = window(Y0 + ky, LH, sy0, sh)
        for kx, wx in enumerate((128 - px, px)):
            X = window(X0 + kx, LW, sx0, sw)
            w = wy * wx * counts[Y, X]
            T += w
            S += w[:, :, None] * v[Y, X]
    ok = inside & (T > 0)
    res = (2 * S + T[:, :, None]) // np.maximum(2 * T, 1)[:, :, None]
    if mode == 2:
        wys, wxs = R.cubic_weights(py), R.cubic_weights(px)
        Sc, full = np.zeros((oh, ow, C), dtype=np.int64), inside.copy()
        for ky in range(4):
            Y = window(Y0 - 1 + ky, LH, sy0, sh)
            for kx in range(4):
                X = window(X0 - 1 + kx, LW, sx0, sw)
                full &= counts[Y, X]
                Sc += (wys[ky] * wxs[kx])[:, :, None] * v[Y, X]
        res = np.where(full[:, :, None], np.clip((Sc + (1 << 43)) >> 44, 0, top), res)
        ok = ok | full
    out[ok] = res[ok].astype(src.dtype)
    return out, ok


def gridded(src, sval, sy0, sx0, l, LH, LW, H, W, G, S, size, mode, nodata=None, fill=0):
    """the gridded read of a window: positions, then the sampler"""
    Py, Px, whole = positions(G, S, size)
    return sample(src, sval, sy0, sx0, l, LH, LW, H, W, Py, Px, whole, mode, nodata, fill)


def pixel(src, sval, sy0, sx0, l, LH, LW, H, W, G, S, i, j, mode, nodata=None, fill=0):
    """one output pixel in Python's integers -> (C values, valid): warp_ref.pixel at the mesh's position, which it takes
    as the view (Py, 0, 0, Px, 0, 0) of its pixel (0, 0)"""
    P, _ = position(G, S, i, j)
    if P is None:
        return [fill] * src.shape[2], False
    return R.pixel(src, sval, sy0, sx0, l, LH, LW, H, W, (P[0], 0, 0, P[1], 0, 0), 0, 0, mode, nodata, fill)[:2]


def whole_cells(G):
    some = G[..., 0] != NONE
    return some[:-1, :-1] & some[:-1, 1:] & some[1:, :-1] & some[1:, 1:]


def level(n_levels, G, S):
    """the largest l < n_levels with 4^l 2^32 S^2 <= min |E|^2 over the edges between nodes that are not none, in
    Python's integers; else 0"""
    nh1, nw1, _ = G.shape
    least = None
    for a in range(nh1):
        for b in range(nw1):
            for a2, b2 in ((a + 1, b), (a, b + 1)):
                if a2 < nh1 and b2 < nw1 and int(G[a, b, 0]) != NONE and int(G[a2, b2, 0]) != NONE:
                    e = (int(G[a2, b2, 0]) - int(G[a, b, 0])) ** 2 + (int(G[a2, b2, 1]) - int(G[a, b, 1])) ** 2
                    least = e if least is None else min(least, e)
    fit = [] if least is None else [l for l in range(n_levels) if 4 ** l * 2 ** 32 * S * S <= least]
    return max(fit) if fit else 0


def window(l, LH, LW, H, W, G, mode):
    """the box of the nodes of the whole cells, axis by axis through warp_ref's taps; None beside the image or without
    a whole cell"""
    cells = np.argwhere(whole_cells(G))
    if not len(cells):
        return None
    nodes = [[int(v) for v in G[a + da, b + db]] for a, b in cells for da in (0, 1) for db in (0, 1)]
    box = []
    for x, N, L in ((0, H, LH), (1, W, LW)):
        lo, hi = max(2 * min(n[x] for n in nodes), 0), min(2 * max(n[x] for n in nodes), (N << 17) - 1)
        if lo > hi:
            return None
        taps = R.axis_taps(lo, l, L, mode) + R.axis_taps(hi, l, L, mode)
        box.append((min(Y for Y, _ in taps), max(Y for Y, _ in taps)))
    (ya, yb), (xa, xb) = box
    return ya, xa, yb - ya + 1, xb - xa + 1


def brute_window(l, LH, LW, H, W, G, S, size, mode):
    """the box of every tap of every inside pixel, pixel by pixel; None without an inside pixel"""
    ys, xs = [], []
    for i in range(size[0]):
        for j in range(size[1]):
            P, _ = position(G, S, i, j)
            if P is not None and 0 <= P[0] < H << 17 and 0 <= P[1] < W << 17:
                ys += [Y for Y, _ in R.axis_taps(P[0], l, LH, mode)]
                xs += [X for X, _ in R.axis_taps(P[1], l, LW, mode)]
    return (min(ys), min(xs), max(ys) - min(ys) + 1, max(xs) - min(xs) + 1) if ys else None


# ---- meshes -----------------------------------------------------------------------------------------------------------
def affine(m, size, S):
    """the mesh of the Q16 matrix m, in Python's integers"""
    nh1, nw1, _ = shape(size, S)
    return np.array([[[m[0] * a * S + m[1] * b * S + m[2], m[3] * a * S + m[4] * b * S + m[5]] for b in range(nw1)]
                     for a in range(nh1)], dtype=np.int64)


def round_half_even(q):
    n, r = divmod(q.numerator, q.denominator)
    return n + (1 if 2 * r > q.denominator or (2 * r == q.denominator and n & 1) else 0)


def projective(h, size, S):
    """(y', x', w') = h (i, j, 1) at the nodes in exact fractions of the float64 entries, rounded once half to even to
    Q16; w' <= 0: none"""
    nh1, nw1, _ = shape(size, S)
    h = [[Fraction(v) for v in row] for row in h]
    G = np.zeros((nh1, nw1, 2), dtype=np.int64)
    for a in range(nh1):
        for b in range(nw1):
            py, px, w = (r[0] * a * S + r[1] * b * S + r[2] for r in h)
            G[a, b] = (NONE, 0) if w <= 0 else (round_half_even(py / w * 65536), round_half_even(px / w * 65536))
    return G


def projective_h(H, W, oh, ow):
    """a tilted view of all of an H x W image at oh x ow: the far edge a third shorter"""
    return [[0.9 * H / oh, 0.1 * H / ow, 0.02 * H], [0.05 * W / oh, 0.95 * W / ow, 0.01 * W], [0.3 / oh, 0.2 / ow, 1.0]]


MESHES = ["affine", "projective", "bulge", "jitter", "fold", "overhang", "holes"]


def mesh_function(kind, H, W, oh, ow):
    """the smooth map of a mesh kind: fn(i, j) over float64 output corner coordinates -> (y, x) in level-0 pixels"""
    def bulge(i, j):                                   # a radial quadratic about the view's centre
        di, dj = (i - oh / 2) / oh, (j - ow / 2) / ow
        f = 0.8 + 0.6 * (di * di + dj * dj)
        return H / 2 + H * di * f, W / 2 + W * dj * f

    def fold(i, j):                                    # not monotone on either axis: the view doubles back on itself
        u, v = i / oh, j / ow
        return H * (0.5 - 0.45 * np.cos(2.5 * np.pi * u)) + 0 * v, W * (0.5 + 0.45 * np.sin(2 * np.pi * v + u))

    def overhang(i, j):                                # a fifth of the view on every side lies outside the image
        u, v = i / oh, j / ow
        return -0.2 * H + 1.4 * H * u + 0.1 * H * np.sin(3 * v), -0.15 * W + 1.3 * W * v + 0 * u

    def sheared(i, j):
        u, v = i / oh, j / ow
        return 0.9 * H * u + 0.05 * H * v + 0.01 * H, 0.9 * W * v + 0.05 * W * u + 0.02 * W
    return {"bulge": bulge, "fold": fold, "overhang": overhang, "jitter": sheared, "holes": sheared}[kind]


def mesh(kind, H, W, size, S, matrix="rot30"):
    """the mesh of a kind for a view of `size` of an H x W image.  affine: warp_ref's named matrix; jitter: every node
    moved on its own by up to 0.3 of a cell's extent, so that a cell must use its own four nodes; holes: about a
    quarter of the nodes none"""
    oh, ow = size
    if kind == "affine":
        return affine(R.matrix(matrix, H, W, oh, ow), size, S)
    if kind == "projective":
        return projective(projective_h(H, W, oh, ow), size, S)
    nh1, nw1, _ = shape(size, S)
    i, j = np.broadcast_arrays(np.arange(nh1, dtype=np.float64)[:, None] * S, np.arange(nw1, dtype=np.float64)[None, :] * S)
    y, x = mesh_function(kind, H, W, oh, ow)(i, j)
    rng = np.random.default_rng([oh, ow, S, H, W])
    if kind == "jitter":
        y = y + rng.uniform(-0.3, 0.3, y.shape) * H * S / oh
        x = x + rng.uniform(-0.3, 0.3, x.shape) * W * S / ow
    G = np.stack([np.rint(y * 65536), np.rint(x * 65536)], axis=-1).astype(np.int64)
    if kind == "holes":
        G[rng.random((nh1, nw1)) < 0.25, 0] = NONE
    return G


# ---- the kernel sweep of test_gpu_grid.py; test_grid_cpu.py checks its coverage too -------------------------------------
def sweep(si, ki, k):
    """The thinned product: per (source size, kind, mesh kind) one shift, output size, mask, window margin, step and,
    for the affine mesh, matrix; all three modes run under it."""
    turn = si + ki + k
    return (R.SHIFTS[turn % 3], R.OUT_SIZES[(2 * si + ki + k) % 5], MASKS[(si + ki // 3 + k // 3 + k) % 3], (turn // 2) % 2,
            STEPS[(si + 2 * ki + 2 * k) % 3], R.MATRICES[(5 * si + 2 * ki) % len(R.MATRICES)])


def kernel_case(src_size, out_size, l, kind, S, mode, margin=0, matrix="rot30"):
    """One kernel call: the level-0 size, the mesh and the planned source window, `margin` level pixels wider where the
    level has room; a view without an inside pixel gets the level's first pixel as its window."""
    (LH, LW), (oh, ow) = src_size, out_size
    H, W = R.image_size(LH, l), R.image_size(LW, l)
    G = mesh(kind, H, W, out_size, S, matrix)
    win = window(l, LH, LW, H, W, G, mode) or (0, 0, 1, 1)
    ya, xa = max(win[0] - margin, 0), max(win[1] - margin, 0)
    yb, xb = min(win[0] + win[2] + margin, LH), min(win[1] + win[3] + margin, LW)
    return {"H": H, "W": W, "LH": LH, "LW": LW, "shift": l, "G": G, "step": S, "size": (oh, ow), "sy0": ya, "sx0": xa,
            "sh": yb - ya, "sw": xb - xa}


def run_case(img, val, c, mode, nodata=None, fill=0):
    """the restatement on a kernel case: the window is cut from the level here"""
    ys, xs = slice(c["sy0"], c["sy0"] + c["sh"]), slice(c["sx0"], c["sx0"] + c["sw"])
    return gridded(img[ys, xs], None if val is None else val[ys, xs], c["sy0"], c["sx0"], c["shift"], c["LH"], c["LW"],
                   c["H"], c["W"], c["G"], c["step"], c["size"], mode, nodata, fill)
