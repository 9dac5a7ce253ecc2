"""NumPy / pure-integer restatement of the warped reads (csrc/warp.hip, codec.ImageReader.read_warped / render_warped,
codec.affine_q16, view.warp_level, view.warp_window).  No tests here; test_warp_cpu.py holds the restatement to its own
properties and to float64, test_gpu_warp.py holds the kernels and the reader to it.

A view is six Q16 integers m (row, column order).  Output pixel (i, j) samples the level-0 position P / 2^17,
  Py = m0 (2 i + 1) + m1 (2 j + 1) + 2 m2,  Px = m3 (2 i + 1) + m4 (2 j + 1) + 2 m5,
inside iff 0 <= Py < H 2^17 and 0 <= Px < W 2^17; outside: fill, invalid.  At level l (LH x LW), taps clamped to it:
  nearest:  pixel (min(Py >> (17 + l), LH - 1), ...), a copy of pixel and validity
  q = P - 2^(16+l), Y0 = q >> (17 + l), p = (q >> (10 + l)) & 127
  bilinear: taps Y0, Y0 + 1, weights (128 - p, p) per axis, (2 S + T) // (2 T) over the taps that count; T = 0: fill
  cubic:    taps Y0 - 1 .. Y0 + 2, Keys a = -1/2 scaled by 2^22 per axis; all 16 taps count:
            clamp((S + 2^43) >> 44, 0, top); else the bilinear pixel
A tap counts iff its validity byte is not 0 (a validity window), else iff its channels do not all equal nodata, else
always.  `pixel` is the rule for one output pixel in Python's integers; `warp` is the same over a whole view in int64,
which holds S (|S| < 2^61, asserted in test_warp_cpu.py) - the two are held equal there."""
import math

import numpy as np

import view_ref

MODES = {"bilinear": 0, "nearest": 1, "cubic": 2}
TOP = {np.dtype(np.uint8): 255, np.dtype(np.uint16): 65535}


def q16(matrix):
    return tuple(int(round(v * 65536)) for row in matrix for v in row)


def level_size(n, l):
    return -(-n // (1 << l))


def position(m3, i, j):
    return m3[0] * (2 * i + 1) + m3[1] * (2 * j + 1) + 2 * m3[2]


def cubic_weights(p):
    return [-p ** 3 + 256 * p ** 2 - 16384 * p, 3 * p ** 3 - 640 * p ** 2 + 2 ** 22,
            -3 * p ** 3 + 512 * p ** 2 + 16384 * p, p ** 3 - 128 * p ** 2]


def axis_taps(P, l, L, mode):
    """one axis of one inside sample -> [(clamped level index, weight)]: 1 tap (nearest), 2 or 4"""
    if mode == 1:
        return [(min(P >> (17 + l), L - 1), 1)]
    q = P - (1 << (16 + l))
    Y0, p = q >> (17 + l), (q >> (10 + l)) & 127
    if mode == 0:
        return [(min(max(Y0 + k, 0), L - 1), w) for k, w in enumerate((128 - p, p))]
    return [(min(max(Y0 - 1 + k, 0), L - 1), w) for k, w in enumerate(cubic_weights(p))]


def _counts(src, sval, nodata, Y, X):
    if sval is not None:
        return bool(sval[Y, X] != 0)
    return nodata is None or not bool((src[Y, X] == nodata).all())


def pixel(src, sval, sy0, sx0, l, LH, LW, H, W, m, i, j, mode, nodata=None, fill=0):
    """One output pixel in Python's integers -> (list of C values, valid, the largest |S| met in the cubic sum)."""
    C, top = src.shape[2], TOP[src.dtype]
    Py, Px = position(m[:3], i, j), position(m[3:], i, j)
    if not (0 <= Py < H << 17 and 0 <= Px < W << 17):
        return [fill] * C, False, 0
    if mode == 1:
        Y, X = axis_taps(Py, l, LH, 1)[0][0] - sy0, axis_taps(Px, l, LW, 1)[0][0] - sx0
        return [int(v) for v in src[Y, X]], True if sval is None else bool(sval[Y, X] != 0), 0
    big = 0
    if mode == 2:
        ty, tx = axis_taps(Py, l, LH, 2), axis_taps(Px, l, LW, 2)
        if all(_counts(src, sval, nodata, Y - sy0, X - sx0) for Y, _ in ty for X, _ in tx):
            out = []
            for c in range(C):
                S = sum(wy * wx * int(src[Y - sy0, X - sx0, c]) for Y, wy in ty for X, wx in tx)
                big = max(big, abs(S), sum(abs(wy * wx) * int(src[Y - sy0, X - sx0, c]) for Y, wy in ty for X, wx in tx))
                out.append(min(max((S + (1 << 43)) >> 44, 0), top))
            return out, True, big
    ty, tx = axis_taps(Py, l, LH, 0), axis_taps(Px, l, LW, 0)
    live = [(Y - sy0, X - sx0, wy * wx) for Y, wy in ty for X, wx in tx if _counts(src, sval, nodata, Y - sy0, X - sx0)]
    T = sum(w for _, _, w in live)
    if T == 0:
        return [fill] * C, False, big
    return [(2 * sum(w * int(src[Y, X, c]) for Y, X, w in live) + T) // (2 * T) for c in range(C)], True, big


def warp(src, sval, sy0, sx0, l, LH, LW, H, W, m, size, mode, nodata=None, fill=0):
    """src: uint8 / uint16 [sh][sw][C], the window of level l from its pixel (sy0, sx0); sval: None or its validity
    bytes [sh][sw] -> (image [oh][ow][C], valid bool [oh][ow]).  Every tap must lie inside the window."""
    oh, ow = size
    sh, sw, C = src.shape
    top = TOP[src.dtype]
    i = np.arange(oh, dtype=np.int64)[:, None]
    j = np.arange(ow, dtype=np.int64)[None, :]
    Py = m[0] * (2 * i + 1) + m[1] * (2 * j + 1) + 2 * m[2]
    Px = m[3] * (2 * i + 1) + m[4] * (2 * j + 1) + 2 * m[5]
    inside = (Py >= 0) & (Py < H << 17) & (Px >= 0) & (Px < W << 17)
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
        wys, wxs = cubic_weights(py), cubic_weights(px)
        Sc, full = np.zeros((oh, ow, C), dtype=np.int64), inside.copy()
        for ky in range(4):
            Y = window(Y0 - 1 + ky, LH, sy0, sh)
            for kx in range(4):
                X = window(X0 - 1 + kx, LW, sx0, sw)
                full &= counts[Y, X]
                Sc += (wys[ky] * wxs[kx])[:, :, None] * v[Y, X]
        cubic = np.clip((Sc + (1 << 43)) >> 44, 0, top)
        res = np.where(full[:, :, None], cubic, res)
        ok = ok | full
    out[ok] = res[ok].astype(src.dtype)
    return out, ok


def warp_level(n_levels, m):
    step = min(m[0] ** 2 + m[3] ** 2, m[1] ** 2 + m[4] ** 2)
    fit = [l for l in range(n_levels) if 4 ** l * 2 ** 32 <= step]
    return max(fit) if fit else 0


def warp_window(l, LH, LW, H, W, m, oh, ow, mode):
    """the corner rule, axis by axis; None when the corners' bounding box misses the image"""
    box = []
    for m3, N, L in ((m[:3], H, LH), (m[3:], W, LW)):
        P = [position(m3, i, j) for i in (0, oh - 1) for j in (0, ow - 1)]
        lo, hi = max(min(P), 0), min(max(P), (N << 17) - 1)
        if lo > hi:
            return None
        taps = axis_taps(lo, l, L, mode) + axis_taps(hi, l, L, mode)
        box.append((min(Y for Y, _ in taps), max(Y for Y, _ in taps)))
    (ya, yb), (xa, xb) = box
    return ya, xa, yb - ya + 1, xb - xa + 1


def brute_window(l, LH, LW, H, W, m, oh, ow, mode):
    """the box of every tap of every inside pixel, pixel by pixel; None without an inside pixel"""
    ys, xs = [], []
    for i in range(oh):
        for j in range(ow):
            Py, Px = position(m[:3], i, j), position(m[3:], i, j)
            if 0 <= Py < H << 17 and 0 <= Px < W << 17:
                ys += [Y for Y, _ in axis_taps(Py, l, LH, mode)]
                xs += [X for X, _ in axis_taps(Px, l, LW, mode)]
    return (min(ys), min(xs), max(ys) - min(ys) + 1, max(xs) - min(xs) + 1) if ys else None


def rotation(cy, cx, degrees, scale, oh, ow):
    c, s = {0: (1, 0), 90: (0, 1), 180: (-1, 0), 270: (0, -1)}.get(
        degrees % 360, (math.cos(math.radians(degrees)), math.sin(math.radians(degrees))))
    a, b = scale * c, scale * s
    return [[a, b, cy - (a * oh + b * ow) / 2], [-b, a, cx - (-b * oh + a * ow) / 2]]


# ---- float64 anchors --------------------------------------------------------------------------------------------------
def float_pixel(src, l, LH, LW, m, i, j, mode):
    """float64 bilinear (mode 0) or Keys cubic (mode 2) interpolation of a whole level `src` at the truncated phases
    p / 128, edge replicated; cubic not clamped -> C float64 values"""
    def taps(P, L):
        q = P - (1 << (16 + l))
        Y0, t = q >> (17 + l), ((q >> (10 + l)) & 127) / 128.0
        if mode == 0:
            ws, first = [1 - t, t], Y0
        else:
            ws = [-0.5 * t ** 3 + t ** 2 - 0.5 * t, 1.5 * t ** 3 - 2.5 * t ** 2 + 1, -1.5 * t ** 3 + 2 * t ** 2 + 0.5 * t,
                  0.5 * t ** 3 - 0.5 * t ** 2]
            first = Y0 - 1
        return [(min(max(first + k, 0), L - 1), w) for k, w in enumerate(ws)]
    ty, tx = taps(position(m[:3], i, j), LH), taps(position(m[3:], i, j), LW)
    return sum(wy * wx * src[Y, X].astype(np.float64) for Y, wy in ty for X, wx in tx)


# ---- the kernel sweep of test_gpu_warp.py; test_warp_cpu.py runs the restatement over the same cases ----------------
KINDS = [("u8", 3), ("u8", 4), ("u16", 1), ("u16", 2), ("u16", 3), ("u16", 4)]
SRC_SIZES = [(1, 1), (2, 2), (5, 7), (17, 33), (40, 68)]                     # the level's size LH x LW
OUT_SIZES = [(1, 1), (7, 9), (16, 16), (17, 33), (70, 130)]
SHIFTS = (0, 1, 2)
NODATA, FILL = view_ref.NODATA, {"u8": 201, "u16": 51234}
MATRICES = ["identity", "translate", "magnify3", "magnify5.25", "minify2.5", "rot90", "rot180", "rot30", "shear",
            "mirror", "overhang", "zero column"]


def image_size(level_size_, l):
    """a level-0 side whose level l has level_size_ pixels and that is no multiple of 2^l for l > 0"""
    return max(1, (level_size_ << l) - (1 << l) + 1)


def matrix(name, H, W, oh, ow):
    """the named view of an H x W image at oh x ow, as Q16"""
    cy, cx = H / 2, W / 2
    fit = max(H / oh, W / ow)                                                 # level-0 pixels per output pixel: all of it
    table = {
        "identity": [[1, 0, 0], [0, 1, 0]],
        "translate": [[1, 0, 0.37], [0, 1, -0.61]],
        "magnify3": [[1 / 3, 0, H / 5], [0, 1 / 3, W / 7]],
        "magnify5.25": [[1 / 5.25, 0, 0.3], [0, 1 / 5.25, W / 3]],
        "minify2.5": [[2.5, 0, 0.25], [0, 2.5, 0.5]],
        "rot90": rotation(cy, cx, 90, fit, oh, ow),
        "rot180": rotation(cy, cx, 180, H / oh, oh, ow),
        "rot30": rotation(cy, cx, 30, 0.8 * fit, oh, ow),
        "shear": [[H / oh, 0.5, 0], [0.25, W / ow, -1]],
        "mirror": [[-H / oh, 0, H], [0, -W / ow, W]],
        "overhang": [[(H + 9) / oh, 0, -4.5], [0, (W + 11) / ow, -5.5]],
        "zero column": [[0.5, 0, 1], [0.25, 0, 0.5]],
    }
    return q16(table[name])


def kernel_case(src_size, out_size, l, name, mode, margin=0):
    """One kernel call: the level-0 size, the matrix and the planned source window, `margin` level pixels wider where
    the level has room; a view beside the image gets the level's first pixel as its window."""
    (LH, LW), (oh, ow) = src_size, out_size
    H, W = image_size(LH, l), image_size(LW, l)
    assert (level_size(H, l), level_size(W, l)) == (LH, LW)
    m = matrix(name, H, W, oh, ow)
    win = warp_window(l, LH, LW, H, W, m, oh, ow, mode) or (0, 0, 1, 1)
    ya, xa = max(win[0] - margin, 0), max(win[1] - margin, 0)
    yb, xb = min(win[0] + win[2] + margin, LH), min(win[1] + win[3] + margin, LW)
    return {"H": H, "W": W, "LH": LH, "LW": LW, "shift": l, "m": m, "size": (oh, ow), "sy0": ya, "sx0": xa, "sh": yb - ya,
            "sw": xb - xa}


def level_image(kind, C, LH, LW):
    """the whole level: view_ref's kernel image (random values, nodata blocks and speckle, blocks of 0 and of the top)"""
    return view_ref.kernel_image(kind, C, LH, LW)


def validity(LH, LW, seed=0):
    """validity bytes of a level: about 70 % valid, any non-zero byte, nothing valid over the top-left quarter"""
    rng = np.random.default_rng(LH * 13 + LW + seed)
    valid = rng.random((LH, LW)) < 0.7
    if LH > 1 or LW > 1:
        valid[:max(1, LH // 2), :max(1, LW // 2)] = False
    return valid.astype(np.uint8) * rng.integers(1, 256, size=valid.shape).astype(np.uint8)


def run_case(img, val, c, mode, nodata=None, fill=0):
    """the restatement on a kernel case: the window is cut from the level here"""
    ys, xs = slice(c["sy0"], c["sy0"] + c["sh"]), slice(c["sx0"], c["sx0"] + c["sw"])
    return warp(img[ys, xs], None if val is None else val[ys, xs], c["sy0"], c["sx0"], c["shift"], c["LH"], c["LW"], c["H"],
                c["W"], c["m"], c["size"], mode, nodata, fill)
