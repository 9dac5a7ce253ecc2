"""NumPy restatement of the index views (render.h's index tail in csrc/view.hip and csrc/warp.hip, the index histogram of
csrc/histogram.hip, codec.ImageReader.render_index / render_index_warped / index_histogram / index_stretch,
codec.colormap_from_anchors).  No tests here; test_index_cpu.py holds the restatement to exact rationals and to its own
properties, test_gpu_index.py holds the kernels and the reader to it.  The resampling is view_ref's and valid_ref's, the
warp warp_ref's, the stretch and the percentile rule render_ref's.

An index is (kind, a, b) over the samples A and B of bands a and b, top = 255 or 65535, kept as u = v - vmin:
  band:        u = A                                  v in 0 .. top
  difference:  u = A - B + top                        v = A - B in -top .. top
  nd:          u = (40000 A + s) // (2 s), s = A + B  v = 10000 (A - B) / s rounded half up, in -10000 .. 10000;
               s = 0: not defined, the pixel is invalid
  display:     k = stretch(u, lo - vmin, hi - vmin) for a pair (lo, hi) in v units, the pixel is cmap[k]; an invalid
               pixel is `background` in the three bands; alpha 255 (valid) or 0
  histogram:   hist[u] = the counted pixels (render_ref.histogram's rule) with a defined index u"""
import numpy as np

import render_ref

SCALE = 10000
KINDS = {"band": 0, "difference": 1, "nd": 2}


def top_of(img):
    return 255 if img.dtype == np.uint8 else 65535


def value_range(kind, top):
    """(vmin, vmax)"""
    return {"band": (0, top), "difference": (-top, top), "nd": (-SCALE, SCALE)}[kind]


def parse(index):
    """("nd", a, b) / ("difference", a, b) / ("band", a) -> (kind, a, b)"""
    kind = index[0]
    assert kind in KINDS and len(index) == (2 if kind == "band" else 3)
    return kind, index[1], index[-1]


def index_value(img, kind, a, b):
    """img: uint8 / uint16 [...][C] -> (u int64 [...], defined bool [...]); u is 0 where the index is not defined"""
    top = top_of(img)
    A, B = img[..., a].astype(np.int64), img[..., b].astype(np.int64)
    if kind == "band":
        return A, np.ones(A.shape, dtype=bool)
    if kind == "difference":
        return A - B + top, np.ones(A.shape, dtype=bool)
    assert kind == "nd"
    s = A + B
    return np.where(s != 0, (40000 * A + s) // np.maximum(2 * s, 1), 0), s != 0


def stretch(u, lo, hi):
    """render_ref.stretch where it reaches; past its 65535 (a uint16 difference has u up to 131070) the same rule"""
    if hi <= 65535:
        return render_ref.stretch(u, lo, hi)
    assert 0 <= lo <= hi <= 2 * 65535
    R = hi - lo
    d = np.clip(np.asarray(u).astype(np.int64), lo, hi) - lo
    return ((510 * d + R) // (2 * R)).astype(np.uint8)


def display_index(res, ok, index, pair, cmap, alpha=False, background=0):
    """res: uint8 / uint16 [h][w][C], already resampled or warped; ok: bool [h][w] or None (all valid); pair: (lo, hi)
    in v units; cmap: uint8 [256][3] -> uint8 [h][w][3 (+ 1)]"""
    kind, a, b = parse(index)
    vmin, vmax = value_range(kind, top_of(res))
    assert vmin <= pair[0] <= pair[1] <= vmax
    u, defined = index_value(res, kind, a, b)
    ok = defined if ok is None else defined & (np.asarray(ok) != 0)
    k = stretch(u, pair[0] - vmin, pair[1] - vmin)
    out = np.zeros(res.shape[:2] + (3 + int(alpha),), dtype=np.uint8)
    out[:, :, :3] = np.where(ok[:, :, None], np.asarray(cmap)[k], background)
    if alpha:
        out[:, :, 3] = np.where(ok, 255, 0)
    return out


def histogram(img, valid=None, nodata=None, index=("band", 0)):
    """img: uint8 / uint16 [H][W][C] -> int64 [vmax - vmin + 1]"""
    kind, a, b = parse(index)
    if kind == "band":
        return render_ref.histogram(img, valid, nodata)[a]
    vmin, vmax = value_range(kind, top_of(img))
    ok = np.ones(img.shape[:2], dtype=bool) if valid is None else np.asarray(valid) != 0
    if nodata is not None:
        ok = ok & ~(img == nodata).all(axis=2)
    u, defined = index_value(img, kind, a, b)
    return np.bincount(u[ok & defined], minlength=vmax - vmin + 1)


def index_stretch(hist, index, top, percent=(2, 98)):
    """render_ref.percentile_stretch of an index histogram, shifted by vmin"""
    lo, hi = render_ref.percentile_stretch(np.asarray(hist)[None], percent)[0]
    vmin = value_range(parse(index)[0], top)[0]
    return lo + vmin, hi + vmin


def colormap_from_anchors(anchors):
    """[(p, (r, g, b)), ...] -> uint8 [256][3]: between neighbours p0 < p1, D = p1 - p0, entry i is
    (2 (c0 (p1 - i) + c1 (i - p0)) + D) // (2 D) per component"""
    assert anchors[0][0] == 0 and anchors[-1][0] == 255
    cmap = np.zeros((256, 3), dtype=np.uint8)
    for (p0, c0), (p1, c1) in zip(anchors, anchors[1:]):
        assert p0 < p1
        i = np.arange(p0, p1 + 1, dtype=np.int64)[:, None]
        c0, c1, D = np.asarray(c0, dtype=np.int64), np.asarray(c1, dtype=np.int64), p1 - p0
        cmap[p0:p1 + 1] = (2 * (c0 * (p1 - i) + c1 * (i - p0)) + D) // (2 * D)
    return cmap
