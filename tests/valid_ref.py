"""NumPy restatement of the validity masks of the whole-image codec (stream version 8; csrc/mask.hip's valid exports,
csrc/valid.hip, the masked resampler of csrc/view.hip).  No tests here and nothing of dsic_amd; the tile geometry, the
planes and the payloads are mask_ref's, the halving taps pyramid_ref's, the resampling geometry view_ref's.

valid is a bool [H][W] array, True = the pixel holds data.  What the stream stores is the invalid mask ~valid, tile by
tile exactly as mask_ref stores a nodata mask: a set plane bit means owned, inside the image and invalid.

Masked halving: an output pixel takes the taps rows 2y and min(2y+1, H-1), columns 2x and min(2x+1, W-1), a repeated tap
counting twice.  k = the valid taps; the output is valid iff k > 0 and is (2 S + k) // (2 k) per channel with S the sum
over the valid taps; for k = 0 it is (a + b + c + d + 2) >> 2 over all four."""
import struct

import numpy as np

import mask_ref
import pyramid_ref
import view_ref


# ---- states, planes, the block ----------------------------------------------------------------------------------------
def counts(valid, th, tw):
    """invalid pixels per tile among its owned pixels"""
    H, W = valid.shape
    return mask_ref.counts(~valid, H, W, th, tw)


def states(valid, th, tw):
    H, W = valid.shape
    return mask_ref.states(~valid, H, W, th, tw)


def m_planes(valid, th, tw):
    """per tile the m plane, bool [th][tw]: owned, inside the image and invalid"""
    H, W = valid.shape
    return [mask_ref.m_plane(~valid, t, th, tw) for t in mask_ref.tiles(H, W, th, tw)]


def block(valid, fill, th, tw):
    """the mask block of a validity mask (its nodata field carries fill), and its states"""
    st = states(valid, th, tw)
    recs, bodies = [], []
    for t, (s, m) in enumerate(zip(st, m_planes(valid, th, tw))):
        if s == mask_ref.MIXED:
            mode, body = mask_ref.payload(mask_ref.delta(m))
            recs.append(struct.pack("<3I", t, mode, len(body)))
            bodies.append(body)
    n = len(st)
    return (b"".join([mask_ref.MAGIC, struct.pack("<5I", n, th, tw, fill, len(recs)), bytes(st), b"\0" * (-n % 4)]
                     + recs + bodies), st)


def head(version, tag, H, W, C, kind, th, tw, N, M, in_ch, spatial, batch, batches, segments, fill, coded, scale=None):
    """the bytes of a version-8 stream in front of the mask block's length word"""
    out = struct.pack("<6sHI6I4I2I", b"DSICI\0", version, tag, H, W, C, kind, th, tw, N, M, in_ch, spatial, batch, batches)
    out += struct.pack("<4I", segments, 0, fill, coded)
    for lo, hi in scale or ():
        out += struct.pack("<2I", lo, hi)
    return out


# ---- the window movers ------------------------------------------------------------------------------------------------
def _rects(window, H, W, th, tw, desc):
    """per listed tile inside the grid whose owned rectangle meets the window: (plane index, oy, ox, a, b, c, d)"""
    wy, wx, wh, ww = window
    grid = mask_ref.tiles(H, W, th, tw)
    for t, pi in desc:
        if not 0 <= t < len(grid):
            continue
        oy, ox, y0, y1, x0, x1 = grid[t]
        a, b, c, d = max(y0, wy), min(y1, wy + wh), max(x0, wx), min(x1, wx + ww)
        if a < b and c < d:
            yield pi, oy, ox, a, b, c, d


def apply(win, window, H, W, th, tw, desc, planes, fill):
    """win: uint8 or uint16 [h][w][C], the window (y0, x0, h, w) of the image; desc: (tile, plane index or -1 for all
    set).  A copy with fill at the listed tiles' owned pixels inside the window whose bit is set."""
    out = win.copy()
    wy, wx = window[:2]
    for pi, oy, ox, a, b, c, d in _rects(window, H, W, th, tw, desc):
        sel = np.ones((b - a, d - c), dtype=bool) if pi < 0 else planes[pi][a - oy:b - oy, c - ox:d - ox]
        out[a - wy:b - wy, c - wx:d - wx][sel] = fill
    return out


def window_valid(pre, window, H, W, th, tw, desc, planes):
    """pre: uint8 [h][w], the caller's pre-fill.  A copy with 0 (bit set, or plane -1) or 1 at every owned pixel of the
    listed tiles inside the window; the rest as it was."""
    out = pre.copy()
    wy, wx = window[:2]
    for pi, oy, ox, a, b, c, d in _rects(window, H, W, th, tw, desc):
        sel = np.ones((b - a, d - c), dtype=bool) if pi < 0 else planes[pi][a - oy:b - oy, c - ox:d - ox]
        out[a - wy:b - wy, c - wx:d - wx] = (~sel).astype(np.uint8)
    return out


# ---- masked halving and range -----------------------------------------------------------------------------------------
def halve(img, valid):
    """uint8 or uint16 [H][W][C], bool [H][W] -> (the halved image, the halved mask)"""
    assert img.dtype in (np.uint8, np.uint16) and img.ndim == 3 and valid.shape == img.shape[:2] and valid.dtype == bool
    y0, y1 = pyramid_ref._taps(img.shape[0])
    x0, x1 = pyramid_ref._taps(img.shape[1])
    v = img.astype(np.int64)
    taps = [(y0, x0), (y0, x1), (y1, x0), (y1, x1)]
    S = np.zeros((len(y0), len(x0), img.shape[2]), dtype=np.int64)
    A = S.copy()
    k = np.zeros((len(y0), len(x0)), dtype=np.int64)
    for ys, xs in taps:
        ok = valid[ys][:, xs]
        px = v[ys][:, xs]
        A += px
        S += px * ok[:, :, None]
        k += ok
    kk = np.maximum(k, 1)[:, :, None]
    out = np.where(k[:, :, None] > 0, (2 * S + kk) // (2 * kk), (A + 2) >> 2)
    return out.astype(img.dtype), k > 0


def chain(img, valid, n):
    levels, masks = [img], [valid]
    for _ in range(n):
        a, m = halve(levels[-1], masks[-1])
        levels.append(a)
        masks.append(m)
    return levels, masks


def band_range(img, valid):
    """per band (min, max) over the valid pixels; (0, 0) where there is none"""
    out = []
    for c in range(img.shape[2]):
        v = img[:, :, c][valid]
        out.append((int(v.min()), int(v.max())) if v.size else (0, 0))
    return out


# ---- masked resample --------------------------------------------------------------------------------------------------
def resample(src, sval, sy0, sx0, shift, region, size, mode="average", fill=0):
    """src: uint8 / uint16 [sh][sw][C]; sval: bool or uint8 [sh][sw] -> (out [oh][ow][C], its validity bool [oh][ow]).
    view_ref.resample with the mask in the place of the value comparison: a source pixel stays out of S and T iff it is
    invalid, T = 0 gives fill and invalid; nearest copies pixel and validity."""
    y0, x0, h, w = region
    oh, ow = size
    C = src.shape[2]
    sval = np.asarray(sval) != 0
    out = np.zeros((oh, ow, C), dtype=src.dtype)
    oval = np.zeros((oh, ow), dtype=bool)
    if mode == "nearest":
        ys, xs = view_ref.nearest_index(y0, h, oh, shift), view_ref.nearest_index(x0, w, ow, shift)
        for i, Y in enumerate(ys):
            for j, X in enumerate(xs):
                out[i, j] = src[Y - sy0, X - sx0]
                oval[i, j] = sval[Y - sy0, X - sx0]
        return out, oval
    assert mode == "average"
    rows, cols = view_ref.axis_weights(y0, h, oh, shift), view_ref.axis_weights(x0, w, ow, shift)
    for i, row in enumerate(rows):
        for j, col in enumerate(cols):
            T, S = 0, np.zeros(C, dtype=np.int64)
            for Y, wy in row:
                for X, wx in col:
                    if not sval[Y - sy0, X - sx0]:
                        continue
                    T += wy * wx
                    S = S + np.int64(wy * wx) * src[Y - sy0, X - sx0].astype(np.int64)
            oval[i, j] = T > 0
            out[i, j] = (2 * S + T) // (2 * T) if T else fill
    return out, oval
