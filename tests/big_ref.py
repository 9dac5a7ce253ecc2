"""Banded restatements for images too large to hold on the host (no tests here, nothing of dsic_amd).

Each function gives the selected part of one kernel's output (a tile row, a band of output rows, a window) and asks its
source for rows by number; it never holds the image.  None of them states a kernel's arithmetic: each cuts the rows the
part depends on out of the source and hands them, with their origin, to the full restatement of codec_ref, u16_ref,
pyramid_ref, valid_ref, mask_ref, view_ref, render_ref, warp_ref, index_ref, composite_ref or best_pixel_ref.
test_big_scene_cpu.py shows on small images that every part equals the same part of the full restatement.

A source has H, W, C, kind ("u8", "u16" HWC; "f32" CHW), rows(ys) -> the rows ys in that layout, and valid(ys) -> uint8
[len(ys)][W].  ArraySource wraps a host array, SceneSource a closed-form scene of big_scene.py.
"""
import functools

import numpy as np

import best_pixel_ref
import blend_ref
import codec_ref
import composite_ref
import index_ref
import mask_ref
import pyramid_ref
import render_ref
import u16_ref
import valid_ref
import view_ref
import warp_ref


class ArraySource:
    def __init__(self, img, valid=None):
        self.img, self.val = img, valid
        self.kind = {"uint8": "u8", "uint16": "u16", "float32": "f32"}[img.dtype.name]
        self.C, self.H, self.W = (img.shape if self.kind == "f32" else (img.shape[2], img.shape[0], img.shape[1]))

    def rows(self, ys):
        ys = np.asarray(ys, dtype=np.int64)
        assert ys.min() >= 0 and ys.max() < self.H
        return self.img[:, ys] if self.kind == "f32" else self.img[ys]

    def valid(self, ys):
        return self.val[np.asarray(ys, dtype=np.int64)].astype(np.uint8)


class SceneSource:
    """a big_scene.Scene on the host; the last few bands asked for are kept"""

    def __init__(self, scene, keep=48):
        import big_scene
        self.scene, self.xp, self.keep, self.cache = scene, big_scene.NP, keep, {}
        self.kind, self.H, self.W, self.C = scene.kind, scene.H, scene.W, scene.C

    def _get(self, what, ys, make):
        ys = np.asarray(ys, dtype=np.int64)
        assert ys.min() >= 0 and ys.max() < self.H
        key = (what, ys.tobytes())
        if key not in self.cache:
            while len(self.cache) >= self.keep:
                self.cache.pop(next(iter(self.cache)))
            out = make(self.xp, ys)
            out.setflags(write=False)
            self.cache[key] = out
        return self.cache[key]

    def rows(self, ys):
        return self._get("rows", ys, self.scene.rows)

    def valid(self, ys):
        return self._get("valid", ys, self.scene.valid_rows)


class RowBand:
    """rows [y0, y0 + len(band)) of a [H][W] array, indexed with the image's own row numbers"""

    def __init__(self, band, y0):
        self.band, self.y0 = band, y0

    def __getitem__(self, key):
        ys, xs = key
        assert ys.start >= self.y0 and ys.stop <= self.y0 + len(self.band), (ys, self.y0, len(self.band))
        return self.band[ys.start - self.y0:ys.stop - self.y0, xs]


# ---- tile geometry ------------------------------------------------------------------------------------------------
def tile_rows(H, th, overlap=0):
    """the number of tile rows"""
    return blend_ref.axis(H, th, overlap)["n"]


def tiles_per_row(W, tw, overlap=0):
    return blend_ref.axis(W, tw, overlap)["n"]


@functools.lru_cache(maxsize=16)
def _row_axis(H, th, overlap):
    """(origins of the tile rows, the image row of every padded row)"""
    return tuple(blend_ref.axis(H, th, overlap)["o"]), codec_ref._reflect(H, codec_ref.ceil16(H))


def source_rows(H, th, overlap, i):
    """the image rows that tile row i reads, in tile order (reflected past the last row)"""
    origins, reflected = _row_axis(H, th, overlap)
    return reflected[origins[i]:origins[i] + th]


def tile_rows_reading(H, th, overlap, ys):
    """the tile rows that read one of the image rows ys"""
    ys = np.asarray(sorted(set(int(y) for y in ys)), dtype=np.int64)
    return [i for i in range(tile_rows(H, th, overlap)) if np.isin(source_rows(H, th, overlap, i), ys).any()]


def owned_rows(H, th, i):
    """(origin, first owned row, one past the last owned row inside the image) of tile row i (no overlap)"""
    return mask_ref.axis(H, th)[i]


# ---- readers ------------------------------------------------------------------------------------------------------
def gather_tile_row(src, th, tw, overlap, i, scale=None):
    """the tiles of tile row i: uint8 [nx][th][tw][C], float32 [nx][C][th][tw] (f32, and u16 with its scale).  The th
    rows the tile row reads, in its order, are an image of th rows: a grid of one tile row that reflects no row."""
    small = src.rows(source_rows(src.H, th, overlap, i))
    if src.kind == "u8":
        out = codec_ref.gather_u8(small, th, tw, overlap)
    elif src.kind == "u16":
        out = u16_ref.gather(small, th, tw, scale, overlap)
    else:
        out = codec_ref.gather_f32(small, th, tw, overlap)
    assert out.shape[0] == tiles_per_row(src.W, tw, overlap)
    return out


def _mask_band(src, y0, y1, nodata):
    """the mask (True = nodata, or invalid when nodata is None) of rows [y0, y1), addressed by image row"""
    ys = np.arange(y0, y1)
    m = (src.valid(ys) == 0) if nodata is None else mask_ref.nodata_mask(src.rows(ys), nodata)
    return RowBand(m, y0)


def classify_tile_row(src, th, tw, i, nodata=None):
    """counts of the tiles of tile row i (nodata pixels, or invalid ones when nodata is None)"""
    _, y0, y1 = owned_rows(src.H, th, i)
    return mask_ref.counts_in(_mask_band(src, y0, y1, nodata), mask_ref.tile_row(src.H, src.W, th, tw, i))


def m_planes_tile_row(src, th, tw, i, nodata=None):
    """the m planes of the tiles of tile row i, bool [nx][th][tw]"""
    _, y0, y1 = owned_rows(src.H, th, i)
    band = _mask_band(src, y0, y1, nodata)
    return [mask_ref.m_plane(band, t, th, tw) for t in mask_ref.tile_row(src.H, src.W, th, tw, i)]


def delta_planes_tile_row(src, th, tw, i, nodata=None):
    """(d planes as dwords [nx][th*tw/32], their popcounts)"""
    d = [mask_ref.delta(m) for m in m_planes_tile_row(src, th, tw, i, nodata)]
    return np.stack([mask_ref.plane_dwords(p) for p in d]), [int(p.sum()) for p in d]


def quantize_tile_row(src, x_hat, th, tw, i, scale, tau):
    """residual16_ref.quantize of a uint16 image against the predictor of x_hat (float32 [nx][C][th][tw], the decoded
    tiles of tile row i) over the pixels each tile owns inside the image, 0 elsewhere -> (q int64 [nx][C][th][tw], the
    largest |q| of every tile)"""
    import residual16_ref
    _, y0, y1 = owned_rows(src.H, th, i)
    band = src.rows(np.arange(y0, y1))
    p = residual16_ref.predictor(x_hat, scale)
    out = np.zeros(x_hat.shape, dtype=np.int64)
    for j, (oy, ox, a, b, c, d) in enumerate(mask_ref.tile_row(src.H, src.W, th, tw, i)):
        x = band[a - y0:b - y0, c:d].astype(np.int64).transpose(2, 0, 1)
        out[j][:, a - oy:b - oy, c - ox:d - ox] = residual16_ref.quantize(x, p[j][:, a - oy:b - oy, c - ox:d - ox], tau)
    return out, [int(np.abs(t).max()) for t in out]


def _level_rows(H, shift, region):
    """the rows [ya, yb) of the level-`shift` image of H rows that a region of level 0 covers"""
    ya, _, nh, _ = view_ref.level_window(shift, *region)
    assert ya + nh <= H
    return ya, ya + nh


def resample(src, shift, region, size, mode, nodata=None):
    """view_ref.resample of the whole image as the level-`shift` window at (0, 0): only its covered rows are cut out"""
    ya, yb = _level_rows(src.H, shift, region)
    return view_ref.resample(src.rows(np.arange(ya, yb)), ya, 0, shift, region, size, mode, nodata)


def resample_valid(src, shift, region, size, mode, fill):
    ya, yb = _level_rows(src.H, shift, region)
    ys = np.arange(ya, yb)
    return valid_ref.resample(src.rows(ys), src.valid(ys), ya, 0, shift, region, size, mode, fill)


def render(src, with_valid, shift, region, size, bands, pairs, mode, nodata, alpha, background):
    ya, yb = _level_rows(src.H, shift, region)
    ys = np.arange(ya, yb)
    return render_ref.render(src.rows(ys), src.valid(ys) if with_valid else None, ya, 0, shift, region, size, bands,
                             pairs, mode, nodata, alpha, background)


def index_render(src, with_valid, shift, region, size, index, pair, cmap, mode, nodata, alpha, background):
    """the index view of the same window: the resample of valid_ref (a validity window) or view_ref, then
    index_ref.display_index, as test_gpu_index.py pairs them"""
    ya, yb = _level_rows(src.H, shift, region)
    ys = np.arange(ya, yb)
    if with_valid:
        res, ok = valid_ref.resample(src.rows(ys), src.valid(ys), ya, 0, shift, region, size, mode, 0)
    else:
        res, ok = view_ref.resample(src.rows(ys), ya, 0, shift, region, size, mode, nodata if mode == "average" else None), None
    return index_ref.display_index(res, ok, index, pair, cmap, alpha, background)


# ---- warped reads of a whole level ----------------------------------------------------------------------------------
def warp_image(src, l):
    """(H, W) of the level-0 image whose level l the source is: warp_ref.image_size of its sides"""
    return warp_ref.image_size(src.H, l), warp_ref.image_size(src.W, l)


def warp(src, l, m, size, mode, with_valid=False, nodata=None, fill=0):
    """warp_ref.warp with the whole source as the level-l window at (0, 0): only the rows of warp_ref.warp_window are
    cut out, those of the cubic taps for every mode (they hold the others', and warp_ref.warp asserts that every tap
    lies inside what it was given), so that the modes of one view ask the source for the same rows"""
    H, W = warp_image(src, l)
    win = warp_ref.warp_window(l, src.H, src.W, H, W, m, *size, 2) or (0, 0, 1, 1)
    ys = np.arange(win[0], win[0] + win[2])
    return warp_ref.warp(src.rows(ys), src.valid(ys) if with_valid else None, win[0], 0, l, src.H, src.W, H, W, m, size, mode,
                         nodata, fill)


def warp_render(src, l, m, size, mode, with_valid, nodata, bands, pairs, alpha, background):
    res, ok = warp(src, l, m, size, mode, with_valid, nodata, 0)
    return render_ref.display(res, ok, bands, pairs, alpha, background)


def warp_index(src, l, m, size, mode, with_valid, nodata, index, pair, cmap, alpha, background):
    res, ok = warp(src, l, m, size, mode, with_valid, nodata, 0)
    return index_ref.display_index(res, ok, index, pair, cmap, alpha, background)


def warp_rows(img, val, geometry, m, size, mode, nodata, fill, i0, i1, j0=0, j1=None):
    """Output rows [i0, i1) (columns [j0, j1) of them) of the warped view of a small host image, the whole level l:
    geometry = (l, LH, LW, H, W).  The view with m2 + m0 i0 + m1 j0 and m5 + m3 i0 + m4 j0 in the place of m2 and m5,
    exactly: P is affine in i and j, and m0 (2 (i + i0) + 1) + 2 m2 = m0 (2 i + 1) + 2 (m2 + m0 i0)."""
    l, LH, LW, H, W = geometry
    j1 = size[1] if j1 is None else j1
    assert 0 <= i0 < i1 <= size[0] and 0 <= j0 < j1 <= size[1] and img.shape[:2] == (LH, LW)
    moved = (m[0], m[1], m[2] + m[0] * i0 + m[1] * j0, m[3], m[4], m[5] + m[3] * i0 + m[4] * j0)
    return warp_ref.warp(img, val, 0, 0, l, LH, LW, H, W, moved, (i1 - i0, j1 - j0), mode, nodata, fill)


# ---- composites -----------------------------------------------------------------------------------------------------
class NoValidity:
    """a source handed to the composite without its validity window"""

    def __init__(self, src):
        self.rows, self.valid = src.rows, None


def _validity(s, ys):
    if s.valid is None or (isinstance(s, ArraySource) and s.val is None):
        return None
    return s.valid(ys)


def composite_rows(sources, rects, nodata, ids, C, oh, ow, mode, index, fill, y0, y1):
    """Output rows [y0, y1) of a composite of placed sources (anything with rows(ys) and valid(ys); valid = None: no
    validity window): every source is cut to the band and its rect moved, one that misses the band is dropped, the
    others keep their order and ids.  index = None: composite_ref.composite -> (dst, valid, count); else
    best_pixel_ref.pick -> (dst, valid, count, source).  A band that no source meets has no candidate anywhere, which
    both restatements give for a source that is nowhere valid: the first source's first row stands in, invalid."""
    assert 0 <= y0 < y1 <= oh
    srcs, vals, cut, nds, kept = [], [], [], [], []
    for k, (s, (dy, dx, h, w)) in enumerate(zip(sources, rects)):
        a, b = max(dy, y0), min(dy + h, y1)
        if a < b:
            ys = np.arange(a - dy, b - dy)
            srcs.append(s.rows(ys))
            vals.append(_validity(s, ys))
            cut.append((a - y0, dx, b - a, w))
            nds.append(nodata[k])
            kept.append(k)
    if not srcs:
        dy, dx, h, w = rects[0]
        srcs, cut, nds, kept = [sources[0].rows(np.arange(1))], [(0, dx, 1, w)], [nodata[0]], [0]
        vals = [np.zeros((1, w), dtype=np.uint8)]
    if index is None:
        return composite_ref.composite(srcs, vals, cut, nds, C, y1 - y0, ow, mode, fill)
    return best_pixel_ref.pick(srcs, vals, cut, nds, [k if ids is None else ids[k] for k in kept], C, y1 - y0, ow, mode, index,
                               fill)                                            # without ids a source's id is its position


# ---- writers ------------------------------------------------------------------------------------------------------
def halve_rows(src, y0, y1, with_valid=False):
    """rows [y0, y1) of the halved image (and of the halved validity): the source rows [2 y0, min(2 y1, H)) are an
    image of their own whose halving they are, as an odd count of them can only end at the image's last row"""
    s0, s1 = 2 * y0, min(2 * y1, src.H)
    assert 0 <= y0 < y1 <= pyramid_ref.halved(src.H)
    ys = np.arange(s0, s1)
    band = src.rows(ys)
    if with_valid:
        return valid_ref.halve(band, src.valid(ys) != 0)
    if src.kind == "u8":
        return pyramid_ref.halve_u8(band)
    return u16_ref.halve(band) if src.kind == "u16" else pyramid_ref.halve_f32(band)


def stitch_rows(tiles, ids, H, W, th, tw, y0, y1, kind, fill, scale=None):
    """rows [y0, y1) of the image the stitch writes with the whole image as its window: the window (y0, 0, y1-y0, W)"""
    win = (y0, 0, y1 - y0, W)
    if kind == "u16":
        return u16_ref.stitch(tiles, ids, H, W, th, tw, win, scale, fill)
    return codec_ref.stitch(tiles, ids, H, W, th, tw, win, kind, fill)


def blend_rows(tiles, ids, H, W, C, th, tw, overlap, y0, y1):
    """rows [y0, y1) of the unfinished canvas [C][H][W] that the blend of the tiles `ids` (ascending) leaves, from
    zeros: blend_ref.blend_f32 with its row window"""
    return blend_ref.blend_f32([list(zip(ids, tiles))], H, W, C, th, tw, overlap, rows=(y0, y1))


def blend_support_rows(ids, H, W, th, tw, overlap):
    """the merged row ranges, inside the image, of the supports of the tiles `ids`"""
    ay, ax = blend_ref.grid(H, W, th, tw, overlap)
    spans = sorted({(ay["sup"][t // ax["n"]][0], min(ay["sup"][t // ax["n"]][1], H)) for t in ids})
    out = []
    for a, b in spans:
        if out and a <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], b))
        else:
            out.append((a, b))
    return out


QMAX = 4                                       # stitch_res_rows takes residual steps in -QMAX .. QMAX


def stitch_res_rows(tiles, q, tau, ids, H, W, th, tw, y0, y1, kind, fill, scale=None):
    """The same of the stitch with a residual (kind u8 or u16): reconstruct(p, q, tau) of residual_ref / residual16_ref
    where a tile of the call owns the pixel, p the plain stitch's value there.  Which tile's q a pixel takes, and
    whether any does, is read off two more stitches into float32, which move values in [0, 1] unchanged: one of
    (q + QMAX) / (2 QMAX), exact in float32, and one of ones over a fill of 0."""
    import residual16_ref
    import residual_ref
    q = np.asarray(q)
    assert np.array_equal(q, np.round(q)) and np.abs(q).max() <= QMAX
    p = stitch_rows(tiles, ids, H, W, th, tw, y0, y1, kind, fill, scale)
    win = (y0, 0, y1 - y0, W)
    moved = codec_ref.stitch(((q + QMAX) / (2 * QMAX)).astype(np.float32), ids, H, W, th, tw, win, "f32", np.float32(0.5))
    owned = codec_ref.stitch(np.ones_like(tiles), ids, H, W, th, tw, win, "f32", np.float32(0)) == 1
    steps = np.round(moved.astype(np.float64) * (2 * QMAX) - QMAX).astype(np.int64).transpose(1, 2, 0)
    ref = residual_ref if kind == "u8" else residual16_ref
    return np.where(owned.transpose(1, 2, 0), ref.reconstruct(p, steps, tau), p).astype(p.dtype)


def finish_rows(canvas_band, kind, scale=None):
    """the finished rows of a band [C][rows][W] of the canvas: HWC for u8 and u16, CHW for f32"""
    if kind == "u8":
        return blend_ref.finish_u8(canvas_band)
    return u16_ref.blend_finish(canvas_band, scale) if kind == "u16" else blend_ref.finish_f32(canvas_band)


def mask_apply_rows(pre_band, H, W, th, tw, y0, desc, planes, v):
    """rows [y0, y0 + len) of the image mask_apply writes with the whole image as its window; pre_band is what those
    rows held before (uint8 / uint16 [rows][W][C] or float32 [C][rows][W])"""
    rows = pre_band.shape[1] if pre_band.dtype == np.float32 else pre_band.shape[0]
    win = (y0, 0, rows, W)
    if pre_band.dtype == np.uint16:
        return valid_ref.apply(pre_band, win, H, W, th, tw, desc, planes, v)
    return mask_ref.apply(pre_band, win, H, W, th, tw, desc, planes, v)


def mask_window_rows(pre_band, H, W, th, tw, y0, desc, planes):
    return valid_ref.window_valid(pre_band, (y0, 0, pre_band.shape[0], W), H, W, th, tw, desc, planes)
