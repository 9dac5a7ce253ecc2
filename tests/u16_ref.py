"""NumPy restatements of the 16-bit image kind (csrc/image_u16.hip, codec.py stream version 6), for the uint16 tests
(no tests here, nothing of dsic_amd).

Per band the scale is a pair of integers lo <= hi in 0 .. 65535, R = hi - lo.
  norm(v)   = R == 0 ? 0.0f : float32(min(max(v, lo), hi) - lo) / float32(R)      one float32 division
  denorm(x) = lo + uint32(clamp(x, 0, 1) * float32(R) + 0.5f)                     one multiply, one add, truncated
clamp(x, 0, 1) is x > 0 ? (x > 1 ? 1 : x) : 0, which sends a NaN to 0.  Images are uint16 [H][W][C]; the model's side is
float32 [C][H][W].  The tile grid (with overlap) is blend_ref.axis', the reflect padding and the owned rectangles are
codec_ref's.  Halving is pyramid_ref's uint8 rule on 32-bit sums: (a + b + c + d + 2) >> 2.
"""
import numpy as np

import blend_ref
import codec_ref
import pyramid_ref


def norm(v, lo, hi):
    """values of one band (any integer array) -> float32"""
    v = np.clip(np.asarray(v).astype(np.int64), lo, hi) - lo
    if hi == lo:
        return np.zeros(v.shape, dtype=np.float32)
    return v.astype(np.float32) / np.float32(hi - lo)


def clamp01(x):
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(x > 0, np.where(x > 1, np.float32(1), x), np.float32(0)).astype(np.float32)


def denorm(x, lo, hi):
    """float32 values of one band -> uint16"""
    y = clamp01(x) * np.float32(hi - lo)
    assert y.dtype == np.float32
    y = y + np.float32(0.5)
    return (y.astype(np.uint32) + np.uint32(lo)).astype(np.uint16)


def norm_image(img_hwc, scale):
    """uint16 [H][W][C] -> float32 [C][H][W]"""
    assert img_hwc.dtype == np.uint16 and img_hwc.ndim == 3 and len(scale) == img_hwc.shape[2]
    return np.stack([norm(img_hwc[:, :, c], lo, hi) for c, (lo, hi) in enumerate(scale)])


def denorm_image(x_chw, scale):
    """float32 [C][h][w] -> uint16 [h][w][C]"""
    assert len(scale) == x_chw.shape[0]
    return np.ascontiguousarray(np.stack([denorm(x_chw[c], lo, hi) for c, (lo, hi) in enumerate(scale)], axis=2))


def band_range(img_hwc):
    return [(int(img_hwc[:, :, c].min()), int(img_hwc[:, :, c].max())) for c in range(img_hwc.shape[2])]


def gather(img_hwc, th, tw, scale, overlap=0):
    """uint16 [H][W][C] -> float32 [n][C][th][tw]: the tiles of norm(img), reflect-padded, tiles row-major"""
    H, W = img_hwc.shape[:2]
    ay, ax = blend_ref.axis(H, th, overlap), blend_ref.axis(W, tw, overlap)
    assert ay["t"] == th and ax["t"] == tw
    x = norm_image(img_hwc, scale)
    ry, rx = codec_ref._reflect(H, ay["Lp"]), codec_ref._reflect(W, ax["Lp"])
    return np.stack([x[:, ry[y:y + th]][:, :, rx[c:c + tw]] for y in ay["o"] for c in ax["o"]])


def stitch(tiles, ids, H, W, th, tw, window, scale, fill):
    """tiles float32 [len(ids)][C][th][tw]; window (y0, x0, h, w) -> uint16 [h][w][C].  A pixel no tile of ids owns
    keeps fill; ids outside the grid write nothing."""
    g = codec_ref.grid(H, W, th, tw)
    C = tiles.shape[1]
    wy, wx, wh, ww = window
    out = np.full((wh, ww, C), fill, dtype=np.uint16)
    for k, t in enumerate(ids):
        if t < 0 or t >= g["n"]:
            continue
        i, j = divmod(t, g["nx"])
        y0, y1 = max(g["own_y"][i][0], wy), min(g["own_y"][i][1], H, wy + wh)
        x0, x1 = max(g["own_x"][j][0], wx), min(g["own_x"][j][1], W, wx + ww)
        if y0 >= y1 or x0 >= x1:
            continue
        oy, ox = g["ys"][i], g["xs"][j]
        out[y0 - wy:y1 - wy, x0 - wx:x1 - wx] = denorm_image(tiles[k][:, y0 - oy:y1 - oy, x0 - ox:x1 - ox], scale)
    return out


def blend_finish(canvas_chw, scale):
    """float32 [C][h][w] canvas -> uint16 [h][w][C]: denorm(min(v, 1))"""
    with np.errstate(invalid="ignore"):
        v = np.where(canvas_chw > 1, np.float32(1), canvas_chw).astype(np.float32)
    return denorm_image(v, scale)


def halve(img_hwc):
    """uint16 [H][W][C] -> uint16 [ceil(H/2)][ceil(W/2)][C]"""
    assert img_hwc.dtype == np.uint16 and img_hwc.ndim == 3
    y0, y1 = pyramid_ref._taps(img_hwc.shape[0])
    x0, x1 = pyramid_ref._taps(img_hwc.shape[1])
    v = img_hwc.astype(np.uint32)
    s = v[y0][:, x0] + v[y0][:, x1] + v[y1][:, x0] + v[y1][:, x1] + np.uint32(2)
    return (s >> np.uint32(2)).astype(np.uint16)


def chain(img_hwc, n):
    out = [img_hwc]
    for _ in range(n):
        out.append(halve(out[-1]))
    return out
