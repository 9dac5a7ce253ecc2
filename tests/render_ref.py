"""NumPy restatement of the rendered views (csrc/view.hip's render kernel, csrc/histogram.hip, codec.ImageReader.render /
.histogram, codec.stretch_from_histogram).  No tests here; test_render_cpu.py holds the restatement to its own
properties, test_gpu_render.py holds the kernels and the reader to it.  The resampling is view_ref's and valid_ref's.

  stretch: for a sample m and a pair lo <= hi, R = hi - lo, d = min(max(m, lo), hi) - lo, the byte is 0 for R = 0 and
           (510 d + R) // (2 R) otherwise: 255 d / R rounded half up
  render:  the resampled window (with a validity window: the masked one), output band b = channel bands[b] stretched
           with pairs[bands[b]]; an invalid output pixel is `background` in every band; alpha 255 (valid) or 0
  histogram: hist[c][v] = the counted pixels whose channel c is v; a validity plane leaves out its zeros, a nodata
           value the pixels whose channels all equal it
  percentiles: q = round(100 p); lo (hi) is the least v with cum(v) >= 1 and 10000 cum(v) >= q0 n (q1 n); n = 0: (0, 0)"""
import numpy as np

import valid_ref
import view_ref


def stretch(m, lo, hi):
    """m: an integer array (or scalar) -> uint8, through Python-sized int64 arithmetic"""
    assert 0 <= lo <= hi <= 65535
    R = hi - lo
    d = np.clip(np.asarray(m).astype(np.int64), lo, hi) - lo
    if R == 0:
        return np.zeros(d.shape, dtype=np.uint8)
    return ((510 * d + R) // (2 * R)).astype(np.uint8)


def display(img, valid, bands, pairs, alpha=False, background=0):
    """img: uint8 / uint16 [h][w][C], already resampled; valid: bool [h][w] or None (all valid) -> uint8
    [h][w][len(bands) (+ 1)]"""
    h, w, C = img.shape
    assert len(pairs) == C and len(bands) in (1, 3)
    out = np.zeros((h, w, len(bands) + int(alpha)), dtype=np.uint8)
    ok = np.ones((h, w), dtype=bool) if valid is None else np.asarray(valid) != 0
    for b, c in enumerate(bands):
        out[:, :, b] = np.where(ok, stretch(img[:, :, c], *pairs[c]), background)
    if alpha:
        out[:, :, len(bands)] = np.where(ok, 255, 0)
    return out


def render(src, sval, sy0, sx0, shift, region, size, bands, pairs, mode="average", nodata=None, alpha=False,
           background=0):
    """src: uint8 / uint16 [sh][sw][C]; sval: None, or the validity window [sh][sw] (then nodata is ignored)"""
    if sval is None:
        img = view_ref.resample(src, sy0, sx0, shift, region, size, mode, nodata if mode == "average" else None)
        return display(img, None, bands, pairs, alpha, background)
    img, oval = valid_ref.resample(src, sval, sy0, sx0, shift, region, size, mode, 0)
    return display(img, oval, bands, pairs, alpha, background)


def histogram(img, valid=None, nodata=None):
    """img: uint8 / uint16 [H][W][C] -> int64 [C][256 or 65536]"""
    bins = 256 if img.dtype == np.uint8 else 65536
    ok = np.ones(img.shape[:2], dtype=bool) if valid is None else np.asarray(valid) != 0
    if nodata is not None:
        ok = ok & ~(img == nodata).all(axis=2)
    return np.stack([np.bincount(img[:, :, c][ok].astype(np.int64), minlength=bins) for c in range(img.shape[2])])


def percentile_stretch(hist, percent=(2, 98)):
    """the rule, value by value, in Python's integers"""
    out = []
    q0, q1 = (int(round(100 * p)) for p in percent)
    for row in np.asarray(hist):
        n = sum(int(k) for k in row)
        pair = []
        for q in (q0, q1):
            cum, pick = 0, 0
            for v, k in enumerate(row):
                cum += int(k)
                if cum >= 1 and 10000 * cum >= q * n:
                    pick = v
                    break
            pair.append(pick if n else 0)
        out.append(tuple(pair))
    return out
