"""Numpy restatement of the near-lossless residual layer, written from its definition and independent of the package:
the predictor p, the quantized residual q, the reconstruction x', the per-tile support, the table formula, and the
layout of the residual block and of the version-4 stream head."""
import struct

import numpy as np

BANDS = 16
BINS = 512


def q_max(tau):
    return (255 + tau) // (2 * tau + 1)


def lmax(tau):
    return (2 * q_max(tau) + 1 + 7) // 8 * 8


def predictor(x_hat):
    """p = (uint8)(clamp(x_hat, 0, 1) * 255): float32 product, truncated.  x_hat float32, any shape -> int64."""
    v = np.asarray(x_hat, dtype=np.float32)
    v = np.where(v < 0, np.float32(0), np.where(v > 1, np.float32(1), v)).astype(np.float32)
    return (v * np.float32(255.0)).astype(np.float32).astype(np.uint8).astype(np.int64)


def quantize(x, p, tau):
    """x, p integer arrays in 0 .. 255 -> q = sign(r) floor((|r| + tau) / s), r = x - p, s = 2 tau + 1."""
    r = np.asarray(x, dtype=np.int64) - np.asarray(p, dtype=np.int64)
    return np.sign(r) * ((np.abs(r) + tau) // (2 * tau + 1))


def reconstruct(p, q, tau):
    """x' = clamp(p + q s, 0, 255)."""
    return np.clip(np.asarray(p, dtype=np.int64) + np.asarray(q, dtype=np.int64) * (2 * tau + 1), 0, 255)


def owned_mask(th, tw, own):
    y0, y1, x0, x1 = own
    m = np.zeros((th, tw), dtype=bool)
    m[y0:y1, x0:x1] = True
    return m


def tile_q(x_hwc, x_hat_chw, own, tau):
    """One tile: x uint8 [th][tw][C], x_hat float32 [C][th][tw], own (y0, y1, x0, x1) -> q int64 [C][th][tw], 0 at the
    pixels the tile does not own."""
    q = quantize(np.transpose(x_hwc, (2, 0, 1)), predictor(x_hat_chw), tau)
    return np.where(owned_mask(x_hwc.shape[0], x_hwc.shape[1], own)[None], q, 0)


def histogram(q, tau):
    """q [C][th][tw] -> int64 [C][512] at bin q + Q (np.bincount)."""
    Q = q_max(tau)
    return np.stack([np.bincount((plane + Q).ravel(), minlength=BINS) for plane in q])


def support(q):
    """(smin, L) of a tile: min .. max of q over all its channels."""
    return int(q.min()), int(q.max()) - int(q.min()) + 1


def table(h, npix):
    """h: the histogram of one channel over the support (length L, python ints or int64) -> c[0 .. L-1] with
    c[k] = floor(cum[k] (65536 - L) / npix) + k in exact integers."""
    L, cum, out = len(h), 0, []
    for k in range(L):
        out.append(cum * (65536 - L) // int(npix) + k)
        cum += int(h[k])
    return np.array(out, dtype=np.int64)


def tile_tables(q, tau):
    """q [C][th][tw] -> (smin, L, tables int64 [C][L])."""
    smin, L = support(q)
    Q, hist = q_max(tau), histogram(q, tau)
    return smin, L, np.stack([table(hist[c, smin + Q:smin + Q + L], q[c].size) for c in range(q.shape[0])])


def code_bits(h, c, npix):
    """Ideal code length in bits per symbol of table c (c[L] = 65536 implicit) under the histogram h."""
    width = np.diff(np.append(np.asarray(c, dtype=np.float64), 65536.0))
    h = np.asarray(h, dtype=np.float64)
    return float(-(h[h > 0] * np.log2(width[h > 0] / 65536.0)).sum() / npix)


def entropy_bits(h, npix):
    h = np.asarray(h, dtype=np.float64)
    h = h[h > 0]
    return float(-(h * np.log2(h / npix)).sum() / npix)


def pack_block(C, th, tw, tau, tiles):
    """tiles: per tile (smin, tables [C][L], the 16 strings) -> the residual block."""
    head = b"DSICR\x00" + struct.pack("<6I", len(tiles), C, th, tw, tau, BANDS)
    recs, segs, spans = b"", b"", b""
    for smin, tabs, strings in tiles:
        span = np.asarray(tabs).astype("<u2").tobytes() + b"".join(strings)
        recs += struct.pack("<iII", smin, np.asarray(tabs).shape[1], len(span))
        segs += struct.pack("<16I", *[len(s) for s in strings])
        spans += span
    return head + recs + segs + spans


def pack_stream_v4(h, blobs, residuals):
    """The version-4 stream: the version-3 head (68 bytes, overlap word 0), max_error, res_bands, then per batch
    u64 length | container, u64 length | residual block."""
    out = struct.pack("<6sHI6I4I2I", b"DSICI\x00", 4, h["numerics"], h["H"], h["W"], h["C"], h["kind"], h["th"], h["tw"],
                      h["N"], h["M"], h["in_ch"], h["spatial_params"], h["batch"], len(blobs))
    out += struct.pack("<4I", h.get("segments", 1), 0, h["max_error"], BANDS)
    for b, r in zip(blobs, residuals):
        out += struct.pack("<Q", len(b)) + b + struct.pack("<Q", len(r)) + r
    return out
