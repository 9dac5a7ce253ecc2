"""Numpy restatement of the bounded-error residual layer for uint16 imagery, written from its definition and
independent of the package (no tests here, nothing of dsic_amd): the predictor p, the quantized residual q, the
reconstruction x', the per-tile shift k with the split into hi and lo, the bit planes, the table formula, and the
layout of the wide residual block and of the version-9 stream.

    p  = lo + uint32(clamp(x_hat,0,1) * float32(R) + 0.5f)    per band, R = hi - lo
    r  = x - p,  s = 2 tau + 1,  q = sign(r) * floor((|r| + tau) / s),  |q| <= Q16 = floor((65535 + tau) / s)
    x' = clamp(p + q s, 0, 65535)
    k  = the least k >= 0 with max |q| <= 255 * 2^k;  hi = q >> k (floor),  lo = q & (2^k - 1)
"""
import struct

import numpy as np

BANDS = 16
BINS = 512
TOP = 255
K_EDGES = [(255, 0), (256, 1), (510, 1), (511, 2), (65280, 8), (65281, 9)]     # (max |q|, k)


def q16_max(tau):
    return (65535 + tau) // (2 * tau + 1)


def shift_for(m):
    k = 0
    while m > 255 * 2 ** k:
        k += 1
    return k


def predictor(x_hat, scale):
    """x_hat float32 [..., C, h, w] (band axis third from the end), scale C pairs (lo, hi) -> int64 of the same
    shape: float32 product and sum, truncated; a NaN clamps to 0."""
    v = np.asarray(x_hat, dtype=np.float32)
    out = np.empty(v.shape, dtype=np.int64)
    for c, (lo, hi) in enumerate(scale):
        b = v[..., c, :, :]
        with np.errstate(invalid="ignore"):
            b = np.where(b > 0, np.where(b > 1, np.float32(1), b), np.float32(0)).astype(np.float32)
        y = (b * np.float32(hi - lo)).astype(np.float32) + np.float32(0.5)
        assert y.dtype == np.float32
        out[..., c, :, :] = y.astype(np.uint32).astype(np.int64) + lo
    return out


def quantize(x, p, tau):
    r = np.asarray(x, dtype=np.int64) - np.asarray(p, dtype=np.int64)
    return np.sign(r) * ((np.abs(r) + tau) // (2 * tau + 1))


def reconstruct(p, q, tau):
    return np.clip(np.asarray(p, dtype=np.int64) + np.asarray(q, dtype=np.int64) * (2 * tau + 1), 0, 65535)


def owned_mask(th, tw, own):
    y0, y1, x0, x1 = own
    m = np.zeros((th, tw), dtype=bool)
    m[y0:y1, x0:x1] = True
    return m


def split(q, k=None):
    """q int64 [C][th][tw] -> (k, hi, lo); k from the tile's own maximum unless given."""
    q = np.asarray(q, dtype=np.int64)
    if k is None:
        k = shift_for(int(np.abs(q).max()))
    return k, q >> k, q & ((1 << k) - 1)


def join(hi, lo, k, tau=None):
    q = (np.asarray(hi, dtype=np.int64) << k) + np.asarray(lo, dtype=np.int64)
    return q if tau is None else np.clip(q, -q16_max(tau), q16_max(tau))


def planes_by_definition(lo, k):
    """lo [C][th][tw] -> bytes: plane j, byte i, bit b = bit j of lo of sample 8 i + b (a plain loop)."""
    flat = [int(v) for v in np.asarray(lo).ravel()]
    out = bytearray()
    for j in range(k):
        for i in range(len(flat) // 8):
            byte = 0
            for b in range(8):
                byte |= ((flat[8 * i + b] >> j) & 1) << b
            out.append(byte)
    return bytes(out)


def planes(lo, k):
    """The same through np.packbits, for sizes where the loop is slow."""
    flat = np.asarray(lo, dtype=np.int64).ravel()
    return b"".join(np.packbits(((flat >> j) & 1).astype(np.uint8), bitorder="little").tobytes() for j in range(k))


def unpack_planes(buf, k, count):
    """k planes of count / 8 bytes -> lo int64 [count]."""
    a = np.frombuffer(buf, dtype=np.uint8).reshape(k, count // 8) if k else np.zeros((0, count // 8), dtype=np.uint8)
    lo = np.zeros(count, dtype=np.int64)
    for j in range(k):
        lo |= np.unpackbits(a[j], bitorder="little").astype(np.int64) << j
    return lo


def histogram(hi):
    """hi [C][th][tw] -> int64 [C][512] at bin hi + 255."""
    return np.stack([np.bincount((plane + TOP).ravel(), minlength=BINS) for plane in np.asarray(hi, dtype=np.int64)])


def table(h, npix):
    """c[j] = floor(cum[j] (65536 - L) / npix) + j in exact integers, h the band's histogram over the support."""
    L, cum, out = len(h), 0, []
    for j in range(L):
        out.append(cum * (65536 - L) // int(npix) + j)
        cum += int(h[j])
    return np.array(out, dtype=np.int64)


def tile_tables(hi):
    """hi [C][th][tw] -> (smin, L, tables int64 [C][L]): the support is min .. max over all bands of the tile."""
    hi = np.asarray(hi, dtype=np.int64)
    smin, L = int(hi.min()), int(hi.max()) - int(hi.min()) + 1
    hist = histogram(hi)
    return smin, L, np.stack([table(hist[c, smin + TOP:smin + TOP + L], hi[c].size) for c in range(hi.shape[0])])


def entropy_bits(values):
    """Empirical entropy in bits per sample of an integer array."""
    _, counts = np.unique(np.asarray(values).ravel(), return_counts=True)
    p = counts / counts.sum()
    return float(-(p * np.log2(p)).sum())


def pack_block(C, th, tw, tau, tiles):
    """tiles: per tile (smin, tables [C][L], k, the k planes as bytes, the 16 strings) -> the wide residual block."""
    head = b"DSICW\x00" + struct.pack("<6I", len(tiles), C, th, tw, tau, BANDS)
    recs, segs, spans = b"", b"", b""
    for smin, tabs, k, pl, strings in tiles:
        assert len(pl) == k * C * th * tw // 8 and len(strings) == BANDS
        span = np.asarray(tabs).astype("<u2").tobytes() + pl + b"".join(strings)
        recs += struct.pack("<iIII", smin, np.asarray(tabs).shape[1], k, len(span))
        segs += struct.pack("<16I", *[len(s) for s in strings])
        spans += span
    return head + recs + segs + spans


def pack_stream_v9(h, blobs, residuals):
    """The version-9 stream: the version-3 head (68 bytes, overlap word 0), C x (lo, hi), tolerance, res_bands, then
    per batch u64 length | container, u64 length | wide residual block."""
    out = struct.pack("<6sHI6I4I2I", b"DSICI\x00", 9, h["numerics"], h["H"], h["W"], h["C"], 2, h["th"], h["tw"],
                      h["N"], h["M"], h["in_ch"], h["spatial_params"], h["batch"], len(blobs))
    out += struct.pack("<2I", h.get("segments", 1), 0)
    for lo, hi in h["scale"]:
        out += struct.pack("<2I", lo, hi)
    out += struct.pack("<2I", h["tolerance"], BANDS)
    for b, r in zip(blobs, residuals):
        out += struct.pack("<Q", len(b)) + b + struct.pack("<Q", len(r)) + r
    return out
