"""Bounded-error residual layer for uint16 imagery (codec.compress_image with tolerance = tau, stream version 9): the
uint16 sibling of residual.py, whose max_error mode stays uint8-only.

The decoder's x_hat equals the encoder's forward x_hat bit for bit, so the lossy uint16 image p = denorm(x_hat) =
lo + uint32(clamp(x_hat,0,1) * float32(R) + 0.5f) is a predictor both sides share.  Per tile the encoder codes

    r = x - p,   s = 2 tau + 1,   q = sign(r) * floor((|r| + tau) / s),   |q| <= Q16 = floor((65535 + tau) / s)

(q = 0 at pixels the tile does not own) and the decoder writes x' = clamp(p + q s, 0, 65535), so |x' - x| <= tau on every
pixel and band; tau = 0 returns the image itself, whatever the scale (lo, hi): the scale only shapes the predictor, and
so the rate.  q has up to 131 071 values, too many for the range coder's 16-bit tables, so it is split per tile.  With
m = max |q| over the tile's bands and k the least k >= 0 with m <= 255 * 2^k (0 .. 9):

    hi = q >> k (arithmetic shift, floor) in [-255, 255],   lo = q & (2^k - 1),   q = (hi << k) + lo

hi is coded as residual.py codes its q at tau = 0: histogram at bin hi + 255 of 512, support [smin, smin + L) over the
tile's bands, c[j] = floor(cum[j] (65536 - L) / (th tw)) + j in rows of 512, 16 row bands per plane as 16 segments.  lo
travels raw as k bit planes of C th tw / 8 bytes: bit b of byte i of plane j is bit j of lo of sample 8 i + b, samples in
[C][th][tw] order.  Known limitation: k follows the tile's maximum, so one outlier in a quiet tile costs k raw bits on
every sample of the tile, unowned pixels included.

The wide residual block of a batch (little endian):

    "DSICW\\0" | n, C, th, tw, tau, bands u32 | n x (smin i32, L u32, k u32, span_bytes u32) | n x 16 u32 segment lengths |
    per tile its span: C x L uint16 tables | k planes of C th tw / 8 bytes | the 16 segment strings
"""
from __future__ import annotations

import struct

import numpy as np
import torch

from . import lib as _lib
from . import residual as _residual
from .ops import _int_option, _p, _stream

MAGIC = b"DSICW\x00"
BANDS = _residual.BANDS
BINS = _residual.BINS
TOP = 255                          # |hi| <= TOP
LMAX = 512                         # rows of the coder tables: residual.table_lmax(0)
PLANES = 9                         # the largest shift
MAX_TOLERANCE = 32767
MAX_TILES = _residual.MAX_TILES
_REC = struct.Struct("<iIII")      # per tile: smin, L, k, span_bytes
FORMAT = _residual.BlockFormat(MAGIC, _REC, "wide residual", lambda tau: TOP, PLANES)


def check_tolerance(tolerance, what) -> int:
    """tolerance as an int in 0 .. 32767, else ValueError."""
    return _int_option(tolerance, "tolerance", MAX_TOLERANCE, what, " (lossless)")


def q16_max(tau) -> int:
    """Q16: the largest |q| at step 2 tau + 1."""
    return (65535 + tau) // (2 * tau + 1)


def shift_for(maxabs) -> int:
    """k: the least k >= 0 with maxabs <= 255 * 2^k."""
    k = 0
    while maxabs > TOP << k:
        k += 1
    return k


def plane_bytes(C, th, tw) -> int:
    return C * th * tw // 8


def head_bytes(n) -> int:
    """Bytes of a block in front of its first span: head, records, segment lengths."""
    return _residual.format_head_bytes(FORMAT, n)


def pack_block(C, th, tw, tau, tiles) -> bytes:
    """The wide residual block of a batch (pure Python).  tiles: per tile (smin, tables, k, planes, strings): tables a
    uint16 array [C][L] (or its bytes), planes the k bit planes back to back (bytes, or a uint8 array), strings the 16
    segment strings."""
    return _residual.format_pack_block(FORMAT, C, th, tw, tau, tiles)


def read_block_head(read_at, off, size, n, C, th, tw, tau, what="DSICI stream"):
    """residual.format_read_block_head for the wide residual block: per tile {"r_off", "r_len", "r_smin", "r_L", "r_k",
    "r_segs"}, the support being that of hi and r_k the tile's shift."""
    return _residual.format_read_block_head(FORMAT, read_at, off, size, n, C, th, tw, tau, what)


def check_tables(buf, C, L, what="DSICI stream"):
    """The C tables of a span (2 C L bytes): c[0] = 0, strictly increasing, L <= 511; else ValueError."""
    _residual.format_check_tables(FORMAT, buf, C, L, None, what)


def quantize(img, x_hat, H, W, th, tw, lohi, tau, first):
    """img uint16 [H,W,C] (device), x_hat float32 [n,C,th,tw] of tiles first .. first + n - 1, lohi the scale as the
    uint16 kernels take it -> (q int32 [n,C,th,tw], maxabs int32 [n])."""
    n, C = x_hat.shape[:2]
    if n > MAX_TILES:
        raise ValueError(f"residual16.quantize: {n} tiles in one batch, the residual kernels take {MAX_TILES}")
    q = torch.empty((n, C, th, tw), dtype=torch.int32, device=img.device)
    maxabs = torch.zeros(n, dtype=torch.int32, device=img.device)
    _lib.check(_lib.load().dsic_residual_quantize_u16(_p(img), _p(x_hat), H, W, C, th, tw, lohi, tau, first, n, _p(q),
                                                      _p(maxabs), _stream()), "residual_quantize_u16")
    return q, maxabs


def split(q, maxabs):
    """q int32 [n,C,th,tw], maxabs int32 [n] -> (hi float32 [n,C,th,tw], hist int32 [n,C,512] at bin hi + 255, k int32
    [n], planes int64 [n,9,C th tw / 64] of which the first k[t] of tile t are written)."""
    n, C, th, tw = q.shape
    dev = q.device
    hi = torch.empty((n, C, th, tw), dtype=torch.float32, device=dev)
    hist = torch.zeros((n, C, BINS), dtype=torch.int32, device=dev)
    k = torch.empty(n, dtype=torch.int32, device=dev)
    planes = torch.empty((n, PLANES, C * th * tw // 64), dtype=torch.int64, device=dev)
    _lib.check(_lib.load().dsic_residual_split_u16(_p(q), _p(maxabs), n, C, th, tw, _p(hi), _p(hist), _p(k), _p(planes),
                                                   _stream()), "residual_split_u16")
    return hi, hist, k, planes


def tables(hist, th, tw):
    """hist int32 [n,C,512] -> (meta int32 [n,4] = (smin, L, 0, 1), compact uint16 [n,C,512], coder uint16
    [n,C*16,512])."""
    n, C, _ = hist.shape
    dev = hist.device
    meta = torch.empty((n, 4), dtype=torch.int32, device=dev)
    compact = torch.empty((n, C, LMAX), dtype=torch.uint16, device=dev)
    coder = torch.empty((n, C * BANDS, LMAX), dtype=torch.uint16, device=dev)
    _lib.check(_lib.load().dsic_residual_tables_u16(_p(hist), n, C, th, tw, _p(meta), _p(compact), _p(coder), _stream()),
               "residual_tables_u16")
    return meta, compact, coder


def pack_on_device(c, meta, k, compact, planes, C, th, tw, tau):
    """residual.encode's outputs for hi, with the tile shifts and planes -> (the wide residual block in a device buffer,
    its size, the coder's error word); size and error word come back in one 16-byte copy."""
    n = c["bytes"].shape[0]
    dev = c["bytes"].device
    out = torch.empty(head_bytes(n) + n * (2 * C * LMAX + PLANES * plane_bytes(C, th, tw) + BANDS * c["cap_seg"]),
                      dtype=torch.uint8, device=dev)
    ws = torch.empty((C + 1 + BANDS) * n + 3, dtype=torch.int64, device=dev)
    _lib.check(_lib.load().dsic_residual_pack_u16(_p(c["bytes"]), c["cap_z"], c["cap_seg"], _p(c["lengths"]), _p(meta),
                                                  _p(k), _p(compact), _p(planes), _p(c["err"]), n, C, th, tw, tau,
                                                  _p(ws), _p(out), _stream()), "residual_pack_u16")
    nbytes, code = (int(v) for v in ws[:2].cpu())
    return out, nbytes, code


@torch.no_grad()
def encode_block(img, x_hat, H, W, th, tw, lohi, tau, first) -> bytes:
    """The wide residual block of one batch: img the uint16 [H,W,C] image on the device, read in place, x_hat the
    forward reconstruction [n,C,th,tw] of tiles first .. first + n - 1 of its grid.  Only the block's bytes leave the
    device."""
    from . import entropy
    C = x_hat.shape[1]
    q, maxabs = quantize(img, x_hat.contiguous(), H, W, th, tw, lohi, tau, first)
    hi, hist, k, planes = split(q, maxabs)
    meta, compact, coder = tables(hist, th, tw)
    c = _residual.encode(hi, meta, coder, 0)
    out, nbytes, code = pack_on_device(c, meta, k, compact, planes, C, th, tw, tau)
    entropy._raise_err(code, "compress_image (residual layer)")
    return out[:nbytes].cpu().numpy().tobytes()


def control_words(spec) -> np.ndarray:
    """What decode_q reads on the device, as int64 words for the upload's control block: residual.control_words for hi
    (descriptors, meta, segment lengths), then int64 [n] plane offsets inside the uploaded bytes and int32 [n] shifts."""
    n = len(spec["desc"])
    words = np.zeros(n + (n + 1) // 2, dtype=np.int64)
    words[:n] = np.asarray(spec["plane_off"], dtype=np.int64)
    words[n:].view(np.int32)[:n] = np.asarray(spec["k"], dtype=np.int32)
    return np.concatenate([_residual.control_words(spec), words])


def decode_q(d_blob, total, words, spec):
    """The q planes float32 [n,C,th,tw] of one decode batch: hi by residual.decode_q at tau = 0, then joined with the
    planes, which are read where they lie in the uploaded bytes (dsic_residual_join_u16), and clamped to +-Q16."""
    n, C, th, tw, tau = len(spec["desc"]), spec["C"], spec["th"], spec["tw"], spec["tau"]
    base = 6 * n + BANDS // 2 * n
    hi = _residual.decode_q(d_blob, total, words[:base], dict(spec, tau=0))
    q = torch.empty_like(hi)
    _lib.check(_lib.load().dsic_residual_join_u16(_p(hi), _p(d_blob), total, _p(words[base:base + n]),
                                                  _p(words[base + n:].view(torch.int32)), n, C, th, tw, tau, _p(q),
                                                  _stream()), "residual_join_u16")
    return q


def stitch_window_u16(x_hat, q, tau, ids, img, H, W, C, th, tw, y0, x0, h, w, lohi):
    """dsic_tile_stitch_window_u16 with the residual added: clamp(denorm(x_hat) + q (2 tau + 1), 0, 65535)."""
    _lib.check(_lib.load().dsic_tile_stitch_window_u16_res(_p(x_hat), _p(q), tau, _p(ids), x_hat.shape[0], _p(img), H,
                                                           W, C, th, tw, y0, x0, h, w, lohi, _stream()),
               "tile_stitch_window_u16_res")


OUT, stitch_window = "u16", stitch_window_u16
