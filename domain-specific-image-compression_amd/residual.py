"""Near-lossless residual layer of the whole-image codec (codec.compress_image with max_error = tau).

The decoder's x_hat equals the encoder's forward x_hat bit for bit, so the lossy uint8 image p =
(uint8)(clamp(x_hat,0,1)*255) is a predictor both sides share.  Per tile the encoder codes, beside the lossy strings,

    r = x - p,   s = 2 tau + 1,   q = sign(r) * floor((|r| + tau) / s),   |q| <= Q = floor((255 + tau) / s)

(q = 0 at pixels the tile does not own) and the decoder writes x' = clamp(p + q s, 0, 255), so |x' - x| <= tau on every
pixel and channel; tau = 0 is lossless.  q is coded by the project's range coder with one static table per (tile,
colour channel), built from the tile's own histogram and sent in the stream:

    support [smin, smin + L) = min .. max of q over all channels of the tile
    c[k] = floor(cum[k] * (65536 - L) / (th tw)) + k,  k < L;  c[L] = 65536 implicit

The q plane of a tile, float32 [C][th][tw], is the coder's NCHW latent [C 16][(th / 16) tw] as it lies: 16 row bands
per colour plane, coded as BANDS = 16 independent segments that a decoder reads on 16 waves.

The residual block of a batch (little endian):

    "DSICR\\0" | n, C, th, tw, tau, bands u32 | n x (smin i32, L u32, span_bytes u32) | n x bands u32 segment lengths |
    per tile its span: C x L uint16 table entries, then the 16 segment strings
"""
from __future__ import annotations

import collections
import struct

import numpy as np
import torch

from . import lib as _lib
from .ops import _int_option, _p, _stream

MAGIC = b"DSICR\x00"
BANDS = 16
BINS = 512
MAX_TILES = 3000                   # tiles per kernel call (dsic_residual_*)
_HEAD = struct.Struct("<6s6I")     # magic, n, C, th, tw, tau, bands
_REC = struct.Struct("<iII")       # per tile: smin, L, span_bytes


def check_max_error(max_error, what) -> int:
    """max_error as an int in 0 .. 127, else ValueError."""
    return _int_option(max_error, "max_error", 127, what, " (lossless)")


def q_max(tau) -> int:
    """Q: the largest |q| at step 2 tau + 1."""
    return (255 + tau) // (2 * tau + 1)


def table_lmax(tau) -> int:
    """Row length of the residual's coder tables: ceil8(2 Q + 1), known from tau alone."""
    return (2 * q_max(tau) + 1 + 7) // 8 * 8


# ---- one block format, two widths: this module's DSICR block and residual16's DSICW block -------------------------
# magic | n, C, th, tw, tau, bands u32 | n x (smin i32, L u32, [k u32,] span_bytes u32) | n x 16 u32 segment lengths |
# per tile its span: C x L uint16 tables | [k planes of C th tw / 8 bytes] | the 16 segment strings
# rec: the record's struct; name: the block in messages; top(tau): the bound on the support, |symbol| <= top; planes:
# the largest k, 0 for a block whose records carry no k and whose spans no planes
BlockFormat = collections.namedtuple("BlockFormat", "magic rec name top planes")
FORMAT = BlockFormat(MAGIC, _REC, "residual", q_max, 0)


def _bytes_of(v, dtype):
    return v if isinstance(v, (bytes, bytearray, memoryview)) else np.ascontiguousarray(v, dtype=dtype).tobytes()


def format_head_bytes(fmt, n) -> int:
    return _HEAD.size + (fmt.rec.size + 4 * BANDS) * n


def format_pack_block(fmt, C, th, tw, tau, tiles) -> bytes:
    """A block of a batch (pure Python).  tiles: per tile (smin, tables, strings), with planes (smin, tables, k, planes,
    strings)."""
    recs, segs, spans = [], [], []
    pb = C * th * tw // 8
    for smin, tables, *kp, strings in tiles:
        tb, (k, pl) = _bytes_of(tables, "<u2"), (kp[0], _bytes_of(kp[1], np.uint8)) if fmt.planes else (0, b"")
        if len(strings) != BANDS or len(tb) % (2 * C) or len(pl) != k * pb:
            raise ValueError(f"pack_block: a tile takes {C} tables of one width" +
                             (f", k planes of {pb} bytes" if fmt.planes else "") + f" and {BANDS} strings")
        span = bytes(tb) + bytes(pl) + b"".join(bytes(s) for s in strings)
        recs.append(fmt.rec.pack(int(smin), len(tb) // (2 * C), *([int(k)] if fmt.planes else []), len(span)))
        segs.append(struct.pack(f"<{BANDS}I", *[len(s) for s in strings]))
        spans.append(span)
    return b"".join([_HEAD.pack(fmt.magic, len(tiles), C, th, tw, tau, BANDS)] + recs + segs + spans)


def format_read_block_head(fmt, read_at, off, size, n, C, th, tw, tau, what):
    """The head, records and segment lengths of the block that fills bytes [off, off + size) behind read_at(offset,
    count); the spans are not read.  n, C, th, tw, tau: what the stream's head says the block must hold.  Returns per
    tile {"r_off", "r_len", "r_smin", "r_L", "r_segs"} and, with planes, "r_k": the absolute offset and length of its
    span, its support, its shift, and the lengths of its 16 strings, which follow the span's C * r_L table entries and
    r_k planes back to back.  ValueError where the block contradicts the head, is truncated, or a record cannot be a
    tile's."""
    name = fmt.name
    head = read_at(off, min(size, _HEAD.size))
    if len(head) < _HEAD.size or bytes(head[:6]) != fmt.magic:
        raise ValueError(f"{what}: not a {name} block" if bytes(head[:6]) != fmt.magic[:len(head)]
                         else f"{what}: truncated {name} block")
    _, bn, bC, bth, btw, btau, bands = _HEAD.unpack(head)
    if bands != BANDS:
        raise ValueError(f"{what}: {name} block with {bands} bands, this reader knows {BANDS}")
    if (bn, bC, bth, btw, btau) != (n, C, th, tw, tau):
        raise ValueError(f"{what}: {name} block of (n, C, th, tw, tau) = {(bn, bC, bth, btw, btau)}, the stream's "
                         f"head says {(n, C, th, tw, tau)}")
    if size < format_head_bytes(fmt, n):
        raise ValueError(f"{what}: truncated {name} block")
    recs = list(fmt.rec.iter_unpack(read_at(off + _HEAD.size, fmt.rec.size * n)))
    flat = struct.unpack(f"<{BANDS * n}I", read_at(off + _HEAD.size + fmt.rec.size * n, 4 * BANDS * n))
    Q, pb, pos, out = fmt.top(tau), C * th * tw // 8, off + format_head_bytes(fmt, n), []
    for t, rec in enumerate(recs):
        smin, L, k, span = rec if fmt.planes else (rec[0], rec[1], 0, rec[2])
        segs = list(flat[t * BANDS:(t + 1) * BANDS])
        if k > fmt.planes:
            raise ValueError(f"{what}: residual shift k={k} of tile {t} (0 .. {fmt.planes})")
        if fmt.planes and (L < 1 or L > 2 * Q + 1):
            raise ValueError(f"{what}: residual table width L={L} of tile {t} (1 .. {2 * Q + 1})")
        if L < 1 or L > 2 * Q + 1 or smin < -Q or smin + L - 1 > Q:
            raise ValueError(f"{what}: residual support [{smin}, {smin + L}) of tile {t} leaves [-{Q}, {Q}]")
        if span != 2 * C * L + k * pb + sum(segs):
            raise ValueError(f"{what}: residual tile {t}: tables{', planes' if fmt.planes else ''} and segment lengths "
                             "do not add up to its span")
        out.append({"r_off": pos, "r_len": span, "r_smin": smin, "r_L": L, "r_segs": segs})
        if fmt.planes:
            out[-1]["r_k"] = k
        pos += span
    if pos != off + size:
        raise ValueError(f"{what}: truncated or oversized {name} block")
    return out


def format_check_tables(fmt, buf, C, L, tau, what):
    """The C tables of a span (2 C L bytes): c[0] = 0, strictly increasing, L <= 2 top + 1; else ValueError."""
    if L < 1 or L > 2 * fmt.top(tau) + 1 or len(buf) != 2 * C * L:
        raise ValueError(f"{what}: residual tables of width {L}" + ("" if fmt.planes else f" for max_error={tau}"))
    t = np.frombuffer(buf, dtype="<u2").reshape(C, L).astype(np.int64)
    if (t[:, 0] != 0).any() or (np.diff(t, axis=1) <= 0).any():
        raise ValueError(f"{what}: a residual table does not start at 0 or is not strictly increasing")


def decode_spec(layer, recs, C, th, tw, tau, at, tables_of) -> dict:
    """What layer.control_words and layer.decode_q take for one decode batch (layer: this module or residual16).  recs:
    the tiles' index records; at(offset, length): where a stream range lies in the upload; tables_of(rec): the tables
    of its span as they arrived, which are checked here, before anything is uploaded."""
    fmt = layer.FORMAT
    for r in recs:
        format_check_tables(fmt, tables_of(r), C, r["r_L"], tau, "DSICI stream")
    pb = C * th * tw // 8
    tables = [(at(r["r_off"], r["r_len"]), 2 * C * r["r_L"]) for r in recs]
    ks = [r.get("r_k", 0) for r in recs]
    spec = {"layer": layer, "C": C, "th": th, "tw": tw, "tau": tau, "smin": [r["r_smin"] for r in recs],
            "L": [r["r_L"] for r in recs], "segs": [r["r_segs"] for r in recs],
            "desc": [(a, tb, a + tb + k * pb, sum(r["r_segs"])) for (a, tb), k, r in zip(tables, ks, recs)]}
    if fmt.planes:
        spec.update(k=ks, plane_off=[a + tb for a, tb in tables])
    return spec


def head_bytes(n) -> int:
    """Bytes of a block in front of its first span: head, records, segment lengths."""
    return format_head_bytes(FORMAT, n)


def pack_block(C, th, tw, tau, tiles) -> bytes:
    """The residual block of a batch (pure Python).  tiles: per tile (smin, tables, strings): tables a uint16 array
    [C][L] (or its bytes), strings the 16 segment strings."""
    return format_pack_block(FORMAT, C, th, tw, tau, tiles)


def read_block_head(read_at, off, size, n, C, th, tw, tau, what="DSICI stream"):
    """format_read_block_head for the residual block: per tile {"r_off", "r_len", "r_smin", "r_L", "r_segs"}."""
    return format_read_block_head(FORMAT, read_at, off, size, n, C, th, tw, tau, what)


def check_tables(buf, C, L, tau, what="DSICI stream"):
    """The C tables of a span (2 C L bytes): c[0] = 0, strictly increasing, L <= 2 Q + 1; else ValueError."""
    format_check_tables(FORMAT, buf, C, L, tau, what)


def _shape(tiles, what):
    n, th, tw, C = tiles.shape
    if n > MAX_TILES:
        raise ValueError(f"{what}: {n} tiles in one batch, the residual kernels take {MAX_TILES}")
    return n, th, tw, C


def quantize(tiles, x_hat, own, tau):
    """tiles uint8 [n,th,tw,C], x_hat float32 [n,C,th,tw], own int32 [n,4] (device) -> (q float32 [n,C,th,tw], hist
    int32 [n,C,512] at bin q + Q)."""
    n, th, tw, C = _shape(tiles, "residual.quantize")
    q = torch.empty((n, C, th, tw), dtype=torch.float32, device=tiles.device)
    hist = torch.zeros((n, C, BINS), dtype=torch.int32, device=tiles.device)
    _lib.check(_lib.load().dsic_residual_quantize_u8(_p(tiles), _p(x_hat), _p(own), n, C, th, tw, tau, _p(q),
                                                     _p(hist), _stream()), "residual_quantize_u8")
    return q, hist


def tables(hist, th, tw, tau):
    """hist int32 [n,C,512] -> (meta int32 [n,4] = (smin, L, 0, 1), compact uint16 [n,C,Lmax], coder uint16
    [n,C*16,Lmax])."""
    n, C, _ = hist.shape
    Lmax, dev = table_lmax(tau), hist.device
    meta = torch.empty((n, 4), dtype=torch.int32, device=dev)
    compact = torch.empty((n, C, Lmax), dtype=torch.uint16, device=dev)
    coder = torch.empty((n, C * BANDS, Lmax), dtype=torch.uint16, device=dev)
    _lib.check(_lib.load().dsic_residual_tables(_p(hist), n, C, th, tw, tau, Lmax, _p(meta), _p(compact), _p(coder),
                                                _stream()), "residual_tables")
    return meta, compact, coder


def encode(q, meta, coder, tau):
    """The q planes [n,C,th,tw] through the range encoder (dsic_range_encode_seg_ws) as its y family of C*16 channels
    in 16 segments, beside a one-symbol dummy z family -> dict(bytes uint8 [n, cap_z + 16 cap_seg], lengths int32
    [n,17] (dummy, segment 0 .. 15), cap_z, cap_seg, err)."""
    from . import entropy
    n, C, th, tw = q.shape
    dev, Lmax = q.device, table_lmax(tau)
    M, HW = C * BANDS, th // BANDS * tw
    cap_seg, cap_z = entropy._cap(M * HW // BANDS), 8
    out = torch.zeros((n, (cap_z + BANDS * cap_seg) // 4), dtype=torch.int32, device=dev).view(torch.uint8)
    lengths = torch.zeros((n, 1 + BANDS), dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    z = torch.zeros((n, 1), dtype=torch.float32, device=dev)            # the dummy: symbol 0 of the support [0, 1)
    tab_z = torch.zeros((n, 1, Lmax), dtype=torch.uint16, device=dev)
    L = _lib.load()
    nbytes = L.dsic_range_encode_seg_workspace_size(n, M, HW, 1, 1, BANDS)
    ws = torch.empty(((nbytes + 3) // 4,), dtype=torch.int32, device=dev)
    _lib.check(L.dsic_range_encode_seg_ws(_p(q), _p(z), _p(meta), _p(coder), _p(tab_z), Lmax, n, M, HW, 1, 1, _p(out),
                                          cap_seg, cap_z, _p(lengths), _p(err), 0, BANDS, _p(ws), ws.numel() * 4,
                                          _stream()), "range_encode_seg_ws(residual)")
    return {"bytes": out, "lengths": lengths, "cap_z": cap_z, "cap_seg": cap_seg, "err": err}


def pack_on_device(c, meta, compact, C, th, tw, tau):
    """encode's outputs -> (the residual block in a device buffer, its size, the coder's error word); size and error
    word come back in one 16-byte copy."""
    n = c["bytes"].shape[0]
    Lmax, dev = table_lmax(tau), c["bytes"].device
    out = torch.empty(head_bytes(n) + n * (2 * C * Lmax + BANDS * c["cap_seg"]), dtype=torch.uint8, device=dev)
    ws = torch.empty((C + BANDS) * n + 3, dtype=torch.int64, device=dev)
    _lib.check(_lib.load().dsic_residual_pack(_p(c["bytes"]), c["cap_z"], c["cap_seg"], _p(c["lengths"]), _p(meta),
                                              _p(compact), _p(c["err"]), n, C, th, tw, tau, Lmax, _p(ws), _p(out),
                                              _stream()), "residual_pack")
    nbytes, code = (int(v) for v in ws[:2].cpu())
    return out, nbytes, code


@torch.no_grad()
def encode_block(tiles, x_hat, own, tau) -> bytes:
    """The residual block of one batch: tiles uint8 [n,th,tw,C] (device), x_hat the forward reconstruction of the same
    batch [n,C,th,tw], own per tile (y0, y1, x0, x1), the rectangle of the tile that it owns inside the image.  Only
    the block's bytes leave the device."""
    from . import entropy
    n, th, tw, C = _shape(tiles, "residual.encode_block")
    own_d = torch.tensor(own, dtype=torch.int32).reshape(n, 4).to(tiles.device)
    q, hist = quantize(tiles, x_hat.contiguous(), own_d, tau)
    meta, compact, coder = tables(hist, th, tw, tau)
    c = encode(q, meta, coder, tau)
    out, nbytes, code = pack_on_device(c, meta, compact, C, th, tw, tau)
    entropy._raise_err(code, "compress_image (residual layer)")
    return out[:nbytes].cpu().numpy().tobytes()


def control_words(spec) -> np.ndarray:
    """What decode_q reads on the device, as int64 words for the upload's control block: descriptors [n][4] (tables
    offset, tables bytes, strings offset, strings bytes inside the uploaded bytes), then int32 meta [n][4] (smin, L,
    0, 1) and int32 [n][16] segment lengths."""
    n = len(spec["desc"])
    words = np.zeros(4 * n + 2 * n + BANDS // 2 * n, dtype=np.int64)
    words[:4 * n] = np.asarray(spec["desc"], dtype=np.int64).ravel()
    meta = words[4 * n:6 * n].view(np.int32).reshape(n, 4)
    meta[:, 0], meta[:, 1], meta[:, 2], meta[:, 3] = spec["smin"], spec["L"], 0, 1
    words[6 * n:].view(np.int32)[:] = np.asarray(spec["segs"], dtype=np.int32).ravel()
    return words


def decode_q(d_blob, total, words, spec):
    """The q planes float32 [n,C,th,tw] of one decode batch.  d_blob: the uploaded bytes (entropy._upload_padded),
    words: the device copy of control_words(spec).  The spans are spread by the select mover (tables as its first
    family, strings as its second), the compact tables replicated to the 16 band rows, and the strings decoded by
    dsic_range_decode_seg on 16 waves per tile."""
    from . import entropy
    n, C, th, tw, tau = len(spec["desc"]), spec["C"], spec["th"], spec["tw"], spec["tau"]
    dev, Lmax, L = d_blob.device, table_lmax(tau), _lib.load()
    desc = np.asarray(spec["desc"], dtype=np.int64).reshape(n, 4)
    tmax, smax = int(desc[:, 1].max()), int(desc[:, 3].max())
    tstride, sstride = max(4, (tmax + 3) // 4 * 4), max(4, (smax + 3) // 4 * 4)
    tbuf = torch.zeros(n * tstride, dtype=torch.uint8, device=dev)
    sbuf = torch.empty(n * sstride, dtype=torch.uint8, device=dev)
    lengths = torch.empty((n, 2), dtype=torch.int32, device=dev)
    _lib.check(L.dsic_strings_scatter_select(_p(d_blob), total, _p(words), n, max(tmax, smax), _p(tbuf), tstride,
                                             _p(sbuf), sstride, _p(lengths), _stream()),
               "strings_scatter_select(residual)")
    meta = words[4 * n:6 * n].view(torch.int32).view(n, 4)
    segs = words[6 * n:].view(torch.int32)
    # compact [C][L] per tile -> the coder's rows [C 16][Lmax]: entry k of colour c is word c L + k of the tile
    width = meta[:, 1].to(torch.int64).view(n, 1, 1)
    k = torch.arange(Lmax, device=dev).view(1, 1, Lmax)
    idx = (torch.arange(C, device=dev).view(1, C, 1) * width + torch.minimum(k, width - 1)).clamp_(0, tstride // 2 - 1)
    rows = torch.gather(tbuf.view(torch.int16).view(n, tstride // 2), 1, idx.view(n, C * Lmax)).view(n, C, Lmax)
    coder = torch.repeat_interleave(rows, BANDS, dim=1).contiguous()
    q = torch.empty((n, C, th, tw), dtype=torch.float32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.check(L.dsic_range_decode_seg(_p(sbuf), sstride, _p(lengths), 2, 1, _p(segs), BANDS, _p(meta), 0, _p(coder),
                                       Lmax, n, C * BANDS, th // BANDS * tw, 0, _p(q), _p(err), _stream()),
               "range_decode_seg(residual)")
    entropy._check_err(err, "residual layer")
    return q


def stitch_window_u8(x_hat, q, tau, ids, img, H, W, C, th, tw, y0, x0, h, w):
    """dsic_tile_stitch_window_u8 with the residual added: clamp(p + q (2 tau + 1), 0, 255) into the window image."""
    _lib.check(_lib.load().dsic_tile_stitch_window_u8_res(_p(x_hat), _p(q), tau, _p(ids), x_hat.shape[0], _p(img), H,
                                                          W, C, th, tw, y0, x0, h, w, _stream()),
               "tile_stitch_window_u8_res")


OUT, stitch_window = "u8", stitch_window_u8    # what codec._assemble_window asks of a layer: its image, and its stitch
