"""Nodata masks of the whole-image codec (codec.compress_image with nodata = v, stream version 5).

A pixel of a uint8 [H,W,C] image is nodata iff all its C channels equal v.  Per grid tile, over the pixels it owns
inside H x W (codec._owned_in_tile; reflect padding and a neighbour's rows or columns never count):

    state 0, empty: all of them are nodata      state 1, full: none is      state 2, mixed: anything else

Empty tiles are not coded at all; a mixed tile carries its mask beside its strings, as a bit plane in tile coordinates:
th*tw bits, row-major, bit y*tw + x in byte (y*tw + x) / 8, LSB first; 1 iff the pixel is owned, inside H x W and
nodata.  What travels is the vertical delta plane d[y][x] = m[y][x] ^ m[y-1][x] (m[-1] = 0) in one of two modes:
mode 0 is d itself, th*tw/8 bytes; mode 1 is the positions y*tw + x of the set bits of d, ascending, u16 little endian
if th*tw <= 65536, else u32.  The encoder writes mode 1 iff it is strictly shorter.  The decoder sets the positions in
an empty plane and takes the XOR prefix down every column; both steps are exact and order-free.

The mask block of a stream (little endian):

    "DSICM\\0" | n u32 | th u32 | tw u32 | nodata u32 | mixed u32 (nm) | n state bytes, zero-padded to a multiple of 4 |
    nm x (tile u32, mode u32, bytes u32), ascending tile | the nm payloads back to back

Set bits outside a tile's owned rectangle are harmless: the apply kernel writes only pixels the tile owns.

A validity mask (codec.compress_image with valid = mask, stream version 8) uses the same states, planes, payloads and
block with "invalid" in the place of "nodata": the mask arrives as a uint8 [H,W] image, 0 = invalid (classify_valid,
delta_planes_valid: the kernels above on a one-channel image whose nodata value is 0; each shares its body with its
nodata twin, _classify and _delta_planes), the block's nodata field carries the fill, apply_window also fills uint16
windows, and window_valid writes a window's validity.  check_nodata and check_fill are ops._int_option, the one
integer-option check of the codec.
"""
from __future__ import annotations

import struct

import numpy as np
import torch

from . import lib as _lib
from .ops import _int_option, _p, _stream

MAGIC = b"DSICM\x00"
EMPTY, FULL, MIXED = 0, 1, 2
MAX_TILES = 1024                   # tiles per kernel call of the plane movers (256 x 256 tiles: 8 MiB of planes)
_HEAD = struct.Struct("<6s5I")     # magic, n, th, tw, nodata, mixed
_REC = struct.Struct("<3I")        # per mixed tile: tile, mode, bytes


def check_nodata(nodata, what) -> int:
    """nodata as an int in 0 .. 255, else ValueError."""
    return _int_option(nodata, "nodata", 255, what)


def raw_bytes(th, tw) -> int:
    """Bytes of a plane, the mode-0 payload."""
    return th * tw // 8


def pos_bytes(th, tw) -> int:
    """Bytes of one position of a mode-1 payload."""
    return 2 if th * tw <= 65536 else 4


def states_bytes(n) -> int:
    return (n + 3) // 4 * 4


def head_bytes(n, mixed) -> int:
    """Bytes of a block in front of its first payload."""
    return _HEAD.size + states_bytes(n) + _REC.size * mixed


def tile_states(counts, owned_pixels) -> list:
    """Nodata counts and owned pixel counts per tile -> states."""
    return [EMPTY if c == p else (FULL if c == 0 else MIXED) for c, p in zip(counts, owned_pixels)]


def pack_block(th, tw, nodata, states, records, payloads) -> bytes:
    """The mask block (pure Python).  states: one of 0, 1, 2 per grid tile; records: (tile, mode, bytes) per mixed
    tile, ascending; payloads: their bytes, one per record or already joined."""
    n = len(states)
    body = payloads if isinstance(payloads, (bytes, bytearray, memoryview)) else b"".join(bytes(p) for p in payloads)
    return b"".join([_HEAD.pack(MAGIC, n, th, tw, nodata, len(records)),
                     bytes(states) + b"\0" * (states_bytes(n) - n)]
                    + [_REC.pack(*(int(v) for v in r)) for r in records] + [bytes(body)])


def read_block_head(read_at, off, size, n, th, tw, nodata, what="DSICI stream"):
    """The head, states and records of the mask block that fills bytes [off, off + size) behind read_at(offset,
    count); the payloads are not read.  n, th, tw, nodata: what the stream's head says the block must hold.  Returns
    (states, {tile: {"m_off", "m_len", "m_mode"}}) with absolute payload offsets.  ValueError where the block
    contradicts the head, is truncated or oversized, holds a state above 2, records that are not exactly the mixed
    tiles in ascending order, a mode above 1, or a length no payload of that mode can have."""
    head = read_at(off, min(size, _HEAD.size))
    if len(head) < _HEAD.size or bytes(head[:6]) != MAGIC:
        raise ValueError(f"{what}: not a mask block" if bytes(head[:6]) != MAGIC[:len(head)]
                         else f"{what}: truncated mask block")
    _, bn, bth, btw, bv, nm = _HEAD.unpack(head)
    if (bn, bth, btw, bv) != (n, th, tw, nodata):
        raise ValueError(f"{what}: mask block of (n, th, tw, nodata) = {(bn, bth, btw, bv)}, the stream's head says "
                         f"{(n, th, tw, nodata)}")
    if nm > n or size < head_bytes(n, nm):
        raise ValueError(f"{what}: truncated mask block")
    states = list(bytes(read_at(off + _HEAD.size, states_bytes(n)))[:n])
    if any(s > MIXED for s in states):
        raise ValueError(f"{what}: mask block with a tile state above 2")
    mixed = [t for t, s in enumerate(states) if s == MIXED]
    if len(mixed) != nm:
        raise ValueError(f"{what}: mask block with {nm} records for {len(mixed)} mixed tiles")
    recs = list(_REC.iter_unpack(read_at(off + _HEAD.size + states_bytes(n), _REC.size * nm)))
    if [r[0] for r in recs] != mixed:
        raise ValueError(f"{what}: the mask records are not the mixed tiles in ascending order")
    raw, ps, pos, out = raw_bytes(th, tw), pos_bytes(th, tw), off + head_bytes(n, nm), {}
    for tile, mode, length in recs:
        if mode > 1:
            raise ValueError(f"{what}: mask of tile {tile} in mode {mode}, this reader knows 0 and 1")
        if mode == 0 and length != raw:
            raise ValueError(f"{what}: raw mask of tile {tile} of {length} bytes, a plane has {raw}")
        if mode == 1 and (length % ps or length >= raw):
            raise ValueError(f"{what}: mask list of tile {tile} of {length} bytes: not a multiple of {ps}, or not "
                             f"shorter than the plane's {raw}")
        out[tile] = {"m_off": pos, "m_len": length, "m_mode": mode}
        pos += length
    if pos != off + size:
        raise ValueError(f"{what}: truncated or oversized mask block")
    return states, out


def check_payload(buf, mode, th, tw, what="DSICI stream"):
    """A mode-1 payload as it arrived, before anything is uploaded: positions strictly ascending and below th*tw."""
    if mode != 1 or not len(buf):
        return
    p = np.frombuffer(buf, dtype="<u2" if pos_bytes(th, tw) == 2 else "<u4").astype(np.int64)
    if p[-1] >= th * tw or (np.diff(p) <= 0).any():
        raise ValueError(f"{what}: mask positions that do not ascend strictly, or leave the {th}x{tw} tile")


# ---- the device side ------------------------------------------------------------------------------------------------
# The nodata calls (dsic_mask_*_u8) and the validity calls (dsic_valid_*) are one body each: `what` names the export,
# channels and value are (C,) and (nodata,) where the export takes them, () where it does not.
def _classify(what, img, g, channels, value) -> np.ndarray:
    fn = getattr(_lib.load(), "dsic_" + what)
    counts = torch.zeros(g["n"], dtype=torch.int32, device=img.device)
    for first in range(0, g["n"], 65535):
        n = min(65535, g["n"] - first)
        _lib.check(fn(_p(img), g["H"], g["W"], *channels, g["th"], g["tw"], *value, first, n, _p(counts[first:]),
                      _stream()), what)
    return counts.cpu().numpy().astype(np.int64)


def _delta_planes(what, img, g, channels, value, ids):
    n = ids.numel()
    planes = torch.empty((n, g["th"] * g["tw"] // 32), dtype=torch.int32, device=img.device)
    pop = torch.zeros(n, dtype=torch.int32, device=img.device)
    _lib.check(getattr(_lib.load(), "dsic_" + what)(_p(img), g["H"], g["W"], *channels, g["th"], g["tw"], *value,
                                                    _p(ids), n, _p(planes), _p(pop), _stream()), what)
    return planes, pop


def classify(img, g, C, nodata) -> np.ndarray:
    """uint8 [H,W,C] on the device -> int64 [n]: per grid tile the nodata pixels among its owned pixels inside H x W.
    One pass over the image (dsic_mask_classify_u8) and one small copy."""
    return _classify("mask_classify_u8", img, g, (C,), (nodata,))


def delta_planes(img, g, C, nodata, ids):
    """ids int32 [n] on the device -> (d planes int32 [n, th*tw/32], popcounts int32 [n])."""
    return _delta_planes("mask_delta_planes_u8", img, g, (C,), (nodata,), ids)


def pack_on_device(planes, pop, ids, th, tw):
    """planes, popcounts, ids of n tiles -> (device buffer: n records, then the payloads; its bytes)."""
    n = ids.numel()
    out = torch.empty(n * (_REC.size + raw_bytes(th, tw)), dtype=torch.uint8, device=planes.device)
    ws = torch.empty(n + 2, dtype=torch.int64, device=planes.device)
    _lib.check(_lib.load().dsic_mask_pack(_p(planes), _p(pop), _p(ids), n, th, tw, _p(ws), _p(out), _stream()),
               "mask_pack")
    return out, int(ws[0].cpu())


def check_fill(fill, top, what) -> int:
    """fill as an int in 0 .. top (255 for uint8 images, 65535 for uint16), else ValueError."""
    return _int_option(fill, "fill", top, what)


def classify_valid(valid, g) -> np.ndarray:
    """uint8 [H,W] on the device, 0 = invalid -> int64 [n]: per grid tile the invalid pixels among its owned pixels
    inside H x W (dsic_valid_classify: classify of a one-channel image whose nodata value is 0)."""
    return _classify("valid_classify", valid, g, (), ())


def delta_planes_valid(valid, g, ids):
    """delta_planes of a validity image (dsic_valid_delta_planes)."""
    return _delta_planes("valid_delta_planes", valid, g, (), (), ids)


@torch.no_grad()
def encode_block(img, g, C, nodata, states) -> bytes:
    """The mask block of an image on the device from its tile states; only the block's bytes leave the device.
    C = None: img is a validity image (uint8 [H,W], 0 = invalid) and nodata the fill the block's field carries."""
    th, tw = g["th"], g["tw"]
    mixed = [t for t, s in enumerate(states) if s == MIXED]
    records, payloads = [], []
    for c0 in range(0, len(mixed), MAX_TILES):
        sel = mixed[c0:c0 + MAX_TILES]
        ids = torch.tensor(sel, dtype=torch.int32).to(img.device)
        planes, pop = delta_planes_valid(img, g, ids) if C is None else delta_planes(img, g, C, nodata, ids)
        out, nbytes = pack_on_device(planes, pop, ids, th, tw)
        host = out[:nbytes].cpu().numpy().tobytes()
        records += list(_REC.iter_unpack(host[:_REC.size * len(sel)]))
        payloads.append(host[_REC.size * len(sel):])
    return pack_block(th, tw, nodata, states, records, b"".join(payloads))


def unpack_planes(d_blob, total, desc, n, th, tw):
    """The uploaded payloads and the device copy of desc int32 [n,3] = (mode, offset, bytes) -> m planes int32
    [n, th*tw/32]."""
    planes = torch.empty((n, th * tw // 32), dtype=torch.int32, device=d_blob.device)
    _lib.check(_lib.load().dsic_mask_unpack(_p(d_blob), total, _p(desc), n, th, tw, _p(planes), _stream()),
               "mask_unpack")
    return planes


def apply_window(planes, n_planes, desc, n, nodata, img, kind_u8, H, W, C, th, tw, y0, x0, h, w):
    """desc int32 [n,2] on the device = (tile, plane index or -1 for all set): nodata (uint8 [h,w,C]) or
    nodata / 255.0f (float32 [C,h,w]) at the tiles' owned pixels inside the window whose bit is set."""
    L = _lib.load()
    fn, what = (L.dsic_mask_apply_u8, "mask_apply_u8") if kind_u8 else (L.dsic_mask_apply_f32, "mask_apply_f32")
    if img.dtype == torch.uint16:                                  # a version-8 stream of a uint16 image: the fill
        fn, what = L.dsic_mask_apply_u16, "mask_apply_u16"
    _lib.check(fn(_p(planes) if planes is not None else None, n_planes, _p(desc), n, nodata, _p(img), H, W, C, th, tw,
                  y0, x0, h, w, _stream()), what)


def window_valid(planes, n_planes, desc, n, out, H, W, th, tw, y0, x0, h, w):
    """desc as apply_window takes it: 1 or 0 into the uint8 [h,w] validity window `out` at every owned pixel of the
    listed tiles inside the window (dsic_mask_window_u8); the pixels of other tiles keep the caller's pre-fill."""
    _lib.check(_lib.load().dsic_mask_window_u8(_p(planes) if planes is not None else None, n_planes, _p(desc), n,
                                               _p(out), H, W, th, tw, y0, x0, h, w, _stream()), "mask_window_u8")
