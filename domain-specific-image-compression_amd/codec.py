"""Whole-image codec: an image of any size -> one byte stream -> the image, at its own size.

The reference's driver (code/modelv2/eval_selfcontained_entropy.py:126-159) codes one PNG in one forward pass and
needs no size bookkeeping because its images are multiples of 16.  Here an image is cut into tiles of the size the
codec is tuned for (256 x 256, batches of 64), each batch becomes one DSIC2 container (entropy.compress_to_container),
and the containers travel in one stream with the image's geometry:

    magic "DSICI\\0" | version u16 | numerics tag u32 | H, W, C, kind, th, tw u32 | N, M, in_ch, spatial_params u32 |
    batch, batches u32 | per batch: u64 length, DSIC2 container            (little endian, fixed-size fields)

kind 0 = uint8 [H,W,C] (PIL / numpy layout), 1 = float32 [C,H,W] in [0,1].  Tiling (tile_grid): the image is
reflect-padded bottom/right to multiples of 16 inside the gather kernel; the last row / column of tiles shifts inward
(overlap, no extra padding) and every pixel is written back by the one tile that owns it.  Tiles are coded
independently, as the reference's patch-trained model sees them; seams are not blended.
"""
from __future__ import annotations

import struct

import torch

from . import entropy
from . import lib as _lib
from .entropy import EntropyError
from .ops import _p, _stream

MAGIC = b"DSICI\x00"
VERSION = 1
KIND_U8_HWC, KIND_F32_CHW = 0, 1
_HEAD = struct.Struct("<6sHI6I4I2I")
_LEN = struct.Struct("<Q")


def _ceil16(n):
    return (n + 15) // 16 * 16


def _grid(H, W, th, tw):
    Hp, Wp = _ceil16(H), _ceil16(W)
    ny, nx = -(-Hp // th), -(-Wp // tw)
    return {"H": H, "W": W, "Hp": Hp, "Wp": Wp, "th": th, "tw": tw, "ny": ny, "nx": nx, "n": ny * nx,
            "ys": [min(i * th, Hp - th) for i in range(ny)], "xs": [min(j * tw, Wp - tw) for j in range(nx)],
            "own_y": [(i * th, min((i + 1) * th, Hp)) for i in range(ny)],
            "own_x": [(j * tw, min((j + 1) * tw, Wp)) for j in range(nx)]}


def _check_image(H, W):
    if H < 1 or W < 1:
        raise ValueError(f"empty image {H}x{W}")
    Hp, Wp = _ceil16(H), _ceil16(W)
    if Hp < 32 or Wp < 32:
        raise ValueError(f"image {H}x{W}: padded to {Hp}x{Wp}, under the 32x32 the model path is tested at")
    if Hp - H >= H or Wp - W >= W:
        raise ValueError(f"image {H}x{W}: the reflect padding to {Hp}x{Wp} must be smaller than the image")


def tile_grid(H, W, tile=256) -> dict:
    """Tile geometry of an H x W image (pure Python).  Hp = ceil16(H), th = min(tile, Hp); tile row origins 0, th, 2th,
    ... with the last clamped to Hp - th; tile row i owns padded rows [i*th, min((i+1)*th, Hp)) (overlap rows belong
    to the earlier tile).  Columns likewise; tiles are numbered row-major.  Returns H, W, Hp, Wp, th, tw, ny, nx, n,
    ys, xs (origins) and own_y, own_x (owned ranges)."""
    tile = int(tile)
    if tile % 16 or tile < 32:
        raise ValueError(f"tile={tile} must be a multiple of 16 and at least 32")
    _check_image(H, W)
    return _grid(H, W, min(tile, _ceil16(H)), min(tile, _ceil16(W)))


def _model_shape(model):
    in_ch = model.g_a.g_a[0].in_channels
    return int(model.N), int(model.M), int(in_ch), int(bool(getattr(model, "spatial_params", False)))


def pack_image_stream(header: dict, blobs) -> bytes:
    """header (the fields unpack_image_stream returns) + the DSIC2 containers -> the stream (pure Python)."""
    h = header
    head = _HEAD.pack(MAGIC, VERSION, h["numerics"] & 0xFFFFFFFF, h["H"], h["W"], h["C"], h["kind"], h["th"], h["tw"],
                      h["N"], h["M"], h["in_ch"], h["spatial_params"], h["batch"], len(blobs))
    return b"".join([head] + [_LEN.pack(len(b)) + bytes(b) for b in blobs])


def unpack_image_stream(stream) -> dict:
    """stream -> header fields (version, numerics, H, W, C, kind, th, tw, N, M, in_ch, spatial_params, batch,
    batches) and "blobs", the list of inner DSIC2 containers (pure Python).  ValueError on a wrong magic, a truncated
    stream or trailing bytes."""
    s = bytes(stream)
    if len(s) < _HEAD.size:
        raise ValueError("truncated DSICI stream" if s[:6] == MAGIC[:len(s)] else "not a DSICI image stream")
    f = _HEAD.unpack_from(s, 0)
    if f[0] != MAGIC:
        raise ValueError("not a DSICI image stream")
    keys = ("version", "numerics", "H", "W", "C", "kind", "th", "tw", "N", "M", "in_ch", "spatial_params", "batch",
            "batches")
    h = dict(zip(keys, f[1:]))
    if h["version"] != VERSION:
        raise ValueError(f"DSICI stream version {h['version']}, this reader knows {VERSION}")
    off, blobs = _HEAD.size, []
    for _ in range(h["batches"]):
        if off + _LEN.size > len(s):
            raise ValueError("truncated DSICI stream")
        (n,) = _LEN.unpack_from(s, off)
        off += _LEN.size
        if off + n > len(s):
            raise ValueError("truncated DSICI stream")
        blobs.append(s[off:off + n])
        off += n
    if off != len(s):
        raise ValueError(f"DSICI stream: {len(s) - off} trailing bytes")
    h["blobs"] = blobs
    return h


def image_bpp(stream) -> float:
    """8 * stream bytes / (H * W): the whole stream, headers included."""
    h = _HEAD.unpack_from(bytes(stream[:_HEAD.size]), 0)
    return 8.0 * len(stream) / (h[3] * h[4])


def _gather(img, kind, g, C, first, n):
    L = _lib.load()
    if kind == KIND_U8_HWC:
        tiles = torch.empty((n, g["th"], g["tw"], C), dtype=torch.uint8, device=img.device)
        fn, what = L.dsic_tile_gather_u8, "tile_gather_u8"
    else:
        tiles = torch.empty((n, C, g["th"], g["tw"]), dtype=torch.float32, device=img.device)
        fn, what = L.dsic_tile_gather_f32, "tile_gather_f32"
    _lib.check(fn(_p(img), _p(tiles), g["H"], g["W"], C, g["th"], g["tw"], first, n, _stream()), what)
    return tiles


@torch.no_grad()
def compress_image(model, img, tile=256, batch=64, tail=10) -> bytes:
    """img: uint8 [H,W,C] or float32 [C,H,W] in [0,1], on the CPU or the GPU -> one DSICI stream.  The image is
    uploaded once; each batch of `batch` tiles is gathered on the device (reflect padding included) and becomes one
    DSIC2 container."""
    dev = next(model.parameters()).device
    if img.dim() != 3:
        raise ValueError(f"compress_image: expected uint8 [H,W,C] or float32 [C,H,W], got {tuple(img.shape)}")
    if img.dtype == torch.uint8:
        kind, (H, W, C) = KIND_U8_HWC, img.shape
    elif img.dtype == torch.float32:
        kind, (C, H, W) = KIND_F32_CHW, img.shape
    else:
        raise TypeError(f"compress_image: expected uint8 or float32, got {img.dtype}")
    N, M, in_ch, spatial = _model_shape(model)
    if C != in_ch:
        raise ValueError(f"compress_image: image has {C} channels, the model takes {in_ch}")
    batch = int(batch)
    if batch < 1:
        raise ValueError(f"compress_image: batch={batch}")
    g = tile_grid(H, W, tile)
    x = img.to(dev).contiguous()
    blobs = []
    for first in range(0, g["n"], batch):
        tiles = _gather(x, kind, g, C, first, min(batch, g["n"] - first))
        blobs.append(entropy.compress_to_container(model, tiles, tail))
    header = {"numerics": entropy.numerics_tag(), "H": H, "W": W, "C": C, "kind": kind, "th": g["th"], "tw": g["tw"],
              "N": N, "M": M, "in_ch": in_ch, "spatial_params": spatial, "batch": batch}
    return pack_image_stream(header, blobs)


@torch.no_grad()
def decompress_image(model, stream, out=None):
    """DSICI stream -> the image on the model's device: uint8 [H,W,C] ((uint8)(clamp(x,0,1)*255), truncating, as
    torchvision's to_pil_image) or float32 [C,H,W] (clamp(x,0,1)); by default the kind of the encoder's input,
    out="u8" / "f32" overrides it.  Each decoded batch is stitched straight into the image."""
    h = unpack_image_stream(stream)
    if out not in (None, "u8", "f32"):
        raise ValueError(f"decompress_image: out={out!r} (None, 'u8' or 'f32')")
    if int(h["numerics"]) != entropy.numerics_tag():
        raise EntropyError(f"decompress_image: the stream was written with numerics tag {h['numerics']:#x}, this "
                           f"decoder is {entropy.numerics_tag():#x}")
    mine = _model_shape(model)
    theirs = (h["N"], h["M"], h["in_ch"], h["spatial_params"])
    if mine != theirs:
        raise EntropyError(f"decompress_image: the stream was written by a model with (N, M, in_ch, spatial_params) = "
                           f"{theirs}, this one is {mine}")
    H, W, C, th, tw = h["H"], h["W"], h["C"], h["th"], h["tw"]
    if C != h["in_ch"] or h["kind"] not in (KIND_U8_HWC, KIND_F32_CHW) or h["batch"] < 1:
        raise ValueError("DSICI stream: inconsistent header")
    _check_image(H, W)
    if th % 16 or tw % 16 or th < 32 or tw < 32 or th > _ceil16(H) or tw > _ceil16(W):
        raise ValueError(f"DSICI stream: tile {th}x{tw} does not fit a {H}x{W} image")
    g = _grid(H, W, th, tw)
    if h["batches"] != -(-g["n"] // h["batch"]):
        raise ValueError(f"DSICI stream: {h['batches']} batches for {g['n']} tiles in batches of {h['batch']}")
    kind = {None: h["kind"], "u8": KIND_U8_HWC, "f32": KIND_F32_CHW}[out]
    dev = next(model.parameters()).device
    L = _lib.load()
    if kind == KIND_U8_HWC:
        if C not in (3, 4):
            raise ValueError(f"decompress_image: uint8 output needs 3 or 4 channels, the stream has {C}")
        img = torch.empty((H, W, C), dtype=torch.uint8, device=dev)
        fn, what = L.dsic_tile_stitch_u8, "tile_stitch_u8"
    else:
        img = torch.empty((C, H, W), dtype=torch.float32, device=dev)
        fn, what = L.dsic_tile_stitch_f32, "tile_stitch_f32"
    for k, blob in enumerate(h["blobs"]):
        first = k * h["batch"]
        n = min(h["batch"], g["n"] - first)
        _, shape_y, _, _ = entropy._container_records(blob)
        if shape_y[0] != n or shape_y[2:] != [th // 16, tw // 16]:
            raise ValueError(f"DSICI stream: batch {k} holds {shape_y[0]} latents of {shape_y[2]}x{shape_y[3]}, "
                             f"expected {n} of {th // 16}x{tw // 16}")
        tiles = entropy._decompress_container_raw(model, blob, what="decompress_image").contiguous()
        _lib.check(fn(_p(tiles), _p(img), H, W, C, th, tw, first, n, _stream()), what)
    return img
