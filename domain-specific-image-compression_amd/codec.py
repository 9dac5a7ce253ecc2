"""Whole-image codec: an image of any size -> one byte stream -> the image, at its own size.

The reference's driver (code/modelv2/eval_selfcontained_entropy.py:126-159) codes one PNG in one forward pass and
needs no size bookkeeping because its images are multiples of 16.  Here an image is cut into tiles of the size the
codec is tuned for (256 x 256, batches of 64), each batch becomes one DSIC2 container (entropy.compress_to_container),
and the containers travel in one DSICI stream with the image's geometry:

    magic "DSICI\\0" | version u16 | numerics tag u32 | H, W, C, kind, th, tw u32 | N, M, in_ch, spatial_params u32 |
    batch, batches u32 | the version's fields, u32 words | [u64 length, mask block] |
    per batch: u64 length, container [, u64 length, residual block]          (little endian, fixed-size fields)

What follows the 60 fixed bytes is stated once, in the table FORMATS below: per version the kinds it goes with, its
fields in order with their constraints, and whether a mask block precedes the containers or a residual block follows
each.  In one line each:

    1  the plain stream                          5  nodata: a mask block, only the tiles that are not empty are coded
    2  segments = K > 1: DSIC3 containers        6  a uint16 image (kind 2) with its per-band scale
    3  overlap = O > 0: blended seams            8  a validity mask with its fill (kind 0 or 2); 7 is unassigned
    4  max_error: a residual block per batch     9  tolerance: a uint16 image with a wide residual block per batch

kind 0 = uint8 [H,W,C] (PIL / numpy layout), 1 = float32 [C,H,W] in [0,1], 2 = uint16 [H,W,C].  Tiling (tile_grid): the
image is reflect-padded bottom/right to multiples of 16 inside the gather kernel; the last row / column of tiles shifts
inward (overlap, no extra padding) and every pixel is written back by the one tile that owns it.  Tiles are coded
independently, as the reference's patch-trained model sees them; at the default overlap = 0 seams are not blended.

segments = K > 1 (entropy.compress_latents): every tile's y string is K independent strings, so that a decoder reads a
tile on K waves; version 1 is written whenever K = 1 and nothing else asks for more.

overlap = O > 0 (a multiple of 16, at most half a tile side): neighbouring tiles share O pixels (tile_grid: stride
t - O) and their reconstructions are cross-faded over them with linear ramps that sum to 1; the blend is a fixed float32
fold over a pixel's contributing tiles in ascending tile number (dsic_tile_blend_window_f32), so a window decodes to the
same bits however its tiles are batched.

max_error = tau (an integer 0 .. 127; uint8 images, overlap = 0), the near-lossless mode: behind every container (the
bytes the same call without max_error writes) goes a residual block (residual.py): per tile the quantized difference
between the tile and the lossy uint8 reconstruction, coded with tables built from the tile's own histogram.  The
decoders add it back in the stitch, and every decoded pixel lies within tau of the original; tau = 0 is lossless.
Tiles stay independent, so a region still decodes from its own tiles' bytes alone.

nodata = v (an integer 0 .. 255; uint8 images, overlap = 0, no max_error, no overviews): a pixel is nodata iff all its
channels equal v.  Per tile, over the pixels it owns inside H x W, the mask block (mask.py) holds a state: 0 empty (all
nodata), 1 full (none), 2 mixed.  The coded tiles are those of state 1 and 2 in ascending tile number, container k
holds coded tiles k batch ... (0 containers are allowed); their strings are byte for byte those of the stream without
nodata.  A mixed tile's mask travels in the block as the vertical delta of its bit plane, raw or as a list of
positions.  The decoders skip empty tiles altogether and write v at every nodata pixel after the stitch
(dsic_mask_apply_u8 / _f32, which write only pixels a tile owns, so stray set bits outside a tile's owned rectangle are
harmless).

Because tiles are independent and the DSIC2 heads hold every string's length, any window of a stream can be decoded
from only the tiles that own its pixels: stream_index finds their bytes from the heads alone, decompress_region decodes
them in dense batches and stitches them into the window, byte for byte the crop of decompress_image's result.
decompress_image is the same decode (_decode_window) of the window (0, 0, H, W), one batch per container.

A uint16 [H,W,C] image (kind 2: 16-bit imagery such as Sentinel-2 reflectances, C at most 4) carries a per-band scale
(lo, hi): by default the band's own minimum and maximum (dsic_band_range_u16), or the caller's.  With R = hi - lo the
model sees norm(v) = R == 0 ? 0 : float32(min(max(v, lo), hi) - lo) / float32(R), the arithmetic of the reference's
code/combinebandsall.py:7-12, computed in the tile gather (dsic_tile_gather_u16), so every container is byte for byte
that of the float32 image norm(img); the decoders return denorm(x) = lo + uint32(clamp(x, 0, 1) * float32(R) + 0.5f),
rounded to nearest (stitch and blend finish), and denorm(norm(v)) == v inside [lo, hi].  max_error and nodata are
refused with uint16 images: the residual tables and the mask classifier are 8-bit; max_error stays the uint8 mode, and
a uint16 image takes tolerance instead.

tolerance = tau (an integer 0 .. 32767; uint16 images, overlap = 0), the bounded-error mode of 16-bit imagery: behind
every container (the bytes of the version-6 stream of the same call without tolerance) goes a wide residual block
(residual16.py): per tile the quantized difference between the image and the lossy uint16 reconstruction, split into a
high part of at most 511 values, coded as the version-4 residual is, and k raw bit planes.  Every decoded value lies
within tau of the original and tau = 0 returns it, also outside the scale; the decoders return uint16.  k follows each
tile's largest step, so one outlier in a quiet tile costs k raw bits on every sample of the tile (escape coding is not
done).

overviews = n > 0 writes a pyramid, the image at full, 1/2, 1/4, ... 1/2^n resolution in one DSICP stream:

    magic "DSICP\\0" | version u16 = 1 | levels u32 (n + 1 >= 2) | levels x (H u32, W u32, offset u64, length u64) |
    the level streams back to back, level 0 first                 (little endian; offsets count from the magic)

Level l + 1 is level l halved on the device (build_overviews: ceil(H/2) x ceil(W/2), the mean of each 2 x 2 block with
the last row or column of an odd side counted twice; uint8 and uint16 (a + b + c + d + 2) >> 2, float32 ((a + b) +
(c + d)) * 0.25f), and every level's bytes are the DSICI stream compress_image writes for that level's image, so a level is
read, indexed and decoded on its own (level=l of the decoders and of stream_index) through a view of its byte range.

valid = mask (a torch.bool [H,W] plane beside a uint8 or uint16 image, True = the pixel holds data) with fill = f is the
general form of the nodata mask: nothing is guessed from pixel values.  The mask block is mask.py's, a set bit meaning
owned, inside the image and invalid, its nodata field carrying fill; states, coded tiles and containers are as with
nodata, and the coded tiles' strings are those of the stream without the mask (version 1 / 2, or version 6 with the
same scale).  The decoders write fill at every invalid pixel and can return the mask (with_valid, decompress_valid).
With overviews the levels come from the masked halving (build_overviews with valid): of the four taps k are valid with
the sum S, the output is valid iff k > 0 and is (2 S + k) // (2 k), and for k = 0 the unmasked mean; every level is the
version-8 stream of its own image and mask, with level 0's fill and scale.

ImageReader (view.py) keeps a stream open for pan and zoom: levels opened once, decoded tiles cached on the device and
assembled by the calls decompress_region makes (_assemble_window), requests decoded together (read_many), and windows
resampled to a size asked for from the level view_level picks (csrc/view.hip); read_warped samples an affine view
(csrc/warp.hip) and read_gridded a reprojected one, its sample positions interpolated from a coordinate mesh
(csrc/grid.hip; affine_grid, projective_grid, function_grid, grid_level and grid_window are its planning).  SceneStack (view.py) places several
readers on one grid and composites their windows per pixel in one launch (csrc/composite.hip): first, last, mean,
median, or the whole pixel of the scene whose index is largest or smallest (stack_reduce names the forms).
SceneStack.read_warped samples every scene under its own affine and combines them in the same launch
(csrc/warp_composite.hip; compose_q16 and stack_warp_parts are its planning).
ImageReader.zonal_stats and SceneStack.zonal_stats measure instead of showing: per zone of a uint16 zone raster the count,
sum, sum of squares, minimum and maximum of every band or of an index, in integers, reduced on the device strip by strip
(csrc/zonal.hip); zonal_table makes means and deviations of the table, zonal_percentile medians of the optional bins.
"""
from __future__ import annotations

import bisect
import collections
import ctypes
import operator
import struct

import numpy as np
import torch

from . import entropy
from . import lib as _lib
from . import mask as _mask
from . import residual as _residual
from . import residual16 as _residual16
from .entropy import EntropyError
from .ops import _int_option, _p, _stream

MAGIC = b"DSICI\x00"
VERSION = 1
VERSION_SEG = 2            # segments > 1
VERSION_OV = 3             # overlap > 0
VERSION_RES = 4            # max_error: a residual block per batch
VERSION_MASK = 5           # nodata: a mask block, then the coded tiles' batches
VERSION_U16 = 6            # a uint16 image with its per-band scale
VERSION_VALID = 8          # a validity mask with its fill; 7 is unassigned
VERSION_TOL = 9            # tolerance: a uint16 image with a wide residual block per batch
BLEND_IDS = 64             # tiles per dsic_tile_blend_window_f32 call
KIND_U8_HWC, KIND_F32_CHW, KIND_U16_HWC = 0, 1, 2
_OUT_KINDS = {"u8": KIND_U8_HWC, "f32": KIND_F32_CHW, "u16": KIND_U16_HWC}
_HEAD = struct.Struct("<6sHI6I4I2I")
_HEAD_KEYS = ("version", "numerics", "H", "W", "C", "kind", "th", "tw", "N", "M", "in_ch", "spatial_params", "batch",
              "batches")
_LEN = struct.Struct("<Q")
PMAGIC = b"DSICP\x00"
PVERSION = 1
_PHEAD = struct.Struct("<6sHI")                                            # magic, version, levels
_PLEVEL = struct.Struct("<IIQQ")                                           # H, W, offset, length
_SAME_IN_LEVELS = ("C", "kind", "N", "M", "in_ch", "spatial_params", "numerics", "scale", "fill")


def _ceil16(n):
    return (n + 15) // 16 * 16


def _axis(Lp, t, O):
    """One axis of the grid: (stride, origins, nominal ranges, supports)."""
    if Lp <= t:
        return t, [0], [(0, Lp)], [(0, Lp)]
    s = t - O
    n = -(-(Lp - O) // s)
    return (s, [min(i * s, Lp - t) for i in range(n)], [(i * s, min((i + 1) * s, Lp)) if i < n - 1 else (i * s, Lp)
                                                        for i in range(n)],
            [(i * s, (i + 1) * s + O) if i < n - 1 else (i * s, Lp) for i in range(n)])


def _grid(H, W, th, tw, O=0):
    Hp, Wp = _ceil16(H), _ceil16(W)
    sy, ys, own_y, sup_y = _axis(Hp, th, O)
    sx, xs, own_x, sup_x = _axis(Wp, tw, O)
    ny, nx = len(ys), len(xs)
    return {"H": H, "W": W, "Hp": Hp, "Wp": Wp, "th": th, "tw": tw, "ny": ny, "nx": nx, "n": ny * nx,
            "ys": ys, "xs": xs, "own_y": own_y, "own_x": own_x,
            "overlap": O, "sy": sy, "sx": sx, "sup_y": sup_y, "sup_x": sup_x}


def _check_overlap(O, th, tw, what):
    """overlap as a stream and the kernels take it: 0, or a multiple of 16 of at most half the smaller tile side."""
    try:
        O = operator.index(O)
    except TypeError:
        raise ValueError(f"{what}: overlap={O!r} is not an integer") from None
    if O < 0 or O % 16 or 2 * O > min(th, tw):
        raise ValueError(f"{what}: overlap={O!r} must be 0 or a multiple of 16 from 16 to half the smaller side of "
                         f"the {th}x{tw} tiles")
    return O


def check_scale(scale, C, what) -> list:
    """scale as a stream holds it: C pairs of integers (lo, hi), 0 <= lo <= hi <= 65535 -> [(lo, hi), ...]."""
    try:
        pairs = [tuple(operator.index(v) for v in pair) for pair in scale]
    except TypeError:
        raise ValueError(f"{what}: scale={scale!r} is not a sequence of integer pairs (lo, hi)") from None
    if len(pairs) != C or any(len(pair) != 2 for pair in pairs):
        raise ValueError(f"{what}: scale={scale!r} must hold one pair (lo, hi) for each of the {C} bands")
    for lo, hi in pairs:
        if not 0 <= lo <= hi <= 65535:
            raise ValueError(f"{what}: scale pair ({lo}, {hi}) must have 0 <= lo <= hi <= 65535")
    return pairs


def _lohi(scale):
    """The scale as the uint16 kernels take it: a host array of 2 C uint32 (lo0, hi0, lo1, hi1, ...)."""
    flat = [v for pair in scale for v in pair]
    return (ctypes.c_uint32 * len(flat))(*flat)


def _check_image(H, W):
    if H < 1 or W < 1:
        raise ValueError(f"empty image {H}x{W}")
    Hp, Wp = _ceil16(H), _ceil16(W)
    if Hp < 32 or Wp < 32:
        raise ValueError(f"image {H}x{W}: padded to {Hp}x{Wp}, under the 32x32 the model path is tested at")
    if Hp - H >= H or Wp - W >= W:
        raise ValueError(f"image {H}x{W}: the reflect padding to {Hp}x{Wp} must be smaller than the image")


def tile_grid(H, W, tile=256, overlap=0) -> dict:
    """Tile geometry of an H x W image (pure Python).  Hp = ceil16(H), th = min(tile, Hp); tile row origins 0, th, 2th,
    ... with the last clamped to Hp - th; tile row i owns padded rows [i*th, min((i+1)*th, Hp)) (overlap rows belong
    to the earlier tile).  Columns likewise; tiles are numbered row-major.  Returns H, W, Hp, Wp, th, tw, ny, nx, n,
    ys, xs (origins) and own_y, own_x (owned ranges).

    overlap = O (0, or a multiple of 16 with 16 <= O <= tile / 2): an axis of more than one tile has the stride
    s = t - O, ceil((Lp - O) / s) tiles, nominal origins a(i) = i*s and real origins min(i*s, Lp - t) (only the last
    shifts inward).  own_y / own_x are the nominal ranges [a(i), a(i+1)) (the last ends at Lp); sup_y / sup_x the
    supports [a(i), a(i+1) + O) (the last ends at Lp), outside which the tile's blend weight is 0: it ramps up as
    (2k+1)/(2O) over the first O positions of the support (i > 0), down as (2(O-1-k)+1)/(2O) over its last O
    (i < n-1) and is 1 between, so the weights at a position sum to 1 and at most two tiles per axis contribute.
    Also returns overlap, sy, sx (strides; t on an axis of one tile, which has no ramp)."""
    tile = int(tile)
    if tile % 16 or tile < 32:
        raise ValueError(f"tile={tile} must be a multiple of 16 and at least 32")
    overlap = _check_overlap(overlap, tile, tile, "tile_grid")
    _check_image(H, W)
    return _grid(H, W, min(tile, _ceil16(H)), min(tile, _ceil16(W)), overlap)


def _model_shape(model):
    in_ch = model.g_a.g_a[0].in_channels
    return int(model.N), int(model.M), int(in_ch), int(bool(getattr(model, "spatial_params", False)))


# ---- the DSICI head: the fixed 60 bytes (_HEAD), then the version's fields, each a run of u32 words ----------------------
# A field, stated once.  count(e, h): its words in a stream of entry e whose fixed head is h; load(e, h, w): the reader's
# check of its words w, and what it keeps of them in h; dump(e, h, what): the words a writer emits for a header h whose
# segments, overlap and coded it has settled, checking a caller's value as compress_image does.
_Field = collections.namedtuple("_Field", "count load dump")


def _one(e, h):
    return 1


def _load_segments(e, h, w):
    h["segments"] = w[0]
    allowed = entropy.SEGMENTS[1:] if e.segments == "many" else entropy.SEGMENTS
    if w[0] not in allowed or h["M"] % w[0]:
        raise ValueError(f"DSICI stream: segments={w[0]} is not one of {allowed} dividing M={h['M']}")


def _load_overlap(e, h, w):
    if e.overlap == "zero":
        if w[0] != 0:
            raise ValueError(f"DSICI stream: version {h['version']} with overlap={w[0]} "
                             f"({'a mask' if e.mask else 'a residual layer'} over blended tiles is not supported)")
        return
    if e.overlap == "positive" and w[0] == 0:
        raise ValueError(f"DSICI stream: version {h['version']} with overlap=0")
    h["overlap"] = _check_overlap(w[0], h["th"], h["tw"], "DSICI stream")


def _ranged(key, top, note="", hint=""):
    """The field key = v with 0 <= v <= top(h); the writer's test of a caller's value is ops._int_option, whose message
    says `hint` behind the 0."""
    def load(e, h, w):
        h[key] = w[0]
        if w[0] > top(h):
            raise ValueError(f"DSICI stream: {key}={w[0]} (0 .. {top(h)}{note.format(**h)})")
    return _Field(_one, load, lambda e, h, what: [_int_option(h[key], key, top(h), what, hint)])


def _load_bands(e, h, w):
    if w[0] != e.layer.BANDS:
        raise ValueError(f"DSICI stream: version {h['version']} with res_bands={w[0]}, this reader knows {e.layer.BANDS}")


def _load_scale(e, h, w):
    if w:
        h["scale"] = list(zip(w[0::2], w[1::2]))
    for lo, hi in zip(w[0::2], w[1::2]):
        if lo > hi or hi > 65535:
            raise ValueError(f"DSICI stream: scale pair ({lo}, {hi}) must have lo <= hi <= 65535")


def _dump_scale(e, h, what):
    return [v for pair in check_scale(h["scale"], h["C"], what) for v in pair] if h["kind"] == KIND_U16_HWC else []


_FIELDS = {
    "segments": _Field(_one, _load_segments, lambda e, h, what: [h["segments"]]),
    "overlap": _Field(_one, _load_overlap, lambda e, h, what: [h["overlap"]]),
    "max_error": _ranged("max_error", lambda h: 127, hint=" (lossless)"),
    "res_bands": _Field(_one, _load_bands, lambda e, h, what: [e.layer.BANDS]),
    "nodata": _ranged("nodata", lambda h: 255),
    "coded": _Field(_one, lambda e, h, w: h.update(coded=w[0]), lambda e, h, what: [h["coded"]]),
    "fill": _ranged("fill", lambda h: 65535 if h["kind"] == KIND_U16_HWC else 255, " for kind {kind}"),
    # C pairs (lo, hi) of a uint16 image; a version that also takes kind 0 (8) has none there
    "scale": _Field(lambda e, h: 2 * h["C"] if h["kind"] == KIND_U16_HWC else 0, _load_scale, _dump_scale),
    "tolerance": _ranged("tolerance", lambda h: _residual16.MAX_TOLERANCE, hint=" (lossless)"),
}

# A version, stated once.  kinds: the image kinds it goes with; fields: what follows the fixed head, in order; segments:
# "many" (K > 1) or "any"; overlap: "positive", "free" (0 allowed) or "zero"; key: the header key that makes a writer
# choose the version, name: what messages call it; mask: a mask block (mask.py) precedes the containers, its fill value
# being h[key]; layer: the module (residual or residual16) of the residual block that follows every container, its
# bound being h[key].
_Version = collections.namedtuple("_Version", "kinds fields segments overlap key name mask layer",
                                  defaults=((), None, None, None, None, False, None))
_U8_F32, _U16 = (KIND_U8_HWC, KIND_F32_CHW), (KIND_U16_HWC,)
FORMATS = {
    VERSION: _Version(_U8_F32),
    VERSION_SEG: _Version(_U8_F32, ("segments",), "many"),
    VERSION_OV: _Version(_U8_F32, ("segments", "overlap"), "any", "positive"),
    VERSION_RES: _Version(_U8_F32, ("segments", "overlap", "max_error", "res_bands"), "any", "zero", "max_error",
                          "max_error", layer=_residual),
    VERSION_MASK: _Version(_U8_F32, ("segments", "overlap", "nodata", "coded"), "any", "zero", "nodata", "nodata",
                           mask=True),
    VERSION_U16: _Version(_U16, ("segments", "overlap", "scale"), "any", "free", "scale", "a uint16 image"),
    VERSION_VALID: _Version((KIND_U8_HWC, KIND_U16_HWC), ("segments", "overlap", "fill", "coded", "scale"), "any", "zero",
                            "fill", "a validity mask", mask=True),
    VERSION_TOL: _Version(_U16, ("segments", "overlap", "scale", "tolerance", "res_bands"), "any", "zero", "tolerance",
                          "tolerance", layer=_residual16),
}


def _format_of(h) -> _Version:
    """The table entry of a header that a reader has accepted."""
    return FORMATS[h["version"]]


def _listed(names, last) -> str:
    """["a", "b", "c"], "or" -> "a, b or c"."""
    names = [str(n) for n in names]
    return f"{', '.join(names[:-1])} {last} {names[-1]}" if len(names) > 1 else names[0]


def _version_for(h) -> int:
    """The version a header is written as: the highest whose key it holds (tolerance, fill, scale, nodata, max_error),
    else 3 for overlap > 0, 2 for segments > 1, else 1."""
    return next((v for v in sorted(FORMATS, reverse=True) if h.get(FORMATS[v].key) is not None),
                VERSION_OV if h.get("overlap", 0) else VERSION_SEG if h.get("segments", 1) > 1 else VERSION)


def _check_kind(e, version, kind, what):
    """The kind against the version, where the head's layout hangs on it: a uint16 image has a scale, so kind 2 and the
    versions that take it are held to each other here; another kind nobody knows is left to _stream_grid."""
    if kind not in e.kinds and KIND_U16_HWC in e.kinds + (kind,):
        raise ValueError(f"{what}: version {version} with kind {kind} ({e.name or 'it'} goes with kind "
                         f"{_listed(e.kinds, 'or')}; kind {KIND_U16_HWC}, the uint16 image, and the versions "
                         "that carry a scale go together)")


def pack_image_stream(header: dict, blobs, residuals=None, mask=None) -> bytes:
    """header (the fields unpack_image_stream returns) + the DSIC2 containers -> the stream (pure Python).  The version
    is the highest one whose key (FORMATS) the header holds: tolerance, fill, scale, nodata, max_error; else 3 for
    "overlap" > 0, 2 for "segments" > 1, else 1.  ValueError for a key, an overlap > 0 or a block the version does not
    take, and for a value a field refuses.  residuals: behind every container its residual block (residual.pack_block
    for max_error, residual16.pack_block for tolerance); mask: the mask block (mask.pack_block) of a header with nodata
    or fill, whose nodata field is that value; the containers then hold the tiles that are not empty, counted from the
    block's states, `batch` to a container, and there may be none."""
    what = "pack_image_stream"
    h = dict(header)
    K = h["segments"] = entropy.check_segments(h.get("segments", 1), h["M"], what)
    O = h["overlap"] = _check_overlap(h.get("overlap", 0), h["th"], h["tw"], what)
    if (h.get("scale") is not None) != (h["kind"] == KIND_U16_HWC):
        raise ValueError("pack_image_stream: a scale goes with kind 2 (uint16 [H,W,C]), and only with it")
    version = _version_for(h)
    e = FORMATS[version]
    _check_kind(e, version, h["kind"], what)
    # what the version does not take: overlap > 0, and the keys of the versions it ranks above
    rivals = [r for r in (FORMATS[v] for v in sorted(FORMATS) if v < version) if r.key and r.key not in e.fields]
    if (O and e.overlap == "zero") or any(h.get(r.key) is not None for r in rivals):
        names = ["overlap > 0"] * (e.overlap == "zero") + [r.name for r in rivals]
        raise ValueError(f"pack_image_stream: {e.name} together with {_listed(names, 'or')} is not supported")
    if not e.mask and mask is not None:
        raise ValueError("pack_image_stream: a mask block without nodata in the header")
    if e.layer is None and residuals is not None:
        raise ValueError("pack_image_stream: residual blocks without max_error in the header")
    if e.layer is not None and (residuals is None or len(residuals) != len(blobs)):
        raise ValueError(f"pack_image_stream: {e.key} needs one {e.layer.FORMAT.name} block per container")
    parts = []
    if e.mask:
        if mask is None:
            raise ValueError(f"pack_image_stream: {e.key} needs the mask block")
        mask = bytes(mask)
        (v,) = _FIELDS[e.key].dump(e, h, what)
        n = _grid(h["H"], h["W"], h["th"], h["tw"])["n"]
        states, _ = _mask.read_block_head(lambda o, c: mask[o:o + c], 0, len(mask), n, h["th"], h["tw"], v, what)
        coded = sum(1 for s in states if s != _mask.EMPTY)
        if e.key == "fill" and h.get("coded", coded) != coded:         # a nodata header's count was never read
            raise ValueError(f"pack_image_stream: the header says {h['coded']} coded tiles, the mask block's states "
                             f"{coded}")
        if len(blobs) != -(-coded // h["batch"]):
            raise ValueError(f"pack_image_stream: {len(blobs)} containers for {coded} coded tiles in batches of "
                             f"{h['batch']}")
        h["coded"] = coded
        parts = [_LEN.pack(len(mask)), mask]
    words = [w for name in e.fields for w in _FIELDS[name].dump(e, h, what)]
    head = _HEAD.pack(MAGIC, version, h["numerics"] & 0xFFFFFFFF, *(h[k] for k in _HEAD_KEYS[2:-1]), len(blobs))
    for i, b in enumerate(blobs):
        parts += [_LEN.pack(len(b)), bytes(b)]
        if e.layer is not None:
            parts += [_LEN.pack(len(residuals[i])), bytes(residuals[i])]
    return b"".join([head, struct.pack(f"<{len(words)}I", *words)] + parts)


class _Source:
    """Random access to a stream held as bytes or behind a binary file object (seek + read); counts what it reads."""

    def __init__(self, src):
        if isinstance(src, (bytes, bytearray, memoryview)):
            self.buf, self.f = memoryview(src).cast("B"), None
            self.size = len(self.buf)
        elif hasattr(src, "seek") and hasattr(src, "read"):
            self.buf, self.f = None, src
            self.size = src.seek(0, 2)
            if self.size is None:                                          # a seek that returns nothing: ask tell
                self.size = src.tell()
        else:
            raise TypeError(f"expected bytes or a binary file object with seek and read, got {type(src).__name__}")
        self.bytes_read = 0

    def read_at(self, off, n):
        """Up to n bytes at off (fewer only at the end of the stream)."""
        n = max(0, min(n, self.size - off))
        if self.f is None:
            out = self.buf[off:off + n]                                    # a view: copied once, into the upload
        else:
            self.f.seek(off)
            out = self.f.read(n)
            if len(out) != n:
                raise ValueError("truncated DSICI stream")
        self.bytes_read += len(out)
        return out


def _read_frame(src, off):
    """`u64 length, bytes` at off -> (where the bytes begin, the length)."""
    if off + _LEN.size > src.size:
        raise ValueError("truncated DSICI stream")
    (size,) = _LEN.unpack(src.read_at(off, _LEN.size))
    if off + _LEN.size + size > src.size:
        raise ValueError("truncated DSICI stream")
    return off + _LEN.size, size


def _read_framing(src, head=None):
    """The DSICI head and the length words of a _Source -> (header fields, (offset, bytes) of every batch's container,
    the same of every batch's residual block: empty unless the version has a residual layer); what lies inside them is
    not read.  head: the first _HEAD.size bytes, where the caller has read them already."""
    if head is None:
        head = src.read_at(0, _HEAD.size)
    if len(head) < _HEAD.size:
        raise ValueError("truncated DSICI stream" if head[:6] == MAGIC[:len(head)] else "not a DSICI image stream")
    f = _HEAD.unpack(head)
    if f[0] != MAGIC:
        raise ValueError("not a DSICI image stream")
    h = dict(zip(_HEAD_KEYS, f[1:]))
    if h["version"] not in FORMATS:
        raise ValueError(f"DSICI stream version {h['version']}, this reader knows {_listed(sorted(FORMATS), 'and')}")
    e = _format_of(h)
    _check_kind(e, h["version"], h["kind"], "DSICI stream")
    if h["kind"] == KIND_U16_HWC and not 1 <= h["C"] <= 4:
        raise ValueError(f"DSICI stream: a uint16 image of {h['C']} bands (1 .. 4)")
    off, h["segments"], h["overlap"] = _HEAD.size, 1, 0
    counts = [_FIELDS[name].count(e, h) for name in e.fields]
    if counts:
        words = src.read_at(off, 4 * sum(counts))
        if len(words) < 4 * sum(counts):
            raise ValueError("truncated DSICI stream")
        words = struct.unpack(f"<{sum(counts)}I", words)
        off += 4 * len(words)
        for name, n in zip(e.fields, counts):
            _FIELDS[name].load(e, h, words[:n])
            words = words[n:]
    if e.mask:
        h["mask_offset"], h["mask_bytes"] = _read_frame(src, off)
        off = h["mask_offset"] + h["mask_bytes"]
    frames, rframes = [], []
    for _ in range(h["batches"]):
        for into in (frames, rframes) if e.layer is not None else (frames,):
            into.append(_read_frame(src, off))
            off = sum(into[-1])
    if off != src.size:
        raise ValueError(f"DSICI stream: {src.size - off} trailing bytes")
    return h, frames, rframes


def unpack_image_stream(stream) -> dict:
    """stream -> header fields (version, numerics, H, W, C, kind, th, tw, N, M, in_ch, spatial_params, batch,
    batches, segments: 1 for a version-1 stream, overlap: 0 for versions 1 and 2) and "blobs", the list of inner DSIC2 containers (pure Python).  ValueError on a wrong magic, a truncated
    stream or trailing bytes.  A version-4 stream also gives "max_error" and "residuals", the list of its residual
    blocks; the dicts of versions 1 to 3 have neither key.  A version-5 stream gives "nodata", "coded" (the tiles that
    are not empty: the containers hold these, in ascending tile number), "mask_offset", "mask_bytes" and "mask", its
    mask block (mask.py); no other version has these keys.  A version-6 stream (kind 2, the uint16 image) gives
    "scale", the list of its C pairs (lo, hi); no other version has that key.  A version-8 stream (a validity mask;
    kind 0 or 2) gives "fill", "coded", "mask_offset", "mask_bytes", "mask" and, for kind 2, "scale"; it has no "nodata"
    key.  ValueError also for a version-8 head with kind 1, overlap != 0, a fill beyond the kind's range or a bad
    scale pair.  A version-9 stream (kind 2 with a tolerance) gives "scale", "tolerance" and "residuals", the list of
    its wide residual blocks (residual16.py); ValueError for a version-9 head with another kind, overlap != 0, a
    tolerance over 32767 or res_bands other than 16."""
    s = bytes(stream)
    h, frames, rframes = _read_framing(_Source(s))
    h["blobs"] = [s[off:off + size] for off, size in frames]
    if _format_of(h).layer is not None:
        h["residuals"] = [s[off:off + size] for off, size in rframes]
    if _format_of(h).mask:
        h["mask"] = s[h["mask_offset"]:h["mask_offset"] + h["mask_bytes"]]
    return h


def image_bpp(stream) -> float:
    """8 * stream bytes / (H * W): the whole stream, headers included.  A DSICP stream: all its levels over the pixels
    of level 0."""
    if bytes(stream[:6]) == PMAGIC:
        H, W, _, _ = _PLEVEL.unpack_from(bytes(stream[_PHEAD.size:_PHEAD.size + _PLEVEL.size]), 0)
        return 8.0 * len(stream) / (H * W)
    h = _HEAD.unpack_from(bytes(stream[:_HEAD.size]), 0)
    return 8.0 * len(stream) / (h[3] * h[4])


# ---- overviews: the image at 1/2, 1/4, ... resolution beside it, each level a stream of its own ------------------
def _halved(n):
    return (n + 1) // 2


def overview_shapes(H, W, n) -> list:
    """[(H, W), (ceil(H/2), ceil(W/2)), ...]: the sizes of an H x W image and its n overview levels, each the one
    before it halved and rounded up (pure Python).  ValueError if n is not an integer >= 0, or if a level is not an
    image the codec takes (its padded side under 32, or its reflect padding not smaller than the level); the message
    names the first such level."""
    try:
        n = operator.index(n)
    except TypeError:
        raise ValueError(f"overviews={n!r} is not an integer") from None
    if n < 0:
        raise ValueError(f"overviews={n} must be at least 0")
    shapes = [(int(H), int(W))]
    for _ in range(n):
        shapes.append((_halved(shapes[-1][0]), _halved(shapes[-1][1])))
    for level, (h, w) in enumerate(shapes):
        try:
            _check_image(h, w)
        except ValueError as e:
            raise ValueError(f"overview level {level} of a {H}x{W} image: {e}") from None
    return shapes


def level_window(level, y0, x0, h, w) -> tuple:
    """The smallest window (y0', x0', h', w') of overview level `level` that covers the level-0 window rows
    [y0, y0+h) x columns [x0, x0+w) (pure Python): a pixel of level l covers the 2^l x 2^l block of level 0 at
    (y << l, x << l), so y0' = y0 >> l and h' = ceil((y0 + h) / 2^l) - y0'; columns likewise."""
    level, y0, x0, h, w = (operator.index(v) for v in (level, y0, x0, h, w))
    if level < 0 or y0 < 0 or x0 < 0 or h < 1 or w < 1:
        raise ValueError(f"level_window: level {level}, window {h}x{w} at ({y0}, {x0})")
    s = (1 << level) - 1
    return y0 >> level, x0 >> level, ((y0 + h + s) >> level) - (y0 >> level), ((x0 + w + s) >> level) - (x0 >> level)


def level_for(index, max_side) -> int:
    """The coarsest level of a stream_index dict whose longer side is still >= max_side, or 0 if none is (always 0 for
    a DSICI stream): the level to decode for a view of max_side pixels without magnifying (pure Python)."""
    levels = index.get("levels") or [{"H": index["H"], "W": index["W"]}]
    fit = [l for l, lv in enumerate(levels) if max(lv["H"], lv["W"]) >= max_side]
    return max(fit) if fit else 0


def _image_kind(img, what):
    """(kind, H, W, C) of a uint8 [H,W,C], uint16 [H,W,C] or float32 [C,H,W] tensor."""
    if img.dim() != 3:
        raise ValueError(f"{what}: expected uint8 or uint16 [H,W,C] or float32 [C,H,W], got {tuple(img.shape)}")
    if img.dtype in (torch.uint8, torch.uint16):
        H, W, C = img.shape
        return (KIND_U8_HWC if img.dtype == torch.uint8 else KIND_U16_HWC), H, W, C
    if img.dtype == torch.float32:
        C, H, W = img.shape
        return KIND_F32_CHW, H, W, C
    raise TypeError(f"{what}: expected uint8, uint16 or float32, got {img.dtype}")


def _check_valid(valid, H, W, what):
    """valid as compress_image takes it: a torch.bool [H,W] tensor, else ValueError."""
    if not isinstance(valid, torch.Tensor) or valid.dtype != torch.bool or tuple(valid.shape) != (H, W):
        got = f"{valid.dtype} {tuple(valid.shape)}" if isinstance(valid, torch.Tensor) else type(valid).__name__
        raise ValueError(f"{what}: valid must be a torch.bool [{H}, {W}] tensor (True = the pixel holds data), got {got}")


@torch.no_grad()
def build_overviews(img, n, valid=None):
    """[img, level 1, ..., level n] on the device: img uint8 or uint16 [H,W,C] or float32 [C,H,W] on the GPU, each
    level the one before it halved by dsic_image_halve_u8 / _u16 / _f32 (one launch per level): ceil(H/2) x ceil(W/2),
    a pixel the mean of its 2 x 2 block, the last row or column of an odd side counted twice; uint8 and uint16 round
    half up, (a + b + c + d + 2) >> 2, float32 is ((a + b) + (c + d)) * 0.25f.  The sizes are
    overview_shapes(H, W, n).
    valid: a torch.bool [H,W] mask on the GPU beside a uint8 or uint16 image (True = the pixel holds data) -> (levels,
    masks), the masked halving (dsic_image_halve_valid_u8 / _u16, one launch per level): of the same four taps k are
    valid, with the sum S per channel; the output pixel is valid iff k > 0 and is (2 S + k) // (2 k), the mean over the
    valid taps rounded half up, and for k = 0 the unmasked mean of the four taps.  With an all-True mask every level
    is the level without a mask, bit for bit."""
    kind, H, W, C = _image_kind(img, "build_overviews")
    if not img.is_cuda:
        raise RuntimeError(f"build_overviews: expected a tensor on the GPU (no CPU fallback), got {img.device}")
    shapes = overview_shapes(H, W, n)
    L = _lib.load()
    levels = [img.contiguous()]
    if valid is not None:
        if kind == KIND_F32_CHW:
            raise ValueError("build_overviews: a validity mask goes with a uint8 or uint16 [H,W,C] image, not float32")
        _check_valid(valid, H, W, "build_overviews")
        if not valid.is_cuda:
            raise RuntimeError(f"build_overviews: expected the mask on the GPU (no CPU fallback), got {valid.device}")
        masks = [valid.to(torch.uint8).contiguous()]
        suffix, dtype = ("u8", torch.uint8) if kind == KIND_U8_HWC else ("u16", torch.uint16)
        for (h, w), (h2, w2) in zip(shapes, shapes[1:]):
            dst = torch.empty((h2, w2, C), dtype=dtype, device=img.device)
            dval = torch.empty((h2, w2), dtype=torch.uint8, device=img.device)
            _lib.check(getattr(L, "dsic_image_halve_valid_" + suffix)(_p(levels[-1]), _p(masks[-1]), _p(dst), _p(dval), h,
                                                                      w, C, _stream()), "image_halve_valid_" + suffix)
            levels.append(dst)
            masks.append(dval)
        return levels, [m.bool() for m in masks]
    for (h, w), (h2, w2) in zip(shapes, shapes[1:]):
        src = levels[-1]
        if kind == KIND_U8_HWC:
            dst = torch.empty((h2, w2, C), dtype=torch.uint8, device=src.device)
            _lib.check(L.dsic_image_halve_u8(_p(src), _p(dst), h, w, C, _stream()), "image_halve_u8")
        elif kind == KIND_U16_HWC:
            dst = torch.empty((h2, w2, C), dtype=torch.uint16, device=src.device)
            _lib.check(L.dsic_image_halve_u16(_p(src), _p(dst), h, w, C, _stream()), "image_halve_u16")
        else:
            dst = torch.empty((C, h2, w2), dtype=torch.float32, device=src.device)
            _lib.check(L.dsic_image_halve_f32(_p(src), _p(dst), C, h, w, _stream()), "image_halve_f32")
        levels.append(dst)
    return levels


def pack_pyramid_stream(level_streams) -> bytes:
    """DSICI streams of an image and its overviews, level 0 first -> one DSICP stream (pure Python): the directory
    (H, W from each stream's own head; absolute offset and length of its bytes), then the streams back to back.
    ValueError for fewer than two levels, sizes that are not the halving chain of level 0, or levels that disagree on
    C, kind, the model's shape or the numerics tag."""
    streams = [bytes(s) for s in level_streams]
    if len(streams) < 2:
        raise ValueError(f"pack_pyramid_stream: {len(streams)} level(s); a pyramid has at least two")
    heads = [_read_framing(_Source(s))[0] for s in streams]
    _check_levels([(h["H"], h["W"]) for h in heads], heads)
    off = _PHEAD.size + _PLEVEL.size * len(streams)
    parts = [_PHEAD.pack(PMAGIC, PVERSION, len(streams))]
    for h, s in zip(heads, streams):
        parts.append(_PLEVEL.pack(h["H"], h["W"], off, len(s)))
        off += len(s)
    return b"".join(parts + streams)


def _check_levels(sizes, heads):
    """sizes: (H, W) per level as the directory has them; heads: the DSICI header fields of the levels that were read
    (None for the others)."""
    for l in range(1, len(sizes)):
        want = (_halved(sizes[l - 1][0]), _halved(sizes[l - 1][1]))
        if tuple(sizes[l]) != want:
            raise ValueError(f"DSICP stream: level {l} is {sizes[l][0]}x{sizes[l][1]}, level {l - 1} "
                             f"({sizes[l - 1][0]}x{sizes[l - 1][1]}) halves to {want[0]}x{want[1]}")
    first = None
    for l, h in enumerate(heads):
        if h is None:
            continue
        if (h["H"], h["W"]) != tuple(sizes[l]):
            raise ValueError(f"DSICP stream: the directory gives level {l} as {sizes[l][0]}x{sizes[l][1]}, its own "
                             f"head says {h['H']}x{h['W']}")
        if first is None:
            first = l
        for key in _SAME_IN_LEVELS:
            if h.get(key) != heads[first].get(key):                        # scale: version 6 only
                raise ValueError(f"DSICP stream: levels {first} and {l} disagree on {key} ({heads[first].get(key)} "
                                 f"and {h.get(key)})")


def _read_directory(src, head):
    """The directory of a DSICP _Source whose first _HEAD.size bytes are `head` (the directory of two levels is just
    as long) -> [{"H", "W", "offset", "length"}]; the level streams are not read."""
    if len(head) < _PHEAD.size:
        raise ValueError("truncated DSICP stream")
    _, version, levels = _PHEAD.unpack_from(head, 0)
    if version != PVERSION:
        raise ValueError(f"DSICP stream version {version}, this reader knows {PVERSION}")
    if levels < 2:
        raise ValueError(f"DSICP stream: {levels} level(s); a pyramid has at least two")
    end = _PHEAD.size + _PLEVEL.size * levels
    if end > src.size:
        raise ValueError("truncated DSICP stream")
    table = bytes(head[:end])
    if end > len(table):
        table += bytes(src.read_at(len(table), end - len(table)))
    out, off = [], end
    for l in range(levels):
        H, W, offset, length = _PLEVEL.unpack_from(table, _PHEAD.size + _PLEVEL.size * l)
        if offset != off:
            raise ValueError(f"DSICP stream: level {l} at offset {offset}, expected {off} (the directory's end, then "
                             "the levels back to back)")
        off += length
        if off > src.size:
            raise ValueError("truncated DSICP stream")
        out.append({"H": H, "W": W, "offset": offset, "length": length})
    if off != src.size:
        raise ValueError(f"DSICP stream: {src.size - off} trailing bytes")
    _check_levels([(d["H"], d["W"]) for d in out], [])
    return out


class _Level:
    """One level's bytes of a DSICP _Source as a source of its own: offsets count from the level's first byte, and
    nothing outside its `size` bytes is read, so the DSICI checks for truncated and trailing bytes hold per level."""

    def __init__(self, source, base, size):
        self.source, self.base, self.size = source, base, size

    @property
    def bytes_read(self):
        return self.source.bytes_read

    def read_at(self, off, n):
        return self.source.read_at(self.base + off, max(0, min(n, self.size - off)))


def _open_level(src, level):
    """src (bytes or a file object) -> (the source the chosen level's DSICI stream is read from, its index with
    offsets inside that source, the level's first byte in src, the DSICP directory or None for a DSICI src)."""
    source = _Source(src)
    head = source.read_at(0, _HEAD.size)
    try:
        level = 0 if level is None else operator.index(level)
    except TypeError:
        raise ValueError(f"level={level!r} is not an integer") from None
    if bytes(head[:len(PMAGIC)]) != PMAGIC:
        if level != 0:
            raise ValueError(f"level={level}: a DSICI stream holds one image, level 0")
        return source, _index_of(source, head), 0, None
    levels = _read_directory(source, head)
    if not 0 <= level < len(levels):
        raise ValueError(f"level={level}: the DSICP stream holds levels 0 .. {len(levels) - 1}")
    d = levels[level]
    view = _Level(source, d["offset"], d["length"])
    ix = _index_of(view)
    _check_levels([(v["H"], v["W"]) for v in levels], [None] * level + [ix])
    ix.update(level=level, levels=levels)
    return view, ix, d["offset"], levels


def unpack_pyramid_stream(stream) -> dict:
    """DSICP stream -> {"version", "levels": [{"H", "W", "offset", "length", "stream"}]}, stream the level's DSICI
    bytes (pure Python).  ValueError on a wrong magic or version, fewer than two levels, a truncated directory or
    stream, offsets that are not the directory's end and then back to back, trailing bytes, sizes that are not the
    halving chain of level 0, a level whose own head gives another H or W than the directory, and levels that
    disagree on C, kind, N, M, in_ch, spatial_params or the numerics tag."""
    s = bytes(stream)
    src = _Source(s)
    head = src.read_at(0, _HEAD.size)
    if bytes(head[:len(PMAGIC)]) != PMAGIC:
        raise ValueError("truncated DSICP stream" if len(head) < len(PMAGIC) and bytes(head) == PMAGIC[:len(head)]
                         else "not a DSICP pyramid stream")
    levels = _read_directory(src, head)
    for d in levels:
        d["stream"] = s[d["offset"]:d["offset"] + d["length"]]
    _check_levels([(d["H"], d["W"]) for d in levels], [_read_framing(_Source(d["stream"]))[0] for d in levels])
    return {"version": PVERSION, "levels": levels}


def band_range(img, valid=None) -> list:
    """[(lo, hi), ...]: per band the minimum and maximum of a uint16 [H,W,C] image on the GPU (dsic_band_range_u16:
    one pass over the image on many workgroups, then one small copy to the host).  The default scale of
    compress_image.  valid: a torch.bool or uint8 [H,W] mask on the GPU; then over the valid pixels only
    (dsic_band_range_valid_u16), and a band without a valid pixel is (0, 0)."""
    kind, H, W, C = _image_kind(img, "band_range")
    if kind != KIND_U16_HWC:
        raise TypeError(f"band_range: expected uint16 [H,W,C], got {img.dtype}")
    if not img.is_cuda:
        raise RuntimeError(f"band_range: expected a tensor on the GPU (no CPU fallback), got {img.device}")
    img = img.contiguous()
    out = torch.empty(2 * C, dtype=torch.int32, device=img.device)
    if valid is not None:
        if tuple(valid.shape) != (H, W) or valid.dtype not in (torch.bool, torch.uint8) or valid.device != img.device:
            raise ValueError(f"band_range: valid must be a bool or uint8 [{H}, {W}] tensor on {img.device}")
        valid = valid.to(torch.uint8).contiguous()
        _lib.check(_lib.load().dsic_band_range_valid_u16(_p(img), _p(valid), H, W, C, _p(out), _stream()),
                   "band_range_valid_u16")
    else:
        _lib.check(_lib.load().dsic_band_range_u16(_p(img), H, W, C, _p(out), _stream()), "band_range_u16")
    v = [int(x) & 0xFFFFFFFF for x in out.cpu().tolist()]
    return list(zip(v[0::2], v[1::2]))


# What gathers the tiles of a kind: the export, whether the tiles are planar ([n,C,th,tw]; else [n,th,tw,C]), their dtype,
# and whether the export takes the scale (a uint16 image is normalised on the way: the tiles gather_f32 cuts from norm(img)).
_Gather = collections.namedtuple("_Gather", "export planar dtype lohi")
_GATHERS = {KIND_U8_HWC: _Gather("tile_gather_u8", False, torch.uint8, False),
            KIND_F32_CHW: _Gather("tile_gather_f32", True, torch.float32, False),
            KIND_U16_HWC: _Gather("tile_gather_u16", True, torch.float32, True)}


def _gather(img, kind, g, C, ids, scale=None):
    """The tiles `ids` (ascending tile numbers) of an image on the device as one batch tensor: one library call per run
    of consecutive numbers, into that run's slice, so a batch of consecutive tiles is one call."""
    e = _GATHERS[kind]
    what = e.export + ("_ov" if g["overlap"] else "")
    export = getattr(_lib.load(), "dsic_" + what)
    tiles = torch.empty((len(ids), C, g["th"], g["tw"]) if e.planar else (len(ids), g["th"], g["tw"], C), dtype=e.dtype,
                        device=img.device)
    args = ((g["H"], g["W"], C, g["th"], g["tw"]) + ((g["overlap"],) if g["overlap"] else ())
            + ((_lohi(scale),) if e.lohi else ()))
    a = 0
    while a < len(ids):
        b = a + 1
        while b < len(ids) and ids[b] == ids[b - 1] + 1:
            b += 1
        _lib.check(export(_p(img), _p(tiles[a:b]), *args, ids[a], b - a, _stream()), what)
        a = b
    return tiles


# ---- compress_image's options: what each goes with, stated once -----------------------------------------------------------
# _REFUSALS: (an option, what it meets, the refusal), in the order a caller meets them: the first row that applies is the
# message.  "value": the option's own check (_checked_options), which for an option that FORMATS knows is the check of
# its field (_FIELDS); "kind": an image kind its version of FORMATS does not list; any other name is a flag of
# _checked_options.  Beyond FORMATS the writer refuses float32 with max_error and nodata, nodata with overviews, fill
# without valid; and max_error's own rows stand behind level 0's geometry, which they are checked against.
def _with(a, b, note=""):
    return a, b, f"compress_image: {a} together with {b} is not supported{note}"


_8BIT = " (the residual tables and the mask classifier are 8-bit)"
_OPTION_KINDS = {"valid" if e.key == "fill" else e.key: e.kinds for e in FORMATS.values() if e.key}
_REFUSALS = (
    ("max_error", "value", None), ("tolerance", "value", None),
    ("tolerance", "kind", "compress_image: tolerance bounds the error of a uint16 [H,W,C] image; for a uint8 image use "
                          "max_error (float32 has neither)"),
    _with("tolerance", "overlap > 0"), _with("tolerance", "valid"), _with("tolerance", "nodata"),
    _with("tolerance", "max_error"),
    ("fill", "no valid", "compress_image: fill={fill!r} goes with valid, the mask it fills"),
    ("valid", "kind", "compress_image: a validity mask goes with integer pixel values; pass the image as uint8 or uint16 "
                      "[H,W,C], not float32"),
    _with("valid", "overlap > 0"), _with("valid", "max_error"), _with("valid", "nodata"),
    ("valid", "value", None), ("fill", "value", None),
    ("max_error", "kind", _with("max_error", "a uint16 image", _8BIT)[2]),
    ("nodata", "kind", _with("nodata", "a uint16 image", _8BIT)[2]),
    ("a uint16 image", "value", None),
    ("scale", "kind", "compress_image: scale goes with a uint16 [H,W,C] image, not with uint8 or float32"),
    ("scale", "value", None), ("nodata", "value", None),
    ("nodata", "float32", "compress_image: nodata compares integer pixel values; pass the image as uint8 [H,W,C], not "
                          "float32"),
    _with("nodata", "overlap > 0"), _with("nodata", "max_error"), _with("nodata", "overviews > 0"),
    ("segments", "value", None), ("channels", "value", None), ("batch", "value", None), ("level 0", "value", None),
    ("max_error", "float32", "compress_image: max_error bounds the error of integer pixel values; pass the image as uint8 "
                             "[H,W,C], not float32"),
    _with("max_error", "overlap > 0", " (the predictor would be the blended image)"),
    ("overviews > 0", "value", None),
)
_Options = collections.namedtuple("_Options", "tile batch tail segments overlap tau nodata scale fill tol masked")


def _checked_options(model, kind, H, W, C, tile, batch, tail, segments, overlap, max_error, overviews, nodata, scale, valid,
                     fill, tolerance) -> _Options:
    """compress_image's arguments, checked against each other and the image before anything touches the device (the
    rows of _REFUSALS, in order) -> the options as the levels take them; scale is None where band_range decides it."""
    what = "compress_image"
    N, M, in_ch, spatial = _model_shape(model)
    v = {"max_error": max_error, "tolerance": tolerance, "nodata": nodata, "scale": scale, "fill": fill}
    on = {"max_error": max_error is not None, "tolerance": tolerance is not None, "nodata": nodata is not None,
          "scale": scale is not None, "valid": valid is not None, "no valid": valid is None, "overlap > 0": overlap != 0,
          "fill": not (isinstance(fill, int) and not isinstance(fill, bool) and fill == 0), "overviews > 0": overviews != 0,
          "a uint16 image": kind == KIND_U16_HWC, "float32": kind == KIND_F32_CHW}
    shapes = [(H, W)]

    def need(ok, text):
        if not ok:
            raise ValueError(f"{what}: {text}")

    def field(key):                        # the check of a caller's value that the stream's field table holds
        return lambda: _FIELDS[key].dump(None, {key: v[key], "kind": kind}, what)[0]

    def level(l):                          # the geometry of one level -> the overlap as a stream holds it
        if l == 0 and on["overviews > 0"]:
            shapes[:] = overview_shapes(H, W, overviews)
        try:
            g = tile_grid(*shapes[l], tile, overlap)
            return _check_overlap(overlap, g["th"], g["tw"], what)
        except ValueError as e:
            raise ValueError(f"{e} (overview level {l}, {shapes[l][0]}x{shapes[l][1]})" if l else str(e)) from None

    checks = {"max_error": field("max_error"), "tolerance": field("tolerance"), "nodata": field("nodata"),
              "fill": field("fill"), "scale": lambda: check_scale(scale, C, what),
              "valid": lambda: _check_valid(valid, H, W, what),
              "a uint16 image": lambda: need(1 <= C <= 4, f"a uint16 image has 1 to 4 bands, got {C}"),
              "segments": lambda: entropy.check_segments(segments, M, what),
              "channels": lambda: need(C == in_ch, f"image has {C} channels, the model takes {in_ch}"),
              "batch": lambda: need(int(batch) >= 1, f"batch={int(batch)}") or int(batch),
              "level 0": lambda: level(0), "overviews > 0": lambda: [level(l) for l in range(1, len(shapes))]}
    for option, other, text in _REFUSALS:
        if not on.get(option, True):       # segments, channels, batch and level 0 are always there
            continue
        if other == "value":
            v[option] = checks[option]()
        elif kind not in _OPTION_KINDS[option] if other == "kind" else on[other]:
            raise ValueError(text.format(fill=fill))
    return _Options(tile, v["batch"], tail, v["segments"], v["level 0"], v["max_error"], v["nodata"], v["scale"],
                    v["fill"] if on["valid"] else None, v["tolerance"], on["valid"])


def _at_level(o, level) -> _Options:
    """The options of one level of the pyramid: level 0 alone carries the error bounds (an overview is a preview)."""
    return o if level == 0 else o._replace(tau=None, tol=None)


def _compress_level(model, x, o, valid=None) -> bytes:
    """One image that lies contiguous on the model's device, with its level's checked options (and its validity image:
    uint8 [H,W], 0 = invalid) -> its DSICI stream.  The header is made first; the version it will be written as says
    what travels beside the containers.  With a mask block only the tiles that are not empty are coded, in ascending
    tile number, `batch` to a container; gathered run by run, every tile's strings are those of the stream without the
    mask.  With a residual layer compress_to_container's work is done here, keeping the forward x_hat: the predictor
    the decoder will have bit for bit."""
    kind, H, W, C = _image_kind(x, "compress_image")
    N, M, in_ch, spatial = _model_shape(model)
    g = tile_grid(H, W, o.tile, o.overlap)
    header = {"numerics": entropy.numerics_tag(), "H": H, "W": W, "C": C, "kind": kind, "th": g["th"], "tw": g["tw"],
              "N": N, "M": M, "in_ch": in_ch, "spatial_params": spatial, "batch": o.batch, "segments": o.segments,
              "overlap": o.overlap}
    header.update({key: value for key, value in (("max_error", o.tau), ("nodata", o.nodata), ("scale", o.scale),
                                                 ("fill", o.fill), ("tolerance", o.tol)) if value is not None})
    e = FORMATS[_version_for(header)]
    ids = range(g["n"])
    if e.mask:                             # nodata: the mask is read off the pixels; valid: it comes from the mask itself
        owned = [_owned_in_tile(g, t) for t in ids]
        counts = _mask.classify(x, g, C, header[e.key]) if valid is None else _mask.classify_valid(valid, g)
        states = _mask.tile_states(counts, [(b - a) * (d - c) for a, b, c, d in owned])
        ids = [t for t, s in enumerate(states) if s != _mask.EMPTY]
    blobs, residuals, block = [], None if e.layer is None else [], None
    for first in range(0, len(ids), o.batch):
        sel = ids[first:first + o.batch]
        tiles = _gather(x, kind, g, C, sel, o.scale)
        if e.layer is None:
            blobs.append(entropy.compress_to_container(model, tiles, o.tail, segments=o.segments))
            continue
        c = entropy._coded_batch(model, tiles, o.tail, entropy.DEFAULT_LMAX, "compress_image", pack=True,
                                 segments=o.segments)
        blobs.append(c["container"][:c["container_bytes"]].cpu().numpy().tobytes())
        if e.layer is _residual16:             # the gathered tiles are normalised float32: the image is read in place
            residuals.append(_residual16.encode_block(x, c["x_hat"], H, W, g["th"], g["tw"], _lohi(o.scale), o.tol, sel[0]))
        else:
            residuals.append(_residual.encode_block(tiles, c["x_hat"], [_owned_in_tile(g, t) for t in sel], o.tau))
    if e.mask:
        block = (_mask.encode_block(x, g, C, header[e.key], states) if valid is None else
                 _mask.encode_block(valid, g, None, header[e.key], states))
    return pack_image_stream(header, blobs, residuals, block)


@torch.no_grad()
def compress_image(model, img, tile=256, batch=64, tail=10, segments=1, overlap=0, max_error=None,
                   overviews=0, nodata=None, scale=None, valid=None, fill=0, tolerance=None) -> bytes:
    """img: uint8 [H,W,C], uint16 [H,W,C] or float32 [C,H,W] in [0,1], on the CPU or the GPU -> one DSICI stream.  The
    image is uploaded once; each batch of `batch` tiles is gathered on the device (reflect padding included) and becomes one
    DSIC2 container.  segments = K > 1 (1, 2, 4, 8 or 16, dividing M): every tile's y string is K independent strings
    (DSIC3 containers, stream version 2), which the decoders read on K waves per tile; the decoded image is the same.
    overlap = O > 0 (a multiple of 16, at most half a tile side): tiles share O pixels with their neighbours
    (tile_grid) and the decoders cross-fade them over that band (stream version 3).
    max_error = tau (an integer 0 .. 127; uint8 images, overlap = 0): the near-lossless mode (stream version 4).
    Behind every container, byte for byte the one written without max_error, goes a residual block (residual.py),
    and the decoders return a uint8 image within tau of img on every pixel and channel; 0 is lossless.
    overviews = n > 0 writes a DSICP stream instead (pack_pyramid_stream): the image and its n overview levels
    (build_overviews, made on the device from the one upload), every level coded with the same tile, batch, tail,
    segments and overlap, its bytes the DSICI stream this call returns for that level's image alone; a level smaller
    than a tile is one smaller tile (tile_grid), and a level the codec does not take (overview_shapes), or whose
    tiles are too small for the overlap, is a ValueError before anything is coded.  max_error applies to level 0
    only, which is then the version-4 stream of the call without overviews; the overview levels are the lossy
    streams: an overview is a preview, and a residual layer there would add bytes to bound an error against an image
    the caller never supplied.
    nodata = v (an integer 0 .. 255; uint8 images): a pixel whose C channels all equal v is nodata, and the stream
    (version 5) keeps that mask exactly (mask.py).  Tiles whose owned pixels inside the image are all nodata are
    neither gathered, coded nor decoded; the other tiles' strings are byte for byte those of the stream without
    nodata, and a tile that holds both kinds of pixel carries its mask beside them.  The decoders return v on all
    channels (v / 255.0f for out="f32") at every nodata pixel of img, and at every other pixel the bits the stream
    without nodata decodes to.  Not promised: a valid pixel may happen to decode to (v, ..., v), as it can today.
    A uint16 image (1 to 4 bands) writes stream version 6, which carries a per-band scale (lo, hi): scale = None takes
    each band's own minimum and maximum (band_range, on the device), otherwise scale is a sequence of C integer pairs
    with 0 <= lo <= hi <= 65535, e.g. [(0, 10000)] * C, and values outside a pair clip to it.  The model codes
    norm(img) (module docstring), so every container is byte for byte that of the float32 image norm(img) compressed
    with the same arguments; segments and overlap work unchanged, and the decoders return uint16 by default.  With
    overviews the scale is decided once, at level 0, and every level is written with it (halved values stay inside
    [lo, hi]).  max_error stays the uint8 mode; the bounded-error mode of a uint16 image is tolerance.
    tolerance = tau (an integer 0 .. 32767; uint16 images, overlap = 0): the bounded-error mode of 16-bit imagery
    (stream version 9).  Behind every container, byte for byte the one the version-6 stream of the same call without
    tolerance holds, goes a wide residual block (residual16.py), and the decoders return a uint16 image within tau of
    img on every pixel and band; 0 returns img itself, also where its values leave the scale (lo, hi), which then only
    affects the rate.  With overviews it applies to level 0 only, as max_error does; the overview levels are the
    version-6 streams.  The decoders take out=None or "u16" on such a stream; "u8" and "f32" are a ValueError.  The
    split of the residual follows each tile's largest step, so one outlier in a quiet tile costs raw bits on every
    sample of that tile (residual16.py).
    valid = mask (a torch.bool [H,W] tensor on the CPU or the GPU, True = the pixel holds data; uint8 and uint16
    images, with segments and with overviews) with fill = f (an integer 0 .. 255 for uint8, 0 .. 65535 for uint16, the
    value the decoders write at invalid pixels): the stream (version 8) keeps that mask exactly (mask.py; the block's
    nodata field carries fill).  Tiles whose owned pixels inside the image are all invalid are neither gathered, coded
    nor decoded; the other tiles' strings are byte for byte those of the same call without valid (for uint16: the
    version-6 stream written with the same scale), and a tile that holds both kinds of pixel carries its mask beside
    them.  With a uint16 image and scale = None the scale is each band's minimum and maximum over the valid pixels only
    (band_range(img, valid)); a band without a valid pixel gets (0, 0).  The decoders return f on all channels at every
    invalid pixel of img (f / 255.0f for a uint8 stream with out="f32"; out="u8" / "f32" on a uint16 stream is a
    ValueError: the normalised image has no value that means fill), and at every other pixel the bits the stream
    without valid decodes to; with_valid=True of the decoders and decompress_valid return the mask itself.  With
    overviews every level is the version-8 stream of that level's image and mask alone (build_overviews(img, n, valid),
    the masked halving), with level 0's fill and scale.  Invalid pixels inside coded tiles are coded as the caller left
    them: filling them with something smoother is a bit-rate optimisation that would give up the "same strings as the
    stream without valid" property.
    Every option's default (0 or None) writes the stream the call wrote before the option existed.  What does not go
    together is a ValueError before anything touches the device (_REFUSALS, in the order reported): max_error, nodata,
    valid and tolerance exclude each other and overlap > 0 (the predictor, the blend across skipped tiles and the
    halving would each need a masked variant of its own), nodata also overviews > 0; max_error and nodata go with uint8
    images only (the residual tables and the mask classifier are 8-bit, and float32 has no integer pixel values), valid
    with uint8 or uint16, tolerance and scale with uint16; fill goes with valid; and a value outside its range, or a
    mask of another shape or dtype."""
    kind, H, W, C = _image_kind(img, "compress_image")
    o = _checked_options(model, kind, H, W, C, tile, batch, tail, segments, overlap, max_error, overviews, nodata, scale,
                         valid, fill, tolerance)
    dev = next(model.parameters()).device
    x = img.to(dev).contiguous()
    v8 = valid.to(dev).to(torch.uint8).contiguous() if o.masked else None
    if kind == KIND_U16_HWC and o.scale is None:
        o = o._replace(scale=band_range(x, v8))
    levels, masks = [x], [v8]
    if overviews != 0 and o.masked:
        levels, masks = build_overviews(x, overviews, v8.bool())
        masks = [m.to(torch.uint8) for m in masks]
    elif overviews != 0:
        levels = build_overviews(x, overviews)
        masks = [None] * len(levels)
    streams = [_compress_level(model, lv, _at_level(o, level), m) for level, (lv, m) in enumerate(zip(levels, masks))]
    return streams[0] if overviews == 0 else pack_pyramid_stream(streams)


def _owned_in_tile(g, t):
    """(y0, y1, x0, x1): the rows and columns of tile t, counted from its origin, that it owns inside the H x W image."""
    i, j = divmod(t, g["nx"])
    (a, b), (c, d) = g["own_y"][i], g["own_x"][j]
    return a - g["ys"][i], min(b, g["H"]) - g["ys"][i], c - g["xs"][j], min(d, g["W"]) - g["xs"][j]


def _refuse_foreign(model, h, what):
    """A stream this decoder cannot rebuild the coder tables of: another numerics tag, or another model shape."""
    if int(h["numerics"]) != entropy.numerics_tag():
        raise EntropyError(f"{what}: the stream was written with numerics tag {h['numerics']:#x}, this "
                           f"decoder is {entropy.numerics_tag():#x}")
    mine = _model_shape(model)
    theirs = (h["N"], h["M"], h["in_ch"], h["spatial_params"])
    if mine != theirs:
        raise EntropyError(f"{what}: the stream was written by a model with (N, M, in_ch, spatial_params) = "
                           f"{theirs}, this one is {mine}")


def _stream_grid(h):
    """The tile grid a DSICI header describes; ValueError where its fields contradict each other."""
    H, W, C, th, tw = h["H"], h["W"], h["C"], h["th"], h["tw"]
    if C != h["in_ch"] or h["kind"] not in _format_of(h).kinds or h["batch"] < 1:
        raise ValueError("DSICI stream: inconsistent header")
    _check_image(H, W)
    if th % 16 or tw % 16 or th < 32 or tw < 32 or th > _ceil16(H) or tw > _ceil16(W):
        raise ValueError(f"DSICI stream: tile {th}x{tw} does not fit a {H}x{W} image")
    g = _grid(H, W, th, tw, _check_overlap(h.get("overlap", 0), th, tw, "DSICI stream"))
    coded = h.get("coded", g["n"])
    if coded > g["n"] or h["batches"] != -(-coded // h["batch"]):
        raise ValueError(f"DSICI stream: {h['batches']} batches for {coded} of {g['n']} tiles in batches of "
                         f"{h['batch']}")
    return g


def _check_batch_shape(k, shape_y, n, th, tw):
    if shape_y[0] != n or shape_y[2:] != [th // 16, tw // 16]:
        raise ValueError(f"DSICI stream: batch {k} holds {shape_y[0]} latents of {shape_y[2]}x{shape_y[3]}, "
                         f"expected {n} of {th // 16}x{tw // 16}")


def _out_image(kind, C, h, w, dev, what):
    """The empty output image of a decode and the stitch call's name stem: uint8 [h,w,C], uint16 [h,w,C] or float32
    [C,h,w]."""
    if kind == KIND_U16_HWC:
        return torch.empty((h, w, C), dtype=torch.uint16, device=dev), "u16"
    if kind == KIND_U8_HWC:
        if C not in (3, 4):
            raise ValueError(f"{what}: uint8 output needs 3 or 4 channels, the stream has {C}")
        return torch.empty((h, w, C), dtype=torch.uint8, device=dev), "u8"
    return torch.empty((C, h, w), dtype=torch.float32, device=dev), "f32"


# ---- decode: any window of an image stream from only its tiles; the whole image is the window (0, 0, H, W) ------
def _index_of(src, head=None):
    """stream_index on an open _Source (head: as _read_framing takes it)."""
    ix, frames, rframes = _read_framing(src, head)
    g, e = _stream_grid(ix), _format_of(ix)
    tiles, containers = [], []
    ids = None                                 # a mask: the grid numbers of the coded tiles, ascending
    if e.mask:
        states, mrecs = _mask.read_block_head(src.read_at, ix["mask_offset"], ix["mask_bytes"], g["n"], ix["th"],
                                              ix["tw"], ix[e.key])
        ids = [t for t, s in enumerate(states) if s != _mask.EMPTY]
        if len(ids) != ix["coded"]:
            raise ValueError(f"DSICI stream: the head says {ix['coded']} coded tiles, the mask block's states "
                             f"{len(ids)}")
    n_coded = g["n"] if ids is None else len(ids)
    for k, (off, size) in enumerate(frames):
        tag, shape_y, shape_z, images, segs, seg = entropy.read_container_segments(src.read_at, off, size)
        if segs != ix["segments"]:
            raise ValueError(f"DSICI stream: batch {k} holds {segs} segments per y string, the header says "
                             f"{ix['segments']}")
        if tag != ix["numerics"]:
            raise ValueError(f"DSICI stream: batch {k} carries numerics tag {tag:#x}, the stream's is "
                             f"{ix['numerics']:#x}")
        first = k * ix["batch"]
        _check_batch_shape(k, shape_y, min(ix["batch"], n_coded - first), ix["th"], ix["tw"])
        if (shape_y[1], shape_z[1]) != (ix["M"], ix["N"]):
            raise ValueError(f"DSICI stream: batch {k} holds latents of {shape_y[1]} and {shape_z[1]} channels, the "
                             f"header says {ix['M']} and {ix['N']}")
        if containers and shape_z[2:] != containers[0]["shape_z"][2:]:
            raise ValueError(f"DSICI stream: batch {k} holds hyper-latents of {shape_z[2]}x{shape_z[3]}, batch 0 of "
                             f"{containers[0]['shape_z'][2]}x{containers[0]['shape_z'][3]}")
        for b, (min_y, max_y, min_z, max_z, z_off, z_len, y_off, y_len) in enumerate(images):
            tiles.append({"k": k, "b": b, "min_y": min_y, "max_y": max_y, "min_z": min_z, "max_z": max_z,
                          "z_off": z_off, "z_len": z_len, "y_off": y_off, "y_len": y_len, "y_segs": seg[b]})
        containers.append({"offset": off, "bytes": size, "first": first, "tiles": len(images), "shape_y": shape_y,
                           "shape_z": shape_z})
        if ids is not None:
            containers[-1]["ids"] = ids[first:first + len(images)]
        if rframes:
            recs = e.layer.read_block_head(src.read_at, rframes[k][0], rframes[k][1], len(images), ix["C"], ix["th"],
                                           ix["tw"], ix[e.key])
            for tile, rec in zip(tiles[first:], recs):
                tile.update(rec)
            containers[-1].update(r_offset=rframes[k][0], r_bytes=rframes[k][1])
    if ids is not None:                        # the coded tiles' records, spread over the grid
        coded, tiles = dict(zip(ids, tiles)), []
        for t, state in enumerate(states):
            rec = coded.get(t) or {"k": None, "b": None, "min_y": 0, "max_y": 0, "min_z": 0, "max_z": 0, "z_off": 0,
                                   "z_len": 0, "y_off": 0, "y_len": 0, "y_segs": [0] * ix["segments"]}
            rec["state"] = state
            rec.update(mrecs.get(t, {}))
            tiles.append(rec)
    ix.update(grid=g, tiles=tiles, containers=containers, stream_bytes=src.size, index_bytes=src.bytes_read)
    return ix


def stream_index(src, level=None) -> dict:
    """Where every tile of a DSICI stream lies, from its heads alone (pure Python).  src: bytes / bytearray /
    memoryview, or a binary file object with seek and read.  Only the 60-byte header and, per batch, the 8-byte
    length, the 38-byte DSIC2 header and the 24-byte records are read (version 2: 64 bytes, and per batch the 42-byte
    DSIC3 header, the records and 4 bytes per y segment); the strings are skipped.  Returns the header fields of
    unpack_image_stream (no "blobs"; segments = y segments per tile, 1 for version 1; overlap, 0 for versions 1
    and 2, whose words add 8 bytes to a version-3 head) and
      grid         tile_grid's dict for H, W, th, tw
      tiles        per tile t (row-major, as the grid numbers them): k (batch), b (slot in it), min_y, max_y, min_z,
                   max_z, z_off, z_len, y_off, y_len (absolute byte offsets and lengths of its two strings), y_segs
                   (the lengths of the y string's segments, back to back from y_off; [y_len] for segments = 1)
      containers   per batch: offset, bytes, first (tile), tiles, shape_y, shape_z
    and for a version-4 stream (only then) max_error; per tile r_off, r_len (its span in the batch's residual block:
    C x r_L table entries, then 16 strings), r_smin, r_L (the residual's support) and r_segs (the 16 string lengths);
    per batch r_offset, r_bytes (the block).  Of a residual block the 30-byte head, the 12-byte records and the 64
    bytes of segment lengths per tile are read.
    and for a version-9 stream (only then) tolerance and scale; per tile r_off, r_len (its span in the batch's wide
    residual block: C x r_L table entries, r_k bit planes of C th tw / 8 bytes, then 16 strings), r_smin, r_L, r_k and
    r_segs; per batch r_offset, r_bytes.  Of a wide residual block the 30-byte head, the 16-byte records and the 64
    bytes of segment lengths per tile are read.
    and for a version-5 stream (only then) nodata, coded, mask_offset, mask_bytes (the mask block); per tile state (0
    empty, 1 full, 2 mixed), for an empty tile k = b = None and zero lengths, for a mixed tile m_off, m_len, m_mode (its
    mask payload, which tile_spans includes); per container ids, the grid numbers of its tiles.  Of the mask block the
    26-byte head, the state bytes and the 12-byte records are read.
    and for a version-8 stream (a validity mask) fill, coded, mask_offset, mask_bytes, per tile state and m_off, m_len,
    m_mode, per container ids, exactly as for version 5, and scale for kind 2; the nodata key is not set.
    and for a version-6 stream (only then) scale, the C pairs (lo, hi) of the uint16 image; they add 8 C bytes to the
    version-3 head, which index_bytes counts.
      stream_bytes, index_bytes (what this call read).
    ValueError as unpack_image_stream, entropy.unpack_container and decompress_image raise it: wrong magic or version,
    DSIC1 container, truncated stream or container, trailing bytes, batches that do not match the grid, latents that
    do not match the tile size, a container whose numerics tag or segment count is not the stream's, segment lengths
    that do not add up.

    On a DSICP stream: the index of level 0, or of `level`, read from the directory and that level's heads alone.
    Every offset (offset, r_offset, z_off, y_off, r_off) counts from the start of src, so tile_spans gives byte ranges
    of src; beside the keys above the dict has level, levels (the directory: H, W, offset, length per level),
    stream_bytes (the whole pyramid) and index_bytes (what this call read).  ValueError as unpack_pyramid_stream,
    for a level the stream does not hold, and for a level other than 0 of a DSICI stream."""
    _, ix, base, levels = _open_level(src, level)
    if levels is not None:
        _absolute_offsets(ix, base, levels)
    return ix


def _absolute_offsets(ix, base, levels):
    """The index of a DSICP level, its offsets counted inside the level's bytes -> counted from the pyramid's start."""
    if "mask_offset" in ix:
        ix["mask_offset"] += base
    for c in ix["containers"]:
        c["offset"] += base
        if "r_offset" in c:
            c["r_offset"] += base
    for t in ix["tiles"]:
        for key in ("z_off", "y_off", "r_off", "m_off"):
            if key in t:
                t[key] += base
    ix.update(stream_bytes=levels[-1]["offset"] + levels[-1]["length"])


def window_tiles(index_or_grid, y0, x0, h, w) -> list:
    """The tiles whose owned rectangle, clipped to H x W, meets the window rows [y0, y0+h) x columns [x0, x0+w),
    ascending (pure Python).  Owned ranges partition each axis, so these are tile rows y0 // th ... (y0+h-1) // th
    and the columns likewise.  On a grid with overlap these are the tiles with a non-zero blend weight on some pixel
    of the window: those whose support rectangle (sup_y x sup_x), clipped to H x W, meets it.  ValueError for an
    empty window or one that leaves the image."""
    g = index_or_grid.get("grid", index_or_grid)
    y0, x0, h, w = int(y0), int(x0), int(h), int(w)
    if y0 < 0 or x0 < 0 or h < 1 or w < 1 or y0 + h > g["H"] or x0 + w > g["W"]:
        raise ValueError(f"window {h}x{w} at ({y0}, {x0}) is empty or outside the {g['H']}x{g['W']} image")
    if g.get("overlap", 0):
        rows = [i for i, (a, b) in enumerate(g["sup_y"]) if a < y0 + h and min(b, g["H"]) > y0]
        cols = [j for j, (a, b) in enumerate(g["sup_x"]) if a < x0 + w and min(b, g["W"]) > x0]
    else:
        rows = range(y0 // g["th"], (y0 + h - 1) // g["th"] + 1)
        cols = range(x0 // g["tw"], (x0 + w - 1) // g["tw"] + 1)
    return [i * g["nx"] + j for i in rows for j in cols]


def tile_spans(index, tiles, masks=True) -> list:
    """Byte ranges (offset, length) of the stream that hold the strings of the given tiles (in a version-4
    stream also their residual spans; in a version-5 stream also the mask payloads of mixed tiles, unless masks is
    False): ascending, ranges that touch merged into one, empty strings dropped (pure Python)."""
    parts = []
    for t in tiles:
        r = index["tiles"][t]
        if r["z_len"]:
            parts.append((r["z_off"], r["z_len"]))
        if r["y_len"]:
            parts.append((r["y_off"], r["y_len"]))
        if r.get("r_len"):
            parts.append((r["r_off"], r["r_len"]))
        if masks and r.get("m_len"):
            parts.append((r["m_off"], r["m_len"]))
    parts.sort()
    spans = []
    for off, n in parts:
        if spans and spans[-1][0] + spans[-1][1] >= off + n:               # a tile named twice
            continue
        if spans and spans[-1][0] + spans[-1][1] == off:
            spans[-1][1] += n
        else:
            spans.append([off, n])
    return [tuple(s) for s in spans]


def _apply_mask(source, ix, tiles, img, kind, window, valid_out=None) -> int:
    """The nodata pixels of a window of a version-5 stream, after its coded tiles have been stitched: the payloads of
    the window's mixed tiles are read, checked (mask.check_payload) and uploaded in one small copy with their
    descriptors, unpacked to m planes (dsic_mask_unpack), and one pass (dsic_mask_apply_u8 / _f32) writes nodata at the
    set bits of the mixed tiles and over the whole owned rectangle of the empty ones; mask.MAX_TILES tiles at a time.
    Returns the padded payload bytes uploaded.
    A version-8 stream (a validity mask) goes the same way with its fill in the place of nodata, dsic_mask_apply_u16
    for a uint16 window.  valid_out: a uint8 [h,w] tensor of ones on the device, or None; the same planes then also
    give the window's validity (dsic_mask_window_u8).  img None: only that."""
    H, W, C, th, tw = ix["H"], ix["W"], ix["C"], ix["th"], ix["tw"]
    v = ix[_format_of(ix).key]
    masked = [t for t in tiles if ix["tiles"][t]["state"] != _mask.FULL]
    dev = img.device if img is not None else valid_out.device
    uploaded = 0
    for c0 in range(0, len(masked), _mask.MAX_TILES):
        sel = masked[c0:c0 + _mask.MAX_TILES]
        mixed = [t for t in sel if ix["tiles"][t]["state"] == _mask.MIXED]
        slot = {t: i for i, t in enumerate(mixed)}
        words = np.zeros(3 * len(mixed) + 2 * len(sel), dtype=np.int32)
        parts, off = [], 0
        for i, t in enumerate(mixed):
            r = ix["tiles"][t]
            parts.append(source.read_at(r["m_off"], r["m_len"]))
            _mask.check_payload(parts[-1], r["m_mode"], th, tw)
            words[3 * i:3 * i + 3] = (r["m_mode"], off, r["m_len"])
            off += r["m_len"]
        words[3 * len(mixed):] = np.array([(t, slot.get(t, -1)) for t in sel], dtype=np.int32).ravel()
        d_blob, total, d_words = entropy._upload_padded(parts, words, dev)
        d_words = d_words.view(torch.int32)
        planes = _mask.unpack_planes(d_blob, total, d_words, len(mixed), th, tw) if mixed else None
        if img is not None:
            _mask.apply_window(planes, len(mixed), d_words[3 * len(mixed):], len(sel), v, img, kind == KIND_U8_HWC, H,
                               W, C, th, tw, *window)
        if valid_out is not None:
            _mask.window_valid(planes, len(mixed), d_words[3 * len(mixed):], len(sel), valid_out, H, W, th, tw, *window)
        uploaded += entropy._padded_bytes(total) if mixed else 0
    return uploaded


def _check_out(out, ix, what):
    """out as the decoders take it -> the kind of the result; ix None: only whether out is a known word."""
    if out not in (None, "u8", "f32", "u16"):
        raise ValueError(f"{what}: out={out!r} (None, 'u8', 'f32' or 'u16')")
    if ix is None:
        return None
    e, u16 = _format_of(ix), ix["kind"] == KIND_U16_HWC                 # a uint16 stream, of any version, has a scale
    if out == "u16" and not u16:
        raise ValueError(f"{what}: out='u16' needs the scale of a uint16 stream (version {VERSION_U16}); this one is "
                         f"version {ix['version']}")
    if out in ("u8", "f32") and u16 and e.layer is not None:
        raise ValueError(f"{what}: out={out!r} on a uint16 stream with a tolerance (version {VERSION_TOL}): the bound "
                         "is on the uint16 values; take out=None or 'u16'")
    if out in ("u8", "f32") and u16 and e.mask:
        raise ValueError(f"{what}: out={out!r} on a uint16 stream with a validity mask (version {VERSION_VALID}): the "
                         "normalised image has no value that means fill")
    return ix["kind"] if out is None else _OUT_KINDS[out]


def _coded_tiles(ix, tiles):
    """Of a window's tiles those that hold strings: all, or in a masked stream (version 5 or 8) those that are not
    empty."""
    return tiles if not _format_of(ix).mask else [t for t in tiles if ix["tiles"][t]["state"] != _mask.EMPTY]


def _decode_tiles(model, source, ix, sel, what):
    """One dense decode batch: the tiles `sel` (ascending) of an indexed level, their strings read from `source` in
    one upload -> (g_s's output [n,C,th,tw], contiguous and not clamped; the padded string bytes uploaded; the device
    copy of sel; the q planes of a stream with a residual layer, else None)."""
    C, th, tw, e = ix["C"], ix["th"], ix["tw"], _format_of(ix)
    N, Hz, Wz = ix["containers"][0]["shape_z"][1:] if ix["containers"] else (ix["N"], 0, 0)
    n = len(sel)
    # the upload is the tiles' spans back to back: a string at stream offset o lies where its span does
    spans = tile_spans(ix, sel, masks=False)               # the mask payloads travel with _apply_mask
    starts, base = [off for off, _ in spans], [0]
    for _, length in spans:
        base.append(base[-1] + length)

    def at(off, length):
        i = bisect.bisect_right(starts, off) - 1
        return base[i] + off - starts[i] if length else 0

    recs = [ix["tiles"][t] for t in sel]
    images = [(r["min_y"], r["max_y"], r["min_z"], r["max_z"], at(r["z_off"], r["z_len"]), r["z_len"],
               at(r["y_off"], r["y_len"]), r["y_len"]) for r in recs]
    parts = [source.read_at(off, length) for off, length in spans]

    def tables_of(r):                          # a span begins with its tables
        i = bisect.bisect_right(starts, r["r_off"]) - 1
        a = r["r_off"] - starts[i]
        return parts[i][a:a + 2 * C * r["r_L"]]

    spec = None if e.layer is None else _residual.decode_spec(e.layer, recs, C, th, tw, ix[e.key], at, tables_of)
    x_hat, nbytes, ids, *q = entropy._decode_selected(model, images, parts, [n, ix["M"], th // 16, tw // 16],
                                                      [n, N, Hz, Wz], what, ride=sel, segments=ix["segments"],
                                                      seg_lengths=[r["y_segs"] for r in recs], residual=spec)
    return x_hat.contiguous(), nbytes, ids, (q[0] if q else None)


def _assemble_window(model, source, ix, tiles, window, kind, batches, what, valid_out=None):
    """The window image from its tiles' decoded batches.  batches yields (x_hat, padded bytes uploaded, ids, q or
    None) as _decode_tiles returns them, the window's coded tiles in ascending order; each is stitched (blended) into
    the window as it arrives.  Then the nodata or invalid pixels (_apply_mask) and the blend's finish.  Returns (the
    image, the bytes uploaded, the batches taken).  valid_out: None, or a uint8 [h,w] tensor of ones on the device that
    receives the window's validity (left all ones by a stream without a mask)."""
    H, W, C, th, tw = ix["H"], ix["W"], ix["C"], ix["th"], ix["tw"]
    y0, x0, h, w = window
    lohi = (_lohi(ix["scale"]),) if kind == KIND_U16_HWC else ()        # the uint16 calls take the scale last
    layer = _format_of(ix).layer               # a residual layer: the result is its integer image, converted for "f32"
    img, suffix = _out_image(kind if layer is None else _OUT_KINDS[layer.OUT], C, h, w,
                             next(model.parameters()).device, what)
    L, O = _lib.load(), ix["overlap"]
    fn = getattr(L, "dsic_tile_stitch_window_" + suffix)
    if O:       # the window's float32 canvas, zeroed: the output itself, or a temporary that the finish turns to uint8
        canvas = img.zero_() if kind == KIND_F32_CHW else torch.zeros((C, h, w), dtype=torch.float32, device=img.device)
    uploaded = taken = 0
    for x_hat, nbytes, ids, q in batches:
        n = x_hat.shape[0]
        if q is not None:
            layer.stitch_window(x_hat, q, ix[_format_of(ix).key], ids, img, H, W, C, th, tw, y0, x0, h, w, *lohi)
        elif O:
            for c0 in range(0, n, BLEND_IDS):
                _lib.check(L.dsic_tile_blend_window_f32(_p(x_hat[c0:]), _p(ids[c0:]), min(BLEND_IDS, n - c0),
                                                        _p(canvas), H, W, C, th, tw, O, y0, x0, h, w, _stream()),
                           "tile_blend_window_f32")
        else:
            _lib.check(fn(_p(x_hat), _p(ids), n, _p(img), H, W, C, th, tw, y0, x0, h, w, *lohi, _stream()),
                       "tile_stitch_window_" + suffix)
        uploaded += nbytes
        taken += 1
    if _format_of(ix).mask:                    # empty tiles hold no strings, and are filled here
        uploaded += _apply_mask(source, ix, tiles, img, kind, (y0, x0, h, w), valid_out)
    if O and kind == KIND_F32_CHW:
        _lib.check(L.dsic_tile_blend_finish_f32(_p(canvas), C, h, w, _stream()), "tile_blend_finish_f32")
    elif O and kind == KIND_U16_HWC:
        _lib.check(L.dsic_tile_blend_finish_u16(_p(canvas), _p(img), C, h, w, *lohi, _stream()), "tile_blend_finish_u16")
    elif O:
        _lib.check(L.dsic_tile_blend_finish_u8(_p(canvas), _p(img), C, h, w, _stream()), "tile_blend_finish_u8")
    if layer is not None and kind == KIND_F32_CHW:
        img = (img.permute(2, 0, 1).to(torch.float32) / 255).contiguous()
    return img, uploaded, taken


def _decode_window(model, src, window, out, batch, stats, what, level=0, opened=None, with_valid=False):
    """decompress_region's work; window None = the whole image, batch None = the stream's tiles per container.  Of a
    DSICP stream the chosen level is decoded, through a view of its bytes.  opened: (source, index) of a level that
    an ImageReader has opened and checked against the model already; then bytes_read counts from this call on."""
    _check_out(out, None, what)
    source, ix = opened if opened is not None else _open_level(src, level)[:2]
    read0 = source.bytes_read if opened is not None else 0
    kind = _check_out(out, ix, what)
    if opened is None:
        _refuse_foreign(model, ix, what)
    y0, x0, h, w = (0, 0, ix["H"], ix["W"]) if window is None else window
    tiles = window_tiles(ix, y0, x0, h, w)
    window = (int(y0), int(x0), int(h), int(w))
    batch = ix["batch"] if batch is None else batch
    coded = _coded_tiles(ix, tiles)
    batches = (_decode_tiles(model, source, ix, coded[first:first + batch], what)
               for first in range(0, len(coded), batch))
    valid = torch.ones(window[2:], dtype=torch.uint8, device=next(model.parameters()).device) if with_valid else None
    img, uploaded, decode_batches = _assemble_window(model, source, ix, tiles, window, kind, batches, what, valid)
    if stats is not None:
        stats.update(tiles=tiles, decode_batches=decode_batches, bytes_read=source.bytes_read - read0,
                     bytes_uploaded=uploaded)
    return (img, valid.bool()) if with_valid else img


@torch.no_grad()
def decompress_image(model, stream, out=None, level=0, with_valid=False):
    """DSICI stream -> the image on the model's device: uint8 [H,W,C] ((uint8)(clamp(x,0,1)*255), truncating, as
    torchvision's to_pil_image) or float32 [C,H,W] (clamp(x,0,1)); by default the kind of the encoder's input,
    out="u8" / "f32" overrides it.  The whole image as a window, decoded container by container; each decoded batch
    is stitched straight into the image.  A stream with overlap (version 3) is blended instead: each decoded batch
    is added into a zeroed float32 canvas (the output itself for float32) with the tiles' ramp weights, and a finishing
    pass takes min(v, 1) and, for uint8, (uint8)(v*255).  A near-lossless stream (version 4) decodes to the uint8 image
    clamp(p + q s, 0, 255) of residual.py, within max_error of the original; out="f32" returns that image / 255.  A DSICP stream (compress_image with
    overviews) decodes to its level `level`, 0 the full image, as that level's own DSICI stream does; any other level
    than 0 of a DSICI stream, or a level the pyramid does not hold, is a ValueError.  A uint16 stream (version 6)
    decodes by default, or with out="u16", to uint16 [H,W,C]: lo + uint32(clamp(x,0,1) * float32(hi - lo) + 0.5f) per
    band with the stream's own scale, rounded to nearest (with overlap: of the blended canvas); out="u8" / "f32" give
    the normalised image as for any other stream, the uint8 one being what the reference's (rgb*255).astype(uint8)
    saves.  out="u16" on a stream of another version is a ValueError: it has no scale.
    A stream with a validity mask (version 8, compress_image with valid) decodes to fill on all channels at every
    invalid pixel (fill / 255.0f for a uint8 stream with out="f32") and at every other pixel to the bits the stream
    without the mask decodes to; out="u8" / "f32" on a uint16 stream with a mask is a ValueError.  with_valid = True
    returns (image, valid), valid a torch.bool [H,W] on the device: the stream's mask, all True for a stream without
    one (a version-5 stream gives its nodata mask, inverted)."""
    return _decode_window(model, stream, None, out, None, None, "decompress_image", level, with_valid=with_valid)


@torch.no_grad()
def decompress_region(model, src, y0, x0, h, w, out=None, batch=64, stats=None, level=0, with_valid=False):
    """The window rows [y0, y0+h) x columns [x0, x0+w) of a DSICI stream, decoded from only the tiles that own its
    pixels: uint8 [h,w,C] or float32 [C,h,w] on the model's device, the same bytes decompress_image(...) gives there
    (out as in decompress_image).  src: the stream as bytes, or a binary file object, of which only the heads
    (stream_index) and the selected tiles' strings (tile_spans) are read.  The selected tiles are decoded in dense
    batches of at most `batch`, in ascending tile order, whatever containers they come from; each batch is one
    upload and is stitched (blended, for a stream with overlap: then "own" reads "weigh on", and the bits do not
    depend on `batch`) into the window as soon as it is decoded.  stats (a dict) receives tiles, decode_batches,
    bytes_read and bytes_uploaded (the padded string bytes; 52 bytes of descriptors per tile travel beside them).
    level: of a DSICP stream, the overview level to decode; the window is in that level's own pixel grid
    (level_window maps a level-0 window to it), and only the directory, that level's heads and its selected tiles'
    strings are read.  with_valid = True returns (image, valid) as decompress_image does, valid a torch.bool [h,w]."""
    batch = int(batch)
    if batch < 1:
        raise ValueError(f"decompress_region: batch={batch}")
    return _decode_window(model, src, (y0, x0, h, w), out, batch, stats, "decompress_region", level,
                          with_valid=with_valid)


@torch.no_grad()
def decompress_valid(src, y0=0, x0=0, h=None, w=None, level=0, device="cuda"):
    """The validity of the window rows [y0, y0+h) x columns [x0, x0+w) (h, w None: to the image's end) of a stream's
    level, torch.bool [h,w] on `device`, as decompress_region(..., with_valid=True) returns it.  No model is needed and
    nothing is decoded: only the heads and the mask payloads of the window's mixed tiles are read, and the planes are
    unpacked and written on the device (dsic_mask_unpack, dsic_mask_window_u8).  All True for a stream without a mask."""
    source, ix = _open_level(src, level)[:2]
    y0, x0 = int(y0), int(x0)
    h, w = ix["H"] - y0 if h is None else int(h), ix["W"] - x0 if w is None else int(w)
    tiles = window_tiles(ix, y0, x0, h, w)
    valid = torch.ones((h, w), dtype=torch.uint8, device=device)
    if _format_of(ix).mask:
        _apply_mask(source, ix, tiles, None, None, (y0, x0, h, w), valid)
    return valid.bool()


from .view import ImageReader, stretch_from_histogram, view_level  # noqa: E402  (view.py builds on the functions above)
from .view import affine_q16, rotation_affine, warp_level, warp_window, window_affine  # noqa: E402
from .view import COLORMAPS, colormap_from_anchors  # noqa: E402
from .view import SceneStack, stack_levels, stack_parts, stack_reduce  # noqa: E402
from .view import check_q16, compose_q16, stack_warp_parts  # noqa: E402
from .view import GRID_NONE, GRID_STEPS, affine_grid, check_grid, function_grid, grid_error, grid_level  # noqa: E402
from .view import grid_shape, grid_window, projective_grid  # noqa: E402
from .view import ZONE_NONE, zonal_args, zonal_percentile, zonal_table  # noqa: E402
