"""CPU-only: the overview pyramid without a GPU.  The NumPy restatement of the two halvings (pyramid_ref.py) against
float64 means, the pure-Python geometry of codec.py (overview_shapes, level_window, level_for), the DSICP stream
(pack / unpack round trip and every refusal), the index of a level with offsets that count from the pyramid's first
byte, and the two new names in the C header and the binding."""
import io
import os
import random
import re
import struct

import numpy as np
import pytest

import pyramid_ref as P
from dsic_amd import codec, entropy, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAG = 0x40302
N, M = 128, 192


# ---- the restatement against float64 ------------------------------------------------------------------------------
def _edge_padded(img, axes):
    """the image with its last row / column repeated to even sides"""
    pad = [(0, 0)] * 3
    for ax in axes:
        pad[ax] = (0, img.shape[ax] % 2)
    return np.pad(img, pad, mode="edge")


def _block_means_f64(img, axes):
    """float64 mean of every 2 x 2 block of an image with even sides along `axes`"""
    v = img.astype(np.float64)
    ay, ax = axes
    sl = [slice(None)] * 3

    def take(dy, dx):
        s = list(sl)
        s[ay], s[ax] = slice(dy, None, 2), slice(dx, None, 2)
        return v[tuple(s)]
    return (take(0, 0) + take(0, 1) + take(1, 0) + take(1, 1)) / 4.0


@pytest.mark.parametrize("H,W,C", [(64, 48, 3), (33, 35, 4), (1, 7, 3), (6, 1, 1)])
def test_uint8_restatement_is_the_mean_rounded_half_up(H, W, C):
    rng = np.random.default_rng(H * 1000 + W)
    for img in (rng.integers(0, 256, size=(H, W, C), dtype=np.uint8), np.zeros((H, W, C), np.uint8),
                np.full((H, W, C), 255, np.uint8)):
        got = P.halve_u8(img)
        assert got.dtype == np.uint8 and got.shape == (P.halved(H), P.halved(W), C)
        want = np.floor(_block_means_f64(_edge_padded(img, (0, 1)), (0, 1)) + 0.5)
        assert np.array_equal(got.astype(np.float64), want)
    assert P.halve_u8(np.zeros((H, W, C), np.uint8)).max() == 0
    assert P.halve_u8(np.full((H, W, C), 255, np.uint8)).min() == 255


def test_uint8_rounding_on_every_block_sum():
    """every sum 0 .. 1020 of a block: sums of the form 4k + 2 round up, 4k + 1 down"""
    sums = np.arange(1021)
    a = np.minimum(sums, 255)
    b = np.minimum(sums - a, 255)
    c = np.minimum(sums - a - b, 255)
    d = sums - a - b - c
    img = np.stack([np.stack([a, b], 1).ravel(), np.stack([c, d], 1).ravel()]).astype(np.uint8)[:, :, None]
    assert np.array_equal(P.halve_u8(img)[0, :, 0], (sums + 2) // 4)


@pytest.mark.parametrize("C,H,W", [(3, 64, 48), (1, 33, 35), (4, 17, 2)])
def test_float32_restatement_lies_within_one_ulp_of_the_float64_mean(C, H, W):
    rng = np.random.default_rng(C * 100 + H)
    img = rng.random((C, H, W), dtype=np.float32)
    got = P.halve_f32(img)
    assert got.dtype == np.float32 and got.shape == (C, P.halved(H), P.halved(W))
    want = _block_means_f64(_edge_padded(img, (1, 2)), (1, 2))
    assert np.all(np.abs(got.astype(np.float64) - want) <= np.spacing(want.astype(np.float32)).astype(np.float64))


def test_float32_restatement_keeps_nan_and_negative_zero():
    img = np.zeros((1, 4, 4), np.float32)
    img[0, :2, :2] = -0.0
    img[0, 2, 2] = np.nan
    got = P.halve_f32(img)
    assert np.signbit(got[0, 0, 0]) and got[0, 0, 0] == 0 and not np.signbit(got[0, 0, 1])
    assert np.isnan(got[0, 1, 1]) and not np.isnan(got[0, 1, 0])


def test_odd_sides_repeat_the_last_row_and_column():
    rng = np.random.default_rng(5)
    u8 = rng.integers(0, 256, size=(7, 9, 3), dtype=np.uint8)
    f32 = rng.random((3, 7, 9), dtype=np.float32)
    assert np.array_equal(P.halve_u8(u8), P.halve_u8(_edge_padded(u8, (0, 1))))
    assert np.array_equal(P.halve_f32(f32), P.halve_f32(_edge_padded(f32, (1, 2))))
    # the last output row of an odd side is the mean of one source row, the corner one source pixel
    assert np.array_equal(P.halve_u8(u8)[-1, -1], u8[-1, -1])
    assert np.array_equal(P.halve_u8(u8)[-1, 0], (u8[-1, 0].astype(int) + u8[-1, 1] + 1) >> 1)
    assert np.array_equal(P.halve_f32(f32)[:, -1, -1], f32[:, -1, -1])
    one = P.chain(u8, 4)
    assert [a.shape[:2] for a in one] == P.shapes(7, 9, 4) == [(7, 9), (4, 5), (2, 3), (1, 2), (1, 1)]


# ---- geometry -------------------------------------------------------------------------------------------------------
def test_overview_shapes():
    assert codec.overview_shapes(330, 530, 4) == [(330, 530), (165, 265), (83, 133), (42, 67), (21, 34)]
    assert codec.overview_shapes(330, 530, 4) == P.shapes(330, 530, 4)
    assert codec.overview_shapes(330, 530, 0) == [(330, 530)]
    with pytest.raises(ValueError, match="level 5"):                      # 11 x 17 pads to 16 rows
        codec.overview_shapes(330, 530, 5)
    with pytest.raises(ValueError, match="level 0"):
        codec.overview_shapes(8, 530, 2)
    with pytest.raises(ValueError, match="level 2"):                      # 17 rows pad to 32: 15 of reflection < 17; 9 do not
        codec.overview_shapes(36, 100, 3)
    assert codec.overview_shapes(36, 100, 1) == [(36, 100), (18, 50)]
    for bad in (-1, 1.5, "2", None):
        with pytest.raises(ValueError):
            codec.overview_shapes(330, 530, bad)


def test_level_window_covers_the_window_and_is_minimal():
    H, W = 13, 11
    for level in range(4):
        s = 1 << level
        for y0 in range(H):
            for h in range(1, H - y0 + 1):
                rows = {y >> level for y in range(y0, y0 + h)}           # the level rows whose blocks meet the window
                for x0, w in ((0, 1), (3, 5), (W - 1, 1), (2, W - 2), (5, 3)):
                    cols = {x >> level for x in range(x0, x0 + w)}
                    ly, lx, lh, lw = codec.level_window(level, y0, x0, h, w)
                    assert (ly, ly + lh - 1, lx, lx + lw - 1) == (min(rows), max(rows), min(cols), max(cols))
                    assert ly * s <= y0 and (ly + lh) * s >= y0 + h and lx * s <= x0 and (lx + lw) * s >= x0 + w
    assert codec.level_window(0, 3, 4, 5, 6) == (3, 4, 5, 6)
    # a window of the image stays inside the level
    for level, (h, w) in enumerate(P.shapes(330, 530, 4)):
        assert codec.level_window(level, 0, 0, 330, 530) == (0, 0, h, w)
        assert codec.level_window(level, 329, 529, 1, 1) == (h - 1, w - 1, 1, 1)
    with pytest.raises(ValueError):
        codec.level_window(1, 0, 0, 0, 4)
    with pytest.raises(ValueError):
        codec.level_window(-1, 0, 0, 4, 4)


def test_level_for():
    levels = [{"H": h, "W": w} for h, w in P.shapes(330, 530, 3)]        # longer sides 530, 265, 133, 67
    ix = {"H": 330, "W": 530, "levels": levels}
    assert codec.level_for(ix, 67) == 3 and codec.level_for(ix, 68) == 2 and codec.level_for(ix, 133) == 2
    assert codec.level_for(ix, 134) == 1 and codec.level_for(ix, 266) == 0 and codec.level_for(ix, 530) == 0
    assert codec.level_for(ix, 531) == 0 and codec.level_for(ix, 10 ** 6) == 0      # none is: level 0
    assert codec.level_for(ix, 1) == 3
    assert codec.level_for({"H": 330, "W": 530}, 10) == 0                # a plain stream's index


# ---- the DSICP stream -------------------------------------------------------------------------------------------
def _level_stream(H, W, tile=128, batch=5, seed=0, **over):
    """A DSICI stream in pure Python with made-up strings -> (stream, strings per tile)."""
    rng = random.Random(seed * 7919 + H)
    g = codec.tile_grid(H, W, tile)
    header = {"numerics": TAG, "H": H, "W": W, "C": 3, "kind": 0, "th": g["th"], "tw": g["tw"], "N": N, "M": M,
              "in_ch": 3, "spatial_params": 0, "batch": batch}
    header.update(over)
    strings, blobs = [], []
    for first in range(0, g["n"], batch):
        B = min(batch, g["n"] - first)
        comp = {"strings": [[bytes(rng.getrandbits(8) for _ in range(rng.choice([0, 3, 17, 40]))),
                             bytes(rng.getrandbits(8) for _ in range(rng.choice([1, 16, 33, 250])))] for _ in range(B)],
                "shape_y": [B, header["M"], g["th"] // 16, g["tw"] // 16],
                "shape_z": [B, header["N"], g["th"] // 64, g["tw"] // 64],
                "min_y": [-3] * B, "max_y": [4] * B, "min_z": [-2] * B, "max_z": [2] * B,
                "numerics": header["numerics"]}
        strings += comp["strings"]
        blobs.append(entropy.pack_container(comp))
    return codec.pack_image_stream(header, blobs), strings


def _levels(n=3, H=330, W=530, **kw):
    built = [_level_stream(h, w, seed=l, **kw) for l, (h, w) in enumerate(P.shapes(H, W, n))]
    return [s for s, _ in built], [t for _, t in built]


def _join(streams, sizes=None, version=1, count=None, offsets=None, tail=b""):
    """A DSICP stream put together by hand, with whatever the directory is told to say"""
    sizes = sizes or [struct.unpack_from("<II", s, 12) for s in streams]
    off = 12 + 24 * len(streams)
    out = struct.pack("<6sHI", b"DSICP\0", version, len(streams) if count is None else count)
    for l, (s, (h, w)) in enumerate(zip(streams, sizes)):
        out += struct.pack("<IIQQ", h, w, off if offsets is None else offsets[l], len(s))
        off += len(s)
    return out + b"".join(streams) + tail


def test_pack_and_unpack_round_trip():
    streams, _ = _levels(3)
    pyr = codec.pack_pyramid_stream(streams)
    assert pyr == _join(streams)
    assert pyr[:6] == b"DSICP\0" and struct.unpack_from("<HI", pyr, 6) == (1, 4)
    u = codec.unpack_pyramid_stream(pyr)
    assert u["version"] == 1 and len(u["levels"]) == 4
    off = 12 + 24 * 4
    for lv, s, (h, w) in zip(u["levels"], streams, P.shapes(330, 530, 3)):
        assert (lv["H"], lv["W"], lv["offset"], lv["length"]) == (h, w, off, len(s))
        assert lv["stream"] == s == pyr[lv["offset"]:lv["offset"] + lv["length"]]
        off += len(s)
    assert off == len(pyr)
    assert codec.unpack_pyramid_stream(bytearray(pyr))["levels"][3]["stream"] == streams[3]
    assert codec.image_bpp(pyr) == 8.0 * len(pyr) / (330 * 530)
    assert codec.image_bpp(streams[0]) == 8.0 * len(streams[0]) / (330 * 530)
    two = codec.pack_pyramid_stream(streams[:2])
    assert len(codec.unpack_pyramid_stream(two)["levels"]) == 2 and len(two) == 60 + len(streams[0]) + len(streams[1])


def test_the_image_reader_keeps_refusing_a_pyramid_and_the_pyramid_reader_an_image():
    streams, _ = _levels(1)
    pyr = codec.pack_pyramid_stream(streams)
    with pytest.raises(ValueError, match="not a DSICI"):
        codec.unpack_image_stream(pyr)
    with pytest.raises(ValueError, match="not a DSICP"):
        codec.unpack_pyramid_stream(streams[0])
    with pytest.raises(ValueError):
        codec.unpack_pyramid_stream(b"DSI")


def test_pyramid_refusals():
    streams, _ = _levels(2)
    good = _join(streams)
    assert len(codec.unpack_pyramid_stream(good)["levels"]) == 3
    end = 12 + 24 * 3

    def refused(data, match):
        with pytest.raises(ValueError, match=match):
            codec.unpack_pyramid_stream(data)
        with pytest.raises(ValueError, match=match):                     # the readers of a level refuse alike
            codec.stream_index(data, level=0)
        with pytest.raises(ValueError, match=match):
            codec.stream_index(io.BytesIO(data), level=2)

    refused(_join(streams, version=2), "version 2")
    refused(_join(streams, version=0), "version 0")
    refused(_join(streams[:1], count=1), "at least two")
    refused(_join(streams, count=0), "at least two")
    for cut in (7, 12, 40, end - 1):                                      # inside the directory
        refused(good[:cut], "truncated")
    refused(good[:end + 10], "truncated")                                 # inside level 0
    refused(good[:-1], "truncated")                                       # inside the last level
    refused(_join(streams, offsets=[end + 1, end + 1 + len(streams[0]), end + 1 + len(streams[0]) + len(streams[1])],
                  tail=b"x"), "level 0 at offset")
    refused(_join(streams, offsets=[0, len(streams[0]), len(streams[0]) + len(streams[1])]), "level 0 at offset")
    refused(_join(streams, offsets=[end, end + len(streams[0]) + 1, end + len(streams[0]) + len(streams[1])]),
            "level 1 at offset")
    refused(_join(streams, offsets=[end, end, end]), "level 1 at offset")
    refused(good + b"\0", "1 trailing")
    refused(_join(streams, sizes=[(330, 530), (165, 266), (83, 133)]), "level 1 is 165x266")
    refused(_join(streams, sizes=[(330, 530), (165, 265), (82, 133)]), "level 2 is 82x133")
    # a chain of its own that level 0's head does not share: refused by whoever reads level 0
    forged = _join(streams, sizes=[(331, 530), (166, 265), (83, 133)])
    with pytest.raises(ValueError, match="level 0 as 331x530"):
        codec.unpack_pyramid_stream(forged)
    with pytest.raises(ValueError, match="level 0 as 331x530"):
        codec.stream_index(forged)


def test_a_level_whose_own_head_disagrees_with_the_directory():
    streams, _ = _levels(2)
    other, _ = _level_stream(166, 265, seed=1)                            # a sound stream of another height
    forged = _join([streams[0], other, streams[2]], sizes=P.shapes(330, 530, 2))
    with pytest.raises(ValueError, match="level 1 as 165x265, its own head says 166x265"):
        codec.unpack_pyramid_stream(forged)
    with pytest.raises(ValueError, match="its own head says 166x265"):
        codec.stream_index(forged, level=1)
    assert codec.stream_index(forged, level=2)["H"] == 83                 # a level is read alone
    with pytest.raises(ValueError, match="level 1 is 166x265"):
        codec.pack_pyramid_stream([streams[0], other, streams[2]])
    with pytest.raises(ValueError, match="at least two"):
        codec.pack_pyramid_stream(streams[:1])


@pytest.mark.parametrize("key,value", [("C", 4), ("kind", 1), ("N", 64), ("M", 320), ("in_ch", 4),
                                       ("spatial_params", 1), ("numerics", TAG + 1)])
def test_levels_that_disagree_with_each_other(key, value):
    streams, _ = _levels(2)
    odd, _ = _level_stream(165, 265, seed=1, **{key: value})
    assert codec.unpack_image_stream(odd)[key] == value
    with pytest.raises(ValueError, match=f"levels 0 and 1 disagree on {key}"):
        codec.pack_pyramid_stream([streams[0], odd, streams[2]])
    with pytest.raises(ValueError, match=f"levels 0 and 1 disagree on {key}"):
        codec.unpack_pyramid_stream(_join([streams[0], odd, streams[2]]))


class Counting:
    """A binary file object that records the reads made through it."""

    def __init__(self, data):
        self.f, self.reads = io.BytesIO(data), []

    def seek(self, *a):
        return self.f.seek(*a)

    def tell(self):
        return self.f.tell()

    def read(self, n=-1):
        pos = self.f.tell()
        out = self.f.read(n)
        self.reads.append((pos, len(out)))
        return out


@pytest.mark.parametrize("level", [None, 0, 1, 3])
def test_index_of_a_level_counts_from_the_start_of_the_pyramid(level):
    streams, strings = _levels(3)
    pyr = codec.pack_pyramid_stream(streams)
    l = level or 0
    directory = codec.unpack_pyramid_stream(pyr)["levels"]
    ix = codec.stream_index(pyr) if level is None else codec.stream_index(pyr, level=level)
    alone = codec.stream_index(streams[l])
    base = directory[l]["offset"]
    assert ix["level"] == l and ix["stream_bytes"] == len(pyr)
    assert ix["levels"] == [{k: d[k] for k in ("H", "W", "offset", "length")} for d in directory]
    for key in ("version", "H", "W", "C", "kind", "th", "tw", "batch", "batches", "segments", "overlap", "grid"):
        assert ix[key] == alone[key], key
    assert (ix["H"], ix["W"]) == P.shapes(330, 530, 3)[l]
    assert len(ix["tiles"]) == len(strings[l]) == alone["grid"]["n"]
    for r, ra, (z, y) in zip(ix["tiles"], alone["tiles"], strings[l]):
        assert pyr[r["z_off"]:r["z_off"] + r["z_len"]] == z and pyr[r["y_off"]:r["y_off"] + r["y_len"]] == y
        assert (r["z_off"], r["y_off"]) == (ra["z_off"] + base, ra["y_off"] + base)
    for c, ca in zip(ix["containers"], alone["containers"]):
        assert c["offset"] == ca["offset"] + base and c["bytes"] == ca["bytes"]
    every = list(range(len(ix["tiles"])))
    assert codec.tile_spans(ix, every) == [(o + base, n) for o, n in codec.tile_spans(alone, every)]
    # from a file object: only the directory and this level's heads
    f = Counting(pyr)
    assert codec.stream_index(f, level=level) == ix
    end = 12 + 24 * 4
    assert ix["index_bytes"] == sum(n for _, n in f.reads) == end + alone["index_bytes"]
    lo, hi = base, base + directory[l]["length"]
    for pos, n in f.reads:
        assert pos + n <= end or (lo <= pos and pos + n <= hi), (pos, n)


def test_levels_a_stream_does_not_hold():
    streams, _ = _levels(3)
    pyr = codec.pack_pyramid_stream(streams)
    for bad in (4, -1, 100):
        with pytest.raises(ValueError, match="levels 0 .. 3"):
            codec.stream_index(pyr, level=bad)
    with pytest.raises(ValueError, match="one image"):
        codec.stream_index(streams[0], level=1)
    with pytest.raises(ValueError):
        codec.stream_index(pyr, level=1.5)
    plain = codec.stream_index(streams[0])
    assert codec.stream_index(streams[0], level=0) == plain and "level" not in plain and "levels" not in plain


def test_the_new_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "dsic_hip.h")).read()
    declared = set(re.findall(r"\b(dsic_[a-zA-Z0-9_]+)\s*\(", header))
    new = {"dsic_image_halve_u8", "dsic_image_halve_f32"}
    assert new <= declared and new <= set(lib.SIGNATURES)
    for name in new:
        res, args = lib.SIGNATURES[name]
        assert len(args) == 6 and getattr(lib.load(), name) is not None


def test_the_halving_calls_check_their_arguments_without_a_gpu():
    import ctypes
    L = lib.load()
    buf = (ctypes.c_uint8 * 4096)()
    at = ctypes.addressof(buf)
    p = lambda off: ctypes.c_void_p(at + off)
    for fn, dims in ((L.dsic_image_halve_u8, lambda H, W, C: (H, W, C)), (L.dsic_image_halve_f32, lambda H, W, C: (C, H, W))):
        assert fn(None, p(0), *dims(4, 4, 3), None) == lib.DSIC_EINVAL and b"null" in L.dsic_last_error()
        assert fn(p(0), None, *dims(4, 4, 3), None) == lib.DSIC_EINVAL
        for H, W, C in ((0, 4, 3), (4, 0, 3), (4, 4, 0), (-1, 4, 3), (4, 4, -2)):
            assert fn(p(0), p(2048), *dims(H, W, C), None) == lib.DSIC_EINVAL
            assert b"at least 1" in L.dsic_last_error()
    # a 4 x 4 x 3 uint8 image is 48 bytes and halves to 12: dst inside src, and ending inside it
    assert L.dsic_image_halve_u8(p(0), p(40), 4, 4, 3, None) == lib.DSIC_EINVAL and b"overlap" in L.dsic_last_error()
    assert L.dsic_image_halve_u8(p(100), p(92), 4, 4, 3, None) == lib.DSIC_EINVAL
    assert L.dsic_image_halve_f32(p(0), p(188), 3, 4, 4, None) == lib.DSIC_EINVAL and b"overlap" in L.dsic_last_error()
    assert L.dsic_image_halve_f32(p(1024), p(1024), 3, 4, 4, None) == lib.DSIC_EINVAL


def test_compress_image_checks_every_level_before_it_touches_the_device():
    """the argument checks of the pyramid path that need no GPU: a model stub with the shape compress_image reads"""
    import torch

    class Stub(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.N, self.M = N, M
            self.g_a = torch.nn.Module()
            self.g_a.g_a = torch.nn.ModuleList([torch.nn.Conv2d(3, 4, 1)])

    model, img = Stub(), torch.zeros((330, 530, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="level 5"):
        codec.compress_image(model, img, tile=128, overviews=5)
    with pytest.raises(ValueError, match="overviews=-1"):
        codec.compress_image(model, img, tile=128, overviews=-1)
    # level 3 is 42 x 67, one tile of 48 x 80: an overlap of 32 is over half its side, as compress_image says of it alone
    with pytest.raises(ValueError, match=r"overlap=32.*overview level 3, 42x67"):
        codec.compress_image(model, img, tile=128, overlap=32, overviews=3)
    with pytest.raises(ValueError, match="overlap=32"):
        codec.compress_image(model, torch.zeros((42, 67, 3), dtype=torch.uint8), tile=128, overlap=32)
    with pytest.raises(RuntimeError, match="GPU"):
        codec.build_overviews(img, 2)
