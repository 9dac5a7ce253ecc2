"""CPU-only: the 16-bit image kind without a GPU.  The NumPy restatement (u16_ref.py) round-trips every value of six
scales, also with the normalised value one ulp off; the version-6 framing of codec.py (pack / unpack identity, the
index's offsets, every refusal of the readers, a pyramid whose levels disagree on the scale); compress_image's and the
decoders' argument refusals fire before any device call; and the new exports are declared, bound, and refuse bad
arguments."""
import ctypes
import io
import os
import random
import re
import struct

import numpy as np
import pytest
import torch

import u16_ref as R
from dsic_amd import codec, entropy, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAG = 0x40302
N, M = 128, 192
SCALES = [(0, 65535), (0, 10000), (1, 2), (123, 40000), (0, 1), (7, 7)]


# ---- the arithmetic ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lo,hi", SCALES)
def test_denorm_inverts_norm_on_every_value_of_the_scale(lo, hi):
    v = np.arange(lo, hi + 1, dtype=np.int64)
    x = R.norm(v, lo, hi)
    assert x.dtype == np.float32 and x.min() >= 0 and x.max() <= 1
    if hi > lo:                                                          # one correctly rounded float32 division
        want = (v - lo).astype(np.float32) / np.float32(hi - lo)
        assert x.tobytes() == want.tobytes() and x[0] == 0 and x[-1] == 1
        exact = (v - lo).astype(np.float64) / float(hi - lo)
        assert (np.abs(x.astype(np.float64) - exact) <= np.spacing(x) / 2).all()
    got = R.denorm(x, lo, hi)
    assert got.dtype == np.uint16 and np.array_equal(got, v)
    for side in (np.float32(-np.inf), np.float32(np.inf)):               # one ulp off either way
        assert np.array_equal(R.denorm(np.nextafter(x, side), lo, hi), v), side
    assert R.denorm(np.float32([2.0, 1.0, np.inf]), lo, hi).tolist() == [hi] * 3      # never above hi


def test_values_outside_the_scale_clip_and_an_empty_scale_is_zero():
    v = np.array([0, 99, 100, 101, 5000, 9999, 10000, 10001, 65535])
    x = R.norm(v, 100, 10000)
    assert x[:3].tolist() == [0, 0, 0] and x[-3:].tolist() == [1, 1, 1] and 0 < x[3] < x[4] < x[5] < 1
    assert R.denorm(x, 100, 10000).tolist() == [100, 100, 100, 101, 5000, 9999, 10000, 10000, 10000]
    z = R.norm(v, 7, 7)
    assert z.dtype == np.float32 and not z.any() and not np.signbit(z).any()
    assert R.denorm(z, 7, 7).tolist() == [7] * len(v)
    assert R.denorm(np.float32([0.3, 1.0, -1.0, np.nan]), 7, 7).tolist() == [7] * 4
    # rounds to nearest, where the uint8 kind truncates; -0.0, a NaN and anything below 0 give lo
    assert R.denorm(np.float32([0.49, 0.51, -0.0, np.nan, -3.0]), 10, 11).tolist() == [10, 11, 10, 10, 10]
    img = np.array([[[5, 300], [9, 100]]], dtype=np.uint16)             # [1][2][2]
    x = R.norm_image(img, [(5, 9), (0, 200)])
    assert x.shape == (2, 1, 2) and x.tolist() == [[[0.0, 1.0]], [[1.0, 0.5]]]
    assert R.denorm_image(x, [(5, 9), (0, 200)]).tolist() == [[[5, 200], [9, 100]]]
    assert R.band_range(img) == [(5, 9), (100, 300)]
    assert R.halve(np.array([[[1], [2], [65535]], [[4], [6], [65535]]], dtype=np.uint16)).tolist() == [[[3], [65535]]]


# ---- version-6 framing ------------------------------------------------------------------------------------------------
def _build(H=300, W=530, C=3, tile=128, batch=4, scale=((0, 10000), (5, 5), (123, 65535)), seed=0, **extra):
    """A version-6 stream in pure Python, with made-up strings."""
    rng = random.Random(seed)
    g = codec.tile_grid(H, W, tile, extra.get("overlap", 0))
    blobs, strings = [], []
    for first in range(0, g["n"], batch):
        B = min(batch, g["n"] - first)
        comp = {"strings": [], "shape_y": [B, M, g["th"] // 16, g["tw"] // 16],
                "shape_z": [B, N, g["th"] // 64, g["tw"] // 64], "min_y": [-3] * B, "max_y": [4] * B,
                "min_z": [-2] * B, "max_z": [2] * B, "numerics": TAG}
        for _ in range(B):
            strings.append([bytes(rng.getrandbits(8) for _ in range(rng.choice([0, 3, 17, 100]))),
                            bytes(rng.getrandbits(8) for _ in range(rng.choice([1, 16, 250])))])
            comp["strings"].append(strings[-1])
        blobs.append(entropy.pack_container(comp))
    header = {"numerics": TAG, "H": H, "W": W, "C": C, "kind": 2, "th": g["th"], "tw": g["tw"], "N": N, "M": M,
              "in_ch": C, "spatial_params": 0, "batch": batch, "scale": [tuple(p) for p in scale], **extra}
    return codec.pack_image_stream(header, blobs), header, blobs, strings


def test_pack_then_unpack_is_the_identity_and_the_index_finds_every_byte():
    stream, header, blobs, strings = _build()
    assert codec.KIND_U16_HWC == 2 and codec.VERSION_U16 == 6
    want = (struct.pack("<6sHI6I4I2I", b"DSICI\0", 6, TAG, 300, 530, 3, 2, 128, 128, N, M, 3, 0, 4, len(blobs))
            + struct.pack("<2I", 1, 0) + struct.pack("<6I", 0, 10000, 5, 5, 123, 65535)
            + b"".join(struct.pack("<Q", len(b)) + b for b in blobs))
    assert stream == want
    u = codec.unpack_image_stream(stream)
    assert u["version"] == 6 and u["kind"] == 2 and u["scale"] == [(0, 10000), (5, 5), (123, 65535)]
    assert u["segments"] == 1 and u["overlap"] == 0 and u["blobs"] == blobs and "max_error" not in u and "nodata" not in u
    assert codec.pack_image_stream(u, u["blobs"]) == stream
    assert codec.image_bpp(stream) == 8.0 * len(stream) / (300 * 530)
    ix = codec.stream_index(stream)
    assert ix["scale"] == u["scale"] and ix["grid"]["n"] == 15 == len(strings)
    for t, r in enumerate(ix["tiles"]):
        assert (r["k"], r["b"]) == divmod(t, 4)
        assert stream[r["z_off"]:r["z_off"] + r["z_len"]] == strings[t][0]
        assert stream[r["y_off"]:r["y_off"] + r["y_len"]] == strings[t][1]
    assert ix["containers"][0]["offset"] == 60 + 8 + 8 * 3 + 8
    assert codec._index_of(codec._Source(io.BytesIO(stream))) == ix
    assert ix["index_bytes"] == 60 + 8 + 8 * 3 + sum(8 + 38 + 24 * c["tiles"] for c in ix["containers"])
    assert ix["stream_bytes"] == len(stream)
    # overlap and segments ride in the same head; four bands make it 100 bytes
    s4, h4, b4, _ = _build(C=4, scale=[(0, 1)] * 4, overlap=16)
    u4 = codec.unpack_image_stream(s4)
    assert u4["overlap"] == 16 and u4["scale"] == [(0, 1)] * 4 and u4["version"] == 6
    assert codec.stream_index(s4)["containers"][0]["offset"] == 60 + 8 + 32 + 8
    assert codec.pack_image_stream(u4, u4["blobs"]) == s4
    # the other versions have no scale
    plain = dict(header, kind=0)
    del plain["scale"]
    p = codec.pack_image_stream(plain, blobs)
    assert codec.unpack_image_stream(p)["version"] == 1 and "scale" not in codec.stream_index(p)


def _patched(stream, at, fmt, *vals):
    b = bytearray(stream)
    struct.pack_into(fmt, b, at, *vals)
    return bytes(b)


def test_every_refusal_of_the_readers():
    stream, header, blobs, _ = _build()
    plain = dict(header, kind=0)
    del plain["scale"]
    v1 = codec.pack_image_stream(plain, blobs)
    v3 = codec.pack_image_stream(dict(plain, overlap=16), _build(overlap=16)[2])

    def refuses(s, match):
        for reader in (codec.stream_index, codec.unpack_image_stream):
            with pytest.raises(ValueError, match=match):
                reader(s)

    refuses(_patched(stream, 24, "<I", 0), "go together")                # version 6 with kind 0
    refuses(_patched(stream, 24, "<I", 1), "go together")
    refuses(_patched(v1, 24, "<I", 2), "go together")                    # kind 2 in version 1
    refuses(_patched(v3, 24, "<I", 2), "go together")                    # ... and in version 3
    with pytest.raises(ValueError, match="inconsistent"):                # a kind nobody knows, from _stream_grid
        codec.stream_index(_patched(v1, 24, "<I", 3))
    refuses(_patched(stream, 6, "<H", 7), "version 7")
    refuses(_patched(stream, 68, "<2I", 10001, 10000), "lo <= hi")       # band 0: lo > hi
    refuses(_patched(stream, 80, "<I", 65536), "65535")                  # band 1: hi > 65535
    refuses(_patched(stream, 84, "<2I", 70000, 70000), "65535")
    refuses(_patched(stream, 64, "<I", 8), "overlap")                    # not a multiple of 16
    refuses(_patched(stream, 64, "<I", 80), "overlap")                   # over half a tile
    refuses(_patched(stream, 60, "<I", 3), "segments")
    refuses(_patched(stream, 20, "<I", 5), "bands|inconsistent")         # C
    refuses(_patched(stream, 20, "<I", 0), "bands|inconsistent")
    with pytest.raises(ValueError, match="inconsistent|truncated|scale pair"):   # C = 4: a pair out of the first length
        codec.stream_index(_patched(stream, 20, "<I", 4))
    refuses(_patched(stream, 56, "<I", len(blobs) + 1), "batches|truncated")
    refuses(stream + b"\0", "trailing")
    for cut in (61, 66, 68, 70, 75, 91, 92, 95, len(stream) - 1):       # in the words, in the scale, in the lengths
        refuses(stream[:cut], "truncated")
    # the writer
    with pytest.raises(ValueError, match="kind 2"):
        codec.pack_image_stream(dict(header, kind=0), blobs)
    with pytest.raises(ValueError, match="kind 2"):
        codec.pack_image_stream(dict(header, scale=None), blobs)
    with pytest.raises(ValueError, match="max_error or nodata"):
        codec.pack_image_stream(dict(header, max_error=1), blobs, residuals=[b""] * len(blobs))
    with pytest.raises(ValueError, match="max_error or nodata"):
        codec.pack_image_stream(dict(header, nodata=0), blobs, mask=b"x")
    for bad in ([(0, 1)] * 2, [(2, 1), (0, 1), (0, 1)], [(0, 65536)] * 3, [(0.0, 1.0)] * 3, [(0, 1, 2)] * 3, 5,
                [(-1, 4)] * 3):
        with pytest.raises(ValueError, match="scale"):
            codec.pack_image_stream(dict(header, scale=bad), blobs)


def test_a_pyramid_whose_levels_disagree_on_the_scale_is_refused():
    s0, _, _, _ = _build(300, 530)
    s1, _, _, _ = _build(150, 265)
    other, _, _, _ = _build(150, 265, scale=((0, 10000), (5, 5), (123, 65534)))
    p = codec.pack_pyramid_stream([s0, s1])
    assert [lv["stream"] for lv in codec.unpack_pyramid_stream(p)["levels"]] == [s0, s1]
    assert codec.stream_index(p, level=1)["scale"] == codec.stream_index(p)["scale"] == [(0, 10000), (5, 5), (123, 65535)]
    with pytest.raises(ValueError, match="disagree on scale"):
        codec.pack_pyramid_stream([s0, other])
    at = p.index(s1) + 68 + 20                                          # hi of band 2 in level 1's head
    bad = _patched(p, at, "<I", 65534)
    with pytest.raises(ValueError, match="disagree on scale"):
        codec.unpack_pyramid_stream(bad)
    # a level read alone is read from the directory and its own head: each gives the scale it carries
    assert codec.stream_index(bad)["scale"][2] == (123, 65535) and codec.stream_index(bad, level=1)["scale"][2] == (123, 65534)
    plain = dict(codec.unpack_image_stream(s1), kind=0)                  # a uint8 level under a uint16 one
    blobs = plain.pop("blobs")
    del plain["scale"]
    with pytest.raises(ValueError, match="disagree on kind"):
        codec.pack_pyramid_stream([s0, codec.pack_image_stream(plain, blobs)])


# ---- compress_image's and the decoders' argument checks ---------------------------------------------------------------
class Stub(torch.nn.Module):
    def __init__(self, in_ch=3):
        super().__init__()
        self.N, self.M = N, M
        self.g_a = torch.nn.Module()
        self.g_a.g_a = torch.nn.ModuleList([torch.nn.Conv2d(in_ch, 4, 1)])


def test_compress_image_refuses_before_it_touches_the_device():
    model, img = Stub(), torch.zeros((330, 530, 3), dtype=torch.uint16)
    for bad in ([(0, 1)] * 2, [(0, 1)] * 4, [(2, 1), (0, 1), (0, 1)], [(0, 65536)] * 3, [(-1, 5)] * 3, [(0.0, 1.0)] * 3,
                [(0, 1, 2)] * 3, [0, 1, 2], 7, "abc"):
        with pytest.raises(ValueError, match="scale"):
            codec.compress_image(model, img, tile=128, scale=bad)
    for other in (torch.zeros((330, 530, 3), dtype=torch.uint8), torch.zeros((3, 330, 530))):
        with pytest.raises(ValueError, match="scale goes with a uint16"):
            codec.compress_image(model, other, tile=128, scale=[(0, 10000)] * 3)
    with pytest.raises(ValueError, match="max_error together with a uint16 image"):
        codec.compress_image(model, img, tile=128, max_error=2)
    with pytest.raises(ValueError, match="nodata together with a uint16 image"):
        codec.compress_image(model, img, tile=128, nodata=0)
    with pytest.raises(ValueError, match="1 to 4 bands"):
        codec.compress_image(Stub(5), torch.zeros((64, 64, 5), dtype=torch.uint16), tile=64)
    with pytest.raises(ValueError, match="4 channels, the model takes 3"):
        codec.compress_image(model, torch.zeros((64, 64, 4), dtype=torch.uint16), tile=64, scale=[(0, 1)] * 4)
    with pytest.raises(ValueError, match="overlap"):
        codec.compress_image(model, img, tile=128, overlap=8, scale=[(0, 1)] * 3)
    with pytest.raises(ValueError, match="level 5"):
        codec.compress_image(model, img, tile=128, overviews=5, scale=[(0, 1)] * 3)
    with pytest.raises(TypeError, match="uint8, uint16 or float32"):
        codec.compress_image(model, torch.zeros((330, 530, 3), dtype=torch.int16), tile=128)
    assert codec.check_scale([(np.uint16(3), np.int64(9))] * 2, 2, "x") == [(3, 9), (3, 9)]
    # no CPU fallback for the two device helpers
    with pytest.raises(RuntimeError, match="GPU"):
        codec.band_range(img)
    with pytest.raises(RuntimeError, match="GPU"):
        codec.build_overviews(img, 1)
    with pytest.raises(TypeError, match="uint16"):
        codec.band_range(torch.zeros((64, 64, 3), dtype=torch.uint8))


def test_out_u16_needs_a_stream_with_a_scale():
    stream, header, blobs, _ = _build()
    plain = dict(header, kind=0)
    del plain["scale"]
    for s in (codec.pack_image_stream(plain, blobs), codec.pack_image_stream(dict(plain, overlap=16), _build(overlap=16)[2])):
        with pytest.raises(ValueError, match="out='u16' needs the scale"):
            codec.decompress_image(Stub(), s, out="u16")
        with pytest.raises(ValueError, match="out='u16' needs the scale"):
            codec.decompress_region(Stub(), io.BytesIO(s), 0, 0, 8, 8, out="u16")
    with pytest.raises(ValueError, match="out='u32'"):
        codec.decompress_image(Stub(), stream, out="u32")


def test_the_command_line_reads_one_pair_or_one_per_band():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_dsic_image_tool", os.path.join(ROOT, "tools", "dsic_image.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert tool.scale_pairs("0,10000", 3) == [(0, 10000)] * 3 and tool.scale_pairs("5,9", 1) == [(5, 9)]
    assert tool.scale_pairs("0,10000,100,9500,0,65535", 3) == [(0, 10000), (100, 9500), (0, 65535)]
    assert tool.scale_pairs("1,2,3,4", 2) == [(1, 2), (3, 4)]
    for bad, C in (("0", 3), ("0,1,2", 3), ("0,1,2,3", 3), ("0,1,2,3,4,5,6,7", 3), ("a,b", 3), ("", 3), ("0,1.5", 3)):
        with pytest.raises(ValueError):
            tool.scale_pairs(bad, C)
    with pytest.raises(SystemExit):                                      # --scale is for compress
        tool.main(["decompress", "a.dsic", "b.npy", "--weights", "w.pt", "--scale", "0,1"])


# ---- the exports ------------------------------------------------------------------------------------------------------
NEW = {"dsic_band_range_u16": 6, "dsic_tile_gather_u16": 11, "dsic_tile_gather_u16_ov": 12,
       "dsic_tile_stitch_window_u16": 15, "dsic_tile_blend_finish_u16": 7, "dsic_image_halve_u16": 6}


def test_the_new_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "dsic_hip.h")).read()
    declared = set(re.findall(r"\b(dsic_[a-zA-Z0-9_]+)\s*\(", header))
    assert set(NEW) <= declared and set(NEW) <= set(lib.SIGNATURES)
    for name, nargs in NEW.items():
        res, args = lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs and getattr(lib.load(), name) is not None
    assert lib.load().dsic_abi_version() == 4


def _lohi(*pairs):
    flat = [v for p in pairs for v in p]
    return (ctypes.c_uint32 * 8)(*(flat + [0] * (8 - len(flat))))


def test_the_u16_calls_check_their_arguments_without_a_gpu():
    L = lib.load()
    one = 16   # any non-null, 16-byte aligned address: every call below is refused before a launch
    E = lib.DSIC_EINVAL
    ok = _lohi((0, 65535), (0, 10000), (7, 7), (1, 2))
    err = L.dsic_last_error
    big = 1 << 29                                                        # a row of 2^29 pixels of 4 uint16: 2^32 bytes

    assert L.dsic_band_range_u16(None, 64, 64, 3, one, None) == E and b"null" in err()
    assert L.dsic_band_range_u16(one, 64, 64, 3, None, None) == E and b"null" in err()
    assert L.dsic_band_range_u16(one, 64, 64, 0, one, None) == E and b"C=0" in err()
    assert L.dsic_band_range_u16(one, 64, 64, 5, one, None) == E and b"C=5" in err()
    assert L.dsic_band_range_u16(one + 1, 64, 64, 3, one, None) == E and b"2-byte aligned" in err()
    assert L.dsic_band_range_u16(one, 0, 64, 3, one, None) == E and b"empty" in err()
    assert L.dsic_band_range_u16(one, 64, -1, 3, one, None) == E
    assert L.dsic_band_range_u16(one, 1, big, 4, one, None) == E and b"2^31" in err()
    assert L.dsic_band_range_u16(one, 64, 64, 3, one + 2, None) == E and b"4-byte aligned" in err()

    for ov in (False, True):
        def gather(img=one, tiles=one, H=64, W=64, C=3, th=32, tw=32, O=16, lohi=ok, first=0, n=4):
            if ov:
                return L.dsic_tile_gather_u16_ov(img, tiles, H, W, C, th, tw, O, lohi, first, n, None)
            return L.dsic_tile_gather_u16(img, tiles, H, W, C, th, tw, lohi, first, n, None)
        assert gather(img=None) == E and b"null" in err()
        assert gather(tiles=None) == E and b"null" in err()
        assert gather(lohi=None) == E and b"null" in err()
        assert gather(C=0) == E and gather(C=5) == E and b"C=5" in err()
        assert gather(img=one + 1) == E and b"2-byte aligned" in err()
        assert gather(lohi=_lohi((5, 4))) == E and b"lo must not exceed hi" in err()
        assert gather(lohi=_lohi((0, 1), (0, 65536))) == E and b"65535" in err()
        assert gather(lohi=_lohi((0, 1), (0, 1), (70000, 70000))) == E
        assert gather(H=0) == E and b"empty" in err()
        assert gather(th=24) == E and gather(tw=80) == E and gather(H=17, th=32) == E
        assert gather(first=2, n=8) == E and b"outside the grid" in err()
        assert gather(n=0) == E and gather(first=-1) == E
        assert gather(tiles=one + 4) == E and b"16-byte aligned" in err()
        assert gather(H=64, W=big, C=4, n=1) == E and b"2^31" in err()
        if ov:
            assert gather(O=8) == E and b"overlap" in err()
            assert gather(O=32) == E and gather(O=-16) == E

    def stitch(tiles=one, ids=one, n=1, out=one, H=64, W=64, C=3, th=32, tw=32, win=(0, 0, 64, 64), lohi=ok):
        return L.dsic_tile_stitch_window_u16(tiles, ids, n, out, H, W, C, th, tw, *win, lohi, None)
    assert stitch(tiles=None) == E and b"null" in err()
    assert stitch(ids=None) == E and stitch(out=None) == E and stitch(lohi=None) == E and b"null" in err()
    assert stitch(C=0) == E and stitch(C=5) == E and b"C=5" in err()
    assert stitch(out=one + 1) == E and b"2-byte aligned" in err()
    assert stitch(lohi=_lohi((0, 1), (3, 2))) == E and b"lo must not exceed hi" in err()
    assert stitch(lohi=_lohi((0, 1 << 16))) == E and b"65535" in err()
    assert stitch(th=24) == E and stitch(H=0) == E and stitch(tw=96) == E
    assert stitch(win=(0, 1, 64, 64)) == E and b"window" in err()
    assert stitch(win=(0, 0, 0, 64)) == E and stitch(win=(-1, 0, 8, 8)) == E
    assert stitch(n=0) == E and stitch(n=70000) == E
    assert stitch(W=big, C=4, win=(0, 0, 1, big)) == E and b"2^31" in err()

    def finish(canvas=one, out=one, C=3, h=8, w=8, lohi=ok):
        return L.dsic_tile_blend_finish_u16(canvas, out, C, h, w, lohi, None)
    assert finish(canvas=None) == E and finish(out=None) == E and finish(lohi=None) == E and b"null" in err()
    assert finish(C=0) == E and finish(C=5) == E and b"C=5" in err()
    assert finish(out=one + 3) == E and b"2-byte aligned" in err()
    assert finish(lohi=_lohi((2, 1))) == E and finish(lohi=_lohi((0, 65536))) == E and b"65535" in err()
    assert finish(h=0) == E and finish(w=0) == E and b"empty" in err()
    assert finish(C=4, h=1, w=big) == E and b"2^31" in err()

    assert L.dsic_image_halve_u16(None, one, 4, 4, 3, None) == E and b"null" in err()
    assert L.dsic_image_halve_u16(one, None, 4, 4, 3, None) == E
    assert L.dsic_image_halve_u16(one, 4096, 4, 4, 0, None) == E and L.dsic_image_halve_u16(one, 4096, 4, 4, 5, None) == E
    assert L.dsic_image_halve_u16(one + 1, 4096, 4, 4, 3, None) == E and b"2-byte aligned" in err()
    assert L.dsic_image_halve_u16(one, 4097, 4, 4, 3, None) == E and b"2-byte aligned" in err()
    assert L.dsic_image_halve_u16(one, 4096, 0, 4, 3, None) == E and L.dsic_image_halve_u16(one, 4096, 4, 0, 3, None) == E
    assert L.dsic_image_halve_u16(one, 1 << 40, 1, big, 4, None) == E and b"2^31" in err()
    assert L.dsic_image_halve_u16(one, one + 94, 4, 4, 3, None) == E and b"overlap" in err()   # src is 96 bytes
    assert L.dsic_image_halve_u16(one + 22, one, 4, 4, 3, None) == E and b"overlap" in err()   # dst is 24 bytes
