"""CPU-only: validity masks without a GPU.  The version-8 framing of codec.py (pack / unpack identity for both kinds,
literal head offsets, the index's offsets, every refusal of the readers); compress_image's new argument refusals fire
before any device call and the old ones still do; the NumPy restatement (valid_ref.py) is anchored to the restatements
it generalises (pyramid_ref, u16_ref, view_ref, mask_ref); and the new exports are declared, bound, and refuse bad
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

import mask_ref
import pyramid_ref
import u16_ref
import valid_ref as R
import view_ref
from dsic_amd import codec, entropy, lib
from dsic_amd import mask as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAG = 0x40302
N, M = 128, 192


# ---- version-8 framing ------------------------------------------------------------------------------------------------
def _valid(H=300, W=530, seed=3):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W]
    valid = ~(2 * yy + xx < 500)
    valid[200:260, 400:460] &= rng.random((60, 60)) < 0.5
    return valid


def _build(valid, kind, C, tile, batch, fill, scale=None, segments=1, seed=0):
    """A version-8 stream in pure Python: the restatement's mask block, made-up strings for the coded tiles."""
    rng = random.Random(seed)
    H, W = valid.shape
    g = codec.tile_grid(H, W, tile)
    block, st = R.block(valid, fill, g["th"], g["tw"])
    ids = [t for t, s in enumerate(st) if s]
    blobs, strings = [], {}
    for first in range(0, len(ids), batch):
        sel = ids[first:first + batch]
        B = len(sel)
        comp = {"strings": [], "shape_y": [B, M, g["th"] // 16, g["tw"] // 16],
                "shape_z": [B, N, g["th"] // 64, g["tw"] // 64], "min_y": [-3] * B, "max_y": [4] * B,
                "min_z": [-2] * B, "max_z": [2] * B, "numerics": TAG}
        if segments > 1:
            comp.update(segments=segments, seg_lengths_y=[])
        for t in sel:
            y = [bytes(rng.getrandbits(8) for _ in range(rng.choice([1, 16, 250]))) for _ in range(segments)]
            strings[t] = [bytes(rng.getrandbits(8) for _ in range(rng.choice([0, 3, 17, 100]))), b"".join(y)]
            comp["strings"].append(strings[t])
            if segments > 1:
                comp["seg_lengths_y"].append([len(v) for v in y])
        blobs.append(entropy.pack_container(comp))
    header = {"numerics": TAG, "H": H, "W": W, "C": C, "kind": kind, "th": g["th"], "tw": g["tw"], "N": N, "M": M,
              "in_ch": C, "spatial_params": 0, "batch": batch, "fill": fill, "segments": segments}
    if scale is not None:
        header["scale"] = [tuple(p) for p in scale]
    return codec.pack_image_stream(header, blobs, mask=block), header, blobs, block, st, strings


SCALE4 = ((0, 10000), (5, 5), (123, 65535), (7, 9))


@pytest.mark.parametrize("kind,C,fill,scale", [(0, 3, 255, None), (2, 4, 65535, SCALE4)])
def test_pack_then_unpack_is_the_identity_and_the_index_finds_every_byte(kind, C, fill, scale):
    valid = _valid()
    stream, header, blobs, block, st, strings = _build(valid, kind, C, 128, 4, fill, scale)
    assert codec.VERSION_VALID == 8 and set(st) == {0, 1, 2}
    coded = sum(1 for s in st if s)
    # the head, byte by byte: 60 bytes of version 1, segments, overlap 0, fill, coded, the scale, the block's length
    want = struct.pack("<6sHI6I4I2I", b"DSICI\0", 8, TAG, 300, 530, C, kind, 128, 128, N, M, C, 0, 4, len(blobs))
    want += struct.pack("<4I", 1, 0, fill, coded)
    if scale:
        want += struct.pack("<8I", *[v for p in scale for v in p])
    mo = 76 + (8 * C if scale else 0) + 8
    assert stream[:mo] == want + struct.pack("<Q", len(block))
    assert stream[:mo - 8] == R.head(8, TAG, 300, 530, C, kind, 128, 128, N, M, C, 0, 4, len(blobs), 1, fill, coded, scale)
    assert stream == stream[:mo] + block + b"".join(struct.pack("<Q", len(b)) + b for b in blobs)
    assert struct.unpack_from("<I", stream, 68) == (fill,) and struct.unpack_from("<I", stream, 72) == (coded,)
    assert struct.unpack_from("<I", block, 18) == (fill,)               # the block's nodata field carries fill
    u = codec.unpack_image_stream(stream)
    assert u["version"] == 8 and u["fill"] == fill and u["coded"] == coded and u["overlap"] == 0 and "nodata" not in u
    assert u["blobs"] == blobs and u["mask"] == block and u["batches"] == len(blobs) == -(-coded // 4)
    assert (u["mask_offset"], u["mask_bytes"]) == (mo, len(block))
    assert u.get("scale") == (None if scale is None else [tuple(p) for p in scale])
    assert codec.pack_image_stream(u, u["blobs"], mask=u["mask"]) == stream
    ix = codec.stream_index(stream)
    assert "nodata" not in ix
    for key in ("fill", "coded", "mask_offset", "mask_bytes"):
        assert ix[key] == u[key]
    _, _, _, _, _, payloads = mask_ref.parse_block(block)
    ids = [t for t, s in enumerate(st) if s]
    assert [c["ids"] for c in ix["containers"]] == [ids[i:i + 4] for i in range(0, len(ids), 4)]
    modes = set()
    for t, r in enumerate(ix["tiles"]):
        assert r["state"] == st[t]
        if st[t] == 0:
            assert r["k"] is None and r["b"] is None and r["z_len"] == r["y_len"] == 0 and "m_off" not in r
            continue
        assert (r["k"], r["b"]) == divmod(ids.index(t), 4)
        assert stream[r["z_off"]:r["z_off"] + r["z_len"]] == strings[t][0]
        assert stream[r["y_off"]:r["y_off"] + r["y_len"]] == strings[t][1]
        if st[t] == 2:
            assert (r["m_mode"], stream[r["m_off"]:r["m_off"] + r["m_len"]]) == payloads[t]
            modes.add(r["m_mode"])
        else:
            assert "m_off" not in r
    assert modes == {0, 1}
    every = list(range(len(st)))
    want_bytes = sum(len(a) + len(b) for a, b in strings.values()) + sum(len(p) for _, p in payloads.values())
    assert sum(n for _, n in codec.tile_spans(ix, every)) == want_bytes
    assert codec._coded_tiles(ix, every) == ids and codec.window_tiles(ix, 0, 0, 300, 530) == every
    assert codec._index_of(codec._Source(io.BytesIO(stream))) == ix
    assert ix["index_bytes"] == mo + 26 + K.states_bytes(len(st)) + 12 * len(payloads) + sum(
        8 + 38 + 24 * len(c["ids"]) for c in ix["containers"])


def test_segments_and_zero_coded_tiles():
    valid = _valid()
    stream, header, blobs, block, st, strings = _build(valid, 0, 3, 128, 4, 9, segments=4)
    u = codec.unpack_image_stream(stream)
    assert u["segments"] == 4 and u["version"] == 8 and struct.unpack_from("<I", stream, 60) == (4,)
    ix = codec.stream_index(stream)
    for t, r in enumerate(ix["tiles"]):
        if st[t]:
            assert len(r["y_segs"]) == 4 and stream[r["y_off"]:r["y_off"] + r["y_len"]] == strings[t][1]
    assert codec.pack_image_stream(u, u["blobs"], mask=u["mask"]) == stream
    for kind, C, fill, scale in ((0, 3, 0, None), (2, 2, 40000, ((1, 2), (0, 0)))):
        none = np.zeros((100, 90), bool)
        stream, *_, st, _ = _build(none, kind, C, 64, 4, fill, scale)
        assert set(st) == {0}
        u = codec.unpack_image_stream(stream)
        assert u["batches"] == 0 and u["coded"] == 0 and u["blobs"] == [] and u["fill"] == fill
        ix = codec.stream_index(stream)
        assert ix["containers"] == [] and all(r["state"] == 0 and r["k"] is None for r in ix["tiles"])
        assert codec.tile_spans(ix, list(range(len(st)))) == []
        stream, *_, st, _ = _build(~none, kind, C, 64, 4, fill, scale)
        assert set(st) == {1} and codec.unpack_image_stream(stream)["coded"] == len(st)


def _patched(stream, at, fmt, *vals):
    b = bytearray(stream)
    struct.pack_into(fmt, b, at, *vals)
    return bytes(b)


def test_every_refusal_of_the_readers():
    valid = _valid()
    s8, header, blobs, block, st, _ = _build(valid, 0, 3, 128, 4, 7)
    s16, h16, b16, _, _, _ = _build(valid, 2, 4, 128, 4, 7, SCALE4)
    ix = codec.stream_index(s8)
    full = st.index(1)

    def refuses(s, match):
        for reader in (codec.stream_index, codec.unpack_image_stream):
            with pytest.raises(ValueError, match=match):
                reader(s)

    refuses(_patched(s8, 6, "<H", 7), "version 7")                       # still unassigned
    refuses(_patched(s8, 24, "<I", 1), "version 8 with kind 1")
    refuses(_patched(_patched(s8, 6, "<H", 5), 24, "<I", 2), "go together")   # kind 2 stays out of version 5
    refuses(_patched(s8, 6, "<H", 6), "go together")                     # ... and version 6 is kind 2 alone
    refuses(_patched(s8, 64, "<I", 16), "overlap=16")
    refuses(_patched(s8, 68, "<I", 256), "fill=256")                     # beyond uint8
    refuses(_patched(s16, 68, "<I", 65536), "fill=65536")
    codec.stream_index(_patched(_patched(s16, 68, "<I", 256), 76 + 32 + 8 + 18, "<I", 256))   # fine for uint16
    refuses(_patched(s16, 76, "<2I", 10001, 10000), "lo <= hi")          # band 0: lo > hi
    refuses(_patched(s16, 76 + 12, "<I", 65536), "65535")                # band 1: hi > 65535
    with pytest.raises(ValueError, match="batches|coded"):
        codec.stream_index(_patched(s8, 72, "<I", ix["coded"] + 1))      # coded in the head against the states
    with pytest.raises(ValueError, match="coded tiles"):
        codec.stream_index(_patched(s8, 84 + 26 + full, "<B", 0))        # a state against coded
    with pytest.raises(ValueError, match="head says"):
        codec.stream_index(_patched(s8, 84 + 18, "<I", 8))               # the block's fill against the head's
    refuses(_patched(s8, 60, "<I", 3), "segments")
    refuses(_patched(s8, 56, "<I", len(blobs) + 1), "batches|truncated")
    refuses(s8 + b"\0", "trailing")
    refuses(s16 + b"\0", "trailing")
    for cut in (61, 70, 75, 80, 84 + 10, len(s8) - 1):
        refuses(s8[:cut], "truncated")
    for cut in (76 + 5, 76 + 31, 76 + 32 + 4, len(s16) - 1):
        refuses(s16[:cut], "truncated")
    # the writer
    with pytest.raises(ValueError, match="kind 0 or 2"):
        codec.pack_image_stream(dict(header, kind=1), blobs, mask=block)
    with pytest.raises(ValueError, match="fill="):
        codec.pack_image_stream(dict(header, fill=256), blobs, mask=block)
    with pytest.raises(ValueError, match="fill="):
        codec.pack_image_stream(dict(h16, fill=65536), b16, mask=block)
    with pytest.raises(ValueError, match="kind 2"):
        codec.pack_image_stream(dict(header, scale=[(0, 1)] * 3), blobs, mask=block)
    with pytest.raises(ValueError, match="kind 2"):
        codec.pack_image_stream(dict(h16, scale=None), b16, mask=block)
    with pytest.raises(ValueError, match="needs the mask block"):
        codec.pack_image_stream(header, blobs)
    with pytest.raises(ValueError, match="containers for"):
        codec.pack_image_stream(header, blobs[:-1], mask=block)
    with pytest.raises(ValueError, match="coded"):
        codec.pack_image_stream(dict(header, coded=ix["coded"] - 1), blobs, mask=block)
    for extra in ({"overlap": 16}, {"max_error": 1}, {"nodata": 0}):
        with pytest.raises(ValueError, match="overlap|max_error|nodata"):
            codec.pack_image_stream(dict(header, **extra), blobs, mask=block)
    with pytest.raises(ValueError, match="head says"):
        codec.pack_image_stream(dict(header, fill=8), blobs, mask=block)  # the block was made for fill 7


def test_a_pyramid_of_masked_levels_must_agree_on_fill():
    levels, masks = R.chain(np.zeros((300, 530, 3), np.uint8), _valid(), 1)
    s0 = _build(masks[0], 0, 3, 128, 4, 7)[0]
    s1 = _build(masks[1], 0, 3, 128, 4, 7)[0]
    p = codec.pack_pyramid_stream([s0, s1])
    assert "fill" in codec._SAME_IN_LEVELS
    assert codec.stream_index(p, level=1)["fill"] == 7 and codec.stream_index(p, level=1)["version"] == 8
    with pytest.raises(ValueError, match="disagree on fill"):
        codec.pack_pyramid_stream([s0, _build(masks[1], 0, 3, 128, 4, 8)[0]])


# ---- compress_image's argument checks ---------------------------------------------------------------------------------
class Stub(torch.nn.Module):
    def __init__(self, in_ch=3):
        super().__init__()
        self.N, self.M = N, M
        self.g_a = torch.nn.Module()
        self.g_a.g_a = torch.nn.ModuleList([torch.nn.Conv2d(in_ch, 4, 1)])


def test_compress_image_refuses_before_it_touches_the_device():
    model = Stub()
    u8, u16 = torch.zeros((330, 530, 3), dtype=torch.uint8), torch.zeros((330, 530, 3), dtype=torch.uint16)
    ok = torch.ones((330, 530), dtype=torch.bool)
    with pytest.raises(ValueError, match="float32"):
        codec.compress_image(model, torch.zeros((3, 330, 530)), tile=128, valid=ok)
    for img in (u8, u16):
        with pytest.raises(ValueError, match="valid together with overlap"):
            codec.compress_image(model, img, tile=128, valid=ok, overlap=16)
        with pytest.raises(ValueError, match="valid together with max_error"):
            codec.compress_image(model, img, tile=128, valid=ok, max_error=1)
        with pytest.raises(ValueError, match="valid together with nodata"):
            codec.compress_image(model, img, tile=128, valid=ok, nodata=0)
        for bad in (torch.ones((330, 529), dtype=torch.bool), torch.ones((530, 330), dtype=torch.bool),
                    torch.ones((330, 530, 1), dtype=torch.bool), torch.ones((330, 530), dtype=torch.uint8),
                    torch.ones((330, 530)), np.ones((330, 530), bool), 1):
            with pytest.raises(ValueError, match="valid must be"):
                codec.compress_image(model, img, tile=128, valid=bad)
        for bad in (-1, 1.0, "0", True, 65536):
            with pytest.raises(ValueError, match="fill="):
                codec.compress_image(model, img, tile=128, valid=ok, fill=bad)
        with pytest.raises(ValueError, match="fill=.*goes with valid"):
            codec.compress_image(model, img, tile=128, fill=3)
    with pytest.raises(ValueError, match="fill=256"):
        codec.compress_image(model, u8, tile=128, valid=ok, fill=256)
    # the refusals of nodata stand as they were
    with pytest.raises(ValueError, match="nodata together with a uint16 image"):
        codec.compress_image(model, u16, tile=128, nodata=0)
    with pytest.raises(ValueError, match="nodata together with overviews"):
        codec.compress_image(model, u8, tile=128, nodata=0, overviews=1)
    with pytest.raises(ValueError, match="nodata="):
        codec.compress_image(model, u8, tile=128, nodata=256)
    assert K.check_fill(np.uint16(65535), 65535, "x") == 65535 and K.check_fill(0, 255, "x") == 0


# ---- the restatement against the restatements it generalises ----------------------------------------------------------
HALVE_SIZES = [(1, 1), (1, 7), (33, 65), (300, 280)]


@pytest.mark.parametrize("H,W", HALVE_SIZES)
def test_masked_halving_with_all_or_none_valid_is_the_plain_halving(H, W):
    rng = np.random.default_rng(H * 1000 + W)
    for dtype, C, plain in ((np.uint8, 3, pyramid_ref.halve_u8), (np.uint16, 4, u16_ref.halve)):
        img = rng.integers(0, np.iinfo(dtype).max + 1, size=(H, W, C)).astype(dtype)
        img[:: 3, :: 2] = np.iinfo(dtype).max
        got, m = R.halve(img, np.ones((H, W), bool))
        assert got.dtype == dtype and np.array_equal(got, plain(img)) and m.all() and m.shape == got.shape[:2]
        got, m = R.halve(img, np.zeros((H, W), bool))
        assert np.array_equal(got, plain(img)) and not m.any()


def test_masked_halving_by_hand():
    img = np.array([[[10], [20], [31]], [[40], [50], [61]], [[7], [9], [200]]], dtype=np.uint8)       # 3 x 3 x 1
    for y, x in ((0, 0), (0, 1), (1, 0), (1, 1)):                        # a single valid tap gives that tap's value
        valid = np.zeros((3, 3), bool)
        valid[y, x] = True
        got, m = R.halve(img, valid)
        assert got[0, 0, 0] == img[y, x, 0] and m.tolist() == [[True, False], [False, False]]
    valid = np.array([[1, 1, 0], [0, 1, 1], [0, 0, 1]], bool)
    got, m = R.halve(img, valid)
    assert m.tolist() == [[True, True], [False, True]]
    # k = 3: 80 / 3 rounds to 27; k = 2 of a repeated column; k = 0: the unmasked (7 + 9 + 7 + 9 + 2) >> 2; k = 4
    assert got[:, :, 0].tolist() == [[27, 61], [8, 200]]
    img16 = np.array([[[65535], [65534]], [[0], [3]]], dtype=np.uint16)
    got, m = R.halve(img16, np.array([[1, 1], [0, 0]], bool))
    assert got.tolist() == [[[65535]]] and m.all()                       # (2 * 131069 + 2) // 4: half rounds up


@pytest.mark.parametrize("src_size,out_size", view_ref.SIZES)
def test_masked_resample_with_an_all_valid_window_is_the_plain_resample(src_size, out_size):
    for shift in view_ref.SHIFTS:
        case = view_ref.kernel_case(src_size, out_size, shift)
        for kind, C in (("u8", 3), ("u16", 2)):
            src = view_ref.kernel_image(kind, C, case["sh"], case["sw"])
            ones = np.ones((case["sh"], case["sw"]), bool)
            for mode in ("average", "nearest"):
                want = view_ref.resample(src, case["sy0"], case["sx0"], shift, case["region"], out_size, mode)
                got, oval = R.resample(src, ones, case["sy0"], case["sx0"], shift, case["region"], out_size, mode, 9)
                assert got.dtype == src.dtype and np.array_equal(got, want) and oval.all()
            # the mask "all channels equal v" and fill v give view_ref's nodata resample
            v = view_ref.NODATA[kind]
            sval = ~(src == v).all(axis=2)
            want = view_ref.resample(src, case["sy0"], case["sx0"], shift, case["region"], out_size, "average", nodata=v)
            got, oval = R.resample(src, sval, case["sy0"], case["sx0"], shift, case["region"], out_size, "average", v)
            assert np.array_equal(got, want)
            if not sval.any():
                assert not oval.any() and (got == v).all()


def test_a_mask_derived_from_a_value_gives_the_nodata_block():
    rng = np.random.default_rng(11)
    for H, W, tile, v in ((40, 70, 32, 0), (300, 280, 272, 7), (330, 530, 128, 255)):
        img = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
        yy, xx = np.mgrid[:H, :W]
        img[2 * yy + xx < (2 * H + W) // 2] = v
        img[H // 2:, W // 2:][rng.random((H - H // 2, W - W // 2)) < 0.3] = v
        th, tw = min(tile, mask_ref.ceil16(H)), min(tile, mask_ref.ceil16(W))
        valid = ~mask_ref.nodata_mask(img, v)
        assert R.block(valid, v, th, tw) == mask_ref.block(img, v, th, tw)
        assert R.counts(valid, th, tw) == mask_ref.counts(~valid, H, W, th, tw)
        grid = mask_ref.tiles(H, W, th, tw)
        desc = [(t, t) for t in range(len(grid))] + [(len(grid), 0), (0, -1)]
        planes = R.m_planes(valid, th, tw)
        win = (H // 3, W // 4, H // 2 + 1, W // 2 + 3)
        pre = rng.integers(0, 256, size=(win[2], win[3], 3), dtype=np.uint8)
        assert np.array_equal(R.apply(pre, win, H, W, th, tw, desc, planes, v),
                              mask_ref.apply(pre, win, H, W, th, tw, desc, planes, v))
        got = R.window_valid(np.full(win[2:], 9, np.uint8), win, H, W, th, tw, [(t, t) for t in range(1, len(grid))],
                             planes)
        want = valid[win[0]:win[0] + win[2], win[1]:win[1] + win[3]].astype(np.uint8)
        oy, ox, y0, y1, x0, x1 = grid[0]                                  # tile 0 is not listed: the pre-fill stays
        own0 = np.zeros((H, W), bool)
        own0[y0:y1, x0:x1] = True
        own0 = own0[win[0]:win[0] + win[2], win[1]:win[1] + win[3]]
        assert np.array_equal(got[~own0], want[~own0]) and (got[own0] == 9).all()
    img16 = rng.integers(0, 65536, size=(9, 11, 2)).astype(np.uint16)
    valid = rng.random((9, 11)) < 0.5
    valid[0, 0], valid[8, 10] = True, True
    img16[0, 0], img16[8, 10] = (0, 65535), (65535, 0)
    assert R.band_range(img16, valid) == [(0, 65535), (0, 65535)]
    assert R.band_range(img16, np.zeros((9, 11), bool)) == [(0, 0), (0, 0)]
    assert R.band_range(img16, np.ones((9, 11), bool)) == u16_ref.band_range(img16)


# ---- the exports ------------------------------------------------------------------------------------------------------
NEW = {"dsic_valid_classify": 9, "dsic_valid_delta_planes": 10, "dsic_mask_apply_u16": 16, "dsic_mask_window_u8": 14,
       "dsic_image_halve_valid_u8": 8, "dsic_image_halve_valid_u16": 8, "dsic_band_range_valid_u16": 7,
       "dsic_window_resample_valid_u8": 19, "dsic_window_resample_valid_u16": 19}


def test_the_new_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "dsic_hip.h")).read()
    declared = set(re.findall(r"\b(dsic_[a-zA-Z0-9_]+)\s*\(", header))
    assert set(NEW) <= declared and set(NEW) <= set(lib.SIGNATURES)
    for name, nargs in NEW.items():
        res, args = lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs and getattr(lib.load(), name) is not None
        decl = re.search(name + r"\s*\(([^;]*)\);", header).group(1)
        assert decl.count(",") + 1 == nargs, name


def test_the_new_calls_check_their_arguments_without_a_gpu():
    L = lib.load()
    one, far = 16, 1 << 20   # non-null, 16-byte aligned addresses far apart: every call below is refused before a launch
    E = lib.DSIC_EINVAL
    # classify
    assert L.dsic_valid_classify(None, 64, 64, 32, 32, 0, 4, one, None) == E and b"null" in L.dsic_last_error()
    assert L.dsic_valid_classify(one, 64, 64, 32, 32, 0, 4, None, None) == E
    assert L.dsic_valid_classify(one, 64, 64, 24, 32, 0, 4, one, None) == E                          # the grid
    assert L.dsic_valid_classify(one, 64, 64, 80, 32, 0, 1, one, None) == E
    assert L.dsic_valid_classify(one, 0, 64, 32, 32, 0, 1, one, None) == E
    assert L.dsic_valid_classify(one, 64, 64, 32, 32, 2, 3, one, None) == E and b"outside the grid" in L.dsic_last_error()
    assert L.dsic_valid_classify(one, 16384, 16384, 32, 32, 0, 70000, one, None) == E and b"65535" in L.dsic_last_error()
    assert L.dsic_valid_classify(one, 64, 64, 32, 32, 0, 4, one + 2, None) == E and b"aligned" in L.dsic_last_error()
    # delta planes
    d = (one, 64, 64, 32, 32)
    assert L.dsic_valid_delta_planes(None, 64, 64, 32, 32, one, 1, one, one, None) == E and b"null" in L.dsic_last_error()
    assert L.dsic_valid_delta_planes(*d, None, 1, one, one, None) == E
    assert L.dsic_valid_delta_planes(*d, one, 1, None, one, None) == E
    assert L.dsic_valid_delta_planes(*d, one, 1, one, None, None) == E
    assert L.dsic_valid_delta_planes(*d, one, 0, one, one, None) == E
    assert L.dsic_valid_delta_planes(*d, one, 70000, one, one, None) == E and b"65535" in L.dsic_last_error()
    assert L.dsic_valid_delta_planes(*d, one, 1, one + 2, one, None) == E and b"aligned" in L.dsic_last_error()
    assert L.dsic_valid_delta_planes(one, 64, 64, 32, 40, one, 1, one, one, None) == E
    # apply_u16 and window_u8
    ok = (64, 64, 3, 32, 32, 0, 0, 64, 64)
    fn = L.dsic_mask_apply_u16
    assert fn(one, 1, None, 1, 0, one, *ok, None) == E and b"null" in L.dsic_last_error()
    assert fn(one, 1, one, 1, 0, None, *ok, None) == E
    assert fn(None, 1, one, 1, 0, one, *ok, None) == E and b"planes" in L.dsic_last_error()
    assert fn(one, -1, one, 1, 0, one, *ok, None) == E
    assert fn(one, 1, one, 0, 0, one, *ok, None) == E
    assert fn(one, 1, one, 70000, 0, one, *ok, None) == E and b"65535" in L.dsic_last_error()
    assert fn(one, 1, one, 1, 65536, one, *ok, None) == E and b"fill" in L.dsic_last_error()
    assert fn(one, 1, one, 1, -1, one, *ok, None) == E
    assert fn(one, 1, one, 1, 0, one + 1, *ok, None) == E and b"aligned" in L.dsic_last_error()
    assert fn(one + 2, 1, one, 1, 0, one, *ok, None) == E and b"aligned" in L.dsic_last_error()
    assert fn(one, 1, one, 1, 0, one, 64, 64, 3, 32, 32, 0, 1, 64, 64, None) == E and b"window" in L.dsic_last_error()
    assert fn(one, 1, one, 1, 0, one, 64, 64, 3, 32, 24, 0, 0, 64, 64, None) == E
    assert fn(one, 1, one, 1, 0, one, 64, 64, 5, 32, 32, 0, 0, 64, 64, None) == E and b"C=" in L.dsic_last_error()
    assert fn(one, 1, one, 1, 0, one, 64, 64, 0, 32, 32, 0, 0, 64, 64, None) == E
    okw = (64, 64, 32, 32, 0, 0, 64, 64)
    fn = L.dsic_mask_window_u8
    assert fn(one, 1, None, 1, one, *okw, None) == E and b"null" in L.dsic_last_error()
    assert fn(one, 1, one, 1, None, *okw, None) == E
    assert fn(None, 1, one, 1, one, *okw, None) == E and b"planes" in L.dsic_last_error()
    assert fn(one, 1, one, 0, one, *okw, None) == E
    assert fn(one, 1, one, 70000, one, *okw, None) == E and b"65535" in L.dsic_last_error()
    assert fn(one, 1, one + 1, 1, one, *okw, None) == E and b"aligned" in L.dsic_last_error()
    assert fn(one, 1, one, 1, one, 64, 64, 32, 32, 1, 0, 64, 64, None) == E and b"window" in L.dsic_last_error()
    assert fn(one, 1, one, 1, one, 64, 64, 24, 32, 0, 0, 64, 64, None) == E
    # halving: src 64 x 64 x 3 at `one`, its validity, dst and dst validity far apart
    for fn, elem in ((L.dsic_image_halve_valid_u8, 1), (L.dsic_image_halve_valid_u16, 2)):
        a, b, c, d = far, 2 * far, 3 * far, 4 * far
        for k in range(4):
            args = [a, b, c, d]
            args[k] = None
            assert fn(*args, 64, 64, 3, None) == E and b"null" in L.dsic_last_error()
        assert fn(a, b, c, d, 64, 64, 5, None) == E and b"C=" in L.dsic_last_error()
        assert fn(a, b, c, d, 64, 64, 0, None) == E
        assert fn(a, b, c, d, 0, 64, 3, None) == E
        assert fn(a, b, c, d, 64, 0, 3, None) == E
        assert fn(a, b, a + 64 * 64 * 3 * elem - elem, d, 64, 64, 3, None) == E and b"overlap" in L.dsic_last_error()
        assert fn(a, b, c, b + 100, 64, 64, 3, None) == E and b"overlap" in L.dsic_last_error()
        assert fn(a, b, c, c + 5, 64, 64, 3, None) == E and b"overlap" in L.dsic_last_error()
        assert fn(a, b, b + 8, d, 64, 64, 3, None) == E and b"overlap" in L.dsic_last_error()
        if elem == 2:
            assert fn(a + 1, b, c, d, 64, 64, 3, None) == E and b"aligned" in L.dsic_last_error()
            assert fn(a, b, c + 1, d, 64, 64, 3, None) == E and b"aligned" in L.dsic_last_error()
    # band range
    fn = L.dsic_band_range_valid_u16
    assert fn(None, one, 8, 8, 3, one, None) == E and b"null" in L.dsic_last_error()
    assert fn(one, None, 8, 8, 3, one, None) == E
    assert fn(one, one, 8, 8, 3, None, None) == E
    assert fn(one, one, 8, 8, 5, one, None) == E and b"C=" in L.dsic_last_error()
    assert fn(one, one, 0, 8, 3, one, None) == E
    assert fn(one + 1, one, 8, 8, 3, one, None) == E and b"aligned" in L.dsic_last_error()
    assert fn(one, one, 8, 8, 3, one + 2, None) == E and b"aligned" in L.dsic_last_error()
    # resample: a 4 x 4 source at level 0 that holds the region (0, 0, 4, 4), to 2 x 2
    for fn, cmin, top, elem in ((L.dsic_window_resample_valid_u8, 3, 255, 1), (L.dsic_window_resample_valid_u16, 1, 65535, 2)):
        a, b, c, d = far, 2 * far, 3 * far, 4 * far
        geo = (4, 4, 0, 0, 3, 0, 0, 0, 4, 4)
        assert fn(None, b, *geo, c, d, 2, 2, 0, 0, None) == E and b"null" in L.dsic_last_error()
        assert fn(a, None, *geo, c, d, 2, 2, 0, 0, None) == E and b"null" in L.dsic_last_error()
        assert fn(a, b, *geo, None, d, 2, 2, 0, 0, None) == E and b"null" in L.dsic_last_error()
        assert fn(a, b, 4, 4, 0, 0, 5, 0, 0, 0, 4, 4, c, d, 2, 2, 0, 0, None) == E and b"C=" in L.dsic_last_error()
        assert fn(a, b, 4, 4, 0, 0, cmin - 1, 0, 0, 0, 4, 4, c, d, 2, 2, 0, 0, None) == E
        assert fn(a, b, *geo, c, d, 2, 2, 2, 0, None) == E and b"mode" in L.dsic_last_error()
        assert fn(a, b, *geo, c, d, 2, 2, 0, top + 1, None) == E and b"fill" in L.dsic_last_error()
        assert fn(a, b, *geo, c, d, 2, 2, 0, -1, None) == E and b"fill" in L.dsic_last_error()
        assert fn(a, b, *geo, c, d, 0, 2, 0, 0, None) == E
        assert fn(a, b, 4, 4, 0, 0, 3, 0, 0, 0, 5, 4, c, d, 2, 2, 0, 0, None) == E and b"outside" in L.dsic_last_error()
        assert fn(a, b, *geo, a + 8, d, 2, 2, 0, 0, None) == E and b"overlap" in L.dsic_last_error()
        assert fn(a, b, *geo, b + 2, d, 2, 2, 0, 0, None) == E and b"overlap" in L.dsic_last_error()
        assert fn(a, b, *geo, c, b + 2, 2, 2, 0, 0, None) == E and b"overlap" in L.dsic_last_error()
        assert fn(a, b, *geo, c, c + 2, 2, 2, 0, 0, None) == E and b"overlap" in L.dsic_last_error()
        if elem == 2:
            assert fn(a + 1, b, *geo, c, d, 2, 2, 0, 0, None) == E and b"aligned" in L.dsic_last_error()
