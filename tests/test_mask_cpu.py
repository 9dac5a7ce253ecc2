"""CPU-only: nodata masks without a GPU.  The NumPy restatement (mask_ref.py) round-trips crafted tiles in both
modes and both position sizes; the version-5 framing of codec.py (pack / unpack identity, the index's offsets, every
refusal of the readers); the stream without nodata is the stream of today; compress_image's argument refusals fire
before any device call; and the new exports are declared, bound, and refuse bad arguments."""
import ctypes
import io
import os
import random
import re
import struct

import numpy as np
import pytest
import torch

import mask_ref as R
from dsic_amd import codec, entropy, lib
from dsic_amd import mask as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAG = 0x40302
N, M = 128, 192


# ---- the restatement on crafted tiles -------------------------------------------------------------------------------
def _round_trip(m, mode):
    th, tw = m.shape
    got_mode, body = R.payload(R.delta(m))
    assert got_mode == mode, (got_mode, len(body))
    assert len(body) == th * tw // 8 if mode == 0 else len(body) < th * tw // 8
    assert np.array_equal(R.unpack_payload(got_mode, body, th, tw), m)
    assert np.array_equal(R.undelta(R.delta(m)), m)
    assert np.array_equal(R.unpack_bits(R.pack_bits(m), th, tw), m)
    K.check_payload(body, got_mode, th, tw)
    return body


def test_crafted_tiles_round_trip():
    th = tw = 64
    one = np.zeros((th, tw), bool)
    one[17, 5] = True
    body = _round_trip(one, 1)
    assert np.frombuffer(body, "<u2").tolist() == [17 * tw + 5, 18 * tw + 5]         # on at row 17, off at row 18
    _round_trip(~one, 1)
    straight = np.zeros((th, tw), bool)
    straight[:, :23] = True
    assert len(_round_trip(straight, 1)) == 2 * 23                                   # one bit per column of the edge
    yy, xx = np.mgrid[:th, :tw]
    assert len(_round_trip(2 * yy + xx < 70, 1)) <= 2 * 2 * tw                       # a column goes on at row 0 and off once
    _round_trip((yy + xx) % 2 == 0, 0)                                               # checkerboard: d is all ones below row 0
    # a list exactly as long as the plane: th*tw/16 set bits of d at 2 bytes each
    d = np.zeros(th * tw, bool)
    d[:th * tw // 16] = True
    m = R.undelta(d.reshape(th, tw))
    assert R.payload(R.delta(m))[0] == 0 and len(_round_trip(m, 0)) == th * tw // 8
    d[th * tw // 16 - 1] = False                                                      # one fewer: the list wins
    assert len(_round_trip(R.undelta(d.reshape(th, tw)), 1)) == th * tw // 8 - 2


def test_position_sizes():
    last = np.zeros((256, 256), bool)
    last[255, 255] = True                                                             # th*tw = 65536: u16, position 65535
    assert np.frombuffer(_round_trip(last, 1), "<u2").tolist() == [65535]
    assert K.pos_bytes(256, 256) == 2 and K.pos_bytes(272, 256) == 4 and K.pos_bytes(272, 272) == 4
    big = np.zeros((272, 272), bool)
    big[271, 271] = big[100, 3] = True
    assert np.frombuffer(_round_trip(big, 1), "<u4").tolist() == [100 * 272 + 3, 101 * 272 + 3, 271 * 272 + 271]
    assert R.pos_dtype(272, 272) == "<u4" and R.pos_dtype(256, 256) == "<u2"


def test_states_ignore_padding_and_neighbours_rows():
    # 40 x 70, tile 32: rows 32..39 belong to tile row 1, whose origin is 16; columns 64..69 to tile column 2 (origin 48)
    img = np.full((40, 70, 3), 9, np.uint8)
    img[32:, 64:] = 0
    st = R.states(R.nodata_mask(img, 0), 40, 70, 32, 32)
    assert st == [1, 1, 1, 1, 1, 0]
    m = R.m_plane(R.nodata_mask(img, 0), R.tiles(40, 70, 32, 32)[5], 32, 32)
    assert m.sum() == 8 * 6 and m[16:24, 16:22].all()
    img[39, 69] = 1
    assert R.states(R.nodata_mask(img, 0), 40, 70, 32, 32)[5] == 2
    assert [K.tile_states([0, 5, 9], [9, 9, 9])] == [[1, 2, 0]]
    g = codec.tile_grid(40, 70, 32)
    for t, (oy, ox, y0, y1, x0, x1) in enumerate(R.tiles(40, 70, 32, 32)):
        assert codec._owned_in_tile(g, t) == (y0 - oy, y1 - oy, x0 - ox, x1 - ox)


# ---- version-5 framing ------------------------------------------------------------------------------------------------
def _scene(H=300, W=530, v=0, seed=3):
    rng = np.random.default_rng(seed)
    img = rng.integers(1, 256, size=(H, W, 3), dtype=np.uint8)
    yy, xx = np.mgrid[:H, :W]
    img[2 * yy + xx < 500] = v
    img[200:260, 400:460][rng.random((60, 60)) < 0.5] = v
    return img


def _build(img, v, tile, batch, seed=0):
    """A version-5 stream in pure Python: the restatement's mask block, made-up strings for the coded tiles."""
    rng = random.Random(seed)
    H, W, C = img.shape
    g = codec.tile_grid(H, W, tile)
    block, st = R.block(img, v, g["th"], g["tw"])
    ids = [t for t, s in enumerate(st) if s]
    blobs, strings = [], {}
    for first in range(0, len(ids), batch):
        sel = ids[first:first + batch]
        B = len(sel)
        comp = {"strings": [], "shape_y": [B, M, g["th"] // 16, g["tw"] // 16],
                "shape_z": [B, N, g["th"] // 64, g["tw"] // 64], "min_y": [-3] * B, "max_y": [4] * B,
                "min_z": [-2] * B, "max_z": [2] * B, "numerics": TAG}
        for t in sel:
            strings[t] = [bytes(rng.getrandbits(8) for _ in range(rng.choice([0, 3, 17, 100]))),
                          bytes(rng.getrandbits(8) for _ in range(rng.choice([1, 16, 250])))]
            comp["strings"].append(strings[t])
        blobs.append(entropy.pack_container(comp))
    header = {"numerics": TAG, "H": H, "W": W, "C": C, "kind": 0, "th": g["th"], "tw": g["tw"], "N": N, "M": M,
              "in_ch": C, "spatial_params": 0, "batch": batch, "nodata": v}
    return codec.pack_image_stream(header, blobs, mask=block), header, blobs, block, st, strings


def test_pack_then_unpack_is_the_identity_and_the_index_finds_every_byte():
    img = _scene()
    stream, header, blobs, block, st, strings = _build(img, 0, 128, 4)
    assert set(st) == {0, 1, 2}
    u = codec.unpack_image_stream(stream)
    assert u["version"] == 5 and u["nodata"] == 0 and u["coded"] == sum(1 for s in st if s) and u["overlap"] == 0
    assert u["blobs"] == blobs and u["mask"] == block and u["batches"] == len(blobs) == -(-u["coded"] // 4)
    assert codec.pack_image_stream(u, u["blobs"], mask=u["mask"]) == stream
    assert stream[u["mask_offset"]:u["mask_offset"] + u["mask_bytes"]] == block and u["mask_offset"] == 76 + 8
    assert codec.image_bpp(stream) == 8.0 * len(stream) / (300 * 530)
    ix = codec.stream_index(stream)
    for key in ("nodata", "coded", "mask_offset", "mask_bytes"):
        assert ix[key] == u[key]
    _, _, _, _, _, payloads = R.parse_block(block)
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
            assert (r["m_off"], r["m_len"]) in [(o, n) for o, n in codec.tile_spans(ix, [t])] or r["m_len"] == 0
        else:
            assert "m_off" not in r
    assert modes == {0, 1}
    every = list(range(len(st)))
    want = sum(len(a) + len(b) for a, b in strings.values()) + sum(len(p) for _, p in payloads.values())
    assert sum(n for _, n in codec.tile_spans(ix, every)) == want
    # from a file: the heads, the mask block's head, states and records; no string and no payload
    f = io.BytesIO(stream)
    src = codec._Source(f)
    assert codec._index_of(src) == ix
    nm = len(payloads)
    assert ix["index_bytes"] == 60 + 16 + 8 + 26 + K.states_bytes(len(st)) + 12 * nm + sum(8 + 38 + 24 * len(c["ids"])
                                                                                           for c in ix["containers"])
    assert codec.window_tiles(ix, 0, 0, 300, 530) == every


def test_all_nodata_and_no_nodata_streams():
    img = np.zeros((100, 90, 3), np.uint8)
    stream, *_ , st, _ = _build(img, 0, 64, 4)
    assert set(st) == {0}
    u = codec.unpack_image_stream(stream)
    assert u["batches"] == 0 and u["coded"] == 0 and u["blobs"] == []
    ix = codec.stream_index(stream)
    assert ix["containers"] == [] and all(r["state"] == 0 and r["k"] is None for r in ix["tiles"])
    assert codec.tile_spans(ix, list(range(len(st)))) == []
    stream, *_, st, _ = _build(img + 5, 0, 64, 4)
    assert set(st) == {1} and codec.unpack_image_stream(stream)["coded"] == len(st)


def test_a_stream_without_nodata_is_the_stream_of_today():
    img = _scene()
    _, header, blobs, _, _, _ = _build(np.full_like(img, 7), 0, 128, 4)              # every tile coded
    plain = dict(header)
    del plain["nodata"]
    want = (struct.pack("<6sHI6I4I2I", b"DSICI\0", 1, TAG, 300, 530, 3, 0, 128, 128, N, M, 3, 0, 4, len(blobs))
            + b"".join(struct.pack("<Q", len(b)) + b for b in blobs))
    assert codec.pack_image_stream(plain, blobs) == want
    assert codec.pack_image_stream(dict(plain, nodata=None), blobs) == want
    ix = codec.stream_index(want)
    assert "nodata" not in ix and "state" not in ix["tiles"][0] and "ids" not in ix["containers"][0]
    assert set(ix["tiles"][0]) == {"k", "b", "min_y", "max_y", "min_z", "max_z", "z_off", "z_len", "y_off", "y_len",
                                   "y_segs"}
    with pytest.raises(ValueError, match="mask block without nodata"):
        codec.pack_image_stream(plain, blobs, mask=b"x")
    with pytest.raises(ValueError, match="needs the mask block"):
        codec.pack_image_stream(header, blobs)


def _patched(stream, at, fmt, *vals):
    b = bytearray(stream)
    struct.pack_into(fmt, b, at, *vals)
    return bytes(b)


def test_every_refusal_of_the_readers():
    img = _scene()
    stream, header, blobs, block, st, _ = _build(img, 0, 128, 4)
    n, nm = len(st), st.count(2)
    mo = 84                                                    # the mask block: 60 + 16 head bytes, 8 of length
    states_at, recs_at = mo + 26, mo + 26 + K.states_bytes(n)
    mixed = [t for t, s in enumerate(st) if s == 2]
    full = st.index(1)
    ix = codec.stream_index(stream)
    raw = 128 * 128 // 8

    def refuses(s, match):
        with pytest.raises(ValueError, match=match):
            codec.stream_index(s)

    refuses(_patched(stream, states_at + full, "<B", 3), "state above 2")
    refuses(_patched(stream, states_at + full, "<B", 0), "coded tiles")                  # nc against the states
    refuses(_patched(stream, 72, "<I", ix["coded"] + 1), "batches|coded")                # nc in the head
    refuses(_patched(stream, mo + 22, "<I", nm + 1), "truncated|records")                # nm against the states
    refuses(_patched(stream, states_at + full, "<B", 2), "records")                      # one more mixed tile than records
    refuses(_patched(stream, recs_at, "<I", mixed[0] + 1 if mixed[0] + 1 not in mixed else full), "ascending")
    if nm > 1:
        a, b = stream[recs_at:recs_at + 12], stream[recs_at + 12:recs_at + 24]
        refuses(stream[:recs_at] + b + a + stream[recs_at + 24:], "ascending")
    refuses(_patched(stream, recs_at + 4, "<I", 2), "mode 2")
    mode0 = next(i for i, t in enumerate(mixed) if ix["tiles"][t]["m_mode"] == 0)
    mode1 = next(i for i, t in enumerate(mixed) if ix["tiles"][t]["m_mode"] == 1)
    refuses(_patched(stream, recs_at + 12 * mode0 + 8, "<I", raw - 2), "raw mask")
    refuses(_patched(stream, recs_at + 12 * mode1 + 8, "<I", ix["tiles"][mixed[mode1]]["m_len"] + 1), "multiple of 2")
    refuses(_patched(stream, recs_at + 12 * mode1 + 4, "<II", 1, raw), "not shorter")
    refuses(_patched(stream, recs_at + 12 * mode1 + 8, "<I", ix["tiles"][mixed[mode1]]["m_len"] + 2), "truncated or oversized")
    for at, what in ((mo + 6, "n"), (mo + 10, "th"), (mo + 14, "tw"), (mo + 18, "nodata")):
        refuses(_patched(stream, at, "<I", 48), "head says")
    refuses(_patched(stream, mo, "<6s", b"DSICX\0"), "not a mask block")
    refuses(_patched(stream, 64, "<I", 16), "overlap=16")
    refuses(_patched(stream, 68, "<I", 256), "nodata=256")
    refuses(_patched(stream, 56, "<I", len(blobs) + 1), "batches|truncated")
    last = ix["containers"][-1]["offset"] - 8                 # the stream without its last container, the head agreeing
    refuses(_patched(stream[:last], 56, "<I", len(blobs) - 1), "batches for")
    refuses(stream + b"\0", "trailing")
    for cut in (70, 80, mo + 10, recs_at + 5, len(stream) - 1):
        refuses(stream[:cut], "truncated")
    with pytest.raises(ValueError, match="truncated"):
        codec.unpack_image_stream(stream[:mo + 3])
    with pytest.raises(ValueError, match="containers for"):
        codec.pack_image_stream(header, blobs[:-1], mask=block)
    with pytest.raises(ValueError, match="overlap"):
        codec.pack_image_stream(dict(header, overlap=16), blobs, mask=block)
    with pytest.raises(ValueError, match="max_error"):
        codec.pack_image_stream(dict(header, max_error=1), blobs, mask=block)
    # positions are checked on the host as they arrive, before any upload
    t1 = mixed[mode1]
    body = stream[ix["tiles"][t1]["m_off"]:ix["tiles"][t1]["m_off"] + ix["tiles"][t1]["m_len"]]
    K.check_payload(body, 1, 128, 128)
    pos = np.frombuffer(body, "<u2").copy()
    for bad in (np.r_[pos[1], pos[0], pos[2:]], np.r_[pos[0], pos[0], pos[2:]], np.r_[pos[:-1], 128 * 128]):
        with pytest.raises(ValueError, match="ascend"):
            K.check_payload(bad.astype("<u2" if bad.max() < 65536 else "<u4").tobytes(), 1, 128, 128)
    with pytest.raises(ValueError, match="ascend"):
        K.check_payload(struct.pack("<2I", 5, 272 * 272), 1, 272, 272)


# ---- compress_image's argument checks ---------------------------------------------------------------------------------
def test_compress_image_refuses_before_it_touches_the_device():
    class Stub(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.N, self.M = N, M
            self.g_a = torch.nn.Module()
            self.g_a.g_a = torch.nn.ModuleList([torch.nn.Conv2d(3, 4, 1)])

    model, img = Stub(), torch.zeros((330, 530, 3), dtype=torch.uint8)
    for bad in (True, False, 256, -1, 1.0, "0", np.bool_(True)):
        with pytest.raises(ValueError, match="nodata="):
            codec.compress_image(model, img, tile=128, nodata=bad)
    with pytest.raises(ValueError, match="uint8"):
        codec.compress_image(model, torch.zeros((3, 330, 530)), tile=128, nodata=0)
    with pytest.raises(ValueError, match="nodata together with overlap"):
        codec.compress_image(model, img, tile=128, nodata=0, overlap=16)
    with pytest.raises(ValueError, match="nodata together with max_error"):
        codec.compress_image(model, img, tile=128, nodata=0, max_error=0)
    with pytest.raises(ValueError, match="nodata together with overviews"):
        codec.compress_image(model, img, tile=128, nodata=255, overviews=1)
    assert K.check_nodata(np.uint8(255), "x") == 255 and K.check_nodata(0, "x") == 0


# ---- the exports ------------------------------------------------------------------------------------------------------
NEW = {"dsic_mask_classify_u8": 11, "dsic_mask_delta_planes_u8": 12, "dsic_mask_pack": 9, "dsic_mask_unpack": 8,
       "dsic_mask_apply_u8": 16, "dsic_mask_apply_f32": 16}


def test_the_new_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "dsic_hip.h")).read()
    declared = set(re.findall(r"\b(dsic_[a-zA-Z0-9_]+)\s*\(", header))
    assert set(NEW) <= declared and set(NEW) <= set(lib.SIGNATURES)
    for name, nargs in NEW.items():
        res, args = lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs and getattr(lib.load(), name) is not None


def test_the_mask_calls_check_their_arguments_without_a_gpu():
    L = lib.load()
    one = 16   # any non-null, 16-byte aligned address: every call below is refused before a launch
    E = lib.DSIC_EINVAL
    assert L.dsic_mask_classify_u8(None, 64, 64, 3, 32, 32, 0, 0, 4, one, None) == E and b"null" in L.dsic_last_error()
    assert L.dsic_mask_classify_u8(one, 64, 64, 3, 32, 32, 0, 0, 4, None, None) == E
    assert L.dsic_mask_classify_u8(one, 64, 64, 5, 32, 32, 0, 0, 4, one, None) == E                 # C
    assert L.dsic_mask_classify_u8(one, 64, 64, 3, 32, 32, 256, 0, 4, one, None) == E and b"nodata" in L.dsic_last_error()
    assert L.dsic_mask_classify_u8(one, 64, 64, 3, 32, 32, -1, 0, 4, one, None) == E
    assert L.dsic_mask_classify_u8(one, 64, 64, 3, 24, 32, 0, 0, 4, one, None) == E                 # tile not a multiple of 16
    assert L.dsic_mask_classify_u8(one, 64, 64, 3, 80, 32, 0, 0, 1, one, None) == E                 # tile larger than the image
    assert L.dsic_mask_classify_u8(one, 64, 64, 3, 32, 32, 0, 2, 3, one, None) == E                 # tiles 2..4 of 4
    assert b"outside the grid" in L.dsic_last_error()
    assert L.dsic_mask_classify_u8(one, 0, 64, 3, 32, 32, 0, 0, 1, one, None) == E
    d = (one, 64, 64, 3, 32, 32, 0)
    assert L.dsic_mask_delta_planes_u8(*d, None, 1, one, one, None) == E and b"null" in L.dsic_last_error()
    assert L.dsic_mask_delta_planes_u8(*d, one, 1, None, one, None) == E
    assert L.dsic_mask_delta_planes_u8(*d, one, 1, one, None, None) == E
    assert L.dsic_mask_delta_planes_u8(*d, one, 0, one, one, None) == E
    assert L.dsic_mask_delta_planes_u8(*d, one, 70000, one, one, None) == E
    assert L.dsic_mask_delta_planes_u8(*d, one, 1, one + 2, one, None) == E and b"aligned" in L.dsic_last_error()
    assert L.dsic_mask_delta_planes_u8(one, 64, 64, 3, 32, 32, 300, one, 1, one, one, None) == E
    assert L.dsic_mask_pack(None, one, one, 1, 32, 32, one, one, None) == E and b"null" in L.dsic_last_error()
    assert L.dsic_mask_pack(one, one, one, 1, 32, 32, None, one, None) == E
    assert L.dsic_mask_pack(one, one, one, 0, 32, 32, one, one, None) == E
    assert L.dsic_mask_pack(one, one, one, 1, 32, 40, one, one, None) == E
    assert L.dsic_mask_pack(one, one, one, 1, 16, 32, one, one, None) == E
    assert L.dsic_mask_pack(one, one, one, 1, 32, 32, one, one + 1, None) == E and b"aligned" in L.dsic_last_error()
    assert L.dsic_mask_unpack(None, 10, one, 1, 32, 32, one, None) == E and b"null" in L.dsic_last_error()
    assert L.dsic_mask_unpack(one, 10, None, 1, 32, 32, one, None) == E
    assert L.dsic_mask_unpack(one, -1, one, 1, 32, 32, one, None) == E
    assert L.dsic_mask_unpack(one, 10, one, 1, 32, 8192, one, None) == E                            # tw over 4096
    assert L.dsic_mask_unpack(one, 10, one, 1, 32, 32, one + 4, None) == E and b"aligned" in L.dsic_last_error()
    assert L.dsic_mask_unpack(one, 10, one, 0, 32, 32, one, None) == E
    for fn, C in ((L.dsic_mask_apply_u8, 3), (L.dsic_mask_apply_f32, 3)):
        ok = (64, 64, C, 32, 32, 0, 0, 64, 64)
        assert fn(one, 1, None, 1, 0, one, *ok, None) == E and b"null" in L.dsic_last_error()
        assert fn(one, 1, one, 1, 0, None, *ok, None) == E
        assert fn(None, 1, one, 1, 0, one, *ok, None) == E and b"planes" in L.dsic_last_error()
        assert fn(one, -1, one, 1, 0, one, *ok, None) == E
        assert fn(one, 1, one, 0, 0, one, *ok, None) == E
        assert fn(one, 1, one, 1, 256, one, *ok, None) == E and b"nodata" in L.dsic_last_error()
        assert fn(one, 1, one, 1, 0, one + 8, *ok, None) == E and b"aligned" in L.dsic_last_error()
        assert fn(one, 1, one, 1, 0, one, 64, 64, C, 32, 32, 0, 1, 64, 64, None) == E and b"window" in L.dsic_last_error()
        assert fn(one, 1, one, 1, 0, one, 64, 64, C, 32, 24, 0, 0, 64, 64, None) == E
        assert fn(one, 1, one, 1, 0, one, 64, 64, 9, 32, 32, 0, 0, 64, 64, None) == E                # C
