"""CPU-only: the whole-image codec's tile geometry, its stream framing and the argument checks of its kernels."""
import itertools
import struct

import numpy as np
import pytest

from dsic_amd import codec


def _restated(H, W, tile):
    """numpy restatement of the tiling rule: per axis, origins min(i*t, P-t) and owned [i*t, min((i+1)*t, P))."""
    out = {}
    for name, n in (("y", H), ("x", W)):
        P = -(-n // 16) * 16
        t = min(tile, P)
        i = np.arange(-(-P // t))
        out[name] = (P, t, np.minimum(i * t, P - t), np.stack([i * t, np.minimum((i + 1) * t, P)], 1))
    return out


SIZES = [17, 20, 31, 32, 33, 48, 100, 120, 127, 128, 129, 250, 256, 257, 300, 511, 600, 1000, 1023]
TILES = [32, 48, 64, 128, 256, 512]


@pytest.mark.parametrize("tile", TILES)
def test_tile_grid_matches_restatement_and_covers_once(tile):
    for H, W in itertools.product(SIZES, SIZES[::3]):
        g = codec.tile_grid(H, W, tile)
        r = _restated(H, W, tile)
        for axis, P_k, t_k, o_k, own_k in (("y", "Hp", "th", "ys", "own_y"), ("x", "Wp", "tw", "xs", "own_x")):
            P, t, origins, owned = r[axis]
            assert g[P_k] == P and g[t_k] == t
            assert g[o_k] == origins.tolist()
            assert [list(o) for o in g[own_k]] == owned.tolist()
            # owned ranges cover [0, P) exactly once, each inside its tile, every tile inside the padded image
            cover = np.zeros(P, dtype=int)
            for (a, b), o in zip(g[own_k], g[o_k]):
                cover[a:b] += 1
                assert o <= a < b <= o + t
                assert 0 <= o and o + t <= P and o % 16 == 0
            assert (cover == 1).all()
            if P <= tile:
                assert len(g[o_k]) == 1 and t == P
        assert g["n"] == g["ny"] * g["nx"] == len(g["ys"]) * len(g["xs"])
        assert g["th"] % 16 == 0 and g["tw"] % 16 == 0 and g["th"] >= 32 and g["tw"] >= 32


def test_tile_grid_examples():
    g = codec.tile_grid(600, 1000, 256)
    assert (g["Hp"], g["Wp"], g["ny"], g["nx"]) == (608, 1008, 3, 4)
    assert g["ys"] == [0, 256, 352] and g["xs"] == [0, 256, 512, 752]
    assert g["own_y"][-1] == (512, 608) and g["own_x"][-1] == (768, 1008)
    g = codec.tile_grid(120, 100, 256)
    assert (g["th"], g["tw"], g["n"], g["ys"], g["xs"]) == (128, 112, 1, [0], [0])


@pytest.mark.parametrize("H,W,tile", [(256, 256, 0), (256, 256, 16), (256, 256, 100), (256, 256, 24),
                                      (16, 256, 256), (256, 16, 256), (10, 300, 64), (300, 1, 64), (0, 64, 64)])
def test_tile_grid_refusals(H, W, tile):
    with pytest.raises(ValueError):
        codec.tile_grid(H, W, tile)


def _header(**kw):
    h = {"numerics": 0x40302, "H": 600, "W": 1000, "C": 3, "kind": 0, "th": 256, "tw": 256, "N": 128, "M": 192,
         "in_ch": 3, "spatial_params": 0, "batch": 5}
    h.update(kw)
    return h


def test_stream_header_round_trip():
    blobs = [b"DSIC2\x00" + bytes(range(50)), b"", b"\x01" * 7]
    h = _header()
    s = codec.pack_image_stream(h, blobs)
    u = codec.unpack_image_stream(s)
    assert u["blobs"] == blobs
    assert u["version"] == codec.VERSION and u["batches"] == 3
    for k, v in h.items():
        assert u[k] == v, k
    assert len(s) == 60 + sum(8 + len(b) for b in blobs)
    assert s[:6] == b"DSICI\x00"
    assert struct.unpack_from("<Q", s, 60)[0] == len(blobs[0])
    assert codec.image_bpp(s) == 8.0 * len(s) / (600 * 1000)
    assert codec.unpack_image_stream(bytearray(s))["blobs"] == blobs


def test_stream_framing_refusals():
    s = codec.pack_image_stream(_header(), [b"abc", b"defgh"])
    with pytest.raises(ValueError, match="not a DSICI"):
        codec.unpack_image_stream(b"DSICX\x00" + s[6:])
    with pytest.raises(ValueError, match="not a DSICI"):
        codec.unpack_image_stream(b"garbage")
    for cut in (1, 5, 30, 59, 60, 66, 70, len(s) - 1):
        with pytest.raises(ValueError, match="truncated"):
            codec.unpack_image_stream(s[:cut])
    with pytest.raises(ValueError, match="trailing"):
        codec.unpack_image_stream(s + b"\x00")
    with pytest.raises(ValueError, match="version"):
        codec.unpack_image_stream(s[:6] + struct.pack("<H", 99) + s[8:])


def test_kernel_argument_validation_without_gpu():
    from dsic_amd import lib
    L = lib.load()
    one = 16   # any non-null, 16-byte aligned address: every call below is refused before a launch
    assert L.dsic_tile_gather_u8(None, None, 64, 64, 3, 64, 64, 0, 1, None) == 1
    assert b"null" in L.dsic_last_error()
    assert L.dsic_tile_gather_u8(one, one, 64, 64, 5, 64, 64, 0, 1, None) == 1        # C
    assert L.dsic_tile_gather_f32(one, one, 64, 64, 3, 24, 64, 0, 1, None) == 1        # tile not a multiple of 16
    assert L.dsic_tile_stitch_f32(one, one, 64, 64, 3, 80, 64, 0, 1, None) == 1        # tile larger than the image
    assert L.dsic_tile_stitch_u8(one, one, 8, 64, 3, 32, 32, 0, 1, None) == 1          # padding not smaller than H
    assert L.dsic_tile_stitch_u8(one, one, 600, 1000, 3, 256, 256, 10, 3, None) == 1   # tiles 10..12 of 12
    assert b"outside the grid" in L.dsic_last_error()
    assert L.dsic_container_pack(None, 8, 8, None, None, None, 1, 0, 1, 1, 1, 1, 1, 1, None, None, None) == 1
    assert L.dsic_container_pack(one, 6, 8, one, one, None, 1, 0, 1, 1, 1, 1, 1, 1, one, one, None) == 1
    assert L.dsic_container_scatter(one, 40, 1, 4, one, 4, one, 4, one, one, one, None) == 1  # shorter than 38 + 24
    assert L.dsic_container_scatter(one, 100, 1, 4, one, 6, one, 4, one, one, one, None) == 1  # stride
