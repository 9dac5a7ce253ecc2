"""CPU-only: overlapped tiles with blended seams: the geometry and its weights in exact fractions, window_tiles
against brute force, version 3 of the image stream, the float32 blend restatement against float64, and the argument
checks of the new kernels."""
import random
import struct
from fractions import Fraction

import numpy as np
import pytest

import blend_ref as R
from dsic_amd import codec, entropy

TAG = 0x40302
N, M = 128, 192


def _sizes(tile):
    """L <= tile, L = tile + 1, multiples, and sizes that shift the last tile inward."""
    base = [17, 31, 32, 33, 48, 63, 64, 65, 100, 127, 128, 129, 200, 250, 256, 257, 300, 500, 511, 513, 600, 777, 899]
    near = [tile - 1, tile, tile + 1, tile + 15, tile + 16, tile + 17, 2 * tile - 16, 2 * tile, 2 * tile + 1,
            3 * tile - 33, 3 * tile + 40]
    return sorted({L for L in base + near if L >= 17})


@pytest.mark.parametrize("tile", [32, 64, 256])
def test_weights_are_a_partition_of_unity_inside_the_real_tiles(tile):
    for O in R.valid_overlaps(tile):
        for L in _sizes(tile):
            ax = R.axis(L, tile, O)
            w = R.weights_exact(ax, O)
            n, Lp = ax["n"], ax["Lp"]
            for p in range(Lp):
                col = [w[i][p] for i in range(n)]
                assert sum(col) == 1, (tile, O, L, p)
                assert sum(1 for v in col if v != 0) <= 2, (tile, O, L, p)
                assert all(0 <= v <= 1 for v in col)
            for i, (lo, hi) in enumerate(ax["sup"]):
                assert ax["o"][i] <= lo < hi <= ax["o"][i] + ax["t"] <= Lp, (tile, O, L, i)
                assert all(w[i][p] == 0 for p in range(Lp) if not lo <= p < hi)
                assert all(w[i][p] > 0 for p in range(lo, hi))
            assert ax["a"][-1] + (O if n > 1 else 0) <= Lp
            assert ax["o"][:-1] == ax["a"][:-1]                          # only the last tile shifts inward
            if Lp <= tile:
                assert n == 1 and ax["t"] == Lp
            # the float32 weights are the exact ones rounded: within 2 ulp (the reciprocal, then the multiply)
            w32 = R.weights_f32(ax, O)
            exact = np.array([[float(v) for v in row] for row in w], dtype=np.float64)
            assert np.all(np.abs(w32.astype(np.float64) - exact) <= 2.0 ** -23 * exact)
            assert np.all(w32[exact == 1] == 1) and np.all(w32[exact == 0] == 0)


def _todays_grid(H, W, tile):
    Hp, Wp = R.ceil16(H), R.ceil16(W)
    th, tw = min(tile, Hp), min(tile, Wp)
    ny, nx = -(-Hp // th), -(-Wp // tw)
    return {"H": H, "W": W, "Hp": Hp, "Wp": Wp, "th": th, "tw": tw, "ny": ny, "nx": nx, "n": ny * nx,
            "ys": [min(i * th, Hp - th) for i in range(ny)], "xs": [min(j * tw, Wp - tw) for j in range(nx)],
            "own_y": [(i * th, min((i + 1) * th, Hp)) for i in range(ny)],
            "own_x": [(j * tw, min((j + 1) * tw, Wp)) for j in range(nx)]}


def test_tile_grid_without_overlap_is_todays():
    for tile in (32, 48, 64, 256):
        for H in (17, 33, 64, 100, 129, 257, 600):
            for W in (20, 65, 256, 300, 1000):
                want = _todays_grid(H, W, tile)
                for g in (codec.tile_grid(H, W, tile), codec.tile_grid(H, W, tile, overlap=0)):
                    assert {k: g[k] for k in want} == want
                    assert g["overlap"] == 0 and (g["sy"], g["sx"]) == (g["th"], g["tw"])
                    assert g["sup_y"] == g["own_y"] and g["sup_x"] == g["own_x"]


def test_tile_grid_with_overlap_matches_the_restatement():
    for tile in (32, 64, 256):
        for O in R.valid_overlaps(tile):
            for H, W in ((70, 90), (120, 200), (130, 64), (64, 300), (300, 300), (150, 200), (tile + 1, 3 * tile)):
                g = codec.tile_grid(H, W, tile, overlap=O)
                ay, ax = R.axis(H, tile, O), R.axis(W, tile, O)
                assert (g["Hp"], g["th"], g["sy"], g["ny"], g["ys"]) == (ay["Lp"], ay["t"], ay["s"], ay["n"], ay["o"])
                assert (g["Wp"], g["tw"], g["sx"], g["nx"], g["xs"]) == (ax["Lp"], ax["t"], ax["s"], ax["n"], ax["o"])
                assert g["sup_y"] == ay["sup"] and g["sup_x"] == ax["sup"]
                assert g["own_y"] == [(a, b) for a, b in zip(ay["a"], ay["a"][1:] + [ay["Lp"]])]
                assert g["own_x"] == [(a, b) for a, b in zip(ax["a"], ax["a"][1:] + [ax["Lp"]])]
                assert g["overlap"] == O and g["n"] == ay["n"] * ax["n"]
    g = codec.tile_grid(150, 200, 64, overlap=16)
    assert (g["ny"], g["nx"], g["ys"], g["xs"]) == (3, 4, [0, 48, 96], [0, 48, 96, 144])
    g = codec.tile_grid(4096, 4096, 256, overlap=16)
    assert (g["ny"], g["nx"]) == (17, 17)


@pytest.mark.parametrize("overlap", [-16, 8, 24, 144, 1 << 20, "16", 16.0])
def test_tile_grid_refuses_a_bad_overlap(overlap):
    with pytest.raises(ValueError):
        codec.tile_grid(600, 1000, 256, overlap=overlap)
    assert codec.tile_grid(600, 1000, 256, overlap=128)["overlap"] == 128


def test_window_tiles_equals_brute_force():
    rng = random.Random(3)
    for tile, O, H, W in list(R.CASES.values()) + [(64, 16, 150, 200), (64, 32, 150, 200), (32, 16, 33, 200)]:
        g = codec.tile_grid(H, W, tile, overlap=O)
        g0 = codec.tile_grid(H, W, tile)
        wins = [(0, 0, H, W), (0, 0, 1, 1), (H - 1, W - 1, 1, 1)]
        for _ in range(40):
            y0, x0 = rng.randrange(H), rng.randrange(W)
            wins.append((y0, x0, rng.randint(1, H - y0), rng.randint(1, W - x0)))
        for win in wins:
            got = codec.window_tiles(g, *win)
            assert got == R.contributing(H, W, g["th"], g["tw"], O, *win), (tile, O, H, W, win)
            assert got == sorted(set(got))
            assert codec.window_tiles({"grid": g}, *win) == got
            # at overlap 0: today's list, the tiles whose owned rectangle meets the window
            y0, x0, h, w = win
            today = [i * g0["nx"] + j for i in range(y0 // g0["th"], (y0 + h - 1) // g0["th"] + 1)
                     for j in range(x0 // g0["tw"], (x0 + w - 1) // g0["tw"] + 1)]
            assert codec.window_tiles(g0, *win) == today == R.contributing(H, W, g0["th"], g0["tw"], 0, *win)
    with pytest.raises(ValueError, match="window"):
        codec.window_tiles(codec.tile_grid(150, 200, 64, overlap=16), 0, 0, 151, 10)


# ---- version-3 streams ------------------------------------------------------------------------------------------
def _comp(B, K, rng, hy, wy):
    comp = {"strings": [], "shape_y": [B, M, hy, wy], "shape_z": [B, N, max(1, hy // 4), max(1, wy // 4)],
            "min_y": [], "max_y": [], "min_z": [], "max_z": [], "numerics": TAG}
    seg = []
    for _ in range(B):
        lens = [rng.choice([0, 1, 3, 15, 16, 33]) for _ in range(K)]
        zl = rng.choice([0, 1, 3, 16, 17])
        comp["strings"].append([bytes(rng.getrandbits(8) for _ in range(zl)),
                                bytes(rng.getrandbits(8) for _ in range(sum(lens)))])
        seg.append(lens)
        comp["min_y"].append(-5), comp["max_y"].append(7), comp["min_z"].append(-3), comp["max_z"].append(2)
    if K > 1:
        comp["segments"], comp["seg_lengths_y"] = K, seg
    return comp


def _stream(H, W, tile, batch, K, O, seed=0, n_tiles=None):
    rng = random.Random(seed)
    g = codec.tile_grid(H, W, tile, overlap=O)
    n = g["n"] if n_tiles is None else n_tiles
    comps = [_comp(min(batch, n - first), K, rng, g["th"] // 16, g["tw"] // 16) for first in range(0, n, batch)]
    blobs = [entropy.pack_container(c) for c in comps]
    header = {"numerics": TAG, "H": H, "W": W, "C": 3, "kind": 0, "th": g["th"], "tw": g["tw"], "N": N, "M": M,
              "in_ch": 3, "spatial_params": 0, "batch": batch, "segments": K, "overlap": O}
    return codec.pack_image_stream(header, blobs), g, comps, blobs, header


@pytest.mark.parametrize("K", [1, 4])
def test_version_3_round_trip_and_index(K):
    stream, g, comps, blobs, header = _stream(150, 200, 64, 5, K, 16, seed=K)
    assert g["n"] == 12 and len(blobs) == 3
    assert struct.unpack_from("<H", stream, 6)[0] == 3 == codec.VERSION_OV
    assert struct.unpack_from("<2I", stream, 60) == (K, 16)
    assert blobs[0][:6] == (b"DSIC2\x00" if K == 1 else b"DSIC3\x00")
    u = codec.unpack_image_stream(stream)
    assert u["version"] == 3 and u["segments"] == K and u["overlap"] == 16 and u["blobs"] == blobs
    for k, v in header.items():
        assert u[k] == v, k
    assert codec.pack_image_stream(u, u["blobs"]) == stream
    ix = codec.stream_index(stream)
    assert ix["overlap"] == 16 and ix["segments"] == K and ix["grid"] == g and len(ix["tiles"]) == 12
    for t, r in enumerate(ix["tiles"]):
        k, b = divmod(t, 5)
        zs, ys = comps[k]["strings"][b]
        assert stream[r["z_off"]:r["z_off"] + r["z_len"]] == zs and stream[r["y_off"]:r["y_off"] + r["y_len"]] == ys
    head = 38 if K == 1 else 42
    assert ix["index_bytes"] == 68 + sum(8 + head + (24 + (4 * K if K > 1 else 0)) * c["tiles"]
                                         for c in ix["containers"])
    assert codec.window_tiles(ix, 40, 40, 20, 20) == [0, 1, 4, 5]        # rows 48..63 and columns 48..63 are ramps


def test_version_3_refusals():
    stream, g, _, blobs, header = _stream(150, 200, 64, 5, 1, 16)
    for bad in (8, 24, 48, -16, 1 << 31):                                # not a multiple of 16, or over half a tile
        with pytest.raises(ValueError, match="overlap"):
            codec.pack_image_stream(dict(header, overlap=bad), blobs)
        if bad > 0:
            forged = stream[:64] + struct.pack("<I", bad & 0xFFFFFFFF) + stream[68:]
            with pytest.raises(ValueError, match="overlap"):
                codec.unpack_image_stream(forged)
            with pytest.raises(ValueError, match="overlap"):
                codec.stream_index(forged)
    zero = stream[:64] + struct.pack("<I", 0) + stream[68:]              # a version-3 head with overlap 0
    with pytest.raises(ValueError, match="overlap"):
        codec.unpack_image_stream(zero)
    with pytest.raises(ValueError, match="overlap"):
        codec.stream_index(zero)
    with pytest.raises(ValueError, match="segments"):
        codec.unpack_image_stream(stream[:60] + struct.pack("<I", 3) + stream[64:])
    for cut in (61, 64, 67):
        with pytest.raises(ValueError, match="truncated"):
            codec.unpack_image_stream(stream[:cut])
    # 128 x 128 in tiles of 64: 4 tiles without overlap (one batch of 5), 9 with overlap 16 (two batches)
    four, *_ = _stream(128, 128, 64, 5, 1, 16, n_tiles=4)
    assert codec.unpack_image_stream(four)["batches"] == 1
    with pytest.raises(ValueError, match="batches"):
        codec.stream_index(four)
    full, _, _, blobs9, header9 = _stream(128, 128, 64, 5, 1, 16)
    assert codec.stream_index(full)["grid"]["n"] == 9 and len(blobs9) == 2
    as_v1 = codec.pack_image_stream(dict(header9, overlap=0), blobs9)
    assert struct.unpack_from("<H", as_v1, 6)[0] == 1
    with pytest.raises(ValueError, match="batches"):
        codec.stream_index(as_v1)
    # an overlap that fits tile_grid's tile but not the stream's smaller tiles
    small = dict(header, H=40, W=200, th=48, tw=64, overlap=32)
    with pytest.raises(ValueError, match="overlap"):
        codec.pack_image_stream(small, blobs)


def test_overlap_0_streams_are_byte_identical():
    rng = random.Random(9)
    g = codec.tile_grid(150, 200, 64)
    for K, version, head_len in ((1, 1, 60), (4, 2, 64)):
        blobs = [entropy.pack_container(_comp(min(5, g["n"] - f), K, rng, 4, 4)) for f in range(0, g["n"], 5)]
        header = {"numerics": TAG, "H": 150, "W": 200, "C": 3, "kind": 0, "th": 64, "tw": 64, "N": N, "M": M,
                  "in_ch": 3, "spatial_params": 0, "batch": 5, "segments": K}
        want = struct.pack("<6sHI6I4I2I", b"DSICI\x00", version, TAG, 150, 200, 3, 0, 64, 64, N, M, 3, 0, 5, len(blobs))
        if K > 1:
            want += struct.pack("<I", K)
        want += b"".join(struct.pack("<Q", len(b)) + b for b in blobs)
        assert codec.pack_image_stream(header, blobs) == want
        assert codec.pack_image_stream(dict(header, overlap=0), blobs) == want
        assert len(want) == head_len + sum(8 + len(b) for b in blobs)
        u = codec.unpack_image_stream(want)
        assert u["overlap"] == 0 and u["version"] == version
        assert codec.stream_index(want)["overlap"] == 0


# ---- the float32 restatement against float64 --------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(R.CASES))
@pytest.mark.parametrize("C", [3, 4])
def test_float32_blend_stays_within_the_rounding_bound(case, C):
    tile, O, H, W = R.CASES[case]
    tiles = R.make_tiles(case, C)
    assert tiles.min() < 0 and tiles.max() > 1 and np.abs(tiles[tiles != 0]).min() > 1e-30
    th, tw = tiles.shape[2:]
    batch = [(t, tiles[t]) for t in range(len(tiles))]
    got = R.blend_f32([batch], H, W, C, th, tw, O)
    ref, mass = R.blend_f64([batch], H, W, C, th, tw, O)
    err = np.abs(got.astype(np.float64) - ref)
    bound = R.error_bound(mass)
    print(f"{case} C={C}: max |f32 - f64| = {err.max():.3e}, smallest bound/err margin = "
          f"{(bound - err).min():.3e}, max before the finish = {got.max()!r}")
    assert np.all(err <= bound)
    assert R.BOUND_ROUNDINGS <= 12
    assert np.all(err <= 12 * 2.0 ** -24 * mass)
    assert np.all(ref <= 1 + 1e-12) and np.all(ref >= 0)
    fin = R.finish_f32(got)
    assert fin.dtype == np.float32 and fin.min() >= 0 and fin.max() <= 1
    u8 = R.finish_u8(got)
    assert u8.shape == (H, W, C) and u8.dtype == np.uint8
    # cutting the tiles into batches does not enter the restatement
    ones = [[b] for b in batch]
    assert np.array_equal(R.blend_f32(ones, H, W, C, th, tw, O), got)
    # a pixel with one contributor of weight 1 is that tile's clamp01 value
    ay, ax = R.grid(H, W, th, tw, O)
    wy, wx = R.weights_exact(ay, O), R.weights_exact(ax, O)
    for t in range(len(tiles)):
        i, j = divmod(t, ax["n"])
        ys = [p for p in range(H) if wy[i][p] == 1]
        xs = [p for p in range(W) if wx[j][p] == 1]
        if ys and xs:
            sub = tiles[t][:, ys[0] - ay["o"][i]:ys[-1] + 1 - ay["o"][i], xs[0] - ax["o"][j]:xs[-1] + 1 - ax["o"][j]]
            assert np.array_equal(got[:, ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1], np.clip(sub, 0, 1))


def test_float32_weights_can_exceed_one_before_the_finish():
    """Why the finish pass exists: for some overlaps the four float32 weights of a corner pixel sum above 1."""
    worst = 0.0
    for O in (48, 80, 96, 112):
        ax = R.axis(3 * 256, 256, O)
        w = R.weights_f32(ax, O)
        a1 = ax["a"][1]
        dn, up = w[0][a1:a1 + O], w[1][a1:a1 + O]                       # tile 0 fades out, tile 1 fades in
        tot = ((dn[:, None] * dn[None, :] + dn[:, None] * up[None, :]) + up[:, None] * dn[None, :]) \
            + up[:, None] * up[None, :]
        assert tot.dtype == np.float32
        worst = max(worst, float(tot.max()))
    assert 1.0 < worst <= 1.0 + 2 * 2.0 ** -23


# ---- the new exports refuse bad arguments before any launch -----------------------------------------------------
def test_new_kernels_validate_arguments_without_gpu():
    from dsic_amd import lib
    L = lib.load()
    one = 16
    assert L.dsic_tile_gather_u8_ov(None, None, 150, 200, 3, 64, 64, 16, 0, 1, None) == 1
    assert b"null" in L.dsic_last_error()
    assert L.dsic_tile_gather_u8_ov(one, one, 150, 200, 5, 64, 64, 16, 0, 1, None) == 1          # C
    assert L.dsic_tile_gather_u8_ov(one, one, 150, 200, 3, 64, 64, 24, 0, 1, None) == 1          # not a multiple of 16
    assert b"overlap" in L.dsic_last_error()
    assert L.dsic_tile_gather_f32_ov(one, one, 150, 200, 3, 64, 64, 48, 0, 1, None) == 1         # over half a tile
    assert b"overlap" in L.dsic_last_error()
    assert L.dsic_tile_gather_f32_ov(one, one, 150, 200, 3, 64, 64, -16, 0, 1, None) == 1
    assert L.dsic_tile_gather_f32_ov(one, one, 150, 200, 3, 64, 64, 16, 10, 3, None) == 1        # tiles 10..12 of 12
    assert b"outside the grid" in L.dsic_last_error()
    assert L.dsic_tile_gather_f32_ov(one, one, 128, 128, 3, 64, 64, 0, 3, 2, None) == 1          # 4 tiles at overlap 0
    assert b"outside the grid of 4" in L.dsic_last_error()
    assert L.dsic_tile_gather_f32_ov(one, one, 128, 128, 3, 64, 64, 16, 8, 2, None) == 1         # 9 at overlap 16
    assert b"outside the grid of 9" in L.dsic_last_error()
    assert L.dsic_tile_gather_f32_ov(None, one, 150, 200, 3, 64, 64, 16, 0, 1, None) == 1

    def blend(tiles=one, ids=one, n=1, canvas=one, H=150, W=200, C=3, th=64, tw=64, O=16, win=(0, 0, 150, 200)):
        return L.dsic_tile_blend_window_f32(tiles, ids, n, canvas, H, W, C, th, tw, O, *win, None)

    for kw, word in (({"tiles": None}, b"null"), ({"ids": None}, b"null"), ({"canvas": None}, b"null"),
                     ({"C": 0}, b"C="), ({"C": 9}, b"C="), ({"O": 8}, b"overlap"), ({"O": 48}, b"overlap"),
                     ({"O": -16}, b"overlap"), ({"th": 48, "O": 32}, b"overlap"), ({"th": 40}, b"multiples of 16"),
                     ({"win": (0, 0, 151, 200)}, b"window"), ({"win": (0, 1, 150, 200)}, b"window"),
                     ({"win": (-1, 0, 4, 4)}, b"window"), ({"win": (3, 3, 0, 4)}, b"window"),
                     ({"n": 0}, b"tiles per call"), ({"n": 65}, b"tiles per call"), ({"canvas": 20}, b"aligned")):
        assert blend(**kw) == 1, kw
        assert word in L.dsic_last_error(), (kw, L.dsic_last_error())
    assert L.dsic_tile_blend_finish_f32(None, 3, 10, 10, None) == 1
    assert b"null" in L.dsic_last_error()
    assert L.dsic_tile_blend_finish_f32(one, 9, 10, 10, None) == 1
    assert L.dsic_tile_blend_finish_f32(one, 3, 0, 10, None) == 1
    assert L.dsic_tile_blend_finish_f32(20, 3, 10, 10, None) == 1
    assert L.dsic_tile_blend_finish_u8(one, None, 3, 10, 10, None) == 1
    assert L.dsic_tile_blend_finish_u8(one, one, 5, 10, 10, None) == 1
    assert b"C=" in L.dsic_last_error()
    assert L.dsic_tile_blend_finish_u8(one, one, 3, 10, 0, None) == 1
    assert L.dsic_tile_blend_finish_u8(one, 24, 3, 10, 10, None) == 1
    assert L.dsic_abi_version() == 4


def test_header_declares_the_new_exports():
    import os
    import re
    from dsic_amd import lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "dsic_hip.h")).read()
    declared = set(re.findall(r"\b(dsic_\w+)\s*\(", header))
    new = {"dsic_tile_gather_u8_ov", "dsic_tile_gather_f32_ov", "dsic_tile_blend_window_f32",
           "dsic_tile_blend_finish_f32", "dsic_tile_blend_finish_u8"}
    assert new <= declared and new <= set(lib.SIGNATURES)
    L = lib.load()
    for name in new:
        assert getattr(L, name) is not None
