"""CPU-only: tests/codec_ref.py, the restatement the byte-mover kernels are held to, checked against the package's
pure-Python geometry and container code and against itself, so that the GPU test does not compare the kernels with a
wrong reference.  The library is not loaded."""
import itertools

import numpy as np
import pytest

import codec_ref as R
from dsic_amd import codec, entropy
from test_image_codec_cpu import SIZES, TILES


@pytest.mark.parametrize("tile", TILES)
def test_grid_equals_tile_grid(tile):
    for H, W in itertools.product(SIZES, SIZES):
        g = codec.tile_grid(H, W, tile)
        r = R.grid(H, W, min(tile, R.ceil16(H)), min(tile, R.ceil16(W)))
        for k in ("Hp", "Wp", "th", "tw", "ny", "nx", "n", "ys", "xs"):
            assert r[k] == g[k], (H, W, k)
        assert [tuple(o) for o in g["own_y"]] == r["own_y"] and [tuple(o) for o in g["own_x"]] == r["own_x"]


GEOMETRIES = [(17, 33, 32), (33, 35, 32), (40, 34, 32), (64, 36, 32), (50, 100, 48)]


@pytest.mark.parametrize("H,W,tile", GEOMETRIES)
@pytest.mark.parametrize("C", [1, 3, 4, 8])
def test_stitch_of_gather_is_the_image(H, W, tile, C):
    rng = np.random.default_rng(H * 1000 + W + C)
    g = R.grid(H, W, tile, tile)
    ids = list(range(g["n"]))
    u8 = rng.integers(0, 256, size=(H, W, C), dtype=np.uint8)
    f32 = (u8.transpose(2, 0, 1).astype(np.float32) / np.float32(255)).astype(np.float32)       # values k/255
    tiles_u8 = R.gather_u8(u8, tile, tile)
    tiles_f32 = R.gather_f32(f32, tile, tile)
    assert tiles_u8.shape == (g["n"], tile, tile, C) and tiles_f32.shape == (g["n"], C, tile, tile)
    # the two gathers are one indexing rule
    assert np.array_equal(tiles_u8.transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255), tiles_f32)
    # reflected rows and columns: padded position p reads 2*(L-1) - p
    if H < tile:
        assert np.array_equal(tiles_f32[0][:, H, :min(W, tile)], f32[:, H - 2, :min(W, tile)])
    if W % 16:
        last = g["nx"] - 1
        assert np.array_equal(tiles_u8[last][:min(H, tile), W - g["xs"][last]], u8[:min(H, tile), W - 2])
    back = R.stitch(tiles_f32, ids, H, W, tile, tile, (0, 0, H, W), "f32", np.float32(-3))
    assert back.dtype == np.float32 and np.array_equal(back, f32)
    # k/255 * 255 truncates to k in float32 for every k, so the uint8 stitch of the float tiles is the uint8 image
    back = R.stitch(tiles_f32, ids, H, W, tile, tile, (0, 0, H, W), "u8", 7)
    assert back.dtype == np.uint8 and np.array_equal(back, u8)
    # a window, tiles in another order, one left out, foreign and repeated numbers
    win = (1, 1, H - 2, W - 3)
    order = ids[::-1] + [-1, g["n"], ids[0]]
    t2 = np.stack([tiles_f32[t] if 0 <= t < g["n"] else np.full_like(tiles_f32[0], 0.5) for t in order])
    got = R.stitch(t2, order, H, W, tile, tile, win, "f32", np.float32(-3))
    assert np.array_equal(got, f32[:, 1:H - 1, 1:W - 2])
    got = R.stitch(tiles_f32[1:], ids[1:], H, W, tile, tile, (0, 0, H, W), "f32", np.float32(-3))
    oy, ox = g["own_y"][0], g["own_x"][0]
    hole = np.zeros((C, H, W), dtype=bool)
    hole[:, oy[0]:min(oy[1], H), ox[0]:min(ox[1], W)] = True
    assert np.array_equal(got == -3, hole) and np.array_equal(got[~hole], f32[~hole])


def test_clamp_and_truncation():
    x = np.float32([-0.5, -0.0, 0.0, 1.0, np.nextafter(np.float32(1), np.float32(2)), 2.0, 0.999999])
    c = R.clamp01(x)
    assert c.tobytes() == np.float32([0.0, -0.0, 0.0, 1.0, 1.0, 1.0, 0.999999]).tobytes()
    assert R.to_u8(x).tolist() == [0, 0, 0, 255, 255, 255, 254]


def _batch(B, K, seed, cap_z=8, cap_y=36):
    rng = np.random.default_rng(seed)
    rows = rng.integers(1, 256, size=(B, cap_z + K * cap_y), dtype=np.uint8)
    lengths = np.concatenate([rng.integers(0, cap_z + 1, size=(B, 1)), rng.integers(0, cap_y + 1, size=(B, K))], 1)
    lengths[0] = [cap_z] + [cap_y] * K
    lengths[-1, -1] = 0
    meta = np.stack([rng.integers(-40, 1, B), rng.integers(1, 90, B), rng.integers(-9, 1, B), rng.integers(1, 20, B)],
                    1).astype(np.int32)
    return rows, lengths.astype(np.int32), meta


def _as_dict(rows, lengths, meta, tag, shape, cap_z, cap_y, K):
    B = rows.shape[0]
    My, Hy, Wy, Nz, Hz, Wz = shape
    strings = []
    for b in range(B):
        segs = [rows[b, cap_z + j * cap_y:cap_z + j * cap_y + lengths[b, 1 + j]].tobytes() for j in range(K)]
        strings.append([rows[b, :lengths[b, 0]].tobytes(), b"".join(segs)])
    d = {"strings": strings, "shape_y": [B, My, Hy, Wy], "shape_z": [B, Nz, Hz, Wz], "numerics": tag,
         "min_y": [int(m[0]) for m in meta], "max_y": [int(m[0] + m[1] - 1) for m in meta],
         "min_z": [int(m[2]) for m in meta], "max_z": [int(m[2] + m[3] - 1) for m in meta]}
    if K > 1:
        d["segments"] = K
        d["seg_lengths_y"] = [[int(v) for v in lengths[b, 1:]] for b in range(B)]
    return d


@pytest.mark.parametrize("B", [1, 3, 40])
@pytest.mark.parametrize("K", [1, 2, 16])
def test_pack_container_equals_the_package_and_unpacks(B, K):
    cap_z, cap_y, tag = 8, 36, 0xDEADBEEF
    shape = (16 * K, 4, 6, 5, 1, 2)
    rows, lengths, meta = _batch(B, K, seed=B * 31 + K)
    blob, total, offsets = R.pack_container(rows, lengths, meta, tag, *shape, cap_z, cap_y, K)
    d = _as_dict(rows, lengths, meta, tag, shape, cap_z, cap_y, K)
    assert blob == entropy.pack_container(d)
    assert total == len(blob) and len(offsets) == B * (1 + K) + 1
    assert offsets == [0] + np.cumsum(lengths.ravel()).tolist()
    u = entropy.unpack_container(blob)
    for k, v in d.items():
        assert u[k] == v, k


def test_pack_container_clamps_lengths():
    cap_z, cap_y, K = 8, 36, 2
    rows, lengths, meta = _batch(3, K, seed=5)
    forged = lengths.copy()
    forged[0] = [-1, cap_y + 1, 2 ** 31 - 1]
    forged[1, 0] = cap_z + 1
    cut = forged.copy()
    cut[0] = [0, cap_y, cap_y]
    cut[1, 0] = cap_z
    args = (meta, 1, 32, 4, 6, 5, 1, 2, cap_z, cap_y, K)
    assert R.pack_container(rows, forged, *args) == R.pack_container(rows, cut, *args)


@pytest.mark.parametrize("B", [1, 3, 40])
def test_scatter_of_pack_returns_the_rows(B):
    cap_z, cap_y, fill = 8, 36, 0xA5
    rows, lengths, meta = _batch(B, 1, seed=B)
    blob, total, offsets = R.pack_container(rows, lengths, meta, 9, 16, 4, 6, 5, 1, 2, cap_z, cap_y, 1)
    host = np.zeros(R.ceil16(total) + 16, dtype=np.uint8)
    host[:total] = np.frombuffer(blob, dtype=np.uint8)
    z, y, got_len, got_meta = R.scatter(host, total, B, cap_z, cap_y, fill)
    assert np.array_equal(got_len, lengths) and np.array_equal(got_meta, meta)
    base = R.HEAD_BYTES + R.REC_BYTES * B
    desc = np.array([[base + offsets[2 * b], lengths[b, 0], base + offsets[2 * b + 1], lengths[b, 1]]
                     for b in range(B)], dtype=np.int64)
    z2, y2, len2 = R.scatter_select(host, total, desc, cap_z, cap_y, fill)
    assert np.array_equal(z, z2) and np.array_equal(y, y2) and np.array_equal(len2, lengths)
    for b in range(B):
        nz, ny = lengths[b]
        assert np.array_equal(z[b, :nz], rows[b, :nz]) and (z[b, nz:] == fill).all()
        assert np.array_equal(y[b, :ny], rows[b, cap_z:cap_z + ny]) and (y[b, ny:] == fill).all()


def test_scatter_cuts_forged_descriptors():
    fill = 0xA5
    blob = np.arange(1, 65, dtype=np.uint8)
    desc = [[0, 9, 60, 9],          # over the z stride; past the blob
            [-4, 4, 64, 4],         # offsets outside / at the end
            [65, 4, 3, -2]]         # offset past the end; negative length
    z, y, lengths = R.scatter_select(blob, 64, desc, 8, 12, fill)
    assert lengths.tolist() == [[8, 4], [0, 0], [0, 0]]
    assert z[0].tolist() == list(range(1, 9)) and y[0].tolist() == [61, 62, 63, 64] + [fill] * 8
    assert (z[1:] == fill).all() and (y[1:] == fill).all()
