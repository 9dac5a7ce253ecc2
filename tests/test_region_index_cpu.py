"""CPU-only: the stream index of the region decoder (offsets of every tile's strings from the heads alone), the
window -> tiles rule against a painted ownership map, the byte spans of a tile selection, the refusals, and the
argument checks of the region decoder's kernels."""
import io
import random
import struct

import numpy as np
import pytest

from dsic_amd import codec, entropy

TAG = 0x40302
N, M = 128, 192
# H, W, tile, batch
GRIDS = [(600, 1000, 256, 5), (120, 100, 256, 64), (300, 530, 128, 7)]


def _build(H, W, tile, batch, seed=0, tag=TAG, container_tags=None):
    """A DSICI stream in pure Python with made-up strings (some empty) -> (stream, grid, strings per tile, records)."""
    rng = random.Random(seed)
    g = codec.tile_grid(H, W, tile)
    strings, recs, blobs = [], [], []
    for k, first in enumerate(range(0, g["n"], batch)):
        B = min(batch, g["n"] - first)
        comp = {"strings": [], "shape_y": [B, M, g["th"] // 16, g["tw"] // 16],
                "shape_z": [B, N, g["th"] // 64, g["tw"] // 64], "min_y": [], "max_y": [], "min_z": [], "max_z": [],
                "numerics": tag if container_tags is None else container_tags[k]}
        for b in range(B):
            zl = rng.choice([0, 1, 3, 16, 17, 40, 100])
            yl = rng.choice([0, 1, 15, 16, 33, 250, 1000])
            comp["strings"].append([bytes(rng.getrandbits(8) for _ in range(zl)),
                                    bytes(rng.getrandbits(8) for _ in range(yl))])
            lo_y, lo_z = rng.randint(-40, -1), rng.randint(-9, -1)
            comp["min_y"].append(lo_y), comp["max_y"].append(lo_y + rng.randint(1, 80))
            comp["min_z"].append(lo_z), comp["max_z"].append(lo_z + rng.randint(1, 20))
            recs.append((k, b, comp["min_y"][-1], comp["max_y"][-1], comp["min_z"][-1], comp["max_z"][-1]))
        strings += comp["strings"]
        blobs.append(entropy.pack_container(comp))
    header = {"numerics": tag, "H": H, "W": W, "C": 3, "kind": 0, "th": g["th"], "tw": g["tw"], "N": N, "M": M,
              "in_ch": 3, "spatial_params": 0, "batch": batch}
    return codec.pack_image_stream(header, blobs), g, strings, recs


class Counting:
    """A binary file object that counts the bytes read through it."""

    def __init__(self, data):
        self.f, self.count, self.reads = io.BytesIO(data), 0, []

    def seek(self, *a):
        return self.f.seek(*a)

    def tell(self):
        return self.f.tell()

    def read(self, n=-1):
        pos = self.f.tell()
        out = self.f.read(n)
        self.count += len(out)
        self.reads.append((pos, len(out)))
        return out


@pytest.mark.parametrize("H,W,tile,batch", GRIDS)
def test_index_slices_the_stream_to_the_strings(H, W, tile, batch):
    stream, g, strings, recs = _build(H, W, tile, batch, seed=H)
    ix = codec.stream_index(stream)
    u = codec.unpack_image_stream(stream)
    for key in ("version", "numerics", "H", "W", "C", "kind", "th", "tw", "N", "M", "in_ch", "spatial_params", "batch",
                "batches"):
        assert ix[key] == u[key], key
    assert "blobs" not in ix
    for key in ("H", "W", "Hp", "Wp", "th", "tw", "ny", "nx", "n", "ys", "xs", "own_y", "own_x"):
        assert ix["grid"][key] == g[key], key
    assert len(ix["tiles"]) == g["n"] == len(strings)
    for t, r in enumerate(ix["tiles"]):
        assert (r["k"], r["b"]) == divmod(t, batch)
        assert (r["k"], r["b"], r["min_y"], r["max_y"], r["min_z"], r["max_z"]) == recs[t]
        assert stream[r["z_off"]:r["z_off"] + r["z_len"]] == strings[t][0], t
        assert stream[r["y_off"]:r["y_off"] + r["y_len"]] == strings[t][1], t
    assert ix["stream_bytes"] == len(stream)
    # the same index from a file object, a bytearray and a memoryview, and only the heads are read
    f = Counting(stream)
    from_file = codec.stream_index(f)
    assert from_file == ix
    Bs = [min(batch, g["n"] - first) for first in range(0, g["n"], batch)]
    assert f.count == 60 + sum(8 + 38 + 24 * B for B in Bs) == ix["index_bytes"]
    assert codec.stream_index(io.BytesIO(stream)) == ix
    assert codec.stream_index(bytearray(stream)) == ix and codec.stream_index(memoryview(stream)) == ix
    assert [c["tiles"] for c in ix["containers"]] == Bs
    assert [stream[c["offset"]:c["offset"] + c["bytes"]] for c in ix["containers"]] == u["blobs"]


def _owner_map(g):
    m = np.full((g["Hp"], g["Wp"]), -1, dtype=np.int64)
    for i, (a, b) in enumerate(g["own_y"]):
        for j, (c, d) in enumerate(g["own_x"]):
            assert (m[a:b, c:d] == -1).all()
            m[a:b, c:d] = i * g["nx"] + j
    assert (m >= 0).all()
    return m[:g["H"], :g["W"]]


@pytest.mark.parametrize("H,W,tile,batch", GRIDS)
def test_window_tiles_against_the_painted_map(H, W, tile, batch):
    g = codec.tile_grid(H, W, tile)
    ix = codec.stream_index(_build(H, W, tile, batch)[0])
    owner = _owner_map(g)
    rng = random.Random(7 * H + W)
    windows = [(0, 0, 1, 1), (0, W - 1, 1, 1), (H - 1, 0, 1, 1), (H - 1, W - 1, 1, 1), (0, 0, H, W)]
    for (a, b) in g["own_y"]:                       # windows that end on, start on and straddle an ownership boundary
        for (c, d) in g["own_x"]:
            b_, d_ = min(b, H), min(d, W)
            windows += [(a, c, b_ - a, d_ - c), (a, c, 1, 1), (b_ - 1, d_ - 1, 1, 1)]
            if b_ < H and d_ < W:
                windows += [(b_ - 1, d_ - 1, 2, 2), (b_, d_, 1, 1)]
    if H == 600:
        windows += [(352, 0, 160, W), (360, 100, 100, 300), (352, 255, 160, 2), (400, 3, 150, 777), (511, 255, 2, 2)]
    for _ in range(300):
        y0, x0 = rng.randrange(H), rng.randrange(W)
        windows.append((y0, x0, rng.randint(1, H - y0), rng.randint(1, W - x0)))
    for y0, x0, h, w in windows:
        want = np.unique(owner[y0:y0 + h, x0:x0 + w]).tolist()
        assert codec.window_tiles(g, y0, x0, h, w) == want, (y0, x0, h, w)
        assert codec.window_tiles(ix, y0, x0, h, w) == want, (y0, x0, h, w)
    if H == 600:   # rows 352..511 lie in both tile rows 1 and 2 and are owned by row 1
        assert codec.window_tiles(g, 352, 0, 160, W) == [4, 5, 6, 7]
        assert codec.window_tiles(g, 200, 700, 360, 300) == [2, 3, 6, 7, 10, 11]


@pytest.mark.parametrize("y0,x0,h,w", [(-1, 0, 5, 5), (0, -1, 5, 5), (0, 0, 0, 5), (0, 0, 5, 0), (0, 0, 601, 5),
                                       (0, 0, 5, 1001), (599, 999, 2, 1), (599, 999, 1, 2), (600, 0, 1, 1),
                                       (10, 10, -3, 4)])
def test_window_refusals(y0, x0, h, w):
    g = codec.tile_grid(600, 1000, 256)
    with pytest.raises(ValueError, match="window"):
        codec.window_tiles(g, y0, x0, h, w)


@pytest.mark.parametrize("H,W,tile,batch", GRIDS)
def test_tile_spans(H, W, tile, batch):
    stream, g, strings, _ = _build(H, W, tile, batch, seed=3)
    ix = codec.stream_index(stream)
    rng = random.Random(11)
    picks = [list(range(g["n"])), [0], [g["n"] - 1]] + [sorted(rng.sample(range(g["n"]), rng.randint(1, g["n"])))
                                                       for _ in range(50)]
    for tiles in picks:
        spans = codec.tile_spans(ix, tiles)
        want = sum(len(strings[t][0]) + len(strings[t][1]) for t in tiles)
        assert sum(n for _, n in spans) == want
        assert all(n > 0 for _, n in spans)
        for (a, n), (b, _) in zip(spans, spans[1:]):
            assert a + n < b                                        # ascending, apart, and merged where they touch
        assert b"".join(stream[a:a + n] for a, n in spans) == b"".join(strings[t][0] + strings[t][1] for t in tiles)
    # all tiles of one container: its strings are one run of bytes
    for c in ix["containers"]:
        tiles = list(range(c["first"], c["first"] + c["tiles"]))
        spans = codec.tile_spans(ix, tiles)
        body = c["bytes"] - 38 - 24 * c["tiles"]
        assert spans == ([(c["offset"] + 38 + 24 * c["tiles"], body)] if body else [])


def test_refusals():
    stream, g, _, _ = _build(600, 1000, 256, 5, seed=5)
    ix = codec.stream_index(stream)
    with pytest.raises(ValueError, match="not a DSICI"):
        codec.stream_index(b"DSICX\x00" + stream[6:])
    with pytest.raises(ValueError, match="not a DSICI"):
        codec.stream_index(b"garbage")
    c0 = ix["containers"][0]["offset"]
    c1 = ix["containers"][1]["offset"]
    cuts = (1, 5, 30, 59, 60, 66, c0 + 10, c0 + 38, c0 + 38 + 24 + 7, ix["tiles"][2]["y_off"], c1 - 8 + 3, c1 + 50,
            len(stream) - 1)
    for cut in cuts:
        for src in (stream[:cut], io.BytesIO(stream[:cut])):
            with pytest.raises(ValueError, match="truncated"):
                codec.stream_index(src)
    with pytest.raises(ValueError, match="trailing"):
        codec.stream_index(stream + b"\x00")
    with pytest.raises(ValueError, match="version"):
        codec.stream_index(stream[:6] + struct.pack("<H", 99) + stream[8:])
    with pytest.raises(ValueError, match="DSIC1"):
        codec.stream_index(stream[:c0] + b"DSIC1\x00" + stream[c0 + 6:])
    with pytest.raises(ValueError, match="not a DSIC container"):
        codec.stream_index(stream[:c1] + b"DSIC9\x00" + stream[c1 + 6:])
    # a record whose length does not add up to the container's size
    rec_len = c0 + 38 + 16
    (zl,) = struct.unpack_from("<I", stream, rec_len)
    with pytest.raises(ValueError, match="truncated or oversized"):
        codec.stream_index(stream[:rec_len] + struct.pack("<I", zl + 1) + stream[rec_len + 4:])
    # a container written under another numerics tag than the stream's
    odd, _, _, _ = _build(600, 1000, 256, 5, seed=5, container_tags=[TAG, TAG ^ 0x100, TAG])
    with pytest.raises(ValueError, match="batch 1 carries numerics tag"):
        codec.stream_index(odd)
    # ... and both decoders refuse it the same way, from the index, before they touch the model
    with pytest.raises(ValueError, match="batch 1 carries numerics tag"):
        codec.decompress_image(None, odd)
    with pytest.raises(ValueError, match="batch 1 carries numerics tag"):
        codec.decompress_region(None, odd, 0, 0, 8, 8)
    # batches versus grid: a dropped batch, a batch size that needs four batches, batches in the wrong places
    u = codec.unpack_image_stream(stream)
    head = {k: u[k] for k in ("numerics", "H", "W", "C", "kind", "th", "tw", "N", "M", "in_ch", "spatial_params",
                              "batch")}
    with pytest.raises(ValueError, match="batches"):
        codec.stream_index(codec.pack_image_stream(head, u["blobs"][:2]))
    with pytest.raises(ValueError, match="batches"):
        codec.stream_index(codec.pack_image_stream(dict(head, batch=3), u["blobs"]))
    with pytest.raises(ValueError, match="holds 5 latents"):
        codec.stream_index(codec.pack_image_stream(dict(head, batch=4), u["blobs"]))
    with pytest.raises(ValueError, match="holds 2 latents"):
        codec.stream_index(codec.pack_image_stream(head, [u["blobs"][0], u["blobs"][2], u["blobs"][2]]))
    with pytest.raises(ValueError, match="latents of 16x16, expected 14 of 8x8"):       # latent shape versus tile size
        codec.stream_index(codec.pack_image_stream(dict(head, th=128, tw=128, batch=14), u["blobs"]))
    with pytest.raises(ValueError, match="tile"):
        codec.stream_index(codec.pack_image_stream(dict(head, th=100), u["blobs"]))
    with pytest.raises(ValueError, match="inconsistent"):
        codec.stream_index(codec.pack_image_stream(dict(head, C=4), u["blobs"]))
    with pytest.raises(TypeError):
        codec.stream_index("a path is not a stream")
    # windows outside the image or empty, through the index
    for win in ((0, 0, 601, 1), (0, 990, 5, 11), (5, 5, 0, 1), (-1, 0, 2, 2)):
        with pytest.raises(ValueError, match="window"):
            codec.window_tiles(ix, *win)


def test_region_kernel_argument_validation_without_gpu():
    from dsic_amd import lib
    L = lib.load()
    one = 16   # any non-null, 16-byte aligned address: every call below is refused before a launch
    for fn, C in ((L.dsic_tile_stitch_window_f32, 3), (L.dsic_tile_stitch_window_u8, 3)):
        assert fn(None, one, 1, one, 600, 1000, C, 256, 256, 0, 0, 10, 10, None) == 1
        assert b"null" in L.dsic_last_error()
        assert fn(one, None, 1, one, 600, 1000, C, 256, 256, 0, 0, 10, 10, None) == 1
        assert fn(one, one, 1, None, 600, 1000, C, 256, 256, 0, 0, 10, 10, None) == 1
        assert fn(one, one, 1, one, 600, 1000, 9 if fn is L.dsic_tile_stitch_window_f32 else 5, 256, 256, 0, 0, 10,
                  10, None) == 1
        assert b"C=" in L.dsic_last_error()
        assert fn(one, one, 1, one, 600, 1000, C, 250, 256, 0, 0, 10, 10, None) == 1        # tile not a multiple of 16
        assert fn(one, one, 1, one, 600, 1000, C, 256, 256, 595, 0, 10, 10, None) == 1      # rows 595..604 of 600
        assert b"outside" in L.dsic_last_error()
        assert fn(one, one, 1, one, 600, 1000, C, 256, 256, 0, 995, 10, 10, None) == 1
        assert fn(one, one, 1, one, 600, 1000, C, 256, 256, -1, 0, 10, 10, None) == 1
        assert fn(one, one, 1, one, 600, 1000, C, 256, 256, 0, 0, 0, 10, None) == 1         # empty window
        assert fn(one, one, 0, one, 600, 1000, C, 256, 256, 0, 0, 10, 10, None) == 1        # n = 0
        assert b"n=0" in L.dsic_last_error()
        assert fn(one, one, 65536, one, 600, 1000, C, 256, 256, 0, 0, 10, 10, None) == 1
        assert fn(one, one, 1, one + 4, 600, 1000, C, 256, 256, 0, 0, 10, 10, None) == 1    # misaligned out
        assert b"aligned" in L.dsic_last_error()
    assert L.dsic_tile_stitch_window_u8(one, one, 1, one, 600, 1000, 5, 256, 256, 0, 0, 10, 10, None) == 1   # C = 5
    sel = L.dsic_strings_scatter_select
    assert sel(None, 64, one, 1, 8, one, 8, one, 8, one, None) == 1
    assert b"null" in L.dsic_last_error()
    assert sel(one, 64, None, 1, 8, one, 8, one, 8, one, None) == 1
    assert sel(one, 64, one, 1, 8, one, 8, one, 8, None, None) == 1
    assert sel(one, 64, one, 0, 8, one, 8, one, 8, one, None) == 1                          # n = 0
    assert b"n=0" in L.dsic_last_error()
    assert sel(one, 64, one, 40000, 8, one, 8, one, 8, one, None) == 1
    assert sel(one, 64, one, 1, 8, one, 6, one, 8, one, None) == 1                          # stride
    assert sel(one, 64, one, 1, 8, one, 8, one, 0, one, None) == 1
    assert sel(one, -1, one, 1, 8, one, 8, one, 8, one, None) == 1
    assert sel(one + 4, 64, one, 1, 8, one, 8, one, 8, one, None) == 1                      # misaligned blob
    assert b"aligned" in L.dsic_last_error()
