"""The closed-form scenes of big_scene.py and the banded restatements of big_ref.py, held to their conditions on the host.

(a) torch on the CPU and NumPy evaluate the same bytes.
(b) For every geometry of the large-image tests the pattern differs from itself read 2^31 or 2^32 elements or bytes
    earlier at 99 % of 10^5 sampled positions at least, so an offset that wraps cannot return the right sample by
    chance.  The validity plane holds two classes only (zero, non-zero); what a kernel takes from it is the class, and
    the classes of two positions 2^31 apart must differ at a quarter of the sampled positions at least.  A wrapped
    offset misreads whole rows, thousands of pixels at a time, so a quarter of them is far more than a comparison bit
    for bit needs; the bytes themselves differ at three quarters at least.  The 99 % hold for the formula itself.  The
    scenes that plant a nodata value repeat it over about 0.27 of their pixels; with the plants in, two positions a
    wrap apart are equal only where both are planted or the samples collide, so they must still differ at 90 % of
    the positions (1 - 0.27^2 - 1/256 is 0.92), which is asserted too.
(c) On the small geometries of the GPU tests every banded restatement equals the same part of the full restatement,
    for every tile row, band of rows and window it can be asked for, the image's last rows among them (reflected rows,
    the last tile row shifted inward).
(d) The same for the viewing path (test_gpu_big_views.py): the banded warps, index views and composites equal the full
    restatements; every view and window that module uses on the big scenes (big_views.py, which both files import)
    gives another expected output when its taps or its validity bytes are read a wrap earlier; and the sizes its tests
    lean on hold: outputs under 2^31 pixels for the composites, past 2^32 bytes and 2^20 workgroups for the writers.
"""
import numpy as np
import pytest
import torch

import big_ref as B
import big_scene as S
import blend_ref
import codec_ref
import mask_ref
import pyramid_ref
import render_ref
import u16_ref
import valid_ref
import view_ref as V

GEOMETRIES = [(17, 33, 32), (33, 35, 32), (40, 34, 32), (64, 36, 32), (50, 100, 48)]     # test_gpu_codec_movers.py
SIZES = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 5), (17, 33), (33, 35), (40, 34), (64, 36), (50, 100), (70, 1030)]
KINDS = [("u8", 3), ("u16", 4), ("f32", 3)]
SCALE = [(20000, 40000), (1, 65534), (30000, 30001), (0, 65535)]
DT = {"u8": np.uint8, "u16": np.uint16, "f32": np.float32}


def test_the_geometry_lists_are_those_of_the_gpu_tests():
    import test_gpu_codec_movers
    import test_gpu_pyramid
    assert GEOMETRIES == test_gpu_codec_movers.GEOMETRIES and SIZES == test_gpu_pyramid.SIZES
    import big_views
    import test_gpu_big_views
    assert test_gpu_big_views.G is big_views and (test_gpu_big_views.CMAP == CMAP).all()


# ---- (a) ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,C", [("u8", 1), ("u8", 3), ("u8", 4), ("u16", 1), ("u16", 4), ("f32", 1), ("f32", 3)])
@pytest.mark.parametrize("H,W", [(1, 1), (17, 33), (70, 1030)])
def test_torch_and_numpy_evaluate_the_same_bytes(kind, C, H, W):
    plants = ((H - 1, W - 1, C - 1, 3),) + (((0, 0, 0, 250),) if H > 1 else ())
    for nodata in ((None,) if kind == "f32" else (None, 7)):
        scene = S.Scene("t", kind, H, W, C, valid=True, nodata=nodata, plants=plants)
        ys = np.r_[np.arange(H), [H - 1, 0]]
        a, b = scene.rows(S.NP, ys), scene.rows(S.torch_namespace("cpu"), ys).numpy()
        assert a.dtype == DT[kind] and a.shape == scene.shape(len(ys)) and a.tobytes() == b.tobytes()
        va, vb = scene.valid_rows(S.NP, ys), scene.valid_rows(S.torch_namespace("cpu"), ys).numpy()
        assert va.dtype == np.uint8 and va.shape == (len(ys), W) and va.tobytes() == vb.tobytes()
        # the block-wise fill writes the same image
        img = torch.zeros(scene.shape(), dtype=torch.int16 if kind == "u16" else getattr(torch, a.dtype.name))
        val = torch.zeros((H, W), dtype=torch.uint8)
        scene.fill(S.torch_namespace("cpu"), img, val)
        assert img.numpy().tobytes() == scene.band(0, H).tobytes() and val.numpy().tobytes() == scene.valid_band(0, H).tobytes()
        px = a if kind != "f32" else a.transpose(1, 2, 0)
        assert px[-2, -1, C - 1] == (3 if kind != "f32" else np.float32(3) / np.float32(1 << 24))


def test_the_scene_holds_what_the_tests_need():
    scene = S.Scene("t", "u8", 640, 1030, 3, valid=True, nodata=7)
    img, val = scene.band(0, 640), scene.valid_band(0, 640)
    nd = mask_ref.nodata_mask(img, 7)
    for mask in (nd, val == 0):
        counts = mask_ref.counts(mask, 640, 1030, 32, 32)
        full = sum(1 for c, t in zip(counts, mask_ref.tiles(640, 1030, 32, 32)) if c == (t[3] - t[2]) * (t[5] - t[4]))
        assert full >= 20 and counts.count(0) >= 20 and sum(1 for c in counts if 0 < c < 1024) >= 20
    assert set(np.unique(img)) == set(range(256))
    u16 = S.Scene("t", "u16", 64, 1030, 4).band(0, 64)
    assert u16.min() >= S.U16_LO and u16.max() < S.U16_LO + S.U16_SPAN
    f32 = S.Scene("t", "f32", 64, 1030, 3).band(0, 64)
    assert f32.min() >= 0 and f32.max() < 1 and len(np.unique(f32)) > 190000


# ---- (b) ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(S.table()))
def test_the_pattern_differs_from_itself_a_wrap_earlier(name):
    scene = S.table(bands=False)[name]
    rng = np.random.default_rng(len(name))
    if scene.nodata is not None:                                              # with the planted rectangles in
        for what, e in scene.crossings().items():
            pos = rng.integers(e, scene.elements, 100000)
            a, b = scene.coords(pos), scene.coords(pos - e)
            va = np.where(S.nodata_class(a[0], a[1]) == 0, scene.nodata, S.value(*a, scene.kind))
            vb = np.where(S.nodata_class(b[0], b[1]) == 0, scene.nodata, S.value(*b, scene.kind))
            assert float((va != vb).mean()) >= 0.90, (name, what)
    scene.nodata = None                                                       # planted rectangles only repeat the value
    for what, e in scene.crossings().items():
        pos = rng.integers(e, scene.elements, 100000)
        differ = float((scene.at(pos) != scene.at(pos - e)).mean())
        assert differ >= 0.99, (name, what, differ)
    if name in ("u8c3", "u8c1v", "u16c4", "f32c3"):
        assert scene.crossings(), name
    pixels = scene.H * scene.W
    if scene.valid and pixels > 1 << 31:
        pos = rng.integers(1 << 31, pixels, 100000)
        a = S.validity(*np.divmod(pos, scene.W))
        b = S.validity(*np.divmod(pos - (1 << 31), scene.W))
        assert float((a != b).mean()) >= 0.75 and float(((a == 0) != (b == 0)).mean()) >= 0.25


def test_the_table_crosses_what_it_names():
    t = S.table()
    assert t["u8c3"].nbytes > 1 << 32 and t["u8c1v"].H * t["u8c1v"].W > 1 << 31
    assert t["u16c4"].elements > 1 << 31 and t["u16c4"].nbytes > 1 << 32
    f = t["f32c3"]
    assert f.elements > 1 << 31 and f.nbytes > 1 << 32 and 2 * f.H * f.W < 1 << 31 < 3 * f.H * f.W   # inside plane 2
    assert f.H * f.W < 1 << 30 < 2 * f.H * f.W                                 # 2^32 bytes: inside plane 1
    for s in t.values():
        assert s.H % 16 and s.W % 16
    g = codec_ref.grid(8209, 8209, 32, 32)
    assert g["n"] == 66049


# ---- (c) ------------------------------------------------------------------------------------------------------------
def _small(kind, C, H, W):
    rng = np.random.default_rng(H * 1009 + W * 17 + C)
    if kind == "f32":
        img = rng.random((C, H, W), dtype=np.float32)
    else:
        img = rng.integers(0, 256 if kind == "u8" else 65536, size=(H, W, C)).astype(DT[kind])
        img[rng.random((H, W)) < 0.3] = 7
    valid = rng.random((H, W)) < 0.6
    valid[:H // 2, :W // 3] = False
    return img, valid


def _tileable(H, W, t):
    return t <= codec_ref.ceil16(H) and t <= codec_ref.ceil16(W) and codec_ref.ceil16(H) - H < H and \
        codec_ref.ceil16(W) - W < W


CASES = GEOMETRIES + [(H, W, 32) for H, W in SIZES if _tileable(H, W, 32) and (H, W, 32) not in GEOMETRIES]


@pytest.mark.parametrize("H,W,tile", CASES)
@pytest.mark.parametrize("kind,C", KINDS)
def test_a_gathered_tile_row_is_that_row_of_the_full_gather(H, W, tile, kind, C):
    img, _ = _small(kind, C, H, W)
    src = B.ArraySource(img)
    for O in (0, 16):
        if kind == "u8":
            full = codec_ref.gather_u8(img, tile, tile, O)
        elif kind == "u16":
            full = u16_ref.gather(img, tile, tile, SCALE[:C], O)
        else:
            full = codec_ref.gather_f32(img, tile, tile, O)
        ny, nx = B.tile_rows(H, tile, O), B.tiles_per_row(W, tile, O)
        assert full.shape[0] == ny * nx
        if O == 0:
            assert (ny, nx) == (codec_ref.grid(H, W, tile, tile)["ny"], codec_ref.grid(H, W, tile, tile)["nx"])
        for i in range(ny):
            got = B.gather_tile_row(src, tile, tile, O, i, SCALE[:C])
            assert got.dtype == full.dtype and got.tobytes() == full[i * nx:(i + 1) * nx].tobytes(), (O, i)
        # the last tile row reads the image's last row; with padding it reads a reflected one as well
        last = B.source_rows(H, tile, O, ny - 1)
        assert H - 1 in last and (H % 16 == 0 or (np.diff(last) < 0).any())
        assert B.tile_rows_reading(H, tile, O, [H - 1])[-1] == ny - 1


@pytest.mark.parametrize("H,W,tile", CASES)
def test_counts_and_planes_of_a_tile_row_are_those_of_the_full_restatement(H, W, tile):
    img, valid = _small("u8", 3, H, W)
    src = B.ArraySource(img, valid)
    ny, nx = B.tile_rows(H, tile), B.tiles_per_row(W, tile)
    grid = mask_ref.tiles(H, W, tile, tile)
    for nodata, mask in ((7, mask_ref.nodata_mask(img, 7)), (None, ~valid)):
        counts = mask_ref.counts(mask, H, W, tile, tile)
        for i in range(ny):
            assert mask_ref.tile_row(H, W, tile, tile, i) == grid[i * nx:(i + 1) * nx]
            assert B.classify_tile_row(src, tile, tile, i, nodata) == counts[i * nx:(i + 1) * nx]
            planes = B.m_planes_tile_row(src, tile, tile, i, nodata)
            dwords, pops = B.delta_planes_tile_row(src, tile, tile, i, nodata)
            for j in range(nx):
                m = mask_ref.m_plane(mask, grid[i * nx + j], tile, tile)
                assert np.array_equal(planes[j], m)
                assert np.array_equal(dwords[j], mask_ref.plane_dwords(mask_ref.delta(m)))
                assert pops[j] == int(mask_ref.delta(m).sum())
    assert valid_ref.counts(valid, tile, tile) == mask_ref.counts(~valid, H, W, tile, tile)


def _bands(n):
    """every band of one and of two rows, every band that ends at the last row, and bands of 32"""
    out = {(y, y + 1) for y in range(n)} | {(y, min(y + 2, n)) for y in range(n)} | {(y, n) for y in range(n)}
    return sorted(out | {(y, min(y + 32, n)) for y in range(0, n, 7)})


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("kind,C", [("u8", 1), ("u8", 3), ("u8", 5), ("u16", 2), ("f32", 3)])
def test_halved_rows_are_those_of_the_full_halving(H, W, kind, C):
    img, valid = _small(kind, C, H, W)
    src = B.ArraySource(img, valid)
    full = pyramid_ref.halve(img) if kind != "u16" else u16_ref.halve(img)
    H2 = pyramid_ref.halved(H)
    for y0, y1 in _bands(H2):
        got = B.halve_rows(src, y0, y1)
        want = full[:, y0:y1] if kind == "f32" else full[y0:y1]
        assert got.dtype == want.dtype and got.tobytes() == np.ascontiguousarray(want).tobytes(), (y0, y1)
    if kind != "f32" and C <= 4:
        fimg, fval = valid_ref.halve(img, valid)
        for y0, y1 in _bands(H2):
            gimg, gval = B.halve_rows(src, y0, y1, with_valid=True)
            assert np.array_equal(gimg, fimg[y0:y1]) and np.array_equal(gval, fval[y0:y1]), (y0, y1)


@pytest.mark.parametrize("H,W,tile", GEOMETRIES)
@pytest.mark.parametrize("kind,C", KINDS)
def test_stitched_finished_and_masked_rows_are_those_of_the_whole_image(H, W, tile, kind, C):
    g = codec_ref.grid(H, W, tile, tile)
    rng = np.random.default_rng(H + W + C)
    ids = [int(t) for t in rng.permutation(g["n"] + 2) - 1][:-1]               # one tile left out, one number outside
    tiles = rng.uniform(-0.25, 1.25, size=(len(ids), C, tile, tile)).astype(np.float32)
    fill = {"u8": 0x5A, "u16": 0x5A5A, "f32": np.float32(-7)}[kind]
    scale = SCALE[:C]
    if kind == "u16":
        full = u16_ref.stitch(tiles, ids, H, W, tile, tile, (0, 0, H, W), scale, fill)
    else:
        full = codec_ref.stitch(tiles, ids, H, W, tile, tile, (0, 0, H, W), kind, fill)
    canvas = rng.uniform(-0.1, 1.3, size=(C, H, W)).astype(np.float32)
    finished = B.finish_rows(canvas, kind, scale)
    _, valid = _small("u8", 3, H, W)
    planes = valid_ref.m_planes(valid, tile, tile)
    desc = [(t, t if t % 3 else -1) for t in range(g["n"]) if t != 1] + [(g["n"], 0), (-1, 0)]
    pre = full                                                                  # any image will do as the pre-fill
    if kind == "u16":
        masked = valid_ref.apply(pre, (0, 0, H, W), H, W, tile, tile, desc, planes, 9)
    else:
        masked = mask_ref.apply(pre, (0, 0, H, W), H, W, tile, tile, desc, planes, 9)
    pre_val = np.full((H, W), 0x5A, dtype=np.uint8)
    window = valid_ref.window_valid(pre_val, (0, 0, H, W), H, W, tile, tile, desc, planes)

    def rows(a, y0, y1):
        return np.ascontiguousarray(a[:, y0:y1] if kind == "f32" else a[y0:y1])

    for y0, y1 in _bands(H):
        assert B.stitch_rows(tiles, ids, H, W, tile, tile, y0, y1, kind, fill, scale).tobytes() == \
            rows(full, y0, y1).tobytes(), (y0, y1)
        assert B.finish_rows(canvas[:, y0:y1], kind, scale).tobytes() == rows(finished, y0, y1).tobytes()
        assert B.mask_apply_rows(rows(pre, y0, y1), H, W, tile, tile, y0, desc, planes, 9).tobytes() == \
            rows(masked, y0, y1).tobytes(), (y0, y1)
        assert np.array_equal(B.mask_window_rows(pre_val[y0:y1], H, W, tile, tile, y0, desc, planes), window[y0:y1])


@pytest.mark.parametrize("case", sorted(blend_ref.CASES))
def test_blended_rows_are_those_of_the_whole_canvas(case):
    tile, O, H, W = blend_ref.CASES[case]
    C = 3
    tiles = blend_ref.make_tiles(case, C)
    ay, ax = blend_ref.axis(H, tile, O), blend_ref.axis(W, tile, O)
    th, tw, n = ay["t"], ax["t"], len(tiles)
    for ids in (list(range(n)), list(range(0, n, 2)), [n - 1], list(range(n // 2, n))):
        full = blend_ref.blend_f32([[(t, tiles[t]) for t in ids]], H, W, C, th, tw, O)
        for y0, y1 in _bands(H):
            got = B.blend_rows(tiles[ids], ids, H, W, C, th, tw, O, y0, y1)
            assert got.dtype == np.float32 and got.tobytes() == np.ascontiguousarray(full[:, y0:y1]).tobytes(), (ids, y0, y1)
        spans = B.blend_support_rows(ids, H, W, th, tw, O)
        outside = np.ones(H, dtype=bool)
        for a, b in spans:
            outside[a:b] = False
        assert not full[:, outside].any() and all(a < b <= H for a, b in spans)


def _full_res(tiles, q, tau, ids, H, W, tile, kind, fill, scale):
    """The stitch with a residual over the whole image, as test_gpu_near_lossless.py states it: per tile of the call,
    in order, reconstruct(predictor(x_hat), q, tau) over the pixels it owns inside the image."""
    import residual16_ref
    import residual_ref
    g = codec_ref.grid(H, W, tile, tile)
    out = np.full((H, W, tiles.shape[1]), fill, dtype=DT[kind])
    for k, t in enumerate(ids):
        if not 0 <= t < g["n"]:
            continue
        i, j = divmod(t, g["nx"])
        (ya, yb), (xa, xb), oy, ox = g["own_y"][i], g["own_x"][j], g["ys"][i], g["xs"][j]
        yb, xb = min(yb, H), min(xb, W)
        if kind == "u8":
            rec = residual_ref.reconstruct(residual_ref.predictor(tiles[k]), q[k], tau)
        else:
            rec = residual16_ref.reconstruct(residual16_ref.predictor(tiles[k], scale), q[k], tau)
        out[ya:yb, xa:xb] = rec[:, ya - oy:yb - oy, xa - ox:xb - ox].transpose(1, 2, 0)
    return out


@pytest.mark.parametrize("H,W,tile", GEOMETRIES)
@pytest.mark.parametrize("kind,C,tau", [("u8", 3, 3), ("u8", 4, 0), ("u16", 4, 300), ("u16", 1, 32767)])
def test_stitched_rows_with_a_residual_are_those_of_the_whole_image(H, W, tile, kind, C, tau):
    g = codec_ref.grid(H, W, tile, tile)
    rng = np.random.default_rng(H + W + C + tau)
    ids = [int(t) for t in rng.permutation(g["n"] + 2) - 1][:-1] + [0]          # one left out, one outside, one twice
    tiles = rng.uniform(-0.25, 1.25, size=(len(ids), C, tile, tile)).astype(np.float32)
    q = rng.integers(-B.QMAX, B.QMAX + 1, size=tiles.shape).astype(np.int64)
    fill, scale = {"u8": 0x5A, "u16": 0x5A5A}[kind], SCALE[:C]
    full = _full_res(tiles, q, tau, ids, H, W, tile, kind, fill, scale)
    assert (full != (codec_ref.stitch(tiles, ids, H, W, tile, tile, (0, 0, H, W), kind, fill) if kind == "u8" else
                     u16_ref.stitch(tiles, ids, H, W, tile, tile, (0, 0, H, W), scale, fill))).any()
    for y0, y1 in _bands(H):
        got = B.stitch_res_rows(tiles, q.astype(np.float32), tau, ids, H, W, tile, tile, y0, y1, kind, fill, scale)
        assert got.dtype == full.dtype and np.array_equal(got, full[y0:y1]), (y0, y1)


@pytest.mark.parametrize("H,W,tile", GEOMETRIES)
@pytest.mark.parametrize("C,tau", [(1, 0), (4, 2), (3, 1000)])
def test_the_quantized_residual_of_a_tile_row_is_that_of_the_whole_image(H, W, tile, C, tau):
    """the whole image as test_gpu_near_lossless_u16.py states it: per tile, quantize over its owned pixels, 0 elsewhere"""
    import residual16_ref
    img, _ = _small("u16", C, H, W)
    g = codec_ref.grid(H, W, tile, tile)
    x_hat = np.random.default_rng(H + C).uniform(-0.2, 1.2, size=(g["n"], C, tile, tile)).astype(np.float32)
    p = residual16_ref.predictor(x_hat, SCALE[:C])
    full = np.zeros(x_hat.shape, dtype=np.int64)
    for t in range(g["n"]):
        i, j = divmod(t, g["nx"])
        (ya, yb), (xa, xb), oy, ox = g["own_y"][i], g["own_x"][j], g["ys"][i], g["xs"][j]
        yb, xb = min(yb, H), min(xb, W)
        x = img[ya:yb, xa:xb].astype(np.int64).transpose(2, 0, 1)
        full[t][:, ya - oy:yb - oy, xa - ox:xb - ox] = residual16_ref.quantize(x, p[t][:, ya - oy:yb - oy, xa - ox:xb - ox], tau)
    src, nx = B.ArraySource(img), g["nx"]
    for i in range(g["ny"]):
        q, top = B.quantize_tile_row(src, x_hat[i * nx:(i + 1) * nx], tile, tile, i, SCALE[:C], tau)
        assert np.array_equal(q, full[i * nx:(i + 1) * nx]) and top == [int(np.abs(t).max()) for t in full[i * nx:(i + 1) * nx]]
    assert full.any()


def _regions(sh, sw, shift):
    """regions of level 0 over the whole level-`shift` image, its first rows, its last rows and one in between"""
    H0, W0 = sh << shift, sw << shift
    if sh * sw > 10000:                                                         # the restatement is a Python loop
        return [(0, 0, H0 // 4, W0 // 8), (H0 - H0 // 4, W0 - W0 // 8, H0 // 4, W0 // 8)]
    out = [(0, 0, H0, W0), (0, 0, max(1, H0 // 3), W0), (H0 - max(1, H0 // 3), 0, max(1, H0 // 3), W0)]
    if H0 >= 8 and W0 >= 8:
        out.append((H0 // 2 - 1, W0 // 4 + 1, 5, W0 // 2))
    return out


@pytest.mark.parametrize("src_size,out_size", V.SIZES)
@pytest.mark.parametrize("kind,C", KINDS)
def test_a_resampled_window_is_that_of_the_full_restatement(src_size, out_size, kind, C):
    sh, sw = src_size
    img, valid = _small(kind, C, sh, sw)
    src = B.ArraySource(img, valid)
    big = sh * sw > 10000
    for shift in V.SHIFTS:
        for region in _regions(sh, sw, shift):
            size = (min(out_size[0], 5), min(out_size[1], 7)) if big else out_size
            for mode in ("average", "nearest"):
                nodata = None if kind == "f32" else 7
                want = V.resample(img, 0, 0, shift, region, size, mode, nodata)
                assert B.resample(src, shift, region, size, mode, nodata).tobytes() == want.tobytes()
                if kind == "f32":
                    continue
                wimg, wval = valid_ref.resample(img, valid, 0, 0, shift, region, size, mode, 9)
                gimg, gval = B.resample_valid(src, shift, region, size, mode, 9)
                assert np.array_equal(gimg, wimg) and np.array_equal(gval, wval)
                pairs = [(10, 200)] * C if kind == "u8" else SCALE[:C]
                for with_valid in (False, True):
                    want = render_ref.render(img, valid if with_valid else None, 0, 0, shift, region, size, [2, 0, 1], pairs,
                                             mode, 7, True, 33)
                    got = B.render(src, with_valid, shift, region, size, [2, 0, 1], pairs, mode, 7, True, 33)
                    assert np.array_equal(got, want)


def test_the_tile_calls_refuse_a_grid_of_over_2_31_blocks_before_any_launch():
    """tile numbers and ny * nx are ints in the kernels: over 2^31 - 1 blocks of 16 x 16 is refused (no GPU needed)"""
    from dsic_amd import lib
    L = lib.load()
    one = 16                                                                   # a pointer no call gets to follow
    for H, W in ((1 << 20, 1 << 20), (2 ** 31 - 8, 32), (32, 2 ** 31 - 1)):
        assert L.dsic_tile_gather_u8(one, one, H, W, 3, 32, 32, 0, 1, None) == lib.DSIC_EINVAL
        assert b"blocks of 16 x 16" in L.dsic_last_error()
        assert L.dsic_valid_classify(one, H, W, 32, 32, 0, 1, one, None) == lib.DSIC_EINVAL
        assert b"blocks of 16 x 16" in L.dsic_last_error()
    # 2^15 x (2^16 - 1) blocks are inside the limit: the refusal is then that of the tile number
    assert L.dsic_tile_gather_u8(one, one, 2 ** 15 * 16, (2 ** 16 - 1) * 16, 3, 32, 32, 2 ** 31 - 2, 1, None) == lib.DSIC_EINVAL
    assert b"outside the grid" in L.dsic_last_error()


def test_a_scene_source_gives_the_scenes_rows():
    scene = S.Scene("t", "u16", 70, 1030, 4, valid=True)
    src = B.SceneSource(scene, keep=2)
    full, val = scene.band(0, 70), scene.valid_band(0, 70)
    for ys in ([0], [69, 68, 69], list(range(70)), [5, 3]):
        assert np.array_equal(src.rows(ys), full[ys]) and np.array_equal(src.valid(ys), val[ys])
    assert len(src.cache) <= 2
    assert blend_ref.axis(70, 32, 16)["n"] == B.tile_rows(70, 32, 16)


# ---- the viewing path: warped reads, index views and composites (test_gpu_big_views.py) ---------------------------------
import best_pixel_ref  # noqa: E402
import big_views as G  # noqa: E402
import composite_ref  # noqa: E402
import index_ref  # noqa: E402
import warp_ref  # noqa: E402

CMAP = np.stack([np.arange(256), 255 - np.arange(256), (7 * np.arange(256) + 3) % 256], axis=1).astype(np.uint8)
VIEW_SCENES = ("u8c3", "u8c3v", "u8c1v", "u16c4")


@pytest.mark.parametrize("kind,C", [("u8", 3), ("u16", 4), ("u16", 1)])
@pytest.mark.parametrize("LH,LW", [(17, 33), (40, 68)])
def test_a_banded_warp_is_the_full_restatement(kind, C, LH, LW):
    img = warp_ref.level_image(kind, C, LH, LW)
    val = warp_ref.validity(LH, LW, seed=C)
    src = B.ArraySource(img, val)
    pairs = [(10, 200)] * C if kind == "u8" else SCALE[:C]
    bands, index = [C - 1, 0, 0], ("nd", C - 1, 0) if C > 1 else ("band", 0)
    pair = (-1500, 2500) if C > 1 else (100, 40000)
    some = 0
    for l in (0, 1, 2):
        H, W = warp_ref.image_size(LH, l), warp_ref.image_size(LW, l)
        assert B.warp_image(src, l) == (H, W)
        for name, size in (("rot30", (16, 16)), ("magnify3", (17, 33)), ("overhang", (24, 20)), ("minify2.5", (7, 9))):
            m = warp_ref.matrix(name, H, W, *size)
            for mode in (0, 1, 2):
                for with_valid, nodata in ((True, None), (False, warp_ref.NODATA[kind]), (False, None)):
                    want, ok = warp_ref.warp(img, val if with_valid else None, 0, 0, l, LH, LW, H, W, m, size, mode, nodata, 9)
                    got, gok = B.warp(src, l, m, size, mode, with_valid, nodata, 9)
                    assert got.dtype == want.dtype and got.tobytes() == want.tobytes() and np.array_equal(gok, ok)
                    some += int(ok.any() and not ok.all())
                    zero = warp_ref.warp(img, val if with_valid else None, 0, 0, l, LH, LW, H, W, m, size, mode, nodata, 0)
                    shown = B.warp_render(src, l, m, size, mode, with_valid, nodata, bands, pairs, True, 33)
                    assert np.array_equal(shown, render_ref.display(*zero, bands, pairs, True, 33))
                    shown = B.warp_index(src, l, m, size, mode, with_valid, nodata, index, pair, CMAP, False, 200)
                    assert np.array_equal(shown, index_ref.display_index(*zero, index, pair, CMAP, False, 200))
    assert some >= 12
    # a view beside the image: fill and invalid
    got, gok = B.warp(src, 0, (65536, 0, 65536 * 4 * LH, 0, 65536, 0), (5, 7), 2, True, None, 9)
    assert (got == 9).all() and not gok.any()


@pytest.mark.parametrize("src_size,out_size", V.SIZES[2:5])
@pytest.mark.parametrize("kind,C", [("u8", 3), ("u16", 4)])
def test_a_banded_index_view_is_the_full_restatement(src_size, out_size, kind, C):
    sh, sw = src_size
    img, valid = _small(kind, C, sh, sw)
    src = B.ArraySource(img, valid)
    for shift in V.SHIFTS:
        for region in _regions(sh, sw, shift):
            for mode in ("average", "nearest"):
                for k, index in enumerate((("nd", C - 1, 0), ("difference", 0, C - 1), ("band", 1))):
                    vmin, vmax = index_ref.value_range(index[0], index_ref.top_of(img))
                    pair = (vmin // 2, vmax // 2 + 1)
                    res = V.resample(img, 0, 0, shift, region, out_size, mode, 7 if mode == "average" else None)
                    want = index_ref.display_index(res, None, index, pair, CMAP, k % 2, 33)
                    assert np.array_equal(B.index_render(src, False, shift, region, out_size, index, pair, CMAP, mode, 7, k % 2, 33), want)
                    res, ok = valid_ref.resample(img, valid, 0, 0, shift, region, out_size, mode, 0)
                    want = index_ref.display_index(res, ok, index, pair, CMAP, k % 2, 33)
                    assert np.array_equal(B.index_render(src, True, shift, region, out_size, index, pair, CMAP, mode, 7, k % 2, 33), want)


@pytest.mark.parametrize("name,size", [("rot30", (70, 130)), ("magnify5.25", (33, 40)), ("overhang", (40, 34)),
                                       ("mostly outside", (64, 50))])
def test_warped_rows_are_the_rows_of_the_full_view(name, size):
    """a rotation, a magnification, a view that hangs over the image and one that lies mostly outside it"""
    for kind, C, l in (("u8", 3, 0), ("u16", 4, 1), ("u16", 2, 2)):
        LH, LW = 40, 68
        H, W = warp_ref.image_size(LH, l), warp_ref.image_size(LW, l)
        img, val = warp_ref.level_image(kind, C, LH, LW), warp_ref.validity(LH, LW, seed=l)
        if name == "mostly outside":
            m = warp_ref.q16(warp_ref.rotation(H - 3, W - 5, 30, 1.5 * (1 << l), *size))
        else:
            m = warp_ref.matrix(name, H, W, *size)
        geometry = (l, LH, LW, H, W)
        for mode in (0, 1, 2):
            for v, nodata in ((val, None), (None, warp_ref.NODATA[kind]), (None, None)):
                full, ok = warp_ref.warp(img, v, 0, 0, l, LH, LW, H, W, m, size, mode, nodata, 9)
                assert ok.any() and not ok.all() or name in ("rot30", "magnify5.25")
                if name == "mostly outside":
                    assert ok.mean() < 0.25
                for i0, i1 in _bands(size[0])[::5]:
                    got, gok = B.warp_rows(img, v, geometry, m, size, mode, nodata, 9, i0, i1)
                    assert got.tobytes() == np.ascontiguousarray(full[i0:i1]).tobytes() and np.array_equal(gok, ok[i0:i1]), (i0, i1)
                    j0, j1 = size[1] // 3, size[1] - 2
                    got, gok = B.warp_rows(img, v, geometry, m, size, mode, nodata, 9, i0, i1, j0, j1)
                    assert np.array_equal(got, full[i0:i1, j0:j1]) and np.array_equal(gok, ok[i0:i1, j0:j1]), (i0, i1)


@pytest.mark.parametrize("ki,si", [(1, 2), (6, 2), (2, 1), (4, 3)])
def test_composited_rows_are_those_of_the_whole_composite(ki, si):
    """the sweeps of the small GPU tests (n from 1 to 16, the four modes and max / min, every layout): bands of one and
    two rows, bands to the last row and bands of 32 cut through sources, miss them, and hold a source exactly"""
    (oh, ow), (kind, C) = composite_ref.SIZES[si], composite_ref.KINDS[ki]
    if ow > 1000:
        oh, ow = 40, 300                                                       # the restatement sorts in int64
    seen = set()
    for case in composite_ref.sweep(ki, si) + [dict(c, mode=3) for c in composite_ref.sweep(ki, si)[::3]]:
        srcs, masks, rects, nodata = composite_ref.case_inputs(kind, C, oh, ow, case)
        sources = [B.ArraySource(s.reshape(r[2], r[3], C), m) for s, m, r in zip(srcs, masks, rects)]
        full = composite_ref.composite(srcs, masks, rects, nodata, C, oh, ow, case["mode"], 5)
        spans = _bands(oh)[::3] + [(r[0], r[0] + r[2]) for r in rects]         # the last: exactly a source's rows
        for y0, y1 in spans:
            got = B.composite_rows(sources, rects, nodata, None, C, oh, ow, case["mode"], None, 5, y0, y1)
            for g, w in zip(got, full):
                assert g.dtype == w.dtype and np.array_equal(g, w[y0:y1]), (case, y0, y1)
            kept = sum(1 for r in rects if max(r[0], y0) < min(r[0] + r[2], y1))
            seen |= {("n", case["n"]), ("mode", case["mode"]), "missed" if kept < case["n"] else "all", "none" if kept == 0 else "some"}
    assert {("mode", m) for m in range(4)} | {("n", n) for n in composite_ref.NS} | {"missed", "all", "some"} <= seen
    for case in best_pixel_ref.sweep(ki, si):
        srcs, masks, rects, nodata, ids = best_pixel_ref.case_inputs(kind, C, oh, ow, case)
        sources = [B.ArraySource(s.reshape(r[2], r[3], C), m) for s, m, r in zip(srcs, masks, rects)]
        full = best_pixel_ref.pick(srcs, masks, rects, nodata, ids, C, oh, ow, case["mode"], case["index"], 5)
        for y0, y1 in _bands(oh)[::4] + [(r[0], r[0] + r[2]) for r in rects]:
            got = B.composite_rows(sources, rects, nodata, ids, C, oh, ow, case["mode"], case["index"], 5, y0, y1)
            for g, w in zip(got, full):
                assert g.dtype == w.dtype and np.array_equal(g, w[y0:y1]), (case, y0, y1)
        seen.add(("pick", case["mode"]))
    assert {("pick", m) for m in best_pixel_ref.MODE_TURNS} <= seen
    # the disjoint layout leaves rows that no source meets: fill, nothing valid, and no source
    rects = composite_ref.layout("disjoint", 4, 33, 130)
    rng = np.random.default_rng(5)
    sources = [B.ArraySource(composite_ref.scene(kind, C, r[2], r[3], rng, i)) for i, r in enumerate(rects)]
    free = sorted(set(range(33)) - {y for r in rects for y in range(r[0], r[0] + r[2])})
    assert free
    got = B.composite_rows(sources, rects, [-1] * 4, [9, 8, 7, 6], C, 33, 130, best_pixel_ref.MAX, ("band", 0), 5, free[0], free[0] + 1)
    assert (got[0] == 5).all() and not got[1].any() and not got[2].any() and (got[3] == 255).all()


def _box(scene, ya, xa, nh, nw, delta=None, pixel_delta=None):
    """the samples and the validity bytes of a box of a scene by its formula; with delta, what a read `delta` elements
    earlier finds at and past element delta, with pixel_delta the same of the validity plane"""
    y = np.arange(ya, ya + nh, dtype=np.int64)[:, None, None]
    x = np.arange(xa, xa + nw, dtype=np.int64)[None, :, None]
    c = np.arange(scene.C, dtype=np.int64)[None, None, :]
    e = (y * scene.W + x) * scene.C + c
    if delta is not None:
        y, x, c = scene.coords(np.where(e >= delta, e - delta, e))
    img = S.NP.cast(scene.samples(S.NP, y + 0 * e, x + 0 * e, c + 0 * e), scene.kind)
    p = np.arange(ya, ya + nh, dtype=np.int64)[:, None] * scene.W + np.arange(xa, xa + nw, dtype=np.int64)[None, :]
    if pixel_delta is not None:
        p = np.where(p >= pixel_delta, p - pixel_delta, p)
    return img, S.NP.cast(S.validity(*np.divmod(p, scene.W)), "u8")


def _deltas(scene):
    """(elements, pixels) a wrapped offset falls short by: 2^32 bytes and 2^31 elements; 2^31 pixels of validity"""
    return sorted({(1 << 32) // scene.item, 1 << 31}), 1 << 31


@pytest.mark.parametrize("name", VIEW_SCENES)
def test_a_wrapped_offset_changes_every_warped_view_past_it(name):
    """every view of test_gpu_big_views.py on the big scenes whose centre lies at or past element 2^31 or byte 2^32 of the
    scene gives another expected output when its taps are read that far earlier, and another one when its validity bytes
    are read 2^31 pixels earlier"""
    s = S.table()[name]
    views = G.warp_views(s)
    where = [c for c in G.centres(s) for _ in G.LEVELS]
    assert len(views) == len(where) and {v[1] for v in views} == {0, 1, 2} and {v[4] for v in views} == {0, 1, 2}
    deltas, pixel_delta = _deltas(s)
    held, shown = {d: 0 for d in deltas + ["validity"]}, 0
    for (_, y, x), (what, l, m, size, mode) in zip(where, views):
        assert warp_ref.warp_level(3, m) == l, what                           # the scale asks for this level
        H, W = warp_ref.image_size(s.H, l), warp_ref.image_size(s.W, l)
        win = warp_ref.warp_window(l, s.H, s.W, H, W, m, *size, mode)
        assert win is not None and win[0] <= y < win[0] + win[2] and win[1] <= x < win[1] + win[3], what

        def view(img, val, nodata=None):
            return warp_ref.warp(img, val, win[0], win[1], l, s.H, s.W, H, W, m, size, mode, nodata, 9)

        img, val = _box(s, *win)
        right, right_valid, plain = view(img, None, s.nodata), view(img, val), view(img, None)
        shown += int(right[1].any() and right_valid[1].any())
        for d in deltas:
            if (y * s.W + x) * s.C >= d:
                early = _box(s, *win, delta=d)[0]
                assert not np.array_equal(view(early, None)[0], plain[0]), (what, d)
                assert not np.array_equal(view(early, None, s.nodata)[0], right[0]), (what, d)
                assert not np.array_equal(view(early, val)[0], right_valid[0]) or not right_valid[1].any(), (what, d)
                held[d] += 1
        if y * s.W + x >= pixel_delta:
            early = _box(s, *win, pixel_delta=pixel_delta)[1]
            got = view(img, early)
            assert not np.array_equal(got[1], right_valid[1]) or not np.array_equal(got[0], right_valid[0]), what
            held["validity"] += 1
    crossed = [d for d in deltas if d < s.elements]
    assert crossed and all(held[d] >= 3 for d in crossed)                     # each crossing at every level
    assert held["validity"] >= (6 if s.H * s.W > pixel_delta else 0)
    assert shown >= len(views) - 3                 # a view may lie inside a planted block of nodata or of invalid pixels


@pytest.mark.parametrize("name", ["u8c3", "u8c3v", "u16c4"])
def test_a_wrapped_offset_changes_every_index_view_past_it(name):
    """the same of the windows that test_gpu_big_views.py takes from test_gpu_big_images._windows"""
    from types import SimpleNamespace

    from test_gpu_big_images import _windows
    s = S.table()[name]
    deltas, pixel_delta = _deltas(s)
    held = {d: 0 for d in deltas + ["validity"]}
    for shift in (0, 1, 2):
        for region, size in _windows(SimpleNamespace(scene=s), shift):
            ya, xa, nh, nw = V.level_window(shift, *region)
            img, val = _box(s, ya, xa, nh, nw)
            for mode in ("average", "nearest"):
                right = V.resample(img, ya, xa, shift, region, size, mode, s.nodata if mode == "average" else None)
                right_valid = valid_ref.resample(img, val, ya, xa, shift, region, size, mode, 0)
                for d in deltas:
                    if (ya * s.W + xa) * s.C >= d:
                        early = _box(s, ya, xa, nh, nw, delta=d)[0]
                        assert not np.array_equal(V.resample(early, ya, xa, shift, region, size, mode, None), right), (region, d)
                        held[d] += 1
                if ya * s.W + xa >= pixel_delta:
                    early = _box(s, ya, xa, nh, nw, pixel_delta=pixel_delta)[1]
                    got = valid_ref.resample(img, early, ya, xa, shift, region, size, mode, 0)
                    assert not np.array_equal(got[1], right_valid[1]) or not np.array_equal(got[0], right_valid[0]), region
                    held["validity"] += 1
    assert all(held[d] >= 6 for d in deltas if d < s.elements)
    assert held["validity"] >= (6 if s.H * s.W > pixel_delta else 0)


def test_the_conditions_the_large_view_tests_lean_on():
    t = S.table()
    # composites: the output holds the scene's rect and stays under 2^31 pixels; past 2^20 workgroups of 4 x 64
    for name in ("u16c4", "u8c3"):
        s = t[name]
        oh, ow = G.composite_size(s)
        assert (oh, ow) == (s.H + 3, s.W + 5) and oh * ow < 1 << 31 and s.nbytes > 1 << 32
        assert -(-oh // 4) * -(-ow // 64) > 1 << 20
        for n, place in G.LISTS:
            rects, k = G.composite_rects(s, n, place)
            assert len(rects) == n and rects[k] == (1, 2, s.H, s.W) and k == (0 if place == "first" else n - 1)
            assert all(dy >= 0 and dx >= 0 and dy + h <= oh and dx + w <= ow for dy, dx, h, w in rects)
            rows = {y for j, r in enumerate(rects) if j != k for y in range(r[0], r[0] + r[2])}
            want = {0, oh - 1} | set(G.dst_crossing_rows(s)) | {int(y) + 1 for y in s.crossing_rows()}
            assert want <= rows or n < 7                                       # n = 3 has two small sources only
            G.composite_ids(n, k, 254)
        assert len(G.dst_crossing_rows(s)) == 2                              # dst itself passes 2^31 and 2^32 bytes
    assert G.composite_size(t["u8c3"])[0] * G.composite_size(t["u8c3"])[1] == 1433182824
    assert {n for n, _ in G.LISTS} == {3, 7, 13}
    for name in ("u8c1v", "u8c3v"):                                           # no composite source: its rect holds 2^31 pixels
        assert t[name].H * t[name].W >= 1 << 31
    # the histogram whose one bin passes 2^31
    assert (1 << 31) < t["u8c1v"].H * t["u8c1v"].W < (1 << 32) and t["u8c1v"].C == 1
    # writers: every output passes 2^32 bytes and 2^20 workgroups of 16 x 16, and holds the byte each view aims at
    exports = set()
    for export, kind, C, side, pb in G.WRITERS:
        assert side * side * pb > 1 << 32 and (-(-side // 16)) ** 2 > 1 << 20 and side <= 1 << 20
        assert pb == (C * (1 if kind == "u8" else 2) if export == "warp" else pb) and pb in (3, 4, 8)
        exports.add((export, kind))
        views = G.writer_views(side, pb)
        assert [v[2] for v in views] == [1 << 31, 1 << 32, None]
        for _, m, byte, box in views[:2]:
            y, x = G.writer_target(side, pb, byte)
            assert box[0] <= y < box[1] and box[2] <= x < box[3] and (y * side + x) * pb <= byte < (y * side + x + 1) * pb
            assert all(abs(v) < 1 << 26 for v in (m[0], m[1], m[3], m[4])) and abs(m[2]) < 1 << 47 and abs(m[5]) < 1 << 47
    assert exports == {(e, k) for e in ("warp", "warp_render", "warp_index_render") for k in ("u8", "u16")}
    assert {pb for e, _, _, _, pb in G.WRITERS if e != "warp"} == {3, 4}       # the byte store and the dword store


def test_the_recorded_index_histograms_name_the_pattern():
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "big_scene_index_counts.npz")
    biggest = max(os.path.getsize(os.path.join(os.path.dirname(path), f)) for f in ("big_scene_counts.npz",))
    assert os.path.getsize(path) <= biggest
    z = np.load(path)
    meta = json.loads(bytes(z["meta"]).decode())
    assert meta["constants"] == json.loads(json.dumps(S.CONSTANTS))
    t = S.table()
    for name, shape in meta["shapes"].items():
        assert shape == [t[name].H, t[name].W, t[name].C] and meta["nodata"][name] == t[name].nodata
    keys = {f"u8c3_{k}_{c}" for k in ("nd", "difference") for c in ("plain", "nodata", "valid", "valid_nodata")} | \
        {f"u16c4_{k}_{c}" for k in ("nd", "difference") for c in ("plain", "valid")}
    assert set(z.files) == keys | {"meta"}
    for key in keys:
        bins = 20001 if "_nd_" in key else (511 if key.startswith("u8") else 131071)
        assert z[key].shape == (bins,) and z[key].dtype == np.uint32
    assert int(z["u8c3_difference_plain"].astype(np.int64).sum()) == t["u8c3"].H * t["u8c3"].W
    assert int(z["u16c4_difference_plain"].astype(np.int64).sum()) == t["u16c4"].H * t["u16c4"].W


def test_the_size_limits_of_composites_and_index_histograms_are_refused_before_any_launch():
    """an output of exactly 2^31 pixels, an image of exactly 2^32 pixels: host checks, no GPU needed"""
    import ctypes

    from dsic_amd import lib
    L = lib.load()
    one = 16                                                                   # a pointer no call gets to follow
    head = [(ctypes.c_void_p * 1)(one), (ctypes.c_void_p * 1)(None), (ctypes.c_int * 4)(0, 0, 8, 8), (ctypes.c_int * 1)(-1)]
    for oh, ow in ((32768, 65536), (65536, 32768)):
        assert L.dsic_window_composite_u16(*head, 1, 3, one, None, None, oh, ow, 3, 0, None) == lib.DSIC_EINVAL
        assert b"under 2^31 pixels" in L.dsic_last_error()
        assert L.dsic_window_composite_pick_u8(*head, None, 1, 3, one, None, None, one, oh, ow, 4, 2, 0, 1, 0, None) == lib.DSIC_EINVAL
        assert b"under 2^31 pixels" in L.dsic_last_error()
    for fn in (L.dsic_index_histogram_u8, L.dsic_index_histogram_u16):
        assert fn(one, None, 65536, 65536, 3, -1, 2, 0, 1, one, None) == lib.DSIC_EINVAL
        assert b"under 2^32 pixels" in L.dsic_last_error()
        assert fn(one, None, 65536, 65535, 3, -1, 0, 0, 1, one, None) == lib.DSIC_EINVAL      # inside the limit: another refusal
        assert b"kind=0" in L.dsic_last_error()
