"""Nodata masks on the GPU.  The five steps of csrc/mask.hip alone (classify, delta planes, pack, unpack, apply), bit
for bit against the NumPy restatement of tests/mask_ref.py, outputs between guards and inputs inside a larger
allocation at byte offsets 0 to 3 as in test_gpu_pyramid.py; then the version-5 stream of codec.py on the 330 x 530
scene of test_gpu_pyramid.py with the same synthetic model (tile 128, batch 5, 15 tiles): a wedge 2y + x < 640 and a
64 x 64 block of speckle set to v = 0.  By hand that is 4 empty, 6 mixed and 5 full tiles, the speckle tile in mode 0
and the other mixed tiles in mode 1, so 11 coded tiles in containers of 5, 5 and 1; the tests take the truth from the
restatement and assert only that all three states and both modes occur and that fewer tiles are coded than the grid
has."""
import io
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

import mask_ref as R
from dsic_amd import codec, lib
from dsic_amd import mask as K
from dsic_amd import synthetic as S
from dsic_amd.entropy import EntropyError
from dsic_amd.model import CompressionModel
from dsic_amd.ops import _p, _stream

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GUARD = 64                                   # bytes on either side of an output and around an input
U8_GUARD, U8_FILL, U8_PAD = 0xCD, 0x5A, 0xEE
_CACHE = {}


class Out:
    """n bytes between guards inside one device allocation, `offset` bytes past a 16-byte aligned point, the interior
    pre-filled with `fill` (0xCD guards)."""

    def __init__(self, n, fill=U8_FILL, offset=0):
        self.n, self.lo = int(n), GUARD + offset
        host = np.full(self.lo + self.n + GUARD, U8_GUARD, dtype=np.uint8)
        host[self.lo:self.lo + self.n] = fill
        self.buf = torch.from_numpy(host).cuda()
        self.view = self.buf[self.lo:self.lo + self.n]

    def host(self, what):
        """The interior on the host, after the guards have been checked."""
        a = self.buf.cpu().numpy()
        g = np.concatenate([a[:self.lo], a[self.lo + self.n:]])
        assert (g == U8_GUARD).all(), f"{what}: guard overwritten"
        return a[self.lo:self.lo + self.n]


def _inside(arr, offset):
    """The array's bytes on the device, `offset` bytes past an aligned point of a larger allocation."""
    flat = np.ascontiguousarray(arr).view(np.uint8).ravel()
    host = np.full(GUARD + offset + flat.size + GUARD, U8_PAD, dtype=np.uint8)
    host[GUARD + offset:GUARD + offset + flat.size] = flat
    return torch.from_numpy(host).cuda()[GUARD + offset:GUARD + offset + flat.size]


def _same(got, want, what):
    got, want = np.ascontiguousarray(got).view(np.uint8).ravel(), np.ascontiguousarray(want).view(np.uint8).ravel()
    assert got.size == want.size, (what, got.size, want.size)
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero(got != want)
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {got.size} bytes differ, first at {i}: got {got[i]}, want {want[i]}")


def _i32(values):
    return torch.tensor(np.asarray(values, dtype=np.int32).ravel(), dtype=torch.int32, device="cuda")


# ---- the kernels ----------------------------------------------------------------------------------------------------
SHAPES = [(32, 32, 32), (40, 70, 32), (64, 100, 48), (300, 280, 272), (256, 256, 256)]
MASKS = ["none", "all", "wedge", "speckle", "corners"]


def _mask_of(kind, H, W, tile, rng):
    yy, xx = np.mgrid[:H, :W]
    if kind == "none":
        return np.zeros((H, W), bool)
    if kind == "all":
        return np.ones((H, W), bool)
    if kind == "wedge":
        return 2 * yy + xx < (2 * H + W) // 2
    if kind == "speckle":
        return rng.random((H, W)) < 0.5
    m = np.zeros((H, W), bool)                                           # a single pixel in each corner of every owned rectangle
    for _, _, y0, y1, x0, x1 in R.tiles(H, W, min(tile, R.ceil16(H)), min(tile, R.ceil16(W))):
        m[y0, x0] = m[y0, x1 - 1] = m[y1 - 1, x0] = m[y1 - 1, x1 - 1] = True
    return m


def _image(mask, C, v, rng):
    """random bytes; a valid pixel differs from v in channel 0 and may equal it in the others"""
    H, W = mask.shape
    img = rng.integers(0, 256, size=(H, W, C), dtype=np.uint8)
    img[..., 1:][rng.random((H, W, C - 1)) < 0.5] = v
    img[..., 0] = np.where(img[..., 0] == v, (v + 1) % 256, img[..., 0])
    img[mask] = v
    return img


@pytest.mark.parametrize("H,W,tile", SHAPES)
@pytest.mark.parametrize("C", [3, 4])
def test_mask_kernels_equal_the_restatement(H, W, tile, C):
    L = lib.load()
    th, tw = min(tile, R.ceil16(H)), min(tile, R.ceil16(W))
    grid = R.tiles(H, W, th, tw)
    n, D, raw = len(grid), th * tw // 32, th * tw // 8
    rng = np.random.default_rng(H * 1009 + W * 17 + C)
    run = 0
    for v in (0, 7, 255):
        for kind in MASKS:
            off = run % 4                                                # every byte offset of the inputs, in turn
            run += 1
            what = f"{H}x{W}x{C} tile {tile} v={v} {kind}, offset {off}"
            mask = _mask_of(kind, H, W, tile, rng)
            img = _image(mask, C, v, rng)
            assert np.array_equal(R.nodata_mask(img, v), mask)
            d_img = _inside(img, off)
            # 1. classify
            counts = Out(4 * n, fill=0)
            lib.check(L.dsic_mask_classify_u8(_p(d_img), H, W, C, th, tw, v, 0, n, _p(counts.view), _stream()), what)
            want_counts = R.counts(mask, H, W, th, tw)
            _same(counts.host(what + " classify"), np.array(want_counts, dtype="<i4"), what + " classify")
            # 2. delta planes of every tile and of a number outside the grid
            ids = list(range(n)) + [n]
            d_ids = _i32(ids)
            planes, pop = Out(4 * D * (n + 1)), Out(4 * (n + 1), fill=0)
            lib.check(L.dsic_mask_delta_planes_u8(_p(d_img), H, W, C, th, tw, v, _p(d_ids), n + 1, _p(planes.view),
                                                  _p(pop.view), _stream()), what)
            ms = [R.m_plane(mask, g, th, tw) for g in grid]
            ds = [R.delta(m) for m in ms] + [np.zeros((th, tw), bool)]
            _same(planes.host(what + " planes"), np.concatenate([R.plane_dwords(d) for d in ds]), what + " planes")
            _same(pop.host(what + " popcounts"), np.array([int(d.sum()) for d in ds], dtype="<i4"), what + " popcounts")
            # 3. pack
            pays = [R.payload(d) for d in ds]
            want = b"".join(struct.pack("<3I", t, mode, len(body)) for t, (mode, body) in zip(ids, pays))
            want += b"".join(body for _, body in pays)
            out, ws = Out((n + 1) * (12 + raw)), Out(8 * (n + 3))
            lib.check(L.dsic_mask_pack(_p(planes.view), _p(pop.view), _p(d_ids), n + 1, th, tw, _p(ws.view),
                                       _p(out.view), _stream()), what)
            got = out.host(what + " pack")
            assert ws.host(what + " ws")[:16].view("<i8").tolist() == [len(want), 0], what
            _same(got[:len(want)], np.frombuffer(want, np.uint8), what + " pack")
            assert (got[len(want):] == U8_FILL).all(), what + ": pack wrote past its bytes"
            # 4. unpack
            blob = b"".join(body for _, body in pays)
            desc, at = [], 0
            for mode, body in pays:
                desc.append((mode, at, len(body)))
                at += len(body)
            d_desc = _i32(desc)
            d_blob = _inside(np.frombuffer(blob + b"\0" * 16, np.uint8), off)
            mplanes = Out(4 * D * (n + 1))
            lib.check(L.dsic_mask_unpack(_p(d_blob), len(blob), _p(d_desc), n + 1, th, tw, _p(mplanes.view),
                                         _stream()), what)
            _same(mplanes.host(what + " unpack"), np.concatenate([R.plane_dwords(m) for m in ms + [ds[-1]]]),
                  what + " unpack")
            # 5. apply: the whole image and a window that cuts tiles; a number outside the grid, and "all set" for tile 0
            adesc = [(t, t) for t in range(1, n)] + [(n, 0), (-1, 0), (0, -1)]
            d_adesc = _i32(adesc)
            windows = [(0, 0, H, W), (H // 3, W // 4, H // 2 + 1, W // 2 + 3)]
            for win in windows:
                wy, wx, wh, ww = win
                pre = rng.integers(0, 256, size=(wh, ww, C), dtype=np.uint8)
                o = Out(pre.size)
                o.view.copy_(torch.from_numpy(pre.ravel()).cuda())
                lib.check(L.dsic_mask_apply_u8(_p(mplanes.view), n + 1, _p(d_adesc), len(adesc), v, _p(o.view), H, W,
                                               C, th, tw, wy, wx, wh, ww, _stream()), what)
                _same(o.host(what + " apply_u8"), R.apply(pre, win, H, W, th, tw, adesc, ms, v), f"{what} apply_u8 {win}")
                pre = rng.random((C, wh, ww), dtype=np.float32)
                o = Out(4 * pre.size)
                o.view.copy_(torch.from_numpy(pre.view(np.uint8).ravel()).cuda())
                lib.check(L.dsic_mask_apply_f32(_p(mplanes.view), n + 1, _p(d_adesc), len(adesc), v, _p(o.view), H, W,
                                                C, th, tw, wy, wx, wh, ww, _stream()), what)
                _same(o.host(what + " apply_f32"), R.apply(pre, win, H, W, th, tw, adesc, ms, v),
                      f"{what} apply_f32 {win}")


def test_mask_pack_of_more_than_256_tiles_in_one_call():
    """290 records in one dsic_mask_pack, so the offsets scan of its head kernel runs a second pass of 256 with the
    carry of the first (mask.MAX_TILES lets the codec send 1024).  A 544 x 544 x 3 image in tiles of 32 (17 x 17 = 289,
    and the number 289 outside the grid): a wedge above row 480 makes list-mode tiles of differing lengths, speckle
    below it makes tiles 255 .. 288 raw, on both sides of record 256.  Steps 2 to 4 of the kernel test above."""
    L = lib.load()
    H = W = 544
    C, th, tw, v, off = 3, 32, 32, 7, 1
    grid = R.tiles(H, W, th, tw)
    n, D, raw = len(grid), th * tw // 32, th * tw // 8
    rng = np.random.default_rng(544)
    yy, xx = np.mgrid[:H, :W]
    mask = np.where(yy < 480, 2 * yy + xx < 816, rng.random((H, W)) < 0.5)
    img = _image(mask, C, v, rng)
    ids = list(range(n)) + [n]
    ms = [R.m_plane(mask, g, th, tw) for g in grid]
    ds = [R.delta(m) for m in ms] + [np.zeros((th, tw), bool)]
    pays = [R.payload(d) for d in ds]
    modes = [mode for mode, _ in pays]
    assert n == 289 and len(ids) > 256 and set(modes) == {0, 1}
    assert all(modes[t] == 0 for t in range(255, 289)), "raw tiles on both sides of record 256"
    assert len({len(body) for mode, body in pays[:255]}) > 2, "list payloads of differing lengths before them"
    d_img, d_ids = _inside(img, off), _i32(ids)
    planes, pop = Out(4 * D * (n + 1)), Out(4 * (n + 1), fill=0)
    lib.check(L.dsic_mask_delta_planes_u8(_p(d_img), H, W, C, th, tw, v, _p(d_ids), n + 1, _p(planes.view),
                                          _p(pop.view), _stream()), "delta planes")
    _same(planes.host("planes"), np.concatenate([R.plane_dwords(d) for d in ds]), "planes")
    _same(pop.host("popcounts"), np.array([int(d.sum()) for d in ds], dtype="<i4"), "popcounts")
    want = b"".join(struct.pack("<3I", t, mode, len(body)) for t, (mode, body) in zip(ids, pays))
    want += b"".join(body for _, body in pays)
    out, ws = Out((n + 1) * (12 + raw)), Out(8 * (n + 3))
    lib.check(L.dsic_mask_pack(_p(planes.view), _p(pop.view), _p(d_ids), n + 1, th, tw, _p(ws.view), _p(out.view),
                               _stream()), "pack")
    got = out.host("pack")
    assert ws.host("ws")[:16].view("<i8").tolist() == [len(want), 0]
    _same(got[:len(want)], np.frombuffer(want, np.uint8), "pack")
    assert (got[len(want):] == U8_FILL).all(), "pack wrote past its bytes"
    blob = b"".join(body for _, body in pays)
    desc, at = [], 0
    for mode, body in pays:
        desc.append((mode, at, len(body)))
        at += len(body)
    d_desc, d_blob = _i32(desc), _inside(np.frombuffer(blob + b"\0" * 16, np.uint8), off)
    mplanes = Out(4 * D * (n + 1))
    lib.check(L.dsic_mask_unpack(_p(d_blob), len(blob), _p(d_desc), n + 1, th, tw, _p(mplanes.view), _stream()),
              "unpack")
    _same(mplanes.host("unpack"), np.concatenate([R.plane_dwords(m) for m in ms + [ds[-1]]]), "unpack")


def test_the_last_position_of_a_u16_tile():
    """one 256 x 256 tile whose only nodata pixel is the last: d has bit 65535 alone"""
    L = lib.load()
    img = np.full((256, 256, 3), 200, np.uint8)
    img[255, 255] = 7
    d_img, zero, desc = _inside(img, 1), _i32([0]), _i32([(1, 0, 2)])
    planes, pop = Out(8192), Out(4, fill=0)
    lib.check(L.dsic_mask_delta_planes_u8(_p(d_img), 256, 256, 3, 256, 256, 7, _p(zero), 1, _p(planes.view),
                                          _p(pop.view), _stream()), "delta")
    got = planes.host("planes")
    assert got[-1] == 0x80 and not got[:-1].any() and pop.host("pop").view("<i4")[0] == 1
    out, ws = Out(12 + 8192), Out(24)
    lib.check(L.dsic_mask_pack(_p(planes.view), _p(pop.view), _p(zero), 1, 256, 256, _p(ws.view), _p(out.view),
                               _stream()), "pack")
    assert out.host("pack")[:14].tobytes() == struct.pack("<3IH", 0, 1, 2, 65535)
    m = Out(8192)
    blob = _inside(np.frombuffer(struct.pack("<H", 65535) + b"\0" * 16, np.uint8), 3)
    lib.check(L.dsic_mask_unpack(_p(blob), 2, _p(desc), 1, 256, 256, _p(m.view), _stream()), "unpack")
    got = m.host("unpack")
    assert got[-1] == 0x80 and not got[:-1].any()


# ---- the codec ------------------------------------------------------------------------------------------------------
H0, W0, TILE, BATCH, V = 330, 530, 128, 5, 0
ARGS = {"tile": TILE, "batch": BATCH}
CONFIGS = {"plain": (3, {}), "segments": (3, {"segments": 4}), "bands4": (4, {})}


def _model(in_ch=3, N=128, M=192):
    key = ("model", in_ch, N, M)
    if key not in _CACHE:
        sd = S.make_state_dict(seed=1, N=N, M=M, in_ch=in_ch, spatial_params=False)
        m = CompressionModel(N=N, M=M, spatial_params=False, min_nu=2, max_nu=100.0, in_ch=in_ch)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        _CACHE[key] = (m.cuda().eval(), sd)
    return _CACHE[key][0]


def _scene(in_ch=3):
    """The scene of test_gpu_pyramid.py with the wedge and the speckle block set to V, NumPy uint8 HWC, read-only."""
    if ("scene", in_ch) not in _CACHE:
        x = S.make_patches(21, 1, H0, W0, in_ch)[0].astype(np.float32)
        img = np.ascontiguousarray((x * 255.0 + 0.5).astype(np.uint8).transpose(1, 2, 0))
        yy, xx = np.mgrid[:H0, :W0]
        img[2 * yy + xx < 640] = V
        block = img[258:322, 388:452]
        block[np.random.default_rng(5).random((64, 64)) < 0.5] = V
        img.setflags(write=False)
        _CACHE[("scene", in_ch)] = img
    return _CACHE[("scene", in_ch)]


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _streams(config):
    """(the version-5 stream of the scene, the stream without nodata, the scene, its mask), coded once per config"""
    if ("streams", config) not in _CACHE:
        in_ch, kw = CONFIGS[config]
        img, model = _scene(in_ch), _model(in_ch)
        masked = codec.compress_image(model, _dev(img), nodata=V, **ARGS, **kw)
        plain = codec.compress_image(model, _dev(img), **ARGS, **kw)
        _CACHE[("streams", config)] = (masked, plain, img, R.nodata_mask(img, V))
    return _CACHE[("streams", config)]


def _decodes(config):
    """the plain stream's decode per out, and what the masked stream must decode to"""
    if ("decodes", config) not in _CACHE:
        _, plain, _, mask = _streams(config)
        model = _model(CONFIGS[config][0])
        out = {}
        for kind in (None, "u8", "f32"):
            dec = codec.decompress_image(model, plain, out=kind).cpu().numpy()
            want = dec.copy()
            if dec.dtype == np.uint8:
                want[mask] = V
            else:
                want[:, mask] = np.float32(V) / np.float32(255)
            out[kind] = (dec, want)
        _CACHE[("decodes", config)] = out
    return _CACHE[("decodes", config)]


def _crop(full, win):
    y0, x0, h, w = win
    return full[y0:y0 + h, x0:x0 + w] if full.dtype == np.uint8 else full[:, y0:y0 + h, x0:x0 + w]


@pytest.mark.parametrize("config", list(CONFIGS))
def test_the_stream_keeps_the_mask_and_the_coded_tiles_strings(config):
    masked, plain, img, mask = _streams(config)
    in_ch, kw = CONFIGS[config]
    model = _model(in_ch)
    block, states = R.block(img, V, TILE, TILE)
    u = codec.unpack_image_stream(masked)
    ix, px = codec.stream_index(masked), codec.stream_index(plain)
    assert u["version"] == 5 and u["nodata"] == V and u["segments"] == kw.get("segments", 1)
    assert set(states) == {0, 1, 2} and u["coded"] == sum(1 for s in states if s) < len(states) == 15
    assert u["mask"] == block, "the mask block is not the restatement's"
    assert {r["m_mode"] for r in ix["tiles"] if r["state"] == 2} == {0, 1}
    assert u["batches"] == -(-u["coded"] // BATCH) == len(ix["containers"])
    if config == "plain":
        assert (states.count(0), states.count(2), states.count(1)) == (4, 6, 5), states
    for t, (r, p) in enumerate(zip(ix["tiles"], px["tiles"])):
        assert r["state"] == states[t]
        if states[t] == 0:
            assert r["k"] is None and r["z_len"] == r["y_len"] == 0
            continue
        for o, n in (("z_off", "z_len"), ("y_off", "y_len")):
            assert masked[r[o]:r[o] + r[n]] == plain[p[o]:p[o] + p[n]], f"tile {t} {o}"
        assert (r["min_y"], r["max_y"], r["min_z"], r["max_z"], r["y_segs"]) == (p["min_y"], p["max_y"], p["min_z"],
                                                                                   p["max_z"], p["y_segs"])
    # the whole image, exactly: nodata where the original had it, the plain decode elsewhere
    for kind, (dec, want) in _decodes(config).items():
        got = codec.decompress_image(model, masked, out=kind).cpu().numpy()
        assert got.dtype == want.dtype and got.shape == want.shape
        assert np.array_equal(got, want), (config, kind, int((got != want).sum()))
        sel = mask if got.dtype == np.uint8 else (slice(None), mask)
        assert (got[sel] == (V if got.dtype == np.uint8 else np.float32(V) / np.float32(255))).all()
    # two runs give the same bytes
    assert codec.compress_image(model, _dev(img), nodata=V, **ARGS, **kw) == masked


def _windows(ix):
    """the corner pixels, one inside an empty tile, one crossing empty, mixed and full tiles, the whole image"""
    g, states = ix["grid"], [r["state"] for r in ix["tiles"]]
    e = states.index(0)
    y0, x0 = g["own_y"][e // g["nx"]][0], g["own_x"][e % g["nx"]][0]
    return [(0, 0, 1, 1), (H0 - 1, W0 - 1, 1, 1), (y0 + 5, x0 + 7, 40, 50), (100, 90, 200, 400), (0, 0, H0, W0)]


@pytest.mark.parametrize("config", list(CONFIGS))
def test_windows_are_crops_of_the_full_decode_at_any_batch(config):
    masked, _, _, _ = _streams(config)
    model = _model(CONFIGS[config][0])
    ix = codec.stream_index(masked)
    wins = _windows(ix)
    met = {ix["tiles"][t]["state"] for t in codec.window_tiles(ix, *wins[3])}
    assert met == {0, 1, 2}, met
    for batch in (1, 4, 64):
        for win in wins:
            for kind in (None, "f32"):
                stats = {}
                got = codec.decompress_region(model, masked, *win, out=kind, batch=batch, stats=stats).cpu().numpy()
                want = _crop(_decodes(config)[kind][1], win)
                assert got.dtype == want.dtype and np.array_equal(got, want), (config, batch, win, kind)
                coded = [t for t in stats["tiles"] if ix["tiles"][t]["state"]]
                assert stats["tiles"] == codec.window_tiles(ix, *win)
                assert stats["decode_batches"] == -(-len(coded) // batch)


def test_a_window_of_empty_tiles_reads_no_strings_and_decodes_nothing():
    masked, _, _, _ = _streams("plain")
    model, ix = _model(), codec.stream_index(masked)
    win = _windows(ix)[2]
    assert all(ix["tiles"][t]["state"] == 0 for t in codec.window_tiles(ix, *win))
    for src in (masked, io.BytesIO(masked)):
        stats = {}
        got = codec.decompress_region(model, src, *win, stats=stats)
        assert got.shape == (40, 50, 3) and bool((got == V).all())
        assert stats["bytes_read"] == ix["index_bytes"] and stats["decode_batches"] == 0
        assert stats["bytes_uploaded"] == 0


class Recording:
    """A binary file object that records the position and length of every read."""

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


def test_a_file_is_read_only_at_the_heads_and_the_selected_tiles_spans():
    masked, _, _, _ = _streams("plain")
    model, ix = _model(), codec.stream_index(masked)
    win = (100, 90, 200, 400)
    f, stats = Recording(masked), {}
    got = codec.decompress_region(model, f, *win, stats=stats)
    assert np.array_equal(got.cpu().numpy(), _crop(_decodes("plain")[None][1], win))
    spans = codec.tile_spans(ix, stats["tiles"])
    assert any(ix["tiles"][t].get("m_len") for t in stats["tiles"])
    assert sum(n for _, n in f.reads) == stats["bytes_read"] == ix["index_bytes"] + sum(n for _, n in spans)
    heads = [(0, 60 + 16 + 8), (ix["mask_offset"], K.head_bytes(15, sum(1 for r in ix["tiles"] if r["state"] == 2)))]
    heads += [(c["offset"] - 8, 8 + 38 + 4 + 24 * c["tiles"]) for c in ix["containers"]]
    for pos, n in f.reads:
        assert any(a <= pos and pos + n <= a + m for a, m in heads + spans), f"read of {n} bytes at {pos}"
    assert stats["bytes_read"] < len(masked)


def test_all_nodata_and_no_nodata_images_round_trip():
    model = _model()
    blank = np.full((H0, W0, 3), 9, np.uint8)
    stream = codec.compress_image(model, _dev(blank), nodata=9, **ARGS)
    u = codec.unpack_image_stream(stream)
    assert u["batches"] == 0 and u["coded"] == 0 and u["blobs"] == []
    for kind in (None, "f32"):
        got = codec.decompress_image(model, stream, out=kind).cpu().numpy()
        assert np.array_equal(got, blank if kind is None else np.full((3, H0, W0), np.float32(9) / np.float32(255)))
    assert bool((codec.decompress_region(model, stream, 7, 9, 100, 200, batch=2) == 9).all())
    # not one nodata pixel: every tile full, and the decode is the plain one
    _, plain, img, _ = _streams("plain")
    v = 3
    clean = np.where((img == v).all(axis=2, keepdims=True), np.uint8(4), img)
    stream = codec.compress_image(model, _dev(clean), nodata=v, **ARGS)
    ix = codec.stream_index(stream)
    assert ix["coded"] == 15 and {r["state"] for r in ix["tiles"]} == {1}
    want = codec.decompress_image(model, codec.compress_image(model, _dev(clean), **ARGS))
    assert torch.equal(codec.decompress_image(model, stream), want)


def test_a_foreign_model_is_refused_as_today():
    masked, _, _, _ = _streams("plain")
    for other in (_model(M=128), _model(N=64)):
        with pytest.raises(EntropyError, match="model"):
            codec.decompress_image(other, masked)
        with pytest.raises(EntropyError, match="model"):
            codec.decompress_region(other, masked, 0, 0, 8, 8)


def test_command_line_round_trip(tmp_path):
    model = _model()
    sd = _CACHE[("model", 3, 128, 192)][1]
    torch.save({"model": {k: torch.from_numpy(v) for k, v in sd.items()}}, tmp_path / "ckpt.pt")
    u8 = np.array(_scene()[100:250, 150:320])                            # 150 x 170: wedge, valid pixels and an empty tile
    np.save(tmp_path / "in.npy", u8)
    tool = os.path.join(ROOT, "tools", "dsic_image.py")
    w = ["--weights", str(tmp_path / "ckpt.pt")]
    region = (5, 6, 120, 130)
    runs = (["compress", str(tmp_path / "in.npy"), str(tmp_path / "s.dsic"), "--tile", "64", "--batch", "4",
             "--nodata", "0"] + w,
            ["info", str(tmp_path / "s.dsic")],
            ["decompress", str(tmp_path / "s.dsic"), str(tmp_path / "win.npy"), "--region",
             ",".join(str(v) for v in region)] + w)
    outs = []
    for args in runs:
        r = subprocess.run([sys.executable, tool, *args], cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        outs.append(r.stdout)
    stream = codec.compress_image(model, torch.from_numpy(u8), tile=64, batch=4, nodata=0)
    assert (tmp_path / "s.dsic").read_bytes() == stream
    want = codec.decompress_region(model, stream, *region)
    assert np.array_equal(np.load(tmp_path / "win.npy"), want.cpu().numpy()) and want.shape == (120, 130, 3)
    ix = codec.stream_index(stream)
    st = [r["state"] for r in ix["tiles"]]
    assert st.count(0) and st.count(2)
    assert (f"nodata 0: {st.count(0)} empty, {st.count(1)} full, {st.count(2)} mixed tile(s), {ix['coded']} coded; "
            f"mask block {ix['mask_bytes']} bytes") in outs[1], outs[1]
    assert f"nodata 0: {ix['coded']} coded tile(s)" in outs[0]
