"""Pan and zoom on the GPU.  The three resampling kernels alone, bit for bit against the NumPy restatement of
tests/view_ref.py, outputs between guards and inputs inside a larger allocation as in test_gpu_pyramid.py; then
codec.ImageReader on the 330 x 530 scene and the synthetic model of that file (tile 128, batch 5: 3 x 5 tiles): its
plain reads equal decompress_region for every kind of stream whatever the cache holds, its counters follow the cache
model of view_ref.py, read_many shares decode batches, and resampled reads are the restatement applied to
decompress_region's output of the covering window."""
import ctypes
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import view_ref as V
from dsic_amd import codec, lib
from dsic_amd.ops import _p, _stream
from test_gpu_mask import V as NODATA
from test_gpu_mask import _streams as _mask_streams
from test_gpu_pyramid import _CACHE as _PCACHE
from test_gpu_pyramid import BATCH, H0, W0, Out, Recording, _alone, _inside, _model, _pyramid, _same
from test_gpu_u16 import EXPLICIT, _u16_stream

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_REF = {}
MODES = {"average": 0, "nearest": 1}


# ---- the kernels ----------------------------------------------------------------------------------------------------
def _resample(kind, src, c, C, dst, mode, nodata):
    L = lib.load()
    y0, x0, h, w = c["region"]
    oh, ow = c["size"]
    head = (_p(src), c["sh"], c["sw"], c["sy0"], c["sx0"], C, c["shift"], y0, x0, h, w, _p(dst), oh, ow, mode)
    if kind == "f32":
        return L.dsic_window_resample_f32(*head, ctypes.c_float(0.0 if nodata is None else nodata),
                                          int(nodata is not None), _stream())
    return getattr(L, "dsic_window_resample_" + kind)(*head, -1 if nodata is None else nodata, _stream())


@pytest.mark.parametrize("src_size,out_size", V.SIZES)
@pytest.mark.parametrize("kind,C", V.KINDS)
def test_resampling_kernels_equal_the_restatement(src_size, out_size, kind, C):
    for shift in V.SHIFTS:
        c = V.kernel_case(src_size, out_size, shift)
        img = V.kernel_image(kind, C, c["sh"], c["sw"])
        src = _inside(img, shift)                                            # the input at several element offsets
        for mode, nodata in (("average", None), ("average", V.NODATA[kind]), ("nearest", V.NODATA[kind])):
            want = V.resample(img, c["sy0"], c["sx0"], shift, c["region"], c["size"], mode, nodata)
            out = Out(want.size, img.dtype, (0, 1, 3)[shift])
            what = f"window_resample_{kind} {src_size}->{out_size} C={C} shift={shift} {mode} nodata={nodata}"
            lib.check(_resample(kind, src, c, C, out.view, MODES[mode], nodata), what)
            _same(out.host(what), want, what)
            if nodata is not None and mode == "average" and src_size[0] >= 17 and out_size[0] < src_size[0]:
                first = want[0, 0] if kind != "f32" else want[:, 0, 0]
                assert (first == img.dtype.type(nodata)).all(), what       # the top-left quarter is all nodata


def test_halving_the_whole_image_is_the_overview_level():
    """size = (H/2, W/2) of an even-sided image at shift 0: (a + b + c + d + 2) >> 2, what build_overviews gives"""
    for kind, dtype in (("u8", torch.uint8), ("u16", torch.uint16)):
        img = V.kernel_image(kind, 3, 40, 68)
        dev = torch.from_numpy(img).cuda()
        want = codec.build_overviews(dev, 1)[1]
        got = torch.empty((20, 34, 3), dtype=dtype, device="cuda")
        c = {"sh": 40, "sw": 68, "sy0": 0, "sx0": 0, "shift": 0, "region": (0, 0, 40, 68), "size": (20, 34)}
        lib.check(_resample(kind, dev, c, 3, got, 0, None), kind)
        assert np.array_equal(got.cpu().numpy(), want.cpu().numpy())


def test_the_calls_refuse_through_their_error_return_and_write_nothing():
    src = torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda")
    out = Out(4 * 4 * 3, np.uint8)
    ok = {"sh": 8, "sw": 8, "sy0": 0, "sx0": 0, "shift": 0, "region": (0, 0, 8, 8), "size": (4, 4)}
    for change, word in (({"region": (0, 0, 9, 8)}, "outside the source window"), ({"shift": 16}, "shift=16"),
                         ({"sy0": 1}, "outside the source window"), ({"size": (0, 4)}, "output")):
        assert _resample("u8", src, dict(ok, **change), 3, out.view, 0, None) == lib.DSIC_EINVAL
        assert word.encode() in lib.load().dsic_last_error()
    assert _resample("u8", src, ok, 2, out.view, 0, None) == lib.DSIC_EINVAL
    with pytest.raises(ValueError, match="mode=3"):
        lib.check(_resample("u8", src, ok, 3, out.view, 3, None), "window_resample_u8")
    assert (out.host("refused calls") == 0x5A).all()


# ---- the reader -----------------------------------------------------------------------------------------------------
def _stream_of(name):
    if name == "nodata":
        return _mask_streams("plain")[0]
    if name == "u16":
        return _u16_stream(scale=EXPLICIT)
    if name == "pyramid":
        return _pyramid()[0]
    return _alone("u8", 0, **{"plain": {}, "segments": {"segments": 4}, "overlap": {"overlap": 32},
                              "max_error": {"max_error": 2}}[name])


def _outs(name):
    return (None, "u8", "f32", "u16") if name == "u16" else (None, "u8", "f32")


def _windows(h, w):
    """one pixel, inside one tile, across four tiles (where the level has them), the whole level"""
    return [(h - 1, w - 1, 1, 1), (5, 7, min(60, h - 5), min(90, w - 7)), (h // 3, w // 5, h // 2, w // 2),
            (0, 0, h, w)]


def _region(name, level, win, out):
    """decompress_region's result, computed once and shared"""
    key = (name, level, win, out)
    if key not in _REF:
        _REF[key] = codec.decompress_region(_model(), _stream_of(name), *win, out=out, batch=BATCH, level=level)
    return _REF[key]


def _tile_bytes(ix):
    return 4 * ix["C"] * ix["th"] * ix["tw"] * (2 if "max_error" in ix else 1)


def _eq(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want)


CASES = [("plain", 0), ("segments", 0), ("overlap", 0), ("max_error", 0), ("nodata", 0), ("u16", 0), ("pyramid", 0),
         ("pyramid", 1), ("pyramid", 2), ("pyramid", 3)]


@pytest.mark.parametrize("name,level", CASES)
def test_a_plain_read_equals_decompress_region_whatever_the_cache_holds(name, level):
    model, stream = _model(), _stream_of(name)
    ix = codec.stream_index(stream, level=level)
    wins = _windows(ix["H"], ix["W"])
    two = 2 * _tile_bytes(ix)
    for cache_bytes in (1 << 30, two, 0):
        with codec.ImageReader(model, stream, cache_bytes=cache_bytes, batch=BATCH) as r:
            assert r.shape == (H0, W0, 3) and r.levels[0] == (H0, W0)
            for rnd in range(2 if cache_bytes == 1 << 30 else 1):            # the second pass comes from the cache
                for win in wins:
                    for out in _outs(name):
                        st = {}
                        got = r.read(*win, level=level, out=out, stats=st)
                        assert _eq(got, _region(name, level, win, out)), (cache_bytes, rnd, win, out)
                        assert st["tiles"] == [(level, t) for t in codec.window_tiles(ix, *win)]
                        coded = len(codec._coded_tiles(ix, [t for _, t in st["tiles"]]))
                        assert st["hits"] + st["decoded"] == coded
                        if cache_bytes == 0 or coded * _tile_bytes(ix) > cache_bytes:
                            assert st["hits"] == 0 and st["decoded"] == coded
                        elif cache_bytes == 1 << 30 and (rnd or out is not None):
                            assert st["decoded"] == 0 and st["decode_batches"] == 0
            assert r._used <= cache_bytes and r.stats["decoded"] >= 1
    assert r._closed and not r._slabs
    with pytest.raises(ValueError, match="closed"):
        r.read(0, 0, 1, 1)


def test_refusals_are_those_of_decompress_region_and_the_readers_own():
    model = _model()
    with codec.ImageReader(model, _stream_of("pyramid"), batch=BATCH) as r:
        assert r.levels == [(330, 530), (165, 265), (83, 133), (42, 67)] and r.kind == codec.KIND_U8_HWC
        assert r.index(2)["grid"]["n"] == 2 and r.index(2) == dict(codec.stream_index(_stream_of("pyramid"), level=2),
                                                                   index_bytes=r.index(2)["index_bytes"])
        for bad in (4, -1):
            with pytest.raises(ValueError, match="levels 0 .. 3"):
                r.read(0, 0, 8, 8, level=bad)
            with pytest.raises(ValueError, match="levels 0 .. 3"):
                r.read(0, 0, 8, 8, size=(4, 4), level=bad)
        with pytest.raises(ValueError, match="window"):
            r.read(0, 0, 166, 8, level=1)
        with pytest.raises(ValueError, match="window"):
            r.read(0, 0, 331, 8, size=(4, 4))
        with pytest.raises(ValueError, match="resampling"):
            r.read(0, 0, 8, 8, size=(4, 4), resampling="cubic")
        for size in ((0, 4), (4,), (4.5, 4), "ab", (4, -1)):
            with pytest.raises(ValueError, match="size"):
                r.read(0, 0, 8, 8, size=size)
        with pytest.raises(ValueError, match="out="):
            r.read(0, 0, 8, 8, out="u4")
        with pytest.raises(ValueError, match="u16"):
            r.read(0, 0, 8, 8, out="u16")
    with pytest.raises(ValueError, match="one image"):
        codec.ImageReader(model, _stream_of("plain")).read(0, 0, 8, 8, level=1)
    with pytest.raises(codec.EntropyError, match="model"):
        codec.ImageReader(_model(M=128), _stream_of("plain")).read(0, 0, 8, 8)
    with pytest.raises(ValueError, match="trailing"):
        codec.ImageReader(model, _stream_of("pyramid") + b"\0")


def _span_bytes(ix, tiles):
    return sum(n for _, n in codec.tile_spans(ix, tiles))


def test_the_counters_tell_hits_from_decodes_and_the_index_is_read_once():
    model, stream = _model(), _stream_of("pyramid")
    f = Recording(stream)
    r = codec.ImageReader(model, f, batch=BATCH)
    ix = r.index(0)
    opened = r.stats["bytes_read"]
    assert opened == sum(n for _, n in f.reads) and ix["index_bytes"] < opened
    a, b = {}, {}
    r.read(10, 10, 200, 200, stats=a)
    assert [t for _, t in a["tiles"]] == [0, 1, 5, 6] and (a["hits"], a["decoded"], a["decode_batches"]) == (0, 4, 1)
    assert a["bytes_read"] == _span_bytes(ix, [0, 1, 5, 6]) and a["bytes_uploaded"] > 0     # the index was read before
    r.read(10, 10, 200, 200, stats=b)                                        # the same again: nothing to do
    assert (b["hits"], b["decoded"], b["decode_batches"], b["bytes_read"], b["bytes_uploaded"]) == (4, 0, 0, 0, 0)
    c = {}
    r.read(10, 138, 200, 200, stats=c)                                       # one tile column to the right
    assert [t for _, t in c["tiles"]] == [1, 2, 6, 7] and (c["hits"], c["decoded"], c["decode_batches"]) == (2, 2, 1)
    assert c["bytes_read"] == _span_bytes(ix, [2, 7])                        # exactly the new column's strings
    d, e = {}, {}
    r.read(0, 0, 100, 100, level=1, stats=d)                                 # a level's index: on first use, once
    ix1 = r.index(1)
    assert d["bytes_read"] == ix1["index_bytes"] + _span_bytes(ix1, [0]) and d["decoded"] == 1
    r.read(0, 130, 100, 100, level=1, stats=e)
    assert e["bytes_read"] == _span_bytes(ix1, [1]) and (e["hits"], e["decoded"]) == (0, 1)
    assert r.stats["bytes_read"] == sum(n for _, n in f.reads)
    assert (r.stats["tiles"], r.stats["hits"], r.stats["decoded"], r.stats["decode_batches"]) == (14, 6, 8, 4)
    r.close()


def test_hits_and_decodes_follow_the_cache_model():
    model, stream = _model(), _stream_of("pyramid")
    ix = codec.stream_index(stream)
    assert _tile_bytes(ix) == _tile_bytes(codec.stream_index(stream, level=1))   # levels 0 and 1: tiles of one size
    script = [(0, (10, 10, 200, 200)), (1, (0, 0, 100, 200)), (0, (10, 138, 200, 200)), (0, (10, 10, 200, 200)),
              (0, (0, 0, 330, 530)), (1, (100, 100, 60, 160)), (0, (200, 300, 130, 230)), (0, (10, 10, 100, 100)),
              (1, (0, 0, 165, 265)), (0, (10, 10, 200, 200)), (0, (130, 10, 10, 500))]
    model_lru = V.LRU(6)
    with codec.ImageReader(model, stream, cache_bytes=6 * _tile_bytes(ix) + 100, batch=BATCH) as r:
        for step, (level, win) in enumerate(script):
            st = {}
            got = r.read(*win, level=level, stats=st)
            assert (st["hits"], st["decoded"]) == model_lru.call(st["tiles"]), (step, st)
            assert sorted(r._lru) == sorted(model_lru.order) and list(r._lru)[-1] == model_lru.order[-1]
            assert _eq(got, _region("pyramid", level, win, None)), step
        assert r.stats["hits"] > 0 and r.stats["decoded"] > 15 and r._used == 6 * _tile_bytes(ix)


def test_read_many_shares_the_decode_batches():
    model, stream = _model(), _stream_of("pyramid")
    reqs = [{"window": (5, 5, 20, 20)}, {"window": (100, 100, 60, 200)}, {"window": (300, 500, 30, 30)},
            {"window": (0, 0, 60, 60), "level": 1}, {"window": (130, 10, 30, 250), "level": 1},
            {"window": (16, 24, 256, 400), "size": (64, 100)}, {"window": (5, 5, 20, 20)},
            {"window": (200, 0, 100, 530), "size": (25, 130)}]
    with codec.ImageReader(model, stream, batch=BATCH) as one:
        want = [one.read(*q["window"], size=q.get("size"), level=q.get("level")) for q in reqs]
    with codec.ImageReader(model, stream, batch=BATCH) as r:
        warm = {}
        r.read(5, 5, 20, 20, stats=warm)                                     # tile 0 of level 0 is there already
        st = {}
        got = r.read_many(reqs, stats=st)
        assert len(got) == len(want) and all(_eq(g, w) for g, w in zip(got, want))
        need = {}
        for level, t in st["tiles"]:
            need.setdefault(level, set()).add(t)
        assert len(st["tiles"]) == sum(len(v) for v in need.values()) and sorted(need) == [0, 1, 2]
        missing = {l: len(v - ({t for _, t in warm["tiles"]} if l == 0 else set())) for l, v in need.items()}
        assert st["decoded"] == sum(missing.values()) and st["hits"] == len(warm["tiles"])
        assert st["decode_batches"] == sum(-(-m // BATCH) for m in missing.values())
        assert missing[0] > BATCH                                            # more than one batch at level 0
        again = {}
        assert all(_eq(g, w) for g, w in zip(r.read_many(reqs, stats=again), want))
        assert (again["decoded"], again["decode_batches"], again["bytes_read"]) == (0, 0, 0)
    with codec.ImageReader(model, stream, cache_bytes=3 * _tile_bytes(codec.stream_index(stream)), batch=BATCH) as r:
        assert all(_eq(g, w) for g, w in zip(r.read_many(reqs), want))       # the union does not fit: one by one


VIEWS = [((16, 24, 256, 400), (64, 100), None, "average", 2), ((100, 200, 20, 30), (50, 77), None, "average", 0),
         ((3, 5, 300, 500), (150, 250), None, "average", 1), ((7, 9, 200, 333), (77, 100), None, "nearest", 1),
         ((0, 0, 64, 64), (10, 10), 0, "average", 0), ((1, 2, 329, 528), (41, 66), None, "average", 3),
         ((40, 50, 33, 35), (33, 35), None, "average", 0)]


@pytest.mark.parametrize("win,size,level,resampling,picked", VIEWS)
def test_a_resampled_read_is_the_restatement_of_the_covering_window(win, size, level, resampling, picked):
    model, stream = _model(), _stream_of("pyramid")
    assert codec.view_level(4, win[2], win[3], *size) == V.view_level(4, win[2], win[3], *size)
    assert (codec.view_level(4, win[2], win[3], *size) if level is None else level) == picked
    lw = codec.level_window(picked, *win)
    with codec.ImageReader(model, stream, batch=BATCH) as r:
        for out in (None, "f32"):
            st = {}
            got = r.read(*win, size=size, level=level, out=out, resampling=resampling, stats=st)
            src = _region("pyramid", picked, lw, out)
            assert (st["level"], st["level_window"]) == (picked, lw)
            if size == (win[2], win[3]) and picked == 0:
                assert _eq(got, src)                                         # the resample is skipped
                continue
            want = V.resample(src.cpu().numpy(), lw[0], lw[1], picked, win, size, resampling)
            assert got.is_cuda and got.is_contiguous()
            _same(got.cpu().numpy().ravel(), want, f"{win} -> {size} {out}")


def test_averaging_a_nodata_stream_keeps_nodata_out():
    model, stream = _model(), _stream_of("nodata")
    ix = codec.stream_index(stream)
    assert ix["tiles"][0]["state"] == 0 and any(t["state"] == 2 for t in ix["tiles"])
    with codec.ImageReader(model, stream, batch=BATCH) as r:
        inside = r.read(0, 0, 128, 128, size=(16, 16))                       # every footprint inside the empty tile
        assert inside.dtype == torch.uint8 and bool((inside == NODATA).all())
        for out, value in ((None, NODATA), ("f32", float(np.float32(NODATA) / np.float32(255)))):
            win, size = (0, 0, H0, W0), (33, 53)
            got = r.read(*win, size=size, out=out)
            src = _region("nodata", 0, win, out).cpu().numpy()
            _same(got.cpu().numpy().ravel(), V.resample(src, 0, 0, 0, win, size, nodata=value), f"nodata {out}")
            near = r.read(*win, size=size, out=out, resampling="nearest")
            _same(near.cpu().numpy().ravel(), V.resample(src, 0, 0, 0, win, size, "nearest"), f"nearest {out}")
        px = got[:, 0, 0]
        assert bool((px == px[0]).all()) and float(px[0]) == float(np.float32(NODATA) / np.float32(255))


def test_the_tool_writes_the_resampled_window(tmp_path):
    model, stream = _model(), _stream_of("pyramid")
    sd = _PCACHE[("model", 3, 128, 192)][1]
    torch.save({"model": {k: torch.from_numpy(v) for k, v in sd.items()}}, tmp_path / "ckpt.pt")
    (tmp_path / "s.dsic").write_bytes(stream)
    tool = os.path.join(ROOT, "tools", "dsic_image.py")
    r = subprocess.run([sys.executable, tool, "decompress", str(tmp_path / "s.dsic"), str(tmp_path / "view.npy"),
                        "--weights", str(tmp_path / "ckpt.pt"), "--batch", str(BATCH), "--region", "16,24,256,400",
                        "--size", "64,100", "--resampling", "average"], cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    with codec.ImageReader(model, io.BytesIO(stream), batch=BATCH) as reader:
        want = reader.read(16, 24, 256, 400, size=(64, 100))
    assert np.array_equal(np.load(tmp_path / "view.npy"), want.cpu().numpy()) and want.shape == (64, 100, 3)
    assert "64x100" in r.stdout and "level 2" in r.stdout
