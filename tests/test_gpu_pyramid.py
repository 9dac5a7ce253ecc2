"""Image overviews on the GPU.  The two halving kernels alone, bit for bit against the NumPy restatement of
tests/pyramid_ref.py, outputs between guards and inputs inside a larger allocation as in test_gpu_codec_movers.py;
then the pyramid of codec.py on a 330 x 530 scene with the synthetic model of test_gpu_region_decode.py (tile 128,
batch 5, overviews 3: 15 + 6 + 2 + 1 tiles): every level's bytes are the stream compress_image writes for that
level's restated image, and every level decodes, whole and by window, as that stream does alone.

overlap = 32 runs with overviews = 2: level 3 of the scene is 42 x 67, one tile of 48 x 80, and compress_image refuses
an overlap over half a tile side for that image on its own, so the pyramid call refuses it too
(test_pyramid_cpu.py::test_compress_image_checks_every_level_before_it_touches_the_device)."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pyramid_ref as P
from dsic_amd import codec, lib
from dsic_amd import synthetic as S
from dsic_amd.entropy import EntropyError
from dsic_amd.model import CompressionModel
from dsic_amd.ops import _p, _stream

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GUARD = 64                                   # elements on either side of an output and around an input
U8_GUARD, U8_FILL, U8_PAD = 0xCD, 0x5A, 0xEE
F32_FILL, F32_PAD = -7.0, 1e30
SIZES = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 5), (17, 33), (33, 35), (40, 34), (64, 36), (50, 100), (70, 1030)]
# uint8: 1 .. 4 channels are the instantiations with a window path, 5 goes tap by tap with C at run time
KINDS = [("u8", 1), ("u8", 2), ("u8", 3), ("u8", 4), ("u8", 5), ("f32", 1), ("f32", 3), ("f32", 4)]
_CACHE = {}


class Out:
    """n elements between guards inside one device allocation, `offset` elements past a 16-byte aligned point, the
    interior pre-filled (float32: NaN guards, a finite fill; uint8: 0xCD guards, another fill)."""

    def __init__(self, n, dtype, offset=0):
        self.dtype, self.n, self.lo = np.dtype(dtype), int(n), GUARD + offset
        f32 = self.dtype == np.float32
        host = np.full(self.lo + self.n + GUARD, np.nan if f32 else U8_GUARD, dtype=self.dtype)
        host[self.lo:self.lo + self.n] = F32_FILL if f32 else U8_FILL
        self.buf = torch.from_numpy(host).cuda()
        self.view = self.buf[self.lo:self.lo + self.n]

    def host(self, what):
        """The interior on the host, after the guards have been checked."""
        a = self.buf.cpu().numpy()
        g = np.concatenate([a[:self.lo], a[self.lo + self.n:]])
        assert (np.isnan(g) if self.dtype == np.float32 else g == U8_GUARD).all(), f"{what}: guard overwritten"
        return a[self.lo:self.lo + self.n]


def _inside(arr, offset):
    """The array's elements on the device, `offset` elements past an aligned point of a larger allocation."""
    flat = np.ascontiguousarray(arr).ravel()
    host = np.full(GUARD + offset + flat.size + GUARD, F32_PAD if flat.dtype == np.float32 else U8_PAD, dtype=flat.dtype)
    host[GUARD + offset:GUARD + offset + flat.size] = flat
    return torch.from_numpy(host).cuda()[GUARD + offset:GUARD + offset + flat.size]


def _same(got, want, what):
    """bit for bit (a float32 -0.0 is not 0.0, and a NaN is its bits)"""
    want = np.ascontiguousarray(want).ravel()
    assert got.dtype == want.dtype and got.size == want.size, what
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero((got.view(np.uint8).reshape(got.size, -1) != want.view(np.uint8).reshape(got.size, -1))
                             .any(axis=1))
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {got.size} differ, first at {i}: got {got[i]!r}, want {want[i]!r}")


# ---- the kernels ----------------------------------------------------------------------------------------------------
def _kernel_image(H, W, kind, C):
    """uint8: random bytes with 0 and 255 blocks.  float32: random values in [0, 1) with, where the image has room,
    a NaN at (0, 0), -0.0 over the 2 x 2 block at rows 0-1, columns 2-3, denormals over the block at columns 4-5 and
    at the last pixel (so they meet the repeated row and column of an odd side), in every plane."""
    rng = np.random.default_rng(H * 100003 + W * 101 + C)
    if kind == "u8":
        img = rng.integers(0, 256, size=(H, W, C), dtype=np.uint8)
        img[:2, :2] = 255
        img[-1:, -2:] = 0
        return img
    img = rng.random((C, H, W), dtype=np.float32)
    tiny = np.float32(1e-45)                                             # the smallest denormal
    img[:, -1, -1] = tiny * 3
    if W >= 4:
        img[:, :2, 2:4] = -0.0
    if W >= 6:
        img[:, :2, 4:6] = np.array([[1, 2], [3, 5]], dtype=np.float32)[:H] * tiny
    img[:, 0, 0] = np.nan
    return img


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("kind,C", KINDS)
def test_halving_kernels_equal_the_restatement(H, W, kind, C):
    L = lib.load()
    img = _kernel_image(H, W, kind, C)
    want = P.halve(img)
    assert want.shape == ((P.halved(H), P.halved(W), C) if kind == "u8" else (C, P.halved(H), P.halved(W)))
    if kind == "f32":
        assert np.isnan(want[:, 0, 0]).all() and np.isnan(want).sum() == C
        if W >= 6 and H >= 2:
            assert np.signbit(want[0, 0, 1]) and want[0, 0, 1] == 0 and 0 < want[0, 0, 2] < 1e-44
    # the input at every element offset; the output at offsets that move its ragged head and tail
    for off, out_off in zip(range(4), (0, 1, 7, 15) if kind == "u8" else (0, 1, 2, 3)):
        src = _inside(img, off)
        out = Out(want.size, img.dtype, out_off)
        if kind == "u8":
            lib.check(L.dsic_image_halve_u8(_p(src), _p(out.view), H, W, C, _stream()), "image_halve_u8")
        else:
            lib.check(L.dsic_image_halve_f32(_p(src), _p(out.view), C, H, W, _stream()), "image_halve_f32")
        what = f"image_halve_{kind} {H}x{W}x{C}, input offset {off}, output offset {out_off}"
        _same(out.host(what), want, what)


def test_halving_calls_refuse_overlapping_images():
    L = lib.load()
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    assert L.dsic_image_halve_u8(_p(buf), _p(buf[40:]), 4, 4, 3, _stream()) == lib.DSIC_EINVAL
    assert L.dsic_image_halve_f32(_p(buf), _p(buf[188:]), 3, 4, 4, _stream()) == lib.DSIC_EINVAL
    with pytest.raises(ValueError, match="overlap"):
        lib.check(L.dsic_image_halve_u8(_p(buf[8:]), _p(buf), 4, 4, 3, _stream()), "image_halve_u8")
    assert not bool(buf.any())


# ---- the pyramid ----------------------------------------------------------------------------------------------------
H0, W0, TILE, BATCH, LEVELS = 330, 530, 128, 5, 3
ARGS = {"tile": TILE, "batch": BATCH}


def _model(in_ch=3, N=128, M=192):
    key = ("model", in_ch, N, M)
    if key not in _CACHE:
        sd = S.make_state_dict(seed=1, N=N, M=M, in_ch=in_ch, spatial_params=False)
        m = CompressionModel(N=N, M=M, spatial_params=False, min_nu=2, max_nu=100.0, in_ch=in_ch)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        _CACHE[key] = (m.cuda().eval(), sd)
    return _CACHE[key][0]


def _chain(kind):
    """The scene and its restated levels, NumPy, read-only: [level 0, ..., level 4]."""
    if ("chain", kind) not in _CACHE:
        x = S.make_patches(21, 1, H0, W0, 3)[0].astype(np.float32)       # [3, H, W] in [0, 1]
        img = np.ascontiguousarray((x * 255.0 + 0.5).astype(np.uint8).transpose(1, 2, 0)) if kind == "u8" else x
        levels = P.chain(img, 4)
        for a in levels:
            a.setflags(write=False)
        _CACHE[("chain", kind)] = levels
    return _CACHE[("chain", kind)]


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _pyramid(kind="u8", overviews=LEVELS, **kw):
    """(the DSICP stream of the scene, its unpacked levels), coded once per set of arguments"""
    key = ("pyramid", kind, overviews, tuple(sorted(kw.items())))
    if key not in _CACHE:
        stream = codec.compress_image(_model(), _dev(_chain(kind)[0]), overviews=overviews, **ARGS, **kw)
        _CACHE[key] = (stream, codec.unpack_pyramid_stream(stream)["levels"])
    return _CACHE[key]


def _alone(kind, level, **kw):
    """compress_image of the restated level image on its own"""
    key = ("alone", kind, level, tuple(sorted(kw.items())))
    if key not in _CACHE:
        _CACHE[key] = codec.compress_image(_model(), _dev(_chain(kind)[level]), **ARGS, **kw)
    return _CACHE[key]


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_build_overviews_equals_the_restated_chain(kind):
    want = _chain(kind)
    got = codec.build_overviews(_dev(want[0]), 4)
    assert len(got) == 5 and [tuple(g.shape) for g in got] == [w.shape for w in want]
    assert [w.shape[:2] if kind == "u8" else w.shape[1:] for w in want] == codec.overview_shapes(H0, W0, 4)
    for l, (g, w) in enumerate(zip(got, want)):
        assert g.is_cuda and g.is_contiguous()
        _same(g.cpu().numpy().ravel(), w, f"{kind} level {l}")
    assert len(codec.build_overviews(_dev(want[0]), 0)) == 1


@pytest.mark.parametrize("kind,overviews,kw", [("u8", 3, {}), ("u8", 3, {"segments": 4}), ("u8", 2, {"overlap": 32}),
                                               ("f32", 3, {})])
def test_every_level_is_the_stream_of_its_image(kind, overviews, kw):
    stream, levels = _pyramid(kind, overviews, **kw)
    assert stream[:6] == b"DSICP\0" and len(levels) == overviews + 1
    for l, lv in enumerate(levels):
        assert (lv["H"], lv["W"]) == P.shapes(H0, W0, overviews)[l]
        assert lv["stream"] == _alone(kind, l, **kw), f"level {l}"
        h = codec.unpack_image_stream(lv["stream"])
        assert h["kind"] == (0 if kind == "u8" else 1) and h["segments"] == kw.get("segments", 1)
        assert h["overlap"] == kw.get("overlap", 0)
    if not kw and overviews == 3:
        assert [codec.stream_index(stream, level=l)["grid"]["n"] for l in range(4)] == [15, 6, 2, 1]


def test_no_overviews_is_the_stream_of_today():
    img = _dev(_chain("u8")[0])
    plain = codec.compress_image(_model(), img, **ARGS)
    assert codec.compress_image(_model(), img, overviews=0, **ARGS) == plain == _alone("u8", 0)
    assert plain[:6] == b"DSICI\0"
    # the image may come from the host: it is uploaded once and halved on the device
    assert codec.compress_image(_model(), img.cpu(), overviews=LEVELS, **ARGS) == _pyramid()[0]


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_a_level_decodes_as_its_stream_alone(kind):
    model = _model()
    stream, levels = _pyramid(kind)
    for l, lv in enumerate(levels):
        for out in (None, "u8", "f32"):
            got = codec.decompress_image(model, stream, out=out, level=l)
            want = codec.decompress_image(model, lv["stream"], out=out)
            assert got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want), (l, out)
        assert tuple(got.shape) == (3, lv["H"], lv["W"])
    # level 0 is the default, and it is the decode of the plain stream
    plain = codec.decompress_image(model, _alone(kind, 0))
    assert torch.equal(codec.decompress_image(model, stream), plain)
    assert plain.dtype == (torch.uint8 if kind == "u8" else torch.float32)
    assert torch.equal(codec.decompress_region(model, stream, 7, 9, 100, 200), _crop(plain, (7, 9, 100, 200)))


def _crop(full, win):
    y0, x0, h, w = win
    return full[y0:y0 + h, x0:x0 + w] if full.dtype == torch.uint8 else full[:, y0:y0 + h, x0:x0 + w]


def _windows(h, w):
    """the two corner pixels, the whole level, and a window that crosses the tile seams where the level has any"""
    return [(0, 0, 1, 1), (h - 1, w - 1, 1, 1), (0, 0, h, w), (h // 3, w // 5, h // 2, w // 2)]


@pytest.mark.parametrize("level", [0, 1, 3])
def test_a_window_of_a_level_is_the_crop_of_its_decode(level):
    model = _model()
    stream, levels = _pyramid()
    h, w = levels[level]["H"], levels[level]["W"]
    full = {out: codec.decompress_image(model, stream, out=out, level=level) for out in (None, "f32")}
    for win in _windows(h, w):
        for out in (None, "f32"):
            stats = {}
            got = codec.decompress_region(model, stream, *win, out=out, stats=stats, level=level)
            assert torch.equal(got, _crop(full[out], win)), (level, win, out)
    if level < 3:                                                        # the last window met more than one tile
        assert len(stats["tiles"]) >= 4
    with pytest.raises(ValueError, match="window"):                      # the window counts in the level's own grid
        codec.decompress_region(model, stream, 0, 0, h + 1, w, level=level)
    if level:
        y0, x0, hh, ww = codec.level_window(level, 100, 200, 64, 64)
        assert codec.decompress_region(model, stream, y0, x0, hh, ww, level=level).shape == (hh, ww, 3)


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


@pytest.mark.parametrize("level,win", [(0, (100, 100, 60, 200)), (1, (0, 0, 165, 265)), (2, (80, 3, 3, 100)),
                                       (3, (41, 66, 1, 1))])
def test_a_file_is_read_only_at_the_directory_and_the_chosen_level(level, win):
    model = _model()
    stream, levels = _pyramid()
    end = 12 + 24 * len(levels)
    lo, hi = levels[level]["offset"], levels[level]["offset"] + levels[level]["length"]
    f, stats = Recording(stream), {}
    got = codec.decompress_region(model, f, *win, stats=stats, level=level)
    assert torch.equal(got, codec.decompress_region(model, stream, *win, level=level))
    assert f.reads and sum(n for _, n in f.reads) == stats["bytes_read"]
    for pos, n in f.reads:
        assert pos + n <= end or (lo <= pos and pos + n <= hi), f"read of {n} bytes at {pos}: level {level} is [{lo}, {hi})"
    ix = codec.stream_index(stream, level=level)
    spans = codec.tile_spans(ix, stats["tiles"])
    assert all(lo <= o and o + n <= hi for o, n in spans)
    assert stats["bytes_read"] == ix["index_bytes"] + sum(n for _, n in spans)
    if len(stats["tiles"]) < ix["grid"]["n"]:
        assert stats["bytes_read"] < end + levels[level]["length"]


def test_max_error_bounds_level_0_and_leaves_the_overviews_lossy():
    model = _model()
    u8 = _chain("u8")[0]
    stream, levels = _pyramid(max_error=2)
    assert levels[0]["stream"] == _alone("u8", 0, max_error=2)
    assert codec.unpack_image_stream(levels[0]["stream"])["version"] == 4
    for out in (None, "u8"):
        dec = codec.decompress_image(model, stream, out=out)
        err = (dec.cpu().numpy().astype(np.int32) - u8.astype(np.int32))
        assert dec.dtype == torch.uint8 and np.abs(err).max() <= 2, np.abs(err).max()
    win = (100, 100, 60, 200)
    assert torch.equal(codec.decompress_region(model, stream, *win), _crop(dec, win))
    for l in (1, 2, 3):
        h = codec.unpack_image_stream(levels[l]["stream"])
        assert h["version"] < 4 and "max_error" not in h and "residuals" not in h
        assert levels[l]["stream"] == _alone("u8", l)                     # the lossy stream of the level
    ix = codec.stream_index(stream)
    assert ix["max_error"] == 2 and "max_error" not in codec.stream_index(stream, level=1)


def test_refusals():
    model = _model()
    stream, _ = _pyramid()
    plain = _alone("u8", 0)
    for bad in (4, -1):
        with pytest.raises(ValueError, match="levels 0 .. 3"):
            codec.decompress_image(model, stream, level=bad)
        with pytest.raises(ValueError, match="levels 0 .. 3"):
            codec.decompress_region(model, stream, 0, 0, 8, 8, level=bad)
    with pytest.raises(ValueError, match="one image"):
        codec.decompress_image(model, plain, level=1)
    with pytest.raises(ValueError, match="one image"):
        codec.decompress_region(model, plain, 0, 0, 8, 8, level=1)
    assert codec.decompress_image(model, plain, level=0).shape == (H0, W0, 3)
    for other in (_model(M=128), _model(N=64)):
        for l in (0, 2):
            with pytest.raises(EntropyError, match="model"):
                codec.decompress_image(other, stream, level=l)
    with pytest.raises(RuntimeError, match="GPU"):
        codec.build_overviews(torch.from_numpy(np.array(_chain("u8")[0])), 2)
    with pytest.raises(ValueError, match="trailing"):
        codec.decompress_image(model, stream + b"\0", level=1)
    with pytest.raises(ValueError, match="level 5"):
        codec.compress_image(model, _dev(_chain("u8")[0]), overviews=5, **ARGS)


def test_command_line_round_trip(tmp_path):
    model = _model()
    sd = _CACHE[("model", 3, 128, 192)][1]
    torch.save({"model": {k: torch.from_numpy(v) for k, v in sd.items()}}, tmp_path / "ckpt.pt")
    u8 = np.ascontiguousarray((S.make_patches(71, 1, 150, 170, 3)[0] * 255.0 + 0.5).astype(np.uint8).transpose(1, 2, 0))
    np.save(tmp_path / "in.npy", u8)
    tool = os.path.join(ROOT, "tools", "dsic_image.py")
    w = ["--weights", str(tmp_path / "ckpt.pt")]
    region = (5, 6, 20, 30)                                              # level 2 is 38 x 43
    runs = (["compress", str(tmp_path / "in.npy"), str(tmp_path / "s.dsic"), "--tile", "64", "--batch", "4",
             "--overviews", "2"] + w,
            ["info", str(tmp_path / "s.dsic")],
            ["decompress", str(tmp_path / "s.dsic"), str(tmp_path / "win.npy"), "--level", "2", "--region",
             ",".join(str(v) for v in region)] + w)
    outs = []
    for args in runs:
        r = subprocess.run([sys.executable, tool, *args], cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        outs.append(r.stdout)
    stream = codec.compress_image(model, torch.from_numpy(u8), tile=64, batch=4, overviews=2)
    assert (tmp_path / "s.dsic").read_bytes() == stream
    want = codec.decompress_region(model, stream, *region, level=2)
    assert np.array_equal(np.load(tmp_path / "win.npy"), want.cpu().numpy()) and want.shape == (20, 30, 3)
    info = outs[1]
    levels = codec.unpack_pyramid_stream(stream)["levels"]
    for l, (size, tiles) in enumerate((("150x170", 9), ("75x85", 4), ("38x43", 1))):
        assert f"level {l}: {size}, {levels[l]['length']} bytes" in info and f"{tiles} tile(s)" in info, info
    assert "of level 2" in outs[2]
