"""The rendered views without a GPU: the restatement of tests/render_ref.py against its own properties (the stretch is
255 d / R rounded half up, monotone, lo -> 0 and hi -> 255; the percentile rule is a pick from the sorted samples; the
histogram leaves out what it should), codec.stretch_from_histogram against the restatement, the new entry points'
declarations and refusals (which need the library, not a device), the reader's and the tool's argument errors."""
import ctypes
import importlib.util
import os
import re
import types
from fractions import Fraction

import numpy as np
import pytest

import render_ref as R
import view_ref as V
from dsic_amd import codec, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"dsic_window_render_u8": 23, "dsic_window_render_u16": 23, "dsic_band_histogram_u8": 8,
       "dsic_band_histogram_u16": 8}


# ---- the stretch ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R_", [0, 1, 2, 3, 254, 255, 256, 509, 510, 511, 1000, 10000, 65534, 65535])
def test_the_stretch_is_255_d_over_R_rounded_half_up(R_):
    for lo in {0, 65535 - R_, (65535 - R_) // 3}:
        hi = lo + R_
        d = np.arange(R_ + 1, dtype=np.int64)
        got = R.stretch(lo + d, lo, hi)
        assert got.dtype == np.uint8
        if R_ == 0:
            assert got.tolist() == [0]
            continue
        # every d: the quotient, and one more where the remainder is at least half of R
        assert np.array_equal(got, 255 * d // R_ + (2 * (255 * d % R_) >= R_))
        step = max(1, R_ // 997)                                            # as fractions: every d for small R, else a comb
        for k in sorted(set(range(0, R_ + 1, step)) | {R_ - 1, R_, R_ // 2, R_ // 2 + 1}):
            f = Fraction(255 * k, R_)
            want = f.numerator // f.denominator + (1 if 2 * (f - f.numerator // f.denominator) >= 1 else 0)
            assert int(got[k]) == want, (lo, hi, k)
        assert (np.diff(got.astype(np.int64)) >= 0).all() and got[0] == 0 and got[-1] == 255
    if R_ == 510:
        assert R.stretch(1, 0, 510) == 1 and R.stretch(0, 0, 510) == 0      # 255 / 510 is the exact half: up
        assert R.stretch(3, 0, 510) == 2                                    # 1.5 -> 2


def test_the_stretch_clips_outside_the_pair_and_fits_32_bits():
    assert R.stretch(np.array([0, 99, 100, 150, 200, 201, 65535]), 100, 200).tolist() == [0, 0, 0, 128, 255, 255, 255]
    assert R.stretch(np.array([0, 7, 65535]), 7, 7).tolist() == [0, 0, 0]
    assert 510 * 65535 + 65535 < 2 ** 32
    m = np.arange(65536)
    full = R.stretch(m, 0, 65535)
    assert full[0] == 0 and full[65535] == 255 and full[128] == 0 and full[129] == 1      # 255 * 129 / 65535 = 0.502
    assert np.array_equal(R.stretch(np.arange(256), 0, 255), np.arange(256))


def test_display_picks_bands_and_marks_invalid_pixels():
    img = np.arange(2 * 3 * 4, dtype=np.uint16).reshape(2, 3, 4) * 1000
    pairs = [(0, 23000), (0, 65535), (5000, 5000), (3000, 19000)]
    valid = np.array([[1, 0, 1], [1, 1, 0]], dtype=np.uint8)
    out = R.display(img, valid, (3, 0, 0), pairs, alpha=True, background=200)
    assert out.shape == (2, 3, 4) and out.dtype == np.uint8
    assert out[0, 1].tolist() == [200, 200, 200, 0] and out[1, 2].tolist() == [200, 200, 200, 0]
    assert out[0, 0].tolist() == [0, 0, 0, 255] and out[1, 1].tolist() == [255, int(R.stretch(16000, 0, 23000)),
                                                                          int(R.stretch(16000, 0, 23000)), 255]
    grey = R.display(img, None, (2,), pairs)
    assert grey.shape == (2, 3, 1) and not grey.any()                       # lo == hi
    # a render is the display of the resample, and with all pixels valid the mask changes nothing
    src = V.kernel_image("u16", 4, 9, 11)
    args = (src, 0, 0, 0, (0, 0, 9, 11), (4, 5), (0, 1, 2), pairs)
    plain = R.render(args[0], None, *args[1:])
    assert np.array_equal(plain, R.display(V.resample(src, 0, 0, 0, (0, 0, 9, 11), (4, 5)), None, (0, 1, 2), pairs))
    assert np.array_equal(R.render(args[0], np.ones((9, 11), np.uint8), *args[1:]), plain)


# ---- histogram and percentiles --------------------------------------------------------------------------------------
def test_the_histogram_leaves_out_invalid_and_nodata_pixels():
    img = np.array([[[1, 2, 3], [7, 7, 7]], [[7, 7, 8], [255, 0, 7]]], dtype=np.uint8)
    h = R.histogram(img)
    assert h.shape == (3, 256) and h.dtype == np.int64 and h.sum(axis=1).tolist() == [4, 4, 4] and h[0, 7] == 2
    h = R.histogram(img, nodata=7)
    assert h.sum(axis=1).tolist() == [3, 3, 3] and (h[0, 7], h[2, 7], h[2, 8]) == (1, 1, 1)   # one channel differs: counted
    h = R.histogram(img, valid=np.array([[1, 0], [0, 3]]))
    assert h.sum(axis=1).tolist() == [2, 2, 2] and h[0, 255] == 1 and h[0, 1] == 1
    assert R.histogram(img, valid=np.zeros((2, 2))).sum() == 0
    assert R.histogram(img.astype(np.uint16) * 257).shape == (3, 65536)


def _brute(samples, percent):
    """the pick from the sorted samples: the max(1, ceil(q n / 10000))-th smallest"""
    if not len(samples):
        return (0, 0)
    s = sorted(int(v) for v in samples)
    n = len(s)
    return tuple(s[max(1, -(-int(round(100 * p)) * n // 10000)) - 1] for p in percent)


PERCENTS = [(2, 98), (0, 100), (0, 0), (100, 100), (50, 50), (0.01, 99.99), (33.33, 66.67), (1, 1), (99.5, 100)]


def test_the_percentile_rule_is_a_pick_from_the_sorted_samples():
    rng = np.random.default_rng(11)
    cases = [np.array([], dtype=np.int64), np.array([5]), np.full(40, 200), np.array([0, 255]), np.array([3, 3, 9]),
             rng.integers(0, 256, size=1000), rng.integers(100, 110, size=37), np.arange(256).repeat(3),
             np.concatenate([np.zeros(500, dtype=np.int64), [255]]), rng.integers(0, 65536, size=300)]
    for samples in cases:
        bins = 65536 if samples.size and samples.max() > 255 else 256
        hist = np.stack([np.bincount(samples, minlength=bins), np.bincount(samples[::2], minlength=bins)])
        for percent in PERCENTS:
            want = [_brute(samples, percent), _brute(samples[::2], percent)]
            assert R.percentile_stretch(hist, percent) == want, (samples[:5], percent)
            got = codec.stretch_from_histogram(hist, percent)
            assert got == want and all(type(v) is int for pair in got for v in pair)
            assert all(lo <= hi for lo, hi in got)
    one = np.bincount([4, 9, 9, 200], minlength=256)[None]
    assert codec.stretch_from_histogram(one, (0, 100)) == [(4, 200)]        # minimum and maximum
    assert codec.stretch_from_histogram(one, (50, 50)) == [(9, 9)] and codec.stretch_from_histogram(one) == [(4, 200)]
    assert codec.stretch_from_histogram(np.zeros((2, 256), dtype=np.int64)) == [(0, 0), (0, 0)]


def test_stretch_from_histogram_refuses_a_bad_percent():
    hist = np.ones((1, 256), dtype=np.int64)
    for bad in ((98, 2), (-1, 50), (0, 100.5), (5,), (1, 2, 3), "ab", None, (float("nan"), 50), ("a", 2)):
        with pytest.raises(ValueError, match="percent"):
            codec.stretch_from_histogram(hist, bad)
    for bad in (np.ones(256), np.ones((1, 256)) * 0.5, -np.ones((1, 4), dtype=np.int64)):
        with pytest.raises(ValueError, match="hist"):
            codec.stretch_from_histogram(bad)


# ---- the exports ----------------------------------------------------------------------------------------------------
def test_the_new_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "dsic_hip.h")).read()
    for name, nargs in NEW.items():
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert decl, name
        assert len(decl.group(1).split(",")) == nargs
        res, args = lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs and getattr(lib.load(), name) is not None
    assert lib.load().dsic_abi_version() == 4


def test_the_render_calls_check_their_arguments_without_a_gpu():
    L = lib.load()
    E, err = lib.DSIC_EINVAL, L.dsic_last_error
    a, b, m = 1 << 20, 1 << 24, 1 << 22         # non-null, aligned, far apart: every call below is refused before a launch
    ok = dict(src=a, val=None, sh=8, sw=8, sy0=0, sx0=0, C=3, shift=0, y0=0, x0=0, h=8, w=8, bands=(0, 1, 2), dst=b, oh=4,
              ow=4, mode=0, nodata=-1, alpha=0, background=0)

    def call(name, lohi=None, **kw):
        p = dict(ok, **kw)
        top = 255 if name == "u8" else 65535
        pairs = [(0, top)] * 4 if lohi is None else lohi
        bands = None if p["bands"] is None else (ctypes.c_int * len(p["bands"]))(*p["bands"])
        flat = None if pairs == "null" else (ctypes.c_uint32 * 8)(*[v for pair in pairs for v in pair])
        return getattr(L, "dsic_window_render_" + name)(
            p["src"], p["val"], p["sh"], p["sw"], p["sy0"], p["sx0"], p["C"], p["shift"], p["y0"], p["x0"], p["h"], p["w"],
            bands, kw.get("nb", 3 if bands is None else len(bands)), flat, p["dst"], p["oh"], p["ow"], p["mode"],
            p["nodata"], p["alpha"], p["background"], None)

    for name, top in (("u8", 255), ("u16", 65535)):
        assert call(name, src=None) == E and b"null" in err()
        assert call(name, dst=None) == E and b"null" in err()
        assert call(name, bands=None, nb=3) == E and b"null" in err()
        assert call(name, lohi="null") == E and b"null" in err()
        for C in (0, 5):
            assert call(name, C=C, bands=(0,)) == E and f"C={C}".encode() in err()
        for nb in (0, 2, 4):
            assert call(name, nb=nb) == E and f"nb={nb}".encode() in err()
        assert call(name, bands=(0, 3, 1)) == E and b"band 3" in err()
        assert call(name, bands=(-1,)) == E and b"band -1" in err()
        assert call(name, C=1, bands=(0, 0, 1)) == E and b"band 1" in err()
        assert call(name, alpha=2) == E and b"alpha=2" in err()
        assert call(name, alpha=-1) == E and b"alpha" in err()
        assert call(name, background=256) == E and b"background=256" in err()
        assert call(name, background=-1) == E and b"background" in err()
        assert call(name, lohi=[(0, top), (9, 8), (0, top), (0, top)]) == E and b"(9, 8)" in err()
        assert call(name, lohi=[(0, top + 1)] + [(0, top)] * 3) == E and f"({0}, {top + 1})".encode() in err()
        # every pair of a band the stream holds is checked, chosen or not
        assert call(name, C=4, bands=(0,), lohi=[(0, top)] * 3 + [(9, 8)]) == E and b"(9, 8)" in err()
        assert call(name, shift=16) == E and b"shift=16" in err()
        assert call(name, mode=2) == E and b"mode=2" in err()
        assert call(name, oh=0) == E and b"output" in err()
        assert call(name, h=0) == E and b"region" in err()
        assert call(name, h=9) == E and b"outside the source window" in err()
        assert call(name, sx0=2, x0=3, shift=1, w=8, sw=4) == E and b"outside the source window" in err()
        assert call(name, sh=1 << 24, sw=1 << 24, h=(1 << 23) + 1, w=1 << 23) == E and b"2^46" in err()
        assert call(name, nodata=top + 1) == E and f"nodata={top + 1}".encode() in err()
        assert call(name, nodata=-2) == E and b"nodata" in err()
        assert call(name, dst=a + 16) == E and b"overlap" in err()
        assert call(name, val=m, dst=m + 32) == E and b"overlap" in err()  # the validity window is 64 bytes
        assert call(name, val=m, dst=m - 16, alpha=1) == E and b"overlap" in err()     # dst is 4 * 4 * 4 = 64 bytes
    assert call("u16", src=a + 1) == E and b"2-byte aligned" in err()


def test_the_histogram_calls_check_their_arguments_without_a_gpu():
    L = lib.load()
    E, err = lib.DSIC_EINVAL, L.dsic_last_error
    a, b, m = 1 << 20, 1 << 24, 1 << 22
    for name, top, elem in (("u8", 255, 1), ("u16", 65535, 2)):
        fn = getattr(L, "dsic_band_histogram_" + name)
        assert fn(None, None, 4, 4, 3, -1, b, None) == E and b"null" in err()
        assert fn(a, None, 4, 4, 3, -1, None, None) == E and b"null" in err()
        for C in (0, 5):
            assert fn(a, None, 4, 4, C, -1, b, None) == E and f"C={C}".encode() in err()
        assert fn(a, None, 0, 4, 3, -1, b, None) == E and fn(a, None, 4, 0, 3, -1, b, None) == E and b"image" in err()
        assert fn(a, None, 65536, 65536, 1, -1, 1 << 44, None) == E and b"2^32" in err()
        assert fn(a, None, 4, 4, 3, top + 1, b, None) == E and f"nodata={top + 1}".encode() in err()
        assert fn(a, None, 4, 4, 3, -2, b, None) == E and b"nodata" in err()
        assert fn(a, None, 4, 4, 3, -1, b + 2, None) == E and b"aligned" in err()
        assert fn(a, None, 4, 4, 3, -1, a + 16 * 3 * elem - 4, None) == E and b"overlap" in err()
        assert fn(a, None, 4, 4, 3, -1, a - 4 * 3 * (top + 1) + 4, None) == E and b"overlap" in err()
        assert fn(a, m, 4, 4, 3, -1, m + 12, None) == E and b"overlap" in err()
    assert L.dsic_band_histogram_u16(a + 1, None, 4, 4, 3, -1, b, None) == E and b"aligned" in err()


def test_both_render_exports_refuse_faulty_display_arguments_in_the_same_words():
    """One display check behind dsic_window_render_* and dsic_window_warp_render_*: each fault alone, nothing launched."""
    L = lib.load()
    a, b = 1 << 20, 1 << 24
    for name, top in (("u8", 255), ("u16", 65535)):
        good = dict(bands=(0, 1, 2), nb=3, lohi=[(0, top)] * 3, alpha=1, background=0)
        for fault, word in ((dict(nb=2), "nb=2"), (dict(alpha=2), "alpha=2"), (dict(background=256), "background=256"),
                            (dict(bands=None), "null pointer"), (dict(lohi=[(0, top), (9, 8), (0, top)]), "stretch pair (9, 8)"),
                            (dict(lohi=[(0, top + 1)] + [(0, top)] * 2), f"stretch pair (0, {top + 1})"),
                            (dict(bands=(0, 3, 1)), "band 3"), (dict(bands=(-1, 0, 0)), "band -1")):
            p = dict(good, **fault)
            bands = None if p["bands"] is None else (ctypes.c_int * 3)(*p["bands"])
            display = (bands, p["nb"], codec._lohi(p["lohi"]), b, 8, 8, 0, -1, p["alpha"], p["background"], None)
            said = []
            for export, geometry in (("window_render_", (8, 8, 0, 0, 3, 0, 0, 0, 8, 8)),
                                     ("window_warp_render_", (8, 8, 0, 0, 3, 0, 8, 8, 8, 8,
                                                              (ctypes.c_int64 * 6)(65536, 0, 0, 0, 65536, 0)))):
                assert getattr(L, "dsic_" + export + name)(a, None, *geometry, *display) == lib.DSIC_EINVAL, (export, fault)
                head, _, rest = L.dsic_last_error().decode().partition(": ")
                assert head == export + name and rest
                said.append(rest)
            assert said[0] == said[1] and said[0].startswith(word), (name, fault, said)


# ---- the reader's and the tool's argument errors ----------------------------------------------------------------------
def _reader(C, kind, **extra):
    """A reader over nothing, one level open: every refusal below comes before the first read of a tile"""
    r = object.__new__(codec.ImageReader)
    r._closed, r._dir, r._source = False, None, types.SimpleNamespace(bytes_read=0)
    r._open = {0: (None, dict({"C": C, "kind": kind, "H": 64, "W": 64, "version": 1}, **extra), 0)}
    return r


def test_render_refuses_before_any_launch():
    u8, u16 = _reader(3, codec.KIND_U8_HWC), _reader(4, codec.KIND_U16_HWC, scale=[(0, 65535)] * 4, version=6)
    win = (0, 0, 8, 8)
    for r, C, top in ((u8, 3, 255), (u16, 4, 65535)):
        full = [(0, top)] * C
        for bands in ((), (0, 1), (0, 1, 2, 0), (C,), (0, -1, 1), (0.5,), 7, "ab"):
            with pytest.raises(ValueError, match="bands"):
                r.render(*win, bands=bands, stretch=full)
        for stretch in (full[:-1], full + [(0, 1)], [(0, top + 1)] + full[1:], [(5, 4)] + full[1:], [(-1, 4)] + full[1:],
                        [(0, 1, 2)] * C, [(0.5, 3)] * C, 7, [7] * C):
            with pytest.raises(ValueError, match="stretch"):
                r.render(*win, stretch=stretch)
        for background in (-1, 256, 0.5, None):
            with pytest.raises(ValueError, match="background"):
                r.render(*win, stretch=full, background=background)
        with pytest.raises(ValueError, match="resampling"):
            r.render(*win, stretch=full, resampling="cubic")
        with pytest.raises(ValueError, match="size"):
            r.render(*win, stretch=full, size=(0, 4))
        with pytest.raises(ValueError, match="bands"):
            r.render_many([{"window": win, "bands": (0, 1), "stretch": full}])
        with pytest.raises(ValueError, match="stretch"):
            r.render_many([{"window": win, "stretch": full[1:]}])
    with pytest.raises(ValueError, match="stretch pair .0, 256."):         # a uint8 stream's top is 255
        u8.render(*win, stretch=[(0, 256)] * 3)
    nodata = _reader(3, codec.KIND_U8_HWC, nodata=7, version=5)
    with pytest.raises(ValueError, match="valid="):
        nodata.render(*win, alpha=True)
    with pytest.raises(ValueError, match="valid="):
        nodata.render_many([{"window": win}], alpha=True)
    assert {"render", "render_many", "histogram", "stretch"} <= set(dir(codec.ImageReader))
    assert codec.stretch_from_histogram.__module__.endswith("view")


def _tool():
    spec = importlib.util.spec_from_file_location("_dsic_image_tool", os.path.join(ROOT, "tools", "dsic_image.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_the_tools_argument_errors(capsys):
    tool = _tool()
    base = ["render", "a.dsic", "b.npy", "--weights", "w.pt"]
    for extra, word in ((["--bands", "0,1"], "--bands"), (["--bands", "0,1,2,3"], "--bands"), (["--bands", "r"], "--bands"),
                        (["--stretch", "0,9", "--percent", "2,98"], "exclude"), (["--percent", "5"], "--percent"),
                        (["--percent", "98,2"], "--percent"), (["--percent", "0,101"], "--percent"),
                        (["--background", "300"], "--background"), (["--region", "1,2,3"], "--region"),
                        (["--size", "4"], "--size"), (["--out", "u8"], "--out"), (["--scale", "0,1"], "--scale")):
        with pytest.raises(SystemExit) as e:
            tool.main(base + extra)
        assert e.value.code == 2 and word in capsys.readouterr().err, extra
    for dst, extra, word in (("b.jpg", [], ".npy"), ("b.ppm", ["--alpha"], "alpha"), ("b.pgm", ["--alpha"], "alpha")):
        with pytest.raises(SystemExit) as e:
            tool.main(["render", "a.dsic", dst, "--weights", "w.pt"] + extra)
        assert e.value.code == 2 and word in capsys.readouterr().err, dst
    with pytest.raises(SystemExit):                                        # no destination
        tool.main(["render", "a.dsic", "--weights", "w.pt"])
    for extra in (["--bands", "0"], ["--stretch", "0,9"], ["--percent", "2,98"], ["--alpha"], ["--background", "9"]):
        with pytest.raises(SystemExit) as e:                               # render's options are render's alone
            tool.main(["decompress", "a.dsic", "b.npy", "--weights", "w.pt"] + extra)
        assert e.value.code == 2 and "go with render" in capsys.readouterr().err


def test_the_tool_writes_ppm_and_pgm_in_pure_python(tmp_path):
    tool = _tool()
    rgb = np.arange(2 * 3 * 3, dtype=np.uint8).reshape(2, 3, 3) * 14
    tool.write_display(str(tmp_path / "a.ppm"), rgb)
    assert (tmp_path / "a.ppm").read_bytes() == b"P6\n3 2\n255\n" + rgb.tobytes()
    tool.write_display(str(tmp_path / "a.pgm"), rgb[:, :, :1])
    assert (tmp_path / "a.pgm").read_bytes() == b"P5\n3 2\n255\n" + rgb[:, :, 0].tobytes()
    tool.write_display(str(tmp_path / "a.npy"), rgb)
    assert np.array_equal(np.load(tmp_path / "a.npy"), rgb)
