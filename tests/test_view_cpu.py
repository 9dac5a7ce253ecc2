"""The resampled reads without a GPU: the restatement of tests/view_ref.py against its own properties (weights that
sum to the region, identity, exact halving = the pyramid's level, nearest indices inside the covering window, nodata),
codec.view_level, the float32 fold against the float64 mean on the inputs test_gpu_view.py holds the kernel to, the
cache model, and the new entry points' declarations and refusals (which need the library, not a device)."""
import ctypes
import os
import re

import numpy as np
import pytest

import pyramid_ref as P
import view_ref as V
from dsic_amd import codec, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"dsic_window_resample_u8": 17, "dsic_window_resample_u16": 17, "dsic_window_resample_f32": 18}


def test_weights_sum_to_the_region_and_stay_inside_the_covering_window():
    for h in (1, 2, 3, 7, 64, 65, 100):
        for n in (1, 2, 3, 5, 64, 99, 130):
            for l in (0, 1, 2, 3):
                for o in (0, 1, 5, 8, 13):
                    rows = V.axis_weights(o, h, n, l)
                    first, _, count, _ = V.level_window(l, o, 0, h, 1)
                    assert len(rows) == n
                    for i, row in enumerate(rows):
                        assert sum(wgt for _, wgt in row) == h, (h, n, l, o, i)
                        assert all(first <= Y < first + count for Y, _ in row)
                        assert [Y for Y, _ in row] == list(range(row[0][0], row[-1][0] + 1))
                        assert row[0][0] == (o + i * h // n) >> l and row[-1][0] == (o + ((i + 1) * h - 1) // n) >> l
                    per_source = {}
                    for row in rows:
                        for Y, wgt in row:
                            per_source[Y] = per_source.get(Y, 0) + wgt
                    # a level pixel spends n per level-0 pixel of the region under it
                    for Y, total in per_source.items():
                        under = min((Y + 1) << l, o + h) - max(Y << l, o)
                        assert total == under * n
                    near = V.nearest_index(o, h, n, l)
                    assert all(first <= Y < first + count for Y in near) and near == sorted(near)
                    assert near == [(o + ((2 * i + 1) * h) // (2 * n)) >> l for i in range(n)]
    assert V.level_window(2, 5, 9, 7, 30) == codec.level_window(2, 5, 9, 7, 30)


@pytest.mark.parametrize("kind,C", V.KINDS)
def test_the_same_size_at_shift_0_returns_the_source(kind, C):
    img = V.kernel_image(kind, C, 9, 11)
    win = img[2:8, 3:10] if kind != "f32" else img[:, 2:8, 3:10]
    for mode in ("average", "nearest"):
        got = V.resample(img, 4, 6, 0, (6, 9, 6, 7), (6, 7), mode)
        assert got.dtype == img.dtype and got.shape == win.shape
        if kind == "f32" and mode == "average":      # float32(42) * v / float32(42): within the fold's bound for K = 1
            assert np.abs(got.astype(np.float64) - win.astype(np.float64)).max() <= 3 * 2.0 ** -24
        else:
            assert got.tobytes() == np.ascontiguousarray(win).tobytes()


@pytest.mark.parametrize("kind,C", V.KINDS)
def test_exact_halving_is_the_pyramids_level(kind, C):
    img = V.kernel_image(kind, C, 12, 18)
    got = V.resample(img, 0, 0, 0, (0, 0, 12, 18), (6, 9))
    if kind == "f32":
        want = P.halve_f32(img)
        K = V.footprint((0, 0, 12, 18), (6, 9), 0)
        assert K == 4 and np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= (K + 2) * 2.0 ** -24
    else:
        v = img.astype(np.int64)
        want = (v[0::2, 0::2] + v[0::2, 1::2] + v[1::2, 0::2] + v[1::2, 1::2] + 2) >> 2
        assert np.array_equal(got, want)
        if kind == "u8":
            assert np.array_equal(got, P.halve_u8(img))
    # and from level 1 at shift 1 the same region at half size is level 1 itself
    level1 = got
    again = V.resample(level1, 0, 0, 1, (0, 0, 12, 18), (6, 9))
    assert again.tobytes() == level1.tobytes()


def test_nodata_pixels_stay_out_of_the_averages():
    img = np.full((4, 4, 3), 100, dtype=np.uint8)
    img[:2, :2] = 9                                                          # a nodata block
    img[2, 2] = (9, 9, 8)                                                    # one channel differs: valid
    img[3, 3] = 9
    got = V.resample(img, 0, 0, 0, (0, 0, 4, 4), (2, 2), nodata=9)
    assert got[0, 0].tolist() == [9, 9, 9]                                   # nothing but nodata under it
    assert got[0, 1].tolist() == [100, 100, 100] and got[1, 0].tolist() == [100, 100, 100]
    assert got[1, 1].tolist() == [(2 * 209 + 3) // 6, (2 * 209 + 3) // 6, (2 * 208 + 3) // 6]
    plain = V.resample(img, 0, 0, 0, (0, 0, 4, 4), (2, 2))
    assert plain[0, 0].tolist() == [9, 9, 9] and plain[1, 1].tolist() == [(218 + 2) // 4 + 0] * 2 + [(217 + 2) // 4]
    near = V.resample(img, 0, 0, 0, (0, 0, 4, 4), (2, 2), "nearest", nodata=9)
    assert np.array_equal(near, img[1::2, 1::2])
    f = (img.transpose(2, 0, 1) / np.float32(255)).astype(np.float32)
    nd = np.float32(9) / np.float32(255)
    gf = V.resample(f, 0, 0, 0, (0, 0, 4, 4), (2, 2), nodata=nd)
    assert (gf[:, 0, 0] == nd).all() and np.allclose(gf[:, 0, 1], 100 / 255, atol=1e-6)
    assert abs(gf[2, 1, 1] - 208 / 3 / 255) < 1e-6


def test_view_level():
    for fn in (codec.view_level, V.view_level):
        assert fn(4, 1024, 1024, 513, 513) == 0 and fn(4, 1024, 1024, 512, 512) == 1       # either side of 2
        assert fn(4, 1024, 1024, 511, 511) == 1
        assert fn(4, 1024, 1024, 257, 257) == 1 and fn(4, 1024, 1024, 256, 256) == 2       # either side of 4
        assert fn(4, 1024, 1024, 255, 300) == 1 and fn(4, 1024, 1024, 255, 255) == 2       # both sides must fit
        assert fn(2, 1024, 1024, 16, 16) == 1 and fn(1, 1024, 1024, 16, 16) == 0           # fewer levels than asked
        assert fn(4, 100, 100, 101, 50) == 0 and fn(4, 100, 100, 400, 400) == 0            # magnifying
        assert fn(4, 768, 1024, 384, 512) == 1 and fn(4, 1, 1, 1, 1) == 0
    for h, w, oh, ow in [(330, 530, 80, 130), (330, 530, 83, 133), (7, 9, 3, 2), (64, 64, 64, 64)]:
        for n in (1, 2, 4):
            assert codec.view_level(n, h, w, oh, ow) == V.view_level(n, h, w, oh, ow)
    with pytest.raises(ValueError):
        codec.view_level(0, 8, 8, 4, 4)
    with pytest.raises(ValueError):
        codec.view_level(2, 8, 8, 0, 4)


@pytest.mark.parametrize("src_size,out_size", V.SIZES)
def test_the_float32_fold_lies_within_its_bound_of_the_float64_mean(src_size, out_size):
    """(K + 2) 2^-24 for inputs in [0, 1]: K float32 additions of terms that sum to at most T, the products' roundings
    together at most one more unit, and the division."""
    for shift in V.SHIFTS:
        c = V.kernel_case(src_size, out_size, shift)
        K = V.footprint(c["region"], c["size"], shift)
        for C in (1, 3, 4):
            img = V.kernel_image("f32", C, c["sh"], c["sw"])
            assert img.min() >= 0 and img.max() <= 1
            for nodata in (None, V.NODATA["f32"]):
                got = V.resample(img, c["sy0"], c["sx0"], shift, c["region"], c["size"], nodata=nodata)
                want = V.resample(img, c["sy0"], c["sx0"], shift, c["region"], c["size"], nodata=nodata, fold="f64")
                err = np.abs(got.astype(np.float64) - want).max()
                assert got.dtype == np.float32 and err <= (K + 2) * 2.0 ** -24, (shift, C, nodata, err, K)


def test_the_cache_model():
    lru = V.LRU(4)
    assert lru.call([(0, 0), (0, 1)]) == (0, 2) and lru.call([(0, 0), (0, 1)]) == (2, 0)
    assert lru.call([(0, 2), (0, 3)]) == (0, 2) and lru.order == [(0, 0), (0, 1), (0, 2), (0, 3)]
    assert lru.call([(0, 0), (1, 0)]) == (1, 1) and lru.order == [(0, 2), (0, 3), (0, 0), (1, 0)]    # (0, 1) left
    assert lru.call([(0, k) for k in range(5)]) == (0, 5) and len(lru.order) == 4                    # too large
    assert lru.call([(0, 3), (0, 4), (0, 5), (0, 6)]) == (1, 3) and lru.order == [(0, 3), (0, 4), (0, 5), (0, 6)]
    sized = V.LRU(10, cost=lambda key: 4 if key[0] == 0 else 1)
    assert sized.call([(0, 0), (0, 1)]) == (0, 2) and sized.call([(1, 0), (1, 1)]) == (0, 2)
    assert sized.call([(1, 2)]) == (0, 1) and sized.order == [(0, 1), (1, 0), (1, 1), (1, 2)]


def test_the_new_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "dsic_hip.h")).read()
    for name, nargs in NEW.items():
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert decl, name
        assert len(decl.group(1).split(",")) == nargs
        res, args = lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs and getattr(lib.load(), name) is not None
    assert lib.SIGNATURES["dsic_window_resample_f32"][1][15] is ctypes.c_float


def test_the_resample_calls_check_their_arguments_without_a_gpu():
    L = lib.load()
    E, err = lib.DSIC_EINVAL, L.dsic_last_error
    a, b = 1 << 20, 1 << 24                     # non-null, aligned, far apart: every call below is refused before a launch
    ok = dict(sh=8, sw=8, sy0=0, sx0=0, C=3, shift=0, y0=0, x0=0, h=8, w=8, oh=4, ow=4, mode=0, nodata=-1)

    def call(name, src=a, dst=b, **kw):
        p = dict(ok, **kw)
        tail = (p["nodata"],) if name != "f32" else (ctypes.c_float(0.5), 1)
        return getattr(L, "dsic_window_resample_" + name)(src, p["sh"], p["sw"], p["sy0"], p["sx0"], p["C"], p["shift"],
                                                          p["y0"], p["x0"], p["h"], p["w"], dst, p["oh"], p["ow"],
                                                          p["mode"], *tail, None)

    for name, bad_c, good_c in (("u8", (1, 2, 5), 3), ("u16", (0, 5), 1), ("f32", (0, 9), 8)):
        assert call(name, src=None, C=good_c) == E and b"null" in err()
        assert call(name, dst=None, C=good_c) == E and b"null" in err()
        for C in bad_c:
            assert call(name, C=C) == E and f"C={C}".encode() in err()
        assert call(name, C=good_c, shift=16) == E and b"shift=16" in err()
        assert call(name, C=good_c, shift=-1) == E and b"shift" in err()
        assert call(name, C=good_c, mode=2) == E and b"mode=2" in err()
        assert call(name, C=good_c, oh=0) == E and b"output" in err()
        assert call(name, C=good_c, h=0) == E and b"region" in err()
        assert call(name, C=good_c, y0=-1) == E and b"region" in err()
        # the covering window must lie inside the source window, on every side
        assert call(name, C=good_c, h=9) == E and b"outside the source window" in err()
        assert call(name, C=good_c, x0=1) == E and b"outside the source window" in err()
        assert call(name, C=good_c, sy0=1) == E and b"outside the source window" in err()
        assert call(name, C=good_c, shift=1, h=17, sh=8) == E and b"outside the source window" in err()
        assert call(name, C=good_c, sx0=2, x0=3, shift=1, w=8, sw=4) == E and b"outside the source window" in err()
        # 2^23 x 2^23 + one row: over 2^46 pixels
        assert call(name, C=good_c, sh=1 << 24, sw=1 << 24, h=(1 << 23) + 1, w=1 << 23) == E and b"2^46" in err()
        assert call(name, C=good_c, dst=a + 16) == E and b"overlap" in err()
    assert call("u8", nodata=256) == E and b"nodata=256" in err()
    assert call("u16", nodata=65536) == E and b"nodata=65536" in err()
    assert call("u8", nodata=-2) == E and b"nodata" in err()
    assert call("u16", src=a + 1) == E and b"2-byte aligned" in err()
    assert call("f32", dst=b + 2) == E and b"4-byte aligned" in err()


def test_the_reader_is_exported_beside_decompress_region():
    assert codec.ImageReader.__module__.endswith("view") and callable(codec.view_level)
    assert {"read", "read_many", "index", "close"} <= set(dir(codec.ImageReader))
