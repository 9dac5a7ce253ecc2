"""The warped reads without a GPU: the restatement of tests/warp_ref.py against its own properties (identity, rotation,
halving, weight sums, the int64 bound on the cubic sum), against float64 interpolation at the truncated phase, its
clamping, masks and fill; view.warp_window against every tap by brute force and view.warp_level at its thresholds;
codec.affine_q16; and the new entry points' declarations and refusals (which need the library, not a device)."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import warp_ref as R
from dsic_amd import codec, lib, view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"dsic_window_warp_u8": 21, "dsic_window_warp_u16": 21, "dsic_window_warp_render_u8": 24,
       "dsic_window_warp_render_u16": 24}
Q = 65536
KINDS = [("u8", 3), ("u16", 2)]


def _whole(img, l, H, W, m, size, mode, sval=None, nodata=None, fill=0):
    """the restatement with the whole level as its window"""
    LH, LW = img.shape[:2]
    return R.warp(img, sval, 0, 0, l, LH, LW, H, W, m, size, mode, nodata, fill)


# ---- properties and weights -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,C", KINDS)
def test_identity_rotation_and_halving(kind, C):
    img = R.level_image(kind, C, 12, 18)
    y0, x0, h, w = 3, 4, 6, 9
    win = img[y0:y0 + h, x0:x0 + w]
    for mode in R.MODES.values():
        got, ok = _whole(img, 0, 12, 18, (Q, 0, y0 * Q, 0, Q, x0 * Q), (h, w), mode)
        assert ok.all() and got.dtype == img.dtype and np.array_equal(got, win), mode
        got, ok = _whole(img, 0, 12, 18, (0, Q, y0 * Q, -Q, 0, (x0 + w) * Q), (w, h), mode)
        assert ok.all() and np.array_equal(got, np.rot90(win)), mode
        assert codec.affine_q16(codec.window_affine(y0, x0, h, w, h, w)) == (Q, 0, y0 * Q, 0, Q, x0 * Q)
        assert codec.affine_q16(codec.rotation_affine(y0 + h / 2, x0 + w / 2, 90, 1, w, h)) == \
            (0, Q, y0 * Q, -Q, 0, (x0 + w) * Q)
        # halving: level 1 of a 24 x 36 image is 12 x 18, and the view of every second pixel returns its own pixels
        got, ok = _whole(img, 1, 24, 36, (2 * Q, 0, 0, 0, 2 * Q, 0), (12, 18), mode)
        assert ok.all() and np.array_equal(got, img), mode
    assert view.warp_level(4, (2 * Q, 0, 0, 0, 2 * Q, 0)) == 1


def test_the_weights_sum_to_a_power_of_two_for_every_phase_pair():
    cubic = [R.cubic_weights(p) for p in range(128)]
    assert all(sum(w) == 1 << 22 for w in cubic) and cubic[0] == [0, 1 << 22, 0, 0]
    for py in range(128):
        for px in range(128):
            assert sum(a * b for a in (128 - py, py) for b in (128 - px, px)) == 1 << 14
            assert sum(a * b for a in cubic[py] for b in cubic[px]) == 1 << 44
    worst = max(sum(abs(a * b) for a in cubic[py] for b in cubic[px]) for py in range(128) for px in range(128))
    assert worst == 25 * (1 << 44) // 16 and worst * 65535 < 1 << 61       # 1.5625 2^44, at phase 64 on both axes


def test_the_cubic_sum_stays_inside_int64_on_the_worst_input():
    """an alternating 0 / 65535 pattern sampled at every phase of a magnified view, in Python's integers"""
    yy, xx = np.mgrid[:6, :6]
    img = (((yy + xx) % 2) * 65535).astype(np.uint16)[:, :, None]
    m = (Q // 128, 0, 2 * Q, 0, Q // 128, 2 * Q)                             # one phase step per output pixel
    big = 0
    for i in range(0, 256, 3):
        for j in range(0, 256, 5):
            vals, ok, s = R.pixel(img, None, 0, 0, 0, 6, 6, 6, 6, m, i, j, 2)
            big = max(big, s)
            assert ok and 0 <= vals[0] <= 65535
    assert 1 << 59 < big < 1 << 61 < 1 << 63
    got, _ = _whole(img, 0, 6, 6, m, (256, 256), 2)
    assert all(got[i, j, 0] == R.pixel(img, None, 0, 0, 0, 6, 6, 6, 6, m, i, j, 2)[0][0]
               for i in range(0, 256, 7) for j in range(0, 256, 11))


def test_the_vectorised_restatement_is_the_rule_pixel_by_pixel():
    """warp (int64, NumPy) against pixel (Python's integers) over a thinned kernel sweep, masks and nodata included"""
    for si, src_size in enumerate(R.SRC_SIZES):
        for k, name in enumerate(R.MATRICES):
            kind, C = R.KINDS[(si + k) % len(R.KINDS)]
            l, mode, out_size = R.SHIFTS[(si + k) % 3], (si + k) % 3, R.OUT_SIZES[(si + 2 * k) % 4]
            c = R.kernel_case(src_size, out_size, l, name, mode, margin=k % 2)
            img = R.level_image(kind, C, *src_size)
            val = R.validity(*src_size) if k % 3 == 0 else None
            nodata = R.NODATA[kind] if k % 3 == 1 else None
            got, ok = R.run_case(img, val, c, mode, nodata, R.FILL[kind])
            ys, xs = slice(c["sy0"], c["sy0"] + c["sh"]), slice(c["sx0"], c["sx0"] + c["sw"])
            for i in range(out_size[0]):
                for j in range(out_size[1]):
                    vals, valid, _ = R.pixel(img[ys, xs], None if val is None else val[ys, xs], c["sy0"], c["sx0"], l,
                                             c["LH"], c["LW"], c["H"], c["W"], c["m"], i, j, mode, nodata, R.FILL[kind])
                    assert got[i, j].tolist() == vals and bool(ok[i, j]) == valid, (src_size, name, mode, i, j)


# ---- the float64 anchor ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,C", KINDS)
def test_bilinear_and_cubic_lie_within_half_a_unit_of_float64(kind, C):
    """The integer sums are exact, so only the final rounding differs from the float64 interpolation at the same
    phase: 0.5, plus the rounding of the float64 evaluation itself, at most 16 products and 15 additions of terms
    whose absolute values sum to at most 1.5625^2 top: 40 * 2^-53 * 2.45 * top < 1e-9 for top = 65535."""
    top = 255 if kind == "u8" else 65535
    eps = 40 * 2.0 ** -53 * 2.45 * top
    assert eps < 1e-9
    img = R.level_image(kind, C, 9, 11)
    worst = 0.0
    for l, (H, W) in ((0, (9, 11)), (1, (17, 21))):
        for name in ("translate", "magnify5.25", "rot30", "shear", "mirror"):
            m = R.matrix(name, H, W, 13, 15)
            for mode in (0, 2):
                got, ok = _whole(img, l, H, W, m, (13, 15), mode)
                assert ok.any()
                for i, j in zip(*np.nonzero(ok)):
                    want = R.float_pixel(img, l, 9, 11, m, int(i), int(j), mode)
                    if mode == 2:
                        want = np.clip(want, 0, top)
                    err = np.abs(got[i, j].astype(np.float64) - want).max()
                    worst = max(worst, err)
                    assert err <= 0.5 + eps, (kind, l, name, mode, i, j, err)
    assert worst > 0.4                                                       # the bound is met, not idle


# ---- cubic clamping --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["u8", "u16"])
def test_a_magnified_step_edge_clamps_at_both_ends_under_cubic(kind):
    top = 255 if kind == "u8" else 65535
    img = np.array([0, 0, top, top], dtype=R.view_ref.DTYPES[kind])[None, :, None].repeat(3, axis=0)
    m = (Q, 0, Q, 0, Q // 16, 0)                                             # 16 output pixels per source column
    got, ok = _whole(img, 0, 3, 4, m, (1, 64), 2)
    raw = [sum(wy * wx * int(img[Y, X, 0]) for Y, wy in R.axis_taps(R.position(m[:3], 0, j), 0, 3, 2)
               for X, wx in R.axis_taps(R.position(m[3:], 0, j), 0, 4, 2)) for j in range(64)]
    before = [(S + (1 << 43)) >> 44 for S in raw]
    assert ok.all() and min(before) < 0 and max(before) > top                # both clamps fire
    assert got[0, :, 0].tolist() == [min(max(v, 0), top) for v in before]
    assert got.min() == 0 and got.max() == top
    bil, _ = _whole(img, 0, 3, 4, m, (1, 64), 0)
    assert (np.diff(bil[0, :, 0].astype(np.int64)) >= 0).all()               # bilinear never overshoots


# ---- masks and fill ----------------------------------------------------------------------------------------------------
def test_a_tap_out_of_the_mask_turns_a_cubic_pixel_into_the_bilinear_one():
    img = R.level_image("u16", 2, 9, 11)
    m = R.matrix("magnify3", 9, 11, 12, 14)
    val = np.ones((9, 11), dtype=np.uint8)
    val[3, 4] = 0
    cubic, ok = _whole(img, 0, 9, 11, m, (12, 14), 2, sval=val)
    plain, _ = _whole(img, 0, 9, 11, m, (12, 14), 2)
    bil, okb = _whole(img, 0, 9, 11, m, (12, 14), 0, sval=val)
    near = np.zeros((12, 14), dtype=bool)                                    # pixels with (3, 4) among their 16 taps
    for i in range(12):
        for j in range(14):
            ty = R.axis_taps(R.position(m[:3], i, j), 0, 9, 2)
            tx = R.axis_taps(R.position(m[3:], i, j), 0, 11, 2)
            near[i, j] = any(Y == 3 for Y, _ in ty) and any(X == 4 for X, _ in tx)
    assert near.any() and not near.all() and ok.all() and okb.all()
    assert np.array_equal(cubic[near], bil[near]) and np.array_equal(cubic[~near], plain[~near])
    assert not np.array_equal(cubic[near], plain[near])
    # the same by value: a nodata pixel (all channels equal) is out, one with a single channel equal is in
    img2 = img.copy()
    img2[5, 5] = (7, 8)
    val2 = (~(img2 == 7).all(axis=2)).astype(np.uint8)
    assert val2[5, 5] == 1 and not val2.all() and val2.any()
    byvalue, okv = _whole(img2, 0, 9, 11, m, (12, 14), 2, nodata=7, fill=7)
    masked, okm = _whole(img2, 0, 9, 11, m, (12, 14), 2, sval=val2, fill=7)
    assert np.array_equal(byvalue, masked) and np.array_equal(okv, okm) and not okv.all()


def test_a_pixel_with_no_counting_tap_is_fill_and_invalid():
    img = R.level_image("u8", 3, 8, 8)
    val = np.ones((8, 8), dtype=np.uint8)
    val[:4, :4] = 0
    for mode in (0, 2):
        got, ok = _whole(img, 0, 8, 8, (Q // 2, 0, 0, 0, Q // 2, 0), (16, 16), mode, sval=val, fill=99)
        assert not ok[:6, :6].any() and (got[:6, :6] == 99).all() and ok[10:, 10:].all()
    got, ok = _whole(img, 0, 8, 8, (Q // 2, 0, 0, 0, Q // 2, 0), (16, 16), 1, sval=val, fill=99)
    assert np.array_equal(ok, np.kron(val, np.ones((2, 2), dtype=np.uint8)) != 0)
    assert np.array_equal(got, np.kron(img, np.ones((2, 2, 1), dtype=np.uint8)))   # nearest copies pixel and validity


def test_outside_samples_are_fill_and_invalid_on_all_four_sides():
    img = R.level_image("u8", 3, 5, 7)
    m = R.matrix("overhang", 5, 7, 14, 18)                                   # one level-0 pixel per output pixel
    assert m == (Q, 0, -9 * Q // 2, 0, Q, -11 * Q // 2)
    for mode in R.MODES.values():
        got, ok = _whole(img, 0, 5, 7, m, (14, 18), mode, fill=77)
        inside = np.zeros((14, 18), dtype=bool)
        inside[4:9, 5:12] = True                                             # y = i - 4 in 0 .. 4, x = j - 5 in 0 .. 6
        assert np.array_equal(ok, inside), mode
        assert (got[~ok] == 77).all() and not ok[0].any() and not ok[-1].any() and not ok[:, 0].any() and not ok[:, -1].any()
    assert view.warp_window(0, 5, 7, 5, 7, m, 14, 18, 2) == (0, 0, 5, 7)


# ---- window and level -------------------------------------------------------------------------------------------------
def test_warp_window_contains_every_tap_of_every_output_pixel():
    for src_size in R.SRC_SIZES:
        for out_size in R.OUT_SIZES[:4]:
            for k, name in enumerate(R.MATRICES):
                l = R.SHIFTS[k % 3]
                for mode in R.MODES.values():
                    c = R.kernel_case(src_size, out_size, l, name, mode)
                    args = (l, c["LH"], c["LW"], c["H"], c["W"], c["m"], *out_size, mode)
                    win, brute = view.warp_window(*args), R.brute_window(*args)
                    assert win == R.warp_window(*args), (src_size, out_size, name, mode)
                    if brute is None:                                        # the box of the corners may still meet the image
                        continue
                    assert win is not None, (src_size, out_size, name, mode)
                    assert win[0] <= brute[0] and win[1] <= brute[1], (src_size, out_size, name, mode, win, brute)
                    assert win[0] + win[2] >= brute[0] + brute[2] and win[1] + win[3] >= brute[1] + brute[3]
                    assert win[0] >= 0 and win[1] >= 0 and win[0] + win[2] <= c["LH"] and win[1] + win[3] <= c["LW"]
                    corners = [(R.position(c["m"][:3], i, j), R.position(c["m"][3:], i, j))
                               for i in (0, out_size[0] - 1) for j in (0, out_size[1] - 1)]
                    if all(0 <= Py < c["H"] << 17 and 0 <= Px < c["W"] << 17 for Py, Px in corners):
                        assert win == brute, (src_size, out_size, name, mode, win, brute)    # corners inside: exact


def test_warp_window_is_none_for_a_view_beside_the_image():
    for m in ((Q, 0, 40 * Q, 0, Q, 0), (Q, 0, -20 * Q, 0, Q, 0), (Q, 0, 0, 0, Q, 70 * Q), (Q, 0, 0, 0, Q, -9 * Q)):
        for mode in R.MODES.values():
            assert view.warp_window(0, 40, 68, 40, 68, m, 8, 8, mode) is None
            assert R.brute_window(0, 40, 68, 40, 68, m, 8, 8, mode) is None
    assert view.warp_window(0, 40, 68, 40, 68, (Q, 0, -7 * Q, 0, Q, 0), 8, 8, 0) == (0, 0, 2, 9)   # one row overlaps
    # a turned view whose corners' bounding box meets the image though no pixel does: a window, not None
    m = codec.affine_q16(codec.rotation_affine(-6, -6, 45, 1, 12, 12))
    assert R.brute_window(0, 40, 68, 40, 68, m, 12, 12, 0) is None
    assert view.warp_window(0, 40, 68, 40, 68, m, 12, 12, 0) is not None


def test_warp_level_at_its_thresholds():
    for fn in (view.warp_level, R.warp_level):
        for l in (1, 2, 3):
            s = Q << l
            assert fn(5, (s, 0, 0, 0, s, 0)) == l and fn(5, (s - 1, 0, 0, 0, s - 1, 0)) == l - 1
            assert fn(5, (s + 1, 0, 0, 0, s + 1, 0)) == l and fn(l, (s, 0, 0, 0, s, 0)) == l - 1     # fewer levels
            assert fn(5, (0, s, 0, -s, 0, 0)) == l and fn(5, (0, s - 1, 0, -s, 0, 0)) == l - 1       # turned by 90
        assert fn(5, (Q, 0, 0, 0, Q, 0)) == 0 and fn(5, (Q // 3, 0, 0, 0, Q // 3, 0)) == 0            # magnifying
        assert fn(5, (8 * Q, 0, 0, 0, 2 * Q, 0)) == 1 and fn(5, (2 * Q, 0, 0, 0, 8 * Q, 0)) == 1      # the shorter step
        assert fn(5, (Q // 2, 0, Q, Q // 4, 0, Q)) == 0 and fn(1, (64 * Q, 0, 0, 0, 64 * Q, 0)) == 0  # a zero column
        assert fn(5, (1 << 26, 0, 0, 0, 1 << 26, 0)) == 4
    with pytest.raises(ValueError):
        view.warp_level(0, (Q, 0, 0, 0, Q, 0))


# ---- quantiser, refusals, ABI -----------------------------------------------------------------------------------------
def test_affine_q16_rounds_once_and_refuses_what_is_out_of_range():
    assert codec.affine_q16([[1, 0, 0], [0, 1, 0]]) == (Q, 0, 0, 0, Q, 0)
    assert codec.affine_q16([[0.1, -0.1, 1 / 3], [Fraction(1, 3), 2.5, -7.25]]) == (6554, -6554, 21845, 21845, 163840, -475136)
    assert codec.affine_q16(np.array([[1.5, 0, 2], [0, 1.5, 3]])) == (98304, 0, 131072, 0, 98304, 196608)
    assert codec.affine_q16([[0.7 / Q, 0.4 / Q, 0], [-0.7 / Q, -0.4 / Q, 0]]) == (1, 0, 0, -1, 0, 0)
    assert codec.affine_q16([[1024, -1024, 2 ** 31 - 1], [0, 0, -(2 ** 31) + 1]])[2] == (2 ** 31 - 1) * Q
    for bad in ([[1024.001, 0, 0], [0, 1, 0]], [[1, 0, 2 ** 31], [0, 1, 0]], [[1, 0, 0], [0, -1025, 0]],
                [[1, 0, 0], [0, 1, -(2 ** 31)]], [[float("nan"), 0, 0], [0, 1, 0]], [[float("inf"), 0, 0], [0, 1, 0]],
                [[1, 0], [0, 1]], [[1, 0, 0]], "ab", None, [[1, 0, "x"], [0, 1, 0]]):
        with pytest.raises(ValueError):
            codec.affine_q16(bad)
    for size in ((0, 4), (4, (1 << 20) + 1)):
        with pytest.raises(ValueError, match="size"):
            view.warp_window(0, 8, 8, 8, 8, (Q, 0, 0, 0, Q, 0), *size, 0)
    assert view.warp_window(0, 8, 8, 8, 8, (1, 0, 0, 0, 1, 0), 1 << 20, 1 << 20, 2) == (0, 0, 8, 8)
    assert view.warp_window(0, 8, 8, 8, 8, (1, 0, 0, 0, 1, 0), 1 << 16, 1 << 16, 2) == (0, 0, 3, 3)
    with pytest.raises(ValueError):
        view.warp_window(0, 8, 8, 8, 8, ((1 << 26) + 1, 0, 0, 0, Q, 0), 4, 4, 0)
    with pytest.raises(ValueError):
        codec.window_affine(0, 0, 8, 8, 0, 4)


def test_the_new_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "dsic_hip.h")).read()
    for name, nargs in NEW.items():
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert decl, name
        assert len(decl.group(1).split(",")) == nargs
        res, args = lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs and getattr(lib.load(), name) is not None
    assert {"read_warped", "render_warped"} <= set(dir(codec.ImageReader))
    assert all(callable(getattr(codec, n)) for n in ("affine_q16", "window_affine", "rotation_affine"))


def test_the_warp_calls_check_their_arguments_without_a_gpu():
    L = lib.load()
    E, err = lib.DSIC_EINVAL, L.dsic_last_error
    a, b, v = 1 << 20, 1 << 24, 1 << 26                   # non-null, aligned, far apart: every call is refused before a launch
    ok = dict(sval=None, sh=8, sw=8, sy0=0, sx0=0, C=3, shift=0, LH=8, LW=8, H=8, W=8, m=(Q, 0, 0, 0, Q, 0), oval=None,
              oh=8, ow=8, mode=0, nodata=-1, fill=0)
    bands, lohi = (ctypes.c_int * 3)(0, 1, 2), codec._lohi([(0, 255)] * 4)

    def call(name, src=a, dst=b, **kw):
        p = dict(ok, **kw)
        m = None if p["m"] is None else (ctypes.c_int64 * 6)(*p["m"])
        head = (src, p["sval"], p["sh"], p["sw"], p["sy0"], p["sx0"], p["C"], p["shift"], p["LH"], p["LW"], p["H"], p["W"], m)
        if name.startswith("render"):
            return getattr(L, "dsic_window_warp_" + name)(*head, bands, p.get("nb", 3), lohi, dst, p["oh"], p["ow"],
                                                          p["mode"], p["nodata"], p.get("alpha", 1), p.get("background", 0),
                                                          None)
        return getattr(L, "dsic_window_warp_" + name)(*head, dst, p["oval"], p["oh"], p["ow"], p["mode"], p["nodata"],
                                                      p["fill"], None)

    for name, bad_c in (("u8", (2, 5)), ("u16", (0, 5)), ("render_u8", (0, 5)), ("render_u16", (0, 5))):
        assert call(name, src=None) == E and b"null" in err()
        assert call(name, dst=None) == E and b"null" in err()
        assert call(name, m=None) == E and b"null" in err()
        for C in bad_c:
            assert call(name, C=C) == E and f"C={C}".encode() in err()
        assert call(name, mode=3) == E and b"mode=3" in err()
        assert call(name, mode=-1) == E and b"mode=-1" in err()
        assert call(name, shift=16) == E and b"shift=16" in err()
        assert call(name, LH=7) == E and b"level 0" in err()
        assert call(name, shift=1, H=17, W=15) == E and b"level 1" in err()   # level 1 of 17 x 15 is 9 x 8
        assert call(name, sy0=1) == E and b"source window" in err()
        assert call(name, oh=0) == E and b"output" in err()
        assert call(name, ow=(1 << 20) + 1) == E and b"output" in err()
        assert call(name, m=((1 << 26) + 1, 0, 0, 0, Q, 0)) == E and b"matrix entry 0" in err()
        assert call(name, m=(Q, 0, 0, 0, -(1 << 26) - 1, 0)) == E and b"matrix entry 4" in err()
        assert call(name, m=(Q, 0, 1 << 47, 0, Q, 0)) == E and b"matrix entry 2" in err()
        assert call(name, m=(Q, 0, 0, 0, Q, -(1 << 47))) == E and b"matrix entry 5" in err()
        # the window must hold every tap: the identity over 8 x 8 needs all of the level
        assert call(name, sh=7) == E and b"outside the source window" in err()
        assert call(name, sx0=1, sw=7) == E and b"outside the source window" in err()
        assert call(name, m=(Q, 0, Q // 2, 0, Q, 0), sh=7, mode=1) == E and b"outside the source window" in err()
        assert call(name, m=(2 * Q, 0, 0, 0, 2 * Q, 0), oh=4, ow=4, sh=7, mode=2) == E and b"rows 0..7" in err()
        assert call(name, dst=a + 16) == E and b"overlap" in err()
        assert call(name, sval=b + 8) == E and b"overlap" in err()
        assert call(name, nodata=65536) == E and b"nodata=65536" in err()
    assert call("u8", nodata=256) == E and b"nodata=256" in err()
    assert call("u8", fill=256) == E and b"fill=256" in err()
    assert call("u16", fill=-1) == E and b"fill" in err()
    assert call("u16", src=a + 1) == E and b"2-byte aligned" in err()
    assert call("u8", sval=v, oval=v + 8) == E and b"overlap" in err()
    assert call("u8", oval=b + 4) == E and b"overlap" in err()
    assert call("render_u8", nb=2) == E and b"nb=2" in err()
    assert call("render_u8", alpha=2) == E and b"alpha=2" in err()
    assert call("render_u16", background=256) == E and b"background" in err()
