"""Gridded reads without a GPU: the restatement of tests/grid_ref.py against warp_ref.py on affine meshes (the anchor:
an affine mesh gives the affine position exactly, for every step), against its own per-pixel rule and its bounds;
view.grid_window by brute force, view.grid_level at its thresholds, the mesh builders, the ABI and the argument checks
of the six calls."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import grid_ref as G
import grid_stream_cases as GSC
import stream_cases as SC
import warp_ref as R
from dsic_amd import codec, lib, view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = 65536
NEW = {"dsic_window_grid_u8": 23, "dsic_window_grid_u16": 23, "dsic_window_grid_render_u8": 26,
       "dsic_window_grid_render_u16": 26, "dsic_window_grid_index_render_u8": 29, "dsic_window_grid_index_render_u16": 29}


# ---- the anchor: affine meshes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", G.STEPS)
def test_an_affine_mesh_gives_the_affine_positions_exactly(S):
    for name in R.MATRICES:
        for n, size in enumerate(R.OUT_SIZES):
            H, W = (37, 71) if n % 2 else (330, 530)
            m = R.matrix(name, H, W, *size)
            mesh = G.affine(m, size, S)
            assert np.array_equal(mesh, view.affine_grid(m, size, S)) and mesh.shape == view.grid_shape(size, S)
            Py, Px, whole = G.positions(mesh, S, size)
            i, j = np.arange(size[0], dtype=np.int64)[:, None], np.arange(size[1], dtype=np.int64)[None, :]
            assert whole.all()
            assert np.array_equal(Py, m[0] * (2 * i + 1) + m[1] * (2 * j + 1) + 2 * m[2]), (name, size)
            assert np.array_equal(Px, m[3] * (2 * i + 1) + m[4] * (2 * j + 1) + 2 * m[5]), (name, size)
            for i, j in {(0, 0), (size[0] - 1, size[1] - 1), (size[0] // 2, size[1] // 3), (size[0] - 1, 0)}:
                assert G.position(mesh, S, i, j)[0] == (R.position(m[:3], i, j), R.position(m[3:], i, j))


@pytest.mark.parametrize("kind,C", [("u8", 3), ("u16", 2)])
def test_whole_views_of_affine_meshes_equal_the_warp_restatement(kind, C):
    LH, LW = 17, 33
    img, val = R.level_image(kind, C, LH, LW), R.validity(LH, LW)
    for k, name in enumerate(R.MATRICES):
        for n, size in enumerate(R.OUT_SIZES):
            l = (k + n) % 3
            H, W = R.image_size(LH, l), R.image_size(LW, l)
            m = R.matrix(name, H, W, *size)
            for mode in (0, 1, 2):
                t = (k + n + mode) % 3
                sval, nodata = (val, None) if t == 0 else (None, R.NODATA[kind] if t == 1 else None)
                want = R.warp(img, sval, 0, 0, l, LH, LW, H, W, m, size, mode, nodata, 7)
                for S in G.STEPS:
                    got = G.gridded(img, sval, 0, 0, l, LH, LW, H, W, G.affine(m, size, S), S, size, mode, nodata, 7)
                    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (name, size, S, mode)


# ---- the restatement against itself -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh_kind", ["jitter", "holes", "projective", "fold", "overhang", "bulge"])
def test_the_vectorised_restatement_equals_the_per_pixel_rule(mesh_kind):
    LH, LW, l, size = 17, 33, 1, (40, 70)                          # 3 x 5 cells, the last of each axis partial
    H, W = R.image_size(LH, l), R.image_size(LW, l)
    img, val = R.level_image("u16", 2, LH, LW), R.validity(LH, LW)
    mesh = G.mesh(mesh_kind, H, W, size, 16)
    Py, Px, whole = G.positions(mesh, 16, size)
    for i in range(size[0]):
        for j in range(size[1]):
            P, _ = G.position(mesh, 16, i, j)
            assert (P is not None) == bool(whole[i, j]) and (P is None or P == (Py[i, j], Px[i, j]))
    seen = 0
    for mode, sval, nodata in ((0, val, None), (1, None, None), (2, None, R.NODATA["u16"])):
        got, ok = G.gridded(img, sval, 0, 0, l, LH, LW, H, W, mesh, 16, size, mode, nodata, 9)
        for i in range(size[0]):
            for j in range(size[1]):
                px, v = G.pixel(img, sval, 0, 0, l, LH, LW, H, W, mesh, 16, i, j, mode, nodata, 9)
                assert (list(got[i, j]), bool(ok[i, j])) == (px, v), (mesh_kind, mode, i, j)
        seen += int(ok.sum())
    assert seen > 0 and (mesh_kind != "holes" or not whole.all())


def test_the_rearranged_form_in_wrapped_64_bit_is_the_four_weight_form_and_the_sum_stays_under_2_62():
    rng = np.random.default_rng(5)
    top = (1 << 48) - 1
    for S in G.STEPS:
        size = (2 * S, 2 * S)
        meshes = [np.full(G.shape(size, S), top, dtype=np.int64), np.full(G.shape(size, S), -top, dtype=np.int64),
                  rng.choice(np.array([top, -top], dtype=np.int64), G.shape(size, S)),
                  rng.integers(-top, top + 1, G.shape(size, S), dtype=np.int64)]
        big = 0
        for mesh in meshes:
            for i, j in [(0, 0), (S - 1, S - 1), (S, S - 1), (2 * S - 1, 0), (S // 2, S + 3)] + [tuple(p) for p in rng.integers(0, 2 * S, (40, 2))]:
                P, most = G.position(mesh, S, int(i), int(j))
                big = max(big, most)
                assert P == (G.rearranged_u64(mesh, S, int(i), int(j), 0), G.rearranged_u64(mesh, S, int(i), int(j), 1))
        assert big == top << (2 * (S.bit_length() - 1) + 2) and big < 1 << 62
    assert top << 14 < 1 << 62


# ---- the window -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh_kind", ["jitter", "projective", "fold", "overhang", "holes"])
def test_grid_window_holds_every_tap_of_every_inside_pixel(mesh_kind):
    some = 0
    for (LH, LW), size, l, S in (((17, 33), (17, 33), 0, 16), ((40, 68), (70, 130), 1, 32), ((5, 7), (16, 16), 2, 16),
                                 ((40, 68), (7, 9), 0, 64)):
        H, W = R.image_size(LH, l), R.image_size(LW, l)
        mesh = G.mesh(mesh_kind, H, W, size, S)
        for mode in (0, 1, 2):
            win = view.grid_window(l, LH, LW, H, W, mesh, mode)
            assert win == G.window(l, LH, LW, H, W, mesh, mode)
            brute = G.brute_window(l, LH, LW, H, W, mesh, S, size, mode)
            if brute is None:
                continue
            some += 1
            assert win is not None, (mesh_kind, size, mode)
            assert win[0] <= brute[0] and win[1] <= brute[1] and win[0] + win[2] >= brute[0] + brute[2] and \
                win[1] + win[3] >= brute[1] + brute[3], (mesh_kind, size, mode, win, brute)
            assert 0 <= win[0] and win[0] + win[2] <= LH and 0 <= win[1] and win[1] + win[3] <= LW
    assert some >= 6


def test_grid_window_contains_warp_window_and_is_none_beside_the_image_or_without_a_whole_cell():
    for name in R.MATRICES:
        for size in R.OUT_SIZES:
            m = R.matrix(name, 37, 71, *size)
            for S in G.STEPS:
                for mode in (0, 1, 2):
                    w, g = view.warp_window(0, 37, 71, 37, 71, m, *size, mode), view.grid_window(0, 37, 71, 37, 71, G.affine(m, size, S), mode)
                    if w is not None:
                        assert g[0] <= w[0] and g[1] <= w[1] and g[0] + g[2] >= w[0] + w[2] and g[1] + g[3] >= w[1] + w[3]
    beside = G.affine((Q, 0, 400 * Q, 0, Q, 0), (20, 30), 16)
    assert view.grid_window(0, 37, 71, 37, 71, beside, 0) is None
    holed = G.affine((Q, 0, 0, 0, Q, 0), (40, 40), 16)              # 3 x 3 cells around the one inner node
    holed[1, 1, 0] = holed[2, 2, 0] = G.NONE
    assert not G.whole_cells(holed)[:2, :2].any() and G.whole_cells(holed).any()
    holed[1, 2, 0] = holed[2, 1, 0] = G.NONE
    assert not G.whole_cells(holed).any() and view.grid_window(0, 37, 71, 37, 71, holed, 2) is None
    with pytest.raises(ValueError):
        view.grid_window(0, 37, 71, 37, 71, beside, 3)


# ---- the level --------------------------------------------------------------------------------------------------------
def test_grid_level_at_its_thresholds_and_on_affine_meshes():
    for S in G.STEPS:
        for name in R.MATRICES:
            for H, W, size in ((330, 530, (70, 130)), (3300, 5300, (17, 33)), (37, 71, (70, 130))):
                m = R.matrix(name, H, W, *size)
                for n in (1, 3, 5):
                    assert view.grid_level(n, G.affine(m, size, S), S) == R.warp_level(n, m) == view.warp_level(n, m), (name, S)
        for l in (1, 2, 3):
            s = Q << l
            at = lambda v: view.affine_grid((v, 0, 0, 0, v, 0), (40, 40), S)
            assert view.grid_level(5, at(s), S) == l and view.grid_level(5, at(s - 1), S) == l - 1
            assert view.grid_level(l, at(s), S) == l - 1                                        # fewer levels
            one_short = at(s)
            one_short[1, 1, 0] -= 1                                                              # one edge a hair shorter
            assert view.grid_level(5, one_short, S) == l - 1
            one_short[1, 1, 0] = G.NONE                                                          # its node gone: not looked at
            assert view.grid_level(5, one_short, S) == l
        for kind in ("jitter", "fold", "holes", "bulge"):
            mesh = G.mesh(kind, 3300, 5300, (70, 130), S)
            assert view.grid_level(5, mesh, S) == G.level(5, mesh, S), (kind, S)
    far = np.zeros((2, 2, 2), dtype=np.int64)                      # edges whose squares pass 2^63: Python integers
    far[1, :, 0], far[:, 1, 1] = (1 << 48) - 1, -((1 << 48) - 1)
    assert view.grid_level(12, far, 16) == G.level(12, far, 16) == 11
    none = np.full((2, 2, 2), G.NONE, dtype=np.int64)
    assert view.grid_level(5, none, 16) == 0
    with pytest.raises(ValueError):
        view.grid_level(0, far, 16)
    with pytest.raises(ValueError):
        view.grid_level(3, far, 24)


# ---- the builders -----------------------------------------------------------------------------------------------------
def test_function_grid_rounds_once_and_marks_what_is_not_finite():
    size, S = (40, 70), 32
    seen = []

    def fn(i, j):
        seen.append((i.copy(), j.copy()))
        y = 0.1 * i + j / 3 + 0.37
        y[1, 2] = np.nan
        x = np.where((i == 64) & (j == 0), np.inf, 2.5 * j - i / 7)
        return y, x
    got = view.function_grid(fn, size, S)
    i, j = seen[0]
    assert got.dtype == np.int64 and got.shape == (3, 4, 2) == view.grid_shape(size, S) and i.dtype == np.float64
    assert np.array_equal(i, np.broadcast_to(np.array([[0.], [32.], [64.]]), (3, 4))) and np.array_equal(j[0], [0, 32, 64, 96])
    for a in range(3):
        for b in range(4):
            if (a, b) in ((1, 2), (2, 0)):
                assert got[a, b, 0] == G.NONE
            else:
                want = (np.rint((0.1 * (a * S) + (b * S) / 3 + 0.37) * Q), np.rint((2.5 * (b * S) - (a * S) / 7) * Q))
                assert tuple(got[a, b]) == tuple(int(v) for v in want)
    assert view.function_grid(lambda i, j: (i * 0 + 0.5 / Q, j * 0 + 1.5 / Q), (16, 16), 16)[0, 0].tolist() == [0, 2]   # half to even
    with pytest.raises(ValueError):
        view.function_grid(lambda i, j: (i * 2.0 ** 33, j), size, S)
    with pytest.raises(ValueError, match="2\\^32"):              # finite, but not after the scaling: an error, not a hole
        view.function_grid(lambda i, j: (i + 1e305, j), size, S)
    with pytest.raises(ValueError):
        view.function_grid(lambda i, j: (i[:2], j[:2]), size, S)
    assert np.array_equal(view.check_grid(got, size, S), got) and codec.function_grid is view.function_grid


def test_projective_grid_against_fractions_at_the_nodes():
    for H, W, size, S in ((330, 530, (70, 130), 16), (37, 71, (17, 33), 32), (1000, 3, (70, 130), 64)):
        h = G.projective_h(H, W, *size)
        assert np.array_equal(view.projective_grid(h, size, S), G.projective(h, size, S))
    h = [[1, 0, 0], [0, 1, 0], [0, -1 / 32, 1]]                   # the denominator reaches 0 at column 32 and goes on down
    got = view.projective_grid(h, (16, 70), 16)
    assert np.array_equal(got, G.projective(h, (16, 70), 16))
    assert (got[:, :2, 0] != G.NONE).all() and (got[:, 2:, 0] == G.NONE).all()
    assert got[1, 1].tolist() == [int(Fraction(16) / Fraction(1, 2) * Q)] * 2
    third = view.projective_grid([[1, 0, 0], [0, 1, 0], [0, 0, 3]], (16, 16), 16)
    assert third[1, 1].tolist() == [349525, 349525]               # 16 / 3 in Q16 = 349525.33: rounded once
    eye = view.projective_grid([[1.5, 0, 2], [0, 0.25, -3], [0, 0, 1]], (40, 40), 16)
    assert np.array_equal(eye, view.affine_grid(codec.affine_q16([[1.5, 0, 2], [0, 0.25, -3]]), (40, 40), 16))
    for bad in ([[1, 0, 0], [0, 1, 0]], [[1, 0, 0], [0, 1, 0], [0, 0, float("nan")]], "abc", None):
        with pytest.raises(ValueError):
            view.projective_grid(bad, (16, 16), 16)


def test_grid_error_is_zero_on_an_affine_function_and_tells_the_steps_apart():
    fn = lambda i, j: (0.75 * i - 0.25 * j + 3.0, 0.5 * i + 1.25 * j - 7.5)      # exact in Q16
    for S in G.STEPS:
        assert view.grid_error(fn, view.function_grid(fn, (70, 130), S), (70, 130), S) == 0.0
    bulge = G.mesh_function("bulge", 3300, 5300, 700, 1300)
    errs = [view.grid_error(bulge, view.function_grid(bulge, (700, 1300), S), (700, 1300), S) for S in G.STEPS]
    assert 0 < errs[0] < errs[1] < errs[2] and 3.5 < errs[1] / errs[0] < 4.5   # a quadratic: the error goes with S^2
    holed = view.function_grid(fn, (16, 16), 16)
    holed[0, 0, 0] = G.NONE
    assert view.grid_error(fn, holed, (16, 16), 16) == 0.0


def test_check_grid_refuses_what_the_library_refuses():
    ok = view.affine_grid((Q, 0, 0, 0, Q, 0), (40, 70), 16)
    assert view.GRID_NONE == G.NONE == -(1 << 63) and view.GRID_STEPS == G.STEPS and ok.shape == (4, 6, 2)
    assert np.array_equal(view.check_grid(ok.astype(np.int32), (40, 70), 16), ok)
    for change, word in ((lambda g: g[:3], "shape"), (lambda g: g.astype(np.float64), "integer"),
                         (lambda g: _set(g, (1, 1, 1), G.NONE), "x entry"), (lambda g: _set(g, (0, 2, 0), 1 << 48), "2\\^48"),
                         (lambda g: _set(g, (3, 5, 1), -(1 << 48)), "2\\^48")):
        with pytest.raises(ValueError, match=word):
            view.check_grid(change(ok.copy()), (40, 70), 16)
    assert view.check_grid(_set(_set(ok.copy(), (1, 1, 0), G.NONE), (1, 1, 1), 1 << 60), (40, 70), 16)[1, 1, 0] == G.NONE
    assert view.check_grid(_set(ok.copy(), (0, 2, 0), (1 << 48) - 1), (40, 70), 16) is not None
    for size, step in (((40, 70), 24), ((40, 70), 8), ((0, 4), 16), ((1 << 20, 1 << 20), 16)):
        with pytest.raises(ValueError):
            view.grid_shape(size, step)
    assert view.grid_shape((1 << 20, 1 << 10), 64) == (16385, 17, 2)


def _set(g, at, v):
    g[at] = v
    return g


# ---- the ABI, the sweep, the recipes ----------------------------------------------------------------------------------
def test_the_six_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "dsic_hip.h")).read()
    for name, nargs in NEW.items():
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert decl, name
        assert len(decl.group(1).split(",")) == nargs and "mesh_host" in decl.group(1) and "mesh_dev" in decl.group(1)
        res, args = lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs and getattr(lib.load(), name) is not None
        warp = lib.SIGNATURES[name.replace("_grid_", "_warp_")][1]
        assert len(args) == len(warp) + 2 and args[:12] == warp[:12] and args[15:] == warp[13:]
    declared = set(re.findall(r"\b(dsic_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == set(lib.SIGNATURES)
    assert {"read_gridded", "render_gridded", "render_index_gridded"} <= set(dir(codec.ImageReader))
    for n in ("affine_grid", "function_grid", "projective_grid", "grid_error", "grid_level", "grid_window", "grid_shape",
              "check_grid"):
        assert getattr(codec, n) is getattr(view, n)
    assert codec.GRID_NONE == view.GRID_NONE and codec.GRID_STEPS == (16, 32, 64)


def test_the_sweep_takes_every_value_of_every_axis():
    for ki in range(len(R.KINDS)):
        seen = set()
        for si in range(len(R.SRC_SIZES)):
            for k, name in enumerate(G.MESHES):
                l, out_size, mask, margin, S, matrix = G.sweep(si, ki, k)
                seen |= {("shift", l), ("out", out_size), ("mask", mask), ("margin", margin), ("step", S),
                         (R.SRC_SIZES[si], l), (R.SRC_SIZES[si], S)}
        assert {("shift", l) for l in R.SHIFTS} | {("out", s) for s in R.OUT_SIZES} | {("mask", m) for m in G.MASKS} <= seen
        assert {("step", S) for S in G.STEPS} | {("margin", 0), ("margin", 1)} <= seen
        assert {(s, l) for s in R.SRC_SIZES for l in R.SHIFTS} | {(s, S) for s in R.SRC_SIZES for S in G.STEPS} <= seen
    every = [(name,) + G.sweep(si, ki, k) for ki in range(len(R.KINDS)) for si in range(len(R.SRC_SIZES))
             for k, name in enumerate(G.MESHES)]
    assert {(e[0], e[3]) for e in every} == {(name, m) for name in G.MESHES for m in G.MASKS}
    assert {(e[0], e[5]) for e in every} == {(name, S) for name in G.MESHES for S in G.STEPS}
    assert {(e[0], e[1]) for e in every} == {(name, l) for name in G.MESHES for l in R.SHIFTS}
    assert {(e[2], e[5]) for e in every} == {(o, S) for o in R.OUT_SIZES for S in G.STEPS}
    assert {e[6] for e in every if e[0] == "affine"} == set(R.MATRICES)


def test_the_grid_recipes_are_in_the_table():
    assert len(GSC.NAMES) == 12 and set(GSC.NAMES) <= set(SC.names())
    L = lib.load()
    assert {e for n in GSC.NAMES for e in SC.build(n, L).exports} == set(NEW)
    assert all(SC.family(n) == "views" for n in GSC.NAMES)


def test_the_tool_refuses_what_does_not_go_with_a_mesh_before_it_loads_anything(tmp_path, capsys):
    import importlib.util
    spec = importlib.util.spec_from_file_location("dsic_image_tool", os.path.join(ROOT, "tools", "dsic_image.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    np.save(tmp_path / "mesh.npy", view.affine_grid((Q, 0, 0, 0, Q, 0), (64, 100), 16))
    base = ["decompress", str(tmp_path / "none.dsic"), str(tmp_path / "out.npy"), "--weights", "none.pt", "--size", "64,100"]
    mesh = ["--grid", str(tmp_path / "mesh.npy")]
    for extra, word in ((mesh + ["--rotate", "30"], "do not go with"), (mesh + ["--region", "0,0,8,8"], "do not go with"),
                        (mesh + ["--affine", "1,0,0,0,1,0"], "do not go with"), (mesh + ["--grid-step", "24"], "step"),
                        (mesh + ["--grid-step", "32"], "shape"), (mesh + ["--projective", "1,0,0,0,1,0,0,0,1"], "exclude"),
                        (["--projective", "1,0,0,0,1,0"], "nine numbers"), (["--rotate", "30", "--grid-step", "32"], "--grid-step goes with"),
                        (mesh + ["--resampling", "average"], "average"), (["--grid", str(tmp_path / "no.npy")], "no.npy")):
        with pytest.raises(SystemExit) as e:
            tool.main(base + extra)
        assert e.value.code == 2 and word in capsys.readouterr().err, (extra, word)
    with pytest.raises(SystemExit):
        tool.main(["compress", "a.png", "b.dsic", "--weights", "none.pt"] + mesh)


# ---- the argument checks, without a GPU -------------------------------------------------------------------------------
def test_the_grid_calls_check_their_arguments_without_a_gpu():
    L = lib.load()
    E, err = lib.DSIC_EINVAL, L.dsic_last_error
    a, b, v, d = 1 << 20, 1 << 24, 1 << 26, 1 << 28     # non-null, aligned, far apart: every call is refused before a launch
    eye = view.affine_grid((Q, 0, 0, 0, Q, 0), (8, 8), 16)
    ok = dict(sval=None, sh=8, sw=8, sy0=0, sx0=0, C=3, shift=0, LH=8, LW=8, H=8, W=8, mesh=eye, step=16, oval=None, oh=8, ow=8,
              mode=0, nodata=-1, fill=0)
    bands, lohi = (ctypes.c_int * 3)(0, 1, 2), codec._lohi([(0, 255)] * 4)

    def call(name, src=a, dst=b, mdev=d, **kw):
        p = dict(ok, **kw)
        mesh = None if p["mesh"] is None else np.ascontiguousarray(p["mesh"], dtype=np.int64)
        head = (src, p["sval"], p["sh"], p["sw"], p["sy0"], p["sx0"], p["C"], p["shift"], p["LH"], p["LW"], p["H"], p["W"],
                None if mesh is None else mesh.ctypes.data, mdev, p["step"])
        fn = getattr(L, "dsic_window_grid_" + name)
        if name.startswith("render"):
            return fn(*head, bands, p.get("nb", 3), lohi, dst, p["oh"], p["ow"], p["mode"], p["nodata"], p.get("alpha", 1),
                      p.get("background", 0), None)
        if name.startswith("index"):
            return fn(*head, p.get("kind", 2), 0, 1, p.get("lo", -100), 100, v, dst, p["oh"], p["ow"], p["mode"], p["nodata"],
                      p.get("alpha", 1), p.get("background", 0), None)
        return fn(*head, dst, p["oval"], p["oh"], p["ow"], p["mode"], p["nodata"], p["fill"], None)

    def mesh_with(at, value, size=(8, 8), step=16):
        g = view.affine_grid((Q, 0, 0, 0, Q, 0), size, step)
        g[at] = value
        return g

    for name, bad_c in (("u8", (2, 5)), ("u16", (0, 5)), ("render_u8", (0, 5)), ("render_u16", (0, 5)),
                        ("index_render_u8", (0, 5)), ("index_render_u16", (0, 5))):
        assert call(name, src=None) == E and b"null" in err()
        assert call(name, dst=None) == E and b"null" in err()
        assert call(name, mesh=None) == E and b"null" in err()
        assert call(name, mdev=None) == E and b"null" in err()
        for C in bad_c:
            assert call(name, C=C) == E and f"C={C}".encode() in err()
        assert call(name, mode=3) == E and b"mode=3" in err()
        assert call(name, shift=16) == E and b"shift=16" in err()
        assert call(name, LH=7) == E and b"level 0" in err()
        assert call(name, sy0=1) == E and b"source window" in err()
        assert call(name, oh=0) == E and b"output" in err()
        assert call(name, ow=(1 << 20) + 1) == E and b"output" in err()
        for step in (0, 8, 24, 128):
            assert call(name, step=step) == E and f"step={step}".encode() in err()
        assert call(name, oh=1 << 20, ow=1 << 20) == E and b"2^22" in err()
        assert call(name, mesh=mesh_with((1, 0, 0), 1 << 48)) == E and b"node (1, 0)" in err() and b"2^48" in err()
        assert call(name, mesh=mesh_with((0, 1, 1), -(1 << 48))) == E and b"node (0, 1)" in err()
        assert call(name, mesh=mesh_with((1, 1, 1), G.NONE)) == E and b"x entry" in err()
        # the window must hold every tap the mesh can ask for: the identity over 8 x 8, whose cell reaches (16, 16)
        assert call(name, sh=7) == E and b"outside the source window" in err() and b"rows 0..7" in err()
        assert call(name, sx0=1, sw=7) == E and b"outside the source window" in err()
        assert call(name, mdev=b + 16) == E and b"device mesh and dst overlap" in err()
        assert call(name, dst=a + 16) == E and b"overlap" in err()
        assert call(name, mdev=d + 4) == E and b"8-byte aligned" in err()
        assert call(name, nodata=65536) == E and b"nodata=65536" in err()
    # a none node frees its cells from the window test: with the only cell holed nothing is asked of the window
    assert call("u8", mesh=mesh_with((1, 1, 0), G.NONE), sh=1, sw=1, nodata=256) == E and b"nodata=256" in err()
    small = view.affine_grid((Q, 0, 0, 0, Q, 0), (8, 8), 16)
    small[1, :, 0], small[:, 1, 1] = 4 * Q, 4 * Q                  # the cell spans 0 .. 4: rows and columns 0..4 of the level
    assert call("u8", mesh=small, sh=4, nodata=256) == E and b"rows 0..4" in err()
    assert call("u8", mesh=small, sh=5, sw=5, nodata=256) == E and b"nodata=256" in err()
    assert call("u8", fill=256) == E and b"fill=256" in err()
    assert call("u16", src=a + 1) == E and b"2-byte aligned" in err()
    assert call("u8", oval=b + 4) == E and b"overlap" in err()
    assert call("render_u8", nb=2) == E and b"nb=2" in err()
    assert call("render_u16", background=256) == E and b"background" in err()
    assert call("index_render_u8", kind=3) == E and b"kind=3" in err()
    assert call("index_render_u16", lo=-70000) == E and b"stretch pair" in err()
