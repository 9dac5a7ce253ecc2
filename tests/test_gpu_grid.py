"""Gridded reads on the GPU.  The three kinds of kernel alone, bit for bit against the restatement of tests/grid_ref.py,
outputs between guards and inputs inside a larger allocation as in test_gpu_warp.py; then
codec.ImageReader.read_gridded / render_gridded / render_index_gridded on the streams of test_gpu_warp.py: a gridded
read is the restatement applied to decompress_region's output of the planned window, a gridded read of an affine mesh is
read_warped of its matrix bit for bit; and the command-line tool."""
import ctypes
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import grid_ref as G
import grid_stream_cases  # noqa: F401  (its recipes join the table that test_gpu_stream_order.py runs)
import index_ref as X
import render_ref as D
import warp_ref as R
from dsic_amd import codec, lib
from dsic_amd.ops import _p, _stream
from test_gpu_pyramid import _CACHE as _PCACHE
from test_gpu_pyramid import BATCH, H0, W0, Out, _inside, _model, _same
from test_gpu_view import _stream_of
from test_gpu_warp import STREAMS, _cut, _open, _views

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = 65536
_MESHES = {}


# ---- the kernels ----------------------------------------------------------------------------------------------------
def _mesh(c):
    """(host mesh, device mesh) of a case; the device copy is made once per mesh"""
    key = c["G"].tobytes() + bytes(c["G"].shape)
    if key not in _MESHES:
        host = np.ascontiguousarray(c["G"], dtype=np.int64)
        _MESHES[key] = (host, torch.from_numpy(host).cuda())
    return _MESHES[key]


def _head(src, sval, c, C):
    host, dev = _mesh(c)
    return (_p(src), None if sval is None else _p(sval), c["sh"], c["sw"], c["sy0"], c["sx0"], C, c["shift"], c["LH"],
            c["LW"], c["H"], c["W"], host.ctypes.data, _p(dev), c["step"])


def _grid(kind, src, sval, c, C, dst, oval, mode, nodata, fill):
    return getattr(lib.load(), "dsic_window_grid_" + kind)(
        *_head(src, sval, c, C), _p(dst), None if oval is None else _p(oval), *c["size"], mode,
        -1 if nodata is None else nodata, fill, _stream())


def _grid_render(kind, src, sval, c, C, bands, pairs, dst, mode, nodata, alpha, background):
    return getattr(lib.load(), "dsic_window_grid_render_" + kind)(
        *_head(src, sval, c, C), (ctypes.c_int * len(bands))(*bands), len(bands), codec._lohi(pairs), _p(dst), *c["size"],
        mode, -1 if nodata is None else nodata, alpha, background, _stream())


def _grid_index(kind, src, sval, c, C, index, pair, cmap, dst, mode, nodata, alpha, background):
    name, a, b = X.parse(index)
    return getattr(lib.load(), "dsic_window_grid_index_render_" + kind)(
        *_head(src, sval, c, C), X.KINDS[name], a, b, pair[0], pair[1], _p(cmap), _p(dst), *c["size"], mode,
        -1 if nodata is None else nodata, alpha, background, _stream())


def test_the_sweep_takes_every_value_of_every_axis():
    every = [(name,) + G.sweep(si, ki, k) for ki in range(len(R.KINDS)) for si in range(len(R.SRC_SIZES))
             for k, name in enumerate(G.MESHES)]
    for ki in range(len(R.KINDS)):
        mine = [G.sweep(si, ki, k) for si in range(len(R.SRC_SIZES)) for k in range(len(G.MESHES))]
        assert {e[0] for e in mine} == set(R.SHIFTS) and {e[1] for e in mine} == set(R.OUT_SIZES)
        assert {e[2] for e in mine} == set(G.MASKS) and {e[3] for e in mine} == {0, 1} and {e[4] for e in mine} == set(G.STEPS)
    assert {(e[0], e[3]) for e in every} == {(name, m) for name in G.MESHES for m in G.MASKS}
    assert {(e[0], e[5]) for e in every} == {(name, S) for name in G.MESHES for S in G.STEPS}
    assert {(e[0], e[2]) for e in every} == {(name, o) for name in G.MESHES for o in R.OUT_SIZES}
    assert {e[6] for e in every if e[0] == "affine"} == set(R.MATRICES)


@pytest.mark.parametrize("si", range(len(R.SRC_SIZES)))
@pytest.mark.parametrize("ki", range(len(R.KINDS)))
def test_grid_kernels_equal_the_restatement(si, ki):
    src_size, (kind, C) = R.SRC_SIZES[si], R.KINDS[ki]
    img, fill = R.level_image(kind, C, *src_size), R.FILL[kind]
    inside_some = 0
    for k, name in enumerate(G.MESHES):
        l, out_size, mask, margin, S, matrix = G.sweep(si, ki, k)
        val = R.validity(*src_size, seed=k) if mask == "valid" else None
        nodata = R.NODATA[kind] if mask == "nodata" else None
        for mode in (0, 1, 2):
            c = G.kernel_case(src_size, out_size, l, name, S, mode, margin, matrix)
            want, ok = G.run_case(img, val, c, mode, nodata, fill)
            src = _inside(_cut(img, c), (k + mode) % 4)                      # the input at several element offsets
            sval = None if val is None else _inside(_cut(val, c), (k + 2 * mode) % 4)
            out, oval = Out(want.size, img.dtype, (0, 1, 3, 2)[(k + mode) % 4]), Out(ok.size, np.uint8, (k + mode) % 3)
            what = (f"window_grid_{kind} {src_size}->{out_size} C={C} shift={l} {name} {matrix if name == 'affine' else ''} "
                    f"step={S} mode={mode} {mask} margin={margin}")
            lib.check(_grid(kind, src, sval, c, C, out.view, oval.view, mode, nodata, fill), what)
            _same(out.host(what), want, what)
            _same(oval.host(what), ok.astype(np.uint8), what + " validity")
            inside_some += int(ok.any())
            if name == "affine":                                             # the anchor, on the device: the warp call's bits
                m = R.matrix(matrix, c["H"], c["W"], *out_size)
                w_img, w_ok = R.warp(_cut(img, c), None if val is None else _cut(val, c), c["sy0"], c["sx0"], l, c["LH"],
                                     c["LW"], c["H"], c["W"], m, out_size, mode, nodata, fill)
                assert np.array_equal(w_img, want) and np.array_equal(w_ok, ok), what
            if mode == 2 and k % 3 == 0:                                     # and without an output validity
                alone = Out(want.size, img.dtype, 1)
                lib.check(_grid(kind, src, sval, c, C, alone.view, None, mode, nodata, fill), what)
                _same(alone.host(what), want, what + " image alone")
    assert inside_some >= len(G.MESHES)                                      # the sweep is not a sweep of empty views


# ---- the render and index exports -----------------------------------------------------------------------------------
RENDERS = [((17, 33), (16, 16), 0, "jitter", 16, "valid"), ((40, 68), (70, 130), 1, "overhang", 64, "none"),
           ((5, 7), (17, 33), 2, "projective", 16, "nodata"), ((40, 68), (70, 130), 0, "holes", 16, "valid"),
           ((40, 68), (7, 9), 0, "fold", 32, "none"), ((2, 2), (1, 1), 0, "affine", 32, "none"),
           ((17, 33), (70, 130), 1, "bulge", 32, "nodata")]


def _render_case(n, kind, C):
    src_size, out_size, l, name, S, mask = RENDERS[n]
    img = R.level_image(kind, C, *src_size)
    if src_size[0] >= 3:                                                     # a block of 0 in all bands: A + B = 0 for nd
        img[-(src_size[0] // 3):, :src_size[1] // 3] = 0
    val = R.validity(*src_size, seed=n) if mask == "valid" else None
    return src_size, out_size, l, name, S, mask, img, val, R.NODATA[kind] if mask == "nodata" else None


@pytest.mark.parametrize("kind,C", R.KINDS + [("u8", 1)])
def test_grid_render_kernels_equal_the_restated_display(kind, C):
    top = 255 if kind == "u8" else 65535
    partly = 0
    for n in range(len(RENDERS)):
        src_size, out_size, l, name, S, mask, img, val, nodata = _render_case(n, kind, C)
        pairs = [[(top // 3, top // 3), (0, top), (3 * (top // 8), 5 * (top // 8)), (top // 10, top - top // 10)][(c + n) % 4]
                 for c in range(C)]
        for mode in (0, 1, 2):
            c = G.kernel_case(src_size, out_size, l, name, S, mode, n % 2, "identity")
            res, ok = G.run_case(img, val, c, mode, nodata, 0)
            src = _inside(_cut(img, c), 1 + mode)
            sval = None if val is None else _inside(_cut(val, c), 3)
            # 4 bytes per pixel at an aligned and at an odd address (the dword stores and not), and 1, 2 and 3 bytes
            shows = [((C - 1, 0, 0), 1, 200, 0), ((C - 1, 0, 0), 1, 0, 1 + mode), ((0,), 0, 77, 0), ((C - 1,), 1, 9, 2)]
            if C >= 3:
                shows.append(((0, 1, 2), 0, 200, mode))
            for bands, alpha, background, offset in shows:
                want = D.display(res, ok, bands, pairs, alpha, background)
                out = Out(want.size, np.uint8, offset)
                what = (f"window_grid_render_{kind} {src_size}->{out_size} C={C} shift={l} {name} step={S} mode={mode} {mask} "
                        f"bands={bands} alpha={alpha} background={background} offset={offset}")
                lib.check(_grid_render(kind, src, sval, c, C, bands, pairs, out.view, mode, nodata, alpha, background), what)
                _same(out.host(what), want, what)
            partly += int(ok.any() and not ok.all())
    assert partly >= len(RENDERS)                                            # views with valid and invalid pixels


@pytest.mark.parametrize("kind,C", [("u8", 3), ("u8", 4), ("u16", 1), ("u16", 2), ("u16", 4)])
def test_grid_index_render_kernels_equal_the_restated_index(kind, C):
    top = 255 if kind == "u8" else 65535
    cmap = np.random.default_rng(77).integers(0, 256, size=(256, 3)).astype(np.uint8)
    d_cmap = torch.from_numpy(cmap).cuda()
    undefined_some = 0
    for n in range(len(RENDERS)):
        src_size, out_size, l, name, S, mask, img, val, nodata = _render_case(n, kind, C)
        for mode in (0, 1, 2):
            c = G.kernel_case(src_size, out_size, l, name, S, mode, n % 2, "identity")
            res, ok = G.run_case(img, val, c, mode, nodata, 0)
            src = _inside(_cut(img, c), (1 + mode) * img.dtype.itemsize)
            sval = None if val is None else _inside(_cut(val, c), 3)
            for k, iname in enumerate(["band"] if C == 1 else ["nd", "difference", "band"]):
                t = n + mode + k
                a = t % C
                b = a if C == 1 else (a + 1 + t % (C - 1)) % C
                index = ("band", a) if iname == "band" else (iname, a, b)
                vmin, vmax = X.value_range(iname, top)
                pair = [(vmin, vmax), (vmin + (vmax - vmin) // 3, vmax - (vmax - vmin) // 4), (vmax // 5, vmax // 5)][t % 3]
                alpha, background = (t // 2) % 2, (200, 0)[t % 2]
                want = X.display_index(res, ok, index, pair, cmap, alpha, background)
                for offset in {0, 1 + mode}:
                    out = Out(want.size, np.uint8, offset)
                    what = (f"window_grid_index_render_{kind} {src_size}->{out_size} C={C} shift={l} {name} step={S} "
                            f"mode={mode} {mask} index={index} pair={pair} alpha={alpha} background={background} offset={offset}")
                    lib.check(_grid_index(kind, src, sval, c, C, index, pair, d_cmap, out.view, mode, nodata, alpha,
                                          background), what)
                    _same(out.host(what), want, what)
                if iname == "nd":
                    undefined_some += int((ok & (res[..., a].astype(np.int64) + res[..., b] == 0)).any())
    assert C == 1 or undefined_some > 0                                      # the zero block is met


# ---- refusals -------------------------------------------------------------------------------------------------------
def test_the_calls_refuse_through_their_error_return_and_write_nothing():
    src = torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda")
    out, oval = Out(8 * 8 * 4, np.uint8), Out(64, np.uint8)
    cmap = torch.zeros((256, 3), dtype=torch.uint8, device="cuda")
    eye = G.affine((Q, 0, 0, 0, Q, 0), (8, 8), 16)
    ok = {"sh": 8, "sw": 8, "sy0": 0, "sx0": 0, "shift": 0, "LH": 8, "LW": 8, "H": 8, "W": 8, "G": eye, "step": 16, "size": (8, 8)}
    full = [(0, 255)] * 3

    def mesh_with(at, value):
        g = eye.copy()
        g[at] = value
        return g
    for change, C, mode, word in (({"sh": 7}, 3, 0, "outside the source window"), ({}, 3, 3, "mode=3"), ({}, 2, 0, "C=2"),
                                  ({}, 5, 0, "C=5"), ({"step": 24}, 3, 0, "step=24"), ({"step": 8}, 3, 0, "step=8"),
                                  ({"G": mesh_with((1, 1, 0), 1 << 48)}, 3, 0, "node (1, 1)"),
                                  ({"G": mesh_with((0, 1, 1), G.NONE)}, 3, 0, "x entry"),
                                  ({"size": (8, (1 << 20) + 1)}, 3, 0, "output")):
        c = dict(ok, **change)
        assert _grid("u8", src, None, c, C, out.view, oval.view, mode, None, 0) == lib.DSIC_EINVAL
        assert word.encode() in lib.load().dsic_last_error(), word
        if C != 2:
            assert _grid_render("u8", src, None, c, C, (0, 1, 2), full, out.view, mode, None, 1, 0) == lib.DSIC_EINVAL
            assert word.encode() in lib.load().dsic_last_error(), word
            assert _grid_index("u8", src, None, c, C, ("nd", 0, 1), (-100, 100), cmap, out.view, mode, None, 1, 0) == lib.DSIC_EINVAL
            assert word.encode() in lib.load().dsic_last_error(), word
    assert _grid("u8", src, None, ok, 3, out.view, out.view[100:], 0, None, 0) == lib.DSIC_EINVAL
    assert b"overlap" in lib.load().dsic_last_error()                        # the output validity inside the output
    assert _grid("u8", src, None, ok, 3, src, None, 0, None, 0) == lib.DSIC_EINVAL
    host, dev = _mesh(ok)                                                    # the output over the device mesh
    assert getattr(lib.load(), "dsic_window_grid_u8")(_p(src), None, 8, 8, 0, 0, 3, 0, 8, 8, 8, 8, host.ctypes.data, _p(dev),
                                                      16, _p(dev), None, 2, 2, 0, -1, 0, _stream()) == lib.DSIC_EINVAL
    assert b"device mesh and dst overlap" in lib.load().dsic_last_error()
    with pytest.raises(ValueError, match="band 3"):
        lib.check(_grid_render("u8", src, None, ok, 3, (0, 1, 3), full, out.view, 0, None, 1, 0), "window_grid_render_u8")
    assert (out.host("refused calls") == 0x5A).all() and (oval.host("refused calls") == 0x5A).all() and not bool(src.any())
    assert np.array_equal(dev.cpu().numpy(), host)


# ---- the reader -----------------------------------------------------------------------------------------------------
def _mesh_views():
    """(mesh, size, step, level, resampling) over the 330 x 530 scene: tilted, bulged onto an overview, folded, holed
    and overhanging"""
    views = []
    for kind, size, S, level, resampling in (("projective", (96, 120), 16, None, "bilinear"), ("bulge", (80, 128), 32, None, "cubic"),
                                             ("fold", (50, 70), 16, 0, "nearest"), ("holes", (100, 150), 16, None, "cubic"),
                                             ("overhang", (64, 100), 64, None, "bilinear"), ("jitter", (40, 60), 16, 1, "bilinear")):
        views.append((G.mesh(kind, H0, W0, size, S), size, S, level, resampling))
    return views


def _restated(model, stream, st, mesh, size, S, resampling, ix0):
    """the restatement applied to decompress_region of the planned window"""
    level, lw = st["level"], st["level_window"]
    ix = codec.stream_index(stream, level=level)
    masked = "fill" in ix
    src = codec.decompress_region(model, stream, *lw, batch=BATCH, level=level, with_valid=masked)
    src, sval = (src[0].cpu().numpy(), src[1].cpu().numpy().astype(np.uint8)) if masked else (src.cpu().numpy(), None)
    fill = ix.get("fill", ix.get("nodata", 0))
    return G.gridded(src, sval, lw[0], lw[1], level, ix["H"], ix["W"], ix0["H"], ix0["W"], mesh, S, size, R.MODES[resampling],
                     ix.get("nodata"), fill)


@pytest.mark.parametrize("name", STREAMS)
def test_a_gridded_read_is_the_restatement_of_the_planned_window(name):
    model, stream = _open(name)
    ix0 = codec.stream_index(stream)
    levels = len(ix0.get("levels", [0]))
    picked = set()
    with codec.ImageReader(model, stream, batch=BATCH) as r:
        for mesh, size, S, level, resampling in _mesh_views():
            if level is not None and level >= levels:
                level = 0
            st, again = {}, {}
            got, valid = r.read_gridded(mesh, size, step=S, level=level, resampling=resampling, stats=st, with_valid=True)
            assert st["grid_step"] == S and st["level"] == (codec.grid_level(levels, mesh, S) if level is None else level)
            assert st["level"] == (G.level(levels, mesh, S) if level is None else level)
            lw = st["level_window"]
            LH, LW = r.levels[st["level"]]
            assert lw == codec.grid_window(st["level"], LH, LW, H0, W0, mesh, R.MODES[resampling]) and lw is not None
            want, ok = _restated(model, stream, st, mesh, size, S, resampling, ix0)
            assert got.is_cuda and got.is_contiguous() and tuple(got.shape) == size + (ix0["C"],)
            _same(got.cpu().numpy().ravel(), want, f"{name} {size} step {S} {resampling}")
            assert valid.dtype == torch.bool and np.array_equal(valid.cpu().numpy(), ok), (name, size)
            assert ok.any()
            ix = codec.stream_index(stream, level=st["level"])
            assert st["tiles"] == [(st["level"], t) for t in codec.window_tiles(ix, *lw)]
            held = list(r._meshes)                                           # the mesh's device copy is kept: no second upload
            same = r.read_gridded(mesh, size, step=S, level=level, resampling=resampling, stats=again)
            assert list(r._meshes) == held and len(held) <= 8
            assert again["decoded"] == 0 and again["hits"] == len(codec._coded_tiles(ix, [t for _, t in again["tiles"]]))
            assert torch.equal(same.view(torch.uint8), got.view(torch.uint8))
            picked.add(st["level"])
        if levels > 1:
            assert {0, 1} <= picked


@pytest.mark.parametrize("name", STREAMS)
def test_a_gridded_read_of_an_affine_mesh_is_the_warped_read(name):
    model, stream = _open(name)
    with codec.ImageReader(model, stream, batch=BATCH) as r:
        for matrix, size, level, resampling in _views():
            st = {}
            want, w_ok = r.read_warped(matrix, size, level=level, resampling=resampling, stats=st, with_valid=True)
            m = st["matrix_q16"]
            for S in codec.GRID_STEPS:
                gs = {}
                got, ok = r.read_gridded(codec.affine_grid(m, size, S), size, S, level=st["level"], resampling=resampling,
                                         with_valid=True, stats=gs)
                assert torch.equal(got.view(torch.uint8), want.view(torch.uint8)) and torch.equal(ok, w_ok), (name, matrix, S)
                lw, ww = gs["level_window"], st["level_window"]              # the mesh's box holds the affine one
                assert lw[0] <= ww[0] and lw[1] <= ww[1] and lw[0] + lw[2] >= ww[0] + ww[2] and lw[1] + lw[3] >= ww[1] + ww[3]
                free = r.read_gridded(codec.affine_grid(m, size, S), size, S, resampling=resampling, stats=gs)
                assert gs["level"] == st["level"] or level is not None      # grid_level is warp_level on an affine mesh
                if level is None:
                    assert torch.equal(free.view(torch.uint8), want.view(torch.uint8))


@pytest.mark.parametrize("name", ["plain", "nodata", "u16", "masked u16", "pyramid"])
def test_gridded_renders_are_the_stretch_and_the_index_of_the_gridded_read(name):
    model, stream = _open(name)
    cmap = np.random.default_rng(3).integers(0, 256, size=(256, 3)).astype(np.uint8)
    with codec.ImageReader(model, stream, batch=BATCH) as r, codec.ImageReader(model, stream, batch=BATCH) as plain:
        C, top = r.shape[2], 65535 if r.kind == codec.KIND_U16_HWC else 255
        pairs = [[(top // 10, top - top // 10), (0, top), (top // 4, top // 2), (top // 3, top // 3)][c] for c in range(C)]
        for k, (mesh, size, S, level, resampling) in enumerate(_mesh_views()):
            level = None if level is not None and level >= len(r.levels) else level
            bands = [(0, 1, 2), (C - 1, 0, 0), (1,)][k % 3]
            alpha, background = bool(k % 2) and name != "nodata", (0, 200)[(k // 2) % 2]
            st = {}
            got = r.render_gridded(mesh, size, S, level=level, bands=bands, stretch=pairs, alpha=alpha, background=background,
                                   resampling=resampling, stats=st)
            img, valid = plain.read_gridded(mesh, size, S, level=level, resampling=resampling, with_valid=True)
            want = D.display(img.cpu().numpy(), valid.cpu().numpy(), bands, pairs, alpha, background)
            assert got.dtype == torch.uint8 and got.is_contiguous() and np.array_equal(got.cpu().numpy(), want), (name, k)
            assert st["grid_step"] == S
            index = [("nd", 0, 1), ("difference", C - 1, 0), ("band", 1)][k % 3]
            vmin, vmax = X.value_range(index[0], top)
            pair = (vmin + (vmax - vmin) // 4, vmax - (vmax - vmin) // 4)
            got = r.render_index_gridded(mesh, size, index, S, level=level, stretch=pair, colormap=cmap, alpha=alpha,
                                         background=background, resampling=resampling)
            want = X.display_index(img.cpu().numpy(), valid.cpu().numpy(), index, pair, cmap, alpha, background)
            assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want), (name, k, index)
        mesh, size, S = _mesh_views()[0][:3]                                 # the default stretches are the siblings'
        if top == 65535:
            assert torch.equal(r.render_gridded(mesh, size, S), r.render_gridded(mesh, size, S, stretch=r.stretch()))
        assert torch.equal(r.render_index_gridded(mesh, size, ("nd", 0, 1), S),
                           r.render_index_gridded(mesh, size, ("nd", 0, 1), S, stretch=(-10000, 10000)))


def test_a_mesh_beside_the_image_launches_nothing_and_the_refusals():
    with codec.ImageReader(_model(), _stream_of("pyramid"), batch=BATCH) as r:
        before, st = r.stats, {}
        beside = codec.affine_grid((Q, 0, 400 * Q, 0, Q, 0), (20, 30), 16)
        holed = codec.affine_grid((Q, 0, 0, 0, Q, 0), (16, 16), 32)
        holed[0, 1, 0] = codec.GRID_NONE
        for mesh, size, S in ((beside, (20, 30), 16), (holed, (16, 16), 32)):
            got, valid = r.read_gridded(mesh, size, S, stats=st, with_valid=True)
            assert st["level_window"] is None and st["tiles"] == [] and r.stats["decoded"] == before["decoded"]
            assert tuple(got.shape) == size + (3,) and not bool(got.any()) and not bool(valid.any())
            shown = r.render_gridded(mesh, size, S, alpha=True, background=31, stats=st)
            assert st["tiles"] == [] and bool((shown[..., :3] == 31).all()) and not bool(shown[..., 3].any())
            shown = r.render_index_gridded(mesh, size, ("nd", 0, 1), S, alpha=True, background=32, stats=st)
            assert st["tiles"] == [] and bool((shown[..., :3] == 32).all()) and not bool(shown[..., 3].any())
        assert r.stats["decoded"] == before["decoded"]
        eye = codec.affine_grid((Q, 0, 0, 0, Q, 0), (8, 8), 16)
        for kw, word in (({"out": "f32"}, "float32"), ({"out": "u16"}, "u16"), ({"resampling": "average"}, "resampling"),
                         ({"level": 4}, "levels 0 .. 3"), ({"size": (0, 4)}, "size"), ({"step": 24}, "step"),
                         ({"size": (40, 8)}, "shape"), ({"grid": eye.astype(np.float32)}, "integer"),
                         ({"grid": np.full((2, 2, 2), 1 << 48)}, "2\\^48")):
            args = dict({"grid": eye, "size": (8, 8)}, **kw)
            with pytest.raises(ValueError, match=word):
                r.read_gridded(**args)
        for kw, word in (({"bands": (0, 1)}, "bands"), ({"stretch": [(9, 8)] * 3}, "stretch"), ({"background": 256}, "background")):
            with pytest.raises(ValueError, match=word):
                r.render_gridded(eye, (8, 8), **kw)
        with pytest.raises(ValueError, match="index"):
            r.render_index_gridded(eye, (8, 8), ("nd", 0, 7))
        assert r.stats["decoded"] == before["decoded"]
        assert torch.equal(r.read_gridded(eye, (8, 8)), r.read(0, 0, 8, 8))


# ---- the tool -------------------------------------------------------------------------------------------------------
def test_the_tool_writes_a_projective_view(tmp_path):
    model, stream = _model(), _stream_of("pyramid")
    sd = _PCACHE[("model", 3, 128, 192)][1]
    torch.save({"model": {k: torch.from_numpy(v) for k, v in sd.items()}}, tmp_path / "ckpt.pt")
    (tmp_path / "s.dsic").write_bytes(stream)
    tool = os.path.join(ROOT, "tools", "dsic_image.py")
    h = G.projective_h(H0, W0, 64, 100)
    p = subprocess.run([sys.executable, tool, "render", str(tmp_path / "s.dsic"), str(tmp_path / "view.npy"), "--weights",
                        str(tmp_path / "ckpt.pt"), "--batch", str(BATCH), "--projective", ",".join(repr(v) for row in h for v in row),
                        "--grid-step", "32", "--size", "64,100", "--resampling", "cubic", "--alpha"], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    mesh = G.projective(h, (64, 100), 32)
    np.save(tmp_path / "mesh.npy", mesh)
    with codec.ImageReader(model, io.BytesIO(stream), batch=BATCH) as reader:
        want = reader.render_gridded(mesh, (64, 100), 32, resampling="cubic", alpha=True)
        raw = reader.read_gridded(mesh, (64, 100), 32)
    assert np.array_equal(np.load(tmp_path / "view.npy"), want.cpu().numpy()) and want.shape == (64, 100, 4)
    assert "64x100" in p.stdout and "mesh view of 3x5 nodes at step 32" in p.stdout
    p = subprocess.run([sys.executable, tool, "decompress", str(tmp_path / "s.dsic"), str(tmp_path / "raw.npy"), "--weights",
                        str(tmp_path / "ckpt.pt"), "--batch", str(BATCH), "--grid", str(tmp_path / "mesh.npy"), "--grid-step",
                        "32", "--size", "64,100"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    assert np.array_equal(np.load(tmp_path / "raw.npy"), raw.cpu().numpy())
