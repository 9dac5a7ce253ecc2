"""The stream recipes of the gridded exports (dsic_window_grid_u8 / _u16, dsic_window_grid_render_*,
dsic_window_grid_index_render_*), in the form of tests/stream_cases.py and registered in its table when this module is
imported, as tests/index_stream_cases.py registers its own: the warp recipes' source and output under a jittered mesh
of 3 x 3 nodes.  The mesh is one array in both input sets, since the call checks its host copy against the window.
test_grid_cpu.py and test_gpu_grid.py import this module."""
import ctypes

import numpy as np

import grid_ref as GR
import stream_cases as SC

NAMES = []
STEP = 16
MESH = GR.mesh("jitter", SC.IH, SC.IW, (SC.WOH, SC.WOW), STEP)


def _register(make, name):
    make.__name__ = name
    NAMES.append(name)
    if name not in SC.names():                   # a second import of this module adds nothing
        SC.RECIPES.append(make)


def _grid(kind, what, valid=True):
    export = "dsic_window_grid_" + what + kind
    name = export[5:] + ("" if valid else "_all_valid")   # with and without a validity window: two launch statements

    def make(L):
        c = SC.Case(name, export)
        SC._view_src(c, kind, 3, valid)
        c.same("mesh", MESH, bound=(-(1 << 48), 1 << 48))
        c.hostarr("mesh_host", ctypes.c_int64, [int(v) for v in MESH.ravel()])
        fn = getattr(L, export)
        sv = (lambda p: p.sv) if valid else (lambda p: None)
        geo = (SC.IH, SC.IW, 0, 0, 3, 0, SC.IH, SC.IW, SC.IH, SC.IW)
        if what == "render_":
            SC._display(c, kind)
            c.out("dst", SC.U8, SC.WOH * SC.WOW * 4)
            c.call = lambda L, p, s: fn(p.src, sv(p), *geo, p.mesh_host, p.mesh, STEP, p.bands, 3, p.lohi8, p.dst, SC.WOH,
                                        SC.WOW, 2, -1, 1, 17, s)
        elif what == "index_render_":
            SC._ab(c, "cmap", lambda r: r.integers(0, 256, (256, 3), dtype=np.uint8))
            show = (2, 2, 0, -4000, 6000) if kind == "u8" else (1, 0, 1, -30000, 50000)   # nd; difference
            c.out("dst", SC.U8, SC.WOH * SC.WOW * 4)
            c.call = lambda L, p, s: fn(p.src, sv(p), *geo, p.mesh_host, p.mesh, STEP, *show, p.cmap, p.dst, SC.WOH, SC.WOW,
                                        2, -1, 1, 17, s)
        else:
            c.out("dst", SC.U8 if kind == "u8" else SC.U16, SC.WOH * SC.WOW * 3)
            c.out("dv", SC.U8, SC.WOH * SC.WOW)
            c.call = lambda L, p, s: fn(p.src, sv(p), *geo, p.mesh_host, p.mesh, STEP, p.dst, p.dv, SC.WOH, SC.WOW, 2, -1,
                                        9, s)

            def restate(i):
                img, ok = GR.gridded(i["src"], i.get("sv"), 0, 0, 0, SC.IH, SC.IW, SC.IH, SC.IW, MESH, STEP,
                                     (SC.WOH, SC.WOW), 2, None, 9)
                return img.tobytes() + ok.astype(np.uint8).tobytes()
            c.restate = restate
        return c
    _register(make, name)


for _k in ("u8", "u16"):
    for _v in (True, False):
        for _w in ("", "render_", "index_render_"):
            _grid(_k, _w, _v)
