"""The stream recipes of the index exports (dsic_window_index_render_*, dsic_window_warp_index_render_*,
dsic_index_histogram_*), in the form of tests/stream_cases.py and registered in its table when this module is imported:
test_stream_cases_cpu.py asks a recipe of every export that takes a stream, and test_gpu_stream_order.py runs every
recipe of the table behind late inputs and beside a neighbour.  test_index_cpu.py and test_gpu_index.py import this
module, and both are collected before the files that read the table; once stream_cases.py itself may change, these
recipes belong at its end, beside the render and warp recipes they are modelled on."""
import ctypes

import numpy as np

import index_ref
import stream_cases as SC

ND, DIFFERENCE = index_ref.KINDS["nd"], index_ref.KINDS["difference"]
NAMES = []


def _register(make, name):
    make.__name__ = name
    NAMES.append(name)
    if name not in SC.names():                   # a second import of this module adds nothing
        SC.RECIPES.append(make)


def _cmap(c):
    SC._ab(c, "cmap", lambda r: r.integers(0, 256, (256, 3), dtype=np.uint8))


def _show(kind):
    """index, bands, the pair in index units: a normalised difference for uint8, a difference for uint16"""
    return (ND, 2, 0, -4000, 6000) if kind == "u8" else (DIFFERENCE, 0, 1, -30000, 50000)


def _render(kind, valid=True):
    export = "dsic_window_index_render_" + kind
    name = export[5:] + ("" if valid else "_all_valid")   # with and without a validity window: two launch statements

    def make(L):
        c = SC.Case(name, export)
        SC._view_src(c, kind, 3, valid)
        _cmap(c)
        c.out("dst", SC.U8, SC.OH * SC.OW * 4)
        fn = getattr(L, export)
        c.call = lambda L, p, s: fn(p.src, p.sv if valid else None, SC.IH, SC.IW, 0, 0, 3, 0, *SC.REGION, *_show(kind), p.cmap,
                                    p.dst, SC.OH, SC.OW, 0, -1, 1, 17, s)
        return c
    _register(make, name)


def _warp(kind, valid=True):
    export = "dsic_window_warp_index_render_" + kind
    name = export[5:] + ("" if valid else "_all_valid")

    def make(L):
        c = SC.Case(name, export)
        SC._view_src(c, kind, 3, valid)
        _cmap(c)
        c.hostarr("m", ctypes.c_int64, SC.WARP_M)
        c.out("dst", SC.U8, SC.WOH * SC.WOW * 4)
        fn = getattr(L, export)
        geo = (SC.IH, SC.IW, 0, 0, 3, 0, SC.IH, SC.IW, SC.IH, SC.IW)
        c.call = lambda L, p, s: fn(p.src, p.sv if valid else None, *geo, p.m, *_show(kind), p.cmap, p.dst, SC.WOH, SC.WOW, 2,
                                    -1, 1, 17, s)
        return c
    _register(make, name)


def _histogram(kind, index):
    """nd: 20001 global counters; a uint8 difference: 511 counters in LDS; a uint16 difference: 131071 global ones"""
    export = "dsic_index_histogram_" + kind
    name = f"index_histogram_{kind}_{index[0]}"

    def make(L):
        c = SC.Case(name, export)
        dtype = np.uint8 if kind == "u8" else np.uint16
        SC._ab(c, "img", SC._img(dtype, 3))
        SC._ab(c, "v", SC._validity(SC.IH, SC.IW))
        vmin, vmax = index_ref.value_range(index[0], 255 if kind == "u8" else 65535)
        c.out("hist", SC.U32, vmax - vmin + 1, zero=True)
        fn = getattr(L, export)
        c.call = lambda L, p, s: fn(p.img, p.v, SC.IH, SC.IW, 3, -1, index_ref.KINDS[index[0]], index[1], index[2], p.hist, s)
        c.restate = lambda i: index_ref.histogram(i["img"], i["v"], None, index).astype(np.uint32).tobytes()
        return c
    _register(make, name)


for _k in ("u8", "u16"):
    _render(_k)
    _render(_k, False)
    _warp(_k)
    _warp(_k, False)
    _histogram(_k, ("nd", 2, 0))
    _histogram(_k, ("difference", 0, 1))

if "index_histogram" not in SC.FAMILIES["views"]:
    SC.FAMILIES["views"] += ("index_histogram",)           # the family of the band histogram
