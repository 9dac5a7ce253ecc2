"""The stream recipes of the composite exports (dsic_window_composite_u8 / _u16), in the form of tests/stream_cases.py
and registered in its table when this module is imported, as tests/index_stream_cases.py registers its own:
test_stream_cases_cpu.py asks a recipe of every export that takes a stream, and test_gpu_stream_order.py runs every
recipe of the table behind late inputs and beside a neighbour.  test_composite_cpu.py and test_gpu_composite.py import
this module, and both are collected before the files that read the table; once stream_cases.py itself may change, these
recipes belong at its end, beside the render recipes."""
import ctypes

import numpy as np

import composite_ref
import stream_cases as SC

NAMES = []
N, C = 3, 3
OH, OW = 24, 40
RECTS = [(0, 0, 16, 30), (5, 8, 19, 32), (2, 20, 20, 15)]        # overlapping by pairs and all three, a corner left open


def _register(make, name):
    make.__name__ = name
    NAMES.append(name)
    if name not in SC.names():                   # a second import of this module adds nothing
        SC.RECIPES.append(make)


def _composite(kind, valid=True):
    export = "dsic_window_composite_" + kind
    name = export[5:] + ("" if valid else "_all_valid")   # with and without validity windows

    def make(L):
        c = SC.Case(name, export)
        dtype = np.uint8 if kind == "u8" else np.uint16
        top = 256 if kind == "u8" else 65536
        for i, (_, _, h, w) in enumerate(RECTS):
            SC._ab(c, f"src{i}", lambda r, h=h, w=w: r.integers(0, top, (h, w, C), dtype=dtype))
            if valid:
                SC._ab(c, f"sv{i}", SC._validity(h, w))
        c.out("dst", dtype, OH * OW * C)
        c.out("dv", SC.U8, OH * OW)
        c.out("dn", SC.U8, OH * OW)
        fn = getattr(L, export)
        rect = (ctypes.c_int * (4 * N))(*[v for r in RECTS for v in r])
        nodata = (ctypes.c_int * N)(*[-1] * N)

        def call(L, p, s):                       # the host pointer arrays, from the case's device buffers
            src = (ctypes.c_void_p * N)(*[getattr(p, f"src{i}") for i in range(N)])
            sv = (ctypes.c_void_p * N)(*[getattr(p, f"sv{i}") if valid else None for i in range(N)])
            return fn(src, sv, rect, nodata, N, C, p.dst, p.dv, p.dn, OH, OW, composite_ref.MEDIAN, 9, s)
        c.call = call

        def restate(i):
            dst, dv, dn = composite_ref.composite([i[f"src{k}"] for k in range(N)],
                                                  [i[f"sv{k}"] if valid else None for k in range(N)], RECTS, [-1] * N, C,
                                                  OH, OW, composite_ref.MEDIAN, 9)
            return dst.tobytes() + dv.tobytes() + dn.tobytes()
        c.restate = restate
        return c
    _register(make, name)


for _k in ("u8", "u16"):
    _composite(_k)
    _composite(_k, False)
