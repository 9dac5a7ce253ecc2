"""The stream recipes of the best-pixel exports (dsic_window_composite_pick_u8 / _u16), in the form of
tests/stream_cases.py and registered in its table when this module is imported, as tests/composite_stream_cases.py
registers its own: max over a normalised difference with the source plane, with and without validity windows.
test_best_pixel_cpu.py and test_gpu_best_pixel.py import this module, and both are collected before the files that read
the table."""
import ctypes

import numpy as np

import best_pixel_ref as BP
import stream_cases as SC
from composite_stream_cases import C, N, OH, OW, RECTS

NAMES = []
INDEX = ("nd", 2, 0)
IDS = [5, 254, 0]
FILL = 9


def _register(make, name):
    make.__name__ = name
    NAMES.append(name)
    if name not in SC.names():                   # a second import of this module adds nothing
        SC.RECIPES.append(make)


def _pick(kind, valid=True):
    export = "dsic_window_composite_pick_" + kind
    name = export[5:] + ("" if valid else "_all_valid")

    def make(L):
        c = SC.Case(name, export)
        dtype = np.uint8 if kind == "u8" else np.uint16
        top = 8 if kind == "u8" else 65536       # uint8: few values, so equal indices and A + B = 0 occur
        for i, (_, _, h, w) in enumerate(RECTS):
            SC._ab(c, f"src{i}", lambda r, h=h, w=w: r.integers(0, top, (h, w, C), dtype=dtype))
            if valid:
                SC._ab(c, f"sv{i}", SC._validity(h, w))
        c.out("dst", dtype, OH * OW * C)
        c.out("dv", SC.U8, OH * OW)
        c.out("dn", SC.U8, OH * OW)
        c.out("ds", SC.U8, OH * OW)
        fn = getattr(L, export)
        rect = (ctypes.c_int * (4 * N))(*[v for r in RECTS for v in r])
        nodata = (ctypes.c_int * N)(*[-1] * N)
        ids = (ctypes.c_int * N)(*IDS)

        def call(L, p, s):                       # the host pointer arrays, from the case's device buffers
            src = (ctypes.c_void_p * N)(*[getattr(p, f"src{i}") for i in range(N)])
            sv = (ctypes.c_void_p * N)(*[getattr(p, f"sv{i}") if valid else None for i in range(N)])
            return fn(src, sv, rect, nodata, ids, N, C, p.dst, p.dv, p.dn, p.ds, OH, OW, BP.MAX,
                      BP.index_ref.KINDS[INDEX[0]], INDEX[1], INDEX[2], FILL, s)
        c.call = call

        def restate(i):
            outs = BP.pick([i[f"src{k}"] for k in range(N)], [i[f"sv{k}"] if valid else None for k in range(N)], RECTS,
                           [-1] * N, IDS, C, OH, OW, BP.MAX, INDEX, FILL)
            return b"".join(o.tobytes() for o in outs)
        c.restate = restate
        return c
    _register(make, name)


for _k in ("u8", "u16"):
    _pick(_k)
    _pick(_k, False)
