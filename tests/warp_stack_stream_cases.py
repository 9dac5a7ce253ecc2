"""The stream recipes of the warped-stack exports (dsic_window_warp_composite_u8 / _u16), in the form of
tests/stream_cases.py and registered in its table when this module is imported, as tests/best_pixel_stream_cases.py
registers its own: three sources under three views, the median with the count plane and the maximum of a normalised
difference with the source plane.  test_warp_stack_cpu.py and test_gpu_warp_stack.py import this module."""
import ctypes

import numpy as np

import stream_cases as SC
import warp_ref as R
import warp_stack_ref as WS
from dsic_amd import lib

NAMES = []
N, C, OH, OW = 3, 3, 17, 33
IDS = [5, 254, 0]
FILL = 9
VIEWS = [("rot30", 0, 24, 40), ("mirror", 1, 20, 30), ("overhang", 0, 12, 20)]        # view, shift, the level's size


def _register(make, name):
    make.__name__ = name
    NAMES.append(name)
    if name not in SC.names():                   # a second import of this module adds nothing
        SC.RECIPES.append(make)


def _geometry(sample):
    out = []
    for view, l, LH, LW in VIEWS:
        H, W = R.image_size(LH, l), R.image_size(LW, l)
        out.append(dict(sy0=0, sx0=0, sh=LH, sw=LW, shift=l, LH=LH, LW=LW, H=H, W=W, m=R.matrix(view, H, W, OH, OW), nodata=-1))
    return out


def _recipe(kind, reduce, index, sample):
    export = "dsic_window_warp_composite_" + kind
    name = export[5:] + "_" + {WS.MEDIAN: "median", WS.MAX: "max"}[reduce]

    def make(L):
        c = SC.Case(name, export)
        dtype = np.uint8 if kind == "u8" else np.uint16
        top = 8 if kind == "u8" else 65536       # uint8: few values, so equal indices and A + B = 0 occur
        geo = _geometry(sample)
        for i, g in enumerate(geo):
            SC._ab(c, f"src{i}", lambda r, g=g: r.integers(0, top, (g["sh"], g["sw"], C), dtype=dtype))
            SC._ab(c, f"sv{i}", SC._validity(g["sh"], g["sw"]))
        c.out("dst", dtype, OH * OW * C)
        c.out("dv", SC.U8, OH * OW)
        c.out("dn", SC.U8, OH * OW)
        if reduce == WS.MAX:
            c.out("ds", SC.U8, OH * OW)
        fn = getattr(L, export)
        kinds = {"band": 0, "difference": 1, "nd": 2}

        def call(L, p, s):                       # the host table, from the case's device buffers
            table = (lib.WarpSource * N)()
            for i, g in enumerate(geo):
                table[i] = lib.WarpSource(getattr(p, f"src{i}"), getattr(p, f"sv{i}"), g["sh"], g["sw"], 0, 0, g["shift"], g["LH"],
                                          g["LW"], g["H"], g["W"], -1, IDS[i], 0, (ctypes.c_int64 * 6)(*g["m"]))
            return fn(table, N, C, p.dst, p.dv, p.dn, p.ds if reduce == WS.MAX else None, OH, OW, sample, reduce,
                      kinds[index[0]], index[1], index[-1], FILL, s)
        c.call = call

        def restate(i):
            srcs = [dict(g, src=i[f"src{k}"].reshape(g["sh"], g["sw"], C), val=i[f"sv{k}"].reshape(g["sh"], g["sw"]))
                    for k, g in enumerate(geo)]
            outs = WS.warp_composite(srcs, C, (OH, OW), sample, reduce, index, FILL, IDS)
            return b"".join(o.tobytes() for o in outs if o is not None)
        c.restate = restate
        return c
    _register(make, name)


for _k in ("u8", "u16"):
    _recipe(_k, WS.MEDIAN, ("band", 0), 0)
    _recipe(_k, WS.MAX, ("nd", 2, 0), 2)
