"""The stream recipes of the zonal exports (dsic_zonal_stats_u8 / _u16), in the form of tests/stream_cases.py and
registered in its table when this module is imported, as tests/index_stream_cases.py registers its own.  One recipe per
width, without and with the per-zone histogram: uint8 measures the three bands of 9 zones, a table gathered in LDS;
uint16 measures a normalised difference over one zone more than LDS holds, so its spills are global atomics.  The zone
rasters hold ids at and above Z, which belong to no zone.  The table is an input that the call works on in place: it is
loaded with its initial words (0, 0, 0, INT64_MAX, INT64_MIN) before every call, as a histogram is zeroed; the histogram
is zeroed.  test_per_zone_cpu.py and test_gpu_per_zone.py import this module, and both are collected before the files
that read the table."""
import ctypes

import numpy as np

import per_zone_ref as Z
import stream_cases as SC

NAMES = []
SHAPE = {"u8": (3, None, 9), "u16": (3, ("nd", 2, 0), Z.lds_zones(1) + 1)}      # C, of, the zone count


def _register(make, name):
    make.__name__ = name
    NAMES.append(name)
    if name not in SC.names():                   # a second import of this module adds nothing
        SC.RECIPES.append(make)


def _pairs(kind, of, K):
    top = Z.u_top(kind, of)
    return [(0, top), (top // 7, top - top // 5), (3, top // 2)][:K]


def _zonal(kind, with_hist):
    export = "dsic_zonal_stats_" + kind
    name = export[5:] + ("_hist" if with_hist else "")

    def make(L):
        c = SC.Case(name, export)
        C, of, nz = SHAPE[kind]
        K = Z.n_values(C, of)
        SC._ab(c, "img", SC._img(np.uint8 if kind == "u8" else np.uint16, C))
        SC._ab(c, "v", SC._validity(SC.IH, SC.IW))
        SC._ab(c, "zones", lambda r: r.integers(0, nz + 3, (SC.IH, SC.IW)).astype(np.uint16), bound=(0, 65536))
        c.inp("stats", Z.fresh(nz, K), Z.fresh(nz, K), inout=True)
        pairs = _pairs(kind, of, K) if with_hist else None
        if with_hist:
            c.out("hist", SC.U32, nz * K * 256, zero=True)
            c.hostarr("lohi", ctypes.c_uint32, [v for pair in pairs for v in pair])
        fn = getattr(L, export)
        code = Z.what_code(of)
        c.call = lambda L, p, s: fn(p.img, p.v, p.zones, SC.IH, SC.IW, C, -1, *code, nz, p.stats,
                                    p.lohi if with_hist else None, p.hist if with_hist else None, s)

        def restate(i):
            table, hist = Z.zonal(i["img"], i["v"], None, i["zones"], nz, of, table=i["stats"], pairs=pairs)
            return table.tobytes() + (hist.tobytes() if with_hist else b"")
        c.restate = restate
        return c
    _register(make, name)


for _k in ("u8", "u16"):
    _zonal(_k, False)
    _zonal(_k, True)

if "zonal_" not in SC.FAMILIES["views"]:
    SC.FAMILIES["views"] += ("zonal_",)                      # the family of the histograms
