"""Zonal statistics without a GPU: the restatement of tests/per_zone_ref.py against an independent formulation and against
index_ref; the sweep of the kernel tests; codec.zonal_table and codec.zonal_percentile on hand-made tables; the two
entry points in the header, in lib.py and in the recipe table; every refusal of the exports through the error return and
dsic_last_error (they return before the first HIP call); the refusals of codec.zonal_args and of the tool."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import index_ref as X
import per_zone_ref as Z
import per_zone_stream_cases as ZSC
import render_ref
import stream_cases as SC
from dsic_amd import codec, lib, view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dsic_zonal_stats_u8", "dsic_zonal_stats_u16")


# ---- the restatement ------------------------------------------------------------------------------------------------
def _independent(img, valid, nodata, zones, nz, of):
    """per zone np.where over float64 values: count, mean, std, min, max as floats"""
    if of is None:
        v = img.astype(np.float64)
        defined = np.ones(img.shape[:2], dtype=bool)
    else:
        A, B = img[:, :, of[1]].astype(np.float64), img[:, :, of[-1]].astype(np.float64)
        defined = np.ones(A.shape, dtype=bool)
        if of[0] == "band":
            v = A
        elif of[0] == "difference":
            v = A - B
        else:
            defined = A + B != 0
            v = np.floor(10000.0 * (A - B) / np.where(defined, A + B, 1.0) + 0.5)    # exact: the quotient is far from 2^53
        v = v[:, :, None]
    ok = defined & (zones < nz)
    if valid is not None:
        ok &= valid != 0
    if nodata is not None:
        ok &= (img != nodata).any(axis=2)
    out = {}
    for z in range(nz):
        where = np.where(ok & (zones == z))
        for k in range(v.shape[2]):
            x = v[:, :, k][where]
            out[z, k] = (x.size, x.mean(), x.std(), x.min(), x.max()) if x.size else (0,)
    return out


@pytest.mark.parametrize("kind,C,of,mask", [("u8", 3, None, "valid"), ("u16", 4, None, "nodata"), ("u16", 3, ("nd", 2, 0), "valid"),
                                            ("u8", 4, ("difference", 3, 0), "none"), ("u16", 1, ("band", 0), "nodata"),
                                            ("u8", 3, ("nd", 2, 0), "nothing")])
def test_the_restatement_agrees_with_an_independent_formulation(kind, C, of, mask):
    H, W, nz = 37, 129, 7
    img, val = Z.image(kind, C, H, W), Z.validity(H, W, mask)
    nodata = Z.NODATA[kind] if mask == "nodata" else None
    zones = Z.raster("noise_holes", H, W, nz)
    table, _ = Z.zonal(img, val, nodata, zones, nz, of)
    got, want = Z.result(table), _independent(img, val, nodata, zones, nz, of)
    # float64 eps times the largest zone's pixel count (under 4773 here), with room: 4773 * 2.2e-16 = 1.1e-12
    rel = lambda a, b: abs(a - b) <= 1e-9 * max(abs(a), abs(b), 1e-300)
    counted = 0
    for (z, k), w in want.items():
        assert got["count"][z, k] == w[0], (z, k)
        counted += w[0]
        if w[0]:
            assert rel(got["mean"][z, k], w[1]) and rel(got["std"][z, k], w[2]), (z, k, got["mean"][z, k], w[1], got["std"][z, k], w[2])
            assert got["min"][z, k] == w[3] and got["max"][z, k] == w[4]
        else:
            assert math.isnan(got["mean"][z, k]) and math.isnan(got["std"][z, k]) and got["min"][z, k] == got["max"][z, k] == 0
    assert (counted == 0) == (mask == "nothing")


def test_the_index_values_and_the_bins_are_those_of_index_ref():
    for kind, C in (("u8", 3), ("u16", 4)):
        img = Z.image(kind, C, 37, 129)
        top = X.top_of(img)
        for of in (("band", 1), ("difference", C - 1, 0), ("nd", C - 1, 0)):
            name, a, b = X.parse(of)
            v, u, defined = Z.values(img, of)
            u_ref, d_ref = X.index_value(img, name, a, b)
            vmin, vmax = X.value_range(name, top)
            assert np.array_equal(u[:, :, 0], u_ref) and np.array_equal(defined, d_ref)
            assert np.array_equal(v[:, :, 0], u_ref + vmin) and v[defined].min() >= vmin and v[defined].max() <= vmax
            # one zone, bins over the whole u range: the stretch of index_ref over its histogram of the same pixels
            val = Z.validity(37, 129, "valid")
            zones = np.zeros((37, 129), dtype=np.uint16)
            _, hist = Z.zonal(img, val, None, zones, 1, of, pairs=[(0, vmax - vmin)])
            h = X.histogram(img, val, None, of)
            want = np.bincount(X.stretch(np.arange(h.size), 0, vmax - vmin), weights=h, minlength=256).astype(np.int64)
            assert np.array_equal(hist[0, 0], want) and int(hist.sum()) == int(h.sum())
    # every band of a uint8 image with (0, 255): the exact band histogram
    img, val = Z.image("u8", 3, 37, 129), Z.validity(37, 129, "valid")
    _, hist = Z.zonal(img, val, None, np.zeros((37, 129), dtype=np.uint16), 1, None, pairs=[(0, 255)] * 3)
    assert np.array_equal(hist[0], render_ref.histogram(img, val, None))


def test_two_strips_into_one_table_are_one_call_on_the_whole():
    img, val = Z.image("u16", 3, 37, 129), Z.validity(37, 129, "valid")
    zones = Z.raster("blocks", 37, 129, 9)
    whole, hist = Z.zonal(img, val, None, zones, 9, None, pairs=[(0, 65535)] * 3)
    top, htop = Z.zonal(img[:20], val[:20], None, zones[:20], 9, None, pairs=[(0, 65535)] * 3)
    both, hboth = Z.zonal(img[20:], val[20:], None, zones[20:], 9, None, table=top, pairs=[(0, 65535)] * 3, hist=htop)
    assert np.array_equal(whole, both) and np.array_equal(hist, hboth)
    assert int(whole[:, :, 2].max()) > 1 << 32                      # a uint16 zone's sum of squares passes 2^32


def test_the_sweep_takes_every_value_of_every_axis():
    every = [(si, ki, r) + Z.sweep(si, ki, r) for si in range(len(Z.SHAPES)) for ki in range(len(Z.KINDS))
             for r in range(len(Z.RASTERS))]
    assert {e[3] for e in every} == set(Z.WHATS) and {e[4] for e in every} == set(Z.MASKS) and {e[5] for e in every} == set(Z.ZSEL)
    assert {e[6] for e in every} == {True, False}
    for axis, values in ((3, Z.WHATS), (4, Z.MASKS), (5, Z.ZSEL)):
        assert {(e[2], e[axis]) for e in every} == {(r, v) for r in range(len(Z.RASTERS)) for v in values}    # per raster
        assert {(e[0], e[axis]) for e in every} == {(s, v) for s in range(len(Z.SHAPES)) for v in values}     # per shape
        assert {(e[1], e[axis]) for e in every} == {(k, v) for k in range(len(Z.KINDS)) for v in values}      # per kind
    assert {(e[3], e[5]) for e in every} == {(w, z) for w in Z.WHATS for z in Z.ZSEL}
    assert {(e[3], e[6]) for e in every} == {(w, h) for w in Z.WHATS for h in (True, False)}
    assert {(e[5], e[6]) for e in every} == {(z, h) for z in Z.ZSEL for h in (True, False)}
    # 65535 zones carry bins where a pixel has one value (case() leaves them out where it has more): such cases exist
    one_value = lambda e: Z.n_values(Z.KINDS[e[1]][1], Z.index_of(e[3], Z.KINDS[e[1]][1])) == 1
    assert sum(e[5] == "max" and e[6] and one_value(e) for e in every) >= 4
    # the limit is the library's own, and the sweep stands on both sides of it
    assert Z.lds_zones(1) * 40 <= lib.ZONAL_LDS_BYTES < (Z.lds_zones(1) + 1) * 40
    assert Z.lds_zones(3) * 120 <= lib.ZONAL_LDS_BYTES < (Z.lds_zones(3) + 1) * 120
    assert Z.SHAPES[-1][0] * Z.SHAPES[-1][1] > 2048 * 256
    c = Z.case(3, 4, 5)                                            # a small case, and what it holds
    assert c["zones"].max() == 65535 and (c["zones"] >= c["Z"]).any() and c["table"].shape == (c["Z"], c["K"], 5)


# ---- zonal_table, zonal_percentile -----------------------------------------------------------------------------------
def test_zonal_table_on_hand_made_tables():
    big = 3_000_000_000                                             # pixels of 65535: the sum of squares passes 2^63
    words = Z.fresh(4, 2)
    words[0, 0] = [3, (-6) & Z.MASK, 14, (-3) & Z.MASK, (-1) & Z.MASK]           # -1, -2, -3
    words[0, 1] = [2, 10, 52, 4, 6]                                               # 4, 6
    words[2, 0] = [big, big * 65535, big * 65535 * 65535, 65535, 65535]
    words[3, 1] = [4, 0, 4 * 10000 ** 2, (-10000) & Z.MASK, 10000]                # +-10000 twice each
    assert big * 65535 * 65535 > 1 << 63
    for given in (words, words.view(np.int64)):
        t = codec.zonal_table(given)
        assert all(t[k].shape == (4, 2) for k in ("count", "sum", "sumsq", "min", "max", "mean", "std"))
        assert t["count"].dtype == t["sum"].dtype == t["min"].dtype == t["max"].dtype == np.int64
        assert t["sumsq"].dtype == np.uint64 and t["mean"].dtype == t["std"].dtype == np.float64
        assert t["count"].tolist() == [[3, 2], [0, 0], [big, 0], [0, 4]]
        assert t["sum"][0].tolist() == [-6, 10] and t["min"][0].tolist() == [-3, 4] and t["max"][0].tolist() == [-1, 6]
        assert t["mean"][0].tolist() == [-2.0, 5.0] and t["std"][0, 0] == math.sqrt(6 / 9) and t["std"][0, 1] == 1.0
        assert int(t["sumsq"][2, 0]) == big * 65535 * 65535 and t["mean"][2, 0] == 65535.0 and t["std"][2, 0] == 0.0
        assert t["mean"][3, 1] == 0.0 and t["std"][3, 1] == 10000.0 and (t["min"][3, 1], t["max"][3, 1]) == (-10000, 10000)
        empty = t["count"] == 0
        assert np.isnan(t["mean"][empty]).all() and np.isnan(t["std"][empty]).all()
        assert (t["min"][empty] == 0).all() and (t["max"][empty] == 0).all() and "hist" not in t
        want = Z.result(words)
        for key in want:
            assert np.array_equal(t[key], want[key], equal_nan=key in ("mean", "std")), key
    for bad in (words[:, :, :4], words.astype(np.float64), words[0]):
        with pytest.raises(ValueError, match="64-bit words"):
            codec.zonal_table(bad)
    with pytest.raises(ValueError, match="hist"):
        codec.zonal_table(words, np.zeros((4, 2, 255), dtype=np.uint32))


def test_zonal_percentile_on_hand_made_bins():
    words = Z.fresh(3, 1)
    hist = np.zeros((3, 1, 256), dtype=np.uint32)
    hist[0, 0, [10, 20, 30]] = [1, 2, 1]                            # 10, 20, 20, 30
    hist[2, 0, 255] = 0xFFFFFFFF                                    # a full uint32 counter stays positive
    words[0, 0] = [4, 80, 1800, 10, 30]
    words[2, 0] = [0xFFFFFFFF, 255 * 0xFFFFFFFF, 255 * 255 * 0xFFFFFFFF, 255, 255]
    for given in (hist, hist.view(np.int32)):
        t = codec.zonal_table(words, given)
        assert t["hist"].dtype == np.int64 and t["hist"][2, 0, 255] == 0xFFFFFFFF and t["hist"].min() == 0
        t["bins"] = np.array([(0, 255)])
        assert codec.zonal_percentile(t, 50)[:, 0].tolist()[0] == 20.0 and codec.zonal_percentile(t, 0)[0, 0] == 10.0
        assert codec.zonal_percentile(t, 100)[0, 0] == 30.0 and codec.zonal_percentile(t, 75)[0, 0] == 20.0
        assert codec.zonal_percentile(t, 76)[0, 0] == 30.0 and codec.zonal_percentile(t, 50)[2, 0] == 255.0
        assert math.isnan(codec.zonal_percentile(t, 50)[1, 0])
        # the rule is stretch_from_histogram's, zone by zone
        for q in (0, 2, 50, 98, 100):
            assert codec.zonal_percentile(t, q)[0, 0] == codec.stretch_from_histogram(t["hist"][0], (q, q))[0][0]
        # wider bins: bin k stands for lo + k (hi - lo) / 255 rounded half up, in value units
        t["bins"] = np.array([(-10000, 10000)])
        assert codec.zonal_percentile(t, 50)[0, 0] == -10000 + (2 * 20 * 20000 + 255) // 510
        assert codec.zonal_percentile(t, 100)[2, 0] == 10000.0
    with pytest.raises(ValueError, match="bins"):
        codec.zonal_percentile(codec.zonal_table(words), 50)
    with pytest.raises(ValueError):
        codec.zonal_percentile(t, 101)


# ---- the ABI and the recipes ----------------------------------------------------------------------------------------
def test_the_two_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "dsic_hip.h")).read()
    for name in NEW:
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert decl, name
        args = [a.split()[-1].lstrip("*") for a in decl.group(1).split(",")]
        assert args == ["img_hwc", "valid_hw", "zones_hw", "H", "W", "C", "nodata", "what", "band_a", "band_b", "Z", "stats", "lohi",
                        "hist", "stream"]
        res, types = lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(types) == 15 and getattr(lib.load(), name) is not None
    assert re.search(r"#define\s+DSIC_ZONAL_BANDS\s+\(-1\)", header) and lib.ZONAL_BANDS == -1
    assert int(re.search(r"#define\s+DSIC_ZONAL_LDS_BYTES\s+(\d+)", header).group(1)) == lib.ZONAL_LDS_BYTES
    declared = set(re.findall(r"\b(dsic_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == set(lib.SIGNATURES)
    assert "zonal_stats" in dir(codec.ImageReader) and "zonal_stats" in dir(codec.SceneStack)
    for n in ("zonal_table", "zonal_percentile", "zonal_args"):
        assert getattr(codec, n) is getattr(view, n)
    assert codec.ZONE_NONE == 65535


def test_the_zonal_recipes_are_in_the_table():
    assert len(ZSC.NAMES) == 4 and set(ZSC.NAMES) <= set(SC.names())
    L = lib.load()
    assert {e for n in ZSC.NAMES for e in SC.build(n, L).exports} == set(NEW)
    assert all(SC.family(n) == "views" for n in ZSC.NAMES)
    for n in ZSC.NAMES:
        c = SC.build(n, L)
        assert c.judged() == (["stats", "hist"] if n.endswith("_hist") else ["stats"]) and c.bufs["stats"]["inout"]
        assert c.bufs["stats"]["A"].tobytes() == Z.fresh(*c.bufs["stats"]["A"].shape[:2]).tobytes()
        assert c.restate(c.inputs("A")) != c.restate(c.inputs("B"))
    # both sides of the LDS limit are reached by the recipes
    sizes = {SC.build(n, L).bufs["stats"]["A"].nbytes for n in ZSC.NAMES}
    assert min(sizes) <= lib.ZONAL_LDS_BYTES < max(sizes)


# ---- the argument checks, without a GPU ---------------------------------------------------------------------------------
def test_the_zonal_calls_check_their_arguments_without_a_gpu():
    L = lib.load()
    E, err = lib.DSIC_EINVAL, L.dsic_last_error
    img, val, zon, tab, his = 1 << 20, 1 << 22, 1 << 24, 1 << 26, 1 << 28   # non-null, aligned, far apart
    ok = dict(img=img, valid=val, zones=zon, H=8, W=8, C=3, nodata=-1, what=-1, a=0, b=0, Z=4, stats=tab, lohi=None, hist=None)

    def call(kind, **kw):
        p = dict(ok, **kw)
        lohi = None if p["lohi"] is None else (ctypes.c_uint32 * len(p["lohi"]))(*p["lohi"])
        return getattr(L, "dsic_zonal_stats_" + kind)(p["img"], p["valid"], p["zones"], p["H"], p["W"], p["C"], p["nodata"],
                                                      p["what"], p["a"], p["b"], p["Z"], p["stats"], lohi, p["hist"], None)

    for kind, top in (("u8", 255), ("u16", 65535)):
        for name in ("img", "zones", "stats"):
            assert call(kind, **{name: None}) == E and b"null" in err()
        for C in (0, 5):
            assert call(kind, C=C) == E and f"C={C}".encode() in err()
        assert call(kind, H=0) == E and b"at least 1x1" in err()
        assert call(kind, W=0) == E and b"at least 1x1" in err()
        assert call(kind, H=1 << 16, W=1 << 16) == E and b"2^32" in err()
        for nz in (0, -1, 65536):
            assert call(kind, Z=nz) == E and f"Z={nz}".encode() in err()
        for what in (-2, 3):
            assert call(kind, what=what) == E and f"what={what}".encode() in err()
        assert call(kind, what=0, a=3) == E and b"band 3" in err()
        assert call(kind, what=2, a=0, b=-1) == E and b"band -1" in err()
        assert call(kind, what=1, a=-1, b=0) == E and b"band -1" in err()
        for nodata in (-2, top + 1):
            assert call(kind, nodata=nodata) == E and f"nodata={nodata}".encode() in err()
        assert call(kind, zones=zon + 1) == E and b"aligned" in err()
        assert call(kind, stats=tab + 4) == E and b"aligned" in err()
        assert call(kind, hist=his + 2, lohi=[0, 1] * 3) == E and b"aligned" in err()
        assert call(kind, hist=his) == E and b"lohi goes with hist" in err()
        assert call(kind, lohi=[0, 1] * 3) == E and b"lohi goes with hist" in err()
        assert call(kind, hist=his, lohi=[0, 1, 5, 4, 0, 1]) == E and b"pair (5, 4) of value 1" in err()
        assert call(kind, hist=his, lohi=[0, 1, 0, 1, 0, top + 1]) == E and f"<= {top}".encode() in err()
        assert call(kind, hist=his, lohi=[0, 2 * top + 1], what=1, a=0, b=1) == E and f"<= {2 * top}".encode() in err()
        assert call(kind, hist=his, lohi=[0, 20001], what=2, a=0, b=1) == E and b"<= 20000" in err()
        esz = 1 if kind == "u8" else 2
        assert call(kind, stats=img + 8 * 8 * 3 * esz - 8) == E and b"stats overlaps" in err()          # the image's last bytes
        assert call(kind, stats=val + 56) == E and b"stats overlaps" in err()
        assert call(kind, stats=zon - 4 * 3 * 40 + 8) == E and b"stats overlaps" in err()             # the table's last word
        assert call(kind, hist=img, lohi=[0, 1] * 3) == E and b"hist overlaps the image" in err()
        assert call(kind, hist=zon + 64, lohi=[0, 1] * 3) == E and b"hist overlaps the image" in err()
        assert call(kind, hist=tab + 4 * 3 * 40 - 4, lohi=[0, 1] * 3) == E and b"hist overlaps stats" in err()
        assert call(kind, hist=tab - 4 * 3 * 1024 + 4, lohi=[0, 1] * 3) == E and b"hist overlaps stats" in err()
    assert call("u16", img=img + 1) == E and b"2-byte" in err()
    # a band index reads band_b only where the kind has one
    assert call("u8", what=0, a=2, b=9, nodata=256) == E and b"nodata=256" in err()
    assert call("u8", what=-1, a=7, b=9, nodata=256) == E and b"nodata=256" in err()      # and the bands' none at all


def test_zonal_args_refuses_before_anything_is_read():
    z = np.zeros((4, 6), dtype=np.uint16)
    z[1, 2], z[3, 3] = 7, 65535
    zones, window, code, K, nz, vmin, pairs = codec.zonal_args("t", z, (10, 10), 3, 255, 2, 4)
    assert window == (2, 4, 4, 6) and code == (lib.ZONAL_BANDS, 0, 0) and (K, nz, vmin, pairs) == (3, 8, 0, None)
    assert codec.zonal_args("t", np.full((2, 2), 65535, dtype=np.uint16), (2, 2), 1, 255)[4] == 1
    _, _, code, K, nz, vmin, pairs = codec.zonal_args("t", z, (4, 6), 4, 65535, of=("nd", 3, 0), n_zones=3, bins=[(-2000, 8000)])
    assert code == (2, 3, 0) and (K, nz, vmin, pairs) == (1, 3, -10000, [(8000, 18000)])
    assert codec.zonal_args("t", z, (4, 6), 4, 65535, of=("difference", 1, 0), bins=[(-5, 5)])[5:] == (-65535, [(65530, 65540)])
    import torch
    assert codec.zonal_args("t", torch.from_numpy(z), (4, 6), 3, 255)[4] == 8
    for kw, word in ((dict(zones=z.astype(np.int32)), "uint16"), (dict(zones=z[0]), "uint16"), (dict(zones=[[1]]), "uint16"),
                     (dict(zones=torch.zeros((2, 2), dtype=torch.int16)), "uint16"),
                     (dict(y0=7), "leave the 10x10 level"), (dict(x0=5), "leave"), (dict(y0=-1), "leave"), (dict(y0=1.5), "integers"),
                     (dict(of=("nd", 3, 0)), "bands in 0 .. 2"), (dict(of=("ratio", 1, 0)), "index="), (dict(of=("band", 0, 1)), "index="),
                     (dict(n_zones=0), "n_zones=0"), (dict(n_zones=65536), "n_zones=65536"), (dict(n_zones=2.5), "not an integer"),
                     (dict(bins=[(0, 255)]), "one pair"), (dict(bins=[(0, 255)] * 2 + [(5, 4)]), "(5, 4)"),
                     (dict(bins=[(0, 256)] * 3), "<= 255"), (dict(bins=[(0, 1.5)] * 3), "integer pairs"),
                     (dict(of=("nd", 1, 0), bins=[(-10001, 0)]), "-10000 <= lo")):
        args = dict(zones=z, level_shape=(10, 10), C=3, top=255)
        args.update(kw)
        with pytest.raises(ValueError, match=re.escape(word)):
            codec.zonal_args("ImageReader.zonal_stats", **args)


def test_the_tool_refuses_bad_zonal_requests_before_it_loads_anything(tmp_path, capsys):
    import importlib.util
    spec = importlib.util.spec_from_file_location("dsic_image_tool", os.path.join(ROOT, "tools", "dsic_image.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    np.save(tmp_path / "z.npy", np.zeros((4, 4), dtype=np.uint16))
    np.save(tmp_path / "z32.npy", np.zeros((4, 4), dtype=np.int32))
    zones, out = ["--zones", str(tmp_path / "z.npy")], ["--out", str(tmp_path / "t.csv")]
    base = ["zonal", str(tmp_path / "none.dsic"), "--weights", "none.pt"]
    for extra, word in ((out, "zonal needs"), (zones, "zonal needs"), (zones + ["--out", "t.txt"], "zonal needs"),
                        (zones + out + ["--index", "nd:3,0", "--band", "1"], "exclude each other"),
                        (zones + out + ["--index", "ndvi:3,0"], "--index ndvi:3,0"), (zones + out + ["--band", "-1"], "0 or more"),
                        (zones + out + ["--at", "3"], "--at 3"), (zones + out + ["--at=-1,0"], "--at -1,0"),
                        (zones + out + ["--bins", "5,4"], "--bins 5,4"), (zones + out + ["--bins", "a,b"], "--bins a,b"),
                        (zones + out + ["--region", "0,0,4,4"], "zonal takes"), (zones + out + ["--alpha"], "zonal takes"),
                        (zones + out + ["--size", "4,4"], "zonal takes"), (zones + out + ["--reduce", "median"], "zonal takes"),
                        (["--zones", str(tmp_path / "no.npy")] + out, "no.npy"),
                        (["--zones", str(tmp_path / "z32.npy")] + out, "uint16")):
        with pytest.raises(SystemExit) as e:
            tool.main(base + extra)
        assert e.value.code == 2 and word in capsys.readouterr().err, (extra, word)
    assert not os.path.exists(tmp_path / "t.csv")
    for mode in (["decompress", "a.dsic", "b.npy"], ["render", "a.dsic", "b.npy"], ["compress", "a.npy", "b.dsic"]):
        with pytest.raises(SystemExit):
            tool.main(mode + ["--weights", "none.pt"] + zones)
        assert "go with zonal" in capsys.readouterr().err
    with pytest.raises(SystemExit):                                   # --out keeps its three kinds elsewhere
        tool.main(["decompress", "a.dsic", "b.npy", "--weights", "none.pt", "--out", "t.csv"])
    assert "invalid choice" in capsys.readouterr().err
