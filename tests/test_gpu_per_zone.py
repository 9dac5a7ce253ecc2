"""Zonal statistics on the GPU.  The kernel alone, every table word and every bin against the restatement of
tests/per_zone_ref.py, outputs between guards and inputs inside larger allocations as in test_gpu_grid.py; strips that
accumulate into one table; the refusals, which write nothing; then codec.ImageReader.zonal_stats and
codec.SceneStack.zonal_stats on the scenes of test_gpu_render.py and test_gpu_composite.py against the restatement applied
to what read returns for the same window; and the command-line tool."""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import index_ref as X
import per_zone_ref as Z
import per_zone_stream_cases as ZSC  # (its recipes join the table that test_gpu_stream_order.py runs)
import stream_cases as SC
from dsic_amd import codec, lib
from dsic_amd.ops import _p, _stream
from test_gpu_composite import _extra_reader
from test_gpu_pyramid import Out, _inside, _same
from test_gpu_render import _CACHE, BATCH, H0, W0, _model, _np, _reader, _stream_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the kernel -----------------------------------------------------------------------------------------------------
def _table_out(table, offset=0):
    """a table's words between guards, holding `table`"""
    out = Out(table.size, np.int64, offset)
    out.view.copy_(torch.from_numpy(np.ascontiguousarray(table).view(np.int64).ravel()).cuda())
    return out


def _hist_out(Zn, K, offset=0):
    out = Out(Zn * K * 256, np.int32, offset)
    out.view.zero_()
    return out


def _call(kind, img, valid, zones, H, W, C, nodata, of, Zn, table, pairs, hist):
    lohi = None if pairs is None else codec._lohi(pairs)
    return getattr(lib.load(), "dsic_zonal_stats_" + kind)(
        _p(img), None if valid is None else _p(valid), _p(zones), H, W, C, -1 if nodata is None else nodata, *Z.what_code(of),
        Zn, _p(table), lohi, None if hist is None else _p(hist), _stream())


def _same_hist(hist, want, what):
    got = hist.host(what).view(np.uint32)
    at = np.flatnonzero(got)
    assert np.array_equal(at, want[0]) and np.array_equal(got[at], want[1]), what + ": the bins"


@pytest.mark.parametrize("si", range(len(Z.SHAPES)))
@pytest.mark.parametrize("ki", range(len(Z.KINDS)))
def test_the_kernel_equals_the_restatement(si, ki):
    counted = 0
    for r in range(len(Z.RASTERS)):
        c = Z.case(si, ki, r)
        what = "zonal_stats_" + c["what"]
        img = _inside(c["img"], (r + si) % 4)                                   # the inputs at several element offsets
        val = None if c["valid"] is None else _inside(c["valid"], (r + 2 * ki) % 4)
        zones = _inside(c["zones"], (r + ki) % 3)
        table = _table_out(Z.fresh(c["Z"], c["K"]), r % 2)
        hist = None if c["pairs"] is None else _hist_out(c["Z"], c["K"], (r + 1) % 3)
        lib.check(_call(c["kind"], img, val, zones, c["H"], c["W"], c["C"], c["nodata"], c["of"], c["Z"], table.view,
                        c["pairs"], hist and hist.view), what)
        _same(table.host(what).view(np.uint64), c["table"], what)
        if hist is not None:
            _same_hist(hist, c["hist"], what)
        counted += int(c["table"][:, :, 0].sum())
    assert counted > 0                                                          # the sweep is not a sweep of empty zones


def test_two_strips_into_one_table_equal_one_call_on_the_whole():
    for kind, C, of, Zn in (("u16", 3, None, 9), ("u8", 4, ("nd", 3, 0), Z.lds_zones(1) + 1)):      # LDS; global atomics
        H, W = 37, 129
        img, val, zones = Z.image(kind, C, H, W), Z.validity(H, W, "valid"), Z.raster("blocks", H, W, Zn)
        K = Z.n_values(C, of)
        pairs = [(0, Z.u_top(kind, of))] * K
        want, want_hist = Z.zonal(img, val, None, zones, Zn, of, pairs=pairs)
        table, hist = _table_out(Z.fresh(Zn, K)), _hist_out(Zn, K)
        for rows in (slice(0, 20), slice(20, H)):                               # no host work between the two calls
            h = rows.stop - rows.start
            lib.check(_call(kind, _inside(img[rows], 1), _inside(val[rows], 3), _inside(zones[rows], 1), h, W, C, None, of, Zn,
                            table.view, pairs, hist.view), kind)
        _same(table.host(kind).view(np.uint64), want, f"{kind}: two strips")
        _same(hist.host(kind).view(np.uint32), want_hist, f"{kind}: two strips, the bins")
        if kind == "u16":
            assert int(want[:, :, 2].max()) > 1 << 32                           # a zone's sum of squares past 2^32


def test_the_recipes_equal_their_restatement():
    """the stream recipes' own shapes, once on the default stream: table and bins, byte for byte"""
    L = lib.load()
    for name in ZSC.NAMES:
        case = SC.build(name, L)
        i = case.inputs("A")
        dev = {k: _inside(v.view(np.int64) if v.dtype == np.uint64 else v, 0) for k, v in i.items()}
        addr = {k: _p(t) for k, t in dev.items()}
        if "hist" in case.bufs:
            dev["hist"] = torch.zeros(case.bufs["hist"]["n"], dtype=torch.int32, device="cuda")
            addr["hist"] = _p(dev["hist"])
        lib.check(case.call(L, SC.Ptrs(addr, case.host), _stream()), name)
        got = _np(dev["stats"]).tobytes() + (_np(dev["hist"]).tobytes() if "hist" in dev else b"")
        assert got == case.restate(i), name


def test_refused_calls_write_nothing():
    H, W, C, Zn = 8, 8, 3, 4
    img = torch.zeros((H, W, C), dtype=torch.uint8, device="cuda")
    val = torch.ones((H, W), dtype=torch.uint8, device="cuda")
    zones = torch.zeros((H, W), dtype=torch.int16, device="cuda")
    fresh = Z.fresh(Zn, C)
    table, hist = _table_out(fresh), _hist_out(Zn, C)
    ok = dict(img=img.data_ptr(), valid=val.data_ptr(), zones=zones.data_ptr(), H=H, W=W, C=C, nodata=-1, what=-1, a=0, b=0,
              Z=Zn, stats=table.view.data_ptr(), pairs=[(0, 255)] * 3, hist=hist.view.data_ptr())      # addresses as integers

    def call(**kw):
        p = dict(ok, **kw)
        return lib.load().dsic_zonal_stats_u8(p["img"], p["valid"], p["zones"], p["H"], p["W"], p["C"], p["nodata"], p["what"],
                                              p["a"], p["b"], p["Z"], p["stats"], None if p["pairs"] is None else codec._lohi(p["pairs"]),
                                              p["hist"], _stream())

    for kw, word in ((dict(img=None), "null"), (dict(zones=None), "null"), (dict(C=5), "C=5"), (dict(H=0), "at least 1x1"),
                     (dict(Z=0), "Z=0"), (dict(Z=65536), "Z=65536"), (dict(what=3), "what=3"), (dict(what=2, a=0, b=3), "band 3"),
                     (dict(nodata=256), "nodata=256"), (dict(stats=table.view.data_ptr() + 4), "aligned"),
                     (dict(hist=hist.view.data_ptr() + 2), "aligned"), (dict(pairs=None), "lohi goes with hist"),
                     (dict(pairs=[(0, 255), (9, 8), (0, 255)]), "pair (9, 8)"), (dict(pairs=[(0, 256)] * 3), "<= 255"),
                     (dict(stats=val.data_ptr()), "stats overlaps"), (dict(hist=zones.data_ptr()), "hist overlaps the image"),
                     (dict(hist=table.view.data_ptr() + 8), "hist overlaps stats")):
        assert call(**kw) == lib.DSIC_EINVAL and word.encode() in lib.load().dsic_last_error(), word
    torch.cuda.synchronize()
    _same(table.host("refused calls").view(np.uint64), fresh, "refused calls: the table")
    assert not hist.host("refused calls").any() and not bool(img.any()) and bool(val.all()) and not bool(zones.any())
    assert call() == lib.DSIC_OK
    got = table.host("a legal call").view(np.uint64).reshape(Zn, C, 5)
    assert got[0, :, 0].tolist() == [64] * 3 and np.array_equal(got[1:], fresh[1:]) and int(hist.host("a legal call").sum()) == 192


# ---- the reader -----------------------------------------------------------------------------------------------------
def _zones_for(h, w, n, seed):
    """blocks of 16 x 24 pixels numbered through 0 .. n - 1, speckled with 65535, and the one-pixel zone n: n + 1 zones"""
    y, x = np.mgrid[0:h, 0:w]
    zones = (((y // 16) * 5 + x // 24) % n).astype(np.uint16)
    zones[np.random.default_rng(seed).random((h, w)) < 0.05] = 65535
    zones[0, 0] = n
    return zones


def _restated(img, valid, nodata, zones, n, of, pairs_v=None):
    """zonal_table's dict from the restatement; pairs_v in value units"""
    vmin = 0 if of is None else X.value_range(of[0], X.top_of(img))[0]
    pairs = None if pairs_v is None else [(lo - vmin, hi - vmin) for lo, hi in pairs_v]
    return Z.result(*Z.zonal(img, valid, nodata, zones, n, of, pairs=pairs))


def _same_result(got, want, what):
    assert set(got) - {"bins"} == set(want), what
    for key, w in want.items():
        assert got[key].dtype == w.dtype and got[key].shape == w.shape, (what, key)
        assert np.array_equal(got[key], w, equal_nan=key in ("mean", "std")), (what, key)


@pytest.mark.parametrize("name", ["u8", "u16_valid", "u8_nodata", "f32"])
def test_a_readers_zonal_stats_are_the_restatement_of_its_read(name):
    with _reader(name) as r, _reader(name) as plain:
        C = r.shape[2]
        out = "u8" if name == "f32" else None
        levels = [0, 2] if len(r.levels) == 3 else [0]
        for level in levels:
            LH, LW = r.levels[level]
            ix = plain.index(level)
            for k, (y0, x0, h, w) in enumerate(((LH // 3, LW // 4, LH // 2, LW // 2), (0, 0, LH, LW), (LH - 1, LW - 1, 1, 1))):
                zones = _zones_for(h, w, 6, k)
                if name == "u16_valid" or name == "u8_nodata":
                    img, valid = plain.read(y0, x0, h, w, level=level, out=out, with_valid=name == "u16_valid"), None
                    if name == "u16_valid":
                        img, valid = img
                        valid = _np(valid).astype(np.uint8)
                else:
                    img, valid = plain.read(y0, x0, h, w, level=level, out=out), None
                img = _np(img)
                top = X.top_of(img)
                for of, bins in ((None, None), (("nd", C - 1, 0), [(-3000, 9000)]), (None, [(0, top)] * C),
                                 (("difference", 0, C - 1), None), (("band", 1), [(10, top // 2)])):
                    st = {}
                    zt = torch.from_numpy(zones).cuda() if k == 1 else zones     # a device tensor serves as well
                    got = r.zonal_stats(zt, y0, x0, level=level, of=of, bins=bins, stats=st)
                    what = f"{name} level {level} window {(y0, x0, h, w)} of={of} bins={bins}"
                    _same_result(got, _restated(img, valid, ix.get("nodata"), zones, 7, of, bins), what)
                    assert got["count"].shape == (7, C if of is None else 1)    # one more than the largest id but 65535
                    # only the tiles under the zones, and all of them
                    assert sorted(t for _, t in st["tiles"]) == codec.window_tiles(ix, y0, x0, h, w), what
                    assert {l for l, _ in st["tiles"]} == {level}
                    if bins is not None:
                        assert np.array_equal(got["bins"], np.array(bins)) and got["hist"].sum() == got["count"].sum()
                        med = codec.zonal_percentile(got, 50)
                        assert med.shape == got["count"].shape and (np.isnan(med) == (got["count"] == 0)).all()
                if k == 0:                                                      # n_zones below the ids: the rest is ignored
                    got = r.zonal_stats(zones, y0, x0, level=level, n_zones=3)
                    _same_result(got, _restated(img, valid, ix.get("nodata"), zones, 3, None), f"{name}: n_zones=3")
        # the exact median of a uint8 band from bins (0, 255)
        if name == "u8":
            zones = _zones_for(H0, W0, 4, 9)
            got = r.zonal_stats(zones, bins=[(0, 255)] * 3)
            img = _np(plain.read(0, 0, H0, W0))
            for z in range(4):
                v = np.sort(img[:, :, 1][zones == z])
                assert codec.zonal_percentile(got, 50)[z, 1] == v[(v.size + 1) // 2 - 1]
        before = r.stats["decoded"]
        for kw, word in ((dict(zones=np.zeros((4, 4), np.int32)), "uint16"), (dict(y0=r.levels[0][0] - 3), "leave"),
                         (dict(of=("nd", C, 0)), "bands"), (dict(n_zones=0), "n_zones"), (dict(bins=[(0, 1)]), "bins"),
                         (dict(level=7), "level")):
            args = dict(zones=np.zeros((4, 4), np.uint16))
            args.update(kw)
            if word == "bins" and C == 1:
                continue
            with pytest.raises(ValueError, match=word):
                r.zonal_stats(**args)
        assert r.stats["decoded"] == before


# ---- the stack ------------------------------------------------------------------------------------------------------
def test_a_stacks_zonal_stats_are_the_restatement_of_its_composite():
    with _reader("u16") as a, _reader("u16_valid") as b, _extra_reader("u16", 22) as c:
        stack = codec.SceneStack([b, a, c], [(0, 0), (40, 60), (100, 0)])
        for level, (y0, x0, h, w) in ((0, (10, 150, 200, 110)), (2, (0, 0, 63, 65))):      # with pixels under no scene
            zones = _zones_for(h, w, 5, level)
            for reduce in ("median", ("max", ("nd", 3, 0))):
                img, valid = stack.read(y0, x0, h, w, level=level, reduce=reduce, fill=77, with_valid=True)
                img, valid = _np(img), _np(valid).astype(np.uint8)
                assert not valid.all() and valid.any()
                for of, bins in ((None, None), (("nd", 3, 0), [(-10000, 10000)])):
                    got = stack.zonal_stats(zones, y0, x0, level=level, reduce=reduce, of=of, bins=bins, fill=77)
                    _same_result(got, _restated(img, valid, None, zones, 6, of, bins), f"stack level {level} {reduce} of={of}")
                    assert got["count"].sum() > 0
        for kw, word in ((dict(zones=np.zeros((4, 4), np.uint8)), "uint16"), (dict(y0=249), "outside"), (dict(level=3), "levels 0 .. 2"),
                         (dict(reduce="mode"), "reduce"), (dict(fill=65536), "fill"), (dict(n_zones=65536), "n_zones")):
            args = dict(zones=np.zeros((4, 4), np.uint16))
            args.update(kw)
            with pytest.raises(ValueError, match=word):
                stack.zonal_stats(**args)


# ---- the tool -------------------------------------------------------------------------------------------------------
def test_the_tool_writes_the_readers_table(tmp_path):
    sd = (_model(4), _CACHE[("model", 4)][1])[1]
    torch.save({"model": {k: torch.from_numpy(v) for k, v in sd.items()}}, tmp_path / "ckpt.pt")
    (tmp_path / "a.dsic").write_bytes(_stream_of("u16_valid"))
    zones = _zones_for(40, 60, 5, 3)
    np.save(tmp_path / "zones.npy", zones)
    tool = os.path.join(ROOT, "tools", "dsic_image.py")
    base = [sys.executable, tool, "zonal", str(tmp_path / "a.dsic"), "--weights", str(tmp_path / "ckpt.pt"), "--batch", str(BATCH),
            "--zones", str(tmp_path / "zones.npy"), "--at", "20,30", "--level", "1"]
    with _reader("u16_valid") as r:
        for extra, of, bins, names in ((["--index", "nd:3,0", "--bins=-2000,9000"], ("nd", 3, 0), [(-2000, 9000)], ["nd:3;0"]),
                                       ([], None, None, ["0", "1", "2", "3"])):
            path = tmp_path / f"t{len(extra)}.csv"
            p = subprocess.run(base + extra + ["--out", str(path)], cwd=ROOT, capture_output=True, text=True, timeout=600)
            assert p.returncode == 0, p.stdout + p.stderr
            want = r.zonal_stats(zones, 20, 30, level=1, of=of, bins=bins)
            rows = list(csv.reader(open(path)))
            assert rows[0] == ["zone", "value", "count", "mean", "std", "min", "max"] + (["median"] if bins else [])
            assert len(rows) == 1 + 6 * len(names)
            med = codec.zonal_percentile(want, 50) if bins else None
            for row, (z, k) in zip(rows[1:], ((z, k) for z in range(6) for k in range(len(names)))):
                assert row[:3] == [str(z), names[k], str(int(want["count"][z, k]))]
                assert [float(row[3]), float(row[4])] == [float(want["mean"][z, k]), float(want["std"][z, k])] or want["count"][z, k] == 0
                assert row[5:7] == [str(int(want["min"][z, k])), str(int(want["max"][z, k]))]
                if bins:
                    assert float(row[7]) == float(med[z, k]) or want["count"][z, k] == 0
            assert "6 zone(s)" in p.stdout and "of level 1" in p.stdout
