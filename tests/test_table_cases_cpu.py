"""CPU only: the case list of tests/table_cases.py.  The host export equals the oracle on every row and support, the
oracle's Student-t tables equal the same float32 flow fed with SciPy's stdtr, every table is usable by the coder, and
the list itself sits on both sides of every branch condition that the device code takes (restated in table_cases.py),
so that a later edit cannot hollow it out.  test_gpu_table_elements.py holds the device to the same oracle tables."""
import ctypes

import numpy as np
import pytest
from scipy import special

import table_cases as T
from oracle import entropy_ref as E
from test_oracle_entropy import _bounds, _np_table

ALL_SUPPORTS = [(Lmax, s) for Lmax in T.LMAXES for s in T.SUPPORTS[Lmax]]


@pytest.fixture(scope="module")
def host():
    from dsic_amd import lib
    return lib.load()


def _host_table(host, student, sigma, nu, smin, L):
    out = np.zeros(L, dtype=np.uint16)
    raw = np.zeros(L + 1, dtype=np.uint16)
    assert host.dsic_host_cdf_table(student, float(sigma), float(nu), smin, L, out.ctypes.data_as(ctypes.c_void_p),
                                    raw.ctypes.data_as(ctypes.c_void_p)) == 0
    return out, raw


def test_the_list_is_what_it_says():
    assert T.ROW_SIGMA.size == T.ROW_NU.size == 91 and T.SIGMAS.size == 13
    assert len({(float(s), float(n)) for s, n in zip(T.ROW_SIGMA, T.ROW_NU)}) == 91
    assert T.SIGMAS[0] == 0 and np.isinf(T.SIGMAS[-1]) and 0 < T.SIGMAS[1] < np.finfo(np.float32).tiny
    assert T.NUS[1] == 2 and T.NUS[2] > 2 and T.NUS[2] - T.NUS[1] == np.float32(2.0 ** -22)
    for Lmax in T.LMAXES:
        assert all(T.valid(s, Lmax) for s in T.SUPPORTS[Lmax])
        assert not any(T.valid(s, Lmax) for s in T.refused(Lmax))
        mixed = T.with_refused(Lmax)
        assert [s for s in mixed if T.valid(s, Lmax)] == T.SUPPORTS[Lmax]
        assert [s for s in mixed if not T.valid(s, Lmax)] == T.refused(Lmax)
        assert T.valid(mixed[0], Lmax) and not T.valid(mixed[-1], Lmax)
    assert sorted(set(T.PER_ELEMENT_ROWS)) == sorted(T.PER_ELEMENT_ROWS) and len(T.PER_ELEMENT_ROWS) == 21
    assert all(T.valid(s, T.PER_ELEMENT_LMAX) for s in T.PER_ELEMENT_SUPPORTS)


@pytest.mark.parametrize("Lmax", T.LMAXES)
def test_host_export_equals_oracle(host, Lmax):
    for smin, L in T.SUPPORTS[Lmax]:
        want, want_raw = T.oracle_student(smin, L)
        for r, (sg, nu) in enumerate(zip(T.ROW_SIGMA, T.ROW_NU)):
            out, raw = _host_table(host, 1, sg, nu, smin, L)
            assert np.array_equal(out, want[r]) and np.array_equal(raw, want_raw[r]), (smin, L, sg, nu)
        want, want_raw = T.oracle_gauss(smin, L)
        for c, sg in enumerate(T.SIGMAS):
            out, raw = _host_table(host, 0, sg, 0.0, smin, L)
            assert np.array_equal(out, want[c]) and np.array_equal(raw, want_raw[c]), (smin, L, sg)


def _scipy_F(smin, L, sg, nu):
    """Boundary CDFs in float32 from SciPy's stdtr on float64 b / sigma, as the oracle divides."""
    b = _bounds(smin, L).astype(np.float64)
    with np.errstate(divide="ignore"):
        return special.stdtr(float(nu), b / float(sg)).astype(np.float32)


def test_student_tables_vs_scipy_on_the_list():
    """The raw tables differ by at most 1 count, on at most 5 entries over the whole list (the cap and its reasoning
    are test_student_tables_vs_scipy_over_the_clamp_box's: a 1e-14 float64 disagreement crosses a float32 rounding
    boundary about once in 1e6 values).  Measured: 0 of 509 201 entries."""
    rows = [r for r in range(91) if 0 < T.ROW_SIGMA[r] < np.inf]
    assert len(rows) == 77
    total = bad = 0
    for _, (smin, L) in ALL_SUPPORTS:
        _, raw = T.oracle_student(smin, L)
        for r in rows:
            want = _np_table(_scipy_F(smin, L, T.ROW_SIGMA[r], T.ROW_NU[r]), L, raw=True)
            d = np.abs(want.astype(np.int64) - raw[r].astype(np.int64))
            assert d.max() <= 1, (smin, L, T.ROW_SIGMA[r], T.ROW_NU[r])
            bad += np.count_nonzero(d)
            total += d.size
    print(f"scipy flow: {bad} of {total} raw entries differ")
    assert bad <= 5, (bad, total)


def test_every_table_is_usable_by_the_coder():
    for _, (smin, L) in ALL_SUPPORTS:
        for tab in (T.oracle_student(smin, L)[0], T.oracle_gauss(smin, L)[0]):
            t = tab.astype(np.int64)
            assert np.all(t[:, 0] == 0) and np.all(t[:, -1] <= 65535)
            assert np.all(np.diff(t, axis=1) >= 1), (smin, L)       # non-empty intervals
            assert np.all(t >= np.arange(L)) and np.all(t != T.sentinel(L).astype(np.int64))
    for B in T.GAUSS_BATCHES:
        for Lmax in T.LMAXES:
            for s in T.gauss_layout(B, Lmax):
                if T.valid(s, Lmax):
                    t = T.oracle_gauss(*s)[0].astype(np.int64)
                    assert np.all(t[:, 0] == 0) and np.all(t[:, -1] <= 65535) and np.all(np.diff(t, axis=1) >= 1)


def test_the_list_covers_both_sides_of_the_student_branches():
    sup = {s for _, s in ALL_SUPPORTS}
    # smin <= 0 && smin + L >= 1, one step to either side of each condition with the other one true
    assert any(smin <= 0 and smin + L == 1 for smin, L in sup)
    assert any(smin <= 0 and smin + L == 0 for smin, L in sup)
    assert any(smin == 0 and smin + L >= 1 for smin, L in sup)
    assert any(smin == 1 and smin + L >= 1 for smin, L in sup)
    routes = {T.student_route(*s) for s in sup}
    assert routes == {"mirror", "each"}
    # whi from either operand, lopsided by more than a wave pass either way, and the tie
    mirror = [s for s in sup if T.student_route(*s) == "mirror"]
    assert any(T.whi_operand(*s) == "right" and (s[0] + s[1]) - (1 - s[0]) > 64 for s in mirror)
    assert any(T.whi_operand(*s) == "left" and (1 - s[0]) - (s[0] + s[1]) > 64 for s in mirror)
    assert any(s[0] + s[1] == 1 - s[0] for s in mirror)
    # a one-sided support on either side of 0
    assert any(smin >= 1 for smin, L in sup) and any(smin + L <= 0 for smin, L in sup)
    # float(u) inexact: beyond 2^24
    assert any(abs(smin) > 2 ** 24 for smin, L in sup) and any(smin < 2 ** 24 < smin + L + 8 for smin, L in sup)


def test_the_list_covers_the_widths():
    widths = {L for _, (smin, L) in ALL_SUPPORTS}
    assert {1, 63, 64, 255, 256, 257, 999, 1000} <= widths
    for Lmax in T.LMAXES:
        assert any(L == Lmax for smin, L in T.SUPPORTS[Lmax])
        assert {L for smin, L in T.refused(Lmax)} >= {Lmax + 1, 0} and any(L < 0 for smin, L in T.refused(Lmax))
    assert {T.sum_levels(L) for L in widths} == {1, 2, 3}
    assert {T.finish_passes(L) for L in widths} >= {1, 4, 5, 11, 16}
    assert T.sum_levels(255) == 2 and T.sum_levels(256) == 3 and T.finish_passes(1000) == 16


def test_the_list_covers_the_pmf_clamp():
    """At least one (row, support) with more than 90 % of the PMF entries on the 1e-12 clamp, at least one with
    none; counted on the SciPy flow's float32 boundary values."""
    frac = []
    for smin, L in ((-500, 1000), (-40, 41)):
        for r in range(91):
            F = _scipy_F(smin, L, T.ROW_SIGMA[r], T.ROW_NU[r])
            frac.append(np.count_nonzero(F[1:] - F[:-1] < np.float32(1e-12)) / L)
    assert max(frac) > 0.9 and min(frac) == 0.0, (max(frac), min(frac))


def test_the_gauss_layouts_cover_the_group_conditions():
    assert T.GAUSS_BATCHES == [1, 16, 17, 33]
    for Lmax in T.LMAXES:
        shared, own = T.group_shared_edge(Lmax), T.group_own_edge(Lmax)
        assert T.gauss_width(shared, Lmax) == 4 * Lmax - 1 and T.gauss_shares_row(shared, Lmax)
        assert T.gauss_width(own, Lmax) == 4 * Lmax and not T.gauss_shares_row(own, Lmax)
        assert all(T.valid(s, Lmax) for s in shared + own)
        bad = T.group_refused(Lmax)
        assert [s for s in bad if not T.valid(s, Lmax)] == T.refused(Lmax) and T.gauss_shares_row(bad, Lmax)
        assert sum(T.valid(s, Lmax) for s in bad) == 12
        far = T.group_far_apart(Lmax)
        assert all(abs(b[0] - a[0]) >= 8990 for a, b in zip(far, far[1:])) and not T.gauss_shares_row(far, Lmax)
        for B in T.GAUSS_BATCHES:
            lay = T.gauss_layout(B, Lmax)
            assert len(lay) == B and all(len(g) <= T.ZT_IMGS for g in T.groups_of(lay))
        lay = T.gauss_layout(33, Lmax)
        assert lay[:16] == shared and lay[16:32] == own
        assert T.gauss_layout(17, Lmax)[:16] == bad and T.gauss_layout(16, Lmax) == far


def test_support_restatement_equals_the_oracle_on_finite_cases():
    names = set()
    for name, y, z, tail in T.scan_cases():
        names.add(name)
        meta = T.meta_restated(y, z, tail)
        for b in range(len(y)):
            for half, v in ((0, y[b]), (2, z[b])):
                lo, hi = E.support(v, tail)
                assert (meta[b, half], meta[b, half + 1]) == (lo, hi - lo + 1), (name, b)
        assert np.all(np.abs(meta) < 2 ** 31)
    assert len(names) == len(T.scan_cases())
    assert T.support_restated(np.array([-3.5, 7.25], np.float32), 0) == (-4, 13)
    assert T.support_restated(np.array([-0.0], np.float32), 0) == (0, 1)
    assert T.support_restated(np.array([T.GUARD_MAX], np.float32), 1000) == (999998936, 2001)
    assert float(T.GUARD_MAX) < 1e9 <= float(np.nextafter(T.GUARD_MAX, np.float32(np.inf)))


def test_support_restatement_refuses_what_the_guard_refuses():
    for _, v in T.SCAN_BAD:
        for n in (1, 5):
            for pos in (0, -1):
                a = np.ones(n, np.float32)
                a[pos] = v
                assert T.support_restated(a, 10) == (0, 0)
    for name, y, z, tail, in T.bad_scan_cases():
        meta = T.meta_restated(y, z, tail)
        where = name.rsplit("_", 1)[1]
        ybad, zbad = (meta[:, 1] == 0), (meta[:, 3] == 0)
        assert list(ybad) == {"y": [1, 1, 1], "z": [0, 0, 0], "image": [0, 1, 0]}[where], name
        assert list(zbad) == {"y": [0, 0, 0], "z": [1, 1, 1], "image": [0, 1, 0]}[where], name
        assert np.all(meta[ybad, 0] == 0) and np.all(meta[zbad, 2] == 0)
        ok = np.concatenate([meta[~ybad, 1], meta[~zbad, 3]])
        assert np.all((ok >= 1) & (ok <= T.BAD_SCAN_LMAX))


def test_the_scan_cases_cover_sizes_positions_and_values():
    cases = T.scan_cases()
    assert {(y.shape[1], z.shape[1]) for n, y, z, t in cases} >= {(a, b) for a in T.SCAN_SIZES for b in T.SCAN_SIZES}
    assert {t for n, y, z, t in cases} == {0, 10, 1000}
    seen_min, seen_max = set(), set()
    for name, y, z, t in cases:
        if name.startswith("extrema"):
            for a in (y, z):
                seen_min |= set(np.argmin(a, axis=1)); seen_max |= set(np.argmax(a, axis=1))
                assert np.all(a.min(axis=1) == -3.5) and np.all(a.max(axis=1) == 7.25)
    want = {0, 63, 64, 255, 256, 999}
    assert seen_min >= want and seen_max >= want
    flat = [a[b] for n, y, z, t in cases for a in (y, z) for b in range(len(a))]
    assert any(v.max() < 0 for v in flat) and any(v.min() > 0 for v in flat)
    assert any(v.min() == v.max() and v.size > 1 for v in flat)
    assert any(np.all(v == 0) and np.all(np.signbit(v)) for v in flat)
    assert any(v.max() == T.GUARD_MAX for v in flat) and any(v.min() == -T.GUARD_MAX for v in flat)
    assert any(v.min() != np.floor(v.min()) for v in flat) and any(v.max() != np.ceil(v.max()) for v in flat)
