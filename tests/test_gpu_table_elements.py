"""The support scan and the device's CDF tables (csrc/entropy.hip: support_kernel, tables_kernel<true>,
gauss_tables_kernel, finish_table_wave) against the oracle, row by row, on the case list of tests/table_cases.py:
sigma from 0 to inf, nu beyond both clamp ends, supports up to Lmax = 1000 and on both sides of every branch
condition, refused supports among valid ones.  The table buffers are pre-filled with a sentinel that no table can
hold (table_cases.sentinel), so a write outside [:L] of a valid row or anywhere in a refused row shows.
test_table_cases_cpu.py holds the same oracle tables to the host export and to SciPy, and the list to its coverage."""
import functools

import numpy as np
import pytest
import torch

import table_cases as T
from oracle import entropy_ref as E

pytestmark = pytest.mark.gpu


def _lib():
    from dsic_amd import lib
    return lib.load()


def _meta(supports, half):
    """int32 [B, 4] on the device: the supports in the half (0: y, 2: z) that the call reads, (0, 0) in the other."""
    m = np.zeros((len(supports), 4), dtype=np.int64)
    m[:, half:half + 2] = supports
    return torch.from_numpy(m.astype(np.int32)).cuda()


def _prefilled(B, rows, Lmax):
    s = np.broadcast_to(T.sentinel(Lmax), (B, rows, Lmax)).copy()
    return torch.from_numpy(s.view(np.int16)).cuda()


def _student(meta, sigma, nu, Lmax):
    """sigma, nu float32 [B, rows] -> (tables uint16 [B, rows, Lmax], err)."""
    from dsic_amd import lib
    from dsic_amd.ops import _p, _stream
    B, rows = sigma.shape
    sg, nv = torch.from_numpy(np.ascontiguousarray(sigma)).cuda(), torch.from_numpy(np.ascontiguousarray(nu)).cuda()
    tab = _prefilled(B, rows, Lmax)
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    lib.check(_lib().dsic_cdf_tables_student(_p(sg), _p(nv), _p(meta), _p(tab), B, rows, Lmax, _p(err), _stream()),
              "student")
    return tab.cpu().numpy().view(np.uint16), int(err.item())


def _gauss(meta, sigma, Lmax):
    """sigma float32 [N] -> (tables uint16 [B, N, Lmax], err)."""
    from dsic_amd import lib
    from dsic_amd.ops import _p, _stream
    B, N = meta.shape[0], sigma.size
    sg = torch.from_numpy(np.ascontiguousarray(sigma)).cuda()
    tab = _prefilled(B, N, Lmax)
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    lib.check(_lib().dsic_cdf_tables_gauss(_p(sg), _p(meta), _p(tab), B, N, Lmax, _p(err), _stream()), "gauss")
    return tab.cpu().numpy().view(np.uint16), int(err.item())


def _held(tab, supports, Lmax, want_of):
    """Every valid image's rows equal want_of(b, smin, L) [rows, L] on [:L] and the sentinel behind; every refused
    image's rows are the sentinel."""
    sent = T.sentinel(Lmax)
    for b, (smin, L) in enumerate(supports):
        if not T.valid((smin, L), Lmax):
            assert np.array_equal(tab[b], np.broadcast_to(sent, tab[b].shape)), ("refused row written", b, smin, L)
            continue
        want = want_of(b, smin, L)
        diff = np.argwhere(tab[b, :, :L] != want)
        assert diff.size == 0, (b, smin, L, len(diff), "first (row, k):", diff[0], tab[b, diff[0][0], diff[0][1]],
                                want[diff[0][0], diff[0][1]])
        assert np.array_equal(tab[b, :, L:], np.broadcast_to(sent[L:], (tab.shape[1], Lmax - L))), \
            ("written behind L", b, smin, L)


def _err_held(err, supports, Lmax):
    if all(T.valid(s, Lmax) for s in supports):
        assert err == 0
    else:
        assert err & 1 and not err & ~1


@pytest.mark.parametrize("with_refused", [False, True])
@pytest.mark.parametrize("Lmax", T.LMAXES)
def test_student_tables_equal_oracle(Lmax, with_refused):
    supports = T.with_refused(Lmax) if with_refused else T.SUPPORTS[Lmax]
    B = len(supports)
    tab, err = _student(_meta(supports, 0), np.tile(T.ROW_SIGMA, (B, 1)), np.tile(T.ROW_NU, (B, 1)), Lmax)
    _err_held(err, supports, Lmax)
    _held(tab, supports, Lmax, lambda b, smin, L: T.oracle_student(smin, L)[0])


@pytest.mark.parametrize("with_refused", [False, True])
@pytest.mark.parametrize("Lmax", T.LMAXES)
def test_gauss_tables_equal_oracle(Lmax, with_refused):
    supports = T.with_refused(Lmax) if with_refused else T.SUPPORTS[Lmax]
    tab, err = _gauss(_meta(supports, 2), T.SIGMAS, Lmax)
    _err_held(err, supports, Lmax)
    _held(tab, supports, Lmax, lambda b, smin, L: T.oracle_gauss(smin, L)[0])


@pytest.mark.parametrize("Lmax", T.LMAXES)
@pytest.mark.parametrize("B", T.GAUSS_BATCHES)
def test_gauss_group_layouts_equal_oracle(B, Lmax):
    """1, 16, 17 and 33 images: a lone image, supports 9000 apart, the refused supports inside a group that shares
    its row, a union of exactly 4 Lmax - 1 (shared row) beside one of exactly 4 Lmax (own boundaries), and a last
    group of one image."""
    supports = T.gauss_layout(B, Lmax)
    tab, err = _gauss(_meta(supports, 2), T.SIGMAS, Lmax)
    _err_held(err, supports, Lmax)
    _held(tab, supports, Lmax, lambda b, smin, L: T.oracle_gauss(smin, L)[0])


def test_student_per_element_shape():
    """B = 3 with 7 rows per image, every row its own (sigma, nu): 21 tables, the last workgroup has one live wave."""
    supports, Lmax = T.PER_ELEMENT_SUPPORTS, T.PER_ELEMENT_LMAX
    rows = T.PER_ELEMENT_ROWS.reshape(3, 7)
    tab, err = _student(_meta(supports, 0), T.ROW_SIGMA[rows], T.ROW_NU[rows], Lmax)
    assert err == 0
    _held(tab, supports, Lmax, lambda b, smin, L: T.oracle_student(smin, L)[0][rows[b]])


def _scan(y, z, tail):
    from dsic_amd import lib
    from dsic_amd.ops import _p, _stream
    B = len(y)
    ty, tz = torch.from_numpy(np.ascontiguousarray(y)).cuda(), torch.from_numpy(np.ascontiguousarray(z)).cuda()
    meta = torch.full((B, 4), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    lib.check(_lib().dsic_latent_support(_p(ty), _p(tz), _p(meta), B, y.shape[1], z.shape[1], tail, _stream()),
              "latent_support")
    return meta


def test_support_scan_equals_restatement():
    """Element counts from 1 to 1000 on either half, the extrema at the first and last index and at the wave and block
    seams, non-integer, one-sided, constant and signed-zero data, tails 0, 10 and 1000, the largest magnitudes the
    guard admits."""
    wrong = []
    for name, y, z, tail in T.scan_cases():
        got = _scan(y, z, tail).cpu().numpy().astype(np.int64)
        want = T.meta_restated(y, z, tail)
        if not np.array_equal(got, want):
            b = int(np.argwhere((got != want).any(axis=1))[0][0])
            wrong.append((name, b, got[b].tolist(), want[b].tolist()))
    assert not wrong, (len(wrong), wrong[:8])


@functools.lru_cache(maxsize=None)
def _scan_oracle_student(smin, L):
    return E.tables_student(T.ROW_SIGMA[T.BAD_SCAN_ROWS], T.ROW_NU[T.BAD_SCAN_ROWS], smin, L)


def test_support_scan_refuses_a_bad_half_and_the_tables_refuse_its_rows():
    """+-1e9, NaN and +-inf at the first or the last index, in y only, in z only and in one image of three: the bad
    half reads (0, 0), the other half and the other images are right; both table calls raise error bit 1 on that
    meta, leave the refused rows untouched and build the oracle's tables for the rest."""
    Lmax = T.BAD_SCAN_LMAX
    sg = np.tile(T.ROW_SIGMA[T.BAD_SCAN_ROWS], (3, 1))
    nu = np.tile(T.ROW_NU[T.BAD_SCAN_ROWS], (3, 1))
    for name, y, z, tail in T.bad_scan_cases():
        meta = _scan(y, z, tail)
        got = meta.cpu().numpy().astype(np.int64)
        want = T.meta_restated(y, z, tail)
        assert np.array_equal(got, want), (name, got.tolist(), want.tolist())
        ysup, zsup = [tuple(r) for r in want[:, 0:2].tolist()], [tuple(r) for r in want[:, 2:4].tolist()]
        ty, erry = _student(meta, sg, nu, Lmax)
        tz, errz = _gauss(meta, T.SIGMAS, Lmax)
        _err_held(erry, ysup, Lmax)
        _err_held(errz, zsup, Lmax)
        assert (erry | errz) & 1, name
        _held(ty, ysup, Lmax, lambda b, smin, L: _scan_oracle_student(smin, L))
        _held(tz, zsup, Lmax, lambda b, smin, L: T.oracle_gauss(smin, L)[0])
