"""The split range encoder (pack -> chain -> place, dsic_range_encode_ws) writes the same bytes, lengths and error
bits as the single-kernel encoder (dsic_range_encode) for every input, and where no error bit is set both write the
strings of the bit-serial CPU oracle on the run's tables (the two encoders share their interval arithmetic, so their
equality alone does not check it)."""
import numpy as np
import pytest
import torch

import coder_oracle as O
from dsic_amd import synthetic as S

pytestmark = pytest.mark.gpu


def _both(y, z, sy, ny, sz, tail=10, Lmax=192):
    from dsic_amd import entropy
    t = [torch.as_tensor(a).cuda() for a in (y, z, sy, ny, sz)]
    new = entropy.compress_latents(*t, tail=tail, Lmax=Lmax, split=True)
    old = entropy.compress_latents(*t, tail=tail, Lmax=Lmax, split=False)
    return new, old


def _same(new, old):
    assert torch.equal(new["lengths"], old["lengths"])
    assert int(new["err"].item()) == int(old["err"].item())
    assert torch.equal(new["bytes"], old["bytes"])


def _oracle(new, old, y, z):
    """both encoders' strings are the oracle's (runs without an error bit)"""
    assert int(new["err"].item()) == 0 and int(old["err"].item()) == 0
    want = O.oracle_strings(y, z, new["meta"], new["tab_y"], new["tab_z"])
    O.assert_oracle(new, want, new["cap_z"])
    O.assert_oracle(old, want, old["cap_z"])


def _stress(case, rng):
    B, M, N, Hy, Wy, Hz, Wz = 3, 16, 8, 8, 12, 2, 3
    if case == "single":
        B, M, N, Hy, Wy, Hz, Wz = 2, 1, 1, 1, 1, 1, 1
    if case == "random":
        y = np.rint(rng.standard_t(2.5, size=(B, M, Hy, Wy)) * 3).clip(-60, 60)
        sy = rng.uniform(0.5, 6.0, (B, M)); ny = rng.uniform(2.0, 50.0, (B, M))
    elif case == "peaky":
        y = np.zeros((B, M, Hy, Wy)); y[:, :, ::3, ::5] = rng.integers(-9, 10, size=y[:, :, ::3, ::5].shape)
        sy = np.full((B, M), 1e-3); ny = np.full((B, M), 2.0)
    elif case == "runs":
        y = np.where(rng.random((B, M, Hy, Wy)) < 0.5, 0.0, -1.0)
        sy = np.full((B, M), 40.0); ny = np.full((B, M), 100.0)
    else:
        y = np.array([3.0, -2.0]).reshape(B, 1, 1, 1)
        sy = np.full((B, M), 1.0); ny = np.full((B, M), 5.0)
    z = np.rint(rng.normal(size=(B, N, Hz, Wz)) * 4)
    sz = rng.uniform(0.5, 5.0, N)
    return [a.astype(np.float32) for a in (y, z, sy, ny, sz)]


@pytest.mark.parametrize("case", ["random", "peaky", "runs", "single"])
def test_stress_cases(case):
    args = _stress(case, np.random.default_rng(11))
    new, old = _both(*args)
    _same(new, old)
    _oracle(new, old, args[0], args[1])


def test_top_symbol_c_high_65536():
    """tail=0: the largest symbol is the last table entry (c_high = 65536), in full groups of 64 and in the tail."""
    rng = np.random.default_rng(3)
    B, M, N = 2, 8, 4
    y = np.rint(rng.normal(size=(B, M, 9, 15)) * 2).clip(-3, 3)
    y[:, :, ::2, :] = 3.0                       # many top symbols in every group
    z = np.rint(rng.normal(size=(B, N, 3, 3)) * 2).clip(-2, 2)
    z[:, :, 0, :] = 2.0
    sy = rng.uniform(0.5, 3.0, (B, M)); ny = rng.uniform(2.0, 30.0, (B, M)); sz = rng.uniform(0.5, 3.0, N)
    new, old = _both(*[a.astype(np.float32) for a in (y, z, sy, ny, sz)], tail=0)
    assert int(new["err"].item()) == 0
    _same(new, old)
    _oracle(new, old, y, z)


def test_long_pending_runs_across_place_slices():
    """Long strings of near-certain symbols: thousands of symbols emit no bit, so the pending count and the bit
    offsets are carried across many of the place kernel's slices; a two-valued stream adds long E3 runs."""
    rng = np.random.default_rng(5)
    B, M, N, H, W = 2, 48, 4, 64, 64
    y = np.zeros((B, M, H, W))
    y[0, :, ::37, ::41] = rng.integers(-3, 4, size=y[0, :, ::37, ::41].shape)
    y[1] = np.where(rng.random((M, H, W)) < 0.5, 0.0, -1.0)
    sy = np.where(np.arange(B)[:, None] == 0, 1e-3, 40.0) * np.ones((B, M))
    ny = np.where(np.arange(B)[:, None] == 0, 2.0, 100.0) * np.ones((B, M))
    z = np.rint(rng.normal(size=(B, N, 4, 4)) * 3)
    sz = rng.uniform(0.5, 5.0, N)
    new, old = _both(*[a.astype(np.float32) for a in (y, z, sy, ny, sz)])
    assert int(new["err"].item()) == 0
    _same(new, old)
    _oracle(new, old, y, z)


def test_non_finite_latents():
    for bad in (float("nan"), float("inf")):
        y = np.zeros((2, 4, 2, 2), np.float32); y[1, 2, 0, 1] = bad
        z = np.zeros((2, 2, 1, 1), np.float32)
        new, old = _both(y, z, np.ones((2, 4), np.float32), np.full((2, 4), 3.0, np.float32), np.ones(2, np.float32),
                         Lmax=64)
        assert int(new["err"].item()) & 1
        _same(new, old)


def test_symbol_outside_support_and_overflow():
    """A hand-made support that misses symbols (error bit 2) and capacities too small for the strings (bit 4)."""
    from dsic_amd import entropy, lib as _lib
    from dsic_amd.ops import _p, _stream
    L = _lib.load()
    rng = np.random.default_rng(9)
    B, M, N, HWy, HWz, Lmax = 2, 4, 2, 200, 4, 64
    y = torch.from_numpy(np.rint(rng.normal(size=(B, M, HWy)) * 6).astype(np.float32)).cuda()
    z = torch.from_numpy(np.rint(rng.normal(size=(B, N, HWz)) * 2).astype(np.float32)).cuda()
    meta = torch.tensor([[-5, 11, -12, 25], [-30, 61, -12, 25]], dtype=torch.int32, device="cuda")
    sy = torch.from_numpy(rng.uniform(1.0, 8.0, (B, M)).astype(np.float32)).cuda()
    ny = torch.full((B, M), 4.0, device="cuda")
    tab_y = torch.zeros((B, M, Lmax), dtype=torch.int16, device="cuda")
    tab_z = torch.zeros((B, N, Lmax), dtype=torch.int16, device="cuda")
    err0 = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(L.dsic_cdf_tables_gauss(_p(torch.ones(N, device="cuda")), _p(meta), _p(tab_z), B, N, Lmax, _p(err0),
                                       _stream()), "tables")
    _lib.check(L.dsic_cdf_tables_student(_p(sy), _p(ny), _p(meta), _p(tab_y), B, M, Lmax, _p(err0), _stream()),
               "tables")
    for cap_y, cap_z in ((entropy._cap(M * HWy), entropy._cap(N * HWz)), (32, 8)):
        res = []
        for split in (True, False):
            out = torch.zeros((B, (cap_z + cap_y) // 4), dtype=torch.int32, device="cuda").view(torch.uint8)
            lengths = torch.zeros((B, 2), dtype=torch.int32, device="cuda")
            err = torch.zeros(1, dtype=torch.int32, device="cuda")
            args = (_p(y), _p(z), _p(meta), _p(tab_y), _p(tab_z), Lmax, B, M, HWy, N, HWz, _p(out), cap_y, cap_z,
                    _p(lengths), _p(err))
            if split:
                nb = L.dsic_range_encode_workspace_size(B, M, HWy, N, HWz)
                ws = torch.empty(((nb + 3) // 4,), dtype=torch.int32, device="cuda")
                _lib.check(L.dsic_range_encode_ws(*args, 0, _p(ws), ws.numel() * 4, _stream()), "ws")
            else:
                _lib.check(L.dsic_range_encode(*args, 1, 0, _stream()), "single")
            res.append({"bytes": out, "lengths": lengths, "err": err})
        assert int(res[0]["err"].item()) & 2
        if cap_y == 32:
            assert int(res[0]["err"].item()) & 4
        _same(*res)
        # the symbols outside the support coded as symbol 0: the oracle's strings, cut where the capacity ends
        want = O.oracle_strings(y, z, meta, tab_y, tab_z)
        for r in res:
            O.assert_oracle_prefix(r, want, cap_z, cap_y)


@pytest.fixture(scope="module")
def bench_latents():
    from dsic_amd.model import CompressionModel
    m = CompressionModel(N=128, M=192, spatial_params=False, min_nu=2, max_nu=100.0)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in S.make_state_dict(seed=1).items()}, strict=True)
    m = m.cuda().eval()
    x = torch.from_numpy(S.make_patches(0, 64, 256, 256)).cuda()
    with torch.no_grad():
        return m, m(x, quant_mode="round")


def test_bench_batch_through_model(bench_latents):
    from dsic_amd import entropy
    m, out = bench_latents
    args = (out["y_tilde"], out["z_tilde"], entropy._per_channel(out["sigma"]), entropy._per_channel(out["nu"]),
            entropy.sigma_z_of(m), 10, entropy.DEFAULT_LMAX)
    new = entropy.compress_latents(*args, split=True)
    old = entropy.compress_latents(*args, split=False)
    assert int(new["err"].item()) == 0
    _same(new, old)
    _oracle(new, old, out["y_tilde"], out["z_tilde"])


def test_spatial_params():
    from dsic_amd import entropy
    from dsic_amd.model import CompressionModel
    sd = S.make_state_dict(seed=4, spatial_params=True)
    m = CompressionModel(N=128, M=192, spatial_params=True, min_nu=2, max_nu=100.0)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    m = m.cuda().eval()
    x = torch.from_numpy(S.make_patches(500, 2, 128, 64)).cuda()
    with torch.no_grad():
        out = m(x, quant_mode="round")
    Lmax = min(1000, entropy._tight_lmax(entropy.latent_support(out["y_tilde"], out["z_tilde"], 10)))
    args = (out["y_tilde"], out["z_tilde"], entropy._per_channel(out["sigma"]), entropy._per_channel(out["nu"]),
            entropy.sigma_z_of(m), 10, Lmax)
    new = entropy.compress_latents(*args, split=True)
    old = entropy.compress_latents(*args, split=False)
    assert int(new["err"].item()) == 0
    _same(new, old)
    _oracle(new, old, out["y_tilde"], out["z_tilde"])
