"""The place step of the split encoder in slices (summarize -> emit), and the CDF tables that share evaluations:
bytes, lengths and error bits equal to the single-kernel encoder and its strings to the bit-serial CPU oracle's on the
run's tables, tables equal to the oracle's."""
import numpy as np
import pytest
import torch

import coder_oracle as O
from oracle import entropy_ref as E

pytestmark = pytest.mark.gpu


def _encode(y, z, sy, ny, sz, split, tail=10, Lmax=192):
    from dsic_amd import entropy
    t = [torch.as_tensor(a).cuda() for a in (y, z, sy, ny, sz)]
    return entropy.compress_latents(*t, tail=tail, Lmax=Lmax, split=split)


def _same(new, old):
    assert torch.equal(new["lengths"], old["lengths"])
    assert int(new["err"].item()) == int(old["err"].item())
    assert torch.equal(new["bytes"], old["bytes"])


def _latents(rng, B, M, Hy, Wy, N, Hz, Wz, scale=3.0):
    y = np.rint(rng.standard_t(3.0, size=(B, M, Hy, Wy)) * scale).clip(-40, 40)
    z = np.rint(rng.normal(size=(B, N, Hz, Wz)) * 3)
    sy = rng.uniform(0.5, 6.0, (B, M)); ny = rng.uniform(2.0, 50.0, (B, M)); sz = rng.uniform(0.5, 5.0, N)
    return [a.astype(np.float32) for a in (y, z, sy, ny, sz)]


@pytest.mark.parametrize("B,M,Hy,Wy,N,Hz,Wz", [
    (1, 7, 13, 11, 3, 1, 5),        # y: 1 001 symbols (two slices, the last partial); z: 15, less than one slice
    (64, 7, 13, 11, 3, 1, 5),
    (64, 4, 16, 8, 2, 16, 16),      # y exactly one slice of 512, z exactly one
    (1, 192, 32, 32, 128, 8, 8),    # y: 196 608 symbols, 256 slices of 768
])
def test_slice_geometry(B, M, Hy, Wy, N, Hz, Wz):
    args = _latents(np.random.default_rng(B * 1000 + M), B, M, Hy, Wy, N, Hz, Wz)
    new, old = _encode(*args, split=True), _encode(*args, split=False)
    assert int(new["err"].item()) == 0
    _same(new, old)
    O.assert_oracle_of(new, args[0], args[1])
    O.assert_oracle_of(old, args[0], args[1])


def test_e3_runs_across_many_slices():
    """A two-valued stream of near-even probability: long E3 runs and long stretches without a final bit, carried
    across dozens of slice boundaries; one image of very peaked tables where most symbols emit nothing."""
    rng = np.random.default_rng(21)
    B, M, N, H, W = 3, 64, 4, 32, 32
    y = np.where(rng.random((B, M, H, W)) < 0.5, 0.0, -1.0)
    y[2] = 0.0
    y[2, :, ::29, ::31] = 1.0
    sy = np.full((B, M), 40.0); sy[2] = 1e-3
    ny = np.full((B, M), 100.0); ny[2] = 2.0
    z = np.rint(rng.normal(size=(B, N, 4, 4)) * 3)
    sz = rng.uniform(0.5, 5.0, N)
    args = [a.astype(np.float32) for a in (y, z, sy, ny, sz)]
    new, old = _encode(*args, split=True), _encode(*args, split=False)
    assert int(new["err"].item()) == 0
    _same(new, old)
    O.assert_oracle_of(new, args[0], args[1])
    O.assert_oracle_of(old, args[0], args[1])


def _ws_call(L, t, meta, tab_y, tab_z, Lmax, shape, ws, stream):
    from dsic_amd import entropy, lib as _lib
    from dsic_amd.ops import _p
    B, M, HWy, N, HWz = shape
    cap_y, cap_z = entropy._cap(M * HWy), entropy._cap(N * HWz)
    out = torch.zeros((B, (cap_z + cap_y) // 4), dtype=torch.int32, device="cuda").view(torch.uint8)
    lengths = torch.zeros((B, 2), dtype=torch.int32, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(L.dsic_range_encode_ws(_p(t[0]), _p(t[1]), _p(meta), _p(tab_y), _p(tab_z), Lmax, B, M, HWy, N, HWz,
                                      _p(out), cap_y, cap_z, _p(lengths), _p(err), 0, _p(ws), ws.numel() * 4,
                                      stream), "range_encode_ws")
    return {"bytes": out, "lengths": lengths, "err": err}


def test_garbage_workspace_and_two_streams():
    """The workspace may hold anything when a call starts (0xFF here, twice in a row), and two calls in flight on two
    streams, each with its own workspace, give the same bytes as the single kernel."""
    from dsic_amd import entropy, lib as _lib
    L = _lib.load()
    B, M, Hy, Wy, N, Hz, Wz, Lmax = 8, 48, 16, 16, 16, 4, 4, 192
    y, z, sy, ny, sz = _latents(np.random.default_rng(33), B, M, Hy, Wy, N, Hz, Wz)
    t = [torch.from_numpy(a).cuda() for a in (y, z)]
    meta = entropy.latent_support(t[0], t[1], 10)
    tab_y, tab_z, err0 = entropy.cdf_tables(torch.from_numpy(sy).cuda(), torch.from_numpy(ny).cuda(),
                                            torch.from_numpy(sz).cuda(), meta, Lmax)
    assert int(err0.item()) == 0
    ref = _encode(y, z, sy, ny, sz, split=False, Lmax=Lmax)
    assert int(ref["err"].item()) == 0
    want = O.oracle_strings(y, z, meta, tab_y, tab_z)
    O.assert_oracle(ref, want, ref["cap_z"])
    shape = (B, M, Hy * Wy, N, Hz * Wz)
    nbytes = L.dsic_range_encode_workspace_size(*shape)
    cur = torch.cuda.current_stream()
    ws = torch.full(((nbytes + 3) // 4,), -1, dtype=torch.int32, device="cuda")
    for _ in range(2):
        got = _ws_call(L, t, meta, tab_y, tab_z, Lmax, shape, ws, cur.cuda_stream)
        _same(got, ref)
        O.assert_oracle(got, want, ref["cap_z"])
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    wss = [torch.full_like(ws, -1) for _ in streams]
    torch.cuda.synchronize()
    res = []
    for st, w in zip(streams, wss):
        res.append(_ws_call(L, t, meta, tab_y, tab_z, Lmax, shape, w, st.cuda_stream))
    torch.cuda.synchronize()
    for r in res:
        _same(r, ref)
        O.assert_oracle(r, want, ref["cap_z"])


def _tables(meta_rows, sigma_z, sigma_y, nu_y, Lmax):
    from dsic_amd import lib as _lib
    from dsic_amd.ops import _p, _stream
    L = _lib.load()
    B = len(meta_rows)
    meta = torch.tensor(meta_rows, dtype=torch.int32, device="cuda")
    sz, sy, ny = (torch.from_numpy(a).cuda() for a in (sigma_z, sigma_y, nu_y))
    N, M = sz.numel(), sy.shape[1]
    tab_z = torch.zeros((B, N, Lmax), dtype=torch.int16, device="cuda")
    tab_y = torch.zeros((B, M, Lmax), dtype=torch.int16, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(L.dsic_cdf_tables_gauss(_p(sz), _p(meta), _p(tab_z), B, N, Lmax, _p(err), _stream()), "gauss")
    _lib.check(L.dsic_cdf_tables_student(_p(sy), _p(ny), _p(meta), _p(tab_y), B, M, Lmax, _p(err), _stream()),
               "student")
    return tab_y.cpu().numpy().view(np.uint16), tab_z.cpu().numpy().view(np.uint16), int(err.item())


@pytest.mark.parametrize("B", [1, 20, 64])
def test_tables_with_per_image_supports_equal_oracle(B):
    """smin differs per image; supports straddle 0 (symmetric and lopsided) or lie on one side of it, and the
    z supports of a workgroup's images overlap only in part."""
    rng = np.random.default_rng(40 + B)
    Lmax, N, M = 160, 6, 5
    kinds = [(-30, 61), (-12, 25), (-70, 90), (1, 40), (-60, 45), (-5, 6), (0, 1), (-90, 91), (3, 21), (-25, 26)]
    rows = []
    for b in range(B):
        ys, yl = kinds[b % len(kinds)]
        zs, zl = kinds[(3 * b + 1) % len(kinds)]
        rows.append([ys + int(rng.integers(-3, 4)) * (b % 3 == 1), yl, zs - (b % 4), zl + (b % 5)])
    sz = rng.uniform(0.3, 8.0, N).astype(np.float32)
    sy = rng.uniform(0.3, 8.0, (B, M)).astype(np.float32)
    ny = rng.uniform(2.0, 80.0, (B, M)).astype(np.float32)
    ty, tz, err = _tables(rows, sz, sy, ny, Lmax)
    assert err == 0
    for b, (ys, yl, zs, zl) in enumerate(rows):
        assert np.array_equal(tz[b, :, :zl], E.tables_gauss(sz, zs, zl)), b
        assert np.array_equal(ty[b, :, :yl], E.tables_student(sy[b], ny[b], ys, yl)), b


def test_tables_far_apart_supports_and_bad_width():
    """z supports too far apart to share one row (each table evaluates its own), and a support wider than Lmax (error
    bit 1) beside valid ones."""
    rng = np.random.default_rng(7)
    Lmax, N, M = 64, 3, 2
    rows = [[-20, 41, -5000, 30], [-20, 41, 4000, 21], [-3, 7, -10, 200], [-8, 17, 20, 11]]
    sz = rng.uniform(0.5, 4.0, N).astype(np.float32)
    sy = rng.uniform(0.5, 4.0, (4, M)).astype(np.float32)
    ny = rng.uniform(2.0, 30.0, (4, M)).astype(np.float32)
    ty, tz, err = _tables(rows, sz, sy, ny, Lmax)
    assert err & 1
    for b, (ys, yl, zs, zl) in enumerate(rows):
        assert np.array_equal(ty[b, :, :yl], E.tables_student(sy[b], ny[b], ys, yl)), b
        if zl <= Lmax:
            assert np.array_equal(tz[b, :, :zl], E.tables_gauss(sz, zs, zl)), b
