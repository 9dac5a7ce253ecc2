"""The kernels of csrc/hyper_rate.hip, element by element, against the float64 reference of tests/rate_ref.py.

Whole-model tests see these kernels only through per-image sums; here every output element is held to the reference
at its own position (sigma and nu differ per channel and x per pixel, so a value stored at a wrong place fails), the
quantised latents are compared bit for bit with torch.round on the host, and the shapes walk the LDS tile of
rate_kernel (RATE_PT = 16 pixels x M channels, float4 stores when HWy % 4 == 0, 16 slices per image, the dynamic-LDS
opt-in above M = 294) and both pooling layouts of hyper_params_kernel.  All inputs are seeded and built on the host.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import rate_ref as R

pytestmark = pytest.mark.gpu

K_GPU = R.K_GPU
U32 = R.U32


@pytest.fixture(scope="module")
def ops():
    from dsic_amd import ops as _ops
    return _ops


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def same_bits(a, b):
    """Bit equality (torch.equal would take -0.0 for +0.0)."""
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def tie_table(big=True):
    """Exact ties k + 1/2 for even and odd k of both signs, their float32 neighbours on both sides, +-0,
    +-0.49999997 (the largest float32 below 1/2) and, with `big`, a value above 2^23 (no fraction bits left)."""
    ks = np.array([0, 1, 2, 3, 6, 7, 38, 39, -1, -2, -3, -4, -7, -8, -39, -40], dtype=np.float32)
    ties = ks + np.float32(0.5)
    parts = [ties, np.nextafter(ties, np.float32(np.inf)), np.nextafter(ties, np.float32(-np.inf)),
             np.array([0.0, -0.0, 0.49999997, -0.49999997], dtype=np.float32)]
    if big:
        parts.append(np.array([8388609.0, -8388609.0], dtype=np.float32))
    t = np.concatenate(parts).astype(np.float32)
    assert t[0] == 0.5 and np.float32(0.49999997) < np.float32(0.5)
    return torch.from_numpy(t)


def _plant(x, table):
    """Write `table` at the start of every image of x (flattened) and, where the image is large enough, reversed at
    its end, so that the planted values also sit in the last slice / the tail block."""
    B = x.shape[0]
    flat = x.view(B, -1)
    n = min(flat.shape[1], table.numel())
    flat[:, :n] = table[:n]
    if flat.shape[1] >= 2 * table.numel():
        flat[:, -table.numel():] = table.flip(0)
    return x


def _log_uniform(shape, lo, hi, g):
    return torch.exp(torch.rand(shape, generator=g, dtype=torch.float64) * (math.log(hi) - math.log(lo))
                     + math.log(lo)).to(torch.float32)


def _f32(v):
    return np.float32(v)


SIGMA_PLANTS = [_f32(1e-3), np.nextafter(_f32(1e-3), _f32(0)), _f32(1e3), np.nextafter(_f32(1e3), _f32(np.inf))]
NU_PLANTS = [_f32(2), np.nextafter(_f32(2), _f32(0)), _f32(100), np.nextafter(_f32(100), _f32(np.inf))]

RATE_CASES = [
    # (B, Hy, Wy, M, Hz, Wz, N, per_element, mode)
    (2, 16, 16, 192, 4, 4, 128, False, "round"),   # reference shape, float4 path
    (3, 3, 5, 192, 1, 2, 128, False, "round"),     # HWy = 15: scalar stores, slices 4..15 empty
    (2, 3, 6, 192, 1, 1, 128, False, "round"),     # HWy = 18: last non-empty slice holds 2 pixels
    (1, 1, 1, 8, 1, 1, 16, False, "round"),        # one pixel, smallest M and N; slice 15 owns z and has no y
    (2, 4, 17, 96, 2, 2, 80, False, "noise"),      # HWy = 68: pps = 8, a 4-pixel last slice, y_noisy / z_noisy given
    (2, 4, 6, 320, 1, 2, 192, False, "round"),     # M > 294: the dynamic-LDS opt-in on its first call
    (1, 2, 2, 512, 1, 1, 256, False, "round"),     # M = MAXM
    (2, 32, 32, 192, 8, 8, 128, False, "round"),   # 512x512 patch latents, several LDS tiles per slice
    (2, 5, 7, 96, 2, 2, 80, True, "round"),        # per_element
    (2, 4, 4, 320, 1, 1, 192, True, "noise"),      # per_element with large M and noise
]


def _rate_inputs(case, seed):
    B, Hy, Wy, M, Hz, Wz, N, per_element, mode = case
    g = torch.Generator().manual_seed(seed)
    y = _plant((torch.rand((B, Hy, Wy, M), generator=g) * 2 - 1) * 40, tie_table())
    z = _plant((torch.rand((B, Hz, Wz, N), generator=g) * 2 - 1) * 40, tie_table(big=False))
    shape = (B, M, Hy, Wy) if per_element else (B, M)
    sigma = _log_uniform(shape, 2e-4, 5e3, g)
    nu = _log_uniform(shape, 1.1, 250.0, g)
    # both clamp bounds, and the float32 neighbour just outside each, on channels (elements) of their own
    sf, nf = sigma.view(B, -1), nu.view(B, -1)
    sf[:, 0:4] = torch.tensor(SIGMA_PLANTS)
    nf[:, 4:8] = torch.tensor(NU_PLANTS)
    z_log_sigma = (torch.rand(N, generator=g) * 2 - 1) * 9
    z_log_sigma[0], z_log_sigma[1] = -9.0, 9.0
    y_noisy = z_noisy = None
    if mode == "noise":
        y_noisy = y + (torch.rand(y.shape, generator=g) - 0.5)
        z_noisy = z + (torch.rand(z.shape, generator=g) - 0.5)
    return y, z, sigma, nu, z_log_sigma, y_noisy, z_noisy


def _run_rate(ops, inp, rows=slice(None)):
    y, z, sigma, nu, zls, yn, zn = inp
    c = lambda t: None if t is None else t[rows].cuda()
    out = ops.rate(c(y), c(z), c(sigma), c(nu), zls.cuda(), c(yn), c(zn))
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


RATE_KEYS = ("y_hat_nhwc", "y_tilde", "z_tilde", "nll_y", "nll_z", "sums")


@pytest.mark.parametrize("case", RATE_CASES, ids=["-".join(str(int(v) if isinstance(v, bool) else v) for v in c)
                                                  for c in RATE_CASES])
def test_rate_elementwise(ops, case):
    B, Hy, Wy, M, Hz, Wz, N, per_element, mode = case
    inp = _rate_inputs(case, seed=1000 + RATE_CASES.index(case))
    y, z, sigma, nu, zls, yn, zn = inp
    out = _run_rate(ops, inp)
    # 1. the latents the coder writes
    assert same_bits(out["y_hat_nhwc"], torch.round(y))
    # 2./3. what the rate is evaluated at, in the reference's NCHW layout
    y_t = (yn if mode == "noise" else torch.round(y)).permute(0, 3, 1, 2).contiguous()
    z_t = (zn if mode == "noise" else torch.round(z)).permute(0, 3, 1, 2).contiguous()
    assert same_bits(out["y_tilde"], y_t)
    assert same_bits(out["z_tilde"], z_t)
    # 4. every element of the rate inside the envelope of the float64 reference at ITS sigma, nu and x
    s4 = sigma if per_element else sigma.view(B, M, 1, 1)
    n4 = nu if per_element else nu.view(B, M, 1, 1)
    ref_y, env_y = R.student_bits64(y_t, s4, n4), R.env_student(y_t, s4, n4)
    zl4 = R.channel_log_sigma(zls)
    ref_z, env_z = R.gauss_bits64(z_t, zl4), R.env_gauss(z_t, zl4)
    ratio_y = (out["nll_y"].double() - ref_y).abs() / env_y
    ratio_z = (out["nll_z"].double() - ref_z).abs() / env_z
    print(f"rate {case}: worst |device - float64| / envelope: nll_y {float(ratio_y.max()):.2f}, "
          f"nll_z {float(ratio_z.max()):.2f}")
    assert out["nll_y"].shape == ref_y.shape and out["nll_z"].shape == ref_z.shape
    assert torch.isfinite(out["nll_y"]).all() and torch.isfinite(out["nll_z"]).all()
    assert float(ratio_y.max()) <= K_GPU, np.unravel_index(int(ratio_y.argmax()), ratio_y.shape)
    assert float(ratio_z.max()) <= K_GPU, np.unravel_index(int(ratio_z.argmax()), ratio_z.shape)
    # 5. the per-image sums count every element exactly once (fp64 accumulation) ...
    sums = out["sums"]
    assert sums.shape == (B, 2) and sums.dtype == torch.float64
    for col, nll, ref, env in ((0, out["nll_y"], ref_y, env_y), (1, out["nll_z"], ref_z, env_z)):
        own = nll.double().sum(dim=(1, 2, 3))
        assert float(((sums[:, col] - own).abs() / own.abs()).max()) <= 1e-9, col
        # ... and lie within the summed envelope of the reference's sum
        assert bool(((sums[:, col] - ref.sum(dim=(1, 2, 3))).abs() <= K_GPU * env.sum(dim=(1, 2, 3))).all()), col
    # 6. the stand-alone kernels use the same arithmetic
    yt_d, zt_d = out["y_tilde"].cuda(), out["z_tilde"].cuda()
    if not per_element:
        sc, nc = sigma.cuda().view(B, M, 1, 1), nu.cuda().view(B, M, 1, 1)
        per_channel = ops.student_t_bits(yt_d, sc.expand_as(yt_d), nc.expand_as(yt_d))
        assert same_bits(per_channel, out["nll_y"]), "student_t_bits, per-channel path"
        full = ops.student_t_bits(yt_d, sc.expand_as(yt_d).contiguous(), nc.expand_as(yt_d).contiguous())
    else:
        full = ops.student_t_bits(yt_d, sigma.cuda(), nu.cuda())
    assert same_bits(full, out["nll_y"]), "student_t_bits, per-element path"
    assert same_bits(ops.gaussian_bits(zt_d, zls.cuda()), out["nll_z"]), "gaussian_bits"
    # 7. run-to-run determinism, and an image does not depend on its batch
    again = _run_rate(ops, inp)
    for k in RATE_KEYS:
        assert same_bits(again[k], out[k]), k
    alone = _run_rate(ops, inp, slice(B - 1, B))
    for k in RATE_KEYS:
        assert same_bits(alone[k], out[k][B - 1:]), k


def _raw_rate_args(B, Hy, Wy, M, Hz, Wz, N):
    dev = "cuda"
    t = {"y": torch.zeros((B, Hy, Wy, M), device=dev), "z": torch.zeros((B, Hz, Wz, N), device=dev),
         "sigma": torch.ones((B, M), device=dev), "nu": torch.full((B, M), 5.0, device=dev),
         "zls": torch.zeros(N, device=dev)}
    sentinel = -12345.0
    o = {"y_hat": torch.full((B, Hy, Wy, M), sentinel, device=dev), "y_t": torch.full((B, M, Hy, Wy), sentinel, device=dev),
         "z_t": torch.full((B, N, Hz, Wz), sentinel, device=dev), "nll_y": torch.full((B, M, Hy, Wy), sentinel, device=dev),
         "nll_z": torch.full((B, N, Hz, Wz), sentinel, device=dev),
         "sums": torch.full((B, 2), sentinel, dtype=torch.float64, device=dev),
         "work": torch.full((B * 32,), sentinel, dtype=torch.float64, device=dev)}
    return t, o, sentinel


def _raw_rate(L, t, o, B, HWy, M, HWz, N, null=None):
    p = lambda name, x: ctypes.c_void_p(0 if name == null else x.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    return L.dsic_rate(p("y", t["y"]), p("z", t["z"]), ctypes.c_void_p(0), ctypes.c_void_p(0), p("sigma", t["sigma"]),
                       p("nu", t["nu"]), p("zls", t["zls"]), p("y_hat", o["y_hat"]), p("y_t", o["y_t"]),
                       p("z_t", o["z_t"]), p("nll_y", o["nll_y"]), p("nll_z", o["nll_z"]), p("sums", o["sums"]),
                       p("work", o["work"]), B, HWy, M, HWz, N, 0, stream)


def test_rate_refusals(ops):
    """Each refused before anything is launched, with the error class test_bad_arguments_raise expects (ValueError
    for an invalid argument)."""
    from dsic_amd import lib
    L = lib.load()
    with pytest.raises(ValueError, match="M=520"):           # above MAXM = 512
        ops.rate(torch.zeros((1, 1, 1, 520), device="cuda"), torch.zeros((1, 1, 1, 16), device="cuda"),
                 torch.ones((1, 520), device="cuda"), torch.full((1, 520), 5.0, device="cuda"),
                 torch.zeros(16, device="cuda"))
    B, Hy, Wy, M, Hz, Wz, N = 1, 2, 2, 8, 1, 1, 16
    t, o, sentinel = _raw_rate_args(B, Hy, Wy, M, Hz, Wz, N)
    assert lib.DSIC_OK == _raw_rate(L, t, o, B, Hy * Wy, M, Hz * Wz, N)          # the raw call itself is well formed
    torch.cuda.synchronize()
    assert float(o["nll_y"].min()) > sentinel
    t, o, sentinel = _raw_rate_args(B, Hy, Wy, M, Hz, Wz, N)
    for what, kw, match in (("HWy*M = 2^31", dict(HWy=1 << 22, M=512), "too large"),
                            ("B = 0", dict(B=0), "empty"),
                            ("null sigma", dict(null="sigma"), "null"),
                            ("null output", dict(null="nll_y"), "null")):
        a = dict(B=B, HWy=Hy * Wy, M=M, HWz=Hz * Wz, N=N, null=None)
        a.update(kw)
        rc = _raw_rate(L, t, o, a["B"], a["HWy"], a["M"], a["HWz"], a["N"], a["null"])
        assert rc == lib.DSIC_EINVAL, what
        with pytest.raises(ValueError, match=match):
            lib.check(rc, "rate")
    torch.cuda.synchronize()
    for k, v in o.items():                                    # nothing was launched: no output was touched
        assert bool((v == sentinel).all()), k


HYPER_CASES = [(2, 16, 16, 128, 192),    # the model's shape: two half streams per channel
               (3, 1, 1, 128, 192),      # one pixel: the second half stream is empty
               (1, 1, 3, 16, 8),         # smallest N and M, odd pixel count
               (2, 5, 7, 80, 96),        # N below 128, odd pixel count
               (2, 4, 4, 160, 320),      # 128 < N <= 256: one stream per thread; 2M > 256 outputs
               (1, 32, 32, 256, 512),    # N = MAXN, longest pooling sum
               (5, 2, 2, 128, 192)]


def _hyper_inputs(B, Ht, Wt, N, M, seed):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    t = torch.relu(rn(B, Ht, Wt, N) + 0.3) * 2.0              # what h_s hands over: a ReLU output
    args = []
    for head in ("sigma", "nu"):
        w1, b1 = rn(N, N) * (2.0 / math.sqrt(N)), rn(N) * 0.5          # hidden units of both signs
        w2 = rn(N, M) * (0.5 / math.sqrt(N))
        if head == "sigma":
            b2 = (torch.rand(M, generator=g) * 2 - 1) * 3
        else:                                                  # exp(log_nu) from far below min_nu to far above max_nu
            b2 = torch.rand(M, generator=g) * 8 - 1.5
            b2[0], b2[1] = -6.0, 12.0
        args += [w1, b1, w2, b2]
    return t, args


@pytest.mark.parametrize("B,Ht,Wt,N,M", HYPER_CASES)
def test_hyper_params_vs_float64(ops, B, Ht, Wt, N, M):
    min_nu, max_nu = 1.1, 100.0
    t, args = _hyper_inputs(B, Ht, Wt, N, M, seed=7 * N + M + B)
    val, bnd = R.hyper_params64(t, *args, min_nu, max_nu)
    pre = t.double().mean(dim=(1, 2)) @ args[0].double() + args[1].double()
    assert bool((pre < 0).any()) and bool((pre > 0).any())     # the ReLU is exercised
    lo, hi = float(np.float32(min_nu)), float(np.float32(max_nu))
    below = val["nu_unclamped"] + bnd["nu_unclamped"] < lo
    above = val["nu_unclamped"] - bnd["nu_unclamped"] > hi
    assert int(below.sum()) > 0 and int(above.sum()) > 0 and int((~below & ~above).sum()) > 0
    dargs = [a.cuda() for a in args]
    got = dict(zip(("log_sigma", "log_nu", "sigma", "nu"),
                   (o.cpu() for o in ops.hyper_params(t.cuda(), *dargs, M, min_nu, max_nu))))
    for k, v in got.items():
        assert v.shape == (B, M)
        ratio = float(((v.double() - val[k]).abs() / bnd[k]).max())
        print(f"hyper_params {(B, Ht, Wt, N, M)}: {k} error / forward-error bound = {ratio:.3f}")
        assert ratio <= 1.0, k
    assert bool((got["nu"][below] == np.float32(min_nu)).all())
    assert bool((got["nu"][above] == np.float32(max_nu)).all())
    assert float(got["nu"].min()) >= np.float32(min_nu) and float(got["nu"].max()) <= np.float32(max_nu)
    for b in range(B):                                         # an image does not depend on its batch
        alone = ops.hyper_params(t[b:b + 1].cuda(), *dargs, M, min_nu, max_nu)
        for k, a in zip(got, alone):
            assert same_bits(a, got[k][b:b + 1]), (k, b)


def test_hyper_params_refuses_wide_n(ops):
    N, M = 272, 8                                              # above MAXN = 256
    z = lambda *s: torch.zeros(*s, device="cuda")
    with pytest.raises(ValueError, match="N=272"):
        ops.hyper_params(z(1, 1, 1, N), z(N, N), z(N), z(N, M), z(M), z(N, N), z(N), z(N, M), z(M), M, 1.1, 100.0)


def test_round_half_even_bit_exact(ops):
    special = torch.cat([tie_table(), torch.tensor([float("inf"), float("-inf")])])
    assert same_bits(ops.round_half_even(special.cuda()), torch.round(special))
    want = torch.round(tie_table())
    assert want[0] == 0.0 and want[1] == 2.0 and same_bits(want[8:9], torch.tensor([-0.0]))   # half to even, signed zero
    g = torch.Generator().manual_seed(4)
    for n in (1, 255, 256, 257, 100003):                       # around the 256-thread block, and a long tail block
        x = (torch.rand(n, generator=g) * 2 - 1) * 100
        k = min(n, special.numel())
        x[n - k:] = special[:k]                                # ties in the tail block as well
        assert same_bits(ops.round_half_even(x.cuda()), torch.round(x)), n
    nan = ops.round_half_even(torch.tensor([float("nan"), 1.5, float("nan")], device="cuda")).cpu()
    assert bool(torch.isnan(nan[0])) and bool(torch.isnan(nan[2])) and float(nan[1]) == 2.0


@pytest.mark.parametrize("B,H,W,M", [(1, 1, 1, 8), (2, 3, 5, 96), (2, 8, 4, 192)])
def test_sigma_nu_spatial_positions_and_values(ops, B, H, W, M):
    min_nu, max_nu = 1.1, 100.0
    n = B * H * W * M
    idx = torch.arange(n, dtype=torch.float64)
    # the value encodes the NHWC index: neighbours differ by far more than the tolerance
    ls = (idx / n * 16 - 8).to(torch.float32).view(B, H, W, M)
    ln = (((idx * 7919) % n) / n * 6 - 0.5).to(torch.float32).view(B, H, W, M)   # exp from 0.6 to 245: both clamps
    sigma, nu = (o.cpu() for o in ops.sigma_nu_spatial(ls.cuda(), ln.cuda(), min_nu, max_nu))
    assert sigma.shape == nu.shape == (B, M, H, W)
    want_s = torch.exp(ls.double()).permute(0, 3, 1, 2)
    raw_n = torch.exp(ln.double()).permute(0, 3, 1, 2)
    lo, hi = float(np.float32(min_nu)), float(np.float32(max_nu))
    assert float(((sigma.double() - want_s).abs() / want_s).max()) <= 4 * U32
    assert float(((nu.double() - raw_n.clamp(lo, hi)).abs() / raw_n.clamp(lo, hi)).max()) <= 4 * U32
    below, above = raw_n * (1 + 4 * U32) < lo, raw_n * (1 - 4 * U32) > hi
    if n > 8:
        assert int(below.sum()) > 0 and int(above.sum()) > 0
    assert bool((nu[below] == np.float32(min_nu)).all()) and bool((nu[above] == np.float32(max_nu)).all())


@pytest.mark.parametrize("B,C,H,W", [(1, 1, 1, 1), (2, 16, 5, 7), (3, 192, 4, 6)])
@pytest.mark.parametrize("inverse", [False, True])
def test_gdn_nchw_vs_float64(ops, B, C, H, W, inverse):
    g = torch.Generator().manual_seed(100 * C + H)
    x = (torch.rand(B, C, H, W, generator=g) * 2 - 1) * 10 ** (torch.rand(B, C, H, W, generator=g) * 6 - 3)
    beta = 1e-6 + (4 - 1e-6) * torch.rand(C, generator=g)
    gamma = 2 * torch.rand(C, generator=g)
    xf = x.view(-1)
    xf[0] = 1e3
    if C > 1:
        beta[0], beta[1], gamma[1], gamma[2] = 1e-6, 4.0, 0.0, 2.0
        xf[1], xf[2], xf[-1] = 0.0, -1e3, -0.0
    got = ops.gdn_nchw(x.cuda(), beta.cuda(), gamma.cuda(), inverse).cpu()
    want = R.gdn64(x, beta, gamma, inverse)
    # multiply, multiply, add, square root, then multiply or divide, each correctly rounded: the three before the
    # root are halved by it, 3.5 * 2^-24 in all
    excess = (got.double() - want).abs() - 4 * U32 * want.abs()
    assert float(excess.max()) <= 0.0, np.unravel_index(int(excess.argmax()), excess.shape)
