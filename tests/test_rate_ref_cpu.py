"""Anchors of tests/rate_ref.py, the float64 reference the GPU rate-tail tests compare against: scipy and mpmath for
the two densities, the fp32 oracle and the reference's own recorded bits for the envelope, and the oracle's hyper
heads and GDN for the other two restatements."""
import math
import os

import numpy as np
import torch

import rate_ref as R
from dsic_amd import synthetic as S
from oracle import ref_model as O

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
LN2 = math.log(2.0)


def _rel(a, b):
    return float(((a - b).abs() / b.abs()).max())


def test_bits_match_scipy_on_the_clamp_box():
    from scipy import stats
    sig = np.exp(np.linspace(math.log(R.SIGMA_MIN), math.log(R.SIGMA_MAX), 25))
    nus = np.exp(np.linspace(math.log(2.0), math.log(100.0), 23))
    xs = np.concatenate([np.arange(-200.0, 201.0, 12.5), [-0.5, -1e-3, 0.0, 1e-3, 0.37, 0.5, 1.5]])
    x, s, n = (torch.from_numpy(a.copy()) for a in np.meshgrid(xs, sig, nus, indexing="ij"))
    want = torch.from_numpy(-stats.t.logpdf(x.numpy(), n.numpy(), scale=s.numpy()) / LN2)
    got = R.student_bits64(x, s, n)
    print(f"student_bits64 vs scipy.stats.t: max rel {_rel(got, want):.3e} over {got.numel()} points")
    assert _rel(got, want) <= 1e-12
    ls = torch.from_numpy(np.linspace(math.log(R.SIGMA_MIN), math.log(R.SIGMA_MAX), 57))
    xg, lg = torch.meshgrid(torch.from_numpy(xs), ls, indexing="ij")
    want = torch.from_numpy(-stats.norm.logpdf(xg.numpy(), scale=np.exp(lg.numpy())) / LN2)
    got = R.gauss_bits64(xg, lg)
    print(f"gauss_bits64 vs scipy.stats.norm: max rel {_rel(got, want):.3e} over {got.numel()} points")
    assert _rel(got, want) <= 1e-12
    # outside the box the parameters are clamped first
    assert torch.equal(R.student_bits64(x[:, :1, :1], 1e-5, 0.5), R.student_bits64(x[:, :1, :1], R.SIGMA_MIN, 2.0))
    assert torch.equal(R.student_bits64(x[:, :1, :1], 1e5, 500.0), R.student_bits64(x[:, :1, :1], R.SIGMA_MAX, 100.0))
    assert torch.equal(R.gauss_bits64(xg[:, :1], 9.0), R.gauss_bits64(xg[:, :1], math.log(R.SIGMA_MAX)))


def test_bits_match_mpmath_at_50_digits():
    import mpmath as mp
    mp.mp.dps = 50

    def t_bits(x, s, n):
        x, s, n = mp.mpf(x), mp.mpf(s), mp.mpf(n)
        logc = mp.loggamma((n + 1) / 2) - mp.loggamma(n / 2) - mp.log(n * mp.pi) / 2 - mp.log(s)
        return -(logc - (n + 1) / 2 * mp.log1p((x / s) ** 2 / n)) / mp.log(2)

    def g_bits(x, s):
        x, s = mp.mpf(x), mp.mpf(s)
        return (mp.log(2 * mp.pi * s * s) / 2 + x * x / (2 * s * s)) / mp.log(2)

    pts = [(200.0, R.SIGMA_MIN, 2.0), (-200.0, R.SIGMA_MIN, 100.0), (0.0, R.SIGMA_MIN, 2.0), (0.0, R.SIGMA_MAX, 100.0),
           (200.0, R.SIGMA_MAX, 2.0), (0.5, 0.37, 2.0), (-1.5, 0.37, 100.0), (3.0, 1.0, 7.25), (-40.0, 12.5, 3.0),
           (1.0, 1e-2, 55.5), (8388609.0, R.SIGMA_MIN, 2.0), (-0.49999997, 250.0, 99.0)]
    worst = 0.0
    for x, s, n in pts:
        want = t_bits(x, s, n)
        got = float(R.student_bits64(torch.tensor(x, dtype=torch.float64), s, n))
        worst = max(worst, float(abs((mp.mpf(got) - want) / want)))
    print(f"student_bits64 vs mpmath: max rel {worst:.3e}")
    assert worst <= 1e-12
    worst = 0.0
    for x, s, _ in pts:
        want = g_bits(x, s)
        got = float(R.gauss_bits64(torch.tensor(x, dtype=torch.float64), math.log(s)))
        # log(s) is itself rounded to float64: evaluate the reference where the test does
        want = g_bits(x, mp.exp(mp.mpf(math.log(s)))) if R.SIGMA_MIN < s < R.SIGMA_MAX else want
        worst = max(worst, float(abs((mp.mpf(got) - want) / want)))
    print(f"gauss_bits64 vs mpmath: max rel {worst:.3e}")
    assert worst <= 1e-12


def _sweep(n=1_000_000, seed=20260101):
    """The fixed sweep: sigma log-uniform in [e^-8, e^8], nu log-uniform in [0.8, 330], log_sigma uniform in
    [-9, 9], x an integer in [-200, 200] with every second point shifted by U(-1/2, 1/2); blocks pinned at both sigma
    clamps, both nu clamps and x = 0."""
    g = np.random.default_rng(seed)
    sigma = np.exp(g.uniform(-8.0, 8.0, n))
    nu = np.exp(g.uniform(math.log(0.8), math.log(330.0), n))
    log_sigma = g.uniform(-9.0, 9.0, n)
    x = g.integers(-200, 201, n).astype(np.float64)
    x[1::2] += g.uniform(-0.5, 0.5, n // 2)
    blk = n // 50
    sigma[0 * blk:1 * blk] = 1e-3
    sigma[1 * blk:2 * blk] = 1e3
    log_sigma[0 * blk:1 * blk] = math.log(1e-3)
    log_sigma[1 * blk:2 * blk] = math.log(1e3)
    nu[2 * blk:3 * blk] = 2.0
    nu[3 * blk:4 * blk] = 100.0
    x[4 * blk:5 * blk] = 0.0
    x[:blk:3] = 0.0                                             # the clamps at the mode as well
    return tuple(torch.from_numpy(a.astype(np.float32)) for a in (x, sigma, nu, log_sigma))


def test_fp32_oracle_stays_inside_the_envelope_on_the_fixed_sweep():
    x, sigma, nu, log_sigma = _sweep()
    assert x.numel() == 1_000_000
    ratio_t = ((O.student_t_bits(x, sigma, nu).double() - R.student_bits64(x, sigma, nu)).abs()
               / R.env_student(x, sigma, nu))
    got_g = _oracle_gauss_elementwise(x, log_sigma)
    ratio_g = (got_g.double() - R.gauss_bits64(x, log_sigma)).abs() / R.env_gauss(x, log_sigma)
    i, j = int(ratio_t.argmax()), int(ratio_g.argmax())
    print(f"fp32 oracle / envelope, worst of 1e6: student-t {float(ratio_t.max()):.2f} "
          f"(x={float(x[i])}, sigma={float(sigma[i]):.4g}, nu={float(nu[i]):.4g}), "
          f"gaussian {float(ratio_g.max()):.2f} (x={float(x[j])}, log_sigma={float(log_sigma[j]):.4g})")
    assert float(ratio_t.max()) <= R.K_ORACLE
    assert float(ratio_g.max()) <= R.K_ORACLE


def _oracle_gauss_elementwise(x, log_sigma):
    """O.gaussian_bits takes one log_sigma per channel: lay the sweep out as [1, n, 1, 1]."""
    return O.gaussian_bits(x.view(1, -1, 1, 1), log_sigma).view(-1)


def test_reference_fixture_bits_inside_the_envelope():
    u = np.load(os.path.join(GOLDEN, "units.npz"))
    x = torch.from_numpy(u["studentt/x"])
    sig = torch.from_numpy(u["studentt/sigma"]).view(1, -1, 1, 1)
    nu = torch.from_numpy(u["studentt/nu"]).view(1, -1, 1, 1)
    r_t = (torch.from_numpy(u["studentt/bits"]).double() - R.student_bits64(x, sig, nu)).abs() / R.env_student(x, sig, nu)
    ls = R.channel_log_sigma(torch.from_numpy(u["gauss/log_sigma"]))
    r_g = (torch.from_numpy(u["gauss/bits"]).double() - R.gauss_bits64(x, ls)).abs() / R.env_gauss(x, ls)
    print(f"recorded reference bits / envelope: student-t {float(r_t.max()):.2f}, gaussian {float(r_g.max()):.2f}")
    assert float(r_t.max()) <= R.K_ORACLE and float(r_g.max()) <= R.K_ORACLE


def _head_args(sd):
    def im(key):                                               # Conv2d 1x1 weight [out,in,1,1] -> input-major [in][out]
        w = torch.from_numpy(sd[key + ".weight"])
        return w.view(w.shape[0], w.shape[1]).t().contiguous(), torch.from_numpy(sd[key + ".bias"])
    args = []
    for head in ("mlp_sigma", "mlp_nu"):
        for layer in (0, 2):
            args += list(im(f"h_s.{head}.{layer}"))
    return args


def test_hyper_params64_bounds_hold_the_fp32_oracle():
    for seed, N, M, B, hz, wz in ((3, 128, 192, 2, 2, 3), (11, 80, 96, 3, 1, 1)):
        sd = S.make_state_dict(seed=seed, N=N, M=M)
        z_hat = torch.round(torch.from_numpy(S.hash_uniform(B * N * hz * wz, seed, 77)).view(B, N, hz, wz) * 16 - 8)
        taps = {}
        ls, ln = O.hyper_synthesis(sd, z_hat, taps)
        t = taps["h_s.2"]                                      # [B,N,4hz,4wz], what the heads pool
        assert t.shape == (B, N, 4 * hz, 4 * wz)
        for min_nu, max_nu in ((2.0, 100.0), (1.1, 100.0)):
            val, bnd = R.hyper_params64(t.permute(0, 2, 3, 1), *_head_args(sd), min_nu, max_nu)
            got = {"log_sigma": ls[:, :, 0, 0], "log_nu": ln[:, :, 0, 0], "sigma": torch.exp(ls[:, :, 0, 0]),
                   "nu": torch.clamp(torch.exp(ln[:, :, 0, 0]), min_nu, max_nu)}
            for k, v in got.items():
                ratio = float(((v.double() - val[k]).abs() / bnd[k]).max())
                print(f"hyper_params64 N={N} M={M} min_nu={min_nu}: oracle {k} error / bound = {ratio:.3f}")
                assert ratio <= 1.0, k
            lo, hi = float(np.float32(min_nu)), float(np.float32(max_nu))
            assert int((val["nu"] == lo).sum()) > 0 and int((val["nu"] == hi).sum()) > 0   # both clamps are reached


def test_gdn64_matches_the_oracle():
    g = torch.Generator().manual_seed(9)
    for C, H, W in ((1, 1, 1), (16, 5, 7), (192, 4, 6)):
        x = (torch.rand(2, C, H, W, generator=g) * 2 - 1) * 10 ** (torch.rand(2, C, H, W, generator=g) * 6 - 3)
        beta_p = torch.sqrt(1e-6 + 4 * torch.rand(C, generator=g) + O.REPARAM_OFFSET)
        gam_p = torch.sqrt(2 * torch.rand(C, generator=g) + O.REPARAM_OFFSET)
        beta, gamma = beta_p ** 2 - O.REPARAM_OFFSET, gam_p ** 2 - O.REPARAM_OFFSET   # as the oracle forms them, fp32
        for inverse in (False, True):
            want = R.gdn64(x, beta, gamma, inverse)
            got = O.gdn(x, beta_p, gam_p.view(-1, 1, 1, 1), inverse).double()
            assert float(((got - want).abs() - 4 * R.U32 * want.abs()).max()) <= 0.0, (C, inverse)
