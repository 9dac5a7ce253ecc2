"""Anchors of tests/ssim_ref.py, the float64 reference the GPU metric tests compare against: the independent float64
MS-SSIM of tests/test_oracle_metrics.py for the formulas, the C library's expf for the window, the fp32 oracle for the
envelope, torch's avg_pool2d for the pools, float32 numpy restatements for the finalize and squared-error envelopes;
and the condition on the test inputs that makes one output pixel counted zero times or twice impossible to pass."""
import ctypes
import ctypes.util

import numpy as np
import torch
import torch.nn.functional as F

import ssim_ref as R
from oracle import ref_metrics as RM
from test_oracle_metrics import _np_msssim, _pair


def _oracle_level(X, Y, clamp):
    """The fp32 oracle on planes [P,H,W] -> (mean cs [P], mean ssim [P]), float64."""
    x, y = torch.from_numpy(X)[None], torch.from_numpy(Y)[None]
    if clamp:
        x = x.clamp(0, 1)
    s, cs = RM._ssim_cs(x, y, 1.0, RM._gauss_1d())
    return cs[0].double().numpy(), s[0].double().numpy()


def test_window_is_the_one_the_kernel_builds():
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    libm.expf.restype, libm.expf.argtypes = ctypes.c_float, [ctypes.c_float]
    g, s = [], np.float32(0.0)
    for i in range(R.WIN):                                      # ssim_level_launch, operation by operation
        d = np.float32(i - R.WIN // 2)
        g.append(np.float32(libm.expf(np.float32(-(d * d)) / np.float32(np.float32(2.0) * np.float32(1.5) * np.float32(1.5)))))
        s = np.float32(s + g[-1])
    want = np.array([np.float32(v / s) for v in g], dtype=np.float32)
    got = R.window32()
    assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32))
    # the oracle's taps (torch sums them in another order) are the same to an ulp of the largest
    theirs = RM._gauss_1d().numpy()
    assert np.max(np.abs(theirs.astype(np.float64) - got)) <= 2.0 ** -24 * float(got.max()) * 2


def test_reference_reproduces_the_independent_float64_ms_ssim():
    c = np.arange(11) - 5
    g = np.exp(-(c ** 2) / (2 * 1.5 ** 2))
    g /= g.sum()                                                # the float64 window and constants of _np_msssim
    worst = 0.0
    for (H, W, wts) in ((256, 256, (0.3, 0.5, 0.2)), (176, 200, RM.DEFAULT_WEIGHTS), (165, 163, (0.3, 0.5, 0.2))):
        x, y = _pair(2, H, W, 3)
        want = _np_msssim(y, x, wts)
        B, C = y.shape[:2]
        a, b = y.reshape(B * C, H, W).astype(np.float64), x.reshape(B * C, H, W).astype(np.float64)
        means = np.zeros((len(wts), B * C, 2))
        for lvl in range(len(wts)):
            ref = R.level64(a, b, 0.01 ** 2, 0.03 ** 2, window=g)
            means[lvl, :, 0], means[lvl, :, 1] = ref["mean_cs"], ref["mean_ss"]
            a, b = R.pool64(a), R.pool64(b)
        w64 = np.asarray(wts, dtype=np.float64)
        v = np.maximum(np.where((np.arange(len(wts)) == len(wts) - 1)[:, None], means[..., 1], means[..., 0]), 0)
        got = np.prod(v ** w64[:, None], axis=0).reshape(B, C).mean(axis=1)
        worst = max(worst, float(np.max(np.abs(got - want))))
        # finalize64 reads the weights as the kernel does, in float32: the same to their rounding
        fin, _ = R.finalize64(means, wts, 1, B, C)
        assert np.max(np.abs(fin - want)) <= 1e-7
    print(f"level64 + pool64 vs _np_msssim: max |diff| {worst:.3e}")
    assert worst <= 1e-12


def test_fp32_oracle_stays_inside_the_envelope():
    C1, C2 = R.constants()
    theirs = RM._gauss_1d().numpy()
    worst, worst_pool, where = 0.0, 0.0, None
    for fam, case, kind, clamp in R.all_level_cases():
        X, Y = R.make_inputs(*case, R.case_seed(case), kind)
        level = 0
        while min(X.shape[-2:]) >= R.WIN and level < 2:
            ref = R.level64(X, Y, C1, C2, clamp, window=theirs)
            cs, ss = _oracle_level(X, Y, clamp)
            ratio = max(float(np.max(np.abs(cs - ref["mean_cs"]) / ref["env_cs"])),
                        float(np.max(np.abs(ss - ref["mean_ss"]) / ref["env_ss"])))
            if ratio > worst:
                worst, where = ratio, (fam, case, kind, level)
            assert ratio <= R.K_ORACLE, (fam, case, kind, level, ratio)
            # the oracle's pooled planes (they feed its next level) against pool64, and pool32 bit for bit
            xc = np.clip(X, np.float32(0), np.float32(1)) if clamp else X
            pad = [d % 2 for d in X.shape[-2:]]
            nxt = []
            for a in (xc, Y):
                got = F.avg_pool2d(torch.from_numpy(a)[None], kernel_size=2, padding=pad)[0].numpy()
                env = R.env_pool(a)
                r = np.abs(got.astype(np.float64) - R.pool64(a))
                worst_pool = max(worst_pool, float(np.max(np.where(env > 0, r / np.where(env > 0, env, 1), 0))))
                assert bool(np.all(r <= R.K_ORACLE * env))
                nxt.append(got)
            X, Y, clamp, level = nxt[0], nxt[1], 0, level + 1
    print(f"fp32 oracle / envelope: levels {worst:.3f} at {where}, pooled planes {worst_pool:.3f}; K_ORACLE = {R.K_ORACLE}")
    assert R.K_GPU == 2 * R.K_ORACLE


def test_every_output_pixel_counts_and_planes_are_told_apart():
    """A condition on the inputs, not a measurement: on every "ramp" case each pixel's share of the plane mean,
    |v| / (Ho Wo), is at least 8 K_GPU envelopes of that mean, for the cs and the ssim map alike - a pixel counted
    zero times or twice moves the mean by 8 times what the comparison allows; and the means of any two planes of a
    case differ by more than 16 K_GPU envelopes, so a plane read in another's place cannot pass either."""
    C1, C2 = R.constants()
    smallest, smallest_pair = np.inf, np.inf
    for fam, case, kind, clamp in R.all_level_cases():
        if kind != "ramp":
            continue
        planes, H, W = case
        X, Y = R.make_inputs(*case, R.case_seed(case), kind)
        ref = R.level64(X, Y, C1, C2, clamp)
        n = (H - 10) * (W - 10)
        for v, e, m in (("cs", "env_cs", "mean_cs"), ("ss", "env_ss", "mean_ss")):
            share = np.abs(ref[v]).min(axis=(-2, -1)) / n / ref[e]
            smallest = min(smallest, float(share.min()))
            assert float(share.min()) >= 8 * R.K_GPU, (case, v, float(share.min()))
            if planes > 1:
                order = np.argsort(ref[m])
                gap = np.diff(ref[m][order]) / np.maximum(ref[e][order][1:], ref[e][order][:-1])
                smallest_pair = min(smallest_pair, float(gap.min()))
                assert float(gap.min()) > 16 * R.K_GPU, (case, m, float(gap.min()))
    print(f"smallest pixel share / envelope {smallest:.1f} (needs {8 * R.K_GPU:.0f}); "
          f"smallest gap between two planes' means / envelope {smallest_pair:.1f} (needs {16 * R.K_GPU:.0f})")


def test_pool32_matches_avg_pool2d_and_pool64():
    rng = np.random.default_rng(5)
    for shape in ((3, 9, 13), (2, 10, 13), (2, 9, 12), (1, 1, 1), (5, 64, 64)):
        a = (rng.random(shape) * 1.4 - 0.2).astype(np.float32)
        pad = [d % 2 for d in shape[-2:]]
        for clamp in (False, True):
            src = np.clip(a, np.float32(0), np.float32(1)) if clamp else a
            want = F.avg_pool2d(torch.from_numpy(src)[None], kernel_size=2, padding=pad)[0].numpy()
            got = R.pool32(a, clamp)
            assert got.shape == want.shape == shape[:1] + R.pooled_shape(*shape[-2:])
            ulp = np.spacing(np.abs(want).astype(np.float32))
            assert bool(np.all(np.abs(got.astype(np.float64) - want) <= ulp)), shape
        # multiples of 2^-10 in [-1, 1]: every partial sum is exact in float32, so pool32 is pool64 rounded
        q = (rng.integers(-1024, 1025, shape) / 1024.0).astype(np.float32)
        exact = R.pool64(q).astype(np.float32)
        assert np.array_equal(R.pool32(q).view(np.int32), exact.view(np.int32)), shape


def test_finalize_and_sqerr_envelopes_hold_a_float32_restatement():
    worst = 0.0
    for levels, B, C in R.FINALIZE_CASES:
        means = R.finalize_means(levels, B, C, seed=100 * levels + 10 * B + C)
        for relu_last in ((0, 1) if levels == 1 else (1,)):
            want, env = R.finalize64(means, R.FINALIZE_WEIGHTS[levels], relu_last, B, C)
            got = R.finalize32(means, R.FINALIZE_WEIGHTS[levels], relu_last, B, C).astype(np.float64)
            err = np.abs(got - want)
            assert bool(np.all(err <= R.K_ORACLE * env)), (levels, B, C, relu_last)
            worst = max([worst] + (err[env > 0] / env[env > 0]).tolist())
    worst_sq = 0.0
    for B, n in R.SQERR_CASES:
        a, b = R.sqerr_inputs(B, n, seed=n + B)
        for clamp in (False, True):
            want, env = R.sqerr64(a, b, clamp)
            err = np.abs(R.sqerr32(a, b, clamp) - want)
            assert bool(np.all(err <= R.K_ORACLE * env)), (B, n, clamp)
            worst_sq = max(worst_sq, float(np.max(err / env)))
        assert float(R.sqerr32(a, a)[0]) == 0.0 and float(R.sqerr64(a, a)[0][0]) == 0.0
    print(f"float32 restatement / envelope: finalize {worst:.3f}, sqerr {worst_sq:.3f}")
    # the planted values do what they are there for
    m = R.finalize_means(1, 1, 4, seed=1)
    assert m[0, 3, 1] < 0 and R.finalize64(m, (1.0,), 0, 1, 4)[0][0] < R.finalize64(m, (1.0,), 1, 1, 4)[0][0]
    one = np.full((1, 1, 2), -0.25)
    assert R.finalize64(one, (1.0,), 1, 1, 1)[0][0] == 0.0 and R.finalize64(one, (1.0,), 0, 1, 1)[0][0] == -0.25
