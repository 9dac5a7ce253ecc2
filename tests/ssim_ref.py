"""Float64 reference of the distortion metrics (csrc/metrics.hip): one SSIM level (per-pixel cs and ssim maps and their
per-plane means), the 2x2 average pool between levels, the MS-SSIM product and the per-image squared error, each with
the error envelope an fp32 evaluation of the same formula is entitled to.

A helper for tests/test_ssim_ref_cpu.py (which anchors it against the independent float64 MS-SSIM of
tests/test_oracle_metrics.py, the fp32 oracle and torch's avg_pool2d, and checks that the test inputs make every
output pixel count) and tests/test_gpu_metrics_levels.py (which holds the kernels to it level by level).  It restates
the formulas in numpy float64; it shares no code with the oracle or the product package.  Float32 inputs are widened
exactly, so a comparison measures the arithmetic of the implementation under test and not the rounding of its inputs.

Envelope of one SSIM level.  With f_ab = filt(|a*b|) (for the non-negative images the metric is defined on this is
filt(a*b); where a product is negative the rounding error of the sum follows the magnitudes, not the signed sum),
mu = filt(x or y), D = sigma1^2 + sigma2^2 + C2 and l the luminance factor, one float32 half-ulp of every term that
enters a pixel gives

    e_cs = U32 * [2 (f_xy + |mu1 mu2|) + |cs| (f_xx + f_yy + mu1^2 + mu2^2) + |cs| D] / D
    e_ss = |l| e_cs + 4 U32 |ss|

(numerator, denominator and the division of cs; the luminance factor's two sums, its division and the product with
cs).  The envelope of a plane mean is the mean of the per-pixel envelopes: the kernels accumulate in float64.

Measured |error| / envelope, largest over the cases (the tests print them):
    fp32 oracle on the host, levels (test_ssim_ref_cpu.py)   0.52 (constant planes; 0.27 on the textured kinds)
    fp32 oracle on the host, pooled planes                   0.85
    float32 numpy restatements of finalize / sqerr           0.31 / 0.37
    MI355X, per family of cases                              GPU_RATIOS below: not measured yet
"""
from __future__ import annotations

import numpy as np

U32 = 2.0 ** -24                     # float32 unit roundoff: half an ulp, relative
WIN, SIGMA = 11, 1.5
K_ORACLE = 1.0                       # cap the fp32 oracle meets on the host (test_ssim_ref_cpu.py measures it)
K_GPU = 2.0 * K_ORACLE               # twice that: v_rcp_f32 (1 ulp) in place of the IEEE division, fused multiply-adds
# largest |device - float64| / envelope seen on the MI355X per family of cases (tests/test_gpu_metrics_levels.py
# prints them); a value above K_GPU is a finding to explain, never a cap to raise.  Empty: not measured yet.
GPU_RATIOS = {}


def f64(a) -> np.ndarray:
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a).astype(np.float64)


def window32() -> np.ndarray:
    """The 11 float32 taps the kernel's host code builds: expf(-(d*d)/(2*1.5*1.5)) with every operation in float32,
    summed in ascending order, each divided by the sum.  expf is taken as the correctly rounded exponential (float64
    exp, rounded once); test_ssim_ref_cpu.py checks that against the C library's expf."""
    d = np.arange(WIN, dtype=np.float32) - np.float32(WIN // 2)
    q = -(d * d) / np.float32(2.0 * SIGMA * SIGMA)
    g = np.exp(q.astype(np.float64)).astype(np.float32)
    s = np.float32(0.0)
    for v in g:
        s = np.float32(s + v)
    return (g / s).astype(np.float32)


def _filt(a: np.ndarray, g: np.ndarray) -> np.ndarray:
    """Valid 11-tap filtering along H, then along W, taps in ascending order."""
    H, W = a.shape[-2:]
    t = g[0] * a[..., 0:H - WIN + 1, :]
    for k in range(1, WIN):
        t = t + g[k] * a[..., k:H - WIN + 1 + k, :]
    o = g[0] * t[..., :, 0:W - WIN + 1]
    for k in range(1, WIN):
        o = o + g[k] * t[..., :, k:W - WIN + 1 + k]
    return o


def constants(data_range=1.0):
    """(C1, C2) as the float32 values the kernel receives through its C ABI."""
    return np.float32((0.01 * data_range) ** 2), np.float32((0.03 * data_range) ** 2)


def level64(X, Y, C1, C2, clamp_x=False, window=None) -> dict:
    """One SSIM level of planes X, Y [..., H, W].  Returns cs, ss (per-pixel maps [..., H-10, W-10]), e_cs, e_ss
    (their per-pixel envelopes), mean_cs, mean_ss and env_cs, env_ss (per plane).  C1 and C2 are taken as given: pass
    the float32 values of constants() to compare with the kernel.  `window`: the 11 taps of the implementation under
    test where they are not the kernel's (torch sums the taps in another order than the
    kernel's host code, which moves every tap of the oracle's window by an ulp of the sum; that is a property of its
    window and not of its arithmetic)."""
    x, y = f64(X), f64(Y)
    if clamp_x:
        x = np.clip(x, 0.0, 1.0)
    C1, C2 = float(C1), float(C2)                               # np.float32 values (constants()) widen exactly
    g = (window32() if window is None else np.asarray(window)).astype(np.float64)
    H, W = x.shape[-2:]
    lead = x.shape[:-2]
    x, y = x.reshape(-1, H, W), y.reshape(-1, H, W)
    step = max(1, (1 << 16) // (H * W))                         # a few planes at a time: the maps stay in cache
    parts = [_level_planes(x[i:i + step], y[i:i + step], C1, C2, g) for i in range(0, x.shape[0], step)]
    out = {k: np.concatenate([p[k] for p in parts]).reshape(lead + parts[0][k].shape[1:]) for k in parts[0]}
    for k, e in (("cs", "e_cs"), ("ss", "e_ss")):
        out["mean_" + k] = out[k].mean(axis=(-2, -1))
        out["env_" + k] = out[e].mean(axis=(-2, -1))
    return out


def _level_planes(x, y, C1, C2, g):
    mu1, mu2 = _filt(x, g), _filt(y, g)
    fxx, fyy, fxy = _filt(x * x, g), _filt(y * y, g), _filt(x * y, g)
    axy = _filt(np.abs(x * y), g)
    mu1sq, mu2sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    D = (fxx - mu1sq) + (fyy - mu2sq) + C2
    cs = (2.0 * (fxy - mu12) + C2) / D
    lum = (2.0 * mu12 + C1) / (mu1sq + mu2sq + C1)
    ss = lum * cs
    e_cs = U32 * (2.0 * (axy + np.abs(mu12)) + np.abs(cs) * (fxx + fyy + mu1sq + mu2sq) + np.abs(cs) * D) / D
    e_ss = np.abs(lum) * e_cs + 4.0 * U32 * np.abs(ss)
    return {"cs": cs, "ss": ss, "e_cs": e_cs, "e_ss": e_ss}


def pooled_shape(H, W):
    return (H + 2 * (H % 2) - 2) // 2 + 1, (W + 2 * (W % 2) - 2) // 2 + 1


def _quads(a):
    """The four addends of every 2x2 window, padding = size % 2 with zeros: (0,0), (0,1), (1,0), (1,1)."""
    H, W = a.shape[-2:]
    ph, pw = H % 2, W % 2
    Ho, Wo = pooled_shape(H, W)
    p = np.pad(a, [(0, 0)] * (a.ndim - 2) + [(ph, ph), (pw, pw)])[..., :2 * Ho, :2 * Wo]
    return p[..., 0::2, 0::2], p[..., 0::2, 1::2], p[..., 1::2, 0::2], p[..., 1::2, 1::2]


def pool64(a) -> np.ndarray:
    """2x2 average pooling, padding = size % 2, zeros counted (count_include_pad), in float64."""
    q = _quads(f64(a))
    return 0.25 * (((q[0] + q[1]) + q[2]) + q[3])


def env_pool(a) -> np.ndarray:
    """Three float32 additions, each bounded by the sum of the magnitudes; the factor 1/4 is exact."""
    return 3.0 * U32 * pool64(np.abs(f64(a)))


def pool32(a, clamp=False) -> np.ndarray:
    """The same in float32, in the kernels' documented order (((a+b)+c)+d)*0.25f; the clamp to [0,1] comes first.
    Both GPU pools must equal it bit for bit (inputs of -0.0 aside: a padded sum starts from +0)."""
    a = np.asarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a)
    assert a.dtype == np.float32
    if clamp:
        a = np.clip(a, np.float32(0.0), np.float32(1.0))
    q = _quads(a)
    out = (((q[0] + q[1]) + q[2]) + q[3]) * np.float32(0.25)
    assert out.dtype == np.float32
    return out


def _finalize_terms(means, weights, relu_last):
    means = f64(means)
    L, P, _ = means.shape
    w = np.asarray(weights, dtype=np.float32).astype(np.float64)   # the kernel reads float32 weights
    assert w.shape == (L,)
    v = np.where((np.arange(L) == L - 1)[:, None], means[..., 1], means[..., 0])   # [L, P]
    relu = np.ones(L, dtype=bool)
    relu[L - 1] = bool(relu_last)
    v = np.where(relu[:, None], np.maximum(v, 0.0), v)
    return v, w


def finalize64(means, weights, relu_last, B, C):
    """means [levels, B*C, 2] (mean cs, mean ssim) -> (out [B], envelope [B]):  out[b] = mean_c prod_l v_l^w_l with
    v_l = relu(cs) below the last level and ssim (relu'd when relu_last) at it; one level without relu is the plain
    mean (no power: the value may be negative).

    Envelope, one float32 half-ulp per rounded operation of an fp32 evaluation: per factor the rounding of the float64
    mean to float32 (which the power scales by w_l), the power and the multiplication into the product (w_l + 2);
    then C additions into the channel sum and the division (each bounded by the sum of the magnitudes)."""
    v, w = _finalize_terms(means, weights, relu_last)
    L = v.shape[0]
    if L == 1 and not relu_last:
        prod = v[0]
        per = np.abs(prod) * 1.0                                # the rounding to float32 only
    else:
        with np.errstate(invalid="ignore"):
            prod = np.prod(np.power(v, w[:, None]), axis=0)
        per = np.abs(prod) * float(np.sum(w + 2.0))
    prod, per = prod.reshape(B, C), per.reshape(B, C)
    out = prod.mean(axis=1)
    env = U32 * (per.sum(axis=1) + (C + 1) * np.abs(prod).sum(axis=1)) / C
    return out, env


def finalize32(means, weights, relu_last, B, C) -> np.ndarray:
    """float32 numpy restatement of the same evaluation (the host anchor of the finalize envelope)."""
    v, w = _finalize_terms(means, weights, relu_last)
    v32, w32 = v.astype(np.float32), w.astype(np.float32)
    L = v.shape[0]
    out = np.zeros(B, dtype=np.float32)
    for b in range(B):
        acc = np.float32(0.0)
        for c in range(C):
            prod = np.float32(1.0)
            for l in range(L):
                t = v32[l, b * C + c]
                prod = np.float32(prod * (t if (L == 1 and not relu_last) else np.power(t, w32[l])))
            acc = np.float32(acc + prod)
        out[b] = np.float32(acc / np.float32(C))
    return out


def sqerr64(a, b, clamp_a=False):
    """Per-image sum of (a - b)^2 over everything but the first axis -> (sum [B], envelope [B]).  An fp32 evaluation
    rounds the difference (which the square doubles) and the square: 3 half-ulps of every addend; the sum itself is
    accumulated in float64."""
    x, y = f64(a), f64(b)
    if clamp_a:
        x = np.clip(x, 0.0, 1.0)
    d2 = ((x - y) ** 2).reshape(x.shape[0], -1)
    s = d2.sum(axis=1)
    return s, 3.0 * U32 * s


def sqerr32(a, b, clamp_a=False) -> np.ndarray:
    """float32 differences and squares, float64 sum (the host anchor of the sqerr envelope)."""
    x, y = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    if clamp_a:
        x = np.clip(x, np.float32(0.0), np.float32(1.0))
    d = (x - y).astype(np.float32)
    return (d * d).astype(np.float32).astype(np.float64).reshape(x.shape[0], -1).sum(axis=1)


def finalize_means(levels, B, C, seed) -> np.ndarray:
    """Hand-made means [levels, B*C, 2] for the finalize tests: values in [0.3, 1), with a plane at exactly 1, one at
    exactly 0, a negative cs below the last level and a negative ssim at the last level planted on planes of their
    own where there are that many."""
    rng = np.random.default_rng(seed)
    P = B * C
    m = rng.uniform(0.3, 1.0, (levels, P, 2))
    m[:, 0, :] = 1.0
    m[levels // 2, 1 % P, :] = 0.0
    m[0, 2 % P, 0] = -0.125
    m[levels - 1, 3 % P, 1] = -0.25
    return m


FINALIZE_WEIGHTS = {1: (1.0,), 3: (0.3, 0.5, 0.2), 5: (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)}
FINALIZE_CASES = [(levels, B, C) for levels in (1, 3, 5) for B in (1, 3, 70) for C in (1, 3, 4)]
SQERR_CASES = [(B, n) for B in (1, 5) for n in (1, 100, 255, 256, 257, 3 * 176 * 203)]


def sqerr_inputs(B, n, seed):
    """a leaves [0,1] (for clamp_a), b stays inside."""
    rng = np.random.default_rng(seed)
    a = (rng.random((B, n)) * 1.4 - 0.2).astype(np.float32)
    b = rng.random((B, n)).astype(np.float32)
    return a, b


KINDS = ("ramp", "out_of_range", "anti", "flat")


def make_inputs(planes, H, W, seed, kind="ramp"):
    """Deterministic float32 planes (X, Y), each [planes, H, W].

    "ramp": one white texture T in [0,1) and one noise field N in [-1/2, 1/2) shared by the planes, and a parameter
    p = (plane + 1) / planes distinct per plane.  X = T (1 - 0.3 p) + 0.15 p (in [0,1], mean 1/2),
    Y = X (1 - 0.2 col p) + 0.1 row + amp N with amp = 0.04 + 0.3 p (0.5 + 0.5 row col), row and col in [0,1].  The
    per-plane means fall monotonically with p (the noise grows, the gain leaves 1), so a wrong plane of either image
    moves them; the gradients along both axes move them under a transposed axis, and a read shifted by a pixel
    decorrelates X from Y.  Every pixel's cs and ssim stay near 1, so each counts in the mean.
    "out_of_range": the same with both images stretched out of [0,1] (for clamp_x: X is clamped, Y is not).
    "anti": Y = 1 - X: cs means near -1.
    "flat": constant planes, X at 1, 0.5, 0 in turn and Y one step on: sigma = 0, D = C2, the largest envelope."""
    assert kind in KINDS, kind
    rng = np.random.default_rng(seed)
    T = 0.5 - 0.5 * np.cos(np.pi * rng.random((H, W)))           # arcsine law: the most variance a [0,1] texture has
    N = rng.random((H, W)) - 0.5
    row = (np.arange(H, dtype=np.float64) / max(H - 1, 1))[:, None]
    col = (np.arange(W, dtype=np.float64) / max(W - 1, 1))[None, :]
    p = ((np.arange(planes, dtype=np.float64) + 1.0) / planes)[:, None, None]
    X = T * (1.0 - 0.3 * p) + 0.15 * p
    amp = np.sqrt(0.01 + 0.2 * p * (0.5 + 0.5 * row * col))
    Y = X * (1.0 - 0.2 * col * p) + 0.1 * row + amp * N
    Y = np.maximum(Y, 0.0)
    if kind == "out_of_range":
        X, Y = 1.5 * X - 0.25, 1.3 * Y - 0.1
    elif kind == "anti":
        Y = 1.0 - X
    elif kind == "flat":
        vals = np.array([1.0, 0.5, 0.0])
        X = np.broadcast_to(vals[np.arange(planes) % 3][:, None, None], (planes, H, W))
        Y = np.broadcast_to(vals[(np.arange(planes) + 1) % 3][:, None, None], (planes, H, W))
    return np.ascontiguousarray(X, dtype=np.float32), np.ascontiguousarray(Y, dtype=np.float32)


# (planes, H, W) of tests/test_gpu_metrics_levels.py by the branch of ssim_level_kernel each exists for; the kinds
# beyond "ramp" and the clamp cases are chosen there
LEVEL_CASES = {
    "four planes per wave": [(13, 12, 64), (7, 18, 40), (5, 27, 61), (1, 11, 11)],
    "two planes per wave": [(2, 20, 128), (3, 21, 100), (3, 24, 66)],
    "one strip of 256": [(2, 30, 256), (3, 37, 250), (2, 11, 256), (1, 64, 11)],
    "several strips": [(3, 35, 300), (3, 28, 496), (2, 28, 492), (3, 40, 740), (2, 26, 498), (2, 30, 500),
                       (1, 32, 1000), (2, 64, 520)],
    "bands above 8 rows": [(600, 150, 64)],
}
CLAMP_CASES = [(7, 18, 40), (3, 24, 66), (3, 37, 250), (3, 28, 496), (600, 150, 64)]   # one per branch
KIND_CASES = [(7, 18, 40), (3, 28, 496)]                                                # "anti" and "flat"


def all_level_cases():
    """[(family, (planes, H, W), kind, clamp_x)] - every level case of the suite."""
    out = []
    for fam, cases in LEVEL_CASES.items():
        for c in cases:
            out.append((fam, c, "ramp", 0))
            if c in CLAMP_CASES:
                out.append((fam, c, "out_of_range", 1))
            if c in KIND_CASES:
                out.append((fam, c, "anti", 0))
                out.append((fam, c, "flat", 0))
    return out


def case_seed(case):
    planes, H, W = case
    return 7919 * planes + 131 * H + W
