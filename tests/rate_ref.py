"""Float64 reference of the rate tail (csrc/hyper_rate.hip): Student-t / Gaussian bits, the hyper-parameter heads and
GDN, each with the error envelope an fp32 evaluation of the same formula is entitled to.

A helper for tests/test_rate_ref_cpu.py (which anchors it against scipy, mpmath, the fp32 oracle and the reference's
recorded fixture) and tests/test_gpu_rate_tail.py (which holds the kernels to it element by element).  It restates
the formulas of distributions.py:20-31,39-46, layers.py:19-27,131-139,147-151 and model.py:54-55 in torch float64; it
shares no code with the oracle or the product package.

Inputs are taken as they are (float32 tensors are widened exactly), so a comparison measures the arithmetic of the
implementation under test and not the rounding of its inputs.  The clamp bounds are the float32 values of 1e-3, 1e3,
2 and 100: those are the bounds every fp32 implementation compares against (only 1e-3 is inexact, by 4.7e-8).
"""
from __future__ import annotations

import math

import numpy as np
import torch

U32 = 2.0 ** -24                     # float32 unit roundoff: half an ulp, relative
LOG2E = 1.0 / math.log(2.0)
SIGMA_MIN, SIGMA_MAX = float(np.float32(1e-3)), float(np.float32(1e3))
NU_MIN, NU_MAX = 2.0, 100.0
K_ORACLE = 8.0                       # cap the fp32 oracle meets on the host (test_rate_ref_cpu.py measures it)
K_GPU = 16.0                         # twice that: device log1pf/logf/expf are specified to 1-2 ulp, the host's < 1


def f64(t) -> torch.Tensor:
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(t)
    if not isinstance(t, torch.Tensor):
        return torch.as_tensor(t, dtype=torch.float64)         # python scalars must not pass through float32
    return t.detach().cpu().to(torch.float64)


def _student_terms(x, sigma, nu):
    x, sigma, nu = f64(x), f64(sigma), f64(nu)
    sigma = sigma.clamp(SIGMA_MIN, SIGMA_MAX)
    nu = nu.clamp(NU_MIN, NU_MAX)
    a = (nu + 1.0) / 2.0
    logC = torch.lgamma(a) - torch.lgamma(nu / 2.0) - 0.5 * torch.log(nu * math.pi) - torch.log(sigma)
    q = x / sigma
    L = torch.log1p(q * q / nu)
    return logC, a, L


def student_bits64(x, sigma, nu) -> torch.Tensor:
    """-log2 of the Student-t density (location 0, scale sigma, nu degrees of freedom), sigma and nu clamped."""
    logC, a, L = _student_terms(x, sigma, nu)
    return -(logC - a * L) * LOG2E


def env_student(x, sigma, nu) -> torch.Tensor:
    """One float32 half-ulp of every term that enters the result: logC, the product a*L, and a itself (an ulp of the
    log1p argument moves L by up to that much, and L is multiplied by a)."""
    logC, a, L = _student_terms(x, sigma, nu)
    return U32 * (logC.abs() + a * L + a) * LOG2E


def _gauss_terms(x, log_sigma):
    x = f64(x)
    sigma = torch.exp(f64(log_sigma)).clamp(SIGMA_MIN, SIGMA_MAX)
    var = sigma * sigma
    return 0.5 * torch.log(2.0 * math.pi * var), 0.5 * x * x / var


def gauss_bits64(x, log_sigma) -> torch.Tensor:
    """-log2 of the zero-mean normal density with sigma = clamp(exp(log_sigma)); log_sigma broadcasts against x."""
    lt, qt = _gauss_terms(x, log_sigma)
    return (lt + qt) * LOG2E


def env_gauss(x, log_sigma) -> torch.Tensor:
    """Half an ulp of the log term, of the quadratic term, and of 1 (a relative error of sigma moves log sigma by
    that much absolutely)."""
    lt, qt = _gauss_terms(x, log_sigma)
    return U32 * (lt.abs() + qt + 1.0) * LOG2E


def channel_log_sigma(log_sigma, ndim=4):
    """[C] -> [1,C,1,1]: how the factorised prior broadcasts over an NCHW tensor."""
    return f64(log_sigma).view(1, -1, *([1] * (ndim - 2)))


def _gamma(n):
    return n * U32


def hyper_params64(t, w1s, b1s, w2s, b2s, w1n, b1n, w2n, b2n, min_nu, max_nu):
    """Mean over pixels, then the two ReLU-MLP heads (sigma, nu), exp and the nu clamp, in float64.

    t: [B,HW,N] (or [B,H,W,N]); weights input-major, w1* [N][N], w2* [N][M].
    Returns (values, bounds): dicts with log_sigma, log_nu, sigma, nu, each [B,M].  bounds[k] is an absolute bound on
    |fp32 result - values[k]| for any fp32 evaluation of the same expression, in any summation order, with or without
    fused multiply-adds: the standard forward-error bound gamma_n * sum|w_i||h_i| (gamma_n = n * 2^-24, n = the
    roundings a term can pass through: its product and one addition per input and the bias), propagated through both
    layers; the pooling contributes HW * 2^-24 * mean|t| (HW - 1 additions and the division).  The bound of a log
    output is, to first order, the relative bound of its exponential; expf adds 4 * 2^-24 (2 ulp).  The clamp is
    1-Lipschitz, so nu keeps the bound of exp(log_nu).
    """
    t = f64(t)
    if t.dim() == 4:
        t = t.reshape(t.shape[0], -1, t.shape[-1])
    B, HW, N = t.shape
    pooled = t.mean(dim=1)                                     # [B,N]
    e_pool = _gamma(HW) * t.abs().mean(dim=1)
    min_nu, max_nu = float(np.float32(min_nu)), float(np.float32(max_nu))   # the kernel takes them as float
    values, bounds = {}, {}
    for head, (w1, b1, w2, b2) in (("sigma", (w1s, b1s, w2s, b2s)), ("nu", (w1n, b1n, w2n, b2n))):
        w1, b1, w2, b2 = f64(w1), f64(b1), f64(w2), f64(b2)
        assert w1.shape == (N, N) and w2.shape[0] == N, (w1.shape, w2.shape)
        pre = pooled @ w1 + b1                                 # [B,N]
        e_pre = _gamma(N + 1) * (pooled.abs() @ w1.abs() + b1.abs()) + e_pool @ w1.abs()
        hid = pre.clamp(min=0.0)                               # ReLU is 1-Lipschitz: e_pre carries over
        out = hid @ w2 + b2                                    # [B,M]
        e_out = _gamma(N + 1) * (hid.abs() @ w2.abs() + b2.abs()) + e_pre @ w2.abs()
        ex = torch.exp(out)
        e_ex = (e_out + 4.0 * U32) * ex
        values["log_" + head], bounds["log_" + head] = out, e_out
        if head == "nu":
            values["nu_unclamped"], bounds["nu_unclamped"] = ex, e_ex
            ex = ex.clamp(min_nu, max_nu)
        values[head], bounds[head] = ex, e_ex
    return values, bounds


def gdn64(x, beta, gamma, inverse) -> torch.Tensor:
    """x / sqrt(beta_c + gamma_c x^2), or x * sqrt(...) for the inverse; x is [B,C,...], beta and gamma are the
    effective (reparametrised) per-channel values [C]."""
    x = f64(x)
    shape = (1, -1) + (1,) * (x.dim() - 2)
    d = torch.sqrt(f64(beta).view(shape) + f64(gamma).view(shape) * x * x)
    return x * d if inverse else x / d
