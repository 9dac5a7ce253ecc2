"""The kernels of csrc/metrics.hip, export by export, against the float64 reference of tests/ssim_ref.py.

tests/test_gpu_metrics.py sees these kernels only through the final MS-SSIM scalar at 1e-4; here every per-plane
(mean cs, mean ssim) of one level is held to K_GPU envelopes of the float64 reference (the inputs are built so that a
single output pixel counted zero times or twice, or one plane read for another, cannot pass: test_ssim_ref_cpu.py),
the pooled planes are compared bit for bit with a float32 restatement, and the shapes walk every branch of
ssim_level_kernel: 4 / 2 / 1 planes per wave, one strip and several, vector and scalar loads, the fused 2x2 pool and
the separate one, ragged last bands.  Every output buffer carries 64 guard elements on each side and starts as NaN: an
element never written or a store outside the buffer fails the case.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import ssim_ref as R

pytestmark = pytest.mark.gpu

K_GPU = R.K_GPU
GUARD, SENTINEL = 64, -777.0
C1, C2 = (float(v) for v in R.constants())              # float32 values, as python floats for ctypes
_worst = {}                                                     # family -> largest |device - float64| / envelope


@pytest.fixture(scope="module")
def L():
    from dsic_amd import lib
    return lib.load()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Guarded:
    """n elements of NaN between two guards of 64 sentinels."""

    def __init__(self, n, dtype):
        self.n = int(n)
        self.buf = torch.full((self.n + 2 * GUARD,), float("nan"), dtype=dtype, device="cuda")
        self.buf[:GUARD] = SENTINEL
        self.buf[GUARD + self.n:] = SENTINEL
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + GUARD * self.buf.element_size())

    def take(self, what):
        """The written interior on the host; fails on a touched guard or an element left unwritten."""
        host = self.buf.cpu()
        assert bool((host[:GUARD] == SENTINEL).all()) and bool((host[GUARD + self.n:] == SENTINEL).all()), \
            f"{what}: a store outside the buffer"
        inner = host[GUARD:GUARD + self.n]
        bad = torch.isnan(inner).nonzero().flatten()
        assert bad.numel() == 0, f"{what}: {bad.numel()} of {self.n} elements never written, first at {int(bad[0])}"
        return inner.numpy()

    def untouched(self):
        host = self.buf.cpu()
        return bool((host[:GUARD] == SENTINEL).all()) and bool((host[GUARD + self.n:] == SENTINEL).all()) \
            and bool(torch.isnan(host[GUARD:GUARD + self.n]).all())


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _device(a, offset=0):
    """A float32 array on the device, `offset` floats past an aligned allocation."""
    flat = torch.empty(a.size + offset, dtype=torch.float32, device="cuda")
    flat[offset:] = torch.from_numpy(a).reshape(-1).cuda()
    view = flat[offset:]
    assert view.data_ptr() % 16 == 4 * offset
    return view


def _level(L, xd, yd, planes, H, W, clamp, pool):
    """One call of dsic_ssim_level (pool=False) or dsic_ssim_level_pool -> dict of host arrays."""
    nd = L.dsic_ssim_partial_doubles(planes, H, W)
    assert nd > 0 and nd % (2 * planes) == 0
    partial, means = Guarded(nd, torch.float64), Guarded(2 * planes, torch.float64)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    out = {}
    if pool:
        Hn, Wn = R.pooled_shape(H, W)
        xn, yn = Guarded(planes * Hn * Wn, torch.float32), Guarded(planes * Hn * Wn, torch.float32)
        rc = L.dsic_ssim_level_pool(p(xd), p(yd), partial.ptr, means.ptr, xn.ptr, yn.ptr, planes, H, W, C1, C2, clamp,
                                    _stream())
    else:
        rc = L.dsic_ssim_level(p(xd), p(yd), partial.ptr, means.ptr, planes, H, W, C1, C2, clamp, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    out["partial"] = partial.take("partial").reshape(planes, -1, 2)
    out["means"] = means.take("means").reshape(planes, 2)
    if pool:
        out["Xn"] = xn.take("Xn").reshape(planes, Hn, Wn)
        out["Yn"] = yn.take("Yn").reshape(planes, Hn, Wn)
    return out


def _avgpool(L, src_d, planes, H, W, clamp):
    Hn, Wn = R.pooled_shape(H, W)
    dst = Guarded(planes * Hn * Wn, torch.float32)
    rc = L.dsic_avgpool2(ctypes.c_void_p(src_d.data_ptr()), dst.ptr, planes, H, W, clamp, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return dst.take("avgpool2").reshape(planes, Hn, Wn)


@functools.lru_cache(maxsize=None)
def _reference(case, kind, clamp):
    """Inputs, float64 level and float32 pooled planes of a case: computed once, never modified."""
    X, Y = R.make_inputs(*case, R.case_seed(case), kind)
    ref = R.level64(X, Y, C1, C2, clamp)
    ref = {k: ref[k] for k in ("mean_cs", "mean_ss", "env_cs", "env_ss")}
    return X, Y, ref, R.pool32(X, clamp), R.pool32(Y)


def _ratio(means, ref):
    return max(float(np.max(np.abs(means[:, 0] - ref["mean_cs"]) / ref["env_cs"])),
               float(np.max(np.abs(means[:, 1] - ref["mean_ss"]) / ref["env_ss"])))


def _note(family, ratio):
    _worst[family] = max(_worst.get(family, 0.0), ratio)


LEVEL_PARAMS = R.all_level_cases()


@pytest.mark.parametrize("family,case,kind,clamp", LEVEL_PARAMS,
                         ids=[f"{c[0]}x{c[1]}x{c[2]}-{k}" for _, c, k, _ in LEVEL_PARAMS])
def test_level_vs_float64(L, family, case, kind, clamp):
    planes, H, W = case
    X, Y, ref, px, py = _reference(case, kind, clamp)
    n_out = (H - 10) * (W - 10)
    xd, yd = _device(X), _device(Y)
    plain = _level(L, xd, yd, planes, H, W, clamp, pool=False)
    pooled = _level(L, xd, yd, planes, H, W, clamp, pool=True)
    fused = bool(L.dsic_ssim_level_pool_fused(H, W))
    assert fused == (H % 2 == 0 and W % 4 == 0)
    # 1. every plane's two means inside the envelope of the float64 reference, with and without the pool
    for name, got in (("ssim_level", plain), ("ssim_level_pool", pooled)):
        ratio = _ratio(got["means"], ref)
        _note(family, ratio)
        print(f"{name} {case} {kind}: worst |device - float64| / envelope {ratio:.3f} "
              f"(envelope {float(ref['env_cs'].max()):.2e}, {'fused' if fused else 'separate'} pool)")
        assert ratio <= K_GPU, (name, ratio)
        # 2. the means are the partial sums in their fixed order, times 1 / (Ho Wo)
        total = np.zeros((planes, 2))
        for t in range(got["partial"].shape[1]):
            total = total + got["partial"][:, t, :]
        assert same_bits(total * (1.0 / float(n_out)), got["means"]), name
    # 3. the pooled planes bit for bit: X clamped when asked, Y never; the fused pass and dsic_avgpool2 agree
    assert same_bits(pooled["Xn"], px), _first_diff(pooled["Xn"], px)
    assert same_bits(pooled["Yn"], py), _first_diff(pooled["Yn"], py)
    assert same_bits(_avgpool(L, xd, planes, H, W, clamp), pooled["Xn"])
    assert same_bits(_avgpool(L, yd, planes, H, W, 0), pooled["Yn"])
    # 4. pointers one float past alignment: scalar loads and the separate pools
    xu, yu = _device(X, 1), _device(Y, 1)
    unaligned = _level(L, xu, yu, planes, H, W, clamp, pool=True)
    ratio = _ratio(unaligned["means"], ref)
    _note(family, ratio)
    print(f"unaligned {case} {kind}: worst |device - float64| / envelope {ratio:.3f}")
    assert ratio <= K_GPU, ratio
    assert same_bits(unaligned["Xn"], pooled["Xn"]) and same_bits(unaligned["Yn"], pooled["Yn"])
    # 5. run to run
    for pool, first in ((False, plain), (True, pooled)):
        again = _level(L, xd, yd, planes, H, W, clamp, pool)
        for k, v in first.items():
            assert same_bits(again[k], v), (pool, k)


def _first_diff(a, b):
    d = np.argwhere(_bits(a) != _bits(b))
    return f"{len(d)} elements differ, first at (plane, row, col) {tuple(d[0])}" if len(d) else "equal"


def test_level_ratios_reported():
    """Prints the largest ratio of each family seen by the cases above (run in file order)."""
    for fam, r in _worst.items():
        print(f"largest |device - float64| / envelope, {fam}: {r:.3f}")
    assert all(r <= K_GPU for r in _worst.values())


def test_planes_below_the_window_are_refused(L):
    from dsic_amd import lib
    for H, W in ((10, 64), (64, 10), (10, 10)):
        assert L.dsic_ssim_partial_doubles(3, H, W) == 0
    assert L.dsic_ssim_partial_doubles(0, 64, 64) == 0 and L.dsic_ssim_partial_doubles(3, 11, 11) > 0
    x = torch.zeros(3 * 64 * 64, device="cuda")
    for H, W in ((10, 64), (64, 10)):
        partial, means = Guarded(64, torch.float64), Guarded(6, torch.float64)
        xn, yn = Guarded(3 * 32 * 32, torch.float32), Guarded(3 * 32 * 32, torch.float32)
        p = ctypes.c_void_p(x.data_ptr())
        rc = L.dsic_ssim_level(p, p, partial.ptr, means.ptr, 3, H, W, C1, C2, 0, _stream())
        assert rc == lib.DSIC_EINVAL
        with pytest.raises(ValueError, match="smaller than the 11x11 window"):
            lib.check(rc, "ssim_level")
        rc = L.dsic_ssim_level_pool(p, p, partial.ptr, means.ptr, xn.ptr, yn.ptr, 3, H, W, C1, C2, 0, _stream())
        assert rc == lib.DSIC_EINVAL
        torch.cuda.synchronize()
        assert partial.untouched() and means.untouched() and xn.untouched() and yn.untouched()


@pytest.mark.parametrize("shape", [(3, 9, 13), (2, 10, 13), (2, 9, 12), (1, 1, 1), (5, 64, 64)])
@pytest.mark.parametrize("clamp", [0, 1])
def test_avgpool2_bit_exact(L, shape, clamp):
    rng = np.random.default_rng(sum(shape))
    a = (rng.random(shape) * 1.4 - 0.2).astype(np.float32)      # leaves [0,1] on both sides
    assert a.size < 4 or (a.min() < 0 and a.max() > 1)
    got = _avgpool(L, _device(a), *shape, clamp)
    want = R.pool32(a, bool(clamp))
    assert same_bits(got, want), _first_diff(got, want)


@pytest.mark.parametrize("levels,B,C", R.FINALIZE_CASES)
def test_finalize_vs_float64(L, levels, B, C):
    weights = R.FINALIZE_WEIGHTS[levels]
    means = R.finalize_means(levels, B, C, seed=100 * levels + 10 * B + C)
    md = torch.from_numpy(means).cuda()
    wd = torch.tensor(weights, dtype=torch.float32, device="cuda")
    for relu_last in ((0, 1) if levels == 1 else (1,)):
        out = Guarded(B, torch.float32)
        rc = L.dsic_msssim_finalize(ctypes.c_void_p(md.data_ptr()), ctypes.c_void_p(wd.data_ptr()), out.ptr, levels, B,
                                    C, relu_last, _stream())
        assert rc == 0
        torch.cuda.synchronize()
        got = out.take("finalize").astype(np.float64)
        want, env = R.finalize64(means, weights, relu_last, B, C)
        err = np.abs(got - want)
        ratio = max([0.0] + (err[env > 0] / env[env > 0]).tolist())
        print(f"finalize levels={levels} B={B} C={C} relu_last={relu_last}: worst error / envelope {ratio:.3f}")
        assert bool(np.all(err <= K_GPU * env)), (relu_last, int(np.argmax(err - K_GPU * env)))


def test_finalize_planted_values(L):
    """A negative last-level ssim gives exactly 0 with relu_last and passes through without it (one level); a negative
    cs below the last level zeroes the product; means of exactly 1 give exactly 1."""
    def run(means, weights, B, C, relu_last):
        md = torch.tensor(means, dtype=torch.float64, device="cuda").reshape(len(weights), B * C, 2)
        wd = torch.tensor(weights, dtype=torch.float32, device="cuda")
        out = Guarded(B, torch.float32)
        assert 0 == L.dsic_msssim_finalize(ctypes.c_void_p(md.data_ptr()), ctypes.c_void_p(wd.data_ptr()), out.ptr,
                                           len(weights), B, C, relu_last, _stream())
        torch.cuda.synchronize()
        return out.take("finalize")
    assert same_bits(run([[[0.5, -0.25]]], (1.0,), 1, 1, 1), np.array([0.0], dtype=np.float32))
    assert same_bits(run([[[0.5, -0.25]]], (1.0,), 1, 1, 0), np.array([-0.25], dtype=np.float32))
    w3 = R.FINALIZE_WEIGHTS[3]
    assert same_bits(run([[[-0.125, 0.9]], [[0.8, 0.9]], [[0.8, 0.9]]], w3, 1, 1, 1), np.array([0.0], dtype=np.float32))
    assert same_bits(run([[[0.7, 0.9]], [[0.8, 0.9]], [[0.8, -0.9]]], w3, 1, 1, 1), np.array([0.0], dtype=np.float32))
    assert same_bits(run([[[1.0, 1.0]] * 4] * 3, w3, 2, 2, 1), np.array([1.0, 1.0], dtype=np.float32))


@pytest.mark.parametrize("B,n", R.SQERR_CASES)
def test_sqerr_vs_float64(L, B, n):
    a, b = R.sqerr_inputs(B, n, seed=n + B)
    ad, bd = _device(a), _device(b)

    def run(x, y, clamp):
        out = Guarded(B, torch.float64)
        assert 0 == L.dsic_sqerr_per_image(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr()), out.ptr, B, n,
                                           clamp, _stream())
        torch.cuda.synchronize()
        return out.take("sqerr")
    for clamp in (0, 1):
        got = run(ad, bd, clamp)
        want, env = R.sqerr64(a, b, bool(clamp))
        ratio = float(np.max(np.abs(got - want) / env))
        print(f"sqerr B={B} n={n} clamp={clamp}: worst error / envelope {ratio:.3f}")
        assert ratio <= K_GPU, (clamp, ratio)
        assert same_bits(run(ad, bd, clamp), got)
    assert same_bits(run(ad, ad, 0), np.zeros(B))
    inside = _device(np.clip(a, np.float32(0), np.float32(1)))
    assert same_bits(run(ad, inside, 1), np.zeros(B))           # the clamp is applied to a, and only to a


@pytest.mark.parametrize("shape,weights", [((1, 3, 176, 992), (0.3, 0.5, 0.2)),             # level 1 is 88 x 496
                                           ((1, 1, 352, 1968), R.FINALIZE_WEIGHTS[5])])     # levels 1, 2: 984, 492 wide
def test_ms_ssim_end_to_end_through_the_suspected_widths(shape, weights):
    from dsic_amd import metrics
    B, C, H, W = shape
    X, Y = R.make_inputs(B * C, H, W, R.case_seed((B * C, H, W)), "ramp")
    xd, yd = torch.from_numpy(X).view(shape).cuda(), torch.from_numpy(Y).view(shape).cuda()
    got = metrics.ms_ssim(xd, yd, data_range=1.0, size_average=False, weights=weights).cpu().numpy().astype(np.float64)
    levels = metrics._levels(xd, yd, len(weights), 1.0, False).cpu().numpy()
    # float64 all the way: level64, pool64, finalize64, at the project's own bar
    a, b = X.astype(np.float64), Y.astype(np.float64)
    means = np.zeros((len(weights), B * C, 2))
    for lvl in range(len(weights)):
        ref = R.level64(a, b, C1, C2)
        means[lvl, :, 0], means[lvl, :, 1] = ref["mean_cs"], ref["mean_ss"]
        a, b = R.pool64(a), R.pool64(b)
    want, _ = R.finalize64(means, weights, 1, B, C)
    print(f"ms_ssim {shape}: device {got}, float64 {want}")
    assert float(np.max(np.abs(got - want))) < 1e-4
    # level by level on the planes the device pools (pool32 restates them bit for bit): inside the envelope
    a32, b32 = X, Y
    for lvl in range(len(weights)):
        ref = R.level64(a32, b32, C1, C2)
        ratio = _ratio(levels[lvl], ref)
        print(f"ms_ssim {shape} level {lvl} ({a32.shape[-2]} x {a32.shape[-1]}): |device - float64| / envelope {ratio:.3f}")
        assert ratio <= K_GPU, (lvl, ratio)
        a32, b32 = R.pool32(a32), R.pool32(b32)
