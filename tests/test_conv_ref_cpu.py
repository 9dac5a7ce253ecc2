"""Anchors of tests/conv_ref.py, on the CPU: the float64 references against independent evaluations, the Winograd
mappings against the direct ones, the recorded emulation peaks R behind the GPU bars against a fresh measurement on
the GPU test's own inputs, every bar against its derived ceiling, and the power of the split bar: four mutant
emulations of the two-plane contraction must each exceed it."""
import math

import pytest
import torch
import torch.nn.functional as F

import conv_ref as R


def _rel(a, b, E):
    return float(((a - b).abs() / E).max())


# ------------------------------------------------------------------------------- float64 values, two ways

def _conv_unfold(x, w, b, k, stride):
    B, Ci, H, W = x.shape
    cols = F.unfold(x, kernel_size=k, padding=(k - 1) // 2, stride=stride)
    y = torch.einsum("bnt,on->bot", cols, w.reshape(w.shape[0], -1))
    return y.view(B, -1, -(-H // stride), -(-W // stride)) + b.view(1, -1, 1, 1)


def _convT_scatter(x, w, b):
    """Every input pixel adds its 5x5 stamp at (2i - 2, 2j - 2); rows and columns 0 .. 2H - 1 are kept."""
    B, Ci, H, W = x.shape
    full = x.new_zeros(B, w.shape[1], 2 * H + 3, 2 * W + 3)
    for ky in range(5):
        for kx in range(5):
            full[:, :, ky:ky + 2 * H:2, kx:kx + 2 * W:2] += torch.einsum("bchw,co->bohw", x, w[:, :, ky, kx])
    return full[:, :, 2:2 * H + 2, 2:2 * W + 2] + b.view(1, -1, 1, 1)


SMALL = [c for c in R.ALL_CASES if c.H * c.W <= 160 and c.Cin <= 192]


@pytest.mark.parametrize("c", SMALL, ids=R.case_id)
def test_float64_values_two_ways(c):
    for kind in R.kinds_of(c):
        inp, v, E = R.reference(c, kind)
        x, w, b = R.x_as_float64(inp["x"]), inp["w"].double(), inp["b"].double()
        if c.op == "ct":
            other = _convT_scatter(x, w, b)
            E_dir = F.conv_transpose2d(x.abs(), w.abs(), b.abs(), stride=2, padding=2, output_padding=1)
        else:
            k = w.shape[-1]
            other = _conv_unfold(x, w, b, k, 1 if k == 3 else 2)
            E_dir = F.conv2d(x.abs(), w.abs(), b.abs(), stride=1 if k == 3 else 2, padding=(k - 1) // 2)
        assert other.shape == v.shape
        assert _rel(other, v, E_dir) <= 1e-13, (kind, _rel(other, v, E_dir))
        if R.is_wino(c):
            # the Winograd mapping (3x3, space-to-depth, four phases) in float64 is the same function
            y = R.evaluate(c.op, x, w, b, "f64", True)
            assert _rel(y, v, E_dir) <= 1e-13, (kind, _rel(y, v, E_dir))
            assert bool((E >= E_dir * (1 - 1e-12)).all())          # E_win never below E_dir
        else:
            assert _rel(E, E_dir, E_dir) <= 1e-13


def test_activation_envelope():
    g = torch.Generator().manual_seed(3)
    v = (torch.rand((1, 5, 4, 6), generator=g, dtype=torch.float64) * 2 - 1) * 6
    beta, gamma = 0.5 + torch.rand(5, generator=g), 0.02 + 0.28 * torch.rand(5, generator=g)
    e = torch.full_like(v, 1e-4)
    for act in ("none", "relu", "gdn", "igdn"):
        f0 = R.act64(v, act, beta, gamma)
        env = R.act_envelope(v, e, act, beta, gamma)
        for s in (-1.0, -0.37, 0.51, 1.0):
            moved = (R.act64(v + s * e, act, beta, gamma) - f0).abs()
            assert bool((moved <= env).all()), act
    # closed forms of f' against a central difference (h = 1e-5: truncation 1e-10 f''', rounding 1e-11)
    h = 1e-5
    for act, form in (("gdn", lambda b, g_, a: b * (b + g_ * a * a) ** -1.5),
                      ("igdn", lambda b, g_, a: (b + 2 * g_ * a * a) / torch.sqrt(b + g_ * a * a))):
        d = (R.act64(v + h, act, beta, gamma) - R.act64(v - h, act, beta, gamma)) / (2 * h)
        want = form(beta.double().view(1, -1, 1, 1), gamma.double().view(1, -1, 1, 1), v)
        assert float((d - want).abs().max()) < 1e-8


# ------------------------------------------------------------------------------- the bars are measured here

@pytest.fixture(scope="module")
def peaks():
    """max |emulation - ref64| / E per (family, contraction, kind) over every judged (case, kind)."""
    out, excluded, ranges = {}, 0, []
    for c, kind, contraction in R.judged_pairs():
        inp, v, E = R.reference(c, kind)
        excluded += int((E <= 0).sum())
        r = _rel(R.emulate(c, kind, contraction).double(), v, E)
        key = (R.family(c), contraction, kind)
        out[key] = max(out.get(key, 0.0), r)
        if kind == "range" and contraction == R.contractions(c)[0]:
            ranges.append((R.case_id(c), float(v.abs().min()), float(v.abs().max())))
    return out, excluded, ranges


def test_recorded_peaks(peaks):
    measured, excluded, _ = peaks
    assert excluded == 0                                          # E > 0: every element is judged
    print("R_LOG2 = {")
    for key in sorted(measured):
        print(f"    {key!r}: {math.log2(measured[key]):.3f},")
    print("}")
    assert set(measured) == set(R.R_LOG2), "conv_ref.R_LOG2 must hold exactly the judged (family, contraction, kind)"
    for key, m in sorted(measured.items()):
        print(f"{key}: measured peak 2^{math.log2(m):.3f}, recorded R 2^{R.R_LOG2[key]:.3f}")
        # the recorded value IS the measurement: the sums run in a fixed order (conv_ref._mm32), so what is left to the
        # host is the order inside a block of four terms and the float64 reference's own rounding
        assert abs(math.log2(m) - R.R_LOG2[key]) <= 0.05, (key, math.log2(m), R.R_LOG2[key])


def test_bars_below_their_ceilings():
    """The GPU bar of every judged case: K_GPU * R, or the ceiling where that is lower (said here)."""
    capped = set()
    for c, kind, contraction in R.judged_pairs():
        n = R.contraction_length(c)
        b, ceil_ = R.bar(R.family(c), contraction, kind, n), R.ceiling(contraction, n)
        assert 0 < b <= ceil_
        if b == ceil_:
            capped.add((R.family(c), contraction, kind, n))
    for fam, contraction, kind, n in sorted(capped):
        print(f"bar = ceiling 2^{math.log2(R.ceiling(contraction, n)):.2f} (K_GPU R = "
              f"2^{math.log2(R.K_GPU * R.R(fam, contraction, kind)):.2f}): {fam} {contraction} {kind} n={n}")
    for key in sorted(R.R_LOG2):
        print(f"{key}: K_GPU R = 2^{math.log2(R.K_GPU * R.R(*key)):.2f}")


def test_range_inputs_span_the_range(peaks):
    _, _, ranges = peaks
    assert ranges
    for name, lo, hi in ranges:
        assert lo * 256.0 <= hi, (name, lo, hi)


# ------------------------------------------------------------------------------- the bar has power

WINO_CASES = [c for c in R.WINO32_CASES + R.WINO64_CASES if "split" in R.contractions(c)]


@pytest.mark.parametrize("op", ["c3", "c5", "ct"])
def test_mutants_exceed_the_split_bar(op):
    """Each mutant emulation, on the GPU test's own inputs of the mapping, is over the split bar on at least one
    judged element of at least one input kind; the global-maximum bar of test_gpu_conv.py is printed beside it."""
    worst = {m: 0.0 for m in R.MUTANTS}
    old = []
    for c in (c for c in WINO_CASES if c.op == op):
        for kind in R.kinds_of(c):
            inp, v, E = R.reference(c, kind)
            b = R.bar("wino", "split", kind, R.contraction_length(c))
            old.append(24.0 * R.old_bar_factor(c, v, E, b))
            for m in R.MUTANTS:
                worst[m] = max(worst[m], _rel(R.emulate(c, kind, m).double(), v, E) / b)
    for m, r in worst.items():
        print(f"{op} {m}: worst error / split bar {r:.2f}")
    old.sort()
    print(f"{op}: the global-maximum bar sits {old[0]:.0f}x .. {old[-1]:.0f}x (median {old[len(old) // 2]:.0f}x) above "
          f"the median per-element bar")
    assert all(r > 1.0 for r in worst.values()), worst
