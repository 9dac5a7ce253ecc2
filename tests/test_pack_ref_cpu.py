"""tests/pack_ref.py is checked before it judges a kernel (tests/test_gpu_weight_packers.py).

Contraction: every restated buffer is read back the way its consumer reads it (tap by tap for the two implicit-GEMM
forms and the image form; A^T [U (.) B^T d B] A for the three Winograd forms, bf16 planes summed back) and contracted in
float64 with a small random input.  The result is conv_ref.conv64 / convT64 of the ORIGINAL weights: to float64 rounding
where the buffer holds the weights themselves or the float64 U, and inside a derived bound where it holds rounded
values (float32 U: 5 * 2^-24 of the absolute-value evaluation, test_gpu_weight_packers.py holds the kernel to the same
bound; P bf16 planes: 2^-9P more).  This ties the restatement to the operation, not to the kernel's index arithmetic.
The padded input channels carry data, so a non-zero padding element shows; padded output columns must come out 0.

Mutants: on the GPU test's own inputs each named mutant of the restatement gives another buffer than the restatement,
at every shape where it is not the identity by construction, so a kernel with that defect cannot be bit-equal to it.

Sizes: the restated size functions against the library's (host-only calls) for every shape the GPU test uses.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_ref as R
import pack_ref as P

U64 = 2.0 ** -53
H, W = 6, 8          # input grid of the contraction checks: even (Winograd tiles, space-to-depth), not square


def _x(C, h=H, w=W, seed=5):
    g = torch.Generator().manual_seed(seed * 1000 + C)
    return (torch.rand((1, C, h, w), generator=g, dtype=torch.float64) * 2 - 1)


def _shift(x, dy, dx):
    """x [1,C,H,W] -> s with s[i][j] = x[i+dy][j+dx], zero outside."""
    _, _, h, w = x.shape
    p = F.pad(x, (2, 2, 2, 2))
    return p[:, :, 2 + dy:2 + dy + h, 2 + dx:2 + dx + w]


def _close(got, want, E, n, what, extra=0.0):
    """|got - want| <= (2 (n + 2) 2^-53 + extra) E element-wise: two float64 evaluations of an n-term sum whose
    absolute-value evaluation is E, and `extra` for what the buffer's values were rounded by."""
    tol = (2.0 * (n + 2) * U64 + extra) * E
    err = (got - want).abs()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert bool((err <= tol).all()), f"{what}: worst |error| / E = {float((err / E).max()):.3e}, allowed " \
                                     f"{2.0 * (n + 2) * U64 + extra:.3e}"


def _w_t(w):
    return torch.from_numpy(np.ascontiguousarray(w))


# ---------------------------------------------------------------------------------------------------- direct forms

@pytest.mark.parametrize("k,Cout,Cin", P.CONV_SHAPES)
def test_conv_buffer_contracts_to_the_convolution(k, Cout, Cin):
    w = P.weights("conv", (k, Cout, Cin))
    buf = P.pack_conv_weight(w, k)
    assert buf.dtype == np.float32 and buf.size == P.packed_conv_weight_floats(Cout, Cin, k)
    C8, CoutP = P.round_up(Cin, 8) // 8, P.round_up(Cout, 32)
    Wt = torch.from_numpy(buf.astype(np.float64)).view(k * k, C8, CoutP, 8).permute(0, 2, 1, 3).reshape(k * k, CoutP, C8 * 8)
    for stride in ((1,) if k == 1 else (1, 2)):
        x = _x(C8 * 8)                       # the padded channels carry data: a non-zero padding weight would show
        pad = (k - 1) // 2
        xp = F.pad(x, (pad, pad, pad, pad))
        Ho, Wo = -(-H // stride), -(-W // stride)
        y = torch.zeros(1, CoutP, Ho, Wo, dtype=torch.float64)
        for t in range(k * k):
            ky, kx = divmod(t, k)            # tap t = ky*k + kx reads input (s*oy + ky - pad, s*ox + kx - pad)
            xs = xp[:, :, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride]
            y += torch.einsum("nc,bchw->bnhw", Wt[t], xs)
        ref = F.conv2d(x[:, :Cin], R.f64(_w_t(w)), None, stride=stride, padding=pad)
        E = F.conv2d(x[:, :Cin].abs(), R.f64(_w_t(w)).abs(), None, stride=stride, padding=pad)
        if k != 1:
            assert torch.equal(ref, R.conv64(x[:, :Cin], _w_t(w), torch.zeros(Cout), k, stride))
        _close(y[:, :Cout], ref, E, Cin * k * k, f"conv k={k} s={stride}")
        assert bool((y[:, Cout:] == 0).all()), "padded columns must contract to exactly 0"


def _phase_out(parts, Cout):
    y = torch.zeros(1, Cout, 2 * H, 2 * W, dtype=torch.float64)
    for (py, px), v in parts.items():
        y[:, :, py::2, px::2] = v
    return y


@pytest.mark.parametrize("Cin,Cout", P.CONVT_SHAPES)
def test_convT_buffer_contracts_to_the_transposed_convolution(Cin, Cout):
    w = P.weights("convT", (Cin, Cout))
    buf = P.pack_convT_weight(w)
    assert buf.dtype == np.float32 and buf.size == P.packed_convT_weight_floats(Cout, Cin)
    CoutP = P.round_up(Cout, 32)
    Wt = torch.from_numpy(buf.astype(np.float64)).view(25, Cin // 8, CoutP, 8).permute(0, 2, 1, 3).reshape(25, CoutP, Cin)
    x = _x(Cin)
    parts = {p: torch.zeros(1, CoutP, H, W, dtype=torch.float64) for p in P.PHASES}
    # the geometry alone (which input a tap reads); which kernel element it holds is what the buffer must get right
    for T, (py, px, ty, tx, _, _) in enumerate(P.convT_taps()):
        parts[(py, px)] += torch.einsum("nc,bchw->bnhw", Wt[T], _shift(x, ty + py - 1, tx + px - 1))
    y = _phase_out(parts, CoutP)
    ref = R.convT64(x, _w_t(w), torch.zeros(Cout))
    E = R.convT64(x.abs(), _w_t(w).abs(), torch.zeros(Cout))
    _close(y[:, :Cout], ref, E, Cin * 9, "convT")
    assert bool((y[:, Cout:] == 0).all())


@pytest.mark.parametrize("Cin,Cimg", P.IMAGE_SHAPES)
def test_image_buffers_contract_to_the_transposed_convolution(Cin, Cimg):
    w = P.weights("image", (Cin, Cimg))
    first, second = P.pack_convT_image_weight(w, Cin, Cimg)
    assert first.dtype == np.float32 and second.dtype == np.uint16
    assert first.size + second.size // 2 == P.convT_image_weight_floats(Cin)
    C16 = Cin // 16
    W1 = torch.from_numpy(first.astype(np.float64)).view(9, C16, 16, 16).permute(0, 2, 1, 3).reshape(9, 16, Cin)
    pl = P.bf16_value(second.reshape(C16, 9, 2, 2, 16, 8)).astype(np.float64)          # [c16][t][plane][half][col][e]
    W2 = torch.from_numpy(pl.sum(axis=2)).permute(1, 3, 0, 2, 4).reshape(9, 16, Cin)    # [t][col][c16, half, e]
    x = _x(Cin)
    ref = R.convT64(x, _w_t(w), torch.zeros(Cimg))
    E = R.convT64(x.abs(), _w_t(w).abs(), torch.zeros(Cimg))
    # two roundings to 8 significant bits: |v - (hi + mid)| <= 2^-9 |v - hi| <= 2^-18 |v|
    for what, Wt, extra in (("fp32 block", W1, 0.0), ("hi + mid", W2, 2.0 ** -18)):
        cols = torch.zeros(1, 16, H, W, dtype=torch.float64)
        for t in range(9):
            wr, wc = divmod(t, 3)            # output (2i+py, 2j+px) reads input (i-1+wr, j-1+wc)
            cols += torch.einsum("nc,bchw->bnhw", Wt[t], _shift(x, wr - 1, wc - 1))
        y = _phase_out({p: cols[:, ph * Cimg:(ph + 1) * Cimg] for ph, p in enumerate(P.PHASES)}, Cimg)
        _close(y, ref, E, Cin * 9, f"image {what}", extra)
        assert bool((cols[:, 4 * Cimg:] == 0).all()), "columns >= 4*Cimg must be zero"
    # the planes are those of the fp32 block, value by value
    v = P.image_g(w, Cin, Cimg)
    hi, mid = R._planes(torch.from_numpy(v))
    got = P.bf16_value(second.reshape(C16, 9, 2, 2, 16, 8))
    want = torch.stack([hi, mid]).view(2, 9, 16, C16, 2, 8).permute(3, 1, 0, 4, 2, 5).numpy()
    assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


# ---------------------------------------------------------------------------------------------------- Winograd forms

def _wino_contract(x, U, absolute=False):
    """A^T [U (.) B^T d B] A in float64: x [1,Ci,H,W] (even H, W), U [16][Co][Ci] -> [1,Co,H,W]."""
    BT, AT = (torch.tensor(m, dtype=torch.float64) for m in (R._BT, R._AT))
    if absolute:
        BT, AT, x, U = BT.abs(), AT.abs(), x.abs(), U.abs()
    B, Ci, h, w = x.shape
    th, tw = h // 2, w // 2
    d = F.unfold(F.pad(x, (1, 1, 1, 1)), kernel_size=4, stride=2).view(B, Ci, 4, 4, th * tw)
    V = torch.einsum("ij,bcjkt,lk->ilbtc", BT, d, BT).reshape(16, B * th * tw, Ci)
    M = torch.bmm(V, U.transpose(1, 2)).view(4, 4, B, th, tw, U.shape[1])
    return torch.einsum("ij,jkbhwo,lk->bohiwl", AT, M, AT).reshape(B, U.shape[1], h, w)


def _wino_checks(what, bufs, Cout, Cin, nphase, x, ref):
    """bufs (U32, U64, A) in the packed layout; x the 3x3 layers' input; ref [1,Cout,...] what the phases must give."""
    u32, u64, A = bufs
    assert u32.dtype == np.float32 and u32.size == nphase * P.wino_weight_floats(Cout, Cin)
    CinP = P.round_up(Cin, 8)
    x = F.pad(x, (0, 0, 0, 0, 0, CinP - Cin), value=0.75)        # the padded channels carry data
    forms = [("U64", u64, 0.0, None), ("U32", u32, 5 * 2.0 ** -24, None)]
    if Cin % 32 == 0:
        for Pn in (2, 3):
            forms.append((f"{Pn} planes", u32, 5 * 2.0 ** -24 + 2.0 ** (-9 * Pn) * (1 + 5 * 2.0 ** -24), Pn))
    Aun = torch.from_numpy(P.unpack_wino(A, Cout, Cin, nphase))
    for name, buf, extra, Pn in forms:
        if Pn is None:
            U = P.unpack_wino(buf, Cout, Cin, nphase).astype(np.float64)
        else:
            bits = P.split_bf16(buf, Cout, Cin, nphase, Pn)
            assert bits.dtype == np.uint16 and bits.size * 2 == nphase * P.wino_bf16_weight_bytes(Cout, Cin, Pn)
            U = P.unsplit_bf16(bits, Cout, Cin, nphase, Pn).astype(np.float64).sum(axis=0)
        U = torch.from_numpy(U)
        ys = [_wino_contract(x, U[ph]) for ph in range(nphase)]
        Es = [_wino_contract(x, Aun[ph], absolute=True) for ph in range(nphase)]
        if nphase == 4:
            y, E = (_phase_out(dict(zip(P.PHASES, v)), U.shape[2]) for v in (ys, Es))
        else:
            y, E = ys[0], Es[0]
        # 16 positions x Cin terms, and the transforms' own roundings
        _close(y[:, :Cout], ref, E[:, :Cout], 16 * Cin + 32, f"{what} {name}", extra)
        assert bool((y[:, Cout:] == 0).all()), f"{what} {name}: padded columns must contract to exactly 0"


@pytest.mark.parametrize("Cout,Cin", P.WINO_SHAPES)
def test_wino_buffer_contracts_to_the_convolution(Cout, Cin):
    w = P.weights("wino", (Cout, Cin))
    x = _x(Cin)
    _wino_checks("wino", P.pack_wino_weight(w), Cout, Cin, 1, x, R.conv64(x, _w_t(w), torch.zeros(Cout), 3, 1))


@pytest.mark.parametrize("Cout,Cs", P.WINO_S2_SHAPES)
def test_wino_s2_buffer_contracts_to_the_strided_convolution(Cout, Cs):
    w = P.weights("wino_s2", (Cout, Cs))
    x = _x(Cs, 2 * H, 2 * W)
    X, _ = R.s2d_operands(x, R.f64(_w_t(w)))                      # the space-to-depth image of the input
    _wino_checks("wino_s2", P.pack_wino_s2_weight(w), Cout, 4 * Cs, 1, X, R.conv64(x, _w_t(w), torch.zeros(Cout), 5, 2))


@pytest.mark.parametrize("Cin,Cout", P.WINO_CONVT_SHAPES)
def test_wino_convT_buffer_contracts_to_the_transposed_convolution(Cin, Cout):
    w = P.weights("wino_convT", (Cin, Cout))
    x = _x(Cin)
    _wino_checks("wino_convT", P.pack_wino_convT_weight(w), Cout, Cin, 4, x, R.convT64(x, _w_t(w), torch.zeros(Cout)))


@pytest.mark.parametrize("export", ["wino", "wino_s2", "wino_convT"])
def test_float32_U_is_inside_the_bound_the_kernel_is_held_to(export):
    """|U32 - U64| <= 5 * 2^-24 A: four roundings (two per pass, the second pass acting on rounded rows) and their
    second-order terms; the padding is zero in all three."""
    for shape in P.EXPORTS[export][0]:
        u32, u64, A = {"wino": P.pack_wino_weight, "wino_s2": P.pack_wino_s2_weight,
                       "wino_convT": P.pack_wino_convT_weight}[export](P.weights(export, shape))
        assert np.all(np.abs(u32.astype(np.float64) - u64) <= 5 * 2.0 ** -24 * A)
        assert np.all((A == 0) <= (u32.view(np.uint32) == 0)), "where A is 0 the element is +0.0"


# ---------------------------------------------------------------------------------------------------- the split

def test_bf16_rounding_is_round_to_nearest_even():
    v = np.concatenate([P.handmade_values(), P.weights("wino", (36, 32)).reshape(-1)])
    for Pn in (2, 3):
        pl = P.bf16_value(P.planes(v, Pn))
        rem = torch.from_numpy(v)
        for q in range(Pn):
            want = rem.bfloat16().float()                         # torch's conversion: round to nearest even
            assert np.array_equal(pl[q].view(np.uint32), want.numpy().view(np.uint32)), q
            rem = rem - want
    hi, mid = R._planes(torch.from_numpy(v))
    pl = P.bf16_value(P.planes(v, 2))
    assert np.array_equal(pl[0].view(np.uint32), hi.numpy().view(np.uint32))
    assert np.array_equal(pl[1].view(np.uint32), mid.numpy().view(np.uint32))


def test_handmade_values_are_what_their_description_says():
    v = P.handmade_values()
    bits = v.view(np.uint32)
    assert bits[0] == 0 and bits[1] == 0x80000000
    low = bits & 0xFFFF
    exact = v[(low == 0) & (v != 0)]
    assert exact.size >= 8 and np.all(P.planes(exact, 2)[1] == 0), "an exact bf16 value leaves mid = +0"
    ties = bits[low == 0x8000]
    up = (ties >> 16) & 1
    assert set(up.tolist()) == {0, 1} and {int(b >> 31) for b in ties} == {0, 1}, "ties of both parities and signs"
    assert np.array_equal(P.bf16_rne(ties.view(np.float32)), ((ties >> 16) + up).astype(np.uint16))
    rem = v - P.bf16_value(P.bf16_rne(v))
    rties = rem.view(np.uint32)[(rem.view(np.uint32) & 0xFFFF) == 0x8000]
    assert {int((b >> 16) & 1) for b in rties} == {0, 1} and {int(b >> 31) for b in rties} == {0, 1}, \
        "remainders that tie, of both parities and signs"
    a = np.abs(v[v != 0])
    assert a.min() >= 2.0 ** -20 and a.max() < 2.0 ** 11 and np.all(np.isfinite(v))
    assert set(np.floor(np.log2(a)).astype(int).tolist()) >= set(range(-20, 11))
    # the remainder is exact: hi + mid + lo gives v back wherever 24 bits suffice
    pl = P.bf16_value(P.planes(v, 3)).astype(np.float64)
    assert np.all(np.abs(pl.sum(axis=0) - v) <= 2.0 ** -26 * np.abs(v))


@pytest.mark.parametrize("Cout,Cin,nphase", P.SPLIT_SHAPES)
def test_split_layout_reads_back(Cout, Cin, nphase):
    for name, u in P.split_inputs(Cout, Cin, nphase).items():
        assert u.size == nphase * P.wino_weight_floats(Cout, Cin)
        for Pn in (2, 3):
            bits = P.split_bf16(u, Cout, Cin, nphase, Pn)
            back = P.unsplit_bf16(bits, Cout, Cin, nphase, Pn)
            want = P.bf16_value(P.planes(P.unpack_wino(u, Cout, Cin, nphase), Pn))
            assert np.array_equal(back.view(np.uint32), want.view(np.uint32)), name
            # one position of the layout by hand: [ph][pos][chunk][plane][n][16]
            ph, pos, n, c, q = nphase - 1, 13, Cout - 1, Cin - 5, Pn - 1
            CoutP = P.round_up(Cout, 32)
            i = ((((ph * 16 + pos) * (Cin // 16) + c // 16) * Pn + q) * CoutP + n) * 16 + c % 16
            assert bits[i] == P.planes(P.unpack_wino(u, Cout, Cin, nphase)[ph, pos, n, c], Pn)[q]
            assert np.all(back[:, :, :, Cout:] == 0) and not np.any(np.signbit(back[:, :, :, Cout:]))


# ---------------------------------------------------------------------------------------------------- mutants

MUTANTS = {
    "conv": ("padding",),
    "convT": ("swap", "phases", "forward", "padding"),
    "wino": ("padding",),
    "wino_s2": ("padding",),
    "wino_convT": ("swap", "phases", "forward", "padding"),
    "image": ("swap", "phases", "forward", "padding", "truncate", "mid_from_v", "half_col"),
}


def _identity_by_construction(export, shape, mutant):
    if mutant == "padding":
        if export == "image":
            return shape[1] == 4                                  # 16 columns, all real
        Cout, Cin = {"conv": lambda k, o, i: (o, i), "convT": lambda i, o: (o, i), "wino": lambda o, i: (o, i),
                     "wino_s2": lambda o, cs: (o, 4 * cs), "wino_convT": lambda i, o: (o, i)}[export](*shape)
        return Cout % 32 == 0 and Cin % 8 == 0
    return export == "image" and mutant == "swap" and shape[1] == 1   # [Cin][1] read as [1][Cin] is the same tensor


def _flat(b):
    return np.concatenate([x.view(np.uint8) for x in b]) if isinstance(b, tuple) else b.view(np.uint8)


@pytest.mark.parametrize("export", sorted(MUTANTS))
def test_every_mutant_differs_on_the_gpu_tests_inputs(export):
    for mutant in MUTANTS[export]:
        told = 0
        for shape in P.EXPORTS[export][0]:
            w = P.weights(export, shape)
            same = np.array_equal(_flat(P.restate(export, shape, w)), _flat(P.restate(export, shape, w, mutant)))
            if _identity_by_construction(export, shape, mutant):
                assert same, (export, shape, mutant)
                continue
            assert not same, f"{export} {shape}: the inputs cannot tell the mutant '{mutant}' from the restatement"
            told += 1
        assert told, f"{export}: no shape can show the mutant '{mutant}'"


@pytest.mark.parametrize("Cout,Cin,nphase", P.SPLIT_SHAPES)
def test_every_split_mutant_differs_on_the_gpu_tests_inputs(Cout, Cin, nphase):
    for name, u in P.split_inputs(Cout, Cin, nphase).items():
        for Pn in (2, 3):
            want = P.split_bf16(u, Cout, Cin, nphase, Pn)
            for mutant in ("truncate", "mid_from_v"):
                assert not np.array_equal(want, P.split_bf16(u, Cout, Cin, nphase, Pn, mutant)), (name, Pn, mutant)
    # the hand-made block alone tells truncation apart at the ties, and a mid taken from v at the exact values
    ties = P._f32_bits(0x3F818000, 0xBF818000)
    assert np.all(P.planes(ties, 2)[0] != P.planes(ties, 2, "truncate")[0])
    assert np.all(P.planes(np.float32([1.0, -1.5]), 2, "mid_from_v")[1] != 0)


def test_weights_are_fixed_and_no_index_exchange_maps_them_onto_themselves():
    w = P.weights("wino_convT", (32, 64))
    assert np.array_equal(w, P.weights("wino_convT", (32, 64))) and abs(float(w.mean())) < 0.05
    sq = P.make_weights((16, 16, 5, 5), 3)
    assert not np.array_equal(sq, sq.transpose(1, 0, 2, 3)) and not np.array_equal(sq, sq[:, :, ::-1, ::-1])
    flat = sq.reshape(256, 25)
    assert len({tuple(r) for r in flat.tolist()}) == 256, "no two (c0, c1) kernels are equal"


# ---------------------------------------------------------------------------------------------------- sizes

def test_size_functions_equal_the_librarys():
    from dsic_amd import lib
    L = lib.load()
    Pn = int(L.dsic_wino_bf16_planes())
    assert Pn in (2, 3)
    for k, Cout, Cin in P.CONV_SHAPES:
        assert L.dsic_packed_conv_weight_floats(Cout, Cin, k) == P.packed_conv_weight_floats(Cout, Cin, k)
    for Cin, Cout in P.CONVT_SHAPES:
        assert L.dsic_packed_conv_weight_floats(Cout, Cin, 5) == P.packed_convT_weight_floats(Cout, Cin)
    for Cout, Cin in P.WINO_SHAPES + [(o, 4 * cs) for o, cs in P.WINO_S2_SHAPES] + [(o, i) for i, o in P.WINO_CONVT_SHAPES]:
        assert L.dsic_wino_weight_floats(Cout, Cin) == P.wino_weight_floats(Cout, Cin)
    for Cout, Cin, _ in P.SPLIT_SHAPES:
        assert L.dsic_wino_bf16_weight_bytes(Cout, Cin) == P.wino_bf16_weight_bytes(Cout, Cin, Pn)
    for Cin, _ in P.IMAGE_SHAPES:
        assert L.dsic_convT_image_weight_floats(Cin) == P.convT_image_weight_floats(Cin)
