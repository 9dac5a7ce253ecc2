"""Chunk-major (CM16, [B][C/16][H][W][16]) activations: every kernel that reads or writes them computes the same bits
as its NHWC path on the same inputs - only the addresses change."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from dsic_amd import layers as _layers
    from dsic_amd import ops as _ops
    if not _layers.wino_bf16():
        pytest.fail("chunk-major activations belong to the split-bf16 kernels (DSIC_WINO_BF16=1, the default)")
    return _ops


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(shape, generator=g) * 2 - 1) * scale).cuda()


def _gdn(seed, C=128):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(C, generator=g) + 0.5).cuda(), (torch.rand(C, generator=g) * 0.2).cuda()


def _same(ops, y_cm, y_nhwc):
    assert torch.equal(ops.cm16_to_nhwc(y_cm), y_nhwc)


def test_layout_conversions_roundtrip(ops):
    x = _rand((2, 8, 8, 64), 1)
    cm = ops.nhwc_to_cm16(x)
    assert cm.shape == (2, 4, 8, 8, 16)
    assert torch.equal(cm[1, 2, 3, 4], x[1, 3, 4, 32:48])
    assert torch.equal(ops.cm16_to_nhwc(cm), x)


@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("s2d", [True, False])
def test_first_layer_chunk_major_output(ops, u8, s2d):
    B, H, W = 2, 64, 48
    w, bias = _rand((128, 3, 3, 3), 2, 0.3), _rand((128,), 3, 0.1)
    beta, gamma = _gdn(4)
    if u8:
        g = torch.Generator().manual_seed(5)
        x = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8).cuda()
    else:
        x = _rand((B, 3, H, W), 5).abs()
    ref = ops.conv_first_nchw(x, w, bias, ops.ACT_GDN, beta, gamma, s2d_out=s2d)
    got = ops.conv_first_nchw(x, w, bias, ops.ACT_GDN, beta, gamma, s2d_out=s2d, cm_out=True)
    torch.cuda.synchronize()
    _same(ops, got, ref)


@pytest.mark.parametrize("s2d_out", [False, True])
@pytest.mark.parametrize("H,W", [(64, 64), (32, 48)])
def test_conv3x3_chunk_major_in_and_out(ops, H, W, s2d_out):
    B, C = 2, 128
    assert ops._lib.load().dsic_wino_bf16_m64(H, W, C, 1)
    x = _rand((B, H, W, C), 10)
    u = ops.split_wino_weight_bf16(ops.pack_wino_weight(_rand((C, C, 3, 3), 11, 0.05)), C, C, 1)
    bias = _rand((C,), 12, 0.1)
    beta, gamma = _gdn(13)
    ref = ops.conv3x3_wino_nhwc(x, u, bias, C, ops.ACT_GDN, beta, gamma, s2d_out=s2d_out)
    xc = ops.nhwc_to_cm16(x)
    for cm_in, cm_out in ((True, False), (False, True), (True, True)):
        got = ops.conv3x3_wino_nhwc(xc if cm_in else x, u, bias, C, ops.ACT_GDN, beta, gamma, s2d_out=s2d_out,
                                    cm_in=cm_in, cm_out=cm_out)
        torch.cuda.synchronize()
        if cm_out:
            _same(ops, got, ref)
        else:
            assert torch.equal(got, ref)


@pytest.mark.parametrize("s2d_out", [False, True])
def test_conv5x5_s2_over_space_to_depth_chunk_major(ops, s2d_out):
    B, Cs, H2, W2 = 2, 128, 32, 32
    x = _rand((B, H2, W2, 4 * Cs), 20)
    u = ops.split_wino_weight_bf16(ops.pack_wino_s2_weight(_rand((128, Cs, 5, 5), 21, 0.03)), 128, 4 * Cs, 1)
    bias = _rand((128,), 22, 0.1)
    beta, gamma = _gdn(23)
    ref = ops.conv3x3_wino_nhwc(x, u, bias, 128, ops.ACT_GDN, beta, gamma, s2d_in=True, s2d_out=s2d_out)
    got = ops.conv3x3_wino_nhwc(ops.nhwc_to_cm16(x), u, bias, 128, ops.ACT_GDN, beta, gamma, s2d_in=True,
                                s2d_out=s2d_out, cm_in=True, cm_out=True)
    torch.cuda.synchronize()
    _same(ops, got, ref)


def test_conv_transpose_chunk_major_in_and_out(ops):
    B, Cin, Cout, H, W = 2, 128, 128, 16, 32
    x = _rand((B, H, W, Cin), 30)
    u = ops.split_wino_weight_bf16(ops.pack_wino_convT_weight(_rand((Cin, Cout, 5, 5), 31, 0.03)), Cout, Cin, 4)
    bias = _rand((Cout,), 32, 0.1)
    beta, gamma = _gdn(33)
    ref = ops.conv_transpose2d_wino_nhwc(x, u, bias, Cout, ops.ACT_IGDN, beta, gamma)
    xc = ops.nhwc_to_cm16(x)
    for cm_in, cm_out in ((True, False), (False, True), (True, True)):
        got = ops.conv_transpose2d_wino_nhwc(xc if cm_in else x, u, bias, Cout, ops.ACT_IGDN, beta, gamma,
                                             cm_in=cm_in, cm_out=cm_out)
        torch.cuda.synchronize()
        if cm_out:
            _same(ops, got, ref)
        else:
            assert torch.equal(got, ref)


def test_chunk_major_needs_the_64_tile_kernel(ops):
    x = ops.nhwc_to_cm16(_rand((1, 16, 16, 128), 40))   # one 16x16 tile per image: the 32-tile kernel's layer
    u = ops.split_wino_weight_bf16(ops.pack_wino_weight(_rand((128, 128, 3, 3), 41, 0.05)), 128, 128, 1)
    with pytest.raises(ValueError, match="chunk-major"):
        ops.conv3x3_wino_nhwc(x, u, _rand((128,), 42), 128, cm_in=True)


def _chain_model():
    from dsic_amd import synthetic as S
    from dsic_amd.model import CompressionModel
    sd = S.make_state_dict(seed=3)
    m = CompressionModel(N=128, M=192, spatial_params=False, min_nu=2, max_nu=100.0)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m.cuda().eval()


def test_analysis_and_synthesis_chains_match_nhwc(ops, monkeypatch):
    """g_a.0 -> g_a.2 and every 64-tile edge of g_a / g_s: same outputs and taps at every level of layers.CHUNK_MAJOR.
    128x128 is the smallest size with 64-tile edges in both chains, 48x80 the smallest whose bottom layers run on the
    direct kernel."""
    from dsic_amd import layers, synthetic as S
    m = _chain_model()
    firsts = []
    real_first = ops.conv_first_nchw
    monkeypatch.setattr(ops, "conv_first_nchw", lambda *a, **k: firsts.append(k.get("cm_out")) or real_first(*a, **k))

    def run(x, cm):
        monkeypatch.setattr(layers, "CHUNK_MAJOR", cm)
        ta, ts = [], []
        y = m.g_a.forward_from_image(x, ta)
        xh = m.g_s.forward_nhwc(y[..., :192].contiguous(), ts)
        torch.cuda.synchronize()
        return y, xh, ta, ts

    for H, W in ((128, 128), (48, 80)):
        x = torch.from_numpy(S.make_patches(0, 2, H, W)).cuda()
        del firsts[:]
        y0, xh0, ta0, ts0 = run(x, 0)
        # g_a.2 reads the first layer's output as a space-to-depth map of 512 channels: chunk-major where that is a
        # 64-tile layer
        first_cm = True if (H, W) == (128, 128) else bool(ops._lib.load().dsic_wino_bf16_m64(H // 2, W // 2, 512, 1))
        for level in (1, 2):
            y1, xh1, ta1, ts1 = run(x, level)
            assert firsts == [False] + [first_cm] * level, (H, W, level)
            assert torch.equal(y0, y1) and torch.equal(xh0, xh1)
            assert len(ta0) == len(ta1) and len(ts0) == len(ts1)
            for a, b in zip(ta0 + ts0, ta1 + ts1):
                assert torch.equal(a, b)


def test_chains_give_the_same_bits_at_every_grid(ops):
    """The same chains with the Winograd kernels' persistent grid capped at 1 and at 3 workgroups
    (dsic_wino_grid), where a workgroup walks from work item to work item through every layer: the outputs of one
    tile leave during the next one's phases.  At the device's grid these sizes give a workgroup one item, two at
    the most.  Every edge of the plan in that state: the space-to-depth first edge, chunk-major in and out, the
    Cout slices of g_a.14, split-K.  Outputs and every tap equal the default grid's bit for bit."""
    from dsic_amd import synthetic as S
    m = _chain_model()
    L = ops._lib.load()

    def run(x):
        ta, ts = [], []
        y = m.g_a.forward_from_image(x, ta)
        xh = m.g_s.forward_nhwc(y[..., :192].contiguous(), ts)
        torch.cuda.synchronize()
        assert not bool(ops._ticket(x.device).any())
        return [y, xh] + ta + ts

    was = L.dsic_wino_grid(-1)
    try:
        for H, W in ((128, 128), (48, 80)):
            x = torch.from_numpy(S.make_patches(0, 2, H, W)).cuda()
            L.dsic_wino_grid(0)
            ref = run(x)
            assert len(ref) > 10 and all(bool(torch.isfinite(t).all()) for t in ref)
            for grid in (1, 3):
                assert L.dsic_wino_grid(grid) in (0, 1) and L.dsic_wino_grid(-1) == grid
                got = run(x)
                assert len(got) == len(ref)
                for i, (a, b) in enumerate(zip(got, ref)):
                    assert torch.equal(a, b), f"{H}x{W}, grid {grid}: tensor {i} of {len(ref)} (outputs, then taps) " \
                                              f"differs from the default grid's"
    finally:
        L.dsic_wino_grid(was)
