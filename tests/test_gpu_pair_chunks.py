"""The 64-tile Winograd kernel with the half-empty pass-B chunks paired (csrc/conv_wino_pair.h) writes the same bits
as with every chunk in a chunk-pass of its own: every accumulator receives the same products in the same order.
The unpaired side is the schedule that tests/test_gpu_conv_elements.py holds to float64, at the device's grid (one
work item per workgroup) and with the persistent grid capped at 1, 2 and 3 workgroups (dsic_wino_grid), where a
workgroup walks from item to item.  The B = 2 cases run here at those caps too: at one workgroup the items follow
each other in ticket order, a transposed layer's four phases - four lengths of pass B, four pairing starts - in
turn."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from dsic_amd import layers as _layers
    from dsic_amd import ops as _ops
    if not _layers.wino_bf16():
        pytest.fail("the paired schedule belongs to the split-bf16 kernels (DSIC_WINO_BF16=1, the default)")
    L = _ops._lib.load()
    was, grid_was = L.dsic_wino_pair_chunks(-1), L.dsic_wino_grid(-1)
    yield _ops
    L.dsic_wino_pair_chunks(was)
    L.dsic_wino_grid(grid_was)


def _rand(shape, seed, scale=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.rand(shape, generator=g, device="cuda") * 2 - 1) * scale


def _gdn(seed, C):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(C, generator=g) + 0.5).cuda(), (torch.rand(C, generator=g) * 0.2).cuda()


def _both_schedules(ops, run, grids=(0,)):
    """run(act, cm) -> output; every activation and both layouts, paired against unpaired, at every cap of the
    persistent grid in grids (0: the device's grid, first); the unpaired bits do not depend on the grid."""
    L = ops._lib.load()
    assert grids[0] == 0
    grid_was = L.dsic_wino_grid(-1)
    try:
        for act in (ops.ACT_GDN, ops.ACT_IGDN, ops.ACT_NONE):
            for cm in (False, True):
                first = None
                for grid in grids:
                    L.dsic_wino_grid(grid)
                    assert L.dsic_wino_grid(-1) == grid
                    assert L.dsic_wino_pair_chunks(0) in (0, 1)
                    plain = run(act, cm)
                    assert L.dsic_wino_pair_chunks(1) == 0
                    paired = run(act, cm)
                    assert L.dsic_wino_pair_chunks(-1) == 1
                    torch.cuda.synchronize()
                    assert bool(torch.isfinite(plain).all()) and float(plain.abs().max()) > 0
                    assert torch.equal(paired, plain), (act, cm, grid)
                    if first is None:
                        first = plain
                    assert torch.equal(plain, first), (act, cm, grid)
    finally:
        L.dsic_wino_grid(grid_was)


def _grids(B):
    """The B = 2 cases also with the grid capped at 1 and 3 workgroups; B = 80 is for the device's grid."""
    return (0, 1, 3) if B == 2 else (0,)


# (B, grid, Cs).  32x32: four tiles per image, all at the image border; 48x48: nine, one interior.  Cs = 32: eight
# chunks, blocks of two - a single chunk next to a pair, a pair at a block boundary; Cs = 128: the flagship's 32.
# B = 80: 320 tiles on 256 workgroups, so some run two tiles back to back (the prefetch across the tile boundary
# behind a shorter pass B).
@pytest.mark.parametrize("B,G,Cs", [(2, 32, 32), (2, 32, 128), (2, 48, 32), (80, 32, 32), (80, 32, 128)])
def test_conv5x5_s2_over_space_to_depth(ops, B, G, Cs):
    Cout = 128
    assert ops._lib.load().dsic_wino_bf16_m64(G, G, 4 * Cs, 1)
    x = _rand((B, G, G, 4 * Cs), 100 + Cs)
    xc = ops.nhwc_to_cm16(x)
    u = ops.split_wino_weight_bf16(ops.pack_wino_s2_weight(_rand((Cout, Cs, 5, 5), 101, 0.03)), Cout, 4 * Cs, 1)
    bias = _rand((Cout,), 102, 0.1)
    beta, gamma = _gdn(103, Cout)
    _both_schedules(ops, lambda act, cm: ops.conv3x3_wino_nhwc(xc if cm else x, u, bias, Cout, act, beta, gamma,
                                                              s2d_in=True, cm_in=cm, cm_out=cm),
                    _grids(B))


# (B, input size, Cin).  16x16: one tile per image, its four phase items; 48x48: an interior tile; B = 80: 320 items on
# 256 workgroups - a workgroup's second item follows one of another phase, i.e. of another length.
@pytest.mark.parametrize("B,G,Cin", [(2, 16, 64), (2, 16, 128), (2, 48, 64), (80, 16, 128)])
def test_conv_transpose(ops, B, G, Cin):
    Cout = 128
    assert ops._lib.load().dsic_wino_bf16_m64(G, G, Cin, 4)
    x = _rand((B, G, G, Cin), 200 + Cin)
    xc = ops.nhwc_to_cm16(x)
    u = ops.split_wino_weight_bf16(ops.pack_wino_convT_weight(_rand((Cin, Cout, 5, 5), 201, 0.03)), Cout, Cin, 4)
    bias = _rand((Cout,), 202, 0.1)
    beta, gamma = _gdn(203, Cout)
    _both_schedules(ops, lambda act, cm: ops.conv_transpose2d_wino_nhwc(xc if cm else x, u, bias, Cout, act, beta, gamma,
                                                                       cm_in=cm, cm_out=cm),
                    _grids(B))


def test_conv3x3_is_untouched(ops):
    B, G, C = 2, 32, 128
    assert ops._lib.load().dsic_wino_bf16_m64(G, G, C, 1)
    x = _rand((B, G, G, C), 300)
    xc = ops.nhwc_to_cm16(x)
    u = ops.split_wino_weight_bf16(ops.pack_wino_weight(_rand((C, C, 3, 3), 301, 0.05)), C, C, 1)
    bias = _rand((C,), 302, 0.1)
    beta, gamma = _gdn(303, C)
    _both_schedules(ops, lambda act, cm: ops.conv3x3_wino_nhwc(xc if cm else x, u, bias, C, act, beta, gamma,
                                                              cm_in=cm, cm_out=cm))
