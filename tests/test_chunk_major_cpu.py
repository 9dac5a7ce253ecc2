"""Chunk-major (CM16) layout plumbing on the host: the conversions the taps use and the edges the chains choose."""
import torch

from dsic_amd import layers, ops


def test_cm16_roundtrip_and_element_order():
    x = torch.arange(2 * 4 * 6 * 48, dtype=torch.float32).view(2, 4, 6, 48)
    cm = ops.nhwc_to_cm16(x)
    assert cm.shape == (2, 3, 4, 6, 16) and cm.is_contiguous()
    assert ops.cm16_shape(cm) == (2, 4, 6, 48)
    assert torch.equal(cm[1, 2, 3, 5], x[1, 3, 5, 32:48])
    assert torch.equal(ops.cm16_to_nhwc(cm), x)


def test_chunk_major_edges_of_the_analysis_transform():
    """At 256x256 every edge into a 64-tile layer is chunk-major except the one into the split-K layer g_a.14."""
    if not layers.wino_bf16():
        return
    mods = list(layers.AnalysisTransform(N=128, M=192).g_a)
    # (index of the consumer, its input size before space-to-depth, s2d)
    assert layers._Chain._wants_cm(mods, 2, 256, 256, True)       # g_a.0 -> g_a.2
    assert layers._Chain._wants_cm(mods, 4, 128, 128, False)      # g_a.2 -> g_a.4
    assert layers._Chain._wants_cm(mods, 6, 128, 128, True)       # g_a.4 -> g_a.6
    assert layers._Chain._wants_cm(mods, 12, 32, 32, False)       # g_a.10 -> g_a.12
    assert not layers._Chain._wants_cm(mods, 14, 32, 32, True)    # g_a.12 -> g_a.14 (split-K kernel)
    assert not layers._Chain._wants_cm(mods, 2, 32, 32, True)     # a 16x16 s2d grid: one tile per image
