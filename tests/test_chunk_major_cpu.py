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


def test_chunk_major_edges_of_the_analysis_transform(monkeypatch):
    """At 256x256 every edge into a 64-tile layer is chunk-major except the one into the split-K layer g_a.14."""
    if not layers.wino_bf16():
        return
    monkeypatch.setattr(layers, "CHUNK_MAJOR", 2)
    monkeypatch.setattr(layers, "USE_WINOGRAD", True)
    g_a = layers.AnalysisTransform(N=128, M=192).g_a
    K, Lay = layers.Kernel, layers.Layout
    plan = g_a.plan((2, 3, 256, 256), torch.float32, from_image=True)
    assert [st.conv for st in plan] == [g_a[i] for i in range(0, 16, 2)]
    out = [st.lay_out for st in plan]
    assert out[0] == Lay(s2d=True, cm=True)           # g_a.0 -> g_a.2
    assert out[1] == Lay(s2d=False, cm=True)          # g_a.2 -> g_a.4
    assert out[2] == Lay(s2d=True, cm=True)           # g_a.4 -> g_a.6
    assert out[3:6] == [Lay(False, True), Lay(True, True), Lay(False, True)]     # ... g_a.10 -> g_a.12, a 32x32 map
    assert out[6] == Lay(s2d=True, cm=False)          # g_a.12 -> g_a.14 (split-K kernel)
    assert out[7] == layers.NHWC
    assert [st.lay_in for st in plan] == [layers.NHWC] + out[:-1]
    assert [st.kernel for st in plan] == [K.FIRST] + [K.BF16_64] * 6 + [K.BF16_32]
    assert [st.act for st in plan] == [ops.ACT_GDN] * 7 + [ops.ACT_NONE]
    assert [st.gdn for st in plan] == [g_a[i] for i in range(1, 15, 2)] + [None]
    # a 16x16 s2d grid: one tile per image
    assert g_a.plan((2, 3, 32, 32), torch.float32, from_image=True)[0].lay_out == Lay(s2d=True, cm=False)
    # the levels of the switch: 1 keeps only the first layer's output chunk-major, 0 none
    monkeypatch.setattr(layers, "CHUNK_MAJOR", 1)
    assert [st.lay_out.cm for st in g_a.plan((2, 3, 256, 256), torch.float32, from_image=True)] == [True] + [False] * 7
    monkeypatch.setattr(layers, "CHUNK_MAJOR", 0)
    assert not any(st.lay_out.cm for st in g_a.plan((2, 3, 256, 256), torch.float32, from_image=True))
