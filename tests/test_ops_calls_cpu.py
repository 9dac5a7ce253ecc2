"""The calls ops.py makes into the library, case by case, against a recording of them (tests/golden/ops_calls.json).

ops.py turns tensors into raw pointers and integers; the roofline figures of bench.py come from what it hands the
kernel timer.  Here lib.load() is replaced by a stand-in whose launch exports log their integer and float arguments
and which of their pointers are null, and return 0; the host predicates and size functions (dsic_wino_bf16_m64,
_ksplit, _planes, *_floats, *_bytes) go to the real library.  Tensors live on the meta device and say they are on the
GPU; _p, _stream, _ticket and the current-device query behind _f32c are patched, so no GPU is needed.  A timer
installed with set_kernel_timer logs (name, flops, exec_flops).

    python tests/test_ops_calls_cpu.py --record OUT.json [--root TREE]

writes the traces of TREE (default: this tree).  The stored file was recorded on the commit before the Winograd
wrappers of ops.py got one _timed call each and the pack wrappers one helper.
"""
import contextlib
import json
import os
import sys

import torch

META = torch.device("meta")
FORWARDED = ("dsic_wino_bf16_m64", "dsic_wino_bf16_ksplit", "dsic_wino_bf16_planes")


class _OnGpu(torch.Tensor):
    """A meta tensor that answers is_cuda like the device tensors ops.py insists on."""
    is_cuda = property(lambda self: True)


def T(*shape, dtype=torch.float32):
    return torch.empty(shape, dtype=dtype, device=META).as_subclass(_OnGpu)


def U8(*shape):
    return T(*shape, dtype=torch.uint8)


class _Library:
    def __init__(self, real, log):
        self._real, self._log = real, log

    def __getattr__(self, name):
        if name in FORWARDED or name.endswith(("_floats", "_bytes")):
            return getattr(self._real, name)

        def launch(*args):
            assert all(a is None or isinstance(a, (int, float, str)) for a in args), (name, args)
            self._log.append([name] + list(args))
            return 0
        return launch


class _Timer:
    def __init__(self, log):
        self.log = log

    def record(self, name, flops, launch, exec_flops):
        self.log.append(["timer", name, flops, exec_flops])
        return launch()


@contextlib.contextmanager
def _patched(ops, log, timer=True, splitk=True):
    from dsic_amd import lib
    saved = (lib.load, ops._p, ops._stream, ops._ticket, torch.cuda.current_device, ops.WINO_SPLITK, ops._kernel_timer)
    stand_in = _Library(lib.load(), log)
    try:
        lib.load = lambda: stand_in
        ops._p = lambda t: None if t is None else "p"
        ops._stream = lambda: "stream"
        ops._ticket = lambda device: torch.empty(2, dtype=torch.int64, device=META)
        torch.cuda.current_device = lambda: None          # a meta tensor's device index
        ops.WINO_SPLITK = splitk
        ops.set_kernel_timer(_Timer(log) if timer else None)
        yield
    finally:
        lib.load, ops._p, ops._stream, ops._ticket, torch.cuda.current_device, ops.WINO_SPLITK = saved[:6]
        ops.set_kernel_timer(saved[6])


def _cases(O):
    """{id: (function of nothing that makes the call, WINO_SPLITK)}"""
    out = {}

    def add(cid, fn, splitk=True):
        assert cid not in out, cid
        out[cid] = (fn, splitk)

    f32u, bf16u, bias, par = T(1000), U8(1000), T(128), T(128)

    # conv3x3_wino_nhwc
    for name, u in (("f32", f32u), ("bf16", bf16u)):
        # 64x64: 64-tile kernel; 20x36: ragged, 32-tile kernel; 16x16 and 8x8: split-K for the bf16 planes
        for H, W in ((64, 64), (20, 36), (16, 16), (8, 8)):
            for Cin in (128, 512):
                k = f"wino_{name}/{H}x{W}_Cin{Cin}"
                add(k, lambda u=u, H=H, W=W, Cin=Cin: O.conv3x3_wino_nhwc(T(2, H, W, Cin), u, bias, 128))
                add(k + "_gdn_s2d_out", lambda u=u, H=H, W=W, Cin=Cin: O.conv3x3_wino_nhwc(
                    T(2, H, W, Cin), u, bias, 128, O.ACT_GDN, par, par, s2d_out=True))
                add(k + "_s2d_in", lambda u=u, H=H, W=W, Cin=Cin: O.conv3x3_wino_nhwc(
                    T(2, H, W, Cin), u, bias, 96, O.ACT_RELU, s2d_in=True, algo_flops=1.5e9))
                add(k + "_s2d_in_out", lambda u=u, H=H, W=W, Cin=Cin: O.conv3x3_wino_nhwc(
                    T(2, H, W, Cin), u, bias, 128, s2d_in=True, s2d_out=True))
                add(k + "_slice", lambda u=u, H=H, W=W, Cin=Cin: O.conv3x3_wino_nhwc(
                    T(2, H, W, Cin), u, bias, 64, O.ACT_IGDN, par, par, out=T(2, H, W, 192), out_coff=128))
                add(k + "_out", lambda u=u, H=H, W=W, Cin=Cin: O.conv3x3_wino_nhwc(
                    T(2, H, W, Cin), u, bias, 128, out=T(2, H, W, 128), algo_flops=7.0))
                add(k + "_no_split_k", lambda u=u, H=H, W=W, Cin=Cin: O.conv3x3_wino_nhwc(
                    T(2, H, W, Cin), u, bias, 128, split_k=False))
                add(k + "_splitk_off", lambda u=u, H=H, W=W, Cin=Cin: O.conv3x3_wino_nhwc(
                    T(2, H, W, Cin), u, bias, 128), splitk=False)
                add(k + "_cm_in", lambda u=u, H=H, W=W, Cin=Cin: O.conv3x3_wino_nhwc(
                    T(2, Cin // 16, H, W, 16), u, bias, 128, cm_in=True))
                add(k + "_cm_out", lambda u=u, H=H, W=W, Cin=Cin: O.conv3x3_wino_nhwc(
                    T(2, H, W, Cin), u, bias, 128, O.ACT_GDN, par, par, cm_out=True))
                add(k + "_cm_in_out_s2d", lambda u=u, H=H, W=W, Cin=Cin: O.conv3x3_wino_nhwc(
                    T(2, Cin // 16, H, W, 16), u, bias, 128, s2d_in=True, s2d_out=True, cm_in=True, cm_out=True))
                add(k + "_cm_out_given", lambda u=u, H=H, W=W, Cin=Cin: O.conv3x3_wino_nhwc(
                    T(2, H, W, Cin), u, bias, 128, out=T(2, 8, H, W, 16), cm_out=True))
    add("wino/f16_input", lambda: O.conv3x3_wino_nhwc(T(2, 16, 16, 128, dtype=torch.float16), bf16u, bias, 128))
    add("wino/cpu_input", lambda: O.conv3x3_wino_nhwc(torch.empty(2, 16, 16, 128, device=META), bf16u, bias, 128))
    add("wino/cm_in_not_16", lambda: O.conv3x3_wino_nhwc(T(2, 8, 16, 16, 8), bf16u, bias, 128, cm_in=True))

    # conv_transpose2d_wino_nhwc
    for name, u in (("f32", f32u), ("bf16", bf16u)):
        for H, W in ((32, 32), (16, 16), (10, 18), (8, 8)):          # 16x16 is the smallest the 64-tile kernel takes
            for Cin in (128, 192):
                k = f"winoT_{name}/{H}x{W}_Cin{Cin}"
                add(k, lambda u=u, H=H, W=W, Cin=Cin: O.conv_transpose2d_wino_nhwc(T(2, H, W, Cin), u, bias, 128))
                add(k + "_igdn_out", lambda u=u, H=H, W=W, Cin=Cin: O.conv_transpose2d_wino_nhwc(
                    T(2, H, W, Cin), u, bias, 96, O.ACT_IGDN, par, par, out=T(2, 2 * H, 2 * W, 96)))
                add(k + "_cm_in", lambda u=u, H=H, W=W, Cin=Cin: O.conv_transpose2d_wino_nhwc(
                    T(2, Cin // 16, H, W, 16), u, bias, 128, cm_in=True))
                add(k + "_cm_out", lambda u=u, H=H, W=W, Cin=Cin: O.conv_transpose2d_wino_nhwc(
                    T(2, H, W, Cin), u, bias, 128, O.ACT_RELU, cm_out=True))
                add(k + "_cm_in_out", lambda u=u, H=H, W=W, Cin=Cin: O.conv_transpose2d_wino_nhwc(
                    T(2, Cin // 16, H, W, 16), u, bias, 128, cm_in=True, cm_out=True))

    # conv_first_nchw: uint8 NHWC bytes and float NCHW
    w3, w4 = T(128, 3, 3, 3), T(40, 4, 3, 3)
    for name, x3, x4 in (("u8", U8(2, 34, 50, 3), U8(2, 64, 64, 4)), ("f32", T(2, 3, 34, 50), T(2, 4, 64, 64))):
        for s2d in (False, True):
            for cm in (False, True):
                k = f"first_{name}/s2d{int(s2d)}_cm{int(cm)}"
                add(k, lambda x=x3, s2d=s2d, cm=cm: O.conv_first_nchw(x, w3, bias, O.ACT_GDN, par, par, s2d_out=s2d, cm_out=cm))
                add(k + "_4ch", lambda x=x4, s2d=s2d, cm=cm: O.conv_first_nchw(x, w4, bias, s2d_out=s2d, cm_out=cm))
    add("first/u8_cpu", lambda: O.conv_first_nchw(torch.empty((2, 8, 8, 3), dtype=torch.uint8, device=META), w3, bias))
    add("first/f32_cpu", lambda: O.conv_first_nchw(torch.empty((2, 3, 8, 8), device=META), w3, bias))
    add("first/f16", lambda: O.conv_first_nchw(T(2, 3, 8, 8, dtype=torch.float16), w3, bias))
    add("first/f16_weight", lambda: O.conv_first_nchw(T(2, 3, 8, 8), T(128, 3, 3, 3, dtype=torch.float16), bias))

    # the packers, each with a kernel it takes and one it refuses
    add("pack_conv_weight/3", lambda: O.pack_conv_weight(T(128, 3, 3, 3)))
    add("pack_conv_weight/5", lambda: O.pack_conv_weight(T(192, 128, 5, 5)))
    add("pack_conv_weight/1", lambda: O.pack_conv_weight(T(100, 36, 1, 1)))
    add("pack_conv_weight/3x5", lambda: O.pack_conv_weight(T(128, 3, 3, 5)))
    add("pack_conv_weight/cpu", lambda: O.pack_conv_weight(torch.empty(128, 3, 3, 3, device=META)))
    for name in ("pack_convT_weight", "pack_wino_convT_weight", "pack_wino_s2_weight"):
        add(f"{name}/5", lambda name=name: getattr(O, name)(T(192, 128, 5, 5)))
        add(f"{name}/5_odd", lambda name=name: getattr(O, name)(T(40, 100, 5, 5)))
        add(f"{name}/3", lambda name=name: getattr(O, name)(T(192, 128, 3, 3)))
        add(f"{name}/5x3", lambda name=name: getattr(O, name)(T(192, 128, 5, 3)))
        add(f"{name}/f16", lambda name=name: getattr(O, name)(T(192, 128, 5, 5, dtype=torch.float16)))
    add("pack_wino_weight/3", lambda: O.pack_wino_weight(T(128, 192, 3, 3)))
    add("pack_wino_weight/3_odd", lambda: O.pack_wino_weight(T(100, 36, 3, 3)))
    add("pack_wino_weight/5", lambda: O.pack_wino_weight(T(128, 192, 5, 5)))
    add("pack_wino_weight/3x1", lambda: O.pack_wino_weight(T(128, 192, 3, 1)))
    add("pack_convT_image_weight/3", lambda: O.pack_convT_image_weight(T(128, 3, 5, 5)))
    add("pack_convT_image_weight/4", lambda: O.pack_convT_image_weight(T(64, 4, 5, 5)))
    add("pack_convT_image_weight/k3", lambda: O.pack_convT_image_weight(T(128, 3, 3, 3)))
    add("pack_convT_image_weight/Cin_40", lambda: O.pack_convT_image_weight(T(40, 3, 5, 5)))
    add("pack_convT_image_weight/Cimg_5", lambda: O.pack_convT_image_weight(T(128, 5, 5, 5)))
    add("pack_convT_image_weight/Cimg_0", lambda: O.pack_convT_image_weight(T(128, 0, 5, 5)))
    add("split_wino_weight_bf16/1", lambda: O.split_wino_weight_bf16(T(1000), 128, 192))
    add("split_wino_weight_bf16/4", lambda: O.split_wino_weight_bf16(T(1000), 96, 128, 4))
    return out


def _flat(r):
    if isinstance(r, torch.Tensor):
        return [list(r.shape), str(r.dtype).replace("torch.", "")]
    return r


def trace_all(timer=True):
    """{case id: list of records} of the dsic_amd that is importable now."""
    from dsic_amd import ops
    traces = {}
    for cid, (fn, splitk) in _cases(ops).items():
        log = []
        with _patched(ops, log, timer, splitk):
            try:
                log.append(["returns", _flat(fn())])
            except Exception as e:     # a call ops.py refuses: nothing may have been launched before it
                log.append(["raises", type(e).__name__, str(e)])
        traces[cid] = [json.dumps(r, separators=(",", ":")) for r in log]
    return traces


def test_ops_calls_equal_the_recording(golden_dir):
    want = json.load(open(os.path.join(golden_dir, "ops_calls.json")))
    want = {cid: [json.dumps(r, separators=(",", ":")) for r in tr] for cid, tr in want.items()}
    got = trace_all()
    assert sorted(got) == sorted(want), "the case table and the recording differ: re-record"
    bad = [f"{cid}:\n  got      {got[cid]}\n  recorded {want[cid]}" for cid in got if got[cid] != want[cid]]
    assert not bad, f"{len(bad)} of {len(got)} cases differ; first ones:\n" + "\n".join(bad[:10])


def test_without_a_timer_the_same_launches_are_made():
    timed, plain = trace_all(), trace_all(timer=False)
    for cid, tr in timed.items():
        assert [r for r in tr if not r.startswith('["timer",')] == plain[cid], cid


def test_the_recording_covers_every_branch(golden_dir):
    """the case table is worth something only if the traces differ where the code has a choice"""
    want = json.load(open(os.path.join(golden_dir, "ops_calls.json")))
    recs = [r for tr in want.values() for r in tr]
    exports = {r[0] for r in recs}
    assert {"dsic_conv3x3_wino_nhwc", "dsic_conv3x3_wino_bf16_nhwc", "dsic_conv3x3_wino_bf16_splitk_nhwc",
            "dsic_conv_transpose2d_wino_nhwc", "dsic_conv_transpose2d_wino_bf16_layout", "dsic_conv_first_nchw",
            "dsic_conv_first_u8hwc", "dsic_pack_conv_weight", "dsic_pack_convT_weight", "dsic_pack_convT_image_weight",
            "dsic_pack_wino_weight", "dsic_pack_wino_s2_weight", "dsic_pack_wino_convT_weight",
            "dsic_split_wino_weight_bf16", "timer", "returns", "raises"} <= exports
    names = {r[1] for r in recs if r[0] == "timer"}
    assert {f"conv_wino{k}_kernel<{m}>" for k in ("", "_bf16", "_bf16m") for m in (0, 1, 2)} <= names
    assert {"conv_first_kernel<3>", "conv_first_kernel<4>"} <= names
    assert {r[1] for r in recs if r[0] == "raises"} >= {"ValueError", "RuntimeError", "TypeError", "AssertionError"}
    # split-K taken at 16x16 and 8x8, and refused by each of its three switches
    d = {cid: [r[0] for r in tr] for cid, tr in want.items()}
    for size in ("16x16", "8x8"):
        assert "dsic_conv3x3_wino_bf16_splitk_nhwc" in d[f"wino_bf16/{size}_Cin512"]
        for how in ("_no_split_k", "_splitk_off", "_cm_in"):
            assert "dsic_conv3x3_wino_bf16_nhwc" in d[f"wino_bf16/{size}_Cin512{how}"]


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", required=True, metavar="OUT.json")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import dsic_amd
    traces = {cid: [json.loads(r) for r in tr] for cid, tr in trace_all().items()}
    with open(a.record, "w") as f:
        json.dump(traces, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(f"{a.record}: {len(traces)} cases of {os.path.dirname(dsic_amd.__file__)}")
