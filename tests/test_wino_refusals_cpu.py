"""What the six Winograd conv exports refuse, case by case, against a recording (tests/golden/wino_refusals.json).

The library loads without a GPU and checks every requirement on its arguments before its first HIP call, so a call
with dummy host pointers that breaks one requirement returns DSIC_EINVAL and a message, and touches nothing.  Each
case below is a valid call with exactly one requirement broken; the stored file holds status and message per case.

    python tests/test_wino_refusals_cpu.py --record OUT.json [--root TREE]

writes what the library of TREE (default: this tree) answers.  The stored file was recorded on the commit before the
three Winograd translation units got one shared set of layer checks; no case may be one that reaches a launch.
"""
import ctypes
import json
import os
import sys

PATTERN = bytes(range(64))

# argument names per export, in ABI order (include/dsic_hip.h)
_PTRS = ["in", "u", "bias", "beta", "gamma", "out"]
_GEO = ["B", "H", "W", "Cin", "Cout", "act"]
EXPORTS = {
    "dsic_conv3x3_wino_nhwc": _PTRS + _GEO + ["s2d_out", "s2d_in", "ticket", "stream"],
    "dsic_conv_transpose2d_wino_nhwc": _PTRS + _GEO + ["ticket", "stream"],
    "dsic_conv3x3_wino_bf16_nhwc": _PTRS + _GEO + ["s2d_out", "s2d_in", "out_cstride", "out_coff", "ticket", "stream"],
    "dsic_conv3x3_wino_bf16_splitk_nhwc": _PTRS + _GEO + ["s2d_out", "s2d_in", "out_cstride", "out_coff", "ksplit",
                                                          "partials", "ticket", "stream"],
    "dsic_conv_transpose2d_wino_bf16_nhwc": _PTRS + _GEO + ["ticket", "stream"],
    "dsic_conv_transpose2d_wino_bf16_layout": _PTRS + _GEO + ["layout_in", "layout_out", "ticket", "stream"],
}
SHORT = {"dsic_conv3x3_wino_nhwc": "f32", "dsic_conv_transpose2d_wino_nhwc": "f32T",
         "dsic_conv3x3_wino_bf16_nhwc": "bf16", "dsic_conv3x3_wino_bf16_splitk_nhwc": "splitk",
         "dsic_conv_transpose2d_wino_bf16_nhwc": "bf16T", "dsic_conv_transpose2d_wino_bf16_layout": "bf16L"}
POINTERS = {"in", "u", "bias", "beta", "gamma", "out", "ticket", "partials"}
# a call every export accepts: one 16x16 image, 128 -> 128 channels, no activation, NHWC, two-way split-K
VALID = {"B": 1, "H": 16, "W": 16, "Cin": 128, "Cout": 128, "act": 0, "s2d_out": 0, "s2d_in": 0, "out_cstride": 0,
         "out_coff": 0, "ksplit": 2, "layout_in": 0, "layout_out": 0, "stream": None}
CM16 = 2
F32 = ["dsic_conv3x3_wino_nhwc", "dsic_conv_transpose2d_wino_nhwc"]
BF16 = [e for e in EXPORTS if e not in F32]
CONV3 = ["dsic_conv3x3_wino_nhwc", "dsic_conv3x3_wino_bf16_nhwc", "dsic_conv3x3_wino_bf16_splitk_nhwc"]
SLICED = ["dsic_conv3x3_wino_bf16_nhwc", "dsic_conv3x3_wino_bf16_splitk_nhwc"]
SPLITK = "dsic_conv3x3_wino_bf16_splitk_nhwc"
PLAIN, LAYOUT = "dsic_conv3x3_wino_bf16_nhwc", "dsic_conv_transpose2d_wino_bf16_layout"


def cases():
    """[(id, export, {argument: value})]: the valid call with one requirement broken."""
    out = []

    def add(what, exports, **over):
        for e in exports:
            assert set(over) <= set(EXPORTS[e]), (what, e)
            out.append((f"{SHORT[e]}/{what}", e, over))

    for e in EXPORTS:
        for p in ("in", "u", "bias", "out", "ticket") + (("partials",) if e == SPLITK else ()):
            add(f"null_{p}", [e], **{p: None})
    for k in ("B", "H", "W"):
        add(f"empty_{k}", EXPORTS, **{k: 0})
    add("negative_B", EXPORTS, B=-1)
    add("Cin_0", F32, Cin=0)
    add("Cin_negative", EXPORTS, Cin=-32)
    add("Cin_48", EXPORTS, Cin=48)
    add("Cin_32", BF16, Cin=32)                      # the fp32 kernels take it
    add("Cin_80", BF16, Cin=80)
    add("Cout_0", EXPORTS, Cout=0)
    add("Cout_6", EXPORTS, Cout=6)
    add("Cout_132", EXPORTS, Cout=132)
    add("act_negative", EXPORTS, act=-1)
    add("act_4", EXPORTS, act=4)
    add("gdn_without_beta", EXPORTS, act=1, beta=None)
    add("igdn_without_gamma", EXPORTS, act=2, gamma=None)
    add("gdn_without_both", EXPORTS, act=1, beta=None, gamma=None)
    add("s2d_out_odd_H", CONV3, s2d_out=1, H=15)
    add("s2d_out_odd_W", CONV3, s2d_out=1, W=15)
    add("s2d_in_Cin_64", CONV3, s2d_in=1, Cin=64)
    add("s2d_in_Cin_192", CONV3, s2d_in=1, Cin=192)
    add("cm_in", ["dsic_conv3x3_wino_nhwc", SPLITK], s2d_in=CM16)
    add("cm_out", ["dsic_conv3x3_wino_nhwc", SPLITK], s2d_out=CM16)
    add("layout_in_1", [LAYOUT], layout_in=1)
    add("layout_out_3", [LAYOUT], layout_out=3)
    add("layout_in_negative", [LAYOUT], layout_in=-2)
    # chunk-major on layers the 64-tile kernel does not take: fewer than 4 work items, H not a multiple of 16
    add("cm_in_16x16", [PLAIN], s2d_in=CM16)
    add("cm_out_24x32", [PLAIN], s2d_out=CM16, H=24, W=32)
    add("cm_in_8x8", [LAYOUT], layout_in=CM16, H=8, W=8)
    add("cm_out_24x32", [LAYOUT], layout_out=CM16, H=24, W=32)
    # chunk-major output of a layer the 64-tile kernel does take
    add("cm_out_Cout_120", [PLAIN], s2d_out=CM16, H=32, W=32, Cout=120)
    add("cm_out_Cout_120", [LAYOUT], layout_out=CM16, Cout=120)
    add("cm_out_slice", [PLAIN], s2d_out=CM16, H=32, W=32, Cout=64, out_cstride=128)
    add("cm_out_slice_offset", [PLAIN], s2d_out=CM16, H=32, W=32, Cout=64, out_cstride=128, out_coff=64)
    add("slice_past_stride", SLICED, out_cstride=128, out_coff=4)
    add("slice_negative_offset", SLICED, Cout=64, out_cstride=128, out_coff=-4)
    add("slice_offset_2", SLICED, Cout=64, out_cstride=128, out_coff=2)
    add("slice_stride_130", SLICED, Cout=64, out_cstride=130)
    add("slice_stride_below_Cout", SLICED, out_cstride=64)
    add("slice_s2d", SLICED, s2d_out=1, out_cstride=256)
    for k in (1, 0, -1):
        add(f"ksplit_{k}", [SPLITK], ksplit=k)
    add("ksplit_3", [SPLITK], ksplit=3)                               # 8 chunks do not divide by 3
    add("ksplit_4_runs_of_2", [SPLITK], ksplit=4)                     # 8 chunks: four runs of 2 < 4
    add("ksplit_2_runs_of_3", [SPLITK], ksplit=2, Cin=96)             # 6 chunks: two odd runs
    add("ksplit_256", [SPLITK], ksplit=256, Cin=256 * 4 * 16)         # even runs of 4 chunks, but ksplit >= 256
    # 2^31 tiles: a 16x16 image is two 16x8-pixel tiles; a transposed layer has four phases per tile
    add("too_many_tiles", ["dsic_conv3x3_wino_nhwc", PLAIN], B=1 << 30)
    add("too_many_tiles", ["dsic_conv_transpose2d_wino_nhwc", "dsic_conv_transpose2d_wino_bf16_nhwc", LAYOUT], B=1 << 29)
    add("too_many_tiles", [SPLITK], B=1 << 29)                        # times ksplit = 2
    add("image_in_2GiB", EXPORTS, H=2048, W=2048)                     # 2048 * 2048 * 128 * 4 = 2^31
    add("image_out_2GiB", ["dsic_conv3x3_wino_nhwc"], H=2048, W=4096, Cin=32)
    add("image_out_2GiB", [e for e in EXPORTS if "transpose" in e], H=1024, W=1024, Cin=64)   # four times the pixels
    add("image_out_stride_2GiB", SLICED, H=1024, W=1024, Cout=64, out_cstride=512)
    add("weights_2GiB", CONV3, Cin=1 << 18)                           # 16 * Cin * 128 * 4 bytes = 2^31
    add("weights_2GiB", [e for e in EXPORTS if "transpose" in e], Cin=1 << 16)   # four phases
    ids = [c[0] for c in out]
    assert len(ids) == len(set(ids))
    return out


def answers(L):
    """{case id: [status, message, output untouched]} of library L."""
    got = {}
    for cid, export, over in cases():
        bufs = {p: ctypes.create_string_buffer(PATTERN, len(PATTERN)) for p in POINTERS}
        args = []
        for name in EXPORTS[export]:
            if name in POINTERS:
                v = over.get(name, bufs[name])
                args.append(None if v is None else ctypes.cast(v, ctypes.c_void_p))
            else:
                args.append(over.get(name, VALID[name]))
        status = getattr(L, export)(*args)
        msg = L.dsic_last_error().decode(errors="replace") if status else ""
        got[cid] = [status, msg, all(b.raw == PATTERN for b in bufs.values())]
    return got


def test_every_refusal_equals_the_recording(golden_dir):
    from dsic_amd import lib
    want = json.load(open(os.path.join(golden_dir, "wino_refusals.json")))
    got = answers(lib.load())
    assert sorted(got) == sorted(want), "the case table and the recording differ: re-record"
    bad = [f"{cid}: got {got[cid][:2]}, recorded {want[cid]}" for cid in got if got[cid][:2] != want[cid]]
    assert not bad, f"{len(bad)} of {len(got)} cases differ:\n" + "\n".join(bad[:20])
    assert all(ok for _, _, ok in got.values()), [cid for cid, v in got.items() if not v[2]]


def test_every_recorded_case_is_a_refusal_with_its_own_message(golden_dir):
    """a case that reached a launch would be recorded with another status; every requirement has its message"""
    want = json.load(open(os.path.join(golden_dir, "wino_refusals.json")))
    assert all(status == 1 and msg for status, msg in want.values())
    fragments = ["null pointer", "empty tensor", "must be a positive multiple of 32", "must be a multiple of 32, >= 64",
                 "must be a multiple of 4, <= 128", "act=", "needs beta and gamma", "needs even H and W",
                 "needs Cin = 4*Cs", "chunk-major activations are not supported", "layout_in=",
                 "64-tile kernel only", "whole 16-channel chunks", "does not fit a pixel stride",
                 "cannot be stored space-to-depth", "ksplit=", "does not divide Cin", "too many tiles",
                 "one image must stay below 2 GiB", "transformed weights must stay below 2 GiB"]
    for f in fragments:
        assert any(f in msg for _, msg in want.values()), f


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", required=True, metavar="OUT.json")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import dsic_amd
    from dsic_amd import lib
    got = answers(lib.load())
    reached = [cid for cid, (status, _, ok) in got.items() if status != 1 or not ok]
    assert not reached, f"not refused with DSIC_EINVAL, or wrote to a buffer: {reached}"
    with open(a.record, "w") as f:
        json.dump({cid: v[:2] for cid, v in got.items()}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{a.record}: {len(got)} cases of {os.path.dirname(dsic_amd.__file__)}")
