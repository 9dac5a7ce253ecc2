"""The calls layers.py makes into ops, case by case, against a recording of them (tests/golden/chain_calls.json).

ops.py forwards its arguments to the library unchanged, so a chain that makes the same ops calls with the same
arguments launches the same kernels on the same data.  Here the ops entry points that layers.py uses are replaced by
shape-only stand-ins that log their arguments and return an empty tensor of the right shape on the meta device; the
real library is still loaded for its host predicates (dsic_wino_bf16_m64, dsic_split_bf16), so no GPU is needed.

    python tests/test_chain_calls_cpu.py --record OUT.json [--root TREE]

writes the traces of TREE (default: this tree).  The stored file was recorded on the commit before layers.py got its
per-layer kernel decision and per-chain plan; a change of layers.py that is meant to launch something else re-records.
"""
import contextlib
import json
import os
import sys

import torch
import torch.nn as nn

SIZES = [(32, 32), (48, 80), (64, 64), (128, 96), (128, 128), (192, 192), (256, 256), (512, 512)]
# (N, M): the reference's; a second multiple of 32; N % 32 != 0 (direct kernels everywhere); below 64; above 128
WIDTHS = [(128, 192), (96, 160), (80, 120), (32, 64), (160, 256)]
# each switch alone against the default
SWITCHES = ["default", "cm0", "cm1", "nowino", "f32", "nosplitk"]
META = torch.device("meta")


def _sh(t):
    return list(t.shape)


def _dt(t):
    return str(t.dtype).replace("torch.", "")


def _empty(*shape):
    return torch.empty(shape, dtype=torch.float32, device=META)


def _act_shape(B, H, W, C, cm):
    return (B, C // 16, H, W, 16) if cm else (B, H, W, C)


class _StandIns:
    """Shape-only stand-ins for the ops entry points layers.py calls.  Each logs one short record."""

    def __init__(self, ops, log):
        self.ops, self.log = ops, log

    # packers: only the dtype of what they return is looked at (by the stand-ins below)
    def _pack_f32(self, *a, **k):
        return torch.empty(1, dtype=torch.float32)

    pack_conv_weight = pack_convT_weight = pack_convT_image_weight = _pack_f32
    pack_wino_weight = pack_wino_s2_weight = pack_wino_convT_weight = _pack_f32

    def split_wino_weight_bf16(self, u, Cout, Cin, nphase=1):
        return torch.empty(1, dtype=torch.uint8)

    def conv_first_nchw(self, x, w, bias, act=0, beta=None, gamma=None, s2d_out=False, cm_out=False):
        Cout = w.shape[0]
        B, H, W = (x.shape[0], x.shape[1], x.shape[2]) if x.dtype == torch.uint8 else (x.shape[0], x.shape[2], x.shape[3])
        self.log.append(["first", _sh(x), _dt(x), _dt(w), Cout, act, beta is not None, bool(s2d_out), bool(cm_out)])
        return _empty(*(_act_shape(B, H // 2, W // 2, 4 * Cout, cm_out) if s2d_out else _act_shape(B, H, W, Cout, cm_out)))

    def conv3x3_wino_nhwc(self, x, u, bias, Cout, act=0, beta=None, gamma=None, out=None, s2d_out=False,
                          algo_flops=None, s2d_in=False, out_coff=0, split_k=True, cm_in=False, cm_out=False):
        if (cm_in or cm_out) and u.dtype != torch.uint8:
            raise ValueError("conv3x3_wino_nhwc: chunk-major activations need the split-bf16 kernel")
        B, H, W, Cin = self.ops.cm16_shape(x) if cm_in else x.shape
        if algo_flops is None:             # what ops.conv3x3_wino_nhwc itself puts in its place
            algo_flops = 2.0 * B * H * W * Cout * Cin * 9
        self.log.append(["wino", _sh(x), _dt(x), _dt(u), Cout, act, beta is not None, bool(s2d_in), bool(s2d_out),
                         bool(cm_in), bool(cm_out), out_coff, None if out is None else _sh(out), bool(split_k),
                         algo_flops, _sh(bias), None if beta is None else _sh(beta)])
        if out is not None:
            return out
        return _empty(*(_act_shape(B, H // 2, W // 2, 4 * Cout, cm_out) if s2d_out else _act_shape(B, H, W, Cout, cm_out)))

    def conv2d_nhwc(self, x, w, bias, Cout, k, stride, act=0, beta=None, gamma=None, out=None, cin_real=None):
        B, H, W, _ = x.shape
        self.log.append(["direct", _sh(x), _dt(x), _dt(w), Cout, k, stride, act, beta is not None, cin_real,
                         None if out is None else _sh(out)])
        return _empty(B, -(-H // stride), -(-W // stride), Cout)

    def conv_transpose2d_wino_nhwc(self, x, u, bias, Cout, act=0, beta=None, gamma=None, out=None, cm_in=False,
                                   cm_out=False):
        if (cm_in or cm_out) and u.dtype != torch.uint8:
            raise ValueError("conv_transpose2d_wino_nhwc: chunk-major activations need the split-bf16 kernel")
        B, H, W, _ = self.ops.cm16_shape(x) if cm_in else x.shape
        self.log.append(["winoT", _sh(x), _dt(x), _dt(u), Cout, act, beta is not None, bool(cm_in), bool(cm_out),
                         None if out is None else _sh(out)])
        return _empty(*_act_shape(B, 2 * H, 2 * W, Cout, cm_out))

    def conv_transpose2d_nhwc(self, x, w, bias, Cout, act=0, beta=None, gamma=None, out=None):
        B, H, W, _ = x.shape
        self.log.append(["directT", _sh(x), _dt(x), _dt(w), Cout, act, beta is not None,
                         None if out is None else _sh(out)])
        return _empty(B, 2 * H, 2 * W, Cout)

    def conv_transpose2d_image(self, x, w, bias, Cimg, out=None):
        B, H, W, _ = x.shape
        self.log.append(["imageT", _sh(x), _dt(x), _dt(w), Cimg, None if out is None else _sh(out)])
        return _empty(B, Cimg, 2 * H, 2 * W)

    def to_tensor_u8(self, x):
        B, H, W, C = x.shape
        self.log.append(["to_tensor_u8", _sh(x), _dt(x)])
        return _empty(B, C, H, W)

    def image_to_nhwc8(self, x):
        B, C, H, W = x.shape
        self.log.append(["image_to_nhwc8", _sh(x), _dt(x)])
        return _empty(B, H, W, 8)

    def nchw_to_nhwc(self, x):
        B, C, H, W = x.shape
        self.log.append(["nchw_to_nhwc", _sh(x), _dt(x)])
        return _empty(B, H, W, C)

    def nhwc_to_nchw(self, x):
        B, H, W, C = x.shape
        self.log.append(["nhwc_to_nchw", _sh(x), _dt(x)])
        return _empty(B, C, H, W)

    def gdn_nchw(self, x, beta, gamma, inverse):
        self.log.append(["gdn_nchw", _sh(x), _dt(x), bool(inverse)])
        return _empty(*x.shape)

    def sigma_nu_spatial(self, ls, ln, min_nu, max_nu):
        B, H, W, M = ls.shape
        self.log.append(["sigma_nu_spatial", _sh(ls), _sh(ln)])
        return _empty(B, M, H, W), _empty(B, M, H, W)

    def hyper_params(self, t, w1s, b1s, w2s, b2s, w1n, b1n, w2n, b2n, M, min_nu, max_nu):
        self.log.append(["hyper_params", _sh(t), _dt(t), _sh(w1s), _sh(w2s), _sh(w1n), _sh(w2n), M])
        return [_empty(t.shape[0], M) for _ in range(4)]


_NAMES = [n for n in dir(_StandIns) if not n.startswith("_")]


@contextlib.contextmanager
def _standins(ops, log):
    s = _StandIns(ops, log)
    saved = {n: getattr(ops, n) for n in _NAMES}
    try:
        for n in _NAMES:
            setattr(ops, n, getattr(s, n))
        yield
    finally:
        for n, f in saved.items():
            setattr(ops, n, f)


@contextlib.contextmanager
def _switch(layers, ops, name):
    """One A/B switch away from the default for the duration of a case."""
    saved = (layers.USE_WINOGRAD, layers.CHUNK_MAJOR, getattr(layers, "USE_CHUNK_MAJOR", None), ops.WINO_SPLITK,
             layers.wino_bf16())
    try:
        if name in ("cm0", "cm1"):
            layers.CHUNK_MAJOR = int(name[2])
            if saved[2] is not None:          # trees with the second variable: what DSIC_CHUNK_MAJOR would set
                layers.USE_CHUNK_MAJOR = layers.CHUNK_MAJOR > 0
        elif name == "nowino":
            layers.USE_WINOGRAD = False
        elif name == "f32":
            layers.set_wino_bf16(False)
        elif name == "nosplitk":
            ops.WINO_SPLITK = False
        else:
            assert name == "default", name
        yield
    finally:
        layers.USE_WINOGRAD, layers.CHUNK_MAJOR, ops.WINO_SPLITK = saved[0], saved[1], saved[3]
        if saved[2] is not None:
            layers.USE_CHUNK_MAJOR = saved[2]
        layers.set_wino_bf16(saved[4])


class _Models:
    """The four transforms per (N, M, in_ch, spatial_params), built once (their weights are never read)."""

    def __init__(self, layers):
        self.layers, self._m = layers, {}

    def get(self, N, M, in_ch=3, spatial=False):
        key = (N, M, in_ch, spatial)
        if key not in self._m:
            L = self.layers
            self._m[key] = {"g_a": L.AnalysisTransform(N, M, in_ch=in_ch), "g_s": L.SynthesisTransform(N, M, out_ch=in_ch),
                            "h_a": L.HyperAnalysis(M, N), "h_s": L.HyperSynthesis(N, M, spatial_params=spatial)}
        return self._m[key]


def _cases(layers):
    """(id, switch, function of (models, taps list or None) that runs the case)."""
    out = []

    def chains(N, M, in_ch, B, H, W, sw, with_taps):
        Hy, Wy = -(-H // 16), -(-W // 16)
        Hz, Wz = -(-Hy // 4), -(-Wy // 4)
        tag = f"N{N}M{M}c{in_ch}_B{B}_{H}x{W}_{sw}_{'taps' if with_taps else 'notaps'}"
        runs = {
            "g_a_f32": lambda ms, t: ms.get(N, M, in_ch)["g_a"].forward_from_image(_empty(B, in_ch, H, W), t),
            "g_a_u8": lambda ms, t: ms.get(N, M, in_ch)["g_a"].forward_from_image(
                torch.empty((B, H, W, in_ch), dtype=torch.uint8, device=META), t),
            "h_a": lambda ms, t: ms.get(N, M, in_ch)["h_a"].forward_nhwc(_empty(B, Hy, Wy, M), t),
            "h_s": lambda ms, t: ms.get(N, M, in_ch)["h_s"].params_nhwc(_empty(B, Hz, Wz, N), 2.0, 100.0, t),
            "h_s_spatial": lambda ms, t: ms.get(N, M, in_ch, True)["h_s"].params_nhwc(_empty(B, Hz, Wz, N), 2.0, 100.0, t),
            "g_s": lambda ms, t: ms.get(N, M, in_ch)["g_s"].forward_nhwc(_empty(B, Hy, Wy, M), t),
        }
        for name, fn in runs.items():
            out.append((f"{name}/{tag}", sw, fn, with_taps))

    for H, W in SIZES:
        for sw in SWITCHES:
            for with_taps in (False, True):
                chains(128, 192, 3, 2, H, W, sw, with_taps)
        chains(128, 192, 4, 2, H, W, "default", True)
        for N, M in WIDTHS[1:]:
            chains(N, M, 3, 2, H, W, "default", True)
            chains(N, M, 3, 2, H, W, "f32", False)
    for sw in SWITCHES:
        chains(128, 192, 3, 64, 256, 256, sw, True)
    chains(128, 192, 3, 2, 34, 50, "default", True)       # odd maps: no space-to-depth edge below the first

    # the NCHW forwards of the transforms and of single layers
    def nchw(N, M, B, H, W, sw):
        Hy, Wy = -(-H // 16), -(-W // 16)
        tag = f"N{N}M{M}_B{B}_{H}x{W}_{sw}"
        out.append((f"fwd_g_a/{tag}", sw, lambda ms, t: ms.get(N, M)["g_a"](_empty(B, 3, H, W)), False))
        out.append((f"fwd_g_s/{tag}", sw, lambda ms, t: ms.get(N, M)["g_s"](_empty(B, M, Hy, Wy)), False))
        out.append((f"fwd_h_a/{tag}", sw, lambda ms, t: ms.get(N, M)["h_a"](_empty(B, M, Hy, Wy)), False))
        out.append((f"fwd_h_s/{tag}", sw, lambda ms, t: ms.get(N, M)["h_s"](_empty(B, N, -(-Hy // 4), -(-Wy // 4))), False))
        out.append((f"fwd_h_s_spatial/{tag}", sw,
                    lambda ms, t: ms.get(N, M, 3, True)["h_s"](_empty(B, N, -(-Hy // 4), -(-Wy // 4))), False))

    L = layers
    singles = {
        "conv3_128_128_3_1": lambda: L.Conv2d(128, 128, 3, 1), "conv_128_128_5_2": lambda: L.Conv2d(128, 128, 5, 2),
        "conv_128_192_5_2": lambda: L.Conv2d(128, 192, 5, 2), "conv_3_128_3_1": lambda: L.Conv2d(3, 128, 3, 1),
        "conv_192_128_3_1": lambda: L.Conv2d(192, 128, 3, 1), "conv_128_192_3_1": lambda: L.Conv2d(128, 192, 3, 1),
        "conv_80_80_3_1": lambda: L.Conv2d(80, 80, 3, 1), "conv_32_64_3_1": lambda: L.Conv2d(32, 64, 3, 1),
        "conv_128_128_1_1": lambda: L.Conv2d(128, 128, 1),
        "convT_192_128": lambda: L.ConvTranspose2d(192, 128, 5, 2, 2, output_padding=1),
        "convT_128_128": lambda: L.ConvTranspose2d(128, 128, 5, 2, 2, output_padding=1),
        "convT_128_3": lambda: L.ConvTranspose2d(128, 3, 5, 2, 2, output_padding=1),
        "convT_80_80": lambda: L.ConvTranspose2d(80, 80, 5, 2, 2, output_padding=1),
        "convT_32_32": lambda: L.ConvTranspose2d(32, 32, 5, 2, 2, output_padding=1),
        "gdn_128": lambda: L.GDN(128), "igdn_128": lambda: L.GDN(128, inverse=True),
    }
    built = {}

    def single(name):
        if name not in built:
            built[name] = singles[name]()
        return built[name]

    def cin(name):
        m = single(name)
        return m.in_channels if hasattr(m, "in_channels") else 128

    for sw in SWITCHES:
        for H, W in SIZES:
            nchw(128, 192, 2, H, W, sw)
        for H, W in [(8, 8), (16, 16), (20, 36), (64, 64), (128, 128)]:
            for name in singles:
                out.append((f"fwd_{name}/B2_{H}x{W}_{sw}", sw,
                            lambda ms, t, name=name, H=H, W=W: single(name)(_empty(2, cin(name), H, W)), False))
    for N, M in WIDTHS[1:]:
        nchw(N, M, 2, 64, 64, "default")
        nchw(N, M, 2, 256, 256, "default")

    # single layers through run_nhwc as the tests and the spatial heads call it
    gdn, igdn = (lambda: single("gdn_128")), (lambda: single("igdn_128"))
    for sw in ("default", "f32", "cm0", "nowino"):
        for H, W in [(10, 18), (16, 16), (32, 32), (64, 64)]:
            for name in ("conv_128_128_5_2", "conv_128_192_5_2"):
                out.append((f"run_s2d_{name}/B2_{H}x{W}_{sw}", sw, lambda ms, t, name=name, H=H, W=W: single(name).run_nhwc(
                    _empty(2, H, W, 512), L.ops.ACT_GDN, None, x_is_s2d=True), False))
                out.append((f"run_s2d_gdn_{name}/B2_{H}x{W}_{sw}", sw, lambda ms, t, name=name, H=H, W=W: single(name).run_nhwc(
                    _empty(2, H, W, 512), L.ops.ACT_GDN, single("gdn_128") if name.endswith("128_5_2") else L.GDN(192),
                    x_is_s2d=True), False))
            out.append((f"run_s2d_s2dout/B2_{H}x{W}_{sw}", sw, lambda ms, t, H=H, W=W: single("conv_128_128_5_2").run_nhwc(
                _empty(2, H, W, 512), L.ops.ACT_GDN, gdn(), True, True), False))
            out.append((f"run_s2dout/B2_{H}x{W}_{sw}", sw, lambda ms, t, H=H, W=W: single("conv3_128_128_3_1").run_nhwc(
                _empty(2, H, W, 128), L.ops.ACT_IGDN, igdn(), False, True), False))
            out.append((f"run_cm_in_out/B2_{H}x{W}_{sw}", sw, lambda ms, t, H=H, W=W: single("conv3_128_128_3_1").run_nhwc(
                _empty(2, 8, H, W, 16), L.ops.ACT_RELU, None, cm_in=True, cm_out=True), False))
            out.append((f"run_cm_s2d/B2_{H}x{W}_{sw}", sw, lambda ms, t, H=H, W=W: single("conv_128_128_5_2").run_nhwc(
                _empty(2, 32, H, W, 16), L.ops.ACT_GDN, gdn(), x_is_s2d=True, s2d_out=True, cm_in=True, cm_out=True), False))
            out.append((f"run_cm_out_T/B2_{H}x{W}_{sw}", sw, lambda ms, t, H=H, W=W: single("convT_128_128").run_nhwc(
                _empty(2, H, W, 128), L.ops.ACT_IGDN, igdn(), cm_out=True), False))
            out.append((f"run_cm_in_T/B2_{H}x{W}_{sw}", sw, lambda ms, t, H=H, W=W: single("convT_192_128").run_nhwc(
                _empty(2, 12, H, W, 16), cm_in=True), False))
            out.append((f"run_cm_image/B2_{H}x{W}_{sw}", sw, lambda ms, t, H=H, W=W: single("convT_128_3").run_nhwc(
                _empty(2, 8, H, W, 16), cm_in=True), False))

    # chains of other make: a wide 5x5/s2 layer asked for a space-to-depth output, stand-alone activations, a first
    # layer followed by an inverse GDN, an image layer in the middle
    other = {
        "wide_then_s2": lambda: L._Chain(L.conv(128, 128, 3, 1), L.conv(128, 192, 5, 2), L.conv(192, 128, 5, 2)),
        "lone_acts": lambda: L._Chain(L.GDN(128), L.conv(128, 128, 3, 1), nn.ReLU(), nn.ReLU(), L.GDN(128, inverse=True),
                                      L.conv(128, 128, 5, 2)),
        "first_igdn": lambda: L._Chain(L.conv(3, 128, 3, 1), L.GDN(128, inverse=True), L.conv(128, 128, 3, 1)),
        "first_relu_s2": lambda: L._Chain(L.conv(3, 64, 3, 1), nn.ReLU(), L.conv(64, 64, 5, 2), L.conv(64, 64, 3, 1)),
        "first_40": lambda: L._Chain(L.conv(3, 40, 3, 1), L.GDN(40), L.conv(40, 40, 5, 2)),
        "T_then_s2": lambda: L._Chain(L.ConvTranspose2d(128, 128, 5, 2, 2, output_padding=1), L.conv(128, 128, 5, 2),
                                      L.ConvTranspose2d(128, 3, 5, 2, 2, output_padding=1), nn.ReLU()),
        "unknown_module": lambda: L._Chain(L.conv(128, 128, 3, 1), nn.Sigmoid()),
        "empty": lambda: L._Chain(),
    }
    for name in other:
        for H, W in [(32, 32), (64, 64), (128, 128)]:
            for sw in ("default", "f32", "nowino"):
                def run(ms, t, name=name, H=H, W=W):
                    if name not in built:
                        built[name] = other[name]()
                    c = built[name]
                    m0 = next(iter(c), None)
                    if isinstance(m0, L.Conv2d) and m0.in_channels == 3:
                        return c.forward_from_image(_empty(2, 3, H, W), t)
                    return c.forward_nhwc(_empty(2, H, W, 128), t)
                out.append((f"chain_{name}/B2_{H}x{W}_{sw}", sw, run, True))
    # an image whose channel count the first layer does not take
    for name, x in (("g_a_f32_wrong_channels", _empty(2, 4, 64, 64)), ("g_a_12_channels", _empty(2, 12, 64, 64)),
                    ("g_a_u8_wrong_channels", torch.empty((2, 64, 64, 4), dtype=torch.uint8, device=META))):
        out.append((name, "default", lambda ms, t, x=x: ms.get(128, 192)["g_a"].forward_from_image(x, t), True))
    ids = [c[0] for c in out]
    assert len(ids) == len(set(ids))
    return out


def _flat(r):
    """Tensors in a case's return value -> their shapes."""
    if isinstance(r, torch.Tensor):
        return _sh(r)
    if isinstance(r, (tuple, list)):
        return [_flat(v) for v in r]
    return r


_traces = None


def trace_all():
    """{case id: list of records} of the dsic_amd that is importable now (traced once per process)."""
    global _traces
    if _traces is None:
        _traces = _trace_all()
    return _traces


def _trace_all():
    from dsic_amd import layers, ops
    models = _Models(layers)
    traces = {}
    with torch.no_grad():
        for cid, sw, fn, with_taps in _cases(layers):
            log = []
            taps = [] if with_taps else None
            with _switch(layers, ops, sw), _standins(ops, log):
                try:
                    log.append(["returns", _flat(fn(models, taps))])
                    if taps is not None:
                        log.append(["taps", [_sh(t) for t in taps]])
                except Exception as e:     # a case the code refuses is recorded as the exception's type alone
                    log = [["raises", type(e).__name__]]
            traces[cid] = [json.dumps(r, separators=(",", ":")) for r in log]
    return traces


def _encode(traces):
    """Short file: every distinct record once, every distinct trace once (as record numbers), cases -> trace number."""
    records, rec_no, tr_list, tr_no, cases = [], {}, [], {}, {}
    for cid, tr in traces.items():
        key = tuple(rec_no.setdefault(r, len(rec_no)) for r in tr)
        if key not in tr_no:
            tr_no[key] = len(tr_list)
            tr_list.append(list(key))
        cases[cid] = tr_no[key]
    records = [json.loads(r) for r in rec_no]
    return {"records": records, "traces": tr_list, "cases": cases}


def _decode(doc):
    recs = [json.dumps(r, separators=(",", ":")) for r in doc["records"]]
    return {cid: [recs[i] for i in doc["traces"][t]] for cid, t in doc["cases"].items()}


def test_chain_calls_equal_the_recording(golden_dir):
    want = _decode(json.load(open(os.path.join(golden_dir, "chain_calls.json"))))
    got = trace_all()
    assert sorted(got) == sorted(want), "the case table and the recording differ: re-record"
    bad = []
    for cid in got:
        g, w = got[cid], want[cid]
        if g != w:
            i = next((i for i, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
            bad.append(f"{cid}: call {i}: got {g[i] if i < len(g) else 'nothing'}, recorded {w[i] if i < len(w) else 'nothing'}")
    assert not bad, f"{len(bad)} of {len(got)} cases differ; first: {bad[0]}\n" + "\n".join(bad[1:20])


def test_the_recording_covers_every_kernel_and_layout():
    """the case table is worth something only if the traces differ where the code has a choice"""
    from dsic_amd import layers
    if not layers.wino_bf16():
        return
    tr = trace_all()
    ops_seen = {json.loads(r)[0] for t in tr.values() for r in t}
    assert {"first", "wino", "direct", "winoT", "directT", "imageT", "to_tensor_u8", "image_to_nhwc8", "raises"} <= ops_seen
    wino = [json.loads(r) for t in tr.values() for r in t if r.startswith('["wino",')]
    assert any(r[9] and r[10] for r in wino) and any(r[11] for r in wino) and any(r[3] == "float32" for r in wino)
    d, c0 = tr["g_a_f32/N128M192c3_B2_256x256_default_taps"], tr["g_a_f32/N128M192c3_B2_256x256_cm0_taps"]
    assert d != c0 and d != tr["g_a_f32/N128M192c3_B2_256x256_cm1_taps"] != c0


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", required=True, metavar="OUT.json")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    doc = _encode(trace_all())
    with open(a.record, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    import dsic_amd
    print(f"{a.record}: {len(doc['cases'])} cases, {len(doc['traces'])} traces, {len(doc['records'])} records "
          f"of {os.path.dirname(dsic_amd.__file__)}")
