"""The three promises at the head of include/dsic_hip.h, held for every export that takes a stream (the recipes of
tests/stream_cases.py, through the C ABI alone): all device work of a call is enqueued on `stream`, in order; the call
returns without waiting for the device; calls on different streams with disjoint buffers do not affect each other.

Late input: on a side stream that really runs beside the null stream, the call is enqueued behind a sleep that is
still running when the call returns, with its inputs copied in behind that sleep too, over the finished state of
another, equally valid input set B.  A launch on another stream reads B (valid data, by the recipes' construction)
and the bytes differ from those of the same call on the default stream.  Neighbours: two side streams run the two
input sets at the same time on two sets of buffers and swap, three rounds.

Every buffer lies between guard bytes inside an allocation of its own, at the element offset of the Out / _inside
helpers of the other GPU tests, and the guards of all buffers, inputs included, are checked after every scenario."""
import time

import numpy as np
import pytest
import torch

import stream_cases as SC
from dsic_amd import lib

pytestmark = pytest.mark.gpu

GUARD = 64                                       # elements on either side, as in tests/test_gpu_codec_movers.py
GUARD_BYTE = 0xCD
MIN_SLEEP_MS, HOST_FACTOR, RETRY_FACTOR = 5.0, 50.0, 8
MAX_CANDIDATES = 8
_SIDE = {}                                       # the session's streams and the sleep calibration
_REF = {}                                        # recipe -> (Dev, want_A, want_B, host milliseconds of one call)
MEASURED = {"sleep_ms": {}, "retried": []}       # what a run observed (printed by the last test)


# ---- the side streams -------------------------------------------------------------------------------------------
def _cycles_per_ms():
    if "cycles" not in _SIDE:
        torch.cuda._sleep(1000)                  # loads the kernel
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        torch.cuda._sleep(20_000_000)
        b.record()
        b.synchronize()
        _SIDE["cycles"] = 20_000_000 / a.elapsed_time(b)
    return _SIDE["cycles"]


def _sleep(ms):
    torch.cuda._sleep(int(_cycles_per_ms() * ms))


def _runs_beside(sleeper, other):
    """True if a tiny fill on `other` completes while a 20 ms sleep on `sleeper` is still pending: the two do not
    share a hardware queue."""
    tiny = _SIDE.setdefault("tiny", torch.zeros(16, device="cuda"))
    torch.cuda.synchronize()
    with torch.cuda.stream(sleeper):
        _sleep(20.0)
        asleep = torch.cuda.Event()
        asleep.record(sleeper)
    with torch.cuda.stream(other):
        tiny.fill_(1.0)
        done = torch.cuda.Event()
        done.record(other)
    done.synchronize()
    beside = not asleep.query()
    torch.cuda.synchronize()
    return beside


def side_streams():
    """(S1, S2): S1 runs beside the default stream, S2 beside the default stream and beside S1.  At most
    MAX_CANDIDATES streams are tried for each; finding none is a failure, never a skip."""
    if "streams" not in _SIDE:
        null = torch.cuda.default_stream()
        tried, found = [], []                    # rejected streams stay alive, so the next one is another stream
        for want in (1, 2):
            for _ in range(MAX_CANDIDATES):
                cand = torch.cuda.Stream()
                tried.append(cand)
                if all(_runs_beside(cand, o) and _runs_beside(o, cand) for o in [null] + found):
                    found.append(cand)
                    break
            else:
                pytest.fail(f"none of {MAX_CANDIDATES} streams of torch.cuda.Stream() runs beside "
                            f"{'the default stream' if want == 1 else 'the default stream and the first side stream'}"
                            ": a misplaced launch could not show, so nothing below can be judged")
            _SIDE.setdefault("tried", []).append(len(tried))
        _SIDE["streams"], _SIDE["kept"] = tuple(found), tried
    return _SIDE["streams"]


# ---- one recipe's buffers on the device -------------------------------------------------------------------------
class Dev:
    def __init__(self, case):
        self.case = case
        self.whole, self.inner, self.stage = {}, {}, {}
        for name, b in case.bufs.items():
            g, nbytes = GUARD * b["dtype"].itemsize, b["n"] * b["dtype"].itemsize
            t = torch.full((g + nbytes + g,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
            self.whole[name], self.inner[name] = t, t[g:g + nbytes]
            self.inner[name].fill_(SC.FILL)
            if b["kind"] == "in":
                self.stage[name] = {w: torch.from_numpy(b[w].view(np.uint8).reshape(-1).copy()).cuda()
                                    for w in ("A", "B")}
        self.ptrs = SC.Ptrs({k: v.data_ptr() for k, v in self.inner.items()}, case.host)

    def load(self, which):
        """device-to-device, on the current stream"""
        for name, st in self.stage.items():
            self.inner[name].copy_(st[which], non_blocking=True)

    def prepare(self):
        """what the caller owes the export, on the current stream: zeros where the header says so, the fill in every
        other output.  A workspace keeps what the last call left in it, so a kernel that read it out of turn would
        read the finished state of a valid call."""
        for name, b in self.case.bufs.items():
            if b["zero"]:
                self.inner[name].zero_()
            elif b["kind"] == "out":
                self.inner[name].fill_(SC.FILL)

    def call(self, stream):
        L = lib.load()
        lib.check(self.case.call(L, self.ptrs, stream.cuda_stream or None), self.case.name)

    def keep(self):
        """copies of the judged buffers, on the current stream"""
        return {k: self.inner[k].clone() for k in self.case.judged()}

    def guards(self, what):
        for name, b in self.case.bufs.items():
            g = GUARD * b["dtype"].itemsize
            w = self.whole[name]
            assert bool((w[:g] == GUARD_BYTE).all()) and bool((w[-g:] == GUARD_BYTE).all()), \
                f"{self.case.name}: {what}: the guard of `{name}` was overwritten"


def _bytes(kept):
    return {k: v.cpu().numpy().tobytes() for k, v in kept.items()}


def _reference(name):
    """want_A, want_B on the default stream, directly after host synchronisations, and the host time of the call"""
    if name not in _REF:
        case = SC.build(name, lib.load())
        if case.reach:
            case.reach(lib.load())
        d = Dev(case)
        null = torch.cuda.default_stream()
        want, host_ms = {}, 0.0
        for which in ("A", "B"):
            d.load(which)
            d.prepare()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            d.call(null)
            host_ms = (time.perf_counter() - t0) * 1e3          # B's: the modules are loaded by then
            torch.cuda.synchronize()
            want[which] = _bytes(d.keep())
            d.guards(f"default stream, set {which}")
        assert any(want["A"][k] != want["B"][k] for k in want["A"]), f"{name}: want_A == want_B"
        _REF[name] = (d, want["A"], want["B"], host_ms)
    return _REF[name]


def _differences(got, want):
    bad = []
    for k in want:
        if got[k] != want[k]:
            a, b = np.frombuffer(got[k], np.uint8), np.frombuffer(want[k], np.uint8)
            d = np.flatnonzero(a != b)
            bad.append(f"`{k}`: {d.size} of {a.size} bytes differ, first at {int(d[0])}")
    return bad


def test_a_side_stream_runs_beside_the_default_stream():
    s1, s2 = side_streams()
    assert s1.cuda_stream != 0 and s2.cuda_stream != 0 and s1.cuda_stream != s2.cuda_stream
    print(f"\ncandidates tried: first side stream after {_SIDE['tried'][0]}, second after {_SIDE['tried'][1]} in all; "
          f"{_cycles_per_ms():.0f} sleep cycles per ms")


@pytest.mark.parametrize("name", SC.names())
def test_late_input(name):
    s1, _ = side_streams()
    d, want_a, want_b, host_ms = _reference(name)
    null = torch.cuda.default_stream()
    sleep_ms = max(MIN_SLEEP_MS, HOST_FACTOR * host_ms)
    for factor in (1, RETRY_FACTOR):
        if factor > 1:                           # back to the finished state of B
            d.load("B")
            d.prepare()
            d.call(null)
            MEASURED["retried"].append(name)
        torch.cuda.synchronize()
        with torch.cuda.stream(s1):
            _sleep(sleep_ms * factor)
            gate = torch.cuda.Event()
            gate.record(s1)
            d.load("A")
            d.prepare()
            d.call(s1)
            pending = not gate.query()
            kept = d.keep()
            d.load("B")                          # a kernel that runs later than its place on the stream sees B
        s1.synchronize()
        torch.cuda.synchronize()
        if pending:
            break
    else:
        pytest.fail(f"{name}: the call returned only after a sleep of {sleep_ms * RETRY_FACTOR:.0f} ms on its stream "
                    f"had ended, twice: {', '.join(d.case.exports)} holds the host for that long")
    MEASURED["sleep_ms"][name] = sleep_ms * factor
    d.guards("late input")
    bad = _differences(_bytes(kept), want_a)
    assert not bad, f"{name} on a side stream, behind late inputs, differs from the default stream: " + "; ".join(bad)


@pytest.mark.parametrize("name", SC.names())
def test_neighbours(name):
    s1, s2 = side_streams()
    d1, want_a, want_b, host_ms = _reference(name)
    if name not in _SIDE.setdefault("second", {}):
        _SIDE["second"] = {name: Dev(d1.case)}   # one recipe's second set at a time
    d2 = _SIDE["second"][name]
    want = {"A": want_a, "B": want_b}
    sleep_ms = max(MIN_SLEEP_MS, HOST_FACTOR * host_ms)
    torch.cuda.synchronize()
    for rnd in range(3):
        sets = ("A", "B") if rnd % 2 == 0 else ("B", "A")
        kept = []
        for d, s, which in ((d1, s1, sets[0]), (d2, s2, sets[1])):
            with torch.cuda.stream(s):
                _sleep(sleep_ms)
                d.load(which)
                d.prepare()
                d.call(s)
                kept.append(d.keep())
        s1.synchronize()
        s2.synchronize()
        for d, k, which, s in ((d1, kept[0], sets[0], "first"), (d2, kept[1], sets[1], "second")):
            d.guards(f"neighbours, round {rnd}")
            bad = _differences(_bytes(k), want[which])
            assert not bad, (f"{name}, round {rnd}: set {which} on the {s} stream beside set "
                             f"{'B' if which == 'A' else 'A'} on the other: " + "; ".join(bad))


# ---- the Python wrappers ----------------------------------------------------------------------------------------
# Under `with torch.cuda.stream(S)`, behind a sleep and with inputs that arrive behind it.  These paths synchronise
# with the host by design, so only the bits are judged: those of the same call on the default stream.
def _late(stream, buffers, stages_a, stages_b, fn):
    """fn() on `stream` behind a sleep, the A contents copied into `buffers` behind it too and B's after the call"""
    with torch.cuda.stream(stream):
        _sleep(MIN_SLEEP_MS)
        for b, a in zip(buffers, stages_a):
            b.copy_(a, non_blocking=True)
        got = fn()
        got = [g.clone() for g in got] if isinstance(got, (list, tuple)) else got
        for b, st in zip(buffers, stages_b):
            b.copy_(st, non_blocking=True)
    return got


def _conv_cases():
    from dsic_amd import ops
    L = lib.load()
    g = torch.Generator().manual_seed(5)

    def rnd(*shape):
        return (torch.rand(*shape, generator=g) * 2 - 1).cuda()

    cases = []
    for name, H, W, Cin, Cout, kind in (("plain", 9, 11, 32, 8, "f32"), ("split-K", 16, 16, 128, 128, "bf16"),
                                       ("64-tile", 32, 32, 64, 16, "bf16"), ("transposed", 5, 7, 32, 8, "T")):
        xa, xb, bias = rnd(1, H, W, Cin), rnd(1, H, W, Cin), rnd(Cout)
        if kind == "T":
            u = ops.pack_wino_convT_weight(rnd(Cin, Cout, 5, 5))
            fn = lambda x, u=u, bias=bias, Cout=Cout: ops.conv_transpose2d_wino_nhwc(x, u, bias, Cout)
        else:
            u = ops.pack_wino_weight(rnd(Cout, Cin, 3, 3))
            if kind == "bf16":
                u = ops.split_wino_weight_bf16(u, Cout, Cin)
            fn = lambda x, u=u, bias=bias, Cout=Cout: ops.conv3x3_wino_nhwc(x, u, bias, Cout)
        if name == "split-K":
            assert L.dsic_wino_bf16_ksplit(H, W, Cin) > 1
        if name == "64-tile":
            assert L.dsic_wino_bf16_m64(H, W, Cin, 1) == 1
        cases.append((name, xa, xb, fn))
    return cases


def test_conv_wrappers_on_two_streams_at_once_take_a_ticket_each():
    from dsic_amd import ops
    s1, s2 = side_streams()
    dev = torch.device("cuda", torch.cuda.current_device())
    for name, xa, xb, fn in _conv_cases():
        want = {"A": fn(xa).clone(), "B": fn(xb).clone()}
        torch.cuda.synchronize()
        bufs = [xb.clone(), xa.clone()]                                   # each holds the other set until the copy
        torch.cuda.synchronize()
        got1 = _late(s1, [bufs[0]], [xa], [xb], lambda: fn(bufs[0]))
        got2 = _late(s2, [bufs[1]], [xb], [xa], lambda: fn(bufs[1]))
        s1.synchronize()
        s2.synchronize()
        assert torch.equal(got1.view(torch.int32), want["A"].view(torch.int32)), f"{name}: first stream"
        assert torch.equal(got2.view(torch.int32), want["B"].view(torch.int32)), f"{name}: second stream"
    tickets = []
    for s in (torch.cuda.default_stream(), s1, s2):
        with torch.cuda.stream(s):
            tickets.append(ops._ticket(dev))
    assert len({t.data_ptr() for t in tickets}) == 3, "streams share a Winograd ticket"
    torch.cuda.synchronize()
    assert all(int(t.abs().sum()) == 0 for t in tickets), "a ticket is not zero after its launches"


def test_ms_ssim_under_a_side_stream():
    from dsic_amd import metrics
    s1, _ = side_streams()
    g = torch.Generator().manual_seed(9)
    xa, ya, xb, yb = (torch.rand(2, 3, 176, 176, generator=g).cuda() for _ in range(4))
    want = metrics.ms_ssim_per_image(xa, ya).clone()
    assert not torch.equal(want, metrics.ms_ssim_per_image(xb, yb))
    x, y = xb.clone(), yb.clone()
    torch.cuda.synchronize()
    got = _late(s1, [x, y], [xa, ya], [xb, yb], lambda: metrics.ms_ssim_per_image(x, y).clone())
    s1.synchronize()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


def _model():
    from dsic_amd import synthetic as S
    from dsic_amd.model import CompressionModel
    if "model" not in _SIDE:
        sd = S.make_state_dict(seed=1, N=128, M=192, in_ch=3, spatial_params=False)
        m = CompressionModel(N=128, M=192, spatial_params=False, min_nu=2, max_nu=100.0, in_ch=3)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        _SIDE["model"] = m.cuda().eval()
    return _SIDE["model"]


def _scene(seed):
    from dsic_amd import synthetic as S
    return torch.from_numpy((S.make_patches(seed, 1, 150, 200, 3)[0] * 255.0 + 0.5).astype(np.uint8)).permute(
        1, 2, 0).contiguous().cuda()


def _coded():
    """the 150 x 200 scene of tests/test_gpu_near_lossless.py, coded and decoded on the default stream"""
    from dsic_amd import codec
    if "coded" not in _SIDE:
        a = _scene(31)
        stream = codec.compress_image(_model(), a, tile=64, batch=5, overviews=1)
        _SIDE["coded"] = (a, stream, codec.decompress_image(_model(), stream).clone())
    return _SIDE["coded"]


def test_codec_round_trip_under_a_side_stream():
    from dsic_amd import codec
    s1, _ = side_streams()
    a, want_stream, want_img = _coded()
    b = _scene(32)
    assert not torch.equal(a, b)
    img = b.clone()
    torch.cuda.synchronize()

    def both():
        stream = codec.compress_image(_model(), img, tile=64, batch=5, overviews=1)
        return stream, codec.decompress_image(_model(), stream).clone()
    with torch.cuda.stream(s1):
        _sleep(MIN_SLEEP_MS)
        img.copy_(a, non_blocking=True)
        stream, out = both()
        img.copy_(b, non_blocking=True)
    s1.synchronize()
    assert stream == want_stream, "the stream coded under a side stream differs"
    assert torch.equal(out, want_img)


def test_reader_opened_and_used_under_a_side_stream():
    from dsic_amd import codec
    s1, _ = side_streams()
    _, stream, _ = _coded()
    matrix = codec.rotation_affine(75, 100, 20, 1.5, 40, 60)

    def views(r):
        return [r.read(40, 50, 33, 35).clone(), r.read(8, 8, 120, 160, size=(30, 40)).clone(),
                r.render(8, 8, 120, 160, size=(30, 40), bands=(2, 0, 1), stretch=[(10, 200)] * 3).clone(),
                r.read_warped(matrix, (40, 60)).clone()]
    with codec.ImageReader(_model(), stream, batch=5) as r:
        want = views(r)
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        _sleep(MIN_SLEEP_MS)
        with codec.ImageReader(_model(), stream, batch=5) as r:
            got = views(r)
    s1.synchronize()
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and torch.equal(g, w), f"view {i} under a side stream differs"


def test_report():
    """what this run measured (pytest -s shows it)"""
    s = MEASURED["sleep_ms"]
    if s:
        longest = sorted(s.items(), key=lambda kv: -kv[1])[:5]
        print(f"\nsleep: {min(s.values()):.1f} .. {max(s.values()):.1f} ms over {len(s)} recipes; longest {longest}; "
              f"retried with {RETRY_FACTOR} x: {MEASURED['retried']}")
