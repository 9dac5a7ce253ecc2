"""tests/pipeline_driver.py's bookkeeping against the order bench.py documents, with a recording model, coder and
runtime in place of the GPU: which stage runs when, which state and which coder result reach which decode_stage, which
buffers a host-to-host step uses, and whose coded size enters which step.  Every batch, state and coder result carries
its batch index as data, so a wrong pairing shows as a wrong number, not only as a wrong call."""
import contextlib
import math

import pytest
import torch

import pipeline_driver as P

K = 6
B = 2


class _Out(dict):
    sums = None


class FakeStream:
    def __init__(self, name, log):
        self.name, self.log = name, log

    def wait_event(self, ev):
        self.log.append(("wait_event", self.name, ev.tag))

    def wait_stream(self, other):
        self.log.append(("wait_stream", self.name, other.name))


class FakeEvent:
    def __init__(self, log, tag=None):
        self.log, self.tag, self.on = log, tag, None

    def record(self, stream=None):
        self.on = stream.name if stream is not None else "current"
        self.log.append(("record", self.tag, self.on))

    def synchronize(self):
        self.log.append(("event_sync", self.tag, self.on))


class FakeRuntime:
    def __init__(self, log):
        self.log = log
        self.main = FakeStream("main", log)
        self.cur = self.main
        self.allocs = []             # (tensor, pinned) in allocation order
        self.events = 0
        self.x_scale = 1             # run_e2e hands MS-SSIM the uint8 image / 255

    def current_stream(self):
        return self.cur

    @contextlib.contextmanager
    def stream(self, s):
        prev, self.cur = self.cur, s
        try:
            yield
        finally:
            self.cur = prev

    def event(self, timing=False):
        self.events += 1
        return FakeEvent(self.log, ("rt", self.events - 1))

    def empty(self, shape, dtype, pinned=False):
        t = torch.zeros(shape, dtype=dtype)
        self.allocs.append((t, pinned))
        return t

    def index_of(self, t):
        return [i for i, (a, _) in enumerate(self.allocs) if a is t][0]

    def copy(self, dst, src):
        self.log.append(("copy", self.index_of(dst), self.cur.name, int(src.reshape(-1)[0])))
        dst.copy_(src)

    def to_tensor(self, u8):
        return u8.permute(0, 3, 1, 2).float() / 255.0

    def ms_ssim(self, x_hat, x):
        self.log.append(("ms_ssim", self.cur.name, int(x_hat.reshape(-1)[0]),
                         int(round(float(x.reshape(-1)[0]) * self.x_scale))))
        return torch.full((x.shape[0],), float(x_hat.reshape(-1)[0]))


class FakeCoder:
    """AsyncCompressor's surface: streams, calls, last, timing, reserve_events, wait; called as after_rate."""
    tail, Lmax, streams_per_wg, segments = 10, 256, 1, 1

    def __init__(self, depth, log):
        self.log = log
        self.streams = [FakeStream(f"coder{d}", log) for d in range(depth)]
        self.calls, self.last, self.timing, self.reserved = 0, None, False, None

    def reserve_events(self, n):
        self.reserved = n

    def __call__(self, partial):
        tag = int(partial["tag"])
        side = self.streams[self.calls % len(self.streams)]
        self.calls += 1
        self.log.append(("code", tag, side.name))
        self.last = {"tag": tag, "bytes": torch.full((B, 8), tag, dtype=torch.uint8),
                     "lengths": torch.tensor([[tag + 1, 10 * tag + 1]] * B, dtype=torch.int32),
                     "err": torch.zeros(1, dtype=torch.int32), "cap_z": 4, "cap_y": 4, "segments": 1,
                     "done": FakeEvent(self.log, ("done", tag))}

    def wait(self):
        self.log.append(("coder_wait",))
        return self.last


class FakeModel:
    """encode_stage / decode_stage / forward that record their calls; the batch index travels in the data."""

    def __init__(self, log, rt):
        self.log, self.rt, self.reserved = log, rt, None

    def reserve_stage_events(self, n):
        self.reserved = n

    def encode_stage(self, x, quant_mode="noise", after_rate=None):
        tag = int(x.reshape(-1)[0])
        self.log.append(("A", tag, self.rt.cur.name, quant_mode, x.dtype))
        t = lambda n, dt=torch.float32: torch.full((n,), tag, dtype=dt)     # noqa: E731
        r = {"y_tilde": t(5), "z_tilde": t(3), "nll_y": t(5), "nll_z": t(3), "sums": t(4, torch.float64),
             "y_hat_nhwc": t(5)}
        if after_rate is not None:
            after_rate({"tag": tag})
        return {"B": B, "tag": tag, "y": t(5), "y_hat": t(5), "y_noisy": None, "z": t(3), "sigma": t(2), "nu": t(2),
                "r": r, "taps": None, "joined": None}

    def decode_stage(self, st):
        self.log.append(("S", st["tag"], self.rt.cur.name))
        out = _Out({k: torch.full((B, 1), st["tag"], dtype=torch.float32) for k in P.KEYS})
        out["tag"] = st["tag"]
        out.sums = torch.full((B, 2), st["tag"], dtype=torch.float64)
        return out

    def __call__(self, x, quant_mode="noise", after_rate=None):
        return self.decode_stage(self.encode_stage(x, quant_mode, after_rate))


def _world(depth):
    log = []
    rt = FakeRuntime(log)
    coder = FakeCoder(depth, log) if depth else None
    return log, rt, FakeModel(log, rt), coder


def _batches():
    return [torch.full((B, 3, 4, 4), float(i)) for i in range(K)]


def _stages(log):
    return [f"{e[0]}{e[1]}" for e in log if e[0] in ("A", "S")]


@pytest.mark.parametrize("depth", [0, 1, 2])
def test_staggered_order_and_pairing(depth):
    log, rt, model, coder = _world(depth)
    res = P.run_staggered(model, _batches(), coder, depth, rt=rt)
    want = ["A0", "A1"] + [s for i in range(K - 2) for s in (f"S{i}", f"A{i + 2}")] + [f"S{K - 2}", f"S{K - 1}"]
    assert _stages(log) == want and want[:5] == ["A0", "A1", "S0", "A2", "S1"] and want[-1] == f"S{K - 1}"
    assert model.reserved == K + 2
    if coder is not None:
        assert coder.reserved == K + 1 and coder.timing is True and log[-1] == ("coder_wait",)
        assert [e[1:] for e in log if e[0] == "code"] == [(i, f"coder{i % depth}") for i in range(K)]
    assert all(e[3] == "round" for e in log if e[0] == "A")
    for i, r in enumerate(res):
        # the state of its own batch, the coder result captured at its own encode_stage, its own image
        assert r["out"]["tag"] == i and int(r["sums"][0, 0]) == i
        assert (r["coded"]["tag"] == i) if coder is not None else (r["coded"] is None)
        assert float(r["bpp"][0]) == 2 * i / 16.0              # sums.sum(dim=1) / (H * W)
        assert float(r["ms_ssim"][0]) == i
    assert [e[2:] for e in log if e[0] == "ms_ssim"] == [(i, i) for i in range(K)]


@pytest.mark.parametrize("depth", [1, 2])
def test_late_coded_size_belongs_to_the_batch_depth_steps_earlier(depth):
    log, rt, model, coder = _world(depth)
    res = P.run_staggered(model, _batches(), coder, depth, rt=rt)
    for i, r in enumerate(res):
        if i < depth:
            assert r["late"] is None and r["late_of"] is None
            continue
        j = i - depth
        assert r["late_of"] == j
        assert int(r["late"]) == B * ((j + 1) + (10 * j + 1))  # lengths of batch j, summed
    # joined on the caller's stream through that batch's own `done` event, after S(i) and nowhere on the host
    waits = [e for e in log if e[0] == "wait_event"]
    assert waits == [("wait_event", "main", ("done", i - depth)) for i in range(depth, K)]
    for i in range(depth, K):
        assert log.index(("wait_event", "main", ("done", i - depth))) > log.index(("S", i, "main"))
    assert not [e for e in log if e[0] == "event_sync"]


def test_quant_mode_reaches_every_encode_stage():
    log, rt, model, _ = _world(0)
    P.run_staggered(model, _batches(), None, 2, quant_mode="noise", rt=rt)
    assert [e[3] for e in log if e[0] == "A"] == ["noise"] * K


def test_poison_allocates_one_block_per_state_tensor_after_every_stage(monkeypatch):
    log, rt, model, coder = _world(1)
    fills = []
    real_full = torch.full

    def full(size, value, **kw):
        if isinstance(value, float) and math.isnan(value):
            fills.append((len(_stages(log)), size[0] * 4))
        return real_full(size, value, **kw)

    monkeypatch.setattr(torch, "full", full)
    P.run_staggered(model, _batches()[:2], coder, 1, rt=rt)
    # y y_hat z sigma nu (y_noisy is None) + the six tensors of r, float32 but for the float64 sums
    sizes = [20, 20, 12, 8, 8] + [20, 12, 20, 12, 32, 20]
    assert [n for _, n in fills] == sizes * 4
    assert [at for at, _ in fills] == [1] * 11 + [2] * 11 + [3] * 11 + [4] * 11      # A0 A1 S0 S1
    fills.clear()
    P.run_staggered(model, _batches()[:2], coder, 1, poison=False, rt=rt)
    assert not fills


def test_lanes_alternate_and_are_joined():
    log, rt, model, coder = _world(2)
    lanes = [FakeStream("lane0", log), FakeStream("lane1", log)]
    res = P.run_lanes(model, _batches(), coder, lanes, rt=rt)
    assert log[:2] == [("wait_stream", "lane0", "main"), ("wait_stream", "lane1", "main")]
    assert [(e[0], e[1], e[2]) for e in log if e[0] in ("A", "S")] == \
        [(s, i, f"lane{i % 2}") for i in range(K) for s in ("A", "S")]
    assert log[-3:] == [("wait_stream", "main", "lane0"), ("wait_stream", "main", "lane1"), ("coder_wait",)]
    assert rt.cur is rt.main
    # the coded size is joined on the lane that runs the step, two steps late
    assert [e for e in log if e[0] == "wait_event"] == [("wait_event", f"lane{i % 2}", ("done", i - 2))
                                                         for i in range(2, K)]
    for i, r in enumerate(res):
        assert r["out"]["tag"] == i and r["coded"]["tag"] == i
        assert r["late_of"] == (i - 2 if i >= 2 else None)
    assert [e[1:] for e in log if e[0] == "ms_ssim"] == [(f"lane{i % 2}", i, i) for i in range(K)]


@pytest.mark.parametrize("depth", [1, 2])
def test_e2e_buffers_rotate_by_three_and_by_two(depth):
    log, rt, model, coder = _world(depth)
    host = [torch.full((B, 4, 4, 3), i, dtype=torch.uint8) for i in range(K)]
    rt.x_scale = 255
    res = P.run_e2e(model, host, coder, rt=rt)
    # allocation order: three device inputs, then (at the first step) two byte buffers and two length buffers
    assert [p for _, p in rt.allocs] == [False] * 3 + [True] * 4
    dev_in, hb, hl = (0, 1, 2), (3, 4), (5, 6)
    copies = [e for e in log if e[0] == "copy"]
    uploads = [e for e in copies if e[1] in dev_in]
    assert uploads == [("copy", dev_in[i % 3], "main", i) for i in range(K)]
    d2h = [e for e in copies if e[1] not in dev_in]
    want = []
    for i in range(K):
        side = f"coder{i % depth}"
        want += [("copy", hb[i & 1], side, i), ("copy", hl[i & 1], side, i + 1)]
    assert d2h == want
    # every encode_stage reads the uint8 device buffer of its step; order A0 A1 S0 ... as the resident loop
    assert [e[4] for e in log if e[0] == "A"] == [torch.uint8] * K
    assert _stages(log)[:5] == ["A0", "A1", "S0", "A2", "S1"] and _stages(log)[-1] == f"S{K - 1}"
    assert model.reserved == K + 5 and coder.reserved == K + 4
    # one event per D2H on its coder stream; the host waits for exactly that event before the buffer is written again
    for i in range(K):
        rec = log.index(("record", ("rt", i), f"coder{i % depth}"))
        sync = log.index(("event_sync", ("rt", i), f"coder{i % depth}"))
        assert log.index(("copy", hl[i & 1], f"coder{i % depth}", i + 1)) < rec < sync
        if i + 2 < K:
            assert sync < log.index(("copy", hb[i & 1], f"coder{(i + 2) % depth}", i + 2))
    assert len([e for e in log if e[0] == "event_sync"]) == K
    for i, r in enumerate(res):
        assert r["out"]["tag"] == i
        assert torch.equal(r["host_bytes"], torch.full((B, 8), i, dtype=torch.uint8))
        assert torch.equal(r["host_lengths"], torch.tensor([[i + 1, 10 * i + 1]] * B, dtype=torch.int32))
    # MS-SSIM against the rotating device buffer, which still holds this batch one step later
    assert [e[2:] for e in log if e[0] == "ms_ssim"] == [(i, i) for i in range(K)]


def test_state_tensors_lists_what_the_model_puts_in_a_stage_state():
    """the names poison_like walks are the ones model.encode_stage returns (read from its source: no GPU here)"""
    import inspect
    from dsic_amd import model as M, ops
    src = inspect.getsource(M.CompressionModel.encode_stage)
    for k in P.STATE_TENSORS + ("r",):
        assert f'"{k}": ' in src, k
    assert '"sums": sums' in inspect.getsource(ops.rate)
