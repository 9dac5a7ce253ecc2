"""The step orders bench.py measures, restated once so that tests can run them on DISTINCT batches.

bench.py keeps its step closures inside main() and feeds every step the same batch, so they can be neither imported
nor told apart by their data.  This file RESTATES them; it does not call them.  What it restates, by bench.py line:

    run_staggered   step() 308-318, drain() 320-324, finish() 326-344, the reservations 377-379, coder.wait() 393-394
    run_lanes       the lane streams 295-299, step() 310-312 under run_step() 352-356, the lane join 390-392
    run_e2e         the buffers 441-446, e2e_finish() 450-454, e2e_step() 456-472, e2e_drain() 474-476, 478-479, 488

and what it leaves out: the metric all-reduce and `totals` (one rank here), the kernel timer, the clock.  A change of
those bench.py lines has to be carried over here by hand; tests/test_pipeline_driver_cpu.py holds this file to the
order bench.py documents (A0 A1 S0 A2 S1 ... S(K-1), buffers i % 3 and i & 1, coded size `depth` steps late).

reference() is the plain restatement the pipelines are compared with: one batch at a time on one stream, a host
synchronisation after every call, nothing overlapping anything.

Streams, events, buffers, copies, to_tensor and MS-SSIM go through a small runtime object (CudaRuntime), so that the
CPU test can put a recording stand-in in its place; the module itself imports without a GPU.
"""
import math

import torch

KEYS = ("x_hat", "nll_y", "nll_z", "y", "y_tilde", "z", "z_tilde", "sigma", "nu")
STATE_TENSORS = ("y", "y_hat", "y_noisy", "z", "sigma", "nu")


class CudaRuntime:
    """The real thing: torch.cuda streams and events, pinned host buffers, the package's MS-SSIM."""

    def current_stream(self):
        return torch.cuda.current_stream()

    def stream(self, s):
        return torch.cuda.stream(s)

    def event(self, timing=False):
        return torch.cuda.Event(enable_timing=timing)

    def empty(self, shape, dtype, pinned=False):
        if pinned:
            return torch.empty(shape, dtype=dtype).pin_memory()
        return torch.empty(shape, dtype=dtype, device="cuda")

    def copy(self, dst, src):
        dst.copy_(src, non_blocking=True)

    def ms_ssim(self, x_hat, x):
        from dsic_amd import metrics
        return metrics.ms_ssim_per_image(x_hat, x, clamp_x=True)

    def to_tensor(self, u8):
        from dsic_amd import ops
        return ops.to_tensor_u8(u8)


def state_tensors(st):
    """every tensor a stage state holds: y, y_hat, y_noisy, z, sigma, nu and the tensors of r"""
    ts = [st.get(k) for k in STATE_TENSORS] + list(st["r"].values())
    return [t for t in ts if torch.is_tensor(t)]


def poison_like(st):
    """One NaN-filled tensor of the byte size of each tensor of the stage state, allocated on the caller's stream and
    dropped at once.

    In a correct pipeline these allocations are served from free blocks only, and the NaNs land in memory nobody reads.
    If the caching allocator hands out a block that a kernel on another stream still reads or writes (a tensor dropped
    before its last reader was ordered behind it), the NaN lands in a result.  This makes a lifetime error LIKELY to
    show, not certain: the allocator must pick the block in question, and the fill must win the race."""
    for t in state_tensors(st):
        nbytes = t.numel() * t.element_size()
        p = torch.full(((nbytes + 3) // 4,), math.nan, dtype=torch.float32, device=t.device)
        del p


def coder_args_of(coder):
    """what reference() hands compress_latents so that it codes like `coder`"""
    return {"tail": coder.tail, "Lmax": coder.Lmax, "streams_per_wg": coder.streams_per_wg, "segments": coder.segments}


def _reserve(model, coder, n_stage, n_coder):
    model.reserve_stage_events(n_stage)
    if coder is not None:
        coder.reserve_events(n_coder)
        coder.timing = True


class _Finisher:
    """bench.py finish(): per-image bpp and MS-SSIM against the batch's OWN image, and the coded size of the batch
    `depth` steps earlier, joined through the coder's `done` event and enqueued with no host synchronisation."""

    def __init__(self, xs, coder, depth, rt):
        self.xs, self.coder, self.depth, self.rt = xs, coder, depth, rt
        self.pending = []
        self.results = [None] * len(xs)

    def __call__(self, i, out, clast):
        x = self.xs[i]
        H, W = x.shape[-2], x.shape[-1]
        bpp = out.sums.sum(dim=1) / float(H * W)
        msssim = self.rt.ms_ssim(out["x_hat"], x)
        late, late_of = None, None
        if self.coder is not None:
            self.pending.append((i, clast))
            if len(self.pending) > max(1, self.depth):
                late_of, prev = self.pending.pop(0)
                self.rt.current_stream().wait_event(prev["done"])
                late = prev["lengths"].sum()                 # a device scalar; nothing waits for it on the host
        self.results[i] = {"out": out, "sums": out.sums, "bpp": bpp, "ms_ssim": msssim, "late": late,
                           "late_of": late_of, "coded": clast}
        return out


def run_staggered(model, xs, coder, depth, poison=True, quant_mode="round", rt=None, marks=None):
    """bench.py's default order over the distinct batches xs: A0 A1 S0 A2 S1 ... S(K-1), A = encode_stage (+ the coder's
    start), S = decode_stage + finish.  -> one dict per batch: out (the nine keys), sums, bpp, ms_ssim, late (the coded
    size that entered THIS step's reduction, a device scalar, None in the first `depth` steps), late_of (the batch it
    belongs to), coded (the coder's result captured at this batch's encode_stage: bytes, lengths, err, cap_z, ...).

    poison: see poison_like(); after every stage call, on the caller's stream.  marks: a list that receives one
    timing event per step, recorded on the caller's stream where the step starts (measurements only)."""
    rt = rt or CudaRuntime()
    _reserve(model, coder, len(xs) + 2, len(xs) + 1)
    finish = _Finisher(xs, coder, depth, rt)
    staged = []

    def decode(i, st, clast):
        out = model.decode_stage(st)
        if poison:
            poison_like(st)
        finish(i, out, clast)

    for i, x in enumerate(xs):
        if marks is not None:
            e = rt.event(timing=True)
            e.record()
            marks.append(e)
        st = model.encode_stage(x, quant_mode=quant_mode, after_rate=coder)
        if poison:
            poison_like(st)
        staged.append((i, st, coder.last if coder is not None else None))
        if len(staged) < 2:
            continue
        decode(*staged.pop(0))
    while staged:                                            # drain(): the synthesis the order still owes
        decode(*staged.pop(0))
    if coder is not None:
        coder.wait()                                         # stream-level join, as before bench.py's clock stops
    return finish.results


def run_lanes(model, xs, coder, lanes, rt=None):
    """bench.py --lanes: step i is a whole forward(x_i, after_rate=coder) + finish on stream lanes[i % L].  Every lane
    first waits for the caller's stream; all lanes (and the coder) are joined to it at the end.  The coded size is
    taken len(coder.streams) steps late, as in run_staggered.  -> the same dicts."""
    rt = rt or CudaRuntime()
    _reserve(model, coder, len(xs) + 2, len(xs) + 1)
    finish = _Finisher(xs, coder, len(coder.streams) if coder is not None else 1, rt)
    caller = rt.current_stream()
    for ln in lanes:
        ln.wait_stream(caller)
    for i, x in enumerate(xs):
        with rt.stream(lanes[i % len(lanes)]):
            out = model(x, quant_mode="round", after_rate=coder)
            finish(i, out, coder.last if coder is not None else None)
    for ln in lanes:
        caller.wait_stream(ln)
    if coder is not None:
        coder.wait()
    return finish.results


def run_e2e(model, host_u8, coder, poison=True, rt=None):
    """bench.py --e2e over the distinct pinned uint8 [B,H,W,C] batches host_u8: three rotating device input buffers
    filled on the main stream (i % 3), encode_stage on the uint8 buffer, the strings and lengths copied to two rotating
    pinned buffers (i & 1) on the coder stream of that call, decode_stage + MS-SSIM against the DEVICE buffer one step
    later.  After each D2H an event is recorded on that coder stream; before the buffer is written again the host waits
    for that event alone and snapshots the buffer.  -> per batch: out, sums, ms_ssim, host_bytes, host_lengths (the
    snapshots), cap_z, cap_y, segments, err."""
    rt = rt or CudaRuntime()
    n = len(host_u8)
    _reserve(model, coder, n + 5, n + 4)
    dev_in = [rt.empty(tuple(host_u8[0].shape), torch.uint8) for _ in range(3)]
    copied = [rt.event() for _ in range(n)]
    host_bytes = host_len = None
    slot = [None, None]                                      # per pinned buffer: (batch, its D2H's event)
    results = [None] * n
    e_staged = []

    def snapshot(j):
        if slot[j] is not None:
            b, ev = slot[j]
            ev.synchronize()                                 # this copy alone, not the device
            results[b].update(host_bytes=host_bytes[j].clone(), host_lengths=host_len[j].clone())
            slot[j] = None

    def finish(i, st, k):
        o = model.decode_stage(st)
        if poison:
            poison_like(st)
        # bench.py:453 writes dev_in[k].permute(0, 3, 1, 2).float() / 255.0, which torch evaluates on the device as a
        # product with 1 / 255: one ulp off to_tensor's quotient in some pixels.  The image MS-SSIM is held to is
        # to_tensor's, so the same read of the rotating buffer goes through the package's own kernel
        xf = rt.to_tensor(dev_in[k])
        results[i].update(out=o, sums=o.sums, ms_ssim=rt.ms_ssim(o["x_hat"], xf))

    for i in range(n):
        k, j = i % 3, i & 1
        rt.copy(dev_in[k], host_u8[i])
        st = model.encode_stage(dev_in[k], quant_mode="round", after_rate=coder)
        if poison:
            poison_like(st)
        last = coder.last
        results[i] = {"cap_z": last["cap_z"], "cap_y": last["cap_y"], "segments": last["segments"], "err": last["err"]}
        if host_bytes is None:
            host_bytes = [rt.empty(tuple(last["bytes"].shape), torch.uint8, pinned=True) for _ in range(2)]
            host_len = [rt.empty(tuple(last["lengths"].shape), torch.int32, pinned=True) for _ in range(2)]
        snapshot(j)
        side = coder.streams[(coder.calls - 1) % len(coder.streams)]
        with rt.stream(side):
            rt.copy(host_bytes[j], last["bytes"])
            rt.copy(host_len[j], last["lengths"])
            copied[i].record(side)
        slot[j] = (i, copied[i])
        e_staged.append((i, st, k))
        if len(e_staged) > 1:
            finish(*e_staged.pop(0))
    while e_staged:
        finish(*e_staged.pop(0))
    coder.wait()
    for j in (n & 1, (n + 1) & 1):                           # oldest buffer first
        snapshot(j)
    return results


def _per_channel(t):
    """[B,M,H,W] spatially constant (an expanded view) -> contiguous [B,M]; per-element tensors pass through"""
    if t.dim() == 4 and t.stride(2) == 0 and t.stride(3) == 0:
        return t[:, :, 0, 0].contiguous()
    return t.contiguous()


def reference(model, xs, coder_args, quant_mode="round"):
    """The plain restatement: model.HYPER_STREAM off, one batch at a time on the current stream with a device
    synchronisation after every call: forward(), then (coder_args not None) entropy.compress_latents synchronously on
    that forward's y_tilde, z_tilde, sigma, nu and sigma_z_of(model), then ms_ssim_per_image.  Nothing here overlaps
    anything.  -> per batch: out, sums, bpp, ms_ssim, coded (compress_latents' dict, or None)."""
    from dsic_amd import entropy, metrics, model as M
    saved = M.HYPER_STREAM
    res = []
    try:
        M.HYPER_STREAM = False
        sigma_z = entropy.sigma_z_of(model) if coder_args is not None else None
        torch.cuda.synchronize()
        for x in xs:
            out = model(x, quant_mode=quant_mode)
            torch.cuda.synchronize()
            coded = None
            if coder_args is not None:
                coded = entropy.compress_latents(out["y_tilde"], out["z_tilde"], _per_channel(out["sigma"]),
                                                 _per_channel(out["nu"]), sigma_z, **coder_args)
                torch.cuda.synchronize()
            ms = metrics.ms_ssim_per_image(out["x_hat"], x, clamp_x=True)
            torch.cuda.synchronize()
            bpp = out.sums.sum(dim=1) / float(x.shape[-2] * x.shape[-1])
            torch.cuda.synchronize()
            res.append({"out": out, "sums": out.sums, "bpp": bpp, "ms_ssim": ms, "coded": coded})
    finally:
        M.HYPER_STREAM = saved
    return res
