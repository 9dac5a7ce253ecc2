#!/usr/bin/env python3
"""Headline benchmark: 256x256x3 satellite patches through the modelv2 hot path.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--batch B] [--dump-outputs DIR] [--full]

One "step" = one pass of the hot path over one batch of B synthetic patches per
GPU (inputs resident in HBM before the timed region): analysis -> hyper-analysis
-> round -> hyper-synthesis -> Student-t/Gaussian rate -> CDF tables + range
coder of the z,y strings (second stream) -> synthesis, per-image bpp + MS-SSIM,
then the cross-GPU all-reduce of the metric sums: BASELINE.json config 3, the
largest single-GPU configuration (`--no-entropy` drops the coder: config 2;
`--size 512 --channels 4 --batch 32` is the per-GPU shape of config 5).
Prints ONE JSON line on rank 0 (contract in the task statement).

A plain run sets up, warms up, times the K steps and prints the line (`--dump-outputs DIR` also writes what the
last timed step computed as DIR/<name>.npy).  `--full` adds what the headline figure does not need: HIP events
around the dominant kernel's launches in the timed steps (the `roofline` object) and the CPU baseline.

For N > 1 the driver launches this file with torch.distributed.run, one rank
per GPU; images are sharded by global index, there is no data-path collective.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# The workload uses five HIP streams per process (main, hyperprior branch, two coder streams, RCCL's).  The HIP
# runtime maps streams onto 4 hardware queues by default; a fifth stream then shares a queue, and the metric
# all-reduce queued behind a 4.7 ms encoder kernel cost 2 ms per step under torch.distributed.run (6 720 instead
# of 8 520 patches/s).  Must be set before the runtime initialises; a smaller value in the environment (4, the
# runtime's own default, is often exported) is raised to 8.
try:
    _queues = int(os.environ.get("GPU_MAX_HW_QUEUES", "0"))
except ValueError:
    _queues = 0
if _queues < 8:
    os.environ["GPU_MAX_HW_QUEUES"] = "8"

import numpy as np  # noqa: E402
import torch  # noqa: E402

FLOP_PER_IMAGE_256 = 36.211e9        # 18.105 GMAC, conv/convT MACs x 2
PEAK_FP32_MFMA_TFLOPS = 157.3        # MI355X_MICROARCH.md: fp32-input MFMA peak
PEAK_BF16_MFMA_TFLOPS = 2500.0       # MI355X_MICROARCH.md: bf16 dense MFMA peak (16x the fp32-input rate)
PEAK_HBM_GBS = 8000.0


class KernelTimer:
    """HIP-event pairs around chosen launches on the launching stream.

    Events come from a pool that is created AND first recorded during warm-up: creating a HIP
    event costs host time (the first record of a torch event calls hipEventCreate), which would
    otherwise stall the enqueue thread inside the timed region."""

    def __init__(self):
        self.enabled = False
        self.only = None             # None: every conv launch; else the set of kernel symbols that get events
        self.events = True           # False: only note the symbols in `seen` (a plain run's timed steps carry no events)
        self.seen = set()            # symbols bracketed (or, without events, passed) while enabled since reset()
        self.records = []
        self.pool = []
        self.used = 0

    def _event(self):
        if self.used == len(self.pool):
            self.pool.append(torch.cuda.Event(enable_timing=True))
        e = self.pool[self.used]
        self.used += 1
        return e

    def reserve(self, n):
        """make sure n events exist and have been recorded once (forces hipEventCreate)"""
        while len(self.pool) < n:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self.pool.append(e)

    def reset(self):
        self.records = []
        self.seen = set()
        self.used = 0

    def record(self, name, flops, launch, exec_flops):
        if not self.enabled or (self.only is not None and name not in self.only):
            return launch()
        self.seen.add(name)
        if not self.events:
            return launch()
        e0, e1 = self._event(), self._event()
        e0.record()
        r = launch()
        e1.record()
        self.records.append((name, flops, e0, e1, exec_flops))
        return r

    def mark(self):
        """one event on the current stream (step boundaries)"""
        e = self._event()
        e.record()
        return e

    def summary(self):
        agg = {}
        for name, flops, e0, e1, ex in self.records:
            a = agg.setdefault(name, [0, 0.0, 0.0, 0.0])
            a[0] += 1
            a[1] += e0.elapsed_time(e1) * 1e-3
            a[2] += flops
            a[3] += ex
        return agg


def cpu_baseline(sd, patches, H, W, threads, with_coder, budget_s):
    """The oracle on the host cores, one image per call like modelseval.py:158-173: eager fp32
    forward (oracle/ref_model.py) + bpp + MS-SSIM[.3,.5,.2] (oracle/ref_metrics.py,
    modelseval.py:78-94) and, for config 3, the per-image tables + range coder of
    eval_selfcontained_entropy.py:36-62 (oracle/entropy_ref.c).  -> (images/s, images timed)."""
    from oracle import entropy_ref as E, ref_metrics as RM, ref_model as O
    torch.set_num_threads(threads)
    imgs = [torch.from_numpy(patches[i:i + 1]) for i in range(min(4, len(patches)))]
    sigma_z = np.exp(sd["z_prior.log_sigma"].astype(np.float64)).astype(np.float32)

    def one(x):
        out = O.forward(sd, x, "round")
        bpp = float((out["nll_y"].sum() + out["nll_z"].sum()) / (H * W))
        ms = float(RM.ms_ssim(out["x_hat"].clamp(0, 1), x, data_range=1.0, weights=(0.3, 0.5, 0.2)))
        nbytes = 0
        if with_coder:
            c = E.compress(out["y_tilde"].numpy(), out["z_tilde"].numpy(), out["sigma"][:, :, 0, 0].numpy(),
                           out["nu"][:, :, 0, 0].numpy(), sigma_z, tail=10)
            nbytes = sum(len(b) for b in c["strings"][0])
        return bpp, ms, nbytes

    one(imgs[0])
    times = []
    n = 0
    t_start = time.perf_counter()
    while n < 12 and (n < 2 or time.perf_counter() - t_start < budget_s):
        t0 = time.perf_counter()
        one(imgs[n % len(imgs)])
        times.append(time.perf_counter() - t0)
        n += 1
    return 1.0 / float(np.median(times)), n


DUMP_BUDGET_BYTES = 64 * 10**6
DUMP_SAMPLE = 8              # images of the batch whose per-element outputs are written


def dump_outputs(path, out, bpp, msssim, totals, coded):
    """What the last timed step handed its caller, as <path>/<name>.npy (float32, or float64 where the path computes
    in it): per-image bpp and MS-SSIM, the reduced metric sums, the coded string lengths for the whole batch; for a
    fixed sample of the batch's images (seeded, at most DUMP_SAMPLE, fewer if the files would exceed
    DUMP_BUDGET_BYTES) the forward outputs (x_hat, y, y_tilde, nll_y, z, z_tilde, nll_z, sigma, nu) and the z / y
    strings as byte values, zero past each string's length."""
    B = int(bpp.shape[0])
    per_image = {k: out[k] for k in ("x_hat", "y", "y_tilde", "nll_y", "z", "z_tilde", "nll_z", "sigma", "nu")
                 if out.get(k) is not None}
    for k in ("sigma", "nu"):
        t = per_image.get(k)
        if t is not None and t.dim() == 4 and t.stride(2) == 0 and t.stride(3) == 0:
            per_image[k] = t[:, :, 0, 0]             # spatially constant (expanded view): one value per channel
    lengths = coded["lengths"].cpu().numpy().astype(np.int64) if coded is not None else None
    if coded is not None:
        raw, cap_z = coded["bytes"], coded["cap_z"]
        per_image["z_strings"] = raw[:, :max(1, int(lengths[:, 0].max()))]
        per_image["y_strings"] = raw[:, cap_z:cap_z + max(1, int(lengths[:, 1].max()))]
    fixed = {"bpp": bpp, "ms_ssim": msssim, "metric_sums": totals}
    if lengths is not None:
        fixed["string_lengths"] = torch.from_numpy(lengths).double()
    fixed_bytes = sum(t.numel() * 8 for t in fixed.values())
    image_bytes = sum(t[0].numel() * 4 for t in per_image.values())
    k = min(B, DUMP_SAMPLE)
    while k > 1 and fixed_bytes + k * (image_bytes + 8) > DUMP_BUDGET_BYTES:
        k //= 2
    idx = np.sort(np.random.default_rng(0).choice(B, size=k, replace=False))
    arrays = {"image_index": idx.astype(np.float64)}
    for name, t in fixed.items():
        a = t.detach().cpu().numpy()
        arrays[name] = a if a.dtype == np.float64 else a.astype(np.float32)
    sel = torch.from_numpy(idx)
    for name, t in per_image.items():
        a = t.detach()[sel.to(t.device)].cpu().numpy()
        if name.endswith("_strings"):
            a = a.astype(np.float32)
            col = np.arange(a.shape[1])[None, :]
            a[col >= lengths[idx, 0 if name == "z_strings" else 1][:, None]] = 0.0
        arrays[name] = a if a.dtype == np.float64 else a.astype(np.float32)
    os.makedirs(path, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(a))
    return sum(a.nbytes for a in arrays.values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64, help="patches per GPU per step")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline figure does not need: HIP events around the dominant kernel's "
                         "launches in the timed steps (`roofline`) and the CPU baseline (unless --no-cpu-baseline)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed as DIR/<name>.npy (rank 0's shard)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--kernels", action="store_true",
                    help="bracket every conv launch of the timed steps with HIP events (adds `roofline`) and print the "
                         "per-kernel timings to stderr")
    ap.add_argument("--streams-per-wg", type=int, default=1,
                    help="range-coder waves per workgroup (1..16; 1: a wave has its CU's scalar unit to itself, "
                         "4.4 instead of 5.1 ms per batch and a 1 %% faster step than 4)")
    ap.add_argument("--decode", action="store_true",
                    help="also time entropy.custom_decompress of the same batch (eval_selfcontained_entropy.py:76-123): "
                         "adds a `decoder` object")
    ap.add_argument("--e2e", action="store_true",
                    help="also time the step from pinned-host uint8 [B,H,W,C] images to strings + lengths in pinned host "
                         "memory (modelseval.py:164, eval_selfcontained_entropy.py:68-74): adds an `e2e` object; `value` "
                         "stays the HBM-resident figure")
    ap.add_argument("--spatial-params", action="store_true",
                    help="the spatial_params=True branch (layers.py:127-129,143-145, model.py:49-51): per-element sigma / nu "
                         "heads, one coder table row per latent element")
    ap.add_argument("--coder-depth", type=int, default=2,
                    help="batches whose strings may be in the coder at once (side streams, round-robin); the coded "
                         "size of batch i enters the metric reduction of step i + depth")
    ap.add_argument("--coder-cus", type=int, default=0,
                    help="CUs reserved for the range coder's stream (0 = no CU masking)")
    ap.add_argument("--lanes", type=int, default=1,
                    help="batches in flight: step i runs on stream i %% lanes (kernel tails of one batch overlap the next)")
    ap.add_argument("--no-stagger", action="store_true",
                    help="analysis and synthesis of a batch back to back (default: the analysis runs one batch ahead)")
    ap.add_argument("--no-entropy", action="store_true",
                    help="BASELINE config 2 (transforms + rate + metrics only).  The default is config 3: the "
                         "CDF tables and the range coder of the z,y strings also run on the GPU (second stream)")
    ap.add_argument("--entropy", action="store_true", help="(default; kept for older command lines)")
    args = ap.parse_args()
    kernel_events = args.full or args.kernels        # HIP events inside the timed steps

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("--gpus N>1 must be launched with torch.distributed.run (one rank per GPU)")
        args.gpus = world
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    from dsic_amd import distributed as D
    D.init("nccl", dev)                                  # RCCL over xGMI when world > 1

    from dsic_amd import entropy, metrics, ops, synthetic as S
    from dsic_amd.model import CompressionModel

    B, H, W, C = args.batch, args.size, args.size, args.channels
    if args.lanes > 1 and not args.no_entropy and args.coder_depth % args.lanes:
        raise SystemExit("--lanes must divide --coder-depth (the lanes share the coder's side streams and buffers)")
    spatial = bool(args.spatial_params)
    sd = S.make_state_dict(seed=S.WEIGHT_SEED, in_ch=C, spatial_params=spatial)
    model = CompressionModel(N=128, M=192, spatial_params=spatial, min_nu=2, max_nu=100.0, in_ch=C)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    model = model.to(dev).eval()
    # this rank's slice of the global batch, resident in HBM before timing
    patches = S.make_patches(D.shard_first_index(rank, B), B, H, W, C)
    x = torch.from_numpy(patches).to(dev)

    timer = KernelTimer()
    ops.set_kernel_timer(timer)
    totals = torch.zeros(4, dtype=torch.float64, device=dev)
    coder = None
    main_stream = torch.cuda.current_stream()
    if not args.no_entropy:
        if args.coder_cus > 0:
            # the serial coder owns a few CUs (8 streams per CU); conv kernels use the others
            main_stream, side = entropy.masked_streams(args.coder_cus)
            coder = entropy.AsyncCompressor(model, stream=side, streams_per_wg=8)
        else:
            coder = entropy.AsyncCompressor(model, streams_per_wg=args.streams_per_wg, depth=args.coder_depth)
        coder.timing = True
    torch.cuda.set_stream(main_stream)
    count = torch.tensor(float(B), dtype=torch.float64, device=dev)
    zero = torch.zeros((), dtype=torch.float64, device=dev)

    pending = []
    last_step = {}

    # --lanes L: step i runs on stream i % L, so the tail of one batch's kernels (workgroups of a persistent kernel
    # finish up to one tile apart) and its small layers overlap the next batch's; every lane is joined before the
    # clock stops
    lanes = None
    if args.lanes > 1:
        lanes = [torch.cuda.Stream() for _ in range(args.lanes)]
        for ln in lanes:
            ln.wait_stream(torch.cuda.current_stream())

    # Step order.  A step = analysis (+ hyperprior branch, rate, coder start) of one batch and synthesis (+ metrics) of one
    # batch.  By default the analysis runs ONE BATCH AHEAD of the synthesis (A0 A1 S0 A2 S1 ... S(K-1): K analyses and K
    # syntheses inside the timed region, every batch complete before the clock stops): the serial range coder of a batch
    # (4.4 ms) then hides behind the syntheses of two batches instead of one, and the run no longer ends with 2.5 ms in
    # which only the last batch's coder works.  --no-stagger runs A_i S_i back to back.
    staged = []

    def step():
        # range coder of this batch runs on a second stream beside synthesis + MS-SSIM
        if args.no_stagger or lanes is not None:
            out = model(x, quant_mode="round", after_rate=coder)
            return finish(out, coder.last if coder is not None else None)
        st = model.encode_stage(x, quant_mode="round", after_rate=coder)
        staged.append((st, coder.last if coder is not None else None))
        if len(staged) < 2:
            return None
        st, clast = staged.pop(0)
        return finish(model.decode_stage(st), clast)

    def drain():
        # the synthesis (+ metrics) the staggered order still owes at the end
        while staged:
            st, clast = staged.pop(0)
            finish(model.decode_stage(st), clast)

    def finish(out, clast):
        bpp = out.sums.sum(dim=1) / float(H * W)                 # per image (modelseval.py:90-94)
        msssim = metrics.ms_ssim_per_image(out["x_hat"], x, clamp_x=True)
        real = zero
        if coder is not None:
            # the strings of THIS step are still being coded beside synthesis (and the next steps'
            # analysis); the coded size that enters this step's reduction is that of the step
            # `coder_depth` earlier (same batch), joined at stream level without a host sync.  The
            # last steps are joined before the clock stops.
            pending.append(clast)
            if len(pending) > max(1, args.coder_depth):
                prev = pending.pop(0)
                torch.cuda.current_stream().wait_event(prev["done"])
                real = prev["lengths"].sum().double() * 8.0 / float(H * W)   # eval_selfcontained_entropy.py:148-149
        t = torch.stack([bpp.sum(), msssim.double().sum(), count, real])
        D.reduce_metric_sums(t)                                  # the one collective: 4 x fp64
        totals.copy_(t)
        last_step.update(out=out, bpp=bpp, msssim=msssim)        # what the caller of this step receives
        return out

    def barrier():
        D.barrier()
        torch.cuda.synchronize()

    # warm-up; its last step runs with the kernel timer on so that the event pool (and the coder's)
    # exists before the clock starts
    def run_step(i):
        if lanes is None:
            return step()
        with torch.cuda.stream(lanes[i % len(lanes)]):
            return step()

    for i in range(max(args.warmup, args.lanes if lanes else 0)):
        timer.enabled = i == max(args.warmup, args.lanes if lanes else 0) - 1
        run_step(i)
    timer.enabled = False
    drain()                      # (outside the bracketed step: the dominant symbol is picked from ONE analysis + ONE synthesis)
    per_step = timer.used + 1
    if not args.kernels:
        # An event pair costs the queue ~11 us per launch (two markers the command processor serialises on):
        # with every conv launch bracketed that is ~0.3 ms = 4 % of a step.  The timed region therefore
        # brackets only the launches of the dominant kernel symbol, found from the fully bracketed last
        # warm-up step; --kernels brackets everything (and says so in the JSON).
        torch.cuda.synchronize()
        warm = timer.summary()
        if warm:
            timer.only = {max(warm.items(), key=lambda kv: kv[1][1])[0]}
    if kernel_events:
        timer.reserve(per_step * args.steps + 8)
    else:
        timer.events = False     # the timed steps only note the dominant symbol (it names `dtype`), no events
    if coder is not None:
        coder.reserve_events(args.steps + 1)
    model.reserve_stage_events(args.steps + 2)
    timer.reset()
    barrier()
    timer.enabled = True
    marks = []
    t0 = time.perf_counter()
    for i in range(args.steps):
        if kernel_events:
            marks.append(timer.mark())
        run_step(i)
    drain()
    if lanes is not None:
        for ln in lanes:
            torch.cuda.current_stream().wait_stream(ln)
    if coder is not None:
        last = coder.wait()                                      # strings of the final step
        extra = torch.zeros(4, dtype=torch.float64, device=dev)
        extra[3] = last["lengths"].sum().double() * 8.0 / float(H * W)
        D.reduce_metric_sums(extra)
        totals[3] = extra[3]
    barrier()
    elapsed = time.perf_counter() - t0
    timer.enabled = False
    elapsed = D.max_over_ranks(elapsed, dev)

    tot = totals.cpu().numpy()
    n_img = tot[2]
    value = args.steps * B * world / elapsed
    if coder is not None:
        err = int(coder.last["err"].item())
        if err:
            raise SystemExit(f"range coder reported error flags {err:#x} (support wider than Lmax?): mean_bpp_coded would be wrong")
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, last_step["out"], last_step["bpp"], last_step["msssim"], totals,
                     coder.last if coder is not None else None)

    decoder_stats = e2e_stats = None
    if args.decode and rank == 0:
        # Decode side: the strings of one batch as Python bytes (the reference's dict) -> upload, z tables,
        # range decode z, h_s, y tables, range decode y, g_s, clamp.  Wall time per call, host work included.
        comp = entropy.custom_compress(model, x)
        ref_hat = model(x, quant_mode="round")["x_hat"].clamp(0, 1)
        x_dec = entropy.custom_decompress(model, comp)
        exact = bool(torch.equal(x_dec, ref_hat))
        torch.cuda.synchronize()
        reps = max(3, min(args.steps, 10))
        td = time.perf_counter()
        for _ in range(reps):
            entropy.custom_decompress(model, comp)
        torch.cuda.synchronize()
        dms = (time.perf_counter() - td) / reps * 1e3
        n_sym = B * (model.M * (H // 16) * (W // 16) + model.N * (H // 64) * (W // 64))
        decoder_stats = {
            "ms_per_batch": dms, "images_per_s": B / dms * 1e3, "symbols_per_s": n_sym / dms * 1e3,
            "string_bytes_per_batch": sum(len(t) for e in comp["strings"] for t in e),
            "round_trip_exact": exact,
            "note": "entropy.custom_decompress of the batch's strings held as Python bytes (upload + both range decodes "
                    "+ h_s + g_s), wall time of back-to-back calls; one wave per string",
        }
    if args.e2e and rank == 0 and coder is not None and C in (1, 3, 4):
        # Host to host: uint8 HWC images in pinned memory -> H2D on a copy stream -> forward with the fused to_tensor
        # ingest (dsic_conv_first_u8hwc) + metrics + coder -> strings and lengths D2H into pinned memory.
        u8 = (x.permute(0, 2, 3, 1).clamp(0, 1) * 255.0).round().to(torch.uint8).contiguous()
        host_in = u8.cpu().pin_memory()
        dev_in = [torch.empty_like(u8) for _ in range(3)]
        cap = coder.last["bytes"].shape[1]
        host_bytes = [torch.empty((B, cap), dtype=torch.uint8).pin_memory() for _ in range(2)]
        host_len = [torch.empty((B, 2), dtype=torch.int32).pin_memory() for _ in range(2)]
        ms_img = None
        e_staged = []

        def e2e_finish(st, k):
            nonlocal ms_img
            o = model.decode_stage(st)
            xf = dev_in[k].permute(0, 3, 1, 2).float() / 255.0
            ms_img = metrics.ms_ssim_per_image(o["x_hat"], xf, clamp_x=True)

        def e2e_step(i):
            # the same order as the resident step: analysis (+ coder start) of batch i, then synthesis + metrics of
            # batch i - 1 (three input buffers: a batch's image is read again by its MS-SSIM one step later)
            k = i % 3
            # the upload runs on the main stream itself (0.23 ms for 12.6 MB): on a stream of its own it shared a hardware
            # queue with the coder's streams and cost 1.2 ms per step
            dev_in[k].copy_(host_in, non_blocking=True)
            st = model.encode_stage(dev_in[k], quant_mode="round", after_rate=coder)
            last = coder.last
            # on the coder's own side stream, behind the encoder (a sixth stream for the D2H alone shared a hardware
            # queue with the others: +3.5 ms per step)
            with torch.cuda.stream(coder.streams[(coder.calls - 1) % len(coder.streams)]):
                host_bytes[i & 1].copy_(last["bytes"], non_blocking=True)
                host_len[i & 1].copy_(last["lengths"], non_blocking=True)
            e_staged.append((st, k))
            if len(e_staged) > 1:
                e2e_finish(*e_staged.pop(0))

        def e2e_drain():
            while e_staged:
                e2e_finish(*e_staged.pop(0))

        coder.reserve_events(args.steps + 4)      # (creating a HIP event inside the loop stalls the enqueue thread)
        model.reserve_stage_events(args.steps + 5)
        for i in range(3):
            e2e_step(i)
        e2e_drain()
        torch.cuda.synchronize()
        te = time.perf_counter()
        for i in range(args.steps):
            e2e_step(i)
        e2e_drain()
        coder.wait()
        torch.cuda.synchronize()
        ems = (time.perf_counter() - te) / args.steps * 1e3
        e2e_stats = {
            "ms_per_step": ems, "images_per_s": B / ems * 1e3,
            "h2d_bytes_per_step": int(host_in.numel()), "d2h_bytes_per_step": int(B * cap + B * 8),
            "note": "pinned uint8 HWC images -> H2D (main stream) -> dsic_conv_first_u8hwc ... coder -> worst-case string "
                    "buffers + lengths D2H (on the coder's stream, behind the encoder) into pinned memory; copies overlap the next / "
                    "previous batch; same staggered step order as the resident figure",
        }

    if rank == 0:
        agg = timer.summary()
        if args.kernels:
            print("step periods (ms, step-start events on the main stream): "
                  + " ".join(f"{a.elapsed_time(b):.2f}" for a, b in zip(marks, marks[1:])), file=sys.stderr)
            for k, (c, t, f, ex) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
                print(f"{k:40s} {c:5d} launches {t / args.steps * 1e3:8.3f} ms/step  {f / t / 1e12:7.1f} TF/s algorithmic "
                      f"{ex / t / 1e12:7.1f} executed", file=sys.stderr)
        roofline = None
        if kernel_events:
            name, (cnt, secs, flops, exflops) = max(agg.items(), key=lambda kv: kv[1][1])
            executed = exflops / secs / 1e12
            algorithmic = flops / secs / 1e12
            # the split-bf16 Winograd kernels run on the bf16 MFMA path (3 bf16 MFMAs per fp32-equivalent one)
            is_bf16 = "bf16" in name
            peak = PEAK_BF16_MFMA_TFLOPS if is_bf16 else PEAK_FP32_MFMA_TFLOPS
            conv_secs = sum(v[1] for v in agg.values())

            def from_profile(fname, key=None):
                """Numbers of a SEPARATE rocprofv3 --pmc pass, committed under profiles/ (not measured by
                this invocation): returned with the file they come from, or (None, None)."""
                path = os.path.join(ROOT, "profiles", fname)
                if not os.path.exists(path):
                    return None, None
                with open(path) as f:
                    d = json.load(f)
                v = d.get(name)
                if key is not None and isinstance(v, dict):
                    v = v.get(key)
                return v, f"profiles/{fname}" + (f" (commit {d['_commit']})" if "_commit" in d else "")

            traffic, traffic_src = from_profile("pmc_traffic.json")
            mfma_pmc, mfma_src = from_profile("mfma_util.json", "mfma_util")
            if (H, W, C) != (256, 256, 3):
                traffic = traffic_src = mfma_pmc = mfma_src = None      # the committed PMC passes are 256x256x3
            roofline = {
                "bound": "mfma",
                "kernel": name,
                "launches": cnt,
                "avg_launch_ms": secs / cnt * 1e3,
                # FLOPs the kernel's algorithm executes on the MFMA pipe (Winograd F(2x2,3x3) with
                # zero-position skipping: 12.25 of every 25 direct-convolution MACs of a 5x5/s2
                # layer) / its HIP-event time; frac <= 1 by construction
                "achieved": executed,
                "peak": peak,
                "peak_dtype": "bf16 MFMA (fp32 operands split into 2 bf16 planes, 3 products, fp32 accumulate)"
                              if is_bf16 else "fp32-input MFMA",
                "unit": "TFLOP/s",
                "frac": executed / peak,
                "traffic": traffic,
                "traffic_source": traffic_src,
                # direct-convolution FLOP count of SURVEY.md §8(d) / the same time: may exceed the
                # peak because Winograd executes fewer multiplies; not a roofline fraction
                "algorithmic_tflops": algorithmic,
                "algorithmic_over_fp32_mfma_peak": algorithmic / PEAK_FP32_MFMA_TFLOPS,
                "mfma_busy_pmc": mfma_pmc,
                "mfma_busy_source": mfma_src,
                "events": "every conv launch bracketed (--kernels: costs ~4 % of the step)" if timer.only is None
                          else "launches of the dominant symbol bracketed; it was picked from the fully bracketed "
                               "last warm-up step",
            }
            if timer.only is None:
                roofline["all_conv_algorithmic_tflops"] = sum(v[2] for v in agg.values()) / conv_secs / 1e12
                roofline["conv_share_of_step"] = conv_secs / elapsed
        coder_stats = None
        if coder is not None and coder.times:
            ms = [e0.elapsed_time(e1) for e0, e1 in coder.times[-args.steps:]]
            n_sym = B * (model.M * (H // 16) * (W // 16) + model.N * (H // 64) * (W // 64))
            coded_bytes = float(tot[3] / n_img) * H * W / 8.0 * B
            coder_stats = {
                "ms_per_batch": float(np.mean(ms)),
                "symbols_per_s": n_sym / (float(np.mean(ms)) * 1e-3),
                "string_bytes_per_s": coded_bytes / (float(np.mean(ms)) * 1e-3),
                "symbols_per_batch": n_sym,
                "note": "support scan + CDF tables + range encoder of one batch on the side stream, HIP events "
                        "on that stream, while the main stream runs synthesis / MS-SSIM / the next analysis",
            }
        res = {
            "metric": "256x256 satellite patches encoded/s per GPU; bpp + MS-SSIM vs reference",
            "value": value,
            "unit": "images/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,          # BASELINE.md holds no published throughput for this metric
            "dtype": "f32 (Winograd contractions as split-bf16 MFMA with fp32 accumulate)"
                     if any("bf16" in k for k in timer.seen) else "f32",
            "data": "synthetic",
            "config": {
                "workload": f"batch={B}/GPU {H}x{W}x{C} synthetic patches, modelv2 encode->decode "
                            "(g_a,h_a,round,h_s,Student-t/Gaussian rate,g_s) + bpp + MS-SSIM[.3,.5,.2] on GPU"
                            + (" [BASELINE config 2]" if args.no_entropy else
                               " + CDF tables and range coder (z,y strings) on GPU [BASELINE config 3]")
                            + ("" if (H, W, C) == (256, 256, 3) else " [shape of BASELINE config 5]")
                            + (" [spatial_params=True: per-element sigma/nu and coder tables]" if spatial else ""),
                "global_batch": B * world,
                "parallelism": f"per-image sharding x{world}, one all-reduce of 4 fp64",
                "weights": "synthetic seed 1 (checkpoints absent from the reference)",
            },
            "mean_bpp": float(tot[0] / n_img),
            "mean_ms_ssim": float(tot[1] / n_img),
            "mean_bpp_coded": (float(tot[3] / n_img) if not args.no_entropy else None),
            "images_per_s_per_gpu": value / world,
            "coder": coder_stats,
            "decoder": decoder_stats,
            "e2e": e2e_stats,
            "roofline": roofline,
        }
        if args.full and world == 1 and not args.no_cpu_baseline:
            # the GPU box gives one job a 16-CPU share of a larger host
            cores = min(len(os.sched_getaffinity(0)), 16)
            with_coder = not args.no_entropy
            v_all, n_all = cpu_baseline(sd, patches, H, W, cores, with_coder, 14.0)
            v_one, n_one = cpu_baseline(sd, patches, H, W, 1, with_coder, 14.0)
            res["cpu_baseline"] = {
                "value": v_all, "unit": "images/s", "cores": cores, "kind": "port",
                "sample": f"{n_all} single-image calls of the oracle (eager-fp32 forward of oracle/ref_model.py, "
                          "verified against the imported reference in the build container, + bpp + "
                          "MS-SSIM[.3,.5,.2]" + (" + per-image CDF tables and range coder of oracle/entropy_ref.c"
                                                  if with_coder else "")
                          + f"), median; 1 thread: {v_one:.3f} images/s over {n_one} images (cpu.sbatch:5 requests 1 CPU)",
                "value_1thread": v_one,
            }
            res["vs_cpu_baseline"] = value / v_all        # context only: the roofline fraction is the quality measure
        print(json.dumps(res))
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
