#!/usr/bin/env python3
"""Timing of the entropy path stages at the bench shape (diagnostic).

    python tools/entropy_bench.py [--segments 8] [--reps 7] [--json OUT]
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/entropy_bench.py --segments 8
    python tools/entropy_bench.py --kernel-trace DIR/.../*_kernel_trace.csv [--json OUT]

--segments K   the coder with the y strings whole (K = 1) and in K segments, read alternately in one run; every figure is
               the median of --reps readings, each the mean of 5 calls between two events.
--kernel-trace summarises a rocprofv3 kernel trace of such a run (no GPU needed): per kernel and grid size the number of
               launches and the median microseconds.  enc_chain_kernel runs one 64-lane workgroup per string, so its
               grid tells the whole strings (2 B workgroups) from the segmented ones ((K + 1) B).
"""
import argparse, csv, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def kernel_trace(path):
    rows = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"].split("(")[0]
            grid = int(r["Grid_Size_X"]) * int(r.get("Grid_Size_Y", 1) or 1) * int(r.get("Grid_Size_Z", 1) or 1)
            rows.setdefault((name, grid), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return [{"kernel": k, "grid": g, "launches": len(v), "median_us": round(statistics.median(v), 2),
             "min_us": round(min(v), 2)} for (k, g), v in sorted(rows.items())]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=1)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--json", default=None)
    ap.add_argument("--kernel-trace", default=None)
    a = ap.parse_args()
    if a.kernel_trace:
        res = {"kernels": [r for r in kernel_trace(a.kernel_trace) if "enc_" in r["kernel"] or "range_" in r["kernel"]
                           or "tables" in r["kernel"] or "support" in r["kernel"]]}
        for r in res["kernels"]:
            print(f"{r['kernel']:<60} grid {r['grid']:>8}  x{r['launches']:<4} median {r['median_us']:>10.2f} us")
    else:
        res = measure(a)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


def measure(a):
    import torch
    from dsic_amd import entropy, synthetic as S
    from dsic_amd.model import CompressionModel

    B = int(os.environ.get("B", "64"))
    sd = S.make_state_dict(seed=1)
    m = CompressionModel(min_nu=2).cuda().eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    x = torch.from_numpy(S.make_patches(0, B, 256, 256)).cuda()
    out = m(x, "round")
    sy, ny = out["sigma"][:, :, 0, 0].contiguous(), out["nu"][:, :, 0, 0].contiguous()
    sz = torch.exp(m.z_prior.log_sigma)

    def timeit(f, reps=5):
        f(); torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps): f()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    meta = entropy.latent_support(out["y_tilde"], out["z_tilde"])
    res = {"B": B, "reps": a.reps}
    res["support_ms"] = timeit(lambda: entropy.latent_support(out["y_tilde"], out["z_tilde"]))
    res["tables_ms"] = timeit(lambda: entropy.cdf_tables(sy, ny, sz, meta))
    res["forward_ms"] = timeit(lambda: m(x, "round"))
    print("support   %.3f ms" % res["support_ms"])
    print("tables    %.3f ms" % res["tables_ms"])
    print("forward   %.3f ms" % res["forward_ms"])
    Ks = [1] if a.segments == 1 else [1, a.segments]
    reads = {K: [] for K in Ks}
    for _ in range(a.reps):                      # alternately, so that a drift of the clocks meets both alike
        for K in Ks:
            reads[K].append(timeit(lambda: entropy.compress_latents(out["y_tilde"], out["z_tilde"], sy, ny, sz,
                                                                    segments=K)))
    res["compress_ms"] = {}
    for K in Ks:
        c = entropy.compress_latents(out["y_tilde"], out["z_tilde"], sy, ny, sz, segments=K)
        med = statistics.median(reads[K])
        res["compress_ms"][str(K)] = {"median": round(med, 3), "all": [round(v, 3) for v in reads[K]],
                                      "bytes_per_image": float(c["lengths"].sum().item()) / B}
        print("compress  %.3f ms (support+tables+encode), segments=%d, median of %d (%.3f .. %.3f); err %d, "
              "bytes/img %.1f" % (med, K, a.reps, min(reads[K]), max(reads[K]), int(c["err"].item()),
                                  res["compress_ms"][str(K)]["bytes_per_image"]))
    print("meta0", c["meta"][0].tolist())
    # the coder on its side stream beside the forward pass that follows it (AsyncCompressor, as bench.py's config 3):
    # ms from the coder's first launch to its last, and of the step
    coders = {K: entropy.AsyncCompressor(m, segments=K) for K in Ks}
    beside = {K: {"coder": [], "step": []} for K in Ks}
    for coder in coders.values():
        coder.timing = True
        for _ in range(3):
            m(x, quant_mode="round", after_rate=coder)
        coder.wait(); torch.cuda.synchronize()
        coder.times.clear()
    for _ in range(a.reps):
        for K in Ks:
            coder = coders[K]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(4):
                m(x, quant_mode="round", after_rate=coder)
            coder.wait()
            e1.record(); torch.cuda.synchronize()
            beside[K]["step"].append(e0.elapsed_time(e1) / 4)
            beside[K]["coder"].append(statistics.median(s0.elapsed_time(s1) for s0, s1 in coder.times))
            coder.times.clear()
    res["beside_forward_ms"] = {}
    for K in Ks:
        cm, sm = statistics.median(beside[K]["coder"]), statistics.median(beside[K]["step"])
        res["beside_forward_ms"][str(K)] = {"coder": round(cm, 3), "step": round(sm, 3),
                                            "coder_all": [round(v, 3) for v in beside[K]["coder"]],
                                            "step_all": [round(v, 3) for v in beside[K]["step"]]}
        print("beside a forward pass, segments=%d: coder %.3f ms per batch, step %.3f ms (medians of %d)"
              % (K, cm, sm, a.reps))
    return res


if __name__ == "__main__":
    main()
