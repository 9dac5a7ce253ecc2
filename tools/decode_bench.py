#!/usr/bin/env python3
"""Timing of custom_decompress and of its range-decode launches at the bench shape (diagnostic).

    python tools/decode_bench.py [--segments 8] [--reps 7] [--json OUT]

--segments K: the y strings whole (K = 1) and in K segments (one wave per segment), read alternately in one run; every
figure is the median of --reps readings, each the mean of 3 calls."""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from dsic_amd import entropy, ops, lib as _lib, synthetic as S
from dsic_amd.entropy import _p, _stream, _upload_strings, sigma_z_of, DEFAULT_LMAX
from dsic_amd.model import CompressionModel
ap = argparse.ArgumentParser()
ap.add_argument("--segments", type=int, default=1)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--json", default=None)
a = ap.parse_args()
Ks = [1] if a.segments == 1 else [1, a.segments]
B = int(os.environ.get("B", "64"))
m = CompressionModel(min_nu=2).cuda().eval()
m.load_state_dict({k: torch.from_numpy(v) for k, v in S.make_state_dict(seed=1).items()})
x = torch.from_numpy(S.make_patches(0, B, 256, 256)).cuda()
cs = {K: entropy.custom_compress(m, x, segments=K) for K in Ks}
c = cs[1]
ref = entropy.custom_decompress(m, c)
for K in Ks:
    assert torch.equal(entropy.custom_decompress(m, cs[K]), ref), f"segments={K} decodes to another image"
torch.cuda.synchronize()


def whole(K):
    t0 = time.perf_counter()
    for _ in range(3): entropy.custom_decompress(m, cs[K])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / 3 * 1e3


reads = {K: [] for K in Ks}
for _ in range(a.reps):
    for K in Ks:
        reads[K].append(whole(K))
res = {"B": B, "reps": a.reps, "custom_decompress_ms": {}, "range_decode_y_ms": {}}
for K in Ks:
    dt = statistics.median(reads[K])
    res["custom_decompress_ms"][str(K)] = {"median": round(dt, 3), "all": [round(v, 3) for v in reads[K]]}
    print(f"custom_decompress (incl. H2D), segments={K}: {dt:.1f} ms per batch of {B} -> {B/dt*1e3:.0f} patches/s "
          f"(median of {a.reps}: {min(reads[K]):.1f} .. {max(reads[K]):.1f})")

# the two range-decode launches alone
dev = x.device
L = _lib.load()
_, M, Hy, Wy = c["shape_y"]; _, N, Hz, Wz = c["shape_z"]
meta_np = np.array([[c["min_y"][b], c["max_y"][b] - c["min_y"][b] + 1, c["min_z"][b], c["max_z"][b] - c["min_z"][b] + 1]
                    for b in range(B)], dtype=np.int32)
Lmax = max(DEFAULT_LMAX, int(meta_np[:, [1, 3]].max()))
print("support widths L_y min/median/max", int(meta_np[:, 1].min()), int(np.median(meta_np[:, 1])), int(meta_np[:, 1].max()),
      " L_z", int(meta_np[:, 3].min()), int(meta_np[:, 3].max()), " Lmax", Lmax)
meta = torch.from_numpy(meta_np).to(dev)
err = torch.zeros(1, dtype=torch.int32, device=dev)
tab_z = torch.zeros((B, N, Lmax), dtype=torch.uint16, device=dev)
_lib.check(L.dsic_cdf_tables_gauss(_p(sigma_z_of(m)), _p(meta), _p(tab_z), B, N, Lmax, _p(err), _stream()), "tables")
zbuf, zlen, zstride = _upload_strings(c["strings"], 0, dev)
z_hat = torch.empty((B, N, Hz, Wz), dtype=torch.float32, device=dev)
dec_z = lambda: _lib.check(L.dsic_range_decode(_p(zbuf), zstride, _p(zlen), 1, 0, _p(meta), 2, _p(tab_z), Lmax, B, N, Hz * Wz, 0,
                                               _p(z_hat), _p(err), _stream()), "decode z")
dec_z()
(_, _, sigma_y, nu_y), _ = m.h_s.params_nhwc(ops.nchw_to_nhwc(z_hat), m.min_nu, m.max_nu)
tab_y = torch.zeros((B, M, Lmax), dtype=torch.uint16, device=dev)
_lib.check(L.dsic_cdf_tables_student(_p(sigma_y.contiguous()), _p(nu_y.contiguous()), _p(meta), _p(tab_y), B, M, Lmax, _p(err),
                                     _stream()), "tables y")
y_hat = torch.empty((B, M, Hy, Wy), dtype=torch.float32, device=dev)
bufs = {K: _upload_strings(cs[K]["strings"], 1, dev) for K in Ks}
segl = {K: torch.tensor(cs[K]["seg_lengths_y"], dtype=torch.int32, device=dev) for K in Ks if K > 1}


def dec_y(K):
    ybuf, ylen, ystride = bufs[K]
    if K == 1:
        _lib.check(L.dsic_range_decode(_p(ybuf), ystride, _p(ylen), 1, 0, _p(meta), 0, _p(tab_y), Lmax, B, M, Hy * Wy, 0,
                                       _p(y_hat), _p(err), _stream()), "decode y")
    else:
        _lib.check(L.dsic_range_decode_seg(_p(ybuf), ystride, _p(ylen), 1, 0, _p(segl[K]), K, _p(meta), 0, _p(tab_y), Lmax,
                                           B, M, Hy * Wy, 0, _p(y_hat), _p(err), _stream()), "decode y segments")


def launch_ms(f):
    f(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(3): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 3


ms = launch_ms(dec_z)
res["range_decode_z_ms"] = round(ms, 4)
print(f"range_decode z: {ms:.3f} ms per launch, {ms * 1e6 / (N * Hz * Wz):.0f} ns per symbol of a string ({B} strings side by side)")
out = m(x, "round")
reads = {K: [] for K in Ks}
for _ in range(a.reps):
    for K in Ks:
        reads[K].append(launch_ms(lambda: dec_y(K)))
for K in Ks:
    y_hat.zero_()
    dec_y(K)
    ok = bool(torch.equal(y_hat, out["y_tilde"]))
    ms = statistics.median(reads[K])
    res["range_decode_y_ms"][str(K)] = {"median": round(ms, 4), "all": [round(v, 4) for v in reads[K]], "exact": ok}
    print(f"range_decode y, segments={K}: {ms:.3f} ms per launch (median of {a.reps}: {min(reads[K]):.3f} .. "
          f"{max(reads[K]):.3f}), {ms * 1e6 * K / (M * Hy * Wy):.0f} ns per symbol of a string ({B * K} strings side by "
          f"side); decoded y equals the encoder's latents: {ok}, err {int(err.item())}")
if len(Ks) > 1:
    r = res["range_decode_y_ms"][str(Ks[1])]["median"] / res["range_decode_y_ms"]["1"]["median"]
    res["range_decode_y_ratio"] = round(r, 4)
    print(f"range_decode y: segments={Ks[1]} takes {r:.3f} of segments=1")
if a.json:
    with open(a.json, "w") as f:
        json.dump(res, f, indent=1)
