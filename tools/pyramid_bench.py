#!/usr/bin/env python3
"""Timings of the overview pyramid (codec.compress_image(..., overviews=n), csrc/pyramid.hip).

    python tools/pyramid_bench.py halve   [--size 4096] [--json OUT.json]
    python tools/pyramid_bench.py pyramid [--size 2048] [--overviews 3] [--reps 10]
    python tools/pyramid_bench.py levels  [--size 2048] [--overviews 3] [--reps 10]

halve: one dsic_image_halve_u8 / _u16 / _f32 / _valid_u8 / _valid_u16 launch on a size x size x 3 image (the masked
ones with a size x size validity image beside it, about one pixel in eight invalid), device events around back-to-back
launches
that walk through enough distinct images (over 512 MB) that no launch finds its source in the last-level cache; beside
it the bytes the launch moves (source read once, destination written once) over the copy bandwidth of tools/hbm_bw.py's
probe (2.1 GB read and written), taken in the same process.
pyramid: compress_image(img, overviews=n) of one uint8 image that lies on the host, host clock around the call (it
returns the stream's bytes, so the device has finished).  levels: the n + 1 plain compress_image calls on the level
images, halved with NumPy beforehand and lying on the host, one after the other; this mode uses nothing of the
pyramid and runs on a tree without it.  Both print the median, the fastest and the slowest of --reps calls."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _halve_u8(img):
    """pyramid.hip's uint8 arithmetic in NumPy: ceil sizes, the last row / column repeated, (a + b + c + d + 2) >> 2"""
    import numpy as np
    y = 2 * np.arange((img.shape[0] + 1) // 2)
    x = 2 * np.arange((img.shape[1] + 1) // 2)
    y1, x1 = np.minimum(y + 1, img.shape[0] - 1), np.minimum(x + 1, img.shape[1] - 1)
    v = img.astype(np.int32)
    return ((v[y][:, x] + v[y][:, x1] + v[y1][:, x] + v[y1][:, x1] + 2) >> 2).astype(np.uint8)


def _scene(size, tile=256):
    """synthetic patches laid side by side, uint8 [size, size, 3] (tools/image_codec_bench.py's scene)"""
    import numpy as np
    from dsic_amd import synthetic as S
    per = size // tile
    p = S.make_patches(0, per * per, tile, tile)
    return (p.reshape(per, per, 3, tile, tile).transpose(0, 3, 1, 4, 2).reshape(size, size, 3) * 255 + 0.5).astype(np.uint8)


def _model():
    import torch
    from dsic_amd import synthetic as S
    from dsic_amd.model import CompressionModel
    sd = S.make_state_dict(seed=1)
    model = CompressionModel(N=128, M=192, spatial_params=False, min_nu=2, max_nu=100.0)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return model.cuda().eval()


def _event_ms(fn, count):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(count):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / count


def halve(a):
    import torch
    from dsic_amd import lib
    from dsic_amd.ops import _p, _stream
    L = lib.load()
    n, h = a.size, (a.size + 1) // 2
    # the probe: tools/hbm_bw.py's copy
    x = torch.empty(64 * 256 * 256 * 128, dtype=torch.float32, device="cuda").fill_(1.0)
    y = torch.empty_like(x)
    _event_ms(lambda i: y.copy_(x), 3)
    copy_ms = _event_ms(lambda i: y.copy_(x), 10)
    copy_tbs = 2 * x.numel() * 4 / 1e9 / copy_ms
    del x, y
    res = {"size": n, "probe_copy_TBps": round(copy_tbs, 3), "kinds": {}}
    for kind in ("u8", "u16", "f32", "valid_u8", "valid_u16"):
        if kind == "f32":
            src_bytes, dst_bytes = 4 * n * n * 3, 4 * h * h * 3
            k = -(-512 * 2 ** 20 // src_bytes)
            srcs = [torch.rand((3, n, n), dtype=torch.float32, device="cuda") for _ in range(k)]
            dsts = [torch.empty((3, h, h), dtype=torch.float32, device="cuda") for _ in range(k)]
            fn = lambda i: L.dsic_image_halve_f32(_p(srcs[i % k]), _p(dsts[i % k]), 3, n, n, _stream())
        else:
            wide, masked = kind.endswith("u16"), kind.startswith("valid")
            es = 2 if wide else 1
            src_bytes, dst_bytes = (3 * es + masked) * n * n, (3 * es + masked) * h * h
            k = -(-512 * 2 ** 20 // src_bytes)
            dt = torch.uint16 if wide else torch.uint8
            if wide:                                                     # random bits, seen as uint16
                srcs = [torch.randint(-32768, 32768, (n, n, 3), dtype=torch.int16, device="cuda").view(dt)
                        for _ in range(k)]
            else:
                srcs = [torch.randint(0, 256, (n, n, 3), dtype=dt, device="cuda") for _ in range(k)]
            dsts = [torch.empty((h, h, 3), dtype=dt, device="cuda") for _ in range(k)]
            if masked:
                svals = [(torch.randint(0, 8, (n, n), device="cuda") != 0).to(torch.uint8) for _ in range(k)]
                dvals = [torch.empty((h, h), dtype=torch.uint8, device="cuda") for _ in range(k)]
                call = L.dsic_image_halve_valid_u16 if wide else L.dsic_image_halve_valid_u8
                fn = lambda i: call(_p(srcs[i % k]), _p(svals[i % k]), _p(dsts[i % k]), _p(dvals[i % k]), n, n, 3,
                                    _stream())
            else:
                call = L.dsic_image_halve_u16 if wide else L.dsic_image_halve_u8
                fn = lambda i: call(_p(srcs[i % k]), _p(dsts[i % k]), n, n, 3, _stream())
        lib.check(fn(0), "image_halve_" + kind)
        _event_ms(fn, 2 * k)
        runs = [_event_ms(fn, 10 * k) for _ in range(5)]
        ms = statistics.median(runs)
        moved = src_bytes + dst_bytes
        res["kinds"][kind] = {"images": k, "launches_per_run": 10 * k, "ms_per_launch": round(ms, 5),
                              "ms_runs": [round(r, 5) for r in runs], "bytes_moved": moved,
                              "TBps": round(moved / 1e9 / ms, 3),
                              "floor_ms_at_probe": round(moved / 1e9 / copy_tbs, 5)}
        del srcs, dsts, fn
        svals = dvals = None
    return res


def end_to_end(a):
    import torch
    from dsic_amd import codec
    model = _model()
    levels = [_scene(a.size)]
    for _ in range(a.overviews):
        levels.append(_halve_u8(levels[-1]))
    host = [torch.from_numpy(lv) for lv in levels]
    if a.mode == "pyramid":
        call = lambda: [codec.compress_image(model, host[0], tile=a.tile, batch=a.batch, overviews=a.overviews)]
    else:
        call = lambda: [codec.compress_image(model, lv, tile=a.tile, batch=a.batch) for lv in host]
    for _ in range(3):
        out = call()
    times = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        times.append((time.perf_counter() - t0) * 1e3)
    return {"mode": a.mode, "size": a.size, "overviews": a.overviews, "tile": a.tile, "batch": a.batch,
            "reps": a.reps, "stream_bytes": sum(len(s) for s in out), "ms_median": round(statistics.median(times), 3),
            "ms_min": round(min(times), 3), "ms_max": round(max(times), 3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("mode", choices=("halve", "pyramid", "levels"))
    ap.add_argument("--size", type=int, default=None)
    ap.add_argument("--overviews", type=int, default=3)
    ap.add_argument("--tile", type=int, default=256)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.size is None:
        a.size = 4096 if a.mode == "halve" else 2048
    res = halve(a) if a.mode == "halve" else end_to_end(a)
    print(json.dumps(res))
    if a.json:
        with open(a.json, "a") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
