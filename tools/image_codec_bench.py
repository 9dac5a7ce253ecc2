"""Tiles per second of the whole-image codec on a synthetic scene, against the host-packed path on the same tiles.

    python tools/image_codec_bench.py [--size 4096] [--tile 256] [--batch 64] [--reps 3] [--json OUT]
    python tools/image_codec_bench.py --overlap 16,32 [--json profiles/overlap_bench.json]

device path  compress_image (gather on the device, compress_to_container per batch) and decompress_image
             (decompress_container per batch, stitched into a uint8 image);
host path    the same tiles through custom_compress + pack_container, and unpack_container + custom_decompress.
Every figure is the best of --reps full passes over the scene after one warm-up pass, wall clock, synchronised.

    python tools/image_codec_bench.py --region [--json profiles/region_decode_bench.json]

--segments K  (with or without --region) the same figures for streams whose y strings are whole (K = 1) and in K
          segments, read alternately in one run, each the median of --reps readings; "segments" in the result holds
          them per K beside the stream-size ratio.  The K = 1 stream's figures stay where they were.

--overlap O[,O2...]  overlapped tiles with blended seams: streams of overlap 0 and of every O given, read alternately
          in one run (medians of --reps readings): stream bytes and tile counts against overlap 0, compress_image /
          decompress_image in tiles per second, and a seam figure: the mean absolute step of the reconstruction error
          x_hat - x across the nominal tile boundaries of each stream's own grid, relative to its mean step at all other
          rows and columns (the error, not the image, because the synthetic scene has edges of its own every 256
          pixels).  With synthetic weights the seam figure shows the mechanism, not a trained model's quality.
          Written to profiles/overlap_bench.json (or --json).  Records, not bars.

--max-error T[,T2...]  the near-lossless mode: the lossy stream and a stream of every T given, read alternately in one
          run (medians of --reps readings): stream bytes split into the lossy and the residual layer, the worst pixel
          error of the decode, compress_image / decompress_image and a one-tile decompress_region in ms.  Written to
          profiles/near_lossless_bench.json (or --json).  Records, not bars.

--nodata  nodata masks: the scene with a wedge of fill pixels (value 0) that empties about a third of its tiles, coded
          without nodata and with nodata=0, read alternately in one run (medians of --reps readings): stream bytes, the
          mask block's bytes, tile states, compress_image / decompress_image and decompress_region of one empty and of
          one full tile in ms, and the classify pass alone.  Written to profiles/nodata_bench.json (or --json).
          Records, not bars.

--u16     16-bit imagery: the scene as uint8 and as uint16 [H,W,3] (another offset and span per band; stream version 6),
          once with scale=None (one more pass over the scene, dsic_band_range_u16) and once with the scale given, read
          alternately in one run (medians of --reps readings): stream bytes, compress_image / decompress_image and a
          four-tile decompress_region in ms, and the band-range pass alone.  Written to profiles/u16_bench.json (or
          --json).  Records, not bars.

--tolerance T[,T2...]  the bounded-error mode of 16-bit imagery: a four-band uint16 scene over (0, 10000), its
          version-6 stream and a version-9 stream of every T given, read alternately in one run (medians of --reps
          readings): stream bytes split into the lossy and the residual layer, residual bits per sample beside the
          empirical entropy of q (so that the overhead of the per-tile split shows), the tiles per shift k, the worst
          error of the decode, compress_image / decompress_image and a one-tile decompress_region in ms.  Written to
          profiles/tolerance_u16_bench.json (or --json).  Records, not bars.

--region  decompress_region of the same stream for an aligned one-tile window, an unaligned 2 x 2-tile-sized window
          (9 tiles), an unaligned half-scene window and the whole image, beside decompress_image before and after
          them in the same run (the two readings show the run-to-run spread).  Records, not bars.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _times(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def _best(fn, reps):
    return min(_times(fn, reps))


def region_records(model, stream, a):
    """decompress_region on four windows of the scene beside decompress_image, one run."""
    import torch
    from dsic_amd import codec
    t, size = a.tile, a.size
    off = 4 * t - 24                                       # not a multiple of 16: ragged row ends on every tile
    windows = [("tile_aligned", (4 * t, 4 * t, t, t)), ("unaligned_2x2", (off, off, 2 * t, 2 * t)),
               ("unaligned_half", (off, off, size // 2, size // 2)), ("whole_image", (0, 0, size, size))]

    def ms(ts):
        return [round(1e3 * v, 3) for v in ts]

    full = codec.decompress_image(model, stream)
    before = _times(lambda: codec.decompress_image(model, stream), a.reps)
    recs = {}
    for name, win in windows:
        stats = {}
        got = codec.decompress_region(model, stream, *win, batch=a.batch, stats=stats)
        y0, x0, h, w = win
        assert torch.equal(got, full[y0:y0 + h, x0:x0 + w]), f"{name}: the window differs from the full decode"
        ts = _times(lambda: codec.decompress_region(model, stream, *win, batch=a.batch), a.reps)
        recs[name] = {"window_y0_x0_h_w": list(win), "ms": min(ms(ts)), "ms_all": ms(ts),
                      "tiles_decoded": len(stats["tiles"]), "decode_batches": stats["decode_batches"],
                      "bytes_uploaded": stats["bytes_uploaded"], "bytes_read": stats["bytes_read"]}
    after = _times(lambda: codec.decompress_image(model, stream), a.reps)
    best_full = min(before + after)
    ix = codec.stream_index(stream)
    return {"scene": f"{size}x{size}x3 uint8", "tiles": ix["grid"]["n"], "tile": t, "batch": a.batch,
            "stream_bytes": len(stream), "reps": a.reps,
            "decompress_image": {"ms": round(1e3 * best_full, 3), "ms_before": ms(before), "ms_after": ms(after),
                                 "tiles_decoded": ix["grid"]["n"], "decode_batches": ix["batches"]},
            "decompress_region": recs,
            "whole_image_over_decompress_image": round(recs["whole_image"]["ms"] / (1e3 * best_full), 4),
            "unaligned_2x2_over_decompress_image": round(recs["unaligned_2x2"]["ms"] / (1e3 * best_full), 4)}


def segment_records(model, img, a, n):
    """K = 1 and K = a.segments alternately: compress_image / decompress_image tiles per second and, with --region,
    the one-tile and nine-tile windows; medians of a.reps readings."""
    import statistics
    import torch
    from dsic_amd import codec
    t = a.tile
    off = 4 * t - 24
    Ks = [1, a.segments]
    streams = {K: codec.compress_image(model, img, tile=t, batch=a.batch, segments=K) for K in Ks}
    full = codec.decompress_image(model, streams[1])
    assert torch.equal(codec.decompress_image(model, streams[a.segments]), full), "segments decode to another image"
    jobs = {"compress_image": lambda K: codec.compress_image(model, img, tile=t, batch=a.batch, segments=K),
            "decompress_image": lambda K: codec.decompress_image(model, streams[K])}
    if a.region:
        jobs["region_one_tile"] = lambda K: codec.decompress_region(model, streams[K], 4 * t, 4 * t, t, t, batch=a.batch)
        jobs["region_nine_tiles"] = lambda K: codec.decompress_region(model, streams[K], off, off, 2 * t, 2 * t,
                                                                      batch=a.batch)
    reads = {name: {K: [] for K in Ks} for name in jobs}
    for name, job in jobs.items():
        for K in Ks:
            job(K)                                                     # warm-up
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for K in Ks:
                t0 = time.perf_counter()
                job(K)
                torch.cuda.synchronize()
                reads[name][K].append(1e3 * (time.perf_counter() - t0))
    res = {"K": a.segments, "reps": a.reps, "stream_bytes": {str(K): len(streams[K]) for K in Ks},
           "stream_size_ratio": round(len(streams[a.segments]) / len(streams[1]), 6)}
    for name in jobs:
        res[name] = {}
        for K in Ks:
            med = statistics.median(reads[name][K])
            res[name][str(K)] = {"ms_median": round(med, 3), "ms_all": [round(v, 3) for v in reads[name][K]]}
            if name in ("compress_image", "decompress_image"):
                res[name][str(K)]["tiles_per_s"] = round(n / med * 1e3, 1)
    return res


def _seam_figure(err, g):
    """err float32 [C,H,W] (x_hat - x): mean |step| across the nominal tile boundaries over the mean |step| at all
    other rows and columns."""
    import torch
    dy = (err[:, 1:, :] - err[:, :-1, :]).abs().mean(dim=(0, 2))       # step between rows r and r+1, at index r
    dx = (err[:, :, 1:] - err[:, :, :-1]).abs().mean(dim=(0, 1))
    at, off = [], []
    for d, own in ((dy, g["own_y"]), (dx, g["own_x"])):
        seam = torch.zeros(d.numel(), dtype=torch.bool, device=d.device)
        for a, _ in own[1:]:
            if a - 1 < d.numel():
                seam[a - 1] = True
        at.append(d[seam])
        off.append(d[~seam])
    at, off = torch.cat(at), torch.cat(off)
    return {"mean_step_at_boundaries": float(at.mean()), "mean_step_elsewhere": float(off.mean()),
            "ratio": round(float(at.mean() / off.mean()), 4), "boundaries": int(at.numel())}


def overlap_records(model, img, a, overlaps):
    """Overlap 0 and every O of `overlaps`, alternately."""
    import statistics
    import torch
    from dsic_amd import codec
    t = a.tile
    Os = [0] + [o for o in overlaps if o]
    streams = {O: codec.compress_image(model, img, tile=t, batch=a.batch, overlap=O) for O in Os}
    grids = {O: codec.stream_index(streams[O])["grid"] for O in Os}
    x = img.permute(2, 0, 1).to(torch.float32).div(255)
    seams = {O: _seam_figure(codec.decompress_image(model, streams[O], out="f32") - x, grids[O]) for O in Os}
    jobs = {"compress_image": lambda O: codec.compress_image(model, img, tile=t, batch=a.batch, overlap=O),
            "decompress_image": lambda O: codec.decompress_image(model, streams[O])}
    reads = {name: {O: [] for O in Os} for name in jobs}
    for name, job in jobs.items():
        for O in Os:
            job(O)                                                     # warm-up
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for O in Os:
                t0 = time.perf_counter()
                job(O)
                torch.cuda.synchronize()
                reads[name][O].append(1e3 * (time.perf_counter() - t0))
    res = {"what": "overlap 0 against overlapped tiles with blended seams, read alternately in one run on one MI355X; "
                   "medians.  Synthetic weights: the seam figure shows the mechanism, not a trained model's quality",
           "scene": f"{a.size}x{a.size}x3 uint8", "tile": t, "batch": a.batch, "reps": a.reps, "overlaps": {}}
    for O in Os:
        n = grids[O]["n"]
        rec = {"tiles": n, "grid": f"{grids[O]['ny']}x{grids[O]['nx']}", "stride": grids[O]["sy"],
               "tiles_over_overlap_0": round(n / grids[0]["n"], 4), "stream_bytes": len(streams[O]),
               "bytes_over_overlap_0": round(len(streams[O]) / len(streams[0]), 4),
               "bpp": round(codec.image_bpp(streams[O]), 4), "seam": seams[O]}
        for name in jobs:
            med = statistics.median(reads[name][O])
            rec[name] = {"ms_median": round(med, 3), "ms_all": [round(v, 3) for v in reads[name][O]],
                         "tiles_per_s": round(n / med * 1e3, 1)}
        res["overlaps"][str(O)] = rec
    return res


def near_lossless_records(model, img, a, taus):
    """The lossy stream (None) and max_error = every tau of `taus`, alternately."""
    import statistics
    import torch
    from dsic_amd import codec
    t = a.tile
    modes = [None] + list(taus)
    streams = {m: codec.compress_image(model, img, tile=t, batch=a.batch, max_error=m) for m in modes}
    lossy = codec.unpack_image_stream(streams[None])["blobs"]
    jobs = {"compress_image": lambda m: codec.compress_image(model, img, tile=t, batch=a.batch, max_error=m),
            "decompress_image": lambda m: codec.decompress_image(model, streams[m]),
            "region_one_tile": lambda m: codec.decompress_region(model, streams[m], 4 * t, 4 * t, t, t, batch=a.batch)}
    reads = {name: {m: [] for m in modes} for name in jobs}
    for name, job in jobs.items():
        for m in modes:
            job(m)                                                     # warm-up
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for m in modes:
                t0 = time.perf_counter()
                job(m)
                torch.cuda.synchronize()
                reads[name][m].append(1e3 * (time.perf_counter() - t0))
    res = {"what": "the lossy stream against near-lossless streams (max_error = tau), read alternately in one run on "
                   "one MI355X; medians.  Synthetic weights: the lossy layer predicts poorly, so the residual bytes "
                   "are an upper end, not a trained model's",
           "scene": f"{a.size}x{a.size}x3 uint8", "tile": t, "batch": a.batch, "reps": a.reps, "modes": {}}
    for m in modes:
        u = codec.unpack_image_stream(streams[m])
        out = codec.decompress_image(model, streams[m])
        worst = int((out.to(torch.int16) - img.to(torch.int16)).abs().max())
        rec = {"stream_bytes": len(streams[m]), "lossy_bytes": sum(len(b) for b in u["blobs"]),
               "residual_bytes": sum(len(b) for b in u.get("residuals", [])), "bpp": round(codec.image_bpp(streams[m]), 4),
               "max_abs_error": worst}
        if m is not None:
            assert u["blobs"] == lossy and worst <= m, "the near-lossless stream broke its contract"
        for name in jobs:
            med = statistics.median(reads[name][m])
            rec[name] = {"ms_median": round(med, 3), "ms_all": [round(v, 3) for v in reads[name][m]]}
        res["modes"]["lossy" if m is None else str(m)] = rec
    return res


def nodata_records(model, img, a):
    """The scene with a wedge of nodata, coded without (None) and with nodata = 0, alternately."""
    import statistics
    import torch
    from dsic_amd import codec
    from dsic_amd import mask as _mask
    t, size = a.tile, a.size
    yy = torch.arange(size, device=img.device).view(size, 1)
    xx = torch.arange(size, device=img.device).view(1, size)
    img = img.clone()
    img[(10 * xx < 8 * (size - yy))] = 0                               # 40 % of the pixels, along the top-left edge
    modes = [None, 0]
    streams = {m: codec.compress_image(model, img, tile=t, batch=a.batch, nodata=m) for m in modes}
    ix = codec.stream_index(streams[0])
    states = [r["state"] for r in ix["tiles"]]
    empty, full = states.index(0), len(states) - 1 - states[::-1].index(1)
    g = ix["grid"]
    wins = {"region_empty_tile": (g["own_y"][empty // g["nx"]][0], g["own_x"][empty % g["nx"]][0], t, t),
            "region_full_tile": (g["own_y"][full // g["nx"]][0], g["own_x"][full % g["nx"]][0], t, t)}
    plain = codec.decompress_image(model, streams[None])
    nod = (img == 0).all(dim=2)
    want = torch.where(nod.unsqueeze(2), torch.zeros_like(plain), plain)
    assert torch.equal(codec.decompress_image(model, streams[0]), want), "the masked stream broke its contract"
    jobs = {"compress_image": lambda m: codec.compress_image(model, img, tile=t, batch=a.batch, nodata=m),
            "decompress_image": lambda m: codec.decompress_image(model, streams[m])}
    for name, win in wins.items():
        jobs[name] = lambda m, win=win: codec.decompress_region(model, streams[m], *win, batch=a.batch)
    reads = {name: {m: [] for m in modes} for name in jobs}
    for name, job in jobs.items():
        for m in modes:
            job(m)                                                     # warm-up
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for m in modes:
                t0 = time.perf_counter()
                job(m)
                torch.cuda.synchronize()
                reads[name][m].append(1e3 * (time.perf_counter() - t0))
    cls = [1e3 * v for v in _times(lambda: _mask.classify(img, g, 3, 0), a.reps)]
    res = {"what": "the scene with a wedge of nodata, coded without and with nodata=0, read alternately in one run on "
                   "one MI355X; medians",
           "scene": f"{size}x{size}x3 uint8", "tile": t, "batch": a.batch, "reps": a.reps, "tiles": g["n"],
           "nodata_pixels": int(nod.sum()), "states": {"empty": states.count(0), "full": states.count(1),
                                                       "mixed": states.count(2)},
           "coded_tiles": ix["coded"], "mask_block_bytes": ix["mask_bytes"],
           "mask_modes": {"raw": sum(1 for r in ix["tiles"] if r.get("m_mode") == 0),
                          "list": sum(1 for r in ix["tiles"] if r.get("m_mode") == 1)},
           "windows_y0_x0_h_w": {k: list(v) for k, v in wins.items()},
           "classify": {"ms_median": round(statistics.median(cls), 3), "ms_all": [round(v, 3) for v in cls],
                        "what": "dsic_mask_classify_u8 and the copy of the counts, wall clock",
                        "image_GB_per_s": round(img.numel() / statistics.median(cls) / 1e6, 1)},
           "modes": {}}
    for m in modes:
        rec = {"stream_bytes": len(streams[m]), "bpp": round(codec.image_bpp(streams[m]), 4)}
        for name in jobs:
            med = statistics.median(reads[name][m])
            rec[name] = {"ms_median": round(med, 3), "ms_all": [round(v, 3) for v in reads[name][m]]}
        coded = ix["coded"] if m is not None else g["n"]
        for name in ("compress_image", "decompress_image"):
            rec[name]["ms_per_coded_tile"] = round(rec[name]["ms_median"] / coded, 4)
        res["modes"]["plain" if m is None else f"nodata={m}"] = rec
    return res


def u16_records(model, scene01, img_u8, a):
    """The scene as uint8 and as uint16 (another offset and span per band), coded and decoded alternately; uint16 with
    the bands' own range (one more pass over the scene, dsic_band_range_u16) and with the caller's scale."""
    import statistics
    import numpy as np
    import torch
    from dsic_amd import codec
    t, size = a.tile, a.size
    offs, spans = (100.0, 1000.0, 0.0), (9900.0, 30000.0, 65535.0)
    img16 = torch.from_numpy(np.stack([(o + scene01[..., c].astype(np.float64) * s + 0.5).astype(np.uint16)
                                       for c, (o, s) in enumerate(zip(offs, spans))], axis=2)).cuda()
    own = codec.band_range(img16)
    modes = {"uint8": (img_u8, {}), "uint16, scale=None": (img16, {}), "uint16, scale given": (img16, {"scale": own})}
    streams = {m: codec.compress_image(model, x, tile=t, batch=a.batch, **kw) for m, (x, kw) in modes.items()}
    assert streams["uint16, scale=None"] == streams["uint16, scale given"], "the band range is not the scale written"
    win = (size // 2 - t // 2, size // 2 - t // 2, t, t)                # meets four tiles
    jobs = {"compress_image": lambda m: codec.compress_image(model, modes[m][0], tile=t, batch=a.batch, **modes[m][1]),
            "decompress_image": lambda m: codec.decompress_image(model, streams[m]),
            "decompress_region": lambda m: codec.decompress_region(model, streams[m], *win, batch=a.batch)}
    reads = {name: {m: [] for m in modes} for name in jobs}
    for name, job in jobs.items():
        for m in modes:
            job(m)                                                     # warm-up
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for m in modes:
                t0 = time.perf_counter()
                job(m)
                torch.cuda.synchronize()
                reads[name][m].append(1e3 * (time.perf_counter() - t0))
    rng = [1e3 * v for v in _times(lambda: codec.band_range(img16), a.reps)]
    res = {"what": "the scene as uint8 and as uint16, read alternately in one run on one MI355X; medians",
           "scene": f"{size}x{size}x3", "tile": t, "batch": a.batch, "reps": a.reps, "scale": [list(p) for p in own],
           "window_y0_x0_h_w": list(win),
           "band_range": {"ms_median": round(statistics.median(rng), 3), "ms_all": [round(v, 3) for v in rng],
                          "what": "dsic_band_range_u16 and the copy of the 2 C words, wall clock",
                          "image_GB_per_s": round(2 * img16.numel() / statistics.median(rng) / 1e6, 1)},
           "modes": {}}
    for m in modes:
        rec = {"stream_bytes": len(streams[m]), "bpp": round(codec.image_bpp(streams[m]), 4)}
        for name in jobs:
            rec[name] = {"ms_median": round(statistics.median(reads[name][m]), 3),
                         "ms_all": [round(v, 3) for v in reads[name][m]]}
        res["modes"][m] = rec
    return res


def tolerance_records(a, taus):
    """A four-band uint16 scene over (0, 10000): the version-6 stream (None) and tolerance = every tau of `taus`,
    alternately."""
    import statistics
    import numpy as np
    import torch
    from dsic_amd import codec
    from dsic_amd import synthetic as S
    from dsic_amd.model import CompressionModel
    t, size, C = a.tile, a.size, 4
    sd = S.make_state_dict(seed=1, in_ch=C)
    model = CompressionModel(N=128, M=192, spatial_params=False, min_nu=2, max_nu=100.0, in_ch=C)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    model = model.cuda().eval()
    per = size // t
    p = S.make_patches(0, per * per, t, t, C)
    scene = p.reshape(per, per, C, t, t).transpose(0, 3, 1, 4, 2).reshape(size, size, C).astype(np.float64)
    img = torch.from_numpy((scene * 10000.0 + 0.5).astype(np.uint16)).cuda()
    scale = [(0, 10000)] * C
    modes = [None] + list(taus)
    streams = {m: codec.compress_image(model, img, tile=t, batch=a.batch, scale=scale, tolerance=m) for m in modes}
    lossy = codec.unpack_image_stream(streams[None])["blobs"]
    x = img.to(torch.int32)
    pred = codec.decompress_image(model, streams[None]).to(torch.int32)
    jobs = {"compress_image": lambda m: codec.compress_image(model, img, tile=t, batch=a.batch, scale=scale, tolerance=m),
            "decompress_image": lambda m: codec.decompress_image(model, streams[m]),
            "region_one_tile": lambda m: codec.decompress_region(model, streams[m], 4 * t, 4 * t, t, t, batch=a.batch)}
    reads = {name: {m: [] for m in modes} for name in jobs}
    for name, job in jobs.items():
        for m in modes:
            job(m)                                                     # warm-up
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for m in modes:
                t0 = time.perf_counter()
                job(m)
                torch.cuda.synchronize()
                reads[name][m].append(1e3 * (time.perf_counter() - t0))
    res = {"what": "the version-6 stream of a uint16 scene against bounded-error streams (tolerance = tau), read "
                   "alternately in one run on one MI355X; medians.  Synthetic weights: the lossy layer predicts poorly, "
                   "so the residual bytes are an upper end, not a trained model's",
           "scene": f"{size}x{size}x{C} uint16 over (0, 10000)", "tile": t, "batch": a.batch, "reps": a.reps,
           "samples": size * size * C, "modes": {}}
    for m in modes:
        u = codec.unpack_image_stream(streams[m])
        out = codec.decompress_image(model, streams[m]).to(torch.int32)
        worst = int((out - x).abs().max())
        rbytes = sum(len(b) for b in u.get("residuals", []))
        rec = {"stream_bytes": len(streams[m]), "lossy_bytes": sum(len(b) for b in u["blobs"]), "residual_bytes": rbytes,
               "bpp": round(codec.image_bpp(streams[m]), 4), "max_abs_error": worst}
        if m is not None:
            assert u["blobs"] == lossy and worst <= m, "the bounded-error stream broke its contract"
            r = x - pred
            q = torch.sign(r) * ((r.abs() + m) // (2 * m + 1))         # the arithmetic of residual16.py, on every sample
            counts = torch.unique(q, return_counts=True)[1].to(torch.float64)
            pr = counts / counts.sum()
            ks = [tile["r_k"] for tile in codec.stream_index(streams[m])["tiles"]]
            rec.update(residual_bits_per_sample=round(8.0 * rbytes / (size * size * C), 4),
                       entropy_of_q_bits_per_sample=round(float(-(pr * torch.log2(pr)).sum()), 4),
                       max_abs_q=int(q.abs().max()), tiles_per_k={str(k): ks.count(k) for k in sorted(set(ks))})
        for name in jobs:
            med = statistics.median(reads[name][m])
            rec[name] = {"ms_median": round(med, 3), "ms_all": [round(v, 3) for v in reads[name][m]]}
        res["modes"]["version 6" if m is None else str(m)] = rec
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--tile", type=int, default=256)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--region", action="store_true", help="measure decompress_region windows instead")
    ap.add_argument("--segments", type=int, default=1, help="also measure streams of K y segments, alternately")
    ap.add_argument("--overlap", default=None, metavar="O[,O2...]",
                    help="measure overlapped tiles with blended seams against overlap 0, alternately")
    ap.add_argument("--max-error", default=None, metavar="T[,T2...]",
                    help="measure near-lossless streams (max_error = T) against the lossy stream, alternately")
    ap.add_argument("--nodata", action="store_true",
                    help="measure a scene with a wedge of nodata, coded without and with nodata=0, alternately")
    ap.add_argument("--u16", action="store_true",
                    help="measure the scene as uint16 (stream version 6) against the uint8 scene, alternately")
    ap.add_argument("--tolerance", default=None, metavar="T[,T2...]",
                    help="measure bounded-error uint16 streams (tolerance = T) against the version-6 stream, alternately")
    a = ap.parse_args()
    if a.tolerance is not None:
        res = tolerance_records(a, [int(v) for v in a.tolerance.split(",")])
        print(json.dumps(res))
        with open(a.json or os.path.join(ROOT, "profiles", "tolerance_u16_bench.json"), "w") as f:
            json.dump(res, f, indent=1)
        return

    import numpy as np
    import torch
    from dsic_amd import codec, entropy
    from dsic_amd import synthetic as S
    from dsic_amd.model import CompressionModel

    sd = S.make_state_dict(seed=1)
    model = CompressionModel(N=128, M=192, spatial_params=False, min_nu=2, max_nu=100.0)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    model = model.cuda().eval()
    # the scene: synthetic patches laid side by side (a scene generated at full size costs minutes of numpy)
    g = codec.tile_grid(a.size, a.size, a.tile)
    per = a.size // a.tile
    p = S.make_patches(0, per * per, a.tile, a.tile)
    scene = (p.reshape(per, per, 3, a.tile, a.tile).transpose(0, 3, 1, 4, 2).reshape(a.size, a.size, 3) * 255 + 0.5)
    img = torch.from_numpy(scene.astype(np.uint8)).cuda()
    n = g["n"]

    if a.u16:
        res = u16_records(model, scene / 255, img, a)
        print(json.dumps(res))
        with open(a.json or os.path.join(ROOT, "profiles", "u16_bench.json"), "w") as f:
            json.dump(res, f, indent=1)
        return
    if a.nodata:
        res = nodata_records(model, img, a)
        print(json.dumps(res))
        with open(a.json or os.path.join(ROOT, "profiles", "nodata_bench.json"), "w") as f:
            json.dump(res, f, indent=1)
        return
    if a.max_error is not None:
        res = near_lossless_records(model, img, a, [int(v) for v in a.max_error.split(",")])
        print(json.dumps(res))
        with open(a.json or os.path.join(ROOT, "profiles", "near_lossless_bench.json"), "w") as f:
            json.dump(res, f, indent=1)
        return
    if a.overlap is not None:
        res = overlap_records(model, img, a, [int(v) for v in a.overlap.split(",")])
        print(json.dumps(res))
        with open(a.json or os.path.join(ROOT, "profiles", "overlap_bench.json"), "w") as f:
            json.dump(res, f, indent=1)
        return
    stream = codec.compress_image(model, img, tile=a.tile, batch=a.batch)
    seg = segment_records(model, img, a, n) if a.segments > 1 else None
    if a.region:
        res = region_records(model, stream, a)
        if seg:
            res["segments"] = seg
        print(json.dumps(res))
        with open(a.json or os.path.join(ROOT, "profiles", "region_decode_bench.json"), "w") as f:
            json.dump(res, f, indent=1)
        return
    t_enc = _best(lambda: codec.compress_image(model, img, tile=a.tile, batch=a.batch), a.reps)
    t_dec = _best(lambda: codec.decompress_image(model, stream), a.reps)

    tiles = img.view(per, a.tile, per, a.tile, 3).permute(0, 2, 1, 3, 4).reshape(n, a.tile, a.tile, 3).contiguous()
    batches = [tiles[i:i + a.batch] for i in range(0, n, a.batch)]
    blobs = []

    def host_enc():
        blobs[:] = [entropy.pack_container(entropy.custom_compress(model, b)) for b in batches]

    def host_dec():
        for b in blobs:
            entropy.custom_decompress(model, entropy.unpack_container(b))

    t_henc = _best(host_enc, a.reps)
    t_hdec = _best(host_dec, a.reps)
    assert blobs == codec.unpack_image_stream(stream)["blobs"], "host and device containers differ"
    res = {"scene": f"{a.size}x{a.size}x3 uint8", "tiles": n, "tile": a.tile, "batch": a.batch,
           "stream_bytes": len(stream), "bpp": round(codec.image_bpp(stream), 4),
           "compress_image_tiles_per_s": round(n / t_enc, 1), "decompress_image_tiles_per_s": round(n / t_dec, 1),
           "host_compress_tiles_per_s": round(n / t_henc, 1), "host_decompress_tiles_per_s": round(n / t_hdec, 1),
           "ms": {"compress_image": round(1e3 * t_enc, 2), "decompress_image": round(1e3 * t_dec, 2),
                  "host_compress": round(1e3 * t_henc, 2), "host_decompress": round(1e3 * t_hdec, 2)}}
    if seg:
        res["segments"] = seg
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
