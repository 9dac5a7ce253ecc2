"""Pan and zoom: codec.ImageReader against one decompress_region call per frame, and the resampling kernel alone.

    python tools/view_bench.py [--size 4096] [--tile 256] [--reps 3] [--json profiles/view_bench.json] [--only warp|grid|index|composite|warp_composite|zonal]

The scene of image_codec_bench.py (synthetic patches side by side, uint8) is coded once with overviews=3.  A viewport
of 768 rows x 1024 columns pans right in 32 steps of 64 pixels (33 frames).  Per frame, alternately in one process:
  reader   ImageReader.read of the window (one reader per pass, so frame 0 starts with an empty cache)
  region   decompress_region of the window, which is unchanged by the reader's arrival and so is the way without it
then the same frames as a 384 x 512 view: the reader's read(..., size=(384, 512)) (level 1, resampled) against
decompress_region of that level's covering window (what a caller could do before: no resampling, a grid of its own).
render(..., size=(384, 512), alpha=True), the display path, is timed twice against that read.  render_view: a reader
of its own over the same frames with the same decompress_region call between every two frames, so under reader_view's
conditions.  view_cached: one reader whose cache an untimed pan has filled, read and render of every frame one after
the other, the order swapping from frame to frame: the cost of a frame that decodes nothing, side by side.
Every frame is wall clock around the call and a device synchronise; one untimed pass warms every shape, then --reps
passes, and a frame's figure is the median over the passes.  Last, dsic_window_resample_u8 alone on three shapes,
device events around 50 launches after 5 warm-up launches, with the bytes it must move (source window + output), and
dsic_window_render_u8 (three bands + alpha) on the same shapes.  The histogram behind a percentile stretch: a fresh
reader's histogram() of the coarsest and of the full level (wall clock, the decode included), and the kernels alone on
the full level as uint8 and as uint16, once on the scene and once on a constant image.
warp: the 384 x 512 view of the middle frame from a reader whose cache holds its tiles, rendered axis-aligned with
render(..., alpha=True) and with render_warped at 0 and at 30 degrees about the frame's centre, the same 2 level-0 pixels
per output pixel, bilinear and cubic: the median wall clock of 30 calls each, the order rotating from round to round,
and each call's kernel alone on the window it planned (device events, as above).  --only warp measures that record
alone and puts it into the --json file beside the records already there.
grid (--only grid alone): the same four warped views as render_warped, and each as render_gridded of its affine mesh
(codec.affine_grid) at the steps 16 and 64 at the same level, so the same pixels bit for bit; and one tilted view
(codec.projective_grid, step 16) with the distance grid_error gives its mesh at every step.  Calls and kernels are timed
as in the warp record, all in one rotation, so a gridded figure stands beside the affine one of the same process.
Those kernels take about 10 us, near the launch itself, and the host reads the mesh before every launch; so `large` times
the render kernels alone on a 4096 x 4096 view turned by 30 degrees, affine against its mesh at the steps 16 and 64.
index: the same frame and the same requests as index views: render_index with ("nd", 0, 1) through "ndvi" beside
render with three bands, render_index_warped beside render_warped at 0 and 30 degrees (bilinear), all with alpha, each
as a call (the median wall clock of 30, the order rotating) and as its kernel alone on the window it planned; and
index_histogram(("nd", 0, 1)) and (("difference", 0, 1)) beside histogram through fresh readers on the coarsest and the
full level, with the kernels alone on the full level, scene and constant image.  --only index measures that record
alone.
composite (--only composite alone; --size 1024 is the measured one): 16 uint16 x 4 synthetic scenes of --size, each with
a validity mask of its own (blocks of 64 x 64 pixels, six in ten valid), coded once, as temporal stacks of the first 4,
8 and 16.  Per n and mode (first, last, mean, median, and max over ("nd", 3, 0) through
dsic_window_composite_pick_u16, on the same inputs and under the median's byte model): SceneStack.read of the whole grid from warm caches (the median wall clock of 7 calls, the
readers' window assembly included), dsic_window_composite_u16 alone on the readers' windows (device events, as above),
the bytes that launch must move (the validity bytes it has to look at, the pixels it needs, the image it writes), and
the same image built with torch.where / torch.sort on the padded int32 stack [n, H, W, C] (built outside the timing;
checked equal once).  Those windows fit the caches, so the kernel and the torch expression are timed again on 16
random 4096 x 4096 x 4 sources with masks of the same kind: 2 GB of pixels, past the 256 MB Infinity Cache.
warp_composite (--only warp_composite alone): those 16 random 4096 x 4096 x 4 sources and masks under a 4096 x 4096 view
turned by 30 degrees at 0.8 level-0 pixels per output pixel, every source a fraction of a pixel off the others.  Per row
(n = 4, 8, 16 x first, mean, median, max at bilinear; n = 16 median at cubic and at nearest): the one launch of
dsic_window_warp_composite_u16 beside the chain it is defined as, n launches of dsic_window_warp_u16 into n full-size
intermediates and one of dsic_window_composite(_pick)_u16 over them, in the same process on the same inputs, checked
equal once; device events, 20 launches after 5, three rounds alternating.  A fused figure is "within" up to the chain's
slowest round, "margin" up to that plus the chain's spread, else "OUTSIDE".  Each row states a byte model: the validity
and pixel lines under the taps of the sources looked at plus the output, and for the chain that plus n oh ow (C elem + 1)
written and read again.
zonal (--only zonal alone): dsic_zonal_stats_u16 on 4096 x 4096 x 4 random uint16 pixels on the device, as a reader's cached
level hands them over, under three zone rasters, one zone (Z = 1, and again as zone 0 of Z = 4096), blocks of 64 x 64 pixels
(4096 zones) and per-pixel noise over 4096 zones, and under 256 blocks of 256 x 256 pixels, whose table fits LDS as the
single zone's does; every band and ("nd", 3, 0).  Beside each: dsic_band_histogram_u16
on the same pixels, the same table composed in torch on the same device tensors (int64 copies, scatter_add_ and
scatter_reduce_; checked equal once), and the bytes read per second against the read probe of tools/hbm_bw.py.
Records, not bars."""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

VIEW_H, VIEW_W, STEP, STEPS, SIZE = 768, 1024, 64, 32, (384, 512)


def _frame_ms(fn):
    import torch
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _summary(per_pass):
    """per_pass[p][k] = ms of frame k in pass p -> the medians over the passes, summarised"""
    frames = [statistics.median(col) for col in zip(*per_pass)]
    return {"first_frame_ms": round(frames[0], 3), "later_frames_median_ms": round(statistics.median(frames[1:]), 3),
            "later_frames_max_ms": round(max(frames[1:]), 3), "sequence_ms": round(sum(frames), 2),
            "frames_ms": [round(f, 3) for f in frames]}


def _per_launch_us(launch, n=50):
    import torch
    for _ in range(5):
        launch()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(n):
        launch()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / n


def _warp_record(model, stream, win, batch, rounds=30):
    """The `warp` record: see the module's docstring."""
    import torch
    from dsic_amd import codec, lib
    from dsic_amd.ops import _p, _stream
    L = lib.load()
    cy, cx, scale = win[0] + win[2] / 2, win[1] + win[3] / 2, win[2] / SIZE[0]
    views = {f"render_warped {deg} deg {res}": (codec.rotation_affine(cy, cx, deg, scale, *SIZE), res)
             for deg in (0, 30) for res in ("bilinear", "cubic")}
    rec = {"view_size": list(SIZE), "level0_pixels_per_output_pixel": scale, "centre": [cy, cx], "rounds": rounds}
    bands, lohi = (ctypes.c_int * 3)(0, 1, 2), codec._lohi([(0, 255)] * 3)
    rgba = torch.empty(SIZE + (4,), dtype=torch.uint8, device="cuda")
    with codec.ImageReader(model, stream, batch=batch) as r:
        calls = {"render axis-aligned average": lambda: r.render(*win, size=SIZE, alpha=True)}
        for name, (matrix, res) in views.items():
            calls[name] = lambda matrix=matrix, res=res: r.render_warped(matrix, SIZE, alpha=True, resampling=res)
        for fn in calls.values():                                          # untimed: the tiles into the cache, every shape
            fn(), fn()
        torch.cuda.synchronize()
        times, names = {name: [] for name in calls}, list(calls)
        for k in range(rounds):
            for name in names[k % len(names):] + names[:k % len(names)]:
                times[name].append(_frame_ms(calls[name]))
        H, W = r.levels[0]
        for name in names:
            st = {}
            if name in views:
                r.render_warped(views[name][0], SIZE, alpha=True, resampling=views[name][1], stats=st)
            else:
                r.render(*win, size=SIZE, alpha=True, stats=st)
            level, lw = st["level"], st["level_window"]
            src = torch.randint(0, 256, (lw[2], lw[3], 3), dtype=torch.uint8, device="cuda")
            if name in views:
                m = (ctypes.c_int64 * 6)(*st["matrix_q16"])
                mode = {"bilinear": 0, "cubic": 2}[views[name][1]]

                def launch():
                    lib.check(L.dsic_window_warp_render_u8(_p(src), None, lw[2], lw[3], lw[0], lw[1], 3, level,
                                                           *r.levels[level], H, W, m, bands, 3, lohi, _p(rgba), *SIZE, mode,
                                                           -1, 1, 0, _stream()), "window_warp_render_u8")
            else:
                def launch():
                    lib.check(L.dsic_window_render_u8(_p(src), None, lw[2], lw[3], lw[0], lw[1], 3, level, *win, bands, 3,
                                                      lohi, _p(rgba), *SIZE, 0, -1, 1, 0, _stream()), "window_render_u8")
            rec[name] = {"call_median_ms": round(statistics.median(times[name]), 4),
                         "call_max_ms": round(max(times[name]), 4), "level": level, "level_window": list(lw),
                         "kernel_us_per_launch": round(_per_launch_us(launch), 2)}
    return rec


def _grid_record(model, stream, win, batch, rounds=30):
    """The `grid` record: see the module's docstring."""
    import torch
    from dsic_amd import codec, lib
    from dsic_amd.ops import _p, _stream
    L = lib.load()
    cy, cx, scale = win[0] + win[2] / 2, win[1] + win[3] / 2, win[2] / SIZE[0]
    rec = {"view_size": list(SIZE), "level0_pixels_per_output_pixel": scale, "centre": [cy, cx], "rounds": rounds}
    bands, lohi = (ctypes.c_int * 3)(0, 1, 2), codec._lohi([(0, 255)] * 3)
    rgba = torch.empty(SIZE + (4,), dtype=torch.uint8, device="cuda")
    # a tilted view of the same frame: the far edge a quarter shorter
    tilt = [[scale, 0, win[0]], [0, scale, win[1]], [0.25 / SIZE[0], 0, 1]]
    with codec.ImageReader(model, stream, batch=batch) as r:
        H, W = r.levels[0]
        calls, plans = {}, {}
        for deg in (0, 30):
            for res in ("bilinear", "cubic"):
                matrix = codec.rotation_affine(cy, cx, deg, scale, *SIZE)
                m = codec.affine_q16(matrix)
                level = codec.warp_level(len(r.levels), m)
                name = f"{deg} deg {res}"
                calls[f"render_warped {name}"] = lambda matrix=matrix, res=res: r.render_warped(
                    matrix, SIZE, alpha=True, resampling=res)
                plans[f"render_warped {name}"] = (None, m, None, res, level)
                for S in (16, 64):
                    mesh = codec.affine_grid(m, SIZE, S)
                    calls[f"render_gridded {name} step {S}"] = lambda mesh=mesh, S=S, res=res, level=level: r.render_gridded(
                        mesh, SIZE, S, level=level, alpha=True, resampling=res)
                    plans[f"render_gridded {name} step {S}"] = (mesh, None, S, res, level)
        tilted = codec.projective_grid(tilt, SIZE, 16)
        name = "render_gridded projective bilinear step 16"
        calls[name] = lambda: r.render_gridded(tilted, SIZE, 16, alpha=True)
        plans[name] = (tilted, None, 16, "bilinear", codec.grid_level(len(r.levels), tilted, 16))

        def exact(i, j):                                                   # the map the tilted meshes interpolate
            w = 0.25 / SIZE[0] * i + 1
            return (scale * i + win[0]) / w, (scale * j + win[1]) / w
        rec["projective_grid_error_pixels"] = {str(S): round(codec.grid_error(exact, codec.projective_grid(tilt, SIZE, S), SIZE, S), 6)
                                               for S in codec.GRID_STEPS}
        for fn in calls.values():                                          # untimed: the tiles into the cache, every shape
            fn(), fn()
        torch.cuda.synchronize()
        times, names = {name: [] for name in calls}, list(calls)
        for k in range(rounds):
            for name in names[k % len(names):] + names[:k % len(names)]:
                times[name].append(_frame_ms(calls[name]))
        for name in names:
            mesh, m, S, res, level = plans[name]
            mode = {"bilinear": 0, "cubic": 2}[res]
            if mesh is None:
                lw = codec.warp_window(level, *r.levels[level], H, W, m, *SIZE, mode)
                where = ((ctypes.c_int64 * 6)(*m),)
                export = L.dsic_window_warp_render_u8
            else:
                lw = codec.grid_window(level, *r.levels[level], H, W, mesh, mode)
                dev = torch.from_numpy(mesh).cuda()
                where = (mesh.ctypes.data, _p(dev), S)
                export = L.dsic_window_grid_render_u8
            src = torch.randint(0, 256, (lw[2], lw[3], 3), dtype=torch.uint8, device="cuda")

            def launch():
                lib.check(export(_p(src), None, lw[2], lw[3], lw[0], lw[1], 3, level, *r.levels[level], H, W, *where, bands, 3,
                                 lohi, _p(rgba), *SIZE, mode, -1, 1, 0, _stream()), name)
            rec[name] = {"call_median_ms": round(statistics.median(times[name]), 4),
                         "call_max_ms": round(max(times[name]), 4), "level": level, "level_window": list(lw),
                         "kernel_us_per_launch": round(_per_launch_us(launch), 2)}
    rec["large"] = _grid_large(L, lib, bands, lohi)
    return rec


def _grid_large(L, lib, bands, lohi, side=4096, rounds=3):
    """The kernels alone where the launch and the host's look at the mesh do not show: a 4096 x 4096 view of a random
    4096 x 4096 x 3 level turned by 30 degrees at 0.8 level pixels per output pixel (warp_ref's rot30), as
    dsic_window_warp_render_u8 and as dsic_window_grid_render_u8 of its affine mesh at the steps 16 and 64; device
    events, 20 launches after 5, three rounds, the three kinds alternating within a round."""
    import torch
    from dsic_amd import codec
    from dsic_amd.ops import _p, _stream
    src = torch.randint(0, 256, (side, side, 3), dtype=torch.uint8, device="cuda")
    rgba = torch.empty((side, side, 4), dtype=torch.uint8, device="cuda")
    m = codec.affine_q16(codec.rotation_affine(side / 2, side / 2, 30, 0.8, side, side))
    out = {"view_size": [side, side], "matrix_q16": list(m), "rounds": rounds}
    for res, mode in (("bilinear", 0), ("cubic", 2)):
        kinds = {"warp": (L.dsic_window_warp_render_u8, ((ctypes.c_int64 * 6)(*m),), None)}
        for S in (16, 64):
            mesh = codec.affine_grid(m, (side, side), S)
            kinds[f"grid step {S}"] = (L.dsic_window_grid_render_u8, (mesh.ctypes.data, None, S), torch.from_numpy(mesh).cuda())
        us = {k: [] for k in kinds}
        for _ in range(rounds):
            for k, (export, where, dev) in kinds.items():
                if dev is not None:
                    where = (where[0], _p(dev), where[2])

                def launch():
                    lib.check(export(_p(src), None, side, side, 0, 0, 3, 0, side, side, side, side, *where, bands, 3, lohi,
                                     _p(rgba), side, side, mode, -1, 1, 0, _stream()), k)
                us[k].append(round(_per_launch_us(launch, 20), 1))
        out[res] = us
    return out


def _index_record(model, stream, img, win, batch, rounds=30):
    """The `index` record: see the module's docstring."""
    import torch
    from dsic_amd import codec, lib
    from dsic_amd.ops import _p, _stream
    L = lib.load()
    cy, cx, scale = win[0] + win[2] / 2, win[1] + win[3] / 2, win[2] / SIZE[0]
    index, nd = ("nd", 0, 1), 2
    views = {deg: codec.rotation_affine(cy, cx, deg, scale, *SIZE) for deg in (0, 30)}
    rec = {"view_size": list(SIZE), "index": list(index), "colormap": "ndvi", "rounds": rounds}
    bands, lohi = (ctypes.c_int * 3)(0, 1, 2), codec._lohi([(0, 255)] * 3)
    cmap = torch.from_numpy(codec.COLORMAPS["ndvi"]).cuda()
    rgba = torch.empty(SIZE + (4,), dtype=torch.uint8, device="cuda")
    with codec.ImageReader(model, stream, batch=batch) as r:
        calls = {"render": lambda st=None: r.render(*win, size=SIZE, alpha=True, stats=st),
                 "render_index": lambda st=None: r.render_index(*win, index, size=SIZE, colormap="ndvi", alpha=True, stats=st)}
        for deg, matrix in views.items():
            calls[f"render_warped {deg} deg"] = lambda st=None, m=matrix: r.render_warped(m, SIZE, alpha=True, stats=st)
            calls[f"render_index_warped {deg} deg"] = lambda st=None, m=matrix: r.render_index_warped(
                m, SIZE, index, colormap="ndvi", alpha=True, stats=st)
        for fn in calls.values():                                          # untimed: the tiles into the cache, every shape
            fn(), fn()
        torch.cuda.synchronize()
        times, names = {name: [] for name in calls}, list(calls)
        for k in range(rounds):
            for name in names[k % len(names):] + names[:k % len(names)]:
                times[name].append(_frame_ms(calls[name]))
        H, W = r.levels[0]
        for name in names:
            st = {}
            calls[name](st)
            level, lw = st["level"], st["level_window"]
            src = torch.randint(0, 256, (lw[2], lw[3], 3), dtype=torch.uint8, device="cuda")
            head = (_p(src), None, lw[2], lw[3], lw[0], lw[1], 3, level)
            if "warped" in name:
                head += (*r.levels[level], H, W, (ctypes.c_int64 * 6)(*st["matrix_q16"]))
                export = "window_warp_index_render_u8" if "index" in name else "window_warp_render_u8"
            else:
                head += tuple(win)
                export = "window_index_render_u8" if "index" in name else "window_render_u8"
            show = (nd, 0, 1, -10000, 10000, _p(cmap)) if "index" in name else (bands, 3, lohi)

            def launch(export=export, head=head, show=show):
                lib.check(getattr(L, "dsic_" + export)(*head, *show, _p(rgba), *SIZE, 0, -1, 1, 0, _stream()), export)
            rec[name] = {"call_median_ms": round(statistics.median(times[name]), 4),
                         "call_max_ms": round(max(times[name]), 4), "level": level, "level_window": list(lw),
                         "kernel_us_per_launch": round(_per_launch_us(launch), 2)}
    hist = {}
    counted = {"histogram": lambda r, lv: r.histogram(lv), "index_histogram nd": lambda r, lv: r.index_histogram(index, lv),
               "index_histogram difference": lambda r, lv: r.index_histogram(("difference", 0, 1), lv)}
    with codec.ImageReader(model, stream, batch=batch) as r:               # untimed: the first call of every shape
        for fn in counted.values():
            fn(r, None), fn(r, 0)
    for name, fn in counted.items():
        for where, lv in (("coarsest_level", None), ("full_level", 0)):
            with codec.ImageReader(model, stream, batch=batch) as r:
                hist[f"{name} {where}_reader_ms"] = round(_frame_ms(lambda: fn(r, lv)), 2)
    side = img.shape[0]
    for what, image in (("scene", img), ("constant", torch.full_like(img, 77))):
        counts = torch.zeros((3, 256), dtype=torch.int32, device="cuda")

        def launch_band():
            lib.check(L.dsic_band_histogram_u8(_p(image), None, side, side, 3, -1, _p(counts), _stream()), "band_histogram_u8")
        hist[f"kernel band_histogram_u8 {what}_us"] = round(_per_launch_us(launch_band, n=10), 1)
        for label, kind, bins in (("nd", nd, 20001), ("difference", 1, 511)):
            part = torch.zeros((bins,), dtype=torch.int32, device="cuda")

            def launch_index(kind=kind, part=part):
                lib.check(L.dsic_index_histogram_u8(_p(image), None, side, side, 3, -1, kind, 0, 1, _p(part), _stream()),
                          "index_histogram_u8")
            hist[f"kernel index_histogram_u8 {label} {what}_us"] = round(_per_launch_us(launch_index, n=10), 1)
    rec["histogram"] = hist
    return rec


MAX_INDEX = ("nd", 3, 0)                         # the index of the composite record's `max` rows


def _composite_kernels(imgs, masks, size, C, reads=None):
    """dsic_window_composite_u16 alone on n = 4, 8, 16 full-cover sources (imgs uint16 [size, size, C], masks uint8
    [size, size]) per mode, the bytes it must move, and the same image from torch on the padded int32 stack.
    reads: n -> mode -> the image a SceneStack returned for the same sources, held equal to both."""
    import torch
    from dsic_amd import lib
    from dsic_amd.ops import _p, _stream
    L, out, big = lib.load(), {}, 1 << 20
    dst = torch.empty((size, size, C), dtype=torch.uint16, device="cuda")
    for n in (4, 8, 16):
        vals = torch.stack([i.view(torch.int16).to(torch.int32) & 0xFFFF for i in imgs[:n]])   # int32 [n, H, W, C]
        ok = torch.stack(masks[:n]).bool()
        k = ok.sum(0)
        src = (ctypes.c_void_p * n)(*[_p(i) for i in imgs[:n]])
        sv = (ctypes.c_void_p * n)(*[_p(m) for m in masks[:n]])
        rect, nodata = (ctypes.c_int * (4 * n))(*([0, 0, size, size] * n)), (ctypes.c_int * n)(*([-1] * n))
        first = torch.where(k > 0, ok.int().argmax(0) + 1, n)                               # sources looked at up to the winner
        last = torch.where(k > 0, ok.flip(0).int().argmax(0) + 1, n)
        px, out_bytes = 2 * C, size * size * 2 * C
        need = {"first": (int(first.sum()), px * int((k > 0).sum())), "last": (int(last.sum()), px * int((k > 0).sum())),
                "mean": (n * size * size, px * int(k.sum())), "median": (n * size * size, px * int(k.sum())),
                # max: all n validity bytes; bands a and b of every candidate fetch the lines of its pixel
                "max": (n * size * size, px * int(k.sum()))}

        def by_torch(mode):
            if mode in ("first", "last"):
                img = torch.zeros_like(vals[0])
                for i in (range(n - 1, -1, -1) if mode == "first" else range(n)):
                    img = torch.where(ok[i][..., None], vals[i], img)
                return img
            kk = k.clamp(min=1)[..., None]
            if mode == "mean":
                return torch.where(k[..., None] > 0, (2 * (vals * ok[..., None]).sum(0) + kk) // (2 * kk), 0)
            if mode == "max":                                              # the largest nd of bands 3 and 0, the first of equals
                A, s = vals[..., MAX_INDEX[1]], vals[..., MAX_INDEX[1]] + vals[..., MAX_INDEX[2]]
                u = torch.where(ok & (s > 0), (40000 * A.long() + s) // (2 * s).clamp(min=1), -1)
                key = u * n + (n - 1 - torch.arange(n, device=u.device)[:, None, None])      # one maximum per pixel
                win = key.argmax(0)
                img = torch.gather(vals, 0, win[None, ..., None].expand(1, size, size, C))[0]
                return torch.where((u >= 0).any(0)[..., None], img, 0)
            v = torch.sort(torch.where(ok[..., None], vals, big), dim=0).values
            at = lambda idx: torch.gather(v, 0, idx.expand(1, size, size, C))[0]
            return torch.where(k[..., None] > 0, (at(((kk - 1) // 2)[None]) + at((kk // 2)[None]) + 1) >> 1, 0)

        for mode, code in (("first", 0), ("last", 1), ("mean", 2), ("median", 3), ("max", 4)):
            def launch(code=code):
                if code == 4:                                              # DSIC_COMPOSITE_MAX: the pick export alone
                    lib.check(L.dsic_window_composite_pick_u16(src, sv, rect, nodata, None, n, C, _p(dst), None, None, None,
                                                               size, size, code, 2, MAX_INDEX[1], MAX_INDEX[2], 0, _stream()),
                              "window_composite_pick_u16")
                    return
                lib.check(L.dsic_window_composite_u16(src, sv, rect, nodata, n, C, _p(dst), None, None, size, size, code, 0,
                                                      _stream()), "window_composite_u16")
            launch()
            want = by_torch(mode)
            assert torch.equal(dst.view(torch.int16).to(torch.int32) & 0xFFFF, want), (n, mode)
            if reads is not None:
                assert torch.equal(reads[n][mode].view(torch.int16).to(torch.int32) & 0xFFFF, want), (n, mode)
            del want
            torch_ms = sorted(_frame_ms(lambda: by_torch(mode)) for _ in range(5))[2]
            us = _per_launch_us(launch, n=20)
            moved = sum(need[mode]) + out_bytes
            out[f"n={n} {mode}"] = {"kernel_ms": round(us / 1e3, 4), "bytes_validity": need[mode][0], "bytes_pixels": need[mode][1],
                                    "bytes_output": out_bytes, "GB_per_s": round(moved / us / 1e3, 1),
                                    "torch_median_ms": round(torch_ms, 3), "torch_over_kernel": round(torch_ms * 1e3 / us, 1)}
        del vals, ok
    return out


def _block_masks(size, rng, n=16):
    import numpy as np
    import torch
    return [torch.from_numpy(np.kron(rng.random((size // 64, size // 64)) < 0.6, np.ones((64, 64), dtype=bool))).cuda()
            for _ in range(n)]


def _composite_record(size, tile, batch, kernel_size=4096):
    """The `composite` record: see the module's docstring."""
    import numpy as np
    import torch
    from dsic_amd import codec
    from dsic_amd import synthetic as S
    from dsic_amd.model import CompressionModel
    sd = S.make_state_dict(seed=1, N=128, M=192, in_ch=4, spatial_params=False)
    model = CompressionModel(N=128, M=192, spatial_params=False, min_nu=2, max_nu=100.0, in_ch=4)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    model = model.cuda().eval()
    per, C, rng = size // tile, 4, np.random.default_rng(11)
    streams = []
    for s, valid in enumerate(_block_masks(size, rng)):
        p = S.make_patches(1000 * s, per * per, tile, tile, C)
        scene = p.reshape(per, per, C, tile, tile).transpose(0, 3, 1, 4, 2).reshape(size, size, C) * 10000 + 0.5
        streams.append(codec.compress_image(model, torch.from_numpy(scene.astype(np.uint16)).cuda(), tile=tile, batch=batch,
                                            scale=[(0, 12000)] * C, valid=valid, fill=0))
    readers = [codec.ImageReader(model, st, batch=batch) for st in streams]
    window = (0, 0, size, size)
    parts = [r.read(*window, with_valid=True) for r in readers]
    rec = {"scenes": f"16 of {size}x{size} uint16 x {C}, tile {tile}, a validity mask each", "read": {}}
    reads = {}
    for n in (4, 8, 16):
        stack = codec.SceneStack(readers[:n])
        reduces = {"first": "first", "last": "last", "mean": "mean", "median": "median", "max": ("max", MAX_INDEX)}
        reads[n] = {mode: stack.read(*window, reduce=reduce) for mode, reduce in reduces.items()}
        for mode in reads[n]:
            calls = sorted(_frame_ms(lambda: stack.read(*window, reduce=reduces[mode])) for _ in range(7))
            rec["read"][f"n={n} {mode}"] = {"read_median_ms": round(calls[3], 3)}
    rec["kernel_on_the_scenes"] = _composite_kernels([p[0] for p in parts], [p[1].to(torch.uint8) for p in parts], size, C, reads)
    for r in readers:
        r.close()
    del parts, reads
    # past the caches: 16 sources of kernel_size^2 are 2 GB of pixels, against 256 MB of Infinity Cache
    imgs = [torch.randint(0, 10001, (kernel_size, kernel_size, C), dtype=torch.int32, device="cuda").to(torch.int16)
            .view(torch.uint16) for _ in range(16)]
    masks = [m.to(torch.uint8) for m in _block_masks(kernel_size, rng)]
    rec["kernel_size"] = kernel_size
    rec["kernel_past_the_caches"] = _composite_kernels(imgs, masks, kernel_size, C)
    return rec


def _warp_composite_record(kernel_size=4096, rounds=3):
    """The `warp_composite` record: see the module's docstring."""
    import numpy as np
    import torch
    from dsic_amd import codec, lib
    from dsic_amd.ops import _p, _stream
    L, C, size, rng = lib.load(), 4, kernel_size, np.random.default_rng(12)
    imgs = [torch.randint(0, 10001, (size, size, C), dtype=torch.int32, device="cuda").to(torch.int16).view(torch.uint16)
            for _ in range(16)]
    masks = [m.to(torch.uint8) for m in _block_masks(size, rng)]
    # the view of warp_ref's rot30 (0.8 level-0 pixels per output pixel about the centre), each source a fraction of a
    # pixel off the others
    base = codec.rotation_affine(size / 2, size / 2, 30, 0.8, size, size)
    mats = [codec.affine_q16([[base[0][0], base[0][1], base[0][2] + 0.13 * i], [base[1][0], base[1][1], base[1][2] - 0.21 * i]])
            for i in range(16)]
    table = (lib.WarpSource * 16)(*[lib.WarpSource(_p(imgs[i]), _p(masks[i]), size, size, 0, 0, 0, size, size, size, size, -1, i, 0,
                                                   (ctypes.c_int64 * 6)(*mats[i])) for i in range(16)])
    mids = [torch.empty((size, size, C), dtype=torch.uint16, device="cuda") for _ in range(16)]
    mvals = [torch.empty((size, size), dtype=torch.uint8, device="cuda") for _ in range(16)]
    dst, want = (torch.empty((size, size, C), dtype=torch.uint16, device="cuda") for _ in range(2))
    rect, nodata = (ctypes.c_int * 64)(*([0, 0, size, size] * 16)), (ctypes.c_int * 16)(*([-1] * 16))
    src = (ctypes.c_void_p * 16)(*[_p(t) for t in mids])
    sv = (ctypes.c_void_p * 16)(*[_p(t) for t in mvals])
    rows = [(n, mode, "bilinear") for n in (4, 8, 16) for mode in ("first", "mean", "median", "max")]
    rows += [(16, "median", "cubic"), (16, "median", "nearest")]
    codes = {"first": 0, "mean": 2, "median": 3, "max": 4}
    taps = {"bilinear": 4, "nearest": 1, "cubic": 16}
    out = {}
    for n, mode, resampling in rows:
        sample, code = {"bilinear": 0, "nearest": 1, "cubic": 2}[resampling], codes[mode]

        def fused(to=dst):
            lib.check(L.dsic_window_warp_composite_u16(table, n, C, _p(to), None, None, None, size, size, sample, code, 2,
                                                       MAX_INDEX[1], MAX_INDEX[2], 0, _stream()), "window_warp_composite_u16")

        def chain(to=want):
            for i in range(n):
                lib.check(L.dsic_window_warp_u16(_p(imgs[i]), _p(masks[i]), size, size, 0, 0, C, 0, size, size, size, size,
                                                 (ctypes.c_int64 * 6)(*mats[i]), _p(mids[i]), _p(mvals[i]), size, size, sample, -1, 0,
                                                 _stream()), "window_warp_u16")
            if code == 4:
                lib.check(L.dsic_window_composite_pick_u16(src, sv, rect, nodata, None, n, C, _p(to), None, None, None, size, size,
                                                           code, 2, MAX_INDEX[1], MAX_INDEX[2], 0, _stream()),
                          "window_composite_pick_u16")
            else:
                lib.check(L.dsic_window_composite_u16(src, sv, rect, nodata, n, C, _p(to), None, None, size, size, code, 0,
                                                      _stream()), "window_composite_u16")
        fused()
        chain()
        torch.cuda.synchronize()
        assert torch.equal(dst.view(torch.int16), want.view(torch.int16)), (n, mode, resampling)
        f_us, c_us = [], []
        for _ in range(rounds):                                            # alternating: the chain's spread is the yardstick's
            c_us.append(_per_launch_us(chain, n=20))
            f_us.append(_per_launch_us(fused, n=20))
        # bytes: an output pixel advances 0.8 level pixels a side, so the taps of all output pixels cover the 0.64 of a
        # source that the view meets, each line once if the caches hold it between neighbours (a lower bound on the
        # traffic under the taps); first stops at the winner, about 1 / 0.6 sources per pixel
        opix, under = size * size, 0.64 * size * size
        looked = min(n, 1 / 0.6) if mode == "first" else n
        fused_bytes = int(looked * under * (2 * C + 1) + opix * 2 * C)
        chain_bytes = int(n * under * (2 * C + 1) + opix * 2 * C + 2 * n * opix * (2 * C + 1))
        slow, spread = max(c_us), max(c_us) - min(c_us)
        marks = ["within" if f <= slow else "margin" if f <= slow + spread else "OUTSIDE" for f in f_us]
        out[f"n={n} {mode} {resampling}"] = {
            "fused_us": [round(v, 1) for v in f_us], "chain_us": [round(v, 1) for v in c_us], "marks": marks,
            "launches_fused": 1, "launches_chain": n + 1, "taps_per_source": taps[resampling],
            "bytes_fused_model": fused_bytes, "bytes_chain_model": chain_bytes,
            "fused_GB_per_s": round(fused_bytes / statistics.median(f_us) / 1e3, 1),
            "chain_over_fused": round(statistics.median(c_us) / statistics.median(f_us), 2)}
    return {"sources": f"16 random {size}x{size}x{C} uint16 with 64x64-block validity, rot30 at 0.8, sub-pixel offsets per source",
            "timing": f"device events, 20 launches after 5, {rounds} alternating rounds, chain first", "rows": out}


def _zonal_torch(img, zones, Z, of):
    """The table of dsic_zonal_stats_u16 composed in torch on the same device tensors: widened int64 copies, scatter_add_
    for count, sum and sum of squares, scatter_reduce_ for the extremes; ids at or above Z go to a row that is cut off."""
    import torch
    px = img.view(torch.int16).to(torch.int64).bitwise_and_(0xFFFF).reshape(-1, img.shape[2])
    idx = zones.view(torch.int16).to(torch.int64).bitwise_and_(0xFFFF).reshape(-1)
    idx = torch.where(idx < Z, idx, Z)
    if of is None:
        v = px
    else:
        A, B = px[:, of[1]], px[:, of[2]]
        s = A + B
        idx = torch.where(s != 0, idx, Z)
        v = ((40000 * A + s) // (2 * s).clamp_(min=1) - 10000)[:, None]
    K = v.shape[1]
    at = idx[:, None].expand(-1, K)
    table = torch.zeros((Z + 1, K, 5), dtype=torch.int64, device=img.device)
    table[:, :, 3], table[:, :, 4] = (1 << 63) - 1, -(1 << 63)
    table[:, :, 0].scatter_add_(0, at, torch.ones_like(v))
    table[:, :, 1].scatter_add_(0, at, v)
    table[:, :, 2].scatter_add_(0, at, v * v)
    table[:, :, 3].scatter_reduce_(0, at, v, "amin")
    table[:, :, 4].scatter_reduce_(0, at, v, "amax")
    return table[:Z]


def _zonal_record(size=4096, C=4, Z=4096):
    """The `zonal` record: see the module's docstring."""
    import torch
    from dsic_amd import lib
    from dsic_amd.ops import _p, _stream
    L = lib.load()
    img = torch.randint(0, 10001, (size, size, C), dtype=torch.int32, device="cuda").to(torch.int16).view(torch.uint16)
    y, x = torch.meshgrid(torch.arange(size, device="cuda"), torch.arange(size, device="cuda"), indexing="ij")
    rasters = {"one zone": (1, torch.zeros((size, size), dtype=torch.int32, device="cuda")),
               "one zone of 4096": (Z, torch.zeros((size, size), dtype=torch.int32, device="cuda")),
               "64 x 64 blocks": (Z, ((y // 64) * (size // 64) + x // 64).to(torch.int32) % Z),
               "per-pixel noise": (Z, torch.randint(0, Z, (size, size), dtype=torch.int32, device="cuda")),
               "256 x 256 blocks, 256 zones": (256, ((y // 256) * (size // 256) + x // 256).to(torch.int32) % 256)}
    rasters = {k: (nz, v.to(torch.int16).view(torch.uint16).contiguous()) for k, (nz, v) in rasters.items()}
    # the read probe of tools/hbm_bw.py: the sum of 2.1 GB of float32
    probe = torch.empty(64 * 256 * 256 * 128, dtype=torch.float32, device="cuda").fill_(1.0)
    probe_us = _per_launch_us(lambda: probe.sum(), n=10)
    read_TB_s = probe.numel() * 4 / probe_us / 1e6
    del probe
    hist = torch.zeros((C, 65536), dtype=torch.int32, device="cuda")
    hist_us = _per_launch_us(lambda: lib.check(L.dsic_band_histogram_u16(_p(img), None, size, size, C, -1, _p(hist), _stream()),
                                               "band_histogram_u16"), n=20)
    rows = {}
    for name, (Z, zones) in rasters.items():
        for label, of in (("bands", None), ("nd", ("nd", 3, 0))):
            K = C if of is None else 1
            code = (lib.ZONAL_BANDS, 0, 0) if of is None else (2, of[1], of[2])
            table = torch.zeros((Z, K, 5), dtype=torch.int64, device="cuda")

            def fresh():
                table.zero_()
                table[:, :, 3], table[:, :, 4] = (1 << 63) - 1, -(1 << 63)

            def kernel():
                lib.check(L.dsic_zonal_stats_u16(_p(img), None, _p(zones), size, size, C, -1, *code, Z, _p(table), None, None,
                                                 _stream()), "zonal_stats_u16")
            fresh()
            kernel()
            want = _zonal_torch(img, zones, Z, of)
            torch.cuda.synchronize()
            assert torch.equal(table, want), (name, label)
            k_us = _per_launch_us(kernel, n=20)
            t_us = _per_launch_us(lambda: _zonal_torch(img, zones, Z, of), n=3)
            moved = size * size * (2 * C + 2)                              # the pixels and the zone ids, read once
            rows[f"{name}, {label}"] = {
                "kernel_us": round(k_us, 1), "torch_us": round(t_us, 1), "torch_over_kernel": round(t_us / k_us, 2),
                "band_histogram_u16_us": round(hist_us, 1), "bytes_read": moved, "GB_per_s": round(moved / k_us / 1e3, 1),
                "fraction_of_read_probe": round(moved / k_us / 1e6 / read_TB_s, 3), "zones": Z,
                "table": "LDS" if Z * K * 40 <= lib.ZONAL_LDS_BYTES else "global atomics"}
    return {"pixels": f"{size}x{size}x{C} uint16, random in 0..10000, no validity plane",
            "timing": "device events, 20 launches after 5 (torch: 3 after 5)", "read_probe_TB_per_s": round(read_TB_s, 2),
            "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--tile", type=int, default=256)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "view_bench.json"))
    ap.add_argument("--only", choices=("warp", "grid", "index", "composite", "warp_composite", "zonal"), default=None,
                    help="measure this record alone and put it into the --json file beside the others")
    a = ap.parse_args()

    import numpy as np
    import torch
    from dsic_amd import codec, lib
    from dsic_amd import synthetic as S
    from dsic_amd.model import CompressionModel
    from dsic_amd.ops import _p, _stream

    if not torch.cuda.is_available():
        raise SystemExit("view_bench: no GPU; nothing is measured without one")
    if a.only in ("composite", "warp_composite", "zonal"):                 # inputs of their own: nothing below is needed
        res = {}
        if os.path.exists(a.json):
            with open(a.json) as f:
                res = json.load(f)
        res[a.only] = _composite_record(a.size, a.tile, a.batch) if a.only == "composite" else \
            _zonal_record() if a.only == "zonal" else _warp_composite_record()
        print(json.dumps(res[a.only]))
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
        return
    sd = S.make_state_dict(seed=1)
    model = CompressionModel(N=128, M=192, spatial_params=False, min_nu=2, max_nu=100.0)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    model = model.cuda().eval()
    per = a.size // a.tile
    p = S.make_patches(0, per * per, a.tile, a.tile)
    scene = (p.reshape(per, per, 3, a.tile, a.tile).transpose(0, 3, 1, 4, 2).reshape(a.size, a.size, 3) * 255 + 0.5)
    img = torch.from_numpy(scene.astype(np.uint8)).cuda()
    stream = codec.compress_image(model, img, tile=a.tile, batch=a.batch, overviews=3)
    y0, x_first = 1000, 500
    frames = [(y0, x_first + STEP * k, VIEW_H, VIEW_W) for k in range(STEPS + 1)]
    assert frames[-1][1] + VIEW_W <= a.size and y0 + VIEW_H <= a.size
    level = codec.view_level(4, VIEW_H, VIEW_W, *SIZE)
    if a.only is not None:
        with open(a.json) as f:
            res = json.load(f)
        if a.only == "warp":
            res["warp"] = _warp_record(model, stream, frames[STEPS // 2], a.batch)
        elif a.only == "grid":
            res["grid"] = _grid_record(model, stream, frames[STEPS // 2], a.batch)
        else:
            res["index"] = _index_record(model, stream, img, frames[STEPS // 2], a.batch)
        print(json.dumps(res[a.only]))
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
        return

    def one_pass(timed):
        rows = {"reader": [], "region": [], "reader_view": [], "region_level": [], "render_view": [],
                "view_cached_read": [], "view_cached_render": []}
        with codec.ImageReader(model, stream, batch=a.batch) as r:
            for win in frames:
                rows["reader"].append(_frame_ms(lambda: r.read(*win)))
                rows["region"].append(_frame_ms(lambda: codec.decompress_region(model, stream, *win, batch=a.batch)))
            stats = r.stats
        with codec.ImageReader(model, stream, batch=a.batch) as r:
            for win in frames:
                lw = codec.level_window(level, *win)
                rows["reader_view"].append(_frame_ms(lambda: r.read(*win, size=SIZE)))
                rows["region_level"].append(_frame_ms(lambda: codec.decompress_region(model, stream, *lw, level=level,
                                                                                      batch=a.batch)))
        with codec.ImageReader(model, stream, batch=a.batch) as r:
            for win in frames:
                lw = codec.level_window(level, *win)
                rows["render_view"].append(_frame_ms(lambda: r.render(*win, size=SIZE, alpha=True)))
                _frame_ms(lambda: codec.decompress_region(model, stream, *lw, level=level, batch=a.batch))
        with codec.ImageReader(model, stream, batch=a.batch) as r:
            for win in frames:                                             # untimed: every tile of the pan into the cache
                r.read(*win, size=SIZE)
            for k, win in enumerate(frames):
                calls = [("view_cached_read", lambda: r.read(*win, size=SIZE)),
                         ("view_cached_render", lambda: r.render(*win, size=SIZE, alpha=True))]
                for key, fn in calls[::-1] if k % 2 else calls:
                    rows[key].append(_frame_ms(fn))
        return rows, stats

    # the results are the same pixels: checked once, outside the timed passes
    with codec.ImageReader(model, stream, batch=a.batch) as r:
        for win in (frames[0], frames[7], frames[-1]):
            assert torch.equal(r.read(*win), codec.decompress_region(model, stream, *win, batch=a.batch))
    one_pass(False)                                                        # warm-up: every shape of the timed passes
    passes = [one_pass(True) for _ in range(a.reps)]
    res = {"scene": f"{a.size}x{a.size} uint8, tile {a.tile}, overviews 3, {len(stream)} bytes",
           "viewport": [VIEW_H, VIEW_W], "step": STEP, "frames": len(frames), "view_size": list(SIZE),
           "view_level": level, "reps": a.reps,
           "reader_counters_of_one_pan": {k: v for k, v in passes[0][1].items()}}
    for key in ("reader", "region", "reader_view", "region_level", "render_view"):
        res[key] = _summary([rows[key] for rows, _ in passes])
    for key in ("view_cached_read", "view_cached_render"):                 # no frame differs from another here
        full = _summary([rows[key] for rows, _ in passes])
        res[key] = {"frames_median_ms": round(statistics.median(full["frames_ms"]), 3),
                    "frames_max_ms": round(max(full["frames_ms"]), 3), "sequence_ms": full["sequence_ms"],
                    "frames_ms": full["frames_ms"]}

    # the kernels alone
    L = lib.load()

    per_launch_us = _per_launch_us

    kernel, render = [], []
    for name, (sh, sw, shift, region, size) in {
            "viewport 768x1024 of level 0 -> 384x512": (768, 1024, 0, (0, 0, 768, 1024), SIZE),
            "its covering window of level 1 -> 384x512": (385, 513, 1, (1000, 501, 768, 1024), SIZE),
            "whole level 0 -> 2048x2048": (a.size, a.size, 0, (0, 0, a.size, a.size), (a.size // 2, a.size // 2))}.items():
        src = torch.randint(0, 256, (sh, sw, 3), dtype=torch.uint8, device="cuda")
        dst = torch.empty((size[0], size[1], 3), dtype=torch.uint8, device="cuda")
        sy0, sx0 = region[0] >> shift, region[1] >> shift

        def launch():
            lib.check(L.dsic_window_resample_u8(_p(src), sh, sw, sy0, sx0, 3, shift, *region, _p(dst), size[0], size[1],
                                                0, -1, _stream()), "window_resample_u8")
        us = per_launch_us(launch)
        moved = sh * sw * 3 + size[0] * size[1] * 3
        kernel.append({"case": name, "us_per_launch": round(us, 2), "bytes_moved": moved,
                       "GB_per_s": round(moved / us / 1e3, 1)})
        rgba = torch.empty((size[0], size[1], 4), dtype=torch.uint8, device="cuda")
        bands, lohi = (ctypes.c_int * 3)(0, 1, 2), codec._lohi([(10, 240)] * 3)

        def launch_render():
            lib.check(L.dsic_window_render_u8(_p(src), None, sh, sw, sy0, sx0, 3, shift, *region, bands, 3, lohi, _p(rgba),
                                              size[0], size[1], 0, -1, 1, 0, _stream()), "window_render_u8")
        us = per_launch_us(launch_render)
        moved = sh * sw * 3 + size[0] * size[1] * 4
        render.append({"case": name, "us_per_launch": round(us, 2), "bytes_moved": moved,
                       "GB_per_s": round(moved / us / 1e3, 1)})
    res["resample_kernel_u8"] = kernel
    res["render_kernel_u8"] = render

    # the histogram: through a fresh reader, and the kernels alone on the full level
    hist = {}
    with codec.ImageReader(model, stream, batch=a.batch) as r:            # untimed: the first call of either shape
        r.histogram(None), r.histogram(0)
    for name, lv in (("coarsest_level", None), ("full_level", 0)):
        with codec.ImageReader(model, stream, batch=a.batch) as r:
            hist[name + "_reader_ms"] = round(_frame_ms(lambda: r.histogram(lv)), 2)
    for name, image in (("scene", img), ("constant", torch.full_like(img, 77))):
        wide = torch.from_numpy(image.cpu().numpy().astype(np.uint16) * 257).cuda()
        for kind, dev in (("u8", image), ("u16", wide)):
            counts = torch.zeros((3, 256 if kind == "u8" else 65536), dtype=torch.int32, device="cuda")
            fn = getattr(L, "dsic_band_histogram_" + kind)

            def launch_hist():
                lib.check(fn(_p(dev), None, a.size, a.size, 3, -1, _p(counts), _stream()), "band_histogram_" + kind)
            hist[f"kernel_{kind}_{name}_us"] = round(per_launch_us(launch_hist, n=10), 1)
    res["histogram"] = hist
    res["warp"] = _warp_record(model, stream, frames[STEPS // 2], a.batch)
    res["index"] = _index_record(model, stream, img, frames[STEPS // 2], a.batch)
    print(json.dumps(res))
    with open(a.json, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
