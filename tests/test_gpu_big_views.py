"""The viewing path at the sizes of a real scene: the warp, index and composite kernels past 2^31 and 2^32 elements and
bytes, past 2^20 workgroups and past 2^31 in one histogram bin, bit for bit against the banded restatements of big_ref.py
between guards.  A sibling of test_gpu_big_images.py, whose scenes, pads, guards, sentinel and one-live-image discipline
it imports; the geometry (centres, layouts, writer views) is big_views.py's, which test_big_scene_cpu.py holds to its
conditions without a GPU.  No test holds more than 12 GiB of device memory; the last one asserts the peak.

Which export meets which (S: a source past 2^32 bytes or, for u8c3v / u8c1v, past 2^31 pixels; O: an output past 2^32
bytes; G: more than 2^20 workgroups, so a second trip of the grid-stride loop or a grid of that size; B: a histogram bin
past 2^31):

  dsic_window_warp_u8                 S (u8c3, u8c3v)        O, G (37900 x 37900 x 3)
  dsic_window_warp_u16                S (u16c4)              O, G (23200 x 23200 x 4)
  dsic_window_warp_render_u8          S (u8c3, u8c3v, u8c1v) O, G (32800 x 32800, dword store)
  dsic_window_warp_render_u16         S (u16c4)              O, G (37900 x 37900, byte store)
  dsic_window_warp_index_render_u8    S (u8c3, u8c3v)        O, G (37900 x 37900, byte store)
  dsic_window_warp_index_render_u16   S (u16c4)              O, G (32800 x 32800, dword store)
  dsic_window_index_render_u8 / _u16  S (u8c3, u8c3v / u16c4)
  dsic_index_histogram_u8             S (u8c3), B (u8c1v: one bin holds 2,149,679,137, in LDS and in global memory)
  dsic_index_histogram_u16            S (u16c4; the 131071-bin difference in global memory)
  dsic_window_composite_u8 / _u16     S, O (u8c3), G (5.6 and 2.1 million workgroups: median with N = 4, 8, 16)
  dsic_window_composite_pick_u8/_u16  S, O (u8c3), G (the same grids: rank with N = 4, 8, 16, pick's ballot loop)

Readers give a small output, compared whole.  Composites and writers fill an output of their own size between guards:
bands of rows (test_gpu_big_images._bands) and every row or box that a small source or the writers' image reaches are
compared on the host, and everything else is counted on the device against what it must hold - for a composite the
scene tensor that torch filled (outside the small sources the scene is the only candidate), for a writer the fill."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import big_ref as B
import big_scene as S
import big_views as G
import composite_ref
import index_ref
import warp_ref
from dsic_amd import lib
from dsic_amd.ops import _p, _stream
from test_gpu_big_images import (GIB, LIMIT, SCALE4, SENTINEL, TORCH, Big, BigOut, Handle, Images, _bands,  # noqa: F401
                                 _complement, _crossing_rows, _need, _windows)
from test_gpu_u16 import Out, _inside, _lohi, _same

pytestmark = pytest.mark.gpu
INDEX_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "big_scene_index_counts.npz")
FILL = {"u8": 201, "u16": 51234}
CMAP = np.stack([np.arange(256), 255 - np.arange(256), (7 * np.arange(256) + 3) % 256], axis=1).astype(np.uint8)
MARK = 0x0BADBAD


@pytest.fixture(scope="module")
def images():
    torch.cuda.reset_peak_memory_stats()
    holder = Images()
    yield holder
    holder.clear()


@pytest.fixture(scope="module")
def cmap():
    assert len({tuple(c) for c in CMAP.tolist()}) == 256                     # a wrong entry cannot pass
    return torch.from_numpy(CMAP).cuda()


@pytest.fixture(scope="module")
def golden():
    from test_gpu_big_images import GOLDEN
    table, out = S.table(), {}
    for path in GOLDEN + [INDEX_GOLDEN]:
        z = np.load(path)
        meta = json.loads(bytes(z["meta"]).decode())
        assert meta["constants"] == json.loads(json.dumps(S.CONSTANTS)), "the fixture was made from another pattern"
        for name, shape in meta["shapes"].items():
            s = table[name]
            assert shape == [s.H, s.W, s.C] and meta["nodata"][name] == s.nodata
            assert meta["plants"][name] == [list(map(int, q)) for q in s.plants]
        out.update({k: z[k].astype(np.int64) for k in z.files if k != "meta"})
    return out


def _m6(m):
    return (ctypes.c_int64 * 6)(*m)


def _ints(values):
    return (ctypes.c_int * len(values))(*values)


def _pairs(s):
    return [(10, 200)] * s.C if s.kind == "u8" else SCALE4[:s.C]


def _masks(s):
    """(name, with validity, nodata): with validity, with nodata where the scene has one, with neither"""
    return [("valid", True, None)] + ([("nodata", False, s.nodata)] if s.nodata is not None else []) + [("none", False, None)]


# ---- readers: a whole scene as the level-l window of a warped view -------------------------------------------------------
def _source_head(big, l, with_valid, m):
    s = big.scene
    H, W = B.warp_image(big.src, l)
    return [_p(big.img), _p(big.val) if with_valid else None, s.H, s.W, 0, 0, s.C, l, s.H, s.W, H, W, _m6(m)]


def _nd(nodata):
    return -1 if nodata is None else nodata


def _check_warp(big, name):
    s, L = big.scene, lib.load()
    views = G.warp_views(s)
    assert len(views) >= 12 and {v[4] for v in views} == {0, 1, 2}
    overhang = 0
    for what, l, m, size, mode in views:
        for mask, with_valid, nodata in _masks(s):
            label = f"window_warp_{s.kind} {name} {what} mode {mode} {mask}"
            want, ok = B.warp(big.src, l, m, size, mode, with_valid, nodata, FILL[s.kind])
            out, oval = Out(want.nbytes), Out(ok.size)
            lib.check(getattr(L, "dsic_window_warp_" + s.kind)(*_source_head(big, l, with_valid, m), _p(out.view),
                                                               _p(oval.view), *size, mode, _nd(nodata), FILL[s.kind],
                                                               _stream()), label)
            _same(out.host(label), want, label, s.item)
            _same(oval.host(label), ok.astype(np.uint8), label + " validity")
            if what.startswith("overhang"):
                inside = B.warp(big.src, l, m, size, 1)[1]
                overhang += int(inside.any() and not inside.all())
    assert overhang == 3 * len(_masks(s))                                     # fill and clamped taps at the far end
    big.pads_ok()


def _check_warp_render(big, name):
    s, L = big.scene, lib.load()
    bands = [2, 0, 1] if s.C >= 3 else [0, 0, 0]
    masks = _masks(s)
    for k, (what, l, m, size, mode) in enumerate(G.warp_views(s)):
        mask, with_valid, nodata = masks[k % len(masks)]
        for alpha, background in ((1, 33), (0, 200)):                         # the dword store and the byte store
            label = f"window_warp_render_{s.kind} {name} {what} mode {mode} {mask} alpha {alpha}"
            want = B.warp_render(big.src, l, m, size, mode, with_valid, nodata, bands, _pairs(s), alpha, background)
            out = Out(want.nbytes)
            lib.check(getattr(L, "dsic_window_warp_render_" + s.kind)(*_source_head(big, l, with_valid, m), _ints(bands), 3,
                                                                      _lohi(_pairs(s)), _p(out.view), *size, mode, _nd(nodata),
                                                                      alpha, background, _stream()), label)
            _same(out.host(label), want, label)
    big.pads_ok()


INDEX_CASES = {"u8c3": [("nd", 0, 2), ("difference", 0, 2)], "u16c4": [("nd", 3, 0), ("band", 3)],
               "u8c3v": [("nd", 0, 2)]}


def _index_args(index, s):
    kind, a, b = index_ref.parse(index)
    lo, hi = index_ref.value_range(kind, 255 if s.kind == "u8" else 65535)
    if kind != "nd":
        lo, hi = lo // 2, hi // 2 + 1                                         # values on both sides of the pair
    return [index_ref.KINDS[kind], a, b, lo, hi], (lo, hi)


def _check_warp_index_render(big, name, cmap):
    s, L = big.scene, lib.load()
    masks = _masks(s) if name != "u8c3v" else _masks(s)[:1]                   # u8c3v: pixel 2^31 under validity
    for k, (what, l, m, size, mode) in enumerate(G.warp_views(s)):
        mask, with_valid, nodata = masks[k % len(masks)]
        for n, index in enumerate(INDEX_CASES[name]):
            args, pair = _index_args(index, s)
            alpha, background = (k + n) % 2, (200, 9)[n % 2]
            label = f"window_warp_index_render_{s.kind} {name} {what} mode {mode} {mask} {index} alpha {alpha}"
            want = B.warp_index(big.src, l, m, size, mode, with_valid, nodata, index, pair, CMAP, alpha, background)
            out = Out(want.nbytes)
            lib.check(getattr(L, "dsic_window_warp_index_render_" + s.kind)(
                *_source_head(big, l, with_valid, m), *args, _p(cmap), _p(out.view), *size, mode, _nd(nodata), alpha, background,
                _stream()), label)
            _same(out.host(label), want, label)
    big.pads_ok()


def _check_index_render(big, name, cmap):
    """the windows of test_gpu_big_images._check_render"""
    s, L = big.scene, lib.load()
    for shift in (0, 1, 2):
        for k, (region, size) in enumerate(_windows(big, shift)):
            for mode in (0, 1):
                for with_valid in ((True,) if name == "u8c3v" else (False, True)):
                    index = INDEX_CASES[name][(k + mode + shift) % len(INDEX_CASES[name])]
                    args, pair = _index_args(index, s)
                    alpha, background = (k + mode) % 2, 33
                    label = f"window_index_render_{s.kind} {name} shift {shift} region {region} mode {mode} valid {with_valid} {index}"
                    want = B.index_render(big.src, with_valid, shift, region, size, index, pair, CMAP, ("average", "nearest")[mode],
                                          s.nodata, alpha, background)
                    out = Out(want.nbytes)
                    lib.check(getattr(L, "dsic_window_index_render_" + s.kind)(
                        _p(big.img), _p(big.val) if with_valid else None, s.H, s.W, 0, 0, s.C, shift, *region, *args, _p(cmap),
                        _p(out.view), *size, mode, _nd(s.nodata), alpha, background, _stream()), label)
                    _same(out.host(label), want, label)
    big.pads_ok()


# ---- composites with a scene-sized source ----------------------------------------------------------------------------
NODATA = composite_ref.NODATA
# (mode, index, n and the scene's place (big_views.LISTS), the scene's id or None for no ids)
PLAIN = [("first", 0), ("last", 1), ("mean", 2), ("median", 0), ("median", 1), ("median", 2)]
PICKS = [("first", None, 1, 17), ("last", None, 2, 254), ("max", "nd", 0, 3), ("min", "nd", 1, 254), ("max", "band", 2, 40),
         ("min", "band", 0, None), ("min", "nd", 2, None), ("max", "band", 1, 7)]
SCENE_INDEX = {"u8c3": {"nd": ("nd", 0, 2), "band": ("band", 1)}, "u16c4": {"nd": ("nd", 3, 0), "band": ("band", 2)}}


def _small_sources(kind, C, rects, scene_k):
    """host-made sources for the small rects: every third with a validity window, every third with a nodata value"""
    out = []
    rng = np.random.default_rng(len(rects) * 31 + scene_k)
    for i, (_, _, h, w) in enumerate(rects):
        if i == scene_k:
            out.append(None)
            continue
        img = composite_ref.scene(kind, C, h, w, rng, i)
        val, nodata = None, -1
        if i % 3 == 0:
            val = (rng.random((h, w)) < 0.7).astype(np.uint8) * rng.integers(1, 256, size=(h, w)).astype(np.uint8)
        if i % 3 == 1:
            nodata = NODATA[kind]
            img[rng.random((h, w)) < 0.4] = nodata
        out.append((img, val, nodata))
    return out


def _merged(spans):
    out = []
    for a, b in sorted(spans):
        if out and a <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], b))
        else:
            out.append((a, b))
    return out


def _as_torch(v, kind):
    """a sample value as a scalar torch compares with the tensors of the kind (uint16 bits are held as int16)"""
    return (v + 32768) % 65536 - 32768 if kind == "u16" else v


def _scene_alone(big, dst, planes, oh, ow, small_spans, index, fill, scene_id, nodata):
    """Outside the rows of the small sources the scene is the only candidate: every mode gives the scene's pixel where
    the scene counts (inside its rect, validity not 0, not nodata in all channels, for a normalised difference
    A + B != 0) and fill elsewhere; count is 0 or 1, valid equals count, source is the scene's id or 255.  Returns the
    elements that disagree, counted on the device in pieces of big_scene.BLOCK_BYTES against the scene tensor."""
    s = big.scene
    C, (oy, ox) = s.C, G.ORIGIN
    out = dst.view.view(TORCH[s.kind]).view(oh, ow, C)
    step = max(1, S.BLOCK_BYTES // (ow * C * s.item))
    bad = 0
    for a0, b0 in _complement(small_spans, oh):
        for a in range(a0, b0, step):
            b = min(a + step, b0)
            want = torch.full((b - a, ow, C), _as_torch(fill, s.kind), dtype=TORCH[s.kind], device="cuda")
            cnt = torch.zeros((b - a, ow), dtype=torch.uint8, device="cuda")
            ya, yb = max(a - oy, 0), min(b - oy, s.H)
            if ya < yb:
                img = big.img[ya:yb]
                ok = big.val[ya:yb] != 0
                if nodata >= 0:
                    ok &= ~(img == _as_torch(nodata, s.kind)).all(dim=2)
                if index is not None and index[0] == "nd":
                    ok &= (img[:, :, index[1]] != 0) | (img[:, :, index[2]] != 0)         # A + B != 0
                want[ya + oy - a:yb + oy - a, ox:ox + s.W] = torch.where(ok[:, :, None], img, want[:1, :1])
                cnt[ya + oy - a:yb + oy - a, ox:ox + s.W] = ok
            bad += int((out[a:b] != want).sum())
            for name, plane in planes.items():
                got = plane.view.view(oh, ow)[a:b]
                if name == "source":
                    bad += int((got != torch.where(cnt != 0, scene_id, 255).to(torch.uint8)).sum())
                else:
                    bad += int((got != cnt).sum())
            del want, cnt
    return bad


def _check_composite(big, pick, mode_name, index, which, scene_id, turn):
    s, L = big.scene, lib.load()
    n, place = G.LISTS[which]
    oh, ow = G.composite_size(s)
    assert oh * ow < 1 << 31
    rects, scene_k = G.composite_rects(s, n, place)
    small = _small_sources(s.kind, s.C, rects, scene_k)
    nodata = [(-1 if s.nodata is None else s.nodata) if t is None else t[2] for t in small]
    ids = None if scene_id is None else G.composite_ids(n, scene_k, scene_id)
    fill = FILL[s.kind]
    what = f"window_composite_{'pick_' if pick else ''}{s.kind} {s.name} {mode_name} {index} n={n} scene {place} ids {ids}"
    # the outputs: dst, and as many planes as 12 GiB allow (u8c3: one, taking turns over the cases)
    names = ["valid", "count"] + (["source"] if pick else [])
    if s.name == "u8c3":
        names = [names[turn % len(names)]]
    dst = BigOut(oh * ow * s.C * s.item, what)
    planes = {name: BigOut(oh * ow, what) for name in names}
    held = [None if t is None else (_inside(t[0], s.item * (1 + 2 * (i % 2))), None if t[1] is None else _inside(t[1], 1 + 2 * (i % 3)))
            for i, t in enumerate(small)]
    srcs = [_p(big.img) if h is None else _p(h[0]) for h in held]
    vals = [_p(big.val) if h is None else None if h[1] is None else _p(h[1]) for h in held]
    opt = lambda key: _p(planes[key].view) if key in planes else None
    head = [(ctypes.c_void_p * n)(*srcs), (ctypes.c_void_p * n)(*vals), _ints([v for r in rects for v in r]), _ints(nodata)]
    if pick:
        mode = {"first": 0, "last": 1, "max": 4, "min": 5}[mode_name]
        ix = ("band", 0) if index is None else index
        lib.check(getattr(L, "dsic_window_composite_pick_" + s.kind)(
            *head, None if ids is None else _ints(ids), n, s.C, _p(dst.view), opt("valid"), opt("count"), opt("source"), oh, ow,
            mode, index_ref.KINDS[ix[0]], ix[1], ix[-1], fill, _stream()), what)
    else:
        mode, ix = composite_ref.MODES[mode_name], None
        lib.check(getattr(L, "dsic_window_composite_" + s.kind)(*head, n, s.C, _p(dst.view), opt("valid"), opt("count"), oh, ow,
                                                                mode, fill, _stream()), what)
    torch.cuda.synchronize()
    # bands on the host: the rows under every small source, and the bands around every crossing
    sources = [big.wide if t is None else B.ArraySource(t[0], t[1]) for t in small]
    under = _merged([(r[0], r[0] + r[2]) for k, r in enumerate(rects) if k != scene_k])
    crossings = G.dst_crossing_rows(s) + [int(y) + G.ORIGIN[0] for y in s.crossing_rows()]
    rb = ow * s.C * s.item
    order = ["valid", "count", "source"]
    for y0, y1 in _merged(under + _bands(oh, crossings, 20 + which)):
        want = B.composite_rows(sources, rects, nodata, ids, s.C, oh, ow, mode, ix, fill, y0, y1)
        _same(dst.bytes(y0 * rb, y1 * rb), want[0], f"{what} rows [{y0}, {y1})", s.item)
        for name, plane in planes.items():
            _same(plane.bytes(y0 * ow, y1 * ow), want[1 + order.index(name)], f"{what} {name} rows [{y0}, {y1})")
    # everything else on the device
    sid = scene_k if ids is None else scene_id
    assert _scene_alone(big, dst, planes, oh, ow, under, index if pick and mode >= 4 else None, fill, sid, nodata[scene_k]) == 0, what
    dst.guards_ok(what)
    for plane in planes.values():
        plane.guards_ok(what)
    big.pads_ok()


def _composite_big(images, name):
    big = images.get(name)
    if not hasattr(big, "wide"):                                              # every band of a case stays cached for the next
        big.wide = B.SceneSource(big.scene, keep=400)
    return big


@pytest.mark.parametrize("turn", range(len(PLAIN)))
@pytest.mark.parametrize("name", ["u16c4", "u8c3"])
def test_composite_with_a_scene_sized_source(images, name, turn):
    mode_name, which = PLAIN[turn]
    _check_composite(_composite_big(images, name), False, mode_name, None, which, None, turn)


@pytest.mark.parametrize("turn", range(len(PICKS)))
@pytest.mark.parametrize("name", ["u16c4", "u8c3"])
def test_composite_pick_with_a_scene_sized_source(images, name, turn):
    mode_name, index, which, scene_id = PICKS[turn]
    _check_composite(_composite_big(images, name), True, mode_name, None if index is None else SCENE_INDEX[name][index], which,
                     scene_id, turn)


# ---- writers: warp outputs past 2^32 bytes from a small source --------------------------------------------------------
def _not_pattern(buf2d, pattern, boxes):
    """the elements of the 2-d device tensor outside the boxes [(y0, y1, x0, x1)] that differ from the pattern, counted
    in pieces of 256 MiB"""
    rows, width = buf2d.shape
    step = max(1, (256 << 20) // (width * buf2d.element_size()))
    bad = 0
    spans = _merged([(y0, y1) for y0, y1, _, _ in boxes])
    for a0, b0 in _complement(spans, rows):
        for a in range(a0, b0, step):
            bad += int((buf2d[a:min(a + step, b0)] != pattern).sum())
    for y0, y1, x0, x1 in boxes:
        bad += int((buf2d[y0:y1, :x0] != pattern).sum()) + int((buf2d[y0:y1, x1:] != pattern).sum())
    return bad


def _writer_source(kind, C, turn):
    LH, LW = G.SOURCE
    img = warp_ref.level_image(kind, C, LH, LW)
    val = warp_ref.validity(LH, LW, seed=turn) if turn % 2 else None
    return img, val


@pytest.mark.parametrize("turn", range(len(G.WRITERS)))
def test_warp_writes_an_output_past_2_32_bytes(images, cmap, turn):
    export, kind, C, side, pb = G.WRITERS[turn]
    images.clear()
    L = lib.load()
    img, val = _writer_source(kind, C, turn)
    LH, LW = G.SOURCE
    geometry = (0, LH, LW, LH, LW)
    d_img, d_val = _inside(img, img.dtype.itemsize), None if val is None else _inside(val, 3)
    nodata = None if val is not None else warp_ref.NODATA[kind]
    name = f"dsic_window_{export}_{kind}"
    assert side * side * pb > 1 << 32 and (-(-side // G.TILE)) ** 2 > 1 << 20
    out = BigOut(side * side * pb, name)
    oval = BigOut(side * side, name) if export == "warp" else None
    item = img.dtype.itemsize
    fill, background = (0x3B3B if kind == "u16" else 0x3B), 0x3B
    bands, pairs = [C - 1, 0, 1], ([(10, 200)] * C if kind == "u8" else SCALE4[:C])
    index = ("nd", C - 1, 0)
    for k, (what, m, t, box) in enumerate(G.writer_views(side, pb)):
        mode = (turn + k) % 3
        label = f"{name} {side}x{side} {what} mode {mode}"
        head = [_p(d_img), None if d_val is None else _p(d_val), LH, LW, 0, 0, C, 0, LH, LW, LH, LW, _m6(m)]
        if k:
            out.view.fill_(SENTINEL)
            if oval is not None:
                oval.view.fill_(SENTINEL)
        if export == "warp":
            lib.check(getattr(L, name)(*head, _p(out.view), _p(oval.view), side, side, mode, _nd(nodata), fill, _stream()), label)
            tail = lambda res, ok: res
            pattern = torch.tensor(_as_torch(fill, kind), dtype=TORCH[kind], device="cuda")
            flat = out.view.view(TORCH[kind]).view(side, side * C)
            per = C
        elif export == "warp_render":
            alpha = 1 if pb == 4 else 0
            lib.check(getattr(L, name)(*head, _ints(bands), 3, _lohi(pairs), _p(out.view), side, side, mode, _nd(nodata), alpha,
                                       background, _stream()), label)
            tail = lambda res, ok: B.render_ref.display(res, ok, bands, pairs, alpha, background)
        else:
            alpha = 1 if pb == 4 else 0
            lib.check(getattr(L, name)(*head, index_ref.KINDS["nd"], C - 1, 0, -10000, 10000, _p(cmap), _p(out.view), side, side,
                                       mode, _nd(nodata), alpha, background, _stream()), label)
            tail = lambda res, ok: index_ref.display_index(res, ok, index, (-10000, 10000), CMAP, alpha, background)
        if export != "warp":
            if pb == 4:                                                       # background three times and alpha 0, as one word
                pattern = torch.tensor(background * 0x010101, dtype=torch.int32, device="cuda")
                flat, per = out.view.view(torch.int32).view(side, side), 1
            else:
                pattern = torch.tensor(background, dtype=torch.uint8, device="cuda")
                flat, per = out.view.view(side, side * 3), 3
        torch.cuda.synchronize()
        wfill = fill if export == "warp" else 0
        rb = side * pb
        boxes = []
        if box is not None:
            # the box of output pixels the image can reach, on the host, and where its inside pixels are
            y0, y1, x0, x1 = box
            res, ok = B.warp_rows(img, val, geometry, m, (side, side), mode, nodata, wfill, y0, y1, x0, x1)
            inside = B.warp_rows(img, None, geometry, m, (side, side), 1, None, 0, y0, y1, x0, x1)[1]
            ys, xs = np.nonzero(inside)
            at = (ys.astype(np.int64) + y0) * rb + (xs.astype(np.int64) + x0) * pb
            yc = t // rb
            assert at.min() < t <= at.max() and ys.min() + y0 < yc < ys.max() + y0, label    # the byte is straddled
            edge = (y0 > 0 and inside[0].any()) or (y1 < side and inside[-1].any()) or (x0 > 0 and inside[:, 0].any()) or \
                (x1 < side and inside[:, -1].any())
            assert not edge, label                                             # no inside pixel beside the box
            assert not ok.all() and ok.any(), label
            got = out.view.view(side, rb)[y0:y1, x0 * pb:x1 * pb].cpu().numpy()
            _same(got, tail(res, ok), f"{label} box {box}", item if export == "warp" else 1)
            if oval is not None:
                _same(oval.view.view(side, side)[y0:y1, x0:x1].cpu().numpy(), ok.astype(np.uint8), f"{label} validity box {box}")
            boxes = [box]
        else:
            assert not B.warp_rows(img, None, geometry, m, (side, side), 1, None, 0, 0, side, 0, 1)[1].any()
            assert not B.warp_rows(img, None, geometry, m, (side, side), 1, None, 0, 0, side, side - 1, side)[1].any()
        # whole rows: the first, the last, rows drawn with a fixed seed, and in the view beside the image those of the bytes
        for y0, y1 in _bands(side, _crossing_rows(rb, side) if box is None else [], 30 + turn):
            res, ok = B.warp_rows(img, val, geometry, m, (side, side), mode, nodata, wfill, y0, y1)
            _same(out.bytes(y0 * rb, y1 * rb), tail(res, ok), f"{label} rows [{y0}, {y1})", item if export == "warp" else 1)
            if oval is not None:
                _same(oval.bytes(y0 * side, y1 * side), ok.astype(np.uint8), f"{label} validity rows [{y0}, {y1})")
        # everything outside the rows the image reaches: fill and invalid, or background and alpha 0
        assert _not_pattern(flat, pattern, [(a, b, c * per, d * per) for a, b, c, d in boxes]) == 0, label
        if oval is not None:
            zero = torch.tensor(0, dtype=torch.uint8, device="cuda")
            assert _not_pattern(oval.view.view(side, side), zero, boxes) == 0, label
            oval.guards_ok(label)
        out.guards_ok(label)


# ---- index histograms -------------------------------------------------------------------------------------------------
def _index_histogram(big, with_valid, nodata, index):
    s = big.scene
    kind, a, b = index_ref.parse(index)
    lo, hi = index_ref.value_range(kind, 255 if s.kind == "u8" else 65535)
    bins = hi - lo + 1
    hist = torch.zeros(bins + 32, dtype=torch.int32, device="cuda")
    hist[bins:] = MARK
    name = "dsic_index_histogram_" + s.kind
    lib.check(getattr(lib.load(), name)(_p(big.img), _p(big.val) if with_valid else None, s.H, s.W, s.C, nodata,
                                        index_ref.KINDS[kind], a, b, _p(hist), _stream()), name)
    got = hist.cpu().numpy()
    assert (got[bins:] == MARK).all(), f"{name}: written past the histogram"
    return got[:bins].view(np.uint32).astype(np.int64)


def _check_histogram_u8c1v(big, golden):
    """u8c1v has one channel: with bands (0, 0) every counted pixel has the difference 0, and the normalised difference 0
    unless it is 0 itself (A + B = 0: not defined).  The difference is counted in LDS, the nd in global memory."""
    s = big.scene
    pixels = s.H * s.W
    assert (1 << 31) < pixels < (1 << 32)
    valid, zeros = golden["u8c1v_valid"][0], int(golden["u8c1v_plain"][0][0])
    cases = [(("difference", 0, 0), False, pixels), (("difference", 0, 0), True, int(valid.sum())),
             (("nd", 0, 0), False, pixels - zeros), (("nd", 0, 0), True, int(valid.sum() - valid[0]))]
    for index, with_valid, count in cases:
        u, defined = index_ref.index_value(np.full((1, 1, 1), 5, dtype=np.uint8), *index)
        assert defined.all()
        got = _index_histogram(big, with_valid, -1, index)
        want = np.zeros_like(got)
        want[int(u[0, 0])] = count
        assert np.array_equal(got, want), (index, with_valid, int(got.sum()), count)
    # the difference's bin passes 2^31 in its LDS counter and in the global word; the nd's is one hot global word
    assert cases[0][2] > 1 << 31 and cases[2][2] > 1 << 30 and 0 < cases[3][2] < cases[1][2] < cases[2][2] < pixels
    big.pads_ok()


def _check_histogram_u8c3(big, golden):
    pixels = big.scene.H * big.scene.W
    sums = {}
    for kind in ("nd", "difference"):
        for case, with_valid, nodata in (("plain", False, -1), ("nodata", False, 7), ("valid", True, -1), ("valid_nodata", True, 7)):
            got = _index_histogram(big, with_valid, nodata, (kind, 0, 2))
            assert np.array_equal(got, golden[f"u8c3_{kind}_{case}"]), (kind, case)
            sums[kind, case] = int(got.sum())
            # a difference is defined everywhere: it counts the pixels that the band histogram of the case counts
            if kind == "difference":
                assert sums[kind, case] == int(golden[f"u8c3_{case}"][0].sum()), case
    assert sums["difference", "plain"] == pixels
    for kind in ("nd", "difference"):
        a, b, c, d = (sums[kind, case] for case in ("plain", "nodata", "valid", "valid_nodata"))
        assert a > b > d and a > c > d                                        # each condition leaves pixels out
    # A + B = 0 takes both bands to be 0: at most as many pixels as either band has zeros, and some
    z = min(int(golden["u8c3_plain"][0][0]), int(golden["u8c3_plain"][2][0]))
    assert pixels - z <= sums["nd", "plain"] < pixels
    big.pads_ok()


def _check_histogram_u16c4(big, golden):
    """the 131071 bins of the difference and the 20001 of the nd are both counted in global memory"""
    pixels = big.scene.H * big.scene.W
    for kind in ("nd", "difference"):
        for case, with_valid in (("plain", False), ("valid", True)):
            got = _index_histogram(big, with_valid, -1, (kind, 3, 0))
            assert np.array_equal(got, golden[f"u16c4_{kind}_{case}"]), (kind, case)
            assert int(got.sum()) == int(golden[f"u16c4_{case}"][0].sum())     # no sample is 0: both are defined everywhere
    assert int(golden["u16c4_nd_plain"].sum()) == pixels > int(golden["u16c4_nd_valid"].sum()) > 0
    assert len(golden["u16c4_difference_plain"]) == 131071
    big.pads_ok()


# ---- the readers, scene by scene: each scene is built once ---------------------------------------------------------------
READERS = [("u8c3v", "warp"), ("u8c3v", "warp_render"), ("u8c3v", "warp_index_render"), ("u8c3v", "index_render"),
           ("u8c1v", "warp_render"), ("u8c1v", "index_histogram"),
           ("u16c4", "warp"), ("u16c4", "warp_render"), ("u16c4", "warp_index_render"), ("u16c4", "index_render"),
           ("u16c4", "index_histogram"),
           ("u8c3", "warp"), ("u8c3", "warp_render"), ("u8c3", "warp_index_render"), ("u8c3", "index_render"),
           ("u8c3", "index_histogram")]


@pytest.mark.parametrize("name,export", READERS)
def test_a_whole_scene_is_the_source(images, cmap, golden, name, export):
    big = Handle(images, name)
    if export == "warp":
        _check_warp(big, name)
    elif export == "warp_render":
        _check_warp_render(big, name)
    elif export == "warp_index_render":
        _check_warp_index_render(big, name, cmap)
    elif export == "index_render":
        _check_index_render(big, name, cmap)
    else:
        {"u8c1v": _check_histogram_u8c1v, "u16c4": _check_histogram_u16c4, "u8c3": _check_histogram_u8c3}[name](big, golden)


# ---- limits, as refusals ----------------------------------------------------------------------------------------------
def test_the_size_limits_are_refused_and_nothing_is_written():
    """composite and pick: an output of exactly 2^31 pixels; the index histogram: an image of exactly 2^32 pixels"""
    L = lib.load()
    src = torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda")
    out, plane, hist = Out(8 * 8 * 3), Out(64), Out(4 * 20001)
    head = [(ctypes.c_void_p * 1)(_p(src)), (ctypes.c_void_p * 1)(None), _ints([0, 0, 8, 8]), _ints([-1])]
    for oh, ow in ((32768, 65536), (65536, 32768), (1 << 30, 2)):
        assert L.dsic_window_composite_u8(*head, 1, 3, _p(out.view), _p(plane.view), None, oh, ow, 0, 0, _stream()) == lib.DSIC_EINVAL
        assert b"under 2^31 pixels" in L.dsic_last_error()
        assert L.dsic_window_composite_pick_u8(*head, None, 1, 3, _p(out.view), None, None, _p(plane.view), oh, ow, 4, 2, 0, 1, 0,
                                               _stream()) == lib.DSIC_EINVAL
        assert b"under 2^31 pixels" in L.dsic_last_error()
    for H, W in ((65536, 65536), (1 << 30, 4)):
        for kind in (1, 2):
            assert L.dsic_index_histogram_u8(_p(src), None, H, W, 3, -1, kind, 0, 1, _p(hist.view), _stream()) == lib.DSIC_EINVAL
            assert b"under 2^32 pixels" in L.dsic_last_error()
    # one pixel fewer is inside both limits: the refusal is then another one (a null pointer)
    assert L.dsic_window_composite_u8(*head, 1, 3, None, None, None, 32768, 65535, 0, 0, _stream()) == lib.DSIC_EINVAL
    assert b"null pointer" in L.dsic_last_error()
    assert L.dsic_index_histogram_u8(_p(src), None, 65536, 65535, 3, -1, 0, 0, 1, _p(hist.view), _stream()) == lib.DSIC_EINVAL
    assert b"kind=0" in L.dsic_last_error()
    torch.cuda.synchronize()
    for o in (out, plane, hist):
        assert (o.host("refused calls") == 0x5A).all()
    assert not bool(src.any())


def test_the_module_stayed_within_12_gib(images):
    images.clear()
    peak = torch.cuda.max_memory_allocated()
    print(f"peak device memory of the large-view tests: {peak / GIB:.2f} GiB")
    assert peak <= LIMIT
