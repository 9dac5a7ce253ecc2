"""The kernels that touch a whole image, at the smallest images that cross 2^31 and 2^32 elements and bytes, and at tile
numbers past 65535: bit for bit against the banded restatements of big_ref.py, between guards.

The images are the closed-form scenes of big_scene.py (test_big_scene_cpu.py holds them to their conditions): the device
image is filled by torch block by block, the host evaluates only the rows a comparison needs.  Every image lies inside
a larger allocation of the test's own, so a read that wraps lands in the same allocation and shows as a wrong value.
One large image is live at a time (Images.get drops the others), and no test holds more than 12 GiB of device memory;
the last test of the module asserts the peak.  A case that finds less free memory than it needs skips and says so.

Readers give a small output, compared whole: tile calls over the first tile row, the last two and every tile row that
reads an image row holding a crossing; windows at the first rows, at every crossing and at the last rows.  Writers give
an output that crosses a threshold itself: it is pre-filled with a sentinel, bands of rows are compared (the first 32,
32 around every crossing, the last 32 and 64 rows drawn with a fixed seed), everything the call does not own is counted
against the sentinel on the device, and the guards are checked.

The band histograms and ranges of the large scenes take minutes to stream on the host; they are recorded in
tests/golden/big_scene_counts.npz and big_scene_counts_more.npz by tests/golden/make_golden_big_scene.py, with the
constants of the pattern.  A fixture hands out a handle that builds its image again when another one took its place.
"""
import ctypes
import json
import os
import struct

import numpy as np
import pytest
import torch

import big_ref as B
import big_scene as S
import mask_ref
import render_ref
from dsic_amd import lib
from dsic_amd.ops import _p, _stream
from test_gpu_u16 import Out, _i32, _inside, _lohi, _same

pytestmark = pytest.mark.gpu

PAD = 256                                     # bytes of 0xEE around an image, of 0xCD around a large output
SENTINEL = 0x5A
TILE = 32
GIB = 1 << 30
LIMIT = 12 * GIB
TORCH = {"u8": torch.uint8, "u16": torch.int16, "f32": torch.float32}
SCALE4 = [(20000, 40000), (1, 65534), (30000, 30001), (0, 65535)]
GOLDEN = [os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name)
          for name in ("big_scene_counts.npz", "big_scene_counts_more.npz")]


def _need(nbytes, what):
    """skips when the device has less free memory than the case needs"""
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < nbytes + (256 << 20):
        pytest.skip(f"{what} needs {nbytes / GIB:.2f} GiB of device memory, {free / GIB:.2f} GiB are free")


def _padded(nbytes, pad_byte):
    buf = torch.empty(PAD + nbytes + PAD, dtype=torch.uint8, device="cuda")
    buf[:PAD] = pad_byte
    buf[PAD + nbytes:] = pad_byte
    return buf, buf[PAD:PAD + nbytes]


class Big:
    """a scene on the device, inside an allocation with pads before and after it; its validity plane likewise"""

    def __init__(self, scene):
        self.scene = scene
        _need(scene.nbytes + (scene.H * scene.W if scene.valid else 0) + 2 * S.BLOCK_BYTES * 8, scene.name)
        self.buf, flat = _padded(scene.nbytes, 0xEE)
        self.img = flat.view(TORCH[scene.kind]).view(scene.shape())
        self.vbuf = self.val = None
        if scene.valid:
            self.vbuf, vflat = _padded(scene.H * scene.W, 0xEE)
            self.val = vflat.view(scene.H, scene.W)
        scene.fill(S.torch_namespace("cuda"), self.img, self.val)
        self.src = B.SceneSource(scene)

    def drop(self):
        """frees the device memory; the fixture that handed this image out may outlive it"""
        self.buf = self.img = self.vbuf = self.val = None
        self.src.cache.clear()

    def pads_ok(self):
        for b in (self.buf, self.vbuf):
            if b is not None:
                assert bool((b[:PAD] == 0xEE).all()) and bool((b[-PAD:] == 0xEE).all()), "a pad around an input was written"


class Images:
    def __init__(self):
        self.live = {}

    def get(self, name, scene=None):
        if name not in self.live:
            self.clear()
            self.live[name] = Big(scene or S.table()[name])
        return self.live[name]

    def clear(self):
        for big in self.live.values():
            big.drop()
        self.live.clear()
        torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def images():
    torch.cuda.reset_peak_memory_stats()
    holder = Images()
    yield holder
    holder.clear()


class Handle:
    """What a fixture hands out: the scene's image on the device, built (again) whenever it is not the live one, so a
    test that comes back to an earlier image in another order than the file's finds it whole."""

    def __init__(self, images, name, scene=None):
        self._images, self._name, self._scene = images, name, scene

    def __getattr__(self, key):
        return getattr(self._images.get(self._name, self._scene), key)


@pytest.fixture(scope="module")
def u8c3(images):
    return Handle(images, "u8c3")


@pytest.fixture(scope="module")
def u8c1v(images):
    return Handle(images, "u8c1v")


@pytest.fixture(scope="module")
def u8c3v(images):
    return Handle(images, "u8c3v")


@pytest.fixture(scope="module")
def u16c4(images):
    return Handle(images, "u16c4")


@pytest.fixture(scope="module")
def halve_valid_u16(images):
    return Handle(images, "halve_valid_u16")


@pytest.fixture(scope="module")
def f32c3(images):
    return Handle(images, "f32c3")


@pytest.fixture(scope="module")
def tiles16_u8(images):
    return Handle(images, "tiles16_u8")


@pytest.fixture(scope="module")
def tiles16_u16(images):
    return Handle(images, "tiles16_u16")


@pytest.fixture(scope="module")
def golden():
    table, out = S.table(), {}
    for path in GOLDEN:
        z = np.load(path)
        meta = json.loads(bytes(z["meta"]).decode())
        assert meta["constants"] == json.loads(json.dumps(S.CONSTANTS)), "the fixture was made from another pattern"
        for name, shape in meta["shapes"].items():
            s = table[name]
            assert shape == [s.H, s.W, s.C] and meta["nodata"][name] == s.nodata
            assert meta["plants"][name] == [list(map(int, q)) for q in s.plants]
        out.update({k: z[k].astype(np.int64) for k in z.files if k != "meta"})
    return out


class BigOut:
    """n bytes between 0xCD guards, pre-filled with the sentinel on the device"""

    def __init__(self, nbytes, what, sentinel=SENTINEL):
        _need(nbytes, what)
        self.n, self.sentinel = int(nbytes), sentinel
        self.buf, self.view = _padded(self.n, 0xCD)
        self.view.fill_(sentinel)

    def bytes(self, a, b):
        return self.view[a:b].cpu().numpy()

    def guards_ok(self, what):
        assert bool((self.buf[:PAD] == 0xCD).all()) and bool((self.buf[-PAD:] == 0xCD).all()), f"{what}: guard overwritten"

    def not_sentinel(self, ranges, chunk=256 << 20):
        """the bytes of the byte ranges that no longer hold the sentinel, counted on the device"""
        bad = 0
        for a, b in ranges:
            for lo in range(a, b, chunk):
                bad += int((self.view[lo:min(lo + chunk, b)] != self.sentinel).sum())
        return bad


def _complement(ranges, n):
    out, at = [], 0
    for a, b in sorted(ranges):
        if a > at:
            out.append((at, a))
        at = max(at, b)
    if at < n:
        out.append((at, n))
    return out


def _crossing_rows(row_bytes, rows):
    """the rows of an output of `rows` rows of row_bytes bytes that hold byte 2^31 or 2^32"""
    return [int(t // row_bytes) for t in (1 << 31, 1 << 32) if t // row_bytes < rows]


def _bands(rows, crossings, seed):
    """[(y0, y1)]: the first 32 rows, 32 around each crossing, the last 32, and 64 rows drawn with a fixed seed"""
    out = [(0, min(32, rows)), (max(rows - 32, 0), rows)] + [(max(y - 16, 0), min(y + 16, rows)) for y in crossings]
    out += [(int(y), int(y) + 1) for y in np.random.default_rng(seed).integers(0, rows, 64)]
    return out


def _tile_rows(big, overlap=0):
    """the first tile row, the last two, and those that read a row holding a crossing"""
    s = big.scene
    ny = B.tile_rows(s.H, TILE, overlap)
    return sorted({0, ny - 2, ny - 1} | set(B.tile_rows_reading(s.H, TILE, overlap, s.crossing_rows())))


def _ptr(t):
    return _p(t)


# ---- readers: uint8 HWC, 2^31 and 2^32 bytes --------------------------------------------------------------------------
def _check_gather(big, name, overlap, scale=None, rows=None):
    L = lib.load()
    s = big.scene
    nx = B.tiles_per_row(s.W, TILE, overlap)
    item = 1 if s.kind == "u8" else 4
    for i in (_tile_rows(big, overlap) if rows is None else rows):
        want = B.gather_tile_row(big.src, TILE, TILE, overlap, i, scale)
        out = Out(want.nbytes)
        args = [_ptr(big.img), _p(out.view), s.H, s.W, s.C, TILE, TILE]
        args += [overlap] if name.endswith("_ov") else []
        args += [_lohi(scale)] if scale else []
        what = f"{name} {s.name} overlap {overlap}, tile row {i}"
        lib.check(getattr(L, name)(*args, i * nx, nx, _stream()), what)
        _same(out.host(what), want, what, item)
    big.pads_ok()


@pytest.mark.parametrize("name,overlap", [("dsic_tile_gather_u8", 0), ("dsic_tile_gather_u8_ov", 0),
                                          ("dsic_tile_gather_u8_ov", 16)])
def test_gather_u8_past_2_32_bytes(u8c3, name, overlap):
    assert len(_tile_rows(u8c3, overlap)) >= 4
    _check_gather(u8c3, name, overlap)


def _check_masks(big, nodata, rows=None):
    """classify over whole tile rows and the d planes of the same tiles, listed in descending order"""
    L = lib.load()
    s = big.scene
    nx = B.tiles_per_row(s.W, TILE)
    D = TILE * TILE // 32
    for i in (_tile_rows(big) if rows is None else rows):
        what = f"{s.name} tile row {i} nodata {nodata}"
        counts, planes, pop = Out(4 * nx, fill=0), Out(4 * nx * D), Out(4 * nx, fill=0)
        ids = list(range(i * nx, (i + 1) * nx))[::-1]
        d_ids = _i32(ids)
        if nodata is None:
            lib.check(L.dsic_valid_classify(_ptr(big.val), s.H, s.W, TILE, TILE, i * nx, nx, _p(counts.view), _stream()), what)
            lib.check(L.dsic_valid_delta_planes(_ptr(big.val), s.H, s.W, TILE, TILE, _p(d_ids), nx, _p(planes.view),
                                                _p(pop.view), _stream()), what)
        else:
            lib.check(L.dsic_mask_classify_u8(_ptr(big.img), s.H, s.W, s.C, TILE, TILE, nodata, i * nx, nx, _p(counts.view),
                                              _stream()), what)
            lib.check(L.dsic_mask_delta_planes_u8(_ptr(big.img), s.H, s.W, s.C, TILE, TILE, nodata, _p(d_ids), nx,
                                                  _p(planes.view), _p(pop.view), _stream()), what)
        want = B.classify_tile_row(big.src, TILE, TILE, i, nodata)
        assert counts.host(what).view("<i4").tolist() == want, what
        dwords, pops = B.delta_planes_tile_row(big.src, TILE, TILE, i, nodata)
        _same(planes.host(what), dwords[::-1], what + " d planes", 4)
        assert pop.host(what).view("<i4").tolist() == pops[::-1], what
        # the scene gives the row empty, partial and full tiles (the last tile row owns fewer rows than a tile)
        owned = B.owned_rows(s.H, TILE, i)
        if owned[2] - owned[1] == TILE:
            assert 0 in want and TILE * TILE in want and any(0 < c < TILE * TILE for c in want), what
    big.pads_ok()


def test_mask_classify_and_delta_planes_past_2_32_bytes(u8c3):
    _check_masks(u8c3, 7)


def _windows(big, shift):
    """regions of level 0 whose level-`shift` rows are the image's first rows, the rows of every crossing and its last
    rows: [(region, size)]; origins and lengths are no multiples of 2^shift"""
    s = big.scene
    out = []
    at = [(0, 0), (s.H - 9, s.W - 12)] + [(min(max(int(y) - 4, 0), s.H - 9), min(max(int(x) - 6, 0), s.W - 12))
                                          for y, x, _ in (s.coords(e) for e in s.crossings().values())]
    if s.layout == "hwc" and s.H * s.W > 1 << 31:                             # pixel 2^31: the validity's own crossing
        at.append((min((1 << 31) // s.W - 4, s.H - 9), min(max((1 << 31) % s.W - 6, 0), s.W - 12)))
    for y, x in dict.fromkeys(at):
        a = 1 if shift else 0
        out.append((((y << shift) + a, (x << shift) + a, (9 << shift) - 2 * a, (12 << shift) - 2 * a), (4, 5)))
    return out


def _check_resample(big, with_valid):
    L = lib.load()
    s = big.scene
    name = f"dsic_window_resample_{'valid_' if with_valid else ''}{s.kind}"
    item = s.item
    for shift in (0, 1, 2):
        for region, size in _windows(big, shift):
            for mode in (0, 1):
                what = f"{name} {s.name} shift {shift} region {region} mode {mode}"
                out, oval = Out(size[0] * size[1] * s.C * item), Out(size[0] * size[1])
                head = [_ptr(big.img)] + ([_ptr(big.val)] if with_valid else []) + [s.H, s.W, 0, 0, s.C, shift, *region]
                m = ("average", "nearest")[mode]
                if with_valid:
                    lib.check(getattr(L, name)(*head, _p(out.view), _p(oval.view), *size, mode, 9, _stream()), what)
                    want, wval = B.resample_valid(big.src, shift, region, size, m, 9)
                    _same(oval.host(what), wval.astype(np.uint8), what + " validity")
                elif s.kind == "f32":
                    lib.check(getattr(L, name)(*head, _p(out.view), *size, mode, ctypes.c_float(0.0), 0, _stream()), what)
                    want = B.resample(big.src, shift, region, size, m, None)
                else:
                    lib.check(getattr(L, name)(*head, _p(out.view), *size, mode, s.nodata if s.nodata is not None else -1,
                                               _stream()), what)
                    want = B.resample(big.src, shift, region, size, m, s.nodata if mode == 0 else None)
                _same(out.host(what), want, what, item)
    big.pads_ok()


def _check_render(big, with_valid):
    L = lib.load()
    s = big.scene
    name = f"dsic_window_render_{s.kind}"
    pairs = [(10, 200)] * s.C if s.kind == "u8" else SCALE4[:s.C]
    bands = [2, 0, 1] if s.C >= 3 else [0, 0, 0]
    for shift in (0, 1, 2):
        for region, size in _windows(big, shift):
            for mode in (0, 1):
                what = f"{name} {s.name} valid {with_valid} shift {shift} region {region} mode {mode}"
                out = Out(size[0] * size[1] * 4)
                nodata = s.nodata if s.nodata is not None else -1
                lib.check(getattr(L, name)(_ptr(big.img), _ptr(big.val) if with_valid else None, s.H, s.W, 0, 0, s.C, shift,
                                           *region, _p(_i32(bands)), 3, _lohi(pairs), _p(out.view), *size, mode, nodata, 1,
                                           33, _stream()), what)
                want = B.render(big.src, with_valid, shift, region, size, bands, pairs, ("average", "nearest")[mode],
                                s.nodata, True, 33)
                _same(out.host(what), want, what)
    big.pads_ok()


def test_window_resample_and_render_u8_past_2_32_bytes(u8c3):
    assert len(_windows(u8c3, 0)) == 4                                        # first rows, last rows, two crossings
    _check_resample(u8c3, False)
    _check_resample(u8c3, True)
    _check_render(u8c3, False)
    _check_render(u8c3, True)


def _histogram(big, name, with_valid, nodata):
    L = lib.load()
    s = big.scene
    bins = 256 if s.kind == "u8" else 65536
    hist = torch.zeros(s.C * bins + 32, dtype=torch.int32, device="cuda")
    hist[s.C * bins:] = 0x0BADBAD
    lib.check(getattr(L, name)(_ptr(big.img), _ptr(big.val) if with_valid else None, s.H, s.W, s.C, nodata, _p(hist),
                               _stream()), name)
    got = hist.cpu().numpy()
    assert (got[s.C * bins:] == 0x0BADBAD).all(), f"{name}: written past the histogram"
    return got[:s.C * bins].view(np.uint32).astype(np.int64).reshape(s.C, bins)


def test_band_histogram_u8_past_2_32_bytes(u8c3, golden):
    for case, with_valid, nodata in (("plain", False, -1), ("nodata", False, 7), ("valid", True, -1),
                                     ("valid_nodata", True, 7)):
        got = _histogram(u8c3, "dsic_band_histogram_u8", with_valid, nodata)
        assert np.array_equal(got, golden[f"u8c3_{case}"]), case
    assert int(golden["u8c3_plain"].sum()) == u8c3.scene.elements
    sums = [int(golden[f"u8c3_{case}"][0].sum()) for case in ("plain", "nodata", "valid", "valid_nodata")]
    assert sums[0] > sums[1] > sums[3] and sums[0] > sums[2] > sums[3]         # each condition leaves pixels out
    u8c3.pads_ok()


# ---- readers: pixel index 2^31 in the image and in its validity -----------------------------------------------------
def test_valid_classify_and_delta_planes_past_pixel_2_31(u8c1v):
    assert u8c1v.scene.H * u8c1v.scene.W > 1 << 31
    _check_masks(u8c1v, None)


def test_band_histogram_u8_past_pixel_2_31(u8c1v, golden):
    for case, with_valid in (("plain", False), ("valid", True)):
        got = _histogram(u8c1v, "dsic_band_histogram_u8", with_valid, -1)
        assert np.array_equal(got, golden[f"u8c1v_{case}"]), case
    assert int(golden["u8c1v_plain"].sum()) == u8c1v.scene.H * u8c1v.scene.W
    u8c1v.pads_ok()


def test_band_histogram_u8_one_value_held_by_over_2_31_pixels(u8c1v):
    """The image's rows but the last 33 are set to one value on the device (the scene is built again for the tests
    behind this one): its count passes 2^31 in a 32-bit counter."""
    s = u8c1v.scene
    keep = 33
    assert (s.H - keep) * s.W > 1 << 31
    u8c1v.img[:s.H - keep] = 200
    try:
        got = _histogram(u8c1v, "dsic_band_histogram_u8", False, -1)
    finally:
        u8c1v.src.cache.clear()
        s.fill(S.torch_namespace("cuda"), u8c1v.img, None)
    want = render_ref.histogram(s.band(s.H - keep, s.H))
    want[0, 200] += (s.H - keep) * s.W
    assert want[0, 200] > 1 << 31 and np.array_equal(got, want)
    u8c1v.pads_ok()


def _check_halve_valid(big, name, seed):
    """the masked halving of a scene and its validity; both outputs between guards"""
    L = lib.load()
    s = big.scene
    H2, W2 = (s.H + 1) // 2, (s.W + 1) // 2
    rb = W2 * s.C * s.item
    out, oval = BigOut(H2 * rb, name), BigOut(H2 * W2, name)
    lib.check(getattr(L, name)(_ptr(big.img), _ptr(big.val), _p(out.view), _p(oval.view), s.H, s.W, s.C, _stream()), name)
    src_cross = [int(y) // 2 for y in s.crossing_rows()] + [int((1 << 31) // s.W) // 2] + _crossing_rows(rb, H2)
    for y0, y1 in _bands(H2, [y for y in src_cross if y < H2], seed):
        wimg, wval = B.halve_rows(big.src, y0, y1, with_valid=True)
        _same(out.bytes(y0 * rb, y1 * rb), wimg, f"{name} rows [{y0}, {y1})", s.item)
        _same(oval.bytes(y0 * W2, y1 * W2), wval.astype(np.uint8), f"{name} validity rows [{y0}, {y1})")
    out.guards_ok(name)
    oval.guards_ok(name)
    big.pads_ok()


def test_halve_valid_u8_with_source_pixels_past_2_31(u8c1v):
    """The destination stays under 2^31 bytes here.  A uint8 destination of 2^31 bytes takes S = 2^33 source bytes, S / C
    of validity, S / 4 of output and S / (4 C) of output validity: 1.25 S (1 + 1 / C), at C = 4 (the most channels)
    13.4 GB, over the 12 GiB of this module.  The uint16 case below passes 2^31 on the same kernel template."""
    _check_halve_valid(u8c1v, "dsic_image_halve_valid_u8", 1)


def test_window_render_u8_past_pixel_2_31(u8c1v):
    """one channel: render takes it (the uint8 resamplers want three; u8c3v below).  Windows at pixel 2^31 and at the
    last rows, whose pixel and validity indices are past 2^31."""
    assert len(_windows(u8c1v, 0)) == 3
    _check_render(u8c1v, False)
    _check_render(u8c1v, True)


def test_window_resample_and_render_u8_with_validity_past_pixel_2_31(u8c3v):
    s = u8c3v.scene
    assert s.H * s.W > 1 << 31 and s.valid
    _check_resample(u8c3v, False)
    _check_resample(u8c3v, True)
    _check_render(u8c3v, False)
    _check_render(u8c3v, True)


def test_halve_valid_u16_with_a_destination_past_2_31_bytes(halve_valid_u16):
    s = halve_valid_u16.scene
    assert ((s.H + 1) // 2) * ((s.W + 1) // 2) * s.C * 2 > 1 << 31
    _check_halve_valid(halve_valid_u16, "dsic_image_halve_valid_u16", 7)


# ---- readers: uint16, 2^31 elements and 2^32 bytes --------------------------------------------------------------------
@pytest.mark.parametrize("name,overlap", [("dsic_tile_gather_u16", 0), ("dsic_tile_gather_u16_ov", 0),
                                          ("dsic_tile_gather_u16_ov", 16)])
def test_gather_u16_past_2_32_bytes(u16c4, name, overlap):
    assert len(_tile_rows(u16c4, overlap)) >= 4
    _check_gather(u16c4, name, overlap, SCALE4)


def _range_of(hist):
    return [(int(np.flatnonzero(h)[0]), int(np.flatnonzero(h)[-1])) for h in hist]


def test_band_range_and_histogram_u16_past_2_32_bytes(u16c4, golden):
    L = lib.load()
    s = u16c4.scene
    for case, with_valid in (("plain", False), ("valid", True)):
        got = _histogram(u16c4, "dsic_band_histogram_u16", with_valid, -1)
        assert np.array_equal(got, golden[f"u16c4_{case}"]), case
        out = Out(8 * s.C, fill=0x77)
        if with_valid:
            lib.check(L.dsic_band_range_valid_u16(_ptr(u16c4.img), _ptr(u16c4.val), s.H, s.W, s.C, _p(out.view), _stream()),
                      case)
        else:
            lib.check(L.dsic_band_range_u16(_ptr(u16c4.img), s.H, s.W, s.C, _p(out.view), _stream()), case)
        flat = out.host(case).view("<u4").tolist()
        assert list(zip(flat[0::2], flat[1::2])) == _range_of(golden[f"u16c4_{case}"]), case
    # the minimum and the maximum of every band lie in the last 16 rows only: a pass that stops early misses them
    assert _range_of(golden["u16c4_plain"]) == [(3 + c, 65535 - c) for c in range(4)]
    assert all(y >= s.H - 16 for y, _, _, _ in s.plants)
    u16c4.pads_ok()


def _check_quantize(big, rows, scale, tau, first=None, count=None):
    """residual_quantize_u16 over whole tile rows, or over tiles [first, first + count) of the tile rows `rows`"""
    L = lib.load()
    s = big.scene
    nx = B.tiles_per_row(s.W, TILE)
    for group in ([[i] for i in rows] if first is None else [rows]):
        x_hat = _some_tiles(nx * len(group), s.C, group[0])
        parts = [B.quantize_tile_row(big.src, x_hat[k * nx:(k + 1) * nx], TILE, TILE, i, scale, tau)
                 for k, i in enumerate(group)]
        want, top = np.concatenate([p[0] for p in parts]), sum((p[1] for p in parts), [])
        a = 0 if first is None else first - group[0] * nx
        n = len(want) - a if count is None else count
        d_hat = torch.from_numpy(np.ascontiguousarray(x_hat[a:a + n])).cuda()
        q, maxabs = Out(4 * n * s.C * TILE * TILE), Out(4 * n, fill=0)
        what = f"residual_quantize_u16 {s.name} tile rows {group}"
        lib.check(L.dsic_residual_quantize_u16(_ptr(big.img), _p(d_hat), s.H, s.W, s.C, TILE, TILE, _lohi(scale), tau,
                                               group[0] * nx + a, n, _p(q.view), _p(maxabs.view), _stream()), what)
        _same(q.host(what), want[a:a + n].astype("<i4"), what, 4)
        assert maxabs.host(what).view("<i4").tolist() == top[a:a + n], what
        assert max(top) > 0
    big.pads_ok()


def test_residual_quantize_u16_past_2_32_bytes(u16c4):
    _check_quantize(u16c4, _tile_rows(u16c4), SCALE4, 2)


def test_window_resample_and_render_u16_past_2_32_bytes(u16c4):
    _check_resample(u16c4, False)
    _check_resample(u16c4, True)
    _check_render(u16c4, False)
    _check_render(u16c4, True)


def test_halve_u16_and_halve_valid_u16_with_a_source_past_2_32_bytes(u16c4):
    L = lib.load()
    s = u16c4.scene
    _check_halve_valid(u16c4, "dsic_image_halve_valid_u16", 2)
    H2, W2 = (s.H + 1) // 2, (s.W + 1) // 2
    rb = W2 * s.C * 2
    out = BigOut(H2 * rb, "image_halve_u16")
    lib.check(L.dsic_image_halve_u16(_ptr(u16c4.img), _p(out.view), s.H, s.W, s.C, _stream()), "image_halve_u16")
    for y0, y1 in _bands(H2, [int(y) // 2 for y in s.crossing_rows()], 3):
        _same(out.bytes(y0 * rb, y1 * rb), B.halve_rows(u16c4.src, y0, y1), f"image_halve_u16 rows [{y0}, {y1})", 2)
    out.guards_ok("image_halve_u16")
    u16c4.pads_ok()


# ---- float32 CHW: 2^31 elements inside plane 2, 2^32 bytes inside plane 1 ---------------------------------------------
@pytest.mark.parametrize("name,overlap", [("dsic_tile_gather_f32", 0), ("dsic_tile_gather_f32_ov", 0),
                                          ("dsic_tile_gather_f32_ov", 16)])
def test_gather_f32_past_2_32_bytes(f32c3, name, overlap):
    assert len(_tile_rows(f32c3, overlap)) >= 4
    _check_gather(f32c3, name, overlap)


def test_window_resample_f32_past_2_32_bytes(f32c3):
    _check_resample(f32c3, False)


def _plane_rows(out, C, H2, W2, y0, y1):
    """rows [y0, y1) of every plane of a float32 [C][H2][W2] output -> [C][rows][W2]"""
    return np.stack([out.bytes(4 * (c * H2 + y0) * W2, 4 * (c * H2 + y1) * W2).view(np.float32).reshape(y1 - y0, W2)
                     for c in range(C)])


def test_halve_f32_with_a_destination_past_2_31_bytes(f32c3):
    L = lib.load()
    s = f32c3.scene
    H2, W2 = (s.H + 1) // 2, (s.W + 1) // 2
    assert 4 * s.C * H2 * W2 > 1 << 31
    out = BigOut(4 * s.C * H2 * W2, "image_halve_f32")
    lib.check(L.dsic_image_halve_f32(_ptr(f32c3.img), _p(out.view), s.C, s.H, s.W, _stream()), "image_halve_f32")
    cross = [((1 << 31) // 4 // W2) % H2] + [int(y) // 2 for y in s.crossing_rows()]
    for y0, y1 in _bands(H2, cross, 4):
        _same(_plane_rows(out, s.C, H2, W2, y0, y1), B.halve_rows(f32c3.src, y0, y1), f"image_halve_f32 rows [{y0}, {y1})", 4)
    out.guards_ok("image_halve_f32")
    f32c3.pads_ok()


def test_blend_finish_u8_u16_and_f32_on_a_canvas_past_2_32_bytes(f32c3):
    """The canvas is the scene times 1.5 (one float32 rounding in both libraries), so the finish's min(v, 1) acts on a
    third of it.  uint8: 3 planes, the output passes 2^31 bytes; uint16: 2 planes (3 would pass 12 GiB with the
    canvas), the output passes 2^31 bytes; float32 in place, last."""
    L = lib.load()
    s = f32c3.scene
    f32c3.img.mul_(1.5)
    try:
        def canvas(y0, y1, C):
            return (f32c3.src.rows(np.arange(y0, y1)) * np.float32(1.5))[:C]

        for kind, C, item in (("u8", 3, 1), ("u16", 2, 2)):
            rb = s.W * C * item
            out = BigOut(s.H * rb, f"blend_finish_{kind}")
            assert out.n > 1 << 31
            if kind == "u8":
                lib.check(L.dsic_tile_blend_finish_u8(_ptr(f32c3.img), _p(out.view), C, s.H, s.W, _stream()), kind)
            else:
                lib.check(L.dsic_tile_blend_finish_u16(_ptr(f32c3.img), _p(out.view), C, s.H, s.W, _lohi(SCALE4[:C]),
                                                       _stream()), kind)
            for y0, y1 in _bands(s.H, _crossing_rows(rb, s.H), 5):
                _same(out.bytes(y0 * rb, y1 * rb), B.finish_rows(canvas(y0, y1, C), kind, SCALE4[:C]),
                      f"blend_finish_{kind} rows [{y0}, {y1})", item)
            out.guards_ok(kind)
            del out
        lib.check(L.dsic_tile_blend_finish_f32(_ptr(f32c3.img), s.C, s.H, s.W, _stream()), "blend_finish_f32")
        for y0, y1 in _bands(s.H, s.crossing_rows(), 6):
            got = f32c3.img[:, y0:y1].cpu().numpy()
            _same(got, B.finish_rows(canvas(y0, y1, s.C), "f32"), f"blend_finish_f32 rows [{y0}, {y1})", 4)
        f32c3.pads_ok()
    finally:
        s.fill(S.torch_namespace("cuda"), f32c3.img, None)


# ---- the uint8 halvings with a destination past 2^31 bytes -------------------------------------------------------------
HALVE_H, HALVE_ROW = 92801, 92804              # the source: 92801 rows of 92804 bytes, 8.6 GB (C = 4: 23201 pixels)


class FlatRows:
    """the halving source read as H x W x C of uint8 or uint16: row y is bytes [y W C item, (y + 1) W C item) of the
    flat byte scene"""

    def __init__(self, scene, W, C, kind):
        self.flat, self.H, self.W, self.C, self.kind = scene, scene.H, W, C, kind
        self.item = 1 if kind == "u8" else 2

    def rows(self, ys):
        rb = self.W * self.C * self.item
        e = np.asarray(ys, dtype=np.int64)[:, None] * rb + np.arange(rb, dtype=np.int64)[None, :]
        b = self.flat.at(e).astype(np.uint8)
        return b.view(np.uint8 if self.kind == "u8" else "<u2").reshape(len(ys), self.W, self.C)


@pytest.fixture(scope="module")
def halve_source(images):
    return Handle(images, "halve_source", S.Scene("halve_source", "u8", HALVE_H, HALVE_ROW, 1))


@pytest.mark.parametrize("kind,C", [("u8", 1), ("u8", 2), ("u8", 3), ("u8", 4), ("u8", 5), ("u16", 2)])
def test_halve_with_a_destination_past_2_31_bytes(halve_source, kind, C):
    """C = 1, 2 and uint16 run halve.h's halve_kernel, C = 3, 4 halve_u8_kernel's window path, C = 5 its tap-by-tap
    path: the widest W with W C bytes inside the source's rows, so every destination passes 2^31 bytes."""
    L = lib.load()
    item = 1 if kind == "u8" else 2
    W = HALVE_ROW // (C * item)
    src = FlatRows(halve_source.scene, W, C, kind)
    H2, W2 = (HALVE_H + 1) // 2, (W + 1) // 2
    rb = W2 * C * item
    assert H2 * rb > 1 << 31 and HALVE_H * W * C * item <= halve_source.scene.nbytes
    name = f"dsic_image_halve_{kind}"
    out = BigOut(H2 * rb, name)
    lib.check(getattr(L, name)(_ptr(halve_source.img), _p(out.view), HALVE_H, W, C, _stream()), name)
    src_cross = [int(t // (W * C * item)) // 2 for t in (1 << 31, 1 << 32)]
    for y0, y1 in _bands(H2, _crossing_rows(rb, H2) + src_cross, 10 + C):
        _same(out.bytes(y0 * rb, y1 * rb), B.halve_rows(src, y0, y1), f"{name} C={C} rows [{y0}, {y1})", item)
    out.guards_ok(name)
    halve_source.pads_ok()


# ---- writers over a whole image: stitch, mask apply and the validity window -------------------------------------------
ITEM = {"u8": 1, "u16": 2, "f32": 4, "hw": 1}
FILLS = {"u8": SENTINEL, "u16": SENTINEL * 0x0101, "hw": SENTINEL,
         "f32": np.frombuffer(bytes([SENTINEL] * 4), dtype=np.float32)[0]}


def _some_tiles(n, C, seed):
    rng = np.random.default_rng(seed)
    base = rng.uniform(-0.25, 1.25, size=(64, C, TILE, TILE)).astype(np.float32)
    return base[rng.integers(0, 64, n)]


class Canvas:
    """An output of a whole image between guards, pre-filled with the sentinel: uint8 / uint16 [H][W][C], float32
    [C][H][W], or the validity window uint8 [H][W] (kind "hw", C = 1)."""

    def __init__(self, kind, H, W, C, what, sentinel=SENTINEL):
        self.kind, self.H, self.W, self.C, self.item = kind, H, W, C, ITEM[kind]
        self.out = BigOut(H * W * C * self.item, what, sentinel)

    def _ranges(self, y0, y1):
        if self.kind == "f32":
            return [(4 * (c * self.H + y0) * self.W, 4 * (c * self.H + y1) * self.W) for c in range(self.C)]
        rb = self.W * self.C * self.item
        return [(y0 * rb, y1 * rb)]

    def rows(self, y0, y1):
        """rows [y0, y1) as the restatements shape them"""
        parts = [self.out.bytes(a, b) for a, b in self._ranges(y0, y1)]
        if self.kind == "f32":
            return np.stack([p.view(np.float32).reshape(y1 - y0, self.W) for p in parts])
        if self.kind == "hw":
            return parts[0].reshape(y1 - y0, self.W)
        return parts[0].view(np.uint8 if self.kind == "u8" else "<u2").reshape(y1 - y0, self.W, self.C)

    def blank(self, y0, y1):
        """what rows [y0, y1) held before the calls"""
        shape = {"f32": (self.C, y1 - y0, self.W), "hw": (y1 - y0, self.W)}.get(self.kind, (y1 - y0, self.W, self.C))
        return np.full(shape, FILLS[self.kind], dtype={"u8": np.uint8, "u16": np.uint16, "f32": np.float32, "hw": np.uint8}
                       [self.kind])

    def crossing_tile_rows(self):
        rb = self.W * (self.C if self.kind in ("u8", "u16") else 1) * self.item
        return {int((t // rb) % self.H) // TILE for t in (1 << 31, 1 << 32) if t < self.out.n}

    def untouched(self, tile_rows, what):
        """nothing outside the rows that the tile rows own was written, nor a guard"""
        self.untouched_rows([(i * TILE, min((i + 1) * TILE, self.H)) for i in tile_rows], what)

    def untouched_rows(self, row_ranges, what):
        owned = [r for a, b in row_ranges for r in self._ranges(a, b)]
        assert self.out.not_sentinel(_complement(owned, self.out.n)) == 0, f"{what}: bytes outside the tiles of the calls"
        self.out.guards_ok(what)


def _tile_row_lists(canvas):
    """per call the tiles of one tile row, descending, and two numbers outside the grid: the first tile row, those of
    the crossings and the last two"""
    ny, nx = B.tile_rows(canvas.H, TILE), B.tiles_per_row(canvas.W, TILE)
    rows = sorted({0, ny - 2, ny - 1} | canvas.crossing_tile_rows())
    assert len(rows) >= 4
    return [list(range(i * nx, (i + 1) * nx))[::-1] + [-1, nx * ny] for i in rows]


def _touched(canvas, id_lists):
    ny, nx = B.tile_rows(canvas.H, TILE), B.tiles_per_row(canvas.W, TILE)
    return sorted({t // nx for ids in id_lists for t in ids if 0 <= t < nx * ny})


def _check_stitch(canvas, id_lists, scale=None, tau=None):
    """tile_stitch_window_<kind>, or with tau its _res sibling: residual steps in -QMAX .. QMAX ride along"""
    L = lib.load()
    kind, H, W, C = canvas.kind, canvas.H, canvas.W, canvas.C
    name = f"dsic_tile_stitch_window_{kind}" + ("" if tau is None else "_res")
    tiles = [_some_tiles(len(ids), C, k) for k, ids in enumerate(id_lists)]
    steps = [np.round(_some_tiles(len(ids), C, 100 + k) * 2 * B.QMAX - B.QMAX).clip(-B.QMAX, B.QMAX).astype(np.float32)
             for k, ids in enumerate(id_lists)]
    held = []                                                                 # the calls' inputs stay allocated
    for t, q, ids in zip(tiles, steps, id_lists):
        held.append((torch.from_numpy(t).cuda(), torch.from_numpy(q).cuda(), _i32(ids)))
        d_tiles, d_q, d_ids = held[-1]
        args = [_p(d_tiles)] + ([] if tau is None else [_p(d_q), tau])
        args += [_p(d_ids), len(ids), _p(canvas.out.view), H, W, C, TILE, TILE, 0, 0, H, W]
        lib.check(getattr(L, name)(*args, *([_lohi(scale)] if kind == "u16" else []), _stream()), name)
    torch.cuda.synchronize()
    every, all_q, all_ids = np.concatenate(tiles), np.concatenate(steps), [t for ids in id_lists for t in ids]
    rows = _touched(canvas, id_lists)
    for i in rows:
        y0, y1 = i * TILE, min((i + 1) * TILE, H)
        if tau is None:
            want = B.stitch_rows(every, all_ids, H, W, TILE, TILE, y0, y1, kind, FILLS[kind], scale)
        else:
            want = B.stitch_res_rows(every, all_q, tau, all_ids, H, W, TILE, TILE, y0, y1, kind, FILLS[kind], scale)
        _same(canvas.rows(y0, y1), want, f"{name} {H}x{W}x{C} tile row {i}", canvas.item)
    canvas.untouched(rows, name)


def _check_mask_writer(canvas, id_lists, v):
    """mask_apply_u8 / _u16 / _f32 and mask_window_u8 with the whole image as the window; the planes take turns"""
    L = lib.load()
    kind, H, W, C = canvas.kind, canvas.H, canvas.W, canvas.C
    rng = np.random.default_rng(H + C)
    planes = [rng.random((TILE, TILE)) < p for p in (0.5, 0.1, 0.9, 0.5, 0.02, 0.98, 0.5, 0.3)]
    d_planes = torch.from_numpy(np.stack([mask_ref.plane_dwords(m) for m in planes]).astype(np.int32)).cuda()
    descs = [[(t, (t % 9) - 1) for t in ids] for ids in id_lists]
    name = "dsic_mask_window_u8" if kind == "hw" else f"dsic_mask_apply_{kind}"
    held = [_i32(desc) for desc in descs]                                      # the calls' inputs stay allocated
    for desc, d_desc in zip(descs, held):
        head = [_p(d_planes), len(planes), _p(d_desc), len(desc)] + ([] if kind == "hw" else [v])
        tail = [H, W] + ([] if kind == "hw" else [C]) + [TILE, TILE, 0, 0, H, W]
        lib.check(getattr(L, name)(*head, _p(canvas.out.view), *tail, _stream()), name)
    torch.cuda.synchronize()
    every = [d for desc in descs for d in desc]
    rows = _touched(canvas, id_lists)
    for i in rows:
        y0, y1 = i * TILE, min((i + 1) * TILE, H)
        if kind == "hw":
            want = B.mask_window_rows(canvas.blank(y0, y1), H, W, TILE, TILE, y0, every, planes)
        else:
            want = B.mask_apply_rows(canvas.blank(y0, y1), H, W, TILE, TILE, y0, every, planes, v)
        _same(canvas.rows(y0, y1), want, f"{name} {H}x{W}x{C} tile row {i}", canvas.item)
    canvas.untouched(rows, name)


@pytest.mark.parametrize("kind,H,W,C", [("u8", 39801, 36001, 3), ("u16", 32801, 16401, 4), ("f32", 26801, 26801, 3),
                                        ("hw", 32801, 65537, 1)])
def test_stitch_and_mask_writers_over_a_whole_image_past_2_31_and_2_32_bytes(images, kind, H, W, C):
    """the window is the whole image; a call holds one whole tile row"""
    images.clear()
    canvas = Canvas(kind, H, W, C, f"a whole {kind} image")
    assert canvas.out.n > (1 << 31 if kind == "hw" else 1 << 32)
    lists = _tile_row_lists(canvas)
    if kind != "hw":
        _check_stitch(canvas, lists, SCALE4[:C])
        canvas.out.view.fill_(SENTINEL)
    if kind in ("u8", "u16"):
        _check_stitch(canvas, lists, SCALE4[:C], tau=3 if kind == "u8" else 300)
        canvas.out.view.fill_(SENTINEL)
    _check_mask_writer(canvas, lists, 9)


# ---- tile numbers past 65535 ---------------------------------------------------------------------------------------
FIRST, COUNT = 65530, 519


def _tiles16_rows(scene):
    nx = B.tiles_per_row(scene.W, TILE)
    assert nx * B.tile_rows(scene.H, TILE) == 66049 == FIRST + COUNT
    return nx, list(range(FIRST // nx, 66049 // nx))


def _check_gather_16(big, name, scale=None):
    L = lib.load()
    s = big.scene
    nx, rows = _tiles16_rows(s)
    want = np.concatenate([B.gather_tile_row(big.src, TILE, TILE, 0, i, scale) for i in rows])[FIRST - rows[0] * nx:]
    assert want.shape[0] == COUNT
    out = Out(want.nbytes)
    args = [_ptr(big.img), _p(out.view), s.H, s.W, s.C, TILE, TILE] + ([0] if name.endswith("_ov") else [])
    args += [_lohi(scale)] if scale else []
    lib.check(getattr(L, name)(*args, FIRST, COUNT, _stream()), name)
    _same(out.host(name), want, f"{name} tiles [{FIRST}, {FIRST + COUNT})", 1 if s.kind == "u8" else 4)


def _check_masks_16(big, nodata):
    """classify over [65530, 66049), and the d planes of a list that mixes numbers below and above 65535"""
    L = lib.load()
    s = big.scene
    nx, rows = _tiles16_rows(s)
    counts = Out(4 * COUNT, fill=0)
    if nodata is None:
        lib.check(L.dsic_valid_classify(_ptr(big.val), s.H, s.W, TILE, TILE, FIRST, COUNT, _p(counts.view), _stream()), "16")
    else:
        lib.check(L.dsic_mask_classify_u8(_ptr(big.img), s.H, s.W, s.C, TILE, TILE, nodata, FIRST, COUNT, _p(counts.view),
                                          _stream()), "16")
    want = sum((B.classify_tile_row(big.src, TILE, TILE, i, nodata) for i in rows), [])[FIRST - rows[0] * nx:]
    assert counts.host("classify").view("<i4").tolist() == want
    ids = [66048, 3, 65535, 65536, 0, 65534, 66000, nx * rows[0] + 5, 256, 65793]
    D = TILE * TILE // 32
    planes, pop = Out(4 * len(ids) * D), Out(4 * len(ids), fill=0)
    if nodata is None:
        lib.check(L.dsic_valid_delta_planes(_ptr(big.val), s.H, s.W, TILE, TILE, _p(_i32(ids)), len(ids), _p(planes.view),
                                            _p(pop.view), _stream()), "16")
    else:
        lib.check(L.dsic_mask_delta_planes_u8(_ptr(big.img), s.H, s.W, s.C, TILE, TILE, nodata, _p(_i32(ids)), len(ids),
                                              _p(planes.view), _p(pop.view), _stream()), "16")
    by_row = {}
    want_d, want_p = [], []
    for t in ids:
        i, j = divmod(t, nx)
        if i not in by_row:
            by_row[i] = B.delta_planes_tile_row(big.src, TILE, TILE, i, nodata)
        want_d.append(by_row[i][0][j])
        want_p.append(by_row[i][1][j])
    _same(planes.host("planes"), np.stack(want_d), "d planes of tiles below and above 65535", 4)
    assert pop.host("pop").view("<i4").tolist() == want_p
    # mask_pack records the tile numbers with the payloads; mask_unpack gives the m planes back
    ms = []
    for t in ids:
        i, j = divmod(t, nx)
        ms.append(B.m_planes_tile_row(big.src, TILE, TILE, i, nodata)[j])
    pays = [mask_ref.payload(mask_ref.delta(m)) for m in ms]
    want = b"".join(struct.pack("<3I", t, mode, len(body)) for t, (mode, body) in zip(ids, pays))
    want += b"".join(body for _, body in pays)
    d_ids = _i32(ids)
    out, ws = Out(len(ids) * (12 + TILE * TILE // 8)), Out(8 * (len(ids) + 2))
    lib.check(L.dsic_mask_pack(_p(planes.view), _p(pop.view), _p(d_ids), len(ids), TILE, TILE, _p(ws.view), _p(out.view),
                               _stream()), "mask_pack")
    got = out.host("mask_pack")
    assert ws.host("mask_pack ws")[:16].view("<i8").tolist() == [len(want), 0]
    _same(got[:len(want)], np.frombuffer(want, np.uint8), "mask_pack of tiles below and above 65535")
    assert (got[len(want):] == 0x5A).all(), "mask_pack wrote past its bytes"
    blob, desc = b"".join(body for _, body in pays), []
    for mode, body in pays:
        desc.append((mode, sum(d[2] for d in desc), len(body)))
    d_desc, d_blob = _i32(desc), _inside(np.frombuffer(blob + b"\0" * 16, np.uint8), 0)
    mplanes = Out(4 * D * len(ids))
    lib.check(L.dsic_mask_unpack(_p(d_blob), len(blob), _p(d_desc), len(ids), TILE, TILE, _p(mplanes.view), _stream()),
              "mask_unpack")
    _same(mplanes.host("mask_unpack"), np.concatenate([mask_ref.plane_dwords(m) for m in ms]), "mask_unpack", 4)
    big.pads_ok()


def test_tile_numbers_past_65535_uint8(tiles16_u8):
    for name in ("dsic_tile_gather_u8", "dsic_tile_gather_u8_ov"):
        _check_gather_16(tiles16_u8, name)
    _check_masks_16(tiles16_u8, 7)
    _check_masks_16(tiles16_u8, None)


def test_tile_numbers_past_65535_uint16(tiles16_u16):
    for name in ("dsic_tile_gather_u16", "dsic_tile_gather_u16_ov"):
        _check_gather_16(tiles16_u16, name, SCALE4[:3])
    _check_masks_16(tiles16_u16, None)
    _check_quantize(tiles16_u16, _tiles16_rows(tiles16_u16.scene)[1], SCALE4[:3], 2, FIRST, COUNT)


MIXED = [66048, 3, 65535, 65536, 0, 65534, 66000, 65283, 256, 65793]   # tile numbers on either side of 65535


@pytest.mark.parametrize("kind", ["u8", "u16", "f32", "hw"])
def test_tile_numbers_past_65535_in_the_writers(images, kind):
    images.clear()
    canvas = Canvas(kind, 8209, 8209, 1 if kind == "hw" else 3, f"a {kind} image of 66049 tiles")
    lists = [MIXED[:6], MIXED[6:] + [-1, 66049]]
    if kind != "hw":
        _check_stitch(canvas, lists, SCALE4[:3])
        canvas.out.view.fill_(SENTINEL)
    if kind in ("u8", "u16"):
        _check_stitch(canvas, lists, SCALE4[:3], tau=3 if kind == "u8" else 300)
        canvas.out.view.fill_(SENTINEL)
    _check_mask_writer(canvas, lists, 9)


def test_band_histogram_u16_with_nodata_and_validity(tiles16_u16, golden):
    s = tiles16_u16.scene
    for case, with_valid in (("nodata", False), ("valid_nodata", True)):
        got = _histogram(tiles16_u16, "dsic_band_histogram_u16", with_valid, s.nodata)
        assert np.array_equal(got, golden[f"tiles16_u16_{case}"]), case
    assert s.H * s.W > int(golden["tiles16_u16_nodata"][0].sum()) > int(golden["tiles16_u16_valid_nodata"][0].sum()) > 0
    tiles16_u16.pads_ok()


# ---- the blend: tile_blend_window_f32 into a canvas of the whole image, then the finishes --------------------------------
OVERLAP = 16


def _blend_ids(H, W, y, x):
    """64 tiles of the overlapped grid, ascending: 32 of the tile row whose support begins at or before row y and 32 of
    the one above it (below it for the first), around column x; their ramps meet in both directions"""
    import blend_ref
    ay, ax = blend_ref.grid(H, W, TILE, TILE, OVERLAP)
    i = min(y // ay["s"], ay["n"] - 1)
    rows = (i - 1, i) if i else (0, 1)
    j0 = min(max(x // ax["s"] - 16, 0), ax["n"] - 32)
    return [r * ax["n"] + j for r in rows for j in range(j0, j0 + 32)]


def _check_blend(canvas, id_lists):
    """One call per id list (their supports share no row), each compared over the rows of its supports; the rest of the
    canvas keeps its zeros.  Returns the row ranges written."""
    L = lib.load()
    H, W, C = canvas.H, canvas.W, canvas.C
    held, spans = [], []
    for k, ids in enumerate(id_lists):
        assert ids == sorted(set(ids)) and len(ids) <= 64
        tiles = _some_tiles(len(ids), C, 50 + k)
        held.append((tiles, torch.from_numpy(tiles).cuda(), _i32(ids)))
        lib.check(L.dsic_tile_blend_window_f32(_p(held[-1][1]), _p(held[-1][2]), len(ids), _p(canvas.out.view), H, W, C, TILE,
                                               TILE, OVERLAP, 0, 0, H, W, _stream()), "tile_blend_window_f32")
    torch.cuda.synchronize()
    for (tiles, _, _), ids in zip(held, id_lists):
        mine = B.blend_support_rows(ids, H, W, TILE, TILE, OVERLAP)
        assert not any(a < d and c < b for a, b in mine for c, d in spans), "the calls' supports must not share rows"
        spans += mine
        for a, b in mine:
            want = B.blend_rows(tiles, ids, H, W, C, TILE, TILE, OVERLAP, a, b)
            assert want.any()
            _same(canvas.rows(a, b), want, f"tile_blend_window_f32 {H}x{W}x{C} rows [{a}, {b})", 4)
    canvas.untouched_rows(spans, "tile_blend_window_f32")
    return spans


def test_blend_window_and_the_finishes_on_a_canvas_past_2_32_bytes(images):
    """the canvas is the whole image; calls at its first rows, at every crossing and at its last rows"""
    L = lib.load()
    images.clear()
    scene = S.table()["f32c3"]
    H, W, C = scene.H, scene.W, scene.C
    canvas = Canvas("f32", H, W, C, "a whole float32 canvas", sentinel=0)
    assert canvas.out.n > 1 << 32
    points = [(0, 0), (H - 1, W - 1)] + [(int(y), int(x)) for y, x, _ in (scene.coords(e) for e in scene.crossings().values())]
    spans = _check_blend(canvas, [_blend_ids(H, W, y, x) for y, x in points])
    assert len(spans) == 5
    # the finish into uint8: the blended rows, and rows drawn with a fixed seed (zeros but inside a support)
    rb = W * C
    out = BigOut(H * rb, "tile_blend_finish_u8")
    lib.check(L.dsic_tile_blend_finish_u8(_p(canvas.out.view), _p(out.view), C, H, W, _stream()), "tile_blend_finish_u8")
    for y0, y1 in spans + _bands(H, _crossing_rows(rb, H), 8):
        _same(out.bytes(y0 * rb, y1 * rb), B.finish_rows(canvas.rows(y0, y1), "u8"), f"blend_finish_u8 rows [{y0}, {y1})")
    out.guards_ok("tile_blend_finish_u8")
    del out
    # the float32 finish in place
    before = {(a, b): canvas.rows(a, b) for a, b in spans}
    lib.check(L.dsic_tile_blend_finish_f32(_p(canvas.out.view), C, H, W, _stream()), "tile_blend_finish_f32")
    for (a, b), rows in before.items():
        _same(canvas.rows(a, b), B.finish_rows(rows, "f32"), f"blend_finish_f32 rows [{a}, {b})", 4)
    canvas.untouched_rows(spans, "tile_blend_finish_f32")


def test_tile_numbers_past_65535_in_the_blend(images):
    images.clear()
    canvas = Canvas("f32", 8209, 8209, 3, "a float32 canvas of 263169 overlapped tiles", sentinel=0)
    _check_blend(canvas, [sorted(MIXED)])


def test_a_grid_of_over_2_31_blocks_is_refused_and_nothing_is_written():
    """tile numbers are ints: the tile calls refuse an image whose padded size holds over 2^31 - 1 blocks of 16 x 16"""
    L = lib.load()
    img = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    out, ids = Out(4096), _i32([0])
    lohi = _lohi(SCALE4[:3])
    side = 1 << 20                                                            # 2^16 x 2^16 blocks = 2^32
    for H, W in ((side, side), (2 ** 31 - 8, 32), (32, 2 ** 31 - 1)):
        calls = [L.dsic_tile_gather_u8(_p(img), _p(out.view), H, W, 3, 32, 32, 0, 1, _stream()),
                 L.dsic_tile_gather_f32_ov(_p(img), _p(out.view), H, W, 3, 32, 32, 16, 0, 1, _stream()),
                 L.dsic_tile_gather_u16(_p(img), _p(out.view), H, W, 3, 32, 32, lohi, 0, 1, _stream()),
                 L.dsic_tile_stitch_window_u8(_p(img), _p(ids), 1, _p(out.view), H, W, 3, 32, 32, 0, 0, 1, 1, _stream()),
                 L.dsic_tile_stitch_window_u16(_p(img), _p(ids), 1, _p(out.view), H, W, 3, 32, 32, 0, 0, 1, 1, lohi,
                                               _stream()),
                 L.dsic_tile_blend_window_f32(_p(img), _p(ids), 1, _p(out.view), H, W, 3, 32, 32, 16, 0, 0, 1, 1, _stream()),
                 L.dsic_mask_classify_u8(_p(img), H, W, 3, 32, 32, 7, 0, 1, _p(out.view), _stream()),
                 L.dsic_valid_delta_planes(_p(img), H, W, 32, 32, _p(ids), 1, _p(out.view), _p(out.view[2048:]), _stream()),
                 L.dsic_mask_apply_u8(None, 0, _p(_i32([0, -1])), 1, 7, _p(out.view), H, W, 3, 32, 32, 0, 0, 1, 1, _stream())]
        assert calls == [lib.DSIC_EINVAL] * len(calls), (H, W, calls)
        assert b"blocks of 16 x 16" in L.dsic_last_error(), (H, W)
    # one block fewer along a side is inside the limit: the refusal is then another one (the tile is outside the grid)
    assert L.dsic_tile_gather_u8(_p(img), _p(out.view), 2 ** 15 * 16, (2 ** 16 - 1) * 16, 3, 32, 32, 2 ** 31 - 2, 1,
                                 _stream()) == lib.DSIC_EINVAL
    assert b"outside the grid" in L.dsic_last_error()
    assert (out.host("refused calls") == 0x5A).all() and not bool(img.any())


def test_the_module_stayed_within_12_gib(images):
    images.clear()
    peak = torch.cuda.max_memory_allocated()
    print(f"peak device memory of the large-image tests: {peak / GIB:.2f} GiB")
    assert peak <= LIMIT
