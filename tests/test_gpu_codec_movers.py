"""The image codec's byte movers alone, bit for bit against the NumPy restatement of tests/codec_ref.py: the tile
gathers and stitches, the DSIC2 / DSIC3 container pack, the container scatter and dsic_strings_scatter_select (and
with them copy_bytes, load16_any and block_exclusive_scan), then the layout helpers of layout.hip and the uint8 image
conversion.  No model: every shape is the smallest that reaches a branch of the kernels.

Every output lies between guards inside one allocation (float32: NaN guards around an interior pre-filled with a
finite sentinel; integers: 0xCD bytes around an interior pre-filled with another value), and the guards are checked
after every call.  Every input lies inside a larger allocation of the test's own, so a wrong read returns a wrong
value, not a fault."""
import numpy as np
import pytest
import torch

import codec_ref as R
from dsic_amd import lib
from dsic_amd.ops import _p, _stream

pytestmark = pytest.mark.gpu

GUARD = 64                                   # elements on either side: 64 bytes at least, so interiors stay 16-byte aligned
GUARDS = {np.dtype(np.uint8): 0xCD, np.dtype(np.int32): -0x32323233, np.dtype(np.int64): -0x3232323232323233,
          np.dtype(np.float32): float("nan")}
PADS = {np.dtype(np.uint8): 0xEE, np.dtype(np.int32): 0x0BADBAD0, np.dtype(np.int64): 0x0BADBAD0,
        np.dtype(np.float32): 1e30}           # what surrounds an input
U8_FILL, F32_FILL, INT_FILL = 0x5A, -7.0, 0x71717171
GEOMETRIES = [(17, 33, 32),                  # one tile row, 15 reflected rows and columns, W*3 % 4 = 3
              (33, 35, 32),                  # 2 x 2 tiles, the last of each axis shifted inward, W*3 % 4 = 1
              (40, 34, 32),                  # W*3 % 4 = 2
              (64, 36, 32),                  # exact tile rows, 16-byte aligned float rows
              (50, 100, 48)]                 # 2 x 3 tiles of 48 with origins 0, 48, 64
KINDS = [("u8", 3), ("u8", 4), ("f32", 1), ("f32", 3), ("f32", 4), ("f32", 8)]
_CACHE = {}


class Out:
    """n elements between guards inside one device allocation, the interior pre-filled."""

    def __init__(self, n, dtype, fill):
        self.dtype, self.n = np.dtype(dtype), int(n)
        host = np.full(GUARD + self.n + GUARD, GUARDS[self.dtype], dtype=self.dtype)
        host[GUARD:GUARD + self.n] = fill
        self.buf = torch.from_numpy(host).cuda()
        self.view = self.buf[GUARD:GUARD + self.n]

    def host(self, what=""):
        """The interior on the host, after the guards have been checked."""
        a = self.buf.cpu().numpy()
        g = np.concatenate([a[:GUARD], a[GUARD + self.n:]])
        if self.dtype == np.float32:
            assert np.isnan(g).all(), f"{what}: guard overwritten"
        else:
            assert (g == GUARDS[self.dtype]).all(), f"{what}: guard overwritten"
        return a[GUARD:GUARD + self.n]


def _inside(arr, offset=0):
    """The array's elements on the device, `offset` elements past an aligned point of a larger allocation."""
    flat = np.ascontiguousarray(arr).ravel()
    host = np.full(GUARD + offset + flat.size + GUARD, PADS[flat.dtype], dtype=flat.dtype)
    host[GUARD + offset:GUARD + offset + flat.size] = flat
    return torch.from_numpy(host).cuda()[GUARD + offset:GUARD + offset + flat.size]


def _same(got, want, what):
    """bit for bit (a float32 -0.0 is not 0.0)"""
    want = np.ascontiguousarray(want).ravel()
    assert got.dtype == want.dtype and got.size == want.size, what
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero((got.view(np.uint8).reshape(got.size, -1) != want.view(np.uint8).reshape(got.size, -1))
                             .any(axis=1))
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {got.size} differ, first at {i}: got {got[i]!r}, want {want[i]!r}")


# ---- gathers ------------------------------------------------------------------------------------------------------
def _image(H, W, kind, C):
    key = ("image", H, W, kind, C)
    if key not in _CACHE:
        rng = np.random.default_rng(H * 100003 + W * 101 + C)
        img = (rng.integers(0, 256, size=(H, W, C), dtype=np.uint8) if kind == "u8"
               else rng.random((C, H, W), dtype=np.float32))
        img.setflags(write=False)
        _CACHE[key] = img
    return _CACHE[key]


@pytest.mark.parametrize("H,W,tile", GEOMETRIES)
@pytest.mark.parametrize("kind,C", KINDS)
def test_gathers_equal_the_restatement(H, W, tile, kind, C):
    L = lib.load()
    img = _image(H, W, kind, C)
    want = (R.gather_u8 if kind == "u8" else R.gather_f32)(img, tile, tile)
    n = want.shape[0]
    per_tile = want[0].size
    dtype, fill = (np.uint8, U8_FILL) if kind == "u8" else (np.float32, F32_FILL)
    splits = {"one call": [(0, n)], "first = 1": [(1, n - 1)], "one tile per call": [(t, 1) for t in range(n)]}
    for off in range(4):                                                 # bytes (uint8) or floats (float32)
        d_img = _inside(img, off)
        for name, extra in ((f"dsic_tile_gather_{kind}", ()), (f"dsic_tile_gather_{kind}_ov", (0,))):
            for split, calls in splits.items():
                for first, cnt in calls:
                    out = Out(cnt * per_tile, dtype, fill)
                    lib.check(getattr(L, name)(_p(d_img), _p(out.view), H, W, C, tile, tile, *extra, first, cnt,
                                               _stream()), name)
                    what = f"{name} offset {off}, {split}, tiles [{first}, {first + cnt})"
                    _same(out.host(what), want[first:first + cnt], what)


# ---- stitches -----------------------------------------------------------------------------------------------------
def _edge_values():
    k = (np.arange(256, dtype=np.float32) / np.float32(255.0)).astype(np.float32)
    return np.concatenate([np.nextafter(k, np.float32(-1)), k, np.nextafter(k, np.float32(2)),
                           np.float32([-0.0, 1.0]), np.nextafter(np.float32([1.0]), np.float32(2))]).astype(np.float32)


def _tiles(H, W, tile, C):
    """float32 [n][C][th][tw] in [-0.25, 1.25]; every k/255 with its two float32 neighbours, -0.0, 1.0 and the float
    above 1.0 planted among the pixels each tile owns inside the image (as many as fit)."""
    key = ("tiles", H, W, tile, C)
    if key not in _CACHE:
        g = R.grid(H, W, tile, tile)
        rng = np.random.default_rng(H * 7919 + W * 31 + C)
        t = rng.uniform(-0.25, 1.25, size=(g["n"], C, tile, tile)).astype(np.float32)
        edge = _edge_values()
        for k in range(g["n"]):
            i, j = divmod(k, g["nx"])
            (ya, yb), (xa, xb) = g["own_y"][i], g["own_x"][j]
            yy, xx = np.meshgrid(np.arange(ya, min(yb, H)) - g["ys"][i], np.arange(xa, min(xb, W)) - g["xs"][j],
                                 indexing="ij")
            cells = np.stack([yy.ravel(), xx.ravel()], 1)
            for c in range(C):
                m = min(len(cells), edge.size)
                pos = cells[rng.permutation(len(cells))[:m]]
                t[k, c, pos[:, 0], pos[:, 1]] = rng.permutation(edge)[:m]
        t.setflags(write=False)
        _CACHE[key] = t
    return _CACHE[key]


def _windows(H, W, tile):
    x_seam = min(tile - 2, W - 5)                                        # 5 wide across the seam at column `tile`
    assert x_seam < tile < x_seam + 5
    return [(0, 0, H, W), (1, 1, H - 2, W - 3), (H - 1, W - 1, 1, 1), (H // 2, x_seam, 3, 5), (0, tile, H, 1),
            (H // 2 + 1, 0, 1, W)]


def _pick(tiles, ids):
    dummy = np.full_like(tiles[0], 0.5)
    return np.stack([tiles[t] if 0 <= t < len(tiles) else dummy for t in ids])


def _stitch_out(kind, C, h, w):
    return Out(C * h * w, np.uint8 if kind == "u8" else np.float32, U8_FILL if kind == "u8" else F32_FILL)


def _fill(kind):
    return U8_FILL if kind == "u8" else np.float32(F32_FILL)


@pytest.mark.parametrize("H,W,tile", GEOMETRIES)
@pytest.mark.parametrize("kind,C", KINDS)
def test_window_stitches_equal_the_restatement(H, W, tile, kind, C):
    L = lib.load()
    fn = getattr(L, f"dsic_tile_stitch_window_{kind}")
    tiles = _tiles(H, W, tile, C)
    g = R.grid(H, W, tile, tile)
    n = g["n"]
    every = list(range(n))
    for win in _windows(H, W, tile):
        wy, wx, wh, ww = win
        corner = (wy // tile) * g["nx"] + wx // tile                     # the tile that owns the window's first pixel
        id_lists = {"ascending": every, "reversed": every[::-1],
                    "one left out": [t for t in every if t != corner],
                    "foreign numbers": [-1] + every + [n, n + 5],
                    "a repeated id": every + [corner]}
        for name, ids in id_lists.items():
            picked = _pick(tiles, ids)
            want = R.stitch(picked, ids, H, W, tile, tile, win, kind, _fill(kind))
            if name == "one left out":
                assert want.ravel()[0] == _fill(kind)                    # its pixels keep the fill
            d_tiles = _inside(picked)
            d_ids = _inside(np.array(ids, dtype=np.int32))
            out = _stitch_out(kind, C, wh, ww)
            lib.check(fn(_p(d_tiles), _p(d_ids), len(ids), _p(out.view), H, W, C, tile, tile, wy, wx, wh, ww,
                         _stream()), "stitch_window")
            what = f"stitch_window_{kind} window {win}, ids {name}"
            _same(out.host(what), want, what)


@pytest.mark.parametrize("H,W,tile", GEOMETRIES)
@pytest.mark.parametrize("kind,C", KINDS)
def test_whole_image_stitches_equal_the_restatement_and_the_window_call(H, W, tile, kind, C):
    L = lib.load()
    whole, window = getattr(L, f"dsic_tile_stitch_{kind}"), getattr(L, f"dsic_tile_stitch_window_{kind}")
    tiles = _tiles(H, W, tile, C)
    n = len(tiles)
    every = list(range(n))
    want = R.stitch(tiles, every, H, W, tile, tile, (0, 0, H, W), kind, _fill(kind))
    d_tiles = _inside(tiles)
    per_tile = tiles[0].size

    def run(calls):
        out = _stitch_out(kind, C, H, W)
        for first, cnt in calls:
            lib.check(whole(_p(d_tiles[first * per_tile:]), _p(out.view), H, W, C, tile, tile, first, cnt, _stream()),
                      "tile_stitch")
        return out.host(f"tile_stitch_{kind} {calls}")

    two, three = [(0, n // 2), (n // 2, n - n // 2)], [(t, 1) for t in range(n)][:2] + [(2, n - 2)][:n - 2]
    results = {}
    for calls in ([(0, n)], two, three, three[::-1]):
        results[str(calls)] = got = run(calls)
        _same(got, want, f"tile_stitch_{kind} in calls {calls}")
    # only the first of two calls: the pixels of the other tiles keep the fill
    _same(run(two[:1]), R.stitch(tiles[:n // 2], every[:n // 2], H, W, tile, tile, (0, 0, H, W), kind, _fill(kind)),
          f"tile_stitch_{kind}, first half only")
    out = _stitch_out(kind, C, H, W)
    d_ids = _inside(np.array(every, dtype=np.int32))
    lib.check(window(_p(d_tiles), _p(d_ids), n, _p(out.view), H, W, C, tile, tile, 0, 0, H, W, _stream()),
              "stitch_window")
    _same(out.host("window over the image"), results[str([(0, n)])], f"window_{kind} over (0, 0, H, W) against whole")


# ---- container pack -----------------------------------------------------------------------------------------------
CAP_Z, CAP_Y, TAG = 8, 36, 0xDEADBEEF
SHAPE = (4, 6, 5, 1, 2)                                                  # Hy, Wy, Nz, Hz, Wz


def _cycle(cap):
    out = []
    for v in (0, 1, 3, 15, 16, 17, 31, 33, cap - 1, cap):
        if v <= cap and v not in out:
            out.append(v)
    return out


def _batch(B, K):
    """rows of non-zero bytes, in-range lengths that cycle through the head / tail splits of copy_bytes, and meta with
    negative minima: (rows uint8 [B][cap_z + K cap_y], lengths int32 [B][1 + K], meta int32 [B][4])."""
    key = ("batch", B, K)
    if key not in _CACHE:
        rng = np.random.default_rng(B * 37 + K)
        rows = rng.integers(1, 256, size=(B, CAP_Z + K * CAP_Y), dtype=np.uint8)
        zc, yc = _cycle(CAP_Z), _cycle(CAP_Y)
        lengths = np.zeros((B, 1 + K), dtype=np.int32)
        iy = 0
        for b in range(B):
            lengths[b, 0] = zc[(b + b // 3) % len(zc)]                   # drifts against the y cycle: see B = 300
            for j in range(K):
                lengths[b, 1 + j] = yc[iy % len(yc)]
                iy += 1
        meta = np.stack([rng.integers(-40, 1, B), rng.integers(1, 90, B), rng.integers(-9, 1, B),
                         rng.integers(1, 20, B)], 1).astype(np.int32)
        meta[0, 0], meta[0, 2] = -40, -9
        for a in (rows, lengths, meta):
            a.setflags(write=False)
        _CACHE[key] = (rows, lengths, meta)
    return _CACHE[key]


def _capacity(B, K):
    """the bytes the header documents for out"""
    if K == 1:
        return 38 + 24 * B + B * (CAP_Z + CAP_Y)
    return 42 + (24 + 4 * K) * B + B * (CAP_Z + K * CAP_Y)


def _pack(rows, lengths, meta, K, err):
    """One pack call -> (out bytes [capacity] on the host, workspace on the host, the Out of the container)."""
    L = lib.load()
    B = rows.shape[0]
    out = Out(_capacity(B, K), np.uint8, U8_FILL)
    ws = Out(B * (1 + K) + 3, np.int64, INT_FILL)
    d_rows, d_len, d_meta = _inside(rows), _inside(lengths), _inside(meta)
    d_err = None if err is None else _inside(np.array([err], dtype=np.int32))
    My = 16 * K
    if K == 1:
        rc = L.dsic_container_pack(_p(d_rows), CAP_Z, CAP_Y, _p(d_len), _p(d_meta), _p(d_err), B, TAG, My, *SHAPE,
                                   _p(ws.view), _p(out.view), _stream())
    else:
        rc = L.dsic_container_pack_seg(_p(d_rows), CAP_Z, CAP_Y, K, _p(d_len), _p(d_meta), _p(d_err), B, TAG, My,
                                       *SHAPE, _p(ws.view), _p(out.view), _stream())
    lib.check(rc, "container_pack")
    return out.host("container"), ws.host("workspace"), out


def _check_pack(rows, lengths, meta, K, err, what):
    B = rows.shape[0]
    blob, total, offsets = R.pack_container(rows, lengths, meta, TAG, 16 * K, *SHAPE, CAP_Z, CAP_Y, K)
    got, ws, _ = _pack(rows, lengths, meta, K, err)
    assert int(ws[0]) == total, (what, int(ws[0]), total)
    assert int(ws[1]) == (0 if err is None else err), what
    _same(ws[2:], np.array(offsets, dtype=np.int64), f"{what}: string offsets")
    assert total <= _capacity(B, K)
    _same(got[:total], np.frombuffer(blob, dtype=np.uint8), f"{what}: container bytes")
    assert (got[total:] == U8_FILL).all(), f"{what}: bytes behind the container were written"


@pytest.mark.parametrize("B", [1, 3, 300])
@pytest.mark.parametrize("K", [1, 2, 16])
def test_container_pack_equals_the_restatement(B, K):
    rows, lengths, meta = _batch(B, K)
    if B == 300:
        # every length of the cycle meets every residue of the destination (out is 16-byte aligned); more than 256
        # strings, so the scan carries between rounds; and the copies stay under 100 KiB
        _, _, offsets = R.pack_container(rows, lengths, meta, TAG, 16 * K, *SHAPE, CAP_Z, CAP_Y, K)
        body = 38 + 24 * B + (4 + 4 * B * K if K > 1 else 0)
        seen = {(int(n), (body + o) % 16) for n, o in zip(lengths.ravel(), offsets)}
        assert {(n, r) for n in _cycle(CAP_Y) for r in range(16)} <= seen
        assert offsets[-1] < 100 * 1024
    _check_pack(rows, lengths, meta, K, None, f"B={B} K={K} err=NULL")
    _check_pack(rows, lengths, meta, K, 5, f"B={B} K={K} err=5")


@pytest.mark.parametrize("K", [1, 2, 16])
def test_container_pack_clamps_forged_lengths(K):
    rows, lengths, meta = _batch(3, K)
    forged = lengths.copy()
    forged[0, 0], forged[0, 1] = -1, CAP_Y + 1
    forged[1, 0], forged[1, K] = CAP_Z + 1, 2 ** 31 - 1
    forged[2, 0], forged[2, 1] = 2 ** 31 - 1, -1
    _check_pack(rows, forged, meta, K, None, f"forged lengths K={K}")


# ---- container scatter and select -----------------------------------------------------------------------------
def _padded(blob_bytes, spare=16):
    """bytes -> uint8 array of whole 16-byte chunks and a spare one, as the header asks of a blob"""
    a = np.frombuffer(bytes(blob_bytes), dtype=np.uint8)
    host = np.full(R.ceil16(a.size) + spare, 0x99, dtype=np.uint8)
    host[:a.size] = a
    return host


def _scatter(d_blob, blob_bytes, B, zstride, ystride, max_len, what):
    L = lib.load()
    z, y = Out(B * zstride, np.uint8, U8_FILL), Out(B * ystride, np.uint8, U8_FILL)
    lengths, meta = Out(2 * B, np.int32, INT_FILL), Out(4 * B, np.int32, INT_FILL)
    ws = Out(2 * B + 3, np.int64, INT_FILL)
    lib.check(L.dsic_container_scatter(_p(d_blob), blob_bytes, B, max_len, _p(z.view), zstride, _p(y.view), ystride,
                                       _p(lengths.view), _p(meta.view), _p(ws.view), _stream()), "container_scatter")
    ws.host(f"{what}: workspace")
    return (z.host(f"{what}: zbuf"), y.host(f"{what}: ybuf"), lengths.host(f"{what}: lengths"),
            meta.host(f"{what}: meta"))


def _select(d_blob, blob_bytes, desc, zstride, ystride, max_len, what):
    L = lib.load()
    n = len(desc)
    z, y = Out(n * zstride, np.uint8, U8_FILL), Out(n * ystride, np.uint8, U8_FILL)
    lengths = Out(2 * n, np.int32, INT_FILL)
    d_desc = _inside(np.asarray(desc, dtype=np.int64))
    lib.check(L.dsic_strings_scatter_select(_p(d_blob), blob_bytes, _p(d_desc), n, max_len, _p(z.view), zstride,
                                            _p(y.view), ystride, _p(lengths.view), _stream()), "scatter_select")
    return z.host(f"{what}: zbuf"), y.host(f"{what}: ybuf"), lengths.host(f"{what}: lengths")


def _check_scatter(host_blob, blob_bytes, B, what, zstride=CAP_Z, ystride=CAP_Y):
    want = R.scatter(host_blob, blob_bytes, B, zstride, ystride, U8_FILL)
    got = _scatter(_inside(host_blob), blob_bytes, B, zstride, ystride, max(zstride, ystride), what)
    for g, w, name in zip(got, want, ("z rows", "y rows", "lengths", "meta")):
        _same(g, w, f"{what}: {name}")
    return want


def _check_select(host_blob, blob_bytes, desc, what, zstride=CAP_Z, ystride=CAP_Y):
    want = R.scatter_select(host_blob, blob_bytes, desc, zstride, ystride, U8_FILL)
    got = _select(_inside(host_blob), blob_bytes, desc, zstride, ystride, max(zstride, ystride), what)
    for g, w, name in zip(got, want, ("z rows", "y rows", "lengths")):
        _same(g, w, f"{what}: {name}")
    return want


@pytest.mark.parametrize("B", [1, 3, 300])
def test_pack_then_scatter_on_the_device_returns_the_rows(B):
    rows, lengths, meta = _batch(B, 1)
    got, ws, out = _pack(rows, lengths, meta, 1, None)
    total = int(ws[0])
    zrows, yrows, got_len, got_meta = _scatter(out.view, total, B, CAP_Z, CAP_Y, CAP_Y, f"round trip B={B}")
    _same(got_len, lengths, "lengths")
    _same(got_meta, meta, "meta")
    base = 38 + 24 * B
    desc = [[base + int(ws[2 + 2 * b]), lengths[b, 0], base + int(ws[3 + 2 * b]), lengths[b, 1]] for b in range(B)]
    zsel, ysel, len_sel = _select(out.view, total, desc, CAP_Z, CAP_Y, CAP_Y, f"round trip select B={B}")
    _same(len_sel, lengths, "select lengths")
    for zr, yr in ((zrows, yrows), (zsel, ysel)):
        zr, yr = zr.reshape(B, CAP_Z), yr.reshape(B, CAP_Y)
        for b in range(B):
            nz, ny = lengths[b]
            assert np.array_equal(zr[b, :nz], rows[b, :nz]) and (zr[b, nz:] == U8_FILL).all(), b
            assert np.array_equal(yr[b, :ny], rows[b, CAP_Z:CAP_Z + ny]) and (yr[b, ny:] == U8_FILL).all(), b


def _reference_blob(B):
    rows, lengths, meta = _batch(B, 1)
    blob, total, offsets = R.pack_container(rows, lengths, meta, TAG, 16, *SHAPE, CAP_Z, CAP_Y, 1)
    return blob, total, offsets, lengths


def _set_len(host, b, which, value):
    at = 38 + 24 * b + 16 + 4 * which
    host[at:at + 4] = np.frombuffer(np.array([value & 0xFFFFFFFF], dtype="<u4").tobytes(), dtype=np.uint8)


def test_container_scatter_equals_the_restatement_on_sound_and_forged_records():
    B = 300
    blob, total, offsets, lengths = _reference_blob(B)
    base = 38 + 24 * B
    # the test's blobs start 16-byte aligned: strings of a chunk or more begin at every residue of the source address
    assert {(base + o) % 16 for n, o in zip(lengths.ravel(), offsets) if n >= 16} == set(range(16))
    host = _padded(blob)
    want = _check_scatter(host, total, B, "sound container")
    assert np.array_equal(want[2], lengths)
    # blob_bytes cuts the last strings short
    _check_scatter(host, total - 7, B, "blob_bytes inside the last string")
    _check_scatter(host, base + offsets[2 * B - 3] + 1, B, "blob_bytes inside an earlier string")
    # lengths over the strides (later strings move with them), the last string running past blob_bytes
    forged = host.copy()
    _set_len(forged, 2, 0, CAP_Z + 5)
    _set_len(forged, 3, 1, CAP_Y + 100)
    assert lengths[B - 2, 1] < CAP_Y and lengths[B - 1, 1] == CAP_Y
    _set_len(forged, B - 2, 1, CAP_Y)
    _check_scatter(forged, total, B, "lengths over the stride and past the blob")
    # a negative length: nothing behind it is inside the blob any more
    forged = host.copy()
    _set_len(forged, 1, 0, -3)
    want = _check_scatter(forged, total, B, "negative length")
    assert (want[0][1:] == U8_FILL).all() and (want[1][1:] == U8_FILL).all()


def test_scatter_select_equals_the_restatement_on_sound_and_forged_descriptors():
    blob, total, _, _ = _reference_blob(40)
    host = _padded(blob)
    lens = _cycle(CAP_Y)
    # offsets at all 16 residues, lengths through every head / tail split, rows at every destination residue mod 16
    desc = [[100 + r, _cycle(CAP_Z)[r % 5], 333 + 17 * r, lens[r % len(lens)]] for r in range(16)]
    desc += [[7 + r, CAP_Z, 200 + r, lens[(r + 5) % len(lens)]] for r in range(16)]
    assert {d[0] % 16 for d in desc} == set(range(16)) and {d[2] % 16 for d in desc} == set(range(16))
    want = _check_select(host, total, desc, "sound descriptors")
    assert np.array_equal(want[2], np.array([[d[1], d[3]] for d in desc]))
    forged = [[0, CAP_Z + 1, 0, CAP_Y + 1000],                           # over the stride
              [total - 3, CAP_Z, total - 20, CAP_Y],                     # running past blob_bytes
              [-4, 4, -4, 20],                                           # offsets outside the blob
              [total, 4, total, 20],
              [total + 1, 4, total + 1, 20],
              [16, -1, 5, -2 ** 40],                                     # negative lengths
              [2 ** 40, 4, -2 ** 40, 4],
              [33, 2 ** 40, 1, 2 ** 62]]
    want = _check_select(host, total, forged, "forged descriptors")
    assert want[2].tolist() == [[CAP_Z, CAP_Y], [3, 20], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [CAP_Z, CAP_Y]]
    _check_select(host, total - 5, forged[:2] + desc[:4], "blob_bytes below the blob's end")


def test_long_strings_split_over_several_workgroups():
    """max_len over 4 KiB: copy_bytes runs in more than one workgroup per string"""
    blob, total, _, _ = _reference_blob(300)
    assert total > 9100
    host = _padded(blob)
    desc = [[5, 8, 3, 9000], [77, 1, 101, 8999], [0, 0, 38, 4097]]
    _check_select(host, total, desc, "long strings", zstride=8, ystride=9000)


# ---- layout.hip and the image conversion ----------------------------------------------------------------------
@pytest.mark.parametrize("R_,Cc", [(1, 1), (31, 33), (32, 32), (33, 65), (5, 192)])
@pytest.mark.parametrize("B", [1, 3])
def test_transposes_equal_numpy(R_, Cc, B):
    L = lib.load()
    rng = np.random.default_rng(R_ * 1000 + Cc + B)
    src = rng.standard_normal((B, R_, Cc)).astype(np.float32)
    want = np.ascontiguousarray(src.transpose(0, 2, 1))
    d_src = _inside(src, 1)
    # NCHW [B][C][H*W] -> NHWC: rows are channels; NHWC [B][H*W][C] -> NCHW: rows are pixels
    out = Out(src.size, np.float32, F32_FILL)
    lib.check(L.dsic_nchw_to_nhwc(_p(d_src), _p(out.view), B, R_, 1, Cc, _stream()), "nchw_to_nhwc")
    _same(out.host("nchw_to_nhwc"), want, "nchw_to_nhwc")
    out = Out(src.size, np.float32, F32_FILL)
    lib.check(L.dsic_nhwc_to_nchw(_p(d_src), _p(out.view), B, R_, 1, Cc, _stream()), "nhwc_to_nchw")
    _same(out.host("nhwc_to_nchw"), want, "nhwc_to_nchw")
    if R_ > 1 and R_ % 3 == 0:                                            # H x W = 3 x R/3: the same bytes
        out = Out(src.size, np.float32, F32_FILL)
        lib.check(L.dsic_nhwc_to_nchw(_p(d_src), _p(out.view), B, 3, R_ // 3, Cc, _stream()), "nhwc_to_nchw")
        _same(out.host("nhwc_to_nchw"), want, "nhwc_to_nchw 3 x R/3")


@pytest.mark.parametrize("H,W,pad_h,pad_w", [(5, 7, 4, 6), (17, 33, 15, 15), (8, 8, 0, 0), (9, 4, 0, 3)])
def test_reflect_pad_br_equals_numpy(H, W, pad_h, pad_w):
    L = lib.load()
    planes = 3
    src = np.random.default_rng(H * 100 + W).standard_normal((planes, H, W)).astype(np.float32)
    want = np.pad(src, ((0, 0), (0, pad_h), (0, pad_w)), mode="reflect")
    py, px = np.arange(H + pad_h), np.arange(W + pad_w)
    iy, ix = np.where(py < H, py, 2 * (H - 1) - py), np.where(px < W, px, 2 * (W - 1) - px)
    assert np.array_equal(want, src[:, iy][:, :, ix])                     # numpy's reflect is the 2*(L-1) - p rule
    out = Out(want.size, np.float32, F32_FILL)
    lib.check(L.dsic_reflect_pad_br(_p(_inside(src, 1)), _p(out.view), planes, H, W, pad_h, pad_w, _stream()),
              "reflect_pad_br")
    _same(out.host("reflect_pad_br"), want, "reflect_pad_br")


@pytest.mark.parametrize("C", range(1, 9))
def test_image_to_nhwc8_equals_numpy(C):
    L = lib.load()
    B, H, W = 2, 7, 37
    src = np.random.default_rng(C).standard_normal((B, C, H, W)).astype(np.float32)
    src[src == 0] = 1.0
    want = np.zeros((B, H, W, 8), dtype=np.float32)
    want[..., :C] = src.transpose(0, 2, 3, 1)
    out = Out(want.size, np.float32, F32_FILL)
    lib.check(L.dsic_image_to_nhwc8(_p(_inside(src, 1)), _p(out.view), B, C, H, W, _stream()), "image_to_nhwc8")
    got = out.host("image_to_nhwc8")
    _same(got, want, "image_to_nhwc8")
    assert got.reshape(B, H, W, 8)[..., C:].tobytes() == bytes(4 * B * H * W * (8 - C))   # +0.0, bit for bit


@pytest.mark.parametrize("C", [3, 4])
def test_image_u8hwc_to_f32nchw_equals_numpy(C):
    L = lib.load()
    B, H, W = 2, 5, 13
    rng = np.random.default_rng(C)
    flat = np.concatenate([np.arange(256), rng.integers(0, 256, B * H * W * C - 256)]).astype(np.uint8)
    src = rng.permutation(flat).reshape(B, H, W, C)
    assert len(np.unique(src)) == 256
    want = src.transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255.0)   # the kernel divides: (float)v / 255.0f
    assert want.dtype == np.float32
    for off in range(4):
        out = Out(want.size, np.float32, F32_FILL)
        lib.check(L.dsic_image_u8hwc_to_f32nchw(_p(_inside(src, off)), _p(out.view), B, C, H, W, _stream()),
                  "image_u8hwc_to_f32nchw")
        _same(out.host("image_u8hwc_to_f32nchw"), want, f"image_u8hwc_to_f32nchw offset {off}")
