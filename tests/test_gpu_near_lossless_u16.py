"""Bounded-error mode for uint16 imagery on the GPU: compress_image(tolerance=tau) decodes to within tau of the image
on every pixel and band (tau = 0: the image, also outside the scale), equals tests/residual16_ref.py applied to the
version-6 decode of the same call, keeps the version-6 containers byte for byte, decodes by region, through overviews
and through ImageReader, and its kernels equal numpy and the coder oracle element by element between guards.

Synthetic weights: the lossy layer predicts poorly, so the residuals are wide, which is the hard case.  C = 1 is held
at kernel level only: synthetic.make_state_dict(in_ch=1) builds weights, but the model's first layer takes an image of
3 or 4 channels (conv_first), so no one-band model exists to code a scene end to end."""
import io

import numpy as np
import pytest
import torch

import residual16_ref as R
import residual_ref as R8
from dsic_amd import codec, lib, residual, residual16
from dsic_amd import synthetic as S
from dsic_amd.model import CompressionModel
from dsic_amd.ops import _p, _stream
from oracle import entropy_ref as E
from test_residual16_cpu import _lohi, check_argument_refusals

pytestmark = pytest.mark.gpu
_MODELS = {}
_SCENES = {}


def _model(in_ch=3, N=128, M=192):
    if in_ch not in _MODELS:
        sd = S.make_state_dict(seed=1, N=N, M=M, in_ch=in_ch, spatial_params=False)
        m = CompressionModel(N=N, M=M, spatial_params=False, min_nu=2, max_nu=100.0, in_ch=in_ch)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        _MODELS[in_ch] = m.cuda().eval()
    return _MODELS[in_ch]


def _scene_u16(seed, H, W, C=3, top=10000.0):
    x = S.make_patches(seed, 1, H, W, C)[0].astype(np.float64)         # [C, H, W] in [0, 1]
    img = np.ascontiguousarray((x * top + 0.5).astype(np.uint16).transpose(1, 2, 0))
    img.setflags(write=False)
    return img


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _np(t):
    return t.cpu().view(torch.int16).numpy().view(np.uint16)


def _scene(name, H, W, tile, batch, C=3, top=10000.0, **kw):
    """(model, image, the version-6 stream and its uint16 decode), computed once and left unchanged."""
    if name not in _SCENES:
        model = _model(C)
        img = _scene_u16(31, H, W, C, top)
        plain = codec.compress_image(model, _dev(img), tile=tile, batch=batch, **kw)
        _SCENES[name] = (model, img, plain, _np(codec.decompress_image(model, plain)))
    return _SCENES[name]


def _near(name, H, W, tile, batch, tau, C=3, top=10000.0, **kw):
    key = (name, tau)
    if key not in _SCENES:
        model, img, _, _ = _scene(name, H, W, tile, batch, C, top, **kw)
        stream = codec.compress_image(model, _dev(img), tile=tile, batch=batch, tolerance=tau, **kw)
        _SCENES[key] = (stream, codec.decompress_image(model, stream))
    return _SCENES[key]


def _shifts(stream):
    return [r["r_k"] for r in codec.stream_index(stream)["tiles"]]


def _check_decode(name, H, W, tile, batch, tau, C=3, top=10000.0, **kw):
    model, img, plain, p = _scene(name, H, W, tile, batch, C, top, **kw)
    stream, out = _near(name, H, W, tile, batch, tau, C, top, **kw)
    x = img.astype(np.int64)
    assert out.dtype == torch.uint16 and tuple(out.shape) == (H, W, C)
    got = _np(out).astype(np.int64)
    err = int(np.abs(got - x).max())
    print(f"{name} tau={tau}: max |x' - x| = {err}, lossy max error {int(np.abs(p.astype(np.int64) - x).max())}, "
          f"stream {len(stream)} B (version 6: {len(plain)} B), k over tiles {sorted(_shifts(stream))}")
    if tau == 0:
        assert (got == x).all()
    assert err <= tau
    assert (got == R.reconstruct(p, R.quantize(x, p, tau), tau)).all()
    u, u6 = codec.unpack_image_stream(stream), codec.unpack_image_stream(plain)
    assert u["version"] == 9 and u["tolerance"] == tau and u6["version"] == 6 and u["scale"] == u6["scale"]
    assert u["blobs"] == u6["blobs"]                                   # the lossy layer is untouched
    assert len(u["residuals"]) == len(u["blobs"])
    assert codec.compress_image(model, _dev(img), tile=tile, batch=batch, tolerance=tau, **kw) == stream
    return model, img, stream, out


# ---- end to end ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau", [0, 3, 200])
def test_end_to_end_150x200(tau):
    """150 x 200: padded to 160 x 208, 12 tiles of 64 in batches of 5, 5 and 2, reflect padding on both axes, the last
    row and column of tiles shifted inward.  Both regimes of the split occur: at tau = 0 the wide residuals of the
    synthetic weights need raw planes, at tau = 200 a step of 401 leaves |q| <= 24 and every k is 0."""
    _, _, stream, _ = _check_decode("main", 150, 200, 64, 5, tau)
    assert codec.unpack_image_stream(stream)["batches"] == 3
    ks = _shifts(stream)
    if tau == 0:
        assert max(ks) >= 1
    if tau == 200:
        assert ks == [0] * 12


def test_one_tile_smaller_than_the_tile():
    """48 x 40 under tile 64: one tile of 48 x 48, row bands of 3 rows, 8 columns of reflect padding."""
    _, _, stream, _ = _check_decode("small", 48, 40, 64, 64, 0)
    ix = codec.stream_index(stream)
    assert (ix["th"], ix["tw"], len(ix["tiles"])) == (48, 48, 1)


@pytest.mark.parametrize("tau", [0, 50])
def test_four_bands(tau):
    """in_ch = 4, 96 x 80 at tile 32: 64 band channels per tile, 9 tiles in batches of 4."""
    _check_decode("four", 96, 80, 32, 4, tau, C=4)


def test_values_outside_an_explicit_scale_stay_lossless():
    """scale (2000, 6000) under data over 0 .. 10000: the predictor stays inside the scale, the residual carries the
    rest, and tau = 0 still returns the image."""
    _, img, stream, _ = _check_decode("clipped", 96, 80, 32, 4, 0, scale=[(2000, 6000)] * 3)
    assert img.min() < 2000 and img.max() > 6000
    assert codec.unpack_image_stream(stream)["scale"] == [(2000, 6000)] * 3


def test_a_quiet_scene_needs_no_planes():
    """values over 0 .. 200 at tau = 0: |q| <= 200, every k = 0 and the block carries no plane"""
    _, _, stream, _ = _check_decode("quiet", 96, 80, 32, 4, 0, top=200.0, scale=[(0, 200)] * 3)
    ix = codec.stream_index(stream)
    assert _shifts(stream) == [0] * 9
    assert all(r["r_len"] == 2 * 3 * r["r_L"] + sum(r["r_segs"]) for r in ix["tiles"])


def test_default_path_is_unchanged():
    model, img, plain, _ = _scene("main", 150, 200, 64, 5)
    again = codec.compress_image(model, _dev(img), tile=64, batch=5, tolerance=None)
    assert again == plain and codec.unpack_image_stream(plain)["version"] == 6


def test_segments_decode_to_the_same_image():
    model, img, _, _ = _scene("main", 150, 200, 64, 5)
    _, one = _near("main", 150, 200, 64, 5, 3)
    s4 = codec.compress_image(model, _dev(img), tile=64, batch=5, tolerance=3, segments=4)
    u = codec.unpack_image_stream(s4)
    assert u["version"] == 9 and u["segments"] == 4
    assert (_np(codec.decompress_image(model, s4)) == _np(one)).all()


def test_overviews_bound_level_0_only():
    model, img, _, _ = _scene("main", 150, 200, 64, 5)
    alone, full = _near("main", 150, 200, 64, 5, 3)
    p = codec.compress_image(model, _dev(img), tile=64, batch=5, tolerance=3, overviews=2)
    levels = codec.unpack_pyramid_stream(p)["levels"]
    assert levels[0]["stream"] == alone
    assert [codec.unpack_image_stream(lv["stream"])["version"] for lv in levels] == [9, 6, 6]
    assert (_np(codec.decompress_image(model, p)) == _np(full)).all()
    l1 = codec.decompress_image(model, p, level=1)
    assert l1.dtype == torch.uint16 and tuple(l1.shape) == (75, 100, 3)
    assert (_np(codec.decompress_region(model, p, 100, 150, 50, 50)) == _np(full)[100:150, 150:200]).all()


def _record_at(stream, t):
    """byte offset of tile t's record (smin, L, k, span) in its batch's block"""
    ix = codec.stream_index(stream)
    r = ix["tiles"][t]
    return ix["containers"][r["k"]]["r_offset"] + 30 + 16 * r["b"]


def test_decoders_refuse_a_forged_table_and_a_forged_shift():
    model, _, _, _ = _scene("main", 150, 200, 64, 5)
    stream, _ = _near("main", 150, 200, 64, 5, 3)
    r = codec.stream_index(stream)["tiles"][7]
    assert r["r_L"] >= 2
    forged = bytearray(stream)
    forged[r["r_off"] + 2:r["r_off"] + 4] = b"\x00\x00"               # c[1] = c[0] = 0
    with pytest.raises(ValueError, match="strictly increasing"):
        codec.decompress_image(model, bytes(forged))
    with pytest.raises(ValueError, match="strictly increasing"):
        codec.decompress_region(model, bytes(forged), 64, 192, 1, 1)
    forged = bytearray(stream)
    forged[_record_at(stream, 7) + 8:_record_at(stream, 7) + 12] = (10).to_bytes(4, "little")
    with pytest.raises(ValueError, match="k=10"):
        codec.decompress_image(model, bytes(forged))
    with pytest.raises(ValueError, match="k=10"):
        codec.decompress_region(model, bytes(forged), 64, 192, 1, 1)


# ---- region decode and the reader -------------------------------------------------------------------------------------
class Counting:
    def __init__(self, data):
        self.f, self.count = io.BytesIO(data), 0

    def seek(self, *a):
        return self.f.seek(*a)

    def tell(self):
        return self.f.tell()

    def read(self, n=-1):
        out = self.f.read(n)
        self.count += len(out)
        return out


WINDOWS = [(10, 70, 20, 30), (60, 60, 10, 10), (149, 199, 1, 1)]      # inside one tile, across four, the last pixel


@pytest.mark.parametrize("batch", [1, 64])
def test_region_decode_is_the_crop(batch):
    model, _, _, _ = _scene("main", 150, 200, 64, 5)
    stream, full = _near("main", 150, 200, 64, 5, 0)
    full = _np(full)
    for (y0, x0, h, w), ntiles in zip(WINDOWS, (1, 4, 1)):
        want = full[y0:y0 + h, x0:x0 + w]
        stats = {}
        f = Counting(stream)
        got = codec.decompress_region(model, f, y0, x0, h, w, batch=batch, stats=stats)
        assert got.dtype == torch.uint16 and (_np(got) == want).all(), (y0, x0, h, w)
        assert len(stats["tiles"]) == ntiles
        assert f.count == stats["bytes_read"] < len(stream)
        ix = codec.stream_index(stream)
        assert stats["bytes_read"] == ix["index_bytes"] + sum(n for _, n in codec.tile_spans(ix, stats["tiles"]))


def test_the_reader_equals_the_region_decode_and_caches_q():
    model, _, _, _ = _scene("main", 150, 200, 64, 5)
    stream, full = _near("main", 150, 200, 64, 5, 3)
    full = _np(full)
    with codec.ImageReader(model, stream) as reader:
        for y0, x0, h, w in WINDOWS + [(0, 0, 150, 200)]:
            got = reader.read(y0, x0, h, w)
            assert (_np(got) == _np(codec.decompress_region(model, stream, y0, x0, h, w))).all()
            assert (_np(got) == full[y0:y0 + h, x0:x0 + w]).all()
        st = {}
        again = reader.read(60, 60, 10, 10, stats=st)
        assert st["decoded"] == 0 and st["hits"] == 4 and st["decode_batches"] == 0
        assert (_np(again) == full[60:70, 60:70]).all()
        small = reader.read(0, 0, 150, 200, size=(75, 100))
        assert small.dtype == torch.uint16 and tuple(small.shape) == (75, 100, 3)


# ---- the kernels on their own ---------------------------------------------------------------------------------------
TH, TW, NT = 32, 48, 2
KH, KW = 40, 40                                                        # padded to 48 x 48: two tiles of 32 x 48
OWN = [(0, 32, 0, 40), (16, 24, 0, 40)]                                # tile 1 starts at row 16 and owns rows 32 .. 39
SCALES = [(0, 65535), (0, 10000), (5, 5), (123, 40000)]
GUARD = 64


def _guarded(shape, dtype, fill, inner=None):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    mid = buf[GUARD:GUARD + n].view(shape)
    if inner is not None:
        mid.fill_(inner)
    return buf, mid


def _guards_intact(buf, fill):
    ends = torch.cat([buf[:GUARD], buf[-GUARD:]])
    return bool(torch.isnan(ends).all()) if isinstance(fill, float) else bool((ends == fill).all())


def _kernel_scene(C, seed):
    """img uint16 [40][40][C] and x_hat float32 [2][C][32][48]: predictions at and beside the rounding points, below 0
    and above 1, half the pixels close to the prediction, and r = +65535 and -65535 where the scale allows."""
    rng = np.random.default_rng(seed)
    scale = SCALES[:C]
    x_hat = rng.uniform(-0.1, 1.1, size=(NT, C, TH, TW)).astype(np.float32)
    edge = np.float32([-0.5, -1e-30, -0.0, 0.0, 0.5, 0.49999997, 0.50000006, 1.0, 1.0000001, 2.0, 1e30, -1e30, np.nan])
    for t in range(NT):
        for c in range(C):
            plane = x_hat[t, c].reshape(-1)
            plane[rng.permutation(plane.size)[:edge.size]] = edge
    x_hat[0, :, 6, 8], x_hat[0, :, 7, 9] = -0.25, 1.5
    x_hat[1, :, 17, 8], x_hat[1, :, 18, 9] = -0.25, 1.5
    img = rng.integers(0, 65536, size=(KH, KW, C)).astype(np.int64)
    g = codec._grid(KH, KW, TH, TW)
    assert g["n"] == NT and g["ys"] == [0, 16] and [codec._owned_in_tile(g, t) for t in range(NT)] == OWN
    p = R.predictor(x_hat, scale)
    near = rng.random((KH, KW, C)) < 0.5
    for t, (y0, y1, x0, x1) in enumerate(OWN):
        oy = g["ys"][t]
        pt = np.transpose(p[t][:, y0:y1, x0:x1], (1, 2, 0))
        sel = near[oy + y0:oy + y1, x0:x1]
        img[oy + y0:oy + y1, x0:x1] = np.where(sel, np.clip(pt + rng.integers(-300, 301, size=pt.shape), 0, 65535),
                                               img[oy + y0:oy + y1, x0:x1])
    img[6, 8], img[7, 9] = 65535, 0                                    # r = +(65535 - lo) and -hi
    img[33, 8], img[34, 9] = 65535, 0
    return img.astype(np.uint16), x_hat, scale, g


def _want_q(img, x_hat, scale, g, tau):
    p = R.predictor(x_hat, scale)
    out = np.zeros(x_hat.shape, dtype=np.int64)
    for t, (y0, y1, x0, x1) in enumerate(OWN):
        oy = g["ys"][t]
        x = np.transpose(img[oy + y0:oy + y1, x0:x1].astype(np.int64), (2, 0, 1))
        out[t][:, y0:y1, x0:x1] = R.quantize(x, p[t][:, y0:y1, x0:x1], tau)
    return out


@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("tau", [0, 2, 1000, 32767])
def test_quantize_against_numpy(C, tau):
    """the image is a slice that starts at an odd uint16 offset of its buffer"""
    L = lib.load()
    img, x_hat, scale, g = _kernel_scene(C, 7 * C + tau)
    want = _want_q(img, x_hat, scale, g, tau)
    if tau == 0:
        assert want.max() == 65535 and want.min() == -65535            # band 0 spans the whole range
    held = _dev(np.concatenate([[9], img.ravel(), [9] * 7]).astype(np.uint16))
    d_img = held[1:1 + img.size].view(KH, KW, C)
    assert d_img.data_ptr() % 4 == 2
    qbuf, q = _guarded((NT, C, TH, TW), torch.int32, -7)
    mbuf, maxabs = _guarded((NT,), torch.int32, -7, inner=0)
    d_h, d_h1 = _dev(x_hat), _dev(x_hat[1:])
    lib.check(L.dsic_residual_quantize_u16(_p(d_img), _p(d_h), KH, KW, C, TH, TW, _lohi(*scale), tau, 0, NT,
                                           _p(q), _p(maxabs), _stream()), "residual_quantize_u16")
    assert (q.cpu().numpy() == want).all()
    assert maxabs.cpu().tolist() == [int(np.abs(want[t]).max()) for t in range(NT)]
    assert (want[1][:, :16] == 0).all() and (want[:, :, :, 40:] == 0).all()
    assert _guards_intact(qbuf, -7) and _guards_intact(mbuf, -7)
    # one tile of the grid alone: first_tile = 1
    q1 = torch.empty((1, C, TH, TW), dtype=torch.int32, device="cuda")
    m1 = torch.zeros(1, dtype=torch.int32, device="cuda")
    lib.check(L.dsic_residual_quantize_u16(_p(d_img), _p(d_h1), KH, KW, C, TH, TW, _lohi(*scale), tau, 1, 1,
                                           _p(q1), _p(m1), _stream()), "residual_quantize_u16")
    assert (q1.cpu().numpy()[0] == want[1]).all()


def _edge_q(C, m, sign, seed, NT=NT):
    """q int64 [NT][C][32][48]: an even tile random in [-m, m] with sign * m reached once and -sign * m never, an odd
    tile quiet inside tile 1's owned rectangle and 0 outside."""
    rng = np.random.default_rng(seed)
    q = np.zeros((NT, C, TH, TW), dtype=np.int64)
    y0, y1, x0, x1 = OWN[1]
    for t in range(NT):
        if t % 2:
            q[t][:, y0:y1, x0:x1] = rng.integers(-3, 4, size=(C, y1 - y0, x1 - x0))
            continue
        q[t] = rng.integers(-m, m + 1, size=(C, TH, TW))
        q[t][np.abs(q[t]) == m] = 0
        q[t, C - 1, 31, 47] = sign * m
        q[t, 0, :4, :8] = 0                                            # a whole wave's worth of zeros among the rest
    return q


@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("m,k", R.K_EDGES)
def test_split_tables_strings_and_block(C, m, k):
    """split on each side of every k edge (the maximum with both signs), then the tables against residual_ref.table,
    the strings against the coder oracle, and the block against the reference's pack_block"""
    _split_case(C, m, k, NT)


def test_a_block_of_more_than_256_pieces():
    """13 tiles at C = 3 are (3 + 1 + 16) * 13 = 260 pieces, so the offsets scan of dsic_residual_pack_u16's head kernel
    runs a second pass of 256 with the carry of the first; the two kinds of tile alternate."""
    _split_case(3, 511, 2, 13)


def _split_case(C, m, k, NT):
    L = lib.load()
    tau = 3
    npix, per = TH * TW, C * TH * TW
    for sign in (1, -1):
        qn = _edge_q(C, m, sign, 11 * C + m, NT)
        d_q = _dev(qn.astype(np.int32))
        d_max = _dev(np.abs(qn).reshape(NT, -1).max(axis=1).astype(np.int32))
        hbuf, hi = _guarded((NT, C, TH, TW), torch.float32, float("nan"))
        sbuf, hist = _guarded((NT, C, 512), torch.int32, -1, inner=0)
        kbuf, kk = _guarded((NT,), torch.int32, -1)
        pbuf, planes = _guarded((NT, 9, per // 64), torch.int64, -1)
        lib.check(L.dsic_residual_split_u16(_p(d_q), _p(d_max), NT, C, TH, TW, _p(hi), _p(hist), _p(kk), _p(planes),
                                            _stream()), "residual_split_u16")
        refs = [R.split(qn[t]) for t in range(NT)]
        assert [r[0] for r in refs] == ([k, 0] * NT)[:NT] == kk.cpu().tolist()
        got_planes = planes.cpu().numpy()
        for t, (kt, want_hi, want_lo) in enumerate(refs):
            assert (hi[t].cpu().numpy() == want_hi).all()
            assert (hist[t].cpu().numpy() == R.histogram(want_hi)).all()
            assert got_planes[t, :kt].tobytes() == R.planes(want_lo, kt)
            assert (got_planes[t, kt:] == -1).all()                    # only the first k planes are written
        assert all(_guards_intact(b, f) for b, f in ((hbuf, float("nan")), (sbuf, -1), (kbuf, -1), (pbuf, -1)))
    # tables (of the last sign)
    mbuf, meta = _guarded((NT, 4), torch.int32, -1)
    cbuf, compact = _guarded((NT, C, 512), torch.int16, -1)
    rbuf, coder = _guarded((NT, C * 16, 512), torch.int16, -1)
    lib.check(L.dsic_residual_tables_u16(_p(hist), NT, C, TH, TW, _p(meta), _p(compact), _p(coder), _stream()),
              "residual_tables_u16")
    got_meta = meta.cpu().numpy()
    got_compact = compact.cpu().numpy().view(np.uint16)
    got_coder = coder.cpu().numpy().view(np.uint16)
    tabs = []
    for t, (kt, want_hi, _) in enumerate(refs):
        smin, Ls = int(want_hi.min()), int(want_hi.max()) - int(want_hi.min()) + 1
        h = R.histogram(want_hi)
        tab = np.stack([R8.table(h[c, smin + 255:smin + 255 + Ls], npix) for c in range(C)])
        assert (tab == R.tile_tables(want_hi)[2]).all()
        assert tuple(got_meta[t]) == (smin, Ls, 0, 1)
        want = np.zeros((C, 512), dtype=np.int64)
        want[:, :Ls] = tab
        assert (got_compact[t] == want).all()
        assert (got_coder[t] == np.repeat(want, 16, axis=0)).all()
        tabs.append((smin, Ls, tab))
    assert _guards_intact(mbuf, -1) and _guards_intact(cbuf, -1) and _guards_intact(rbuf, -1)
    # the strings: the existing encoder, 16 segments of C band channels each
    c = residual.encode(hi, meta, coder.view(torch.uint16), 0)
    assert int(c["err"].item()) == 0
    raw, lengths = c["bytes"].cpu().numpy(), c["lengths"].cpu().numpy()
    HW = TH // 16 * TW
    tiles_ref = []
    for t, (smin, Ls, tab) in enumerate(tabs):
        sym = (refs[t][1] - smin).reshape(C * 16, HW)
        rows = np.repeat(tab, 16, axis=0).astype(np.uint16)
        strings = []
        for j in range(16):
            want_s = E.range_encode(sym[j * C:(j + 1) * C], rows[j * C:(j + 1) * C], HW)
            a = c["cap_z"] + j * c["cap_seg"]
            assert raw[t, a:a + lengths[t, 1 + j]].tobytes() == want_s, (t, j)
            strings.append(want_s)
        tiles_ref.append((smin, tab, refs[t][0], R.planes(refs[t][2], refs[t][0]), strings))
    # the block
    out, nbytes, code = residual16.pack_on_device(c, meta, kk, compact.view(torch.uint16), planes, C, TH, TW, tau)
    assert code == 0
    block = out[:nbytes].cpu().numpy().tobytes()
    assert block == R.pack_block(C, TH, TW, tau, tiles_ref)
    recs = residual16.read_block_head(lambda off, n: block[off:off + n], 0, len(block), NT, C, TH, TW, tau)
    assert [(r["r_smin"], r["r_L"], r["r_k"]) for r in recs] == [(s, l, r[0]) for (s, l, _), r in zip(tabs, refs)]


@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("tau", [0, 3])
def test_join_against_numpy(C, tau):
    """planes read in place at odd byte offsets; an over-range record (hi = +-255, k = 9, lo = 511) is clamped to
    +-Q16; a tile whose planes would leave the uploaded bytes joins with lo = 0"""
    L = lib.load()
    rng = np.random.default_rng(C + tau)
    per = C * TH * TW
    pb = per // 8
    ks = [5, 9, 1]
    n = len(ks)
    hi = rng.integers(-255, 256, size=(n, C, TH, TW))
    lo = [rng.integers(0, 1 << k, size=(C, TH, TW)) for k in ks]
    hi[1, 0, 0, :4], lo[1][0, 0, :4] = [255, -255, 255, -255], [511, 0, 0, 511]
    parts, offs, pos = [], [], 0
    for t in range(2):
        pad = bytes(rng.integers(0, 256, size=3 + 2 * t, dtype=np.uint8))
        parts += [pad, R.planes(lo[t], ks[t])]
        offs.append(pos + len(pad))
        pos += len(pad) + ks[t] * pb
    total = pos
    offs.append(total - 1)                                             # tile 2: its one plane would end past the bytes
    blob = torch.zeros((total + 31) // 16 * 16, dtype=torch.uint8, device="cuda")
    blob[:total] = _dev(np.frombuffer(b"".join(parts), dtype=np.uint8))
    d_off, d_k = _dev(np.array(offs, dtype=np.int64)), _dev(np.array(ks, dtype=np.int32))
    qbuf, q = _guarded((n, C, TH, TW), torch.float32, float("nan"))
    d_hi = _dev(hi.astype(np.float32))
    lib.check(L.dsic_residual_join_u16(_p(d_hi), _p(blob), total, _p(d_off), _p(d_k), n, C, TH,
                                       TW, tau, _p(q), _stream()), "residual_join_u16")
    got = q.cpu().numpy()
    Q16 = R.q16_max(tau)
    for t in range(2):
        assert (got[t] == R.join(hi[t], lo[t], ks[t], tau)).all()
    assert got[1, 0, 0, :4].tolist() == [Q16, -Q16, min(Q16, 255 * 512), -min(Q16, 255 * 512 - 511)]
    assert (got[2] == R.join(hi[2], 0, 1, tau)).all()
    assert _guards_intact(qbuf, float("nan"))


@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("tau", [0, 3, 32767])
def test_stitch_window_res_against_numpy(C, tau):
    """40 x 48 in tiles of 32 x 48: two tiles, the second shifted inward; windows at an odd 2-byte alignment"""
    L = lib.load()
    H, W = 40, 48
    g = codec._grid(H, W, TH, TW)
    assert g["n"] == NT and g["ys"] == [0, 16]
    rng = np.random.default_rng(C + tau)
    scale = SCALES[:C]
    x_hat = rng.uniform(-0.2, 1.2, size=(NT, C, TH, TW)).astype(np.float32)
    Q16 = R.q16_max(tau)
    q = rng.integers(-Q16, Q16 + 1, size=(NT, C, TH, TW))
    q[0, :, 0, :2] = [[Q16, -Q16]] * C
    full = np.zeros((H, W, C), dtype=np.int64)
    for t in range(NT):
        (a, b) = g["own_y"][t]
        b, oy = min(b, H), g["ys"][t]
        rec = R.reconstruct(R.predictor(x_hat[t], scale), q[t], tau)
        full[a:b] = np.transpose(rec[:, a - oy:b - oy], (1, 2, 0))
    d_h, d_q = _dev(x_hat), _dev(q.astype(np.float32))
    ids = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    for y0, x0, h, w in ((0, 0, H, W), (5, 3, 33, 41), (31, 47, 2, 1)):
        host = np.full(h * w * C + 2 * 63, 0xABCD, dtype=np.uint16)
        host[63:63 + h * w * C] = 7
        held = _dev(host)
        out = held[63:63 + h * w * C].view(h, w, C)
        assert out.data_ptr() % 4 == 2
        lib.check(L.dsic_tile_stitch_window_u16_res(_p(d_h), _p(d_q), tau, _p(ids), NT, _p(out), H, W, C, TH, TW, y0,
                                                    x0, h, w, _lohi(*scale), _stream()), "tile_stitch_window_u16_res")
        back = _np(held)
        assert (back[63:63 + h * w * C].reshape(h, w, C) == full[y0:y0 + h, x0:x0 + w]).all(), (y0, x0, h, w)
        assert (back[:63] == 0xABCD).all() and (back[-63:] == 0xABCD).all()


def test_the_exports_refuse_bad_arguments():
    check_argument_refusals()


def test_command_line_round_trip(tmp_path, capsys):
    """compress --tolerance T and decompress through tools/dsic_image.py, run in this process"""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("_dsic_image_tool", os.path.join(root, "tools", "dsic_image.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    model, img, _, _ = _scene("main", 150, 200, 64, 5)
    stream, full = _near("main", 150, 200, 64, 5, 3)
    sd = S.make_state_dict(seed=1, N=128, M=192, in_ch=3, spatial_params=False)
    torch.save({"model": {k: torch.from_numpy(v) for k, v in sd.items()}}, tmp_path / "ckpt.pt")
    np.save(tmp_path / "in.npy", img)
    w = ["--weights", str(tmp_path / "ckpt.pt")]
    tool.main(["compress", str(tmp_path / "in.npy"), str(tmp_path / "s.dsic"), "--tile", "64", "--batch", "5",
               "--tolerance", "3"] + w)
    assert "tolerance 3" in capsys.readouterr().out
    assert (tmp_path / "s.dsic").read_bytes() == stream
    tool.main(["decompress", str(tmp_path / "s.dsic"), str(tmp_path / "out.npy")] + w)
    out = np.load(tmp_path / "out.npy")
    assert out.dtype == np.uint16 and np.array_equal(out, _np(full))
    np.save(tmp_path / "in8.npy", (img >> 8).astype(np.uint8))
    with pytest.raises(ValueError, match="use max_error"):
        tool.main(["compress", str(tmp_path / "in8.npy"), str(tmp_path / "x.dsic"), "--tolerance", "3"] + w)
