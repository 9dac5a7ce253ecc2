"""Near-lossless mode on the GPU: compress_image(max_error=tau) decodes to within tau of the image on every pixel
(tau = 0: the image), equals tests/residual_ref.py applied to the lossy decode, keeps the lossy containers byte for
byte, decodes by region, and its kernels equal numpy and the coder oracle element by element between guards."""
import io

import numpy as np
import pytest
import torch

import residual_ref as R
from dsic_amd import codec, lib, residual
from dsic_amd import synthetic as S
from dsic_amd.model import CompressionModel
from dsic_amd.ops import _p, _stream
from oracle import entropy_ref as E

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


def _scene_u8(seed, H, W, C=3):
    return torch.from_numpy((S.make_patches(seed, 1, H, W, C)[0] * 255.0 + 0.5).astype(np.uint8)).permute(
        1, 2, 0).contiguous()


def _scene(name, H, W, tile, batch, C=3):
    """(model, image, the lossy stream and its uint8 decode), computed once and left unchanged."""
    if name not in _SCENES:
        model = _model(C)
        u8 = _scene_u8(31, H, W, C)
        lossy = codec.compress_image(model, u8.cuda(), tile=tile, batch=batch)
        _SCENES[name] = (model, u8, lossy, codec.decompress_image(model, lossy).cpu().numpy())
    return _SCENES[name]


def _near(name, H, W, tile, batch, tau, C=3):
    key = (name, tau)
    if key not in _SCENES:
        model, u8, _, _ = _scene(name, H, W, tile, batch, C)
        stream = codec.compress_image(model, u8.cuda(), tile=tile, batch=batch, max_error=tau)
        _SCENES[key] = (stream, codec.decompress_image(model, stream))
    return _SCENES[key]


def _check_decode(name, H, W, tile, batch, tau, C=3):
    model, u8, lossy, p = _scene(name, H, W, tile, batch, C)
    stream, out = _near(name, H, W, tile, batch, tau, C)
    x = u8.numpy().astype(np.int64)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (H, W, C)
    got = out.cpu().numpy().astype(np.int64)
    err = int(np.abs(got - x).max())
    print(f"{name} tau={tau}: max |x' - x| = {err}, lossy max error {int(np.abs(p.astype(np.int64) - x).max())}, "
          f"stream {len(stream)} B (lossy {len(lossy)} B)")
    if tau == 0:
        assert torch.equal(out.cpu(), u8)
    assert err <= tau
    assert (got == R.reconstruct(p, R.quantize(x, p, tau), tau)).all()
    u, ul = codec.unpack_image_stream(stream), codec.unpack_image_stream(lossy)
    assert u["version"] == 4 and u["max_error"] == tau and ul["version"] == 1
    assert u["blobs"] == ul["blobs"]                                   # the lossy layer is untouched
    assert len(u["residuals"]) == len(u["blobs"])
    return model, u8, stream, out


# ---- end to end ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau", [0, 1, 3])
def test_end_to_end_150x200(tau):
    """150 x 200: padded to 160 x 208, 12 tiles of 64 in batches of 5, 5 and 2, reflect padding on both axes, the last
    row and column of tiles shifted inward."""
    model, u8, stream, out = _check_decode("main", 150, 200, 64, 5, tau)
    assert codec.unpack_image_stream(stream)["batches"] == 3
    f32 = codec.decompress_image(model, stream, out="f32")
    assert f32.dtype == torch.float32 and torch.equal(f32, out.permute(2, 0, 1).float() / 255)


@pytest.mark.parametrize("tau", [0, 2])
def test_one_tile_smaller_than_the_tile(tau):
    """48 x 40 under tile 64: one tile of 48 x 48, row bands of 3 rows, 8 columns of reflect padding."""
    _, _, stream, _ = _check_decode("small", 48, 40, 64, 64, tau)
    ix = codec.stream_index(stream)
    assert (ix["th"], ix["tw"], len(ix["tiles"])) == (48, 48, 1)


@pytest.mark.parametrize("tau", [0, 2])
def test_four_channels(tau):
    """in_ch = 4, 96 x 80 at tile 32: 64 band channels per tile, 9 tiles in batches of 4."""
    _check_decode("four", 96, 80, 32, 4, tau, C=4)


def test_default_path_is_unchanged():
    model, u8, lossy, _ = _scene("main", 150, 200, 64, 5)
    again = codec.compress_image(model, u8.cuda(), tile=64, batch=5, max_error=None)
    assert again == lossy and codec.unpack_image_stream(lossy)["version"] == 1


def test_run_to_run_bits():
    model, u8, _, _ = _scene("main", 150, 200, 64, 5)
    a = codec.compress_image(model, u8.cuda(), tile=64, batch=5, max_error=2)
    b = codec.compress_image(model, u8.cuda(), tile=64, batch=5, max_error=2)
    assert a == b


def test_decoder_refuses_a_forged_table():
    model, _, _, _ = _scene("main", 150, 200, 64, 5)
    stream, _ = _near("main", 150, 200, 64, 5, 1)
    r = codec.stream_index(stream)["tiles"][7]
    assert r["r_L"] >= 2
    forged = bytearray(stream)
    forged[r["r_off"] + 2:r["r_off"] + 4] = b"\x00\x00"               # c[1] = c[0] = 0
    with pytest.raises(ValueError, match="strictly increasing"):
        codec.decompress_image(model, bytes(forged))
    with pytest.raises(ValueError, match="strictly increasing"):
        codec.decompress_region(model, bytes(forged), 64, 192, 1, 1)


# ---- region decode ------------------------------------------------------------------------------------------------
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


WINDOWS = [(50, 50, 40, 90), (0, 0, 150, 200), (149, 199, 1, 1), (63, 63, 2, 2), (10, 70, 20, 30), (120, 0, 30, 200)]


@pytest.mark.parametrize("batch", [1, 64])
def test_region_decode_is_the_crop(batch):
    model, _, _, _ = _scene("main", 150, 200, 64, 5)
    stream, full = _near("main", 150, 200, 64, 5, 1)
    for y0, x0, h, w in WINDOWS:
        want = full[y0:y0 + h, x0:x0 + w]
        stats = {}
        got = codec.decompress_region(model, stream, y0, x0, h, w, batch=batch, stats=stats)
        assert torch.equal(got, want), (y0, x0, h, w)
        f = Counting(stream)
        assert torch.equal(codec.decompress_region(model, f, y0, x0, h, w, batch=batch), want), (y0, x0, h, w)
        assert f.count == stats["bytes_read"]
        if len(stats["tiles"]) == 1:
            assert stats["bytes_read"] < len(stream)
    got = codec.decompress_region(model, stream, 50, 50, 40, 90, out="f32", batch=batch)
    assert torch.equal(got, full[50:90, 50:140].permute(2, 0, 1).float() / 255)


# ---- the kernels on their own ---------------------------------------------------------------------------------------
TH, TW, NT = 32, 48, 2
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


def _adversarial(C, seed, NT=NT):
    """x uint8 [NT][32][48][C] and x_hat float32 [NT][C][32][48]: x_hat at and beside every k/255, below 0 and above 1,
    r = +255 and -255 in every tile."""
    rng = np.random.default_rng(seed)
    k = (np.arange(256, dtype=np.float32) / np.float32(255.0)).astype(np.float32)
    edge = np.concatenate([np.nextafter(k, np.float32(-1)), k, np.nextafter(k, np.float32(2)),
                           np.float32([-0.5, -1e-30, -0.0, 1.0000001, 2.0, 1e30, -1e30, 0.999999])]).astype(np.float32)
    x_hat = rng.uniform(-0.1, 1.1, size=(NT, C, TH, TW)).astype(np.float32)
    x = rng.integers(0, 256, size=(NT, TH, TW, C), dtype=np.uint8)
    near = rng.random((NT, TH, TW, C)) < 0.5                           # half the pixels close to the prediction
    for t in range(NT):
        for c in range(C):
            plane = x_hat[t, c].reshape(-1)
            plane[rng.permutation(plane.size)[:edge.size]] = edge
        x[t, 6, 8], x_hat[t, :, 6, 8] = 255, -0.25                     # r = +255 inside every owned rectangle below
        x[t, 7, 9], x_hat[t, :, 7, 9] = 0, 1.5                         # r = -255
    p = np.transpose(R.predictor(x_hat), (0, 2, 3, 1))
    x = np.where(near, np.clip(p + rng.integers(-4, 5, size=p.shape), 0, 255), x).astype(np.uint8)
    x[:, 6, 8], x[:, 7, 9] = 255, 0
    return x, x_hat


def _flat(C, delta, NT=NT):
    """every pixel delta above its prediction: one symbol, L = 1"""
    x_hat = np.full((NT, C, TH, TW), 0.5, dtype=np.float32)
    x = np.full((NT, TH, TW, C), 127 + delta, dtype=np.uint8)
    return x, x_hat


OWN = [(0, TH, 0, TW), (3, 29, 5, 41)]                                 # tile 1: rows and columns cut on every side
CASES = [("adv", 0), ("adv", 2), ("adv", 127), ("flat", 0)]


@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("kind,tau", CASES)
def test_kernels_against_numpy_and_the_oracle(C, kind, tau):
    _kernels_case(C, kind, tau, NT)


def test_kernels_with_more_than_256_pieces_in_one_block():
    """14 tiles at C = 3 are (3 + 16) * 14 = 266 pieces, so the offsets scan of dsic_residual_pack's head kernel runs a
    second pass of 256 with the carry of the first; the two owned rectangles repeat."""
    _kernels_case(3, "adv", 2, 14)


def _kernels_case(C, kind, tau, NT):
    L = lib.load()
    x, x_hat = _adversarial(C, 7 * C + tau, NT) if kind == "adv" else _flat(C, 3, NT)
    own = (OWN if kind == "adv" else [OWN[0], OWN[0]]) * (NT // 2)
    Q, Lmax, npix = R.q_max(tau), R.lmax(tau), TH * TW
    want_q = np.stack([R.tile_q(x[t], x_hat[t], own[t], tau) for t in range(NT)])
    want_hist = np.stack([R.histogram(want_q[t], tau) for t in range(NT)])
    assert (want_hist.sum(axis=2) == npix).all()
    if kind == "adv":
        assert (want_q[1][:, :3] == 0).all() and (want_q[1][:, :, 41:] == 0).all()
        assert want_q.min() == -Q and want_q.max() == Q                # tau = 0: L = 511
    # quantize
    d_x, d_h = torch.from_numpy(x).cuda(), torch.from_numpy(x_hat).cuda()
    d_own = torch.tensor(own, dtype=torch.int32, device="cuda")
    qbuf, q = _guarded((NT, C, TH, TW), torch.float32, float("nan"))
    hbuf, hist = _guarded((NT, C, 512), torch.int32, -1, inner=0)
    lib.check(L.dsic_residual_quantize_u8(_p(d_x), _p(d_h), _p(d_own), NT, C, TH, TW, tau, _p(q), _p(hist),
                                          _stream()), "residual_quantize_u8")
    assert (q.cpu().numpy() == want_q).all()
    assert (hist.cpu().numpy() == want_hist).all()
    assert _guards_intact(qbuf, float("nan")) and _guards_intact(hbuf, -1)
    # tables
    mbuf, meta = _guarded((NT, 4), torch.int32, -1)
    cbuf, compact = _guarded((NT, C, Lmax), torch.int16, -1)
    rbuf, coder = _guarded((NT, C * 16, Lmax), torch.int16, -1)
    lib.check(L.dsic_residual_tables(_p(hist), NT, C, TH, TW, tau, Lmax, _p(meta), _p(compact), _p(coder), _stream()),
              "residual_tables")
    got_meta = meta.cpu().numpy()
    got_compact = compact.cpu().numpy().view(np.uint16)
    got_coder = coder.cpu().numpy().view(np.uint16)
    refs = [R.tile_tables(want_q[t], tau) for t in range(NT)]
    for t, (smin, Ls, tabs) in enumerate(refs):
        assert tuple(got_meta[t]) == (smin, Ls, 0, 1)
        if kind == "flat":
            assert (smin, Ls) == (3 // (2 * tau + 1) if tau else 3, 1)
        if kind == "adv" and tau == 0:
            assert Ls == 511
        want = np.zeros((C, Lmax), dtype=np.int64)
        want[:, :Ls] = tabs
        assert (got_compact[t] == want).all()
        assert (got_coder[t] == np.repeat(want, 16, axis=0)).all()
    assert _guards_intact(mbuf, -1) and _guards_intact(cbuf, -1) and _guards_intact(rbuf, -1)
    # the strings: the existing encoder, 16 segments of C band channels each
    c = residual.encode(q, meta, coder.view(torch.uint16), tau)
    assert int(c["err"].item()) == 0
    raw, lengths = c["bytes"].cpu().numpy(), c["lengths"].cpu().numpy()
    HW = TH // 16 * TW
    tiles_ref = []
    for t, (smin, Ls, tabs) in enumerate(refs):
        sym = (want_q[t] - smin).reshape(C * 16, HW)
        rows = np.repeat(tabs, 16, axis=0).astype(np.uint16)
        strings = []
        for k in range(16):
            want_s = E.range_encode(sym[k * C:(k + 1) * C], rows[k * C:(k + 1) * C], HW)
            a = c["cap_z"] + k * c["cap_seg"]
            got_s = raw[t, a:a + lengths[t, 1 + k]].tobytes()
            assert got_s == want_s, (t, k)
            assert (E.range_decode(got_s, C * HW, rows[k * C:(k + 1) * C], HW).reshape(C, HW)
                    == sym[k * C:(k + 1) * C]).all()
            strings.append(want_s)
        tiles_ref.append((smin, tabs, strings))
    # the block
    out, nbytes, code = residual.pack_on_device(c, meta, compact.view(torch.uint16), C, TH, TW, tau)
    assert code == 0
    block = out[:nbytes].cpu().numpy().tobytes()
    assert block == R.pack_block(C, TH, TW, tau, tiles_ref)
    assert [(r["r_smin"], r["r_L"]) for r in residual.read_block_head(
        lambda off, n: block[off:off + n], 0, len(block), NT, C, TH, TW, tau)] == [(s, l) for s, l, _ in refs]


@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("tau", [0, 3])
def test_stitch_window_res_against_numpy(C, tau):
    """40 x 48 in tiles of 32 x 48: two tiles, the second shifted inward; an unaligned window across the seam."""
    L = lib.load()
    H, W = 40, 48
    g = codec._grid(H, W, TH, TW)
    assert g["n"] == NT and g["ys"] == [0, 16]
    rng = np.random.default_rng(C + tau)
    x_hat = rng.uniform(-0.2, 1.2, size=(NT, C, TH, TW)).astype(np.float32)
    Q = R.q_max(tau)
    q = rng.integers(-Q, Q + 1, size=(NT, C, TH, TW)).astype(np.float32)
    full = np.zeros((H, W, C), dtype=np.int64)
    for t in range(NT):
        (a, b) = g["own_y"][t]
        b, oy = min(b, H), g["ys"][t]
        rec = R.reconstruct(R.predictor(x_hat[t]), q[t].astype(np.int64), tau)          # [C][th][tw]
        full[a:b] = np.transpose(rec[:, a - oy:b - oy], (1, 2, 0))
    d_h, d_q = torch.from_numpy(x_hat).cuda(), torch.from_numpy(q).cuda()
    ids = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    for y0, x0, h, w in ((0, 0, H, W), (5, 3, 33, 41), (31, 47, 2, 1)):
        buf, out = _guarded((h, w, C), torch.uint8, 255, inner=7)
        lib.check(L.dsic_tile_stitch_window_u8_res(_p(d_h), _p(d_q), tau, _p(ids), NT, _p(out), H, W, C, TH, TW, y0, x0,
                                                   h, w, _stream()), "tile_stitch_window_u8_res")
        assert (out.cpu().numpy() == full[y0:y0 + h, x0:x0 + w]).all(), (y0, x0, h, w)
        assert _guards_intact(buf, 255)
