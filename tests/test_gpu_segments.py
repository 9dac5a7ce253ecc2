"""Segmented range coding on the GPU: a tile's y string as K independent strings, one per group of M / K channels.
Every segment is the oracle's string for its channels, the z strings and the decoded latents are those of K = 1,
and containers, image streams and region decodes carry the segments through."""
import struct

import numpy as np
import pytest
import torch

from dsic_amd import codec, entropy
from dsic_amd import synthetic as S
from dsic_amd.model import CompressionModel
from oracle import entropy_ref as E

pytestmark = pytest.mark.gpu
KS = [2, 4, 8, 16]
SHAPES = {"64": (3, 64, 64), "256": (4, 256, 256)}
_CACHE = {}


def _model(spatial=False):
    key = ("model", spatial)
    if key not in _CACHE:
        sd = S.make_state_dict(seed=4 if spatial else 1, spatial_params=spatial)
        m = CompressionModel(N=128, M=192, spatial_params=spatial, min_nu=2, max_nu=100.0)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        _CACHE[key] = m.cuda().eval()
    return _CACHE[key]


def _case(shape):
    """The forward pass of one batch, the K = 1 coder output and the oracle's symbols and tables per image."""
    if shape not in _CACHE:
        B, H, W = SHAPES[shape]
        m = _model()
        x = torch.from_numpy(S.make_patches(700, B, H, W)).cuda()
        with torch.no_grad():
            out = m(x, quant_mode="round")
        args = (out["y_tilde"], out["z_tilde"], entropy._per_channel(out["sigma"]), entropy._per_channel(out["nu"]),
                entropy.sigma_z_of(m), 10, entropy.DEFAULT_LMAX)
        c1 = entropy.compress_latents(*args, split=True)
        assert int(c1["err"].item()) == 0
        y = out["y_tilde"].cpu().numpy()
        sy, ny = args[2].cpu().numpy(), args[3].cpu().numpy()
        meta = c1["meta"].cpu().numpy()
        sym = [y[b].astype(np.int32) - int(meta[b, 0]) for b in range(B)]
        tabs = [E.tables_student(sy[b], ny[b], int(meta[b, 0]), int(meta[b, 1])) for b in range(B)]
        _CACHE[shape] = {"x": x, "out": out, "args": args, "c1": c1, "sym": sym, "tabs": tabs, "meta": meta}
    return _CACHE[shape]


def _segments_of(c):
    """compress_latents' dict -> per image the list of its y segment strings (host bytes)."""
    K, raw, lens = c["segments"], c["bytes"].cpu().numpy(), c["lengths"].cpu().numpy()
    return [[raw[b, c["cap_z"] + k * c["cap_y"]:c["cap_z"] + k * c["cap_y"] + lens[b, 1 + k]].tobytes()
             for k in range(K)] for b in range(raw.shape[0])]


def _decode_segments(segs, meta, tab_y, Lmax, shape_y, per_element=0, seg_lengths=None, guard=0):
    """The segments of every image back to back -> dsic_range_decode_seg -> (y_hat, err, the whole output buffer)."""
    from dsic_amd import lib as _lib
    from dsic_amd.ops import _p, _stream
    B, M, Hy, Wy = shape_y
    K = len(segs[0])
    strings = [[b"", b"".join(s)] for s in segs]
    ybuf, ylen, ystride = entropy._upload_strings(strings, 1, "cuda")
    sl = [[len(v) for v in s] for s in segs] if seg_lengths is None else seg_lengths
    sl = torch.tensor(sl, dtype=torch.int32, device="cuda")
    n = B * M * Hy * Wy
    buf = torch.full((n + 2 * guard,), -12345.0, dtype=torch.float32, device="cuda")
    y_hat = buf[guard:guard + n]
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(_lib.load().dsic_range_decode_seg(_p(ybuf), ystride, _p(ylen), 1, 0, _p(sl), K, _p(meta), 0, _p(tab_y),
                                                 Lmax, B, M, Hy * Wy, per_element, _p(y_hat), _p(err), _stream()),
               "range_decode_seg")
    torch.cuda.synchronize()
    return y_hat.view(B, M, Hy, Wy), int(err.item()), buf


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("shape", ["64", "256"])
def test_encoder_segments_are_the_oracles_strings(shape, K):
    cs = _case(shape)
    B, H, W = SHAPES[shape]
    HW = (H // 16) * (W // 16)
    c1 = cs["c1"]
    cK = entropy.compress_latents(*cs["args"], segments=K)
    assert int(cK["err"].item()) == 0 and cK["segments"] == K
    assert torch.equal(cK["meta"], c1["meta"])
    for b in range(B):                                                     # entries past the support are never written
        Ly = int(cs["meta"][b, 1])
        assert torch.equal(cK["tab_y"][b, :, :Ly], c1["tab_y"][b, :, :Ly])
    l1, lK = c1["lengths"].cpu().numpy(), cK["lengths"].cpu().numpy()
    assert lK.shape == (B, 1 + K) and np.array_equal(lK[:, 0], l1[:, 0])
    r1, rK = c1["bytes"].cpu().numpy(), cK["bytes"].cpu().numpy()
    assert np.array_equal(rK[:, :cK["cap_z"]], r1[:, :c1["cap_z"]])          # the z strings, padding included
    got = _segments_of(cK)
    step = 192 // K
    for b in range(B):
        for k in range(K):
            rows = slice(k * step, (k + 1) * step)
            want = E.range_encode(cs["sym"][b][rows], cs["tabs"][b][rows], HW)
            assert lK[b, 1 + k] == len(want), (b, k)
            assert got[b][k] == want, (b, k)
            # and the oracle's decoder reads the GPU's segment back
            assert np.array_equal(E.range_decode(got[b][k], step * HW, cs["tabs"][b][rows], HW),
                                  cs["sym"][b][rows].ravel())
        # rate: a segment boundary costs its flush (one pending bit and the deciding bit) and the padding to a whole
        # byte, at most 9 bits; the oracle's own sweep stays under 1 byte per extra segment
        print(f"rate shape={shape} K={K} image {b}: {int(lK[b, 1:].sum())} bytes in segments, {int(l1[b, 1])} whole")
        assert int(lK[b, 1:].sum()) <= int(l1[b, 1]) + 2 * (K - 1)
    # the bytes behind every segment's end are still the zeros the caller wrote
    for b in range(B):
        for k in range(K):
            a = cK["cap_z"] + k * cK["cap_y"]
            assert not rK[b, a + lK[b, 1 + k]:a + cK["cap_y"]].any()


@pytest.mark.parametrize("case", ["model", "errors"])
def test_one_segment_is_the_unsegmented_encoder(case):
    """dsic_range_encode_seg_ws with segs = 1: the out, lengths and err of dsic_range_encode_ws, error bits included."""
    from dsic_amd import lib as _lib
    from dsic_amd.ops import _p, _stream
    L = _lib.load()
    if case == "model":
        cs = _case("64")
        y, z = cs["out"]["y_tilde"].contiguous(), cs["out"]["z_tilde"].contiguous()
        meta, tab_y, tab_z = cs["c1"]["meta"], cs["c1"]["tab_y"], cs["c1"]["tab_z"]
        B, M, HWy, N, HWz, Lmax = 3, 192, 16, 128, 1, entropy.DEFAULT_LMAX
        caps = [(entropy._cap(M * HWy), entropy._cap(N * HWz))]
    else:   # a support that misses symbols (bit 2) and capacities too small for the strings (bit 4)
        rng = np.random.default_rng(9)
        B, M, N, HWy, HWz, Lmax = 2, 4, 2, 200, 4, 64
        y = torch.from_numpy(np.rint(rng.normal(size=(B, M, HWy)) * 6).astype(np.float32)).cuda()
        z = torch.from_numpy(np.rint(rng.normal(size=(B, N, HWz)) * 2).astype(np.float32)).cuda()
        meta = torch.tensor([[-5, 11, -12, 25], [-30, 61, -12, 25]], dtype=torch.int32, device="cuda")
        sy = torch.from_numpy(rng.uniform(1.0, 8.0, (B, M)).astype(np.float32)).cuda()
        ny = torch.full((B, M), 4.0, device="cuda")
        tab_y, tab_z, _ = entropy.cdf_tables(sy, ny, torch.ones(N, device="cuda"), meta, Lmax)
        caps = [(entropy._cap(M * HWy), entropy._cap(N * HWz)), (32, 8)]
    assert L.dsic_range_encode_seg_workspace_size(B, M, HWy, N, HWz, 1) == \
        L.dsic_range_encode_workspace_size(B, M, HWy, N, HWz)
    for cap_y, cap_z in caps:
        res = []
        for seg in (True, False):
            out = torch.zeros((B, (cap_z + cap_y) // 4), dtype=torch.int32, device="cuda").view(torch.uint8)
            lengths = torch.zeros((B, 2), dtype=torch.int32, device="cuda")
            err = torch.zeros(1, dtype=torch.int32, device="cuda")
            nb = L.dsic_range_encode_workspace_size(B, M, HWy, N, HWz)
            ws = torch.empty(((nb + 3) // 4,), dtype=torch.int32, device="cuda")
            args = (_p(y), _p(z), _p(meta), _p(tab_y), _p(tab_z), Lmax, B, M, HWy, N, HWz, _p(out), cap_y, cap_z,
                    _p(lengths), _p(err), 0)
            if seg:
                _lib.check(L.dsic_range_encode_seg_ws(*args, 1, _p(ws), ws.numel() * 4, _stream()), "seg_ws")
            else:
                _lib.check(L.dsic_range_encode_ws(*args, _p(ws), ws.numel() * 4, _stream()), "ws")
            res.append((out, lengths, int(err.item())))
        assert res[0][2] == res[1][2] and torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][0], res[1][0])
        if case == "errors":
            assert res[0][2] & 2 and (cap_y != 32 or res[0][2] & 4)
        else:
            assert res[0][2] == 0 and torch.equal(res[0][0], _case("64")["c1"]["bytes"])


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("shape", ["64", "256"])
def test_decoder_reads_the_segments(shape, K):
    cs = _case(shape)
    m = _model()
    B = SHAPES[shape][0]
    d1 = entropy.custom_compress(m, cs["x"])
    dK = entropy.custom_compress(m, cs["x"], segments=K)
    assert set(d1) == {"strings", "shape_y", "shape_z", "min_y", "max_y", "min_z", "max_z", "numerics"}
    assert set(dK) == set(d1) | {"segments", "seg_lengths_y"} and dK["segments"] == K
    for key in ("shape_y", "shape_z", "min_y", "max_y", "min_z", "max_z", "numerics"):
        assert dK[key] == d1[key], key
    cK = entropy.compress_latents(*cs["args"], segments=K)
    segs = _segments_of(cK)
    for b in range(B):
        assert dK["strings"][b][0] == d1["strings"][b][0]
        assert dK["strings"][b][1] == b"".join(segs[b])
        assert dK["seg_lengths_y"][b] == [len(s) for s in segs[b]]
    x1 = entropy.custom_decompress(m, d1)
    xK = entropy.custom_decompress(m, dK)
    assert torch.equal(xK, x1) and torch.equal(xK, cs["out"]["x_hat"].clamp(0, 1))
    # the decoded latents themselves, from segments that start at any byte alignment
    y_hat, err, _ = _decode_segments(segs, cK["meta"], cK["tab_y"], entropy.DEFAULT_LMAX, cK["shape_y"])
    assert err == 0 and torch.equal(y_hat, cs["out"]["y_tilde"])
    assert len({sum(len(s) for s in row[:k]) & 3 for row in segs for k in range(K)}) > 1


def test_wide_supports_take_the_general_path():
    """Supports wider than 64 entries: the decoder walks a table row in several registers (and in 64-bit products)."""
    rng = np.random.default_rng(21)
    B, M, N, Hy, Wy = 2, 16, 4, 6, 10
    y = np.rint(rng.standard_t(3.0, size=(B, M, Hy, Wy)) * 25).clip(-150, 150).astype(np.float32)
    z = np.rint(rng.normal(size=(B, N, 2, 3)) * 3).astype(np.float32)
    sy = rng.uniform(5.0, 40.0, (B, M)).astype(np.float32)
    ny = rng.uniform(2.0, 30.0, (B, M)).astype(np.float32)
    sz = rng.uniform(0.5, 5.0, N).astype(np.float32)
    t = [torch.from_numpy(a).cuda() for a in (y, z, sy, ny, sz)]
    for K in (2, 8, 16):
        c = entropy.compress_latents(*t, tail=10, Lmax=384, segments=K)
        meta = c["meta"].cpu().numpy()
        assert int(c["err"].item()) == 0 and meta[:, 1].min() > 64
        segs = _segments_of(c)
        step = M // K
        for b in range(B):
            tab = E.tables_student(sy[b], ny[b], int(meta[b, 0]), int(meta[b, 1]))
            sym = y[b].astype(np.int32) - int(meta[b, 0])
            for k in range(K):
                rows = slice(k * step, (k + 1) * step)
                assert segs[b][k] == E.range_encode(sym[rows], tab[rows], Hy * Wy), (K, b, k)
        y_hat, err, _ = _decode_segments(segs, c["meta"], c["tab_y"], 384, c["shape_y"])
        assert err == 0 and torch.equal(y_hat, t[0])


def test_spatial_params_in_four_segments():
    """spatial_params: a table row per symbol, so a segment's rows start at its first symbol (the oracle with hw = 1)."""
    m = _model(spatial=True)
    K = 4
    x = torch.from_numpy(S.make_patches(500, 2, 128, 64)).cuda()
    with torch.no_grad():
        out = m(x, quant_mode="round")
    y = out["y_tilde"].cpu().numpy()
    sy, ny = out["sigma"].cpu().numpy(), out["nu"].cpu().numpy()
    d1 = entropy.custom_compress(m, x)
    dK = entropy.custom_compress(m, x, segments=K)
    n = y[0].size
    for b in range(2):
        assert dK["strings"][b][0] == d1["strings"][b][0]
        ymin = dK["min_y"][b]
        tab = E.tables_student(np.ravel(sy[b]), np.ravel(ny[b]), ymin, dK["max_y"][b] - ymin + 1)
        sym = y[b].astype(np.int32).ravel() - ymin
        off = 0
        for k, ln in enumerate(dK["seg_lengths_y"][b]):
            rows = slice(k * n // K, (k + 1) * n // K)
            want = E.range_encode(sym[rows], tab[rows], 1)
            assert dK["strings"][b][1][off:off + ln] == want, (b, k)
            off += ln
        assert off == len(dK["strings"][b][1])
    xK = entropy.custom_decompress(m, dK)
    assert torch.equal(xK, out["x_hat"].clamp(0, 1)) and torch.equal(xK, entropy.custom_decompress(m, d1))
    blob = entropy.compress_to_container(m, x, segments=K)
    assert blob == entropy.pack_container(dK)
    assert torch.equal(entropy.decompress_container(m, blob), xK)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("shape", ["64", "256"])
def test_device_container_equals_host_container(shape, K):
    cs = _case(shape)
    m = _model()
    comp = entropy.custom_compress(m, cs["x"], segments=K)
    want = entropy.pack_container(comp)
    got = entropy.compress_to_container(m, cs["x"], segments=K)
    assert isinstance(got, bytes) and got[:6] == b"DSIC3\x00" and got == want
    assert entropy.unpack_container(got) == comp
    dec = entropy.decompress_container(m, got)
    assert torch.equal(dec, entropy.custom_decompress(m, comp))
    assert torch.equal(dec, cs["out"]["x_hat"].clamp(0, 1))
    # one segment: today's DSIC2 bytes
    one = entropy.compress_to_container(m, cs["x"], segments=1)
    assert one == entropy.compress_to_container(m, cs["x"]) and one[:6] == b"DSIC2\x00"


def test_image_stream_and_region_decode():
    m = _model()
    H, W, K = 600, 777, 8
    img = torch.from_numpy((S.make_patches(900, 1, H, W, 3)[0] * 255.0 + 0.5).astype(np.uint8)).permute(1, 2, 0)
    img = img.contiguous()
    s1 = codec.compress_image(m, img, tile=256, batch=5)
    sK = codec.compress_image(m, img, tile=256, batch=5, segments=K)
    assert struct.unpack_from("<H", s1, 6)[0] == 1 and struct.unpack_from("<H", sK, 6)[0] == 2
    assert s1 == codec.compress_image(m, img, tile=256, batch=5, segments=1)
    full1 = codec.decompress_image(m, s1)
    fullK = codec.decompress_image(m, sK)
    assert fullK.dtype == torch.uint8 and tuple(fullK.shape) == (H, W, 3)
    assert torch.equal(fullK, full1)
    ix1, ixK = codec.stream_index(s1), codec.stream_index(sK)
    assert ixK["segments"] == K and ix1["segments"] == 1 and len(ixK["tiles"]) == len(ix1["tiles"]) == 12
    for r1, rK in zip(ix1["tiles"], ixK["tiles"]):
        assert len(rK["y_segs"]) == K and sum(rK["y_segs"]) == rK["y_len"]
        assert r1["y_segs"] == [r1["y_len"]] and rK["z_len"] == r1["z_len"]
        assert sK[rK["z_off"]:rK["z_off"] + rK["z_len"]] == s1[r1["z_off"]:r1["z_off"] + r1["z_len"]]
        assert rK["y_len"] <= r1["y_len"] + 2 * (K - 1)
    print(f"stream bytes: {len(sK)} in {K} segments, {len(s1)} whole ({len(sK) / len(s1):.5f})")
    # one window inside a single tile, one over several tiles and containers, one in the shifted last row and column
    for y0, x0, h, w in ((10, 20, 100, 120), (200, 130, 300, 500), (520, 700, 80, 77)):
        stats = {}
        got = codec.decompress_region(m, sK, y0, x0, h, w, stats=stats)
        assert torch.equal(got, fullK[y0:y0 + h, x0:x0 + w])
        assert stats["tiles"] == codec.window_tiles(ixK, y0, x0, h, w)
    assert len(codec.window_tiles(ixK, 10, 20, 100, 120)) == 1
    assert torch.equal(codec.decompress_region(m, sK, 200, 130, 300, 500, batch=4), fullK[200:500, 130:630])


def test_refusals():
    m = _model()
    cs = _case("64")
    for bad in (3, 0, 32, 6):
        with pytest.raises(ValueError):
            entropy.custom_compress(m, cs["x"], segments=bad)
        with pytest.raises(ValueError):
            entropy.compress_latents(*cs["args"], segments=bad)
    with pytest.raises(ValueError):
        codec.compress_image(m, torch.zeros((64, 64, 3), dtype=torch.uint8), segments=3)
    # 24 channels do not divide into 16 segments
    rng = np.random.default_rng(2)
    y = torch.from_numpy(np.rint(rng.normal(size=(2, 24, 4, 4)) * 3).astype(np.float32)).cuda()
    z = torch.from_numpy(np.rint(rng.normal(size=(2, 4, 1, 1))).astype(np.float32)).cuda()
    sy, ny, sz = torch.ones((2, 24), device="cuda"), torch.full((2, 24), 5.0, device="cuda"), torch.ones(4).cuda()
    with pytest.raises(ValueError):
        entropy.compress_latents(y, z, sy, ny, sz, segments=16)
    assert int(entropy.compress_latents(y, z, sy, ny, sz, segments=8)["err"].item()) == 0
    from dsic_amd import lib as _lib
    L = _lib.load()
    assert L.dsic_range_encode_seg_workspace_size(2, 24, 16, 4, 1, 16) == -1
    assert L.dsic_range_encode_seg_workspace_size(2, 24, 16, 4, 1, 3) == -1
    # segments need the split encoder
    with pytest.raises(ValueError):
        entropy.compress_latents(*cs["args"], split=False, segments=2)
    with pytest.raises(ValueError):
        entropy.compress_latents(*cs["args"], streams_per_wg=2, segments=2)
    # a container whose segment lengths do not add up is refused on the host
    blob = bytearray(entropy.compress_to_container(m, cs["x"], segments=4))
    at = 42 + 24 * 3 + 4 * 6
    struct.pack_into("<I", blob, at, struct.unpack_from("<I", blob, at)[0] + 5)
    with pytest.raises(ValueError):
        entropy.decompress_container(m, bytes(blob))
    with pytest.raises(ValueError):
        entropy.custom_decompress(m, dict(entropy.custom_compress(m, cs["x"], segments=4), segments=3))


def test_forged_segment_length_stays_inside_the_string_and_the_output():
    """The device clamps a segment's start and length to what is left of its string: an over-long entry decodes
    something for the segments behind it, raises no error bit (none is defined for it) and writes only its own
    outputs."""
    cs = _case("64")
    K = 4
    cK = entropy.compress_latents(*cs["args"], segments=K)
    segs = _segments_of(cK)
    forged = [[len(v) for v in s] for s in segs]
    forged[1][1] = 1 << 30
    guard = 4096
    y_hat, err, buf = _decode_segments(segs, cK["meta"], cK["tab_y"], entropy.DEFAULT_LMAX, cK["shape_y"],
                                       seg_lengths=forged, guard=guard)
    assert err == 0
    assert bool((buf[:guard] == -12345.0).all()) and bool((buf[-guard:] == -12345.0).all())
    want = cs["out"]["y_tilde"]
    assert torch.equal(y_hat[0], want[0]) and torch.equal(y_hat[2], want[2])
    assert torch.equal(y_hat[1, :192 // K], want[1, :192 // K])        # the segment in front of the forged one
    lo, L = int(cs["meta"][1, 0]), int(cs["meta"][1, 1])
    assert bool(((y_hat[1] >= lo) & (y_hat[1] <= lo + L - 1)).all())   # every symbol written, each inside the support
    # negative and zero lengths read zeros
    forged[1] = [-7, 0, 1 << 30, 5]
    y_hat, err, buf = _decode_segments(segs, cK["meta"], cK["tab_y"], entropy.DEFAULT_LMAX, cK["shape_y"],
                                       seg_lengths=forged, guard=guard)
    assert err == 0 and torch.equal(y_hat[0], want[0]) and torch.equal(y_hat[2], want[2])
    assert bool((buf[:guard] == -12345.0).all()) and bool((buf[-guard:] == -12345.0).all())
    assert bool(((y_hat[1] >= lo) & (y_hat[1] <= lo + L - 1)).all())
