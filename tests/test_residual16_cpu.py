"""Bounded-error mode for uint16 imagery without a GPU: the arithmetic of tests/residual16_ref.py holds the bound, the
split and the bit planes round-trip at every edge of the shift, the package's pure-Python writers and readers of the
wide residual block and of stream version 9 agree with the restatement byte for byte, and every refusal of the readers,
of compress_image and of the new exports is raised where it should be."""
import ctypes
import io
import os
import random
import re
import struct

import numpy as np
import pytest
import torch

import residual16_ref as R
from dsic_amd import codec, entropy, lib, residual16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAG = 0x40302
N, M = 128, 192
TAUS = [0, 1, 7, 127, 1000, 32767]


# ---- the arithmetic ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau", TAUS)
def test_the_reference_holds_the_bound(tau):
    rng = np.random.default_rng(tau)
    corners = np.array([0, 1, 2, 32767, 32768, 65534, 65535], dtype=np.int64)
    x = np.concatenate([np.repeat(corners, corners.size), rng.integers(0, 65536, 20000)])
    p = np.concatenate([np.tile(corners, corners.size), rng.integers(0, 65536, 20000)])
    q = R.quantize(x, p, tau)
    assert np.abs(q).max() <= R.q16_max(tau) == residual16.q16_max(tau)
    got = R.reconstruct(p, q, tau)
    assert np.abs(got - x).max() <= tau
    if tau == 0:
        assert (got == x).all()
    assert np.abs(p + q * (2 * tau + 1)).max() < 2 ** 31               # the decoder's sum stays inside int32
    # x outside the scale: the predictor stays inside [lo, hi], the residual carries the rest
    x_hat = rng.uniform(-0.2, 1.2, size=(2, 8, 8)).astype(np.float32)
    x_hat[0, 0, :4] = [np.nan, -0.0, 1.0, 2.0]
    pp = R.predictor(x_hat, [(2000, 6000), (7, 7)])
    assert pp[0].min() >= 2000 and pp[0].max() <= 6000 and (pp[1] == 7).all() and pp[0, 0, 0] == 2000
    xx = rng.integers(0, 65536, size=pp.shape)
    assert np.abs(R.reconstruct(pp, R.quantize(xx, pp, tau), tau) - xx).max() <= tau


def test_the_predictor_is_the_uint16_stitch_rounding():
    import u16_ref
    x_hat = np.random.default_rng(1).uniform(-0.1, 1.1, size=(3, 16, 16)).astype(np.float32)
    scale = [(0, 10000), (123, 65535), (5, 5)]
    assert (np.transpose(R.predictor(x_hat, scale), (1, 2, 0)) == u16_ref.denorm_image(x_hat, scale)).all()


@pytest.mark.parametrize("m,k", R.K_EDGES)
def test_split_and_join_round_trip_at_every_edge_of_the_shift(m, k):
    assert R.shift_for(m) == k == residual16.shift_for(m)
    rng = np.random.default_rng(m)
    for sign in (1, -1):
        q = rng.integers(-m, m + 1, size=(2, 8, 16))
        q[0, 0, 0], q[1, 7, 15] = sign * m, -sign * (m // 2)
        if sign * m != -m:
            q[q == -m] = 0                                             # only the chosen sign reaches the maximum
        else:
            q[q == m] = 0
        kk, hi, lo = R.split(q)
        assert kk == k and np.abs(hi).max() <= 255 and lo.min() >= 0 and lo.max() < 2 ** k
        assert (R.join(hi, lo, k) == q).all()
        buf = R.planes(lo, k)
        assert len(buf) == k * q.size // 8
        assert (R.unpack_planes(buf, k, q.size).reshape(q.shape) == lo).all()
    assert R.shift_for(0) == 0 and R.shift_for(65535) == 9 and R.shift_for(R.q16_max(0)) == 9


def test_plane_packing_is_packbits_of_the_definition():
    rng = np.random.default_rng(3)
    lo = rng.integers(0, 8, size=(2, 4, 16))
    assert R.planes(lo, 3) == R.planes_by_definition(lo, 3)
    flat = lo.ravel()
    word = int.from_bytes(R.planes(lo, 3)[:8], "little")              # the 64-bit ballot of samples 0 .. 63, plane 0
    assert [(word >> i) & 1 for i in range(64)] == [int(v) & 1 for v in flat[:64]]
    assert R.planes(lo, 0) == b""


# ---- the block and the version-9 stream --------------------------------------------------------------------------------
def _tile(rng, C, th, tw, k, L=None):
    """One made-up tile: (smin, tables [C][L], k, planes, 16 strings)."""
    L = rng.choice([1, 2, 17, 511]) if L is None else L
    smin = rng.randint(-255, 255 - (L - 1))
    tabs = np.stack([np.sort(np.random.default_rng(rng.getrandbits(32)).choice(np.arange(1, 60000), L - 1,
                                                                              replace=False)) for _ in range(C)])
    tabs = np.concatenate([np.zeros((C, 1), dtype=np.int64), tabs], axis=1)
    planes = bytes(rng.getrandbits(8) for _ in range(k * C * th * tw // 8))
    strings = [bytes(rng.getrandbits(8) for _ in range(rng.choice([0, 1, 9, 40]))) for _ in range(16)]
    return smin, tabs, k, planes, strings


def _build(H=100, W=150, C=3, tile=64, batch=4, tau=5, scale=((0, 10000), (5, 5), (123, 65535)), seed=0, **extra):
    """A version-9 stream in pure Python, with made-up strings, tables and planes."""
    rng = random.Random(seed)
    g = codec.tile_grid(H, W, tile)
    blobs, residuals, tiles = [], [], []
    for first in range(0, g["n"], batch):
        B = min(batch, g["n"] - first)
        comp = {"strings": [], "shape_y": [B, M, g["th"] // 16, g["tw"] // 16],
                "shape_z": [B, N, g["th"] // 64, g["tw"] // 64], "min_y": [-3] * B, "max_y": [4] * B,
                "min_z": [-2] * B, "max_z": [2] * B, "numerics": TAG}
        for _ in range(B):
            comp["strings"].append([bytes(rng.getrandbits(8) for _ in range(rng.choice([0, 3, 17]))),
                                    bytes(rng.getrandbits(8) for _ in range(rng.choice([1, 16, 50])))])
        blobs.append(entropy.pack_container(comp))
        batch_tiles = [_tile(rng, C, g["th"], g["tw"], rng.choice([0, 1, 3, 9])) for _ in range(B)]
        tiles += batch_tiles
        residuals.append(R.pack_block(C, g["th"], g["tw"], tau, batch_tiles))
    header = {"numerics": TAG, "H": H, "W": W, "C": C, "kind": 2, "th": g["th"], "tw": g["tw"], "N": N, "M": M,
              "in_ch": C, "spatial_params": 0, "batch": batch, "scale": [tuple(p) for p in scale], "tolerance": tau,
              **extra}
    return codec.pack_image_stream(header, blobs, residuals), header, blobs, residuals, tiles


def test_pack_block_equals_the_reference():
    rng = random.Random(5)
    tiles = [_tile(rng, 3, 32, 48, k) for k in (0, 2, 9)]
    block = residual16.pack_block(3, 32, 48, 7, tiles)
    assert block == R.pack_block(3, 32, 48, 7, tiles)
    assert block[:6] == b"DSICW\0" and residual16.head_bytes(3) == 30 + 3 * (16 + 64)
    recs = residual16.read_block_head(lambda o, c: block[o:o + c], 0, len(block), 3, 3, 32, 48, 7)
    pos = residual16.head_bytes(3)
    for r, (smin, tabs, k, planes, strings) in zip(recs, tiles):
        assert (r["r_smin"], r["r_L"], r["r_k"], r["r_segs"]) == (smin, tabs.shape[1], k, [len(s) for s in strings])
        assert r["r_off"] == pos and block[pos:pos + r["r_len"]] == tabs.astype("<u2").tobytes() + planes + b"".join(strings)
        residual16.check_tables(block[pos:pos + 2 * 3 * r["r_L"]], 3, r["r_L"])
        pos += r["r_len"]
    assert pos == len(block)
    with pytest.raises(ValueError, match="planes"):
        residual16.pack_block(3, 32, 48, 7, [tiles[1][:3] + (b"",) + tiles[1][4:]])


def test_the_version_9_stream_round_trips():
    stream, header, blobs, residuals, tiles = _build()
    assert codec.VERSION_TOL == 9
    assert stream == R.pack_stream_v9(header, blobs, residuals)
    u = codec.unpack_image_stream(stream)
    assert (u["version"], u["kind"], u["tolerance"], u["overlap"], u["segments"]) == (9, 2, 5, 0, 1)
    assert u["scale"] == header["scale"] and u["blobs"] == blobs and u["residuals"] == residuals
    assert "max_error" not in u and "fill" not in u
    assert codec.pack_image_stream(u, u["blobs"], u["residuals"]) == stream
    ix = codec.stream_index(stream)
    assert ix["tolerance"] == 5 and ix["scale"] == header["scale"] and ix["grid"]["n"] == len(tiles) == 6
    pb = 3 * 64 * 64 // 8
    for r, (smin, tabs, k, planes, strings) in zip(ix["tiles"], tiles):
        assert (r["r_smin"], r["r_L"], r["r_k"], r["r_segs"]) == (smin, tabs.shape[1], k, [len(s) for s in strings])
        a = r["r_off"] + 2 * 3 * r["r_L"]
        assert stream[a:a + k * pb] == planes and r["r_len"] == 2 * 3 * r["r_L"] + k * pb + sum(r["r_segs"])
    assert codec._index_of(codec._Source(io.BytesIO(stream))) == ix
    spans = codec.tile_spans(ix, [1])
    assert sum(n for _, n in spans) == sum(ix["tiles"][1][key] for key in ("z_len", "y_len", "r_len"))
    # four bands and segments ride in the same head
    s4, h4, b4, r4, _ = _build(C=4, scale=[(0, 1)] * 4, tau=0, segments=1)
    assert codec.unpack_image_stream(s4)["tolerance"] == 0 and s4 == R.pack_stream_v9(h4, b4, r4)
    # a pyramid: level 0 bounded, level 1 the plain uint16 stream
    g1 = codec.tile_grid(50, 75, 64)
    B = g1["n"]
    v6 = dict(header, H=50, W=75, th=g1["th"], tw=g1["tw"])
    del v6["tolerance"]
    comp = {"strings": [[b"ab", b"cde"]] * B, "shape_y": [B, M, g1["th"] // 16, g1["tw"] // 16],
            "shape_z": [B, N, g1["th"] // 64, g1["tw"] // 64], "min_y": [0] * B, "max_y": [1] * B, "min_z": [0] * B,
            "max_z": [1] * B, "numerics": TAG}
    s1 = codec.pack_image_stream(v6, [entropy.pack_container(comp)])
    p = codec.pack_pyramid_stream([stream, s1])
    assert codec.stream_index(p)["tolerance"] == 5 and "tolerance" not in codec.stream_index(p, level=1)
    assert codec.stream_index(p, level=1)["version"] == 6


def _patched(stream, at, fmt, *vals):
    b = bytearray(stream)
    struct.pack_into(fmt, b, at, *vals)
    return bytes(b)


def test_every_refusal_of_the_readers():
    stream, header, blobs, residuals, tiles = _build()
    ix = codec.stream_index(stream)
    words = 68 + 8 * 3                                                  # tolerance and res_bands follow the scale

    def refuses(s, match):
        for reader in (codec.stream_index, codec.unpack_image_stream):
            with pytest.raises(ValueError, match=match):
                reader(s)

    def index_refuses(s, match):
        with pytest.raises(ValueError, match=match):
            codec.stream_index(s)

    refuses(_patched(stream, 24, "<I", 0), "version 9 with kind 0")
    refuses(_patched(stream, 24, "<I", 1), "version 9 with kind 1")
    refuses(_patched(stream, 64, "<I", 16), "version 9 with overlap=16")
    refuses(_patched(stream, words, "<I", 32768), "tolerance=32768")
    refuses(_patched(stream, words + 4, "<I", 8), "res_bands=8")
    refuses(_patched(stream, 6, "<H", 7), "version 7")
    refuses(_patched(stream, 72, "<I", 70000), "65535")
    refuses(stream + b"\0", "trailing")
    for cut in (61, 70, words + 3, words + 7, words + 12, len(stream) - 1):
        refuses(stream[:cut], "truncated")
    # the block: one forged field at a time
    b0 = ix["containers"][0]["r_offset"]
    index_refuses(_patched(stream, b0 + 4, "<B", ord("R")), "not a wide residual block")
    index_refuses(_patched(stream, b0 + 6, "<I", 3), "the stream's head says")           # n
    index_refuses(_patched(stream, b0 + 10, "<I", 4), "the stream's head says")          # C
    index_refuses(_patched(stream, b0 + 14, "<I", 32), "the stream's head says")         # th
    index_refuses(_patched(stream, b0 + 22, "<I", 6), "the stream's head says")          # tau
    index_refuses(_patched(stream, b0 + 26, "<I", 8), "8 bands")
    rec = b0 + 30                                                        # tile 0: smin, L, k, span
    smin, L, k, span = struct.unpack_from("<iIII", stream, rec)
    index_refuses(_patched(stream, rec + 8, "<I", 10), "k=10")
    index_refuses(_patched(stream, rec + 4, "<I", 0), "L=0")
    index_refuses(_patched(stream, rec + 4, "<I", 512), "L=512")
    index_refuses(_patched(stream, rec, "<i", -256), "leaves")
    index_refuses(_patched(stream, rec, "<i", 256 - L + 1), "leaves|add up")
    index_refuses(_patched(stream, rec + 12, "<I", span + 1), "add up")
    index_refuses(_patched(stream, rec + 8, "<I", (k + 1) % 10), "add up")              # another k, the old span
    index_refuses(_patched(stream, b0 + 30 + 16 * 4, "<I", len(tiles[0][4][0]) + 1), "add up")
    # a block cut short inside the stream, its length word adjusted: truncated
    r0 = residuals[0]
    for cut in (10, 29, 40, len(r0) - 1):
        bad = codec.pack_image_stream(header, blobs, [r0[:cut]] + residuals[1:])
        index_refuses(bad, "truncated|not a wide")
    index_refuses(codec.pack_image_stream(header, blobs, [r0 + b"\0"] + residuals[1:]), "oversized")
    # tables
    good = tiles[1][1].astype("<u2").tobytes()
    Lw = tiles[1][1].shape[1]
    residual16.check_tables(good, 3, Lw)
    if Lw >= 2:
        with pytest.raises(ValueError, match="strictly increasing"):
            residual16.check_tables(good[:2] + good[:2] + good[4:], 3, Lw)               # c[1] = c[0]
    with pytest.raises(ValueError, match="start at 0"):
        residual16.check_tables(b"\x01\x00" + good[2:], 3, Lw)
    with pytest.raises(ValueError, match="width"):
        residual16.check_tables(good[:-2], 3, Lw)
    # the writer
    with pytest.raises(ValueError, match="kind 2"):
        codec.pack_image_stream(dict(header, kind=0, scale=None), blobs, residuals)
    with pytest.raises(ValueError, match="tolerance together with"):
        codec.pack_image_stream(dict(header, max_error=1), blobs, residuals)
    with pytest.raises(ValueError, match="tolerance together with"):
        codec.pack_image_stream(dict(header, overlap=16), blobs, residuals)
    with pytest.raises(ValueError, match="tolerance together with"):
        codec.pack_image_stream(dict(header, fill=0), blobs, residuals, mask=b"x")
    with pytest.raises(ValueError, match="one wide residual block per container"):
        codec.pack_image_stream(header, blobs, residuals[:1])
    with pytest.raises(ValueError, match="one wide residual block per container"):
        codec.pack_image_stream(header, blobs)
    for bad in (-1, 32768, True, 1.5):
        with pytest.raises(ValueError, match="tolerance="):
            codec.pack_image_stream(dict(header, tolerance=bad), blobs, residuals)
    # without tolerance the old refusal stands
    plain = dict(header)
    del plain["tolerance"]
    with pytest.raises(ValueError, match="max_error or nodata"):
        codec.pack_image_stream(dict(plain, max_error=1), blobs, residuals=[b""] * len(blobs))


# ---- compress_image's and the decoders' argument checks ---------------------------------------------------------------
class Stub(torch.nn.Module):
    def __init__(self, in_ch=3):
        super().__init__()
        self.N, self.M = N, M
        self.g_a = torch.nn.Module()
        self.g_a.g_a = torch.nn.ModuleList([torch.nn.Conv2d(in_ch, 4, 1)])


def test_compress_image_refuses_before_it_touches_the_device():
    model, img = Stub(), torch.zeros((100, 150, 3), dtype=torch.uint16)
    with pytest.raises(ValueError, match="use max_error"):
        codec.compress_image(model, torch.zeros((100, 150, 3), dtype=torch.uint8), tile=64, tolerance=2)
    with pytest.raises(ValueError, match="use max_error"):
        codec.compress_image(model, torch.zeros((3, 100, 150)), tile=64, tolerance=2)
    with pytest.raises(ValueError, match="tolerance together with overlap"):
        codec.compress_image(model, img, tile=64, tolerance=2, overlap=16)
    with pytest.raises(ValueError, match="tolerance together with valid"):
        codec.compress_image(model, img, tile=64, tolerance=2, valid=torch.ones((100, 150), dtype=torch.bool))
    with pytest.raises(ValueError, match="tolerance together with nodata"):
        codec.compress_image(model, img, tile=64, tolerance=2, nodata=0)
    with pytest.raises(ValueError, match="tolerance together with max_error"):
        codec.compress_image(model, img, tile=64, tolerance=2, max_error=1)
    for bad in (-1, 32768, True, 1.5):
        with pytest.raises(ValueError, match="tolerance="):
            codec.compress_image(model, img, tile=64, tolerance=bad)
    assert residual16.check_tolerance(np.int64(32767), "x") == 32767 and residual16.check_tolerance(0, "x") == 0
    # what is refused today stays refused, with today's message
    with pytest.raises(ValueError, match="max_error together with a uint16 image"):
        codec.compress_image(model, img, tile=64, max_error=2)
    with pytest.raises(ValueError, match="nodata together with a uint16 image"):
        codec.compress_image(model, img, tile=64, nodata=0)


def test_the_decoders_return_uint16_only():
    stream = _build()[0]
    for out in ("u8", "f32"):
        with pytest.raises(ValueError, match="bound is on the uint16 values"):
            codec.decompress_image(Stub(), stream, out=out)
        with pytest.raises(ValueError, match="bound is on the uint16 values"):
            codec.decompress_region(Stub(), io.BytesIO(stream), 0, 0, 8, 8, out=out)


def test_the_command_line_prints_the_tolerance_and_the_shifts(tmp_path, capsys):
    import importlib.util
    spec = importlib.util.spec_from_file_location("_dsic_image_tool", os.path.join(ROOT, "tools", "dsic_image.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    stream, _, _, residuals, tiles = _build()
    (tmp_path / "s.dsic").write_bytes(stream)
    tool.main(["info", str(tmp_path / "s.dsic")])
    out = capsys.readouterr().out
    ks = [t[2] for t in tiles]
    assert f"tolerance 5, residual layer {sum(len(r) for r in residuals)} bytes" in out and "stream version 9" in out
    assert "tiles per shift k: " + ", ".join(f"k={k}: {ks.count(k)}" for k in sorted(set(ks))) in out


# ---- the exports ----------------------------------------------------------------------------------------------------------
NEW = {"dsic_residual_quantize_u16": 14, "dsic_residual_split_u16": 11, "dsic_residual_tables_u16": 9,
       "dsic_residual_pack_u16": 17, "dsic_residual_join_u16": 12, "dsic_tile_stitch_window_u16_res": 17}


def test_the_new_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "dsic_hip.h")).read()
    declared = set(re.findall(r"\b(dsic_[a-zA-Z0-9_]+)\s*\(", header))
    assert set(NEW) <= declared and set(NEW) <= set(lib.SIGNATURES)
    for name, nargs in NEW.items():
        res, args = lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs and getattr(lib.load(), name) is not None


def _lohi(*pairs):
    flat = [v for p in pairs for v in p]
    return (ctypes.c_uint32 * 8)(*(flat + [0] * (8 - len(flat))))


def check_argument_refusals():
    """Every call below is refused before a launch: null pointers, C = 5, tau = 32768, misaligned buffers."""
    L = lib.load()
    one = 16                                                             # any non-null, 16-byte aligned address
    E, err = lib.DSIC_EINVAL, L.dsic_last_error
    ok = _lohi((0, 65535), (0, 10000), (7, 7), (1, 2))

    def quantize(img=one, x_hat=one, H=64, W=64, C=3, th=32, tw=32, lohi=ok, tau=1, first=0, n=4, q=one, maxabs=one):
        return L.dsic_residual_quantize_u16(img, x_hat, H, W, C, th, tw, lohi, tau, first, n, q, maxabs, None)
    for name in ("img", "x_hat", "lohi", "q", "maxabs"):
        assert quantize(**{name: None}) == E and b"null" in err()
    assert quantize(C=5) == E and b"C=5" in err() and quantize(C=0) == E
    assert quantize(tau=32768) == E and b"tau=32768" in err() and quantize(tau=-1) == E
    assert quantize(img=one + 1) == E and b"2-byte aligned" in err()
    assert quantize(x_hat=one + 4) == E and b"16-byte" in err() and quantize(q=one + 8) == E
    assert quantize(maxabs=one + 2) == E and b"4-byte" in err()
    assert quantize(lohi=_lohi((5, 4))) == E and b"lo must not exceed hi" in err()
    assert quantize(first=2, n=8) == E and b"outside the grid" in err() and quantize(th=24) == E

    def split(q=one, maxabs=one, n=2, C=3, th=32, tw=48, hi=one, hist=one, k=one, planes=one):
        return L.dsic_residual_split_u16(q, maxabs, n, C, th, tw, hi, hist, k, planes, None)
    for name in ("q", "maxabs", "hi", "hist", "k", "planes"):
        assert split(**{name: None}) == E and b"null" in err()
    assert split(C=5) == E and b"C=5" in err() and split(n=0) == E and split(n=3001) == E and split(th=40) == E
    assert split(planes=one + 4) == E and b"8-byte" in err() and split(hi=one + 2) == E

    def tables(hist=one, n=2, C=3, th=32, tw=48, meta=one, compact=one, coder=one):
        return L.dsic_residual_tables_u16(hist, n, C, th, tw, meta, compact, coder, None)
    for name in ("hist", "meta", "compact", "coder"):
        assert tables(**{name: None}) == E and b"null" in err()
    assert tables(C=5) == E and b"C=5" in err() and tables(tw=40) == E
    assert tables(compact=one + 8) == E and b"16-byte" in err() and tables(coder=one + 2) == E

    def pack(bytes_=one, cap_z=8, cap_seg=64, lengths=one, meta=one, k=one, compact=one, planes=one, err_=None, n=2,
             C=3, th=32, tw=48, tau=1, ws=one, out=one):
        return L.dsic_residual_pack_u16(bytes_, cap_z, cap_seg, lengths, meta, k, compact, planes, err_, n, C, th, tw,
                                        tau, ws, out, None)
    for name in ("bytes_", "lengths", "meta", "k", "compact", "planes", "ws", "out"):
        assert pack(**{name: None}) == E and b"null" in err()
    assert pack(C=5) == E and b"C=5" in err() and pack(tau=32768) == E and b"tau=32768" in err()
    assert pack(cap_seg=6) == E and b"capacities" in err() and pack(bytes_=one + 2) == E and pack(planes=one + 4) == E

    def join(hi=one, blob=one, total=100, off=one, k=one, n=2, C=3, th=32, tw=48, tau=1, q=one):
        return L.dsic_residual_join_u16(hi, blob, total, off, k, n, C, th, tw, tau, q, None)
    for name in ("hi", "blob", "off", "k", "q"):
        assert join(**{name: None}) == E and b"null" in err()
    assert join(C=5) == E and b"C=5" in err() and join(tau=32768) == E and b"tau=32768" in err()
    assert join(hi=one + 4) == E and b"16-byte" in err() and join(off=one + 4) == E and join(total=-1) == E

    def stitch(tiles=one, q=one, tau=1, ids=one, n=2, out=one, H=40, W=48, C=3, th=32, tw=48, y0=0, x0=0, h=40, w=48,
               lohi=ok):
        return L.dsic_tile_stitch_window_u16_res(tiles, q, tau, ids, n, out, H, W, C, th, tw, y0, x0, h, w, lohi, None)
    for name in ("tiles", "q", "ids", "out", "lohi"):
        assert stitch(**{name: None}) == E and b"null" in err()
    assert stitch(C=5) == E and b"C=5" in err() and stitch(tau=32768) == E and b"tau=32768" in err()
    assert stitch(out=one + 1) == E and b"2-byte aligned" in err()
    assert stitch(y0=1) == E and b"outside" in err() and stitch(n=0) == E


def test_the_exports_check_their_arguments_without_a_gpu():
    check_argument_refusals()
