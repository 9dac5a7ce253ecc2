"""CPU-only: the arithmetic of the near-lossless residual layer (error bound, table formula, code length), the
version-4 stream and its residual blocks in pure Python, the refusals, and the argument checks of the new exports."""
import io
import random
import struct

import numpy as np
import pytest

import residual_ref as R
from dsic_amd import codec, entropy, residual

TAG = 0x40302
N, M = 128, 192
TAUS = (0, 1, 2, 3, 7, 127)


# ---- arithmetic ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau", TAUS)
def test_error_bound_over_every_pair(tau):
    x, p = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    q = R.quantize(x, p, tau)
    assert np.abs(q).max() <= R.q_max(tau)
    xr = R.reconstruct(p, q, tau)
    assert xr.min() >= 0 and xr.max() <= 255
    assert np.abs(xr - x).max() <= tau
    if tau == 0:
        assert (xr == x).all()
    assert residual.q_max(tau) == R.q_max(tau) and residual.table_lmax(tau) == R.lmax(tau)
    assert residual.table_lmax(tau) % 8 == 0 and residual.table_lmax(tau) <= 512


def _histograms(rng, npix):
    """(name, histogram over a support) for random and degenerate cases; every one sums to npix."""
    out = [("L=1", [npix]), ("two equal", [npix // 2, npix - npix // 2]), ("one rare", [npix - 1, 1]),
           ("L=511 flat", list(np.bincount(np.arange(npix) % 511, minlength=511))),
           ("L=511 one heavy", [1] * 510 + [npix - 510]),
           ("L=511 ends only", [1] + [0] * 509 + [npix - 1]),
           ("zeros inside", [5, 0, 0, npix - 12, 0, 7])]
    for L in (2, 3, 17, 64, 200, 511):
        w = rng.dirichlet(np.full(L, 0.3))
        h = np.floor(w * (npix - 2)).astype(np.int64)
        h[0] += 1
        h[-1] += npix - int(h.sum())                                   # both ends of a support are occupied
        out.append((f"random L={L}", list(h)))
    return out


@pytest.mark.parametrize("npix", [32 * 48, 256 * 256, 48 * 48])
def test_tables_increase_and_cost_less_than_the_bound(npix):
    rng = np.random.default_rng(npix)
    for name, h in _histograms(rng, npix):
        assert sum(h) == npix and min(h) >= 0, name
        L = len(h)
        c = R.table(h, npix)
        assert c[0] == 0 and (np.diff(c) >= 1).all() and c[-1] <= 65535, name
        # every entry's width exceeds h (65536 - L) / npix, so the cost stays below H0 + log2(65536 / 65025)
        width = np.diff(np.append(c, 65536))
        assert (width * npix > np.asarray(h) * (65536 - L)).all(), name
        assert R.code_bits(h, c, npix) < R.entropy_bits(h, npix) + np.log2(65536 / 65025), name
        residual.check_tables(c.astype("<u2").tobytes(), 1, L, 0)      # the decoder's validation accepts it


def test_check_tables_refuses():
    good = np.array([[0, 5, 9], [0, 1, 2]], dtype="<u2")
    residual.check_tables(good.tobytes(), 2, 3, 7)
    for bad in ([[1, 5, 9], [0, 1, 2]], [[0, 5, 5], [0, 1, 2]], [[0, 5, 9], [0, 2, 1]]):
        with pytest.raises(ValueError, match="strictly increasing"):
            residual.check_tables(np.array(bad, dtype="<u2").tobytes(), 2, 3, 7)
    with pytest.raises(ValueError, match="width"):
        residual.check_tables(np.zeros((3, 5), dtype="<u2").tobytes(), 3, 5, 127)      # 2 Q + 1 = 3 at tau 127
    with pytest.raises(ValueError, match="width"):
        residual.check_tables(good.tobytes(), 2, 2, 7)                                  # bytes of another width


# ---- version-4 streams in pure Python -----------------------------------------------------------------------------
def _tile(rng, C, tau):
    Q = R.q_max(tau)
    L = rng.randint(1, 2 * Q + 1)
    smin = rng.randint(-Q, Q - L + 1)
    tabs = np.stack([np.sort(np.array([0] + rng.sample(range(1, 65536), L - 1))) for _ in range(C)])
    strings = [bytes(rng.getrandbits(8) for _ in range(rng.choice([0, 1, 5, 16, 33, 100]))) for _ in range(16)]
    return smin, tabs, strings


def _build(H, W, tile, batch, tau, seed=0, C=3, segments=1):
    rng = random.Random(seed)
    g = codec.tile_grid(H, W, tile)
    blobs, blocks, tiles = [], [], []
    for first in range(0, g["n"], batch):
        B = min(batch, g["n"] - first)
        comp = {"strings": [[bytes(rng.getrandbits(8) for _ in range(rng.choice([0, 3, 40]))),
                             bytes(rng.getrandbits(8) for _ in range(rng.choice([0, 16, 250])))] for _ in range(B)],
                "shape_y": [B, M, g["th"] // 16, g["tw"] // 16], "shape_z": [B, N, g["th"] // 64, g["tw"] // 64],
                "min_y": [-5] * B, "max_y": [9] * B, "min_z": [-3] * B, "max_z": [4] * B, "numerics": TAG}
        if segments > 1:
            comp["segments"] = segments
            comp["seg_lengths_y"] = [[len(s[1])] + [0] * (segments - 1) for s in comp["strings"]]
        blobs.append(entropy.pack_container(comp))
        batch_tiles = [_tile(rng, C, tau) for _ in range(B)]
        tiles += batch_tiles
        blocks.append(R.pack_block(C, g["th"], g["tw"], tau, batch_tiles))
    header = {"numerics": TAG, "H": H, "W": W, "C": C, "kind": 0, "th": g["th"], "tw": g["tw"], "N": N, "M": M,
              "in_ch": C, "spatial_params": 0, "batch": batch, "segments": segments, "max_error": tau}
    return header, blobs, blocks, tiles, g


@pytest.mark.parametrize("H,W,tile,batch,tau,segments", [(150, 200, 64, 5, 2, 1), (600, 1000, 256, 5, 0, 4),
                                                         (48, 40, 64, 64, 127, 1)])
def test_version4_pack_unpack_index_spans(H, W, tile, batch, tau, segments):
    header, blobs, blocks, tiles, g = _build(H, W, tile, batch, tau, seed=H, segments=segments)
    stream = codec.pack_image_stream(header, blobs, blocks)
    assert stream == R.pack_stream_v4(header, blobs, blocks)
    assert [residual.pack_block(3, g["th"], g["tw"], tau, tiles[f:f + batch]) for f in range(0, g["n"], batch)] == blocks
    u = codec.unpack_image_stream(stream)
    assert u["version"] == 4 and u["max_error"] == tau and u["overlap"] == 0 and u["segments"] == segments
    assert u["blobs"] == blobs and u["residuals"] == blocks
    assert codec.pack_image_stream(u, u["blobs"], u["residuals"]) == stream
    ix = codec.stream_index(stream)
    assert ix["max_error"] == tau and len(ix["tiles"]) == g["n"]
    for t, r in enumerate(ix["tiles"]):
        smin, tabs, strings = tiles[t]
        assert (r["r_smin"], r["r_L"]) == (smin, tabs.shape[1])
        assert r["r_segs"] == [len(s) for s in strings]
        assert stream[r["r_off"]:r["r_off"] + r["r_len"]] == tabs.astype("<u2").tobytes() + b"".join(strings)
    assert [stream[c["r_offset"]:c["r_offset"] + c["r_bytes"]] for c in ix["containers"]] == blocks

    # heads and records only, also from a file object
    class Counting(io.BytesIO):
        count = 0

        def read(self, n=-1):
            out = super().read(n)
            self.count += len(out)
            return out
    f = Counting(stream)
    assert codec.stream_index(f) == ix
    Bs = [min(batch, g["n"] - first) for first in range(0, g["n"], batch)]
    seg_head = (4 if segments > 1 else 0)
    assert f.count == ix["index_bytes"] == 76 + sum(
        8 + 38 + seg_head + (24 + (4 * segments if segments > 1 else 0)) * B + 8 + 30 + 76 * B for B in Bs)
    # spans: the strings and the residual span of every selected tile, merged where they touch
    for sel in ([0], [g["n"] - 1], list(range(g["n"])), [0, g["n"] - 1]):
        sel = sorted(set(sel))
        spans = codec.tile_spans(ix, sel)
        assert spans == sorted(spans) and all(a + n <= b for (a, n), (b, _) in zip(spans, spans[1:]))
        covered = b"".join(stream[a:a + n] for a, n in spans)
        want = sum(ix["tiles"][t]["z_len"] + ix["tiles"][t]["y_len"] + ix["tiles"][t]["r_len"] for t in sel)
        assert len(covered) == want
        for t in sel:
            r = ix["tiles"][t]
            assert any(a <= r["r_off"] and r["r_off"] + r["r_len"] <= a + n for a, n in spans)


def test_versions_1_to_3_are_unchanged():
    header, blobs, _, _, g = _build(150, 200, 64, 5, 2)
    h1 = {k: v for k, v in header.items() if k not in ("max_error", "segments")}
    base = struct.pack("<6sHI6I4I2I", b"DSICI\x00", 1, TAG, 150, 200, 3, 0, 64, 64, N, M, 3, 0, 5, len(blobs))
    body = b"".join(struct.pack("<Q", len(b)) + b for b in blobs)
    s1 = codec.pack_image_stream(h1, blobs)
    assert s1 == base + body == codec.pack_image_stream(dict(h1, max_error=None), blobs)
    s3 = codec.pack_image_stream(dict(h1, overlap=16), blobs)
    assert s3 == base[:6] + struct.pack("<H", 3) + base[8:] + struct.pack("<2I", 1, 16) + body
    keys = {"version", "numerics", "H", "W", "C", "kind", "th", "tw", "N", "M", "in_ch", "spatial_params", "batch",
            "batches", "segments", "overlap", "blobs"}
    for s in (s1, s3):
        assert set(codec.unpack_image_stream(s)) == keys
        ix = codec.stream_index(s)
        assert "max_error" not in ix
        assert set(ix["tiles"][0]) == {"k", "b", "min_y", "max_y", "min_z", "max_z", "z_off", "z_len", "y_off", "y_len",
                                       "y_segs"}
        assert set(ix["containers"][0]) == {"offset", "bytes", "first", "tiles", "shape_y", "shape_z"}
        assert codec.tile_spans(ix, [0]) == [(ix["tiles"][0]["z_off"], ix["tiles"][0]["z_len"]
                                              + ix["tiles"][0]["y_len"])]


# ---- refusals -----------------------------------------------------------------------------------------------------
def test_refusals_of_the_stream():
    header, blobs, blocks, tiles, g = _build(150, 200, 64, 5, 2)
    stream = codec.pack_image_stream(header, blobs, blocks)
    codec.stream_index(stream)
    for bad in (-1, 128, 1.5, "2", True):
        with pytest.raises(ValueError, match="max_error"):
            codec.pack_image_stream(dict(header, max_error=bad), blobs, blocks)
    with pytest.raises(ValueError, match="overlap"):
        codec.pack_image_stream(dict(header, overlap=16), blobs, blocks)
    with pytest.raises(ValueError, match="residual"):
        codec.pack_image_stream(header, blobs)
    with pytest.raises(ValueError, match="residual"):
        codec.pack_image_stream(header, blobs, blocks[:-1])
    with pytest.raises(ValueError, match="residual"):
        codec.pack_image_stream({k: v for k, v in header.items() if k != "max_error"}, blobs, blocks)
    # a version-4 head with overlap != 0, bands != 16, max_error > 127
    for at, word, match in ((64, 16, "overlap"), (72, 8, "res_bands"), (68, 128, "max_error")):
        with pytest.raises(ValueError, match=match):
            codec.stream_index(stream[:at] + struct.pack("<I", word) + stream[at + 4:])
    for cut in (61, 70, 75, 80, len(stream) - 1):
        with pytest.raises(ValueError, match="truncated"):
            codec.stream_index(stream[:cut])
    with pytest.raises(ValueError, match="trailing"):
        codec.stream_index(stream + b"\x00")

    def with_block(k, block):
        return codec.pack_image_stream(header, blobs, blocks[:k] + [block] + blocks[k + 1:])

    b0, n0 = blocks[0], 5
    # n, C, th, tw, tau that contradict the head; bands
    for field, value in enumerate((4, 4, 32, 128, 3)):
        forged = b0[:6 + 4 * field] + struct.pack("<I", value) + b0[10 + 4 * field:]
        with pytest.raises(ValueError, match="head says"):
            codec.stream_index(with_block(0, forged))
    with pytest.raises(ValueError, match="bands"):
        codec.stream_index(with_block(0, b0[:26] + struct.pack("<I", 8) + b0[30:]))
    with pytest.raises(ValueError, match="not a residual block"):
        codec.stream_index(with_block(1, b"DSICX\x00" + blocks[1][6:]))
    # lengths that do not add up
    for forged in (b0[:-1], b0 + b"\x00", b0[:20], b0[:30 + 12 * n0 + 10]):
        with pytest.raises(ValueError, match="truncated"):
            codec.stream_index(with_block(0, forged))
    rec = 30 + 12 * 2                                                   # tile 2's record: smin, L, span_bytes
    smin, L, span = struct.unpack_from("<iII", b0, rec)
    with pytest.raises(ValueError, match="add up"):
        codec.stream_index(with_block(0, b0[:rec + 8] + struct.pack("<I", span + 1) + b0[rec + 12:]))
    seg = 30 + 12 * n0 + 64 * 2
    with pytest.raises(ValueError, match="add up"):
        codec.stream_index(with_block(0, b0[:seg] + struct.pack("<I", struct.unpack_from("<I", b0, seg)[0] + 2)
                                      + b0[seg + 4:]))
    Q = R.q_max(2)
    for s_bad, L_bad in ((-Q - 1, 1), (Q, 2), (0, 0), (-Q, 2 * Q + 2)):
        with pytest.raises(ValueError, match="support"):
            codec.stream_index(with_block(0, b0[:rec] + struct.pack("<iI", s_bad, L_bad) + b0[rec + 8:]))


def test_compress_image_refuses_before_any_gpu_work():
    import torch
    from dsic_amd.model import CompressionModel
    model = CompressionModel(N=16, M=16, spatial_params=False, min_nu=2, max_nu=100.0, in_ch=3)
    u8 = torch.zeros((64, 64, 3), dtype=torch.uint8)
    for bad in (-1, 128, 2.0, "1", True):
        with pytest.raises(ValueError, match="max_error"):
            codec.compress_image(model, u8, tile=64, max_error=bad)
    with pytest.raises(ValueError, match="uint8"):
        codec.compress_image(model, torch.zeros((3, 64, 64), dtype=torch.float32), tile=64, max_error=1)
    with pytest.raises(ValueError, match="overlap"):
        codec.compress_image(model, torch.zeros((128, 128, 3), dtype=torch.uint8), tile=64, overlap=16, max_error=1)


# ---- the new exports refuse bad arguments before any launch ---------------------------------------------------------
def test_new_exports_validate_arguments_without_gpu():
    from dsic_amd import lib
    L = lib.load()
    one = 16

    def quant(tiles=one, x_hat=one, own=one, n=2, C=3, th=32, tw=48, tau=1, q=one, hist=one):
        return L.dsic_residual_quantize_u8(tiles, x_hat, own, n, C, th, tw, tau, q, hist, None)

    def tabs(hist=one, n=2, C=3, th=32, tw=48, tau=1, Lmax=None, meta=one, compact=one, coder=one):
        return L.dsic_residual_tables(hist, n, C, th, tw, tau, R.lmax(max(0, min(tau, 127))) if Lmax is None else Lmax,
                                      meta, compact, coder, None)

    def pack(bytes_=one, cap_z=8, cap_seg=64, lengths=one, meta=one, compact=one, n=2, C=3, th=32, tw=48, tau=1,
             Lmax=None, ws=one, out=one):
        return L.dsic_residual_pack(bytes_, cap_z, cap_seg, lengths, meta, compact, None, n, C, th, tw, tau,
                                    R.lmax(max(0, min(tau, 127))) if Lmax is None else Lmax, ws, out, None)

    def stitch(tiles=one, q=one, tau=1, ids=one, n=1, out=one, H=150, W=200, C=3, th=64, tw=64, win=(0, 0, 150, 200)):
        return L.dsic_tile_stitch_window_u8_res(tiles, q, tau, ids, n, out, H, W, C, th, tw, *win, None)

    common = (({"C": 2}, b"C="), ({"C": 5}, b"C="), ({"tau": -1}, b"tau"), ({"tau": 128}, b"tau"),
              ({"th": 40}, b"th % 16"), ({"n": 0}, b"tiles per call"))
    for fn, extra in ((quant, (({"tiles": None}, b"null"), ({"x_hat": None}, b"null"), ({"own": None}, b"null"),
                               ({"q": None}, b"null"), ({"hist": None}, b"null"), ({"q": 20}, b"aligned"),
                               ({"tw": 40}, b"multiples of 16"))),
                      (tabs, (({"hist": None}, b"null"), ({"meta": None}, b"null"), ({"compact": None}, b"null"),
                              ({"coder": None}, b"null"), ({"Lmax": 256}, b"Lmax"), ({"coder": 24}, b"aligned"))),
                      (pack, (({"bytes_": None}, b"null"), ({"lengths": None}, b"null"), ({"compact": None}, b"null"),
                              ({"ws": None}, b"null"), ({"out": None}, b"null"), ({"Lmax": 8}, b"Lmax"),
                              ({"cap_seg": 6}, b"capacities"), ({"bytes_": 18}, b"aligned")))):
        for kw, word in common + extra:
            assert fn(**kw) == 1, (fn.__name__, kw)
            assert word in L.dsic_last_error(), (fn.__name__, kw, L.dsic_last_error())
    for kw, word in (({"tiles": None}, b"null"), ({"q": None}, b"null"), ({"ids": None}, b"null"),
                     ({"out": None}, b"null"), ({"C": 5}, b"C="), ({"tau": -1}, b"tau"), ({"tau": 128}, b"tau"),
                     ({"th": 40}, b"multiples of 16"), ({"win": (0, 0, 151, 200)}, b"window"), ({"n": 0}, b"tiles"),
                     ({"out": 20}, b"aligned")):
        assert stitch(**kw) == 1, kw
        assert word in L.dsic_last_error(), (kw, L.dsic_last_error())
    assert L.dsic_abi_version() == 4
