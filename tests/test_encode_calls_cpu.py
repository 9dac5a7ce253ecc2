"""What compress_image refuses and what it does, case by case, against a recording (tests/golden/encode_calls.json).

The write side of codec.py checks its options, gathers tiles batch by batch, hands each batch to the coder and to the
residual layer, and frames the results.  Here everything beneath that is a stand-in, so no GPU is needed: the model is
a shape-only module on the CPU, lib.load() is a logger whose exports return 0, codec._p gives a tensor's shape, dtype
and storage offset (so the slice a run of tiles is gathered into shows), codec._stream is a token, and deterministic
stubs stand at the module boundaries: entropy.compress_to_container and _coded_batch return bytes that name the tiles
they were given, the two residual layers' encode_block log their arguments, mask.classify / classify_valid return
counts that make the tile states a case asks for, mask.encode_block packs a real block from its states, band_range
returns fixed pairs and build_overviews zero images of overview_shapes' sizes.  What comes out is a real DSICI or DSICP
stream around stub payloads.  A case's outcome is the exception's exact text, or the ordered log plus the unpacked
stream without its payloads' bytes.  The recording holds every distinct record once and, per case, their numbers.

    python tests/test_encode_calls_cpu.py --record OUT.json [--root TREE]

writes the outcomes of TREE (default: this tree).  The stored file was recorded on the commit before the encode path
got one option check, one gather and one batch loop per level.
"""
import contextlib
import itertools
import json
import os
import sys

import numpy as np
import torch

N, M = 128, 192
PATTERNS = ("full", "empty", "gaps", "alternate", "mixed")


class Stub(torch.nn.Module):
    def __init__(self, in_ch=3, m=M):
        super().__init__()
        self.N, self.M = N, m
        self.g_a = torch.nn.Module()
        self.g_a.g_a = torch.nn.ModuleList([torch.nn.Conv2d(in_ch, 4, 1)])


def _states(pattern, n):
    """0 empty, 1 full, 2 mixed per tile: the patterns the masked cases are run with."""
    return {"full": [1] * n, "empty": [0] * n, "gaps": [0 if t in (0, 5, 11) else 1 for t in range(n)],
            "alternate": [1 - t % 2 for t in range(n)], "mixed": [(2, 1, 0)[t % 3] for t in range(n)]}[pattern]


def _t(x):
    return [list(x.shape), str(x.dtype).replace("torch.", "")]


def _plain(a):
    """An argument as JSON holds it."""
    if isinstance(a, torch.Tensor):
        return _t(a)
    if isinstance(a, (int, float, str, bool)) or a is None:
        return a
    return [_plain(v) for v in a]                      # lists, tuples, ctypes arrays


class _Library:
    def __init__(self, log):
        self._log = log

    def __getattr__(self, name):
        def export(*args):
            self._log.append([name] + [_plain(a) for a in args])
            return 0
        return export


@contextlib.contextmanager
def _patched(log, pattern):
    from dsic_amd import codec, entropy, lib, mask, residual, residual16

    def grid(g):
        return [g["H"], g["W"], g["th"], g["tw"], g["n"], g["overlap"]]

    def name(what, x, segments):
        return f"{what}{list(x.shape)}{str(x.dtype).replace('torch.', '')}/K{segments}".encode()

    def compress_to_container(model, x, tail=10, Lmax=entropy.DEFAULT_LMAX, segments=1):
        log.append(["compress_to_container", _t(x), tail, Lmax, segments])
        return name("container", x, segments)

    def coded_batch(model, x, tail, Lmax, what, pack=False, segments=1):
        log.append(["_coded_batch", _t(x), tail, Lmax, what, pack, segments])
        blob = name("coded", x, segments)
        n, (th, tw) = x.shape[0], (x.shape[1:3] if x.dtype == torch.uint8 else x.shape[2:4])
        return {"container": torch.frombuffer(bytearray(blob + b"-spare"), dtype=torch.uint8),
                "container_bytes": len(blob), "x_hat": torch.zeros((n, model.g_a.g_a[0].in_channels, th, tw))}

    def encode_block(tiles, x_hat, own, tau):
        log.append(["residual.encode_block", _t(tiles), _t(x_hat), _plain(own), tau])
        return f"residual{list(tiles.shape)}/tau{tau}".encode()

    def encode_block16(img, x_hat, H, W, th, tw, lohi, tau, first):
        log.append(["residual16.encode_block", _t(img), _t(x_hat), H, W, th, tw, _plain(lohi), tau, first])
        return f"residual16{list(x_hat.shape)}/tau{tau}/first{first}".encode()

    def counts(g):
        owned = [codec._owned_in_tile(g, t) for t in range(g["n"])]
        return np.array([{0: (b - a) * (d - c), 1: 0, 2: 1}[s]
                         for s, (a, b, c, d) in zip(_states(pattern, g["n"]), owned)], dtype=np.int64)

    def classify(img, g, C, nodata):
        log.append(["mask.classify", _t(img), grid(g), C, nodata])
        return counts(g)

    def classify_valid(valid, g):
        log.append(["mask.classify_valid", _t(valid), grid(g)])
        return counts(g)

    def mask_block(img, g, C, nodata, states):
        log.append(["mask.encode_block", _t(img), grid(g), C, nodata, list(states)])
        ps = mask.pos_bytes(g["th"], g["tw"])
        mixed = [t for t, s in enumerate(states) if s == mask.MIXED]
        return mask.pack_block(g["th"], g["tw"], nodata, states, [(t, 1, ps) for t in mixed], [bytes(ps)] * len(mixed))

    def band_range(img, valid=None):
        log.append(["band_range", _t(img), None if valid is None else _t(valid)])
        return [(10 * c, 1000 + c) for c in range(img.shape[2])]

    def build_overviews(img, n, valid=None):
        log.append(["build_overviews", _t(img), n, None if valid is None else _t(valid)])
        kind, H, W, C = codec._image_kind(img, "build_overviews")
        shapes = codec.overview_shapes(H, W, n)
        levels = [img] + [torch.zeros((C, h, w) if kind == codec.KIND_F32_CHW else (h, w, C), dtype=img.dtype)
                          for h, w in shapes[1:]]
        return levels if valid is None else (levels, [torch.ones((h, w), dtype=torch.bool) for h, w in shapes])

    stand_in = _Library(log)
    patches = [(lib, "load", lambda: stand_in), (codec, "_stream", lambda: "stream"),
               (codec, "_p", lambda t: _t(t) + [t.storage_offset()]),
               (entropy, "compress_to_container", compress_to_container), (entropy, "_coded_batch", coded_batch),
               (residual, "encode_block", encode_block), (residual16, "encode_block", encode_block16),
               (mask, "classify", classify), (mask, "classify_valid", classify_valid), (mask, "encode_block", mask_block),
               (codec, "band_range", band_range), (codec, "build_overviews", build_overviews)]
    saved = [(mod, key, getattr(mod, key)) for mod, key, _ in patches]
    try:
        for mod, key, new in patches:
            setattr(mod, key, new)
        yield
    finally:
        for mod, key, old in saved:
            setattr(mod, key, old)


def _image(kind, H, W, C=3):
    if kind == "f32":
        return torch.zeros((C, H, W))
    return torch.zeros((H, W, C), dtype=torch.uint8 if kind == "u8" else torch.uint16)


def _options(C, H, W):
    """The eight options of the refusal cases, by name."""
    return {"overlap": 16, "max_error": 1, "nodata": 0, "scale": [(0, 1000)] * C,
            "valid": torch.ones((H, W), dtype=torch.bool), "fill": 3, "tolerance": 2, "overviews": 1}


def _cases():
    """{id: (model, image, keyword arguments, state pattern)}"""
    out = {}

    def add(cid, model, img, kw, pattern="full"):
        assert cid not in out, cid
        out[cid] = (model, img, kw, pattern)

    m3, m4, m24 = Stub(3), Stub(4), Stub(3, 24)
    # ---- refusals: every subset of at most three of the eight options, per kind ----------------------------------
    H, W = 100, 150
    images = {"u8": (m3, _image("u8", H, W)), "u16": (m3, _image("u16", H, W)), "f32": (m3, _image("f32", H, W)),
              "u16x5": (m3, _image("u16", H, W, 5))}
    for name, (model, img) in images.items():
        opts = _options(5 if name == "u16x5" else 3, H, W)
        for r in range(4):
            for names in itertools.combinations(opts, r):
                add(f"opts/{name}/{'+'.join(names) or 'none'}", model, img, {k: opts[k] for k in names})
    # ---- refusals: single bad values, per kind ------------------------------------------------------------------------
    ok = torch.ones((H, W), dtype=torch.bool)
    bad = {"nodata=256": {"nodata": 256}, "nodata=True": {"nodata": True}, "fill=256": {"valid": ok, "fill": 256},
           "fill=65536": {"valid": ok, "fill": 65536}, "fill=True": {"valid": ok, "fill": True},
           "fill=True_alone": {"fill": True}, "fill=0.0_alone": {"fill": 0.0}, "tolerance=-1": {"tolerance": -1},
           "tolerance=32768": {"tolerance": 32768}, "max_error=128": {"max_error": 128},
           "max_error=True": {"max_error": True}, "max_error=1.5": {"max_error": 1.5},
           "scale_short": {"scale": [(0, 1000)] * 2}, "scale_reversed": {"scale": [(5, 1)] * 3},
           "scale_not_pairs": {"scale": 7}, "batch=0": {"batch": 0}, "segments=3": {"segments": 3},
           "valid_shape": {"valid": torch.ones((H, W - 1), dtype=torch.bool)},
           "valid_transposed": {"valid": torch.ones((W, H), dtype=torch.bool)},
           "valid_uint8": {"valid": torch.ones((H, W), dtype=torch.uint8)}, "valid_numpy": {"valid": np.ones((H, W), bool)},
           "tile=48": {"tile": 48}, "tile=40": {"tile": 40}, "tile=16": {"tile": 16}, "overlap=64_tile=64": {"tile": 64, "overlap": 64},
           "overlap=8": {"overlap": 8}, "overlap=-16": {"overlap": -16}, "overlap=str": {"overlap": "a"},
           "overlap=32_level2": {"tile": 64, "overlap": 32, "overviews": 2}, "overviews=3": {"overviews": 3},
           "overviews=-1": {"overviews": -1}, "overviews=1.5": {"overviews": 1.5},
           "max_error_overlap_overviews": {"max_error": 1, "overlap": 16, "overviews": 1},
           # max_error's own rules come after level 0's geometry and before level 1's
           "max_error_tile=40": {"max_error": 1, "tile": 40},
           "max_error_overlap=32_level2": {"max_error": 1, "tile": 64, "overlap": 32, "overviews": 2},
           "nodata=256_overlap": {"nodata": 256, "overlap": 16}, "tolerance=-1_valid": {"tolerance": -1, "valid": ok},
           "segments=3_batch=0_tile=40": {"segments": 3, "batch": 0, "tile": 40}, "batch=0_tile=40": {"batch": 0, "tile": 40},
           "overviews=3_nodata": {"overviews": 3, "nodata": 0}, "overviews=3_batch=0": {"overviews": 3, "batch": 0},
           "overviews=1.5_segments=3": {"overviews": 1.5, "segments": 3}, "batch=x_segments=3": {"batch": "x", "segments": 3},
           "batch=x_tile=40": {"batch": "x", "tile": 40}}
    for name in ("u8", "u16", "f32"):
        for cid, kw in bad.items():
            add(f"bad/{name}/{cid}", *images[name], kw)
    add("bad/u8/segments=16_M=24", m24, images["u8"][1], {"segments": 16})
    add("bad/u8/channels", m3, _image("u8", H, W, 4), {})
    add("bad/u16/channels", m3, _image("u16", H, W, 4), {})
    add("bad/f32/channels", m4, images["f32"][1], {})
    add("bad/u8/tiny", m3, _image("u8", 10, 150), {})
    add("bad/u8/4_dims", m3, torch.zeros((1, H, W, 3), dtype=torch.uint8), {})
    add("bad/i32/dtype", m3, torch.zeros((H, W, 3), dtype=torch.int32), {})
    # ---- traces: tile 64, batch 4; 150 x 200 is 12 tiles (a whole last batch), 150 x 270 is 15 (a last batch of 3) ----
    T = {"tile": 64, "batch": 4}
    kinds = {"u8": (m3, 3), "u16": (m3, 3), "u16x4": (m4, 4), "f32": (m3, 3)}
    for name, (model, C) in kinds.items():
        for H, W in ((150, 200), (150, 270), (40, 50)):
            main = (H, W) == (150, 200)
            if name == "u16x4" and not main:
                continue
            img = _image(name[:3], H, W, C)
            k = f"trace/{name}/{H}x{W}"
            add(k + "/plain", model, img, T)
            add(k + "/segments=2", model, img, dict(T, segments=2))
            add(k + "/overlap=16", model, img, dict(T, overlap=16))
            if main:
                add(k + "/overlap=16_segments=2_tail=12", model, img, dict(T, overlap=16, segments=2, tail=12))
            if H > 40:
                add(k + "/overviews=2", model, img, dict(T, overviews=2))         # level 2 is smaller than a tile
            if main:
                add(k + "/overviews=2_overlap=16", model, img, dict(T, overviews=2, overlap=16))
            bound = {"u8": {"max_error": 2}, "u16": {"tolerance": 3}}.get(name[:3])
            if bound:
                add(k + "/bound", model, img, dict(T, **bound))
                if main:
                    add(k + "/bound_segments=2", model, img, dict(T, segments=2, **bound))
                if H > 40:
                    add(k + "/bound_overviews=2", model, img, dict(T, overviews=2, **bound))  # level 0 only
            if name[:3] == "u16":
                add(k + "/scale", model, img, dict(T, scale=[(100, 9000 + c) for c in range(C)]))
            if name == "f32" or H == 40 or W == 270 and name != "u8":
                continue
            valid = torch.ones((H, W), dtype=torch.bool)
            for pattern in PATTERNS if name != "u16x4" else ("gaps", "mixed"):
                if name == "u8":
                    add(f"{k}/nodata_{pattern}", model, img, dict(T, nodata=7), pattern)
                    if main and pattern == "gaps":
                        add(f"{k}/nodata_segments=2_{pattern}", model, img, dict(T, nodata=7, segments=2), pattern)
                add(f"{k}/valid_{pattern}", model, img, dict(T, valid=valid, fill=9), pattern)
                if main:
                    add(f"{k}/valid_overviews=2_{pattern}", model, img, dict(T, valid=valid, overviews=2), pattern)
                if name[:3] == "u16":
                    scale = [(100, 9000 + c) for c in range(C)]
                    add(f"{k}/valid_scale_{pattern}", model, img, dict(T, valid=valid, fill=60000, scale=scale), pattern)
                    add(f"{k}/valid_scale_overviews=2_{pattern}", model, img,
                        dict(T, valid=valid, scale=scale, overviews=2, segments=2), pattern)
    return out


def _unpacked(codec, stream):
    """The stream as records: per level its place in the pyramid, its header fields, and its payloads apart (the stub
    payloads are names, kept as text; the mask block as hex)."""
    if bytes(stream[:6]) == codec.PMAGIC:
        p = codec.unpack_pyramid_stream(stream)
        return [["pyramid", p["version"], len(p["levels"])]] + [r for d in p["levels"] for r in
                                                                [["level", d["H"], d["W"], d["offset"], d["length"]]]
                                                                + _unpacked(codec, d["stream"])]
    h = codec.unpack_image_stream(stream)
    blobs, residuals, mask = h.pop("blobs"), h.pop("residuals", None), h.pop("mask", None)
    parts = {"model": ("numerics", "N", "M", "in_ch", "spatial_params", "C", "kind"), "image": ("H", "W", "th", "tw"),
             "scale": ("scale",)}                                      # header fields that many streams share, apart
    out = [[name, {k: _plain(h.pop(k)) for k in keys if k in h}] for name, keys in parts.items()]
    out = [r for r in out if r[1]] + [["stream", {k: _plain(v) for k, v in sorted(h.items())}],
                                      ["blobs"] + [b.decode() for b in blobs]]
    if residuals is not None:
        out.append(["residuals"] + [b.decode() for b in residuals])
    return out + ([["mask", mask.hex()]] if mask is not None else [])


def outcomes():
    """{case id: outcome} of the dsic_amd that is importable now.  An outcome is the refusal, "Type: text", or the list
    of records: the ordered log, then the unpacked stream; every record as its JSON text."""
    from dsic_amd import codec
    out = {}
    for cid, (model, img, kw, pattern) in _cases().items():
        log = []
        with _patched(log, pattern):
            try:
                got = log + _unpacked(codec, codec.compress_image(model, img, **kw))
                out[cid] = [json.dumps(r, separators=(",", ":"), sort_keys=True) for r in got]
            except Exception as e:     # a refusal comes before anything is launched; one that does not says so
                out[cid] = f"{type(e).__name__}: {e}" + (f" (after {len(log)} calls)" if log else "")
    return out


def _write(path, got):
    """The recording: the distinct records once ("records"), the refusals by text with the cases that meet each
    ("refused"), and per accepted case the numbers of its records ("accepted"); one entry per line."""
    records, refused, accepted = {}, {}, {}
    for cid, o in got.items():
        if isinstance(o, str):
            refused.setdefault(o, []).append(cid)
        else:
            accepted[cid] = [records.setdefault(r, len(records)) for r in o]

    def lines(items):
        return ",\n".join(items)
    with open(path, "w") as f:
        f.write('{"records": [\n' + lines(records) + '\n],\n"refused": {\n'
                + lines(f"{json.dumps(t)}: {json.dumps(ids)}" for t, ids in refused.items()) + '\n},\n"accepted": {\n'
                + lines(f"{json.dumps(cid)}: {json.dumps(ix, separators=(',', ':'))}" for cid, ix in accepted.items())
                + "\n}}\n")


def _recording(golden_dir):
    """The stored file as outcomes() gives them."""
    want = json.load(open(os.path.join(golden_dir, "encode_calls.json")))
    records = [json.dumps(r, separators=(",", ":"), sort_keys=True) for r in want["records"]]
    out = {cid: text for text, ids in want["refused"].items() for cid in ids}
    out.update({cid: [records[i] for i in ix] for cid, ix in want["accepted"].items()})
    return out


def test_every_refusal_and_trace_equals_the_recording(golden_dir):
    want, got = _recording(golden_dir), outcomes()
    assert sorted(got) == sorted(want), "the case table and the recording differ: re-record"
    bad = [f"{cid}:\n  got      {got[cid]}\n  recorded {want[cid]}" for cid in got if got[cid] != want[cid]]
    assert not bad, f"{len(bad)} of {len(got)} cases differ; first ones:\n" + "\n".join(bad[:10])


def test_the_recording_covers_every_branch(golden_dir):
    """the case table is worth something only if the outcomes differ where the code has a choice"""
    want = _recording(golden_dir)
    refused = {cid: o for cid, o in want.items() if isinstance(o, str)}
    want = {cid: [json.loads(r) for r in o] for cid, o in want.items() if cid not in refused}
    assert not [t for t in refused.values() if t.endswith("calls)")], "a refusal after something was launched"
    assert len(set(refused.values())) >= 40 and len(want) >= 150
    assert len([c for c in list(want) + list(refused) if c.startswith("opts/")]) == 4 * (1 + 8 + 28 + 56)
    calls = {r[0] for o in want.values() for r in o}
    assert {"dsic_tile_gather_" + k + ov for k in ("u8", "u16", "f32") for ov in ("", "_ov")} <= calls
    assert {"compress_to_container", "_coded_batch", "residual.encode_block", "residual16.encode_block", "mask.classify",
            "mask.classify_valid", "mask.encode_block", "band_range", "build_overviews"} <= calls

    def gathers(cid):
        return [(r[0], r[2][0][0], r[2][2], r[-3], r[-2]) for r in want[cid] if r[0].startswith("dsic_tile_gather")]

    def heads(cid):                        # per level the header fields, put together again
        rs = [r for r in want[cid] if r[0] in ("model", "image", "scale", "stream")]
        return [dict(kv for r in rs[i:j + 1] for kv in r[1].items())
                for i, j in zip([0] + [k + 1 for k, r in enumerate(rs) if r[0] == "stream"][:-1],
                                [k for k, r in enumerate(rs) if r[0] == "stream"])]
    # (export, tiles of the slice, its offset in the batch tensor, first tile, tiles): whole batches are one call each
    tile = 64 * 64 * 3
    assert gathers("trace/u8/150x200/plain") == [("dsic_tile_gather_u8", 4, 0, f, 4) for f in (0, 4, 8)]
    assert [g[3:] for g in gathers("trace/f32/150x270/plain")] == [(0, 4), (4, 4), (8, 4), (12, 3)]
    # empty tiles at 0, 5 and 11: coded 1 2 3 4 | 6 7 8 9 | 10, as runs (1..4), (6..9), (10)
    assert gathers("trace/u8/150x200/nodata_gaps") == [("dsic_tile_gather_u8", 4, 0, 1, 4), ("dsic_tile_gather_u8", 4, 0, 6, 4),
                                                       ("dsic_tile_gather_u8", 1, 0, 10, 1)]
    # 15 tiles without 0, 5, 11: 1 2 3 4 | 6 7 8 9 | 10 12 13 14, the last batch as runs of 1 and 3
    assert gathers("trace/u8/150x270/valid_gaps")[2:] == [("dsic_tile_gather_u8", 1, 0, 10, 1),
                                                          ("dsic_tile_gather_u8", 3, tile, 12, 3)]
    alt = gathers("trace/u16/150x200/valid_alternate")
    assert [g[4] for g in alt] == [1] * 6 and [g[2] for g in alt] == [0, tile, 2 * tile, 3 * tile, 0, tile]
    assert not gathers("trace/u8/150x200/valid_empty") and heads("trace/u8/150x200/valid_empty")[0]["batches"] == 0
    # the error bound is level 0's alone, and a masked stream is written with overlap 0
    for cid, key in (("trace/u8/150x200/bound_overviews=2", "max_error"), ("trace/u16/150x200/bound_overviews=2", "tolerance")):
        assert [key in h for h in heads(cid)] == [True, False, False]
        assert [h["version"] for h in heads(cid)][1:] in ([1, 1], [6, 6])
    assert {h["version"] for c in want if "/nodata_" in c for h in heads(c)} == {5}
    assert {h["overlap"] for c in want if "/nodata_" in c or "/valid_" in c for h in heads(c)} == {0}
    assert {h["th"] for h in heads("trace/f32/150x200/overviews=2")} == {64, 48}


def test_the_refusal_table_holds_what_the_formats_exclude():
    """every pair of options that pack_image_stream would refuse from FORMATS is a row of the writer's table, and the
    table adds only what the writer alone refuses"""
    from dsic_amd import codec
    name = {"fill": "valid", "scale": "a uint16 image"}
    derived = set()
    for v, e in codec.FORMATS.items():
        if e.key:
            a = name.get(e.key, e.key)
            rivals = [r for u, r in codec.FORMATS.items() if u < v and r.key and r.key not in e.fields]
            derived |= {frozenset((a, b)) for b in ["overlap > 0"] * (e.overlap == "zero") + [name.get(r.key, r.key) for r in rivals]}
    rows = {frozenset((a, "a uint16 image" if b == "kind" else b)) for a, b, text in codec._REFUSALS
            if text and "together with" in text}
    assert rows - derived == {frozenset(("nodata", "overviews > 0"))} and not derived - rows


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", required=True, metavar="OUT.json")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import dsic_amd
    got = outcomes()
    _write(a.record, got)
    print(f"{a.record}: {len(got)} cases of {os.path.dirname(dsic_amd.__file__)}")
