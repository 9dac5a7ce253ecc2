"""CPU-only: the DSICI writer and reader and the two residual block formats against tests/golden/dsici_heads.json, the
bytes and dicts recorded by tests/golden/make_golden_dsici_heads.py at the commit before the format became a table: one
case per head layout (v1, v2, v3 with K = 1 and 2, v4, v5, v6 with and without overlap, v8 of kind 0 and 2, v9), and
one DSICR and one DSICW block."""
import json
import os

import pytest

from dsic_amd import codec, residual, residual16

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dsici_heads.json")) as f:
    FIXTURE = json.load(f)
STREAMS = {case["name"]: case for case in FIXTURE["streams"]}


def _jsonable(v):
    """The generator's normal form: bytes as hex, tuples as lists."""
    if isinstance(v, (bytes, bytearray, memoryview)):
        return bytes(v).hex()
    if isinstance(v, dict):
        return {k: _jsonable(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_jsonable(x) for x in v]
    return v


def _blocks(hexes):
    return None if hexes is None else [bytes.fromhex(b) for b in hexes]


def test_the_fixture_covers_every_layout():
    assert sorted(STREAMS) == ["v1", "v2_k4", "v3_k1", "v3_k2", "v4", "v5", "v6_o0", "v6_o16", "v8_kind0", "v8_kind2", "v9"]
    versions = {case["unpacked"]["version"] for case in STREAMS.values()}
    assert versions == {1, 2, 3, 4, 5, 6, 8, 9} == set(codec.FORMATS)


@pytest.mark.parametrize("name", sorted(STREAMS))
def test_pack_writes_the_recorded_stream_and_unpack_returns_the_recorded_dict(name):
    case = STREAMS[name]
    mask = None if case["mask"] is None else bytes.fromhex(case["mask"])
    stream = codec.pack_image_stream(case["header"], _blocks(case["blobs"]), _blocks(case["residuals"]), mask)
    assert stream.hex() == case["stream"]
    got = _jsonable(codec.unpack_image_stream(bytes.fromhex(case["stream"])))
    assert sorted(got) == sorted(case["unpacked"])
    for key, want in case["unpacked"].items():
        assert got[key] == want, key


def _tiles(case):
    tiles = []
    for smin, tables, *kp, strings in case["tiles"]:
        kp = [kp[0], bytes.fromhex(kp[1])] if kp else []
        tiles.append((smin, bytes.fromhex(tables), *kp, [bytes.fromhex(s) for s in strings]))
    return tiles


@pytest.mark.parametrize("name,layer,ks", [("DSICR", residual, None), ("DSICW", residual16, [0, 9])])
def test_the_residual_blocks_are_the_recorded_ones(name, layer, ks):
    case = FIXTURE["blocks"][name]
    tiles = _tiles(case)
    C, th, tw, tau = case["C"], case["th"], case["tw"], case["tau"]
    assert (len(tiles), C, th, tw) == (2, 3, 32, 32)
    block = layer.pack_block(C, th, tw, tau, tiles)
    assert block.hex() == case["block"] and block[:6] == layer.MAGIC
    recs = layer.read_block_head(lambda off, n: block[off:off + n], 0, len(block), 2, C, th, tw, tau)
    assert _jsonable(recs) == case["records"] and recs[0]["r_off"] == layer.head_bytes(2)
    assert [r.get("r_k") for r in recs] == (ks or [None, None])
