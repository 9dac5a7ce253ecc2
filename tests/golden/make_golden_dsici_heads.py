#!/usr/bin/env python3
"""Generate tests/golden/dsici_heads.json: what the DSICI writer and reader, and the two residual block formats, did
at the commit the fixture was made at.

    python tests/golden/make_golden_dsici_heads.py

Only pack_image_stream, unpack_image_stream, mask.pack_block, residual.pack_block / read_block_head and
residual16.pack_block / read_block_head are called, so the script runs unchanged on any later tree; the test
(tests/test_stream_golden_cpu.py) holds that tree to the recorded bytes and dicts.  One case per head layout: v1, v2,
v3 (K = 1 and 2), v4, v5, v6 (overlap 0 and 16), v8 (kind 0 and 2) and v9.  The containers are a handful of made-up
bytes (neither function looks inside them); the masked cases have a 2 x 2 grid with an empty, a full and two mixed
tiles (one payload per mode).  The file holds data only: header dicts, blocks and streams as hex, the returned dicts
with their bytes as hex.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from dsic_amd import codec, mask, residual, residual16  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "dsici_heads.json")
TAG, N, M = 0x40302, 128, 192


def jsonable(v):
    """bytes -> hex, tuples -> lists, through dicts and lists: the form the fixture stores and the test compares."""
    if isinstance(v, (bytes, bytearray, memoryview)):
        return bytes(v).hex()
    if isinstance(v, dict):
        return {k: jsonable(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [jsonable(x) for x in v]
    return v


def _bytes(seed, n):
    return bytes((seed * 37 + 11 * i) & 0xFF for i in range(n))


def _header(kind, C, H=64, W=64, batch=2, **more):
    h = {"numerics": TAG, "H": H, "W": W, "C": C, "kind": kind, "th": 32, "tw": 32, "N": N, "M": M, "in_ch": C,
         "spatial_params": 0, "batch": batch}
    h.update(more)
    return h


def _mask_block(fill):
    """2 x 2 tiles of 32 x 32: empty, full, mixed in mode 0 (the 128-byte plane), mixed in mode 1 (three positions)."""
    raw = _bytes(5, mask.raw_bytes(32, 32))
    pos = b"".join(p.to_bytes(2, "little") for p in (3, 40, 1000))
    return mask.pack_block(32, 32, fill, [0, 1, 2, 2], [(2, 0, len(raw)), (3, 1, len(pos))], [raw, pos])


def _res_tiles(C, n, seed):
    return [(-1 - t, bytes(2 * C * (2 + t)), [_bytes(seed + t + j, (j + t) % 4) for j in range(16)]) for t in range(n)]


def _wide_tiles(C, ks, seed):
    pb = residual16.plane_bytes(C, 32, 32)
    return [(-2 - t, bytes(2 * C * (3 + t)), k, _bytes(seed + t, k * pb),
             [_bytes(seed + t + j, (j + 2 * t) % 5) for j in range(16)]) for t, k in enumerate(ks)]


def _stream_cases():
    blobs4 = [_bytes(1, 5), _bytes(2, 9)]                              # 4 tiles in batches of 2
    blobs6 = [_bytes(3, 7), _bytes(4, 3)]                              # v3: a 64 x 80 image at overlap 16 has 6 tiles
    scale2 = [[0, 10000], [5, 5]]
    res = [residual.pack_block(3, 32, 32, 2, _res_tiles(3, 2, s)) for s in (1, 9)]
    wide = [residual16.pack_block(2, 32, 32, 300, _wide_tiles(2, ks, s)) for s, ks in ((1, (0, 1)), (9, (2, 0)))]
    yield "v1", _header(0, 3), blobs4, None, None
    yield "v2_k4", _header(1, 3, segments=4), blobs4, None, None
    yield "v3_k1", _header(0, 3, H=64, W=80, batch=4, segments=1, overlap=16), blobs6, None, None
    yield "v3_k2", _header(1, 3, H=64, W=80, batch=4, segments=2, overlap=16), blobs6, None, None
    yield "v4", _header(0, 3, segments=1, overlap=0, max_error=2), blobs4, res, None
    yield "v5", _header(0, 3, segments=2, nodata=255), blobs4, None, _mask_block(255)
    yield "v6_o0", _header(2, 2, segments=1, overlap=0, scale=scale2), blobs4, None, None
    yield "v6_o16", _header(2, 2, H=64, W=80, batch=4, segments=2, overlap=16, scale=scale2), blobs6, None, None
    yield "v8_kind0", _header(0, 3, segments=1, fill=7), blobs4, None, _mask_block(7)
    yield "v8_kind2", _header(2, 2, segments=4, fill=65535, scale=scale2), blobs4, None, _mask_block(65535)
    yield "v9", _header(2, 2, segments=1, scale=scale2, tolerance=300), blobs4, wide, None


def _block_case(layer, C, tau, tiles):
    block = layer.pack_block(C, 32, 32, tau, tiles)
    recs = layer.read_block_head(lambda o, c: block[o:o + c], 0, len(block), len(tiles), C, 32, 32, tau)
    return {"C": C, "th": 32, "tw": 32, "tau": tau, "tiles": jsonable(tiles), "block": block.hex(),
            "records": jsonable(recs)}


def main():
    streams = []
    for name, header, blobs, residuals, block in _stream_cases():
        stream = codec.pack_image_stream(header, blobs, residuals, block)
        streams.append({"name": name, "header": jsonable(header), "blobs": jsonable(blobs),
                        "residuals": jsonable(residuals), "mask": jsonable(block), "stream": stream.hex(),
                        "unpacked": jsonable(codec.unpack_image_stream(stream))})
    blocks = {"DSICR": _block_case(residual, 3, 2, _res_tiles(3, 2, 4)),
              "DSICW": _block_case(residual16, 3, 300, _wide_tiles(3, (0, 9), 4))}
    with open(OUT, "w") as f:
        json.dump({"streams": streams, "blocks": blocks}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
