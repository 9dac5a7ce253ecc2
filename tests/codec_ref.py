"""NumPy restatements of the image codec's byte movers, for the mover tests (no tests here, nothing of dsic_amd).

Tile grid (per axis, L pixels, P = ceil16(L), tile side t <= P): n = ceil(P / t) tiles, origin of tile i = min(i*t,
P - t), tile i owns padded positions [i*t, min((i+1)*t, P)); tiles are numbered row-major.  Padding reflects at the
bottom and right without repeating the edge: padded position p >= L reads 2*(L-1) - p.

gather: uint8 [H][W][C] -> [n][th][tw][C]; float32 [C][H][W] -> [n][C][th][tw].
stitch: tile k of the call is grid tile ids[k]; it writes the pixels it owns that lie in the image and in the window,
as clamp(x, 0, 1) (float32 [C][h][w]) or as the truncated float32 product clamp(x, 0, 1) * 255 (uint8 [h][w][C]).
clamp(x, 0, 1) is x < 0 ? 0 : (x > 1 ? 1 : x), which keeps -0.0.

Container (little endian): magic "DSIC2\\0" | tag u32 | B, My, Hy, Wy, Nz, Hz, Wz u32 | B x (min_y, max_y, min_z,
max_z i32, len_z, len_y u32) | B x (z string, y string).  K > 1 segments per y string: magic "DSIC3\\0", a segs u32
behind the head, len_y = the sum of the image's segments, B x K u32 segment lengths behind the records, and per image
the z string, then the K segments.  The packer takes meta [B][4] = (min_y, L_y, min_z, L_z) with max = min + L - 1 and
clamps every length to [0, capacity] first.

scatter (DSIC2): string s (z0, y0, z1, ...) lies at 38 + 24 B + the sum of the recorded lengths in front of it, read
as u32; lengths [B][2] is the recorded value as int32; the copy is cut to [0, stride], then to what the blob holds
behind the offset, and an offset past the blob moves nothing.  scatter_select: descriptors [n][4] = (z offset, z
length, y offset, y length); a length is cut to [0, stride] and to blob_bytes - offset, an offset outside
[0, blob_bytes] moves nothing, and lengths [n][2] holds the bytes moved.
"""
import struct

import numpy as np

HEAD_BYTES, REC_BYTES = 38, 24


def ceil16(n):
    return (n + 15) // 16 * 16


def _axis(L, t):
    P = ceil16(L)
    n = -(-P // t)
    return P, [min(i * t, P - t) for i in range(n)], [(i * t, min((i + 1) * t, P)) for i in range(n)]


def grid(H, W, th, tw):
    """dict Hp, Wp, th, tw, ny, nx, n, ys, xs (origins), own_y, own_x (owned ranges [a, b))."""
    Hp, ys, own_y = _axis(H, th)
    Wp, xs, own_x = _axis(W, tw)
    return {"H": H, "W": W, "Hp": Hp, "Wp": Wp, "th": th, "tw": tw, "ny": len(ys), "nx": len(xs),
            "n": len(ys) * len(xs), "ys": ys, "xs": xs, "own_y": own_y, "own_x": own_x}


def _reflect(L, P):
    p = np.arange(P)
    return np.where(p < L, p, 2 * (L - 1) - p)


def _origins(H, W, th, tw, overlap):
    """(row origins, column origins) of the tiles; with an overlap they are blend_ref.axis' (the grid of the seams)"""
    if not overlap:
        g = grid(H, W, th, tw)
        return g["ys"], g["xs"]
    import blend_ref
    ay, ax = blend_ref.axis(H, th, overlap), blend_ref.axis(W, tw, overlap)
    assert ay["t"] == th and ax["t"] == tw
    return ay["o"], ax["o"]


def gather_u8(img_hwc, th, tw, overlap=0):
    H, W = img_hwc.shape[:2]
    ys, xs = _origins(H, W, th, tw, overlap)
    ry, rx = _reflect(H, ceil16(H)), _reflect(W, ceil16(W))
    return np.stack([img_hwc[ry[y:y + th]][:, rx[x:x + tw]] for y in ys for x in xs])


def gather_f32(img_chw, th, tw, overlap=0):
    H, W = img_chw.shape[1:]
    ys, xs = _origins(H, W, th, tw, overlap)
    ry, rx = _reflect(H, ceil16(H)), _reflect(W, ceil16(W))
    return np.stack([img_chw[:, ry[y:y + th]][:, :, rx[x:x + tw]] for y in ys for x in xs])


def clamp01(x):
    x = np.asarray(x, dtype=np.float32)
    return np.where(x < 0, np.float32(0), np.where(x > 1, np.float32(1), x)).astype(np.float32)


def to_u8(x):
    """(uint8)(clamp(x, 0, 1) * 255): one float32 multiply, truncated."""
    return (clamp01(x) * np.float32(255)).astype(np.uint8)


def stitch(tiles, ids, H, W, th, tw, window, kind, fill):
    """tiles float32 [len(ids)][C][th][tw]; window (y0, x0, h, w); kind "f32" -> [C][h][w], "u8" -> [h][w][C].
    A pixel no tile of ids owns keeps fill; ids outside the grid write nothing."""
    g = grid(H, W, th, tw)
    C = tiles.shape[1]
    wy, wx, wh, ww = window
    out = np.full((C, wh, ww), fill, dtype=np.float32 if kind == "f32" else np.uint8)
    for k, t in enumerate(ids):
        if t < 0 or t >= g["n"]:
            continue
        i, j = divmod(t, g["nx"])
        y0, y1 = max(g["own_y"][i][0], wy), min(g["own_y"][i][1], H, wy + wh)
        x0, x1 = max(g["own_x"][j][0], wx), min(g["own_x"][j][1], W, wx + ww)
        if y0 >= y1 or x0 >= x1:
            continue
        oy, ox = g["ys"][i], g["xs"][j]
        src = tiles[k][:, y0 - oy:y1 - oy, x0 - ox:x1 - ox]
        out[:, y0 - wy:y1 - wy, x0 - wx:x1 - wx] = clamp01(src) if kind == "f32" else to_u8(src)
    return out if kind == "f32" else np.ascontiguousarray(out.transpose(1, 2, 0))


def _u32(v):
    return int(v) & 0xFFFFFFFF


def pack_container(rows, lengths, meta, tag, My, Hy, Wy, Nz, Hz, Wz, cap_z, cap_y, K):
    """rows uint8 [B][cap_z + K*cap_y], lengths [B][1 + K] (z, then the K segments), meta [B][4].  Returns (the
    container's bytes, its size, the exclusive offsets of the B (1 + K) strings behind the head and the total behind
    them: B (1 + K) + 1 numbers)."""
    rows = np.asarray(rows, dtype=np.uint8)
    B = rows.shape[0]
    S = 1 + K
    lens = [[min(max(int(v), 0), cap_y if j else cap_z) for j, v in enumerate(row)] for row in np.asarray(lengths)]
    head = [b"DSIC3\x00" if K > 1 else b"DSIC2\x00", struct.pack("<8I", _u32(tag), B, My, Hy, Wy, Nz, Hz, Wz)]
    if K > 1:
        head.append(struct.pack("<I", K))
    for b in range(B):
        m = [int(v) for v in meta[b]]
        head.append(struct.pack("<6I", _u32(m[0]), _u32(m[0] + m[1] - 1), _u32(m[2]), _u32(m[2] + m[3] - 1),
                                lens[b][0], _u32(sum(lens[b][1:]))))
    if K > 1:
        head.append(struct.pack(f"<{B * K}I", *[v for row in lens for v in row[1:]]))
    body, offsets, pos = [], [], 0
    for b in range(B):
        for j in range(S):
            start = 0 if j == 0 else cap_z + (j - 1) * cap_y
            body.append(rows[b, start:start + lens[b][j]].tobytes())
            offsets.append(pos)
            pos += lens[b][j]
    offsets.append(pos)
    blob = b"".join(head + body)
    assert len(blob) == HEAD_BYTES + (4 if K > 1 else 0) + REC_BYTES * B + (4 * B * K if K > 1 else 0) + pos
    return blob, len(blob), offsets


def _move(row, blob, off, n):
    if n > 0:
        row[:n] = blob[off:off + n]


def scatter(blob, blob_bytes, B, zstride, ystride, fill):
    """blob uint8 array holding a DSIC2 container of blob_bytes bytes.  Returns (z rows [B][zstride], y rows
    [B][ystride], lengths int32 [B][2], meta int32 [B][4] = (min_y, L_y, min_z, L_z))."""
    blob = np.asarray(blob, dtype=np.uint8)
    z = np.full((B, zstride), fill, dtype=np.uint8)
    y = np.full((B, ystride), fill, dtype=np.uint8)
    rec = blob[HEAD_BYTES:HEAD_BYTES + REC_BYTES * B].copy().view("<i4").reshape(B, 6).astype(np.int64)
    meta = np.stack([rec[:, 0], rec[:, 1] - rec[:, 0] + 1, rec[:, 2], rec[:, 3] - rec[:, 2] + 1], axis=1)
    meta = ((meta + 2 ** 31) % 2 ** 32 - 2 ** 31).astype(np.int32)            # int32 arithmetic wraps
    lengths = rec[:, 4:6].astype(np.int32)
    off = HEAD_BYTES + REC_BYTES * B
    for b in range(B):
        for which, (rows, stride) in enumerate(((z, zstride), (y, ystride))):
            n = min(max(int(lengths[b, which]), 0), stride)
            if off + n > blob_bytes:
                n = blob_bytes - off
            _move(rows[b], blob, off, n)
            off += _u32(lengths[b, which])
    return z, y, lengths, meta


def scatter_select(blob, blob_bytes, desc, zstride, ystride, fill):
    """desc int64 [n][4].  Returns (z rows, y rows, lengths int32 [n][2] = the bytes moved)."""
    blob = np.asarray(blob, dtype=np.uint8)
    desc = np.asarray(desc, dtype=np.int64).reshape(-1, 4)
    n_t = desc.shape[0]
    z = np.full((n_t, zstride), fill, dtype=np.uint8)
    y = np.full((n_t, ystride), fill, dtype=np.uint8)
    lengths = np.zeros((n_t, 2), dtype=np.int32)
    for b in range(n_t):
        for which, (rows, stride) in enumerate(((z, zstride), (y, ystride))):
            off, ln = int(desc[b, 2 * which]), int(desc[b, 2 * which + 1])
            n = min(max(ln, 0), stride)
            if off < 0 or off > blob_bytes:
                n = 0
            else:
                n = min(n, blob_bytes - off)
            lengths[b, which] = n
            _move(rows[b], blob, off, n)
    return z, y, lengths
