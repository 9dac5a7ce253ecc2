"""NumPy restatement of the nodata masks of the whole-image codec (dsic_amd/mask.py, csrc/mask.hip): the tile states,
the m and d planes, the mode choice, the payloads, unpack, apply, and pack and parse of the mask block.  It shares no
code with the package; the kernels and the codec are held to it bit for bit.

A pixel of a uint8 [H,W,C] image is nodata iff all its channels equal v.  Tile t of the grid (row-major; origins
min(i*th, Hp - th), owned padded rows [i*th, min((i+1)*th, Hp)), columns likewise, Hp = ceil16(H)) has the mask m, a
[th][tw] bit plane in tile coordinates: 1 iff the pixel is owned, inside H x W and nodata.  d[y] = m[y] ^ m[y-1],
m[-1] = 0.  Bits are packed row-major, bit y*tw + x in byte (y*tw + x) / 8, LSB first."""
import struct

import numpy as np

EMPTY, FULL, MIXED = 0, 1, 2
MAGIC = b"DSICM\0"


def ceil16(n):
    return (n + 15) // 16 * 16


def axis(L, t):
    """[(origin, owned lo, owned hi)] of one axis, owned cut to the image"""
    Lp = ceil16(L)
    n = 1 if Lp <= t else -(-Lp // t)
    return [(min(i * t, Lp - t), i * t, min(min((i + 1) * t, Lp), L)) for i in range(n)]


def tiles(H, W, th, tw):
    """per tile (oy, ox, y0, y1, x0, x1): origin and owned rectangle inside H x W, image coordinates"""
    return [(oy, ox, y0, y1, x0, x1) for oy, y0, y1 in axis(H, th) for ox, x0, x1 in axis(W, tw)]


def nodata_mask(img, v):
    return (img == v).all(axis=2)


def m_plane(mask, tile, th, tw):
    """bool [th][tw]: the tile's mask in tile coordinates"""
    oy, ox, y0, y1, x0, x1 = tile
    m = np.zeros((th, tw), dtype=bool)
    m[y0 - oy:y1 - oy, x0 - ox:x1 - ox] = mask[y0:y1, x0:x1]
    return m


def tile_row(H, W, th, tw, i):
    """the tiles of tile row i, as tiles() lists them"""
    oy, y0, y1 = axis(H, th)[i]
    return [(oy, ox, y0, y1, x0, x1) for ox, x0, x1 in axis(W, tw)]


def counts_in(mask, rects):
    """per tile of rects (entries of tiles()) the set pixels of the mask among its owned pixels"""
    return [int(mask[y0:y1, x0:x1].sum()) for _, _, y0, y1, x0, x1 in rects]


def counts(mask, H, W, th, tw):
    return counts_in(mask, tiles(H, W, th, tw))


def states(mask, H, W, th, tw):
    out = []
    for c, (_, _, y0, y1, x0, x1) in zip(counts(mask, H, W, th, tw), tiles(H, W, th, tw)):
        out.append(EMPTY if c == (y1 - y0) * (x1 - x0) else (FULL if c == 0 else MIXED))
    return out


def delta(m):
    d = m.copy()
    d[1:] ^= m[:-1]
    return d


def undelta(d):
    return np.bitwise_xor.accumulate(d, axis=0)


def pack_bits(plane):
    return np.packbits(plane.ravel(), bitorder="little").tobytes()


def unpack_bits(buf, th, tw):
    return np.unpackbits(np.frombuffer(buf, dtype=np.uint8), bitorder="little")[:th * tw].reshape(th, tw).astype(bool)


def plane_dwords(plane):
    return np.frombuffer(pack_bits(plane), dtype="<u4")


def pos_dtype(th, tw):
    return "<u2" if th * tw <= 65536 else "<u4"


def payload(d):
    """(mode, bytes) of a d plane: the list of positions iff it is strictly shorter than the plane"""
    th, tw = d.shape
    pos = np.flatnonzero(d.ravel()).astype(pos_dtype(th, tw))
    return (1, pos.tobytes()) if pos.nbytes < th * tw // 8 else (0, pack_bits(d))


def unpack_payload(mode, buf, th, tw):
    """payload -> the m plane"""
    if mode == 0:
        d = unpack_bits(buf, th, tw)
    else:
        d = np.zeros(th * tw, dtype=bool)
        d[np.frombuffer(buf, dtype=pos_dtype(th, tw)).astype(np.int64)] = True
        d = d.reshape(th, tw)
    return undelta(d)


def apply(win, window, H, W, th, tw, desc, planes, v):
    """win: uint8 [h][w][C] or float32 [C][h][w], the window (y0, x0, h, w) of the image; desc: (tile, plane index or
    -1 for all set); planes: m planes, bool [th][tw].  Returns a copy with v (v / 255 in float32) at the tiles' owned
    pixels inside the window whose bit is set.  A tile outside the grid writes nothing."""
    out = win.copy()
    wy, wx, wh, ww = window
    grid = tiles(H, W, th, tw)
    for t, pi in desc:
        if not 0 <= t < len(grid):
            continue
        oy, ox, y0, y1, x0, x1 = grid[t]
        a, b, c, d = max(y0, wy), min(y1, wy + wh), max(x0, wx), min(x1, wx + ww)
        if a >= b or c >= d:
            continue
        sel = np.ones((b - a, d - c), dtype=bool) if pi < 0 else planes[pi][a - oy:b - oy, c - ox:d - ox]
        if out.dtype == np.uint8:
            out[a - wy:b - wy, c - wx:d - wx][sel] = v
        else:
            out[:, a - wy:b - wy, c - wx:d - wx][:, sel] = np.float32(v) / np.float32(255)
    return out


def block(img, v, th, tw):
    """the mask block of an image, and its states"""
    H, W, _ = img.shape
    mask = nodata_mask(img, v)
    st = states(mask, H, W, th, tw)
    grid = tiles(H, W, th, tw)
    recs, bodies = [], []
    for t, s in enumerate(st):
        if s == MIXED:
            mode, body = payload(delta(m_plane(mask, grid[t], th, tw)))
            recs.append(struct.pack("<3I", t, mode, len(body)))
            bodies.append(body)
    n = len(st)
    return (b"".join([MAGIC, struct.pack("<5I", n, th, tw, v, len(recs)), bytes(st), b"\0" * (-n % 4)] + recs + bodies),
            st)


def parse_block(buf):
    """block -> (n, th, tw, v, states, {tile: (mode, payload)})"""
    assert buf[:6] == MAGIC
    n, th, tw, v, nm = struct.unpack_from("<5I", buf, 6)
    st = list(buf[26:26 + n])
    off = 26 + n + (-n % 4)
    recs = [struct.unpack_from("<3I", buf, off + 12 * i) for i in range(nm)]
    off += 12 * nm
    out = {}
    for t, mode, length in recs:
        out[t] = (mode, buf[off:off + length])
        off += length
    assert off == len(buf)
    return n, th, tw, v, st, out
