"""NumPy restatement of the zonal statistics (csrc/zonal.hip, codec.ImageReader.zonal_stats, codec.SceneStack.zonal_stats),
written from the definition in include/dsic_hip.h as a plain loop over the zones with masks; the input makers and the
case sweep of the kernel tests.  No tests here: test_per_zone_cpu.py holds the restatement to an independent formulation
and to index_ref, test_gpu_per_zone.py holds the kernel, the reader, the stack and the tool to it.

  a pixel counts:   zones[p] < Z, its validity byte is not 0, its C channels do not all equal nodata, its index is defined
  its values:       of = None: K = C, v = px[k], u = v;  of = an index: K = 1, u as index_ref.index_value, v = u + vmin
  table [Z][K][5]:  [0] += n   [1] += sum v   [2] += sum v^2   [3] = min([3], min v)   [4] = max([4], max v)
                    as 64-bit words: 1, 3 and 4 two's complement; a fresh table is (0, 0, 0, INT64_MAX, INT64_MIN)
  hist [Z][K][256]: hist[z][k][stretch(u, lo, hi)] += 1 per counted pixel, (lo, hi) per value in u units"""
import numpy as np

import index_ref
from dsic_amd import lib

WORDS = 5
MASK = (1 << 64) - 1
I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)


def n_values(C, of):
    return C if of is None else 1


def lds_zones(K):
    """the largest Z whose table of K values per zone is gathered in LDS"""
    return lib.ZONAL_LDS_BYTES // (8 * WORDS * K)


def fresh(Z, K):
    """a table before its first call: uint64 [Z][K][5]"""
    t = np.zeros((Z, K, WORDS), dtype=np.uint64)
    t[:, :, 3] = np.uint64(I64_MAX)
    t[:, :, 4] = np.uint64(I64_MIN & MASK)
    return t


def signed(word):
    word = int(word)
    return word - (1 << 64) if word >> 63 else word


def values(img, of):
    """img uint8 / uint16 [H][W][C] -> (v int64 [H][W][K], u int64 [H][W][K], defined bool [H][W])"""
    if of is None:
        v = img.astype(np.int64)
        return v, v, np.ones(img.shape[:2], dtype=bool)
    kind, a, b = index_ref.parse(of)
    u, defined = index_ref.index_value(img, kind, a, b)
    vmin = index_ref.value_range(kind, index_ref.top_of(img))[0]
    return (u + vmin)[:, :, None], u[:, :, None], defined


def counted(img, valid, nodata, defined):
    ok = defined.copy()
    if valid is not None:
        ok &= np.asarray(valid) != 0
    if nodata is not None:
        ok &= ~(img == nodata).all(axis=2)
    return ok


def zonal(img, valid, nodata, zones, Z, of=None, table=None, pairs=None, hist=None):
    """One call: (table, hist) after it, from `table` and `hist` before it (None: fresh, zeros); the arguments are left
    unchanged.  pairs: None, or one (lo, hi) in u units per value, and then hist uint32 [Z][K][256] is counted too."""
    H, W, C = img.shape
    K = n_values(C, of)
    assert zones.shape == (H, W) and zones.dtype == np.uint16 and 1 <= Z <= 65535
    table = fresh(Z, K) if table is None else table.copy()
    if pairs is not None:
        hist = np.zeros((Z, K, 256), dtype=np.uint32) if hist is None else hist.copy()
    v, u, defined = values(img, of)
    ok = counted(img, valid, nodata, defined)
    present = np.zeros(65536, dtype=bool)
    present[zones[ok]] = True
    for z in np.flatnonzero(present[:Z]):                        # an id at or above Z belongs to no zone
        m = ok & (zones == z)
        for k in range(K):
            vz = v[:, :, k][m]                                 # int64; |v| <= 65535 and under 2^32 of them:
            n, s = vz.size, int(vz.sum(dtype=np.int64))        # the sum is exact in int64,
            q = int((vz * vz).astype(np.uint64).sum(dtype=np.uint64))      # the sum of squares in uint64
            rec = table[z, k]
            rec[0] = (int(rec[0]) + n) & MASK
            rec[1] = (int(rec[1]) + s) & MASK
            rec[2] = (int(rec[2]) + q) & MASK
            rec[3] = min(signed(rec[3]), int(vz.min())) & MASK
            rec[4] = max(signed(rec[4]), int(vz.max())) & MASK
            if pairs is not None:
                np.add.at(hist[z, k], index_ref.stretch(u[:, :, k][m], *pairs[k]), 1)
    return table, hist


def result(table, hist=None):
    """what codec.zonal_table makes of a table, restated with Python's integers and fractions.Fraction-free floats"""
    import math
    Z, K, _ = table.shape
    out = {key: np.zeros((Z, K), dtype=np.int64) for key in ("count", "sum", "min", "max")}
    out["sumsq"] = np.zeros((Z, K), dtype=np.uint64)
    out["mean"], out["std"] = np.full((Z, K), np.nan), np.full((Z, K), np.nan)
    for z in range(Z):
        for k in range(K):
            n, s, q = int(table[z, k, 0]), signed(table[z, k, 1]), int(table[z, k, 2])
            out["count"][z, k], out["sum"][z, k], out["sumsq"][z, k] = n, s, q
            if n:
                out["min"][z, k], out["max"][z, k] = signed(table[z, k, 3]), signed(table[z, k, 4])
                out["mean"][z, k], out["std"][z, k] = s / n, math.sqrt((n * q - s * s) / (n * n))
    if hist is not None:
        out["hist"] = hist.astype(np.int64)
    return out


# ---- inputs ---------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (1, 63), (3, 65), (37, 129), (750, 701)]     # the last: more than 2048 x 256 pixels, a second trip
KINDS = [("u8", 1), ("u8", 3), ("u8", 4), ("u16", 1), ("u16", 3), ("u16", 4)]
WHATS = ["bands", "band", "difference", "nd"]
MASKS = ["valid", "nodata", "none", "nothing"]                  # nothing: a validity plane of zeros
RASTERS = ["one", "stripes", "checker", "blocks", "noise", "noise_holes"]
ZSEL = ["one", "lds", "over", "max"]                            # Z = 1, the LDS limit, one above it, 65535
NODATA = {"u8": 7, "u16": 300}
_MADE = {}


def image(kind, C, H, W):
    """Random pixels with a block of zeros (A + B = 0), a block of nodata, a block at the top of the range (two uint16
    pixels of 65535 already bring a zone's sum of squares past 2^32) and smooth rows, read-only."""
    key = ("image", kind, C, H, W)
    if key not in _MADE:
        rng = np.random.default_rng(H * 100003 + W * 101 + C + (7 if kind == "u16" else 0))
        top = 255 if kind == "u8" else 65535
        img = rng.integers(0, top + 1, size=(H, W, C)).astype(np.uint8 if kind == "u8" else np.uint16)
        img[H // 2:, :max(1, W // 3)] = 0
        img[:max(1, H // 4), W // 2:W // 2 + max(1, W // 5)] = NODATA[kind]
        img[H // 4:H // 2, :max(1, W // 4)] = top
        if H >= 3:
            img[-1] = (np.arange(W)[:, None] // 9 + np.arange(C)[None, :]) % (top + 1)
        img.setflags(write=False)
        _MADE[key] = img
    return _MADE[key]


def validity(H, W, mask, seed=0):
    if mask == "nothing":
        return np.zeros((H, W), dtype=np.uint8)
    if mask != "valid":
        return None
    rng = np.random.default_rng(H * 31 + W + seed)
    v = (rng.random((H, W)) < 0.7).astype(np.uint8) * rng.integers(1, 256, (H, W), dtype=np.uint8)
    v[:max(1, H // 5), :max(1, W // 5)] = 0
    return v


def raster(name, H, W, Z, seed=0):
    """uint16 [H][W]: at most min(Z, 4096) ids (40 on the large shape, which keeps the restatement's loop short), spread
    over 0 .. Z - 1 with the last zone among them.  noise_holes replaces some pixels by 65535 and by ids from Z upwards."""
    D = min(Z, 40 if H * W > 100000 else 4096)
    y, x = np.mgrid[0:H, 0:W]
    rng = np.random.default_rng(H * 7 + W * 13 + Z + seed)
    if name == "one":
        t = np.full((H, W), D - 1)
    elif name == "stripes":                                    # 5 wide: boundaries inside a wave
        t = (x // 5) % D
    elif name == "checker":                                    # every lane its own run
        t = (x + y) % min(D, 2) + (D - min(D, 2))
    elif name == "blocks":
        t = ((y // 16) * ((W + 15) // 16) + x // 16) % D
    else:
        t = rng.integers(0, D, (H, W))
    step = (Z - 1) // (D - 1) if D > 1 else 1
    ids = (t * step).astype(np.uint16)
    if D > 1:
        ids[t == D - 1] = Z - 1
    if name == "noise_holes":
        holes = rng.random((H, W))
        ids[holes < 0.1] = 65535
        over = holes > 0.9
        ids[over] = np.minimum(Z + rng.integers(0, 4, (H, W)), 65535).astype(np.uint16)[over]
    return ids


def index_of(what, C):
    """the `of` of a case: None for the bands, else an index over bands C - 1 and 0"""
    return None if what == "bands" else ("band", C - 1) if what == "band" else (what, C - 1, 0)


def what_code(of):
    """(what, a, b) as the export takes them"""
    if of is None:
        return lib.ZONAL_BANDS, 0, 0
    kind, a, b = index_ref.parse(of)
    return index_ref.KINDS[kind], a, b


def u_top(kind, of):
    """the largest u of a value"""
    top = 255 if kind == "u8" else 65535
    if of is None:
        return top
    vmin, vmax = index_ref.value_range(of[0], top)
    return vmax - vmin


def sweep(si, ki, r):
    """shape si, kind ki, raster r -> (what, mask, which Z, with a histogram): every value of every axis is taken, and
    every raster meets every `what`, every mask and every Z"""
    return WHATS[(si + ki + r) % 4], MASKS[(si + 2 * ki + r) % 4], ZSEL[(si + ki + 2 * r + r // 2) % 4], (si + ki + r) % 3 == 0


def zone_count(zsel, K):
    return {"one": 1, "lds": lds_zones(K), "over": lds_zones(K) + 1, "max": 65535}[zsel]


def case(si, ki, r):
    """the inputs and the restated outputs of one case of the sweep, made once"""
    key = ("case", si, ki, r)
    if key not in _MADE:
        (H, W), (kind, C) = SHAPES[si], KINDS[ki]
        what, mask, zsel, with_hist = sweep(si, ki, r)
        of = index_of(what, C)
        K = n_values(C, of)
        Z = zone_count(zsel, K)
        with_hist = with_hist and (zsel != "max" or K == 1)      # 65535 zones of one value: 64 MB of bins; of four: 256 MB
        img, val = image(kind, C, H, W), validity(H, W, mask, seed=r)
        nodata = NODATA[kind] if mask == "nodata" else None
        zones = raster(RASTERS[r], H, W, Z, seed=si + ki)
        top = u_top(kind, of)
        pairs = [(0, top), (top // 7, top - top // 5), (top // 2, top // 2), (3, top)][:K] if with_hist else None
        table, hist = zonal(img, val, nodata, zones, Z, of, pairs=pairs)
        if hist is not None:                                     # kept as its non-zero bins: (flat positions, counts)
            at = np.flatnonzero(hist)
            hist = (at, hist.ravel()[at])
        _MADE[key] = dict(kind=kind, C=C, H=H, W=W, of=of, K=K, Z=Z, img=img, valid=val, nodata=nodata, zones=zones,
                          pairs=pairs, table=table, hist=hist,
                          what=f"{kind} {H}x{W} C={C} {what} {mask} {RASTERS[r]} Z={Z} ({zsel}){' hist' if with_hist else ''}")
    return _MADE[key]
