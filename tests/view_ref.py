"""NumPy restatement of the resampled reads (csrc/view.hip, codec.ImageReader): the three resamplers, view_level, and
a model of the reader's tile cache.  No tests here; test_view_cpu.py holds the restatement to its own properties and
to float64, test_gpu_view.py holds the kernels and the reader to it.

A region (y0, x0, h, w) of level 0 is resampled to oh x ow from a window of level l (`shift`) whose first pixel is
that level's pixel (sy0, sx0).  On the row axis, scaled by oh, output row i covers [i h, (i+1) h) and level row Y
covers [(Y << l) oh - y0 oh, ((Y+1) << l) oh - y0 oh); wy(i, Y) is the length they share.  Columns likewise.
  average, uint8 / uint16 [sh,sw,C]: S = sum wy wx v, T = sum wy wx in int64, output (2 S + T) // (2 T)
  average, float32 [C,sh,sw]:        the float32 left fold over Y, then X, of float32(wy wx) * v, over float32(T)
  nodata: a source pixel whose channels all equal the value stays out of S and T; T = 0 gives the value
  nearest: level row (y0 2 oh + (2 i + 1) h) // (2 oh) >> l, columns likewise"""
import numpy as np


def view_level(n_levels, h, w, oh, ow):
    """the largest l < n_levels with (oh << l) <= h and (ow << l) <= w, else 0"""
    fit = [l for l in range(n_levels) if (oh << l) <= h and (ow << l) <= w]
    return max(fit) if fit else 0


def level_window(l, y0, x0, h, w):
    ya, xa = y0 >> l, x0 >> l
    return ya, xa, ((y0 + h - 1) >> l) - ya + 1, ((x0 + w - 1) >> l) - xa + 1


def axis_weights(o, length, n, l):
    """per output index i of n: [(Y, weight)], Y the indices of level l with a positive weight, ascending"""
    out = []
    for i in range(n):
        lo, hi = i * length, (i + 1) * length
        row = []
        Y = (o + lo // n) >> l
        while True:
            a = (Y << l) * n - o * n
            b = a + (n << l)
            if a >= hi:
                break
            wgt = min(b, hi) - max(a, lo)
            assert wgt > 0
            row.append((Y, wgt))
            Y += 1
        out.append(row)
    return out


def nearest_index(o, length, n, l):
    return [((o * 2 * n + (2 * i + 1) * length) // (2 * n)) >> l for i in range(n)]


def _pixel(src, hwc, Y, X):
    return src[Y, X, :] if hwc else src[:, Y, X]


def resample(src, sy0, sx0, shift, region, size, mode="average", nodata=None, fold="f32"):
    """src: uint8 / uint16 [sh,sw,C] or float32 [C,sh,sw].  fold (float32 average only): "f32" the kernel's fold,
    "f64" the weighted mean in float64 (returned as float64)."""
    y0, x0, h, w = region
    oh, ow = size
    hwc = src.dtype != np.float32
    C = src.shape[2] if hwc else src.shape[0]
    wide = (not hwc) and mode == "average" and fold == "f64"
    out = np.zeros((oh, ow, C) if hwc else (C, oh, ow), dtype=np.float64 if wide else src.dtype)

    def put(i, j, vals):
        if hwc:
            out[i, j, :] = vals
        else:
            out[:, i, j] = vals

    if mode == "nearest":
        ys, xs = nearest_index(y0, h, oh, shift), nearest_index(x0, w, ow, shift)
        for i, Y in enumerate(ys):
            for j, X in enumerate(xs):
                put(i, j, _pixel(src, hwc, Y - sy0, X - sx0))
        return out
    assert mode == "average"
    rows, cols = axis_weights(y0, h, oh, shift), axis_weights(x0, w, ow, shift)
    nd = None if nodata is None else src.dtype.type(nodata)
    assert 2 * 65535 * h * w < 2 ** 63                                       # int64 holds 2 S + T
    acc_t = np.int64 if hwc else (np.float64 if wide else np.float32)
    for i, row in enumerate(rows):
        for j, col in enumerate(cols):
            T, S = 0, np.zeros(C, dtype=acc_t)
            for Y, wy in row:
                for X, wx in col:
                    px = _pixel(src, hwc, Y - sy0, X - sx0)
                    if nd is not None and bool((px == nd).all()):
                        continue
                    wgt = wy * wx
                    T += wgt
                    if hwc or wide:
                        S = S + acc_t(wgt) * px.astype(acc_t)
                    else:
                        S = S + np.float32(wgt) * px                         # two float32 roundings per term
                        assert S.dtype == np.float32
            if T == 0:
                put(i, j, nd)
            elif hwc:
                put(i, j, (2 * S + T) // (2 * T))
            elif wide:
                put(i, j, S / T)
            else:
                put(i, j, S / np.float32(T))
    return out


def footprint(region, size, shift):
    """K: the number of source pixels in the largest footprint of an output pixel"""
    y0, x0, h, w = region
    return (max(len(r) for r in axis_weights(y0, h, size[0], shift)) *
            max(len(r) for r in axis_weights(x0, w, size[1], shift)))


class LRU:
    """The reader's tile cache as a model: keys (level, tile), `cost(key)` bytes each, `capacity` bytes in all.
    call(keys) is one read (keys ascending): a call whose keys cost more than the capacity is decoded beside the
    cache and leaves it alone; otherwise the keys held become the most recently used in order, then each missing key
    is stored after the least recently used keys that the call does not need have been evicted to make room.
    Returns (hits, decoded) of the call."""

    def __init__(self, capacity, cost=lambda key: 1):
        self.capacity, self.cost, self.order = capacity, cost, []            # order: oldest first

    def call(self, keys):
        keys = list(keys)
        if sum(self.cost(k) for k in keys) > self.capacity:
            return 0, len(keys)
        held = [k for k in keys if k in self.order]
        missing = [k for k in keys if k not in self.order]
        for k in held:
            self.order.remove(k)
            self.order.append(k)
        for k in missing:
            while sum(self.cost(q) for q in self.order) + self.cost(k) > self.capacity:
                self.order.remove(next(q for q in self.order if q not in keys))
            self.order.append(k)
        return len(held), len(missing)


# ---- the kernel sweep of test_gpu_view.py; test_view_cpu.py asserts the float32 fold bound on these very inputs ------
SIZES = [((1, 1), (1, 1)), ((2, 2), (1, 1)), ((3, 5), (2, 3)), ((17, 33), (5, 7)), ((64, 36), (64, 36)),
         ((5, 7), (17, 33)), ((70, 1030), (9, 129)), ((33, 35), (16, 17))]
SHIFTS = (0, 1, 2)
KINDS = [("u8", 3), ("u8", 4), ("u16", 1), ("u16", 2), ("u16", 3), ("u16", 4), ("f32", 1), ("f32", 3), ("f32", 4)]
NODATA = {"u8": 7, "u16": 7, "f32": 0.5}
DTYPES = {"u8": np.uint8, "u16": np.uint16, "f32": np.float32}


def _axis_case(c, l):
    """An axis whose covering window has c pixels of level l, begins at level pixel 2 l + 1 and, for l > 0, at a
    level-0 origin that is no multiple of 2^l: (source origin, source length, region origin, region length); the
    source window is l pixels longer than the covering one at its start and 2 l at its end."""
    first = 2 * l + 1 if l else 0
    a = 1 if l else 0
    length = (c << l) - a
    if l and length > 1:
        length -= 1
    o = (first << l) + a
    assert (o >> l, (o + length - 1) >> l) == (first, first + c - 1)
    return first - l, c + 3 * l, o, length


def kernel_case(src_size, out_size, shift):
    sy0, sh, y0, h = _axis_case(src_size[0], shift)
    sx0, sw, x0, w = _axis_case(src_size[1], shift)
    return {"sy0": sy0, "sx0": sx0, "sh": sh, "sw": sw, "shift": shift, "region": (y0, x0, h, w), "size": out_size}


def kernel_image(kind, C, sh, sw):
    """Random values with, where there is room, a block of nodata pixels over the top-left quarter and single ones
    elsewhere, blocks of 0 and of the largest value, and for float32 (values in [0, 1]) -0.0 and denormals."""
    rng = np.random.default_rng(sh * 100003 + sw * 101 + C + len(kind))
    hwc = kind != "f32"
    if hwc:
        top = 255 if kind == "u8" else 65535
        img = rng.integers(0, top + 1, size=(sh, sw, C)).astype(DTYPES[kind])
        px = img
    else:
        top = 1.0
        img = rng.random((C, sh, sw), dtype=np.float32)
        px = img.transpose(1, 2, 0)                                           # a view: [sh, sw, C]
    px[rng.random((sh, sw)) < 0.1] = NODATA[kind]
    px[:max(1, sh // 2), :max(1, sw // 2)] = NODATA[kind]
    if sh >= 4 and sw >= 4:
        px[-2:, -2:] = top
        px[-2:, :2] = 0
    if not hwc and sw >= 8:
        px[-1, 2:4] = -0.0
        px[-1, 4:6] = np.float32(1e-45) * np.array([[1], [3]], dtype=np.float32)
    return img
