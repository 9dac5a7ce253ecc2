"""The NumPy restatement of dsic_window_composite_u8 / _u16 (include/dsic_hip.h), written from the definition with a
plain loop over the sources and np.sort, and the inputs the composite tests share: ladder and random validity, the rect
layouts, and the thinned sweep of test_gpu_composite.py (kept here so that a test without a GPU can hold it)."""
import numpy as np

FIRST, LAST, MEAN, MEDIAN = 0, 1, 2, 3
MODES = {"first": FIRST, "last": LAST, "mean": MEAN, "median": MEDIAN}
TOP = {"u8": 255, "u16": 65535}
DTYPES = {"u8": np.uint8, "u16": np.uint16}


def composite(srcs, valids, rects, nodata, C, oh, ow, mode, fill):
    """srcs[i]: [h_i][w_i][C]; valids[i]: None or [h_i][w_i], 0 = invalid; rects[i] = (dy, dx, h, w); nodata[i]: -1 or a
    value -> (dst [oh][ow][C] of the sources' dtype, valid uint8 [oh][ow], count uint8 [oh][ow])"""
    n = len(srcs)
    assert n == len(valids) == len(rects) == len(nodata) and n >= 1
    vals = np.zeros((n, oh, ow, C), dtype=np.int64)
    cand = np.zeros((n, oh, ow), dtype=bool)
    for i in range(n):
        dy, dx, h, w = rects[i]
        assert h >= 1 and w >= 1 and dy >= 0 and dx >= 0 and dy + h <= oh and dx + w <= ow
        px = np.asarray(srcs[i]).reshape(h, w, C).astype(np.int64)
        ok = np.ones((h, w), dtype=bool) if valids[i] is None else np.asarray(valids[i]).reshape(h, w) != 0
        if nodata[i] >= 0:
            ok = ok & ~(px == nodata[i]).all(axis=2)
        vals[i, dy:dy + h, dx:dx + w] = px
        cand[i, dy:dy + h, dx:dx + w] = ok
    k = cand.sum(axis=0)
    dst = np.full((oh, ow, C), fill, dtype=np.int64)
    if mode in (FIRST, LAST):
        taken = np.zeros((oh, ow), dtype=bool)
        for i in (range(n) if mode == FIRST else range(n - 1, -1, -1)):
            pick = cand[i] & ~taken
            dst[pick] = vals[i][pick]
            taken |= pick
    elif mode == MEAN:
        S = (vals * cand[..., None]).sum(axis=0)
        kk = np.maximum(k, 1)[..., None]
        dst = np.where(k[..., None] > 0, (2 * S + kk) // (2 * kk), dst)
    elif mode == MEDIAN:
        v = np.sort(np.where(cand[..., None], vals, 1 << 40), axis=0)      # the candidates first, ascending
        kk = np.maximum(k, 1)[None, ..., None]
        at = lambda idx: np.take_along_axis(v, np.broadcast_to(idx, (1, oh, ow, C)), axis=0)[0]
        odd = at((kk - 1) // 2)
        even = (at(np.maximum(kk // 2 - 1, 0)) + at(kk // 2) + 1) >> 1
        dst = np.where(k[..., None] == 0, dst, np.where(k[..., None] % 2 == 1, odd, even))
    else:
        raise ValueError(mode)
    return dst.astype(np.asarray(srcs[0]).dtype), (k > 0).astype(np.uint8), k.astype(np.uint8)


# ---- inputs ---------------------------------------------------------------------------------------------------------
def ladder_validity(n, oh, ow):
    """n masks [oh][ow] over the whole output: with q = y ow + x the count at q is q mod (n + 1), and source i is valid
    iff ((i + q // (n + 1)) mod n) < that count, so every count 0 .. n occurs once oh ow >= (n + 1) n and the sources
    that make up a count rotate"""
    q = np.arange(oh * ow, dtype=np.int64).reshape(oh, ow)
    target, turn = q % (n + 1), q // (n + 1)
    return [(((i + turn) % n) < target).astype(np.uint8) * np.uint8(1 + (37 * i) % 255) for i in range(n)]


def random_validity(n, oh, ow, rng, p=0.6):
    return [(rng.random((oh, ow)) < p).astype(np.uint8) * rng.integers(1, 256, size=(oh, ow)).astype(np.uint8)
            for _ in range(n)]


LAYOUTS = ("full", "staggered", "disjoint", "one_pixel", "flush")


def layout(name, n, oh, ow):
    """n rects (dy, dx, h, w) inside oh x ow"""
    if name == "full":
        return [(0, 0, oh, ow)] * n
    if name == "one_pixel":                                                # one 1 x 1 source, the first; the rest cover
        return [(oh // 2, ow // 2, 1, 1)] + [(0, 0, oh, ow)] * (n - 1)
    if name == "staggered":                                                # two thirds of each side, stepping across
        h, w = max(1, (2 * oh + 2) // 3), max(1, (2 * ow + 2) // 3)
        d = max(1, n - 1)
        return [((i * (oh - h)) // d, ((n - 1 - i) * (ow - w)) // d, h, w) for i in range(n)]
    if name == "flush":                                                    # strips along the four edges, in turn
        h, w = max(1, oh // 3), max(1, ow // 3)
        return [[(0, 0, h, ow), (oh - h, 0, h, ow), (0, 0, oh, w), (0, ow - w, oh, w)][i % 4] for i in range(n)]
    if name == "disjoint":                                                 # a grid of cells, each source one row and one
        cols = int(np.ceil(np.sqrt(n)))                                    # column short of its cell: holes between them
        rows = (n + cols - 1) // cols
        ch, cw = max(1, oh // rows), max(1, ow // cols)
        return [(min((i // cols) * ch, oh - 1), min((i % cols) * cw, ow - 1), max(1, ch - 1) if (i // cols) * ch + ch <= oh
                 else 1, max(1, cw - 1) if (i % cols) * cw + cw <= ow else 1) for i in range(n)]
    raise ValueError(name)


def scene(kind, C, h, w, rng, i):
    """source i of a case: random over the whole range, with a block of the least and a block of the largest value"""
    img = rng.integers(0, TOP[kind] + 1, size=(h, w, C)).astype(DTYPES[kind])
    if i % 3 == 0:
        img[: max(1, h // 4), : max(1, w // 4)] = TOP[kind]
    if i % 3 == 1:
        img[-max(1, h // 4):, -max(1, w // 4):] = 0
    return img


# ---- the thinned sweep of the kernel test ---------------------------------------------------------------------------------
KINDS = [("u8", 1), ("u8", 3), ("u8", 4), ("u16", 1), ("u16", 2), ("u16", 3), ("u16", 4)]
NS = [1, 2, 3, 4, 5, 8, 9, 15, 16]                                         # both sides of the median's buckets 4, 8, 16
SIZES = [(1, 1), (3, 5), (33, 130), (70, 1030)]
VALIDITY = ("none", "ladder", "random", "nodata")
NODATA = {"u8": 7, "u16": 300}


def sweep(ki, si):
    """The cases of (kind, size): one per n, with mode, layout, validity, fill and the optional outputs taking turns.
    The ladder goes with the full layout and a count, so that the case's own count can be held to 0 .. n."""
    cases = []
    for ni, n in enumerate(NS):
        t = ki * len(SIZES) + si + ni
        validity = VALIDITY[(ki + si + 3 * ni) % 4]
        ladder = validity == "ladder"
        cases.append(dict(n=n, mode=(t + ni // 4) % 4, layout="full" if ladder else LAYOUTS[(ki + 2 * si + ni) % 5],
                          validity=validity, fill=TOP[KINDS[ki][0]] * ((t // 2 + ni) % 2), want_valid=bool((t // 2) % 2),
                          want_count=ladder or bool((t + ni // 2) % 2), offset=(t // 3) % 2))
    return cases


def case_inputs(kind, C, oh, ow, case):
    """(srcs, valids, rects, nodata) of a sweep case"""
    n = case["n"]
    rng = np.random.default_rng([oh, ow, C, n, case["mode"]])
    rects = layout(case["layout"], n, oh, ow)
    srcs = [scene(kind, C, h, w, rng, i) for i, (_, _, h, w) in enumerate(rects)]
    nodata = [-1] * n
    if case["validity"] == "none":
        masks = [None] * n
    elif case["validity"] == "nodata":                                     # every other source by value, the rest all valid
        masks = [None] * n
        for i in range(0, n, 2):
            nodata[i] = NODATA[kind]
            h, w = rects[i][2:]
            hole = rng.random((h, w)) < 0.4
            srcs[i][hole] = NODATA[kind]
            srcs[i][0, 0] = NODATA[kind]
            if C > 1:
                srcs[i][h - 1, w - 1] = NODATA[kind]
                srcs[i][h - 1, w - 1, C - 1] ^= 1                          # one channel keeps the pixel in
    else:
        whole = ladder_validity(n, oh, ow) if case["validity"] == "ladder" else random_validity(n, oh, ow, rng)
        masks = [np.ascontiguousarray(m[dy:dy + h, dx:dx + w]) for m, (dy, dx, h, w) in zip(whole, rects)]
        if case["validity"] == "random" and n > 1:
            masks[n - 1] = None                                            # a source without a validity window among them
    return srcs, masks, rects, nodata
