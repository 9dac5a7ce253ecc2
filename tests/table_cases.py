"""The case list of the CDF-table and support-scan element tests (test_table_cases_cpu.py,
test_gpu_table_elements.py): the (sigma, nu) rows, the supports per Lmax, the refused supports, the layouts of the
Gauss kernel's groups of 16 images, one per-element-shaped Student call and the support-scan inputs, with small Python
restatements of the device's branch conditions (csrc/entropy.hip) so that the CPU test can assert that the list sits
on both sides of each.  Plain data and NumPy; the oracle's tables are computed once per support and shared."""
import functools

import numpy as np

from oracle import entropy_ref as E

_f = np.float32

# ---- parameter rows ------------------------------------------------------------------------------------------------
# The table path takes sigma = exp(log_sigma) unclamped: any float32 >= 0, with 0 (exp underflows), a subnormal and
# inf.  nu: beyond both ends of the usual clamp [2, 100], and the float32 next to 2.  NaN sigma is deliberately not
# here: (uint32_t) of a NaN is undefined in C++, host and device may differ (DESIGN.md "Entropy path").
SIGMAS = np.array([0.0, 1e-38, 1e-6, 1e-3, 1e-2, 0.3, 1.0, 8.0, 50.0, 1e3, 1e6, 3.4e38, np.inf], dtype=_f)
NUS = np.array([1.01, 2.0, np.nextafter(_f(2), _f(3)), 3.0, 17.5, 100.0, 1000.0], dtype=_f)
ROW_SIGMA = np.repeat(SIGMAS, NUS.size)          # 91 Student rows: every (sigma, nu) pair
ROW_NU = np.tile(NUS, SIGMAS.size)

# ---- supports (smin, L), by the Lmax they are launched with ---------------------------------------------------------
SUPPORTS = {
    1000: [(-500, 1000), (1, 1000), (-1000, 1000),                    # L == Lmax: straddling and one-sided
           (-499, 999), (-128, 257), (-127, 255), (-128, 256),        # around the 256-entry flush of the float32 sum
           (-700, 701), (-5, 700),                                    # lopsided either way
           (-40, 40), (-40, 41),                                      # the two sides of smin + L >= 1
           (0, 40), (1, 40),                                          # the two sides of smin <= 0
           (-1, 2),
           (16777210, 12),                                            # float(u) stops being exact at 2^24
           (-999999990, 30)],
    64: [(-31, 64), (-32, 64), (-31, 63), (0, 1), (3, 21)],
    1: [(0, 1), (5, 1), (-3, 1)],
}
LMAXES = [1000, 64, 1]


def refused(Lmax):
    """Supports every consumer of `meta` refuses (error bit 1): L > Lmax, L < 1."""
    return [(0, Lmax + 1), (0, 0), (0, -3), (-2 ** 31, 0)]


def valid(s, Lmax):
    return 1 <= s[1] <= Lmax


def with_refused(Lmax):
    """The Lmax group's supports with the refused supports placed among them and one behind the last."""
    sup, bad = list(SUPPORTS[Lmax]), refused(Lmax)
    step = max(1, len(sup) // len(bad))
    out = []
    for i, s in enumerate(sup):
        out.append(s)
        if i % step == 0 and len(bad) > 1:
            out.append(bad.pop(0))
    return out + bad


# ---- restatements of the device's branch conditions ----------------------------------------------------------------
def student_route(smin, L):
    """tables_kernel<true>: "mirror" evaluates one tail per |boundary| and writes F at both signs, "each" evaluates
    every boundary on its own."""
    return "mirror" if smin <= 0 and smin + L >= 1 else "each"


def whi_operand(smin, L):
    """The mirror route walks w = 1 .. whi = max(smin + L, 1 - smin): which operand sets the bound."""
    assert student_route(smin, L) == "mirror"
    return "right" if smin + L > 1 - smin else "left"


def sum_levels(L):
    """Levels of sum_f32_torch that receive a flush for L entries: 1 below 16, 2 from 16, 3 from 256."""
    return 1 + (L >= 16) + (L >= 256)


def finish_passes(L):
    """64-lane passes of finish_table_wave."""
    return (L + 63) // 64


def gauss_union(group, Lmax):
    """(lo, hi) over the valid supports' u = smin .. smin + L of one workgroup's images, or None."""
    ok = [s for s in group if valid(s, Lmax)]
    if not ok:
        return None
    return min(s[0] for s in ok), max(s[0] + s[1] for s in ok)


def gauss_width(group, Lmax):
    u = gauss_union(group, Lmax)
    return None if u is None else u[1] - u[0]


def gauss_shares_row(group, Lmax):
    """gauss_tables_kernel evaluates one CDF row for the group iff the union is at most 4 Lmax - 1 wide."""
    w = gauss_width(group, Lmax)
    return w is not None and w < 4 * Lmax


def support_restated(values, tail):
    """support_kernel on one half (y or z) of one image: (lo, L) = (floor(min) - tail, ceil(max) + tail - lo + 1);
    a NaN, an infinity or a magnitude of 1e9 or more anywhere gives (0, 0), which every consumer refuses."""
    v = np.asarray(values, dtype=_f).ravel()
    if not np.all(np.abs(v) < _f(1.0e9)):
        return 0, 0
    lo = int(np.floor(v.min())) - tail
    hi = int(np.ceil(v.max())) + tail
    return lo, hi - lo + 1


def meta_restated(y, z, tail):
    """[B, 4] int64 {ymin - tail, Ly, zmin - tail, Lz} of y [B, ny], z [B, nz]."""
    return np.array([[*support_restated(y[b], tail), *support_restated(z[b], tail)] for b in range(len(y))],
                    dtype=np.int64)


# ---- Gauss group layouts ----------------------------------------------------------------------------------------------
ZT_IMGS = 16           # images per workgroup of gauss_tables_kernel
GAUSS_BATCHES = [1, 16, 17, 33]


def _fill(first, last, Lmax, n=ZT_IMGS):
    """n supports inside [first.smin, last.smin + last.L]: the two given ones at the ends of the group's images,
    narrower ones of varying width between them."""
    lo, hi = first[0], last[0] + last[1]
    mid = []
    for i in range(n - 2):
        L = 1 + (i * 37) % Lmax
        smin = lo + (i * 53) % max(1, hi - lo - L + 1)
        mid.append((smin, L))
    return [first] + mid + [last]


def group_shared_edge(Lmax):
    """Union exactly 4 Lmax - 1 wide: the widest that still shares the row."""
    lo = -2 * Lmax
    return _fill((lo, Lmax), (lo + 3 * Lmax - 1, Lmax), Lmax)


def group_own_edge(Lmax):
    """Union exactly 4 Lmax wide: every table evaluates its own boundaries."""
    lo = -2 * Lmax
    return _fill((lo, Lmax), (lo + 3 * Lmax, Lmax), Lmax)


def group_refused(Lmax):
    """Each refused support beside valid ones.  The union of the valid ones is narrow: the row is shared."""
    g = _fill((-Lmax, Lmax), (0, Lmax), Lmax)
    for i, s in zip((1, 6, 11, 15), refused(Lmax)):
        g[i] = s
    return g


def group_far_apart(Lmax):
    """Supports 9000 apart."""
    return [(9000 * (i - 8) - (i % 3), 1 + (i * 29) % Lmax) for i in range(ZT_IMGS)]


def gauss_layout(B, Lmax):
    """The images' z supports of one launch, group after group."""
    if B == 1:
        return [SUPPORTS[Lmax][0]]
    if B == 16:
        return group_far_apart(Lmax)
    if B == 17:
        return group_refused(Lmax) + [SUPPORTS[Lmax][-1]]
    assert B == 33
    return group_shared_edge(Lmax) + group_own_edge(Lmax) + [SUPPORTS[Lmax][1]]


def groups_of(layout):
    return [layout[i:i + ZT_IMGS] for i in range(0, len(layout), ZT_IMGS)]


# ---- one per-element-shaped Student call: B = 3, 7 rows per image -> 21 tables, a last workgroup of one wave --------
PER_ELEMENT_LMAX = 64
PER_ELEMENT_SUPPORTS = [(-31, 64), (0, 1), (3, 21)]
PER_ELEMENT_ROWS = (np.arange(21) * 10 + 5) % ROW_SIGMA.size      # 21 distinct rows of the 91


# ---- oracle tables, once per support ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_student(smin, L):
    """-> (tables [91, L], raw [91, L + 1]) uint16 of every parameter row; read-only."""
    out, raw = E.tables_student(ROW_SIGMA, ROW_NU, smin, L, raw=True)
    out.setflags(write=False)
    raw.setflags(write=False)
    return out, raw


@functools.lru_cache(maxsize=None)
def oracle_gauss(smin, L):
    """-> (tables [13, L], raw [13, L + 1]) uint16 of every sigma; read-only."""
    out, raw = E.tables_gauss(SIGMAS, smin, L, raw=True)
    out.setflags(write=False)
    raw.setflags(write=False)
    return out, raw


# ---- support-scan cases: (name, y [B, ny], z [B, nz], tail) ---------------------------------------------------------------
SCAN_SIZES = [1, 63, 64, 255, 256, 257, 1000]       # below, at and above the wave (64) and block (256) seams
SCAN_POSITIONS = [0, -1, 63, 64, 255, 256]          # -1: the last index
SCAN_TAILS = [0, 10, 1000]
GUARD_MAX = _f(999999936.0)                         # the largest float32 below 1e9
SCAN_BAD = [("p1e9", _f(1e9)), ("m1e9", _f(-1e9)), ("nan", _f(np.nan)), ("pinf", _f(np.inf)), ("minf", _f(-np.inf))]


def _noise(rng, B, n, lo=-3.0, hi=7.0):
    """Non-integer values strictly inside (lo, hi)."""
    return rng.uniform(lo + 0.01, hi - 0.01, (B, n)).astype(_f)


def scan_cases():
    cases = []
    rng = np.random.default_rng(2024)
    # element counts, y and z independently; non-integer one-off extremes so that floor and ceil both move
    for i, ny in enumerate(SCAN_SIZES):
        for j, nz in enumerate(SCAN_SIZES):
            y, z = _noise(rng, 2, ny), _noise(rng, 2, nz, -9.0, 2.0)
            cases.append((f"size_{ny}_{nz}", y, z, SCAN_TAILS[(i + j) % 3]))
    # the minimum (-3.5) and the maximum (7.25) at every pair of positions: one image per pair
    for n in (257, 1000):
        pairs = [(p, q) for p in SCAN_POSITIONS for q in SCAN_POSITIONS if p % n != q % n]
        y, z = _noise(rng, len(pairs), n), _noise(rng, len(pairs), n)
        for b, (p, q) in enumerate(pairs):
            y[b, p], y[b, q] = -3.5, 7.25
            z[b, q], z[b, p] = -3.5, 7.25
        for tail in SCAN_TAILS:
            cases.append((f"extrema_{n}_tail{tail}", y, z, tail))
    # one-sided, constant and signed-zero data
    for n in (1, 64, 300):
        y = np.stack([-_noise(rng, 1, n, 2.0, 9.0)[0], _noise(rng, 1, n, 2.0, 9.0)[0], np.full(n, 4.0, _f),
                      np.full(n, -0.0, _f), np.full(n, -2.5, _f), np.full(n, 2.5, _f)])
        z = np.ascontiguousarray(y[::-1])
        for tail in SCAN_TAILS:
            cases.append((f"onesided_{n}_tail{tail}", y, z, tail))
    # the largest magnitudes the guard admits, at the first and the last index
    for n in (1, 257):
        y, z = _noise(rng, 4, n), _noise(rng, 4, n)
        y[0, 0], y[1, -1], y[2, 0], y[2, -1] = GUARD_MAX, -GUARD_MAX, GUARD_MAX, -GUARD_MAX
        z[0, -1], z[1, 0], z[3, -1], z[3, 0] = -GUARD_MAX, GUARD_MAX, GUARD_MAX, -GUARD_MAX
        for tail in SCAN_TAILS:
            cases.append((f"guard_{n}_tail{tail}", y, z, tail))
    return cases


def bad_scan_cases():
    """(name, y [3, 300], z [3, 257], tail 10, bad image): a value the guard refuses at the first or the last index
    of y only, of z only, and of one image of three in both; the valid halves stay within |v| < 20 (L <= 61)."""
    cases = []
    rng = np.random.default_rng(77)
    for name, v in SCAN_BAD:
        for pos in (0, -1):
            for where in ("y", "z", "image"):
                y, z = np.rint(_noise(rng, 3, 300, -19.0, 17.0)), np.rint(_noise(rng, 3, 257, -12.0, 19.0))
                y[:, 5], z[:, 7] = -6.5, 8.25           # non-integer extremes may also stand beside a refused half
                if where == "y":
                    y[:, pos] = v
                elif where == "z":
                    z[:, pos] = v
                else:
                    y[1, pos] = z[1, pos] = v
                cases.append((f"{name}_{'first' if pos == 0 else 'last'}_{where}", y.astype(_f), z.astype(_f), 10))
    return cases


BAD_SCAN_LMAX = 64
BAD_SCAN_ROWS = (np.arange(7) * 17 + 3) % ROW_SIGMA.size          # 7 of the 91 rows for the tables built from a scan


# ---- the sentinel -----------------------------------------------------------------------------------------------------
def sentinel(Lmax):
    """Pre-fill of a table row, uint16 [Lmax]: (k - 1) mod 2^16 at position k.  No table holds it there: entry k of
    any table is floor(u16 (65536 - L) / 65535) + k >= k > k - 1, and entry 0 is 0, never 0xFFFF.  An overrun of the row in front of it
    would write that row's entry Lmax + k here, which is >= Lmax + k."""
    return ((np.arange(Lmax, dtype=np.int64) - 1) & 0xFFFF).astype(np.uint16)
