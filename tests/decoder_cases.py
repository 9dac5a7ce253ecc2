"""The case list of the range decoder's element tests (test_decoder_cases_cpu.py, test_gpu_decoder_elements.py):
hand-made valid coder tables, symbol streams and geometries aimed at the decoder paths that model latents with
tail = 10 never reach (the full 2^32 interval after a step, the top and the bottom symbol, supports of exactly 64 and
65 entries, a table row per symbol), a coder on Python integers that counts what a case reaches, and the layout of a
batch as the C entry points take it.  No GPU code, no product package."""
import functools
import zlib
from dataclasses import dataclass

import numpy as np

from oracle import entropy_ref as E

GEOMETRIES = [(1, 1), (1, 63), (1, 64), (1, 65), (3, 1), (5, 13), (2, 64), (4, 100), (16, 4)]
# a table row per symbol goes down the general path, which stores symbol by symbol: the geometries that differ only
# in the one-register path's 64-symbol store are left out
GEOMETRIES_PER_ELEMENT = [(1, 1), (1, 65), (3, 1), (5, 13), (4, 100), (16, 4)]
STREAMS = ["uniform", "bottom", "top", "alternate", "runs"]
ONECOUNT_L = [2, 63, 64, 65, 127, 128, 129, 192, 261]
SIGMA_NU = [(s, nu) for s in (1e-3, 0.7, 40.0) for nu in (2.0, 100.0)]   # the corners of the (sigma, nu) clamp box
FILLS = ["zeros", "ones", "random"]


# ---- table builders: uint16 [rows, L], strictly increasing, c[0] = 0, c[L-1] <= 65535 ------------------------------
def dyadic(L, rows=1):
    """c[k] = k 65536 / L for L a power of two: every symbol narrows the interval by whole bits."""
    assert L & (L - 1) == 0
    return np.tile((np.arange(L, dtype=np.int64) * 65536 // L).astype(np.uint16), (rows, 1))


def onecount_low(L, rows=1):
    """c[k] = k: every symbol but the last has one count, the last holds the rest of the mass."""
    return np.tile(np.arange(L, dtype=np.uint16), (rows, 1))


def onecount_high(L, rows=1):
    """c[0] = 0, c[k] = 65536 - L + k: the bottom symbol holds the mass, every other one count."""
    c = 65536 - L + np.arange(L, dtype=np.int64)
    c[0] = 0
    return np.tile(c.astype(np.uint16), (rows, 1))


def half(d, rows=1):
    return np.tile(np.array([0, 32768 + d], dtype=np.uint16), (rows, 1))


def mixed(L, rows=1):
    """Rows that differ: one-count low, one-count high and even counts in turn, so that a wrong row shows."""
    even = (np.arange(L, dtype=np.int64) * 65536 // L).astype(np.uint16)
    kinds = [onecount_low(L)[0], onecount_high(L)[0], even]
    return np.stack([kinds[r % 3] for r in range(rows)])


def product(L, smin, rows=1):
    """The coder's own Student-t tables at the corners of the clamp box, rows cycling through them."""
    sig = np.array([SIGMA_NU[r % len(SIGMA_NU)][0] for r in range(rows)], dtype=np.float32)
    nu = np.array([SIGMA_NU[r % len(SIGMA_NU)][1] for r in range(rows)], dtype=np.float32)
    return E.tables_student(sig, nu, smin, L)


def _smin(L):
    return -(L // 2)


# name -> (family, L, builder(rows))
TABLES = {}
for _L in (1, 2, 4, 64):
    TABLES[f"dyadic{_L}"] = ("dyadic", _L, functools.partial(dyadic, _L))
for _L in ONECOUNT_L:
    TABLES[f"low{_L}"] = ("onecount_low", _L, functools.partial(onecount_low, _L))
    TABLES[f"high{_L}"] = ("onecount_high", _L, functools.partial(onecount_high, _L))
for _d in (-1, 0, 1):
    TABLES[f"half{_d:+d}"] = ("half", 2, functools.partial(half, _d))
for _L in (64, 65, 128):
    TABLES[f"mixed{_L}"] = ("mixed", _L, functools.partial(mixed, _L))
for _L in (21, 64, 65, 130):
    TABLES[f"product{_L}"] = ("product", _L, functools.partial(product, _L, _smin(_L)))
FAMILIES = ["dyadic", "onecount_low", "onecount_high", "half", "mixed", "product"]


@dataclass(frozen=True)
class Case:
    table: str
    C: int
    HW: int
    per_element: int
    stream: str
    seed: int = 0          # of the uniform stream

    @property
    def family(self):
        return TABLES[self.table][0]

    @property
    def L(self):
        return TABLES[self.table][1]

    @property
    def smin(self):
        return _smin(self.L)

    @property
    def n(self):
        return self.C * self.HW

    @property
    def rows(self):
        return self.n if self.per_element else self.C

    @property
    def hw(self):
        """symbols per table row, as the oracle counts them"""
        return 1 if self.per_element else self.HW

    @property
    def general(self):
        """decoded by the decoder's general path (a row in several registers, or a row per symbol)"""
        return bool(self.per_element) or self.L > 64

    @property
    def id(self):
        return f"{self.table}-C{self.C}xHW{self.HW}-pe{self.per_element}-{self.stream}{self.seed or ''}"

    def tables(self):
        return _tables(self.table, self.rows)

    def symbols(self):
        L, n = self.L, self.n
        i = np.arange(n)
        if self.stream == "uniform":
            rng = np.random.default_rng([self.seed, zlib.crc32(self.table.encode()), self.C, self.HW])
            s = rng.integers(0, L, size=n)
        elif self.stream == "bottom":
            s = np.zeros(n)
        elif self.stream == "top":
            s = np.full(n, L - 1)
        elif self.stream == "alternate":
            s = np.where(i % 2 == 0, 0, L - 1)
        else:                                   # a run of each symbol in turn
            s = (i // max(1, n // L)) % L
        return s.astype(np.int32)


@functools.lru_cache(maxsize=None)
def _tables(name, rows):
    t = np.ascontiguousarray(TABLES[name][2](rows=rows), dtype=np.uint16)
    L = TABLES[name][1]
    assert t.shape == (rows, L) and not t[:, 0].any() and (np.diff(t.astype(np.int64), axis=1) > 0).all()
    t.setflags(write=False)
    return t


# Strings of exactly 256 and 512 bytes (they end on a switch of the reader's 64-dword window): uniform streams over one
# row, the symbol count trimmed on the CPU until the oracle's string has that length (test_decoder_cases_cpu.py holds
# the lengths).  (table, symbols, seed)
EXACT = [("product64", 131, 1), ("product64", 261, 1), ("product65", 128, 1), ("product65", 259, 1),
         ("dyadic64", 341, 1), ("dyadic64", 682, 1)]
EXACT_BYTES = [256, 512, 256, 512, 256, 512]


@functools.lru_cache(maxsize=None)
def cases():
    out = [Case(t, C, HW, pe, st) for t in TABLES for pe in (0, 1)
           for (C, HW) in (GEOMETRIES_PER_ELEMENT if pe else GEOMETRIES) for st in STREAMS]
    out += [Case(t, 1, n, 0, "uniform", seed) for t, n, seed in EXACT]
    return tuple(out)


def batches(family=None):
    """The cases in batches of at most 8 images that share a geometry, a stream kind and a family: every image has its
    own table and support, so a batch of one-count tables mixes L = 64 (one register) with L = 65 (two)."""
    groups = {}
    for c in cases():
        if family is None or c.family == family:
            groups.setdefault((c.family, c.C, c.HW, c.per_element, c.stream, c.seed), []).append(c)
    out = []
    for g in groups.values():
        out += [g[i:i + 8] for i in range(0, len(g), 8)]
    return out


@functools.lru_cache(maxsize=None)
def oracle_string(case):
    return E.range_encode(case.symbols(), case.tables(), case.hw)


# ---- the frozen coder on Python integers: 32-bit low / high, 16-bit counts, E1 / E2 / E3, zero bits past the end ----
TOP, HALF, QUARTER = 1 << 32, 1 << 31, 1 << 30


def _narrow(low, high, row, L, s):
    span = high - low + 1
    c_low, c_high = row[s], (row[s + 1] if s + 1 < L else 65536)
    return low + span * c_low // 65536, low + span * c_high // 65536 - 1


def py_encode(sym, table, L, hw):
    low, high, pending, bits = 0, TOP - 1, 0, []
    rows = {}
    for i, s in enumerate(sym):
        r = i // hw
        if r not in rows:
            rows[r] = [int(v) for v in table[r][:L]]
        low, high = _narrow(low, high, rows[r], L, int(s))
        while True:
            if high < HALF or low >= HALF:
                bit = int(low >= HALF)
                bits += [bit] + [1 - bit] * pending
                pending = 0
                low, high = low - bit * HALF, high - bit * HALF
            elif low >= QUARTER and high < 3 * QUARTER:
                pending += 1
                low, high = low - QUARTER, high - QUARTER
            else:
                break
            low, high = 2 * low, 2 * high + 1
    bit = int(low >= QUARTER)
    bits += [bit] + [1 - bit] * (pending + 1)
    bits += [0] * (-len(bits) % 8)
    return bytes(int("".join(map(str, bits[k:k + 8])), 2) for k in range(0, len(bits), 8))


MUTANTS = {
    "a": "the full 2^32 interval treated as span 0",
    "b": "the top symbol's c_high read from entry L of the row instead of 65536",
    "c": "the last dword of the string not masked",
    "d": "c_high of the symbol at entry 63 taken as 65536",
    "e": "the table row advanced every HW + 1 symbols",
}


def py_decode(buf, nbytes, n, table, L, hw, mutant=None):
    """-> (symbols, counters).  buf may be longer than nbytes (the bytes behind a string's end in its row) and table
    wider than L (the entries behind the support): a correct decoder looks at neither.  A mutant decodes until its
    value leaves the interval, and -1 from there on."""
    if mutant == "c":
        nbytes = min(len(buf), (nbytes + 3) // 4 * 4)
    # the string's bits, then zeros: 32 to begin with and at most 18 per step (a step leaves a span of 2^14 or more)
    bits = np.unpackbits(np.frombuffer(bytes(buf[:nbytes]), dtype=np.uint8)).tolist() + [0] * (32 + 18 * n)
    low, high, value, pos = 0, TOP - 1, int("".join(map(str, bits[:32])), 2), 32
    out = []
    st = {"full": 0, "max_shift": 0, "top": 0, "bottom": 0, "lo63_hi64": 0, "mult64": 0}
    rows = {}
    for i in range(n):
        r = i // (hw + 1 if mutant == "e" else hw)
        if r not in rows:
            rows[r] = [int(v) for v in table[min(r, len(table) - 1)]]
        row = rows[r]
        span = high - low + 1
        count = ((value - low + 1) * 65536 - 1) // span
        s = max(k for k in range(L) if row[k] <= count) if L < 8 else _search(row, L, count)
        if mutant == "a" and span == TOP:
            s = L - 1                           # every product floor(0 c / 2^16) = 0 passes the search
        out.append(s)
        st["top"] += s == L - 1
        st["bottom"] += s == 0
        st["lo63_hi64"] += s == 63 and L >= 65
        st["mult64"] += s % 64 == 0 or (s + 1) % 64 == 0
        if mutant == "b" and s == L - 1:
            row = row[:L] + [row[L], row[L]]
            low, high = _narrow(low, high, row, L + 1, s)
        elif mutant == "d" and s == 63:
            low, high = _narrow(low, high, row, 64, s)
        else:
            low, high = _narrow(low, high, row, L, s)
        if not low <= value <= high:
            assert mutant, "the decoder's value left its interval"
            return out + [-1] * (n - len(out)), st
        shift = 0
        while True:
            if high < HALF or low >= HALF:
                off = HALF if low >= HALF else 0
            elif low >= QUARTER and high < 3 * QUARTER:
                off = QUARTER
            else:
                break
            low, high, value = 2 * (low - off), 2 * (high - off) + 1, 2 * (value - off) + bits[pos]
            pos += 1
            shift += 1
        st["max_shift"] = max(st["max_shift"], shift)
        st["full"] += low == 0 and high == TOP - 1
    return out, st


def _search(row, L, count):
    lo, hi = 0, L
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if row[mid] <= count:
            lo = mid
        else:
            hi = mid
    return lo


# ---- a batch as dsic_range_decode takes it -----------------------------------------------------------------------
def lay_out(batch, strings, fill="ones", behind="ones", lstride=3, loff=1, seed=0):
    """Images that share (C, HW, per_element), each with its own (smin, L) in meta and its own table, and one string
    per image.  tables [B][rows][Lmax] with Lmax > every L and the entries k >= L_b from `fill`; the strings in rows of
    round_up(max_len, 4) + 8 bytes with every byte behind a string's end from `behind`; lengths int32
    [B][lstride] with the length in column loff and junk in the others; junk in the z half of meta."""
    rng = np.random.default_rng(seed)
    B, rows = len(batch), batch[0].rows
    assert all((c.C, c.HW, c.per_element) == (batch[0].C, batch[0].HW, batch[0].per_element) for c in batch)
    Lmax = max(c.L for c in batch) + 3
    tables = _filled((B, rows, Lmax), fill, rng, np.uint16)
    meta = rng.integers(-9999, 9999, size=(B, 4)).astype(np.int32)
    stride = (max(len(s) for s in strings) + 3) // 4 * 4 + 8
    raw = _filled((B, stride), behind, rng, np.uint8)
    lengths = rng.integers(-(1 << 31), 1 << 31, size=(B, lstride)).astype(np.int32)
    for b, (c, s) in enumerate(zip(batch, strings)):
        tables[b, :, :c.L] = c.tables()
        meta[b, :2] = (c.smin, c.L)
        raw[b, :len(s)] = np.frombuffer(s, dtype=np.uint8)
        lengths[b, loff] = len(s)
    return {"meta": meta, "tables": tables, "bytes": raw, "lengths": lengths, "Lmax": Lmax, "stride": stride,
            "lstride": lstride, "loff": loff}


def _filled(shape, how, rng, dtype):
    top = np.iinfo(dtype).max
    if how == "random":
        return rng.integers(0, top + 1, size=shape).astype(dtype)
    return np.full(shape, top if how == "ones" else 0, dtype=dtype)
