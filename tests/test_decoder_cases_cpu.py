"""The decoder's case list (decoder_cases.py) on the CPU: the bit-serial oracle against a coder on Python integers
for every case and for arbitrary bytes, the conditions under which the list reaches what it claims to reach, and five
wrong decoders that the list must tell from the right one."""
import numpy as np
import pytest

import decoder_cases as D
from oracle import entropy_ref as E

_STATS = {}


def _decoded(case):
    """The Python-integer decode of the case's oracle string, with its counters (once per case)."""
    if case not in _STATS:
        s = D.oracle_string(case)
        _STATS[case] = D.py_decode(s, len(s), case.n, case.tables(), case.L, case.hw)
    return _STATS[case]


def _family_cases(family):
    return [c for c in D.cases() if c.family == family]


def test_the_list_is_what_the_tests_assume():
    cs = D.cases()
    assert len(set(c.id for c in cs)) == len(cs)
    assert max(c.n for c in cs) < 20000 and all(len(b) <= 8 for b in D.batches())
    assert sum(len(b) for b in D.batches()) == len(cs)
    assert {c.family for c in cs} == set(D.FAMILIES)
    assert {(c.C, c.HW) for c in cs} >= set(D.GEOMETRIES)
    for L in D.ONECOUNT_L:
        lo, hi = D.onecount_low(L)[0].astype(int), D.onecount_high(L)[0].astype(int)
        assert list(lo) == list(range(L)) and hi[0] == 0 and list(hi[1:]) == [65536 - L + k for k in range(1, L)]
    assert [list(D.half(d)[0]) for d in (-1, 0, 1)] == [[0, 32767], [0, 32768], [0, 32769]]
    # a batch of one-count tables holds supports of 64 and of 65 entries side by side
    assert any({64, 65} <= {c.L for c in b} for b in D.batches("onecount_low"))
    assert any(c.per_element and c.L <= 64 for c in cs)


@pytest.mark.parametrize("family", D.FAMILIES)
def test_oracle_encodes_and_decodes_as_python_integers(family):
    for c in _family_cases(family):
        sym, tab = c.symbols(), c.tables()
        s = D.oracle_string(c)
        assert s == D.py_encode(sym, tab, c.L, c.hw), c.id
        assert np.array_equal(E.range_decode(s, c.n, tab, c.hw), sym), c.id
        assert _decoded(c)[0] == sym.tolist(), c.id


@pytest.mark.parametrize("family", D.FAMILIES)
def test_oracle_decodes_arbitrary_bytes_as_python_integers(family):
    """Random bytes and truncated strings have one right answer too: the decoder keeps low <= value <= high whatever
    it reads (py_decode asserts it), so every symbol lies inside the support."""
    rng = np.random.default_rng(17)
    for c in _family_cases(family):
        if c.stream in ("bottom", "top") or (c.per_element and c.family not in ("mixed", "product")):
            continue          # one symbol only; rows that are all alike, so the string of the per-channel case
        s, tab = D.oracle_string(c), c.tables()
        tries = [s[:cut] for cut in sorted({0, 1, len(s) // 2, len(s) - 1}) if cut <= len(s)]
        tries.append(rng.integers(0, 256, size=int(rng.integers(0, len(s) + 6)), dtype=np.uint8).tobytes())
        for t in tries:
            want = E.range_decode(t or b"\0", c.n, tab, c.hw)
            got, _ = D.py_decode(t, len(t), c.n, tab, c.L, c.hw)
            assert got == want.tolist(), (c.id, len(t))
            assert 0 <= min(got) and max(got) < c.L


def test_exact_lengths():
    got = [len(D.oracle_string(c)) for c in D.cases()[-len(D.EXACT):]]
    assert got == D.EXACT_BYTES


def test_coverage_conditions():
    """What the list must reach, from the counters of the Python-integer decoder: conditions, not measurements."""
    cs = D.cases()
    st = {c: _decoded(c)[1] for c in cs}
    for L in (1, 63, 64, 65, 128, 129, 261):
        assert any(c.L == L and st[c]["top"] >= 20 and st[c]["bottom"] >= 20 for c in cs), L
    assert any(not c.general and st[c]["full"] >= 50 for c in cs)
    assert any(c.general and st[c]["full"] >= 50 for c in cs)
    assert any(c.general and c.per_element and c.L <= 64 and st[c]["full"] >= 50 for c in cs)
    assert any(c.L >= 65 and st[c]["lo63_hi64"] > 0 for c in cs)
    assert any(c.L >= 65 and not c.per_element and st[c]["mult64"] >= 20 for c in cs)
    assert any(c.L == 128 and st[c]["top"] > 0 for c in cs)
    assert any(c.L == 64 and not c.per_element and st[c]["top"] >= 20 for c in cs)
    lens = {len(D.oracle_string(c)) for c in cs}
    assert 256 in lens and 512 in lens
    # One step's renormalisation shift (E1 / E2 plus E3).  After renormalisation the interval lies neither inside a
    # half nor inside the middle half, so span > 2^30.  A symbol holds at least one of the 2^16 counts, and
    # floor(a + b) - floor(a) >= floor(b), so a step leaves span' >= floor(span / 2^16) >= 2^14.  Every shift doubles
    # the span exactly, and the span never exceeds 2^32: 2^14 2^shift <= 2^32.  Equality (shift 18) needs span' = 2^14
    # exactly AND a low on a multiple of 2^14, from where 18 E1 / E2 shifts end on the full interval; everything else
    # stays at 17 or below, and that is what the list must show.  Either way nb + m is far below 32.
    # The other way round a one-count symbol leaves span' <= 2^16 and the next span is again > 2^30: shift >= 15.
    shifts = [s["max_shift"] for s in st.values()]
    print("largest single-step shift over the list:", max(shifts))
    assert max(shifts) <= 17
    assert max(shifts) >= 15


# the family in which each mutant is looked for
AIMED_AT = {"a": "dyadic", "b": "onecount_high", "c": "half", "d": "onecount_low", "e": "mixed"}


@pytest.mark.parametrize("mutant", sorted(D.MUTANTS))
def test_the_list_sees_a_wrong_decoder(mutant):
    """Each mutant of the Python-integer decoder reads a batch as the device gets it (garbage behind the support and
    behind the string) and must decode some case differently from the oracle; the unchanged decoder must not."""
    seen = []
    for batch in D.batches(AIMED_AT[mutant]):
        if len(seen) >= 3:
            break
        whole = [D.oracle_string(c) for c in batch]
        # a whole string decodes alike whatever follows it (that is what the encoder's flush is for), so the bytes
        # behind the end can only show behind a string that was cut
        for strings in (whole, [s[:len(s) // 2] for s in whole]):
            for fill in ("zeros", "ones"):
                lay = D.lay_out(batch, strings, fill=fill, behind="ones")
                for b, c in enumerate(batch):
                    args = (lay["bytes"][b].tolist(), len(strings[b]), c.n, lay["tables"][b], c.L, c.hw)
                    want = E.range_decode(strings[b] or b"\0", c.n, c.tables(), c.hw).tolist()
                    if D.py_decode(*args, mutant=mutant)[0] != want:
                        seen.append(f"{c.id}/{fill}/{len(strings[b])} of {len(whole[b])} bytes")
                        assert D.py_decode(*args)[0] == want, c.id
    print(f"mutant {mutant} ({D.MUTANTS[mutant]}): first seen by {seen[:3]}")
    assert seen, D.MUTANTS[mutant]
