"""CPU-only: the paired schedule of pass B of the 64-tile Winograd kernel (csrc/conv_wino_pair.h) feeds every
accumulator the same (chunk, position) products in the same order as the unpaired one.  The sequences come from
dsic_wino_pair_schedule, a host walk over the constexpr step, slot and chunk-pass tables the kernel itself reads; it
also fails (negative) if the V slot an MFMA step reads is not the one the helpers commit that (chunk, position) to,
or if the wave half that sits out a paired chunk-pass had a live position in it."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def L():
    from dsic_amd import lib
    return lib.load()


def _seq(L, mode, nchunks, phase, paired, pq, acc):
    cap = 4 * nchunks
    buf = (ctypes.c_int * (2 * cap))()
    n = L.dsic_wino_pair_schedule(mode, nchunks, phase, paired, pq, acc, buf, cap)
    assert 0 <= n <= cap, (mode, nchunks, phase, paired, pq, acc, n)
    return [(buf[2 * i], buf[2 * i + 1]) for i in range(n)]


@pytest.mark.parametrize("nchunks", [4, 8, 16, 32])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_paired_and_unpaired_sequences_are_equal(L, mode, nchunks):
    for phase in range(4):
        for pq in range(2):
            for acc in range(4):
                plain = _seq(L, mode, nchunks, phase, 0, pq, acc)
                paired = _seq(L, mode, nchunks, phase, 1, pq, acc)
                assert paired == plain, (mode, nchunks, phase, pq, acc)
                # the unpaired order itself: one position per accumulator, its live chunks ascending
                assert len({g for _, g in plain}) <= 1
                assert [c for c, _ in plain] == sorted({c for c, _ in plain})
                xi = 0 if pq == 0 else 3
                assert all(g >> 2 == xi for _, g in plain)


def test_live_chunks_per_row(L):
    """What the structural zeros leave: space-to-depth blocks 2, 3 have no row 3 (and blocks 1, 3 no column 3),
    ConvTranspose phases 2, 3 no row 0 (phases 1, 3 no column 0)."""
    n = 8
    # mode 1, row 3 (pq 1): chunks of blocks 0, 1 only; its column-3 accumulator only block 0
    for acc in range(4):
        seq = _seq(L, 1, n, 0, 1, 1, acc)
        g = seq[0][1]
        assert [c for c, _ in seq] == ([0, 1] if g & 3 == 3 else [0, 1, 2, 3])
        seq = _seq(L, 1, n, 0, 1, 0, acc)
        g = seq[0][1]
        assert [c for c, _ in seq] == ([0, 1, 4, 5] if g & 3 == 3 else list(range(8)))
    for phase in range(4):
        for pq in range(2):
            for acc in range(4):
                seq = _seq(L, 2, n, phase, 1, pq, acc)
                dead_row = pq == 0 and phase >> 1
                if dead_row:
                    assert seq == []
                    continue
                g = seq[0][1] if seq else None
                if seq:
                    assert [c for c, _ in seq] == list(range(n))
                else:
                    assert phase & 1   # the column-0 accumulator of a phase 1 / 3 item
    assert L.dsic_wino_pair_schedule(3, 8, 0, 1, 0, 0, None, 0) == -1
    assert L.dsic_wino_pair_schedule(1, 7, 0, 1, 0, 0, None, 0) == -1
