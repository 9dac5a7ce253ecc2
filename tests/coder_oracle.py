"""The bit-serial CPU coder (oracle/entropy_ref.c) as the reference of the GPU encoders: a helper of
test_gpu_split_coder.py and test_gpu_place_slices.py.  The split encoder and the single kernel share their interval
arithmetic, so their equality no longer checks it; the oracle's strings on the run's own tables do."""
import numpy as np
import torch

from oracle import entropy_ref as E


def _tables(t):
    """device uint16 / int16 coder tables -> numpy uint16"""
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def oracle_strings(y, z, meta, tab_y, tab_z):
    """Per image (z string, y string) of the oracle for the latents y [B, M, ...], z [B, N, ...] on the supports `meta`
    and the device tables of the run (a row per channel, or per symbol: hw = 1).  A symbol outside its support is coded
    as symbol 0, as the encoders do beside error bit 2."""
    y, z = (np.asarray(a.cpu() if torch.is_tensor(a) else a) for a in (y, z))
    meta = np.asarray(meta.cpu() if torch.is_tensor(meta) else meta)
    tabs = (_tables(tab_z), _tables(tab_y))
    out = []
    for b in range(y.shape[0]):
        pair = []
        for which, lat in enumerate((z, y)):           # which as the encoders count: 0 = z, 1 = y
            smin, L = int(meta[b, 2 - 2 * which]), int(meta[b, 3 - 2 * which])
            sym = lat[b].astype(np.int32).ravel() - smin
            sym[(sym < 0) | (sym >= L)] = 0
            rows = tabs[which][b]
            C = lat.shape[1]
            hw = 1 if rows.shape[0] != C else sym.size // C
            pair.append(E.range_encode(sym, rows[:, :L], hw))
        out.append(tuple(pair))
    return out


def assert_oracle(res, want, cap_z):
    """bytes[:length] and length of every z and y string of an encoder output (rows [cap_z | cap_y]) equal the
    oracle's string, and the capacity behind the string is still zero."""
    raw, lens = res["bytes"].cpu().numpy(), res["lengths"].cpu().numpy()
    for b, strings in enumerate(want):
        for which, s in enumerate(strings):
            off, end = (cap_z, raw.shape[1]) if which else (0, cap_z)
            assert int(lens[b, which]) == len(s), (b, which, int(lens[b, which]), len(s))
            assert raw[b, off:off + len(s)].tobytes() == s, (b, which)
            assert not raw[b, off + len(s):end].any(), (b, which)


def assert_oracle_of(c, y, z):
    """assert_oracle for compress_latents' dict c (unsegmented) of the latents y, z."""
    assert c["segments"] == 1
    assert_oracle(c, oracle_strings(y, z, c["meta"], c["tab_y"], c["tab_z"]), c["cap_z"])


def assert_oracle_prefix(res, want, cap_z, cap_y):
    """Capacities that may be too small (error bit 4): a string that fits is the oracle's, with its length, behind it
    zeros; one that does not is a bit-prefix of the oracle's string with nothing but zeros behind it.  A piece is at
    most 32 bits and is dropped whole, so the prefix ends less than 32 bits before the capacity."""
    raw, lens = res["bytes"].cpu().numpy(), res["lengths"].cpu().numpy()
    for b, strings in enumerate(want):
        for which, s in enumerate(strings):
            off, cap = (cap_z, cap_y) if which else (0, cap_z)
            got = np.unpackbits(raw[b, off:off + cap])
            ref = np.unpackbits(np.frombuffer(s, dtype=np.uint8))
            if len(s) <= cap:
                assert int(lens[b, which]) == len(s), (b, which, int(lens[b, which]), len(s))
                assert np.array_equal(got[:ref.size], ref) and not got[ref.size:].any(), (b, which)
                continue
            differ = np.nonzero(got != ref[:got.size])[0]
            end = int(differ[0]) if differ.size else got.size      # the common prefix
            assert end > got.size - 32, (b, which, end, got.size)
            assert not got[end:].any(), (b, which)
