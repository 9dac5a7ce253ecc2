"""The range decoder (dsic_range_decode, dsic_range_decode_seg) symbol by symbol against the bit-serial CPU oracle on
the case list of decoder_cases.py: hand-made valid tables that bring the interval back to the full 2^32 after a step
(span = 0 in the one-register path), top and bottom symbols, supports of exactly 64 and 65 entries, a table row per
symbol with narrow supports, strings that end on a window switch, arbitrary and truncated bytes, garbage behind the
support and behind the string, and a bad support among good ones.  The model's latents with tail = 10 reach none of
these.  The encoders meet the same tables at the end."""
import functools

import numpy as np
import pytest
import torch

import coder_oracle as O
import decoder_cases as D
from oracle import entropy_ref as E

pytestmark = pytest.mark.gpu
GUARD, SENTINEL = 4096, -12345.0
KS = [2, 4, 8, 16]


def _dev(a):
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _decode(lay, C, HW, per_element, segs=None, seg_lengths=None):
    """One call of dsic_range_decode (segs None) or dsic_range_decode_seg on a laid-out batch -> (out [B, C HW] numpy,
    err).  The output is a slice of a sentinel buffer with a guard on each side, which must come back untouched."""
    from dsic_amd import lib as _lib
    from dsic_amd.ops import _p, _stream
    B, n = lay["meta"].shape[0], C * HW
    raw, lengths, meta, tables = (_dev(lay[k]) for k in ("bytes", "lengths", "meta", "tables"))
    buf = torch.full((B * n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    out = buf[GUARD:GUARD + B * n]
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    L = _lib.load()
    if segs is None:
        _lib.check(L.dsic_range_decode(_p(raw), lay["stride"], _p(lengths), lay["lstride"], lay["loff"], _p(meta), 0,
                                       _p(tables), lay["Lmax"], B, C, HW, per_element, _p(out), _p(err), _stream()),
                   "range_decode")
    else:
        sl = torch.tensor(seg_lengths, dtype=torch.int32, device="cuda")
        _lib.check(L.dsic_range_decode_seg(_p(raw), lay["stride"], _p(lengths), lay["lstride"], lay["loff"], _p(sl),
                                           segs, _p(meta), 0, _p(tables), lay["Lmax"], B, C, HW, per_element, _p(out),
                                           _p(err), _stream()), "range_decode_seg")
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all()), "a guard was written"
    return out.view(B, n).cpu().numpy(), int(err.item())


def _assert_symbols(out, batch, want, what):
    """out [B, n] floats = want[b] + smin_b, element for element; a failure names the case, the image and the first
    wrong symbol."""
    for b, c in enumerate(batch):
        got = out[b].astype(np.int64) - c.smin
        w = np.asarray(want[b], dtype=np.int64)
        if not np.array_equal(out[b], (w + c.smin).astype(np.float32)):
            i = int(np.nonzero(got != w)[0][0])
            pytest.fail(f"{what}: {c.id} (L = {c.L}), image {b}: symbol {i} of {c.n} decodes to {got[i]}, the oracle "
                        f"has {w[i]}")


def _geometry(batch):
    return batch[0].C, batch[0].HW, batch[0].per_element


@functools.lru_cache(maxsize=None)
def _segment_strings(case, K):
    """The oracle's string of each of the K channel groups of a case, coded on its own."""
    sym, tab = case.symbols(), case.tables()
    ns, nr = case.n // K, case.rows // K
    return tuple(E.range_encode(sym[k * ns:(k + 1) * ns], tab[k * nr:(k + 1) * nr], case.hw) for k in range(K))


def _oracle_decode(case, data):
    return E.range_decode(data or b"\0", case.n, case.tables(), case.hw)      # no bytes: a zero, which reads alike


@pytest.mark.parametrize("fill", D.FILLS)
@pytest.mark.parametrize("family", D.FAMILIES)
def test_exact_symbols_from_the_oracles_strings(family, fill):
    """Every case of the family: out == symbol + smin, err == 0, whatever stands in the table entries k >= L_b
    (zeros, 0xFFFF, random) and behind the strings (random).  Through dsic_range_decode, through
    dsic_range_decode_seg with one segment, and where the channels divide with 2 to 16 segments that the oracle coded
    one by one and that lie back to back."""
    for batch in D.batches(family):
        C, HW, pe = _geometry(batch)
        want = [c.symbols() for c in batch]
        strings = [D.oracle_string(c) for c in batch]
        lay = D.lay_out(batch, strings, fill=fill, behind="random", seed=len(strings[0]))
        out, err = _decode(lay, C, HW, pe)
        assert err == 0
        _assert_symbols(out, batch, want, f"range_decode, fill {fill}")
        if fill != "random":
            continue
        out1, err = _decode(lay, C, HW, pe, segs=1, seg_lengths=[[len(s)] for s in strings])
        assert err == 0 and np.array_equal(out1, out), batch[0].id
        for K in KS:
            if C % K:
                continue
            segs = [_segment_strings(c, K) for c in batch]
            lay = D.lay_out(batch, [b"".join(s) for s in segs], fill=fill, behind="random", seed=K)
            out, err = _decode(lay, C, HW, pe, segs=K, seg_lengths=[[len(v) for v in s] for s in segs])
            assert err == 0
            _assert_symbols(out, batch, want, f"range_decode_seg, {K} segments")


def test_segments_start_at_all_four_byte_alignments():
    starts = {sum(len(v) for v in _segment_strings(c, K)[:k]) & 3
              for c in D.cases() for K in KS if c.C % K == 0 for k in range(K)}
    assert starts == {0, 1, 2, 3}


ARBITRARY_LENGTHS = [0, 1, 2, 3, 4, 5, 255, 256, 257, 511, 512, 513]
# (table, per_element): narrow and wide supports, and rows per symbol with a narrow one
ARBITRARY_TABLES = [("dyadic64", 0), ("low65", 0), ("high64", 0), ("half+1", 0), ("mixed65", 0), ("product21", 0),
                    ("product64", 0), ("product130", 0), ("mixed64", 1), ("product64", 1)]


@pytest.mark.parametrize("table,pe", ARBITRARY_TABLES)
def test_arbitrary_bytes_decode_as_the_oracle_decodes_them(table, pe):
    """Random bytes of lengths around the reader's dword and window edges, and a real string cut short: any bytes have
    one right answer (the oracle's decoder is total), every symbol lies in the support, nothing is touched outside the
    output.  The bytes behind each length are random and must not count."""
    case = D.Case(table, 4, 500, pe, "uniform")
    rng = np.random.default_rng(23)
    s = D.oracle_string(case)
    strings = [rng.integers(0, 256, size=k, dtype=np.uint8).tobytes() for k in ARBITRARY_LENGTHS]
    strings += [s[:cut] for cut in (0, 1, len(s) // 2, len(s) - 1)]
    for at in range(0, len(strings), 8):
        part = strings[at:at + 8]
        batch = [case] * len(part)
        lay = D.lay_out(batch, part, fill="random", behind="random", seed=at)
        out, err = _decode(lay, case.C, case.HW, pe)
        assert err == 0
        assert out.min() >= case.smin and out.max() <= case.smin + case.L - 1
        _assert_symbols(out, batch, [_oracle_decode(case, p) for p in part], f"arbitrary bytes {[len(p) for p in part]}")


@pytest.mark.parametrize("family", D.FAMILIES)
def test_bytes_behind_the_end_do_not_matter(family):
    """Zeros, 0xFF and random bytes behind lengths[b], inside the last dword and beyond it.  A whole string decodes
    alike whatever follows it (the encoder's flush sees to that), so the strings are cut in half: then the bits that
    follow decide symbols, and a reader that lets them in decodes something else than the oracle does."""
    for batch in D.batches(family):
        if batch[0].stream in ("bottom", "top"):
            continue
        C, HW, pe = _geometry(batch)
        strings = [D.oracle_string(c)[:len(D.oracle_string(c)) // 2] for c in batch]
        want = [_oracle_decode(c, s) for c, s in zip(batch, strings)]
        for behind in D.FILLS:
            lay = D.lay_out(batch, strings, fill="ones", behind=behind, seed=7)
            out, err = _decode(lay, C, HW, pe)
            assert err == 0
            _assert_symbols(out, batch, want, f"bytes behind the end: {behind}")


@pytest.mark.parametrize("lstride,loff", [(1, 0), (2, 0), (3, 1), (5, 4)])
def test_lengths_stride_and_offset(lstride, loff):
    for batch in D.batches("product") + D.batches("half"):
        if batch[0].stream != "uniform":
            continue
        C, HW, pe = _geometry(batch)
        lay = D.lay_out(batch, [D.oracle_string(c) for c in batch], lstride=lstride, loff=loff)
        out, err = _decode(lay, C, HW, pe)
        assert err == 0
        _assert_symbols(out, batch, [c.symbols() for c in batch], f"lengths [B][{lstride}], column {loff}")


@pytest.mark.parametrize("pe", [0, 1])
def test_a_bad_support_among_good_ones(pe):
    """L = 0 and L = Lmax + 1 in images 1 and 3 of 5: error bit 1 and nothing else, their outputs untouched, the other
    three images exact; the same in four segments."""
    batch = [D.Case(t, 4, 100, pe, "uniform") for t in ("product64", "low65", "dyadic64", "high129", "product130")]
    want = [c.symbols() for c in batch]
    for K in (None, 4):
        if K is None:
            strings, sl = [D.oracle_string(c) for c in batch], None
        else:
            segs = [_segment_strings(c, K) for c in batch]
            strings, sl = [b"".join(s) for s in segs], [[len(v) for v in s] for s in segs]
        lay = D.lay_out(batch, strings, fill="random", behind="random")
        lay["meta"][1, 1] = 0
        lay["meta"][3, 1] = lay["Lmax"] + 1
        out, err = _decode(lay, 4, 100, pe, segs=K, seg_lengths=sl)
        assert err == 1
        assert (out[1] == SENTINEL).all() and (out[3] == SENTINEL).all()
        keep = [0, 2, 4]
        _assert_symbols(out[keep], [batch[b] for b in keep], [want[b] for b in keep], f"bad supports, segments {K}")


# ---- the encoders on the same tables ---------------------------------------------------------------------------------
def _encode(batch, lay, how, K=1):
    """The batch's symbols as y latents beside a one-symbol z family through one of the three encoders ->
    (bytes [B, cap_z + K cap_y], lengths [B, 1 + K], err, cap_z, cap_y)."""
    from dsic_amd import entropy, lib as _lib
    from dsic_amd.ops import _p, _stream
    L = _lib.load()
    C, HW, pe = _geometry(batch)
    B, Lmax = len(batch), lay["Lmax"]
    y = _dev(np.stack([(c.symbols() + c.smin).astype(np.float32).reshape(C, HW) for c in batch]))
    z = torch.zeros((B, 1, 1), dtype=torch.float32, device="cuda")
    meta = lay["meta"].copy()
    meta[:, 2:] = (0, 1)                                  # the z support: the one symbol 0, its table the entry 0
    meta, tab_y = _dev(meta), _dev(lay["tables"])
    tab_z = torch.zeros((B, 1, Lmax), dtype=torch.int16, device="cuda")
    cap_y, cap_z = entropy._cap(C * HW // K), 8
    out = torch.zeros((B, (cap_z + K * cap_y) // 4), dtype=torch.int32, device="cuda").view(torch.uint8)
    lengths = torch.zeros((B, 1 + K), dtype=torch.int32, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    args = (_p(y), _p(z), _p(meta), _p(tab_y), _p(tab_z), Lmax, B, C, HW, 1, 1, _p(out), cap_y, cap_z, _p(lengths),
            _p(err))
    if how == "single":
        _lib.check(L.dsic_range_encode(*args, 1, pe, _stream()), "range_encode")
    else:
        nb = L.dsic_range_encode_seg_workspace_size(B, C, HW, 1, 1, K)
        ws = torch.empty(((nb + 3) // 4,), dtype=torch.int32, device="cuda")
        if how == "ws":
            _lib.check(L.dsic_range_encode_ws(*args, pe, _p(ws), ws.numel() * 4, _stream()), "range_encode_ws")
        else:
            _lib.check(L.dsic_range_encode_seg_ws(*args, pe, K, _p(ws), ws.numel() * 4, _stream()),
                       "range_encode_seg_ws")
    torch.cuda.synchronize()
    return out, lengths, int(err.item()), cap_z, cap_y


@pytest.mark.parametrize("family", D.FAMILIES)
def test_encoders_on_the_hand_made_tables(family):
    """dsic_range_encode, dsic_range_encode_ws and, where the channels divide, dsic_range_encode_seg_ws write the
    oracle's bytes and lengths with zeros behind them on tables whose intervals return to the full 2^32 and whose top
    symbol is coded; the decoder reads the encoders' own bytes back to the symbols."""
    zs = E.range_encode(np.zeros(1, np.int32), np.zeros((1, 1), np.uint16), 1)
    for batch in D.batches(family):
        C, HW, pe = _geometry(batch)
        want = [c.symbols() for c in batch]
        strings = [D.oracle_string(c) for c in batch]
        lay = D.lay_out(batch, strings, fill="random")
        for how in ("single", "ws"):
            out, lengths, err, cap_z, cap_y = _encode(batch, lay, how)
            assert err == 0, (how, batch[0].id)
            try:
                O.assert_oracle({"bytes": out, "lengths": lengths}, [(zs, s) for s in strings], cap_z)
            except AssertionError as e:
                pytest.fail(f"encoder {how}, batch of {batch[0].id}: (image, string, ...) = {e}")
            back = {"meta": lay["meta"], "tables": lay["tables"], "Lmax": lay["Lmax"],
                    "bytes": out.cpu().numpy()[:, cap_z:], "stride": cap_y,     # _dev packs the y halves
                    "lengths": lengths.cpu().numpy(), "lstride": 2, "loff": 1}
            dec, err = _decode(back, C, HW, pe)
            assert err == 0
            _assert_symbols(dec, batch, want, f"decoder on the bytes of encoder {how}")
        for K in KS:
            if C % K:
                continue
            out, lengths, err, cap_z, cap_y = _encode(batch, lay, "seg", K)
            assert err == 0
            raw, lens = out.cpu().numpy(), lengths.cpu().numpy()
            for b, c in enumerate(batch):
                assert lens[b, 0] == len(zs) and raw[b, :len(zs)].tobytes() == zs and not raw[b, len(zs):cap_z].any()
                for k, s in enumerate(_segment_strings(c, K)):
                    a = cap_z + k * cap_y
                    assert lens[b, 1 + k] == len(s), (c.id, K, k)
                    assert raw[b, a:a + len(s)].tobytes() == s, (c.id, K, k)
                    assert not raw[b, a + len(s):a + cap_y].any(), (c.id, K, k)
