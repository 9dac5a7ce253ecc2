"""The recipes of tests/stream_cases.py against include/dsic_hip.h, without a GPU: every export that takes a stream has
a recipe, the two input sets of a recipe are two different, equally shaped, equally legal sets, and the last error is
each thread's own."""
import ctypes
import os
import re
import threading

import numpy as np
import pytest

import stream_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# dsic_stream_destroy(void* stream) ends in a stream too, but that is the object it destroys, not a stream it works
# on; it belongs to the CU-masked streams, which have no recipe
NO_WORK = {"dsic_stream_destroy"}


def _prototypes():
    text = open(os.path.join(ROOT, "include", "dsic_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.findall(r"\b(dsic_\w+)\s*\(([^;{]*?)\)\s*;", text)


def _stream_exports():
    return {n for n, args in _prototypes() if re.search(r"void\s*\*\s*stream\s*$", args.strip())}


@pytest.fixture(scope="module")
def L():
    from dsic_amd import lib
    return lib.load()


def test_every_export_that_takes_a_stream_has_a_recipe(L):
    every = {n for n, _ in _prototypes()}
    streamed = _stream_exports()
    from dsic_amd import lib
    assert every == set(lib.SIGNATURES), "the prototypes parsed from the header are not the exports lib.py binds"
    assert len(streamed) >= 104 and NO_WORK <= streamed, len(streamed)      # 104 when this test was written
    named = set()
    for name in SC.names():
        named |= set(SC.build(name, L).exports)
    assert not named - every, f"recipes name exports the header does not have: {sorted(named - every)}"
    assert not named - streamed, f"recipes name exports that take no stream: {sorted(named - streamed)}"
    missing = streamed - named - NO_WORK
    assert not missing, f"exports that take a stream and have no recipe in tests/stream_cases.py: {sorted(missing)}"
    assert len(SC.names()) == len(set(SC.names()))
    for name in SC.names():
        SC.family(name)                          # every recipe belongs to a family of the DESIGN.md table


@pytest.mark.parametrize("name", SC.names())
def test_the_two_input_sets_are_two_equally_legal_sets(name, L):
    c = SC.build(name, L)
    if c.reach:
        c.reach(L)                               # host-side predicates and restated launch counts
    a, b = c.inputs("A"), c.inputs("B")
    assert a and c.judged(), name
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (name, k)
        if a[k].dtype.kind == "f":
            assert np.isfinite(a[k]).all() and np.isfinite(b[k]).all(), (name, k)
    assert any(a[k].tobytes() != b[k].tobytes() for k in a), f"{name}: A and B are the same bytes"
    for k, buf in c.bufs.items():
        if buf["kind"] == "in" and buf["bound"] is not None:
            lo, hi = buf["bound"]
            for w in ("A", "B"):
                v = buf[w]
                assert v.dtype.kind in "iu" and int(v.min()) >= lo and int(v.max()) < hi, (name, k, w, lo, hi)
    # buffers of a call are separate objects: no name is both an input and an output unless the call works in place
    assert all(b["kind"] in ("in", "out", "work") for b in c.bufs.values())
    if c.restate:
        assert c.restate(a) != c.restate(b), f"{name}: the restated outputs of A and B are equal"


def test_index_arrays_that_must_agree_are_one_array_in_both_sets(L):
    """a support with its tables, a popcount with its plane, ascending tile ids: the same values in A and B, so a
    kernel that reads one of them late still reads a pair that belongs together"""
    for name, keys in (("range_encode", ["meta"]), ("range_encode_ws", ["meta"]), ("range_encode_seg_ws", ["meta"]),
                       ("range_decode", ["meta"]), ("range_decode_seg", ["meta"]), ("mask_pack", ["pop", "ids"]),
                       ("mask_unpack", ["desc"]), ("tile_blend_window_f32", ["ids"]),
                       ("residual_pack", ["meta"]), ("residual_pack_u16", ["meta", "k"]),
                       ("container_scatter", []), ("strings_scatter_select", [])):
        c = SC.build(name, L)
        for k in keys:
            assert c.bufs[k]["A"].tobytes() == c.bufs[k]["B"].tobytes(), (name, k)
    # the coder's symbols lie inside the one support, under either set's tables
    for name in ("range_encode", "range_encode_ws", "range_encode_seg_ws"):
        c = SC.build(name, L)
        ymin, Ly, zmin, Lz = SC.CODER["meta"]
        for w in ("A", "B"):
            y, z = c.bufs["y"][w], c.bufs["z"][w]
            assert ymin <= y.min() and y.max() < ymin + Ly and zmin <= z.min() and z.max() < zmin + Lz
            for tab, n in ((c.bufs["tab_y"][w], Ly), (c.bufs["tab_z"][w], Lz)):
                t = tab[:, :n].astype(np.int64)
                assert (t[:, 0] == 0).all() and (np.diff(t, axis=1) > 0).all() and (t[:, -1] < 65536).all()
    # the two containers of the scatter recipes carry the same records' lengths at the same places
    for name in ("container_scatter", "strings_scatter_select"):
        c = SC.build(name, L)
        A, B = c.bufs["blob"]["A"], c.bufs["blob"]["B"]
        for b in range(3):
            at = 38 + 24 * b + 16
            assert A[at:at + 8].tobytes() == B[at:at + 8].tobytes()
    # equal popcounts, other planes
    c = SC.build("mask_pack", L)
    pa, pb = c.bufs["planes"]["A"], c.bufs["planes"]["B"]
    count = lambda p: np.unpackbits(p.view(np.uint8).reshape(len(p), -1), axis=1).sum(1)
    assert (count(pa) == c.bufs["pop"]["A"]).all() and (count(pb) == c.bufs["pop"]["A"]).all()


# ---- dsic_last_error is per thread ------------------------------------------------------------------------------
def _refuse_round(L):
    return L.dsic_round(None, None, 5, None)


def _refuse_wino(L):
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    return L.dsic_conv3x3_wino_nhwc(p, p, p, p, p, p, 1, 16, 16, 48, 128, 0, 0, 0, p, None)


def test_last_error_is_each_threads_own(L):
    """Refusals return before the first HIP call, so no device is needed; ctypes releases the GIL around each call,
    so the two threads really interleave inside the library."""
    want = {}
    for key, fn in (("round", _refuse_round), ("wino", _refuse_wino)):
        assert fn(L) == 1
        want[key] = L.dsic_last_error()
    assert want["round"] and want["wino"] and want["round"] != want["wino"]
    wrong, start = {"round": [], "wino": []}, threading.Barrier(2)

    def run(key, fn):
        start.wait()
        for i in range(2000):
            status = fn(L)
            msg = L.dsic_last_error()
            if status != 1 or msg != want[key]:
                wrong[key].append((i, status, msg))

    threads = [threading.Thread(target=run, args=(k, f)) for k, f in (("round", _refuse_round), ("wino", _refuse_wino))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not wrong["round"] and not wrong["wino"], (wrong["round"][:3], wrong["wino"][:3])
