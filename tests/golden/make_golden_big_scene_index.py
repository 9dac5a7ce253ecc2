"""Writes tests/golden/big_scene_index_counts.npz: the index histograms of the large closed-form scenes of
tests/big_scene.py, streamed band by band through index_ref.histogram on the host (minutes of CPU time, which is why they
are recorded), in the style of make_golden_big_scene.py and with its meta block.

    python tests/golden/make_golden_big_scene_index.py [processes]

Keys are <scene>_<index kind>_<case>: u8c3 with nd (0, 2) and difference (0, 2), each plain, with nodata, with validity
and with both; u16c4 with nd (3, 0) and difference (3, 0), plain and with validity.  test_gpu_big_views.py refuses a
fixture whose constants are not those of big_scene.py.
"""
import json
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import big_scene  # noqa: E402
import index_ref  # noqa: E402

ROWS = 64
FILE = "big_scene_index_counts.npz"
# per scene the indices, and the cases of each: name -> (with validity, with nodata)
INDICES = {"u8c3": (("nd", 0, 2), ("difference", 0, 2)), "u16c4": (("nd", 3, 0), ("difference", 3, 0))}
CASES = {"u8c3": {"plain": (False, False), "nodata": (False, True), "valid": (True, False), "valid_nodata": (True, True)},
         "u16c4": {"plain": (False, False), "valid": (True, False)}}


def _band(job):
    name, y0, y1 = job
    scene = big_scene.table()[name]
    img, valid = scene.band(y0, y1), scene.valid_band(y0, y1)
    out = {}
    for index in INDICES[name]:
        for case, (with_valid, with_nodata) in CASES[name].items():
            out[f"{name}_{index[0]}_{case}"] = index_ref.histogram(img, valid if with_valid else None,
                                                                   scene.nodata if with_nodata else None, index)
    return out


def main():
    procs = int(sys.argv[1]) if len(sys.argv) > 1 else min(16, os.cpu_count())
    scenes = big_scene.table()
    jobs = [(name, y0, min(y0 + ROWS, scenes[name].H)) for name in INDICES for y0 in range(0, scenes[name].H, ROWS)]
    total = {}
    with multiprocessing.Pool(procs) as pool:
        for k, out in enumerate(pool.imap_unordered(_band, jobs, chunksize=4)):
            for key, h in out.items():
                total[key] = total[key] + h if key in total else h
            if k % 200 == 0:
                print(f"{FILE}: {k} of {len(jobs)} bands", flush=True)
    arrays = {}
    for key, h in total.items():
        assert int(h.max()) < 2 ** 32
        arrays[key] = h.astype(np.uint32)
    shapes = {name: [scenes[name].H, scenes[name].W, scenes[name].C] for name in INDICES}
    arrays["meta"] = np.frombuffer(json.dumps({"constants": big_scene.CONSTANTS, "shapes": shapes,
                                               "nodata": {n: scenes[n].nodata for n in INDICES},
                                               "plants": {n: [list(map(int, q)) for q in scenes[n].plants] for n in INDICES},
                                               "indices": {n: [list(i) for i in INDICES[n]] for n in INDICES}},
                                              sort_keys=True).encode(), dtype=np.uint8)
    path = os.path.join(HERE, FILE)
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
