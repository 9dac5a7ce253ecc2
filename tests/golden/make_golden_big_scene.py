"""Writes tests/golden/big_scene_counts.npz and big_scene_counts_more.npz: the band histograms of the large closed-form
scenes of tests/big_scene.py, streamed band by band through render_ref.histogram on the host (minutes of CPU time,
which is why they are recorded).  Two files, so that each stays under the size a committed file may have.

    python tests/golden/make_golden_big_scene.py [processes [file name]]

Each file names the constants of the pattern it was made from; test_gpu_big_images.py refuses a fixture whose
constants are not those of big_scene.py.  The band ranges follow from the histograms (first and last non-empty bin).
"""
import json
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import big_scene  # noqa: E402
import render_ref  # noqa: E402

ROWS = 64
# per file and scene the histograms recorded: name -> (with validity, with nodata)
FILES = {"big_scene_counts.npz": {"u8c3": {"plain": (False, False), "nodata": (False, True)},
                                  "u8c1v": {"plain": (False, False), "valid": (True, False)},
                                  "u16c4": {"plain": (False, False), "valid": (True, False)}},
         "big_scene_counts_more.npz": {"u8c3": {"valid": (True, False), "valid_nodata": (True, True)},
                                       "tiles16_u16": {"nodata": (False, True), "valid_nodata": (True, True)}}}


def _band(job):
    cases, name, y0, y1 = job
    scene = big_scene.table()[name]
    img = scene.band(y0, y1)
    valid = scene.valid_band(y0, y1) if scene.valid else None
    out = {}
    for case, (with_valid, with_nodata) in cases.items():
        out[case] = render_ref.histogram(img, valid if with_valid else None, scene.nodata if with_nodata else None)
    return name, out


def make(file_name, procs):
    cases = FILES[file_name]
    scenes = big_scene.table()
    jobs = [(cases[name], name, y0, min(y0 + ROWS, scenes[name].H)) for name in cases
            for y0 in range(0, scenes[name].H, ROWS)]
    total = {}
    with multiprocessing.Pool(procs) as pool:
        for k, (name, out) in enumerate(pool.imap_unordered(_band, jobs, chunksize=4)):
            for case, h in out.items():
                key = f"{name}_{case}"
                total[key] = total[key] + h if key in total else h
            if k % 200 == 0:
                print(f"{file_name}: {k} of {len(jobs)} bands", flush=True)
    arrays = {}
    for key, h in total.items():
        assert int(h.max()) < 2 ** 32
        arrays[key] = h.astype(np.uint32)
    shapes = {name: [scenes[name].H, scenes[name].W, scenes[name].C] for name in cases}
    arrays["meta"] = np.frombuffer(json.dumps({"constants": big_scene.CONSTANTS, "shapes": shapes,
                                               "nodata": {n: scenes[n].nodata for n in cases},
                                               "plants": {n: [list(map(int, q)) for q in scenes[n].plants]
                                                          for n in cases}},
                                              sort_keys=True).encode(), dtype=np.uint8)
    path = os.path.join(HERE, file_name)
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")


def main():
    procs = int(sys.argv[1]) if len(sys.argv) > 1 else min(16, os.cpu_count())
    for file_name in ([sys.argv[2]] if len(sys.argv) > 2 else FILES):
        make(file_name, procs)


if __name__ == "__main__":
    main()
