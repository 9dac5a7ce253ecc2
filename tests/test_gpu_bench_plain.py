"""bench.py without --full: the result line of the headline figure alone (no `roofline`, no CPU baseline), and
--dump-outputs: what the last timed step computed, as .npy files that agree with the line's means."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    out_dir = tmp_path / "outputs"
    r = subprocess.run([sys.executable, "bench.py", "--steps", "3", "--warmup", "2", "--dump-outputs", str(out_dir)],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 2 and d["unit"] == "images/s" and d["higher_is_better"] is True
    assert d["value"] > 0 and d["dtype"].startswith("f32")
    assert abs(d["ms_per_step"] - 64 / d["value"] * 1e3) < 1e-6 * d["ms_per_step"]     # batch 64, one GPU
    assert d["roofline"] is None and "cpu_baseline" not in d

    files = {f[:-4]: np.load(out_dir / f) for f in os.listdir(out_dir)}
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= 64 * 10**6
    idx = files["image_index"].astype(np.int64)
    assert len(idx) == 8 and np.all(np.diff(idx) > 0) and idx[-1] < 64
    assert files["x_hat"].shape == (8, 3, 256, 256) and files["y_tilde"].shape == (8, 192, 16, 16)
    assert np.array_equal(np.round(files["y_tilde"]), files["y_tilde"])
    assert files["bpp"].shape == (64,) and files["metric_sums"][2] == 64
    assert abs(files["bpp"].mean() - d["mean_bpp"]) < 1e-9
    assert abs(files["ms_ssim"].astype(np.float64).mean() - d["mean_ms_ssim"]) < 1e-7
    lengths = files["string_lengths"]
    assert abs(lengths.sum() * 8.0 / (256 * 256) / 64 - d["mean_bpp_coded"]) < 1e-9
    y_len = lengths[idx, 1].astype(np.int64)
    assert files["y_strings"].shape[1] >= y_len.max() and files["y_strings"][0, :y_len[0]].any()
