"""Resources of the image codec's byte movers (no GPU: gfx950 cross-compile with resource remarks).  They are
memory-bound kernels that run beside or between the conv kernels: none of them may spill to scratch, the band range
reduces through 128 bytes of LDS per workgroup, and the HWC movers that walk their output in 16-byte chunks (stitch,
blend finish, halving, mask apply, mask window) use no LDS at all."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "domain-specific-image-compression_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FILES = ["image_codec.hip", "image_u16.hip", "pyramid.hip", "valid.hip", "mask.hip"]

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")


def _resources(src):
    cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950",
           "-ffp-contract=off", "--cuda-device-only", f"-I{os.path.join(ROOT, 'include')}", f"-I{CSRC}", "-c",
           os.path.join(CSRC, src), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?)\s*\[-Rpass-analysis", line)
        if not m:
            continue
        body = m.group(1)
        if body.startswith("Function Name:"):
            cur = kernels.setdefault(body.split(":", 1)[1].strip(), {})
        elif cur is not None and ":" in body:
            k, v = body.split(":", 1)
            cur[k.strip()] = v.strip()
    return kernels


@pytest.fixture(scope="module")
def kernels():
    """mangled kernel name -> resources, over the five files"""
    out = {}
    for src in FILES:
        got = _resources(src)
        assert got, src
        out.update(got)
    return out


def test_no_mover_kernel_uses_scratch(kernels):
    assert len(kernels) >= 40, sorted(kernels)
    for name, res in kernels.items():
        assert int(res["ScratchSize [bytes/lane]"]) == 0, name


def test_band_range_kernels_reduce_through_128_bytes_of_lds(kernels):
    hits = {k: v for k, v in kernels.items() if "band_range_kernel" in k}
    assert len(hits) == 8, sorted(kernels)                               # C = 1 .. 4, with and without validity
    for name, res in hits.items():
        assert int(res["LDS Size [bytes/block]"]) == 128, name


@pytest.mark.parametrize("fragment,count", [("stitch_hwc_kernel", 4), ("blend_finish_hwc_kernel", 2),
                                            ("halve_kernel", 14), ("halve_u8_kernel", 3), ("mask_apply_hwc_kernel", 2),
                                            ("mask_window_u8_kernel", 1)])
def test_chunk_walk_kernels_use_no_lds(kernels, fragment, count):
    hits = {k: v for k, v in kernels.items() if fragment in k}
    assert len(hits) == count, sorted(kernels)
    for name, res in hits.items():
        assert int(res["LDS Size [bytes/block]"]) == 0, name
