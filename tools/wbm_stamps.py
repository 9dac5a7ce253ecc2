#!/usr/bin/env python3
"""Reads the in-kernel cycle stamps of a -DWBM_STAMP=1 [-DWBM_STAMP_C0=<first chunk-pass>] build of
conv_wino_bf16m.hip (diagnostic; third tile of every workgroup, medians over workgroups): the MFMA waves 0 (PQ 0)
and 4 (PQ 1) and helper wave 8, for the 32 chunk-passes from C0 on.

  LAYER=3x3 (default, 8 chunks per pass) | s2 (5x5/s2 over space-to-depth, Cin = 512: 32 chunks) | convT (8)
  CM=1     input and output chunk-major (ops.LAYOUT_CM16) instead of NHWC
  PAIR=0   the unpaired schedule of pass B (dsic_wino_pair_chunks); default: the library's setting
  C0=<n>   the WBM_STAMP_C0 the library was built with (labels only)
  PHASES=23 | 01   convT: keep the workgroups whose stamped item has one of these phases (default 23: row xi = 0 dead)
  DSIC_LIB_ROOT: the repository tree whose package (and library) to load; DSIC_LIB: the stamped library."""
import ctypes, os, sys
sys.path.insert(0, os.environ.get("DSIC_LIB_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from dsic_amd import ops, lib
B, h = 64, 128
layer = os.environ.get("LAYER", "3x3")
cm = os.environ.get("CM", "0") == "1"
c0 = int(os.environ.get("C0", "0"))
phases = {int(c) for c in os.environ.get("PHASES", "23")}
L = lib.load()
if "PAIR" in os.environ:
    L.dsic_wino_pair_chunks(int(os.environ["PAIR"]))
pair = bool(L.dsic_wino_pair_chunks(-1))
kw = dict(cm_in=True, cm_out=True) if cm else {}
cmx = (lambda t: ops.nhwc_to_cm16(t)) if cm else (lambda t: t)
bias = torch.randn(128, device="cuda"); beta = torch.rand(128, device="cuda") + 0.5; gamma = torch.rand(128, device="cuda") * 0.2
if layer == "s2":
    x = cmx(torch.randn(B, h, h, 512, device="cuda"))
    w = ops.split_wino_weight_bf16(ops.pack_wino_s2_weight(torch.randn(128, 128, 5, 5, device="cuda") * 0.05), 128, 512)
    n = 32; run = lambda: ops.conv3x3_wino_nhwc(x, w, bias, 128, ops.ACT_GDN, beta, gamma, s2d_in=True, **kw)
elif layer == "convT":
    x = cmx(torch.randn(B, h // 2, h // 2, 128, device="cuda"))
    w = ops.split_wino_weight_bf16(ops.pack_wino_convT_weight(torch.randn(128, 128, 5, 5, device="cuda") * 0.05), 128, 128, 4)
    n = 8; run = lambda: ops.conv_transpose2d_wino_nhwc(x, w, bias, 128, ops.ACT_IGDN, beta, gamma, **kw)
else:
    x = cmx(torch.randn(B, h, h, 128, device="cuda"))
    w = ops.split_wino_weight_bf16(ops.pack_wino_weight(torch.randn(128, 128, 3, 3, device="cuda") * 0.05), 128, 128)
    n = 8; run = lambda: ops.conv3x3_wino_nhwc(x, w, bias, 128, ops.ACT_GDN, beta, gamma, **kw)
for _ in range(3): run()
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record(); run(); e1.record(); torch.cuda.synchronize()
print(f"{layer} {'CM16' if cm else 'NHWC'} {'paired' if pair else 'unpaired'} pass B, stamps from chunk-pass {c0}: kernel ms {e0.elapsed_time(e1):.3f} (stamped build: shares, not length)")
buf = np.zeros(256 * 384, dtype=np.int64)
L.dsic_debug_wbm_stamps.restype = ctypes.c_int
assert L.dsic_debug_wbm_stamps(buf.ctypes.data_as(ctypes.c_void_p)) == 0
s = buf.reshape(256, 384).astype(np.float64)
s = s[s[:, 0] > 0]
if layer == "convT":
    s = s[np.isin(s[:, 127].astype(np.int64) & 3, list(phases))]
    print(f"  items of phase {sorted(phases)}: {len(s)} workgroups")
# the tile's schedule (conv_wino_pair.h): pass B runs single chunks up to pfirst, then pairs
dead = layer == "s2" or (layer == "convT" and min(phases) >= 2)
pfirst = n
if pair and layer == "s2" and n % 8 == 0: pfirst = n // 2
if pair and layer == "convT" and min(phases) >= 2 and n % 4 == 0: pfirst = 0
nb = pfirst + (n - pfirst) // 2
total = n + nb
def label(sig):
    if sig < n: return f"A {sig:2d}     "
    j = sig - n
    if j < pfirst:
        half = dead and (layer == "convT" or j >= n // 2)
        return f"B {j:2d}{' half' if half else '     '}"
    c = pfirst + 2 * (j - pfirst)
    return f"B {c:2d}+{c + 1:<2d} "
m0, hlp, m4 = s[:, :128], s[:, 128:256], s[:, 256:384]
d = lambda arr, a, b: np.median((arr[:, b] - arr[:, a]) % 2.0 ** 32)
print("chunk-pass    : PQ 0 wave 0: mfma-phase | barrier wait | gap    PQ 1 wave 4: mfma-phase | barrier wait | gap    "
      "helper wave 8: stage | commit | barrier wait | gap    period")
per = {}
for sig in range(c0, min(total, c0 + 32)):
    i = sig - c0
    nxt = sig + 1 < min(total, c0 + 32) and sig + 1 != n   # the mid fold lies between chunk-pass n - 1 and n
    row = f"  {sig:2d} {label(sig)}:"
    for arr in (m0, m4):
        row += f" {d(arr, 3*i, 3*i+1):7.0f} | {d(arr, 3*i+1, 3*i+2):7.0f} | {d(arr, 3*i+2, 3*i+3) if nxt else 0:7.0f}      "
    row += f" {d(hlp, 4*i, 4*i+1):6.0f} | {d(hlp, 4*i+1, 4*i+2):6.0f} | {d(hlp, 4*i+2, 4*i+3):6.0f} | {d(hlp, 4*i+3, 4*i+4) if nxt else 0:6.0f}"
    if nxt:
        if sig: per[sig] = d(hlp, 4 * i, 4 * i + 4)   # chunk-pass 0 waits for the MFMA waves' final fold of the tile before
        row += f"   {d(hlp, 4 * i, 4 * i + 4):6.0f}"
    print(row)
def mean_period(sel):
    v = [per[k] for k in per if sel(k)]
    return f"{np.mean(v):.0f} ({len(v)})" if v else "-"
print(f"mean period (helper wave, chunk-passes stamped): pass A {mean_period(lambda k: k < n)}; "
      f"pass B full {mean_period(lambda k: k >= n and 'half' not in label(k) and '+' not in label(k))}; "
      f"pass B half-empty, single {mean_period(lambda k: 'half' in label(k))}; pass B paired {mean_period(lambda k: '+' in label(k))}")
if c0 + 32 >= total:
    print(f"final fold (no barrier): PQ 0 {d(m0, 120, 121):6.0f}  PQ 1 {d(m4, 120, 121):6.0f}")
if c0 <= n - 1 < c0 + 32:
    i = n - 1 - c0
    print(f"mid fold (PQ 0): compute+write m0 {d(m0, 3*i+2, 122):6.0f} | M1 wait {d(m0, 122, 123):6.0f} | read+init+M2+write m1 {d(m0, 123, 124):6.0f} | M3 wait {d(m0, 124, 125):6.0f} | read+init+M4 {d(m0, 125, 126):6.0f}")
