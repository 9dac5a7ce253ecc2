"""conv_wino_bf16m: the paired against the unpaired schedule of pass B (dsic_wino_pair_chunks), alternately in one
process, at the flagship's layer shapes (B = 64, chunk-major activations): median and minimum per launch."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from dsic_amd import ops, lib
L = lib.load()
B = 64
def ev(run, n=5):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): run()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n
cases = []
for g in (128, 64, 32):
    cases.append(("s2d", g, 512))
for g, c in ((16, 192), (32, 128), (64, 128)):
    cases.append(("convT", g, c))
bias = torch.randn(128, device="cuda"); beta = torch.rand(128, device="cuda") + 0.5; gamma = torch.rand(128, device="cuda") * 0.2
for kind, g, cin in cases:
    x = ops.nhwc_to_cm16(torch.randn(B, g, g, cin, device="cuda"))
    if kind == "s2d":
        w = ops.split_wino_weight_bf16(ops.pack_wino_s2_weight(torch.randn(128, cin // 4, 5, 5, device="cuda") * 0.05), 128, cin)
        run = lambda: ops.conv3x3_wino_nhwc(x, w, bias, 128, ops.ACT_GDN, beta, gamma, s2d_in=True, cm_in=True, cm_out=True)
    else:
        w = ops.split_wino_weight_bf16(ops.pack_wino_convT_weight(torch.randn(cin, 128, 5, 5, device="cuda") * 0.05), 128, cin, 4)
        run = lambda: ops.conv_transpose2d_wino_nhwc(x, w, bias, 128, ops.ACT_IGDN, beta, gamma, cm_in=True, cm_out=True)
    for _ in range(5): run()
    torch.cuda.synchronize()
    t = {0: [], 1: []}
    for r in range(30):
        for p in (0, 1):
            L.dsic_wino_pair_chunks(p)
            t[p].append(ev(run))
    m0, m1 = np.median(t[0]), np.median(t[1])
    print(f"{kind} grid {g} Cin {cin}: unpaired {m0*1e3:8.1f} us (min {min(t[0])*1e3:.1f})  paired {m1*1e3:8.1f} us (min {min(t[1])*1e3:.1f})  ratio {m1/m0:.4f}", flush=True)
    del x
