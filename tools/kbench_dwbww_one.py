#!/usr/bin/env python3
"""one depthwise 7 x 7 weight-gradient launch (plus its partial reduce) at the four flagship stage shapes, 16 images, us per call.
route: auto = what iseg_dwconv2d_bwd_weight picks, mfma = the matrix-core kernel (csrc/dwconv_wgrad_mfma.hip) named explicitly.
  kbench_dwbww_one.py [auto|mfma|both] [label]"""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from iseg_amd import kernels as K
def timeit(fn, iters=30, warm=3):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3
route = sys.argv[1] if len(sys.argv) > 1 else "both"
out = []
for (S, C) in [(128, 96), (64, 192), (32, 384), (16, 768)]:
    x = torch.randn(16, S, S, C, device="cuda").to(torch.bfloat16)
    dy = torch.randn(16, S, S, C, device="cuda").to(torch.bfloat16)
    dwg = torch.zeros(49, C, device="cuda"); dbg = torch.zeros(C, device="cuda")
    r = f"S{S}C{C}"
    if route in ("auto", "both"): r += f" auto {timeit(lambda: K.dwconv2d_bwd_weight(x, dy, dwg, dbg, 7, 1, 3, 3)):6.1f}"
    if route in ("mfma", "both"): r += f" mfma {timeit(lambda: K.dwconv2d7_bwd_weight_mfma(x, dy, dwg, dbg, 3, 3)):6.1f}"
    out.append(r)
print(sys.argv[2] if len(sys.argv) > 2 else "", " | ".join(out), flush=True)
