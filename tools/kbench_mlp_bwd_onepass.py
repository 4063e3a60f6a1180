#!/usr/bin/env python3
"""Backward pass of the fused ConvNeXt MLP at the flagship stage-0 shape (M = 262144, C = 96) in isolation: the pair of kernels (data-gradient
chain through the LayerNorm backward + recomputing weight-gradient kernel, each with its reductions) against the one-pass kernel
(csrc/mlp_bwd_onepass.hip) that forms the hidden tile once.
usage: python3 tools/kbench_mlp_bwd_onepass.py [iters]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from iseg_amd import kernels as K  # noqa: E402

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20


def timeit(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


S, C = 128, 96
M = 16 * S * S
bf = torch.bfloat16
y1 = (torch.randn(M, C, device="cuda") * 1.7 + 0.3).to(bf)
dy = torch.randn(M, C, device="cuda").to(bf)
W1 = torch.randn(C, 4 * C, device="cuda") / C ** 0.5
W2 = torch.randn(4 * C, C, device="cuda") / (4 * C) ** 0.5
b1 = torch.randn(4 * C, device="cuda") * 0.1
b2 = torch.randn(C, device="cuda") * 0.1
gamma = torch.rand(C, device="cuda") + 0.5
lng, lnb = torch.rand(C, device="cuda") + 0.5, torch.randn(C, device="cuda") * 0.2
rs = torch.ones(16, device="cuda")
_, mean, rstd = K.layernorm_fwd(y1, lng, lnb, 1e-6)
ln = (mean, rstd, lng, lnb)
fw, bw = K.convnext_mlp_prep(W1, W2, gamma)
gW1, gb1, gW2, gb2, gg, glg, glb = (torch.zeros(s, device="cuda") for s in ((C, 4 * C), (4 * C,), (4 * C, C), (C,), (C,), (C,), (C,)))

t_data = timeit(lambda: K.convnext_mlp_bwd_data_ln(y1, dy, bw, b1, ln, glg, glb, rs, S * S))
t_wg = timeit(lambda: K.convnext_mlp_wgrad(y1, dy, bw, b1, W2, b2, gamma, gW1, gb1, gW2, gb2, gg, rs, S * S, ln=ln))
t_one = timeit(lambda: K.convnext_mlp_bwd_onepass(y1, dy, bw, b1, W2, b2, gamma, ln, glg, glb, gW1, gb1, gW2, gb2, gg, rs, S * S))
print(f"C={C} M={M}: chain + LayerNorm backward {t_data:.1f} us + weight gradients {t_wg:.1f} us = {t_data + t_wg:.1f} us | one pass {t_one:.1f} us"
      " (each with its reduction and finish launches)")
