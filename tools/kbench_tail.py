#!/usr/bin/env python3
"""Logits tail of the flagship step (16 x 512 x 512, 21 classes, logits at 16 x 16): the fused upsample + CE + gradient + confusion kernel
against the three separate kernels, and the OHEM tail (use_ohem: materialised logits, per-position loss, labelled-class probabilities, radix
select with the masked mean, loss kernel again with grad_px = keep, resize gradient).  usage: python3 tools/kbench_tail.py [iters] [rounds]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from iseg_amd import kernels as K  # noqa: E402

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
N, Hi, Wi, C, Ho, Wo = 16, 16, 16, 21, 512, 512
z = (torch.randn(N, Hi, Wi, C, device="cuda") * 2).to(torch.bfloat16)
y = torch.randint(0, C, (N, Ho, Wo), dtype=torch.int32, device="cuda")
y[torch.rand(N, Ho, Wo, device="cuda") < 0.1] = 255
cm = torch.zeros(C * C, dtype=torch.int64, device="cuda")
P = N * Ho * Wo


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


def separate():
    full = K.resize_bilinear(z, Ho, Wo, out_dtype=torch.float32)
    _, s, dl = K.softmax_ce_ignore(full.reshape(-1, C), y.reshape(-1), 255, want_px=False, want_sum=True, sum_scale=1.0 / P, want_grad=True,
                                   grad_scale=1.0 / P, cm=cm)
    return K.resize_bilinear_bwd(dl.reshape(N, Ho, Wo, C), Hi, Wi, torch.bfloat16)


def ohem(thresh=0.7, min_kept_total=100000 * N):
    full = K.resize_bilinear(z, Ho, Wo, out_dtype=torch.float32).reshape(-1, C)
    yf = y.reshape(-1)
    px, _, _ = K.softmax_ce_ignore(full, yf, 255, want_px=True, cm=cm)
    prob = K.ohem_label_prob(full, yf, 255)
    keep, _, s, _, _ = K.ohem_select(prob, px, min_kept_total, thresh, want_sum=True, sum_scale=1.0 / P)
    _, _, dl = K.softmax_ce_ignore(full, yf, 255, want_px=False, want_grad=True, grad_scale=1.0 / P, grad_px=keep)
    return K.resize_bilinear_bwd(dl.reshape(N, Ho, Wo, C), Hi, Wi, torch.bfloat16)


def ohem_select_only(prob, px):
    return K.ohem_select(prob, px, 100000 * N, 0.7, want_sum=True, sum_scale=1.0 / P)


full = K.resize_bilinear(z, Ho, Wo, out_dtype=torch.float32).reshape(-1, C)
px = K.softmax_ce_ignore(full, y.reshape(-1), 255, want_px=True)[0]
prob = K.ohem_label_prob(full, y.reshape(-1), 255)
for r in range(rounds):      # the routes alternate inside one process: the spread between rounds is the noise of the comparison
    tf = timeit(lambda: K.upsample_ce(z, y, Ho, Wo, 255, sum_scale=1.0 / P, grad_scale=1.0 / P, cm=cm))
    ts = timeit(separate)
    to = timeit(ohem)
    tp = timeit(lambda: K.ohem_label_prob(full, y.reshape(-1), 255))
    tsel = timeit(lambda: ohem_select_only(prob, px))
    print(f"round {r}: fused tail {tf:.1f} us ({(P * 4 + N * Hi * Wi * C * 4) / tf * 1e-3:.0f} GB/s of labels + logits), three kernels {ts:.1f} us, "
          f"OHEM tail {to:.1f} us (label_prob {tp:.1f} us, select of {P} values {tsel:.1f} us)")
