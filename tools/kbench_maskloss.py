#!/usr/bin/env python3
"""MaskLoss at the flagship logits shape (16 x 512 x 512, 21 classes, fp32, 10 % ignored): loss + gradient from the fused kernels
(csrc/mask_loss.hip) against the composed route (ISEG_MASKLOSS_FUSED=0) and against the ignore-label cross-entropy kernel (loss + gradient)
on the same tensor.  The arms are interleaved round by round in one process; medians and the min..max spread are reported.
usage: python3 tools/kbench_maskloss.py [rounds] [iters per round] [--json PATH] [--small]"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from iseg_amd import functional as F  # noqa: E402
from iseg_amd.losses.mask_loss import MaskLoss  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
rounds = int(args[0]) if len(args) > 0 else 7
iters = int(args[1]) if len(args) > 1 else 10
N, H, W, C = (2, 64, 64, 21) if "--small" in sys.argv else (16, 512, 512, 21)
g = torch.Generator(device="cuda").manual_seed(0)
z = (torch.randn(N, H, W, C, device="cuda", generator=g) * 4).clamp_(-12, 12)
y = torch.randint(0, C, (N, H, W), dtype=torch.int32, device="cuda", generator=g)
y[torch.rand(N, H, W, device="cuda", generator=g) < 0.1] = 255
loss = MaskLoss(num_class=C, ignore_label=255)
logits_bytes = z.numel() * 4


def fused():
    os.environ["ISEG_MASKLOSS_FUSED"] = "1"
    zz = z.detach().requires_grad_(True)
    with F.unit_loss_grad():      # as Trainer.train_step differentiates its losses
        loss.fused_mean(y, zz).backward()
    return zz.grad


def composed():
    os.environ["ISEG_MASKLOSS_FUSED"] = "0"
    zz = z.detach().requires_grad_(True)
    with F.unit_loss_grad():      # as Trainer.train_step differentiates its losses
        loss.fused_mean(y, zz).backward()
    return zz.grad


def ce():
    zz = z.detach().requires_grad_(True)
    with F.unit_loss_grad():
        F.softmax_ce_mean(zz, y, C, 255).backward()
    return zz.grad


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3      # us per call


arms = {"fused": fused, "composed": composed, "ce": ce}
for fn in arms.values():      # warm-up: code objects, workspaces, the allocator's blocks
    for _ in range(3):
        fn()
torch.cuda.synchronize()
times = {k: [] for k in arms}
for _ in range(rounds):
    for k, fn in arms.items():
        times[k].append(timed(fn))
os.environ["ISEG_MASKLOSS_FUSED"] = "1"
res = {"shape": [N, H, W, C], "rounds": rounds, "iters": iters}
for k, v in times.items():
    res[k] = {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)}
    print(f"{k:9s} median {res[k]['median_us']:9.1f} us   min {min(v):9.1f}   max {max(v):9.1f}")
mf, mc, me = (res[k]["median_us"] for k in ("fused", "composed", "ce"))
res["composed_over_fused"] = mc / mf
res["fused_over_ce"] = mf / me
res["fused_bytes"] = 3 * logits_bytes
res["fused_TBps"] = 3 * logits_bytes / mf * 1e-6
res["ce_TBps"] = 2 * logits_bytes / me * 1e-6
print(f"composed / fused = {mc / mf:.2f} x;  fused / CE kernel = {mf / me:.2f} x")
print(f"fused: {3 * logits_bytes / 1e9:.2f} GB of logits traffic (2 reads + 1 write) -> {res['fused_TBps']:.2f} TB/s;  "
      f"CE: {2 * logits_bytes / 1e9:.2f} GB -> {res['ce_TBps']:.2f} TB/s   (6.3 TB/s: achievable HBM streaming rate)")
for a in sys.argv:
    if a == "--json":
        path = sys.argv[sys.argv.index(a) + 1]
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        json.dump(res, open(path, "w"), indent=1)
