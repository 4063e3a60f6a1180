#!/usr/bin/env python3
"""One update_state of all five SOD metrics (a SodMetricSet) at 16 x 512 x 512 and 4 x 1024 x 1024, fp32 prediction and bool gt: the fused
kernels (csrc/sod_metrics.hip) against the composed route (ISEG_SODMETRICS_FUSED=0), and the fused route without the weighted F-measure (the
two streaming passes + finalize alone).  The arms are interleaved round by round in one process; medians and the min..max spread are reported.
A last arm times the distance transform's worst case, one foreground pixel at 1024 x 1024.
usage: python3 tools/kbench_sod_metrics.py [rounds] [iters per round] [--json PATH] [--small] [--fused-only]"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from iseg_amd.metrics.sod import (SodMetricSet, TFEmeasureMetric, TFFmeasureMetric, TFMAEMetric, TFSmeasureMetric,  # noqa: E402
                                  TFWeightedFmeasureMetric)

args = [a for a in sys.argv[1:] if not a.startswith("--") and not a.endswith(".json")]
rounds = int(args[0]) if len(args) > 0 else 5
iters = int(args[1]) if len(args) > 1 else 5
shapes = [(2, 64, 64)] if "--small" in sys.argv else [(16, 512, 512), (4, 1024, 1024)]


def inputs(B, H, W):
    """a near-binary saliency-like map: ~90 % of the pixels exactly 0 or 1, blobby gt"""
    g = torch.Generator(device="cuda").manual_seed(0)
    coarse = torch.rand(B, 1, H // 8, W // 8, device="cuda", generator=g)
    gt = torch.nn.functional.interpolate(coarse, size=(H, W), mode="nearest")[:, 0] < 0.3
    p = gt.float()
    wrong = torch.rand(B, H, W, device="cuda", generator=g) < 0.04
    p = torch.where(wrong, 1.0 - p, p)
    soft = torch.rand(B, H, W, device="cuda", generator=g) < 0.1
    p = torch.where(soft, torch.rand(B, H, W, device="cuda", generator=g), p)
    return p.contiguous(), gt.contiguous()


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3      # us per call


res = {"rounds": rounds, "iters": iters, "shapes": {}}
for B, H, W in shapes:
    P, G = inputs(B, H, W)
    full = SodMetricSet(TFMAEMetric(), TFSmeasureMetric(), TFEmeasureMetric(), TFFmeasureMetric(), TFWeightedFmeasureMetric())
    nowfm = SodMetricSet(TFMAEMetric(), TFSmeasureMetric(), TFEmeasureMetric(), TFFmeasureMetric())

    def fused():
        os.environ["ISEG_SODMETRICS_FUSED"] = "1"
        full.update_state(P, G)

    def fused_nowfm():
        os.environ["ISEG_SODMETRICS_FUSED"] = "1"
        nowfm.update_state(P, G)

    def composed():
        os.environ["ISEG_SODMETRICS_FUSED"] = "0"
        full.update_state(P, G)

    arms = {"fused": (fused, iters), "fused_without_wfm": (fused_nowfm, iters)}
    if "--fused-only" not in sys.argv:
        arms["composed"] = (composed, 1)      # seconds per call: one call per round
    for fn, _ in arms.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(rounds):
        for k, (fn, n) in arms.items():
            times[k].append(timed(fn, n))
    os.environ["ISEG_SODMETRICS_FUSED"] = "1"
    r = {k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for k, v in times.items()}
    px = B * H * W
    r["two_pass_bytes"] = 2 * 5 * px      # passes A and B: 4 B of pred + 1 B of gt per pixel, each
    if "composed" in r:
        r["composed_over_fused"] = r["composed"]["median_us"] / r["fused"]["median_us"]
    res["shapes"][f"{B}x{H}x{W}"] = r
    print(f"{B} x {H} x {W}")
    for k in arms:
        print(f"  {k:18s} median {r[k]['median_us']:12.1f} us   min {r[k]['min_us']:12.1f}   max {r[k]['max_us']:12.1f}")
    if "composed" in r:
        print(f"  composed / fused = {r['composed_over_fused']:.1f} x")
    print(f"  passes A + B move {r['two_pass_bytes'] / 1e6:.1f} MB of pred + gt")
if "--small" not in sys.argv:
    # the row pass of the distance transform scans outward from every pixel up to its nearest foreground pixel: one foreground pixel in a corner
    # of a 1024 x 1024 image is its worst case at this size
    Ps = torch.zeros(1, 1024, 1024, device="cuda")
    Gs = torch.zeros(1, 1024, 1024, dtype=torch.bool, device="cuda")
    Gs[0, 0, 0] = True
    sparse = SodMetricSet(TFWeightedFmeasureMetric())
    os.environ["ISEG_SODMETRICS_FUSED"] = "1"
    sparse.update_state(Ps, Gs)
    torch.cuda.synchronize()
    v = [timed(lambda: sparse.update_state(Ps, Gs), iters) for _ in range(rounds)]
    res["sparse_1x1024x1024_one_fg_pixel"] = {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)}
    print(f"1 x 1024 x 1024, one foreground pixel (weighted F only): median {statistics.median(v):.1f} us   min {min(v):.1f}   max {max(v):.1f}")
for a in sys.argv:
    if a == "--json":
        path = sys.argv[sys.argv.index(a) + 1]
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        json.dump(res, open(path, "w"), indent=1)
