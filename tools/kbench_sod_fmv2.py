#!/usr/bin/env python3
"""One update_state of a TFFmeasureV2 evaluator with all ten handlers at 16 x 512 x 512, fp32 prediction and uint8 prediction under normalize,
with dynamic + adaptive + binary modes and with the dynamic mode alone.  Three routes, interleaved round by round in one process, device
events around a warm loop, medians and the min..max spread:
  fused      csrc/sod_fmv2.hip (one call of iseg_sod_fmv2)
  composed   ISEG_SODFMV2_FUSED=0 (bincount, cumsum, masked counts, image by image)
  yardstick  what the package offered before this kernel: kernels.sod_metrics(wfm=False, want_ints=True) for the histograms and adaptive counts,
             torch ops for the p > 0.5 counts, and the handler formulas on the [B, 256] count tensors
The fraction of HBM bandwidth is bytes of pred + gt read (once, or twice when the adaptive mode adds the second pass of the fp32 route) over
the fused time, against the 8 TB/s peak.
usage: python3 tools/kbench_sod_fmv2.py [rounds] [iters per round] [--json PATH] [--small]"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import iseg_amd.metrics.sod as sod  # noqa: E402
from iseg_amd import kernels as K  # noqa: E402
from iseg_amd.metrics.sod import fmeasurev2 as F  # noqa: E402
from iseg_amd.metrics.sod import sod_metric_utils as U  # noqa: E402

HBM_PEAK = 8.0e12
args = [a for a in sys.argv[1:] if not a.startswith("--") and not a.endswith(".json")]
rounds = int(args[0]) if len(args) > 0 else 5
iters = int(args[1]) if len(args) > 1 else 20
B, H, W = (2, 64, 64) if "--small" in sys.argv else (16, 512, 512)
CLASSES = ("TFIOUHandler", "TFSpecificityHandler", "TFDICEHandler", "TFOverallAccuracyHandler", "TFKappaHandler", "TFPrecisionHandler",
           "TFRecallHandler", "TFFPRHandler", "TFBERHandler", "TFFmeasureHandler")


def inputs(B, H, W):
    """a near-binary saliency-like map: ~90 % of the pixels exactly 0 or 1, blobby gt; and its grey-level version"""
    g = torch.Generator(device="cuda").manual_seed(0)
    coarse = torch.rand(B, 1, H // 8, W // 8, device="cuda", generator=g)
    gt = torch.nn.functional.interpolate(coarse, size=(H, W), mode="nearest")[:, 0] < 0.3
    p = gt.float()
    wrong = torch.rand(B, H, W, device="cuda", generator=g) < 0.04
    p = torch.where(wrong, 1.0 - p, p)
    soft = torch.rand(B, H, W, device="cuda", generator=g) < 0.1
    p = torch.where(soft, torch.rand(B, H, W, device="cuda", generator=g), p)
    u = (p * 200.0 + 20.0 + torch.randint(0, 6, (B, H, W), device="cuda", generator=g)).clamp(0, 255).to(torch.uint8)
    g8 = torch.where(gt, torch.randint(129, 256, (B, H, W), device="cuda", generator=g), torch.randint(0, 129, (B, H, W), device="cuda", generator=g))
    return p.contiguous(), gt.contiguous(), u.contiguous(), g8.to(torch.uint8).contiguous()


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3      # us per call


def yardstick(pred, gt, normalize, table, state, count):
    """the same [n, 264] state from iseg_sod_metrics' integers and tensor ops"""
    ints, _, _, _ = K.sod_metrics(pred, gt, normalize=normalize, wfm=False, want_ints=True)
    ints = ints.to(torch.int64)
    p, g = U.prepare_data(pred, gt) if normalize else (pred, gt)
    hi = p > 0.5
    size = pred.shape[1] * pred.shape[2]
    FG = ints[:, 512]
    BG = size - FG

    def four(tp, pos):
        fg, bg = (FG, BG) if tp.dim() == 1 else (FG[:, None], BG[:, None])
        fp = pos - tp
        return tp, fp, bg - fp, fg - tp

    tps = torch.cumsum(torch.flip(ints[:, :256], [1]), 1)
    pos = tps + torch.cumsum(torch.flip(ints[:, 256:512], [1]), 1)
    dyn = four(tps, pos)
    adp = four(ints[:, 514], ints[:, 513])
    bny = four((hi & g).sum((1, 2)), hi.sum((1, 2)))
    for h, (kind, modes, beta) in enumerate(table):
        if modes & F.DYNAMIC:
            state[h, :256] += F.metric_on_counts(kind, beta, *dyn).sum(0)
        if modes & F.ADAPTIVE:
            state[h, 256] += F.metric_on_counts(kind, beta, *adp).sum()
        if modes & F.BINARY:
            state[h, 257] += F.metric_on_counts(kind, beta, *bny).sum()
            state[h, 258:262] += torch.stack(bny).to(torch.float64).sum(1)
    count += pred.shape[0]


res = {"rounds": rounds, "iters": iters, "shape": f"{B}x{H}x{W}", "arms": {}}
P, G, U8, G8 = inputs(B, H, W)
for dtype, (pred, gt, normalize) in {"fp32": (P, G, False), "uint8_normalize": (U8, G8, True)}.items():
    for modes_name, (dy, ad, bi) in {"dynamic+adaptive+binary": (True, True, True), "dynamic": (True, False, False)}.items():
        ev = sod.TFFmeasureV2({c: getattr(sod, c)(dy, ad, with_binary=bi) for c in CLASSES})
        ev_c = sod.TFFmeasureV2({c: getattr(sod, c)(dy, ad, with_binary=bi) for c in CLASSES})
        table = ev._table()
        ystate, ycount = torch.zeros_like(ev.state), torch.zeros_like(ev.count)

        def fused():
            os.environ["ISEG_SODFMV2_FUSED"] = "1"
            ev.update_state(pred, gt, normalize=normalize)

        def composed():
            os.environ["ISEG_SODFMV2_FUSED"] = "0"
            ev_c.update_state(pred, gt, normalize=normalize)

        def yard():
            yardstick(pred, gt, normalize, table, ystate, ycount)

        arms = {"fused": (fused, iters), "yardstick": (yard, max(1, iters // 4)), "composed": (composed, 1)}
        for fn, _ in arms.values():
            fn()
        torch.cuda.synchronize()
        # the three routes agree before they are timed
        assert int(ev.count) == int(ev_c.count) == int(ycount) == B
        assert float((ev.state - ev_c.state).abs().max()) < 1e-9 * B and float((ev.state - ystate).abs().max()) < 1e-9 * B
        times = {k: [] for k in arms}
        for _ in range(rounds):
            for k, (fn, n) in arms.items():
                times[k].append(timed(fn, n))
        os.environ["ISEG_SODFMV2_FUSED"] = "1"
        r = {k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for k, v in times.items()}
        passes = 1 if normalize or not ad else 2
        r["bytes_read"] = passes * B * H * W * (2 if normalize else 5)
        r["fused_hbm_fraction"] = r["bytes_read"] / (r["fused"]["median_us"] * 1e-6) / HBM_PEAK
        r["yardstick_over_fused"] = r["yardstick"]["median_us"] / r["fused"]["median_us"]
        r["composed_over_fused"] = r["composed"]["median_us"] / r["fused"]["median_us"]
        res["arms"][f"{dtype} {modes_name}"] = r
        print(f"{B} x {H} x {W} {dtype}, ten handlers, {modes_name}")
        for k in arms:
            print(f"  {k:10s} median {r[k]['median_us']:12.1f} us   min {r[k]['min_us']:12.1f}   max {r[k]['max_us']:12.1f}")
        print(f"  yardstick / fused = {r['yardstick_over_fused']:.2f} x   composed / fused = {r['composed_over_fused']:.1f} x")
        print(f"  fused reads {r['bytes_read'] / 1e6:.1f} MB of pred + gt in {passes} pass(es): {100 * r['fused_hbm_fraction']:.1f} % of the 8 TB/s HBM peak")
for a in sys.argv:
    if a == "--json":
        path = sys.argv[sys.argv.index(a) + 1]
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        json.dump(res, open(path, "w"), indent=1)
