"""ResNet-18 basic-block tail, relu(bn2(z2) + avg_pool_s(bn0(z0) or x)), forward and backward at the block shapes of a 16 x 512^2 batch at
output stride 32 (slim stacks, plus the non-slim Stack's BN0 / stride-2 kind), bf16 storage, training statistics.  The fused tail
(csrc/resblock.hip) and the composed operators (ISEG_RESBLOCK_FUSED=0) are timed in the same process, alternating between them:

    python tools/kbench_resblock.py [--iters 20] [--repeats 5] [--shapes 0,3] [--json out.json]
    python tools/kbench_resblock.py --step [--json out.json]          # the graph-replayed ResNet-18 + ASPP training step, both ways
    rocprofv3 --kernel-trace --stats -d out -- python tools/kbench_resblock.py --only fused --iters 5

Per shape: forward and backward microseconds, the median of `repeats` timings of `iters` calls each (CUDA events, after three warm-ups; host
launch cost included), and the activation bytes each route moves in the forward, counted from the shapes (the statistics pass, the same in
both routes, not included).  --only runs one route, for a profiler run of its own."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (input side, C, stride, BN0 shortcut) of the ResNet-18 block tails at 512 x 512, output stride 32; the last one is the non-slim Stack's
SHAPES = [(128, 64, 1, False), (128, 64, 2, False), (64, 128, 1, True), (64, 128, 2, False), (32, 256, 1, True), (32, 256, 2, False),
          (16, 512, 1, True), (16, 512, 1, False), (128, 128, 2, True)]
ROUTES = ("fused", "composed")


def _timeit(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def _route(r):
    os.environ["ISEG_RESBLOCK_FUSED"] = "1" if r == "fused" else "0"


def fwd_bytes(N, S, C, s, bn0, esize, route):
    """activation bytes read + written by the forward after the statistics, from the shapes"""
    So = -(-S // s)
    pin, po = N * S * S * C, N * So * So * C
    if route == "fused":
        return (po + pin + po) * esize      # z2, the shortcut input, out
    b = 2 * po + 3 * po                    # bn2 apply (z2 -> a), add + relu (a, shortcut -> out)
    if bn0:
        b += 2 * pin                       # bn0 apply
    if s > 1:
        b += pin + po                      # the pool
    return b * esize


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--shapes", default="")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", choices=ROUTES, default=None)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    if a.step:
        return graphed_step(a)

    from iseg_amd import functional as F
    from iseg_amd import nn
    from iseg_amd.layers.base_layers import BatchNormalization

    nn.set_compute_dtype(torch.bfloat16)
    nn.set_device("cuda:0")
    routes = (a.only,) if a.only else ROUTES
    picks = [int(i) for i in a.shapes.split(",")] if a.shapes else range(len(SHAPES))
    rows = []
    for i in picks:
        S, C, s, bn0 = SHAPES[i]
        So = -(-S // s)
        g = torch.Generator().manual_seed(i)
        bn2 = BatchNormalization(momentum=0.9, epsilon=1.001e-5, name=f"k{i}_2_bn")
        bn2.build((C,))
        b0 = None
        if bn0:
            b0 = BatchNormalization(momentum=0.9, epsilon=1.001e-5, name=f"k{i}_0_bn")
            b0.build((C,))
        z2 = torch.randn(a.batch, So, So, C, generator=g).to(torch.bfloat16).cuda().requires_grad_(True)
        sc = torch.randn(a.batch, S, S, C, generator=g).to(torch.bfloat16).cuda().requires_grad_(True)
        dy = torch.randn(a.batch, So, So, C, generator=g).to(torch.bfloat16).cuda()
        assert F.resblock_tail_supported(z2, sc, bn2, b0, s)

        def tail():
            return F.resblock_tail(z2, bn2, sc, b0, s, True)

        def fwd():
            with torch.no_grad():
                tail()

        ys = {}
        for r in routes:
            _route(r)
            ys[r] = tail()
        times = {r: {"fwd": [], "bwd": []} for r in routes}
        for _ in range(a.repeats):
            for r in routes:      # alternate the routes within every repeat
                _route(r)
                times[r]["fwd"].append(_timeit(fwd, a.iters))
                times[r]["bwd"].append(_timeit(lambda: torch.autograd.backward(ys[r], dy, retain_graph=True), a.iters))
        row = {"side": S, "c": C, "stride": s, "bn0": bn0}
        parts = []
        for r in routes:
            tf, tb = statistics.median(times[r]["fwd"]), statistics.median(times[r]["bwd"])
            mb = fwd_bytes(a.batch, S, C, s, bn0, 2, r) / 1e6
            row.update({f"{r}_fwd_us": round(tf, 1), f"{r}_bwd_us": round(tb, 1), f"{r}_fwd_MB": round(mb, 1)})
            parts.append(f"{r} fwd {tf:.1f} us ({mb:.0f} MB) bwd {tb:.1f} us")
        rows.append(row)
        print(f"{S}x{S} C{C} s{s} {'bn0' if bn0 else 'identity'}: " + " | ".join(parts), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"batch": a.batch, "rows": rows}, f, indent=1)


def graphed_step(a):
    """ms per replayed training step of ResNet-18 + ASPP, fused and composed tails, alternating (median of `repeats` timings of `iters`
    replays).  The route is fixed when a trainer's step is captured."""
    from iseg_amd import heads
    from iseg_amd.core_env import common_env_setup
    from iseg_amd.core_optimizer import get_optimizer
    from iseg_amd.core_train import CoreTrain
    from iseg_amd.data import synthetic_batch
    from iseg_amd.graphs import GraphedTrainStep
    from iseg_amd.modelhelper import model_common_setup

    x, y = synthetic_batch(a.batch, 512, 512, seed=1)
    x, y = x.cuda(), y.cuda()
    steps = {}
    for r in ((a.only,) if a.only else ROUTES):
        _route(r)
        strategy = common_env_setup(use_one_device_strategy=True, mixed_precision=True, random_seed=3)
        model = heads.resnet18_aspp(output_stride=32, build_input_size=(512, 512), dropout_rate=0.1)
        helper = model_common_setup(model, restore_checkpoint=False)
        helper.set_optimizer(get_optimizer(strategy, initial_lr=1e-3, end_lr=0.0, epoch_steps=1000, train_epoch=1, warmup_steps=0,
                                           warmup_lr=0.0, optimizer="adamw", adamw_weight_decay=0.05, clipnorm=None))
        tm = CoreTrain(helper, None).create_trainable_model(21, ignore_label=255, batch_size=a.batch)
        step = GraphedTrainStep(tm, warmup=2)
        step(x, y)
        step(x, y)
        step(x, y)
        assert any(e.get("graph") is not None for e in step.entries.values()), "the step was never captured"
        steps[r] = step
    times = {r: [] for r in steps}
    for _ in range(a.repeats):
        for r, step in steps.items():
            times[r].append(_timeit(lambda: step(x, y), a.iters) / 1e3)
    out = {"batch": a.batch}
    for r in steps:
        t = statistics.median(times[r])
        out[f"{r}_graphed_step_ms"] = round(t, 3)
        print(f"{r} ResNet-18 + ASPP graphed training step, {a.batch} x 512^2, output stride 32: {t:.3f} ms", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
