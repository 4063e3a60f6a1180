"""Xception separable unit (relu -> depthwise 3 x 3 -> BN -> pointwise 1 x 1, the pointwise output before its BN) forward and backward at the
distinct unit shapes of a 16 x 512^2 batch at output stride 16, bf16 storage, training statistics.  One variant per process, chosen by
ISEG_SEPCONV_FUSED (1 = csrc/sepconv.hip, 0 = the composed operators), so a rocprofv3 --kernel-trace run, or a FETCH_SIZE / WRITE_SIZE counter
run of its own, can wrap it:

    ISEG_SEPCONV_FUSED=1 python tools/kbench_sepconv.py [--iters 20] [--shapes 0,3] [--json out.json]
    ISEG_SEPCONV_FUSED=0 rocprofv3 --kernel-trace --stats -d out -- python tools/kbench_sepconv.py --iters 5

Prints one line per shape: forward and backward microseconds, the median of `repeats` timings of `iters` calls each (CUDA events, after three
warm-ups; host launch cost included).  --step instead times the whole Xception-65 + ASPP training step (512 x 512, output stride 16, bf16,
AdamW) replayed as one HIP graph by graphs.GraphedTrainStep, which takes the host launch cost out."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (input side, Cin, Cout, stride, dilation) of the activation=False units of Xception-65 at 512 x 512, output stride 16
SHAPES = [(256, 64, 128, 1, 1), (256, 128, 128, 1, 1), (256, 128, 128, 2, 1), (128, 128, 256, 1, 1), (128, 256, 256, 2, 1),
          (64, 256, 728, 1, 1), (64, 728, 728, 2, 1), (32, 728, 728, 1, 1), (32, 728, 1024, 1, 1), (32, 1024, 1024, 1, 1)]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--shapes", default="")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    if a.step:
        return graphed_step(a)

    from iseg_amd import functional as F
    from iseg_amd import nn
    from iseg_amd.backbones.xception import XceptionDepthWiseConv
    from iseg_amd.kernels import same_pad
    from iseg_amd.param_store import ParamStore

    nn.set_compute_dtype(torch.bfloat16)
    nn.set_device("cuda:0")
    fused = F.sepconv_fused_enabled()
    picks = [int(i) for i in a.shapes.split(",")] if a.shapes else range(len(SHAPES))
    rows = []
    for i in picks:
        S, Cin, Cout, s, d = SHAPES[i]
        u = XceptionDepthWiseConv(90 + i, 1, Cout, strides=(s, s))
        u.atrous_rates = (d, d)
        u.build((1, 1, 1, Cin))
        dw, bn, pw = u.depthwise_conv, u.depthwise_bn, u.pointwise_conv
        ParamStore([dw.depthwise_kernel, bn.gamma, bn.beta, pw.kernel])
        g = torch.Generator().manual_seed(i)
        So = same_pad(S, 3, s, d)[0]
        x = torch.randn(a.batch, S, S, Cin, generator=g).to(torch.bfloat16).cuda().requires_grad_(True)
        dy = torch.randn(a.batch, So, So, Cout, generator=g).to(torch.bfloat16).cuda()
        assert (not fused) or F.sepconv_supported(x, dw.depthwise_kernel, bn, pw.kernel, s, d)
        rep = lambda fn: statistics.median(_timeit(fn, a.iters) for _ in range(a.repeats))      # noqa: E731

        def unit():
            return F.sepconv_unit(x, dw.depthwise_kernel, bn, pw.kernel, True, strides=s, dilation=d)

        def fwd():
            with torch.no_grad():
                unit()

        y = unit()

        def bwd():
            torch.autograd.backward(y, dy, retain_graph=True)

        t_f, t_b = rep(fwd), rep(bwd)
        row = {"side": S, "cin": Cin, "cout": Cout, "stride": s, "dilation": d, "fwd_us": round(t_f, 1), "bwd_us": round(t_b, 1)}
        line = f"{'fused' if fused else 'composed'} {S}x{S} {Cin}->{Cout} s{s} d{d}: fwd {t_f:.1f} us  bwd {t_b:.1f} us"
        rows.append(row)
        print(line, flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"variant": "fused" if fused else "composed", "batch": a.batch, "rows": rows}, f, indent=1)

def graphed_step(a):
    """ms per replayed training step of Xception-65 + ASPP (median of `repeats` timings of `iters` replays)"""
    from iseg_amd import functional as F
    from iseg_amd import heads
    from iseg_amd.core_env import common_env_setup
    from iseg_amd.core_optimizer import get_optimizer
    from iseg_amd.core_train import CoreTrain
    from iseg_amd.data import synthetic_batch
    from iseg_amd.graphs import GraphedTrainStep
    from iseg_amd.modelhelper import model_common_setup

    strategy = common_env_setup(use_one_device_strategy=True, mixed_precision=True, random_seed=3)
    model = heads.xception65_aspp(output_stride=16, build_input_size=(512, 512), dropout_rate=0.1)
    helper = model_common_setup(model, restore_checkpoint=False)
    helper.set_optimizer(get_optimizer(strategy, initial_lr=1e-3, end_lr=0.0, epoch_steps=1000, train_epoch=1, warmup_steps=0, warmup_lr=0.0,
                                       optimizer="adamw", adamw_weight_decay=0.05, clipnorm=None))
    tm = CoreTrain(helper, None).create_trainable_model(21, ignore_label=255, batch_size=a.batch)
    step = GraphedTrainStep(tm, warmup=2)
    x, y = synthetic_batch(a.batch, 512, 512, seed=1)
    x, y = x.cuda(), y.cuda()
    t = statistics.median(_timeit(lambda: step(x, y), a.iters) for _ in range(a.repeats)) / 1e3
    assert any(e.get("graph") is not None for e in step.entries.values()), "the step was never captured"
    variant = "fused" if F.sepconv_fused_enabled() else "composed"
    print(f"{variant} Xception-65 + ASPP graphed training step, {a.batch} x 512^2: {t:.3f} ms", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"variant": variant, "batch": a.batch, "graphed_step_ms": round(t, 3)}, f, indent=1)


if __name__ == "__main__":
    main()
