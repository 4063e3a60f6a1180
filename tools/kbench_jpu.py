#!/usr/bin/env python3
"""The JointPyramidUpsampling tail (functional.jpu_tail: four branches depthwise 3x3 d = 1, 2, 4, 8 -> BN -> pointwise 1x1 over one tensor), forward
plus backward with training statistics in bf16: the fused node (csrc/jpu.hip, ISEG_JPU_FUSED=1) against the composed operators
(ISEG_JPU_FUSED=0) in the same process.  The two routes alternate round by round; the spread over the rounds of one route is the noise of the
comparison.  Prints one line per round and a JSON summary per shape (median, min, max in microseconds, and the ratio composed / fused).

usage: python3 tools/kbench_jpu.py [--iters 10] [--rounds 5] [--shapes 0,1] [--json out.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

# N, H, W, C, Cout: 16 x 512^2 at stride 8 with width 512; the same batch at stride 16 with width 256
SHAPES = [(16, 64, 64, 1536, 512), (16, 32, 32, 768, 256)]
RATES = (1, 2, 4, 8)


def build(C, Cout):
    from iseg_amd.layers.base_layers import BatchNormalization, Conv2D, DepthwiseConv2D
    from iseg_amd.param_store import ParamStore

    dws = [DepthwiseConv2D((3, 3), padding="same", dilation_rate=r, name=f"kb/dw_{r}") for r in RATES]
    bns = [BatchNormalization(momentum=0.9, epsilon=1e-3, synchronized=True, name=f"kb/bn_{r}") for r in RATES]
    pws = [Conv2D(Cout, (1, 1), padding="same", use_bias=False, name=f"kb/pw_{r}") for r in RATES]
    for layer in dws + bns + pws:
        layer.build((1, 1, 1, C))
    store = ParamStore([p for layer in dws + bns + pws for p in layer.parameters()])
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for dw, bn in zip(dws, bns):
            dw.bias.copy_((torch.randn(C, generator=g) * 0.1).cuda())
            bn.gamma.copy_((torch.rand(C, generator=g) + 0.5).cuda())
    store.sync_shadow()
    return dws, bns, pws, store


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="0,1")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kbench_jpu: no GPU; a timing needs one")
    from iseg_amd import functional as F
    from iseg_amd import nn

    nn.set_compute_dtype(torch.bfloat16)
    nn.set_device("cuda:0")
    results = []
    for si in [int(s) for s in args.shapes.split(",")]:
        N, H, W, C, Cout = SHAPES[si]
        dws, bns, pws, store = build(C, Cout)
        pwk = [p.kernel for p in pws]
        g = torch.Generator().manual_seed(1)
        x = torch.randn(N, H, W, C, generator=g).to("cuda", torch.bfloat16)
        dvs = [torch.randn(N, H, W, Cout, generator=g).to("cuda", torch.bfloat16) for _ in RATES]
        assert F.jpu_tail_supported(x, dws, bns, pwk)

        def step():
            store.zero_grad()
            xg = x.detach().requires_grad_(True)
            vs = F.jpu_tail(xg, dws, bns, pwk, True)
            torch.autograd.backward(list(vs), dvs)
            return vs, xg.grad

        def timeit(fused):
            os.environ["ISEG_JPU_FUSED"] = "1" if fused else "0"
            for _ in range(3):
                step()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                step()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / args.iters * 1e3

        # the two routes compute the same thing (on the same seeded inputs, at the size that is timed)
        os.environ["ISEG_JPU_FUSED"] = "1"
        vf, dxf = step()
        os.environ["ISEG_JPU_FUSED"] = "0"
        vc, dxc = step()
        rel = lambda a, b: float((a.float() - b.float()).abs().max() / b.float().abs().max())  # noqa: E731
        agree = dict(v8=rel(vf[3], vc[3]), v1=rel(vf[0], vc[0]), dx=rel(dxf, dxc))
        times = {True: [], False: []}
        for r in range(args.rounds):
            for fused in ((True, False) if r % 2 == 0 else (False, True)):
                times[fused].append(timeit(fused))
            print(f"shape {SHAPES[si]} round {r}: fused {times[True][-1]:.1f} us, composed {times[False][-1]:.1f} us", flush=True)
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        out = dict(shape=SHAPES[si], dtype="bf16", iters=args.iters, rounds=args.rounds,
                   fused_us=dict(median=med[True], min=min(times[True]), max=max(times[True])),
                   composed_us=dict(median=med[False], min=min(times[False]), max=max(times[False])),
                   composed_over_fused=med[False] / med[True], max_rel_difference=agree)
        print(json.dumps(out), flush=True)
        results.append(out)
        del x, dvs, store, dws, bns, pws
        torch.cuda.empty_cache()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
