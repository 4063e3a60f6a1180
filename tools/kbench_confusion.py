#!/usr/bin/env python3
"""Confusion matrices of 16 x 512 x 512 label / prediction maps (csrc/confusion.hip, iseg_confusion_batched): C = 21, 150 (and, for the route
table, 203 and 256) in the three weight modes, per-image matrices.  Device events around a warm loop, several rounds, medians and the
min..max spread; the routes are interleaved round by round.
  fused      one call of iseg_confusion_batched (the memset of the matrices and one kernel)
  composed   torch ops on the same device, a yardstick only (never on the product path): torch.bincount of (b * C + label) * C + pred with the
             weights as float64, reshaped to [B, C, C]
The algorithmic traffic is 8 (no weights), 9 (byte weights) or 12 (fp32 weights) bytes per element; the fraction printed is those bytes over the
fused call's time against the 8 TB/s HBM peak.  The fused result is compared with the composed one before anything is timed (exactly: the
weights are multiples of 1/8).

Route A/B: the library takes the LDS route (label-row bands, one pass of the index streams per band) or direct global atomics.  The process
re-runs itself with ISEG_CONFUSION_ROUTE=1 (LDS wherever its bands fit) and =2 (global atomics) -- the variable is read once per process -- and
prints both beside the dispatcher's own choice.  Labels are drawn two ways: uniformly ("uniform": every bin equally likely, the friendliest
case for atomics) and as a segmentation map would have them ("blocky": 32 x 32 tiles of one class, the prediction equal to the label on 90 %
of the pixels: whole wavefronts add to ONE bin).
usage: python3 tools/kbench_confusion.py [rounds] [iters per round] [--json PATH] [--small] [--route-only]"""
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from iseg_amd import kernels as K  # noqa: E402

HBM_PEAK = 8.0e12
args = [a for a in sys.argv[1:] if not a.startswith("--") and not a.endswith(".json")]
rounds = int(args[0]) if len(args) > 0 else 5
iters = int(args[1]) if len(args) > 1 else 50
B, H, W = (2, 64, 80) if "--small" in sys.argv else (16, 512, 512)
CHILD = "--route-only" in sys.argv
CLASSES = (21, 150, 203, 256)
MODES = {"none": 8, "u8": 9, "f32": 12}      # bytes per element


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3      # us per call


def maps(C, kind, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    if kind == "uniform":
        lab = torch.randint(0, C, (B, H, W), device="cuda", generator=g, dtype=torch.int32)
        prd = torch.randint(0, C, (B, H, W), device="cuda", generator=g, dtype=torch.int32)
    else:
        tiles = torch.randint(0, C, (B, (H + 31) // 32, (W + 31) // 32), device="cuda", generator=g, dtype=torch.int32)
        lab = tiles.repeat_interleave(32, 1).repeat_interleave(32, 2)[:, :H, :W].contiguous()
        other = torch.randint(0, C, (B, H, W), device="cuda", generator=g, dtype=torch.int32)
        prd = torch.where(torch.rand(B, H, W, device="cuda", generator=g) < 0.9, lab, other)
    return lab.reshape(B, -1).contiguous(), prd.reshape(B, -1).contiguous()


def weights(mode, seed):
    g = torch.Generator(device="cuda").manual_seed(seed + 1)
    if mode == "none":
        return None
    if mode == "u8":
        return (torch.rand(B, H * W, device="cuda", generator=g) < 0.9).to(torch.uint8)      # a not-ignore mask
    return torch.randint(-248, 249, (B, H * W), device="cuda", generator=g).to(torch.float32) / 8


def composed(lab, prd, w, C):
    idx = (torch.arange(B, device="cuda").view(B, 1) * C + lab.long()) * C + prd.long()
    return torch.bincount(idx.reshape(-1), weights=None if w is None else w.reshape(-1).double(), minlength=B * C * C).reshape(B, C, C)


res = {"rounds": rounds, "iters": iters, "shape": f"{B}x{H}x{W}", "route_override": os.environ.get("ISEG_CONFUSION_ROUTE", "0"), "arms": {}}
for C in CLASSES:
    for kind in ("uniform", "blocky"):
        lab, prd = maps(C, kind, C)
        for mode, bpe in MODES.items():
            w = weights(mode, C)
            e = K.confusion_weight_exponent(K.confusion_absmax(w)) if mode == "f32" else 0
            cm = torch.empty(B, C, C, dtype=torch.int64, device="cuda")
            counters = torch.zeros(8, dtype=torch.int64, device="cuda")

            def fused():
                K.confusion_batched(lab, prd, C, weights=w, w_exp=e, cm=cm, counters=counters)

            def comp():
                composed(lab, prd, w, C)

            fused()
            want = composed(lab, prd, w, C)
            got = torch.ldexp(cm.double(), torch.tensor(-e, device="cuda"))
            assert torch.equal(got, want.double()) and not counters.any(), f"C {C} {kind} {mode}: the routes disagree"
            arms = {"fused": (fused, iters)} if CHILD else {"fused": (fused, iters), "composed": (comp, max(1, iters // 5))}
            for fn, _ in arms.values():      # warm-up of every arm at this shape
                for _ in range(3):
                    fn()
            times = {k: [] for k in arms}
            for _ in range(rounds):
                for k, (fn, n) in arms.items():
                    times[k].append(timed(fn, n))
            r = {k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for k, v in times.items()}
            r["bytes_per_element"] = bpe
            r["fused_bytes_per_s"] = B * H * W * bpe / (r["fused"]["median_us"] * 1e-6)
            r["fused_hbm_fraction"] = r["fused_bytes_per_s"] / HBM_PEAK
            res["arms"][f"C{C} {kind} {mode}"] = r
            line = f"C {C:3d} {kind:8s} {mode:5s} fused {r['fused']['median_us']:9.1f} us ({r['fused']['min_us']:.1f}..{r['fused']['max_us']:.1f})"
            if not CHILD:
                line += (f"   composed {r['composed']['median_us']:9.1f} us   {bpe} B/element at {r['fused_bytes_per_s'] / 1e12:.3f} TB/s = "
                         f"{100 * r['fused_hbm_fraction']:.1f} % of the HBM peak")
            print(line, flush=True)

if not CHILD:
    # the two forced routes, each in a fresh process (the library reads the variable once)
    for route, name in (("1", "lds"), ("2", "global")):
        env = dict(os.environ, ISEG_CONFUSION_ROUTE=route)
        path = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"kbench_confusion_route{route}.json")
        cmd = [sys.executable, os.path.abspath(__file__), str(rounds), str(iters), "--route-only", "--json", path] + (["--small"] if "--small" in sys.argv else [])
        print(f"--- forced route: {name}", flush=True)
        out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        print(out.stdout + out.stderr[-2000:], flush=True)
        if out.returncode != 0:      # nothing more is started on the device after a failed run
            sys.exit(out.returncode)
        res[f"forced_{name}"] = json.load(open(path))["arms"]
for a in sys.argv:
    if a == "--json":
        path = sys.argv[sys.argv.index(a) + 1]
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        json.dump(res, open(path, "w"), indent=1)
