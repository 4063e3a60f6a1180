#!/usr/bin/env python3
"""Connected-components labelling of a 16 x 512 x 512 int32 mask at foreground densities 0.3, 0.59 (just under the site-percolation threshold:
large, tortuous clusters) and 0.9.  Two routes, interleaved round by round in one process, device events around a warm loop, medians and the
min..max spread:
  fused      csrc/ccl.hip (one call of iseg_ccl_label: six launches)
  composed   torch ops on the same device: every foreground pixel starts with its linear index and takes the minimum over itself and its four
             neighbours, masked, until nothing changes (one torch.equal, i.e. one host read, per trip); then the roots (pixels that kept their
             own index) are ranked by a cumulative sum and every pixel gathers its root's rank.  Its trip count is the longest shortest path
             from a component's first pixel, in pixels.
The two agree bit for bit before they are timed.  The floor is one read of the mask and one write of the labels, 8 bytes per pixel; the
fraction printed is those bytes over the fused call's time, against the 8 TB/s HBM peak.
usage: python3 tools/kbench_ccl.py [rounds] [iters per round] [--json PATH] [--small]"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from iseg_amd import kernels as K  # noqa: E402

HBM_PEAK = 8.0e12
args = [a for a in sys.argv[1:] if not a.startswith("--") and not a.endswith(".json")]
rounds = int(args[0]) if len(args) > 0 else 5
iters = int(args[1]) if len(args) > 1 else 20
N, H, W = (2, 64, 80) if "--small" in sys.argv else (16, 512, 512)
DENSITIES = (0.3, 0.59, 0.9)


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3      # us per call


def composed(mask):
    """-> (labels, counts, trips)"""
    n, h, w = mask.shape
    big = h * w
    fg = mask != 0
    idx = torch.arange(big, dtype=torch.int32, device=mask.device).view(1, h, w).expand(n, h, w)
    lab = torch.where(fg, idx, big)
    trips = 0
    while True:
        p = torch.nn.functional.pad(lab, (1, 1, 1, 1), value=big)
        near = torch.minimum(torch.minimum(p[:, :-2, 1:-1], p[:, 2:, 1:-1]), torch.minimum(p[:, 1:-1, :-2], p[:, 1:-1, 2:]))
        new = torch.where(fg, torch.minimum(lab, near), lab)
        trips += 1
        if torch.equal(new, lab):
            break
        lab = new
    roots = fg & (lab == idx)
    rank = torch.cumsum(roots.view(n, -1).to(torch.int32), 1, dtype=torch.int32)
    labels = torch.where(fg, rank.gather(1, lab.clamp(max=big - 1).view(n, -1).long()).view(n, h, w), 0).to(torch.int32)
    return labels, rank[:, -1].contiguous(), trips


res = {"rounds": rounds, "iters": iters, "shape": f"{N}x{H}x{W}", "arms": {}}
for density in DENSITIES:
    g = torch.Generator(device="cuda").manual_seed(int(density * 100))
    mask = (torch.rand(N, H, W, device="cuda", generator=g) < density).to(torch.int32).contiguous()
    labels, counts = torch.empty_like(mask), torch.empty(N, dtype=torch.int32, device="cuda")
    trips = [0]

    def fused():
        K.ccl_label(mask, labels=labels, counts=counts)

    def comp():
        trips[0] = composed(mask)[2]

    arms = {"fused": (fused, iters), "composed": (comp, 1)}
    fused()
    cl, cc, _ = composed(mask)
    torch.cuda.synchronize()
    # the two routes agree before they are timed
    assert torch.equal(labels, cl) and torch.equal(counts, cc), f"density {density}: the routes disagree"
    times = {k: [] for k in arms}
    for _ in range(rounds):
        for k, (fn, n) in arms.items():
            times[k].append(timed(fn, n))
    r = {k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for k, v in times.items()}
    r["composed_trips"] = trips[0]
    r["components_per_image"] = float(counts.float().mean())
    r["floor_bytes"] = N * H * W * 8
    r["fused_bytes_per_s"] = r["floor_bytes"] / (r["fused"]["median_us"] * 1e-6)
    r["fused_hbm_fraction"] = r["fused_bytes_per_s"] / HBM_PEAK
    r["composed_over_fused"] = r["composed"]["median_us"] / r["fused"]["median_us"]
    res["arms"][f"density {density}"] = r
    print(f"{N} x {H} x {W} int32 mask, density {density}: {r['components_per_image']:.0f} components per image")
    for k in arms:
        print(f"  {k:10s} median {r[k]['median_us']:12.1f} us   min {r[k]['min_us']:12.1f}   max {r[k]['max_us']:12.1f}")
    print(f"  composed / fused = {r['composed_over_fused']:.1f} x   ({trips[0]} trips of the composed route)")
    print(f"  fused moves the floor's {r['floor_bytes'] / 1e6:.1f} MB (mask read + label write) at {r['fused_bytes_per_s'] / 1e12:.3f} TB/s: "
          f"{100 * r['fused_hbm_fraction']:.1f} % of the 8 TB/s HBM peak")
for a in sys.argv:
    if a == "--json":
        path = sys.argv[sys.argv.index(a) + 1]
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        json.dump(res, open(path, "w"), indent=1)
