#!/usr/bin/env python3
"""One launch of the batched projective transform (csrc/projective.hip) as RandomRotateAugment uses it -- 16 x 512 x 512 x 3 fp32, bilinear image
with the replace step + nearest label, one angle per sample -- beside one launch of the crop gather (K.augment_crop_batch) at the same
output size, the yardstick: both read at most 4 source pixels and write 12 B + 4 B per output pixel.  The two are interleaved round by round
in one process, device events around a warm loop, medians and the min..max spread.  Bytes per output pixel, the least the algorithm moves
(every source pixel and label read once, every output written once): 12 + 4 read, 12 + 4 written = 32 B, against the 8 TB/s HBM peak.
usage: python3 tools/kbench_rotate.py [rounds] [iters per round] [--json PATH] [--small]"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from iseg_amd import kernels as K  # noqa: E402
from iseg_amd.data_process.augments.random_rotate_augment import get_rotation_matrix  # noqa: E402

HBM_PEAK = 8.0e12
args = [a for a in sys.argv[1:] if not a.startswith("--") and not a.endswith(".json")]
rounds = int(args[0]) if len(args) > 0 else 5
iters = int(args[1]) if len(args) > 1 else 50
B, H, W = (2, 64, 64) if "--small" in sys.argv else (16, 512, 512)


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3      # us per call


g = torch.Generator(device="cuda").manual_seed(0)
images = torch.rand(B, H, W, 3, device="cuda", generator=g) * 255.0
labels = torch.randint(0, 21, (B, H, W), device="cuda", generator=g, dtype=torch.int32)
angles = np.random.default_rng(0).uniform(0.0, 2.0 * np.pi, B).astype(np.float32)
arms = {}
for name, a in {"rotate": angles, "rotate_angle_0": np.zeros(B, dtype=np.float32)}.items():
    t = torch.from_numpy(get_rotation_matrix(a, H, W)).cuda()
    arms[name] = (lambda t=t: K.projective_transform_batch(images, labels, t, image_fill=-1.0, replace=[0.0, 0.0, 0.0], label_fill=255))
# the yardstick: the crop gather with an identity table (no scale, offset 0) and with the pipeline's usual work (scale 1.3, flip)
for name, (s, flip) in {"crop_identity": (1.0, 0), "crop_scale_1.3_flip": (1.3, 1)}.items():
    tab = np.zeros((B, K.augment_params_ints()), dtype=np.int32)
    tab[:, :8] = [H, W, int(H * s), int(W * s), 0, 0, flip, 0]
    p = torch.from_numpy(tab).cuda()
    arms[name] = (lambda p=p: K.augment_crop_batch(images, labels, p, [127.5] * 3, (1.0,) * 3, (0.0,) * 3, 255, H, W, 0))

for fn in arms.values():
    fn()
torch.cuda.synchronize()
times = {k: [] for k in arms}
for _ in range(rounds):
    for k, fn in arms.items():
        times[k].append(timed(fn, iters))
bytes_moved = B * H * W * 32
res = {"rounds": rounds, "iters": iters, "shape": f"{B}x{H}x{W}x3", "bytes_moved": bytes_moved, "arms": {}}
print(f"{B} x {H} x {W} x 3 fp32 + int32 labels, {bytes_moved / 1e6:.1f} MB per launch")
for k, v in times.items():
    med = statistics.median(v)
    res["arms"][k] = {"median_us": med, "min_us": min(v), "max_us": max(v), "bytes_per_s": bytes_moved / (med * 1e-6),
                      "hbm_fraction": bytes_moved / (med * 1e-6) / HBM_PEAK}
    print(f"  {k:22s} median {med:9.1f} us   min {min(v):9.1f}   max {max(v):9.1f}   {bytes_moved / (med * 1e-6) / 1e12:6.3f} TB/s "
          f"= {100 * res['arms'][k]['hbm_fraction']:5.1f} % of the 8 TB/s HBM peak")
res["rotate_over_crop_identity"] = res["arms"]["rotate"]["median_us"] / res["arms"]["crop_identity"]["median_us"]
print(f"  rotate / crop_identity = {res['rotate_over_crop_identity']:.2f} x")
for a in sys.argv:
    if a == "--json":
        path = sys.argv[sys.argv.index(a) + 1]
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        json.dump(res, open(path, "w"), indent=1)
