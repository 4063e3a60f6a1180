"""micro-benchmark of the packed attention kernels on the ViT-B/16 window shape (4 windows x 1025 tokens x 12 heads x 64):
python tools/kbench_flash.py [B T H D] [train]
Times the inference forward; with `train` also the training pair (attention_fwd_train, then attention_bwd: row-dot, dQ, dK/dV)."""
import sys

import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from iseg_amd import kernels as K  # noqa: E402

args = [a for a in sys.argv[1:] if a != "train"]
train = "train" in sys.argv[1:]
B, T, H, D = (int(a) for a in (args[:4] if len(args) >= 4 else (4, 1025, 12, 64)))
qkv = (torch.randn(B, T, 3 * H * D, device="cuda") * 1.0).bfloat16()
scale = D ** -0.5
flops = 4.0 * B * H * T * T * D      # forward: two products


def timed(fn, n=50):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


us = timed(lambda: K.attention_fwd(qkv, H, scale))
print(f"flash fwd B={B} T={T} H={H}: {us:.1f} us  {flops / us / 1e6:.1f} TFLOP/s")
if train:
    dout = torch.randn(B, T, H * D, device="cuda").bfloat16()
    out, lse = K.attention_fwd_train(qkv, H, scale)
    us = timed(lambda: K.attention_fwd_train(qkv, H, scale))
    print(f"flash fwd_train B={B} T={T} H={H}: {us:.1f} us  {flops / us / 1e6:.1f} TFLOP/s")
    us = timed(lambda: K.attention_bwd(qkv, out, dout, lse, H, scale))      # dQ: three products, dK/dV: four
    print(f"flash bwd B={B} T={T} H={H}: {us:.1f} us  {3.5 * flops / us / 1e6:.1f} TFLOP/s")
