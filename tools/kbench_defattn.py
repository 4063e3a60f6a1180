"""Deformable-attention core forward + backward at the head shape in-process (for rocprofv3 --kernel-trace --stats, or timed by itself):
python tools/kbench_defattn.py [N] [S] [C] [heads] [points] [iters]      (defaults 16 32 256 4 4 50, bf16)
Prints one line with the event-timed mean of each call and the HBM-byte floor it is to be read against (DESIGN.md 'Deformable attention')."""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from iseg_amd import kernels as K

arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d
N, S, C, heads, P, iters = arg(1, 16), arg(2, 32), arg(3, 256), arg(4, 4), arg(5, 4), arg(6, 50)
v = torch.randn(N, S, S, C, device="cuda").to(torch.bfloat16)
off = (torch.randn(N, S, S, heads * P * 2, device="cuda") * 1.5).to(torch.bfloat16)
att = torch.randn(N, S, S, heads * P, device="cuda").to(torch.bfloat16)
dout = torch.randn(N, S, S, C, device="cuda").to(torch.bfloat16)


def timed(fn):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters * 1e3


fwd_us = timed(lambda: K.defattn_fwd(v, off, att, heads, P, 8.0))
bwd_us = timed(lambda: K.defattn_bwd(v, off, att, dout, heads, P, 8.0))
el, lg = v.numel(), off.numel() + att.numel()
fwd_bytes = 2 * (2 * el + lg)                       # value + out + logits, once each
bwd_bytes = 2 * (3 * el + 2 * lg) + 3 * 8 * el      # value, dout, dvalue, logits and their gradients + the int64 workspace: zeroed, accumulated, read
print(f"defattn {N}x{S}x{S}x{C} heads {heads} points {P} bf16: fwd {fwd_us:.1f} us ({fwd_bytes / 1e6:.1f} MB), "
      f"bwd {bwd_us:.1f} us ({bwd_bytes / 1e6:.1f} MB, {4 * P * el * 8 / 1e6:.0f} MB of int64 atomic adds)")
