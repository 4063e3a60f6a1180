"""SelfAttention core (64-wide query / key, wide value) forward and forward + backward at one shape in-process, the fused kernels of
csrc/selfattn.hip beside the composed route of F.attention_packed (for rocprofv3 --kernel-trace --stats, or timed by itself):
python tools/kbench_selfattn.py [B] [T] [dv] [iters]      (defaults 16 4096 512 10, bf16, dk 64, scale 1/8)
Prints one line per route with the event-timed mean of each pass, and the size of the probability tensor the composed route keeps."""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from iseg_amd import functional as F
from iseg_amd import nn

arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d
B, T, dv, iters = arg(1, 16), arg(2, 4096), arg(3, 512), arg(4, 10)
nn.set_compute_dtype(torch.bfloat16)
nn.set_device("cuda:0")
q, k = ((torch.randn(B, T, 64, device="cuda") * 0.35).to(torch.bfloat16).requires_grad_(True) for _ in range(2))
v = torch.randn(B, T, dv, device="cuda").to(torch.bfloat16).requires_grad_(True)
dout = torch.randn(B, T, dv, device="cuda").to(torch.bfloat16)


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def forward():
    with torch.no_grad():
        F.self_attention_core(q, k, v, 0.125)


def forward_backward():
    q.grad = k.grad = v.grad = None
    F.self_attention_core(q, k, v, 0.125).backward(dout)


for mode, label in (("1", "fused"), ("0", "composed")):
    os.environ["ISEG_SELFATTN_FUSED"] = mode
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fwd_ms, both_ms = timed(forward), timed(forward_backward)
    q.grad = k.grad = v.grad = None
    print(f"selfattn {B}x{T} dk 64 dv {dv} bf16 {label}: fwd {fwd_ms:.2f} ms, fwd+bwd {both_ms:.2f} ms, "
          f"peak {(torch.cuda.max_memory_allocated() - base) / 2 ** 20:.0f} MiB above the operands "
          f"(one probability tensor: {B * T * T * 2 / 2 ** 20:.0f} MiB)", flush=True)
