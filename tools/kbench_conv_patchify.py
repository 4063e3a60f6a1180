#!/usr/bin/env python3
"""The three passes of ConvNeXt's 2x2 / stride-2 downsampling convolutions at the flagship shapes (16 images): the routes functional._Conv2dFn
takes without the patch view (implicit-GEMM forward, GEMM + col2im data gradient, implicit-GEMM weight gradient + column-sum bias gradient)
against the plain GEMMs over the patch view (csrc/conv_patchify.hip).  Device events around back-to-back calls, both routes in one process.
Writes the table to profiles/conv_patchify_kbench.md (or the path given as the first argument)."""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from iseg_amd import kernels as K

BF = torch.bfloat16


def timeit(fn, iters=50, warm=5):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


rows = []
N = 16
for (S, Cin, Cout) in [(128, 96, 192), (64, 192, 384), (32, 384, 768)]:
    k = s = 2
    Ho = S // 2
    geom = K.conv_geom(N, S, S, Cin, Cout, k, k, s, s, 1, 1, 0, 0, Ho, Ho, 1)
    x = torch.randn(N, S, S, Cin, device="cuda").to(BF)
    w = (torch.randn(k, k, Cin, Cout, device="cuda") * 0.05).to(BF)
    wt = w.reshape(-1, Cout).t().contiguous()
    b = torch.randn(Cout, device="cuda")
    dy = torch.randn(N, Ho, Ho, Cout, device="cuda").to(BF)
    dw, db = torch.zeros(k, k, Cin, Cout, device="cuda"), torch.zeros(Cout, device="cuda")
    M, Kd = N * Ho * Ho, k * k * Cin

    def fwd_old():
        if K.conv2d_igemm_fwd_kt_supported(geom, BF):
            return K.conv2d_igemm_fwd_kt(x, wt, b, geom)
        return K.conv2d_igemm_fwd(x, w, b, geom)

    def dgrad_old():
        dcol = torch.empty((M, Kd), dtype=BF, device="cuda")
        K.gemm(dy.reshape(M, Cout), w.reshape(Kd, Cout), dcol, M, Kd, Cout, lda=Cout, ldb=Cout, ldd=Kd, a_kcontig=1, b_kcontig=1)
        return K.col2im(dcol, N, S, S, Cin, k, k, s, s, 1, 1, 0, 0, Ho, Ho)

    def wgrad_old():
        K.colsum(dy.reshape(M, Cout), Cout, 0, 1, M, Cout, db, accumulate=True)
        K.conv2d_igemm_bwd_weight(x, dy, dw, geom, accumulate=True)

    passes = [("forward", K.PATCH_FWD, fwd_old, lambda: K.conv2d_patch_fwd(x, wt, b, geom)),
              ("data gradient", K.PATCH_BWD_DATA, dgrad_old, lambda: K.conv2d_patch_bwd_data(dy, w, geom)),
              ("weight + bias gradient", K.PATCH_BWD_WEIGHT, wgrad_old, lambda: K.conv2d_patch_bwd_weight(x, dy, dw, geom, accumulate=True, bias_grad=db))]
    for name, which, old, new in passes:
        if not K.conv2d_patch_supported(geom, BF, which):
            rows.append((f"{S}x{S}x{Cin}->{Cout}", name, timeit(old), None, "refused"))
            continue
        note = ""
        if which != K.PATCH_BWD_WEIGHT:
            a, c = old(), new()
            note = "same bits" if torch.equal(a, c) else f"max diff {(a.float() - c.float()).abs().max().item():.3g}"
        t_old, t_new = timeit(old), timeit(new)
        t_old2, t_new2 = timeit(old), timeit(new)      # a second pair: the spread between the two is the noise of the figure
        rows.append((f"{S}x{S}x{Cin}->{Cout}", name, min(t_old, t_old2), min(t_new, t_new2), f"{note} (runs {t_old:.1f}/{t_old2:.1f} vs {t_new:.1f}/{t_new2:.1f})"))

lines = ["| layer (16 images) | pass | old route, us | patch view, us | |", "|---|---|---|---|---|"]
for shape, name, o, n, note in rows:
    lines.append(f"| {shape} | {name} | {o:.1f} | {'-' if n is None else f'{n:.1f}'} | {note} |")
tot_o = sum(r[2] for r in rows if r[3] is not None)
tot_n = sum(r[3] for r in rows if r[3] is not None)
lines.append(f"| all | all | {tot_o:.1f} | {tot_n:.1f} | |")
text = "\n".join(lines)
print(text, flush=True)
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "conv_patchify_kbench.md")
with open(out, "w") as f:
    f.write("# Patchify convolutions: old routes against GEMMs over the patch view (tools/kbench_conv_patchify.py, MI355X)\n\n" + text + "\n")
