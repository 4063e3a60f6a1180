#!/usr/bin/env python3
"""The language-model head's cross-entropy at the Gemma-2B head (d = 2048, V = 256000, bf16) for M = 2048 and 8192 tokens: the chunked route of
csrc/lm_head_ce.hip (K.lm_head_ce_fwd / K.lm_head_ce_bwd, what F.lm_head_cross_entropy runs) against the stored-logits route of the parent
commit.  Device events around a warm loop, several rounds, medians and the min..max spread, arms interleaved round by round; peak memory by
torch.cuda.max_memory_allocated above what is allocated before the call (inputs, table, gradient buffer).

  fused fwd / fwd+bwd       at the chunk widths 2048, 4096, 8192, 16384 and at the library's default
  fused, GEMMs only         the same chunk loop with the kernels of lm_head_ce.hip left out (3 GEMMs per chunk in the backward pass + the logits
                            GEMM of the forward pass), and
  fused, kernels only       chunk_fwd / chunk_bwd alone on one chunk buffer, with the bytes they move per second
  composed                  F.embedding_logits' GEMM storing [M, V] bf16, the cast to fp32 and back that F.softmax_ce_per_pixel makes, and the two
                            gradient GEMMs.  iseg_softmax_ce_ignore itself REFUSES more than 256 classes, so its pass over the fp32 logits (one
                            read, one write of dlogits) is NOT in this figure: the composed time and memory are lower bounds of a route that
                            cannot run at this vocabulary at all.
usage: python3 tools/kbench_lm_head_ce.py [rounds] [iters per round] [--json PATH] [--small]"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from iseg_amd import kernels as K  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--") and not a.endswith(".json")]
rounds = int(args[0]) if len(args) > 0 else 5
iters = int(args[1]) if len(args) > 1 else 3
SMALL = "--small" in sys.argv
V, d = (4100, 64) if SMALL else (256000, 2048)
MS = (130, 260) if SMALL else (2048, 8192)
CHUNKS = (256, 512, 1024) if SMALL else (2048, 4096, 8192, 16384)
BF = torch.bfloat16


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n      # ms per call


def peak_of(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def stats(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}


def show(name, r, extra=""):
    print(f"  {name:34s} {r['median_ms']:9.3f} ms ({r['min_ms']:.3f}..{r['max_ms']:.3f}){extra}", flush=True)


res = {"rounds": rounds, "iters": iters, "V": V, "d": d, "cases": {}}
g = torch.Generator(device="cuda").manual_seed(1)
table = (torch.randn((V, d), device="cuda", generator=g) * d ** -0.5).to(BF)
dtable = torch.zeros((V, d), device="cuda", dtype=torch.float32)
for M in MS:
    x = torch.randn((M, d), device="cuda", generator=g).to(BF)
    t = torch.randint(0, V, (M,), device="cuda", generator=g).to(torch.int32)
    up = torch.ones(M, device="cuda")
    default = K.lm_head_ce_chunk_default(M, V)
    case = res["cases"][f"M{M}"] = {"default_chunk": default}
    print(f"M {M} V {V} d {d} bf16 (default chunk {default})", flush=True)

    def fwd(c):
        return K.lm_head_ce_fwd(x, table, t, None, c)

    def fwd_bwd(c):
        out = K.lm_head_ce_fwd(x, table, t, None, c)
        return K.lm_head_ce_bwd(x, table, t, None, out[5], out[6], up, 1.0, c, dtable=dtable, want_dx=True)

    def gemms(c, backward):
        ld = K.lm_head_ce_pitch(min(c, V))
        z = torch.empty((M, ld), dtype=torch.float32, device="cuda")
        gbuf = torch.zeros((M, ld), dtype=BF, device="cuda")
        dx32 = torch.empty((M, d), dtype=torch.float32, device="cuda")

        def run():
            for i, (v0, w) in enumerate(K.lm_head_ce_chunks(V, c)):
                K.lm_head_ce_logits(x, table, z, v0, w)
                if backward:
                    K.lm_head_ce_logits(x, table, z, v0, w)
                    K.gemm(gbuf, table[v0:v0 + w], dx32, M, d, w, lda=ld, ldb=d, ldd=d, a_kcontig=1, b_kcontig=0, accumulate=i > 0)
                    K.dense_wgrad(gbuf[:, :w], x, dtable[v0:v0 + w])
        return run

    def kernels_only(c, backward):
        ld = K.lm_head_ce_pitch(min(c, V))
        z = torch.randn((M, ld), dtype=torch.float32, device="cuda", generator=g)
        gbuf = torch.empty((M, ld), dtype=BF, device="cuda")
        state = K.lm_head_ce_state(M, "cuda")
        K.lm_head_ce_chunk_fwd(z, t, state, 0, min(c, V))

        def run():
            for v0, w in K.lm_head_ce_chunks(V, c):
                K.lm_head_ce_chunk_fwd(z, t, state, v0, w)
                if backward:
                    K.lm_head_ce_chunk_bwd(z, state[0], state[1], t, None, up, 1.0, gbuf, V, v0, w)
        return run

    arms = {}
    for c in CHUNKS:
        arms[f"fused fwd chunk {c}"] = lambda c=c: fwd(c)
        arms[f"fused fwd+bwd chunk {c}"] = lambda c=c: fwd_bwd(c)
    arms["fused GEMMs only fwd"] = gemms(default, False)
    arms["fused GEMMs only fwd+bwd"] = gemms(default, True)
    arms["fused kernels only fwd"] = kernels_only(default, False)
    arms["fused kernels only fwd+bwd"] = kernels_only(default, True)

    # the stored-logits route, without the loss kernel that refuses this vocabulary
    logits = torch.empty((M, V), dtype=BF, device="cuda")
    dz32 = torch.randn((M, V), dtype=torch.float32, device="cuda", generator=g) * 1e-3

    def composed_fwd():
        K.dense_fwd_t(x, table, out=logits)
        return K.cast(logits, torch.float32)

    def composed_fwd_bwd():
        composed_fwd()
        dz = K.cast(dz32, BF)
        K.dense_wgrad(dz, x, dtable)
        return K.dense_fwd(dz, table)

    arms["composed fwd (no loss kernel)"] = composed_fwd
    arms["composed fwd+bwd (no loss kernel)"] = composed_fwd_bwd
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            times[k].append(timed(fn, iters))
    for k, v in times.items():
        case[k] = stats(v)
    nchunks = len(K.lm_head_ce_chunks(V, default))
    zbytes = M * V * 4
    for k in arms:
        extra = ""
        if k == "fused kernels only fwd":
            extra = f"   {zbytes / case[k]['median_ms'] / 1e6:8.1f} GB/s of Z read ({nchunks} chunks)"
        if k == "fused kernels only fwd+bwd":
            both = zbytes * 2 + M * V * 2
            extra = f"   {both / case[k]['median_ms'] / 1e6:8.1f} GB/s of Z read twice + G written"
        show(k, case[k], extra)
    del logits, dz32
    mem = {f"fused fwd+bwd chunk {c}": peak_of(lambda c=c: fwd_bwd(c)) for c in CHUNKS}
    logits = torch.empty((M, V), dtype=BF, device="cuda")
    dz32 = torch.zeros((M, V), dtype=torch.float32, device="cuda")
    mem["composed fwd+bwd (no loss kernel)"] = peak_of(composed_fwd_bwd) + logits.numel() * 2 + dz32.numel() * 4
    case["peak_bytes"] = mem
    for k, v in mem.items():
        print(f"  peak memory {k:36s} {v / 2 ** 20:10.1f} MiB", flush=True)
    del logits, dz32, x, t, up

for a in sys.argv:
    if a == "--json":
        path = sys.argv[sys.argv.index(a) + 1]
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        json.dump(res, open(path, "w"), indent=1)
