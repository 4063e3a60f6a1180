#!/usr/bin/env python3
"""One sampling step over a [B, 256000] bf16 logits matrix (csrc/token_sample.hip, iseg_token_sample: the chunk pass and the draw, two launches)
at batch 1, 8 and 64 for the three modes: top-k (k = 5), top-p (p = 0.9, no k) and random.  Device events around a warm loop, several rounds,
medians and the min..max spread; the arms are interleaved round by round.
  fused      one call of F.sample_tokens with the launcher's own chunk plan, walking a ring of logit buffers of 512 MB in all -- larger than the
             256 MB last-level cache -- so that every call reads its logits from HBM
  hot        the same call on ONE buffer over and over: it stays in cache
  composed   the torch composition on the same tensors, code that is not under test: softmax -> topk -> multinomial (top-k),
             softmax -> sort -> cumsum -> mask -> multinomial (top-p), softmax -> multinomial (random); on the ring as well
The uniforms are drawn before the loop (one torch.rand per step is the sampler's, not the kernel's).  Before anything is timed the fused top-k
tokens are checked to lie among torch.topk's indices.

Then the per-token time of GemmaCausalLM.generate_step on the 2-layer model of tools/kbench_gemma_decode.py (Gemma-2B's width, vocabulary 256000),
batch 1 and 8, prompts of 16 tokens generated to 272 positions: "greedy" against TopKSampler(k=5), TopPSampler(p=0.9) and RandomSampler; the
seeding pass is timed on its own and subtracted.
usage: python3 tools/kbench_token_sample.py [rounds] [iters per round] [--json PATH] [--small] [--no-model]"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from iseg_amd import functional as F  # noqa: E402
from iseg_amd import kernels as K  # noqa: E402

RING_BYTES = 512 << 20
HOST_FLOOR_US = 17.0      # one Python call with two launches (profiles/gemma_decode_kbench.md)
args = [a for a in sys.argv[1:] if not a.startswith("--") and not a.endswith(".json")]
rounds = int(args[0]) if len(args) > 0 else 5
iters = int(args[1]) if len(args) > 1 else 50
SMALL = "--small" in sys.argv
V = 4099 if SMALL else 256000
BATCHES = (1, 3) if SMALL else (1, 8, 64)
MODES = {"top_k": dict(mode="top_k", k=5), "top_p": dict(mode="top_p", p=0.9), "random": dict(mode="random")}


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3      # us per call


def composed(x, name):
    pr = torch.softmax(x.float(), dim=-1)
    if name == "top_k":
        v, i = torch.topk(pr, 5, dim=-1)
        return i.gather(1, torch.multinomial(v, 1))
    if name == "top_p":
        sp, si = torch.sort(pr, dim=-1, descending=True)
        keep = (torch.cumsum(sp, dim=-1) - sp) <= 0.9
        return si.gather(1, torch.multinomial(sp * keep, 1))
    return torch.multinomial(pr, 1)


res = {"rounds": rounds, "iters": iters, "V": V, "arms": {}}
for B in BATCHES:
    nbytes = B * V * 2
    ring = 2 if SMALL else max(2, min(1024, -(-RING_BYTES // nbytes)))
    g = torch.Generator(device="cuda").manual_seed(B)
    bufs = (2.0 * torch.randn((ring, B, V), device="cuda", generator=g, dtype=torch.float32)).to(torch.bfloat16)
    u = torch.rand(B, device="cuda", generator=g)
    splits = K.token_sample_splits(B, V)
    tok = F.sample_tokens(bufs[0], u, mode="top_k", k=5)
    top = torch.topk(bufs[0].float(), 5, dim=-1).values[:, -1:]
    assert bool((bufs[0].float().gather(1, tok.long()[:, None]) >= top).all()), "a top-k token lies outside torch.topk's five"
    for name, kw in MODES.items():
        turn = [0, 0]

        def fused():
            turn[0] = (turn[0] + 1) % ring
            F.sample_tokens(bufs[turn[0]], u, **kw)

        def hot():
            F.sample_tokens(bufs[0], u, **kw)

        def comp():
            turn[1] = (turn[1] + 1) % ring
            composed(bufs[turn[1]], name)

        arms = {"fused": (fused, iters), "hot": (hot, iters), "composed": (comp, max(1, iters // 5))}
        for fn, _ in arms.values():
            for _ in range(3):
                fn()
        times = {k: [] for k in arms}
        for _ in range(rounds):
            for k, (fn, n) in arms.items():
                times[k].append(timed(fn, n))
        r = {k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for k, v in times.items()}
        r.update(logit_bytes=nbytes, splits=splits, ring=ring, speedup=r["composed"]["median_us"] / r["fused"]["median_us"],
                 over_host_floor=r["fused"]["median_us"] / HOST_FLOOR_US)
        res["arms"][f"{name} B{B}"] = r
        print(f"{name:6s} B {B:2d} V {V}: fused {r['fused']['median_us']:8.1f} us ({r['fused']['min_us']:.1f}..{r['fused']['max_us']:.1f}), hot "
              f"{r['hot']['median_us']:8.1f} us ({r['hot']['min_us']:.1f}..{r['hot']['max_us']:.1f}), composed {r['composed']['median_us']:9.1f} us "
              f"({r['composed']['min_us']:.1f}..{r['composed']['max_us']:.1f}), composed / fused {r['speedup']:6.2f}, fused / 17 us host floor "
              f"{r['over_host_floor']:5.2f}, splits {splits}, ring {ring}", flush=True)
    del bufs

if "--no-model" not in sys.argv:
    # the per-token time of generate_step on the 2-layer model of tools/kbench_gemma_decode.py, greedy against the samplers
    import time

    from iseg_amd import nn
    from iseg_amd.nlp.gemma import GemmaBackbone, GemmaCausalLM
    from iseg_amd.nlp.samplers import RandomSampler, TopKSampler, TopPSampler
    from iseg_amd.param_store import ParamStore

    nn.set_compute_dtype(torch.bfloat16)
    nn.set_device("cuda:0")
    cfg = dict(vocabulary_size=1000, num_layers=2, num_query_heads=4, num_key_value_heads=1, hidden_dim=256, intermediate_dim=1024, head_dim=64) \
        if SMALL else dict(vocabulary_size=256000, num_layers=2, num_query_heads=8, num_key_value_heads=1, hidden_dim=2048,
                           intermediate_dim=32768, head_dim=256)
    prompt, length = (4, 24) if SMALL else (16, 272)
    model = GemmaCausalLM(GemmaBackbone(**cfg))
    with nn.dry_run_scope():
        model({"token_ids": torch.zeros(1, 8, dtype=torch.int64, device="cuda"), "padding_mask": torch.ones(1, 8, dtype=torch.int32, device="cuda")})
    model._iseg_store = ParamStore(list(model.parameters()))
    model._iseg_store.sync_shadow()
    res["generate"] = {"config": cfg, "prompt": prompt, "length": length}

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for B in (1, 2) if SMALL else (1, 8):
        ids = torch.randint(1, cfg["vocabulary_size"], (B, length), device="cuda", generator=torch.Generator(device="cuda").manual_seed(B))
        mask = torch.zeros(B, length, dtype=torch.bool, device="cuda")
        mask[:, :prompt] = True
        inputs = {"token_ids": ids * mask, "padding_mask": mask}
        seed_s = None
        for name, sampler in (("greedy", "greedy"), ("top_k", TopKSampler(k=5, seed=1)), ("top_p", TopPSampler(p=0.9, seed=1)),
                              ("random", RandomSampler(seed=1))):
            model.compile(sampler=sampler)
            wall(lambda: model.generate_step(inputs))      # warm-up of every shape
            if seed_s is None:
                seed_s = statistics.median(wall(lambda: model._build_cache(inputs["token_ids"])) for _ in range(3))
            total_s = statistics.median(wall(lambda: model.generate_step(inputs)) for _ in range(3))
            per_token_us = (total_s - seed_s) / (length - prompt) * 1e6
            res["generate"][f"{name} B{B}"] = {"seed_ms": seed_s * 1e3, "total_ms": total_s * 1e3, "per_token_us": per_token_us}
            print(f"generate_step B {B} {name:6s}: {length - prompt} tokens, seeding pass {seed_s * 1e3:.2f} ms, whole call {total_s * 1e3:.2f} ms, "
                  f"{per_token_us:.1f} us per token (host launches included)", flush=True)

for a in sys.argv:
    if a == "--json":
        path = sys.argv[sys.argv.index(a) + 1]
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        json.dump(res, open(path, "w"), indent=1)
