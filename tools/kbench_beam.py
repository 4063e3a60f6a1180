#!/usr/bin/env python3
"""One beam-search step (csrc/beam_search.hip: F.beam_select, two launches, and F.beam_reorder, two launches) against the composed route, the
reference's op sequence in torch (ISEG_BEAM_FUSED=0: log-softmax, add, [B, nb V] top-k with the order pinned down, then index_select over the
WHOLE cache; `reference ops` is the select half without the second, integer top-k that pins the tie order down: softmax, log, add, reshape,
top-k and nothing else), at Gemma-2B's head and cache: V = 256000 bf16 logits, cache [B nb, 18, 2, S, 1, 256] bf16 with S = 4096 positions of which
128, 1024 or 4096 are filled, B nb = 4, 16 and 32 rows in groups of nb = 4 beams.  Device events around a warm loop, several rounds, medians
and the min..max spread; the arms are interleaved round by round.  The logits walk a ring of buffers of 512 MB in all, larger than the 256 MB
last-level cache; the cache is far larger than that by itself.  The parents are random with repeats (a beam usually has several children), so
about three quarters of the rows move.

The bytes each kernel has to move are printed beside the time: the logits once; for the reorder a write of the filled prefix of every row
that is not its own parent and a read of every distinct parent among them (at most twice the filled prefix of all rows).  `copy` is the
rate of one torch copy of 1 GiB (read + write bytes over time), the yardstick for the fraction reached.

Then the time per generated token of GemmaCausalLM.generate_step on the 2-layer model of tools/kbench_gemma_decode.py (Gemma-2B's width,
vocabulary 256000), one prompt of 16 tokens generated to 272 positions: "greedy" against BeamSampler(num_beams=1) and (num_beams=4), fused and
composed; the seeding pass is timed on its own and subtracted.
usage: python3 tools/kbench_beam.py [rounds] [iters per round] [--json PATH] [--small] [--no-model]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from iseg_amd import functional as F  # noqa: E402
from iseg_amd import kernels as K  # noqa: E402

RING_BYTES = 512 << 20
args = [a for a in sys.argv[1:] if not a.startswith("--") and not a.endswith(".json")]
rounds = int(args[0]) if len(args) > 0 else 5
iters = int(args[1]) if len(args) > 1 else 20
SMALL = "--small" in sys.argv
V = 4099 if SMALL else 256000
LAYERS, S, NKV, H = (2, 64, 1, 64) if SMALL else (18, 4096, 1, 256)
ROWS = (4, 8) if SMALL else (4, 16, 32)
FILLS = (8, 64) if SMALL else (128, 1024, 4096)
NB = 4


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3      # us per call


def route(fused):
    os.environ["ISEG_BEAM_FUSED"] = "1" if fused else "0"


def measure(arms):
    for fn, _ in arms.values():
        for _ in range(2):
            fn()
    times = {k: [] for k in arms}
    for _ in range(rounds):
        for k, (fn, n) in arms.items():
            times[k].append(timed(fn, n))
    return {k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for k, v in times.items()}


res = {"rounds": rounds, "iters": iters, "V": V, "cache": [LAYERS, 2, S, NKV, H], "nb": NB, "select": {}, "reorder": {}}
big = torch.empty((64 << 20) if SMALL else (1 << 30), dtype=torch.uint8, device="cuda")
dst = torch.empty_like(big)
copy_us = statistics.median(timed(lambda: dst.copy_(big), 5) for _ in range(rounds))
res["copy_GBps"] = copy_rate = 2 * big.numel() / copy_us / 1e3
print(f"copy of {big.numel() >> 20} MiB: {copy_us:.1f} us, {copy_rate:.0f} GB/s read + write", flush=True)
del big, dst

for R in ROWS:
    g = torch.Generator(device="cuda").manual_seed(R)
    nbytes = R * V * 2
    ring = 2 if SMALL else max(2, min(256, -(-RING_BYTES // nbytes)))
    bufs = (2.0 * torch.randn((ring, R, V), device="cuda", generator=g, dtype=torch.float32)).to(torch.bfloat16)
    lp = -10.0 * torch.rand(R, device="cuda", generator=g)
    route(True)
    got = F.beam_select(bufs[0], lp, NB)
    route(False)
    want = F.beam_select(bufs[0], lp, NB)
    assert bool((got[2] - want[2]).abs().max() < 1e-4), "the fused and the composed selection disagree"
    turn = [0, 0]

    def sel_fused():
        route(True)
        turn[0] = (turn[0] + 1) % ring
        F.beam_select(bufs[turn[0]], lp, NB)

    def sel_hot():
        route(True)
        F.beam_select(bufs[0], lp, NB)

    def sel_composed():
        route(False)
        turn[1] = (turn[1] + 1) % ring
        F.beam_select(bufs[turn[1]], lp, NB)

    def sel_reference():      # the reference's five ops and nothing else: no pinned tie order
        turn[1] = (turn[1] + 1) % ring
        x = bufs[turn[1]]
        torch.topk((torch.log(torch.softmax(x.float() / 1.0, dim=-1)) + lp[:, None]).reshape(R // NB, NB * V), NB, dim=-1)

    # a select call is some 25 us: ten times the calls of the other arms, so that a timed window is milliseconds long
    r = measure({"fused": (sel_fused, 10 * iters), "hot": (sel_hot, 10 * iters), "composed": (sel_composed, iters),
                 "reference": (sel_reference, iters)})
    r.update(logit_bytes=nbytes, splits=K.beam_select_splits(R, V), GBps=nbytes / r["fused"]["median_us"] / 1e3,
             speedup=r["composed"]["median_us"] / r["fused"]["median_us"], speedup_reference=r["reference"]["median_us"] / r["fused"]["median_us"])
    r["of_copy"] = r["GBps"] / copy_rate
    res["select"][f"R{R}"] = r
    print(f"select  R {R:2d}: fused {r['fused']['median_us']:8.1f} us ({r['fused']['min_us']:.1f}..{r['fused']['max_us']:.1f}), hot "
          f"{r['hot']['median_us']:7.1f} us, composed {r['composed']['median_us']:9.1f} us ({r['composed']['min_us']:.1f}..{r['composed']['max_us']:.1f}), "
          f"composed / fused {r['speedup']:6.2f}, reference ops {r['reference']['median_us']:9.1f} us ({r['reference']['min_us']:.1f}..{r['reference']['max_us']:.1f}), "
          f"reference / fused {r['speedup_reference']:6.2f}; {nbytes / 1e6:.1f} MB of logits, {r['GBps']:.0f} GB/s = {100 * r['of_copy']:.0f} % of copy, "
          f"splits {r['splits']}", flush=True)
    del bufs

    cache = torch.randn((R, LAYERS, 2, S, NKV, H), device="cuda", generator=g, dtype=torch.float32).to(torch.bfloat16) if SMALL else \
        torch.empty((R, LAYERS, 2, S, NKV, H), device="cuda", dtype=torch.bfloat16).normal_(generator=g)
    prompt = torch.randint(0, V, (R, S), device="cuda", generator=g)
    mask = torch.zeros((R, S), dtype=torch.bool, device="cuda")
    parents = torch.randint(0, NB, (R,), device="cuda", generator=g).to(torch.int32)
    tokens = torch.randint(0, V, (R,), device="cuda", generator=g).to(torch.int32)
    own = torch.arange(R, dtype=torch.int32) % NB
    moved = int((parents.cpu() != own).sum())
    # rows that are read: the distinct (group, parent) pairs among the rows that move (children of one parent share its read through the caches)
    sources = len({(r // NB, int(p)) for r, p in enumerate(parents.cpu().tolist()) if p != r % NB})
    for fill in FILLS:
        index = min(fill, S - 1)
        state = [cache]

        def re_fused():
            route(True)
            F.beam_reorder(cache, prompt, mask, parents, tokens, index, NB, length=fill)

        def re_composed():
            route(False)
            state[0] = F.beam_reorder(cache, prompt, mask, parents, tokens, index, NB, length=fill)[0]

        r = measure({"fused": (re_fused, iters), "composed": (re_composed, max(1, iters // 4))})
        state[0] = None
        prefix = LAYERS * 2 * fill * NKV * H * 2
        must = (moved + sources) * prefix
        r.update(rows_moved=moved, rows_read=sources, prefix_bytes_per_row=prefix, bytes=must, at_most_bytes=2 * R * prefix,
                 whole_cache_bytes=cache.numel() * 2,
                 GBps=must / r["fused"]["median_us"] / 1e3, speedup=r["composed"]["median_us"] / r["fused"]["median_us"])
        r["of_copy"] = r["GBps"] / copy_rate
        res["reorder"][f"R{R} fill{fill}"] = r
        print(f"reorder R {R:2d} filled {fill:4d}: fused {r['fused']['median_us']:9.1f} us ({r['fused']['min_us']:.1f}..{r['fused']['max_us']:.1f}), "
              f"composed {r['composed']['median_us']:10.1f} us ({r['composed']['min_us']:.1f}..{r['composed']['max_us']:.1f}), composed / fused "
              f"{r['speedup']:7.2f}; {moved} of {R} rows written, {sources} read, {must / 1e6:.1f} MB, {r['GBps']:.0f} GB/s = "
              f"{100 * r['of_copy']:.0f} % of copy", flush=True)
        s_us = res["select"][f"R{R}"]
        step_f, step_c = s_us["fused"]["median_us"] + r["fused"]["median_us"], s_us["composed"]["median_us"] + r["composed"]["median_us"]
        step_r = s_us["reference"]["median_us"] + r["composed"]["median_us"]
        res["reorder"][f"R{R} fill{fill}"]["step"] = {"fused_us": step_f, "composed_us": step_c, "speedup": step_c / step_f, "reference_us": step_r,
                                                      "speedup_reference": step_r / step_f}
        print(f"step    R {R:2d} filled {fill:4d}: fused {step_f:9.1f} us, composed {step_c:10.1f} us, composed / fused {step_c / step_f:7.2f}, "
              f"reference ops {step_r:10.1f} us, reference / fused {step_r / step_f:7.2f}", flush=True)
    del cache, prompt, mask

if "--no-model" not in sys.argv:
    from iseg_amd import nn
    from iseg_amd.nlp.gemma import GemmaBackbone, GemmaCausalLM
    from iseg_amd.nlp.samplers import BeamSampler
    from iseg_amd.param_store import ParamStore

    nn.set_compute_dtype(torch.bfloat16)
    nn.set_device("cuda:0")
    cfg = dict(vocabulary_size=1000, num_layers=2, num_query_heads=4, num_key_value_heads=1, hidden_dim=256, intermediate_dim=1024, head_dim=64) \
        if SMALL else dict(vocabulary_size=256000, num_layers=2, num_query_heads=8, num_key_value_heads=1, hidden_dim=2048,
                           intermediate_dim=32768, head_dim=256)
    plen, length = (4, 24) if SMALL else (16, 272)
    model = GemmaCausalLM(GemmaBackbone(**cfg))
    with nn.dry_run_scope():
        model({"token_ids": torch.zeros(1, 8, dtype=torch.int64, device="cuda"), "padding_mask": torch.ones(1, 8, dtype=torch.int32, device="cuda")})
    model._iseg_store = ParamStore(list(model.parameters()))
    model._iseg_store.sync_shadow()
    res["generate"] = {"config": cfg, "prompt": plen, "length": length}

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    ids = torch.randint(1, cfg["vocabulary_size"], (1, length), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    mask = torch.zeros(1, length, dtype=torch.bool, device="cuda")
    mask[:, :plen] = True
    inputs = {"token_ids": ids * mask, "padding_mask": mask}
    seed_s = None
    for name, sampler, fused in (("greedy", "greedy", True), ("beam 1 fused", BeamSampler(num_beams=1), True), ("beam 4 fused", BeamSampler(num_beams=4), True),
                                 ("beam 1 composed", BeamSampler(num_beams=1), False), ("beam 4 composed", BeamSampler(num_beams=4), False)):
        route(fused)
        model.compile(sampler=sampler)
        wall(lambda: model.generate_step(inputs))      # warm-up of every shape
        if seed_s is None:
            seed_s = statistics.median(wall(lambda: model._build_cache(inputs["token_ids"])) for _ in range(3))
        total_s = statistics.median(wall(lambda: model.generate_step(inputs)) for _ in range(3))
        per_token_us = (total_s - seed_s) / (length - plen) * 1e6
        res["generate"][name] = {"seed_ms": seed_s * 1e3, "total_ms": total_s * 1e3, "per_token_us": per_token_us, "tokens_per_s": 1e6 / per_token_us}
        print(f"generate_step {name:16s}: {length - plen} tokens, seeding pass {seed_s * 1e3:.2f} ms, whole call {total_s * 1e3:.2f} ms, "
              f"{per_token_us:.1f} us per token = {1e6 / per_token_us:.0f} tokens/s (host launches included)", flush=True)
    os.environ.pop("ISEG_BEAM_FUSED", None)

for a in sys.argv:
    if a == "--json":
        path = sys.argv[sys.argv.index(a) + 1]
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        json.dump(res, open(path, "w"), indent=1)
