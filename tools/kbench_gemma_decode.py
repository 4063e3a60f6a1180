#!/usr/bin/env python3
"""Single-token attention over a key/value cache (csrc/gemma_decode.hip, iseg_gemma_decode_attention: the split-KV pass and the merge) at the
head layouts of Gemma-2B (nq 8, nkv 1, h 256) and Gemma-7B (16, 16, 256), batch 1 and 8, 1 024 and 8 192 visible keys.  Device events around a
warm loop, several rounds, medians and the min..max spread; the arms are interleaved round by round.
  fused      one call of K.gemma_decode_attention with the launcher's own chunk plan (two launches)
  hot        the same call on ONE cache over and over: it stays in the last-level cache, so this is not an HBM figure
  composed   F.gemma_cached_attention_core with ISEG_GEMMA_FUSED=0 (a packed [B, S, .] copy, repeated K / V, attention_packed with a T x T
             mask): the yardstick route, timed only where its T x T tensors stay below 5 GB
The cache bytes are 2 * keys * nkv * h * 2 per sample; the ratio printed is the fused call's time over those bytes at 6.3 TB/s (the measured
copy rate of the chip).  The fused arm walks a ring of caches larger than the 256 MB last-level cache, so every call reads its cache from HBM.
The fused result is compared with the composed one (or, where that is not run, with a second chunk count) before anything is timed.

Then the per-token time of GemmaCausalLM.generate_step on a 2-layer model of Gemma-2B's width (hidden 2048, intermediate 32768, vocabulary
256000), batch 1 and 8: prompts of 16 tokens generated to 272 positions; the seeding pass is timed on its own and subtracted.
usage: python3 tools/kbench_gemma_decode.py [rounds] [iters per round] [--json PATH] [--small] [--no-model]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from iseg_amd import functional as F  # noqa: E402
from iseg_amd import kernels as K  # noqa: E402
from iseg_amd import nn  # noqa: E402

COPY_RATE = 6.3e12
RING_BYTES = 512 << 20
COMPOSED_LIMIT = 5e9
args = [a for a in sys.argv[1:] if not a.startswith("--") and not a.endswith(".json")]
rounds = int(args[0]) if len(args) > 0 else 5
iters = int(args[1]) if len(args) > 1 else 50
SMALL = "--small" in sys.argv
LAYOUTS = {"2B": (8, 1, 256), "7B": (16, 16, 256)}
BATCHES = (1, 2) if SMALL else (1, 8)
KEYS = (128, 320) if SMALL else (1024, 8192)


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3      # us per call


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


nn.set_compute_dtype(torch.bfloat16)
nn.set_device("cuda:0")
res = {"rounds": rounds, "iters": iters, "arms": {}}
for name, (nq, nkv, h) in LAYOUTS.items():
    for B in BATCHES:
        for keys in KEYS:
            S, pos0 = keys, keys - 1
            cache_bytes = B * 2 * keys * nkv * h * 2
            ring = max(2, min(512, -(-RING_BYTES // cache_bytes))) if not SMALL else 2
            g = torch.Generator(device="cuda").manual_seed(keys + B)
            caches = torch.randn((ring, B, 2, S, nkv, h), device="cuda", generator=g, dtype=torch.float32).to(torch.bfloat16)
            q = torch.randn((B, 1, nq * h), device="cuda", generator=g, dtype=torch.float32).to(torch.bfloat16)
            scale = float(h) ** -0.5
            splits = K.gemma_decode_attention_splits(B, pos0, 1, nq, nkv, h)
            turn = [0]

            def fused():
                turn[0] = (turn[0] + 1) % ring
                K.gemma_decode_attention(q, caches[turn[0]], pos0, nq, nkv, h, scale)

            def hot():
                K.gemma_decode_attention(q, caches[0], pos0, nq, nkv, h, scale)

            def comp():
                os.environ["ISEG_GEMMA_FUSED"] = "0"
                try:
                    return F.gemma_cached_attention_core(q, caches[0], pos0, nq, nkv, h)
                finally:
                    os.environ.pop("ISEG_GEMMA_FUSED", None)

            run_composed = B * nq * S * S * 4.0 <= COMPOSED_LIMIT
            got = K.gemma_decode_attention(q, caches[0], pos0, nq, nkv, h, scale)
            want = comp() if run_composed else K.gemma_decode_attention(q, caches[0], pos0, nq, nkv, h, scale, splits=1)
            err = rel(got, want)
            assert err < 1.5e-2, f"{name} B {B} keys {keys}: the routes disagree ({err:.3e})"
            arms = {"fused": (fused, iters), "hot": (hot, iters)}
            if run_composed:
                arms["composed"] = (comp, max(1, iters // 25))
            for fn, _ in arms.values():
                for _ in range(3):
                    fn()
            times = {k: [] for k in arms}
            for _ in range(rounds):
                for k, (fn, n) in arms.items():
                    times[k].append(timed(fn, n))
            r = {k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for k, v in times.items()}
            floor_us = cache_bytes / COPY_RATE * 1e6
            r.update(cache_bytes=cache_bytes, splits=splits, ring=ring, floor_us=floor_us, ratio=r["fused"]["median_us"] / floor_us,
                     routes_rel=err)
            res["arms"][f"{name} B{B} keys{keys}"] = r
            line = (f"{name} nq {nq:2d} nkv {nkv:2d} h {h} B {B} keys {keys:5d}: fused {r['fused']['median_us']:8.1f} us "
                    f"({r['fused']['min_us']:.1f}..{r['fused']['max_us']:.1f}), hot {r['hot']['median_us']:8.1f} us, splits {splits:3d}, cache "
                    f"{cache_bytes / 1e6:8.2f} MB, at 6.3 TB/s {floor_us:7.2f} us, ratio {r['ratio']:6.1f}")
            line += f", composed {r['composed']['median_us']:10.1f} us" if run_composed else ", composed not run"
            print(line, flush=True)
            del caches

if "--no-model" not in sys.argv:
    from iseg_amd.nlp.gemma import GemmaBackbone, GemmaCausalLM
    from iseg_amd.param_store import ParamStore

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
    for B in BATCHES:
        ids = torch.randint(1, cfg["vocabulary_size"], (B, length), device="cuda", generator=torch.Generator(device="cuda").manual_seed(B))
        mask = torch.zeros(B, length, dtype=torch.bool, device="cuda")
        mask[:, :prompt] = True
        inputs = {"token_ids": ids * mask, "padding_mask": mask}

        def wall(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        wall(lambda: model.generate_step(inputs))      # warm-up of every shape
        seed_s = statistics.median(wall(lambda: model._build_cache(inputs["token_ids"])) for _ in range(3))
        total_s = statistics.median(wall(lambda: model.generate_step(inputs)) for _ in range(3))
        per_token_us = (total_s - seed_s) / (length - prompt) * 1e6
        res["generate"][f"B{B}"] = {"seed_ms": seed_s * 1e3, "total_ms": total_s * 1e3, "per_token_us": per_token_us}
        print(f"generate_step B {B}: {length - prompt} tokens, seeding pass {seed_s * 1e3:.2f} ms, whole call {total_s * 1e3:.2f} ms, "
              f"{per_token_us:.1f} us per token (host launches included)", flush=True)

for a in sys.argv:
    if a == "--json":
        path = sys.argv[sys.argv.index(a) + 1]
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        json.dump(res, open(path, "w"), indent=1)
