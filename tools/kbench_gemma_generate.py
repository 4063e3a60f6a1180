#!/usr/bin/env python3
"""Per-token wall time of GemmaCausalLM.generate_step, the eager loop against the decode step replayed from one captured HIP graph
(compile(graph_decode=True)), on the configuration of the `generate_step` table of profiles/gemma_decode_kbench.md: 2 layers, hidden 2048,
intermediate 32768, 8 query heads on 1 key/value head, head width 256, vocabulary 256000, bf16; prompts of 16 tokens generated to 272 positions
at batch 1 and 8; greedy and TopKSampler(k=5).  Then a deeper model of the same width (18 layers, vocabulary 8192), where a step is several
hundred launches.  Wall clock around the call with a device synchronise, median of 3 after a warm-up (which also captures the graph); the
seeding pass is timed on its own and subtracted, as the table does.  The arms are interleaved.  The graphed tokens are checked against the
eager ones before anything is timed.  On a tree without graph_decode (the parent commit) only the eager arm runs.
usage: python3 tools/kbench_gemma_generate.py [--json PATH] [--small] [--no-deep]"""
import inspect
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from iseg_amd import nn  # noqa: E402
from iseg_amd.nlp.gemma import GemmaBackbone, GemmaCausalLM  # noqa: E402
from iseg_amd.nlp.samplers import TopKSampler  # noqa: E402
from iseg_amd.param_store import ParamStore  # noqa: E402

SMALL = "--small" in sys.argv
HAS_GRAPH = "graph_decode" in inspect.signature(GemmaCausalLM.compile).parameters
WIDTH = dict(num_query_heads=4, num_key_value_heads=1, hidden_dim=256, intermediate_dim=1024, head_dim=64) if SMALL else \
    dict(num_query_heads=8, num_key_value_heads=1, hidden_dim=2048, intermediate_dim=32768, head_dim=256)
MODELS = [("2 layers", dict(vocabulary_size=1000 if SMALL else 256000, num_layers=2, **WIDTH), (1, 2) if SMALL else (1, 8))]
if "--no-deep" not in sys.argv:
    MODELS.append(("18 layers", dict(vocabulary_size=1000 if SMALL else 8192, num_layers=4 if SMALL else 18, **WIDTH), (1,)))
PROMPT, LENGTH = (4, 24) if SMALL else (16, 272)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def sampler(name):
    return "greedy" if name == "greedy" else TopKSampler(k=5, seed=1)


nn.set_compute_dtype(torch.bfloat16)
nn.set_device("cuda:0")
res = {"prompt": PROMPT, "length": LENGTH, "graph_decode": HAS_GRAPH, "rows": []}
for label, cfg, batches in MODELS:
    model = GemmaCausalLM(GemmaBackbone(**cfg))
    with nn.dry_run_scope():
        model({"token_ids": torch.zeros(1, 8, dtype=torch.int64, device="cuda"), "padding_mask": torch.ones(1, 8, dtype=torch.int32, device="cuda")})
    model._iseg_store = ParamStore(list(model.parameters()))
    model._iseg_store.sync_shadow()
    for B in batches:
        ids = torch.randint(1, cfg["vocabulary_size"], (B, LENGTH), device="cuda", generator=torch.Generator(device="cuda").manual_seed(B))
        mask = torch.zeros(B, LENGTH, dtype=torch.bool, device="cuda")
        mask[:, :PROMPT] = True
        inputs = {"token_ids": ids * mask, "padding_mask": mask}
        seed_s = None
        for name in ("greedy", "top_k"):
            arms = {"eager": False, "graphed": True} if HAS_GRAPH else {"eager": False}
            outs = {}
            for arm, graph in arms.items():      # warm-up of every shape; the graphed arm captures here
                model.compile(sampler=sampler(name), **({"graph_decode": graph} if HAS_GRAPH else {}))
                outs[arm] = model.generate_step(inputs)["token_ids"]
            if HAS_GRAPH:
                assert torch.equal(outs["eager"], outs["graphed"]), f"{label} B {B} {name}: the graphed tokens are not the eager ones"
            if seed_s is None:
                seed_s = statistics.median(wall(lambda: model._build_cache(inputs["token_ids"])) for _ in range(3))
            totals = {arm: [] for arm in arms}
            for _ in range(3):
                for arm, graph in arms.items():
                    model.compile(sampler=sampler(name), **({"graph_decode": graph} if HAS_GRAPH else {}))
                    totals[arm].append(wall(lambda: model.generate_step(inputs)))
            row = {"model": label, "B": B, "sampler": name, "seed_ms": seed_s * 1e3}
            for arm, ts in totals.items():
                per = [(t - seed_s) / (LENGTH - PROMPT) * 1e6 for t in ts]
                row[arm] = {"per_token_us": statistics.median(per), "min_us": min(per), "max_us": max(per), "total_ms": statistics.median(ts) * 1e3}
            res["rows"].append(row)
            line = ", ".join(f"{arm} {r['per_token_us']:.1f} us per token ({r['min_us']:.1f}..{r['max_us']:.1f})" for arm, r in row.items()
                             if isinstance(r, dict))
            ratio = f", eager / graphed {row['eager']['per_token_us'] / row['graphed']['per_token_us']:.2f}" if HAS_GRAPH else ""
            print(f"{label:9s} B {B} {name:6s}: seeding pass {seed_s * 1e3:.2f} ms, {line}{ratio}", flush=True)
    if HAS_GRAPH:
        model.release_decode_graphs()
    del model
    torch.cuda.empty_cache()

for a in sys.argv:
    if a == "--json":
        path = sys.argv[sys.argv.index(a) + 1]
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        json.dump(res, open(path, "w"), indent=1)
