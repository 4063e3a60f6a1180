#!/usr/bin/env python3
"""One contrastive-search step (csrc/contrastive.hip: F.contrastive_candidates, two launches; F.contrastive_select, two launches;
F.contrastive_commit, one launch) against the composed route (ISEG_CONTRASTIVE_FUSED=0: the same three functions in torch) and against the
reference's bare op sequence on the same tensors, at Gemma-2B's head and cache: V = 256000 bf16 logits, hidden width D = 2048, cache
[B k, 18, 2, 4096, 1, 256] bf16 of which 128, 1024 or 4096 positions are filled (the history and the prompt have one position more, so that
the full cache still has a step to take; its commit lands on the last cache position), B k = 5, 20 and 40 rows in groups of k = 5 candidates.  The
model's forward pass on the B k candidate rows is common to all three and is not part of the step.

  fused      candidates read the winners' rows of the [B k, V] logits through the row map; select streams the filled prefix of the history
             once; commit moves one cache position.
  composed   index_select of the winners' logits, fp32 softmax, top-k with the order pinned down (a second, integer top-k); the history
             repeated k times, a batched matmul, norms, max, argmax; index_select of the WHOLE cache by the winners and repeat_interleave k
             times into a new tensor.
  reference  keras_nlp's ops and nothing else: softmax, top_k; repeat_interleave of the whole B-row cache to B k rows (create_beams) and
             the gather of the winners back to B rows (gather_best_token); repeat of the history, matmul, norms, divide, max, argmax; a new
             history tensor with the winner's row (slice_update); the gather of the winners' logits.

Device events around a warm loop, several rounds, medians and the min..max spread; the arms are interleaved round by round.  The logits walk
a ring of buffers of 512 MB in all, larger than the 256 MB last-level cache.  `copy` is the rate of one torch copy of 1 GiB (read + write bytes
over time), the yardstick.  The fused and the composed route must agree before anything is timed.
usage: python3 tools/kbench_contrastive.py [rounds] [iters per round] [--json PATH] [--small]"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from iseg_amd import functional as F  # noqa: E402
from iseg_amd import kernels as K  # noqa: E402

RING_BYTES = 512 << 20
args = [a for a in sys.argv[1:] if not a.startswith("--") and not a.endswith(".json")]
rounds = int(args[0]) if len(args) > 0 else 5
iters = int(args[1]) if len(args) > 1 else 10
SMALL = "--small" in sys.argv
V, D = (4099, 256) if SMALL else (256000, 2048)
LAYERS, S, NKV, H = (2, 64, 1, 64) if SMALL else (18, 4096, 1, 256)
ROWS = (5, 10) if SMALL else (5, 20, 40)
FILLS = (8, 64) if SMALL else (128, 1024, 4096)      # index: the positions < index are filled; the step writes cache position min(index, S - 1)
KC, ALPHA, T = 5, 0.6, 1.0


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3      # us per call


def route(fused):
    os.environ["ISEG_CONTRASTIVE_FUSED"] = "1" if fused else "0"


def measure(arms):
    for fn, _ in arms.values():
        for _ in range(2):
            fn()
    times = {k: [] for k in arms}
    for _ in range(rounds):
        for k, (fn, n) in arms.items():
            times[k].append(timed(fn, n))
    return {k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for k, v in times.items()}


def spread(r):
    return f"{r['median_us']:9.1f} us ({r['min_us']:.1f}..{r['max_us']:.1f})"


res = {"rounds": rounds, "iters": iters, "V": V, "D": D, "cache": [LAYERS, 2, S, NKV, H], "k": KC, "alpha": ALPHA, "steps": {}}
big = torch.empty((64 << 20) if SMALL else (1 << 30), dtype=torch.uint8, device="cuda")
dst = torch.empty_like(big)
copy_us = statistics.median(timed(lambda: dst.copy_(big), 5) for _ in range(rounds))
res["copy_GBps"] = copy_rate = 2 * big.numel() / copy_us / 1e3
print(f"copy of {big.numel() >> 20} MiB: {copy_us:.1f} us, {copy_rate:.0f} GB/s read + write", flush=True)
del big, dst

for R in ROWS:
    B = R // KC
    g = torch.Generator(device="cuda").manual_seed(R)
    nbytes = R * V * 2
    ring = 2 if SMALL else max(2, min(64, -(-RING_BYTES // nbytes)))
    logits = (2.0 * torch.randn((ring, R, V), device="cuda", generator=g, dtype=torch.float32)).to(torch.bfloat16)
    cache = torch.empty((R, LAYERS, 2, S, NKV, H), device="cuda", dtype=torch.bfloat16).normal_(generator=g)
    cache_b = cache[::KC].contiguous()      # the reference's B-row state
    prompt = torch.randint(0, V, (R, S + 1), device="cuda", generator=g)
    hist = torch.empty((B, S + 1, D), device="cuda", dtype=torch.bfloat16).normal_(generator=g)
    cand = torch.empty((R, D), device="cuda", dtype=torch.bfloat16).normal_(generator=g)
    prev = torch.randint(0, KC, (B,), device="cuda", generator=g).to(torch.int32)      # the previous step's winners: the row map
    rows_prev = (torch.arange(B, device="cuda") * KC + prev.long())
    for fill in FILLS:
        index, pos = fill, min(fill, S - 1)
        # ---- agreement first --------------------------------------------------------------------------------------------------------------
        outs = {}
        for fused in (True, False):
            route(fused)
            probs, tokens = F.contrastive_candidates(logits[0], KC, T, prev)
            winner, scores, max_sim = F.contrastive_select(hist, index, cand, probs.reshape(-1), ALPHA)
            c2, p2, h2 = F.contrastive_commit(cache.clone() if fused else cache, prompt.clone(), hist.clone(), cand, winner, index, KC, pos)
            outs[fused] = (probs, tokens, winner, scores, max_sim, c2[:, :, :, pos].clone(), p2[:, index].clone(), h2[:, index].clone())
            del c2
        a, b = outs[True], outs[False]
        assert torch.equal(a[1], b[1]), "the candidates' tokens differ"
        assert bool(((a[0] - b[0]).abs() <= 1e-5 * b[0] + 1e-30).all()), "the probabilities differ"
        assert bool((a[4] - b[4]).abs().max() <= (2 * D + 8) * 2.0 ** -23) and bool((a[3] - b[3]).abs().max() <= (2 * D + 8) * 2.0 ** -23), "scores differ"
        assert torch.equal(a[2], b[2]) or bool((b[3].view(B, KC).max(-1).values - b[3].view(B, KC).gather(1, a[2].long()[:, None])[:, 0]).max() < 1e-3)
        if torch.equal(a[2], b[2]):
            assert torch.equal(a[5], b[5]) and torch.equal(a[6], b[6]) and torch.equal(a[7], b[7]), "the commits differ"
        del outs, a, b
        torch.cuda.empty_cache()

        turn = [0, 0, 0]
        keep = [None]

        def cand_fused():
            route(True)
            turn[0] = (turn[0] + 1) % ring
            return F.contrastive_candidates(logits[turn[0]], KC, T, prev)

        probs, _ = cand_fused()
        probs = probs.reshape(-1)
        winner = F.contrastive_select(hist, index, cand, probs, ALPHA)[0]

        def select_fused():
            route(True)
            return F.contrastive_select(hist, index, cand, probs, ALPHA)

        def commit_fused():
            route(True)
            F.contrastive_commit(cache, prompt, hist, cand, winner, index, KC, pos)

        def step_fused():
            p, _ = cand_fused()
            w = F.contrastive_select(hist, index, cand, p.reshape(-1), ALPHA)[0]
            F.contrastive_commit(cache, prompt, hist, cand, w, index, KC, pos)

        def step_composed():
            route(False)
            turn[1] = (turn[1] + 1) % ring
            p, _ = F.contrastive_candidates(logits[turn[1]], KC, T, prev)
            w = F.contrastive_select(hist, index, cand, p.reshape(-1), ALPHA)[0]
            keep[0] = None
            keep[0] = F.contrastive_commit(cache, prompt, hist, cand, w, index, KC, pos)[0]

        def step_reference():
            turn[2] = (turn[2] + 1) % ring
            x = logits[turn[2]].index_select(0, rows_prev)      # gather_best_token on the logits
            p, _ = torch.topk(torch.softmax(x.float() / T, dim=-1), KC, dim=-1)
            keep[0] = None
            beams = torch.repeat_interleave(cache_b, KC, dim=0)      # create_beams on the cache
            h1 = torch.repeat_interleave(hist[:, :index], KC, dim=0)
            h2 = cand[:, :, None]
            sim = torch.matmul(h1, h2)[:, :, 0] / (torch.linalg.vector_norm(h1, dim=-1) * torch.linalg.vector_norm(h2, dim=-2))
            score = (1.0 - ALPHA) * p.reshape(-1).to(sim.dtype) - ALPHA * torch.max(sim, dim=-1).values
            rows = torch.arange(B, device="cuda") * KC + torch.argmax(score.view(B, KC), dim=-1)
            keep[0] = beams.index_select(0, rows)      # gather_best_token on the cache
            new_hist = hist.clone()      # slice_update returns a new tensor
            new_hist[:, index] = cand.index_select(0, rows)

        r = measure({"fused": (step_fused, iters), "composed": (step_composed, max(1, iters // 2)), "reference": (step_reference, max(1, iters // 2)),
                     "candidates": (cand_fused, 4 * iters), "select": (select_fused, 4 * iters), "commit": (commit_fused, 4 * iters)})
        keep[0] = None
        hist_bytes = B * index * D * 2
        r.update(hist_bytes=hist_bytes, logit_bytes=B * V * 2, commit_bytes=R * LAYERS * 2 * NKV * H * 2,
                 select_GBps=hist_bytes / r["select"]["median_us"] / 1e3, candidates_GBps=B * V * 2 / r["candidates"]["median_us"] / 1e3,
                 select_splits=K.contrastive_select_splits(B, index, D, KC, torch.bfloat16), whole_cache_bytes=cache.numel() * 2,
                 speedup=r["composed"]["median_us"] / r["fused"]["median_us"], speedup_reference=r["reference"]["median_us"] / r["fused"]["median_us"])
        res["steps"][f"R{R} fill{fill}"] = r
        print(f"step R {R:2d} filled {fill:4d}: fused {spread(r['fused'])}, composed {spread(r['composed'])}, composed / fused {r['speedup']:7.2f}, "
              f"reference ops {spread(r['reference'])}, reference / fused {r['speedup_reference']:7.2f}", flush=True)
        print(f"     kernels: candidates {spread(r['candidates'])} {r['candidates_GBps']:.0f} GB/s of {B * V * 2 / 1e6:.1f} MB; select "
              f"{spread(r['select'])} {r['select_GBps']:.0f} GB/s = {100 * r['select_GBps'] / copy_rate:.0f} % of copy of {hist_bytes / 1e6:.1f} MB "
              f"in {r['select_splits']} chunks; commit {spread(r['commit'])} of {r['commit_bytes'] / 1e6:.2f} MB", flush=True)
    del logits, cache, cache_b, prompt, hist, cand
    torch.cuda.empty_cache()

os.environ.pop("ISEG_CONTRASTIVE_FUSED", None)
for a in sys.argv:
    if a == "--json":
        path = sys.argv[sys.argv.index(a) + 1]
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        json.dump(res, open(path, "w"), indent=1)
