"""ContrastiveSampler on the host: the composed route (plain torch) of iseg_amd.nlp.samplers.ContrastiveSampler, F.contrastive_candidates,
F.contrastive_select and F.contrastive_commit against the fp64 oracle of tests/contrastive_ref.py on `next` functions small enough to check by
hand, the refusals, the configuration round trip, what GemmaCausalLM accepts and passes, and the host arithmetic and refusals of the C entry
points.  No GPU: CPU tensors take the composed route."""
import ctypes
import os
import re

import pytest
import torch

from tests import contrastive_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 1      # the token that contrastive search prefers in the hand-made model


def _model(table, hidden):
    """next whose logits and hidden state depend on the previous token alone: rows table[prompt[:, index - 1]] and hidden[prompt[:, index - 1]];
    records the (index, rows) it was asked for"""
    seen = []

    def next(prompt, cache, index):
        seen.append((index, prompt.shape[0]))
        tok = prompt[:, index - 1].long()
        return table[tok].clone(), hidden[tok].clone(), cache

    return next, seen


def _hand():
    """6 tokens with orthogonal hidden states (e_token).  After token 0: token 0 again has p = 0.6, A has 0.3, the rest 0.1 together.  Token 0
    repeats the hidden state of the prompt's token exactly (similarity 1); every other token has similarity 0 to it."""
    p = torch.full((6, 6), 1.0 / 6.0, dtype=torch.float64)
    p[0] = torch.tensor([0.6, 0.3, 0.025, 0.025, 0.025, 0.025])
    return torch.log(p).float(), torch.eye(6, 8)


def _random(V, D, seed):
    gen = torch.Generator().manual_seed(seed)
    return 3.0 * torch.randn(V, V, generator=gen), torch.randn(V, D, generator=gen)


def _history(hidden, prompt):
    return hidden[prompt.long()].clone()


def test_contrastive_search_avoids_the_repetition_that_greedy_takes():
    from iseg_amd.nlp.gemma.gemma_causal import greedy_sample
    from iseg_amd.nlp.samplers import ContrastiveSampler

    table, hidden = _hand()
    prompt = torch.zeros(1, 2, dtype=torch.int64)
    mask = torch.tensor([[True, False]])
    nxt, seen = _model(table, hidden)
    assert greedy_sample(nxt, prompt, None, 1, mask)[0, 1].item() == 0      # the repetition
    # the two scores at alpha = 0.6: the repetition has similarity 1 to position 0, A has 0
    repeat, other = 0.4 * 0.6 - 0.6 * 1.0, 0.4 * 0.3 - 0.6 * 0.0
    assert repeat < 0 < other
    hs = _history(hidden, prompt)
    before = hs.clone()
    del seen[:]
    out = ContrastiveSampler(k=2, alpha=0.6)(nxt, prompt, None, 1, mask, hidden_states=hs)
    assert out.tolist() == [[0, A]] and tuple(out.shape) == (1, 2) and out.dtype == prompt.dtype
    assert seen == [(1, 1), (2, 2)]      # once on the B rows, then on the B k candidate rows
    assert prompt.tolist() == [[0, 0]] and torch.equal(hs, before)      # the caller's tensors are not written
    # the functional pieces on that step
    from iseg_amd import functional as F

    probs, tokens = F.contrastive_candidates(table[[0]], 2)
    assert tokens.tolist() == [[0, A]] and tokens.dtype == torch.int32 and probs.dtype == torch.float32
    assert torch.allclose(probs, torch.tensor([[0.6, 0.3]]), atol=1e-6)
    winner, scores, max_sim = F.contrastive_select(hs, 1, hidden[[0, A]], probs.reshape(-1), 0.6)
    assert winner.tolist() == [1] and winner.dtype == torch.int32 and max_sim.tolist() == [1.0, 0.0]
    assert abs(scores[0].item() - repeat) < 1e-6 and abs(scores[1].item() - other) < 1e-6
    assert ContrastiveSampler(k=2, alpha=0.0)(nxt, prompt, None, 1, mask, hidden_states=hs).tolist() == [[0, 0]]


@pytest.mark.parametrize("k,alpha", [(1, 0.0), (1, 0.5), (1, 1.0), (2, 0.0), (5, 0.0), (16, 0.0)])
def test_alpha_zero_and_one_candidate_are_greedy(k, alpha):
    from iseg_amd.nlp.gemma.gemma_causal import greedy_sample
    from iseg_amd.nlp.samplers import ContrastiveSampler

    V = 23
    table, hidden = _random(V, 16, 1)      # continuous values: no ties
    prompt = torch.randint(0, V, (3, 9), generator=torch.Generator().manual_seed(2))
    mask = torch.zeros(3, 9, dtype=torch.bool)
    for b, n in enumerate((2, 4, 3)):
        mask[b, :n] = True
    for end in (None, 5):
        nxt, _ = _model(table, hidden)
        want = greedy_sample(nxt, prompt, None, 2, mask, end_token_id=end)
        got = ContrastiveSampler(k=k, alpha=alpha)(nxt, prompt, None, 2, mask, end_token_id=end, hidden_states=_history(hidden, prompt))
        assert torch.equal(got, want), (k, alpha, end)


@pytest.mark.parametrize("k,alpha,T", [(2, 0.6, 1.0), (3, 0.5, 0.7), (5, 0.5, 1.0), (5, 0.9, 2.0), (16, 0.3, 1.0)])
def test_the_loop_against_the_oracle_with_user_tokens_on_the_longer_rows(k, alpha, T):
    from iseg_amd.nlp.samplers import ContrastiveSampler

    V, D, S = 29, 16, 10
    table, hidden = _random(V, D, 10 * k + 3)
    prompt = torch.randint(0, V, (3, S), generator=torch.Generator().manual_seed(4))
    mask = torch.zeros(3, S, dtype=torch.bool)
    for b, n in enumerate((2, 5, 3)):
        mask[b, :n] = True
    hs = _history(hidden, prompt)
    nxt, _ = _model(table, hidden)
    want, margin = R.contrastive_search(nxt, prompt, None, 2, mask, hs, k, alpha, T)
    print(f"k {k} alpha {alpha} T {T}: the oracle's smallest winning margin is {margin:.3e}")
    assert margin > 4 * R.eps_score(alpha, D), "the hand-made model leaves no clear winner: choose another seed"
    cache = torch.arange(3.0).reshape(3, 1, 1, 1, 1, 1).repeat(1, 2, 2, S, 1, 4)      # rides along: row b holds b
    got = ContrastiveSampler(k=k, alpha=alpha, temperature=T)(nxt, prompt, cache, 2, mask, hidden_states=hs)
    assert torch.equal(got, want)
    assert torch.equal(got[mask], prompt[mask])      # user tokens of the longer rows are kept
    assert torch.equal(cache, torch.arange(3.0).reshape(3, 1, 1, 1, 1, 1).repeat(1, 2, 2, S, 1, 4))


def test_the_loop_stops_when_every_row_holds_an_end_token():
    from iseg_amd.nlp.samplers import ContrastiveSampler

    V, D, S = 11, 8, 12
    table, hidden = _random(V, D, 5)
    prompt = torch.zeros(2, S, dtype=torch.int32)
    prompt[:, 0] = torch.tensor([3, 4])
    mask = torch.zeros(2, S, dtype=torch.bool)
    mask[:, 0] = True
    nxt, seen = _model(table, hidden)
    hs = _history(hidden, prompt)
    full = ContrastiveSampler(k=3, alpha=0.4)(nxt, prompt, None, 1, mask, hidden_states=hs)
    end = int(full[0, 3])
    want, _ = R.contrastive_search(nxt, prompt, None, 1, mask, hs, 3, 0.4, end_token_id=end)
    del seen[:]
    got = ContrastiveSampler(k=3, alpha=0.4)(nxt, prompt, None, 1, mask, end_token_id=end, hidden_states=hs)
    assert torch.equal(got, want.to(got.dtype)) and got.dtype == torch.int32
    steps = len(seen) - 1
    assert bool(((got[:, :1 + steps] == end) & ~mask[:, :1 + steps]).any(dim=-1).all())
    if steps < S - 1:
        assert bool((got[:, 1 + steps:] == 0).all())      # the loop stopped: the rest is the prompt's padding


def test_candidates_composed_pins_the_order_down():
    from iseg_amd import functional as F

    x = torch.tensor([[1.0, 3.0, 3.0, -1.0, 3.0, 0.0], [0.0, float("nan"), 2.0, 1.0, 0.0, 0.0], [float("-inf")] * 5 + [0.5]])
    probs, tokens = F.contrastive_candidates(x, 3)
    assert tokens[0].tolist() == [1, 2, 4] and tokens[1].tolist() == [0, 1, 2] and tokens[2].tolist() == [5, 0, 1]
    assert bool(torch.isnan(probs[1]).all()) and probs[2].tolist() == [1.0, 0.0, 0.0]
    # a row map reads row b g + map[b]
    logits = torch.randn(6, 40, generator=torch.Generator().manual_seed(8))
    row_map = torch.tensor([2, 0], dtype=torch.int32)
    p2, t2 = F.contrastive_candidates(logits, 4, 0.5, row_map)
    p1, t1 = F.contrastive_candidates(logits[[2, 3]], 4, 0.5)
    assert torch.equal(p1, p2) and torch.equal(t1, t2)
    for T in (0.25, 1.0, 4.0):
        p, t = F.contrastive_candidates(logits.bfloat16(), 5, T, row_map)
        bad, worst = R.candidates_accepted(p, t, logits.bfloat16(), 5, T, row_map, units=8)      # torch's fp32 softmax, not the kernel's
        assert not bad, bad


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_select_and_commit_composed_against_the_oracle(dtype):
    from iseg_amd import functional as F

    gen = torch.Generator().manual_seed(21)
    B, k, S, D, index = 3, 5, 12, 24, 7
    hs = torch.randn(B, S, D, generator=gen).to(dtype)
    hs[:, index:] = float("nan")
    cand = torch.randn(B * k, D, generator=gen).to(dtype)
    cand[3] = hs[0, 2]      # a repetition
    probs = torch.softmax(torch.randn(B, 50, generator=gen), -1)[:, :k].reshape(-1).contiguous()
    for alpha in (0.0, 0.5, 1.0):
        winner, scores, max_sim = F.contrastive_select(hs, index, cand, probs, alpha)
        bad, w_ms, w_sc = R.select_accepted(winner, scores, max_sim, hs, index, cand, probs, alpha, k)
        assert not bad, (alpha, bad)
    assert abs(max_sim[3].item() - 1.0) <= R.eps_sim(D)
    prompt = torch.randint(0, 99, (B * k, S), generator=gen)
    for Sc in (S - 3, S + 2):
        cache = torch.randn(B * k, 2, 2, Sc, 1, 8, generator=gen).to(dtype)
        want = R.commit_broadcast(cache, prompt, hs, cand, winner, index, k)
        keep = (cache.clone(), prompt.clone(), hs.clone())
        got = F.contrastive_commit(cache, prompt, hs, cand, winner, index, k)
        rows = (torch.arange(B) * k + winner.long())
        # the composed route gathers whole rows; the groups of this cache are not equal elsewhere, so compare the rows it states
        assert torch.equal(got[1][:, index], want[1][:, index]) and torch.equal(got[2][:, :index + 1], want[2][:, :index + 1])
        assert torch.equal(got[0], torch.repeat_interleave(cache[rows], k, dim=0))
        for t, u in zip((cache, prompt, hs), keep):      # new tensors: the inputs are not written
            assert torch.equal(torch.nan_to_num(t.float()), torch.nan_to_num(u.float()))


def test_refusals_name_the_argument():
    from iseg_amd import functional as F
    from iseg_amd.nlp.samplers import ContrastiveSampler

    table, hidden = _hand()
    nxt, _ = _model(table, hidden)
    prompt, mask = torch.zeros(1, 3, dtype=torch.int64), torch.tensor([[True, False, False]])
    with pytest.raises(ValueError, match="hidden_states"):
        ContrastiveSampler()(nxt, prompt, None, 1, mask)
    with pytest.raises(ValueError, match="hidden_states"):
        ContrastiveSampler()(nxt, prompt, None, 1, mask, hidden_states=None)
    for k in (0, 17, -1, 2.0, True, "5", None):
        with pytest.raises(ValueError, match="k is an integer in 1 .. 16"):
            ContrastiveSampler(k=k)
    for alpha in (-0.1, 1.5, float("nan"), "0.5", None):
        with pytest.raises(ValueError, match="alpha"):
            ContrastiveSampler(alpha=alpha)
    for T in (0.0, -1.0, float("inf")):
        with pytest.raises(ValueError, match="temperature"):
            ContrastiveSampler(temperature=T)
    with pytest.raises(NotImplementedError, match="call the sampler"):
        ContrastiveSampler().get_next_token(torch.zeros(1, 4))
    with pytest.raises(ValueError, match="at least k"):      # k > V
        ContrastiveSampler(k=7)(nxt, prompt, None, 1, mask, hidden_states=_history(hidden, prompt))
    x = torch.randn(4, 10)
    with pytest.raises(ValueError, match="at least k"):
        F.contrastive_candidates(x, 11)
    with pytest.raises(ValueError, match="k is an integer"):
        F.contrastive_candidates(x, 17)
    with pytest.raises(RuntimeError, match="inference only"):
        F.contrastive_candidates(x.clone().requires_grad_(), 2)
    with pytest.raises(ValueError, match="temperature"):
        F.contrastive_candidates(x, 2, 0.0)
    with pytest.raises(ValueError, match="floating point"):
        F.contrastive_candidates(x.long(), 2)
    with pytest.raises(ValueError, match="row_map"):
        F.contrastive_candidates(x, 2, 1.0, torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="whole number"):
        F.contrastive_candidates(x, 2, 1.0, torch.zeros(3, dtype=torch.int32))
    hs, cand, probs = torch.randn(2, 6, 8), torch.randn(4, 8), torch.rand(4)
    with pytest.raises(RuntimeError, match="inference only"):
        F.contrastive_select(hs.clone().requires_grad_(), 3, cand, probs, 0.5)
    with pytest.raises(RuntimeError, match="inference only"):
        F.contrastive_select(hs, 3, cand.clone().requires_grad_(), probs, 0.5)
    with pytest.raises(ValueError, match="alpha"):
        F.contrastive_select(hs, 3, cand, probs, 1.5)
    with pytest.raises(ValueError, match="index"):
        F.contrastive_select(hs, 0, cand, probs, 0.5)
    with pytest.raises(ValueError, match="index"):
        F.contrastive_select(hs, 7, cand, probs, 0.5)
    with pytest.raises(ValueError, match="whole number"):
        F.contrastive_select(hs, 3, torch.randn(5, 8), torch.rand(5), 0.5)
    with pytest.raises(ValueError, match="float32"):
        F.contrastive_select(hs, 3, cand, probs.double(), 0.5)
    with pytest.raises(ValueError, match="dtype"):
        F.contrastive_select(hs, 3, cand.bfloat16(), probs, 0.5)
    with pytest.raises(ValueError, match=r"\[B \* k, D\]"):
        F.contrastive_select(hs, 3, torch.randn(4, 9), probs, 0.5)
    prompt4, winner = torch.zeros(4, 6, dtype=torch.int64), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="winner"):
        F.contrastive_commit(None, prompt4, hs, cand, winner.long(), 3, 2)
    with pytest.raises(ValueError, match="position"):
        F.contrastive_commit(None, prompt4, hs, cand, winner, 6, 2)
    with pytest.raises(ValueError, match="cache"):
        F.contrastive_commit(torch.zeros(3, 1, 2, 6, 1, 8), prompt4, hs, cand, winner, 3, 2)
    with pytest.raises(ValueError, match="cache of 4"):
        F.contrastive_commit(torch.zeros(4, 1, 2, 4, 1, 8), prompt4, hs, cand, winner, 4, 2)
    with pytest.raises(RuntimeError, match="inference only"):
        F.contrastive_commit(None, prompt4, hs.clone().requires_grad_(), cand, winner, 3, 2)
    with pytest.raises(ValueError, match="int32 or int64"):
        F.contrastive_commit(None, prompt4.float(), hs, cand, winner, 3, 2)


def test_dry_run_and_empty_batch_shapes():
    from iseg_amd import functional as F
    from iseg_amd import nn

    hs, cand, probs = torch.randn(2, 6, 8), torch.randn(6, 8), torch.rand(6)
    with nn.dry_run_scope():
        p, t = F.contrastive_candidates(torch.zeros(4, 10), 3)
        assert tuple(p.shape) == (4, 3) and tuple(t.shape) == (4, 3) and t.dtype == torch.int32 and p.dtype == torch.float32
        w, s, m = F.contrastive_select(hs, 3, cand, probs, 0.5)
        assert tuple(w.shape) == (2,) and w.dtype == torch.int32 and tuple(s.shape) == (6,) and tuple(m.shape) == (6,)
    p, t = F.contrastive_candidates(torch.zeros(0, 10), 3)
    assert tuple(p.shape) == (0, 3) and tuple(t.shape) == (0, 3)
    w, s, m = F.contrastive_select(torch.zeros(0, 6, 8), 3, torch.zeros(0, 8), torch.zeros(0), 0.5)
    assert tuple(w.shape) == (0,) and tuple(s.shape) == (0,) and tuple(m.shape) == (0,)


def test_config_round_trip():
    from iseg_amd.nlp.samplers import ContrastiveSampler

    s = ContrastiveSampler()
    assert s.get_config() == {"temperature": 1.0, "k": 5, "alpha": 0.5}      # keras_nlp's defaults
    s = ContrastiveSampler(k=3, alpha=0.25, temperature=0.7)
    t = ContrastiveSampler.from_config(s.get_config())
    assert type(t) is ContrastiveSampler and t.get_config() == s.get_config() == {"temperature": 0.7, "k": 3, "alpha": 0.25}


def test_what_the_model_accepts_and_whom_it_passes_hidden_states(monkeypatch):
    from iseg_amd.nlp.gemma import GemmaBackbone, GemmaCausalLM
    from iseg_amd.nlp.samplers import ContrastiveSampler, Sampler
    from tests.test_gemma_host import TINY

    model = GemmaCausalLM(GemmaBackbone(**TINY))
    sampler = ContrastiveSampler(k=2)
    model.compile(sampler=sampler)
    assert model.sampler is sampler
    model.compile(sampler=sampler, graph_decode=True)
    assert model._graph_decode_sampler() == (False, sampler)      # a contrastive step keeps the eager loop
    with pytest.raises(NotImplementedError, match="BeamSampler"):
        model.compile(sampler="contrastive")
    assert model.sampler is sampler

    # generate_step without a device: the seeding pass and the step are stand-ins; what is checked is who receives hidden_states=
    B, S, D, V = 2, 5, 8, 13
    hs = torch.randn(B, S, D)
    monkeypatch.setattr(model, "_build_cache", lambda token_ids, cache=None: (hs, torch.zeros(B, 1, 2, S, 1, 4)))
    table = torch.randn(V, V, generator=torch.Generator().manual_seed(3))
    hidden = torch.randn(V, D, generator=torch.Generator().manual_seed(4))

    def call_with_cache(token_ids, cache, index):
        tok = token_ids[:, 0].long()
        return table[tok][:, None], hidden[tok][:, None], cache

    monkeypatch.setattr(model, "call_with_cache", call_with_cache)
    inputs = {"token_ids": torch.tensor([[1, 2, 0, 0, 0], [3, 4, 5, 0, 0]]), "padding_mask": torch.tensor([[1, 1, 0, 0, 0], [1, 1, 1, 0, 0]]).bool()}
    got = {}

    class Spy(ContrastiveSampler):
        def __call__(self, next, prompt, cache=None, index=0, mask=None, end_token_id=None, hidden_states=None):
            got["hidden_states"] = hidden_states
            return super().__call__(next, prompt, cache, index, mask, end_token_id=end_token_id, hidden_states=hidden_states)

    model.compile(sampler=Spy(k=3, alpha=0.5))
    out = model.generate_step(inputs)
    assert got["hidden_states"] is hs
    assert tuple(out["token_ids"].shape) == (B, S) and out["token_ids"].dtype == inputs["token_ids"].dtype
    assert torch.equal(out["token_ids"][inputs["padding_mask"]], inputs["token_ids"][inputs["padding_mask"]])
    model.compile(sampler=Spy(k=3, alpha=0.5), graph_decode=True)      # the eager loop: no device is needed
    assert torch.equal(model.generate_step(inputs)["token_ids"], out["token_ids"])

    class Old(Sampler):      # a caller's sampler with the signature of before: it is not passed hidden_states
        def __call__(self, next, prompt, cache=None, index=0, mask=None, end_token_id=None):
            got["old"] = True
            return super().__call__(next, prompt, cache, index, mask, end_token_id)

        def get_next_token(self, logits):
            return torch.argmax(logits, dim=-1)

    model.compile(sampler=Old())
    old = model.generate_step(inputs)["token_ids"]
    assert got["old"] and tuple(old.shape) == (B, S)
    model.compile(sampler="greedy")
    assert torch.equal(model.generate_step(inputs)["token_ids"], old)


def test_the_symbols_are_declared_exported_and_bound():
    from iseg_amd import _hip
    from iseg_amd import functional as F
    from iseg_amd import kernels as K
    from iseg_amd import build
    from iseg_amd.nlp import samplers

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "iseg_hip.h")).read(), flags=re.S)
    names = ("iseg_contrastive_candidates_supported", "iseg_contrastive_candidates_splits", "iseg_contrastive_candidates_scratch_bytes",
             "iseg_contrastive_candidates", "iseg_contrastive_select_supported", "iseg_contrastive_select_splits",
             "iseg_contrastive_select_scratch_bytes", "iseg_contrastive_select", "iseg_contrastive_commit")
    if not os.path.exists(_hip.LIB_PATH):
        build.build(verbose=False)
    dll = ctypes.CDLL(_hip.LIB_PATH)
    for name in names:
        assert re.search(r"\b(?:int|size_t)\s+%s\s*\(" % name, header), name
        assert name in _hip.SIGNATURES and hasattr(dll, name), name
    assert "contrastive.hip" in build.SOURCES
    for mod, fns in ((K, ("contrastive_candidates", "contrastive_candidates_supported", "contrastive_candidates_splits", "contrastive_select",
                          "contrastive_select_supported", "contrastive_select_splits", "contrastive_commit")),
                     (F, ("contrastive_candidates", "contrastive_select", "contrastive_commit", "contrastive_fused"))):
        for fn in fns:
            assert callable(getattr(mod, fn)), fn
    assert F.CONTRASTIVE_MAX_K == 16 and issubclass(samplers.ContrastiveSampler, samplers.Sampler)
    with pytest.raises(_hip.HipCallError):      # no CPU route below F
        K.contrastive_candidates(torch.zeros(2, 4), 2, 1.0)
    with pytest.raises(_hip.HipCallError):
        K.contrastive_select(torch.zeros(1, 4, 8), 2, torch.zeros(2, 8), torch.zeros(2), 0.5)


def test_the_switch(monkeypatch):
    from iseg_amd import functional as F

    monkeypatch.delenv("ISEG_CONTRASTIVE_FUSED", raising=False)
    assert F.contrastive_fused()
    monkeypatch.setenv("ISEG_CONTRASTIVE_FUSED", "0")
    assert not F.contrastive_fused()
    monkeypatch.setenv("ISEG_CONTRASTIVE_FUSED", "1")
    assert F.contrastive_fused()


def test_the_plan_and_the_scratch_size_are_host_arithmetic():
    from iseg_amd import _hip
    from iseg_amd import kernels as K

    L = _hip.lib()
    # candidates: beam search's chunk plan over the OUTPUT rows
    for rows, V in ((1, 1), (1, 2048), (1, 256000), (16, 256000), (1000, 256000), (0, 100), (1, 0), (1, (1 << 20) + 1)):
        assert L.iseg_contrastive_candidates_splits(rows, V) == L.iseg_beam_select_splits(rows, V)
    assert K.contrastive_candidates_splits(1, 256000) == 62
    record = lambda k: 8 * (1 + k)      # noqa: E731  (the fp64 sum, then k packed pairs)
    tiles = -(-70001 // 2048)
    assert L.iseg_contrastive_candidates_scratch_bytes(6, 70001, 3, 2) == 6 * 2 * record(3)
    assert L.iseg_contrastive_candidates_scratch_bytes(6, 70001, 3, 10 ** 6) == 6 * tiles * record(3)
    assert L.iseg_contrastive_candidates_scratch_bytes(6, 70001, 3, 0) == 6 * L.iseg_contrastive_candidates_splits(6, 70001) * record(3)
    assert L.iseg_contrastive_candidates_scratch_bytes(6, 70001, 0, 1) == 0 and L.iseg_contrastive_candidates_scratch_bytes(6, 70001, 17, 1) == 0
    assert L.iseg_contrastive_candidates_scratch_bytes(6, 4, 5, 1) == 0      # k > V
    for dtype in (_hip.BF16, _hip.F32):
        assert L.iseg_contrastive_candidates_supported(1, 1, dtype) == 1 and L.iseg_contrastive_candidates_supported(1 << 20, 16, dtype) == 1
        assert L.iseg_contrastive_candidates_supported(0, 1, dtype) == 0 and L.iseg_contrastive_candidates_supported((1 << 20) + 1, 1, dtype) == 0
        assert L.iseg_contrastive_candidates_supported(100, 0, dtype) == 0 and L.iseg_contrastive_candidates_supported(100, 17, dtype) == 0
        assert L.iseg_contrastive_candidates_supported(4, 5, dtype) == 0 and L.iseg_contrastive_candidates_supported(5, 5, dtype) == 1
        assert L.iseg_contrastive_select_supported(8, 1, dtype) == 1 and L.iseg_contrastive_select_supported(16384, 16, dtype) == 1
        assert L.iseg_contrastive_select_supported(0, 1, dtype) == 0 and L.iseg_contrastive_select_supported(12, 1, dtype) == 0
        assert L.iseg_contrastive_select_supported(16392, 1, dtype) == 0
        assert L.iseg_contrastive_select_supported(64, 0, dtype) == 0 and L.iseg_contrastive_select_supported(64, 17, dtype) == 0
    assert L.iseg_contrastive_candidates_supported(100, 2, 2) == 0 and L.iseg_contrastive_select_supported(64, 2, 2) == 0
    assert K.contrastive_candidates_supported(100, 2, torch.bfloat16) and not K.contrastive_candidates_supported(100, 2, torch.float16)
    assert K.contrastive_select_supported(2048, 5, torch.bfloat16) and not K.contrastive_select_supported(2048, 5, torch.float16)
    # select: chunks of at least 16 positions, enough workgroups for two per CU of a 256-CU chip; one candidate group while k D elements fit 128 KB
    S = L.iseg_contrastive_select_splits
    assert S(1, 1, 2048, 5, _hip.BF16) == 1 and S(1, 31, 2048, 5, _hip.BF16) == 1 and S(1, 32, 2048, 5, _hip.BF16) == 2
    assert S(1, 4096, 2048, 5, _hip.BF16) == 256 and S(1, 100000, 2048, 5, _hip.BF16) == 512 and S(8, 100000, 2048, 5, _hip.BF16) == 64
    assert S(1000, 4096, 2048, 5, _hip.BF16) == 1
    assert S(1, 100000, 3072, 16, _hip.F32) == 256      # 16 * 3072 * 4 bytes = 192 KB: two groups of 8
    assert S(0, 10, 64, 2, _hip.BF16) == 0 and S(1, 0, 64, 2, _hip.BF16) == 0 and S(1, 10, 12, 2, _hip.BF16) == 0
    assert K.contrastive_select_splits(8, 100000, 2048, 5, torch.bfloat16) == 64
    Z = L.iseg_contrastive_select_scratch_bytes
    assert Z(3, 1000, 64, 5, 7, _hip.BF16) == 3 * 7 * 5 * 4
    assert Z(3, 10, 64, 5, 1000, _hip.BF16) == 3 * 10 * 5 * 4      # clipped to the filled positions
    assert Z(3, 1000, 64, 5, 0, _hip.BF16) == 3 * S(3, 1000, 64, 5, _hip.BF16) * 5 * 4
    assert Z(0, 10, 64, 5, 1, _hip.BF16) == 0 and Z(3, 0, 64, 5, 1, _hip.BF16) == 0 and Z(3, 10, 60, 5, 1, _hip.BF16) == 0


@pytest.mark.skipif(torch.cuda.is_available(), reason="passes host buffers to launchers: only where no kernel could ever receive them")
def test_the_launchers_refuse_before_touching_memory():
    from iseg_amd import _hip

    L = _hip.lib()
    ARG, UNSUPPORTED, WORKSPACE = -1, -3, -4
    buf = ctypes.create_string_buffer((1 << 16) + 64)
    a = (ctypes.addressof(buf) + 63) // 64 * 64
    need = L.iseg_contrastive_candidates_scratch_bytes(4, 100, 2, 0)
    assert 0 < need <= 1 << 15

    def candidates(ld=100, V=100, rows=4, k=2, T=1.0, dtype=_hip.BF16, ws_bytes=need, logits=a, row_map=None, group=1):
        return L.iseg_contrastive_candidates(logits, ld, row_map, group, a + 4096, a + 6144, a + (1 << 15), ws_bytes, rows, V, k, T, 0, dtype, None)

    for T in (0.0, -1.0, float("inf"), float("nan")):
        assert candidates(T=T) == ARG and "temperature" in _hip.last_error()
    assert candidates(ld=99) == ARG and "pitch" in _hip.last_error()
    assert candidates(row_map=a + 8192, group=0) == ARG and "group" in _hip.last_error()
    assert candidates(ws_bytes=need - 1) == WORKSPACE and str(need) in _hip.last_error()
    assert candidates(V=0) == UNSUPPORTED and candidates(V=(1 << 20) + 1, ld=1 << 21) == UNSUPPORTED
    assert candidates(k=0) == UNSUPPORTED and candidates(k=17) == UNSUPPORTED and candidates(dtype=2) == UNSUPPORTED
    assert candidates(V=3, k=4) == UNSUPPORTED and "min(16, V)" in _hip.last_error()
    assert candidates(logits=None) == ARG

    need = L.iseg_contrastive_select_scratch_bytes(2, 5, 64, 3, 0, _hip.BF16)
    assert 0 < need <= 1 << 12

    def select(hist=a, hs_b=8 * 64, hs_t=64, S=8, index=5, cand=a + 8192, ldc=64, D=64, k=3, alpha=0.5, dtype=_hip.BF16, ws_bytes=need, groups=2):
        return L.iseg_contrastive_select(hist, hs_b, hs_t, S, index, cand, ldc, a + 16384, a + 20480, a + 24576, a + 28672, a + (1 << 15), ws_bytes,
                                         groups, D, k, alpha, 0, dtype, None)

    assert select(D=60) == UNSUPPORTED and select(D=0) == UNSUPPORTED and select(k=0) == UNSUPPORTED and select(k=17) == UNSUPPORTED
    assert select(dtype=2) == UNSUPPORTED and "multiple of 8" in _hip.last_error()
    assert select(index=0) == ARG and select(index=9) == ARG and "index" in _hip.last_error()
    assert select(alpha=-0.1) == ARG and select(alpha=1.1) == ARG and select(alpha=float("nan")) == ARG and "alpha" in _hip.last_error()
    assert select(hs_t=56) == ARG and select(ldc=60) == ARG and select(hs_b=7 * 64) == ARG and select(hist=a + 8) == ARG and select(cand=a + 8196) == ARG
    assert select(ws_bytes=need - 1) == WORKSPACE and str(need) in _hip.last_error()
    assert select(hist=None) == ARG and select(groups=0) == ARG

    def commit(cache=a, planes=4, Sc=8, row_bytes=128, pos=3, prompt=a + 16384, S=8, ld=None, index=3, ids=_hip.IDS_I64, hist=a + 20480, hs_b=8 * 64,
               hs_t=64, Sh=8, cand=a + 24576, ldc=64, D=64, dtype=_hip.BF16, winner=a + 32768, groups=1, k=2):
        ld = S if ld is None else ld
        return L.iseg_contrastive_commit(cache, planes, Sc, row_bytes, pos, prompt, S, ld, index, ids, hist, hs_b, hs_t, Sh, cand, ldc, D, dtype, winner,
                                         groups, k, None)

    assert commit(k=0) == ARG and commit(k=17) == ARG and "k" in _hip.last_error()
    assert commit(row_bytes=24) == ARG and "16" in _hip.last_error()
    assert commit(cache=a + 8) == ARG
    assert commit(pos=8) == ARG and commit(pos=-1) == ARG and "cache of 8" in _hip.last_error()
    # the cache's positions are its own
    assert commit(Sc=4, S=12, pos=6, index=6, Sh=12, hs_b=12 * 64) == ARG and "cache of 4" in _hip.last_error()
    assert commit(Sc=12, S=8, pos=9, index=9) == ARG and "prompt of 8" in _hip.last_error()
    assert commit(index=8) == ARG and commit(index=-1) == ARG
    assert commit(prompt=None, index=8, pos=3) == ARG and "history of 8" in _hip.last_error()
    assert commit(ld=7) == ARG and "pitch" in _hip.last_error()
    assert commit(ids=2) == ARG and commit(winner=None) == ARG
    assert commit(D=4) == ARG and commit(hs_t=60) == ARG and commit(cand=None) == ARG and commit(dtype=2) == ARG


def test_the_documents_no_longer_list_contrastive_search_as_missing():
    for path in ("README.md", "INTEGRATION.md", "iseg_amd/nlp/samplers.py", "iseg_amd/nlp/gemma/gemma_causal.py"):
        text = open(os.path.join(ROOT, path)).read()
        assert "ContrastiveSampler" in text and "ISEG_CONTRASTIVE_FUSED" in text, path
        for line in text.splitlines():
            if "Out of scope" in line or "Not built" in line or "out of scope" in line:
                tail = line.split("Out of scope")[-1].split("Not built")[-1].split("out of scope")[-1]
                assert not re.search(r"[Cc]ontrastive", tail), (path, line)
