"""BeamSampler on the host: the composed route (plain torch) of iseg_amd.nlp.samplers.BeamSampler, F.beam_select and F.beam_reorder against the
fp64 oracle of tests/beam_search_ref.py on `next` functions small enough to check by hand, the refusals, the configuration round trip, what
GemmaCausalLM accepts, and the host arithmetic and refusals of the C entry points.  No GPU: CPU tensors take the composed route."""
import ctypes
import itertools
import math
import os
import re

import pytest
import torch

from tests import beam_search_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, B_, C_ = 1, 2, 3      # tokens of the hand-made model


def _markov(table):
    """next whose logits depend on the previous token alone, row table[prompt[:, index - 1]], or with a [S, V, V] table on the position too
    (two orders of the same transitions then score differently: no exact ties between hypotheses); records the indices it was asked for"""
    seen = []

    def next(prompt, cache, index):
        seen.append(index)
        rows = table if table.dim() == 2 else table[index]
        return rows[prompt[:, index - 1].long()].clone(), None, cache

    return next, seen


def _hand_table():
    """6 tokens.  After the start token 0: A has p = 0.5, B 0.4, the rest 0.1 together.  After A a flat row (1/6 each); after B token C has 0.9.
    Greedy takes A and ends with 0.5 / 6 = 0.083; the best two-token continuation is B C with 0.36."""
    p = torch.full((6, 6), 1.0 / 6.0, dtype=torch.float64)
    p[0] = torch.tensor([0.025, 0.5, 0.4, 0.025, 0.025, 0.025])
    p[B_] = torch.tensor([0.02, 0.02, 0.02, 0.9, 0.02, 0.02])
    return torch.log(p).float()


def _random_table(V, seed, S=None):
    return 3.0 * torch.randn(*((V, V) if S is None else (S, V, V)), generator=torch.Generator().manual_seed(seed))


def test_beam_finds_the_sequence_that_greedy_misses():
    from iseg_amd.nlp.gemma.gemma_causal import greedy_sample
    from iseg_amd.nlp.samplers import BeamSampler

    table = _hand_table()
    prompt = torch.zeros(1, 3, dtype=torch.int64)
    mask = torch.tensor([[True, False, False]])
    nxt, _ = _markov(table)
    greedy = greedy_sample(nxt, prompt, None, 1, mask)
    assert greedy[0, 1].item() == A
    beam = BeamSampler(num_beams=2)(nxt, prompt, None, 1, mask)
    assert beam.tolist() == [[0, B_, C_]] and tuple(beam.shape) == (1, 3) and beam.dtype == prompt.dtype
    assert prompt.tolist() == [[0, 0, 0]]      # the caller's prompt is not written
    # the true best of all 36 continuations
    logp = torch.log_softmax(table.double(), dim=-1)
    best = max(itertools.product(range(6), repeat=2), key=lambda s: (logp[0, s[0]] + logp[s[0], s[1]]).item())
    assert list(best) == [B_, C_]
    prompts, scores = BeamSampler(num_beams=2, return_all_beams=True)(nxt, prompt, None, 1, mask)
    assert tuple(prompts.shape) == (1, 2, 3) and tuple(scores.shape) == (1, 2) and scores.dtype == torch.float32
    assert prompts[0, 0].tolist() == [0, B_, C_] and abs(scores[0, 0].item() - math.log(0.36)) < 1e-5
    assert prompts[0, 1, 1].item() == A and abs(scores[0, 1].item() - math.log(0.5 / 6)) < 1e-5


def test_one_beam_is_greedy():
    from iseg_amd.nlp.gemma.gemma_causal import greedy_sample
    from iseg_amd.nlp.samplers import BeamSampler

    V = 23
    table = _random_table(V, 1)      # continuous values: no ties
    prompt = torch.randint(0, V, (3, 9), generator=torch.Generator().manual_seed(2))
    mask = torch.zeros(3, 9, dtype=torch.bool)
    for b, n in enumerate((2, 4, 3)):
        mask[b, :n] = True
    for end in (None, 5):
        nxt, seen = _markov(table)
        want = greedy_sample(nxt, prompt, None, 2, mask, end_token_id=end)
        asked = list(seen)
        del seen[:]
        got = BeamSampler(num_beams=1, temperature=0.5)(nxt, prompt, None, 2, mask, end_token_id=end)
        assert torch.equal(got, want) and seen == asked


def test_the_first_step_extends_beam_zero_alone():
    """all beams hold the same prompt at the first step: without the -1e9 start the best token would be chosen num_beams times"""
    from iseg_amd.nlp.samplers import BeamSampler

    V, nb = 11, 4
    table = _random_table(V, 3)
    prompt = torch.tensor([[7, 0], [2, 0]])
    nxt, seen = _markov(table)
    prompts, scores = BeamSampler(num_beams=nb, return_all_beams=True)(nxt, prompt, None, 1)
    assert seen == [1]
    logp = torch.log_softmax(table.double(), dim=-1)
    for b, first in enumerate((7, 2)):
        top = torch.topk(logp[first], nb)
        assert prompts[b, :, 1].tolist() == top.indices.tolist() and prompts[b, :, 0].tolist() == [first] * nb
        assert torch.allclose(scores[b].double(), top.values, atol=1e-5)


@pytest.mark.parametrize("nb", [2, 5])
@pytest.mark.parametrize("T", [1.0, 0.5])
def test_the_loop_against_the_oracle_with_user_tokens_on_the_longer_rows(nb, T):
    """rows of 2, 5 and 3 user tokens, generation starts at 2: the longer rows keep their tokens, and the running score still takes the selected
    candidate's value there (the reference's behaviour) -- the oracle loop does the same, literally"""
    from iseg_amd.nlp.samplers import BeamSampler

    V, S = 13, 8
    table = _random_table(V, 5, S)
    prompt = torch.randint(0, V, (3, S), generator=torch.Generator().manual_seed(6))
    mask = torch.zeros(3, S, dtype=torch.bool)
    for b, n in enumerate((2, 5, 3)):
        mask[b, :n] = True
    nxt, seen = _markov(table)
    want_prompts, want_scores, asked = R.beam_loop(_markov(table)[0], prompt, mask, 2, nb, T)
    prompts, scores = BeamSampler(num_beams=nb, return_all_beams=True, temperature=T)(nxt, prompt, None, 2, mask)
    assert seen == asked == list(range(2, S))
    assert torch.equal(prompts, want_prompts)
    assert torch.allclose(scores.double(), want_scores, rtol=1e-5, atol=1e-5)
    assert all(torch.equal(prompts[b, j][mask[b]], prompt[b][mask[b]]) for b in range(3) for j in range(nb))      # user tokens are kept
    # the score of row 1 moved at the positions its user tokens fill: it is the sum of the SELECTED candidates' log-probabilities
    logp = torch.log_softmax(table.double() / T, dim=-1)
    own = sum(logp[i, prompts[1, 0, i - 1], prompts[1, 0, i]].item() for i in range(5, S))
    assert scores[1, 0].item() < own - 1e-3
    best = BeamSampler(num_beams=nb, temperature=T)(_markov(table)[0], prompt, None, 2, mask)
    assert torch.equal(best, want_prompts[:, 0])


def test_the_loop_stops_when_every_beam_row_holds_an_end_token():
    from iseg_amd.nlp.samplers import BeamSampler

    V, S, nb, end = 9, 12, 3, 4
    table = _random_table(V, 8, S)
    table[:, :, end] += 2.0      # likely, not certain
    prompt = torch.randint(0, V, (2, S), generator=torch.Generator().manual_seed(9))
    prompt[prompt == end] = 0
    mask = torch.zeros(2, S, dtype=torch.bool)
    mask[:, :2] = True
    want_prompts, want_scores, asked = R.beam_loop(_markov(table)[0], prompt, mask, 2, nb, 1.0, end_token_id=end)
    assert 1 <= len(asked) < S - 2      # the case means something: the loop runs and stops early
    nxt, seen = _markov(table)
    prompts, scores = BeamSampler(num_beams=nb, return_all_beams=True)(nxt, prompt, None, 2, mask, end_token_id=end)
    assert seen == asked and torch.equal(prompts, want_prompts)
    stop = asked[-1] + 1
    assert bool((prompts[:, :, :stop] == end).any(dim=-1).all())                       # every one of the B nb rows holds one
    before = R.beam_loop(_markov(table)[0], prompt[:, :stop - 1], mask[:, :stop - 1], 2, nb, 1.0, end_token_id=end)[0]
    assert not bool((before == end).any(dim=-1).all())                                 # and one step earlier some row did not
    assert torch.equal(prompts[:, :, stop:], prompt[:, None, stop:].expand(-1, nb, -1))      # nothing is written after the stop


def test_all_beams_come_back_sorted():
    from iseg_amd.nlp.samplers import BeamSampler

    V = 17
    table = _random_table(V, 10, 7)
    prompt = torch.randint(0, V, (4, 7), generator=torch.Generator().manual_seed(11))
    prompts, scores = BeamSampler(num_beams=5, return_all_beams=True)(_markov(table)[0], prompt, None, 1)
    assert bool((scores[:, 1:] <= scores[:, :-1]).all())
    best = BeamSampler(num_beams=5)(_markov(table)[0], prompt, None, 1)
    assert torch.equal(best, prompts[:, 0])
    logp = torch.log_softmax(table.double(), dim=-1)
    for b in range(4):
        for j in range(5):
            seq = prompts[b, j]
            assert abs(sum(logp[i, seq[i - 1], seq[i]].item() for i in range(1, 7)) - scores[b, j].item()) < 1e-4


def test_select_composed_pins_the_order_down():
    """ties by flat index, NaN above everything, -inf candidates last, on the route the host runs"""
    from iseg_amd import functional as F

    nb, V = 3, 5
    logits = torch.zeros(2 * nb, V)
    lp = torch.zeros(2 * nb)
    lp[3:] = torch.tensor([-1.0, 0.0, -1.0])
    logits[4, 2] = 1.0
    parents, tokens, scores = F.beam_select(logits, lp, nb)
    assert parents.dtype == tokens.dtype == torch.int32 and scores.dtype == torch.float32
    assert parents[:3].tolist() == [0, 0, 0] and tokens[:3].tolist() == [0, 1, 2]      # eighteen equal candidates: the first three
    assert parents[3:].tolist() == [1, 1, 1] and tokens[3:].tolist() == [2, 0, 1]
    assert not R.accepted(parents, tokens, scores, logits, lp, nb, 1.0, 4.0)
    logits[1, 3] = float("nan")
    logits[0, :] = -float("inf")
    logits[0, 4] = 0.0
    parents, tokens, scores = F.beam_select(logits, lp, nb)
    assert parents[:3].tolist() == [1, 1, 1] and tokens[:3].tolist() == [0, 1, 2] and bool(torch.isnan(scores[:3]).all())
    assert not R.in_range_and_distinct(parents, tokens, nb, V)
    lp[1] = -float("inf")
    logits[1, 3] = 0.0
    parents, tokens, scores = F.beam_select(logits, lp, nb)
    assert (parents[0].item(), tokens[0].item(), scores[0].item()) == (0, 4, 0.0)
    assert not R.accepted(parents, tokens, scores, logits, lp, nb, 1.0, 4.0)


@pytest.mark.parametrize("T", [0.25, 1.0, 4.0])
def test_select_composed_against_the_oracle(T):
    from iseg_amd import functional as F

    gen = torch.Generator().manual_seed(int(T * 4))
    for nb, Bn, V in ((1, 3, 7), (2, 1, 257), (5, 3, 65), (16, 2, 33)):
        logits = 2.0 * torch.randn(Bn * nb, V, generator=gen)
        logits[0, torch.rand(V, generator=gen) < 0.3] = -float("inf")
        logits[0, 0] = 0.5
        lp = -50.0 * torch.rand(Bn * nb, generator=gen)
        got = F.beam_select(logits[:, None, :], lp, nb, temperature=T)
        # the yardstick itself is fp32 torch: x / T, log_softmax (max, exp, a sum over V terms, log) and one add, 16 * 2^-23 max(1, |score|) at most
        assert not R.accepted(*got, logits, lp, nb, T, 16.0), R.accepted(*got, logits, lp, nb, T, 16.0)


def test_reorder_composed_is_the_statement():
    from iseg_amd import functional as F

    nb, Bn, S = 3, 2, 6
    gen = torch.Generator().manual_seed(12)
    cache = torch.randn(Bn * nb, 2, 2, S, 1, 8, generator=gen)
    prompt = torch.randint(0, 99, (Bn * nb, S), generator=gen)
    mask = torch.zeros(Bn * nb, S, dtype=torch.bool)
    mask[3:, 4] = True
    parents = torch.tensor([2, 2, 0, 1, 0, 1], dtype=torch.int32)
    tokens = torch.tensor([50, 51, 52, 53, 54, 55], dtype=torch.int32)
    new_cache, new_prompt = F.beam_reorder(cache, prompt, mask, parents, tokens, 4, nb)
    rows = [2, 2, 0, 4, 3, 4]
    assert torch.equal(new_cache, cache[rows]) and new_cache.data_ptr() != cache.data_ptr()
    want = prompt[rows].clone()
    want[:3, 4] = tokens[:3]
    assert torch.equal(new_prompt, want)
    none_cache, again = F.beam_reorder(None, prompt, mask, parents, tokens, 4, nb)
    assert none_cache is None and torch.equal(again, want)


def test_refusals_name_the_argument():
    from iseg_amd import functional as F
    from iseg_amd.nlp.samplers import BeamSampler

    for kw in ({"num_beams": 0}, {"num_beams": 17}, {"num_beams": 2.0}, {"num_beams": True}, {"num_beams": -3}):
        with pytest.raises(ValueError, match="num_beams"):
            BeamSampler(**kw)
    with pytest.raises(ValueError, match="return_all_beams"):
        BeamSampler(return_all_beams=1)
    for T in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="temperature"):
            BeamSampler(temperature=T)
    with pytest.raises(NotImplementedError, match="running scores"):
        BeamSampler().get_next_token(torch.zeros(2, 5))
    with pytest.raises(ValueError, match=r"\[B, S\]"):
        BeamSampler()(lambda *a: None, torch.zeros(3, dtype=torch.int64))
    x, lp = torch.zeros(4, 10), torch.zeros(4)
    for args, word in (((x, lp, 3), "num_beams|rows|B \\*"), ((x, lp, 0), "num_beams"), ((x, lp, 17), "num_beams"), ((x, torch.zeros(3), 2), "log_probs"),
                       ((x, lp.double(), 2), "float32"), ((x.long(), lp, 2), "floating")):
        with pytest.raises(ValueError, match=word):
            F.beam_select(*args)
    with pytest.raises(ValueError, match="temperature"):
        F.beam_select(x, lp, 2, temperature=0.0)
    with pytest.raises(RuntimeError, match="inference only"):
        F.beam_select(x.clone().requires_grad_(), lp, 2)
    prompt, mask, ids = torch.zeros(4, 5, dtype=torch.int64), torch.zeros(4, 5, dtype=torch.bool), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="position"):
        F.beam_reorder(None, prompt, mask, ids, ids, 5, 2)
    with pytest.raises(ValueError, match="parents"):
        F.beam_reorder(None, prompt, mask, ids.long(), ids, 1, 2)
    with pytest.raises(ValueError, match="groups"):
        F.beam_reorder(None, prompt, mask, ids, ids, 1, 3)
    with pytest.raises(ValueError, match="cache"):
        F.beam_reorder(torch.zeros(4, 2, 5), prompt, mask, ids, ids, 1, 2)


def test_dry_run_shapes():
    from iseg_amd import functional as F
    from iseg_amd import nn

    with nn.dry_run_scope():
        out = F.beam_select(torch.zeros(6, 1, 50), torch.zeros(6), 3)
    assert [tuple(t.shape) for t in out] == [(6,)] * 3 and [t.dtype for t in out] == [torch.int32, torch.int32, torch.float32]


def test_config_round_trip():
    from iseg_amd.nlp.samplers import BeamSampler

    s = BeamSampler()
    assert s.get_config() == {"temperature": 1.0, "num_beams": 5, "return_all_beams": False}      # keras_nlp's defaults
    s = BeamSampler(num_beams=3, return_all_beams=True, temperature=0.7)
    t = BeamSampler.from_config(s.get_config())
    assert type(t) is BeamSampler and t.get_config() == s.get_config() == {"temperature": 0.7, "num_beams": 3, "return_all_beams": True}


def test_what_the_model_accepts():
    from iseg_amd.nlp.gemma import GemmaBackbone, GemmaCausalLM
    from iseg_amd.nlp.samplers import BeamSampler
    from tests.test_gemma_host import TINY

    model = GemmaCausalLM(GemmaBackbone(**TINY))
    sampler = BeamSampler(num_beams=2)
    model.compile(sampler=sampler)
    assert model.sampler is sampler
    model.compile(sampler=sampler, graph_decode=True)
    assert model._graph_decode_sampler() == (False, sampler)      # a beam step keeps the eager loop
    with pytest.raises(NotImplementedError, match="BeamSampler"):
        model.compile(sampler="beam")
    assert model.sampler is sampler
    model.compile(sampler=BeamSampler(num_beams=2, return_all_beams=True))
    inputs = {"token_ids": torch.zeros(1, 4, dtype=torch.int64), "padding_mask": torch.ones(1, 4, dtype=torch.bool)}
    with pytest.raises(ValueError, match="call the sampler directly"):
        model.generate_step(inputs)


def test_the_symbols_are_declared_exported_and_bound():
    from iseg_amd import _hip
    from iseg_amd import functional as F
    from iseg_amd import kernels as K
    from iseg_amd import build
    from iseg_amd.nlp import samplers

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "iseg_hip.h")).read(), flags=re.S)
    names = ("iseg_beam_select_supported", "iseg_beam_select_splits", "iseg_beam_select_scratch_bytes", "iseg_beam_select", "iseg_beam_reorder")
    if not os.path.exists(_hip.LIB_PATH):
        build.build(verbose=False)
    dll = ctypes.CDLL(_hip.LIB_PATH)
    for name in names:
        assert re.search(r"\b(?:int|size_t)\s+%s\s*\(" % name, header), name
        assert name in _hip.SIGNATURES and hasattr(dll, name), name
    assert "beam_search.hip" in build.SOURCES
    for mod, fns in ((K, ("beam_select", "beam_select_supported", "beam_select_splits", "beam_reorder")), (F, ("beam_select", "beam_reorder", "beam_fused"))):
        for fn in fns:
            assert callable(getattr(mod, fn)), fn
    assert issubclass(samplers.BeamSampler, samplers.Sampler)
    with pytest.raises(_hip.HipCallError):      # no CPU route below F
        K.beam_select(torch.zeros(2, 4), torch.zeros(2), 2, 1.0)


def test_the_plan_and_the_scratch_size_are_host_arithmetic():
    from iseg_amd import _hip
    from iseg_amd import kernels as K

    L = _hip.lib()
    assert L.iseg_beam_select_splits(1, 1) == 1 and L.iseg_beam_select_splits(1, 2048) == 1 and L.iseg_beam_select_splits(1, 256000) == 62
    assert L.iseg_beam_select_splits(16, 256000) == 32 and L.iseg_beam_select_splits(1000, 256000) == 1
    assert L.iseg_beam_select_splits(0, 100) == 0 and L.iseg_beam_select_splits(1, 0) == 0 and L.iseg_beam_select_splits(1, (1 << 20) + 1) == 0
    assert K.beam_select_splits(16, 256000) == 32
    record = lambda nb: 8 * (1 + nb)      # noqa: E731  (the fp64 sum, then nb packed pairs)
    tiles = -(-70001 // 2048)
    assert L.iseg_beam_select_scratch_bytes(6, 70001, 3, 2) == 6 * 2 * record(3)
    assert L.iseg_beam_select_scratch_bytes(6, 70001, 3, 10 ** 6) == 6 * tiles * record(3)      # clipped to the tiles that hold an element
    assert L.iseg_beam_select_scratch_bytes(6, 70001, 3, 0) == 6 * L.iseg_beam_select_splits(6, 70001) * record(3)
    assert L.iseg_beam_select_scratch_bytes(16, 5, 16, 0) == 16 * record(16)
    assert L.iseg_beam_select_scratch_bytes(6, 70001, 0, 1) == 0 and L.iseg_beam_select_scratch_bytes(6, 70001, 17, 1) == 0
    for dtype in (_hip.BF16, _hip.F32):
        assert L.iseg_beam_select_supported(1, 1, dtype) == 1 and L.iseg_beam_select_supported(1 << 20, 16, dtype) == 1
        assert L.iseg_beam_select_supported(0, 1, dtype) == 0 and L.iseg_beam_select_supported((1 << 20) + 1, 1, dtype) == 0
        assert L.iseg_beam_select_supported(100, 0, dtype) == 0 and L.iseg_beam_select_supported(100, 17, dtype) == 0
    assert L.iseg_beam_select_supported(100, 2, 2) == 0
    assert K.beam_select_supported(100, 2, torch.bfloat16) and not K.beam_select_supported(100, 2, torch.float16)


@pytest.mark.skipif(torch.cuda.is_available(), reason="passes host buffers to launchers: only where no kernel could ever receive them")
def test_the_launchers_refuse_before_touching_memory():
    from iseg_amd import _hip

    L = _hip.lib()
    ARG, UNSUPPORTED, WORKSPACE = -1, -3, -4
    buf = ctypes.create_string_buffer((1 << 16) + 64)
    a = (ctypes.addressof(buf) + 63) // 64 * 64
    need = L.iseg_beam_select_scratch_bytes(4, 100, 2, 0)
    assert 0 < need <= 1 << 15

    def select(ld=100, V=100, rows=4, nb=2, T=1.0, dtype=_hip.BF16, ws_bytes=need, logits=a):
        return L.iseg_beam_select(logits, ld, a + 2048, a + 4096, a + 6144, a + 8192, a + (1 << 15), ws_bytes, rows, V, nb, T, 0, dtype, None)

    for T in (0.0, -1.0, float("inf"), float("nan")):
        assert select(T=T) == ARG and "temperature" in _hip.last_error()
    assert select(ld=99) == ARG and "pitch" in _hip.last_error()
    assert select(rows=5) == ARG and "groups" in _hip.last_error()
    assert select(ws_bytes=need - 1) == WORKSPACE and str(need) in _hip.last_error()
    assert select(V=0) == UNSUPPORTED and select(V=(1 << 20) + 1, ld=1 << 21) == UNSUPPORTED
    assert select(nb=0) == UNSUPPORTED and select(nb=17, rows=17) == UNSUPPORTED and select(dtype=2) == UNSUPPORTED
    assert select(logits=None) == ARG

    def reorder(cache=a, planes=4, Sc=8, row_bytes=128, length=3, prompt=a + 16384, S=8, ld=None, index=3, ids=_hip.IDS_I64, parents=a + 32768, groups=1,
                nb=2):
        ld = S if ld is None else ld
        return L.iseg_beam_reorder(cache, planes, Sc, row_bytes, length, prompt, S, ld, a + 20480, ld, a + 24576, index, ids, parents, groups, nb, None)

    assert reorder(nb=0) == ARG and reorder(nb=17) == ARG and "nb" in _hip.last_error()
    assert reorder(row_bytes=24) == ARG and "16" in _hip.last_error()
    assert reorder(cache=a + 8) == ARG
    assert reorder(length=9) == ARG and reorder(length=-1) == ARG and "filled" in _hip.last_error()
    # the cache's positions are its own: a prompt of 12 does not make room for 6 filled positions in a cache of 4, nor does a cache of 12
    # make position 9 lie inside a prompt of 8
    assert reorder(Sc=4, S=12, length=6) == ARG and "cache of 4" in _hip.last_error()
    assert reorder(Sc=12, S=8, length=10, index=9) == ARG and "prompt of 8" in _hip.last_error()
    assert reorder(Sc=0, length=0) == ARG and reorder(S=0, index=0) == ARG
    assert reorder(index=8) == ARG and reorder(index=-1) == ARG and "position" in _hip.last_error()
    assert reorder(ld=7) == ARG and "pitch" in _hip.last_error()
    assert reorder(ids=2) == ARG and reorder(parents=None) == ARG


def test_reorder_with_a_cache_longer_or_shorter_than_the_prompt_and_with_expanded_rows():
    """the cache's position axis is its own (a cache allocated to a maximum length): the statement holds for Sc != S; so it does for a mask
    that is one row expanded over the beams; K.beam_reorder, the layer below, refuses what the kernels cannot take"""
    from iseg_amd import _hip
    from iseg_amd import functional as F
    from iseg_amd import kernels as K

    nb, S = 2, 6
    gen = torch.Generator().manual_seed(13)
    prompt = torch.randint(0, 99, (2 * nb, S), generator=gen)
    parents = torch.tensor([1, 1, 0, 0], dtype=torch.int32)
    tokens = torch.tensor([50, 51, 52, 53], dtype=torch.int32)
    rows = [1, 1, 2, 2]
    for Sc in (4, 9):
        cache = torch.randn(2 * nb, 2, 2, Sc, 1, 8, generator=gen)
        mask = torch.zeros(1, S, dtype=torch.bool).expand(2 * nb, S)
        new_cache, new_prompt = F.beam_reorder(cache, prompt, mask, parents, tokens, 3, nb)
        want = prompt[rows].clone()
        want[:, 3] = tokens.long()
        assert torch.equal(new_cache, cache[rows]) and torch.equal(new_prompt, want)
        with pytest.raises(ValueError, match="filled"):
            F.beam_reorder(cache, prompt, mask, parents, tokens, 5, nb, length=Sc + 1)
    with pytest.raises(_hip.HipCallError):      # host tensors
        K.beam_reorder(None, 0, prompt, torch.zeros(2 * nb, S, dtype=torch.bool), tokens, 3, parents, nb)


def test_the_documents_no_longer_list_beam_search_as_missing():
    for path in ("README.md", "INTEGRATION.md", "iseg_amd/nlp/samplers.py", "iseg_amd/nlp/gemma/gemma_causal.py"):
        text = open(os.path.join(ROOT, path)).read()
        assert "BeamSampler" in text and "ISEG_BEAM_FUSED" in text, path
        for line in text.splitlines():
            if "Out of scope" in line or "Not built" in line:
                assert not re.search(r"\bbeam\b|BeamSampler", line.split("Out of scope")[-1].split("Not built")[-1]), (path, line)
