"""The beam-search kernels on the GPU (csrc/beam_search.hip through F.beam_select, F.beam_reorder and iseg_amd.nlp.samplers.BeamSampler) against
the fp64 oracle of tests/beam_search_ref.py, and beam search through GemmaCausalLM.

The selection must pass R.accepted with eps = C 2^-23 max(1, |score|), C = 3.  The derivation (inputs are exact: the oracle reads the stored
values):  the kernel forms the exponent (x - m) log2(e) / T in fp64 (2^-53, nothing) and splits it into an fp32 head and tail; v_exp_f32 on
the head costs one ulp, at most 2^-23 of the weight; the tail's fma and the product 2^-24 each: a weight is off by at most 2 * 2^-23 of
itself, and so is their sum, which is formed in fp64 in a fixed order (2^-53 per addition over <= 2^20 terms: nothing), as are the merge of
the chunk sums (exp2 in fp64), the logarithm, the division by T and the additions of the score; log S moves by at most 2 * 2^-23.  The score
is rounded to fp32 once: 2^-24 |score|.  Together 2 * 2^-23 + 2^-24 |score| <= 2.5 * 2^-23 max(1, |score|); C = 3 is that, rounded up.  Every
case prints its worst figure."""
import numpy as np
import pytest
import torch

from tests import beam_search_ref as R
from tests import guarded_memory as GM
from tests.test_gemma_cache_gpu import B as MB
from tests.test_gemma_cache_gpu import PROMPTS, S as MS
from tests.test_gemma_cache_gpu import _model, _prompts, bf16  # noqa: F401  (bf16 is a fixture)
from tests.test_token_sample_gpu import _ld, _pitched, _rows

pytestmark = pytest.mark.gpu

C_UNITS = 3.0
TILE = 2048
VS = [1, 2, 63, 64, 65, 257, 2047, 2048, 2049, 4099, 70001]
NBS = [1, 2, 5, 8, 16]
BS = [1, 3]
TS = [0.25, 1.0, 4.0]
LP_KINDS = ["initial", "random", "equal", "one_inf"]
PITCHES = ["tight", "plus24", "aligned"]


def _log_probs(kind, Bn, nb, gen):
    if kind == "initial":
        return torch.tensor([0.0] + [-1e9] * (nb - 1)).repeat(Bn)
    if kind == "equal":      # ties between the beams wherever the rows tie
        return torch.full((Bn * nb,), -3.5)
    lp = -2000.0 * torch.rand(Bn * nb, generator=gen)
    if kind == "one_inf":
        lp[torch.arange(Bn) * nb + torch.randint(0, nb, (Bn,), generator=gen)] = -float("inf")
    return lp


def _same_bits(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("V", VS)
def test_select_against_the_oracle(cuda, V, dtype):
    """every num_beams at this V and dtype; the batch size, the temperature, the kind of running scores, the forced chunk count (0: the plan; 1;
    2; 3; one chunk per tile -- borders fall inside every V above one tile), the row pitch (padding columns hold NaN) and the first row's logit
    family rotate with num_beams and the case, so that over the cases every value meets every V.  Rows of a batch are of successive families
    (gaussian, four levels with heavy ties, one far above, a third masked).  A second call returns the same bits."""
    from iseg_amd import functional as F

    case = VS.index(V) * 2 + (dtype == torch.float32)
    gen = torch.Generator().manual_seed(2000 + case)
    tiles = -(-V // TILE)
    worst = 0.0
    for i, nb in enumerate(NBS):
        for rep in range(2):
            j = 2 * i + rep + case
            Bn, T, kind = BS[j % 2], TS[(j // 2) % 3], LP_KINDS[(j // 3) % 4]
            splits, pitch = [0, 1, 2, tiles, 3][j % 5], PITCHES[(j // 5) % 3]
            x = _rows(Bn * nb, V, dtype, gen, j % 4)
            lp = _log_probs(kind, Bn, nb, gen)
            xd, lpd = _pitched(x, _ld(V, pitch), cuda), lp.to(cuda)
            got = F.beam_select(xd, lpd, nb, temperature=T, splits=splits)
            note = (V, nb, Bn, T, kind, splits, pitch)
            assert [t.dtype for t in got] == [torch.int32, torch.int32, torch.float32] and all(tuple(t.shape) == (Bn * nb,) for t in got), note
            worst = max(worst, R.worst_units(got[2], got[0], got[1], x, lp, nb, T))
            bad = R.accepted(*got, x, lp, nb, T, C_UNITS)
            assert not bad, (note, bad[:3])
            assert _same_bits(got, F.beam_select(xd, lpd, nb, temperature=T, splits=splits)), note
    print(f"V {V} {dtype}: worst score error {worst:.2f} units of 2^-23 max(1, |score|)")
    assert worst <= C_UNITS


def test_a_quarter_million_entries(cuda):
    """V = 256000, bf16, Gemma's head: the chunk plan, one chunk and the most chunks, four and sixteen beams"""
    from iseg_amd import functional as F
    from iseg_amd import kernels as K

    V, gen = 256000, torch.Generator().manual_seed(5)
    assert K.beam_select_splits(4, V) > 1
    for nb, Bn, T, splits, kind in ((4, 1, 1.0, 0, "random"), (16, 1, 0.25, 1, "equal"), (2, 2, 4.0, V // TILE, "initial")):
        x = _rows(Bn * nb, V, torch.bfloat16, gen, 0)
        lp = _log_probs(kind, Bn, nb, gen)
        got = F.beam_select(x.to(cuda), lp.to(cuda), nb, temperature=T, splits=splits)
        print(f"nb {nb} splits {splits}: worst {R.worst_units(got[2], got[0], got[1], x, lp, nb, T):.2f} units")
        bad = R.accepted(*got, x, lp, nb, T, C_UNITS)
        assert not bad, (nb, splits, bad[:3])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_select_with_non_finite_rows(cuda, dtype):
    """a NaN logit in one beam row and a row of -inf alone, beside ordinary rows: the pairs are in range and distinct (and the call returns);
    such a row's candidates are its first tokens with NaN scores, in front of every number; the groups without one pass the oracle"""
    from iseg_amd import functional as F

    nan, inf = float("nan"), float("inf")
    for V, nb, splits in ((1, 2, 0), (3, 5, 0), (65, 5, 0), (4099, 8, 3), (70001, 16, 0)):
        gen = torch.Generator().manual_seed(V)
        x = _rows(3 * nb, V, dtype, gen, 0).float()
        x[0, (2 * V) // 3] = nan                 # group 0: beam 0 holds a NaN
        x[nb + nb - 1, :] = -inf                 # group 1: its last beam is masked altogether
        x = x.to(dtype)
        lp = _log_probs("random", 3, nb, gen)
        parents, tokens, scores = F.beam_select(x.to(cuda), lp.to(cuda), nb, splits=splits)
        assert not R.in_range_and_distinct(parents, tokens, nb, V), (V, nb)
        k = min(nb, V)
        assert parents[:k].tolist() == [0] * k and tokens[:k].tolist() == list(range(k)) and bool(torch.isnan(scores[:k]).all())
        assert parents[nb:nb + k].tolist() == [nb - 1] * k and tokens[nb:nb + k].tolist() == list(range(k)) and bool(torch.isnan(scores[nb:nb + k]).all())
        assert not bool(torch.isnan(scores[k:nb]).any()) and not bool(torch.isnan(scores[2 * nb:]).any())
        bad = R.accepted(parents[2 * nb:], tokens[2 * nb:], scores[2 * nb:], x[2 * nb:], lp[2 * nb:], nb, 1.0, C_UNITS)
        assert not bad, (V, nb, bad[:3])


def test_the_three_dimensional_view_and_the_route_switch(cuda, monkeypatch):
    """[B nb, 1, V] as call_with_cache's logits sliced out of [B nb, Tn, V]: the pitch is the view's.  ISEG_BEAM_FUSED=0 takes the composed
    route on the same device tensors; on tie-free rows both select the same pairs"""
    from iseg_amd import functional as F

    gen = torch.Generator().manual_seed(9)
    x = (2.0 * torch.randn(6, 257, generator=gen)).to(torch.bfloat16).float() + 1e-3 * torch.rand(6, 257, generator=gen)
    lp = -5.0 * torch.rand(6, generator=gen)      # small scores: one fp32 ulp is far below the gaps between candidates
    full = torch.full((6, 2, 257), float("nan"), dtype=torch.float32, device=cuda)
    full[:, 1] = x.to(cuda)
    got = F.beam_select(full[:, 1:2], lp.to(cuda), 3)
    assert not R.accepted(*got, x, lp, 3, 1.0, C_UNITS)
    assert _same_bits(got, F.beam_select(x.to(cuda), lp.to(cuda), 3))
    monkeypatch.setenv("ISEG_BEAM_FUSED", "0")
    assert not F.beam_fused()
    composed = F.beam_select(x.to(cuda), lp.to(cuda), 3)
    assert torch.equal(composed[0], got[0]) and torch.equal(composed[1], got[1])
    assert not R.accepted(*composed, x, lp, 3, 1.0, 16.0)


def test_select_inside_guard_bands(cuda):
    """logits, running scores, the three outputs and a scratch buffer of EXACTLY iseg_beam_select_scratch_bytes between bands of poison
    (tests/guarded_memory.py): the bands are intact after the call, the scratch buffer was asked for, and the results are the unguarded call's"""
    from iseg_amd import kernels as K

    for Bn, nb, V, dtype, splits in ((1, 5, 4099, torch.bfloat16, 0), (2, 16, 70001, torch.bfloat16, 0), (3, 1, 257, torch.float32, 0),
                                     (1, 8, 70001, torch.float32, 35), (2, 2, 4104, torch.bfloat16, 2)):
        gen = torch.Generator().manual_seed(V + nb)
        x = _rows(Bn * nb, V, dtype, gen, 0)
        lp = _log_probs("random", Bn, nb, gen)
        plain = K.beam_select(x.to(cuda), lp.to(cuda), nb, 1.0, splits)
        arena = GM.Arena(cuda, 32 << 20)
        with GM.guarded(arena):
            xd = arena.alloc(x.shape, x.dtype, "operand")
            ld = arena.alloc(lp.shape, lp.dtype, "operand")
            xd.copy_(x)
            ld.copy_(lp)
            got = K.beam_select(xd, ld, nb, 1.0, splits)
            arena.check()
            roles = [r.role for r in arena.records]
            assert roles.count("workspace") == 1 and roles.count("output") == 3
            ws = [r for r in arena.records if r.role == "workspace"][0]
            assert ws.end - ws.start == K._hip.lib().iseg_beam_select_scratch_bytes(Bn * nb, V, nb, splits) > 0
            assert all(0 <= arena.offset_of(t) < arena.nbytes for t in got)
        assert _same_bits([t.cpu() for t in got], [t.cpu() for t in plain])
        assert not R.accepted(*got, x, lp, nb, 1.0, C_UNITS)


# ---- reorder ---------------------------------------------------------------------------------------------------------------------------------
MAPPINGS = ["identity", "all_from_one", "cyclic", "swap", "random"]


def _mapping(kind, nb, gen):
    j = torch.arange(nb)
    if kind == "all_from_one":
        return torch.full((nb,), nb - 1)
    if kind == "cyclic":
        return (j + 1) % nb
    if kind == "swap":
        j[0], j[nb - 1] = nb - 1, 0
        return j
    if kind == "random":      # with repeats: a beam usually has several children
        return torch.randint(0, nb, (nb,), generator=gen)
    return j


def _want_reorder(cache, prompt, mask, parents, tokens, index, nb, length):
    """the host statement: torch.take_along_dim (numpy's take_along_axis) over the beams of a batch row, positions >= length of the cache left as they are"""
    Bn = parents.numel() // nb
    par = parents.view(Bn, nb).long()
    want_cache = None
    if cache is not None:
        grouped = cache.view(Bn, nb, *cache.shape[1:])
        moved = torch.take_along_dim(grouped, par.view(Bn, nb, 1, 1, 1, 1, 1).expand_as(grouped), dim=1).reshape(cache.shape)
        want_cache = cache.clone()
        want_cache[:, :, :, :length] = moved[:, :, :, :length]
    S = prompt.shape[1]
    want_prompt = torch.take_along_dim(prompt.view(Bn, nb, S), par.view(Bn, nb, 1).expand(-1, -1, S), dim=1).reshape(Bn * nb, S)
    want_prompt[:, index] = torch.where(mask[:, index], want_prompt[:, index], tokens.to(prompt.dtype))
    return want_cache, want_prompt


@pytest.mark.parametrize("nkv,h", [(1, 64), (2, 64), (1, 256), (2, 256)], ids=["1x64", "2x64", "1x256", "2x256"])
@pytest.mark.parametrize("nb", [1, 2, 5, 16])
def test_reorder_is_take_along_axis_bit_for_bit(cuda, nb, nkv, h):
    """cache [B nb, 2, 2, 37, nkv, h] of random bf16 BIT PATTERNS (NaNs among them), every beam different at every position, so the positions
    >= len are poisoned with values the gather would change; B in {1, 3}, len in {0, 1, 17, 37}, the five mappings rotating over the batch rows.
    The cache and the prompt must equal the host statement bit for bit, which leaves the positions >= len as they were.  Prompts in int64 and
    int32 with user tokens (kept) at the step's position in some rows."""
    from iseg_amd import functional as F

    L, S = 2, 37
    gen = torch.Generator().manual_seed(nb * 1000 + nkv * 300 + h)
    turn = 0
    for Bn in (1, 3):
        for length in (0, 1, 17, 37):
            for first in range(0, len(MAPPINGS), 2 if Bn == 3 else 1):
                turn += 1
                cache = torch.randint(-32768, 32768, (Bn * nb, L, 2, S, nkv, h), generator=gen, dtype=torch.int32).to(torch.int16)
                ids_dtype = torch.int64 if turn % 2 else torch.int32
                prompt = torch.randint(0, 1000, (Bn * nb, S), generator=gen).to(ids_dtype)
                mask = torch.rand(Bn * nb, S, generator=gen) < 0.3
                parents = torch.cat([_mapping(MAPPINGS[(first + b) % len(MAPPINGS)], nb, gen) for b in range(Bn)]).to(torch.int32)
                tokens = torch.randint(1000, 2000, (Bn * nb,), generator=gen).to(torch.int32)
                index = min(length, S - 1)
                want_cache, want_prompt = _want_reorder(cache, prompt, mask, parents, tokens, index, nb, length)
                cd, pd = cache.to(cuda).view(torch.bfloat16), prompt.to(cuda)
                back_cache, back_prompt = F.beam_reorder(cd, pd, mask.to(cuda), parents.to(cuda), tokens.to(cuda), index, nb, length=length)
                assert back_cache is cd and back_prompt is pd      # in place
                note = (Bn, length, MAPPINGS[first], ids_dtype)
                assert torch.equal(cd.view(torch.int16).cpu(), want_cache), note
                assert torch.equal(pd.cpu(), want_prompt), note


def test_reorder_leaves_a_group_with_a_bad_parent_alone(cuda):
    """three groups, the middle one with a parent of nb (once) and of -1 (once): cache and prompt of that group keep their bits, the others move"""
    from iseg_amd import functional as F

    nb, Bn, S = 4, 3, 9
    gen = torch.Generator().manual_seed(21)
    for badp in (nb, -1):
        cache = torch.randint(-32768, 32768, (Bn * nb, 1, 2, S, 1, 64), generator=gen, dtype=torch.int32).to(torch.int16)
        prompt = torch.randint(0, 1000, (Bn * nb, S), generator=gen)
        mask = torch.zeros(Bn * nb, S, dtype=torch.bool)
        parents = torch.tensor([1, 0, 3, 3, 2, badp, 0, 1, 3, 3, 0, 0], dtype=torch.int32)
        tokens = torch.arange(2000, 2000 + Bn * nb, dtype=torch.int32)
        valid = parents.clone()
        valid[nb:2 * nb] = torch.arange(nb, dtype=torch.int32)
        want_cache, want_prompt = _want_reorder(cache, prompt, mask, valid, tokens, 5, nb, 5)
        want_prompt[nb:2 * nb] = prompt[nb:2 * nb]      # not even the tokens are written
        cd, pd = cache.to(cuda).view(torch.bfloat16), prompt.to(cuda)
        F.beam_reorder(cd, pd, mask.to(cuda), parents.to(cuda), tokens.to(cuda), 5, nb)
        assert torch.equal(cd.view(torch.int16).cpu(), want_cache) and torch.equal(pd.cpu(), want_prompt)


def test_reorder_without_a_cache_with_a_cache_of_another_length_and_with_expanded_rows(cuda):
    """the prompt-only launch (cache None); a cache whose position axis is longer (53) or shorter (20) than the prompt's 37, filled to its
    end and less: the cache's addresses follow ITS length; a mask that is one row expanded over the beams takes the composed route (new
    tensors) with the statement's result.  All bit for bit against the host statement."""
    from iseg_amd import functional as F

    nb, Bn, S = 5, 3, 37
    gen = torch.Generator().manual_seed(41)
    prompt = torch.randint(0, 1000, (Bn * nb, S), generator=gen)
    mask = torch.rand(Bn * nb, S, generator=gen) < 0.3
    parents = torch.cat([_mapping(k, nb, gen) for k in ("random", "cyclic", "all_from_one")]).to(torch.int32)
    tokens = torch.randint(1000, 2000, (Bn * nb,), generator=gen).to(torch.int32)
    _, want_prompt = _want_reorder(None, prompt, mask, parents, tokens, 30, nb, 0)
    pd = prompt.to(cuda)
    back = F.beam_reorder(None, pd, mask.to(cuda), parents.to(cuda), tokens.to(cuda), 30, nb)
    assert back[0] is None and back[1] is pd and torch.equal(pd.cpu(), want_prompt)
    for Sc, length, index in ((53, 53, 36), (53, 41, 36), (20, 20, 19), (20, 7, 7)):
        cache = torch.randint(-32768, 32768, (Bn * nb, 2, 2, Sc, 1, 64), generator=gen, dtype=torch.int32).to(torch.int16)
        want_cache, want_prompt = _want_reorder(cache, prompt, mask, parents, tokens, index, nb, length)
        cd, pd = cache.to(cuda).view(torch.bfloat16), prompt.to(cuda)
        back = F.beam_reorder(cd, pd, mask.to(cuda), parents.to(cuda), tokens.to(cuda), index, nb, length=length)
        assert back[0] is cd and back[1] is pd
        assert torch.equal(cd.view(torch.int16).cpu(), want_cache) and torch.equal(pd.cpu(), want_prompt), (Sc, length)
    shared = (torch.rand(1, S, generator=gen) < 0.3)
    cache = torch.randint(-32768, 32768, (Bn * nb, 1, 2, S, 1, 64), generator=gen, dtype=torch.int32).to(torch.int16)
    want_cache, want_prompt = _want_reorder(cache, prompt, shared.expand(Bn * nb, S), parents, tokens, 30, nb, S)
    cd, pd = cache.to(cuda).view(torch.bfloat16), prompt.to(cuda)
    new_cache, new_prompt = F.beam_reorder(cd, pd, shared.to(cuda).expand(Bn * nb, S), parents.to(cuda), tokens.to(cuda), 30, nb, length=S)
    assert new_cache is not cd and torch.equal(new_cache.view(torch.int16).cpu(), want_cache) and torch.equal(new_prompt.cpu(), want_prompt)
    assert torch.equal(pd.cpu(), prompt)      # the composed route does not write its inputs
    with pytest.raises(ValueError, match="lies on"):
        F.beam_reorder(None, pd, mask, parents.to(cuda), tokens.to(cuda), 30, nb)


def test_reorder_inside_guard_bands(cuda):
    """cache, prompt, mask, parents and tokens between bands of poison: the bands are intact after the call and the result is the statement's"""
    from iseg_amd import kernels as K

    nb, Bn, S, length = 5, 3, 37, 17
    gen = torch.Generator().manual_seed(31)
    cache = torch.randint(-32768, 32768, (Bn * nb, 2, 2, S, 1, 64), generator=gen, dtype=torch.int32).to(torch.int16)
    prompt = torch.randint(0, 1000, (Bn * nb, S), generator=gen)
    mask = torch.rand(Bn * nb, S, generator=gen) < 0.3
    parents = torch.randint(0, nb, (Bn * nb,), generator=gen).to(torch.int32)
    tokens = torch.randint(1000, 2000, (Bn * nb,), generator=gen).to(torch.int32)
    want_cache, want_prompt = _want_reorder(cache, prompt, mask, parents, tokens, length, nb, length)
    arena = GM.Arena(cuda, 32 << 20)
    with GM.guarded(arena):
        dev = []
        for t in (cache, prompt, mask, parents, tokens):
            d = arena.alloc(t.shape, t.dtype, "operand")
            d.copy_(t)
            dev.append(d)
        cd, pd, md, pard, tokd = dev
        K.beam_reorder(cd.view(torch.bfloat16), length, pd, md, tokd, length, pard, nb)
        arena.check()
    assert torch.equal(cd.cpu(), want_cache) and torch.equal(pd.cpu(), want_prompt)


# ---- the model -------------------------------------------------------------------------------------------------------------------------------
def _inputs(cuda):
    ids, mask = _prompts()
    ids = ids * mask
    return ids, mask, {"token_ids": ids.to(cuda), "padding_mask": mask.to(cuda)}


def _next_of(model):
    def next(prompt, cache, index):
        logits, hidden, cache = model.call_with_cache(prompt[:, index - 1:index], cache, index - 1)
        return logits[:, 0], hidden[:, 0], cache

    return next


def test_one_beam_is_the_greedy_generation(cuda, bf16):  # noqa: F811
    from iseg_amd.nlp.samplers import BeamSampler

    model, _ = _model(torch.bfloat16)
    ids, mask, inputs = _inputs(cuda)
    model.compile(sampler="greedy")
    want = model.generate_step(inputs)
    end = int(want["token_ids"][0, PROMPTS[0] + 2].item())
    want_end = model.generate_step(inputs, end_token_id=end)
    model.compile(sampler=BeamSampler(num_beams=1))
    for ref, e in ((want, None), (want_end, end)):
        got = model.generate_step(inputs, end_token_id=e)
        assert torch.equal(got["token_ids"], ref["token_ids"]) and torch.equal(got["padding_mask"], ref["padding_mask"])
    assert torch.equal(inputs["token_ids"].cpu(), ids)


@pytest.mark.parametrize("nb", [2, 5])
def test_beam_generation_step_by_step(cuda, bf16, nb, monkeypatch):  # noqa: F811
    """a spy around F.beam_select records every step's logits, running scores and selection: each step passes the oracle; the final prompts
    and scores are a numpy replay of the recorded parents and tokens; generate_step returns the first beam; user tokens are kept.
    The cache: the prompts as they stood in front of the last step are each row's own lineage, so the plain per-token decode over them, at the
    same batch size B nb on a cache seeded the same way, must give the last step's logits bit for bit -- a row's arithmetic does not depend on
    its batch neighbours, and a wrong in-place reorder leaves some row with another lineage's keys and values.  With graph_decode=True the
    result is the eager one (a beam step keeps the eager loop)."""
    from iseg_amd import functional as F
    from iseg_amd.nlp.samplers import BeamSampler

    model, _ = _model(torch.bfloat16)
    ids, mask, inputs = _inputs(cuda)
    index = PROMPTS[0]
    steps, inner = [], F.beam_select

    def spy(logits, log_probs, num_beams, temperature=1.0, splits=0):
        out = inner(logits, log_probs, num_beams, temperature, splits)
        steps.append((logits.clone(), log_probs.cpu(), [t.cpu() for t in out]))
        return out

    monkeypatch.setattr(F, "beam_select", spy)
    _, cache = model._build_cache(inputs["token_ids"])
    prompts, scores = BeamSampler(num_beams=nb, return_all_beams=True)(_next_of(model), inputs["token_ids"], cache, index, inputs["padding_mask"])
    assert len(steps) == MS - index and tuple(prompts.shape) == (MB, nb, MS) and tuple(scores.shape) == (MB, nb)
    worst = 0.0
    state = np.repeat(ids.numpy(), nb, axis=0)
    rmask = np.repeat(mask.numpy(), nb, axis=0)
    base = (np.arange(MB * nb) // nb) * nb
    before_last = None
    for k, (logits, lp, (parents, tokens, new_lp)) in enumerate(steps):
        x = logits.cpu()
        bad = R.accepted(parents, tokens, new_lp, x, lp, nb, 1.0, C_UNITS)
        assert not bad, (k, bad[:3])
        worst = max(worst, R.worst_units(new_lp, parents, tokens, x, lp, nb, 1.0))
        if k:
            assert torch.equal(lp, steps[k - 1][2][2])      # the running scores are the previous selection's
        if k == len(steps) - 1:
            before_last = state.copy()
        state = state[base + parents.numpy()]
        state[:, index + k] = np.where(rmask[:, index + k], state[:, index + k], tokens.numpy())
    print(f"nb {nb}: worst score error over {len(steps)} steps {worst:.2f} units")
    assert np.array_equal(prompts.cpu().numpy().reshape(MB * nb, MS), state)      # the last selection is sorted: no further reordering
    assert torch.equal(scores.cpu().reshape(-1), steps[-1][2][2])
    assert all(torch.equal(prompts[b, j].cpu()[mask[b]], ids[b][mask[b]]) for b in range(MB) for j in range(nb))
    assert len({tuple(r) for r in state[:nb].tolist()}) == nb      # the beams of a row are different hypotheses

    monkeypatch.setattr(F, "beam_select", inner)
    _, seed = model._build_cache(inputs["token_ids"])
    replay = torch.repeat_interleave(seed, nb, dim=0)
    lineage = torch.from_numpy(before_last).to(cuda)
    for i in range(index, MS):
        logits, _, replay = model.call_with_cache(lineage[:, i - 1:i], replay, i - 1)
    assert torch.equal(logits[:, 0].view(torch.int16), steps[-1][0].view(torch.int16))

    model.compile(sampler=BeamSampler(num_beams=nb))
    eager = model.generate_step(inputs)
    assert torch.equal(eager["token_ids"], prompts[:, 0]) and bool(eager["padding_mask"].all())
    assert torch.equal(inputs["token_ids"].cpu(), ids)
    model.compile(sampler=BeamSampler(num_beams=nb), graph_decode=True)
    graphed = model.generate_step(inputs)
    assert torch.equal(graphed["token_ids"], eager["token_ids"])
    model.compile(sampler=BeamSampler(num_beams=nb, return_all_beams=True))
    with pytest.raises(ValueError, match="call the sampler directly"):
        model.generate_step(inputs)
