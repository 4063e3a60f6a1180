"""The contrastive-search kernels on the GPU (csrc/contrastive.hip through F.contrastive_candidates, F.contrastive_select, F.contrastive_commit and
iseg_amd.nlp.samplers.ContrastiveSampler) against the fp64 oracle of tests/contrastive_ref.py, and contrastive search through GemmaCausalLM.

Tolerances (derived in tests/contrastive_ref.py; the oracle reads the stored values, so inputs are exact):
  probabilities  3 units of 2^-23, relative (the weight-and-sum derivation at the head of tests/test_beam_search_gpu.py; the candidate's own
                 weight and the quotient are fp64 and rounded once);
  max_sim        eps_sim = (2 D + 8) 2^-24, absolute;
  scores         eps_score = (1 - alpha) 3 2^-23 + alpha eps_sim + 2^-23;
  winner         ref_score[winner] >= max ref_score - 2 eps_score, and the oracle's argmax wherever its margin exceeds that.  No case is left out.
Every case prints its worst figure in these units."""
import os

import pytest
import torch

from tests import contrastive_ref as R
from tests import guarded_memory as GM
from tests.test_beam_search_gpu import _inputs, _next_of
from tests.test_gemma_cache_gpu import B as MB
from tests.test_gemma_cache_gpu import PROMPTS, S as MS
from tests.test_gemma_cache_gpu import _model, bf16  # noqa: F401  (bf16 is a fixture)
from tests.test_token_sample_gpu import _ld, _pitched, _rows

pytestmark = pytest.mark.gpu

TILE = 2048
VS = ["k", 63, 64, 65, 2047, 2048, 2049, 4099, 70001]
KS = [1, 2, 5, 16]
BS = [1, 3]
TS = [0.25, 1.0, 4.0]
PITCHES = ["tight", "plus24", "aligned"]
DS = [8, 64, 72, 256, 2048, 3072]
INDEXES = [1, 2, 15, 16, 17, 63, 64, 65, 1000]


def _same_bits(a, b):
    return all(torch.equal(x.cpu().view(torch.int32), y.cpu().view(torch.int32)) for x, y in zip(a, b))


@pytest.fixture
def composed_route():
    """ISEG_CONTRASTIVE_FUSED=0 for the calls made through the returned function"""

    def run(fn, *args, **kwargs):
        os.environ["ISEG_CONTRASTIVE_FUSED"] = "0"
        try:
            return fn(*args, **kwargs)
        finally:
            os.environ.pop("ISEG_CONTRASTIVE_FUSED", None)

    yield run
    os.environ.pop("ISEG_CONTRASTIVE_FUSED", None)


# ---- candidates ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("V", VS)
def test_candidates_against_the_oracle(cuda, V, dtype):
    """every k <= V at this V ("k": V = k) and dtype; the batch size, the temperature, the forced chunk count (0: the plan; 1; 2; 3; one chunk
    per tile), the row pitch (padding columns hold NaN), the first row's logit family and whether a row map is used rotate with k and the case.
    Rows of a batch are of successive families (gaussian, four levels with heavy ties, one far above, a third at -inf).  A second call
    returns the same bits."""
    from iseg_amd import functional as F

    case = VS.index(V) * 2 + (dtype == torch.float32)
    gen = torch.Generator().manual_seed(3000 + case)
    worst = 0.0
    for i, k in enumerate(KS):
        Vk = k if V == "k" else V
        if k > Vk:
            continue
        tiles = -(-Vk // TILE)
        for rep in range(2):
            j = 2 * i + rep + case
            Bn, T = BS[j % 2], TS[(j // 2) % 3]
            splits, pitch, mapped = [0, 1, 2, tiles, 3][j % 5], PITCHES[(j // 5) % 3], (j // 2) % 2 == 1
            g = (1, 2, k)[j % 3] if mapped else 1
            x = _rows(Bn * g, Vk, dtype, gen, j % 4)
            row_map = torch.randint(0, g, (Bn,), generator=gen).to(torch.int32) if mapped else None
            xd = _pitched(x, _ld(Vk, pitch), cuda)
            md = None if row_map is None else row_map.to(cuda)
            probs, tokens = F.contrastive_candidates(xd, k, T, md, splits=splits)
            note = (Vk, k, Bn, T, splits, pitch, g, None if row_map is None else row_map.tolist())
            assert probs.dtype == torch.float32 and tokens.dtype == torch.int32 and tuple(probs.shape) == tuple(tokens.shape) == (Bn, k), note
            bad, w = R.candidates_accepted(probs, tokens, x, k, T, row_map)
            worst = max(worst, w)
            assert not bad, (note, bad[:3])
            again = F.contrastive_candidates(xd, k, T, md, splits=splits)
            assert _same_bits((probs, tokens), again), note
    print(f"V {V} {dtype}: worst probability error {worst:.2f} units of 2^-23 relative")
    assert worst <= R.PROB_UNITS


def test_candidates_of_a_quarter_million_entries(cuda):
    """V = 256000, bf16, Gemma's head: the chunk plan, one chunk and the most chunks; with a row map over five candidate rows"""
    from iseg_amd import functional as F
    from iseg_amd import kernels as K

    V, gen = 256000, torch.Generator().manual_seed(6)
    assert K.contrastive_candidates_splits(1, V) > 1
    for k, Bn, T, splits, g in ((5, 1, 1.0, 0, 5), (16, 1, 0.25, 1, 1), (2, 2, 4.0, V // TILE, 1)):
        x = _rows(Bn * g, V, torch.bfloat16, gen, 0)
        row_map = torch.randint(0, g, (Bn,), generator=gen).to(torch.int32) if g > 1 else None
        probs, tokens = F.contrastive_candidates(x.to(cuda), k, T, None if row_map is None else row_map.to(cuda), splits=splits)
        bad, w = R.candidates_accepted(probs, tokens, x, k, T, row_map)
        print(f"k {k} splits {splits}: worst {w:.2f} units")
        assert not bad, (k, splits, bad[:3])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_candidates_with_non_finite_rows_and_the_composed_route(cuda, dtype, composed_route):
    """a NaN logit, a +inf logit and a row of -inf alone beside an ordinary row: NaN probabilities and the first k tokens; the composed route
    (torch's fp32 softmax: 8 units) gives the same tokens and NaN pattern"""
    from iseg_amd import functional as F

    V, k = 4099, 5
    x = _rows(4, V, dtype, torch.Generator().manual_seed(9), 0)
    x[0, 3000] = float("nan")
    x[1, 17] = float("inf")
    x[2] = float("-inf")
    probs, tokens = F.contrastive_candidates(x.to(cuda), k, 1.0)
    bad, _ = R.candidates_accepted(probs, tokens, x, k, 1.0)
    assert not bad, bad
    assert bool(torch.isnan(probs[:3]).all()) and tokens[:3].cpu().tolist() == [list(range(k))] * 3
    cp, ct = composed_route(F.contrastive_candidates, x.to(cuda), k, 1.0)
    assert torch.equal(ct, tokens) and torch.equal(torch.isnan(cp), torch.isnan(probs))
    bad, _ = R.candidates_accepted(cp, ct, x, k, 1.0, units=8)
    assert not bad, bad


def test_candidates_inside_guard_bands(cuda):
    from iseg_amd import kernels as K

    for Bn, g, k, V, dtype, splits in ((1, 5, 5, 4099, torch.bfloat16, 0), (2, 1, 16, 70001, torch.bfloat16, 0), (3, 2, 1, 257, torch.float32, 0),
                                       (1, 1, 8, 70001, torch.float32, 35)):
        gen = torch.Generator().manual_seed(V + k)
        x = _rows(Bn * g, V, dtype, gen, 0)
        row_map = torch.randint(0, g, (Bn,), generator=gen).to(torch.int32) if g > 1 else None
        plain = K.contrastive_candidates(x.to(cuda), k, 1.0, None if row_map is None else row_map.to(cuda), splits)
        arena = GM.Arena(cuda, 32 << 20)
        with GM.guarded(arena):
            xd = arena.alloc(x.shape, x.dtype, "operand")
            xd.copy_(x)
            md = None
            if row_map is not None:
                md = arena.alloc(row_map.shape, row_map.dtype, "operand")
                md.copy_(row_map)
            got = K.contrastive_candidates(xd, k, 1.0, md, splits)
            arena.check()
            roles = [r.role for r in arena.records]
            assert roles.count("workspace") == 1 and roles.count("output") == 2
            ws = [r for r in arena.records if r.role == "workspace"][0]
            assert ws.end - ws.start == K._hip.lib().iseg_contrastive_candidates_scratch_bytes(Bn, V, k, splits) > 0
        assert _same_bits(got, plain)
        bad, _ = R.candidates_accepted(*got, x, k, 1.0, row_map)
        assert not bad, bad


# ---- select ----------------------------------------------------------------------------------------------------------------------------------
def _select_inputs(Bn, k, S, D, index, dtype, gen):
    """hidden states ~ N(0, 1) with a common offset (similarities spread over (0, 1)), NaN at every position >= index; probabilities of a
    softmax's k largest"""
    hs = (torch.randn(Bn, S, D, generator=gen) + 0.5 * torch.randn(Bn, 1, D, generator=gen)).to(dtype)
    hs[:, index:] = float("nan")
    cand = (torch.randn(Bn * k, D, generator=gen) + 0.3).to(dtype)
    probs = torch.sort(torch.softmax(2.0 * torch.randn(Bn, 4 * k, generator=gen), -1), dim=-1, descending=True).values[:, :k].reshape(-1).contiguous()
    return hs, cand, probs


def _forced_splits(index):
    return sorted({0, 1, min(2, index), min(3, index), index})


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("D", DS)
def test_select_against_the_oracle(cuda, D, dtype):
    """every filled length at this D and dtype; k, the batch size and alpha rotate with the length and the case, so that over the cases every
    value meets every D.  S > index and every position >= index holds NaN: none may reach an output.  Every forced chunk count (the plan, 1,
    2, 3, one position per chunk) returns the same bits."""
    from iseg_amd import functional as F

    case = DS.index(D) * 2 + (dtype == torch.float32)
    gen = torch.Generator().manual_seed(4000 + case)
    worst_ms = worst_sc = 0.0
    for i, index in enumerate(INDEXES):
        for rep in range(2):
            j = 2 * i + rep + case
            k, Bn, alpha = KS[j % 4], BS[(j // 4) % 2], (0.5, 0.6, 0.9, 0.1)[(j // 2) % 4]
            if index == 1000 and D >= 2048:
                Bn = 1      # the oracle's [B, k, index] einsum over D stays small
            S = index + (1, 3)[j % 2]
            hs, cand, probs = _select_inputs(Bn, k, S, D, index, dtype, gen)
            hd, cd, pd = hs.to(cuda), cand.to(cuda), probs.to(cuda)
            first = None
            for splits in _forced_splits(index):
                got = F.contrastive_select(hd, index, cd, pd, alpha, splits=splits)
                if first is None:
                    first = got
                    note = (D, index, k, Bn, alpha)
                    assert [t.dtype for t in got] == [torch.int32, torch.float32, torch.float32], note
                    assert [tuple(t.shape) for t in got] == [(Bn,), (Bn * k,), (Bn * k,)], note
                    bad, w_ms, w_sc = R.select_accepted(*got, hs, index, cand, probs, alpha, k)
                    worst_ms, worst_sc = max(worst_ms, w_ms), max(worst_sc, w_sc)
                    assert not bad, (note, bad[:3])
                else:
                    assert _same_bits(first, got), (D, index, k, Bn, splits)
    print(f"D {D} {dtype}: worst max_sim error {worst_ms:.3f} eps_sim, worst score error {worst_sc:.3f} eps_score")
    assert worst_ms <= 1.0 and worst_sc <= 1.0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_select_planted_cases(cuda, dtype, composed_route):
    """a candidate equal to the history vector at the first position, at the last, and on either side of each border of three forced chunks:
    max_sim within eps_sim of 1, and that candidate loses at alpha = 1; alpha = 0: candidate 0 (the most probable) wins; a zero vector in the
    history: NaN for every candidate of that row; a zero vector as a candidate: NaN for that candidate, which wins -- NaN exactly where the
    composed route has it"""
    from iseg_amd import functional as F

    Bn, k, D, index, S = 2, 5, 72, 64, 70
    gen = torch.Generator().manual_seed(77)
    borders = sorted({0, index - 1} | {s * index // 3 - d for s in (1, 2) for d in (0, 1)})
    for t in borders:
        hs, cand, probs = _select_inputs(Bn, k, S, D, index, dtype, gen)
        cand[3] = hs[0, t]
        cand[k + 1] = 2.0 * hs[1, t].float()      # a positive multiple: the same direction (exact in both dtypes)
        for alpha in (1.0, 0.0, 0.5):
            got = None
            for splits in (3, 0, 1, index):
                out = F.contrastive_select(hs.to(cuda), index, cand.to(cuda), probs.to(cuda), alpha, splits=splits)
                assert got is None or _same_bits(got, out)
                got = out
            winner, scores, max_sim = (x.cpu() for x in got)
            bad, _, _ = R.select_accepted(winner, scores, max_sim, hs, index, cand, probs, alpha, k)
            assert not bad, (t, alpha, bad)
            assert abs(max_sim[3].item() - 1.0) <= R.eps_sim(D) and abs(max_sim[k + 1].item() - 1.0) <= R.eps_sim(D), (t, max_sim.tolist())
            if alpha == 1.0:
                assert winner[0].item() != 3 and winner[1].item() != 1
            if alpha == 0.0:
                assert winner.tolist() == [0, 0]
    hs, cand, probs = _select_inputs(Bn, k, S, D, index, dtype, gen)
    hs[1, 40] = 0.0      # a zero vector in the history of row 1
    cand[2] = 0.0        # and a zero candidate in row 0
    args = (hs.to(cuda), index, cand.to(cuda), probs.to(cuda), 0.5)
    winner, scores, max_sim = (x.cpu() for x in F.contrastive_select(*args))
    cw, cs, cm = (x.cpu() for x in composed_route(F.contrastive_select, *args))
    want_nan = torch.tensor([False, False, True, False, False] + [True] * k)
    assert torch.equal(torch.isnan(max_sim), want_nan) and torch.equal(torch.isnan(cm), want_nan)
    assert torch.equal(torch.isnan(scores), want_nan) and torch.equal(torch.isnan(cs), want_nan)
    assert winner.tolist() == cw.tolist() == [2, 0]
    bad, _, _ = R.select_accepted(winner, scores, max_sim, hs, index, cand, probs, 0.5, k)
    assert not bad, bad
    bad, _, _ = R.select_accepted(cw, cs, cm, hs, index, cand, probs, 0.5, k)
    assert not bad, bad


def test_select_inside_guard_bands(cuda):
    """hidden states, candidates, probabilities, the three outputs and a scratch buffer of EXACTLY iseg_contrastive_select_scratch_bytes between
    bands of poison; positions >= index hold NaN.  The bands are intact, and the results are the unguarded call's"""
    from iseg_amd import kernels as K

    for Bn, k, D, index, S, dtype, splits in ((1, 5, 2048, 65, 66, torch.bfloat16, 0), (3, 16, 72, 17, 20, torch.float32, 0),
                                              (2, 2, 8, 1, 2, torch.bfloat16, 0), (1, 16, 3072, 100, 101, torch.float32, 7),
                                              (2, 1, 256, 1000, 1001, torch.bfloat16, 0)):
        gen = torch.Generator().manual_seed(D + k)
        hs, cand, probs = _select_inputs(Bn, k, S, D, index, dtype, gen)
        plain = K.contrastive_select(hs.to(cuda), index, cand.to(cuda), probs.to(cuda), 0.5, splits)
        arena = GM.Arena(cuda, 64 << 20)
        with GM.guarded(arena):
            ops = []
            for t in (hs, cand, probs):
                d = arena.alloc(t.shape, t.dtype, "operand")
                d.copy_(t)
                ops.append(d)
            got = K.contrastive_select(ops[0], index, ops[1], ops[2], 0.5, splits)
            arena.check()
            roles = [r.role for r in arena.records]
            assert roles.count("workspace") == 1 and roles.count("output") == 3
            ws = [r for r in arena.records if r.role == "workspace"][0]
            assert ws.end - ws.start == K._hip.lib().iseg_contrastive_select_scratch_bytes(Bn, index, D, k, splits, K.dt(hs)) > 0
        assert _same_bits(got, plain)
        bad, _, _ = R.select_accepted(*got, hs, index, cand, probs, 0.5, k)
        assert not bad, bad


def test_select_unsupported_shapes_take_the_composed_route(cuda):
    """D = 12 is no multiple of 8 and fp16 is no kernel dtype: the composed route answers, within its own fp32 bounds"""
    from iseg_amd import functional as F

    gen = torch.Generator().manual_seed(31)
    for D, dtype in ((12, torch.float32), (64, torch.float16)):
        hs, cand, probs = _select_inputs(2, 3, 9, D, 7, dtype, gen)
        got = F.contrastive_select(hs.to(cuda), 7, cand.to(cuda), probs.to(cuda), 0.5)
        bad, _, _ = R.select_accepted(*got, hs, 7, cand, probs, 0.5, 3)
        assert not bad, bad


# ---- commit ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,ids_dtype", [(torch.bfloat16, torch.int64), (torch.float32, torch.int32)], ids=["bf16-i64", "fp32-i32"])
@pytest.mark.parametrize("k", KS)
def test_commit_is_the_composed_broadcast_and_touches_nothing_else(cuda, k, dtype, ids_dtype):
    """a cache [B k, L, 2, Sc, nkv, h] with Sc != S, index at 0, in the middle and at Sc - 1, every tensor in guarded memory: afterwards every
    tensor equals the composed broadcast on clones bit for bit (so every byte outside position `index` is unchanged) and the bands are intact"""
    from iseg_amd import functional as F

    L, Sc, nkv, h, D = 2, 7, 2, 16, 72
    S = Sc + 3
    gen = torch.Generator().manual_seed(500 + k)
    for Bn in BS:
        for index in (0, 3, Sc - 1):
            cache = torch.randn(Bn * k, L, 2, Sc, nkv, h, generator=gen).to(dtype)
            prompt = torch.randint(0, 1000, (Bn * k, S), generator=gen).to(ids_dtype)
            hs = torch.randn(Bn, S, D, generator=gen).to(dtype)
            cand = torch.randn(Bn * k, D, generator=gen).to(dtype)
            winner = torch.randint(0, k, (Bn,), generator=gen).to(torch.int32)
            arena = GM.Arena(cuda, 16 << 20)
            ops = []
            for t in (cache, prompt, hs, cand, winner):
                d = arena.alloc(t.shape, t.dtype, "operand")
                d.copy_(t)
                ops.append(d)
            want = R.commit_broadcast(cache, prompt, hs, cand, winner, index, k)
            got = F.contrastive_commit(ops[0], ops[1], ops[2], ops[3], ops[4], index, k)
            arena.check()
            assert got[0].data_ptr() == ops[0].data_ptr() and got[1].data_ptr() == ops[1].data_ptr() and got[2].data_ptr() == ops[2].data_ptr()
            bits = torch.int16 if dtype == torch.bfloat16 else torch.int32
            assert torch.equal(got[0].cpu().view(bits), want[0].view(bits)), (k, Bn, index)
            assert torch.equal(got[1].cpu(), want[1]) and torch.equal(got[2].cpu().view(bits), want[2].view(bits)), (k, Bn, index)
            assert torch.equal(ops[3].cpu().view(bits), cand.view(bits)) and torch.equal(ops[4].cpu(), winner)


def test_commit_without_a_cache_and_with_a_winner_out_of_range(cuda, composed_route):
    from iseg_amd import functional as F

    gen = torch.Generator().manual_seed(41)
    Bn, k, S, D = 2, 3, 6, 16
    prompt = torch.randint(0, 99, (Bn * k, S), generator=gen)
    hs, cand = torch.randn(Bn, S, D, generator=gen), torch.randn(Bn * k, D, generator=gen)
    winner = torch.tensor([2, 1], dtype=torch.int32)
    want = R.commit_broadcast(None, prompt, hs, cand, winner, 4, k)
    got = F.contrastive_commit(None, prompt.to(cuda), hs.to(cuda), cand.to(cuda), winner.to(cuda), 4, k)
    assert got[0] is None and torch.equal(got[1].cpu(), want[1]) and torch.equal(got[2].cpu(), want[2])
    comp = composed_route(F.contrastive_commit, None, prompt.to(cuda), hs.to(cuda), cand.to(cuda), winner.to(cuda), 4, k)
    assert torch.equal(comp[1][:, 4].cpu(), want[1][:, 4]) and torch.equal(comp[2].cpu(), want[2])
    bad = torch.tensor([7, 1], dtype=torch.int32)      # group 0 is left untouched
    got = F.contrastive_commit(None, prompt.to(cuda), hs.to(cuda), cand.to(cuda), bad.to(cuda), 4, k)
    assert torch.equal(got[1][:k].cpu(), prompt[:k]) and torch.equal(got[2][0].cpu(), hs[0])
    assert torch.equal(got[1][k:].cpu(), want[1][k:]) and torch.equal(got[2][1].cpu(), want[2][1])


# ---- through GemmaCausalLM -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 5])
def test_contrastive_generation_step_by_step(cuda, bf16, k, monkeypatch):  # noqa: F811
    """spies around F.contrastive_select and F.contrastive_commit record every step.  Each recorded selection passes the oracle's acceptance rule
    on its own inputs (teacher-forced: no margin condition on the model's logits); each commit equals the composed broadcast on clones, bit
    for bit.  At the end the k rows of every group agree bit for bit over the filled prefix of prompt and cache; the result is [B, S] in the
    prompt's dtype; user tokens of the longer rows are kept; the caller's tensors are unwritten; graph_decode=True returns the eager tokens."""
    from iseg_amd import functional as F
    from iseg_amd.nlp.samplers import ContrastiveSampler

    model, _ = _model(torch.bfloat16)
    ids, mask, inputs = _inputs(cuda)
    index = PROMPTS[0]
    alpha = 0.6
    selects, commits = [], []
    inner_select, inner_commit = F.contrastive_select, F.contrastive_commit

    def spy_select(hidden_states, idx, cand_hidden, probs, a, splits=0):
        out = inner_select(hidden_states, idx, cand_hidden, probs, a, splits)
        selects.append((hidden_states.cpu(), idx, cand_hidden.cpu(), probs.cpu(), a, [t.cpu() for t in out]))
        return out

    def spy_commit(cache, prompt, hidden_states, cand_hidden, winner, idx, kk, position=None):
        want = R.commit_broadcast(cache, prompt, hidden_states, cand_hidden, winner, idx, kk, position)
        out = inner_commit(cache, prompt, hidden_states, cand_hidden, winner, idx, kk, position)
        commits.append((idx, all(torch.equal(o.view(torch.int16) if o.dtype == torch.bfloat16 else o, w.view(torch.int16) if w.dtype == torch.bfloat16 else w)
                                 for o, w in zip(out, want)), out))
        return out

    monkeypatch.setattr(F, "contrastive_select", spy_select)
    monkeypatch.setattr(F, "contrastive_commit", spy_commit)
    hidden, cache = model._build_cache(inputs["token_ids"])
    keep_cache, keep_hidden = cache.clone(), hidden.clone()
    out = ContrastiveSampler(k=k, alpha=alpha)(_next_of(model), inputs["token_ids"], cache, index, inputs["padding_mask"], hidden_states=hidden)
    assert len(selects) == len(commits) == MS - index
    assert tuple(out.shape) == (MB, MS) and out.dtype == inputs["token_ids"].dtype
    worst_ms = worst_sc = 0.0
    for step, (hs, idx, cand, probs, a, got) in enumerate(selects):
        assert idx == index + step and a == alpha and tuple(cand.shape) == (MB * k, hs.shape[2])
        bad, w_ms, w_sc = R.select_accepted(*got, hs, idx, cand, probs, a, k)
        worst_ms, worst_sc = max(worst_ms, w_ms), max(worst_sc, w_sc)
        assert not bad, (step, bad[:3])
    print(f"k {k}: over {len(selects)} steps worst max_sim error {worst_ms:.3f} eps_sim, worst score error {worst_sc:.3f} eps_score")
    assert all(ok for _, ok, _ in commits), [i for i, ok, _ in commits if not ok]
    last_cache, last_prompt, last_hist = commits[-1][2]
    groups_p, groups_c = last_prompt.view(MB, k, MS), last_cache.view(MB, k, *last_cache.shape[1:])
    for j in range(1, k):
        assert torch.equal(groups_p[:, j], groups_p[:, 0])
        assert torch.equal(groups_c[:, j].view(torch.int16), groups_c[:, 0].view(torch.int16))      # every position is filled at the end
    assert torch.equal(out, groups_p[:, 0])
    assert torch.equal(out.cpu()[mask], ids[mask])      # user tokens are kept
    assert torch.equal(inputs["token_ids"].cpu(), ids)
    assert torch.equal(cache.view(torch.int16), keep_cache.view(torch.int16)) and torch.equal(hidden.view(torch.int16), keep_hidden.view(torch.int16))
    # the history the loop kept is the winners' hidden states
    for step, (_, _, cand, _, _, got) in enumerate(selects):
        rows = torch.arange(MB) * k + got[0].long()
        assert torch.equal(last_hist[:, index + step].cpu().view(torch.int16), cand[rows].view(torch.int16))

    monkeypatch.setattr(F, "contrastive_select", inner_select)
    monkeypatch.setattr(F, "contrastive_commit", inner_commit)
    model.compile(sampler=ContrastiveSampler(k=k, alpha=alpha))
    eager = model.generate_step(inputs)
    assert torch.equal(eager["token_ids"], out) and bool(eager["padding_mask"].all())
    end = int(out[0, PROMPTS[0] + 2].item())
    ended = model.generate_step(inputs, end_token_id=end)
    assert tuple(ended["token_ids"].shape) == (MB, MS) and not bool(ended["padding_mask"][0].all())
    model.compile(sampler=ContrastiveSampler(k=k, alpha=alpha), graph_decode=True)
    graphed = model.generate_step(inputs)
    assert torch.equal(graphed["token_ids"], eager["token_ids"])
    assert torch.equal(inputs["token_ids"].cpu(), ids)
