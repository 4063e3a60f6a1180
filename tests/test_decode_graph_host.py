"""The replayed decode step, CPU side: the commit state machine (tests/decode_commit_ref.py) iterated against sample_loop of
iseg_amd/nlp/samplers.py on synthetic `next` functions, the freeze, the monotone split plan that lets a capacity-sized grid and workspace serve
every position (host arithmetic of the library, no device), the new bindings, and the refusals and defaults of compile(graph_decode=)."""
import os

import pytest
import torch

from tests import decode_commit_ref as R
from tests.test_gemma_host import TINY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
END = 7


def _choose(forced=None):
    """a synthetic model: the token at `index` is a function of the row, the previous token and the index, in [8, 8 + 89) so that it is never
    the end token 7 nor the padding 0; forced = {index: [tokens]} overrides whole steps"""
    forced = forced or {}

    def choose(prompt, index):
        if index in forced:
            return list(forced[index])
        return [8 + (5 * int(row[index - 1]) + 3 * index + 11 * b) % 89 for b, row in enumerate(prompt)]

    return choose


def _sample_loop(prompt, mask, index, end, choose):
    from iseg_amd.nlp.samplers import sample_loop

    calls = []

    def next(p, cache, i):
        calls.append(i)
        return torch.tensor(choose(p.tolist(), i)), None, cache

    out = sample_loop(lambda logits: logits, next, torch.tensor(prompt), None, index, torch.tensor(mask), end_token_id=end)
    return out.tolist(), calls


def _ragged(S, lengths, fill=0, seed=0):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(8, 90, (len(lengths), S), generator=g)
    mask = torch.zeros(len(lengths), S, dtype=torch.bool)
    for b, n in enumerate(lengths):
        mask[b, :n] = True
    ids = torch.where(mask, ids, torch.full_like(ids, fill))
    return ids.tolist(), mask.tolist(), min(lengths)


CASES = {
    # ragged masks, no end token: every position from the shortest prompt on is visited, longer rows keep their tokens
    "ragged_no_end": dict(S=12, lengths=(3, 5, 8), end=None, forced=None),
    # ragged masks with an end token that nobody emits
    "ragged_end_never": dict(S=12, lengths=(3, 5, 8), end=END, forced=None),
    # all rows reach the end token early: row 0 and 1 at index 5, row 2 (a user token there) at index 9
    "all_rows_end_early": dict(S=16, lengths=(3, 4, 8), end=END, forced={5: [END, END, END], 9: [20, 21, END]}),
    # one row ends, the others never do: the loop runs to the end and the finished row keeps generating
    "one_row_ends": dict(S=10, lengths=(2, 4), end=END, forced={3: [END, 30]}),
    # the end token equals the padding the prompt already holds (0): every padded row is done at the start
    "end_is_padding": dict(S=10, lengths=(3, 5), end=0, forced=None),
    # ... and with a row that has no padding at all the loop runs on
    "end_is_padding_one_full_row": dict(S=8, lengths=(8, 3), end=0, forced=None),
    # index == S: nothing to do
    "index_is_S": dict(S=6, lengths=(6, 6), end=END, forced=None),
    "single_row": dict(S=9, lengths=(1,), end=END, forced={4: [END]}),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_iterated_commit_is_sample_loop(name):
    c = CASES[name]
    prompt, mask, index = _ragged(c["S"], c["lengths"])
    choose = _choose(c["forced"])
    want, calls = _sample_loop(prompt, mask, index, c["end"], choose)
    st = R.State(prompt, mask, index, c["end"])
    live = R.run(st, choose)
    assert st.prompt == want
    assert live == len(calls) and calls == list(range(index, index + live))
    if live:
        assert st.pos == calls[-1] and st.cur_ids == [row[st.pos] for row in want]
    # user tokens are kept
    assert all(w == p for wr, pr, mr in zip(want, prompt, mask) for w, p, m in zip(wr, pr, mr) if m)
    if name == "all_rows_end_early":
        assert live == 7 and st.done == [True, True, True]      # the steps at indices 3 .. 9; the check in front of index 10 stops the loop
    if name in ("end_is_padding", "index_is_S"):
        assert live == 0 and st.prompt == prompt
    if name in ("ragged_no_end", "ragged_end_never", "one_row_ends", "end_is_padding_one_full_row"):
        assert live == c["S"] - index


@pytest.mark.parametrize("name", sorted(CASES))
def test_extra_launches_after_completion_change_nothing(name):
    c = CASES[name]
    prompt, mask, index = _ragged(c["S"], c["lengths"])
    choose = _choose(c["forced"])
    st = R.State(prompt, mask, index, c["end"])
    live = R.run(st, choose)
    before = st.snapshot()
    assert R.frozen(st)
    for _ in range(20):
        assert not R.commit(st, [END] * st.B)
    assert st.snapshot() == before
    # and the number of launches in between two looks at the state does not matter: extra launches inside run() are frozen too
    st2 = R.State(prompt, mask, index, c["end"])
    assert R.run(st2, choose, extra=15) == live and st2.snapshot() == before


def test_out_of_range_positions_are_frozen():
    st = R.State([[1, 2, 3]], [[True, False, False]], 1)
    for pos in (-2, -7, 2, 3, 100):
        st.pos = pos
        assert R.frozen(st) and not R.commit(st, [5])
    st.pos = -1      # p + 1 = 0 is a position
    assert R.commit(st, [5]) and st.pos == 0 and st.prompt == [[1, 2, 3]]


# ---- the split plan: what suffices for the capacity suffices for every position -----------------------------------------------------------------
def _lib():
    from iseg_amd import _hip

    if not os.path.exists(_hip.LIB_PATH):
        from iseg_amd.build import build

        build(verbose=False)
    return _hip.lib()


@pytest.mark.parametrize("groups", [1, 2, 8, 64])
def test_split_plan_and_scratch_are_monotone_in_the_position(groups):
    """for batch x nkv in {1, 2, 8, 64} and every pos0 < 4096: the planned chunk count and the scratch bytes (the plan's, and a forced count's)
    never decrease with pos0, hence never exceed those at S - 1 for any cache length S <= 4096"""
    L = _lib()
    nq, h = 8, 256
    for batch, nkv in ((groups, 1), (1, groups)) if groups > 1 else ((1, 1),):
        nqh = nq if nq % nkv == 0 else nkv
        last = (0, 0, 0)
        for pos0 in range(4096):
            got = (L.iseg_gemma_decode_attention_splits(batch, pos0, 1, nqh, nkv, h),
                   L.iseg_gemma_decode_attention_scratch_bytes(batch, pos0, 1, nqh, nkv, h, 0),
                   L.iseg_gemma_decode_attention_scratch_bytes(batch, pos0, 1, nqh, nkv, h, 3))
            assert got[0] >= 1 and got[1] > 0 and got[2] > 0
            assert all(a >= b for a, b in zip(got, last)), (batch, nkv, pos0, got, last)
            last = got
        top = (L.iseg_gemma_decode_attention_splits(batch, 4095, 1, nqh, nkv, h), L.iseg_gemma_decode_attention_scratch_bytes(batch, 4095, 1, nqh, nkv, h, 0))
        assert last[:2] == top and top[0] == min(-(-512 // groups), 32)


# ---- bindings, refusals, defaults -----------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound():
    from iseg_amd import _hip, build
    from iseg_amd import functional as F
    from iseg_amd import kernels as K

    header = open(os.path.join(ROOT, "include", "iseg_hip.h")).read()
    L = _lib()
    for name in ("iseg_gemma_rope_cache_at", "iseg_gemma_decode_attention_at", "iseg_decode_commit"):
        assert name in _hip.SIGNATURES and name + "(" in header and hasattr(L, name)
    for macro, value in (("ISEG_IDS_I32", _hip.IDS_I32), ("ISEG_IDS_I64", _hip.IDS_I64)):
        assert f"#define {macro} {value}" in header
    assert "decode_commit.hip" in build.SOURCES
    for mod, fns in ((K, ("gemma_rope_cache_at", "gemma_decode_attention_at", "decode_commit")), (F, ("decode_commit",))):
        for fn in fns:
            assert callable(getattr(mod, fn))


def test_compile_graph_decode_refusals_and_defaults():
    from iseg_amd.nlp import samplers as S
    from iseg_amd.nlp.gemma import GemmaBackbone, GemmaCausalLM

    model = GemmaCausalLM(GemmaBackbone(**TINY))
    assert model.graph_decode is False
    model.compile()
    assert model.graph_decode is False and model.sampler == "greedy"      # without the keyword generate_step stays on the old loop
    for bad in (1, 0, "yes", None):
        with pytest.raises(ValueError, match="graph_decode"):
            model.compile(graph_decode=bad)
    model.compile(sampler=S.TopKSampler(k=3, seed=1), graph_decode=True)
    assert model.graph_decode is True
    model.compile(sampler="greedy")
    assert model.graph_decode is False      # compile() sets both, as it sets the sampler
    assert model._decode_graphs == {}
    model.release_decode_graphs()


def test_only_the_library_samplers_take_the_graph():
    from iseg_amd.nlp import samplers as S
    from iseg_amd.nlp.gemma import GemmaBackbone, GemmaCausalLM

    class Mine(S.TopKSampler):
        def get_next_token(self, logits):
            return torch.zeros(logits.shape[0], dtype=torch.int64)

    class Plain(S.Sampler):
        def get_next_token(self, logits):
            return torch.argmax(logits, dim=-1)

    model = GemmaCausalLM(GemmaBackbone(**TINY))
    model.compile(graph_decode=True)
    assert model._graph_decode_sampler() == (True, None)
    for sampler in (S.GreedySampler(), S.RandomSampler(seed=1), S.TopKSampler(k=2, seed=1), S.TopPSampler(p=0.5, seed=1)):
        model.compile(sampler=sampler, graph_decode=True)
        assert model._graph_decode_sampler() == (True, sampler)
    for sampler in (Mine(k=2, seed=1), Plain()):
        model.compile(sampler=sampler, graph_decode=True)
        assert model._graph_decode_sampler()[0] is False      # routed to the eager loop

    # a subclass on the eager loop: generate_step must reach sample_loop through the sampler, not the graph
    seen = []
    model.compile(sampler=Plain(), graph_decode=True)
    model._build_cache = lambda ids, cache=None: (None, "cache")
    model._generate_graphed = lambda *a, **k: (_ for _ in ()).throw(AssertionError("a caller's sampler took the graph"))
    model.sampler.__class__.__call__ = lambda self, next, prompt, cache, index, mask, end_token_id=None: (seen.append((cache, index)), prompt)[1]
    ids = torch.tensor([[3, 4, 0, 0]])
    out = model.generate_step({"token_ids": ids, "padding_mask": ids != 0})
    assert seen == [("cache", 2)] and torch.equal(out["token_ids"], ids)


def test_sampler_signatures_and_rules():
    from iseg_amd.nlp import samplers as S

    a, b = S.TopKSampler(k=5, seed=7), S.TopKSampler(k=5, seed=8)
    assert a.graph_signature() == b.graph_signature() != S.TopKSampler(k=6, seed=7).graph_signature()
    assert a.graph_signature() != S.TopPSampler(p=0.9, k=5, seed=7).graph_signature()
    assert S.RandomSampler(temperature=0.5).graph_signature() != S.RandomSampler().graph_signature()
    assert S.GreedySampler().token_rule()(torch.tensor([[0.0, 2.0, 2.0], [3.0, 1.0, 0.0]])).tolist() == [1, 0]
    # uniforms_into is `uniforms`: the same generator, the same numbers, into the caller's buffer
    x, y, buf = S.RandomSampler(seed=3), S.RandomSampler(seed=3), torch.empty(5)
    logits = torch.zeros(5, 4)
    for _ in range(3):
        back = x.uniforms_into(buf)
        assert back.data_ptr() == buf.data_ptr() and torch.equal(buf, y.uniforms(logits))
    with pytest.raises(ValueError):
        x.uniforms_into(torch.empty(5, dtype=torch.float64))


def test_tensor_position_refuses_the_composed_and_seeding_routes(monkeypatch):
    """a tensor position with a shape or type outside the decode kernels' set is a ValueError before any memory is touched (CPU tensors here)"""
    from iseg_amd import functional as F
    from iseg_amd import nn

    pos = torch.zeros(1, dtype=torch.int32)
    nn.set_compute_dtype(torch.float32)
    q, cache = torch.zeros(1, 1, 4 * 64), torch.zeros(1, 2, 8, 2, 64)
    with pytest.raises(ValueError, match="tensor position"):
        F.gemma_cached_attention_core(q, cache, pos, 4, 2, 64)      # fp32: the composed route
    nn.set_compute_dtype(torch.bfloat16)
    try:
        with pytest.raises(ValueError, match="tensor position"):      # head width 96
            F.gemma_cached_attention_core(torch.zeros(1, 1, 4 * 96, dtype=torch.bfloat16), torch.zeros(1, 2, 8, 2, 96, dtype=torch.bfloat16), pos, 4, 2, 96)
        with pytest.raises(ValueError, match="tensor position"):      # 17 stacked rows
            F.gemma_cached_attention_core(torch.zeros(1, 1, 17 * 64, dtype=torch.bfloat16), torch.zeros(1, 2, 8, 1, 64, dtype=torch.bfloat16), pos, 17, 1, 64)
        with pytest.raises(ValueError, match="tensor position"):      # the seeding call: 8 rows x 4 heads per group
            F.gemma_cached_attention_core(torch.zeros(1, 8, 8 * 64, dtype=torch.bfloat16), torch.zeros(1, 2, 8, 2, 64, dtype=torch.bfloat16), pos, 8, 2, 64)
        monkeypatch.setenv("ISEG_GEMMA_FUSED", "0")
        with pytest.raises(ValueError, match="tensor position"):
            F.gemma_cached_attention_core(torch.zeros(1, 1, 4 * 64, dtype=torch.bfloat16), torch.zeros(1, 2, 8, 2, 64, dtype=torch.bfloat16), pos, 4, 2, 64)
        monkeypatch.delenv("ISEG_GEMMA_FUSED")
        for bad in (torch.zeros(1, dtype=torch.int64), torch.zeros(2, dtype=torch.int32)):
            with pytest.raises(ValueError, match="ONE int32"):
                F.gemma_cached_attention_core(torch.zeros(1, 1, 4 * 64, dtype=torch.bfloat16), torch.zeros(1, 2, 8, 2, 64, dtype=torch.bfloat16), bad, 4, 2, 64)
            with pytest.raises(ValueError, match="ONE int32"):
                F.gemma_rope_cache(torch.zeros(1, 1, 8 * 64, dtype=torch.bfloat16), torch.zeros(1, 2, 8, 2, 64, dtype=torch.bfloat16), bad, 4, 2, 64)
    finally:
        nn.set_compute_dtype(torch.float32)


def test_graph_decode_refuses_where_the_fused_kernels_do_not_run(monkeypatch):
    from iseg_amd import nn
    from iseg_amd.nlp.gemma import GemmaBackbone, GemmaCausalLM

    model = GemmaCausalLM(GemmaBackbone(**TINY))
    model.build = lambda: None
    model.built = True
    model.compile(graph_decode=True)
    ids = torch.tensor([[3, 4, 0, 0]])
    inputs = {"token_ids": ids, "padding_mask": ids != 0}
    nn.set_compute_dtype(torch.float32)
    with pytest.raises(ValueError, match="compute dtype"):
        model.generate_step(inputs)
    nn.set_compute_dtype(torch.bfloat16)
    try:
        monkeypatch.setenv("ISEG_GEMMA_FUSED", "0")
        with pytest.raises(ValueError, match="ISEG_GEMMA_FUSED"):
            model.generate_step(inputs)
        monkeypatch.delenv("ISEG_GEMMA_FUSED")
        model.backbone.head_dim = 96
        with pytest.raises(ValueError, match="head width 96"):
            model.generate_step(inputs)
        with pytest.raises(ValueError, match="check_every"):
            model.generate_step(inputs, check_every=0)
    finally:
        nn.set_compute_dtype(torch.float32)
