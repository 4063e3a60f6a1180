"""Token samplers, CPU side: hand-worked answers of the fp64 oracle (tests/token_sample_ref.py), the sampler classes of iseg_amd.nlp.samplers and
their decoding loop on a stub model, GemmaCausalLM.compile(sampler=), the new entry points, and the launcher's plan and refusals, which are host
arithmetic and need no device."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from tests import token_sample_ref as R
from tests.test_gemma_host import TINY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LN2 = math.log(2.0)
# weights 1/4, 1, 1, 1/2 (W = 2.75): two tied maxima at ids 1 and 2; the order is 1, 2, 3, 0
ROW = [0.0, 2 * LN2, 2 * LN2, LN2]
U_LAST = float(np.nextafter(np.float32(1), np.float32(0)))


def test_order_and_ties():
    assert R.order(np.array(ROW)).tolist() == [1, 2, 3, 0]
    assert R.order(np.array([1.0, float("nan"), float("inf"), -float("inf"), float("nan"), float("inf")])).tolist() == [1, 4, 2, 5, 0, 3]
    assert R.order(np.array([-0.0, 0.0, -1.0])).tolist() == [0, 1, 2]      # -0 ties with +0: the index decides


def test_top_k_known_answers():
    x = torch.tensor([ROW], dtype=torch.float64)
    assert R.kept_set(x[0], "top_k", k=1) == {1}
    assert R.kept_set(x[0], "top_k", k=2) == {1, 2}
    assert R.kept_set(x[0], "top_k", k=3) == {1, 2, 3} and R.kept_set(x[0], "top_k", k=9) == {0, 1, 2, 3}
    for u in (0.0, 0.3, U_LAST):
        assert R.exact_token(x[0], u, "top_k", k=1) == 1
        assert R.accepted_tokens(x, [u], "top_k", k=1) == [{1}]
    # k = 2: ids 1 and 2 weigh 1 each, S = 2; C_1 = 1 exceeds u S below u = 0.5 and not at it
    assert R.exact_token(x[0], 0.49, "top_k", k=2) == 1 and R.exact_token(x[0], 0.5, "top_k", k=2) == 2
    assert R.exact_token(x[0], 0.0, "top_k", k=2) == 1 and R.exact_token(x[0], U_LAST, "top_k", k=2) == 2
    assert R.accepted_tokens(x, [0.49], "top_k", k=2) == [{1}]
    assert R.accepted_tokens(x, [0.5], "top_k", k=2) == [{1, 2}]      # on the border the tolerance admits both neighbours
    assert R.accepted_tokens(x, [0.51], "top_k", k=2) == [{2}]


def test_top_p_known_answers():
    x = torch.tensor([ROW], dtype=torch.float64)
    first = 1.0 / 2.75      # the first position's share of the full softmax mass
    assert R.kept_set(x[0], "top_p", p=first - 1e-3) == {1}
    assert R.kept_set(x[0], "top_p", p=first + 1e-3) == {1, 2}
    assert R.kept_set(x[0], "top_p", p=1e-6) == {1}      # the first is always kept
    assert R.kept_set(x[0], "top_p", p=2 * first + 1e-3) == {1, 2, 3}
    assert R.kept_set(x[0], "top_p", p=1.0) == {0, 1, 2, 3}
    assert R.kept_set(x[0], "top_p", p=1.0, k=2) == {1, 2}      # only the first k positions are looked at
    assert R.exact_token(x[0], 0.9, "top_p", p=first - 1e-3) == 1
    assert R.exact_token(x[0], 0.9, "top_p", p=first + 1e-3) == 2
    # a cut within eps of p W: both kept sets are admissible, so u = 0.9 may give 1 (alone) or 2 (of two)
    assert R.accepted_tokens(x, [0.9], "top_p", p=first, eps=1e-5) == [{1, 2}]
    assert R.accepted_tokens(x, [0.9], "top_p", p=first, eps=1e-5, candidates=[1]) == [{1}]
    assert R.accepted_tokens(x, [0.9], "top_p", p=first, eps=1e-5, candidates=[3]) == [set()]
    assert R.accepted_tokens(x, [0.9], "top_p", p=first + 1e-3) == [{2}]


def test_random_known_answers_and_the_ends_of_u():
    x = torch.tensor([ROW, [-float("inf"), 2 * LN2, 2 * LN2, LN2]], dtype=torch.float64)
    # cumulative weights in id order: 0.25, 1.25, 2.25, 2.75
    assert R.exact_token(x[0], 0.0, "random") == 0 and R.exact_token(x[0], U_LAST, "random") == 3
    assert R.exact_token(x[0], 0.25 / 2.75 + 1e-9, "random") == 1 and R.exact_token(x[0], 0.8, "random") == 2
    # T = 2: weights 0.5, 1, 1, 0.7071, C = 0.5, 1.5, 2.5, 3.2071; u S = 1.6036 is first exceeded at id 2, u S = 1.4432 at id 1
    assert R.exact_token(x[0], 0.5, "random", T=2.0) == 2 and R.exact_token(x[0], 0.45, "random", T=2.0) == 1
    # -inf weighs nothing: u = 0 gives the first id with a weight
    assert R.exact_token(x[1], 0.0, "random") == 1
    assert R.accepted_tokens(x, [0.0, 0.0], "random") == [{0}, {0, 1}]      # the empty interval of id 0 touches u S = 0: tolerated by the oracle
    assert R.accepted_tokens(x, [U_LAST, U_LAST], "random") == [{3}, {3}]


def test_non_finite_rows():
    inf, nan = float("inf"), float("nan")
    x = torch.tensor([[-inf] * 4, [1.0, nan, 5.0, nan], [1.0, inf, inf, 0.0], [nan, inf, 1.0, 1.0]], dtype=torch.float64)
    for mode, kw in (("random", {}), ("top_k", {"k": 2}), ("top_p", {"p": 0.5})):
        assert R.accepted_tokens(x, [0.7] * 4, mode, **kw) == [{0}, {1}, {1}, {0}]
        assert [R.exact_token(x[b], 0.7, mode, **kw) for b in range(4)] == [0, 1, 1, 0]


def test_sampler_constructors_and_configs():
    from iseg_amd.nlp import samplers as S

    assert S.Sampler().get_config() == {"temperature": 1.0}
    assert S.GreedySampler(temperature=0.5).get_config() == {"temperature": 0.5}
    assert S.RandomSampler().get_config() == {"temperature": 1.0, "seed": None}
    assert S.TopKSampler().get_config() == {"temperature": 1.0, "seed": None, "k": 5}
    assert S.TopPSampler().get_config() == {"temperature": 1.0, "seed": None, "p": 0.1, "k": None}
    cfg = S.TopPSampler(p=0.9, k=40, seed=3, temperature=0.7).get_config()
    assert cfg == {"temperature": 0.7, "seed": 3, "p": 0.9, "k": 40}
    assert S.TopPSampler.from_config(cfg).get_config() == cfg
    assert S.TopKSampler.from_config(S.TopKSampler(k=2, seed=1).get_config()).k == 2
    for bad in (lambda: S.Sampler(temperature=0.0), lambda: S.RandomSampler(temperature=-1.0), lambda: S.GreedySampler(temperature=float("inf")),
                lambda: S.TopKSampler(k=0), lambda: S.TopKSampler(k=2.5), lambda: S.TopPSampler(p=0.0), lambda: S.TopPSampler(p=1.5),
                lambda: S.TopPSampler(k=0), lambda: S.RandomSampler(seed="x"), lambda: S.TopKSampler(temperature=float("nan"))):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(NotImplementedError):
        S.Sampler().get_next_token(torch.zeros(1, 3))
    assert S.GreedySampler().get_next_token(torch.tensor([[0.0, 2.0, 2.0], [3.0, 1.0, 0.0]])).tolist() == [1, 0]


def test_compile_takes_instances_and_greedy():
    from iseg_amd.nlp import samplers as S
    from iseg_amd.nlp.gemma import GemmaBackbone, GemmaCausalLM

    model = GemmaCausalLM(GemmaBackbone(**TINY))
    assert model.sampler == "greedy"
    for sampler in (S.TopKSampler(k=3, seed=1), S.TopPSampler(p=0.5), S.RandomSampler(), S.GreedySampler()):
        model.compile(sampler=sampler)
        assert model.sampler is sampler
    model.compile(sampler="greedy")
    assert model.sampler == "greedy"
    with pytest.raises(NotImplementedError, match="TopKSampler"):
        model.compile(sampler="top_k")
    with pytest.raises(ValueError):
        model.compile(sampler=5)


def test_symbols_are_declared_exported_and_bound():
    from iseg_amd import _hip, build
    from iseg_amd import functional as F
    from iseg_amd import kernels as K

    names = ("iseg_token_sample_supported", "iseg_token_sample_splits", "iseg_token_sample_scratch_bytes", "iseg_token_sample")
    header = open(os.path.join(ROOT, "include", "iseg_hip.h")).read()
    L = _hip.lib()
    for name in names:
        assert name in _hip.SIGNATURES and name + "(" in header and hasattr(L, name)
    for macro, value in (("ISEG_SAMPLE_RANDOM", _hip.SAMPLE_RANDOM), ("ISEG_SAMPLE_TOP_K", _hip.SAMPLE_TOP_K), ("ISEG_SAMPLE_TOP_P", _hip.SAMPLE_TOP_P)):
        assert f"#define {macro} {value}" in header
    assert "token_sample.hip" in build.SOURCES
    for mod, fns in ((K, ("token_sample_supported", "token_sample_splits", "token_sample")), (F, ("sample_tokens",))):
        for fn in fns:
            assert callable(getattr(mod, fn))


def test_plan_and_scratch_are_functions_of_their_arguments():
    from iseg_amd import _hip

    L = _hip.lib()
    RANDOM, TOP_K, TOP_P = _hip.SAMPLE_RANDOM, _hip.SAMPLE_TOP_K, _hip.SAMPLE_TOP_P
    head, hist = 16, 256 * 4 + 256 * 8
    assert L.iseg_token_sample_splits(1, 256000) > 1 and L.iseg_token_sample_splits(1, 256000) == L.iseg_token_sample_splits(1, 256000)
    assert L.iseg_token_sample_splits(1, 1) == 1 and L.iseg_token_sample_splits(1, 2048) == 1 and L.iseg_token_sample_splits(3, 4099) == 1
    assert L.iseg_token_sample_splits(64, 256000) < L.iseg_token_sample_splits(1, 256000)      # many rows already cover the chip
    assert L.iseg_token_sample_splits(1, 256000) * 2 <= -(-256000 // 2048)      # at least two tiles per chunk
    assert L.iseg_token_sample_splits(0, 100) == 0 and L.iseg_token_sample_splits(1, 0) == 0 and L.iseg_token_sample_splits(1, (1 << 20) + 1) == 0
    assert L.iseg_token_sample_scratch_bytes(3, 70001, TOP_K, 5, 2) == 3 * 2 * (head + hist)
    assert L.iseg_token_sample_scratch_bytes(3, 70001, TOP_P, 0, 2) == 3 * 2 * (head + hist)
    assert L.iseg_token_sample_scratch_bytes(3, 70001, RANDOM, 0, 2) == 3 * 2 * head
    tiles = -(-70001 // 2048)
    assert L.iseg_token_sample_scratch_bytes(3, 70001, TOP_K, 5, 10 ** 6) == 3 * tiles * (head + hist)      # clipped to the tiles that hold an element
    assert L.iseg_token_sample_scratch_bytes(3, 70001, TOP_K, 5, 0) == 3 * L.iseg_token_sample_splits(3, 70001) * (head + hist)
    sizes = [L.iseg_token_sample_scratch_bytes(1, 70001, TOP_K, 5, s) for s in (1, 2, 3, tiles)]
    assert sizes == sorted(sizes) and len(set(sizes)) == 4
    assert L.iseg_token_sample_scratch_bytes(1, 70001, TOP_K, 0, 1) == 0 and L.iseg_token_sample_scratch_bytes(1, 0, RANDOM, 0, 1) == 0


def test_the_support_set():
    from iseg_amd import _hip
    from iseg_amd import kernels as K

    L = _hip.lib()
    RANDOM, TOP_K, TOP_P = _hip.SAMPLE_RANDOM, _hip.SAMPLE_TOP_K, _hip.SAMPLE_TOP_P
    for dtype in (_hip.BF16, _hip.F32):
        for V in (1, 2, 256000, 1 << 20):
            assert L.iseg_token_sample_supported(V, RANDOM, 0, dtype) == 1 and L.iseg_token_sample_supported(V, TOP_K, 1, dtype) == 1
            assert L.iseg_token_sample_supported(V, TOP_K, V + 3, dtype) == 1 and L.iseg_token_sample_supported(V, TOP_P, 0, dtype) == 1
            assert L.iseg_token_sample_supported(V, TOP_P, 40, dtype) == 1
        assert L.iseg_token_sample_supported(0, RANDOM, 0, dtype) == 0 and L.iseg_token_sample_supported((1 << 20) + 1, TOP_K, 5, dtype) == 0
        assert L.iseg_token_sample_supported(100, TOP_K, 0, dtype) == 0 and L.iseg_token_sample_supported(100, TOP_P, -1, dtype) == 0
        assert L.iseg_token_sample_supported(100, 3, 1, dtype) == 0 and L.iseg_token_sample_supported(100, -1, 1, dtype) == 0
    assert L.iseg_token_sample_supported(100, TOP_K, 5, 2) == 0
    assert K.token_sample_supported(100, TOP_K, 5, torch.bfloat16) and K.token_sample_supported(100, TOP_K, 5, torch.float32)
    assert not K.token_sample_supported(100, TOP_K, 5, torch.float16) and not K.token_sample_supported(100, TOP_K, 0, torch.float32)


def test_the_launcher_refuses_before_touching_memory():
    """host buffers stand in for device pointers: every call below must return before a launch"""
    from iseg_amd import _hip

    L = _hip.lib()
    TOP_K, TOP_P = _hip.SAMPLE_TOP_K, _hip.SAMPLE_TOP_P
    ARG, UNSUPPORTED, WORKSPACE = -1, -3, -4
    buf = ctypes.create_string_buffer(1 << 16)
    a = ctypes.addressof(buf)
    need = L.iseg_token_sample_scratch_bytes(2, 100, TOP_K, 5, 0)
    assert 0 < need <= 1 << 15

    def call(ld=100, V=100, mode=TOP_K, k=5, p=1.0, T=1.0, dtype=_hip.BF16, ws_bytes=need, logits=a):
        return L.iseg_token_sample(logits, ld, a + 4096, a + 8192, a + (1 << 15), ws_bytes, 2, V, mode, k, p, T, 0, dtype, None)

    for T in (0.0, -1.0, float("inf"), float("nan")):
        assert call(T=T) == ARG and "temperature" in _hip.last_error()
    for p in (0.0, -0.5, 1.5, float("nan")):
        assert call(mode=TOP_P, p=p) == ARG and "p must" in _hip.last_error()
    assert call(ld=99) == ARG and "pitch" in _hip.last_error()
    assert call(ws_bytes=need - 1) == WORKSPACE and str(need) in _hip.last_error()
    assert call(V=0) == UNSUPPORTED and call(V=(1 << 20) + 1, ld=1 << 21) == UNSUPPORTED
    assert call(k=0) == UNSUPPORTED and call(k=-1, mode=TOP_P) == UNSUPPORTED and call(mode=7) == UNSUPPORTED
    assert call(dtype=2) == UNSUPPORTED
    assert call(logits=None) == ARG


def test_functional_refuses_by_naming_the_limit():
    from iseg_amd import functional as F

    x, u = torch.zeros(2, 10), torch.zeros(2)
    for kw, word in (({"mode": "beam"}, "mode"), ({"mode": "top_k", "k": 0}, "k >= 1"), ({"mode": "top_p", "p": 0.0}, "p must"),
                     ({"mode": "random", "temperature": 0.0}, "temperature"), ({"mode": "top_p", "k": -1}, "k >= 0")):
        with pytest.raises(ValueError, match=word):
            F.sample_tokens(x, u, **kw)
    with pytest.raises(ValueError, match="vocabulary"):
        F.sample_tokens(torch.zeros(1, (1 << 20) + 1), torch.zeros(1), mode="random")
    with pytest.raises(ValueError, match="bfloat16 or float32"):
        F.sample_tokens(x.to(torch.float16), u, mode="random")
    with pytest.raises(ValueError, match=r"\[B\]"):
        F.sample_tokens(x, torch.zeros(3), mode="random")
    with pytest.raises(RuntimeError, match="inference only"):
        F.sample_tokens(x.clone().requires_grad_(), u, mode="random")


def test_functional_dry_run_shape():
    from iseg_amd import functional as F
    from iseg_amd import nn

    with nn.dry_run_scope():
        out = F.sample_tokens(torch.zeros(3, 1, 50), torch.zeros(3), mode="top_k", k=5)
    assert tuple(out.shape) == (3,) and out.dtype == torch.int32


def _stub(script):
    """a `next` whose logits at step `index` put script[index][row] on top; records the indices it was asked for"""
    seen = []

    def next(prompt, cache, index):
        seen.append(index)
        logits = torch.zeros(prompt.shape[0], 11)
        for b, tok in enumerate(script[index]):
            logits[b, tok] = 1.0
        return logits, None, cache

    return next, seen


def test_the_sampler_loop_on_a_stub():
    """the stub pattern of test_gemma_cache_host.py with a get_next_token of the test's own: user tokens are kept, the loop stops once every row
    holds a generated end token, the caller's prompt is not written, and get_next_token sees each step's [B, V] logits once"""
    from iseg_amd.nlp.samplers import Sampler

    class Second(Sampler):
        """the runner-up by index: (argmax + 1) mod V"""

        def __init__(self):
            super().__init__()
            self.calls = 0

        def get_next_token(self, logits):
            assert tuple(logits.shape) == (2, 11)
            self.calls += 1
            return (torch.argmax(logits, dim=-1) + 1) % 11

    prompt = torch.tensor([[1, 2, 0, 0, 0, 0, 0, 0], [3, 4, 5, 9, 0, 0, 0, 0]])
    mask = torch.tensor([[1, 1, 0, 0, 0, 0, 0, 0], [1, 1, 1, 1, 0, 0, 0, 0]], dtype=torch.bool)
    script = {2: (6, 6), 3: (8, 6), 4: (5, 7), 5: (5, 7), 6: (4, 8), 7: (0, 0)}      # the tokens of the greedy test, each minus one
    nxt, seen = _stub(script)
    sampler = Second()
    out = sampler(nxt, prompt, None, 2, mask, end_token_id=9)
    assert seen == [2, 3, 4, 5, 6] and sampler.calls == 5
    assert out.tolist() == [[1, 2, 7, 9, 6, 6, 5, 0], [3, 4, 5, 9, 8, 8, 9, 0]]
    assert prompt[0, 2].item() == 0 and out.dtype == prompt.dtype
    nxt, seen = _stub(script)
    out = Second()(nxt, prompt, index=2, mask=mask)
    assert seen == [2, 3, 4, 5, 6, 7] and out[:, 7].tolist() == [1, 1]
    # no mask: nothing is a user token, generation starts at index 0
    nxt, seen = _stub({i: (i, i + 1) for i in range(3)})
    assert Second()(nxt, torch.zeros(2, 3, dtype=torch.int64)).tolist() == [[1, 2, 3], [2, 3, 4]]


def test_greedy_sample_still_runs_the_shared_loop():
    from iseg_amd.nlp.gemma.gemma_causal import greedy_sample
    from iseg_amd.nlp.samplers import GreedySampler

    prompt = torch.tensor([[1, 2, 0, 0, 0, 0, 0, 0], [3, 4, 5, 9, 0, 0, 0, 0]])
    mask = torch.tensor([[1, 1, 0, 0, 0, 0, 0, 0], [1, 1, 1, 1, 0, 0, 0, 0]], dtype=torch.bool)
    script = {2: (7, 7), 3: (9, 7), 4: (6, 8), 5: (6, 8), 6: (5, 9), 7: (1, 1)}
    a = greedy_sample(_stub(script)[0], prompt, None, 2, mask, end_token_id=9)
    b = GreedySampler()(_stub(script)[0], prompt, None, 2, mask, end_token_id=9)
    assert torch.equal(a, b) and a.tolist() == [[1, 2, 7, 9, 6, 6, 5, 0], [3, 4, 5, 9, 8, 8, 9, 0]]


def test_a_seeded_sampler_draws_the_same_uniforms_again():
    from iseg_amd.nlp.samplers import RandomSampler, TopKSampler

    x = torch.zeros(4, 7)
    a, b, c = TopKSampler(k=3, seed=7), TopKSampler(k=3, seed=7), RandomSampler(seed=8)
    ua = [a.uniforms(x) for _ in range(3)]
    ub = [b.uniforms(x) for _ in range(3)]
    assert all(torch.equal(p, q) for p, q in zip(ua, ub)) and not torch.equal(ua[0], ua[1]) and not torch.equal(ua[0], c.uniforms(x))
    assert ua[0].dtype == torch.float32 and tuple(ua[0].shape) == (4,) and bool(((ua[0] >= 0) & (ua[0] < 1)).all())
    assert not torch.equal(TopKSampler(k=3).uniforms(x), TopKSampler(k=3).uniforms(x))      # unseeded: the library's seed stream moves on
