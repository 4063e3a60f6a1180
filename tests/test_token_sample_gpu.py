"""The fused token samplers on the GPU (csrc/token_sample.hip through F.sample_tokens and iseg_amd.nlp.samplers) against the fp64 oracle of
tests/token_sample_ref.py.  Every returned token must lie in accepted_tokens (eps = 1e-5: inputs are exact, x / T and expf cost at most
0.37 * 2 * 2^-24 of mass, a tree or fixed-point sum over V <= 2^20 at most 20 * 2^-24; 1e-5 is about five times the total; the kernel's
exp2 on v_exp_f32 moves a row's mass by at most 2.6e-6, csrc/token_sample.hip derives it); a top-k token must also lie in the oracle's exact
kept set, with no tolerance; an id of weight zero never comes back."""
import numpy as np
import pytest
import torch

from tests import guarded_memory as GM
from tests import token_sample_ref as R
from tests.test_gemma_cache_gpu import B as MB
from tests.test_gemma_cache_gpu import PROMPTS, S as MS
from tests.test_gemma_cache_gpu import _model, _prompts, bf16  # noqa: F401  (bf16 is a fixture)

pytestmark = pytest.mark.gpu

EPS = 1e-5
TILE = 2048
U_LAST = float(np.nextafter(np.float32(1), np.float32(0)))
VS = [1, 2, 63, 64, 65, 257, 4099, 70001]
BS = [1, 3, 17]
TS = [0.25, 1.0, 4.0]
FAMILIES = ["gaussian", "four_levels", "one_far_above", "third_masked"]
U_KINDS = ["random", "zero", "last"]


def _configs(V):
    """(mode, k, p): every k of the top-k list, every p of the top-p list without a k and with one, and the random sampler"""
    out = [("top_k", k, 1.0) for k in (1, 5, 64, V, V + 3)]
    out += [("top_p", 0, p) for p in (1e-6, 0.1, 0.9, 1.0)]
    out += [("top_p", k, p) for k, p in ((5, 1e-6), (64, 0.1), (5, 0.9), (64, 1.0))]
    return out + [("random", 0, 1.0)]


def _rows(B, V, dtype, gen, first_family):
    """row b is of family (first_family + b) mod 4, rounded to dtype: the oracle reads the stored values"""
    x = torch.empty(B, V, dtype=torch.float32)
    for b in range(B):
        fam = FAMILIES[(first_family + b) % len(FAMILIES)]
        if fam == "gaussian":
            x[b] = 2.0 * torch.randn(V, generator=gen)
        elif fam == "four_levels":      # heavy ties across the k-th position and across chunk borders
            x[b] = torch.tensor([-1.0, 0.0, 0.5, 2.0])[torch.randint(0, 4, (V,), generator=gen)]
        elif fam == "one_far_above":      # the other weights underflow (T <= 1) or nearly do
            x[b] = torch.randn(V, generator=gen)
            x[b, int(torch.randint(0, V, (1,), generator=gen))] += 80.0
        else:
            x[b] = 2.0 * torch.randn(V, generator=gen)
            x[b, torch.rand(V, generator=gen) < 1.0 / 3.0] = -float("inf")
            x[b, int(torch.randint(0, V, (1,), generator=gen))] = 0.5      # never all masked
    return x.to(dtype)


def _uniforms(B, gen, first_kind):
    u = torch.rand(B, generator=gen, dtype=torch.float32)
    for b in range(B):
        kind = U_KINDS[(first_kind + b) % len(U_KINDS)]
        if kind != "random":
            u[b] = 0.0 if kind == "zero" else U_LAST
    return u


def _pitched(x, ld, device):
    """the rows of x inside a [B, ld] buffer whose other columns hold NaN: a kernel that reads past column V sees a NaN on top"""
    B, V = x.shape
    full = torch.full((B, ld), float("nan"), dtype=x.dtype, device=device)
    full[:, :V] = x.to(device)
    return full[:, :V]


def _check(x, u, tokens, mode, k, p, T, note):
    tokens = tokens.cpu()
    assert tokens.dtype == torch.int32 and tuple(tokens.shape) == (x.shape[0],)
    assert bool(((tokens >= 0) & (tokens < x.shape[1])).all()), (note, tokens.tolist())
    accepted = R.accepted_tokens(x, u, mode, k=k, p=p, T=T, eps=EPS, candidates=tokens)
    x64 = x.double()
    for b, tok in enumerate(tokens.tolist()):
        assert tok in accepted[b], (note, b, tok, R.exact_token(x[b], float(u[b]), mode, k=k, p=p, T=T))
        if mode == "top_k":
            assert tok in R.kept_set(x[b], "top_k", k=k), (note, b, tok)
        row = x64[b]
        if bool(torch.isfinite(row.max())) and not bool(torch.isnan(row).any()):
            assert R.weights(row.numpy(), T)[tok] > 0.0, (note, b, tok)      # -inf and underflowed ids are never drawn


def _ld(V, pitch):
    return {"tight": V, "plus24": V + 24, "aligned": (V + 7) // 8 * 8 + 8}[pitch]


@pytest.mark.parametrize("pitch", ["tight", "plus24", "aligned"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("V", VS)
def test_kernel_against_the_oracle(cuda, V, dtype, pitch):
    """every (mode, k, p) of _configs at this V, dtype and pitch ("aligned": a pitch of whole 16-byte groups, so that the 128-bit loads meet a
    ragged tail); batch size, temperature, splits, the first row's logit family and the first row's kind of u rotate with the configuration and
    the case, so that over the cases every value meets every V.  Rows of a batch are of successive families and successive kinds of u."""
    from iseg_amd import functional as F

    case = VS.index(V) * 7 + (dtype == torch.float32) * 3 + ["tight", "plus24", "aligned"].index(pitch)
    gen = torch.Generator().manual_seed(1000 + case)
    tiles = -(-V // TILE)
    big = V > 10000
    for i, (mode, k, p) in enumerate(_configs(V)):
        j = i + case
        Bn = BS[j % 3]
        if big and Bn == 17 and i % 4:      # the CPU oracle at 70001 entries: seventeen rows for every fourth configuration, three otherwise
            Bn = 3
        T, splits = TS[(j // 3) % 3], [0, 1, 2, tiles][j % 4]
        x = _rows(Bn, V, dtype, gen, (j // 3) % 4)
        u = _uniforms(Bn, gen, (j // 2) % 3)
        got = F.sample_tokens(_pitched(x, _ld(V, pitch), cuda), u.to(cuda), mode=mode, k=k, p=p, temperature=T, splits=splits)
        _check(x, u, got, mode, k, p, T, (V, mode, k, p, T, splits, Bn))


def test_a_quarter_million_entries(cuda):
    """V = 262144, B = 2, bf16: the chunk plan, one chunk and the most chunks"""
    from iseg_amd import functional as F

    V, gen = 262144, torch.Generator().manual_seed(5)
    x = _rows(2, V, torch.bfloat16, gen, 0)
    xd = x.to(cuda)
    for i, (mode, k, p, T, splits) in enumerate((("top_k", 5, 1.0, 1.0, 0), ("top_k", V, 1.0, 4.0, 1), ("top_p", 0, 0.9, 1.0, V // TILE),
                                                 ("top_p", 64, 0.1, 0.25, 0), ("random", 0, 1.0, 1.0, 2))):
        u = _uniforms(2, gen, i)
        _check(x, u, F.sample_tokens(xd, u.to(cuda), mode=mode, k=k, p=p, temperature=T, splits=splits), mode, k, p, T, (V, mode, k, p, T, splits))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_rows_with_a_non_finite_top(cuda, dtype):
    """a NaN on top (also behind a +inf), +inf on top twice, an all -inf row, beside an ordinary row: the lowest index holding the top value,
    whatever u says; several chunks at 4099 and 70001"""
    from iseg_amd import functional as F

    inf, nan = float("inf"), float("nan")
    for V in (1, 65, 4099, 70001):
        gen = torch.Generator().manual_seed(V)
        x = _rows(5, V, dtype, gen, 0).float()
        a, b = V // 3, (2 * V) // 3
        x[0, b] = nan
        x[0, a] = inf
        x[1, b], x[1, a] = inf, inf
        x[2, :] = -inf
        x[3, b] = nan
        if V > 1:
            x[3, V - 1] = nan
        x = x.to(dtype)
        want = [b, a, 0, b]
        for mode, k, p in (("random", 0, 1.0), ("top_k", 5, 1.0), ("top_p", 0, 0.9)):
            for splits in (0, 1, -(-V // TILE)):
                u = _uniforms(5, gen, splits % 3)
                got = F.sample_tokens(x.to(cuda), u.to(cuda), mode=mode, k=k, p=p, splits=splits)
                assert got[:4].tolist() == want, (V, mode, splits, got.tolist())
                _check(x, u, got, mode, k, p, 1.0, (V, mode, splits))


def test_the_three_dimensional_view(cuda):
    """[B, 1, V] as call_with_cache's logits sliced out of [B, Tn, V]: the pitch is the view's"""
    from iseg_amd import functional as F

    gen = torch.Generator().manual_seed(9)
    x = _rows(3, 257, torch.bfloat16, gen, 0)
    u = _uniforms(3, gen, 0)
    full = torch.full((3, 2, 257), float("nan"), dtype=torch.bfloat16, device=cuda)
    full[:, 1] = x.to(cuda)
    got = F.sample_tokens(full[:, 1:2], u.to(cuda), mode="top_k", k=5)
    _check(x, u, got, "top_k", 5, 1.0, 1.0, "view")
    assert torch.equal(got, F.sample_tokens(x.to(cuda), u.to(cuda), mode="top_k", k=5))


def test_a_second_call_returns_the_same_tokens(cuda):
    from iseg_amd import functional as F
    from iseg_amd import kernels as K

    V, gen = 70001, torch.Generator().manual_seed(11)
    assert K.token_sample_splits(17, V) > 1
    for dtype in (torch.bfloat16, torch.float32):
        x = _rows(17, V, dtype, gen, 0).to(cuda)
        u = torch.rand(17, generator=gen).to(cuda)
        for mode, k, p in (("random", 0, 1.0), ("top_k", 64, 1.0), ("top_p", 0, 0.9)):
            first = F.sample_tokens(x, u, mode=mode, k=k, p=p, temperature=0.7)
            assert torch.equal(first, F.sample_tokens(x, u, mode=mode, k=k, p=p, temperature=0.7))


def test_inside_guard_bands(cuda):
    """logits, u, the tokens and a scratch buffer of EXACTLY iseg_token_sample_scratch_bytes between bands of poison (tests/guarded_memory.py):
    the bands are intact after the call, the scratch buffer was asked for, and the tokens are the unguarded call's (no poison reached them)"""
    from iseg_amd import kernels as K

    modes = {"random": K.SAMPLE_RANDOM, "top_k": K.SAMPLE_TOP_K, "top_p": K.SAMPLE_TOP_P}
    for Bn, V, dtype, mode, k, p, splits in ((3, 4099, torch.bfloat16, "top_k", 5, 1.0, 0), (2, 70001, torch.bfloat16, "top_p", 0, 0.9, 0),
                                             (3, 257, torch.float32, "random", 0, 1.0, 0), (1, 70001, torch.float32, "top_k", 64, 1.0, 35),
                                             (2, 4104, torch.bfloat16, "top_p", 64, 0.1, 2)):
        gen = torch.Generator().manual_seed(V + Bn)
        x = _rows(Bn, V, dtype, gen, 0)
        u = _uniforms(Bn, gen, 0)
        plain = K.token_sample(x.to(cuda), u.to(cuda), modes[mode], k, p, 1.0, splits)
        arena = GM.Arena(cuda, 16 << 20)
        with GM.guarded(arena):
            xd = arena.alloc(x.shape, x.dtype, "operand")
            ud = arena.alloc(u.shape, u.dtype, "operand")
            xd.copy_(x)
            ud.copy_(u)
            got = K.token_sample(xd, ud, modes[mode], k, p, 1.0, splits)
            arena.check()
            roles = [r.role for r in arena.records]
            assert roles.count("workspace") == 1 and roles.count("output") == 1
            ws = [r for r in arena.records if r.role == "workspace"][0]
            assert ws.end - ws.start == K._hip.lib().iseg_token_sample_scratch_bytes(Bn, V, modes[mode], k, splits)
            assert 0 <= arena.offset_of(got) < arena.nbytes
        assert torch.equal(got.cpu(), plain.cpu())
        _check(x, u, got, mode, k, p, 1.0, ("guarded", V, mode))


# ---- the model ---------------------------------------------------------------------------------------------------------------------------------
def _inputs(cuda):
    ids, mask = _prompts()
    ids = ids * mask
    return ids, mask, {"token_ids": ids.to(cuda), "padding_mask": mask.to(cuda)}


def test_one_kept_token_is_greedy(cuda, bf16):  # noqa: F811
    """TopKSampler(k=1) and TopPSampler(p=1e-6) keep the first of the order alone: generate_step's output is the greedy one's, token for token"""
    from iseg_amd.nlp.samplers import GreedySampler, TopKSampler, TopPSampler

    model, _ = _model(torch.bfloat16)
    ids, mask, inputs = _inputs(cuda)
    model.compile(sampler="greedy")
    want = model.generate_step(inputs)
    end = int(want["token_ids"][0, PROMPTS[0] + 2].item())
    want_end = model.generate_step(inputs, end_token_id=end)
    for sampler in (TopKSampler(k=1, seed=3), TopPSampler(p=1e-6, seed=4), TopPSampler(p=1e-6, k=7, temperature=0.5), GreedySampler()):
        model.compile(sampler=sampler)
        for ref, e in ((want, None), (want_end, end)):
            got = model.generate_step(inputs, end_token_id=e)
            assert torch.equal(got["token_ids"], ref["token_ids"]) and torch.equal(got["padding_mask"], ref["padding_mask"]), type(sampler).__name__


@pytest.mark.parametrize("with_end", [False, True], ids=["no_end_token", "end_token"])
def test_top_k_generation(cuda, bf16, with_end):  # noqa: F811
    """TopKSampler(k=5, seed=7): the same seed gives the same tokens, another seed other ones somewhere; every generated token lies in the exact
    top five of the logits row that call_with_cache returned for its step (recorded by a wrapper), user tokens are kept, and with an end token
    (the third token row 0 generates in the free run) the loop stops where the sampler's condition says"""
    from iseg_amd.nlp.samplers import TopKSampler

    model, _ = _model(torch.bfloat16)
    ids, mask, inputs = _inputs(cuda)
    recorded = {}
    inner = model.call_with_cache

    def recording(token_ids, cache, cache_update_index):
        logits, hidden, cache = inner(token_ids, cache, cache_update_index)
        if token_ids.shape[1] == 1:
            recorded[cache_update_index + 1] = logits[:, 0].cpu()
        return logits, hidden, cache

    model.call_with_cache = recording
    end = None
    if with_end:
        model.compile(sampler=TopKSampler(k=5, seed=7))
        end = int(model.generate_step(inputs)["token_ids"][0, PROMPTS[0] + 2].item())
    model.compile(sampler=TopKSampler(k=5, seed=7))
    recorded.clear()
    result = model.generate_step(inputs, end_token_id=end)
    out, out_mask = result["token_ids"].cpu(), result["padding_mask"].cpu()
    steps = dict(recorded)
    assert torch.equal(inputs["token_ids"].cpu(), ids) and torch.equal(out[mask], ids[mask])
    stopped = MS
    for i in range(PROMPTS[0], MS):
        state = torch.cat([out[:, :i], ids[:, i:]], dim=1)
        if end is not None and bool(((state == end) & ~mask).any(dim=-1).all()):
            stopped = i
            break
        for b in range(MB):
            if not mask[b, i]:
                assert int(out[b, i]) in R.kept_set(steps[i][b], "top_k", k=5), (i, b)
    assert sorted(steps) == list(range(PROMPTS[0], stopped))
    assert torch.equal(out[:, stopped:], ids[:, stopped:])
    if end is None:
        assert out_mask.all()
    else:
        assert bool(((out == end) & ~mask).any())
    model.compile(sampler=TopKSampler(k=5, seed=7))
    again = model.generate_step(inputs, end_token_id=end)
    assert torch.equal(again["token_ids"].cpu(), out) and torch.equal(again["padding_mask"].cpu(), out_mask)
    model.compile(sampler=TopKSampler(k=5, seed=8))
    other = model.generate_step(inputs, end_token_id=end)["token_ids"].cpu()
    assert torch.equal(other[mask], ids[mask]) and not torch.equal(other, out)
