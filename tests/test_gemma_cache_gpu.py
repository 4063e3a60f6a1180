"""Gemma with a key/value cache on the device (csrc/gemma_decode.hip, F.gemma_rope_cache / gemma_cached_attention_core / embedding_logits,
nlp/gemma/gemma_causal.py) against the fp64 restatement in tests/gemma_cache_ref.py: the decode core on both routes (split-KV kernels, and
ISEG_GEMMA_FUSED=0: the composed route), the rotary embedding into the cache, the refusals and the guard bands of the C entry points, the model
teacher-forced through the cache, greedy generation and score()."""
import os

import pytest
import torch

from tests import gemma_cache_ref as C
from tests import guarded_memory as GM
from tests.test_gemma_cache_host import tiny_weights
from tests.test_gemma_gpu import CFG
from tests.test_kernels_gpu import DTYPES, rnd

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -3, -4

# (B, S, pos0, Tn, nq, nkv, h, splits): one key; an exact tile; one key in the second tile, two kv heads, two slabs; the 2B head layout with a
# cache longer than what is visible; ungrouped heads; sixteen stacked rows with the causal step inside the chunk at a tile edge; a long cache
# (the plan must cut it); three forced chunks of which the third holds one key that only the second token sees
CASES = [(2, 1, 0, 1, 1, 1, 64, 0), (1, 64, 63, 1, 2, 1, 64, 0), (2, 65, 64, 1, 4, 2, 128, 0), (1, 300, 129, 1, 8, 1, 256, 0),
         (1, 200, 196, 1, 16, 16, 64, 0), (2, 130, 63, 2, 8, 1, 256, 0), (1, 4096, 4000, 1, 8, 1, 256, 0), (1, 192, 127, 2, 8, 1, 256, 3)]


def _rel(a, b):
    return (a - b).norm().item() / max(b.norm().item(), 1e-300)


@pytest.fixture
def bf16():
    from iseg_amd import nn

    nn.set_compute_dtype(torch.bfloat16)
    nn.set_device("cuda:0")
    try:
        yield
    finally:
        os.environ.pop("ISEG_GEMMA_FUSED", None)
        nn.set_compute_dtype(torch.float32)


def _core_case(case):
    """bf16-rounded q and cache ~ N(0, 1) (scores h^-0.5 q.k of standard deviation 1); the device cache holds NaN in every row past the last
    visible key, the restatement's zeros; -> (q, device cache, fp64 output)"""
    B, S, pos0, Tn, nq, nkv, h, _ = case
    q = rnd((B, Tn, nq * h), 1).to(torch.bfloat16)
    cache = rnd((B, 2, S, nkv, h), 2).to(torch.bfloat16)
    nvis = pos0 + Tn
    clean = cache.double()
    clean[:, :, nvis:] = 0
    want = C.cached_attention_core(q.double().reshape(B, Tn, nq, h), clean[:, 0], clean[:, 1], pos0, nq, nkv)
    cache[:, :, nvis:] = float("nan")
    return q, cache, want


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


@pytest.mark.parametrize("case", CASES, ids=["x".join(map(str, c)) for c in CASES])
def test_decode_core_both_routes_against_fp64(cuda, bf16, case):
    """the bound of tests/test_gemma_gpu.py::test_core_both_routes_against_fp64: relative Frobenius error 1.5e-2 on the output, fp64 the yardstick
    of both routes.  Also: everything finite although the cache past the last visible key is NaN, the cache itself is not written, a second fused
    run is bit-identical; forced chunks agree with one chunk to the same bound; the long cache is cut by the plan"""
    from iseg_amd import functional as F
    from iseg_amd import kernels as K

    B, S, pos0, Tn, nq, nkv, h, splits = case
    q, cache, want = _core_case(case)
    qd, cd = q.cuda(), cache.cuda()
    before = _bits(cd).clone()
    if S == 4096:
        assert K.gemma_decode_attention_splits(B, pos0, Tn, nq, nkv, h) > 1
    out = {}
    for mode in ("1", "0"):
        os.environ["ISEG_GEMMA_FUSED"] = mode
        assert F.gemma_cached_attention_fused(Tn, nq, nkv, h, torch.bfloat16) == (mode == "1")
        y = F.gemma_cached_attention_core(qd, cd, pos0, nq, nkv, h, splits=splits)
        assert y.dtype == torch.bfloat16 and tuple(y.shape) == (B, Tn, nq * h) and y.grad_fn is None
        out[mode] = y.cpu().double()
        print(f"mode {mode} out rel {_rel(out[mode], want):.3e}")
    for mode in ("1", "0"):
        assert torch.isfinite(out[mode]).all(), mode
        assert _rel(out[mode], want) < 1.5e-2, mode
    assert torch.equal(_bits(cd), before)
    os.environ["ISEG_GEMMA_FUSED"] = "1"
    again = F.gemma_cached_attention_core(qd, cd, pos0, nq, nkv, h, splits=splits).cpu().double()
    assert torch.equal(again, out["1"])
    if splits:
        one = F.gemma_cached_attention_core(qd, cd, pos0, nq, nkv, h, splits=1).cpu().double()
        print(f"splits 1 out rel {_rel(one, want):.3e}, against splits {splits} {_rel(one, out['1']):.3e}")
        assert torch.isfinite(one).all() and _rel(one, want) < 1.5e-2 and _rel(one, out["1"]) < 1.5e-2


def test_cached_path_refuses_inputs_that_require_grad(cuda, bf16):
    from iseg_amd import functional as F

    q = torch.zeros(1, 1, 64, dtype=torch.bfloat16, device="cuda", requires_grad=True)
    cache = torch.zeros(1, 2, 4, 1, 64, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError, match="inference only"):
        F.gemma_cached_attention_core(q, cache, 0, 1, 1, 64)
    qkv = torch.zeros(1, 1, 192, dtype=torch.bfloat16, device="cuda", requires_grad=True)
    with pytest.raises(RuntimeError, match="inference only"):
        F.gemma_rope_cache(qkv, cache, 0, 1, 1, 64)


# ---- rotary embedding into the cache ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_rope_cache_at_position_300(cuda, dtype):
    """three new tokens at positions 300 .. 302 of a cache of 310 rows, where bf16 angles could not tell positions apart.  q and the cache's new key
    rows against the restatement within one rounding of the storage type (2^-8 |y| for bf16, 2^-22 for fp32) plus the fp32 table's error (1e-4 of
    the pair's norm), the bound of tests/test_gemma_gpu.py::test_rope_matches_the_restatement_above_position_256; the new value rows are the input's
    bits; every other cache row keeps its poison pattern bit for bit; q and k are the bits of the uncached F.gemma_rope at those positions"""
    from iseg_amd import functional as F
    from iseg_amd import kernels as K
    from iseg_amd import nn

    B, S, pos0, Tn, nq, nkv, h = 2, 310, 300, 3, 2, 1, 64
    nn.set_compute_dtype(dtype)
    try:
        x = rnd((B, Tn, (nq + 2 * nkv) * h), 5).to(dtype)
        cache = torch.empty((B, 2, S, nkv, h), dtype=dtype, device="cuda")
        pattern = 0x7FA5 if dtype == torch.bfloat16 else 0x7FA5A5A5
        _bits(cache).fill_(pattern)
        q = F.gemma_rope_cache(x.cuda(), cache, pos0, nq, nkv, h)
        assert q.dtype == dtype and tuple(q.shape) == (B, Tn, nq * h) and q.grad_fn is None
        want_q, want_cache = C.rope_cache(x.double(), torch.zeros(B, 2, S, nkv, h, dtype=torch.float64), pos0, nq, nkv)
        ulp = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -22

        def check(got, want, src):
            r = (src[..., :h // 2] ** 2 + src[..., h // 2:] ** 2).sqrt()
            r_out = torch.stack([r, r], dim=-1).reshape(src.shape)
            assert ((got - want).abs() <= ulp * want.abs() + 1e-4 * r_out).all(), (got - want).abs().max().item()

        xq = x.double()[..., :nq * h].reshape(B, Tn, nq, h)
        xk = x.double()[..., nq * h:(nq + nkv) * h].reshape(B, Tn, nkv, h)
        check(q.cpu().double().reshape(B, Tn, nq, h), want_q, xq)
        got = cache.cpu()
        check(got[:, 0, pos0:pos0 + Tn].double(), want_cache[:, 0, pos0:pos0 + Tn], xk)
        assert torch.equal(_bits(got[:, 1, pos0:pos0 + Tn].reshape(B, Tn, nkv * h)), _bits(x[..., (nq + nkv) * h:].contiguous()))
        rest = torch.cat([_bits(got)[:, :, :pos0], _bits(got)[:, :, pos0 + Tn:]], dim=2)
        assert (rest == pattern).all()
        assert not torch.equal(got[0, 0, pos0], got[0, 0, pos0 + 1])
        # the same bits as the uncached rotary embedding at rows 300 .. 302 of a sequence of 310
        full = torch.zeros((B, S, (nq + 2 * nkv) * h), dtype=dtype)
        full[:, pos0:pos0 + Tn] = x
        y = K.gemma_rope(full.cuda(), F.gemma_rope_table(S, h, q.device), S, nq, nkv, h, out=torch.empty_like(full.cuda()))[:, pos0:pos0 + Tn].cpu()
        assert torch.equal(_bits(y[..., :nq * h].contiguous()), _bits(q.cpu()))
        assert torch.equal(_bits(y[..., nq * h:(nq + nkv) * h].contiguous()), _bits(got[:, 0, pos0:pos0 + Tn].reshape(B, Tn, nkv * h).contiguous()))
    finally:
        nn.set_compute_dtype(torch.float32)


# ---- refusals and guard bands of the C entry points ----------------------------------------------------------------------------------------------
def _decode_status(q, cache, out, ws, ws_bytes, pos0, Tn, nq, nkv, h, dtype_code, S=None, splits=0):
    from iseg_amd import _hip
    from iseg_amd import kernels as K

    B = cache.shape[0]
    return _hip.lib().iseg_gemma_decode_attention(q.data_ptr(), nq * h, cache[:, 0].data_ptr(), cache.stride(0), cache.stride(2), cache[:, 1].data_ptr(),
                                                  cache.stride(0), cache.stride(2), out.data_ptr(), nq * h, ws.data_ptr(), ws_bytes, B,
                                                  cache.shape[2] if S is None else S, pos0, Tn, nq, nkv, h, float(h) ** -0.5, splits, dtype_code,
                                                  K.stream())


def test_entry_points_refuse_before_memory_is_touched(cuda):
    """(nq / nkv) * Tn = 17, h = 96 and fp32 are ISEG_ERR_UNSUPPORTED; pos0 + Tn > S is ISEG_ERR_ARG from both entry points; a workspace one byte
    short is ISEG_ERR_WORKSPACE; after every refusal the output, the workspace and the cache still hold their poison"""
    from iseg_amd import _hip
    from iseg_amd import kernels as K

    L = _hip.lib()
    n = 17 * 256 * 4
    poison = 0x7FA5

    def buffers():
        ts = [torch.empty(m, dtype=torch.bfloat16, device="cuda") for m in (n, 2 * 2 * 130 * 256)] + [torch.empty(1 << 20, dtype=torch.uint8, device="cuda")]
        _bits(ts[0]).fill_(poison)
        _bits(ts[1]).fill_(poison)
        ts[2].fill_(0xA5)
        return ts

    def untouched(out, cache, ws):
        return bool((_bits(out) == poison).all()) and bool((_bits(cache) == poison).all()) and bool((ws == 0xA5).all())

    q = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
    for (S, pos0, Tn, nq, nkv, h, code, want) in ((8, 3, 1, 17, 1, 64, _hip.BF16, ERR_UNSUPPORTED), (8, 3, 1, 4, 2, 96, _hip.BF16, ERR_UNSUPPORTED),
                                                 (8, 3, 1, 4, 2, 64, _hip.F32, ERR_UNSUPPORTED), (8, 7, 2, 4, 2, 64, _hip.BF16, ERR_ARG),
                                                 (8, -1, 1, 4, 2, 64, _hip.BF16, ERR_ARG)):
        out, flat, ws = buffers()
        cache = flat[:2 * 2 * S * nkv * h].view(2, 2, S, nkv, h)
        assert _decode_status(q, cache, out, ws, ws.numel(), pos0, Tn, nq, nkv, h, code) == want, (S, pos0, Tn, nq, nkv, h, code)
        torch.cuda.synchronize()
        assert untouched(out, flat, ws)
    S, pos0, Tn, nq, nkv, h = 130, 127, 2, 8, 1, 256
    need = L.iseg_gemma_decode_attention_scratch_bytes(2, pos0, Tn, nq, nkv, h, 2)
    assert need == 2 * 2 * (32 + 16 * 256) * 4
    out, flat, ws = buffers()
    cache = flat[:2 * 2 * S * nkv * h].view(2, 2, S, nkv, h)
    assert _decode_status(q, cache, out, ws, need - 1, pos0, Tn, nq, nkv, h, _hip.BF16, splits=2) == ERR_WORKSPACE
    assert "workspace" in _hip.last_error()
    torch.cuda.synchronize()
    assert untouched(out, flat, ws)
    # the rotary embedding into the cache: rows past the end of the cache
    out, flat, ws = buffers()
    cache = flat[:2 * 2 * 8 * 2 * 64].view(2, 2, 8, 2, 64)
    table = torch.zeros(8, 64, device="cuda")
    for pos0 in (7, -1):
        rc = L.iseg_gemma_rope_cache(q.data_ptr(), 8 * 64, out.data_ptr(), 4 * 64, cache[:, 0].data_ptr(), cache.stride(0), cache.stride(2),
                                     cache[:, 1].data_ptr(), cache.stride(0), cache.stride(2), table.data_ptr(), 2, 8, pos0, 2, 4, 2, 64, _hip.BF16,
                                     K.stream())
        assert rc == ERR_ARG
    torch.cuda.synchronize()
    assert untouched(out, flat, ws)


def test_decode_attention_inside_guard_bands(cuda, bf16):
    """operands, the output and a workspace of EXACTLY iseg_gemma_decode_attention_scratch_bytes between bands of poison (tests/guarded_memory.py): the
    bands are intact after the call, the workspace was asked for, and the result is the unguarded call's"""
    from iseg_amd import kernels as K

    for case in ((2, 130, 63, 2, 8, 1, 256, 0), (1, 192, 127, 2, 8, 1, 256, 3), (2, 65, 64, 1, 4, 2, 128, 0)):
        B, S, pos0, Tn, nq, nkv, h, splits = case
        q, cache, want = _core_case(case)
        plain = K.gemma_decode_attention(q.cuda(), cache.cuda(), pos0, nq, nkv, h, float(h) ** -0.5, splits)
        arena = GM.Arena(cuda, 16 << 20)
        with GM.guarded(arena):
            qd = arena.alloc(q.shape, q.dtype, "operand")
            cd = arena.alloc(cache.shape, cache.dtype, "operand")
            qd.copy_(q)
            cd.copy_(cache)
            y = K.gemma_decode_attention(qd, cd, pos0, nq, nkv, h, float(h) ** -0.5, splits)
            arena.check()
            roles = [r.role for r in arena.records]
            assert roles.count("workspace") == 1 and roles.count("output") == 1
            ws = [r for r in arena.records if r.role == "workspace"][0]
            assert ws.end - ws.start == K._hip.lib().iseg_gemma_decode_attention_scratch_bytes(B, pos0, Tn, nq, nkv, h, splits)
            assert 0 <= arena.offset_of(y) < arena.nbytes
        assert torch.equal(y.cpu(), plain.cpu()) and _rel(y.cpu().double(), want) < 1.5e-2


# ---- the model ---------------------------------------------------------------------------------------------------------------------------------
SEED = 4      # of tiny_weights and (100 + SEED) of the prompts: chosen by the top-2 margins of the fp64 greedy run (test_greedy_generation)
B, S, PROMPTS = 2, 40, (5, 9)
GEOM = (CFG["num_layers"], CFG["num_query_heads"], CFG["num_key_value_heads"])


def _model(dtype):
    """GemmaCausalLM on the 2-layer CFG of tests/test_gemma_gpu.py with the weights of tiny_weights(CFG, SEED): kernels ~ N(0, fan_in^-0.5),
    embedding std 0.02; -> (model, fp64 weights as the kernels read them)"""
    from iseg_amd import nn
    from iseg_amd.nlp.gemma import GemmaBackbone, GemmaCausalLM
    from iseg_amd.param_store import ParamStore

    model = GemmaCausalLM(GemmaBackbone(**CFG))
    ids = torch.zeros(B, S, dtype=torch.int64)
    with nn.dry_run_scope():
        model({"token_ids": ids.cuda(), "padding_mask": torch.ones(B, S, dtype=torch.int32).cuda()})
    model._iseg_store = ParamStore(list(model.parameters()))
    w = tiny_weights(CFG, SEED)
    for p in model.parameters():
        p.data.copy_(w[p.iseg_name].float().to(p.device))
    model._iseg_store.sync_shadow()
    return model, {p.iseg_name: p.data.detach().cpu().to(dtype).double() for p in model.parameters()}


def _prompts():
    ids = torch.randint(1, CFG["vocabulary_size"], (B, S), generator=torch.Generator().manual_seed(100 + SEED))
    mask = torch.zeros(B, S, dtype=torch.bool)
    for b, n in enumerate(PROMPTS):
        mask[b, :n] = True
    return ids, mask


def _uncached_composed(model, ids):
    """logits of the uncached forward on the composed attention route: code of the parent commit up to the logits GEMM"""
    prev = os.environ.get("ISEG_GEMMA_FUSED")
    os.environ["ISEG_GEMMA_FUSED"] = "0"
    try:
        with torch.no_grad():
            return model({"token_ids": ids.cuda(), "padding_mask": torch.ones(ids.shape, dtype=torch.int32).cuda()}).cpu().double()
    finally:
        if prev is None:
            os.environ.pop("ISEG_GEMMA_FUSED", None)
        else:
            os.environ["ISEG_GEMMA_FUSED"] = prev


def test_model_teacher_forced_through_the_cache_bf16(cuda, bf16):
    """seed the cache with the prompts (5 and 9 tokens, the rest of the 40 positions token 0), then feed a fixed sequence token by token from index 5.
    The logits of every step and row against fp64 on the bf16-rounded weights, all steps and rows as ONE vector (the idiom of
    tests/test_gemma_gpu.py::test_backbone_bf16_fused_against_composed): the fused cached route's relative error is at most 1.5 x that of the
    uncached composed forward on the same prefix, row by row the prefix's last.  The cache tensor that comes back is the one that went in."""
    model, w = _model(torch.bfloat16)
    final, mask = _prompts()
    want = C.causal_lm(final, None, w, *GEOM, act_dtype=torch.bfloat16)
    os.environ["ISEG_GEMMA_FUSED"] = "1"
    _, cache = model._build_cache((final * mask).cuda())
    assert tuple(cache.shape) == (B, CFG["num_layers"], 2, S, CFG["num_key_value_heads"], CFG["head_dim"]) and cache.dtype == torch.bfloat16
    got, base, ref = [], [], []
    for i in range(PROMPTS[0], S):
        logits, hidden, back = model.call_with_cache(final[:, i:i + 1].cuda(), cache, i)
        assert back is cache and tuple(logits.shape) == (B, 1, CFG["vocabulary_size"]) and tuple(hidden.shape) == (B, 1, CFG["hidden_dim"])
        got.append(logits[:, 0].cpu().double())
        base.append(_uncached_composed(model, final[:, :i + 1])[:, i])
        ref.append(want[:, i])
    got, base, ref = torch.stack(got), torch.stack(base), torch.stack(ref)
    assert torch.isfinite(got).all()
    e_cached, e_composed = _rel(got, ref), _rel(base, ref)
    print(f"cached fused {e_cached:.3e}, uncached composed {e_composed:.3e}; worst step: cached {(got - ref).abs().max().item():.3e} "
          f"composed {(base - ref).abs().max().item():.3e} of {ref.abs().max().item():.3e}")
    assert e_cached <= 1.5 * e_composed


def test_model_teacher_forced_through_the_cache_fp32(cuda):
    """the fp32 model runs the composed cached route: every step's logits to 3e-4 of the largest logit, the band of
    tests/test_gemma_gpu.py::test_backbone_fp32_matches_the_restatement"""
    from iseg_amd import nn

    nn.set_compute_dtype(torch.float32)
    nn.set_device("cuda:0")
    model, w = _model(torch.float32)
    final, mask = _prompts()
    want = C.causal_lm(final, None, w, *GEOM, act_dtype=torch.float32)
    hidden, cache = model._build_cache((final * mask).cuda())
    assert cache.dtype == torch.float32
    worst = 0.0
    for i in range(PROMPTS[0], S):
        logits, _, cache = model.call_with_cache(final[:, i:i + 1].cuda(), cache, i)
        worst = max(worst, (logits[:, 0].cpu().double() - want[:, i]).abs().max().item())
    print(f"worst logit error {worst:.3e} of {want.abs().max().item():.3e}")
    assert worst <= 3e-4 * want.abs().max().item()


@pytest.mark.parametrize("with_end", [False, True], ids=["no_end_token", "end_token"])
def test_greedy_generation(cuda, bf16, with_end):
    """generate_step to 40 positions from prompts of 5 and 9 tokens; with_end: the end token is the third token the free run generates in row 0.
    At every step the fp64 restatement is recomputed from the library's own prefix (one near-tie cannot derail the rest) and the chosen token
    must be the fp64 argmax or lie within tol of it, tol = 2 x the largest absolute logit error of the uncached composed forward (parent-commit
    code, never the cached route) against fp64 on that prefix.  The test means something only where the margins are wider than tol: at least
    three quarters of the generated positions must have an fp64 top-2 margin above tol (asserted).  Weights and prompts: seed 4, whose fp64
    greedy run on the CPU had top-2 margins, relative to the row's largest |logit|, of at least 0.036 with a lower quartile of 0.13 and a median
    of 0.24 -- the condition holds while tol stays below a few per cent of the largest logit.  The loop must stop exactly where the
    restatement's condition says, and the output padding mask is the restatement's."""
    model, w = _model(torch.bfloat16)
    ids, mask = _prompts()
    ids = ids * mask
    os.environ["ISEG_GEMMA_FUSED"] = "1"
    inputs = {"token_ids": ids.cuda(), "padding_mask": mask.cuda()}
    end = None
    if with_end:
        end = int(model.generate_step(inputs)["token_ids"][0, PROMPTS[0] + 2].item())
    result = model.generate_step(inputs, end_token_id=end)
    out, out_mask = result["token_ids"].cpu(), result["padding_mask"].cpu()
    assert torch.equal(inputs["token_ids"].cpu(), ids)      # the caller's tensors are not written
    assert torch.equal(out[mask], ids[mask])                # user tokens are kept
    strict = total = 0
    stopped = S
    for i in range(PROMPTS[0], S):
        state = torch.cat([out[:, :i], ids[:, i:]], dim=1)      # what the loop held before the step at index i
        if end is not None and bool(((state == end) & ~mask).any(dim=-1).all()):
            stopped = i
            break
        prefix = out[:, :i]
        want = C.causal_lm(prefix, None, w, *GEOM, act_dtype=torch.bfloat16)
        tol = 2 * (_uncached_composed(model, prefix) - want).abs().max().item()
        row = want[:, -1]
        top = row.topk(2, dim=-1).values
        for b in range(B):
            if mask[b, i]:
                continue
            total += 1
            strict += int((top[b, 0] - top[b, 1]).item() > tol)
            assert row[b, out[b, i]].item() >= top[b, 0].item() - tol, (i, b, out[b, i].item(), row[b].argmax().item(), tol)
    print(f"{strict} of {total} generated positions have an fp64 top-2 margin above tol; stopped at {stopped}; end token {end}")
    assert total >= 1 and 4 * strict >= 3 * total
    assert torch.equal(out[:, stopped:], ids[:, stopped:])      # nothing is generated after the loop's condition turned false
    if end is not None:
        assert bool(((out == end) & ~mask).any())               # the end token occurs
    assert torch.equal(out_mask, C.output_padding_mask(out, mask, end))
    if end is None:
        assert out_mask.all()


def test_score_logits_loss_and_the_tied_gradient(cuda):
    """fp32: score("logits") is __call__'s tensor; score("loss") against the fp64 per-token cross-entropy, and the gradient of its sum on
    token_embedding/embeddings against fp64 autograd through BOTH uses of the table (lookup and logits), to 3e-4 of the largest entry (the band of
    the fp32 model tests).  The lookup-only part differs from the total by far more than that, so a missing use would show."""
    from iseg_amd import nn

    nn.set_compute_dtype(torch.float32)
    nn.set_device("cuda:0")
    model, w = _model(torch.float32)
    ids, _ = _prompts()
    targets = torch.roll(ids, shifts=-1, dims=1)
    pad = torch.ones(B, S, dtype=torch.int32)
    with torch.no_grad():
        logits = model.score(ids.cuda(), pad.cuda())
        assert torch.equal(logits, model({"token_ids": ids.cuda(), "padding_mask": pad.cuda()}))
        assert torch.equal(logits, model.score(ids.cuda()))
    wr = {k: v.clone().requires_grad_(k == "token_embedding/embeddings") for k, v in w.items()}
    ref_logits = C.causal_lm(ids, pad, wr, *GEOM, act_dtype=torch.float32)
    assert (logits.cpu().double() - ref_logits.detach()).abs().max().item() <= 3e-4 * ref_logits.abs().max().item()
    ref_loss = torch.nn.functional.cross_entropy(ref_logits.reshape(B * S, -1), targets.reshape(-1), reduction="none").reshape(B, S)
    ref_loss.sum().backward()
    want_grad = wr["token_embedding/embeddings"].grad
    for p in model.parameters():
        p.grad = None
    seen = []
    loss = model.score(ids.cuda(), pad.cuda(), scoring_mode="loss", target_ids=targets.cuda(),
                       layer_intercept_fn=lambda x, i: (seen.append((i, tuple(x.shape))), x)[1])
    assert [i for i, _ in seen] == [-1, 0, 1] and all(s == (B, S, CFG["hidden_dim"]) for _, s in seen)
    assert tuple(loss.shape) == (B, S) and loss.dtype == torch.float32
    assert (loss.detach().cpu().double() - ref_loss.detach()).abs().max().item() <= 3e-4 * ref_loss.abs().max().item()
    loss.backward(torch.ones_like(loss))
    table = [p for p in model.parameters() if p.iseg_name == "token_embedding/embeddings"][0]
    got = table.grad.detach().cpu().double()
    assert (got - want_grad).abs().max().item() <= 3e-4 * want_grad.abs().max().item()
    # the logits use alone: d loss / d table through x @ table^T with the hidden states held fixed
    hid = C.R.backbone(ids, pad, {k: v.detach() for k, v in wr.items()}, *GEOM, act_dtype=torch.float32)
    t2 = w["token_embedding/embeddings"].clone().requires_grad_(True)
    torch.nn.functional.cross_entropy((hid @ t2.T).reshape(B * S, -1), targets.reshape(-1), reduction="sum").backward()
    assert (want_grad - t2.grad).abs().max().item() > 1e-2 * want_grad.abs().max().item()
    assert (t2.grad).abs().max().item() > 1e-2 * want_grad.abs().max().item()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_embedding_logits_keeps_the_gradient_buffer_contract(cuda, dtype):
    """F.embedding_logits is the dense node with the kernel stored [out, in]: forward x @ table^T, dx = dy @ table, and the four clauses of
    tests/grad_contract_cases.py on this route -- the table's gradient is ADDED to what its buffer holds, autograd is handed None for it, a frozen
    table receives nothing, and dx is produced whatever is frozen.  Max-norm bands relative to the largest entry: 3e-4 in fp32 and 1.2e-2 in bf16,
    the bands of the GEMM tests (tests/test_kernels_gpu.py::close)"""
    from iseg_amd import functional as F
    from iseg_amd import nn

    vocab, d, n = 75, 128, 37
    tol = 3e-4 if dtype == torch.float32 else 1.2e-2
    nn.set_compute_dtype(dtype)
    try:
        x = rnd((1, n, d), 41).to(dtype)
        dy = rnd((1, n, vocab), 42).to(dtype)
        base = rnd((vocab, d), 43).float()

        def table(trainable):
            t = torch.nn.Parameter(rnd((vocab, d), 44).to(dtype).float().cuda(), requires_grad=trainable)
            t.iseg_name, t.iseg_compute = "token_embedding/embeddings", t.data.to(dtype)
            return t

        def near(got, want):
            return (got.detach().cpu().double() - want).abs().max().item() <= tol * want.abs().max().item()

        tw = table(True).data.cpu().double()
        for trainable in (True, False):
            t = table(trainable)
            if trainable:
                t.grad = base.clone().cuda()
            xd = x.cuda().requires_grad_(True)
            y = F.embedding_logits(xd, t)
            assert y.dtype == dtype and tuple(y.shape) == (1, n, vocab) and type(y.grad_fn).__name__.startswith("_DenseFn")
            assert near(y, x.double() @ tw.T)
            y.backward(dy.cuda())
            assert near(xd.grad, dy.double() @ tw)
            if trainable:
                assert near(t.grad - base.cuda(), dy.double()[0].T @ x.double()[0])
            else:
                assert t.grad is None
    finally:
        nn.set_compute_dtype(torch.float32)
