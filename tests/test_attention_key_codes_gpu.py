"""Row-exact tests of the fused attention kernels' masks, tiles and tails on the key-coded inputs of tests/attention_key_codes.py: causal
grouped-query prefill forward and backward (csrc/gemma.hip), split-KV decode with its _at twin (csrc/gemma_decode.hip) and the 64-wide-key /
wide-value self-attention (csrc/selfattn.hip), against the suite's fp64 restatements.  Every output row names the key or keys it attended, so
the output is compared BITWISE with bf16(reference) and the gradients per element with bounds derived in the helper; the kernel-level calls
run inside the guard arena of tests/guarded_memory.py, where whatever lies past the last row is NaN poison.
tests/test_attention_key_codes_host.py pins the inputs: ties, gaps, out-scoring invisible keys, and which mask errors they expose.

What reaches what (hot key = a key that out-scores every other for every query):
  64-key tile edges   prefill 1x130x8x1x256 hot 64 / hot 128, 1x130x6x2x64 hot 128, 1x197x16x16x64 hot 128, 2x65x4x2x128 hot 64 (padded);
                      decode pos0 = 63, 64, 127 (hot 127 / 128), 191 (hot 192), 255; self-attention T = 63, 64, 65, 130 with the hot key at T - 1
  a tile with one key prefill T = 65, 130 (two keys), 197 (five); decode nvis = 65, 129, 193; self-attention T = 65
  single-tile chunks  decode 1x160x127x2x8x1x256 with three chunks, the last holding key 128 alone, visible to the second token only
  g = 3 stacking      prefill 1x130x6x2x64 (R / g is not a shift)
  the row past T      every prefill and self-attention case inside the arena (NaN there), self-attention's sample 1 starting with marked keys,
                      decode rows nvis and nvis + 1 marked and finite, NaN behind"""
import functools
import os

import pytest
import torch

from tests import attention_key_codes as AK
from tests import guarded_memory as GM

pytestmark = pytest.mark.gpu


@pytest.fixture
def bf16():
    from iseg_amd import nn

    nn.set_compute_dtype(torch.bfloat16)
    nn.set_device("cuda:0")
    try:
        yield
    finally:
        os.environ.pop("ISEG_GEMMA_FUSED", None)
        os.environ.pop("ISEG_SELFATTN_FUSED", None)
        nn.set_compute_dtype(torch.float32)


@functools.lru_cache(maxsize=None)
def _problem(kind, entry):
    """(Problem, reference, bounds): built once per case, shared, never modified"""
    p = {"prefill": AK.prefill, "decode": AK.decode, "self": AK.self_attention}[kind](*entry)
    ref = AK.reference(p)
    return p, ref, AK.bounds(p, ref)


def _put(arena, t):
    d = arena.alloc(t.shape, t.dtype, "operand")
    d.copy_(t)
    return d


def _bits(t):
    return t.contiguous().view(torch.int16)


def _differing(got, want):
    """the first rows whose bf16 values differ, as (sample, token, head): got[:4] / want[:4]"""
    rows = torch.nonzero((got != want).any(-1))
    return f"{rows.shape[0]} rows differ; " + "; ".join(f"{tuple(r.tolist())}: {got[tuple(r)][:4].tolist()} / {want[tuple(r)][:4].tolist()}"
                                                          for r in rows[:6])


def _check_out(p, ref, out, who):
    want = AK.bf16_round(ref[0])
    assert torch.isfinite(out).all(), who
    assert torch.equal(out, want), (who, _differing(out, want))
    empty = ~p.vis.any(-1)
    assert out[empty].abs().sum().item() == 0, who


def _check_grads(p, ref, bounds, grads, who):
    empty, unseen = ~p.vis.any(-1), AK.unseen_keys(p)
    frac = []
    for name, a, r, b in zip(("dq", "dk", "dv"), grads, ref[1:], bounds):
        assert torch.isfinite(a).all(), (who, name)
        err = (a - r).abs()
        frac.append(f"{name} {(err / b).max().item():.2f}")
        bad = err > b
        assert not bad.any(), (who, name, int(bad.sum()), torch.nonzero(bad)[:4].tolist(), a[bad][:4].tolist(), r[bad][:4].tolist())
    print(f"{who}: fraction of the bounds " + " ".join(frac))
    assert grads[0][empty].abs().sum().item() == 0, who
    assert grads[1][unseen].abs().sum().item() == 0 and grads[2][unseen].abs().sum().item() == 0, who


# ---- prefill -----------------------------------------------------------------------------------------------------------------------------------
def _split(p, rows):
    B, T, nq, nkv, h = p.case
    t = rows.detach().cpu().double()
    return (t[..., :nq * h].reshape(B, T, nq, h), t[..., nq * h:(nq + nkv) * h].reshape(B, T, nkv, h), t[..., (nq + nkv) * h:].reshape(B, T, nkv, h))


@pytest.mark.parametrize("entry", AK.PREFILL, ids=[AK.ident(e) for e in AK.PREFILL])
def test_prefill_kernels_row_exact(cuda, entry):
    """gemma_attention_fwd / _bwd inside the guard arena: out bitwise bf16(reference), dq / dk / dv within the derived bounds, exact zeros for rows
    without a visible key and for keys nobody sees, everything finite, a second run bit-identical, operands unchanged, bands intact"""
    from iseg_amd import kernels as K

    p, ref, bounds = _problem("prefill", entry)
    B, T, nq, nkv, h = p.case
    arena = GM.Arena(cuda, 32 << 20)
    runs = []
    with GM.guarded(arena):
        x, d = _put(arena, p.qkv), _put(arena, p.dout_rows)
        mask = None if p.pad is None else _put(arena, (p.pad != 0).to(torch.uint8))
        for _ in range(2):
            out, lse = K.gemma_attention_fwd(x, mask, nq, nkv, h, p.scale, True)
            runs.append((out, K.gemma_attention_bwd(x, mask, out, d, lse, nq, nkv, h, p.scale)))
        arena.check()
    assert torch.equal(_bits(runs[0][0]), _bits(runs[1][0])) and torch.equal(_bits(runs[0][1]), _bits(runs[1][1]))
    assert torch.equal(_bits(x.cpu()), _bits(p.qkv)) and torch.equal(_bits(d.cpu()), _bits(p.dout_rows))
    who = AK.ident(entry)
    _check_out(p, ref, runs[0][0].cpu().double().reshape(B, T, nq, h), who)
    _check_grads(p, ref, bounds, _split(p, runs[0][1]), who)


def _core(p, mode):
    from iseg_amd import functional as F

    B, T, nq, nkv, h = p.case
    os.environ["ISEG_GEMMA_FUSED"] = mode
    x = p.qkv.cuda().requires_grad_(True)
    out = F.gemma_attention_core(x, None if p.pad is None else p.pad.cuda(), nq, nkv, h)
    names, stack = set(), [out.grad_fn]
    while stack:
        fn = stack.pop()
        if fn is not None:
            names.add(type(fn).__name__)
            stack += [f for f, _ in fn.next_functions]
    assert any(n.startswith("_GemmaAttentionFn") for n in names) == (mode == "1"), names
    assert any(n.startswith("_AttentionFn") for n in names) == (mode == "0"), names
    out.backward(p.dout_rows.cuda())
    return out.detach().cpu().double().reshape(B, T, nq, h), _split(p, x.grad)


def test_prefill_through_autograd_on_the_fused_node(cuda, bf16):
    """the g = 3 case through F.gemma_attention_core with ISEG_GEMMA_FUSED=1: the fused node is in the graph, the same checks"""
    entry = ((1, 130, 6, 2, 64), "holes", (128,))
    assert entry in AK.PREFILL
    p, ref, bounds = _problem("prefill", entry)
    out, grads = _core(p, "1")
    _check_out(p, ref, out, "fused node")
    _check_grads(p, ref, bounds, grads, "fused node")


@pytest.mark.parametrize("entry", AK.PREFILL, ids=[AK.ident(e) for e in AK.PREFILL])
def test_prefill_composed_route(cuda, bf16, entry):
    """ISEG_GEMMA_FUSED=0 rounds the scores to bf16 (spacing 16 at |score| <= 3349: ties stay ties, a gap of 64 stays at least 32).  Out is asserted
    bitwise where the helper's restatement with bf16-rounded scores reproduces the reference on the CPU (AK.COMPOSED_EXACT, pinned by the host test)"""
    p, ref, _ = _problem("prefill", entry)
    out, _ = _core(p, "0")
    want = AK.bf16_round(ref[0])
    print(f"{AK.ident(entry)} composed: {int((out != want).any(-1).sum())} rows differ")
    if AK.ident(entry) in AK.COMPOSED_EXACT:
        _check_out(p, ref, out, "composed")


# ---- decode ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", AK.DECODE, ids=[AK.ident(e) for e in AK.DECODE])
def test_decode_kernels_row_exact(cuda, bf16, entry):
    """gemma_decode_attention inside the guard arena: out bitwise bf16(reference) and finite although the cache holds marked keys right behind
    the last visible one and NaN behind those; the cache is not written; a second run, splits = 1 and the _at launcher at pos_d = pos0 give the
    same bits (so every split does); the composed route as in test_prefill_composed_route"""
    from iseg_amd import functional as F
    from iseg_amd import kernels as K

    p, ref, _ = _problem("decode", entry)
    B, S, pos0, Tn, nq, nkv, h, splits = p.case
    want = AK.bf16_round(ref[0])
    arena = GM.Arena(cuda, 32 << 20)
    with GM.guarded(arena):
        qd, cd = _put(arena, p.q_rows), _put(arena, p.cache)
        pos_d = _put(arena, torch.tensor([pos0], dtype=torch.int32))
        outs = {"first": K.gemma_decode_attention(qd, cd, pos0, nq, nkv, h, p.scale, splits),
                "second": K.gemma_decode_attention(qd, cd, pos0, nq, nkv, h, p.scale, splits),
                "splits 1": K.gemma_decode_attention(qd, cd, pos0, nq, nkv, h, p.scale, 1),
                "_at": K.gemma_decode_attention_at(qd, cd, pos_d, nq, nkv, h, p.scale, splits)}
        arena.check()
    assert torch.equal(_bits(cd.cpu()), _bits(p.cache)) and torch.equal(_bits(qd.cpu()), _bits(p.q_rows))
    for who, y in outs.items():
        _check_out(p, ref, y.cpu().double().reshape(B, Tn, nq, h), who)
    os.environ["ISEG_GEMMA_FUSED"] = "0"
    y = F.gemma_cached_attention_core(p.q_rows.cuda(), p.cache.cuda(), pos0, nq, nkv, h).cpu().double().reshape(B, Tn, nq, h)
    print(f"{AK.ident(entry)} composed: {int((y != want).any(-1).sum())} rows differ")
    if AK.ident(entry) in AK.COMPOSED_EXACT:
        _check_out(p, ref, y, "composed")


# ---- self-attention ----------------------------------------------------------------------------------------------------------------------------
def _self_checks(p, ref, bounds, got, who):
    out, dq, dk, dvv = (t.detach().cpu().double()[:, :, None, :] for t in got)
    _check_out(p, ref, out, who)
    _check_grads(p, ref, bounds, (dq, dk, dvv), who)


@pytest.mark.parametrize("run", AK.SELF_RUNS, ids=AK.SELF_IDS)
def test_self_attention_kernels_row_exact(cuda, run):
    """self_attention_fwd / _bwd on two contiguous samples inside the guard arena (rows T .. of sample 0 are sample 1's marked first keys; behind
    sample 1 lies NaN): out bitwise bf16(reference), dq / dk / dv within the derived bounds (no group sum here), everything finite, a second run
    bit-identical, bands intact"""
    from iseg_amd import kernels as K

    p, ref, bounds = _problem("self", run)
    arena = GM.Arena(cuda, 32 << 20)
    runs = []
    with GM.guarded(arena):
        q, k, v, d = (_put(arena, t[:, :, 0].to(torch.bfloat16)) for t in (p.q, p.k, p.v, p.dout))
        for _ in range(2):
            out, lse = K.self_attention_fwd(q, k, v, p.scale, True)
            runs.append((out,) + K.self_attention_bwd(q, k, v, out, d, lse, p.scale))
        arena.check()
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(*runs))
    _self_checks(p, ref, bounds, runs[0], AK.SELF_IDS[AK.SELF_RUNS.index(run)])


def test_self_attention_pitched_operands(cuda):
    """q | k | v as column ranges of one [B, T, 64 + 64 + dv] tensor inside the arena, as test_core_pitched_and_aliased_operands builds them"""
    from iseg_amd import kernels as K

    run = (130, 512, 129)
    assert run in AK.SELF_RUNS
    p, ref, bounds = _problem("self", run)
    arena = GM.Arena(cuda, 32 << 20)
    with GM.guarded(arena):
        packed = _put(arena, torch.cat([t[:, :, 0] for t in (p.q, p.k, p.v)], dim=-1).to(torch.bfloat16))
        d = _put(arena, p.dout[:, :, 0].to(torch.bfloat16))
        q, k, v = packed[..., :64], packed[..., 64:128], packed[..., 128:]
        assert all(not t.is_contiguous() and K._pitched(t)[1] == 128 + 512 and K._pitched(t)[0].data_ptr() == t.data_ptr() for t in (q, k, v))
        out, lse = K.self_attention_fwd(q, k, v, p.scale, True)
        got = (out,) + K.self_attention_bwd(q, k, v, out, d, lse, p.scale)
        arena.check()
    _self_checks(p, ref, bounds, got, "pitched")


@pytest.mark.parametrize("run", AK.SELF_RUNS, ids=AK.SELF_IDS)
def test_self_attention_composed_route(cuda, bf16, run):
    """ISEG_SELFATTN_FUSED=0: F.attention_packed (its materialised route rounds the scores to bf16; at dv = 64 it may take the equal-width flash
    kernels instead): out bitwise, as the host test's restatement with rounded scores"""
    from iseg_amd import functional as F

    p, ref, _ = _problem("self", run)
    os.environ["ISEG_SELFATTN_FUSED"] = "0"
    q, k, v = (t[:, :, 0].to(torch.bfloat16).cuda().requires_grad_(True) for t in (p.q, p.k, p.v))
    out = F.self_attention_core(q, k, v, p.scale)
    assert not type(out.grad_fn).__name__.startswith("_SelfAttentionFn")
    _check_out(p, ref, out.detach().cpu().double()[:, :, None, :], "composed")
