"""Gemma backbone on the device (iseg_amd/nlp/gemma, csrc/gemma.hip) against the fp64 restatement in tests/gemma_ref.py: the attention core on both
routes (fused kernels, and ISEG_GEMMA_FUSED=0: repeated K / V through F.attention_packed with an additive mask), the rotary embedding, the tanh
GELU in the activation and gated-product kernels, the embedding gradient, and the whole backbone with every parameter gradient."""
import math
import os

import pytest
import torch

from tests import gemma_ref as R
from tests import range_edge_inputs as E
from tests.test_kernels_gpu import DTYPES, rnd
from tests.util_models import randomize_parameters

pytestmark = pytest.mark.gpu

# (B, T, nq, nkv, h): one token; an exact tile with a group of two; ragged tiles, two kv heads, two slabs; a group of eight at the full width
# over three key tiles; sixteen ungrouped heads over four key tiles; a stacked-row count (8 * 63) that ends inside a tile
CASES = [(2, 1, 1, 1, 64), (1, 64, 2, 1, 64), (2, 65, 4, 2, 128), (1, 130, 8, 1, 256), (1, 197, 16, 16, 64), (2, 63, 8, 1, 256)]
MASKS = ["none", "right", "left3", "left70"]
CORE = [(c, m) for c in CASES for m in MASKS if m != "left70" or c[1] >= 130]


def _padding(kind, B, T):
    """none; right padding to a ragged length per sample; left padding of 3 tokens (rows 0..2 see nothing); left padding of 70 (the whole
    first key tile is invisible)"""
    if kind == "none":
        return None
    m = torch.ones(B, T, dtype=torch.int32)
    for b in range(B):
        if kind == "right":
            m[b, max(1, T - 5 - 3 * b):] = 0
        else:
            m[b, :min(T, 3 if kind == "left3" else 70)] = 0
    return m


def _core_case(case, kind):
    """bf16-rounded packed rows ~ N(0, 1) (scores h^-0.5 q.k of standard deviation 1) and dout; the restatement's fp64 output and gradients"""
    B, T, nq, nkv, h = case
    W = (nq + 2 * nkv) * h
    qkv = rnd((B, T, W), 1).to(torch.bfloat16)
    dout = rnd((B, T, nq * h), 2).to(torch.bfloat16)
    pad = _padding(kind, B, T)
    ref = qkv.double().requires_grad_(True)
    q, k, v = ref[..., :nq * h], ref[..., nq * h:(nq + nkv) * h], ref[..., (nq + nkv) * h:]
    want = R.attention_core(q.reshape(B, T, nq, h), k.reshape(B, T, nkv, h), v.reshape(B, T, nkv, h), pad, nq, nkv)
    want.backward(dout.double())
    return qkv, dout, pad, want.detach(), ref.grad


def _split(t, nq, nkv, h):
    return t[..., :nq * h], t[..., nq * h:(nq + nkv) * h], t[..., (nq + nkv) * h:]


def _run_core(qkv, dout, pad, case, mode):
    from iseg_amd import functional as F

    _, _, nq, nkv, h = case
    os.environ["ISEG_GEMMA_FUSED"] = mode
    x = qkv.cuda().requires_grad_(True)
    out = F.gemma_attention_core(x, None if pad is None else pad.cuda(), nq, nkv, h)
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == tuple(dout.shape)
    names = set()
    stack = [out.grad_fn]
    while stack:
        fn = stack.pop()
        if fn is not None:
            names.add(type(fn).__name__)
            stack += [f for f, _ in fn.next_functions]
    assert any(n.startswith("_GemmaAttentionFn") for n in names) == (mode == "1"), names
    assert any(n.startswith("_AttentionFn") for n in names) == (mode == "0"), names
    out.backward(dout.cuda())
    return out.detach().cpu().double(), x.grad.detach().cpu().double()


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


@pytest.mark.parametrize("case,kind", CORE, ids=["x".join(map(str, c)) + "-" + m for c, m in CORE])
def test_core_both_routes_against_fp64(cuda, bf16, case, kind):
    """the bounds of tests/test_self_attention_gpu.py::test_core_both_routes_against_fp64: relative Frobenius error 1.5e-2 for the output, 3e-2 for
    each of dq, dk, dv with the floor 1e-3 * |g| for slices that are (nearly) zero; fp64 is the yardstick of both routes.  Also: everything finite,
    rows without a visible key exactly zero in out and dq, a second fused run bit-identical, the inference forward the training forward's bits."""
    from iseg_amd import functional as F

    B, T, nq, nkv, h = case
    qkv, dout, pad, want, grads = _core_case(case, kind)
    gparts = _split(grads, nq, nkv, h)
    gnorm = grads.norm().item()
    vis = R.attention_mask(pad, B, T)
    empty = ~vis.any(dim=-1)      # [B, T]
    res = {}
    for mode in ("1", "0"):
        res[mode] = _run_core(qkv, dout, pad, case, mode)
        out, dqkv = res[mode]
        print(f"mode {mode} out rel {_rel(out, want):.3e} " + " ".join(
            f"{n} {(a - r).norm().item():.3e}/{r.norm().item():.3e}" for n, a, r in zip(("dq", "dk", "dv"), _split(dqkv, nq, nkv, h), gparts)))
    for mode in ("1", "0"):
        out, dqkv = res[mode]
        assert torch.isfinite(out).all() and torch.isfinite(dqkv).all(), mode
        assert _rel(out, want) < 1.5e-2, mode
        for name, a, r in zip(("dq", "dk", "dv"), _split(dqkv, nq, nkv, h), gparts):
            assert (a - r).norm().item() <= 3e-2 * max(r.norm().item(), 1e-3 * gnorm), (mode, name)
        assert out[empty].abs().max().item() == 0 if empty.any() else True, mode
        assert dqkv[..., :nq * h][empty].abs().max().item() == 0 if empty.any() else True, mode
    again = _run_core(qkv, dout, pad, case, "1")
    assert torch.equal(again[0], res["1"][0]) and torch.equal(again[1], res["1"][1])
    os.environ["ISEG_GEMMA_FUSED"] = "1"
    with torch.no_grad():
        y = F.gemma_attention_core(qkv.cuda(), None if pad is None else pad.cuda(), nq, nkv, h)
    assert y.grad_fn is None and torch.equal(y.cpu().double(), res["1"][0])


def test_core_masked_pairs_give_exact_zeros_in_dk_dv(cuda, bf16):
    """keys that no query may see (left padding of 70 at T = 130) receive dk = dv = 0 exactly on the fused route"""
    case = (1, 130, 8, 1, 256)
    qkv, dout, pad, _, _ = _core_case(case, "left70")
    _, dqkv = _run_core(qkv, dout, pad, case, "1")
    _, dk, dv = _split(dqkv, *case[2:])
    assert dk[0, :70].abs().max().item() == 0 and dv[0, :70].abs().max().item() == 0
    assert dk[0, 70:].abs().max().item() > 0 and dv[0, 70:].abs().max().item() > 0


def test_core_forward_keeps_no_t_by_t_tensor(cuda, bf16):
    """peak device memory above the level before a forward at B = 1, T = 2048, nq = 8 on nkv = 1, h = 64: below the 8 MiB of ONE head's bf16
    probability tensor on the fused route (output 2 MiB, log-sum-exp 64 KiB, mask bytes); far above on the composed route, which shows that the
    probe sees such tensors"""
    from iseg_amd import functional as F

    B, T, nq, nkv, h = 1, 2048, 8, 1, 64
    qkv = rnd((B, T, (nq + 2 * nkv) * h), 3).to(torch.bfloat16).cuda()
    pad = _padding("right", B, T).cuda()
    peak = {}
    for mode in ("0", "1"):
        os.environ["ISEG_GEMMA_FUSED"] = mode
        x = qkv.clone().requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        y = F.gemma_attention_core(x, pad, nq, nkv, h)
        torch.cuda.synchronize()
        peak[mode] = torch.cuda.max_memory_allocated() - base
        del y, x
    print(f"peak above base: fused {peak['1']} composed {peak['0']}")
    assert peak["1"] < T * T * 2 < peak["0"]


def test_core_refuses_unsupported_shapes(cuda, bf16):
    from iseg_amd import _hip
    from iseg_amd import functional as F
    from iseg_amd import kernels as K

    assert not K.gemma_attention_supported(4, 2, 96, torch.bfloat16) and not K.gemma_attention_supported(4, 2, 320, torch.bfloat16)
    assert not K.gemma_attention_supported(4, 3, 64, torch.bfloat16) and not K.gemma_attention_supported(4, 2, 64, torch.float32)
    assert all(K.gemma_attention_supported(8, 1, h, torch.bfloat16) for h in (64, 128, 192, 256))
    qkv = torch.zeros(1, 8, (4 + 4) * 32, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(_hip.HipCallError):
        K.gemma_attention_fwd(qkv, None, 4, 2, 32, 1.0, False)
    os.environ["ISEG_GEMMA_FUSED"] = "1"      # an unsupported width takes the composed route whatever the switch says
    y = F.gemma_attention_core(qkv.requires_grad_(True), None, 4, 2, 32)
    assert type(y.grad_fn).__name__.startswith("_AttentionFn")


# ---- rotary embedding -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_rope_matches_the_restatement_above_position_256(cuda, dtype):
    """T = 300: bf16 angles (the reference's compute dtype) could not tell positions 256 .. 300 apart.  Forward within one rounding of the storage
    type (2^-8 |y| for bf16, 2^-22 for fp32) plus the fp32 table's error (angles up to 300 carry an ulp of 3e-5: 1e-4 of the pair's norm); forward
    followed by inverse returns the input within two roundings (each at most 2^-8 of its value: 2^-8 (sqrt(2) r + |x|) <= 2.5 * 2^-8 r per pair of norm r); v columns bit-unchanged;
    in place gives the bits of out of place"""
    from iseg_amd import functional as F
    from iseg_amd import kernels as K
    from iseg_amd import nn

    B, T, nq, nkv, h = 1, 300, 2, 1, 64
    nn.set_compute_dtype(dtype)
    try:
        x = rnd((B, T, (nq + 2 * nkv) * h), 5).to(dtype)
        xd = x.cuda().requires_grad_(True)
        y = F.gemma_rope(xd, nq, nkv, h)
        assert type(y.grad_fn).__name__.startswith("_GemmaRopeFn")
        qk = x.double()[..., :(nq + nkv) * h].reshape(B, T, nq + nkv, h)
        want = R.apply_rope(qk, torch.arange(T, dtype=torch.float64)[None])
        got = y.detach().cpu().double()
        gq = got[..., :(nq + nkv) * h].reshape(B, T, nq + nkv, h)
        r = (qk[..., :h // 2] ** 2 + qk[..., h // 2:] ** 2).sqrt()      # pair norms, [.., h/2]
        r_out = torch.stack([r, r], dim=-1).reshape(qk.shape)          # at the interleaved output positions
        ulp = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -22
        assert ((gq - want).abs() <= ulp * want.abs() + 1e-4 * r_out).all(), (gq - want).abs().max().item()
        assert torch.equal(y.detach()[..., (nq + nkv) * h:], xd.detach()[..., (nq + nkv) * h:])
        # a position above 256 differs from its bf16-rounded neighbour: the table is fp32
        assert not torch.equal(y.detach()[0, 299, :h], y.detach()[0, 298, :h])
        table = F.gemma_rope_table(T, h, xd.device)
        assert table.dtype == torch.float32 and tuple(table.shape) == (T, h) and F.gemma_rope_table(T, h, xd.device) is table
        back = K.gemma_rope(y.detach(), table, T, nq, nkv, h, inverse=True, out=torch.empty_like(y)).cpu().double()
        bq = back[..., :(nq + nkv) * h].reshape(B, T, nq + nkv, h)
        r_in = torch.cat([r, r], dim=-1)
        assert ((bq - qk).abs() <= 2.5 * ulp * r_in + 2e-4 * r_in).all(), (bq - qk).abs().max().item()
        inplace = xd.detach().clone()
        K.gemma_rope(inplace, table, T, nq, nkv, h)
        assert torch.equal(inplace, y.detach())
        # backward = the transposed rotation of the gradient
        g = rnd(tuple(x.shape), 6).to(dtype)
        y.backward(g.cuda())
        assert torch.equal(xd.grad, K.gemma_rope(g.cuda(), table, T, nq, nkv, h, inverse=True, out=torch.empty_like(g.cuda())))
    finally:
        nn.set_compute_dtype(torch.float32)


# ---- tanh GELU --------------------------------------------------------------------------------------------------------------------------------
def _gelu_bounds(dtype, want):
    """storage rounding (2^-8 relative in bf16; 2e-5 in fp32, the band of the other activations) plus 2e-6 absolute: 0.5 (1 + tanh u) cancels for
    x < 0 and carries the fp32 ulp of 1 (6e-8) times |x| <= 10 where it matters"""
    return (2.0 ** -8 if dtype == torch.bfloat16 else 2e-5) * want.abs() + 2e-6


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_gelu_tanh_activation_on_the_range_edge_grid(cuda, dtype):
    from iseg_amd import kernels as K

    x = torch.cat([E.act_grid(dtype), E.rq(torch.linspace(-9, 9, 41, dtype=torch.float64), dtype)])
    want, dwant = R.gelu_tanh(x), R.gelu_tanh_grad(x)
    xd = x.to(dtype).cuda()
    y = K.act_fwd(xd, K.ACT_GELU_TANH).cpu().double()
    dx = K.act_bwd(torch.full_like(xd, 1.5), xd, K.ACT_GELU_TANH).cpu().double()
    assert torch.isfinite(y).all() and torch.isfinite(dx).all()
    bad = (y - want).abs() > _gelu_bounds(dtype, want)
    assert not bad.any(), (x[bad].tolist(), y[bad].tolist(), want[bad].tolist())
    bad = (dx - 1.5 * dwant).abs() > 1.5 * _gelu_bounds(dtype, dwant)
    assert not bad.any(), (x[bad].tolist(), dx[bad].tolist(), (1.5 * dwant[bad]).tolist())


@pytest.mark.parametrize("cols", [256, 262], ids=["vec8", "anywidth"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_gelu_tanh_gated_product(cuda, dtype, cols):
    """iseg_glu_fwd / _bwd with ISEG_ACT_GELU_TANH: 256 columns take the 16-byte form, 262 the one-element-per-lane form; the first row's gate holds
    the range-edge grid"""
    from iseg_amd import kernels as K

    rows = 7
    gate = rnd((rows, cols), 11).double() * 3
    grid = E.act_grid(dtype).double()
    gate[0, :grid.numel()] = grid
    gate = E.rq(gate, dtype)
    xv = E.rq(rnd((rows, cols), 12).double(), dtype)
    dout = E.rq(rnd((rows, cols), 13).double(), dtype)
    a, da = R.gelu_tanh(gate), R.gelu_tanh_grad(gate)
    gd, xd, dd = (t.to(dtype).cuda() for t in (gate, xv, dout))
    out = K.glu_fwd(gd, xd, K.ACT_GELU_TANH).cpu().double()
    dg, dx = torch.empty_like(gd), torch.empty_like(xd)
    K.glu_bwd(dd, gd, xd, dg, dx, K.ACT_GELU_TANH)
    dg, dx = dg.cpu().double(), dx.cpu().double()
    assert all(torch.isfinite(t).all() for t in (out, dg, dx))
    # a product of the activation with a stored factor: the activation's band times the factor, plus the product's own rounding
    assert ((out - a * xv).abs() <= _gelu_bounds(dtype, a) * xv.abs() + _gelu_bounds(dtype, a * xv)).all()
    assert ((dx - a * dout).abs() <= _gelu_bounds(dtype, a) * dout.abs() + _gelu_bounds(dtype, a * dout)).all()
    f = dout * xv
    assert ((dg - da * f).abs() <= _gelu_bounds(dtype, da) * f.abs() + _gelu_bounds(dtype, da * f)).all()


# ---- embedding --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_embedding_gradient_with_repeated_tokens(cuda, dtype):
    """37 tokens over a vocabulary of 11 with two ids absent (4 and 10): every present row repeats at least three times.  Against fp64 to 3e-4 of
    the largest entry, two runs bit-identical, rows of absent tokens exactly zero; through F.embedding the forward is table[ids] * scale with the
    scale rounded to the activation type"""
    from iseg_amd import functional as F
    from iseg_amd import kernels as K
    from iseg_amd import nn

    vocab, d, n = 11, 128, 37
    present = [v for v in range(vocab) if v not in (4, 10)]
    ids = torch.tensor([present[(i * 5) % len(present)] for i in range(n)], dtype=torch.int64)
    assert all((ids == v).sum() >= 3 for v in present)
    dy = rnd((n, d), 21).to(dtype)
    scale = float(torch.tensor(math.sqrt(d)).to(dtype))
    want = torch.zeros(vocab, d, dtype=torch.float64).index_add_(0, ids, dy.double()) * scale
    sorted_ids, order = torch.sort(ids.cuda(), stable=True)
    runs = [K.embedding_grad(dy.cuda(), sorted_ids, order, torch.zeros(vocab, d, device="cuda"), scale) for _ in range(2)]
    assert torch.equal(runs[0], runs[1])
    got = runs[0].cpu().double()
    assert (got - want).abs().max().item() <= 3e-4 * want.abs().max().item()
    assert got[4].abs().max().item() == 0 and got[10].abs().max().item() == 0 and all(got[v].abs().max().item() > 0 for v in present)
    # the node: forward and the gradient that lands in table.grad
    nn.set_compute_dtype(dtype)
    try:
        table = torch.nn.Parameter(rnd((vocab, d), 22).float().cuda())
        table.iseg_name, table.iseg_compute = "token_embedding/embeddings", table.data.to(dtype)
        y = F.embedding(ids.reshape(1, n).cuda(), table, math.sqrt(d))
        assert y.dtype == dtype and tuple(y.shape) == (1, n, d)
        ref = table.data.to(dtype).double().cpu()[ids] * scale
        assert ((y.detach().cpu().double()[0] - ref).abs() <= (2.0 ** -8 if dtype == torch.bfloat16 else 1e-6) * ref.abs()).all()
        y.backward(dy.reshape(1, n, d).cuda())
        assert torch.equal(table.grad, runs[0])
    finally:
        nn.set_compute_dtype(torch.float32)


# ---- the whole backbone -----------------------------------------------------------------------------------------------------------------------
CFG = dict(vocabulary_size=97, num_layers=2, num_query_heads=4, num_key_value_heads=2, hidden_dim=128, intermediate_dim=512, head_dim=64)


def _backbone_inputs():
    B, T = 2, 37
    ids = torch.randint(0, CFG["vocabulary_size"], (B, T), generator=torch.Generator().manual_seed(31))
    pad = torch.ones(B, T, dtype=torch.int32)
    pad[1, 29:] = 0
    dout = rnd((B, T, CFG["hidden_dim"]), 32)
    return ids, pad, dout


def _backbone(dtype, seed=7):
    from iseg_amd import nn
    from iseg_amd.nlp.gemma.gemma_backbone import GemmaBackbone
    from iseg_amd.param_store import ParamStore

    model = GemmaBackbone(**CFG)
    ids, pad, _ = _backbone_inputs()
    with nn.dry_run_scope():
        model({"token_ids": ids.cuda(), "padding_mask": pad.cuda()})
    model._iseg_store = ParamStore(list(model.parameters()))
    randomize_parameters(model, seed)
    model._iseg_store.sync_shadow()
    return model


def _backbone_reference(model, dtype):
    """fp64 output and parameter gradients on the values the kernels read (bf16-rounded under mixed precision)"""
    ids, pad, dout = _backbone_inputs()
    w = {p.iseg_name: p.data.detach().cpu().to(dtype).double().requires_grad_(True) for p in model.parameters()}
    out = R.backbone(ids, pad, w, CFG["num_layers"], CFG["num_query_heads"], CFG["num_key_value_heads"], act_dtype=dtype)
    out.backward(dout.to(dtype).double())
    return out.detach(), w


def _backbone_run(model, dtype, training=True):
    ids, pad, dout = _backbone_inputs()
    for p in model.parameters():
        p.grad = None
    out = model({"token_ids": ids.cuda(), "padding_mask": pad.cuda()}, training=training)
    out.backward(dout.to(dtype).cuda())
    return out.detach().cpu().double(), {p.iseg_name: p.grad.detach().cpu().double().clone() for p in model.parameters()}


def test_backbone_fp32_matches_the_restatement(cuda):
    """output and every parameter gradient to 3e-4 of the tensor's largest entry (gradients: with the floor 1e-3 of the largest gradient entry
    of the model), the band of the fp32 model tests; fp32 runs on the composed route"""
    from iseg_amd import nn

    nn.set_compute_dtype(torch.float32)
    nn.set_device("cuda:0")
    model = _backbone(torch.float32)
    want, w = _backbone_reference(model, torch.float32)
    out, grads = _backbone_run(model, torch.float32)
    assert torch.isfinite(out).all()
    assert (out - want).abs().max().item() <= 3e-4 * want.abs().max().item(), (out - want).abs().max().item()
    gmax = max(t.grad.abs().max().item() for t in w.values())
    bad = {}
    for name, t in w.items():
        e = (grads[name] - t.grad).abs().max().item() / max(t.grad.abs().max().item(), 1e-3 * gmax)
        if not e <= 3e-4:
            bad[name] = e
    assert not bad, bad


def test_backbone_bf16_fused_against_composed(cuda, bf16):
    """both routes on the same bf16 model and inputs, each against fp64: the fused route's error (output; all parameter gradients as one vector) is at
    most 1.5 x the composed route's; every parameter receives a finite, non-zero gradient"""
    model = _backbone(torch.bfloat16)
    want, w = _backbone_reference(model, torch.bfloat16)
    gref = torch.cat([w[p.iseg_name].grad.reshape(-1) for p in model.parameters()])
    err = {}
    for mode in ("0", "1"):
        os.environ["ISEG_GEMMA_FUSED"] = mode
        out, grads = _backbone_run(model, torch.bfloat16)
        assert torch.isfinite(out).all()
        for p in model.parameters():
            g = grads[p.iseg_name]
            assert torch.isfinite(g).all() and g.abs().max().item() > 0, (mode, p.iseg_name)
        gvec = torch.cat([grads[p.iseg_name].reshape(-1) for p in model.parameters()])
        err[mode] = (_rel(out, want), _rel(gvec, gref))
        print(f"mode {mode}: output error {err[mode][0]:.3e}, gradient error {err[mode][1]:.3e}")
    assert err["1"][0] <= 1.5 * err["0"][0] and err["1"][1] <= 1.5 * err["0"][1], err
