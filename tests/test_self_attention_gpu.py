"""SelfAttention (iseg_amd/layers/self_attention.py) and its fused attention core (csrc/selfattn.hip: 64-wide query / key, wide value) against the
fp64 restatement of layers/self_attention.py:65-93 in tests/self_attention_ref.py: the core on both routes (fused, and ISEG_SELFATTN_FUSED=0: the
materialised route of F.attention_packed), pitched and aliased operands, run-to-run identity, peaked rows, the absence of a T x T tensor, and the
layer with every parameter gradient."""
import functools
import os

import pytest
import torch

from tests import self_attention_ref as R
from tests.test_kernels_gpu import DTYPES, rnd
from tests.util_models import randomize_parameters

pytestmark = pytest.mark.gpu

# (B, T, dv): a single token; exact, +1 and +2 ragged tiles; more than one value slab; a slab count that is no power of two; the upper bound
CASES = [(2, 1, 64), (3, 64, 64), (1, 65, 128), (2, 130, 512), (1, 197, 192), (1, 320, 1024)]
SCALES = [1.0, 64 ** -0.5]
DK = 64


@functools.lru_cache(maxsize=None)
def _case(B, T, dv, scale, qk_std=0.35):
    """bf16-rounded host operands (q, k about qk_std * N(0,1): unscaled scores of standard deviation 64^0.5 * qk_std^2 ~ 1; v, dout N(0,1)) and the
    restatement's fp64 output and gradients, computed once and never modified"""
    host = [(rnd((B, T, DK), 1) * qk_std).to(torch.bfloat16), (rnd((B, T, DK), 2) * qk_std).to(torch.bfloat16),
            rnd((B, T, dv), 3).to(torch.bfloat16), rnd((B, T, dv), 4).to(torch.bfloat16)]
    q, k, v = (t.double().requires_grad_(True) for t in host[:3])
    out = R.core(q, k, v, scale)
    out.backward(host[3].double())
    return host, out.detach(), (q.grad, k.grad, v.grad)


def _run(host, scale, mode):
    """forward + backward of F.self_attention_core on one route -> (out, dq, dk, dv) as fp64 host tensors"""
    from iseg_amd import functional as F

    os.environ["ISEG_SELFATTN_FUSED"] = mode
    q, k, v = (t.cuda().requires_grad_(True) for t in host[:3])
    out = F.self_attention_core(q, k, v, scale)
    assert out.grad_fn is not None and tuple(out.shape) == tuple(v.shape) and out.dtype == torch.bfloat16
    assert type(out.grad_fn).__name__.startswith("_SelfAttentionFn") == (mode == "1")
    out.backward(host[3].cuda())
    return tuple(t.detach().cpu().double() for t in (out, q.grad, k.grad, v.grad))


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
        os.environ.pop("ISEG_SELFATTN_FUSED", None)
        nn.set_compute_dtype(torch.float32)


@pytest.mark.parametrize("scale", SCALES, ids=["unscaled", "scaled"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_core_both_routes_against_fp64(cuda, bf16, case, scale):
    """bounds of test_inference_flash_attention_matches_materialised_route_and_oracle: relative Frobenius error 1.5e-2 for the output, 3e-2 for each
    of dq, dk, dv on its own (with that test's floor for slices that are exactly zero at T = 1), fused against composed within 4e-2 of the
    composed maximum; fp64 is the yardstick for both routes"""
    from iseg_amd import functional as F

    host, want, grads = _case(*case, scale)
    gnorm = sum(g.norm().item() ** 2 for g in grads) ** 0.5
    res = {}
    for mode in ("1", "0"):
        res[mode] = _run(host, scale, mode)
        out = res[mode][0]
        print(f"mode {mode} out rel {_rel(out, want):.3e} " + " ".join(f"{n} {(a - r).norm().item():.3e}/{r.norm().item():.3e}"
                                                                     for n, a, r in zip(("dq", "dk", "dv"), res[mode][1:], grads)))
    for mode in ("1", "0"):
        out = res[mode][0]
        assert all(torch.isfinite(t).all() for t in res[mode]), mode
        assert _rel(out, want) < 1.5e-2, mode
        for name, a, r in zip(("dq", "dk", "dv"), res[mode][1:], grads):
            assert (a - r).norm().item() <= 3e-2 * max(r.norm().item(), 1e-3 * gnorm), (mode, name)
    assert (res["1"][0] - res["0"][0]).abs().max() < 4e-2 * res["0"][0].abs().max()
    # inference: the forward without the log-sum-exp vector gives the training forward's bits
    os.environ["ISEG_SELFATTN_FUSED"] = "1"
    with torch.no_grad():
        y = F.self_attention_core(*(t.cuda() for t in host[:3]), scale)
    assert y.grad_fn is None and torch.equal(y.cpu().double(), res["1"][0])


def test_core_pitched_and_aliased_operands(cuda, bf16):
    """q | k | v as column ranges of one [B, T, 64 + 64 + dv] tensor (row pitch 640, bases 128 B apart) give the bits of separate tensors; with k
    aliasing q the kernels read one buffer, and the gradient that reaches it is dq + dk"""
    from iseg_amd import functional as F
    from iseg_amd import kernels as K

    B, T, dv = 2, 130, 512
    host, _, _ = _case(B, T, dv, 1.0)
    os.environ["ISEG_SELFATTN_FUSED"] = "1"
    sep = [t.cuda().requires_grad_(True) for t in host[:3]]
    dout = host[3].cuda()
    y = F.self_attention_core(*sep, 1.0)
    y.backward(dout)
    packed = torch.cat(host[:3], dim=-1).cuda().requires_grad_(True)
    views = (packed[..., :DK], packed[..., DK:2 * DK], packed[..., 2 * DK:])
    assert all(not t.is_contiguous() and K._pitched(t)[1] == 2 * DK + dv and K._pitched(t)[0].data_ptr() == t.data_ptr() for t in views)
    yp = F.self_attention_core(*views, 1.0)
    yp.backward(dout)
    assert torch.equal(yp, y)
    assert torch.equal(packed.grad, torch.cat([t.grad for t in sep], dim=-1))
    # k is q
    q2, k2 = (host[0].cuda().requires_grad_(True) for _ in range(2))
    v2 = host[2].cuda().requires_grad_(True)
    y2 = F.self_attention_core(q2, k2, v2, 1.0)
    y2.backward(dout)
    qa, va = host[0].cuda().requires_grad_(True), host[2].cuda().requires_grad_(True)
    ya = F.self_attention_core(qa, qa, va, 1.0)
    ya.backward(dout)
    assert torch.equal(ya, y2) and torch.equal(va.grad, v2.grad)
    assert torch.equal(qa.grad, q2.grad + k2.grad)
    want = R.core(*(t.double() for t in (host[0], host[0], host[2])), 1.0)
    assert _rel(ya.detach().cpu().double(), want) < 1.5e-2


def test_core_two_runs_are_bit_identical(cuda, bf16):
    from iseg_amd import kernels as K

    host, _, _ = _case(2, 130, 512, 1.0)
    q, k, v, dout = (t.cuda() for t in host)
    runs = []
    for _ in range(2):
        out, lse = K.self_attention_fwd(q, k, v, 1.0, True)
        runs.append((out, lse) + K.self_attention_bwd(q, k, v, out, dout, lse, 1.0))
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_core_peaked_rows(cuda, bf16):
    """q, k about 2.5 * N(0,1): scores 64^0.5 * 6.25 = 50 in standard deviation, four of them ~ +-200 at T = 130, scale 1.  The materialised route
    rounds such scores to bf16 before its softmax and the fused kernels keep them in fp32, so the two round P at different points: the bound for
    each fused result is 1.5 x the error the composed route itself has against fp64 on the same inputs.  Range used: +-200 (the composed route
    is finite there)."""
    B, T, dv = 1, 130, 128
    host, want, grads = _case(B, T, dv, 1.0, 2.5)
    s = torch.matmul(host[0].double(), host[1].double().transpose(1, 2))
    assert 150.0 < s.abs().max().item() < 300.0, s.abs().max().item()
    composed = _run(host, 1.0, "0")
    fused = _run(host, 1.0, "1")
    assert all(torch.isfinite(t).all() for t in composed), "composed route not finite at this range"
    assert all(torch.isfinite(t).all() for t in fused)
    for name, a, c, r in zip(("out", "dq", "dk", "dv"), fused, composed, (want,) + grads):
        print(f"{name}: fused {(a - r).norm().item():.3e} composed {(c - r).norm().item():.3e} of {r.norm().item():.3e}")
        assert (a - r).norm().item() <= 1.5 * (c - r).norm().item(), name


def test_core_keeps_no_t_by_t_tensor(cuda, bf16):
    """peak device memory above the level before a forward + backward at B = 1, T = 2048, dv = 128: below the 8 MiB of one bf16 probability tensor
    on the fused route (operands' gradients, output and the two float vectors are about 3 MiB); above it on the composed route, which shows
    that the probe sees such a tensor"""
    from iseg_amd import functional as F

    B, T, dv = 1, 2048, 128
    q, k = ((rnd((B, T, DK), s) * 0.35).to(torch.bfloat16).cuda() for s in (1, 2))
    v, dout = (rnd((B, T, dv), s).to(torch.bfloat16).cuda() for s in (3, 4))
    peak = {}
    for mode in ("0", "1"):
        os.environ["ISEG_SELFATTN_FUSED"] = mode
        ops = [t.clone().requires_grad_(True) for t in (q, k, v)]
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        F.self_attention_core(*ops, 1.0).backward(dout)
        torch.cuda.synchronize()
        peak[mode] = torch.cuda.max_memory_allocated() - base
        del ops
    print(f"peak above base: fused {peak['1']} composed {peak['0']}")
    assert peak["1"] < B * T * T * 2 < peak["0"], peak


def test_core_default_route(cuda, bf16):
    """ISEG_SELFATTN_FUSED unset: inference runs on the fused kernels; a training step takes the composed route (the faster one while its
    tensors fit) until the [B, T, T] probabilities and their gradient together pass a quarter of the device's memory"""
    from iseg_amd import functional as F

    os.environ.pop("ISEG_SELFATTN_FUSED", None)
    host, want, _ = _case(1, 65, 128, 1.0)
    ops = [t.cuda().requires_grad_(True) for t in host[:3]]
    y = F.self_attention_core(*ops, 1.0)
    assert type(y.grad_fn).__name__.startswith("_AttentionFn")
    os.environ["ISEG_SELFATTN_FUSED"] = "1"
    with torch.no_grad():
        forced = F.self_attention_core(*ops, 1.0)
    os.environ.pop("ISEG_SELFATTN_FUSED")
    with torch.no_grad():
        assert torch.equal(F.self_attention_core(*ops, 1.0), forced)
    assert _rel(forced.cpu().double(), want) < 1.5e-2
    dev = ops[0].device
    total = torch.cuda.get_device_properties(dev).total_memory
    assert not F._self_attention_route(16, 4096, dev, True) and F._self_attention_route(16, 4096, dev, False)
    big_T = int((total / 4 / 4) ** 0.5) + 64      # one sample whose 2 * T * T * 2 bytes pass total / 4
    assert F._self_attention_route(1, big_T, dev, True) and not F._self_attention_route(1, big_T // 2, dev, True)


def test_core_refuses_unsupported_calls_on_the_device(cuda, bf16):
    from iseg_amd import _hip
    from iseg_amd import kernels as K

    q = torch.zeros(1, 8, 32, dtype=torch.bfloat16, device="cuda")
    v = torch.full((1, 8, 64), 3.0, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(_hip.HipCallError):
        K.self_attention_fwd(q, q, v, 1.0, False)
    q = torch.zeros(1, 8, 64, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(_hip.HipCallError):
        K.self_attention_fwd(q, q, v[..., :40], 1.0, False)


# ---- the layer ------------------------------------------------------------------------------------------------------------------------------
def _setup(layer, build_inputs, seed=7):
    from iseg_amd import nn
    from iseg_amd.param_store import ParamStore

    with nn.dry_run_scope():
        layer(build_inputs)
    layer._iseg_store = ParamStore(list(layer.parameters()))
    randomize_parameters(layer, seed)
    layer._iseg_store.sync_shadow()


def _check_grads(layer, w, tol, l2=False, skip=()):
    gmax = max(w[p.iseg_name].grad.abs().max().item() for p in layer.parameters() if w[p.iseg_name].grad is not None)
    bad = {}
    for p in layer.parameters():
        r = w[p.iseg_name].grad
        if r is None or p.iseg_name.endswith(tuple(skip)) and skip:
            continue
        d = p.grad.detach().cpu().double() - r
        if l2:
            e = d.norm().item() / max(r.norm().item(), 1e-3 * gmax * r.numel() ** 0.5)
        else:
            e = d.abs().max().item() / max(r.abs().max().item(), 1e-3 * gmax)
        if e > tol:
            bad[p.iseg_name] = e
    assert not bad, bad


def _lrel(a, b):
    a = a.detach().cpu()
    d = a.double() - b
    if a.dtype == torch.bfloat16:
        return d.norm().item() / max(b.norm().item(), 1e-8)
    return d.abs().max().item() / max(b.abs().max().item(), 1e-8)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("apply_scale", [False, True], ids=["unscaled", "scaled"])
@pytest.mark.parametrize("out_projection", [False, True], ids=["plain", "outproj"])
@pytest.mark.parametrize("shared_querykey", [False, True], ids=["qk", "sharedqk"])
@pytest.mark.parametrize("shape,filters", [((2, 5, 13, 48), 128), ((1, 8, 8, 32), 64)], ids=["2x5x13x48-f128", "1x8x8x32-f64"])
def test_layer_forward_and_gradients(cuda, monkeypatch, dtype, shape, filters, shared_querykey, out_projection, apply_scale):
    """output, input gradient and every weight gradient against the restatement carrying the same weights, at the bounds of test_mhsa_layer
    (fp32: 2e-5 / 2e-4 / 2e-4 in the max-norm; bf16: 3e-2 / 5e-2 / 6e-2 in relative L2).  fp32 runs on the composed route, bf16 on the
    fused kernels (ISEG_SELFATTN_FUSED=1: at these sizes a training step would otherwise take the composed route).
    The input is 0.35 * N(0,1), so that the projected queries and keys give unscaled scores of order 1 as in the core tests."""
    from iseg_amd import kernels as K
    from iseg_amd import nn
    from iseg_amd.layers.self_attention import SelfAttention
    from oracle import models as OM

    nn.set_compute_dtype(dtype)
    nn.set_device("cuda:0")
    os.environ["ISEG_SELFATTN_FUSED"] = "1"
    try:
        layer = SelfAttention(guided_filters=64, filters=filters, shared_querykey=shared_querykey, apply_scale=apply_scale,
                              use_out_projection=out_projection, name="sa")
        _setup(layer, torch.empty(shape, dtype=dtype, device="cuda"))
        f32 = dtype == torch.float32
        x = (rnd(shape, 1) * 0.35).to(dtype)
        xg = x.cuda().requires_grad_(True)
        fused_calls = []
        fwd = K.self_attention_fwd
        monkeypatch.setattr(K, "self_attention_fwd", lambda *a, **kw: fused_calls.append(1) or fwd(*a, **kw))
        y = layer(xg, training=True)
        assert len(fused_calls) == (0 if f32 else 1)
        assert tuple(y.shape) == (*shape[:3], filters) and y.dtype == dtype
        w = {k_: v.requires_grad_(True) for k_, v in OM.export_weights(layer).items()}
        xr = x.double().requires_grad_(True)
        yr = R.layer(w, "sa", xr, shared_querykey=shared_querykey, apply_scale=apply_scale, use_out_projection=out_projection)
        print(f"out {_lrel(y, yr.detach()):.3e}")
        assert _lrel(y, yr.detach()) < (2e-5 if f32 else 3e-2)
        dy = rnd(y.shape, 2).to(dtype)
        y.backward(dy.cuda())
        yr.backward(dy.double())
        print(f"dx {_lrel(xg.grad, xr.grad):.3e}")
        assert _lrel(xg.grad, xr.grad) < (2e-4 if f32 else 5e-2)
        # the key bias shifts every score of a row by the same amount: its gradient is analytically zero (rounding noise only)
        _check_grads(layer, w, 2e-4 if f32 else 6e-2, l2=not f32, skip=("key_conv/bias",))
    finally:
        os.environ.pop("ISEG_SELFATTN_FUSED", None)
        nn.set_compute_dtype(torch.float32)


def test_layer_dropouts(cuda, monkeypatch):
    """training=False: both dropouts are identities (the restatement's result, on the fused kernels); attention dropout in training takes the
    composed route, stays finite and changes the output"""
    from iseg_amd import kernels as K
    from iseg_amd import nn
    from iseg_amd.layers.self_attention import SelfAttention
    from oracle import models as OM

    nn.set_compute_dtype(torch.bfloat16)
    nn.set_device("cuda:0")
    try:
        shape = (2, 5, 13, 48)
        layer = SelfAttention(filters=64, attention_dropout_rate=0.5, feature_dropout_rate=0.5, name="sa")
        _setup(layer, torch.empty(shape, dtype=torch.bfloat16, device="cuda"))
        x = (rnd(shape, 1) * 0.35).to(torch.bfloat16)
        calls = []
        fwd = K.self_attention_fwd
        monkeypatch.setattr(K, "self_attention_fwd", lambda *a, **kw: calls.append(1) or fwd(*a, **kw))
        with torch.no_grad():
            y_eval = layer(x.cuda(), training=False)
            assert len(calls) == 1
            y_train = layer(x.cuda(), training=True)
            assert len(calls) == 1
        yr = R.layer(OM.export_weights(layer), "sa", x.double())
        assert _lrel(y_eval, yr) < 3e-2
        assert torch.isfinite(y_train).all() and not torch.equal(y_train, y_eval)
        only_attention = SelfAttention(filters=64, attention_dropout_rate=0.5, name="sa")
        _setup(only_attention, torch.empty(shape, dtype=torch.bfloat16, device="cuda"))
        with torch.no_grad():      # (same name, same seed: the weights of `layer`)
            y_train = only_attention(x.cuda(), training=True)
        assert len(calls) == 1
        assert torch.isfinite(y_train).all() and not torch.equal(y_train, y_eval)
    finally:
        nn.set_compute_dtype(torch.float32)
