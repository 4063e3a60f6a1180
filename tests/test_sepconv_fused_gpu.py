"""The fused Xception separable unit (functional.sepconv_unit, csrc/sepconv.hip): relu -> depthwise 3 x 3 -> BN folded into the pointwise
GEMM, forward and backward, against fp64 CPU autograd of the composed unit -- fp32 and bf16 storage, training and moving statistics, stride 1
and 2 on even and odd sizes, dilation 1 / 2 / 4, C in {8, 64, 728, 1024}, N in {1, 3, 16}, and one case with a large per-channel mean.
Also: the statistics message, run-to-run bit identity, the predicate's refusals (which fall back to the composed path without error), an
inference backward after an in-place update of the moving statistics, and the fused Xception unit against the composed one."""
import pytest
import torch

from oracle import tf_ops as O

pytestmark = pytest.mark.gpu

KEYS = ("v", "dx", "ddw", "dpw", "dgamma", "dbeta", "moving_mean", "moving_variance")


@pytest.fixture(autouse=True)
def _restore_policy():
    from iseg_amd import nn

    yield
    nn.set_compute_dtype(torch.float32)


def _unit(C, Cout, stride, dil, dtype, seed=0, shift=False):
    from iseg_amd import nn
    from iseg_amd.backbones.xception import XceptionDepthWiseConv
    from iseg_amd.param_store import ParamStore

    nn.set_compute_dtype(dtype)
    nn.set_device("cuda:0")
    u = XceptionDepthWiseConv(2, 1, Cout, strides=(stride, stride))
    u.atrous_rates = (dil, dil)
    u.build((1, 1, 1, C))
    dw, bn, pw = u.depthwise_conv, u.depthwise_bn, u.pointwise_conv
    u._iseg_store = ParamStore([dw.depthwise_kernel, bn.gamma, bn.beta, pw.kernel])
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        if shift:      # all-positive depthwise taps on a shifted input: |mean| / std of z is about 4
            dw.depthwise_kernel.copy_((0.1 + 0.02 * torch.randn(3, 3, C, 1, generator=g)).cuda())
        else:
            dw.depthwise_kernel.copy_((torch.randn(3, 3, C, 1, generator=g) / 3).cuda())
        bn.gamma.copy_((torch.rand(C, generator=g) + 0.5).cuda())
        bn.beta.copy_((torch.randn(C, generator=g) * 0.1).cuda())
        pw.kernel.copy_((torch.randn(1, 1, C, Cout, generator=g) * C ** -0.5).cuda())
        bn.moving_mean.copy_((torch.randn(C, generator=g) * 0.1).cuda())
        bn.moving_variance.copy_((torch.rand(C, generator=g) + 0.5).cuda())
    u._iseg_store.sync_shadow()
    u._init_stats = (bn.moving_mean.clone(), bn.moving_variance.clone())
    return u


def _run(u, x, dv, training, stride, dil, fused, monkeypatch):
    from iseg_amd import functional as F

    monkeypatch.setenv("ISEG_SEPCONV_FUSED", "1" if fused else "0")
    dw, bn, pw = u.depthwise_conv, u.depthwise_bn, u.pointwise_conv
    u._iseg_store.zero_grad()
    bn.moving_mean.copy_(u._init_stats[0])
    bn.moving_variance.copy_(u._init_stats[1])
    xg = x.detach().requires_grad_(True)      # an alias: a misaligned view stays misaligned
    v = F.sepconv_unit(xg, dw.depthwise_kernel, bn, pw.kernel, training, strides=stride, dilation=dil)
    v.backward(dv)
    torch.cuda.synchronize()
    return dict(v=v.detach().clone(), dx=xg.grad.clone(), ddw=dw.depthwise_kernel.grad.clone(), dpw=pw.kernel.grad.clone(),
                dgamma=bn.gamma.grad.clone(), dbeta=bn.beta.grad.clone(), moving_mean=bn.moving_mean.clone(),
                moving_variance=bn.moving_variance.clone())


def _reference(u, x, dv, training, stride, dil):
    """fp64 CPU autograd of relu -> depthwise -> BN -> 1 x 1"""
    dw, bn, pw = u.depthwise_conv, u.depthwise_bn, u.pointwise_conv
    p = {k: t.detach().cpu().double().requires_grad_(True) for k, t in
         dict(ddw=dw.depthwise_kernel, dgamma=bn.gamma, dbeta=bn.beta, dpw=pw.kernel).items()}
    mm, mv = (t.cpu().double() for t in u._init_stats)
    xd = x.detach().cpu().double().requires_grad_(True)
    z = O.depthwise_conv2d(torch.relu(xd), p["ddw"], None, stride, dil, "same")
    if training:
        y, mean, var = O.batch_norm_train(z, p["dgamma"], p["dbeta"], 1e-3)
        mm, mv = O.moving_update(mm, mean.detach(), 0.9), O.moving_update(mv, var.detach(), 0.9)
    else:
        y = O.batch_norm_infer(z, p["dgamma"], p["dbeta"], mm, mv, 1e-3)
    v = O.conv2d(y, p["dpw"], None, 1, 1, "same")
    v.backward(dv.detach().cpu().double())
    out = {k: t.grad for k, t in p.items()}
    out.update(v=v.detach(), dx=xd.grad, moving_mean=mm, moving_variance=mv)
    return out


def _err(got, want):
    return (got.detach().cpu().double() - want).abs().max().item() / max(want.abs().max().item(), 1e-12)


def _inputs(N, H, W, C, Cout, stride, dil, dtype, seed, shift=False):
    from iseg_amd.kernels import same_pad

    g = torch.Generator().manual_seed(seed + 100)
    x = torch.randn(N, H, W, C, generator=g) + (1.0 if shift else 0.0)
    Ho, Wo = same_pad(H, 3, stride, dil)[0], same_pad(W, 3, stride, dil)[0]
    dv = torch.randn(N, Ho, Wo, Cout, generator=g)
    return x.to("cuda", dtype), dv.to("cuda", dtype)


# N, H, W, C, Cout, stride, dilation
CASES = [
    (1, 9, 7, 8, 16, 1, 1),
    (3, 10, 12, 64, 32, 2, 1),
    (3, 11, 9, 64, 72, 2, 1),
    (3, 12, 10, 64, 128, 1, 2),
    (1, 13, 11, 8, 24, 1, 4),
    (16, 8, 8, 728, 728, 1, 1),
    (3, 7, 9, 728, 1024, 2, 1),
    (1, 6, 6, 1024, 64, 1, 2),
]


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("case", CASES, ids=[f"N{c[0]}_{c[1]}x{c[2]}_C{c[3]}to{c[4]}_s{c[5]}_d{c[6]}" for c in CASES])
def test_fp32_against_fp64(cuda, case, training, monkeypatch):
    N, H, W, C, Cout, s, d = case
    u = _unit(C, Cout, s, d, torch.float32, seed=sum(case))
    x, dv = _inputs(N, H, W, C, Cout, s, d, torch.float32, sum(case))
    got = _run(u, x, dv, training, s, d, True, monkeypatch)
    ref = _reference(u, x, dv, training, s, d)
    errs = {k: _err(got[k], ref[k]) for k in KEYS}
    bad = {k: v for k, v in errs.items() if v > 1e-4}
    assert not bad, bad


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("case", CASES, ids=[f"N{c[0]}_{c[1]}x{c[2]}_C{c[3]}to{c[4]}_s{c[5]}_d{c[6]}" for c in CASES])
def test_bf16_within_twice_composed_error(cuda, case, training, monkeypatch):
    N, H, W, C, Cout, s, d = case
    u = _unit(C, Cout, s, d, torch.bfloat16, seed=sum(case))
    x, dv = _inputs(N, H, W, C, Cout, s, d, torch.bfloat16, sum(case))
    fused = _run(u, x, dv, training, s, d, True, monkeypatch)
    composed = _run(u, x, dv, training, s, d, False, monkeypatch)
    ref = _reference(u, x, dv, training, s, d)
    bad = {}
    for k in KEYS:
        ef, ec = _err(fused[k], ref[k]), _err(composed[k], ref[k])
        if ef > 2 * ec + 1e-3:
            bad[k] = (ef, ec)
    assert not bad, bad


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_large_channel_mean(cuda, dtype, monkeypatch):
    """|mean| / std of z about 4: the fold's cancellation (z W' against c^T W, G against mean * dbeta) shows up here first"""
    N, H, W, C, Cout, s, d = 3, 10, 10, 64, 96, 1, 1
    u = _unit(C, Cout, s, d, dtype, seed=5, shift=True)
    x, dv = _inputs(N, H, W, C, Cout, s, d, dtype, 5, shift=True)
    z = O.depthwise_conv2d(torch.relu(x.cpu().double()), u.depthwise_conv.depthwise_kernel.detach().cpu().double(), None, 1, 1, "same")
    ratio = (z.mean((0, 1, 2)).abs() / z.std((0, 1, 2))).median().item()
    assert 2.5 < ratio < 8, ratio
    fused = _run(u, x, dv, True, s, d, True, monkeypatch)
    ref = _reference(u, x, dv, True, s, d)
    if dtype == torch.float32:
        errs = {k: _err(fused[k], ref[k]) for k in KEYS}
        assert not {k: v for k, v in errs.items() if v > 1e-4}, errs
    else:
        composed = _run(u, x, dv, True, s, d, False, monkeypatch)
        bad = {k: (_err(fused[k], ref[k]), _err(composed[k], ref[k])) for k in KEYS
               if _err(fused[k], ref[k]) > 2 * _err(composed[k], ref[k]) + 1e-3}
        assert not bad, bad


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("stride,H,W", [(1, 9, 11), (2, 10, 7)])
def test_stats_message(cuda, dtype, stride, H, W):
    """the packed [sum z | sum z^2 | count] message of iseg_bn_stats, over the stored z"""
    from iseg_amd import kernels as K

    C = 64
    g = torch.Generator().manual_seed(2)
    x = torch.randn(3, H, W, C, generator=g).to("cuda", dtype)
    w = (torch.randn(9, C, generator=g) / 3).cuda()
    z, packed = K.relu_dwconv3_stats(x, w, stride, 1, stats=True)
    zr = O.depthwise_conv2d(torch.relu(x.cpu().double()), w.cpu().double().reshape(3, 3, C, 1), None, stride, 1, "same")
    assert tuple(z.shape) == tuple(zr.shape)
    assert _err(z, zr) < (1e-5 if dtype == torch.float32 else 8e-3)
    zs = z.cpu().double().reshape(-1, C)      # the message sums the stored z
    want = torch.cat([zs.sum(0), (zs * zs).sum(0), torch.tensor([float(zs.shape[0])], dtype=torch.float64)])
    assert _err(packed, want) < 1e-5
    assert packed[-1].item() == zs.shape[0]
    z2, _ = K.relu_dwconv3_stats(x, w, stride, 1, stats=False)
    assert torch.equal(z, z2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_two_runs_bit_identical(cuda, dtype, monkeypatch):
    N, H, W, C, Cout, s, d = 16, 8, 8, 728, 728, 1, 1
    u = _unit(C, Cout, s, d, dtype, seed=4)
    x, dv = _inputs(N, H, W, C, Cout, s, d, dtype, 4)
    a = _run(u, x, dv, True, s, d, True, monkeypatch)
    b = _run(u, x, dv, True, s, d, True, monkeypatch)
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k


def test_predicate_refusals_fall_back(cuda, monkeypatch):
    from iseg_amd import functional as F

    # C % 8 != 0: refused by the predicate (the composed depthwise kernels need C % 8 == 0 as well, so no unit of that width exists)
    u = _unit(12, 16, 1, 1, torch.float32, seed=1)
    x, _ = _inputs(2, 6, 6, 12, 16, 1, 1, torch.float32, 1)
    assert not F.sepconv_supported(x, u.depthwise_conv.depthwise_kernel, u.depthwise_bn, u.pointwise_conv.kernel)
    # a misaligned (contiguous) view of x
    u = _unit(64, 32, 2, 1, torch.bfloat16, seed=2)
    x, dv = _inputs(2, 9, 9, 64, 32, 2, 1, torch.bfloat16, 2)
    buf = torch.empty(x.numel() + 1, dtype=x.dtype, device=x.device)
    xm = buf[1:].view(x.shape)
    xm.copy_(x)
    assert xm.data_ptr() % 16 and not F.sepconv_supported(xm, u.depthwise_conv.depthwise_kernel, u.depthwise_bn, u.pointwise_conv.kernel, 2)
    assert F.sepconv_supported(x, u.depthwise_conv.depthwise_kernel, u.depthwise_bn, u.pointwise_conv.kernel, 2)
    a = _run(u, xm, dv, True, 2, 1, True, monkeypatch)      # refused: the composed operators run on the view as it is
    b = _run(u, xm, dv, True, 2, 1, False, monkeypatch)
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k
    ref = _reference(u, x, dv, True, 2, 1)
    assert _err(a["v"], ref["v"]) < 2e-2
    # stride 2 with dilation 2 is never built by the surgery; the kernels refuse it
    from iseg_amd import kernels as K

    assert not K.sepconv_supported(1, 8, 8, 64, 2, 2, torch.float32)


def test_inference_backward_after_moving_stats_update(cuda, monkeypatch):
    """a moving-statistics forward, then a training-mode call that updates the moving statistics in place, then the first call's backward:
    it must use the statistics of its own forward"""
    from iseg_amd import functional as F

    monkeypatch.setenv("ISEG_SEPCONV_FUSED", "1")
    N, H, W, C, Cout = 2, 8, 8, 64, 32
    u = _unit(C, Cout, 1, 1, torch.float32, seed=9)
    x, dv = _inputs(N, H, W, C, Cout, 1, 1, torch.float32, 9)
    ref = _reference(u, x, dv, False, 1, 1)
    dw, bn, pw = u.depthwise_conv, u.depthwise_bn, u.pointwise_conv
    u._iseg_store.zero_grad()
    xg = x.clone().requires_grad_(True)
    v = F.sepconv_unit(xg, dw.depthwise_kernel, bn, pw.kernel, False)
    with torch.no_grad():
        F.sepconv_unit(x * 3 + 1, dw.depthwise_kernel, bn, pw.kernel, True)      # moves moving_mean / moving_variance in place
    assert not torch.equal(bn.moving_mean, u._init_stats[0])
    v.backward(dv)
    assert _err(v, ref["v"]) < 1e-4
    assert _err(xg.grad, ref["dx"]) < 1e-4
    assert _err(pw.kernel.grad, ref["dpw"]) < 1e-4
    assert _err(bn.gamma.grad, ref["dgamma"]) < 1e-4
    assert _err(dw.depthwise_kernel.grad, ref["ddw"]) < 1e-4


@pytest.mark.parametrize("training", [True, False])
def test_xception_unit_fused_matches_composed(cuda, training, monkeypatch):
    """the whole XceptionDepthWiseConv (pointwise BN included), fused against ISEG_SEPCONV_FUSED=0, fp32"""
    from iseg_amd import nn

    N, H, W, C, Cout = 3, 12, 12, 64, 128
    u = _unit(C, Cout, 2, 1, torch.float32, seed=13)
    u.pointwise_bn.build((1, 1, 1, Cout))
    u.pointwise_bn.built = True
    params = list(u.parameters())
    from iseg_amd.param_store import ParamStore

    u._iseg_store = ParamStore(params)
    x, _ = _inputs(N, H, W, C, Cout, 2, 1, torch.float32, 13)
    outs = {}
    for fused in (True, False):
        monkeypatch.setenv("ISEG_SEPCONV_FUSED", "1" if fused else "0")
        u._iseg_store.zero_grad()
        xg = x.clone().requires_grad_(True)
        y = u(xg, training=training)
        dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(1)).cuda()
        y.backward(dy)
        outs[fused] = (y.detach().clone(), xg.grad.clone(), {p.iseg_name: p.grad.clone() for p in params})
    assert nn.compute_dtype() == torch.float32
    (yf, dxf, gf), (yc, dxc, gc) = outs[True], outs[False]
    assert _err(yf, yc.cpu().double()) < 1e-4 and _err(dxf, dxc.cpu().double()) < 1e-4
    # a training-mode pointwise BN removes the per-channel mean of its input gradient, so the depthwise BN's dbeta is zero up to rounding:
    # errors are measured against the larger of the tensor's own scale and a small fraction of the largest gradient
    gmax = max(g.abs().max().item() for g in gc.values())
    for k in gf:
        err = (gf[k] - gc[k]).abs().max().item() / max(gc[k].abs().max().item(), 1e-2 * gmax)
        assert err < 1e-4, (k, err)
