"""The fused ResNet basic-block tail (csrc/resblock.hip through functional.resblock_tail): relu(bn2(z2) + avg_pool_s(bn0(z0) or x)) against
the fp64 restatement of tests/resnet_small_ref.py -- forward, dz2, the shortcut gradient, dgamma / dbeta of both BatchNorms and the moving
statistics -- for the four block kinds (identity / BN0 shortcut, stride 1 / 2), training and moving statistics, C in {32, 64, 128, 512} and odd
H x W (partial pooling windows); bf16 against the composed route's error; a large-mean case; run-to-run bit identity; refused inputs; and an
inference backward after an in-place update of the moving statistics."""
import pytest
import torch

from tests import resnet_small_ref as R

pytestmark = pytest.mark.gpu

KINDS = [(False, 1), (False, 2), (True, 1), (True, 2)]      # (BN0 shortcut, stride)


@pytest.fixture(autouse=True)
def _policy():
    from iseg_amd import nn

    nn.set_device("cuda:0")
    yield
    nn.set_compute_dtype(torch.float32)


def _bn(name, C, seed):
    from iseg_amd.layers.base_layers import BatchNormalization

    b = BatchNormalization(momentum=0.9, epsilon=1.001e-5, name=name)
    b.build((C,))
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        b.gamma.copy_(torch.rand(C, generator=g) + 0.5)
        b.beta.copy_(torch.randn(C, generator=g) * 0.3)
        b.moving_mean.copy_(torch.randn(C, generator=g) * 0.2)
        b.moving_variance.copy_(torch.rand(C, generator=g) + 0.5)
    return b


def _case(bn0, s, C, H=33, W=31, N=2, seed=0, mean=0.0):
    g = torch.Generator().manual_seed(seed)
    Ho, Wo = -(-H // s), -(-W // s)
    z2 = torch.randn(N, Ho, Wo, C, generator=g) + mean
    sc = torch.randn(N, H, W, C, generator=g) + mean
    dout = torch.randn(N, Ho, Wo, C, generator=g)
    layers = {"t_2_bn": _bn("t_2_bn", C, seed + 1)}
    if bn0:
        layers["t_0_bn"] = _bn("t_0_bn", C, seed + 2)
    return z2, sc, dout, layers


def _weights(layers):
    w = {}
    for name, b in layers.items():
        for k in ("gamma", "beta", "moving_mean", "moving_variance"):
            t = getattr(b, k).detach().cpu().double().clone()
            w[f"{name}/{k}"] = t.requires_grad_(k in ("gamma", "beta"))
    return w


def _run(z2, sc, dout, layers, s, training, dtype=torch.float32, z2_dev=None, sc_dev=None):
    """the product's tail on the GPU: (out, dz2, dsc, {param name: grad}, {moving name: value}) on the host in fp64"""
    from iseg_amd import functional as F
    from iseg_amd import nn

    nn.set_compute_dtype(dtype)
    for b in layers.values():
        for p in (b.gamma, b.beta):
            p.grad = None
    z = (z2_dev if z2_dev is not None else z2.to("cuda", dtype)).detach().requires_grad_(True)
    x = (sc_dev if sc_dev is not None else sc.to("cuda", dtype)).detach().requires_grad_(True)
    out = F.resblock_tail(z, layers["t_2_bn"], x, layers.get("t_0_bn"), s, training)
    out.backward(dout.to("cuda", dtype))
    grads = {f"{n}/{k}": getattr(b, k).grad.detach().cpu().double() for n, b in layers.items() for k in ("gamma", "beta")}
    moving = {f"{n}/{k}": getattr(b, k).detach().cpu().double().clone() for n, b in layers.items() for k in ("moving_mean", "moving_variance")}
    return out.detach().cpu().double(), z.grad.cpu().double(), x.grad.cpu().double(), grads, moving


def _ref(z2, sc, dout, w, s, bn0, training, mask=None):
    """fp64 tail; the backward takes the ReLU mask `mask` (the product's out > 0) when given: a pre-activation within rounding of zero may
    take the other branch in fp32 / bf16, which moves that element's gradient by O(1) and says nothing about the arithmetic"""
    new_stats = {}
    w = {k: v.detach().clone().requires_grad_(v.requires_grad) for k, v in w.items()}
    z = z2.double().requires_grad_(True)
    x = sc.double().requires_grad_(True)
    pre = R.tail_pre(w, "t", z, x, s, bn0, training, new_stats=new_stats)
    out = torch.relu(pre)
    (pre * mask if mask is not None else out).backward(dout.double())
    grads = {k: v.grad for k, v in w.items() if v.requires_grad}
    return out.detach(), z.grad, x.grad, grads, new_stats


def _against_ref(got, z2, sc, dout, w, s, bn0, training):
    return _ref(z2, sc, dout, w, s, bn0, training, mask=(got[0] > 0).double())


def _rel(a, b):
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-8)


def _check(got, want, tol, training):
    out, dz2, dsc, grads, moving = got
    rout, rdz2, rdsc, rgrads, rstats = want
    assert _rel(out, rout) < tol
    assert _rel(dz2, rdz2) < tol
    assert _rel(dsc, rdsc) < tol
    for k, v in rgrads.items():
        assert _rel(grads[k], v) < tol, k
    if training:
        for k, v in rstats.items():
            assert _rel(moving[k], v) < tol, k


@pytest.mark.parametrize("C", [32, 64, 128, 512])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("bn0,s", KINDS)
def test_tail_fp32_against_fp64(cuda, bn0, s, training, C):
    from iseg_amd import functional as F

    z2, sc, dout, layers = _case(bn0, s, C, seed=C + s)
    assert F.resblock_tail_supported(z2.cuda(), sc.cuda(), layers["t_2_bn"], layers.get("t_0_bn"), s)
    w = _weights(layers)
    got = _run(z2, sc, dout, layers, s, training)
    _check(got, _against_ref(got, z2, sc, dout, w, s, bn0, training), 1e-3, training)


@pytest.mark.parametrize("bn0,s", KINDS)
def test_tail_even_size_and_batch(cuda, bn0, s):
    z2, sc, dout, layers = _case(bn0, s, 64, H=16, W=24, N=3, seed=9)
    w = _weights(layers)
    got = _run(z2, sc, dout, layers, s, True)
    _check(got, _against_ref(got, z2, sc, dout, w, s, bn0, True), 1e-3, True)


@pytest.mark.parametrize("bn0,s", KINDS)
def test_tail_large_channel_mean(cuda, bn0, s):
    """inputs centred far from zero: the BatchNorm arithmetic must not lose the small deviations"""
    z2, sc, dout, layers = _case(bn0, s, 64, seed=4, mean=40.0)
    w = _weights(layers)
    got = _run(z2, sc, dout, layers, s, True)
    _check(got, _against_ref(got, z2, sc, dout, w, s, bn0, True), 1e-3, True)


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("bn0,s", KINDS)
def test_tail_bf16_within_twice_composed(cuda, monkeypatch, bn0, s, training):
    z2, sc, dout, layers = _case(bn0, s, 64, seed=11)
    w = _weights(layers)
    snapshot = {n: (b.moving_mean.clone(), b.moving_variance.clone()) for n, b in layers.items()}

    def errs(route):
        monkeypatch.setenv("ISEG_RESBLOCK_FUSED", "1" if route == "fused" else "0")
        with torch.no_grad():
            for n, b in layers.items():
                b.moving_mean.copy_(snapshot[n][0])
                b.moving_variance.copy_(snapshot[n][1])
        got = _run(z2, sc, dout, layers, s, training, dtype=torch.bfloat16)
        want = _against_ref(got, z2, sc, dout, w, s, bn0, training)
        return [_rel(got[i], want[i]) for i in range(3)] + [_rel(got[3][k], v) for k, v in want[3].items()]

    fused, composed = errs("fused"), errs("composed")
    for f, c in zip(fused, composed):
        assert f <= 2 * c + 2e-3, (fused, composed)


def test_tail_bit_identical_runs(cuda):
    z2, sc, dout, layers = _case(True, 2, 128, N=4, seed=5)
    snapshot = {n: (b.moving_mean.clone(), b.moving_variance.clone()) for n, b in layers.items()}
    runs = []
    for _ in range(2):
        with torch.no_grad():
            for n, b in layers.items():
                b.moving_mean.copy_(snapshot[n][0])
                b.moving_variance.copy_(snapshot[n][1])
        runs.append(_run(z2, sc, dout, layers, 2, True))
    a, b = runs
    for i in range(3):
        assert torch.equal(a[i], b[i])
    for k in a[3]:
        assert torch.equal(a[3][k], b[3][k]), k


def test_refused_inputs_fall_back(cuda):
    from iseg_amd import functional as F
    from iseg_amd import kernels as K

    # a contiguous view that starts 4 bytes into its buffer
    z2, sc, dout, layers = _case(True, 2, 64, seed=6)
    buf = torch.empty(z2.numel() + 1, device="cuda")
    z_view = buf[1:].view(z2.shape)
    z_view.copy_(z2.cuda())
    assert not F.resblock_tail_supported(z_view, sc.cuda(), layers["t_2_bn"], layers["t_0_bn"], 2)
    w = _weights(layers)
    got = _run(z2, sc, dout, layers, 2, True, z2_dev=z_view)
    _check(got, _against_ref(got, z2, sc, dout, w, 2, True, True), 1e-3, True)
    # C % 8 != 0: refused by the host predicate and by the kernels' own (the composed BatchNorm kernels need C % 8 == 0 as well)
    z2, sc, dout, layers = _case(False, 2, 12, seed=7)
    assert not F.resblock_tail_supported(z2.cuda(), sc.cuda(), layers["t_2_bn"], None, 2)
    assert not K.resblock_tail_supported(12, 2, torch.float32) and K.resblock_tail_supported(16, 2, torch.bfloat16)
    assert not K.resblock_tail_supported(16, 3, torch.float32)


def test_inference_backward_after_moving_update(cuda):
    """a moving-statistics forward, then a training-mode forward that updates the buffers in place, then the first call's backward: it reads
    the statistics of its own call"""
    from iseg_amd import functional as F

    z2, sc, dout, layers = _case(True, 1, 64, seed=8)
    w = _weights(layers)
    z = z2.cuda().requires_grad_(True)
    x = sc.cuda().requires_grad_(True)
    out = F.resblock_tail(z, layers["t_2_bn"], x, layers["t_0_bn"], 1, False)
    want = _ref(z2, sc, dout, w, 1, True, False, mask=(out.detach().cpu() > 0).double())
    with torch.no_grad():
        F.resblock_tail(z2.cuda() + 1.0, layers["t_2_bn"], sc.cuda() - 1.0, layers["t_0_bn"], 1, True)      # moves the buffers
    assert not torch.equal(layers["t_2_bn"].moving_mean.cpu().double(), w["t_2_bn/moving_mean"])
    out.backward(dout.cuda())
    assert _rel(out.detach().cpu().double(), want[0]) < 1e-3
    assert _rel(z.grad.cpu().double(), want[1]) < 1e-3
    assert _rel(x.grad.cpu().double(), want[2]) < 1e-3
    for k, v in want[3].items():
        n, p = k.split("/")
        assert _rel(getattr(layers[n], p).grad.cpu().double(), v) < 1e-3, k
