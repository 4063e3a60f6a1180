"""The fused MBConv tail (functional.bn_swish_se, csrc/mbconv.hip): BN -> swish -> squeeze-excite -> gate, forward (squeeze / excite / gate)
and backward (reduce / excite-backward / apply), against fp64 autograd on the CPU -- fp32 and bf16 storage, training and moving statistics,
odd H*W, Cse in {1, 4, 10, 48}, N in {1, 3, 16} -- two runs bit for bit, and the fused block against the composed one (ISEG_MBCONV_FUSED=0)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS, MOMENTUM = 1e-3, 0.9

SHAPES = [      # N, H, W, C, Cse
    (1, 7, 9, 32, 1),
    (3, 15, 13, 96, 4),
    (16, 5, 7, 240, 10),
    (3, 9, 11, 1152, 48),
    (16, 33, 31, 32, 8),      # two row parts per sample
    (1, 129, 127, 16, 4),     # sixteen row parts
]


@pytest.fixture(autouse=True)
def _restore_policy():
    from iseg_amd import nn

    yield
    nn.set_compute_dtype(torch.float32)


def _rel(a, b):
    return (a.detach().cpu().double() - b).abs().max().item() / max(b.abs().max().item(), 1e-12)


def _params(C, Cse, seed):
    g = torch.Generator().manual_seed(seed)
    t = {
        "gamma": torch.rand(C, generator=g) + 0.5, "beta": torch.randn(C, generator=g) * 0.3,
        "W1": torch.randn(1, 1, C, Cse, generator=g) * C ** -0.5, "b1": torch.randn(Cse, generator=g) * 0.1,
        "W2": torch.randn(1, 1, Cse, C, generator=g) * Cse ** -0.5, "b2": torch.randn(C, generator=g) * 0.1,
        "mm": torch.randn(C, generator=g) * 0.2, "mv": torch.rand(C, generator=g) + 0.5,
    }
    return t


def _reference(x, p, training, dO):
    """fp64 autograd; returns out, dict of gradients (x, gamma, beta, W1, b1, W2, b2) and the batch mean / biased variance"""
    x = x.double().clone().requires_grad_(True)
    q = {k: v.double().clone().requires_grad_(k not in ("mm", "mv")) for k, v in p.items()}
    C, Cse = q["W1"].shape[2], q["W1"].shape[3]
    if training:
        mean, var = x.mean(dim=(0, 1, 2)), x.var(dim=(0, 1, 2), unbiased=False)
    else:
        mean, var = q["mm"], q["mv"]
    z = (x - mean) * torch.rsqrt(var + EPS) * q["gamma"] + q["beta"]
    a = z * torch.sigmoid(z)
    m = a.mean(dim=(1, 2))
    h = m @ q["W1"].reshape(C, Cse) + q["b1"]
    h = h * torch.sigmoid(h)
    gate = torch.sigmoid(h @ q["W2"].reshape(Cse, C) + q["b2"])
    out = a * gate[:, None, None, :]
    out.backward(dO.double())
    grads = {"x": x.grad}
    grads.update({k: q[k].grad for k in ("gamma", "beta", "W1", "b1", "W2", "b2")})
    return out.detach(), grads, mean.detach(), var.detach()


def _fused(x, p, training, dO, dtype):
    from iseg_amd import functional as F
    from iseg_amd import nn

    nn.set_compute_dtype(dtype)
    dev = "cuda"
    prm = {k: torch.nn.Parameter(v.clone().to(dev), requires_grad=k not in ("mm", "mv")) for k, v in p.items()}
    mm, mv = prm["mm"].data.clone(), prm["mv"].data.clone()
    xd = x.to(dev).to(dtype).requires_grad_(True)
    assert F.bn_swish_se_supported(xd, p["W1"].shape[-1])
    out = F.bn_swish_se(xd, prm["gamma"], prm["beta"], mm, mv, EPS, MOMENTUM, training, prm["W1"], prm["b1"], prm["W2"], prm["b2"], sync=False)
    out.backward(dO.to(dev).to(dtype))
    torch.cuda.synchronize()
    grads = {"x": xd.grad}
    grads.update({k: prm[k].grad for k in ("gamma", "beta", "W1", "b1", "W2", "b2")})
    return out.detach(), grads, mm, mv


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_fused_tail_fp32_matches_fp64(cuda, shape, training):
    N, H, W, C, Cse = shape
    g = torch.Generator().manual_seed(N * 1000 + C + Cse)
    x = torch.randn(N, H, W, C, generator=g) * 1.5 + 0.3
    dO = torch.randn(N, H, W, C, generator=g)
    p = _params(C, Cse, C + Cse)
    out, grads, mm, mv = _fused(x, p, training, dO, torch.float32)
    want, wg, mean, var = _reference(x, p, training, dO)
    assert _rel(out, want) < 1e-5
    for k in wg:
        assert _rel(grads[k], wg[k]) < 1e-5, (k, _rel(grads[k], wg[k]))
    if training:      # the moving statistics are updated exactly as by _BatchNormTrainFn
        assert _rel(mm, p["mm"].double() * MOMENTUM + mean * (1 - MOMENTUM)) < 1e-5
        assert _rel(mv, p["mv"].double() * MOMENTUM + var * (1 - MOMENTUM)) < 1e-5
    else:
        assert torch.equal(mm.cpu(), p["mm"]) and torch.equal(mv.cpu(), p["mv"])


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3], SHAPES[4]])
def test_fused_tail_bf16_matches_fp64(cuda, shape, training):
    """bf16 storage of x / out / dO / dx, fp32 arithmetic: the reference runs on the bf16-rounded x and dO; bands as for the bf16 MLP kernels"""
    N, H, W, C, Cse = shape
    g = torch.Generator().manual_seed(7 + C)
    x = (torch.randn(N, H, W, C, generator=g) * 1.5 + 0.3).bfloat16().float()
    dO = torch.randn(N, H, W, C, generator=g).bfloat16().float()
    p = _params(C, Cse, 3 + Cse)
    out, grads, _, _ = _fused(x, p, training, dO, torch.bfloat16)
    assert out.dtype == torch.bfloat16 and grads["x"].dtype == torch.bfloat16
    want, wg, _, _ = _reference(x, p, training, dO)
    assert _rel(out, want) < 1e-2
    for k in wg:
        assert _rel(grads[k], wg[k]) < 1.5e-2, (k, _rel(grads[k], wg[k]))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fused_tail_two_runs_bit_identical(cuda, dtype):
    N, H, W, C, Cse = SHAPES[3]
    g = torch.Generator().manual_seed(5)
    x = torch.randn(N, H, W, C, generator=g)
    dO = torch.randn(N, H, W, C, generator=g)
    p = _params(C, Cse, 9)
    a = _fused(x, p, True, dO, dtype)
    b = _fused(x, p, True, dO, dtype)
    assert torch.equal(a[0], b[0])
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])


def test_unsupported_shape_is_refused(cuda):
    from iseg_amd import _hip, kernels as K

    assert not K.mbconv_supported(2, 9, 12, 3)      # C % 8 != 0
    assert K.mbconv_supported(2, 9, 16, 3)
    x = torch.zeros(2, 3, 3, 12, device="cuda")
    z = torch.zeros(12, device="cuda")
    part = torch.zeros(1024, device="cuda")
    assert _hip.lib().iseg_bn_swish_se_squeeze(x.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), part.data_ptr(), 4096, 2, 9,
                                               12, 0, K.stream()) == -3      # ISEG_ERR_UNSUPPORTED


def _block(N, H, W, cin, training, seed):
    from iseg_amd import nn
    from iseg_amd.backbones.efficientnet import Block
    from iseg_amd.param_store import ParamStore
    from tests.util_models import randomize_parameters

    nn.set_compute_dtype(torch.float32)
    nn.set_device("cuda:0")
    blk = Block(filters_in=cin, filters_out=cin, kernel_size=5, strides=1, expand_ratio=6, se_ratio=0.25, drop_rate=0.0, name="fusedtest_")
    with nn.dry_run_scope():
        blk(torch.empty(N, H, W, cin, device="cuda"))
    blk._iseg_store = ParamStore(list(blk.parameters()))
    randomize_parameters(blk, seed)
    return blk


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("N,H,W,cin", [(3, 13, 11, 16), (16, 8, 8, 40)])
def test_fused_block_equals_composed_block(cuda, monkeypatch, training, N, H, W, cin):
    """one MBConv block (expand, depthwise, tail, project, residual) through both routes from the same weights: outputs and every gradient
    (input, gamma / beta of the depthwise BN, se_reduce / se_expand kernels and biases, all other weights) within 1e-5 in fp32"""
    g = torch.Generator().manual_seed(N + cin)
    x = torch.randn(N, H, W, cin, generator=g)
    dy = torch.randn(N, H, W, cin, generator=g)
    res = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("ISEG_MBCONV_FUSED", fused)
        blk = _block(N, H, W, cin, training, seed=4)
        xd = x.cuda().requires_grad_(True)
        y = blk(xd, training=training)
        y.backward(dy.cuda())
        torch.cuda.synchronize()
        res[fused] = (y.detach().cpu(), xd.grad.cpu(), {p.iseg_name: p.grad.detach().cpu().clone() for p in blk.parameters()},
                      {b.iseg_name: b.detach().cpu().clone() for b in blk.buffers() if hasattr(b, "iseg_name")})
    (yf, dxf, gf, bf), (yc, dxc, gc, bc) = res["1"], res["0"]

    def rel(a, b):
        return (a.double() - b.double()).abs().max().item() / max(b.double().abs().max().item(), 1e-12)

    assert rel(yf, yc) < 1e-5
    assert rel(dxf, dxc) < 1e-5
    assert set(gf) == set(gc) and any("se_reduce" in k for k in gf)
    bad = {k: rel(gf[k], gc[k]) for k in gf if rel(gf[k], gc[k]) >= 1e-5}
    assert not bad, bad
    for k in bf:
        assert rel(bf[k], bc[k]) < 1e-5, k


def test_misaligned_tensors_route_to_the_composed_path(cuda):
    """the host predicate refuses what the kernels would refuse (a contiguous x or a per-channel vector off 16-byte alignment), so
    Block._bn_swish_se takes the composed route instead of raising"""
    from iseg_amd import functional as F

    N, H, W, C, Cse = 2, 5, 7, 32, 4
    flat = torch.randn(N * H * W * C + 1, device="cuda")
    good, bad = flat[:-1].view(N, H, W, C), flat[1:].view(N, H, W, C)
    vec = torch.ones(C + 1, device="cuda")
    assert F.bn_swish_se_supported(good, Cse, vec[:C])
    assert not F.bn_swish_se_supported(bad, Cse, vec[:C])
    assert not F.bn_swish_se_supported(good, Cse, vec[1:])
    assert F.bn_swish_se_supported(bad.transpose(1, 2), Cse)      # non-contiguous: copied into an aligned buffer first


def test_inference_backward_reads_the_statistics_of_its_own_call(cuda):
    """an inference-mode call followed by a training-mode call that updates the moving statistics in place: the first call's backward still
    runs, with the statistics it was evaluated with"""
    from iseg_amd import functional as F

    N, H, W, C, Cse = 3, 9, 11, 96, 4
    g = torch.Generator().manual_seed(12)
    x = torch.randn(N, H, W, C, generator=g)
    dO = torch.randn(N, H, W, C, generator=g)
    p = _params(C, Cse, 21)
    prm = {k: torch.nn.Parameter(v.clone().cuda(), requires_grad=k not in ("mm", "mv")) for k, v in p.items()}
    mm, mv = prm["mm"].data.clone(), prm["mv"].data.clone()
    xd = x.cuda().requires_grad_(True)
    args = (prm["W1"], prm["b1"], prm["W2"], prm["b2"])
    out = F.bn_swish_se(xd, prm["gamma"], prm["beta"], mm, mv, EPS, MOMENTUM, False, *args, sync=False)
    F.bn_swish_se(x.cuda() * 2.0, prm["gamma"], prm["beta"], mm, mv, EPS, MOMENTUM, True, *args, sync=False)      # moves mm / mv in place
    assert not torch.equal(mm.cpu(), p["mm"])
    out.backward(dO.cuda())
    _, want, _, _ = _reference(x, p, False, dO)
    assert _rel(xd.grad, want["x"]) < 1e-5
