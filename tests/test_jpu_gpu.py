"""JointPyramidUpsampling (layers/jpu.py) and the ResNet-18 + JPU + ASPP head on the GPU, against the fp64 restatement tests/jpu_ref.py: the
layer's output, every input gradient and every parameter gradient with training and with moving statistics, on the fused route (F.jpu_tail,
csrc/jpu.hip) and on the composed one (ISEG_JPU_FUSED=0); the two routes against each other; trainable=False; one bf16 training step of the
whole model."""
import pytest
import torch

from oracle import models as OM
from tests import jpu_ref as R
from tests.util_models import randomize_parameters

pytestmark = pytest.mark.gpu

# the last three are used; the first, finer one must be ignored
SHAPES = [(2, 32, 40, 8), (2, 16, 20, 24), (2, 8, 10, 40), (2, 4, 5, 56)]


@pytest.fixture(autouse=True)
def _restore_policy():
    from iseg_amd import nn

    yield
    nn.set_compute_dtype(torch.float32)


def _rel(a, b):
    return (a.detach().cpu().double() - b).abs().max().item() / max(b.abs().max().item(), 1e-8)


def _layer(trainable=True, seed=11):
    from iseg_amd import nn
    from iseg_amd.layers.jpu import JointPyramidUpsampling
    from iseg_amd.param_store import ParamStore

    nn.set_compute_dtype(torch.float32)
    nn.set_device("cuda:0")
    jpu = JointPyramidUpsampling(width=16, trainable=trainable, name="jpu")
    with nn.dry_run_scope():
        jpu([torch.empty(s, device="cuda") for s in SHAPES])
    jpu._iseg_store = ParamStore(list(jpu.parameters()))
    randomize_parameters(jpu, seed)
    return jpu


def _inputs():
    return [torch.randn(s, generator=torch.Generator().manual_seed(20 + i)) for i, s in enumerate(SHAPES)]


def _run(jpu, xs, dy, training, fused, monkeypatch, stats0):
    monkeypatch.setenv("ISEG_JPU_FUSED", "1" if fused else "0")
    jpu._iseg_store.zero_grad()
    for b in jpu.buffers():
        b.copy_(stats0[b.iseg_name])
    xg = [x.cuda().requires_grad_(True) for x in xs]
    y = jpu(xg, training=training)
    y.backward(dy.cuda())
    torch.cuda.synchronize()
    return dict(y=y.detach().clone(), dx=[None if x.grad is None else x.grad.clone() for x in xg],
                grads={p.iseg_name: p.grad.clone() for p in jpu.parameters()}, stats={b.iseg_name: b.clone() for b in jpu.buffers()})


@pytest.fixture(scope="module")
def reference():
    """(layer weights, inputs, dy, {training: fp64 result}): computed once, shared, left unchanged"""
    cache = {}

    def get(jpu, training):
        if training not in cache:
            xs = _inputs()
            dy = torch.randn((2, 16, 20, 64), generator=torch.Generator().manual_seed(40))
            w = {k: v.requires_grad_(True) if not k.endswith(("moving_mean", "moving_variance")) else v for k, v in OM.export_weights(jpu).items()}
            xr = [x.double().requires_grad_(True) for x in xs]
            new_stats = {}
            yr = R.jpu_forward(w, xr, "jpu", training=training, new_stats=new_stats)
            yr.backward(dy.double())
            cache[training] = dict(xs=xs, dy=dy, y=yr.detach(), dx=[x.grad for x in xr], grads={k: v.grad for k, v in w.items() if v.requires_grad},
                                   stats=new_stats)
        return cache[training]

    return get


def _check(got, ref, tol, training):
    """parameter gradients in test_nasfpn's measure (max-norm, floored at 1e-3 of the largest gradient).  One kind is zero up to rounding: the
    depthwise bias in front of a training-mode BN, which removes any per-channel constant -- the reference leaves 1e-17, a relative error is
    meaningless, and what an fp32 route leaves is the rounding of the sum it forms.  That sum runs over the same terms dz_r, at the same
    scale, as the branch's depthwise-kernel gradient sum x dz_r (x of order one), so it is held to `tol` of THAT gradient's largest entry
    (the rule tests/test_jpu_fused_gpu.py applies with dbeta_r, which is zero as well inside the whole layer)."""
    assert tuple(got["y"].shape) == (2, 16, 20, 64)
    errs = {"y": _rel(got["y"], ref["y"])}
    assert got["dx"][0] is None and ref["dx"][0] is None, "the finer fourth endpoint must not be used"
    for i in (1, 2, 3):
        errs[f"dx{i}"] = _rel(got["dx"][i], ref["dx"][i])
    gmax = max(g.abs().max().item() for g in ref["grads"].values())
    for k, g in ref["grads"].items():
        if training and "/end_depthwise_conv_" in k and k.endswith("/bias"):
            assert g.abs().max().item() < 1e-9 * gmax      # the reference's own value: nothing
            errs[k] = got["grads"][k].abs().max().item() / ref["grads"][k[:-len("bias")] + "depthwise_kernel"].abs().max().item()
            continue
        errs[k] = (got["grads"][k].cpu().double() - g).abs().max().item() / max(g.abs().max().item(), 1e-3 * gmax)
    for k, s in ref["stats"].items():
        errs[k] = _rel(got["stats"][k], s)
    print({k: f"{v:.2e}" for k, v in errs.items()})
    bad = {k: v for k, v in errs.items() if v > tol}
    assert not bad, bad


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
@pytest.mark.parametrize("training", [True, False], ids=["training_stats", "moving_stats"])
def test_layer_against_fp64(cuda, training, fused, monkeypatch, reference):
    """fp32 bound 3e-4: test_nasfpn's bound for a head of this depth (parameter gradients in its measure: max-norm, floored at 1e-3 of the largest)"""
    from iseg_amd import functional as F

    jpu = _layer()
    stats0 = {b.iseg_name: b.clone() for b in jpu.buffers()}
    ref = reference(jpu, training)
    if fused:      # the route under test is the fused one: the predicate accepts the merged map
        calls = []
        real = F._JpuTailFn.apply
        monkeypatch.setattr(F._JpuTailFn, "apply", lambda *a: (calls.append(1), real(*a))[1])
    got = _run(jpu, ref["xs"], ref["dy"], training, fused, monkeypatch, stats0)
    if fused:
        assert calls == [1]
    _check(got, ref, 3e-4, training)


@pytest.mark.parametrize("training", [True, False], ids=["training_stats", "moving_stats"])
def test_fused_against_composed(cuda, training, monkeypatch):
    jpu = _layer()
    stats0 = {b.iseg_name: b.clone() for b in jpu.buffers()}
    xs = _inputs()
    dy = torch.randn((2, 16, 20, 64), generator=torch.Generator().manual_seed(41))
    a = _run(jpu, xs, dy, training, True, monkeypatch, stats0)
    b = _run(jpu, xs, dy, training, False, monkeypatch, stats0)
    errs = {"y": _rel(a["y"], b["y"].cpu().double())}
    for i in (1, 2, 3):
        errs[f"dx{i}"] = _rel(a["dx"][i], b["dx"][i].cpu().double())
    # a training-mode BN removes the per-channel mean of its input gradient, so the gradients in front of it (depthwise bias, the BN's own
    # beta) are zero up to rounding: errors are measured against the larger of the tensor's own scale and a small fraction of the largest gradient
    gmax = max(g.abs().max().item() for g in b["grads"].values())
    for k in a["grads"]:
        errs[k] = (a["grads"][k] - b["grads"][k]).abs().max().item() / max(b["grads"][k].abs().max().item(), 1e-2 * gmax)
    for k in a["stats"]:
        errs[k] = _rel(a["stats"][k], b["stats"][k].cpu().double())
    print({k: f"{v:.2e}" for k, v in errs.items()})
    bad = {k: v for k, v in errs.items() if v > 1e-4}
    assert not bad, bad


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
def test_not_trainable(cuda, fused, monkeypatch):
    """trainable=False: no parameter receives a gradient, the moving statistics do not move, the inputs still get theirs"""
    jpu = _layer(trainable=False)
    monkeypatch.setenv("ISEG_JPU_FUSED", "1" if fused else "0")
    stats0 = {b.iseg_name: b.clone() for b in jpu.buffers()}
    jpu._iseg_store.zero_grad()
    xg = [x.cuda().requires_grad_(True) for x in _inputs()]
    y = jpu(xg, training=True)
    y.backward(torch.randn(y.shape, generator=torch.Generator().manual_seed(1)).cuda())
    torch.cuda.synchronize()
    assert not any(p.requires_grad for p in jpu.parameters())
    assert float(jpu._iseg_store.flat_g.abs().max()) == 0.0
    for b in jpu.buffers():
        assert torch.equal(b, stats0[b.iseg_name]), b.iseg_name
    assert xg[0].grad is None and all(x.grad is not None and torch.isfinite(x.grad).all() and float(x.grad.abs().max()) > 0 for x in xg[1:])
    w = OM.export_weights(jpu)
    ref = R.jpu_forward(w, [x.detach().cpu().double() for x in xg], "jpu", training=False)      # frozen layers run on their moving statistics
    assert _rel(y, ref) < 3e-4


def test_resnet18_jpu_aspp_bf16_training_step(cuda, monkeypatch):
    """64 x 64, N = 2, bf16 storage: logits of both routes against fp64 (fused error <= 2 x composed error + 1e-3), finite gradients, and one
    step of the project's SGD"""
    from iseg_amd import functional as F
    from iseg_amd import nn
    from iseg_amd.core_optimizer import get_optimizer
    from iseg_amd.data import synthetic_batch
    from iseg_amd.distribution.distribution_utils import Strategy
    from iseg_amd.heads import resnet18_jpu_aspp
    from iseg_amd.trainer import TrainableModel

    nn.set_compute_dtype(torch.bfloat16)
    nn.set_device("cuda:0")
    model = resnet18_jpu_aspp(num_class=21, build_input_size=(64, 64), jpu_width=64, dropout_rate=0.0)
    opt = get_optimizer(Strategy(one_device=True), initial_lr=1e-3, epoch_steps=10, train_epoch=1, optimizer="sgd", sgd_momentum_rate=0.9)
    tm = TrainableModel(model, optimizer=opt, loss=model.custom_losses(21, 255, 2), loss_weights=model.custom_losses_weights(),
                        metrics=model.custom_metrics(21, 255))
    randomize_parameters(model, 3)      # after the ParamStore took over the storage
    tm.store.sync_shadow()
    x, y = synthetic_batch(2, 64, 64, seed=5)
    xc, yc = x.cuda(), y.cuda()
    w = OM.export_weights(model)
    ref = R.resnet18_jpu_aspp_forward(w, x.double(), training=True)["logits"]
    logits = {}
    for fused in (True, False):
        monkeypatch.setenv("ISEG_JPU_FUSED", "1" if fused else "0")
        with torch.no_grad():
            logits[fused] = model(xc, training=True)[0]
        assert tuple(logits[fused].shape) == (2, 64, 64, 21) and logits[fused].dtype == torch.float32
    ef, ec = _rel(logits[True], ref), _rel(logits[False], ref)
    print(f"logits against fp64: fused {ef:.3e} composed {ec:.3e}")
    assert ef <= 2 * ec + 1e-3, (ef, ec)
    # gradients of one forward / backward on the fused route
    monkeypatch.setenv("ISEG_JPU_FUSED", "1")
    tm.store.zero_grad()
    loss = F.softmax_ce_mean(model(xc, training=True)[0], yc, 21, 255)
    loss.backward()
    assert torch.isfinite(loss).item()
    assert torch.isfinite(tm.store.flat_g).all().item()
    for name in ("jpu_aspp_head/jpu/end_depthwise_conv_8/depthwise_kernel", "jpu_aspp_head/jpu/end_pointwise_convs_1/conv/kernel",
                 "jpu_aspp_head/jpu/endpoint_conv_2/conv/kernel", "conv1_1_conv/kernel"):
        g = next(p.grad for p in model.parameters() if p.iseg_name == name)
        assert float(g.abs().max()) > 0, name
    tm.store.zero_grad()
    w0 = tm.store.flat_w.clone()
    out = tm.train_step(xc, yc)
    torch.cuda.synchronize()
    assert torch.isfinite(torch.as_tensor(float(out[0]))).item()
    assert torch.isfinite(tm.store.flat_w).all().item() and not torch.equal(tm.store.flat_w, w0)
