"""Xception-65 (reference backbones/xception_common.py) through get_backbone against the fp64 restatement of tests/xception_ref.py: endpoints at
output strides 8 / 16 / 32 and an odd size (moving and batch statistics), a training-mode gradient check of the whole backbone at fp32, one
bf16 run; Xception-65 + ASPP forward / loss / gradients against the oracle; and the HIP-graph replay of its training step against the eager
step, bit for bit."""
import pytest
import torch

from oracle import models as OM
from tests import xception_ref as R
from tests.util_models import randomize_parameters

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _restore_policy():
    from iseg_amd import nn

    yield
    nn.set_compute_dtype(torch.float32)


def _rel(a, b):
    return (a.detach().cpu().double() - b).abs().max().item() / max(b.abs().max().item(), 1e-8)


def _x65(output_stride, dtype=torch.float32, seed=3, return_endpoints=True):
    from iseg_amd import nn
    from iseg_amd.backbones.feature_extractor import get_backbone
    from iseg_amd.param_store import ParamStore

    nn.set_compute_dtype(dtype)
    nn.set_device("cuda:0")
    m = get_backbone("xception65", output_stride=output_stride, return_endpoints=return_endpoints, image_shape=(1, 64, 64, 3))
    m._iseg_store = ParamStore(list(m.parameters()))
    randomize_parameters(m, seed)
    return m


@pytest.fixture(params=["fused", "composed"])
def route(request, monkeypatch):
    """the separable units through csrc/sepconv.hip (ISEG_SEPCONV_FUSED=1) or the composed operators"""
    monkeypatch.setenv("ISEG_SEPCONV_FUSED", "1" if request.param == "fused" else "0")
    return request.param


@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("output_stride,size", [(32, (64, 96)), (16, (65, 47)), (8, (64, 64))])
def test_endpoints_match_restatement(cuda, output_stride, size, training, route):
    m = _x65(output_stride)
    x = torch.randn(2, size[0], size[1], 3, generator=torch.Generator().manual_seed(1))
    w = OM.export_weights(m)
    with torch.no_grad():
        ends = m(x.cuda(), training=training)
    ref = R.xception_forward(w, x.double(), output_stride=output_stride, training=training)
    assert len(ends) == len(ref) == {32: 6, 16: 5, 8: 4}[output_stride]
    for got, want in zip(ends, ref):
        assert tuple(got.shape) == tuple(want.shape)
        assert _rel(got, want) < 2e-4


def test_training_gradients_fp32(cuda, route):
    m = _x65(16, return_endpoints=False, seed=8)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, 64, 64, 3, generator=g)
    w = {k: v.requires_grad_(True) if v.is_floating_point() and not k.endswith(("moving_mean", "moving_variance")) else v
         for k, v in OM.export_weights(m).items()}
    new_stats = {}
    y = m(x.cuda(), training=True)
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy.cuda())
    ref = R.xception_forward(w, x.double(), output_stride=16, training=True, new_stats=new_stats)[-1]
    ref.backward(dy.double())
    assert _rel(y, ref.detach()) < 5e-4
    gmax = max(w[p.iseg_name].grad.norm().item() for p in m.parameters())
    errs = {}
    for p in m.parameters():
        ref_g = w[p.iseg_name].grad
        errs[p.iseg_name] = (p.grad.cpu().double() - ref_g).norm().item() / max(ref_g.norm().item(), 1e-3 * gmax)
    bad = {k: round(v, 5) for k, v in errs.items() if v > 5e-2}
    assert not bad, bad
    for b in m.buffers():      # the moving statistics the training-mode call left behind
        if b.iseg_name in new_stats:
            assert _rel(b, new_stats[b.iseg_name]) < 1e-3, b.iseg_name


def test_bf16_against_fp64(cuda, route):
    """bf16 storage through all 21 blocks: the last endpoint within 5 % of the largest fp64 value, the others within 3 %"""
    m = _x65(16, dtype=torch.bfloat16, seed=2)
    x = torch.randn(2, 64, 64, 3, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        ends = m(x.cuda(), training=False)
    ref = R.xception_forward(OM.export_weights(m), x.double(), output_stride=16, training=False)
    for i, (got, want) in enumerate(zip(ends, ref)):
        assert got.dtype == torch.bfloat16
        assert _rel(got.float(), want) < (5e-2 if i == len(ref) - 1 else 3e-2), i


def test_aspp_one_training_step_matches_oracle(cuda, route):
    from iseg_amd import functional as F
    from iseg_amd import nn
    from iseg_amd.data import synthetic_batch
    from iseg_amd.heads import xception65_aspp
    from iseg_amd.param_store import ParamStore

    nn.set_compute_dtype(torch.float32)
    nn.set_device("cuda:0")
    model = xception65_aspp(num_class=21, output_stride=16, build_input_size=(96, 96), dropout_rate=0.0)
    model._iseg_store = ParamStore(list(model.parameters()))
    randomize_parameters(model, 6)
    x, y = synthetic_batch(2, 96, 96, seed=7)
    w = OM.export_weights(model)
    model._iseg_store.zero_grad()
    logits = model(x.cuda(), training=True)[0]
    loss = F.softmax_ce_mean(logits, y.cuda(), 21, 255)
    loss.backward()
    wr = {k: v.clone().requires_grad_(not k.endswith(("moving_mean", "moving_variance"))) for k, v in w.items()}
    ref = R.xception_aspp_forward(wr, x.double(), training=True, output_stride=16)
    ref_loss = OM.mean_ce_loss(ref["logits"], y)
    ref_loss.backward()
    assert (logits.detach().cpu().double() - ref["logits"]).abs().max().item() < 1e-3
    assert abs(loss.item() - ref_loss.item()) < 1e-4 * max(1.0, abs(ref_loss.item()))
    gmax = max(wr[p.iseg_name].grad.norm().item() for p in model.parameters())
    errs = {}
    for p in model.parameters():
        gr = wr[p.iseg_name].grad
        errs[p.iseg_name] = (p.grad.detach().cpu().double() - gr).norm().item() / max(gr.norm().item(), 1e-3 * gmax)
    bad = {k: round(v, 5) for k, v in errs.items() if v > 5e-2}
    assert not bad, bad


def _trainer():
    from iseg_amd import heads
    from iseg_amd.core_env import common_env_setup
    from iseg_amd.core_optimizer import get_optimizer
    from iseg_amd.core_train import CoreTrain
    from iseg_amd.modelhelper import model_common_setup

    strategy = common_env_setup(use_one_device_strategy=True, mixed_precision=True, random_seed=3)
    model = heads.xception65_aspp(build_input_size=(128, 128), dropout_rate=0.1)
    helper = model_common_setup(model, restore_checkpoint=False)
    helper.set_optimizer(get_optimizer(strategy, initial_lr=1e-3, end_lr=0.0, epoch_steps=20, train_epoch=1, warmup_steps=3, warmup_lr=1e-5,
                                       optimizer="adamw", adamw_weight_decay=0.05, clipnorm=None))
    return CoreTrain(helper, None).create_trainable_model(21, ignore_label=255, batch_size=4)


def _run(graphed, batches, steps=3):
    from iseg_amd import functional as F
    from iseg_amd.graphs import GraphedTrainStep

    F._RNG_COUNTER[0] = 0
    F._DROP_PATH_POOL.__init__()
    tm = _trainer()
    w0 = tm.store.flat_w.clone()
    step = GraphedTrainStep(tm, warmup=1) if graphed else tm.train_step
    losses = []
    for i in range(steps):
        x, y = batches[i % len(batches)]
        out = step(x, y)
        losses.append(float(out[0]))
    torch.cuda.synchronize()
    return losses, tm.store.flat_w.clone(), w0, step


def test_aspp_graphed_train_steps_follow_eager(cuda, route):
    """three steps of Xception-65 + ASPP (dropout, bf16 storage): the HIP-graph replay gives the eager step's bits"""
    from iseg_amd.data import synthetic_batch

    batches = []
    for s in (5, 6, 7):
        x, y = synthetic_batch(4, 128, 128, seed=s)
        batches.append((x.cuda(), y.cuda()))
    le, we, w0e, _ = _run(False, batches)
    lg, wg, w0g, step = _run(True, batches)
    assert torch.equal(w0e, w0g), "the two trainers did not start from the same weights"
    assert any(e.get("graph") is not None for e in step.entries.values()), "the step was never captured"
    assert le == lg, (le, lg)
    assert torch.equal(we, wg), float((we - wg).abs().max())
