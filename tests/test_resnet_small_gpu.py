"""ResNet-9 / 10 / 18 (reference backbones/resnet_blocks_small.py, resnet_common.py:348-418) on the GPU, through the fused block tail
(ISEG_RESBLOCK_FUSED=1) and the composed operators: the fused block against the composed one for every block kind; ResNet-18 endpoints and
every parameter gradient against the fp64 restatement of tests/resnet_small_ref.py at output strides 32 / 16 / 8; one forward each of
ResNet-9 and ResNet-10; one ResNet-18 + ASPP training step against the restatement plus the oracle's ASPP; and the HIP-graph replay of the
training step against the eager step, bit for bit."""
import pytest
import torch

from oracle import models as OM
from tests import resnet_small_ref as R
from tests.util_models import randomize_parameters

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _restore_policy():
    from iseg_amd import nn

    yield
    nn.set_compute_dtype(torch.float32)


@pytest.fixture(params=["fused", "composed"])
def route(request, monkeypatch):
    """the block tails through csrc/resblock.hip (ISEG_RESBLOCK_FUSED=1) or the composed operators"""
    monkeypatch.setenv("ISEG_RESBLOCK_FUSED", "1" if request.param == "fused" else "0")
    return request.param


def _rel(a, b):
    return (a.detach().cpu().double() - b).abs().max().item() / max(b.abs().max().item(), 1e-8)


def _net(name, output_stride, slim=True, seed=3, return_endpoints=True):
    from iseg_amd import nn
    from iseg_amd.backbones.feature_extractor import get_backbone
    from iseg_amd.param_store import ParamStore

    nn.set_compute_dtype(torch.float32)
    nn.set_device("cuda:0")
    m = get_backbone(name, output_stride=output_stride, resnet_slim=slim, return_endpoints=return_endpoints, image_shape=(1, 64, 64, 3))
    m._iseg_store = ParamStore(list(m.parameters()))
    randomize_parameters(m, seed)
    return m


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("cin,filters,stride", [(64, 64, 1), (64, 64, 2), (64, 128, 1), (64, 128, 2)])
def test_fused_block_matches_composed(cuda, monkeypatch, cin, filters, stride, training):
    from iseg_amd import nn
    from iseg_amd.backbones.resnet_blocks_small import BlockType2Small
    from iseg_amd.param_store import ParamStore

    nn.set_compute_dtype(torch.float32)
    nn.set_device("cuda:0")
    blk = BlockType2Small(filters, stride=stride, name="b")
    with nn.dry_run_scope():
        blk(torch.empty(2, 17, 15, cin), training=training)
    store = ParamStore(list(blk.parameters()))
    randomize_parameters(blk, 4)
    assert blk.conv_shortcut == (cin != filters)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 17, 15, cin, generator=g).cuda()
    dy = torch.randn(2, -(-17 // stride), -(-15 // stride), filters, generator=g).cuda()
    moving0 = [b.clone() for b in blk.buffers()]
    res = {}
    for r in ("fused", "composed"):
        monkeypatch.setenv("ISEG_RESBLOCK_FUSED", "1" if r == "fused" else "0")
        with torch.no_grad():
            for b, v in zip(blk.buffers(), moving0):
                b.copy_(v)
        store.zero_grad()
        xi = x.clone().requires_grad_(True)
        y = blk(xi, training=training)
        y.backward(dy)
        res[r] = (y.detach().double().cpu(), xi.grad.double().cpu(), {p.iseg_name: p.grad.double().cpu().clone() for p in blk.parameters()},
                  [b.double().cpu().clone() for b in blk.buffers()])
    f, c = res["fused"], res["composed"]
    assert _rel(f[0], c[0]) < 1e-4
    assert _rel(f[1], c[1]) < 1e-4
    for k in c[2]:
        assert _rel(f[2][k], c[2][k]) < 1e-4, k
    for a, b in zip(f[3], c[3]):
        assert _rel(a, b) < 1e-5


@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("output_stride,size", [(32, (64, 96)), (16, (65, 47)), (8, (64, 64))])
def test_resnet18_endpoints_match_restatement(cuda, output_stride, size, training, route):
    m = _net("resnet18", output_stride)
    x = torch.randn(2, size[0], size[1], 3, generator=torch.Generator().manual_seed(1))
    w = OM.export_weights(m)
    with torch.no_grad():
        ends = m(x.cuda(), training=training)
    ref = R.resnet_forward(w, x.double(), "resnet18", output_stride=output_stride, training=training)
    assert len(ends) == len(ref) == 5
    for got, want in zip(ends, ref):
        assert tuple(got.shape) == tuple(want.shape)
        assert _rel(got, want) < 2e-4


@pytest.mark.parametrize("slim", [True, False])
@pytest.mark.parametrize("output_stride", [32, 16, 8])
def test_resnet18_training_gradients(cuda, output_stride, slim, route):
    m = _net("resnet18", output_stride, slim=slim, return_endpoints=False, seed=8)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, 64, 64, 3, generator=g)
    w = {k: v.requires_grad_(True) if v.is_floating_point() and not k.endswith(("moving_mean", "moving_variance")) else v
         for k, v in OM.export_weights(m).items()}
    new_stats = {}
    y = m(x.cuda(), training=True)
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy.cuda())
    ref = R.resnet_forward(w, x.double(), "resnet18", output_stride=output_stride, slim=slim, training=True, new_stats=new_stats)[-1]
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


@pytest.mark.parametrize("name", ["resnet9", "resnet10"])
def test_resnet9_10_forward(cuda, name, route):
    m = _net(name, 16)
    x = torch.randn(2, 63, 64, 3, generator=torch.Generator().manual_seed(2))
    w = OM.export_weights(m)
    with torch.no_grad():
        ends = m(x.cuda(), training=True)
    ref = R.resnet_forward(w, x.double(), name, output_stride=16, training=True)
    for got, want in zip(ends, ref):
        assert tuple(got.shape) == tuple(want.shape)
        assert _rel(got, want) < 2e-4


def test_aspp_one_training_step_matches_oracle(cuda, route):
    from iseg_amd import functional as F
    from iseg_amd import nn
    from iseg_amd.data import synthetic_batch
    from iseg_amd.heads import resnet18_aspp
    from iseg_amd.param_store import ParamStore

    nn.set_compute_dtype(torch.float32)
    nn.set_device("cuda:0")
    model = resnet18_aspp(num_class=21, output_stride=16, build_input_size=(96, 96), dropout_rate=0.0)
    model._iseg_store = ParamStore(list(model.parameters()))
    randomize_parameters(model, 6)
    x, y = synthetic_batch(2, 96, 96, seed=7)
    w = OM.export_weights(model)
    model._iseg_store.zero_grad()
    logits = model(x.cuda(), training=True)[0]
    loss = F.softmax_ce_mean(logits, y.cuda(), 21, 255)
    loss.backward()
    wr = {k: v.clone().requires_grad_(not k.endswith(("moving_mean", "moving_variance"))) for k, v in w.items()}
    ref = R.resnet_aspp_forward(wr, x.double(), "resnet18", training=True, output_stride=16)
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
    model = heads.resnet18_aspp(build_input_size=(128, 128), dropout_rate=0.1)
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
    """three steps of ResNet-18 + ASPP (dropout, bf16 storage): the HIP-graph replay gives the eager step's bits"""
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
