"""MaskLoss through the HIP kernels (csrc/mask_loss.hip) against the fp64 restatement tests/mask_loss_ref.py: the scalar, the per-pixel tensor
and the gradients of both routes, every element compared; the fused route against the composed one; run-to-run identity, graph replay and a
training step through CoreTrain.

Tolerance (fixed before the kernels ran): the project's loss bound, 2e-5 on O(1) values (tests/test_focal_gpu.py), scaled by the largest
expected magnitude: 2e-5 * max(1, max|want|) for values, 2e-5 * max|want_grad| for gradients.  The restatement evaluated in fp32 on the host
is itself off by 1.3e-7 of the maximum on values and 7e-7 of the maximum on gradients; the kernels use the hardware exp / log (~1e-6)."""
import pytest
import torch

from tests import mask_loss_ref as R

pytestmark = pytest.mark.gpu

REL = 2e-5


def _case(B, H, W, C, ignore=255, seed=0, label_hw=None, ignored_image=None):
    g = torch.Generator().manual_seed(seed)
    z = (torch.randn(B, H, W, C, generator=g) * 4).clamp(-12, 12).float()
    h, w = label_hw or (H, W)
    if ignore == 0:
        y = torch.randint(0, C + 1, (B, h, w), generator=g, dtype=torch.int32)      # 0 = ignore, 1..C = classes
    else:
        y = torch.randint(0, C, (B, h, w), generator=g, dtype=torch.int32)
        r = torch.rand(B, h, w, generator=g)
        y[r < 0.15] = ignore
        y[(r > 0.15) & (r < 0.18)] = 254 if C < 254 else ignore      # out of range, not the ignore label: valid, all-negative row
    if ignored_image is not None:
        y[ignored_image] = ignore
    return y, z


def _check(name, got, want, grad=False):
    got, want = got.detach().double().cpu().reshape(-1), want.detach().double().reshape(-1)
    scale = float(want.abs().max())
    bound = REL * (scale if grad else max(1.0, scale))
    err = float((got - want).abs().max())
    print(f"{name}: max|want| {scale:.6g}  max error {err:.3e}  bound {bound:.3e}")
    assert bool(torch.isfinite(got).all()) and err <= bound, (name, err, bound)


def _parity(y, z, tag, **kw):
    from iseg_amd.losses.mask_loss import MaskLoss

    ref_kw = {k: v for k, v in kw.items()}
    C = z.shape[-1]
    ignore = kw.pop("ignore_label", 255)
    ref_kw["ignore_label"] = ignore
    # the restatement: scalar and its gradient, per-pixel tensor and the gradient of a weighted sum of it
    zr = z.double().requires_grad_(True)
    want_s = R.mask_loss(y, zr, num_class=C, **ref_kw)
    (want_ds,) = torch.autograd.grad(want_s, zr)
    want_px = R.mask_loss(y, zr, reduction=True, num_class=C, **ref_kw)
    up = torch.rand(want_px.shape, generator=torch.Generator().manual_seed(11), dtype=torch.float64) + 0.5
    (want_dpx,) = torch.autograd.grad((want_px * up).sum(), zr)

    zc = z.cuda().requires_grad_(True)
    got_s = MaskLoss(num_class=C, ignore_label=ignore, **kw)(y.cuda(), zc)
    (got_ds,) = torch.autograd.grad(got_s, zc)
    got_px = MaskLoss(num_class=C, ignore_label=ignore, reduction=True, **kw)(y.cuda(), zc)
    (got_dpx,) = torch.autograd.grad((got_px * up.float().cuda()).sum(), zc)
    assert got_s.shape == () and tuple(got_px.shape) == tuple(want_px.shape)
    _check(f"{tag} scalar", got_s, want_s)
    _check(f"{tag} per-pixel", got_px, want_px)
    _check(f"{tag} dlogits(scalar)", got_ds, want_ds, grad=True)
    _check(f"{tag} dlogits(per-pixel)", got_dpx, want_dpx, grad=True)
    return got_s, got_px, got_ds, got_dpx


FLAG_CASES = {
    "defaults": {},
    "sigmoid_only": dict(use_dice_loss=False, use_ce_loss=False),
    "dice_only": dict(use_sigmoid_loss=False, use_ce_loss=False),
    "ce_only": dict(use_sigmoid_loss=False, use_dice_loss=False),
    "plain_sigmoid": dict(apply_focal_sigmoid_loss=False),
    "class_balancing": dict(apply_class_balancing=True),
    "focal_ce": dict(apply_focal_ce_loss=True),
    "coefficients": dict(ce_loss_coefficient=0.5, sigmoid_loss_coefficient=5.0, dice_loss_coefficient=2.0, apply_focal_sigmoid_loss=False,
                         apply_focal_ce_loss=True),
}


@pytest.mark.parametrize("flags", list(FLAG_CASES))
def test_parity_flag_combinations(cuda, flags):
    y, z = _case(2, 33, 29, 21, seed=1)
    _parity(y, z, flags, **FLAG_CASES[flags])


@pytest.mark.parametrize("C", [2, 5, 21, 150])
@pytest.mark.parametrize("B", [1, 3])
def test_parity_classes_and_image_boundaries(cuda, C, B):
    """33 x 29 = 957 pixels per image: not a multiple of any tile (256 / 64 pixels), so the last tile of every image is partial"""
    y, z = _case(B, 33, 29, C, seed=2 + C)
    _parity(y, z, f"C={C} B={B}")


def test_parity_ignore_label_zero(cuda):
    y, z = _case(2, 33, 29, 5, ignore=0, seed=3)
    _parity(y, z, "ignore_label=0", ignore_label=0)
    _parity(y, z, "ignore_label=0 focal_ce", ignore_label=0, apply_focal_ce_loss=True)


def test_parity_labels_at_half_resolution(cuda):
    y, z = _case(2, 32, 28, 21, seed=4, label_hw=(16, 14))
    _parity(y, z, "half-resolution labels")
    y, z = _case(2, 33, 29, 5, seed=4, label_hw=(17, 15))
    _parity(y, z, "odd-size labels")


def test_parity_fully_ignored_image_and_batch(cuda):
    from iseg_amd.losses.mask_loss import MaskLoss

    y, z = _case(3, 33, 29, 21, seed=5, ignored_image=1)
    _, px, ds, _ = _parity(y, z, "one ignored image")
    assert float(px[1].abs().max()) == 0.0 and float(ds[1].abs().max()) == 0.0
    y[:] = 255
    zc = z.cuda().requires_grad_(True)
    L = MaskLoss()(y.cuda(), zc)
    L.backward()
    assert float(L) == 0.0 and float(zc.grad.abs().max()) == 0.0


def test_known_answers_through_the_kernels(cuda):
    """the host file's known answers: zero logits, C = 4, defaults -> 20 * 0.25 ln 2 + 2/3 + ln 4; an out-of-range label is a valid all-negative row"""
    import math

    from iseg_amd.losses.mask_loss import MaskLoss

    y = torch.randint(0, 4, (2, 5, 6), generator=torch.Generator().manual_seed(0), dtype=torch.int32)
    z = torch.zeros(2, 5, 6, 4)
    want = 20 * 0.25 * math.log(2.0) + (1 - 1 / 3) + math.log(4.0)
    got = float(MaskLoss(num_class=4)(y.cuda(), z.cuda()))
    px = MaskLoss(num_class=4, reduction=True)(y.cuda(), z.cuda())
    print("zero logits:", got, want)
    assert abs(got - want) < REL * want and float((px - want).abs().max()) < REL * want
    z1 = torch.tensor([[[[0.3, -1.2, 2.0]]]])
    s = [1 / (1 + math.exp(-v)) for v in (0.3, -1.2, 2.0)]
    want1 = 20 * sum(si ** 2 * (-math.log(1 - si)) for si in s) / 3 + 1 - 1e-7 / (sum(s) + 1e-7)
    got1 = float(MaskLoss(num_class=3)(torch.tensor([[[254]]], dtype=torch.int32).cuda(), z1.cuda()))
    print("out-of-range label:", got1, want1)
    assert abs(got1 - want1) < REL * max(1.0, want1)


def test_num_class_beyond_one_lds_tile_is_refused(cuda):
    from iseg_amd import _hip
    from iseg_amd.losses.mask_loss import MaskLoss

    with pytest.raises(_hip.HipCallError):
        MaskLoss(num_class=257)(torch.zeros(1, 4, 4, dtype=torch.int32).cuda(), torch.zeros(1, 4, 4, 257).cuda())


@pytest.mark.parametrize("flags", ["defaults", "plain_sigmoid", "focal_ce", "dice_only"])
def test_fused_route_equals_composed_route(cuda, monkeypatch, flags):
    from iseg_amd.losses.mask_loss import MaskLoss

    kw = FLAG_CASES[flags]
    y, z = _case(2, 33, 29, 21, seed=6)
    up = (torch.rand(2, 33 * 29, generator=torch.Generator().manual_seed(11)) + 0.5).cuda()
    out = {}
    for route in ("1", "0"):
        monkeypatch.setenv("ISEG_MASKLOSS_FUSED", route)
        zc = z.cuda().requires_grad_(True)
        s = MaskLoss(**kw)(y.cuda(), zc)
        (ds,) = torch.autograd.grad(s, zc)
        px = MaskLoss(reduction=True, **kw)(y.cuda(), zc)
        (dpx,) = torch.autograd.grad((px * up).sum(), zc)
        fm = MaskLoss(**kw).fused_mean(y.cuda(), zc, 0.4)
        out[route] = (s, px, ds, dpx, fm)
    zr = z.double().requires_grad_(True)
    want = R.mask_loss(y, zr, num_class=21, **kw)
    for route in ("1", "0"):
        _check(f"{flags} route {route} scalar vs restatement", out[route][0], want)
        _check(f"{flags} route {route} fused_mean(weight 0.4)", out[route][4], 0.4 * want)
    for k, name in enumerate(("scalar", "per-pixel", "dlogits(scalar)", "dlogits(per-pixel)")):
        _check(f"{flags} fused vs composed {name}", out["1"][k], out["0"][k].double().cpu(), grad=k >= 2)


def test_loss_and_gradient_are_bit_identical_run_to_run(cuda):
    from iseg_amd.losses.mask_loss import MaskLoss

    y, z = _case(3, 65, 61, 21, seed=7)
    runs = []
    for _ in range(3):
        zc = z.cuda().requires_grad_(True)
        s = MaskLoss()(y.cuda(), zc)
        s.backward()
        px = MaskLoss(reduction=True)(y.cuda(), zc.detach())
        runs.append((s.detach().clone(), zc.grad.clone(), px.clone()))
    for r in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(runs[0], r))


def _trainer(calls=None):
    from iseg_amd import heads
    from iseg_amd.core_env import common_env_setup
    from iseg_amd.core_optimizer import get_optimizer
    from iseg_amd.core_train import CoreTrain
    from iseg_amd.losses.mask_loss import MaskLoss
    from iseg_amd.modelhelper import model_common_setup

    class Counted(MaskLoss):
        def fused_mean(self, *a, **k):
            if calls is not None:
                calls.append(1)
            return MaskLoss.fused_mean(self, *a, **k)

    strategy = common_env_setup(use_one_device_strategy=True, mixed_precision=True, random_seed=3)
    model = heads.resnet18_aspp(build_input_size=(64, 64), dropout_rate=0.1)
    model.custom_main_loss_fn = lambda **kw: Counted(**kw)      # the binding a reference script uses
    helper = model_common_setup(model, restore_checkpoint=False)
    helper.set_optimizer(get_optimizer(strategy, initial_lr=1e-3, end_lr=0.0, epoch_steps=20, train_epoch=1, warmup_steps=3, warmup_lr=1e-5,
                                       optimizer="adamw", adamw_weight_decay=0.05, clipnorm=None))
    return CoreTrain(helper, None).create_trainable_model(21, ignore_label=255, batch_size=4)


def _batches():
    from iseg_amd.data import synthetic_batch

    out = []
    for s in (5, 6, 7):
        x, y = synthetic_batch(4, 64, 64, seed=s)
        out.append((x.cuda(), y.cuda()))
    return out


def test_training_step_through_core_train_takes_fused_mean(cuda):
    from iseg_amd import functional as F
    from iseg_amd.losses.mask_loss import MaskLoss

    F._RNG_COUNTER[0] = 0
    F._DROP_PATH_POOL.__init__()
    calls = []
    tm = _trainer(calls)
    assert isinstance(tm._loss_fn(0), MaskLoss)
    w0 = tm.store.flat_w.clone()
    x, y = _batches()[0]
    losses = tm.train_step(x, y)
    torch.cuda.synchronize()
    assert len(calls) == 1, "the trainer did not take MaskLoss.fused_mean"
    assert bool(torch.isfinite(losses[0])) and float(losses[0]) > 0
    assert bool(torch.isfinite(tm.store.flat_w).all()) and not torch.equal(w0, tm.store.flat_w)


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
        losses.append(float(step(x, y)[0]))
    torch.cuda.synchronize()
    return losses, tm.store.flat_w.clone(), w0, step


def test_mask_loss_train_step_graph_replay_follows_eager(cuda):
    """three steps of ResNet-18 + ASPP with MaskLoss as the main loss: the HIP-graph replay gives the eager step's losses and weights, bit for bit
    (nothing of the loss reads the host: V, the dice values and the scalar stay on the device)"""
    batches = _batches()
    le, we, w0e, _ = _run(False, batches)
    lg, wg, w0g, step = _run(True, batches)
    assert torch.equal(w0e, w0g)
    assert any(e.get("graph") is not None for e in step.entries.values()), "the step was never captured"
    assert le == lg, (le, lg)
    assert torch.equal(we, wg), float((we - wg).abs().max())
