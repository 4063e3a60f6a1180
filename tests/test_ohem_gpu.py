"""Online hard example mining on the GPU (csrc/ohem.hip) against the restatement tests/ohem_ref.py: the radix select alone, bit for bit; the
labelled-class probabilities; the selected loss and its gradient through catecrossentropy_ignore_label_loss and SegFoundation.custom_losses;
guard bands around every buffer; the launchers' refusals; one training step with use_ohem=True, eager twice and replayed from a HIP graph."""
import os

import numpy as np
import pytest
import torch

from tests import guarded_memory as GM
from tests import ohem_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(2, 5, 7, 5), (3, 37, 53, 21)]
IGNORE = 255


def case(N, H, W, C, seed=11):
    """(labels [N,H,W] int64 with about one ignored pixel in eight, logits [N,H,W,C] fp32 ~ 4 N(0, 1)) as NumPy arrays"""
    rng = np.random.default_rng(seed + C)
    y = rng.integers(0, C, size=(N, H, W))
    y[rng.random((N, H, W)) < 0.125] = IGNORE
    return y, (4.0 * rng.standard_normal((N, H, W, C))).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the selection alone
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _values(content, P, rng):
    if content == "all_equal":
        return np.full(P, 0.375, np.float32)
    if content == "all_zero":
        return np.zeros(P, np.float32)
    if content == "five_levels":
        return rng.choice(np.array([0.0, 0.125, 0.5, 0.7, 1.0], np.float32), size=P)
    if content == "denormals_and_zeros":
        v = (rng.integers(0, 4000, size=P).astype(np.uint32)).view(np.float32)      # bit patterns 0 .. 3999: +0 and the smallest denormals
        v[rng.random(P) < 0.3] = 0.0
        return v
    if content == "lowest_mantissa_byte":
        return (np.uint32(0x3F000000) + rng.integers(0, 256, size=P).astype(np.uint32)).view(np.float32)      # 0.5 + j * 2^-24, j < 256
    if content == "signed":
        return (rng.standard_normal(P) * np.exp(6 * rng.standard_normal(P))).astype(np.float32)
    raise KeyError(content)


def _cap_trip():
    """the smallest P at which the capped grid of the streaming passes takes a second trip, plus a ragged tail"""
    from iseg_amd import kernels as K

    return K.OHEM_PARTIAL_FLOATS * 1024 + 1029


SELECT_P = [1, 70, 4133, "cap"]
CONTENTS = ["all_equal", "all_zero", "five_levels", "denormals_and_zeros", "lowest_mantissa_byte", "signed"]


def _check_select(values, loss, mkt, thresh):
    from iseg_amd import kernels as K

    want = R.select_values(values, loss, mkt, thresh)
    v, l = torch.from_numpy(values).cuda(), torch.from_numpy(loss).cuda()
    runs = [K.ohem_select(v, l, mkt, thresh, want_loss=True, want_sum=True, sum_scale=0.25) for _ in range(2)]
    keep, out, s, thr, nnz = runs[0]
    tag = f"P={values.size} mkt={mkt} thresh={thresh}"
    assert torch.equal(thr.cpu(), torch.tensor([want["threshold"]], dtype=torch.float32)), (tag, float(thr), want["threshold"])
    assert torch.equal(nnz.cpu(), torch.tensor([want["nnz"]], dtype=torch.int32)), (tag, int(nnz), want["nnz"])
    assert torch.equal(keep.cpu(), torch.from_numpy(want["keep"].astype(np.float32))), tag
    assert torch.equal(out.cpu(), torch.from_numpy(want["out"])), tag
    exact = 0.25 * want["out"].astype(np.float64).sum()
    scale = 0.25 * np.abs(want["out"].astype(np.float64)).sum()      # = |exact| unless the kept losses have both signs
    # (2^-149: the spacing of fp32 below 2^-126 -- a sum of denormals times the scale cannot be closer to the fp64 value than half of that)
    assert abs(float(s) - exact) <= 1e-6 * scale + 2.0 ** -149, (tag, float(s), exact)
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b), tag


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("P", SELECT_P)
def test_select_matches_the_restatement_bit_for_bit(cuda, P, content):
    """keep, loss_out, threshold_out and nnz_out equal the restatement's exactly, at the ranks k = 0, k in the middle and k = nnz - 1 (thresh
    below every value, so the selected value is the threshold) and with thresh above the selected value; masked_sum within 1e-6 relative of the
    fp64 sum (plus one fp32 denormal spacing) and identical between two calls.  'signed' runs in loss mode only (probabilities are never negative)."""
    P = _cap_trip() if P == "cap" else P
    rng = np.random.default_rng(P % 1000 + len(content))
    values = _values(content, P, rng)
    loss = (rng.random(P) * 3).astype(np.float32)
    nnz = int(np.count_nonzero(values))
    if content != "signed":
        for mkt in sorted({0, nnz // 2, max(nnz - 1, 0), nnz + 5}):
            _check_select(values, loss, mkt, -1.0)
        _check_select(values, loss, nnz // 2, 0.6)
    for mkt in sorted({0, P // 2, P - 1}):
        _check_select(values, values, mkt, None)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the probabilities
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ignore", [IGNORE, 0])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_label_prob_against_fp64(cuda, shape, ignore):
    """prob against the fp64 restatement.  The tolerance is not fixed in advance: the existing cross-entropy kernel's own deviation from the same
    reference on the same inputs, taken as |exp(-loss) - prob64|, is measured first, and prob may deviate twice that.  Zero rows are exactly 0.
    Measured on an MI355X (max over positions; CE kernel / prob kernel; the same for ignore_label 255 and 0):
        2x5x7x5:    8.070e-08 / 6.516e-08          3x37x53x21: 3.079e-07 / 3.334e-07"""
    from iseg_amd import kernels as K

    y, z = case(*shape)
    if ignore == 0:
        y = np.where(y == IGNORE, 0, y + 1)      # the same classes, stored one higher, with 0 as the ignored label
    C = shape[-1]
    want = R.label_prob(z, y, ignore)
    zd, yd = torch.from_numpy(z).cuda().reshape(-1, C), torch.from_numpy(y).cuda().reshape(-1).to(torch.int32)
    px, _, _ = K.softmax_ce_ignore(zd, yd, ignore, want_px=True)
    prob = K.ohem_label_prob(zd, yd, ignore)
    zero_rows = ~R.label_rows(y, ignore, C)[1]
    assert 0 < zero_rows.sum() < zero_rows.size
    ce_dev = float(np.abs(np.exp(-px.cpu().numpy().astype(np.float64)) - want)[~zero_rows].max())
    got = prob.cpu().numpy()
    prob_dev = float(np.abs(got.astype(np.float64) - want).max())
    print(f"label_prob {shape} ignore {ignore}: CE kernel deviates {ce_dev:.3e}, prob kernel {prob_dev:.3e}")
    assert ce_dev > 0
    assert prob_dev <= 2 * ce_dev, (prob_dev, ce_dev)
    assert not got[zero_rows].any() and (got[~zero_rows] > 0).all()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------------------------------
_PLAIN = {}


def _loss_kwargs(C, focal, weighted):
    kw = dict(num_class=C, ignore_label=IGNORE, batch_size=4)
    if focal:
        kw.update(use_focal_loss=True, focal_loss_gamma=2.0, focal_loss_alpha=0.25)
    if weighted:
        kw["class_weights"] = [0.5 + 0.25 * c for c in range(C)]
    return kw


def _plain(shape, focal, weighted):
    """per-position loss and d(sum loss)/d(logits) of the unselected loss, computed once per configuration and left unchanged"""
    from iseg_amd.losses.catecrossentropy_ignore_label import catecrossentropy_ignore_label_loss

    key = (shape, focal, weighted)
    if key not in _PLAIN:
        y, z = case(*shape)
        yd, zd = torch.from_numpy(y).cuda(), torch.from_numpy(z).cuda().requires_grad_(True)
        lv = catecrossentropy_ignore_label_loss(**_loss_kwargs(shape[-1], focal, weighted))(yd, zd)
        lv.sum().backward()
        _PLAIN[key] = (yd, zd.detach(), lv.detach(), zd.grad.reshape(-1, shape[-1]))
    return _PLAIN[key]


def _end_to_end(fn, shape, focal, weighted, thresh, min_kept):
    from iseg_amd import kernels as K

    N, C = shape[0], shape[-1]
    yd, zd, plain_loss, plain_grad = _plain(shape, focal, weighted)
    P = plain_loss.numel()
    z1 = zd.clone().requires_grad_(True)
    lv = fn(yd, z1)
    assert lv.shape == (P,)
    lv.sum().backward()
    # the selection the kernels made (the same calls, the same bits), and the restatement's
    y32 = yd.reshape(-1).to(torch.int32)
    if thresh is None:
        values = plain_loss
        want = R.select_values(plain_loss.cpu().numpy(), plain_loss.cpu().numpy(), min_kept * N, None)      # exact: fp32 compares on the same losses
        near = np.zeros(P, bool)
    else:
        values = K.ohem_label_prob(zd.reshape(-1, C), y32, IGNORE)
        want = R.ohem(zd.cpu().numpy(), yd.cpu().numpy(), plain_loss.cpu().numpy(), IGNORE, N, thresh, min_kept)
        near = np.abs(want["values"] - want["threshold"]) <= 1e-5 * want["threshold"]
    keep = K.ohem_select(values, plain_loss, min_kept * N, thresh)[0]
    assert near.sum() <= max(2, P // 1000), int(near.sum())
    ok = torch.from_numpy(~near).cuda()
    assert torch.equal(keep[ok].cpu(), torch.from_numpy(want["keep"][~near].astype(np.float32)))
    assert float(keep.sum()) < P and bool(keep.any()) == bool(want["keep"].any())      # (ties at the top of a clipped focal loss: nothing is strictly above)
    # outside the excluded pixels: the unselected loss times keep, the plain gradient times keep, bit for bit
    assert torch.equal(lv.detach()[ok], (plain_loss * keep)[ok])
    assert torch.equal(z1.grad.reshape(-1, C)[ok], (plain_grad * keep[:, None])[ok])
    # the fused mean: loss and gradient within 1e-6 relative of weighted_loss(...).mean() and its gradient
    z2 = zd.clone().requires_grad_(True)
    fn(yd, z2).mean().backward()
    z3 = zd.clone().requires_grad_(True)
    fm = fn.fused_mean(yd, z3, 1.0)
    fm.backward()
    mean = float(lv.detach().double().mean())
    assert abs(float(fm) - mean) <= 1e-6 * abs(mean), (float(fm), mean)
    assert torch.allclose(z3.grad, z2.grad, rtol=1e-6, atol=0), float((z3.grad - z2.grad).abs().max())
    return want


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "class_weights"])
@pytest.mark.parametrize("focal", [False, True], ids=["ce", "focal"])
@pytest.mark.parametrize("thresh,min_kept", [(0.05, 7), (0.7, 100000), (None, 7)])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_selected_loss_and_gradient_through_the_loss_factory(cuda, shape, thresh, min_kept, focal, weighted):
    """catecrossentropy_ignore_label_loss(post_compute_fn=get_ohem_fn(thresh, min_kept)): the keep mask is the restatement's except on pixels whose
    fp64 probability lies within 1e-5 relative of the fp64 threshold (at most max(2, 0.1 % of P), asserted); elsewhere the per-position loss
    is exactly the unselected loss times keep and the gradient exactly the plain gradient times keep.  (0.05, 7): the selected probability is
    the threshold; (0.7, 100000): the reference's default, k = nnz - 1; (None, 7): selection on the loss itself."""
    from iseg_amd.losses.catecrossentropy_ignore_label import catecrossentropy_ignore_label_loss
    from iseg_amd.losses.ohem import get_ohem_fn

    fn = catecrossentropy_ignore_label_loss(post_compute_fn=get_ohem_fn(thresh=thresh, min_kept=min_kept), **_loss_kwargs(shape[-1], focal, weighted))
    assert fn.fused_upsample_mean is None
    want = _end_to_end(fn, shape, focal, weighted, thresh, min_kept)
    if thresh == 0.05:
        assert want["threshold"] > thresh and want["k"] == min_kept * shape[0]
    if thresh == 0.7:
        assert want["k"] == want["nnz"] - 1


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_selected_loss_through_seg_foundation(cuda, shape):
    """SegFoundation(use_ohem=True).custom_losses: the main output selects with (ohem_thresh, 100000), the auxiliary output stays plain"""
    from iseg_amd.core_model import SegFoundation

    C = shape[-1]
    losses = SegFoundation(num_class=C, use_ohem=True, ohem_thresh=0.7, num_aux_loss=1).custom_losses(C, IGNORE, 4)
    _end_to_end(losses["output_1"], shape, False, False, 0.7, 100000)
    yd, zd, plain_loss, _ = _plain(shape, False, False)
    assert torch.equal(losses["output_2"](yd, zd), plain_loss)


def test_one_hot_rows_select_like_integer_labels(cuda):
    """ohem_selector with the reference's own y_true, the one-hot rows [P, C] (a zero row for an ignored pixel)"""
    from iseg_amd.losses.ohem import ohem_selector

    shape = SHAPES[0]
    C = shape[-1]
    yd, zd, plain_loss, _ = _plain(shape, False, False)
    yf = yd.reshape(-1)
    onehot = torch.zeros(yf.numel(), C, device="cuda")
    valid = yf != IGNORE
    onehot[valid, yf[valid]] = 1.0
    a = ohem_selector(plain_loss, onehot, zd.reshape(-1, C), batch_size=shape[0], thresh=0.05, min_kept=7)
    b = ohem_selector(plain_loss, yf, zd.reshape(-1, C), batch_size=shape[0], thresh=0.05, min_kept=7)
    assert torch.equal(a, b) and 0 < int((a != 0).sum()) < int((plain_loss != 0).sum())


# ---------------------------------------------------------------------------------------------------------------------------------------------
# guard bands, refusals
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [70, 4133])
def test_nothing_outside_the_buffers_is_written(cuda, P):
    """prob, keep, loss_out, the sums and the two fixed scratch blocks at exact size inside the poisoned arena: every byte around them stays poison"""
    from iseg_amd import kernels as K

    C = 21
    rng = np.random.default_rng(P)
    z = torch.from_numpy((4 * rng.standard_normal((P, C))).astype(np.float32)).cuda()
    y = torch.from_numpy(rng.integers(0, C, size=P).astype(np.int32)).cuda()
    prob0 = K.ohem_label_prob(z, y, IGNORE)
    px = K.softmax_ce_ignore(z, y, IGNORE, want_px=True)[0]
    want = [K.ohem_select(prob0, px, 9, 0.05, want_loss=True, want_sum=True), K.ohem_select(px, px, 9, None, want_loss=True, want_sum=True)]
    arena = GM.Arena(cuda, nbytes=8 << 20)
    with GM.guarded(arena):
        prob = K.ohem_label_prob(z, y, IGNORE)
        got = [K.ohem_select(prob, px, 9, 0.05, want_loss=True, want_sum=True), K.ohem_select(px, px, 9, None, want_loss=True, want_sum=True)]
    arena.check()
    sizes = sorted(r.end - r.start for r in arena.records)
    assert 4 * K.OHEM_STATE_INTS in sizes and 4 * K.OHEM_PARTIAL_FLOATS in sizes and sizes.count(4 * P) == 5      # prob, 2 x (keep, loss_out)
    assert torch.equal(prob, prob0)
    for g, w in zip(got, want):
        assert all(torch.equal(a, b) for a, b in zip(g, w))


def _select_args(P=64):
    dev = "cuda"
    f = lambda n: torch.zeros(n, dtype=torch.float32, device=dev)      # noqa: E731
    i = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)      # noqa: E731
    from iseg_amd import kernels as K

    return dict(values=f(P), loss=f(P), P=P, mkt=3, thresh=0.5, loss_mode=0, keep=f(P), loss_out=f(P), masked_sum=f(1), scale=1.0,
                threshold=f(1), nnz=i(1), state=i(K.OHEM_STATE_INTS), partials=f(K.OHEM_PARTIAL_FLOATS))


REFUSED_SELECT = {
    "null values": dict(values=None),
    "null keep": dict(keep=None),
    "null threshold_out": dict(threshold=None),
    "null nnz_out": dict(nnz=None),
    "null state": dict(state=None),
    "null loss with loss_out": dict(loss=None),
    "null partials with masked_sum": dict(partials=None),
    "P=0": dict(P=0),
    "P=2^31": dict(P=1 << 31),
    "values==keep": dict(alias=True),
    "min_kept_total<0": dict(mkt=-1),
    "loss mode index == P": dict(loss_mode=1, mkt=64),
}


@pytest.mark.parametrize("name", sorted(REFUSED_SELECT))
def test_select_launcher_refuses_bad_arguments(cuda, name):
    """ISEG_STATUS_ARG and a message that starts with the entry point's name; device tensors throughout, nothing is launched"""
    from iseg_amd import _hip
    from iseg_amd import kernels as K

    a = _select_args()
    kw = dict(REFUSED_SELECT[name])
    if kw.pop("alias", False):
        a["keep"] = a["values"]
    a.update(kw)
    p = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    status = _hip.lib().iseg_ohem_select(p(a["values"]), p(a["loss"]), a["P"], a["mkt"], a["thresh"], a["loss_mode"], p(a["keep"]), p(a["loss_out"]),
                                         p(a["masked_sum"]), a["scale"], p(a["threshold"]), p(a["nnz"]), p(a["state"]), p(a["partials"]), K.stream())
    message = _hip.last_error()
    assert status == -1, (name, status, message)
    assert message.startswith("iseg_ohem_select:"), message


@pytest.mark.parametrize("name", ["null logits", "null labels", "null prob", "P=0", "P=2^31", "C=0", "C=257"])
def test_label_prob_launcher_refuses_bad_arguments(cuda, name):
    from iseg_amd import _hip
    from iseg_amd import kernels as K

    z, y, prob = torch.zeros(8, 4, device="cuda"), torch.zeros(8, dtype=torch.int32, device="cuda"), torch.zeros(8, device="cuda")
    a = dict(logits=z.data_ptr(), labels=y.data_ptr(), prob=prob.data_ptr(), P=8, C=4)
    a.update({"null logits": dict(logits=None), "null labels": dict(labels=None), "null prob": dict(prob=None), "P=0": dict(P=0),
              "P=2^31": dict(P=1 << 31), "C=0": dict(C=0), "C=257": dict(C=257)}[name])
    status = _hip.lib().iseg_ohem_label_prob(a["logits"], a["labels"], a["P"], a["C"], IGNORE, a["prob"], K.stream())
    message = _hip.last_error()
    assert status == -1, (name, status, message)
    assert message.startswith("iseg_ohem_label_prob:"), message


# ---------------------------------------------------------------------------------------------------------------------------------------------
# one training step
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _trainer():
    from iseg_amd import heads
    from iseg_amd.core_env import common_env_setup
    from iseg_amd.core_optimizer import get_optimizer
    from iseg_amd.core_train import CoreTrain
    from iseg_amd.modelhelper import model_common_setup

    strategy = common_env_setup(use_one_device_strategy=True, mixed_precision=True, random_seed=3)
    model = heads.resnet18_aspp(build_input_size=(64, 64), dropout_rate=0.1)
    model.use_ohem, model.ohem_thresh = True, 0.7
    helper = model_common_setup(model, restore_checkpoint=False)
    helper.set_optimizer(get_optimizer(strategy, initial_lr=1e-3, end_lr=0.0, epoch_steps=20, train_epoch=1, warmup_steps=3, warmup_lr=1e-5,
                                       optimizer="adamw", adamw_weight_decay=0.05, clipnorm=None))
    tm = CoreTrain(helper, None).create_trainable_model(21, ignore_label=255, batch_size=4)
    assert tm._loss_fn(0).fused_mean.__name__ == "fused_ohem_mean"
    return tm


def _run(graphed, batches, steps=3):
    from iseg_amd import functional as F
    from iseg_amd import kernels as K
    from iseg_amd.graphs import GraphedTrainStep

    F._RNG_COUNTER[0] = 0
    F._DROP_PATH_POOL.__init__()
    tm = _trainer()
    w0 = tm.store.flat_w.clone()
    step = GraphedTrainStep(tm, warmup=1) if graphed else tm.train_step
    captured_streams, real_stream = set(), K.stream

    def stream():
        s = real_stream()
        if torch.cuda.is_current_stream_capturing():
            captured_streams.add(s)
        return s

    K.stream = stream
    try:
        losses = [float((step(*batches[i % len(batches)]))[0]) for i in range(steps)]
    finally:
        K.stream = real_stream
    torch.cuda.synchronize()
    cm = [m.metric.total_cm.clone() for ms in (tm.metrics.values() if isinstance(tm.metrics, dict) else [tm.metrics]) for m in ms][0]
    return losses, tm.store.flat_w.clone(), cm, step, w0, captured_streams


def test_ohem_training_steps_eager_twice_and_graphed_are_bit_identical(cuda):
    """three steps of a ResNet-18 + ASPP trainer with use_ohem=True: two eager runs give the same bits; the HIP-graph replay follows the eager run
    bit for bit (losses, weights, running confusion matrix); the running mIoU is updated; the capture stays on one stream and no environment
    variable changes"""
    from iseg_amd.data import synthetic_batch

    batches = [tuple(t.cuda() for t in synthetic_batch(4, 64, 64, seed=s)) for s in (5, 6, 7)]
    la, wa, cma, _, w0a, _ = _run(False, batches)
    lb, wb, cmb, _, w0b, _ = _run(False, batches)
    env = dict(os.environ)      # (after the eager runs: common_env_setup pins PYTHONHASHSEED to the seed)
    lg, wg, cmg, step, w0g, streams = _run(True, batches)
    assert torch.equal(w0a, w0b) and torch.equal(w0a, w0g), "the trainers did not start from the same weights"
    assert all(np.isfinite(la)) and len(set(la)) == 3
    assert la == lb and torch.equal(wa, wb) and torch.equal(cma, cmb)
    assert any(e.get("graph") is not None for e in step.entries.values()), "the step was never captured"
    assert la == lg, (la, lg)
    assert torch.equal(wa, wg), float((wa - wg).abs().max())
    assert int(cma.sum()) > 0 and torch.equal(cma, cmg), "the running mIoU was not updated"
    assert not torch.equal(wa, w0a)
    assert len(streams) == 1, f"the captured step launched on {len(streams)} streams"
    assert dict(os.environ) == env
