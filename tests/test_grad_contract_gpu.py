"""The gradient-buffer contract of the tape nodes, case by case (tests/grad_contract_cases.py), and of the optimizers behind them.

Parameter gradients never pass through autograd here: every Function.backward writes them into `param.grad`, a view of ParamStore.flat_g.  Each
run below starts from a flat_g filled with the sentinel 0.5 -- padding between the segments included -- and does one forward and one backward
through the call the layer makes:

    seeded     every parameter trainable: flat_g - 0.5 and dx match the fp64 oracle (an overwriting body loses the 0.5), padding still 0.5
    frozen     all / the even-indexed / the odd-indexed parameters frozen before the store exists: frozen segments and padding are exactly the
               sentinel, `p.grad` of a frozen parameter is still the store's view, trainable segments and dx match the oracle
    no dx      the inputs take no gradient (a model's first layer): parameter gradients match, dx is None
    shared     y = L(x1) + L(x2) and a second backward on a new batch without zeroing: the buffer holds the oracle's sum over all four uses

Bands: the case's (taken from the layer's parity test, see the table) relative to the largest entry of the reference gradient, plus
2^-23 |0.5 + g| for the one extra rounding of the sum with the sentinel.

The optimizer half: frozen segments of flat_g -- whatever lies in them -- enter neither clipnorm nor global_clipnorm, and frozen weights, moments
and bf16 shadows do not move."""
import pytest
import torch

from oracle import tf_ops as O
from tests import grad_contract_cases as T

pytestmark = pytest.mark.gpu

SENTINEL = 0.5


@pytest.fixture(autouse=True)
def _restore_policy():
    from iseg_amd import nn

    yield
    nn.set_compute_dtype(torch.float32)


_ORACLE = {}


def _oracle(case, built, seeds, shared):
    """computed once per (case, seeds, shared), shared among the runs, left unchanged"""
    key = (case.name, tuple(seeds), shared)
    if key not in _ORACLE:
        _ORACLE[key] = T.oracle(case, built, seeds, shared)
    return _ORACLE[key]


def _execute(case, monkeypatch, frozen=(), input_grad=True, seeds=(0,), shared=False, ran=None):
    """ran: a dict that receives, per Function the case covers, how often the run went through it"""
    from iseg_amd import functional as F
    from iseg_amd import kernels as K
    from iseg_amd import nn
    from iseg_amd.param_store import ParamStore

    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    if ran is not None:
        for name in case.covers:
            real = getattr(F, name).apply
            ran[name] = 0

            def counted(*a, _name=name, _real=real):
                ran[_name] += 1
                return _real(*a)

            monkeypatch.setattr(getattr(F, name), "apply", staticmethod(counted), raising=False)
    nn.set_compute_dtype(case.dtype)
    nn.set_device("cuda:0")
    built = case.build()
    for i in frozen:
        built.params[i].requires_grad_(False)
    store = ParamStore(built.params)
    store.flat_g.fill_(SENTINEL)
    views = [p.grad for p in built.params]
    dxs, shapes = [], []
    for seed in seeds:
        Xs = [[(t.cuda().to(case.dtype).requires_grad_(d and input_grad) if t.is_floating_point() else t.cuda()) for t, d in X]
              for X in T.batches(built, seed, shared)]
        ys = [T.as_tuple(built.run(X)) for X in Xs]
        y = [sum(parts[1:], parts[0]) for parts in zip(*ys)]
        shapes.append([tuple(t.shape) for t in y])
        if any(t.requires_grad for t in y):
            dys = [d.cuda().to(t.dtype) for d, t in zip(T.upstream(case, shapes[-1], seed), y)]
            torch.autograd.backward(y, dys)
        dxs.append([[t.grad if t.is_floating_point() else None for t in X] for X in Xs])
    K.deferred_flush()
    torch.cuda.synchronize()
    return built, store, views, dxs, shapes


def _within(got, ref, tol, what, sentinel=0.0, norm="max"):
    got = got.detach().cpu().double()
    if norm == "l2":      # the band of a parity test that measures the relative L2 error
        err = (got - sentinel - ref).norm().item()
        extra = (2.0 ** -23 * (sentinel + ref).abs()).norm().item() if sentinel else 0.0
        assert err <= tol * ref.norm().item() + extra, f"{what}: L2 err {err:.3e} against {tol:.1e} x {ref.norm().item():.3e}"
        return
    band = tol * ref.abs().max().item() + (2.0 ** -23 * (sentinel + ref).abs() if sentinel else 0.0)
    err = (got - sentinel - ref).abs()
    worst = (err - band).max().item()
    assert worst <= 0.0, f"{what}: max err {err.max().item():.3e} against {tol:.1e} x {ref.abs().max().item():.3e}"


def _check(case, run, ref, frozen=(), input_grad=True):
    built, store, views, dxs, shapes = run
    grads, rdxs, rshapes = ref
    assert shapes == rshapes
    norm = case.tol.get("norm", "max")
    pad = torch.ones(store.total, dtype=torch.bool)
    for i, (p, o, n) in enumerate(store.segments):
        pad[o:o + n] = False
        seg = store.flat_g[o:o + n]
        assert p.grad is views[i] and p.grad.data_ptr() == seg.data_ptr() and tuple(p.grad.shape) == tuple(p.shape), p.iseg_name
        if i in frozen:
            assert torch.equal(seg, torch.full_like(seg, SENTINEL)), f"frozen {p.iseg_name} received a gradient"
        else:
            _within(seg.view(p.shape), grads[i], case.tol["param"], p.iseg_name, SENTINEL, norm)
    padding = store.flat_g[pad.cuda()]
    assert torch.equal(padding, torch.full_like(padding, SENTINEL)), "the padding between the segments was written"
    for got_seed, ref_seed in zip(dxs, rdxs):
        for got_X, ref_X in zip(got_seed, ref_seed):
            for j, (g, r) in enumerate(zip(got_X, ref_X)):
                if r is None or not input_grad:
                    assert g is None, f"input {j} must take no gradient"
                else:
                    assert g is not None, f"input {j} received no gradient"
                    _within(g, r, case.tol["dx"], f"dx[{j}]", norm=norm)


def _reference_in_range(case, built):
    grads = _oracle(case, built, (0,), False)[0]
    T.assert_oracle_gradient_range(case, grads, built.params)


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.name)
def test_seeded_buffer_accumulates(cuda, case, monkeypatch):
    ran = {}
    run = _execute(case, monkeypatch, ran=ran)
    assert all(n >= 1 for n in ran.values()), f"the call did not take the route the case is about: {ran}"
    _reference_in_range(case, run[0])
    _check(case, run, _oracle(case, run[0], (0,), False))


@pytest.mark.parametrize("mask", ["all", "even", "odd"])
@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.name)
def test_frozen_parameters_receive_nothing(cuda, case, mask, monkeypatch):
    n = len(case.build().params)
    frozen = tuple(i for i in range(n) if mask == "all" or i % 2 == (0 if mask == "even" else 1))
    run = _execute(case, monkeypatch, frozen=frozen)
    _check(case, run, _oracle(case, run[0], (0,), False), frozen=frozen)


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.name)
def test_first_layer_without_input_gradient(cuda, case, monkeypatch):
    run = _execute(case, monkeypatch, input_grad=False)
    _check(case, run, _oracle(case, run[0], (0,), False), input_grad=False)


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.name)
def test_shared_parameters_sum_over_uses_and_batches(cuda, case, monkeypatch):
    run = _execute(case, monkeypatch, seeds=(0, 1), shared=True)
    _check(case, run, _oracle(case, run[0], (0, 1), True))


# ---------------------------------------------------------------------------------------------------------
# the optimizer half: frozen variables stay out of the update AND out of the clipping norms
# ---------------------------------------------------------------------------------------------------------
FROZEN = (1, 4)      # of the six variables of tests/test_optimizer_gpu.py: a/bias (300 elements) and b/beta (257: a segment with padding)


def _load_gradients(ps, step, seed, poison):
    """trainable segments: the gradients of tests/test_optimizer_gpu.py; frozen segments: what a backward body must never leave there"""
    from tests.test_optimizer_gpu import _grads

    gs = _grads(step, seed, nan=False)
    for i, (p, g) in enumerate(zip(ps, gs)):
        if i in FROZEN:
            g = torch.full_like(g, float("nan")) if poison == "nan" else g * 1e4
        p.grad.copy_(g.cuda())
    return [g.double() for i, g in enumerate(gs) if i not in FROZEN]


@pytest.mark.parametrize("poison", ["large", "nan"])
@pytest.mark.parametrize("clip", [dict(clipnorm=1.0), dict(global_clipnorm=2.0)], ids=["clipnorm", "global_clipnorm"])
@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_frozen_segments_stay_out_of_the_step_and_the_clipping_norms(cuda, kind, clip, poison):
    """two of six variables frozen before build(); their gradient segments hold large finite values or NaN.  The reference hands only trainable
    variables to apply_gradients, so clipnorm / global_clipnorm are formed over those alone: three steps follow O.clip_gradients + the oracle
    step over the trainable gradients, and the frozen weights, moments and bf16 shadows keep their bits"""
    from iseg_amd.optimizers.modern import SGD, AdamW
    from iseg_amd.param_store import ParamStore
    from tests.test_optimizer_gpu import _params

    ps = _params(6)
    for i in FROZEN:
        ps[i].requires_grad_(False)
    store = ParamStore(ps)
    opt = AdamW(learning_rate=1e-2, weight_decay=0.05, **clip) if kind == "adamw" else SGD(learning_rate=0.05, momentum=0.9, **clip)
    opt.build(store)
    live = [i for i in range(len(ps)) if i not in FROZEN]
    w = {i: ps[i].data.detach().cpu().double() for i in live}
    m = {i: torch.zeros_like(w[i]) for i in live}
    v = {i: torch.zeros_like(w[i]) for i in live}
    w0, shadow0 = store.flat_w.clone(), store.flat_bf16.clone()
    for step in range(3):
        gs = _load_gradients(ps, step, 13, poison)
        opt.apply_gradients()
        gd = O.clip_gradients(gs, **clip)
        for i, g in zip(live, gd):
            mult = float(getattr(ps[i], "lr_multiplier", 1.0))
            if kind == "adamw":
                w[i], m[i], v[i] = O.adamw_step(w[i], g, m[i], v[i], step + 1, 1e-2, mult, 0.05)
            else:
                w[i], m[i] = O.sgd_step(w[i], g, m[i], 0.05, mult, 0.9, 0.0, False)
        for i, (p, o, n) in enumerate(store.segments):
            if i in FROZEN:
                sl = slice(o, o + store.padded(n))
                assert torch.equal(store.flat_w[sl], w0[sl]) and torch.equal(store.flat_bf16[sl], shadow0[sl]), (step, p.iseg_name)
                assert float(opt.m[sl].abs().max()) == 0.0 and (kind == "sgd" or float(opt.v[sl].abs().max()) == 0.0), (step, p.iseg_name)
            else:
                got = p.data.cpu().double()
                assert torch.isfinite(got).all(), (step, p.iseg_name)
                err = (got - w[i]).abs()
                assert (err <= 3e-6 * torch.clamp(w[i].abs(), min=1.0)).all(), (step, p.iseg_name, err.max().item())
    assert torch.isfinite(store.flat_w).all() and torch.isfinite(store.flat_bf16.float()).all() and torch.isfinite(opt.m).all()
    assert kind == "sgd" or torch.isfinite(opt.v).all()


@pytest.mark.parametrize("stem", ["frozen_stem", "trainable_stem"])
def test_train_step_with_a_frozen_backbone_clips_over_the_trainable_gradients(cuda, stem):
    """one trainer.train_step of a ConvNeXt (depths 1-1-1-1, 8 / 16 / 32 / 64 filters) frozen behind a trainable head, AdamW with global_clipnorm:
    the frozen weights keep their bits, the frozen part of the gradient buffer is exactly zero, and the trainable update is the oracle step fed
    with the trainer's own trainable gradients -- so the clipping norm covers those only.  With the whole backbone frozen the tape ends at the
    head; with the stem left trainable the backward pass runs THROUGH the frozen blocks, LayerNorms and downsampling convolutions."""
    from iseg_amd import nn
    from iseg_amd.backbones import convnext as cx
    from iseg_amd.data import synthetic_batch
    from iseg_amd.layers.core_model_ext import SegManaged
    from iseg_amd.layers.model_builder import ConvNormAct
    from iseg_amd.optimizers.modern import AdamW
    from iseg_amd.trainer import TrainableModel
    from tests.util_models import randomize_parameters

    class Head(nn.Layer):
        def __init__(self, name="head"):
            super().__init__(name=name)
            self.end_conv = ConvNormAct(16, (1, 1), name=f"{self.name}/end_conv")

        def call(self, inputs, training=None):
            return self.end_conv(inputs[-1], training=training)

    nn.set_compute_dtype(torch.float32)
    nn.set_device("cuda:0")
    model = SegManaged(backbone_name="convnext_tiny", output_stride=32, num_class=21, build_input_size=(64, 64), name="seg",
                       backbone_custom_fn=lambda return_endpoints=False: cx.ConvNeXt(depths=[1, 1, 1, 1], filters_list=[8, 16, 32, 64],
                                                                                     return_endpoints=return_endpoints))
    model.head = Head()
    model.build_with_dummy()
    frozen = {id(p) for p in model.backbone.parameters() if stem == "frozen_stem" or "downsample_layers/0/" not in p.iseg_name}
    for p in model.backbone.parameters():
        p.requires_grad_(id(p) not in frozen)
    assert stem == "frozen_stem" or len(frozen) < len(list(model.backbone.parameters()))
    clip = 0.05      # far below the gradient norm of a fresh model: the clipping factor is 0.05 / ||g||
    tm = TrainableModel(model, optimizer=AdamW(learning_rate=1e-2, weight_decay=0.0, global_clipnorm=clip), loss=model.custom_losses(21, 255, 2),
                        loss_weights=model.custom_losses_weights(), metrics=model.custom_metrics(21, 255))
    randomize_parameters(model, 4)
    store = tm.store
    assert 0 < len(frozen) < len(store.params)
    w0 = store.flat_w.clone()
    x, y = synthetic_batch(2, 64, 64, seed=5)
    loss = tm.train_step(x.cuda(), y.cuda())
    torch.cuda.synchronize()
    assert torch.isfinite(torch.as_tensor(float(loss[0])))
    live = [(p, o, n) for p, o, n in store.segments if id(p) not in frozen]
    for p, o, n in store.segments:
        if id(p) in frozen:
            sl = slice(o, o + store.padded(n))
            assert torch.equal(store.flat_w[sl], w0[sl]), p.iseg_name
            assert float(store.flat_g[sl].abs().max()) == 0.0, f"frozen {p.iseg_name} received a gradient"
    gs = [store.flat_g[o:o + n].cpu().double() for _, o, n in live]
    gnorm = torch.sqrt(sum((g * g).sum() for g in gs)).item()
    assert gnorm > 4 * clip, gnorm
    for (p, o, n), g in zip(live, O.clip_gradients(gs, global_clipnorm=clip)):
        start = w0[o:o + n].cpu().double()
        want, _, _ = O.adamw_step(start, g, torch.zeros_like(start), torch.zeros_like(start), 1, 1e-2, float(getattr(p, "lr_multiplier", 1.0)), 0.0)
        err = (store.flat_w[o:o + n].cpu().double() - want).abs()
        assert (err <= 3e-6 * torch.clamp(want.abs(), min=1.0)).all(), (p.iseg_name, err.max().item())
