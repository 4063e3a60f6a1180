"""The fused JointPyramidUpsampling tail (functional.jpu_tail, csrc/jpu.hip): four branches depthwise 3 x 3 (dilation 1, 2, 4, 8, with bias) -> BN
folded into the pointwise GEMM over one tensor, forward and backward, against fp64 CPU autograd of the composed tail -- fp32 and bf16 storage,
training and moving statistics, at the smallest shapes at which each mechanism can go wrong (see CASES).  Also: a large per-channel mean, the
statistics message, run-to-run bit identity, the predicate's refusals (which fall back to the composed route), the launchers inside guard-band
memory with exact-size and short workspaces, and an inference backward after an in-place update of the moving statistics.

Bounds are those of tests/test_sepconv_fused_gpu.py, which tests the same arithmetic: fp32 1e-4 in max-norm relative error against fp64; bf16
fused error <= 2 x composed error + 1e-3.  The depthwise bias gradient under training statistics is zero up to rounding (the BN removes a
per-channel constant), so it is measured against dbeta_r, a sum of the same terms at the same scale."""
import pytest
import torch

from oracle import tf_ops as O

pytestmark = pytest.mark.gpu

RATES = (1, 2, 4, 8)
PER_RATE = ("v", "ddw", "ddb", "dpw", "dgamma", "dbeta", "moving_mean", "moving_variance")
KEYS = ("dx",) + tuple(f"{k}_{r}" for r in RATES for k in PER_RATE)


@pytest.fixture(autouse=True)
def _restore_policy():
    from iseg_amd import nn

    yield
    nn.set_compute_dtype(torch.float32)


class _Tail:
    pass


def _tail(C, Cout, dtype, seed=0, bias=None):
    """the twelve layers of the tail with random variables; bias: [4, C] depthwise biases instead of N(0, 0.1)"""
    from iseg_amd import nn
    from iseg_amd.layers.base_layers import BatchNormalization, Conv2D, DepthwiseConv2D
    from iseg_amd.param_store import ParamStore

    nn.set_compute_dtype(dtype)
    nn.set_device("cuda:0")
    t = _Tail()
    t.dws = [DepthwiseConv2D((3, 3), padding="same", dilation_rate=r, name=f"tail/dw_{r}") for r in RATES]
    t.bns = [BatchNormalization(momentum=0.9, epsilon=1e-3, synchronized=True, name=f"tail/bn_{r}") for r in RATES]
    t.pws = [Conv2D(Cout, (1, 1), padding="same", use_bias=False, name=f"tail/pw_{r}") for r in RATES]
    for layer in t.dws + t.bns + t.pws:
        layer.build((1, 1, 1, C))
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for i, (dw, bn, pw) in enumerate(zip(t.dws, t.bns, t.pws)):
            dw.depthwise_kernel.copy_((torch.randn(3, 3, C, 1, generator=g) / 3).cuda())
            dw.bias.copy_((torch.randn(C, generator=g) * 0.1 if bias is None else bias[i]).cuda())
            bn.gamma.copy_((torch.rand(C, generator=g) + 0.5).cuda())
            bn.beta.copy_((torch.randn(C, generator=g) * 0.1).cuda())
            pw.kernel.copy_((torch.randn(1, 1, C, Cout, generator=g) * C ** -0.5).cuda())
            bn.moving_mean.copy_((torch.randn(C, generator=g) * 0.1).cuda())
            bn.moving_variance.copy_((torch.rand(C, generator=g) + 0.5).cuda())
    t.store = ParamStore([p for layer in t.dws + t.bns + t.pws for p in layer.parameters()])
    t.store.sync_shadow()
    t.init_stats = [(bn.moving_mean.clone(), bn.moving_variance.clone()) for bn in t.bns]
    return t


def _run(t, x, dvs, training, fused, monkeypatch):
    from iseg_amd import functional as F

    monkeypatch.setenv("ISEG_JPU_FUSED", "1" if fused else "0")
    t.store.zero_grad()
    for bn, (mm, mv) in zip(t.bns, t.init_stats):
        bn.moving_mean.copy_(mm)
        bn.moving_variance.copy_(mv)
    xg = x.detach().requires_grad_(True)      # an alias: a misaligned view stays misaligned
    vs = F.jpu_tail(xg, t.dws, t.bns, [pw.kernel for pw in t.pws], training)
    torch.autograd.backward(list(vs), list(dvs))
    torch.cuda.synchronize()
    out = dict(dx=xg.grad.clone())
    for r, v, dw, bn, pw in zip(RATES, vs, t.dws, t.bns, t.pws):
        out.update({f"v_{r}": v.detach().clone(), f"ddw_{r}": dw.depthwise_kernel.grad.clone(), f"ddb_{r}": dw.bias.grad.clone(),
                    f"dpw_{r}": pw.kernel.grad.clone(), f"dgamma_{r}": bn.gamma.grad.clone(), f"dbeta_{r}": bn.beta.grad.clone(),
                    f"moving_mean_{r}": bn.moving_mean.clone(), f"moving_variance_{r}": bn.moving_variance.clone()})
    return out


def _reference(t, x, dvs, training):
    """fp64 CPU autograd of the composed tail: per rate depthwise (with bias) -> BN -> 1 x 1, the four input gradients summed by autograd"""
    xd = x.detach().cpu().double().requires_grad_(True)
    out, vs = {}, []
    params = []
    for r, dw, bn, pw, (mm, mv) in zip(RATES, t.dws, t.bns, t.pws, t.init_stats):
        p = {k: v.detach().cpu().double().requires_grad_(True) for k, v in
             dict(ddw=dw.depthwise_kernel, ddb=dw.bias, dgamma=bn.gamma, dbeta=bn.beta, dpw=pw.kernel).items()}
        mm, mv = mm.cpu().double(), mv.cpu().double()
        z = O.depthwise_conv2d(xd, p["ddw"], p["ddb"], 1, r, "same")
        if training:
            y, mean, var = O.batch_norm_train(z, p["dgamma"], p["dbeta"], 1e-3)
            mm, mv = O.moving_update(mm, mean.detach(), 0.9), O.moving_update(mv, var.detach(), 0.9)
        else:
            y = O.batch_norm_infer(z, p["dgamma"], p["dbeta"], mm, mv, 1e-3)
        v = O.conv2d(y, p["dpw"], None, 1, 1, "same")
        vs.append(v)
        params.append(p)
        out.update({f"v_{r}": v.detach(), f"moving_mean_{r}": mm, f"moving_variance_{r}": mv})
    torch.autograd.backward(vs, [dv.detach().cpu().double() for dv in dvs])
    for r, p in zip(RATES, params):
        out.update({f"{k}_{r}": v.grad for k, v in p.items()})
    out["dx"] = xd.grad
    return out


def _amax(t):
    return t.detach().cpu().double().abs().max().item()


def _err(got, want, scale=None):
    return (got.detach().cpu().double() - want).abs().max().item() / max(_amax(want) if scale is None else scale, 1e-12)


def _errors(got, ref, training):
    """max-norm relative error per key; ddb_r under training statistics (reference zero up to rounding): max |ddb_r| over max |dbeta_r|"""
    errs = {}
    for k in KEYS:
        if training and k.startswith("ddb_"):
            errs[k] = _amax(got[k]) / max(_amax(ref["dbeta_" + k[4:]]), 1e-12)
        else:
            errs[k] = _err(got[k], ref[k])
    return errs


def _inputs(N, H, W, C, Cout, dtype, seed):
    g = torch.Generator().manual_seed(seed + 100)
    x = torch.randn(N, H, W, C, generator=g)
    dvs = [torch.randn(N, H, W, Cout, generator=g).to("cuda", dtype) for _ in RATES]
    return x.to("cuda", dtype), dvs


# N, H, W, C, Cout
CASES = [
    (1, 5, 6, 8, 16),         # every non-centre tap of rate 8 falls in the padding, most of rate 4's do too; one chunk
    (1, 9, 17, 8, 24),        # one row and one column just past rate 8; the width crosses a 16-wide tile
    (2, 19, 21, 24, 16),      # three tiles each way (a rate-8 halo covers a whole neighbouring 8-row tile); three chunks against groups of two; two samples
    (1, 6, 6, 1536, 64),      # the layer's real channel count: the channel-group loop
    (16, 8, 8, 64, 64),       # many samples through the statistics partials
]
IDS = [f"N{c[0]}_{c[1]}x{c[2]}_C{c[3]}to{c[4]}" for c in CASES]


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fp32_against_fp64(cuda, case, training, monkeypatch):
    N, H, W, C, Cout = case
    t = _tail(C, Cout, torch.float32, seed=sum(case))
    x, dvs = _inputs(N, H, W, C, Cout, torch.float32, sum(case))
    from iseg_amd import functional as F

    assert F.jpu_tail_supported(x, t.dws, t.bns, [pw.kernel for pw in t.pws])
    got = _run(t, x, dvs, training, True, monkeypatch)
    ref = _reference(t, x, dvs, training)
    errs = _errors(got, ref, training)
    print({k: f"{v:.2e}" for k, v in errs.items()})
    bad = {k: v for k, v in errs.items() if v > 1e-4}
    assert not bad, bad


def _bf16_bad(fused, composed, ref, training):
    ef, ec = _errors(fused, ref, training), _errors(composed, ref, training)
    print({k: (f"{ef[k]:.2e}", f"{ec[k]:.2e}") for k in KEYS})
    return {k: (ef[k], ec[k]) for k in KEYS if ef[k] > 2 * ec[k] + 1e-3}


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_bf16_within_twice_composed_error(cuda, case, training, monkeypatch):
    N, H, W, C, Cout = case
    t = _tail(C, Cout, torch.bfloat16, seed=sum(case))
    x, dvs = _inputs(N, H, W, C, Cout, torch.bfloat16, sum(case))
    fused = _run(t, x, dvs, training, True, monkeypatch)
    composed = _run(t, x, dvs, training, False, monkeypatch)
    ref = _reference(t, x, dvs, training)
    bad = _bf16_bad(fused, composed, ref, training)
    assert not bad, bad


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_large_channel_mean(cuda, dtype, monkeypatch):
    """a depthwise bias of about 4 standard deviations of dw_r(x): the fold's cancellation (z W' against c^T W, G against mean * dbeta) shows up
    here first"""
    N, H, W, C, Cout = 3, 20, 20, 64, 96
    x, dvs = _inputs(N, H, W, C, Cout, dtype, 5)
    t = _tail(C, Cout, dtype, seed=5)
    xd = x.cpu().double()
    bias = torch.stack([4.0 * O.depthwise_conv2d(xd, dw.depthwise_kernel.detach().cpu().double(), None, 1, r, "same").std((0, 1, 2))
                        for r, dw in zip(RATES, t.dws)]).float()
    with torch.no_grad():
        for dw, b in zip(t.dws, bias):
            dw.bias.copy_(b.cuda())
    t.store.sync_shadow()
    for r, dw in zip(RATES, t.dws):
        z = O.depthwise_conv2d(xd, dw.depthwise_kernel.detach().cpu().double(), dw.bias.detach().cpu().double(), 1, r, "same")
        ratio = (z.mean((0, 1, 2)).abs() / z.std((0, 1, 2))).median().item()
        assert 2.5 < ratio < 8, (r, ratio)
    fused = _run(t, x, dvs, True, True, monkeypatch)
    ref = _reference(t, x, dvs, True)
    if dtype == torch.float32:
        errs = _errors(fused, ref, True)
        print({k: f"{v:.2e}" for k, v in errs.items()})
        assert not {k: v for k, v in errs.items() if v > 1e-4}, errs
    else:
        composed = _run(t, x, dvs, True, False, monkeypatch)
        bad = _bf16_bad(fused, composed, ref, True)
        assert not bad, bad


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("N,H,W,C", [(2, 19, 21, 24), (1, 5, 6, 8)])
def test_stats_message(cuda, dtype, N, H, W, C):
    """the four packed [sum z | sum z^2 | count] messages of iseg_bn_stats, over the stored z; z itself against the oracle"""
    from iseg_amd import kernels as K

    g = torch.Generator().manual_seed(2)
    x = torch.randn(N, H, W, C, generator=g).to("cuda", dtype)
    w = (torch.randn(4, 9, C, generator=g) / 3).cuda()
    b = (torch.randn(4, C, generator=g) * 0.5).cuda()
    z, packed = K.jpu_dwconv3x4_stats(x, w, b, stats=True)
    assert tuple(z.shape) == (4, N, H, W, C) and tuple(packed.shape) == (4, 2 * C + 1)
    z2, none = K.jpu_dwconv3x4_stats(x, w, b, stats=False)
    assert none is None and torch.equal(z, z2)
    for i, r in enumerate(RATES):
        zr = O.depthwise_conv2d(x.cpu().double(), w[i].cpu().double().reshape(3, 3, C, 1), b[i].cpu().double(), 1, r, "same")
        assert _err(z[i], zr) < (1e-5 if dtype == torch.float32 else 8e-3), r
        zs = z[i].cpu().double().reshape(-1, C)      # the message sums the stored z
        want = torch.cat([zs.sum(0), (zs * zs).sum(0), torch.tensor([float(zs.shape[0])], dtype=torch.float64)])
        assert _err(packed[i], want) < 1e-5, r
        assert packed[i, -1].item() == zs.shape[0]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_two_runs_bit_identical(cuda, dtype, monkeypatch):
    N, H, W, C, Cout = 16, 8, 8, 64, 64
    t = _tail(C, Cout, dtype, seed=4)
    x, dvs = _inputs(N, H, W, C, Cout, dtype, 4)
    a = _run(t, x, dvs, True, True, monkeypatch)
    b = _run(t, x, dvs, True, True, monkeypatch)
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k


def _forbid_fused(monkeypatch):
    from iseg_amd import kernels as K

    def never(*a, **kw):
        raise AssertionError("the fused launcher ran on a route that must be composed")

    monkeypatch.setattr(K, "jpu_dwconv3x4_stats", never)
    monkeypatch.setattr(K, "jpu_bnfold_dwconv3x4_bwd", never)


def test_predicate_refusals_fall_back(cuda, monkeypatch):
    """C = 12, a view of x misaligned by one element, ISEG_JPU_FUSED=0: the composed operators run, bit for bit, and the fused launchers are not
    called.  (At C = 12 the composed depthwise kernels refuse as well -- they need C % 8 == 0 too -- so no tail of that width can run on either
    route: the predicate's refusal is checked, and that the error is the composed operator's, the same on both routes.)"""
    from iseg_amd import _hip
    from iseg_amd import functional as F
    from iseg_amd import kernels as K

    t = _tail(12, 16, torch.float32, seed=1)
    x, dvs = _inputs(2, 6, 6, 12, 16, torch.float32, 1)
    assert not K.jpu_supported(2, 6, 6, 12, torch.float32)
    assert not F.jpu_tail_supported(x, t.dws, t.bns, [pw.kernel for pw in t.pws])
    messages = []
    for fused in (True, False):
        with pytest.raises(_hip.HipCallError) as e:
            _run(t, x, dvs, True, fused, monkeypatch)
        messages.append(str(e.value))
    assert messages[0] == messages[1] and "iseg_dwconv2d_fwd" in messages[0], messages
    # a misaligned (contiguous) view of x
    t = _tail(64, 32, torch.bfloat16, seed=2)
    x, dvs = _inputs(2, 9, 9, 64, 32, torch.bfloat16, 2)
    pwk = [pw.kernel for pw in t.pws]
    buf = torch.empty(x.numel() + 1, dtype=x.dtype, device=x.device)
    xm = buf[1:].view(x.shape)
    xm.copy_(x)
    assert xm.data_ptr() % 16 and not F.jpu_tail_supported(xm, t.dws, t.bns, pwk)
    assert F.jpu_tail_supported(x, t.dws, t.bns, pwk)
    b = _run(t, xm, dvs, True, False, monkeypatch)
    fused_aligned = _run(t, x, dvs, True, True, monkeypatch)
    _forbid_fused(monkeypatch)
    a = _run(t, xm, dvs, True, True, monkeypatch)      # refused: the composed operators run on the view as it is
    c = _run(t, x, dvs, True, False, monkeypatch)      # ISEG_JPU_FUSED=0 on tensors the predicate accepts
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k
        assert torch.equal(c[k], b[k]), k
    assert any(not torch.equal(fused_aligned[k], b[k]) for k in KEYS)      # the fused route is another computation: the comparison above is not vacuous
    ref = _reference(t, x, dvs, True)
    assert _err(a["v_8"], ref["v_8"]) < 2e-2


def _launch_both(K, x, w, b, D, train, fwd_short=None, bwd_short=None):
    N, H, W, C = x.shape
    z, packed = K.jpu_dwconv3x4_stats(x, w, b, stats=True, ws_bytes=fwd_short)
    ones = torch.ones((4, C), dtype=torch.float32, device=x.device)
    sums = torch.zeros((4, 2 * C), dtype=torch.float32, device=x.device)
    dw = torch.zeros((4, 9, C), dtype=torch.float32, device=x.device)
    db = torch.zeros((4, C), dtype=torch.float32, device=x.device)
    dx = K.jpu_bnfold_dwconv3x4_bwd(D, z, x, w, sums[:, :C].contiguous(), ones, ones, sums, 1.0 / (N * H * W), train, dw, db, ws_bytes=bwd_short)
    return z, packed, dx, dw, db


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_launchers_in_guarded_memory_and_short_workspaces(cuda, dtype):
    """both launchers with workspaces of exactly iseg_jpu_partials_bytes, full of NaN, every buffer between bands of poison at addresses = 16
    (mod 512): the bands stay untouched and the results are those of the oracle; one byte (and the guard's 16 bytes) short: ISEG_ERR_WORKSPACE
    from the launcher by name, and nothing ran -- every buffer of the refused call is still poison"""
    from iseg_amd import _hip
    from iseg_amd import kernels as K
    from tests import guarded_memory as GM

    N, H, W, C = 2, 19, 21, 24
    g = torch.Generator().manual_seed(7)
    arena = GM.Arena(cuda, 32 << 20)
    lib = _hip.lib()
    need_f, need_b = lib.iseg_jpu_partials_bytes(N, H, W, C, 0), lib.iseg_jpu_partials_bytes(N, H, W, C, 1)
    assert need_f > 0 and need_b > 0

    def operands():
        out = []
        for shape, scale in (((N, H, W, C), 1.0), ((4, 9, C), 1 / 3), ((4, C), 0.5), ((4, N, H, W, C), 1.0)):
            src = (torch.randn(shape, generator=torch.Generator().manual_seed(len(out) + 7)) * scale)
            d = arena.alloc(shape, dtype if len(shape) >= 4 else torch.float32, "operand")
            d.copy_(src)
            out.append(d)
        return out

    with GM.guarded(arena):
        x, w, b, D = operands()
        z, packed, dx, dw, db = _launch_both(K, x, w, b, D, 0)
        torch.cuda.synchronize()
        arena.check()
        assert arena.untouched("output")[0] == 0
    xd, Dd = x.cpu().double(), D.cpu().double()
    want_dx = 0
    for i, r in enumerate(RATES):
        k = w[i].cpu().double().reshape(3, 3, C, 1).requires_grad_(True)
        bb = b[i].cpu().double().requires_grad_(True)
        xr = xd.clone().requires_grad_(True)
        zr = O.depthwise_conv2d(xr, k, bb, 1, r, "same")
        zr.backward(Dd[i])
        tol = 1e-5 if dtype == torch.float32 else 8e-3
        assert _err(z[i], zr.detach()) < tol, r
        assert _err(dw[i], k.grad.reshape(9, C)) < 1e-4 and _err(db[i], bb.grad) < 1e-4, r
        want_dx = want_dx + xr.grad
    assert _err(dx, want_dx) < (1e-5 if dtype == torch.float32 else 8e-3)
    assert not torch.isnan(packed).any()
    # one byte short, forward then backward
    for which, short in (("iseg_jpu_dwconv3x4_stats", dict(fwd_short=need_f - 1)), ("iseg_jpu_bnfold_dwconv3x4_bwd", dict(bwd_short=need_b - 1))):
        arena.reset()
        with GM.guarded(arena):
            x, w, b, D = operands()
            since = len(arena.records)
            if which.endswith("bwd"):      # a complete forward first; the refused call's own buffers are counted from here
                z, _ = K.jpu_dwconv3x4_stats(x, w, b, stats=False)
                since = len(arena.records)
                dwb = [arena.alloc(s, torch.float32, "output") for s in ((4, 9, C), (4, C))]
                with pytest.raises(_hip.HipCallError, match=r"status -4\b") as e:
                    K.jpu_bnfold_dwconv3x4_bwd(D, z, x, w, None, None, None, None, 0.0, 0, dwb[0], dwb[1], ws_bytes=need_b - 1)
            else:
                with pytest.raises(_hip.HipCallError, match=r"status -4\b") as e:
                    K.jpu_dwconv3x4_stats(x, w, b, stats=True, **{"ws_bytes": need_f - 1})
            assert str(e.value).startswith(which + " failed with status"), e.value
            torch.cuda.synchronize()
            arena.check()
            untouched, total = arena.untouched(role=None, since=since)
            assert total >= 2 and untouched == total, (which, untouched, total)
    # the guard's own short mode: every workspace 16 bytes short
    arena.reset()
    with GM.guarded(arena, short_workspace=16) as scope:
        x, w, b, D = operands()
        with pytest.raises(_hip.HipCallError, match=r"status -4\b") as e:
            K.jpu_dwconv3x4_stats(x, w, b, stats=True)
        assert str(e.value).startswith("iseg_jpu_dwconv3x4_stats failed with status")
        arena.check()
        untouched, total = arena.untouched(role=None, since=scope.refused_from)
        assert total >= 1 and untouched == total


def test_inference_backward_after_moving_stats_update(cuda, monkeypatch):
    """a moving-statistics forward, then a training-mode call that updates the moving statistics in place, then the first call's backward:
    it must use the statistics of its own forward"""
    from iseg_amd import functional as F

    monkeypatch.setenv("ISEG_JPU_FUSED", "1")
    N, H, W, C, Cout = 2, 8, 8, 64, 32
    t = _tail(C, Cout, torch.float32, seed=9)
    x, dvs = _inputs(N, H, W, C, Cout, torch.float32, 9)
    ref = _reference(t, x, dvs, False)
    pwk = [pw.kernel for pw in t.pws]
    t.store.zero_grad()
    xg = x.clone().requires_grad_(True)
    vs = F.jpu_tail(xg, t.dws, t.bns, pwk, False)
    with torch.no_grad():
        F.jpu_tail(x * 3 + 1, t.dws, t.bns, pwk, True)      # moves moving_mean / moving_variance in place
    for bn, (mm, _) in zip(t.bns, t.init_stats):
        assert not torch.equal(bn.moving_mean, mm)
    torch.autograd.backward(list(vs), list(dvs))
    assert _err(xg.grad, ref["dx"]) < 1e-4
    for r, v, dw, bn, pw in zip(RATES, vs, t.dws, t.bns, t.pws):
        assert _err(v, ref[f"v_{r}"]) < 1e-4
        assert _err(pw.kernel.grad, ref[f"dpw_{r}"]) < 1e-4
        assert _err(bn.gamma.grad, ref[f"dgamma_{r}"]) < 1e-4
        assert _err(dw.depthwise_kernel.grad, ref[f"ddw_{r}"]) < 1e-4
        assert _err(dw.bias.grad, ref[f"ddb_{r}"]) < 1e-4
