"""Several convolutions of one input (csrc/conv_igemm.hip iseg_conv2d_branches_*; reference layers/aspp.py:33-52, the pixel-level 1x1 and the
dilated 3x3 branches): grouped forward and weight gradient, K-joined data gradient, through the C ABI against the oracle's keras Conv2D
restatement (summed over the branches for dx) and against the single-branch entry points on the same operands; then the ASPP layer on the
grouped route against its per-branch route."""
import ctypes as C

import pytest
import torch

from oracle import tf_ops as O
from tests.test_kernels_gpu import close, q, rnd

pytestmark = pytest.mark.gpu
BF = torch.bfloat16

# (N, H, W, Cin), Cout, [(kernel, dilation), ...]
CASES = [
    ((2, 8, 8, 64), 64, [(1, 1), (3, 3), (3, 6), (3, 9)]),      # dilation 9 > map: every non-centre tap is halo; M = 128: one tile; one K-step per tap
    ((1, 8, 12, 128), 128, [(3, 1), (3, 4)]),                   # M = 96 < one tile; two K-steps per tap; non-square map
    ((3, 16, 16, 64), 192, [(1, 1), (3, 2), (3, 5), (3, 9)]),   # several row tiles; the joined data gradient's N = 64 < BN
    ((2, 8, 8, 64), 64, [(3, 3)]),                              # one branch only
]
_REF = {}


def _problem(ci):
    """operands and the fp64 oracle of a case, computed once and shared (never written to)"""
    if ci in _REF:
        return _REF[ci]
    shape, Cout, taps = CASES[ci]
    N, H, W, Cin = shape
    x, xr = q(rnd(shape, 1), BF)
    xx = xr.clone().requires_grad_(True)
    ws, wrs, dys, ys, gws = [], [], [], [], []
    for i, (kk, d) in enumerate(taps):
        w, wr = q(rnd((kk, kk, Cin, Cout), 10 + i, (kk * kk * Cin) ** -0.5), BF)
        dy, dyr = q(rnd((N, H, W, Cout), 20 + i), BF)
        ww = wr.clone().requires_grad_(True)
        yo = O.conv2d(xx, ww, None, 1, d)
        yo.backward(dyr)
        ws.append(w), wrs.append(ww), dys.append(dy), ys.append(yo.detach())
        gws.append(ww.grad)
    _REF[ci] = dict(x=x, ws=ws, dys=dys, ys=ys, gws=gws, dx=xx.grad)
    return _REF[ci]


def _table(k, ci):
    shape, Cout, taps = CASES[ci]
    return k.conv_branches(*shape, Cout, [(kk, kk, d, d) for kk, d in taps])


def _geom(k, ci, b):
    (N, H, W, Cin), Cout, taps = CASES[ci]
    kk, d = taps[b]
    Ho, pt = k.same_pad(H, kk, 1, d)
    Wo, pl = k.same_pad(W, kk, 1, d)
    return k.conv_geom(N, H, W, Cin, Cout, kk, kk, 1, 1, d, d, pt, pl, Ho, Wo, 1)


def _wt(w):
    return w.reshape(-1, w.shape[3]).t().contiguous()


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_branches_forward(cuda, ci):
    from iseg_amd import kernels as k

    r = _problem(ci)
    assert k.conv2d_branches_supported(_table(k, ci), BF)
    ys = k.conv2d_branches_fwd(r["x"], [_wt(w) for w in r["ws"]], _table(k, ci))
    for b, (y, yo) in enumerate(zip(ys, r["ys"])):
        close(y, yo, BF, f"branches fwd, branch {b}")
        close(y, k.conv2d_igemm_fwd(r["x"], r["ws"][b], None, _geom(k, ci, b)).double().cpu(), BF, f"branches fwd vs single, branch {b}")


def test_branches_forward_bias_and_column_slices(cuda):
    """every branch writes its column slice of one wide buffer (ldy > Cout, y_col) and adds its own bias; the other columns stay untouched"""
    from iseg_amd import _hip, kernels as k

    ci = 0
    (N, H, W, Cin), Cout, taps = CASES[ci]
    r = _problem(ci)
    t = _table(k, ci)
    wts = [_wt(w) for w in r["ws"]]
    biases = [rnd((Cout,), 30 + b).float().cuda() for b in range(len(taps))]
    ld = (len(taps) + 1) * Cout
    buf = torch.full((N * H * W, ld), 3.0, dtype=BF, device="cuda")
    for b in range(len(taps)):
        t.b[b].wt, t.b[b].bias, t.b[b].y, t.b[b].ldy, t.b[b].y_col = wts[b].data_ptr(), biases[b].data_ptr(), buf.data_ptr(), ld, (b + 1) * Cout
    _hip.call("iseg_conv2d_branches_fwd", r["x"].data_ptr(), C.byref(t), k.dt(BF), None, 0, k.stream())
    assert torch.all(buf[:, :Cout] == 3.0)
    for b in range(len(taps)):
        want = r["ys"][b].reshape(-1, Cout) + biases[b].double().cpu()
        close(buf[:, (b + 1) * Cout:(b + 2) * Cout], want, BF, f"branches fwd into a slice, branch {b}")


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_branches_data_gradient(cuda, ci):
    from iseg_amd import kernels as k

    r = _problem(ci)
    (N, H, W, Cin), Cout, taps = CASES[ci]
    dx = k.conv2d_branches_bwd_data([d.reshape(-1, Cout) for d in r["dys"]], [Cout] * len(taps), r["ws"], _table(k, ci))
    close(dx, r["dx"], BF, "branches dx", bf16_tol=1.5e-2)
    single = sum(k.conv2d_igemm_bwd_data(r["dys"][b], r["ws"][b], _geom(k, ci, b)).double().cpu() for b in range(len(taps)))
    close(dx, single, BF, "branches dx vs the single-branch sum", bf16_tol=1.5e-2)
    res, resr = q(rnd((N, H, W, Cin), 40), BF)
    dx = k.conv2d_branches_bwd_data([d.reshape(-1, Cout) for d in r["dys"]], [Cout] * len(taps), r["ws"], _table(k, ci), residual=res)
    close(dx, r["dx"] + resr, BF, "branches dx + residual", bf16_tol=1.5e-2)


def test_branches_data_gradient_reads_column_slices(cuda):
    """the branch gradients as they arrive from a concatenation: column slices of one wide dy"""
    from iseg_amd import kernels as k

    ci = 2
    r = _problem(ci)
    (N, H, W, Cin), Cout, taps = CASES[ci]
    wide = torch.cat([d.reshape(-1, Cout) for d in r["dys"]], dim=1)
    dx = k.conv2d_branches_bwd_data([wide[:, b * Cout:] for b in range(len(taps))], [wide.shape[1]] * len(taps), r["ws"], _table(k, ci))
    close(dx, r["dx"], BF, "branches dx from slices", bf16_tol=1.5e-2)


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_branches_weight_gradient(cuda, ci):
    from iseg_amd import kernels as k

    r = _problem(ci)
    (N, H, W, Cin), Cout, taps = CASES[ci]
    dy2, ld = [d.reshape(-1, Cout) for d in r["dys"]], [Cout] * len(taps)
    gws = [torch.full((kk, kk, Cin, Cout), 0.5, device="cuda") for kk, _ in taps]      # accumulate onto a non-zero buffer
    k.conv2d_branches_bwd_weight(r["x"], dy2, ld, gws, _table(k, ci), accumulate=True)
    for b, gw in enumerate(gws):
        close(gw - 0.5, r["gws"][b], torch.float32, f"branches dW, branch {b}", f32_tol=2e-4)
    gws = [torch.full((kk, kk, Cin, Cout), float("nan"), device="cuda") for kk, _ in taps]      # overwrite a poisoned one
    k.conv2d_branches_bwd_weight(r["x"], dy2, ld, gws, _table(k, ci), accumulate=False)
    for b, gw in enumerate(gws):
        close(gw, r["gws"][b], torch.float32, f"branches dW (overwrite), branch {b}", f32_tol=2e-4)
        single = torch.zeros_like(gw)
        k.conv2d_igemm_bwd_weight(r["x"], r["dys"][b], single, _geom(k, ci, b), accumulate=False)
        close(gw, single.double().cpu(), torch.float32, f"branches dW vs single, branch {b}", f32_tol=2e-4)


def test_branches_are_deterministic(cuda):
    from iseg_amd import _hip, kernels as k

    ci = 2
    r = _problem(ci)
    (N, H, W, Cin), Cout, taps = CASES[ci]
    dy2, ld = [d.reshape(-1, Cout) for d in r["dys"]], [Cout] * len(taps)
    joined = k.conv_branches_joined_geom(_table(k, ci))
    assert _hip.lib().iseg_conv2d_igemm_workspace_bytes(C.byref(joined), 1) > 0      # (the split data gradient: fixed-order slabs)
    runs = []
    for _ in range(2):
        gws = [torch.zeros((kk, kk, Cin, Cout), device="cuda") for kk, _ in taps]
        k.conv2d_branches_bwd_weight(r["x"], dy2, ld, gws, _table(k, ci), accumulate=False)
        ys = k.conv2d_branches_fwd(r["x"], [_wt(w) for w in r["ws"]], _table(k, ci))
        runs.append(ys + [k.conv2d_branches_bwd_data(dy2, ld, r["ws"], _table(k, ci)).clone()] + gws)
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_branches_refuse_what_they_cannot_do(cuda):
    from iseg_amd import _hip, kernels as k

    L = _hip.lib()
    taps = [(3, 3, 2, 2), (1, 1, 1, 1)]
    assert not k.conv2d_branches_supported(k.conv_branches(2, 8, 8, 72, 64, taps), BF)           # Cin = 72: no 64-channel K-steps
    assert not k.conv2d_branches_supported(k.conv_branches(2, 8, 8, 64, 64, taps), torch.float32)
    assert k.conv2d_branches_supported(k.conv_branches(2, 8, 8, 64, 64, taps), BF)
    x = torch.zeros((2, 8, 8, 72), dtype=BF, device="cuda")
    t = k.conv_branches(2, 8, 8, 72, 64, taps)
    assert L.iseg_conv2d_branches_fwd(x.data_ptr(), C.byref(t), k.dt(BF), None, 0, k.stream()) == -3      # ISEG_ERR_UNSUPPORTED
    t = k.conv_branches(2, 8, 8, 64, 64, taps)
    assert L.iseg_conv2d_branches_fwd(x.data_ptr(), C.byref(t), k.dt(torch.float32), None, 0, k.stream()) == -3
    # more branches than the table holds
    t = k.conv_branches(2, 8, 8, 64, 64, taps * 3)
    assert t.count == 6 and not k.conv2d_branches_supported(t, BF)
    assert L.iseg_conv2d_branches_fwd(x.data_ptr(), C.byref(t), k.dt(BF), None, 0, k.stream()) < 0
    assert L.iseg_conv2d_branches_bwd_weight(x.data_ptr(), C.byref(t), 1, k.dt(BF), None, 0, k.stream()) < 0
    assert L.iseg_conv2d_branches_bwd_data(C.byref(t), x.data_ptr(), None, 0, k.dt(BF), None, 0, k.stream()) < 0
    # null operands
    t = k.conv_branches(2, 8, 8, 64, 64, taps)
    assert L.iseg_conv2d_branches_fwd(x.data_ptr(), C.byref(t), k.dt(BF), None, 0, k.stream()) == -1      # ISEG_ERR_ARG


def test_branches_data_gradient_refuses_a_short_workspace(cuda):
    from iseg_amd import _hip, kernels as k

    ci = 2
    r = _problem(ci)
    (N, H, W, Cin), Cout, taps = CASES[ci]
    t = _table(k, ci)
    need = _hip.lib().iseg_conv2d_igemm_workspace_bytes(C.byref(k.conv_branches_joined_geom(t)), 1)      # the joined product's slabs
    assert need > 0
    for b, (dy, w) in enumerate(zip(r["dys"], r["ws"])):
        t.b[b].dy, t.b[b].lddy, t.b[b].w = dy.data_ptr(), Cout, w.data_ptr()
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    dx = torch.full((N, H, W, Cin), 5.0, dtype=BF, device="cuda")
    st = _hip.lib().iseg_conv2d_branches_bwd_data(C.byref(t), dx.data_ptr(), None, 0, k.dt(BF), ws.data_ptr(), need - 1, k.stream())
    assert st == -4      # ISEG_ERR_WORKSPACE, nothing launched
    torch.cuda.synchronize()
    assert torch.all(dx == 5.0)
    _hip.call("iseg_conv2d_branches_bwd_data", C.byref(t), dx.data_ptr(), None, 0, k.dt(BF), ws.data_ptr(), need, k.stream())
    close(dx, r["dx"], BF, "branches dx on an exact workspace", bf16_tol=1.5e-2)


def test_aspp_layer_grouped_route_matches_per_branch_route(cuda, monkeypatch):
    """AtrousSpatialPyramidPooling forward and every gradient: the pixel-level convolutions as one node against one node per branch"""
    from iseg_amd import functional as F, nn
    from iseg_amd.layers.aspp import AtrousSpatialPyramidPooling
    from iseg_amd.param_store import ParamStore
    from tests.util_models import randomize_parameters

    nn.set_compute_dtype(BF)
    nn.set_device("cuda:0")
    try:
        shape = (2, 8, 8, 64)
        layer = AtrousSpatialPyramidPooling(filters=64, name="aspp")
        with nn.dry_run_scope():
            layer(torch.empty(shape, dtype=BF, device="cuda"), training=True)
        store = ParamStore(list(layer.parameters()))
        layer._iseg_store = store
        randomize_parameters(layer, 5)
        x, _ = q(rnd(shape, 1), BF)
        dy = None
        calls = []
        real = F.conv2d_branches
        monkeypatch.setattr(F, "conv2d_branches", lambda *a: calls.append(1) or real(*a))
        runs = []
        for grouped in (True, False):
            if not grouped:
                monkeypatch.setattr(F, "conv2d_branches_supported", lambda *a: False)
            store.flat_g.zero_()
            xg = x.clone().requires_grad_(True)
            y = layer(xg, training=True)
            if dy is None:
                dy, _ = q(rnd(tuple(y.shape), 2), BF)
            y.backward(dy)
            runs.append([y.detach().clone(), xg.grad.clone()] + [p.grad.detach().clone() for p in layer.parameters() if p.requires_grad])
        assert len(calls) == 1      # the first run took the grouped node, the second did not
        assert tuple(runs[0][0].shape) == (2, 8, 8, 5 * 64)
        for i, (a, b) in enumerate(zip(*runs)):
            close(a, b.double().cpu(), BF, f"ASPP grouped vs per-branch, tensor {i}")
    finally:
        nn.set_compute_dtype(torch.float32)
