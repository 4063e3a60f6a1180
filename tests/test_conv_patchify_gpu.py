"""Patchify convolutions (kernel == stride) as plain GEMMs over a patch view of the NHWC tensor (csrc/conv_patchify.hip; reference
backbones/convnext.py:72-75): the three passes through the C ABI against the oracle's keras Conv2D restatement in fp64 on the bf16-rounded
operands, with the bands tests/test_conv_igemm_gpu.py uses for the same passes (default bf16 band forward, 1.5e-2 for dx, 2e-4 of the scale
for dW and the bias gradient).  The shapes are the small ones at which the view's addressing can go wrong: fewer rows than a tile (the row
clamp), a Wo that is no power of two (row groups cut tiles; the weight gradient recomputes its base per stage), one K-step per segment, four
segments, a ragged last reduction stage.

The data gradient is the product iseg_gemm runs for the column buffer, stored at the pixels: it is compared bit for bit with gemm + col2im.

Refusals: (2,12,12,16) k2 has kw*C = 32, less than a K-step, so the forward pass is refused (and the weight gradient, far below 2048 pixel
rows); its data gradient only needs kw*C % 8 == 0 and is taken.  Odd H, two groups, fp32 storage and dilation 2 are refused for every pass."""
import functools

import pytest
import torch

from oracle import tf_ops as O
from tests.test_kernels_gpu import close, q, rnd

pytestmark = pytest.mark.gpu
BF = torch.bfloat16

# (N, H, W, Cin), Cout, k (= stride)
FWD_DGRAD = [
    ((2, 16, 16, 96), 192, 2),      # 128 rows: less than one row tile, the clamp path
    ((1, 24, 40, 192), 384, 2),     # Wo = 20: row groups cut tiles
    ((3, 16, 16, 32), 64, 2),       # one K-step per segment
    ((1, 16, 16, 16), 32, 4),       # four segments
]
WGRAD = [
    ((2, 64, 64, 96), 192, 2),
    ((5, 40, 48, 64), 128, 2),      # Wo = 24, 2400 rows: a ragged last stage, the base recomputed per stage
    ((2, 128, 128, 16), 128, 4),
]


def _geom(k, shape, kk, Cout, s=None, d=1, groups=1):
    N, H, W, C = shape
    s = kk if s is None else s
    Ho, pt = k.same_pad(H, kk, s, d)
    Wo, pl = k.same_pad(W, kk, s, d)
    return k.conv_geom(N, H, W, C, Cout, kk, kk, s, s, d, d, pt, pl, Ho, Wo, groups)


@functools.lru_cache(maxsize=None)
def _case(shape, Cout, kk):
    """operands on the device and the oracle's fp64 results, computed once per shape and shared (nobody writes to them)"""
    N, H, W, C = shape
    x, xr = q(rnd(shape, 1), BF)
    w, wr = q(rnd((kk, kk, C, Cout), 2, (kk * kk * C) ** -0.5), BF)
    b = rnd((Cout,), 3).float()
    dy, dyr = q(rnd((N, H // kk, W // kk, Cout), 4), BF)
    xx, ww, bb = xr.clone().requires_grad_(True), wr.clone().requires_grad_(True), b.double().requires_grad_(True)
    yo = O.conv2d(xx, ww, bb, kk, 1)
    yo.backward(dyr)
    return dict(x=x, w=w, b=b.cuda(), dy=dy, y=yo.detach(), dx=xx.grad, dw=ww.grad, db=bb.grad)


def _gemm_col2im(k, dy, w, geom):
    """the data gradient as functional._Conv2dFn composes it without the patch view: dcol = dy @ W^T, then the permutation"""
    M, Kd, Cout = geom.N * geom.Ho * geom.Wo, geom.KH * geom.KW * geom.Cin, geom.Cout
    dcol = torch.empty((M, Kd), dtype=BF, device="cuda")
    k.gemm(dy.reshape(M, Cout), w.reshape(Kd, Cout), dcol, M, Kd, Cout, lda=Cout, ldb=Cout, ldd=Kd, a_kcontig=1, b_kcontig=1)
    return k.col2im(dcol, geom.N, geom.H, geom.W, geom.Cin, geom.KH, geom.KW, geom.sh, geom.sw, 1, 1, 0, 0, geom.Ho, geom.Wo)


@pytest.mark.parametrize("shape,Cout,kk", FWD_DGRAD)
def test_patch_forward_and_data_gradient(cuda, shape, Cout, kk):
    from iseg_amd import kernels as k

    c = _case(shape, Cout, kk)
    geom = _geom(k, shape, kk, Cout)
    assert k.conv2d_patch_supported(geom, BF, k.PATCH_FWD) and k.conv2d_patch_supported(geom, BF, k.PATCH_BWD_DATA)
    wt = c["w"].reshape(-1, Cout).t().contiguous()
    y = k.conv2d_patch_fwd(c["x"], wt, c["b"], geom)
    assert tuple(y.shape) == tuple(c["y"].shape)
    close(y, c["y"], BF, "patch fwd")
    close(k.conv2d_patch_fwd(c["x"], wt, None, geom), c["y"] - c["b"].double().cpu(), BF, "patch fwd (no bias)")
    assert torch.equal(k.conv2d_patch_fwd(c["x"], wt, c["b"], geom), y)
    dx = k.conv2d_patch_bwd_data(c["dy"], c["w"], geom)
    close(dx, c["dx"], BF, "patch dx", bf16_tol=1.5e-2)
    assert torch.equal(k.conv2d_patch_bwd_data(c["dy"], c["w"], geom).view(torch.int16), dx.view(torch.int16))
    assert torch.equal(_gemm_col2im(k, c["dy"], c["w"], geom).view(torch.int16), dx.view(torch.int16)), "not the bits of gemm + col2im"


@pytest.mark.parametrize("shape,Cout,kk", WGRAD)
def test_patch_weight_and_bias_gradient(cuda, shape, Cout, kk):
    from iseg_amd import kernels as k

    c = _case(shape, Cout, kk)
    geom = _geom(k, shape, kk, Cout)
    assert k.conv2d_patch_supported(geom, BF, k.PATCH_BWD_WEIGHT)
    C = shape[3]
    dw = torch.full((kk, kk, C, Cout), 0.5, device="cuda")
    db = torch.full((Cout,), -2.0, device="cuda")
    k.conv2d_patch_bwd_weight(c["x"], c["dy"], dw, geom, accumulate=True, bias_grad=db)
    close(dw - 0.5, c["dw"], torch.float32, "patch dw", f32_tol=2e-4)
    close(db + 2.0, c["db"], torch.float32, "patch db", f32_tol=2e-4)
    dw2, db2 = torch.full_like(dw, 7.0), torch.full_like(db, 7.0)
    k.conv2d_patch_bwd_weight(c["x"], c["dy"], dw2, geom, accumulate=False, bias_grad=db2)
    close(dw2, c["dw"], torch.float32, "patch dw (overwrite)", f32_tol=2e-4)
    close(db2, c["db"], torch.float32, "patch db (overwrite)", f32_tol=2e-4)
    dw3, db3 = torch.full_like(dw, 1.0), torch.full_like(db, 1.0)
    k.conv2d_patch_bwd_weight(c["x"], c["dy"], dw3, geom, accumulate=False, bias_grad=db3)
    assert torch.equal(dw3, dw2) and torch.equal(db3, db2)      # fixed-order slabs: the same bits every time
    dw4 = torch.full_like(dw, 7.0)
    k.conv2d_patch_bwd_weight(c["x"], c["dy"], dw4, geom, accumulate=False)      # without the ones-row
    assert torch.equal(dw4, dw2)


def _layer(nn, dtype, shape, Cout, kk, s, d, groups, seed=5):
    from iseg_amd.layers.base_layers import Conv2D
    from iseg_amd.param_store import ParamStore
    from tests.util_models import randomize_parameters

    layer = Conv2D(Cout, kk, strides=s, padding="same", dilation_rate=d, groups=groups, use_bias=True, name="conv")
    with nn.dry_run_scope():
        layer(torch.empty(shape, dtype=dtype, device="cuda"))
    layer._iseg_store = ParamStore(list(layer.parameters()))
    randomize_parameters(layer, seed)
    return layer


def _old_route(k, nn, x, layer, dy, geom, dtype):
    """the kernel calls functional._Conv2dFn makes for this convolution without the patch view: (y, dx, dW, db)"""
    N, H, W, Cin, Cout, kk, groups = geom.N, geom.H, geom.W, geom.Cin, geom.Cout, geom.KH, geom.groups
    s, d, Ho, Wo, pt, pl = geom.sh, geom.dh, geom.Ho, geom.Wo, geom.pt, geom.pl
    M, cg, og = N * Ho * Wo, Cin // groups, Cout // groups
    Kd = kk * kk * cg
    w, b = nn.w(layer.kernel), layer.bias.data
    dy2 = dy.reshape(M, Cout)
    db = torch.zeros((Cout,), device="cuda")
    k.colsum(dy2, Cout, 0, 1, M, Cout, db, accumulate=True)
    dw = torch.zeros((kk, kk, cg, Cout), device="cuda")
    dx = torch.empty((N, H, W, Cin), dtype=dtype, device="cuda")

    def group_slice(g):
        if groups == 1:
            return x
        out = torch.empty((N, H, W, cg), dtype=dtype, device="cuda")
        k.copy2d(x.reshape(-1, Cin)[:, g * cg:], Cin, out.reshape(-1, cg), cg, N * H * W, cg)
        return out

    def dx_by_col2im(g):
        dcol = torch.empty((M, Kd), dtype=dtype, device="cuda")
        k.gemm(dy2[:, g * og:], w.reshape(Kd, Cout)[:, g * og:], dcol, M, Kd, og, lda=Cout, ldb=Cout, ldd=Kd, a_kcontig=1, b_kcontig=1)
        dxg = k.col2im(dcol, N, H, W, cg, kk, kk, s, s, d, d, pt, pl, Ho, Wo)
        if groups == 1:
            return dxg
        k.copy2d(dxg.reshape(-1, cg), cg, dx.reshape(-1, Cin)[:, g * cg:], Cin, N * H * W, cg)
        return dx

    if dtype == BF:
        y = k.conv2d_igemm_fwd(x, w, b, geom)
        k.conv2d_igemm_bwd_weight(x, dy, dw, geom, accumulate=True)
        if s == 1:
            dx = k.conv2d_igemm_bwd_data(dy, w, geom)
        else:
            for g in range(groups):
                dx = dx_by_col2im(g)
    else:
        y = torch.empty((M, Cout), dtype=dtype, device="cuda")
        for g in range(groups):
            col = k.im2col(group_slice(g), kk, kk, s, s, d, d, pt, pl, Ho, Wo, dtype)
            k.gemm(col, w.reshape(Kd, Cout)[:, g * og:], y[:, g * og:], M, og, Kd, lda=col.stride(0), ldb=Cout, ldd=Cout, a_kcontig=1, b_kcontig=0,
                   bias=b[g * og:(g + 1) * og])
            k.gemm(col, dy2[:, g * og:], dw.reshape(Kd, Cout)[:, g * og:], Kd, og, M, lda=col.stride(0), ldb=Cout, ldd=Cout, a_kcontig=0, b_kcontig=0,
                   accumulate=True)
            dx = dx_by_col2im(g)
        y = y.reshape(N, Ho, Wo, Cout)
    return y, dx, dw, db


# shape, Cout, k, stride, dilation, groups, dtype, passes that must be refused
REFUSED = [
    ((2, 12, 12, 16), 32, 2, 2, 1, 1, BF, (0, 2)),                 # kw*C = 32 is less than a K-step
    ((2, 13, 12, 96), 192, 2, 2, 1, 1, BF, (0, 1, 2)),             # odd H
    ((2, 12, 12, 32), 64, 2, 2, 1, 2, BF, (0, 1, 2)),              # two groups
    ((2, 12, 12, 16), 32, 2, 2, 1, 1, torch.float32, (0, 1, 2)),   # fp32 storage
    ((2, 12, 12, 16), 32, 2, 1, 2, 1, BF, (0, 1, 2)),              # the dilated form build_dilated_convnext produces
]


@pytest.mark.parametrize("shape,Cout,kk,s,d,groups,dtype,refused", REFUSED)
def test_refused_convolutions_keep_their_route(cuda, shape, Cout, kk, s, d, groups, dtype, refused):
    from iseg_amd import kernels as k, nn

    geom = _geom(k, shape, kk, Cout, s, d, groups)
    for p in refused:
        assert not k.conv2d_patch_supported(geom, dtype, p), f"pass {p}"
    nn.set_compute_dtype(dtype)
    nn.set_device("cuda:0")
    try:
        layer = _layer(nn, dtype, shape, Cout, kk, s, d, groups)
        x, _ = q(rnd(shape, 1), dtype)
        xg = x.clone().requires_grad_(True)
        y = layer(xg)
        dy, _ = q(rnd(tuple(y.shape), 2), dtype)
        y.backward(dy)
        yo, dxo, dwo, dbo = _old_route(k, nn, x, layer, dy, geom, dtype)
        assert torch.equal(y.detach(), yo) and torch.equal(xg.grad, dxo)
        assert torch.equal(layer.kernel.grad, dwo) and torch.equal(layer.bias.grad, dbo)
    finally:
        nn.set_compute_dtype(torch.float32)


def test_patch_launchers_refuse_what_the_query_refuses(cuda):
    from iseg_amd import _hip, kernels as k

    geom = _geom(k, (2, 13, 12, 96), 2, 192)
    x = torch.zeros((2, 13, 12, 96), dtype=BF, device="cuda")
    wt = torch.zeros((192, 384), dtype=BF, device="cuda")
    dy = torch.zeros((2, 7, 6, 192), dtype=BF, device="cuda")
    with pytest.raises(_hip.HipCallError):
        k.conv2d_patch_fwd(x, wt, None, geom)
    with pytest.raises(_hip.HipCallError):
        k.conv2d_patch_bwd_data(dy, wt, geom)
    with pytest.raises(_hip.HipCallError):
        k.conv2d_patch_bwd_weight(x, dy, torch.zeros((2, 2, 96, 192), device="cuda"), geom)


def test_weight_gradient_refuses_a_short_workspace(cuda):
    """the launcher enforces what iseg_conv2d_igemm_workspace_bytes(geom, 3) answers: 16 bytes short is status -4 and nothing is launched"""
    import ctypes as C

    from iseg_amd import _hip, kernels as k

    shape, Cout, kk = WGRAD[0]
    c = _case(shape, Cout, kk)
    geom = _geom(k, shape, kk, Cout)
    L = _hip.lib()
    need = L.iseg_conv2d_igemm_workspace_bytes(C.byref(geom), 3)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    dw = torch.full((kk, kk, shape[3], Cout), 3.0, device="cuda")
    db = torch.full((Cout,), 3.0, device="cuda")
    args = (k.ptr(c["x"]), k.ptr(c["dy"]), k.ptr(dw), k.ptr(db), 0, C.byref(geom), k.dt(c["x"]), k.ptr(ws))
    assert L.iseg_conv2d_patch_bwd_weight(*args, need - 16, k.stream()) == -4
    assert "workspace" in _hip.last_error()
    torch.cuda.synchronize()
    assert bool((dw == 3.0).all()) and bool((db == 3.0).all())
    assert L.iseg_conv2d_patch_bwd_weight(*args, need, k.stream()) == 0      # the exact size is enough
    close(dw, c["dw"], torch.float32, "patch dw (exact workspace)", f32_tol=2e-4)


def test_patch_route_through_autograd(cuda):
    """a ConvNeXt downsampling convolution through functional.conv2d: all three passes take the patch view"""
    from iseg_amd import kernels as k, nn

    shape, Cout, kk = (2, 64, 64, 96), 192, 2
    geom = _geom(k, shape, kk, Cout)
    assert all(k.conv2d_patch_supported(geom, BF, p) for p in (0, 1, 2))
    nn.set_compute_dtype(BF)
    nn.set_device("cuda:0")
    try:
        layer = _layer(nn, BF, shape, Cout, kk, kk, 1, 1)
        x, xr = q(rnd(shape, 1), BF)
        xg = x.requires_grad_(True)
        y = layer(xg)
        dy, dyr = q(rnd(tuple(y.shape), 2), BF)
        y.backward(dy)
        wr = layer.kernel.data.to(BF).double().cpu().requires_grad_(True)
        br = layer.bias.data.double().cpu().requires_grad_(True)
        xx = xr.clone().requires_grad_(True)
        yo = O.conv2d(xx, wr, br, kk, 1)
        yo.backward(dyr)
        close(y, yo, BF, "layer fwd")
        close(xg.grad, xx.grad, BF, "layer dx", bf16_tol=1.5e-2)
        close(layer.kernel.grad, wr.grad, torch.float32, "layer dW", f32_tol=2e-4)
        close(layer.bias.grad, br.grad, torch.float32, "layer db", f32_tol=2e-4)
        # and they are the patch-view kernels' results
        assert torch.equal(y.detach(), k.conv2d_patch_fwd(x.detach(), nn.wt(layer.kernel, (kk * kk * shape[3], Cout)), layer.bias.data, geom))
        assert torch.equal(xg.grad, k.conv2d_patch_bwd_data(dy, nn.w(layer.kernel), geom))
    finally:
        nn.set_compute_dtype(torch.float32)
