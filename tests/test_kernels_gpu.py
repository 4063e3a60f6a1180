"""HIP kernels (through the C ABI) vs the CPU oracle on seeded inputs.  fp32 storage is checked at fp32
tolerances, bf16 storage at bf16 output-rounding tolerances (inputs are rounded to bf16 BEFORE the oracle sees them,
so only accumulation order and the final rounding differ).

What close() does not see: it bounds the LARGEST error by tol x the LARGEST element, and for bf16 storage tol is 1.2e-2 to 3e-2 -- 1.5 to 4
bf16 ulps of the largest output, granted to every element.  A store that truncates instead of rounding to nearest-even, split-K or slab partial
sums kept in bf16, and an intermediate rounded to bf16 in front of an epilogue all stay inside it.  Whether a bf16 output is the fp32-accurate
value rounded ONCE is the business of tests/test_rounding_budget_gpu.py (statistic, cases and fp32 restatements: tests/rounding_budget.py; the
proof that the three defects pass close() and miss the statistic: tests/test_rounding_budget_host.py).  close() also sees only finite inputs: where
a NaN or an infinity inside an operand must come out is the business of tests/test_nonfinite_gpu.py."""
import math

import numpy as np
import pytest
import torch

from oracle import tf_ops as O

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]


def K():
    from iseg_amd import kernels

    return kernels


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g, dtype=torch.float64) * scale)


def q(t, dtype):
    """round to storage dtype, return (device tensor, float64 CPU copy of the rounded values)"""
    s = t.to(dtype)
    return s.cuda(), s.to(torch.float64)


def close(got, want, dtype, what="", f32_tol=2e-5, bf16_tol=1.2e-2):
    got = got.detach().to("cpu", torch.float64)
    want = want.detach().to(torch.float64)
    tol = f32_tol if dtype == torch.float32 else bf16_tol
    scale = max(want.abs().max().item(), 1e-6)
    err = (got - want).abs().max().item()
    assert err <= tol * scale, f"{what}: max err {err:.3e} > {tol:.1e} * scale {scale:.3e}"


# --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,Kd", [(256, 128, 96), (1000, 384, 96), (130, 96, 384), (77, 21, 256), (512, 192, 48), (300, 64, 1280),
                                   (64, 1536, 384), (33, 40, 24)])
def test_gemm_forward_orientation(cuda, dtype, M, N, Kd):
    k = K()
    x, xr = q(rnd((M, Kd), 1), dtype)
    w, wr = q(rnd((Kd, N), 2, Kd ** -0.5), dtype)
    b = rnd((N,), 3).float()
    y = k.dense_fwd(x, w, b.cuda())
    close(y, xr @ wr + b.double(), dtype, "dense_fwd")


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_epilogues(cuda, dtype):
    k = K()
    M, N, Kd, G = 384, 96, 384, 128
    x, xr = q(rnd((M, Kd), 1), dtype)
    w, wr = q(rnd((Kd, N), 2, Kd ** -0.5), dtype)
    res, resr = q(rnd((M, N), 4), dtype)
    b = rnd((N,), 3).float()
    cs = (rnd((N,), 5) * 0.5 + 1).float()
    rs = torch.tensor([0.0, 1.25, 1.25])
    y = k.dense_fwd(x, w, b.cuda(), colscale=cs.cuda(), rowscale=rs.cuda(), rows_per_group=G, residual=res)
    want = resr + (xr @ wr + b.double()) * cs.double() * rs.double().repeat_interleave(G).unsqueeze(1)
    close(y, want, dtype, "scale+residual")
    # gelu with saved pre-activation
    pre = torch.empty((M, N), dtype=dtype, device="cuda")
    y = k.dense_fwd(x, w, b.cuda(), act=k.ACT_GELU, pre_out=pre)
    h = xr @ wr + b.double()
    close(pre, h, dtype, "pre_out")
    close(y, O.gelu(h), dtype, "gelu")
    y = k.dense_fwd(x, w, None, act=k.ACT_RELU)
    close(y, torch.relu(xr @ wr), dtype, "relu")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,Kd", [(512, 384, 96), (200, 96, 384), (70, 21, 256), (128, 256, 1280)])
def test_gemm_dgrad_and_gelu_grad(cuda, dtype, M, N, Kd):
    k = K()
    dy, dyr = q(rnd((M, N), 1), dtype)
    w, wr = q(rnd((Kd, N), 2, N ** -0.5), dtype)
    dx = k.dense_dgrad(dy, w)
    close(dx, dyr @ wr.T, dtype, "dgrad")
    h, hr = q(rnd((M, Kd), 3), dtype)
    dx = k.dense_dgrad(dy, w, act=k.ACT_GELU_GRAD, aux=h)
    hh = hr.clone().requires_grad_(True)
    O.gelu(hh).backward(dyr @ wr.T)
    close(dx, hh.grad, dtype, "dgrad*gelu'")
    dx = k.dense_dgrad(dy, w, act=k.ACT_RELU_GRAD, aux=h)
    close(dx, (dyr @ wr.T) * (hr > 0), dtype, "dgrad*relu'")
    # forward epilogue that saves gelu'(pre) (pre_deriv) + the one-multiply backward epilogue (ACT_MUL_AUX)
    x, xr = q(rnd((M, N), 5), dtype)
    w1, w1r = q(rnd((N, Kd), 6, N ** -0.5), dtype)
    b1 = (rnd((Kd,), 7) * 0.2).float()
    d = torch.empty((M, Kd), dtype=dtype, device="cuda")
    y = k.dense_fwd(x, w1, b1.cuda(), act=k.ACT_GELU, pre_out=d, pre_deriv=True)
    pre = (xr @ w1r + b1.double()).requires_grad_(True)
    yo = O.gelu(pre)
    yo.backward(torch.ones_like(yo))
    close(y, yo, dtype, "gelu fwd with saved derivative")
    close(d, pre.grad, dtype, "saved gelu'")
    dx = k.dense_dgrad(dy, w, act=k.ACT_MUL_AUX, aux=d)
    close(dx, (dyr @ wr.T) * d.detach().cpu().double(), dtype, "dgrad * saved gelu'")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,Kd,split", [(4096, 384, 96, 0), (5000, 96, 384, 0), (1030, 21, 256, 3), (640, 768, 3072, 0),
                                         (9000, 256, 200, 0)])
def test_gemm_wgrad_splitk(cuda, dtype, M, N, Kd, split):
    k = K()
    x, xr = q(rnd((M, Kd), 1), dtype)
    dy, dyr = q(rnd((M, N), 2), dtype)
    out = torch.full((Kd, N), 0.5, dtype=torch.float32, device="cuda")
    k.gemm(x, dy, out, Kd, N, M, lda=x.stride(0), ldb=dy.stride(0), ldd=N, a_kcontig=0, b_kcontig=0, accumulate=True, split_k=split)
    want = xr.T @ dyr + 0.5
    close(out, want, torch.float32 if dtype == torch.float32 else dtype, "wgrad", f32_tol=5e-5, bf16_tol=2e-4)


@pytest.mark.parametrize("rows,C,N,form", [(16384, 1536, 384, 7), (16384, 384, 1536, 8), (4096, 3072, 768, 7), (4096, 768, 3072, 7),
                                           (2048, 136, 200, 7), (6144, 392, 128, 7), (2176, 128, 520, 8),
                                           (17424, 384, 1536, 8), (8200, 768, 2304, 7), (2049, 128, 128, 7),       # ragged reductions: rows % 64 != 0
                                           (4096, 96, 384, 8), (4096, 384, 96, 7), (8192, 112, 336, 8), (4096, 96, 288, 0)])     # a side below 128 (clamped columns); too small: register kernel
@pytest.mark.parametrize("bias", [False, True])
def test_wgrad_lds_dma_pipeline(cuda, rows, C, N, form, bias):
    """weight gradients in the ConvNeXt stage-2 / stage-3 shapes (and ragged ones: M, N not multiples of the tile) take the LDS-DMA kernel of
    csrc/gemm_dma_tn.h (256 x 128 / 128 x 256 tiles, split over the reduction, ones-row by one more MFMA per fragment): dW and db against the oracle,
    the slab form (dense_wgrad_slabs) against the summed form, and two runs bit-identical (use_deterministic, core_env.py:39-48)"""
    import ctypes as Ct

    from iseg_amd import _hip

    k = K()
    x, xr = q(rnd((rows, C), 11), torch.bfloat16)
    dy, dyr = q(rnd((rows, N), 12), torch.bfloat16)
    g = _hip.GemmArgs()
    g.A, g.lda, g.a_kcontig = x.data_ptr(), x.stride(0), 0
    g.B, g.ldb, g.b_kcontig = dy.data_ptr(), dy.stride(0), 0
    g.M, g.N, g.K, g.in_dtype, g.out_dtype, g.batch, g.batch_inner = C, N, rows, 1, 0, 1, 1
    dummy = torch.zeros(1, device="cuda")
    g.D, g.ldd = dummy.data_ptr(), N
    if bias:
        g.colsum_out = dummy.data_ptr()
    assert int(_hip.lib().iseg_gemm_variant(Ct.byref(g))) == form, "the problem did not plan onto the LDS-DMA weight-gradient kernel"
    dW = torch.full((C, N), 0.25, device="cuda")
    db = torch.full((N,), -1.0, device="cuda")
    if bias:
        k.gemm(x, dy, dW, C, N, rows, lda=x.stride(0), ldb=dy.stride(0), ldd=N, a_kcontig=0, b_kcontig=0, accumulate=True, colsum_out=db,
               colsum_accumulate=True)
    else:
        k.gemm(x, dy, dW, C, N, rows, lda=x.stride(0), ldb=dy.stride(0), ldd=N, a_kcontig=0, b_kcontig=0, accumulate=True)
    want = xr.T @ dyr
    close(dW, want + 0.25, torch.float32, "dW", f32_tol=2e-5)
    if bias:
        close(db, dyr.sum(0) - 1.0, torch.float32, "db", f32_tol=2e-5)
    dW2 = torch.full((C, N), 0.25, device="cuda")
    db2 = torch.full((N,), -1.0, device="cuda")
    k.gemm(x, dy, dW2, C, N, rows, lda=x.stride(0), ldb=dy.stride(0), ldd=N, a_kcontig=0, b_kcontig=0, accumulate=True,
           colsum_out=db2 if bias else None, colsum_accumulate=True)
    assert torch.equal(dW, dW2) and (not bias or torch.equal(db, db2)), "two runs of the split weight gradient differ"
    if bias and N % 4 == 0 and k.wgrad_can_fuse_bias(x):
        got = k.dense_wgrad_slabs(x, dy)
        assert got is not None
        slabs, n = got
        total = slabs.view(-1, C + 1, N)[:n].double().sum(0).cpu()
        close(total[:C], want, torch.float32, "slab sum", f32_tol=2e-5)
        close(total[C], dyr.sum(0), torch.float32, "ones-row of the slabs", f32_tol=2e-5)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,C", [(520, 96), (300, 192), (130, 384)])
def test_gemm_a_operand_gelu_transform(cuda, dtype, M, C):
    """pwconv2(gelu(h)) and Z = gelu(h)^T dout with GELU applied while the A operand is staged (no gelu tensor in HBM)"""
    k = K()
    h, hr = q(rnd((M, 4 * C), 1), dtype)
    w2, w2r = q(rnd((4 * C, C), 2, (4 * C) ** -0.5), dtype)
    b2 = rnd((C,), 3).float()
    y = k.dense_fwd(h, w2, b2.cuda(), a_act=k.ACT_GELU)
    close(y, O.gelu(hr) @ w2r + b2.double(), dtype, "fwd gelu(A)", bf16_tol=2e-2)
    dy, dyr = q(rnd((M, C), 4), dtype)
    Z = torch.zeros((4 * C, C), device="cuda")
    k.dense_wgrad(h, dy, Z, accumulate=False, a_act=k.ACT_GELU)
    close(Z, O.gelu(hr).T @ dyr, torch.float32, "wgrad gelu(A)", f32_tol=5e-5 if dtype == torch.float32 else 1e-2)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,C,N", [(5000, 96, 384), (700, 192, 768), (300, 384, 1536), (64, 96, 21)])
def test_wgrad_with_fused_bias_gradient(cuda, dtype, M, C, N):
    """db = colsum(dY) rides the weight-gradient GEMM through a virtual ones-row of X^T when C % 128 != 0 (else: colsum)"""
    k = K()
    x, xr = q(rnd((M, C), 1), dtype)
    dy, dyr = q(rnd((M, N), 2), dtype)
    dW = torch.full((C, N), 0.25, device="cuda")
    db = torch.full((N,), -1.0, device="cuda")
    k.dense_wgrad(x, dy, dW, bias_grad=db)
    close(dW, xr.T @ dyr + 0.25, torch.float32, "dW", f32_tol=5e-5 if dtype == torch.float32 else 2e-4)
    close(db, dyr.sum(0) - 1.0, torch.float32, "db", f32_tol=5e-5 if dtype == torch.float32 else 2e-4)
    k.dense_wgrad(x, dy, dW, bias_grad=db, accumulate=False)
    close(dW, xr.T @ dyr, torch.float32, "dW overwrite", f32_tol=5e-5 if dtype == torch.float32 else 2e-4)
    close(db, dyr.sum(0), torch.float32, "db overwrite", f32_tol=5e-5 if dtype == torch.float32 else 2e-4)


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_strided_output_into_concat(cuda, dtype):
    k = K()
    M, N, Kd = 256, 256, 768
    x, xr = q(rnd((M, Kd), 1), dtype)
    w, wr = q(rnd((Kd, N), 2, Kd ** -0.5), dtype)
    cat = torch.zeros((M, 1280), dtype=dtype, device="cuda")
    k.dense_fwd(x, w, None, out=cat[:, 512:768], ldd=1280)
    close(cat[:, 512:768], xr @ wr, dtype, "slice")
    assert cat[:, :512].abs().max().item() == 0 and cat[:, 768:].abs().max().item() == 0


# --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,C", [(1003, 96), (517, 192), (300, 384), (129, 768), (65, 1536), (40, 3072), (7, 8), (1, 96),
                                    (203, 2730), (1000, 262), (77, 263), (9, 5)])      # widths that are not multiples of 8: the one-wavefront-per-row kernels
def test_layernorm_fwd_bwd(cuda, dtype, rows, C):
    k = K()
    x, xr = q(rnd((rows, C), 1) * 2 + 0.3, dtype)
    g = (rnd((C,), 2) * 0.3 + 1).float()
    b = (rnd((C,), 3) * 0.2).float()
    y, mean, rstd = k.layernorm_fwd(x, g.cuda(), b.cuda(), 1e-6)
    xx = xr.clone().requires_grad_(True)
    gg, bb = g.double().requires_grad_(True), b.double().requires_grad_(True)
    yo = O.layer_norm(xx, gg, bb, 1e-6)
    close(y, yo, dtype, "ln fwd")
    close(mean, xr.mean(-1), torch.float32, "ln mean", f32_tol=1e-5)
    dy, dyr = q(rnd((rows, C), 4), dtype)
    add, addr = q(rnd((rows, C), 5), dtype)
    yo.backward(dyr)
    dgam = torch.zeros(C, device="cuda")
    dbet = torch.zeros(C, device="cuda")
    dx = k.layernorm_bwd(dy, x, g.cuda(), mean, rstd, dgam, dbet, dx_add=add)
    close(dx, xx.grad + addr, dtype, "ln dx", f32_tol=1e-4, bf16_tol=2e-2)
    close(dgam, gg.grad, torch.float32, "ln dgamma", f32_tol=2e-4 if dtype == torch.float32 else 2e-2)
    close(dbet, bb.grad, torch.float32, "ln dbeta", f32_tol=2e-4)


# --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,C,groups", [(1003, 96, 1), (4 * 130, 112, 4), (300, 384, 3), (64, 768, 2), (7, 8, 1)])
@pytest.mark.parametrize("use_cs,use_rs,use_res", [(True, True, True), (False, False, False), (True, False, True)])
def test_layernorm_post_norm_tail(cuda, dtype, rows, C, groups, use_cs, use_rs, use_res):
    """iseg_layernorm_post_fwd / _bwd: residual + rowscale[group] * colscale * LN(x) (backbones/intern_image/intern_image.py:226-236 with
    utils/drops.py:8-22) against fp64 autograd -- the three parameter gradients come from the same two column sums"""
    k = K()
    x, xr = q(rnd((rows, C), 1) * 2 + 0.3, dtype)
    g = (rnd((C,), 2) * 0.3 + 1).float()
    b = (rnd((C,), 3) * 0.2).float()
    cs = (rnd((C,), 6) * 0.4 + 1).float()
    rs = torch.tensor([0.0, 1.25, 1.25, 2.5][:groups] if groups > 1 else [1.25], dtype=torch.float32)
    res, resr = q(rnd((rows, C), 7), dtype)
    rpg = rows // groups
    y, mean, rstd = k.layernorm_post_fwd(x, g.cuda(), b.cuda(), 1e-6, colscale=cs.cuda() if use_cs else None, rowscale=rs.cuda() if use_rs else None,
                                         rows_per_group=rpg if use_rs else 0, residual=res if use_res else None)
    xx = xr.clone().requires_grad_(True)
    gg, bb, cc = g.double().requires_grad_(True), b.double().requires_grad_(True), cs.double().requires_grad_(True)
    yo = O.layer_norm(xx, gg, bb, 1e-6)
    if use_cs:
        yo = yo * cc
    if use_rs:
        yo = yo * rs.double()[torch.arange(rows) // rpg][:, None]
    if use_res:
        yo = yo + resr
    close(y, yo, dtype, "ln post fwd")
    dy, dyr = q(rnd((rows, C), 4), dtype)
    yo.backward(dyr)
    dgam, dbet, dcs = torch.full((C,), 0.5, device="cuda"), torch.full((C,), -0.25, device="cuda"), torch.full((C,), 2.0, device="cuda")
    dx = k.layernorm_post_bwd(dy, x, g.cuda(), b.cuda(), mean, rstd, dgam, dbet, colscale=cs.cuda() if use_cs else None,
                              dcolscale=dcs if use_cs else None, rowscale=rs.cuda() if use_rs else None, rows_per_group=rpg if use_rs else 0)
    tol = 2e-4 if dtype == torch.float32 else 2e-2
    close(dx, xx.grad, dtype, "ln post dx", f32_tol=1e-4, bf16_tol=2e-2)
    close(dgam - 0.5, gg.grad, torch.float32, "ln post dgamma (accumulated)", f32_tol=tol)
    close(dbet + 0.25, bb.grad, torch.float32, "ln post dbeta (accumulated)", f32_tol=tol)
    if use_cs:
        close(dcs - 2.0, cc.grad, torch.float32, "ln post dcolscale (accumulated)", f32_tol=tol)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,C,pad_every", [(900, 96, 7), (257, 192, 3), (64, 32, 0)])
def test_layernorm_with_row_tables_and_gather_fma(cuda, dtype, rows, C, pad_every):
    """iseg_layernorm_gather_fwd / _bwd and iseg_gather_rows_fma: norm1 + pad / roll / window partition, window reverse + drop path + skip
    (backbones/swin.py:246-279) with arbitrary permutation tables: padding rows (-1) are zero, the inverse table routes the gradient back"""
    k = K()
    gen = torch.Generator().manual_seed(11)
    perm = torch.randperm(rows, generator=gen)
    fwd = []                                  # output row -> source row, with padding rows sprinkled in
    for i, src in enumerate(perm.tolist()):
        if pad_every and i % pad_every == 0:
            fwd.append(-1)
        fwd.append(src)
    fwd = torch.tensor(fwd, dtype=torch.int32)
    inv = torch.empty(rows, dtype=torch.int32)
    inv[fwd[fwd >= 0].long()] = torch.nonzero(fwd >= 0).flatten().int()
    x, xr = q(rnd((rows, C), 1) * 2 + 0.3, dtype)
    g = (rnd((C,), 2) * 0.3 + 1).float()
    b = (rnd((C,), 3) * 0.2).float()
    y, mean, rstd = k.layernorm_gather_fwd(x, fwd.cuda(), g.cuda(), b.cuda(), 1e-5)
    xx = xr.clone().requires_grad_(True)
    gg, bb = g.double().requires_grad_(True), b.double().requires_grad_(True)
    ln = O.layer_norm(xx, gg, bb, 1e-5)
    yo = torch.where((fwd >= 0)[:, None], ln[fwd.clamp(min=0).long()], torch.zeros((), dtype=torch.float64))
    close(y, yo, dtype, "ln gather fwd")
    assert (y[(fwd < 0).cuda()] == 0).all()
    dy, dyr = q(rnd(tuple(yo.shape), 4), dtype)
    add, addr = q(rnd((rows, C), 5), dtype)
    yo.backward(dyr)
    dgam, dbet = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    dx = k.layernorm_gather_bwd(dy, inv.cuda(), x, g.cuda(), mean, rstd, dgam, dbet, dx_add=add)
    close(dx, xx.grad + addr, dtype, "ln gather dx", f32_tol=1e-4, bf16_tol=2e-2)
    close(dgam, gg.grad, torch.float32, "ln gather dgamma", f32_tol=2e-4 if dtype == torch.float32 else 2e-2)
    close(dbet, bb.grad, torch.float32, "ln gather dbeta", f32_tol=2e-4)
    # window reverse + drop path + skip: out[m] = res[m] + f[m // rpg] * w[inv[m]]; gradient to the window rows by the forward table, factor of the source row
    groups = 3 if rows % 3 == 0 else 1
    rpg = rows // groups
    f = torch.tensor([1.25, 0.0, 2.0][:groups], dtype=torch.float32)
    w, wr = q(rnd(tuple(yo.shape), 8), dtype)
    res, resr = q(rnd((rows, C), 9), dtype)
    out = k.gather_rows_fma(w, inv.cuda(), f.cuda(), rpg, False, res)
    fo = f.double()[torch.arange(rows) // rpg][:, None]
    close(out, resr + fo * wr[inv.long()], dtype, "gather fma fwd")
    d, dr = q(rnd((rows, C), 10), dtype)
    dw = k.gather_rows_fma(d, fwd.cuda(), f.cuda(), rpg, True, None)
    want = torch.where((fwd >= 0)[:, None], (fo * dr)[fwd.clamp(min=0).long()], torch.zeros((), dtype=torch.float64))
    close(dw, want, dtype, "gather fma bwd")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,Hc,Wc", [((2, 16, 16, 64), 8, 8), ((1, 24, 32, 96), 12, 16), ((2, 10, 14, 32), 4, 5), ((1, 9, 9, 8), 9, 9)])
def test_bn_relu_upsample_add_and_remask_backward(cuda, dtype, shape, Hc, Wc):
    """iseg_bn_relu_upsample_add + iseg_bn_bwd_{reduce,apply}_remask + the one-pass x2 bilinear backward: one level of the FPN top-down pathway
    (layers/fpn.py:46-57) against fp64 autograd through batch_norm_train / relu / resize_bilinear"""
    k = K()
    N, H, W, C = shape
    rows = N * H * W
    z, zr = q(rnd(shape, 1) * 1.5 + 0.2, dtype)
    xc, xcr = q(rnd((N, Hc, Wc, C), 2), dtype)
    g = (rnd((C,), 3) * 0.3 + 1).float()
    b = (rnd((C,), 4) * 0.2).float()
    packed = k.bn_stats(z.reshape(rows, C), C, rows, C)
    mean, rstd = k.bn_finalize(packed, C, 1e-3, 0.9, None, None)
    out = k.bn_relu_upsample_add(z, mean, rstd, g.cuda(), b.cuda(), xc)
    zz, xx = zr.clone().requires_grad_(True), xcr.clone().requires_grad_(True)
    gg, bb = g.double().requires_grad_(True), b.double().requires_grad_(True)
    bn, _, _ = O.batch_norm_train(zz, gg, bb, 1e-3)
    # the device's own pre-activation decides the mask (ties at zero cannot differ between the two sides)
    pre = (z.reshape(rows, C).double().cpu() - mean.cpu().double()) * rstd.cpu().double() * g.double() + b.double()
    mask = (pre.float() > 0).reshape(shape)
    yo = bn * mask + O.resize_bilinear(xx, (H, W))
    close(out, yo, dtype, "bn relu upsample add", f32_tol=1e-4, bf16_tol=2e-2)
    dy, dyr = q(rnd(shape, 5), dtype)
    yo.backward(dyr)
    d2, z2 = dy.reshape(rows, C), z.reshape(rows, C)
    sums = k.bn_bwd_reduce_remask(d2, C, z2, C, mean, rstd, g.cuda(), b.cuda(), rows, C)
    tol = 3e-4 if dtype == torch.float32 else 3e-2
    close(sums[:C], bb.grad, torch.float32, "remask dbeta", f32_tol=tol)
    close(sums[C:], gg.grad, torch.float32, "remask dgamma", f32_tol=tol)
    dz = k.bn_bwd_apply_remask(d2, C, z2, C, mean, rstd, g.cuda(), b.cuda(), sums, 1.0 / rows, torch.empty_like(z2), C, rows, C)
    close(dz.reshape(shape), zz.grad, dtype, "remask dz", f32_tol=3e-4, bf16_tol=3e-2)
    dxc = k.resize_bilinear_bwd(dy, Hc, Wc, dtype)      # exact x2 shapes take the one-pass kernel, the others the two-pass form
    close(dxc, xx.grad, dtype, "resize bwd", f32_tol=1e-4, bf16_tol=2e-2)


# --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,Kk,dil", [((2, 13, 17, 96), 7, 1), ((1, 40, 70, 32), 7, 1), ((1, 16, 16, 768), 7, 2), ((2, 9, 9, 192), 7, 1), ((1, 20, 11, 64), 3, 1),
                                         ((1, 8, 8, 112), 3, 2), ((1, 33, 5, 384), 5, 1), ((3, 64, 64, 64), 7, 1), ((1, 73, 100, 32), 7, 1), ((2, 16, 16, 96), 7, 1),
                                         ((1, 7, 5, 32), 7, 1), ((5, 32, 32, 160), 7, 1)])
def test_dwconv_fwd_bwd(cuda, dtype, shape, Kk, dil):
    k = K()
    N, H, W, C = shape
    x, xr = q(rnd(shape, 1), dtype)
    w = (rnd((Kk, Kk, C, 1), 2) / Kk).float()
    b = (rnd((C,), 3) * 0.1).float()
    pad = (Kk - 1) * dil // 2
    y = k.dwconv2d(x, w.reshape(Kk * Kk, C).cuda(), b.cuda(), Kk, dil, pad, pad)
    xx = xr.clone().requires_grad_(True)
    ww, bb = w.double().requires_grad_(True), b.double().requires_grad_(True)
    yo = O.depthwise_conv2d(xx, ww, bb, 1, dil)
    close(y, yo, dtype, "dw fwd")
    dy, dyr = q(rnd(shape, 4), dtype)
    res, resr = q(rnd(shape, 5), dtype)
    yo.backward(dyr)
    padb = (Kk - 1) * dil - pad
    dx = k.dwconv2d(dy, w.reshape(Kk * Kk, C).cuda(), None, Kk, dil, padb, padb, flip=True, add=res)
    close(dx, xx.grad + resr, dtype, "dw dx")
    dw = torch.zeros((Kk * Kk, C), device="cuda")
    db = torch.zeros(C, device="cuda")
    k.dwconv2d_bwd_weight(x, dy, dw, db, Kk, dil, pad, pad)
    close(dw, ww.grad.reshape(Kk * Kk, C), torch.float32, "dw dW", f32_tol=1e-4)
    close(db, bb.grad, torch.float32, "dw db", f32_tol=1e-4)


# --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,C,relu", [(4096, 256, True), (16, 256, True), (1000, 48, False), (333, 2048, True), (20000, 64, True), (1024, 2048, False)])
def test_batchnorm_train(cuda, dtype, rows, C, relu):
    k = K()
    x, xr = q(rnd((rows, C), 1) * 1.5 + 0.2, dtype)
    g = (rnd((C,), 2) * 0.3 + 1).float()
    b = (rnd((C,), 3) * 0.2).float()
    mm = rnd((C,), 6).float().cuda()
    mv = (rnd((C,), 7).abs() + 0.5).float().cuda()
    mm0, mv0 = mm.cpu().double(), mv.cpu().double()
    packed = k.bn_stats(x, C, rows, C)
    close(packed[:C], xr.sum(0), torch.float32, "sum", f32_tol=1e-4)
    close(packed[C:2 * C], (xr * xr).sum(0), torch.float32, "sumsq", f32_tol=1e-4)
    assert packed[2 * C].item() == rows
    mean, rstd = k.bn_finalize(packed, C, 1e-3, 0.9, mm, mv)
    xx = xr.clone().requires_grad_(True)
    gg, bb = g.double().requires_grad_(True), b.double().requires_grad_(True)
    yo, mo, vo = O.batch_norm_train(xx, gg, bb, 1e-3)
    if relu:
        yo = torch.relu(yo)
    close(mm, O.moving_update(mm0, mo.detach(), 0.9), torch.float32, "moving mean", f32_tol=1e-4)
    close(mv, O.moving_update(mv0, vo.detach(), 0.9), torch.float32, "moving var", f32_tol=1e-3)
    y = torch.empty_like(x)
    k.bn_apply_fwd(x, C, mean, rstd, g.cuda(), b.cuda(), y, C, rows, C, relu)
    close(y, yo, dtype, "bn fwd", f32_tol=1e-4)
    dy, dyr = q(rnd((rows, C), 4), dtype)
    # use the device's own y for the relu mask so that mask ties cannot differ
    ymask = (y.cpu().double() > 0) if relu else torch.ones_like(dyr, dtype=torch.bool)
    yo2, _, _ = O.batch_norm_train(xx, gg, bb, 1e-3)
    yo2.backward(dyr * ymask)
    sums = k.bn_bwd_reduce(dy, C, x, C, y, C, mean, rstd, rows, C, relu)
    close(sums[:C], bb.grad, torch.float32, "dbeta", f32_tol=3e-4 if dtype == torch.float32 else 3e-2)
    close(sums[C:], gg.grad, torch.float32, "dgamma", f32_tol=3e-4 if dtype == torch.float32 else 3e-2)
    dx = torch.empty_like(x)
    k.bn_bwd_apply(dy, C, x, C, y, C, mean, rstd, g.cuda(), sums, 1.0 / rows, dx, C, rows, C, relu)
    close(dx, xx.grad, dtype, "bn dx", f32_tol=3e-4, bf16_tol=3e-2)


# --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,kh,s,d,Cout", [((2, 16, 16, 64), 3, 1, 3, 32), ((1, 32, 32, 3), 4, 4, 1, 96), ((2, 16, 16, 96), 2, 2, 1, 192),
                                              ((1, 15, 17, 16), 3, 2, 1, 24), ((1, 12, 12, 40), 3, 1, 9, 16), ((1, 16, 16, 32), 2, 1, 2, 64),
                                              ((1, 16, 16, 4), 3, 1, 1, 16), ((2, 18, 20, 12), 3, 2, 1, 8), ((1, 20, 24, 4), 5, 1, 1, 8)])
def test_conv_via_im2col_gemm(cuda, dtype, shape, kh, s, d, Cout):
    k = K()
    N, H, W, C = shape
    xin = rnd(shape, 1)
    x, xr = q(xin, dtype)
    w, wr = q(rnd((kh, kh, C, Cout), 2, (kh * kh * C) ** -0.5), dtype)
    Ho, pt = k.same_pad(H, kh, s, d)
    Wo, pl = k.same_pad(W, kh, s, d)
    col = k.im2col(x, kh, kh, s, s, d, d, pt, pl, Ho, Wo, dtype)
    Kd = kh * kh * C
    y = torch.empty((N * Ho * Wo, Cout), dtype=dtype, device="cuda")
    k.gemm(col, w.reshape(Kd, Cout), y, N * Ho * Wo, Cout, Kd, lda=col.stride(0), ldb=Cout, ldd=Cout, a_kcontig=1, b_kcontig=0)
    xx = xr.clone().requires_grad_(True)
    yo = O.conv2d(xx, wr, None, s, d)
    assert tuple(yo.shape) == (N, Ho, Wo, Cout)
    close(y.reshape(N, Ho, Wo, Cout), yo, dtype, "conv fwd")
    dy, dyr = q(rnd((N, Ho, Wo, Cout), 3), dtype)
    yo.backward(dyr)
    dcol = torch.empty_like(col)
    if dcol.shape[1] > Kd:
        dcol.zero_()
    k.gemm(dy.reshape(-1, Cout), w.reshape(Kd, Cout), dcol, N * Ho * Wo, Kd, Cout, lda=Cout, ldb=Cout, ldd=dcol.stride(0), a_kcontig=1,
           b_kcontig=1)
    dx = k.col2im(dcol, N, H, W, C, kh, kh, s, s, d, d, pt, pl, Ho, Wo)
    close(dx, xx.grad, dtype, "conv dx", bf16_tol=2e-2)


@pytest.mark.parametrize("dtype", DTYPES)
def test_im2col_casts_f32_image(cuda, dtype):
    k = K()
    x = rnd((1, 16, 16, 3), 1).float()
    col = k.im2col(x.cuda(), 4, 4, 4, 4, 1, 1, 0, 0, 4, 4, dtype)
    assert col.shape == (16, 48) and col.dtype == dtype
    want = x.reshape(1, 4, 4, 4, 4, 3).permute(0, 1, 3, 2, 4, 5).reshape(16, 48)
    close(col, want.to(dtype).double(), dtype, "patchify")


# --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_colsum_broadcast_axpby_rowscale(cuda, dtype):
    k = K()
    B, R, C = 3, 257, 96
    x, xr = q(rnd((B, R, C), 1), dtype)
    out = torch.zeros((B, C), device="cuda")
    k.colsum(x, C, R * C, B, R, C, out, scale=1.0 / R)
    close(out, xr.mean(1), torch.float32, "gap", f32_tol=1e-4 if dtype == torch.float32 else 1e-3)
    # odd width (21 classes) takes the scalar path
    x2, x2r = q(rnd((1000, 21), 2), dtype)
    o2 = torch.ones(21, device="cuda")
    k.colsum(x2, 21, 0, 1, 1000, 21, o2, accumulate=True)
    close(o2, x2r.sum(0) + 1, torch.float32, "colsum21", f32_tol=1e-4 if dtype == torch.float32 else 1e-3)
    # column slice of a concat buffer
    cat, catr = q(rnd((2, 64, 1280), 3), dtype)
    o3 = torch.zeros((2, 256), device="cuda")
    k.colsum(cat[:, :, 256:512], 1280, 64 * 1280, 2, 64, 256, o3)
    close(o3, catr[:, :, 256:512].sum(1), torch.float32, "slice colsum", f32_tol=1e-4 if dtype == torch.float32 else 1e-3)
    v, vr = q(rnd((B, C), 4), dtype)
    y = torch.zeros((B, R, 2 * C), dtype=dtype, device="cuda")
    k.broadcast_rows(v, y[:, :, C:], 2 * C, R * 2 * C, B, R, C, scale=0.5)
    close(y[:, :, C:], 0.5 * vr.unsqueeze(1).expand(B, R, C), dtype, "broadcast")
    assert y[:, :, :C].abs().max().item() == 0
    a, ar = q(rnd((1001,), 5), dtype)
    b, br = q(rnd((1001,), 6), dtype)
    close(k.axpby(a, b, 2.0, -1.0), 2 * ar - br, dtype, "axpby")
    s = torch.tensor([0.0, 2.0, 1.0])
    xs, xsr = q(rnd((3 * 40, C), 7), dtype)
    close(k.rowscale(xs, s.cuda(), 40), xsr * s.double().repeat_interleave(40).unsqueeze(1), dtype, "rowscale")


@pytest.mark.parametrize("dtype", DTYPES)
def test_dropout_and_drop_path(cuda, dtype):
    k = K()
    x = torch.ones(1 << 18, dtype=dtype, device="cuda")
    y = k.dropout(x, 0.1, 1234)
    yc = y.float().cpu()
    kept = (yc != 0)
    assert abs(kept.float().mean().item() - 0.9) < 5e-3
    assert torch.allclose(yc[kept], torch.full_like(yc[kept], 1 / 0.9), rtol=1e-2)
    y2 = k.dropout(x, 0.1, 1234)
    assert torch.equal(y, y2), "mask must be a pure function of the seed (backward re-derives it)"
    assert not torch.equal(y, k.dropout(x, 0.1, 99))
    s = k.drop_path_mask(4096, 0.75, 7, x.device).cpu()
    assert all(v == 0.0 or abs(v - 1 / 0.75) < 1e-5 for v in s.unique().tolist())
    assert abs((s > 0).float().mean().item() - 0.75) < 0.03


# --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_dtype", DTYPES)
@pytest.mark.parametrize("Hi,Wi,Ho,Wo,C", [(16, 16, 512, 512, 21), (7, 5, 13, 17, 8), (33, 31, 16, 16, 3), (16, 16, 32, 32, 96), (1, 1, 4, 4, 2),
                                          (20, 20, 20, 20, 5)])
def test_resize_bilinear_fwd_bwd(cuda, in_dtype, Hi, Wi, Ho, Wo, C):
    k = K()
    N = 2
    x, xr = q(rnd((N, Hi, Wi, C), 1), in_dtype)
    y = k.resize_bilinear(x, Ho, Wo, out_dtype=torch.float32)
    xx = xr.clone().requires_grad_(True)
    yo = O.resize_bilinear(xx, (Ho, Wo))
    close(y, yo, torch.float32, "resize fwd", f32_tol=1e-5)
    dy = rnd((N, Ho, Wo, C), 2).float()
    yo.backward(dy.double())
    add, addr = q(rnd((N, Hi, Wi, C), 3), in_dtype)
    dx = k.resize_bilinear_bwd(dy.cuda(), Hi, Wi, in_dtype, dx_add=add)
    close(dx, xx.grad + addr, in_dtype, "resize bwd", f32_tol=2e-5)


def test_resize_nearest_labels(cuda):
    k = K()
    lab = torch.randint(0, 21, (2, 16, 12, 1), dtype=torch.int32)
    y = k.resize_nearest_i32(lab.cuda(), 37, 29)
    want = O.resize_nearest(lab, (37, 29))
    assert torch.equal(y.cpu(), want)


# --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,ignore,use_w", [(21, 255, False), (21, 255, True), (150, 255, False), (19, 0, True), (3, 255, False)])
def test_softmax_ce_ignore(cuda, C, ignore, use_w):
    k = K()
    P = 5 * 37 * 41
    z = (rnd((P, C), 1) * 3).float()
    g = torch.Generator().manual_seed(5)
    y = torch.randint(0, C if ignore != 0 else C + 1, (P,), generator=g, dtype=torch.int32)
    y[torch.rand(P, generator=g) < 0.1] = ignore
    cw = (torch.rand(C, generator=g) + 0.5) if use_w else None
    zz = z.double().requires_grad_(True)
    lo = O.softmax_ce_ignore(y, zz, C, ignore, cw)
    scale = 0.37 / P
    (lo.sum() * scale).backward()
    px, sm, dz = k.softmax_ce_ignore(z.cuda(), y.cuda(), ignore, class_w=None if cw is None else cw.cuda(), want_px=True, want_sum=True,
                                     sum_scale=1.0 / P, want_grad=True, grad_scale=scale)
    close(px, lo, torch.float32, "loss px", f32_tol=1e-5)
    assert abs(sm.item() - lo.mean().item()) <= 1e-5 * max(1.0, abs(lo.mean().item()))
    close(dz, zz.grad, torch.float32, "dlogits", f32_tol=1e-5)
    assert (px.cpu()[y == ignore] == 0).all()


@pytest.mark.parametrize("C,ignore,use_w,alpha,gamma", [(21, 255, False, 0.25, 2.0), (21, 255, True, 1.0, 2.0), (19, 0, True, 0.5, 1.5),
                                                        (4, 255, False, 0.25, 0.0)])
def test_softmax_focal_ce_ignore(cuda, C, ignore, use_w, alpha, gamma):
    """use_focal_loss branch (keras CategoricalFocalCrossentropy from logits): loss, its mean and d(loss)/d(logits)"""
    k = K()
    P = 3 * 29 * 31
    z = (rnd((P, C), 11) * 3).float()
    g = torch.Generator().manual_seed(6)
    y = torch.randint(0, C if ignore != 0 else C + 1, (P,), generator=g, dtype=torch.int32)
    y[torch.rand(P, generator=g) < 0.1] = ignore
    cw = (torch.rand(C, generator=g) + 0.5) if use_w else None
    zz = z.double().requires_grad_(True)
    lo = O.softmax_focal_ce_ignore(y, zz, C, ignore, cw, alpha, gamma)
    scale = 0.41 / P
    (lo.sum() * scale).backward()
    px, sm, dz = k.softmax_ce_ignore(z.cuda(), y.cuda(), ignore, class_w=None if cw is None else cw.cuda(), want_px=True, want_sum=True,
                                     sum_scale=1.0 / P, want_grad=True, grad_scale=scale, focal=(alpha, gamma))
    close(px, lo, torch.float32, "focal loss px", f32_tol=2e-5)
    assert abs(sm.item() - lo.mean().item()) <= 2e-5 * max(1.0, abs(lo.mean().item()))
    close(dz, zz.grad, torch.float32, "focal dlogits", f32_tol=5e-5)
    assert (px.cpu()[y == ignore] == 0).all()
    if gamma == 0.0 and not use_w:      # gamma = 0: alpha * plain cross-entropy (away from the clip)
        plain = O.softmax_ce_ignore(y, z.double(), C, ignore, None)
        close(px, alpha * plain, torch.float32, "gamma 0 = scaled CE", f32_tol=2e-5)


def test_argmax_confusion_first_max_and_ignore(cuda):
    k = K()
    C, P = 21, 10007
    z = rnd((P, C), 1).float()
    z[::7, 5] = z[::7].max(-1).values  # ties: class 5 equals the max -> first maximal index wins
    z[::7, 3] = z[::7, 5]
    g = torch.Generator().manual_seed(2)
    y = torch.randint(0, C, (P,), generator=g, dtype=torch.int32)
    y[::11] = 255
    cm = torch.zeros(C * C, dtype=torch.int64, device="cuda")
    pred = k.argmax_confusion(z.cuda(), y.cuda(), 255, cm=cm, want_pred=True)
    want_pred = O.argmax_first(z)
    assert torch.equal(pred.cpu().long(), want_pred)
    want_cm = O.confusion_matrix(y, want_pred, C, 255)
    assert torch.equal(cm.cpu().reshape(C, C).double(), want_cm)
    k.argmax_confusion(z.cuda(), y.cuda(), 255, cm=cm)  # accumulates
    assert torch.equal(cm.cpu().reshape(C, C).double(), 2 * want_cm)


@pytest.mark.parametrize("M,N,Kd,split", [(300, 64, 256, 0),        # 128 x 64 tile, 4-deep ring, ragged M
                                         (1000, 136, 128, 0),      # 128 x 128 thin grid (3-deep ring), ragged M and N % 128 != 0
                                         (7000, 384, 192, 0),      # 128 x 128 again, whole tiles along N
                                         (16384, 512, 128, 0),     # 256 x 128 tile
                                         (25000, 264, 320, 0),     # 256 x 128, ragged both ways
                                         (640, 128, 2048, 4)])     # split-K slabs from the DMA kernel
def test_gemm_dma_pipeline_matches_oracle_and_register_staged_kernel(cuda, M, N, Kd, split):
    """csrc/gemm_dma.h (bf16, A and B K-contiguous, K % 64 == 0): every tile variant, ragged edges, the fused epilogues, fp32
    accumulate output and split-K slabs against the fp64 oracle"""
    k = K()
    dt = torch.bfloat16
    a, ar = q(rnd((M, Kd), 1), dt)
    b, br = q(rnd((N, Kd), 2, Kd ** -0.5), dt)
    bias = rnd((N,), 3).float()
    cs = (rnd((N,), 4) * 0.5 + 1.0).float()
    res, resr = q(rnd((M, N), 5), dt)
    aux, auxr = q(rnd((M, N), 6), dt)
    out = torch.empty((M, N), dtype=dt, device="cuda")
    k.gemm(a, b, out, M, N, Kd, lda=Kd, ldb=Kd, ldd=N, a_kcontig=1, b_kcontig=1, split_k=split)
    close(out, ar @ br.T, dt, "plain")
    k.gemm(a, b, out, M, N, Kd, lda=Kd, ldb=Kd, ldd=N, a_kcontig=1, b_kcontig=1, bias=bias.cuda(), colscale=cs.cuda(), residual=res, ldr=N,
           act=k.ACT_GELU, split_k=split)
    want = O.gelu(ar @ br.T + bias.double()) * cs.double() + resr
    close(out, want, dt, "bias+gelu+colscale+residual")
    k.gemm(a, b, out, M, N, Kd, lda=Kd, ldb=Kd, ldd=N, a_kcontig=1, b_kcontig=1, act=k.ACT_GELU_GRAD, aux=aux, ldaux=N, split_k=split)
    hh = auxr.clone().requires_grad_(True)
    O.gelu(hh).backward(ar @ br.T)
    close(out, hh.grad, dt, "gelu'")
    o32 = torch.full((M, N), 0.25, dtype=torch.float32, device="cuda")
    k.gemm(a, b, o32, M, N, Kd, lda=Kd, ldb=Kd, ldd=N, a_kcontig=1, b_kcontig=1, accumulate=True, alpha=0.5, split_k=split)
    close(o32, 0.5 * (ar @ br.T) + 0.25, torch.float32, "fp32 accumulate", f32_tol=2e-5)


@pytest.mark.parametrize("M,N,Kd,split", [(300, 64, 72, 0),          # 64 + one chunk
                                         (1000, 136, 96, 0),       # Swin-T / ConvNeXt-T stage-0 width
                                         (7000, 384, 112, 0),      # InternImage-B stage-0 width
                                         (131072, 112, 112, 0),    # ... at its real row count (256 x 128 tiles)
                                         (16384, 512, 200, 0),
                                         (25000, 264, 328, 0),
                                         (640, 128, 2040, 4)])     # the tail inside the last split
def test_gemm_dma_pipeline_k_tail(cuda, M, N, Kd, split):
    """csrc/gemm_dma.h with K % 64 != 0 (round 5): the last K-step's missing 16-B chunks are requested from a run of zeros.  The problems plan
    onto the LDS-DMA kernel; results against the fp64 oracle; the operands sit in larger buffers filled with NaN around them, so a chunk read past
    a row's end would show"""
    import ctypes as Ct

    from iseg_amd import _hip

    k = K()
    dt = torch.bfloat16
    _, ar = q(rnd((M, Kd), 1), dt)
    _, br = q(rnd((N, Kd), 2, Kd ** -0.5), dt)
    lda = ldb = Kd + 64      # rows padded with NaN: eight more chunks behind every row
    abuf = torch.full((M, lda), float("nan"), dtype=dt, device="cuda")
    bbuf = torch.full((N, ldb), float("nan"), dtype=dt, device="cuda")
    abuf[:, :Kd] = ar.to(dt).cuda()
    bbuf[:, :Kd] = br.to(dt).cuda()
    g = _hip.GemmArgs()
    g.A, g.lda, g.a_kcontig = abuf.data_ptr(), lda, 1
    g.B, g.ldb, g.b_kcontig = bbuf.data_ptr(), ldb, 1
    g.M, g.N, g.K, g.in_dtype, g.out_dtype, g.batch, g.batch_inner, g.split_k = M, N, Kd, 1, 1, 1, 1, split
    out = torch.empty((M, N), dtype=dt, device="cuda")
    g.D, g.ldd = out.data_ptr(), N
    assert int(_hip.lib().iseg_gemm_variant(Ct.byref(g))) in (1, 2, 4, 6), "the problem did not plan onto the LDS-DMA kernel"
    k.gemm(abuf, bbuf, out, M, N, Kd, lda=lda, ldb=ldb, ldd=N, a_kcontig=1, b_kcontig=1, split_k=split)
    close(out, ar @ br.T, dt, "plain")
    bias = rnd((N,), 3).float()
    aux, auxr = q(rnd((M, N), 6), dt)
    k.gemm(abuf, bbuf, out, M, N, Kd, lda=lda, ldb=ldb, ldd=N, a_kcontig=1, b_kcontig=1, bias=bias.cuda(), act=k.ACT_GELU, split_k=split)
    close(out, O.gelu(ar @ br.T + bias.double()), dt, "bias+gelu")
    k.gemm(abuf, bbuf, out, M, N, Kd, lda=lda, ldb=ldb, ldd=N, a_kcontig=1, b_kcontig=1, act=k.ACT_GELU_GRAD, aux=aux, ldaux=N, split_k=split)
    hh = auxr.clone().requires_grad_(True)
    O.gelu(hh).backward(ar @ br.T)
    close(out, hh.grad, dt, "gelu'")


def test_gemm_dma_pipeline_strided_batch(cuda):
    k = K()
    dt = torch.bfloat16
    Bz, H, T, d = 3, 4, 200, 128
    C = H * d
    qkv, qr = q(rnd((Bz, T, 2 * C), 7), dt)
    P = torch.empty((Bz * H, T, T), dtype=dt, device="cuda")
    ld = 2 * C
    k.gemm(qkv[:, :, :C], qkv[:, :, C:], P, T, T, d, lda=ld, ldb=ld, ldd=T, a_kcontig=1, b_kcontig=1, alpha=0.125, batch=Bz * H,
           batch_inner=H, sa=(T * ld, d), sb=(T * ld, d), sd=(H * T * T, T * T))
    qh = qr[:, :, :C].reshape(Bz, T, H, d).permute(0, 2, 1, 3)
    kh = qr[:, :, C:].reshape(Bz, T, H, d).permute(0, 2, 1, 3)
    close(P.reshape(Bz, H, T, T), 0.125 * (qh @ kh.transpose(-1, -2)), dt, "batched q k^T")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape,k,s,dil", [((2, 16, 16, 32), 3, 2, 1), ((1, 15, 9, 16), 3, 2, 1), ((2, 12, 13, 8), 5, 2, 1), ((1, 17, 17, 24), 3, 3, 1),
                                           ((2, 16, 10, 16), 3, 2, 2), ((2, 30, 28, 40), 3, 2, 1), ((1, 14, 14, 8), 7, 2, 1)])
def test_strided_depthwise_conv_matches_oracle(cuda, dtype, shape, k, s, dil):
    """keras DepthwiseConv2D(strides=s, padding="same") (the separable / inverted-residual families): TF's 'same' positions for even and odd
    sizes, forward and both gradients"""
    from iseg_amd import functional as F
    from iseg_amd import nn

    nn.set_compute_dtype(dtype)
    try:
        g = torch.Generator().manual_seed(sum(shape) + 7 * k + s)
        N, H, W, C = shape
        x = torch.randn(shape, generator=g).to(dtype)
        w = torch.randn(k, k, C, 1, generator=g) / k
        b = torch.randn(C, generator=g) * 0.1
        wp = torch.nn.Parameter(w.clone().cuda())
        bp = torch.nn.Parameter(b.clone().cuda())
        if dtype == torch.bfloat16:
            wp.iseg_compute, bp.iseg_compute = None, None
        xg = x.cuda().requires_grad_(True)
        y = F.depthwise_conv2d(xg, wp, bp, dil, strides=s)
        xr, wr, br = x.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
        yr = O.depthwise_conv2d(xr, wr, br, s, dil, "same")
        assert tuple(y.shape) == tuple(yr.shape)
        dy = torch.randn(yr.shape, generator=g).to(dtype)
        y.backward(dy.cuda())
        yr.backward(dy.double())
        tol = 1e-5 if dtype == torch.float32 else 2e-2

        def rel(a, b_):
            return (a.detach().cpu().double() - b_).abs().max().item() / max(b_.abs().max().item(), 1e-8)

        assert rel(y, yr.detach()) < tol
        assert rel(xg.grad, xr.grad) < tol and rel(wp.grad, wr.grad) < 2 * tol and rel(bp.grad, br.grad) < 2 * tol
        # dedicated kernels (csrc/dwconv_strided.hip): fixed summation order -> a second backward pass reproduces the weight gradient exactly
        first = wp.grad.clone()
        wp.grad.zero_(); bp.grad.zero_()
        F.depthwise_conv2d(xg, wp, bp, dil, strides=s).backward(dy.cuda())
        assert torch.equal(wp.grad, first)
    finally:
        nn.set_compute_dtype(torch.float32)


def test_gelu_approximations_on_a_dense_grid(cuda):
    """The transcendental-free GELU / GELU' of the bf16 kernels (csrc/common.h gelu_poly / gelu_poly_grad, round 5) through the C-ABI
    activation kernels on EVERY bf16 value in [-8, 8], against the exact-erf oracle (keras.activations.gelu, backbones/convnext.py:53):
    approximation error <= 1e-3 / 2e-3 (the round-4 verdict's gate) on top of the bf16 output rounding (2^-8 relative).  fp32 storage
    keeps erff and is checked at 2e-6."""
    k = K()
    bits = torch.arange(0, 1 << 16, dtype=torch.int32)
    allbf = bits.to(torch.int16).view(torch.bfloat16)
    x = allbf[torch.isfinite(allbf.float()) & (allbf.float().abs() <= 8)]
    xd = x.double()
    want = O.gelu(xd)
    xg = xd.clone().requires_grad_(True)
    (dwant,) = torch.autograd.grad(O.gelu(xg).sum(), xg)
    y = k.act_fwd(x.cuda(), k.ACT_GELU).cpu().double()
    assert ((y - want).abs() <= 1e-3 + 2.0 ** -8 * want.abs()).all(), (y - want).abs().max().item()
    ones = torch.ones_like(x)
    d = k.act_bwd(ones.cuda(), x.cuda(), k.ACT_GELU).cpu().double()
    assert ((d - dwant).abs() <= 2e-3 + 2.0 ** -8 * dwant.abs()).all(), (d - dwant).abs().max().item()
    # the tails: gelu(x) -> x, gelu'(x) -> 1 on the right, both -> 0 on the left, for every finite bf16 beyond the grid
    far = allbf[torch.isfinite(allbf.float()) & (allbf.float().abs() > 8) & (allbf.float().abs() < 1e18)]
    yf = k.act_fwd(far.cuda(), k.ACT_GELU).cpu().double()
    fd = far.double()
    assert ((yf - torch.where(fd > 0, fd, torch.zeros_like(fd))).abs() <= 2.0 ** -8 * fd.abs()).all()
    x32 = x.float()
    y32 = k.act_fwd(x32.cuda(), k.ACT_GELU).cpu().double()
    assert (y32 - want).abs().max().item() < 2e-6


@pytest.mark.parametrize("rows,Cc", [(4096, 384), (2112, 768), (16384, 384)])
def test_weight_gradient_pair_launch(cuda, rows, Cc):
    """K.dense_wgrad_pair (csrc/gemm_dma_tn.h gemm_bf16_dma_tn_pair_kernel, round 5): the two weight-gradient products of an un-fused ConvNeXt block
    (backbones/convnext.py:51-54 backward: Z = gelu(h)^T dout with its ones-row S = colsum(dout), dW1 += y2^T dH with db1 += colsum(dH)) as ONE launch
    over both problems' tiles, against fp64 products of the same bf16 operands; accumulating into non-zero gradient buffers; bit-reproducible"""
    k = K()
    bf = torch.bfloat16
    g = rnd((rows, 4 * Cc), 1).to(bf)
    dbr = rnd((rows, Cc), 2).to(bf)
    y2 = rnd((rows, Cc), 3).to(bf)
    dh = rnd((rows, 4 * Cc), 4).to(bf)
    dW1_0, db1_0 = rnd((Cc, 4 * Cc), 5).float(), rnd((4 * Cc,), 6).float()
    outs = []
    for _ in range(2):
        dW1, db1 = dW1_0.clone().cuda(), db1_0.clone().cuda()
        got = k.dense_wgrad_pair(g.cuda(), dbr.cuda(), y2.cuda(), dh.cuda(), dW1, db1)
        if Cc >= 768:      # 72 + 72 tiles: fewer than two splits fit one resident round -- the entry declines and the caller runs the products one by one
            assert got is None
            return
        assert got is not None, "the stage-2 shaped problems must pair"
        slabs, n = got
        Zs = slabs.reshape(n, 4 * Cc + 1, Cc).sum(0)
        outs.append((Zs.clone(), dW1.clone(), db1.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    Zs, dW1, db1 = outs[0]
    Z_ref = g.double().T @ dbr.double()
    scale = Z_ref.abs().max().item()
    assert (Zs[:-1].cpu().double() - Z_ref).abs().max().item() < 1e-4 * scale
    assert (Zs[-1].cpu().double() - dbr.double().sum(0)).abs().max().item() < 1e-4 * dbr.double().sum(0).abs().max().item() + 1e-3
    W_ref = dW1_0.double() + y2.double().T @ dh.double()
    assert (dW1.cpu().double() - W_ref).abs().max().item() < 1e-4 * W_ref.abs().max().item()
    b_ref = db1_0.double() + dh.double().sum(0)
    assert (db1.cpu().double() - b_ref).abs().max().item() < 1e-4 * b_ref.abs().max().item() + 1e-3


@pytest.mark.parametrize("rows,Cc", [(4096, 384), (16384, 384)])
def test_weight_gradient_pair_with_the_slab_sum_in_the_layer_scale_launch(cuda, rows, Cc):
    """round 6: dense_wgrad_pair(defer_second=True) leaves dW1 / db1 in their split-K slabs and layerscale_grads_slabs(extra=...) sums them in the
    launch that consumes Z's slabs -- one launch instead of two, and BIT-identical to the two it replaces (same slab order, same operations) for
    every gradient of the block's MLP: dW1, db1, dW2, dgamma, db2 (backbones/convnext.py:51-63 backward)"""
    k = K()
    bf = torch.bfloat16
    g = rnd((rows, 4 * Cc), 1).to(bf).cuda()
    dbr = rnd((rows, Cc), 2).to(bf).cuda()
    y2 = rnd((rows, Cc), 3).to(bf).cuda()
    dh = rnd((rows, 4 * Cc), 4).to(bf).cuda()
    W2, b2, gamma = rnd((4 * Cc, Cc), 7).float().cuda(), rnd((Cc,), 8).float().cuda(), rnd((Cc,), 9).float().cuda()
    init = [rnd((Cc, 4 * Cc), 5).float(), rnd((4 * Cc,), 6).float(), rnd((4 * Cc, Cc), 10).float(), rnd((Cc,), 11).float(), rnd((Cc,), 12).float()]

    def run(merged):
        dW1, db1, dW2, dgam, db2 = [t.clone().cuda() for t in init]
        sl = k.dense_wgrad_pair(g, dbr, y2, dh, dW1, db1, defer_second=merged)
        assert sl is not None and (len(sl) == 3) == merged
        k.layerscale_grads_slabs(sl[0], sl[1], W2, b2, gamma, dW2, dgam, db2, extra=sl[2] if merged else None)
        k.deferred_flush()
        torch.cuda.synchronize()
        return [dW1, db1, dW2, dgam, db2]

    two, one = run(False), run(True)
    for a, b, name in zip(two, one, ("dW1", "db1", "dW2", "dgamma", "db2")):
        assert torch.equal(a, b), name
    W_ref = init[0].double() + y2.cpu().double().T @ dh.cpu().double()
    assert (one[0].cpu().double() - W_ref).abs().max().item() < 1e-4 * W_ref.abs().max().item()


# --------------------------------------------------------------------------------------------------------
def _dma_stage_depth_outputs(check=False):
    """every LDS-DMA epilogue kind on shapes the 32-deep ring stages take by default (whole K <= 512, K % 32 == 0, K >= 96), ragged M and N included"""
    k = K()
    outs = []
    # the last five: problems whose 256 x 128 (128 x 128) tiles leave CUs idle in their single round and that take 128 x 192 (64 x 192) tiles instead
    for M, N, Kd in ((256, 128, 96), (1000, 384, 128), (4096, 520, 160), (777, 1536, 384), (2048, 256, 512), (300, 136, 352),
                     (16384, 384, 1536), (16300, 384, 64), (10800, 576, 192), (4000, 768, 256), (4096, 768, 3072)):
        g = torch.Generator().manual_seed(M + N + Kd)
        x = (torch.randn(M, Kd, generator=g)).bfloat16().cuda()
        w = (torch.randn(N, Kd, generator=g) * Kd ** -0.5).bfloat16().cuda()
        aux = torch.randn(M, N, generator=g).bfloat16().cuda()
        res = torch.randn(M, N, generator=g).bfloat16().cuda()
        bias = torch.randn(N, generator=g).cuda()
        scale = torch.rand(N, generator=g).cuda()
        rs = torch.rand((M + 63) // 64, generator=g).cuda()
        kw = dict(lda=Kd, ldb=Kd, ldd=N, a_kcontig=1, b_kcontig=1)
        d = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
        k.gemm(x, w, d, M, N, Kd, **kw)
        outs.append(d.clone())
        if check:      # the plain product against fp32 arithmetic on the same bf16 operands
            want = x.float() @ w.float().t()
            err = (d.float() - want).abs().max().item()
            assert err <= 1.2e-2 * want.abs().max().item(), (M, N, Kd, err)
        p = torch.empty_like(d)
        k.gemm(x, w, d, M, N, Kd, bias=bias, act=k.ACT_GELU, pre_out=p, ldp=N, pre_deriv=True, **kw)
        outs += [d.clone(), p.clone()]
        k.gemm(x, w, d, M, N, Kd, act=k.ACT_MUL_AUX, aux=aux, ldaux=N, **kw)
        outs.append(d.clone())
        k.gemm(x, w, d, M, N, Kd, bias=bias, colscale=scale, residual=res, ldr=N, rowscale=rs, rows_per_group=64, **kw)
        outs.append(d.clone())
    return [o.cpu() for o in outs]


def test_gemm_dma_stage_depths_agree_bit_for_bit(cuda, tmp_path):
    """the two-workgroups-per-CU form (32-deep stages) and the 128 x 192 tiles (both round 6) walk K in the same order as the 256 x 128 form on
    64-deep stages: same bits.  The forms are chosen once per process (ISEG_GEMM_DMA_BK32, ISEG_GEMM_DMA_128X192, ISEG_GEMM_DMA_64X192), so the plain run is a child process."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = str(tmp_path / "deep64.pt")
    code = ("import torch, tests.test_kernels_gpu as t; "
            f"torch.save(t._dma_stage_depth_outputs(), {path!r})")
    env = dict(os.environ, ISEG_GEMM_DMA_BK32="0", ISEG_GEMM_DMA_128X192="0", ISEG_GEMM_DMA_64X192="0", PYTHONPATH=root)
    subprocess.run([sys.executable, "-c", code], cwd=root, env=env, check=True, timeout=600)
    deep64 = torch.load(path)
    deep32 = _dma_stage_depth_outputs(check=True)
    assert len(deep32) == len(deep64) == 55
    for i, (a, b) in enumerate(zip(deep32, deep64)):
        assert torch.isfinite(a.float()).all()

        assert torch.equal(a, b), f"output {i}: {(a.float() - b.float()).abs().max().item()}"
