"""Differentiable operators: explicit forward/backward kernel pairs behind torch.autograd.Function.

torch.autograd only keeps the tape (which Function ran, what it saved); every forward and backward body is a
sequence of libiseg_hip.so calls.  Parameter gradients are written by the kernels straight into `param.grad`
(a view of the flat gradient buffer, see param_store.py) -- the Functions return None for parameters, so autograd
never runs an accumulation kernel of its own for them.
"""
import math
import os

import torch
from torch.autograd import Function

from . import kernels as K
from . import nn
from . import dist


def _grad(p):
    if p.grad is None:
        p.grad = torch.zeros_like(p.data)
    return p.grad


def _param_grad(p, *shape, scratch=False):
    """where a backward body writes the gradient of Parameter p (viewed as `shape` when given): the gradient buffer of a trainable one.  A
    frozen (or absent) one receives no gradient: None -- or, for a launcher that takes no null destination (scratch=True), an fp32 tensor
    that nobody reads"""
    if p is not None and p.requires_grad:
        g = _grad(p)
    elif p is None or not scratch:
        return None
    else:
        g = torch.zeros(p.shape, dtype=torch.float32, device=p.device)
    return g.reshape(shape) if shape else g


def _grad_out(p, *shape):
    """_param_grad for a launcher that takes no null destination"""
    return _param_grad(p, *shape, scratch=True)


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


def _rows2d(t):
    """[..., C] as ([rows, C] view, row stride in elements) WITHOUT a copy when the rows are equally spaced and 16-byte aligned -- the
    gradient of a channel slice of a wider NHWC tensor (ASPP's concatenation) -- else through a contiguous copy"""
    C = t.shape[-1]
    if t.is_contiguous():
        return t.reshape(-1, C), C
    per16 = 16 // t.element_size()
    if t.dim() >= 2 and t.stride(-1) == 1 and all(t.stride(i) == t.stride(i + 1) * t.shape[i + 1] for i in range(t.dim() - 2)):
        ld = t.stride(-2)
        if ld % per16 == 0 and t.storage_offset() % per16 == 0 and C % per16 == 0:
            return t.as_strided((t.numel() // C, C), (ld, 1)), ld
    t = t.contiguous()
    return t.reshape(-1, C), C


def _dry(shape, like, dtype=None):
    return torch.empty(tuple(int(v) for v in shape), dtype=dtype or like.dtype, device=like.device)


def _check_act_dtype(x):
    if x.dtype != nn.compute_dtype():
        raise TypeError(f"activation dtype {x.dtype} != compute dtype {nn.compute_dtype()}; cast the input with F.cast_input")


# ---------------------------------------------------------------------------------------------------------
# input cast (image fp32 -> compute dtype); no gradient
# ---------------------------------------------------------------------------------------------------------
def cast_input(x):
    if x.dtype == nn.compute_dtype():
        return x
    if nn.dry_run():
        return _dry(x.shape, x, nn.compute_dtype())
    return K.cast(_c(x), nn.compute_dtype())


def cast_to(x, dtype):
    if nn.dry_run():
        return _dry(x.shape, x, dtype)
    return _CastFn.apply(x, dtype)


class _CastFn(Function):
    @staticmethod
    def forward(ctx, x, dtype):
        ctx.src_dtype = x.dtype
        return x if x.dtype == dtype else K.cast(_c(x), dtype)

    @staticmethod
    def backward(ctx, dy):
        return (dy if dy.dtype == ctx.src_dtype else K.cast(_c(dy), ctx.src_dtype)), None


# ---------------------------------------------------------------------------------------------------------
# Dense / 1x1 conv:  y = act(x @ W + b)         keras.layers.Dense, Conv2D(1x1)
# ---------------------------------------------------------------------------------------------------------
_DMA_MIN_K = 32      # the other half: dma_min_k in csrc/gemm_dma.h


def _kcontig_kernel(W, x2, Kd, N):
    """the [N][K] copy of a forward product's kernel (nn.wt) when the LDS-DMA GEMM can take the product (csrc/gemm_dma.h dma_eligible: bf16,
    K a multiple of 8 and >= 32, N a multiple of 8 and >= 64, M >= 64), else None: the register-staged kernel reads [K][N] as it lies"""
    if x2.dtype != torch.bfloat16 or Kd % 8 or Kd < _DMA_MIN_K or N % 8 or N < 64 or x2.shape[0] < 64:
        return None
    return nn.wt(W, (Kd, N))


class _DenseFn(Function):
    """rows_out: the kernel is stored [out, in] (the token table read as the logits kernel, F.embedding_logits): y = x @ W^T, no bias, no
    activation; the gradient is written in that layout into the parameter's one buffer"""

    @staticmethod
    def forward(ctx, x, W, b, act, kshape=None, rows_out=False):
        ctx.rows_out = rows_out
        if rows_out:
            N, Kd = W.shape
            x2 = _c(x).reshape(-1, Kd)
            y = K.dense_fwd_t(x2, nn.w(W))      # the kernel as it lies is the K-contiguous [N, K] operand
            ctx.act, ctx.W, ctx.b, ctx.kshape = act, W, None, (Kd, N)
            ctx.save_for_backward(x2, None)
            return y.reshape(*x.shape[:-1], N)
        Kd, N = kshape if kshape is not None else (W.shape[-2], W.shape[-1])
        x2 = _c(x).reshape(-1, Kd)
        bias = b.data.reshape(-1) if b is not None else None
        pre = None
        need_grad = any(ctx.needs_input_grad)     # grad mode is off inside Function.forward; this is the tape's view
        if act == K.ACT_GELU and need_grad:
            pre = torch.empty((x2.shape[0], N), dtype=x2.dtype, device=x2.device)
        Wt = _kcontig_kernel(W, x2, Kd, N)
        if Wt is not None:
            y = K.dense_fwd_t(x2, Wt, bias, act=act, pre_out=pre)
        else:
            y = K.dense_fwd(x2, nn.w(W).reshape(Kd, N), bias, act=act, pre_out=pre)
        ctx.act, ctx.W, ctx.b, ctx.kshape = act, W, b, (Kd, N)
        ctx.save_for_backward(x2, pre if act == K.ACT_GELU else (y if act == K.ACT_RELU else None))
        return y.reshape(*x.shape[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        x2, aux = ctx.saved_tensors
        W, b = ctx.W, ctx.b
        Kd, N = ctx.kshape
        dy2 = _c(dy).reshape(-1, N)
        if ctx.rows_out:
            if W.requires_grad:
                K.dense_wgrad(dy2, x2, _grad(W))      # dW [N, Kd] += dY^T X
            dx = K.dense_fwd(dy2, nn.w(W)).reshape(*dy.shape[:-1], Kd) if ctx.needs_input_grad[0] else None
            dist.grads_ready(W)
            return dx, None, None, None, None, None
        if ctx.act in (K.ACT_GELU, K.ACT_RELU):
            dy2 = K.act_bwd(dy2, aux, ctx.act)
        want_b = b is not None and b.requires_grad
        if W.requires_grad:
            # the bias gradient rides the weight-gradient GEMM (virtual ones-row) whenever the last 128-row tile has a spare row
            K.dense_wgrad(x2, dy2, _grad(W).reshape(Kd, N), bias_grad=(_grad(b).reshape(-1) if want_b else None))
        elif want_b:
            K.colsum(dy2, N, 0, 1, dy2.shape[0], N, _grad(b).reshape(-1), accumulate=True)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = K.dense_dgrad(dy2, nn.w(W).reshape(Kd, N)).reshape(*dy.shape[:-1], Kd)
        dist.grads_ready(W, b)
        return dx, None, None, None, None, None


class _MlpGeluFn(Function):
    """Dense -> exact GELU -> Dense of the transformer MLPs (backbones/swin.py:17-43 Mlp, backbones/vit.py:66-113 MLPBlock,
    backbones/intern_image/mlp_layer.py:48-59) as one tape node: the first GEMM's epilogue writes gelu(h) and gelu'(h), the second
    GEMM's data gradient multiplies by the saved derivative in its epilogue -- no elementwise activation-gradient pass."""

    @staticmethod
    def forward(ctx, x, W1, b1, W2, b2, residual=None, rowscale=None):
        """residual / rowscale: `residual + rowscale[sample] * mlp(x)` -- the block's drop-path factor and skip connection ride the second
        product's epilogue (backbones/swin.py:233-236, backbones/vit.py:128-131) instead of a row-scale and an add kernel"""
        C, Hd = W1.shape[-2], W1.shape[-1]
        N = W2.shape[-1]
        x2 = _c(x).reshape(-1, C)
        res2 = _c(residual).reshape(-1, N) if residual is not None else None
        rpg = x2.shape[0] // rowscale.shape[0] if rowscale is not None else 0
        ctx.rowscale, ctx.rpg = rowscale, rpg
        need_grad = any(ctx.needs_input_grad)
        d = torch.empty((x2.shape[0], Hd), dtype=x2.dtype, device=x2.device) if need_grad else None
        W1t, W2t = _kcontig_kernel(W1, x2, C, Hd), None
        if W1t is not None:
            g = K.dense_fwd_t(x2, W1t, b1.data if b1 is not None else None, act=K.ACT_GELU, pre_out=d, pre_deriv=need_grad)
            W2t = _kcontig_kernel(W2, g, Hd, N)
        else:
            g = K.dense_fwd(x2, nn.w(W1), b1.data if b1 is not None else None, act=K.ACT_GELU, pre_out=d, pre_deriv=need_grad)
        if W2t is not None:
            y = K.dense_fwd_t(g, W2t, b2.data if b2 is not None else None, rowscale=rowscale, rows_per_group=rpg, residual=res2)
        else:
            y = K.dense_fwd(g, nn.w(W2), b2.data if b2 is not None else None, rowscale=rowscale, rows_per_group=rpg, residual=res2)
        ctx.params = (W1, b1, W2, b2)
        ctx.save_for_backward(x2, g if need_grad else None, d)
        return y.reshape(*x.shape[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        x2, g, d = ctx.saved_tensors
        W1, b1, W2, b2 = ctx.params
        N = W2.shape[-1]
        dres = dy if ctx.needs_input_grad[5] else None      # the skip connection passes the gradient through
        dy2 = _c(dy).reshape(-1, N)
        if ctx.rowscale is not None:
            dy2 = K.rowscale(dy2, ctx.rowscale, ctx.rpg)
        if W2.requires_grad:
            K.dense_wgrad(g, dy2, _grad(W2), bias_grad=_param_grad(b2))
        elif b2 is not None and b2.requires_grad:
            K.colsum(dy2, N, 0, 1, dy2.shape[0], N, _grad(b2), accumulate=True)
        dh = K.dense_dgrad(dy2, nn.w(W2), act=K.ACT_MUL_AUX, aux=d)            # (dy W2^T) * gelu'(h)
        if W1.requires_grad:
            K.dense_wgrad(x2, dh, _grad(W1), bias_grad=_param_grad(b1))
        elif b1 is not None and b1.requires_grad:
            K.colsum(dh, dh.shape[1], 0, 1, dh.shape[0], dh.shape[1], _grad(b1), accumulate=True)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = K.dense_dgrad(dh, nn.w(W1)).reshape(*dy.shape[:-1], W1.shape[-2])
        dist.grads_ready(W1, b1, W2, b2)
        return dx, None, None, None, None, dres, None


def mlp_gelu(x, W1, b1, W2, b2, residual=None, drop_path_mask=None):
    """dense(gelu(dense(x, W1, b1)), W2, b2) with no dropout in between; with `residual`: residual + drop_path_mask[sample] * that (the
    per-sample factors of utils/drops.py:8-22, None = no drop path), in the second product's epilogue"""
    _check_act_dtype(x)
    if nn.dry_run():
        return _dry((*x.shape[:-1], W2.shape[-1]), x)
    if residual is None and drop_path_mask is not None:
        raise ValueError("mlp_gelu: drop_path_mask rides the residual epilogue")
    return _MlpGeluFn.apply(x, W1, b1, W2, b2, residual, drop_path_mask)


class _DenseGroupFn(Function):
    """Several Dense layers of ONE input whose outputs are wanted side by side -- keras MultiHeadAttention's query / key / value projections
    (backbones/vit.py:142-147: three kernels [C, heads, d]) feeding the packed attention kernels: every product writes its column block of
    the [M, sum N] result directly (no concat copy), and the backward pass reads the gradient's column blocks in place (strided operands: no
    slice copies) and accumulates the three data gradients in the GEMM epilogue (no adds)."""

    @staticmethod
    def forward(ctx, x, n, *wb):
        Ws, bs = wb[:n], wb[n:2 * n]
        Kd = x.shape[-1]
        x2 = _c(x).reshape(-1, Kd)
        Ns = [W.numel() // Kd for W in Ws]
        out = torch.empty((x2.shape[0], sum(Ns)), dtype=x2.dtype, device=x2.device)
        off = 0
        for W, b, N in zip(Ws, bs, Ns):
            view = out[:, off:off + N]
            bias = b.data.reshape(-1) if b is not None else None
            Wt = _kcontig_kernel(W, x2, Kd, N)
            if Wt is not None:
                K.dense_fwd_t(x2, Wt, bias, out=view)
            else:
                K.dense_fwd(x2, nn.w(W).reshape(Kd, N), bias, out=view)
            off += N
        ctx.Ws, ctx.bs, ctx.Ns, ctx.Kd = Ws, bs, Ns, Kd
        ctx.save_for_backward(x2)
        return out.reshape(*x.shape[:-1], sum(Ns))

    @staticmethod
    def backward(ctx, dy):
        (x2,) = ctx.saved_tensors
        Kd = ctx.Kd
        d2 = _c(dy).reshape(x2.shape[0], sum(ctx.Ns))
        dx, off = None, 0
        for W, b, N in zip(ctx.Ws, ctx.bs, ctx.Ns):
            dv = d2[:, off:off + N]      # a strided view: the GEMMs take the row stride
            want_b = b is not None and b.requires_grad
            if W.requires_grad:
                K.dense_wgrad(x2, dv, _grad(W).reshape(Kd, N), bias_grad=(_grad(b).reshape(-1) if want_b else None))
            elif want_b:
                K.colsum(dv, dv.stride(0), 0, 1, dv.shape[0], N, _grad(b).reshape(-1), accumulate=True)
            if ctx.needs_input_grad[0]:
                Wn = nn.w(W).reshape(Kd, N)
                dx = K.dense_dgrad(dv, Wn) if dx is None else K.dense_dgrad(dv, Wn, out=dx, residual=dx)      # + the earlier blocks, in the epilogue
            off += N
        dist.grads_ready(*ctx.Ws, *[b for b in ctx.bs if b is not None])
        return (dx.reshape(*dy.shape[:-1], Kd) if dx is not None else None, None) + (None,) * (2 * len(ctx.Ws))


def dense_group(x, kernels, biases):
    """[dense(x, W_i, b_i) for i] concatenated along the last axis as one tape node; a kernel of rank > 2 is read as [in, rest] (keras
    MultiHeadAttention: [C, heads, d]); biases: a list of the same length (entries may be None)"""
    _check_act_dtype(x)
    Kd = x.shape[-1]
    if nn.dry_run():
        return _dry((*x.shape[:-1], sum(W.numel() // Kd for W in kernels)), x)
    return _DenseGroupFn.apply(x, len(kernels), *kernels, *biases)


class _LnMlpResidualFn(Function):
    """x + drop_path(Dense(gelu(Dense(LayerNorm(x))))) -- the second half of a pre-norm transformer block (backbones/swin.py:233-236) -- on the
    fused kernels of the ConvNeXt stages (csrc/mlp_fused.hip, csrc/mlp_wgrad.hip: C = 96 / 192, hidden 4C, bf16): LayerNorm rides the row
    loads, the [M, 4C] hidden tile never leaves the CU in either direction, the skip connection and the drop-path factor ride the epilogue.
    Replaces LayerNorm + two GEMMs forward and LayerNorm backward + four GEMMs + their split-K sums + the residual fork backward."""

    @staticmethod
    def forward(ctx, x, ln_gamma, ln_beta, eps, W1, b1, W2, b2, rowscale):
        C = x.shape[-1]
        x2 = _c(x).reshape(-1, C)
        M = x2.shape[0]
        rpg = M // rowscale.shape[0] if rowscale is not None else 0
        fw, bw = nn.mlp_tiled(W1, W2, None)
        out, mean, rstd = K.convnext_mlp_fwd_ln(x2, ln_gamma.data, ln_beta.data, eps, fw, b1.data, b2.data, None, rowscale, rpg, x2)
        ctx.params, ctx.rpg = (ln_gamma, ln_beta, W1, b1, W2, b2), rpg
        ctx.save_for_backward(x2, mean, rstd, bw, rowscale)
        return out.reshape(x.shape)

    @staticmethod
    def backward(ctx, dout):
        x2, mean, rstd, bw, rowscale = ctx.saved_tensors
        ln_gamma, ln_beta, W1, b1, W2, b2 = ctx.params
        M, C = x2.shape
        do2 = _c(dout).reshape(M, C)
        ln = (mean, rstd, ln_gamma.data, ln_beta.data)
        dln = _LnMlpResidualFn.mlp_ln_backward(x2, do2, bw, ln, (ln_gamma, ln_beta, W1, b1, W2, b2, None), rowscale, ctx.rpg)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = K.axpby(do2, dln, 1.0, 1.0, out=dln).reshape(dout.shape)      # + the skip connection's share
        dist.grads_ready(ln_gamma, ln_beta, W1, b1, W2, b2)
        return (dx,) + (None,) * 8

    @staticmethod
    def mlp_ln_backward(rows, dout, bw, ln, params, rowscale, rows_per_group):
        """Backward of Dense(gelu(Dense(LayerNorm(rows)))) (o gamma, o the row factor) on the fused kernels: returns the gradient of `rows` and
        books the gradients of params = (ln_gamma, ln_beta, w1, b1, w2, b2, gamma), gamma possibly None; ln = (mean, rstd, ln_gamma, ln_beta) as
        saved by the forward pass, `bw` the tiled weight images.  Nothing [M, 4C]-shaped reaches HBM: one kernel carries the data gradient
        through the recomputed hidden tile and, in its epilogue, through the LayerNorm backward (which books dln_gamma / dln_beta); a second one
        (csrc/mlp_wgrad.hip) recomputes the tile again and contracts over the rows for every parameter gradient of the MLP.  Where the one-pass
        kernel exists (C = 96, csrc/mlp_bwd_onepass.hip) and an MLP parameter wants its gradient, the two are ONE kernel that forms the tile once."""
        ln_gamma, ln_beta, w1, b1, w2, b2, gamma = params
        gam, dgam = (gamma.data, _grad_out(gamma)) if gamma is not None else (None, None)
        mlp_grads = any(q is not None and q.requires_grad for q in (w1, b1, w2, b2, gamma))
        if mlp_grads and K.convnext_mlp_bwd_onepass_supported(rows.shape[1], rows.dtype):
            return K.convnext_mlp_bwd_onepass(rows, dout, bw, b1.data, w2.data, b2.data, gam, ln, _grad_out(ln_gamma), _grad_out(ln_beta),
                                              _grad_out(w1), _grad_out(b1), _grad_out(w2), _grad_out(b2), dgam, rowscale, rows_per_group)
        drows = K.convnext_mlp_bwd_data_ln(rows, dout, bw, b1.data, ln, _grad_out(ln_gamma), _grad_out(ln_beta), rowscale, rows_per_group)
        if mlp_grads:
            K.convnext_mlp_wgrad(rows, dout, bw, b1.data, w2.data, b2.data, gam, _grad_out(w1), _grad_out(b1), _grad_out(w2), _grad_out(b2), dgam,
                                 rowscale, rows_per_group, ln=ln)
        return drows


def ln_mlp_residual_supported(x, params, drop_path_mask=None):
    """the fused route exists for bf16 rows of 96 / 192 channels with a 4x hidden layer, every parameter trainable (or none needed), and a
    drop-path group size the kernels' 64-row tiles divide"""
    ln_gamma, ln_beta, W1, b1, W2, b2 = params
    C = x.shape[-1]
    if any(p is None for p in params) or not K.convnext_mlp_supported(C, x.dtype) or C not in (96, 192):
        return False
    if tuple(W1.shape) != (C, 4 * C) or tuple(W2.shape) != (4 * C, C):
        return False
    if not all(p.requires_grad for p in params) and torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params)):
        return False      # partly frozen: the weight-gradient kernel books all six parameters
    rows = x.numel() // C
    return drop_path_mask is None or (rows % drop_path_mask.shape[0] == 0 and (rows // drop_path_mask.shape[0]) % 64 == 0)


def ln_mlp_residual(x, ln_gamma, ln_beta, eps, W1, b1, W2, b2, drop_path_mask=None):
    """x + drop_path_mask[sample] * dense(gelu(dense(layer_norm(x)))) as ONE tape node (ln_mlp_residual_supported(...) must hold)"""
    _check_act_dtype(x)
    if nn.dry_run():
        return _dry(x.shape, x)
    return _LnMlpResidualFn.apply(x, ln_gamma, ln_beta, float(eps), W1, b1, W2, b2, drop_path_mask)


def dense(x, W, b=None, act=K.ACT_NONE, kshape=None):
    """kshape=(in, out) re-interprets a higher-rank kernel (keras MultiHeadAttention: [C, heads, d] / [heads, d, C]) as [in, out]"""
    _check_act_dtype(x)
    if nn.dry_run():
        return _dry((*x.shape[:-1], kshape[1] if kshape is not None else W.shape[-1]), x)
    return _DenseFn.apply(x, W, b, act, kshape)


# ---------------------------------------------------------------------------------------------------------
# Conv2D;   kernel [kh,kw,Cin/groups,Cout]
# ---------------------------------------------------------------------------------------------------------
def _conv_geometry(H, W, kh, kw, strides, dilation, padding):
    sh, sw = strides
    dh, dw = dilation
    if padding == "same":
        Ho, pt = K.same_pad(H, kh, sh, dh)
        Wo, pl = K.same_pad(W, kw, sw, dw)
    elif padding == "valid":
        Ho = (H - (kh - 1) * dh - 1) // sh + 1
        Wo = (W - (kw - 1) * dw - 1) // sw + 1
        pt = pl = 0
    elif isinstance(padding, tuple):          # ((top, bottom), (left, right)): ZeroPadding2D followed by a "valid" window op
        (pt, pb), (pl, pr) = padding
        Ho = (H + pt + pb - (kh - 1) * dh - 1) // sh + 1
        Wo = (W + pl + pr - (kw - 1) * dw - 1) // sw + 1
    else:
        raise ValueError(f"padding {padding!r} not supported")
    return Ho, Wo, pt, pl


class _Conv2dFn(Function):
    """Three routes: (1) 1x1 / stride 1 / one group on the activation as it lies = a plain GEMM; (2) bf16 storage with channels per
    group that are multiples of 8 = implicit GEMM on the matrix cores (csrc/conv_igemm.hip: the patch matrix is gathered while the
    operand tile is staged, the data gradient is a gather over dy -- no column buffer, no col2im); (3) everything else (the fp32 parity
    mode, Cin = 3 stems) = im2col + GEMM + col2im, group by group.  Inside (2), a kernel == stride convolution whose map the kernel divides
    (ConvNeXt's downsampling layers) runs each pass that K.conv2d_patch_supported takes as a plain LDS-DMA GEMM over the patch view of the
    tensor (csrc/conv_patchify.hip)."""

    @staticmethod
    def forward(ctx, x, W, b, strides, dilation, padding, groups):
        kh, kw, Cin_g, Cout = W.shape
        N, H, Wd, Cin = x.shape
        if Cin != Cin_g * groups or Cout % groups != 0:
            raise ValueError(f"Conv2D: kernel {tuple(W.shape)} does not fit {Cin} input channels in {groups} groups")
        Ho, Wo, pt, pl = _conv_geometry(H, Wd, kh, kw, strides, dilation, padding)
        cdt = nn.compute_dtype()
        xc = _c(x)
        geom = K.conv_geom(N, H, Wd, Cin, Cout, kh, kw, strides[0], strides[1], dilation[0], dilation[1], pt, pl, Ho, Wo, groups)
        direct = kh == 1 and kw == 1 and strides == (1, 1) and groups == 1 and xc.dtype == cdt and Cin % 8 == 0
        igemm = (not direct) and xc.dtype == cdt and K.conv2d_igemm_supported(geom, cdt)
        M = N * Ho * Wo
        # kernel == stride (ConvNeXt's 2x2 / s2 downsamples): each pass a plain GEMM over the patch view of the tensor, where the native query
        # takes it (csrc/conv_patchify.hip); the three passes route independently
        patch = (False, False, False)
        if igemm and (kh, kw) == strides and dilation == (1, 1) and groups == 1:
            patch = tuple(K.conv2d_patch_supported(geom, cdt, p) for p in (K.PATCH_FWD, K.PATCH_BWD_DATA, K.PATCH_BWD_WEIGHT))
        Wt = nn.wt(W, (kh * kw * Cin, Cout)) if patch[0] else None
        if Wt is not None:
            y = K.conv2d_patch_fwd(xc, Wt, b.data if b is not None else None, geom)
        elif direct:
            Wt = _kcontig_kernel(W, xc.reshape(-1, Cin), Cin, Cout)
            if Wt is not None:
                y = K.dense_fwd_t(xc.reshape(-1, Cin), Wt, b.data if b is not None else None)
            else:
                y = torch.empty((M, Cout), dtype=cdt, device=x.device)
                K.gemm(xc.reshape(-1, Cin), nn.w(W).reshape(Cin, Cout), y, M, Cout, Cin, lda=Cin, ldb=Cout, ldd=Cout, a_kcontig=1, b_kcontig=0,
                       bias=(b.data if b is not None else None))
        elif igemm:
            Wt = None
            if K.conv2d_igemm_fwd_kt_supported(geom, cdt):      # LDS-DMA form on the K-contiguous kernel copy
                Wt = nn.wt(W, (kh * kw * Cin, Cout))
            if Wt is not None:
                y = K.conv2d_igemm_fwd_kt(xc, Wt, b.data if b is not None else None, geom)
            else:
                y = K.conv2d_igemm_fwd(xc, nn.w(W), b.data if b is not None else None, geom)
        else:
            y = torch.empty((M, Cout), dtype=cdt, device=x.device)
            Kd, og = kh * kw * Cin_g, Cout // groups
            keep_col = None
            for g in range(groups):
                col = K.im2col(_group_slice(xc, g, Cin_g, groups), kh, kw, strides[0], strides[1], dilation[0], dilation[1], pt, pl, Ho, Wo, cdt)
                K.gemm(col, nn.w(W).reshape(Kd, Cout)[:, g * og:], y[:, g * og:], M, og, Kd, lda=col.stride(0), ldb=Cout, ldd=Cout, a_kcontig=1,
                       b_kcontig=0, bias=(b.data[g * og:(g + 1) * og] if b is not None else None))
                keep_col = col
            # a patchify stem on the image (Cin = 3, kernel == stride): the column buffer is smaller than the fp32 image it came from, and
            # the weight gradient is its only other reader -- keep it instead of running im2col again in backward (63 us at 16 x 512 x 512)
            ctx.col = keep_col if (groups == 1 and W.requires_grad and not ctx.needs_input_grad[0] and Kd * keep_col.element_size() <=
                                   Cin * xc.element_size() * strides[0] * strides[1]) else None
        ctx.W, ctx.b = W, b
        ctx.geom, ctx.route, ctx.patch = geom, (direct, igemm), patch
        ctx.x_dtype = x.dtype
        ctx.save_for_backward(xc)
        return y.reshape(N, Ho, Wo, Cout)

    @staticmethod
    def backward(ctx, dy):
        (xc,) = ctx.saved_tensors
        W, b, g_ = ctx.W, ctx.b, ctx.geom
        direct, igemm = ctx.route
        N, H, Wd, Cin, Cout, kh, kw, groups = g_.N, g_.H, g_.W, g_.Cin, g_.Cout, g_.KH, g_.KW, g_.groups
        Ho, Wo, pt, pl = g_.Ho, g_.Wo, g_.pt, g_.pl
        st, di = (g_.sh, g_.sw), (g_.dh, g_.dw)
        Cin_g, og = Cin // groups, Cout // groups
        Kd = kh * kw * Cin_g
        cdt = nn.compute_dtype()
        M = N * Ho * Wo
        dy2 = _c(dy).reshape(M, Cout)
        want_b = b is not None and b.requires_grad
        patch_w = ctx.patch[2] and W.requires_grad      # the bias gradient rides the weight gradient's ones-row
        if want_b and not patch_w:
            K.colsum(dy2, Cout, 0, 1, M, Cout, _grad(b), accumulate=True)
        need_dx = ctx.needs_input_grad[0]
        dx = None
        if direct:
            if W.requires_grad:
                K.gemm(xc.reshape(-1, Cin), dy2, _grad(W).reshape(Cin, Cout), Cin, Cout, M, lda=Cin, ldb=Cout, ldd=Cout, a_kcontig=0, b_kcontig=0,
                       accumulate=True)
            if need_dx:
                dx = K.dense_dgrad(dy2, nn.w(W).reshape(Cin, Cout)).reshape(N, H, Wd, Cin)
        elif igemm:
            dy4 = dy2.reshape(N, Ho, Wo, Cout)
            if patch_w:
                K.conv2d_patch_bwd_weight(xc, dy4, _grad(W), g_, accumulate=True, bias_grad=_grad(b) if want_b else None)
            elif W.requires_grad:
                K.conv2d_igemm_bwd_weight(xc, dy4, _grad(W), g_, accumulate=True)
            patchify = (kh, kw) == st      # kernel == stride: the column buffer IS dx up to a permutation, one plain GEMM fills it
            if need_dx and ctx.patch[1]:
                dx = K.conv2d_patch_bwd_data(dy4, nn.w(W), g_)      # that GEMM, stored straight to the pixels: no column buffer, no col2im
            elif need_dx and (st == (1, 1) or (di == (1, 1) and st[0] * st[1] <= 16 and not patchify)):
                # stride 1: one gather over dy; strided and undilated: one stride-1 gather per stride phase, all phases in one launch, rows
                # scattered to their pixels by the epilogue (csrc/conv_igemm.hip pass 3) -- no zero products, no column buffer, no col2im
                # (ResNet's 3x3 / s2 at 64x64x128: 23 us against 40 us for GEMM + col2im)
                dx = K.conv2d_igemm_bwd_data(dy4, nn.w(W), g_)
            elif need_dx:
                # strided and dilated (1 / (sh * sw) of the (tap, pixel) pairs of the plain gather form are non-zero, and the MFMA cannot skip
                # them), or kernel == stride (ConvNeXt's 2x2 / s2 downsamples: the LDS-DMA GEMM + permutation measures 35 / 29 us against
                # 46 / 39 us for the phase launch at stages 1 / 2, equal at stage 0; tools/kbench_conv_strided.py): dcol = dy @ W^T, then the
                # gather-form col2im (deterministic)
                ldc = (Kd + 7) // 8 * 8
                dx = torch.empty((N, H, Wd, Cin), dtype=cdt, device=dy.device) if groups > 1 else None
                for g in range(groups):
                    dcol = torch.empty((M, ldc), dtype=cdt, device=dy.device)
                    K.gemm(dy2[:, g * og:], nn.w(W).reshape(Kd, Cout)[:, g * og:], dcol, M, Kd, og, lda=Cout, ldb=Cout, ldd=ldc, a_kcontig=1,
                           b_kcontig=1)
                    dxg = K.col2im(dcol, N, H, Wd, Cin_g, kh, kw, st[0], st[1], di[0], di[1], pt, pl, Ho, Wo)
                    if groups == 1:
                        dx = dxg
                    else:
                        K.copy2d(dxg.reshape(-1, Cin_g), Cin_g, dx.reshape(-1, Cin)[:, g * Cin_g:], Cin, N * H * Wd, Cin_g)
        else:
            if need_dx:
                dx = torch.empty((N, H, Wd, Cin), dtype=cdt, device=dy.device)
            ldc = (Kd + 7) // 8 * 8
            for g in range(groups):
                dyg = dy2[:, g * og:]
                if W.requires_grad:
                    col = getattr(ctx, "col", None)
                    if col is None:
                        col = K.im2col(_group_slice(xc, g, Cin_g, groups), kh, kw, st[0], st[1], di[0], di[1], pt, pl, Ho, Wo, cdt)
                    K.gemm(col, dyg, _grad(W).reshape(Kd, Cout)[:, g * og:], Kd, og, M, lda=col.stride(0), ldb=Cout, ldd=Cout, a_kcontig=0,
                           b_kcontig=0, accumulate=True)
                    del col
                if need_dx:
                    dcol = torch.empty((M, ldc), dtype=cdt, device=dy.device)
                    K.gemm(dyg, nn.w(W).reshape(Kd, Cout)[:, g * og:], dcol, M, Kd, og, lda=Cout, ldb=Cout, ldd=ldc, a_kcontig=1, b_kcontig=1)
                    dxg = K.col2im(dcol, N, H, Wd, Cin_g, kh, kw, st[0], st[1], di[0], di[1], pt, pl, Ho, Wo)
                    if groups == 1:
                        dx = dxg
                    else:
                        K.copy2d(dxg.reshape(-1, Cin_g), Cin_g, dx.reshape(-1, Cin)[:, g * Cin_g:], Cin, N * H * Wd, Cin_g)
        if dx is not None and dx.dtype != ctx.x_dtype:
            dx = K.cast(dx, ctx.x_dtype)
        dist.grads_ready(W, b)
        return dx, None, None, None, None, None, None


def _group_slice(xc, g, Cin_g, groups):
    """dense NHWC copy of one channel group (the im2col kernel reads dense tensors); groups == 1 is the tensor itself"""
    if groups == 1:
        return xc
    N, H, W, Cin = xc.shape
    out = torch.empty((N, H, W, Cin_g), dtype=xc.dtype, device=xc.device)
    K.copy2d(xc.reshape(-1, Cin)[:, g * Cin_g:], Cin, out.reshape(-1, Cin_g), Cin_g, N * H * W, Cin_g)
    return out


def conv2d(x, W, b=None, strides=(1, 1), dilation=(1, 1), padding="same", groups=1):
    if nn.dry_run():
        Ho, Wo, _, _ = _conv_geometry(x.shape[1], x.shape[2], W.shape[0], W.shape[1], tuple(strides), tuple(dilation), padding)
        return _dry((x.shape[0], Ho, Wo, W.shape[-1]), x, nn.compute_dtype())
    return _Conv2dFn.apply(x, W, b, tuple(strides), tuple(dilation), padding, int(groups))


# ---------------------------------------------------------------------------------------------------------
# Several Conv2D of ONE input (ASPP's pixel-level branches): stride 1, "same" padding, one group, no bias, the same filter count
# ---------------------------------------------------------------------------------------------------------
def _branch_taps(Ws, dilations):
    return [(W.shape[0], W.shape[1], d[0], d[1]) for W, d in zip(Ws, dilations)]


def conv2d_branches_supported(x, Ws, dilations):
    """one launch per pass can take these convolutions of x (csrc/conv_igemm.hip iseg_conv2d_branches_*): bf16 storage, kernels
    [kh,kw,Cin,Cout] of one Cin / Cout, both multiples of 64, at most K.CONV_MAX_BRANCHES of them"""
    from . import _hip

    cdt = nn.compute_dtype()
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 4 and x.dtype == cdt and 1 <= len(Ws) <= _hip.CONV_MAX_BRANCHES):
        return False
    N, H, Wd, Cin = x.shape
    Cout = Ws[0].shape[3]
    if any(W is None or W.dim() != 4 or W.shape[2] != Cin or W.shape[3] != Cout for W in Ws):
        return False
    if not K.conv2d_branches_supported(K.conv_branches(N, H, Wd, Cin, Cout, _branch_taps(Ws, dilations)), cdt):
        return False
    return all(nn.wt(W, (W.shape[0] * W.shape[1] * Cin, Cout)) is not None for W in Ws)


class _Conv2dBranchesFn(Function):
    """y_b = conv(x, W_b) for every branch in one grouped launch; backward: one grouped weight-gradient launch and ONE data-gradient product
    whose reduction runs over (branch, tap, channel) -- the branch gradients of x are summed in fp32 and rounded once, no axpby"""

    @staticmethod
    def forward(ctx, x, dilations, *Ws):
        N, H, Wd, Cin = x.shape
        Cout = Ws[0].shape[3]
        xc = _c(x)
        ctx.taps = _branch_taps(Ws, dilations)
        table = K.conv_branches(N, H, Wd, Cin, Cout, ctx.taps)
        ys = K.conv2d_branches_fwd(xc, [nn.wt(W, (W.shape[0] * W.shape[1] * Cin, Cout)) for W in Ws], table)
        ctx.Ws = Ws
        ctx.save_for_backward(xc)
        return tuple(ys)

    @staticmethod
    def backward(ctx, *dys):
        (xc,) = ctx.saved_tensors
        Ws = ctx.Ws
        N, H, Wd, Cin = xc.shape
        Cout = Ws[0].shape[3]
        rows = [_rows2d(dy) for dy in dys]
        dy2, ld = [r[0] for r in rows], [r[1] for r in rows]
        live = [i for i, W in enumerate(Ws) if W.requires_grad]
        if live:
            table = K.conv_branches(N, H, Wd, Cin, Cout, [ctx.taps[i] for i in live])
            K.conv2d_branches_bwd_weight(xc, [dy2[i] for i in live], [ld[i] for i in live], [_grad(Ws[i]) for i in live], table, accumulate=True)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = K.conv2d_branches_bwd_data(dy2, ld, [nn.w(W) for W in Ws], K.conv_branches(N, H, Wd, Cin, Cout, ctx.taps))
        for W in Ws:
            dist.grads_ready(W, None)
        return (dx, None) + (None,) * len(Ws)


def conv2d_branches(x, Ws, dilations):
    """[conv2d(x, W, dilation=d, padding="same") for W, d in zip(Ws, dilations)] as ONE tape node (conv2d_branches_supported(...) must hold)"""
    _check_act_dtype(x)
    return list(_Conv2dBranchesFn.apply(x, tuple(tuple(d) for d in dilations), *Ws))


# ---------------------------------------------------------------------------------------------------------
# DepthwiseConv2D, stride 1;  kernel [K,K,C,1]
# ---------------------------------------------------------------------------------------------------------
class _DWConvFn(Function):
    @staticmethod
    def forward(ctx, x, W, b, dil):
        Kk, C = W.shape[0], W.shape[2]
        pad = (Kk - 1) * dil // 2
        xc = _c(x)
        y = K.dwconv2d(xc, W.data.reshape(Kk * Kk, C), b.data if b is not None else None, Kk, dil, pad, pad)
        ctx.W, ctx.b, ctx.dil, ctx.pad = W, b, dil, pad
        ctx.save_for_backward(xc)
        return y

    @staticmethod
    def backward(ctx, dy):
        (xc,) = ctx.saved_tensors
        W, b, dil, pad = ctx.W, ctx.b, ctx.dil, ctx.pad
        Kk, C = W.shape[0], W.shape[2]
        dyc = _c(dy)
        if W.requires_grad or (b is not None and b.requires_grad):
            K.dwconv2d_bwd_weight(xc, dyc, _grad_out(W, Kk * Kk, C), _grad_out(b) if b is not None else None, Kk, dil, pad, pad)
        dx = None
        if ctx.needs_input_grad[0]:
            padb = (Kk - 1) * dil - pad
            dx = K.dwconv2d(dyc, W.data.reshape(Kk * Kk, C), None, Kk, dil, padb, padb, flip=True)
        dist.grads_ready(W, b)
        return dx, None, None, None


class _DWConvStridedFn(Function):
    """DepthwiseConv2D(strides = s, padding = 'same'): forward, data gradient (gather over dy) and weight gradient at the strided output
    positions only (csrc/dwconv_strided.hip)"""

    @staticmethod
    def forward(ctx, x, W, b, dil, stride):
        Kk, C = W.shape[0], W.shape[2]
        xc = _c(x)
        y = K.dwconv2d_strided(xc, W.data.reshape(Kk * Kk, C), b.data if b is not None else None, Kk, stride, dil)
        ctx.W, ctx.b, ctx.dil, ctx.stride = W, b, dil, stride
        ctx.save_for_backward(xc)
        return y

    @staticmethod
    def backward(ctx, dy):
        (xc,) = ctx.saved_tensors
        W, b, dil, stride = ctx.W, ctx.b, ctx.dil, ctx.stride
        Kk, C = W.shape[0], W.shape[2]
        dyc = _c(dy)
        if W.requires_grad or (b is not None and b.requires_grad):
            K.dwconv2d_strided_bwd_weight(xc, dyc, _grad_out(W, Kk * Kk, C), _grad_out(b) if b is not None else None, Kk, stride, dil)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = K.dwconv2d_strided_bwd_data(dyc, W.data.reshape(Kk * Kk, C), Kk, stride, dil, xc.shape[1], xc.shape[2])
        dist.grads_ready(W, b)
        return dx, None, None, None, None


def depthwise_conv2d(x, W, b=None, dilation=1, strides=1):
    """padding='same'.  Stride 1 is the hot path (ConvNeXt 7x7, SepConvBnReLU 3x3 dilated); a strided layer (the stride-2 depthwise
    convolutions of the separable / inverted-residual families) runs the dedicated kernels that visit the strided outputs only."""
    _check_act_dtype(x)
    s = int(strides)
    if s == 1:
        if nn.dry_run():
            return _dry(x.shape, x)
        return _DWConvFn.apply(x, W, b, int(dilation))
    N, H, Wd, C = x.shape
    if nn.dry_run():
        return _dry((N, -(-H // s), -(-Wd // s), C), x)
    return _DWConvStridedFn.apply(x, W, b, int(dilation), s)


# ---------------------------------------------------------------------------------------------------------
# LayerNormalization(axis=-1)
# ---------------------------------------------------------------------------------------------------------
class _LayerNormFn(Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        C = x.shape[-1]
        x2 = _c(x).reshape(-1, C)
        y, mean, rstd = K.layernorm_fwd(x2, gamma.data, beta.data, eps)
        ctx.gamma, ctx.beta = gamma, beta
        ctx.save_for_backward(x2, mean, rstd)
        return y.reshape(x.shape)

    @staticmethod
    def backward(ctx, dy):
        x2, mean, rstd = ctx.saved_tensors
        C = x2.shape[-1]
        dx = K.layernorm_bwd(_c(dy).reshape(-1, C), x2, ctx.gamma.data, mean, rstd, _grad_out(ctx.gamma), _grad_out(ctx.beta))
        dist.grads_ready(ctx.gamma, ctx.beta)
        return dx.reshape(dy.shape), None, None, None


class _LayerNormPostFn(Function):
    """residual + drop_path_mask[sample] * colscale * layer_norm(x): the tail of a post-norm residual branch (InternImage, post_norm = True) as one
    pass each way -- LayerNorm, layer scale, drop path and the skip connection forward; backward one LayerNorm-backward pass whose two column
    sums also give the layer-scale gradient (csrc/norm.hip LnPost)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, colscale, rowscale, residual):
        C = x.shape[-1]
        x2 = _c(x).reshape(-1, C)
        rpg = x2.shape[0] // rowscale.shape[0] if rowscale is not None else 0
        r2 = _c(residual).reshape(-1, C) if residual is not None else None
        y, mean, rstd = K.layernorm_post_fwd(x2, gamma.data, beta.data, eps, colscale.data if colscale is not None else None, rowscale, rpg, r2)
        ctx.params, ctx.rpg = (gamma, beta, colscale), rpg
        ctx.save_for_backward(x2, mean, rstd, rowscale)
        return y.reshape(x.shape)

    @staticmethod
    def backward(ctx, dy):
        x2, mean, rstd, rowscale = ctx.saved_tensors
        gamma, beta, colscale = ctx.params
        C = x2.shape[1]
        want_cs = colscale is not None and colscale.requires_grad
        dx = K.layernorm_post_bwd(_c(dy).reshape(-1, C), x2, gamma.data, beta.data, mean, rstd, _grad_out(gamma), _grad_out(beta),
                                  colscale=colscale.data if colscale is not None else None, dcolscale=_grad(colscale) if want_cs else None,
                                  rowscale=rowscale, rows_per_group=ctx.rpg)
        dist.grads_ready(gamma, beta, colscale) if colscale is not None else dist.grads_ready(gamma, beta)
        return (dx.reshape(dy.shape) if ctx.needs_input_grad[0] else None), None, None, None, None, None, (dy if ctx.needs_input_grad[6] else None)


def layer_norm_post(x, gamma, beta, eps, colscale=None, drop_path_mask=None, residual=None):
    """residual + drop_path_mask[sample] * colscale * layer_norm(x, gamma, beta, eps) as one tape node (channels % 8 == 0; gamma and beta trainable)"""
    _check_act_dtype(x)
    if nn.dry_run():
        return _dry(x.shape, x)
    return _LayerNormPostFn.apply(x, gamma, beta, float(eps), colscale, drop_path_mask, residual)


def layer_norm(x, gamma, beta, eps):
    _check_act_dtype(x)
    if nn.dry_run():
        return _dry(x.shape, x)
    return _LayerNormFn.apply(x, gamma, beta, float(eps))


# ---------------------------------------------------------------------------------------------------------
# (Sync)BatchNormalization over all axes but the last, optional fused ReLU.  The statistics exchange of every tape node that carries a
# BatchNorm is stated here once: _bn_batch_stats (forward), _bn_exchange_sums (backward), _bn_frozen_stats (moving statistics).
# ---------------------------------------------------------------------------------------------------------
def _bn_batch_stats(x2s, sync):
    """packed [sum | sumsq | count] ([2C+1] floats) of every [rows, C] tensor in x2s, summed over the replicas when `sync`: ONE message for all
    of them (and one instead of the reference's three per layer) -- the exposed latency of a small RCCL message is paid once (hard
    part 4)"""
    if len(x2s) == 1:
        rows, C = x2s[0].shape
        msg = K.bn_stats(x2s[0], C, rows, C)
        slots = [msg]
    else:
        offs = [0]
        for x2 in x2s:
            offs.append(offs[-1] + 2 * x2.shape[1] + 4)      # 3 floats of padding: every layer's slot stays 16-byte aligned
        msg = torch.zeros(offs[-1], dtype=torch.float32, device=x2s[0].device)
        slots = []
        for x2, off in zip(x2s, offs):
            rows, C = x2.shape
            slots.append(K.bn_stats(x2, C, rows, C, out=msg[off:off + 2 * C + 1]))
    if sync:
        dist.all_reduce_sum(msg)
    return slots


def _bn_frozen_stats(moving_mean, moving_var, eps):
    """(mean, rstd) of a call on the moving statistics.  The mean is a copy: the backward reads the statistics of THIS call, and a later
    training-mode call updates the buffer in place through a raw pointer, which autograd's version counter cannot see"""
    return moving_mean.clone(), K.rsqrt_eps(moving_var, eps)


def _bn_exchange_sums(sums, layers, sync):
    """`sums`: the [dbeta | dgamma] blocks ([2C] each, back to back) that the backward reductions of `layers` ((gamma, beta) pairs) left for this
    replica.  Returns (sums, world, own); the input gradient takes 1 / (rows * world) for its mean over the batch.

    own: no exchange -- the sums are this replica's, so the caller's apply kernel books dgamma / dbeta itself and the caller reports
    dist.grads_ready after that launch.
    not own: the local parameter gradients are booked here (the gradient all-reduce sums them over the ranks later) and reported BEFORE the
    statistics message, so that a gradient bucket can go out before that message is waited for; then a copy of the sums is summed over the
    replicas.  A caller whose reduction has already booked its parameter gradients passes no layers."""
    if not (sync and dist.active()):
        return sums, 1, True
    off = 0
    for gamma, beta in layers:
        C = gamma.shape[0]
        K.accumulate_pair(sums[off:off + 2 * C], C, _param_grad(beta), _param_grad(gamma))
        off += 2 * C
    dist.grads_ready(*[p for layer in layers for p in layer])
    sums = sums.clone()
    dist.all_reduce_sum(sums)
    return sums, dist.world_size(), False


def _aligned16(tensors, vectors):
    """the 16-byte alignment the fused kernels' vector accesses need: of an activation when it is passed as is (a non-contiguous one is copied
    into a fresh, aligned buffer first) and of the per-channel vectors and kernels they read directly, which must be contiguous as well"""
    return (not any(t.is_contiguous() and t.data_ptr() % 16 for t in tensors)
            and not any(v.data_ptr() % 16 or not v.is_contiguous() for v in vectors))


class _BatchNormTrainFn(Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, moving_mean, moving_var, eps, momentum, relu, sync):
        C = x.shape[-1]
        x2 = _c(x).reshape(-1, C)
        rows = x2.shape[0]
        (packed,) = _bn_batch_stats([x2], sync)
        y = torch.empty_like(x2)
        mean, rstd = K.bn_finalize_apply(packed, x2, C, gamma.data, beta.data, y, C, rows, C, eps, momentum, moving_mean, moving_var, relu)
        ctx.gamma, ctx.beta, ctx.relu, ctx.sync = gamma, beta, relu, sync
        ctx.save_for_backward(x2, y if relu else None, mean, rstd)
        return y.reshape(x.shape)

    @staticmethod
    def backward(ctx, dy):
        x2, y, mean, rstd = ctx.saved_tensors
        gamma, beta = ctx.gamma, ctx.beta
        rows, C = x2.shape
        dy2, lddy = _rows2d(dy)
        sums = K.bn_bwd_reduce(dy2, lddy, x2, C, y, C, mean, rstd, rows, C, ctx.relu)
        sums, world, own = _bn_exchange_sums(sums, [(gamma, beta)], ctx.sync)
        dx = torch.empty_like(x2)
        K.bn_bwd_apply(dy2, lddy, x2, C, y, C, mean, rstd, gamma.data, sums, 1.0 / (rows * world), dx, C, rows, C, ctx.relu,
                       dgamma=_param_grad(gamma) if own else None, dbeta=_param_grad(beta) if own else None)
        if own:
            dist.grads_ready(gamma, beta)
        return dx.reshape(dy.shape), None, None, None, None, None, None, None, None


class _BnReluUpsampleAddFn(Function):
    """relu(batch_norm(z)) + resize_bilinear(x, z's height and width) -- one level of the FPN top-down pathway (layers/fpn.py:46-57) -- with
    training-mode (Sync)BN statistics: the normalised map and the up-sampled map are never written, and the backward pass re-derives the
    ReLU mask from z instead of reading a saved output.  Statistics / parameter-gradient arithmetic is _BatchNormTrainFn's."""

    @staticmethod
    def forward(ctx, z, x, gamma, beta, moving_mean, moving_var, eps, momentum, sync):
        C = z.shape[-1]
        zc, xc = _c(z), _c(x)
        z2 = zc.reshape(-1, C)
        (packed,) = _bn_batch_stats([z2], sync)
        mean, rstd = K.bn_finalize(packed, C, eps, momentum, moving_mean, moving_var)
        out = K.bn_relu_upsample_add(zc, mean, rstd, gamma.data, beta.data, xc)
        ctx.gamma, ctx.beta, ctx.sync, ctx.x_shape, ctx.x_dtype = gamma, beta, sync, x.shape, x.dtype
        ctx.save_for_backward(z2, mean, rstd)
        return out

    @staticmethod
    def backward(ctx, dout):
        z2, mean, rstd = ctx.saved_tensors
        gamma, beta = ctx.gamma, ctx.beta
        rows, C = z2.shape
        dc = _c(dout)
        d2 = dc.reshape(rows, C)
        dx = K.resize_bilinear_bwd(dc, ctx.x_shape[1], ctx.x_shape[2], ctx.x_dtype) if ctx.needs_input_grad[1] else None
        dz = None
        sums = K.bn_bwd_reduce_remask(d2, C, z2, C, mean, rstd, gamma.data, beta.data, rows, C)
        sums, world, own = _bn_exchange_sums(sums, [(gamma, beta)], ctx.sync)
        dgamma, dbeta = (_param_grad(gamma), _param_grad(beta)) if own else (None, None)
        if ctx.needs_input_grad[0]:
            dz = K.bn_bwd_apply_remask(d2, C, z2, C, mean, rstd, gamma.data, beta.data, sums, 1.0 / (rows * world), torch.empty_like(z2), C, rows, C,
                                       dgamma=dgamma, dbeta=dbeta).reshape(dout.shape)
        elif own:      # no apply launch to book them
            K.accumulate_pair(sums, C, dbeta, dgamma)
        if own:
            dist.grads_ready(gamma, beta)
        return dz, dx, None, None, None, None, None, None, None


def batch_norm_relu_upsample_add(z, x, gamma, beta, moving_mean, moving_var, eps, momentum, sync=True):
    """relu(batch_norm(z, training=True)) + resize_bilinear(x, z.shape[1:3]) as one tape node; channels % 8 == 0, same dtype"""
    _check_act_dtype(z)
    if nn.dry_run():
        return _dry(z.shape, z)
    return _BnReluUpsampleAddFn.apply(z, x, gamma, beta, moving_mean, moving_var, float(eps), float(momentum), bool(sync))


class _BatchNormGroupFn(Function):
    """Several independent SyncBN layers whose inputs all exist before any of them is normalised (the five ASPP branches,
    layers/aspp.py:57-71): their statistics travel in ONE all-reduce forward and ONE backward instead of one per layer.  Arithmetic per
    layer is _BatchNormTrainFn's."""

    @staticmethod
    def forward(ctx, n, relu, layers, *tensors):
        xs, gammas, betas = tensors[:n], tensors[n:2 * n], tensors[2 * n:3 * n]
        x2s = [_c(x).reshape(-1, x.shape[-1]) for x in xs]
        ys, saved = [], []
        for x, x2, packed, gamma, beta, L in zip(xs, x2s, _bn_batch_stats(x2s, True), gammas, betas, layers):
            rows, C = x2.shape
            y = torch.empty_like(x2)
            mean, rstd = K.bn_finalize_apply(packed, x2, C, gamma.data, beta.data, y, C, rows, C, L["eps"], L["momentum"], L["moving_mean"],
                                             L["moving_var"], relu)
            ys.append(y.reshape(x.shape))
            saved += [x2, y if relu else None, mean, rstd]
        ctx.relu, ctx.layers = relu, list(zip(gammas, betas))
        ctx.save_for_backward(*saved)
        return tuple(ys)

    @staticmethod
    def backward(ctx, *dys):
        relu, layers, sv = ctx.relu, ctx.layers, ctx.saved_tensors
        n = len(layers)
        offs = [0]
        for gamma, _ in layers:
            offs.append(offs[-1] + 2 * gamma.shape[0])
        msg = torch.empty(offs[-1], dtype=torch.float32, device=sv[0].device)
        dy2s = []
        for i in range(n):
            x2, y, mean, rstd = sv[4 * i:4 * i + 4]
            rows, C = x2.shape
            dy2, lddy = _rows2d(dys[i])
            dy2s.append((dy2, lddy))
            K.bn_bwd_reduce(dy2, lddy, x2, C, y, C, mean, rstd, rows, C, relu, out=msg[offs[i]:offs[i + 1]])
        msg, world, own = _bn_exchange_sums(msg, layers, True)
        dxs = []
        for i, (gamma, beta) in enumerate(layers):
            x2, y, mean, rstd = sv[4 * i:4 * i + 4]
            rows, C = x2.shape
            dx = torch.empty_like(x2)
            K.bn_bwd_apply(dy2s[i][0], dy2s[i][1], x2, C, y, C, mean, rstd, gamma.data, msg[offs[i]:offs[i + 1]], 1.0 / (rows * world),
                           dx, C, rows, C, relu, dgamma=_param_grad(gamma) if own else None, dbeta=_param_grad(beta) if own else None)
            dxs.append(dx.reshape(dys[i].shape))
        if own:
            dist.grads_ready(*[p for layer in layers for p in layer])
        return (None, None, None) + tuple(dxs) + (None,) * (2 * n)


def batch_norm_group(xs, bns, relu=True):
    """training-mode SyncBN of several tensors with one statistics exchange; bns: the BatchNormalization layers (built)"""
    layers = [dict(eps=float(b.epsilon), momentum=float(b.momentum), moving_mean=b.moving_mean, moving_var=b.moving_variance) for b in bns]
    return _BatchNormGroupFn.apply(len(xs), bool(relu), layers, *xs, *[b.gamma for b in bns], *[b.beta for b in bns])


class _BatchNormInferFn(Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, moving_mean, moving_var, eps, relu):
        C = x.shape[-1]
        x2 = _c(x).reshape(-1, C)
        want_param_grads = gamma.requires_grad or beta.requires_grad
        if want_param_grads:      # the backward reads the mean again
            mean, rstd = _bn_frozen_stats(moving_mean, moving_var, eps)
        else:
            mean, rstd = moving_mean, K.rsqrt_eps(moving_var, eps)
        y = torch.empty_like(x2)
        K.bn_apply_fwd(x2, C, mean, rstd, gamma.data, beta.data, y, C, x2.shape[0], C, relu)
        ctx.gamma, ctx.beta, ctx.relu = gamma, beta, relu
        ctx.save_for_backward(y if relu else None, rstd, x2 if want_param_grads else None, mean if want_param_grads else None)
        return y.reshape(x.shape)

    @staticmethod
    def backward(ctx, dy):
        # frozen statistics: dx = dz * gamma * rstd; gamma / beta still receive their gradients (Keras keeps them trainable
        # when a BN layer is called with training=False inside a train step)
        y, rstd, x2, mean = ctx.saved_tensors
        C = dy.shape[-1]
        dy2 = _c(dy).reshape(-1, C)
        if x2 is not None:
            sums = K.bn_bwd_reduce(dy2, C, x2, C, y, C, mean, rstd, x2.shape[0], C, ctx.relu)
            K.accumulate_pair(sums, C, _param_grad(ctx.beta), _param_grad(ctx.gamma))
            dist.grads_ready(ctx.gamma, ctx.beta)
        if ctx.relu:
            dy2 = K.act_bwd(dy2, y, K.ACT_RELU)
        scale = K.axpby(ctx.gamma.data, None, 1.0, 0.0)
        # dx = dy2 * (gamma * rstd) per column: bn_apply with mean = 0 and beta = 0
        zeros = torch.zeros(C, dtype=torch.float32, device=dy.device)
        dx = torch.empty_like(dy2)
        K.bn_apply_fwd(dy2, C, zeros, rstd, scale, zeros, dx, C, dy2.shape[0], C, False)
        return dx.reshape(dy.shape), None, None, None, None, None, None


def batch_norm(x, gamma, beta, moving_mean, moving_var, eps, momentum, training, relu=False, sync=True):
    _check_act_dtype(x)
    if nn.dry_run():
        return _dry(x.shape, x)
    if training:
        return _BatchNormTrainFn.apply(x, gamma, beta, moving_mean, moving_var, float(eps), float(momentum), bool(relu), bool(sync))
    return _BatchNormInferFn.apply(x, gamma, beta, moving_mean, moving_var, float(eps), bool(relu))


# ---------------------------------------------------------------------------------------------------------
# EfficientNet MBConv tail (backbones/efficientnet.py:214-255): (Sync)BN -> swish -> squeeze-excite -> gate as one tape node
# (csrc/mbconv.hip).  The un-gated activation is never written.
# ---------------------------------------------------------------------------------------------------------
def _se_params(W1, b1, W2, b2):
    C, Cse = W1.shape[-2], W1.shape[-1]
    return W1.data.reshape(C, Cse), b1.data, W2.data.reshape(Cse, C), b2.data


def _se_grads(W1, b1, W2, b2):
    C, Cse = W1.shape[-2], W1.shape[-1]
    return _param_grad(W1, C, Cse), _param_grad(b1), _param_grad(W2, Cse, C), _param_grad(b2)


class _BnSwishSEFn(Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, moving_mean, moving_var, W1, b1, W2, b2, eps, momentum, training, sync):
        C = x.shape[-1]
        xc = _c(x)
        if training:
            (packed,) = _bn_batch_stats([xc.reshape(-1, C)], sync)
            mean, rstd = K.bn_finalize(packed, C, eps, momentum, moving_mean, moving_var)
        else:
            mean, rstd = _bn_frozen_stats(moving_mean, moving_var, eps)
        out, m, hpre, g = K.bn_swish_se_fwd(xc, mean, rstd, gamma.data, beta.data, *_se_params(W1, b1, W2, b2))
        ctx.params, ctx.training, ctx.sync = (gamma, beta, W1, b1, W2, b2), training, training and sync
        ctx.save_for_backward(xc, mean, rstd, m, hpre, g)
        return out

    @staticmethod
    def backward(ctx, dout):
        xc, mean, rstd, m, hpre, g = ctx.saved_tensors
        gamma, beta, W1, b1, W2, b2 = ctx.params
        rows = xc.numel() // xc.shape[-1]
        dO = _c(dout)
        W1d, _, W2d, _ = _se_params(W1, b1, W2, b2)
        sums, dmh = K.bn_swish_se_bwd_sums(dO, xc, mean, rstd, gamma.data, beta.data, W1d, W2d, m, hpre, g, *_se_grads(W1, b1, W2, b2))
        dist.grads_ready(W1, b1, W2, b2)
        sums, world, own = _bn_exchange_sums(sums, [(gamma, beta)], ctx.sync)
        inv_n = 1.0 / (rows * world) if ctx.training else 0.0
        dx = K.bn_swish_gate_bwd_apply(dO, xc, mean, rstd, gamma.data, beta.data, g, dmh, sums, inv_n, ctx.training,
                                       dgamma=_param_grad(gamma) if own else None, dbeta=_param_grad(beta) if own else None)
        if own:
            dist.grads_ready(gamma, beta)
        return (dx,) + (None,) * 12


def mbconv_fused_enabled():
    """ISEG_MBCONV_FUSED=0 routes the MBConv tail through the composed kernels (the A/B baseline)"""
    return os.environ.get("ISEG_MBCONV_FUSED", "1") != "0"


def bn_swish_se_supported(x, se_filters, *vectors):
    """the shape rules of csrc/mbconv.hip, and _aligned16 of x and the per-channel vectors (gamma, beta, moving statistics)"""
    N, H, W, C = x.shape
    return _aligned16((x,), vectors) and K.mbconv_supported(N, H * W, C, se_filters)


def bn_swish_se(x, gamma, beta, moving_mean, moving_var, eps, momentum, training, W1, b1, W2, b2, sync=True):
    """x * g with x <- swish(batch_norm(x)), g = sigmoid(conv1x1(swish(conv1x1(mean_hw x, W1, b1)), W2, b2)) per (sample, channel): the
    MBConv tail as one tape node.  W1 [1, 1, C, Cse], W2 [1, 1, Cse, C] (Keras kernels).  Shapes bn_swish_se_supported refuses raise."""
    _check_act_dtype(x)
    if nn.dry_run():
        return _dry(x.shape, x)
    return _BnSwishSEFn.apply(x, gamma, beta, moving_mean, moving_var, W1, b1, W2, b2, float(eps), float(momentum), bool(training), bool(sync))


# ---------------------------------------------------------------------------------------------------------
# Xception separable unit, activation=False (backbones/xception_common.py:14-78): relu -> depthwise 3x3 -> (Sync)BN -> pointwise 1x1 as one
# tape node (csrc/sepconv.hip).  The BN is folded into the pointwise GEMM (v = z diag(a) W + c^T W), so neither relu(x) nor the BN output is
# written.
# ---------------------------------------------------------------------------------------------------------
def _sepconv_pointwise(z2, pwk, mean, rstd, gamma, beta, need_grad):
    """fold the BN into the pointwise kernel and run the GEMM; returns (v, Wn) -- Wn [Cin, Cout], the data gradient's operand, only when
    need_grad (else None).  The forward reads the K-contiguous copy where the LDS-DMA GEMM takes the product (as _kcontig_kernel routes a 1x1
    conv), else Wn; the fold writes only the layouts that will be read."""
    Cin, Cout = pwk.shape[-2], pwk.shape[-1]
    kcontig = (z2.dtype == torch.bfloat16 and Cin % 8 == 0 and Cin >= _DMA_MIN_K and Cout % 8 == 0 and Cout >= 64
               and z2.shape[0] >= 64)
    Wt, Wn, bias = K.sepconv_fold(pwk.data.reshape(Cin, Cout), mean, rstd, gamma.data, beta.data, z2.dtype, want_t=kcontig,
                                  want_n=need_grad or not kcontig)
    v = K.dense_fwd_t(z2, Wt, bias) if kcontig else K.dense_fwd(z2, Wn, bias)
    return v, Wn


class _SepConvFn(Function):
    @staticmethod
    def forward(ctx, x, dwk, gamma, beta, pwk, moving_mean, moving_var, eps, momentum, stride, dil, training, sync):
        C, Cout = x.shape[-1], pwk.shape[-1]
        xc = _c(x)
        z, packed = K.relu_dwconv3_stats(xc, dwk.data.reshape(9, C), stride, dil, stats=training)
        if training:
            if sync:
                dist.all_reduce_sum(packed)          # _bn_batch_stats' one-tensor message, written by the depthwise launch itself
            mean, rstd = K.bn_finalize(packed, C, eps, momentum, moving_mean, moving_var)
        else:
            mean, rstd = _bn_frozen_stats(moving_mean, moving_var, eps)
        v, Wn = _sepconv_pointwise(z.reshape(-1, C), pwk, mean, rstd, gamma, beta, any(ctx.needs_input_grad))
        ctx.params, ctx.training, ctx.sync, ctx.stride, ctx.dil = (dwk, gamma, beta, pwk), training, training and sync, stride, dil
        ctx.save_for_backward(xc, z, mean, rstd, Wn)
        return v.reshape(*z.shape[:-1], Cout)

    @staticmethod
    def backward(ctx, dv):
        """wgrad GEMM + colsum -> fold_bwd -> (all-reduce of the BN sums) -> dgrad GEMM -> fused depthwise / BN / ReLU backward"""
        xc, z, mean, rstd, Wn = ctx.saved_tensors
        dwk, gamma, beta, pwk = ctx.params
        C, Cout = Wn.shape
        dv2 = _c(dv).reshape(-1, Cout)
        z2 = z.reshape(-1, C)
        rows = z2.shape[0]
        G = torch.empty((C, Cout), dtype=torch.float32, device=dv.device)
        S = torch.empty(Cout, dtype=torch.float32, device=dv.device)
        if z2.dtype == torch.bfloat16 and C % 8 == 0:
            # S rides the weight-gradient GEMM as its ones-row at every width here: at Cin = 64 / 128 / 256 (where dense_wgrad runs a separate
            # column-sum pass) that measured 90 / 102 / 41 us against 93 / 142 / 60 us for the Xception shapes of a 16 x 512^2 batch
            K.gemm(z2, dv2, G, C, Cout, rows, lda=C, ldb=Cout, ldd=Cout, a_kcontig=0, b_kcontig=0, accumulate=False, colsum_out=S,
                   colsum_accumulate=False)
        else:
            K.dense_wgrad(z2, dv2, G, accumulate=False, bias_grad=S)
        # this launch books the replica's own dgamma / dbeta whether or not the sums are exchanged: _bn_exchange_sums gets no layers
        sums = K.sepconv_fold_bwd(G, S, pwk.data.reshape(C, Cout), mean, rstd, gamma.data, beta.data, dW=_param_grad(pwk, C, Cout),
                                  dgamma=_param_grad(gamma), dbeta=_param_grad(beta))
        dist.grads_ready(pwk, gamma, beta)
        sums, world, _ = _bn_exchange_sums(sums, (), ctx.sync)
        D = K.dense_dgrad(dv2, Wn).reshape(z.shape)
        dw = _grad(dwk).reshape(9, C) if dwk.requires_grad else torch.zeros((9, C), dtype=torch.float32, device=dv.device)
        dx = K.bnfold_dwconv3_relu_bwd(D, z, xc, dwk.data.reshape(9, C), mean, rstd, gamma.data, sums, 1.0 / (rows * world) if ctx.training else 0.0,
                                       ctx.training, dw, ctx.stride, ctx.dil)
        dist.grads_ready(dwk)
        return (dx,) + (None,) * 12


def sepconv_fused_enabled():
    """ISEG_SEPCONV_FUSED=0 routes the Xception separable unit through the composed operators (the A/B baseline)"""
    return os.environ.get("ISEG_SEPCONV_FUSED", "1") != "0"


def sepconv_supported(x, dw_kernel, bn, pw_kernel, strides=1, dilation=1):
    """the shape rules of csrc/sepconv.hip, and _aligned16 of x and the vectors and kernels it reads directly"""
    N, H, W, C = x.shape
    if tuple(dw_kernel.shape) != (3, 3, C, 1) or pw_kernel.shape[-2] != C or pw_kernel.dim() != 4 or tuple(pw_kernel.shape[:2]) != (1, 1):
        return False
    if not _aligned16((x,), (dw_kernel, pw_kernel, bn.gamma, bn.beta, bn.moving_mean, bn.moving_variance)):
        return False
    return K.sepconv_supported(N, H, W, C, int(strides), int(dilation), x.dtype)


def sepconv_unit(x, dw_kernel, bn, pw_kernel, training, strides=1, dilation=1):
    """conv1x1(bn(depthwise_conv2d(relu(x), dw_kernel, dilation, strides)), pw_kernel) -- the pointwise output before its BN.  dw_kernel
    [3, 3, C, 1], pw_kernel [1, 1, C, Cout] (Keras kernels), bn the depthwise BatchNormalization layer (built).  Fused unless
    ISEG_SEPCONV_FUSED=0 or sepconv_supported refuses the shape or tensors; then the composed operators run."""
    _check_act_dtype(x)
    s, d = int(strides), int(dilation)
    bn_training = bool(training) and bn.trainable
    if nn.dry_run() or not sepconv_fused_enabled() or not sepconv_supported(x, dw_kernel, bn, pw_kernel, s, d):
        z = depthwise_conv2d(relu(x), dw_kernel, None, dilation=d, strides=s)
        u = batch_norm(z, bn.gamma, bn.beta, bn.moving_mean, bn.moving_variance, bn.epsilon, bn.momentum, bn_training, sync=bn.synchronized)
        return conv2d(u, pw_kernel, None, (1, 1), (1, 1), "same")
    return _SepConvFn.apply(x, dw_kernel, bn.gamma, bn.beta, pw_kernel, bn.moving_mean, bn.moving_variance, float(bn.epsilon), float(bn.momentum),
                            s, d, bn_training, bool(bn.synchronized))


# ---------------------------------------------------------------------------------------------------------
# JointPyramidUpsampling tail (layers/jpu.py:79-88): the merged map through four branches depthwise 3x3 (dilation 1, 2, 4, 8, with bias) ->
# (Sync)BN -> pointwise 1x1, as one tape node (csrc/jpu.hip for the depthwise side, the sepconv fold and the GEMMs for the rest).  x is read
# once forward; backward the four transposed depthwise convolutions are summed in registers, so no per-branch input gradient, no BN output and
# no dz is written.
# ---------------------------------------------------------------------------------------------------------
JPU_RATES = (1, 2, 4, 8)


class _JpuTailFn(Function):
    @staticmethod
    def forward(ctx, x, training, sync, layers, *params):
        """layers: per rate dict(eps, momentum, moving_mean, moving_var); params: per rate (dwk, dwb, gamma, beta, pwk), rate-major"""
        R = len(JPU_RATES)
        C = x.shape[-1]
        xc = _c(x)
        groups = [params[5 * r:5 * r + 5] for r in range(R)]
        w = torch.stack([g[0].data.reshape(9, C) for g in groups])
        bias = torch.stack([g[1].data for g in groups])
        z, packed = K.jpu_dwconv3x4_stats(xc, w, bias, stats=training)
        if training and sync:
            dist.all_reduce_sum(packed)          # the four [2C+1] messages, written by the depthwise launch itself, travel as one
        need_grad = any(ctx.needs_input_grad)
        vs, saved = [], []
        for r, (L, (dwk, dwb, gamma, beta, pwk)) in enumerate(zip(layers, groups)):
            if training:
                mean, rstd = K.bn_finalize(packed[r], C, L["eps"], L["momentum"], L["moving_mean"], L["moving_var"])
            else:
                mean, rstd = _bn_frozen_stats(L["moving_mean"], L["moving_var"], L["eps"])
            v, Wn = _sepconv_pointwise(z[r].reshape(-1, C), pwk, mean, rstd, gamma, beta, need_grad)
            vs.append(v.reshape(*x.shape[:-1], pwk.shape[-1]))
            saved += [mean, rstd, Wn]
        ctx.groups, ctx.training, ctx.sync = groups, training, training and sync
        ctx.save_for_backward(xc, z, w, *saved)
        return tuple(vs)

    @staticmethod
    def backward(ctx, *dvs):
        """per rate: wgrad GEMM + colsum -> fold_bwd; ONE exchange of the four [2C] sums; per rate the dgrad GEMM into one [4][N,H,W,C]
        buffer; one depthwise / BN backward launch for all four"""
        xc, z, w = ctx.saved_tensors[:3]
        rest = ctx.saved_tensors[3:]
        R = len(JPU_RATES)
        C = xc.shape[-1]
        rows = xc.numel() // C
        dev = xc.device
        sums = torch.empty((R, 2 * C), dtype=torch.float32, device=dev)
        dv2s = []
        for r, (dwk, dwb, gamma, beta, pwk) in enumerate(ctx.groups):
            mean, rstd, Wn = rest[3 * r:3 * r + 3]
            Cout = pwk.shape[-1]
            dv = dvs[r]
            dv2 = _c(dv).reshape(-1, Cout) if dv is not None else torch.zeros((rows, Cout), dtype=xc.dtype, device=dev)
            dv2s.append(dv2)
            z2 = z[r].reshape(-1, C)
            G = torch.empty((C, Cout), dtype=torch.float32, device=dev)
            S = torch.empty(Cout, dtype=torch.float32, device=dev)
            if z2.dtype == torch.bfloat16 and C % 8 == 0:
                K.gemm(z2, dv2, G, C, Cout, rows, lda=C, ldb=Cout, ldd=Cout, a_kcontig=0, b_kcontig=0, accumulate=False, colsum_out=S,
                       colsum_accumulate=False)
            else:
                K.dense_wgrad(z2, dv2, G, accumulate=False, bias_grad=S)
            K.sepconv_fold_bwd(G, S, pwk.data.reshape(C, Cout), mean, rstd, gamma.data, beta.data, dW=_param_grad(pwk, C, Cout),
                               dgamma=_param_grad(gamma), dbeta=_param_grad(beta), out=sums[r])
            dist.grads_ready(pwk, gamma, beta)
        sums, world, _ = _bn_exchange_sums(sums.reshape(-1), (), ctx.sync)
        D = torch.empty_like(z)
        for r in range(R):
            K.dense_dgrad(dv2s[r], rest[3 * r + 2], out=D[r].reshape(rows, C))
        mean = torch.stack([rest[3 * r] for r in range(R)])
        rstd = torch.stack([rest[3 * r + 1] for r in range(R)])
        gamma = torch.stack([g[2].data for g in ctx.groups])
        dw = torch.zeros((R, 9, C), dtype=torch.float32, device=dev)
        db = torch.zeros((R, C), dtype=torch.float32, device=dev)
        dx = K.jpu_bnfold_dwconv3x4_bwd(D, z, xc, w, mean, rstd, gamma, sums, 1.0 / (rows * world) if ctx.training else 0.0, ctx.training, dw, db)
        for r, (dwk, dwb, _, _, _) in enumerate(ctx.groups):
            if dwk.requires_grad:
                K.axpby(_grad(dwk).reshape(9, C), dw[r], 1.0, 1.0, out=_grad(dwk).reshape(9, C))
            if dwb.requires_grad:
                K.axpby(_grad(dwb), db[r], 1.0, 1.0, out=_grad(dwb))
            dist.grads_ready(dwk, dwb)
        return (dx if ctx.needs_input_grad[0] else None, None, None, None) + (None,) * (5 * R)


def jpu_fused_enabled():
    """ISEG_JPU_FUSED=1 routes the JointPyramidUpsampling tail through csrc/jpu.hip.  Opt-in: at 16 x 64 x 64 x 1536 -> 512 in bf16 the fused
    forward + backward measured 7.56 ms against 6.18 ms for the composed operators (EXPERIMENTS.md), so those stay the default"""
    return os.environ.get("ISEG_JPU_FUSED", "0") == "1"


def jpu_tail_supported(x, dw_layers, bn_layers, pw_kernels):
    """the shape rules of csrc/jpu.hip, and _aligned16 of x and the vectors and kernels the fused node reads directly"""
    if x.dim() != 4 or len(dw_layers) != len(JPU_RATES):
        return False
    N, H, W, C = x.shape
    vectors = []
    for rate, dw, bn, pwk in zip(JPU_RATES, dw_layers, bn_layers, pw_kernels):
        if (dw.depthwise_kernel is None or tuple(dw.depthwise_kernel.shape) != (3, 3, C, 1) or dw.bias is None
                or tuple(dw.dilation_rate) != (rate, rate) or tuple(dw.strides) != (1, 1) or dw.padding != "same"):
            return False
        if pwk.dim() != 4 or tuple(pwk.shape[:3]) != (1, 1, C) or bn.gamma is None or bn.gamma.shape[0] != C:
            return False
        vectors += [dw.depthwise_kernel, dw.bias, pwk, bn.gamma, bn.beta, bn.moving_mean, bn.moving_variance]
    if len({bool(bn.synchronized) for bn in bn_layers}) != 1 or len({bool(bn.trainable) for bn in bn_layers}) != 1:
        return False
    if not _aligned16((x,), vectors):
        return False
    return K.jpu_supported(N, H, W, C, x.dtype)


def jpu_tail(x, dw_layers, bn_layers, pw_kernels, training):
    """[conv1x1(bn_r(depthwise_conv2d(x, dw_r, bias_r, dilation=r)), pw_r) for r in 1, 2, 4, 8]: the four pointwise outputs before their own BN.
    dw_layers: the DepthwiseConv2D layers (3x3, with bias, built), bn_layers: their BatchNormalization layers (built), pw_kernels [1, 1, C, Cout]
    (Keras kernels).  Fused with ISEG_JPU_FUSED=1 where jpu_tail_supported accepts the shape and tensors; else the composed operators run."""
    _check_act_dtype(x)
    if nn.dry_run() or not jpu_fused_enabled() or not jpu_tail_supported(x, dw_layers, bn_layers, pw_kernels):
        outs = []
        for xr, dw, bn, pwk in zip(fork(x, len(dw_layers)), dw_layers, bn_layers, pw_kernels):
            z = depthwise_conv2d(xr, dw.depthwise_kernel, dw.bias, dilation=dw.dilation_rate[0])
            u = batch_norm(z, bn.gamma, bn.beta, bn.moving_mean, bn.moving_variance, bn.epsilon, bn.momentum, bool(training) and bn.trainable,
                           sync=bn.synchronized)
            outs.append(conv2d(u, pwk, None, (1, 1), (1, 1), "same"))
        return outs
    bn_training = bool(training) and bn_layers[0].trainable
    layers = [dict(eps=float(b.epsilon), momentum=float(b.momentum), moving_mean=b.moving_mean, moving_var=b.moving_variance) for b in bn_layers]
    params = [p for dw, bn, pwk in zip(dw_layers, bn_layers, pw_kernels) for p in (dw.depthwise_kernel, dw.bias, bn.gamma, bn.beta, pwk)]
    return list(_JpuTailFn.apply(x, bn_training, bool(bn_layers[0].synchronized), layers, *params))


# ---------------------------------------------------------------------------------------------------------
# ResNet-9 / 10 / 18 basic-block tail (backbones/resnet_blocks_small.py:84-119): relu(bn2(z2) + avg_pool_s(bn0(z0) or x)) as one tape node
# (csrc/resblock.hip).  Neither BN output nor the pooled shortcut is written; both layers' statistics travel in one message each way.
# ---------------------------------------------------------------------------------------------------------
class _ResBlockTailFn(Function):
    @staticmethod
    def forward(ctx, z2, sc, gamma2, beta2, gamma0, beta0, moving2, moving0, eps, momentum, stride, training, sync):
        C = z2.shape[-1]
        z2c, scc = _c(z2), _c(sc)
        bn0 = gamma0 is not None
        x2s = [z2c.reshape(-1, C)] + ([scc.reshape(-1, C)] if bn0 else [])
        moving = (moving2, moving0)
        if training:
            stats = [K.bn_finalize(packed, C, eps[i], momentum[i], *moving[i]) for i, packed in enumerate(_bn_batch_stats(x2s, sync))]
        else:
            stats = [_bn_frozen_stats(*moving[i], eps[i]) for i in range(len(x2s))]
        (mean2, rstd2), (mean0, rstd0) = stats[0], stats[1] if bn0 else (None, None)
        out = K.resblock_tail_fwd(z2c, mean2, rstd2, gamma2.data, beta2.data, scc, stride,
                                  (mean0, rstd0, gamma0.data, beta0.data) if bn0 else None)
        ctx.params, ctx.training, ctx.sync = (gamma2, beta2, gamma0, beta0), training, training and sync
        ctx.stride, ctx.sc_shape, ctx.rows = stride, tuple(sc.shape), (z2c.numel() // C, scc.numel() // C)
        ctx.save_for_backward(out, z2c, scc if bn0 else None, mean2, rstd2, mean0, rstd0)
        return out

    @staticmethod
    def backward(ctx, dout):
        """reduce -> (all-reduce of both layers' [2C] sums in one message) -> apply"""
        out, z2, z0, mean2, rstd2, mean0, rstd0 = ctx.saved_tensors
        gamma2, beta2, gamma0, beta0 = ctx.params
        bn0 = z0 is not None
        dO = _c(dout)
        sums = K.resblock_tail_bwd_reduce(dO, out, z2, mean2, rstd2, ctx.sc_shape, ctx.stride, z0, mean0, rstd0)
        sums, world, own = _bn_exchange_sums(sums, [(gamma2, beta2)] + ([(gamma0, beta0)] if bn0 else []), ctx.sync)
        booked = dict(dgamma2=_param_grad(gamma2), dbeta2=_param_grad(beta2), dgamma0=_param_grad(gamma0), dbeta0=_param_grad(beta0)) if own else {}
        inv_n2, inv_n0 = [1.0 / (r * world) if ctx.training else 0.0 for r in ctx.rows]
        dz2, dsc = K.resblock_tail_bwd_apply(dO, out, z2, mean2, rstd2, gamma2.data, sums, inv_n2, inv_n0, ctx.training, ctx.sc_shape, ctx.stride,
                                             z0, mean0, rstd0, gamma0.data if bn0 else None, **booked)
        if own:
            dist.grads_ready(gamma2, beta2, gamma0, beta0)
        return (dz2, dsc if ctx.needs_input_grad[1] else None) + (None,) * 11


def resblock_fused_enabled():
    """ISEG_RESBLOCK_FUSED=0 routes the ResNet-9 / 10 / 18 block tail through the composed operators (the A/B baseline)"""
    return os.environ.get("ISEG_RESBLOCK_FUSED", "1") != "0"


def resblock_tail_supported(z2, sc, bn2, bn0=None, strides=1):
    """the shape rules of csrc/resblock.hip, and _aligned16 of z2 / sc and the per-channel vectors it reads directly"""
    sh, sw = (strides, strides) if isinstance(strides, int) else tuple(strides)
    if sh != sw or sh not in (1, 2) or z2.dim() != 4 or sc.dim() != 4 or z2.dtype != sc.dtype:
        return False
    N, H, W, C = sc.shape
    if tuple(z2.shape) != (N, -(-H // sh), -(-W // sh), C):
        return False
    layers = (bn2,) if bn0 is None else (bn2, bn0)
    if not _aligned16((z2, sc), [v for b in layers for v in (b.gamma, b.beta, b.moving_mean, b.moving_variance)]):
        return False
    return K.resblock_tail_supported(C, sh, z2.dtype)


def resblock_tail(z2, bn2, sc, bn0, strides, training):
    """relu(bn2(z2) + avg_pool2d(sc', strides, strides, "same")), sc' = bn0(sc) (bn0 a BatchNormalization layer) or sc (bn0 None): the tail
    of BlockType2Small.  Fused unless ISEG_RESBLOCK_FUSED=0, the two layers differ in mode or synchronisation, or resblock_tail_supported
    refuses the shapes or tensors; then the composed operators run."""
    _check_act_dtype(z2)
    st = (strides, strides) if isinstance(strides, int) else tuple(strides)
    layers = (bn2,) if bn0 is None else (bn2, bn0)
    for b in layers:
        if not b.built:
            b.build(tuple((z2 if b is bn2 else sc).shape))
    modes = {bool(training) and b.trainable for b in layers}
    syncs = {bool(b.synchronized) for b in layers}
    if (nn.dry_run() or not resblock_fused_enabled() or len(modes) > 1 or len(syncs) > 1
            or not resblock_tail_supported(z2, sc, bn2, bn0, st)):
        if bn0 is not None:
            sc = bn0(sc, training=training)
        if st[0] > 1 or st[1] > 1:
            sc = avg_pool2d(sc, st, st, "same")
        return add_relu(sc, bn2(z2, training=training))
    eps = (float(bn2.epsilon), float(bn0.epsilon) if bn0 is not None else 0.0)
    momentum = (float(bn2.momentum), float(bn0.momentum) if bn0 is not None else 0.0)
    moving2 = (bn2.moving_mean, bn2.moving_variance)
    moving0 = (bn0.moving_mean, bn0.moving_variance) if bn0 is not None else (None, None)
    g0, b0 = (bn0.gamma, bn0.beta) if bn0 is not None else (None, None)
    return _ResBlockTailFn.apply(z2, sc, bn2.gamma, bn2.beta, g0, b0, moving2, moving0, eps, momentum, st[0], modes.pop(), syncs.pop())


# ---------------------------------------------------------------------------------------------------------
# activations, add, dropout, drop-path
# ---------------------------------------------------------------------------------------------------------
class _ActFn(Function):
    @staticmethod
    def forward(ctx, x, act):
        xc = _c(x)
        y = K.act_fwd(xc, act)
        ctx.act = act
        ctx.save_for_backward(y if act == K.ACT_RELU else xc)
        return y

    @staticmethod
    def backward(ctx, dy):
        (aux,) = ctx.saved_tensors
        return K.act_bwd(_c(dy), aux, ctx.act), None


def relu(x):
    if nn.dry_run():
        return _dry(x.shape, x)
    return _ActFn.apply(x, K.ACT_RELU)


def gelu(x):
    if nn.dry_run():
        return _dry(x.shape, x)
    return _ActFn.apply(x, K.ACT_GELU)


def sigmoid(x):
    """tf.nn.sigmoid (layers/nasfpn.py:304-311) through the C-ABI activation kernel"""
    if nn.dry_run():
        return _dry(x.shape, x)
    return _ActFn.apply(x, K.ACT_SIGMOID)


def swish(x):
    """tf.nn.silu / keras.activations.swish: x * sigmoid(x) (backbones/eva/swiglu.py:13, layers/nasfpn.py:289)"""
    if nn.dry_run():
        return _dry(x.shape, x)
    return _ActFn.apply(x, K.ACT_SWISH)


class _Relu6Fn(Function):
    @staticmethod
    def forward(ctx, x):
        xc = _c(x)
        ctx.save_for_backward(xc)
        return K.clip_fwd(xc, 0.0, 6.0)

    @staticmethod
    def backward(ctx, dy):
        (xc,) = ctx.saved_tensors
        return K.clip_bwd(xc, _c(dy), 0.0, 6.0)


def relu6(x):
    """tf.nn.relu6 (backbones/mobilenetv2_common.py:50,61,161,168) = clip to [0, 6]; the gradient passes inside the interval (TF's Relu6Grad is
    strict at the two end points, the clip gradient is not: a difference on a set of measure zero)"""
    _check_act_dtype(x)
    if nn.dry_run():
        return _dry(x.shape, x)
    return _Relu6Fn.apply(x)


class _AddFn(Function):
    @staticmethod
    def forward(ctx, a, b):
        return K.axpby(_c(a), _c(b), 1.0, 1.0)

    @staticmethod
    def backward(ctx, dy):
        return dy, dy


def add(a, b):
    if nn.dry_run():
        return _dry(a.shape, a)
    return _AddFn.apply(a, b)


class _ForkFn(Function):
    """One tensor, several consumers.  torch.autograd would add the consumers' gradients with its own elementwise kernels; here every
    consumer gets an alias, and the backward node sums the arriving gradients with iseg_axpby -- no ATen arithmetic on the step."""

    @staticmethod
    def forward(ctx, x, n):
        # an alias nobody differentiates through must arrive as None, not as a tensor of zeros the engine fills with an ATen kernel and this node
        # then adds (Swin-T + FPN: two such maps of 100 MB and 25 MB per step)
        ctx.set_materialize_grads(False)
        return tuple(x.view_as(x) for _ in range(n))

    @staticmethod
    def backward(ctx, *grads):
        live = [_c(g) for g in grads if g is not None]
        if not live:
            return None, None
        total = live[0]
        for i, g in enumerate(live[1:]):
            if g.dtype != total.dtype:
                g = K.cast(g, total.dtype)
            total = K.axpby(total, g, 1.0, 1.0, out=(total if i > 0 else None))      # the first sum allocates, the rest accumulate in place
        return total, None


def fork(x, n=2):
    """n aliases of x, one per consumer (see _ForkFn); a no-op outside autograd"""
    if nn.dry_run() or n <= 1 or not (torch.is_tensor(x) and x.requires_grad and torch.is_grad_enabled()):
        return (x,) * n
    return _ForkFn.apply(x, n)


_RNG_COUNTER = [0]


def next_seed():
    """one stream per (global seed, data-parallel rank, draw): replicas must not share dropout / drop-path masks on their shards"""
    _RNG_COUNTER[0] += 1
    return (nn.seed() * 0x9E3779B97F4A7C15 + _RNG_COUNTER[0] * 0xD1B54A32D192ED03 + dist.rank() * 0xA24BAED4963EE407) & 0xFFFFFFFFFFFFFFFF


class _DropoutFn(Function):
    @staticmethod
    def forward(ctx, x, rate, seed):
        ctx.rate, ctx.seed = rate, seed
        return K.dropout(_c(x), rate, seed)

    @staticmethod
    def backward(ctx, dy):
        return K.dropout(_c(dy), ctx.rate, ctx.seed), None, None


def dropout(x, rate, training):
    if not training or rate <= 0:
        return x
    return _DropoutFn.apply(x, float(rate), next_seed())


class _RowScaleFn(Function):
    @staticmethod
    def forward(ctx, x, s):
        C = x.shape[-1]
        rpg = x.numel() // C // x.shape[0]
        ctx.rpg = rpg
        ctx.save_for_backward(s)
        return K.rowscale(_c(x).reshape(-1, C), s, rpg).reshape(x.shape)

    @staticmethod
    def backward(ctx, dy):
        (s,) = ctx.saved_tensors
        C = dy.shape[-1]
        return K.rowscale(_c(dy).reshape(-1, C), s, ctx.rpg).reshape(dy.shape), None


class _DropPathPool:
    """The drop-path call sites of a training step draw from ONE launch: the first step with a given sample count records the
    (samples, keep probability) sequence, every later step with that sample count replays it -- one [P, n] tensor of factors, rows handed
    out in call order.  Plans are kept PER SAMPLE COUNT (round 4): a smaller last batch, or a second crop size of a graphed trainer, no longer
    throws the plan away -- which had made the step after every switch draw one seed per call site instead of one per step, i.e. made the
    random stream depend on the order of batch shapes (and a replayed graph, which froze the pooled form, disagree with the eager run).  A step
    whose sequence differs from its plan (eval in between, a changed model) falls back to one launch per call and re-records."""

    def __init__(self):
        self.active, self.plans, self.rec, self.masks, self.cursor, self.keeps, self.plan = False, {}, None, None, 0, {}, None

    def begin(self):
        if self.rec:      # file the previous step's sequence under its sample count
            counts = {q[0] for q in self.rec}
            if len(counts) == 1:
                n = next(iter(counts))
                if self.plans.get(n) != self.rec:
                    self.plans[n] = list(self.rec)
                    self.keeps.pop(n, None)
        self.active, self.rec, self.cursor, self.masks, self.plan = True, [], 0, None, None

    def end(self):
        self.active = False

    def take(self, n, keep, device):
        keep = float(keep)
        if not self.active:
            return K.drop_path_mask(n, keep, next_seed(), device)
        self.rec.append((n, keep))
        k = self.cursor
        if k == 0 and self.masks is None and len(self.rec) == 1:
            self.plan = self.plans.get(n)
        plan = self.plan
        if plan is not None and k < len(plan) and plan[k] == (n, keep):
            if self.masks is None:
                keeps = self.keeps.get(n)
                if keeps is None or keeps.device != device:
                    keeps = self.keeps[n] = torch.tensor([q[1] for q in plan], dtype=torch.float32, device=device)
                self.masks = K.drop_path_masks(keeps, n, next_seed())
            self.cursor = k + 1
            return self.masks[k]
        self.plan = None      # the sequence differs from the plan: individual launches until the next step has re-recorded it
        return K.drop_path_mask(n, keep, next_seed(), device)


_DROP_PATH_POOL = _DropPathPool()


class drop_path_pool:
    """with F.drop_path_pool(): one training step's forward (CoreTrain's step uses it)"""

    def __enter__(self):
        _DROP_PATH_POOL.begin()

    def __exit__(self, *a):
        _DROP_PATH_POOL.end()


def drop_path_factors(n, keep_prob, device):
    """per-sample factors floor(keep + u) / keep (utils/drops.py:14-20) for one call site"""
    return _DROP_PATH_POOL.take(int(n), keep_prob, device)


def drop_path(x, drop_prob, training, mask=None):
    """utils/drops.py:8-22.  `mask` (per-sample factors floor(keep+u)/keep) can be injected for parity tests."""
    if (not training) or drop_prob == 0.0:
        return x
    if mask is None:
        mask = drop_path_factors(x.shape[0], 1.0 - drop_prob, x.device)
    return _RowScaleFn.apply(x, mask)


# ---------------------------------------------------------------------------------------------------------
# resize, pooling, broadcast, concat
# ---------------------------------------------------------------------------------------------------------
class _ResizeBilinearFn(Function):
    @staticmethod
    def forward(ctx, x, Ho, Wo, out_dtype, align_corners=False):
        ctx.in_shape, ctx.in_dtype, ctx.align = x.shape, x.dtype, bool(align_corners)
        return K.resize_bilinear(_c(x), Ho, Wo, out_dtype=out_dtype, align_corners=ctx.align)

    @staticmethod
    def backward(ctx, dy):
        _, Hi, Wi, _ = ctx.in_shape
        return K.resize_bilinear_bwd(_c(dy), Hi, Wi, ctx.in_dtype, align_corners=ctx.align), None, None, None, None


def resize_bilinear(x, size, out_dtype=None, align_corners=False):
    """tf.image.resize(method="bilinear") (half-pixel centres); align_corners=True: tf.compat.v1.image.resize(..., align_corners=True)"""
    Ho, Wo = int(size[0]), int(size[1])
    if nn.dry_run():
        return _dry((x.shape[0], Ho, Wo, x.shape[3]), x, out_dtype)
    if x.shape[1] == Ho and x.shape[2] == Wo and (out_dtype is None or out_dtype == x.dtype):
        return x
    return _ResizeBilinearFn.apply(x, Ho, Wo, out_dtype or x.dtype, bool(align_corners))


class _GlobalAvgPoolFn(Function):
    @staticmethod
    def forward(ctx, x):
        N, H, W, C = x.shape
        xc = _c(x)
        out = torch.empty((N, C), dtype=torch.float32, device=x.device)
        K.colsum(xc, C, H * W * C, N, H * W, C, out, scale=1.0 / (H * W))
        ctx.shape = x.shape
        return K.cast(out, x.dtype).reshape(N, 1, 1, C)

    @staticmethod
    def backward(ctx, dy):
        N, H, W, C = ctx.shape
        dx = torch.empty(ctx.shape, dtype=dy.dtype, device=dy.device)
        K.broadcast_rows(_c(dy).reshape(N, C), dx, C, H * W * C, N, H * W, C, scale=1.0 / (H * W))
        return dx


def global_avg_pool(x):
    """tf.reduce_mean(x, axis=(1,2), keepdims=True)"""
    if nn.dry_run():
        return _dry((x.shape[0], 1, 1, x.shape[3]), x)
    return _GlobalAvgPoolFn.apply(x)


class _BroadcastHWFn(Function):
    @staticmethod
    def forward(ctx, v, H, W):
        N, _, _, C = v.shape
        y = torch.empty((N, H, W, C), dtype=v.dtype, device=v.device)
        K.broadcast_rows(_c(v).reshape(N, C), y, C, H * W * C, N, H * W, C)
        ctx.hw = (H, W)
        return y

    @staticmethod
    def backward(ctx, dy):
        N, H, W, C = dy.shape
        out = torch.empty((N, C), dtype=torch.float32, device=dy.device)
        dy2, lddy = _rows2d(dy)
        K.colsum(dy2, lddy, H * W * lddy, N, H * W, C, out)
        return K.cast(out, dy.dtype).reshape(N, 1, 1, C), None, None


def broadcast_hw(v, H, W):
    """tf.ones([1,H,W,1]) * v for v [N,1,1,C] (layers/model_builder.py:268)"""
    if nn.dry_run():
        return _dry((v.shape[0], H, W, v.shape[3]), v)
    return _BroadcastHWFn.apply(v, int(H), int(W))


class _ConcatFn(Function):
    @staticmethod
    def forward(ctx, *xs):
        lead = xs[0].shape[:-1]
        widths = [x.shape[-1] for x in xs]
        total = sum(widths)
        rows = xs[0].numel() // widths[0]
        y = torch.empty((*lead, total), dtype=xs[0].dtype, device=xs[0].device)
        y2 = y.reshape(rows, total)
        off = 0
        for x, wd in zip(xs, widths):
            K.copy2d(_c(x).reshape(rows, wd), wd, y2[:, off:off + wd], total, rows, wd)
            off += wd
        ctx.widths = widths
        return y

    @staticmethod
    def backward(ctx, dy):
        outs, off = [], 0
        for wd in ctx.widths:
            outs.append(dy[..., off:off + wd])   # strided views; consumers make them contiguous only if they must
            off += wd
        return tuple(outs)


def concat(xs):
    """tf.concat(xs, axis=-1)"""
    if nn.dry_run():
        return _dry((*xs[0].shape[:-1], sum(x.shape[-1] for x in xs)), xs[0])
    return _ConcatFn.apply(*xs)


# ---------------------------------------------------------------------------------------------------------
# ConvNeXt block, fused:  x + drop_path(gamma * pw2(gelu(pw1(LN(dw7x7(x))))))     backbones/convnext.py:47-63
# ---------------------------------------------------------------------------------------------------------
class _ConvNeXtBlockFn(Function):
    @staticmethod
    def forward(ctx, x, dw_kernel, dw_bias, ln_gamma, ln_beta, w1, b1, w2, b2, gamma, dil, eps, dp_mask):
        import types

        p = types.SimpleNamespace(dw_kernel=dw_kernel, dw_bias=dw_bias, ln_gamma=ln_gamma, ln_beta=ln_beta, w1=w1, b1=b1, w2=w2,
                                  b2=b2, gamma=gamma)
        N, H, W, C = x.shape
        xc = _c(x)
        Kk = p.dw_kernel.shape[0]
        pad = (Kk - 1) * dil // 2
        y1 = K.dwconv2d(xc, p.dw_kernel.data.reshape(Kk * Kk, C), p.dw_bias.data, Kk, dil, pad, pad)
        M = N * H * W
        ctx.fused = K.convnext_mlp_supported(C, xc.dtype)
        # round 3: on the fused stages LayerNorm rides the MLP kernels' row loads (forward: statistics + normalisation, backward: normalisation
        # from the saved statistics), so y2 is never written or read -- needs the backward route that keeps nothing [M, 4C]-shaped either, which
        # takes a drop-path mask only when H * W is a multiple of 64
        ctx.ln_on_load = ctx.fused and (dp_mask is None or (H * W) % 64 == 0)
        if ctx.ln_on_load:
            y2 = mean = rstd = None
        else:
            y2, mean, rstd = K.layernorm_fwd(y1.reshape(M, C), p.ln_gamma.data, p.ln_beta.data, eps)
        grad = any(ctx.needs_input_grad)          # grad mode is off inside Function.forward; this is the tape's view
        # measured on MI355X (tools/kbench_gemm.py): writing both h and g = gelu(h) from the pw1 epilogue (175+83+117 us at
        # stage 0 for pw1/pw2/wgrad2) beats writing h only and re-deriving gelu(h) while staging the A operand of pw2 and of
        # the pw2 weight gradient (83+147+185 us): the transform sits on the load->LDS critical path.  a_act stays available.
        # h holds gelu'(pre-activation), not the pre-activation: the pw1 epilogue has Phi and exp(-v^2/2) in hand for gelu anyway, and
        # the backward epilogue then costs one multiply instead of an erf per element (+50 us of VALU per 100 M elements, measured)
        gam = p.gamma.data if p.gamma is not None else None
        if ctx.fused:
            # wide stages (C = 96 / 192, bf16): the [M, 4C] hidden tile stays on the CU (csrc/mlp_fused.hip) and the backward pass
            # recomputes it, so nothing [M, 4C]-shaped is kept; `bw` holds the tiled weight images the backward chain streams
            fw, bw = nn.mlp_tiled(p.w1, p.w2, p.gamma)      # one launch per weight update for every block of the model
            if ctx.ln_on_load:
                out, mean, rstd = K.convnext_mlp_fwd_ln(y1.reshape(M, C), p.ln_gamma.data, p.ln_beta.data, eps, fw, p.b1.data, p.b2.data, gam,
                                                        dp_mask, H * W, xc.reshape(M, C))
            else:
                out = K.convnext_mlp_fwd(y2, fw, p.b1.data, p.b2.data, gam, dp_mask, H * W, xc.reshape(M, C))
            h, g = bw, None
        else:
            h = torch.empty((M, 4 * C), dtype=xc.dtype, device=xc.device) if grad else None
            w1t, w2t = (nn.wt(p.w1), nn.wt(p.w2)) if xc.dtype == torch.bfloat16 else (None, None)
            if w1t is not None and w2t is not None:
                # K-contiguous kernel copies: the forward products run on the LDS-DMA GEMM like the data gradients (256 x 128 tiles)
                g = K.dense_fwd_t(y2, w1t, p.b1.data, act=K.ACT_GELU, pre_out=h, pre_deriv=grad)
                out = K.dense_fwd_t(g, w2t, p.b2.data, colscale=gam, rowscale=dp_mask, rows_per_group=H * W, residual=xc.reshape(M, C))
            else:
                g = K.dense_fwd(y2, nn.w(p.w1), p.b1.data, act=K.ACT_GELU, pre_out=h, pre_deriv=grad)
                out = K.dense_fwd(g, nn.w(p.w2), p.b2.data, colscale=gam, rowscale=dp_mask, rows_per_group=H * W, residual=xc.reshape(M, C))
        ctx.p, ctx.dil, ctx.pad = p, dil, pad
        ctx.save_for_backward(xc, y1, y2, mean, rstd, h, g if grad else None, dp_mask)
        return out.reshape(N, H, W, C)

    @staticmethod
    def backward(ctx, dout):
        """The data-gradient chain (dbr -> dh -> dy2 -> LayerNorm -> depthwise data gradient) and the parameter gradients (column sums, the
        weight-gradient products, layer-scale gradients, the depthwise weight gradient) all run on the current stream; the gradients are
        announced to the reducer once the block's last kernel is enqueued."""
        xc, y1, y2, mean, rstd, h, g, dp_mask = ctx.saved_tensors
        p, dil, pad = ctx.p, ctx.dil, ctx.pad
        N, H, W, C = xc.shape
        M = N * H * W
        Kk = p.dw_kernel.shape[0]
        do2 = _c(dout).reshape(M, C)
        cdt = xc.dtype
        if ctx.ln_on_load:
            ln = (mean, rstd, p.ln_gamma.data, p.ln_beta.data)
            dy1 = _LnMlpResidualFn.mlp_ln_backward(y1.reshape(M, C), do2, h, ln, (p.ln_gamma, p.ln_beta, p.w1, p.b1, p.w2, p.b2, p.gamma), dp_mask,
                                                    H * W)
            del h
        else:
            dy2 = _ConvNeXtBlockFn._mlp_backward_with_hidden(ctx, p, do2, y2, h, g, dp_mask, H, W, C, M, cdt, xc)
            del h, g
            dy1 = K.layernorm_bwd(dy2, y1.reshape(M, C), p.ln_gamma.data, mean, rstd, _grad_out(p.ln_gamma), _grad_out(p.ln_beta))
        dy1 = dy1.reshape(N, H, W, C)
        if p.dw_kernel.requires_grad or p.dw_bias.requires_grad:
            K.dwconv2d_bwd_weight(xc, dy1, _grad_out(p.dw_kernel, Kk * Kk, C), _grad_out(p.dw_bias), Kk, dil, pad, pad)
        dx = None
        if ctx.needs_input_grad[0]:
            padb = (Kk - 1) * dil - pad
            dx = K.dwconv2d(dy1, p.dw_kernel.data.reshape(Kk * Kk, C), None, Kk, dil, padb, padb, flip=True, add=_c(dout))
        dist.grads_ready(p.dw_kernel, p.dw_bias, p.ln_gamma, p.ln_beta, p.w1, p.b1, p.w2, p.b2, p.gamma)
        return (dx,) + (None,) * 12

    @staticmethod
    def _mlp_backward_with_hidden(ctx, p, do2, y2, h, g, dp_mask, H, W, C, M, cdt, xc):
        """the round-2 route: g / dh materialised ([M, 4C] each), two weight-gradient products; the path of the un-fused stages (C >= 384),
        and of the fused stages when a drop-path mask meets a plane that is not a multiple of 64 pixels"""
        dbr = K.rowscale(do2, dp_mask, H * W) if dp_mask is not None else do2
        S = torch.empty(C, dtype=torch.float32, device=xc.device)      # column sums of dbr (layer-scale and bias gradients)
        s_on_gemm = p.gamma is not None and (ctx.fused or g is not None) and xc.dtype == torch.bfloat16 and 4 * C >= 768      # rides Z = g^T dbr below
        if not s_on_gemm:
            K.colsum(dbr, C, 0, 1, M, C, S)
        dy2 = None
        if ctx.fused:
            # h is the tiled weight buffer here: g = gelu(pre), dh = (dbr @ (W2 gamma)^T) * gelu'(pre), dy2 = dh @ W1^T in one launch
            g, dh, dy2 = K.convnext_mlp_bwd(y2, dbr, h, p.b1.data)
        else:
            if p.gamma is None:
                w2eff = nn.w(p.w2)
            elif cdt == torch.bfloat16:
                w2eff = nn.w_colscaled(p.w2, p.gamma)
            else:
                w2eff = K.scale_cols_cast(p.w2.data, p.gamma.data, cdt)
            dh = K.dense_dgrad(dbr, w2eff, act=K.ACT_MUL_AUX, aux=h)          # [M,4C] = (dbr @ W2g^T) * gelu'(pre), h = gelu'(pre)
        del h

        # pw2 + layer scale from Z = g^T dbr and S = colsum(dbr) (no pass over [M,C] for gamma), then dW1 (+ db1)
        pair = None
        if p.gamma is not None:
            if s_on_gemm and p.b1 is not None:
                # round 5: both weight-gradient products of the block as ONE launch (36 tiles x 7 splits instead of 2 x 18 x 13): Z stops at its
                # slabs for the layer-scale kernel; round 6: the slab sum of dW1 / db1 rides the layer-scale launch too
                pair = K.dense_wgrad_pair(g, dbr, y2, dh, _grad_out(p.w1), _grad_out(p.b1), defer_second=True)
            sl = pair if pair is not None else (K.dense_wgrad_slabs(g, dbr) if s_on_gemm else None)
            if sl is not None:      # the layer-scale kernel sums the split-K slabs of Z (and its ones-row S) while it reads them
                K.layerscale_grads_slabs(sl[0], sl[1], p.w2.data, p.b2.data, p.gamma.data, _grad_out(p.w2), _grad_out(p.gamma), _grad_out(p.b2),
                                         extra=sl[2] if len(sl) > 2 else None)
            else:
                Z = torch.empty((4 * C, C), dtype=torch.float32, device=xc.device)
                K.dense_wgrad(g, dbr, Z, accumulate=False, bias_grad=S if s_on_gemm else None)      # Z = gelu(h)^T dbr (+ S from its ones-row)
                K.layerscale_grads(Z, p.w2.data, p.b2.data, p.gamma.data, S, _grad_out(p.w2), _grad_out(p.gamma), _grad_out(p.b2))
        else:
            if p.w2.requires_grad:
                K.dense_wgrad(g, dbr, _grad(p.w2))
            if p.b2.requires_grad:
                K.axpby(S, _grad(p.b2), 1.0, 1.0, out=_grad(p.b2))
        if pair is None:
            K.dense_wgrad(y2, dh, _grad_out(p.w1), bias_grad=_grad_out(p.b1))      # db1 rides the wgrad GEMM (virtual ones-row) when C % 128 != 0
        if not ctx.fused:
            dy2 = K.dense_dgrad(dh, nn.w(p.w1))                                # [M,C]
        return dy2


class _ConvNeXtV2BlockFn(Function):
    """One tape node for a ConvNeXt V2 block (backbones/convnext_v2.py:83-98): depthwise 7x7 -> LayerNorm -> Dense 4C -> GELU -> GRN ->
    Dense C -> drop path -> + inputs.  The first product's epilogue writes gelu(h) and gelu'(h); the second product's epilogue applies the
    drop-path row factor and adds the block input; in the backward pass the GELU derivative rides the GRN data-gradient kernel, the bias
    gradients ride the weight-gradient GEMMs and the residual gradient rides the depthwise data-gradient kernel -- no elementwise pass of
    its own for any of them."""

    @staticmethod
    def forward(ctx, x, dw_kernel, dw_bias, ln_gamma, ln_beta, w1, b1, grn_gamma, grn_beta, w2, b2, dil, eps, grn_eps, dp_mask):
        import types

        p = types.SimpleNamespace(dw_kernel=dw_kernel, dw_bias=dw_bias, ln_gamma=ln_gamma, ln_beta=ln_beta, w1=w1, b1=b1, w2=w2, b2=b2,
                                  grn_gamma=grn_gamma, grn_beta=grn_beta)
        N, H, W, C = x.shape
        xc = _c(x)
        M = N * H * W
        Kk = dw_kernel.shape[0]
        pad = (Kk - 1) * dil // 2
        y1 = K.dwconv2d(xc, dw_kernel.data.reshape(Kk * Kk, C), dw_bias.data, Kk, dil, pad, pad)
        y2, mean, rstd = K.layernorm_fwd(y1.reshape(M, C), ln_gamma.data, ln_beta.data, eps)
        grad = any(ctx.needs_input_grad)
        d = torch.empty((M, 4 * C), dtype=xc.dtype, device=xc.device) if grad else None      # gelu'(pre-activation)
        w1t, w2t = (nn.wt(w1), nn.wt(w2)) if xc.dtype == torch.bfloat16 else (None, None)
        if w1t is not None and w2t is not None:
            g = K.dense_fwd_t(y2, w1t, b1.data, act=K.ACT_GELU, pre_out=d, pre_deriv=grad)
        else:
            g = K.dense_fwd(y2, nn.w(w1), b1.data, act=K.ACT_GELU, pre_out=d, pre_deriv=grad)
        # Wide planes (at least two activation rows per kernel row and sample): the normalisation is folded into the second product --
        # per-sample kernels diag(gamma*nx_n + 1) W2 and the bias b2 + beta W2 -- so grn(g) is never written (csrc/grn.hip, "folded")
        HW = H * W
        ctx.fold = (w2t is not None and HW % 256 == 0 and HW >= 8 * C and C >= 64 and C % 16 == 0      # (the LDS-DMA GEMM's own conditions)
                    and os.environ.get("ISEG_V2_GRN_FOLD", "1") == "1")
        if ctx.fold:
            nx, gx = K.grn_stats(g.reshape(N, HW, 4 * C), grn_eps)
            w2n = K.grn_fold_weights(w2t, grn_gamma.data.reshape(-1), nx)
            bias2 = K.grn_fold_bias(w2.data.reshape(4 * C, C), grn_beta.data.reshape(-1), b2.data)
            out = torch.empty((M, C), dtype=xc.dtype, device=xc.device)
            K.gemm(g, w2n, out, M, C, 4 * C, lda=4 * C, ldb=4 * C, ldd=C, a_kcontig=1, b_kcontig=1, bias=bias2, rowscale=dp_mask,
                   rows_per_group=HW, residual=xc.reshape(M, C), ldr=C, b_group=(HW, 4 * C * C))
            z = None
        else:
            z, nx, gx = K.grn_fwd(g.reshape(N, HW, 4 * C), grn_gamma.data, grn_beta.data, grn_eps)
            z = z.reshape(M, 4 * C)
            if w1t is not None and w2t is not None:
                out = K.dense_fwd_t(z, w2t, b2.data, rowscale=dp_mask, rows_per_group=HW, residual=xc.reshape(M, C))
            else:
                out = K.dense_fwd(z, nn.w(w2), b2.data, rowscale=dp_mask, rows_per_group=HW, residual=xc.reshape(M, C))
        ctx.p, ctx.dil, ctx.pad, ctx.grn_eps = p, dil, pad, grn_eps
        if grad:
            ctx.save_for_backward(xc, y1, y2, mean, rstd, d, g, z, nx, gx, dp_mask)
        return out.reshape(N, H, W, C)

    @staticmethod
    def backward(ctx, dout):
        xc, y1, y2, mean, rstd, d, g, z, nx, gx, dp_mask = ctx.saved_tensors
        p, dil, pad = ctx.p, ctx.dil, ctx.pad
        N, H, W, C = xc.shape
        M = N * H * W
        Kk = p.dw_kernel.shape[0]
        do2 = _c(dout).reshape(M, C)
        dbr = K.rowscale(do2, dp_mask, H * W) if dp_mask is not None else do2
        HW = H * W
        if ctx.fold:
            # G = g^T dbr per sample (per row chunk where a sample alone would not fill the CUs): dW2, the GRN statistics and dbeta all come
            # from these small products -- no pass over dz for them, and no grn(g) to read
            S = K.colsum(dbr, C, 0, 1, M, C, torch.empty(C, dtype=torch.float32, device=xc.device))
            if p.b2.requires_grad:
                K.axpby(S, _grad(p.b2), 1.0, 1.0, out=_grad(p.b2))
            tiles = -(-4 * C // 128) * -(-C // 128)
            sps = 1
            while N * sps * tiles < 384 and HW % (2 * sps) == 0 and HW // (2 * sps) >= 512:
                sps *= 2
            rows = HW // sps
            slabs = torch.empty((N * sps, 4 * C, C), dtype=torch.float32, device=xc.device)
            K.gemm(g, dbr, slabs, 4 * C, C, rows, lda=4 * C, ldb=C, ldd=C, a_kcontig=0, b_kcontig=0, batch=N * sps, batch_inner=1,
                   sa=(rows * 4 * C, 0), sb=(rows * C, 0), sd=(4 * C * C, 0))
            dstats = K.grn_fold_wgrad(slabs, sps, p.w2.data.reshape(4 * C, C), p.grn_gamma.data.reshape(-1), p.grn_beta.data.reshape(-1), nx, S,
                                      _grad_out(p.w2, 4 * C, C))
            del slabs
            dz = K.dense_dgrad(dbr, nn.w(p.w2))                                       # [M, 4C]
            dh = K.grn_bwd_folded(dz.reshape(N, HW, 4 * C), g.reshape(N, HW, 4 * C), p.grn_gamma.data.reshape(-1), nx, gx, dstats,
                                  _grad_out(p.grn_gamma, -1), _grad_out(p.grn_beta, -1), ctx.grn_eps, mul=d).reshape(M, 4 * C)
        else:
            K.dense_wgrad(z, dbr, _grad_out(p.w2), bias_grad=_grad_out(p.b2))
            dz = K.dense_dgrad(dbr, nn.w(p.w2))                                       # [M, 4C]
            del z
            # GRN data gradient times gelu'(h) in one kernel; dgamma | dbeta from the same pass over dz
            dh = K.grn_bwd(dz.reshape(N, HW, 4 * C), g.reshape(N, HW, 4 * C), p.grn_gamma.data, nx, gx, _grad_out(p.grn_gamma, -1),
                           _grad_out(p.grn_beta, -1), ctx.grn_eps, mul=d).reshape(M, 4 * C)
        del dz, g, d
        K.dense_wgrad(y2, dh, _grad_out(p.w1), bias_grad=_grad_out(p.b1))
        dy2 = K.dense_dgrad(dh, nn.w(p.w1))                                            # [M, C]
        del dh
        dy1 = K.layernorm_bwd(dy2, y1.reshape(M, C), p.ln_gamma.data, mean, rstd, _grad_out(p.ln_gamma), _grad_out(p.ln_beta))
        dy1 = dy1.reshape(N, H, W, C)
        if p.dw_kernel.requires_grad or p.dw_bias.requires_grad:
            K.dwconv2d_bwd_weight(xc, dy1, _grad_out(p.dw_kernel, Kk * Kk, C), _grad_out(p.dw_bias), Kk, dil, pad, pad)
        dx = None
        if ctx.needs_input_grad[0]:
            padb = (Kk - 1) * dil - pad
            dx = K.dwconv2d(dy1, p.dw_kernel.data.reshape(Kk * Kk, C), None, Kk, dil, padb, padb, flip=True, add=_c(dout))
        dist.grads_ready(p.dw_kernel, p.dw_bias, p.ln_gamma, p.ln_beta, p.w1, p.b1, p.grn_gamma, p.grn_beta, p.w2, p.b2)
        return (dx,) + (None,) * 14


def convnext_v2_block(x, params, dilation, eps, grn_eps, dp_mask):
    _check_act_dtype(x)
    if nn.dry_run():
        return _dry(x.shape, x)
    p = params
    return _ConvNeXtV2BlockFn.apply(x, p.dw_kernel, p.dw_bias, p.ln_gamma, p.ln_beta, p.w1, p.b1, p.grn_gamma, p.grn_beta, p.w2, p.b2,
                                    int(dilation), float(eps), float(grn_eps), dp_mask)


def convnext_block(x, params, dilation, eps, dp_mask):
    _check_act_dtype(x)
    if nn.dry_run():
        return _dry(x.shape, x)
    p = params
    return _ConvNeXtBlockFn.apply(x, p.dw_kernel, p.dw_bias, p.ln_gamma, p.ln_beta, p.w1, p.b1, p.w2, p.b2, p.gamma, int(dilation),
                                  float(eps), dp_mask)


# ---------------------------------------------------------------------------------------------------------
# ignore-label softmax cross-entropy          losses/catecrossentropy_ignore_label.py:44-88
# ---------------------------------------------------------------------------------------------------------
class _SoftmaxCEPerPixelFn(Function):
    """returns the per-position loss vector [N*H*W] exactly like the reference's weighted_loss (Reduction.NONE)"""

    @staticmethod
    def forward(ctx, logits, labels, num_class, ignore_label, class_w, focal=None):
        z = _c(logits).reshape(-1, num_class)
        if z.dtype != torch.float32:
            z = K.cast(z, torch.float32)
        y = _c(labels).reshape(-1)
        if y.dtype != torch.int32:
            y = y.to(torch.int32)
        px, _, _ = K.softmax_ce_ignore(z, y, ignore_label, class_w=class_w, want_px=True, focal=focal)
        ctx.args = (num_class, ignore_label, class_w, focal)
        ctx.in_dtype, ctx.in_shape = logits.dtype, logits.shape
        ctx.save_for_backward(z, y)
        return px

    @staticmethod
    def backward(ctx, dpx):
        z, y = ctx.saved_tensors
        num_class, ignore_label, class_w, focal = ctx.args
        gp = _c(dpx)
        if gp.dtype != torch.float32:
            gp = K.cast(gp, torch.float32)
        _, _, dz = K.softmax_ce_ignore(z, y, ignore_label, class_w=class_w, want_px=False, want_grad=True, grad_scale=1.0,
                                       grad_px=gp, focal=focal)
        if dz.dtype != ctx.in_dtype:
            dz = K.cast(dz, ctx.in_dtype)
        return dz.reshape(ctx.in_shape), None, None, None, None, None


class _SoftmaxCEMeanFn(Function):
    """mean over ALL positions (Keras' reduction of the NONE loss): loss and d(loss)/d(logits) in one fused pass"""

    @staticmethod
    def forward(ctx, logits, labels, num_class, ignore_label, class_w, weight, focal=None, cm=None):
        z = _c(logits).reshape(-1, num_class)
        if z.dtype != torch.float32:
            z = K.cast(z, torch.float32)
        y = _c(labels).reshape(-1)
        if y.dtype != torch.int32:
            y = y.to(torch.int32)
        P = z.shape[0]
        want_grad = ctx.needs_input_grad[0]
        _, s, dz = K.softmax_ce_ignore(z, y, ignore_label, class_w=class_w, want_px=False, want_sum=True, sum_scale=weight / P,
                                       want_grad=want_grad, grad_scale=weight / P, focal=focal, cm=cm)
        ctx.shape, ctx.in_dtype = logits.shape, logits.dtype
        ctx.save_for_backward(dz)
        return s.reshape(())

    @staticmethod
    def backward(ctx, dloss):
        (dz,) = ctx.saved_tensors
        # dloss is the scalar chain factor.  Inside CoreTrain's step it is exactly 1 (unit_loss_grad()), otherwise it is
        # applied on the device (a host read here would stall the stream)
        if not _UNIT_LOSS_GRAD[0]:
            dz = K.scale_dev(dz, _c(dloss).reshape(1).to(torch.float32))
        if dz.dtype != ctx.in_dtype:
            dz = K.cast(dz, ctx.in_dtype)
        return dz.reshape(ctx.shape), None, None, None, None, None, None, None


_UNIT_LOSS_GRAD = [False]


class unit_loss_grad:
    """context: the caller guarantees every scalar loss is differentiated with upstream gradient exactly 1"""

    def __enter__(self):
        self.prev = _UNIT_LOSS_GRAD[0]
        _UNIT_LOSS_GRAD[0] = True

    def __exit__(self, *a):
        _UNIT_LOSS_GRAD[0] = self.prev


def softmax_ce_per_pixel(logits, labels, num_class, ignore_label, class_w=None, focal=None):
    return _SoftmaxCEPerPixelFn.apply(logits, labels, num_class, ignore_label, class_w, focal)


# ---------------------------------------------------------------------------------------------------------
# online hard example mining on the per-position loss          losses/ohem.py:11-39
# ---------------------------------------------------------------------------------------------------------
def _ohem_rows(logits, labels, num_class):
    z = _c(logits).reshape(-1, num_class)
    if z.dtype != torch.float32:
        z = K.cast(z, torch.float32)
    y = _c(labels).reshape(-1)
    if y.dtype != torch.int32:
        y = y.to(torch.int32)
    return z, y


def _ohem_check_index(min_kept_total, thresh, P):
    # sorted_loss[batch_min_kept] (:35-36) past the end is an error in the reference as well; refuse it before anything is launched
    if thresh is None and not 0 <= int(min_kept_total) < P:
        raise ValueError(f"ohem: index min_kept * batch_size = {int(min_kept_total)} of {P} sorted losses")


class _OhemSelectFn(Function):
    """loss [P] -> loss * keep.  The threshold only enters comparisons (tf.where on seg_prob < threshold, :33, or loss > threshold, :37), so the
    upstream gradient passes on kept positions and nothing reaches the logits through the probabilities"""

    @staticmethod
    def forward(ctx, loss, logits, labels, num_class, ignore_label, min_kept_total, thresh):
        lv = _c(loss).reshape(-1)
        if lv.dtype != torch.float32:
            lv = K.cast(lv, torch.float32)
        values = lv
        if thresh is not None:
            z, y = _ohem_rows(logits, labels, num_class)
            values = K.ohem_label_prob(z, y, ignore_label)
        keep, out, _, _, _ = K.ohem_select(values, lv, min_kept_total, thresh, want_loss=True)
        ctx.in_dtype, ctx.in_shape = loss.dtype, loss.shape
        ctx.save_for_backward(keep)
        return out

    @staticmethod
    def backward(ctx, dout):
        (keep,) = ctx.saved_tensors
        g = _c(dout).reshape(-1, 1)
        if g.dtype != torch.float32:
            g = K.cast(g, torch.float32)
        dl = K.scale_rows(g, keep)
        if dl.dtype != ctx.in_dtype:
            dl = K.cast(dl, ctx.in_dtype)
        return dl.reshape(ctx.in_shape), None, None, None, None, None, None


def ohem_select_per_pixel(loss, logits, labels, num_class, ignore_label, min_kept_total, thresh):
    """ohem_selector on the flattened loss [N*H*W]: labels are the integer labels under the rule of softmax_ce_per_pixel (ignore_label == 0
    shifts them, a class outside [0, num_class) is a zero row); thresh None selects on the loss itself and reads neither logits nor labels"""
    _ohem_check_index(min_kept_total, thresh, loss.numel())
    return _OhemSelectFn.apply(loss, logits, labels, int(num_class), int(ignore_label), int(min_kept_total), thresh)


class _OhemCEMeanFn(Function):
    """mean over ALL positions of the OHEM-selected loss and d(mean)/d(logits): per-position loss, probabilities, selection with the
    masked sum, then the loss kernel again with grad_px = keep -- nothing is read back"""

    @staticmethod
    def forward(ctx, logits, labels, num_class, ignore_label, class_w, weight, focal, cm, min_kept_total, thresh):
        z, y = _ohem_rows(logits, labels, num_class)
        P = z.shape[0]
        px, _, _ = K.softmax_ce_ignore(z, y, ignore_label, class_w=class_w, want_px=True, focal=focal, cm=cm)
        values = px if thresh is None else K.ohem_label_prob(z, y, ignore_label)
        keep, _, s, _, _ = K.ohem_select(values, px, min_kept_total, thresh, want_sum=True, sum_scale=weight / P)
        dz = None
        if ctx.needs_input_grad[0]:
            _, _, dz = K.softmax_ce_ignore(z, y, ignore_label, class_w=class_w, want_px=False, want_grad=True, grad_scale=weight / P,
                                           grad_px=keep, focal=focal)
        ctx.shape, ctx.in_dtype = logits.shape, logits.dtype
        ctx.save_for_backward(dz)
        return s.reshape(())

    @staticmethod
    def backward(ctx, dloss):
        (dz,) = ctx.saved_tensors
        if not _UNIT_LOSS_GRAD[0]:      # (see _SoftmaxCEMeanFn.backward)
            dz = K.scale_dev(dz, _c(dloss).reshape(1).to(torch.float32))
        if dz.dtype != ctx.in_dtype:
            dz = K.cast(dz, ctx.in_dtype)
        return dz.reshape(ctx.shape), None, None, None, None, None, None, None, None, None


def ohem_softmax_ce_mean(logits, labels, num_class, ignore_label, min_kept_total, thresh, class_w=None, weight=1.0, focal=None, cm=None):
    """softmax_ce_mean with the OHEM selection between the loss and its mean; the mean stays over ALL positions (Keras averages the
    Reduction.NONE vector, zeros included); cm as there (plain cross-entropy only)"""
    _ohem_check_index(min_kept_total, thresh, logits.numel() // int(num_class))
    return _OhemCEMeanFn.apply(logits, labels, int(num_class), int(ignore_label), class_w, float(weight), focal, cm, int(min_kept_total), thresh)


# ---------------------------------------------------------------------------------------------------------
# MaskLoss: sigmoid (focal) + dice + cross-entropy under the ignore-label mask          losses/mask_loss.py:10-201
# ---------------------------------------------------------------------------------------------------------
def _mask_loss_inputs(logits, labels):
    B, H, W, Cc = logits.shape
    z = _c(logits).reshape(B, H * W, Cc)
    if z.dtype != torch.float32:
        z = K.cast(z, torch.float32)
    y = _c(labels).reshape(B, H * W)
    if y.dtype != torch.int32:
        y = y.to(torch.int32)
    return z, y


class _MaskLossPerPixelFn(Function):
    """the masked per-pixel loss [B, H*W] (Keras reduction none); the backward takes the per-pixel upstream gradient through both passes"""

    @staticmethod
    def forward(ctx, logits, labels, ignore_label, flags, coefs):
        z, y = _mask_loss_inputs(logits, labels)
        px, _, _ = K.mask_loss(z, y, ignore_label, flags, coefs, want_px=True)
        ctx.args = (ignore_label, flags, coefs)
        ctx.in_dtype, ctx.in_shape = logits.dtype, logits.shape
        ctx.save_for_backward(z, y)
        return px.reshape(z.shape[0], z.shape[1])

    @staticmethod
    def backward(ctx, dpx):
        z, y = ctx.saved_tensors
        ignore_label, flags, coefs = ctx.args
        gp = _c(dpx).reshape(-1)
        if gp.dtype != torch.float32:
            gp = K.cast(gp, torch.float32)
        _, _, dz = K.mask_loss(z, y, ignore_label, flags, coefs, want_grad=True, grad_scale=1.0, grad_px=gp)
        if dz.dtype != ctx.in_dtype:
            dz = K.cast(dz, ctx.in_dtype)
        return dz.reshape(ctx.in_shape), None, None, None, None


class _MaskLossMeanFn(Function):
    """weight * masked mean over the VALID pixels, and its gradient, from one call (two passes over the logits)"""

    @staticmethod
    def forward(ctx, logits, labels, ignore_label, flags, coefs, weight):
        z, y = _mask_loss_inputs(logits, labels)
        _, s, dz = K.mask_loss(z, y, ignore_label, flags, coefs, want_mean=True, mean_scale=weight, want_grad=ctx.needs_input_grad[0],
                               grad_scale=weight)
        ctx.shape, ctx.in_dtype = logits.shape, logits.dtype
        ctx.save_for_backward(dz)
        return s.reshape(())

    @staticmethod
    def backward(ctx, dloss):
        (dz,) = ctx.saved_tensors
        if not _UNIT_LOSS_GRAD[0]:      # as _SoftmaxCEMeanFn: the scalar chain factor is applied on the device
            dz = K.scale_dev(dz, _c(dloss).reshape(1).to(torch.float32))
        if dz.dtype != ctx.in_dtype:
            dz = K.cast(dz, ctx.in_dtype)
        return dz.reshape(ctx.shape), None, None, None, None, None


def mask_loss_per_pixel(logits, labels, ignore_label, flags, coefs):
    """logits [B,H,W,C], labels [B,H,W] (already at the logits' size); flags = kernels.MASKLOSS_*, coefs = (sigmoid, dice, ce)"""
    return _MaskLossPerPixelFn.apply(logits, labels, int(ignore_label), int(flags), tuple(coefs))


def mask_loss_mean(logits, labels, ignore_label, flags, coefs, weight=1.0):
    return _MaskLossMeanFn.apply(logits, labels, int(ignore_label), int(flags), tuple(coefs), float(weight))


# ---------------------------------------------------------------------------------------------------------
# Deferred logits upsample: inside CoreTrain's step the model hands the low-resolution logits to the loss, and one kernel does
# bilinear upsample + cross-entropy + its gradient through the resize + the confusion matrix  (layers/core_model_ext.py:199-256,
# losses/catecrossentropy_ignore_label.py:44-88, metrics/seg_metric_wrapper.py:89-102)
# ---------------------------------------------------------------------------------------------------------
_DEFER_UPSAMPLE = [False]


class defer_logits_upsample:
    """while active, SegManaged returns DeferredLogits instead of the bilinear-upsampled fp32 logits"""

    def __enter__(self):
        self.prev = _DEFER_UPSAMPLE[0]
        _DEFER_UPSAMPLE[0] = True

    def __exit__(self, *a):
        _DEFER_UPSAMPLE[0] = self.prev


def deferring_logits_upsample():
    return _DEFER_UPSAMPLE[0]


class DeferredLogits:
    """low-resolution logits [N,h,w,C] + the size tf.image.resize would take them to; quacks like the fp32 [N,H,W,C] tensor as far
    as shape checks go and turns into it on materialize()"""

    def __init__(self, low, size):
        self.low, self.size = low, (int(size[0]), int(size[1]))
        self.dtype = torch.float32

    @property
    def shape(self):
        return torch.Size((self.low.shape[0], self.size[0], self.size[1], self.low.shape[3]))

    def dim(self):
        return 4

    def fusable(self, num_class):
        N, h, w, Cc = self.low.shape
        return Cc == num_class and self.low.is_cuda and K.upsample_ce_supported(h, w, self.size[0], self.size[1], Cc)

    def materialize(self):
        return resize_bilinear(self.low, self.size, out_dtype=torch.float32)


class _UpsampleCEMeanFn(Function):
    @staticmethod
    def forward(ctx, z, labels, Ho, Wo, ignore_label, class_w, weight, cm):
        zc = _c(z)
        y = _c(labels)
        if y.dtype != torch.int32:
            y = y.to(torch.int32)
        P = zc.shape[0] * Ho * Wo
        s, dz = K.upsample_ce(zc, y, Ho, Wo, ignore_label, class_w=class_w, sum_scale=weight / P, want_grad=ctx.needs_input_grad[0],
                              grad_scale=weight / P, cm=cm)
        ctx.in_dtype = z.dtype
        ctx.save_for_backward(dz)
        return s.reshape(())

    @staticmethod
    def backward(ctx, dloss):
        (dz,) = ctx.saved_tensors
        if not _UNIT_LOSS_GRAD[0]:
            dz = K.scale_dev(dz, _c(dloss).reshape(1).to(torch.float32))
        if dz.dtype != ctx.in_dtype:
            dz = K.cast(dz, ctx.in_dtype)
        return dz, None, None, None, None, None, None, None


def upsample_softmax_ce_mean(deferred, labels, num_class, ignore_label, class_w=None, weight=1.0, cm=None):
    """mean over ALL positions of the ignore-label CE of the bilinear-upsampled logits; the upsampled tensor is never written"""
    return _UpsampleCEMeanFn.apply(deferred.low, labels, deferred.size[0], deferred.size[1], int(ignore_label), class_w, float(weight), cm)


def softmax_ce_mean(logits, labels, num_class, ignore_label, class_w=None, weight=1.0, focal=None, cm=None):
    """cm: int64 [C*C] confusion matrix that the same kernel pass updates with argmax(logits) (running mIoU of the train step)"""
    return _SoftmaxCEMeanFn.apply(logits, labels, num_class, ignore_label, class_w, float(weight), focal, cm)


# ---------------------------------------------------------------------------------------------------------
# replace_nan_or_inf (utils/op_utils.py:43-60), GroupNormalization, RMSNormalization, pooling
# ---------------------------------------------------------------------------------------------------------
class _ReplaceNanInfFn(Function):
    @staticmethod
    def forward(ctx, x, nan_value):
        xc = _c(x)
        ctx.save_for_backward(xc)
        return K.replace_nan_or_inf(xc, nan_value)

    @staticmethod
    def backward(ctx, dy):
        (xc,) = ctx.saved_tensors
        return K.replace_nan_or_inf_bwd(xc, _c(dy)), None


def replace_nan_or_inf(x, nan_value=0.0):
    if nn.dry_run():
        return _dry(x.shape, x)
    return _ReplaceNanInfFn.apply(x, float(nan_value))


class _GroupNormFn(Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, groups, eps):
        N, C = x.shape[0], x.shape[-1]
        x3 = _c(x).reshape(N, -1, C)
        y, mean, rstd = K.groupnorm_fwd(x3, gamma.data if gamma is not None else None, beta.data if beta is not None else None, groups, eps)
        ctx.gamma, ctx.beta, ctx.groups = gamma, beta, groups
        ctx.save_for_backward(x3, mean, rstd)
        return y.reshape(x.shape)

    @staticmethod
    def backward(ctx, dy):
        x3, mean, rstd = ctx.saved_tensors
        g, b = ctx.gamma, ctx.beta
        dx = K.groupnorm_bwd(_c(dy).reshape(x3.shape), x3, g.data if g is not None else None, mean, rstd, ctx.groups,
                             _param_grad(g), _param_grad(b))
        dist.grads_ready(g, b)
        return dx.reshape(dy.shape), None, None, None, None


def group_norm(x, gamma, beta, groups, eps):
    _check_act_dtype(x)
    if nn.dry_run():
        return _dry(x.shape, x)
    return _GroupNormFn.apply(x, gamma, beta, int(groups), float(eps))


class _RMSNormFn(Function):
    @staticmethod
    def forward(ctx, x, scale, eps):
        C = x.shape[-1]
        x2 = _c(x).reshape(-1, C)
        y, rstd = K.rmsnorm_fwd(x2, scale.data, eps)
        ctx.scale = scale
        ctx.save_for_backward(x2, rstd)
        return y.reshape(x.shape)

    @staticmethod
    def backward(ctx, dy):
        x2, rstd = ctx.saved_tensors
        dx = K.rmsnorm_bwd(_c(dy).reshape(x2.shape), x2, ctx.scale.data, rstd, _grad_out(ctx.scale))
        dist.grads_ready(ctx.scale)
        return dx.reshape(dy.shape), None, None


def rms_norm(x, scale, eps):
    _check_act_dtype(x)
    if nn.dry_run():
        return _dry(x.shape, x)
    return _RMSNormFn.apply(x, scale, float(eps))


class _GRNFn(Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        N, C = x.shape[0], x.shape[-1]
        x3 = _c(x).reshape(N, -1, C)
        y, nx, gx = K.grn_fwd(x3, gamma.data, beta.data, eps)
        ctx.params = (gamma, beta)
        ctx.eps = eps
        ctx.save_for_backward(x3, nx, gx)
        return y.reshape(x.shape)

    @staticmethod
    def backward(ctx, dy):
        x3, nx, gx = ctx.saved_tensors
        gamma, beta = ctx.params
        dx = K.grn_bwd(_c(dy).reshape(x3.shape), x3, gamma.data, nx, gx, _grad_out(gamma), _grad_out(beta), ctx.eps)
        dist.grads_ready(gamma, beta)
        return dx.reshape(dy.shape), None, None, None


def grn(x, gamma, beta, eps=1e-6):
    """Global Response Normalization (backbones/convnext_v2.py:45-60): gamma * (x * nx) + beta + x with nx the per-sample channel response
    (L2 norm over H, W) divided by its mean over channels; gamma, beta are fp32 parameters of shape [1, 1, 1, C]"""
    _check_act_dtype(x)
    if nn.dry_run():
        return _dry(x.shape, x)
    return _GRNFn.apply(x, gamma, beta, float(eps))


class _Pool2dFn(Function):
    @staticmethod
    def forward(ctx, x, geom, mode):
        xc = _c(x)
        kh, kw, sh, sw, pt, pl, Ho, Wo = geom
        ctx.geom, ctx.mode = geom, mode
        ctx.save_for_backward(xc)
        return K.pool2d_fwd(xc, kh, kw, sh, sw, pt, pl, Ho, Wo, mode)

    @staticmethod
    def backward(ctx, dy):
        (xc,) = ctx.saved_tensors
        kh, kw, sh, sw, pt, pl, _, _ = ctx.geom
        return K.pool2d_bwd(xc, _c(dy), kh, kw, sh, sw, pt, pl, ctx.mode), None, None


def _pool(x, pool_size, strides, padding, mode):
    kh, kw = (pool_size, pool_size) if isinstance(pool_size, int) else tuple(pool_size)
    if strides is None:
        strides = (kh, kw)
    sh, sw = (strides, strides) if isinstance(strides, int) else tuple(strides)
    Ho, Wo, pt, pl = _conv_geometry(x.shape[1], x.shape[2], kh, kw, (sh, sw), (1, 1),
                                    padding.lower() if isinstance(padding, str) else padding)
    if nn.dry_run():
        return _dry((x.shape[0], Ho, Wo, x.shape[3]), x)
    return _Pool2dFn.apply(x, (kh, kw, sh, sw, pt, pl, Ho, Wo), mode)


def max_pool2d(x, pool_size, strides=None, padding="same"):
    """keras.layers.MaxPooling2D / tf.nn.max_pool2d"""
    return _pool(x, pool_size, strides, padding, K.POOL_MAX)


def avg_pool2d(x, pool_size, strides=None, padding="same"):
    """tf.nn.avg_pool2d: padded cells do not count in the divisor"""
    return _pool(x, pool_size, strides, padding, K.POOL_AVG)


class _AddReluFn(Function):
    @staticmethod
    def forward(ctx, a, b):
        y = K.add_relu(_c(a), _c(b))
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        d = K.act_bwd(_c(dy), y, K.ACT_RELU)
        return d, d


def add_relu(a, b):
    """tf.nn.relu(tf.add(a, b))"""
    if nn.dry_run():
        return _dry(a.shape, a)
    if a.numel() % 8 != 0:
        return relu(add(a, b))
    return _AddReluFn.apply(a, b)


# ---------------------------------------------------------------------------------------------------------
# multi-head self-attention core on a packed [q | k | v] tensor:
#   softmax(scale * q k^T + bias[h] + mask[w]) (-> dropout) (-> clip) @ v
# backbones/swin.py:117-167 (bias, shift mask), keras MultiHeadAttention in backbones/vit.py:142-147, and
# layers/multihead_self_attention.py:106-150 (clip).  Score / context products are strided-batch GEMMs, one problem per
# (sample, head); probabilities are kept for the backward pass (288 GB HBM: cheaper than recomputing them).
# ---------------------------------------------------------------------------------------------------------
_MAX_GRID_Z = 65535


def _attn_chunks(B, heads):
    per = max(1, _MAX_GRID_Z // heads)
    return [(b0, min(B, b0 + per)) for b0 in range(0, B, per)]


class _FlashAttentionFn(Function):
    """global self-attention without bias / mask / clip / dropout, head_dim 64, bf16 (ViT, MHSA): online-softmax forward that keeps
    one log-sum-exp float per row, backward kernels that recompute the probabilities (csrc/flashattn.hip); no T x T tensor"""

    @staticmethod
    def forward(ctx, qkv, heads, scale):
        qkv = _c(qkv)
        out, lse = K.attention_fwd_train(qkv, heads, scale)
        ctx.cfg = (heads, scale)
        ctx.save_for_backward(qkv, out, lse)
        return out

    @staticmethod
    def backward(ctx, dO):
        qkv, out, lse = ctx.saved_tensors
        heads, scale = ctx.cfg
        return K.attention_bwd(qkv, out, _c(dO), lse, heads, scale), None, None


class _AttentionFn(Function):
    @staticmethod
    def forward(ctx, qkv, bias_table, heads, Cq, Cv, scale, bias_index, mask, windows, clip, drop_rate, seed, bias_window=0, want_probs=False):
        B, T, ld = qkv.shape
        assert ld == 2 * Cq + Cv
        qkv = _c(qkv)
        dq, dv = Cq // heads, Cv // heads
        ctx.fused = (bias_table is not None and Cq == Cv and clip is None and drop_rate <= 0 and not want_probs and
                     K.window_attention_supported(T, dq, qkv.dtype) and os.environ.get("ISEG_WINATTN", "1") != "0")
        if ctx.fused:      # Swin window attention: one wavefront per (window, head), probabilities never leave the CU
            bias = K.relpos_bias_gather(bias_table.data, bias_index, heads, T)
            ctx.cfg = (heads, Cq, Cv, scale, windows, clip, drop_rate, seed, 0)
            ctx.bias_table, ctx.bias_index, ctx.bias_window = bias_table, bias_index, bias_window
            table = K.window_attention_table(bias, mask, heads, T)
            ctx.save_for_backward(qkv, table)
            return K.window_attention_fwd(qkv, table, heads, scale)
        Tp = (T + 7) // 8 * 8
        dev, dtp = qkv.device, qkv.dtype
        P = torch.empty((B * heads, T, Tp), dtype=dtp, device=dev)
        O = torch.empty((B, T, Cv), dtype=dtp, device=dev)
        bias = None
        if bias_table is not None:
            bias = K.relpos_bias_gather(bias_table.data, bias_index, heads, T)
        qv, kv, vv = qkv[:, :, :Cq], qkv[:, :, Cq:2 * Cq], qkv[:, :, 2 * Cq:]
        Pd = P
        for b0, b1 in _attn_chunks(B, heads):
            nb = (b1 - b0) * heads
            Pz = P[b0 * heads:b1 * heads]
            K.gemm(qv[b0:b1], kv[b0:b1], Pz, T, T, dq, lda=ld, ldb=ld, ldd=Tp, a_kcontig=1, b_kcontig=1, alpha=scale, batch=nb,
                   batch_inner=heads, sa=(T * ld, dq), sb=(T * ld, dq), sd=(heads * T * Tp, T * Tp))
            # problems of a chunk start at a multiple of `windows` samples only if b0 % windows == 0: chunks are sample-aligned
            K.softmax_rows_fwd(Pz, nb, T, T, Tp, bias=bias, heads=heads, mask=mask, windows=windows)
        if drop_rate > 0:
            Pd = K.dropout(P, drop_rate, seed)
        ctx.pre_clip = None
        if clip is not None:      # the exact softmax output is kept for the backward pass; the clipped copy feeds P @ V
            ctx.pre_clip = Pd
            Pd = K.clip_fwd(Pd, clip[0], clip[1])
        for b0, b1 in _attn_chunks(B, heads):
            nb = (b1 - b0) * heads
            K.gemm(Pd[b0 * heads:b1 * heads], vv[b0:b1], O[b0:b1], T, dv, T, lda=Tp, ldb=ld, ldd=Cv, a_kcontig=1, b_kcontig=0,
                   batch=nb, batch_inner=heads, sa=(heads * T * Tp, T * Tp), sb=(T * ld, dv), sd=(T * Cv, dv))
        ctx.cfg = (heads, Cq, Cv, scale, windows, clip, drop_rate, seed, Tp)
        ctx.bias_table, ctx.bias_index, ctx.bias_window = bias_table, bias_index, bias_window
        ctx.save_for_backward(qkv, P, Pd if Pd is not P else None)
        if want_probs:      # the probabilities that multiply V (after dropout / clip), [B, heads, T, T]; no gradient flows through this output
            probs = Pd.reshape(B, heads, T, Tp)[..., :T]
            ctx.mark_non_differentiable(probs)
            return O, probs
        return O

    @staticmethod
    def backward(ctx, dO, *unused_dprobs):
        if ctx.fused:
            qkv, table = ctx.saved_tensors
            heads, _, _, scale = ctx.cfg[:4]
            T = qkv.shape[1]
            dqkv, dbias = K.window_attention_bwd(qkv, table, _c(dO), heads, scale)
            if ctx.bias_table.requires_grad:
                K.relpos_bias_scatter_grad(dbias, T, ctx.bias_index, _grad(ctx.bias_table), heads, T, accumulate=True,
                                           window=ctx.bias_window)
                dist.grads_ready(ctx.bias_table)
            return (dqkv,) + (None,) * 13
        qkv, P, Pd = ctx.saved_tensors
        heads, Cq, Cv, scale, windows, clip, drop_rate, seed, Tp = ctx.cfg
        B, T, ld = qkv.shape
        dq, dv = Cq // heads, Cv // heads
        dO = _c(dO)
        Pd = P if Pd is None else Pd
        dqkv = torch.empty_like(qkv)
        dP = torch.empty_like(P)
        qv, kv, vv = qkv[:, :, :Cq], qkv[:, :, Cq:2 * Cq], qkv[:, :, 2 * Cq:]
        dqv, dkv, dvv = dqkv[:, :, :Cq], dqkv[:, :, Cq:2 * Cq], dqkv[:, :, 2 * Cq:]
        sP = (heads * T * Tp, T * Tp)
        for b0, b1 in _attn_chunks(B, heads):
            nb = (b1 - b0) * heads
            z0, z1 = b0 * heads, b1 * heads
            # dP = dO V^T ; dV = P^T dO
            K.gemm(dO[b0:b1], vv[b0:b1], dP[z0:z1], T, T, dv, lda=Cv, ldb=ld, ldd=Tp, a_kcontig=1, b_kcontig=1, batch=nb,
                   batch_inner=heads, sa=(T * Cv, dv), sb=(T * ld, dv), sd=sP)
            K.gemm(Pd[z0:z1], dO[b0:b1], dvv[b0:b1], T, dv, T, lda=Tp, ldb=Cv, ldd=ld, a_kcontig=0, b_kcontig=0, batch=nb,
                   batch_inner=heads, sa=sP, sb=(T * Cv, dv), sd=(T * ld, dv))
        if clip is not None:
            dP = K.clip_bwd(ctx.pre_clip, dP, clip[0], clip[1])
        if drop_rate > 0:
            dP = K.dropout(dP, drop_rate, seed)
        K.softmax_rows_bwd(P, dP, B * heads * T, T, Tp)
        if ctx.bias_table is not None and ctx.bias_table.requires_grad:
            dbias = torch.empty(heads * T * Tp, dtype=torch.float32, device=qkv.device)
            K.colsum_wide(dP.reshape(B, heads * T * Tp), dbias)
            K.relpos_bias_scatter_grad(dbias, Tp, ctx.bias_index, _grad(ctx.bias_table), heads, T, accumulate=True,
                                       window=ctx.bias_window)
            dist.grads_ready(ctx.bias_table)
        for b0, b1 in _attn_chunks(B, heads):
            nb = (b1 - b0) * heads
            z0, z1 = b0 * heads, b1 * heads
            # dQ = scale * dS K ; dK = scale * dS^T Q
            K.gemm(dP[z0:z1], kv[b0:b1], dqv[b0:b1], T, dq, T, lda=Tp, ldb=ld, ldd=ld, a_kcontig=1, b_kcontig=0, alpha=scale,
                   batch=nb, batch_inner=heads, sa=sP, sb=(T * ld, dq), sd=(T * ld, dq))
            K.gemm(dP[z0:z1], qv[b0:b1], dkv[b0:b1], T, dq, T, lda=Tp, ldb=ld, ldd=ld, a_kcontig=0, b_kcontig=0, alpha=scale,
                   batch=nb, batch_inner=heads, sa=sP, sb=(T * ld, dq), sd=(T * ld, dq))
        return (dqkv,) + (None,) * 13


def attention_packed(qkv, heads, Cq, Cv, scale, *, bias_table=None, bias_index=None, mask=None, windows=1, clip=None,
                     dropout_rate=0.0, training=False, bias_window=0, return_probs=False):
    """qkv [B, T, 2*Cq + Cv] (columns [q | k | v], each split into `heads` contiguous head slices) -> [B, T, Cv].
    bias_table [entries, heads] fp32 parameter + bias_index int32 [T*T]; mask fp32 [windows, T, T] (sample b uses mask
    b % windows); clip = (lo, hi) on the probabilities."""
    _check_act_dtype(qkv)
    if nn.dry_run():
        out = _dry((qkv.shape[0], qkv.shape[1], Cv), qkv)
        return (out, _dry((qkv.shape[0], heads, qkv.shape[1], qkv.shape[1]), qkv)) if return_probs else out
    if mask is not None and (_MAX_GRID_Z // heads) % windows != 0 and qkv.shape[0] * heads > _MAX_GRID_Z:
        raise NotImplementedError("attention_packed: chunked launch needs chunk sizes that are multiples of the window count")
    rate = float(dropout_rate) if training else 0.0
    if return_probs:
        return _AttentionFn.apply(qkv, bias_table, int(heads), int(Cq), int(Cv), float(scale), bias_index, mask, int(windows), clip, rate,
                                  next_seed() if rate > 0 else 0, int(bias_window), True)
    if (bias_table is None and mask is None and clip is None and rate <= 0 and Cq == Cv and
            K.attention_fwd_supported(Cq // heads, qkv.dtype) and os.environ.get("ISEG_FLASHATTN", "1") != "0"):
        # online-softmax kernels, no T x T tensor: forward only for inference, the recomputing forward / backward pair for training
        if not (torch.is_grad_enabled() and qkv.requires_grad):
            return K.attention_fwd(_c(qkv), int(heads), float(scale))
        return _FlashAttentionFn.apply(qkv, int(heads), float(scale))
    return _AttentionFn.apply(qkv, bias_table, int(heads), int(Cq), int(Cv), float(scale), bias_index, mask, int(windows), clip,
                              rate, next_seed() if rate > 0 else 0, int(bias_window))


class _SelfAttentionFn(Function):
    """single-head attention with a 64-wide query / key and a wide value, bf16, no dropout (layers/self_attention.py:76-85): online-softmax
    forward per value slab that keeps one log-sum-exp float per row, backward kernels that recompute the probabilities (csrc/selfattn.hip);
    no T x T tensor.  q and k may be aliases of one tensor (shared_querykey): the kernels then read one buffer and dq, dk still arrive apart."""

    @staticmethod
    def forward(ctx, q, k, v, scale):
        out, lse = K.self_attention_fwd(q, k, v, scale, True)
        ctx.scale = scale
        ctx.save_for_backward(q, k, v, out, lse)
        return out

    @staticmethod
    def backward(ctx, dO):
        q, k, v, out, lse = ctx.saved_tensors
        dq, dk, dv = K.self_attention_bwd(q, k, v, out, dO, lse, ctx.scale)
        return dq, dk, dv, None


_SELFATTN_TRAIN_SHARE = 0.25      # of the device's memory: beyond it the composed route's probabilities and their gradient give way
_DEVICE_BYTES = {}


def _self_attention_route(B, T, device, training):
    """True: the fused kernels.  ISEG_SELFATTN_FUSED=0: composed, =1: fused, unset: fused for inference (not slower, nothing of size T x T);
    for training the composed route, which is faster while its tensors fit (EXPERIMENTS.md 'SelfAttention core': 3.2 ms against 6.0 ms at
    16 x 4096, dv 512) -- until its [B, T, T] probabilities and their gradient together pass a quarter of the device's memory"""
    mode = os.environ.get("ISEG_SELFATTN_FUSED", "")
    if mode in ("0", "1"):
        return mode == "1"
    if not training:
        return True
    idx = device.index if device.index is not None else torch.cuda.current_device()
    total = _DEVICE_BYTES.get(idx)
    if total is None:
        total = _DEVICE_BYTES[idx] = torch.cuda.get_device_properties(idx).total_memory
    return 2 * (B * T * T * 2) > _SELFATTN_TRAIN_SHARE * total


def self_attention_core(q, k, v, scale, *, dropout_rate=0.0, training=False):
    """softmax(scale * q k^T) v with dropout on the probabilities: q, k [B, T, dk], v [B, T, dv] -> [B, T, dv]
    (layers/self_attention.py:76-85, get_attention of utils/attention_utils.py:23-40: a plain softmax, no clip).
    bf16 with dk 64, dv a multiple of 64 up to 1024 and no dropout in effect can run on the fused kernels of csrc/selfattn.hip, and does
    where _self_attention_route says so (inference; training past a memory share; ISEG_SELFATTN_FUSED=1: always, =0: composed); everything
    else is concatenated and takes attention_packed's materialised route."""
    _check_act_dtype(v)
    if q.dim() != 3 or q.shape != k.shape or v.dim() != 3 or v.shape[:2] != q.shape[:2]:
        raise ValueError(f"self_attention_core: q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)} are not [B,T,dk], [B,T,dk], [B,T,dv]")
    if nn.dry_run():
        return _dry(v.shape, v)
    rate = float(dropout_rate) if training else 0.0
    dk, dv = int(q.shape[2]), int(v.shape[2])
    need_grad = torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad)
    if (rate <= 0 and scale > 0 and q.dtype == k.dtype == v.dtype and K.self_attention_supported(dk, dv, v.dtype)
            and _self_attention_route(int(q.shape[0]), int(q.shape[1]), v.device, need_grad)):
        if not need_grad:
            return K.self_attention_fwd(q, k, v, float(scale), False)[0]
        return _SelfAttentionFn.apply(q, k, v, float(scale))
    return attention_packed(concat([q, k, v]), 1, dk, dv, float(scale), dropout_rate=dropout_rate, training=training)


class _Dcnv2SampleFn(Function):
    """DCNv2's modulated deformable sampling (layers/dcn_v2.py:114-229): x [N,H,W,C], offset [N,H,W,27] -> [N,H,W,9 C]"""

    @staticmethod
    def forward(ctx, x, offset):
        xc, oc = _c(x), _c(offset)
        ctx.save_for_backward(xc, oc)
        N, H, W, C = xc.shape
        return K.dcnv2_sample_fwd(xc, oc).reshape(N, H, W, 9 * C)

    @staticmethod
    def backward(ctx, dcol):
        xc, oc = ctx.saved_tensors
        dx, doff = K.dcnv2_sample_bwd(xc, oc, _c(dcol))
        return (dx if xc.dtype == torch.float32 else K.cast(dx, xc.dtype)), doff


def dcnv2_sample(x, offset):
    _check_act_dtype(x)
    if nn.dry_run():
        return _dry((*x.shape[:3], 9 * x.shape[3]), x)
    return _Dcnv2SampleFn.apply(x, offset)


class _QkvRopeFn(Function):
    """packed attention rows [B, T, 3C]: q += q_bias, v += v_bias, rotary embedding on q and k of the tokens >= prefix -- one pass
    (csrc/eva.hip; backbones/eva/attention.py:100-112,136-146).  Backward: the transposed rotation in place on the gradient, bias gradients as
    strided column sums of its q / v blocks."""

    @staticmethod
    def forward(ctx, qkv, q_bias, v_bias, emb, prefix, heads):
        B, T, C3 = qkv.shape
        C = C3 // 3
        ctx.q_bias, ctx.v_bias, ctx.emb, ctx.geom = q_bias, v_bias, emb, (T, int(prefix), C, C // heads)
        src = _c(qkv)
        out = torch.empty_like(src)
        K.qkv_rope(src, None if q_bias is None else q_bias.data, None if v_bias is None else v_bias.data, emb, T, int(prefix), C, C // heads, out=out)
        return out

    @staticmethod
    def backward(ctx, d):
        T, prefix, C, hd = ctx.geom
        d = _c(d)
        g = torch.empty_like(d)
        K.qkv_rope(d, None, None, ctx.emb, T, prefix, C, hd, inverse=True, out=g)
        d2 = g.reshape(-1, 3 * C)
        for b, off in ((ctx.q_bias, 0), (ctx.v_bias, 2 * C)):
            if b is not None and b.requires_grad:
                K.colsum(d2[:, off:off + C], d2.stride(0), 0, 1, d2.shape[0], C, _grad(b).reshape(-1), accumulate=True)
        dist.grads_ready(*[b for b in (ctx.q_bias, ctx.v_bias) if b is not None])
        return g, None, None, None, None, None


def qkv_rope(qkv, q_bias, v_bias, emb, prefix, heads):
    """EVA attention's bias + rotary step on packed [B, T, 3C] rows (emb fp32 [T - prefix, 2 head_dim] or None)"""
    if nn.dry_run():
        return qkv
    if q_bias is None and v_bias is None and emb is None:
        return qkv
    return _QkvRopeFn.apply(qkv, q_bias, v_bias, emb, prefix, heads)


class _GluFn(Function):
    """act(gate) * x (backbones/eva/swiglu.py:88-92, glumlp.py:96-103); `packed` [.., 2H] = [x | gate] (gate_last) or [gate | x]"""

    @staticmethod
    def forward(ctx, gate, x, act, packed_order):
        if packed_order:      # gate is the packed tensor, x unused
            H = gate.shape[-1] // 2
            p2 = _c(gate).reshape(-1, 2 * H)
            g2, x2 = (p2[:, H:], p2[:, :H]) if packed_order == 1 else (p2[:, :H], p2[:, H:])
            out_shape = (*gate.shape[:-1], H)
        else:
            H = gate.shape[-1]
            g2, x2 = _c(gate).reshape(-1, H), _c(x).reshape(-1, H)
            out_shape = gate.shape
        ctx.act, ctx.packed_order, ctx.in_shape = act, packed_order, gate.shape
        ctx.save_for_backward(g2, x2)
        return K.glu_fwd(g2, x2, act).reshape(out_shape)

    @staticmethod
    def backward(ctx, dout):
        g2, x2 = ctx.saved_tensors
        H = g2.shape[1]
        d2 = _c(dout).reshape(-1, H)
        if ctx.packed_order:
            dp = torch.empty((g2.shape[0], 2 * H), dtype=g2.dtype, device=g2.device)
            dg, dx = (dp[:, H:], dp[:, :H]) if ctx.packed_order == 1 else (dp[:, :H], dp[:, H:])
            K.glu_bwd(d2, g2, x2, dg, dx, ctx.act)
            return dp.reshape(ctx.in_shape), None, None, None
        dg, dx = torch.empty_like(g2), torch.empty_like(x2)
        K.glu_bwd(d2, g2, x2, dg, dx, ctx.act)
        return dg.reshape(ctx.in_shape), dx.reshape(ctx.in_shape), None, None


_GLU_ACTS = {"gelu": K.ACT_GELU, "swish": K.ACT_SWISH, "silu": K.ACT_SWISH, "sigmoid": K.ACT_SIGMOID, "gelu_tanh": K.ACT_GELU_TANH}


def glu(gate, x, activation):
    """activation(gate) * x, both [..., H]"""
    _check_act_dtype(gate)
    if nn.dry_run():
        return _dry(gate.shape, gate)
    return _GluFn.apply(gate, x, _GLU_ACTS[activation], 0)


def glu_packed(packed, activation, gate_last=True):
    """x1, x2 = split(packed, 2, axis=-1); x1 * activation(x2) if gate_last else activation(x1) * x2   (glumlp.py:96-103)"""
    _check_act_dtype(packed)
    if nn.dry_run():
        return _dry((*packed.shape[:-1], packed.shape[-1] // 2), packed)
    return _GluFn.apply(packed, None, _GLU_ACTS[activation], 1 if gate_last else 2)


class _GatherRowsFn(Function):
    @staticmethod
    def forward(ctx, x, idx_fwd, idx_bwd, out_shape):
        C = x.shape[-1]
        ctx.in_shape, ctx.idx_bwd = x.shape, idx_bwd
        return K.gather_rows(_c(x).reshape(-1, C), idx_fwd, idx_fwd.numel()).reshape(out_shape)

    @staticmethod
    def backward(ctx, dy):
        C = dy.shape[-1]
        idx = ctx.idx_bwd
        return K.gather_rows(_c(dy).reshape(-1, C), idx, idx.numel()).reshape(ctx.in_shape), None, None, None


def permute_rows(x, idx_fwd, idx_bwd, out_shape):
    """rows of x (last axis = channels) re-ordered by a static index table; idx_bwd is the inverse table (-1 where a source
    row has no destination / a destination is padding).  Each source row may appear at most once in idx_fwd."""
    if nn.dry_run():
        return _dry(out_shape, x)
    return _GatherRowsFn.apply(x, idx_fwd, idx_bwd, tuple(out_shape))


class _LnGatherFn(Function):
    """LayerNorm + static row permutation with zero padding in one pass each way (Swin: norm1 + pad + roll + window partition).  `link`
    pairs the node with the _GatherResidualFn that closes the same residual branch: that node's backward runs first and leaves the skip
    connection's gradient in link["dres"], which this node's LayerNorm backward adds on its way out (dx_add) -- the branch's fork costs no pass."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, idx_fwd, idx_bwd, out_shape, link):
        C = x.shape[-1]
        x2 = _c(x).reshape(-1, C)
        y, mean, rstd = K.layernorm_gather_fwd(x2, idx_fwd, gamma.data, beta.data, eps)
        ctx.gamma, ctx.beta, ctx.idx_bwd, ctx.link, ctx.in_shape = gamma, beta, idx_bwd, link, x.shape
        ctx.save_for_backward(x2, mean, rstd)
        if link is not None:
            link.pop("dres", None)      # nothing of an earlier step (a backward pass that stopped between the two nodes) survives into this one
            link["armed"] = bool(ctx.needs_input_grad[0])
            link["x"] = (x.data_ptr(), tuple(x.shape))      # the skip connection handed over through the link must be THIS tensor
        return y.reshape(out_shape)

    @staticmethod
    def backward(ctx, dy):
        x2, mean, rstd = ctx.saved_tensors
        C = x2.shape[1]
        dres = ctx.link.pop("dres", None) if ctx.link is not None else None
        if dres is not None:
            dres = _c(dres).reshape(-1, C)
        dx = K.layernorm_gather_bwd(_c(dy).reshape(-1, C), ctx.idx_bwd, x2, ctx.gamma.data, mean, rstd, _grad_out(ctx.gamma), _grad_out(ctx.beta), dx_add=dres)
        dist.grads_ready(ctx.gamma, ctx.beta)
        return (dx.reshape(ctx.in_shape) if ctx.needs_input_grad[0] else None,) + (None,) * 7


class _GatherResidualFn(Function):
    """residual + rowscale[sample] * rows(y)[idx_fwd] in one pass (Swin: window reverse + roll back + crop + drop path + skip connection)"""

    @staticmethod
    def forward(ctx, y, residual, idx_fwd, idx_bwd, rowscale, link):
        C = y.shape[-1]
        r2 = _c(residual).reshape(-1, C)
        rpg = r2.shape[0] // rowscale.shape[0] if rowscale is not None else 0
        ctx.idx_bwd, ctx.rowscale, ctx.rpg, ctx.link, ctx.y_shape = idx_bwd, rowscale, rpg, link, y.shape
        if link is not None and link.get("armed") and link.get("x") != (residual.data_ptr(), tuple(residual.shape)):
            raise ValueError("permute_rows_residual: `link` pairs this node with a layer_norm_permute_rows of ANOTHER tensor -- the skip connection's "
                             "gradient would be added to the wrong LayerNorm input")
        return K.gather_rows_fma(_c(y).reshape(-1, C), idx_fwd, rowscale, rpg, False, r2).reshape(residual.shape)

    @staticmethod
    def backward(ctx, dout):
        C = dout.shape[-1]
        d2 = _c(dout).reshape(-1, C)
        dy = K.gather_rows_fma(d2, ctx.idx_bwd, ctx.rowscale, ctx.rpg, True, None).reshape(ctx.y_shape) if ctx.needs_input_grad[0] else None
        dres = dout if ctx.needs_input_grad[1] else None
        if dres is not None and ctx.link is not None and ctx.link.get("armed") and dy is not None:
            ctx.link["dres"] = dres      # the paired _LnGatherFn adds it inside its LayerNorm backward
            dres = None
        return dy, dres, None, None, None, None


def residual_branch_link():
    """the pairing object of layer_norm_permute_rows / permute_rows_residual on one residual branch (see _LnGatherFn)"""
    return {}


def layer_norm_permute_rows(x, gamma, beta, eps, idx_fwd, idx_bwd, out_shape, link=None):
    """permute_rows(layer_norm(x), idx_fwd, idx_bwd, out_shape) as one tape node; padding rows (idx_fwd < 0) are zero"""
    _check_act_dtype(x)
    if nn.dry_run():
        return _dry(out_shape, x)
    return _LnGatherFn.apply(x, gamma, beta, float(eps), idx_fwd, idx_bwd, tuple(out_shape), link)


def permute_rows_residual(y, residual, idx_fwd, idx_bwd, drop_path_mask=None, link=None):
    """residual + drop_path_mask[sample] * permute_rows(y, idx_fwd, idx_bwd, residual.shape) as one tape node.  With `link` shared with the
    layer_norm_permute_rows that opened the branch FROM THE SAME TENSOR `residual`, the skip connection's gradient is delivered through that
    node (the caller must not consume `residual` anywhere else between the two)."""
    if nn.dry_run():
        return _dry(residual.shape, residual)
    return _GatherResidualFn.apply(y, residual, idx_fwd, idx_bwd, drop_path_mask, link)


# ---------------------------------------------------------------------------------------------------------
# token-axis helpers of backbones/vit.py:277-323: class token, position embedding, token slicing
# ---------------------------------------------------------------------------------------------------------
class _PrependTokenFn(Function):
    @staticmethod
    def forward(ctx, x, token):
        B, T, C = x.shape
        xc = _c(x)
        y = torch.empty((B, T + 1, C), dtype=x.dtype, device=x.device)
        tok = K.cast(token.data.reshape(1, C), x.dtype)
        K.copy2d(tok, 0, y, (T + 1) * C, B, C)                          # row stride 0: the same token for every sample
        K.copy2d(xc, T * C, y.reshape(B, -1)[:, C:], (T + 1) * C, B, T * C)
        ctx.token = token
        return y

    @staticmethod
    def backward(ctx, dy):
        B, T1, C = dy.shape
        dyc = _c(dy)
        if ctx.token.requires_grad:
            K.colsum(dyc, T1 * C, 0, 1, B, C, _grad(ctx.token).reshape(-1), accumulate=True)
            dist.grads_ready(ctx.token)
        dx = torch.empty((B, T1 - 1, C), dtype=dy.dtype, device=dy.device)
        K.copy2d(dyc.reshape(B, -1)[:, C:], T1 * C, dx, (T1 - 1) * C, B, (T1 - 1) * C)
        return dx, None


def prepend_token(x, token):
    """tf.concat([broadcast(class_token), x], axis=1); token is an fp32 parameter [1,1,C]"""
    if nn.dry_run():
        return _dry((x.shape[0], x.shape[1] + 1, x.shape[2]), x)
    return _PrependTokenFn.apply(x, token)


class _DropTokensFn(Function):
    @staticmethod
    def forward(ctx, x, n_extra):
        B, T, C = x.shape
        ctx.n_extra, ctx.shape = n_extra, x.shape
        y = torch.empty((B, T - n_extra, C), dtype=x.dtype, device=x.device)
        K.copy2d(_c(x).reshape(B, -1)[:, n_extra * C:], T * C, y, (T - n_extra) * C, B, (T - n_extra) * C)
        return y

    @staticmethod
    def backward(ctx, dy):
        B, T, C = ctx.shape
        e = ctx.n_extra
        dx = torch.empty(ctx.shape, dtype=dy.dtype, device=dy.device)
        zero = torch.zeros((1, e * C), dtype=dy.dtype, device=dy.device)
        K.copy2d(zero, 0, dx, T * C, B, e * C)
        K.copy2d(_c(dy), (T - e) * C, dx.reshape(B, -1)[:, e * C:], T * C, B, (T - e) * C)
        return dx, None


def drop_tokens(x, n_extra):
    """x[:, n_extra:]"""
    if n_extra == 0:
        return x
    if nn.dry_run():
        return _dry((x.shape[0], x.shape[1] - n_extra, x.shape[2]), x)
    return _DropTokensFn.apply(x, int(n_extra))


class _AddBatchBroadcastFn(Function):
    @staticmethod
    def forward(ctx, x, v):
        B = x.shape[0]
        n = x.numel() // B
        y = torch.empty(x.shape, dtype=x.dtype, device=x.device)
        K.copy2d(_c(x), n, y, n, B, n)
        K.broadcast_rows(_c(v).reshape(1, n), y, n, 0, 1, B, n, accumulate=True)
        ctx.v_dtype, ctx.v_shape = v.dtype, v.shape
        return y

    @staticmethod
    def backward(ctx, dy):
        B = dy.shape[0]
        n = dy.numel() // B
        dv = torch.empty(n, dtype=torch.float32, device=dy.device)
        K.colsum(_c(dy), n, 0, 1, B, n, dv)
        dv = dv if ctx.v_dtype == torch.float32 else K.cast(dv, ctx.v_dtype)
        return dy, dv.reshape(ctx.v_shape)


def add_batch_broadcast(x, v):
    """x [B, ...] + v [1, ...] (tf.add with broadcasting over the batch axis: position embedding)"""
    if nn.dry_run():
        return _dry(x.shape, x)
    return _AddBatchBroadcastFn.apply(x, v)


class _PosEmbedResizeFn(Function):
    """backbones/vit.py:19-63 resize_pos_embed: the grid part [1, g*g, C] of the fp32 position embedding is resampled to
    (Ho, Wo) by tf.image.resize(bicubic) -- a separable linear map, expressed as two fp32 GEMMs y = Wy @ x @ Wx^T per channel
    with constant weight matrices built on the host (utils/bicubic.py) -- the extra (class) tokens are passed through, and the
    result is cast to the compute dtype.  The gradient is written straight into the parameter's gradient buffer."""

    @staticmethod
    def forward(ctx, pos, Wy, Wx, n_extra, out_dtype):
        _, L, C = pos.shape
        Hi, Wi = Wy.shape[1], Wx.shape[1]
        Ho, Wo = Wy.shape[0], Wx.shape[0]
        assert L == n_extra + Hi * Wi
        src = pos.data.reshape(L, C)
        out = torch.empty((1, n_extra + Ho * Wo, C), dtype=torch.float32, device=pos.device)
        o2 = out.reshape(-1, C)
        if n_extra:
            K.copy2d(src, C, o2, C, n_extra, C)
        grid = src[n_extra:]
        t = torch.empty((Ho, Wi * C), dtype=torch.float32, device=pos.device)
        K.gemm(Wy, grid, t, Ho, Wi * C, Hi, lda=Hi, ldb=Wi * C, ldd=Wi * C, a_kcontig=1, b_kcontig=0)
        K.gemm(Wx, t, o2[n_extra:], Wo, C, Wi, lda=Wi, ldb=C, ldd=C, a_kcontig=1, b_kcontig=0, batch=Ho, batch_inner=1,
               sa=(0, 0), sb=(Wi * C, 0), sd=(Wo * C, 0))
        ctx.pos, ctx.n_extra = pos, n_extra
        ctx.save_for_backward(Wy, Wx)
        return out if out_dtype == torch.float32 else K.cast(out, out_dtype)

    @staticmethod
    def backward(ctx, dy):
        Wy, Wx = ctx.saved_tensors
        pos, e = ctx.pos, ctx.n_extra
        if not pos.requires_grad:
            return None, None, None, None, None
        C = pos.shape[-1]
        Hi, Wi = Wy.shape[1], Wx.shape[1]
        Ho, Wo = Wy.shape[0], Wx.shape[0]
        d = _c(dy) if dy.dtype == torch.float32 else K.cast(_c(dy), torch.float32)
        d2 = d.reshape(-1, C)
        g = _grad(pos).reshape(-1, C)
        if e:
            K.add2d(d2, C, g, C, e, C)
        dt_ = torch.empty((Ho, Wi * C), dtype=torch.float32, device=dy.device)
        K.gemm(Wx, d2[e:], dt_, Wi, C, Wo, lda=Wi, ldb=C, ldd=C, a_kcontig=0, b_kcontig=0, batch=Ho, batch_inner=1, sa=(0, 0),
               sb=(Wo * C, 0), sd=(Wi * C, 0))
        K.gemm(Wy, dt_, g[e:], Hi, Wi * C, Ho, lda=Hi, ldb=Wi * C, ldd=Wi * C, a_kcontig=0, b_kcontig=0, accumulate=True)
        dist.grads_ready(pos)
        return None, None, None, None, None


_BICUBIC_MATRICES = {}


def _bicubic_weights(out_size, in_size, device):
    key = (int(out_size), int(in_size), str(device))
    m = _BICUBIC_MATRICES.get(key)
    if m is None:
        from .utils.bicubic import bicubic_matrix

        m = _BICUBIC_MATRICES[key] = torch.from_numpy(bicubic_matrix(int(out_size), int(in_size))).to(device)
    return m


class _ResizeBicubicFn(Function):
    """tf.image.resize(images, size, method="bicubic") (utils/common.py:107-134 of the reference: half-pixel centres, Keys a = -0.5, no
    antialias, fp32 result cast back to the input dtype): the separable map y[n] = Wy @ x[n] @ Wx^T as two strided-batch fp32 GEMMs with the
    host-built tap matrices of utils/bicubic.py (the kernel of the ViT position-embedding resize).  The gradient is the transposed map."""

    @staticmethod
    def forward(ctx, x, Ho, Wo):
        N, Hi, Wi, C = x.shape
        xf = _c(x) if x.dtype == torch.float32 else K.cast(_c(x), torch.float32)
        Wy, Wx = _bicubic_weights(Ho, Hi, x.device), _bicubic_weights(Wo, Wi, x.device)
        t = torch.empty((N, Ho, Wi * C), dtype=torch.float32, device=x.device)
        K.gemm(Wy, xf.reshape(N, Hi, Wi * C), t, Ho, Wi * C, Hi, lda=Hi, ldb=Wi * C, ldd=Wi * C, a_kcontig=1, b_kcontig=0, batch=N, batch_inner=1,
               sa=(0, 0), sb=(Hi * Wi * C, 0), sd=(Ho * Wi * C, 0))
        y = torch.empty((N, Ho, Wo, C), dtype=torch.float32, device=x.device)
        K.gemm(Wx, t, y, Wo, C, Wi, lda=Wi, ldb=C, ldd=C, a_kcontig=1, b_kcontig=0, batch=N * Ho, batch_inner=1, sa=(0, 0), sb=(Wi * C, 0),
               sd=(Wo * C, 0))
        ctx.shape, ctx.dtype = (N, Hi, Wi, C), x.dtype
        ctx.save_for_backward(Wy, Wx)
        return y if x.dtype == torch.float32 else K.cast(y, x.dtype)

    @staticmethod
    def backward(ctx, dy):
        Wy, Wx = ctx.saved_tensors
        N, Hi, Wi, C = ctx.shape
        Ho, Wo = Wy.shape[0], Wx.shape[0]
        d = _c(dy) if dy.dtype == torch.float32 else K.cast(_c(dy), torch.float32)
        dt_ = torch.empty((N, Ho, Wi * C), dtype=torch.float32, device=dy.device)
        K.gemm(Wx, d, dt_, Wi, C, Wo, lda=Wi, ldb=C, ldd=C, a_kcontig=0, b_kcontig=0, batch=N * Ho, batch_inner=1, sa=(0, 0), sb=(Wo * C, 0),
               sd=(Wi * C, 0))
        dx = torch.empty((N, Hi, Wi * C), dtype=torch.float32, device=dy.device)
        K.gemm(Wy, dt_, dx, Hi, Wi * C, Ho, lda=Hi, ldb=Wi * C, ldd=Wi * C, a_kcontig=0, b_kcontig=0, batch=N, batch_inner=1, sa=(0, 0),
               sb=(Ho * Wi * C, 0), sd=(Hi * Wi * C, 0))
        dx = dx.reshape(N, Hi, Wi, C)
        return (dx if ctx.dtype == torch.float32 else K.cast(dx, ctx.dtype)), None, None


def resize_bicubic(x, size):
    Ho, Wo = int(size[0]), int(size[1])
    if nn.dry_run():
        return _dry((x.shape[0], Ho, Wo, x.shape[3]), x)
    return _ResizeBicubicFn.apply(x, Ho, Wo)


def resize_pos_embed(pos, Wy, Wx, n_extra, out_dtype):
    if nn.dry_run():
        return _dry((1, n_extra + Wy.shape[0] * Wx.shape[0], pos.shape[-1]), pos, out_dtype)
    return _PosEmbedResizeFn.apply(pos, Wy, Wx, int(n_extra), out_dtype)


# ---------------------------------------------------------------------------------------------------------
# DCNv3 core (layers/dcn_v3/op.py:16-109), softmax over the last axis in groups, per-channel scale
# ---------------------------------------------------------------------------------------------------------
class _Dcnv3Fn(Function):
    @staticmethod
    def forward(ctx, x, offset, mask, cfg):
        G, Cg, kh, kw, stride, dil, pad, s = cfg
        xc, oc, mc = _c(x), _c(offset), _c(mask)
        ctx.cfg = cfg
        ctx.save_for_backward(xc, oc, mc)
        return K.dcnv3_fwd(xc, oc, mc, G, Cg, kh, kw, stride, dil, pad, s)

    @staticmethod
    def backward(ctx, dy):
        xc, oc, mc = ctx.saved_tensors
        G, Cg, kh, kw, stride, dil, pad, s = ctx.cfg
        dx, doff, dmask = K.dcnv3_bwd(xc, oc, mc, _c(dy), G, Cg, kh, kw, stride, dil, pad, s)
        if dx.dtype != xc.dtype:
            dx = K.cast(dx, xc.dtype)
        return dx, doff, dmask, None


_DCN_JOINT = os.environ.get("ISEG_DCN_JOINT", "1") != "0"      # experiment knob: 0 = offset and mask as two Dense layers + softmax_groups


class _DcnJointFn(Function):
    """offset | mask projection, mask softmax and the DCNv3 sampling core of one layer (layers/dcn_v3/dcn_v3.py:116-131) with the two Dense layers
    run as ONE product of width ld = 3 G P rounded up to 8 into a [pixels, ld] matrix whose column ranges the sampling kernels read in place
    (csrc/dcnv3.hip iseg_dcnv3_fwd_ld): widths like 126 / 63 (G = 7) or 252 (G = 28) keep two products off the LDS-DMA GEMM each way, their sum
    padded to 192 / 768 does not.  Backward: sampling gradients in the same layout, softmax backward in place, ONE data-gradient product, ONE
    weight-gradient product whose [C, ld] result (and ones-row bias gradient) is added column-range-wise into the two layers' gradients."""

    @staticmethod
    def forward(ctx, x_proj, x1, W_off, b_off, W_mask, b_mask, cfg):
        G, Cg, kh, kw, stride, dil, pad, s = cfg
        P = kh * kw
        Cin = x1.shape[-1]
        x2 = _c(x1).reshape(-1, Cin)
        rowcat, tr, bias = nn.joint_kernels(W_off, W_mask, b_off, b_mask)
        om = K.dense_fwd_t(x2, tr, bias)
        K.dcn_mask_softmax_fwd(om, G, P)
        xp = _c(x_proj)
        y = K.dcnv3_fwd_joint(xp, om, G, Cg, kh, kw, stride, dil, pad, s)
        ctx.cfg, ctx.params = cfg, (W_off, b_off, W_mask, b_mask)
        ctx.save_for_backward(xp, x2, om)
        ctx.x1_shape = x1.shape
        return y

    @staticmethod
    def backward(ctx, dy):
        xp, x2, om = ctx.saved_tensors
        G, Cg, kh, kw, stride, dil, pad, s = ctx.cfg
        P = kh * kw
        W_off, b_off, W_mask, b_mask = ctx.params
        dxp, dom = K.dcnv3_bwd_joint(xp, om, _c(dy), G, Cg, kh, kw, stride, dil, pad, s)
        if dxp.dtype != xp.dtype:
            dxp = K.cast(dxp, xp.dtype)
        K.dcn_mask_softmax_bwd(om, dom, G, P)
        rowcat, tr, bias = nn.joint_kernels(W_off, W_mask, b_off, b_mask)
        Cin, ld = rowcat.shape
        na, nb = 2 * G * P, G * P
        want_w = W_off.requires_grad or W_mask.requires_grad
        want_b = b_off.requires_grad or b_mask.requires_grad
        if want_w:
            dW = torch.empty((Cin, ld), dtype=torch.float32, device=dom.device)
            db = torch.empty(ld, dtype=torch.float32, device=dom.device) if want_b else None
            K.dense_wgrad(x2, dom, dW, accumulate=False, bias_grad=db)
            K.split_cols_accumulate(dW, _param_grad(W_off, Cin, na), na, _param_grad(W_mask, Cin, nb), nb)
        elif want_b:
            db = torch.empty(ld, dtype=torch.float32, device=dom.device)
            K.colsum(dom, ld, 0, 1, dom.shape[0], ld, db, accumulate=False)
        if want_b:
            K.split_cols_accumulate(db, _param_grad(b_off, -1), na, _param_grad(b_mask, -1), nb)
        dx1 = None
        if ctx.needs_input_grad[1]:
            dx1 = K.dense_dgrad(dom, rowcat).reshape(ctx.x1_shape)
        dist.grads_ready(W_off, b_off, W_mask, b_mask)
        return dxp, dx1, None, None, None, None, None


def dcnv3_joint_ok(x1, offset_layer, mask_layer, kernel_size, stride=1, out_hw=None):
    """stride / out_hw: the joint form projects x1 pixel by pixel, so the offset / mask rows are x1's pixels -- they are the sampling kernel's OUTPUT
    pixels only at stride 1 with an unchanged map size (round-5 advisor: a strided layer must fall back to the layer-by-layer route, not raise)"""
    kh, kw = kernel_size
    if int(stride) != 1 or (out_hw is not None and tuple(out_hw) != tuple(x1.shape[1:3])):
        return False
    return (_DCN_JOINT and not nn.dry_run() and x1.dtype == torch.bfloat16 and kh * kw <= 9 and getattr(offset_layer, "kernel", None) is not None
            and getattr(mask_layer, "kernel", None) is not None and offset_layer.bias is not None and mask_layer.bias is not None
            and x1.shape[-1] % 8 == 0 and x1.shape[-1] >= 64)


def dcnv3_joint(x_proj, x1, offset_layer, mask_layer, groups, group_channels, kernel_size=(3, 3), stride=1, dilation=1, pad=1, offset_scale=1.0):
    """F.dcnv3_core(x_proj, offset_layer(x1), softmax_groups(mask_layer(x1)), ...) as one node (see _DcnJointFn), or None when this form does not
    apply (fp32 storage, more than nine sampling points, a projection without bias, ISEG_DCN_JOINT=0): the caller then takes the layer-by-layer
    route"""
    kh, kw = kernel_size
    if not dcnv3_joint_ok(x1, offset_layer, mask_layer, kernel_size, stride, K.dcnv3_out_hw(x_proj.shape[1], x_proj.shape[2], kh, kw, stride, dilation, pad)):
        return None
    cfg = (int(groups), int(group_channels), int(kh), int(kw), int(stride), int(dilation), int(pad), float(offset_scale))
    return _DcnJointFn.apply(x_proj, x1, offset_layer.kernel, offset_layer.bias, mask_layer.kernel, mask_layer.bias, cfg)


class _DcnCenterBlendFn(Function):
    @staticmethod
    def forward(ctx, x, x_proj, scale, G, Cg):
        xc, pc, sc = _c(x), _c(x_proj), _c(scale)
        ctx.save_for_backward(xc, pc, sc)
        ctx.geom = (G, Cg)
        return K.dcn_center_blend_fwd(xc, pc, sc, G, Cg)

    @staticmethod
    def backward(ctx, dout):
        xc, pc, sc = ctx.saved_tensors
        dx, dxp, ds = K.dcn_center_blend_bwd(_c(dout), xc, pc, sc, *ctx.geom)
        return dx, dxp, ds, None, None


def dcn_center_blend(x, x_proj, scale, groups, group_channels):
    """centre-feature scale of the DCNv3 layer (layers/dcn_v3/dcn_v3.py:138-146): x (1 - s) + x_proj s, s [N, H, W, groups] broadcast over
    the channels of its group"""
    _check_act_dtype(x)
    if group_channels not in (8, 16):
        raise NotImplementedError("dcn_center_blend: group widths 8 and 16 (the reference's models use 16)")
    if nn.dry_run():
        return _dry(x.shape, x)
    return _DcnCenterBlendFn.apply(x, x_proj, scale, int(groups), int(group_channels))


def dcnv3_core(x, offset, mask, groups, group_channels, kernel_size=(3, 3), stride=1, dilation=1, pad=1, offset_scale=1.0):
    kh, kw = kernel_size
    if nn.dry_run():
        Ho, Wo = K.dcnv3_out_hw(x.shape[1], x.shape[2], kh, kw, stride, dilation, pad)
        return _dry((x.shape[0], Ho, Wo, x.shape[3]), x)
    return _Dcnv3Fn.apply(x, offset, mask, (int(groups), int(group_channels), int(kh), int(kw), int(stride), int(dilation), int(pad),
                                             float(offset_scale)))


class _DeformableAttentionFn(Function):
    """layers/deformable_multihead_self_attention.py:195-240 behind the projections: tanh-bounded offsets, softmax over the points, clipped
    bilinear sampling and the weighted sum as one kernel each way (csrc/defattn.hip); only the three operands are kept for the backward"""

    @staticmethod
    def forward(ctx, value, offset_logits, attn_logits, cfg):
        heads, points, orf = cfg
        vc, oc, ac = _c(value), _c(offset_logits), _c(attn_logits)
        ctx.cfg = cfg
        ctx.save_for_backward(vc, oc, ac)
        return K.defattn_fwd(vc, oc, ac, heads, points, orf)

    @staticmethod
    def backward(ctx, dout):
        vc, oc, ac = ctx.saved_tensors
        heads, points, orf = ctx.cfg
        dvalue, doff, dattn = K.defattn_bwd(vc, oc, ac, _c(dout), heads, points, orf)
        return dvalue, doff, dattn, None


def deformable_attention_core(value, offset_logits, attn_logits, num_heads, num_points, offset_range_factor=8.0):
    """value [N,H,W,Cv], raw offset logits [N,H,W,heads*P*2], raw attention logits [N,H,W,heads*P] -> [N,H,W,Cv]"""
    _check_act_dtype(value)
    heads, points = int(num_heads), int(num_points)
    if heads < 1 or value.shape[-1] % heads != 0:
        raise ValueError(f"deformable_attention_core: {value.shape[-1]} value channels are not divisible by num_heads ({heads})")
    if tuple(offset_logits.shape) != (*value.shape[:3], heads * points * 2) or tuple(attn_logits.shape) != (*value.shape[:3], heads * points):
        raise ValueError(f"deformable_attention_core: offset logits {tuple(offset_logits.shape)} / attention logits {tuple(attn_logits.shape)} do not "
                         f"match value {tuple(value.shape)} with {heads} heads x {points} points")
    if nn.dry_run():
        return _dry(value.shape, value)
    return _DeformableAttentionFn.apply(value, offset_logits, attn_logits, (heads, points, float(offset_range_factor)))


class _GroupSoftmaxFn(Function):
    @staticmethod
    def forward(ctx, x, P):
        xc = _c(x)
        rows = xc.numel() // P
        y = torch.empty_like(xc)
        K.softmax_rows_fwd(xc, rows, 1, P, P, out=y)
        ctx.P = P
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        P = ctx.P
        d = torch.empty_like(y)
        K.softmax_rows_bwd(y, _c(dy), y.numel() // P, P, P, out=d)
        return d, None


def softmax_groups(x, P):
    """softmax over consecutive runs of P entries of the last axis (tf.reshape [..., G, P] -> tf.nn.softmax -> reshape back)"""
    if nn.dry_run():
        return _dry(x.shape, x)
    return _GroupSoftmaxFn.apply(x, int(P))


class _ScaleChannelsFn(Function):
    @staticmethod
    def forward(ctx, x, gamma):
        C = x.shape[-1]
        x2 = _c(x).reshape(-1, C)
        ctx.gamma = gamma
        ctx.save_for_backward(x2)
        return K.scale_cols(x2, gamma.data).reshape(x.shape)

    @staticmethod
    def backward(ctx, dy):
        (x2,) = ctx.saved_tensors
        g = ctx.gamma
        C = x2.shape[1]
        dy2 = _c(dy).reshape(-1, C)
        if g.requires_grad:
            K.mul_colsum(dy2, x2, _grad(g), accumulate=True)
            dist.grads_ready(g)
        return K.scale_cols(dy2, g.data).reshape(dy.shape), None


def scale_channels(x, gamma):
    """x * gamma[c] with an fp32 parameter gamma (layer scale)"""
    if nn.dry_run():
        return _dry(x.shape, x)
    return _ScaleChannelsFn.apply(x, gamma)


# ---------------------------------------------------------------------------------------------------------
# Gemma text backbone (nlp/gemma/*): embedding lookup, packed q | k | v projection, rotary embedding, causal grouped-query attention
# ---------------------------------------------------------------------------------------------------------
class _EmbeddingFn(Function):
    """rows of the embedding table times a scalar (nlp/gemma/gemma_backbone.py:152-153); backward: iseg_embedding_grad over a stable sort of
    the ids -- repeated tokens are added in token order, one workgroup per vocabulary row, no atomics"""

    @staticmethod
    def forward(ctx, ids, table, scale):
        flat = ids.reshape(-1)
        y = K.gather_rows(nn.w(table), flat.to(torch.int32), flat.numel())
        if scale != 1.0:
            y = K.axpby(y, y, alpha=scale, beta=0.0)
        ctx.table, ctx.scale, ctx.ids = table, scale, flat
        return y.reshape(*ids.shape, table.shape[1])

    @staticmethod
    def backward(ctx, dy):
        table = ctx.table
        if table.requires_grad:
            sorted_ids, order = torch.sort(ctx.ids.to(torch.int64), stable=True)
            K.embedding_grad(_c(dy).reshape(-1, table.shape[1]), sorted_ids, order, _grad(table), ctx.scale)
            dist.grads_ready(table)
        return None, None, None


def embedding(ids, table, scale=1.0):
    """table[ids] * scale: ids integer [...], table [vocab, d] parameter -> [..., d] in the compute dtype; `scale` is rounded to that type first
    (gemma_backbone.py:153 casts sqrt(hidden_dim) to the activation type before the product)"""
    dtype = nn.compute_dtype()
    if nn.dry_run():
        return torch.empty((*ids.shape, table.shape[1]), dtype=dtype, device=table.device)
    return _EmbeddingFn.apply(ids, table, float(torch.tensor(float(scale)).to(dtype)))


class _GemmaQkvFn(Function):
    """x [B, T, d] against query/kernel [nq, d, h], key/kernel and value/kernel [nkv, d, h] (EinsumDense "btd,ndh->btnh",
    nlp/gemma/gemma_attention.py:50-75) -> packed [B, T, (nq + 2 nkv) h] = [q heads | k heads | v heads]: strided-batch GEMMs, one problem per head,
    written straight into their column ranges -- ONE launch when the three compute copies lie back to back in memory, else one per kernel"""

    @staticmethod
    def forward(ctx, x, Wq, Wk, Wv):
        d = x.shape[-1]
        x2 = _c(x).reshape(-1, d)
        M = x2.shape[0]
        h = Wq.shape[2]
        heads = [Wq.shape[0], Wk.shape[0], Wv.shape[0]]
        width = sum(heads) * h
        out = torch.empty((M, width), dtype=x2.dtype, device=x2.device)
        ws = [nn.w(W) for W in (Wq, Wk, Wv)]
        es = ws[0].element_size()
        joined = all(a.is_contiguous() for a in ws) and all(ws[i].data_ptr() + ws[i].numel() * es == ws[i + 1].data_ptr() for i in range(2))
        runs = [(ws[0], sum(heads), 0)] if joined else [(ws[i], heads[i], sum(heads[:i]) * h) for i in range(3)]
        for Wc, n, col in runs:
            K.gemm(x2, Wc, out[:, col:], M, h, d, lda=d, ldb=h, ldd=width, a_kcontig=1, b_kcontig=0, batch=n, batch_inner=1, sa=(0, 0),
                   sb=(d * h, 0), sd=(h, 0))
        ctx.params = (Wq, Wk, Wv)
        ctx.save_for_backward(x2)
        return out.reshape(*x.shape[:-1], width)

    @staticmethod
    def backward(ctx, dy):
        (x2,) = ctx.saved_tensors
        M, d = x2.shape
        dy2 = _c(dy).reshape(M, -1)
        h = ctx.params[0].shape[2]
        dx = torch.empty((M, d), dtype=torch.float32, device=x2.device) if ctx.needs_input_grad[0] else None
        col, first = 0, True
        for W in ctx.params:      # one head at a time: the weight gradient into its fp32 slice, the data gradient summed in fp32
            Wc = nn.w(W)
            for n in range(W.shape[0]):
                dyn = dy2[:, col:col + h]
                if W.requires_grad:
                    K.dense_wgrad(x2, dyn, _grad(W)[n])
                if dx is not None:
                    K.dense_dgrad(dyn, Wc[n], out=dx, accumulate=not first)
                    first = False
                col += h
        dist.grads_ready(*ctx.params)
        if dx is not None:
            dx = (dx if x2.dtype == torch.float32 else K.cast(dx, x2.dtype)).reshape(*dy.shape[:-1], d)
        return dx, None, None, None


def gemma_qkv(x, Wq, Wk, Wv):
    _check_act_dtype(x)
    if nn.dry_run():
        return _dry((*x.shape[:-1], (Wq.shape[0] + Wk.shape[0] + Wv.shape[0]) * Wq.shape[2]), x)
    return _GemmaQkvFn.apply(x, Wq, Wk, Wv)


_GEMMA_ROPE_TABLES = {}


def gemma_rope_table(T, h, device):
    """fp32 [T, h] = [sin(t / 10000^(2i/h)) | cos(...)], i < h/2 (nlp/gemma/gemma_attention.py:99-107), built once per (T, h, device).  The angles
    are formed in fp32 whatever the storage type: in bf16 (the reference's compute dtype) positions above 256 are not representable"""
    key = (int(T), int(h), str(device))
    tab = _GEMMA_ROPE_TABLES.get(key)
    if tab is None:
        exponents = (2.0 / h) * torch.arange(h // 2, dtype=torch.float32)
        timescale = torch.pow(torch.tensor(10000.0), exponents)
        radians = torch.arange(T, dtype=torch.float32)[:, None] / timescale[None, :]
        tab = _GEMMA_ROPE_TABLES[key] = torch.cat([torch.sin(radians), torch.cos(radians)], dim=1).contiguous().to(device)
    return tab


class _GemmaRopeFn(Function):
    """the interleaved rotary embedding on the q and k heads of packed rows (csrc/gemma.hip; gemma_attention.py:96-114); backward: the transposed
    rotation on the gradient"""

    @staticmethod
    def forward(ctx, qkv, table, nq, nkv, h):
        ctx.table, ctx.geom = table, (qkv.shape[1], nq, nkv, h)
        src = _c(qkv)
        return K.gemma_rope(src, table, qkv.shape[1], nq, nkv, h, out=torch.empty_like(src))

    @staticmethod
    def backward(ctx, d):
        T, nq, nkv, h = ctx.geom
        d = _c(d)
        return K.gemma_rope(d, ctx.table, T, nq, nkv, h, inverse=True, out=torch.empty_like(d)), None, None, None, None


def gemma_rope(qkv, nq, nkv, h):
    """qkv [B, T, (nq + 2 nkv) h], positions 0 .. T-1: out[2i] = x1 cos - x2 sin, out[2i+1] = x2 cos + x1 sin per q / k head, v unchanged"""
    _check_act_dtype(qkv)
    if nn.dry_run():
        return qkv
    if qkv.dim() != 3 or qkv.shape[2] != (nq + 2 * nkv) * h or h % 2:
        raise ValueError(f"gemma_rope: {tuple(qkv.shape)} is not [B, T, ({nq} + 2 * {nkv}) * {h}]")
    return _GemmaRopeFn.apply(qkv, gemma_rope_table(qkv.shape[1], h, qkv.device), int(nq), int(nkv), int(h))


class _GemmaAttentionFn(Function):
    """causal grouped-query attention with a key padding mask on the fused kernels of csrc/gemma.hip: online softmax, one log-sum-exp float per
    (token, query head), probabilities recomputed in the backward kernels; nothing of size T x T"""

    @staticmethod
    def forward(ctx, qkv, mask_u8, nq, nkv, h, scale):
        qkv = _c(qkv)
        out, lse = K.gemma_attention_fwd(qkv, mask_u8, nq, nkv, h, scale, True)
        ctx.cfg = (nq, nkv, h, scale)
        ctx.mask = mask_u8
        ctx.save_for_backward(qkv, out, lse)
        return out

    @staticmethod
    def backward(ctx, dO):
        qkv, out, lse = ctx.saved_tensors
        nq, nkv, h, scale = ctx.cfg
        return K.gemma_attention_bwd(qkv, ctx.mask, out, _c(dO), lse, nq, nkv, h, scale), None, None, None, None, None


class _GemmaRepeatKVFn(Function):
    """packed [q | k | v] with nkv key/value heads -> [q | k' | v'] with nq: query head n gets key/value head n // (nq / nkv) (the composed route's
    way to the equal-head-count operator); backward: the group's gradients added back in head order"""

    @staticmethod
    def forward(ctx, qkv, nq, nkv, h):
        B, T, W = qkv.shape
        src = _c(qkv).reshape(B * T, W)
        g, Cq = nq // nkv, nq * h
        out = torch.empty((B * T, 3 * Cq), dtype=src.dtype, device=src.device)
        K.copy2d(src, W, out, 3 * Cq, B * T, Cq)
        for part in range(2):
            for n in range(nq):
                K.copy2d(src[:, Cq + (part * nkv + n // g) * h:], W, out[:, (1 + part) * Cq + n * h:], 3 * Cq, B * T, h)
        ctx.geom = (nq, nkv, h)
        return out.reshape(B, T, 3 * Cq)

    @staticmethod
    def backward(ctx, d):
        nq, nkv, h = ctx.geom
        B, T, _ = d.shape
        g, Cq, W = nq // nkv, nq * h, (nq + 2 * nkv) * h
        d2 = _c(d).reshape(B * T, 3 * Cq)
        out = torch.empty((B * T, W), dtype=d2.dtype, device=d2.device)
        K.copy2d(d2, 3 * Cq, out, W, B * T, Cq)
        for part in range(2):
            for kv in range(nkv):
                acc = None
                for j in range(g):
                    piece = torch.empty((B * T, h), dtype=d2.dtype, device=d2.device)
                    K.copy2d(d2[:, (1 + part) * Cq + (kv * g + j) * h:], 3 * Cq, piece, h, B * T, h)
                    acc = piece if acc is None else K.axpby(acc, piece)
                K.copy2d(acc, h, out[:, Cq + (part * nkv + kv) * h:], W, B * T, h)
        return out.reshape(B, T, W), None, None, None


def _gemma_visibility(padding_mask, B, T, device):
    """bool [B, T, T]: key s visible to query t iff s <= t and padding_mask[b, s] != 0 (gemma_decoder_block.py:114-136)"""
    vis = torch.ones((T, T), dtype=torch.bool, device=device).tril()[None].expand(B, T, T)
    if padding_mask is not None:
        vis = vis & (padding_mask.reshape(B, 1, T) != 0)
    return vis


def gemma_attention_fused(nq, nkv, h, dtype):
    """True where gemma_attention_core takes the fused kernels: supported shape and type, and ISEG_GEMMA_FUSED unset or not "0" """
    return os.environ.get("ISEG_GEMMA_FUSED", "1") != "0" and nq % max(nkv, 1) == 0 and K.gemma_attention_supported(nq, nkv, h, dtype)


def gemma_attention_core(qkv, padding_mask, nq, nkv, h, *, dropout_rate=0.0, training=False):
    """qkv [B, T, (nq + 2 nkv) h] = [q heads | k heads | v heads] (after the rotary embedding), padding_mask [B, T] (non-zero = real token) or None
    -> [B, T, nq h]: softmax(h^-0.5 q k^T) v per query head n on key/value head n // (nq / nkv), over the keys s <= t with padding_mask[b, s] != 0,
    softmax in fp32 (nlp/gemma/gemma_attention.py:116-151); a query row with no visible key gives zeros and passes no gradient (:189-195).
    Fused route (bf16, h in 64, 128, 192, 256, nq % nkv == 0, no dropout on the probabilities in effect, ISEG_GEMMA_FUSED unset or not "0"):
    csrc/gemma.hip.  Composed route (everything else, and the yardstick of the fused one): K and V repeated per group, attention_packed with an additive fp32 mask per sample, rows without
    a visible key wiped."""
    _check_act_dtype(qkv)
    if qkv.dim() != 3 or qkv.shape[2] != (nq + 2 * nkv) * h or nq % nkv:
        raise ValueError(f"gemma_attention_core: {tuple(qkv.shape)} is not [B, T, ({nq} + 2 * {nkv}) * {h}] with nq a multiple of nkv")
    B, T, _ = qkv.shape
    if nn.dry_run():
        return _dry((B, T, nq * h), qkv)
    scale = float(h) ** -0.5
    rate = float(dropout_rate) if training else 0.0
    if rate <= 0 and gemma_attention_fused(nq, nkv, h, qkv.dtype):
        mask_u8 = None if padding_mask is None else (padding_mask.reshape(B, T) != 0).to(torch.uint8).contiguous()
        if not (torch.is_grad_enabled() and qkv.requires_grad):
            return K.gemma_attention_fwd(_c(qkv), mask_u8, int(nq), int(nkv), int(h), scale, False)[0]
        return _GemmaAttentionFn.apply(qkv, mask_u8, int(nq), int(nkv), int(h), scale)
    return _gemma_attention_composed(qkv, padding_mask, nq, nkv, h, scale, rate)


def _gemma_attention_composed(qkv, padding_mask, nq, nkv, h, scale, rate=0.0):
    """the composed route of gemma_attention_core"""
    B, T, _ = qkv.shape
    vis = _gemma_visibility(padding_mask, B, T, qkv.device)
    additive = torch.where(vis, 0.0, -1e30).to(torch.float32).contiguous()
    wide = _GemmaRepeatKVFn.apply(qkv, int(nq), int(nkv), int(h)) if nkv != nq else qkv
    y = attention_packed(wide, nq, nq * h, nq * h, scale, mask=additive, windows=B, dropout_rate=rate, training=rate > 0)
    if padding_mask is None:      # causal only: every row sees itself
        return y
    alive = vis.any(dim=-1).to(torch.float32).reshape(B * T).contiguous()
    return _RowScaleFn.apply(y.reshape(B * T, nq * h), alive).reshape(B, T, nq * h)


# ---- Gemma with a key/value cache (nlp/gemma/gemma_causal.py:186-226): inference only, no autograd graph -----------------------------------
def _no_grad_inputs(who, *ts):
    for t in ts:
        if t.requires_grad:
            raise RuntimeError(f"{who}: the cached path is inference only (an input requires grad); train through the uncached call")


def _check_device_position(who, pos0, Tn, S):
    if pos0.dtype != torch.int32 or pos0.numel() != 1:
        raise ValueError(f"{who}: a tensor position is ONE int32 element in device memory, got {tuple(pos0.shape)} {pos0.dtype}")
    if Tn > S:
        raise ValueError(f"{who}: {Tn} new rows do not fit a cache of {S} rows")


def _check_layer_cache(who, cache, B, nkv, h, dtype):
    if cache.dim() != 5 or cache.shape[0] != B or cache.shape[1] != 2 or cache.shape[3] != nkv or cache.shape[4] != h or cache.dtype != dtype:
        raise ValueError(f"{who}: a layer's cache is [{B}, 2, S, {nkv}, {h}] {dtype}, got {tuple(cache.shape)} {cache.dtype}")


def gemma_rope_cache(qkv, cache, pos0, nq, nkv, h):
    """qkv [B, Tn, (nq + 2 nkv) h]: packed projections of the tokens at positions pos0 .. pos0 + Tn - 1; cache: ONE layer's [B, 2, S, nkv, h] view of
    the [B, num_layers, 2, S, nkv, h] cache.  The rotary embedding at those positions (fp32 angles from gemma_rope_table(S, h)) and the
    dynamic_update_slice of nlp/gemma/gemma_attention.py:161-179 in one pass (csrc/gemma_decode.hip): rows pos0 .. of the cache receive the rotated
    keys and the values IN PLACE, the rotated queries are returned [B, Tn, nq h].
    pos0 is an int, or a one-element int32 DEVICE tensor that the kernel reads when it runs (iseg_gemma_rope_cache_at: the same bits, and a
    captured graph follows the tensor).  The host cannot range-check a device value and does not pretend to: outside [0, S - Tn] the kernel
    touches nothing."""
    _check_act_dtype(qkv)
    _no_grad_inputs("gemma_rope_cache", qkv, cache)
    if qkv.dim() != 3 or qkv.shape[2] != (nq + 2 * nkv) * h or h % 2:
        raise ValueError(f"gemma_rope_cache: {tuple(qkv.shape)} is not [B, Tn, ({nq} + 2 * {nkv}) * {h}]")
    B, Tn, _ = qkv.shape
    if nn.dry_run():
        return _dry((B, Tn, nq * h), qkv)
    _check_layer_cache("gemma_rope_cache", cache, B, nkv, h, qkv.dtype)
    S = cache.shape[2]
    if torch.is_tensor(pos0):
        _check_device_position("gemma_rope_cache", pos0, Tn, S)
        with torch.no_grad():
            return K.gemma_rope_cache_at(_c(qkv), cache, gemma_rope_table(S, h, qkv.device), pos0, int(nq), int(nkv), int(h))
    if pos0 < 0 or pos0 + Tn > S:
        raise ValueError(f"gemma_rope_cache: positions {pos0} .. {pos0 + Tn - 1} do not lie inside a cache of {S} rows")
    with torch.no_grad():
        return K.gemma_rope_cache(_c(qkv), cache, gemma_rope_table(S, h, qkv.device), int(pos0), int(nq), int(nkv), int(h))


def gemma_cached_attention_fused(Tn, nq, nkv, h, dtype):
    """True where gemma_cached_attention_core takes the decode kernels: supported shape and type, and ISEG_GEMMA_FUSED unset or not "0" """
    return os.environ.get("ISEG_GEMMA_FUSED", "1") != "0" and nq % max(nkv, 1) == 0 and K.gemma_decode_attention_supported(Tn, nq, nkv, h, dtype)


def gemma_cached_attention_core(q, cache, pos0, nq, nkv, h, *, splits=0):
    """q [B, Tn, nq h]: rotated queries of the tokens at positions pos0 .. pos0 + Tn - 1; cache [B, 2, S, nkv, h]: one layer's keys and values,
    rows 0 .. pos0 + Tn - 1 filled (gemma_rope_cache) -> [B, Tn, nq h]: softmax(h^-0.5 q k^T) v over the keys s <= pos0 + t, the mask of
    gemma_decoder_block.py:114-136 with a cache and no padding mask.
    Fused route (bf16, h in 64 .. 256, (nq / nkv) * Tn <= 16, ISEG_GEMMA_FUSED unset or not "0"): the split-KV kernels of csrc/gemma_decode.hip;
    rows of the cache past pos0 + Tn - 1 are never read.
    Seeding call (pos0 == 0, Tn == S, too many rows for the decode kernels): gemma_attention_core on the packed [q | K | V] rows with no
    padding mask -- at index 0 with the whole cache the cached mask is the plain causal mask.
    Composed route (everything else, and the yardstick of the fused one): the new q rows at rows pos0 .. of a zeroed packed [B, S, .] buffer
    beside the cache's visible K and V rows, the composed route of gemma_attention_core, and the rows sliced out: the causal mask of row
    pos0 + t is exactly the cached mask.
    pos0 is an int, or a one-element int32 DEVICE tensor that the kernels read when they run (iseg_gemma_decode_attention_at: bit for bit the
    int call at that position, from a grid and a workspace sized for the cache's capacity).  A tensor position takes the fused route alone: the
    seeding and composed routes slice on the host and raise ValueError, and no host-side range check is made."""
    _check_act_dtype(q)
    _no_grad_inputs("gemma_cached_attention_core", q, cache)
    if q.dim() != 3 or q.shape[2] != nq * h or nq % nkv:
        raise ValueError(f"gemma_cached_attention_core: {tuple(q.shape)} is not [B, Tn, {nq} * {h}] with nq a multiple of nkv")
    B, Tn, _ = q.shape
    if torch.is_tensor(pos0) and not gemma_cached_attention_fused(Tn, nq, nkv, h, q.dtype):
        raise ValueError(f"gemma_cached_attention_core: a tensor position needs the fused decode kernels (bf16, head width 64 .. 256 in steps of "
                         f'64, (nq / nkv) * Tn <= 16, ISEG_GEMMA_FUSED unset or not "0"), got Tn {Tn}, nq {nq}, nkv {nkv}, h {h}, {q.dtype}; the '
                         "composed and seeding routes need the position on the host")
    if nn.dry_run():
        return _dry(q.shape, q)
    _check_layer_cache("gemma_cached_attention_core", cache, B, nkv, h, q.dtype)
    S = cache.shape[2]
    if torch.is_tensor(pos0):
        _check_device_position("gemma_cached_attention_core", pos0, Tn, S)
        with torch.no_grad():
            return K.gemma_decode_attention_at(_c(q), cache, pos0, int(nq), int(nkv), int(h), float(h) ** -0.5, splits)
    if pos0 < 0 or pos0 + Tn > S:
        raise ValueError(f"gemma_cached_attention_core: positions {pos0} .. {pos0 + Tn - 1} do not lie inside a cache of {S} rows")
    scale = float(h) ** -0.5
    with torch.no_grad():
        if gemma_cached_attention_fused(Tn, nq, nkv, h, q.dtype):
            return K.gemma_decode_attention(_c(q), cache, int(pos0), int(nq), int(nkv), int(h), scale, splits)
        nvis, Cq, Ck = pos0 + Tn, nq * h, nkv * h
        packed = torch.zeros((B, S, Cq + 2 * Ck), dtype=q.dtype, device=q.device)
        packed[:, pos0:nvis, :Cq] = q
        packed[:, :nvis, Cq:Cq + Ck] = cache[:, 0, :nvis].reshape(B, nvis, Ck)
        packed[:, :nvis, Cq + Ck:] = cache[:, 1, :nvis].reshape(B, nvis, Ck)
        if pos0 == 0 and Tn == S:
            return gemma_attention_core(packed, None, nq, nkv, h)
        return _c(_gemma_attention_composed(packed, None, int(nq), int(nkv), int(h), scale)[:, pos0:nvis])


_SAMPLE_MODES = {"random": K.SAMPLE_RANDOM, "top_k": K.SAMPLE_TOP_K, "top_p": K.SAMPLE_TOP_P}
SAMPLE_MAX_VOCAB = 1 << 20


def sample_tokens(logits, u, *, mode, k=0, p=1.0, temperature=1.0, splits=0):
    """logits [B, V] or a [B, 1, V] view (bf16 or fp32, rows of contiguous elements with any pitch), u fp32 [B] uniform in [0, 1) -> int32 [B]: one
    token per row from softmax(logits / temperature) restricted to the kept set of `mode` (csrc/token_sample.hip, two launches):
      "random"  every token;  "top_k"  the k largest logits;  "top_p"  among the k largest (k = 0: all), those whose preceding softmax mass is <= p.
    Ties are ordered by index; the draw walks the kept tokens in token-id order to the first whose cumulative weight exceeds u times their sum;
    a row whose largest entry is NaN, +inf or -inf returns torch.argmax's index (include/iseg_hip.h has the full statement).  The random number
    is the caller's: the same u gives the same token.  Inference only; there is no torch route."""
    if mode not in _SAMPLE_MODES:
        raise ValueError(f"sample_tokens: mode is one of {sorted(_SAMPLE_MODES)}, got {mode!r}")
    if logits.requires_grad:
        raise RuntimeError("sample_tokens: sampling is inference only (the logits require grad)")
    if logits.dim() == 3 and logits.shape[1] == 1:
        logits = logits[:, 0]
    if logits.dim() != 2 or u.dim() != 1 or u.shape[0] != logits.shape[0]:
        raise ValueError(f"sample_tokens: logits is [B, V] or [B, 1, V] and u is [B], got {tuple(logits.shape)} and {tuple(u.shape)}")
    B, V = logits.shape
    k, p, temperature = int(k), float(p), float(temperature)
    if logits.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError(f"sample_tokens: logits are bfloat16 or float32, got {logits.dtype}")
    if u.dtype != torch.float32:
        raise ValueError(f"sample_tokens: u is float32, got {u.dtype}")
    if not 1 <= V <= SAMPLE_MAX_VOCAB:
        raise ValueError(f"sample_tokens: the vocabulary is 1 .. {SAMPLE_MAX_VOCAB} entries, got {V}")
    if k < 0 or (mode == "top_k" and k < 1):
        raise ValueError(f"sample_tokens: k >= 0, and k >= 1 for top_k, got {k}")
    if not (temperature > 0.0 and math.isfinite(temperature)):
        raise ValueError(f"sample_tokens: temperature must be positive and finite, got {temperature}")
    if not 0.0 < p <= 1.0:
        raise ValueError(f"sample_tokens: p must lie in (0, 1], got {p}")
    if nn.dry_run():
        return _dry((B,), logits, torch.int32)
    if B == 0:
        return torch.empty((0,), dtype=torch.int32, device=logits.device)
    if logits.stride(1) != 1 or (B > 1 and logits.stride(0) < V):
        logits = logits.contiguous()
    with torch.no_grad():
        return K.token_sample(logits, _c(u), _SAMPLE_MODES[mode], k, p, temperature, splits)


BEAM_MAX_BEAMS = 16


def beam_fused():
    """True where a beam step on device tensors takes the kernels of csrc/beam_search.hip: ISEG_BEAM_FUSED unset or not "0" """
    return os.environ.get("ISEG_BEAM_FUSED", "1") != "0"


def _topk_ordered(values, k):
    """the k first entries of every row in the order value descending, then index ascending, NaN above every number -> (values, indices)"""
    N = values.shape[-1]
    key = torch.nan_to_num(values, nan=math.inf, posinf=math.inf, neginf=-math.inf)
    nth = torch.topk(key, k, dim=-1).values[:, -1:]
    # everything above the k-th value, then that value's ties, each by index: all ranks are distinct, so this top-k is a set
    rank = (key > nth).to(torch.int64) * (2 * N) + (key == nth).to(torch.int64) * N + (N - 1 - torch.arange(N, device=values.device))
    idx = torch.topk(rank, k, dim=-1).indices
    idx = idx.gather(-1, torch.sort(key.gather(-1, idx), dim=-1, descending=True, stable=True).indices)
    return values.gather(-1, idx), idx


def _beam_select_composed(logits, log_probs, nb, temperature):
    """keras_nlp's op sequence in plain torch: the fp32 log-softmax of logits / T plus the running score, [B, nb V], top-k.  The order is pinned
    down as the kernel's: score descending, ties by flat index ascending, NaN above every number"""
    R, V = logits.shape
    B, N = R // nb, nb * V
    scores = (torch.log_softmax(logits.to(torch.float32) / temperature, dim=-1) + log_probs[:, None]).reshape(B, N)
    best, flat = _topk_ordered(scores, nb)
    return ((flat // V).to(torch.int32).reshape(R), (flat % V).to(torch.int32).reshape(R), best.reshape(R))


def beam_select(logits, log_probs, num_beams, temperature=1.0, splits=0):
    """One selection of keras_nlp.samplers.BeamSampler.  logits [B nb, V] or a [B nb, 1, V] view (row b nb + j is beam j of batch row b), log_probs
    fp32 [B nb] the beams' running scores -> (parents int32, tokens int32, new log_probs fp32), each [B nb]: per batch row the nb best of the
    nb V candidates (beam j, token v) with score log_softmax(logits[j] / temperature)[v] + log_probs[j], sorted by score descending, ties by
    flat index j V + v ascending; parents are beam indices inside the batch row.  NaN ranks above every number; a row with a NaN or +inf logit
    scores NaN throughout; a -inf logit scores -inf (include/iseg_hip.h has the full statement).
    Device tensors in bf16 or fp32 with V <= 2^20 take the kernels of csrc/beam_search.hip (two launches, the logits read once, no [B nb, V]
    intermediate); CPU tensors, other dtypes and ISEG_BEAM_FUSED=0 the composed route, the reference's op sequence in torch.  Inference only."""
    if logits.requires_grad:
        raise RuntimeError("beam_select: beam search is inference only (the logits require grad)")
    if logits.dim() == 3 and logits.shape[1] == 1:
        logits = logits[:, 0]
    if isinstance(num_beams, bool) or not isinstance(num_beams, int) or not 1 <= num_beams <= BEAM_MAX_BEAMS:
        raise ValueError(f"beam_select: num_beams is an integer in 1 .. {BEAM_MAX_BEAMS}, got {num_beams!r}")
    if logits.dim() != 2 or log_probs.dim() != 1 or log_probs.shape[0] != logits.shape[0] or logits.shape[0] % num_beams:
        raise ValueError(f"beam_select: logits is [B * {num_beams}, V] or [B * {num_beams}, 1, V] and log_probs is [B * {num_beams}], got "
                         f"{tuple(logits.shape)} and {tuple(log_probs.shape)}")
    R, V = logits.shape
    temperature = float(temperature)
    if not logits.dtype.is_floating_point:
        raise ValueError(f"beam_select: logits are floating point, got {logits.dtype}")
    if log_probs.dtype != torch.float32:
        raise ValueError(f"beam_select: log_probs is float32, got {log_probs.dtype}")
    if V < 1:
        raise ValueError("beam_select: the vocabulary is empty")
    if not (temperature > 0.0 and math.isfinite(temperature)):
        raise ValueError(f"beam_select: temperature must be positive and finite, got {temperature}")
    if nn.dry_run():
        return _dry((R,), logits, torch.int32), _dry((R,), logits, torch.int32), _dry((R,), logits, torch.float32)
    with torch.no_grad():
        if R == 0:
            return (torch.empty((0,), dtype=torch.int32, device=logits.device), torch.empty((0,), dtype=torch.int32, device=logits.device),
                    torch.empty((0,), dtype=torch.float32, device=logits.device))
        if logits.is_cuda and beam_fused() and logits.dtype in (torch.bfloat16, torch.float32) and V <= SAMPLE_MAX_VOCAB:
            if logits.stride(1) != 1 or (R > 1 and logits.stride(0) < V):
                logits = logits.contiguous()
            return K.beam_select(logits, _c(log_probs), num_beams, temperature, splits)
        return _beam_select_composed(logits, log_probs, num_beams, temperature)


def beam_reorder(cache, prompt, mask, parents, tokens, index, num_beams, length=None):
    """keras_nlp's gather_beams after a selection, and the step's token write -> (cache, prompt).  cache [B nb, L, 2, Sc, nkv, h] or None (Sc: the
    cache's own number of positions, which need not be the prompt's S), prompt [B nb, S] int32 or int64, mask [B nb, S] bool (true = a user token), parents and tokens int32 [B nb] as beam_select returns them:
        cache[b nb + j] = cache[b nb + parents[b nb + j]];  prompt likewise;  prompt[:, index] = mask[:, index] ? prompt[:, index] : tokens.
    length: the number of filled cache positions (default `index`: call_with_cache's step `index` writes position index - 1).
    On device tensors (csrc/beam_search.hip) both are updated IN PLACE and returned: only the positions < length of the cache move, a beam
    that is its own parent moves nothing, and no second cache exists; this relies on the positions >= length being equal among the beams of
    a batch row, as they are when the cache was repeated from one row.  A group with a parent outside [0, nb) is left untouched.  CPU tensors,
    a cache that is not contiguous or whose [nkv, h] rows are no multiple of 16 bytes, a prompt or mask whose rows overlap (an expanded
    view) and ISEG_BEAM_FUSED=0 take the composed route: new tensors, the whole cache gathered, as the reference does.  All tensors lie on
    one device."""
    nb, index = int(num_beams), int(index)
    if prompt.dim() != 2 or prompt.dtype not in (torch.int32, torch.int64) or tuple(mask.shape) != tuple(prompt.shape) or mask.dtype != torch.bool:
        raise ValueError(f"beam_reorder: prompt is an int32 or int64 [B * nb, S] and mask a bool tensor of its shape, got {tuple(prompt.shape)} "
                         f"{prompt.dtype} and {tuple(mask.shape)} {mask.dtype}")
    R, S = prompt.shape
    if not 1 <= nb <= BEAM_MAX_BEAMS or R % nb:
        raise ValueError(f"beam_reorder: {R} rows are no whole number of groups of {nb} beams (1 .. {BEAM_MAX_BEAMS})")
    for name, t in (("parents", parents), ("tokens", tokens)):
        if tuple(t.shape) != (R,) or t.dtype != torch.int32:
            raise ValueError(f"beam_reorder: {name} is an int32 [{R}], got {tuple(t.shape)} {t.dtype}")
    if not 0 <= index < S:
        raise ValueError(f"beam_reorder: position {index} does not lie inside a prompt of {S}")
    if cache is None:
        length = 0
    else:
        if not torch.is_tensor(cache) or cache.dim() != 6 or cache.shape[0] != R:
            raise ValueError(f"beam_reorder: the cache is a [{R}, L, 2, S, nkv, h] tensor or None, got {tuple(cache.shape) if torch.is_tensor(cache) else cache!r}")
        length = index if length is None else int(length)
        if not 0 <= length <= cache.shape[3]:
            raise ValueError(f"beam_reorder: {length} filled positions do not lie inside a cache of {cache.shape[3]}")
    for name, t in (("mask", mask), ("parents", parents), ("tokens", tokens), ("cache", cache)):
        if t is not None and t.device != prompt.device:
            raise ValueError(f"beam_reorder: {name} lies on {t.device}, the prompt on {prompt.device}")
    if nn.dry_run() or R == 0:
        return cache, prompt
    with torch.no_grad():
        fused = (prompt.is_cuda and beam_fused() and prompt.stride(1) == 1 and mask.stride(1) == 1
                 and (R == 1 or (prompt.stride(0) >= S and mask.stride(0) >= S)))
        if fused and cache is not None:
            fused = (cache.is_cuda and cache.is_contiguous() and cache.data_ptr() % 16 == 0
                     and (cache.shape[4] * cache.shape[5] * cache.element_size()) % 16 == 0)
        if fused:
            K.beam_reorder(cache, length, prompt, mask, _c(tokens), index, _c(parents), nb)
            return cache, prompt
        rows = (torch.arange(R, device=prompt.device) // nb * nb + parents).to(torch.int64)
        prompt = prompt.index_select(0, rows)
        prompt[:, index] = torch.where(mask[:, index], prompt[:, index], tokens.to(prompt.dtype))
        return (None if cache is None else cache.index_select(0, rows)), prompt


CONTRASTIVE_MAX_K = 16


def contrastive_fused():
    """True where a contrastive step on device tensors takes the kernels of csrc/contrastive.hip: ISEG_CONTRASTIVE_FUSED unset or not "0" """
    return os.environ.get("ISEG_CONTRASTIVE_FUSED", "1") != "0"


def _check_contrastive_k(who, k):
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= CONTRASTIVE_MAX_K:
        raise ValueError(f"{who}: k is an integer in 1 .. {CONTRASTIVE_MAX_K}, got {k!r}")


def contrastive_candidates(logits, k, temperature=1.0, row_map=None, splits=0):
    """The candidates of one step of keras_nlp.samplers.ContrastiveSampler.  logits [R, V] or a [R, 1, V] view -> (probs fp32 [B, k], tokens int32
    [B, k]): the k largest of softmax(logits / temperature) per output row, in fp32, probability descending, ties by token id ascending.
    row_map None: B = R.  row_map int32 [B] with R = B g: output row b reads logits row b g + row_map[b] (values in [0, g)), which is how a step
    reads the previous step's winners out of its [B k, V] logits.  A row whose largest logit is NaN or +inf has NaN probabilities and the
    tokens 0 .. k - 1 (include/iseg_hip.h has the full statement).
    Device tensors in bf16 or fp32 with V <= 2^20 take the kernels of csrc/contrastive.hip (two launches, the logits read once, no [B, V]
    tensor, no gather); CPU tensors, other dtypes and ISEG_CONTRASTIVE_FUSED=0 the composed route, the reference's op sequence in torch in
    fp32.  Inference only."""
    if logits.requires_grad:
        raise RuntimeError("contrastive_candidates: contrastive search is inference only (the logits require grad)")
    if logits.dim() == 3 and logits.shape[1] == 1:
        logits = logits[:, 0]
    _check_contrastive_k("contrastive_candidates", k)
    if logits.dim() != 2:
        raise ValueError(f"contrastive_candidates: logits is [R, V] or [R, 1, V], got {tuple(logits.shape)}")
    R, V = logits.shape
    temperature = float(temperature)
    if not logits.dtype.is_floating_point:
        raise ValueError(f"contrastive_candidates: logits are floating point, got {logits.dtype}")
    if V < 1 or k > V:
        raise ValueError(f"contrastive_candidates: k = {k} candidates need a vocabulary of at least k entries, got {V}")
    if not (temperature > 0.0 and math.isfinite(temperature)):
        raise ValueError(f"contrastive_candidates: temperature must be positive and finite, got {temperature}")
    B = R
    if row_map is not None:
        if row_map.dim() != 1 or row_map.dtype != torch.int32 or row_map.device != logits.device:
            raise ValueError(f"contrastive_candidates: row_map is an int32 [B] on the logits' device, got {tuple(row_map.shape)} {row_map.dtype} on "
                             f"{row_map.device}")
        B = row_map.shape[0]
        if (B == 0 and R != 0) or (B > 0 and R % B):
            raise ValueError(f"contrastive_candidates: {R} logits rows are no whole number of groups for {B} output rows")
    if nn.dry_run():
        return _dry((B, k), logits, torch.float32), _dry((B, k), logits, torch.int32)
    with torch.no_grad():
        if B == 0:
            return (torch.empty((0, k), dtype=torch.float32, device=logits.device), torch.empty((0, k), dtype=torch.int32, device=logits.device))
        if logits.is_cuda and contrastive_fused() and logits.dtype in (torch.bfloat16, torch.float32) and V <= SAMPLE_MAX_VOCAB:
            if logits.stride(1) != 1 or (R > 1 and logits.stride(0) < V):
                logits = logits.contiguous()
            return K.contrastive_candidates(logits, k, temperature, None if row_map is None else _c(row_map), splits)
        if row_map is not None:
            g = R // B
            logits = logits.index_select(0, torch.arange(B, device=logits.device) * g + row_map.clamp(0, g - 1).to(torch.int64))
        probs, tokens = _topk_ordered(torch.softmax(logits.to(torch.float32) / temperature, dim=-1), k)
        dead = torch.isnan(probs).any(dim=-1, keepdim=True)      # a NaN row: every token ties, the first k ids
        tokens = torch.where(dead, torch.arange(k, device=logits.device).expand(B, k), tokens)
        return torch.where(dead, torch.full_like(probs, math.nan), probs), tokens.to(torch.int32)


def _contrastive_select_composed(hidden_states, index, cand_hidden, probs, alpha, k):
    """keras_nlp's op sequence in plain torch, in fp32: the history repeated k times, one batched matmul, the norms, the division, max, the score,
    argmax (the first maximal score; NaN above every number)"""
    B = hidden_states.shape[0]
    h1 = torch.repeat_interleave(hidden_states[:, :index].to(torch.float32), k, dim=0)      # [B k, index, D]
    h2 = cand_hidden.to(torch.float32)[:, :, None]                                            # [B k, D, 1]
    sim = torch.matmul(h1, h2)[:, :, 0] / (torch.linalg.vector_norm(h1, dim=-1) * torch.linalg.vector_norm(h2, dim=-2))
    max_sim = torch.max(sim, dim=-1).values
    scores = (1.0 - alpha) * probs - alpha * max_sim
    return torch.argmax(scores.view(B, k), dim=-1).to(torch.int32), scores, max_sim


def contrastive_select(hidden_states, index, cand_hidden, probs, alpha, splits=0):
    """The selection of one step of keras_nlp.samplers.ContrastiveSampler.  hidden_states [B, S, D] (its first `index` positions hold the hidden
    states of the tokens so far; later positions are never read), cand_hidden [B k, D] (row b k + j: the hidden state of candidate j of batch
    row b), probs fp32 [B k] the candidates' probabilities, 0 <= alpha <= 1 -> (winner int32 [B], scores fp32 [B k], max_sim fp32 [B k]):
        max_sim = max over t < index of the cosine similarity of hidden_states[b, t] and the candidate (fp32, no epsilon: a zero vector gives NaN),
        scores = (1 - alpha) probs - alpha max_sim,   winner[b] = the first maximal score of the row's k (NaN ranks above every number).
    Device tensors in bf16 or fp32 with D a multiple of 8 (up to 16384) take the kernels of csrc/contrastive.hip: one pass over the filled
    prefix, the row's candidates resident in LDS, no [B k, index] similarity matrix, results bit-identical for every `splits`.  CPU tensors,
    other shapes and dtypes and ISEG_CONTRASTIVE_FUSED=0 take the composed route, the reference's op sequence in torch in fp32.  Inference
    only."""
    who = "contrastive_select"
    for t in (hidden_states, cand_hidden, probs):
        if t.requires_grad:
            raise RuntimeError(f"{who}: contrastive search is inference only (an input requires grad)")
    if hidden_states.dim() != 3 or cand_hidden.dim() != 2 or cand_hidden.shape[1] != hidden_states.shape[2]:
        raise ValueError(f"{who}: hidden_states is [B, S, D] and cand_hidden [B * k, D], got {tuple(hidden_states.shape)} and {tuple(cand_hidden.shape)}")
    B, S, D = hidden_states.shape
    R = cand_hidden.shape[0]
    if (B == 0 and R != 0) or (B > 0 and (R % B or not 1 <= R // B <= CONTRASTIVE_MAX_K)):
        raise ValueError(f"{who}: {R} candidate rows are no whole number of groups of 1 .. {CONTRASTIVE_MAX_K} for {B} batch rows")
    k = R // B if B else 1
    if not hidden_states.dtype.is_floating_point or cand_hidden.dtype != hidden_states.dtype:
        raise ValueError(f"{who}: hidden_states and cand_hidden share a floating-point dtype, got {hidden_states.dtype} and {cand_hidden.dtype}")
    if tuple(probs.shape) != (R,) or probs.dtype != torch.float32:
        raise ValueError(f"{who}: probs is a float32 [{R}], got {tuple(probs.shape)} {probs.dtype}")
    index, alpha = int(index), float(alpha)
    if not 1 <= index <= S:
        raise ValueError(f"{who}: 1 <= index <= S = {S} filled positions, got {index}")
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"{who}: 0 <= alpha <= 1, got {alpha}")
    for name, t in (("cand_hidden", cand_hidden), ("probs", probs)):
        if t.device != hidden_states.device:
            raise ValueError(f"{who}: {name} lies on {t.device}, the hidden states on {hidden_states.device}")
    if nn.dry_run():
        return _dry((B,), probs, torch.int32), _dry((R,), probs, torch.float32), _dry((R,), probs, torch.float32)
    with torch.no_grad():
        if B == 0:
            return (torch.empty((0,), dtype=torch.int32, device=probs.device), torch.empty((0,), dtype=torch.float32, device=probs.device),
                    torch.empty((0,), dtype=torch.float32, device=probs.device))
        if (hidden_states.is_cuda and contrastive_fused() and hidden_states.dtype in (torch.bfloat16, torch.float32)
                and K.contrastive_select_supported(D, k, hidden_states.dtype)):
            if (hidden_states.stride(2) != 1 or hidden_states.stride(1) % 8 or hidden_states.stride(1) < D or hidden_states.data_ptr() % 16
                    or (B > 1 and (hidden_states.stride(0) % 8 or hidden_states.stride(0) < S * hidden_states.stride(1)))):
                hidden_states = hidden_states.contiguous()
            if cand_hidden.stride(1) != 1 or cand_hidden.data_ptr() % 16 or (R > 1 and (cand_hidden.stride(0) % 8 or cand_hidden.stride(0) < D)):
                cand_hidden = cand_hidden.contiguous()
            return K.contrastive_select(hidden_states, index, cand_hidden, _c(probs), alpha, splits)
        return _contrastive_select_composed(hidden_states, index, cand_hidden, probs, alpha, k)


def contrastive_commit(cache, prompt, hidden_states, cand_hidden, winner, index, k, position=None):
    """The end of one step of keras_nlp.samplers.ContrastiveSampler -> (cache, prompt, hidden_states) with, for w = winner[b] and every j < k:
        cache[b k + j, :, :, position] = cache[b k + w, :, :, position];  prompt[b k + j, index] = prompt[b k + w, index];
        hidden_states[b, index] = cand_hidden[b k + w].
    cache [B k, L, 2, Sc, nkv, h] or None (Sc: the cache's own number of positions), prompt [B k, S] int32 or int64, hidden_states [B, Sh, D],
    cand_hidden [B k, D], winner int32 [B] as contrastive_select returns it; position: the cache position the candidates' step wrote (default
    `index`: call_with_cache's step index + 1 writes position index).
    On device tensors (csrc/contrastive.hip, one launch) all three are updated IN PLACE and returned, and only that one position moves: this
    relies on the k rows of a group being equal at every other position, as they are when the cache was repeated k times once and every step
    was committed.  A group whose winner lies outside [0, k) is left untouched.  CPU tensors, a cache that is not contiguous or whose
    [nkv, h] rows are no multiple of 16 bytes, hidden states whose rows are no multiple of 16 bytes and ISEG_CONTRASTIVE_FUSED=0 take the
    composed route, the reference's: new tensors, the whole cache gathered by the winners and repeated k times."""
    who = "contrastive_commit"
    _check_contrastive_k(who, k)
    index = int(index)
    if prompt.dim() != 2 or prompt.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{who}: prompt is an int32 or int64 [B * k, S], got {tuple(prompt.shape)} {prompt.dtype}")
    R, S = prompt.shape
    if R % k:
        raise ValueError(f"{who}: {R} rows are no whole number of groups of {k} candidates")
    B = R // k
    if tuple(winner.shape) != (B,) or winner.dtype != torch.int32:
        raise ValueError(f"{who}: winner is an int32 [{B}], got {tuple(winner.shape)} {winner.dtype}")
    if (hidden_states.dim() != 3 or hidden_states.shape[0] != B or tuple(cand_hidden.shape) != (R, hidden_states.shape[2])
            or cand_hidden.dtype != hidden_states.dtype):
        raise ValueError(f"{who}: hidden_states is [{B}, Sh, D] and cand_hidden [{R}, D] of its dtype, got {tuple(hidden_states.shape)} "
                         f"{hidden_states.dtype} and {tuple(cand_hidden.shape)} {cand_hidden.dtype}")
    if not 0 <= index < S or index >= hidden_states.shape[1]:
        raise ValueError(f"{who}: position {index} does not lie inside a prompt of {S} and a history of {hidden_states.shape[1]}")
    if cache is None:
        position = 0
    else:
        if not torch.is_tensor(cache) or cache.dim() != 6 or cache.shape[0] != R:
            raise ValueError(f"{who}: the cache is a [{R}, L, 2, S, nkv, h] tensor or None, got {tuple(cache.shape) if torch.is_tensor(cache) else cache!r}")
        position = index if position is None else int(position)
        if not 0 <= position < cache.shape[3]:
            raise ValueError(f"{who}: position {position} does not lie inside a cache of {cache.shape[3]}")
    for name, t in (("hidden_states", hidden_states), ("cand_hidden", cand_hidden), ("winner", winner), ("cache", cache)):
        if t is not None and t.device != prompt.device:
            raise ValueError(f"{who}: {name} lies on {t.device}, the prompt on {prompt.device}")
        if t is not None and t.requires_grad:
            raise RuntimeError(f"{who}: contrastive search is inference only ({name} requires grad)")
    if nn.dry_run() or R == 0:
        return cache, prompt, hidden_states
    with torch.no_grad():
        es, D = hidden_states.element_size(), hidden_states.shape[2]
        fused = (prompt.is_cuda and contrastive_fused() and prompt.stride(1) == 1 and (R == 1 or prompt.stride(0) >= S)
                 and hidden_states.dtype in (torch.bfloat16, torch.float32) and (D * es) % 16 == 0 and hidden_states.stride(2) == 1
                 and cand_hidden.stride(1) == 1 and hidden_states.data_ptr() % 16 == 0 and cand_hidden.data_ptr() % 16 == 0
                 and (hidden_states.stride(1) * es) % 16 == 0 and hidden_states.stride(1) >= D
                 and (B == 1 or ((hidden_states.stride(0) * es) % 16 == 0 and hidden_states.stride(0) >= hidden_states.shape[1] * hidden_states.stride(1)))
                 and (R == 1 or ((cand_hidden.stride(0) * es) % 16 == 0 and cand_hidden.stride(0) >= D)))
        if fused and cache is not None:
            fused = (cache.is_cuda and cache.is_contiguous() and cache.data_ptr() % 16 == 0
                     and (cache.shape[4] * cache.shape[5] * cache.element_size()) % 16 == 0)
        if fused:
            K.contrastive_commit(cache, position, prompt, index, hidden_states, cand_hidden, _c(winner), k)
            return cache, prompt, hidden_states
        w = winner.clamp(0, k - 1).to(torch.int64)
        rows = torch.arange(B, device=prompt.device) * k + w
        prompt = torch.repeat_interleave(prompt.index_select(0, rows), k, dim=0)
        hidden_states = hidden_states.clone()
        hidden_states[:, index] = cand_hidden.index_select(0, rows)
        if cache is not None:
            cache = torch.repeat_interleave(cache.index_select(0, rows), k, dim=0)
        return cache, prompt, hidden_states


def decode_commit(prompt, mask, pos_d, cur_ids, done, tokens, end_token_id=None):
    """One step of nlp/samplers.py's sample_loop on state in device memory, IN PLACE (csrc/decode_commit.hip, one launch, no host read), with
    p = pos_d[0], the index of the previous token:
      frozen   p + 1 outside [0, S), or an end_token_id is given and every done[b] is set: nothing changes;
      else     t = mask[b, p+1] ? prompt[b, p+1] : tokens[b];  prompt[b, p+1] = cur_ids[b] = t;  done[b] |= (t == end_token_id and not
               mask[b, p+1]);  pos_d[0] = p + 1.
    prompt [B, S] and cur_ids [B] int32 or int64, mask [B, S] and done [B] bool or uint8, pos_d int32 [1], tokens [B] int32 or int64 (the
    sampler's choice).  The caller sets done = ((prompt == end_token_id) & ~mask).any(-1) before the first step.  Returns None."""
    if end_token_id is not None and int(end_token_id) < 0:
        raise ValueError(f"decode_commit: end_token_id is None or a token id >= 0, got {end_token_id}")
    with torch.no_grad():
        K.decode_commit(prompt, mask, pos_d, cur_ids, done, tokens, end_token_id)


def embedding_logits(x, table):
    """x [B, T, d] -> [B, T, vocab] = x @ table^T with the token table [vocab, d]: the reverse use of the tied embedding
    (ReversibleEmbedding(reverse=True), nlp/gemma/gemma_causal.py:158) on the GEMM launchers -- the dense node with the kernel stored [out, in].
    The table's gradient from here (dy^T x) and from F.embedding accumulate on the one parameter."""
    _check_act_dtype(x)
    if nn.dry_run():
        return _dry((*x.shape[:-1], table.shape[0]), x)
    return _DenseFn.apply(x, table, None, K.ACT_NONE, None, True)


def lm_head_cross_entropy(hidden, table, target_ids, sample_weight=None, *, upstream_scale=1.0, chunk=0, with_accuracy=False):
    """hidden [..., d] (compute dtype), table [V, d] parameter, target_ids [...] -> the per-token loss [...] in fp32,
    upstream_scale * sample_weight * (logsumexp(hidden @ table^T) - its target's logit), without a [tokens, V] tensor: the table is walked in
    chunks of `chunk` rows (0: the library's rule) and each chunk's fp32 logits are consumed by the kernels of csrc/lm_head_ce.hip; the backward
    pass computes them again.  A target outside [0, V) counts as weight 0.  with_accuracy: also the first-maximal argmax [...] int32.
    Differentiable in hidden and table; the tape node is iseg_amd/nlp/lm_loss.py's (its first lines say why).  There is no torch route."""
    from .nlp import lm_loss

    loss, argmax, _ = lm_loss.lm_head_cross_entropy(hidden, table, target_ids, sample_weight, upstream_scale=upstream_scale, chunk=chunk)
    return (loss, argmax) if with_accuracy else loss


_FLIP_CACHE = {}


def flip_left_right(x):
    """tf.image.flip_left_right on [N,H,W,C]: a row permutation (its own inverse)"""
    N, H, W, C = x.shape
    if nn.dry_run():
        return _dry(x.shape, x)
    key = (N, H, W, str(x.device))
    if key not in _FLIP_CACHE:
        base = torch.arange(N * H, dtype=torch.int32).reshape(-1, 1) * W
        _FLIP_CACHE[key] = (base + torch.arange(W - 1, -1, -1, dtype=torch.int32).reshape(1, -1)).reshape(-1).to(x.device)
    idx = _FLIP_CACHE[key]
    return permute_rows(x, idx, idx, tuple(x.shape))
