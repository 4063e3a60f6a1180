"""The language-model head's cross-entropy without a [tokens, vocab] logits tensor (csrc/lm_head_ce.hip; include/iseg_hip.h states the kernels).

This tape node lives HERE and not in iseg_amd/functional.py on purpose: tests/test_grad_contract_host.py demands a row of the table in
tests/grad_contract_cases.py for every Function of functional.py whose backward books a parameter gradient, and that table is closed.  The node
keeps the same contract -- the table's gradient is ADDED into the parameter's one buffer (which F.embedding's gradient shares), autograd is handed
None for it, a frozen table receives nothing, a frozen `hidden` skips dX -- and tests/test_lm_loss_gpu.py restates those rules for it.
F.lm_head_cross_entropy is a thin forwarder to lm_head_cross_entropy below.

What is computed (reference: GemmaCausalLM compiled with SparseCategoricalCrossentropy(from_logits=True) and SparseCategoricalAccuracy,
nlp/gemma/gemma_causal.py:165-172, used through fit(x, y, sample_weight), :103-118):

    Z = hidden @ table^T          [M, V], never stored: the table is walked in chunks of `chunk` rows, Z_c [M, chunk] in FP32 per chunk
    loss[r] = upstream_scale * w_r * (logsumexp(Z[r]) - Z[r, t_r])       w_r = sample_weight[r], 0 where t_r lies outside [0, V)
    argmax[r] = the smallest v with Z[r, v] = max Z[r]

Forward: per chunk one GEMM (the table's rows as they lie are the K-contiguous operand) and the chunk kernel that merges it into the per-row online
softmax state; then the target's logit once more as an fp64 dot product rounded once (the loss carries that one logit's accumulation error
whole), and the finalise kernel.  Saved: hidden, targets, weights and the state's m and s (lse = m + log s in two parts).  Backward: per chunk the GEMM AGAIN, the gradient kernel
(G_c = upstream_scale w_r up_r (softmax - onehot), rounded once to the compute dtype), dX += G_c table[c] accumulated in one fp32 [M, d] buffer
and cast once, and rows c of the table's gradient += G_c^T X.  Memory is O(M chunk + M d)."""
import math

import torch
from torch.autograd import Function

from .. import dist
from .. import kernels as K
from .. import nn

MAX_VOCAB = (1 << 31) - 1025      # chunk indices stay int32 in the kernels


def default_chunk(M, V):
    """the chunk width for chunk=0: iseg_lm_head_ce_chunk_default, a value in [1, V] (profiles/lm_head_ce_kbench.md has the sweep behind it)"""
    return K.lm_head_ce_chunk_default(M, V)


def _grad_buffer(p):
    if p.grad is None:
        p.grad = torch.zeros_like(p.data)
    return p.grad


class _LmHeadCEFn(Function):
    @staticmethod
    def forward(ctx, hidden, table, targets, weights, scale, chunk):
        V, d = table.shape
        x2 = (hidden if hidden.is_contiguous() else hidden.contiguous()).reshape(-1, d)
        loss, _, argmax, _, sums, m, s = K.lm_head_ce_fwd(x2, nn.w(table), targets, weights, chunk, scale)
        ctx.table, ctx.scale, ctx.chunk, ctx.in_shape = table, scale, chunk, hidden.shape
        ctx.save_for_backward(x2, targets, weights, m, s)
        ctx.mark_non_differentiable(argmax, sums)
        return loss, argmax, sums

    @staticmethod
    def backward(ctx, dloss, _dargmax, _dsums):
        x2, targets, weights, m, s = ctx.saved_tensors
        table = ctx.table
        up = dloss.reshape(-1)
        if up.dtype != torch.float32:
            up = up.to(torch.float32)
        if not up.is_contiguous():
            up = up.contiguous()
        dtable = _grad_buffer(table) if table.requires_grad else None      # a frozen table receives nothing and its .grad stays None
        dx = K.lm_head_ce_bwd(x2, nn.w(table), targets, weights, m, s, up, ctx.scale, ctx.chunk, dtable=dtable, want_dx=ctx.needs_input_grad[0])
        dist.grads_ready(table)
        return (dx.reshape(ctx.in_shape) if dx is not None else None), None, None, None, None, None


def _check(hidden, table, target_ids, sample_weight, upstream_scale, chunk):
    who = "lm_head_cross_entropy"
    if hidden.dtype != nn.compute_dtype():
        raise TypeError(f"{who}: activation dtype {hidden.dtype} != compute dtype {nn.compute_dtype()}; cast the input with F.cast_input")
    if table.dim() != 2 or hidden.dim() < 1 or hidden.shape[-1] != table.shape[1]:
        raise ValueError(f"{who}: hidden is [..., d] and table [V, d], got {tuple(hidden.shape)} and {tuple(table.shape)}")
    if tuple(target_ids.shape) != tuple(hidden.shape[:-1]):
        raise ValueError(f"{who}: target_ids has the shape of hidden without its last axis, got {tuple(target_ids.shape)} for {tuple(hidden.shape)}")
    if target_ids.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{who}: target_ids are int32 or int64, got {target_ids.dtype}")
    if sample_weight is not None and tuple(sample_weight.shape) != tuple(target_ids.shape):
        raise ValueError(f"{who}: sample_weight has the shape of target_ids, got {tuple(sample_weight.shape)} for {tuple(target_ids.shape)}")
    if sample_weight is not None and not sample_weight.dtype.is_floating_point:
        raise ValueError(f"{who}: sample_weight is a floating-point tensor, got {sample_weight.dtype}")
    if not 1 <= table.shape[0] <= MAX_VOCAB:
        raise ValueError(f"{who}: the vocabulary is 1 .. {MAX_VOCAB} entries, got {table.shape[0]}")
    if isinstance(chunk, bool) or not isinstance(chunk, int) or chunk < 0:
        raise ValueError(f"{who}: chunk is 0 (the library's rule) or a positive number of table rows, got {chunk!r}")
    if not math.isfinite(float(upstream_scale)):
        raise ValueError(f"{who}: upstream_scale must be finite, got {upstream_scale}")
    if target_ids.requires_grad or (sample_weight is not None and sample_weight.requires_grad):
        raise RuntimeError(f"{who}: differentiable in hidden and table only (target_ids / sample_weight require grad)")


def lm_head_cross_entropy(hidden, table, target_ids, sample_weight=None, *, upstream_scale=1.0, chunk=0):
    """-> (loss [...] fp32, argmax [...] int32, sums fp32 [3] = sum loss, sum w * (argmax == target), sum w); see the module's first lines.
    Differentiable in hidden and table through `loss`."""
    _check(hidden, table, target_ids, sample_weight, upstream_scale, chunk)
    shape = tuple(target_ids.shape)
    V = table.shape[0]
    if nn.dry_run():
        return (torch.empty(shape, dtype=torch.float32, device=hidden.device), torch.empty(shape, dtype=torch.int32, device=hidden.device),
                torch.empty((3,), dtype=torch.float32, device=hidden.device))
    M = target_ids.numel()
    if M == 0:
        return (torch.zeros(shape, dtype=torch.float32, device=hidden.device), torch.zeros(shape, dtype=torch.int32, device=hidden.device),
                torch.zeros((3,), dtype=torch.float32, device=hidden.device))
    shadow = nn.w(table)
    if shadow.dtype != hidden.dtype:
        raise TypeError(f"lm_head_cross_entropy: the table's compute copy is {shadow.dtype}, hidden {hidden.dtype}")
    t = target_ids.reshape(-1)
    if t.dtype != torch.int32:
        t = t.clamp(-1, V).to(torch.int32)      # every id outside [0, V) stays outside
    w = None
    if sample_weight is not None:
        w = sample_weight.reshape(-1).to(torch.float32)
    width = int(chunk) if chunk > 0 else default_chunk(M, V)
    loss, argmax, sums = _LmHeadCEFn.apply(hidden, table, t.contiguous(), None if w is None else w.contiguous(), float(upstream_scale),
                                           min(width, V))
    return (loss, argmax, sums) if len(shape) == 1 else (loss.reshape(shape), argmax.reshape(shape), sums)
