"""Thin tensor-level wrappers over the C ABI (include/iseg_hip.h).

torch is used here only for device memory (torch.empty), dtype tags and the current HIP stream; every FLOP
and every byte moved on the hot path happens inside libiseg_hip.so.  Nothing here falls back to torch ops.
"""
import contextlib
import ctypes as C

import torch

from . import _hip
from ._hip import F32, BF16, ACT_NONE, ACT_RELU, ACT_GELU, ACT_GELU_GRAD, ACT_RELU_GRAD, ACT_MUL_AUX, ACT_SIGMOID, ACT_SWISH, ACT_GELU_TANH, GemmArgs  # noqa: F401

_DT = {torch.float32: F32, torch.bfloat16: BF16}


def dt(t):
    try:
        return _DT[t.dtype if isinstance(t, torch.Tensor) else t]
    except KeyError:
        raise TypeError(f"iseg_amd kernels support float32 and bfloat16 storage, got {t.dtype if isinstance(t, torch.Tensor) else t}")


def ptr(t):
    return None if t is None else t.data_ptr()


_DEVICE_INDEX = [None]


def stream():
    """raw hipStream_t of torch's current stream on this process's device.  torch.cuda.current_stream() re-derives the device
    through is_available() -> os.getenv on every call (measured 70 us per launch on the GPU box: 20 of the 41 ms of a batch-1
    ViT inference step were spent there); one process drives one GPU, so the index is resolved once."""
    idx = _DEVICE_INDEX[0]
    if idx is None:
        idx = _DEVICE_INDEX[0] = torch.cuda.current_device()
    return torch._C._cuda_getCurrentRawStream(idx)


def _require_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _hip.HipCallError("iseg_amd kernels need device tensors (cuda:N); there is no CPU path")


# ---------------------------------------------------------------------------------------------------------
# workspace: one growable byte buffer per (device, stream); stream order makes reuse across ops safe
# ---------------------------------------------------------------------------------------------------------
_WS = {}


def workspace(nbytes, device):
    if nbytes <= 0:
        return None, 0
    key = (device.index if device.index is not None else torch.cuda.current_device(), stream())
    buf = _WS.get(key)
    if buf is None or buf.numel() < nbytes:
        size = int(nbytes * 1.25) + 1024
        if torch.cuda.is_current_stream_capturing():
            if buf is not None:      # kernels already captured hold the old pointer: it must not go back to the pool
                raise _hip.HipCallError("workspace growth during hipGraph capture; run one eager warm-up step first")
            # a stream that first appears inside the capture (one that only the captured work uses): give it what
            # the warmed-up streams of this device ended up needing, so that it never has to grow while the capture goes on
            size = max([size] + [b.numel() for (d, _), b in _WS.items() if d == key[0]])
        buf = torch.empty(size, dtype=torch.uint8, device=device)
        _WS[key] = buf
    return buf, buf.numel()


# ---------------------------------------------------------------------------------------------------------
# optional per-launch timing with HIP events on the launch stream (bench.py's live roofline measurement)
# ---------------------------------------------------------------------------------------------------------
KERNEL_TIMER = [None]


class KernelTimer:
    """records a (start, stop) event pair around every instrumented launch, grouped by a shape key; no host sync until report()"""

    def __init__(self, only=None, every=1):
        self.records = {}
        self.seen = {}          # key -> launches seen (timed or not)
        self._cur = None
        self.only = only        # None: every instrumented launch; else the one shape key (or a set / list of keys) to time
        self._only = None if only is None else (set(only) if isinstance(only, (set, list, frozenset)) else {only})
        self.every = max(1, int(every))      # time every k-th matching launch: an event pair costs the stream a few microseconds of idle time

    def begin(self, key):
        if self._only is not None and key not in self._only:
            self._cur = None
            return
        n = self.seen.get(key, 0)
        self.seen[key] = n + 1
        if n % self.every:
            self._cur = None
            return
        e0 = torch.cuda.Event(enable_timing=True)
        e0.record()
        self._cur = (key, e0)

    def end(self):
        if self._cur is None:
            return
        key, e0 = self._cur
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        self.records.setdefault(key, []).append((e0, e1))

    def report(self):
        torch.cuda.synchronize()
        out = {}
        for key, pairs in self.records.items():
            ms = [a.elapsed_time(b) for a, b in pairs]
            out[key] = (sum(ms) / len(ms) * 1e-3, self.seen.get(key, len(ms)))     # seconds per launch (over the timed ones), launches seen
        return out


# ---------------------------------------------------------------------------------------------------------
# GEMM
# ---------------------------------------------------------------------------------------------------------
def _gemm_args(A, B, D, M, N, K, *, lda, ldb, ldd, a_kcontig, b_kcontig, **fields):
    """the iseg_gemm argument block of D[M, N] = A x B; `fields` are further GemmArgs fields by name (pointer fields take a tensor or None)"""
    g = GemmArgs()
    g.A, g.lda, g.a_kcontig = ptr(A), lda, int(a_kcontig)
    g.B, g.ldb, g.b_kcontig = ptr(B), ldb, int(b_kcontig)
    g.D, g.ldd = ptr(D), ldd
    g.M, g.N, g.K = M, N, K
    g.in_dtype, g.out_dtype = dt(A), dt(D)
    g.alpha, g.batch, g.batch_inner = 1.0, 1, 1
    for name, v in fields.items():
        if not hasattr(GemmArgs, name):
            raise TypeError(f"iseg_gemm_args has no field {name}")
        setattr(g, name, ptr(v) if isinstance(v, torch.Tensor) else v)
    return g


@contextlib.contextmanager
def _timed_gemm(g, in_dtype, out_dtype, variant=None):
    """the launch in its body -- iseg_gemm on g, or the pair launch that g leads (variant 9) -- lies between KERNEL_TIMER's events, under the shape
    key bench.py indexes: key[13] is the main loop's variant"""
    timer = KERNEL_TIMER[0]
    if timer is not None:
        L = _hip.lib()
        if variant is None:
            variant = int(L.iseg_gemm_variant(C.byref(g)))
        timer.begin(("gemm", g.a_kcontig, g.b_kcontig, g.M, g.N, g.K, g.act, bool(g.pre_out), bool(g.residual), bool(g.aux), in_dtype, out_dtype,
                     L.iseg_gemm_workspace_bytes(C.byref(g)) > 0, variant) + ((g.batch,) if g.batch > 1 else ()))
    yield
    if timer is not None:
        timer.end()


def gemm(A, B, D, M, N, K, *, lda, ldb, ldd, a_kcontig, b_kcontig, bias=None, colscale=None, rowscale=None,
         rows_per_group=0, residual=None, ldr=0, aux=None, ldaux=0, pre_out=None, ldp=0, act=ACT_NONE, alpha=1.0,
         accumulate=False, split_k=0, a_act=ACT_NONE, colsum_out=None, colsum_accumulate=False, batch=1, batch_inner=1,
         sa=(0, 0), sb=(0, 0), sd=(0, 0), pre_deriv=False, b_group=None):
    """batch > 1: problem z uses X + (z // batch_inner) * sX[0] + (z % batch_inner) * sX[1] (element strides);
    b_group=(rows, stride): rows [i*rows, (i+1)*rows) of A / D use B + i*stride (one kernel per sample; LDS-DMA path only)"""
    _require_cuda(A, B, D)
    if A.dtype != B.dtype:
        raise TypeError(f"gemm operands differ in dtype: {A.dtype} vs {B.dtype}")
    b_group_rows, b_group_stride = (int(b_group[0]), int(b_group[1])) if b_group is not None else (0, 0)
    g = _gemm_args(A, B, D, M, N, K, lda=lda, ldb=ldb, ldd=ldd, a_kcontig=a_kcontig, b_kcontig=b_kcontig, bias=bias, colscale=colscale,
                   rowscale=rowscale, rows_per_group=rows_per_group, residual=residual, ldr=ldr, aux=aux, ldaux=ldaux, pre_out=pre_out, ldp=ldp,
                   act=act, alpha=alpha, accumulate=int(accumulate), split_k=split_k, a_act=a_act, colsum_out=colsum_out,
                   colsum_accumulate=int(colsum_accumulate), batch=int(batch), batch_inner=int(batch_inner), pre_deriv=int(bool(pre_deriv)),
                   b_group_rows=b_group_rows, b_group_stride=b_group_stride, sa_outer=sa[0], sa_inner=sa[1], sb_outer=sb[0], sb_inner=sb[1],
                   sd_outer=sd[0], sd_inner=sd[1])
    for t in (residual, aux, pre_out):
        if t is not None and t.dtype != D.dtype:
            raise TypeError("gemm residual/aux/pre_out must have the output dtype")
    for t in (bias, colscale, rowscale):
        if t is not None and t.dtype != torch.float32:
            raise TypeError("gemm bias/colscale/rowscale must be float32")
    L = _hip.lib()
    need = L.iseg_gemm_workspace_bytes(C.byref(g))
    ws, wsb = workspace(need, A.device)
    g.defer_reduce = 1 if need > 0 else 0
    with _timed_gemm(g, A.dtype, D.dtype):
        _hip.check(L.iseg_gemm(C.byref(g), ptr(ws), wsb, stream()), "iseg_gemm")
    if need > 0:
        _hip.check(L.iseg_gemm_reduce(C.byref(g), ptr(ws), wsb, stream()), "iseg_gemm_reduce")
    return D


def dense_fwd(x2d, W, bias=None, *, act=ACT_NONE, out=None, ldd=None, out_dtype=None, pre_out=None, colscale=None,
              rowscale=None, rows_per_group=0, residual=None, a_act=ACT_NONE, pre_deriv=False):
    """x2d [M,K] (row stride x2d.stride(0)) @ W [K,N] (Keras Dense / 1x1 conv kernel).  pre_deriv: pre_out receives gelu'(pre-activation)
    (act must be GELU); the matching backward epilogue is ACT_MUL_AUX."""
    M, K = x2d.shape
    N = W.shape[1]
    if out is None:
        out = torch.empty((M, N), dtype=out_dtype or x2d.dtype, device=x2d.device)
    return gemm(x2d, W, out, M, N, K, lda=x2d.stride(0), ldb=W.stride(0), ldd=ldd or out.stride(0), a_kcontig=1, b_kcontig=0,
                bias=bias, act=act, pre_out=pre_out, ldp=(pre_out.stride(0) if pre_out is not None else 0), colscale=colscale,
                rowscale=rowscale, rows_per_group=rows_per_group, residual=residual,
                ldr=(residual.stride(0) if residual is not None else 0), a_act=a_act, pre_deriv=pre_deriv)


def dense_fwd_t(x2d, Wt, bias=None, *, act=ACT_NONE, out=None, pre_out=None, colscale=None, rowscale=None, rows_per_group=0, residual=None,
                pre_deriv=False):
    """dense_fwd with the kernel given K-contiguous: Wt [N,K] (nn.wt): both operands K-contiguous, so the LDS-DMA GEMM serves it"""
    M, K = x2d.shape
    N = Wt.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=x2d.dtype, device=x2d.device)
    return gemm(x2d, Wt, out, M, N, K, lda=x2d.stride(0), ldb=Wt.stride(0), ldd=out.stride(0), a_kcontig=1, b_kcontig=1, bias=bias, act=act,
                pre_out=pre_out, ldp=(pre_out.stride(0) if pre_out is not None else 0), colscale=colscale, rowscale=rowscale,
                rows_per_group=rows_per_group, residual=residual, ldr=(residual.stride(0) if residual is not None else 0), pre_deriv=pre_deriv)


def dense_dgrad(dy2d, W, *, out=None, act=ACT_NONE, aux=None, rowscale=None, rows_per_group=0, residual=None, accumulate=False):
    """dX [M,K] = dY [M,N] @ W[K,N]^T : W is consumed as stored (its rows are the N-contiguous reduction)."""
    M, N = dy2d.shape
    K = W.shape[0]
    if out is None:
        out = torch.empty((M, K), dtype=dy2d.dtype, device=dy2d.device)
    return gemm(dy2d, W, out, M, K, N, lda=dy2d.stride(0), ldb=W.stride(0), ldd=out.stride(0), a_kcontig=1, b_kcontig=1, act=act,
                aux=aux, ldaux=(aux.stride(0) if aux is not None else 0), rowscale=rowscale, rows_per_group=rows_per_group,
                residual=residual, ldr=(residual.stride(0) if residual is not None else 0), accumulate=accumulate)


def wgrad_can_fuse_bias(x2d):
    """the bias gradient can ride the weight-gradient GEMM (virtual ones-row = output row K): free when the last 128-row output tile has a spare
    row, one more tile row otherwise -- measured worth it from 3 tile rows on (flagship step 10.05 -> 9.94 ms when the stage-2 b1 gradients
    joined: the column-sum pass over the [M, 4C] tensor and its reduce cost more than a quarter more weight-gradient tiles)"""
    k = x2d.shape[1]
    return x2d.dtype == torch.bfloat16 and k % 8 == 0 and (k % 128 != 0 or k >= 384)


def dense_wgrad(x2d, dy2d, out, *, accumulate=True, alpha=1.0, a_act=ACT_NONE, bias_grad=None):
    """dW [K,N] (+)= X[M,K]^T @ dY[M,N]; out is fp32.  bias_grad [N] (+)= colsum(dY) if given (fused when possible)."""
    M, K = x2d.shape
    N = dy2d.shape[1]
    fuse = bias_grad is not None and wgrad_can_fuse_bias(x2d)
    if bias_grad is not None and not fuse:
        colsum(dy2d, dy2d.stride(0), 0, 1, M, N, bias_grad, accumulate=accumulate)
    return gemm(x2d, dy2d, out, K, N, M, lda=x2d.stride(0), ldb=dy2d.stride(0), ldd=out.stride(0), a_kcontig=0, b_kcontig=0,
                accumulate=accumulate, alpha=alpha, a_act=a_act, colsum_out=(bias_grad if fuse else None),
                colsum_accumulate=accumulate)


def dense_wgrad_slabs(x2d, dy2d):
    """the weight-gradient product X^T dY with its bias-gradient ones-row, stopped in front of the slab sum: (slabs [n, K + 1, N] fp32, n) for a
    consumer that sums the split-K slabs while it reads them (layerscale_grads_slabs), or None when the problem is not split / cannot carry
    the ones-row"""
    M, K = x2d.shape
    N = dy2d.shape[1]
    if not wgrad_can_fuse_bias(x2d) or N % 4 != 0 or x2d.dtype != torch.bfloat16:
        return None
    _require_cuda(x2d, dy2d)
    dummy = torch.empty(1, dtype=torch.float32, device=x2d.device)      # (never written: the problem stops at its slabs)
    g = _gemm_args(x2d, dy2d, dummy, K, N, M, lda=x2d.stride(0), ldb=dy2d.stride(0), ldd=N, a_kcontig=0, b_kcontig=0, colsum_out=dummy)
    L = _hip.lib()
    need = L.iseg_gemm_workspace_bytes(C.byref(g))
    if need == 0:
        return None
    eff = int(L.iseg_gemm_slabs(C.byref(g)))
    slabs = torch.empty(need // 4, dtype=torch.float32, device=x2d.device)      # (its own buffer: the consumer's partials use the workspace)
    g.defer_reduce = 1
    with _timed_gemm(g, x2d.dtype, torch.float32):
        _hip.check(L.iseg_gemm(C.byref(g), ptr(slabs), need, stream()), "iseg_gemm")
    return slabs, int(eff)


def dense_wgrad_pair(g2d, dbr2d, x2d, dh2d, dW1, db1, accumulate=True, defer_second=False):
    """The two weight-gradient products of an un-fused ConvNeXt block as ONE launch (csrc/gemm_dma_tn.h, round 5): Z = g^T dbr [4C, C] with its
    ones-row, stopped at its slabs for layerscale_grads_slabs, and dW1 (+)= x^T dh [C, 4C] (+ db1 from its ones-row), summed by iseg_gemm_reduce.
    Returns (slabs of Z, slab count) or None when the problems do not pair (the caller then runs them one by one)."""
    rows, K4 = g2d.shape
    Cc = dbr2d.shape[1]
    if not (wgrad_can_fuse_bias(g2d) and wgrad_can_fuse_bias(x2d)) or Cc % 4 != 0:
        return None
    _require_cuda(g2d, dbr2d, x2d, dh2d, dW1)
    dummy = torch.empty(1, dtype=torch.float32, device=g2d.device)

    def args(a, b, out, ldd, bias, acc):
        return _gemm_args(a, b, out, a.shape[1], b.shape[1], rows, lda=a.stride(0), ldb=b.stride(0), ldd=ldd, a_kcontig=0, b_kcontig=0,
                          accumulate=int(acc), colsum_out=bias, colsum_accumulate=int(acc), defer_reduce=1)

    g0 = args(g2d, dbr2d, dummy, Cc, dummy, False)
    g1 = args(x2d, dh2d, dW1, dW1.stride(0), db1, accumulate)
    L = _hip.lib()
    s = int(L.iseg_gemm_tn_pair_splits(C.byref(g0), C.byref(g1)))
    if s <= 1:
        return None
    g0.split_k = g1.split_k = s
    need0, need1 = L.iseg_gemm_workspace_bytes(C.byref(g0)), L.iseg_gemm_workspace_bytes(C.byref(g1))
    eff = int(L.iseg_gemm_slabs(C.byref(g0)))
    slabs0 = torch.empty(need0 // 4, dtype=torch.float32, device=g2d.device)      # (its own buffer: the consumer's partials use the workspace)
    # defer_second (round 6): the second product's slabs get their own buffer and are NOT summed here -- layerscale_grads_slabs(extra=...) sums them
    # in the launch that consumes the first product's slabs (one launch instead of two); only for the plain dense case the wide reducer covers
    n2 = (x2d.shape[1] + 1) * dh2d.shape[1]
    n0 = x2d.shape[1] * dh2d.shape[1]
    defer_second = bool(defer_second and dW1.stride(0) == dh2d.shape[1] and n2 % 4 == 0 and n0 % 4 == 0 and dW1.is_contiguous() and db1 is not None)
    if defer_second:
        ws1 = torch.empty(need1 // 4, dtype=torch.float32, device=g2d.device)
        wsb1 = need1
    else:
        ws1, wsb1 = workspace(need1, g2d.device)
    # (variant 9 = the pair launch: bench.py models it as two products [4C, C] and [C, 4C] over `rows`)
    with _timed_gemm(g0, g2d.dtype, torch.float32, variant=9):
        _hip.check(L.iseg_gemm_tn_pair(C.byref(g0), ptr(slabs0), need0, C.byref(g1), ptr(ws1), wsb1, stream()), "iseg_gemm_tn_pair")
    if defer_second:
        eff1 = int(L.iseg_gemm_slabs(C.byref(g1)))
        return slabs0, eff, (ws1, eff1, n2, dW1, db1, n0, bool(accumulate))
    _hip.check(L.iseg_gemm_reduce(C.byref(g1), ptr(ws1), wsb1, stream()), "iseg_gemm_reduce")
    return slabs0, eff


# ---------------------------------------------------------------------------------------------------------
# norms
# ---------------------------------------------------------------------------------------------------------
def convnext_mlp_supported(C, dtype):
    """the fused ConvNeXt MLP kernels (csrc/mlp_fused.hip) cover bf16 storage at C = 96 / 192"""
    return bool(_hip.lib().iseg_convnext_mlp_supported(int(C), _DT[dtype])) if dtype in _DT else False


def convnext_mlp_prep(W1, W2, gamma, backward=True):
    """fp32 Keras kernels -> the tiled bf16 images the fused kernels stream (once per step and block); returns (fw_tiled, bw_tiled)"""
    _require_cuda(W1, W2)
    Cc = W1.shape[0]
    L = _hip.lib()
    fw = torch.empty(L.iseg_convnext_mlp_tiled_bytes(Cc, 0) // 2, dtype=torch.bfloat16, device=W1.device)
    bw = torch.empty(L.iseg_convnext_mlp_tiled_bytes(Cc, 1) // 2, dtype=torch.bfloat16, device=W1.device) if backward else None
    _hip.call("iseg_convnext_mlp_prep", ptr(W1), ptr(W2), ptr(gamma), ptr(fw), ptr(bw), Cc, stream())
    return fw, bw


def convnext_mlp_fwd(y2, fw_tiled, b1, b2, gamma, rowscale, rows_per_group, residual, out=None):
    """out = residual + rowscale[m // rows_per_group] * gamma * (gelu(y2 @ W1 + b1) @ W2 + b2); the [M, 4C] hidden tile stays on the CU"""
    _require_cuda(y2, fw_tiled, residual)
    M, Cc = y2.shape
    if out is None:
        out = torch.empty((M, Cc), dtype=y2.dtype, device=y2.device)
    _hip.call("iseg_convnext_mlp_fwd", ptr(y2), ptr(fw_tiled), ptr(b1), ptr(b2), ptr(gamma), ptr(rowscale), int(rows_per_group),
              ptr(residual), ptr(out), M, Cc, dt(y2), stream())
    return out


def convnext_mlp_bwd(y2, dbr, bw_tiled, b1):
    """backward chain with the hidden tile recomputed: returns (g = gelu(h), dh = (dbr @ (W2 gamma)^T) * gelu'(h), dy2 = dh @ W1^T)"""
    _require_cuda(y2, dbr, bw_tiled)
    M, Cc = y2.shape
    g = torch.empty((M, 4 * Cc), dtype=y2.dtype, device=y2.device)
    dh = torch.empty((M, 4 * Cc), dtype=y2.dtype, device=y2.device)
    dy2 = torch.empty((M, Cc), dtype=y2.dtype, device=y2.device)
    _hip.call("iseg_convnext_mlp_bwd", ptr(y2), ptr(dbr), ptr(bw_tiled), ptr(b1), ptr(g), ptr(dh), ptr(dy2), M, Cc, dt(y2), stream())
    return g, dh, dy2


def convnext_mlp_fwd_ln(y1, ln_gamma, ln_beta, eps, fw_tiled, b1, b2, gamma, rowscale, rows_per_group, residual):
    """convnext_mlp_fwd with LayerNorm(y1) formed while the rows are loaded: returns (out, mean, rstd); y2 is never written"""
    _require_cuda(y1, fw_tiled, residual)
    M, Cc = y1.shape
    out = torch.empty((M, Cc), dtype=y1.dtype, device=y1.device)
    mean = torch.empty(M, dtype=torch.float32, device=y1.device)
    rstd = torch.empty(M, dtype=torch.float32, device=y1.device)
    _hip.call("iseg_convnext_mlp_fwd_ln", ptr(y1), ptr(ln_gamma), ptr(ln_beta), float(eps), ptr(mean), ptr(rstd), ptr(fw_tiled), ptr(b1), ptr(b2),
              ptr(gamma), ptr(rowscale), int(rows_per_group), ptr(residual), ptr(out), M, Cc, dt(y1), stream())
    return out, mean, rstd


def convnext_mlp_bwd_data(y, dout, bw_tiled, b1, rowscale=None, rows_per_group=0, ln=None):
    """dy2 = ((rowscale * dout) @ (W2 gamma)^T * gelu'(h)) @ W1^T with the hidden tile recomputed and kept on the CU (nothing [M, 4C] is
    written); ln = (mean, rstd, ln_gamma, ln_beta) makes `y` the LayerNorm input"""
    _require_cuda(y, dout, bw_tiled)
    M, Cc = y.shape
    dy2 = torch.empty((M, Cc), dtype=y.dtype, device=y.device)
    mean, rstd, lng, lnb = ln if ln is not None else (None, None, None, None)
    _hip.call("iseg_convnext_mlp_bwd_data", ptr(y), ptr(mean), ptr(rstd), ptr(lng), ptr(lnb), ptr(dout), ptr(rowscale), int(rows_per_group),
              ptr(bw_tiled), ptr(b1), ptr(dy2), M, Cc, dt(y), stream())
    return dy2


def convnext_mlp_bwd_data_ln(y1, dout, bw_tiled, b1, ln, dln_gamma, dln_beta, rowscale=None, rows_per_group=0):
    """convnext_mlp_bwd_data carried through the LayerNorm in front of the MLP: returns the gradient of the LayerNorm INPUT y1 and adds the
    LayerNorm parameter gradients to dln_gamma / dln_beta; ln = (mean, rstd, ln_gamma, ln_beta)"""
    _require_cuda(y1, dout, bw_tiled, dln_gamma, dln_beta)
    M, Cc = y1.shape
    dy1 = torch.empty((M, Cc), dtype=y1.dtype, device=y1.device)
    mean, rstd, lng, lnb = ln
    need = _hip.lib().iseg_convnext_mlp_bwd_data_ln_workspace_bytes(M, Cc)
    ws, wsb = workspace(need, y1.device)
    _hip.call("iseg_convnext_mlp_bwd_data_ln", ptr(y1), ptr(mean), ptr(rstd), ptr(lng), ptr(lnb), ptr(dout), ptr(rowscale), int(rows_per_group),
              ptr(bw_tiled), ptr(b1), ptr(dy1), ptr(dln_gamma), ptr(dln_beta), M, Cc, dt(y1), ptr(ws), wsb, stream())
    return dy1


def convnext_mlp_wgrad(y, dout, bw_tiled, b1, W2, b2, gamma, dW1, db1, dW2, db2, dgamma, rowscale=None, rows_per_group=0, ln=None):
    """all parameter gradients of the fused MLP accumulated into dW1 / db1 / dW2 / db2 / dgamma (csrc/mlp_wgrad.hip); ln = (mean, rstd,
    ln_gamma, ln_beta) makes `y` the LayerNorm input"""
    _require_cuda(y, dout, bw_tiled)
    M, Cc = y.shape
    need = _hip.lib().iseg_convnext_mlp_wgrad_workspace_bytes(M, Cc)
    ws, wsb = workspace(need, y.device)
    mean, rstd, lng, lnb = ln if ln is not None else (None, None, None, None)
    _hip.call("iseg_convnext_mlp_wgrad", ptr(y), ptr(mean), ptr(rstd), ptr(lng), ptr(lnb), ptr(dout), ptr(rowscale), int(rows_per_group),
              ptr(bw_tiled), ptr(b1), ptr(W2), ptr(b2), ptr(gamma), ptr(dW1), ptr(db1), ptr(dW2), ptr(db2), ptr(dgamma), M, Cc, dt(y), ptr(ws),
              wsb, stream())


def convnext_mlp_bwd_onepass_supported(C, dtype):
    """the one-pass backward kernel (csrc/mlp_bwd_onepass.hip) exists for bf16 rows of 96 channels"""
    return C == 96 and dtype == torch.bfloat16


def convnext_mlp_bwd_onepass(y1, dout, bw_tiled, b1, W2, b2, gamma, ln, dln_gamma, dln_beta, dW1, db1, dW2, db2, dgamma, rowscale=None,
                             rows_per_group=0):
    """convnext_mlp_bwd_data_ln + convnext_mlp_wgrad in one pass over the rows, the hidden tile formed once (csrc/mlp_bwd_onepass.hip, C = 96):
    returns the gradient of the LayerNorm INPUT y1 and adds every parameter gradient to its buffer; ln = (mean, rstd, ln_gamma, ln_beta)"""
    _require_cuda(y1, dout, bw_tiled, dln_gamma, dln_beta)
    M, Cc = y1.shape
    dy1 = torch.empty((M, Cc), dtype=y1.dtype, device=y1.device)
    mean, rstd, lng, lnb = ln
    need = _hip.lib().iseg_convnext_mlp_wgrad_workspace_bytes(M, Cc)      # one size function for both launchers of the chunk records
    ws, wsb = workspace(need, y1.device)
    _hip.call("iseg_convnext_mlp_bwd_onepass", ptr(y1), ptr(mean), ptr(rstd), ptr(lng), ptr(lnb), ptr(dout), ptr(rowscale), int(rows_per_group),
              ptr(bw_tiled), ptr(b1), ptr(W2), ptr(b2), ptr(gamma), ptr(dy1), ptr(dln_gamma), ptr(dln_beta), ptr(dW1), ptr(db1), ptr(dW2),
              ptr(db2), ptr(dgamma), M, Cc, dt(y1), ptr(ws), wsb, stream())
    return dy1


def layernorm_fwd(x2d, gamma, beta, eps, save_stats=True):
    _require_cuda(x2d)
    rows, Cc = x2d.shape
    y = torch.empty_like(x2d)
    mean = torch.empty(rows, dtype=torch.float32, device=x2d.device) if save_stats else None
    rstd = torch.empty(rows, dtype=torch.float32, device=x2d.device) if save_stats else None
    _hip.call("iseg_layernorm_fwd", ptr(x2d), ptr(gamma), ptr(beta), ptr(y), ptr(mean), ptr(rstd), rows, Cc, eps, dt(x2d), stream())
    return y, mean, rstd


def layernorm_bwd(dy2d, x2d, gamma, mean, rstd, dgamma, dbeta, dx_add=None, accumulate=True):
    rows, Cc = x2d.shape
    dx = torch.empty_like(x2d)
    need = _hip.lib().iseg_layernorm_bwd_workspace_bytes(rows, Cc)
    ws, wsb = workspace(need, x2d.device)
    _hip.call("iseg_layernorm_bwd", ptr(dy2d), ptr(x2d), ptr(gamma), ptr(mean), ptr(rstd), ptr(dx), ptr(dx_add), ptr(dgamma),
              ptr(dbeta), int(accumulate), rows, Cc, dt(x2d), ptr(ws), wsb, stream())
    return dx


def layernorm_post_fwd(x2d, gamma, beta, eps, colscale=None, rowscale=None, rows_per_group=0, residual=None):
    """residual + rowscale[row // rows_per_group] * colscale * LN(x2d) in one pass (iseg_layernorm_post_fwd); returns (y, mean, rstd)"""
    _require_cuda(x2d)
    rows, Cc = x2d.shape
    y = torch.empty_like(x2d)
    mean = torch.empty(rows, dtype=torch.float32, device=x2d.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x2d.device)
    _hip.call("iseg_layernorm_post_fwd", ptr(x2d), ptr(gamma), ptr(beta), ptr(colscale), ptr(rowscale), int(rows_per_group), ptr(residual), ptr(y),
              ptr(mean), ptr(rstd), rows, Cc, eps, dt(x2d), stream())
    return y, mean, rstd


def layernorm_post_bwd(dy2d, x2d, gamma, beta, mean, rstd, dgamma, dbeta, colscale=None, dcolscale=None, rowscale=None, rows_per_group=0):
    """backward of layernorm_post_fwd: returns dx; dgamma / dbeta / dcolscale are accumulated"""
    _require_cuda(dy2d, x2d)
    rows, Cc = x2d.shape
    dx = torch.empty_like(x2d)
    need = _hip.lib().iseg_layernorm_bwd_workspace_bytes(rows, Cc) + 2 * Cc * 4
    ws, wsb = workspace(need, x2d.device)
    _hip.call("iseg_layernorm_post_bwd", ptr(dy2d), ptr(x2d), ptr(gamma), ptr(beta), ptr(colscale), ptr(rowscale), int(rows_per_group), ptr(mean),
              ptr(rstd), ptr(dx), ptr(dgamma), ptr(dbeta), ptr(dcolscale), rows, Cc, dt(x2d), ptr(ws), wsb, stream())
    return dx


def layernorm_gather_fwd(x2d, src_index, gamma, beta, eps):
    """y[r] = LN(x2d[src_index[r]]) or a zero row where src_index[r] < 0; mean / rstd per OUTPUT row (iseg_layernorm_gather_fwd)"""
    _require_cuda(x2d, src_index)
    rows_out, Cc = src_index.numel(), x2d.shape[1]
    y = torch.empty((rows_out, Cc), dtype=x2d.dtype, device=x2d.device)
    mean = torch.empty(rows_out, dtype=torch.float32, device=x2d.device)
    rstd = torch.empty(rows_out, dtype=torch.float32, device=x2d.device)
    _hip.call("iseg_layernorm_gather_fwd", ptr(x2d), ptr(src_index), ptr(gamma), ptr(beta), ptr(y), ptr(mean), ptr(rstd), rows_out, Cc, eps,
              dt(x2d), stream())
    return y, mean, rstd


def layernorm_gather_bwd(dy2d, dy_index, x2d, gamma, mean, rstd, dgamma, dbeta, dx_add=None, accumulate=True):
    """backward of layernorm_gather_fwd over the source rows: the gradient row / statistics of source row r are row dy_index[r] of dy2d / mean / rstd"""
    _require_cuda(dy2d, dy_index, x2d)
    rows, Cc = x2d.shape
    dx = torch.empty_like(x2d)
    need = _hip.lib().iseg_layernorm_bwd_workspace_bytes(rows, Cc)
    ws, wsb = workspace(need, x2d.device)
    _hip.call("iseg_layernorm_gather_bwd", ptr(dy2d), ptr(dy_index), ptr(x2d), ptr(gamma), ptr(mean), ptr(rstd), ptr(dx), ptr(dx_add), ptr(dgamma),
              ptr(dbeta), int(accumulate), rows, Cc, dt(x2d), ptr(ws), wsb, stream())
    return dx


def gather_rows_fma(x2d, idx, scale=None, rows_per_group=0, scale_by_source_row=False, residual=None):
    """y[r] = residual[r] + scale[g] * x2d[idx[r]] (zero where idx[r] < 0), g = (idx[r] if scale_by_source_row else r) // rows_per_group"""
    _require_cuda(x2d, idx)
    rows_out, Cc = idx.numel(), x2d.shape[1]
    y = torch.empty((rows_out, Cc), dtype=x2d.dtype, device=x2d.device)
    _hip.call("iseg_gather_rows_fma", ptr(x2d), ptr(idx), ptr(scale), int(rows_per_group), int(scale_by_source_row), ptr(residual), ptr(y), rows_out,
              Cc, dt(x2d), stream())
    return y


def bn_stats(x2d, ldx, rows, Cc, out=None):
    """packed [2C+1] = (sum, sum of squares, count); `out`: a slice of a larger message (several layers, one all-reduce)"""
    packed = out if out is not None else torch.empty(2 * Cc + 1, dtype=torch.float32, device=x2d.device)
    need = _hip.lib().iseg_bn_workspace_bytes(rows, Cc)
    ws, wsb = workspace(need, x2d.device)
    _hip.call("iseg_bn_stats", ptr(x2d), ldx, ptr(packed), rows, Cc, dt(x2d), ptr(ws), wsb, stream())
    return packed


def bn_finalize(packed, Cc, eps, momentum, moving_mean, moving_var):
    mean = torch.empty(Cc, dtype=torch.float32, device=packed.device)
    rstd = torch.empty(Cc, dtype=torch.float32, device=packed.device)
    _hip.call("iseg_bn_finalize", ptr(packed), Cc, eps, momentum, ptr(mean), ptr(rstd), ptr(moving_mean), ptr(moving_var), stream())
    return mean, rstd


def bn_finalize_apply(packed, x2d, ldx, gamma, beta, y2d, ldy, rows, Cc, eps, momentum, moving_mean, moving_var, relu):
    """bn_finalize + bn_apply_fwd; one launch when the statistics vectors are 16-byte aligned (a slice of a grouped message may not be)"""
    aligned = all(t is None or t.data_ptr() % 16 == 0 for t in (packed, moving_mean, moving_var))
    if not aligned:
        mean, rstd = bn_finalize(packed, Cc, eps, momentum, moving_mean, moving_var)
        bn_apply_fwd(x2d, ldx, mean, rstd, gamma, beta, y2d, ldy, rows, Cc, relu)
        return mean, rstd
    mean = torch.empty(Cc, dtype=torch.float32, device=packed.device)
    rstd = torch.empty(Cc, dtype=torch.float32, device=packed.device)
    _hip.call("iseg_bn_apply_fwd_packed", ptr(x2d), ldx, ptr(packed), eps, momentum, ptr(gamma), ptr(beta), ptr(mean), ptr(rstd),
              ptr(moving_mean), ptr(moving_var), ptr(y2d), ldy, rows, Cc, int(relu), dt(x2d), stream())
    return mean, rstd


def bn_apply_fwd(x2d, ldx, mean, rstd, gamma, beta, y2d, ldy, rows, Cc, relu):
    _hip.call("iseg_bn_apply_fwd", ptr(x2d), ldx, ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(y2d), ldy, rows, Cc, int(relu),
              dt(x2d), stream())
    return y2d


def bn_bwd_reduce(dy2d, lddy, x2d, ldx, y2d, ldy, mean, rstd, rows, Cc, relu, out=None):
    sums = out if out is not None else torch.empty(2 * Cc, dtype=torch.float32, device=x2d.device)
    need = _hip.lib().iseg_bn_workspace_bytes(rows, Cc)
    ws, wsb = workspace(need, x2d.device)
    _hip.call("iseg_bn_bwd_reduce", ptr(dy2d), lddy, ptr(x2d), ldx, ptr(y2d), ldy, ptr(mean), ptr(rstd), ptr(sums), rows, Cc,
              int(relu), dt(x2d), ptr(ws), wsb, stream())
    return sums


def bn_bwd_apply(dy2d, lddy, x2d, ldx, y2d, ldy, mean, rstd, gamma, sums, inv_n, dx2d, lddx, rows, Cc, relu, dgamma=None, dbeta=None):
    """dgamma / dbeta (+)= the packed sums, booked by the same launch -- only valid while `sums` are this replica's own"""
    if dgamma is None and dbeta is None:
        _hip.call("iseg_bn_bwd_apply", ptr(dy2d), lddy, ptr(x2d), ldx, ptr(y2d), ldy, ptr(mean), ptr(rstd), ptr(gamma), ptr(sums), inv_n,
                  ptr(dx2d), lddx, rows, Cc, int(relu), dt(x2d), stream())
    else:
        _hip.call("iseg_bn_bwd_apply_acc", ptr(dy2d), lddy, ptr(x2d), ldx, ptr(y2d), ldy, ptr(mean), ptr(rstd), ptr(gamma), ptr(sums), inv_n,
                  ptr(dx2d), lddx, ptr(dgamma), ptr(dbeta), rows, Cc, int(relu), dt(x2d), stream())
    return dx2d


def bn_bwd_reduce_remask(dy2d, lddy, x2d, ldx, mean, rstd, gamma, beta, rows, Cc, out=None):
    """bn_bwd_reduce with fused ReLU whose mask is re-derived from x (the forward kept no output)"""
    sums = out if out is not None else torch.empty(2 * Cc, dtype=torch.float32, device=x2d.device)
    need = _hip.lib().iseg_bn_workspace_bytes(rows, Cc)
    ws, wsb = workspace(need, x2d.device)
    _hip.call("iseg_bn_bwd_reduce_remask", ptr(dy2d), lddy, ptr(x2d), ldx, ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(sums), rows, Cc,
              dt(x2d), ptr(ws), wsb, stream())
    return sums


def bn_bwd_apply_remask(dy2d, lddy, x2d, ldx, mean, rstd, gamma, beta, sums, inv_n, dx2d, lddx, rows, Cc, dgamma=None, dbeta=None):
    _hip.call("iseg_bn_bwd_apply_remask", ptr(dy2d), lddy, ptr(x2d), ldx, ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(sums), inv_n,
              ptr(dx2d), lddx, ptr(dgamma), ptr(dbeta), rows, Cc, dt(x2d), stream())
    return dx2d


def bn_relu_upsample_add(z, mean, rstd, gamma, beta, x):
    """relu(bn(z)) + bilinear_up(x) in one pass: z [N, Ho, Wo, C], x [N, Hi, Wi, C] (iseg_bn_relu_upsample_add)"""
    _require_cuda(z, x)
    N, Ho, Wo, Cc = z.shape
    _, Hi, Wi, _ = x.shape
    out = torch.empty_like(z)
    _hip.call("iseg_bn_relu_upsample_add", ptr(z), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(x), ptr(out), N, Hi, Wi, Ho, Wo, Cc, dt(z),
              stream())
    return out


def rsqrt_eps(var, eps):
    out = torch.empty_like(var)
    _hip.call("iseg_rsqrt_eps", ptr(var), eps, ptr(out), var.numel(), stream())
    return out


# ---------------------------------------------------------------------------------------------------------
# EfficientNet MBConv tail: BN -> swish -> squeeze-excite -> gate (csrc/mbconv.hip)
# ---------------------------------------------------------------------------------------------------------
def mbconv_supported(N, HW, Cc, Cse):
    return bool(_hip.lib().iseg_mbconv_supported(int(N), int(HW), int(Cc), int(Cse)))


def _mb_partials(N, HW, Cc, backward, device):
    nbytes = _hip.lib().iseg_mbconv_partials_bytes(N, HW, Cc, int(backward))
    return torch.empty(nbytes // 4, dtype=torch.float32, device=device), nbytes


def bn_swish_se_fwd(x, mean, rstd, gamma, beta, W1, b1, W2, b2):
    """out = swish(bn(x)) * sigmoid(W2^T swish(W1^T mean_hw swish(bn(x)) + b1) + b2); x [N, H, W, C]; W1 [C, Cse], W2 [Cse, C] fp32.
    Returns (out, m [N, C], hpre [N, Cse], g [N, C]) -- the last three are what the backward reads."""
    _require_cuda(x, W1, W2)
    N, H, W, Cc = x.shape
    HW, Cse = H * W, W1.shape[-1]
    part, pbytes = _mb_partials(N, HW, Cc, False, x.device)
    _hip.call("iseg_bn_swish_se_squeeze", ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(part), pbytes, N, HW, Cc, dt(x), stream())
    m = torch.empty((N, Cc), dtype=torch.float32, device=x.device)
    hpre = torch.empty((N, Cse), dtype=torch.float32, device=x.device)
    g = torch.empty((N, Cc), dtype=torch.float32, device=x.device)
    _hip.call("iseg_se_excite_fwd", ptr(part), N, HW, Cc, Cse, ptr(W1), ptr(b1), ptr(W2), ptr(b2), ptr(m), ptr(hpre), ptr(g), stream())
    out = torch.empty_like(x)
    _hip.call("iseg_bn_swish_gate_fwd", ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(g), ptr(out), N, HW, Cc, dt(x), stream())
    return out, m, hpre, g


def bn_swish_se_bwd_sums(dO, x, mean, rstd, gamma, beta, W1, W2, m, hpre, g, dW1, db1, dW2, db2, accumulate=True):
    """reduce pass + excite backward: books dW1 / db1 / dW2 / db2 ((+)=, None skipped); returns (sums [2C] = (sum dz, sum dz*xhat),
    dmh [N, C] = dm / HW)"""
    _require_cuda(dO, x)
    N, H, W, Cc = x.shape
    HW, Cse = H * W, W1.shape[-1]
    part, pbytes = _mb_partials(N, HW, Cc, True, x.device)
    _hip.call("iseg_bn_swish_gate_bwd_reduce", ptr(dO), ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(part), pbytes, N, HW, Cc, dt(x),
              stream())
    ws, wsb = workspace(_hip.lib().iseg_se_excite_bwd_workspace_bytes(N, Cc, Cse), x.device)
    dmh = torch.empty((N, Cc), dtype=torch.float32, device=x.device)
    sums = torch.empty(2 * Cc, dtype=torch.float32, device=x.device)
    _hip.call("iseg_se_excite_bwd", ptr(part), N, HW, Cc, Cse, ptr(W1), ptr(W2), ptr(m), ptr(hpre), ptr(g), ptr(dW1), ptr(db1), ptr(dW2), ptr(db2),
              int(accumulate), ptr(dmh), ptr(sums), ptr(ws), wsb, stream())
    return sums, dmh


def bn_swish_gate_bwd_apply(dO, x, mean, rstd, gamma, beta, g, dmh, sums, inv_n, train, dgamma=None, dbeta=None):
    """dx of the tail; dgamma / dbeta (+)= the sums by the same launch -- only while `sums` are this replica's own"""
    N, H, W, Cc = x.shape
    dx = torch.empty_like(x)
    _hip.call("iseg_bn_swish_gate_bwd_apply", ptr(dO), ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(g), ptr(dmh), ptr(sums),
              float(inv_n), int(train), ptr(dx), ptr(dgamma), ptr(dbeta), N, H * W, Cc, dt(x), stream())
    return dx


# ---------------------------------------------------------------------------------------------------------
# Xception separable unit: relu -> depthwise 3x3 -> BN folded into the pointwise GEMM (csrc/sepconv.hip)
# ---------------------------------------------------------------------------------------------------------
def sepconv_supported(N, H, W, Cc, stride, dil, dtype):
    return bool(_hip.lib().iseg_sepconv_supported(int(N), int(H), int(W), int(Cc), int(stride), int(dil), dt(dtype)))


def relu_dwconv3_stats(x, w, stride, dil, stats=True):
    """z = dw3x3(relu(x)) (TF 'same'), and with stats the packed [2C+1] message of bn_stats over z; x [N,H,W,C], w [9, C] fp32"""
    _require_cuda(x, w)
    N, H, W, Cc = x.shape
    Ho, _ = same_pad(H, 3, stride, dil)
    Wo, _ = same_pad(W, 3, stride, dil)
    z = torch.empty((N, Ho, Wo, Cc), dtype=x.dtype, device=x.device)
    packed, ws, wsb = None, None, 0
    if stats:
        packed = torch.empty(2 * Cc + 1, dtype=torch.float32, device=x.device)
        ws, wsb = workspace(_hip.lib().iseg_relu_dwconv3_stats_workspace_bytes(N, H, W, Cc, stride, dil), x.device)
    _hip.call("iseg_relu_dwconv3_stats", ptr(x), ptr(w), ptr(z), ptr(packed), N, H, W, Cc, int(stride), int(dil), dt(x), ptr(ws), wsb, stream())
    return z, packed


def sepconv_fold(W, mean, rstd, gamma, beta, dtype, want_t=True, want_n=True):
    """(Wt [Cout, Cin], Wn [Cin, Cout]) = diag(a) W in the operand dtype (None where not wanted), bias [Cout] = c^T W fp32; a = gamma*rstd,
    c = beta - a*mean"""
    Cin, Cout = W.shape
    Wt = torch.empty((Cout, Cin), dtype=dtype, device=W.device) if want_t else None
    Wn = torch.empty((Cin, Cout), dtype=dtype, device=W.device) if want_n else None
    bias = torch.empty(Cout, dtype=torch.float32, device=W.device)
    _hip.call("iseg_sepconv_fold", ptr(W), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(Wt), ptr(Wn), ptr(bias), Cin, Cout, dt(dtype), stream())
    return Wt, Wn, bias


def sepconv_fold_bwd(G, S, W, mean, rstd, gamma, beta, dW=None, dgamma=None, dbeta=None, out=None):
    """dW (+)= diag(a) G + c S^T; returns sums [2Cin] = [dbeta | dgamma], which the same launch adds into dgamma / dbeta (None: skipped);
    `out`: a [2Cin] slice of a larger message (several layers, one exchange)"""
    Cin, Cout = W.shape
    sums = out if out is not None else torch.empty(2 * Cin, dtype=torch.float32, device=W.device)
    _hip.call("iseg_sepconv_fold_bwd", ptr(G), ptr(S), ptr(W), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(dW), ptr(sums), ptr(dgamma),
              ptr(dbeta), Cin, Cout, stream())
    return sums


def bnfold_dwconv3_relu_bwd(D, z, x, w, mean, rstd, gamma, sums, inv_n, train, dw, stride, dil):
    """dx = [x > 0] dw3x3^T(dz), dw [9, C] += sum relu(x) dz; dz = D + alpha + beta' z (training statistics) or D"""
    _require_cuda(D, z, x, w, dw)
    N, H, W, Cc = x.shape
    dx = torch.empty_like(x)
    ws, wsb = workspace(_hip.lib().iseg_bnfold_dwconv3_relu_bwd_workspace_bytes(N, H, W, Cc, stride, dil), x.device)
    _hip.call("iseg_bnfold_dwconv3_relu_bwd", ptr(D), ptr(z), ptr(x), ptr(w), ptr(mean), ptr(rstd), ptr(gamma), ptr(sums), float(inv_n), int(train),
              ptr(dx), ptr(dw), N, H, W, Cc, int(stride), int(dil), dt(x), ptr(ws), wsb, stream())
    return dx


# ---------------------------------------------------------------------------------------------------------
# JointPyramidUpsampling tail: four depthwise 3x3 branches (dilation 1, 2, 4, 8, with bias) over one tensor (csrc/jpu.hip)
# ---------------------------------------------------------------------------------------------------------
JPU_RATES = 4


def jpu_supported(N, H, W, Cc, dtype):
    return bool(_hip.lib().iseg_jpu_supported(int(N), int(H), int(W), int(Cc), dt(dtype)))


def jpu_dwconv3x4_stats(x, w, bias, stats=True, ws_bytes=None):
    """z [4][N,H,W,C], z[r] = dw3x3(x, w[r], dilation (1, 2, 4, 8)[r]) + bias[r] (TF 'same'), and with stats the four packed [2C+1] messages of
    bn_stats over the stored z; x [N,H,W,C], w [4, 9, C], bias [4, C] fp32.  ws_bytes: the workspace size handed to the launcher (tests)"""
    _require_cuda(x, w, bias)
    N, H, W, Cc = x.shape
    z = torch.empty((JPU_RATES, N, H, W, Cc), dtype=x.dtype, device=x.device)
    packed, ws, wsb = None, None, 0
    if stats:
        packed = torch.empty((JPU_RATES, 2 * Cc + 1), dtype=torch.float32, device=x.device)
        ws, wsb = workspace(_hip.lib().iseg_jpu_partials_bytes(N, H, W, Cc, 0), x.device)
        if ws_bytes is not None:
            wsb = ws_bytes
    _hip.call("iseg_jpu_dwconv3x4_stats", ptr(x), ptr(w), ptr(bias), ptr(z), ptr(packed), N, H, W, Cc, dt(x), ptr(ws), wsb, stream())
    return z, packed


def jpu_bnfold_dwconv3x4_bwd(D, z, x, w, mean, rstd, gamma, sums, inv_n, train, dw, db, ws_bytes=None):
    """dx = sum_r dw3x3_r^T(dz_r), dw [4, 9, C] += sum x dz_r per tap, db [4, C] += sum dz_r; dz_r = D_r + alpha_r + beta'_r z_r (training
    statistics; mean / rstd / gamma [4, C], sums [4][2C]) or D_r"""
    _require_cuda(D, z, x, w, dw, db)
    N, H, W, Cc = x.shape
    dx = torch.empty_like(x)
    ws, wsb = workspace(_hip.lib().iseg_jpu_partials_bytes(N, H, W, Cc, 1), x.device)
    if ws_bytes is not None:
        wsb = ws_bytes
    _hip.call("iseg_jpu_bnfold_dwconv3x4_bwd", ptr(D), ptr(z), ptr(x), ptr(w), ptr(mean), ptr(rstd), ptr(gamma), ptr(sums), float(inv_n), int(train),
              ptr(dx), ptr(dw), ptr(db), N, H, W, Cc, dt(x), ptr(ws), wsb, stream())
    return dx


# ---------------------------------------------------------------------------------------------------------
# ResNet-9 / 10 / 18 basic-block tail: relu(bn2(z2) + avg_pool_s(bn0(z0) or x)) (csrc/resblock.hip)
# ---------------------------------------------------------------------------------------------------------
def resblock_tail_supported(Cc, stride, dtype):
    return bool(_hip.lib().iseg_resblock_tail_supported(int(Cc), int(stride), dt(dtype)))


def resblock_tail_fwd(z2, mean2, rstd2, gamma2, beta2, sc, stride, bn0=None):
    """out = relu(bn2(z2) + pool_s(sc')), sc' = bn0(sc) when bn0 = (mean0, rstd0, gamma0, beta0) is given, else sc; sc [N, H, W, C],
    z2 [N, ceil(H/s), ceil(W/s), C]"""
    _require_cuda(z2, sc)
    N, H, W, Cc = sc.shape
    m0, r0, g0, b0 = bn0 if bn0 is not None else (None,) * 4
    out = torch.empty_like(z2)
    _hip.call("iseg_resblock_tail_fwd", ptr(z2), ptr(mean2), ptr(rstd2), ptr(gamma2), ptr(beta2), ptr(sc), ptr(m0), ptr(r0), ptr(g0), ptr(b0),
              ptr(out), N, H, W, Cc, int(stride), dt(z2), stream())
    return out


def resblock_tail_bwd_reduce(dout, out, z2, mean2, rstd2, sc_shape, stride, z0=None, mean0=None, rstd0=None):
    """sums [2C] = (sum g, sum g*xhat2), g = dout*[out > 0]; with z0 [4C]: + (sum u, sum u*xhat0) over the full-resolution rows"""
    _require_cuda(dout, out, z2)
    N, H, W, Cc = sc_shape
    sums = torch.empty((4 if z0 is not None else 2) * Cc, dtype=torch.float32, device=z2.device)
    ws, wsb = workspace(_hip.lib().iseg_resblock_tail_workspace_bytes(N, H, W, Cc, int(stride), int(z0 is not None)), z2.device)
    _hip.call("iseg_resblock_tail_bwd_reduce", ptr(dout), ptr(out), ptr(z2), ptr(mean2), ptr(rstd2), ptr(z0), ptr(mean0), ptr(rstd0), ptr(sums),
              N, H, W, Cc, int(stride), dt(z2), ptr(ws), wsb, stream())
    return sums


def resblock_tail_bwd_apply(dout, out, z2, mean2, rstd2, gamma2, sums, inv_n2, inv_n0, train, sc_shape, stride, z0=None, mean0=None, rstd0=None,
                            gamma0=None, dgamma2=None, dbeta2=None, dgamma0=None, dbeta0=None):
    """(dz2, dsc): dsc [N, H, W, C] = dz0 (BN0 shortcut) or unpool(g) / count (identity); dgamma / dbeta (+)= the sums by the same launch --
    only while `sums` are this replica's own"""
    _require_cuda(dout, out, z2)
    N, H, W, Cc = sc_shape
    dz2 = torch.empty_like(z2)
    dsc = torch.empty(tuple(sc_shape), dtype=z2.dtype, device=z2.device)
    _hip.call("iseg_resblock_tail_bwd_apply", ptr(dout), ptr(out), ptr(z2), ptr(mean2), ptr(rstd2), ptr(gamma2), ptr(z0), ptr(mean0), ptr(rstd0),
              ptr(gamma0), ptr(sums), float(inv_n2), float(inv_n0), int(train), ptr(dz2), ptr(dsc), ptr(dgamma2), ptr(dbeta2), ptr(dgamma0),
              ptr(dbeta0), N, H, W, Cc, int(stride), dt(z2), stream())
    return dz2, dsc


# ---------------------------------------------------------------------------------------------------------
# depthwise conv
# ---------------------------------------------------------------------------------------------------------
def dwconv2d(x, w, bias, K, dil, pad_t, pad_l, *, flip=False, add=None):
    """x [N,H,W,C]; w [K*K, C] fp32 (Keras [K,K,C,1]); stride 1."""
    _require_cuda(x)
    N, H, W, Cc = x.shape
    y = torch.empty_like(x)
    timer = KERNEL_TIMER[0]
    if timer is not None:      # (bench.py's roofline_memory entry: the depthwise family is the largest non-GEMM group of the flagship step)
        timer.begin(("dwconv", int(N), int(H), int(W), int(Cc), int(K), int(dil), bool(flip), add is not None, x.dtype))
    _hip.call("iseg_dwconv2d_fwd", ptr(x), ptr(w), ptr(bias), ptr(add), ptr(y), N, H, W, Cc, K, dil, pad_t, pad_l, int(flip), dt(x),
              stream())
    if timer is not None:
        timer.end()
    return y


def dwconv2d7_mfma(x, w, bias, pad_t=3, pad_l=3, *, flip=False, add=None):
    """the 7 x 7 depthwise convolution on the matrix cores (csrc/dwconv_mfma.hip), named explicitly; dwconv2d takes this route by itself for large planes"""
    _require_cuda(x)
    N, H, W, Cc = x.shape
    y = torch.empty_like(x)
    _hip.call("iseg_dwconv2d7_mfma", ptr(x), ptr(w), ptr(bias), ptr(add), ptr(y), N, H, W, Cc, pad_t, pad_l, int(flip), stream())
    return y


def dwconv2d_bwd_weight(x, dy, dw, db, K, dil, pad_t, pad_l, accumulate=True):
    N, H, W, Cc = x.shape
    need = _hip.lib().iseg_dwconv2d_bwd_weight_workspace_bytes(N, H, W, Cc, K)
    ws, wsb = workspace(need, x.device)
    _hip.call("iseg_dwconv2d_bwd_weight", ptr(x), ptr(dy), ptr(dw), ptr(db), int(accumulate), N, H, W, Cc, K, dil, pad_t, pad_l,
              dt(x), ptr(ws), wsb, stream())


def dwconv2d7_bwd_weight_mfma(x, dy, dw, db, pad_t=3, pad_l=3, accumulate=True):
    """the 7 x 7 depthwise weight gradient on the matrix cores (csrc/dwconv_wgrad_mfma.hip), named explicitly; dwconv2d_bwd_weight takes this route by
    itself where it measured faster"""
    _require_cuda(x, dy, dw)
    N, H, W, Cc = x.shape
    need = _hip.lib().iseg_dwconv2d_bwd_weight_workspace_bytes(N, H, W, Cc, 7)
    ws, wsb = workspace(need, x.device)
    _hip.call("iseg_dwconv2d7_bwd_weight_mfma", ptr(x), ptr(dy), ptr(dw), ptr(db), int(accumulate), N, H, W, Cc, pad_t, pad_l, ptr(ws), wsb, stream())


def dwconv2d_strided(x, w, bias, K, stride, dil):
    """DepthwiseConv2D(strides=stride, padding='same') at the strided positions only; x [N,H,W,C], w [K*K, C] fp32"""
    _require_cuda(x, w)
    N, H, W, Cc = x.shape
    Ho, pt = same_pad(H, K, stride, dil)
    Wo, pl = same_pad(W, K, stride, dil)
    y = torch.empty((N, Ho, Wo, Cc), dtype=x.dtype, device=x.device)
    _hip.call("iseg_dwconv2d_strided_fwd", ptr(x), ptr(w), ptr(bias), ptr(y), N, H, W, Cc, K, stride, dil, pt, pl, Ho, Wo, dt(x), stream())
    return y


def dwconv2d_strided_bwd_data(dy, w, K, stride, dil, H, W):
    _require_cuda(dy, w)
    N, Ho, Wo, Cc = dy.shape
    _, pt = same_pad(H, K, stride, dil)
    _, pl = same_pad(W, K, stride, dil)
    dx = torch.empty((N, H, W, Cc), dtype=dy.dtype, device=dy.device)
    _hip.call("iseg_dwconv2d_strided_bwd_data", ptr(dy), ptr(w), ptr(dx), N, H, W, Cc, K, stride, dil, pt, pl, Ho, Wo, dt(dy), stream())
    return dx


def dwconv2d_strided_bwd_weight(x, dy, dw, db, K, stride, dil, accumulate=True):
    _require_cuda(x, dy, dw)
    N, H, W, Cc = x.shape
    _, Ho, Wo, _ = dy.shape
    _, pt = same_pad(H, K, stride, dil)
    _, pl = same_pad(W, K, stride, dil)
    need = _hip.lib().iseg_dwconv2d_strided_bwd_weight_workspace_bytes(N, Ho, Wo, Cc, K)
    ws, wsb = workspace(need, x.device)
    _hip.call("iseg_dwconv2d_strided_bwd_weight", ptr(x), ptr(dy), ptr(dw), ptr(db), int(accumulate), N, H, W, Cc, K, stride, dil, pt, pl, Ho, Wo,
              dt(x), ptr(ws), wsb, stream())


# ---------------------------------------------------------------------------------------------------------
# layout / elementwise
# ---------------------------------------------------------------------------------------------------------
def cast(src, dst_dtype, out=None):
    if out is None:
        out = torch.empty(src.shape, dtype=dst_dtype, device=src.device)
    _hip.call("iseg_cast", ptr(src), dt(src), ptr(out), dt(out), src.numel(), stream())
    return out


def scale_cols_cast(src, colscale, dst_dtype):
    rows, cols = src.shape
    out = torch.empty((rows, cols), dtype=dst_dtype, device=src.device)
    _hip.call("iseg_scale_cols_cast", ptr(src), ptr(colscale), ptr(out), rows, cols, dt(out), stream())
    return out


def same_pad(in_size, k, s, d):
    """TF padding="same": returns (out_size, pad_before)."""
    out = -(-in_size // s)
    total = max((out - 1) * s + (k - 1) * d + 1 - in_size, 0)
    return out, total // 2


def im2col(x, KH, KW, sh, sw, dh, dw, pt, pl, Ho, Wo, out_dtype, ldc=None):
    N, H, W, Cc = x.shape
    Kd = KH * KW * Cc
    if ldc is None:
        ldc = (Kd + 7) // 8 * 8
    col = torch.empty((N * Ho * Wo, ldc), dtype=out_dtype, device=x.device)
    _hip.call("iseg_im2col", ptr(x), dt(x), ptr(col), dt(col), N, H, W, Cc, KH, KW, sh, sw, dh, dw, pt, pl, Ho, Wo, ldc, stream())
    return col


def col2im(dcol, N, H, W, Cc, KH, KW, sh, sw, dh, dw, pt, pl, Ho, Wo):
    dx = torch.empty((N, H, W, Cc), dtype=dcol.dtype, device=dcol.device)
    _hip.call("iseg_col2im", ptr(dcol), ptr(dx), N, H, W, Cc, KH, KW, sh, sw, dh, dw, pt, pl, Ho, Wo, dcol.stride(0), dt(dcol),
              stream())
    return dx


def conv_geom(N, H, W, Cin, Cout, KH, KW, sh, sw, dh, dw, pt, pl, Ho, Wo, groups=1):
    return _hip.ConvGeom(N, H, W, Cin, Cout, KH, KW, sh, sw, dh, dw, pt, pl, Ho, Wo, groups)


def conv2d_igemm_supported(geom, dtype):
    """implicit-GEMM convolution (csrc/conv_igemm.hip): bf16 storage, channels per group multiples of 8"""
    return dtype in _DT and bool(_hip.lib().iseg_conv2d_igemm_supported(C.byref(geom), _DT[dtype]))


def _conv_ws(geom, which, device):
    return workspace(_hip.lib().iseg_conv2d_igemm_workspace_bytes(C.byref(geom), which), device)


def conv2d_igemm_fwd(x, w, bias, geom):
    """x [N,H,W,Cin] bf16, w [KH,KW,Cin/groups,Cout] bf16 -> y [N,Ho,Wo,Cout]; the patch matrix is gathered on the fly"""
    _require_cuda(x, w)
    y = torch.empty((geom.N, geom.Ho, geom.Wo, geom.Cout), dtype=x.dtype, device=x.device)
    ws, wsb = _conv_ws(geom, 0, x.device)
    _hip.call("iseg_conv2d_igemm_fwd", ptr(x), ptr(w), ptr(bias), ptr(y), C.byref(geom), dt(x), ptr(ws), wsb, stream())
    return y


def conv2d_igemm_fwd_kt_supported(geom, dtype):
    return dtype in _DT and bool(_hip.lib().iseg_conv2d_igemm_fwd_kt_supported(C.byref(geom), _DT[dtype]))


def conv2d_igemm_fwd_kt(x, wt, bias, geom):
    """the forward pass on the LDS-DMA pipeline: wt = the K-contiguous kernel copy [Cout, KH*KW*Cin] (nn.wt)"""
    _require_cuda(x, wt)
    y = torch.empty((geom.N, geom.Ho, geom.Wo, geom.Cout), dtype=x.dtype, device=x.device)
    ws, wsb = _conv_ws(geom, 0, x.device)
    _hip.call("iseg_conv2d_igemm_fwd_kt", ptr(x), ptr(wt), ptr(bias), ptr(y), C.byref(geom), dt(x), ptr(ws), wsb, stream())
    return y


def conv2d_igemm_bwd_data(dy, w, geom):
    _require_cuda(dy, w)
    dx = torch.empty((geom.N, geom.H, geom.W, geom.Cin), dtype=dy.dtype, device=dy.device)
    ws, wsb = _conv_ws(geom, 1, dy.device)
    _hip.call("iseg_conv2d_igemm_bwd_data", ptr(dy), ptr(w), ptr(dx), C.byref(geom), dt(dy), ptr(ws), wsb, stream())
    return dx


def conv2d_igemm_bwd_weight(x, dy, dw, geom, accumulate=True):
    """dw [KH,KW,Cin/groups,Cout] fp32 (+)= per-tap x^T dy"""
    _require_cuda(x, dy, dw)
    ws, wsb = _conv_ws(geom, 2, x.device)
    _hip.call("iseg_conv2d_igemm_bwd_weight", ptr(x), ptr(dy), ptr(dw), int(accumulate), C.byref(geom), dt(x), ptr(ws), wsb, stream())
    return dw


# ---- patchify convolutions (kernel == stride) as GEMMs over a patch view of the tensor (csrc/conv_patchify.hip) ----
PATCH_FWD, PATCH_BWD_DATA, PATCH_BWD_WEIGHT = 0, 1, 2


def conv2d_patch_supported(geom, dtype, which):
    """pass `which` of this convolution runs as a plain LDS-DMA GEMM over the patch view (the three passes are independent)"""
    return dtype in _DT and bool(_hip.lib().iseg_conv2d_patch_supported(C.byref(geom), _DT[dtype], int(which)))


def conv2d_patch_fwd(x, wt, bias, geom):
    """y [N,Ho,Wo,Cout] = patches(x) @ wt^T (+ bias); wt = the K-contiguous kernel copy [Cout, KH*KW*Cin] (nn.wt)"""
    _require_cuda(x, wt)
    y = torch.empty((geom.N, geom.Ho, geom.Wo, geom.Cout), dtype=x.dtype, device=x.device)
    _hip.call("iseg_conv2d_patch_fwd", ptr(x), ptr(wt), ptr(bias), ptr(y), C.byref(geom), dt(x), None, 0, stream())
    return y


def conv2d_patch_bwd_data(dy, w, geom):
    """dx [N,H,W,Cin] = dy @ w^T written through the patch view: the bits of gemm + col2im without the column buffer"""
    _require_cuda(dy, w)
    dx = torch.empty((geom.N, geom.H, geom.W, geom.Cin), dtype=dy.dtype, device=dy.device)
    _hip.call("iseg_conv2d_patch_bwd_data", ptr(dy), ptr(w), ptr(dx), C.byref(geom), dt(dy), None, 0, stream())
    return dx


def conv2d_patch_bwd_weight(x, dy, dw, geom, accumulate=True, bias_grad=None):
    """dw [KH,KW,Cin,Cout] fp32 (+)= patches(x)^T @ dy; bias_grad [Cout] fp32 (+)= column sums of dy from the kernel's ones-row"""
    _require_cuda(x, dy, dw)
    ws, wsb = _conv_ws(geom, 3, x.device)
    _hip.call("iseg_conv2d_patch_bwd_weight", ptr(x), ptr(dy), ptr(dw), ptr(bias_grad), int(accumulate), C.byref(geom), dt(x), ptr(ws), wsb, stream())
    return dw


# ---- several convolutions of one input (csrc/conv_igemm.hip: grouped forward / weight gradient, K-joined data gradient) ----
def conv_branches(N, H, W, Cin, Cout, taps):
    """branch table for `taps` = [(KH, KW, dh, dw), ...] of a [N,H,W,Cin] -> Cout convolution family (stride 1, "same" padding); the operand
    pointers are filled in by the three passes below"""
    t = _hip.ConvBranches(N, H, W, Cin, Cout, len(taps))
    for b, (kh, kw, dh, dw) in zip(t.b, taps[:_hip.CONV_MAX_BRANCHES]):
        b.KH, b.KW, b.dh, b.dw = kh, kw, dh, dw
        b.pt, b.pl = same_pad(H, kh, 1, dh)[1], same_pad(W, kw, 1, dw)[1]
    return t


def conv2d_branches_supported(table, dtype):
    return dtype in _DT and bool(_hip.lib().iseg_conv2d_branches_supported(C.byref(table), _DT[dtype]))


def conv_branches_joined_geom(table):
    """the K-joined data gradient as ONE stride-1 data gradient whose taps are the taps of every branch in a row: the geometry that sizes its
    workspace (iseg_conv2d_igemm_workspace_bytes, pass 1)"""
    taps = sum(b.KH * b.KW for b in table.b[:table.count])
    return conv_geom(table.N, table.H, table.W, table.Cin, table.Cout, 1, taps, 1, 1, 1, 1, 0, 0, table.H, table.W, 1)


def conv2d_branches_fwd(x, wts, table, biases=None):
    """x [N,H,W,Cin], wts[b] = the K-contiguous kernel copy [Cout, KH*KW*Cin] (nn.wt) -> one [N,H,W,Cout] per branch, ONE launch"""
    _require_cuda(x, *wts)
    ys = [torch.empty((table.N, table.H, table.W, table.Cout), dtype=x.dtype, device=x.device) for _ in wts]
    for i, (b, wt, y) in enumerate(zip(table.b, wts, ys)):
        b.wt, b.y, b.ldy, b.y_col = ptr(wt), ptr(y), table.Cout, 0
        b.bias = ptr(biases[i]) if biases is not None else None
    _hip.call("iseg_conv2d_branches_fwd", ptr(x), C.byref(table), dt(x), None, 0, stream())
    return ys


def conv2d_branches_bwd_data(dys, lddys, ws_, table, residual=None):
    """dx [N,H,W,Cin] = sum over branches of conv^T(dy_b, w_b) (+ residual) as one product; dys[b] = rows of lddys[b] elements, ws_[b] = Keras kernel"""
    _require_cuda(*dys, *ws_)
    dx = torch.empty((table.N, table.H, table.W, table.Cin), dtype=dys[0].dtype, device=dys[0].device)
    for b, dy, ld, w in zip(table.b, dys, lddys, ws_):
        b.dy, b.lddy, b.w = ptr(dy), ld, ptr(w)
    ws, wsb = _conv_ws(conv_branches_joined_geom(table), 1, dx.device)
    _hip.call("iseg_conv2d_branches_bwd_data", C.byref(table), ptr(dx), ptr(residual), table.Cin, dt(dx), ptr(ws), wsb, stream())
    return dx


def conv2d_branches_bwd_weight(x, dys, lddys, gws, table, accumulate=True):
    """gws[b] [KH,KW,Cin,Cout] fp32 (+)= per-tap x^T dy_b, every branch in ONE launch"""
    _require_cuda(x, *dys, *gws)
    for b, dy, ld, gw in zip(table.b, dys, lddys, gws):
        b.dy, b.lddy, b.gw = ptr(dy), ld, ptr(gw)
    _hip.call("iseg_conv2d_branches_bwd_weight", ptr(x), C.byref(table), int(accumulate), dt(x), None, 0, stream())
    return gws


def colsum(x, ldx, batch_stride, batch, rows, Cc, out, scale=1.0, accumulate=False):
    if Cc > 8192 and batch == 1 and scale == 1.0:
        # few rows, very wide (token-axis sums, score gradients): the LDS-staged kernel would need C floats of LDS per workgroup
        L = _hip.lib()
        ws, wsb = workspace(L.iseg_colsum_wide_workspace_bytes(rows, Cc), x.device)
        _hip.check(L.iseg_colsum_wide(ptr(x), ldx, rows, Cc, ptr(out), int(accumulate), dt(x), ptr(ws), wsb, stream()), "iseg_colsum_wide")
        return out
    need = _hip.lib().iseg_colsum_workspace_bytes(batch, rows, Cc)
    ws, wsb = workspace(need, x.device)
    _hip.call("iseg_colsum", ptr(x), ldx, batch_stride, batch, rows, Cc, ptr(out), scale, int(accumulate), dt(x), ptr(ws), wsb,
              stream())
    return out


def accumulate_pair(src, n, dst0, dst1):
    """dst0 += src[:n]; dst1 += src[n:2n]   (fp32; None destinations are skipped)"""
    if dst0 is None and dst1 is None:
        return
    _hip.call("iseg_accumulate_pair", ptr(src), int(n), ptr(dst0), ptr(dst1), stream())


def broadcast_rows(v, y, ldy, batch_stride, batch, rows, Cc, scale=1.0, accumulate=False):
    _hip.call("iseg_broadcast_rows", ptr(v), dt(v), ptr(y), ldy, batch_stride, batch, rows, Cc, scale, int(accumulate), dt(y),
              stream())
    return y


def axpby(a, b, alpha=1.0, beta=1.0, out=None):
    if out is None:
        out = torch.empty_like(a)
    _hip.call("iseg_axpby", ptr(a), ptr(b), ptr(out), alpha, beta, a.numel(), dt(a), stream())
    return out


def rowscale(x2d, s, rows_per_group):
    rows, Cc = x2d.shape
    y = torch.empty_like(x2d)
    _hip.call("iseg_rowscale", ptr(x2d), ptr(s), ptr(y), rows, Cc, rows_per_group, dt(x2d), stream())
    return y


# Device-resident addend of every dropout / drop-path seed.  None outside graph capture; iseg_amd.graphs.GraphedTrainStep points it at a one-word
# device buffer while it captures a training step and moves the word on before every replay, so the replayed launches (frozen
# arguments) draw the numbers the eager step would have drawn.
_SEED_OFFSET = [None]


def set_seed_offset(t):
    _SEED_OFFSET[0] = t


def dropout(x, rate, seed):
    y = torch.empty_like(x)
    _hip.call("iseg_dropout", ptr(x), ptr(y), x.numel(), rate, seed, ptr(_SEED_OFFSET[0]), dt(x), stream())
    return y


def drop_path_mask(n, keep_prob, seed, device):
    s = torch.empty(n, dtype=torch.float32, device=device)
    _hip.call("iseg_drop_path_mask", ptr(s), n, keep_prob, seed, ptr(_SEED_OFFSET[0]), stream())
    return s


def drop_path_masks(keep_probs_dev, n, seed):
    """[P, n] per-sample drop-path factors, row p with keep probability keep_probs_dev[p]: one launch for a whole step"""
    P = keep_probs_dev.numel()
    s = torch.empty((P, n), dtype=torch.float32, device=keep_probs_dev.device)
    _hip.call("iseg_drop_path_masks", ptr(s), ptr(keep_probs_dev), P, n, seed, ptr(_SEED_OFFSET[0]), stream())
    return s


def fill_f32(t, value):
    _hip.call("iseg_fill_f32", ptr(t), value, t.numel(), stream())
    return t


def act_fwd(x, act):
    y = torch.empty_like(x)
    _hip.call("iseg_act_fwd", ptr(x), ptr(y), x.numel(), act, dt(x), stream())
    return y


def act_bwd(dy, aux, act):
    dx = torch.empty_like(dy)
    _hip.call("iseg_act_bwd", ptr(dy), ptr(aux), ptr(dx), dy.numel(), act, dt(dy), stream())
    return dx


def dcnv2_sample_fwd(x, offset):
    """x [N,H,W,C], offset [N,H,W,27] -> col [N,H,W,9,C] (csrc/dcnv3.hip dcnv2_sample_*; layers/dcn_v2.py:114-229)"""
    _require_cuda(x, offset)
    N, H, W, Cc = x.shape
    col = torch.empty((N, H, W, 9, Cc), dtype=x.dtype, device=x.device)
    _hip.call("iseg_dcnv2_sample_fwd", ptr(x), ptr(offset), ptr(col), N, H, W, Cc, dt(x), stream())
    return col


def dcnv2_sample_bwd(x, offset, dcol):
    N, H, W, Cc = x.shape
    dx = torch.empty((N, H, W, Cc), dtype=torch.float32, device=x.device)
    doff = torch.empty_like(offset)
    ws, wsb = workspace(_hip.lib().iseg_dcnv2_sample_bwd_workspace_bytes(N, H, W, Cc), x.device)
    _hip.call("iseg_dcnv2_sample_bwd", ptr(x), ptr(offset), ptr(dcol), ptr(dx), ptr(doff), N, H, W, Cc, dt(x), ptr(ws), wsb, stream())
    return dx, doff


def qkv_rope(qkv, q_bias, v_bias, emb, tokens, prefix, C, head_dim, inverse=False, out=None):
    """packed attention rows [B * tokens, 3 C] (csrc/eva.hip): q / v bias, rotary embedding on q and k of the tokens >= prefix; out=None: in place"""
    _require_cuda(qkv)
    out = qkv if out is None else out
    _hip.call("iseg_qkv_rope", ptr(qkv), ptr(out), ptr(q_bias), ptr(v_bias), ptr(emb), qkv.numel() // (3 * C), tokens, prefix, C, head_dim, int(inverse),
              dt(qkv), stream())
    return out


def glu_fwd(gate, x, act):
    """act(gate) * x; gate / x: [rows, cols] views with unit column stride (row strides free)"""
    rows, cols = gate.shape
    out = torch.empty((rows, cols), dtype=gate.dtype, device=gate.device)
    _hip.call("iseg_glu_fwd", ptr(gate), gate.stride(0), ptr(x), x.stride(0), ptr(out), cols, rows, cols, act, dt(gate), stream())
    return out


def glu_bwd(dout, gate, x, dgate, dx, act):
    rows, cols = gate.shape
    _hip.call("iseg_glu_bwd", ptr(dout), dout.stride(0), ptr(gate), gate.stride(0), ptr(x), x.stride(0), ptr(dgate), dgate.stride(0), ptr(dx),
              dx.stride(0), rows, cols, act, dt(gate), stream())


def copy2d(src, ld_src, dst, ld_dst, rows, cols):
    _hip.call("iseg_copy2d", ptr(src), ld_src, ptr(dst), ld_dst, rows, cols, dt(src), stream())
    return dst


def add2d(src, ld_src, dst, ld_dst, rows, cols):
    _hip.call("iseg_add2d_f32", ptr(src), ld_src, ptr(dst), ld_dst, rows, cols, stream())


def scale_rows(x2d, s):
    y = torch.empty_like(x2d)
    _hip.call("iseg_scale_rows_f32", ptr(x2d), ptr(s), ptr(y), x2d.shape[0], x2d.shape[1], stream())
    return y


def layerscale_grads(Z, W2, b2, gamma, S, dW2, dgamma, db2, accumulate=True):
    Kd, Nd = Z.shape
    need = _hip.lib().iseg_layerscale_grads_workspace_bytes(Kd, Nd)
    ws, wsb = workspace(need, Z.device)
    _hip.call("iseg_layerscale_grads", ptr(Z), ptr(W2), ptr(b2), ptr(gamma), ptr(S), ptr(dW2), ptr(dgamma), ptr(db2), Kd, Nd,
              int(accumulate), ptr(ws), wsb, stream())


def layerscale_grads_slabs(slabs, nslabs, W2, b2, gamma, dW2, dgamma, db2, accumulate=True, extra=None):
    """layerscale_grads from the unreduced split-K slabs of Z = g^T dout (dense_wgrad_slabs): Z and S = colsum(dout) are summed on load.
    extra = dense_wgrad_pair(..., defer_second=True)[2]: the other product's slabs are summed into their gradients by the same launch"""
    Kd, Nd = W2.shape
    need = _hip.lib().iseg_layerscale_grads_workspace_bytes(Kd, Nd)
    ws, wsb = workspace(need, slabs.device)
    if extra is not None:
        part2, p2, n2, out0, out1, n0, acc2 = extra
        _hip.call("iseg_layerscale_grads_slabs_reduce", ptr(slabs), int(nslabs), ptr(W2), ptr(b2), ptr(gamma), ptr(dW2), ptr(dgamma), ptr(db2), Kd,
                  Nd, int(accumulate), ptr(ws), wsb, ptr(part2), int(p2), int(n2), ptr(out0), ptr(out1), int(n0), int(acc2), stream())
        return
    _hip.call("iseg_layerscale_grads_slabs", ptr(slabs), int(nslabs), ptr(W2), ptr(b2), ptr(gamma), ptr(dW2), ptr(dgamma), ptr(db2), Kd, Nd,
              int(accumulate), ptr(ws), wsb, stream())


# ---------------------------------------------------------------------------------------------------------
# input pipeline (csrc/augment.hip)
# ---------------------------------------------------------------------------------------------------------
def augment_params_ints():
    return int(_hip.lib().iseg_augment_params_ints())


def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def augment_params_floats():
    return int(_hip.lib().iseg_augment_params_floats())


def augment_channel_means(images, params, fparams):
    """fill slots 2..4 of the photometric table with the channel means of each sample's scaled (+ brightness) image (tf.image.adjust_contrast)"""
    _require_cuda(images, params, fparams)
    B, Hs, Ws, _ = images.shape
    need = _hip.lib().iseg_augment_means_workspace_bytes(B)
    ws, wsb = workspace(need, images.device)
    _hip.call("iseg_augment_channel_means", ptr(images.contiguous()), 0 if images.dtype == torch.float32 else 2, ptr(params), ptr(fparams), B, Hs, Ws,
              ptr(ws), wsb, stream())


def augment_crop_batch(images, labels, params, mean_pixel, norm_scale, norm_shift, ignore_label, crop_h, crop_w, seed, fparams=None):
    """scale -> [brightness / contrast / saturation / hue] -> pad -> crop -> flip -> erase -> [eval noise] -> normalise as one gather
    (data_process/pipeline.py:85-170); params: int32 [B, n], fparams: float32 [B, m] or None, both on the device"""
    _require_cuda(images, params)
    if images.dtype not in (torch.float32, torch.uint8):
        raise TypeError("augment_crop_batch takes float32 or uint8 images")
    B, Hs, Ws, _ = images.shape
    images = images.contiguous()
    out = torch.empty((B, crop_h, crop_w, 3), dtype=torch.float32, device=images.device)
    lab = out_lab = None
    if labels is not None:
        lab = labels.contiguous()
        if lab.dtype != torch.int32:
            lab = lab.to(torch.int32)
        out_lab = torch.empty((B, crop_h, crop_w), dtype=torch.int32, device=images.device)
    _hip.call("iseg_augment_crop_batch", ptr(images), 0 if images.dtype == torch.float32 else 2, ptr(lab), ptr(params.contiguous()),
              ptr(fparams), _f3(mean_pixel), _f3(norm_scale), _f3(norm_shift), int(ignore_label), ptr(out), ptr(out_lab), B, Hs, Ws,
              int(crop_h), int(crop_w), int(seed), stream())
    return out, out_lab


def projective_transform_batch(images, labels, transforms, sizes=None, interpolation="bilinear", image_fill=0.0, replace=None, label_fill=255):
    """tf.raw_ops.ImageProjectiveTransformV3, CONSTANT fill mode, for a padded batch in one launch (csrc/projective.hip;
    augments/random_rotate_augment.py:20-115, :221-296).  images [B, Hs, Ws, C] (C in 1..4), labels [B, Hs, Ws] int32 or None, transforms
    [B, 8] float32 (output (x, y) -> input point), sizes [B, 2] int32 (H, W) of each sample in its slot or None; replace [C] or None:
    out < -1e-6 -> replace[c].  Labels are sampled nearest with label_fill.  uint8 images are converted to float32 here and the output is
    always float32: TF keeps the input's type, but the reference's fill of -1 and where(out < -1e-6) presuppose a float image anyway.
    -> (float32 [B, Hs, Ws, C], int32 [B, Hs, Ws] or None)"""
    _require_cuda(images, labels, transforms, sizes)
    if interpolation not in ("nearest", "bilinear"):
        raise ValueError(f"interpolation must be 'nearest' or 'bilinear', got {interpolation!r}")
    if images.dim() != 4 or 0 in images.shape:
        raise ValueError(f"images must be a non-empty [B, Hs, Ws, C] batch, got {tuple(images.shape)}")
    B, Hs, Ws, Cc = images.shape
    images = images.to(torch.float32).contiguous()
    transforms = transforms.to(torch.float32).contiguous()
    if tuple(transforms.shape) != (B, 8):
        raise ValueError(f"transforms must be [{B}, 8], got {tuple(transforms.shape)}")
    if sizes is not None:
        sizes = sizes.to(torch.int32).contiguous()
        if tuple(sizes.shape) != (B, 2):
            raise ValueError(f"sizes must be [{B}, 2], got {tuple(sizes.shape)}")
    out = torch.empty((B, Hs, Ws, Cc), dtype=torch.float32, device=images.device)
    lab = out_lab = None
    if labels is not None:
        if tuple(labels.shape) != (B, Hs, Ws):
            raise ValueError(f"labels must be [{B}, {Hs}, {Ws}], got {tuple(labels.shape)}")
        lab = labels.to(torch.int32).contiguous()
        out_lab = torch.empty((B, Hs, Ws), dtype=torch.int32, device=images.device)
    rep = None
    if replace is not None:
        if len(replace) != Cc:
            raise ValueError(f"replace needs one value per channel ({Cc}), got {len(replace)}")
        rep = (C.c_float * Cc)(*[float(v) for v in replace])
    _hip.call("iseg_projective_transform_batch", ptr(images), ptr(lab), ptr(transforms), ptr(sizes), ptr(out), ptr(out_lab), B, Hs, Ws, Cc,
              1 if interpolation == "bilinear" else 0, float(image_fill), rep, int(label_fill), stream())
    return out, out_lab


def normalize_image(x, norm_scale, norm_shift):
    _require_cuda(x)
    y = torch.empty_like(x)
    _hip.call("iseg_normalize_image", ptr(x), ptr(y), x.numel() // 3, _f3(norm_scale), _f3(norm_shift), stream())
    return y


# ---------------------------------------------------------------------------------------------------------
# resize / loss / metric / optimizer
# ---------------------------------------------------------------------------------------------------------
def resize_bilinear(x, Ho, Wo, out_dtype=None, align_corners=False):
    """align_corners: tf.compat.v1.image.resize(..., align_corners=True) coordinates instead of TF2's half-pixel centres"""
    _require_cuda(x)
    N, Hi, Wi, Cc = x.shape
    y = torch.empty((N, Ho, Wo, Cc), dtype=out_dtype or x.dtype, device=x.device)
    _hip.call("iseg_resize_bilinear_ac_fwd" if align_corners else "iseg_resize_bilinear_fwd", ptr(x), dt(x), ptr(y), dt(y), N, Hi, Wi, Ho, Wo,
              Cc, stream())
    return y


def resize_bilinear_bwd(dy, Hi, Wi, dx_dtype, dx_add=None, align_corners=False):
    N, Ho, Wo, Cc = dy.shape
    dx = torch.empty((N, Hi, Wi, Cc), dtype=dx_dtype, device=dy.device)
    need = _hip.lib().iseg_resize_bilinear_bwd_workspace_bytes(N, Hi, Wi, Ho, Wo, Cc)
    ws, wsb = workspace(need, dy.device)
    _hip.call("iseg_resize_bilinear_ac_bwd" if align_corners else "iseg_resize_bilinear_bwd", ptr(dy), dt(dy), ptr(dx), dt(dx), ptr(dx_add), N,
              Hi, Wi, Ho, Wo, Cc, ptr(ws), wsb, stream())
    return dx


def resize_nearest_i32(x, Ho, Wo):
    N, Hi, Wi, Cc = x.shape
    y = torch.empty((N, Ho, Wo, Cc), dtype=torch.int32, device=x.device)
    _hip.call("iseg_resize_nearest_i32", ptr(x), ptr(y), N, Hi, Wi, Ho, Wo, Cc, stream())
    return y


def scale_dev(x, s_dev):
    y = torch.empty_like(x)
    _hip.call("iseg_scale_dev", ptr(x), ptr(s_dev), ptr(y), x.numel(), dt(x), stream())
    return y


def softmax_ce_ignore(logits2d, labels1d, ignore_label, *, class_w=None, want_px=True, want_sum=False, sum_scale=1.0,
                      want_grad=False, grad_scale=1.0, grad_px=None, focal=None, cm=None):
    """focal = (alpha, gamma) selects keras' CategoricalFocalCrossentropy instead of the plain cross-entropy; cm (int64 [C*C]) also
    accumulates the confusion matrix of argmax(logits) in the same pass (plain cross-entropy only)"""
    _require_cuda(logits2d, labels1d)
    P, Cc = logits2d.shape
    dev = logits2d.device
    loss_px = torch.empty(P, dtype=torch.float32, device=dev) if want_px else None
    loss_sum = torch.empty(1, dtype=torch.float32, device=dev) if want_sum else None
    dlogits = torch.empty_like(logits2d) if want_grad else None
    need = _hip.lib().iseg_softmax_ce_workspace_bytes(P, Cc) if want_sum else 0
    ws, wsb = workspace(need, dev)
    if cm is not None:
        if focal is not None:
            raise ValueError("softmax_ce_ignore: cm rides the plain cross-entropy kernel only")
        _hip.call("iseg_softmax_ce_confusion", ptr(logits2d), ptr(labels1d), ptr(class_w), P, Cc, ignore_label, ptr(loss_px), ptr(loss_sum),
                  sum_scale, ptr(dlogits), grad_scale, ptr(grad_px), ptr(cm), ptr(ws), wsb, stream())
    elif focal is not None:
        _hip.call("iseg_softmax_focal_ce_ignore", ptr(logits2d), ptr(labels1d), ptr(class_w), P, Cc, ignore_label, float(focal[0]),
                  float(focal[1]), ptr(loss_px), ptr(loss_sum), sum_scale, ptr(dlogits), grad_scale, ptr(grad_px), ptr(ws), wsb, stream())
    else:
        _hip.call("iseg_softmax_ce_ignore", ptr(logits2d), ptr(labels1d), ptr(class_w), P, Cc, ignore_label, ptr(loss_px), ptr(loss_sum),
                  sum_scale, ptr(dlogits), grad_scale, ptr(grad_px), ptr(ws), wsb, stream())
    return loss_px, loss_sum, dlogits


OHEM_STATE_INTS, OHEM_PARTIAL_FLOATS = 1032, 1024      # ISEG_OHEM_STATE_INTS, ISEG_OHEM_PARTIAL_FLOATS of include/iseg_hip.h


def ohem_label_prob(logits2d, labels1d, ignore_label, *, prob=None):
    """losses/ohem.py:18-20 (csrc/ohem.hip): prob [P] fp32 = softmax probability of the labelled class, exactly 0 on a zero row; labels follow
    the rule of softmax_ce_ignore (ignore_label == 0 shifts them down by one, a class outside [0, C) is the zero row)"""
    _require_cuda(logits2d, labels1d, prob)
    if logits2d.dtype != torch.float32 or labels1d.dtype != torch.int32:
        raise TypeError(f"ohem_label_prob: float32 logits and int32 labels, got {logits2d.dtype} and {labels1d.dtype}")
    P, Cc = logits2d.shape
    if labels1d.numel() != P or not (logits2d.is_contiguous() and labels1d.is_contiguous()):
        raise ValueError(f"ohem_label_prob: contiguous logits [P,C] and labels [P], got {tuple(logits2d.shape)} and {tuple(labels1d.shape)}")
    if prob is None:
        prob = torch.empty(P, dtype=torch.float32, device=logits2d.device)
    elif prob.dtype != torch.float32 or prob.numel() != P or not prob.is_contiguous():
        raise ValueError(f"ohem_label_prob: prob is a contiguous float32 [{P}]")
    _hip.call("iseg_ohem_label_prob", ptr(logits2d), ptr(labels1d), P, Cc, int(ignore_label), ptr(prob), stream())
    return prob


def ohem_select(values, loss, min_kept_total, thresh, *, want_loss=False, want_sum=False, sum_scale=1.0):
    """losses/ohem.py:22-37 (csrc/ohem.hip): thresh a float -> values is the labelled-class probability, keep = values < max(k-th largest, thresh)
    with k = min(min_kept_total, nnz - 1); thresh None -> values is the loss, keep = values > (min_kept_total-th largest).  loss [P] may be values.
    returns (keep [P] fp32 0/1, loss_out [P] | None, masked_sum [1] = sum_scale * sum(keep * loss) | None, threshold [1], nnz [1] int32);
    nothing is read back"""
    _require_cuda(values, loss)
    for name, t in (("values", values), ("loss", loss)):
        if t is not None and (t.dtype != torch.float32 or t.dim() != 1 or not t.is_contiguous() or t.numel() != values.numel()):
            raise ValueError(f"ohem_select: {name} is a contiguous float32 [P]")
    P = values.numel()
    if thresh is None and not 0 <= int(min_kept_total) < P:
        raise ValueError(f"ohem_select: index {int(min_kept_total)} of {P} sorted losses (min_kept * batch_size must be less than N*H*W)")
    dev = values.device
    keep = torch.empty(P, dtype=torch.float32, device=dev)
    loss_out = torch.empty(P, dtype=torch.float32, device=dev) if want_loss else None
    masked_sum = torch.empty(1, dtype=torch.float32, device=dev) if want_sum else None
    threshold = torch.empty(1, dtype=torch.float32, device=dev)
    nnz = torch.empty(1, dtype=torch.int32, device=dev)
    state = torch.empty(OHEM_STATE_INTS, dtype=torch.int32, device=dev)
    partials = torch.empty(OHEM_PARTIAL_FLOATS, dtype=torch.float32, device=dev) if want_sum else None
    _hip.call("iseg_ohem_select", ptr(values), ptr(loss), P, int(min_kept_total), 0.0 if thresh is None else float(thresh), int(thresh is None),
              ptr(keep), ptr(loss_out), ptr(masked_sum), float(sum_scale), ptr(threshold), ptr(nnz), ptr(state), ptr(partials), stream())
    return keep, loss_out, masked_sum, threshold, nnz


MASKLOSS_SIGMOID, MASKLOSS_DICE, MASKLOSS_CE, MASKLOSS_FOCAL_SIGMOID, MASKLOSS_FOCAL_CE, MASKLOSS_CLASS_BALANCING = 1, 2, 4, 8, 16, 32


def mask_loss(logits3d, labels2d, ignore_label, flags, coefs, *, want_px=False, want_mean=False, mean_scale=1.0, want_grad=False,
              grad_scale=1.0, grad_px=None):
    """MaskLoss of losses/mask_loss.py (csrc/mask_loss.hip): logits [B,HW,C] fp32, labels [B,HW] int32, coefs = (sigmoid, dice, ce).
    returns (loss_px [B*HW] | None, loss_mean [1] | None, dlogits | None); with grad_px the gradient is that of sum(grad_px * loss_px)"""
    _require_cuda(logits3d, labels2d, grad_px)
    B, HW, Cc = logits3d.shape
    dev = logits3d.device
    loss_px = torch.empty(B * HW, dtype=torch.float32, device=dev) if want_px else None
    loss_mean = torch.empty(1, dtype=torch.float32, device=dev) if want_mean else None
    dlogits = torch.empty_like(logits3d) if want_grad else None
    ws, wsb = workspace(_hip.lib().iseg_mask_loss_workspace_bytes(B, HW, Cc), dev)
    _hip.call("iseg_mask_loss", ptr(logits3d), ptr(labels2d), B, HW, Cc, int(ignore_label), int(flags), float(coefs[0]), float(coefs[1]),
              float(coefs[2]), ptr(loss_px), ptr(loss_mean), float(mean_scale), ptr(dlogits), float(grad_scale), ptr(grad_px), ptr(ws), wsb,
              stream())
    return loss_px, loss_mean, dlogits


SOD_WFM = 1
SOD_STATE_DOUBLES, SOD_INTS = 1032, 544
SOD_CALLS = [0]      # launches of the shared passes (tests count them: a metric set updates all of its metrics from ONE call)


def sod_metrics(pred, gt, *, normalize=False, wfm=True, alpha=0.5, beta_fm=0.3, beta_wfm=1.0, state=None, count=None, want_ints=False,
                want_per_image=False, want_dist=False):
    """SOD metrics of metrics/sod/sod_metrics.py (csrc/sod_metrics.hip): pred [B,H,W] fp32 in [0,1] (uint8 under normalize), gt [B,H,W] bool / uint8.
    Adds every image's scores to state [1032] fp64 and B to count [1] int64 (see include/iseg_hip.h for the layout); nothing is read back.
    returns (ints [B,544] int32 | None, per_image [B,1032] fp64 | None, dist2 [B,H,W] int32 | None, nearest [B,H,W] int32 | None)"""
    _require_cuda(pred, gt, state, count)
    B, H, W = pred.shape
    if tuple(gt.shape) != (B, H, W):
        raise ValueError("Shape mismatch between prediction and ground truth")
    if normalize and pred.dtype != torch.uint8 or not normalize and pred.dtype != torch.float32:
        raise TypeError("sod_metrics: pred is float32 in [0, 1], or uint8 with normalize=True")
    if gt.dtype not in (torch.bool, torch.uint8):
        raise TypeError("sod_metrics: gt is bool or uint8")
    if not (pred.is_contiguous() and gt.is_contiguous()):
        raise ValueError("sod_metrics: contiguous tensors only")
    dev = pred.device
    flags = SOD_WFM if wfm else 0
    ints = torch.empty(B, SOD_INTS, dtype=torch.int32, device=dev) if want_ints else None
    per = torch.empty(B, SOD_STATE_DOUBLES, dtype=torch.float64, device=dev) if want_per_image else None
    d2 = torch.empty(B, H, W, dtype=torch.int32, device=dev) if want_dist and wfm else None
    nn_ = torch.empty(B, H, W, dtype=torch.int32, device=dev) if want_dist and wfm else None
    ws, wsb = workspace(_hip.lib().iseg_sod_metrics_workspace_bytes(B, H, W, flags), dev)
    SOD_CALLS[0] += 1
    _hip.call("iseg_sod_metrics", ptr(pred), int(normalize), ptr(gt), int(normalize), B, H, W, flags, float(alpha), float(beta_fm), float(beta_wfm),
              ptr(state), ptr(count), ptr(ints), ptr(per), ptr(d2), ptr(nn_), ptr(ws), wsb, stream())
    return ints, per, d2, nn_


(SODV2_IOU, SODV2_SPECIFICITY, SODV2_DICE, SODV2_OA, SODV2_KAPPA, SODV2_PRECISION, SODV2_RECALL, SODV2_FPR, SODV2_BER,
 SODV2_FMEASURE) = range(10)
SODV2_DYNAMIC, SODV2_ADAPTIVE, SODV2_BINARY = 1, 2, 4
SODV2_MAX_HANDLERS, SODV2_HANDLER_DOUBLES, SODV2_INTS = 32, 264, 520
SODV2_CALLS = [0]      # calls of iseg_sod_fmv2 (tests count them: an evaluator updates all of its handlers from ONE call)


def sod_fmv2(pred, gt, handlers, *, normalize=False, state=None, count=None, want_ints=False, want_per_image=False):
    """FmeasureV2 handlers of metrics/sod/fmeasurev2.py (csrc/sod_fmv2.hip): pred [B,H,W] fp32 in [0,1] (uint8 under normalize), gt [B,H,W]
    bool / uint8, handlers a sequence of (kind, modes, beta): SODV2_<kind>, an OR of SODV2_DYNAMIC / ADAPTIVE / BINARY, the F-measure's beta.
    Adds every image's records to state [n,264] fp64 and B to count [1] int64 (see include/iseg_hip.h for the layout); nothing is read back.
    returns (ints [B,520] int32 | None, per_image [B,n,264] fp64 | None)"""
    _require_cuda(pred, gt, state, count)
    B, H, W = pred.shape
    if tuple(gt.shape) != (B, H, W):
        raise ValueError("Shape mismatch between prediction and ground truth")
    if normalize and pred.dtype != torch.uint8 or not normalize and pred.dtype != torch.float32:
        raise TypeError("sod_fmv2: pred is float32 in [0, 1], or uint8 with normalize=True")
    if gt.dtype not in (torch.bool, torch.uint8):
        raise TypeError("sod_fmv2: gt is bool or uint8")
    if not (pred.is_contiguous() and gt.is_contiguous()):
        raise ValueError("sod_fmv2: contiguous tensors only")
    handlers = list(handlers)
    n = len(handlers)
    if state is not None and (state.dtype != torch.float64 or state.numel() != n * SODV2_HANDLER_DOUBLES or not state.is_contiguous()):
        raise ValueError(f"sod_fmv2: state is a contiguous float64 [{n}, {SODV2_HANDLER_DOUBLES}]")
    kinds = (C.c_int32 * n)(*[int(h[0]) for h in handlers])
    modes = (C.c_int32 * n)(*[int(h[1]) for h in handlers])
    betas = (C.c_double * n)(*[float(h[2]) for h in handlers])
    dev = pred.device
    ints = torch.empty(B, SODV2_INTS, dtype=torch.int32, device=dev) if want_ints else None
    per = torch.empty(B, n, SODV2_HANDLER_DOUBLES, dtype=torch.float64, device=dev) if want_per_image else None
    ws, wsb = workspace(_hip.lib().iseg_sod_fmv2_workspace_bytes(B, H, W, n), dev)
    SODV2_CALLS[0] += 1
    _hip.call("iseg_sod_fmv2", ptr(pred), int(normalize), ptr(gt), int(normalize), B, H, W, n, kinds, modes, betas, ptr(state), ptr(count),
              ptr(ints), ptr(per), ptr(ws), wsb, stream())
    return ints, per


def ccl_label(mask, *, labels=None, counts=None):
    """connected-components labelling of ops/ccl.py (csrc/ccl.hip): mask [N,H,W] (or [H,W]: one image) int32 / uint8 / bool, any non-zero value
    foreground.  returns (labels int32 like mask: 0 background, components 1, 2, ... in the raster order of their first pixel, 4-connected;
    counts [N] int32: components per image)"""
    if mask.dtype not in (torch.int32, torch.uint8, torch.bool):
        raise TypeError(f"ccl_label: mask is int32, uint8 or bool, got {mask.dtype}")
    if mask.dim() not in (2, 3):
        raise ValueError(f"ccl_label: mask is [N,H,W] or [H,W], got {tuple(mask.shape)}")
    _require_cuda(mask, labels, counts)
    if not mask.is_contiguous():
        raise ValueError("ccl_label: contiguous tensors only")
    N, H, W = (1,) + tuple(mask.shape) if mask.dim() == 2 else tuple(mask.shape)
    dev = mask.device
    if labels is None:
        labels = torch.empty(mask.shape, dtype=torch.int32, device=dev)
    elif labels.dtype != torch.int32 or labels.shape != mask.shape or not labels.is_contiguous():
        raise ValueError("ccl_label: labels is a contiguous int32 tensor of the mask's shape")
    if counts is None:
        counts = torch.empty(N, dtype=torch.int32, device=dev)
    elif counts.dtype != torch.int32 or counts.numel() != N or not counts.is_contiguous():
        raise ValueError(f"ccl_label: counts is a contiguous int32 [{N}]")
    row_base = torch.empty(N, H, dtype=torch.int32, device=dev)
    _hip.call("iseg_ccl_label", ptr(mask), int(mask.dtype != torch.int32), N, H, W, ptr(labels), ptr(counts), ptr(row_base), stream())
    return labels, counts


def upsample_ce_supported(Hi, Wi, Ho, Wo, Cc):
    return bool(_hip.lib().iseg_upsample_ce_supported(int(Hi), int(Wi), int(Ho), int(Wo), int(Cc)))


def upsample_ce(z, labels, Ho, Wo, ignore_label, *, class_w=None, sum_scale=1.0, want_grad=True, grad_scale=1.0, cm=None):
    """fused logits tail (csrc/loss.hip): bilinear upsample of z [N,Hi,Wi,C] to [Ho,Wo] + ignore-label CE sum + d(sum)/dz + confusion
    matrix, without the full-resolution logits.  returns (loss_sum [1] fp32, dz like z or None)"""
    _require_cuda(z, labels)
    N, Hi, Wi, Cc = z.shape
    loss_sum = torch.empty(1, dtype=torch.float32, device=z.device)
    dz = torch.empty_like(z) if want_grad else None
    ws, wsb = workspace(_hip.lib().iseg_upsample_ce_workspace_bytes(N, Hi, Wi, Ho, Wo, Cc), z.device)
    _hip.call("iseg_upsample_ce", ptr(z), dt(z), ptr(labels), ptr(class_w), N, Hi, Wi, Ho, Wo, Cc, ignore_label, ptr(loss_sum), sum_scale,
              ptr(dz), grad_scale, ptr(cm), ptr(ws), wsb, stream())
    return loss_sum, dz


def argmax_confusion(logits2d, labels1d, ignore_label, cm=None, want_pred=False):
    P, Cc = logits2d.shape
    pred = torch.empty(P, dtype=torch.int32, device=logits2d.device) if want_pred else None
    _hip.call("iseg_argmax_confusion", ptr(logits2d), ptr(labels1d), P, Cc, ignore_label, ptr(pred), ptr(cm), stream())
    return pred


CM_W_NONE, CM_W_U8, CM_W_F32 = 0, 1, 2
CM_SLICE, CM_GRID_CAP, CM_F32_MAX_N = 4096, 1024, 1 << 24      # ISEG_CM_SLICE, ISEG_CM_GRID_CAP, ISEG_CM_F32_MAX_N of the header
CM_COUNTERS = 8


def confusion_supported(Cc, wmode):
    return bool(_hip.lib().iseg_confusion_supported(int(Cc), int(wmode)))


def confusion_weight_exponent(max_abs):
    """w_exp of iseg_confusion_batched for fp32 weights whose largest magnitude is max_abs (finite, >= 0): 38 - ex with max_abs = m * 2^ex,
    m in [0.5, 1), so that max_abs * 2^w_exp lies in [2^37, 2^38); 0 when every weight is 0"""
    import math

    max_abs = float(max_abs)
    if not math.isfinite(max_abs) or max_abs < 0:
        raise ValueError(f"confusion_weight_exponent: a finite, non-negative maximum, got {max_abs}")
    return 38 - math.frexp(max_abs)[1] if max_abs else 0


def confusion_absmax(weights):
    """max |w| of a contiguous fp32 tensor (csrc/confusion.hip: an integer maximum over the bit patterns, exact and order-independent) as a
    Python float: inf or nan when a weight is not finite.  Reads four bytes back: a host synchronisation."""
    import struct

    _require_cuda(weights)
    if weights.dtype != torch.float32 or not weights.is_contiguous():
        raise TypeError("confusion_absmax: a contiguous float32 tensor")
    if weights.numel() == 0:
        return 0.0
    bits = torch.empty(1, dtype=torch.int32, device=weights.device)
    _hip.call("iseg_confusion_absmax_f32", ptr(weights), weights.numel(), ptr(bits), stream())
    return struct.unpack("<f", struct.pack("<I", int(bits.item()) & 0xFFFFFFFF))[0]


def confusion_batched(labels, preds, Cc, *, weights=None, w_exp=0, ignore_label=None, cm=None, accumulate=False, counters=None):
    """iseg_confusion_batched (csrc/confusion.hip): labels, preds [B, n] int32 maps; weights None, [B, n] uint8 / bool (each element adds its
    byte) or [B, n] float32 (each adds llrint(w * 2^w_exp)); ignore_label None or the label that is skipped without a look at the rest.
    cm [B, C, C] int64 (any shape of B*C*C elements; made here when None), cleared first unless accumulate; counters [8] int64, added to (zeros
    when None): labels < 0, predictions < 0, labels >= C, predictions >= C, weights not finite or out of range, weights that were rounded.
    Nothing is read back.  returns (cm, counters)"""
    if labels.dim() != 2 or labels.shape != preds.shape:
        raise ValueError(f"confusion_batched: labels and preds are [B, n] of one shape, got {tuple(labels.shape)} and {tuple(preds.shape)}")
    _require_cuda(labels, preds, weights, cm, counters)
    if labels.dtype != torch.int32 or preds.dtype != torch.int32 or not (labels.is_contiguous() and preds.is_contiguous()):
        raise TypeError("confusion_batched: contiguous int32 labels and preds")
    B, n = labels.shape
    wmode = CM_W_NONE
    if weights is not None:
        if weights.shape != labels.shape or not weights.is_contiguous():
            raise ValueError(f"confusion_batched: weights are contiguous and of the labels' shape, got {tuple(weights.shape)}")
        if weights.dtype in (torch.uint8, torch.bool):
            wmode = CM_W_U8
        elif weights.dtype == torch.float32:
            wmode = CM_W_F32
        else:
            raise TypeError(f"confusion_batched: weights are uint8, bool or float32, got {weights.dtype}")
    dev = labels.device
    if cm is None:
        cm = torch.empty(B, Cc, Cc, dtype=torch.int64, device=dev)
        accumulate = False
    elif cm.dtype != torch.int64 or cm.numel() != B * Cc * Cc or not cm.is_contiguous():
        raise ValueError(f"confusion_batched: cm is a contiguous int64 tensor of {B} x {Cc} x {Cc} elements")
    if counters is None:
        counters = torch.zeros(CM_COUNTERS, dtype=torch.int64, device=dev)
    elif counters.dtype != torch.int64 or counters.numel() != CM_COUNTERS or not counters.is_contiguous():
        raise ValueError(f"confusion_batched: counters is a contiguous int64 [{CM_COUNTERS}]")
    _hip.call("iseg_confusion_batched", ptr(labels), ptr(preds), ptr(weights), wmode, int(w_exp), B, n, int(Cc), int(ignore_label is not None),
              int(ignore_label or 0), ptr(cm), int(bool(accumulate)), ptr(counters), stream())
    return cm, counters


# ---------------------------------------------------------------------------------------------------------
# replace_nan_or_inf, GroupNorm, RMSNorm, pooling (csrc/misc.hip)
# ---------------------------------------------------------------------------------------------------------
def replace_nan_or_inf(x, nan_value=0.0):
    _require_cuda(x)
    y = torch.empty_like(x)
    ws, wsb = workspace(8, x.device)
    _hip.check(_hip.lib().iseg_replace_nan_or_inf(ptr(x), ptr(y), x.numel(), float(nan_value), dt(x), ptr(ws), wsb, stream()),
               "iseg_replace_nan_or_inf")
    return y


def replace_nan_or_inf_bwd(x, dy):
    _require_cuda(x, dy)
    dx = torch.empty_like(dy)
    _hip.check(_hip.lib().iseg_replace_nan_or_inf_bwd(ptr(x), ptr(dy), ptr(dx), x.numel(), dt(x), stream()), "iseg_replace_nan_or_inf_bwd")
    return dx


def groupnorm_fwd(x3d, gamma, beta, groups, eps):
    """x3d [N, HW, C] contiguous -> y, mean [N*G], rstd [N*G]"""
    _require_cuda(x3d)
    N, HW, Cc = x3d.shape
    y = torch.empty_like(x3d)
    mean = torch.empty(N * groups, dtype=torch.float32, device=x3d.device)
    rstd = torch.empty_like(mean)
    _hip.check(_hip.lib().iseg_groupnorm_fwd(ptr(x3d), ptr(gamma), ptr(beta), ptr(y), ptr(mean), ptr(rstd), N, HW, Cc, groups, float(eps),
                                            dt(x3d), stream()), "iseg_groupnorm_fwd")
    return y, mean, rstd


def groupnorm_bwd(dy3d, x3d, gamma, mean, rstd, groups, dgamma, dbeta, accumulate=True):
    _require_cuda(dy3d, x3d)
    N, HW, Cc = x3d.shape
    dx = torch.empty_like(x3d)
    L = _hip.lib()
    ws, wsb = workspace(L.iseg_groupnorm_bwd_workspace_bytes(N, Cc), x3d.device)
    _hip.check(L.iseg_groupnorm_bwd(ptr(dy3d), ptr(x3d), ptr(gamma), ptr(mean), ptr(rstd), ptr(dx), ptr(dgamma), ptr(dbeta), int(accumulate),
                                    N, HW, Cc, groups, dt(x3d), ptr(ws), wsb, stream()), "iseg_groupnorm_bwd")
    return dx


def rmsnorm_fwd(x2d, scale, eps):
    _require_cuda(x2d)
    rows, Cc = x2d.shape
    y = torch.empty_like(x2d)
    rstd = torch.empty(rows, dtype=torch.float32, device=x2d.device)
    _hip.check(_hip.lib().iseg_rmsnorm_fwd(ptr(x2d), ptr(scale), ptr(y), ptr(rstd), rows, Cc, float(eps), dt(x2d), stream()), "iseg_rmsnorm_fwd")
    return y, rstd


def rmsnorm_bwd(dy2d, x2d, scale, rstd, dscale, accumulate=True):
    _require_cuda(dy2d, x2d)
    rows, Cc = x2d.shape
    dx = torch.empty_like(x2d)
    L = _hip.lib()
    ws, wsb = workspace(L.iseg_rmsnorm_bwd_workspace_bytes(rows, Cc), x2d.device)
    _hip.check(L.iseg_rmsnorm_bwd(ptr(dy2d), ptr(x2d), ptr(scale), ptr(rstd), ptr(dx), ptr(dscale), int(accumulate), rows, Cc, dt(x2d),
                                  ptr(ws), wsb, stream()), "iseg_rmsnorm_bwd")
    return dx


def grn_fwd(x3d, gamma, beta, eps):
    """Global Response Normalization (backbones/convnext_v2.py:45-60) on [N, HW, C]: returns y and the per-(sample, channel) nx, gx"""
    _require_cuda(x3d, gamma, beta)
    N, HW, Cc = x3d.shape
    y = torch.empty_like(x3d)
    nx = torch.empty(N, Cc, dtype=torch.float32, device=x3d.device)
    gx = torch.empty_like(nx)
    L = _hip.lib()
    ws, wsb = workspace(L.iseg_grn_workspace_bytes(N, HW, Cc), x3d.device)
    _hip.check(L.iseg_grn_fwd(ptr(x3d), ptr(gamma), ptr(beta), ptr(y), ptr(nx), ptr(gx), N, HW, Cc, float(eps), dt(x3d), ptr(ws), wsb,
                              stream()), "iseg_grn_fwd")
    return y, nx, gx


def grn_bwd(dy3d, x3d, gamma, nx, gx, dgamma, dbeta, eps, accumulate=True, mul=None):
    """dx [* mul] and (+)= dgamma, dbeta; `mul`: saved activation derivative folded into the data gradient (see include/iseg_hip.h)"""
    _require_cuda(dy3d, x3d, dgamma, dbeta)
    if mul is not None and (mul.dtype != x3d.dtype or mul.numel() != x3d.numel() or not mul.is_contiguous()):
        raise ValueError("grn_bwd: mul must be a contiguous tensor shaped and typed like x")
    N, HW, Cc = x3d.shape
    dx = torch.empty_like(x3d)
    L = _hip.lib()
    ws, wsb = workspace(L.iseg_grn_workspace_bytes(N, HW, Cc), x3d.device)
    _hip.check(L.iseg_grn_bwd(ptr(dy3d), ptr(x3d), ptr(gamma), ptr(nx), ptr(gx), ptr(mul), ptr(dx), ptr(dgamma), ptr(dbeta), int(accumulate), N, HW, Cc,
                              float(eps), dt(x3d), ptr(ws), wsb, stream()), "iseg_grn_bwd")
    return dx


def grn_stats(x3d, eps):
    """nx, gx of grn_fwd without writing the normalised tensor (the caller folds gamma*nx + 1 into the next kernel)"""
    _require_cuda(x3d)
    N, HW, Cc = x3d.shape
    nx = torch.empty(N, Cc, dtype=torch.float32, device=x3d.device)
    gx = torch.empty_like(nx)
    L = _hip.lib()
    ws, wsb = workspace(L.iseg_grn_workspace_bytes(N, HW, Cc), x3d.device)
    _hip.check(L.iseg_grn_fwd(ptr(x3d), None, None, None, ptr(nx), ptr(gx), N, HW, Cc, float(eps), dt(x3d), ptr(ws), wsb, stream()), "iseg_grn_fwd")
    return nx, gx


def grn_fold_weights(wt, gamma, nx):
    """[N, Cout, C4] bf16: the K-contiguous kernel copy wt [Cout, C4] times (gamma*nx_n + 1) per sample"""
    _require_cuda(wt, gamma, nx)
    Cout, C4 = wt.shape
    N = nx.shape[0]
    out = torch.empty((N, Cout, C4), dtype=wt.dtype, device=wt.device)
    _hip.call("iseg_grn_fold_weights", ptr(wt), ptr(gamma), ptr(nx), ptr(out), N, Cout, C4, stream())
    return out


def grn_fold_bias(W, beta, b):
    """b + beta @ W for the fp32 kernel W [C4, Cout]"""
    _require_cuda(W, beta)
    C4, Cout = W.shape
    out = torch.empty(Cout, dtype=torch.float32, device=W.device)
    _hip.call("iseg_grn_fold_bias", ptr(W), ptr(beta), ptr(b), ptr(out), C4, Cout, stream())
    return out


def grn_fold_wgrad(slabs, slabs_per_sample, W, gamma, beta, nx, S, dW, accumulate=True):
    """dW (+)= sum_n (gamma*nx_n + 1) (.) G_n + beta (x) S from the per-chunk products slabs [N*sps, C4, Cout]; returns dstats [N, 2*C4]"""
    _require_cuda(slabs, W, dW)
    C4, Cout = W.shape
    N = nx.shape[0]
    dstats = torch.empty((N, 2 * C4), dtype=torch.float32, device=W.device)
    _hip.call("iseg_grn_fold_wgrad", ptr(slabs), int(slabs_per_sample), ptr(W), ptr(gamma), ptr(beta), ptr(nx), ptr(S), ptr(dW), ptr(dstats),
              int(accumulate), N, C4, Cout, stream())
    return dstats


def grn_bwd_folded(dy3d, x3d, gamma, nx, gx, dstats, dgamma, dbeta, eps, accumulate=True, mul=None):
    """grn_bwd with the per-sample statistics given (dstats from grn_fold_wgrad; overwritten)"""
    _require_cuda(dy3d, x3d, dstats, dgamma, dbeta)
    N, HW, Cc = x3d.shape
    if mul is not None and (mul.dtype != x3d.dtype or mul.numel() != x3d.numel() or not mul.is_contiguous()):
        raise ValueError("grn_bwd_folded: mul must be a contiguous tensor shaped and typed like x")
    dx = torch.empty_like(x3d)
    L = _hip.lib()
    ws, wsb = workspace(L.iseg_grn_workspace_bytes(N, HW, Cc), x3d.device)
    _hip.check(L.iseg_grn_bwd_folded(ptr(dy3d), ptr(x3d), ptr(gamma), ptr(nx), ptr(gx), ptr(mul), ptr(dstats), ptr(dx), ptr(dgamma), ptr(dbeta),
                                     int(accumulate), N, HW, Cc, float(eps), dt(x3d), ptr(ws), wsb, stream()), "iseg_grn_bwd_folded")
    return dx


POOL_MAX, POOL_AVG = 0, 1


def pool2d_fwd(x, kh, kw, sh, sw, pt, pl, Ho, Wo, mode):
    _require_cuda(x)
    N, H, W, Cc = x.shape
    y = torch.empty((N, Ho, Wo, Cc), dtype=x.dtype, device=x.device)
    _hip.check(_hip.lib().iseg_pool2d_fwd(ptr(x), ptr(y), N, H, W, Cc, kh, kw, sh, sw, pt, pl, Ho, Wo, mode, dt(x), stream()), "iseg_pool2d_fwd")
    return y


def pool2d_bwd(x, dy, kh, kw, sh, sw, pt, pl, mode):
    _require_cuda(x, dy)
    N, H, W, Cc = x.shape
    Ho, Wo = dy.shape[1], dy.shape[2]
    dx = torch.empty_like(x)
    L = _hip.lib()
    ws, wsb = workspace(L.iseg_pool2d_bwd_workspace_bytes(N, Ho, Wo, Cc, mode), x.device)
    _hip.check(L.iseg_pool2d_bwd(ptr(x), ptr(dy), ptr(dx), N, H, W, Cc, kh, kw, sh, sw, pt, pl, Ho, Wo, mode, dt(x), ptr(ws), wsb,
                                 stream()), "iseg_pool2d_bwd")
    return dx


def add_relu(a, b):
    _require_cuda(a, b)
    y = torch.empty_like(a)
    _hip.check(_hip.lib().iseg_add_relu(ptr(a), ptr(b), ptr(y), a.numel(), dt(a), stream()), "iseg_add_relu")
    return y


# ---------------------------------------------------------------------------------------------------------
# attention pieces (csrc/attention.hip) around the strided-batch GEMMs
# ---------------------------------------------------------------------------------------------------------
def softmax_rows_fwd(scores, problems, Tq, cols, ld, *, bias=None, heads=1, mask=None, windows=1, clip=None, out=None):
    _require_cuda(scores)
    out = scores if out is None else out
    lo, hi = clip if clip is not None else (0.0, 0.0)
    _hip.check(_hip.lib().iseg_softmax_rows_fwd(ptr(scores), ptr(out), problems, Tq, cols, ld, ptr(bias), heads, ptr(mask), windows,
                                               float(lo), float(hi), dt(scores), stream()), "iseg_softmax_rows_fwd")
    return out


def softmax_rows_bwd(probs, dprobs, rows, cols, ld, *, clip=None, out=None):
    _require_cuda(probs, dprobs)
    out = dprobs if out is None else out
    lo, hi = clip if clip is not None else (0.0, 0.0)
    _hip.check(_hip.lib().iseg_softmax_rows_bwd(ptr(probs), ptr(dprobs), ptr(out), rows, cols, ld, float(lo), float(hi), dt(probs),
                                               stream()), "iseg_softmax_rows_bwd")
    return out


def clip_fwd(x, lo, hi):
    _require_cuda(x)
    y = torch.empty_like(x)
    _hip.check(_hip.lib().iseg_clip_fwd(ptr(x), ptr(y), x.numel(), float(lo), float(hi), dt(x), stream()), "iseg_clip_fwd")
    return y


def clip_bwd(x, dy, lo, hi):
    _require_cuda(x, dy)
    dx = torch.empty_like(dy)
    _hip.check(_hip.lib().iseg_clip_bwd(ptr(x), ptr(dy), ptr(dx), x.numel(), float(lo), float(hi), dt(x), stream()), "iseg_clip_bwd")
    return dx


def gather_rows(x2d, idx, rows_out):
    """y[r] = x2d[idx[r]] (idx int32 on device, -1 -> zero row)"""
    _require_cuda(x2d, idx)
    if idx.dtype != torch.int32 or idx.numel() != rows_out:
        raise TypeError("gather_rows: idx must be int32 with one entry per output row")
    rows_in, Cc = x2d.shape
    y = torch.empty((rows_out, Cc), dtype=x2d.dtype, device=x2d.device)
    _hip.check(_hip.lib().iseg_gather_rows(ptr(x2d), ptr(idx), ptr(y), rows_in, rows_out, Cc, dt(x2d), stream()), "iseg_gather_rows")
    return y


def relpos_bias_gather(table, index, heads, T):
    _require_cuda(table, index)
    bias = torch.empty((heads, T, T), dtype=torch.float32, device=table.device)
    _hip.check(_hip.lib().iseg_relpos_bias_gather(ptr(table), ptr(index), ptr(bias), heads, T * T, stream()), "iseg_relpos_bias_gather")
    return bias


def relpos_bias_scatter_grad(dbias, ld, index, dtable, heads, T, accumulate=True, window=0):
    """window = ws > 0 asserts that `index` is the canonical ws x ws table (backbones/swin.py:93-104): fast kernel"""
    _require_cuda(dbias, index, dtable)
    if window > 0 and window * window == T and dtable.shape[0] == (2 * window - 1) ** 2:
        _hip.check(_hip.lib().iseg_relpos_bias_scatter_grad_window(ptr(dbias), ld, ptr(dtable), window, heads, int(accumulate), stream()),
                   "iseg_relpos_bias_scatter_grad_window")
        return dtable
    _hip.check(_hip.lib().iseg_relpos_bias_scatter_grad(ptr(dbias), ld, ptr(index), ptr(dtable), dtable.shape[0], heads, T, int(accumulate),
                                                       stream()), "iseg_relpos_bias_scatter_grad")
    return dtable


# ---------------------------------------------------------------------------------------------------------
# DCNv3 core + per-channel scale gradient (csrc/dcnv3.hip)
# ---------------------------------------------------------------------------------------------------------
def dcnv3_out_hw(H, W, kh, kw, stride, dil, pad):
    return (H + 2 * pad - (dil * (kh - 1) + 1)) // stride + 1, (W + 2 * pad - (dil * (kw - 1) + 1)) // stride + 1


def dcnv3_fwd(x, offset, mask, G, Cg, kh, kw, stride, dil, pad, offset_scale):
    _require_cuda(x, offset, mask)
    N, H, W, Cc = x.shape
    Ho, Wo = dcnv3_out_hw(H, W, kh, kw, stride, dil, pad)
    if Cc != G * Cg or tuple(offset.shape) != (N, Ho, Wo, G * kh * kw * 2) or tuple(mask.shape) != (N, Ho, Wo, G * kh * kw):
        raise ValueError(f"dcnv3_fwd: shapes x {tuple(x.shape)} offset {tuple(offset.shape)} mask {tuple(mask.shape)} do not match "
                         f"G={G} Cg={Cg} k={kh}x{kw} -> {Ho}x{Wo}")
    y = torch.empty((N, Ho, Wo, Cc), dtype=x.dtype, device=x.device)
    _hip.check(_hip.lib().iseg_dcnv3_fwd(ptr(x), ptr(offset), ptr(mask), ptr(y), N, H, W, G, Cg, kh, kw, stride, dil, pad,
                                        float(offset_scale), dt(x), stream()), "iseg_dcnv3_fwd")
    return y


def dcnv3_bwd(x, offset, mask, dy, G, Cg, kh, kw, stride, dil, pad, offset_scale):
    _require_cuda(x, offset, mask, dy)
    N, H, W, Cc = x.shape
    Ho, Wo = dcnv3_out_hw(H, W, kh, kw, stride, dil, pad)
    if tuple(dy.shape) != (N, Ho, Wo, Cc) or Cc != G * Cg:
        raise ValueError("dcnv3_bwd: dy shape does not match the forward geometry")
    dx = torch.empty((N, H, W, Cc), dtype=torch.float32, device=x.device)
    doff = torch.empty_like(offset)
    dmask = torch.empty_like(mask)
    L = _hip.lib()
    ws, wsb = workspace(L.iseg_dcnv3_bwd_workspace_bytes(N, H, W, G, Cg, kh, kw, stride, dil, pad, float(offset_scale)), x.device)
    _hip.check(L.iseg_dcnv3_bwd(ptr(x), ptr(offset), ptr(mask), ptr(dy), ptr(dx), ptr(doff), ptr(dmask), N, H, W, G, Cg, kh, kw,
                                stride, dil, pad, float(offset_scale), dt(x), ptr(ws), wsb, stream()), "iseg_dcnv3_bwd")
    return dx, doff, dmask


# ---------------------------------------------------------------------------------------------------------
# Deformable multi-head self-attention core (csrc/defattn.hip; layers/deformable_multihead_self_attention.py:89-244)
# ---------------------------------------------------------------------------------------------------------
def _defattn_geom(value, offset_logits, attn_logits, heads, points, who):
    N, H, W, Cv = value.shape
    if heads < 1 or points < 1 or Cv % heads != 0 or tuple(offset_logits.shape) != (N, H, W, heads * points * 2) or \
            tuple(attn_logits.shape) != (N, H, W, heads * points):
        raise ValueError(f"{who}: shapes value {tuple(value.shape)} offset logits {tuple(offset_logits.shape)} attention logits "
                         f"{tuple(attn_logits.shape)} do not match heads={heads} points={points}")
    if not (value.dtype == offset_logits.dtype == attn_logits.dtype):
        raise TypeError(f"{who}: value, offset logits and attention logits must share one storage dtype")
    return N, H, W, Cv // heads


def defattn_fwd(value, offset_logits, attn_logits, heads, points, offset_range_factor):
    """value [N,H,W,heads*Ch], raw offset logits [N,H,W,heads*P*2], raw attention logits [N,H,W,heads*P] -> out [N,H,W,heads*Ch]"""
    _require_cuda(value, offset_logits, attn_logits)
    N, H, W, Ch = _defattn_geom(value, offset_logits, attn_logits, heads, points, "defattn_fwd")
    out = torch.empty_like(value)
    _hip.call("iseg_defattn_fwd", ptr(value), ptr(offset_logits), ptr(attn_logits), ptr(out), N, H, W, heads, points, Ch,
              float(offset_range_factor), dt(value), stream())
    return out


def defattn_bwd(value, offset_logits, attn_logits, dout, heads, points, offset_range_factor):
    """-> dvalue, doffset_logits, dattn_logits in the storage dtype (dvalue through int64 fixed-point atomics: bit-identical from run to run)"""
    _require_cuda(value, offset_logits, attn_logits, dout)
    N, H, W, Ch = _defattn_geom(value, offset_logits, attn_logits, heads, points, "defattn_bwd")
    if tuple(dout.shape) != tuple(value.shape) or dout.dtype != value.dtype:
        raise ValueError("defattn_bwd: dout does not match value")
    dvalue, doff, dattn = torch.empty_like(value), torch.empty_like(offset_logits), torch.empty_like(attn_logits)
    ws, wsb = workspace(_hip.lib().iseg_defattn_bwd_workspace_bytes(N, H, W, heads, Ch), value.device)
    _hip.call("iseg_defattn_bwd", ptr(value), ptr(offset_logits), ptr(attn_logits), ptr(dout), ptr(dvalue), ptr(doff), ptr(dattn), N, H, W, heads,
              points, Ch, float(offset_range_factor), dt(value), ptr(ws), wsb, stream())
    return dvalue, doff, dattn


def dcnv3_fwd_joint(x, om, G, Cg, kh, kw, stride, dil, pad, offset_scale):
    """dcnv3_fwd with the offsets and the (soft-maxed) mask as column ranges [0, 2GP) and [2GP, 3GP) of ONE matrix om [pixels, ld]"""
    _require_cuda(x, om)
    N, H, W, Cc = x.shape
    Ho, Wo = dcnv3_out_hw(H, W, kh, kw, stride, dil, pad)
    gp = G * kh * kw
    if Cc != G * Cg or om.dim() != 2 or om.shape[0] != N * Ho * Wo or om.shape[1] < 3 * gp or om.stride(1) != 1:
        raise ValueError(f"dcnv3_fwd_joint: x {tuple(x.shape)} / om {tuple(om.shape)} do not match G={G} Cg={Cg} k={kh}x{kw} -> {Ho}x{Wo}")
    y = torch.empty((N, Ho, Wo, Cc), dtype=x.dtype, device=x.device)
    ld = om.stride(0)
    _hip.check(_hip.lib().iseg_dcnv3_fwd_ld(ptr(x), ptr(om), ptr(om[:, 2 * gp:]), ld, ld, ptr(y), N, H, W, G, Cg, kh, kw, stride, dil, pad,
                                           float(offset_scale), dt(x), stream()), "iseg_dcnv3_fwd_ld")
    return y


def dcnv3_bwd_joint(x, om, dy, G, Cg, kh, kw, stride, dil, pad, offset_scale):
    """-> (dx fp32, dom [pixels, ld]): the offset / mask gradients in om's layout; the columns behind 3GP are NOT written (dcn_mask_softmax_bwd
    clears them)"""
    _require_cuda(x, om, dy)
    N, H, W, Cc = x.shape
    Ho, Wo = dcnv3_out_hw(H, W, kh, kw, stride, dil, pad)
    if tuple(dy.shape) != (N, Ho, Wo, Cc) or Cc != G * Cg:
        raise ValueError("dcnv3_bwd_joint: dy shape does not match the forward geometry")
    gp = G * kh * kw
    if om.dim() != 2 or om.shape[0] != N * Ho * Wo or om.shape[1] < 3 * gp or om.stride(1) != 1:
        raise ValueError(f"dcnv3_bwd_joint: om {tuple(om.shape)} does not match {N * Ho * Wo} output pixels x >= {3 * gp} columns")
    dx = torch.empty((N, H, W, Cc), dtype=x.dtype, device=x.device)
    # the C ABI takes ONE pitch pair for om and dom, so dom is allocated AT om's row pitch: empty_like(om) of a column-sliced om (shape[1] < stride)
    # keeps om's shape but comes back dense, i.e. with a different pitch than the om.stride(0) that was passed for it (round-5 advisor)
    ld = om.stride(0)
    dom = torch.empty((om.shape[0], ld), dtype=om.dtype, device=om.device)[:, :om.shape[1]]
    L = _hip.lib()
    ws, wsb = workspace(L.iseg_dcnv3_bwd_workspace_bytes(N, H, W, G, Cg, kh, kw, stride, dil, pad, float(offset_scale)), x.device)
    side = _dcn_side(L.iseg_dcnv3_bwd_side_bytes(N, H, W, G, Cg, kh, kw, stride, dil, pad, float(offset_scale)), x.device)
    _dcn_side_guard(x.device, True)
    _hip.check(L.iseg_dcnv3_bwd_ld(ptr(x), ptr(om), ptr(om[:, 2 * gp:]), ld, ld, ptr(dy), ptr(dx), dt(dx), ptr(dom), ptr(dom[:, 2 * gp:]), N, H, W, G,
                                   Cg, kh, kw, stride, dil, pad, float(offset_scale), dt(x), ptr(ws), wsb, ptr(side),
                                   side.numel() if side is not None else 0, stream()), "iseg_dcnv3_bwd_ld")
    _dcn_side_guard(x.device, False)
    return dx, dom


# The kept side buffer of the DCNv3 backward (iseg_dcnv3_bwd_ld): zero-filled once when it is (re)allocated, left all zero by every call.  One per
# device, grown to the largest geometry seen; a growth re-homes it, which a captured graph must notice (nn.buffers_generation).
_DCN_SIDE = {}


_DCN_SIDE_DIRTY = set()      # devices whose side buffer a backward call may have left non-zero


def _dcn_side_guard(device, entering):
    """Host-side dirty bit around every call that uses the side buffer (round-5 advisor): set before the launch, cleared once the call has
    returned without an error.  A call that raises in between (a launch error surfacing there, KeyboardInterrupt, a failed graph capture that is
    retried) leaves it set, and the NEXT request for the buffer zero-fills it again instead of feeding stale fixed-point partials or a set poison
    flag into every later input gradient of every DCNv3 layer."""
    key = str(device)
    if entering:
        _DCN_SIDE_DIRTY.add(key)
    else:
        _DCN_SIDE_DIRTY.discard(key)


def _dcn_side(nbytes, device):
    if nbytes == 0:
        return None
    key = str(device)
    buf = _DCN_SIDE.get(key)
    if buf is not None and key in _DCN_SIDE_DIRTY:      # a call that used it did not finish: restore the all-zero invariant
        fill_f32(buf.view(torch.float32), 0.0)
        _DCN_SIDE_DIRTY.discard(key)
    if buf is None or buf.numel() < nbytes:
        from . import nn

        buf = torch.empty((nbytes + 3) // 4 * 4, dtype=torch.uint8, device=device)
        fill_f32(buf.view(torch.float32), 0.0)
        _DCN_SIDE[key] = buf
        nn.bump_buffers_generation()
    return buf


def dcn_mask_softmax_fwd(om, G, P):
    """softmax over each (pixel, group)'s P mask logits, in place on columns [2GP, 3GP) of om [pixels, ld]"""
    _hip.call("iseg_dcn_mask_softmax_fwd", ptr(om), om.shape[0], G, P, om.stride(0), 2 * G * P, dt(om), stream())
    return om


def dcn_mask_softmax_bwd(om, dom, G, P):
    """in place on dom: the softmax backward on the mask columns, zeros in the padding columns behind 3GP"""
    _hip.call("iseg_dcn_mask_softmax_bwd", ptr(om), ptr(dom), om.shape[0], G, P, om.stride(0), 2 * G * P, dt(om), stream())
    return dom


def split_cols_accumulate(src, dst0, n0, dst1, n1):
    """dst0 [rows, n0] += src[:, :n0]; dst1 [rows, n1] += src[:, n0:n0 + n1]   (fp32; src [rows, ld]; None destinations are skipped)"""
    rows = src.shape[0] if src.dim() == 2 else 1
    ld = src.stride(0) if src.dim() == 2 else src.numel()
    _hip.call("iseg_split_cols_accumulate", ptr(src), rows, ld, ptr(dst0), int(n0), ptr(dst1), int(n1), stream())


def dcn_center_blend_fwd(x, x_proj, scale, G, Cg):
    """x (1 - s) + x_proj s, s [.., G] broadcast over each group's Cg channels"""
    _require_cuda(x, x_proj, scale)
    out = torch.empty_like(x)
    _hip.call("iseg_dcn_center_blend_fwd", ptr(x), ptr(x_proj), ptr(scale), ptr(out), x.numel() // (G * Cg), G, Cg, dt(x), stream())
    return out


def dcn_center_blend_bwd(dout, x, x_proj, scale, G, Cg):
    _require_cuda(dout, x, x_proj, scale)
    dx, dxp, ds = torch.empty_like(x), torch.empty_like(x_proj), torch.empty_like(scale)
    _hip.call("iseg_dcn_center_blend_bwd", ptr(dout), ptr(x), ptr(x_proj), ptr(scale), ptr(dx), ptr(dxp), ptr(ds), x.numel() // (G * Cg), G, Cg,
              dt(x), stream())
    return dx, dxp, ds


def mul_colsum(a2d, b2d, out, accumulate=True):
    _require_cuda(a2d, b2d, out)
    rows, Cc = a2d.shape
    L = _hip.lib()
    ws, wsb = workspace(L.iseg_mul_colsum_workspace_bytes(rows, Cc), a2d.device)
    _hip.check(L.iseg_mul_colsum(ptr(a2d), ptr(b2d), rows, Cc, ptr(out), int(accumulate), dt(a2d), ptr(ws), wsb, stream()), "iseg_mul_colsum")
    return out


def scale_cols(x2d, colscale):
    _require_cuda(x2d, colscale)
    rows, Cc = x2d.shape
    y = torch.empty_like(x2d)
    _hip.check(_hip.lib().iseg_scale_cols(ptr(x2d), ptr(colscale), ptr(y), rows, Cc, dt(x2d), stream()), "iseg_scale_cols")
    return y


def colsum_wide(x2d, out, accumulate=False):
    """out[c] (+)= sum_r x2d[r, c] for few rows and very many columns"""
    _require_cuda(x2d, out)
    rows, cols = x2d.shape
    L = _hip.lib()
    ws, wsb = workspace(L.iseg_colsum_wide_workspace_bytes(rows, cols), x2d.device)
    _hip.check(L.iseg_colsum_wide(ptr(x2d), x2d.stride(0), rows, cols, ptr(out), int(accumulate), dt(x2d), ptr(ws), wsb, stream()),
               "iseg_colsum_wide")
    return out


# ---------------------------------------------------------------------------------------------------------
# fused global attention on packed [q|k|v], head_dim 64 (csrc/flashattn.hip)
# ---------------------------------------------------------------------------------------------------------
def attention_fwd_supported(head_dim, dtype):
    return dtype == torch.bfloat16 and bool(_hip.lib().iseg_attention_fwd_supported(int(head_dim), BF16))


def attention_fwd(qkv, heads, scale):
    """forward-only global attention on packed [q|k|v] (inference): [B, T, 3C] -> [B, T, C]"""
    B, T, ld = qkv.shape
    C = ld // 3
    out = torch.empty((B, T, C), dtype=qkv.dtype, device=qkv.device)
    _hip.check(_hip.lib().iseg_attention_fwd(ptr(qkv), ptr(out), B, T, heads, C // heads, float(scale), dt(qkv), stream()),
               "iseg_attention_fwd")
    return out


def attention_fwd_train(qkv, heads, scale):
    """attention_fwd that also returns the per-row log2-sum-exp vector the backward kernels recompute the probabilities from"""
    B, T, ld = qkv.shape
    C = ld // 3
    L = _hip.lib()
    out = torch.empty((B, T, C), dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty(int(L.iseg_attention_lse_elems(B, T, heads)), dtype=torch.float32, device=qkv.device)
    _hip.check(L.iseg_attention_fwd_train(ptr(qkv), ptr(out), ptr(lse), B, T, heads, C // heads, float(scale), dt(qkv), stream()),
               "iseg_attention_fwd_train")
    return out, lse


def attention_bwd(qkv, out, dout, lse, heads, scale):
    B, T, ld = qkv.shape
    C = ld // 3
    L = _hip.lib()
    dqkv = torch.empty_like(qkv)
    ws, wsb = workspace(L.iseg_attention_bwd_workspace_bytes(B, T, heads), qkv.device)
    _hip.check(L.iseg_attention_bwd(ptr(qkv), ptr(out), ptr(dout), ptr(lse), ptr(dqkv), B, T, heads, C // heads, float(scale), dt(qkv),
                                    ptr(ws), wsb, stream()), "iseg_attention_bwd")
    return dqkv


# ---------------------------------------------------------------------------------------------------------
# single-head attention with a 64-wide key and a wide value (csrc/selfattn.hip)
# ---------------------------------------------------------------------------------------------------------
def self_attention_supported(dk, dv, dtype):
    return dtype == torch.bfloat16 and bool(_hip.lib().iseg_self_attention_supported(int(dk), int(dv), BF16))


def _pitched(t):
    """[B, T, C] as (tensor, row pitch in elements) without a copy when its rows are equally spaced across samples (a column range of a
    packed projection output), the pitch is a multiple of 8 elements and the base 16-byte aligned; else through a contiguous copy"""
    B, T, C = t.shape
    ld = t.stride(1)
    if t.stride(2) == 1 and ld >= C and ld % 8 == 0 and (B == 1 or t.stride(0) == T * ld) and t.data_ptr() % 16 == 0:
        return t, ld
    return t.contiguous(), C


def self_attention_fwd(q, k, v, scale, want_lse):
    """softmax(scale * q k^T) v for q, k [B, T, 64], v [B, T, dv]; want_lse: also the per-row log2-sum-exp vector of the backward kernels"""
    _require_cuda(q, k, v)
    B, T, dk = q.shape
    dv = v.shape[2]
    L = _hip.lib()
    (q, ldq), (k, ldk), (v, ldv) = _pitched(q), _pitched(k), _pitched(v)
    out = torch.empty((B, T, dv), dtype=v.dtype, device=v.device)
    lse = torch.empty(int(L.iseg_self_attention_lse_elems(B, T)), dtype=torch.float32, device=v.device) if want_lse else None
    _hip.check(L.iseg_self_attention_fwd(ptr(q), ldq, ptr(k), ldk, ptr(v), ldv, ptr(out), dv, ptr(lse), B, T, dk, dv, float(scale), dt(v),
                                         stream()), "iseg_self_attention_fwd")
    return out, lse


def self_attention_bwd(q, k, v, out, dout, lse, scale):
    """(dq, dk, dv) of self_attention_fwd; dq and dk are separate tensors also when q and k alias"""
    _require_cuda(q, k, v, out, dout, lse)
    B, T, dk = q.shape
    dv = v.shape[2]
    L = _hip.lib()
    (q, ldq), (k, ldk), (v, ldv), (out, ldo), (dout, lddo) = _pitched(q), _pitched(k), _pitched(v), _pitched(out), _pitched(dout)
    dq = torch.empty((B, T, dk), dtype=q.dtype, device=q.device)
    dkk = torch.empty((B, T, dk), dtype=q.dtype, device=q.device)
    dvv = torch.empty((B, T, dv), dtype=v.dtype, device=v.device)
    dsum = torch.empty(int(L.iseg_self_attention_lse_elems(B, T)), dtype=torch.float32, device=v.device)
    _hip.check(L.iseg_self_attention_bwd(ptr(q), ldq, ptr(k), ldk, ptr(v), ldv, ptr(out), ldo, ptr(dout), lddo, ptr(lse), ptr(dsum), ptr(dq), dk,
                                         ptr(dkk), dk, ptr(dvv), dv, B, T, dk, dv, float(scale), dt(v), stream()), "iseg_self_attention_bwd")
    return dq, dkk, dvv


# ---------------------------------------------------------------------------------------------------------
# fused window attention (csrc/winattn.hip)
# ---------------------------------------------------------------------------------------------------------
def window_attention_supported(T, head_dim, dtype):
    return dtype == torch.bfloat16 and bool(_hip.lib().iseg_window_attention_supported(int(T), int(head_dim), BF16))


def window_attention_table(bias, mask, heads, T):
    """[mask windows (1 without mask), heads, 64, 64] fp32 additive table: bias + mask inside T x T, -FLT_MAX outside"""
    _require_cuda(bias)
    nW = mask.shape[0] if mask is not None else 1
    table = torch.empty((nW, heads, 64, 64), dtype=torch.float32, device=bias.device)
    _hip.check(_hip.lib().iseg_window_attention_table(ptr(bias), ptr(mask), ptr(table), T, heads, nW, stream()), "iseg_window_attention_table")
    return table


def window_attention_fwd(qkv, table, heads, scale):
    _require_cuda(qkv, table)
    B, T, ld = qkv.shape
    out = torch.empty((B, T, ld // 3), dtype=qkv.dtype, device=qkv.device)
    _hip.check(_hip.lib().iseg_window_attention_fwd(ptr(qkv), ptr(table), ptr(out), B, T, heads, table.shape[0], float(scale), dt(qkv), stream()),
               "iseg_window_attention_fwd")
    return out


def window_attention_bwd(qkv, table, dout, heads, scale):
    _require_cuda(qkv, table, dout)
    B, T, ld = qkv.shape
    dqkv = torch.empty_like(qkv)
    dbias = torch.empty((heads, T, T), dtype=torch.float32, device=qkv.device)
    L = _hip.lib()
    ws, wsb = workspace(L.iseg_window_attention_bwd_workspace_bytes(B, T, heads), qkv.device)
    _hip.check(L.iseg_window_attention_bwd(ptr(qkv), ptr(table), ptr(dout), ptr(dqkv), ptr(dbias), B, T, heads, table.shape[0], float(scale),
                                           dt(qkv), ptr(ws), wsb, stream()), "iseg_window_attention_bwd")
    return dqkv, dbias


# ---------------------------------------------------------------------------------------------------------
# deferred parameter-gradient reductions (csrc/api.hip): one batched launch instead of ~70 five-microsecond ones per step
# ---------------------------------------------------------------------------------------------------------
_DEFER = {"arena": None, "active": False}


@contextlib.contextmanager
def deferred_reductions(flat_grad, arena_bytes=96 << 20):
    """Between enter and exit, the second stage of LayerNorm / depthwise / bias gradient reductions whose output lies in `flat_grad` (and
    accumulates into it) is queued inside the library and run by ONE launch per flush.  Exit flushes; call deferred_flush() before
    anything else reads the gradient buffer (all-reduce, clipping).  ISEG_DEFER_REDUCE=0 turns the service off."""
    import os

    if not flat_grad.is_cuda or os.environ.get("ISEG_DEFER_REDUCE", "1") == "0" or _DEFER["active"]:
        yield
        return
    arena = _DEFER["arena"]
    if arena is None or arena.device != flat_grad.device or arena.numel() < arena_bytes:
        arena = _DEFER["arena"] = torch.empty(arena_bytes, dtype=torch.uint8, device=flat_grad.device)
    _hip.call("iseg_deferred_begin", ptr(flat_grad), flat_grad.numel() * flat_grad.element_size(), ptr(arena), arena.numel(), stream())
    _DEFER["active"] = True
    try:
        yield
    finally:
        _DEFER["active"] = False
        _hip.call("iseg_deferred_end", stream())


def deferred_flush():
    if _DEFER["active"]:
        _hip.call("iseg_deferred_flush", stream())


# ---------------------------------------------------------------------------------------------------------
# Gemma text backbone (csrc/gemma.hip)
# ---------------------------------------------------------------------------------------------------------
def gemma_rope(qkv, table, T, nq, nkv, h, inverse=False, out=None):
    """packed projection rows [B * T, (nq + 2 nkv) h]: the interleaved rotary embedding of nlp/gemma/gemma_attention.py:96-114 on the q and k
    heads, v copied; table fp32 [T, h] = [sin | cos]; out=None: in place"""
    _require_cuda(qkv, table)
    out = qkv if out is None else out
    W = (nq + 2 * nkv) * h
    _hip.call("iseg_gemma_rope", ptr(qkv), W, ptr(out), W, ptr(table), qkv.numel() // W, T, nq, nkv, h, int(inverse), dt(qkv), stream())
    return out


def gemma_attention_supported(nq, nkv, h, dtype):
    return dtype == torch.bfloat16 and bool(_hip.lib().iseg_gemma_attention_supported(int(nq), int(nkv), int(h), BF16))


def _gemma_split(qkv, nq, nkv, h):
    """column ranges (q, k, v) of a contiguous packed [B, T, (nq + 2 nkv) h] tensor and their common row pitch"""
    Cq, Ck = nq * h, nkv * h
    return qkv[:, :, :Cq], qkv[:, :, Cq:Cq + Ck], qkv[:, :, Cq + Ck:], qkv.shape[2]


def gemma_attention_fwd(qkv, mask_u8, nq, nkv, h, scale, want_lse):
    """causal grouped-query attention on packed rows qkv [B, T, (nq + 2 nkv) h] (contiguous), mask_u8 [B, T] uint8 or None -> ([B, T, nq h], lse)"""
    _require_cuda(qkv)
    B, T, _ = qkv.shape
    L = _hip.lib()
    q, k, v, ld = _gemma_split(qkv, nq, nkv, h)
    out = torch.empty((B, T, nq * h), dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty(int(L.iseg_gemma_attention_lse_elems(B, T, nq, nkv)), dtype=torch.float32, device=qkv.device) if want_lse else None
    _hip.check(L.iseg_gemma_attention_fwd(ptr(q), ld, ptr(k), ld, ptr(v), ld, ptr(mask_u8), ptr(out), nq * h, ptr(lse), B, T, nq, nkv, h, float(scale),
                                          dt(qkv), stream()), "iseg_gemma_attention_fwd")
    return out, lse


def gemma_attention_bwd(qkv, mask_u8, out, dout, lse, nq, nkv, h, scale):
    """gradient of gemma_attention_fwd towards the packed rows: [B, T, (nq + 2 nkv) h]"""
    _require_cuda(qkv, out, dout, lse)
    B, T, _ = qkv.shape
    L = _hip.lib()
    q, k, v, ld = _gemma_split(qkv, nq, nkv, h)
    dqkv = torch.empty_like(qkv)
    dq, dk, dv, _ = _gemma_split(dqkv, nq, nkv, h)
    dsum = torch.empty(int(L.iseg_gemma_attention_lse_elems(B, T, nq, nkv)), dtype=torch.float32, device=qkv.device)
    _hip.check(L.iseg_gemma_attention_bwd(ptr(q), ld, ptr(k), ld, ptr(v), ld, ptr(mask_u8), ptr(out), nq * h, ptr(dout), nq * h, ptr(lse), ptr(dsum),
                                          ptr(dq), ld, ptr(dk), ld, ptr(dv), ld, B, T, nq, nkv, h, float(scale), dt(qkv), stream()),
               "iseg_gemma_attention_bwd")
    return dqkv


def embedding_grad(dy2d, sorted_ids, order, dtable, scale):
    """dtable[id] += scale * sum of the rows of dy2d whose token has that id, in token order (sorted_ids, order: a stable sort of the ids);
    rows of absent ids keep their contents"""
    _require_cuda(dy2d, sorted_ids, order, dtable)
    n, d = dy2d.shape
    _hip.call("iseg_embedding_grad", ptr(dy2d), ptr(sorted_ids), ptr(order), ptr(dtable), n, dtable.shape[0], d, float(scale), dt(dy2d), stream())
    return dtable


# ---------------------------------------------------------------------------------------------------------
# Gemma with a key/value cache (csrc/gemma_decode.hip)
# ---------------------------------------------------------------------------------------------------------
def _gemma_cache_views(cache, nkv, h):
    """one layer's cache [B, 2, S, nkv, h] -> (keys, values, batch stride, row pitch): rows of nkv h contiguous elements, equally spaced"""
    if cache.dim() != 5 or cache.shape[1] != 2 or cache.shape[3] != nkv or cache.shape[4] != h or cache.stride(4) != 1 or cache.stride(3) != h:
        raise ValueError(f"a layer's cache is [B, 2, S, {nkv}, {h}] with contiguous rows, got {tuple(cache.shape)} strides {cache.stride()}")
    return cache[:, 0], cache[:, 1], cache.stride(0), cache.stride(2)


def gemma_rope_cache(qkv, cache, table, pos0, nq, nkv, h):
    """packed projection rows qkv [B, Tn, (nq + 2 nkv) h] (contiguous) of the tokens at positions pos0 .. pos0 + Tn - 1: the interleaved rotary
    embedding of nlp/gemma/gemma_attention.py:161-179 on q and k; the rotated k heads and the v heads are written into rows pos0 .. of
    cache [B, 2, S, nkv, h] (in place), the rotated q heads are returned [B, Tn, nq h]; table fp32 [S, h]"""
    _require_cuda(qkv, cache, table)
    B, Tn, W = qkv.shape
    kc, vc, bs, ld = _gemma_cache_views(cache, nkv, h)
    q = torch.empty((B, Tn, nq * h), dtype=qkv.dtype, device=qkv.device)
    _hip.call("iseg_gemma_rope_cache", ptr(qkv), W, ptr(q), nq * h, ptr(kc), bs, ld, ptr(vc), bs, ld, ptr(table), B, cache.shape[2], int(pos0), Tn,
              nq, nkv, h, dt(qkv), stream())
    return q


def gemma_decode_attention_supported(Tn, nq, nkv, h, dtype):
    return dtype == torch.bfloat16 and bool(_hip.lib().iseg_gemma_decode_attention_supported(int(Tn), int(nq), int(nkv), int(h), BF16))


def gemma_decode_attention_splits(B, pos0, Tn, nq, nkv, h):
    """the chunk count iseg_gemma_decode_attention plans for these arguments"""
    return int(_hip.lib().iseg_gemma_decode_attention_splits(int(B), int(pos0), int(Tn), int(nq), int(nkv), int(h)))


def gemma_decode_attention(q, cache, pos0, nq, nkv, h, scale, splits=0):
    """attention of the Tn new tokens q [B, Tn, nq h] at positions pos0 .. over the keys s <= pos0 + t of cache [B, 2, S, nkv, h]
    -> [B, Tn, nq h]; splits = 0: the launcher's plan"""
    _require_cuda(q, cache)
    B, Tn, _ = q.shape
    kc, vc, bs, ld = _gemma_cache_views(cache, nkv, h)
    L = _hip.lib()
    out = torch.empty((B, Tn, nq * h), dtype=q.dtype, device=q.device)
    ws, nbytes = workspace(L.iseg_gemma_decode_attention_scratch_bytes(B, int(pos0), Tn, nq, nkv, h, int(splits)), q.device)
    _hip.check(L.iseg_gemma_decode_attention(ptr(q), q.stride(1), ptr(kc), bs, ld, ptr(vc), bs, ld, ptr(out), nq * h, ptr(ws), nbytes, B,
                                             cache.shape[2], int(pos0), Tn, nq, nkv, h, float(scale), int(splits), dt(q), stream()),
               "iseg_gemma_decode_attention")
    return out


def _check_pos_d(pos_d):
    if not (torch.is_tensor(pos_d) and pos_d.dtype == torch.int32 and pos_d.numel() == 1):
        raise ValueError("a device position is ONE int32 element in device memory")
    _require_cuda(pos_d)


def gemma_rope_cache_at(qkv, cache, table, pos_d, nq, nkv, h):
    """gemma_rope_cache at the position the int32 device tensor pos_d [1] holds when the kernel runs (outside [0, S - Tn]: nothing is touched)"""
    _require_cuda(qkv, cache, table)
    _check_pos_d(pos_d)
    B, Tn, W = qkv.shape
    kc, vc, bs, ld = _gemma_cache_views(cache, nkv, h)
    q = torch.empty((B, Tn, nq * h), dtype=qkv.dtype, device=qkv.device)
    _hip.call("iseg_gemma_rope_cache_at", ptr(qkv), W, ptr(q), nq * h, ptr(kc), bs, ld, ptr(vc), bs, ld, ptr(table), B, cache.shape[2], ptr(pos_d), Tn,
              nq, nkv, h, dt(qkv), stream())
    return q


def gemma_decode_attention_at(q, cache, pos_d, nq, nkv, h, scale, splits=0):
    """gemma_decode_attention at the position the int32 device tensor pos_d [1] holds when the kernels run: bit for bit the host-position call
    there; the grid and the workspace are those of the cache's capacity (pos0 = S - Tn).  Outside [0, S - Tn] nothing is touched."""
    _require_cuda(q, cache)
    _check_pos_d(pos_d)
    B, Tn, _ = q.shape
    kc, vc, bs, ld = _gemma_cache_views(cache, nkv, h)
    S = cache.shape[2]
    L = _hip.lib()
    out = torch.empty((B, Tn, nq * h), dtype=q.dtype, device=q.device)
    ws, nbytes = workspace(L.iseg_gemma_decode_attention_scratch_bytes(B, S - Tn, Tn, nq, nkv, h, int(splits)), q.device)
    _hip.check(L.iseg_gemma_decode_attention_at(ptr(q), q.stride(1), ptr(kc), bs, ld, ptr(vc), bs, ld, ptr(out), nq * h, ptr(ws), nbytes, B, S,
                                                ptr(pos_d), Tn, nq, nkv, h, float(scale), int(splits), dt(q), stream()),
               "iseg_gemma_decode_attention_at")
    return out


# ---------------------------------------------------------------------------------------------------------
# the commit of a decoding step (csrc/decode_commit.hip)
# ---------------------------------------------------------------------------------------------------------
_IDS = {torch.int32: _hip.IDS_I32, torch.int64: _hip.IDS_I64}


def decode_commit(prompt, mask, pos_d, cur_ids, done, tokens, end_token_id):
    """one step of nlp/samplers.py's sample_loop on device state, IN PLACE (include/iseg_hip.h has the statement): prompt [B, S] and cur_ids [B]
    int32 or int64, mask [B, S] and done [B] bool or uint8, pos_d int32 [1], tokens [B] int32 or int64; end_token_id None or negative: none"""
    _require_cuda(prompt, mask, pos_d, cur_ids, done, tokens)
    _check_pos_d(pos_d)
    if prompt.dim() != 2 or prompt.dtype not in _IDS or cur_ids.dtype != prompt.dtype or tokens.dtype not in _IDS:
        raise ValueError(f"decode_commit: prompt [B, S] and cur_ids [B] share int32 or int64, tokens are int32 or int64, got {prompt.dtype}, "
                         f"{cur_ids.dtype}, {tokens.dtype}")
    B, S = prompt.shape
    if tuple(mask.shape) != (B, S) or mask.element_size() != 1 or done.element_size() != 1:
        raise ValueError(f"decode_commit: mask [{B}, {S}] and done [{B}] hold one byte per entry, got {tuple(mask.shape)} {mask.dtype}, {done.dtype}")
    for name, t in (("cur_ids", cur_ids), ("done", done), ("tokens", tokens)):
        if tuple(t.shape) != (B,) or not t.is_contiguous():
            raise ValueError(f"decode_commit: {name} is a contiguous [{B}], got {tuple(t.shape)}")
    if prompt.stride(1) != 1 or mask.stride(1) != 1:
        raise ValueError("decode_commit: the rows of prompt and mask are contiguous")
    end = -1 if end_token_id is None else int(end_token_id)
    _hip.call("iseg_decode_commit", ptr(prompt), prompt.stride(0) if B > 1 else S, ptr(mask), mask.stride(0) if B > 1 else S, ptr(pos_d), ptr(cur_ids),
              ptr(done), ptr(tokens), B, S, end if end >= 0 else -1, _IDS[prompt.dtype], _IDS[tokens.dtype], stream())


# ---------------------------------------------------------------------------------------------------------
# token sampling (csrc/token_sample.hip)
# ---------------------------------------------------------------------------------------------------------
SAMPLE_RANDOM, SAMPLE_TOP_K, SAMPLE_TOP_P = _hip.SAMPLE_RANDOM, _hip.SAMPLE_TOP_K, _hip.SAMPLE_TOP_P


def token_sample_supported(V, mode, k, dtype):
    return dtype in _DT and bool(_hip.lib().iseg_token_sample_supported(int(V), int(mode), int(k), _DT[dtype]))


def token_sample_splits(B, V):
    """the chunk count iseg_token_sample plans for these arguments"""
    return int(_hip.lib().iseg_token_sample_splits(int(B), int(V)))


def token_sample(logits, u, mode, k, p, temperature, splits=0):
    """one token id per row of logits [B, V] (rows of contiguous elements, any pitch >= V) from the uniforms u fp32 [B]: random, top-k or top-p
    sampling as include/iseg_hip.h states it -> int32 [B]; splits = 0: the launcher's plan"""
    _require_cuda(logits, u)
    B, V = logits.shape
    L = _hip.lib()
    tokens = torch.empty((B,), dtype=torch.int32, device=logits.device)
    ws, nbytes = workspace(L.iseg_token_sample_scratch_bytes(B, V, int(mode), int(k), int(splits)), logits.device)
    _hip.check(L.iseg_token_sample(ptr(logits), logits.stride(0), ptr(u), ptr(tokens), ptr(ws), nbytes, B, V, int(mode), int(k), float(p),
                                   float(temperature), int(splits), dt(logits), stream()), "iseg_token_sample")
    return tokens


# ---------------------------------------------------------------------------------------------------------
# beam search (csrc/beam_search.hip)
# ---------------------------------------------------------------------------------------------------------
def beam_select_supported(V, num_beams, dtype):
    return dtype in _DT and bool(_hip.lib().iseg_beam_select_supported(int(V), int(num_beams), _DT[dtype]))


def beam_select_splits(rows, V):
    """the chunk count iseg_beam_select plans for these arguments"""
    return int(_hip.lib().iseg_beam_select_splits(int(rows), int(V)))


def beam_select(logits, log_probs, num_beams, temperature, splits=0):
    """the num_beams best of each group's num_beams * V candidates, as include/iseg_hip.h states it: logits [B * nb, V] (rows of contiguous
    elements, any pitch >= V), log_probs fp32 [B * nb] -> (parents int32, tokens int32, new log_probs fp32), each [B * nb]; splits = 0: the
    launcher's plan"""
    _require_cuda(logits, log_probs)
    R, V = logits.shape
    L = _hip.lib()
    parents = torch.empty((R,), dtype=torch.int32, device=logits.device)
    tokens = torch.empty((R,), dtype=torch.int32, device=logits.device)
    scores = torch.empty((R,), dtype=torch.float32, device=logits.device)
    ws, nbytes = workspace(L.iseg_beam_select_scratch_bytes(R, V, int(num_beams), int(splits)), logits.device)
    _hip.check(L.iseg_beam_select(ptr(logits), logits.stride(0), ptr(log_probs), ptr(parents), ptr(tokens), ptr(scores), ptr(ws), nbytes, R, V,
                                  int(num_beams), float(temperature), int(splits), dt(logits), stream()), "iseg_beam_select")
    return parents, tokens, scores


def beam_reorder(cache, length, prompt, mask, tokens, index, parents, num_beams):
    """keras_nlp's gather_beams by parents int32 [B * nb], IN PLACE: the first `length` positions of cache [B * nb, L, 2, Sc, nkv, h] (contiguous;
    Sc need not be the prompt's S; None: no cache) and prompt [B * nb, S] (int32 or int64; None: no prompt), whose position `index` then takes
    tokens int32 [B * nb] where mask [B * nb, S] (one byte per entry) is false"""
    _require_cuda(cache, prompt, mask, tokens, parents)
    R = parents.shape[0]
    planes = Sc = row_bytes = 0
    if cache is not None:
        if cache.dim() != 6 or cache.shape[0] != R or not cache.is_contiguous():
            raise ValueError(f"beam_reorder: the cache is a contiguous [{R}, L, 2, Sc, nkv, h], got {tuple(cache.shape)} with strides {cache.stride()}")
        planes, Sc, row_bytes = cache.shape[1] * cache.shape[2], cache.shape[3], cache.shape[4] * cache.shape[5] * cache.element_size()
    S = ld_prompt = ld_mask = ids = 0
    if prompt is not None:
        if prompt.dim() != 2 or prompt.shape[0] != R or tuple(mask.shape) != tuple(prompt.shape) or mask.element_size() != 1 or tuple(tokens.shape) != (R,):
            raise ValueError(f"beam_reorder: prompt [{R}, S], a one-byte mask of its shape and tokens [{R}], got {tuple(prompt.shape)}, "
                             f"{tuple(mask.shape)} {mask.dtype}, {tuple(tokens.shape)}")
        if prompt.stride(1) != 1 or mask.stride(1) != 1:
            raise ValueError("beam_reorder: the rows of prompt and mask are contiguous")
        S, ids = prompt.shape[1], _IDS[prompt.dtype]
        ld_prompt, ld_mask = (prompt.stride(0), mask.stride(0)) if R > 1 else (S, S)
    _hip.call("iseg_beam_reorder", ptr(cache), planes, Sc, row_bytes, int(length), ptr(prompt), S, ld_prompt, ptr(mask), ld_mask, ptr(tokens),
              int(index), ids, ptr(parents), R // int(num_beams), int(num_beams), stream())


# ---------------------------------------------------------------------------------------------------------
# contrastive search (csrc/contrastive.hip)
# ---------------------------------------------------------------------------------------------------------
def contrastive_candidates_supported(V, k, dtype):
    return dtype in _DT and bool(_hip.lib().iseg_contrastive_candidates_supported(int(V), int(k), _DT[dtype]))


def contrastive_candidates_splits(rows, V):
    """the chunk count iseg_contrastive_candidates plans for these arguments"""
    return int(_hip.lib().iseg_contrastive_candidates_splits(int(rows), int(V)))


def contrastive_candidates(logits, k, temperature, row_map=None, splits=0):
    """the k most probable tokens of every output row, as include/iseg_hip.h states it: logits [R, V] (rows of contiguous elements, any pitch >=
    V); row_map None: R output rows; int32 [B]: output row b reads logits row b * (R // B) + row_map[b] -> (probs fp32 [B, k], tokens int32
    [B, k]); splits = 0: the launcher's plan"""
    _require_cuda(logits, row_map)
    R, V = logits.shape
    B = R if row_map is None else row_map.shape[0]
    group = 1
    if row_map is not None:
        if row_map.dtype != torch.int32 or row_map.dim() != 1 or not row_map.is_contiguous() or B < 1 or R % B:
            raise ValueError(f"contrastive_candidates: row_map is a contiguous int32 [B] with B dividing the {R} logits rows, got {tuple(row_map.shape)} "
                             f"{row_map.dtype}")
        group = R // B
    L = _hip.lib()
    probs = torch.empty((B, int(k)), dtype=torch.float32, device=logits.device)
    tokens = torch.empty((B, int(k)), dtype=torch.int32, device=logits.device)
    ws, nbytes = workspace(L.iseg_contrastive_candidates_scratch_bytes(B, V, int(k), int(splits)), logits.device)
    _hip.check(L.iseg_contrastive_candidates(ptr(logits), logits.stride(0) if R > 1 else V, ptr(row_map), group, ptr(probs), ptr(tokens), ptr(ws), nbytes,
                                             B, V, int(k), float(temperature), int(splits), dt(logits), stream()), "iseg_contrastive_candidates")
    return probs, tokens


def contrastive_select_supported(D, k, dtype):
    return dtype in _DT and bool(_hip.lib().iseg_contrastive_select_supported(int(D), int(k), _DT[dtype]))


def contrastive_select_splits(B, index, D, k, dtype):
    """the number of position chunks iseg_contrastive_select plans for these arguments"""
    return int(_hip.lib().iseg_contrastive_select_splits(int(B), int(index), int(D), int(k), _DT[dtype]))


def contrastive_select(hidden_states, index, cand_hidden, probs, alpha, splits=0):
    """hidden_states [B, S, D] (contiguous along D), its first `index` positions filled, cand_hidden [B * k, D] of the same dtype, probs fp32
    [B * k] -> (winner int32 [B], scores fp32 [B * k], max_sim fp32 [B * k]) as include/iseg_hip.h states it; splits = 0: the launcher's plan"""
    _require_cuda(hidden_states, cand_hidden, probs)
    B, S, D = hidden_states.shape
    R = cand_hidden.shape[0]
    k = R // B
    if cand_hidden.dim() != 2 or cand_hidden.shape[1] != D or R != B * k or cand_hidden.dtype != hidden_states.dtype or tuple(probs.shape) != (R,):
        raise ValueError(f"contrastive_select: cand_hidden [B * k, {D}] of {hidden_states.dtype} and probs [B * k], got {tuple(cand_hidden.shape)} "
                         f"{cand_hidden.dtype} and {tuple(probs.shape)}")
    if hidden_states.stride(2) != 1 or cand_hidden.stride(1) != 1 or not probs.is_contiguous():
        raise ValueError("contrastive_select: the hidden states are contiguous along D and probs is contiguous")
    L = _hip.lib()
    winner = torch.empty((B,), dtype=torch.int32, device=probs.device)
    scores = torch.empty((R,), dtype=torch.float32, device=probs.device)
    max_sim = torch.empty((R,), dtype=torch.float32, device=probs.device)
    ws, nbytes = workspace(L.iseg_contrastive_select_scratch_bytes(B, int(index), D, k, int(splits), dt(hidden_states)), probs.device)
    _hip.check(L.iseg_contrastive_select(ptr(hidden_states), hidden_states.stride(0) if B > 1 else S * hidden_states.stride(1), hidden_states.stride(1),
                                         S, int(index), ptr(cand_hidden), cand_hidden.stride(0) if R > 1 else D, ptr(probs), ptr(winner), ptr(scores),
                                         ptr(max_sim), ptr(ws), nbytes, B, D, k, float(alpha), int(splits), dt(hidden_states), stream()),
               "iseg_contrastive_select")
    return winner, scores, max_sim


def contrastive_commit(cache, pos, prompt, index, hidden_states, cand_hidden, winner, k):
    """the winner's state becomes its group's, IN PLACE (include/iseg_hip.h): position `pos` of cache [B * k, L, 2, Sc, nkv, h] (contiguous; None:
    no cache), position `index` of prompt [B * k, S] (int32 or int64; None: none) and hidden_states[b, index] = cand_hidden[b * k + winner[b]]
    (hidden_states [B, Sh, D]; None: none); winner int32 [B]"""
    _require_cuda(cache, prompt, hidden_states, cand_hidden, winner)
    B, k = winner.shape[0], int(k)
    R = B * k
    if winner.dtype != torch.int32 or winner.dim() != 1 or not winner.is_contiguous():
        raise ValueError(f"contrastive_commit: winner is a contiguous int32 [B], got {tuple(winner.shape)} {winner.dtype}")
    planes = Sc = row_bytes = 0
    if cache is not None:
        if cache.dim() != 6 or cache.shape[0] != R or not cache.is_contiguous():
            raise ValueError(f"contrastive_commit: the cache is a contiguous [{R}, L, 2, Sc, nkv, h], got {tuple(cache.shape)} with strides {cache.stride()}")
        planes, Sc, row_bytes = cache.shape[1] * cache.shape[2], cache.shape[3], cache.shape[4] * cache.shape[5] * cache.element_size()
    S = ld_prompt = ids = 0
    if prompt is not None:
        if prompt.dim() != 2 or prompt.shape[0] != R or prompt.stride(1) != 1:
            raise ValueError(f"contrastive_commit: prompt is [{R}, S] with contiguous rows, got {tuple(prompt.shape)}")
        S, ids = prompt.shape[1], _IDS[prompt.dtype]
        ld_prompt = prompt.stride(0) if R > 1 else S
    hs_b = hs_t = Sh = ldc = D = 0
    dtype = _DT[torch.float32]
    if hidden_states is not None:
        if (hidden_states.dim() != 3 or hidden_states.shape[0] != B or cand_hidden is None or tuple(cand_hidden.shape) != (R, hidden_states.shape[2])
                or cand_hidden.dtype != hidden_states.dtype or hidden_states.stride(2) != 1 or cand_hidden.stride(1) != 1):
            raise ValueError(f"contrastive_commit: hidden_states [{B}, Sh, D] and cand_hidden [{R}, D] share a dtype and are contiguous along D, got "
                             f"{tuple(hidden_states.shape)} and {None if cand_hidden is None else tuple(cand_hidden.shape)}")
        Sh, D = hidden_states.shape[1], hidden_states.shape[2]
        hs_t = hidden_states.stride(1)
        hs_b = hidden_states.stride(0) if B > 1 else Sh * hs_t
        ldc = cand_hidden.stride(0) if R > 1 else D
        dtype = dt(hidden_states)
    _hip.call("iseg_contrastive_commit", ptr(cache), planes, Sc, row_bytes, int(pos), ptr(prompt), S, ld_prompt, int(index), ids, ptr(hidden_states), hs_b,
              hs_t, Sh, ptr(cand_hidden), ldc, D, dtype, ptr(winner), B, k, stream())


# ---------------------------------------------------------------------------------------------------------
# chunked-vocabulary cross-entropy of the language-model head (csrc/lm_head_ce.hip)
# ---------------------------------------------------------------------------------------------------------
def lm_head_ce_chunk_default(M, V):
    """the chunk width used when none is forced: in [1, V] (profiles/lm_head_ce_kbench.md)"""
    return int(_hip.lib().iseg_lm_head_ce_chunk_default(int(M), int(V)))


def lm_head_ce_pitch(w):
    """row pitch of the chunk buffers Z_c (fp32) and G_c (compute dtype): whole 16-byte pieces in both"""
    return (int(w) + 7) // 8 * 8


def lm_head_ce_chunks(V, chunk):
    """[(v0, w)] covering [0, V) once, in increasing order; the last chunk may be narrower"""
    return [(v0, min(chunk, V - v0)) for v0 in range(0, V, chunk)]


def lm_head_ce_logits(x2, table, z, v0, w):
    """Z_c [M, w] fp32 (pitch z.stride(0)) = x2 [M, d] @ table[v0 : v0 + w]^T: the table's rows as they lie are the K-contiguous B operand"""
    M, d = x2.shape
    return gemm(x2, table[v0:v0 + w], z, M, w, d, lda=x2.stride(0), ldb=table.stride(0), ldd=z.stride(0), a_kcontig=1, b_kcontig=1)


def lm_head_ce_state(M, device):
    """the empty online-softmax state of M rows: (m = -inf, s = 0, z_t = 0, argmax = 0)"""
    return (torch.full((M,), float("-inf"), dtype=torch.float32, device=device), torch.zeros((M,), dtype=torch.float32, device=device),
            torch.zeros((M,), dtype=torch.float32, device=device), torch.zeros((M,), dtype=torch.int32, device=device))


def lm_head_ce_chunk_fwd(z, targets, state, v0, w):
    m, s, zt, arg = state
    _hip.call("iseg_lm_head_ce_chunk_fwd", ptr(z), z.stride(0), ptr(targets), ptr(m), ptr(s), ptr(zt), ptr(arg), z.shape[0], int(v0), int(w), stream())


def lm_head_ce_target_logit(x2, table, targets, state):
    """the state's z_t again as the fp64 dot product x_r . table[t_r], rounded once: the one logit whose accumulation error the loss carries whole"""
    _hip.call("iseg_lm_head_ce_target_logit", ptr(x2), x2.stride(0), ptr(table), table.stride(0), ptr(targets), ptr(state[2]), x2.shape[0],
              table.shape[0], x2.shape[1], dt(x2), stream())


def lm_head_ce_finalise(state, targets, weights, V, scale=1.0):
    """-> (loss [M], lse [M], match [M] int32, sums [3] = sum loss, sum w match, sum w), all fp32 but match"""
    m, s, zt, arg = state
    M = m.shape[0]
    L = _hip.lib()
    loss = torch.empty((M,), dtype=torch.float32, device=m.device)
    lse = torch.empty((M,), dtype=torch.float32, device=m.device)
    match = torch.empty((M,), dtype=torch.int32, device=m.device)
    sums = torch.empty((3,), dtype=torch.float32, device=m.device)
    ws, nbytes = workspace(L.iseg_lm_head_ce_scratch_bytes(M), m.device)
    _hip.check(L.iseg_lm_head_ce_finalise(ptr(m), ptr(s), ptr(zt), ptr(arg), ptr(targets), ptr(weights), ptr(loss), ptr(lse), ptr(match), ptr(sums),
                                          ptr(ws), nbytes, M, int(V), float(scale), stream()), "iseg_lm_head_ce_finalise")
    return loss, lse, match, sums


def lm_head_ce_chunk_bwd(z, m, s, targets, weights, upstream, scale, g, V, v0, w):
    _hip.call("iseg_lm_head_ce_chunk_bwd", ptr(z), z.stride(0), ptr(m), ptr(s), ptr(targets), ptr(weights), ptr(upstream), float(scale), ptr(g), g.stride(0),
              z.shape[0], int(V), int(v0), int(w), dt(g), stream())


def lm_head_ce_fwd(x2, table, targets, weights, chunk, scale=1.0):
    """x2 [M, d] and table [V, d] in the compute dtype, targets int32 [M], weights fp32 [M] or None -> (loss, lse, argmax, match, sums, m, s) of
    include/iseg_hip.h (m, s: the final state, what the backward pass needs); the only [M, chunk] tensor is the fp32 Z_c, written and consumed
    once per chunk"""
    _require_cuda(x2, table, targets, weights)
    M, V = x2.shape[0], table.shape[0]
    z = torch.empty((M, lm_head_ce_pitch(min(chunk, V))), dtype=torch.float32, device=x2.device)
    state = lm_head_ce_state(M, x2.device)
    for v0, w in lm_head_ce_chunks(V, chunk):
        lm_head_ce_logits(x2, table, z, v0, w)
        lm_head_ce_chunk_fwd(z, targets, state, v0, w)
    lm_head_ce_target_logit(x2, table, targets, state)
    loss, lse, match, sums = lm_head_ce_finalise(state, targets, weights, V, scale)
    return loss, lse, state[3], match, sums, state[0], state[1]


def lm_head_ce_bwd(x2, table, targets, weights, m, s, upstream, scale, chunk, dtable=None, want_dx=True):
    """the gradients of sum_r upstream[r] loss[r]: per chunk Z_c again, G_c (rounded once), dX += G_c E[c] in ONE fp32 [M, d] buffer that is cast
    at the end, and rows [v0, v0 + w) of dtable (fp32 [V, d], None: not wanted) += G_c^T X -- every row of dtable is written by one chunk only.
    -> dX in the compute dtype, or None"""
    _require_cuda(x2, table, targets, weights, m, s, upstream, dtable)
    M, d = x2.shape
    V = table.shape[0]
    if dtable is None and not want_dx:
        return None
    ld = lm_head_ce_pitch(min(chunk, V))
    z = torch.empty((M, ld), dtype=torch.float32, device=x2.device)
    g = torch.empty((M, ld), dtype=x2.dtype, device=x2.device)
    dx32 = torch.empty((M, d), dtype=torch.float32, device=x2.device) if want_dx else None
    for i, (v0, w) in enumerate(lm_head_ce_chunks(V, chunk)):
        lm_head_ce_logits(x2, table, z, v0, w)
        lm_head_ce_chunk_bwd(z, m, s, targets, weights, upstream, scale, g, V, v0, w)
        if want_dx:
            gemm(g, table[v0:v0 + w], dx32, M, d, w, lda=ld, ldb=table.stride(0), ldd=d, a_kcontig=1, b_kcontig=0, accumulate=i > 0)
        if dtable is not None:
            dense_wgrad(g[:, :w], x2, dtable[v0:v0 + w])
    if not want_dx:
        return None
    return dx32 if x2.dtype == torch.float32 else cast(dx32, x2.dtype)
