"""One table of small cases for the gradient-buffer contract (tests/test_grad_contract_gpu.py, tests/test_grad_contract_host.py).

iseg_amd/functional.py writes parameter gradients straight into `param.grad` -- a view of ParamStore.flat_g -- and returns None for them, so
every Function.backward re-implements by hand what autograd would enforce: accumulate into the buffer, give a frozen parameter nothing, sum
over every use of a shared parameter, produce the data gradient whatever is frozen.  Each case below is one tape node (or one of its routes)
at the smallest shape on which the route still runs:

    build()      -> Built(params, run, ref, inputs): `params` are fresh CUDA Parameters, `run(X)` is the
                    call the layer makes on CUDA tensors, `ref(P, X)` restates it in fp64 on CPU tensors (oracle.tf_ops, differentiable),
                    `inputs(seed)` gives the CPU inputs as (tensor, differentiable) pairs
    covers       the Function names of functional.py the call runs through (the host census checks the table against the module)
    tol          {"param": .., "dx": ..}: max-norm bands relative to the largest entry of the reference gradient -- NOT invented here: the band
                 the layer's existing parity test applies to that gradient, named in `parity`
    dy_scale     the upstream gradient is dy_scale * N(0, 1), chosen so that the largest entry of every parameter gradient of the fp64 oracle
                 lies in [2^-4, 2^4] (asserted on the oracle's values by both test files)

bf16 cases hold bf16-representable parameter values and inputs, so the oracle sees exactly what the kernels read."""
import math
import types

import torch

from oracle import tf_ops as O

F32, BF16 = torch.float32, torch.bfloat16


class Built:
    def __init__(self, params, run, ref, inputs):
        self.params, self.run, self.ref, self.inputs = params, run, ref, inputs


class Case:
    def __init__(self, name, build, covers, tol, parity, dtype=F32, dy_scale=0.25, env=None):
        self.name, self.build, self.covers, self.tol, self.parity, self.dtype, self.dy_scale = name, build, covers, tol, parity, dtype, dy_scale
        self.env = env or {}

    def __repr__(self):
        return self.name


CASES = []


def case(name, covers, tol, parity, dtype=F32, dy_scale=0.25, env=None):
    def deco(fn):
        CASES.append(Case(name, lambda: fn(dtype), covers, tol, parity, dtype, dy_scale, env))
        return fn

    return deco


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _dev():
    """where the parameters live: the GPU for the contract tests, the host for the census (which only runs the oracles)"""
    return "cuda" if torch.cuda.is_available() else "cpu"


def _q(t, dtype):
    """values the storage type holds exactly"""
    return t.to(dtype).float() if dtype != F32 else t


class _Maker:
    """fresh CUDA Parameters with the attributes nn.Layer.add_weight gives them"""

    def __init__(self, dtype, seed):
        self.dtype, self.g, self.params = dtype, _gen(seed), []

    def add(self, name, value):
        p = torch.nn.Parameter(_q(value, self.dtype).to(_dev()))
        p.iseg_name, p.lr_multiplier, p.iseg_compute = name, 1.0, None
        self.params.append(p)
        return p

    def kernel(self, name, shape, fan_in=None):
        fan_in = fan_in if fan_in is not None else math.prod(shape[:-1])
        return self.add(name, torch.randn(shape, generator=self.g) * fan_in ** -0.5)

    def bias(self, name, n, scale=0.3):
        return self.add(name, torch.randn(n, generator=self.g) * scale)

    def gamma(self, name, n):
        return self.add(name, torch.rand(n, generator=self.g) + 0.5)


def _randn(shape, seed, dtype, scale=1.0, shift=0.0):
    return _q(torch.randn(shape, generator=_gen(seed)) * scale + shift, dtype)


def _moving(C, seed):
    g = _gen(seed)
    return torch.randn(C, generator=g) * 0.2, torch.rand(C, generator=g) + 0.5


# shapes: N = 2, a 5 x 6 ... 9 x 7 plane, 8 or 16 channels
N, H, W, C = 2, 5, 6, 8

# =========================================================================================================
# Dense family
# =========================================================================================================
_GEMM = {"param": 5e-5, "dx": 2e-5}
_GEMM_PARITY = ("tests/test_kernels_gpu.py::test_gemm_wgrad_splitk (5e-5) / test_wgrad_with_fused_bias_gradient (5e-5) / "
                "test_gemm_dgrad_and_gelu_grad (close(): 2e-5)")


@case("dense_gelu", ["_DenseFn"], _GEMM, _GEMM_PARITY)
def _dense(dtype):
    from iseg_amd import functional as F, kernels as K

    m = _Maker(dtype, 1)
    Wk, b = m.kernel("dense/kernel", (C, 16)), m.bias("dense/bias", 16)
    return Built(m.params, lambda X: F.dense(X[0], Wk, b, act=K.ACT_GELU), lambda P, X: O.gelu(O.dense(X[0], P[0], P[1])),
                 lambda seed: [(_randn((N, H, W, C), seed, dtype), True)])


@case("dense_nobias_kshape", ["_DenseFn"], _GEMM, _GEMM_PARITY)
def _dense_kshape(dtype):
    """keras MultiHeadAttention's output projection: a [heads, d, C] kernel read as [heads * d, C]"""
    from iseg_amd import functional as F

    m = _Maker(dtype, 2)
    Wk = m.kernel("mha/output/kernel", (2, 4, 16), fan_in=8)
    return Built(m.params, lambda X: F.dense(X[0], Wk, None, kshape=(8, 16)), lambda P, X: X[0] @ P[0].reshape(8, 16),
                 lambda seed: [(_randn((N, 7, 8), seed, dtype), True)])


@case("mlp_gelu_residual", ["_MlpGeluFn"], _GEMM, _GEMM_PARITY)
def _mlp(dtype):
    from iseg_amd import functional as F

    m = _Maker(dtype, 3)
    W1, b1, W2, b2 = m.kernel("mlp/fc1/kernel", (C, 32)), m.bias("mlp/fc1/bias", 32), m.kernel("mlp/fc2/kernel", (32, C)), m.bias("mlp/fc2/bias", C)
    mask = torch.tensor([1.25, 0.5])

    def ref(P, X):
        y = O.dense(O.gelu(O.dense(X[0], P[0], P[1])), P[2], P[3])
        return X[1] + mask.double()[:, None, None] * y

    return Built(m.params, lambda X: F.mlp_gelu(X[0], W1, b1, W2, b2, residual=X[1], drop_path_mask=mask.cuda()), ref,
                 lambda seed: [(_randn((N, 15, C), seed, dtype), True), (_randn((N, 15, C), seed + 1, dtype), True)])


@case("dense_group_qkv", ["_DenseGroupFn"], _GEMM, _GEMM_PARITY)
def _dense_group(dtype):
    from iseg_amd import functional as F

    m = _Maker(dtype, 4)
    Wq, Wk, Wv = (m.kernel(f"mha/{n}/kernel", (C, 2, 4), fan_in=C) for n in ("query", "key", "value"))
    bq, bv = m.bias("mha/query/bias", (2, 4)), m.bias("mha/value/bias", (2, 4))

    def ref(P, X):
        q = X[0] @ P[0].reshape(C, 8) + P[3].reshape(8)
        k = X[0] @ P[1].reshape(C, 8)
        v = X[0] @ P[2].reshape(C, 8) + P[4].reshape(8)
        return torch.cat([q, k, v], -1)

    return Built(m.params, lambda X: F.dense_group(X[0], [Wq, Wk, Wv], [bq, None, bv]), ref, lambda seed: [(_randn((N, 15, C), seed, dtype), True)])


# =========================================================================================================
# Conv2D routes
# =========================================================================================================
_CONV = {"param": 5e-5, "dx": 2e-5}
_CONV_PARITY = "tests/test_kernels_gpu.py::test_conv_via_im2col_gemm (close(): 2e-5 dx) / test_gemm_wgrad_splitk (5e-5: the weight gradient is that GEMM)"


def _conv_case(name, kshape, strides, dilation, groups, bias, hw=(H, W), cin=C):
    @case(name, ["_Conv2dFn"], _CONV, _CONV_PARITY)
    def _build(dtype):
        from iseg_amd import functional as F

        m = _Maker(dtype, 10 + len(name))
        Wk = m.kernel("conv/kernel", kshape)
        b = m.bias("conv/bias", kshape[-1]) if bias else None
        return Built(m.params, lambda X: F.conv2d(X[0], Wk, b, strides, dilation, "same", groups),
                     lambda P, X: O.conv2d(X[0], P[0], P[1] if bias else None, strides, dilation, "same", groups),
                     lambda seed: [(_randn((N, hw[0], hw[1], cin), seed, dtype), True)])


_conv_case("conv_im2col_3x3_s2", (3, 3, C, 16), (2, 2), (1, 1), 1, True, hw=(9, 7))
_conv_case("conv_im2col_3x3_d2_grouped", (3, 3, 8, 16), (1, 1), (2, 2), 2, True, cin=16)      # (the group slices are copied 8 channels at a time)
_conv_case("conv_direct_1x1", (1, 1, C, 16), (1, 1), (1, 1), 1, True)
_conv_case("conv_direct_1x1_nobias", (1, 1, C, 16), (1, 1), (1, 1), 1, False)

_DW = {"param": 1e-4, "dx": 2e-5}


@case("dwconv_7x7", ["_DWConvFn"], _DW, "tests/test_kernels_gpu.py::test_dwconv_fwd_bwd (dW, db 1e-4; dx close(): 2e-5)")
def _dw7(dtype):
    from iseg_amd import functional as F

    m = _Maker(dtype, 20)
    Wk, b = m.kernel("dw/depthwise_kernel", (7, 7, C, 1), fan_in=49), m.bias("dw/bias", C)
    return Built(m.params, lambda X: F.depthwise_conv2d(X[0], Wk, b), lambda P, X: O.depthwise_conv2d(X[0], P[0], P[1]),
                 lambda seed: [(_randn((N, 9, 7, C), seed, dtype), True)])


@case("dwconv_3x3_d2", ["_DWConvFn"], _DW, "tests/test_kernels_gpu.py::test_dwconv_fwd_bwd (dW, db 1e-4; dx close(): 2e-5)")
def _dw3(dtype):
    from iseg_amd import functional as F

    m = _Maker(dtype, 21)
    Wk, b = m.kernel("dw/depthwise_kernel", (3, 3, C, 1), fan_in=9), m.bias("dw/bias", C)
    return Built(m.params, lambda X: F.depthwise_conv2d(X[0], Wk, b, dilation=2), lambda P, X: O.depthwise_conv2d(X[0], P[0], P[1], 1, 2),
                 lambda seed: [(_randn((N, H, W, C), seed, dtype), True)])


@case("dwconv_3x3_s2", ["_DWConvStridedFn"], {"param": 2e-5, "dx": 1e-5},
      "tests/test_kernels_gpu.py::test_strided_depthwise_conv_matches_oracle (fp32: dx 1e-5, dW and db 2e-5)")
def _dws(dtype):
    from iseg_amd import functional as F

    m = _Maker(dtype, 22)
    Wk, b = m.kernel("dw/depthwise_kernel", (3, 3, C, 1), fan_in=9), m.bias("dw/bias", C)
    return Built(m.params, lambda X: F.depthwise_conv2d(X[0], Wk, b, strides=2), lambda P, X: O.depthwise_conv2d(X[0], P[0], P[1], 2, 1),
                 lambda seed: [(_randn((N, 9, 7, C), seed, dtype), True)])


# =========================================================================================================
# LayerNorm family
# =========================================================================================================
_LN = {"param": 2e-4, "dx": 1e-4}


@case("layer_norm", ["_LayerNormFn"], _LN, "tests/test_kernels_gpu.py::test_layernorm_fwd_bwd (dgamma, dbeta 2e-4; dx 1e-4)")
def _ln(dtype):
    from iseg_amd import functional as F

    m = _Maker(dtype, 30)
    g, b = m.gamma("ln/gamma", C), m.bias("ln/beta", C)
    return Built(m.params, lambda X: F.layer_norm(X[0], g, b, 1e-6), lambda P, X: O.layer_norm(X[0], P[0], P[1], 1e-6),
                 lambda seed: [(_randn((N, H, W, C), seed, dtype, 2.0, 0.3), True)])


@case("layer_norm_post", ["_LayerNormPostFn"], _LN, "tests/test_kernels_gpu.py::test_layernorm_post_norm_tail (dgamma, dbeta, dcolscale 2e-4; dx 1e-4)")
def _ln_post(dtype):
    from iseg_amd import functional as F

    m = _Maker(dtype, 31)
    g, b, cs = m.gamma("ln/gamma", C), m.bias("ln/beta", C), m.gamma("layer_scale/gamma", C)
    mask = torch.tensor([0.5, 1.25])

    def ref(P, X):
        return X[1] + mask.double()[:, None, None, None] * P[2] * O.layer_norm(X[0], P[0], P[1], 1e-6)

    return Built(m.params, lambda X: F.layer_norm_post(X[0], g, b, 1e-6, colscale=cs, drop_path_mask=mask.cuda(), residual=X[1]), ref,
                 lambda seed: [(_randn((N, H, W, C), seed, dtype, 2.0, 0.3), True), (_randn((N, H, W, C), seed + 1, dtype), True)])


@case("layer_norm_permute_rows", ["_LnGatherFn"], _LN,
      "tests/test_kernels_gpu.py::test_layernorm_with_row_tables_and_gather_fma (dgamma, dbeta 2e-4; dx 1e-4)")
def _ln_gather(dtype):
    """Swin's norm1 + pad + roll + window partition: a permutation of the 30 token rows with two zero padding rows"""
    from iseg_amd import functional as F

    m = _Maker(dtype, 32)
    g, b = m.gamma("norm1/gamma", C), m.bias("norm1/beta", C)
    rows = H * W
    perm = torch.randperm(N * rows, generator=_gen(5)).tolist()
    fwd = torch.tensor(perm[:17] + [-1] + perm[17:40] + [-1] + perm[40:], dtype=torch.int32)
    inv = torch.empty(N * rows, dtype=torch.int32)
    inv[fwd[fwd >= 0].long()] = torch.nonzero(fwd >= 0).flatten().int()
    shape = (2, 31, C)

    def ref(P, X):
        ln = O.layer_norm(X[0].reshape(-1, C), P[0], P[1], 1e-5)
        return torch.where((fwd >= 0)[:, None], ln[fwd.clamp(min=0).long()], torch.zeros((), dtype=torch.float64)).reshape(shape)

    return Built(m.params, lambda X: F.layer_norm_permute_rows(X[0], g, b, 1e-5, fwd.cuda(), inv.cuda(), shape), ref,
                 lambda seed: [(_randn((N, rows, C), seed, dtype, 2.0, 0.3), True)])


@case("group_norm", ["_GroupNormFn"], {"param": 5e-5, "dx": 5e-5}, "tests/test_misc_gpu.py::test_groupnorm (dgamma, dbeta, dx 5e-5)")
def _gn(dtype):
    from iseg_amd import functional as F

    m = _Maker(dtype, 33)
    g, b = m.gamma("gn/gamma", C), m.bias("gn/beta", C)
    return Built(m.params, lambda X: F.group_norm(X[0], g, b, 2, 1e-3), lambda P, X: O.group_norm(X[0], P[0], P[1], 2, 1e-3),
                 lambda seed: [(_randn((N, H, W, C), seed, dtype, 2.0, 0.5), True)])


@case("rms_norm", ["_RMSNormFn"], {"param": 5e-5, "dx": 5e-5}, "tests/test_misc_gpu.py::test_rmsnorm (dscale, dx 5e-5)")
def _rms(dtype):
    from iseg_amd import functional as F

    m = _Maker(dtype, 34)
    s = m.bias("rms/scale", C)
    return Built(m.params, lambda X: F.rms_norm(X[0], s, 1e-6), lambda P, X: O.rms_norm(X[0], P[0], 1e-6),
                 lambda seed: [(_randn((N, 15, C), seed, dtype), True)])


@case("grn", ["_GRNFn"], {"param": 2e-5, "dx": 1e-5},
      "tests/test_convnext_v2_gpu.py::test_grn_forward_backward_match_oracle (fp32: dgamma, dbeta 2e-5; dx 1e-5)")
def _grn(dtype):
    from iseg_amd import functional as F

    m = _Maker(dtype, 35)
    g, b = m.bias("grn/gamma", (1, 1, 1, C)), m.bias("grn/beta", (1, 1, 1, C))
    return Built(m.params, lambda X: F.grn(X[0], g, b, 1e-6), lambda P, X: O.grn(X[0], P[0], P[1], 1e-6),
                 lambda seed: [(_randn((N, H, W, C), seed, dtype), True)])


@case("scale_channels", ["_ScaleChannelsFn"], {"param": 1e-4, "dx": 2e-5},
      "tests/test_kernels_gpu.py::test_colsum_broadcast_axpby_rowscale (column sums 1e-4; the data gradient is one product per element: close() 2e-5)")
def _scale(dtype):
    from iseg_amd import functional as F

    m = _Maker(dtype, 36)
    g = m.gamma("layer_scale/gamma", C)
    return Built(m.params, lambda X: F.scale_channels(X[0], g), lambda P, X: X[0] * P[0], lambda seed: [(_randn((N, H, W, C), seed, dtype), True)])


# =========================================================================================================
# BatchNorm family (training statistics unless said otherwise; sync=False: one replica)
# =========================================================================================================
_BN = {"param": 3e-4, "dx": 3e-4}
_BN_PARITY = "tests/test_kernels_gpu.py::test_batchnorm_train (dgamma, dbeta, dx 3e-4)"


def _bn_case(name, covers, training, relu):
    @case(name, covers, _BN, _BN_PARITY)
    def _build(dtype):
        from iseg_amd import functional as F

        m = _Maker(dtype, 40)
        g, b = m.gamma("bn/gamma", C), m.bias("bn/beta", C)
        mm, mv = _moving(C, 41)

        def ref(P, X):
            y = O.batch_norm_train(X[0], P[0], P[1], 1e-3)[0] if training else O.batch_norm_infer(X[0], P[0], P[1], mm.double(), mv.double(), 1e-3)
            return torch.relu(y) if relu else y

        return Built(m.params, lambda X: F.batch_norm(X[0], g, b, mm.cuda(), mv.cuda(), 1e-3, 0.9, training, relu=relu, sync=False), ref,
                     lambda seed: [(_randn((N, H, W, C), seed, dtype, 1.5, 0.2), True)])


_bn_case("batch_norm_train_relu", ["_BatchNormTrainFn"], True, True)
_bn_case("batch_norm_train", ["_BatchNormTrainFn"], True, False)
_bn_case("batch_norm_moving_stats_relu", ["_BatchNormInferFn"], False, True)


@case("batch_norm_group", ["_BatchNormGroupFn"], _BN, _BN_PARITY)
def _bn_group(dtype):
    """the ASPP branches: two layers of different widths normalised behind one statistics message"""
    from iseg_amd import functional as F

    m = _Maker(dtype, 42)
    widths = (C, 16)
    bns = []
    for i, c in enumerate(widths):
        mm, mv = _moving(c, 43 + i)
        bns.append(types.SimpleNamespace(gamma=m.gamma(f"bn_{i}/gamma", c), beta=m.bias(f"bn_{i}/beta", c), epsilon=1e-3, momentum=0.9,
                                         moving_mean=mm.to(_dev()), moving_variance=mv.to(_dev())))

    def ref(P, X):
        return tuple(torch.relu(O.batch_norm_train(X[i], P[2 * i], P[2 * i + 1], 1e-3)[0]) for i in range(2))

    return Built(m.params, lambda X: F.batch_norm_group(list(X), bns, relu=True), ref,
                 lambda seed: [(_randn((N, H, W, c), seed + i, dtype, 1.5, 0.2), True) for i, c in enumerate(widths)])


@case("bn_relu_upsample_add", ["_BnReluUpsampleAddFn"], _BN,
      "tests/test_kernels_gpu.py::test_bn_relu_upsample_add_and_remask_backward (dgamma, dbeta, dz 3e-4; resize gradient 1e-4)")
def _bn_up(dtype):
    from iseg_amd import functional as F

    m = _Maker(dtype, 45)
    g, b = m.gamma("bn/gamma", C), m.bias("bn/beta", C)
    mm, mv = _moving(C, 46)

    def ref(P, X):
        return torch.relu(O.batch_norm_train(X[0], P[0], P[1], 1e-3)[0]) + O.resize_bilinear(X[1], (10, 14))

    return Built(m.params, lambda X: F.batch_norm_relu_upsample_add(X[0], X[1], g, b, mm.cuda(), mv.cuda(), 1e-3, 0.9, sync=False), ref,
                 lambda seed: [(_randn((N, 10, 14, C), seed, dtype, 1.5, 0.2), True), (_randn((N, 4, 5, C), seed + 1, dtype), True)])


# =========================================================================================================
# token-axis helpers, embeddings
# =========================================================================================================
@case("prepend_token", ["_PrependTokenFn"], {"param": 1e-4, "dx": 0.0},
      "tests/test_kernels_gpu.py::test_colsum_broadcast_axpby_rowscale (column sums 1e-4); the data gradient is a copy: exact")
def _prepend(dtype):
    from iseg_amd import functional as F

    m = _Maker(dtype, 50)
    tok = m.bias("class_token", (1, 1, C))
    return Built(m.params, lambda X: F.prepend_token(X[0], tok), lambda P, X: torch.cat([P[0].expand(X[0].shape[0], 1, C), X[0]], 1),
                 lambda seed: [(_randn((N, 15, C), seed, dtype), True)])


@case("pos_embed_resize", ["_PosEmbedResizeFn"], {"param": 2e-5, "dx": 0.0},
      "tests/test_kernels_gpu.py::test_gemm_forward_orientation (close(): 2e-5): the gradient is two fp32 products with the constant tap matrices")
def _pos(dtype):
    from iseg_amd import functional as F
    from iseg_amd.utils.bicubic import bicubic_matrix

    m = _Maker(dtype, 51)
    pos = m.bias("pos_embed", (1, 1 + 3 * 4, C))
    Wy, Wx = torch.from_numpy(bicubic_matrix(5, 3)).float(), torch.from_numpy(bicubic_matrix(6, 4)).float()

    def ref(P, X):
        grid = P[0][0, 1:].reshape(3, 4, C)
        out = torch.einsum("ah,hwc,bw->abc", Wy.double(), grid, Wx.double()).reshape(30, C)
        return torch.cat([P[0][0, :1], out], 0)[None] + X[0]

    # (the position embedding is added to the token rows; the sum keeps a differentiable input in the case)
    return Built(m.params, lambda X: F.add_batch_broadcast(X[0], F.resize_pos_embed(pos, Wy.cuda(), Wx.cuda(), 1, dtype)), ref,
                 lambda seed: [(_randn((N, 31, C), seed, dtype), False)])


@case("embedding", ["_EmbeddingFn"], {"param": 3e-4, "dx": 0.0}, "tests/test_gemma_gpu.py::test_embedding_gradient_with_repeated_tokens (3e-4)")
def _embedding(dtype):
    from iseg_amd import functional as F

    m = _Maker(dtype, 52)
    table = m.bias("token_embedding/embeddings", (11, 16), 1.0)
    scale = float(torch.tensor(4.0).to(dtype))

    def ids(seed):
        t = torch.randint(0, 11, (N, 19), generator=_gen(seed))
        t[t == 4] = 3      # one vocabulary row stays unused: its gradient is zero
        return t

    return Built(m.params, lambda X: F.embedding(X[0], table, 4.0), lambda P, X: P[0][X[0]] * scale, lambda seed: [(ids(seed), False)])


@case("gemma_qkv", ["_GemmaQkvFn"], _GEMM, _GEMM_PARITY)
def _gqkv(dtype):
    from iseg_amd import functional as F

    m = _Maker(dtype, 53)
    Wq, Wk, Wv = m.kernel("query/kernel", (4, 16, 8), fan_in=16), m.kernel("key/kernel", (2, 16, 8), fan_in=16), m.kernel("value/kernel", (2, 16, 8), fan_in=16)

    def ref(P, X):
        return torch.cat([torch.einsum("btd,ndh->btnh", X[0], p).reshape(N, 19, -1) for p in P], -1)

    return Built(m.params, lambda X: F.gemma_qkv(X[0], Wq, Wk, Wv), ref, lambda seed: [(_randn((N, 19, 16), seed, dtype), True)])


@case("qkv_rope_bias", ["_QkvRopeFn"], {"param": 1e-4, "dx": 2e-5},
      "tests/test_kernels_gpu.py::test_colsum_broadcast_axpby_rowscale (column sums 1e-4); tests/test_eva_gpu.py::"
      "test_qkv_rope_kernel_matches_the_reference_formula_and_its_inverse_is_the_transpose (fp32 rotation)")
def _rope(dtype):
    from iseg_amd import functional as F
    from oracle import models as OM

    m = _Maker(dtype, 54)
    heads, hd, gh, gw = 2, 8, 3, 4
    Cc = heads * hd
    qb, vb = m.bias("attn/q_bias", Cc), m.bias("attn/v_bias", Cc)
    sin, cos = OM.eva_rope_table(gh, gw, hd)
    emb = torch.cat([sin, cos], -1).float()      # [tokens, 2 hd] = [sin | cos], as RotaryEmbeddingCat hands it over

    def ref(P, X):
        B, T, _ = X[0].shape
        q, k, v = X[0][..., :Cc] + P[0], X[0][..., Cc:2 * Cc], X[0][..., 2 * Cc:] + P[1]

        def rot(t):
            th = t.reshape(B, T, heads, hd)
            body = th[:, 1:] * cos[None, :, None, :] + OM.eva_rot(th[:, 1:]) * sin[None, :, None, :]
            return torch.cat([th[:, :1], body], 1).reshape(B, T, Cc)

        return torch.cat([rot(q), rot(k), v], -1)

    return Built(m.params, lambda X: F.qkv_rope(X[0], qb, vb, emb.cuda(), 1, heads), ref,
                 lambda seed: [(_randn((N, 1 + gh * gw, 3 * Cc), seed, dtype), True)])


# =========================================================================================================
# ConvNeXt blocks: the un-fused route in fp32 at C = 8, the fused bf16 route at C = 96 (LayerNorm on the MLP kernels' row loads), V2
# =========================================================================================================
_BLOCK_PARITY = "tests/test_blocks_gpu.py::test_convnext_block_forward_backward (every gradient: fp32 2e-4, bf16 4e-2)"


def _convnext_case(name, dtype, Cc, tol, dy_scale):
    @case(name, ["_ConvNeXtBlockFn"], {"param": tol, "dx": tol}, _BLOCK_PARITY, dtype=dtype, dy_scale=dy_scale)
    def _build(dtype):
        from iseg_amd import functional as F

        m = _Maker(dtype, 60)
        p = types.SimpleNamespace(dw_kernel=m.kernel("dwconv/depthwise_kernel", (7, 7, Cc, 1), fan_in=49), dw_bias=m.bias("dwconv/bias", Cc),
                                  ln_gamma=m.gamma("norm/gamma", Cc), ln_beta=m.bias("norm/beta", Cc),
                                  w1=m.kernel("pwconv1/kernel", (Cc, 4 * Cc)), b1=m.bias("pwconv1/bias", 4 * Cc),
                                  w2=m.kernel("pwconv2/kernel", (4 * Cc, Cc)), b2=m.bias("pwconv2/bias", Cc), gamma=m.gamma("gamma", Cc))
        mask = torch.tensor([1.25, 0.5])
        fused = dtype == BF16      # H * W = 64: the drop-path mask rides the fused kernels

        def ref(P, X):
            y = O.layer_norm(O.depthwise_conv2d(X[0], P[0], P[1]), P[2], P[3], 1e-6)
            y = O.dense(O.gelu(O.dense(y, P[4], P[5])), P[6], P[7]) * P[8]
            return X[0] + mask.double()[:, None, None, None] * y

        return Built(m.params, lambda X: F.convnext_block(X[0], p, 1, 1e-6, mask.cuda()), ref,
                     lambda seed: [(_randn((N, 8, 8, Cc) if fused else (N, 9, 7, Cc), seed, dtype), True)])


_convnext_case("convnext_block_unfused_fp32", F32, C, 2e-4, 0.25)
_convnext_case("convnext_block_fused_bf16_c96", BF16, 96, 4e-2, 0.0625)


@case("convnext_v2_block", ["_ConvNeXtV2BlockFn"], {"param": 2e-4, "dx": 2e-4},
      "tests/test_convnext_v2_gpu.py::test_convnext_v2_block_forward_backward (every gradient: fp32 2e-4)")
def _v2(dtype):
    from iseg_amd import functional as F

    m = _Maker(dtype, 61)
    p = types.SimpleNamespace(dw_kernel=m.kernel("dwconv/depthwise_kernel", (7, 7, C, 1), fan_in=49), dw_bias=m.bias("dwconv/bias", C),
                              ln_gamma=m.gamma("norm/gamma", C), ln_beta=m.bias("norm/beta", C),
                              w1=m.kernel("pwconv1/kernel", (C, 4 * C)), b1=m.bias("pwconv1/bias", 4 * C),
                              grn_gamma=m.bias("grn/gamma", (1, 1, 1, 4 * C)), grn_beta=m.bias("grn/beta", (1, 1, 1, 4 * C)),
                              w2=m.kernel("pwconv2/kernel", (4 * C, C)), b2=m.bias("pwconv2/bias", C))
    mask = torch.tensor([1.25, 0.5])

    def ref(P, X):
        y = O.layer_norm(O.depthwise_conv2d(X[0], P[0], P[1]), P[2], P[3], 1e-6)
        y = O.grn(O.gelu(O.dense(y, P[4], P[5])), P[6], P[7], 1e-6)
        return X[0] + mask.double()[:, None, None, None] * O.dense(y, P[8], P[9])

    return Built(m.params, lambda X: F.convnext_v2_block(X[0], p, 1, 1e-6, 1e-6, mask.cuda()), ref,
                 lambda seed: [(_randn((N, 9, 7, C), seed, dtype), True)])


@case("ln_mlp_residual_bf16_c96", ["_LnMlpResidualFn"], {"param": 4e-2, "dx": 4e-2},
      "tests/test_blocks_gpu.py::test_convnext_block_forward_backward (bf16 4e-2: the same fused MLP kernels, csrc/mlp_fused.hip / mlp_wgrad.hip)",
      dtype=BF16, dy_scale=0.25)
def _ln_mlp(dtype):
    """the second half of a Swin block as backbones/swin.py routes it: the fused node where ln_mlp_residual_supported takes it, else (partly
    frozen parameters) LayerNorm + the GELU MLP with the skip connection in its epilogue"""
    from iseg_amd import functional as F

    Cc = 96
    m = _Maker(dtype, 62)
    g, b = m.gamma("norm2/gamma", Cc), m.bias("norm2/beta", Cc)
    W1, b1, W2, b2 = m.kernel("mlp/fc1/kernel", (Cc, 4 * Cc)), m.bias("mlp/fc1/bias", 4 * Cc), m.kernel("mlp/fc2/kernel", (4 * Cc, Cc)), m.bias("mlp/fc2/bias", Cc)

    def run(X):
        x = X[0]
        if F.ln_mlp_residual_supported(x, (g, b, W1, b1, W2, b2), None):
            return F.ln_mlp_residual(x, g, b, 1e-5, W1, b1, W2, b2, None)
        x, skip = F.fork(x, 2)
        return F.mlp_gelu(F.layer_norm(x, g, b, 1e-5), W1, b1, W2, b2, residual=skip)

    def ref(P, X):
        return X[0] + O.dense(O.gelu(O.dense(O.layer_norm(X[0], P[0], P[1], 1e-5), P[2], P[3])), P[4], P[5])

    return Built(m.params, run, ref, lambda seed: [(_randn((N, 33, Cc), seed, dtype), True)])


# =========================================================================================================
# Conv2D on the matrix cores (bf16): implicit GEMM, the patchify GEMMs, the grouped ASPP branches
# =========================================================================================================
_IGEMM = {"param": 2e-4, "dx": 1.5e-2}


def _conv_bf16_case(name, kshape, strides, hw, cin, parity, tol=None):
    @case(name, ["_Conv2dFn"], tol or _IGEMM, parity, dtype=BF16)
    def _build(dtype):
        from iseg_amd import functional as F

        m = _Maker(dtype, 70 + len(name))
        Wk, b = m.kernel("conv/kernel", kshape), m.bias("conv/bias", kshape[-1])
        return Built(m.params, lambda X: F.conv2d(X[0], Wk, b, strides, (1, 1), "same", 1),
                     lambda P, X: O.conv2d(X[0], P[0], P[1], strides, 1, "same", 1),
                     lambda seed: [(_randn((N, hw[0], hw[1], cin), seed, dtype), True)])


_conv_bf16_case("conv_igemm_3x3_bf16", (3, 3, C, 16), (1, 1), (9, 7), C, "tests/test_conv_igemm_gpu.py::test_conv2d_layer_routes (bf16: dW, db 3e-4; dx 1.5e-2)",
                {"param": 3e-4, "dx": 1.5e-2})
_conv_bf16_case("conv_igemm_3x3_s2_bf16", (3, 3, C, 16), (2, 2), (9, 7), C, "tests/test_conv_igemm_gpu.py::test_conv2d_layer_routes (bf16: dW, db 3e-4; dx 1.5e-2)",
                {"param": 3e-4, "dx": 1.5e-2})
_conv_bf16_case("conv_patchify_2x2_s2_bf16", (2, 2, 64, 128), (2, 2), (8, 16), 64,
                "tests/test_conv_patchify_gpu.py::test_patch_weight_and_bias_gradient (dW, db 2e-4) / test_patch_forward_and_data_gradient (dx 1.5e-2)")


@case("conv_branches_bf16", ["_Conv2dBranchesFn"], _IGEMM,
      "tests/test_conv_branches_gpu.py::test_branches_weight_gradient (dW 2e-4) / test_branches_data_gradient (dx 1.5e-2)", dtype=BF16, dy_scale=0.125)
def _branches(dtype):
    from iseg_amd import functional as F

    Cc = 64
    m = _Maker(dtype, 75)
    Ws = [m.kernel("aspp/conv1x1/kernel", (1, 1, Cc, Cc)), m.kernel("aspp/rate1/kernel", (3, 3, Cc, Cc)), m.kernel("aspp/rate2/kernel", (3, 3, Cc, Cc))]
    dil = [(1, 1), (2, 2), (3, 3)]

    def run(X):
        assert F.conv2d_branches_supported(X[0], Ws, dil)
        return tuple(F.conv2d_branches(X[0], Ws, dil))

    return Built(m.params, run, lambda P, X: tuple(O.conv2d(X[0], w, None, 1, d, "same") for w, d in zip(P, dil)),
                 lambda seed: [(_randn((N, 9, 7, Cc), seed, dtype), True)])


# =========================================================================================================
# fused block tails: MBConv (BN - swish - squeeze-excite), Xception separable unit, JPU tail, ResNet basic-block tail
# =========================================================================================================
def _bn_layer(m, prefix, Cc, seed, sync=False):
    mm, mv = _moving(Cc, seed)
    return types.SimpleNamespace(gamma=m.gamma(f"{prefix}/gamma", Cc), beta=m.bias(f"{prefix}/beta", Cc), moving_mean=mm.to(_dev()),
                                 moving_variance=mv.to(_dev()), epsilon=1e-3, momentum=0.9, trainable=True, synchronized=sync, built=True,
                                 _init=(mm, mv))


def _reset_stats(bn):
    bn.moving_mean.copy_(bn._init[0])
    bn.moving_variance.copy_(bn._init[1])


@case("bn_swish_se", ["_BnSwishSEFn"], {"param": 1e-5, "dx": 1e-5}, "tests/test_mbconv_fused_gpu.py::test_fused_tail_fp32_matches_fp64 (every gradient 1e-5)",
      dy_scale=0.5)
def _mbconv(dtype):
    from iseg_amd import functional as F

    Cc, Cse = 32, 2
    m = _Maker(dtype, 80)
    bn = _bn_layer(m, "bn", Cc, 81)
    W1, b1, W2, b2 = m.kernel("se_reduce/kernel", (1, 1, Cc, Cse)), m.bias("se_reduce/bias", Cse), m.kernel("se_expand/kernel", (1, 1, Cse, Cc)), m.bias("se_expand/bias", Cc)

    def run(X):
        _reset_stats(bn)
        assert F.bn_swish_se_supported(X[0], Cse, bn.gamma, bn.beta, bn.moving_mean, bn.moving_variance)
        return F.bn_swish_se(X[0], bn.gamma, bn.beta, bn.moving_mean, bn.moving_variance, 1e-3, 0.9, True, W1, b1, W2, b2, sync=False)

    def ref(P, X):
        z = O.batch_norm_train(X[0], P[0], P[1], 1e-3)[0]
        a = z * torch.sigmoid(z)
        h = a.mean(dim=(1, 2)) @ P[2].reshape(Cc, Cse) + P[3]
        h = h * torch.sigmoid(h)
        return a * torch.sigmoid(h @ P[4].reshape(Cse, Cc) + P[5])[:, None, None, :]

    return Built(m.params, run, ref, lambda seed: [(_randn((N, 7, 9, Cc), seed, dtype, 1.5, 0.3), True)])


@case("sepconv_unit", ["_SepConvFn"], {"param": 1e-4, "dx": 1e-4}, "tests/test_sepconv_fused_gpu.py::test_fp32_against_fp64 (every gradient 1e-4)")
def _sepconv(dtype):
    from iseg_amd import functional as F

    Cout = 16
    m = _Maker(dtype, 82)
    dwk = m.kernel("dw/depthwise_kernel", (3, 3, C, 1), fan_in=9)
    bn = _bn_layer(m, "dw_bn", C, 83)
    pwk = m.kernel("pw/kernel", (1, 1, C, Cout))

    def run(X):
        _reset_stats(bn)
        assert F.sepconv_supported(X[0], dwk, bn, pwk, 1, 2)
        return F.sepconv_unit(X[0], dwk, bn, pwk, True, strides=1, dilation=2)

    def ref(P, X):
        z = O.depthwise_conv2d(torch.relu(X[0]), P[0], None, 1, 2, "same")
        return O.conv2d(O.batch_norm_train(z, P[1], P[2], 1e-3)[0], P[3], None, 1, 1, "same")

    return Built(m.params, run, ref, lambda seed: [(_randn((N, 9, 7, C), seed, dtype), True)])


@case("jpu_tail_moving_stats", ["_JpuTailFn"], {"param": 1e-4, "dx": 1e-4}, "tests/test_jpu_fused_gpu.py::test_fp32_against_fp64 (every gradient 1e-4)",
      dy_scale=0.0625, env={"ISEG_JPU_FUSED": "1"})
def _jpu(dtype):
    """on the moving statistics: under training statistics the BatchNorm removes the depthwise bias, whose gradient is then zero up to rounding and
    could not meet the sentinel range"""
    from iseg_amd import functional as F

    Cout = 16
    m = _Maker(dtype, 84)
    dws, bns, pws = [], [], []
    for r in (1, 2, 4, 8):
        dws.append(types.SimpleNamespace(depthwise_kernel=m.kernel(f"dw_{r}/depthwise_kernel", (3, 3, C, 1), fan_in=9), bias=m.bias(f"dw_{r}/bias", C),
                                         dilation_rate=(r, r), strides=(1, 1), padding="same"))
        bns.append(_bn_layer(m, f"bn_{r}", C, 85 + r, sync=True))
        pws.append(m.kernel(f"pw_{r}/kernel", (1, 1, C, Cout)))

    def run(X):
        assert F.jpu_tail_supported(X[0], dws, bns, pws)
        return tuple(F.jpu_tail(X[0], dws, bns, pws, False))

    def ref(P, X):
        out = []
        for i, (r, bn) in enumerate(zip((1, 2, 4, 8), bns)):
            dwk, dwb, g, b, pwk = P[5 * i:5 * i + 5]
            z = O.depthwise_conv2d(X[0], dwk, dwb, 1, r, "same")
            out.append(O.conv2d(O.batch_norm_infer(z, g, b, bn._init[0].double(), bn._init[1].double(), 1e-3), pwk, None, 1, 1, "same"))
        return tuple(out)

    return Built(m.params, run, ref, lambda seed: [(_randn((N, 9, 17, C), seed, dtype), True)])


@case("resblock_tail", ["_ResBlockTailFn"], {"param": 1e-3, "dx": 1e-3}, "tests/test_resblock_fused_gpu.py::test_tail_fp32_against_fp64 (every gradient 1e-3)",
      dy_scale=0.125)
def _resblock(dtype):
    from iseg_amd import functional as F

    Cc = 32
    m = _Maker(dtype, 90)
    bn2, bn0 = _bn_layer(m, "t_2_bn", Cc, 91), _bn_layer(m, "t_0_bn", Cc, 92)

    def run(X):
        _reset_stats(bn2), _reset_stats(bn0)
        assert F.resblock_tail_supported(X[0], X[1], bn2, bn0, (2, 2))
        return F.resblock_tail(X[0], bn2, X[1], bn0, 2, True)

    def ref(P, X):
        sc = O.avg_pool_same(O.batch_norm_train(X[1], P[2], P[3], 1e-3)[0], 2, 2)
        return torch.relu(O.batch_norm_train(X[0], P[0], P[1], 1e-3)[0] + sc)

    return Built(m.params, run, ref, lambda seed: [(_randn((N, 5, 4, Cc), seed, dtype), True), (_randn((N, 9, 7, Cc), seed + 1, dtype), True)])


# =========================================================================================================
# attention with a relative-position bias table (both routes), DCNv3's joint offset | mask projection
# =========================================================================================================
def _attention_case(name, dtype, ws, tol, parity, dy_scale):
    @case(name, ["_AttentionFn"], tol, parity, dtype=dtype, dy_scale=dy_scale)
    def _build(dtype):
        from iseg_amd import functional as F
        from iseg_amd.backbones.swin import relative_position_index

        heads, d = 2, 32
        Cc, T = heads * d, ws * ws
        m = _Maker(dtype, 95)
        table = m.bias("attn/relative_position_bias_table", ((2 * ws - 1) ** 2, heads), 0.5)
        index = torch.from_numpy(relative_position_index((ws, ws)).reshape(-1))
        scale = d ** -0.5

        def ref(P, X):
            B = X[0].shape[0]
            q, k, v = (X[0][..., i * Cc:(i + 1) * Cc].reshape(B, T, heads, d).permute(0, 2, 1, 3) for i in range(3))
            bias = P[0][index.long()].reshape(T, T, heads).permute(2, 0, 1)
            p = torch.softmax(scale * (q @ k.transpose(-1, -2)) + bias[None], dim=-1)
            return (p @ v).permute(0, 2, 1, 3).reshape(B, T, Cc)

        return Built(m.params, lambda X: F.attention_packed(X[0], heads, Cc, Cc, scale, bias_table=table, bias_index=index.cuda(), bias_window=ws), ref,
                     lambda seed: [(_randn((3, T, 3 * Cc), seed, dtype), True)])


_attention_case("attention_relpos_fp32", F32, 3, {"param": 1e-4, "dx": 1e-4},
                "tests/test_attention_gpu.py::test_attention_core_forward_backward (swin, fp32: table and qkv gradients 1e-4)", 0.25)
_attention_case("attention_relpos_window_bf16", BF16, 7, {"param": 3e-2, "dx": 3e-2},
                "tests/test_attention_gpu.py::test_attention_core_forward_backward (swin, bf16: table and qkv gradients 3e-2)", 0.25)


@case("dcnv3_joint_bf16", ["_DcnJointFn"], {"param": 3e-2, "dx": 2e-2, "norm": "l2"},
      "tests/test_dcnv3_gpu.py::test_dcnv3_layer_joint_projection_matches_layerwise (relative L2: parameter gradients 3e-2, input gradient 2e-2)",
      dtype=BF16, dy_scale=0.5)
def _dcn(dtype):
    """offsets of b + O(0.05) with b away from the cell borders: the sampling coordinates' floor() is the same in fp32 and fp64, so the offset
    gradient is continuous across the two sides (tests/test_dcnv3_gpu.py::test_dcnv3_core_forward_backward explains the border case)"""
    from iseg_amd import functional as F

    Cc, G, P9 = 64, 4, 9
    m = _Maker(dtype, 97)
    g = _gen(98)
    off = types.SimpleNamespace(kernel=m.add("dcn/offset/kernel", torch.randn(Cc, 2 * G * P9, generator=g) * 0.005),
                                bias=m.add("dcn/offset/bias", torch.sign(torch.randn(2 * G * P9, generator=g)) * (0.3 + 0.4 * torch.rand(2 * G * P9, generator=g))))
    msk = types.SimpleNamespace(kernel=m.kernel("dcn/mask/kernel", (Cc, G * P9)), bias=m.bias("dcn/mask/bias", G * P9))

    def run(X):
        y = F.dcnv3_joint(X[0], X[1], off, msk, G, Cc // G)
        assert y is not None
        return y

    def ref(P, X):
        B, Hh, Ww, _ = X[1].shape
        o = O.dense(X[1], P[0], P[1])
        a = torch.softmax(O.dense(X[1], P[2], P[3]).reshape(B, Hh, Ww, G, P9), dim=-1).reshape(B, Hh, Ww, G * P9)
        return O.dcnv3_op(X[0], o, a, (3, 3), (1, 1), "SAME", (1, 1), G, Cc // G, 1.0)

    return Built(m.params, run, ref, lambda seed: [(_randn((N, 9, 7, Cc), seed, dtype), True), (_randn((N, 9, 7, Cc), seed + 1, dtype), True)])


# =========================================================================================================
# the fp64 side, shared by the GPU tests and the host census
# =========================================================================================================
SHARED_SEED_OFFSET = 1000      # y = L(x1) + L(x2): the second use of the parameters sees the inputs of seed + this


def as_tuple(y):
    return tuple(y) if isinstance(y, (tuple, list)) else (y,)


def batches(built, seed, shared):
    """the input lists of one forward: one, or two for the shared-parameter run"""
    return [built.inputs(seed)] + ([built.inputs(seed + SHARED_SEED_OFFSET)] if shared else [])


def upstream(case, shapes, seed):
    """one upstream gradient per output, dy_scale * N(0, 1) in the case's storage type"""
    return [_q(torch.randn(tuple(shp), generator=_gen(7000 + 10 * seed + i)) * case.dy_scale, case.dtype) for i, shp in enumerate(shapes)]


def oracle(case, built, seeds=(0,), shared=False):
    """fp64 autograd through built.ref with every parameter trainable: (parameter gradients summed over `seeds`, per seed the list of input
    gradient lists (None for an input that takes none), per seed the output shapes)"""
    P = [p.detach().cpu().double().requires_grad_(True) for p in built.params]
    total = [torch.zeros_like(p) for p in P]
    dxs, shapes = [], []
    for seed in seeds:
        Xs = [[t.double().requires_grad_(True) if d else (t.double() if t.is_floating_point() else t) for t, d in X] for X in batches(built, seed, shared)]
        ys = [as_tuple(built.ref(P, X)) for X in Xs]
        y = [sum(parts) for parts in zip(*ys)]
        shapes.append([tuple(t.shape) for t in y])
        loss = sum((t * dy.double()).sum() for t, dy in zip(y, upstream(case, shapes[-1], seed)))
        leaves = [t for X in Xs for t in X if t.requires_grad]
        grads = torch.autograd.grad(loss, P + leaves, allow_unused=True)
        for acc, g in zip(total, grads[:len(P)]):
            if g is not None:
                acc += g
        it = iter(grads[len(P):])
        dxs.append([[next(it) if t.requires_grad else None for t in X] for X in Xs])
    return total, dxs, shapes


GRAD_RANGE = (2.0 ** -4, 2.0 ** 4)


def assert_oracle_gradient_range(case, grads, params):
    """a condition on the reference, not on the kernels: every parameter gradient of the oracle has its largest entry in [2^-4, 2^4], so that the
    sentinel 0.5 the buffer starts from and the gradient meet at comparable magnitudes"""
    for p, g in zip(params, grads):
        top = g.abs().max().item()
        assert GRAD_RANGE[0] <= top <= GRAD_RANGE[1], (case.name, p.iseg_name, top)
