"""JointPyramidUpsampling (reference layers/jpu.py:19-90) on the host, no GPU: the constructor surface and the sub-layer / weight names by a dry-run
build, the reference's assertion on fewer than three endpoints, the freeze of trainable=False, the C ABI of the fused tail (csrc/jpu.hip) by
name, the A/B switch, the head constructor, and the fp64 restatement tests/jpu_ref.py against a loop-based numpy depthwise convolution at a
dilation larger than the image."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

from tests import jpu_ref as R

SHAPES = [(2, 32, 40, 8), (2, 16, 20, 24), (2, 8, 10, 40), (2, 4, 5, 56)]      # the first (finest) endpoint is not used

JPU_SYMBOLS = ["iseg_jpu_supported", "iseg_jpu_partials_bytes", "iseg_jpu_dwconv3x4_stats", "iseg_jpu_bnfold_dwconv3x4_bwd"]


def _build(shapes=SHAPES, **kw):
    from iseg_amd import nn
    from iseg_amd.layers.jpu import JointPyramidUpsampling

    jpu = JointPyramidUpsampling(name="jpu", **kw)
    with nn.dry_run_scope():
        out = jpu([torch.empty(s, device=nn.device()) for s in shapes])
    return jpu, out


def test_constructor_surface():
    from iseg_amd.layers.jpu import JointPyramidUpsampling

    sig = inspect.signature(JointPyramidUpsampling.__init__)
    assert [(k, p.default) for k, p in list(sig.parameters.items())[1:]] == [("width", 512), ("trainable", True), ("name", None)]
    assert JointPyramidUpsampling().width == 512


def test_sublayers_and_weight_names():
    from iseg_amd.layers.base_layers import BatchNormalization, DepthwiseConv2D
    from iseg_amd.layers.model_builder import ConvNormAct

    jpu, out = _build(width=16)
    assert tuple(out.shape) == (2, 16, 20, 64)      # the first of the last three endpoints' size, 4 * width channels
    assert [c.name for c in jpu.endpoints_convs] == [f"jpu/endpoint_conv_{i}" for i in range(3)]
    assert [c.name for c in jpu.end_depthwise_convs] == [f"jpu/end_depthwise_conv_{r}" for r in (1, 2, 4, 8)]
    assert [c.name for c in jpu.end_depthwise_bns] == [f"jpu/end_depthwise_bn_{r}" for r in (1, 2, 4, 8)]
    assert [c.name for c in jpu.end_pointwise_convs] == [f"jpu/end_pointwise_convs_{r}" for r in (1, 2, 4, 8)]
    for c in jpu.endpoints_convs:
        assert isinstance(c, ConvNormAct) and c.conv.kernel_size == (3, 3) and c.conv.filters == 16 and c.conv.bias is None
    for r, dw, bn, pw in zip((1, 2, 4, 8), jpu.end_depthwise_convs, jpu.end_depthwise_bns, jpu.end_pointwise_convs):
        assert isinstance(dw, DepthwiseConv2D) and dw.kernel_size == (3, 3) and dw.dilation_rate == (r, r) and dw.padding == "same"
        # Keras' DepthwiseConv2D default use_bias=True: the bias is a parameter; the merged map has 3 * width channels
        assert dw.use_bias and tuple(dw.bias.shape) == (48,) and tuple(dw.depthwise_kernel.shape) == (3, 3, 48, 1)
        assert isinstance(bn, BatchNormalization) and bn.synchronized and bn.momentum == 0.9 and bn.epsilon == 1e-3
        assert isinstance(pw, ConvNormAct) and pw.conv.kernel_size == (1, 1) and tuple(pw.conv.kernel.shape) == (1, 1, 48, 16)
    names = [p.iseg_name for p in jpu.parameters()]
    assert len(set(names)) == len(names)
    assert sorted(names) == sorted(R.weight_names("jpu"))
    stats = {b.iseg_name for b in jpu.buffers()}
    assert "jpu/end_depthwise_bn_8/moving_variance" in stats and "jpu/end_pointwise_convs_1/bn/moving_mean" in stats


def test_fewer_than_three_endpoints_raise():
    with pytest.raises(AssertionError):
        _build(shapes=SHAPES[:2], width=16)


def test_not_trainable_freezes_every_sublayer():
    jpu, _ = _build(width=16, trainable=False)
    assert list(jpu.parameters()) and not any(p.requires_grad for p in jpu.parameters())
    assert not any(m.trainable for m in jpu.sublayers())


def test_npz_round_trip_by_name(tmp_path):
    from iseg_amd.saver import load_h5_weight_by_name, save_weights

    a, _ = _build(width=16)
    b, _ = _build(width=16)
    with torch.no_grad():
        for i, p in enumerate(a.parameters()):
            p.copy_(torch.randn(p.shape, generator=torch.Generator().manual_seed(i)))
    path = save_weights(a, str(tmp_path / "jpu.npz"))
    n = load_h5_weight_by_name(b, path)
    sa = {p.iseg_name: p for p in a.parameters()}
    sb = {p.iseg_name: p for p in b.parameters()}
    assert n >= len(sa)
    assert all(torch.equal(sa[k], sb[k]) for k in sa)


def test_abi_symbols_declared_exported_and_bound():
    from iseg_amd import _hip

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "iseg_hip.h")).read()
    if not os.path.exists(_hip.LIB_PATH):
        from iseg_amd.build import build

        build(verbose=False)
    dll = ctypes.CDLL(_hip.LIB_PATH)
    for name in JPU_SYMBOLS:
        assert name + "(" in header, f"{name} is not declared in iseg_hip.h"
        assert hasattr(dll, name), f"{name} is not exported"
        assert name in _hip.SIGNATURES, f"{name} has no ctypes signature"
    lib = _hip.lib()
    assert lib.iseg_jpu_supported(16, 64, 64, 1536, 1) == 1 and lib.iseg_jpu_supported(1, 5, 6, 8, 0) == 1
    assert lib.iseg_jpu_supported(1, 5, 6, 12, 0) == 0 and lib.iseg_jpu_supported(65536, 5, 6, 8, 0) == 0 and lib.iseg_jpu_supported(1, 5, 6, 8, 2) == 0
    # the partial rows of the two launches: [part][4][2C] and [part][4][10][C] floats -- a multiple of 8C and 40C floats
    fwd, bwd = lib.iseg_jpu_partials_bytes(2, 19, 21, 24, 0), lib.iseg_jpu_partials_bytes(2, 19, 21, 24, 1)
    assert fwd > 0 and fwd % (8 * 24 * 4) == 0 and bwd == 5 * fwd
    assert lib.iseg_jpu_partials_bytes(1, 5, 6, 12, 0) == 0


def test_fused_knob_is_opt_in(monkeypatch):
    """the composed operators are the default: the fused tail measured slower at the flagship geometry (EXPERIMENTS.md)"""
    from iseg_amd import functional as F

    monkeypatch.delenv("ISEG_JPU_FUSED", raising=False)
    assert not F.jpu_fused_enabled()
    monkeypatch.setenv("ISEG_JPU_FUSED", "0")
    assert not F.jpu_fused_enabled()
    monkeypatch.setenv("ISEG_JPU_FUSED", "1")
    assert F.jpu_fused_enabled()


def test_head_builds():
    from iseg_amd.heads import resnet18_jpu_aspp

    model = resnet18_jpu_aspp(num_class=5, build_input_size=(64, 64), jpu_width=32, dropout_rate=0.0)
    names = {p.iseg_name for p in model.parameters()}
    assert "seg/logits_conv/kernel" in names and "jpu_aspp_head/jpu/end_depthwise_conv_8/bias" in names
    assert tuple(model.head.jpu.end_depthwise_convs[0].depthwise_kernel.shape) == (3, 3, 96, 1)
    assert model.head.aspp.asp_convs[0].conv.dilation_rate == (12, 12)


def test_restatement_against_loops_at_a_rate_larger_than_the_image():
    """one branch at 5 x 6 x 8, dilation 8: every non-centre tap reads padding, which pins TF 'same' (pad = rate on each side at stride 1)"""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 5, 6, 8, generator=g, dtype=torch.float64)
    k = torch.randn(3, 3, 8, 1, generator=g, dtype=torch.float64)
    b = torch.randn(8, generator=g, dtype=torch.float64)
    for rate in (8, 4, 2, 1):
        got = R.O.depthwise_conv2d(x, k, b, 1, rate, "same").numpy()
        want = R.depthwise_loops(x.numpy(), k.numpy(), b.numpy(), rate)
        assert got.shape == want.shape == (1, 5, 6, 8)
        assert np.abs(got - want).max() < 1e-12, rate
    centre_only = (x * k[1, 1, :, 0] + b).numpy()
    assert np.abs(R.depthwise_loops(x.numpy(), k.numpy(), b.numpy(), 8) - centre_only).max() < 1e-12
    # the whole branch of the restatement, moving statistics: depthwise (loops) -> BN -> 1x1 by hand
    w = {"jpu/end_depthwise_conv_8/depthwise_kernel": k, "jpu/end_depthwise_conv_8/bias": b,
         "jpu/end_depthwise_bn_8/gamma": torch.rand(8, generator=g, dtype=torch.float64) + 0.5,
         "jpu/end_depthwise_bn_8/beta": torch.randn(8, generator=g, dtype=torch.float64),
         "jpu/end_depthwise_bn_8/moving_mean": torch.randn(8, generator=g, dtype=torch.float64),
         "jpu/end_depthwise_bn_8/moving_variance": torch.rand(8, generator=g, dtype=torch.float64) + 0.5,
         "jpu/end_pointwise_convs_8/conv/kernel": torch.randn(1, 1, 8, 4, generator=g, dtype=torch.float64)}
    got = R.branch_pre(w, "jpu", 8, x, False).numpy()
    u = (centre_only - w["jpu/end_depthwise_bn_8/moving_mean"].numpy()) / np.sqrt(w["jpu/end_depthwise_bn_8/moving_variance"].numpy() + 1e-3)
    u = u * w["jpu/end_depthwise_bn_8/gamma"].numpy() + w["jpu/end_depthwise_bn_8/beta"].numpy()
    want = u @ w["jpu/end_pointwise_convs_8/conv/kernel"].numpy()[0, 0]
    assert np.abs(got - want).max() < 1e-12
