"""SelfAttention without a GPU: the layer's structure under nn.dry_run_scope(), known answers of the fp64 restatement the GPU tests compare
against (tests/self_attention_ref.py), the four C entry points, and the launchers' refusal of calls outside the support set."""
import ctypes
import math
import os
import re

import pytest
import torch

from tests import self_attention_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("iseg_self_attention_supported", "iseg_self_attention_lse_elems", "iseg_self_attention_fwd", "iseg_self_attention_bwd")


def _rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float64) * scale


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def test_ref_zero_queries_average_the_values():
    """q = 0: every score is 0, the softmax is uniform and each output row is the mean of the value rows"""
    v = _rnd((2, 7, 5), 1)
    out = R.core(torch.zeros(2, 7, 3, dtype=torch.float64), _rnd((2, 7, 3), 2), v, 1.0)
    assert (out - v.mean(dim=1, keepdim=True).expand_as(v)).abs().max().item() < 1e-14


def test_ref_two_tokens_worked_by_hand():
    """T = 2, dk = 1: q = [1, 0], k = [ln 3, 0]; row 0 has scores (ln 3, 0) -> probabilities (3/4, 1/4), row 1 is uniform.
    With apply_scale and dk = 4 the score ln 3 * 2 is halved again."""
    q = torch.tensor([[[1.0], [0.0]]], dtype=torch.float64)
    k = torch.tensor([[[math.log(3.0)], [0.0]]], dtype=torch.float64)
    v = torch.tensor([[[4.0, 0.0], [0.0, 8.0]]], dtype=torch.float64)
    out = R.core(q, k, v, 1.0)
    assert torch.allclose(out, torch.tensor([[[3.0, 2.0], [2.0, 4.0]]], dtype=torch.float64), rtol=0, atol=1e-14)
    q4 = torch.cat([q * 2.0, torch.zeros(1, 2, 3, dtype=torch.float64)], dim=-1)
    k4 = torch.cat([k, torch.zeros(1, 2, 3, dtype=torch.float64)], dim=-1)
    att = R.get_attention(q4, R.transpose_hw_c(k4), apply_scale=True)
    assert torch.allclose(att, torch.tensor([[[0.75, 0.25], [0.5, 0.5]]], dtype=torch.float64), rtol=0, atol=1e-14)


def test_ref_layer_is_the_core_between_its_projections():
    N, H, W, C, G, Fv = 2, 3, 4, 5, 6, 7
    w = {f"sa/{n}/kernel": _rnd((1, 1, C, o), s) for n, o, s in (("query_conv", G, 1), ("key_conv", G, 2), ("value_conv", Fv, 3))}
    w.update({f"sa/{n}/bias": _rnd((o,), s) for n, o, s in (("query_conv", G, 4), ("key_conv", G, 5), ("value_conv", Fv, 6))})
    w["sa/out_projection/kernel"], w["sa/out_projection/bias"] = _rnd((1, 1, Fv, Fv), 7), _rnd((Fv,), 8)
    x = _rnd((N, H, W, C), 9)
    proj = {n: R.flatten_hw(R.linear_1x1(x, w[f"sa/{n}/kernel"], w[f"sa/{n}/bias"])) for n in ("query_conv", "key_conv", "value_conv")}
    want = R.core(proj["query_conv"], proj["key_conv"], proj["value_conv"], G ** -0.5).reshape(N, H, W, Fv)
    assert (R.layer(w, "sa", x, apply_scale=True) - want).abs().max().item() < 1e-13
    want = R.core(proj["query_conv"], proj["query_conv"], proj["value_conv"], 1.0).reshape(N, H, W, Fv)
    got = R.layer(w, "sa", x, shared_querykey=True, use_out_projection=True)
    assert (got - R.linear_1x1(want, w["sa/out_projection/kernel"], w["sa/out_projection/bias"])).abs().max().item() < 1e-13


# ---- the layer under dry run ----------------------------------------------------------------------------------------------------------------
def _dry_layer(shape, **kw):
    from iseg_amd import nn
    from iseg_amd.layers.self_attention import SelfAttention

    nn.set_device("cpu")
    layer = SelfAttention(name="sa", **kw)
    with nn.dry_run_scope():
        y = layer(torch.empty(shape))
    return layer, y


def test_layer_defaults_match_the_reference_constructor():
    import inspect

    from iseg_amd.layers import base_layers
    from iseg_amd.layers.self_attention import SelfAttention

    sig = inspect.signature(SelfAttention.__init__)
    assert [(n, p.default) for n, p in sig.parameters.items() if n != "self"] == [
        ("guided_filters", 64), ("filters", 512), ("shared_querykey_weights", False), ("shared_querykey", False), ("attention_dropout_rate", 0),
        ("feature_dropout_rate", 0), ("apply_scale", False), ("conv_function", base_layers.Conv2D), ("use_out_projection", False), ("name", None)]
    layer = SelfAttention()
    assert (layer.guided_filters, layer.filters, layer.apply_scale, layer.use_out_projection) == (64, 512, False, False)
    assert (layer.attention_dropout.rate, layer.feature_dropout.rate) == (0.0, 0.0)
    assert not hasattr(layer, "out_projection")


@pytest.mark.parametrize("out_projection", [False, True])
@pytest.mark.parametrize("filters", [512, 96])
def test_layer_dry_run_shapes_and_parameter_names(filters, out_projection):
    layer, y = _dry_layer((2, 5, 7, 24), filters=filters, use_out_projection=out_projection)
    assert tuple(y.shape) == (2, 5, 7, filters)
    want = {"sa/query_conv/kernel": (1, 1, 24, 64), "sa/query_conv/bias": (64,), "sa/key_conv/kernel": (1, 1, 24, 64), "sa/key_conv/bias": (64,),
            "sa/value_conv/kernel": (1, 1, 24, filters), "sa/value_conv/bias": (filters,)}
    if out_projection:
        want.update({"sa/out_projection/kernel": (1, 1, filters, filters), "sa/out_projection/bias": (filters,)})
    assert {p.iseg_name: tuple(p.shape) for p in layer.parameters()} == want
    assert [layer.query_conv.name, layer.key_conv.name, layer.value_conv.name] == ["sa/query_conv", "sa/key_conv", "sa/value_conv"]


def test_shared_querykey_shares_one_layer_object():
    layer, y = _dry_layer((1, 4, 4, 16), shared_querykey=True, guided_filters=32, filters=48)
    assert layer.key_conv is layer.query_conv
    assert tuple(y.shape) == (1, 4, 4, 48)
    assert sorted(p.iseg_name for p in layer.parameters()) == ["sa/query_conv/bias", "sa/query_conv/kernel", "sa/value_conv/bias",
                                                               "sa/value_conv/kernel"]


def test_shared_querykey_weights_give_equal_initial_kernels():
    layer, _ = _dry_layer((1, 4, 4, 16), shared_querykey_weights=True)
    assert layer.key_conv is not layer.query_conv
    assert layer.key_conv.kernel.data_ptr() != layer.query_conv.kernel.data_ptr()
    assert torch.equal(layer.key_conv.kernel.data, layer.query_conv.kernel.data) and layer.query_conv.kernel.abs().max().item() > 0
    plain, _ = _dry_layer((1, 4, 4, 16))
    assert not torch.equal(plain.key_conv.kernel.data, plain.query_conv.kernel.data)


def test_conv_function_receives_the_reference_arguments():
    from iseg_amd.layers import base_layers

    seen = []

    def conv(filters, kernel_size, **kw):
        seen.append((filters, kernel_size, kw.get("kernel_initializer"), kw["name"].rsplit("/", 1)[-1]))
        return base_layers.Conv2D(filters, kernel_size, **kw)

    _dry_layer((1, 3, 3, 8), guided_filters=16, filters=40, conv_function=conv, use_out_projection=True)
    assert seen == [(16, 1, "glorot_uniform", "query_conv"), (16, 1, "glorot_uniform", "key_conv"), (40, 1, None, "value_conv"),
                    (40, 1, "glorot_uniform", "out_projection")]


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------
def _lib():
    from iseg_amd import _hip

    if not os.path.exists(_hip.LIB_PATH):
        from iseg_amd.build import build

        build(verbose=False)
    return _hip.lib()


def test_header_declares_and_library_exports_the_entry_points():
    from iseg_amd import _hip

    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "iseg_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(?:int|size_t)\s+(iseg_[a-z0-9_]+)\s*\(", src))
    _lib()
    dll = ctypes.CDLL(_hip.LIB_PATH)
    for name in SYMBOLS:
        assert name in declared and hasattr(dll, name) and name in _hip.SIGNATURES, name
    assert not [n for n in declared if "self_attention" in n and n.endswith("_workspace_bytes")]


def test_support_set_and_lse_size():
    L = _lib()
    ok = [(64, dv) for dv in (64, 128, 192, 512, 1024)]
    bad = [(32, 64), (128, 128), (64, 96), (64, 32), (64, 0), (64, 1088), (64, 520)]
    assert all(L.iseg_self_attention_supported(dk, dv, 1) == 1 for dk, dv in ok)
    assert all(L.iseg_self_attention_supported(dk, dv, 1) == 0 for dk, dv in bad)
    assert L.iseg_self_attention_supported(64, 512, 0) == 0      # fp32 storage
    assert [L.iseg_self_attention_lse_elems(b, t) for b, t in ((1, 1), (3, 64), (2, 65), (16, 4096))] == [64, 192, 256, 65536]


@pytest.mark.parametrize("what,dk,dv,pitch", [("dk", 32, 64, None), ("dv", 64, 96, None), ("pitch", 64, 128, 60), ("pitch", 64, 128, 260)])
def test_launchers_refuse_calls_outside_the_support_set_without_a_device(what, dk, dv, pitch):
    """refused before any memory is touched: the operands are host buffers no kernel could read, and no device exists here"""
    from iseg_amd import _hip

    L = _lib()
    T = 5
    buf = torch.zeros(16 * 1024, dtype=torch.bfloat16)      # host memory, 16-byte aligned by the allocator
    fl = torch.zeros(256, dtype=torch.float32)
    p, f = buf.data_ptr(), fl.data_ptr()
    assert p % 16 == 0 and f % 16 == 0
    ldq = pitch if pitch is not None else dk
    st = L.iseg_self_attention_fwd(p, ldq, p, dk, p, dv, p, dv, f, 1, T, dk, dv, 1.0, 1, None)
    assert st < 0, st
    assert what in _hip.last_error() and "iseg_self_attention_fwd" in _hip.last_error()
    st = L.iseg_self_attention_bwd(p, ldq, p, dk, p, dv, p, dv, p, dv, f, f, p, dk, p + 4096, dk, p, dv, 1, T, dk, dv, 1.0, 1, None)
    assert st < 0, st
    assert what in _hip.last_error() and "iseg_self_attention_bwd" in _hip.last_error()
    assert buf.abs().max().item() == 0 and fl.abs().max().item() == 0


def test_core_dry_run_and_shape_check():
    from iseg_amd import functional as F
    from iseg_amd import nn

    nn.set_device("cpu")
    with nn.dry_run_scope():
        assert tuple(F.self_attention_core(torch.empty(2, 9, 64), torch.empty(2, 9, 64), torch.empty(2, 9, 512), 1.0).shape) == (2, 9, 512)
        with pytest.raises(ValueError):
            F.self_attention_core(torch.empty(2, 9, 64), torch.empty(2, 8, 64), torch.empty(2, 9, 512), 1.0)
