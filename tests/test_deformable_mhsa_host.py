"""DeformableMultiHeadSelfAttentionLayer without a GPU: known answers of the fp64 restatement the GPU tests compare against
(tests/deformable_mhsa_ref.py), and the layer's structure under nn.dry_run_scope()."""
import math

import pytest
import torch

from tests import deformable_mhsa_ref as R


def _rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float64) * scale


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,heads,P", [((2, 5, 4, 6), 3, 4), ((1, 3, 7, 8), 2, 1)])
def test_ref_zero_offsets_return_the_value(shape, heads, P):
    """tanh(0) = 0: every point samples its own pixel with weight (1, 0, 0, 0), and the softmax weights sum to one"""
    N, H, W, C = shape
    v = torch.round(_rnd(shape, 1) * 8)      # small integers: sum_p a_p v is exact whenever sum_p a_p is
    a = torch.full((N, H, W, heads * P), 0.5, dtype=torch.float64)      # equal logits: a_p = 1 / P exactly for P in {1, 4}
    out = R.core(v, torch.zeros(N, H, W, heads * P * 2, dtype=torch.float64), a, heads, P, 8.0)
    assert torch.equal(out, v)
    # any logits: equal up to the rounding of sum_p a_p
    out = R.core(v, torch.zeros(N, H, W, heads * P * 2, dtype=torch.float64), _rnd((N, H, W, heads * P), 2), heads, P, 8.0)
    assert (out - v).abs().max().item() < 1e-13


def test_ref_saturated_offsets_sample_the_bottom_right_pixel():
    """tanh(30) rounds to 1: dy = H, dx = W with offset_range_factor 1, so every sample clips to (H - 1, W - 1) of its own head"""
    N, H, W, heads, P, Ch = 2, 4, 5, 2, 3, 3
    v = _rnd((N, H, W, heads * Ch), 3)
    out = R.core(v, torch.full((N, H, W, heads * P * 2), 30.0, dtype=torch.float64), _rnd((N, H, W, heads * P), 4), heads, P, 1.0)
    want = v[:, H - 1:, W - 1:, :].expand(N, H, W, heads * Ch)
    assert (out - want).abs().max().item() < 1e-13


def test_ref_two_by_two_worked_by_hand():
    """H = W = 2, one head, one point, one channel, offset_range_factor 2 (scales H / 2 = W / 2 = 1).  v = [[1, 2], [3, 4]].
    Pixel (0, 0) gets the y logit atanh(0.5): y = 0 + 0.5, x = 0 -> y0 = 0, y1 = 1, wy1 = 0.5, wx1 = 0:
        out = 0.5 * v[0,0] + 0.5 * v[1,0] = 2
        d out / d y = v[1,0] - v[0,0] = 2;  d y / d logit = 1 * (1 - 0.5^2) = 0.75  -> 1.5;    d out / d x = 0.5 (v[0,1] - v[0,0]) + 0.5 (v[1,1] - v[1,0]) = 1
        d out / d v = 0.5 at (0,0) and (1,0)
    Every other pixel has zero logits and returns itself.  The single attention logit has softmax 1 and gradient 0."""
    v = torch.tensor([[1.0, 2.0], [3.0, 4.0]], dtype=torch.float64).reshape(1, 2, 2, 1).requires_grad_(True)
    off = torch.zeros(1, 2, 2, 2, dtype=torch.float64)
    off[0, 0, 0, 0] = math.atanh(0.5)
    off.requires_grad_(True)
    att = torch.full((1, 2, 2, 1), 0.7, dtype=torch.float64, requires_grad=True)
    out = R.core(v, off, att, 1, 1, 2.0)
    assert torch.allclose(out.reshape(2, 2), torch.tensor([[2.0, 2.0], [3.0, 4.0]], dtype=torch.float64), rtol=0, atol=1e-15)
    out[0, 0, 0, 0].backward()
    assert abs(off.grad[0, 0, 0, 0].item() - 1.5) < 1e-14 and abs(off.grad[0, 0, 0, 1].item() - 1.0) < 1e-14
    assert torch.allclose(v.grad.reshape(2, 2), torch.tensor([[0.5, 0.0], [0.5, 0.0]], dtype=torch.float64), rtol=0, atol=1e-15)
    assert att.grad.abs().max().item() == 0.0


def test_ref_clipped_samples_have_exactly_zero_offset_gradient():
    N, H, W, heads, P, Ch = 2, 6, 5, 2, 4, 3
    v = _rnd((N, H, W, heads * Ch), 5)
    off = (_rnd((N, H, W, heads * P * 2), 6) * 1.5).requires_grad_(True)
    att = _rnd((N, H, W, heads * P), 7)
    yu, xu, _, _ = R.sampling_coordinates(off.detach(), H, W, heads, P, 1.0)
    R.core(v, off, att, heads, P, 1.0).backward(_rnd((N, H, W, heads * Ch), 8))
    g = off.grad.reshape(N, H, W, heads, P, 2)
    clip_y, clip_x = (yu < 0) | (yu > H - 1), (xu < 0) | (xu > W - 1)
    assert clip_y.float().mean().item() > 0.2 and (~clip_y).float().mean().item() > 0.1
    assert g[..., 0][clip_y].abs().max().item() == 0.0 and g[..., 1][clip_x].abs().max().item() == 0.0
    assert g[..., 0][~clip_y].abs().min().item() > 0.0      # ... and only those


# ---- the layer under dry run ----------------------------------------------------------------------------------------------------------------
def _dry_layer(shape, **kw):
    from iseg_amd import nn
    from iseg_amd.layers.deformable_multihead_self_attention import DeformableMultiHeadSelfAttentionLayer

    nn.set_device("cpu")
    layer = DeformableMultiHeadSelfAttentionLayer(name="dmhsa", **kw)
    with nn.dry_run_scope():
        y = layer(torch.empty(shape))
    return layer, y


def test_layer_defaults_match_the_reference_constructor():
    from iseg_amd.layers.deformable_multihead_self_attention import DeformableMultiHeadSelfAttentionLayer

    layer = DeformableMultiHeadSelfAttentionLayer()
    assert (layer.filters, layer.num_heads, layer.num_points, layer.apply_linear, layer.shared_qk, layer.use_dense_for_linear,
            layer.offset_range_factor, layer.use_jit_compile, layer.trainable) == (-1, 4, 4, True, False, False, 8.0, False, True)


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("filters", [-1, 32])
def test_layer_dry_run_shapes_and_parameter_names(filters, dense):
    shape = (2, 9, 7, 16)
    heads, P = 4, 3
    layer, y = _dry_layer(shape, filters=filters, num_heads=heads, num_points=P, use_dense_for_linear=dense)
    Cv = 16 if filters == -1 else filters
    assert tuple(y.shape) == (2, 9, 7, Cv)
    shapes = {p.iseg_name: tuple(p.shape) for p in layer.parameters()}
    k = (lambda cout: (16, cout)) if dense else (lambda cout: (1, 1, 16, cout))
    assert shapes == {"dmhsa/value_proj/kernel": k(Cv), "dmhsa/value_proj/bias": (Cv,),
                      "dmhsa/offset_proj/kernel": k(heads * P * 2), "dmhsa/offset_proj/bias": (heads * P * 2,),
                      "dmhsa/attn_proj/kernel": k(heads * P), "dmhsa/attn_proj/bias": (heads * P,)}


def test_layer_without_linear_has_no_value_projection_and_takes_a_separate_value():
    from iseg_amd import nn

    layer, y = _dry_layer((1, 6, 6, 24), apply_linear=False, num_heads=3)
    assert tuple(y.shape) == (1, 6, 6, 24) and layer.value_proj is None
    assert sorted(p.iseg_name for p in layer.parameters()) == ["dmhsa/attn_proj/bias", "dmhsa/attn_proj/kernel", "dmhsa/offset_proj/bias",
                                                               "dmhsa/offset_proj/kernel"]
    with nn.dry_run_scope():      # value= of another width: the output follows the value
        assert tuple(layer(torch.empty(1, 6, 6, 24), value=torch.empty(1, 6, 6, 12)).shape) == (1, 6, 6, 12)


@pytest.mark.parametrize("filters,channels", [(-1, 18), (30, 16)])
def test_layer_refuses_value_filters_not_divisible_by_heads(filters, channels):
    with pytest.raises(ValueError, match="divisible by num_heads"):
        _dry_layer((1, 4, 4, channels), filters=filters, num_heads=4)
