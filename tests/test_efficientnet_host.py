"""EfficientNet B0-B7 / L2 (reference backbones/efficientnet.py) on the host, no GPU: the nine names construct through get_backbone, block counts
and widths follow round_repeats / round_filters, B0's endpoint shapes and dilation rates after the surgery, use_top, the Keras weight names and
B0's trainable parameter count."""
import math
import re

import pytest
import torch

from tests import efficientnet_ref as R

NAMES = ["efficientnetb0", "efficientnetb1", "efficientnetb2", "efficientnetb3", "efficientnetb4", "efficientnetb5", "efficientnetb6",
         "efficientnetb7", "efficientnetl2"]
COEFFS = {"efficientnetb0": (1.0, 1.0), "efficientnetb1": (1.0, 1.1), "efficientnetb2": (1.1, 1.2), "efficientnetb3": (1.2, 1.4),
          "efficientnetb4": (1.4, 1.8), "efficientnetb5": (1.6, 2.2), "efficientnetb6": (1.8, 2.6), "efficientnetb7": (2.0, 3.1),
          "efficientnetl2": (4.3, 5.3)}


def _b0(output_stride=32, use_top=True, size=224):
    from iseg_amd.backbones.feature_extractor import get_backbone

    return get_backbone("efficientnetb0", output_stride=output_stride, return_endpoints=True, image_shape=(1, size, size, 3),
                        efficientnet_use_top=use_top)


def _endpoint_shapes(m, size=224):
    from iseg_amd import nn

    with nn.dry_run_scope():
        return [tuple(e.shape) for e in m(torch.empty(1, size, size, 3))]


@pytest.mark.parametrize("name", NAMES)
def test_every_name_constructs_with_round_repeats_and_round_filters(name):
    from iseg_amd import static_strings as ss
    from iseg_amd.backbones import efficientnet as E
    from iseg_amd.backbones.feature_extractor import _builtin_backbones, get_backbone

    assert getattr(ss, name.upper()) == name and name in _builtin_backbones()
    width, depth = COEFFS[name]
    m = get_backbone(name, output_stride=32, return_endpoints=False, image_shape=(1, 32, 32, 3))
    assert isinstance(m, E.EfficientNet)
    reps = [1, 2, 2, 3, 3, 4, 1]
    assert len(m.blocks) == sum(int(math.ceil(depth * r)) for r in reps)
    want_out = [R.round_filters(f, width) for f in (16, 24, 40, 80, 112, 192, 320)]
    stage_out = {}
    for b in m.blocks:
        stage_out[int(b.name[5])] = b.filters_out
    assert [stage_out[i] for i in range(1, 8)] == want_out
    assert m.stem_conv.kernel.shape[-1] == R.round_filters(32, width)
    assert m.top_conv.kernel.shape[-1] == R.round_filters(1280, width)
    # se_filters come from the block's INPUT width, not the expanded one
    for b in m.blocks:
        assert b.se_reduce.kernel.shape == (1, 1, b.filters, max(1, int(b.filters_in * 0.25)))
        assert b.se_expand.kernel.shape == (1, 1, max(1, int(b.filters_in * 0.25)), b.filters)


def test_block_counts_b0_b7():
    from iseg_amd.backbones.efficientnet import EfficientNetB0, EfficientNetB7

    assert len(EfficientNetB0().blocks) == 16
    assert len(EfficientNetB7(default_size=600).blocks) == 55      # default_size is accepted and dropped


@pytest.mark.parametrize("output_stride,shapes", [
    (32, [(1, 112, 112, 16), (1, 56, 56, 24), (1, 28, 28, 40), (1, 14, 14, 112), (1, 7, 7, 1280)]),
    (16, [(1, 112, 112, 16), (1, 56, 56, 24), (1, 28, 28, 40), (1, 14, 14, 112), (1, 14, 14, 1280)]),
    (8, [(1, 112, 112, 16), (1, 56, 56, 24), (1, 28, 28, 40), (1, 28, 28, 112), (1, 28, 28, 1280)]),
])
def test_b0_endpoint_shapes(output_stride, shapes):
    assert _endpoint_shapes(_b0(output_stride)) == shapes


# hand-derived from build_dilated_efficientnet (:492-507): blocks 1a 2a 2b 3a 3b 4a 4b 4c 5a 5b 5c 6a 6b 6c 6d 7a
SURGERY = {
    32: ([1, 2, 1, 2, 1, 2, 1, 1, 1, 1, 1, 2, 1, 1, 1, 1], [1] * 16),
    16: ([1, 2, 1, 2, 1, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1], [1] * 11 + [2] * 5),
    8: ([1, 2, 1, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1], [1] * 5 + [2] * 6 + [4] * 5),
}


@pytest.mark.parametrize("output_stride", [32, 16, 8])
def test_b0_dilation_surgery(output_stride):
    m = _b0(output_stride)
    strides, rates = SURGERY[output_stride]
    assert [b.dwconv.strides[0] for b in m.blocks] == strides
    assert [b.dwconv.dilation_rate[0] for b in m.blocks] == rates
    assert all(b.dwconv.padding == "same" for b in m.blocks)
    # endpoints stay on the blocks BUILT with a stride (not re-evaluated after the surgery)
    assert [b.name for b in m.blocks if b.output_endpoint] == ["block2a_", "block3a_", "block4a_", "block6a_"]
    plan = R.plan(output_stride=output_stride)
    assert [p["stride"] for p in plan] == strides and [p["dilation"] for p in plan] == rates


def test_use_top_false_drops_top():
    m = _b0(32, use_top=False)
    names = {p.iseg_name for p in m.parameters()}
    assert not any(n.startswith("top_") for n in names)
    assert not hasattr(m, "top_conv")
    assert _endpoint_shapes(m)[-1] == (1, 7, 7, 320)


def test_b0_weight_names():
    m = _b0(32)
    names = sorted(p.iseg_name for p in m.parameters()) + sorted(b.iseg_name for b in m.buffers())
    pat = re.compile(r"^(stem_conv/kernel|(stem|top)_bn/(gamma|beta|moving_mean|moving_variance)|top_conv/kernel|"
                     r"block[1-7][a-d]_(expand_conv/kernel|dwconv/depthwise_kernel|(se_reduce|se_expand)/(kernel|bias)|project_conv/kernel|"
                     r"(expand_bn|bn|project_bn)/(gamma|beta|moving_mean|moving_variance)))$")
    bad = [n for n in names if not pat.match(n)]
    assert not bad, bad[:5]
    assert "block1a_expand_conv/kernel" not in names      # expand_ratio 1: no expansion
    assert "block2a_expand_conv/kernel" in names and "block7a_se_expand/bias" in names
    assert len(set(names)) == len(names)


def _count_from_table(width=1.0, depth=1.0):
    stem = R.round_filters(32, width)
    n = 3 * 3 * 3 * stem + 2 * stem
    for b in R.plan(width, depth):
        fin, fout, k = b["filters_in"], b["filters_out"], b["k"]
        fexp = fin * b["expand"]
        se = max(1, int(fin * 0.25))
        if b["expand"] != 1:
            n += fin * fexp + 2 * fexp
        n += k * k * fexp + 2 * fexp
        n += fexp * se + se + se * fexp + fexp
        n += fexp * fout + 2 * fout
    top = R.round_filters(1280, width)
    return n + R.round_filters(320, width) * top + 2 * top


def test_b0_trainable_parameter_count():
    """Keras' published figure for EfficientNetB0(include_top=False): 4 007 548 trainable parameters -- confirmed by counting from the block
    table, then against the model"""
    assert _count_from_table() == 4007548
    m = _b0(32)
    assert sum(p.numel() for p in m.parameters() if p.requires_grad) == 4007548


def test_fused_knob_default_on(monkeypatch):
    from iseg_amd import functional as F

    assert F.mbconv_fused_enabled()
    monkeypatch.setenv("ISEG_MBCONV_FUSED", "0")
    assert not F.mbconv_fused_enabled()
