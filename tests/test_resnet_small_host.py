"""ResNet-9 / 10 / 18 (reference backbones/resnet_common.py:348-418, backbones/resnet_blocks_small.py) on the host, no GPU: get_backbone builds
them at output strides 32 / 16 / 8, the block table for Stack2 (slim) and Stack, the stride / dilation table after the atrous surgery and
multi-grid, the endpoints by dry run, the stem widths, the weight names with a strict .npz round trip, and the trainable parameter counts."""
import pytest
import torch

from tests import resnet_small_ref as R

NAMES = ["resnet9", "resnet10", "resnet18"]


def _net(name, output_stride=32, slim=True, size=64, return_endpoints=True):
    from iseg_amd.backbones.feature_extractor import get_backbone

    return get_backbone(name, output_stride=output_stride, resnet_slim=slim, return_endpoints=return_endpoints, image_shape=(1, size, size, 3))


def _endpoint_shapes(m, size):
    from iseg_amd import nn

    with nn.dry_run_scope():
        return [tuple(e.shape) for e in m(torch.empty(1, size, size, 3))]


@pytest.mark.parametrize("output_stride", [32, 16, 8])
@pytest.mark.parametrize("name", NAMES)
def test_get_backbone_builds(name, output_stride):
    from iseg_amd import static_strings as ss
    from iseg_amd.backbones.feature_extractor import _builtin_backbones
    from iseg_amd.backbones.resnet_blocks_small import BlockType2Small
    from iseg_amd.backbones.resnet_common import ResNet

    assert name in _builtin_backbones()
    m = _net(name, output_stride)
    assert isinstance(m, ResNet)
    assert m.name == (ss.RESNET9 if name in ("resnet9", "resnet10") else ss.RESNET18)      # resnet10 keeps the reference's RESNET9 name
    assert all(isinstance(b, BlockType2Small) for s in m.stacks for b in s.blocks)


@pytest.mark.parametrize("slim", [True, False])
@pytest.mark.parametrize("name", NAMES)
def test_block_table(name, slim):
    from iseg_amd.backbones.resnet_common import Stack, Stack2

    m = _net(name, 32, slim)
    want = R.plan(name, 32, slim)
    assert len(m.stacks) == 4
    for stack, ws in zip(m.stacks, want):
        assert isinstance(stack, Stack2 if slim else Stack)
        assert stack.output_endpoint == ws["endpoint"]
        assert [b.name for b in stack.blocks] == [w["name"] for w in ws["blocks"]]
        for b, w in zip(stack.blocks, ws["blocks"]):
            assert b.filters == w["filters"]
            assert b.conv_shortcut == w["conv_shortcut"] == hasattr(b, "shortcut_conv"), b.name
            assert b.strides == w["built_stride"], b.name      # no surgery at output stride 32
            if b.conv_shortcut:
                assert b.shortcut_conv.strides == (1, 1)      # the 1x1 shortcut runs at full resolution
    # the block kinds the fused tail has to cover: identity / BN0 shortcut x stride 1 / 2
    kinds = {(w["conv_shortcut"], w["built_stride"]) for ws in want for w in ws["blocks"]}
    if name == "resnet18":
        assert kinds == ({(False, 1), (False, 2), (True, 1)} if slim else {(False, 1), (True, 2)})


# (stride, dilation) per block after build_atrous_resnet + apply_multi_grid(block_index=-1, grids=[1, 2, 4]), derived by hand
TABLE18 = {
    32: [(1, 1), (2, 1), (1, 1), (2, 1), (1, 1), (2, 1), (1, 1), (1, 2)],
    16: [(1, 1), (2, 1), (1, 1), (2, 1), (1, 1), (1, 2), (1, 2), (1, 4)],
    8: [(1, 1), (2, 1), (1, 1), (1, 2), (1, 2), (1, 4), (1, 4), (1, 8)],
}
TABLE9 = {32: [(2, 1), (2, 1), (2, 1), (1, 1)], 16: [(2, 1), (2, 1), (1, 2), (1, 2)], 8: [(2, 1), (1, 2), (1, 4), (1, 4)]}


@pytest.mark.parametrize("slim", [True, False])
@pytest.mark.parametrize("output_stride", [32, 16, 8])
@pytest.mark.parametrize("name", NAMES)
def test_atrous_surgery_table(name, output_stride, slim):
    m = _net(name, output_stride, slim)
    got = [(b.strides, b.atrous_rates) for s in m.stacks for b in s.blocks]
    assert got == [(b["stride"], b["rate"]) for s in R.plan(name, output_stride, slim) for b in s["blocks"]]
    if slim:
        assert got == (TABLE18 if name == "resnet18" else TABLE9)[output_stride]
    for s in m.stacks:
        for b in s.blocks:      # atrous_rates sets both 3x3 convolutions; strides only the first
            assert b.conv1_conv.dilation_rate == b.conv2_conv.dilation_rate == (b.atrous_rates,) * 2
            assert b.conv2_conv.strides == (1, 1)


# Stack2 records the value before its last block: after the widening first block for ResNet-18, the stack's input for the one-block stacks
ENDPOINTS = {
    ("resnet18", 32): [(32, 32, 64), (16, 16, 64), (8, 8, 128), (4, 4, 256), (2, 2, 512)],
    ("resnet18", 16): [(32, 32, 64), (16, 16, 64), (8, 8, 128), (4, 4, 256), (4, 4, 512)],
    ("resnet18", 8): [(32, 32, 64), (16, 16, 64), (8, 8, 128), (8, 8, 256), (8, 8, 512)],
    ("resnet9", 32): [(32, 32, 64), (16, 16, 64), (8, 8, 64), (4, 4, 128), (2, 2, 512)],
    ("resnet9", 16): [(32, 32, 64), (16, 16, 64), (8, 8, 64), (4, 4, 128), (4, 4, 512)],
    ("resnet9", 8): [(32, 32, 64), (16, 16, 64), (8, 8, 64), (8, 8, 128), (8, 8, 512)],
}


@pytest.mark.parametrize("output_stride", [32, 16, 8])
@pytest.mark.parametrize("name", NAMES)
def test_endpoint_shapes(name, output_stride):
    want = [(1,) + s for s in ENDPOINTS[("resnet9" if name == "resnet10" else name, output_stride)]]
    assert _endpoint_shapes(_net(name, output_stride), 64) == want


def test_endpoint_shapes_odd_size():
    # TF 'same' at stride 2: ceil(size / 2) per stride; the SAME average pool of the shortcut agrees
    assert _endpoint_shapes(_net("resnet18", 32, size=97), 97)[-1] == (1, 4, 4, 512)
    assert _endpoint_shapes(_net("resnet18", 32, slim=False, size=97), 97)[-1] == (1, 4, 4, 512)


@pytest.mark.parametrize("name", NAMES)
def test_stem_widths(name):
    m = _net(name)
    got = [m.conv1_1_conv.filters, m.conv1_2_conv.filters, m.conv1_3_conv.filters]
    assert got == R.stem_widths(name) == ([24, 32, 64] if name == "resnet10" else [32, 32, 64])


@pytest.mark.parametrize("slim", [True, False])
@pytest.mark.parametrize("name", NAMES)
def test_weight_names(name, slim):
    m = _net(name, slim=slim)
    names = [p.iseg_name for p in m.parameters()]
    assert len(set(names)) == len(names)
    assert sorted(names) == sorted(R.weight_names(name, slim))
    stats = {b.iseg_name for b in m.buffers()}
    assert "conv5_block1_0_bn/moving_variance" in stats and "conv2_block1_2_bn/moving_mean" in stats


def test_npz_round_trip_strict(tmp_path):
    """the strict ResNet loader of get_backbone (by layer name, weights by position) reads the product's own .npz"""
    from iseg_amd.saver import save_weights
    from iseg_amd.utils.keras_ops import load_h5_weight

    a, b = _net("resnet18"), _net("resnet18")
    with torch.no_grad():
        for i, p in enumerate(a.parameters()):
            p.copy_(torch.randn(p.shape, generator=torch.Generator().manual_seed(i)))
        for i, t in enumerate(a.buffers()):
            t.copy_(torch.rand(t.shape, generator=torch.Generator().manual_seed(1000 + i)) + 0.5)
    path = save_weights(a, str(tmp_path / "resnet18.npz"))
    load_h5_weight(b, path)
    sa = {p.iseg_name: p for p in list(a.parameters()) + list(a.buffers())}
    sb = {p.iseg_name: p for p in list(b.parameters()) + list(b.buffers())}
    assert sa.keys() == sb.keys()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)


@pytest.mark.parametrize("name,count", [("resnet18", 11195744), ("resnet9", 4925024), ("resnet10", 4922488)])
def test_trainable_parameter_count(name, count):
    """convolution kernels plus BN gamma / beta, 3x3 stem, no biases, moving statistics excluded -- from the block table, then the model"""
    assert R.parameter_count(name) == count
    m = _net(name)
    assert sum(p.numel() for p in m.parameters() if p.requires_grad) == count


def test_fused_knob_default_on(monkeypatch):
    from iseg_amd import functional as F

    monkeypatch.delenv("ISEG_RESBLOCK_FUSED", raising=False)
    assert F.resblock_fused_enabled()
    monkeypatch.setenv("ISEG_RESBLOCK_FUSED", "0")
    assert not F.resblock_fused_enabled()


def test_non_batch_norms_take_the_composed_route():
    from iseg_amd.backbones.resnet_blocks_small import BlockType2Small
    from iseg_amd.layers.normalizations import GROUP_NROM

    b = BlockType2Small(64, stride=2, norm_method=GROUP_NROM, name="gn_block")
    b.build((1, 8, 8, 32))
    assert b.conv_shortcut and not b._tail_fusable()


def test_aspp_head_builds():
    from iseg_amd.heads import resnet18_aspp

    model = resnet18_aspp(num_class=5, output_stride=16, build_input_size=(64, 64), dropout_rate=0.0)
    assert any(p.iseg_name == "seg/logits_conv/kernel" for p in model.parameters())
    assert any(p.iseg_name == "conv5_block2_2_conv/kernel" for p in model.parameters())
