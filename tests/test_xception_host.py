"""Xception-65 (reference backbones/xception_common.py) on the host, no GPU: get_backbone builds it at output strides 8 / 16 / 32, the block
table (21 blocks, 63 separable units, activation flags, filters and skip kinds), the stride / dilation table after build_atrous_xception, the
endpoints by dry run, the weight names with a by-name .npz round trip, and the trainable parameter count."""
import pytest
import torch

from tests import xception_ref as R


def _x65(output_stride=16, size=512, return_endpoints=True):
    from iseg_amd.backbones.feature_extractor import get_backbone

    return get_backbone("xception65", output_stride=output_stride, return_endpoints=return_endpoints, image_shape=(1, size, size, 3))


def _endpoint_shapes(m, size=512):
    from iseg_amd import nn

    with nn.dry_run_scope():
        return [tuple(e.shape) for e in m(torch.empty(1, size, size, 3))]


@pytest.mark.parametrize("output_stride", [8, 16, 32])
def test_get_backbone_builds(output_stride):
    from iseg_amd import static_strings as ss
    from iseg_amd.backbones.feature_extractor import _builtin_backbones
    from iseg_amd.backbones.xception import Xception

    assert ss.XCEPTION65 in _builtin_backbones()
    m = _x65(output_stride, size=64)
    assert isinstance(m, Xception)


def test_block_table():
    m = _x65(32, size=64)
    blocks = list(m.xception_blocks)
    assert len(blocks) == 21 and [b.name for b in blocks] == [f"block{i}" for i in range(2, 23)]
    assert sum(len(b.convs) for b in blocks) == 63
    for b, want in zip(blocks, R.plan(32)):
        assert [c.filters for c in b.convs] == want["filters"]
        assert [c.activation for c in b.convs] == [want["activation"]] * 3
        assert b.skip_connection == want["skip"]
        assert hasattr(b, "shortcut") == (want["skip"] == 2)
        # the stride sits on the last unit; the shortcut carries the same stride
        assert [c.strides[0] for c in b.convs] == [1, 1, want["built_stride"]]
        if want["skip"] == 2:
            assert b.shortcut.strides == (want["built_stride"],) * 2
    assert sum(c.activation for b in blocks for c in b.convs) == 3


# (stride, dilation) per block 2..22 after build_atrous_xception, derived by hand from :241-258
TABLE = {
    32: [(2, 1)] * 3 + [(1, 1)] * 16 + [(2, 1), (1, 1)],
    16: [(2, 1)] * 3 + [(1, 1)] * 16 + [(1, 1), (1, 2)],
    8: [(2, 1)] * 2 + [(1, 1)] + [(1, 2)] * 16 + [(1, 2), (1, 4)],
}


@pytest.mark.parametrize("output_stride", [8, 16, 32])
def test_atrous_surgery_table(output_stride):
    m = _x65(output_stride, size=64)
    got = [(b.strides[0], b.atrous_rates[0]) for b in m.xception_blocks]
    assert got == TABLE[output_stride]
    assert [(p["stride"], p["rate"]) for p in R.plan(output_stride)] == TABLE[output_stride]
    for b in m.xception_blocks:
        for c in b.convs:
            assert c.atrous_rates == b.atrous_rates      # every unit of a block gets the block's rate
            assert c.strides[0] == 1 or c.atrous_rates[0] == 1      # never both > 1 in one depthwise
        if b.skip_connection == 2:
            assert b.shortcut.strides == b.strides


@pytest.mark.parametrize("output_stride,shapes", [
    (32, [(1, 256, 256, 32), (1, 256, 256, 64), (1, 128, 128, 128), (1, 64, 64, 256), (1, 32, 32, 728), (1, 16, 16, 2048)]),
    (16, [(1, 256, 256, 32), (1, 256, 256, 64), (1, 128, 128, 128), (1, 64, 64, 256), (1, 32, 32, 2048)]),
    (8, [(1, 256, 256, 32), (1, 256, 256, 64), (1, 128, 128, 128), (1, 64, 64, 2048)]),
])
def test_endpoint_shapes(output_stride, shapes):
    assert _endpoint_shapes(_x65(output_stride)) == shapes


def test_endpoint_shapes_odd_size():
    # TF 'same' at stride 2: ceil(size / 2) per stride
    assert _endpoint_shapes(_x65(16, size=97), size=97)[-1] == (1, 7, 7, 2048)


def test_weight_names():
    m = _x65(16, size=64)
    names = [p.iseg_name for p in m.parameters()]
    assert len(set(names)) == len(names)
    assert sorted(names) == sorted(R.weight_names())
    stats = {b.iseg_name for b in m.buffers()}
    assert "block22_separable_conv3_pointwise_BN/moving_variance" in stats and "block1_conv1_BN/moving_mean" in stats
    assert "block21_shortcut/kernel" in names and "block20_shortcut/kernel" not in names


def test_npz_round_trip_by_name(tmp_path):
    from iseg_amd.saver import load_h5_weight_by_name, save_weights

    a, b = _x65(16, size=64), _x65(16, size=64)
    with torch.no_grad():
        for i, p in enumerate(a.parameters()):
            p.copy_(torch.randn(p.shape, generator=torch.Generator().manual_seed(i)))
    path = save_weights(a, str(tmp_path / "xception65.npz"))
    n = load_h5_weight_by_name(b, path)
    sa = {p.iseg_name: p for p in a.parameters()}
    sb = {p.iseg_name: p for p in b.parameters()}
    assert n >= len(sa)
    assert all(torch.equal(sa[k], sb[k]) for k in sa)


def test_trainable_parameter_count():
    """37 867 312: convolution kernels plus BN gamma / beta, no biases, moving statistics excluded -- from the block table, then the model"""
    assert R.parameter_count() == 37867312
    m = _x65(16, size=64)
    assert sum(p.numel() for p in m.parameters() if p.requires_grad) == 37867312


def test_fused_knob_default_on(monkeypatch):
    from iseg_amd import functional as F

    monkeypatch.delenv("ISEG_SEPCONV_FUSED", raising=False)
    assert F.sepconv_fused_enabled()
    monkeypatch.setenv("ISEG_SEPCONV_FUSED", "0")
    assert not F.sepconv_fused_enabled()


def test_aspp_head_builds():
    from iseg_amd.heads import xception65_aspp

    model = xception65_aspp(num_class=5, output_stride=16, build_input_size=(64, 64), dropout_rate=0.0)
    assert any(p.iseg_name == "seg/logits_conv/kernel" for p in model.parameters())
