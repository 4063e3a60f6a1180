"""Gemma backbone, CPU side: known answers of the fp64 restatement (tests/gemma_ref.py) that the device tests lean on, the preset parameter
counts from shape arithmetic alone, variable names and shapes, and the refusal of the KV cache."""
import math

import pytest
import torch

from tests import gemma_ref as R

# nlp/gemma/gemma_presets.py: the `params` fields of gemma_2b_en and gemma_7b_en
GEMMA_2B = dict(vocabulary_size=256000, num_layers=18, num_query_heads=8, num_key_value_heads=1, hidden_dim=2048, intermediate_dim=32768, head_dim=256)
GEMMA_7B = dict(vocabulary_size=256000, num_layers=28, num_query_heads=16, num_key_value_heads=16, hidden_dim=3072, intermediate_dim=49152, head_dim=256)
TINY = dict(vocabulary_size=97, num_layers=2, num_query_heads=4, num_key_value_heads=2, hidden_dim=128, intermediate_dim=512, head_dim=64)


def _rnd(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def test_rope_preserves_the_dot_product_at_equal_positions():
    q, k = _rnd((1, 9, 2, 64), 1), _rnd((1, 9, 2, 64), 2)
    pos = torch.arange(9, dtype=torch.float64)[None]
    a, b = R.apply_rope(q, pos), R.apply_rope(k, pos)
    assert torch.allclose((a * b).sum(-1), (q * k).sum(-1), rtol=1e-12, atol=1e-12)


def test_rope_depends_only_on_the_position_difference():
    q, k = _rnd((1, 1, 1, 64), 3), _rnd((1, 1, 1, 64), 4)
    dots = []
    for t, s in ((5, 2), (105, 102), (300, 297)):
        a = R.apply_rope(q, torch.tensor([[float(t)]], dtype=torch.float64))
        b = R.apply_rope(k, torch.tensor([[float(s)]], dtype=torch.float64))
        dots.append((a * b).sum().item())
    assert abs(dots[0] - dots[1]) < 1e-10 and abs(dots[0] - dots[2]) < 1e-10


def test_rope_writes_the_interleaved_layout():
    """a one-hot x1[i] lands on elements 2i (cos) and 2i + 1 (sin); a one-hot x2[i] on 2i (-sin) and 2i + 1 (cos)"""
    h, i, t = 64, 5, 7.0
    angle = t / 10000.0 ** (2.0 * i / h)
    pos = torch.tensor([[t]], dtype=torch.float64)
    x = torch.zeros(1, 1, 1, h, dtype=torch.float64)
    x[..., i] = 1.0
    y = R.apply_rope(x, pos).reshape(h)
    want = torch.zeros(h, dtype=torch.float64)
    want[2 * i], want[2 * i + 1] = math.cos(angle), math.sin(angle)
    assert torch.allclose(y, want, atol=1e-14)
    x = torch.zeros(1, 1, 1, h, dtype=torch.float64)
    x[..., h // 2 + i] = 1.0
    y = R.apply_rope(x, pos).reshape(h)
    want = torch.zeros(h, dtype=torch.float64)
    want[2 * i], want[2 * i + 1] = -math.sin(angle), math.cos(angle)
    assert torch.allclose(y, want, atol=1e-14)


def test_a_query_row_sees_exactly_the_causal_unpadded_keys():
    """with v = one-hot(key index) the output row is the probability row: non-zero exactly where s <= t and the mask is 1"""
    B, T, h = 2, 6, 8
    pad = torch.tensor([[1, 1, 0, 1, 1, 0], [0, 0, 1, 1, 1, 1]])
    q, k = _rnd((B, T, 1, h), 5), _rnd((B, T, 1, h), 6)
    v = torch.eye(T, h, dtype=torch.float64)[None, :, None, :].expand(B, T, 1, h)
    out = R.attention_core(q, k, v, pad, 1, 1).reshape(B, T, h)
    for b in range(B):
        for t in range(T):
            seen = {s for s in range(T) if out[b, t, s] != 0}
            assert seen == {s for s in range(T) if s <= t and pad[b, s] != 0}, (b, t, seen)
            if seen:
                assert abs(out[b, t].sum().item() - 1.0) < 1e-12


def test_rows_without_a_visible_key_are_zero_and_pass_no_gradient():
    B, T, h = 1, 5, 8
    pad = torch.tensor([[0, 0, 1, 1, 1]])
    q, k, v = (_rnd((B, T, 2, h), s).requires_grad_(True) for s in (7, 8, 9))
    out = R.attention_core(q, k, v, pad, 2, 2)
    assert torch.equal(out[0, :2], torch.zeros(2, 2 * h, dtype=torch.float64)) and out[0, 2:].abs().min() > 0
    out.backward(torch.ones_like(out))
    assert torch.equal(q.grad[0, :2], torch.zeros_like(q.grad[0, :2]))
    assert torch.equal(k.grad[0, :2], torch.zeros_like(k.grad[0, :2])) and torch.equal(v.grad[0, :2], torch.zeros_like(v.grad[0, :2]))


def test_grouping_pairs_query_head_n_with_key_value_head_n_over_g():
    """nq = 4 on nkv = 2 equals plain attention with the key/value heads repeated as [0, 0, 1, 1]"""
    B, T, h = 1, 7, 8
    q, k, v = _rnd((B, T, 4, h), 10), _rnd((B, T, 2, h), 11), _rnd((B, T, 2, h), 12)
    grouped = R.attention_core(q, k, v, None, 4, 2)
    idx = torch.tensor([0, 0, 1, 1])
    plain = R.attention_core(q, k[:, :, idx], v[:, :, idx], None, 4, 4)
    assert torch.allclose(grouped, plain, rtol=1e-12, atol=1e-14)
    assert not torch.allclose(grouped, R.attention_core(q, k[:, :, [0, 1, 0, 1]], v[:, :, [0, 1, 0, 1]], None, 4, 4), atol=1e-3)


def test_preset_parameter_counts_from_shapes_alone():
    from iseg_amd.nlp.gemma.gemma_backbone import GemmaBackbone
    from iseg_amd.nlp.gemma.gemma_decoder_block import GemmaDecoderBlock

    assert GemmaBackbone.count_params(**GEMMA_2B) == 2_506_172_416
    assert GemmaBackbone.count_params(**GEMMA_7B) == 8_537_680_896
    per_block = [sum(math.prod(s) for _, s in GemmaDecoderBlock.weight_shapes(c["hidden_dim"], c["intermediate_dim"], c["head_dim"],
                                                                            c["num_query_heads"], c["num_key_value_heads"]))
                 for c in (GEMMA_2B, GEMMA_7B)]
    assert per_block == [110_104_576, 276_830_208]


def test_weight_names_and_shapes_of_a_tiny_configuration():
    """gemma_backbone.py:231-243"""
    from iseg_amd.nlp.gemma.gemma_backbone import GemmaBackbone

    want = [("token_embedding/embeddings", (97, 128))]
    for i in range(2):
        p = f"decoder_block_{i}/"
        want += [(p + "pre_attention_norm/scale", (128,)), (p + "attention/query/kernel", (4, 128, 64)), (p + "attention/key/kernel", (2, 128, 64)),
                 (p + "attention/value/kernel", (2, 128, 64)), (p + "attention/attention_output/kernel", (4, 64, 128)),
                 (p + "pre_ffw_norm/scale", (128,)), (p + "ffw_gating/kernel", (128, 256)), (p + "ffw_gating_2/kernel", (128, 256)),
                 (p + "ffw_linear/kernel", (256, 128))]
    want.append(("final_normalization/scale", (128,)))
    assert GemmaBackbone.weight_shapes(**TINY) == want
    model = GemmaBackbone(**TINY)
    model.build()
    got = sorted((p.iseg_name, tuple(p.shape)) for p in model.parameters())
    assert got == sorted(want)
    assert sum(p.numel() for p in model.parameters()) == GemmaBackbone.count_params(**TINY)


def test_the_kv_cache_and_the_other_unbuilt_parts_raise():
    from iseg_amd.nlp.gemma.gemma_attention import CachedGemmaAttention
    from iseg_amd.nlp.gemma.gemma_backbone import GemmaBackbone, ReversibleEmbedding
    from iseg_amd.nlp.gemma.gemma_decoder_block import GemmaDecoderBlock

    x = torch.zeros(1, 4, 128)
    with pytest.raises(NotImplementedError):
        GemmaDecoderBlock(128, 512, 64, 4, 2)(x, cache=torch.zeros(1, 2, 4, 2, 64))
    with pytest.raises(NotImplementedError):
        CachedGemmaAttention(64, 4, 2)(x, cache=torch.zeros(1, 2, 4, 2, 64), cache_update_index=0)
    with pytest.raises(NotImplementedError):
        CachedGemmaAttention(64, 4, 2)(x, cache_update_index=3)
    with pytest.raises(NotImplementedError):
        ReversibleEmbedding(11, 8, name="token_embedding")(torch.zeros(1, 2), reverse=True)
    with pytest.raises(NotImplementedError):
        GemmaBackbone.get_layout_map(None)
