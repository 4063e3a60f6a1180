"""Gemma with a key/value cache, CPU side: the fp64 restatement of the cached call (tests/gemma_cache_ref.py) against the uncached one
(tests/gemma_ref.py), the greedy sampler's semantics on a stub model -- the restatement's loop and the library's, which must agree --, the
output padding mask, the new entry points and the tied parameter list of GemmaCausalLM."""
import math

import pytest
import torch

from tests import gemma_cache_ref as C
from tests import gemma_ref as R
from tests.test_gemma_host import GEMMA_2B, GEMMA_7B, TINY


def tiny_weights(cfg, seed):
    """fp64 weights of a configuration: kernels ~ N(0, fan_in^-0.5), norm scales ~ 0.1 N(0, 1), embedding std 0.02"""
    from iseg_amd.nlp.gemma.gemma_backbone import GemmaBackbone

    gen = torch.Generator().manual_seed(seed)
    w = {}
    for name, shape in GemmaBackbone.weight_shapes(**cfg):
        t = torch.randn(shape, generator=gen, dtype=torch.float64)
        if name.endswith("scale"):
            t = 0.1 * t
        elif name.endswith("embeddings"):
            t = 0.02 * t
        else:
            fan_in = shape[1] if len(shape) == 3 and "attention_output" not in name else shape[0] if len(shape) == 2 else shape[0] * shape[1]
            t = t / math.sqrt(fan_in)
        w[name] = t
    return w


def _geom(cfg):
    return cfg["num_layers"], cfg["num_query_heads"], cfg["num_key_value_heads"]


def test_stepping_through_the_cache_reproduces_the_uncached_rows():
    """seed the cache with prompts of length 5 and 9 in a sequence of 20 (the rest of the row holds token 0), then feed the final sequence token
    by token from index 5: every step's hidden state and logits equal the uncached backbone's row of the final sequence to 1e-10 -- also at the
    positions whose cache rows still held the seeding pass's stale keys, which the causal mask with a cache index hides"""
    B, S = 2, 20
    w = tiny_weights(TINY, 3)
    L, nq, nkv = _geom(TINY)
    final = torch.randint(1, TINY["vocabulary_size"], (B, S), generator=torch.Generator().manual_seed(4))
    seed_ids = final.clone()
    seed_ids[0, 5:] = 0
    seed_ids[1, 9:] = 0
    want_hidden = R.backbone(final, None, w, L, nq, nkv, act_dtype=torch.float64)
    want_logits = C.causal_lm(final, None, w, L, nq, nkv, act_dtype=torch.float64)
    hidden, cache = C.build_cache(seed_ids, w, L, nq, nkv, act_dtype=torch.float64)
    assert tuple(cache.shape) == (B, L, 2, S, nkv, TINY["head_dim"])
    # the seeding pass itself is the uncached forward of what it was given: rows below the prompt lengths are already final
    assert (hidden[0, :5] - want_hidden[0, :5]).abs().max().item() < 1e-10 and (hidden[1, :9] - want_hidden[1, :9]).abs().max().item() < 1e-10
    assert (hidden[0, 5:] - want_hidden[0, 5:]).abs().max().item() > 1e-3      # and the stale tail is not
    for i in range(5, S):
        stale = cache.clone()
        logits, hid, cache = C.call_with_cache(final[:, i:i + 1], cache, i, w, L, nq, nkv, act_dtype=torch.float64)
        assert (hid[:, 0] - want_hidden[:, i]).abs().max().item() < 1e-10, i
        assert (logits[:, 0] - want_logits[:, i]).abs().max().item() < 1e-10, i
        # dynamic_update_slice: only row i of every layer's keys and values changed
        changed = (cache != stale).any(dim=-1).any(dim=-1)      # [B, L, 2, S]
        assert not changed[..., :i].any() and not changed[..., i + 1:].any()


def test_causal_mask_with_a_cache_index():
    m = C.compute_causal_mask(2, 6, 2, 3)
    assert tuple(m.shape) == (2, 2, 6)
    assert m[0].tolist() == [[True, True, True, True, False, False], [True, True, True, True, True, False]]
    assert torch.equal(C.compute_causal_mask(1, 5, 5, 0)[0], torch.ones(5, 5, dtype=torch.bool).tril())


def _stub(script):
    """a `next` whose argmax at step `index` is script[index][row]; records the indices it was asked for"""
    seen = []

    def next(prompt, cache, index):
        seen.append(index)
        logits = torch.zeros(prompt.shape[0], 11)
        for b, tok in enumerate(script[index]):
            logits[b, tok] = 1.0
        return logits, None, cache

    return next, seen


@pytest.mark.parametrize("which", ["restatement", "library"])
def test_sampler_semantics_on_a_stub(which):
    """rows of prompt length 2 and 4 in a sequence of 8, end token 9.  The loop starts at index 2; row 1's own tokens at positions 2 and 3 survive the
    argmax; row 0 emits the end token at position 3 and keeps generating until row 1 emits one at position 6: the step at index 7 is not taken"""
    from iseg_amd.nlp.gemma.gemma_causal import generated_padding_mask, greedy_sample

    sampler = C.greedy_sampler if which == "restatement" else greedy_sample
    prompt = torch.tensor([[1, 2, 0, 0, 0, 0, 0, 0], [3, 4, 5, 9, 0, 0, 0, 0]])      # row 1's prompt holds the end token: it does not count
    mask = torch.tensor([[1, 1, 0, 0, 0, 0, 0, 0], [1, 1, 1, 1, 0, 0, 0, 0]], dtype=torch.bool)
    script = {2: (7, 7), 3: (9, 7), 4: (6, 8), 5: (6, 8), 6: (5, 9), 7: (1, 1)}
    nxt, seen = _stub(script)
    out = sampler(nxt, prompt, None, 2, mask, end_token_id=9)
    assert seen == [2, 3, 4, 5, 6]
    assert out.tolist() == [[1, 2, 7, 9, 6, 6, 5, 0], [3, 4, 5, 9, 8, 8, 9, 0]]
    assert prompt[0, 2].item() == 0      # the caller's tensor is not written
    want_mask = [[True, True, True, True, False, False, False, False], [True] * 7 + [False]]
    assert C.output_padding_mask(out, mask, 9).tolist() == want_mask
    assert generated_padding_mask(out, mask, 9).tolist() == want_mask
    # without an end token every position is filled and the mask is all ones
    nxt, seen = _stub(script)
    out = sampler(nxt, prompt, None, 2, mask)
    assert seen == [2, 3, 4, 5, 6, 7] and out[:, 7].tolist() == [1, 1]
    assert C.output_padding_mask(out, mask, None).all() and generated_padding_mask(out, mask, None).all()


def test_the_new_entry_points_exist_and_the_refusals_name_them():
    from iseg_amd import _hip
    from iseg_amd import functional as F
    from iseg_amd import kernels as K
    from iseg_amd.nlp.gemma import GemmaCausalLM
    from iseg_amd.nlp.gemma.gemma_attention import CachedGemmaAttention
    from iseg_amd.nlp.gemma.gemma_backbone import ReversibleEmbedding
    from iseg_amd.nlp.gemma.gemma_decoder_block import GemmaDecoderBlock

    for name in ("iseg_gemma_rope_cache", "iseg_gemma_decode_attention", "iseg_gemma_decode_attention_supported",
                 "iseg_gemma_decode_attention_splits", "iseg_gemma_decode_attention_scratch_bytes"):
        assert name in _hip.SIGNATURES
    for mod, names in ((F, ("gemma_rope_cache", "gemma_cached_attention_core", "embedding_logits")),
                       (K, ("gemma_rope_cache", "gemma_decode_attention", "gemma_decode_attention_supported", "gemma_decode_attention_splits")),
                       (GemmaCausalLM, ("call_with_cache", "_build_cache", "generate_step", "generate", "score", "compile")),
                       (CachedGemmaAttention, ("call_with_cache",)), (GemmaDecoderBlock, ("call_with_cache",)), (ReversibleEmbedding, ("logits",))):
        for n in names:
            assert callable(getattr(mod, n)), (mod, n)
    x = torch.zeros(1, 4, 128)
    with pytest.raises(NotImplementedError, match="call_with_cache"):
        GemmaDecoderBlock(128, 512, 64, 4, 2)(x, cache=torch.zeros(1, 2, 4, 2, 64))
    with pytest.raises(NotImplementedError, match="call_with_cache"):
        CachedGemmaAttention(64, 4, 2)(x, cache_update_index=3)
    with pytest.raises(NotImplementedError, match="logits"):
        ReversibleEmbedding(11, 8, name="token_embedding")(torch.zeros(1, 2), reverse=True)


def test_the_plan_is_a_function_of_the_arguments_and_clips():
    """no device needed: the chunk plan and the scratch size are host arithmetic"""
    from iseg_amd import _hip

    L = _hip.lib()
    assert L.iseg_gemma_decode_attention_splits(1, 4000, 1, 8, 1, 256) > 1
    assert L.iseg_gemma_decode_attention_splits(1, 0, 1, 8, 1, 256) == 1 and L.iseg_gemma_decode_attention_splits(1, 63, 1, 8, 1, 256) == 1
    assert L.iseg_gemma_decode_attention_splits(1, 4000, 1, 8, 1, 256) == L.iseg_gemma_decode_attention_splits(1, 4000, 1, 8, 1, 256)
    # many (sample, kv head) groups already cover the chip: fewer chunks each
    assert L.iseg_gemma_decode_attention_splits(64, 4000, 1, 16, 16, 256) < L.iseg_gemma_decode_attention_splits(1, 4000, 1, 16, 16, 256)
    partial = (32 + 16 * 256) * 4      # m[16] | l[16] | 16 rows of 256 accumulators, fp32
    assert L.iseg_gemma_decode_attention_scratch_bytes(1, 127, 2, 8, 1, 256, 3) == 3 * partial
    assert L.iseg_gemma_decode_attention_scratch_bytes(1, 127, 2, 8, 1, 256, 99) == 3 * partial      # clipped to the three tiles with a visible key
    assert L.iseg_gemma_decode_attention_scratch_bytes(1, 127, 2, 8, 1, 256, 0) == \
        L.iseg_gemma_decode_attention_splits(1, 127, 2, 8, 1, 256) * partial
    assert L.iseg_gemma_decode_attention_supported(1, 8, 1, 256, _hip.BF16) == 1 and L.iseg_gemma_decode_attention_supported(2, 8, 1, 256, _hip.BF16) == 1
    assert L.iseg_gemma_decode_attention_supported(3, 8, 1, 256, _hip.BF16) == 0 and L.iseg_gemma_decode_attention_supported(1, 8, 1, 96, _hip.BF16) == 0
    assert L.iseg_gemma_decode_attention_supported(1, 8, 1, 256, _hip.F32) == 0 and L.iseg_gemma_decode_attention_supported(1, 4, 3, 64, _hip.BF16) == 0


def test_causal_lm_has_the_backbones_variables_and_a_tied_embedding():
    from iseg_amd.nlp.gemma import GemmaBackbone, GemmaCausalLM

    for cfg in (GEMMA_2B, GEMMA_7B, TINY):
        assert GemmaCausalLM.weight_shapes(**cfg) == GemmaBackbone.weight_shapes(**cfg)
        assert GemmaCausalLM.count_params(**cfg) == GemmaBackbone.count_params(**cfg)
    backbone = GemmaBackbone(**TINY)
    model = GemmaCausalLM(backbone)
    model.build()
    assert [id(p) for p in model.parameters()] == [id(p) for p in backbone.parameters()]
    assert sum(p.numel() for p in model.parameters()) == GemmaCausalLM.count_params(**TINY)
    assert sum(1 for p in model.parameters() if p.iseg_name == "token_embedding/embeddings") == 1
    with pytest.raises(NotImplementedError):
        model.compile(sampler="top_k")
    model.compile(sampler="greedy")
    with pytest.raises(ValueError):
        model.generate(["a string"])
    with pytest.raises(ValueError):
        model.score(torch.zeros(1, 3, dtype=torch.int64), scoring_mode="probabilities")
    with pytest.raises(ValueError):
        model.score(torch.zeros(1, 3, dtype=torch.int64), scoring_mode="loss")
