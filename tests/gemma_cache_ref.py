"""fp64 torch restatement of the reference's cached Gemma call, line by line, on top of tests/gemma_ref.py: dynamic_update_slice and the cached
branch of CachedGemmaAttention.call (nlp/gemma/gemma_attention.py:161-201), compute_causal_mask(cache_index) as GemmaDecoderBlock uses it
(gemma_decoder_block.py:114-136), GemmaCausalLM.call_with_cache / _build_cache / generate_step (gemma_causal.py:186-314) and the greedy sampler
loop of keras_nlp's Sampler.__call__.  Test infrastructure only.

A layer's cache is [B, 2, S, nkv, h] and the model's [B, num_layers, 2, S, nkv, h], as in the reference; every function returns NEW caches, as the
reference does."""
import math

import torch

from tests import gemma_ref as R


def dynamic_update_slice(operand, update, start):
    """keras.ops.slice_update: a copy of `operand` with `update` written at the index vector `start`"""
    out = operand.clone()
    idx = tuple(slice(int(s), int(s) + n) for s, n in zip(start, update.shape))
    out[idx] = update
    return out


def compute_causal_mask(batch_size, input_length, output_length, cache_index=0):
    """keras_nlp transformer_layer_utils.compute_causal_mask: bool [B, output_length, input_length], row i (a new token at position
    cache_index + i) sees column j iff j <= cache_index + i"""
    i = torch.arange(output_length)[:, None] + int(cache_index)
    j = torch.arange(input_length)[None, :]
    return (i >= j)[None].expand(batch_size, output_length, input_length)


def cached_attention_core(q, key, value, cache_index, nq, nkv):
    """q [B, Tn, nq, h] (rotated), key / value [B, S, nkv, h]: the whole cache after the update -> [B, Tn, nq * h] (gemma_attention.py:185-195 under
    the mask of gemma_decoder_block.py:114-136 with a cache and no padding mask)"""
    B, Tn = q.shape[:2]
    mask = compute_causal_mask(B, key.shape[1], Tn, cache_index)
    return R.wipe(R.compute_attention(q, key, value, mask, nq, nkv), mask).reshape(B, Tn, -1)


def rope_cache(qkv, cache, cache_index, nq, nkv):
    """the projections' part of gemma_attention.py:161-179 on packed rows qkv [B, Tn, (nq + 2 nkv) h]: -> (rotated q [B, Tn, nq, h], new cache)"""
    B, Tn, _ = qkv.shape
    h = cache.shape[-1]
    positions = torch.arange(Tn, dtype=qkv.dtype)[None] + float(cache_index)
    q = R.apply_rope(qkv[..., :nq * h].reshape(B, Tn, nq, h), positions)
    k = R.apply_rope(qkv[..., nq * h:(nq + nkv) * h].reshape(B, Tn, nkv, h), positions)
    v = qkv[..., (nq + nkv) * h:].reshape(B, Tn, nkv, h)
    start = [0, int(cache_index), 0, 0]
    key = dynamic_update_slice(cache[:, 0], k, start)
    value = dynamic_update_slice(cache[:, 1], v, start)
    return q, torch.stack((key, value), dim=1)


def attention_with_cache(x, w, prefix, cache, cache_index, nq, nkv):
    """CachedGemmaAttention.call with a cache (gemma_attention.py:153-201) -> (output, new cache)"""
    q = torch.einsum("btd,ndh->btnh", x, w[prefix + "query/kernel"])
    k = torch.einsum("bsd,kdh->bskh", x, w[prefix + "key/kernel"])
    v = torch.einsum("bsd,kdh->bskh", x, w[prefix + "value/kernel"])
    B, Tn = x.shape[:2]
    qkv = torch.cat([q.reshape(B, Tn, -1), k.reshape(B, Tn, -1), v.reshape(B, Tn, -1)], dim=-1)
    q, cache = rope_cache(qkv, cache, cache_index, nq, nkv)
    vec = cached_attention_core(q, cache[:, 0], cache[:, 1], cache_index, nq, nkv).reshape(B, Tn, nq, -1)
    return torch.einsum("btnh,nhd->btd", vec, w[prefix + "attention_output/kernel"]), cache


def decoder_block_with_cache(x, w, prefix, cache, cache_index, nq, nkv, eps=1e-6):
    """GemmaDecoderBlock.call with a cache (gemma_decoder_block.py:139-178)"""
    normalized = R.rms_norm(x, w[prefix + "pre_attention_norm/scale"], eps)
    attention, cache = attention_with_cache(normalized, w, prefix + "attention/", cache, cache_index, nq, nkv)
    attention_x = x + attention
    normalized = R.rms_norm(attention_x, w[prefix + "pre_ffw_norm/scale"], eps)
    x1 = normalized @ w[prefix + "ffw_gating/kernel"]
    x2 = normalized @ w[prefix + "ffw_gating_2/kernel"]
    return (R.gelu_tanh(x1) * x2) @ w[prefix + "ffw_linear/kernel"] + attention_x, cache


def logits_of(hidden_states, w):
    """ReversibleEmbedding(reverse=True): hidden states against the transposed token table"""
    return hidden_states @ w["token_embedding/embeddings"].T


def causal_lm(token_ids, padding_mask, w, num_layers, nq, nkv, eps=1e-6, act_dtype=torch.float32):
    """GemmaCausalLM.__call__ (gemma_causal.py:156-158)"""
    return logits_of(R.backbone(token_ids, padding_mask, w, num_layers, nq, nkv, eps, act_dtype), w)


def call_with_cache(token_ids, cache, cache_index, w, num_layers, nq, nkv, eps=1e-6, act_dtype=torch.float32):
    """GemmaCausalLM.call_with_cache (gemma_causal.py:186-226) -> (logits, hidden states, new cache)"""
    table = w["token_embedding/embeddings"]
    x = table[token_ids.long()]
    x = x * float(torch.tensor(math.sqrt(float(table.shape[1])), dtype=torch.float32).to(act_dtype))
    caches = []
    for i in range(num_layers):
        x, next_cache = decoder_block_with_cache(x, w, f"decoder_block_{i}/", cache[:, i], cache_index, nq, nkv, eps)
        caches.append(next_cache)
    cache = torch.stack(caches, dim=1)
    hidden_states = R.rms_norm(x, w["final_normalization/scale"], eps)
    return logits_of(hidden_states, w), hidden_states, cache


def build_cache(token_ids, w, num_layers, nq, nkv, eps=1e-6, act_dtype=torch.float32):
    """GemmaCausalLM._build_cache (gemma_causal.py:228-239) -> (hidden states, cache)"""
    B, S = token_ids.shape
    h = w["decoder_block_0/attention/key/kernel"].shape[-1]
    cache = torch.zeros(B, num_layers, 2, S, nkv, h, dtype=torch.float64)
    _, hidden_states, cache = call_with_cache(token_ids, cache, 0, w, num_layers, nq, nkv, eps, act_dtype)
    return hidden_states, cache


def greedy_sampler(next, prompt, cache, index, mask, end_token_id=None):
    """keras_nlp Sampler.__call__ with the greedy get_next_token: the while_loop's cond and body"""
    prompt = prompt.clone()
    mask = mask.bool()
    max_length = prompt.shape[1]
    index = int(index)

    def cond(prompt, index):
        if end_token_id is None:
            return True
        end_tokens = (prompt == end_token_id) & ~mask
        prompt_done = end_tokens.any(dim=-1)
        return not bool(prompt_done.all())

    while index < max_length and cond(prompt, index):
        logits, _, cache = next(prompt, cache, index)
        next_token = torch.argmax(logits, dim=-1).to(prompt.dtype)
        next_token = torch.where(mask[:, index], prompt[:, index], next_token)
        prompt = dynamic_update_slice(prompt, next_token[:, None], [0, index])
        index += 1
    return prompt


def output_padding_mask(token_ids, padding_mask, end_token_id):
    """gemma_causal.py:294-310"""
    if end_token_id is None:
        return torch.ones_like(token_ids, dtype=torch.bool)
    end_locations = ((token_ids == end_token_id) & ~padding_mask.bool()).to(torch.int32)
    cumsum = torch.cumsum(end_locations, dim=-1).to(torch.int32)
    overflow = cumsum - end_locations
    return ~overflow.bool()


def generate_step(token_ids, padding_mask, w, num_layers, nq, nkv, end_token_id=None, eps=1e-6, act_dtype=torch.float32):
    """GemmaCausalLM.generate_step (gemma_causal.py:241-314) -> (token ids, padding mask)"""
    _, cache = build_cache(token_ids, w, num_layers, nq, nkv, eps, act_dtype)
    index = int(padding_mask.to(torch.int32).sum(dim=-1).min())

    def next(prompt, cache, index):
        cache_update_index = index - 1
        logits, hidden_states, cache = call_with_cache(prompt[:, cache_update_index:cache_update_index + 1], cache, cache_update_index, w, num_layers,
                                                       nq, nkv, eps, act_dtype)
        return logits[:, 0], hidden_states[:, 0], cache

    token_ids = greedy_sampler(next, token_ids, cache, index, padding_mask, end_token_id)
    return token_ids, output_padding_mask(token_ids, padding_mask, end_token_id)
