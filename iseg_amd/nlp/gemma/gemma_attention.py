"""nlp/gemma/gemma_attention.py of the reference (CachedGemmaAttention :24-201): grouped-query attention with rotary position embedding.

Projections (:50-91) keep the reference's parameter shapes, so weights load by name: query/kernel [nq, d, h], key/kernel and value/kernel [nkv, d, h],
attention_output/kernel [nq, h, d]; no biases.  q, k and v are written by strided-batch GEMMs into ONE packed [B, T, (nq + 2 nkv) h] buffer, the
rotary embedding (:96-114, interleaved output, fp32 angles -- DESIGN.md) turns its q and k columns, and F.gemma_attention_core (:116-151, and
the wipe of rows without an attended token :189-195) reads column ranges of it.  The attention mask is not an argument: it is always the causal
mask merged with the key padding mask (gemma_decoder_block.py:114-136), which the core builds from `padding_mask`.

The KV cache (:161-179) has an entry point of its own, `call_with_cache(x, cache, cache_update_index)`: inference only, on
F.gemma_rope_cache (rotary embedding at the positions cache_update_index + t, written straight into the cache) and F.gemma_cached_attention_core
(the split-KV decode kernels of csrc/gemma_decode.hip).  The `cache=` / `cache_update_index=` keywords of `call` raise NotImplementedError and
name it."""
import torch

from ... import functional as F
from ...nn import Layer


class CachedGemmaAttention(Layer):
    def __init__(self, head_dim, num_query_heads, num_key_value_heads, kernel_initializer="glorot_uniform", dropout=0, name=None, **kwargs):
        super().__init__(name=name, **kwargs)
        self.head_dim, self.num_query_heads, self.num_key_value_heads = int(head_dim), int(num_query_heads), int(num_key_value_heads)
        if self.num_query_heads % self.num_key_value_heads:
            raise ValueError("CachedGemmaAttention: num_query_heads must be a multiple of num_key_value_heads")
        self.dropout = float(dropout)
        self.kernel_initializer = kernel_initializer
        self.num_key_value_groups = self.num_query_heads // self.num_key_value_heads      # (:45)

    @staticmethod
    def weight_shapes(hidden_dim, head_dim, num_query_heads, num_key_value_heads):
        """(name, shape) of the layer's variables in creation order (gemma_backbone.py:236-239), nothing allocated"""
        return [("query/kernel", (num_query_heads, hidden_dim, head_dim)), ("key/kernel", (num_key_value_heads, hidden_dim, head_dim)),
                ("value/kernel", (num_key_value_heads, hidden_dim, head_dim)), ("attention_output/kernel", (num_query_heads, head_dim, hidden_dim))]

    def build(self, input_shape):
        self.hidden_dim = int(input_shape[-1])
        for name, shape in self.weight_shapes(self.hidden_dim, self.head_dim, self.num_query_heads, self.num_key_value_heads):
            self.add_weight(name, shape, self.kernel_initializer)
        self.built = True

    def call(self, x, padding_mask=None, cache=None, cache_update_index=0, training=None):
        if cache is not None or cache_update_index:
            raise NotImplementedError("CachedGemmaAttention: call() takes no KV cache (cache=, cache_update_index); use call_with_cache(x, cache, "
                                      "cache_update_index)")
        nq, nkv, h = self.num_query_heads, self.num_key_value_heads, self.head_dim
        qkv = F.gemma_qkv(x, self.query_kernel, self.key_kernel, self.value_kernel)
        qkv = F.gemma_rope(qkv, nq, nkv, h)
        y = F.gemma_attention_core(qkv, padding_mask, nq, nkv, h, dropout_rate=self.dropout, training=bool(training))
        return F.dense(y, self.attention_output_kernel, kshape=(nq * h, self.hidden_dim))      # "btnh,nhd->btd" (:82-91)

    def call_with_cache(self, x, cache, cache_update_index):
        """x [B, Tn, d]: the tokens at positions cache_update_index .. + Tn - 1; cache [B, 2, S, nkv, h]: this layer's keys and values -> (out, cache)
        (:161-201 with a cache; the mask is compute_causal_mask(cache_index) alone, no padding mask).  Inference only.  The cache is updated IN
        PLACE and the same tensor is returned; the reference builds a new one (dynamic_update_slice, tf.stack)."""
        if not self.built:
            raise RuntimeError("CachedGemmaAttention.call_with_cache: build the layer first (one uncached call)")
        nq, nkv, h = self.num_query_heads, self.num_key_value_heads, self.head_dim
        with torch.no_grad():
            qkv = F.gemma_qkv(x, self.query_kernel, self.key_kernel, self.value_kernel)
            # a one-element int32 device tensor (the replayed decode step) is passed through unchanged; anything else is a host integer, as ever
            on_device = torch.is_tensor(cache_update_index) and cache_update_index.is_cuda and cache_update_index.dtype == torch.int32
            index = cache_update_index if on_device else int(cache_update_index)
            q = F.gemma_rope_cache(qkv, cache, index, nq, nkv, h)
            y = F.gemma_cached_attention_core(q, cache, index, nq, nkv, h)
            return F.dense(y, self.attention_output_kernel, kshape=(nq * h, self.hidden_dim)), cache
