"""nlp/gemma/gemma_decoder_block.py of the reference (GemmaDecoderBlock :29-178): pre-norm attention and pre-norm GeGLU feed-forward, each with a
residual connection:
    a = x + attention(pre_attention_norm(x))                                                        (:146-166)
    y = a + (gelu_tanh(n W_gating) * (n W_gating_2)) W_linear,   n = pre_ffw_norm(a)                  (:167-174)
ffw_gating/kernel and ffw_gating_2/kernel are [d, intermediate_dim // 2], ffw_linear/kernel [intermediate_dim // 2, d]; no biases.  The gated
product is iseg_glu_fwd / _bwd with ISEG_ACT_GELU_TANH.  Dropout (default 0): on the attention probabilities (gemma_attention.py:145-148) and on
the attention output (:163-164); the reference also constructs `feedforward_dropout` (:68) and never calls it, and so it is here.

The KV cache has an entry point of its own, `call_with_cache(x, cache, cache_update_index)` (inference only); the `cache=` /
`cache_update_index=` keywords of `call` raise NotImplementedError and name it."""
import torch

from ... import functional as F
from ...nn import Layer
from .gemma_attention import CachedGemmaAttention
from .rms_normalization import RMSNormalization


class GemmaDecoderBlock(Layer):
    def __init__(self, hidden_dim, intermediate_dim, head_dim, num_query_heads, num_key_value_heads, layer_norm_epsilon=1e-6, dropout=0, name=None,
                 **kwargs):
        super().__init__(name=name, **kwargs)
        self.hidden_dim, self.intermediate_dim, self.head_dim = int(hidden_dim), int(intermediate_dim), int(head_dim)
        self.num_query_heads, self.num_key_value_heads = int(num_query_heads), int(num_key_value_heads)
        self.layer_norm_epsilon, self.dropout = float(layer_norm_epsilon), float(dropout)
        self.pre_attention_norm = RMSNormalization(epsilon=self.layer_norm_epsilon, name=f"{self.name}/pre_attention_norm")
        self.attention = CachedGemmaAttention(head_dim=head_dim, num_query_heads=num_query_heads, num_key_value_heads=num_key_value_heads,
                                              dropout=dropout, name=f"{self.name}/attention")
        self.pre_ffw_norm = RMSNormalization(epsilon=self.layer_norm_epsilon, name=f"{self.name}/pre_ffw_norm")

    @staticmethod
    def weight_shapes(hidden_dim, intermediate_dim, head_dim, num_query_heads, num_key_value_heads):
        """(name, shape) of the block's variables in the reference's order (gemma_backbone.py:235-243), nothing allocated"""
        half = intermediate_dim // 2
        attn = CachedGemmaAttention.weight_shapes(hidden_dim, head_dim, num_query_heads, num_key_value_heads)
        return ([("pre_attention_norm/scale", (hidden_dim,))] + [("attention/" + n, s) for n, s in attn] +
                [("pre_ffw_norm/scale", (hidden_dim,)), ("ffw_gating/kernel", (hidden_dim, half)), ("ffw_gating_2/kernel", (hidden_dim, half)),
                 ("ffw_linear/kernel", (half, hidden_dim))])

    def build(self, input_shape):
        shape = (None, None, self.hidden_dim)
        self.pre_attention_norm.build(shape)
        self.attention.build(shape)
        self.pre_ffw_norm.build(shape)
        half = self.intermediate_dim // 2
        self.add_weight("ffw_gating/kernel", (self.hidden_dim, half), "glorot_uniform")
        self.add_weight("ffw_gating_2/kernel", (self.hidden_dim, half), "glorot_uniform")
        self.add_weight("ffw_linear/kernel", (half, self.hidden_dim), "glorot_uniform")
        self.built = True

    def call(self, x, padding_mask=None, cache=None, cache_update_index=0, training=None):
        if cache is not None or cache_update_index:
            raise NotImplementedError("GemmaDecoderBlock: call() takes no KV cache (cache=, cache_update_index); use call_with_cache(x, cache, "
                                      "cache_update_index)")
        x, skip = F.fork(x)
        attention = self.attention(self.pre_attention_norm(x), padding_mask=padding_mask, training=training)
        attention = F.dropout(attention, self.dropout, bool(training))
        attention_x = F.add(skip, attention)
        a, skip = F.fork(attention_x)
        normalized, normalized_2 = F.fork(self.pre_ffw_norm(a))
        x1 = F.dense(normalized, self.ffw_gating_kernel)
        x2 = F.dense(normalized_2, self.ffw_gating_2_kernel)
        y = F.dense(F.glu(x1, x2, "gelu_tanh"), self.ffw_linear_kernel)
        return F.add(y, skip)

    def call_with_cache(self, x, cache, cache_update_index):
        """GemmaDecoderBlock.call with a cache (:139-178): x [B, Tn, d] at positions cache_update_index .., cache [B, 2, S, nkv, h] -> (x, cache).
        Inference only, no dropout, no padding mask.  The cache is updated IN PLACE and the same tensor is returned; the reference returns a new one."""
        if not self.built:
            raise RuntimeError("GemmaDecoderBlock.call_with_cache: build the layer first (one uncached call)")
        with torch.no_grad():
            attention, cache = self.attention.call_with_cache(self.pre_attention_norm(x), cache, cache_update_index)
            attention_x = F.add(x, attention)
            normalized = self.pre_ffw_norm(attention_x)
            x1 = F.dense(normalized, self.ffw_gating_kernel)
            x2 = F.dense(normalized, self.ffw_gating_2_kernel)
            y = F.dense(F.glu(x1, x2, "gelu_tanh"), self.ffw_linear_kernel)
            return F.add(y, attention_x), cache
