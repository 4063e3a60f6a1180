"""nlp/gemma/gemma_backbone.py of the reference (GemmaBackbone :32-193): token embedding scaled by sqrt(hidden_dim) rounded to the activation
type (:152-153), `num_layers` decoder blocks (:154-155), a final RMS normalisation (:156).  Called with {"token_ids": [B, T] integers (or
floats holding integers, as the reference's Input declares), "padding_mask": [B, T], non-zero = real token}; returns the final hidden states
[B, T, hidden_dim] in the compute dtype.  Variable names are the reference's (:231-243): token_embedding/embeddings,
decoder_block_{i}/..., final_normalization/scale.

The reverse (logits) use of the tied embedding is `ReversibleEmbedding.logits(x)` (F.embedding_logits); the `reverse=True` keyword of its `call`
raises NotImplementedError and names it.  The KV cache, GemmaCausalLM and generation are in gemma_causal.py.

Out of scope: the tokenizer and preprocessors, presets and their download, and get_layout_map (raises NotImplementedError)."""
import math

import torch

from ... import functional as F
from ... import nn
from ...nn import Layer
from .gemma_decoder_block import GemmaDecoderBlock
from .rms_normalization import RMSNormalization


def _embedding_init(name):
    """keras VarianceScaling(scale=1.0, mode="fan_in", distribution="untruncated_normal") (:117-122); fan_in of a [vocab, d] table is vocab"""
    def init(shape):
        return torch.randn(shape, generator=nn._gen(name)) * math.sqrt(1.0 / shape[0])
    return init


class ReversibleEmbedding(Layer):
    """the token table of :113-125: `call` is the lookup, `logits` the reverse use x @ embeddings^T (one parameter, both gradients add up on it)"""

    def __init__(self, input_dim, output_dim, name=None, **kwargs):
        super().__init__(name=name, **kwargs)
        self.input_dim, self.output_dim = int(input_dim), int(output_dim)

    def build(self, input_shape=None):
        self.add_weight("embeddings", (self.input_dim, self.output_dim), _embedding_init(f"{self.name}/embeddings"))
        self.built = True

    def call(self, token_ids, reverse=False, scale=1.0, training=None):
        if reverse:
            raise NotImplementedError("ReversibleEmbedding: call() has no reverse use; the logits of the tied embedding are logits(x)")
        return F.embedding(token_ids, self.embeddings, scale)

    def logits(self, x):
        """x [B, T, output_dim] -> [B, T, input_dim] = x @ embeddings^T (ReversibleEmbedding(reverse=True), gemma_causal.py:158)"""
        if not self.built:
            self.build()
        return F.embedding_logits(x, self.embeddings)


class GemmaBackbone(Layer):
    def __init__(self, vocabulary_size, num_layers, num_query_heads, num_key_value_heads, hidden_dim, intermediate_dim, head_dim,
                 layer_norm_epsilon=1e-6, dropout=0, name=None, **kwargs):
        super().__init__(name=name, **kwargs)
        self.vocabulary_size, self.num_layers = int(vocabulary_size), int(num_layers)
        self.num_query_heads, self.num_key_value_heads = int(num_query_heads), int(num_key_value_heads)
        self.hidden_dim, self.intermediate_dim, self.head_dim = int(hidden_dim), int(intermediate_dim), int(head_dim)
        self.layer_norm_epsilon, self.dropout = float(layer_norm_epsilon), float(dropout)
        self.token_embedding = ReversibleEmbedding(self.vocabulary_size, self.hidden_dim, name="token_embedding")
        self.transformer_layers = torch.nn.ModuleList([
            GemmaDecoderBlock(intermediate_dim=intermediate_dim, hidden_dim=hidden_dim, num_query_heads=num_query_heads, head_dim=head_dim,
                              num_key_value_heads=num_key_value_heads, layer_norm_epsilon=layer_norm_epsilon, dropout=dropout,
                              name=f"decoder_block_{i}") for i in range(self.num_layers)])
        self.layer_norm = RMSNormalization(epsilon=self.layer_norm_epsilon, name="final_normalization")

    @staticmethod
    def weight_shapes(vocabulary_size, num_layers, num_query_heads, num_key_value_heads, hidden_dim, intermediate_dim, head_dim, **unused):
        """[(name, shape)] of every variable in creation order, from shape arithmetic alone: nothing is allocated, so the preset sizes
        (gemma_presets.py) can be checked without the memory for them"""
        block = GemmaDecoderBlock.weight_shapes(hidden_dim, intermediate_dim, head_dim, num_query_heads, num_key_value_heads)
        out = [("token_embedding/embeddings", (vocabulary_size, hidden_dim))]
        for i in range(num_layers):
            out += [(f"decoder_block_{i}/{n}", s) for n, s in block]
        return out + [("final_normalization/scale", (hidden_dim,))]

    @classmethod
    def count_params(cls, **config):
        return sum(math.prod(s) for _, s in cls.weight_shapes(**config))

    def get_config(self):
        return {k: getattr(self, k) for k in ("vocabulary_size", "num_layers", "num_query_heads", "num_key_value_heads", "hidden_dim",
                                              "intermediate_dim", "head_dim", "layer_norm_epsilon", "dropout")}

    @staticmethod
    def get_layout_map(device_mesh, model_parallel_dim_name="model"):
        raise NotImplementedError("GemmaBackbone.get_layout_map: model-parallel layouts are not built")

    def build(self, input_shape=None):
        self.token_embedding.build()
        shape = (None, None, self.hidden_dim)
        for layer in self.transformer_layers:
            layer.build(shape)
            layer.built = True
        self.layer_norm.build(shape)
        self.token_embedding.built = self.layer_norm.built = True
        self.built = True

    def call(self, inputs, training=None):
        token_ids, padding_mask = inputs["token_ids"], inputs.get("padding_mask")
        x = self.token_embedding(token_ids, scale=math.sqrt(float(self.hidden_dim)))
        for layer in self.transformer_layers:
            x = layer(x, padding_mask=padding_mask, training=training)
        return self.layer_norm(x)
