"""nlp/gemma/gemma_causal.py of the reference (GemmaCausalLM :19-444): the backbone with the tied embedding as the language-model head, the KV cache
and generation (greedy, or with a sampler of nlp/samplers.py).

    logits = model({"token_ids": [B, T], "padding_mask": [B, T]})                    (:156-158)  trainable: backbone + ReversibleEmbedding.logits
    logits, hidden_states, cache = model.call_with_cache(token_ids, cache, index)     (:186-226)  inference only
    out = model.generate_step({"token_ids", "padding_mask"}, end_token_id=None)        (:241-314)
    scores = model.score(token_ids, ..., scoring_mode="logits" | "loss")               (:316-444)
    loss = model.compute_loss(inputs, y, sample_weight)                                (:165-172, :103-118)  the compiled loss and metric of fit(x, y,
                                                                                       sample_weight) on the chunked head of nlp/lm_loss.py

The cache has the reference's shape [B, num_layers, 2, S, num_key_value_heads, head_dim] in the compute dtype.  call_with_cache hands each layer
its [B, 2, S, nkv, h] view, which the layer updates IN PLACE (F.gemma_rope_cache), and returns the same tensor; the reference stacks per-layer
copies into a new one.  Single-token steps run on the split-KV decode kernels of csrc/gemma_decode.hip; the seeding call (the whole prompt at
index 0) on the training kernels of csrc/gemma.hip.  No padding mask is passed on the cached path (the reference passes none).

compile(sampler=) takes "greedy" (the default: keras_nlp's greedy Sampler.__call__, `greedy_sample`) or an instance of nlp/samplers.py:
GreedySampler, RandomSampler, TopKSampler, TopPSampler.  The random ones choose each token with the fused kernels of csrc/token_sample.hip from
one uniform per row and step.  Every other string alias raises NotImplementedError naming the classes.

Out of scope: the tokenizer and preprocessors (strings need a `preprocessor`, and none is built), presets, beam and contrastive samplers, training
through the cache, HIP-graph replay of the decode step (the cache index is a host argument), paged caches."""
import math
import os

import torch

from ... import functional as F
from ... import nn
from ...nn import Layer
from ..samplers import Sampler, sample_loop


def lm_head_fused():
    """True where compute_loss takes the chunked head of nlp/lm_loss.py: ISEG_LMHEAD_FUSED unset or not "0" """
    return os.environ.get("ISEG_LMHEAD_FUSED", "1") != "0"


def _argmax(logits):
    return torch.argmax(logits, dim=-1)


def greedy_sample(next, prompt, cache, index, mask, end_token_id=None):
    """keras_nlp Sampler.__call__ with GreedySampler.get_next_token: while index < max_length, logits = next(prompt, cache, index)[0]; the argmax
    becomes the token at `index` unless mask[:, index] marks a user token, which is kept.  With an end_token_id the loop stops before a step
    once every row holds an end token at a position where `mask` is false; rows that are finished keep generating until all are.
    prompt [B, S] integers (a copy is returned), mask [B, S] bool, index: the first position to fill."""
    return sample_loop(_argmax, next, prompt, cache, index, mask, end_token_id=end_token_id)


def generated_padding_mask(token_ids, padding_mask, end_token_id):
    """the output mask of generate_step (:294-310): true up to and including the first end token that is not part of the prompt"""
    if end_token_id is None:
        return torch.ones_like(token_ids, dtype=torch.bool)
    end_locations = ((token_ids == end_token_id) & ~padding_mask.to(torch.bool)).to(torch.int32)
    overflow = torch.cumsum(end_locations, dim=-1).to(torch.int32) - end_locations
    return ~overflow.to(torch.bool)


class GemmaCausalLM(Layer):
    def __init__(self, backbone, preprocessor=None, name=None, **kwargs):
        super().__init__(name=name, **kwargs)
        self.backbone = backbone
        self.preprocessor = preprocessor
        self.sampler = "greedy"

    # ---- variables: the backbone's, the embedding is tied ---------------------------------------------------------------------------------
    @staticmethod
    def weight_shapes(**config):
        from .gemma_backbone import GemmaBackbone

        return GemmaBackbone.weight_shapes(**config)

    @classmethod
    def count_params(cls, **config):
        return sum(math.prod(s) for _, s in cls.weight_shapes(**config))

    def build(self, input_shape=None):
        if not self.backbone.built:
            self.backbone.build()
        self.built = True

    def compile(self, sampler="greedy", **unused):
        """sampler: "greedy", or an instance of iseg_amd.nlp.samplers (GreedySampler, RandomSampler, TopKSampler, TopPSampler or a Sampler subclass
        of the caller's).  The other string aliases of keras_nlp.samplers.get are not built."""
        if isinstance(sampler, str):
            if sampler != "greedy":
                raise NotImplementedError(f'GemmaCausalLM.compile: the only string alias is "greedy", got {sampler!r}; pass an instance of '
                                          "iseg_amd.nlp.samplers.GreedySampler, RandomSampler, TopKSampler or TopPSampler instead")
        elif not isinstance(sampler, Sampler):
            raise ValueError(f'GemmaCausalLM.compile: sampler is "greedy" or an iseg_amd.nlp.samplers.Sampler instance, got {sampler!r}')
        self.sampler = sampler

    # ---- the trainable forward (:156-158) ------------------------------------------------------------------------------------------------------
    def call(self, inputs, training=None):
        hidden_states = self.backbone(inputs, training=training)
        return self.backbone.token_embedding.logits(hidden_states)

    # ---- the training loss (:165-172 compile(), :103-118 fit(x, y, sample_weight)) ------------------------------------------------------------------
    def compute_loss(self, inputs, y, sample_weight=None, reduction="sum_over_batch_size", with_metrics=False, training=None):
        """SparseCategoricalCrossentropy(from_logits=True) of the model's logits against y [B, T] with sample_weight [B, T] (None: ones), as the
        reference's fit(x, y, sample_weight) computes it, on the chunked head of nlp/lm_loss.py: no [B, T, vocab] tensor exists.
        reduction: "sum_over_batch_size" (Keras: sum w l / (B T), divided by the element count, not by sum w), "sum", or "none" ([B, T] fp32).
        with_metrics: -> (loss, {"sparse_categorical_accuracy": sum w match / sum w}), SparseCategoricalAccuracy with sample weights (the argmax is
        the first maximal logit).  A target outside [0, vocab) counts as weight 0 in both.  ISEG_LMHEAD_FUSED=0 runs the composed route:
        embedding_logits, softmax_ce_per_pixel and torch's argmax on the stored logits; its loss kernel takes up to 256 classes and raises beyond."""
        if reduction not in ("sum_over_batch_size", "sum", "none"):
            raise ValueError(f'GemmaCausalLM.compute_loss: reduction is "sum_over_batch_size", "sum" or "none", got {reduction!r}')
        token_ids = inputs["token_ids"]
        if tuple(y.shape) != tuple(token_ids.shape):
            raise ValueError(f"GemmaCausalLM.compute_loss: y has the shape of token_ids {tuple(token_ids.shape)}, got {tuple(y.shape)}")
        if sample_weight is not None and tuple(sample_weight.shape) != tuple(y.shape):
            raise ValueError(f"GemmaCausalLM.compute_loss: sample_weight has the shape of y {tuple(y.shape)}, got {tuple(sample_weight.shape)}")
        hidden_states = self.backbone(inputs, training=training)
        table = self.backbone.token_embedding.embeddings
        vocab = table.shape[0]
        scale = 1.0 / max(y.numel(), 1) if reduction == "sum_over_batch_size" else 1.0
        if lm_head_fused():
            from .. import lm_loss

            loss, _, sums = lm_loss.lm_head_cross_entropy(hidden_states, table, y, sample_weight, upstream_scale=scale)
            accuracy = sums[1] / sums[2] if with_metrics and not nn.dry_run() else None
        else:
            logits = self.backbone.token_embedding.logits(hidden_states)
            if nn.dry_run():
                loss, accuracy = torch.empty(tuple(y.shape), dtype=torch.float32, device=logits.device), None
            else:
                valid = ((y >= 0) & (y < vocab)).to(torch.float32)
                w = valid if sample_weight is None else valid * sample_weight.to(torch.float32)
                labels = torch.where(valid.bool(), y, torch.full_like(y, -1))
                loss = F.softmax_ce_per_pixel(logits, labels, vocab, -1).reshape(y.shape) * (w * scale)
                accuracy = None
                if with_metrics:
                    accuracy = (w * (torch.argmax(logits.detach(), dim=-1) == y).to(torch.float32)).sum() / w.sum()
        if reduction != "none":
            loss = loss.sum()
        if not with_metrics:
            return loss
        if accuracy is None:
            accuracy = torch.empty((), dtype=torch.float32, device=loss.device)
        return loss, {"sparse_categorical_accuracy": accuracy}

    # ---- the cached forward (:186-226) ---------------------------------------------------------------------------------------------------------
    def call_with_cache(self, token_ids, cache, cache_update_index):
        """token_ids [B, Tn] at positions cache_update_index .. + Tn - 1; cache [B, num_layers, 2, S, nkv, h] -> (logits [B, Tn, vocab], hidden states
        [B, Tn, d], cache).  Inference only; the cache is updated in place and returned (the reference stacks new per-layer caches)."""
        bb = self.backbone
        if not self.built:
            self.build()
        if cache.dim() != 6 or cache.shape[1] != bb.num_layers:
            raise ValueError(f"GemmaCausalLM.call_with_cache: the cache is [B, {bb.num_layers}, 2, S, nkv, h], got {tuple(cache.shape)}")
        with torch.no_grad():
            x = bb.token_embedding(token_ids, scale=math.sqrt(float(bb.hidden_dim)))
            for i, layer in enumerate(bb.transformer_layers):
                x, _ = layer.call_with_cache(x, cache[:, i], cache_update_index)
            hidden_states = bb.layer_norm(x)
            return bb.token_embedding.logits(hidden_states), hidden_states, cache

    def _build_cache(self, token_ids):
        """an empty cache for `token_ids` [B, S], seeded with one forward pass over the whole of it (:228-239) -> (hidden states, cache)"""
        bb = self.backbone
        B, S = token_ids.shape
        cache = torch.zeros((B, bb.num_layers, 2, S, bb.num_key_value_heads, bb.head_dim), dtype=nn.compute_dtype(), device=token_ids.device)
        _, hidden_states, cache = self.call_with_cache(token_ids, cache, 0)
        return hidden_states, cache

    def generate_step(self, inputs, end_token_id=None):
        """one batch of {"token_ids" [B, S], "padding_mask" [B, S]} (true = user token) -> the same dictionary with the remaining positions filled
        by the compiled sampler, greedily by default (:241-314): generation starts at the shortest row's length; longer rows keep their own tokens there"""
        token_ids, padding_mask = inputs["token_ids"], inputs["padding_mask"].to(torch.bool)
        _, cache = self._build_cache(token_ids)
        index = int(padding_mask.to(torch.int32).sum(dim=-1).min().item())

        def next(prompt, cache, index):
            # the cache index is the index of the previous token
            cache_update_index = index - 1
            logits, hidden_states, cache = self.call_with_cache(prompt[:, cache_update_index:cache_update_index + 1], cache, cache_update_index)
            return logits[:, 0], hidden_states[:, 0], cache

        if isinstance(self.sampler, Sampler):
            token_ids = self.sampler(next, token_ids, cache, index, padding_mask, end_token_id=end_token_id)
        else:
            token_ids = greedy_sample(next, token_ids, cache, index, padding_mask, end_token_id=end_token_id)
        return {"token_ids": token_ids, "padding_mask": generated_padding_mask(token_ids, padding_mask, end_token_id)}

    def generate(self, inputs, max_length=None):
        """the {"token_ids", "padding_mask"} dictionary, cut or zero-padded to max_length positions, through generate_step.  Anything else (strings)
        goes through `preprocessor.generate_preprocess` and stops at its tokenizer's end token; none is built here, and without one it raises"""
        end_token_id = None
        if not (isinstance(inputs, dict) and "token_ids" in inputs and "padding_mask" in inputs):
            if self.preprocessor is None:
                raise ValueError('GemmaCausalLM.generate: without a preprocessor the input is a {"token_ids", "padding_mask"} dictionary')
            inputs = self.preprocessor.generate_preprocess(inputs, sequence_length=max_length)
            end_token_id = self.preprocessor.tokenizer.end_token_id
        token_ids, padding_mask = inputs["token_ids"], inputs["padding_mask"].to(torch.bool)
        if max_length is not None and int(max_length) != token_ids.shape[1]:
            S = int(max_length)
            ids = torch.zeros((token_ids.shape[0], S), dtype=token_ids.dtype, device=token_ids.device)
            pad = torch.zeros((token_ids.shape[0], S), dtype=torch.bool, device=token_ids.device)
            n = min(S, token_ids.shape[1])
            ids[:, :n], pad[:, :n] = token_ids[:, :n], padding_mask[:, :n]
            token_ids, padding_mask = ids, pad
        return self.generate_step({"token_ids": token_ids, "padding_mask": padding_mask}, end_token_id=end_token_id)

    # ---- scoring (:316-444) --------------------------------------------------------------------------------------------------------------------
    def score(self, token_ids, padding_mask=None, scoring_mode="logits", layer_intercept_fn=None, target_ids=None):
        """per-token scores: "logits" [B, T, vocab], or "loss" [B, T] = the sparse cross-entropy of the logits against target_ids (fp32, nothing
        ignored).  layer_intercept_fn(x, i) sees and may replace the activations after block i; for i = -1 it is shown the unscaled embeddings and,
        as in the reference (:425-430), what it returns for them is not used."""
        if scoring_mode not in ("logits", "loss"):
            raise ValueError("Unsupported scoring_mode. Must be one of 'logits' or 'loss'.")
        if scoring_mode == "loss" and target_ids is None:
            raise ValueError("Cannot compute loss without targets. Please provide target token ids via the target_ids parameter.")
        if token_ids.dim() != 2:
            raise ValueError(f"GemmaCausalLM.score: token_ids is [batch_size, num_tokens], got {tuple(token_ids.shape)}")
        bb = self.backbone
        if not self.built:
            self.build()
        if padding_mask is None:
            padding_mask = torch.ones(token_ids.shape, dtype=torch.int32, device=token_ids.device)
        if layer_intercept_fn is not None:
            layer_intercept_fn(bb.token_embedding(token_ids), -1)
        x = bb.token_embedding(token_ids, scale=math.sqrt(float(bb.hidden_dim)))
        for i, layer in enumerate(bb.transformer_layers):
            x = layer(x, padding_mask=padding_mask)
            if layer_intercept_fn is not None:
                x = layer_intercept_fn(x, i)
        logits = bb.token_embedding.logits(bb.layer_norm(x))
        if scoring_mode == "logits":
            return logits
        vocab = logits.shape[-1]
        return F.softmax_ce_per_pixel(logits, target_ids, vocab, -1).reshape(token_ids.shape)
