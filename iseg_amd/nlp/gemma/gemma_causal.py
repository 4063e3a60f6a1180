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
GreedySampler, RandomSampler, TopKSampler, TopPSampler, BeamSampler, ContrastiveSampler.  The random ones choose each token with the fused kernels of
csrc/token_sample.hip from one uniform per row and step.  BeamSampler(num_beams=nb) expands the seeded [B, ...] cache to [B nb, ...] once
(call_with_cache does not care how large the batch is) and runs every step on the kernels of csrc/beam_search.hip: the selection reads the
logits once, the cache is reordered in place over its filled prefix (ISEG_BEAM_FUSED=0: the composed route in torch; nlp/samplers.py has the
algorithm and what it pins down beyond the reference).  generate_step returns the best beam; with return_all_beams=True it raises, because
the {"token_ids", "padding_mask"} contract has no beam axis: call the sampler directly.  ContrastiveSampler(k, alpha) is the one sampler that
reads hidden states: generate_step hands it the hidden states of the seeding pass (hidden_states=, which no other sampler is passed), and a
step runs on the kernels of csrc/contrastive.hip (ISEG_CONTRASTIVE_FUSED=0: the composed route; nlp/samplers.py has the algorithm): the cache
is repeated k times once and one position per step moves, so k caches stay resident for the loop.  Every other string alias, "beam" included, raises
NotImplementedError naming the classes.

compile(graph_decode=True) (off by default; no counterpart in the reference, whose tf.function plays this role) makes one generated token one
graph.replay().  The eager loop issues every launch of a step from Python and reads the stop condition on the host before each; here the loop's
state lives in device memory: the prompt, the mask, the position (one int32 that the _at launchers of csrc/gemma_decode.hip read when they run),
the token to embed and the per-row done flags, advanced by one launch of csrc/decode_commit.hip (F.decode_commit).  generate_step seeds the
cache eagerly into a buffer the graph owns, captures on first use of a signature (B, S, compute dtype, sampler type and kernel arguments,
prompt dtype; the end token is a frozen argument of the commit kernel, so each value has its graph) and replays S - index times.  The captured
kernels compute bit for bit what the eager ones do, so the tokens are the eager loop's.  The seeded samplers' uniforms are drawn outside the
graph, one launch in front of each replay, from the sampler's own generator: the eager loop's random stream for the same seed.  Without an end
token the loop reads nothing back.  With one it reads `done` every `check_every` replays (generate_step's keyword, default 16); the commit
kernel freezes once every row is done, so the result does not depend on check_every, but up to check_every - 1 frozen replays each draw
uniforms that the eager loop would not have drawn: the generator of a sampler that is reused afterwards is that far ahead.  A Sampler subclass
of the caller's keeps the eager loop (its get_next_token may read on the host), and so do BeamSampler (a captured beam step would need the
filled length in device memory) and ContrastiveSampler (likewise); the fp32 compute dtype, ISEG_GEMMA_FUSED=0 and an unsupported
head width raise ValueError (a captured step cannot take the composed route).  release_decode_graphs() drops graphs, caches and buffers.

Out of scope: the tokenizer and preprocessors (strings need a `preprocessor`, and none is built), presets, training
through the cache, paged caches."""
import math
import os

import torch

from ... import functional as F
from ... import nn
from ...nn import Layer
from ..samplers import BeamSampler, ContrastiveSampler, Sampler, sample_loop


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
        self.graph_decode = False
        self._decode_graphs = {}      # signature -> the captured step and the buffers it points into (_capture_decode_step)

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

    def compile(self, sampler="greedy", graph_decode=False, **unused):
        """sampler: "greedy", or an instance of iseg_amd.nlp.samplers (GreedySampler, RandomSampler, TopKSampler, TopPSampler, BeamSampler, ContrastiveSampler
        or a Sampler subclass of the caller's).  The other string aliases of keras_nlp.samplers.get are not built.
        graph_decode=True: generate_step replays every decoding step from one captured HIP graph (the module docstring); off by default."""
        if not isinstance(graph_decode, bool):
            raise ValueError(f"GemmaCausalLM.compile: graph_decode is True or False, got {graph_decode!r}")
        if isinstance(sampler, str):
            if sampler != "greedy":
                raise NotImplementedError(f'GemmaCausalLM.compile: the only string alias is "greedy", got {sampler!r}; pass an instance of '
                                          "iseg_amd.nlp.samplers.GreedySampler, RandomSampler, TopKSampler, TopPSampler or BeamSampler instead "
                                          "(or ContrastiveSampler)")
        elif not isinstance(sampler, Sampler):
            raise ValueError(f'GemmaCausalLM.compile: sampler is "greedy" or an iseg_amd.nlp.samplers.Sampler instance, got {sampler!r}')
        self.sampler = sampler
        self.graph_decode = graph_decode

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

    def _build_cache(self, token_ids, cache=None):
        """an empty cache for `token_ids` [B, S], seeded with one forward pass over the whole of it (:228-239) -> (hidden states, cache).
        cache: a buffer of the right shape to seed instead of a new one (every row of it is rewritten)"""
        bb = self.backbone
        B, S = token_ids.shape
        if cache is None:
            cache = torch.zeros((B, bb.num_layers, 2, S, bb.num_key_value_heads, bb.head_dim), dtype=nn.compute_dtype(), device=token_ids.device)
        _, hidden_states, cache = self.call_with_cache(token_ids, cache, 0)
        return hidden_states, cache

    # ---- the decode step as one replayed HIP graph (compile(graph_decode=True)) ---------------------------------------------------------------
    def _graph_decode_sampler(self):
        """the compiled sampler if a captured step may hold its token rule: "greedy" and the EXACT library classes.  A caller's subclass may read
        on the host in get_next_token, so it keeps the eager loop -> (eligible, sampler object or None for the string)"""
        from ..samplers import GreedySampler, RandomSampler, TopKSampler, TopPSampler

        if isinstance(self.sampler, str):
            return True, None
        return type(self.sampler) in (GreedySampler, RandomSampler, TopKSampler, TopPSampler), self.sampler

    def _require_fused_decode(self):
        """a captured step has no host position, so it runs on the fused decode kernels or not at all"""
        bb = self.backbone
        nq, nkv, h, dtype = bb.num_query_heads, bb.num_key_value_heads, bb.head_dim, nn.compute_dtype()
        if F.gemma_cached_attention_fused(1, nq, nkv, h, dtype):
            return
        if dtype != torch.bfloat16:
            why = f"the compute dtype is {dtype}, the decode kernels are bfloat16"
        elif os.environ.get("ISEG_GEMMA_FUSED", "1") == "0":
            why = "ISEG_GEMMA_FUSED=0 selects the composed route"
        else:
            why = f"head width {h} with {nq} query heads on {nkv} key/value heads is outside the decode kernels' supported set"
        raise ValueError(f"GemmaCausalLM.generate_step: graph_decode=True needs the fused decode kernels, but {why}; compile(graph_decode=False) "
                         "runs the eager loop")

    def _decode_entry(self, B, S, ids_dtype, sampler, device):
        """the device state of one signature, which the captured step points into: the cache, the loop's state (prompt, mask, pos, cur_ids, done),
        the uniform buffer of a seeded sampler and the sampler's token rule on it; `graphs` fills as end tokens are met (_decode_graph)"""
        bb = self.backbone
        e = dict(cache=torch.zeros((B, bb.num_layers, 2, S, bb.num_key_value_heads, bb.head_dim), dtype=nn.compute_dtype(), device=device),
                 prompt=torch.zeros((B, S), dtype=ids_dtype, device=device), mask=torch.zeros((B, S), dtype=torch.bool, device=device),
                 pos=torch.zeros(1, dtype=torch.int32, device=device), cur_ids=torch.zeros(B, dtype=ids_dtype, device=device),
                 done=torch.zeros(B, dtype=torch.bool, device=device),
                 uniforms=None if sampler is None or not hasattr(sampler, "uniforms_into") else torch.zeros(B, dtype=torch.float32, device=device),
                 graphs={})
        e["rule"] = _argmax if sampler is None else sampler.token_rule(e["uniforms"])
        return e

    def _decode_step(self, e, end_token_id):
        """one step on the entry's state: embed cur_ids, all blocks at pos, the final norm, the logits, the token rule, F.decode_commit"""
        logits, _, _ = self.call_with_cache(e["cur_ids"].view(-1, 1), e["cache"], e["pos"])
        F.decode_commit(e["prompt"], e["mask"], e["pos"], e["cur_ids"], e["done"], e["rule"](logits[:, 0]), end_token_id)

    def _decode_graph(self, e, end_token_id):
        """the graph of entry e for this end token (a host argument of the commit kernel, frozen at capture: one graph per value), captured on
        first use by GraphedCall's rules: a warm-up run on the capture stream (workspaces, keyed by stream, and lazy tables reach their final
        size; the decode workspace is the capacity's at every position) and a single stream, so the graph has no parallel branches.  Captured
        at position 0 on an all-zero state; generate_step overwrites the state before the first replay."""
        from ...graphs import GraphedCall

        key = -1 if end_token_id is None else int(end_token_id)
        generation = GraphedCall._refresh_derived_weights()
        if e["graphs"] and e["generation"] != generation:
            e["graphs"].clear()      # the buffers the captured launches point into were re-allocated: capture again
        graph = e["graphs"].get(key)
        if graph is None:
            for name in ("prompt", "mask", "pos", "cur_ids", "done"):
                e[name].zero_()
            side = torch.cuda.Stream(device=e["pos"].device)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side), torch.no_grad():
                self._decode_step(e, end_token_id)
            side.synchronize()
            e["pos"].zero_()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.no_grad(), torch.cuda.graph(graph, stream=side):
                self._decode_step(e, end_token_id)
            torch.cuda.current_stream().wait_stream(side)
            e["graphs"][key] = graph
            e["generation"] = GraphedCall._refresh_derived_weights()
        return graph

    def release_decode_graphs(self):
        """drop the captured decode graphs with their caches and state buffers; the next generate_step with graph_decode captures again"""
        self._decode_graphs.clear()

    @staticmethod
    def _graph_decode_start(token_ids, padding_mask, end_token_id):
        """(index, sticky) in ONE host read.  index: the first position to fill.  sticky: the commit kernel's `done`, which only ever turns on,
        follows sample_loop's, which is recomputed from the prompt at every step.  They part only where a row's end token at a non-user position
        is overwritten while the loop still runs; that cannot happen to a row that holds one in front of `index` (never rewritten) or at the
        last position (rewritten by the last step).  Zero padding that equals the end token is such a row.  Other prompts keep the eager loop."""
        S = token_ids.shape[1]
        index = padding_mask.to(torch.int32).sum(dim=-1).min()
        if end_token_id is None:
            return int(index.item()), True
        ends = (token_ids == end_token_id) & ~padding_mask
        cols = torch.arange(S, device=token_ids.device)
        ahead, behind = (ends & (cols >= index)).any(dim=-1), (ends & (cols < index)).any(dim=-1)
        sticky = (~ahead | ends[:, -1] | behind).all()
        index, sticky = torch.stack([index.to(torch.int64), sticky.to(torch.int64)]).tolist()
        return int(index), bool(sticky)

    def _generate_graphed(self, token_ids, padding_mask, index, end_token_id, sampler, check_every):
        """sample_loop with one graph.replay() per token: the state of the loop lives in the entry's device buffers"""
        B, S = token_ids.shape
        sig = (B, S, nn.compute_dtype(), ("greedy",) if sampler is None else sampler.graph_signature(), token_ids.dtype)
        e = self._decode_graphs.get(sig)
        if e is None:
            e = self._decode_graphs[sig] = self._decode_entry(B, S, token_ids.dtype, sampler, token_ids.device)
        graph = self._decode_graph(e, end_token_id)
        self._build_cache(token_ids, e["cache"])      # seeded eagerly, straight into the graph's own cache: no whole-cache copy
        e["prompt"].copy_(token_ids)
        e["mask"].copy_(padding_mask)
        e["pos"].fill_(index - 1)
        e["cur_ids"].copy_(token_ids[:, index - 1])
        if end_token_id is None:
            e["done"].zero_()
        else:
            e["done"].copy_(((token_ids == end_token_id) & ~padding_mask).any(dim=-1))
        draw = None if e["uniforms"] is None else sampler.uniforms_into
        self._replay_decode(graph, e, S - index, end_token_id is not None, draw, check_every)
        return e["prompt"].clone()

    @staticmethod
    def _replay_decode(graph, e, steps, with_end, draw, check_every):
        """`steps` replays, the step's uniforms drawn in front of each (one launch, outside the graph: the random stream is the eager loop's for
        the same seed).  Without an end token nothing is read back.  With one, `done` is read once every check_every replays (the position
        needs no read: it advances once per live replay and the host counts the replays) and the loop stops once every row is done; the
        replays since the commit kernel froze have changed nothing."""
        n = 0
        while n < steps:
            m = min(check_every, steps - n) if with_end else steps
            for _ in range(m):
                if draw is not None:
                    draw(e["uniforms"])
                graph.replay()
            n += m
            if with_end and n < steps and bool(e["done"].all()):
                break

    def generate_step(self, inputs, end_token_id=None, check_every=16):
        """one batch of {"token_ids" [B, S], "padding_mask" [B, S]} (true = user token) -> the same dictionary with the remaining positions filled
        by the compiled sampler, greedily by default (:241-314): generation starts at the shortest row's length; longer rows keep their own tokens there.
        check_every: with compile(graph_decode=True) and an end token, the number of replays between two host reads of the stop condition
        (16 is a choice, not a measurement); the result does not depend on it."""
        token_ids, padding_mask = inputs["token_ids"], inputs["padding_mask"].to(torch.bool)
        if isinstance(self.sampler, BeamSampler) and self.sampler.return_all_beams:
            raise ValueError('GemmaCausalLM.generate_step: the {"token_ids", "padding_mask"} result has no beam axis; with '
                             "BeamSampler(return_all_beams=True) call the sampler directly")
        if self.graph_decode:
            graphable, sampler = self._graph_decode_sampler()
            if graphable:
                if isinstance(check_every, bool) or not isinstance(check_every, int) or check_every < 1:
                    raise ValueError(f"GemmaCausalLM.generate_step: check_every is an integer >= 1, got {check_every!r}")
                if not self.built:
                    self.build()
                self._require_fused_decode()
                index, sticky = self._graph_decode_start(token_ids, padding_mask, end_token_id)
                if 1 <= index < token_ids.shape[1] and sticky:
                    out = self._generate_graphed(token_ids, padding_mask, index, end_token_id, sampler, check_every)
                    return {"token_ids": out, "padding_mask": generated_padding_mask(out, padding_mask, end_token_id)}
        hidden_states, cache = self._build_cache(token_ids)
        index = int(padding_mask.to(torch.int32).sum(dim=-1).min().item())

        def next(prompt, cache, index):
            # the cache index is the index of the previous token
            cache_update_index = index - 1
            logits, hidden_states, cache = self.call_with_cache(prompt[:, cache_update_index:cache_update_index + 1], cache, cache_update_index)
            return logits[:, 0], hidden_states[:, 0], cache

        if isinstance(self.sampler, ContrastiveSampler):      # the one sampler that reads hidden states; no other is passed them
            token_ids = self.sampler(next, token_ids, cache, index, padding_mask, end_token_id=end_token_id, hidden_states=hidden_states)
        elif isinstance(self.sampler, Sampler):
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
