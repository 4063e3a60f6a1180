"""keras_nlp.samplers as GemmaCausalLM.compile(sampler=) takes them (the class docstring of nlp/gemma/gemma_causal.py in the reference): the decoding
loop of Sampler.__call__, the greedy, random, top-k and top-p rules for the next token, beam search and contrastive search.  Defaults are
keras_nlp's.

    sampler = TopKSampler(k=5, seed=7)
    model.compile(sampler=sampler)
    out = model.generate({"token_ids": ..., "padding_mask": ...})

The loop (`sample_loop`) is the one greedy_sample of gemma_causal.py has always run; a subclass supplies get_next_token(logits) alone.  The random
samplers draw one uniform per row and step from a torch.Generator they own (made on the logits' device at first use, seeded with `seed`, or
from the library's seed stream when seed is None) and hand it with the logits to F.sample_tokens: the fused kernels of csrc/token_sample.hip.
The same seed, prompt and weights give the same tokens; the random stream itself is torch's, not the reference's.

For the decode step replayed from a captured graph (GemmaCausalLM.compile(graph_decode=True)) the library's own classes also give
graph_signature() (what a capture freezes of the sampler: its type and kernel arguments), token_rule(uniforms) (get_next_token as a function of
the logits alone, reading its uniforms from a static buffer) and, the seeded ones, uniforms_into(buf) (the step's draw of `uniforms`, written
into that buffer in front of each replay).  sample_loop and the classes' behaviour are unchanged.

BeamSampler(num_beams=5, return_all_beams=False, temperature=1.0) restates keras_nlp's BeamSampler.__call__; it is no get_next_token rule, because a
beam step carries running scores and reorders the cache.  Every prompt row becomes num_beams rows (row b nb + j is beam j of batch row b) with
fp32 running scores [0, -1e9, ..., -1e9], so that the first step extends beam 0 alone.  A step scores every (beam, token) pair with
log softmax(logits / temperature) + the beam's running score, keeps the nb best per batch row (F.beam_select), gathers prompt and cache by
the chosen parents and writes the chosen tokens except over user tokens (F.beam_reorder); the running score keeps the selected candidate's
value even where a user token overrides its token, as in the reference.  The loop stops as sample_loop does, over all B nb rows.  On device
tensors both halves are kernels of csrc/beam_search.hip: the logits are read once and no [B nb, V] tensor is made, and the cache is reordered
in place over its filled prefix only; CPU tensors and ISEG_BEAM_FUSED=0 take the composed route, the reference's op sequence in torch.
Where the reference leaves the result open it is pinned down (include/iseg_hip.h has the full statement):
  order      the selected beams come out sorted by score descending, ties by flat index (beam V + token) ascending;
  scores     (x - max) / T - log sum exp is evaluated directly: where an fp32 softmax underflows to 0 the reference gets -inf and an
             arbitrary order, here such candidates keep their true value and place;
  non-finite a -inf logit scores -inf; a NaN or +inf logit makes its row's scores NaN; NaN ranks above every number, as in torch.topk;
             0 <= parent < nb and 0 <= token < V always.

ContrastiveSampler(k=5, alpha=0.5, temperature=1.0) restates keras_nlp's ContrastiveSampler.__call__ (contrastive search: the token that is
probable AND whose hidden state is unlike every earlier one, which is what stops the repetition loops of greedy and beam search).  It is the
one sampler that reads hidden states: it is called with hidden_states=[B, S, D], the final-norm output of every prompt position, and uses
the second result of next().  One call of next on the B rows gives the first logits; then the cache is repeated k times ONCE (row b k + j is
candidate j of batch row b) and every step
  takes the k most probable tokens of softmax(logits / temperature) as candidates (F.contrastive_candidates; a user token at `index` replaces
  all k), writes them at `index` of the B k rows and calls next at index + 1 on them: the candidates' logits, hidden states and cache rows;
  scores candidate j with (1 - alpha) p_j - alpha max_t cos(hidden_states[b, t], its hidden state), t < index, and picks the first maximal
  score (F.contrastive_select);
  makes the winner's token, hidden state and cache position the group's (F.contrastive_commit) and reads the winner's row of the candidates'
  logits as the next step's logits (the row map of F.contrastive_candidates).
The loop stops as sample_loop does.  On device tensors the three halves are kernels of csrc/contrastive.hip: no [B, V] probability tensor, no
[B k, index] similarity matrix, and after the first repeat only ONE cache position per step moves, where the reference copies the whole cache
k times and gathers it back every step.  The price is that k caches stay resident for the whole loop; the reference holds the same amount
transiently in every step.  CPU tensors, unsupported shapes and ISEG_CONTRASTIVE_FUSED=0 take the composed route, the reference's op sequence
in torch.  Pinned down beyond the reference (include/iseg_hip.h has the full statement):
  candidates probability descending, ties by token id ascending (the reference's top_k(sorted=False) has no order);
  winner     the first maximal score in that order; NaN ranks above every number, as in torch.argmax;
  precision  probabilities and scores are fp32 (the reference rounds the probabilities to the logits' dtype); dot products and norms
             accumulate in fp32; no epsilon: a zero hidden state gives NaN, as in the reference;
  range      0 <= token < V and 0 <= winner < k always.

Out of scope: the string aliases ("top_k", ...) of keras_nlp.samplers.get."""
import math

import torch

from .. import functional as F


def sample_loop(get_next_token, next, prompt, cache, index, mask, end_token_id=None):
    """keras_nlp Sampler.__call__: while index < max_length, logits = next(prompt, cache, index)[0]; get_next_token(logits) becomes the token at
    `index` unless mask[:, index] marks a user token, which is kept.  With an end_token_id the loop stops before a step once every row holds an
    end token at a position where `mask` is false; rows that are finished keep generating until all are.
    prompt [B, S] integers (a copy is returned), mask [B, S] bool, index: the first position to fill."""
    prompt = prompt.clone()
    mask = mask.to(torch.bool)
    max_length = prompt.shape[1]
    index = int(index)
    while index < max_length:
        if end_token_id is not None:
            done = ((prompt == end_token_id) & ~mask).any(dim=-1)
            if bool(done.all()):
                break
        logits, _, cache = next(prompt, cache, index)
        token = get_next_token(logits).to(prompt.dtype)
        prompt[:, index] = torch.where(mask[:, index], prompt[:, index], token)
        index += 1
    return prompt


def _check_temperature(temperature):
    temperature = float(temperature)
    if not (temperature > 0.0 and math.isfinite(temperature)):
        raise ValueError(f"Sampler: temperature must be positive and finite, got {temperature}")
    return temperature


class Sampler:
    """the base class: the loop, and the temperature every subclass carries.  get_next_token(logits [B, V]) -> token ids [B]"""

    def __init__(self, temperature=1.0):
        self.temperature = _check_temperature(temperature)

    def __call__(self, next, prompt, cache=None, index=0, mask=None, end_token_id=None):
        if mask is None:
            mask = torch.zeros_like(prompt, dtype=torch.bool)
        return sample_loop(self.get_next_token, next, prompt, cache, index, mask, end_token_id=end_token_id)

    def get_next_token(self, logits):
        raise NotImplementedError(f"{type(self).__name__}.get_next_token: a sampler defines how the next token is chosen")

    def get_config(self):
        return {"temperature": self.temperature}

    @classmethod
    def from_config(cls, config):
        return cls(**config)


class GreedySampler(Sampler):
    """the most probable token: torch.argmax, the path GemmaCausalLM has always taken (the temperature does not change an argmax)"""

    def get_next_token(self, logits):
        return torch.argmax(logits, dim=-1)

    def graph_signature(self):
        return (type(self).__name__,)

    def token_rule(self, uniforms=None):
        """get_next_token as a function of the logits alone, free of this object's state: what a captured decode step records"""
        return lambda logits: torch.argmax(logits, dim=-1)


class _SeededSampler(Sampler):
    mode = None

    def __init__(self, seed=None, temperature=1.0):
        super().__init__(temperature)
        if seed is not None and (isinstance(seed, bool) or not isinstance(seed, int)):
            raise ValueError(f"{type(self).__name__}: seed is an integer or None, got {seed!r}")
        self.seed = seed
        self._generator = None

    def _generator_on(self, device):
        if self._generator is None or self._generator.device != device:
            self._generator = torch.Generator(device=device)
            self._generator.manual_seed((self.seed if self.seed is not None else F.next_seed()) & 0x7FFFFFFFFFFFFFFF)
        return self._generator

    def uniforms(self, logits):
        """fp32 [B] in [0, 1): one draw per row from this sampler's own generator"""
        return torch.rand(logits.shape[0], generator=self._generator_on(logits.device), device=logits.device, dtype=torch.float32)

    def uniforms_into(self, buf):
        """this step's draw of `uniforms`, written into buf (fp32 [B], contiguous, on the device): the same generator and the same stream of numbers,
        one launch, no allocation -- the buffer a captured decode step reads its uniforms from"""
        if buf.dtype != torch.float32 or buf.dim() != 1 or not buf.is_contiguous():
            raise ValueError(f"{type(self).__name__}.uniforms_into: the buffer is a contiguous float32 [B], got {tuple(buf.shape)} {buf.dtype}")
        return torch.rand(buf.shape[0], generator=self._generator_on(buf.device), out=buf)

    def _kernel_args(self):
        return {}

    def graph_signature(self):
        """what a captured decode step freezes of this sampler: its type and the kernel's arguments (not the seed: the uniforms come from outside)"""
        return (type(self).__name__, self.mode, self.temperature) + tuple(sorted(self._kernel_args().items()))

    def token_rule(self, uniforms):
        """get_next_token as a function of the logits alone, reading the step's uniforms from the static buffer `uniforms` (fp32 [B], filled by
        uniforms_into in front of each step) and free of this object's state: what a captured decode step records"""
        mode, temperature, args = self.mode, self.temperature, dict(self._kernel_args())
        return lambda logits: F.sample_tokens(logits, uniforms, mode=mode, temperature=temperature, **args)

    def get_next_token(self, logits):
        return F.sample_tokens(logits, self.uniforms(logits), mode=self.mode, temperature=self.temperature, **self._kernel_args())

    def get_config(self):
        return {**super().get_config(), "seed": self.seed}


class RandomSampler(_SeededSampler):
    """a draw from softmax(logits / temperature) over the whole vocabulary"""
    mode = "random"


class TopKSampler(_SeededSampler):
    """a draw from softmax(logits / temperature) over the k largest logits (ties by index)"""
    mode = "top_k"

    def __init__(self, k=5, seed=None, temperature=1.0):
        super().__init__(seed, temperature)
        if isinstance(k, bool) or not isinstance(k, int) or k < 1:
            raise ValueError(f"TopKSampler: k is an integer >= 1, got {k!r}")
        self.k = k

    def _kernel_args(self):
        return {"k": self.k}

    def get_config(self):
        return {**super().get_config(), "k": self.k}


class TopPSampler(_SeededSampler):
    """a draw from softmax(logits / temperature) over the most probable tokens whose preceding probability mass is <= p, optionally looking at the
    k largest alone (k = None: the whole vocabulary)"""
    mode = "top_p"

    def __init__(self, p=0.1, k=None, seed=None, temperature=1.0):
        super().__init__(seed, temperature)
        p = float(p)
        if not 0.0 < p <= 1.0:
            raise ValueError(f"TopPSampler: p must lie in (0, 1], got {p}")
        if k is not None and (isinstance(k, bool) or not isinstance(k, int) or k < 1):
            raise ValueError(f"TopPSampler: k is an integer >= 1 or None, got {k!r}")
        self.p, self.k = p, k

    def _kernel_args(self):
        return {"p": self.p, "k": self.k or 0}

    def get_config(self):
        return {**super().get_config(), "p": self.p, "k": self.k}


class BeamSampler(Sampler):
    """beam search: num_beams hypotheses per prompt row, extended jointly; the result is the hypothesis with the largest sum of token
    log-probabilities (the first of equals), or with return_all_beams=True the pair (prompts [B, nb, S], log_probs [B, nb]) sorted by score
    descending.  num_beams is an integer in 1 .. 16; num_beams=1 is greedy search on logits without ties.  The module docstring has the
    algorithm, the two routes and what is pinned down beyond the reference."""

    def __init__(self, num_beams=5, return_all_beams=False, temperature=1.0):
        super().__init__(temperature)
        if isinstance(num_beams, bool) or not isinstance(num_beams, int) or not 1 <= num_beams <= F.BEAM_MAX_BEAMS:
            raise ValueError(f"BeamSampler: num_beams is an integer in 1 .. {F.BEAM_MAX_BEAMS}, got {num_beams!r}")
        if not isinstance(return_all_beams, bool):
            raise ValueError(f"BeamSampler: return_all_beams is True or False, got {return_all_beams!r}")
        self.num_beams, self.return_all_beams = num_beams, return_all_beams

    def __call__(self, next, prompt, cache=None, index=0, mask=None, end_token_id=None):
        """next(prompt [B nb, S], cache, index) -> (logits [B nb, V], hidden states, cache), as sample_loop calls it.  cache: None or a tensor
        whose axis 0 is the batch, in call_with_cache's convention [B, L, 2, S, nkv, h] with step `index` writing position index - 1."""
        nb = self.num_beams
        if prompt.dim() != 2:
            raise ValueError(f"BeamSampler: prompt is [B, S], got {tuple(prompt.shape)}")
        if mask is None:
            mask = torch.zeros_like(prompt, dtype=torch.bool)
        if cache is not None and not torch.is_tensor(cache):
            raise ValueError(f"BeamSampler: the cache is a tensor with the batch on axis 0 or None, got {type(cache).__name__}")
        B, S = prompt.shape
        # copies, num_beams to a row: the caller's tensors are never written
        prompt = torch.repeat_interleave(prompt, nb, dim=0)
        mask = torch.repeat_interleave(mask.to(torch.bool), nb, dim=0)
        if cache is not None:
            cache = torch.repeat_interleave(cache, nb, dim=0)
        log_probs = torch.tensor([0.0] + [-1e9] * (nb - 1), dtype=torch.float32, device=prompt.device).repeat(B)
        index = int(index)
        while index < S:
            if end_token_id is not None:
                done = ((prompt == end_token_id) & ~mask).any(dim=-1)
                if bool(done.all()):
                    break
            logits, _, cache = next(prompt, cache, index)
            parents, tokens, log_probs = F.beam_select(logits, log_probs, nb, self.temperature)
            cache, prompt = F.beam_reorder(cache, prompt, mask, parents, tokens, index, nb)
            index += 1
        prompts, log_probs = prompt.view(B, nb, S), log_probs.view(B, nb)
        if self.return_all_beams:
            order = torch.sort(log_probs, dim=-1, descending=True, stable=True).indices
            return prompts.gather(1, order[:, :, None].expand(-1, -1, S)), log_probs.gather(1, order)
        best = torch.argmax(log_probs, dim=-1)      # the first of equal maxima
        return prompts[torch.arange(B, device=prompt.device), best]

    def get_next_token(self, logits):
        raise NotImplementedError("BeamSampler.get_next_token: a beam step needs the running scores and reorders the cache; call the sampler")

    def get_config(self):
        return {**super().get_config(), "num_beams": self.num_beams, "return_all_beams": self.return_all_beams}


class ContrastiveSampler(Sampler):
    """contrastive search: per step the k most probable tokens are candidates, and the one with the largest
    (1 - alpha) probability - alpha (largest cosine similarity of its hidden state to an earlier position's) becomes the token.  k is an integer
    in 1 .. 16 (k = 1 is greedy search), 0 <= alpha <= 1 (alpha = 0 is greedy search on logits without ties).  k caches stay resident for the
    whole loop (the reference holds as much transiently in every step).  The module docstring has the algorithm, the two routes and what is
    pinned down beyond the reference."""

    def __init__(self, k=5, alpha=0.5, temperature=1.0):
        super().__init__(temperature)
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= F.CONTRASTIVE_MAX_K:
            raise ValueError(f"ContrastiveSampler: k is an integer in 1 .. {F.CONTRASTIVE_MAX_K}, got {k!r}")
        if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not 0.0 <= float(alpha) <= 1.0:
            raise ValueError(f"ContrastiveSampler: 0 <= alpha <= 1, got {alpha!r}")
        self.k, self.alpha = k, float(alpha)

    def __call__(self, next, prompt, cache=None, index=0, mask=None, end_token_id=None, hidden_states=None):
        """next(prompt [rows, S], cache, index) -> (logits [rows, V], hidden states [rows, D], cache) for the token at index - 1, as sample_loop
        calls it, on B or B k rows.  hidden_states [B, S, D]: the hidden states of the prompt's positions (those below `index` are read).
        cache: None or a tensor whose axis 0 is the batch, in call_with_cache's convention [B, L, 2, S, nkv, h] with step `index` writing
        position index - 1.  The caller's prompt, cache and hidden_states are never written."""
        k = self.k
        if hidden_states is None:
            raise ValueError("ContrastiveSampler: contrastive search compares hidden states; pass hidden_states=[B, S, D], the hidden state of "
                             "every prompt position (GemmaCausalLM.generate_step does)")
        if prompt.dim() != 2:
            raise ValueError(f"ContrastiveSampler: prompt is [B, S], got {tuple(prompt.shape)}")
        B, S = prompt.shape
        if hidden_states.dim() != 3 or hidden_states.shape[0] != B or hidden_states.shape[1] < S:
            raise ValueError(f"ContrastiveSampler: hidden_states is [{B}, {S}, D], got {tuple(hidden_states.shape)}")
        if mask is None:
            mask = torch.zeros_like(prompt, dtype=torch.bool)
        if cache is not None and not torch.is_tensor(cache):
            raise ValueError(f"ContrastiveSampler: the cache is a tensor with the batch on axis 0 or None, got {type(cache).__name__}")
        mask = mask.to(torch.bool)
        index = int(index)
        if index >= S:
            return prompt.clone()
        if index < 1:
            raise ValueError("ContrastiveSampler: the first step needs a previous position (index >= 1)")
        history = hidden_states.detach().clone()
        # the one step on B rows, on a copy of the cache; then k rows to a row, once
        logits, _, cache = next(prompt, None if cache is None else cache.clone(), index)
        prompt = torch.repeat_interleave(prompt, k, dim=0)
        if cache is not None:
            cache = torch.repeat_interleave(cache, k, dim=0)
        row_map = None
        while index < S:
            if end_token_id is not None:
                done = ((prompt[::k] == end_token_id) & ~mask).any(dim=-1)
                if bool(done.all()):
                    break
            probs, tokens = F.contrastive_candidates(logits, k, self.temperature, row_map)
            user = mask[:, index, None]
            tokens = torch.where(user, prompt[::k, index, None], tokens.to(prompt.dtype))
            prompt[:, index] = tokens.reshape(-1)
            next_logits, cand_hidden, cache = next(prompt, cache, index + 1)
            winner, _, _ = F.contrastive_select(history, index, cand_hidden, probs.reshape(-1), self.alpha)
            cache, prompt, history = F.contrastive_commit(cache, prompt, history, cand_hidden, winner, index, k)
            logits, row_map = next_logits, winner
            index += 1
        return prompt[::k].clone()

    def get_next_token(self, logits):
        raise NotImplementedError("ContrastiveSampler.get_next_token: a contrastive step reads the candidates' hidden states; call the sampler")

    def get_config(self):
        return {**super().get_config(), "k": self.k, "alpha": self.alpha}
