"""fp64 oracle of one contrastive-search step and of the whole loop, written from the statement in include/iseg_hip.h and
iseg_amd/nlp/samplers.py (no library code): the candidates of a row from the STORED logits, the similarities, scores and margins of a selection
from the STORED hidden states, the acceptance rules, the composed broadcast of a commit, and keras_nlp's ContrastiveSampler.__call__ replayed
over a caller-supplied `next`.  Row b k + j is candidate j of batch row b.

Tolerances (derived, not measured).  An fp32 dot product of D terms in any order is off by at most D 2^-24 sum |h_i c_i| <= D 2^-24 |h| |c|
(Cauchy-Schwarz); the two norms together add as much again; square roots, the product and the division a few units of 2^-24:
    eps_sim(D) = (2 D + 8) 2^-24                                      absolute, on a quantity in [-1, 1]
A probability is within 3 units of 2^-23 of itself (the weight-and-sum derivation at the head of tests/test_beam_search_gpu.py), so
    eps_score(alpha, D) = (1 - alpha) 3 2^-23 + alpha eps_sim(D) + 2^-23     (p <= 1; the last term: the score's own roundings)."""
import numpy as np
import torch

ULP = 2.0 ** -23
PROB_UNITS = 3.0
TINY = 2.0 ** -149      # the spacing of fp32 below its smallest normal: a probability down there has no relative precision to keep


def eps_sim(D):
    return (2.0 * D + 8.0) * 2.0 ** -24


def eps_score(alpha, D):
    return (1.0 - alpha) * PROB_UNITS * ULP + alpha * eps_sim(D) + ULP


# ---- candidates -----------------------------------------------------------------------------------------------------------------------------
def probabilities(logits, T, row_map=None):
    """logits [R, V] (the stored values) -> fp64 [B, V] softmax(x / T) of every output row (row b g + row_map[b] with a map).  NaN throughout
    for a row whose largest entry is NaN or +inf or that holds -inf alone"""
    x = logits.detach().cpu().double().numpy()
    if row_map is not None:
        m = row_map.cpu().numpy().astype(np.int64)
        g = x.shape[0] // m.shape[0]
        x = x[np.arange(m.shape[0]) * g + m]
    with np.errstate(all="ignore"):
        t = (x - x.max(axis=1, keepdims=True)) / float(T)
        e = np.exp(t)
        return e / e.sum(axis=1, keepdims=True)


def candidates_accepted(probs, tokens, logits, k, T, row_map=None, units=PROB_UNITS):
    """-> (complaints, worst error in units of 2^-23 relative).  With p the oracle probabilities of an output row:
      * tokens in [0, V) and distinct; a NaN row: the tokens 0 .. k - 1 and NaN probabilities;
      * each returned probability within `units` 2^-23 of p[token], relative (plus 2^-149, the fp32 spacing where p is subnormal);
      * position r holds the oracle's r-th token (p descending, ties by id) wherever p there differs from its neighbours in the order by more
        than the tolerance; otherwise its p is within the tolerance of the oracle's r-th;
      * where two neighbouring returned tokens have equal STORED logits, the lower id comes first."""
    p = probabilities(logits, T, row_map)
    x = logits.detach().cpu().double().numpy()
    if row_map is not None:
        m = row_map.cpu().numpy().astype(np.int64)
        x = x[np.arange(m.shape[0]) * (x.shape[0] // m.shape[0]) + m]
    B, V = p.shape
    got_p = probs.detach().cpu().double().numpy().reshape(B, k)
    got_t = tokens.cpu().numpy().astype(np.int64).reshape(B, k)
    bad, worst = [], 0.0
    for b in range(B):
        t = got_t[b]
        if not ((t >= 0) & (t < V)).all() or len(set(t.tolist())) != k:
            bad.append(f"row {b}: tokens out of range or repeated: {t.tolist()}")
            continue
        if np.isnan(p[b]).any():
            if t.tolist() != list(range(k)) or not np.isnan(got_p[b]).all():
                bad.append(f"row {b}: a NaN row gives the first k tokens and NaN, got {t.tolist()} {got_p[b].tolist()}")
            continue
        order = np.lexsort((np.arange(V), -p[b]))[:k + 1]
        for r in range(k):
            want = p[b, order[r]]
            tol = units * ULP * want + TINY
            err = abs(got_p[b, r] - p[b, t[r]])
            if p[b, t[r]] > 2.0 ** -126:
                worst = max(worst, err / (ULP * p[b, t[r]]))
            if err > units * ULP * p[b, t[r]] + TINY:
                bad.append(f"row {b} rank {r}: probability {got_p[b, r]!r} of token {t[r]}, oracle {p[b, t[r]]!r}")
            above = p[b, order[r - 1]] if r else np.inf
            below = p[b, order[r + 1]] if r + 1 < len(order) else -np.inf
            if above - want > 2 * tol and want - below > 2 * tol:
                if t[r] != order[r]:
                    bad.append(f"row {b} rank {r}: token {t[r]}, the oracle's is {order[r]} by a clear margin")
            elif abs(p[b, t[r]] - want) > 2 * tol:
                bad.append(f"row {b} rank {r}: token {t[r]} with p {p[b, t[r]]!r} is not the rank's {want!r}")
            if r and x[b, t[r]] == x[b, t[r - 1]] and t[r] < t[r - 1]:
                bad.append(f"row {b} ranks {r - 1}, {r}: equal logits out of token order: {t[r - 1]}, {t[r]}")
            if r and x[b, t[r]] > x[b, t[r - 1]]:
                bad.append(f"row {b} ranks {r - 1}, {r}: logits ascend")
    return bad, worst


# ---- select ---------------------------------------------------------------------------------------------------------------------------------
def similarities(hidden_states, index, cand_hidden, k):
    """-> fp64 [B k, index]: <h_t, c> / (|h_t| |c|) from the stored values; 0 / 0 = NaN"""
    h = hidden_states.detach().cpu().double().numpy()[:, :index]
    B, D = h.shape[0], h.shape[2]
    c = cand_hidden.detach().cpu().double().numpy().reshape(B, k, D)
    with np.errstate(all="ignore"):
        dot = np.einsum("btd,bkd->bkt", h, c)
        sim = dot / (np.sqrt((h * h).sum(-1))[:, None, :] * np.sqrt((c * c).sum(-1))[:, :, None])
    return sim.reshape(B * k, index)


def step(hidden_states, index, cand_hidden, probs, alpha, k):
    """-> (max_sim fp64 [B k], scores fp64 [B k], winner [B]); NaN propagates through the maximum and ranks above every number"""
    sim = similarities(hidden_states, index, cand_hidden, k)
    with np.errstate(all="ignore"):
        max_sim = np.where(np.isnan(sim).any(axis=1), np.nan, np.nanmax(np.where(np.isnan(sim), -np.inf, sim), axis=1))
        scores = (1.0 - alpha) * probs.detach().cpu().double().numpy() - alpha * max_sim
    return max_sim, scores, np.array([first_max(row) for row in scores.reshape(-1, k)])


def first_max(row):
    nan = np.nonzero(np.isnan(row))[0]
    return int(nan[0]) if nan.size else int(np.argmax(row))


def select_accepted(winner, scores, max_sim, hidden_states, index, cand_hidden, probs, alpha, k):
    """-> (complaints, worst max_sim error / eps_sim, worst score error / eps_score).  NaN exactly where the oracle has it; max_sim within
    eps_sim, scores within eps_score; 0 <= winner < k; the winner satisfies ref_score[winner] >= max ref_score - 2 eps_score, and where the
    oracle's margin over its runner-up exceeds that, the winner is the oracle's; a row with a NaN score: the first NaN wins."""
    D = hidden_states.shape[2]
    es, ec = eps_sim(D), eps_score(alpha, D)
    ms, sc, win = step(hidden_states, index, cand_hidden, probs, alpha, k)
    got_ms, got_sc = max_sim.detach().cpu().double().numpy(), scores.detach().cpu().double().numpy()
    got_w = winner.cpu().numpy().astype(np.int64)
    bad = []
    if not (np.isnan(ms) == np.isnan(got_ms)).all() or not (np.isnan(sc) == np.isnan(got_sc)).all():
        bad.append(f"NaN pattern: max_sim {got_ms.tolist()} against {ms.tolist()}, scores {got_sc.tolist()} against {sc.tolist()}")
        return bad, np.inf, np.inf
    with np.errstate(invalid="ignore"):
        e_ms = np.nan_to_num(np.abs(got_ms - ms), nan=0.0)
        e_sc = np.nan_to_num(np.abs(got_sc - sc), nan=0.0)
    w_ms, w_sc = float(e_ms.max() / es), float(e_sc.max() / ec)
    if w_ms > 1.0:
        bad.append(f"max_sim off by {w_ms:.3f} eps_sim")
    if w_sc > 1.0:
        bad.append(f"scores off by {w_sc:.3f} eps_score")
    for b, row in enumerate(sc.reshape(-1, k)):
        w = got_w[b]
        if not 0 <= w < k:
            bad.append(f"row {b}: winner {w} outside [0, {k})")
            continue
        if np.isnan(row).any():
            if w != win[b]:
                bad.append(f"row {b}: the first NaN score wins ({win[b]}), got {w}")
            continue
        top = row.max()
        if not row[w] >= top - 2 * ec:
            bad.append(f"row {b}: winner {w} scores {row[w]!r}, the best {top!r}, more than 2 eps_score = {2 * ec!r} below")
        rest = np.delete(row, win[b])
        if (rest.size == 0 or top - rest.max() > 2 * ec) and w != win[b]:
            bad.append(f"row {b}: the oracle's winner {win[b]} leads by a clear margin, got {w}")
    return bad, w_ms, w_sc


# ---- commit ---------------------------------------------------------------------------------------------------------------------------------
def commit_broadcast(cache, prompt, hidden_states, cand_hidden, winner, index, k, position=None):
    """the composed broadcast on clones -> (cache, prompt, hidden_states): one position of every tensor takes the winner's values"""
    position = index if position is None else position
    B = winner.shape[0]
    rows = (torch.arange(B, device=winner.device) * k + winner.long())
    prompt, hidden_states = prompt.clone(), hidden_states.clone()
    prompt[:, index] = torch.repeat_interleave(prompt[rows, index], k)
    hidden_states[:, index] = cand_hidden[rows]
    if cache is not None:
        cache = cache.clone()
        cache[:, :, :, position] = torch.repeat_interleave(cache[rows][:, :, :, position], k, dim=0)
    return cache, prompt, hidden_states


# ---- the loop -------------------------------------------------------------------------------------------------------------------------------
def contrastive_search(next, prompt, cache, index, mask, hidden_states, k, alpha, T=1.0, end_token_id=None):
    """keras_nlp's ContrastiveSampler.__call__ in fp64 over `next` (which gets and returns float tensors; cache None) -> (prompt [B, S], the
    smallest margin between a winner's score and its runner-up over all steps)"""
    B, S = prompt.shape
    prompt = prompt.clone()
    hist = hidden_states.detach().clone().double()
    logits, _, _ = next(prompt, None, index)
    prompt_k = torch.repeat_interleave(prompt, k, dim=0)
    margin = np.inf
    while index < S:
        if end_token_id is not None and bool((((prompt_k[::k] == end_token_id) & ~mask).any(dim=-1)).all()):
            break
        p = probabilities(logits, T)
        order = np.stack([np.lexsort((np.arange(p.shape[1]), -p[b]))[:k] for b in range(B)])
        probs = torch.from_numpy(np.take_along_axis(p, order, axis=1))
        tokens = torch.from_numpy(order).to(prompt.dtype)
        tokens = torch.where(mask[:, index, None], prompt_k[::k, index, None], tokens)
        prompt_k[:, index] = tokens.reshape(-1)
        next_logits, cand_hidden, _ = next(prompt_k, None, index + 1)
        _, scores, win = step(hist, index, cand_hidden, probs.reshape(-1), alpha, k)
        for b, row in enumerate(scores.reshape(B, k)):
            if k > 1 and not bool(mask[b, index]):
                margin = min(margin, float(row[win[b]] - np.delete(row, win[b]).max()))
        rows = torch.arange(B) * k + torch.from_numpy(win)
        prompt_k = torch.repeat_interleave(prompt_k[rows], k, dim=0)
        hist[:, index] = cand_hidden[rows].double()
        logits = next_logits[rows]
        index += 1
    return prompt_k[::k].clone(), margin
