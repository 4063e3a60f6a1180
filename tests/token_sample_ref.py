"""The oracle of the token samplers (iseg_token_sample / F.sample_tokens), written from the statement in include/iseg_hip.h and not from the kernel:
fp64 numpy on the CPU.

Per row x[0..V): the order pi sorts by x descending, then index ascending, NaN above +inf above the finite values above -inf.  If x[pi[0]] is not
finite the token is pi[0].  Otherwise w_i = exp(x_i / T - max x / T), W = sum w, and the kept set is every index ("random"), the first min(k, V)
of pi ("top_k"), or the positions j of the first k' = min(k, V) (k = 0: V) of pi with sum_{t<j} w_pi(t) <= p W ("top_p": a prefix of pi, the
first always kept).  The kept ids in token-id order have the cumulative weights C_i and the sum S; the token is the smallest kept id with
C_i > u S.

accepted_tokens allows the kernel its fp32 arithmetic: an id is accepted if its interval [C_prev, C_i] comes within eps * S of u * S, and for
"top_p" under any cut (number of kept positions) whose preceding mass lies within eps * W of p * W."""
import numpy as np
import torch

MODES = ("random", "top_k", "top_p")


def _row64(x):
    if isinstance(x, torch.Tensor):
        x = x.detach().to("cpu").to(torch.float64).numpy()
    return np.asarray(x, dtype=np.float64)


def order(x):
    """pi: indices by value descending, then index ascending; NaN first"""
    x = np.asarray(x, dtype=np.float64)
    nan = np.isnan(x)
    neg = np.where(nan, 0.0, -x)
    return np.lexsort((np.arange(x.shape[0]), neg, ~nan))


def weights(x, T):
    """w_i = exp(x_i / T - max_j x_j / T) for a row whose maximum is finite"""
    t = x / float(T)
    with np.errstate(invalid="ignore"):
        return np.exp(t - np.max(t))


def _cut_range(x, mode, k, p, T, eps):
    """(pi, w, n_exact, n_lo, n_hi): the kept set is pi[:n]; n_lo .. n_hi are the cuts the tolerance allows"""
    V = x.shape[0]
    pi = order(x)
    w = weights(x, T)
    if mode == "random":
        return pi, w, V, V, V
    if mode == "top_k":
        n = min(int(k), V)
        return pi, w, n, n, n
    kq = V if int(k) == 0 else min(int(k), V)
    wp = w[pi][:kq]
    W = float(np.sum(w))
    before = np.concatenate(([0.0], np.cumsum(wp)[:-1]))      # mass in front of position j
    target = float(p) * W
    n = max(1, int(np.count_nonzero(before <= target)))
    n_lo = max(1, int(np.count_nonzero(before <= target - eps * W)))
    n_hi = max(1, int(np.count_nonzero(before <= target + eps * W)))
    return pi, w, n, n_lo, n_hi


def kept_set(x, mode, k=0, p=1.0, T=1.0):
    """the exact kept set of one row (no tolerance) as a Python set; a row with a non-finite top keeps that index alone"""
    x = _row64(x)
    pi = order(x)
    if not np.isfinite(x[pi[0]]):
        return {int(pi[0])}
    pi, _, n, _, _ = _cut_range(x, mode, k, p, T, 0.0)
    return set(int(i) for i in pi[:n])


def exact_token(x, u, mode, k=0, p=1.0, T=1.0):
    """the token of one row in fp64, no tolerance"""
    x = _row64(x)
    pi = order(x)
    if not np.isfinite(x[pi[0]]):
        return int(pi[0])
    pi, w, n, _, _ = _cut_range(x, mode, k, p, T, 0.0)
    ids = np.sort(pi[:n])
    C = np.cumsum(w[ids])
    hit = np.nonzero(C > float(u) * C[-1])[0]
    if hit.size:
        return int(ids[hit[0]])
    return int(ids[np.nonzero(w[ids] > 0)[0][-1]])


def _accepted_under_cut(pi, w, n, u, eps):
    ids = np.sort(pi[:n])
    wk = w[ids]
    C = np.cumsum(wk)
    S = C[-1]
    ok = (C - wk - eps * S <= u * S) & (u * S <= C + eps * S)
    return set(int(i) for i in ids[ok])


def _row_accepted(x, u, mode, k, p, T, eps, candidates):
    pi = order(x)
    if not np.isfinite(x[pi[0]]):
        return {int(pi[0])}
    pi, w, _, n_lo, n_hi = _cut_range(x, mode, k, p, T, eps)
    u = float(u)
    if n_lo == n_hi:
        out = _accepted_under_cut(pi, w, n_lo, u, eps)
        return out if candidates is None else out & set(candidates)
    if candidates is None:
        out = set()
        for n in range(n_lo, n_hi + 1):
            out |= _accepted_under_cut(pi, w, n, u, eps)
        return out
    # one candidate at a time, all cuts at once: C_i(n) = the weight of the positions r < n of pi whose id is <= i
    rank = np.empty_like(pi)
    rank[pi] = np.arange(pi.shape[0])
    wp, ip = w[pi][:n_hi], pi[:n_hi]
    S = np.cumsum(wp)
    out = set()
    for i in set(int(c) for c in candidates):
        if not 0 <= i < x.shape[0] or rank[i] >= n_hi:
            continue
        first = max(n_lo, int(rank[i]) + 1)
        C = np.cumsum(np.where(ip <= i, wp, 0.0))[first - 1:]
        Sn = S[first - 1:]
        if np.any((C - w[i] - eps * Sn <= u * Sn) & (u * Sn <= C + eps * Sn)):
            out.add(i)
    return out


def accepted_tokens(x, u, mode, k=0, p=1.0, T=1.0, eps=1e-5, candidates=None):
    """x [B, V], u [B] -> a list of B sets of acceptable token ids.  `candidates` ([B] ids, one per row): only these are examined (the returned
    set is the accepted set intersected with {candidates[b]}), which keeps a large top-p row with many admissible cuts affordable."""
    assert mode in MODES
    x = _row64(x)
    u = _row64(u)
    if x.ndim == 1:
        x, u = x[None], u.reshape(1)
    cand = None if candidates is None else _row64(candidates).astype(np.int64)
    return [_row_accepted(x[b], u[b], mode, k, p, T, eps, None if cand is None else [int(cand[b])]) for b in range(x.shape[0])]
