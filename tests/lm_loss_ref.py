"""fp64 restatement of the language-model head's cross-entropy as include/iseg_hip.h states it (iseg_lm_head_ce_*), on the CPU, from inputs that
the caller has ALREADY rounded to the compute dtype.  Nothing here is chunked: the full logits are formed.

    Z = X E^T;  lse_r = logsumexp(Z_r);  valid_r = 0 <= t_r < V;  w_r = valid_r ? weight_r : 0
    loss_r = scale w_r (lse_r - Z[r, t_r]), exactly 0 where w_r = 0;  argmax_r = the smallest v with Z[r, v] = max Z_r;  match_r = valid_r and argmax_r = t_r
    sums = (sum loss, sum w match, sum w)
    G = scale w_r up_r (softmax(Z_r) - onehot(t_r)), zero rows where w_r = 0;  dX = G E;  dE = G^T X
"""
import torch


def _rows(x, E, t, weights):
    x, E = x.double(), E.double()
    V = E.shape[0]
    t = t.reshape(-1).to(torch.int64)
    valid = (t >= 0) & (t < V)
    w = torch.ones(t.shape, dtype=torch.float64) if weights is None else weights.reshape(-1).double()
    return x.reshape(-1, E.shape[1]), E, t, valid, torch.where(valid, w, torch.zeros_like(w))


def logits(x, E):
    return x.double().reshape(-1, E.shape[1]) @ E.double().T


def first_argmax(Z):
    """the smallest index holding the row maximum"""
    V = Z.shape[-1]
    idx = torch.arange(V, dtype=torch.int64).expand_as(Z)
    return torch.where(Z == Z.max(dim=-1, keepdim=True).values, idx, torch.full_like(idx, V)).min(dim=-1).values


def accepted(Z, eps):
    """bool [M, V]: the indices an argmax may return when every logit is known to within eps / 2"""
    return Z >= Z.max(dim=-1, keepdim=True).values - eps


def forward(x, E, t, weights=None, scale=1.0):
    """-> dict(Z, lse, loss, argmax, match, sums, w), all fp64 / int64 of M = t.numel() rows"""
    x2, E, t, valid, w = _rows(x, E, t, weights)
    Z = x2 @ E.T
    lse = torch.logsumexp(Z, dim=-1)
    zt = Z.gather(1, t.clamp(0, E.shape[0] - 1)[:, None])[:, 0]
    loss = torch.where(w != 0, scale * w * (lse - zt), torch.zeros_like(lse))
    argmax = first_argmax(Z)
    match = valid & (argmax == t)
    sums = torch.stack([loss.sum(), (w * match.double()).sum(), w.sum()])
    return {"Z": Z, "lse": lse, "loss": loss, "argmax": argmax, "match": match, "sums": sums, "w": w}


def backward(x, E, t, weights=None, upstream=None, scale=1.0):
    """-> (G [M, V], dX [M, d], dE [V, d]) for the upstream gradient `upstream` [M] of the per-token loss (None: ones)"""
    x2, E, t, valid, w = _rows(x, E, t, weights)
    Z = x2 @ E.T
    up = torch.ones_like(w) if upstream is None else upstream.reshape(-1).double()
    G = torch.softmax(Z, dim=-1)
    rows = torch.nonzero(valid)[:, 0]
    G[rows, t[rows]] -= 1.0
    G = G * (scale * w * up)[:, None]
    G[w == 0] = 0.0
    return G, G @ E, G.T @ x2


def reduce(loss, w, match, reduction="sum_over_batch_size"):
    """Keras: "sum_over_batch_size" divides sum w l by the ELEMENT count; the accuracy is sum w match / sum w.  `loss` already holds w l"""
    acc = (w * match.double()).sum() / w.sum()
    if reduction == "none":
        return loss, acc
    return (loss.sum() / loss.numel() if reduction == "sum_over_batch_size" else loss.sum()), acc
