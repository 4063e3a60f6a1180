"""Key-coded attention inputs (test infrastructure, CPU only, vectorised): every row of the fp64 reference output NAMES the key or keys the row
attended, so that a row which sees one key too many, one too few, or the wrong key/value head gives a different bf16 value instead of a small
change of a norm.  Used by tests/test_attention_key_codes_host.py (which pins the construction) and tests/test_attention_key_codes_gpu.py (causal
grouped-query prefill of csrc/gemma.hip, split-KV decode of csrc/gemma_decode.hip, wide-value self-attention of csrc/selfattn.hip).

Construction (all values exactly representable in bf16; at most 256 visible keys; head width h >= 64):
  * key code: K[s][i] = +-a_k for i < 8, the sign from bit i of s; K[s][8] is the marker (0, or MARK * a_k); K[s][9:] = 0.  A query aimed at key
    a has q[:8] = a_q * code(a) and scores UNIT * (8 - 2 * hamming(a, s)) on key s with UNIT = a_q * a_k * scale = 32 (45.25.. at h = 128, where
    the scale is inexact; equal integer dot products still give equal fp32 scores, so ties survive).  A tied aim is a_q * (code(a) + code(a')) for
    a' = a ^ 2^i: both score 14 units, every other key at most 10.  A single aim beats every other key by 2 units = 64 in score, so every other
    softmax weight is below e^-64.
  * aims: per (token t, query head n), with a the latest visible key, (position + n) mod 4 selects (0) a alone, (1) a tied with its nearest
    visible one-bit partner below it, (2) a tied with its farthest such partner (another 64-key tile once a >= 64), (3) the first visible key.
    A row without a visible partner aims at a alone.
  * marker: every query has q[8] = a_q, a marked key K[s][8] = MARK * a_k gains MARK = 64 units (2048 in score) on every query, more than any
    code score.  Marked are the padded keys (nobody may see them), the decode cache's two rows behind the last visible key, the first two and the
    last key of the self-attention's second sample, and the "hot" keys: rows before a hot key must not see it, rows from it on attend it alone.
  * values: V[b][s][kvh][j] = ((7 s + 3 j + 5 kvh + 11 b) mod 17) + 1, dout[b][t][n][j] = ((5 t + 3 j + 7 n + 2 b) mod 9) - 4: the output of a
    row is the mean of its targets' V rows, an integer or a half-integer in [1, 17].  V is positive on purpose: where a mean were 0 the
    reference would be its e^-64 terms alone, and no kernel can be asked for THEIR bits.

A Problem holds q [B, Tq, nq, h], k [B, S, nkv, h], v [B, S, nkv, hv], dout [B, Tq, nq, hv] (fp64 tensors of bf16 values) and vis [B, Tq, S].
The fp64 reference comes from tests/gemma_ref.py, tests/gemma_cache_ref.py and tests/self_attention_ref.py; nothing is restated anew except
`fp64_parts`, which exists to form the bounds and is itself checked against the reference's gradients by the host test."""
import math
from types import SimpleNamespace

import torch

from tests import gemma_cache_ref as C
from tests import gemma_ref as R
from tests import self_attention_ref as S

MARK = 64                     # units a marked key gains on every query
BITS = torch.arange(8)
LOG2E = 1.4426950408889634


def amplitudes(h):
    """(a_q, a_k) with a_q * a_k * h^-0.5 = 32 at h = 64 and 256; at h = 128 the unit is 512 / sqrt(128) = 45.25.."""
    return (16.0, 16.0) if h == 64 else (32.0, 16.0)


def sign_code(idx):
    """long [...] -> fp64 [..., 8]: +1 where bit i of idx is set, else -1"""
    return (((idx[..., None] >> BITS) & 1) * 2 - 1).double()


def bf16_round(t):
    return t.to(torch.float32).to(torch.bfloat16).double()


def padding(kind, B, T):
    """the masks of tests/test_gemma_gpu.py, plus holes: every eleventh key from key 5 on is padding"""
    if kind == "none":
        return None
    m = torch.ones(B, T, dtype=torch.int32)
    for b in range(B):
        if kind == "right":
            m[b, max(1, T - 5 - 3 * b):] = 0
        elif kind == "holes":
            m[b, 5::11] = 0
        else:
            m[b, :min(T, 3 if kind == "left3" else 70)] = 0
    return m


# ---- the builder -------------------------------------------------------------------------------------------------------------------------------
def _build(kind, vis, marked, present, pos, nq, nkv, h, hv, anchor=None):
    """vis bool [B, Tq, S]; marked, present bool [B, S] (present: the row holds a finite key); pos long [Tq]: the tokens' positions (they cycle
    the aims); anchor long [B, Tq]: the key `a` of each token instead of its latest visible key.  Asserts the tie count of every row and a gap of at least 2 units."""
    B, Tq, Sk = vis.shape
    g = nq // nkv
    a_q, a_k = amplitudes(h)
    scale = float(h) ** -0.5
    ar = torch.arange(Sk)
    has = vis.any(-1)
    assert int(torch.where(vis, ar, -1).max()) < 256, "the code has eight bits"
    last = torch.where(vis, ar, -1).amax(-1).clamp(min=0) if anchor is None else anchor
    first = torch.where(vis, ar, Sk).amin(-1).clamp(max=Sk - 1)
    cand = last[..., None] ^ (1 << BITS)                                                   # [B, Tq, 8]: below `last` where the bit is set
    ok = ((last[..., None] >> BITS) & 1).bool() & torch.gather(vis, 2, cand.clamp(max=Sk - 1))
    partner = ok.any(-1)
    near = torch.where(partner, torch.where(ok, cand, -1).amax(-1), last)
    far = torch.where(partner, torch.where(ok, cand, Sk).amin(-1), last)
    ca = sign_code(last)
    tied = lambda other: torch.where(partner[..., None], ca + sign_code(other), ca)        # noqa: E731
    choices = torch.stack([ca, tied(near), tied(far), sign_code(first)], dim=2)          # [B, Tq, 4, 8]
    aim = ((pos[None, :, None] + torch.arange(nq)[None, None, :]) % 4).expand(B, Tq, nq)
    qcode = torch.gather(choices, 2, aim[..., None].expand(B, Tq, nq, 8))
    intended = torch.where(((aim == 1) | (aim == 2)) & partner[..., None], 2, 1)

    # integer scores in units, independent of any floating-point path
    kcode = sign_code(ar & 255)                                                            # [S, 8]
    units = (torch.einsum("btni,si->btns", qcode, kcode) + MARK * marked[:, None, None, :].double()).long()
    NEG = -10 ** 6
    visx = vis[:, :, None, :]
    top = torch.where(visx, units, NEG).amax(-1)
    wins = visx & (units == top[..., None])
    count = wins.sum(-1)
    rest = torch.where(visx & ~wins, units, NEG).amax(-1)
    gap = torch.where(rest == NEG, 10 ** 6, top - rest)
    sees_marked = (vis & marked[:, None, :]).any(-1)[..., None].expand(B, Tq, nq)
    live = has[..., None].expand(B, Tq, nq)
    # a row that sees marked keys attends the best-coded of them: one, or two in an exact tie; every other row ties as its aim intends
    assert bool(((count == intended) | sees_marked | ~live).all()), "a row's tie count is not the intended one"
    assert bool((((count >= 1) & (count <= 2)) | ~live).all()), "a row ties more than two ways"
    assert bool(((gap >= 2) | ~live).all()), "a target beats another key by less than two units"
    hidden = present[:, None, None, :] & ~visx
    outscored = live & (torch.where(hidden, units, NEG).amax(-1) >= top)

    q = torch.zeros(B, Tq, nq, h, dtype=torch.float64)
    q[..., :8] = a_q * qcode
    q[..., 8] = a_q
    k = torch.zeros(B, Sk, nkv, h, dtype=torch.float64)
    k[..., :8] = a_k * kcode[None, :, None, :]
    k[..., 8] = MARK * a_k * marked[:, :, None].double()
    bb, ss, kk, jj = torch.meshgrid(torch.arange(B), ar, torch.arange(nkv), torch.arange(hv), indexing="ij")
    v = ((7 * ss + 3 * jj + 5 * kk + 11 * bb) % 17 + 1).double()
    bb, tt, nn, jj = torch.meshgrid(torch.arange(B), torch.arange(Tq), torch.arange(nq), torch.arange(hv), indexing="ij")
    dout = ((5 * tt + 3 * jj + 7 * nn + 2 * bb) % 9 - 4).double()
    weight = wins.double() / count.clamp(min=1)[..., None]                                 # [B, Tq, nq, S]
    closed = torch.einsum("btkgs,bskj->btkgj", weight.reshape(B, Tq, nkv, g, Sk), v).reshape(B, Tq, nq, hv)
    for t in (q, k, v, dout):
        assert torch.equal(bf16_round(t), t)
    return SimpleNamespace(kind=kind, q=q, k=k, v=v, dout=dout, vis=vis, marked=marked, present=present, nq=nq, nkv=nkv, h=h, hv=hv, scale=scale,
                           unit=a_q * a_k * scale, aim=aim, count=count, intended=intended, gap_units=gap, live=live, outscored=outscored,
                           closed_form=closed, max_score=float(units.abs().max()) * a_q * a_k * scale)


def _hot_mask(hot, B, Sk):
    """hot: per sample None, an int, or a tuple of ints"""
    m = torch.zeros(B, Sk, dtype=torch.bool)
    for b, keys in enumerate(hot):
        for s in (() if keys is None else (keys,) if isinstance(keys, int) else keys):
            m[b, s] = True
    return m


def prefill(case, kind, hot):
    """case (B, T, nq, nkv, h), mask kind, hot key(s) per sample -> Problem with .pad (int32 [B, T] or None) and .qkv / .dout_rows, the packed
    bf16 rows of kernels.gemma_attention_fwd"""
    B, T, nq, nkv, h = case
    pad = padding(kind, B, T)
    vis = R.attention_mask(pad, B, T).clone()
    marked = _hot_mask(hot, B, T)
    if pad is not None:
        marked |= pad == 0
    p = _build("prefill", vis, marked, torch.ones(B, T, dtype=torch.bool), torch.arange(T), nq, nkv, h, h)
    p.pad, p.case = pad, case
    p.qkv = torch.cat([p.q.reshape(B, T, -1), p.k.reshape(B, T, -1), p.v.reshape(B, T, -1)], dim=-1).to(torch.bfloat16)
    p.dout_rows = p.dout.reshape(B, T, -1).to(torch.bfloat16)
    return p


def decode(case, hot=()):
    """case (B, S, pos0, Tn, nq, nkv, h, splits), hot keys (the same in every sample) -> Problem with .q_rows bf16 [B, Tn, nq h] and .cache bf16
    [B, 2, S, nkv, h]: coded keys, rows nvis and nvis + 1 marked with finite values, NaN behind; the Problem's k / v hold zeros there"""
    B, Sk, pos0, Tn, nq, nkv, h, _ = case
    nvis = pos0 + Tn
    vis = C.compute_causal_mask(B, Sk, Tn, pos0).clone()
    marked = _hot_mask([tuple(hot)] * B, B, Sk)
    marked[:, nvis:nvis + 2] = True
    present = torch.zeros(B, Sk, dtype=torch.bool)
    present[:, :nvis + 2] = True
    p = _build("decode", vis, marked, present, pos0 + torch.arange(Tn), nq, nkv, h, h)
    p.k[:, nvis + 2:] = 0
    p.v[:, nvis + 2:] = 0
    p.pos0, p.case = pos0, case
    p.q_rows = p.q.reshape(B, Tn, -1).to(torch.bfloat16)
    p.cache = torch.stack([p.k, p.v], dim=1).to(torch.bfloat16)
    p.cache[:, :, nvis + 2:] = float("nan")
    return p


def self_attention(T, dv, hot0):
    """two contiguous samples of T tokens, dk = 64, scale 1/8: sample 0's hot key is hot0 (None: no hot key, its rows tie as they aim, which is
    what makes its dq and dk non-zero); sample 1's first two keys and its last key are marked (rows T .. of sample 0 ARE rows 0 .. of sample 1
    in memory).  Nothing is causal here, so the key `a` of row t is its own key t -> Problem with nq = nkv = 1"""
    B = 2
    vis = torch.ones(B, T, T, dtype=torch.bool)
    marked = _hot_mask([hot0, tuple(sorted({0, min(1, T - 1), T - 1}))], B, T)
    p = _build("self", vis, marked, torch.ones(B, T, dtype=torch.bool), torch.arange(T), 1, 1, 64, dv,
               anchor=torch.arange(T)[None].expand(B, T))
    p.case = (B, T, dv)
    return p


# ---- the fp64 reference ------------------------------------------------------------------------------------------------------------------------
def reference(p, vis=None):
    """(out [B, Tq, nq, hv], dq, dk, dv) from the suite's restatements with autograd.  vis=None: the restatement's own mask (attention_core,
    cached_attention_core, core); a bool [B, Tq, S] replaces the mask (the corruptions of the host test) through the same compute_attention / wipe"""
    q, k, v = (t.clone().requires_grad_(True) for t in (p.q, p.k, p.v))
    B, Tq = q.shape[:2]
    if p.kind == "self":
        assert vis is None
        out = S.core(q[:, :, 0], k[:, :, 0], v[:, :, 0], p.scale)[:, :, None, :]
    elif vis is not None:
        out = R.wipe(R.compute_attention(q, k, v, vis, p.nq, p.nkv), vis)
    elif p.kind == "prefill":
        out = R.attention_core(q, k, v, p.pad, p.nq, p.nkv).reshape(B, Tq, p.nq, p.hv)
    else:
        out = C.cached_attention_core(q, k, v, p.pos0, p.nq, p.nkv).reshape(B, Tq, p.nq, p.hv)
    out.backward(p.dout)
    return out.detach(), q.grad, k.grad, v.grad


def fp64_parts(p):
    """P and dS = P o (dP - D) [B, nkv, g, Tq, S] in fp64 under the Problem's own visibility: the quantities the bounds are formed from"""
    B, Tq = p.q.shape[:2]
    g = p.nq // p.nkv
    s = torch.einsum("btkgh,bskh->bkgts", p.q.reshape(B, Tq, p.nkv, g, p.h), p.k) * p.scale
    m = p.vis[:, None, None]
    P = torch.softmax(torch.where(m, s, -math.inf), dim=-1)
    P = torch.where(m.any(-1, keepdim=True), P, torch.zeros_like(P))
    out = torch.einsum("bkgts,bskj->btkgj", P, p.v)
    do = p.dout.reshape(B, Tq, p.nkv, g, p.hv)
    dP = torch.einsum("btkgj,bskj->bkgts", do, p.v)
    D = (do * out).sum(-1).permute(0, 2, 3, 1)[..., None]
    return P, P * (dP - D)


def gradients_of(p, P, dS):
    """(dq, dk, dv) of given P and dS, fp64"""
    B, Tq = p.q.shape[:2]
    g = p.nq // p.nkv
    dq = p.scale * torch.einsum("bkgts,bskh->btkgh", dS, p.k).reshape(B, Tq, p.nq, p.h)
    dk = p.scale * torch.einsum("bkgts,btkgh->bskh", dS, p.q.reshape(B, Tq, p.nkv, g, p.h))
    dv = torch.einsum("bkgts,btkgj->bskj", P, p.dout.reshape(B, Tq, p.nkv, g, p.hv))
    return dq, dk, dv


def bounds(p, ref):
    """per-element bounds on |kernel - reference| for (dq, dk, dv), derived, from fp64 quantities only:
      dv: 2^-8 |ref| + N 2^-23 A_v + 1e-12 -- one output rounding; P and dout are exact and fp32 sums of integers and halves are exact.  The
      middle term is the matrix cores' accumulation (`_mfma_sum`): an instruction aligns its addends to the largest of them, and an e^-64
      term below that grid can cost one unit of the grid's last place, which is all that is left where the integers cancel to zero.  Each
      of the N addends of an element (its g Tq products and the running sum of each 32-row instruction) loses less than one fp32 unit in
      the last place of the largest addend, which is at most A_v = sum |P| |dout|;
      dq, dk: 2^-8 (1.01 A + |ref|) + 1e-12 with A the same sum over absolute values (scale sum |dS| |K|; scale sum |dS| |Q| over the group) -- one
      rounding of dS and one of the output, safe under cancellation.  1e-12 covers the neglected e^-64 terms."""
    _, dq, dk, dv = ref
    P, dS = fp64_parts(p)
    q, k = p.q, p.k
    absp = SimpleNamespace(q=q.abs(), k=k.abs(), v=p.v, dout=p.dout.abs(), nq=p.nq, nkv=p.nkv, h=p.h, hv=p.hv, scale=p.scale)
    Aq, Ak, Av = gradients_of(absp, P, dS.abs())      # scale sum |dS| |K|, scale sum |dS| |Q|, sum |P| |dout|
    rows = (p.nq // p.nkv) * p.q.shape[1]
    addends = rows + (rows + 31) // 32
    u = 2.0 ** -8
    return u * (1.01 * Aq + dq.abs()) + 1e-12, u * (1.01 * Ak + dk.abs()) + 1e-12, u * dv.abs() + addends * 2.0 ** -23 * Av + 1e-12


def dv_bound_without_accumulation(ref):
    """2^-8 |ref| + 1e-12: the dv bound if fp32 sums of integers and halves were exact beside e^-64 terms (the host test shows they are not)"""
    return 2.0 ** -8 * ref[3].abs() + 1e-12


def unseen_keys(p):
    """bool [B, S]: keys no row may see (dk = dv = 0 exactly)"""
    return ~p.vis.any(1)


# ---- the same computation with the kernels' rounding points ---------------------------------------------------------------------------------------
def _f32(t):
    return t.to(torch.float32)


def _mfma_sum(w, x):
    """sum_n w[..., n, s] x[..., n, j] -> [..., s, j] as a chain of 32-deep matrix-core instructions (v_mfma_f32_16x16x32_bf16, n in kernel
    order): the 32 exact products and the running sum are brought onto the grid 2^(e - 24) of the largest of them, 2^e <= max < 2^(e + 1),
    each truncated downwards, added exactly, and the sum rounded to fp32.  This is the envelope of what the hardware was seen to do: where the
    integer terms of one instruction cancel and an e^-64 term is negative, -2^(e - 24) is left (an MI355X returned exactly that at part of
    the entries where this model does, and the exact sum at the others)."""
    acc = torch.zeros(w.shape[:-2] + (w.shape[-1], x.shape[-1]), dtype=torch.float64)
    for n0 in range(0, w.shape[-2], 32):
        prod = w[..., n0:n0 + 32, :, None] * x[..., n0:n0 + 32, None, :]
        amax = torch.maximum(prod.abs().amax(-3), acc.abs())
        grid = torch.ldexp(torch.ones_like(amax), torch.frexp(amax)[1] - 25)      # frexp: amax = m 2^E, 0.5 <= m < 1, so e = E - 1
        total = (torch.floor(prod / grid[..., None, :, :]).sum(-3) + torch.floor(acc / grid)) * grid
        acc = torch.where(amax > 0, total, acc).float().double()
    return acc


def restate_with_kernel_rounding(p, vis=None, score_bf16=False, mfma="exact"):
    """(out, dq, dk, dv) as fp64 tensors of bf16 values, computed where the kernels compute and rounded where they round:
      scores: the fp32 MFMA sum of exact products (integers below 2^24: exact); score_bf16 (the composed routes): scale * score rounded to bf16;
      softmax in fp32 in the exp2 domain: p = exp2(fma(s, c, -round(m c))), c = scale * log2 e, l = sum p;
      forward: P rounded to bf16 before P V, fp32 accumulation, out = bf16(acc * (1 / l)); rows without a visible key: 0;
      backward: L = fma(m, c, log2 l), p = exp2(fma(s, c, -L)), P rounded to bf16 before P^T dout, D = sum dout * out over the bf16 output in fp32,
      dS = bf16(p * (dP - D) * scale), fp32 accumulation of dS K and dS^T Q, every output rounded once;
      mfma="aligned": the three gradient sums run through `_mfma_sum` in the kernels' order (stacked query rows t g + j for dk and dv, keys for
      dq) instead of exactly.  The forward's P V is left exact: its targets' weights are 1 or 1/2, and a loss of 2^-24 relative per addend
      is nowhere near a bf16 rounding boundary of an integer or half-integer.
    The kernels walk the keys in tiles and rescale by exp2((m_old - m_new) c); on these inputs that factor is 1 (a tie across tiles) or below
    2^-92, so the one-pass form differs by less than 1e-25."""
    vis = p.vis if vis is None else vis
    B, Tq = p.q.shape[:2]
    g = p.nq // p.nkv
    m = vis[:, None, None]
    any_vis = m.any(-1, keepdim=True)
    s = torch.einsum("btkgh,bskh->bkgts", p.q.reshape(B, Tq, p.nkv, g, p.h), p.k)
    assert float(s.abs().max()) < 2 ** 24
    scale32 = _f32(torch.tensor(p.scale))
    if score_bf16:
        s, c = bf16_round(_f32(s) * scale32), _f32(torch.tensor(LOG2E))
    else:
        c = scale32 * _f32(torch.tensor(LOG2E))
    fma = lambda a, b, d: _f32(a.double() * b.double() + d.double())      # noqa: E731  (a product of two fp32 values is exact in fp64)
    s32 = _f32(s)
    mx = torch.where(m, s32, -math.inf).amax(-1, keepdim=True)
    mx = torch.where(any_vis, mx, torch.zeros_like(mx))
    mc = mx * c
    pf = torch.where(m, torch.exp2(fma(s32, c, -mc)), torch.zeros_like(s32))
    l = pf.sum(-1, keepdim=True)
    acc = _f32(torch.einsum("bkgts,bskj->bkgtj", bf16_round(pf), p.v))
    inv = torch.where(any_vis, 1.0 / l, torch.zeros_like(l))
    out = bf16_round(acc * inv)                                            # [B, nkv, g, Tq, hv]
    L = torch.where(any_vis, fma(mx, c, torch.log2(l)), torch.zeros_like(l))
    do = p.dout.reshape(B, Tq, p.nkv, g, p.hv).permute(0, 2, 3, 1, 4)      # [B, nkv, g, Tq, hv]
    D = _f32((do * out).sum(-1, keepdim=True))
    p2 = torch.exp2(fma(s32, c, -L))
    dP = _f32(torch.einsum("bkgtj,bskj->bkgts", do, p.v))
    if score_bf16:
        dS = bf16_round(torch.where(m, p2 * (dP - D), torch.zeros_like(p2))) * float(scale32)      # the scale rides on the GEMM of the composed route
        dS_scaled = dS
    else:
        dS_scaled = bf16_round(torch.where(m, p2 * (dP - D) * scale32, torch.zeros_like(p2)))
    Pb = bf16_round(torch.where(m, p2, torch.zeros_like(p2)))
    unit = SimpleNamespace(q=p.q, k=p.k, v=p.v, dout=p.dout, nq=p.nq, nkv=p.nkv, h=p.h, hv=p.hv, scale=1.0)
    if mfma == "aligned":
        R = Tq * g
        stack = lambda t: t.permute(0, 1, 3, 2, 4).reshape(B, p.nkv, R, t.shape[-1])      # noqa: E731  [B, nkv, g, Tq, x] -> [B, nkv, Tq g, x]
        qs = p.q.reshape(B, Tq, p.nkv, g, p.h).permute(0, 2, 1, 3, 4).reshape(B, p.nkv, R, p.h)
        dv = _mfma_sum(stack(Pb), stack(do)).permute(0, 2, 1, 3)
        dk = _mfma_sum(stack(dS_scaled), qs).permute(0, 2, 1, 3)
        dq = _mfma_sum(stack(dS_scaled).transpose(-1, -2), p.k.permute(0, 2, 1, 3))
        dq = dq.reshape(B, p.nkv, Tq, g, p.h).permute(0, 2, 1, 3, 4).reshape(B, Tq, p.nq, p.h)
        dq, dk, dv = (bf16_round(t) for t in (dq, dk, dv))
    else:
        dq, dk, dv = (bf16_round(_f32(t)) for t in gradients_of(unit, Pb, dS_scaled))
    return out.permute(0, 3, 1, 2, 4).reshape(B, Tq, p.nq, p.hv), dq, dk, dv


# ---- the corruptions the relative Frobenius bound does not see -----------------------------------------------------------------------------------
def corruptions(p):
    """name -> corrupted visibility [B, Tq, S] for the mask errors that apply to this Problem (prefill and decode)"""
    vis = p.vis
    B, Tq, Sk = vis.shape
    out = {}
    pos = torch.arange(Tq) + (p.pos0 if p.kind == "decode" else 0)
    ends = [(t, int(s) + 1) for t, s in enumerate(pos) if int(s) % 64 == 63 and int(s) + 1 < Sk and bool(p.present[:, int(s) + 1].all())]
    if ends and (p.kind == "prefill" or Tq == 1):
        c = vis.clone()
        for t, s in ends:
            c[:, t, s] = True
        out["a tile-end row sees the next key"] = c
    starts = [(t, int(s)) for t, s in enumerate(pos) if int(s) % 64 == 0 and int(s) > 0]
    if starts:
        c = vis.clone()
        for t, s in starts:
            c[:, t, s] = False
        out["a tile-start row misses its own key"] = c
    if p.kind == "prefill" and p.pad is not None:
        c = vis.clone()
        for b in range(B):
            s = int(torch.nonzero(p.pad[b] == 0)[0])
            c[b, s:, s] = True
        out["a padded key is visible from its position on"] = c
    if p.kind == "decode" and Tq > 1:
        c = vis.clone()
        c[:, 0, p.pos0 + 1] = True
        out["a decode row of token 0 sees key pos0 + 1"] = c
    return {name: c for name, c in out.items() if not torch.equal(c, vis)}      # (a tile-start key that is padding is missed already)


def next_sample_leak(p):
    """self-attention: sample 0 extended by the first key of sample 1, as a one-sample Problem"""
    k = torch.cat([p.k[:1], p.k[1:, :1]], dim=1)
    v = torch.cat([p.v[:1], p.v[1:, :1]], dim=1)
    return SimpleNamespace(kind="self", q=p.q[:1], k=k, v=v, dout=p.dout[:1], scale=p.scale, nq=1, nkv=1, h=p.h, hv=p.hv)


def changed_rows(a, b):
    """the number of (sample, token, head) rows whose bf16 values differ"""
    return int((bf16_round(a) != bf16_round(b)).any(-1).sum())


def rel_frobenius(a, b):
    return (a - b).norm().item() / max(b.norm().item(), 1e-300)


# ---- the cases of the GPU file (the host file pins every one of them) ---------------------------------------------------------------------------------
# (case (B, T, nq, nkv, h), mask kind, hot key per sample)
PREFILL = [((1, 130, 8, 1, 256), "none", (64,)), ((1, 130, 8, 1, 256), "none", (128,)), ((2, 65, 4, 2, 128), "right", (64, None)),
           ((1, 130, 6, 2, 64), "holes", (128,)), ((1, 197, 16, 16, 64), "left3", (196,)), ((1, 197, 16, 16, 64), "left3", (128,)),
           ((2, 130, 8, 1, 64), "left70", (129, 71)), ((2, 63, 8, 1, 256), "none", (1, 62)), ((2, 1, 1, 1, 64), "none", (None, 0))]
# (case (B, S, pos0, Tn, nq, nkv, h, splits), hot keys)
DECODE = [((2, 8, 0, 1, 1, 1, 64, 0), ()), ((1, 64, 63, 1, 2, 1, 64, 0), ()), ((2, 80, 64, 1, 4, 2, 128, 0), ()),
          ((1, 160, 127, 2, 8, 1, 256, 3), (128,)), ((1, 160, 127, 2, 8, 1, 256, 3), (127,)), ((1, 256, 191, 2, 8, 1, 64, 2), (0, 192)),
          ((1, 320, 255, 1, 16, 16, 64, 0), ()), ((1, 320, 255, 1, 16, 16, 64, 4), ())]
# (T, dv); each runs with sample 0's hot key at T - 1, at 0, and without one
SELF = [(1, 64), (63, 64), (64, 128), (65, 128), (130, 512), (197, 64)]


def ident(entry):
    case, *rest = entry
    return "x".join(map(str, case)) + "".join("-" + ("_".join(str(x) for x in r) if isinstance(r, tuple) else str(r)) for r in rest)


# the prefill and decode cases whose output the restatement with bf16-rounded scores (the composed routes) reproduces bit for bit on the CPU; the
# host test asserts that this list is exactly those
COMPOSED_EXACT = {ident(e) for e in PREFILL + DECODE}
SELF_RUNS = [(T, dv, hot) for T, dv in SELF for hot in dict.fromkeys((T - 1, 0, None))]
SELF_IDS = [f"{T}x{dv}-hot{hot}" for T, dv, hot in SELF_RUNS]
