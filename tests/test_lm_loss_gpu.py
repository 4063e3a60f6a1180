"""The chunked language-model head (csrc/lm_head_ce.hip, iseg_amd/nlp/lm_loss.py, F.lm_head_cross_entropy, GemmaCausalLM.compute_loss) on the
device against the fp64 restatement of tests/lm_loss_ref.py.

Yardstick of the kernel-level parity tests: the COMPOSED route of the parent commit on the same inputs -- F.embedding_logits (bf16 or fp32 logits,
stored whole) followed by F.softmax_ce_per_pixel.  The fused route's error against fp64, in max-norm relative to the oracle's peak, may be at most
1.5 x the composed route's, for the loss, dX and dE.  iseg_softmax_ce_ignore stops at 256 classes (one tile of fp32 logits must fit the LDS), so
for V > 256 the loss kernel of the composed route is replaced by torch's fp32 logsumexp on the SAME stored logits of F.embedding_logits
(`_composed`): the logits are rounded to the compute dtype and dlogits once more, exactly what the composed route rounds.

The gradient-buffer rules of tests/test_grad_contract_gpu.py are restated here for the node, which lives outside iseg_amd/functional.py."""
import os

import pytest
import torch

from tests import gemma_cache_ref as C
from tests import guarded_memory as GM
from tests import lm_loss_ref as R
from tests.test_kernels_gpu import DTYPES, rnd

pytestmark = pytest.mark.gpu

SHAPES = [(5, 0), (256, 256), (1000, 256), (4100, 512)]      # (V, chunk): one chunk; an exact multiple; a tail of 232; a tail of 4


@pytest.fixture
def policy():
    from iseg_amd import nn

    nn.set_device("cuda:0")
    try:
        yield nn
    finally:
        os.environ.pop("ISEG_LMHEAD_FUSED", None)
        nn.set_compute_dtype(torch.float32)


def _table(E, dtype, trainable=True):
    """a table parameter as ParamStore lays it out: fp32 master of the rounded values, compute-dtype shadow"""
    t = torch.nn.Parameter(E.to(dtype).float().cuda(), requires_grad=trainable)
    t.iseg_name, t.iseg_compute = "token_embedding/embeddings", t.data.to(dtype)
    return t


def _width(V, chunk):
    return chunk if chunk > 0 else V


def _case(M, V, chunk, d, dtype, seed=0):
    """hidden ~ N(0, 1) and table ~ N(0, 1 / d) rounded to the compute dtype (logits of standard deviation 1); targets placed row by row: the last
    column of a chunk, the first of the next, the tail's last, a chunk BEFORE the one that holds the row maximum (s is rescaled after z_t was
    taken), a chunk after it, one out of range; weights positive with zeros; a non-unit upstream gradient"""
    x = rnd((M, d), 11 + seed).to(dtype)
    E = rnd((V, d), 12 + seed, d ** -0.5).to(dtype)
    Z = R.logits(x, E)
    top = R.first_argmax(Z)
    c = _width(V, chunk)
    g = torch.Generator().manual_seed(13 + seed)
    t = torch.randint(0, V, (M,), generator=g)
    kinds = {}
    for r in range(M):
        k, tc = r % 7, int(top[r]) // c
        if k == 0:
            t[r] = min(c - 1 + (r // 7 % max(V // c, 1)) * c, V - 1)
        elif k == 1 and V > c:
            t[r] = min(c * (1 + r // 7 % max((V - 1) // c, 1)), V - 1)
        elif k == 2:
            t[r] = V - 1
        elif k == 3 and tc > 0:
            t[r] = (tc - 1) * c + r % c
            kinds["before"] = kinds.get("before", 0) + 1
        elif k == 4 and (tc + 1) * c < V:
            t[r] = min((tc + 1) * c + r % c, V - 1)
            kinds["after"] = kinds.get("after", 0) + 1
        elif k == 5 and M > 7:
            t[r] = V if r % 2 else -1
    w = torch.rand(M, generator=g, dtype=torch.float64).float() + 0.5
    if M > 7:
        w[6::11] = 0.0
    up = (torch.randn(M, generator=g, dtype=torch.float64) * 0.5 + 1.5).float()
    if V > c and M >= 37:
        assert kinds.get("before", 0) >= 1 and kinds.get("after", 0) >= 1, kinds
    return x, E, t, w, up


def _fused(x, E, t, w, up, dtype, chunk, scale=1.0, trainable=True, seed_grad=None, hidden_grad=True):
    from iseg_amd.nlp import lm_loss

    table = _table(E, dtype, trainable)
    if seed_grad is not None:
        table.grad = seed_grad.float().cuda()
    h = x.to(dtype).cuda().requires_grad_(hidden_grad)
    loss, argmax, sums = lm_loss.lm_head_cross_entropy(h, table, t.cuda(), None if w is None else w.cuda(), upstream_scale=scale, chunk=chunk)
    assert loss.dtype == torch.float32 and argmax.dtype == torch.int32 and tuple(loss.shape) == tuple(t.shape)
    node = loss.grad_fn if t.dim() == 1 else loss.grad_fn.next_functions[0][0]      # (a reshape to [...] sits on top for other shapes)
    assert type(node).__name__.startswith("_LmHeadCEFn")
    loss.backward(torch.ones_like(loss) if up is None else up.cuda())
    return {"loss": loss.detach(), "argmax": argmax, "sums": sums, "dX": h.grad, "dE": table.grad, "table": table}


def _composed(x, E, t, w, up, dtype):
    """the parent commit's route: the logits stored whole by F.embedding_logits, then F.softmax_ce_per_pixel -- or, past its 256 classes, torch's
    fp32 logsumexp on the same stored logits.  -> (loss, dX, dE)"""
    from iseg_amd import functional as F

    V = E.shape[0]
    table = _table(E, dtype)
    h = x.to(dtype).cuda().requires_grad_(True)
    td = t.cuda()
    valid = (td >= 0) & (td < V)
    wd = valid.float() if w is None else valid.float() * w.cuda()
    logits = F.embedding_logits(h[None], table)[0]
    if V <= 256:
        per = F.softmax_ce_per_pixel(logits, torch.where(valid, td, torch.full_like(td, -1)), V, -1)
    else:
        lf = logits.float()
        per = torch.logsumexp(lf, dim=-1) - lf.gather(1, td.clamp(0, V - 1)[:, None])[:, 0]
    loss = per * wd
    loss.backward(torch.ones_like(loss) if up is None else up.cuda())
    return loss.detach(), h.grad, table.grad


def _err(got, want):
    return (got.detach().cpu().double() - want).abs().max().item() / max(want.abs().max().item(), 1e-300)


# ---- forward and backward against the oracle --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("d", [64, 72])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"V{v}c{c}" for v, c in SHAPES])
@pytest.mark.parametrize("M", [1, 37, 130])
def test_forward_and_backward_against_fp64(cuda, policy, M, shape, d, dtype):
    """loss, dX and dE (with sample weights, zero weights, targets out of range and a non-unit upstream gradient): the fused route's max-norm error
    relative to the oracle's peak is at most 1.5 x the composed route's on the same inputs.  lse and the three sums to fp32 rounding of a sum of
    M terms; the argmax inside the accepted set; zero-weight rows are exact zeros in the loss and in dX.
    Measured (profiles/lm_head_ce_kbench.md has every case): bf16 loss 3e-9 .. 6e-8 fused against 3e-5 .. 1.2e-3 composed; bf16 dX 1.9e-3 ..
    4.5e-3 and dE 9e-4 .. 2.9e-3 on both routes, equal to the last bf16 rounding in most cases (worst ratio 1.499, dX of 130-V5c0-72-bf16);
    fp32 loss 2e-9 .. 9.4e-8 (3.4e-8 .. 5.8e-8 from 37 rows on) against 1.7e-8 .. 1.5e-7, dX 5e-8 .. 1.0e-6 against 5e-8 .. 1.5e-6, dE 4e-8 ..
    3.0e-7 on both.  The tightest fp32 loss cases are the one-row ones where both routes return the same float (ratio 1)."""
    V, chunk = shape
    policy.set_compute_dtype(dtype)
    x, E, t, w, up = _case(M, V, chunk, d, dtype)
    ref = R.forward(x, E, t, w)
    _, dX, dE = R.backward(x, E, t, w, up)
    got = _fused(x, E, t, w, up, dtype, chunk)
    base = _composed(x, E, t, w, up, dtype)
    line = []
    for name, f, b, want in (("loss", got["loss"], base[0], ref["loss"]), ("dX", got["dX"], base[1], dX), ("dE", got["dE"], base[2], dE)):
        ef, eb = _err(f, want), _err(b, want)
        line.append(f"{name} fused {ef:.3e} composed {eb:.3e}")
        assert torch.isfinite(f).all()
    print(f"M{M} V{V} c{chunk} d{d} {str(dtype)[6:]}: " + "; ".join(line))
    for name, f, b, want in (("loss", got["loss"], base[0], ref["loss"]), ("dX", got["dX"], base[1], dX), ("dE", got["dE"], base[2], dE)):
        assert _err(f, want) <= 1.5 * _err(b, want), name
    assert got["dX"].dtype == dtype and got["dE"].dtype == torch.float32
    dead = ref["w"] == 0
    assert (got["loss"].cpu()[dead] == 0).all() and (got["dX"].cpu()[dead] == 0).all()
    # the sums: fp32 partial sums of M terms that are themselves within the loss tolerance
    sums = got["sums"].cpu().double()
    tol = max(_err(base[0], ref["loss"]), 2.0 ** -22) * 1.5
    assert abs(sums[0] - ref["sums"][0]).item() <= tol * ref["loss"].abs().max().item() * M
    assert abs(sums[2] - ref["sums"][2]).item() <= 2.0 ** -22 * max(ref["sums"][2].item(), 1.0)
    eps = 2 * (d + 1) * 2.0 ** -23 * (x.double().abs() @ E.double().abs().T).max(dim=-1).values
    ok = R.accepted(ref["Z"], eps[:, None])
    idx = got["argmax"].cpu().long()
    assert ((idx >= 0) & (idx < V)).all() and ok[torch.arange(M), idx].all()


def test_large_logits_stay_finite(cuda, policy):
    """rows scaled so that their logits reach +-80 and +-200 (exp(200) is not an fp32 number: the maximum has to be subtracted): loss and lse
    finite, and within the fp32 budget of the oracle's: two logits' accumulation error, (d + 1) roundings of 2^-24 on sum_k |x_k e_k| each,
    plus four ulps of a number below 256 (2^-16) for m + log s and the difference"""
    from iseg_amd import kernels as K

    policy.set_compute_dtype(torch.float32)
    M, V, d, chunk = 8, 1000, 64, 256
    x, E, t, _, _ = _case(M, V, chunk, d, torch.float32, seed=3)
    t = t.clamp(0, V - 1)
    Z = R.logits(x, E)
    peak = torch.tensor([80.0, 200.0] * (M // 2), dtype=torch.float64)
    x = (x * (peak / Z.abs().max(dim=-1).values)[:, None]).float()
    ref = R.forward(x, E, t)
    assert (ref["Z"].abs().max(dim=-1).values - peak).abs().max() < 1e-3
    xd, Ed = x.cuda(), E.float().cuda()
    loss, lse, *_ = K.lm_head_ce_fwd(xd, Ed, t.to(torch.int32).cuda(), None, chunk)
    print(f"loss err {(loss.cpu().double() - ref['loss']).abs().max().item():.3e} lse err {(lse.cpu().double() - ref['lse']).abs().max().item():.3e}")
    assert torch.isfinite(loss).all() and torch.isfinite(lse).all()
    bound = 2 * (d + 1) * 2.0 ** -24 * (x.double().abs() @ E.double().abs().T).max().item() + 4 * 2.0 ** -16
    assert (loss.cpu().double() - ref["loss"]).abs().max().item() <= bound and (lse.cpu().double() - ref["lse"]).abs().max().item() <= bound


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_argmax_is_the_first_maximal_index(cuda, policy, dtype):
    """the row maximum is duplicated bit for bit: for even rows at ids 100 (chunk 0), 600 and 700 (both chunk 2), for odd rows at 520 and 530 (both
    chunk 2): the smallest id is returned, across chunks and inside one.  Every other logit is far below."""
    from iseg_amd import kernels as K

    policy.set_compute_dtype(dtype)
    M, V, d, chunk = 10, 1000, 64, 256
    E = (rnd((V, d), 21, 0.05)).to(dtype)
    x = (rnd((M, d), 22, 0.05)).to(dtype)
    u1, u2 = torch.zeros(d, dtype=dtype), torch.zeros(d, dtype=dtype)
    u1[0], u2[1] = 2.0, 2.0
    for v in (100, 600, 700):
        E[v] = u1
    for v in (520, 530):
        E[v] = u2
    x[0::2, 0], x[0::2, 1], x[1::2, 0], x[1::2, 1] = 4.0, 0.0, 0.0, 4.0
    want = R.first_argmax(R.logits(x, E))
    assert want.tolist() == [100, 520] * 5
    _, _, argmax, match, sums, *_ = K.lm_head_ce_fwd(x.cuda(), E.cuda(), want.to(torch.int32).cuda(), None, chunk)
    assert argmax.cpu().tolist() == want.tolist() and match.cpu().tolist() == [1] * M and sums[1].item() == float(M)
    # one chunk: the same answer
    assert K.lm_head_ce_fwd(x.cuda(), E.cuda(), want.to(torch.int32).cuda(), None, V)[2].cpu().tolist() == want.tolist()


def test_rows_past_the_first_grid_trip(cuda):
    """the chunk kernels take at most 32768 rows per trip of their grid (8192 workgroups of four wavefronts): 32768 + 37 rows of a two-chunk
    vocabulary of 8 + 3 given as fp32 logits directly.  The argmax is exact (the kernels see the oracle's values); loss and lse to four fp32
    roundings of numbers below 8 (2^-21 each); G = softmax - onehot to 2^-21 of its peak of 1; the rows of the second trip are among them"""
    from iseg_amd import kernels as K

    M, w0, w1 = 32768 + 37, 8, 3
    Z = rnd((M, w0 + w1), 71).float()
    t = torch.randint(0, w0 + w1, (M,), generator=torch.Generator().manual_seed(72)).to(torch.int32)
    z0, z1 = Z[:, :w0].contiguous().cuda(), torch.nn.functional.pad(Z[:, w0:], (0, 5)).contiguous().cuda()      # pitches 8 and 8
    state = K.lm_head_ce_state(M, "cuda")
    K.lm_head_ce_chunk_fwd(z0, t.cuda(), state, 0, w0)
    K.lm_head_ce_chunk_fwd(z1, t.cuda(), state, w0, w1)
    loss, lse, match, sums = K.lm_head_ce_finalise(state, t.cuda(), None, w0 + w1)
    Zd = Z.double()
    want_lse = torch.logsumexp(Zd, dim=-1)
    want = want_lse - Zd.gather(1, t.long()[:, None])[:, 0]
    assert torch.equal(state[3].cpu().long(), R.first_argmax(Zd))
    assert (lse.cpu().double() - want_lse).abs().max().item() <= 4 * 2.0 ** -21 and (loss.cpu().double() - want).abs().max().item() <= 4 * 2.0 ** -21
    assert torch.equal(match.cpu().bool(), R.first_argmax(Zd) == t.long())
    assert abs(sums[0].item() - want.sum().item()) <= 2.0 ** -20 * want.sum().item() and sums[2].item() == float(M)
    g = torch.empty((M, 8), dtype=torch.float32, device="cuda")
    K.lm_head_ce_chunk_bwd(z1, state[0], state[1], t.cuda(), None, None, 1.0, g, w0 + w1, w0, w1)
    G = torch.softmax(Zd, dim=-1)
    G[torch.arange(M), t.long()] -= 1.0
    assert (g[:, :w1].cpu().double() - G[:, w0:]).abs().max().item() <= 2.0 ** -21
    assert (g[-37:, :w1].cpu().double() - G[-37:, w0:]).abs().max().item() <= 2.0 ** -21 and g[-37:, :w1].abs().max().item() > 0.01


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("d", [13, 72, 520])
def test_target_logit_is_the_once_rounded_dot_product(cuda, dtype, d):
    """iseg_lm_head_ce_target_logit: z_t = x_r . E[t_r] summed in fp64 and rounded once -- half an ulp of fp32 (2^-24 |z_t|) from the fp64 dot
    product of the stored values; rows whose target lies outside [0, V) keep what the state held.  d = 13 takes the scalar loads, 72 one
    16-byte step on nine lanes, 520 two steps with a partly idle second one"""
    from iseg_amd import kernels as K

    M, V = 37, 29
    x, E = rnd((M, d), 81).to(dtype), rnd((V, d), 82).to(dtype)
    t = torch.randint(0, V, (M,), generator=torch.Generator().manual_seed(83)).to(torch.int32)
    t[3], t[11], t[36] = -1, V, 1 << 30
    state = K.lm_head_ce_state(M, "cuda")
    state[2].fill_(7.0)
    K.lm_head_ce_target_logit(x.cuda(), E.cuda(), t.cuda(), state)
    got = state[2].cpu().double()
    valid = (t >= 0) & (t < V)
    want = (x.double() * E.double()[t.long().clamp(0, V - 1)]).sum(dim=-1)
    assert (got[~valid] == 7.0).all() and int((~valid).sum()) == 3
    order = d * 2.0 ** -52 * (x.double().abs() * E.double().abs()[t.long().clamp(0, V - 1)]).sum(dim=-1)      # two fp64 summation orders
    assert ((got - want).abs()[valid] <= 2.0 ** -24 * want.abs()[valid] + order[valid]).all()


def test_reductions_and_accuracy(cuda, policy):
    """sum loss, sum w match, sum w with weights, zero weights and targets out of range, where half of the valid targets ARE the fp64 argmax"""
    from iseg_amd import kernels as K

    policy.set_compute_dtype(torch.float32)
    M, V, d, chunk = 130, 1000, 64, 256
    x, E, t, w, _ = _case(M, V, chunk, d, torch.float32, seed=5)
    Z = R.logits(x, E)
    top2 = Z.topk(2, dim=-1).values
    clear = (top2[:, 0] - top2[:, 1]) > 1e-3      # rows whose argmax fp32 cannot move
    hit = clear & (torch.arange(M) % 2 == 0) & (t >= 0) & (t < V)
    t = torch.where(hit, R.first_argmax(Z), t)
    ref = R.forward(x, E, t, w, scale=0.25)
    amb = ~clear & ref["match"]
    assert not amb.any()
    loss, _, argmax, match, sums, *_ = K.lm_head_ce_fwd(x.float().cuda(), E.float().cuda(), t.to(torch.int32).cuda(), w.cuda(), chunk, 0.25)
    assert torch.equal(match.cpu().bool()[clear], ref["match"][clear])
    s = sums.cpu().double()
    print(f"sums {s.tolist()} against {ref['sums'].tolist()}")
    # every row's loss carries two logits' accumulation error ((d + 1) roundings of 2^-24 on sum_k |x_k e_k|) times its weight; the sums add fp32 rounding
    per_row = 2 * (d + 1) * 2.0 ** -24 * (x.double().abs() @ E.double().abs().T).max().item() + 4 * 2.0 ** -21
    assert abs(s[0] - ref["sums"][0]).item() <= 0.25 * per_row * ref["sums"][2].item() + 2.0 ** -20 * ref["sums"][0].abs().item()
    assert abs(s[1] - ref["sums"][1]).item() <= 2.0 ** -22 * ref["sums"][1].item() and ref["sums"][1].item() > 10
    assert abs(s[2] - ref["sums"][2]).item() <= 2.0 ** -22 * ref["sums"][2].item()
    assert abs(loss.cpu().double().sum() - s[0]).item() <= 2.0 ** -20 * s[0].abs().item()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_nan_in_one_row_stays_in_that_row(cuda, policy, dtype):
    """a NaN in one row's hidden state: that row's loss is NaN, every other row's loss has the bits of the run without it"""
    policy.set_compute_dtype(dtype)
    M, V, d, chunk = 37, 1000, 64, 256
    x, E, t, w, _ = _case(M, V, chunk, d, dtype, seed=7)
    t, w = t.clamp(0, V - 1), w.clamp(min=0.5)
    clean = _fused(x, E, t, w, None, dtype, chunk)
    x2 = x.clone()
    x2[17, 5] = float("nan")
    dirty = _fused(x2, E, t, w, None, dtype, chunk)
    keep = torch.arange(M) != 17
    assert torch.isnan(dirty["loss"][17]) and torch.isnan(dirty["sums"][0])
    assert torch.equal(dirty["loss"].cpu()[keep].view(torch.int32), clean["loss"].cpu()[keep].view(torch.int32))
    assert torch.isfinite(dirty["dX"].float().cpu()[keep]).all() and torch.isnan(dirty["dX"].float().cpu()[17]).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_two_calls_are_bit_identical(cuda, policy, dtype):
    policy.set_compute_dtype(dtype)
    M, V, d, chunk = 130, 4100, 72, 512
    x, E, t, w, up = _case(M, V, chunk, d, dtype, seed=9)
    a, b = _fused(x, E, t, w, up, dtype, chunk), _fused(x, E, t, w, up, dtype, chunk)
    for k in ("loss", "sums", "dX", "dE", "argmax"):
        assert torch.equal(a[k], b[k]), k


# ---- the gradient-buffer contract, restated for this node -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_gradient_buffer_contract(cuda, policy, dtype):
    """the clauses of tests/grad_contract_cases.py: a frozen table receives nothing and its .grad stays None while dX is still produced; a seeded
    .grad is added to; a frozen hidden state skips dX while dE is right; the errors stay under that table's ceiling of 4e-2 (max-norm relative
    to the oracle's peak)"""
    policy.set_compute_dtype(dtype)
    M, V, d, chunk = 37, 1000, 64, 256
    x, E, t, w, up = _case(M, V, chunk, d, dtype, seed=15)
    _, dX, dE = R.backward(x, E, t, w, up)
    frozen = _fused(x, E, t, w, up, dtype, chunk, trainable=False)
    assert frozen["table"].grad is None and _err(frozen["dX"], dX) <= 4e-2
    seed = rnd((V, d), 16, dE.abs().max().item())
    seeded = _fused(x, E, t, w, up, dtype, chunk, seed_grad=seed)
    assert _err(seeded["dE"].cpu().double() - seed.float().double(), dE) <= 4e-2 and _err(seeded["dX"], dX) <= 4e-2
    nodx = _fused(x, E, t, w, up, dtype, chunk, hidden_grad=False)
    assert nodx["dX"] is None and _err(nodx["dE"], dE) <= 4e-2
    assert torch.equal(nodx["dE"], _fused(x, E, t, w, up, dtype, chunk)["dE"])


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_table_shared_with_the_embedding_lookup(cuda, policy, dtype):
    """hidden = F.embedding(ids, table, 3) feeds the head that reads the same table: its one gradient buffer holds the sum of both contributions
    (fp64 autograd through both uses), to the ceiling of 4e-2; the lookup's part alone is far from the total"""
    from iseg_amd import functional as F

    policy.set_compute_dtype(dtype)
    M, V, d, chunk = 37, 1000, 64, 256
    _, E, t, w, up = _case(M, V, chunk, d, dtype, seed=17)
    ids = torch.randint(0, V, (M,), generator=torch.Generator().manual_seed(18))
    scale = float(torch.tensor(3.0).to(dtype))
    Ea = E.double().clone().requires_grad_(True)
    h = Ea[ids] * scale
    if dtype == torch.bfloat16:
        h = h + (h.detach().to(dtype).double() - h.detach())      # the lookup's output is rounded to the compute dtype; straight through
    valid = (t >= 0) & (t < V)
    per = torch.logsumexp(h @ Ea.T, dim=-1) - (h @ Ea.T).gather(1, t.clamp(0, V - 1)[:, None])[:, 0]
    (per * valid.double() * w.double() * up.double()).sum().backward()
    table = _table(E, dtype)
    hd = F.embedding(ids.cuda(), table, 3.0)
    loss = F.lm_head_cross_entropy(hd, table, t.cuda(), w.cuda(), chunk=chunk)
    loss.backward(up.cuda())
    e = _err(table.grad, Ea.grad)
    print(f"shared table gradient error {e:.3e}")
    assert e <= 4e-2
    head_only = R.backward(h.detach(), E, t, w, up)[2]
    assert _err(head_only, Ea.grad) > 4e-2


# ---- guard bands ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_inside_guard_bands(cuda, policy, dtype):
    """V = 1000 in chunks of 256 (the tail of 232 is where an overrun would land): every operand, the state, Z_c, G_c, the fp32 dX buffer, the
    outputs, the table's gradient and the exact-size scratch buffer lie between poisoned bands at addresses = 16 (mod 512).  The bands stay
    intact and the results are the bits of the unguarded call"""
    from iseg_amd.nlp import lm_loss

    policy.set_compute_dtype(dtype)
    M, V, d, chunk = 37, 1000, 64, 256
    x, E, t, w, up = _case(M, V, chunk, d, dtype, seed=19)
    plain = _fused(x, E, t, w, up, dtype, chunk)
    arena = GM.Arena("cuda:0", 32 << 20)
    with GM.guarded(arena) as scope:
        def put(src, role="operand"):
            dst = arena.alloc(src.shape, src.dtype, role)
            dst.copy_(src)
            return dst

        table = torch.nn.Parameter(put(E.to(dtype).float()))
        table.iseg_name, table.iseg_compute = "token_embedding/embeddings", put(E.to(dtype))
        if dtype == torch.float32:
            table.iseg_compute = table.data
        table.grad = put(torch.zeros(V, d), "output")
        h = put(x.to(dtype)).requires_grad_(True)
        loss, argmax, sums = lm_loss.lm_head_cross_entropy(h, table, put(t.to(torch.int32)), put(w), chunk=chunk)
        loss.backward(put(up))
        arena.check()
        assert any(r.role == "workspace" and r.end - r.start == 12 for r in arena.records)      # one record of three sums for 37 rows
        for k, v in (("loss", loss.detach()), ("argmax", argmax), ("sums", sums), ("dX", h.grad), ("dE", table.grad)):
            assert torch.equal(v, plain[k]), k
    assert scope.refused_from is None


# ---- memory --------------------------------------------------------------------------------------------------------------------------------------------
def test_peak_memory_is_bounded_by_the_chunk(cuda, policy):
    """M = 130, V = 4100, d = 64, chunk = 512, bf16: the peak of forward + backward above the inputs and the gradient buffers stays under the
    design's  M Vc (4 + 2) + 2 M d 4  bytes (Z_c, G_c, the fp32 dX buffer and its cast) plus ten fp32 / int32 vectors of M rows, times 2 for the
    allocator's rounding -- and the composed route (the stored logits) does not"""
    policy.set_compute_dtype(torch.bfloat16)
    M, V, d, chunk = 130, 4100, 64, 512
    x, E, t, w, up = _case(M, V, chunk, d, torch.bfloat16, seed=23)
    bound = 2 * (M * chunk * (4 + 2) + 2 * M * d * 4 + 10 * 4 * M)

    def peak(run):
        run()      # the stream's workspace and the library's caches exist before the measurement
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        table = _table(E, torch.bfloat16)
        table.grad = torch.zeros(V, d, device="cuda")
        h, td, wd, ud = x.to(torch.bfloat16).cuda().requires_grad_(True), t.cuda(), w.cuda(), up.cuda()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        run(table, h, td, wd, ud)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base - M * d * 2      # h.grad is a gradient buffer

    def fused(table=None, h=None, td=None, wd=None, ud=None):
        from iseg_amd import functional as F

        if table is None:
            return _fused(x, E, t, w, up, torch.bfloat16, chunk)
        F.lm_head_cross_entropy(h, table, td, wd, chunk=chunk).backward(ud)

    def composed(table=None, h=None, td=None, wd=None, ud=None):
        from iseg_amd import functional as F

        if table is None:
            return _composed(x, E, t, w, up, torch.bfloat16)
        lf = F.embedding_logits(h[None], table)[0].float()
        ((torch.logsumexp(lf, dim=-1) - lf.gather(1, td.clamp(0, V - 1)[:, None])[:, 0]) * wd).backward(ud)

    pf, pc = peak(fused), peak(composed)
    print(f"peak bytes above inputs and gradient buffers: fused {pf}, composed {pc}, bound {bound}")
    assert pf <= bound < pc


# ---- model level ----------------------------------------------------------------------------------------------------------------------------------------
def test_compute_loss_fused_against_composed(cuda, policy):
    """the tiny Gemma of tests/test_gemma_cache_gpu.py in bf16 (vocabulary 97: F.softmax_ce_per_pixel takes it): compute_loss on the chunked head
    against ISEG_LMHEAD_FUSED=0, with sample weights.  The per-token loss, the accuracy and every parameter's gradient differ by at most 2 x the
    composed route's own distance from fp64 autograd on the rounded weights (relative Frobenius norms, the idiom of tests/test_gemma_gpu.py);
    after one SGD step on each (lr 0.5, on the summed-over-batch-size loss) the losses still agree to that bound.
    Measured: loss 1.1e-4 fused-composed against 6.2e-4 composed-fp64; gradients 6e-4 .. 7.8e-3 against 8.7e-3 .. 1.8e-2; after the step 1.1e-3
    against 1.8e-3; the three accuracies are equal"""
    from tests.test_gemma_cache_gpu import B, GEOM, S, _model, _prompts

    policy.set_compute_dtype(torch.bfloat16)
    ids, _ = _prompts()
    y = torch.roll(ids, shifts=-1, dims=1)
    pad = torch.ones(B, S, dtype=torch.int32)
    sw = (torch.rand(B, S, generator=torch.Generator().manual_seed(31)) + 0.5) * (torch.arange(S) < S - 3)
    inputs = {"token_ids": ids.cuda(), "padding_mask": pad.cuda()}
    lr = 0.5

    def fp64(w):
        wr = {k: v.clone().requires_grad_(True) for k, v in w.items()}
        logits = C.causal_lm(ids, pad, wr, *GEOM, act_dtype=torch.bfloat16)
        per = torch.nn.functional.cross_entropy(logits.reshape(B * S, -1), y.reshape(-1), reduction="none").reshape(B, S) * sw.double()
        (per.sum() / (B * S)).backward()
        acc = (sw.double() * (logits.argmax(dim=-1) == y)).sum() / sw.double().sum()
        return per.detach(), acc.item(), {k: v.grad for k, v in wr.items()}

    def device(mode):
        os.environ["ISEG_LMHEAD_FUSED"] = mode
        model, w = _model(torch.bfloat16)
        for p in model.parameters():
            p.grad = None
        per, metrics = model.compute_loss(inputs, y.cuda(), sw.cuda(), reduction="none", with_metrics=True)
        (per.sum() / (B * S)).backward()
        grads = {p.iseg_name: p.grad.detach().cpu().double() for p in model.parameters()}
        scalar = model.compute_loss(inputs, y.cuda(), sw.cuda()).item()
        assert abs(scalar - per.sum().item() / (B * S)) <= 1e-5 * abs(scalar)
        with torch.no_grad():
            for p in model.parameters():
                p.data.add_(p.grad, alpha=-lr)
        model._iseg_store.sync_shadow()
        with torch.no_grad():
            after = model.compute_loss(inputs, y.cuda(), sw.cuda(), reduction="none")
        return per.detach().cpu().double(), metrics["sparse_categorical_accuracy"].item(), grads, after.cpu().double(), w

    def rel(a, b):
        return (a - b).norm().item() / max(b.norm().item(), 1e-300)

    lf, af, gf, nf, w = device("1")
    lc, ac, gc, nc, _ = device("0")
    lr64, ar, gr = fp64(w)
    stepped = {k: (v - lr * gr[k]).to(torch.bfloat16).double() for k, v in w.items()}
    nr, _, _ = fp64(stepped)
    print(f"loss: fused-composed {rel(lf, lc):.3e}, composed-fp64 {rel(lc, lr64):.3e}, fused-fp64 {rel(lf, lr64):.3e}; accuracy {af} {ac} {ar}")
    assert rel(lf, lc) <= 2 * rel(lc, lr64)
    assert abs(af - ac) <= 2 * abs(ac - ar)
    for k in gr:
        print(f"{k}: fused-composed {rel(gf[k], gc[k]):.3e}, composed-fp64 {rel(gc[k], gr[k]):.3e}")
    for k in gr:
        assert rel(gf[k], gc[k]) <= 2 * rel(gc[k], gr[k]), k
    print(f"after the step: fused-composed {rel(nf, nc):.3e}, composed-fp64 {rel(nc, nr):.3e}")
    assert rel(nf, nc) <= 2 * rel(nc, nr)
    assert nr.sum().item() < lr64.sum().item()      # the step went downhill
