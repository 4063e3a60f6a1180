"""The host conditions of tests/sampling_kinks.py, from the fp64 references alone: the restated coordinate lines are the oracles', the fp32
coordinate chain stays within TAU / 4 of fp64 and is exact on the lattice, the class shares the device test relies on (border <= 1 % on the random
cases, >= 1 000 lattice elements per operation, >= 50 on a clip bound, >= 200 separated border elements per near-lattice case), the continuity of
every output but the offset gradient -- and the mutants: a restatement that truncates, takes the other side at an integer, closes the clip bound
or takes its weights from the other corner must miss the rule of tests/test_sampling_kinks_gpu.py on the lattice / near-lattice cases, or be shown
to compute the same function."""
import functools

import pytest
import torch

from oracle import tf_ops as O
from tests import deformable_mhsa_ref as R
from tests import sampling_kinks as S

F32, F64, BF = S.F32, S.F64, S.BF
CASE_DT = [(c, dt) for c in S.CASES for dt in S.DTYPES]
case_dt = pytest.mark.parametrize("case,dtype", CASE_DT, ids=[f"{c.id}-{S._dt(dt)}" for c, dt in CASE_DT])


# ---- the restated lines are the oracles' -----------------------------------------------------------------------------------
def _inside(c, lo, hi):
    f = torch.floor(c)
    return ((f >= lo) & (f + 1 <= hi)).reshape(c.shape[:3] + (-1, 2)).all(dim=-1)      # per tap: both axes


def test_dcnv3_coordinates_are_the_oracles():
    """an image that is a ramp in x (in y), a one-hot mask on tap p: where all four corners lie inside the image the oracle returns px (py) itself.
    The offsets are random, so every tap has been moved by a known amount"""
    N, H, W = 1, 6, 7
    off = S.rnd((N, H, W, 18), 5) * 0.4
    coord = S.dcnv3_coordinates(off, H, W, 1)
    ok = _inside(coord, torch.tensor([1.0, 1.0]).repeat(9), torch.tensor([float(W), float(H)]).repeat(9))
    assert ok.double().mean().item() > 0.3
    ramps = (torch.arange(1, W + 1, dtype=F64).reshape(1, 1, W, 1).expand(N, H, W, 1), torch.arange(1, H + 1, dtype=F64).reshape(1, H, 1, 1).expand(N, H, W, 1))
    for p in range(9):
        m = torch.zeros(N, H, W, 9, dtype=F64)
        m[..., p] = 1.0
        for axis, ramp in enumerate(ramps):
            y = O.dcnv3_op(ramp.contiguous(), off, m, (3, 3), (1, 1), "SAME", (1, 1), 1, 1, 1.0)[..., 0]
            want = coord[..., 2 * p + axis]
            assert (y - want)[ok[..., p]].abs().max().item() < 1e-12


def test_dcnv2_coordinates_are_the_oracles():
    N, H, W = 1, 6, 7
    off = torch.cat([S.rnd((N, H, W, 18), 5) * 0.7, torch.zeros(N, H, W, 9, dtype=F64)], dim=-1)      # logits 0: modulation 1/2
    coord = S.dcnv2_coordinates(off, H, W)
    ok = _inside(coord, torch.tensor([1.0, 1.0]).repeat(9), torch.tensor([float(H), float(W)]).repeat(9))
    assert ok.double().mean().item() > 0.3
    ramps = (torch.arange(1, H + 1, dtype=F64).reshape(1, H, 1, 1).expand(N, H, W, 8), torch.arange(1, W + 1, dtype=F64).reshape(1, 1, W, 1).expand(N, H, W, 8))
    for axis, ramp in enumerate(ramps):
        col = S.dcnv2_oracle_col(ramp.contiguous(), off)[..., 0]      # [N, H, W, 9]
        want = 0.5 * coord.reshape(N, H, W, 9, 2)[..., axis]
        assert (col - want)[ok].abs().max().item() < 1e-12


@pytest.mark.parametrize("dtype", [F32, F64])
def test_deformable_attention_coordinates_are_the_restatements(dtype):
    o = (S.rnd((2, 5, 8, 3 * 3 * 2), 2) * 1.5).to(dtype)
    yu, xu, _, _ = R.sampling_coordinates(o, 5, 8, 3, 3, 2.0)
    assert torch.equal(S.defattn_coordinates(o, 5, 8, 3, 3, 2.0), torch.stack([yu, xu], dim=-1).reshape(o.shape))


@pytest.mark.parametrize("case", [c for c in S.CASES if c.kind != "budget"], ids=lambda c: c.id)
def test_unmutated_restatement_is_the_oracle(case):
    op, ops, p = S.OPS[case.op], S.operands(case, F32), case.p
    want, got = op.run(ops, p), op.run(ops, p, oracle=False)
    for k in want:
        assert (got[k] - want[k]).abs().max().item() <= 1e-12 * want[k].abs().max().item(), k


def test_dcnv2_oracle_passes_the_whole_gradient_at_a_clip_bound():
    """one tap exactly on the bound: pixel (0, 1), tap 0 has gy = 0 + 0 + 0.  tf.clip_by_value (layers/dcn_v2.py:161-172) passes the gradient in
    full there, and so does the kernel (dcn2_tap: gy_u >= 0 && gy_u <= hy).  With d0x = 0, d1x = 1 and the zero ring above the image,
    d col / d gy = sigmoid(0) (x[0, 0] - 0): the WHOLE of it, not the half torch.minimum / torch.maximum would pass at a tie"""
    x = S.rnd((1, 3, 3, 8), 1)
    off = torch.zeros(1, 3, 3, 27, dtype=F64, requires_grad=True)
    S.dcnv2_oracle_col(x, off)[0, 0, 1, 0].sum().backward()
    assert off.grad[0, 0, 1, 0].item() == pytest.approx(0.5 * x[0, 0, 0].sum().item(), rel=1e-12)
    t = torch.zeros(1, dtype=F64, requires_grad=True)
    torch.minimum(torch.maximum(t, torch.zeros(1, dtype=F64)), torch.ones(1, dtype=F64)).sum().backward()
    assert t.grad.item() == 0.5, "torch.maximum no longer splits a tie: the remark in oracle/tf_ops.dcnv2 is out of date"


# ---- TAU and the lattice ------------------------------------------------------------------------------------------------------
@case_dt
def test_fp32_chain_stays_within_a_quarter_of_tau_and_is_exact_on_the_lattice(case, dtype):
    op, ops, cls = S.OPS[case.op], S.operands(case, dtype), S.classes(case, dtype)
    c32 = op.coords(ops, case.p, F32).to(F64)
    assert (c32 - cls.coord).abs().max().item() <= cls.tau / 4
    assert torch.equal(c32[cls.lattice], cls.coord[cls.lattice])
    if case.kind == "lattice":      # the deliberate lattice is the exact one: no element is an integer by an accident of fp64 rounding
        assert torch.equal(cls.lattice, cls.delta == 0) and not cls.border.any()
    assert bool((cls.lattice ^ cls.border ^ cls.interior).all()) and not bool((cls.lattice & cls.border).any())


def test_tau_constants():
    assert (S.R_DCNV3, S.R_DCNV2, S.R_DEFATTN) == (10, 1, 7)
    c = torch.tensor([[-3.0, 12.5]], dtype=F64)
    assert S.tau_of(7, c) == 4 * 7 * 2.0 ** -23 * 12.5 and S.tau_of(1, c * 0.01) == 4 * 2.0 ** -23


# ---- class shares ------------------------------------------------------------------------------------------------------------------
@case_dt
def test_class_shares(case, dtype):
    cls = S.classes(case, dtype)
    sh = S.shares(cls)
    print(f"SHARES {case.id} {S._dt(dtype)} n {sh['n']} lattice {sh['lattice']:.5f} border {sh['border']:.5f} on a clip bound {sh['on_bound']} tau {cls.tau:.3e}")
    if case.kind in ("random", "budget"):
        assert sh["border"] <= S.MAX_BORDER_SHARE
    if case.kind == "budget":
        assert int(cls.interior.sum()) >= 40000      # rounding_budget.MIN_N
    if case.kind == "near":
        ref = S.reference(case, dtype)
        n = int(cls.border.sum())
        assert n >= S.MIN_NEAR, f"only {n} border elements: run this case in fp32 only"
        tol = S.TOL[case.op]["doffset"] * ref.base["doffset"].abs().max().item()
        apart = ((ref.plus - ref.minus).abs()[cls.border] > S.SEPARATION * tol).double().mean().item()
        print(f"SHARES {case.id} {S._dt(dtype)} sides apart by > {S.SEPARATION:.0f} tol on {apart:.4f} of the border elements")
        assert apart >= 0.9


@pytest.mark.parametrize("dtype", S.DTYPES, ids=S._dt)
@pytest.mark.parametrize("op", sorted(S.OPS))
def test_lattice_cases_hold_enough_elements(op, dtype):
    lattice = [S.classes(c, dtype) for c in S.CASES if c.op == op and c.kind == "lattice"]
    for axis in (0, 1):
        assert sum(int(c.lattice[..., axis::2].sum()) for c in lattice) >= S.MIN_LATTICE // 2
    assert sum(int(c.lattice.sum()) for c in lattice) >= S.MIN_LATTICE
    if op != "dcnv3":      # DCNv3 clips indices only
        assert sum(int(c.on_bound.sum()) for c in lattice) >= S.MIN_ON_BOUND
        lo = sum(int((c.on_bound & (c.kink == 0)).sum()) for c in lattice)
        assert 0 < lo < sum(int(c.on_bound.sum()) for c in lattice), "both bounds"


# ---- continuity ------------------------------------------------------------------------------------------------------------------------
@case_dt
def test_every_output_but_the_offset_gradient_is_continuous(case, dtype):
    """between the as-is evaluation and the four one-sided ones the forward output and the other gradients move by O(TAU) x scale: they are held
    everywhere against the as-is reference, no element set aside"""
    ref = S.reference(case, dtype)
    print(f"MOVED {case.id} {S._dt(dtype)} " + " ".join(f"{k} {v:.2f}" for k, v in ref.moved.items()) + " (x TAU x scale)")
    assert all(v <= S.LIPSCHITZ for v in ref.moved.values()), ref.moved
    cls = S.classes(case, dtype)
    same = ~cls.border
    assert torch.equal(ref.plus[same], ref.base["doffset"][same]) and torch.equal(ref.minus[same], ref.base["doffset"][same])


# ---- the rule passes the reference and fails the mutants ----------------------------------------------------------------------------------
def _judge(case, dtype, got):
    ref, cls = S.reference(case, dtype), S.classes(case, dtype)
    _, bad = S.judge_offset_gradient(case, dtype, got["doffset"], ref, cls)
    for k in got:
        if k != "doffset":
            bad += S.judge_continuous(case, dtype, k, got[k], ref, False)[1]
    return bad


@pytest.mark.parametrize("case", [c for c in S.CASES if c.kind != "budget"], ids=lambda c: c.id)
def test_rule_passes_the_fp32_evaluation_of_the_restatement(case):
    """the restatement run in torch.float32 on the same operands meets the rule of the device test in every class: the thresholds are attainable"""
    op = S.OPS[case.op]
    got = op.run(S.operands(case, F32), case.p, oracle=False, dtype=F32)
    assert not _judge(case, F32, got)


# what becomes of each mutant: "caught" = it misses the rule on a lattice or near-lattice case; "same function" = its outputs are bit-identical to
# the unmutated restatement's on every case, with the reason.  old_band: whether the relative-L2 band of 5e-2 (test_dcnv3_gpu.py:45,
# test_deformable_mhsa_gpu.py:72) passes the mutant's offset gradient on every random case
MUTANT_TABLE = {
    ("dcnv3", "trunc"): "caught",
    ("dcnv3", "ceil_minus_1"): "caught",
    ("dcnv3", "strict_clip"): "same function",      # DCNv3 clips no coordinate
    ("dcnv3", "swap_corner"): "same function",      # a clipped corner lies in the zero ring of the padded image: its weight multiplies 0
    ("dcnv2", "trunc"): "same function",            # differs from floor only on negative coordinates: both corners clip to row / column 0, the zero ring, and the gradient mask is 0
    ("dcnv2", "ceil_minus_1"): "caught",
    ("dcnv2", "strict_clip"): "caught",
    ("dcnv2", "swap_corner"): "same function",      # as DCNv3: the clip range IS the padded image
    ("defattn", "trunc"): "same function",          # the coordinate is clipped to [0, H - 1] BEFORE the floor: never negative
    ("defattn", "ceil_minus_1"): "caught",
    ("defattn", "strict_clip"): "caught",
    ("defattn", "swap_corner"): "same function",    # floor of a coordinate in [0, H - 1] is an index inside the image: clipping it changes nothing
}


@functools.lru_cache(maxsize=None)
def _unmutated(case):
    return S.OPS[case.op].run(S.operands(case, F32), case.p, oracle=False)


@pytest.mark.parametrize("op,mutant", sorted(MUTANT_TABLE), ids=lambda v: v)
def test_mutants_miss_the_rule_or_compute_the_same_function(op, mutant):
    cases = [c for c in S.CASES if c.op == op and c.kind != "budget"]
    same, caught_on, old_band = True, [], True
    for c in cases:
        got = S.OPS[op].run(S.operands(c, F32), c.p, mut=mutant, oracle=False)
        base = _unmutated(c)
        same = same and all(torch.equal(got[k], base[k]) for k in got)
        if c.kind == "random":
            old_band = old_band and S.rel_l2(got["doffset"], S.reference(c, F32).base["doffset"]) < 5e-2
        elif _judge(c, F32, got):
            caught_on.append(c.id)
    status = "same function" if same else "caught" if caught_on else "MISSED"
    print(f"MUTANT {op} {mutant}: {status}; fails the rule on {caught_on or 'no case'}; the old 5e-2 L2 band on the random cases {'passes' if old_band else 'fails'} it")
    assert status == MUTANT_TABLE[(op, mutant)]
    if status == "caught":
        kinds = {cid.split("-")[1] for cid in caught_on}
        assert "lattice" in kinds, f"{op} {mutant}: only {caught_on} notice"


# ---- what the layer- and model-level bands measure --------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", sorted(S.OPS))
def test_rounding_the_offsets_on_one_side_alone_gives_errors_of_the_size_of_the_layer_bands(op):
    """the layer tests (0.2 to 0.25) and test_configs_gpu.py (0.22) compare with an oracle whose projected offsets are NOT rounded to bf16, while the
    kernel side's are.  In fp64, with no kernel involved: rounding the offsets of the 2 x 40 x 36 case to bf16 moves a few per mille of the taps
    into another cell, each such offset gradient is wrong by about its own size, so the relative L2 error is about sqrt(2 x that share) -- 0.06 to
    0.17, the size of those bands -- while the continuous outputs move by the bf16 step of the offsets only"""
    c = next(c for c in S.CASES if c.op == op and c.kind == "budget")
    o, ops = S.OPS[op], S._random_operands(op, c.p, F64)
    rounded = dict(ops, offset=ops["offset"].to(BF).to(F64))
    a, b = o.run(ops, c.p), o.run(rounded, c.p)
    share = (torch.floor(o.coords(ops, c.p)) != torch.floor(o.coords(rounded, c.p))).double().mean().item()
    err = {k: S.rel_l2(b[k], a[k]) for k in a}
    print(f"ONE-SIDED {op}: {share:.4f} of the taps change cell; relative L2 " + " ".join(f"{k} {v:.3e}" for k, v in err.items()))
    assert 0.001 < share < 0.01
    assert 0.5 < err["doffset"] / (2 * share) ** 0.5 < 2.0
    assert all(v < err["doffset"] / 5 for k, v in err.items() if k != "doffset")
