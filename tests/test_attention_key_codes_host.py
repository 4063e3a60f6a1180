"""Pins the key-coded attention inputs of tests/attention_key_codes.py (CPU only), so that tests/test_attention_key_codes_gpu.py cannot pass
vacuously: for every GPU case the ties and gaps are the intended ones, invisible keys do out-score rows, the suite's fp64 restatements agree
with the closed form, a restatement with the kernels' rounding points gives bf16(reference) bit for bit and gradients inside the derived
bounds -- and the mask errors that the relative Frobenius bounds of the existing tests let through change bf16 values here."""
import itertools

import pytest
import torch

from tests import attention_key_codes as AK

PREFILL_IDS = [AK.ident(e) for e in AK.PREFILL]
DECODE_IDS = [AK.ident(e) for e in AK.DECODE]
SELF_RUNS, SELF_IDS = AK.SELF_RUNS, AK.SELF_IDS


def _pin(p):
    """the checks every case gets -> the reference"""
    live = p.live
    assert bool(live.any())
    gaps = p.gap_units[live & (p.gap_units < 10 ** 6)]      # (a row with one visible key has no runner-up)
    gap = float(gaps.min()) * p.unit if gaps.numel() else float("inf")
    assert gap >= 64, gap
    hidden_marked = (p.marked & p.present)[:, None, :] & ~p.vis                       # [B, Tq, S]
    if bool((hidden_marked.any(-1)[..., None] & live).any()):
        assert bool(p.outscored.any()), "no row is out-scored by a key it must not see"
    ref = AK.reference(p)
    assert all(torch.isfinite(t).all() for t in ref)
    closed_err = (ref[0] - p.closed_form).abs().max().item()
    assert closed_err <= 1e-20, closed_err
    # the quantities the bounds are formed from are the reference's: their gradients are its gradients
    for name, a, r in zip(("dq", "dk", "dv"), AK.gradients_of(p, *AK.fp64_parts(p)), ref[1:]):
        assert (a - r).abs().max().item() <= 1e-9 * max(r.abs().max().item(), 1.0), name
    if bool(((p.count == 2) & live).any()):
        assert ref[1].abs().max().item() > 0 and ref[2].abs().max().item() > 0, "a tie must make dq and dk non-zero"
    got = AK.restate_with_kernel_rounding(p)
    assert torch.equal(got[0], AK.bf16_round(ref[0])), AK.changed_rows(got[0], ref[0])
    frac = []
    for name, a, r, b in zip(("dq", "dk", "dv"), got[1:], ref[1:], AK.bounds(p, ref)):
        f = ((a - r).abs() / b).max().item()
        frac.append(f"{name} {f:.2f}")
        assert f <= 1.0, (name, f)
    # the same with the matrix cores' aligned accumulation: still inside the bounds, whose dv term for it is then what holds the cancelled entries
    aligned = AK.restate_with_kernel_rounding(p, mfma="aligned")
    assert torch.equal(aligned[0], got[0])
    for name, a, r, b in zip(("dq", "dk", "dv"), aligned[1:], ref[1:], AK.bounds(p, ref)):
        f = ((a - r).abs() / b).max().item()
        frac.append(f"{name} aligned {f:.2f}")
        assert f <= 1.0, (name, f)
    over = (aligned[3] - ref[3]).abs() > AK.dv_bound_without_accumulation(ref)
    frac.append(f"(dv entries past 2^-8 |ref| + 1e-12 under aligned accumulation: {int(over.sum())})")
    empty = ~p.vis.any(-1)
    unseen = AK.unseen_keys(p)
    for t in (got, aligned):
        assert t[2][unseen].abs().sum().item() == 0 and t[3][unseen].abs().sum().item() == 0 and t[1][empty].abs().sum().item() == 0
    assert got[0][empty].abs().sum().item() == 0 and got[1][empty].abs().sum().item() == 0
    assert got[2][unseen].abs().sum().item() == 0 and got[3][unseen].abs().sum().item() == 0
    composed = AK.restate_with_kernel_rounding(p, score_bf16=True)
    print(f"min gap {gap:.1f}, largest |score| {p.max_score:.0f}, out-scored rows {int(p.outscored.sum())} of {int(live.sum())}, "
          f"reference - closed form {closed_err:.1e}, fraction of the bounds " + " ".join(frac)
          + f", bf16-rounded scores reproduce out: {torch.equal(composed[0], AK.bf16_round(ref[0]))}")
    return ref, torch.equal(composed[0], AK.bf16_round(ref[0]))


@pytest.mark.parametrize("entry", AK.PREFILL, ids=PREFILL_IDS)
def test_prefill_construction(entry):
    _, same = _pin(AK.prefill(*entry))
    assert same == (AK.ident(entry) in AK.COMPOSED_EXACT)


@pytest.mark.parametrize("entry", AK.DECODE, ids=DECODE_IDS)
def test_decode_construction(entry):
    p = AK.decode(*entry)
    _, same = _pin(p)
    assert same == (AK.ident(entry) in AK.COMPOSED_EXACT)
    nvis = p.pos0 + p.q.shape[1]
    assert torch.isnan(p.cache[:, :, nvis + 2:]).all() and torch.isfinite(p.cache[:, :, :nvis + 2]).all()
    assert bool(p.marked[:, nvis:nvis + 2].all())


@pytest.mark.parametrize("run", SELF_RUNS, ids=SELF_IDS)
def test_self_attention_construction(run):
    _, same = _pin(AK.self_attention(*run))
    assert same


def _normal_like(p, seed=1):
    """the existing tests' kind of input at the Problem's shape: N(0, 1), bf16-rounded, the same visibility"""
    gen = torch.Generator().manual_seed(seed)
    r = AK.SimpleNamespace(**vars(p))
    for name in ("q", "k", "v", "dout"):
        setattr(r, name, AK.bf16_round(torch.randn(getattr(p, name).shape, generator=gen)))
    if p.kind == "self":
        r.q, r.k = AK.bf16_round(r.q * 0.35), AK.bf16_round(r.k * 0.35)
    return r


def _groups(entries, key):
    return [list(g) for _, g in itertools.groupby(sorted(entries, key=key), key=key)]


MASKED = ([("prefill", g) for g in _groups(AK.PREFILL, lambda e: (e[0], e[1]))] + [("decode", g) for g in _groups(AK.DECODE, lambda e: e[0][:7])])


@pytest.mark.parametrize("kind,group", MASKED, ids=[k + "-" + AK.ident(g[0][:2] if k == "prefill" else (g[0][0][:7],)) for k, g in MASKED])
def test_mask_errors_change_bf16_values(kind, group):
    """each mask error, applied to the restatement: on the coded inputs it changes the bf16 output of at least one (token, head) row -- in this case,
    or in the case of the same shape and mask whose hot key is placed for it; on N(0, 1) inputs of that shape its relative Frobenius error is
    printed next to the 1.5e-2 the existing tests allow"""
    seen = {}
    for entry in group:
        p = AK.prefill(*entry) if kind == "prefill" else AK.decode(*entry)
        want = AK.reference(p)[0]
        normal = _normal_like(p)
        base = AK.reference(normal, p.vis)[0]
        for name, vis in AK.corruptions(p).items():
            rows = AK.changed_rows(AK.reference(p, vis)[0], want)
            restated = AK.changed_rows(AK.restate_with_kernel_rounding(p, vis)[0], want)
            frob = AK.rel_frobenius(AK.reference(normal, vis)[0], base)
            print(f"{AK.ident(entry)}: {name}: {rows} rows change on coded inputs ({restated} with the kernels' rounding); "
                  f"relative Frobenius error on N(0, 1) inputs {frob:.1e} ({'passes' if frob < 1.5e-2 else 'fails'} 1.5e-2)")
            assert (rows > 0) == (restated > 0)
            seen[name] = max(seen.get(name, 0), rows)
    for name, rows in seen.items():
        assert rows > 0, name


@pytest.mark.parametrize("run", [r for r in SELF_RUNS if r[0] > 1], ids=[i for r, i in zip(SELF_RUNS, SELF_IDS) if r[0] > 1])
def test_next_sample_leak_changes_bf16_values(run):
    """a self-attention row of sample 0 that also sees the first key of sample 1"""
    p = AK.self_attention(*run)
    want = AK.reference(p)[0][:1]
    rows = AK.changed_rows(AK.reference(AK.next_sample_leak(p))[0], want)
    normal = _normal_like(p)
    frob = AK.rel_frobenius(AK.reference(AK.next_sample_leak(normal))[0], AK.reference(normal)[0][:1])
    print(f"{rows} of {run[0]} rows change on coded inputs; relative Frobenius error on N(0, 1) inputs {frob:.1e} "
          f"({'passes' if frob < 1.5e-2 else 'fails'} 1.5e-2)")
    assert rows > 0


def test_aligned_accumulation_leaves_a_grid_unit_where_the_integers_cancel():
    """why the dv bound carries an accumulation term: at 1x130x8x1x256 with the hot key 64, dv of key 23 is (1 - 0.5 - 1.5 + 2 - 1) + (2 - 2) = 0
    beside one e^-64 term of -1.6e-28 in columns 0, 3, 6, ..  The instruction that adds 2 - 2 - 1.6e-28 returns -2^-23, one unit of the grid of
    its largest addend, for every negative term below the grid (an MI355X returned -2^-23 there): past 2^-8 |ref| + 1e-12, inside the bound with the accumulation term.  Exact accumulation stays inside both."""
    p = AK.prefill(*AK.PREFILL[0])
    ref = AK.reference(p)
    narrow, wide = AK.dv_bound_without_accumulation(ref), AK.bounds(p, ref)[2]
    exact = AK.restate_with_kernel_rounding(p)[3]
    aligned = AK.restate_with_kernel_rounding(p, mfma="aligned")[3]
    assert bool(((exact - ref[3]).abs() <= narrow).all())
    assert abs(ref[3][0, 23, 0, 0].item()) < 1e-25 and -2.0 ** -21 <= aligned[0, 23, 0, 0].item() <= -2.0 ** -23
    over = (aligned - ref[3]).abs() > narrow
    assert bool(over[0, 23, 0, 0::3].all()) and bool((ref[3][over].abs() < 1e-25).all())
    assert bool(((aligned - ref[3]).abs() <= wide).all())
