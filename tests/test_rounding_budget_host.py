"""The rounding-budget statistic of tests/rounding_budget.py on the host: for every case of every family the fp32 restatement, rounded once with
.to(torch.bfloat16), meets the four conditions the device test asserts (so a device failure cannot be blamed on an unattainable threshold), and
each of the three mutants of a correct kernel -- a truncating store, slab sums kept in bf16, an intermediate rounded to bf16 -- misses them (so
the statistic cannot quietly stop discriminating).  All three mutants pass close() of tests/test_kernels_gpu.py at its bf16 tolerance, which is
checked here too."""
import pytest
import torch

from tests import rounding_budget as R
from tests.test_kernels_gpu import close

restated = R.restated      # computed once per case, shared by the tests below, never modified


def test_ideal_rounding_is_one_nearest_even_rounding():
    one = torch.tensor([1.0, -1.0], dtype=torch.float64)
    ulp = 2.0 ** -7
    ties = torch.cat([one * (1 + 0.5 * ulp), one * (1 + 1.5 * ulp)])                    # between even|odd and odd|even neighbours
    assert torch.equal(R.ideal_bf16(ties).double(), torch.cat([one, one * (1 + 2 * ulp)]))
    # a value just above a tie that fp32 rounds ONTO the tie: a conversion through fp32 would then pick the even neighbour below
    v = torch.tensor([1 + 0.5 * ulp + 2.0 ** -30], dtype=torch.float64)
    assert R.ideal_bf16(v).double().item() == 1 + ulp and v.to(torch.bfloat16).double().item() == 1.0
    z = torch.tensor([0.0, -0.0, 3.0, 0.40625], dtype=torch.float64)
    assert torch.equal(R.ideal_bf16(z).double(), z)
    st = R.rounding_stats(torch.tensor([-0.0, 0.0, 3.0, 0.40625], dtype=torch.bfloat16), z)
    assert st.share == 1.0 and st.max_abs_e == 0.0, "+0 and -0 are the same output"


def test_ulp_floor_counts_near_zero_outputs_in_a_typical_elements_ulp():
    want = torch.cat([torch.full((255,), 1.0, dtype=torch.float64), torch.tensor([1e-6], dtype=torch.float64)])
    got = want.clone()
    got[-1] = 0.0
    e = R.errors_in_ulps(got.to(torch.bfloat16), want)
    assert abs(e[-1].item()) < 1e-2 and R.rounding_stats(got.to(torch.bfloat16), want).share < 1.0      # tiny error, still not the ideal element


@pytest.mark.parametrize("c", R.CASES, ids=lambda c: c.id)
def test_restatement_meets_the_device_conditions(c):
    for name, (b16, ref, _) in restated(c).items():
        st = R.rounding_stats(b16, ref)
        bad = R.failures(st, ref.numel(), c.family, R.family_max_e(c.family), c.independent())
        assert not bad, R.report(f"{c.id}:{name} (fp32 restatement)", b16, ref, st) + "\n" + "; ".join(bad)
        # (tier 1 with fp32 sampling coordinates: the written figure of R.FP32_COORDINATES instead of 1e-3, for the reason given there)
        assert c.tier == 2 or st.max_abs_e <= R.FP32_COORDINATES.get(c.family, 0.5 + 1e-3), f"{c.id}:{name}: the restatement itself is {st.max_abs_e:.4f} ulp off"


@pytest.mark.parametrize("c", R.CASES, ids=lambda c: c.id)
def test_mutants_miss_the_device_conditions(c):
    skipped = R.MUTANTS_SKIPPED.get(c.family, {})
    floor = R.share_floor(c.family)
    for name, (b16, ref, r32) in restated(c).items():
        n = ref.numel()
        nb = min(n, c.independent() or n)
        rmax = R.family_max_e(c.family)
        for mutant, got in R.mutants(r32).items():
            if mutant in skipped:
                continue
            st = R.rounding_stats(got, ref)
            what = f"{c.id}:{name} {mutant}: share {st.share:.4f} max|e| {st.max_abs_e:.3f} bias_mag {st.bias_mag:+.4f}"
            close(got, ref, torch.bfloat16, what)      # the gap: the existing tolerance does not see the mutant
            assert st.share < floor and st.share <= 0.95, what
            assert R.failures(st, n, c.family, rmax, c.independent()), what
            if mutant == "truncate":
                # the bias bound grows with 1 - share, so it is taken at the lowest share that still meets condition 1: no kernel that passes
                # on share can carry a truncating store's bias
                assert abs(st.bias_mag) > R.bias_bound(nb, floor), what
            if mutant == "bf16_partials":
                if c.family not in R.UNSTORED_MAX_E:      # (there condition 2 has no cap, and share alone convicts the mutant)
                    assert st.max_abs_e > R.max_e_bound(rmax) and st.max_abs_e > 0.75, what


def test_every_budget_entry_is_backed_by_the_restatement():
    assert set(R.BUDGET) == set(R.FAMILIES)
    for family in R.FAMILIES:
        n = same = 0
        for c in R.family_cases(family):
            for b16, ref, _ in restated(c).values():
                n += ref.numel()
                same += round(R.rounding_stats(b16, ref).share * ref.numel())
        recomputed = same / n
        assert recomputed >= R.BUDGET[family], f"{family}: the restatement reaches {recomputed:.6f}, BUDGET says {R.BUDGET[family]}"
        assert 1 - R.BUDGET[family] <= 1.5 * (1 - recomputed) + 1 / n, f"{family}: BUDGET {R.BUDGET[family]} is slack against {recomputed:.6f}"


def test_unstored_max_e_is_backed_by_the_restatement():
    """the written figure is at least what the restatement shows and at most 1.5 x its excess over 1/2 ulp"""
    for family, written in R.UNSTORED_MAX_E.items():
        measured = R.measured_max_e(family)
        assert measured > 0.75, f"{family}: the restatement is faithfully rounded ({measured:.3f}); the family does not belong in UNSTORED_MAX_E"
        assert measured <= written <= 0.5 + 1.5 * (measured - 0.5), f"{family}: written {written}, the restatement shows {measured:.4f}"
        assert all(c.tier == 2 for c in R.family_cases(family))


def test_fp32_coordinate_families_are_the_sampling_kernels_and_need_their_allowance():
    assert set(R.FP32_COORDINATES) <= {"dcnv3", "dcnv3_bwd", "defattn", "defattn_bwd"} and all(0.5 < v <= 0.53 for v in R.FP32_COORDINATES.values())
    for family in R.FP32_COORDINATES:
        assert R.measured_max_e(family) > 0.5 + 1e-3, f"{family}: the restatement meets the 1e-3 of the other tier-1 families; drop the entry"
        assert all(c.tier == 1 for c in R.family_cases(family))


def test_every_family_is_tiered_and_every_skip_is_explained():
    for family in R.FAMILIES:
        tiers = {c.tier for c in R.family_cases(family)}
        assert len(tiers) == 1 and tiers <= {1, 2}, f"{family}: cases of tiers {tiers}"
    for family, skips in R.MUTANTS_SKIPPED.items():
        assert family in R.BUDGET and set(skips) <= {"truncate", "bf16_partials", "double_rounding"} and all(skips.values())
    for c in R.CASES:
        assert not any(k in c.id for k in ("bit_identical", "refuses", "reproducib", "run_to_run", "graphed", "graph_replay"))


def test_share_floors_are_the_ones_derived_from_the_budget():
    assert R.share_floor("cast") == 1.0 and R.share_floor("elementwise_exact") == 1.0
    assert 0.998 <= R.share_floor("gemm_fwd") and 0.998 <= R.share_floor("layernorm")
    assert 0.98 <= R.share_floor("gelu_approx") < 0.99
    assert all(R.share_floor(f) >= 0.95 for f in R.FAMILIES)
    assert R.max_e_bound(0.5005) == pytest.approx(0.504) and R.max_e_bound(0.9) == 0.75 and R.max_e_bound(0.4) == 0.5
