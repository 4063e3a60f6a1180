"""The GEMM-family planner on the MI355X: reduction splits, slab counts, main loops and workspace sizes of tests/gemm_plan_cases.py against the
`mi355x` section of tests/golden/gemm_plans.json (recorded from the library before the planner was gathered into one place).

Nothing is launched: the queries are host functions that only need the device for its CU count and the dynamic-LDS limit of the weight-gradient
LDS-DMA kernels (forms 7 / 8), which is why their plans differ from the `no_device` ones.
"""
import pytest

from tests import gemm_plan_cases as cases

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(bool(cases.knobs_set()), reason=f"{cases.knobs_set()} set: the library reads them once and plans differently")]


@pytest.fixture(scope="module")
def section():
    return cases.golden("mi355x")


def test_every_case_plans_as_recorded(cuda, section):
    hip, lib = cases.load_library()
    bad = cases.mismatches(section, cases.answers(hip, lib))
    assert not bad, f"{len(bad)} plans differ from the recorded ones:\n" + "\n".join(bad[:40])


def test_recorded_table_covers_the_planner(section):
    """read from the recorded table alone, so the list of cases cannot quietly stop reaching a branch of the planner"""
    assert len(section["gemm"]) >= 200 and section["pairs"] and section["conv"]
    nt = cases.variants(section, (1, 1))
    assert {0, 1, 2, 4, 6, 8, 9} <= nt, f"LDS-DMA forms recorded for the K-contiguous orientation: {sorted(nt)}"
    tn = cases.variants(section, (0, 0))
    assert {0, 7, 8} <= tn, f"main loops recorded for the weight-gradient orientation: {sorted(tn)}"
    everything = {row["variant"] for row in section["gemm"].values()}
    assert 3 not in everything and 5 not in everything, "forms 3 and 5 cannot be planned"
    assert any(row["pair_splits"] > 1 for row in section["pairs"].values()), "no pair of weight gradients that shares a launch"
    assert any(row["pair_splits"] == 0 for row in section["pairs"].values())
    assert any(row["splits"] > 1 and row["slabs"] < row["splits"] for row in section["gemm"].values())
    assert any(row["workspace"][3] > 0 for row in section["conv"].values()), "no patch-view weight gradient on the LDS-DMA form"
    assert any(all(row["patch_supported"]) for row in section["conv"].values())
