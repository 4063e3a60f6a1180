"""The GEMM-family planner without a device: reduction splits, slab counts, main loops and workspace sizes of tests/gemm_plan_cases.py against
the `no_device` section of tests/golden/gemm_plans.json (recorded from the library before the planner was gathered into one place).

The queries never touch the device or their operands; the module still keeps to where no GPU is, because with one the plans are other ones
(the weight-gradient LDS-DMA forms, the real CU count): tests/test_gemm_plan_gpu.py checks those.
"""
import pytest
import torch

from tests import gemm_plan_cases as cases

pytestmark = [pytest.mark.skipif(torch.cuda.is_available(), reason="the no_device plans: with a GPU test_gemm_plan_gpu.py checks the mi355x ones"),
              pytest.mark.skipif(bool(cases.knobs_set()), reason=f"{cases.knobs_set()} set: the library reads them once and plans differently")]


@pytest.fixture(scope="module")
def section():
    return cases.golden("no_device")


def test_every_case_plans_as_recorded(section):
    hip, lib = cases.load_library()
    bad = cases.mismatches(section, cases.answers(hip, lib))
    assert not bad, f"{len(bad)} plans differ from the recorded ones:\n" + "\n".join(bad[:40])


def test_recorded_table_covers_the_planner(section):
    """read from the recorded table alone, so the list of cases cannot quietly stop reaching a branch of the planner"""
    assert len(section["gemm"]) >= 200 and section["pairs"] and section["conv"]
    nt = cases.variants(section, (1, 1))
    assert {0, 1, 2, 4, 6, 8, 9} <= nt, f"LDS-DMA forms recorded for the K-contiguous orientation: {sorted(nt)}"
    everything = {row["variant"] for row in section["gemm"].values()}
    assert 3 not in everything and 5 not in everything, "forms 3 and 5 cannot be planned"
    assert not ({7, 8} & cases.variants(section, (0, 0))), "the weight-gradient LDS-DMA forms need a device"
    fewer = [name for name, row in section["gemm"].items() if row["splits"] > 1 and row["slabs"] < row["splits"]]
    assert fewer, "no split problem whose K range cuts into fewer slabs than splits"
    assert any(row["splits"] > 1 and row["slabs"] == row["splits"] for row in section["gemm"].values())
    assert any(w > 0 for row in section["conv"].values() for w in row["workspace"][:3])
    assert any(row["fwd_kt_supported"] for row in section["conv"].values()) and not all(row["fwd_kt_supported"] for row in section["conv"].values())
