"""The case table of tests/grid_trips.py on the host: every entry's mirrored launcher arithmetic gives at least two full trips plus a
ragged third at its chosen shape, every case stays inside the size budget, every entry has its GPU test, and the table module itself
stays importable without torch."""
import ast
import os
import subprocess
import sys

import pytest

from tests import grid_trips as GT

HERE = os.path.dirname(os.path.abspath(__file__))
IDS = [f"{c.name}-{d}" for c, d, _ in GT.variants()]


@pytest.mark.parametrize("case,dtype,shape", GT.variants(), ids=IDS)
def test_two_full_trips_plus_a_ragged_third(case, dtype, shape):
    trips = case.launcher(dtype, **shape)
    assert trips, "an entry mirrors at least one kernel launch"
    for t in trips:
        assert t.grid >= 1 and t.per_trip == t.grid * t.quantum
        ok = case.name in GT.BOUNDARY_OK      # (an item count that is a multiple of the workgroup quantum by construction: stated in the table)
        assert not GT.violations(t, ok), f"{case.name} [{dtype}] {shape}: {t}: {GT.violations(t, ok)}"
        first = GT.first_of_last_trip(t)
        assert 2 * t.per_trip <= first < t.items


@pytest.mark.parametrize("case,dtype,shape", GT.variants(), ids=IDS)
def test_case_stays_inside_the_size_budget(case, dtype, shape):
    assert 0 < case.elements(dtype, **shape) <= GT.BUDGET, f"{case.name} [{dtype}]: {case.elements(dtype, **shape)} fp32 units"


def test_every_entry_names_its_launcher_and_is_unique():
    names = [c.name for c in GT.CASES]
    assert len(set(names)) == len(names)
    for c in GT.CASES:
        assert c.wrapper and ".hip" in c.source and c.cap, c.name
        assert set(c.shapes) <= {"f32", "bf16"} and c.shapes, c.name
        assert c.source.split(":")[0].split(" ")[0] in os.listdir(os.path.join(os.path.dirname(HERE), "iseg_amd", "csrc")), c.source


def test_every_entry_has_a_gpu_test_and_every_gpu_test_an_entry():
    with open(os.path.join(HERE, "test_grid_trips_gpu.py")) as f:
        tree = ast.parse(f.read())
    tests = {n.name[len("test_"):] for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}
    assert tests == set(GT.BY_NAME), (sorted(set(GT.BY_NAME) - tests), sorted(tests - set(GT.BY_NAME)))


def test_the_table_does_not_need_torch():
    code = "import sys; from tests import grid_trips; assert 'torch' not in sys.modules, 'grid_trips imported torch'"
    subprocess.run([sys.executable, "-c", code], cwd=os.path.dirname(HERE), check=True)


def test_the_rule_itself():
    ok = GT.trip(2048, 256, 2 * 2048 * 256 + 300, tail=5)
    assert not GT.violations(ok) and GT.first_of_last_trip(ok) == 2 * 2048 * 256
    assert GT.violations(GT.trip(2048, 256, 2 * 2048 * 256))                    # no ragged trip
    assert GT.violations(GT.trip(2048, 256, 2 * 2048 * 256 + 512))              # the ragged trip ends on a workgroup boundary
    assert GT.violations(GT.trip(2048, 256, 2048 * 256 + 300))                  # one full trip only
    assert GT.violations(GT.trip(2048, 256, 2 * 2048 * 256 + 300, tail=0))      # no scalar tail
