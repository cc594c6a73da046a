"""plan_step's rerun grid (csrc/step_plan.hpp StepPlan::rerun_grid): the
one-wave workgroups of k_spec_rerun.  Wave b of that launch works in slot b of
the step's K * segs k_spec workspaces, so the grid must never pass them; the
launch is in every step and usually finds no key, so the grid is a small
constant, whatever the chip's size.  Checked on the CPU through
tests/rerun_plan_main.cpp (host C++ only)."""
import itertools
import os
import shutil
import subprocess

import pytest

from lincheck import _native as N
from test_step_plan import BASE, CXX, IN_FIELDS, ROOT

pytestmark = pytest.mark.skipif(not shutil.which(CXX), reason="no ROCm clang++")

KS = (0, 1, 2, 5, 31, 32, 33, 100, 1000, 1024, 1025, 12500, 349526)
CUS = (64, 256, 304)
VARIANTS = {
    "verdicts": dict(),
    "segs 2": dict(spec_segs=2),
    "segs 4": dict(spec_segs=4),
    "finals": dict(want_final=1, want_n_final=1),
    "unvalidated": dict(validated=0),
    "SPEC_OFF": dict(path_flags=N.LC_PATH_SPEC_OFF),
    "peaks": dict(want_peak=1),
}
ROWS = [(v, K, cu) for v in VARIANTS for K in KS for cu in CUS]


@pytest.fixture(scope="module")
def grids(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rerun_plan") / "rerun_plan_main")
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "jepsen-etcd-demo_amd", "csrc"),
                    os.path.join(ROOT, "tests", "rerun_plan_main.cpp"), "-o", exe], check=True, timeout=120)
    text = "".join(" ".join(str(int(dict(BASE, **VARIANTS[v], K=K, cu_count=cu)[f])) for f in IN_FIELDS) + "\n"
                   for v, K, cu in ROWS)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, check=True, timeout=60)
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(ROWS)
    return {row: tuple(map(int, line.split())) for row, line in zip(ROWS, lines)}


def test_some_rows_take_the_speculative_path(grids):
    assert any(spec for spec, _, _, _ in grids.values()) and not all(spec for spec, _, _, _ in grids.values())


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_grid_is_at_least_one_and_within_the_workspace_slots(grids, variant):
    for K, cu in itertools.product(KS, CUS):
        spec, segs, grid, bound = grids[(variant, K, cu)]
        assert grid >= 1, (K, cu)
        assert 1 <= bound <= 1024
        if spec:
            assert segs >= 2
            assert grid <= K * segs, (K, cu, segs, grid)  # a workspace slot per wave
            assert grid == min(bound, K), (K, cu, grid)   # and no wave without a key
        else:
            assert grid == 1, (K, cu, grid)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_grid_does_not_follow_the_chip_size(grids, variant):
    """The same batch on a smaller or larger chip gets the same rerun grid
    (the segments per key, which follow cu_count, do not enter it)."""
    for K in KS:
        got = {grids[(variant, K, cu)][2] for cu in CUS if grids[(variant, K, cu)][0]}
        assert len(got) <= 1, (K, got)
    # and a chip of any size takes the full bound for a batch of many keys
    for cu in CUS:
        spec, _, grid, bound = grids[(variant, 1000, cu)]
        if spec:
            assert grid == bound
