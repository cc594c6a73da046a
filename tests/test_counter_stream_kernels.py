"""The streaming counter kernels' resources, read from
libcounter_stream_kernels.so's code object (no GPU): which kernels the library
holds, that none of them has scratch, and their VGPR and LDS figures as
DESIGN.md section 3.17 records them.  liblincheck.so links the library by its
own directory and holds none of its kernels; libcounter_kernels.so keeps its
nine.  Metadata only."""
import os
import subprocess

import pytest

from test_counter_kernels import code_object_kernels, named
from test_occupancy import LDS_PER_CU, LLVM, SO

KERNEL_LIB = os.path.join(os.path.dirname(SO), "libcounter_stream_kernels.so")
# stem -> its instantiations (events per thread), or None for a plain kernel
KERNELS = {"k_cs_patch": None, "k_cs_tile": (1, 8), "k_cs_carry": None, "k_cs_apply": (1, 8), "k_cs_commit": None,
           "k_cs_judge": None, "k_cs_gather": None, "k_cs_results": None}
CASES = [(stem, ipt) for stem, ipts in KERNELS.items() for ipt in (ipts or (None,))]


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return code_object_kernels(KERNEL_LIB, tmp_path_factory.mktemp("counter_stream_kernels"))


def test_the_library_holds_exactly_the_stream_kernels(kernels):
    assert len(kernels) == len(CASES) == 10, sorted(kernels)
    assert len({named(kernels, s, i) for s, i in CASES}) == 10


@pytest.mark.parametrize("stem, ipt", CASES)
def test_kernel_resources(kernels, stem, ipt):
    """No scratch and no spills; at most 128 VGPRs and an eighth of the CU's
    LDS per workgroup, tests/test_counter_kernels.py's bar: four workgroups of
    four waves stay resident on a CU, each lane with its events' loads in
    flight -- what kernels that only stream need."""
    name = named(kernels, stem, ipt)
    k = kernels[name]
    print(stem, ipt, k)
    assert k["private_segment_fixed_size"] == 0 and k.get("vgpr_spill_count", 0) == 0, f"{name}: {k}"
    assert k["vgpr_count"] <= 128, f"{name}: {k}"
    assert 8 * k["group_segment_fixed_size"] <= LDS_PER_CU, f"{name}: {k}"


def test_the_figures_design_records(kernels):
    """DESIGN.md 3.17's table is this build's."""
    text = open(os.path.join(os.path.dirname(__file__), "..", "DESIGN.md")).read()
    for stem, ipt in CASES:
        k = kernels[named(kernels, stem, ipt)]
        label = f"`{stem}<{ipt}>`" if ipt else f"`{stem}`"
        row = f"| {label} | {k['vgpr_count']} | {k['group_segment_fixed_size']} | 0 |"
        assert row in text, row


def test_liblincheck_links_it_and_holds_none_of_its_kernels(tmp_path):
    out = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-d", SO], check=True, capture_output=True, text=True).stdout
    assert "libcounter_stream_kernels.so" in out and "$ORIGIN" in out
    assert not [n for n in code_object_kernels(SO, tmp_path) if "k_cs_" in n]
    other = tmp_path / "one_shot"
    other.mkdir()
    one_shot = code_object_kernels(os.path.join(os.path.dirname(SO), "libcounter_kernels.so"), other)
    assert len(one_shot) == 9 and not [n for n in one_shot if "k_cs_" in n]
