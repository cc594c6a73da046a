"""The queue kernels' resources, read from libqueue_kernels.so's code object (no
GPU): which kernels the library holds, that none of them has scratch, and their
VGPR and LDS figures as DESIGN.md section 3.15 records them.  liblincheck.so
links the library by its own directory and holds none of its kernels.  Metadata
only."""
import os
import subprocess

import pytest

from test_counter_kernels import code_object_kernels
from test_occupancy import LDS_PER_CU, LLVM, SO

KERNEL_LIB = os.path.join(os.path.dirname(SO), "libqueue_kernels.so")
KERNELS = ("k_queue_reset", "k_queue_tally", "k_queue_classify")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return code_object_kernels(KERNEL_LIB, tmp_path_factory.mktemp("queue_kernels"))


def named(kernels, stem):
    """The kernel `stem` by its mangled name."""
    tag = f"{len(stem)}{stem}E"
    hit = [n for n in kernels if tag in n]
    assert len(hit) == 1, (tag, sorted(kernels))
    return hit[0]


def test_the_library_holds_exactly_the_queue_kernels(kernels):
    assert len(kernels) == len(KERNELS), sorted(kernels)
    assert len({named(kernels, s) for s in KERNELS}) == len(KERNELS)


@pytest.mark.parametrize("stem", KERNELS)
def test_kernel_resources(kernels, stem):
    """No scratch and no spills.  At most 128 VGPRs and an eighth of the CU's
    LDS per workgroup, the bar tests/test_counter_kernels.py sets for kernels
    that stream: four workgroups of four waves stay resident on a CU, which is
    what hides the latency of the tally's dependent loads (slot word, then the
    representative row's key and value)."""
    name = named(kernels, stem)
    k = kernels[name]
    print(stem, k)
    assert k["private_segment_fixed_size"] == 0 and k.get("vgpr_spill_count", 0) == 0, f"{name}: {k}"
    assert k["vgpr_count"] <= 128, f"{name}: {k}"
    assert 8 * k["group_segment_fixed_size"] <= LDS_PER_CU, f"{name}: {k}"


def test_the_figures_design_records(kernels):
    """DESIGN.md 3.15's table is this build's."""
    text = open(os.path.join(os.path.dirname(__file__), "..", "DESIGN.md")).read()
    for stem in KERNELS:
        k = kernels[named(kernels, stem)]
        row = f"| `{stem}` | {k['vgpr_count']} | {k['group_segment_fixed_size']} | 0 |"
        assert row in text, row


def test_liblincheck_links_it_and_holds_none_of_its_kernels(tmp_path):
    out = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-d", SO], check=True, capture_output=True, text=True).stdout
    assert "libqueue_kernels.so" in out and "$ORIGIN" in out
    assert not [n for n in code_object_kernels(SO, tmp_path) if "k_queue" in n]
