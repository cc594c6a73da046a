"""The streaming queue kernels' resources, read from
libqueue_stream_kernels.so's code object (no GPU): which kernels the library
holds, that none of them has scratch, and their VGPR and LDS figures as
DESIGN.md section 3.16 records them.  liblincheck.so links the library by its
own directory and holds none of its kernels; libqueue_kernels.so keeps its
three.  Metadata only."""
import os
import subprocess

import pytest

from test_counter_kernels import code_object_kernels
from test_occupancy import LDS_PER_CU, LLVM, SO

KERNEL_LIB = os.path.join(os.path.dirname(SO), "libqueue_stream_kernels.so")
KERNELS = ("k_qs_tally", "k_qs_settle", "k_qs_gather", "k_qs_rehash", "k_qs_entries")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return code_object_kernels(KERNEL_LIB, tmp_path_factory.mktemp("queue_stream_kernels"))


def named(kernels, stem):
    """The kernel `stem` by its mangled name."""
    tag = f"{len(stem)}{stem}E"
    hit = [n for n in kernels if tag in n]
    assert len(hit) == 1, (tag, sorted(kernels))
    return hit[0]


def test_the_library_holds_exactly_the_stream_kernels(kernels):
    assert len(kernels) == len(KERNELS), sorted(kernels)
    assert len({named(kernels, s) for s in KERNELS}) == len(KERNELS)


@pytest.mark.parametrize("stem", KERNELS)
def test_kernel_resources(kernels, stem):
    """No scratch and no spills; at most 128 VGPRs and an eighth of the CU's
    LDS per workgroup, tests/test_queue_kernels.py's bar: four workgroups of
    four waves stay resident on a CU, which hides the latency of the tally's
    dependent loads (state word, then the slot's or the row's identity)."""
    name = named(kernels, stem)
    k = kernels[name]
    print(stem, k)
    assert k["private_segment_fixed_size"] == 0 and k.get("vgpr_spill_count", 0) == 0, f"{name}: {k}"
    assert k["vgpr_count"] <= 128, f"{name}: {k}"
    assert 8 * k["group_segment_fixed_size"] <= LDS_PER_CU, f"{name}: {k}"


def test_the_figures_design_records(kernels):
    """DESIGN.md 3.16's table is this build's."""
    text = open(os.path.join(os.path.dirname(__file__), "..", "DESIGN.md")).read()
    for stem in KERNELS:
        k = kernels[named(kernels, stem)]
        row = f"| `{stem}` | {k['vgpr_count']} | {k['group_segment_fixed_size']} | 0 |"
        assert row in text, row


def test_liblincheck_links_it_and_holds_none_of_its_kernels(tmp_path):
    out = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-d", SO], check=True, capture_output=True, text=True).stdout
    assert "libqueue_stream_kernels.so" in out and "$ORIGIN" in out
    assert not [n for n in code_object_kernels(SO, tmp_path) if "k_qs_" in n]
    other = tmp_path / "one_shot"
    other.mkdir()
    one_shot = code_object_kernels(os.path.join(os.path.dirname(SO), "libqueue_kernels.so"), other)
    assert len(one_shot) == 3 and not [n for n in one_shot if "k_qs_" in n]
