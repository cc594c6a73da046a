"""The kernels of lc_perf_check_history, read from libperf_pack_kernels.so's
code object (no GPU): which kernels the library holds, that none of them has a
private segment (no scratch, so no array indexed per lane) or spills, that the
front end's, the counter's, the sort's and lc_perf_check's kernels stay in
their own libraries, and that liblincheck.so links the library by its own
directory and holds none of its kernels."""
import os
import subprocess

import pytest

from test_counter_kernels import code_object_kernels
from test_occupancy import LDS_PER_CU, LLVM, SO

LIBDIR = os.path.dirname(SO)
KERNEL_LIB = os.path.join(LIBDIR, "libperf_pack_kernels.so")
PACK = ("k_pp_takes", "k_pp_nemesis", "k_pp_build")
FOREIGN = ("k_rows_", "k_scan_", "k_cp_", "k_perf_", "rocprim")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return code_object_kernels(KERNEL_LIB, tmp_path_factory.mktemp("perf_pack_kernels"))


def ours(kernels, stem):
    hit = [n for n in kernels if f"{len(stem)}{stem}E" in n]
    assert len(hit) == 1, (stem, sorted(kernels))
    return hit[0]


def test_the_library_holds_the_three_kernels_and_nothing_else(kernels):
    own = {ours(kernels, s) for s in PACK}
    assert len(own) == 3 and set(kernels) == own, sorted(kernels)
    assert all("k_pp_" in n for n in kernels) and not [n for n in kernels if any(x in n for x in FOREIGN)]


@pytest.mark.parametrize("stem", PACK)
def test_kernel_resources(kernels, stem):
    """One lane per row or position: no private segment, no spills, at most 128 VGPRs (four workgroups
    of four waves per CU) and an eighth of a CU's LDS at the most."""
    k = kernels[ours(kernels, stem)]
    print(stem, k)
    assert k["private_segment_fixed_size"] == 0 and k.get("vgpr_spill_count", 0) == 0, f"{stem}: {k}"
    assert k.get("sgpr_spill_count", 0) == 0, f"{stem}: {k}"
    assert k["vgpr_count"] <= 128 and 8 * k["group_segment_fixed_size"] <= LDS_PER_CU, f"{stem}: {k}"


def test_the_libraries_link_each_other_by_their_own_directory():
    readelf = os.path.join(LLVM, "llvm-readelf")
    out = subprocess.run([readelf, "-d", SO], check=True, capture_output=True, text=True).stdout
    assert "libperf_pack_kernels.so" in out and "$ORIGIN" in out
    out = subprocess.run([readelf, "-d", KERNEL_LIB], check=True, capture_output=True, text=True).stdout
    assert "libcounter_pack_kernels.so" in out and "$ORIGIN" in out


def test_the_other_libraries_hold_none_of_its_kernels(tmp_path):
    for lib in ("liblincheck.so", "libcounter_pack_kernels.so", "libcounter_kernels.so"):
        d = tmp_path / lib
        d.mkdir()
        names = code_object_kernels(os.path.join(LIBDIR, lib), d)
        assert names and not [n for n in names if "k_pp_" in n], lib
