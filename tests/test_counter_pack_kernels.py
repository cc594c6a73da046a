"""The kernels of lc_counter_check_history, read from
libcounter_pack_kernels.so's code object (no GPU): which kernels the library
holds, that none of them has a private segment (no scratch, so no array indexed
per lane) or spills, and that the libraries around it hold none of them.  The
two radix sorts are rocPRIM's: its kernels are in the library too, are not the
project's, and are not held to these figures (DESIGN.md 3.18 says what they are)."""
import os
import subprocess

import pytest

from test_counter_kernels import code_object_kernels
from test_occupancy import LDS_PER_CU, LLVM, SO

LIBDIR = os.path.dirname(SO)
KERNEL_LIB = os.path.join(LIBDIR, "libcounter_pack_kernels.so")
ROWS = ("k_rows_clear", "k_rows_claim", "k_rows_first", "k_rows_ids", "k_rows_gather", "k_rows_link", "k_scan_tile", "k_scan_carry",
        "k_scan_apply")
COUNTER = ("k_cp_takes", "k_cp_classify", "k_cp_kstart", "k_cp_rule3", "k_cp_flags", "k_cp_offsets", "k_cp_scatter", "k_cp_first")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return code_object_kernels(KERNEL_LIB, tmp_path_factory.mktemp("counter_pack_kernels"))


def ours(kernels, stem):
    hit = [n for n in kernels if f"{len(stem)}{stem}E" in n and "rocprim" not in n]
    assert len(hit) == 1, (stem, sorted(kernels))
    return hit[0]


def test_the_library_holds_the_front_end_the_counters_half_and_the_sort(kernels):
    own = {ours(kernels, s) for s in ROWS + COUNTER}
    assert len(own) == len(ROWS) + len(COUNTER) == 17
    rest = set(kernels) - own
    assert rest and all("rocprim" in n for n in rest), sorted(rest)


@pytest.mark.parametrize("stem", ROWS + COUNTER)
def test_kernel_resources(kernels, stem):
    """One lane per row, position or key: no private segment, no spills, at most 128 VGPRs (four
    workgroups of four waves per CU) and an eighth of a CU's LDS at the most."""
    k = kernels[ours(kernels, stem)]
    print(stem, k)
    assert k["private_segment_fixed_size"] == 0 and k.get("vgpr_spill_count", 0) == 0, f"{stem}: {k}"
    assert k["vgpr_count"] <= 128 and 8 * k["group_segment_fixed_size"] <= LDS_PER_CU, f"{stem}: {k}"


def test_liblincheck_links_it_and_the_other_libraries_hold_none_of_its_kernels(tmp_path):
    out = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-d", SO], check=True, capture_output=True, text=True).stdout
    assert "libcounter_pack_kernels.so" in out and "$ORIGIN" in out
    for lib in ("liblincheck.so", "libcounter_kernels.so", "libcounter_stream_kernels.so"):
        d = tmp_path / lib
        d.mkdir()
        names = code_object_kernels(os.path.join(LIBDIR, lib), d)
        assert not [n for n in names if "k_rows_" in n or "k_cp_" in n or "k_scan_" in n or "rocprim" in n], lib
