"""The register tier's occupancy, read from the built library's gfx950 code
object (no GPU needed).

Round 4 asked the compiler for 8 waves per SIMD on the 8-wave k_spec build
and silently did not get it: a waves-per-SIMD bound that the workgroup's LDS
makes unreachable is dropped, and the build kept 85 VGPRs.  Round 5's 8-wave
and 2-wave builds reach 8 waves per SIMD only while their VGPRs stay at 64
and their LDS lets 4 (8-wave) or 16 (2-wave) workgroups share a CU's 160 KB;
an edit that grows either would lose the occupancy without any test on the
GPU failing (only the time).  So the limits are checked here, in the kernel
descriptors' metadata (llvm-readelf --notes of the offload bundle)."""
import pytest

from helpers import LLVM, SO  # noqa: F401 (test_set_kernels, test_perf_kernels)
from helpers import code_object_kernels as _kernels

LDS_PER_CU = 160 * 1024


def _waves_per_simd(k):
    """Resident waves per SIMD: registers (512 per lane, granule 8) and LDS."""
    vg = max(8, -(-k["vgpr_count"] // 8) * 8)
    by_regs = min(8, 512 // vg)
    waves_per_wg = k["max_flat_workgroup_size"] // 64
    lds = k["group_segment_fixed_size"]
    wg_per_cu = LDS_PER_CU // lds if lds else 32
    by_lds = wg_per_cu * waves_per_wg / 4.0
    return min(by_regs, by_lds)


@pytest.mark.parametrize("name,want", [
    ("_ZN3lcd6k_specILi8ELb1ELb0EEEvNS_6T0ArgsE", 8),  # C2/C5-sized batches: 8 segments, all resident
    ("_ZN3lcd6k_specILi2ELb1ELb0EEEvNS_6T0ArgsE", 8),  # the many-key batches (C3 shards)
    ("_ZN3lcd6k_specILi4ELb1ELb0EEEvNS_6T0ArgsE", 4),
])
def test_spec_builds_keep_their_occupancy(tmp_path, name, want):
    ks = _kernels(tmp_path)
    assert name in ks, f"{name} not in the code object"
    k = ks[name]
    got = _waves_per_simd(k)
    assert got >= want, f"{name}: {got} waves per SIMD ({k}), want {want}"


@pytest.mark.parametrize("name", [
    "_ZN3lcd6k_specILi8ELb1ELb0EEEvNS_6T0ArgsE",  # C2 / C5 (verdict records)
    "_ZN3lcd6k_specILi2ELb1ELb0EEEvNS_6T0ArgsE",  # the C3 shards
    "_ZN3lcd6k_specILi4ELb1ELb0EEEvNS_6T0ArgsE",
])
def test_spec_builds_do_not_spill(tmp_path, name):
    """the 64-VGPR builds held their occupancy by spilling
    to scratch (84 and 148 B per lane; 29.8x and 14.4x the algorithmic HBM
    bytes).  With the workspace rows addressed where used (opq_lane) and the
    key index scalar, no build of the verdict path keeps a private segment."""
    k = _kernels(tmp_path)[name]
    assert k["private_segment_fixed_size"] == 0, f"{name}: {k}"
