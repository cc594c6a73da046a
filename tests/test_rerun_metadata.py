"""k_spec_rerun's shape, read from the built library's gfx950 code object (no
GPU needed).  The launch sits between every two searches of a lane and
usually finds no key; beside the other lane's k_spec<8> blocks (4 workgroups
of ~40 KB of LDS and 8 waves per SIMD of 64 VGPRs on each CU) it is dispatched
at once only while a block of it needs no LDS and no more than the wave slots
and registers one ended k_spec workgroup frees: one wave, no static LDS, no
scratch, and at most the 128 VGPRs that workgroup's two waves on a SIMD held.
An edit that grows any of them fails no GPU test, only the timeline."""
import pytest

from helpers import code_object_kernels as _kernels

NAMES = [f"_ZN3lcd12k_spec_rerunILb{e16}ELb{ex}EEEvNS_6T0ArgsE" for e16 in (0, 1) for ex in (0, 1)]


@pytest.mark.parametrize("name", NAMES)
def test_rerun_is_one_wave_without_lds_or_scratch(tmp_path, name):
    ks = _kernels(tmp_path)
    assert name in ks, f"{name} not in the code object"
    k = ks[name]
    assert k["group_segment_fixed_size"] == 0, f"{name}: {k}"
    assert k["max_flat_workgroup_size"] == 64, f"{name}: {k}"
    assert k["private_segment_fixed_size"] == 0, f"{name}: {k}"


@pytest.mark.parametrize("name", NAMES)
def test_rerun_fits_where_one_spec_workgroup_ended(tmp_path, name):
    """k_spec<8> keeps 2 waves of 64 VGPRs on each SIMD per workgroup."""
    k = _kernels(tmp_path)[name]
    assert -(-k["vgpr_count"] // 8) * 8 <= 128, f"{name}: {k}"
