"""The exact set tier's kernels in the library's code object
(csrc/device_stream_set_exact.hip), and every other kernel's metadata against
the parent's as profiles/stream_exact_set_metadata.json records it: the new
translation unit must leave k_stream_set, k_stream_migrate, k_stream,
k_stream_exact, k_stream_final and the rest as they were -- which kernels share
a module changes their register allocation."""
import json
import os

from helpers import code_object_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "stream_exact_set_metadata.json")
SET_EXACT = "_ZN3lcd18k_stream_set_exactENS_18StreamSetExactArgsE"
SET_FINAL = "_ZN3lcd18k_stream_set_finalENS_18StreamSetExactArgsE"
SHORT = {"vgpr_count": "vgpr", "group_segment_fixed_size": "lds", "private_segment_fixed_size": "private"}


def test_the_exact_set_kernels_code_objects(tmp_path):
    """Both are 256-thread workgroups whose sets live in device memory: no
    private segment, no spills, VGPRs and LDS no more than the recorded build's
    (k_stream_set_exact: k_stream_set's ~0.8 KB of descriptors and counters
    plus one 64-bit word per wave; k_stream_set_final: those four words)."""
    ks = code_object_kernels(tmp_path)
    prof = json.load(open(PROFILE))
    assert SET_EXACT in ks and SET_FINAL in ks, [k for k in ks if "stream" in k]
    assert sorted(prof["new_kernels"]) == [SET_EXACT, SET_FINAL]
    for name in (SET_EXACT, SET_FINAL):
        rec = prof["new_kernels"][name]
        assert rec["private"] == 0 and rec["vgpr_spill"] == 0 and rec["sgpr_spill"] == 0, rec
        assert ks[name]["private_segment_fixed_size"] == 0, ks[name]
        assert ks[name]["max_flat_workgroup_size"] == 256, ks[name]
        assert ks[name]["vgpr_count"] <= rec["vgpr"] <= 64, (ks[name], rec)   # 8 waves per SIMD stay possible
        assert 0 < ks[name]["group_segment_fixed_size"] <= rec["lds"] <= 1024, (ks[name], rec)
    assert prof["new_kernels"][SET_FINAL]["lds"] == 32


def test_every_parent_kernel_keeps_its_metadata(tmp_path):
    ks = code_object_kernels(tmp_path)
    prof = json.load(open(PROFILE))
    assert prof["kernels_of_the_parent_that_differ"] == []
    # stronger, as recorded: each of the parent's units' device code is byte for byte what it was
    assert prof["units_of_the_parent_whose_device_text_differs"] == []
    assert all(v["head"] == v["parent"] for v in prof["device_text_sha256"].values())
    assert prof["parent_kernels"] == len(prof["kernels"]) and prof["head_kernels"] == prof["parent_kernels"] + 2
    assert set(ks) == set(prof["kernels"]) | set(prof["new_kernels"]), sorted(set(ks) ^ (set(prof["kernels"]) | set(prof["new_kernels"])))
    for frag in ("k_stream_setENS", "k_stream_migrateENS", "8k_streamENS", "k_stream_exactENS", "k_stream_finalENS"):
        assert any(frag in k for k in prof["kernels"]), frag
    for name, rec in prof["kernels"].items():
        assert rec["same"] and rec["head"] == rec["parent"], name
        for field, short in SHORT.items():
            assert ks[name][field] == rec["parent"][short], f"{name}: {field} {ks[name][field]}, the parent's {rec['parent'][short]}"
