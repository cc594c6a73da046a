"""The resident set tier's pure rules (csrc/stream_plan.hpp) through
tests/stream_set_plan_main.cpp (host C++ only, no HIP): the set record's
layout, the cap against the least budget a stream accepts, the fallback rule
at its edges; and the new kernels' code objects."""
import os
import re
import shutil
import subprocess

import pytest

from helpers import code_object_kernels
from lincheck import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/llvm/bin/clang++"

pytestmark = pytest.mark.skipif(not shutil.which(CXX), reason="no ROCm clang++")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("stream_set_plan") / "stream_set_plan_main")
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "jepsen-etcd-demo_amd", "csrc"),
                    os.path.join(ROOT, "tests", "stream_set_plan_main.cpp"), "-o", path], check=True, timeout=120)
    return path


def ask(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True, timeout=60)
    rows = [list(map(int, l.split())) for l in out.stdout.strip().splitlines()]
    return rows[0], rows[1], rows[2:]


def test_set_record_layout(exe):
    consts, hdr, rows = ask(exe, ["o 0", "o 1"])
    hdr_words, slots, off_desc, off_s0, off_s1, rec_words, cap, min_budget, slot_bytes, max_slots, max_states = consts
    assert (hdr_words, slots) == (16, 64)              # the header, then one descriptor per window slot
    assert off_desc == hdr_words and off_s0 == off_desc + slots == N.LC_STREAM_SET_HEAD_WORDS
    assert off_s1 == off_s0 + 2 * cap                  # two S arrays of cap u64 configs, 8-byte aligned
    assert rec_words == off_s1 + 2 * cap and off_s0 % 2 == 0 and off_s1 % 2 == 0
    assert slot_bytes == 4 * rec_words                 # a pool slot is one record
    assert rows == [[off_s0], [off_s1]]
    # status, nS, the two pending-slot words, events done, the failing event, the current array
    assert sorted(hdr[:7]) == list(range(7)) and max(hdr[:7]) < hdr_words
    assert hdr[7] == 3                                 # the fallback status, beside live 0 / invalid 1 / error 2
    # the narrow config's reach, as include/lincheck.h has it
    src = open(os.path.join(ROOT, "include", "lincheck.h")).read()
    assert max_slots == int(re.search(r"#define LC_NARROW_MAX_SLOTS\s+(\d+)", src).group(1)) == 56
    assert max_states == int(re.search(r"#define LC_NARROW_MAX_STATES\s+(\d+)", src).group(1)) == 255


def test_cap_is_at_most_the_least_budget_and_holds_a_full_lattice(exe):
    consts, _, _ = ask(exe, [])
    cap, min_budget = consts[6], consts[7]
    assert min_budget == 16 * 64 * 32
    assert cap <= min_budget                           # the exactness argument's premise
    assert cap >= 1024 * 32                            # 1,024 lattice words x 32 states migrate without loss


def test_fallback_rule_at_its_edges(exe):
    consts, _, _ = ask(exe, [])
    cap = consts[6]
    qs = [(cap, cap, 0, 1), (cap + 1, 0, 0, 1), (0, cap + 1, 0, 1), (cap, cap, 55, 255), (1, 1, 56, 1), (1, 1, 55, 1),
          (1, 1, 0, 255), (1, 1, 0, 256), (0, 0, 127, 1), (1 << 33, 0, 0, 1)]
    _, _, rows = ask(exe, [f"f {a} {b} {c} {d}" for a, b, c, d in qs])
    for (n_s, n_i, slot, states), (got,) in zip(qs, rows):
        assert got == int(n_s > cap or n_i > cap or slot >= 56 or states > 255), (n_s, n_i, slot, states)


# ---------------------------------------------------------------- the new kernels' code objects
def test_set_tier_kernels_code_objects(tmp_path):
    """k_stream_migrate is one wave and keeps nothing in LDS; k_stream_set is a
    256-thread workgroup whose sets live in device memory: under 1 KB of LDS
    (descriptors, two candidate lists, counters) and at most 64 VGPRs, so
    neither bounds residency below 8 waves per SIMD.  No scratch in either."""
    ks = code_object_kernels(tmp_path)
    mig, st = "_ZN3lcd16k_stream_migrateENS_13StreamSetArgsE", "_ZN3lcd12k_stream_setENS_13StreamSetArgsE"
    assert mig in ks and st in ks, [k for k in ks if "stream" in k]
    for name in (mig, st):
        assert ks[name]["private_segment_fixed_size"] == 0, ks[name]
        assert ks[name]["vgpr_count"] <= 64, ks[name]
    assert ks[mig]["group_segment_fixed_size"] == 0 and ks[mig]["max_flat_workgroup_size"] == 64, ks[mig]
    assert 0 < ks[st]["group_segment_fixed_size"] <= 1024 and ks[st]["max_flat_workgroup_size"] == 256, ks[st]
