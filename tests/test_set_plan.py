"""plan_set_key / plan_set_step (csrc/set_plan.hpp): how a set key's elements
become ids and which tier checks it, pinned on the CPU through
tests/set_plan_main.cpp (host C++ only, no HIP).  Expected values follow from
the rules stated in the header:
  offset ids iff span <= 1024 or 24 * ceil(span / 64) <= 5 * n_add + 4 * n_read;
  LDS tier iff span <= 65,536 (and every key that is not checked);
  an HBM key: ceil(words / 512) classify chunks, ceil(rows / 4096) mark chunks;
  the three bitmaps (24 bytes per word) against the cap."""
import os
import shutil
import subprocess

import pytest

from lincheck import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/llvm/bin/clang++"
I64_MAX = (1 << 63) - 1

pytestmark = pytest.mark.skipif(not shutil.which(CXX), reason="no ROCm clang++")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("set_plan") / "set_plan_main")
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "jepsen-etcd-demo_amd", "csrc"),
                    os.path.join(ROOT, "tests", "set_plan_main.cpp"), "-o", out], check=True, timeout=120)
    return out


def run(exe, text):
    r = subprocess.run([exe], input=text, capture_output=True, text=True, check=True, timeout=60)
    return [list(map(int, line.split())) for line in r.stdout.strip().splitlines()]


def key(exe, any_, mn, mx, n_add, n_read):
    return tuple(run(exe, f"key {int(any_)} {mn} {mx} {n_add} {n_read}\n")[0])


def step(exe, keys, force=0, cap=8 << 30):
    text = f"step {len(keys)} {force} {cap}\n" + "".join("%d %d %d %d\n" % k for k in keys)
    lines = run(exe, text)
    head = dict(zip("rc n_small n_items n_marks bm_words n_words".split(), lines[0]))
    return head, [dict(zip("base item_base chunks hbm".split(), l)) for l in lines[1:]]


@pytest.mark.parametrize("what,args,want", [
    ("no elements", (0, 0, 0, 0, 0), (0, 0)),
    ("one element", (1, 7, 7, 1, 0), (0, 1)),
    ("the floor: 1,024 ids whatever the rows", (1, 0, 1023, 1, 0), (0, 1024)),
    ("one id past the floor, one row", (1, 0, 1024, 1, 0), (1, 0)),
    # 5 * 2000 + 4 * 998 = 13,992 bytes of input = 583 bitmap words of 24 bytes = 37,312 ids
    ("the ratio, inside", (1, 0, 37311, 2000, 998), (0, 37312)),
    ("the ratio, one id more", (1, 0, 37312, 2000, 998), (1, 0)),
    ("the ratio, one byte of input less", (1, 0, 37311, 1999, 999), (1, 0)),
    ("the demo: 5,000 adds twice, read once", (1, 0, 4999, 10000, 5000), (0, 5000)),
    ("negative minimum", (1, -500, 499, 400, 200), (0, 1000)),
    ("{-5, 10^12}", (1, -5, 10 ** 12, 2, 0), (1, 0)),
    ("the whole range: no overflow", (1, -I64_MAX, I64_MAX, 4, 2), (1, 0)),
])
def test_key_rule(exe, what, args, want):
    assert key(exe, *args) == want


def test_lds_tier_limit(exe):
    head, keys = step(exe, [(65536, 0, 100, 50), (65537, 0, 100, 50), (0, 0, 0, 0), (70000, 1, 0, 0)])
    assert [k["hbm"] for k in keys] == [0, 1, 0, 0]
    assert [k["chunks"] for k in keys] == [1, 3, 1, 1]  # 65,537 ids = 1,025 words = 3 chunks of 512
    assert [k["item_base"] for k in keys] == [0, 1, 4, 5] and head["n_items"] == 6
    assert head["n_small"] == 3 and head["n_marks"] == 2
    assert head["bm_words"] == 3 * head["n_words"]


def test_forced_hbm_tier(exe):
    head, keys = step(exe, [(100, 0, 10, 5), (0, 0, 0, 0), (100, 2, 0, 0)], force=1)
    assert [k["hbm"] for k in keys] == [1, 0, 0] and head["n_small"] == 2 and head["n_marks"] == 2


def test_mark_chunks(exe):
    head, _ = step(exe, [(70000, 0, 4097, 4096), (70000, 0, 0, 1)])
    assert head["n_marks"] == 2 + 1 + 0 + 1


def test_no_hbm_key_no_bitmaps(exe):
    head, _ = step(exe, [(65536, 0, 5, 5)] * 4, cap=0)
    assert head["rc"] == 0 and head["bm_words"] == 0


def test_bitmap_cap(exe):
    # 65,537 ids = 1,025 words, padded to 1,026: 24,624 bytes of bitmaps
    assert step(exe, [(65537, 0, 1, 1)], cap=24624)[0]["rc"] == 0
    assert step(exe, [(65537, 0, 1, 1)], cap=24623)[0]["rc"] == -2  # LC_E_NOMEM


def test_bases_even_and_disjoint(exe):
    spans = [64, 65, 1, 999, 128, 0, 129]
    head, keys = step(exe, [(s, 1 if s == 999 else 0, 1, 1) for s in spans])
    assert [k["base"] for k in keys] == [0, 2, 4, 6, 6, 8, 8]
    assert head["n_words"] == 12
    end = 0
    for s, k in zip(spans, keys):
        if s == 999:
            continue
        assert k["base"] % 2 == 0 and k["base"] >= end
        end = k["base"] + -(-s // 64)


def test_header_is_host_only():
    src = open(os.path.join(ROOT, "jepsen-etcd-demo_amd", "csrc", "set_plan.hpp")).read()
    includes = [line.split()[1] for line in src.splitlines() if line.startswith("#include")]
    assert includes == ["<algorithm>", "<cstdint>", "<vector>", '"../../include/lincheck.h"']


def test_launch_info_matches_the_header():
    import ctypes as C
    import numpy as np
    info = np.zeros(7, np.int64)
    N.check(N.lib().lc_set_launch_info(N.ptr(info, C.c_int64)))
    assert info.tolist() == [128, 8192, 32768, 65536, 1024, 4096, 8192]
