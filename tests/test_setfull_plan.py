"""sf_band_ids / plan_setfull_step (csrc/setfull_plan.hpp): how a set-full
step lays its keys into passes and bands under the matrix cap, pinned on the
CPU through tests/setfull_plan_main.cpp (host C++ only, no HIP).  Expected
values follow from the rules stated in the header:
  a key's matrix is rows x ceil(ids / 64) 64-bit words;
  a key that fits what is left of the pass is one band there;
  else the widest multiple of 256 ids that fits, the rest in the next pass;
  never narrower than 256 ids: an empty pass takes that band above the cap;
  one mark workgroup per (band, non-empty row, 4,096 elements from the row's
  start rounded down to four), one scan workgroup per (band, 256 ids),
  one count slot per 256 ids of a key's span (at least one per key)."""
import os
import shutil
import subprocess

import pytest

from lincheck import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/llvm/bin/clang++"

pytestmark = pytest.mark.skipif(not shutil.which(CXX), reason="no ROCm clang++")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("setfull_plan") / "setfull_plan_main")
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "jepsen-etcd-demo_amd", "csrc"),
                    os.path.join(ROOT, "tests", "setfull_plan_main.cpp"), "-o", out], check=True, timeout=120)
    return out


def run(exe, text):
    r = subprocess.run([exe], input=text, capture_output=True, text=True, check=True, timeout=60)
    return [list(map(int, line.split())) for line in r.stdout.strip().splitlines()]


def band(exe, rows, ids, words, empty):
    return run(exe, f"band {rows} {ids} {words} {int(empty)}\n")[0][0]


def step(exe, keys, cap):
    text = f"step {len(keys)} {cap}\n" + "".join("%d %d %d %d %d\n" % k for k in keys)
    lines = run(exe, text)
    head = dict(zip("passes segs marks scans n_items max_words total_words".split(), lines[0]))
    at = 1
    passes = [dict(zip("mark0 mark1 scan0 scan1 words".split(), l)) for l in lines[at:at + head["passes"]]]
    at += head["passes"]
    segs = [tuple(l) for l in lines[at:at + head["segs"]]]
    at += head["segs"]
    return head, passes, segs, [l[0] for l in lines[at:]]


@pytest.mark.parametrize("what,args,want", [
    ("nothing left", (10, 0, 1000, 1), 0),
    ("no reads: no matrix, all ids at once", (0, 10 ** 6, 0, 0), 10 ** 6),
    ("fits exactly: 10 rows x 16 words", (10, 1000, 160, 0), 1000),
    ("one word short: 15 words per row are 3 whole workgroups", (10, 1000, 159, 0), 768),
    ("one word more", (10, 1000, 161, 0), 1000),
    ("under one workgroup's words, pass in use: a new pass", (10, 1000, 39, 0), 0),
    ("under one workgroup's words, empty pass: the floor band", (10, 1000, 39, 1), 256),
    ("the floor band is no wider than the key", (10, 100, 19, 1), 100),
    ("a narrow key waits for a new pass too", (10, 100, 19, 0), 0),
    ("a narrow key that fits", (10, 100, 20, 0), 100),
    ("2^20 ids x 256 reads under the default cap: 32 MiB", (256, 1 << 20, (128 << 20) // 8, 1), 1 << 20),
    ("2^24 ids x 256 reads: 512 MiB, bands of 2^22 ids", (256, 1 << 24, (128 << 20) // 8, 1), 1 << 22),
])
def test_band(exe, what, args, want):
    assert band(exe, *args) == want, what


def test_cap_edges(exe):
    """1,000 ids x 10 reads of 100 elements are 160 words = 1,280 bytes."""
    key = [(1000, 0, 10, 100, 0)]
    for cap in (1280, 1288):
        head, passes, segs, base = step(exe, key, cap)
        assert head == dict(passes=1, segs=1, marks=10, scans=4, n_items=4, max_words=160, total_words=160), cap
        assert segs == [(0, 0, 1000, 16, 0)] and base == [0, 4]
    head, passes, segs, base = step(exe, key, 1272)  # one word less: 768 ids, then the other 232 in a pass of their own
    assert head == dict(passes=2, segs=2, marks=20, scans=4, n_items=4, max_words=120, total_words=160)
    assert segs == [(0, 0, 768, 12, 0), (0, 768, 232, 4, 0)]
    assert passes == [dict(mark0=0, mark1=10, scan0=0, scan1=3, words=120), dict(mark0=10, mark1=20, scan0=3, scan1=4, words=40)]


def test_floor_band_passes_the_cap(exe):
    head, passes, segs, _ = step(exe, [(600, 0, 100, 1, 0)], 8)
    assert [s[1:4] for s in segs] == [(0, 256, 4), (256, 256, 4), (512, 88, 2)]
    assert [p["words"] for p in passes] == [400, 400, 200] and head["max_words"] == 400 and head["n_items"] == 3


def test_small_keys_share_a_pass_and_edge_keys(exe):
    keys = [(65, 0, 2, 3, 0),    # 2 words x 2 rows
            (0, 0, 3, 0, 0),     # no ids: no band, one count slot
            (500, 0, 0, 0, 0),   # no reads: a band without a matrix
            (300, 2, 5, 9, 0),   # an error key: nothing
            (64, 0, 1, 64, 0)]
    head, passes, segs, base = step(exe, keys, 1 << 20)
    assert head["passes"] == 1 and passes[0]["words"] == 5
    assert segs == [(0, 0, 65, 2, 0), (2, 0, 500, 0, 4), (4, 0, 64, 1, 4)]
    assert head["marks"] == 2 + 1 and head["scans"] == 1 + 2 + 1
    assert base == [0, 1, 2, 4, 5, 6]


def test_mark_chunks_follow_the_rows_alignment(exe):
    # a row of 4,093 elements from element 3 ends at 4,096: one workgroup from 0
    head, _, _, _ = step(exe, [(100, 0, 1, 4093, 3)], 1 << 20)
    assert head["marks"] == 1
    # one element more: a second workgroup from 4,096
    head, _, _, _ = step(exe, [(100, 0, 1, 4094, 3)], 1 << 20)
    assert head["marks"] == 2
    # three such rows back to back: [3, 4097) from 0 is 2 workgroups, [4097, 8191) from 4096 is 1,
    # [8191, 12285) from 8188 is 2
    head, _, _, _ = step(exe, [(100, 0, 3, 4094, 3)], 1 << 20)
    assert head["marks"] == 5
    # a banded key marks every row once per band
    head, _, segs, _ = step(exe, [(1024, 0, 4, 10, 0)], 4 * 8 * 8)
    assert len(segs) == 2 and head["marks"] == 8


def test_launch_info_matches_the_header():
    out = (N.C.c_int64 * 6)()
    N.check(N.lib().lc_setfull_launch_info(out))
    assert list(out) == [64, 256, 4096, 16, 8192, 128 << 20]
