"""csrc/queue_stream_plan.hpp on the CPU, through
tests/queue_stream_plan_main.cpp: the grow rule of a streaming total-queue /
unique-ids' resident table at its edges, the power-of-two result, the byte cap's
refusal, the cut of an append larger than one launch, and the per-key words'
doubling.  Expected values follow from the rules stated in that header."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from lincheck import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jepsen-etcd-demo_amd", "csrc")
CXX = shutil.which("g++")

pytestmark = pytest.mark.skipif(not CXX, reason="no g++")
CAP, MAX_SLOTS = 8 << 30, 1 << 27


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("queue_stream_plan") / "plan_main")
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "queue_stream_plan_main.cpp"), "-o", out], check=True, timeout=120)
    return out


def run(exe, text):
    r = subprocess.run([exe], input=text, capture_output=True, text=True, check=True, timeout=60)
    return [[int(x) for x in line.split()] for line in r.stdout.strip().split("\n")]


def test_constants_are_what_launch_info_reports(exe):
    out = np.zeros(6, np.int64)
    N.check(N.lib().lc_queue_stream_launch_info(N.ptr(out, C.c_int64)))
    block, slot_bytes, per_value, cap, max_slots, first, launch, max_rows, keys0 = run(exe, "consts\n")[0]
    assert out.tolist() == [block, per_value, slot_bytes, cap, first, launch] == [256, 2, 48, CAP, 1 << 16, 1 << 24]
    # the largest power of two of slots within the byte cap; a stream's rows stay below 2^32
    assert max_slots == MAX_SLOTS and max_slots * slot_bytes <= cap < 2 * max_slots * slot_bytes
    assert max_rows == (1 << 32) - 1 and keys0 == 64
    assert N.lib().lc_queue_stream_launch_info(None) == -1


def test_first_slots(exe):
    asks = [(0, 1 << 16), (1, 1), (256, 256), (384, 0), (3, 0), (MAX_SLOTS, MAX_SLOTS), (1 << 28, 0), ((1 << 32) - 1, 0)]
    assert [g[0] for g in run(exe, "".join(f"first {a}\n" for a, _ in asks))] == [w for _, w in asks]


@pytest.mark.parametrize("slots, resident, rows, must, grown", [
    # never overflow: resident + rows against slots -- exactly full, one short of full, one over
    (256, 0, 256, 0, 512), (256, 0, 255, 0, 512), (256, 0, 257, 1, 1024),
    (256, 100, 156, 0, 512), (256, 100, 155, 0, 512), (256, 100, 157, 1, 1024),
    # the load bound on what is resident: 2 x resident against slots -- exactly at it, one short, one over
    (256, 128, 0, 0, 256), (256, 127, 1, 0, 256), (256, 129, 0, 1, 512), (256, 129, 1, 1, 512),
    # an empty append never grows a table within its bound
    (256, 0, 0, 0, 1), (1, 0, 1, 0, 2), (1, 1, 0, 1, 2), (1, 0, 2, 1, 4),
    # the tests' growth case: 255 resident, 257 more
    (256, 255, 257, 1, 1024), (1024, 512, 512, 0, 2048), (1024, 513, 1, 1, 2048),
])
def test_the_grow_rule_at_its_edges(exe, slots, resident, rows, must, grown):
    assert run(exe, f"grow {slots} {resident} {rows}\n") == [[must, grown]]


def test_a_grown_table_is_a_power_of_two_that_restores_the_bound(exe):
    rng = np.random.default_rng(5)
    asks = [(int(r), int(n)) for r, n in zip(rng.integers(0, 1 << 25, 200), rng.integers(0, 1 << 25, 200))]
    got = run(exe, "".join(f"grow 1 {r} {n}\n" for r, n in asks))
    for (r, n), (_, g) in zip(asks, got):
        assert g & (g - 1) == 0 and g >= 2 * (r + n) and (g == 1 or g // 2 < 2 * (r + n)), (r, n, g)


def test_the_byte_cap(exe):
    half = MAX_SLOTS // 2
    # 2 x (resident + rows) is the largest table itself; one more value and the bound cannot be restored:
    # the largest table is taken as long as the append cannot overflow it, then the append is refused
    assert run(exe, f"grow 256 {half - 5} 5\n") == [[1, MAX_SLOTS]]
    assert run(exe, f"grow 256 {half - 5} 6\n") == [[1, MAX_SLOTS]]
    assert run(exe, f"grow 256 {MAX_SLOTS - 5} 5\n") == [[1, MAX_SLOTS]]
    assert run(exe, f"grow 256 {MAX_SLOTS - 5} 6\n") == [[1, 0]]
    assert run(exe, f"grow {MAX_SLOTS} {MAX_SLOTS - 5} 6\n") == [[1, 0]]
    assert run(exe, f"grow {MAX_SLOTS} {(1 << 32) - 2} {(1 << 32) - 1}\n") == [[1, 0]]  # no overflow on the way to the refusal
    # a table at the cap that the append fits is kept past the load bound
    assert run(exe, f"grow {MAX_SLOTS} {MAX_SLOTS - 5} 5\n") == [[1, MAX_SLOTS]]
    assert run(exe, f"grow {MAX_SLOTS} {half} 5\n") == [[0, MAX_SLOTS]]


def test_the_cut_of_an_oversized_append(exe):
    L = 1 << 24
    assert run(exe, f"pieces 0 {L}\n") == [[0, 0]]
    assert run(exe, f"pieces 1 {L}\n") == [[1, 0, 1]]
    assert run(exe, f"pieces {L} {L}\n") == [[1, 0, L]]
    assert run(exe, f"pieces {L + 1} {L}\n") == [[2, 0, L, L + 1]]
    assert run(exe, f"pieces {3 * L - 1} {L}\n") == [[3, 0, L, 2 * L, 3 * L - 1]]
    assert run(exe, f"pieces {(1 << 32) - 1} {L}\n")[0][0] == 256
    assert run(exe, "pieces 10 4\n") == [[3, 0, 4, 8, 10]]


def test_the_per_key_words_double(exe):
    asks = [(0, 1, 64), (0, 64, 64), (0, 65, 128), (64, 64, 64), (64, 65, 128), (64, 300, 512), (128, 129, 256)]
    assert [g[0] for g in run(exe, "".join(f"keys {h} {n}\n" for h, n, _ in asks))] == [w for _, _, w in asks]
