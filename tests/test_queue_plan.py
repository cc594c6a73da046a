"""csrc/queue_plan.hpp on the CPU, through tests/queue_plan_main.cpp: the
default table of lc_queue_check at the row counts around one workgroup and at
2^31 rows, what an asked-for slot count becomes, and the byte cap's refusal.
Expected values follow from the rules stated in that header."""
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
CAP = 8 << 30


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("queue_plan") / "plan_main")
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "queue_plan_main.cpp"), "-o", out], check=True, timeout=120)
    return out


def run(exe, text):
    r = subprocess.run([exe], input=text, capture_output=True, text=True, check=True, timeout=60)
    return [[int(x) for x in line.split()] for line in r.stdout.strip().split("\n")]


def test_constants_are_what_launch_info_reports(exe):
    out = np.zeros(4, np.int64)
    N.check(N.lib().lc_queue_launch_info(N.ptr(out, C.c_int64)))
    block, slot_bytes, per_row, cap = run(exe, "consts\n")[0]
    assert out.tolist() == [block, per_row, slot_bytes, cap] == [256, 2, 16, CAP]


@pytest.mark.parametrize("n, slots", [(0, 256), (1, 256), (127, 256), (128, 256), (129, 512), (1000, 2048), (1024, 2048),
                                      (1025, 4096)])
def test_default_slots(exe, n, slots):
    """The next power of two at or above 2 n, and one workgroup's worth at least."""
    assert run(exe, f"default {n}\n") == [[slots, 16 * slots, 1, slots // 256]]


def test_the_byte_cap(exe):
    # 2^28 rows: a default table of 2^29 slots is the cap itself; one row more doubles it
    assert run(exe, f"default {1 << 28}\n") == [[1 << 29, CAP, 1, 1 << 21]]
    assert run(exe, f"default {(1 << 28) + 1}\n")[0][:3] == [1 << 30, 2 * CAP, 0]
    assert run(exe, f"default {1 << 31}\n")[0][:3] == [1 << 32, 64 << 30, 0]
    assert run(exe, f"default {(1 << 62) + 5}\n")[0][2] == 0  # no overflow on the way to the refusal
    assert run(exe, f"slots {1 << 29} 5\nslots {1 << 30} 5\n") == [[1 << 29, 1], [1 << 30, 0]]


def test_asked_for_slots(exe):
    """A power of two at least the row count, else refused; 0 is the default."""
    asks = [(0, 300, 1024), (512, 300, 512), (256, 300, 0), (384, 300, 0), (1, 1, 1), (1, 0, 1), (1, 2, 0), (2, 2, 2), (3, 2, 0)]
    got = run(exe, "".join(f"slots {a} {n}\n" for a, n, _ in asks))
    assert [g[0] for g in got] == [want for _, _, want in asks]
