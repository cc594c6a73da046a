"""csrc/counter_stream_plan.hpp on the CPU, through
tests/counter_stream_plan_main.cpp: the reads array's first capacity and its
doubling up to the byte cap, the refusal of an append that could take the
stream's reads or events to 2^32, the cut of an append larger than one launch,
and k_cs_patch's launch size.  The 2^32 and byte-cap refusals are pinned here
only: no test affords a stream of that size.  Expected values follow from the
rules stated in that header."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from lincheck import _native as N
from lincheck.counter_stream import launch_info

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jepsen-etcd-demo_amd", "csrc")
CXX = shutil.which("g++")

pytestmark = pytest.mark.skipif(not CXX, reason="no g++")
CAP, READ_BYTES, LIMIT = 8 << 30, 33, (1 << 32) - 1
MAX_READS = CAP // READ_BYTES


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("counter_stream_plan") / "plan_main")
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "counter_stream_plan_main.cpp"), "-o", out], check=True, timeout=120)
    return out


def run(exe, text):
    r = subprocess.run([exe], input=text, capture_output=True, text=True, check=True, timeout=60)
    return [[int(x) for x in line.split()] for line in r.stdout.strip().split("\n")]


def test_constants_are_what_launch_info_reports(exe):
    block, read_bytes, cap, max_reads, first, launch, limit = run(exe, "consts\n")[0]
    info = launch_info()
    assert info == dict(block=block, default_tile=2048, read_bytes=read_bytes, max_bytes=cap, default_reads=first, launch_events=launch)
    assert (block, read_bytes, cap, first, launch, limit) == (256, READ_BYTES, CAP, 1 << 16, 1 << 24, LIMIT)
    # a resident read: key id, rank, lower, value, upper, flag
    assert read_bytes == 4 + 4 + 8 + 8 + 8 + 1 and max_reads == MAX_READS and max_reads * read_bytes <= cap < (max_reads + 1) * read_bytes
    assert N.lib().lc_counter_stream_launch_info(None) == -1


def test_first_capacity(exe):
    asks = [(0, 1 << 16), (1, 1), (256, 256), (300, 300), (MAX_READS, MAX_READS), (MAX_READS + 1, 0), ((1 << 32) - 1, 0)]
    assert [g[0] for g in run(exe, "".join(f"first {a}\n" for a, _ in asks))] == [w for _, w in asks]


def test_the_reads_array_doubles_up_to_the_byte_cap(exe):
    asks = [(256, 256, 256), (256, 257, 512), (256, 513, 1024), (300, 301, 600), (1, 5, 8), (0, 3, 4),
            (1 << 26, (1 << 26) + 1, 1 << 27),
            (1 << 27, (1 << 27) + 1, MAX_READS),    # 2^28 reads pass the cap: the doubling is cut at it
            (1 << 27, MAX_READS, MAX_READS),
            (1 << 27, MAX_READS + 1, 0),            # LC_E_NOMEM
            (MAX_READS, MAX_READS, MAX_READS)]
    assert [g[0] for g in run(exe, "".join(f"cap {h} {n}\n" for h, n, _ in asks))] == [w for _, _, w in asks]


def test_the_2_32_refusals(exe):
    asks = [(0, 0, 0, 0, 0), (LIMIT - 1, 0, 1, 1, 0), (LIMIT, 0, 1, 1, 1), (LIMIT - 5, 0, 6, 6, 1), (0, LIMIT, 0, 1, 2),
            (0, LIMIT - 10, 0, 10, 0), (0, LIMIT - 10, 5, 11, 2), (LIMIT, LIMIT, 0, 0, 0), (LIMIT, LIMIT, 1, 1, 1)]
    assert [g[0] for g in run(exe, "".join(f"refuses {a} {b} {c} {d}\n" for a, b, c, d, _ in asks))] == [w for *_, w in asks]


def test_the_events_of_one_launch_and_the_pieces(exe):
    asks = [(0, 256, 1 << 24), (1, 256, 256), (256, 256, 256), (257, 256, 512), (300, 2048, 2048), (4096, 2048, 4096),
            ((1 << 32) - 1, 2048, 1 << 24)]
    assert [g[0] for g in run(exe, "".join(f"launch {a} {t}\n" for a, t, _ in asks))] == [w for *_, w in asks]
    got = run(exe, "pieces 0 256\npieces 1 256\npieces 256 256\npieces 257 256\npieces 1000 256\n")
    assert got == [[0, 0], [1, 0, 1], [1, 0, 256], [2, 0, 256, 257], [4, 0, 256, 512, 768, 1000]]


def test_patch_launch_size(exe):
    # one lane per resident read from the oldest r0 on, and at least one per patch
    got = run(exe, "patch 1000 1000 1\npatch 1000 0 3\npatch 1000 744 2\npatch 1000 743 2\npatch 10 8 5\n")
    assert got == [[1, 1], [1000, 4], [256, 1], [257, 2], [5, 1]]


def test_open_refuses_what_the_plan_refuses():
    h = C.c_void_p()
    for o in (N.LcCounterStreamOpts(100, 0, 0, 0), N.LcCounterStreamOpts(0, MAX_READS + 1, 0, 0), N.LcCounterStreamOpts(0, 0, 0, 1)):
        assert N.lib().lc_counter_stream_open(None, C.byref(o), C.byref(h)) == -1 and not h.value
    out = np.zeros(6, np.int64)
    N.check(N.lib().lc_counter_stream_launch_info(N.ptr(out, C.c_int64)))
    assert out[0] == 256
