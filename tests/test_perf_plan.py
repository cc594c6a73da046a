"""The pure rules of csrc/perf_plan.hpp (bucket index, quantile index, select
tier, tile window, table layout, digit skipping), pinned on the CPU through
tests/perf_plan_main.cpp (host C++ only, no HIP).  Expected values follow
from the rules stated in DESIGN.md section 3.10 and in the header."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from lincheck import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/llvm/bin/clang++"
QS = (0.5, 0.95, 0.99, 1.0)

pytestmark = pytest.mark.skipif(not shutil.which(CXX), reason="no ROCm clang++")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("perf_plan") / "perf_plan_main")
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "jepsen-etcd-demo_amd", "csrc"),
                    os.path.join(ROOT, "tests", "perf_plan_main.cpp"), "-o", out], check=True, timeout=120)
    return out


def run(exe, text):
    r = subprocess.run([exe], input=text, capture_output=True, text=True, check=True, timeout=60)
    return [list(map(int, line.split())) for line in r.stdout.strip().splitlines()]


@pytest.fixture(scope="module")
def consts(exe):
    return dict(zip("wg tile lds digit share".split(), run(exe, "consts\n")[0]))


@pytest.mark.parametrize("dt", [30 * 10**9, 10 * 10**9, 1000, 1])
def test_bucket_index_at_the_boundaries(exe, dt):
    ts = [k * dt + e for k in (-3, -1, 0, 1, 2, 7) for e in (-1, 0, 1)]
    got = run(exe, "".join(f"bucket {t} {dt}\n" for t in ts))
    for t, (b, mid) in zip(ts, got):
        assert b == t // dt, t  # Python's // floors
        assert mid == b * dt + dt // 2


def test_bucket_equals_jepsens_for_short_runs(exe):
    """(long (/ secs dt)) on doubles equals the integer division on ns while
    the run is short enough for ns -> s to be exact enough: spot values."""
    dt = 30 * 10**9
    for t in (0, 29_999_999_999, 30_000_000_000, 3_600_000_000_001, 86_400 * 10**9 - 1):
        assert run(exe, f"bucket {t} {dt}\n")[0][0] == int((t / 1e9) / 30)


@pytest.mark.parametrize("q", QS)
def test_quantile_index_every_n(exe, q):
    got = run(exe, f"qrange 1 4096 {q!r}\n")[0]
    for n, i in zip(range(1, 4097), got):
        assert i == min(n - 1, math.floor(n * q)), (n, q)
        assert i == min(n - 1, (n * round(q * 100)) // 100), (n, q)  # the exact integer floor, for n < 5000


def test_quantile_index_edges(exe):
    assert run(exe, "qindex 1 0.0\nqindex 10 0.0\nqindex 10 0.3\nqindex 7 1.0\nqindex 1000000007 0.99\n") == \
        [[0], [0], [3], [6], [math.floor(1000000007 * 0.99)]]


def test_tier_at_its_limit(exe, consts):
    L = consts["lds"]
    got = run(exe, "".join(f"tier {n} {f}\n" for f in (0, 1) for n in (0, 1, L - 1, L, L + 1, 1 << 40)))
    assert [g[0] for g in got] == [0, 1, 1, 1, 2, 2, 0, 2, 2, 2, 2, 2]


def test_lds_share_is_derived_from_the_cu(consts):
    """16 bytes a point: the limit's pairs fit a CU's 160 KiB `share` times."""
    assert consts["share"] == (160 * 1024) // (consts["lds"] * 16) >= 4


def test_tile_window(exe, consts):
    T = consts["tile"]
    got = run(exe, "".join(f"tile {b} {b0}\n" for b0 in (0, -5, 10**12) for b in (b0 - 1, b0, b0 + T - 1, b0 + T)))
    assert [g[0] for g in got] == [-1, 0, T - 1, -1] * 3


def test_table_layout(exe):
    # rate [f][3][nr], group [f][nq]
    assert run(exe, "index 0 1 0 7 5\nindex 2 3 6 7 5\nindex 31 2 4 10 5\n") == \
        [[0, 0], [(2 * 3 + 2) * 7 + 6, 2 * 5 + 6], [(31 * 3 + 1) * 10 + 4, 31 * 5 + 4]]


def test_bias_and_skipped_digits(exe, consts):
    """mag = lat < 0 ? ~lat : lat; k = its bit length; latency + 2^k < 2^(k+1)."""
    assert consts["digit"] == 8
    for mag in (0, 1, 254, 255, 256, 2**32 - 1, 2**32, 2**40, 2**62, 2**63 - 1):
        k, live = run(exe, f"bias {mag}\n")[0]
        assert k == mag.bit_length() and live == max(1, -(-(k + 1) // 8))
        for lat in (mag, -mag - 1):
            assert 0 <= lat + (1 << k) < (1 << (k + 1))
    assert run(exe, "dtbits 30000000000\ndtbits 1\ndtbits 256\ndtbits 257\n") == [[35, 5], [0, 1], [8, 1], [9, 2]]


def test_shape(exe):
    S = 10**9
    # 0 records; records but none matched; both; a first bucket that is not 0; negative times
    assert run(exe, f"shape 0 0 0 0 0 0 3 {10 * S} {30 * S}\n")[0] == [0, 0, 0, 0, 0]
    assert run(exe, f"shape 5 0 {12 * S} {41 * S} 0 0 3 {10 * S} {30 * S}\n")[0] == [0, 1, 4, 0, 0]
    assert run(exe, f"shape 5 4 {1 * S} {41 * S} {1 * S} {31 * S} 3 {10 * S} {30 * S}\n")[0] == [0, 0, 5, 0, 2]
    assert run(exe, f"shape 5 4 {95 * S} {99 * S} {94 * S} {95 * S} 3 {10 * S} {30 * S}\n")[0] == [0, 9, 1, 3, 1]
    assert run(exe, "shape 5 4 -1 0 -2001 -1 1 1000 1000\n")[0] == [0, -1, 2, -3, 3]
    assert run(exe, "shape 5 4 0 10 0 10 1 0 1000\n")[0][0] == -1  # LC_E_INVALID
    assert run(exe, "shape 5 4 0 10 0 10 1 1000 -1\n")[0][0] == -1
    assert run(exe, f"shape 5 4 0 {2**40} 0 10 32 1 1000\n")[0][0] == -2  # tables past the cap


def test_launch_info_reports_the_plan(consts):
    out = np.zeros(4, np.int64)
    N.check(N.lib().lc_perf_launch_info(N.ptr(out, C.c_int64)))
    assert out.tolist() == [consts["wg"], consts["tile"], consts["lds"], consts["digit"]]
