"""The stream's pure rules (csrc/stream_plan.hpp) through
tests/stream_plan_main.cpp (host C++ only, no HIP): the per-key record's
layout, the words a load or a save touches for a pending count, the phase a
resumed walk enters, and the deferral rule."""
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
    path = str(tmp_path_factory.mktemp("stream_plan") / "stream_plan_main")
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "jepsen-etcd-demo_amd", "csrc"),
                    os.path.join(ROOT, "tests", "stream_plan_main.cpp"), "-o", path], check=True, timeout=120)
    return path


def ask(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True, timeout=60)
    rows = [list(map(int, l.split())) for l in out.stdout.strip().splitlines()]
    return rows[0], rows[1], rows[2:]


def test_record_layout(exe):
    consts, hdr, _ = ask(exe, [])
    hdr_words, arrays, off_lanes, off_lat, lat_max, rec_words, width, states, min_budget, max_desc = consts
    assert (hdr_words, arrays) == (16, 5)          # the header, then k_v cap_v b_v slot_v dense_v
    assert off_lanes == hdr_words and off_lat == off_lanes + arrays * 64
    assert lat_max == 1024 and rec_words == off_lat + lat_max == N.LC_STREAM_REC_WORDS
    assert (width, states) == (10, 32)             # the register tier's reach (T0_MAX_WIDTH, T0_MAX_STATES)
    assert min_budget == 16 * 64 * 32              # the largest lattice: 16 registers x 64 lanes x 32 states
    assert max_desc == 1089 <= 2048                # 16-bit event words always fit
    # status, n, live, in_mem, dirty, events done, fail event, the two pending-slot words: distinct header words
    assert sorted(hdr) == list(range(10)) and max(hdr) < hdr_words


def test_words_touched_and_resume_phase(exe):
    _, _, rows = ask(exe, [f"n {n} 1 0" for n in range(11)] + [f"n {n} 0 1" for n in (0, 6, 10)])
    for n in range(11):
        lat, load, save, phase, in_ws = rows[n]
        assert lat == 64 * 2 ** max(n - 6, 0)      # one register up to 6 pending, doubling beyond; 1,024 at 10
        assert load == save == 16 + 5 * 64 + lat
        assert phase == (1 if n >= 7 else 0)       # lane phase up to 6 pending, dense from 7
        assert in_ws == (1 if n >= 9 else 0)       # the compact build's 4 registers hold 8
    for row in rows[11:]:
        assert row[1] == 16 and row[2] == 16       # a fresh record loads, a dead key stores, the header alone


def test_deferral_rule(exe):
    qs = [(s, st) for s in (0, 9, 10, 11, 63) for st in (1, 32, 33, 34)]
    _, _, rows = ask(exe, [f"d {s} {st}" for s, st in qs])
    for (s, st), (got,) in zip(qs, rows):
        assert got == int(s >= 10 or st > 32), (s, st)
