"""The exact mode's pure rules (csrc/stream_plan.hpp: LC_STREAM_EXACT) through
tests/stream_exact_plan_main.cpp (host C++ only, no HIP): which budgets a
stream accepts with and without the flag, the peak's word inside the record's
16-word header, the budget status, the layout of the final-config arrays, and
the record still 1,360 words."""
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
    path = str(tmp_path_factory.mktemp("stream_exact_plan") / "stream_exact_plan_main")
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "jepsen-etcd-demo_amd", "csrc"),
                    os.path.join(ROOT, "tests", "stream_exact_plan_main.cpp"), "-o", path], check=True, timeout=120)
    return path


def ask(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True, timeout=60)
    rows = [list(map(int, l.split())) for l in out.stdout.strip().splitlines()]
    return rows[0], rows[1], rows[2:]


def test_header_and_statuses(exe):
    consts, hdr, _ = ask(exe, [])
    hdr_words, rec_words, h_peak, h_started, live, invalid, error, budget, min_budget, max_final = consts
    assert hdr_words == 16 and rec_words == 1360 == N.LC_STREAM_REC_WORDS   # the header had spare words
    assert h_started < h_peak < hdr_words
    words, fallback = hdr[:-1], hdr[-1]
    assert sorted(words) == list(range(11)), "every header word is its own"
    # one status space for both kinds of record: the set record's fallback keeps its value
    assert len({live, invalid, error, fallback, budget}) == 5 and live == 0
    assert min_budget == 16 * 64 * 32
    assert max_final == 16                                                   # lc_opts.max_final at most


def test_budgets_a_stream_accepts(exe):
    edge = 16 * 64 * 32
    budgets = [0, 1, 2, 63, 64, 2048, edge - 1, edge, edge + 1, 1 << 40]
    _, _, rows = ask(exe, [f"b {b} {x}" for b in budgets for x in (0, 1)])
    got = {(b, x): rows[i][0] for i, (b, x) in enumerate((b, x) for b in budgets for x in (0, 1))}
    for b in budgets:
        assert got[(b, 1)] == 1, f"exact: any budget ({b})"
        assert got[(b, 0)] == (1 if b >= edge else 0), f"closed sets are exact from {edge} on ({b})"


def test_final_array_layout(exe):
    qs = [(keys, mf, key, cfg) for keys, mf in ((1, 10), (64, 10), (65, 16), (1000, 1), (7, 0))
          for key in (0, keys - 1) for cfg in (0, max(mf - 1, 0))]
    _, _, rows = ask(exe, [f"f {a} {b} {c} {d}" for a, b, c, d in qs])
    for (keys, mf, key, cfg), (per_key, off, fbytes, nbytes) in zip(qs, rows):
        assert per_key == 2 * mf                           # two 64-bit words per config
        assert off == (key * mf + cfg) * 2                 # lc_result.final_configs' own layout
        assert off + (2 if mf else 0) <= fbytes // 8       # the last config of the last key ends inside the array
        assert fbytes == keys * mf * 16 and nbytes == keys * 4
