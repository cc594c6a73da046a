"""The exact set tier's pure rules (csrc/stream_plan.hpp) through
tests/stream_set_exact_plan_main.cpp (host C++ only, no HIP): what an :ok
decides from (|I|, |S'|, budget) in the oracle's order (oracle/linear_ref.c:
|I| against the budget inside the closure, then |S'| = 0, then |S'| against the
budget) with the cap's fallback behind each budget test; where the closure may
stop; the final configs' sort key; and that the set record gained no word."""
import os
import shutil
import subprocess

import pytest

from lincheck import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/llvm/bin/clang++"

pytestmark = pytest.mark.skipif(not shutil.which(CXX), reason="no ROCm clang++")

CAP = 32768
LIVE, INVALID, ERROR, FALLBACK, BUDGET = 0, 1, 2, 3, 4


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("stream_set_exact_plan") / "stream_set_exact_plan_main")
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "jepsen-etcd-demo_amd", "csrc"),
                    os.path.join(ROOT, "tests", "stream_set_exact_plan_main.cpp"), "-o", path], check=True, timeout=120)
    return path


def ask(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True, timeout=60)
    rows = [list(map(int, l.split())) for l in out.stdout.strip().splitlines()]
    return rows[0], [r[0] for r in rows[1:]]


def test_the_set_record_gains_no_word(exe):
    consts, _ = ask(exe, [])
    hdr_words, h_cur, rec_words, cap, h_peak, reg_hdr, *statuses = consts
    assert hdr_words == 16 and h_cur == 6 < hdr_words            # words 7..15 stay spare
    assert rec_words == N.LC_STREAM_SET_HEAD_WORDS + 4 * cap and cap == CAP
    assert h_peak == 10 < reg_hdr == 16                          # the peak stays in the register record's header
    assert statuses == [LIVE, INVALID, ERROR, FALLBACK, BUDGET]


# (table_full, |I|, |S'|, budget) -> status; hand-made, in the oracle's order
DECISIONS = [
    ((0, 10, 5, 100), LIVE),
    ((0, 100, 100, 100), LIVE),                  # at the budget is within it
    ((1, 10, 5, 100), ERROR),                    # a full table comes before everything
    ((1, 101, 0, 100), ERROR),
    ((0, 101, 5, 100), BUDGET),                  # |I| first ...
    ((0, 101, 0, 100), BUDGET),                  # ... also where S' would be empty: the oracle stops inside the closure
    ((0, 100, 0, 100), INVALID),
    ((0, 0, 0, 100), INVALID),
    ((0, 50, 101, 100), BUDGET),                 # |S'| after |I| (S' also takes configs p was linearized in)
    ((0, 1, 1, 0), BUDGET),
    # budget = cap: the budget is met, never the cap
    ((0, CAP, CAP, CAP), LIVE),
    ((0, CAP + 1, 5, CAP), BUDGET),
    ((0, CAP + 1, 0, CAP), BUDGET),
    ((0, CAP, CAP + 1, CAP), BUDGET),
    # budget = cap + 1: a size of cap + 1 is within the budget and past the cap
    ((0, CAP + 1, 5, CAP + 1), FALLBACK),
    ((0, CAP + 2, 5, CAP + 1), BUDGET),
    ((0, CAP, CAP + 1, CAP + 1), FALLBACK),
    ((0, CAP, CAP + 2, CAP + 1), BUDGET),
    ((0, CAP, CAP, CAP + 1), LIVE),
    # |S'| = 0 with |I| past the cap: the closure was cut short, so S' says nothing -- fall back
    ((0, CAP + 1, 0, 1 << 20), FALLBACK),
    ((0, CAP + 1, 0, CAP + 1), FALLBACK),
    ((0, CAP + 1, 0, CAP), BUDGET),
    ((0, CAP, 0, 1 << 20), INVALID),
    ((0, 1 << 33, 1, 1 << 40), FALLBACK),        # 64-bit sizes and budgets
    ((0, (1 << 40) + 1, 1, 1 << 40), BUDGET),
]


def test_decision_order(exe):
    _, got = ask(exe, ["d %d %d %d %d" % q for q, _ in DECISIONS])
    for (q, want), g in zip(DECISIONS, got):
        assert g == want, f"(table_full, |I|, |S'|, budget) = {q}: {g}, expected {want}"


def test_the_closure_stops_at_the_lesser_of_cap_and_budget(exe):
    budgets = [0, 1, 623, CAP - 1, CAP, CAP + 1, 1 << 20, 1 << 40]
    _, got = ask(exe, [f"c {b}" for b in budgets])
    assert got == [min(b, CAP) for b in budgets]
    # past that size the decision no longer depends on how far the count went, nor on |S'|
    for b in budgets:
        stop = min(b, CAP)
        qs = [(0, stop + 1 + more, ns, b) for more in (0, 1, 1000) for ns in (0, 1, CAP + 5)]
        _, dec = ask(exe, ["d %d %d %d %d" % q for q in qs])
        assert set(dec) <= {BUDGET, FALLBACK} and (b > CAP or set(dec) == {BUDGET}), (b, dec)


def test_a_count_past_the_cap_says_no_more_than_that(exe):
    """Entries past an array's end leave their hash set again, so the kernel's
    count past the cap may name a config twice: it is taken as cap + 1, and a
    budget above the cap is then never met in the set tier -- the key falls back."""
    counts = [0, 1, CAP - 1, CAP, CAP + 1, CAP + 2, 1 << 20, 1 << 40]
    _, got = ask(exe, [f"n {c}" for c in counts])
    assert got == [min(c, CAP + 1) for c in counts]
    qs = [(0, CAP + 1, 5, b) for b in (CAP + 1, 1 << 20)] + [(0, 100, CAP + 1, b) for b in (CAP + 1, 1 << 20)]
    _, dec = ask(exe, ["d %d %d %d %d" % q for q in qs])
    assert dec == [FALLBACK] * 4


def test_sort_key_orders_by_mask_then_state(exe):
    cfg = lambda state, mask: state << 56 | mask
    top = (1 << 56) - 1
    cs = [cfg(s, m) for m in (0, 1, 2, 3, 1 << 10, (1 << 10) | 1, 1 << 55, top) for s in (0, 1, 31, 254)]
    _, keys = ask(exe, [f"k {c}" for c in cs])
    assert keys == sorted(keys) and len(set(keys)) == len(keys)        # listed in (mask, state) order
    assert keys == [(c & top) << 8 | c >> 56 for c in cs]              # the config rotated left by 8 bits
    _, back = ask(exe, [f"u {k}" for k in keys])
    assert back == cs
    assert max(keys) < (1 << 64) - 1                                   # the selection's "none" is no key
    # state alone never outranks a mask
    _, (a, b) = ask(exe, [f"k {cfg(254, 4)}", f"k {cfg(0, 5)}"])
    assert a < b
