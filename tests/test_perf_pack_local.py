"""lc_perf_pack's one pass over the rows, made local:
every row is judged from its predecessor and its successor in its process's
group alone, and the nemesis intervals from the compacted list of :start /
:stop rows.  That restatement, in Python, equals lc_perf_pack (host code,
called through ctypes; no GPU) in the records, the counts, the bounds and the
intervals: on every history of at most 4 rows over a small alphabet, on the
hand-written history and on 300 random ones."""
import itertools
import random

import numpy as np

import perf_helpers as PH
from lincheck import _native as N
from lincheck import perf as P

NO_INVOKE = N.LC_PERF_NO_INVOKE


def local(hist):
    """The rules of section 3.19 over a PerfHistory's columns."""
    n = hist.n
    type_, f, proc, time = hist.type.tolist(), hist.f.tolist(), hist.process.tolist(), hist.time.tolist()
    # what rows_pair gives: predecessor and successor among the rows of the same process
    prev, nxt, last = [None] * n, [None] * n, {}
    for r in range(n):
        if proc[r] == N.LC_NO_PROCESS:
            continue
        if proc[r] in last:
            prev[r] = last[proc[r]]
            nxt[last[proc[r]]] = r
        last[proc[r]] = r
    records, matched, unmatched, orphans = [], 0, 0, 0
    for r in range(n):  # every row on its own
        if proc[r] == N.LC_NO_PROCESS:
            continue
        if type_[r] == N.LC_INVOKE:
            unmatched += nxt[r] is None or type_[nxt[r]] == N.LC_INVOKE
            continue
        if prev[r] is not None and type_[prev[r]] == N.LC_INVOKE:
            matched += 1
            records.append((time[r], time[prev[r]], f[prev[r]] | f[r] << 8 | type_[r] << 16))
        else:
            orphans += 1
            records.append((time[r], NO_INVOKE, f[r] | f[r] << 8 | type_[r] << 16))
    f_start, f_stop = hist.f_id("start"), hist.f_id("stop")
    nem = [(f[r], time[r]) for r in range(n) if proc[r] == N.LC_NO_PROCESS and f[r] in (f_start, f_stop)]
    intervals, open_t = [], None
    for ff, t in nem:
        if ff == f_start and open_t is None:
            open_t = t
        elif ff == f_stop and open_t is not None:
            intervals.append([open_t, t])
            open_t = None
    if open_t is not None:
        intervals.append([open_t, max(time)])
    tc = [x[0] for x in records]
    ti = [x[1] for x in records if x[1] != NO_INVOKE]
    bounds = (min(tc) if tc else 0, max(tc) if tc else 0, min(ti) if ti else 0, max(ti) if ti else 0)
    return records, (matched, unmatched, orphans), bounds, intervals


def agree(ops):
    hist = P.PerfHistory.from_ops(ops)
    packed = P.PackedPerf(hist)
    records, counts, bounds, intervals = local(hist)
    a, v = packed.arrays(), packed.view
    assert list(zip(a["t_comp"].tolist(), a["t_inv"].tolist(), a["meta"].tolist())) == records, ops
    assert (packed.matched, packed.unmatched, packed.orphans) == counts and v.n_matched == counts[0], ops
    assert (v.t_min, v.t_max, v.x_min, v.x_max) == bounds and v.n == len(records), ops
    assert packed.intervals.tolist() == intervals, ops
    return counts, intervals


TIMES = (30, 10, 40, 20)  # not in order: the largest is neither first nor last
ALPHABET = [(t, p) for t in ("invoke", "ok", "fail", "info") for p in (0, 1)] + [("info", f) for f in ("start", "stop", "kill")]


def small_ops(word):
    return [PH.op(t, x, "nemesis", TIMES[i]) if isinstance(x, str) else PH.op(t, "a" if t == "invoke" else "b", x, TIMES[i])
            for i, (t, x) in enumerate(word)]


def test_every_history_of_at_most_four_rows():
    seen, n = set(), 0
    for length in range(5):
        for word in itertools.product(ALPHABET, repeat=length):
            counts, intervals = agree(small_ops(word))
            seen.add((counts, len(intervals)))
            n += 1
    assert n == sum(11 ** k for k in range(5))
    assert {(2, 0, 0), (0, 4, 0), (0, 0, 4), (1, 1, 1)} <= {c for c, _ in seen} and {0, 1, 2} == {i for _, i in seen}


def test_the_hand_written_history():
    counts, intervals = agree(PH.hand_ops())
    assert counts == (PH.HAND_WANT["matched"], PH.HAND_WANT["unmatched"], PH.HAND_WANT["orphans"])
    assert [tuple(x) for x in intervals] == PH.HAND_WANT["nemesis"]


def test_three_hundred_random_histories():
    rng = random.Random(319)
    shapes = list(itertools.product((1, 3, 8, 50), (0, 5, 150)))
    total = np.zeros(4, np.int64)
    for i in range(300):
        procs, nemesis_every = shapes[i % len(shapes)]
        ops = PH.random_ops(rng, rng.randrange(1, 401), procs=procs, nemesis_every=nemesis_every, t0=rng.choice((0, -50000)))
        counts, intervals = agree(ops)
        total += np.array(counts + (len(intervals),))
    assert (total > 100).all()


def test_start_and_stop_under_one_name_or_absent():
    """f_start == f_stop is not reachable through names; the fold's rule for it
    and for -1 is host_perf_pack.cpp's, run by tests/perf_pack_asan_main.cpp.
    Here: a history without :start, one without :stop, one with neither."""
    for fs in (("stop", "stop"), ("start", "start", "kill"), ("kill",)):
        ops = [PH.op("info", f, "nemesis", 5 * i) for i, f in enumerate(fs)] + PH.pairs_ops([(3, 4)])
        counts, intervals = agree(ops)
        # the :start at 0 stays open to the largest time, the :kill row's 10
        assert counts == (1, 0, 0) and intervals == ([[0, 10]] if fs[0] == "start" else [])
