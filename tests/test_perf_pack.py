"""lc_perf_pack against the restatement (tests/perf_helpers.py, rules 1, 2 and
6 of DESIGN.md section 3.10): the records, the pairing counts and the nemesis
intervals.  No GPU."""
import random

import numpy as np
import pytest

import perf_helpers as PH
from lincheck import _native as N
from lincheck import perf as P


def packed_of(ops):
    hist = P.PerfHistory.from_ops(ops)
    return hist, P.PackedPerf(hist)


def records(hist, packed):
    a = packed.arrays()
    return [(hist.names[fi], hist.names[fc], P.TYPE_NAMES[t], tc, None if ti == N.LC_PERF_NO_INVOKE else ti)
            for fi, fc, t, tc, ti in zip(a["f_inv"].tolist(), a["f_comp"].tolist(), a["type"].tolist(),
                                         a["t_comp"].tolist(), a["t_inv"].tolist())]


def agree(ops):
    want = PH.restate(ops)
    hist, packed = packed_of(ops)
    assert records(hist, packed) == want["records"]
    assert (packed.matched, packed.unmatched, packed.orphans) == (want["matched"], want["unmatched"], want["orphans"])
    assert [tuple(x) for x in packed.intervals.tolist()] == want["nemesis"]
    v = packed.view
    if packed.n:
        tc = [r[3] for r in want["records"]]
        assert (v.t_min, v.t_max) == (min(tc), max(tc))
    if packed.matched:
        xs = [r[4] for r in want["records"] if r[4] is not None]
        assert (v.x_min, v.x_max, v.n_matched) == (min(xs), max(xs), len(xs))
    return want, packed


def test_hand_example():
    want, packed = agree(PH.hand_ops())
    for k in ("matched", "unmatched", "orphans", "nemesis", "points"):
        assert want[k] == PH.HAND_WANT[k]
    assert packed.n == 5  # four pairs and the orphan


def test_replaced_pending_invoke():
    ops = [PH.op("invoke", "read", 0, 10), PH.op("invoke", "write", 0, 20), PH.op("ok", "write", 0, 25)]
    want, packed = agree(ops)
    assert want["points"] == [("write", "ok", 20, 5)] and packed.unmatched == 1


def test_orphans_keep_their_own_f_and_time():
    ops = [PH.op("fail", "cas", 3, 7), PH.op("invoke", "read", 3, 8), PH.op("ok", "read", 3, 9), PH.op("ok", "read", 3, 11)]
    want, packed = agree(ops)
    assert packed.orphans == 2 and want["records"][0] == ("cas", "cas", "fail", 7, None)


def test_info_completes_and_clears():
    ops = [PH.op("invoke", "write", 1, 5), PH.op("info", "write", 1, 50), PH.op("ok", "write", 1, 60)]
    want, packed = agree(ops)
    assert want["points"] == [("write", "info", 5, 45)] and packed.orphans == 1


def test_completion_takes_the_invocations_f_and_may_precede_it():
    ops = [PH.op("invoke", "read", 0, 100), PH.op("ok", "write", 0, 90)]
    want, _ = agree(ops)
    assert want["points"] == [("read", "ok", 100, -10)] and want["rate"] == {("write", "ok", 0): 1}


def test_invokes_pending_at_the_end():
    ops = [PH.op("invoke", "read", p, p) for p in range(5)] + [PH.op("ok", "read", 2, 9)]
    _, packed = agree(ops)
    assert (packed.matched, packed.unmatched) == (1, 4)


def test_sparse_and_negative_processes():
    ops = [PH.op("invoke", "read", -4, 1), PH.op("invoke", "read", 10**12, 2), PH.op("ok", "read", 10**12, 3),
           PH.op("ok", "read", -4, 4)]
    want, _ = agree(ops)
    assert [p[3] for p in want["points"]] == [1, 3]


def test_nemesis_intervals():
    n = "nemesis"
    ops = [PH.op("info", "stop", n, 1), PH.op("info", "start", n, 2), PH.op("info", "start", n, 3),
           PH.op("invoke", "start", 0, 4),  # a client op named :start is no nemesis row
           PH.op("info", "stop", n, 5), PH.op("info", "stop", n, 6), PH.op("info", "kill", n, 7),
           PH.op("info", "start", n, 8), PH.op("ok", "start", 0, 30), PH.op("info", "start", n, 9)]
    want, _ = agree(ops)
    assert want["nemesis"] == [(2, 5), (8, 30)]


def test_empty_and_nemesis_only():
    _, packed = agree([])
    assert packed.n == 0 and len(packed.intervals) == 0
    _, packed = agree([PH.op("info", "start", "nemesis", 5), PH.op("info", "stop", "nemesis", 9)])
    assert packed.n == 0 and packed.intervals.tolist() == [[5, 9]]


@pytest.mark.parametrize("seed", range(4))
def test_random(seed):
    want, _ = agree(PH.random_ops(random.Random(seed), 3000, t0=-5000))
    assert want["orphans"] and want["unmatched"] and want["matched"] > 1000


def test_malformed_rows():
    hist = P.PerfHistory.from_ops(PH.hand_ops())
    for col, bad in (("type", 4), ("f", len(hist.names))):
        h = P.PerfHistory(hist.type.copy(), hist.f.copy(), hist.process, hist.time, hist.names)
        getattr(h, col)[2] = bad
        with pytest.raises(N.LincheckError, match="invalid"):
            P.PackedPerf(h)


def test_too_many_names():
    ok = [PH.op("invoke", f"f{i}", 0, i) for i in range(N.LC_PERF_MAX_F)]
    assert P.PackedPerf(P.PerfHistory.from_ops(ok)).unmatched == N.LC_PERF_MAX_F
    with pytest.raises(N.LincheckError, match="unsupported") as e:
        P.PackedPerf(P.PerfHistory.from_ops(ok + [PH.op("invoke", "one-more", 0, 99)]))
    assert e.value.code == -5


def test_shape_and_bad_widths():
    import ctypes as C
    _, packed = packed_of(PH.hand_ops())
    out = np.zeros(4, np.int64)
    N.check(N.lib().lc_perf_shape(C.byref(packed.view), C.byref(P.make_opts()), N.ptr(out, C.c_int64)))
    assert out.tolist() == [0, 5, 0, 2]  # completions from 1 s to 41 s, invocations from 1 s to 31 s
    for key in ("quantile-dt-ns", "rate-dt-ns"):
        for bad in (0, -1):
            o = P.make_opts({key: bad})
            assert N.lib().lc_perf_shape(C.byref(packed.view), C.byref(o), N.ptr(out, C.c_int64)) == -1
