"""The streaming total-queue and unique-ids without a GPU: the host stream
(lc_queue_stream_open without a context) against lc_queue_pack +
lc_queue_check_host of the prefix and the restatements of
tests/queue_helpers.py after EVERY append -- array for array, map for map --
on the hand examples row by row and on seeded random histories cut at random
points; the crashed drain that arrives late, valid going 1 -> 0 -> 1, the
refusals that leave the stream as it was, results() before any append, and the
packer and host fold under AddressSanitizer and UBSan as a stand-alone
program."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import queue_helpers as H
import queue_stream_helpers as S
from lincheck import _native as N
from lincheck import checker as ck
from lincheck import independent
from lincheck import queue as Q
from lincheck.queue_stream import QueueStream, rows_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jepsen-etcd-demo_amd", "csrc")
CXX = shutil.which("g++")
TQ, IDS = S.TQ, S.IDS
MODES = [TQ, IDS]

HAND_IDS = [H.op("invoke", "generate"), H.op("ok", "generate", 5), H.op("invoke", "generate"), H.op("ok", "generate", -2),
            H.op("invoke", "generate"), H.op("fail", "generate"), H.op("invoke", "generate"), H.op("ok", "generate", 5),
            H.op("ok", "generate", None), H.op("invoke", "generate"), H.op("ok", "generate", 5), H.op("ok", "generate", H.I64_MAX)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ops", [H.HAND_QUEUE, HAND_IDS], ids=["queue", "ids"])
def test_hand_examples_row_by_row(ops, mode):
    with QueueStream(None, mode) as s:
        for i, o in enumerate(ops):
            u = s.append([o])
            assert (u.rows, u.n_keys) == (i + 1, 1)
            S.same_as_prefix(s, ops[:i + 1], mode, what=i)
        if mode == TQ and ops is H.HAND_QUEUE:
            assert s.result_map(0) == H.HAND_QUEUE_RESULT


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("seed", range(20))
def test_random_histories_at_random_cuts(seed, mode):
    parts = S.random_case(seed)
    assert any(not p for p in parts)
    so_far = []
    with QueueStream(None, mode) as s:
        before = {}
        for j, part in enumerate(parts):
            u = s.append(part)
            so_far = so_far + part
            want = S.same_as_prefix(s, so_far, mode, what=(seed, j))
            assert (u.rows, u.n_keys) == (len(so_far), len(want.valid))
            # changed: exactly the keys whose valid differs (a key first seen counts as valid before)
            keys = s.keys()
            assert u.changed == [i for i, k in enumerate(keys) if int(want.valid[i]) != before.get(k, 1)], (seed, j)
            before = {k: int(want.valid[i]) for i, k in enumerate(keys)}


def test_a_crashed_drain_arrives_in_a_later_append():
    a = [H.op("invoke", "enqueue", 1, 10), H.op("ok", "enqueue", 1, 10), H.op("invoke", "enqueue", 7, 20), H.op("ok", "enqueue", 7, 20)]
    b = [H.op("ok", "dequeue", 7, 20), H.op("info", "drain", None, 20), H.op("ok", "dequeue", 9, 20), H.op("ok", "dequeue", 1, 10)]
    c = [H.op("ok", "enqueue", 8, 20), H.op("invoke", "enqueue", 2, 10)]
    with QueueStream(None, TQ) as s:
        u = s.append(a)
        assert u.changed == [0, 1] and s.counts()[0].tolist() == [0, 0] and u.distinct == 2
        S.same_as_prefix(s, a, TQ)
        u = s.append(b)
        # key 20 is :unknown from here on, none of this append's rows of it counted; key 10's value came out
        assert u.changed == [0, 1] and u.packed == 1 and s.counts()[0].tolist() == [1, -1]
        assert s.key_error(1) == H.CRASHED_DRAIN and s.key_error(0) is None
        assert s.counts()[1][1].tolist() == [0] * 7
        S.same_as_prefix(s, a + b, TQ)
        u = s.append(c)
        assert u.changed == [] and u.packed == 1
        S.same_as_prefix(s, a + b + c, TQ)
        assert s.result_map(1) == {"valid?": "unknown", "error": H.CRASHED_DRAIN}
        # the :unknown key's values stay resident and make no entries
        assert u.distinct == 3 and not (s.results().ent_key == 1).any()


def test_a_lost_value_dequeued_later_changes_valid_twice():
    rows = [[H.op("invoke", "enqueue", 5)], [H.op("ok", "enqueue", 5)], [H.op("invoke", "dequeue")], [H.op("ok", "dequeue", 5)]]
    with QueueStream(None, TQ) as s:
        got = []
        for i, r in enumerate(rows):
            u = s.append(r)
            got.append((u.changed, int(s.counts()[0][0])))
            S.same_as_prefix(s, sum(rows[:i + 1], []), TQ)
        assert got == [([], 1), ([0], 0), ([], 0), ([0], 1)]
        assert s.result_map(0)["lost"] == [] and s.result_map(0)["ok-count"] == 1


def snapshot(s):
    return s.keys(), [a.tolist() for a in s.counts()], [getattr(s.results(), n).tolist() for n in S.ARRAYS]


@pytest.mark.parametrize("mode", MODES)
def test_refused_appends_leave_the_stream_as_it_was(mode):
    keyed = [H.op("invoke", "enqueue", 1, 3), H.op("ok", "enqueue", 1, 3), H.op("ok", "generate", 4, 3), H.op("ok", "generate", 4, 3)]
    with QueueStream(None, mode) as s:
        s.append(keyed)
        was = snapshot(s)
        with pytest.raises(N.LincheckError) as e:   # the other kind
            s.append([H.op("ok", "dequeue", 1), H.op("ok", "generate", 9)])
        assert e.value.code == -1 and snapshot(s) == was
        bad = Q.QueueHistory.from_ops([H.op("ok", "enqueue", 2, 8), H.op("ok", "dequeue", 2, 3)])
        for col, code in (("type", 4), ("f", 5)):
            h = Q.QueueHistory(bad.type.copy(), bad.f.copy(), bad.key, bad.value, bad.drain_off, bad.drain_val)
            getattr(h, col)[1] = code
            with pytest.raises(N.LincheckError) as e:
                s.append(h)
            assert e.value.code == -1 and snapshot(s) == was   # key 8 of the refused append's first row is not there
        u = s.append([H.op("ok", "dequeue", 1, 3), H.op("ok", "generate", 6, 8)])
        assert u.n_keys == 2 and s.keys() == [3, 8]
        S.same_as_prefix(s, keyed + [H.op("ok", "dequeue", 1, 3), H.op("ok", "generate", 6, 8)], mode)
    with QueueStream(None, mode) as s:   # an unkeyed stream refuses keyed rows
        s.append([H.op("ok", "enqueue", 1), H.op("ok", "generate", 1)])
        was = snapshot(s)
        with pytest.raises(N.LincheckError) as e:
            s.append(keyed)
        assert e.value.code == -1 and snapshot(s) == was and s.keys() == [None]


@pytest.mark.parametrize("mode", MODES)
def test_results_before_any_append_and_open_refusals(mode):
    with QueueStream(None, mode) as s:
        S.same_as_prefix(s, [], mode)
        assert s.keys() == [None] and s.counts()[0].tolist() == [1]
        u = s.append([])
        assert (u.rows, u.n_keys, u.packed, u.distinct, u.grew, u.changed) == (0, 1, 0, 0, False, [])
        # rows that fix nothing: nemesis rows only; then the first keyed append replaces the placeholder key
        s.append([{"type": "info", "f": "start", "value": "x", "process": "nemesis"}])
        S.same_as_prefix(s, [], mode)
        u = s.append([H.op("ok", "dequeue", 4, 77), H.op("ok", "generate", 4, 78)])
        assert s.keys() == [77, 78] and u.n_keys == 2
    for slots in (3, 1 << 28):
        with pytest.raises(N.LincheckError) as e:
            QueueStream(None, mode, {"slots": slots})
        assert e.value.code == -1
    h = N.C.c_void_p()
    assert N.lib().lc_queue_stream_open(None, 2, None, N.C.byref(h)) == -1
    assert N.lib().lc_queue_stream_open(None, mode, N.C.byref(N.LcQueueStreamOpts(0, 1)), N.C.byref(h)) == -1


def test_the_host_stream_mirrors_the_plan():
    """slots and grew follow csrc/queue_stream_plan.hpp, so a host stream's
    updates equal a device stream's field for field."""
    with QueueStream(None, TQ, {"slots": 256}) as s:
        u = s.append([H.op("ok", "enqueue", v) for v in range(255)])
        assert (u.slots, u.grew, u.distinct, u.packed) == (256, False, 255, 255)
        u = s.append([H.op("ok", "enqueue", v) for v in range(255, 512)])
        assert (u.slots, u.grew, u.distinct) == (S.plan_grown(255, 257), True, 512) and u.slots == 1024
        u = s.append([H.op("ok", "dequeue", v) for v in range(512)])
        # 512 resident + 512 rows fill 1,024 slots exactly and 2 x 512 is within them: no grow
        # (never attempted: every value goes from lost to unexpected, and valid stays 0)
        assert (u.slots, u.grew, u.distinct, u.changed) == (1024, False, 512, [])
        u = s.append([H.op("invoke", "enqueue", 600)])
        assert (u.slots, u.grew, u.distinct) == (1024, False, 513)
        u = s.append([H.op("invoke", "enqueue", 601)])   # 2 x 513 resident pass the table
        assert (u.slots, u.grew, u.distinct) == (2048, True, 514)


def test_the_ent_cap_protocol_and_columns():
    ops = []
    for v in range(40):
        ops += [H.op("ok", "enqueue", v), H.op("ok", "dequeue", -v - 1)]
    hist = Q.QueueHistory.from_ops(ops)
    with QueueStream(None, TQ) as s:
        for lo in range(0, hist.n, 16):
            s.append(rows_of(hist, lo, lo + 16))
        full = s.results()
        assert len(full.ent_key) == 80 and not full.retried
        again = s.results(ent_cap=1)
        assert again.retried
        H.same_results(full, again)
        S.same_as_prefix(s, ops, TQ)
    # a drain cut out of its history keeps its elements
    d = Q.QueueHistory.from_ops([H.op("ok", "drain", [1, 2]), H.op("ok", "drain", [3]), H.op("ok", "drain", [4, 5, 6])])
    assert rows_of(d, 1, 3).to_ops()[0]["value"] == [3] and rows_of(d, 1, 3).to_ops()[1]["value"] == [4, 5, 6]


def test_the_checker_shapes():
    hist = Q.synth_queue(n_keys=4, n_values=60, lost=2, duplicated=3, unexpected=1, recovered=4, drain=9, seed=3)
    ops = hist.to_ops()
    tq = ck.total_queue({"host": True})
    want = independent.checker(tq).check({}, ops, {})["results"]
    with tq.stream() as s:
        for lo in range(0, hist.n, 97):
            s.append(rows_of(hist, lo, lo + 97))
        assert s.dev is None and s.result_maps() == want
        for i, k in enumerate(s.keys()):
            assert s.result_map(i) == tq.check({}, independent.subhistory(ops, k), {})
    ids = Q.synth_ids(n_keys=3, n_values=200, dup_rate=0.2, seed=8)
    ui = ck.unique_ids({"host": True})
    with ui.stream() as s:
        for lo in range(0, ids.n, 333):
            s.append(rows_of(ids, lo, lo + 333))
        assert s.result_maps() == independent.checker(ui).check({}, ids, {})["results"]


@pytest.mark.skipif(not CXX, reason="no g++")
def test_packer_and_host_fold_run_clean_under_asan_and_ubsan(tmp_path):
    out = str(tmp_path / "asan_main")
    subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "queue_stream_asan_main.cpp"), os.path.join(CSRC, "host_queue_stream.cpp"),
                    os.path.join(CSRC, "host_queue.cpp"), "-pthread", "-o", out], check=True, timeout=300)
    r = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, \
        r.stderr[-3000:]
