"""checker/total-queue and checker/unique-ids without a GPU: lc_queue_pack and
lc_queue_check_host against the two restatements of the rules in
tests/queue_helpers.py (the oracle; parity with Jepsen unpinned), a hand
example per class, the crashed drain, the top-48 rule, the range's edges, the
checker shapes with the host fold as the backend, and the packer, host fold and
EDN reader under AddressSanitizer and UBSan as a stand-alone program."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import queue_helpers as H
from lincheck import _native as N
from lincheck import checker as ck
from lincheck import independent
from lincheck import queue as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jepsen-etcd-demo_amd", "csrc")
CXX = shutil.which("g++")
TQ, IDS = N.LC_QM_TOTAL_QUEUE, N.LC_QM_UNIQUE_IDS
I64_MAX, I64_MIN = H.I64_MAX, H.I64_MIN


def agree(ops, mode=TQ):
    """Both restatements, lc_queue_pack + lc_queue_check_host's arrays and
    the result maps made of them say the same."""
    exp, maps = H.expected_arrays(ops, mode)
    again = H.restate_independent(ops, H.RESTATE[mode][1], **({"top": None} if mode == IDS else {}))
    assert maps == again, (maps, again)
    packed = Q.PackedQueue(Q.QueueHistory.from_ops(ops), mode)
    assert packed.keys == list(maps)
    res = Q.check_batch(None, packed.view, host=True)
    H.assert_results(res, exp)
    shown = H.restate_independent(ops, H.RESTATE[mode][0])
    assert shown == H.restate_independent(ops, H.RESTATE[mode][1])
    for i, k in enumerate(packed.keys):
        assert Q.result_map(packed, res, i) == shown[k], k
    return shown


def test_hand_example():
    assert agree(H.HAND_QUEUE) == {None: H.HAND_QUEUE_RESULT}
    packed = Q.PackedQueue(Q.QueueHistory.from_ops(H.HAND_QUEUE), TQ)
    a = packed.arrays()
    AT, ACK, DEQ = N.LC_QK_ATTEMPT, N.LC_QK_ACK, N.LC_QK_DEQUEUE
    # the pack is thin: one row per value that counts, in history order, the drain expanded in place
    assert a["row_kind"].tolist() == [AT, ACK, AT, ACK, AT, AT, DEQ, DEQ, DEQ, DEQ, DEQ]
    assert a["row_val"].tolist() == [1, 1, 2, 2, 3, 4, 1, 1, 3, 9, N.LC_NIL]
    assert a["row_key"].tolist() == [0] * 11 and a["status"].tolist() == [0] and a["attempted"].tolist() == [0]


CLASSES = {
    # value 1's rows -> what the result says about it
    "ok": ([("invoke", "enqueue"), ("ok", "enqueue"), ("ok", "dequeue")], dict(ok=1)),
    "lost": ([("invoke", "enqueue"), ("ok", "enqueue")], dict(lost=1)),
    "lost twice": ([("invoke", "enqueue"), ("ok", "enqueue")] * 3 + [("ok", "dequeue")], dict(ok=1, lost=2)),
    "unexpected": ([("ok", "dequeue"), ("ok", "dequeue")], dict(unexpected=2)),
    "duplicated": ([("invoke", "enqueue"), ("ok", "enqueue"), ("ok", "dequeue"), ("ok", "dequeue"), ("ok", "dequeue")],
                   dict(ok=1, duplicated=2)),
    "recovered": ([("invoke", "enqueue"), ("info", "enqueue"), ("ok", "dequeue")], dict(ok=1, recovered=1)),
    "recovered after a failure": ([("invoke", "enqueue"), ("fail", "enqueue"), ("ok", "dequeue")], dict(ok=1, recovered=1)),
    "in flight": ([("invoke", "enqueue")], dict()),
    "acknowledged without an invocation": ([("ok", "enqueue"), ("ok", "dequeue")], dict(unexpected=1)),
    "duplicated and lost": ([("invoke", "enqueue")] + [("ok", "enqueue")] * 4 + [("ok", "dequeue")] * 3,
                            dict(ok=1, duplicated=2, lost=1)),
}


@pytest.mark.parametrize("name", list(CLASSES))
@pytest.mark.parametrize("value", [1, None])
def test_a_hand_example_per_class(name, value):
    rows, want = CLASSES[name]
    ops = [H.op(t, f, value) for t, f in rows]
    got = agree(ops)[None]
    for c in ("ok", "unexpected", "duplicated", "lost", "recovered"):
        assert got[c + "-count"] == want.get(c, 0), c
        if c != "ok":
            assert got[c] == [value] * want.get(c, 0)
    assert got["valid?"] is (not want.get("lost") and not want.get("unexpected"))
    assert got["attempt-count"] == sum(r == ("invoke", "enqueue") for r in rows)
    assert got["acknowledged-count"] == sum(r == ("ok", "enqueue") for r in rows)


def test_duplicates_alone_do_not_invalidate_and_lists_are_sorted_nil_first():
    ops = []
    for v in (5, None, -3, 5):
        ops += [H.op("invoke", "enqueue", v), H.op("ok", "enqueue", v), H.op("ok", "dequeue", v), H.op("ok", "dequeue", v)]
    got = agree(ops)[None]
    assert got["valid?"] is True and got["duplicated"] == [None, -3, 5, 5] and got["duplicated-count"] == 4


def test_a_crashed_drain_next_to_a_healthy_key():
    ops = [H.op("invoke", "enqueue", 1, 10), H.op("invoke", "drain", None, 20), H.op("ok", "enqueue", 1, 10),
           H.op("info", "drain", None, 20), H.op("ok", "drain", [1], 10), H.op("ok", "dequeue", 3, 20)]
    got = agree(ops)
    assert got[20] == {"valid?": "unknown", "error": "Not sure how to handle a crashed drain operation"}
    assert got[10]["valid?"] is True and got[10]["ok-count"] == 1
    packed = Q.PackedQueue(Q.QueueHistory.from_ops(ops), TQ)
    assert packed.status.tolist() == [0, 1] and packed.n_rows == 3 and packed.key_error(0) is None
    r = independent.checker(ck.total_queue({"host": True})).check({}, ops, {})
    assert r["valid?"] == "unknown" and r["results"] == got
    # unique-ids has no drains to crash
    assert agree(ops, IDS)[20]["valid?"] is True


def test_the_empty_history_and_ignored_rows():
    empty = {"valid?": True, "lost": [], "unexpected": [], "duplicated": [], "recovered": []}
    empty.update(dict.fromkeys(H.COUNT_NAMES, 0))
    assert agree([]) == {None: empty}
    assert agree([], IDS) == {None: {"valid?": True, "attempted-count": 0, "acknowledged-count": 0, "duplicated-count": 0,
                                     "duplicated": {}, "range": [None, None]}}
    ignored = [H.op("fail", "enqueue", 1), H.op("info", "enqueue", 2), H.op("invoke", "dequeue"), H.op("fail", "dequeue", 3),
               H.op("info", "dequeue", 4), H.op("invoke", "drain"), H.op("fail", "drain"), H.op("ok", "drain", []),
               H.op("ok", "drain", None), H.op("ok", "generate", 4), H.op("ok", "read", "x"),
               {"type": "info", "f": "start", "value": "x", "process": "nemesis"}]
    assert agree(ignored) == {None: empty}
    # a row without a key among rows with keys is ignored, and a key is made by any queue row
    ops = [H.op("ok", "dequeue", 9), H.op("invoke", "generate", None, 4), H.op("ok", "dequeue", 1, 5)]
    got = agree(ops)
    assert list(got) == [4, 5] and got[4] == empty and got[5]["unexpected"] == [1]


@pytest.mark.parametrize("block", range(4))
def test_small_random_histories(block):
    """2,400 histories of 0-40 rows, 1-3 keys or none, a value domain of 1-6 so
    that every class occurs, drains (crashed ones too), nil values, nemesis
    rows; both checkers."""
    rng = H.rng_of(100 + block)
    seen = set()
    for i in range(600):
        ops = H.random_history(rng, rng.randint(0, 40), n_keys=[0, 1, 2, 3][i % 4], domain=rng.randint(1, 6),
                               p_crash=0.1 if i % 5 == 0 else 0.0)
        for m in agree(ops).values():
            seen.update(c for c in H.CLASS_NAMES if m.get(c))
            seen.add(m["valid?"])
        agree(ops, IDS)
    assert seen == set(H.CLASS_NAMES) | {True, False, "unknown"}


def test_long_random_histories():
    rng = H.rng_of(7)
    for i in range(6):
        ops = H.random_history(rng, 3000, n_keys=[0, 5][i % 2], domain=[40, 2000][i // 2 % 2])
        agree(ops)
        agree(ops, IDS)


def test_unique_ids_shows_the_48_most_frequent_duplicates():
    """60 duplicates whose counts tie in fours: the 48 shown are the highest
    counts, a tie going to the larger value, in ascending value order."""
    ops = []
    for v in range(60):
        ops += [H.op("invoke", "generate")] + [H.op("ok", "generate", 100 - v)] * (2 + v // 4)
    ops += [H.op("ok", "generate", 1000 + v) for v in range(30)]
    H.rng_of(2).shuffle(ops)
    got = agree(ops, IDS)[None]
    assert got["duplicated-count"] == 60 and got["attempted-count"] == 60 and got["valid?"] is False
    # counts 2, 2, 2, 2, 3, ... : the twelve values with the lowest counts are v = 0 .. 11, i.e. 100 down to 89
    assert got["duplicated"] == {100 - v: 2 + v // 4 for v in range(59, 11, -1)}
    assert list(got["duplicated"]) == sorted(got["duplicated"]) and len(got["duplicated"]) == 48
    # with a tie across the cut, the larger values stay
    ops = []
    for v in range(50):
        ops += [H.op("ok", "generate", v)] * 2
    got = agree(ops, IDS)[None]
    assert list(got["duplicated"]) == list(range(2, 50))
    assert agree(ops + [H.op("ok", "generate", None)] * 3, IDS)[None]["duplicated"] == {None: 3, **{v: 2 for v in range(3, 50)}}


def test_range_with_nil_and_the_largest_integer():
    ops = [H.op("ok", "generate", v) for v in (7, I64_MAX, -2, None, 7)]
    got = agree(ops, IDS)[None]
    assert got["range"] == [None, I64_MAX] and got["duplicated"] == {7: 2}
    assert agree(ops[:3], IDS)[None]["range"] == [-2, I64_MAX]
    assert agree([H.op("ok", "generate", I64_MIN + 1), H.op("ok", "generate", None)], IDS)[None]["range"] == [None, I64_MIN + 1]
    assert agree([H.op("ok", "generate", None)], IDS)[None]["range"] == [None, None]
    # only nil acknowledged: a range [nil nil] that is there, unlike a key without acks
    packed = Q.PackedQueue(Q.QueueHistory.from_ops([H.op("ok", "generate", None)]), IDS)
    res = Q.check_batch(None, packed.view, host=True)
    assert res.has_range.tolist() == [1] and res.lo.tolist() == [N.LC_NIL] and res.hi.tolist() == [N.LC_NIL]


def test_the_ent_cap_contract_and_refused_batches():
    ops = []
    for v in range(40):
        ops += [H.op("ok", "enqueue", v), H.op("ok", "dequeue", -v - 1)]
    packed = Q.PackedQueue(Q.QueueHistory.from_ops(ops), TQ)
    full = Q.check_batch(None, packed.view, host=True)
    assert len(full.ent_key) == 80 and not full.retried
    again = Q.check_batch(None, packed.view, ent_cap=1, host=True)
    assert again.retried
    H.same_results(full, again)
    a = packed.arrays()
    for name, at, bad in (("row_key", 5, 1), ("row_kind", 5, 3), ("status", 0, 2)):
        broken = dict(a, **{name: a[name].copy()})
        broken[name][at] = bad
        with pytest.raises(N.LincheckError) as e:
            Q.check_batch(None, Q.batch_of(broken, TQ), host=True)
        assert e.value.code == -1
    with pytest.raises(N.LincheckError):
        Q.check_batch(None, Q.batch_of(dict(a), IDS), host=True)


def test_checker_shapes_on_the_host_fold():
    hist = Q.synth_queue(n_keys=4, n_values=60, lost=2, duplicated=3, unexpected=1, recovered=4, drain=9, seed=3)
    ops = hist.to_ops()
    want = agree(ops)
    for m in want.values():
        assert [m[c + "-count"] for c in ("lost", "duplicated", "unexpected", "recovered")] == [2, 3, 1, 4]
        assert m["attempt-count"] == 60 and m["acknowledged-count"] == 56 and m["ok-count"] == 58
    tq = ck.total_queue({"host": True})
    assert tq.check({}, independent.subhistory(ops, 2), {}) == want[2]
    r = independent.checker(tq).check({}, ops, {})
    assert r["results"] == want and r["failures"] == [0, 1, 2, 3] and r["valid?"] is False
    assert independent.checker(tq).check({}, hist, {})["results"] == want
    both = ck.compose({"optimism": ck.unbridled_optimism(), "queue": tq, "ids": ck.unique_ids({"host": True})})
    one = both.check({}, independent.subhistory(ops, 1), {})
    assert one["queue"] == want[1] and one["ids"]["valid?"] is True and one["valid?"] is False
    r = independent.checker(ck.compose({"optimism": ck.unbridled_optimism(), "queue": tq})).check({}, ops, {})
    assert all(r["results"][k]["queue"] == want[k] and r["results"][k]["optimism"] == {"valid?": True} for k in want)
    # clean, and drained whole
    clean = Q.synth_queue(n_keys=2, n_values=50, drain=50, seed=1)
    r = independent.checker(tq).check({}, clean, {})
    assert r["valid?"] is True and all(m["ok-count"] == 50 and not m["duplicated"] for m in r["results"].values())
    ids = Q.synth_ids(n_keys=3, n_values=200, dup_rate=0.2, seed=8)
    want = agree(ids.to_ops(), IDS)
    r = independent.checker(ck.unique_ids({"host": True})).check({}, ids, {})
    assert r["results"] == want and r["valid?"] is False and all(m["attempted-count"] == 200 for m in want.values())
    assert independent.checker(ck.unique_ids({"host": True})).check({}, Q.synth_ids(2, 100), {})["valid?"] is True


def test_batched_under_independent_checker():
    assert isinstance(ck.batched_set(ck.total_queue()), Q.TotalQueueChecker)
    assert isinstance(ck.batched_set(ck.compose({"a": ck.unique_ids(), "b": ck.unbridled_optimism()})), Q.UniqueIdsChecker)


@pytest.mark.skipif(not CXX, reason="no g++")
def test_pack_host_fold_and_edn_reader_run_clean_under_asan_and_ubsan(tmp_path):
    out = str(tmp_path / "asan_main")
    subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "queue_asan_main.cpp"), os.path.join(CSRC, "host_queue.cpp"),
                    os.path.join(CSRC, "host_edn.cpp"), "-pthread", "-o", out], check=True, timeout=300)
    r = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, \
        r.stderr[-3000:]
