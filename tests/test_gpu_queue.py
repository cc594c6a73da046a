"""lc_queue_check on the GPU: every case compares valid, the seven counts, the
range and the sorted entries for equality with lc_queue_check_host and with
both restatements of tests/queue_helpers.py (checker/total-queue's and
checker/unique-ids' rules restated; parity with Jepsen unpinned).  Everything is
an integer: no tolerances.  Shapes are the smallest at which each kernel can go
wrong, in threads per workgroup T.  No case drives the probe loop to its bound:
the refusals are the host's, or the kernel's flag for a bad row."""
import ctypes as C

import numpy as np
import pytest

import queue_helpers as H
from lincheck import _native as N
from lincheck import checker as ck
from lincheck import independent
from lincheck import queue as Q

pytestmark = pytest.mark.gpu

TQ, IDS = N.LC_QM_TOTAL_QUEUE, N.LC_QM_UNIQUE_IDS
I64_MAX, I64_MIN = H.I64_MAX, H.I64_MIN


def launch_info():
    out = np.zeros(4, np.int64)
    N.check(N.lib().lc_queue_launch_info(N.ptr(out, C.c_int64)))
    return out.tolist()


T = launch_info()[0]


@pytest.fixture(scope="module")
def dev(device):
    return ck.Device(0)


def agree(dev, ops, mode=TQ, slots=0, ent_cap=None, rows=None):
    """Device = host fold = both restatements, array for array and map for map.
    rows: the packed row count the case is about."""
    exp, maps = H.expected_arrays(ops, mode)
    again = H.restate_independent(ops, H.RESTATE[mode][1], **({"top": None} if mode == IDS else {}))
    assert maps == again
    packed = Q.PackedQueue(Q.QueueHistory.from_ops(ops), mode)
    assert packed.keys == list(maps)
    if rows is not None:
        assert packed.n_rows == rows
    res = Q.check_batch(dev, packed.view, slots, ent_cap)
    H.assert_results(res, exp, "device")
    host = Q.check_batch(None, packed.view, host=True)
    H.assert_results(host, exp, "host")
    shown = H.restate_independent(ops, H.RESTATE[mode][0])
    for i, k in enumerate(packed.keys):
        assert Q.result_map(packed, res, i) == shown[k], k
    return packed, res, maps


def enq_deq(values, key=None):
    """Every value enqueued, acknowledged and dequeued once."""
    ops = []
    for v in values:
        ops += [H.op("invoke", "enqueue", v, key), H.op("ok", "enqueue", v, key), H.op("ok", "dequeue", v, key)]
    return ops


# 1 ---- the hand example and the empty shapes ---------------------------------------------------

def test_hand_example(dev):
    packed, res, maps = agree(dev, H.HAND_QUEUE, rows=11)
    assert maps[None] == H.HAND_QUEUE_RESULT and Q.result_map(packed, res, 0) == H.HAND_QUEUE_RESULT
    assert res.timing["kernel_ms"] > 0 and res.timing["total_ms"] > 0


def test_nothing_and_only_ignored_kinds(dev):
    _, res, _ = agree(dev, [], rows=0)
    assert res.valid.tolist() == [1] and not res.counts.any() and len(res.ent_key) == 0
    ignored = [H.op("fail", "enqueue", 1), H.op("info", "enqueue", 2), H.op("invoke", "dequeue"), H.op("fail", "dequeue"),
               H.op("invoke", "drain"), H.op("fail", "drain"), H.op("ok", "generate", 4),
               {"type": "info", "f": "start", "value": "x", "process": "nemesis"}]
    _, res, _ = agree(dev, ignored, rows=0)
    assert res.valid.tolist() == [1] and not res.counts.any()
    _, res, _ = agree(dev, ignored, IDS, rows=1)
    assert res.counts[0, :3].tolist() == [0, 1, 0]
    # a crashed drain's key beside a healthy one; and K = 0 through a caller-built batch
    _, res, _ = agree(dev, [H.op("info", "drain", None, 1), H.op("ok", "dequeue", 5, 1)] + enq_deq([1, 2], 2), rows=6)
    assert res.valid.tolist() == [-1, 1] and not res.counts[0].any()
    res = Q.check_batch(dev, Q.batch_of(dict(row_key=[], row_kind=[], row_val=[], status=[]), TQ))
    assert len(res.valid) == 0 and len(res.ent_key) == 0


# 2 ---- workgroup edges -------------------------------------------------------------------------

@pytest.mark.parametrize("n", [T - 1, T, T + 1, 3 * T + 1])
def test_distinct_values_at_the_workgroup_edges(dev, n):
    """n rows on one key, all values distinct, each acknowledged and never
    dequeued: n lost values, n entries from several workgroups."""
    ops = [H.op("ok", "enqueue", 3 * v - n) for v in range(n)]
    _, res, _ = agree(dev, ops, rows=n)
    assert res.counts[0].tolist() == [0, n, 0, 0, 0, n, 0] and len(res.ent_key) == n


def test_a_full_table_and_a_table_of_one_slot(dev):
    """Load factor 1: slots = T with exactly T distinct values, the longest
    probe chains there can be and wrap-around past the last slot; every value
    still finds its slot, so the probe bound is not reached."""
    rng = H.rng_of(5)
    values = rng.sample(range(-10**6, 10**6), T)
    row = [lambda v: H.op("invoke", "enqueue", v), lambda v: H.op("ok", "enqueue", v), lambda v: H.op("ok", "dequeue", v)]
    ops = [row[i % 3](v) for i, v in enumerate(values)]  # one row per value: the table takes no fewer slots than rows
    _, res, _ = agree(dev, ops, slots=T, rows=T)
    third = [len(range(j, T, 3)) for j in range(3)]
    assert res.counts[0].tolist() == [third[0], third[1], 0, third[2], 0, third[1], 0]
    _, res, _ = agree(dev, [H.op("ok", "dequeue", 42)], slots=1, rows=1)
    assert res.valid.tolist() == [0] and res.counts[0].tolist() == [0, 0, 0, 1, 0, 0, 0]


def test_one_value_65793_times(dev):
    """Contention on one slot, exact 32-bit tallies past 2^16."""
    n = 65793
    ops = [H.op("invoke", "enqueue", 7)] + [H.op("ok", "dequeue", 7)] * n
    _, res, _ = agree(dev, ops, rows=n + 1)
    assert res.counts[0].tolist() == [1, 0, 1, 0, n - 1, 0, 1]
    assert res.ent_class.tolist() == [N.LC_QC_DUPLICATED, N.LC_QC_RECOVERED] and res.ent_mult.tolist() == [n - 1, 1]


def test_the_same_values_in_two_keys_do_not_merge(dev):
    """The key id is part of a slot's identity."""
    ops = []
    for v in range(40):
        ops += [H.op("invoke", "enqueue", v, 10), H.op("ok", "enqueue", v, 10), H.op("ok", "dequeue", v, 20)]
    _, res, _ = agree(dev, ops, rows=120)
    assert res.counts[0].tolist() == [40, 40, 0, 0, 0, 40, 0] and res.counts[1].tolist() == [0, 0, 0, 40, 0, 0, 0]


def test_300_tiny_keys_in_the_smallest_table(dev):
    rng = H.rng_of(6)
    ops = []
    for k in range(300):
        ops += H.random_history(rng, 6, n_keys=0, domain=3)
        ops[-6:] = [dict(o, value=independent.tuple(k, o["value"])) if o["f"] in H.QUEUE_FS else o for o in ops[-6:]]
    packed = Q.PackedQueue(Q.QueueHistory.from_ops(ops), TQ)
    slots = 1
    while slots < packed.n_rows:
        slots *= 2
    agree(dev, ops, slots=slots)
    agree(dev, ops)


def test_extreme_values_and_nil(dev):
    ops = []
    for i, v in enumerate([I64_MIN + 1, I64_MAX, 0, -1, None]):
        if i % 3 == 0:    # duplicated
            ops += enq_deq([v]) + [H.op("ok", "dequeue", v)]
        elif i % 3 == 1:  # lost
            ops += [H.op("invoke", "enqueue", v), H.op("ok", "enqueue", v)]
        else:             # unexpected
            ops += [H.op("ok", "drain", [v, v])]
    packed, res, maps = agree(dev, ops)
    assert maps[None]["duplicated"] == [I64_MIN + 1, -1] and maps[None]["lost"] == [None, I64_MAX]
    assert maps[None]["unexpected"] == [0, 0]
    # and as ids: the range reaches both ends, nil below every integer
    ids = [H.op("ok", "generate", v) for v in [0, I64_MAX, None, I64_MIN + 1, -1, I64_MAX, None]]
    packed, res, maps = agree(dev, ids, IDS)
    assert maps[None]["range"] == [None, I64_MAX] and maps[None]["duplicated"] == {None: 2, I64_MAX: 2}


def test_anomalies_from_several_workgroups_and_a_small_ent_cap(dev):
    """More than T anomalous values spread over the table: the entries come
    from several workgroups' spans of the entry array.  With ent_cap 1 the call
    says how many there are and the second call succeeds."""
    n = 2 * T + 19
    ops = []
    for v in range(n):
        ops += enq_deq([v * 1000003])
        if v % 2:
            ops.append(H.op("ok", "dequeue", v * 1000003))      # duplicated
        if v % 3 == 0:
            ops.append(H.op("ok", "dequeue", -v - 1))            # unexpected
    _, res, _ = agree(dev, ops)
    assert len(res.ent_key) > T
    _, res, _ = agree(dev, ops, ent_cap=1)
    assert res.retried and len(res.ent_key) > T
    # the raw contract: LC_E_NOMEM, n_ent set to the capacity needed, everything else written
    packed = Q.PackedQueue(Q.QueueHistory.from_ops(ops), TQ)
    valid, counts = np.zeros(1, np.int8), np.zeros((1, 7), np.uint64)
    lo, hi, has = np.zeros(1, np.int64), np.zeros(1, np.int64), np.zeros(1, np.uint8)
    ek, ec, ev, em = np.zeros(1, np.uint32), np.zeros(1, np.uint8), np.zeros(1, np.int64), np.zeros(1, np.uint64)
    r = N.LcQueueResult(N.ptr(valid, C.c_int8), N.ptr(counts, C.c_uint64), N.ptr(lo, C.c_int64), N.ptr(hi, C.c_int64),
                        N.ptr(has, C.c_uint8), N.ptr(ek, C.c_uint32), N.ptr(ec, C.c_uint8), N.ptr(ev, C.c_int64),
                        N.ptr(em, C.c_uint64), 1, 0)
    rc = N.lib().lc_queue_check(dev.handle, C.byref(packed.view), C.byref(N.LcQueueOpts(0, 0)), C.byref(r))
    assert rc == -2 and int(r.n_ent) == len(res.ent_key) and str(len(res.ent_key)) in N.lib().lc_last_error().decode()
    assert np.array_equal(counts, res.counts) and valid.tolist() == [0]


# 3 ---- refusals ------------------------------------------------------------------------------------

def test_refusals(dev):
    packed = Q.PackedQueue(Q.QueueHistory.from_ops(enq_deq(range(100))), TQ)
    for slots in (384, 256, 3):  # not a power of two; fewer than the 300 rows
        with pytest.raises(N.LincheckError) as e:
            Q.check_batch(dev, packed.view, slots)
        assert e.value.code == -1
    a = packed.arrays()
    bad = dict(a, row_key=a["row_key"].copy())
    bad["row_key"][250] = 1  # n_keys is 1
    with pytest.raises(N.LincheckError) as e:
        Q.check_batch(dev, Q.batch_of(bad, TQ))
    assert e.value.code == -1 and "row_key" in str(e.value)
    bad = dict(a, row_kind=a["row_kind"].copy())
    bad["row_kind"][17] = 3
    with pytest.raises(N.LincheckError) as e:
        Q.check_batch(dev, Q.batch_of(bad, TQ))
    assert e.value.code == -1
    with pytest.raises(N.LincheckError) as e:  # unique-ids has one kind only
        Q.check_batch(dev, Q.batch_of(dict(a), IDS))
    assert e.value.code == -1
    # the context is as good as before
    H.same_results(Q.check_batch(dev, packed.view), Q.check_batch(None, packed.view, host=True))


# 4 ---- unique-ids ----------------------------------------------------------------------------------

def test_ids_all_distinct(dev):
    n = T + 1
    ops = []
    for v in range(n):
        ops += [H.op("invoke", "generate"), H.op("ok", "generate", 5 * v - 77)]
    _, res, maps = agree(dev, ops, IDS, rows=n)
    assert maps[None] == {"valid?": True, "attempted-count": n, "acknowledged-count": n, "duplicated-count": 0,
                          "duplicated": {}, "range": [-77, 5 * (n - 1) - 77]}


def test_ids_60_duplicates_with_ties(dev):
    """The 48 shown are those with the highest counts, ties towards the larger
    value; the ABI returns all 60."""
    ops = []
    for v in range(60):
        ops += [H.op("ok", "generate", v * 11)] * (2 + v % 4)
    ops += [H.op("ok", "generate", 1000 + v) for v in range(T)]
    H.rng_of(3).shuffle(ops)
    _, res, maps = agree(dev, ops, IDS)
    assert len(res.ent_key) == 60 and maps[None]["duplicated-count"] == 60
    shown = H.restate_ids(ops)["duplicated"]
    assert len(shown) == 48 and set(shown) == {v * 11 for v in range(60) if v % 4 or v >= 48}


def test_ids_range_on_one_key_and_none_on_another(dev):
    ops = [H.op("invoke", "generate", None, 1), H.op("ok", "generate", 9, 1), H.op("ok", "generate", -4, 1),
           H.op("invoke", "generate", None, 2), H.op("fail", "generate", None, 2), H.op("ok", "generate", 9, 3)]
    _, res, maps = agree(dev, ops, IDS, rows=3)
    assert res.has_range.tolist() == [1, 0, 1]
    assert [m["range"] for m in maps.values()] == [[-4, 9], [None, None], [9, 9]]


# 5 ---- the checkers ----------------------------------------------------------------------------------

def test_synth_queue_through_independent_checker(dev):
    hist = Q.synth_queue(n_keys=5, n_values=200, lost=3, duplicated=4, unexpected=2, recovered=5, drain=17, seed=9)
    want = H.restate_independent(hist.to_ops(), H.restate_queue)
    r = independent.checker(ck.total_queue()).check({}, hist, {})
    assert r["results"] == want and r["valid?"] is False and r["failures"] == list(want)
    for m in want.values():
        assert [m[c + "-count"] for c in ("lost", "duplicated", "unexpected", "recovered")] == [3, 4, 2, 5]
    clean = Q.synth_queue(n_keys=3, n_values=100, duplicated=2, drain=100, seed=2)
    r = independent.checker(ck.total_queue()).check({}, clean, {})
    assert r["valid?"] is True and all(m["duplicated-count"] == 2 for m in r["results"].values())
    ids = Q.synth_ids(n_keys=4, n_values=300, dup_rate=0.1, seed=4)
    r = independent.checker(ck.unique_ids()).check({}, ids, {})
    assert r["results"] == H.restate_independent(ids.to_ops(), H.restate_ids) and r["valid?"] is False


def test_compose_next_to_perf(dev):
    ops = [dict(o, time=1000 * i) for i, o in enumerate(H.HAND_QUEUE)]
    both = ck.compose({"perf": ck.perf(), "queue": ck.total_queue(), "ids": ck.unique_ids()})
    r = both.check({}, ops, {})
    assert r["queue"] == H.HAND_QUEUE_RESULT and r["perf"]["valid?"] is True and r["valid?"] is False
    assert r["ids"] == {"valid?": True, "attempted-count": 0, "acknowledged-count": 0, "duplicated-count": 0,
                        "duplicated": {}, "range": [None, None]}


def test_an_edn_file_end_to_end(dev, tmp_path):
    path = tmp_path / "history.edn"
    path.write_text("""
{:type :invoke, :f :enqueue, :value [1 10], :process 0, :time 1}
{:type :ok, :f :enqueue, :value [1 10], :process 0, :time 2}
{:type :invoke, :f :enqueue, :value [2 10], :process 1, :time 3}
{:type :info, :f :start, :value "partition", :process :nemesis, :time 4}
{:type :ok, :f :enqueue, :value [2 10], :process 1, :time 5}
{:type :invoke, :f :drain, :value [1 nil], :process 0, :time 6}
{:type :ok, :f :drain, :value [1 [10 11]], :process 0, :time 7}
{:type :invoke, :f :dequeue, :value [2 nil], :process 1, :time 8}
{:type :fail, :f :dequeue, :value [2 nil], :process 1, :time 9}
""")
    hist = Q.QueueHistory.read_edn(str(path))
    r = independent.checker(ck.total_queue()).check({}, hist, {})
    assert r["results"] == H.restate_independent(hist.to_ops(), H.restate_queue)
    assert r["results"][1]["unexpected"] == [11] and r["results"][2]["lost"] == [10] and r["failures"] == [1, 2]
