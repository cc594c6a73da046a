"""The streaming total-queue and unique-ids on the device.  Every comparison
is integer equality, after EVERY append, with the host stream (updates field
for field, arrays) and with lc_queue_pack + lc_queue_check_host of the prefix;
on the small cases with the restatements of tests/queue_helpers.py and the
result maps too.  Shapes are the smallest that cross the kernels' paths: T - 1,
T, T + 1 and 3T + 1 values around one workgroup of T threads, a table filled to
its last slot, a grow from a full table, one launch's row limit plus three."""
import ctypes as C

import numpy as np
import pytest

import queue_helpers as H
import queue_stream_helpers as S
from lincheck import _native as N
from lincheck import checker as ck
from lincheck import independent
from lincheck import queue as Q
from lincheck.queue_stream import QueueStream, launch_info, rows_of
from test_queue_stream_host import HAND_IDS

pytestmark = pytest.mark.gpu

TQ, IDS = S.TQ, S.IDS
MODES = [TQ, IDS]
T = launch_info()["block"]
INV, OK, INFO = N.LC_INVOKE, N.LC_OK_T, N.LC_INFO
ENQ, DEQ, GEN = N.LC_QF_ENQUEUE, N.LC_QF_DEQUEUE, N.LC_QF_GENERATE


@pytest.fixture(scope="module")
def dev(device):
    return ck.Device(0)


def cols(type_, f, value, key=None):
    """A history from columns (scalars are repeated)."""
    n = len(value)
    full = lambda x, dt: np.full(n, x, dt) if np.isscalar(x) else np.asarray(x, dt)  # noqa: E731
    return Q.QueueHistory(full(type_, np.uint8), full(f, np.uint8), None if key is None else full(key, np.int64),
                          np.asarray(value, np.int64))


def cat(parts):
    """Histories (op-map lists or column histories) as one."""
    if all(isinstance(p, list) for p in parts):
        return sum(parts, [])
    hs = [p if isinstance(p, Q.QueueHistory) else Q.QueueHistory.from_ops(p) for p in parts]
    keyed = any(h.key is not None for h in hs)
    key = np.concatenate([h.key if h.key is not None else np.full(h.n, N.LC_NO_KEY, np.int64) for h in hs]) if keyed else None
    off, dv, base = [np.zeros(1, np.uint64)], [], 0
    for h in hs:
        o = h.drain_off if h.drain_off is not None else np.zeros(h.n + 1, np.uint64)
        off.append(o[1:] + np.uint64(base))
        dv.append(h.drain_val)
        base += int(o[-1])
    return Q.QueueHistory(np.concatenate([h.type for h in hs]), np.concatenate([h.f for h in hs]), key,
                          np.concatenate([h.value for h in hs]), np.concatenate(off), np.concatenate(dv))


def follow(dev, parts, mode, opts=None, maps=True, host_opts=None):
    """Append parts to a device stream and to a host stream; after every
    append both agree with each other and with the one-shot check of the
    prefix.  Returns the updates and the last results."""
    ups = []
    with QueueStream(dev, mode, opts) as d, QueueStream(None, mode, host_opts if host_opts is not None else opts) as h:
        S.same_as_prefix(d, [], mode, maps=False, what="before")
        for j, part in enumerate(parts):
            ud, uh = d.append(part), h.append(part)
            if host_opts is None:
                S.same_update(ud, uh, j)
            want = S.same_as_prefix(d, cat(parts[:j + 1]), mode, maps=maps, what=j)
            H.same_results(d.results(), h.results())
            for a, b in zip(d.counts()[:2], h.counts()[:2]):
                assert np.array_equal(a, b), j
            ups.append(ud)
        return ups, want


@pytest.mark.parametrize("mode", MODES)
def test_hand_examples_row_by_row(dev, mode):
    ops = H.HAND_QUEUE if mode == TQ else HAND_IDS
    ups, _ = follow(dev, [[o] for o in ops], mode)
    assert [u.rows for u in ups] == list(range(1, len(ops) + 1))
    if mode == TQ:
        with QueueStream(dev, TQ) as s:
            s.append(ops[:5])
            s.append(ops[5:])
            assert s.result_map(0) == H.HAND_QUEUE_RESULT


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("seed", [0, 4, 5, 8, 13])
def test_random_histories_at_random_cuts(dev, seed, mode):
    follow(dev, S.random_case(seed), mode, {"slots": 256})


EDGE_VALUES = [None, -H.I64_MAX, H.I64_MAX, 0, -1]  # nil is INT64_MIN itself (LC_NIL); then the integers' ends


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [T - 1, T, T + 1, 3 * T + 1])
def test_the_three_ways_a_row_meets_a_slot(dev, n, mode):
    """First seen in this append (claim), seen twice in one append (match
    against the chunk's row), seen again in a later append (match against the
    settled payload): n distinct values under each of two keys, the same
    values under both."""
    vals = (EDGE_VALUES + list(range(1000, 1000 + n)))[:n]
    f = "enqueue" if mode == TQ else "generate"
    first = [H.op(t, f, v, k) for v in vals for k in (3, 9) for t in (("invoke", "ok") if mode == TQ else ("ok", "ok"))]
    later = [H.op("ok", "dequeue" if mode == TQ else "generate", v, k) for k in (9, 3) for v in reversed(vals)]
    third = [H.op("ok", "dequeue" if mode == TQ else "generate", v, 9) for v in vals[::2]] + [H.op("invoke", f, 77, 5)]
    ups, want = follow(dev, [first, later, third], mode, maps=n <= T + 1)
    assert [u.distinct for u in ups] == [2 * n, 2 * n, 2 * n + (mode == TQ)] and not any(u.grew for u in ups)
    if mode == TQ:
        assert want.valid.tolist() == [1, 1, 1] and want.counts[:2, N.LC_QN_OK].tolist() == [n, n]
        assert want.counts[1, N.LC_QN_DUPLICATED] == len(vals[::2])
    else:
        assert want.counts[:2, N.LC_QN_OK].tolist() == [n, n] and want.counts[1, N.LC_QN_ACKNOWLEDGED] == 3 * n + len(vals[::2])
        assert (want.lo[:2].tolist(), want.hi[:2].tolist()) == ([N.LC_NIL] * 2, [H.I64_MAX] * 2)


def test_growth(dev):
    """T - 1 acknowledged enqueues fit a table of T; T + 2 more grow it to what
    the plan says; every value dequeued after the grow finds its tallies.  A
    stream opened large enough never to grow gives the same arrays."""
    a = cols(OK, ENQ, np.arange(T - 1))
    b = cols(OK, ENQ, np.arange(T - 1, 2 * T + 1))
    c = cat([cols(INV, ENQ, np.arange(2 * T + 1)), cols(OK, DEQ, np.arange(2 * T + 1)[::-1])])
    parts = [a, b, c]
    ups, want = follow(dev, parts, TQ, {"slots": T}, maps=False)
    grown = S.plan_grown(T - 1, T + 2)
    assert not S.plan_must_grow(T, 0, T - 1) and S.plan_must_grow(T, T - 1, T + 2) and grown == 8 * T
    assert [(u.slots, u.grew, u.distinct) for u in ups[:2]] == [(T, False, T - 1), (grown, True, 2 * T + 1)]
    # 2T + 1 resident and 4T + 2 rows fit 8T slots, and 2 (2T + 1) is within them: the third append leaves the table alone
    assert (ups[2].slots, ups[2].grew, ups[2].distinct) == (grown, False, 2 * T + 1)
    assert [u.changed for u in ups] == [[0], [], [0]]
    assert want.valid.tolist() == [1] and want.counts[0].tolist() == [2 * T + 1, 2 * T + 1, 2 * T + 1, 0, 0, 0, 0]
    big, _ = follow(dev, parts, TQ, {"slots": 64 * T}, maps=False)
    assert not any(u.grew for u in big) and {u.slots for u in big} == {64 * T}
    with QueueStream(dev, TQ, {"slots": T}) as s1, QueueStream(dev, TQ, {"slots": 64 * T}) as s2:
        for p in parts:
            s1.append(p), s2.append(p)
            H.same_results(s1.results(), s2.results())
    # a table grown again and again: 12 appends of T values each
    step = [cols(OK, GEN, np.arange(i * T, (i + 1) * T) * 7919) for i in range(12)]
    ups, want = follow(dev, step, IDS, {"slots": T}, maps=False)
    assert sum(u.grew for u in ups) >= 3 and ups[-1].distinct == 12 * T and want.counts[0, N.LC_QN_ACKNOWLEDGED] == 12 * T


def test_a_table_filled_to_its_last_slot(dev):
    """resident + rows == slots exactly: load factor 1 after the append, every
    value at home in the table's last three slots so that every probe wraps past
    the end.  Then a grow from the full table."""
    vals, v = [], 0
    while len(vals) < T:
        if S.slot_hash(0, v) & (T - 1) >= T - 3:
            vals.append(v)
        v += 1
    half = vals[:T // 2]
    parts = [cols(OK, ENQ, half), cols(OK, ENQ, vals[T // 2:]), cols(OK, DEQ, vals[::-1])]
    assert not S.plan_must_grow(T, T // 2, T // 2) and S.plan_must_grow(T, T, T)
    ups, want = follow(dev, parts, TQ, {"slots": T}, maps=False)
    assert [(u.slots, u.grew, u.distinct) for u in ups] == [(T, False, T // 2), (T, False, T), (4 * T, True, T)]
    assert want.counts[0, N.LC_QN_UNEXPECTED] == T and want.counts[0, N.LC_QN_LOST] == 0
    one = [cols(OK, GEN, vals), cols(OK, GEN, vals[:5])]   # the whole table in one append
    ups, want = follow(dev, one, IDS, {"slots": T}, maps=False)
    assert [(u.slots, u.grew, u.distinct) for u in ups] == [(T, False, T), (S.plan_grown(T, 5), True, T)]
    assert want.counts[0, N.LC_QN_OK] == 5


@pytest.mark.parametrize("mode", MODES)
def test_contention_on_one_value(dev, mode):
    """One value acknowledged 65,793 times over two appends, a dequeue among
    them: the tallies are exact and the slot is one distinct value."""
    f = ENQ if mode == TQ else GEN
    n1 = 40000
    first = cat([cols(OK, f, np.full(n1, 7)), cols(OK, DEQ, [7]), cols(INV, GEN, [N.LC_NIL])])
    second = cols(OK, f, np.full(65793 - n1, 7))
    ups, want = follow(dev, [first, second], mode, maps=False)
    assert [u.distinct for u in ups] == [1, 1] and [u.packed for u in ups] == [n1 + (mode == TQ), 65793 - n1]
    if mode == TQ:
        assert want.counts[0].tolist() == [0, 65793, 0, 1, 0, 65792, 0]
        assert (want.ent_class.tolist(), want.ent_mult.tolist()) == ([N.LC_QC_LOST, N.LC_QC_UNEXPECTED], [65792, 1])
    else:
        assert want.counts[0].tolist() == [1, 65793, 1, 0, 0, 0, 0] and want.ent_mult.tolist() == [65793]


def test_keys_in_waves_and_workgroups(dev):
    """Whole workgroups of one key (its rows in a row), then waves that hold
    several keys (round-robin), then both kinds dequeued in another order."""
    run = cols(INV, ENQ, np.arange(3 * T + 5), key=11)
    k = np.arange(5 * 70) % 5
    mixed = cols(OK, ENQ, np.arange(5 * 70) // 5, key=k + 20)
    out = cat([cols(OK, DEQ, np.arange(3 * T + 5)[::-1], key=11), cols(OK, DEQ, (np.arange(5 * 70) // 5)[::3], key=(k + 20)[::3])])
    ups, want = follow(dev, [run, mixed, out], TQ, maps=False)
    assert want.counts[0, N.LC_QN_OK] == 3 * T + 5 and ups[-1].n_keys == 6


def test_keys_appear_late_and_one_goes_unknown(dev):
    """60 new keys per append for six appends: the per-key words double from
    64 to 512.  An :info drain in the third append makes its key :unknown
    beside healthy ones, for good."""
    parts = []
    for j in range(6):
        ops = []
        for k in range(60 * j, 60 * j + 60):
            ops += [H.op("invoke", "enqueue", k % 7, k), H.op("ok", "enqueue", k % 7, k)]
        for k in range(0, 60 * j, 9):
            ops.append(H.op("ok", "dequeue", k % 7, k))
        ops += [H.op("ok", "dequeue", 5, 0), H.op("ok", "enqueue", 99, 1)]   # key 0's rows after the third append must not count
        if j == 2:
            ops[40:40] = [H.op("ok", "dequeue", 3, 0), H.op("info", "drain", None, 0), H.op("ok", "enqueue", 1, 60)]
        parts.append(ops)
    ups, want = follow(dev, parts, TQ)
    assert [u.n_keys for u in ups] == [60 * (j + 1) for j in range(6)]
    assert want.valid[0] == -1 and 0 in ups[2].changed and all(0 not in u.changed for u in ups[3:])
    assert want.counts[0].tolist() == [0] * 7 and want.counts[1, N.LC_QN_LOST] == 7


def test_unique_ids_across_appends(dev):
    parts = [
        [H.op("invoke", "generate", None, 1), H.op("ok", "generate", 10, 1), H.op("invoke", "generate", None, 2)],   # key 2: no ack yet
        [H.op("ok", "generate", 20, 1), H.op("ok", "generate", 5, 1), H.op("invoke", "generate", None, 1)],          # outward both ways
        [H.op("ok", "generate", 10, 1), H.op("ok", "generate", None, 2)],                                              # the duplicate arrives
        [H.op("ok", "generate", H.I64_MAX, 2), H.op("ok", "generate", -7, 1), H.op("ok", "generate", 10, 1)],
    ]
    seen = []
    with QueueStream(dev, IDS) as s:
        for j, p in enumerate(parts):
            u = s.append(p)
            S.same_as_prefix(s, sum(parts[:j + 1], []), IDS, what=j)
            valid, counts, lo, hi, has = s.counts()
            seen.append((valid.tolist(), has.tolist(), int(lo[0]), int(hi[0]), counts[:, 0].tolist(), u.changed))
        assert s.result_map(0)["duplicated"] == {10: 3} and s.result_map(1)["range"] == [None, H.I64_MAX]
    assert seen == [([1, 1], [1, 0], 10, 10, [1, 1], []), ([1, 1], [1, 0], 5, 20, [2, 1], []),
                    ([0, 1], [1, 1], 5, 20, [2, 1], [0]), ([0, 1], [1, 1], -7, 20, [2, 1], [])]


def test_one_drain_of_a_workgroup_and_one_and_the_ent_cap_protocol(dev):
    drained = list(range(T + 1))
    parts = [[H.op("invoke", "drain"), H.op("ok", "drain", drained)], [H.op("ok", "enqueue", -5)]]
    ups, want = follow(dev, parts, TQ)
    assert ups[0].packed == T + 1 and want.counts[0, N.LC_QN_UNEXPECTED] == T + 1 and len(want.ent_key) == T + 2
    with QueueStream(dev, TQ) as s:
        for p in parts:
            s.append(p)
        K, cap = 1, T
        valid, counts = np.zeros(K, np.int8), np.zeros((K, 7), np.uint64)
        lo, hi, has = np.zeros(K, np.int64), np.zeros(K, np.int64), np.zeros(K, np.uint8)
        ek, ec, ev, em = np.zeros(cap, np.uint32), np.zeros(cap, np.uint8), np.zeros(cap, np.int64), np.zeros(cap, np.uint64)
        r = N.LcQueueResult(N.ptr(valid, C.c_int8), N.ptr(counts, C.c_uint64), N.ptr(lo, C.c_int64), N.ptr(hi, C.c_int64),
                            N.ptr(has, C.c_uint8), N.ptr(ek, C.c_uint32), N.ptr(ec, C.c_uint8), N.ptr(ev, C.c_int64),
                            N.ptr(em, C.c_uint64), cap, 0)
        assert N.lib().lc_queue_stream_results(s.handle, C.byref(r)) == -2 and int(r.n_ent) == T + 2   # LC_E_NOMEM, the capacity needed
        assert f"{T + 2} needed" in N.lib().lc_last_error().decode()
        assert valid.tolist() == [0] and counts[0].tolist() == want.counts[0].tolist()   # everything else is written
        again = s.results(ent_cap=1)
        assert again.retried
        H.same_results(again, want)


def test_more_rows_than_one_launch(dev):
    """One launch's row limit plus three in a single append: tallied in two
    pieces, the second of which meets the first's slots settled."""
    L = launch_info()["launch_rows"]
    n, D = L + 3, 4096
    with QueueStream(dev, TQ) as s:
        u = s.append(cols(INV, ENQ, np.arange(n) % D))
        # (the table is sized for the append at its worst, n distinct values)
        assert (u.packed, u.distinct, u.changed, u.grew, u.slots) == (n, D, [], True, S.plan_grown(0, n))
        assert s.counts()[1][0].tolist() == [n, 0, 0, 0, 0, 0, 0]
        u = s.append(cols(OK, DEQ, np.arange(D)))
        # never acknowledged, each out once: ok and recovered
        assert s.counts()[1][0].tolist() == [n, 0, D, 0, 0, 0, D] and u.distinct == D
        res = s.results(ent_cap=16)
        assert res.retried and res.ent_val.tolist() == list(range(D)) and set(res.ent_class.tolist()) == {N.LC_QC_RECOVERED}
        u = s.append(cols(OK, DEQ, np.full(n // D + 2, 2)))   # value 2 went in n // D + 1 times: out twice more than that
        into = n // D + 1
        assert s.counts()[1][0].tolist() == [n, 0, D - 1 + into, 0, 2, 0, D - 1 + into] and u.changed == []
        res = s.results()
        dup = res.ent_class == N.LC_QC_DUPLICATED
        assert (res.ent_val[dup].tolist(), res.ent_mult[dup].tolist()) == ([2], [2]) and res.ent_mult[res.ent_val == 2].tolist() == [2, into]


def test_the_python_surface(dev):
    hist = Q.synth_queue(n_keys=3, n_values=80, lost=2, duplicated=3, unexpected=1, recovered=4, drain=9, seed=5)
    ops = hist.to_ops()
    tq, ui = ck.total_queue(), ck.unique_ids()
    tq.dev = ui.dev = lambda: dev   # the one-shot checks on this module's context too
    with tq.stream(dev) as s:
        for lo in range(0, hist.n, 101):
            s.append(rows_of(hist, lo, lo + 101))
            prefix = ops[:lo + 101]
            want = independent.checker(ck.total_queue({"host": True})).check({}, prefix, {})["results"]
            assert s.result_maps() == want
        assert s.result_maps() == independent.checker(tq).check({}, ops, {})["results"]
        for i, k in enumerate(s.keys()):
            assert s.result_map(i) == tq.check({}, independent.subhistory(ops, k), {})
    ids = Q.synth_ids(n_keys=2, n_values=300, dup_rate=0.2, seed=8)
    with ui.stream(dev) as s:
        for lo in range(0, ids.n, 250):
            s.append(rows_of(ids, lo, lo + 250))
        assert s.result_maps() == independent.checker(ui).check({}, ids, {})["results"]
        assert s.last_timing()["kernel_ms"] > 0
    one = ui.stream(dev)
    one.append([H.op("ok", "generate", 4), H.op("ok", "generate", 4)])
    assert one.result_map(0) == ui.check({}, [H.op("ok", "generate", 4), H.op("ok", "generate", 4)], {})
    one.close()
    with pytest.raises(N.LincheckError, match="unsupported.*one device"):
        QueueStream(ck.Device(0, devices=[0, 0]), TQ)
