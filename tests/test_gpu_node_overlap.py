"""lc_check_node_async with two search lanes: consecutive enqueued
register-tier steps search on two streams and overlap (csrc/lane_plan.hpp),
three steps in flight.  Whatever overlaps, every step's records must equal
lc_check_node's on a fresh context, a buffer given to several steps must end
up with the latest one's records, errors must name their own step, and a
synchronous call must see everything enqueued before it.
LC_PATH_NODE_SERIAL (one search at a time) gives the same bytes."""
import ctypes as C
import itertools

import numpy as np
import pytest

import cref
from lincheck import _native as N
from lincheck import history as H
from lincheck import parallel as P
from lincheck.checker import Device, Packed, PinnedRecords

pytestmark = pytest.mark.gpu

PAD = 3  # records of padding behind every shard's keys (must come back 0)
SHAPES = {
    # long keys, few of them: the step that ends last when all start together
    "L": dict(n_keys=120, ops_per_key=900, concurrency=10, anomaly_rate=0.2, seed=91),
    # short: would finish first if the downloads were unordered
    "S": dict(n_keys=300, ops_per_key=60, concurrency=6, anomaly_rate=0.1, seed=92),
    "M": dict(n_keys=300, ops_per_key=400, concurrency=10, anomaly_rate=0.1, seed=93),
    # more keys than the others: bigger workspaces, result arrays and record blocks
    "G": dict(n_keys=1000, ops_per_key=200, concurrency=10, anomaly_rate=0.05, seed=94),
}


class Case:
    def __init__(self, name):
        self.hist = H.synth(**SHAPES[name])
        self.pk = Packed(self.hist)
        self.block = self.pk.n_keys + PAD
        self.ref = Device(0).check_node(self.pk, self.block)[0].copy()  # a fresh context, synchronous


@pytest.fixture(scope="module")
def cases():
    cs = {name: Case(name) for name in SHAPES}
    for c in cs.values():
        assert c.ref.size == c.block and not c.ref[-PAD:].any()
    assert any(P.unpack_records(c.ref.astype(np.int64))[0][:c.pk.n_keys].min() == 0 for c in cs.values())
    return cs


def _enqueue(dev, case, buf):
    enq, _ = dev.check_node_async(case.pk, case.block, buf)
    assert enq


ORDERS = [p for n in (2, 3) for p in itertools.permutations("LSM", n)]


@pytest.mark.parametrize("order", ORDERS, ids=["".join(o) for o in ORDERS])
def test_same_buffer_holds_the_latest_step(cases, order):
    """Steps of different lengths given one buffer, no wait between: after
    the wait it holds the last enqueued step's records, not those of whichever
    search ended last; with a buffer each, every step's are its own."""
    dev = Device(0)
    buf = PinnedRecords(max(c.block for c in cases.values()))
    buf[:] = 0xDEAD
    for name in order:
        _enqueue(dev, cases[name], buf)
    n, _ = dev.wait()
    assert n == len(order)
    last = cases[order[-1]]
    np.testing.assert_array_equal(np.asarray(buf)[:last.block], last.ref)
    bufs = [PinnedRecords(cases[name].block) for name in order]
    for name, b in zip(order, bufs):
        _enqueue(dev, cases[name], b)
    assert dev.wait()[0] == len(order)
    for name, b in zip(order, bufs):
        np.testing.assert_array_equal(np.asarray(b), cases[name].ref, err_msg=name)


def test_same_buffer_by_wait_step(cases):
    """lc_wait_step over the latest step is enough for the buffer to hold its
    records (the download is part of the step), and partly overlapping
    buffers are ordered like equal ones."""
    dev = Device(0)
    big = PinnedRecords(cases["M"].block + 64)
    _enqueue(dev, cases["L"], big[:cases["L"].block])
    _enqueue(dev, cases["S"], big[64:64 + cases["S"].block])
    _enqueue(dev, cases["M"], big[32:32 + cases["M"].block])
    dev.wait_step(0)
    np.testing.assert_array_equal(np.asarray(big[32:32 + cases["M"].block]), cases["M"].ref)
    assert dev.wait()[0] == 3


@pytest.mark.parametrize("segs", [8, 4, 2])
def test_reruns_on_both_lanes(cases, segs):
    """Checkpoints at the cut (spec_ck (0, 0)) leave most keys to the
    unsegmented rerun: each lane has its own rerun list and counters, so nine
    alternating steps, each with its own buffer, all equal their references."""
    dev = Device(0, path_flags=N.LC_PATH_SPLIT_OFF, spec_segs=segs, spec_ck=(0, 0))
    names = ["L", "M"] * 4 + ["L"]
    bufs = [PinnedRecords(cases[name].block) for name in names]
    for name, b in zip(names, bufs):
        _enqueue(dev, cases[name], b)
    assert dev.wait()[0] == len(names)
    for i, (name, b) in enumerate(zip(names, bufs)):
        np.testing.assert_array_equal(np.asarray(b), cases[name].ref, err_msg=f"step {i} ({name})")


def _batch_copy(pk):
    """Writable copies of a packed batch's arrays and an lc_batch over them."""
    K = pk.n_keys
    arrs = dict(ev_off=pk.ev_off.copy(), events=pk.all_events(),
                trans=np.ctypeslib.as_array(pk.view.trans, shape=(int(pk.view.n_trans),)).copy(),
                width=np.ctypeslib.as_array(pk.view.key_width, shape=(K,)).copy(),
                states=np.ctypeslib.as_array(pk.view.key_states, shape=(K,)).copy())
    b = N.LcBatch()
    b.n_keys = K
    b.ev_off = N.ptr(arrs["ev_off"], C.c_uint64)
    b.events = N.ptr(arrs["events"], C.c_uint32)
    b.trans = N.ptr(arrs["trans"], C.c_uint32)
    b.n_trans = int(pk.view.n_trans)
    b.key_width = N.ptr(arrs["width"], C.c_uint8)
    b.key_states = N.ptr(arrs["states"], C.c_uint16)
    return arrs, b


def test_errors_name_their_own_step_with_three_in_flight(cases):
    """Three malformed copies of one batch, a different bad key in each,
    enqueued back to back on the two lanes: the wait for each step names
    that step's key, nothing is left for lc_wait, and the context goes on."""
    case = cases["M"]
    K = case.pk.n_keys
    dev = Device(0)
    keep = []
    for bad_key in (40, 211, 137):
        arrs, b = _batch_copy(case.pk)
        arrs["events"][int(case.pk.ev_off[bad_key])] |= N.LC_EV_OK_BIT  # an :ok of a slot with no pending op
        out = PinnedRecords(case.block)
        rc = N.check(N.lib().lc_check_node_async(dev.handle, C.byref(b), case.block, N.ptr(out, C.c_uint64), None))
        assert rc == 1
        keep.append((arrs, b, out))
    for back, bad_key in ((2, 40), (1, 211), (0, 137)):
        with pytest.raises(N.LincheckError) as ei:
            dev.wait_step(back)
        assert ei.value.code == -1 and f"key {bad_key}" in str(ei.value), str(ei.value)
    assert dev.wait()[0] == 3  # nothing left to report
    good = PinnedRecords(case.block)
    _enqueue(dev, case, good)
    dev.wait_step(0)
    np.testing.assert_array_equal(np.asarray(good), case.ref)
    assert dev.wait()[0] == 1


def _empty_batch():
    keep = np.zeros(1, np.uint64)  # ev_off of no keys
    b = N.LcBatch()
    b.n_keys = 0
    b.ev_off = N.ptr(keep, C.c_uint64)
    return keep, b


@pytest.fixture(scope="module")
def small_steps():
    """Three steps of 8 keys x 40 ops, one key invalid in each, and their
    lc_check_node records on a fresh context."""
    steps = []
    for seed in (60, 63, 64):
        pk = Packed(H.synth(n_keys=8, ops_per_key=40, concurrency=5, anomaly_rate=0.15, seed=seed))
        ref = Device(0).check_node(pk, pk.n_keys + PAD)[0].copy()
        assert (P.unpack_records(ref.astype(np.int64))[0][:pk.n_keys] == 0).sum() == 1
        steps.append((pk, ref))
    return steps


# (what, Device arguments, page-locked buffers, one buffer for all steps, no keys, the return code)
EXITS = [
    ("pageable", {}, False, False, False, 0),
    ("direct", {}, True, False, False, 1),
    ("lane_block", {}, True, True, False, 1),
    ("node_sync", dict(path_flags=N.LC_PATH_NODE_SYNC), True, False, False, 0),
    ("count_probes", dict(count_probes=True), True, False, False, 0),
    ("no_keys", {}, True, False, True, 0),
]


@pytest.mark.parametrize("what,kw,page_locked,shared,no_keys,want_rc", EXITS, ids=[e[0] for e in EXITS])
def test_every_exit_of_the_enqueue_path(small_steps, what, kw, page_locked, shared, no_keys, want_rc):
    """Every way out of lc_check_node_async, three steps back to back: it
    returns 1 where the step is enqueued and 0 where it ran as lc_check_node
    (a pageable buffer, LC_PATH_NODE_SYNC, probe counting, no keys), and the
    node's bytes are lc_check_node's either way, padding zeroed."""
    dev = Device(0, **kw)
    block = 8 + PAD
    make = PinnedRecords if page_locked else (lambda n: np.zeros(n, np.uint64))
    one = make(block)
    bufs = [one if shared else make(block) for _ in small_steps]
    keep = []
    for (pk, _), buf in zip(small_steps, bufs):
        buf[:] = 0xDEAD
        keep.append(_empty_batch() if no_keys else (pk, pk.view))
        rc = N.check(N.lib().lc_check_node_async(dev.handle, C.byref(keep[-1][1]), block, N.ptr(buf, C.c_uint64), None))
        assert rc == want_rc
    assert dev.wait()[0] == (3 if want_rc else 0)
    if no_keys:
        fresh, empty = Device(0), np.full(block, 0xDEAD, np.uint64)
        N.check(N.lib().lc_check_node(fresh.handle, C.byref(keep[0][1]), block, N.ptr(empty, C.c_uint64), None))
    for i, ((_, ref), buf) in enumerate(zip(small_steps, bufs)):
        want = empty if no_keys else small_steps[-1][1] if shared else ref
        assert not want[0 if no_keys else 8:].any()
        np.testing.assert_array_equal(np.asarray(buf), want, err_msg=f"{what}: step {i}")


def test_synchronous_calls_behind_enqueued_steps(cases):
    """lc_check_batch and lc_check_node right behind three enqueued steps,
    no wait between: both see a context whose lanes they have joined and give
    the oracle's verdicts; the three steps' buffers are untouched by them."""
    dev = Device(0)
    names = ["L", "M", "S"]
    bufs = [PinnedRecords(cases[name].block) for name in names]
    for name, b in zip(names, bufs):
        _enqueue(dev, cases[name], b)
    case = cases["M"]
    K = case.pk.n_keys
    res = dev.check(case.pk)
    rec, _ = dev.check_node(case.pk, case.block)
    rec = rec.copy()
    _, orc = cref.check_history(case.hist.as_c(), budget=dev.budget, threads=8)
    np.testing.assert_array_equal(res.valid, orc["valid"])
    np.testing.assert_array_equal(res.fail_event, orc["fail_event"])
    v, _, fe = P.unpack_records(rec.astype(np.int64))
    np.testing.assert_array_equal(v[:K], orc["valid"])
    np.testing.assert_array_equal(fe[:K], orc["fail_event"])
    np.testing.assert_array_equal(rec, case.ref)
    dev.wait()
    for name, b in zip(names, bufs):
        np.testing.assert_array_equal(np.asarray(b), cases[name].ref, err_msg=name)


@pytest.mark.parametrize("same_buffer", [False, True])
def test_growth_while_in_flight(cases, same_buffer):
    """A step with more keys than any before it, behind two in flight: the
    lanes' workspaces, result arrays and record blocks are regrown only once
    nothing uses them."""
    dev = Device(0)
    names = ["S", "S", "G", "S"]
    shared = PinnedRecords(cases["G"].block)
    bufs = [shared if same_buffer else PinnedRecords(cases[name].block) for name in names]
    for name, b in zip(names, bufs):
        _enqueue(dev, cases[name], b)
        if same_buffer and name == "G":  # (the one buffer: look at the big step's records before the next lands)
            dev.wait_step(0)
            np.testing.assert_array_equal(np.asarray(shared), cases["G"].ref)
    assert dev.wait()[0] == len(names)
    if same_buffer:
        np.testing.assert_array_equal(np.asarray(shared)[:cases["S"].block], cases["S"].ref)
    else:
        for i, (name, b) in enumerate(zip(names, bufs)):
            np.testing.assert_array_equal(np.asarray(b), cases[name].ref, err_msg=f"step {i} ({name})")


def test_serial_and_overlapping_give_the_same_bytes(cases):
    """The A/B switch: the same 12 mixed steps under LC_PATH_NODE_SERIAL and
    under the default, a buffer per step; byte-identical, and both waits
    count 12 steps."""
    seq = ["M", "L", "S", "G", "S", "L", "L", "M", "G", "S", "M", "L"]
    got = {}
    for what, flags in (("serial", N.LC_PATH_NODE_SERIAL), ("lanes", 0)):
        dev = Device(0, path_flags=flags)
        bufs = [PinnedRecords(cases[name].block) for name in seq]
        for name, b in zip(seq, bufs):
            _enqueue(dev, cases[name], b)
        assert dev.wait()[0] == 12
        got[what] = [np.asarray(b).copy() for b in bufs]
    for i, name in enumerate(seq):
        assert got["serial"][i].tobytes() == got["lanes"][i].tobytes(), f"step {i} ({name})"
        np.testing.assert_array_equal(got["lanes"][i], cases[name].ref, err_msg=f"step {i} ({name})")
