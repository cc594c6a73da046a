"""lc_counter_check on the GPU: every case compares valid, n_errors, lower,
upper, err_off and err_idx for equality with the fold of
tests/counter_helpers.py (checker/counter's rules restated; parity with Jepsen
unpinned).  Everything is an integer: no tolerances.  Shapes are the smallest at
which each kernel can go wrong; tile 256 unless a case says otherwise."""
import ctypes as C

import numpy as np
import pytest

import counter_helpers as H
from lincheck import _native as N
from lincheck import checker as ck
from lincheck import counter as CT
from lincheck import independent

pytestmark = pytest.mark.gpu

FIELDS = ("valid", "n_errors", "lower", "upper", "err_off", "err_idx")


@pytest.fixture(scope="module")
def dev(device):
    return ck.Device(0)


def agree(dev, ops, tile=256, err_cap=None, events=None, want=None):
    """Device = fold, array for array.  events: the packed event count the case
    is about; want: the fold's maps when the caller has them key by key already."""
    want = want or H.restate_independent(ops)
    packed = CT.PackedCounter(CT.CounterHistory.from_ops(ops))
    assert packed.keys == list(want)
    if events is not None:
        assert packed.n_events == events
    res = CT.check_batch(dev, packed.view, tile, err_cap)
    exp = H.expected_arrays(want)
    for name in FIELDS:
        got = getattr(res, name)
        assert got.shape == exp[name].shape and np.array_equal(got, exp[name]), \
            (name, np.flatnonzero(got != exp[name])[:8] if got.shape == exp[name].shape else (got.shape, exp[name].shape))
    host = CT.check_batch(None, packed.view, host=True)
    for name in FIELDS:
        assert np.array_equal(getattr(host, name), exp[name]), name
    return packed, res, want


# 1 ---- the hand example and the empty shapes ---------------------------------------------------

def test_hand_example(dev):
    packed, res, want = agree(dev, H.hand_ops(), events=13)
    assert CT.result_map(packed, res, 0) == {"valid?": False, "reads": H.HAND_READS, "errors": H.HAND_ERRORS}
    assert res.timing["kernel_ms"] > 0 and res.timing["total_ms"] > 0


def test_reads_only_adds_only_and_nothing(dev):
    reads = []
    for i in range(5):
        reads += [H.op("invoke", "read", 0), H.op("ok", "read", 0, 0 if i % 2 else 3)]
    _, res, _ = agree(dev, reads, events=10)
    assert res.err_idx.tolist() == [0, 2, 4]
    adds = []
    for i in range(300):
        adds += [H.op("invoke", "add", i % 3, i), H.op("ok", "add", i % 3, i)]
    _, res, _ = agree(dev, adds, events=600)  # R = 0: the judge launches nothing
    assert res.valid.tolist() == [1] and len(res.lower) == 0
    _, res, _ = agree(dev, [], events=0)      # one key, no events, no reads: nothing launches
    assert res.valid.tolist() == [1] and res.err_off.tolist() == [0, 0]
    # an error key alone, and K = 0 through a caller-built batch
    _, res, _ = agree(dev, [H.op("ok", "add", 0, 1)], events=0)
    assert res.valid.tolist() == [-1]
    empty = dict(ev_off=np.zeros(1, np.uint64), ev_kind=[], ev_val=[], read_off=np.zeros(1, np.uint64), read_val=[], status=[])
    res = CT.check_batch(dev, CT.batch_of(empty))
    assert len(res.valid) == 0 and len(res.err_idx) == 0


# 2 ---- one key, every tile-boundary position ---------------------------------------------------

@pytest.mark.parametrize("n", [255, 256, 257, 3 * 256 + 1])
def test_one_key_at_the_tile_boundaries(dev, n):
    """3 * 256 + 1: the middle tiles hold no key head, the carry passes through them."""
    agree(dev, H.exact_key(H.rng_of(n), n, max_add=1000), events=n)


# 3 ---- two keys whose boundary falls around a tile boundary ------------------------------------

@pytest.mark.parametrize("at", [255, 256, 257])
def test_two_keys_meet_at_a_tile_boundary(dev, at):
    """256: the carry must reset at a tile start that is also a key start."""
    rng = H.rng_of(at)
    a, b = H.exact_key(rng, at, max_add=1000), H.exact_key(rng, 300, max_add=1000)
    agree(dev, H.keyed([(5, a), (3, b)]), events=at + 300)
    agree(dev, H.interleave(rng, [(5, a), (3, b)]), events=at + 300)


# 4 ---- many heads in one tile ------------------------------------------------------------------

def test_300_tiny_keys(dev):
    rng = H.rng_of(4)
    groups = []
    for k in range(300):
        kind = k % 4
        if kind == 0:    # adds only: no reads
            ops = [H.op("invoke", "add", 0, rng.randint(0, 9)) for _ in range(1)] + [H.op("info", "add", 0, 1)]
        elif kind == 1:  # reads only: no adds
            ops = [H.op("invoke", "read", 0), H.op("ok", "read", 0, rng.choice([0, 0, 1]))]
        else:
            ops = H.exact_key(rng, rng.randint(1, 5), procs=2, p_wrong=0.3)
        groups.append((1000 - k, ops))
    packed, res, want = agree(dev, H.interleave(rng, groups))
    assert packed.n_keys == 300 and 0 < res.n_errors.sum() < packed.n_reads


# 5 ---- the carry kernel's second chunk -----------------------------------------------------------

BIG = 257 * 256 + 1


def test_one_key_of_65793_events(dev):
    agree(dev, H.exact_key(H.rng_of(5), BIG, p_wrong=0.01, max_add=10 ** 6), events=BIG)


def test_65793_events_over_600_keys(dev):
    rng = H.rng_of(55)
    cuts = sorted(rng.sample(range(1, BIG), 599))
    sizes = [b - a for a, b in zip([0] + cuts, cuts + [BIG])]
    groups = [(k, H.exact_key(rng, n, p_wrong=0.02, max_add=10 ** 6)) for k, n in enumerate(sizes)]
    agree(dev, H.keyed(groups), events=BIG, want={k: H.restate(ops) for k, ops in groups})


# 6 ---- the default tile ----------------------------------------------------------------------------

def test_default_tile_one_key(dev):
    n = 3 * 2048 + 1
    agree(dev, H.exact_key(H.rng_of(6), n, p_wrong=0.05, max_add=10 ** 6), tile=0, events=n)


def test_default_tile_50_keys_across_its_boundaries(dev):
    rng = H.rng_of(66)
    groups = [(k, H.exact_key(rng, rng.randint(100, 400), p_wrong=0.05)) for k in range(50)]
    packed, _, _ = agree(dev, H.keyed(groups), tile=0)
    assert packed.n_events > 3 * 2048
    agree(dev, H.keyed(groups), tile=2048)


# 7 ---- large values ------------------------------------------------------------------------------------

@pytest.mark.parametrize("tile", [256, 0])
def test_large_values_are_summed_exactly(dev, tile):
    """Sums past 2^32 and 2^53 and up to INT64_MAX exactly: a 32-bit or floating-point step shows."""
    adds = [(1 << 32) - 1, 3, (1 << 53) - 1, 1, 1, (1 << 60) + 1, (1 << 61), (1 << 61), (1 << 61)]
    adds.append(H.I64_MAX - sum(adds))
    assert 0 <= adds[-1] <= 1 << 61 and sum(adds) == H.I64_MAX
    ops, acked = [], 0
    for i, v in enumerate(adds):
        ops += [H.op("invoke", "add", 0, v), H.op("invoke", "read", 1), H.op("ok", "add", 0, v)]
        acked += v
        ops += [H.op("ok", "read", 1, acked - (i % 2)), H.op("invoke", "read", 2), H.op("ok", "read", 2, acked + (i % 3 == 1))]
    ops += [H.op("invoke", "add", 0, 0), H.op("info", "add", 0, 0)] * 300  # past one tile
    ops += [H.op("invoke", "read", 1), H.op("ok", "read", 1, H.I64_MAX)]
    _, res, want = agree(dev, ops, tile=tile)
    assert want[None]["reads"][-1] == [H.I64_MAX] * 3 and int(res.upper.max()) == H.I64_MAX


# 8 ---- the judge ---------------------------------------------------------------------------------------

def judged_keys():
    wrong = {0, 255, 256, 257, 599}
    a = []
    for i in range(600):
        a += [H.op("invoke", "add", 0, 1), H.op("ok", "add", 0, 1), H.op("invoke", "read", 1),
              H.op("ok", "read", 1, i + 1 + (i in wrong))]
    b = []
    for i in range(10):
        b += [H.op("invoke", "read", 1), H.op("ok", "read", 1, 1 if i in (2, 9) else 0)]
    c = H.exact_key(H.rng_of(8), 30, p_wrong=0.0)
    d = [H.op("invoke", "read", 0), H.op("ok", "read", 0, -1)]
    return H.keyed([(1, a), (2, b), (3, c), (4, d)])


def test_judge_places_the_errors_in_order_per_key(dev):
    packed, res, want = agree(dev, judged_keys())
    assert res.err_idx.tolist() == [0, 255, 256, 257, 599, 602, 609, packed.n_reads - 1]
    assert res.err_off.tolist() == [0, 5, 7, 7, 8] and res.n_errors.tolist() == [5, 2, 0, 1]
    agree(dev, judged_keys(), tile=0)


def test_err_cap_of_one_says_how_many_and_the_retry_succeeds(dev):
    packed = CT.PackedCounter(CT.CounterHistory.from_ops(judged_keys()))
    K, R = packed.n_keys, packed.n_reads
    valid, n_errors, err_off = np.zeros(K, np.int8), np.zeros(K, np.uint64), np.zeros(K + 1, np.uint64)
    lower, upper, err_idx = np.zeros(R, np.int64), np.zeros(R, np.int64), np.zeros(1, np.uint64)
    r = N.LcCounterResult(N.ptr(valid, C.c_int8), N.ptr(n_errors, C.c_uint64), N.ptr(lower, C.c_int64),
                          N.ptr(upper, C.c_int64), N.ptr(err_off, C.c_uint64), N.ptr(err_idx, C.c_uint64), 1, 0)
    o = N.LcCounterOpts(256, 0)
    assert N.lib().lc_counter_check(dev.handle, C.byref(packed.view), C.byref(o), C.byref(r)) == -2
    assert int(r.n_err) == 8 and b"8 needed" in N.lib().lc_last_error()
    _, res, _ = agree(dev, judged_keys(), err_cap=1)
    assert res.retried and len(res.err_idx) == 8


def test_bad_batches_and_options_are_refused(dev):
    packed = CT.PackedCounter(CT.CounterHistory.from_ops(H.hand_ops()))
    with pytest.raises(N.LincheckError, match="tile"):
        CT.check_batch(dev, packed.view, tile=512)
    a = packed.arrays()
    for name, at, v in (("ev_val", 1, 4), ("ev_val", 1, -1), ("ev_kind", 0, 9)):
        b = {k: x.copy() for k, x in a.items()}
        b[name][at] = v
        with pytest.raises(N.LincheckError, match="invalid"):
            CT.check_batch(dev, CT.batch_of(b), tile=256)
    res = CT.check_batch(dev, CT.batch_of(a), tile=256)  # and the context is as good as before
    assert CT.result_map(packed, res, 0)["errors"] == H.HAND_ERRORS


# 9 ---- a synthetic batch through the checkers ---------------------------------------------------------

def test_synth_batch_through_independent_checker(dev):
    hist = CT.synth_counter(n_keys=64, ops_per_key=400, concurrency=5, info_rate=0.05, fail_rate=0.05, stale_rate=0.02, seed=9)
    ops = hist.to_ops()
    want = H.restate_independent(ops)
    r = independent.checker(ck.counter()).check({}, hist, {})
    assert r["results"] == want and len(want) == 64
    assert r["failures"] == [k for k in want if want[k]["valid?"] is False] and r["failures"]
    assert r["valid?"] is False
    r = independent.checker(ck.counter({"tile": 256})).check({}, ops, {})
    assert r["results"] == want


def test_compose_next_to_perf(dev):
    ops = [dict(o, time=1000 * i) for i, o in enumerate(H.hand_ops())]
    r = ck.compose({"perf": ck.perf(), "counter": ck.counter()}).check({}, ops, {})
    assert r["perf"]["valid?"] is True and r["valid?"] is False
    assert r["counter"] == {"valid?": False, "reads": H.HAND_READS, "errors": H.HAND_ERRORS}


# 10 ---- the EDN path end to end -------------------------------------------------------------------------

def test_edn_file_end_to_end(dev, tmp_path):
    rng = H.rng_of(10)
    groups = [(k, H.exact_key(rng, 100, p_wrong=0.1)) for k in range(6)]
    groups[4] = (4, H.break_key(rng, groups[4][1], "negative-add"))
    ops = H.interleave(rng, groups)
    path = tmp_path / "history.edn"
    path.write_text(H.write_edn(ops))
    want = H.restate_independent(ops)
    r = independent.checker(ck.counter()).check({}, CT.CounterHistory.read_edn(str(path)), {})
    assert list(r["results"]) == list(want) and all(H.same(r["results"][k], want[k]) for k in want)
    assert r["results"][4]["valid?"] == "unknown"
