"""The streaming checker/counter on the device against lc_counter_pack +
lc_counter_check_host of the prefix (and, for the small cases, the restatement
of tests/counter_helpers.py) after EVERY append: the hand-built cases row by
row, seeded random histories at their cuts, the scan at the tile's edges with
segments that start from resident sums, patches over resident reads in every
arrangement, the reads array growing, an append of several launches, and the
results() protocol.  tile = 256 (T) throughout, so that a few hundred events
cross workgroups."""
import numpy as np
import pytest

import counter_helpers as H
import counter_stream_helpers as S
from lincheck import _native as N
from lincheck import checker as ck
from lincheck import counter as CT
from lincheck import independent
from lincheck.counter_stream import CounterStream, rows_of

pytestmark = pytest.mark.gpu

T = S.T
OPTS = {"tile": T}
CASES = S.hand_cases()


@pytest.fixture(scope="module")
def dev(device):
    return ck.Device(0)


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_built_cases_row_by_row(dev, name):
    S.follow(dev, CASES[name], OPTS)


@pytest.mark.parametrize("seed", [0, 3, 5])
def test_random_histories_at_their_cuts(dev, seed):
    parts = S.random_case(seed, 0)
    out = S.follow(dev, parts, OPTS)
    assert sum(u.patched for u, _ in out) > 0 and sum(len(u.changed) for u, _ in out) >= 3


def test_the_default_tile_on_a_random_history(dev):
    S.follow(dev, S.random_case(1, 0), None)


# ---- the scan ----------------------------------------------------------------------------------

def first_append():
    """Leaves lower = 3, upper = 7 and an open read behind."""
    return [H.op("invoke", "add", 30, 3), H.op("ok", "add", 30, 3), H.op("invoke", "add", 31, 4), H.op("invoke", "read", 32)]


@pytest.mark.parametrize("n", [T - 1, T, T + 1, 3 * T + 1])
def test_one_key_at_the_tile_edges_from_resident_sums(dev, n):
    second = S.events_exactly(n)
    out = S.follow(dev, [first_append(), second, [H.op("ok", "read", 32, 5)]], OPTS, maps=False)
    assert out[1][0].events == n and out[0][0].events == 4


def test_a_segment_that_starts_on_a_tiles_first_event(dev):
    a = [S.kop(1, "invoke", "add", 0, 2), S.kop(1, "ok", "add", 0, 2), S.kop(2, "invoke", "add", 0, 10), S.kop(2, "ok", "add", 0, 10)]
    b = H.keyed([(1, S.events_exactly(T)), (2, S.events_exactly(T + 9)), (1, S.events_exactly(6))])
    out = S.follow(dev, [a, b], OPTS, maps=False)
    assert out[1][0].events == 2 * T + 15


@pytest.mark.parametrize("n_keys", [64, 257])
def test_many_keys_of_one_event_each(dev, n_keys):
    a, b, c = [], [], []
    for k in range(n_keys):
        a += [S.kop(k, "invoke", "add", 0, k), S.kop(k, "ok", "add", 0, k), S.kop(k, "invoke", "read", 1)]
        b += [S.kop(k, "invoke", "add", 2, 1)]
        c += [S.kop(k, "ok", "read", 1, k + (k % 7 == 0))]
    out = S.follow(dev, [a, b, c], OPTS, maps=False)
    assert out[1][0].events == n_keys and out[2][0].reads == n_keys


def test_an_append_larger_than_one_launch(dev):
    a = [S.kop(1, "invoke", "add", 0, 2), S.kop(1, "ok", "add", 0, 2), S.kop(2, "invoke", "add", 20, 10)]
    b = H.keyed([(1, S.events_exactly(T + 40)), (2, S.events_exactly(2 * T + 5))])   # key 2's segment spans three launches
    c = [S.kop(2, "fail", "add", 20, 10), S.kop(1, "invoke", "read", 3), S.kop(1, "ok", "read", 3, 0)]
    out = S.follow(dev, [a, b, c], {"tile": T, "launch-events": 100}, maps=False)   # 100: rounded up to one tile, 256
    assert out[1][0].events == 3 * T + 45 and out[2][0].patched == 1


# ---- patches -----------------------------------------------------------------------------------

def reads_of_two_keys(n, open_add):
    """open_add (an :invoke :add of key 1 that stays open), then n :ok reads of
    key 1 mixed with n of key 2; every fifth is out of bounds already."""
    out = [S.kop(1, "invoke", "add", 0, 4), S.kop(1, "ok", "add", 0, 4), S.kop(2, "invoke", "add", 0, 6), S.kop(2, "ok", "add", 0, 6)]
    out += open_add
    for i in range(n):
        out += [S.kop(1, "invoke", "read", 1), S.kop(2, "invoke", "read", 1), S.kop(1, "ok", "read", 1, 7 if i % 5 else 99),
                S.kop(2, "ok", "read", 1, 6 if i % 5 else -1)]
    return out


def test_a_fail_behind_many_resident_reads(dev):
    n = 2 * T + 1
    a = reads_of_two_keys(n, [S.kop(1, "invoke", "add", 9, 5)])
    out = S.follow(dev, [a, [S.kop(1, "fail", "add", 9, 5)], [S.kop(1, "invoke", "read", 1), S.kop(1, "ok", "read", 1, 7)]], OPTS,
                   maps=False)
    u = out[1][0]
    # key 1's reads of 7 were within [4, 9] and are above [4, 4] now; key 2's are looked at and do not move
    assert (u.patched, u.revisited, u.changed, u.events) == (1, 2 * n, [], 0)
    with CounterStream(dev, OPTS) as s:
        s.append(a)
        was = s.results()
        s.append([S.kop(1, "fail", "add", 9, 5)])
        now = s.results()
        k1 = slice(0, n)
        assert (was.upper[k1] == 9).all() and (now.upper[k1] == 4).all() and np.array_equal(was.upper[n:], now.upper[n:])
        assert int(was.n_errors[0]) == -(-n // 5) and int(now.n_errors[0]) == n and np.array_equal(was.n_errors[1:], now.n_errors[1:])


def test_a_fail_with_no_read_behind_it_moves_only_the_sums(dev):
    a = reads_of_two_keys(40, []) + [S.kop(1, "invoke", "add", 9, 5)]
    out = S.follow(dev, [a, [S.kop(1, "fail", "add", 9, 5)], [S.kop(1, "invoke", "read", 1), S.kop(1, "ok", "read", 1, 7)]], OPTS,
                   maps=False)
    assert (out[1][0].patched, out[1][0].revisited) == (1, 0)
    with CounterStream(dev, OPTS) as s:
        for part in (a, [S.kop(1, "fail", "add", 9, 5)], [S.kop(1, "invoke", "read", 1), S.kop(1, "ok", "read", 1, 7)]):
            s.append(part)
        assert s.result_map(0)["reads"][-1] == [4, 7, 4]


def patch_history():
    """Key 1: adds of 5 (process 8) and 3 (process 9) invoked at different
    reads; key 2: an add of 2 (process 8) invoked between its reads."""
    a = [S.kop(1, "invoke", "add", 0, 4), S.kop(1, "ok", "add", 0, 4), S.kop(2, "invoke", "add", 0, 6), S.kop(2, "ok", "add", 0, 6)]
    for i in range(60):
        if i == 10:
            a.append(S.kop(1, "invoke", "add", 8, 5))
        if i == 25:
            a.append(S.kop(2, "invoke", "add", 8, 2))
        if i == 40:
            a.append(S.kop(1, "invoke", "add", 9, 3))
        a += [S.kop(1, "invoke", "read", 1), S.kop(2, "invoke", "read", 1), S.kop(1, "ok", "read", 1, 4 + i % 9),
              S.kop(2, "ok", "read", 1, 6 + i % 3)]
    return a


PATCHES = {
    "two-on-one-key": ([S.kop(1, "fail", "add", 8, 5), S.kop(1, "fail", "add", 9, 3)], 2, 2 * 50),
    "on-two-keys": ([S.kop(2, "fail", "add", 8, 2), S.kop(1, "fail", "add", 9, 3)], 2, 2 * 35),
    "a-positive-and-a-negative-delta": ([S.kop(1, "ok", "add", 9, 11), S.kop(1, "fail", "add", 8, 5)], 2, 2 * 50),
    "an-ok-with-the-same-value": ([S.kop(1, "ok", "add", 9, 3)], 1, 0),
}


@pytest.mark.parametrize("name", sorted(PATCHES))
def test_patches_in_one_append(dev, name):
    second, patched, revisited = PATCHES[name]
    out = S.follow(dev, [patch_history(), second, [S.kop(1, "invoke", "read", 1), S.kop(2, "invoke", "read", 1),
                                                   S.kop(1, "ok", "read", 1, 9), S.kop(2, "ok", "read", 1, 7)]], OPTS, maps=False)
    assert (out[1][0].patched, out[1][0].revisited) == (patched, revisited)


# ---- growth and results() ----------------------------------------------------------------------

def test_the_reads_array_grows_with_the_earlier_reads_intact(dev):
    a = S.events_exactly(2 * 256, read_every=1)   # 256 reads: the first capacity exactly
    b = [H.op("invoke", "add", 40, 5)] + S.events_exactly(2 * 3, read_every=1)
    c = [H.op("fail", "add", 40, 5)]
    out = S.follow(dev, [a, b, c], {"tile": T, "reads": 256}, maps=False)
    assert [u.grew for u, _ in out] == [False, True, False] and [u.reads_total for u, _ in out] == [256, 259, 259]
    assert (out[2][0].patched, out[2][0].revisited) == (1, 3)


def test_results_twice_and_a_small_err_cap(dev):
    hist = CT.synth_counter(n_keys=3, ops_per_key=400, stale_rate=0.2, fail_rate=0.1, seed=4)
    with CounterStream(dev, OPTS) as s:
        for lo in range(0, hist.n, 301):
            s.append(rows_of(hist, lo, lo + 301))
        S.same_as_prefix(s, hist, maps=False)
        full = s.results()
        s._results = None
        twice = s.results()
        small = s.results(err_cap=3)
        assert len(full.err_idx) > 10 and not full.retried and small.retried
        for name in ("valid", "n_errors", "lower", "upper", "err_off", "err_idx"):
            assert np.array_equal(getattr(full, name), getattr(twice, name)), name
            assert np.array_equal(getattr(full, name), getattr(small, name)), name
        assert s.last_timing()["kernel_ms"] > 0


def test_the_python_surface(dev):
    hist = CT.synth_counter(n_keys=4, ops_per_key=300, stale_rate=0.05, fail_rate=0.1, info_rate=0.1, seed=3)
    ops = hist.to_ops()
    c = ck.counter({"tile": T})
    host = ck.counter({"host": True})
    with c.stream(dev) as s:
        so_far = []
        for lo in range(0, hist.n, 700):
            s.append(ops[lo:lo + 700])
            so_far += ops[lo:lo + 700]
            assert s.result_maps() == independent.checker(host).check({}, so_far, {})["results"]
        assert s.dev is dev
        for i, k in enumerate(s.keys()):
            assert s.result_map(i) == host.check({}, independent.subhistory(ops, k), {})
    one = H.hand_ops()
    with c.stream(dev) as s:
        s.append(one)
        assert s.result_map(0) == c.check({}, one, {}) == {"valid?": False, "reads": H.HAND_READS, "errors": H.HAND_ERRORS}


def test_a_context_of_several_devices_is_refused(dev):
    with pytest.raises(N.LincheckError, match="unsupported.*one device"):
        CounterStream(ck.Device(0, devices=[0, 0]), OPTS)
