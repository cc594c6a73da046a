"""lc_counter_check_history on the GPU: a raw history grouped, paired, packed
and checked on the device.  The oracle everywhere is the unchanged host path,
lc_counter_pack + lc_counter_check_host: every case compares the keys and their
order, every key's error text, the batch the device built
(lc_counter_checked_batch: ev_off, ev_kind, ev_val, read_off, read_val, status)
and the results (valid, n_errors, lower, upper, err_off, err_idx) for equality.
Everything is an integer: no tolerances.  Shapes are the smallest at which each
kernel can go wrong; tile 256 unless a case says otherwise."""
import ctypes as C

import numpy as np
import pytest

import counter_helpers as H
import counter_pack_helpers as PH
from lincheck import _native as N
from lincheck import checker as ck
from lincheck import counter as CT
from lincheck import independent

pytestmark = pytest.mark.gpu

I, O, F, X, A, R, Z = PH.INVOKE, PH.OK, PH.FAIL, PH.INFO, PH.ADD, PH.READ, PH.OTHER
I64_MIN = -(1 << 63)


@pytest.fixture(scope="module")
def dev(device):
    return ck.Device(0)


def agree(dev, h, tile=256):
    """Device = host, array for array.  Returns the host's answer."""
    want, _, _ = PH.host_answer(h)
    c = CT.CheckedCounter(dev, h, tile)
    got = c.arrays()
    got["keys"] = c.keys
    got["error"] = [c.key_error(i) for i in range(c.n_keys)]
    for name in PH.RESULT:
        got[name] = getattr(c.res, name)
    PH.same_batch(got, want, PH.BATCH + PH.RESULT + ("keys", "error"))
    assert np.array_equal(c.read_val(), want["read_val"])
    local = PH.local_pack(h)
    assert [c.key_error_row(i) for i in range(c.n_keys)] == local["error_row"]
    return want


def launch_info():
    out = (C.c_int64 * 3)()
    N.check(N.lib().lc_counter_pack_launch_info(out))
    return list(out)


def well_formed(rng, n_rows, n_keys, n_procs, **kw):
    return PH.random_rows(rng, n_rows, n_keys, n_procs, p_wild=0.0, **kw)


# ---- 1. empty and degenerate batches ----------------------------------------------------------

def test_no_rows(dev):
    want = agree(dev, PH.hist([]))
    assert want["keys"] == [None] and list(want["valid"]) == [1]
    agree(dev, PH.hist([], keyed=False, with_process=False))


def test_rows_that_take_no_part(dev):
    rows = [(X, Z, None, None, None), (I, Z, 3, None, 1), (I, A, None, None, 1), (O, A, None, None, 1)]
    assert agree(dev, PH.hist(rows))["keys"] == [None]
    # a key none of whose rows is a client's is still a key
    assert agree(dev, PH.hist([(I, Z, 3, 9, None), (I, A, None, 4, 1), (I, A, 0, 5, 1)]))["keys"] == [9, 4, 5]


def test_key_column_absent_all_none_and_interleaved(dev):
    rng = PH.rng_of(1)
    rows = well_formed(rng, 300, 0, 3)
    a = agree(dev, PH.hist(rows, keyed=False))
    b = agree(dev, PH.hist(rows, keyed=True))
    assert a["keys"] == b["keys"] == [None] and len(a["read_val"]) > 10
    rows = well_formed(rng, 400, 3, 3)
    mixed = [r if i % 3 else (r[0], r[1], r[2], None, r[4]) for i, r in enumerate(rows)]  # every third row loses its key
    want = agree(dev, PH.hist(mixed))
    assert len(want["keys"]) == 3


def test_process_column_absent(dev):
    rows = [(I, A, None, None, 2), (O, A, None, None, 2), (I, R, None, None, None), (O, R, None, None, 2), (I, A, None, None, 1)]
    want = agree(dev, PH.hist(rows, keyed=False, with_process=False))
    assert list(want["ev_kind"]) == [0, 1, 2, 3, 0] and list(want["valid"]) == [1]


# ---- 2. error keys ----------------------------------------------------------------------------

ALONE = {
    PH.SECOND_INVOKE: [(I, R, 0, None, None), (I, R, 0, None, None)],
    PH.NO_OPEN: [(O, A, 0, None, 1)],
    PH.OTHER_F: [(I, A, 0, None, 1), (O, R, 0, None, 1)],
    PH.READ_NIL: [(I, R, 0, None, None), (O, R, 0, None, None)],
    PH.ADD_NIL: [(I, A, 0, None, None)],
    PH.ADD_NEGATIVE: [(I, A, 0, None, 1), (O, A, 0, None, -1)],
    PH.SUM: [(I, A, 0, None, PH.I64_MAX), (I, A, 1, None, 1)],
}


@pytest.mark.parametrize("message", PH.MESSAGES)
def test_each_message_alone(dev, message):
    good = [(I, A, 5, None, 1), (O, A, 5, None, 1)]
    assert agree(dev, PH.hist(good + ALONE[message] + good, keyed=False))["error"] == [message]


def test_the_lower_row_decides_in_both_orders(dev):
    a, b = ALONE[PH.NO_OPEN], [(I, R, 1, None, None), (I, R, 1, None, None)]
    assert agree(dev, PH.hist(a + b, keyed=False))["error"] == [PH.NO_OPEN]
    assert agree(dev, PH.hist(b + a, keyed=False))["error"] == [PH.SECOND_INVOKE]
    # rule 1 goes before rule 3 whatever the rows
    assert agree(dev, PH.hist(ALONE[PH.ADD_NEGATIVE] + a, keyed=False))["error"] == [PH.NO_OPEN]
    # two rule-3 offences: the earlier event's
    assert agree(dev, PH.hist(ALONE[PH.ADD_NIL] + [(I, A, 1, None, -4)], keyed=False))["error"] == [PH.ADD_NIL]
    assert agree(dev, PH.hist([(I, A, 1, None, -4)] + ALONE[PH.ADD_NIL], keyed=False))["error"] == [PH.ADD_NEGATIVE]


def test_an_error_key_between_two_good_keys(dev):
    good = [(I, A, 0, 0, 2), (O, A, 0, 0, 2), (I, R, 1, 0, None), (O, R, 1, 0, 2)]
    rows = [(t, f, p, 10, v) for t, f, p, _, v in good] + [(O, R, 0, 11, 1), (I, A, 0, 11, 1)] + [(t, f, p, 12, v) for t, f, p, _, v in good]
    want = agree(dev, PH.hist(rows))
    assert list(want["ev_off"]) == [0, 4, 4, 8] and list(want["read_off"]) == [0, 1, 1, 2] and list(want["valid"]) == [1, -1, 1]


def test_nil_invoke_repaired_and_the_sum_at_its_edge(dev):
    assert agree(dev, PH.hist([(I, A, 0, None, None), (O, A, 0, None, 3)], keyed=False))["error"] == [None]
    big = [(I, A, 0, None, PH.I64_MAX - 1), (I, A, 1, None, 1)]
    assert agree(dev, PH.hist(big, keyed=False))["error"] == [None]
    assert agree(dev, PH.hist(big + [(I, A, 2, None, 1)], keyed=False))["error"] == [PH.SUM]
    halves = [(I, A, p, None, 1 << 62) for p in range(2)]
    assert agree(dev, PH.hist(halves, keyed=False))["error"] == [PH.SUM]
    assert agree(dev, PH.hist([(I, A, 0, None, (1 << 62) - 1), (I, A, 1, None, 1 << 62)], keyed=False))["error"] == [None]
    # a nil add before the overflow point, and after it
    assert agree(dev, PH.hist([(I, A, 3, None, None)] + big + [(I, A, 2, None, 1)], keyed=False))["error"] == [PH.ADD_NIL]
    assert agree(dev, PH.hist(big + [(I, A, 2, None, 1), (I, A, 3, None, None)], keyed=False))["error"] == [PH.SUM]
    # the sum starts over at every key: two keys of INT64_MAX each
    assert agree(dev, PH.hist([(I, A, 0, 1, PH.I64_MAX), (I, A, 0, 2, PH.I64_MAX)]))["error"] == [None, None]


def test_bad_codes_name_the_lowest_row(dev):
    rows = [(I, A, 0, None, 1)] * 600
    for bad, at in (((7, A, 0, None, 1), 300), ((I, 5, 0, None, 1), 17)):
        h = PH.hist(rows[:at] + [bad] + rows[at:] + [bad], keyed=False)
        with pytest.raises(N.LincheckError) as e:
            CT.CheckedCounter(dev, h, 256)
        assert e.value.code == -1 and f"row {at}: bad :type / :f code" in str(e.value)
        with pytest.raises(N.LincheckError) as e:
            CT.PackedCounter(h)
        assert f"row {at}: bad :type / :f code" in str(e.value)


# ---- 3. survivor rules ------------------------------------------------------------------------

@pytest.mark.parametrize("f, t", [(f, t) for f in (A, R) for t in (F, X, None)])
def test_fail_info_and_open_each_alone(dev, f, t):
    rows = [(I, f, 0, None, 3 if f == A else None)] + ([(t, f, 0, None, 3 if f == A else None)] if t is not None else [])
    want = agree(dev, PH.hist(rows + [(I, R, 1, None, None), (O, R, 1, None, 0)], keyed=False))
    assert list(want["ev_kind"]) == ([0] if f == A and t != F else []) + [2, 3]


def test_survivors_mixed_and_the_hand_example(dev):
    rng = PH.rng_of(3)
    agree(dev, PH.hist(well_formed(rng, 500, 2, 4)))
    h = CT.CounterHistory.from_ops(H.hand_ops())
    agree(dev, h)
    c = CT.CheckedCounter(dev, h, 256)
    assert CT.result_map(c, c.res, 0) == {"valid?": False, "reads": H.HAND_READS, "errors": H.HAND_ERRORS} == H.restate(H.hand_ops())


# ---- 4. keys, processes and the table ---------------------------------------------------------

def test_extreme_keys_and_processes(dev):
    ids = [I64_MIN + 1, -1, 0, PH.I64_MAX - 1, PH.I64_MAX]
    rows = []
    for k in ids:
        for p in ids:
            rows += [(I, A, p, k, 1)]
    for k in ids:
        for p in ids:
            rows += [(O, A, p, k, 1)]
    want = agree(dev, PH.hist(rows))
    assert want["keys"] == ids and list(want["valid"]) == [1] * 5 and len(want["ev_kind"]) == 50


def murmur(k):
    k &= (1 << 64) - 1
    k ^= k >> 33
    k = k * 0xff51afd7ed558ccd & ((1 << 64) - 1)
    k ^= k >> 33
    k = k * 0xc4ceb9fe1a85ec53 & ((1 << 64) - 1)
    return k ^ (k >> 33)


def test_keys_that_collide_in_the_table(dev):
    """Forty keys, and as many processes, that start at two slots of the table (csrc/rows_plan.hpp's
    hash, restated), so that the claims walk over one another's slots."""
    n = 40 * 4
    slots = N.lib().lc_counter_pack_table_slots(n)
    assert slots == 512
    ids, k = [], 0
    while len(ids) < 40:
        if murmur(k) & (slots - 1) in (7, 8):
            ids.append(k)
        k += 1
    rng = PH.rng_of(4)
    rows = []
    for i in rng.sample(range(40), 40):
        rows += [(I, A, ids[i], ids[39 - i], i)]
    for i in rng.sample(range(40), 40):
        rows += [(O, A, ids[i], ids[39 - i], i), (I, R, ids[i], ids[39 - i], None), (O, R, ids[i], ids[39 - i], i)]
    want = agree(dev, PH.hist(rows))
    assert len(want["keys"]) == 40 and list(want["valid"]) == [1] * 40


def test_many_keys_in_order_of_first_appearance(dev):
    """3,000 keys x 4 rows, the keys' rows far apart, then one key per row at 5,000 rows."""
    K = 3000
    perm = PH.rng_of(5).sample(range(K), K)
    rows = [(I, A, 0, 7 * k, k) for k in perm] + [(I, R, 1, 7 * k, None) for k in range(K)]
    rows += [(O, R, 1, 7 * k, k) for k in reversed(range(K))] + [(O, A, 0, 7 * k, k) for k in perm]
    want = agree(dev, PH.hist(rows))
    assert want["keys"] == [7 * k for k in perm] and int(want["valid"].sum()) == K
    want = agree(dev, PH.hist([(I, A, 0, 100000 - r, 1) for r in range(5000)]))
    assert want["keys"] == [100000 - r for r in range(5000)] and len(want["ev_kind"]) == 5000


# ---- 5. boundaries -----------------------------------------------------------------------------

@pytest.mark.parametrize("n", [255, 256, 257, 2047, 2048, 2049])
def test_row_counts_around_the_workgroup_and_the_tiles(dev, n):
    assert launch_info()[:2] == [256, 2048]
    rng = PH.rng_of(n)
    rows = well_formed(rng, n, 2, 3, p_other=0.0)
    assert len(rows) == n
    agree(dev, PH.hist(rows), tile=256)
    agree(dev, PH.hist(rows), tile=2048)


def test_a_group_across_blocks_and_a_key_across_a_tile_edge(dev):
    # process 9 of key 1 invokes at row 0 and completes at the last row, 3,000 rows later
    filler = well_formed(PH.rng_of(6), 3000, 2, 3, p_other=0.0)
    rows = [(I, A, 9, 1, 5)] + filler + [(O, A, 9, 1, 6)]
    want = agree(dev, PH.hist(rows))
    assert int(want["ev_val"][0]) == 6
    agree(dev, PH.hist([(I, A, 9, 1, 5)] + filler + [(F, A, 9, 1, 5)]))
    # key 0: 250 events; key 1's events straddle event 256 (and its reads read 256 at tile 256)
    one = [(I, A, p, 0, 1) for p in range(250)] + [x for i in range(300) for x in ((I, R, 1, 1, None), (O, R, 1, 1, 0))]
    want = agree(dev, PH.hist(one))
    assert list(want["ev_off"]) == [0, 250, 850] and list(want["read_off"]) == [0, 0, 300]


# ---- 6. random differential -------------------------------------------------------------------

def test_random_small_histories(dev):
    rng = PH.rng_of(2024)
    bad = 0
    for _ in range(300):
        rows = PH.random_rows(rng, rng.randrange(1, 65), rng.randrange(0, 4), rng.randrange(1, 5),
                              p_wild=rng.choice((0.0, 0.0, 0.02, 0.06)))
        want = agree(dev, PH.hist(rows, keyed=rng.random() < 0.8, with_process=rng.random() < 0.9))
        bad += any(want["error"])
    assert 60 < bad < 160   # a third to a half of them hold an offence (133 by the host's count)


@pytest.mark.parametrize("seed, n_keys", [(1, 0), (2, 1), (3, 7), (4, 60), (5, 200)])
def test_random_histories_of_twenty_thousand_rows(dev, seed, n_keys):
    rng = PH.rng_of(seed)
    rows = PH.random_rows(rng, 20000, n_keys, rng.randrange(1, 9), p_wild=0.0005 if n_keys >= 60 else 0.0)
    want = agree(dev, PH.hist(rows), tile=2048 if seed % 2 else 256)
    assert len(want["read_val"]) > 1000


# ---- 7. the Python surface --------------------------------------------------------------------

def test_checker_counter_pack_device(dev):
    device, default = ck.counter({"pack": "device", "tile": 256}), ck.counter({"tile": 256})
    ops = H.hand_ops()
    assert device.check({}, ops, {}) == default.check({}, ops, {}) == {"valid?": False, "reads": H.HAND_READS, "errors": H.HAND_ERRORS}
    rng = H.rng_of(11)
    for n_keys, p_bad in ((0, 0.0), (0, 0.05), (3, 0.0), (5, 0.02)):
        ops = H.random_history(rng, 400, n_keys, p_bad=p_bad)
        assert device.check({}, ops, {}) == default.check({}, ops, {})
        a = independent.checker(device).check({}, ops, {})
        assert a == independent.checker(default).check({}, ops, {})
    ops = H.keyed([(1, H.hand_ops()), (2, [H.op("ok", "add", 0, 1)]), (3, H.hand_ops())])
    r = independent.checker(device).check({}, ops, {})
    assert r == independent.checker(default).check({}, ops, {}) and r["results"][2]["valid?"] == "unknown"


def test_refusals(dev):
    h = PH.hist([(I, A, 0, None, 1)], keyed=False)
    c, o, out = h.as_c(), N.LcCounterOpts(0, 0), C.c_void_p()
    c.n = (1 << 31) - 15
    assert N.lib().lc_counter_check_history(dev.handle, C.byref(c), C.byref(o), C.byref(out)) == -5
    c.n = 1
    assert N.lib().lc_counter_check_history(dev.handle, C.byref(c), C.byref(N.LcCounterOpts(100, 0)), C.byref(out)) == -1
    # lc_counter_checked_batch serves the context's latest check only
    first, second = CT.CheckedCounter(dev, h, 256), CT.CheckedCounter(dev, h, 256)
    with pytest.raises(N.LincheckError):
        first.arrays()
    assert list(second.arrays()["ev_kind"]) == [0]
