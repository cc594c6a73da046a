"""What the streaming total-queue / unique-ids tests share: the comparison of
a stream with the one-shot check of the prefix appended so far, the seeded
random histories and their cuts, and the table's hash restated (so that a test
can choose values by their home slot)."""
import numpy as np

import queue_helpers as H
from lincheck import _native as N
from lincheck import queue as Q

TQ, IDS = N.LC_QM_TOTAL_QUEUE, N.LC_QM_UNIQUE_IDS
M64 = (1 << 64) - 1
ARRAYS = ("valid", "counts", "has_range", "ent_key", "ent_class", "ent_val", "ent_mult")


def one_shot(ops, mode):
    """lc_queue_pack + lc_queue_check_host of ops (op maps or a QueueHistory): (packed, QueueResults)."""
    packed = Q.PackedQueue(ops if isinstance(ops, Q.QueueHistory) else Q.QueueHistory.from_ops(ops), mode)
    return packed, Q.check_batch(None, packed.view, host=True)


def same_as_prefix(stream, ops, mode, maps=True, what=""):
    """The stream's keys, counts(), results() and, with maps, result maps
    equal the one-shot host check of ops (everything appended so far) and the
    restatements of tests/queue_helpers.py."""
    packed, want = one_shot(ops, mode)
    assert stream.keys() == packed.keys, (what, stream.keys(), packed.keys)
    valid, counts, lo, hi, has = stream.counts()
    got = stream.results()
    for name, cheap in (("valid", valid), ("counts", counts), ("has_range", has)):
        assert np.array_equal(cheap, getattr(want, name)), (what, "counts()", name, cheap, getattr(want, name))
    for name in ARRAYS:
        assert np.array_equal(getattr(got, name), getattr(want, name)), (what, name, getattr(got, name), getattr(want, name))
    r = want.has_range.astype(bool)
    for mine in ((lo, hi), (got.lo, got.hi)):
        assert np.array_equal(mine[0][r], want.lo[r]) and np.array_equal(mine[1][r], want.hi[r]), (what, "range")
    for i in range(len(packed.keys)):
        assert stream.key_error(i) == packed.key_error(i), (what, i)
    if maps:
        exp, shown_all = H.expected_arrays(ops, mode)
        H.assert_results(got, exp, what)
        shown = H.restate_independent(ops, H.RESTATE[mode][0])
        assert stream.result_maps() == shown, what
        for i, k in enumerate(packed.keys):
            assert stream.result_map(i) == Q.result_map(packed, want, i) == shown[k], (what, k)
    return want


def same_update(a, b, what=""):
    """Two streams' updates of the same append agree field for field."""
    assert a == b, (what, a, b)


def random_case(seed):
    """A seeded history (at most 2,000 rows, 3 keys or none, 40 values, drains,
    a crashed one in every fourth) and its cut into at most 12 appends, an
    empty one and one of ignored rows only among them."""
    rng = H.rng_of(9000 + seed)
    n = rng.randint(200, 2000) if seed % 5 else rng.randint(0, 60)
    ops = H.random_history(rng, n, n_keys=3 if seed % 3 else 0, domain=40, p_crash=0.02 if seed % 4 == 0 else 0.0)
    cuts = sorted(rng.randint(0, len(ops)) for _ in range(rng.randint(1, 9)))
    parts = [ops[a:b] for a, b in zip([0] + cuts, cuts + [len(ops)])]
    keyed = seed % 3 != 0
    ignored = [H.op("fail", "enqueue", 1, 4 if keyed else None), H.op("invoke", "dequeue", None, 4 if keyed else None),
               {"type": "info", "f": "start", "value": "x", "process": "nemesis"}]
    at = rng.randint(1, len(parts))  # (not first: the first append of a keyed history must show its keys)
    parts[at:at] = [[], ignored]
    assert len(parts) <= 12
    return parts


def slot_hash(key, val):
    """csrc/device_queue_stream.hpp's mixer: the home slot of (key id, value) is this & (slots - 1)."""
    x = ((val & M64) ^ (key * 0x9E3779B97F4A7C15)) & M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return (x ^ (x >> 32)) & 0xFFFFFFFF


def plan_must_grow(slots, resident, rows):
    return slots < resident + rows or slots < 2 * resident


def plan_grown(resident, rows):
    p = 1
    while p < 2 * (resident + rows):
        p <<= 1
    return p
