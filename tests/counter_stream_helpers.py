"""What the streaming counter tests share: `follow`, which appends a history
part by part and after EVERY append compares the stream with the one-shot
check of the prefix -- lc_counter_pack + lc_counter_check_host, the code the
stream was built beside -- and, for small histories, with the restatement of
tests/counter_helpers.py; the seeded random histories and their cuts; and
builders of histories that pack to an exact number of events."""
import numpy as np

import counter_helpers as H
from lincheck import counter as CT
from lincheck.counter_stream import CounterStream
from lincheck.independent import Tuple

T = 256  # the small tile


def one_shot(ops):
    """(packed, CounterResults) of ops by lc_counter_pack + lc_counter_check_host."""
    packed = CT.PackedCounter(ops if isinstance(ops, CT.CounterHistory) else CT.CounterHistory.from_ops(ops))
    return packed, CT.check_batch(None, packed.view, host=True)


def same_as_prefix(stream, ops, maps=True, what=""):
    """The stream's keys, counts() and results() equal the one-shot host check
    of ops (everything appended so far); with maps, its result maps equal the
    one-shot's and the restatement's."""
    packed, want = one_shot(ops)
    assert stream.keys() == packed.keys, (what, stream.keys(), packed.keys)
    valid, n_errors, n_reads = stream.counts()
    assert np.array_equal(valid, want.valid), (what, "valid", valid, want.valid)
    assert np.array_equal(n_errors, want.n_errors), (what, "n_errors", n_errors, want.n_errors)
    assert np.array_equal(n_reads.astype(np.int64), np.diff(packed.read_off)), (what, "n_reads", n_reads, packed.read_off)
    got = stream.results()
    for name in ("valid", "n_errors", "lower", "upper", "err_off", "err_idx"):
        assert np.array_equal(getattr(got, name), getattr(want, name)), (what, name, getattr(got, name), getattr(want, name))
    assert np.array_equal(stream.read_values(), packed.read_val()), (what, "values")
    for i in range(packed.n_keys):
        assert (stream.key_error(i) is None) == (packed.key_error(i) is None), (what, i)
    if maps:
        shown = H.restate_independent(ops if isinstance(ops, list) else ops.to_ops())
        mine = stream.result_maps()
        assert list(mine) == list(shown), (what, list(mine), list(shown))
        for i, k in enumerate(packed.keys):
            assert H.same(mine[k], shown[k]), (what, k, mine[k], shown[k])
            theirs = CT.result_map(packed, want, i)
            assert stream.result_map(i) == mine[k]
            assert H.same(mine[k], theirs) and (theirs["valid?"] == "unknown" or mine[k] == theirs), (what, k, mine[k], theirs)
    return packed, want


def follow(dev, parts, opts=None, maps=True, check=None):
    """Append parts one by one to a stream on dev (None: the host stream) and
    compare after every append.  Returns per append (update, {key: valid} of
    the prefix).  check(j, update, stream) runs after append j's comparison."""
    so_far, before, out = [], {}, []
    with CounterStream(dev, opts) as s:
        for j, part in enumerate(parts):
            u = s.append(part)
            so_far = so_far + list(part)
            packed, want = same_as_prefix(s, so_far, maps, what=j)
            assert (u.rows, u.n_keys) == (len(so_far), packed.n_keys), (j, u)
            keys = s.keys()
            # changed: exactly the keys whose valid differs (a key first seen counts as valid before)
            assert u.changed == [i for i, k in enumerate(keys) if int(want.valid[i]) != before.get(k, 1)], (j, u.changed)
            before = {k: int(want.valid[i]) for i, k in enumerate(keys)}
            if check:
                check(j, u, s)
            out.append((u, dict(before)))
    return out


def cut(rng, ops, n_cuts):
    cuts = sorted(rng.randint(0, len(ops)) for _ in range(n_cuts))
    return [ops[a:b] for a, b in zip([0] + cuts, cuts + [len(ops)])]


def random_case(seed, p_bad):
    """random_history(rng, 600, n_keys=3, p_bad) cut at 12 random places."""
    rng = H.rng_of(seed)
    ops = H.random_history(rng, 600, n_keys=3, p_bad=p_bad)
    return cut(rng, ops, 12)


def transitions(parts):
    """Per append the {key: valid} of the prefix by the one-shot check, and the
    number of :fail :add rows whose invocation lies in an earlier append."""
    so_far, seen, late_fails, open_ = [], [], 0, {}
    for j, part in enumerate(parts):
        for o in part:
            if o.get("f") != "add" or not H.is_int(o.get("process")):
                continue
            v = o["value"]
            who = (v[0] if hasattr(v, "__len__") and not isinstance(v, str) else None, o["process"])
            if o["type"] == "invoke":
                open_[who] = j
            else:
                at = open_.pop(who, None)
                late_fails += o["type"] == "fail" and at is not None and at < j
        so_far = so_far + part
        packed, want = one_shot(so_far)
        seen.append({k: int(want.valid[i]) for i, k in enumerate(packed.keys)})
    return seen, late_fails


def events_exactly(n, proc=0, read_every=3):
    """Ops of one key that pack to exactly n events, reads among them: :ok adds
    (2 events), :ok reads (2), and an :info add (1) when n is odd.  A read
    returns the acknowledged sum, which is in bounds."""
    out, lower, left, i = [], 0, n, 0
    if left % 2:
        out += [H.op("invoke", "add", proc + 50, 2), H.op("info", "add", proc + 50, 2)]
        left -= 1
    while left:
        if i % read_every == 0:
            out += [H.op("invoke", "read", proc), H.op("ok", "read", proc, lower if i % 5 else lower + 1000)]
        else:
            out += [H.op("invoke", "add", proc, 1 + i % 4), H.op("ok", "add", proc, 1 + i % 4)]
            lower += 1 + i % 4
        left -= 2
        i += 1
    return out


# ---- hand-built cases: name -> the appends ----------------------------------------------------

def kop(k, type_, f, process, value=None):
    """An op of key k (a tuple value)."""
    return H.op(type_, f, process, Tuple(k, value))


def rows(ops):
    """One append per row."""
    return [[o] for o in ops]


def hand_variant():
    """The hand example with a read completed between `invoke add 0 4` and its :fail."""
    ops = H.hand_ops()
    at = next(i for i, o in enumerate(ops) if o["type"] == "fail" and o["f"] == "add")
    return ops[:at] + [H.op("invoke", "read", 7), H.op("ok", "read", 7, 6)] + ops[at:]


def permanent(kind):
    """Key 1 stays live beside key 2, which `kind` breaks for good in the third
    append; both get rows, reads among them, afterwards."""
    a = [kop(1, "invoke", "add", 0, 2), kop(2, "invoke", "add", 0, 3), kop(2, "invoke", "read", 1), kop(2, "ok", "read", 1, 1),
         kop(1, "ok", "add", 0, 2)]
    b = [kop(2, "invoke", "read", 1), kop(1, "invoke", "read", 1)]
    bad = {"orphan": [kop(2, "ok", "add", 9, 1)],
           "double-invoke": [kop(2, "invoke", "read", 1)],
           "other-f": [kop(2, "ok", "add", 1, 1)],
           "ok-add-nil": [kop(2, "ok", "add", 0, None)],
           "ok-add-negative": [kop(2, "ok", "add", 0, -1)],
           "ok-read-nil": [kop(2, "ok", "read", 1, None)]}[kind]
    c = bad + [kop(1, "ok", "read", 1, 2)]
    d = [kop(2, "invoke", "read", 5), kop(2, "ok", "read", 5, 0), kop(2, "fail", "add", 0, 3), kop(1, "invoke", "read", 1),
         kop(1, "ok", "read", 1, 9)]
    return [a, b, c, d]


PERMANENT = ("orphan", "double-invoke", "other-f", "ok-add-nil", "ok-add-negative", "ok-read-nil")


def hand_cases():
    op, M = H.op, H.I64_MAX
    cases = {
        "hand": rows(H.hand_ops()),
        "hand-read-before-the-fail": rows(hand_variant()),
        # a read above `upper`, then an :ok :add whose value exceeds its invocation's
        "invalid-to-valid": rows([op("invoke", "add", 0, 1), op("invoke", "read", 1), op("ok", "read", 1, 5), op("ok", "add", 0, 7),
                                  op("invoke", "read", 1), op("ok", "read", 1, 7)]),
        "valid-to-invalid-by-a-fail": rows([op("invoke", "add", 0, 5), op("invoke", "read", 1), op("ok", "read", 1, 3),
                                            op("fail", "add", 0, 5), op("invoke", "read", 1), op("ok", "read", 1, 0)]),
        "unknown-and-back-nil-ok-3": rows([op("invoke", "add", 0, None), op("invoke", "read", 1), op("ok", "read", 1, 2),
                                           op("invoke", "read", 1), op("ok", "add", 0, 3), op("ok", "read", 1, 9)]),
        "unknown-and-back-negative-fail": rows([op("invoke", "add", 0, -2), op("invoke", "add", 2, 4), op("invoke", "read", 1),
                                                op("ok", "read", 1, 1), op("fail", "add", 0, -2), op("ok", "add", 2, 4)]),
        # three adds that pass 2^64 between them; the reads taken meanwhile come back with the right bounds
        "unknown-and-back-sum": rows([op("invoke", "add", 2, 5), op("invoke", "add", 0, M), op("invoke", "read", 1),
                                      op("ok", "read", 1, 3), op("invoke", "add", 3, M), op("invoke", "add", 4, M),
                                      op("invoke", "read", 1), op("ok", "read", 1, 6), op("fail", "add", 3, M),
                                      op("fail", "add", 0, M), op("fail", "add", 4, M), op("ok", "add", 2, 5)]),
        # a read invoked two appends before its :ok; its slot reused afterwards, beside a read that stays open
        "a-read-across-appends": [[op("invoke", "read", 1)], [op("invoke", "add", 0, 2), op("ok", "add", 0, 2), op("invoke", "read", 2)],
                                  [op("ok", "read", 1, 1), op("invoke", "add", 0, 3)],
                                  [op("invoke", "read", 1), op("ok", "add", 0, 3), op("invoke", "read", 3), op("ok", "read", 1, 2),
                                   op("ok", "read", 3, 5)],
                                  [op("ok", "read", 2, 4), op("invoke", "read", 1), op("fail", "read", 1), op("invoke", "read", 1),
                                   op("ok", "read", 1, 5)]],
        "a-key-appears-late": [[kop(4, "invoke", "add", 0, 1), kop(4, "ok", "add", 0, 1)], [kop(4, "invoke", "read", 0)],
                               [kop(9, "invoke", "read", 0), kop(4, "ok", "read", 0, 1), kop(9, "ok", "read", 0, 3)],
                               [kop(9, "invoke", "add", 1, 3), kop(2, "invoke", "add", 1, None)], [kop(2, "fail", "add", 1, None)]],
        "empty-appends": [[], [{"type": "info", "f": "start", "process": "nemesis", "value": None}], [], [op("invoke", "add", 0, 1)],
                          [], [op("invoke", "read", 1), op("ok", "read", 1, 2)], [], [op("fail", "add", 0, 1)], []],
    }
    for kind in PERMANENT:
        cases["permanent-" + kind] = permanent(kind)
    return cases
