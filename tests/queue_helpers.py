"""checker/total-queue's and checker/unique-ids' rules written twice,
independently of the library and of each other (the tests' oracle; parity with
Jepsen unpinned), random history generators, and the comparison of a
QueueResults with what the restatements say.

    restate_queue / restate_ids          collections.Counter as Clojure's
                                         multiset, following the checkers'
                                         source step by step: drain expansion,
                                         multiset intersect and minus
    restate_queue_np / restate_ids_np    the per-value formulas of
                                         include/lincheck_queue.h over one sort
"""
import random
from collections import Counter

import numpy as np

from lincheck import _native as N
from lincheck import independent

I64_MAX = 2**63 - 1
I64_MIN = -2**63
QUEUE_FS = ("enqueue", "dequeue", "drain", "generate")
CRASHED_DRAIN = "Not sure how to handle a crashed drain operation"
COUNT_NAMES = ("attempt-count", "acknowledged-count", "ok-count", "unexpected-count", "duplicated-count", "lost-count",
               "recovered-count")
CLASS_NAMES = ("lost", "unexpected", "duplicated", "recovered")


def op(type_, f, value=None, key=None, process=0):
    return {"type": type_, "f": f, "value": value if key is None else independent.tuple(key, value), "process": process}


def rng_of(seed):
    return random.Random(seed)


def nil_first(v):
    """Sort key: nil orders below every integer."""
    return (v is not None, v or 0)


# ---- the split by key -------------------------------------------------------------

def split(ops):
    """{key: sub-history}, keys in order of first appearance among the rows
    with a queue :f; {None: ops} when no such row has a tuple; rows without a
    key among rows with keys are ignored."""
    keyed = [o for o in ops if o["f"] in QUEUE_FS and independent.is_tuple(o["value"])]
    if not keyed:
        return {None: list(ops)}
    out = {}
    for o in keyed:
        out.setdefault(o["value"][0], []).append(dict(o, value=o["value"][1]))
    return out


def restate_independent(ops, fn, **kw):
    return {k: fn(sub, **kw) for k, sub in split(ops).items()}


# ---- total-queue, first: multisets --------------------------------------------------

class CrashedDrain(Exception):
    pass


def expand_queue_drain_ops(history):
    """jepsen.checker/expand-queue-drain-ops."""
    out = []
    for o in history:
        if o["f"] != "drain":
            out.append(o)
        elif o["type"] in ("invoke", "fail"):
            continue
        elif o["type"] == "ok":
            out.extend(dict(o, f="dequeue", value=v) for v in (o["value"] or []))
        else:
            raise CrashedDrain(CRASHED_DRAIN)
    return out


def restate_queue(history):
    try:
        history = expand_queue_drain_ops(history)
    except CrashedDrain as e:  # check-safe
        return {"valid?": "unknown", "error": str(e)}
    attempts = Counter(o["value"] for o in history if o["type"] == "invoke" and o["f"] == "enqueue")
    enqueues = Counter(o["value"] for o in history if o["type"] == "ok" and o["f"] == "enqueue")
    dequeues = Counter(o["value"] for o in history if o["type"] == "ok" and o["f"] == "dequeue")
    ok = dequeues & attempts                                                   # multiset/intersect
    unexpected = Counter({v: n for v, n in dequeues.items() if v not in attempts})
    duplicated = (dequeues - attempts) - unexpected                            # multiset/minus, twice
    lost = enqueues - dequeues
    recovered = ok - enqueues

    def seq(ms):
        return sorted(ms.elements(), key=nil_first)

    return {"valid?": not lost and not unexpected,
            "attempt-count": sum(attempts.values()), "acknowledged-count": sum(enqueues.values()),
            "ok-count": sum(ok.values()), "unexpected-count": sum(unexpected.values()),
            "duplicated-count": sum(duplicated.values()), "lost-count": sum(lost.values()),
            "recovered-count": sum(recovered.values()),
            "lost": seq(lost), "unexpected": seq(unexpected), "duplicated": seq(duplicated), "recovered": seq(recovered)}


# ---- total-queue, second: the formulas over a sort -----------------------------------

def _code(v):
    return I64_MIN if v is None else v


def _decode(v):
    return None if v == I64_MIN else int(v)


def restate_queue_np(history):
    vals, kinds = [], []
    for o in history:
        t, f = o["type"], o["f"]
        if f == "drain":
            if t == "info":
                return {"valid?": "unknown", "error": CRASHED_DRAIN}
            if t == "ok":
                for v in o["value"] or []:
                    vals.append(_code(v)); kinds.append(2)
        elif f == "enqueue" and t in ("invoke", "ok"):
            vals.append(_code(o["value"])); kinds.append(0 if t == "invoke" else 1)
        elif f == "dequeue" and t == "ok":
            vals.append(_code(o["value"])); kinds.append(2)
    vals, kinds = np.array(vals, dtype=object), np.array(kinds, np.int64)
    order = sorted(range(len(vals)), key=lambda i: vals[i])
    rows = {c: [] for c in CLASS_NAMES}
    tot = dict.fromkeys(COUNT_NAMES, 0)
    i = 0
    while i < len(order):
        j = i
        while j < len(order) and vals[order[j]] == vals[order[i]]:
            j += 1
        ks = kinds[order[i:j]]
        a, e, d = int((ks == 0).sum()), int((ks == 1).sum()), int((ks == 2).sum())
        m = {"ok": min(d, a), "unexpected": d if a == 0 else 0, "duplicated": max(d - a, 0) if a > 0 else 0,
             "lost": max(e - d, 0)}
        m["recovered"] = max(m["ok"] - e, 0)
        tot["attempt-count"] += a
        tot["acknowledged-count"] += e
        for c in ("ok",) + CLASS_NAMES:
            tot[c + "-count"] += m[c]
        for c in CLASS_NAMES:
            rows[c] += [_decode(vals[order[i]])] * m[c]   # ascending: the sort's order, nil (INT64_MIN) first
        i = j
    out = {"valid?": tot["lost-count"] == 0 and tot["unexpected-count"] == 0}
    out.update(tot)
    out.update(rows)
    return out


# ---- unique-ids ----------------------------------------------------------------------

def restate_ids(history, top=48):
    attempted = sum(1 for o in history if o["type"] == "invoke" and o["f"] == "generate")
    acks = [o["value"] for o in history if o["type"] == "ok" and o["f"] == "generate"]
    seen = Counter()
    for v in acks:
        seen[v] += 1
    dups = {v: n for v, n in seen.items() if n > 1}
    # (->> dups (sort-by val) reverse (take 48) (into (sorted-map))): the sort is stable over the sorted map's order
    by_count = sorted(sorted(dups.items(), key=lambda kv: nil_first(kv[0])), key=lambda kv: kv[1])[::-1]
    shown = dict(sorted(by_count[:top], key=lambda kv: nil_first(kv[0])))
    lo = hi = acks[0] if acks else None
    for x in acks:
        if nil_first(x) < nil_first(lo):
            lo = x
        if nil_first(x) > nil_first(hi):
            hi = x
    return {"valid?": not dups, "attempted-count": attempted, "acknowledged-count": len(acks), "duplicated-count": len(dups),
            "duplicated": shown, "range": [lo, hi]}


def restate_ids_np(history, top=48):
    inv = sum(o["f"] == "generate" and o["type"] == "invoke" for o in history)
    acks = sorted(_code(o["value"]) for o in history if o["f"] == "generate" and o["type"] == "ok")
    pairs = []  # (count, value) of every value acknowledged more than once
    i = 0
    while i < len(acks):
        j = i
        while j < len(acks) and acks[j] == acks[i]:
            j += 1
        if j - i > 1:
            pairs.append((j - i, acks[i]))
        i = j
    keep = sorted(pairs, reverse=True)[:None if top is None else top]  # highest counts, ties towards the larger value
    shown = {_decode(v): n for n, v in sorted(keep, key=lambda p: p[1])}
    return {"valid?": not pairs, "attempted-count": int(inv), "acknowledged-count": len(acks), "duplicated-count": len(pairs),
            "duplicated": shown, "range": [_decode(acks[0]), _decode(acks[-1])] if acks else [None, None]}


RESTATE = {N.LC_QM_TOTAL_QUEUE: (restate_queue, restate_queue_np), N.LC_QM_UNIQUE_IDS: (restate_ids, restate_ids_np)}


# ---- what the C ABI's arrays must hold ------------------------------------------------

def expected_arrays(ops, mode):
    """valid, counts, lo / hi / has_range and the sorted entries of every key,
    from the first restatement (unique-ids: every duplicate, not only 48)."""
    first = RESTATE[mode][0]
    maps = restate_independent(ops, first, **({"top": None} if mode == N.LC_QM_UNIQUE_IDS else {}))
    K = len(maps)
    valid, counts = np.zeros(K, np.int8), np.zeros((K, 7), np.uint64)
    lo, hi, has = np.zeros(K, np.int64), np.zeros(K, np.int64), np.zeros(K, np.uint8)
    ents = []
    for i, m in enumerate(maps.values()):
        if m["valid?"] == "unknown":
            valid[i] = -1
            continue
        valid[i] = 1 if m["valid?"] else 0
        if mode == N.LC_QM_UNIQUE_IDS:
            counts[i, :3] = [m["attempted-count"], m["acknowledged-count"], m["duplicated-count"]]
            if m["acknowledged-count"]:
                has[i], lo[i], hi[i] = 1, _code(m["range"][0]), _code(m["range"][1])
            ents += [(i, N.LC_QC_DUPLICATED, _code(v), n) for v, n in m["duplicated"].items()]
        else:
            counts[i] = [m[c] for c in COUNT_NAMES]
            for code, name in enumerate(CLASS_NAMES):
                ents += [(i, code, _code(v), n) for v, n in Counter(m[name]).items()]
    ents.sort()
    col = lambda j, dt: np.array([e[j] for e in ents], dt)  # noqa: E731
    return dict(valid=valid, counts=counts, lo=lo, hi=hi, has_range=has, ent_key=col(0, np.uint32),
                ent_class=col(1, np.uint8), ent_val=col(2, np.int64), ent_mult=col(3, np.uint64)), maps


def assert_results(res, exp, what=""):
    """Every output field of a QueueResults against expected_arrays'."""
    for name in ("valid", "counts", "has_range", "ent_key", "ent_class", "ent_val", "ent_mult"):
        assert np.array_equal(getattr(res, name), exp[name]), (what, name, getattr(res, name), exp[name])
    has = exp["has_range"].astype(bool)
    assert np.array_equal(res.lo[has], exp["lo"][has]) and np.array_equal(res.hi[has], exp["hi"][has]), (what, "range")


def same_results(a, b):
    for name in ("valid", "counts", "has_range", "ent_key", "ent_class", "ent_val", "ent_mult"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    has = a.has_range.astype(bool)
    assert np.array_equal(a.lo[has], b.lo[has]) and np.array_equal(a.hi[has], b.hi[has])


# ---- generators --------------------------------------------------------------------------

def random_history(rng, n, n_keys=0, domain=4, p_nil=0.08, p_crash=0.0, p_nemesis=0.05):
    """n rows over `domain` values (and nil), so that every class occurs:
    enqueues and dequeues of every :type, drains (an :ok drain with 0-3
    elements), :generate rows and nemesis rows; n_keys 0: no tuples."""
    def val():
        return None if rng.random() < p_nil else rng.randint(1, domain)

    ops = []
    for _ in range(n):
        key = rng.randrange(n_keys) * 7 - 3 if n_keys else None
        u = rng.random()
        if u < p_nemesis:
            ops.append({"type": "info", "f": rng.choice(["start", "stop"]), "value": rng.choice([None, "x", [1, 2]]),
                        "process": "nemesis"})
        elif u < 0.45:
            ops.append(op(rng.choice(["invoke", "invoke", "ok", "ok", "fail", "info"]), "enqueue", val(), key))
        elif u < 0.70:
            t = rng.choice(["invoke", "ok", "ok", "ok", "fail"])
            ops.append(op(t, "dequeue", val() if t == "ok" else None, key))
        elif u < 0.80:
            t = "info" if rng.random() < p_crash else rng.choice(["invoke", "ok", "ok", "fail"])
            ops.append(op(t, "drain", [val() for _ in range(rng.randint(0, 3))] if t == "ok" else None, key))
        else:
            t = rng.choice(["invoke", "ok", "ok", "ok", "fail", "info"])
            ops.append(op(t, "generate", val() if t == "ok" else None, key))
    return ops


HAND_QUEUE = [
    op("invoke", "enqueue", 1), op("ok", "enqueue", 1),        # 1: enqueued, dequeued twice: ok and duplicated
    op("invoke", "enqueue", 2), op("ok", "enqueue", 2),        # 2: acknowledged and never seen again: lost
    op("invoke", "enqueue", 3), op("info", "enqueue", 3),      # 3: never acknowledged, drained: recovered
    op("invoke", "enqueue", 4), op("fail", "enqueue", 4),      # 4: attempted only: nothing
    op("invoke", "dequeue"), op("ok", "dequeue", 1),
    op("invoke", "dequeue"), op("ok", "dequeue", 1),
    op("invoke", "dequeue"), op("fail", "dequeue"),
    {"type": "info", "f": "start", "value": "partition", "process": "nemesis"},
    op("invoke", "drain"), op("ok", "drain", [3, 9, None]),   # 9 and nil: never attempted: unexpected
]
HAND_QUEUE_RESULT = {"valid?": False, "attempt-count": 4, "acknowledged-count": 2, "ok-count": 2, "unexpected-count": 2,
                     "duplicated-count": 1, "lost-count": 1, "recovered-count": 1, "lost": [2], "unexpected": [None, 9],
                     "duplicated": [1], "recovered": [3]}


# ---- EDN ----------------------------------------------------------------------------------

def _edn(v):
    if v is None:
        return "nil"
    if independent.is_tuple(v):
        return f"[{_edn(v[0])} {_edn(v[1])}]"
    if isinstance(v, (list, tuple)):
        return "[" + " ".join(_edn(x) for x in v) + "]"
    if isinstance(v, str):
        return '"' + v + '"'
    return str(v)


def write_edn(ops):
    """The ops as a history.edn, one op map per line."""
    lines = []
    for i, o in enumerate(ops):
        proc = ":nemesis" if o.get("process") == "nemesis" else _edn(o.get("process", 0))
        lines.append(f"{{:type :{o['type']}, :f :{o['f']}, :value {_edn(o['value'])}, :process {proc}, :time {i * 1000}, :index {i}}}")
    return "\n".join(lines) + "\n"
