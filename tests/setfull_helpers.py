"""Helpers of the set-full tests.  Jepsen itself is not available, so parity
is unpinned; the oracle is the rule set of include/lincheck.h
written twice:

  restate           the fold, literally: elements / reads / dups updated op by
                    op in history order, every tracked element at every read;
  restate_matrix    independently, from the per-element definitions: a numpy
                    presence matrix (reads x elements), the eligibility suffix
                    (reads completed after the element's last invocation) and
                    arg-max over invocation positions.  Serves larger shapes.

Both return (result map, {element: (outcome, latency, known position,
last-absent position)}).  Also here: the hand example of the issue, a random
history generator and an EDN writer with real :process and :time."""
import random
from collections import Counter

import numpy as np

from lincheck.independent import Tuple, is_tuple
from set_helpers import edn_value, is_int, keys_of

I64_MAX = (1 << 63) - 1
QUANTILES = (0, 0.5, 0.95, 0.99, 1)
COLLECTIONS = (set, frozenset, list, tuple)


class FoldError(Exception):
    pass


def with_pos(ops):
    """Copies of the ops with "pos" = the row number in the history."""
    return [dict(op, pos=i) for i, op in enumerate(ops)]


def sub(ops, k):
    """Key k's rows of with_pos(ops), unwrapped."""
    return [dict(op, value=op["value"][1]) for op in ops if is_tuple(op.get("value")) and op["value"][0] == k]


def render(op):
    """An op of the fold as lincheck.setfull renders a row."""
    if op is None:
        return None
    v = op.get("value")
    if isinstance(v, COLLECTIONS):
        v = list(v)
    p = op.get("process")
    return {"type": op["type"], "f": op["f"], "value": v, "process": p if is_int(p) else "nemesis",
            "time": op.get("time", 0), "index": op.get("index", op["pos"])}


def fold(ops):
    """The fold: (elements, dups).  Raises FoldError where check-safe would
    have caught an exception."""
    elements, reads, dups = {}, {}, {}
    for op in ops:
        p = op.get("process")
        if not is_int(p):
            continue
        t, f, v = op["type"], op["f"], op.get("value")
        if f == "add":
            if t == "invoke":
                if not is_int(v):
                    raise FoldError("a set element is nil or not an integer")
                elements[v] = {"known": None, "last-present": None, "last-absent": None}
            elif t == "ok":
                if not is_int(v):
                    raise FoldError("a set element is nil or not an integer")
                if v not in elements:
                    raise FoldError("an :ok :add of an element with no earlier :invoke :add")
                elements[v]["known"] = elements[v]["known"] or op
        elif f == "read":
            if t == "invoke":
                reads[p] = op
            elif t == "fail":
                reads.pop(p, None)
            elif t == "ok":
                if p not in reads:
                    raise FoldError("an :ok :read by a process with no open :read invocation")
                if v is not None and not isinstance(v, COLLECTIONS):
                    raise FoldError("a :read value is no collection")
                vals = [] if v is None else list(v)
                if not all(is_int(x) for x in vals):
                    raise FoldError("a :read value holds nil or a non-integer")
                inv = reads[p]
                for x, c in Counter(vals).items():
                    if c > 1:
                        dups[x] = max(dups.get(x, 0), c)
                held = set(vals)
                for el, e in elements.items():
                    if el in held:
                        e["known"] = e["known"] or op
                        which = "last-present"
                    else:
                        which = "last-absent"
                    if e[which] is None or e[which]["pos"] < inv["pos"]:
                        e[which] = inv
    return elements, dups


def idx(op):
    return -1 if op is None else op["pos"]


def classify(e):
    """(outcome, latency ms or -1) of one element record."""
    known, lp, la = e["known"], e["last-present"], e["last-absent"]
    stable = lp is not None and idx(la) < idx(lp)
    lost = known is not None and la is not None and idx(lp) < idx(la) and idx(known) < idx(la)
    if stable:
        until = la["time"] + 1 if la is not None else 0
        return "stable", max(0, until - known["time"]) // 10 ** 6
    if lost:
        until = lp["time"] + 1 if lp is not None else 0
        return "lost", max(0, until - known["time"]) // 10 ** 6
    return "never-read", -1


def quantile_map(lat):
    s = sorted(lat)
    n = len(s)
    return {q: s[min(n - 1, int(n * q // 1))] for q in QUANTILES}


def shape(per, dups, known_op, la_op, linearizable):
    """The result map from {element: (outcome, latency, known pos, last-absent
    pos)}, the duplicates and functions from an element to its rendered ops."""
    stable = sorted(e for e, r in per.items() if r[0] == "stable")
    lost = sorted(e for e, r in per.items() if r[0] == "lost")
    never = sorted(e for e, r in per.items() if r[0] == "never-read")
    stale = [e for e in stable if per[e][1] > 0]
    valid = False if lost else "unknown" if not stable else False if linearizable and stale else True
    if dups:
        valid = False
    out = {"valid?": valid, "attempt-count": len(per), "stable-count": len(stable), "lost-count": len(lost),
           "never-read-count": len(never), "stale-count": len(stale), "duplicated-count": len(dups),
           "lost": lost, "never-read": never, "stale": stale, "duplicated": dict(sorted(dups.items())),
           "worst-stale": [{"element": e, "outcome": "stable", "stable-latency": per[e][1], "lost-latency": None,
                            "known": known_op(e), "last-absent": la_op(e)}
                           for e in sorted(stale, key=lambda e: (-per[e][1], e))[:8]]}
    if stable:
        out["stable-latencies"] = quantile_map([per[e][1] for e in stable])
    if lost:
        out["lost-latencies"] = quantile_map([per[e][1] for e in lost])
    return out


def restate(ops, linearizable=False):
    """jepsen.checker/set-full over one key's (unwrapped) ops carrying "pos"."""
    try:
        elements, dups = fold(ops)
    except FoldError as err:
        return {"valid?": "unknown", "error": str(err)}, {}
    per = {}
    for el, e in elements.items():
        outcome, lat = classify(e)
        per[el] = (outcome, lat, idx(e["known"]), idx(e["last-absent"]))
    return shape(per, dups, lambda el: render(elements[el]["known"]), lambda el: render(elements[el]["last-absent"]),
                 linearizable), per


def restate_matrix(ops, linearizable=False):
    """The same from the per-element definitions (checked keys only: the fold
    decides what is an error)."""
    ops = [op for op in ops if is_int(op.get("process"))]
    by_pos = {op["pos"]: op for op in ops}
    last_inv = {}
    for op in ops:
        if op["f"] == "add" and op["type"] == "invoke":
            last_inv[op["value"]] = op["pos"]
    els = sorted(last_inv)
    col = {e: j for j, e in enumerate(els)}
    inv_at = np.array([last_inv[e] for e in els], np.int64)
    ack = np.full(len(els), -1, np.int64)
    for op in ops:
        if op["f"] == "add" and op["type"] == "ok":
            j = col[op["value"]]
            if op["pos"] > inv_at[j] and ack[j] < 0:
                ack[j] = op["pos"]
    open_read, rows, dups = {}, [], {}
    for op in ops:
        if op["f"] != "read":
            continue
        if op["type"] == "invoke":
            open_read[op["process"]] = op["pos"]
        elif op["type"] == "fail":
            open_read.pop(op["process"], None)
        elif op["type"] == "ok":
            rows.append((op["pos"], open_read[op["process"]], list(op["value"] or [])))
    n_r = len(rows)
    done = np.array([r[0] for r in rows], np.int64).reshape(n_r, 1)
    invoked = np.array([r[1] for r in rows], np.int64).reshape(n_r, 1)
    m = np.zeros((n_r, len(els)), bool)
    for i, (_, _, vals) in enumerate(rows):
        for x, c in Counter(vals).items():
            if c > 1:
                dups[x] = max(dups.get(x, 0), c)
            if x in col:
                m[i, col[x]] = True
    eligible = done > inv_at.reshape(1, -1)
    lp = np.where(eligible & m, invoked, -1).max(axis=0, initial=-1)
    la = np.where(eligible & ~m, invoked, -1).max(axis=0, initial=-1)
    first = np.full(len(els), -1, np.int64)
    if n_r and els:
        seen = eligible & m
        first = np.where(seen.any(axis=0), done[:, 0][seen.argmax(axis=0)], -1)
    known = np.where(first < 0, ack, np.where(ack < 0, first, np.minimum(first, ack)))
    per = {}
    for j, e in enumerate(els):
        k, p, a = int(known[j]), int(lp[j]), int(la[j])
        if p >= 0 and a < p:
            until = by_pos[a]["time"] + 1 if a >= 0 else 0
            per[e] = ("stable", max(0, until - by_pos[k]["time"]) // 10 ** 6, k, a)
        elif k >= 0 and a >= 0 and p < a and k < a:
            until = by_pos[p]["time"] + 1 if p >= 0 else 0
            per[e] = ("lost", max(0, until - by_pos[k]["time"]) // 10 ** 6, k, a)
        else:
            per[e] = ("never-read", -1, k, a)
    at = lambda pos: render(by_pos[pos]) if pos >= 0 else None  # noqa: E731
    return shape(per, dups, lambda e: at(per[e][2]), lambda e: at(per[e][3]), linearizable), per


def restate_independent(ops, linearizable=False, how=restate):
    """{key: (result map, per element)}; a history without tuples is one key, None."""
    ops = with_pos(ops)
    keys = keys_of(ops)
    if not keys:
        return {None: how(ops, linearizable)}
    return {k: how(sub(ops, k), linearizable) for k in keys}


def norm(result):
    """A result map with the read values inside its rendered ops sorted (a
    set's iteration order is no part of the result)."""
    def fix(op):
        if op and isinstance(op.get("value"), list):
            return dict(op, value=sorted(op["value"], key=lambda x: (x is None, x)))
        return op
    if "worst-stale" not in result:
        return result
    return dict(result, **{"worst-stale": [dict(w, known=fix(w["known"]), **{"last-absent": fix(w["last-absent"])})
                                           for w in result["worst-stale"]]})


def same(got, want):
    """Result maps agree: in full, or for a key that is not checked in
    :valid? and in having an :error."""
    if "error" in want:
        return got.get("valid?") == "unknown" and "error" in got
    return norm(got) == norm(want)


def per_element(packed, res, i):
    """What the device said of key i's tracked ids, as the oracles' second value."""
    from lincheck import _native as N
    from lincheck.setfull import OUTCOMES, elements_of
    arrs = packed.arrays()
    b, n = int(arrs["id_off"][i]), int(arrs["span"][i])
    ids = [x for x in range(n) if res.outcome[b + x] != N.LC_SETFULL_UNTRACKED]
    return {e: (OUTCOMES[int(res.outcome[b + x])], int(res.latency[b + x]), int(res.known[b + x]), int(res.last_absent[b + x]))
            for x, e in zip(ids, elements_of(arrs, i, ids))}


def op(t, f, v, p, time_ms):
    return {"type": t, "f": f, "value": v, "process": p, "time": time_ms * 10 ** 6}


def hand_ops():
    """The hand-checked example of the issue (times in ms)."""
    nem = {"type": "info", "f": "start", "value": None, "process": "nemesis", "time": 21 * 10 ** 6}
    return [op("invoke", "add", 0, 0, 0), op("ok", "add", 0, 0, 1), op("invoke", "add", 1, 1, 2), op("ok", "add", 1, 1, 3),
            op("invoke", "read", None, 2, 4), op("invoke", "add", 2, 0, 5), op("ok", "read", [0], 2, 6),
            op("ok", "add", 2, 0, 7), op("invoke", "add", 3, 1, 8), op("info", "add", 3, 1, 9),
            op("invoke", "add", 4, 0, 10), op("ok", "add", 4, 0, 11), op("invoke", "read", None, 2, 12),
            op("ok", "read", [0, 1, 3, 3], 2, 20), nem, op("invoke", "add", 5, 1, 22), op("fail", "add", 5, 1, 23),
            op("invoke", "read", None, 3, 24), op("invoke", "read", None, 2, 25), op("ok", "read", [0, 1, 2, 3], 2, 26),
            op("ok", "read", [0, 1, 2, 3, 4], 3, 30), op("invoke", "add", 6, 0, 31), op("ok", "add", 6, 0, 32)]


HAND_PER = {0: ("stable", 0, 1, -1), 1: ("stable", 1, 3, 4), 2: ("stable", 5, 7, 12), 3: ("stable", 0, 13, -1),
            4: ("lost", 13, 11, 18), 5: ("never-read", -1, -1, 18), 6: ("never-read", -1, 22, -1)}
HAND_WANT = {"valid?": False, "attempt-count": 7, "stable-count": 4, "lost-count": 1, "never-read-count": 2,
             "stale-count": 2, "duplicated-count": 1, "lost": [4], "never-read": [5, 6], "stale": [1, 2],
             "duplicated": {3: 2}, "stable-latencies": {0: 0, 0.5: 1, 0.95: 5, 0.99: 5, 1: 5},
             "lost-latencies": {0: 13, 0.5: 13, 0.95: 13, 0.99: 13, 1: 13}}
HAND_WORST = [2, 1]  # the elements of :worst-stale


ERROR_KINDS = ("nil-add", "ok-without-invoke", "read-without-invoke", "read-not-collection", "nil-in-read")


def random_key(rng: random.Random, max_adds=40, error_rate=0.015):
    """One key's ops (no times yet): up to five adders and three readers run
    concurrently against a set that applies an add somewhere between its
    invocation and its completion, so reads straddle adds and complete out of
    invocation order.  :fail / :info completions, re-invoked elements, reads
    that drop elements (lost or stale) or hold unexpected ones, vector reads
    with duplicates, nil and empty reads, sparse / extreme / negative
    elements; and each error case of the rules with probability error_rate."""
    n = rng.randint(0, max_adds)
    style = rng.choice(["range", "range", "sparse", "wide", "extreme", "negative"])
    pool = {"range": lambda: rng.randint(0, max(n, 1)),
            "sparse": lambda: rng.randint(-50, 5000),
            "wide": lambda: rng.choice([-5, 0, 1, 2, 10 ** 12, 10 ** 12 + 1, rng.randint(-10 ** 15, 10 ** 15)]),
            "extreme": lambda: rng.choice([-1, 0, 1, I64_MAX, I64_MAX - 1, -I64_MAX, -I64_MAX + 1]),
            "negative": lambda: rng.randint(-3 * max(n, 1), -1)}[style]
    errors = [k for k in ERROR_KINDS if rng.random() < error_rate]
    ops, state, invoked, dropped = [], set(), [], set()
    adds, reads = {}, {}  # process -> pending op
    started = 0
    next_proc = 8
    adders, readers = [0, 1, 2, 3, 4], [5, 6, 7]
    while started < n or adds or reads:
        free_a = [p for p in adders if p not in adds]
        free_r = [p for p in readers if p not in reads]
        moves = []
        if started < n and free_a:
            moves += ["add"] * 3
        if adds:
            moves += ["add-done"] * 3
        if free_r and (started < n or rng.random() < 0.3):
            moves += ["read"]
        if reads:
            moves += ["read-done"] * 2
        move = rng.choice(moves) if moves else "add-done"
        if move == "add":
            p = rng.choice(free_a)
            e = pool() if not invoked or rng.random() > 0.1 else rng.choice(invoked)  # re-invoked elements
            invoked.append(e)
            started += 1
            adds[p] = {"value": e, "applied": False}
            ops.append({"type": "invoke", "f": "add", "value": e, "process": p})
        elif move == "add-done":
            p = rng.choice(sorted(adds))
            a = adds.pop(p)
            how = rng.choices(["ok", "fail", "info"], [0.8, 0.1, 0.1])[0]
            if how == "ok" or (how == "info" and rng.random() < 0.5):
                state.add(a["value"])
            ops.append({"type": how, "f": "add", "value": a["value"], "process": p})
            if how == "info":  # a crashed process is replaced
                adders[adders.index(p)] = next_proc
                next_proc += 1
        elif move == "read":
            p = rng.choice(free_r)
            reads[p] = set(state)
            ops.append({"type": "invoke", "f": "read", "value": None, "process": p})
        else:
            p = rng.choice(sorted(reads))
            snap = reads.pop(p)
            how = rng.choices(["ok", "fail", "info"], [0.85, 0.08, 0.07])[0]
            value = None
            if how == "ok":
                seen = snap if rng.random() < 0.5 else set(state)
                if rng.random() < 0.04 and seen:
                    dropped.add(rng.choice(sorted(seen)))  # lost from here on
                vals = [x for x in seen if x not in dropped and rng.random() > 0.05]  # a stale miss now and then
                if rng.random() < 0.1:
                    vals.append(pool())  # possibly unexpected
                kind = rng.choices(["set", "vector", "empty", "nil"], [0.55, 0.3, 0.08, 0.07])[0]
                value = set(vals) if kind == "set" else vals + (vals[:rng.randint(1, 3)] if rng.random() < 0.3 else []) if kind == "vector" \
                    else set() if kind == "empty" else None
            ops.append({"type": how, "f": "read", "value": value, "process": p})
            if how == "info":
                readers[readers.index(p)] = next_proc
                next_proc += 1
        if rng.random() < 0.02:
            ops.append({"type": "ok", "f": "cas", "value": [1, 2], "process": 0})  # another :f: contributes nothing
    for kind in errors:
        at = rng.randrange(len(ops) + 1)
        if kind == "nil-add":
            ops.insert(at, {"type": "invoke", "f": "add", "value": None, "process": 0})
        elif kind == "ok-without-invoke":
            ops.insert(at, {"type": "ok", "f": "add", "value": 123456789, "process": 0})
        elif kind == "read-without-invoke":
            ops.insert(at, {"type": "ok", "f": "read", "value": [], "process": 99})
        else:
            ops.insert(at, {"type": "invoke", "f": "read", "value": None, "process": 98})
            ops.insert(at + 1, {"type": "ok", "f": "read", "value": 7 if kind == "read-not-collection" else [None],
                                "process": 98})
    return ops


def random_history(rng: random.Random, max_keys=5, max_adds=40, keyed=None, key_base=100, error_rate=0.015):
    """1..max_keys keys of random_key, interleaved keeping each key's order,
    with nemesis rows between, :time strictly ascending in steps of up to 3 ms
    and :index the row number."""
    n_keys = rng.randint(1, max_keys)
    if keyed is None:
        keyed = n_keys > 1 or rng.random() < 0.5
    per_key = [random_key(rng, max_adds, error_rate) for _ in range(n_keys)]
    out, cursors = [], [0] * n_keys
    live = [k for k in range(n_keys) if per_key[k]]
    while live:
        k = rng.choice(live)
        o = dict(per_key[k][cursors[k]])
        if keyed:
            o["value"] = Tuple(key_base + 7 * k, o["value"])
        out.append(o)
        cursors[k] += 1
        if cursors[k] == len(per_key[k]):
            live.remove(k)
        if rng.random() < 0.02:
            out.append({"type": "info", "f": rng.choice(["start", "stop"]), "value": None, "process": "nemesis"})
    t = 0
    for i, o in enumerate(out):
        t += rng.randint(1, 3_000_000)
        o["time"] = t
        o["index"] = i
    return out


def edn_lines(ops):
    """history.edn as Jepsen writes it, one op map per line, with the ops' own :process and :time."""
    out = []
    for i, o in enumerate(ops):
        proc = str(o["process"]) if is_int(o.get("process")) else ":nemesis"
        out.append("{:type :%s, :f :%s, :value %s, :process %s, :time %d, :index %d}"
                   % (o["type"], o["f"], edn_value(o.get("value")), proc, o.get("time", 0), o.get("index", i)))
    return "\n".join(out) + "\n"
