"""checker/counter's rules (include/lincheck_counter.h) written twice, for the
counter tests.  Jepsen is not available to the tests, so these two
restatements of the rule set are the oracle (parity with Jepsen unpinned,
DESIGN.md section 3.14):

  restate      the fold, literally: knossos.history/complete's pairing row by
               row, then lower / upper op by op with a pending-reads map;
  restate_np   independent of it: rows grouped by process to pair them, the
               two contribution columns summed with numpy's cumsum (exact
               Python integers), then a gather at the read rows.

Both take ONE key's ops (values unwrapped) and return the result map:
{"valid?", "reads", "errors"}, or {"valid?": "unknown", "error": text}.
Also here: the hand example, generators of histories and an EDN writer.
"""
import random

import numpy as np

from lincheck.independent import Tuple, history_keys, is_tuple, subhistory

I64_MAX = (1 << 63) - 1


def is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) and -I64_MAX <= int(v) <= I64_MAX


def op(type_, f, process, value=None, **kw):
    return dict({"type": type_, "f": f, "process": process, "value": value}, **kw)


def unknown(why):
    return {"valid?": "unknown", "error": why}


def client_rows(ops):
    return [o for o in ops if o.get("f") in ("add", "read") and is_int(o.get("process"))]


# ---- the fold, literally ---------------------------------------------------------------

def restate(ops):
    rows = client_rows(ops)
    # rule 1: every completion to the open invocation of its process
    value = [o.get("value") for o in rows]
    gone, open_ = set(), {}
    for i, o in enumerate(rows):
        p = o["process"]
        if o["type"] == "invoke":
            if p in open_:
                return unknown("second invocation by a process that has one open")
            open_[p] = i
            continue
        if p not in open_:
            return unknown("completion without an open invocation")
        j = open_.pop(p)
        if rows[j]["f"] != o["f"]:
            return unknown("completion of another :f")
        if o["type"] == "ok":
            value[j] = o.get("value")
        elif o["type"] == "fail":
            gone |= {i, j}
    # rules 2 and 3
    lower = upper = 0
    pending, reads = {}, []
    for i, o in enumerate(rows):
        if i in gone:
            continue
        t, f, p, v = o["type"], o["f"], o["process"], value[i]
        if f == "add" and t in ("invoke", "ok"):
            if not is_int(v) or v < 0:
                return unknown("an add of nil, a non-integer or a negative value")
            if t == "invoke":
                upper += v
                if upper > I64_MAX:
                    return unknown("adds sum past INT64_MAX")
            else:
                lower += v
        elif f == "read" and t == "invoke":
            pending[p] = lower
        elif f == "read" and t == "ok":
            if not is_int(v):
                return unknown("an :ok read of nil or a non-integer")
            reads.append([pending.pop(p), int(v), upper])
    errors = [r for r in reads if not r[0] <= r[1] <= r[2]]
    return {"valid?": not errors, "reads": reads, "errors": errors}


# ---- the same rules through cumsum and a gather ----------------------------------------------

def restate_np(ops):
    rows = client_rows(ops)
    n = len(rows)
    if n == 0:
        return {"valid?": True, "reads": [], "errors": []}
    typ = np.array([("invoke", "ok", "fail", "info").index(o["type"]) for o in rows])
    add = np.array([o["f"] == "add" for o in rows])
    proc = np.array([int(o["process"]) for o in rows], dtype=object)
    vals = [o.get("value") for o in rows]
    # pairing: a process's rows must alternate invocation, completion
    order = sorted(range(n), key=lambda i: (proc[i], i))
    inv, comp = [], []
    at = 0
    while at < n:
        end = at
        while end < n and proc[order[end]] == proc[order[at]]:
            end += 1
        mine = order[at:end]
        for j, i in enumerate(mine):
            if (typ[i] == 0) != (j % 2 == 0):
                return unknown("a process's rows do not alternate invocation and completion")
        for j in range(0, len(mine) - 1, 2):
            inv.append(mine[j])
            comp.append(mine[j + 1])
        at = end
    inv, comp = np.array(inv, dtype=int), np.array(comp, dtype=int)
    if (add[inv] != add[comp]).any():
        return unknown("completion of another :f")
    ok, fail = typ[comp] == 1, typ[comp] == 2
    alive = np.ones(n, bool)
    alive[inv[fail]] = alive[comp[fail]] = False
    final = list(vals)
    for i, c in zip(inv[ok].tolist(), comp[ok].tolist()):
        final[i] = vals[c]
    counted = alive & add & ((typ == 0) | (typ == 1))
    if any(not is_int(final[i]) or final[i] < 0 for i in np.flatnonzero(counted)):
        return unknown("an add of nil, a non-integer or a negative value")
    ok_read = alive & ~add & (typ == 1)
    if any(not is_int(final[i]) for i in np.flatnonzero(ok_read)):
        return unknown("an :ok read of nil or a non-integer")
    up = np.zeros(n, dtype=object)
    low = np.zeros(n, dtype=object)
    for i in np.flatnonzero(counted):
        (up if typ[i] == 0 else low)[i] = int(final[i])
    upper, lower = np.cumsum(up), np.cumsum(low)
    if upper[-1] > I64_MAX:
        return unknown("adds sum past INT64_MAX")
    inv_of = np.full(n, -1)
    inv_of[comp] = inv
    at_ok = np.flatnonzero(ok_read)
    reads = [[int(lower[inv_of[i]]), int(final[i]), int(upper[i])] for i in at_ok]
    errors = [r for r in reads if not r[0] <= r[1] <= r[2]]
    return {"valid?": not errors, "reads": reads, "errors": errors}


def restate_independent(ops, fn=restate):
    """{key: result map} in order of first appearance; {None: ...} when no op is keyed."""
    keys = history_keys(ops)
    if not keys:
        return {None: fn(ops)}
    return {k: fn(subhistory(ops, k)) for k in keys}


def same(got, want):
    """Result maps agree; an :unknown's error text is the implementation's own."""
    if want.get("valid?") == "unknown":
        return got.get("valid?") == "unknown" and isinstance(got.get("error"), str) and bool(got["error"])
    return got == want


def expected_arrays(want):
    """restate_independent's maps as lc_counter_result's arrays (read indices are the batch's)."""
    valid, n_errors, lower, upper, err_off, err_idx = [], [], [], [], [0], []
    base = 0
    for r in want.values():
        if r["valid?"] == "unknown":
            valid.append(-1)
            n_errors.append(0)
        else:
            bad = [i for i, t in enumerate(r["reads"]) if not t[0] <= t[1] <= t[2]]
            valid.append(0 if bad else 1)
            n_errors.append(len(bad))
            lower += [t[0] for t in r["reads"]]
            upper += [t[2] for t in r["reads"]]
            err_idx += [base + i for i in bad]
            base += len(r["reads"])
        err_off.append(len(err_idx))
    return dict(valid=np.array(valid, np.int8), n_errors=np.array(n_errors, np.uint64), lower=np.array(lower, np.int64),
                upper=np.array(upper, np.int64), err_off=np.array(err_off, np.uint64), err_idx=np.array(err_idx, np.uint64))


# ---- the hand example ------------------------------------------------------------------------

HAND_TEXT = """
invoke add 0 1 | invoke read 1 nil | ok add 0 1 | invoke add 2 2 | ok read 1 1 |
invoke add 0 4 | fail add 0 4 | info add 2 2 | invoke read 1 nil | ok read 1 4 |
invoke read 3 nil | invoke add 0 3 | ok add 0 3 | ok read 3 0 |
invoke read 1 nil | fail read 1 nil | invoke read 1 nil | ok read 1 6
"""
HAND_READS = [[0, 1, 3], [1, 4, 3], [1, 0, 6], [4, 6, 6]]
HAND_ERRORS = [[1, 4, 3], [1, 0, 6]]


def hand_ops():
    out = []
    for row in HAND_TEXT.replace("\n", " ").split("|"):
        t, f, p, v = row.split()
        out.append(op(t, f, int(p), None if v == "nil" else int(v)))
    return out


# ---- generators ----------------------------------------------------------------------------------

def keyed(groups):
    """Several keys' ops (key, ops) one after the other as one tuple history."""
    out = []
    for k, ops in groups:
        out += [dict(o, value=Tuple(k, o["value"])) if o["f"] in ("add", "read") else dict(o) for o in ops]
    return out


def interleave(rng, groups):
    """The same, the keys' rows shuffled together (each key's order kept)."""
    tagged = [[dict(o, value=Tuple(k, o["value"])) if o["f"] in ("add", "read") else dict(o) for o in ops] for k, ops in groups]
    at = [0] * len(tagged)
    out = []
    live = [i for i, t in enumerate(tagged) if t]
    while live:
        i = rng.choice(live)
        out.append(tagged[i][at[i]])
        at[i] += 1
        if at[i] == len(tagged[i]):
            live.remove(i)
    return out


def exact_key(rng, n_events, procs=3, p_wrong=0.1, max_add=5):
    """A well-formed key whose packed event list has exactly n_events events:
    :ok adds (2 events), :info adds (1), :ok reads (2), now and then a failed
    op (0), on `procs` processes that overlap.  A read returns the
    acknowledged sum at its completion, or at p_wrong something near it."""
    plan, left = [], n_events
    while left:
        kind = rng.choice(["add-ok", "add-ok", "read-ok", "read-ok", "add-info", "add-fail", "read-fail"])
        cost = {"add-ok": 2, "read-ok": 2, "add-info": 1}.get(kind, 0)
        if cost > left:
            continue
        plan.append(kind)
        left -= cost
    ops, open_, lower, nxt = [], {}, 0, 0
    while nxt < len(plan) or open_:
        free = [p for p in range(procs) if p not in open_]
        if nxt < len(plan) and free and (not open_ or rng.random() < 0.6):
            p, kind = rng.choice(free), plan[nxt]
            nxt += 1
            v = rng.randint(0, max_add) if kind.startswith("add") else None
            open_[p] = (kind, v)
            ops.append(op("invoke", kind.split("-")[0], p, v))
            continue
        p = rng.choice(sorted(open_))
        kind, v = open_.pop(p)
        f, t = kind.split("-")
        if f == "add":
            if t == "ok":
                lower += v
            ops.append(op(t, "add", p, v))
        else:
            got = lower if rng.random() >= p_wrong else lower + rng.choice([-3, -1, 1, 7, 100])
            ops.append(op(t, "read", p, got if t == "ok" else None))
    return ops


BAD_KINDS = ("orphan-completion", "double-invoke", "nil-add", "text-add", "negative-add", "nil-read", "text-read")


def break_key(rng, ops, kind):
    """`ops` (a well-formed key) with one rule-1 or rule-3 error put in."""
    ops = [dict(o) for o in ops]
    at = rng.randint(0, len(ops))
    if kind == "orphan-completion":
        ops.insert(at, op("ok", "add", 77, 1))
    elif kind == "double-invoke":
        ops[at:at] = [op("invoke", "read", 78), op("invoke", "read", 78)]
    elif kind in ("nil-add", "text-add", "negative-add"):
        v = {"nil-add": None, "text-add": "x", "negative-add": -1}[kind]
        ops[at:at] = [op("invoke", "add", 79, 1), op("ok", "add", 79, v)]
    else:
        ops[at:at] = [op("invoke", "read", 80), op("ok", "read", 80, None if kind == "nil-read" else "x")]
    return ops


def random_history(rng, n_rows, n_keys=0, p_bad=0.02, p_nemesis=0.05):
    """About n_rows rows over n_keys interleaved keys (0: no tuples): adds and
    reads on overlapping processes completing :ok, :fail or :info, invocations
    left open, nemesis rows, and at p_bad per row a malformed one (a
    completion nobody invoked, a second invocation, a nil or negative add, a
    nil read)."""
    keys = list(range(n_keys)) or [None]
    state = {k: dict(open={}, lower=0, upper=0) for k in keys}
    out = []

    def emit(k, o):
        if k is not None:
            o["value"] = Tuple(k, o["value"])
        out.append(o)

    for _ in range(n_rows):
        if rng.random() < p_nemesis:
            out.append({"type": "info", "f": rng.choice(["start", "stop"]), "process": "nemesis", "value": None})
            continue
        k = rng.choice(keys)
        s = state[k]
        if rng.random() < p_bad:
            kind = rng.choice(["orphan", "double", "nil-add", "neg-add", "nil-read"])
            if kind == "orphan":
                emit(k, op(rng.choice(["ok", "fail", "info"]), rng.choice(["add", "read"]), 90 + rng.randint(0, 3), 1))
            elif kind == "double" and s["open"]:
                p = rng.choice(sorted(s["open"]))
                emit(k, op("invoke", "read", p))
            elif kind in ("nil-add", "neg-add"):
                p = 95
                if p not in s["open"]:
                    s["open"][p] = ("add", None if kind == "nil-add" else -2)
                    emit(k, op("invoke", "add", p, None if kind == "nil-add" else -2))
            else:
                p = 96
                if p not in s["open"]:
                    emit(k, op("invoke", "read", p))
                    emit(k, op("ok", "read", p, None))
            continue
        free = [p for p in range(4) if p not in s["open"]]
        if free and (not s["open"] or rng.random() < 0.5):
            p = rng.choice(free)
            if rng.random() < 0.5:
                v = rng.randint(0, 9)
                s["open"][p] = ("add", v)
                s["upper"] += v
                emit(k, op("invoke", "add", p, v))
            else:
                s["open"][p] = ("read", None)
                emit(k, op("invoke", "read", p))
        elif s["open"]:
            p = rng.choice(sorted(s["open"]))
            f, v = s["open"].pop(p)
            t = rng.choice(["ok", "ok", "ok", "fail", "info"])
            if f == "add":
                if t == "ok":
                    s["lower"] += v if is_int(v) and v > 0 else 0
                emit(k, op(t, "add", p, v))
            else:
                got = rng.randint(s["lower"] - 1, s["upper"] + 1) if t == "ok" else None
                emit(k, op(t, "read", p, got))
    return out


# ---- EDN --------------------------------------------------------------------------------------------

def edn_value(v):
    if is_tuple(v):
        return f"[{v[0]} {edn_value(v[1])}]"
    return "nil" if v is None else f'"{v}"' if isinstance(v, str) else str(int(v))


def write_edn(ops):
    """history.edn text of the ops, one map per line, :index by position."""
    lines = []
    for i, o in enumerate(ops):
        p = o["process"]
        lines.append(f"{{:type :{o['type']}, :f :{o['f']}, :value {edn_value(o.get('value'))}, "
                     f":process {p if is_int(p) else ':' + str(p)}, :index {i}}}")
    return "\n".join(lines) + "\n"


def rng_of(seed):
    return random.Random(seed)
