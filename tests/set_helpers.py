"""Helpers of the set-workload tests: jepsen.checker/set restated with Python
sets (the oracle of these tests; Jepsen itself is not available, parity is
unpinned), a random history generator and an EDN writer."""
import random

from lincheck.independent import Tuple, is_tuple

I64_MAX = (1 << 63) - 1
NEVER_READ = {"valid?": "unknown", "error": "Set was never read"}


def is_int(v):
    return isinstance(v, int) and not isinstance(v, bool) and -I64_MAX <= v <= I64_MAX


def interval_str(elements):
    """jepsen.util/integer-interval-set-str."""
    runs = []
    for x in sorted(elements):
        if runs and runs[-1][1] + 1 == x:
            runs[-1][1] = x
        else:
            runs.append([x, x])
    return "#{" + " ".join(str(a) if a == b else f"{a}..{b}" for a, b in runs) + "}"


def restate(ops):
    """jepsen.checker/set over one key's (unwrapped) ops."""
    attempts = [op["value"] for op in ops if op["type"] == "invoke" and op["f"] == "add"]
    adds = [op["value"] for op in ops if op["type"] == "ok" and op["f"] == "add"]
    final = None
    for op in ops:  # (reduce (fn [_ x] x) nil): the last :ok :read's value, nil included
        if op["type"] == "ok" and op["f"] == "read":
            final = op["value"]
    if final is None:
        return dict(NEVER_READ)
    if not isinstance(final, (set, frozenset, list, tuple)) or not all(is_int(x) for x in list(attempts) + list(adds) + list(final)):
        return {"valid?": "unknown", "error": "a set element is nil or not an integer"}
    return restate_sets(attempts, adds, final)


def restate_sets(attempts, adds, final):
    """The result map from the three sets of jepsen.checker/set."""
    attempts, adds, final = set(attempts), set(adds), set(final)
    ok = final & attempts
    unexpected = final - attempts
    lost = adds - final
    recovered = ok - adds
    return {"valid?": not lost and not unexpected,
            "attempt-count": len(attempts), "acknowledged-count": len(adds), "ok-count": len(ok),
            "lost-count": len(lost), "recovered-count": len(recovered), "unexpected-count": len(unexpected),
            "ok": interval_str(ok), "lost": interval_str(lost), "unexpected": interval_str(unexpected),
            "recovered": interval_str(recovered)}


def keys_of(ops):
    seen, out = set(), []
    for op in ops:
        v = op.get("value")
        if is_tuple(v) and v[0] not in seen:
            seen.add(v[0])
            out.append(v[0])
    return out


def sub(ops, k):
    """A key's rows, unwrapped (rows without a tuple contribute nothing to a set)."""
    return [dict(op, value=op["value"][1]) for op in ops if is_tuple(op.get("value")) and op["value"][0] == k]


def restate_independent(ops):
    """{key: result map}; a history without tuples is one key, None."""
    keys = keys_of(ops)
    if not keys:
        return {None: restate(ops)}
    return {k: restate(sub(ops, k)) for k in keys}


def restate_hist(h):
    """restate_independent over SetHistory columns whose elements are all
    integers (large synthetic histories: no op maps are made)."""
    import numpy as np
    from lincheck import _native as N
    out = {}
    keyed = h.key is not None and (h.key != N.LC_NO_KEY).any()
    keys = list(dict.fromkeys(h.key[h.key != N.LC_NO_KEY].tolist())) if keyed else [None]
    for k in keys:
        rows = (h.key == k) if keyed else np.ones(h.n, bool)
        add = rows & (h.f == N.LC_SF_ADD)
        reads = np.flatnonzero(rows & (h.f == N.LC_SF_READ) & (h.type == N.LC_OK_T))
        if not len(reads) or h.elem[reads[-1]] == N.LC_NIL:
            out[k] = dict(NEVER_READ)
            continue
        r = int(reads[-1])
        out[k] = restate_sets(h.elem[add & (h.type == N.LC_INVOKE)].tolist(), h.elem[add & (h.type == N.LC_OK_T)].tolist(),
                              h.read_elem[int(h.read_off[r]):int(h.read_off[r + 1])].tolist())
    return out


def hist_of_sets(keys):
    """A SetHistory from [(attempts, adds, final)] per key, elements in the
    order given (tuples with keys 0, 1, ... when there are several)."""
    import numpy as np
    from lincheck import _native as N
    from lincheck.setcheck import SetHistory
    t, f, key, elem, rl, reads = [], [], [], [], [], []
    for k, (attempts, adds, final) in enumerate(keys):
        a, d, r = np.asarray(list(attempts), np.int64), np.asarray(list(adds), np.int64), np.asarray(list(final), np.int64)
        n = len(a) + len(d) + 1
        t.append(np.concatenate([np.full(len(a), N.LC_INVOKE, np.uint8), np.full(len(d) + 1, N.LC_OK_T, np.uint8)]))
        f.append(np.concatenate([np.full(n - 1, N.LC_SF_ADD, np.uint8), np.full(1, N.LC_SF_READ, np.uint8)]))
        elem.append(np.concatenate([a, d, np.zeros(1, np.int64)]))
        key.append(np.full(n, k, np.int64))
        lens = np.zeros(n, np.int64)
        lens[-1] = len(r)
        rl.append(lens)
        reads.append(r)
    read_off = np.zeros(sum(map(len, t)) + 1, np.int64)
    np.cumsum(np.concatenate(rl), out=read_off[1:])
    return SetHistory(np.concatenate(t), np.concatenate(f), np.concatenate(key) if len(keys) > 1 else None,
                      np.concatenate(elem), read_off, np.concatenate(reads))


def same(got, want):
    """Result maps agree: in full, or for a key that is not checked in
    :valid? and in having an :error."""
    if want.get("valid?") == "unknown":
        return got.get("valid?") == "unknown" and ("error" in got) and \
            (want["error"] != NEVER_READ["error"] or got["error"] == want["error"])
    return got == want


def hand_ops():
    """The hand-checked example: attempts 0..9 and 20, adds 8 and 9
    end :info, the final read is #{0 1 2 4 5 6 7 8 30}."""
    ops = []
    for e in list(range(10)) + [20]:
        ops.append({"type": "invoke", "f": "add", "value": e})
        ops.append({"type": "info" if e in (8, 9) else "ok", "f": "add", "value": e})
    ops.append({"type": "invoke", "f": "read", "value": None})
    ops.append({"type": "ok", "f": "read", "value": {0, 1, 2, 4, 5, 6, 7, 8, 30}})
    for i, op in enumerate(ops):
        op["index"] = i
    return ops


HAND_WANT = {"valid?": False, "attempt-count": 11, "acknowledged-count": 9, "ok-count": 8, "lost-count": 2,
             "recovered-count": 1, "unexpected-count": 1, "ok": "#{0..2 4..8}", "lost": "#{3 20}",
             "unexpected": "#{30}", "recovered": "#{8}"}


def random_history(rng: random.Random, max_keys=5, max_adds=80, keyed=None, key_base=100):
    """1..max_keys keys x 0..max_adds adds with everything the packer has to
    get right: :fail / :info completions, nemesis rows and other :f, duplicate
    attempts, vector reads with duplicates, several reads, a nil read after a
    real one, an empty read, a key without a read, the elements -1, INT64_MAX
    and INT64_MIN + 1, a nil element."""
    n_keys = rng.randint(1, max_keys)
    if keyed is None:
        keyed = n_keys > 1 or rng.random() < 0.5
    per_key = []
    for k in range(n_keys):
        ops = []
        n = rng.randint(0, max_adds)
        style = rng.choice(["range", "range", "sparse", "wide", "extreme"])
        pool = {"range": lambda: rng.randint(0, max(n, 1)),
                "sparse": lambda: rng.randint(-50, 5000),
                "wide": lambda: rng.choice([-5, 0, 1, 2, 10 ** 12, 10 ** 12 + 1, rng.randint(-10 ** 15, 10 ** 15)]),
                "extreme": lambda: rng.choice([-1, 0, 1, I64_MAX, I64_MAX - 1, -I64_MAX, -I64_MAX + 1])}[style]
        elems = []
        for _ in range(n):
            e = pool() if not elems or rng.random() > 0.1 else rng.choice(elems)  # duplicate attempts
            elems.append(e)
            ops.append({"type": "invoke", "f": "add", "value": e})
            how = rng.choices(["ok", "fail", "info"], [0.8, 0.1, 0.1])[0]
            ops.append({"type": how, "f": "add", "value": e})
            if rng.random() < 0.05:
                ops.append({"type": "invoke", "f": "read", "value": None})
                some = [x for x in elems if rng.random() < 0.7]
                ops.append({"type": "ok", "f": "read", "value": some})
            if rng.random() < 0.03:
                ops.append({"type": "ok", "f": "cas", "value": [1, 2]})
        if rng.random() < 0.04 and n:
            ops.insert(rng.randrange(len(ops)), {"type": "invoke", "f": "add", "value": None})  # a nil element
        acked = [o["value"] for o in ops if o["type"] == "ok" and o["f"] == "add"]
        crashed = [o["value"] for o in ops if o["type"] == "info" and o["f"] == "add"]
        kind = rng.choices(["set", "vector", "empty", "none", "nil-last"], [0.5, 0.25, 0.08, 0.09, 0.08])[0]
        if kind != "none":
            final = [x for x in acked if rng.random() < 0.9] + [x for x in crashed if rng.random() < 0.5]
            if rng.random() < 0.3:
                final.append(pool())  # possibly unexpected
            ops.append({"type": "invoke", "f": "read", "value": None})
            if kind == "set":
                ops.append({"type": "ok", "f": "read", "value": set(x for x in final if x is not None)})
            elif kind == "vector":
                ops.append({"type": "ok", "f": "read", "value": final + final[:3]})  # duplicates collapse
            elif kind == "empty":
                ops.append({"type": "ok", "f": "read", "value": set()})
            else:
                ops.append({"type": "ok", "f": "read", "value": set(x for x in final if x is not None)})
                ops.append({"type": "invoke", "f": "read", "value": None})
                ops.append({"type": "ok", "f": "read", "value": None})
            if rng.random() < 0.2:
                ops.append({"type": "fail", "f": "read", "value": None})  # no :ok: contributes nothing
        per_key.append(ops)
    # interleave the keys' rows, keeping each key's order, with nemesis rows between
    out, cursors = [], [0] * n_keys
    live = [k for k in range(n_keys) if per_key[k]]
    while live:
        k = rng.choice(live)
        op = dict(per_key[k][cursors[k]])
        if keyed:
            op["value"] = Tuple(key_base + 7 * k, op["value"])
        out.append(op)
        cursors[k] += 1
        if cursors[k] == len(per_key[k]):
            live.remove(k)
        if rng.random() < 0.02:
            out.append({"type": "info", "f": rng.choice(["start", "stop"]), "value": None, "process": "nemesis"})
    for i, op in enumerate(out):
        op["index"] = i
    return out


def edn_value(v):
    if v is None:
        return "nil"
    if is_tuple(v):
        return f"[{v[0]} {edn_value(v[1])}]"
    if isinstance(v, (set, frozenset)):
        return "#{" + " ".join(edn_value(x) for x in v) + "}"
    if isinstance(v, (list, tuple)):
        return "[" + " ".join(edn_value(x) for x in v) + "]"
    if isinstance(v, str):
        return v  # already EDN text
    return str(v)


def edn_lines(ops):
    """history.edn as Jepsen writes it, one op map per line."""
    out = []
    for i, op in enumerate(ops):
        proc = ":nemesis" if op.get("process") == "nemesis" else str(op.get("process", i % 5))
        out.append("{:type :%s, :f :%s, :value %s, :process %s, :time %d, :index %d}"
                   % (op["type"], op["f"], edn_value(op.get("edn", op.get("value"))), proc, 1000 * i, op.get("index", i)))
    return "\n".join(out) + "\n"
