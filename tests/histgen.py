"""Random small Jepsen histories for property tests (any interleaving,
crashes, failures, unmatched invocations, nil reads, several keys, nemesis)."""
import random

from lincheck.independent import Tuple


def random_history(seed: int, n_keys=1, max_ops=7, procs=3, values=(0, 1, 2), p_info=0.15,
                   p_fail=0.1, p_open=0.05, p_nemesis=0.05, p_garbage_read=0.3, model="cas-register"):
    """model: which ops to draw -- cas-register (read/write/cas), register
    (read/write), mutex (acquire/release) or multi-register (:txn of 1-3
    micro-ops over registers "x" / "y"; reads complete with random values)."""
    fs = {"cas-register": ["read", "write", "cas"], "register": ["read", "write"],
          "mutex": ["acquire", "release"], "multi-register": ["txn"]}[model]
    rng = random.Random(seed)
    ops = []
    pending = {}   # process -> (key, f, value)
    next_proc = procs
    idle = list(range(procs))
    budget = {k: rng.randint(1, max_ops) for k in range(n_keys)}
    while idle or pending:
        choices = []
        if idle and any(budget.values()):
            choices.append("invoke")
        if pending:
            choices.append("complete")
        if not choices:
            break
        if rng.random() < p_nemesis:
            f = rng.choice(["start", "stop"])
            ops.append({"type": "info", "f": f, "value": None, "process": "nemesis"})
            ops.append({"type": "info", "f": f, "value": None, "process": "nemesis"})
        c = rng.choice(choices)
        if c == "invoke":
            p = idle.pop(rng.randrange(len(idle)))
            k = rng.choice([k for k, b in budget.items() if b > 0])
            budget[k] -= 1
            f = rng.choice(fs)
            if f == "txn":
                v = [[rng.choice(["read", "write"]), rng.choice(["x", "y"]), None] for _ in range(rng.randint(1, 3))]
                for m in v:
                    if m[0] == "write":
                        m[2] = rng.choice(values)
            else:
                v = None if f in ("read", "acquire", "release") else (
                    rng.choice(values) if f == "write" else [rng.choice(values), rng.choice(values)])
            ops.append({"type": "invoke", "f": f, "value": Tuple(k, v), "process": p})
            pending[p] = (k, f, v)
        else:
            p = rng.choice(list(pending))
            k, f, v = pending.pop(p)
            r = rng.random()
            if r < p_open:          # never completes
                continue
            if r < p_open + p_info:
                ops.append({"type": "info", "f": f, "value": Tuple(k, v), "process": p})
                np_ = next_proc; next_proc += 1
                idle.append(np_)
                continue
            if r < p_open + p_info + p_fail:
                ops.append({"type": "fail", "f": f, "value": Tuple(k, v), "process": p})
                idle.append(p)
                continue
            if f == "read":
                v = rng.choice(list(values) + [None]) if rng.random() < p_garbage_read else rng.choice(list(values))
            elif f == "txn":
                v = [[m[0], m[1], (rng.choice(list(values) + [None]) if m[0] == "read" else m[2])] for m in v]
            ops.append({"type": "ok", "f": f, "value": Tuple(k, v), "process": p})
            idle.append(p)
    for i, op in enumerate(ops):
        op["index"] = i
    return ops


def mutex_history(seed: int, n_keys=100, rounds=40, procs=6, width=2.0, corrupt=0.2):
    """(model/mutex) histories that are linearizable by construction: each
    round one process acquires at lock-free time t and releases at t + hold;
    every op's interval contains its linearization point (width sets how far
    intervals spread, hence how many ops are pending at once).  A corrupted
    key loses one release, so a later acquire finds the lock held."""
    rng = random.Random(seed)
    rows = []
    for k in range(n_keys):
        t = 0.0
        busy_until = {p: -1e9 for p in range(procs)}
        drop = rng.randrange(1, rounds) if rng.random() < corrupt else -1
        for r in range(rounds):
            free = [p for p in range(procs) if busy_until[p] < t - width]
            p = rng.choice(free) if free else min(busy_until, key=busy_until.get)
            hold = rng.uniform(0.5, 2.0)
            a_lin, r_lin = t, t + hold
            a_inv = max(a_lin - rng.uniform(0, width), busy_until[p] + 1e-3)
            a_ok = a_lin + rng.uniform(0, min(width, hold) * 0.9)
            r_inv = max(r_lin - rng.uniform(0, width), a_ok + 1e-3)
            r_ok = r_lin + rng.uniform(0, width)
            rows.append((a_inv, "invoke", "acquire", k, p))
            rows.append((a_ok, "ok", "acquire", k, p))
            if r != drop:
                rows.append((r_inv, "invoke", "release", k, p))
                rows.append((r_ok, "ok", "release", k, p))
                busy_until[p] = r_ok
            else:
                busy_until[p] = a_ok
            t = r_lin + rng.uniform(0.01, 0.5)
    rows.sort(key=lambda x: x[0])
    ops = [{"type": ty, "f": f, "value": Tuple(k, None), "process": 100 * k + p} for _t, ty, f, k, p in rows]
    for i, op in enumerate(ops):
        op["index"] = i
    return ops


def multi_register_history(seed: int, n_keys=50, n_ops=60, procs=5, regs=("x", "y", "z"), values=(0, 1, 2, 3),
                           width=2.0, corrupt=0.2, p_info=0.0, init=None):
    """(model/multi-register) histories linearizable by construction: each op
    is a :txn of 1-3 micro-ops with a linearization point inside its
    interval, applied there to a ground-truth map; reads complete with what
    they saw (the invocation carries nil reads).  A corrupted key has one
    read return a value the register did not hold.  p_info: a crashed op
    (:info, its effect applied with probability 1/2, the process retired)."""
    rng = random.Random(seed)
    rows = []
    for k in range(n_keys):
        points = sorted(rng.uniform(0, n_ops * 1.0) for _ in range(n_ops))
        truth = dict(init or {})
        bad = rng.randrange(n_ops) if rng.random() < corrupt else -1
        free_at = {p: -1e9 for p in range(procs)}
        next_p = procs
        for i, t in enumerate(points):
            txn = [[rng.choice(["read", "write"]), rng.choice(regs), None] for _ in range(rng.randint(1, 3))]
            cands = [p for p in free_at if free_at[p] < t]
            p = rng.choice(cands) if cands else None
            if p is None:
                p = next_p; next_p += 1
            inv = max(t - rng.uniform(0, width), free_at.get(p, -1e9) + 1e-3)
            done = t + rng.uniform(0, width)
            crashed = rng.random() < p_info
            apply = not crashed or rng.random() < 0.5
            seen = dict(truth)
            out = []
            for m in txn:
                if m[0] == "write":
                    m[2] = rng.choice(values)
                    seen[m[1]] = m[2]
                    out.append(list(m))
                else:
                    out.append([m[0], m[1], seen.get(m[1])])
            if i == bad and any(m[0] == "read" for m in out):
                j = next(j for j, m in enumerate(out) if m[0] == "read")
                out[j][2] = rng.choice([v for v in values if v != out[j][2]])
            if apply:
                truth = seen
            rows.append((inv, "invoke", k, p, [list(m) for m in txn]))
            rows.append((done, "info" if crashed else "ok", k, p, [list(m) for m in txn] if crashed else out))
            if crashed:
                free_at[p] = float("inf")  # a crashed process is retired
            else:
                free_at[p] = done
    rows.sort(key=lambda x: x[0])
    ops = [{"type": ty, "f": "txn", "value": Tuple(k, v), "process": 1000 * k + p} for _t, ty, k, p, v in rows]
    for i, op in enumerate(ops):
        op["index"] = i
    return ops


def register_history(seed: int, n_keys=12, n_ops=60, procs=8, n_values=5, width=2.0, corrupt=0.2, p_info=0.0,
                     p_write=0.5):
    """(model/register) histories linearizable by construction: each op is a
    read or a write of one of n_values values with a linearization point
    inside its interval, applied there to the register's true value; a read
    returns the truth (nil before the first write).  A crashed op (:info, with
    probability p_info) retires its process; a crashed write takes effect with
    probability 1/2.  A corrupted key has one completed read in its second half
    return n_values, a value no op writes.  The register has n_values + 1
    states (nil included) once every value has been written."""
    rng = random.Random(seed)
    values = list(range(n_values))
    rows = []
    for k in range(n_keys):
        points = sorted(rng.uniform(0, n_ops * 1.0) for _ in range(n_ops))
        truth = None
        bad = rng.randrange(n_ops // 2, n_ops) if rng.random() < corrupt else -1
        free_at = {p: -1e9 for p in range(procs)}
        next_p = procs
        corrupted = False
        for i, t in enumerate(points):
            f = "write" if rng.random() < p_write else "read"
            cands = [p for p in free_at if free_at[p] < t]
            p = rng.choice(cands) if cands else None
            if p is None:
                p = next_p; next_p += 1
            inv = max(t - rng.uniform(0, width), free_at.get(p, -1e9) + 1e-3)
            done = t + rng.uniform(0, width)
            crashed = rng.random() < p_info
            apply = not crashed or rng.random() < 0.5
            if f == "write":
                v = rng.choice(values)
                if apply:
                    truth = v
                out = v
            else:
                v, out = None, truth
                if bad >= 0 and i >= bad and not corrupted and not crashed:
                    out = n_values  # a value no write installs: no crashed write can stand in for it
                    corrupted = True
            rows.append((inv, "invoke", f, k, p, v))
            rows.append((done, "info" if crashed else "ok", f, k, p, v if crashed else out))
            free_at[p] = float("inf") if crashed else done  # a crashed process is retired
    rows.sort(key=lambda x: x[0])
    ops = [{"type": ty, "f": f, "value": Tuple(k, v), "process": 1000 * k + p} for _t, ty, f, k, p, v in rows]
    for i, op in enumerate(ops):
        op["index"] = i
    return ops


def mutex_crash_history(seed: int, n_keys=12, rounds=30, procs=6, width=2.0, corrupt=0.2, p_info=0.1, tail=4):
    """(model/mutex) histories with crashed acquires and releases,
    linearizable by construction.  Each round a process acquires at a
    lock-free time t and the lock is released at t + hold, every op's interval
    containing its linearization point.  An op crashes with probability p_info
    (:info, its process retired) and then takes effect with probability 1/2:
      * a crashed acquire that took effect is followed by a release from
        another process (the model's lock has no owner); one that did not
        leaves the lock free and the round ends there;
      * a crashed release that took effect frees the lock; after one that did
        not the lock is held for good, and only crashed ops (none of which
        takes effect) follow, `tail` of them at the most, before the key ends.
    A corrupted key loses every release that follows a completed acquire from
    some round on: each later acquire then needs a crashed release to stand in
    for a lost one, and the key is invalid once they run out."""
    rng = random.Random(seed)
    rows = []
    for k in range(n_keys):
        t = 0.0
        free_at = {p: -1e9 for p in range(procs)}
        next_p = [procs]
        drop = rng.randrange(2, rounds) if rng.random() < corrupt else rounds

        def proc(at):
            cands = [p for p in free_at if free_at[p] < at - width]
            if cands:
                return rng.choice(cands)
            next_p[0] += 1
            free_at[next_p[0] - 1] = -1e9
            return next_p[0] - 1

        def op(f, lin, p, lo, hi):
            """One op of process p linearized at lin, acknowledged within
            (lin, lin + hi]: (crashed, took effect, time of its completion)."""
            inv = max(lin - rng.uniform(0, width), free_at[p] + 1e-3, lo)
            inv = min(inv, lin)
            done = lin + rng.uniform(0, hi)
            crashed = rng.random() < p_info
            applied = not crashed or rng.random() < 0.5
            rows.append((inv, "invoke", f, k, p))
            rows.append((done, "info" if crashed else "ok", f, k, p))
            free_at[p] = float("inf") if crashed else done
            return crashed, applied, done

        stuck = False
        for r in range(rounds):
            hold = rng.uniform(0.5, 2.0)
            p = proc(t)
            crashed, applied, a_done = op("acquire", t, p, -1e9, min(width, hold) * 0.9)
            if applied:
                q = p if not crashed else proc(t + hold)
                if r >= drop and not crashed:
                    pass  # the release is lost: the lock stays held as far as the history tells
                else:
                    crashed, applied, _ = op("release", t + hold, q, a_done + 1e-3, width)
                    if not applied:
                        stuck = True
            t += hold + rng.uniform(0.01, 0.5)
            if stuck:
                break
        if stuck:  # held for good: crashed ops only, none takes effect
            for _ in range(rng.randint(0, tail)):
                p = proc(t)
                inv = max(t - rng.uniform(0, width), free_at[p] + 1e-3)
                rows.append((inv, "invoke", rng.choice(["acquire", "release"]), k, p))
                rows.append((t + rng.uniform(0, width), "info", rows[-1][2], k, p))
                free_at[p] = float("inf")
                t += rng.uniform(0.01, 0.5)
    rows.sort(key=lambda x: x[0])
    ops = [{"type": ty, "f": f, "value": Tuple(k, None), "process": 1000 * k + p} for _t, ty, f, k, p in rows]
    for i, op_ in enumerate(ops):
        op_["index"] = i
    return ops
