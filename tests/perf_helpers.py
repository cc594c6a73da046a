"""jepsen.checker/perf's analysis restated with Python ints, `sorted` and
math.floor (rules 1-7), a hand-written history with
its answer written out by hand, and random-history builders.  The device path
(lc_perf_pack, lc_perf_check) is compared with `restate`, never the other way."""
import math

S = 10**9
MS = 10**6
DEFAULT = {"quantile-dt-ns": 30 * S, "rate-dt-ns": 10 * S, "quantiles": [0.5, 0.95, 0.99, 1.0]}


def is_client(op):
    p = op.get("process")
    return isinstance(p, int) and not isinstance(p, bool)


def restate(ops, opts=None):
    """Rules 1-7 over op maps {"type", "f", "process", "time"}."""
    o = dict(DEFAULT, **(opts or {}))
    qdt, rdt, qs = o["quantile-dt-ns"], o["rate-dt-ns"], o["quantiles"]
    pending, points, records = {}, [], []
    unmatched = orphans = 0
    rate = {}
    intervals, open_t = [], None
    for op in ops:
        t = op["time"]
        if not is_client(op):  # rule 6
            if op["f"] == "start" and open_t is None:
                open_t = t
            elif op["f"] == "stop" and open_t is not None:
                intervals.append((open_t, t))
                open_t = None
            continue
        p = op["process"]
        if op["type"] == "invoke":  # rule 2
            if p in pending:
                unmatched += 1
            pending[p] = op
            continue
        key = (op["f"], op["type"], t // rdt)  # rule 5 (// floors)
        rate[key] = rate.get(key, 0) + 1
        inv = pending.pop(p, None)
        if inv is None:
            orphans += 1
            records.append((op["f"], op["f"], op["type"], t, None))
            continue
        points.append((inv["f"], op["type"], inv["time"], t - inv["time"]))  # rule 3
        records.append((inv["f"], op["f"], op["type"], t, inv["time"]))
    unmatched += len(pending)
    if open_t is not None:
        intervals.append((open_t, max(op["time"] for op in ops)))
    groups = {}
    for f, _, x, lat in points:  # rule 4
        groups.setdefault((f, x // qdt), []).append((x, lat))
    quantiles = {}
    for g, pts in groups.items():
        pts = sorted(pts)
        n = len(pts)
        quantiles[g] = [pts[min(n - 1, math.floor(n * q))][1] for q in qs]
    return {"valid?": True, "points": points, "records": records, "groups": {g: len(p) for g, p in groups.items()},
            "quantiles": quantiles, "rate": rate, "nemesis": intervals, "matched": len(points), "unmatched": unmatched,
            "orphans": orphans}


def tables(names, res):
    """lc_perf_check's tables (lincheck.perf.PerfResults) in restate's form:
    empty groups and zero counts absent."""
    groups, quantiles, rate = {}, {}, {}
    for fi, name in enumerate(names):
        for i, n in enumerate(res.group[fi].tolist() if res.group.size else []):
            if n:
                groups[(name, res.q_first + i)] = n
                quantiles[(name, res.q_first + i)] = res.quant[fi, i].tolist()
        for ti, tname in enumerate(("ok", "fail", "info")):
            for i, c in enumerate(res.rate[fi, ti].tolist() if res.rate.size else []):
                if c:
                    rate[(name, tname, res.rate_first + i)] = c
    return {"groups": groups, "quantiles": quantiles, "rate": rate}


def op(type_, f, process, time):
    return {"type": type_, "f": f, "process": process, "time": time}


def hand_ops():
    """15 rows: a replaced invoke, an orphan, an :info completion, an invoke
    left pending, nemesis rows logged twice and an interval left open.  The two
    :read points of window 0 are (1 s, 5 ms) and (5 s, 2 ms): sorted by time
    every quantile is 2 ms; sorted by latency alone they would be 5 ms."""
    return [
        op("invoke", "read", 0, 1 * S),
        op("invoke", "write", 1, 2 * S),
        op("ok", "read", 0, 1 * S + 5 * MS),
        op("info", "start", "nemesis", 3 * S),
        op("info", "start", "nemesis", 3 * S),
        op("fail", "write", 1, 2 * S + 1 * MS),
        op("invoke", "read", 0, 4 * S),
        op("invoke", "read", 0, 5 * S),
        op("ok", "read", 0, 5 * S + 2 * MS),
        op("ok", "read", 2, 12 * S),
        op("info", "stop", "nemesis", 31 * S),
        op("invoke", "write", 1, 31 * S),
        op("info", "write", 1, 41 * S),
        op("invoke", "cas", 3, 42 * S),
        op("info", "start", "nemesis", 43 * S),
    ]


HAND_WANT = {
    "valid?": True,
    "matched": 4, "unmatched": 2, "orphans": 1,
    "points": [("read", "ok", 1 * S, 5 * MS), ("write", "fail", 2 * S, 1 * MS), ("read", "ok", 5 * S, 2 * MS),
               ("write", "info", 31 * S, 10 * S)],
    "groups": {("read", 0): 2, ("write", 0): 1, ("write", 1): 1},
    "quantiles": {("read", 0): [2 * MS] * 4, ("write", 0): [1 * MS] * 4, ("write", 1): [10 * S] * 4},
    "rate": {("read", "ok", 0): 2, ("read", "ok", 1): 1, ("write", "fail", 0): 1, ("write", "info", 4): 1},
    "nemesis": [(3 * S, 31 * S), (43 * S, 43 * S)],
}


def random_ops(rng, n, fs=("read", "write", "cas"), procs=8, step=1000, jitter=3000, nemesis_every=150, t0=0):
    """n rows of a history whose times are almost in order: every row's time is
    the clock plus a jitter of either sign.  Completions are :ok / :fail /
    :info, some invokes are replaced before they complete (crashed ops), some
    completions have no invoke (orphans), nemesis rows come in pairs."""
    ops, pending, t = [], {}, t0
    while len(ops) < n:
        t += rng.randrange(1, step)
        if nemesis_every and rng.randrange(nemesis_every) == 0:
            nem = op("info", rng.choice(["start", "stop", "start", "stop", "kill"]), "nemesis", t)
            ops += [nem, dict(nem)]
            continue
        p = rng.randrange(procs)
        tt = t + rng.randrange(-jitter, jitter + 1)
        r = rng.random()
        if p in pending and r < 0.92:
            ops.append(op(rng.choice(["ok", "ok", "ok", "fail", "info"]), pending.pop(p), p, tt))
        elif p not in pending and r < 0.03:
            ops.append(op(rng.choice(["ok", "fail", "info"]), rng.choice(fs), p, tt))
        else:
            f = rng.choice(fs)
            pending[p] = f
            ops.append(op("invoke", f, p, tt))
    return ops[:n]


def pairs_ops(points, f="read", type_="ok", process=0):
    """One invoke and its completion per (x, latency) point, in the order given."""
    out = []
    for x, lat in points:
        out.append(op("invoke", f, process, x))
        out.append(op(type_, f, process, x + lat))
    return out


def edn_of(ops):
    """history.edn text of op maps (one map per line), with a :value to skip."""
    def kw(x):
        return x if isinstance(x, int) else ":" + str(x)
    return "".join("{:type %s, :f %s, :value %s, :process %s, :time %d, :index %d}\n"
                   % (kw(o["type"]), kw(o["f"]), o.get("value", "nil"), kw(o["process"]), o["time"], i)
                   for i, o in enumerate(ops))
