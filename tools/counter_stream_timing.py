#!/usr/bin/env python3
"""Timing of the streaming checker/counter (lc_counter_stream_*) on one MI355X,
beside re-checking the growing prefix from scratch.

Shapes (lincheck.counter.synth_counter's histories), 20 appends each:
  (a) one key x 2 M rows
  (b) 1,000 keys x 2,000 rows, the keys' rows merged round-robin
  (c) one key x 2,000 rows (the demo's size) at 100 rows per append
  (d) one key x 2 M rows with 2 % failed ops, 75,000 processes: a round of
      invocations and completions is one and a half appends long, so that a
      :fail :add revises reads that an earlier append left resident

Per shape, all in one process, each arm run --warmup + --reps times and the
median over the timed runs kept per append position (then the median, minimum,
maximum and sum over the appends):
  stream        a device stream: the host clock around each append (the call
                ends in a device synchronise) and the library's own clock and
                device events (lc_counter_stream_last_timing): pack, upload,
                kernels, readback, grow; per append the invocations revised
                (patched) and the resident reads looked at again (revisited)
  host_stream   the same appends through the host stream (one thread)
  recheck       the one-shot path, unchanged: lc_counter_pack + lc_counter_check
                of every one of the same prefixes from scratch (host clock
                around both)
After the last append the device stream's arrays must equal the one-shot
check's and the host stream's.

Writes one JSON line per shape to --out (profiles/counter_stream_timing.json).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "jepsen-etcd-demo_amd"))

FIELDS = ("pack_ms", "upload_ms", "kernel_ms", "readback_ms", "grow_ms", "total_ms", "call_ms")
RESULT = ("valid", "n_errors", "lower", "upper", "err_off", "err_idx")
# n_keys, ops per key, synth_counter's other arguments, rows per append (None: a twentieth)
SHAPES = {"a": (1, 1_000_000, dict(concurrency=5, stale_rate=0.001), None),
          "b": (1000, 1000, dict(concurrency=5, stale_rate=0.001), None),
          "c": (1, 1000, dict(concurrency=5, stale_rate=0.001), 100),
          "d": (1, 1_000_000, dict(concurrency=75_000, stale_rate=0.001, fail_rate=0.02), None)}


def round_robin(h, n_keys):
    """The keys' blocks of rows (equal, one after the other) merged row by row."""
    import numpy as np
    from lincheck import counter as CT
    per = h.n // n_keys
    assert per * n_keys == h.n
    order = np.arange(h.n).reshape(n_keys, per).T.reshape(-1)
    return CT.CounterHistory(h.type[order], h.f[order], h.process[order], h.key[order], h.value[order])


def spread(xs):
    xs = sorted(xs)
    return dict(median=statistics.median(xs), min=xs[0], max=xs[-1])


def stream_runs(dev, parts, runs, warmup):
    """Per append position the median of every field over the timed runs; the
    whole streams' wall times; the last run's updates and results."""
    from lincheck.counter_stream import CounterStream
    per_run, totals, ups, res = [], [], [], None
    for i in range(warmup + runs):
        rows, ups = [], []
        t_run = time.perf_counter()
        with CounterStream(dev) as s:
            for p in parts:
                t0 = time.perf_counter()
                u = s.append(p)
                t1 = time.perf_counter()
                t = s.last_timing()
                t["call_ms"] = (t1 - t0) * 1e3
                rows.append(t)
                ups.append(u)
            total = (time.perf_counter() - t_run) * 1e3
            if i == warmup + runs - 1:
                t0 = time.perf_counter()
                res = s.results()
                results_ms = (time.perf_counter() - t0) * 1e3
        if i >= warmup:
            per_run.append(rows)
            totals.append(total)
    per = {f: [statistics.median(run[j][f] for run in per_run) for j in range(len(parts))] for f in FIELDS}
    return per, totals, ups, res, results_ms


def arm(per, totals, ups, results_ms):
    return dict(per_append={f: spread(per[f]) for f in FIELDS}, sum_ms={f: sum(per[f]) for f in FIELDS},
                whole_stream_ms=spread(totals), results_ms=results_ms, grows=[j for j, u in enumerate(ups) if u.grew],
                patched=[u.patched for u in ups], revisited=[u.revisited for u in ups], events=[u.events for u in ups],
                reads_total=ups[-1].reads_total, changed=sum(len(u.changed) for u in ups))


def run_shape(dev, name, reps, warmup):
    import numpy as np
    from lincheck import counter as CT
    from lincheck.counter_stream import rows_of
    n_keys, per_key, kw, per_append = SHAPES[name]
    h = CT.synth_counter(n_keys=n_keys, ops_per_key=per_key, seed=7, **kw)
    if n_keys > 1:
        h = round_robin(h, n_keys)
    step = per_append if per_append else -(-h.n // 20)
    cuts = list(range(step, h.n, step)) + [h.n]
    parts = [rows_of(h, a, b) for a, b in zip([0] + cuts[:-1], cuts)]

    per, totals, ups, res, res_ms = stream_runs(dev, parts, reps, warmup)
    per_h, totals_h, ups_h, res_h, res_ms_h = stream_runs(None, parts, reps, warmup)

    pre, one = [], None
    for c in cuts:   # the same prefixes through the unchanged one-shot path
        ph = rows_of(h, 0, c)
        best = []
        for i in range(warmup + reps):
            t0 = time.perf_counter()
            pp = CT.PackedCounter(ph)
            t1 = time.perf_counter()
            one = CT.check_batch(dev, pp.view)
            t2 = time.perf_counter()
            if i >= warmup:
                best.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, one.timing["kernel_ms"]))
        pre.append(dict(rows=c, pack_ms=statistics.median(b[0] for b in best), check_ms=statistics.median(b[1] for b in best),
                        kernel_ms=statistics.median(b[2] for b in best)))
    for f in RESULT:   # the last prefix is the whole history
        assert np.array_equal(getattr(res, f), getattr(one, f)), ("stream vs one-shot", f)
        assert np.array_equal(getattr(res, f), getattr(res_h, f)), ("stream vs host stream", f)
    pre_sum = sum(p["pack_ms"] + p["check_ms"] for p in pre)
    line = dict(shape=name, n_keys=n_keys, history_rows=int(h.n), appends=len(parts), rows_per_append=step, reps=reps, warmup=warmup,
                reads=int(len(res.lower)), errors=int(len(res.err_idx)),
                stream=arm(per, totals, ups, res_ms), host_stream=arm(per_h, totals_h, ups_h, res_ms_h),
                recheck=dict(per_prefix_ms=spread([p["pack_ms"] + p["check_ms"] for p in pre]),
                             per_prefix_pack_ms=spread([p["pack_ms"] for p in pre]),
                             per_prefix_kernel_ms=spread([p["kernel_ms"] for p in pre]), last_prefix=pre[-1], sum_ms=pre_sum))
    s_sum = line["stream"]["sum_ms"]["call_ms"]
    line["recheck_sum_over_stream_sum"] = pre_sum / s_sum
    line["host_stream_sum_over_stream_sum"] = line["host_stream"]["sum_ms"]["call_ms"] / s_sum
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b,c,d")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "counter_stream_timing.json"))
    a = ap.parse_args()
    from lincheck import checker as ck
    dev = ck.Device(0)
    lines = []
    for name in [s for s in a.shapes.split(",") if s]:
        line = run_shape(dev, name, a.reps, a.warmup)
        lines.append(line)
        print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
