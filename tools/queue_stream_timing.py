#!/usr/bin/env python3
"""Timing of the streaming total-queue / unique-ids (lc_queue_stream_*) on one
MI355X, beside re-checking the growing prefix from scratch.

Shapes (tools/queue_timing.py's histories):
  (a) unique-ids, one key x 2 M rows, every id distinct, in 20 appends
  (b) total-queue, 1,000 keys x 2,000 rows, the keys' rows merged round-robin,
      in 20 appends
  (c) unique-ids, one key x 2 M rows over 16 distinct values (the contended
      case), in 20 appends
  (d) total-queue, one key x 2,000 rows (the demo's size) at 100 rows per append

Per shape, all in one process, each arm run --warmup + --reps times and the
median over the timed runs kept per append position (then the median, minimum,
maximum and sum over the appends):
  stream        a device stream with the default first table: the host clock
                around each append (the call ends in a device synchronise) and
                the library's own clock and device events
                (lc_queue_stream_last_timing): pack, upload, kernels, readback,
                grow; which appends grew the table and to what
  stream_sized  the same with the first table sized for the whole history, so
                that nothing grows
  host_stream   the same appends through the host stream (one thread)
  recheck       the one-shot path, unchanged: lc_queue_pack + lc_queue_check of
                every one of the same prefixes from scratch (host clock around
                both; where a shape has more than --max-prefixes appends, an
                evenly spaced sample, and the sum over all prefixes is then an
                ESTIMATE: the sample's mean times their number; the line says
                which)
After the last append the device stream's arrays must equal the one-shot
check's and the host stream's.

Writes one JSON line per shape to --out (profiles/queue_stream_timing.json).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "jepsen-etcd-demo_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

FIELDS = ("pack_ms", "upload_ms", "kernel_ms", "readback_ms", "grow_ms", "total_ms", "call_ms")
RESULT = ("valid", "counts", "has_range", "ent_key", "ent_class", "ent_val", "ent_mult")
SHAPES = {"a": ("b", 20, None), "b": ("c", 20, None), "c": ("d", 20, None), "d": ("a", None, 100)}  # queue_timing's shape, appends, rows per append


def round_robin(h, n_keys):
    """The keys' blocks of rows (equal, one after the other) merged row by row."""
    import numpy as np
    from lincheck import queue as Q
    per = h.n // n_keys
    assert per * n_keys == h.n
    order = np.arange(h.n).reshape(n_keys, per).T.reshape(-1)
    dn = np.diff(h.drain_off.astype(np.int64))
    off = np.zeros(h.n + 1, np.uint64)
    np.cumsum(dn[order], out=off[1:])
    dv = [h.drain_val[int(h.drain_off[r]):int(h.drain_off[r + 1])] for r in order[dn[order] > 0]]
    return Q.QueueHistory(h.type[order], h.f[order], h.key[order], h.value[order], off, np.concatenate(dv) if dv else None)


def spread(xs):
    xs = sorted(xs)
    return dict(median=statistics.median(xs), min=xs[0], max=xs[-1])


def stream_runs(dev, mode, parts, opts, runs, warmup):
    """Per append position the median of every field over the timed runs; the
    whole streams' wall times; the last run's updates and results."""
    from lincheck.queue_stream import QueueStream
    per_run, totals, ups, res = [], [], [], None
    for i in range(warmup + runs):
        rows, ups = [], []
        t_run = time.perf_counter()
        with QueueStream(dev, mode, opts) as s:
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
                res = s.results(ent_cap=1 << 16)
        if i >= warmup:
            per_run.append(rows)
            totals.append(total)
    per = {f: [statistics.median(run[j][f] for run in per_run) for j in range(len(parts))] for f in FIELDS}
    return per, totals, ups, res


def arm(per, totals, ups):
    grows = [dict(append=j, slots=u.slots) for j, u in enumerate(ups) if u.grew]
    return dict(per_append={f: spread(per[f]) for f in FIELDS}, sum_ms={f: sum(per[f]) for f in FIELDS},
                whole_stream_ms=spread(totals), grows=grows, slots_first=ups[0].slots if not ups[0].grew else None,
                slots_last=ups[-1].slots, distinct_last=ups[-1].distinct)


def run_shape(dev, name, reps, warmup, max_prefixes):
    import numpy as np
    import queue_timing
    from lincheck import queue as Q
    from lincheck.queue_stream import rows_of
    src, n_appends, per_append = SHAPES[name]
    h, mode = queue_timing.history(src)
    if name == "b":
        h = round_robin(h, 1000)
    step = per_append if per_append else -(-h.n // n_appends)
    cuts = list(range(step, h.n, step)) + [h.n]
    parts = [rows_of(h, a, b) for a, b in zip([0] + cuts[:-1], cuts)]

    packed = Q.PackedQueue(h, mode)
    sized = 1
    while sized < 2 * packed.n_rows:
        sized *= 2
    per, totals, ups, res = stream_runs(dev, mode, parts, None, reps, warmup)
    per_s, totals_s, ups_s, res_s = stream_runs(dev, mode, parts, {"slots": sized}, reps, warmup)
    per_h, totals_h, ups_h, res_h = stream_runs(None, mode, parts, None, reps, warmup)
    assert not any(u.grew for u in ups_s), "the sized stream grew"

    # the same prefixes through the unchanged one-shot path
    n_pts = len(cuts)
    sample = list(range(n_pts)) if n_pts <= max_prefixes else sorted({round(j * (n_pts - 1) / (max_prefixes - 1)) for j in range(max_prefixes)})
    pre, one = [], None
    for j in sample:
        ph = rows_of(h, 0, cuts[j])
        best = []
        for i in range(warmup + reps):
            t0 = time.perf_counter()
            pp = Q.PackedQueue(ph, mode)
            t1 = time.perf_counter()
            one = Q.check_batch(dev, pp.view, ent_cap=1 << 16)
            t2 = time.perf_counter()
            if i >= warmup:
                best.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, one.timing["kernel_ms"]))
        pre.append(dict(rows=cuts[j], pack_ms=statistics.median(b[0] for b in best), check_ms=statistics.median(b[1] for b in best),
                        kernel_ms=statistics.median(b[2] for b in best)))
    assert sample[-1] == n_pts - 1
    for f in RESULT:   # the last prefix is the whole history
        assert np.array_equal(getattr(res, f), getattr(one, f)), ("stream vs one-shot", f)
        assert np.array_equal(getattr(res, f), getattr(res_h, f)) and np.array_equal(getattr(res, f), getattr(res_s, f)), f
    pre_sum = sum(p["pack_ms"] + p["check_ms"] for p in pre)
    line = dict(shape=name, mode="unique-ids" if mode else "total-queue", n_keys=packed.n_keys, history_rows=int(h.n),
                packed_rows=packed.n_rows, appends=len(parts), rows_per_append=step, reps=reps, warmup=warmup,
                entries=int(len(res.ent_key)), slot_bytes=48, sized_slots=sized,
                stream=arm(per, totals, ups), stream_sized=arm(per_s, totals_s, ups_s), host_stream=arm(per_h, totals_h, ups_h),
                recheck=dict(prefixes_measured=len(sample), of=n_pts, sampled=len(sample) < n_pts,
                             per_prefix_ms=spread([p["pack_ms"] + p["check_ms"] for p in pre]),
                             per_prefix_pack_ms=spread([p["pack_ms"] for p in pre]),
                             per_prefix_kernel_ms=spread([p["kernel_ms"] for p in pre]),
                             last_prefix=pre[-1], sum_measured_ms=pre_sum,
                             sum_all_prefixes_ms=pre_sum if len(sample) == n_pts else pre_sum / len(sample) * n_pts,
                             sum_is_estimate=len(sample) < n_pts))
    s_sum = line["stream"]["sum_ms"]["call_ms"]
    line["recheck_sum_over_stream_sum"] = line["recheck"]["sum_all_prefixes_ms"] / s_sum
    line["last_recheck_over_median_append"] = (pre[-1]["pack_ms"] + pre[-1]["check_ms"]) / line["stream"]["per_append"]["call_ms"]["median"]
    line["host_stream_sum_over_stream_sum"] = line["host_stream"]["sum_ms"]["call_ms"] / s_sum
    line["sized_sum_over_stream_sum"] = line["stream_sized"]["sum_ms"]["call_ms"] / s_sum
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b,c,d")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-prefixes", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "queue_stream_timing.json"))
    a = ap.parse_args()
    from lincheck import checker as ck
    dev = ck.Device(0)
    lines = []
    for name in [s for s in a.shapes.split(",") if s]:
        line = run_shape(dev, name, a.reps, a.warmup, a.max_prefixes)
        lines.append(line)
        print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
