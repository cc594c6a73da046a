#!/usr/bin/env python3
"""Timing of the streaming set-full (lc_setfull_stream_*) on one MI355X,
beside re-checking the growing prefix from scratch.

For shapes (a), (b) and (c) of tools/setfull_timing.py: the
synthetic history is split at every read point (one append ends with the last
:ok :read of a read point) and streamed.  Per append the library's own clock
and device events (lc_setfull_stream_last_timing) give pack, upload, the mark
kernels, the reset + fold + finish kernels and the readback; the host clock
around the call gives the whole append.  The stream is run --warmup + --reps
times in one process; what is reported per append position is the median over
the timed runs, and of those medians the median, minimum and maximum over the
appends, and their sum.

Beside it, in the same process: lc_setfull_pack + lc_setfull_check of the
same prefixes from scratch (host clock around both, the check ends in a device
synchronise).  Every prefix where the shape has at most --max-prefixes read
points; else an evenly spaced sample of that many, and the sum over all
prefixes is ESTIMATED as the sample's mean times the number of read points --
the line says which.  And one check of the finished history.  After the last
append the stream's counts must equal the one-shot check's.

Writes one JSON line per shape to --out (profiles/setfull_stream_timing.json).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "jepsen-etcd-demo_amd"))

# n_keys, adds per key, read every, stale window, lost rate (tools/setfull_timing.py's)
SHAPES = {"a": (1, 5000, 100, 3, 0.0), "b": (1000, 1000, 100, 3, 0.001), "c": (1, 1 << 20, 8192, 8, 0.0)}
FIELDS = ("pack_ms", "upload_ms", "mark_ms", "fold_ms", "readback_ms", "call_ms")


def read_points(h):
    """Row numbers just past the last :ok :read of every read point."""
    import numpy as np
    from lincheck import _native as N
    ok_read = (h.f == N.LC_SF_READ) & (h.type == N.LC_OK_T)
    nxt = np.append(ok_read[1:], False)
    return (np.flatnonzero(ok_read & ~nxt) + 1).tolist()


def spread(xs):
    xs = sorted(xs)
    return dict(median=statistics.median(xs), min=xs[0], max=xs[-1])


def run_shape(name, reps, warmup, max_prefixes):
    import numpy as np
    from lincheck import checker as ck
    from lincheck import setfull as F
    from lincheck.setfull_stream import SetFullStream, rows_of
    n_keys, adds, every, stale, lost = SHAPES[name]
    h = F.synth_set_full(n_keys=n_keys, adds_per_key=adds, read_every=every, stale_window=stale, lost_rate=lost,
                         overlap=True, seed=42)
    cuts = read_points(h)
    if cuts[-1] != h.n:
        cuts.append(h.n)
    parts = [rows_of(h, a, b) for a, b in zip([0] + cuts[:-1], cuts)]
    dev = ck.Device(0)

    # the finished history, one shot
    one = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        packed = F.PackedSetFull(h)
        t1 = time.perf_counter()
        res = F.check_batch(dev, packed.view, True)
        t2 = time.perf_counter()
        if i >= warmup:
            one.append(dict(pack_ms=(t1 - t0) * 1e3, check_ms=(t2 - t1) * 1e3, total_ms=(t2 - t0) * 1e3))
    want_counts, want_valid = res.counts.copy(), res.valid.copy()

    # the stream, append by append
    per_run, totals, reads, ids = [], [], 0, 0
    for i in range(warmup + reps):
        rows = []
        t_run = time.perf_counter()
        with SetFullStream(dev, {"linearizable?": True}) as s:
            for p in parts:
                t0 = time.perf_counter()
                u = s.append(p)
                t1 = time.perf_counter()
                t = s.last_timing()
                t["call_ms"] = (t1 - t0) * 1e3
                rows.append(t)
            total = (time.perf_counter() - t_run) * 1e3
            valid, counts = s.counts()
            assert np.array_equal(valid, want_valid) and np.array_equal(counts, want_counts), "the stream differs from the one-shot check"
            ids = u.ids
        if i >= warmup:
            per_run.append(rows)
            totals.append(total)
    per_append = {f: [statistics.median(run[j][f] for run in per_run) for j in range(len(parts))] for f in FIELDS}

    # the same prefixes from scratch
    n_pts = len(cuts)
    sample = list(range(n_pts)) if n_pts <= max_prefixes else sorted({round(j * (n_pts - 1) / (max_prefixes - 1)) for j in range(max_prefixes)})
    pre = []
    for j in sample:
        ph = rows_of(h, 0, cuts[j])
        best = []
        for i in range(warmup + reps):
            t0 = time.perf_counter()
            pp = F.PackedSetFull(ph)
            t1 = time.perf_counter()
            F.check_batch(dev, pp.view, True)
            t2 = time.perf_counter()
            if i >= warmup:
                best.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3))
        pre.append(dict(rows=cuts[j], pack_ms=statistics.median(b[0] for b in best), check_ms=statistics.median(b[1] for b in best)))
    pre_sum = sum(p["pack_ms"] + p["check_ms"] for p in pre)
    line = dict(shape=name, n_keys=n_keys, adds_per_key=adds, read_every=every, rows=int(h.n), appends=len(parts), ids=int(ids),
                read_elements=int(h.read_off[-1]), reps=reps, warmup=warmup,
                one_shot={f: spread([o[f] for o in one]) for f in ("pack_ms", "check_ms", "total_ms")},
                stream_per_append={f: spread(per_append[f]) for f in FIELDS},
                stream_sum_ms={f: sum(per_append[f]) for f in FIELDS},
                stream_total_ms=spread(totals),
                prefix_recheck=dict(prefixes_measured=len(sample), of=n_pts, sampled=len(sample) < n_pts,
                                    per_prefix_ms=spread([p["pack_ms"] + p["check_ms"] for p in pre]),
                                    pack_share=sum(p["pack_ms"] for p in pre) / max(pre_sum, 1e-9),
                                    sum_measured_ms=pre_sum,
                                    sum_all_prefixes_ms=pre_sum if len(sample) == n_pts else pre_sum / len(sample) * n_pts,
                                    sum_is_estimate=len(sample) < n_pts))
    line["stream_over_one_shot"] = line["stream_total_ms"]["median"] / line["one_shot"]["total_ms"]["median"]
    line["recheck_over_stream"] = line["prefix_recheck"]["sum_all_prefixes_ms"] / line["stream_total_ms"]["median"]
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b,c")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--max-prefixes", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "setfull_stream_timing.json"))
    a = ap.parse_args()
    lines = []
    for name in [s for s in a.shapes.split(",") if s]:
        line = run_shape(name, a.reps, a.warmup, a.max_prefixes)
        lines.append(line)
        print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
