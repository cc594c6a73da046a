#!/usr/bin/env python3
"""Timing of checker/total-queue and checker/unique-ids (lc_queue_check) on one
MI355X.

For each shape: synthetic history (lincheck.queue.synth_queue / synth_ids),
lc_queue_pack (timed on its own), then warmed lc_queue_check steps.  Per step
the library's own device events (lc_queue_last_timing) give the upload span,
the kernels (reset, tally, classify), the download and the whole call, which
also holds the host's sort of the entries.  Beside them lc_queue_check_host on
the same packed batch -- the same fold over a std::unordered_map on one thread
-- as the baseline, its arrays compared with the device's.

  (a) total-queue, one key x 2,000 rows
  (b) unique-ids, one key x 2 M rows, every value distinct
  (c) total-queue, 1,000 keys x 2,000 rows
  (d) unique-ids, one key x 2 M rows over 16 distinct values: every row lands
      on one of 16 slots, the contended case

--slots-per-row 1,2,4 repeats a shape with the table at the next power of two
at or above that many slots per row (2 is the default plan's), which is how the
default load factor was chosen.

Writes one JSON line per shape and table size to --out
(profiles/queue_timing.json).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "jepsen-etcd-demo_amd"))

FIELDS = ("valid", "counts", "has_range", "ent_key", "ent_class", "ent_val", "ent_mult")


def history(name):
    import numpy as np
    from lincheck import _native as N
    from lincheck import queue as Q
    if name == "a":
        return Q.synth_queue(1, 667, lost=2, duplicated=3, unexpected=1, recovered=2, drain=50, seed=42), N.LC_QM_TOTAL_QUEUE
    if name == "b":
        return Q.synth_ids(1, 2_000_000, dup_rate=0.0, seed=42), N.LC_QM_UNIQUE_IDS
    if name == "c":
        return Q.synth_queue(1000, 667, lost=2, duplicated=3, unexpected=1, recovered=2, drain=50, seed=42), N.LC_QM_TOTAL_QUEUE
    if name == "d":
        h = Q.synth_ids(1, 2_000_000, dup_rate=0.0, seed=42)
        h.value[1::2] = np.random.default_rng(42).integers(0, 16, 2_000_000)  # the :ok rows
        return h, N.LC_QM_UNIQUE_IDS
    raise SystemExit(f"unknown shape {name}")


def run_shape(name, steps, warmup, per_row):
    import numpy as np
    from lincheck import checker as ck
    from lincheck import queue as Q
    t0 = time.perf_counter()
    h, mode = history(name)
    t1 = time.perf_counter()
    packed = Q.PackedQueue(h, mode)
    t2 = time.perf_counter()
    v, n = packed.view, packed.n_rows
    slots = 0
    if per_row != 2:
        slots = 1
        while slots < per_row * n:
            slots *= 2
    used = slots
    if not used:
        used = 256
        while used < 2 * n:
            used *= 2
    dev = ck.Device(0)
    cap = 2 * n
    first, times = None, []
    for i in range(warmup + steps):
        res = Q.check_batch(dev, v, slots, ent_cap=cap)
        if first is None:
            first = res
        if i >= warmup:
            times.append(res.timing)
    host_ms = []
    for i in range(max(1, min(steps, 3))):
        t = time.perf_counter()
        host = Q.check_batch(None, v, ent_cap=cap, host=True)
        host_ms.append((time.perf_counter() - t) * 1e3)
    for field in FIELDS:
        assert np.array_equal(getattr(host, field), getattr(first, field)), field
    distinct = len(np.unique(np.stack([np.ctypeslib.as_array(v.row_key, (n,)).astype(np.int64),
                                       np.ctypeslib.as_array(v.row_val, (n,))]), axis=1).T) if n else 0
    line = dict(shape=name, mode="unique-ids" if mode else "total-queue", n_keys=packed.n_keys, history_rows=int(h.n), rows=n,
                distinct=int(distinct), slots=used, load_factor=distinct / used, table_bytes=16 * used,
                entries=int(len(first.ent_key)), invalid_keys=int((first.valid == 0).sum()), steps=steps, warmup=warmup,
                synth_ms=(t1 - t0) * 1e3, pack_ms=(t2 - t1) * 1e3, upload_bytes=13 * n + packed.n_keys,
                download_bytes=72 * packed.n_keys + 16 + 21 * len(first.ent_key))
    for field in ("upload_ms", "kernel_ms", "download_ms", "total_ms"):
        x = sorted(t[field] for t in times)
        line[field] = dict(median=statistics.median(x), min=x[0], max=x[-1])
    line["kernel_rows_per_us"] = n / (line["kernel_ms"]["median"] * 1e3) if line["kernel_ms"]["median"] > 0 else None
    line["host_fold_ms"] = dict(median=statistics.median(host_ms), min=min(host_ms), max=max(host_ms))
    line["device_total_over_host_fold"] = line["total_ms"]["median"] / line["host_fold_ms"]["median"]
    line["device_kernel_over_host_fold"] = line["kernel_ms"]["median"] / line["host_fold_ms"]["median"]
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b,c,d")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--slots-per-row", default="2", help="comma list; 2 is the default plan")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "queue_timing.json"))
    a = ap.parse_args()
    lines = []
    for name in [s for s in a.shapes.split(",") if s]:
        for per_row in [int(x) for x in a.slots_per_row.split(",") if x]:
            line = run_shape(name, a.steps, a.warmup, per_row)
            lines.append(line)
            print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
