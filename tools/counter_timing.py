#!/usr/bin/env python3
"""Timing of checker/counter (lc_counter_check) on one MI355X.

For each shape: synthetic history (lincheck.counter.synth_counter),
lc_counter_pack, then warmed lc_counter_check steps.  Per step the library's
own device events (lc_counter_last_timing) give the upload span, the kernels
(both scans), the download and the whole call.  Beside them
lc_counter_check_host on the same packed batch -- the same fold in plain C++
on one thread -- as the baseline, its arrays compared with the device's.

  (a) one key x 2,000 rows
  (b) one key x 2 M rows
  (c) 1,000 keys x 2,000 rows
  (d) one key x 50 M rows

The kernels' rate is their algorithmic bytes over the kernel span: 9 bytes per
event read twice (k_counter_tile, k_counter_apply), 24 bytes per read, and the
tile records (17 bytes written and read, 16 bytes of carry written and read,
per tile of either scan).

Writes one JSON line per shape to --out (profiles/counter_timing.json).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "jepsen-etcd-demo_amd"))

# n_keys, rows per key
SHAPES = {"a": (1, 2000), "b": (1, 2_000_000), "c": (1000, 2000), "d": (1, 50_000_000)}
FIELDS = ("valid", "n_errors", "lower", "upper", "err_off", "err_idx")


def run_shape(name, steps, warmup, tile):
    import numpy as np
    from lincheck import checker as ck
    from lincheck import counter as CT
    n_keys, rows = SHAPES[name]
    t0 = time.perf_counter()
    h = CT.synth_counter(n_keys=n_keys, ops_per_key=rows // 2, concurrency=5, info_rate=0.02, fail_rate=0.02,
                         stale_rate=0.001, seed=42)
    t1 = time.perf_counter()
    packed = CT.PackedCounter(h)
    t2 = time.perf_counter()
    v, E, R = packed.view, packed.n_events, packed.n_reads
    used = tile or 2048
    tiles = -(-E // used) + -(-R // used)
    dev = ck.Device(0)
    first, times = None, []
    for i in range(warmup + steps):
        res = CT.check_batch(dev, v, tile, err_cap=R)
        if first is None:
            first = res
        if i >= warmup:
            times.append(res.timing)
    host_ms = []
    for i in range(max(1, min(steps, 3))):
        t = time.perf_counter()
        host = CT.check_batch(None, v, err_cap=R, host=True)
        host_ms.append((time.perf_counter() - t) * 1e3)
    for field in FIELDS:
        assert np.array_equal(getattr(host, field), getattr(first, field)), field
    alg = 18 * E + 24 * R + tiles * (2 * 17 + 2 * 16)
    line = dict(shape=name, n_keys=n_keys, rows=int(h.n), events=E, reads=R, reads_out_of_bounds=int(len(first.err_idx)),
                invalid_keys=int((first.valid == 0).sum()), tile=used, tiles=tiles, steps=steps, warmup=warmup,
                synth_ms=(t1 - t0) * 1e3, pack_ms=(t2 - t1) * 1e3,
                upload_bytes=9 * E + 8 * R + 16 * (packed.n_keys + 1), download_bytes=16 * R + 8 * (packed.n_keys + 1) + 8 * len(first.err_idx),
                kernel_algorithmic_bytes=alg)
    for field in ("upload_ms", "kernel_ms", "download_ms", "total_ms"):
        x = sorted(t[field] for t in times)
        line[field] = dict(median=statistics.median(x), min=x[0], max=x[-1])
    line["kernel_GBps"] = alg / (line["kernel_ms"]["median"] * 1e-3) / 1e9 if line["kernel_ms"]["median"] > 0 else None
    line["host_fold_ms"] = dict(median=statistics.median(host_ms), min=min(host_ms), max=max(host_ms))
    line["device_total_over_host_fold"] = line["total_ms"]["median"] / line["host_fold_ms"]["median"]
    line["device_kernel_over_host_fold"] = line["kernel_ms"]["median"] / line["host_fold_ms"]["median"]
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b,c,d")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tile", type=int, default=0, help="0: the default tile")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "counter_timing.json"))
    a = ap.parse_args()
    lines = []
    for name in [s for s in a.shapes.split(",") if s]:
        line = run_shape(name, a.steps, a.warmup, a.tile)
        lines.append(line)
        print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
