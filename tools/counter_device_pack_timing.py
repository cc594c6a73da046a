#!/usr/bin/env python3
"""Timing of checker/counter from raw rows (lc_counter_check_history) on one
MI355X, against the path it stands beside.

What is timed is the whole call, from an lc_counter_history in (pageable) host
memory to results in host memory, in three forms:

  device   lc_counter_check_history (+ lc_counter_checked_free)
  check    lc_counter_pack + lc_counter_check (+ lc_counter_packed_free)
  host     lc_counter_pack + lc_counter_check_host (+ lc_counter_packed_free)

through ctypes directly, with no Python shaping of the results.  Each form of
each shape runs in a process of its own, one after the other in one session:
warm-up calls, then --steps timed calls (at least 11); median, min and max.
The device form also records the stage split of lc_counter_history_timing
(upload with staging, grouping and pairing, the batch's build, the scan
kernels, download), and checks its results once against the host form's.

  (a) one key x 2,000 rows
  (b) one key x 2 M rows
  (c) 1,000 keys x 2,000 rows
  (d) one key x 50 M rows              (only with --shapes ...,d)
  (e) one key x 2 M rows, 2 % :fail and 2 % :info
  (f) 200,000 keys x 10 rows

Writes one JSON line per shape to --out
(profiles/counter_device_pack_timing.json).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "jepsen-etcd-demo_amd"))

# n_keys, rows per key, :info and :fail rate
SHAPES = {"a": (1, 2000, 0.0), "b": (1, 2_000_000, 0.0), "c": (1000, 2000, 0.0), "d": (1, 50_000_000, 0.0),
          "e": (1, 2_000_000, 0.02), "f": (200_000, 10, 0.0)}
FORMS = ("device", "check", "host")
STAGES = ("upload_ms", "group_ms", "build_ms", "kernel_ms", "download_ms", "total_ms")
FIELDS = ("valid", "n_errors", "lower", "upper", "err_off", "err_idx")


def history(name):
    import numpy as np
    from lincheck import counter as CT
    n_keys, rows, rate = SHAPES[name]
    if n_keys <= 1000:
        return CT.synth_counter(n_keys=n_keys, ops_per_key=rows // 2, concurrency=5, info_rate=rate, fail_rate=rate,
                                stale_rate=0.001, seed=42)
    # many short keys: one key's rows, repeated under every key
    one = CT.synth_counter(n_keys=1, ops_per_key=rows // 2, concurrency=5, info_rate=rate, fail_rate=rate, stale_rate=0.0, seed=42)
    return CT.CounterHistory(np.tile(one.type, n_keys), np.tile(one.f, n_keys), np.tile(one.process, n_keys),
                             np.repeat(np.arange(n_keys, dtype=np.int64), one.n), np.tile(one.value, n_keys))


def child(name, form, steps, warmup, tile):
    import numpy as np
    from lincheck import _native as N
    from lincheck import checker as ck
    from lincheck import counter as CT
    L = N.lib()
    h = history(name)
    c = h.as_c()
    o = N.LcCounterOpts(tile, 0)
    dev = None if form == "host" else ck.Device(0)
    line = dict(shape=name, form=form, rows=int(h.n), steps=steps, warmup=warmup)

    def device_call():
        out = C.c_void_p()
        N.check(L.lc_counter_check_history(dev.handle, C.byref(c), C.byref(o), C.byref(out)))
        L.lc_counter_checked_free(out)

    def packed_call():
        p = C.c_void_p()
        N.check(L.lc_counter_pack(C.byref(c), C.byref(p)))
        v = N.LcCounterBatch()
        N.check(L.lc_counter_packed_view(p, C.byref(v)))
        K = int(v.n_keys)
        R = int(v.read_off[K])
        valid, n_errors, err_off = np.empty(K, np.int8), np.empty(K, np.uint64), np.empty(K + 1, np.uint64)
        lower, upper, err_idx = np.empty(max(R, 1), np.int64), np.empty(max(R, 1), np.int64), np.empty(max(R, 1), np.uint64)
        r = N.LcCounterResult(N.ptr(valid, C.c_int8), N.ptr(n_errors, C.c_uint64), N.ptr(lower, C.c_int64), N.ptr(upper, C.c_int64),
                              N.ptr(err_off, C.c_uint64), N.ptr(err_idx, C.c_uint64), R, 0)
        if form == "host":
            N.check(L.lc_counter_check_host(C.byref(v), C.byref(r)))
        else:
            N.check(L.lc_counter_check(dev.handle, C.byref(v), C.byref(o), C.byref(r)))
        L.lc_counter_packed_free(p)

    call = device_call if form == "device" else packed_call
    if form == "device":   # once, against the host path
        got = CT.CheckedCounter(dev, h, tile)
        packed = CT.PackedCounter(h)
        want = CT.check_batch(None, packed.view, err_cap=max(packed.n_reads, 1), host=True)
        for field in FIELDS:
            assert np.array_equal(getattr(got.res, field), getattr(want, field)), field
        assert got.keys == packed.keys and np.array_equal(got.status, packed.status)
        line.update(n_keys=got.n_keys, events=got.n_events, reads=got.n_reads, reads_out_of_bounds=int(len(want.err_idx)),
                    error_keys=int(packed.status.sum()))
        del got, packed, want
    ms, stages = [], []
    for i in range(warmup + steps):
        t = time.perf_counter()
        call()
        dt = (time.perf_counter() - t) * 1e3
        if i < warmup:
            continue
        ms.append(dt)
        if form == "device":
            s = (C.c_double * 6)()
            N.check(L.lc_counter_history_timing(dev.handle, s))
            stages.append(list(s))
    line["call_ms"] = dict(median=statistics.median(ms), min=min(ms), max=max(ms))
    if stages:
        line["stages"] = {name: statistics.median(s[i] for s in stages) for i, name in enumerate(STAGES)}
    print("RESULT " + json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b,c,e,f")
    ap.add_argument("--steps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tile", type=int, default=0, help="0: the default tile")
    ap.add_argument("--child-timeout", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "counter_device_pack_timing.json"))
    ap.add_argument("--child", nargs=2, metavar=("SHAPE", "FORM"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.steps < 11:
        ap.error("--steps: at least 11")
    if a.child:
        return child(a.child[0], a.child[1], a.steps, a.warmup, a.tile)
    lines = []
    for name in [s for s in a.shapes.split(",") if s]:
        line = dict(shape=name, n_keys_asked=SHAPES[name][0], rows_per_key=SHAPES[name][1], fail_and_info_rate=SHAPES[name][2])
        for form in FORMS:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, form, "--steps", str(a.steps),
                                "--warmup", str(a.warmup), "--tile", str(a.tile)], capture_output=True, text=True,
                               timeout=a.child_timeout)
            got = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
            if p.returncode != 0 or not got:
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit(f"shape {name}, form {form}: exit {p.returncode}")   # nothing more is started
            line[form] = json.loads(got[0][len("RESULT "):])
        dev, chk = line["device"]["call_ms"], line["check"]["call_ms"]
        line["device_median_below_check_min"] = dev["median"] < chk["min"]
        line["check_median_over_device_median"] = chk["median"] / dev["median"]
        line["host_median_over_device_median"] = line["host"]["call_ms"]["median"] / dev["median"]
        lines.append(line)
        print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
