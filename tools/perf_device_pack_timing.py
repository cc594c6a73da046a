#!/usr/bin/env python3
"""Timing of checker/perf from raw rows (lc_perf_check_history) on one MI355X,
against the path it stands beside.

What is timed is the whole call, from an lc_perf_history in (pageable) host
memory to results in host memory, in three forms:

  device   lc_perf_check_history (+ lc_perf_checked_free)
  check    lc_perf_pack + lc_perf_shape + lc_perf_check (+ lc_perf_packed_free)
  pack     lc_perf_pack alone (+ lc_perf_packed_free)

through ctypes directly, with no Python shaping of the results.  Each form of
each shape runs in a process of its own, one after the other in one session:
warm-up calls, then --steps timed calls (at least 11); median, min and max.
The device form also records the stage split of lc_perf_history_timing (upload
with staging, grouping and pairing, the batch's build, the perf kernels,
download), and checks its results once against the check form's.

  (a) the demo-shaped fixture (about 600 ops)
  (b) 10^6 ops at 300 ops/s, ten processes
  (c) 10^8 ops in time order, ten processes       (only with --shapes ...,c)
  (f) 10^6 ops at 300 ops/s over 10,000 processes

Writes one JSON line per shape to --out (profiles/perf_device_pack_timing.json).
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

S = 10**9
# ops, processes, nanoseconds between invocations
SHAPES = {"a": None, "b": (10**6, 10, 6_666_667), "c": (10**8, 10, 2_000_000), "f": (10**6, 10_000, 6_666_667)}
FORMS = ("device", "check", "pack")
STAGES = ("upload_ms", "pair_ms", "build_ms", "kernel_ms", "download_ms", "total_ms")


def synth(n_ops, clients, gap, seed=42):
    """n_ops rows as `clients` processes log them: groups of `clients` invokes
    and then their completions (tools/perf_timing.py's histories, with the
    number of processes free), a nemesis :start / :stop pair every 100,000 rows."""
    import numpy as np
    from lincheck import _native as N
    from lincheck import perf as P
    rng = np.random.default_rng(seed)
    pairs, c = n_ops // 2, clients
    i = np.arange(pairs, dtype=np.int64)
    x = i * gap + rng.integers(0, gap // 2, pairs)
    lat = (rng.lognormal(1.2, 0.8, pairs) * 1e6).astype(np.int64)
    typ = rng.choice(np.array([N.LC_OK_T, N.LC_OK_T, N.LC_OK_T, N.LC_FAIL, N.LC_INFO], np.uint8), pairs)
    f = rng.integers(0, 3, pairs).astype(np.uint8)
    g, pos = i // c, i % c
    size = np.minimum(c, pairs - g * c)
    inv_row, done_row = 2 * g * c + pos, 2 * g * c + size + pos
    n = 2 * pairs
    type_, fcol = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    process, tcol = np.zeros(n, np.int64), np.zeros(n, np.int64)
    type_[done_row] = typ
    fcol[inv_row] = fcol[done_row] = f
    process[inv_row] = process[done_row] = pos
    tcol[inv_row], tcol[done_row] = x, x + lat
    nem = np.arange(50_000, n, 100_000)
    type_[nem], process[nem] = N.LC_INFO, N.LC_NO_PROCESS
    fcol[nem] = 3 + (np.arange(len(nem)) % 2)
    return P.PerfHistory(type_, fcol, process, tcol, ["read", "write", "cas", "start", "stop"])


def history(name):
    from lincheck import perf as P
    if SHAPES[name] is None:
        return P.PerfHistory.read_edn(os.path.join(ROOT, "tests", "golden", "perf_demo_history.edn"))
    return synth(*SHAPES[name])


def child(name, form, steps, warmup):
    import numpy as np
    from lincheck import _native as N
    from lincheck import checker as ck
    from lincheck import perf as P
    L = N.lib()
    h = history(name)
    c = h.as_c()
    o = P.make_opts()
    dev = None if form == "pack" else ck.Device(0)
    line = dict(shape=name, form=form, rows=int(h.n), steps=steps, warmup=warmup)
    bufs = {}

    def device_call():
        out = C.c_void_p()
        N.check(L.lc_perf_check_history(dev.handle, C.byref(c), C.byref(o), C.byref(out)))
        L.lc_perf_checked_free(out)

    def packed_call():
        p = C.c_void_p()
        N.check(L.lc_perf_pack(C.byref(c), C.byref(p)))
        if form == "check":
            v = N.LcPerfBatch()
            N.check(L.lc_perf_packed_view(p, C.byref(v)))
            shape = (C.c_int64 * 4)()
            N.check(L.lc_perf_shape(C.byref(v), C.byref(o), shape))
            F, nr, nq = int(v.n_f), int(shape[1]), int(shape[3])
            sizes = (max(F * 3 * nr, 1), max(F * nq, 1), max(F * nq * int(o.n_q), 1))
            if bufs.get("sizes") != sizes:
                bufs.update(sizes=sizes, rate=np.zeros(sizes[0], np.uint64), group=np.zeros(sizes[1], np.uint64),
                            quant=np.zeros(sizes[2], np.int64))
            r = N.LcPerfResult(N.ptr(bufs["rate"], C.c_uint64), N.ptr(bufs["group"], C.c_uint64), N.ptr(bufs["quant"], C.c_int64),
                               sizes[0], sizes[1], sizes[2], 0, 0, 0, 0)
            N.check(L.lc_perf_check(dev.handle, C.byref(v), C.byref(o), C.byref(r)))
        L.lc_perf_packed_free(p)

    call = device_call if form == "device" else packed_call
    if form == "device":   # once, against the host pack's path
        got = P.CheckedPerf(dev, h, o)
        packed = P.PackedPerf(h)
        want = P.check_batch(dev, packed.view, o)
        for field in ("rate", "group", "quant"):
            assert np.array_equal(getattr(got.results, field), getattr(want, field)), field
        assert (got.n, got.matched, got.unmatched, got.orphans) == (packed.n, packed.matched, packed.unmatched, packed.orphans)
        assert np.array_equal(got.intervals, packed.intervals)
        line.update(records=got.n, matched=got.matched, unmatched=got.unmatched, orphans=got.orphans,
                    intervals=int(len(got.intervals)), processes=int(len(np.unique(h.process))))
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
            N.check(L.lc_perf_history_timing(dev.handle, s))
            stages.append(list(s))
    line["call_ms"] = dict(median=statistics.median(ms), min=min(ms), max=max(ms))
    if stages:
        line["stages"] = {name: statistics.median(s[i] for s in stages) for i, name in enumerate(STAGES)}
    print("RESULT " + json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b,f")
    ap.add_argument("--steps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--child-timeout", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "perf_device_pack_timing.json"))
    ap.add_argument("--child", nargs=2, metavar=("SHAPE", "FORM"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.steps < 11:
        ap.error("--steps: at least 11")
    if a.child:
        return child(a.child[0], a.child[1], a.steps, a.warmup)
    lines = []
    for name in [s for s in a.shapes.split(",") if s]:
        line = dict(shape=name)
        for form in FORMS:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, form, "--steps", str(a.steps),
                                "--warmup", str(a.warmup)], capture_output=True, text=True, timeout=a.child_timeout)
            got = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
            if p.returncode != 0 or not got:
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit(f"shape {name}, form {form}: exit {p.returncode}")   # nothing more is started
            line[form] = json.loads(got[0][len("RESULT "):])
            print(f"# {name} {form}: {line[form]['call_ms']}", flush=True)
        dev, chk = line["device"]["call_ms"], line["check"]["call_ms"]
        line["device_median_below_check_min"] = dev["median"] < chk["min"]
        line["check_median_over_device_median"] = chk["median"] / dev["median"]
        line["pack_median_over_device_median"] = line["pack"]["call_ms"]["median"] / dev["median"]
        lines.append(line)
        print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
