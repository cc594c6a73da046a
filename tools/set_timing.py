#!/usr/bin/env python3
"""Timing of the set-workload check (lc_set_check) on one MI355X.

For each shape: synthetic history (lincheck.setcheck.synth_set), lc_set_pack,
then warmed lc_set_check steps.  Per step the library's own device events
(lc_set_last_timing) give the upload span, the kernel span (bitmap zeroing,
mark, classify, scan, write: what a step costs once its input is in HBM --
the set path has no resident-batch form of its own) and the whole call.
Shapes whose key takes the HBM tier run the two mark paths alternating, step
by step, in the same call (tile form / LC_PATH_SET_DIRECT).

  (a) 1 key x 5,000 adds (the demo; latency only)   (b) 1,000 keys x 1,000
  (c) 10,000 keys x 2,000     (d) 1 key x 2^26, (range) order     (e) the same, shuffled

--profile runs rocprofv3 in runs of their own (this script as the child, a
few steps): --kernel-trace --stats for the per-kernel times, then FETCH_SIZE
and WRITE_SIZE in one pass each for the bytes moved, (2 x FETCH + WRITE) KB
as tools/profile_summary.py corrects them on gfx950.  Algorithmic bytes are
computed here from the shapes: ids and classes read once, the HBM tier's
bitmaps zeroed, marked once per nonzero word and read once, records written.

Writes one JSON line per shape to --out (profiles/set_check_timing.json).
"""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "jepsen-etcd-demo_amd"))

SHAPES = {"a": (1, 5000, False), "b": (1000, 1000, False), "c": (10000, 2000, False),
          "d": (1, 1 << 26, False), "e": (1, 1 << 26, True)}


def host_restatement(h):
    """jepsen.checker/set's counts with numpy on the host, one key at a time:
    a baseline for scale, not a reference implementation."""
    import numpy as np
    from lincheck import _native as N
    t0 = time.perf_counter()
    if h.key is None:
        blocks = [(0, h.n)]
    else:  # synth_set lays the keys out one after the other
        cuts = [0] + (np.flatnonzero(h.key[1:] != h.key[:-1]) + 1).tolist() + [h.n]
        blocks = list(zip(cuts[:-1], cuts[1:]))
    out = []
    for b, e in blocks:
        typ, f, el = h.type[b:e], h.f[b:e], h.elem[b:e]
        attempts = np.unique(el[(f == N.LC_SF_ADD) & (typ == N.LC_INVOKE)])
        adds = np.unique(el[(f == N.LC_SF_ADD) & (typ == N.LC_OK_T)])
        last = b + int(np.flatnonzero((f == N.LC_SF_READ) & (typ == N.LC_OK_T))[-1])
        final = np.unique(h.read_elem[h.read_off[last]:h.read_off[last + 1]])
        ok = np.intersect1d(final, attempts, assume_unique=True)
        out.append((len(attempts), len(adds), len(ok), len(np.setdiff1d(adds, final, assume_unique=True)),
                    len(np.setdiff1d(ok, adds, assume_unique=True)), len(np.setdiff1d(final, attempts, assume_unique=True))))
    return (time.perf_counter() - t0) * 1e3, out


def algorithmic_bytes(arrs, n_runs, lds_bits):
    import numpy as np
    span = arrs["span"].astype(np.int64)
    hbm_words = int(((span[span > lds_bits] + 63) // 64).sum())
    K = len(span)
    inputs = 5 * len(arrs["add_id"]) + 4 * len(arrs["read_id"]) + 8 * len(arrs["vals"])
    bitmaps = 3 * 8 * hbm_words * 3   # zeroed, marked (at most every word once), read
    records = 16 * n_runs + K * (48 + 32 + 1)
    return dict(inputs=inputs, bitmaps=bitmaps, records=records, total=inputs + bitmaps + records)


def run_shape(name, steps, warmup, host, scale):
    import numpy as np
    from lincheck import _native as N
    from lincheck import checker as ck
    from lincheck import setcheck as S
    n_keys, adds, shuffle = SHAPES[name]
    if name in "de" and scale:
        adds >>= scale
    t0 = time.perf_counter()
    h = S.synth_set(n_keys=n_keys, adds_per_key=adds, concurrency=10, info_rate=0.02, lost_rate=0.0005,
                    unexpected_rate=0.0002, seed=42, shuffle=shuffle)
    t1 = time.perf_counter()
    packed = S.PackedSet(h)
    t2 = time.perf_counter()
    arrs = packed.arrays() if name not in "de" else None
    info = np.zeros(7, np.int64)
    N.check(N.lib().lc_set_launch_info(N.ptr(info, __import__("ctypes").c_int64)))
    span = N.carray(packed.view.span, packed.n_keys, np.uint32)
    hbm = bool((span > info[3]).any())
    paths = {"tile": ck.Device(0), "direct": ck.Device(0, path_flags=N.LC_PATH_SET_DIRECT)} if hbm else {"lds": ck.Device(0)}
    times = {p: [] for p in paths}
    res = None
    cap = None
    for i in range(warmup + steps):
        for p, dev in paths.items():   # alternating, step by step
            res = S.check_batch(dev, packed.view, run_cap=cap)
            cap = max(len(res.runs), 1)   # the capacity the first step learned: later steps make one call
            if i >= warmup:
                times[p].append(res.timing)
    line = dict(shape=name, n_keys=n_keys, adds_per_key=adds, shuffled=shuffle, rows=int(h.n), steps=steps, warmup=warmup,
                synth_ms=(t1 - t0) * 1e3, pack_ms=(t2 - t1) * 1e3, n_runs=int(len(res.runs)),
                hbm_tier_keys=int((span > info[3]).sum()), invalid_keys=int((res.valid == 0).sum()))
    for p, ts in times.items():
        for field in ("upload_ms", "kernel_ms", "download_ms", "total_ms"):
            v = sorted(t[field] for t in ts)
            line[f"{p}_{field}"] = dict(median=statistics.median(v), min=v[0], max=v[-1])
    if arrs is None:
        arrs = dict(span=span, add_id=np.zeros(int(packed.view.add_off[packed.n_keys]), np.uint8),
                    read_id=np.zeros(int(packed.view.read_off[packed.n_keys]), np.uint8), vals=np.zeros(0))
    line["algorithmic_bytes"] = algorithmic_bytes(arrs, len(res.runs), int(info[3]))
    if host:
        ms, counts = host_restatement(h)
        assert [tuple(c) for c in res.counts.tolist()] == counts, "device counts differ from the numpy restatement"
        line["host_numpy_restatement_ms"] = ms
    return line


def profile(shapes, scale, tmp):
    """rocprofv3 runs of their own: kernel stats, then FETCH_SIZE, then WRITE_SIZE."""
    me = [sys.executable, os.path.abspath(__file__), "--child", "--shapes", ",".join(shapes), "--steps", "3",
          "--warmup", "1", "--scale", str(scale)]
    out = {}
    d = os.path.join(tmp, "kt")
    subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "kt", "--output-format", "csv", "--"] + me,
                   check=True, capture_output=True, timeout=600)
    for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        out["kernel_stats"] = [dict(name=r["Name"], calls=int(r["Calls"]), average_us=float(r["AverageNs"]) / 1e3,
                                    total_us=float(r["TotalDurationNs"]) / 1e3)
                               for r in csv.DictReader(open(path)) if "k_set_" in r["Name"] or "fillBuffer" in r["Name"]]
    kb = {}
    for counter in ("FETCH_SIZE", "WRITE_SIZE"):
        d = os.path.join(tmp, counter)
        subprocess.run(["rocprofv3", "--pmc", counter, "-d", d, "-o", "pmc", "--output-format", "csv", "--"] + me,
                       check=True, capture_output=True, timeout=600)
        for path in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
            for r in csv.DictReader(open(path)):
                if "k_set_" in r["Kernel_Name"] and r["Counter_Name"] == counter:
                    k = re.search(r"k_set_\w+(<\w+>)?", r["Kernel_Name"]).group(0)
                    kb.setdefault(k, {}).setdefault(counter, []).append(float(r["Counter_Value"]))
    out["bytes_moved_per_launch"] = {
        k: dict(launches=len(v.get("FETCH_SIZE", [])),
                bytes=(2 * statistics.mean(v.get("FETCH_SIZE", [0])) + statistics.mean(v.get("WRITE_SIZE", [0]))) * 1024)
        for k, v in kb.items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b,c,d,e")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=int, default=0, help="shapes d and e at 2^(26 - scale) adds")
    ap.add_argument("--no-host", action="store_true", help="skip the numpy restatement")
    ap.add_argument("--host-max-rows", type=int, default=1 << 26, help="numpy restatement only up to this many rows")
    ap.add_argument("--profile", default="", help="shapes to profile with rocprofv3, each in runs of its own")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "set_check_timing.json"))
    ap.add_argument("--child", action="store_true", help="(the profiled run: steps only, nothing written)")
    a = ap.parse_args()
    lines = []
    for name in [s for s in a.shapes.split(",") if s]:
        n_keys, adds, _ = SHAPES[name]
        rows = 2 * n_keys * (adds >> (a.scale if name in "de" else 0))
        line = run_shape(name, a.steps, a.warmup, not a.no_host and not a.child and rows <= a.host_max_rows, a.scale)
        lines.append(line)
        if not a.child:
            print(json.dumps(line), flush=True)
    if a.child:
        return
    with tempfile.TemporaryDirectory() as tmp:
        for name in [s for s in a.profile.split(",") if s]:
            prof = profile([name], a.scale, os.path.join(tmp, name))
            next(l for l in lines if l["shape"] == name).update(prof)
            print(json.dumps(dict(shape=name, **prof)), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
