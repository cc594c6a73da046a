#!/usr/bin/env python3
"""Timing of checker/set-full (lc_setfull_check) on one MI355X.

For each shape: synthetic history (lincheck.setfull.synth_set_full),
lc_setfull_pack, then warmed lc_setfull_check steps.  Per step the library's
own device events (lc_setfull_last_timing) give the upload span, the matrix
zeroing, the mark kernels, the scan (+ finish) kernels, the download and the
whole call.  Variants of one shape -- the mark kernel's tile form and its
direct form, and several matrix caps -- run alternating, step by step, in the
same process.

  (a) the demo with a read every 100 adds: 1 key x 5,000 adds (every read point is two overlapping reads)
  (b) 1,000 keys x 1,000 adds x 20 reads
  (c) 1 key x 2^20 adds x 256 reads, mostly stable
  (d) the same with 1 % lost elements (their downward walk visits every row)
  (e) 1 key x 2^21 adds x 584 reads: a 146 MiB matrix, past the default cap (banded)

Beside them the per-element definitions with numpy on the host, in the same
process, over the same packed arrays: a baseline for scale, not a reference
(its counts are compared with the device's all the same).

--profile runs rocprofv3 in runs of their own (this script as the child):
--kernel-trace --stats for the per-kernel times, then FETCH_SIZE and
WRITE_SIZE in one pass each for k_setfull_mark's bytes moved, (2 x FETCH +
WRITE) KB as tools/profile_summary.py corrects them on gfx950.  Algorithmic
bytes are computed here from the shapes: every read id once per band, one
32-bit atomic per matrix word that gets a bit.

Writes one JSON line per shape to --out (profiles/setfull_timing.json).
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "jepsen-etcd-demo_amd"))

# n_keys, adds per key, read every, stale window, lost rate
SHAPES = {"a": (1, 5000, 100, 3, 0.0), "b": (1000, 1000, 100, 3, 0.001), "c": (1, 1 << 20, 8192, 8, 0.0),
          "d": (1, 1 << 20, 8192, 8, 0.01), "e": (1, 1 << 21, 7200, 8, 0.0)}
CAPS = {"c": (0, 8 << 20, 1 << 20), "d": (0,), "e": (0, 32 << 20)}  # 0: the default cap
MS = 1_000_000


def host_matrix(arrs):
    """Outcome counts per key from the per-element definitions with numpy,
    one key at a time, ids in blocks of 2^16 columns."""
    import numpy as np
    t0 = time.perf_counter()
    out = []
    for k in range(len(arrs["span"])):
        b, n = int(arrs["id_off"][k]), int(arrs["span"][k])
        r0, r1 = int(arrs["row_off"][k]), int(arrs["row_off"][k + 1])
        off = arrs["el_off"][r0:r1 + 1].astype(np.int64)
        done, inv = arrs["row_pos"][r0:r1, None], arrs["row_inv_pos"][r0:r1, None]
        inv_t, done_t = arrs["row_inv_time"][r0:r1], arrs["row_time"][r0:r1]
        rows = np.repeat(np.arange(r1 - r0), np.diff(off))
        ids = arrs["read_id"][int(off[0]):int(off[-1])].astype(np.int64) if r1 > r0 else np.zeros(0, np.int64)
        tot = np.zeros(5, np.int64)
        for c0 in range(0, n, 1 << 16):
            c1 = min(n, c0 + (1 << 16))
            m = np.zeros((r1 - r0, c1 - c0), bool)
            sel = (ids >= c0) & (ids < c1)
            m[rows[sel], ids[sel] - c0] = True
            at, ack, ack_t = arrs["inv_pos"][b + c0:b + c1], arrs["ack_pos"][b + c0:b + c1], arrs["ack_time"][b + c0:b + c1]
            tracked = at >= 0
            elig = done > at[None, :]
            seen, miss = elig & m, elig & ~m
            lp_r = np.where(seen, inv, -1).argmax(axis=0) if r1 > r0 else np.zeros(c1 - c0, np.int64)
            la_r = np.where(miss, inv, -1).argmax(axis=0) if r1 > r0 else np.zeros(c1 - c0, np.int64)
            has_p, has_a = seen.any(axis=0), miss.any(axis=0)
            lp = np.where(has_p, inv[lp_r, 0] if r1 > r0 else -1, -1)
            la = np.where(has_a, inv[la_r, 0] if r1 > r0 else -1, -1)
            first = seen.argmax(axis=0) if r1 > r0 else np.zeros(c1 - c0, np.int64)
            by_read = has_p & ((ack < 0) | (done[first, 0] < ack)) if r1 > r0 else np.zeros(c1 - c0, bool)
            known = np.where(by_read, done[first, 0] if r1 > r0 else -1, ack)
            known_t = np.where(by_read, done_t[first] if r1 > r0 else 0, ack_t)
            stable = tracked & has_p & (la < lp)
            lost = tracked & ~stable & (known >= 0) & has_a & (lp < la) & (known < la)
            until = np.where(has_a, (inv_t[la_r] if r1 > r0 else 0) + 1, 0)
            stale = stable & (np.maximum(0, until - known_t) // MS > 0)
            tot += [tracked.sum(), stable.sum(), lost.sum(), (tracked & ~stable & ~lost).sum(), stale.sum()]
        out.append(tot.tolist())
    return (time.perf_counter() - t0) * 1e3, out


def run_shape(name, steps, warmup, host):
    import numpy as np
    from lincheck import _native as N
    from lincheck import checker as ck
    from lincheck import setfull as F
    n_keys, adds, every, stale, lost = SHAPES[name]
    t0 = time.perf_counter()
    h = F.synth_set_full(n_keys=n_keys, adds_per_key=adds, read_every=every, stale_window=stale, lost_rate=lost,
                         overlap=True, seed=42)
    t1 = time.perf_counter()
    packed = F.PackedSetFull(h)
    t2 = time.perf_counter()
    v, K = packed.view, packed.n_keys
    n_ids, n_rows = int(v.id_off[K]), int(v.row_off[K])
    n_el = int(v.el_off[n_rows])
    dev = ck.Device(0)
    variants = {}
    for cap in CAPS.get(name, (0,)):
        for form, flags in (("tile", 0), ("direct", N.LC_SETFULL_MARK_DIRECT)):
            if cap and form == "direct":
                continue
            variants[f"{form}_cap{cap >> 20}MiB" if cap else form] = (cap, flags)
    times = {p: [] for p in variants}
    first = None
    for i in range(warmup + steps):
        for p, (cap, flags) in variants.items():   # alternating, step by step
            res = F.check_batch(dev, v, True, cap, flags)
            if first is None:
                first = res
            else:
                for field in ("valid", "counts", "outcome", "latency", "known", "last_absent", "duplicated"):
                    assert np.array_equal(getattr(res, field), getattr(first, field)), (p, field)
            if i >= warmup:
                times[p].append(res.timing)
    line = dict(shape=name, n_keys=n_keys, adds_per_key=adds, read_every=every, rows=int(h.n), reads=n_rows, ids=n_ids,
                read_elements=n_el, steps=steps, warmup=warmup, synth_ms=(t1 - t0) * 1e3, pack_ms=(t2 - t1) * 1e3,
                counts=first.counts.sum(axis=0).tolist(), invalid_keys=int((first.valid == 0).sum()),
                upload_bytes=24 * n_ids + 40 * n_rows + 4 * n_el, download_bytes=26 * n_ids + 49 * K)
    for p, ts in times.items():
        line[p] = dict(passes=ts[0]["passes"], matrix_bytes=ts[0]["matrix_bytes"])
        for field in ("upload_ms", "zero_ms", "mark_ms", "scan_ms", "download_ms", "total_ms"):
            x = sorted(t[field] for t in ts)
            line[p][field] = dict(median=statistics.median(x), min=x[0], max=x[-1])
        # mark's algorithmic bytes: every id once per pass it is re-read in, one 32-bit atomic per word that gets a bit
        passes = ts[0]["passes"] if n_keys == 1 else 1
        line[p]["mark_algorithmic_bytes"] = 4 * n_el * passes + 8 * min(n_el, ts[0]["matrix_bytes"] // 4)
    if host:
        ms, counts = host_matrix(packed._view_arrays())
        assert [c[:5] for c in first.counts.tolist()] == counts, "device counts differ from the numpy restatement"
        line["host_numpy_matrix_ms"] = ms
    return line


def profile(shapes, tmp):
    """rocprofv3 runs of their own: kernel stats, then FETCH_SIZE, then WRITE_SIZE."""
    me = [sys.executable, os.path.abspath(__file__), "--child", "--shapes", ",".join(shapes), "--steps", "2", "--warmup", "1"]
    out = {}
    d = os.path.join(tmp, "kt")
    subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "kt", "--output-format", "csv", "--"] + me,
                   check=True, capture_output=True, timeout=900)
    for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        out["kernel_stats"] = [dict(name=r["Name"], calls=int(r["Calls"]), average_us=float(r["AverageNs"]) / 1e3,
                                    total_us=float(r["TotalDurationNs"]) / 1e3)
                               for r in csv.DictReader(open(path)) if "k_setfull_" in r["Name"] or "fillBuffer" in r["Name"]]
    kb = {}
    for counter in ("FETCH_SIZE", "WRITE_SIZE"):
        d = os.path.join(tmp, counter)
        subprocess.run(["rocprofv3", "--pmc", counter, "-d", d, "-o", "pmc", "--output-format", "csv", "--"] + me,
                       check=True, capture_output=True, timeout=900)
        for path in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
            for r in csv.DictReader(open(path)):
                if "k_setfull_" in r["Kernel_Name"] and r["Counter_Name"] == counter:
                    k = "k_setfull_" + r["Kernel_Name"].split("k_setfull_")[1][:4]
                    kb.setdefault(k, {}).setdefault(counter, []).append(float(r["Counter_Value"]))
    out["bytes_moved_per_launch"] = {
        k: dict(launches=len(x.get("FETCH_SIZE", [])),
                bytes=(2 * statistics.mean(x.get("FETCH_SIZE", [0])) + statistics.mean(x.get("WRITE_SIZE", [0]))) * 1024)
        for k, x in kb.items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b,c,d,e")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy restatement")
    ap.add_argument("--host-max-cells", type=int, default=1 << 30, help="numpy restatement only up to this many (read, id) pairs")
    ap.add_argument("--profile", default="", help="shapes to profile with rocprofv3, each in runs of its own")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "setfull_timing.json"))
    ap.add_argument("--child", action="store_true", help="(the profiled run: steps only, tile form, nothing written)")
    a = ap.parse_args()
    if a.child:
        CAPS.clear()
    lines = []
    for name in [s for s in a.shapes.split(",") if s]:
        n_keys, adds, every, _, _ = SHAPES[name]
        cells = n_keys * adds * 2 * (adds // every + 1)
        line = run_shape(name, a.steps, a.warmup, not a.no_host and not a.child and cells <= a.host_max_cells)
        lines.append(line)
        if not a.child:
            print(json.dumps(line), flush=True)
    if a.child:
        return
    with tempfile.TemporaryDirectory() as tmp:
        for name in [s for s in a.profile.split(",") if s]:
            prof = profile([name], os.path.join(tmp, name))
            next(l for l in lines if l["shape"] == name).update(prof)
            print(json.dumps(dict(shape=name, **prof)), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
