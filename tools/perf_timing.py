#!/usr/bin/env python3
"""Timing of checker/perf's analysis (lc_perf_check) on one MI355X.

For each shape: a synthetic history built with numpy (or the demo-shaped
fixture), lc_perf_pack, then warmed lc_perf_check steps.  Per step the
library's own device events (lc_perf_last_timing) give the upload span, the
kernel span (count, scan, scatter, select) and the whole call.  The paths
alternate step by step in the same call: the library's choice ("auto"), the
count and scatter kernels without their LDS tile (LC_PERF_COUNT_DIRECT) and,
where the shape has groups the LDS select would take, every group through
the HBM select (LC_PERF_SELECT_HBM).

  (a) the demo-shaped fixture (about 600 ops)   (b) 10^6 ops at 300 ops/s   (c) 10^8 ops in time order
  (d) 10^8 ops whose invocation times are shuffled over the run: every record
      of a workgroup in another window, the worst case for the tile
  (e) 2^26 ops of one :f in one 30 s window: one group, the worst case for the HBM select

The same series are computed with numpy on the host in the same process
(lexsort by group, time, latency; bincount): a baseline for scale, not a
reference, though the two must agree.  Algorithmic bytes are computed from
the shapes: the record columns read twice (count, scatter), the pairs written
once and read once per select pass, the tables written.

Writes one JSON line per shape to --out (profiles/perf_check_timing.json).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "jepsen-etcd-demo_amd"))

S = 10**9
SHAPES = {"a": None, "b": (10**6, 3, "slow"), "c": (10**8, 3, "ordered"), "d": (10**8, 3, "shuffled"),
          "e": (1 << 26, 1, "one-group")}


def synth(n_ops, n_f, kind, seed=42):
    """n_ops rows: groups of 10 invokes and then their 10 completions, as ten
    clients log them.  ordered / shuffled: 1,000 ops a second (10^8 ops are 28
    hours, 3,334 quantile windows of about 5,000 points per :f: the HBM
    select); slow: 300 ops a second (about 1,500 points per window and :f: the
    LDS select); one-group: everything inside one 30 s window."""
    import numpy as np
    from lincheck import _native as N
    from lincheck import perf as P
    rng = np.random.default_rng(seed)
    pairs, c = n_ops // 2, 10
    i = np.arange(pairs, dtype=np.int64)
    if kind == "one-group":
        x = (i * (29 * S)) // pairs + S
    else:
        gap = 6_666_667 if kind == "slow" else 2_000_000
        x = i * gap + rng.integers(0, gap // 2, pairs)
        if kind == "shuffled":
            x = x[rng.permutation(pairs)]
    lat = (rng.lognormal(1.2, 0.8, pairs) * 1e6).astype(np.int64)
    typ = rng.choice(np.array([N.LC_OK_T, N.LC_OK_T, N.LC_OK_T, N.LC_FAIL, N.LC_INFO], np.uint8), pairs)
    f = rng.integers(0, n_f, pairs).astype(np.uint8)
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
    return P.PerfHistory(type_, fcol, process, tcol, ["read", "write", "cas"][:n_f])


def host_numpy(arrs, n_f, opts):
    """The same tables with numpy on the host: a baseline for scale."""
    import numpy as np
    from lincheck import _native as N
    t0 = time.perf_counter()
    qdt, rdt = int(opts.quantile_dt_ns), int(opts.rate_dt_ns)
    tc, ti, meta = arrs["t_comp"], arrs["t_inv"], arrs["meta"]
    rb = tc // rdt
    r0 = int(rb.min())
    nr = int(rb.max()) - r0 + 1
    ft = ((meta >> 8) & 0xFF).astype(np.int64) * 3 + (((meta >> 16) & 0xFF).astype(np.int64) - 1)
    rate = np.bincount(ft * nr + (rb - r0), minlength=n_f * 3 * nr).reshape(n_f, 3, nr)
    m = ti != N.LC_PERF_NO_INVOKE
    x, lat = ti[m], (tc - ti)[m]
    qb = x // qdt
    q0 = int(qb.min())
    nq = int(qb.max()) - q0 + 1
    gkey = (meta[m] & 0xFF).astype(np.int64) * nq + (qb - q0)
    order = np.lexsort((lat, x, gkey))
    group = np.bincount(gkey, minlength=n_f * nq)
    off = np.concatenate([[0], np.cumsum(group)])
    live = np.flatnonzero(group)
    quant = np.zeros((n_f * nq, int(opts.n_q)), np.int64)
    ls = lat[order]
    for j in range(int(opts.n_q)):
        idx = np.minimum(group[live] - 1, np.floor(group[live].astype(np.float64) * opts.q[j]).astype(np.int64))
        quant[live, j] = ls[off[live] + idx]
    return (time.perf_counter() - t0) * 1e3, rate, group.reshape(n_f, nq), quant.reshape(n_f, nq, -1)


def algorithmic_bytes(packed, res, info, arrs):
    import numpy as np
    n, nm = packed.n, packed.matched
    lds_max = int(info[2])
    big = int(res.group[res.group > lds_max].sum()) if res.group.size else 0
    lat = arrs["t_comp"] - arrs["t_inv"]
    mag = int(np.abs(lat[arrs["t_inv"] != -(1 << 63)]).max()) if nm else 0
    passes = -(-int(res.quantile_dt_ns - 1).bit_length() // 8) + -(-(mag.bit_length() + 1) // 8)
    records = 2 * 20 * n
    pairs = 16 * nm + 16 * (nm - big) + 16 * big * passes
    tables = 8 * (res.rate.size + res.group.size + res.quant.size)
    return dict(records=records, pairs=pairs, tables=tables, total=records + pairs + tables, hbm_points=big, hbm_passes=passes)


def run_shape(name, steps, warmup, host, scale):
    import ctypes as C

    import numpy as np
    from lincheck import _native as N
    from lincheck import checker as ck
    from lincheck import perf as P
    t0 = time.perf_counter()
    if SHAPES[name] is None:
        h = P.PerfHistory.read_edn(os.path.join(ROOT, "tests", "golden", "perf_demo_history.edn"))
        kind = "fixture"
    else:
        n_ops, n_f, kind = SHAPES[name]
        h = synth(n_ops >> (scale if n_ops > 10**6 else 0), n_f, kind)
    t1 = time.perf_counter()
    packed = P.PackedPerf(h)
    t2 = time.perf_counter()
    info = np.zeros(4, np.int64)
    N.check(N.lib().lc_perf_launch_info(N.ptr(info, C.c_int64)))
    dev = ck.Device(0)
    n_f = len(h.names)
    paths = {"auto": 0, "direct": N.LC_PERF_COUNT_DIRECT}
    res = P.check_batch(dev, packed.view, P.make_opts())
    small = int((res.group[res.group <= info[2]]).sum()) if res.group.size else 0
    if small:
        paths["hbm"] = N.LC_PERF_SELECT_HBM
    opts = {p: P.make_opts({"flags": fl}) for p, fl in paths.items()}
    times = {p: [] for p in paths}
    for i in range(warmup + steps):
        for p in paths:   # alternating, step by step
            r = P.check_batch(dev, packed.view, opts[p])
            assert np.array_equal(r.quant, res.quant) and np.array_equal(r.rate, res.rate), f"path {p} differs"
            if i >= warmup:
                times[p].append(r.timing)
    line = dict(shape=name, kind=kind, rows=int(h.n), records=packed.n, matched=packed.matched, n_f=n_f,
                rate_buckets=int(res.rate.shape[2]), quantile_buckets=int(res.group.shape[1]),
                groups=int((res.group > 0).sum()), largest_group=int(res.group.max()) if res.group.size else 0,
                lds_tier_points=small, steps=steps, warmup=warmup, synth_ms=(t1 - t0) * 1e3, pack_ms=(t2 - t1) * 1e3)
    for p, ts in times.items():
        for field in ("upload_ms", "kernel_ms", "download_ms", "total_ms"):
            v = sorted(t[field] for t in ts)
            line[f"{p}_{field}"] = dict(median=statistics.median(v), min=v[0], max=v[-1])
    arrs = packed.arrays()
    line["algorithmic_bytes"] = algorithmic_bytes(packed, res, info, arrs)
    if host:
        ms, rate, group, quant = host_numpy(arrs, n_f, opts["auto"])
        assert np.array_equal(rate, res.rate.astype(np.int64)) and np.array_equal(group, res.group.astype(np.int64))
        live = res.group > 0
        assert np.array_equal(quant[live], res.quant[live]), "device quantiles differ from numpy's"
        line["host_numpy_ms"] = ms
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b,c,d,e")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=int, default=0, help="shapes c, d and e at their size >> scale")
    ap.add_argument("--no-host", action="store_true", help="skip the numpy baseline")
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "perf_check_timing.json"))
    a = ap.parse_args()
    lines = []
    for name in [s for s in a.shapes.split(",") if s]:
        line = run_shape(name, a.steps, a.warmup, not a.no_host, a.scale)
        lines.append(line)
        print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
