#!/usr/bin/env python3
"""Timing of the incremental check (lincheck.stream.Stream) on one MI355X.

Shapes:
  (a) the C1-shaped history, 100 rows per append: per-append latency
  (b) C2's history merged round-robin (one row of each key in turn, 2 M rows),
      in 20 and in 200 appends
  (c) a C3-shard-sized history (12,500 keys x 2,000 ops), in 20 appends
  (d) 100 keys x 100 ops under the partition nemesis with 2% crashed ops (keys
      leave the register tier), 100 rows per append, the resident set tier
      (set_tier) on and off, alternating: what resuming costs against
      restarting once at finish, the device time split into k_stream, the
      migrations and k_stream_set, the share of leaving keys that fall back,
      and the set-record pool's bytes.  --d-info-rate 0.05: the history whose
      sets grow past the cap.
  (dx) shape (d) in three forms alternating in one process: set_tier alone,
      exact alone (keys that leave the register tier restart at finish) and
      both (the exact set tier): totals, finish, the register tier's kernel,
      the migrations and k_stream_set / k_stream_set_exact device time.  With
      --exact on|off --tree, shapes (a) and (b) against the parent commit's
      tree give the register-only streams beside it
      (profiles/stream_exact_set_timing.json).

Per append: the host clock around the call, and the library's own split
(lc_stream_last_timing): host packing, then device events around the upload,
k_stream and the readback.  State bytes read and written are computed from
the plan rule (csrc/stream_plan.hpp: header, five lane arrays, 64 x
2^max(n - 6, 0) lattice words for n ops pending) and each key's pending count
at the append's two ends.

At (b) two comparisons, each form run --reps times alternating in this one
process, after a warm-up round, records checked equal:
  one-shot      lc_pack + lc_check_batch of the whole history, against the sum
                of the appends: the price of resumability
  from-scratch  what a caller had to do before: pack and check rows[0:r_i]
                again at each of the 20 points

--exact on|off times the exact mode (Stream(dev, exact=True)) against the plain
stream on shapes (a) and (b, 20 appends) and on (e), C5's history merged
round-robin (5 % anomalies: keys die online), without the one-shot and
from-scratch comparisons: per-append time, the register tier's kernel
(k_stream_exact or k_stream) device time, and with `on` k_stream_final at
finish and -- (e) -- what the exact mode replaces: one lc_pack +
lc_check_batch with final configs of the invalid keys' sub-histories.  One
form per process, so that forms and trees alternate in one session; --tree
runs another checkout's package (the parent commit's, option off).

--profile runs rocprofv3 --kernel-trace --stats in a run of its own (this
script as the child, shape b, 20 appends, once) and reports k_stream's row.

Writes one JSON document to --out (profiles/stream_timing.json).  Needs a GPU:
there is no CPU path to time.
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
TREE = next((sys.argv[i + 1] for i, x in enumerate(sys.argv[:-1]) if x == "--tree"), ROOT)
sys.path.insert(0, os.path.join(TREE, "jepsen-etcd-demo_amd"))

HDR, LANES = 16, 5 * 64  # stream_plan.hpp


def lattice_words(n):
    return 64 << max(min(n, 10) - 6, 0)


def rows(h, lo, hi):
    from lincheck import history as H
    return H.History(h.type[lo:hi], h.f[lo:hi], h.process[lo:hi], h.key[lo:hi], h.v0[lo:hi], h.v1[lo:hi], h.index[lo:hi])


def merged_round_robin(h):
    """A key-major history's rows, one row of each key in turn."""
    import numpy as np
    from lincheck import history as H
    key = h.key
    start = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]]))
    block = np.repeat(np.arange(len(start)), np.diff(np.concatenate([start, [len(key)]])))
    rank = np.arange(len(key)) - start[block]
    perm = np.lexsort((block, rank))
    return H.History(h.type[perm], h.f[perm], h.process[perm], h.key[perm], h.v0[perm], h.v1[perm],
                     np.arange(len(perm), dtype=np.int64))


def summary(xs):
    xs = list(xs)
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)} if xs else None


def state_bytes(s, searched_after):
    """Record bytes read and written per append, from the plan rule."""
    import numpy as np
    n_app = len(searched_after)
    rd, wr = [0] * n_app, [0] * n_app
    K = len(searched_after[-1])
    for i in range(K):
        w = s.words(i)
        pend = np.concatenate([[0], np.cumsum(np.where((w >> 31).astype(bool), -1, 1))])
        prev = 0
        for a in range(n_app):
            cur = searched_after[a][i] if i < len(searched_after[a]) else 0
            if cur > prev:
                rd[a] += 4 * (HDR + (LANES + lattice_words(int(pend[prev])) if prev else 0))
                wr[a] += 4 * (HDR + LANES + lattice_words(int(pend[cur])))
            prev = cur
    return rd, wr


def run_stream(dev, h, n_appends, want=None, bytes_too=False, set_tier=False, exact=False):
    import numpy as np
    from lincheck.stream import Stream
    n = len(h)
    step = -(-n // n_appends)
    s = Stream(dev, set_tier=set_tier, exact=True) if exact else Stream(dev, set_tier=set_tier)
    per, searched = [], []
    pool_peak = 0
    for lo in range(0, n, step):
        part = rows(h, lo, min(n, lo + step))
        t0 = time.perf_counter()
        up = s.append(part)
        wall = (time.perf_counter() - t0) * 1e3
        t = s.last_timing()
        per.append(dict(wall_ms=wall, events=up.events, rows_held=up.rows_held, **t))
        if set_tier:
            st = s.set_stats()
            per[-1].update(migrate_ms=st["migrate_ms"], set_kernel_ms=st["set_kernel_ms"])
            pool_peak = max(pool_peak, st["pool_in_use"])
        if bytes_too:
            searched.append([s.key_events(i)["searched"] for i in range(up.n_keys)])
    t0 = time.perf_counter()
    up = s.finish()
    fin = (time.perf_counter() - t0) * 1e3
    res = s.results()
    if want is not None:
        assert np.array_equal(res.valid, want.valid) and np.array_equal(res.fail_event, want.fail_event) and \
            np.array_equal(res.cause, want.cause), "stream records differ from the one-shot check"
    out = dict(appends=len(per), finish_ms=fin, n_deferred=up.n_deferred, total_ms=sum(p["wall_ms"] for p in per) + fin,
               events=sum(p["events"] for p in per), per_append=per)
    if set_tier:
        st, t = s.set_stats(), s.tiers()
        left = sum(s.key_events(i)["deferred_at"] >= 0 for i in range(len(res.keys)))
        out.update(tiers=t, keys_left_register_tier=left, fallback_share=(t["fallen_back"] / left if left else 0.0),
                   pool=dict(slot_bytes=st["slot_bytes"], slots_allocated=st["pool_slots"], peak_in_use=st["pool_peak"],
                             peak_bytes=st["pool_peak"] * st["slot_bytes"],
                             allocated_bytes=st["pool_slots"] * st["slot_bytes"]))
    if exact:
        out["final_kernel_ms"] = s.exact_stats()["final_kernel_ms"]
        out["n_invalid"] = int((res.valid == 0).sum())
        if want is not None and want.n_final is not None:
            assert np.array_equal(res.peak, want.peak) and np.array_equal(res.n_final, want.n_final), \
                "exact stream records differ from the one-shot check"
    if bytes_too:
        searched.append([s.key_events(i)["searched"] for i in range(len(res.keys))])
        rd, wr = state_bytes(s, searched[:-1] if len(searched) > len(per) else searched)
        out["state_bytes_read"], out["state_bytes_written"] = rd, wr
    s.close()
    return out


def digest(run):
    keys = ("wall_ms", "pack_ms", "upload_ms", "kernel_ms", "readback_ms")
    d = {k: summary(p[k] for p in run["per_append"]) for k in keys}
    d.update(appends=run["appends"], total_ms=run["total_ms"], finish_ms=run["finish_ms"], events=run["events"],
             n_deferred=run["n_deferred"])
    for k in ("state_bytes_read", "state_bytes_written"):
        if k in run:
            d[k] = summary(run[k])
            d[k]["sum"] = sum(run[k])
    return d


def one_shot(dev, h):
    from lincheck.checker import Packed
    t0 = time.perf_counter()
    pk = Packed(h)
    t1 = time.perf_counter()
    r = dev.check(pk, verdicts_only=True)
    t2 = time.perf_counter()
    return dict(pack_ms=(t1 - t0) * 1e3, check_ms=(t2 - t1) * 1e3, total_ms=(t2 - t0) * 1e3,
                kernel_ms=r.stats["kernel_ms"]), r


def shape_a(dev, reps):
    from lincheck import history as H
    h = H.synth(**H.CONFIGS["C1"])
    _, want = one_shot(dev, h)
    n_app = -(-len(h) // 100)
    run_stream(dev, h, n_app, want)
    runs = [run_stream(dev, h, n_app, want, bytes_too=(r == 0)) for r in range(reps)]
    return dict(shape="a", rows=len(h), rows_per_append=100, runs=[digest(r) for r in runs])


def shape_b(dev, reps, appends=(20, 200)):
    from lincheck import history as H
    h = merged_round_robin(H.synth(**H.CONFIGS["C2"]))
    n = len(h)
    points = [min(n, (i + 1) * -(-n // 20)) for i in range(20)]
    _, want = one_shot(dev, h)
    run_stream(dev, h, 20, want)  # warm-up of every form
    out = dict(shape="b", rows=n, forms={f"stream_{a}": [] for a in appends})
    out["forms"]["one_shot"], out["forms"]["from_scratch_20"] = [], []
    for r in range(reps):  # the forms alternate
        for a in appends:
            out["forms"][f"stream_{a}"].append(digest(run_stream(dev, h, a, want, bytes_too=(r == 0))))
        o, _ = one_shot(dev, h)
        out["forms"]["one_shot"].append(o)
        t0 = time.perf_counter()
        ev = 0
        for p in points:
            o, res = one_shot(dev, rows(h, 0, p))
            ev += int(res.stats["events"])
        out["forms"]["from_scratch_20"].append(dict(total_ms=(time.perf_counter() - t0) * 1e3, points=len(points)))
    tot = lambda f: summary(x["total_ms"] for x in out["forms"][f])
    out["totals_ms"] = {f: tot(f) for f in out["forms"]}
    return out


def shape_c(dev, reps):
    from lincheck import history as H
    h = H.synth(n_keys=12_500, ops_per_key=2000, concurrency=10, seed=3)
    _, want = one_shot(dev, h)
    runs = [run_stream(dev, h, 20, want) for _ in range(max(1, reps - 1))]
    return dict(shape="c", rows=len(h), runs=[digest(r) for r in runs])


def shape_d(dev, reps, info_rate):
    """Set tier on and off, alternating; off is the stream as it was (restart at finish)."""
    from lincheck import history as H
    h = H.synth(n_keys=100, ops_per_key=100, concurrency=10, interleave=True, nemesis_period=5.0, info_rate=info_rate,
                anomaly_rate=0.1, seed=11 if info_rate == 0.02 else 12)
    _, want = one_shot(dev, h)
    n_app = -(-len(h) // 100)
    for on in (True, False):  # warm-up of both forms
        run_stream(dev, h, n_app, want, set_tier=on)
    out = dict(shape="d", rows=len(h), rows_per_append=100, info_rate=info_rate, forms={"set_tier_on": [], "set_tier_off": []})
    for _ in range(reps):
        for on in (True, False):
            run = run_stream(dev, h, n_app, want, set_tier=on)
            d = digest(run)
            if on:
                for k in ("migrate_ms", "set_kernel_ms"):
                    d[k] = summary(p[k] for p in run["per_append"])
                    d[k]["sum"] = sum(p[k] for p in run["per_append"])
                d["kernel_ms"]["sum"] = sum(p["kernel_ms"] for p in run["per_append"])
                d.update({k: run[k] for k in ("tiers", "keys_left_register_tier", "fallback_share", "pool")})
            out["forms"]["set_tier_on" if on else "set_tier_off"].append(d)
    out["totals_ms"] = {f: summary(x["total_ms"] for x in out["forms"][f]) for f in out["forms"]}
    out["finish_ms"] = {f: summary(x["finish_ms"] for x in out["forms"][f]) for f in out["forms"]}
    return out


def shape_d_exact(dev, reps, info_rate):
    """Shape (d) in three forms, alternating: the set tier alone, the exact mode
    alone (keys that leave the register tier restart at finish) and both (the
    exact set tier: k_stream_set_exact, k_stream_set_final at finish)."""
    from lincheck import history as H
    from lincheck.checker import Packed
    h = H.synth(n_keys=100, ops_per_key=100, concurrency=10, interleave=True, nemesis_period=5.0, info_rate=info_rate,
                anomaly_rate=0.1, seed=11 if info_rate == 0.02 else 12)
    want = dev.check(Packed(h))  # with peaks and final configs: the exact forms' records are compared too
    n_app = -(-len(h) // 100)
    forms = {"set_tier": dict(set_tier=True), "exact": dict(exact=True), "exact_set_tier": dict(set_tier=True, exact=True)}
    for kw in forms.values():  # warm-up of every form
        run_stream(dev, h, n_app, want, **kw)
    out = dict(shape="dx", rows=len(h), rows_per_append=100, info_rate=info_rate, forms={f: [] for f in forms})
    for _ in range(reps):
        for f, kw in forms.items():
            run = run_stream(dev, h, n_app, want, **kw)
            d = digest(run)
            d["kernel_ms"]["sum"] = sum(p["kernel_ms"] for p in run["per_append"])
            if kw.get("set_tier"):
                for k in ("migrate_ms", "set_kernel_ms"):
                    d[k] = summary(p[k] for p in run["per_append"])
                    d[k]["sum"] = sum(p[k] for p in run["per_append"])
                d.update({k: run[k] for k in ("tiers", "keys_left_register_tier", "fallback_share", "pool")})
            if kw.get("exact"):
                d["final_kernel_ms"], d["n_invalid"] = run["final_kernel_ms"], run["n_invalid"]
            out["forms"][f].append(d)
    for k in ("total_ms", "finish_ms"):
        out[k] = {f: summary(x[k] for x in out["forms"][f]) for f in forms}
    out["wall_per_append_ms"] = {f: summary(x["wall_ms"]["median"] for x in out["forms"][f]) for f in forms}
    out["register_kernel_sum_ms"] = {f: summary(x["kernel_ms"]["sum"] for x in out["forms"][f]) for f in forms}
    out["set_kernel_sum_ms"] = {f: summary(x["set_kernel_ms"]["sum"] for x in out["forms"][f]) for f in forms if "set_tier" in f}
    out["migrate_sum_ms"] = {f: summary(x["migrate_ms"]["sum"] for x in out["forms"][f]) for f in forms if "set_tier" in f}
    return out


def shape_exact(dev, name, reps, on):
    """One form (exact on / off) of shape a, b (20 appends) or e."""
    import numpy as np
    from lincheck import history as H
    from lincheck.checker import Packed
    if name == "a":
        h = H.synth(**H.CONFIGS["C1"])
        n_app = -(-len(h) // 100)
    else:
        h = merged_round_robin(H.synth(**H.CONFIGS["C2" if name == "b" else "C5"]))
        n_app = 20
    want = dev.check(Packed(h)) if on else one_shot(dev, h)[1]
    run_stream(dev, h, n_app, want, exact=on)  # warm-up
    out = dict(shape=name, rows=len(h), appends=n_app, exact=on, runs=[])
    for _ in range(reps):
        run = run_stream(dev, h, n_app, want, exact=on)
        d = digest(run)
        d["kernel_ms"]["sum"] = sum(p["kernel_ms"] for p in run["per_append"])
        if on:
            d["final_kernel_ms"], d["n_invalid"] = run["final_kernel_ms"], run["n_invalid"]
        out["runs"].append(d)
    bad = np.flatnonzero(want.valid == 0)
    if on and len(bad):  # what the exact mode replaces: pack and search the invalid keys again, final configs asked for
        keys = [Packed(h).keys[i] for i in bad]
        alt = []
        for _ in range(reps + 1):
            t0 = time.perf_counter()
            pk = Packed(h.select_keys(keys))
            t1 = time.perf_counter()
            r = dev.check(pk, peaks=False)
            alt.append(dict(pack_ms=(t1 - t0) * 1e3, check_ms=(time.perf_counter() - t1) * 1e3, kernel_ms=r.stats["kernel_ms"]))
        out["research_invalid_keys"] = dict(keys=len(keys), runs=alt[1:])
    return out


def profile():
    """k_stream's row of rocprofv3 --kernel-trace --stats, in a run of its own."""
    d = tempfile.mkdtemp(prefix="stream_prof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "kt", "--output-format", "csv", "--", sys.executable,
           os.path.abspath(__file__), "--shapes", "b", "--reps", "1", "--appends", "20", "--out", os.path.join(d, "child.json")]
    subprocess.run(cmd, check=True, timeout=900, capture_output=True)
    for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            if "k_stream" in row.get("Name", ""):
                return {k: row[k] for k in row if k in ("Name", "Calls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs")}
    return None


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="a,b,c")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--appends", default="20,200", help="shape b: the append counts")
    ap.add_argument("--d-info-rate", type=float, default=0.02, help="shape d: 0.02 (seed 11) or 0.05 (seed 12)")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--exact", choices=("on", "off"), help="time the exact mode's form on shapes a, b, e (see above)")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package runs (default: this one)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_timing.json"))
    a = ap.parse_args()
    from lincheck import _native as N
    from lincheck.checker import Device
    if N.lib().lc_device_count() < 1:
        sys.exit("stream_timing: no GPU visible; there is nothing to time without one")
    dev = Device(0)
    doc = {"shapes": []}
    for sh in a.shapes.split(","):
        if a.exact:
            doc["shapes"].append(shape_exact(dev, sh, a.reps, a.exact == "on"))
        elif sh == "a":
            doc["shapes"].append(shape_a(dev, a.reps))
        elif sh == "b":
            doc["shapes"].append(shape_b(dev, a.reps, tuple(int(x) for x in a.appends.split(","))))
        elif sh == "c":
            doc["shapes"].append(shape_c(dev, a.reps))
        elif sh == "d":
            doc["shapes"].append(shape_d(dev, a.reps, a.d_info_rate))
        elif sh == "dx":
            doc["shapes"].append(shape_d_exact(dev, a.reps, a.d_info_rate))
        print(json.dumps({k: v for k, v in doc["shapes"][-1].items() if k != "forms"})[:2000], flush=True)
    if a.profile:
        try:
            doc["k_stream_rocprofv3"] = profile()
        except (OSError, subprocess.SubprocessError) as e:
            doc["k_stream_rocprofv3"] = {"error": repr(e)[:300]}
        print(json.dumps(doc["k_stream_rocprofv3"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
