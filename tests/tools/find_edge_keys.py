#!/usr/bin/env python3
"""Find the keys tests/edge_keys.py pins: keys of lincheck.history.synth
batches whose largest :linear sets sit on a set tier's capacity (CPU only: the
C restatement's cref.key_sizes decides everything).

    python tests/tools/find_edge_keys.py            # search the grids, print the table
    python tests/tools/find_edge_keys.py --check    # and compare it with tests/edge_keys.py TABLE

For every key of every batch of the grids below: the most ops pending (from
the history's rows), max |I| and max |S'| over the unbounded search, and the
class (edge_keys.classify).  The table printed is, per class, the keys
choose() takes in grid order -- the literals of edge_keys.TABLE.  Rerun this
and paste the table when host_synth.cpp changes what a seed produces (the
tests then fail on their preconditions and say so)."""
import argparse
import os
import sys
import time
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "jepsen-etcd-demo_amd"), os.path.join(ROOT, "oracle"), os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import cref  # noqa: E402
import edge_keys as EK  # noqa: E402
from edgegen import pending_before  # noqa: E402
from lincheck import history as H  # noqa: E402
from lincheck.checker import Packed  # noqa: E402

PER_CLASS = 3

# the grids (the issue's, widened where a class needed it)
T1_GRID = [dict(n_keys=3000, ops_per_key=ops, concurrency=conc, anomaly_rate=0.15, seed=seed)
           for seed in range(20, 29) for ops in (40, 60) for conc in (12, 13)]
T2_GRID = [dict(n_keys=300, ops_per_key=ops, concurrency=conc, info_rate=info, anomaly_rate=0.15, seed=seed)
           for ops in (200, 300) for conc in range(11, 17) for info in (0.0, 0.005, 0.01) for seed in range(1, 5)]
HBM_GRID = [dict(n_keys=400, ops_per_key=300, concurrency=16, info_rate=0.01, anomaly_rate=0.15, seed=seed)
            for seed in (1, 2)]
GRIDS = {"t1": T1_GRID, "t2": T2_GRID, "hbm": HBM_GRID}
WANTED = {"t1": ("t1_fit", "t1_over_S", "t1_over_I"), "t2": ("t2_fit", "t2_over_S", "t2_over_I"), "hbm": ("hbm_narrow",)}


def scan(job):
    """One batch: [(kwargs, key, class, max pending, peak, max |I|, valid)] of its edge keys."""
    grid, kw = job
    h = H.synth(**kw)
    order = np.argsort(h.key, kind="stable")
    ks = h.key[order]
    keys, start = np.unique(ks, return_index=True)
    bounds = list(start) + [len(ks)]
    pk = Packed(h)
    at = {k: i for i, k in enumerate(pk.keys)}
    out = []
    for n, k in enumerate(keys.tolist()):
        rows = np.sort(order[bounds[n]:bounds[n + 1]])
        pend = int(pending_before(pk, at[k]).max())
        if grid != "hbm" and pend < EK.LEAVES_REGISTER_TIER:
            continue
        sub = H.History(h.type[rows], h.f[rows], h.process[rows], h.key[rows], h.v0[rows], h.v1[rows], h.index[rows])
        sizeI, sizeS, res = cref.key_sizes(sub.as_c(), k, budget=EK.UNBOUNDED, result=True)
        cls = EK.classify(sizeI, sizeS)
        if cls in WANTED[grid]:
            out.append(((kw, k, cls, pend, int(sizeS.max(initial=1)), int(sizeI.max(initial=1)), int(res.valid)),
                        EK.features(cls, sizeI, sizeS, int(res.valid))))
    return out


def choose(rows):
    """Of one class's keys (row, features) in grid order (hbm_narrow: smallest
    first): those that each add a feature not seen yet (an invalid key, the
    edge met by |S'|, by |I|, exactly or just past), then the next ones up to
    PER_CLASS; a key found again in a longer batch of the same seed is the
    same key and is taken once."""
    seen, same, picked, rest = set(), set(), [], []
    for row, feats in rows:
        kw = row[0]
        ident = (kw["seed"], kw["concurrency"], row[1], row[4], row[5])
        if ident in same:
            continue
        same.add(ident)
        if feats - seen:
            seen |= feats
            picked.append(row)
        else:
            rest.append(row)
    return picked + rest[:max(0, PER_CLASS - len(picked))]


def search(threads):
    jobs = [(g, kw) for g, grid in GRIDS.items() for kw in grid]
    t0 = time.time()
    with Pool(threads) as pool:
        found = [r for rs in pool.map(scan, jobs, chunksize=1) for r in rs]
    table, counts = [], {}
    for cls in [c for g in WANTED.values() for c in g]:
        rows = [r for r in found if r[0][2] == cls]
        counts[cls] = (len(rows), sum(r[0][6] == 0 for r in rows))
        if cls == "hbm_narrow":
            rows.sort(key=lambda r: max(r[0][4], r[0][5]))
        table += choose(rows)
    return table, counts, time.time() - t0, len(jobs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", type=int, default=min(16, os.cpu_count() or 4))
    ap.add_argument("--check", action="store_true", help="fail unless the table found equals edge_keys.TABLE")
    a = ap.parse_args()
    table, counts, dt, nb = search(a.threads)
    print(f"# {nb} batches searched in {dt:.1f} s on {a.threads} processes; keys found (invalid among them):")
    for cls, (n, nbad) in counts.items():
        print(f"#   {cls}: {n} ({nbad})")
    print("TABLE = [")
    print("    # (synth kwargs, key, class, most pending, peak = max |S'|, max |I|, valid)")
    for kw, k, cls, pend, peak, maxI, valid in table:
        print(f"    ({kw!r}, {k}, {cls!r}, {pend}, {peak}, {maxI}, {valid}),")
    print("]")
    if a.check:
        want = [tuple(r) for r in EK.TABLE]
        if [tuple(r) for r in table] != want:
            print("the table found differs from tests/edge_keys.py TABLE", file=sys.stderr)
            return 1
        print("# equal to tests/edge_keys.py TABLE")
    return 0


if __name__ == "__main__":
    sys.exit(main())
