#!/usr/bin/env python3
"""Look for a budget edge inside a stream's resident set tier that |S'| decides
(CPU only; cref.key_sizes decides everything), for
tests/test_gpu_stream_set_exact.py: a key that leaves the register tier at
event defer_at (stream_helpers.Restated), whose least deciding budget `need`
is first reached -- at an :ok past defer_at -- by |S'| while |I| at that :ok is
still below it, with need at most the set tier's cap.

    python tests/tools/find_set_tier_s_edges.py [--seconds 60]

Scans lincheck.history.synth batches of the shapes the stream tests use (10
clients per key, crashed ops) and tests/edgegen.py plans with a crashed write,
and prints every hit as a literal: (synth arguments, key, defer_at, need,
event).  The |I| edges it meets on the way are counted, not listed."""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "jepsen-etcd-demo_amd"), os.path.join(ROOT, "oracle"), os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import cref  # noqa: E402
import edgegen as E  # noqa: E402
import stream_helpers as S  # noqa: E402
from lincheck import history as H  # noqa: E402

CAP = 32768

SYNTH_GRID = [dict(n_keys=60, ops_per_key=ops, concurrency=conc, info_rate=info, anomaly_rate=0.2, seed=seed)
              for seed in range(1, 40) for ops in (150, 300) for conc in (10, 11, 12) for info in (0.02, 0.05)]


def edgegen_batches():
    for seed in range(1, 20):
        plans = [(f"crash-{n}-{c}", E.Plan(n, E.counts(n, 11, drain=True, stuck=1), crash={2: c}, kinds={2: "write"},
                                           apply_at={2: n - 11}, distinct={2: 1}))
                 for n in (61, 81) for c in (10, 14, 20)]
        yield f"edgegen seed {seed}", E.batch(plans, seed=seed).hist


def scan(label, h, hits, counts, deadline):
    rs = S.Restated(h)
    for k in rs.keys:
        d = rs.defer_at[k]
        if d < 0 or k in rs.error:
            continue
        if time.time() > deadline:
            return False
        hk = h.select_keys([k]).as_c()
        sI, sS, rec = cref.key_sizes(hk, k, budget=CAP, result=True)  # (a set past the cap: no edge inside the tier)
        need = int(max(sI.max(initial=1), sS.max(initial=1)))
        if need <= 1 or int(rec.cause) == 2:
            continue
        e = int(np.flatnonzero((sI > need - 1) | (sS > need - 1))[0])
        if e <= d:
            counts["before"] += 1
        elif sI[e] > need - 1:
            counts["by_I"] += 1
        else:
            hits.append((label, k, d, need, e, int(sI[e]), int(sS[e])))
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    a = ap.parse_args()
    t0 = time.time()
    hits, counts, scanned = [], {"before": 0, "by_I": 0}, 0
    jobs = [(repr(kw), lambda kw=kw: H.synth(**kw)) for kw in SYNTH_GRID[:8]]
    jobs += [(label, lambda h=h: h) for label, h in edgegen_batches()]
    jobs += [(repr(kw), lambda kw=kw: H.synth(**kw)) for kw in SYNTH_GRID[8:]]
    for label, make in jobs:
        if time.time() - t0 > a.seconds or not scan(label, make(), hits, counts, t0 + a.seconds):
            break
        scanned += 1
    print(f"{scanned} batches in {time.time() - t0:.0f} s: {counts['by_I']} edges inside the set tier decided by |I|, "
          f"{counts['before']} keys decided before they leave, {len(hits)} decided by |S'|")
    for hit in hits:
        print("  (batch, key, defer_at, need, event, |I|, |S'|) =", hit)
    return 0


if __name__ == "__main__":
    sys.exit(main())
