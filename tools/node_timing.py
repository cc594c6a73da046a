"""The bench's D-1 step on the C2 batch, two ways:

* default: the breakdown of lc_check_node -- LC_TIMING=1 makes the library
  print prepare / upload / enqueue / wait times;
* --pipelined: lc_check_node_async, A/B of the two search lanes (default)
  against LC_PATH_NODE_SERIAL (one search at a time), 200 steps into one
  buffer per arm, arms alternating; ms per step per run and the records
  compared.  --noprio adds LC_PATH_SPEC_NOPRIO to both arms (overlapping
  steps walk by wave age anyway, so it changes the serial arm)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "jepsen-etcd-demo_amd"))

ap = argparse.ArgumentParser()
ap.add_argument("--pipelined", action="store_true")
ap.add_argument("--noprio", action="store_true")
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--runs", type=int, default=5)
args = ap.parse_args()
if not args.pipelined:
    os.environ["LC_TIMING"] = "1"

import numpy as np  # noqa: E402

from lincheck import _native as N  # noqa: E402
from lincheck import history as H  # noqa: E402
from lincheck.checker import Device, Packed, PinnedRecords  # noqa: E402

h = H.synth(n_keys=1000, ops_per_key=1000, concurrency=10, seed=2)
pk = Packed(h)
K = pk.n_keys

if not args.pipelined:
    dev = Device(0)
    for i in range(8):
        t = time.perf_counter()
        _, st = dev.check_node(pk, K)
        print(f"call {i}: wall {(time.perf_counter() - t) * 1e3:.3f} ms", file=sys.stderr, flush=True)
    sys.exit(0)

extra = N.LC_PATH_SPEC_NOPRIO if args.noprio else 0
arms = {"lanes": Device(0, path_flags=extra), "serial": Device(0, path_flags=extra | N.LC_PATH_NODE_SERIAL)}
bufs = {a: PinnedRecords(K) for a in arms}
ms = {a: [] for a in arms}
for a, dev in arms.items():  # warm-up: allocations, first uploads
    for _ in range(5):
        dev.check_node_async(pk, K, bufs[a])
    dev.wait()
for _ in range(args.runs):
    for a, dev in arms.items():
        t = time.perf_counter()
        for _ in range(args.steps):
            dev.check_node_async(pk, K, bufs[a])
        n, span = dev.wait()
        ms[a].append((time.perf_counter() - t) * 1e3 / args.steps)
        assert n == args.steps
ref = Device(0).check_node(pk, K)[0]
out = {"steps": args.steps, "noprio": args.noprio,
       "same_records": bool(np.array_equal(bufs["lanes"], bufs["serial"]) and np.array_equal(bufs["lanes"], ref))}
for a in arms:
    out[a] = {"ms_per_step": [round(x, 4) for x in ms[a]], "median": round(float(np.median(ms[a])), 4)}
out["speedup"] = round(out["serial"]["median"] / out["lanes"]["median"], 3)
print(json.dumps(out))
