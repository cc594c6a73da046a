#!/usr/bin/env python3
"""Writes tests/golden/perf_demo_history.edn: a history of the demo's shape
for the perf tests (tests/test_gpu_perf.py, tests/test_perf_edn.py).

About 600 rows over 32 s, as the register workload logs them (etcdemo.clj:
83-105, :120-125): five clients issuing :read / :write / :cas on independent
tuples [k v] at about 10 ops a second with a few ms of latency, some :fail
(cas) and :info (timeouts, after which the client comes back as process + 5),
and the nemesis's :start / :stop every 5 s, each logged twice.  Rows are in
log order, which is not quite time order: a completion is logged with a clock
read before the row ahead of it.  Deterministic: running it again writes the
same bytes."""
import os
import random

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "perf_demo_history.edn")
S, MS = 10**9, 10**6


def main():
    rng = random.Random(20260119)
    rows = []  # (log position, text)
    proc = list(range(5))
    for c in range(5):
        t = rng.randrange(100 * MS)
        while t < 32 * S:
            f = rng.choice(["read", "write", "cas"])
            k = rng.randrange(3)
            v = {"read": "nil", "write": str(rng.randrange(5)), "cas": "[%d %d]" % (rng.randrange(5), rng.randrange(5))}[f]
            rows.append((t, "{:type :invoke, :f :%s, :value [%d %s], :time %d, :process %d}" % (f, k, v, t, proc[c])))
            r = rng.random()
            if r < 0.04:  # timeout: :info after 5 s, the process is replaced
                done = t + 5 * S
                rows.append((done, "{:type :info, :f :%s, :value [%d %s], :time %d, :process %d, :error :timeout}"
                             % (f, k, v, done, proc[c])))
                proc[c] += 5
            else:
                lat = int(rng.lognormvariate(1.2, 0.8) * MS)
                done = t + lat
                typ = "fail" if f == "cas" and r < 0.5 else "ok"
                if f == "read" and typ == "ok":
                    v = str(rng.randrange(5))
                # the row is logged a little after its clock was read
                done_log = done + rng.randrange(3 * MS)
                rows.append((done_log, "{:type :%s, :f :%s, :value [%d %s], :time %d, :process %d}"
                             % (typ, f, k, v, done, proc[c])))
                done = done_log
            t = done + int(rng.expovariate(1 / (370 * MS)))
    for i, t in enumerate(range(5 * S, 32 * S, 5 * S)):
        f = "start" if i % 2 == 0 else "stop"
        for j in range(2):
            tt = t + j * 40 * MS
            rows.append((tt, "{:type :info, :f :%s, :value nil, :time %d, :process :nemesis}" % (f, tt)))
    rows.sort(key=lambda r: r[0])
    with open(OUT, "w") as out:
        for i, (_, text) in enumerate(rows):
            out.write(text[:-1] + ", :index %d}\n" % i)
    print(f"{len(rows)} rows -> {os.path.normpath(OUT)}")


if __name__ == "__main__":
    main()
