"""plan_lane (csrc/lane_plan.hpp): where an enqueued node step of
lc_check_node_async runs -- its search lane, whether it may overlap the step
before it, how its records reach the caller's buffer, its staging slot.  The
records are the same on every path, so the choice is pinned here, on the CPU,
through tests/lane_plan_main.cpp (host C++ only, no HIP)."""
import os
import shutil
import subprocess

import pytest

from lincheck import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/llvm/bin/clang++"

pytestmark = pytest.mark.skipif(not shutil.which(CXX), reason="no ROCm clang++")

OUT_FIELDS = "lane overlap direct after slot slot_waits".split()
# an enqueued speculative-segment step of C2's size (1,000 keys x 8 segments on 256 CUs x 32 waves), no
# communicator, a device-mapped buffer
BASE = dict(seq=0, run_n=0, async_=1, spec=1, split=0, comm=0, mapped=1, path_flags=0, waves=8000, resident_waves=8192,
            lo=4096, hi=8192, flight=())
# what keeps a step on lane 0, in today's single-stream order
SERIAL = {"LC_PATH_NODE_SERIAL": dict(path_flags=N.LC_PATH_NODE_SERIAL),
          "a communicator": dict(comm=1),
          "a split step": dict(split=1, spec=0),
          "a split step (whatever spec says)": dict(split=1),
          "a lattice step": dict(spec=0),
          "a synchronous step": dict(async_=0),
          "more than one resident round": dict(waves=8193),
          "a C3 shard": dict(waves=25000)}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("lane_plan") / "lane_plan_main")
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "jepsen-etcd-demo_amd", "csrc"),
                    os.path.join(ROOT, "tests", "lane_plan_main.cpp"), "-o", path], check=True, timeout=120)
    return path


def plans(exe, rows):
    """plan_lane of every row (BASE with the row's changes)."""
    text = ""
    for delta in rows:
        r = dict(BASE, **delta)
        f = [r["seq"], r["run_n"], r["async_"], r["spec"], r["split"], r["comm"], r["mapped"], r["path_flags"],
             r["waves"], r["resident_waves"], r["lo"], r["hi"], len(r["flight"])]
        for tri in r["flight"]:
            f += list(tri)
        text += " ".join(str(int(v)) for v in f) + "\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True, timeout=60)
    lines = out.stdout.strip().splitlines()
    assert lines[0].split() == ["2", "3", "2"]  # lanes, staging slots, steps in flight beside a new one
    assert len(lines) == len(rows) + 1
    return [dict(zip(OUT_FIELDS, map(int, line.split()))) for line in lines[1:]]


def test_lanes_alternate_for_overlapping_steps(exe):
    got = plans(exe, [dict(seq=7 + n, run_n=n) for n in range(8)])
    assert [p["lane"] for p in got] == [0, 1, 0, 1, 0, 1, 0, 1]
    assert all(p["overlap"] == 1 for p in got)
    # exactly one resident round, and small launches
    got = plans(exe, [dict(run_n=1, waves=w) for w in (8192, 600, 1)])
    assert all(p["lane"] == 1 and p["overlap"] == 1 for p in got)


@pytest.mark.parametrize("why", list(SERIAL))
def test_single_lane_steps(exe, why):
    """Lane 0 and no overlap, whatever the step's turn; the records keep the
    single-stream rule (in place when the buffer is device-mapped and there
    is no communicator), in-flight steps on the same buffer or not."""
    rows = [dict(SERIAL[why], seq=n, run_n=n, flight=fl) for n in range(6) for fl in ((), ((n + 9, 0, 1 << 20),))]
    got = plans(exe, rows)
    assert all(p["lane"] == 0 and p["overlap"] == 0 and p["after"] == -1 for p in got), got
    assert all(p["direct"] == (0 if why == "a communicator" else 1) for p in got), got
    staged = plans(exe, [dict(SERIAL[why], mapped=0), dict(SERIAL[why], path_flags=N.LC_PATH_NODE_STAGED |
                                                          SERIAL[why].get("path_flags", 0))])
    assert all(p["direct"] == 0 and p["after"] == -1 and p["overlap"] == 0 for p in staged)


def test_records_direct_or_ordered(exe):
    own = dict(lo=1000, hi=2000)
    rows = [
        dict(own),                                                  # nothing in flight
        dict(own, flight=((5, 2000, 3000),)),                       # disjoint: ends where the other begins
        dict(own, flight=((5, 0, 1000),)),                          # disjoint: begins where the other ends
        dict(own, flight=((5, 1999, 3000),)),                       # one byte shared
        dict(own, flight=((5, 0, 1001),)),
        dict(own, flight=((5, 1000, 2000),)),                       # the same buffer
        dict(own, flight=((5, 1000, 2000), (6, 1500, 1600))),       # two: behind the later one
        dict(own, flight=((6, 1500, 1600), (5, 1000, 2000))),
        dict(own, flight=((5, 1000, 2000), (6, 4000, 5000))),       # only the earlier overlaps
        dict(own, flight=((0, 1000, 2000),)),                       # step 0 is a step too
        dict(own, mapped=0),                                        # not device-mapped: staged, no order needed
        dict(own, mapped=0, flight=((5, 1000, 2000),)),
        dict(own, path_flags=N.LC_PATH_NODE_STAGED),
        dict(own, path_flags=N.LC_PATH_NODE_STAGED, flight=((5, 1500, 2500),)),
    ]
    got = [(p["direct"], p["after"]) for p in plans(exe, rows)]
    assert got == [(1, -1), (1, -1), (1, -1), (0, 5), (0, 5), (0, 5), (0, 6), (0, 6), (0, 5), (0, 0),
                   (0, -1), (0, 5), (0, -1), (0, 5)]
    assert all(p["overlap"] == 1 for p in plans(exe, rows))


def test_slot_waits_for_the_step_three_back(exe):
    got = plans(exe, [dict(seq=n, run_n=n % 5) for n in range(64)])
    assert [p["slot"] for p in got] == [n % 3 for n in range(64)]
    assert [p["slot_waits"] for p in got] == [n - 3 if n >= 3 else -1 for n in range(64)]
    # whatever else the step is
    other = plans(exe, [dict(v, seq=n) for n in range(12) for v in SERIAL.values()])
    assert [p["slot"] for p in other] == [n % 3 for n in range(12) for _ in SERIAL]


@pytest.mark.parametrize("seed", range(4))
def test_at_most_three_steps_in_flight(exe, seed):
    """64 steps of any kind in any order: a step is enqueued once the step
    its slot waits for has ended (and others may have ended on their own), so
    never more than three are in flight, they are the newest three, no two
    of them share a slot, and overlapping steps take the lanes in turn from
    lane 0 after every step that does not overlap."""
    import random
    rng = random.Random(seed)
    kinds = [dict()] * 6 + list(SERIAL.values())
    live, run_n = {}, 0
    for n in range(64):
        kind = dict(rng.choice(kinds)) if seed else {}
        p = plans(exe, [dict(kind, seq=n, run_n=run_n)])[0]
        if p["slot_waits"] >= 0:
            live.pop(p["slot_waits"], None)
        for m in [m for m in live if rng.random() < 0.3]:  # some steps end on their own
            del live[m]
        assert p["slot"] not in {q["slot"] for q in live.values()}
        live[n] = p
        assert len(live) <= 3
        assert all(m >= n - 2 for m in live)
        run_n = run_n + 1 if p["overlap"] else 0
        if p["overlap"]:
            assert p["lane"] == (run_n - 1) % 2


def test_flags_are_mirrored():
    hdr = open(os.path.join(ROOT, "include", "lincheck.h")).read()
    assert "#define LC_PATH_NODE_SERIAL  0x10000" in hdr and N.LC_PATH_NODE_SERIAL == 0x10000
    assert "#define LC_PATH_ALL          0x1FFFF" in hdr
    assert "#define LC_ABI_VERSION 13" in hdr


def test_header_is_host_only():
    """lane_plan.hpp stays free of HIP: the rules compile (and are tested)
    with a plain host compiler."""
    src = open(os.path.join(ROOT, "jepsen-etcd-demo_amd", "csrc", "lane_plan.hpp")).read()
    includes = [line.split()[1] for line in src.splitlines() if line.startswith("#include")]
    assert includes == ["<cstdint>", '"../../include/lincheck.h"']
