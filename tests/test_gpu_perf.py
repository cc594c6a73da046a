"""lc_perf_check on the GPU: every case compares the whole result (rate counts,
group counts, every quantile of every non-empty group) with the restatement
of DESIGN.md section 3.10 in tests/perf_helpers.py, on three paths: the
library's own choice, every group through the HBM select
(LC_PERF_SELECT_HBM), and the count and scatter kernels without their LDS
tile (LC_PERF_COUNT_DIRECT)."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import perf_helpers as PH
from lincheck import _native as N
from lincheck import checker as ck
from lincheck import perf as P

pytestmark = pytest.mark.gpu

PATHS = {"auto": 0, "hbm": N.LC_PERF_SELECT_HBM, "direct": N.LC_PERF_COUNT_DIRECT}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "perf_demo_history.edn")


@pytest.fixture(scope="module")
def dev(device):
    return ck.Device(0)


@pytest.fixture(scope="module")
def info():
    out = np.zeros(4, np.int64)
    N.check(N.lib().lc_perf_launch_info(N.ptr(out, C.c_int64)))
    return dict(zip("wg tile lds digit".split(), out.tolist()))


def agree(dev, ops, opts=None, hist=None):
    """The device's tables equal the restatement's on every path."""
    want = PH.restate(ops, opts)
    hist = hist if hist is not None else P.PerfHistory.from_ops(ops)
    packed = P.PackedPerf(hist)
    assert (packed.matched, packed.unmatched, packed.orphans) == (want["matched"], want["unmatched"], want["orphans"])
    assert [tuple(x) for x in packed.intervals.tolist()] == want["nemesis"]
    for path, flags in PATHS.items():
        res = P.check_batch(dev, packed.view, P.make_opts(dict(opts or {}, flags=flags)))
        got = PH.tables(packed.names, res)
        for part in ("rate", "groups", "quantiles"):
            assert got[part] == want[part], (path, part)
    return want


def test_hand_example(dev):
    ops = PH.hand_ops()
    want = agree(dev, ops)
    for k, v in PH.HAND_WANT.items():
        assert want[k] == v, k
    s = P.analyze(dev, ops)
    assert s.quantiles["read"][1.0] == [(15.0, 2.0)] and s.rate["write"]["info"] == [(45.0, 0.1)]
    assert s.nemesis == [(3.0, 31.0), (43.0, 43.0)] and s.points("read", "ok") == [(1.0, 5.0), (5.0, 2.0)]


def test_random_history(dev):
    """4,000 rows, 3 :f, all completion types, times jittered out of order,
    crashed ops, orphans, nemesis rows; about 50 quantile and 150 rate buckets."""
    ops = PH.random_ops(random.Random(5), 4000, t0=-20000)
    span = max(o["time"] for o in ops) - min(o["time"] for o in ops)
    opts = {"quantile-dt-ns": span // 50, "rate-dt-ns": span // 150}
    want = agree(dev, ops, opts)
    assert want["orphans"] and want["unmatched"] and want["nemesis"]
    assert {t for _, t, _ in want["rate"]} == {"ok", "fail", "info"} and len({f for f, _ in want["groups"]}) == 3
    assert 45 <= len({b for _, b in want["groups"]}) <= 52 and min(o["time"] for o in ops) < 0


def test_quantile_rule_every_n(dev):
    """One group of n points for every n in 1..256.  By bucket: random points;
    equal times with distinct latencies; latency falling as time rises (a sort
    by latency alone picks other points); few distinct values (ties across the
    selected indices in both columns)."""
    rng = random.Random(9)
    dt = 1000
    ops = []
    for b in range(256):
        n, base = b + 1, (b + 7) * dt
        if b % 4 == 0:
            pts = [(base + rng.randrange(dt), rng.randrange(1, 10**6)) for _ in range(n)]
        elif b % 4 == 1:
            pts = [(base + 500, v) for v in rng.sample(range(1, 10**6), n)]
        elif b % 4 == 2:
            xs = sorted(rng.randrange(dt) for _ in range(n))
            pts = [(base + x, 10**6 - 100 * x - i) for i, x in enumerate(xs)]
        else:
            pts = [(base + rng.choice([0, 1, 999]), rng.choice([3, 4, 4, 5])) for _ in range(n)]
        rng.shuffle(pts)
        ops += PH.pairs_ops(pts, f=("read", "write")[b % 2])
    want = agree(dev, ops, {"quantile-dt-ns": dt, "rate-dt-ns": 64 * dt})
    assert sorted(want["groups"].values()) == list(range(1, 257))
    # the cases do separate the orderings: by latency alone some group answers differently
    pts_of = {}
    for f, _, x, lat in want["points"]:
        pts_of.setdefault((f, x // dt), []).append(lat)
    assert any(sorted(v)[min(len(v) - 1, int(len(v) * 0.5))] != want["quantiles"][g][0] for g, v in pts_of.items())


DIGIT_LATS = [-2**40, -1, 0, 1, 2**8 - 1, 2**8, 2**32 - 1, 2**32, 2**40, 2**62]


@pytest.mark.parametrize("lats", [DIGIT_LATS, DIGIT_LATS[1:6], [0]], ids=["all", "low", "zero"])
def test_digits(dev, lats):
    """Latencies from values that differ in every digit of the HBM select's key
    and in sign; with [0] every digit pass above the lowest is skipped."""
    rng = random.Random(11)
    dt = 2**20
    ops = []
    for b in range(6):
        pts = [((b + 2) * dt + rng.randrange(4), rng.choice(lats)) for _ in range(40 + 13 * b)]
        ops += PH.pairs_ops(pts, f="cas", process=b)
    want = agree(dev, ops, {"quantile-dt-ns": dt, "rate-dt-ns": 2**62, "quantiles": [0.0, 0.3, 0.5, 0.7, 0.9, 1.0]})
    if len(lats) > 5:
        assert len({v for q in want["quantiles"].values() for v in q}) >= 5


def test_lds_select_limit(dev, info):
    """Groups of L - 1, L and L + 1 points around the LDS select's limit."""
    rng = random.Random(13)
    L, dt = info["lds"], 10**6
    ops = []
    for i, n in enumerate((L - 1, L, L + 1)):
        pts = [(i * dt + rng.randrange(dt), rng.randrange(-50, 10**5)) for _ in range(n)]
        ops += PH.pairs_ops(pts, process=i)
    want = agree(dev, ops, {"quantile-dt-ns": dt, "rate-dt-ns": dt})
    assert sorted(want["groups"].values()) == [L - 1, L, L + 1]


def test_workgroup_record_counts(dev, info):
    """W - 1, W, W + 1 and 2 W + 1 records around the streaming kernels'
    workgroup size (the last lane's partial load, the second workgroup)."""
    rng = random.Random(17)
    W = info["wg"]
    for n in (W - 1, W, W + 1, 2 * W + 1):
        pts = [(i * 10 + rng.randrange(10), rng.randrange(1, 500)) for i in range(n)]
        agree(dev, PH.pairs_ops(pts), {"quantile-dt-ns": 4000, "rate-dt-ns": 1500})


def test_tile_span_reverse_order(dev, info):
    """One workgroup whose records span one bucket more than the LDS tile, in
    reverse time order: the first records are outside the tile."""
    W, T = info["wg"], info["tile"]
    dt = 1000
    pts = [(((T + 1) * dt * (W - 1 - i)) // W + 5 * dt, 1 + i % 7) for i in range(W)]
    want = agree(dev, PH.pairs_ops(pts), {"quantile-dt-ns": dt, "rate-dt-ns": dt})
    assert len(want["groups"]) == T + 1


def test_bucket_boundaries(dev):
    """Times at k dt - 1, k dt and k dt + 1 ns for both widths; the first
    bucket is not bucket 0, and negative times floor."""
    qdt, rdt = 3000, 1000
    for k0 in (4, -3):
        pts = []
        for k in range(k0, k0 + 3):
            for dt in (qdt, rdt):
                pts += [(k * dt + e, 50 + e) for e in (-1, 0, 1)]
        # the same instants as completion times (the rate's clock): latency 7
        ops = PH.pairs_ops(pts) + PH.pairs_ops([(x - 7, 7) for x, _ in pts], f="write", process=1)
        want = agree(dev, ops, {"quantile-dt-ns": qdt, "rate-dt-ns": rdt})
        assert min(b for _, b in want["groups"]) == (min(x for x, _ in pts) - 7) // qdt != 0


def test_max_f(dev):
    for nf in (1, N.LC_PERF_MAX_F):
        ops = []
        for i in range(nf):
            ops += PH.pairs_ops([(100 * i + j, 1 + i + j) for j in range(3)], f=f"f{i}", process=i)
        want = agree(dev, ops, {"quantile-dt-ns": 1000, "rate-dt-ns": 500})
        assert len({f for f, _ in want["groups"]}) == nf
    ops = [PH.op("invoke", f"f{i}", 0, i) for i in range(N.LC_PERF_MAX_F + 1)]
    with pytest.raises(N.LincheckError, match="unsupported") as e:
        P.analyze(dev, ops)
    assert e.value.code == -5 and "33" in str(e.value)


def test_malformed_input_is_refused_on_the_host(dev):
    hist = P.PerfHistory.from_ops(PH.hand_ops())
    for col, bad in (("type", 4), ("f", len(hist.names))):
        h = P.PerfHistory(hist.type.copy(), hist.f.copy(), hist.process, hist.time, hist.names)
        getattr(h, col)[2] = bad
        with pytest.raises(N.LincheckError, match="invalid"):
            P.PackedPerf(h)
    for key in ("quantile-dt-ns", "rate-dt-ns"):
        for bad in (0, -5):
            with pytest.raises(N.LincheckError, match="invalid"):
                P.analyze(dev, PH.hand_ops(), {key: bad})


def test_empty_histories(dev):
    for ops in ([], [PH.op("info", "start", "nemesis", 5), PH.op("info", "stop", "nemesis", 9)]):
        s = P.analyze(dev, ops)
        assert s.quantiles == {} and s.rate == {}
        assert s.nemesis == ([(5e-9, 9e-9)] if ops else [])
        assert ck.perf().check({}, ops, {}) == {"valid?": True}


def test_read_edn_demo_shape(dev):
    """A history of the demo's shape from tests/golden (tools/gen_perf_fixture.py)
    through lc_edn_read_perf, with Jepsen's own widths."""
    hist = P.PerfHistory.read_edn(GOLDEN)
    ops = hist.to_ops()
    assert 500 <= len(ops) <= 800 and {"read", "write", "cas", "start", "stop"} <= set(hist.names)
    want = agree(dev, ops, None, hist)
    assert want["matched"] > 200 and len({b for _, _, b in want["rate"]}) >= 3 and want["nemesis"]


def test_compose_mirrors_the_demo_for_both_workloads(dev, tmp_path):
    """checker/compose {:perf (checker/perf) :indep (:checker workload)}
    (etcdemo.clj:165-167) over op maps that carry :process, :time and
    independent tuples: register workload, then set workload."""
    from lincheck import independent, model
    T = independent.tuple_

    def rows(spec):
        return [dict(PH.op(ty, f, p, t * PH.S), value=v, index=i) for i, (ty, f, p, t, v) in enumerate(spec)]
    register = rows([("invoke", "write", 0, 1, T(7, 3)), ("ok", "write", 0, 2, T(7, 3)),
                     ("info", "start", "nemesis", 2, None), ("invoke", "read", 1, 3, T(7, None)),
                     ("ok", "read", 1, 4, T(7, 3)), ("info", "stop", "nemesis", 5, None),
                     ("invoke", "read", 0, 6, T(8, None)), ("ok", "read", 0, 8, T(8, 5))])  # key 8 reads 5, never written
    lin = ck.linearizable({"model": model.cas_register(), "algorithm": "linear"})
    test = {"store-path": str(tmp_path)}
    r = ck.compose({"perf": ck.perf(), "indep": independent.checker(lin)}).check(test, register, {})
    assert r["perf"] == {"valid?": True} and r["indep"]["failures"] == [8] and r["valid?"] is False
    assert open(tmp_path / "rate.tsv").read().splitlines() == ["write ok\t5.0\t0.1", "read ok\t5.0\t0.2"]
    sets = rows([("invoke", "add", 0, 1, 0), ("ok", "add", 0, 2, 0), ("invoke", "add", 1, 3, 1), ("info", "add", 1, 9, 1),
                 ("invoke", "read", 0, 10, None), ("ok", "read", 0, 12, [0, 1])])
    r = ck.compose({"perf": ck.perf(), "indep": ck.set_()}).check({}, sets, {})
    assert r["perf"] == {"valid?": True} and r["indep"]["valid?"] is True and r["indep"]["recovered-count"] == 1
    assert r["valid?"] is True
