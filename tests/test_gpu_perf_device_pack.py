"""lc_perf_check_history on the GPU: every case compares the device path field
by field and array by array with lc_perf_pack followed by lc_perf_check on the
same history -- the batch's counts and bounds, the record columns (through
lc_perf_checked_records), the info numbers, the intervals and the three tables
-- and, where the history is op maps, with the restatement of DESIGN.md
section 3.10 in tests/perf_helpers.py.  Every case runs on the three paths of
tests/test_gpu_perf.py: the library's own choice, every group through the HBM
select, and the count and scatter kernels without their LDS tile."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import counter_pack_helpers as CPH
import perf_helpers as PH
from lincheck import _native as N
from lincheck import checker as ck
from lincheck import perf as P

pytestmark = pytest.mark.gpu

PATHS = {"auto": 0, "hbm": N.LC_PERF_SELECT_HBM, "direct": N.LC_PERF_COUNT_DIRECT}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "perf_demo_history.edn")
I64_MIN, I64_MAX = -2**63, 2**63 - 1
NARROW = {"quantile-dt-ns": 100000, "rate-dt-ns": 30000}
SIZES = ("n", "n_matched", "t_min", "t_max", "x_min", "x_max", "n_f")


@pytest.fixture(scope="module")
def dev(device):
    return ck.Device(0)


def same(dev, ops=None, opts=None, hist=None):
    """The device path equals the host path in every field, on every path; with
    op maps at hand both equal the restatement.  Returns the last device object."""
    hist = hist if hist is not None else P.PerfHistory.from_ops(ops)
    packed = P.PackedPerf(hist)
    want_a = packed.arrays()
    want = PH.restate(ops, opts) if ops is not None else None
    for path, flags in PATHS.items():
        o = P.make_opts(dict(opts or {}, flags=flags))
        c = P.CheckedPerf(dev, hist, o)
        got_a = c.arrays()  # (before lc_perf_check takes the device's record columns)
        res = P.check_batch(dev, packed.view, o)
        for k in SIZES:
            assert getattr(c.view, k) == getattr(packed.view, k), (path, k)
        assert not c.view.t_comp and not c.view.t_inv and not c.view.meta
        for k in ("t_comp", "t_inv", "meta"):
            assert np.array_equal(got_a[k], want_a[k]), (path, k)
        assert (c.matched, c.unmatched, c.orphans) == (packed.matched, packed.unmatched, packed.orphans), path
        assert np.array_equal(c.intervals, packed.intervals), path
        r = c.results
        assert (r.rate_first, r.q_first) == (res.rate_first, res.q_first), path
        for k in ("rate", "group", "quant"):
            g, w = getattr(r, k), getattr(res, k)
            assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w), (path, k)
        if want is not None:
            got = PH.tables(c.names, r)
            for part in ("rate", "groups", "quantiles"):
                assert got[part] == want[part], (path, part)
            assert (c.matched, c.unmatched, c.orphans) == (want["matched"], want["unmatched"], want["orphans"])
            assert [tuple(x) for x in c.intervals.tolist()] == want["nemesis"]
    return c


def same_error(dev, hist, code, row=None, opts=None):
    """Both paths refuse the history with the same code and, but for the
    function's name, the same words."""
    with pytest.raises(N.LincheckError) as eh:
        P.check_batch(dev, P.PackedPerf(hist).view, P.make_opts(opts))
    with pytest.raises(N.LincheckError) as ed:
        P.CheckedPerf(dev, hist, P.make_opts(opts))
    assert ed.value.code == eh.value.code == code
    words = [str(e.value).replace("lc_perf_check_history:", "").replace("lc_perf_pack:", "") for e in (ed, eh)]
    assert words[0] == words[1], words
    if row is not None:
        assert f"row {row}:" in words[0], words
    return words[0]


def test_hand_example(dev):
    ops = PH.hand_ops()
    c = same(dev, ops)
    want = PH.restate(ops)
    for k, v in PH.HAND_WANT.items():
        assert want[k] == v, k
    assert (c.matched, c.unmatched, c.orphans) == (4, 2, 1) and c.intervals.tolist() == [[3 * PH.S, 31 * PH.S], [43 * PH.S, 43 * PH.S]]
    s = P.analyze(dev, ops, {"pack": "device"})
    assert s.quantiles["read"][1.0] == [(15.0, 2.0)] and s.rate["write"]["info"] == [(45.0, 0.1)]
    assert s.nemesis == [(3.0, 31.0), (43.0, 43.0)] and s.points("read", "ok") == [(1.0, 5.0), (5.0, 2.0)]


def test_random_history(dev):
    ops = PH.random_ops(random.Random(5), 4000, t0=-20000)
    span = max(o["time"] for o in ops) - min(o["time"] for o in ops)
    c = same(dev, ops, {"quantile-dt-ns": span // 50, "rate-dt-ns": span // 150})
    assert c.orphans and c.unmatched and len(c.intervals) and c.matched > 1000


@pytest.fixture(scope="module")
def long_ops():
    return PH.random_ops(random.Random(7), 4097, procs=8)


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 2047, 2048, 2049, 4096, 4097])
def test_workgroup_and_scan_tile_edges(dev, long_ops, n):
    """Prefixes around the workgroup (256 rows) and the scan's tile (2,048)."""
    info = (C.c_int64 * 3)()
    assert N.lib().lc_perf_pack_launch_info(info) == 0 and list(info)[:2] == [256, 2048]
    same(dev, long_ops[:n], NARROW)


def test_one_process(dev):
    c = same(dev, PH.random_ops(random.Random(21), 1500, procs=1), NARROW)
    assert c.matched > 500


def test_every_row_a_process_of_its_own(dev):
    """3,000 rows: every invocation is unmatched, every completion an orphan."""
    ops = [dict(o, process=i) for i, o in enumerate(PH.random_ops(random.Random(22), 3000, nemesis_every=0))]
    c = same(dev, ops, NARROW)
    n_inv = sum(o["type"] == "invoke" for o in ops)
    assert (c.matched, c.unmatched, c.orphans) == (0, n_inv, 3000 - n_inv) and c.orphans > 1000


def test_three_hundred_processes(dev):
    c = same(dev, PH.random_ops(random.Random(23), 5000, procs=300), NARROW)
    assert c.matched > 1000 and c.unmatched > 100


def test_process_ids_that_straddle_the_flat_table_and_collide_in_low_bits(dev):
    ids = [-5, 0, 65535, 65536, 2**40, 2**62, I64_MAX]
    ops = [dict(o, process=ids[o["process"]]) if PH.is_client(o) else o
           for o in PH.random_ops(random.Random(24), 2000, procs=len(ids))]
    assert {o["process"] for o in ops if PH.is_client(o)} == set(ids)
    c = same(dev, ops, NARROW)
    assert c.matched > 500


def nem(f, t):
    return PH.op("info", f, "nemesis", t)


def test_only_nemesis_rows(dev):
    """No record: the tables are as the host path leaves them."""
    for fs in (["start", "stop", "start"], ["stop"], ["kill", "kill"], ["start"] * 700 + ["stop"] * 700 + ["start", "stop"] * 400):
        c = same(dev, [nem(f, 10 * i + 3) for i, f in enumerate(fs)])
        assert c.n == 0 and c.results.rate.size == 0 and c.results.group.size == 0 and c.arrays()["t_comp"].size == 0


def test_only_invocations_and_only_orphans(dev):
    c = same(dev, [PH.op("invoke", "read", i % 5, 100 * i) for i in range(600)], NARROW)
    assert (c.n, c.matched, c.unmatched, c.orphans) == (0, 0, 600, 0)
    c = same(dev, [PH.op(("ok", "fail", "info")[i % 3], ("read", "write")[i % 2], i % 5, 100 * i) for i in range(600)], NARROW)
    assert (c.n, c.matched, c.unmatched, c.orphans) == (600, 0, 0, 600) and c.results.group.size == 0


def test_no_nemesis_row_and_no_start_or_stop_name(dev):
    c = same(dev, PH.random_ops(random.Random(25), 900, nemesis_every=0), NARROW)
    assert len(c.intervals) == 0 and c.hist.f_id("start") == -1
    ops = PH.pairs_ops([(100 * i, 7 + i) for i in range(40)]) + [nem("kill", 50), nem("recover", 60)]
    c = same(dev, ops, NARROW)
    assert (c.hist.f_id("start"), c.hist.f_id("stop"), len(c.intervals)) == (-1, -1, 0)
    c = same(dev, ops + [nem("stop", 70), nem("stop", 80)], NARROW)  # f_start alone is -1
    assert (c.hist.f_id("start"), len(c.intervals)) == (-1, 0)


def test_an_interval_left_open_ends_at_the_largest_time_of_any_row(dev):
    base = PH.pairs_ops([(100 * i, 7) for i in range(30)]) + [nem("start", 500)]
    c = same(dev, base + [PH.op("invoke", "read", 4, 99000)], NARROW)  # on an :invoke that no record sees
    assert c.intervals.tolist() == [[500, 99000]] and c.view.t_max < 99000
    c = same(dev, base + [nem("kill", 88000), PH.op("invoke", "read", 4, 600)], NARROW)  # on a nemesis row that is no :start / :stop
    assert c.intervals.tolist() == [[500, 88000]]


def test_times_out_of_order_negative_and_all_equal(dev):
    rng = random.Random(26)
    ops = PH.random_ops(rng, 1200, t0=-900000)
    times = [o["time"] for o in ops]
    rng.shuffle(times)
    c = same(dev, [dict(o, time=t) for o, t in zip(ops, times)], NARROW)
    assert c.view.t_max < 0 and c.matched > 300
    c = same(dev, [dict(o, time=-77) for o in ops], NARROW)
    assert (c.view.t_min, c.view.t_max, c.view.x_min, c.view.x_max) == (-77,) * 4


def test_an_unmatched_invocation_at_the_reserved_time_is_legal(dev):
    ops = PH.pairs_ops([(100 * i, 9) for i in range(20)])
    ops = [PH.op("invoke", "read", 7, I64_MIN), PH.op("invoke", "read", 7, 5)] + ops + [PH.op("invoke", "write", 8, I64_MIN)]
    c = same(dev, ops, NARROW)
    assert (c.matched, c.unmatched) == (20, 3)


def with_codes(hist, type_at=(), f_at=()):
    h = P.PerfHistory(hist.type.copy(), hist.f.copy(), hist.process, hist.time, hist.names)
    for r in type_at:
        h.type[r] = 4
    for r in f_at:
        h.f[r] = len(h.names)
    return h


def test_bad_codes_name_the_lowest_row(dev):
    hist = P.PerfHistory.from_ops(PH.random_ops(random.Random(27), 3000))
    last = hist.n - 1
    for r in (0, 1500, last):
        assert ":type" in same_error(dev, with_codes(hist, type_at=[r]), -1, r)
    for r in (0, 1234, last):
        assert f"f {len(hist.names)} is not below n_f {len(hist.names)}" in same_error(dev, with_codes(hist, f_at=[r]), -1, r)
    assert ":type" in same_error(dev, with_codes(hist, type_at=[300, 2900], f_at=[301, 2000]), -1, 300)
    assert "n_f" in same_error(dev, with_codes(hist, type_at=[2100, last], f_at=[2099]), -1, 2099)
    assert ":type" in same_error(dev, with_codes(hist, type_at=[257], f_at=[257]), -1, 257)  # both in one row: the host's first check
    same(dev, PH.hand_ops())  # the context is as good as new


def test_a_matched_invocation_at_the_reserved_time(dev):
    pad = PH.pairs_ops([(100 * i, 9) for i in range(300)], process=5)
    ops = pad + [PH.op("invoke", "read", 0, I64_MIN), PH.op("ok", "read", 0, 50)] + pad
    same_error(dev, P.PerfHistory.from_ops(ops), -1, 600)
    # two of them: the host names the invocation of the lowest completion, which is not the lowest invocation
    ops = pad + [PH.op("invoke", "read", 0, I64_MIN), PH.op("invoke", "read", 1, I64_MIN), PH.op("ok", "read", 1, 50),
                 PH.op("ok", "read", 0, 60)] + pad
    same_error(dev, P.PerfHistory.from_ops(ops), -1, 601)
    # a bad code anywhere is found before it
    hist = with_codes(P.PerfHistory.from_ops(ops), type_at=[1100])
    same_error(dev, hist, -1, 1100)
    same(dev, PH.hand_ops())


def test_thirty_three_names_and_the_options_errors(dev):
    ops = [PH.op("invoke", f"f{i}", 0, i) for i in range(N.LC_PERF_MAX_F + 1)]
    assert "33" in same_error(dev, P.PerfHistory.from_ops(ops), -5)
    hist = P.PerfHistory.from_ops(PH.hand_ops())
    for bad in ({"quantile-dt-ns": 0}, {"rate-dt-ns": -5}, {"quantiles": [0.5, 1.5]}):
        same_error(dev, hist, -1, opts=bad)
    same_error(dev, hist, -2, opts={"rate-dt-ns": 1})  # 40 s of 1 ns buckets: the tables pass their limit
    same(dev, PH.hand_ops())


def test_a_group_above_the_lds_select(dev):
    """2,100 points in one window (the LDS select takes 2,048) and a second :f:
    the HBM select runs on a batch the device built."""
    info = np.zeros(4, np.int64)
    N.check(N.lib().lc_perf_launch_info(N.ptr(info, C.c_int64)))
    assert info[2] == 2048
    rng = random.Random(28)
    pts = [(rng.randrange(10**6), rng.randrange(-50, 10**5)) for _ in range(2100)]
    ops = PH.pairs_ops(pts) + PH.pairs_ops([(5, 3), (10**6 + 5, 4)], f="write", process=1)
    c = same(dev, ops, {"quantile-dt-ns": 10**6, "rate-dt-ns": 10**6})
    assert int(c.results.group.max()) == 2100


def test_two_calls_the_larger_first(dev):
    big = PH.random_ops(random.Random(29), 6000, procs=40)
    small = PH.random_ops(random.Random(30), 700, procs=3, t0=10**7)
    same(dev, big, NARROW)
    same(dev, small, NARROW)


def test_interleaved_with_the_other_calls_of_the_context(dev):
    ops = PH.random_ops(random.Random(31), 2500)
    other = PH.random_ops(random.Random(32), 1800, procs=20, t0=-10**6)
    hist, hist2 = P.PerfHistory.from_ops(ops), P.PerfHistory.from_ops(other)
    packed, packed2 = P.PackedPerf(hist), P.PackedPerf(hist2)
    o = P.make_opts(NARROW)
    counter_hist = CPH.hist(CPH.random_rows(CPH.rng_of(3), 1500, 4, 6))
    ch = counter_hist.as_c()
    a = P.CheckedPerf(dev, hist, o)
    res2 = P.check_batch(dev, packed2.view, o)  # lc_perf_check takes the record columns
    with pytest.raises(N.LincheckError, match="invalid"):
        a.arrays()
    out = C.c_void_p()
    N.check(N.lib().lc_counter_check_history(dev.handle, C.byref(ch), C.byref(N.LcCounterOpts(0, 0)), C.byref(out)))
    b = P.CheckedPerf(dev, hist2, o)
    N.lib().lc_counter_checked_free(out)
    out = C.c_void_p()
    N.check(N.lib().lc_counter_check_history(dev.handle, C.byref(ch), C.byref(N.LcCounterOpts(0, 0)), C.byref(out)))
    N.lib().lc_counter_checked_free(out)
    got, want = b.arrays(), packed2.arrays()  # the counter's call leaves them alone
    for k in ("t_comp", "t_inv", "meta"):
        assert np.array_equal(got[k], want[k]), k
    for k in ("rate", "group", "quant"):
        assert np.array_equal(getattr(b.results, k), getattr(res2, k)), k
    res = P.check_batch(dev, packed.view, o)
    for k in ("rate", "group", "quant"):
        assert np.array_equal(getattr(a.results, k), getattr(res, k)), k


def test_records_belong_to_the_latest_call(dev):
    first = P.CheckedPerf(dev, P.PerfHistory.from_ops(PH.random_ops(random.Random(33), 900)))
    second = P.CheckedPerf(dev, P.PerfHistory.from_ops(PH.hand_ops()))
    b = N.LcPerfBatch()
    assert N.lib().lc_perf_checked_records(dev.handle, first.handle, C.byref(b)) == -1
    assert "latest" in N.lib().lc_last_error().decode()
    assert second.arrays()["t_comp"].tolist() == [r[3] for r in PH.restate(PH.hand_ops())["records"]]
    third = P.CheckedPerf(dev, P.PerfHistory.from_ops(PH.hand_ops()))
    assert second.arrays()["t_comp"].size == 5 and third.arrays()["t_comp"].size == 5  # once down, an object keeps its records


def test_read_edn_demo_shape(dev):
    hist = P.PerfHistory.read_edn(GOLDEN)
    c = same(dev, hist.to_ops(), None, hist)
    assert c.matched > 200 and len(c.intervals)


def test_timing_slots(dev):
    P.CheckedPerf(dev, P.PerfHistory.from_ops(PH.random_ops(random.Random(34), 3000)), P.make_opts(NARROW))
    ms = (C.c_double * 6)()
    N.check(N.lib().lc_perf_history_timing(dev.handle, ms))
    assert all(x > 0 for x in ms) and sum(list(ms)[:5]) <= ms[5] * 1.5


def test_compose_writes_the_same_files_on_either_pack(dev, tmp_path):
    ops = [dict(o, value=None, index=i) for i, o in enumerate(PH.random_ops(random.Random(35), 3000, step=10**8, jitter=10**7))]
    files = {}
    for pack in ("host", "device"):
        store = tmp_path / pack
        perf = ck.perf({"pack": pack})
        r = ck.compose({"perf": perf, "indep": ck.unbridled_optimism()}).check({"store-path": str(store)}, ops, {})
        assert r["perf"] == {"valid?": True}
        files[pack] = {n: open(store / n, "rb").read() for n in ("latency-quantiles.tsv", "rate.tsv")}
        files[pack]["points"] = [perf.last.points(f, t) for f in ("read", "write", "cas", "nope") for t in P.COMPLETIONS]
        files[pack]["nemesis"] = perf.last.nemesis
    assert files["host"] == files["device"]
    assert len(files["host"]["rate.tsv"]) > 500 and len(files["host"]["latency-quantiles.tsv"]) > 500 and files["host"]["points"][0]
