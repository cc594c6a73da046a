"""What lincheck.perf makes of lc_perf_check's tables: series units and
midpoints, the TSV files under store-path, and compose with perf.  No GPU:
the tables come from the restatement (tests/perf_helpers.py), put into the
layout lc_perf_check returns."""
import numpy as np

import perf_helpers as PH
from lincheck import checker as ck
from lincheck import perf as P


def restated_tables(packed, opts):
    """PerfResults with the restatement's numbers."""
    want = PH.restate(packed.hist.to_ops(), {"quantile-dt-ns": int(opts.quantile_dt_ns), "rate-dt-ns": int(opts.rate_dt_ns),
                                             "quantiles": [opts.q[j] for j in range(opts.n_q)]})
    names, F, n_q = packed.names, len(packed.names), int(opts.n_q)
    rb = [b for _, _, b in want["rate"]] or [0]
    qb = [b for _, b in want["groups"]] or [0]
    r0, nr = min(rb), (max(rb) - min(rb) + 1 if want["rate"] else 0)
    q0, nq = min(qb), (max(qb) - min(qb) + 1 if want["groups"] else 0)
    rate, group = np.zeros((F, 3, nr), np.uint64), np.zeros((F, nq), np.uint64)
    quant = np.zeros((F, nq, n_q), np.int64)
    for (f, t, b), c in want["rate"].items():
        rate[names.index(f), ("ok", "fail", "info").index(t), b - r0] = c
    for (f, b), n in want["groups"].items():
        group[names.index(f), b - q0] = n
        quant[names.index(f), b - q0] = want["quantiles"][(f, b)]
    return P.PerfResults(F, tuple(opts.q[j] for j in range(n_q)), int(opts.rate_dt_ns), int(opts.quantile_dt_ns), r0, q0,
                         rate, group, quant)


def series_of(ops, opts=None):
    packed = P.PackedPerf(P.PerfHistory.from_ops(ops))
    return P.PerfSeries(packed, restated_tables(packed, P.make_opts(opts)))


def test_units_and_midpoints():
    s = series_of(PH.hand_ops())
    # window midpoints in seconds, latencies in ms: Jepsen plots x / 1e9 against latency / 1e6
    assert s.quantiles == {"read": {q: [(15.0, 2.0)] for q in (0.5, 0.95, 0.99, 1.0)},
                           "write": {q: [(15.0, 1.0), (45.0, 10000.0)] for q in (0.5, 0.95, 0.99, 1.0)}}
    # count / dt per second at the 10 s windows' midpoints; empty windows absent
    assert s.rate == {"read": {"ok": [(5.0, 0.2), (15.0, 0.1)]}, "write": {"fail": [(5.0, 0.1)], "info": [(45.0, 0.1)]}}
    assert s.nemesis == [(3.0, 31.0), (43.0, 43.0)]
    assert "cas" not in s.quantiles and "start" not in s.rate


def test_points_come_from_the_pack():
    s = series_of(PH.hand_ops())
    assert s.points("read", "ok") == [(1.0, 5.0), (5.0, 2.0)]
    assert s.points("write", "fail") == [(2.0, 1.0)] and s.points("write", "info") == [(31.0, 10000.0)]
    assert s.points("write", "ok") == [] and s.points("nope", "ok") == []


def test_options_change_the_windows():
    s = series_of(PH.hand_ops(), {"quantile-dt-ns": 4 * PH.S, "rate-dt-ns": 2 * PH.S, "quantiles": [1.0]})
    assert s.quantiles["read"] == {1.0: [(2.0, 5.0), (6.0, 2.0)]}
    assert s.rate["read"]["ok"] == [(1.0, 0.5), (5.0, 0.5), (13.0, 0.5)]


def test_tsv_files_and_compose(tmp_path, monkeypatch):
    monkeypatch.setattr(P.PerfChecker, "_dev", lambda self: None)
    real, last = P.PackedPerf, {}

    def remember(hist):
        last["packed"] = real(hist)
        return last["packed"]
    monkeypatch.setattr(P, "check_batch", lambda dev, batch, opts=None: restated_tables(last["packed"], opts))
    monkeypatch.setattr(P, "PackedPerf", remember)
    test = {"store-path": str(tmp_path / "store")}
    r = ck.compose({"perf": ck.perf(), "optimism": ck.unbridled_optimism()}).check(test, PH.hand_ops(), {})
    assert r == {"perf": {"valid?": True}, "optimism": {"valid?": True}, "valid?": True}
    q = [l.split("\t") for l in open(tmp_path / "store" / "latency-quantiles.tsv").read().splitlines()]
    assert ["read 0.5", "15.0", "2.0"] in q and ["write 1", "45.0", "10000.0"] in q and len(q) == 12
    rate = [l.split("\t") for l in open(tmp_path / "store" / "rate.tsv").read().splitlines()]
    assert rate == [["read ok", "5.0", "0.2"], ["read ok", "15.0", "0.1"], ["write fail", "5.0", "0.1"],
                    ["write info", "45.0", "0.1"]]
    # without a store nothing is written
    assert ck.perf().check({}, PH.hand_ops(), {}) == {"valid?": True}
    assert sorted(p.name for p in (tmp_path / "store").iterdir()) == ["latency-quantiles.tsv", "rate.tsv"]


def test_history_without_time_is_an_error_not_a_verdict():
    r = ck.check_safe(ck.perf(), {}, [{"type": "invoke", "f": "read", "process": 0}], {})
    assert r["valid?"] == "unknown" and ":time" in r["error"]
