"""(model/multi-register), (model/register) and (model/mutex) through every
set tier, the HBM tiers, WGL and competition, against the oracles.

The bands are tests/model_bands.py's (tests/test_model_bands.py proves on the
CPU what each key is).  Expected records are the C restatement's for register
and mutex and oracle/linear_ref.py's / oracle/wgl_ref.py's for the table model
multi-register, which the C restatement does not know.  What first takes which
model through which kernel -- the proof is always an oracle size past a tier's
capacity (model_bands.tier_class) together with lc_stats.deep_keys:
  k_search_lds T1 / T2 on table rows      test_records_probes_and_routing[mr_narrow]
  narrow HBM tier, LDS pass, table rows   the same (hbm_lds key 6: |S'| 1200 > 1024)
  narrow HBM tier, HBM pass, table rows   the same (hbm_hbm keys 3, 9: |S'| 3092 > 2048, |I| 4543 > 4096)
  wide tier with real sets, table rows    test_records_probes_and_routing[mr_wide] (764+ maps, needs 529 - 2422)
  k_search_layers, register and mutex     ...[reg7-default], ...[mutex-default] (tier3_ms > 0, deep_keys)
  narrow HBM tier, register and mutex     ...[reg7-layers_off], [reg12-*] (13 states), [mutex-layers_off]
  wide tier, register                     ...[reg_wide-*] (329+ states, needs 576 - 3584)
  k_wgl on table rows, LDS / HBM cache    test_wgl_table_model (caches 88 - 987 / 2190, 2688, 9653 > 2048)
  k_wgl past T2, register and mutex       test_wgl_register_and_mutex_past_t2
  competition on table rows               test_competition_table_model

Not populated, and what was searched: the table-model key decided by |S'| is
a T2 key (mr_narrow key 8: |S'| 864 > |I| 848); among seeds 31-34 of the four
two-register shapes no key past T2 had max |S'| > max |I| at a need below
5,000 (one hbm_hbm key of 16 processes has |S'| 2792 > |I| 2720 but WGL's cache
passes 20,000 on it).  LC_PATH_WGL_SMALL's spill point is reached by one key
(mr_narrow key 10: cache 9,653 >= 8,192)."""
import numpy as np
import pytest

import cref
import linear_ref as LR
import model_bands as MB
import wgl_ref as W
from helpers import path_tuple
from lincheck import _native as N
from lincheck import checker as ck
from lincheck import history as H
from lincheck import independent, model
from lincheck import parallel as P
from lincheck.checker import Device, Packed
from test_gpu_budget_edges import flip, same_as_oracle
from test_gpu_multi_register import _path
from test_gpu_wgl import wgl_vs_oracle

pytestmark = pytest.mark.gpu

BUDGET = 1 << 20
PY_ORACLE_MAX_NEED = 5000          # linear_ref.py enumerates the final configs of keys up to this need in seconds
PATHS = {"default": 0, "layers_off": N.LC_PATH_LAYERS_OFF}
BAND_PATHS = ([(b, "default") for b in ("mr_narrow", "mr_wide")] +
              [(b, p) for b in ("reg7", "reg12", "reg_wide", "mutex") for p in PATHS])
STATES_CAUSE = 4


@pytest.fixture(scope="module")
def bands():
    """The bands and their oracle records, built once for the module."""
    yield MB.band
    MB._bands.clear()


def same_records(b, what, budget, valid, cause, fail_event, peak=None):
    orc = b.oracle(budget)
    for f, got in (("valid", valid), ("cause", cause), ("fail_event", fail_event), ("peak", peak)):
        if got is None:
            continue
        ok = (np.asarray(got) == orc[f]) | ((f == "peak") & (orc["cause"] == MB.BUDGET_CAUSE))
        bad = np.flatnonzero(~ok)
        assert not len(bad), (f"{what}: {f} differs on " + "; ".join(
            f"{b.describe(i)} (device {got[i]}, oracle {orc[f][i]})" for i in bad))


# ------------------------------------------------------------------ a. records and routing
@pytest.mark.parametrize("name,path", BAND_PATHS)
def test_records_probes_and_routing(bands, name, path):
    """lc_check_batch with peaks and probe counts at 2^20: the oracle's
    records and probe total; the HBM tiers search exactly the keys past T2 and
    the keys with wide configs; a table batch has no register tier."""
    b = bands(name)
    for i in range(b.pk.n_keys):
        print(b.describe(i))
    r = Device(0, budget=BUDGET, count_probes=True, path_flags=PATHS[path]).check(b.pk)
    orc = b.oracle(BUDGET)
    n_deep = sum(b.deep(i) for i in range(b.pk.n_keys))
    print(f"{name}, {path}: deep_keys {r.stats['deep_keys']} (expected {n_deep}), t0_path {r.stats['t0_path']}, "
          f"tier3_ms {r.stats['tier3_ms']:.3f}, probes {r.stats['probes']} (oracle {int(orc['probes'].sum())})")
    same_records(b, f"{name}, {path}", BUDGET, r.valid, r.cause, r.fail_event, r.peak)
    assert r.stats["probes"] == int(orc["probes"].sum())
    assert r.stats["deep_keys"] == n_deep
    assert r.stats["keys_done"] == b.pk.n_keys
    if b.table:
        assert r.stats["t0_path"] == "none"
    if n_deep:
        assert r.stats["tier3_ms"] > 0


@pytest.mark.parametrize("name,path", BAND_PATHS)
def test_other_entries(bands, name, path):
    """verdicts_only, peaks=False, a resident batch's node step and the node
    step from the host: the same records."""
    b = bands(name)
    pk = b.pk
    dev = Device(0, budget=BUDGET, path_flags=PATHS[path])
    r = dev.check(pk, verdicts_only=True)
    same_records(b, f"{name}, {path}, verdicts_only", BUDGET, r.valid, r.cause, r.fail_event)
    r = dev.check(pk, peaks=False)
    same_records(b, f"{name}, {path}, peaks=False", BUDGET, r.valid, r.cause, r.fail_event)
    db = dev.upload(pk)
    db.check_node(pk.n_keys)
    v, cause, fe = P.unpack_records(dev.node_records(pk.n_keys).astype(np.int64))
    same_records(b, f"{name}, {path}, upload / check_node", BUDGET, v, cause, fe)
    rec, _st = dev.check_node(pk, pk.n_keys)
    v, cause, fe = P.unpack_records(rec.astype(np.int64))
    same_records(b, f"{name}, {path}, check_node", BUDGET, v, cause, fe)


# ------------------------------------------------------------------ b. budget flips
FLIPS = [
    # (band, key, path, what the target is)
    ("mr_narrow", 5, "default", "T1, table rows"),
    ("mr_narrow", 0, "default", "T2, table rows; an invalid key decided long before its failing :ok"),
    ("mr_narrow", 8, "default", "T2, table rows; need by |S'| (864 > max |I| 848)"),
    ("mr_narrow", 6, "default", "narrow HBM tier's LDS pass, table rows"),
    ("mr_narrow", 3, "default", "narrow HBM tier's HBM pass (|S'| 3092 > 2048), table rows"),
    ("mr_narrow", 9, "default", "narrow HBM tier redone on the HBM tables (|I| 4543 > 4096), table rows"),
    ("mr_wide", 3, "default", "wide tier, 969 maps"),
    ("mr_wide", 0, "default", "wide tier, 894 maps, an invalid key"),
    ("reg7", 4, "default", "T1, register"),
    ("reg7", 2, "default", "T2, register"),
    ("reg7", 0, "default", "layered tier, register, 8 states"),
    ("reg7", 0, "layers_off", "narrow HBM tier's LDS pass, register"),
    ("reg7", 5, "default", "layered tier, register, |I| 5216"),
    ("reg7", 5, "layers_off", "narrow HBM tier redone on the HBM tables, register"),
    ("reg12", 0, "default", "13 states: handed on by the layered tier; an invalid key"),
    ("reg_wide", 0, "default", "wide tier, register, 362 states"),
    ("mutex", 2, "default", "T1, mutex"),
    ("mutex", 1, "default", "T2, mutex, an invalid key"),
    ("mutex", 0, "default", "layered tier, mutex"),
    ("mutex", 0, "layers_off", "narrow HBM tier's LDS pass, mutex"),
    ("mutex", 3, "default", "layered tier, mutex, |S'| 2611"),
    ("mutex", 3, "layers_off", "narrow HBM tier's HBM pass, mutex"),
]


@pytest.mark.parametrize("name,i,path,what", FLIPS, ids=[f"{n}-{i}-{p}" for n, i, p, _ in FLIPS])
def test_budget_flip(bands, name, i, path, what):
    """One target per tier class of each model at need - 1 and at need
    (test_gpu_budget_edges.flip with the band's own oracle): :unknown / budget
    at the first event whose |I| or |S'| passes need - 1, the unbounded record
    at need; the whole batch compared at both budgets."""
    b = bands(name)
    below, at = flip(b, i, what, path_flags=PATHS[path])
    if name == "mr_narrow" and i == 8:
        _e, nI, nS = b.deciding(i)
        assert nS == b.need[i] > b.sizes[i][0].max(), "the target is not decided by |S'|"
    if b.table:
        assert below.stats["t0_path"] == at.stats["t0_path"] == "none"
    if b.deep(i):
        assert at.stats["deep_keys"] > 0


# ------------------------------------------------------------------ c. final configs
@pytest.mark.parametrize("name,path", BAND_PATHS)
def test_final_configs_of_invalid_keys(bands, name, path):
    """Every invalid key past T1 (need <= 5,000): the final configs returned
    are distinct configs of the set standing before the failing :ok as
    linear_ref.py enumerates it, min(|set|, 10) of them, the state field
    decoded through the packed batch's own state table."""
    b = bands(name)
    full = b.oracle(BUDGET)
    bad = [i for i in range(b.pk.n_keys) if full["valid"][i] == 0 and b.cls[i] != "t1" and b.need[i] <= PY_ORACLE_MAX_NEED]
    assert bad, f"{name} holds no invalid key past T1"
    r = Device(0, budget=BUDGET, path_flags=PATHS[path]).check(b.pk)
    same_records(b, f"{name}, {path}", BUDGET, r.valid, r.cause, r.fail_event, r.peak)
    for i in bad:
        a = b.analysis(i)
        assert a.valid is False and a.fail_event == full["fail_event"][i] != b.first_ok(i)
        want = MB.oracle_configs(a.final_configs, a.final_slots, b.model_name)
        got = [(MB.device_state(b.pk, i, st, b.model_name), m) for st, m in MB.record_configs(r.final[i], r.n_final[i])]
        print(f"{b.describe(i)}, {path}: {len(got)} of {len(want)} final configs")
        assert len(got) == min(len(want), 10) == len(set(got)), b.describe(i)
        assert set(got) <= want, b.describe(i)


@pytest.mark.parametrize("name", sorted(MB.ROWS))
def test_rendered_counterexamples(bands, name):
    """independent/checker over linearizable {:algorithm :linear} on keys a
    deep tier decided: :op, :previous-ok and :final-paths are the
    restatement's (a subset of LR.final_paths, all of it when it has at most
    10 paths; larger path sets than 2^12 are not enumerated)."""
    b = bands(name)
    full = b.oracle(BUDGET)
    lin = ck.linearizable({"model": b.model, "algorithm": "linear", "max-configs": BUDGET})
    out = independent.checker(lin).check({}, b.ops, {})
    bad = [i for i in range(b.pk.n_keys) if full["valid"][i] == 0]
    assert sorted(out["failures"]) == bad and any(b.cls[i] != "t1" for i in bad)
    for i in bad:
        a, r, sub = b.analysis(i), out["results"][i], b.subs[i]
        assert r["op"]["index"] == sub[a.fail_pos]["index"], b.describe(i)
        prev = sub[a.previous_ok_pos]["index"] if a.previous_ok_pos is not None else None
        assert (r["previous-ok"] or {}).get("index") == prev, b.describe(i)
        if b.need[i] > PY_ORACLE_MAX_NEED:
            continue
        paths = {_path(p) if b.table else path_tuple(p, b.model_name) for p in r["final-paths"]}
        allp = LR.final_paths(a, sub, model=b.model_name, cap=1 << 12)
        print(f"{b.describe(i)}: {len(paths)} paths rendered, {'> 4096' if allp is None else len(allp)} in all")
        assert len(paths) > 0
        if allp is not None:
            assert paths <= allp
            if len(allp) <= ck.TRUNCATE:
                assert paths == allp


# ------------------------------------------------------------------ d. WGL
def wgl_table_vs_oracle(b, budget, path_flags=0):
    """k_wgl on a table batch against wgl_ref.analysis: verdict, cause,
    failing event, cache size of decided keys, and the frontier as {map,
    linearized pending ops}: min(|frontier|, 10) distinct members of it."""
    res = Device(0, budget=budget, algorithm=N.LC_ALGO_WGL, path_flags=path_flags).check(b.pk)
    orc = b.wgl(budget)
    assert (res.analyzer == N.LC_ALGO_WGL).all()
    for i, w in enumerate(orc):
        what = f"{b.describe(i)}, wgl at {budget}"
        events = b.linear(MB.UNBOUNDED)[i].events
        fe = -1
        if w.valid is False:
            (fe,) = [e for e, ev in enumerate(events) if ev[2] == w.fail_pos]
        got = (int(res.valid[i]), int(res.cause[i]), int(res.fail_event[i]))
        assert got == (MB.VALID[w.valid], MB.CAUSE[w.cause], fe), (what, got, w.valid, w.cause, fe)
        if w.cause in ("none", "nonlin"):
            assert int(res.peak[i]) == w.cache_size, (what, int(res.peak[i]), w.cache_size)
        if w.valid is False:
            want = MB.oracle_configs(w.frontier, MB.slots_of(events), b.model_name)
            got = [(MB.device_state(b.pk, i, st, b.model_name), m) for st, m in MB.record_configs(res.final[i], res.n_final[i])]
            assert len(got) == min(len(want), 10) == len(set(got)), (what, len(got), len(want))
            assert set(got) <= want, what
    return res, orc


WGL_PATHS = {"default": 0, "ev_hbm": N.LC_PATH_WGL_EV_HBM, "small": N.LC_PATH_WGL_SMALL}


@pytest.mark.parametrize("path", sorted(WGL_PATHS))
def test_wgl_table_model(bands, path):
    """k_wgl stepping table rows, caches on both sides of the move from LDS to
    HBM (2,048 pairs); events from HBM; the small tables, whose spill point
    (8,192) one key's cache passes."""
    b = bands("mr_narrow")
    res, orc = wgl_table_vs_oracle(b, BUDGET, WGL_PATHS[path])
    caches = [w.cache_size for w in orc]
    print(f"wgl, {path}: caches {caches}, spilled {res.stats['wgl_spilled']}")
    assert {i for i, c in enumerate(caches) if c > MB.WGL_MIGRATE} == set(MB.WGL_ABOVE_MIGRATE)
    assert any(w.valid is False for w in orc) and any(w.valid is True for w in orc)
    if path == "small":
        assert res.stats["wgl_spilled"] == sum(c >= MB.WGL_SMALL_SPILL for c in caches) == len(MB.WGL_SPILLS)


@pytest.mark.parametrize("i", [4, 0])
def test_wgl_table_model_cache_budget(bands, i):
    """The budget bounds Lowe's cache: at cache - 1 :unknown / budget, at
    cache the unbounded record (key 4: 987 pairs, in LDS; key 0: 2,688, moved
    to HBM)."""
    b = bands("mr_narrow")
    need = b.wgl(MB.UNBOUNDED)[i].cache_size
    assert b.wgl(MB.UNBOUNDED)[i].cause != "budget"
    below, _ = wgl_table_vs_oracle(b, need - 1)
    assert (int(below.valid[i]), int(below.cause[i])) == (-1, MB.BUDGET_CAUSE)
    at, orc = wgl_table_vs_oracle(b, need)
    assert int(at.valid[i]) == MB.VALID[orc[i].valid] != -1 and int(at.peak[i]) == need


def test_wgl_table_model_wide(bands):
    """k_wgl on table rows with wide configs (764+ maps)."""
    b = bands("mr_wide")
    res, orc = wgl_table_vs_oracle(b, BUDGET)
    assert any(w.valid is False for w in orc) and any(w.valid is True for w in orc)


@pytest.mark.parametrize("name", ["reg7", "reg12", "reg_wide", "mutex"])
def test_wgl_register_and_mutex_past_t2(bands, name):
    """The register and mutex bands (keys past T2, 13 and 300+ states)
    through wgl_vs_oracle as it is: the C restatement's records and frontier."""
    b = bands(name)
    _pk, res, orc = wgl_vs_oracle(b.hist, BUDGET, b.model_name)
    print(f"{name}: wgl caches {orc['peak'].tolist()}, verdicts {orc['valid'].tolist()}")
    assert (orc["valid"] == 0).any() and (orc["valid"] == 1).any()


# ------------------------------------------------------------------ e. competition
def test_competition_table_model(bands):
    """knossos.competition on the table model at a budget :linear gives up at
    and WGL decides within: WGL answers exactly the budget keys, each record is
    its analyser's own oracle's, and the rendered result names the analyser."""
    b = bands("mr_narrow")
    B = MB.COMPETITION_BUDGET
    lin = b.oracle(B)
    left = lin["cause"] == MB.BUDGET_CAUSE
    wgl = b.wgl(B)
    decided = [i for i in np.flatnonzero(left) if wgl[i].valid != "unknown"]
    assert len(decided) >= 1 and not left.all()  # keys 2, 3, 6, 9 decided; key 10's cache passes the budget as well
    r = Device(0, budget=B, algorithm=N.LC_ALGO_COMPETITION).check(b.pk)
    print(f"competition at {B}: :linear leaves {np.flatnonzero(left).tolist()}, analyzer {r.analyzer.tolist()}")
    np.testing.assert_array_equal(r.analyzer == N.LC_ALGO_WGL, left)
    assert r.stats["wgl_keys"] == int(left.sum())
    for i in range(b.pk.n_keys):
        got = (int(r.valid[i]), int(r.cause[i]), int(r.fail_event[i]))
        if left[i]:
            assert got == (MB.VALID[wgl[i].valid], MB.CAUSE[wgl[i].cause], -1), b.describe(i)
        else:
            assert got == (int(lin["valid"][i]), int(lin["cause"][i]), int(lin["fail_event"][i])), b.describe(i)
    out = independent.checker(ck.linearizable({"model": model.multi_register(), "max-configs": B})).check({}, b.ops, {})
    for i in range(b.pk.n_keys):
        res = out["results"][i]
        want = wgl[i].valid if left[i] else {1: True, 0: False}[int(lin["valid"][i])]
        assert res["analyzer"] == ("wgl" if left[i] else "linear") and res["valid?"] == want, b.describe(i)


# ------------------------------------------------------------------ f. the state-count limit
ALGOS = {"linear": N.LC_ALGO_LINEAR, "wgl": N.LC_ALGO_WGL, "competition": N.LC_ALGO_COMPETITION}


@pytest.fixture(scope="module")
def map_limit(bands):
    """The multi-register keys at the limit and both restatements' analyses
    of them; the count of reachable maps (ten seconds in Python for 32,767) is
    taken once per key for both."""
    saved = LR.reachable_maps
    LR.reachable_maps = MB.memoised_reachable_maps
    try:
        ops = MB.map_limit_ops()
        subs = [LR.subhistory(ops, k) for k in range(4)]
        lin = [LR.analysis(s, budget=BUDGET, model="multi-register") for s in subs]
        wgl = [W.analysis(s, budget=BUDGET, model="multi-register") for s in subs]
    finally:
        LR.reachable_maps = saved
    return ops, Packed(H.History.from_ops(ops), model.multi_register()), lin, wgl


@pytest.mark.parametrize("algo", sorted(ALGOS))
def test_map_count_limit(map_limit, algo):
    """A key with 32,767 reachable maps is decided -- invalid at its last
    read, with the one final config's 15-bit state field decoding to the last
    map -- and one with 32,768 is :unknown / states with no failing event;
    the ordinary keys before and after keep their records."""
    ops, pk, lin, wgl = map_limit
    assert [int(x) for x in N.carray(pk.view.key_states, 4, np.uint16)][1:3] == [32767, 32768]
    orc = wgl if algo == "wgl" else lin
    r = Device(0, budget=BUDGET, algorithm=ALGOS[algo]).check(pk)
    for i in range(4):
        a = orc[i]
        fe = getattr(a, "fail_event", None)
        if algo == "wgl" and a.valid is False:
            (fe,) = [e for e, ev in enumerate(lin[i].events) if ev[2] == a.fail_pos]
        got = (int(r.valid[i]), int(r.cause[i]), int(r.fail_event[i]))
        assert got == (MB.VALID[a.valid], MB.CAUSE[a.cause], -1 if fe is None else fe), (algo, i, got)
    assert (int(r.valid[2]), int(r.cause[2]), int(r.fail_event[2])) == (-1, STATES_CAUSE, -1)
    assert int(r.valid[1]) == 0 and int(r.fail_event[1]) == pk.n_events(1) - 1
    assert int(r.valid[0]) == 0 and int(r.valid[3]) == 1
    last_map = tuple((reg, n) for reg, n in enumerate(MB.MAPS_AT_LIMIT))
    assert int(r.n_final[1]) == 1
    ((st, mask),) = MB.record_configs(r.final[1], 1)
    print(f"{algo}: the last map has state id {st}")
    assert MB.device_state(pk, 1, st, "multi-register") == last_map and mask == 0
    if algo != "wgl":
        assert lin[1].final_configs == [(last_map, frozenset())]


@pytest.fixture(scope="module")
def value_limit():
    ops = MB.value_limit_ops()
    hist = H.History.from_ops(ops)
    return hist, Packed(hist)


@pytest.mark.parametrize("algo", sorted(ALGOS))
def test_value_count_limit(value_limit, algo):
    """cas-register: a key with 32,766 written values (32,767 states) is
    decided, its last read seeing the highest state id; one with 32,767 values
    is :unknown / states; the neighbours keep their records."""
    hist, pk = value_limit
    if algo == "wgl":
        _keys, orc, _fin, _nf = cref.check_history_wgl(hist.as_c(), budget=BUDGET, threads=8)
    else:
        _keys, orc = cref.check_history(hist.as_c(), budget=BUDGET, threads=8)
    assert (int(orc["valid"][1]), int(orc["cause"][1])) == (1, 0)
    assert (int(orc["valid"][2]), int(orc["cause"][2]), int(orc["fail_event"][2])) == (-1, STATES_CAUSE, -1)
    assert pk.state_value(1, MB.VALUES_AT_LIMIT) == MB.VALUES_AT_LIMIT  # the last value written has the highest id
    r = Device(0, budget=BUDGET, algorithm=ALGOS[algo]).check(pk)
    for f in ("valid", "cause", "fail_event"):
        np.testing.assert_array_equal(getattr(r, f), orc[f], err_msg=f"{algo}: {f}")
    if algo == "competition":
        assert (r.analyzer == N.LC_ALGO_LINEAR).all()
