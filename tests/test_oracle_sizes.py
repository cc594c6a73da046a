"""cref.key_sizes: the C restatement's |I| (after the closure) and |S'| (after
apply) of every :ok, by event.  They are the oracle's account of where a
budget falls, so they are pinned first: against the Python restatement event
by event, against the `peak` the ordinary check reports, and by the property
the budget-edge tests rest on --

    need(key) = max(max |I|, max |S'|) over the events the unbounded search walks

is the least budget that decides the key: at `need` the record is the
unbounded one, at `need - 1` the key is :unknown / budget at the first event
whose |I| or |S'| passes the budget."""
import numpy as np
import pytest

import cref
import linear_ref as LR
from histgen import random_history
from lincheck import history as H

CAUSE = {"none": 0, "nonlin": 1, "budget": 2, "window": 3, "states": 4, "error": 5}
UNBOUNDED = 1 << 40

# the batches of the `need` property: every key is checked at need and at need - 1
SMALL = [dict(n_keys=10, ops_per_key=80, concurrency=7, anomaly_rate=0.5, seed=20),
         dict(n_keys=10, ops_per_key=80, concurrency=9, anomaly_rate=0.5, seed=31)]
# a key that fails with its largest set being the failing :ok's |I| (asserted below)
NEED_AT_FAILING_OK = dict(n_keys=10, ops_per_key=80, concurrency=9, anomaly_rate=0.5, seed=31)  # keys 1 (82), 2 (30)


def record(hc, key, budget):
    keys, r = cref.check_history(hc, budget=budget)
    return r[list(keys).index(key)]


def first_past(sizeI, sizeS, budget):
    """The first event whose |I| or |S'| passes the budget."""
    over = np.flatnonzero((sizeI > budget) | (sizeS > budget))
    return int(over[0])


def check_need(hc, key):
    """The `need` property on one key; returns (need, the unbounded record, sizes)."""
    sizeI, sizeS, res = cref.key_sizes(hc, key, budget=UNBOUNDED, result=True)
    full = record(hc, key, UNBOUNDED)
    assert (res.valid, res.cause, res.fail_event, res.peak) == (full["valid"], full["cause"], full["fail_event"],
                                                                 full["peak"])
    assert full["cause"] != CAUSE["budget"]
    assert len(sizeI) == len(sizeS) == full["n_events"] + (full["valid"] == 0)  # the failing :ok is walked too
    assert max(int(sizeS.max(initial=1)), 1) == full["peak"]
    need = cref.need(hc, key)
    assert need == max(int(sizeI.max(initial=1)), int(sizeS.max(initial=1)))
    at = record(hc, key, need)
    for f in ("valid", "cause", "fail_event", "peak", "probes"):
        assert at[f] == full[f], f"budget need = {need}: {f}"
    if need > 1:
        below = record(hc, key, need - 1)
        assert (below["valid"], below["cause"]) == (-1, CAUSE["budget"]), f"budget need - 1 = {need - 1}"
        assert below["fail_event"] == first_past(sizeI, sizeS, need - 1)
        # the sizes the bounded walk records stop there, |I| at budget + 1 if the closure passed it
        bI, bS = cref.key_sizes(hc, key, budget=need - 1)
        e = int(below["fail_event"])
        assert len(bI) == e + 1
        np.testing.assert_array_equal(bI[:e], sizeI[:e])
        np.testing.assert_array_equal(bS[:e], sizeS[:e])
        assert (bI[e], bS[e]) == ((need, 0) if sizeI[e] > need - 1 else (sizeI[e], sizeS[e]))
    return need, full, sizeI, sizeS


@pytest.mark.parametrize("seed", range(40))
def test_sizes_match_python_restatement(seed):
    """Event by event on histgen.random_history keys, unbounded and at
    budgets small enough to end keys inside a closure and after an apply."""
    ops = random_history(seed, n_keys=3, max_ops=12, procs=5)
    hc = H.History.from_ops(ops).as_c()
    for budget in (UNBOUNDED, 2, 3, 5):
        for k in LR.history_keys(ops):
            a = LR.analysis(LR.subhistory(ops, k), budget=budget)
            sizeI, sizeS = cref.key_sizes(hc, k, budget=budget)
            walked = len(a.events) if a.fail_event is None else a.fail_event + 1
            assert len(sizeI) == len(sizeS) == walked
            for e in range(walked):
                assert sizeI[e] == a.size_I.get(e, 0), (seed, budget, k, e)
                assert sizeS[e] == a.size_S.get(e, 0), (seed, budget, k, e)
                assert (a.events[e][0] == "invoke") == (e not in a.size_I)
            if a.cause != "budget":
                assert max(int(sizeS.max(initial=1)), 1) == a.peak_configs


@pytest.mark.parametrize("kw", [
    dict(n_keys=3, ops_per_key=120, concurrency=6, anomaly_rate=0.5, seed=5),
    dict(n_keys=2, ops_per_key=100, concurrency=7, info_rate=0.05, seed=4),
])
def test_sizes_match_python_restatement_on_synthetic(kw):
    ops = H.synth(**kw).to_ops()
    hc = H.History.from_ops(ops).as_c()
    for k in LR.history_keys(ops):
        full = LR.analysis(LR.subhistory(ops, k), budget=UNBOUNDED)
        top = max(list(full.size_I.values()) + list(full.size_S.values()))
        for budget in (UNBOUNDED, top - 1, top // 2):
            a = LR.analysis(LR.subhistory(ops, k), budget=budget)
            sizeI, sizeS = cref.key_sizes(hc, k, budget=budget)
            walked = len(a.events) if a.fail_event is None else a.fail_event + 1
            assert len(sizeI) == walked
            assert {e: int(v) for e, v in enumerate(sizeI) if e in a.size_I} == a.size_I
            assert {e: int(v) for e, v in enumerate(sizeS) if e in a.size_S} == a.size_S
            assert not sizeI[[e for e in range(walked) if e not in a.size_I]].any()


@pytest.mark.parametrize("kw", SMALL, ids=lambda kw: f"seed{kw['seed']}")
def test_need_is_the_least_deciding_budget(kw):
    h = H.synth(**kw)
    hc = h.as_c()
    keys, full = cref.check_history(hc, budget=UNBOUNDED)
    assert (full["valid"] == 0).any() and (full["valid"] == 1).any()
    by_I = by_S = 0
    for k in keys:
        need, _, sizeI, sizeS = check_need(hc, int(k))
        by_I += sizeI.max() > sizeS.max()
        by_S += sizeS.max() >= sizeI.max()
    assert by_I > 0  # (|I| decides almost every key; by_S may be 0 here)


def test_need_attained_by_I_at_the_failing_ok():
    """The failing :ok's |I| is the key's largest set: one below it the key is
    :unknown instead of :invalid, at the same event (the |I| budget test comes
    before the emptiness test)."""
    h = H.synth(**NEED_AT_FAILING_OK)
    hc = h.as_c()
    keys, full = cref.check_history(hc, budget=UNBOUNDED)
    found = []
    for k, r in zip(keys, full):
        if r["valid"] != 0:
            continue
        sizeI, sizeS = cref.key_sizes(hc, int(k), budget=UNBOUNDED)
        e = int(r["fail_event"])
        if sizeI[e] == cref.need(hc, int(k)) and sizeI[:e].max(initial=0) < sizeI[e] and sizeS.max() < sizeI[e]:
            found.append(int(k))
    assert found, "no key with need attained only at its failing :ok: choose another batch"
    for k in found:
        need, full_k, sizeI, sizeS = check_need(hc, k)
        below = record(hc, k, need - 1)
        assert (full_k["valid"], full_k["cause"]) == (0, CAUSE["nonlin"])
        assert (below["valid"], below["cause"]) == (-1, CAUSE["budget"])
        assert below["fail_event"] == full_k["fail_event"]


def test_no_such_key():
    h = H.synth(n_keys=2, ops_per_key=10, concurrency=3, seed=1)
    with pytest.raises(RuntimeError):
        cref.key_sizes(h.as_c(), 12345)
