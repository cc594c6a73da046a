"""The exact mode of a stream's resident set tier on the device
(LC_STREAM_EXACT | LC_STREAM_SET_TIER: k_stream_set_exact and k_stream_set_final
in csrc/device_stream_set_exact.hip, the host's side in csrc/host_stream.cpp).
Expected values come from the oracle (oracle/linear_ref.c through cref: records
and set sizes; oracle/linear_ref.py: config sets) or from the ordinary checker,
never from a stream.

The keys (H.synth of test_gpu_stream_set.HISTORIES "long" and "B", budget 2^20):

  long 51   leaves at event 66, invalid at event 187, peak 768      late failure
  long 15   leaves at 376, need 624 by |I| at event 393             budget edge
  long 48   leaves at 312, need 660 by |I| at event 313             budget edge, the first :ok after the migration
  B 0       leaves at 194, need 648 by |I| at event 196             budget edge
  long 8    leaves at 240, peak 12,288, |I| 43,520 at event 413     fallback
  long 2    leaves at 72 and stays in the set tier to the end
  long 19   leaves at 276 but is invalid at 154, before leaving     control

Every test re-asserts what it relies on from the oracle first, so a change to
host_synth.cpp fails loudly.  No budget edge inside the set tier decided by
|S'| is known (tests/tools/find_set_tier_s_edges.py): the |I| edges here and
tests/test_stream_set_exact_plan.py's triples carry the rule.

Final configs carry the stream's own state ids (its packer numbers a key's
states itself), so the expected selection is made here from the oracle's set
with those ids: the max_final smallest in (slot mask, state id) order."""
import ctypes as C

import numpy as np
import pytest

import cref
import linear_ref as LR
import stream_helpers as S
import stream_set_rule as R
import test_gpu_stream_set as TS
from helpers import config_tuple, path_tuple
from lincheck import _native as N
from lincheck import checker as CK
from lincheck import history as H
from lincheck import model
from lincheck.checker import Device, Packed
from lincheck.stream import Stream

pytestmark = pytest.mark.gpu

BUDGET = 2  # LC_CAUSE_BUDGET
FIELDS = ("valid", "cause", "fail_event", "peak")
CAP = R.CAP
SELECTION = [51, 8, 15, 48, 2, 19]   # of "long"; two keys that stay in the register tier join them
_memo = {}


@pytest.fixture(scope="module")
def dev():
    return Device(0)


def memo(name, make):
    if name not in _memo:
        _memo[name] = make()
    return _memo[name]


def selection():
    """(history, keys, the oracle's records, the restatement, exact runs of the leaving keys) of the selection."""
    def make():
        h, keys, _orc, rs = TS.case("long")
        stay = [k for k in keys if rs.defer_at[k] < 0][:2]
        hs = h.select_keys(SELECTION + stay)
        ks, orc = cref.check_history(hs.as_c(), budget=1 << 20, threads=8)
        rss = S.Restated(hs)
        runs = {i: R.Run(rss.events[k], closed=False) for i, k in enumerate(ks) if rss.defer_at[k] >= 0}
        return hs, list(ks), orc, rss, runs
    return memo("selection", make)


def one_key(name, key):
    """(history, oracle record at 2^20, restatement, sizeI, sizeS) of one key alone."""
    def make():
        h = TS.case(name)[0].select_keys([key])
        ks, orc = cref.check_history(h.as_c(), budget=1 << 20, threads=1)
        assert list(ks) == [key]
        sI, sS = cref.key_sizes(h.as_c(), key, budget=1 << 62)
        return h, orc, S.Restated(h), sI.astype(np.int64), sS.astype(np.int64)
    return memo((name, key), make)


def record(res, i=0):
    return tuple(int(getattr(res, f)[i]) for f in FIELDS)


def oracle_record(orc, i=0):
    return tuple(int(orc[f][i]) for f in FIELDS)


def state_ids(s, i):
    """register value -> the stream's state id of key index i."""
    out, st = {}, 0
    while True:
        try:
            out[s.state_value(i, st)] = st
        except N.LincheckError:
            return out
        st += 1


def got_configs(s, res, i):
    """Key index i's final configs as [(slot mask, state id)]; the record form is
    write_final_mem's: the mask's low word, state << 48 | its (here empty) high bits."""
    n = int(res.n_final[i])
    assert not res.final[i, n:].any(), "words past n_final"
    assert all(int(res.final[i, c, 1]) & ((1 << 48) - 1) == 0 for c in range(n))
    return [(int(res.final[i, c, 0]), int(res.final[i, c, 1]) >> 48) for c in range(n)]


def same_selection(s, res, i, oset, max_final, label):
    """The canonical selection: the max_final smallest of the oracle's set in
    (slot mask, state id) order -- which implies what
    test_gpu_stream_exact.same_configs compares: the same masks in the same
    order, the same values under every mask max_final does not cut."""
    ids = state_ids(s, i)
    want = sorted((mask, ids[v]) for v, mask in oset)[:max_final]
    got = got_configs(s, res, i)
    assert len(got) == min(len(oset), max_final), f"{label}: n_final {len(got)} of a set of {len(oset)}"
    assert got == want, f"{label}: configs {got}, the oracle's smallest {want}"


# ---------------------------------------------------------------- 1. every split
@pytest.mark.parametrize("step", [1, 7, 64, 0])
def test_every_split_ends_with_the_oracle_s_records(dev, step):
    h, keys, orc, rs, runs = selection()
    fev = TS.failing(orc)
    i51, i8, i19 = keys.index(51), keys.index(8), keys.index(19)
    assert oracle_record(orc, i51) == (0, 1, 187, 768) and rs.defer_at[51] == 66
    assert orc["valid"][i19] == 0 and orc["fail_event"][i19] < rs.defer_at[19]
    assert sum(rs.defer_at[k] < 0 for k in keys) == 2 and len(keys) == 8
    s = Stream(dev, exact=True, set_tier=True)
    invalid = set()

    def after(n_rows, up):
        assert not set(up.invalid) & invalid
        invalid.update(up.invalid)
        want = {i for i in range(up.n_keys) if rs.emitted(keys[i], n_rows) > fev[i]}
        assert invalid == want, f"step {step}, {n_rows} rows: invalid {sorted(invalid)}, oracle says {sorted(want)}"

    S.feed(s, h, step or len(h), after)
    up = s.finish()
    res = s.results()
    assert res.keys == keys
    for i in range(len(keys)):
        assert record(res, i) == oracle_record(orc, i), f"step {step}, key {keys[i]}"
    must = {i for i, r in runs.items() if r.falls_back}
    fell = {i for i in range(len(keys)) if s.key_tier(i) == "fallen_back"}
    assert fell == must == {i8}, f"fell back {sorted(fell)}, the exact sets pass the cap in {sorted(must)}"
    t = s.tiers()
    assert up.n_deferred == t["fallen_back"] == 1 and t["register"] == 2 and t["dead"] == 2 and t["set"] == 3, t
    assert s.set_stats()["pool_in_use"] == t["set"]
    s.close()


# ---------------------------------------------------------------- 2. migration is exact
@pytest.mark.parametrize("cut", ["before", "after"])
def test_the_migrated_set_is_the_oracle_s(dev, cut):
    """test_gpu_stream_set.test_migration_at_each_lattice_shape with equality:
    after the migrating append and after each later one the set record holds
    the oracle's set, each config once."""
    shapes, reads = set(), []
    for b, rs in TS.migration_batches():
        for k in b.pk.keys:
            ev, d = rs.events[k], rs.defer_at[k]
            assert d >= 0 and rs.ready[k][d] < S.NEVER
            hist = b.hist.select_keys([k])
            at = rs.ready[k][d] if cut == "after" else rs.ready[k][d] - 1
            n1 = int(np.searchsorted(np.flatnonzero(b.hist.key == k), at))
            s = Stream(dev, exact=True, set_tier=True)
            checked = 0
            for lo, hi in ((0, n1), (n1, n1 + 1), (n1 + 1, n1 + 9), (n1 + 9, len(hist))):
                if lo >= min(hi, len(hist)):
                    continue
                s.append(S.rows(hist, lo, min(hi, len(hist))))
                if s.key_tier(0) != "set":
                    continue
                e = s.key_events(0)["searched"]
                assert e == s.key_events(0)["emitted"] > d
                if checked == 0:
                    reg = s.record(0)
                    assert reg[4] == 0, "an exact record is never dirty"
                    shapes.add((int(reg[1]), bool(reg[3])))  # pending, lattice in the workspace
                rec = s.set_record(0)
                got = [(s.state_value(0, int(c >> np.uint64(56))), int(c & np.uint64((1 << 56) - 1))) for c in rec["configs"]]
                assert len(set(got)) == len(got) == rec["header"][1], "the set record holds a config twice"
                assert set(got) == TS.oracle_set(ev, e), f"key {k} ({cut}), {e} events: {len(got)} configs"
                assert rec["header"][4] == e
                checked += 1
            assert checked >= 1, f"key {k}: the set record was never read"
            reads.append(checked)
            s.finish()
            orc = cref.check_history(hist.as_c(), budget=1 << 20, threads=1)[1]
            assert record(s.results()) == oracle_record(orc), f"key {k}"
            s.close()
    assert sum(r >= 2 for r in reads) >= 3, reads
    assert (10, True) in shapes and any(n <= 6 and not in_ws for n, in_ws in shapes), shapes


# ---------------------------------------------------------------- 3. budget edges inside the set tier
def first_past(sI, sS, budget):
    return int(np.flatnonzero((sI > budget) | (sS > budget))[0])


def feed_around(s, h, rs, key, e, after=None):
    """Append h (one key) cut before, at and after the call that emits event e;
    after(rows appended, update) follows each call, and all of them are returned."""
    r = rs.ready[key][e]
    assert 1 < r < len(h) and rs.emitted(key, r - 1) <= e < rs.emitted(key, r)
    out = []
    for lo, hi in ((0, r - 1), (r - 1, r), (r, min(r + 5, len(h))), (min(r + 5, len(h)), len(h))):
        if lo < hi:
            out.append((hi, s.append(S.rows(h, lo, hi))))
            if after is not None:
                after(*out[-1])
    return out


@pytest.mark.parametrize("name,key,defer_at,need,event", [("long", 15, 376, 624, 393), ("long", 48, 312, 660, 313),
                                                          ("B", 0, 194, 648, 196)])
def test_budget_edges_inside_the_set_tier(name, key, defer_at, need, event):
    """At need - 1 the key is :unknown / budget at the oracle's event, in the
    call that reaches it -- cuts before, at and after it -- with the canonical
    selection of the set standing before that event; at need it gets its
    unbounded record, peak included."""
    h, full, rs, sI, sS = one_key(name, key)
    ev = rs.events[key]
    assert rs.defer_at[key] == defer_at < event and max(sI.max(), sS.max()) == need == sI[event]
    assert first_past(sI, sS, need - 1) == event and full["valid"][0] == 1
    if key == 48:
        assert not any(x[0] for x in ev[defer_at:event]) and ev[event][0], "the first :ok after the migration"
    for budget in (need - 1, need):
        d = Device(0, budget=budget)
        for plain in (dict(), dict(set_tier=True)):
            with pytest.raises(N.LincheckError, match="unsupported"):
                Stream(d, **plain)  # without exact such a budget is still refused
        s = Stream(d, exact=True, set_tier=True)
        label = f"{name} {key} at budget {budget}"

        def after(n_rows, up):
            res = s.results()
            assert not up.invalid and up.n_deferred == 0
            if budget == need or rs.emitted(key, n_rows) <= event:
                assert record(res)[:3] == (1, 0, -1) and res.n_final[0] == 0, f"{label}, {n_rows} rows: {record(res)}"
                assert s.key_tier(0) == ("set" if rs.emitted(key, n_rows) > defer_at else "register")
                assert 1 <= res.peak[0] <= full["peak"][0]
            else:  # from the call that reaches the event on
                assert record(res)[:3] == (-1, BUDGET, event), f"{label}, {n_rows} rows: {record(res)}"
                assert s.key_tier(0) == "dead" and s.set_stats()["pool_in_use"] == 0
                same_selection(s, res, 0, TS.oracle_set(ev, event), d.max_final, label)

        calls = feed_around(s, h, rs, key, event, after)
        assert len(calls) == 4
        up = s.finish()
        res = s.results()
        want = oracle_record(cref.check_history(h.as_c(), budget=budget, threads=1)[1])
        assert not up.invalid and up.n_deferred == 0
        if budget == need - 1:
            assert record(res)[:3] == want[:3] == (-1, BUDGET, event)
        else:
            assert record(res) == want == oracle_record(full), f"{label}: {record(res)}"
            assert s.key_tier(0) == "set"
        s.close()


@pytest.mark.parametrize("budget", [CAP, CAP + 1])
def test_the_cap_and_the_budget_meet_in_the_oracle_s_order(budget):
    """long 8: at budget = cap it is :unknown / budget inside the set tier, at
    the oracle's event for that budget; at cap + 1 the oracle's first size
    above the budget is above the cap too, so the key falls back and finish
    returns the same record."""
    h, full, rs, sI, sS = one_key("long", 8)
    assert rs.defer_at[8] == 240 and full["peak"][0] == 12288 and sI.max() == 43520
    e = first_past(sI, sS, budget)
    assert e > 240 and max(sI[:e].max(), sS[:e].max()) <= CAP, "nothing before the deciding event passes the cap"
    want = oracle_record(cref.check_history(h.as_c(), budget=budget, threads=1)[1])
    assert want[:3] == (-1, BUDGET, e)
    d = Device(0, budget=budget)
    s = Stream(d, exact=True, set_tier=True)
    calls = feed_around(s, h, rs, 8, e)
    res = s.results()
    assert not any(up.invalid for _, up in calls)
    if budget == CAP:
        assert record(res)[:3] == (-1, BUDGET, e) and s.key_tier(0) == "dead" and calls[-1][1].n_deferred == 0
        assert res.n_final[0] == d.max_final
    else:
        assert max(sI[e], sS[e]) > CAP
        assert record(res)[:3] == (1, 0, -1) and s.key_tier(0) == "fallen_back" and calls[-1][1].n_deferred == 1
    s.finish()
    assert record(s.results())[:3] == want[:3]
    assert s.set_stats()["pool_in_use"] == 0
    s.close()


# ---------------------------------------------------------------- 4. final configs
def test_final_configs_of_dead_and_live_set_tier_keys(dev):
    h, keys, orc, rs, runs = selection()
    s = Stream(dev, exact=True, set_tier=True)
    i51 = keys.index(51)
    seen = {}

    def after(n_rows, up):
        if i51 in up.invalid:
            seen[i51] = s.results()
        elif i51 not in seen and up.n_keys > i51 and s.key_tier(i51) == "set":
            res = s.results()  # a live set-tier key: its peak so far, no configs
            assert res.n_final[i51] == 0 and not res.final[i51].any() and 1 <= res.peak[i51] <= 768

    S.feed(s, h, 640, after)
    assert i51 in seen, "long 51 was not reported online"
    res = seen[i51]
    assert record(res, i51) == (0, 1, 187, 768)
    oset = TS.oracle_set(rs.events[51], 187)
    same_selection(s, res, i51, oset, dev.max_final, "long 51, dead at 187")
    s.finish()
    res = s.results()
    assert got_configs(s, res, i51) == got_configs(s, seen[i51], i51)
    live = [i for i in runs if s.key_tier(i) == "set"]
    assert sorted(keys[i] for i in live) == [2, 15, 48]
    for i in live:
        ev = rs.events[keys[i]]
        same_selection(s, res, i, TS.oracle_set(ev, len(ev)), dev.max_final, f"long {keys[i]}, live at the end")
        assert res.peak[i] == orc["peak"][i]
    s.close()


# ---------------------------------------------------------------- 5. analysis online
def test_analysis_in_the_append_that_reports_a_set_tier_key(dev):
    h, keys, orc, rs, _runs = selection()
    ops = h.to_ops()
    lin = CK.linearizable({"model": model.cas_register(), "algorithm": "linear"})
    i51 = keys.index(51)
    s = Stream(dev, exact=True, set_tier=True)
    seen = []

    def after(n_rows, up):
        if i51 not in up.invalid:
            return
        assert rs.defer_at[51] < orc["fail_event"][i51] and s.key_events(i51)["deferred_at"] == rs.defer_at[51]
        m = s.analysis(i51, S.rows(h, 0, n_rows))
        sub = LR.subhistory(ops, 51)
        want = lin.check({}, sub)
        a = LR.analysis(sub, model="cas-register")
        assert a.valid is False and a.fail_event == 187
        assert m["valid?"] is False and want["valid?"] is False
        for f in ("op", "previous-ok", "last-op"):
            assert m[f] == want[f], f"{f}: {m[f]}, the checker's {want[f]}"
        exp_cfgs = {(st, frozenset(sub[a.ops[q].invoke_pos]["index"] for q in L)) for st, L in a.final_configs}
        got_cfgs, want_cfgs = ([config_tuple(c, "cas-register") for c in x["configs"]] for x in (m, want))
        assert len(set(got_cfgs)) == len(got_cfgs) == len(want_cfgs) == min(10, len(exp_cfgs))
        assert set(got_cfgs) <= exp_cfgs
        exp_paths = LR.final_paths(a, sub, "cas-register")
        got_paths = {path_tuple(p, "cas-register") for p in m["final-paths"]}
        assert len(got_paths) == len(m["final-paths"]) == len(want["final-paths"]) > 0
        if exp_paths is not None:
            assert got_paths <= exp_paths
        seen.append(n_rows)

    S.feed(s, h, 64, after)
    assert len(seen) == 1
    s.close()


# ---------------------------------------------------------------- 6. one context
def test_an_exact_set_stream_a_plain_set_stream_and_a_batch_check_share_a_context(dev):
    h, keys, orc, _rs, _runs = selection()
    hb, keysb, orcb, _ = TS.case("B")
    hi, keysi, orci, _ = TS.case("I")
    pki = Packed(hi)
    a, b = Stream(dev, exact=True, set_tier=True), Stream(dev, set_tier=True)
    for lo in range(0, max(len(h), len(hb)), 400):
        if lo < len(h):
            a.append(S.rows(h, lo, min(len(h), lo + 400)))
        r = dev.check(pki)
        for f in FIELDS:
            assert np.array_equal(getattr(r, f), orci[f]), f
        if lo < len(hb):
            b.append(S.rows(hb, lo, min(len(hb), lo + 400)))
    assert a.tiers()["set"] >= 1 and b.tiers()["set"] >= 1
    a.finish(), b.finish()
    res = a.results()
    for i in range(len(keys)):
        assert record(res, i) == oracle_record(orc, i), f"the exact stream, key {keys[i]}"
    TS.final_equal(b, keysb, orcb, "the plain set-tier stream")
    resb = b.results()
    assert resb.peak is None and resb.final is None and resb.n_final is None
    n = len(keysb)
    valid, fev, cause = np.zeros(n, np.int8), np.zeros(n, np.int32), np.zeros(n, np.uint8)
    peak, n_final = np.full(n, 0xABCD, np.uint32), np.full(n, 0xABCD, np.uint32)
    final = np.full((n, dev.max_final, 2), 0xABCD, np.uint64)
    r = N.LcResult()
    r.valid, r.fail_event, r.cause = N.ptr(valid, C.c_int8), N.ptr(fev, C.c_int32), N.ptr(cause, C.c_uint8)
    r.peak_configs, r.n_final, r.final_configs = N.ptr(peak, C.c_uint32), N.ptr(n_final, C.c_uint32), N.ptr(final, C.c_uint64)
    N.check(N.lib().lc_stream_results(b.handle, C.byref(r)))
    assert np.array_equal(valid, orcb["valid"])
    assert (peak == 0xABCD).all() and (n_final == 0xABCD).all() and (final == 0xABCD).all()
    a.close(), b.close()
