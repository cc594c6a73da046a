"""The resident set tier of a stream on the device (LC_STREAM_SET_TIER:
k_stream_migrate and k_stream_set in csrc/device_stream_set.hip, the host's
side in csrc/host_stream.cpp).  Expected values come from the oracle
(oracle/linear_ref.c through cref, oracle/linear_ref.py) or from one-shot
Device.check, never from a stream: a key that leaves the register tier must
turn invalid in the very append whose decided prefix holds its failing :ok,
every split must end with the one-shot records, and a migrated record must lie
between the oracle's exact config set and its closure."""
import numpy as np
import pytest

import cref
import edgegen as E
import linear_ref as LR
import stream_helpers as S
import stream_set_rule as R
from lincheck import _native as N
from lincheck import history as H
from lincheck.checker import Device, Packed
from lincheck.stream import Stream

pytestmark = pytest.mark.gpu

NEVER = np.int64(1) << 40
HISTORIES = {
    "info2": dict(n_keys=100, ops_per_key=100, concurrency=10, interleave=True, nemesis_period=5.0, info_rate=0.02,
                  anomaly_rate=0.1, seed=11),
    "info5": dict(n_keys=100, ops_per_key=100, concurrency=10, interleave=True, nemesis_period=5.0, info_rate=0.05,
                  anomaly_rate=0.1, seed=12),
    "long": dict(n_keys=60, ops_per_key=300, concurrency=10, info_rate=0.02, anomaly_rate=0.2, seed=13),
    "B": dict(n_keys=12, ops_per_key=150, concurrency=10, interleave=True, nemesis_period=5.0, anomaly_rate=0.3,
              info_rate=0.02, seed=3),
    "I": dict(n_keys=24, ops_per_key=120, concurrency=10, interleave=True, nemesis_period=5.0, anomaly_rate=0.3, seed=3),
}
_case = {}


@pytest.fixture(scope="module")
def dev():
    return Device(0)


def failing(orc):
    return np.where(orc["valid"] == 0, orc["fail_event"].astype(np.int64), NEVER)


def case(name):
    """(history, keys, the oracle's records, the decided-prefix restatement), built once."""
    if name not in _case:
        if name == "long12":  # 12 keys of "long": the one that fails after leaving the tier, leaving ones, others
            h, keys, orc, rs = case("long")
            late = [k for i, k in enumerate(keys) if orc["valid"][i] == 0 and 0 <= rs.defer_at[k] < orc["fail_event"][i]]
            left = [k for k in keys if rs.defer_at[k] >= 0 and k not in late]
            stay = [k for k in keys if rs.defer_at[k] < 0]
            h = h.select_keys(late[:1] + left[:7] + stay[:4])
        else:
            h = H.synth(**HISTORIES[name])
        keys, orc = cref.check_history(h.as_c(), budget=1 << 20, threads=8)
        _case[name] = (h, list(keys), orc, S.Restated(h))
    return _case[name]


def final_equal(s, keys, orc, label):
    res = s.results()
    assert res.keys == keys
    for f in ("valid", "cause", "fail_event"):
        got, want = getattr(res, f), orc[f]
        bad = np.flatnonzero(got != want)
        assert not len(bad), f"{label}: {f} differs at keys {bad[:8]}: stream {got[bad[:8]]}, oracle {want[bad[:8]]}"


def run_online(dev, name, step):
    """Feed `name` step rows at a time with the set tier on.  After every
    append the invalid keys are exactly those whose decided prefix (no defer_at
    cap: the search goes on past the register tier) holds the oracle's failing
    :ok, but for keys that fell back, whose verdict waits for finish."""
    h, keys, orc, rs = case(name)
    fev = failing(orc)
    s = Stream(dev, set_tier=True)
    invalid, seen_at = set(), {}

    def after(n_rows, up):
        for i in up.invalid:
            assert i not in invalid, f"{name}: key index {i} turned invalid twice"
            seen_at[i] = n_rows
        invalid.update(up.invalid)
        want = {i for i in range(up.n_keys) if rs.emitted(keys[i], n_rows) > fev[i]}
        fallen = {i for i in want if s.key_tier(i) == "fallen_back"}
        assert invalid == want - fallen, f"{name}, {n_rows} rows: invalid {sorted(invalid)}, oracle says {sorted(want)}"

    S.feed(s, h, step or len(h), after)
    return s, seen_at


# ---------------------------------------------------------------- 1. online past the tier
def test_a_key_past_the_register_tier_turns_invalid_online(dev):
    """The long history has a key whose failing :ok lies past the invoke that
    takes window slot 10 (asserted from the oracle).  With the set tier, appends
    of 50 rows report it in an Update before finish, in the first append whose
    decided prefix holds that :ok.  (Without the set tier it is reported by
    finish.)"""
    h, keys, orc, rs = case("long")
    fev = failing(orc)
    late = [i for i, k in enumerate(keys) if orc["valid"][i] == 0 and 0 <= rs.defer_at[k] < fev[i]]
    assert late, "the oracle has no key that fails after leaving the register tier"
    s, seen_at = run_online(dev, "long", 50)
    for i in late:
        first = next(n for n in list(range(50, len(h), 50)) + [len(h)] if rs.emitted(keys[i], n) > fev[i])
        assert seen_at.get(i) == first, f"key index {i}: reported at {seen_at.get(i)} rows, its failing :ok is decided at {first}"
        assert s.key_tier(i) == "dead" and s.key_events(i)["deferred_at"] == rs.defer_at[keys[i]]
        assert s.results().fail_event[i] == orc["fail_event"][i]
    s.finish()
    final_equal(s, keys, orc, "long, 50 rows")
    s.close()


# ---------------------------------------------------------------- 2. final records, every split
@pytest.mark.parametrize("name,step", [("info2", 640), ("info2", 0), ("info5", 640), ("info5", 0), ("long", 640), ("long", 0),
                                       ("long12", 1), ("long12", 7), ("long12", 64), ("B", 7)])
def test_final_records_equal_the_oracle_s_for_every_split(dev, name, step):
    h, keys, orc, rs = case(name)
    s, _ = run_online(dev, name, step)
    up = s.finish()
    final_equal(s, keys, orc, f"{name}, step {step}")
    t = s.tiers()
    assert sum(t.values()) == len(keys) and up.n_deferred == t["fallen_back"]
    # the device's sets lie between the exact ones and the closed ones: so do the keys that fall back
    runs = {i: R.Run(rs.events[k]) for i, k in enumerate(keys) if rs.defer_at[k] >= 0}
    may = {i for i, r in runs.items() if r.falls_back}
    must = {i for i in may if R.Run(rs.events[keys[i]], closed=False).falls_back}
    fell = {i for i in runs if s.key_tier(i) == "fallen_back"}
    assert must <= fell <= may, f"{name}: fell back {sorted(fell)}, exact sets say {sorted(must)}, closed sets {sorted(may)}"
    assert s.set_stats()["pool_in_use"] == t["set"]
    s.close()


# ---------------------------------------------------------------- 3. migration at each lattice shape
def oracle_set(events, e):
    """The oracle's exact config set after events[:e] of a key, as {(value, slot
    mask)}: linear_ref.analysis of those events followed by a read no state
    satisfies reports, at that read, the set it held (final_configs)."""
    sub, proc = [], {}
    for j, (is_ok, slot, op, _row) in enumerate(events[:e]):
        if not is_ok:
            proc[slot] = j
        sub.append({"type": "ok" if is_ok else "invoke", "f": R.F_NAME[op[0]] if op else None,
                    "value": R.op_value(op) if op else None, "process": proc[slot]})
        if is_ok:
            sub[-1]["f"], sub[-1]["value"] = sub[proc[slot]]["f"], sub[proc[slot]]["value"]
    sub += [{"type": "invoke", "f": "read", "value": 987654321, "process": -1},
            {"type": "ok", "f": "read", "value": 987654321, "process": -1}]
    a = LR.analysis(sub)
    assert a.valid is False and a.fail_event == e + 1, "the prefix itself is not linearizable"
    return {(st, sum(1 << a.final_slots[q] for q in L)) for st, L in a.final_configs}


MIGRATION_KEYS = [
    # name, plan, the batch's values: keys that take window slot 10 with 10 ops pending -- the lattice in the
    # walk's workspace, nothing closed since the ops were invoked -- first thing, after many :oks, with a crashed
    # write among the pending ops; and one that interns its 33rd state with 5 pending (the lattice in a register)
    ("first-thing", lambda: E.Plan(40, E.counts(40, 11, drain=True))),
    ("bump-to-11", lambda: E.Plan(60, E.counts(60, 10, bumps=[(31, 11)], drain=True))),
    # (an odd event count: the crashed write is the one op still pending at the end)
    ("rolling-10-crashed-write", lambda: E.Plan(61, E.counts(61, 11, drain=True, stuck=1), crash={2: 14},
                                                kinds={2: "write"}, apply_at={2: 50}, distinct={2: 1})),
    ("crashed-late-bump", lambda: E.Plan(65, E.counts(65, 10, bumps=[(41, 11)], drain=True, stuck=1), crash={3: 12},
                                         kinds={3: "write"}, apply_at={3: 56}, distinct={3: 1})),
]


def migration_batches():
    if "mig" not in _case:
        slot = E.batch([(n, p()) for n, p in MIGRATION_KEYS], seed=31)
        states = E.batch([("states-33", E.rolling(400, 5))], seed=32, values=range(60), stale=60, garbage=99)
        _case["mig"] = [(b, S.Restated(b.hist)) for b in (slot, states)]
    return _case["mig"]


@pytest.mark.parametrize("cut", ["before", "after"])
def test_migration_at_each_lattice_shape(dev, cut):
    """Cut the stream immediately before (the append ends with the last event
    of the register tier) and immediately after the migrating invoke (the
    append that first emits it); after the migrating append the set record's
    configs are a superset of the oracle's exact set and a subset of its
    closure under the ops then pending, and so they stay as rows go on."""
    shapes, reads = set(), []
    for b, rs in migration_batches():
        for k in b.pk.keys:
            ev, d = rs.events[k], rs.defer_at[k]
            assert d >= 0 and rs.ready[k][d] < S.NEVER, f"key {k} never leaves the register tier before finish"
            hist = b.hist.select_keys([k])
            at = rs.ready[k][d] if cut == "after" else rs.ready[k][d] - 1  # rows of the key appended (it is alone)
            row_of = np.flatnonzero(b.hist.key == k)
            n1 = int(np.searchsorted(row_of, at))  # (the batch is key-major)
            s = Stream(dev, set_tier=True)
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
                    shapes.add((int(reg[1]), bool(reg[3]), bool(reg[4])))  # pending, lattice in the workspace, dirty
                rec = s.set_record(0)
                got = {(s.state_value(0, int(c >> np.uint64(56))), int(c & np.uint64((1 << 56) - 1))) for c in rec["configs"]}
                assert len(got) == len(rec["configs"]) == rec["header"][1], "the set record holds a config twice"
                exact = oracle_set(ev, e)
                pend = {}
                for is_ok, slot, op, _row in ev[:e]:
                    if is_ok:
                        del pend[slot]
                    else:
                        pend[slot] = R.Stepper(op)
                assert exact <= got <= R.close(exact, pend), f"key {k} ({cut}), {e} events: {len(got)} configs"
                pending = sum(1 << q for q in pend)
                assert int(rec["header"][2]) | int(rec["header"][3]) << 32 == pending and rec["header"][4] == e
                checked += 1
            assert checked >= 1, f"key {k}: the set record was never read"
            reads.append(checked)
            s.finish()
            orc = cref.check_history(hist.as_c(), budget=1 << 20, threads=1)[1]
            final_equal(s, [k], orc, f"key {k}")
            s.close()
    assert sum(r >= 2 for r in reads) >= 3, f"set records read again as rows went on: {reads}"
    # 10 pending, the lattice in the workspace, dirty; and a lane-phase record: in a register, closed at its last :ok
    assert (10, True, True) in shapes and any(n <= 6 and not in_ws and not dirty for n, in_ws, dirty in shapes), shapes


# ---------------------------------------------------------------- 4. fallback
@pytest.mark.parametrize("budget", [65536, 1 << 20])
def test_keys_the_set_tier_cannot_hold_fall_back(budget):
    """Concurrency 30 with crashed ops: every key leaves the register tier and
    then outgrows the set tier (or dies in it).  The final records are
    Device.check's at the same budget -- where that gives up, so did the set
    tier, earlier -- and the pool's slots were handed on from key to key."""
    h = H.synth(8, 300, concurrency=30, info_rate=0.02, anomaly_rate=0.5, seed=4)
    dev = Device(0, budget=budget)
    want = dev.check(Packed(h), verdicts_only=True)
    s = Stream(dev, set_tier=True)
    S.feed(s, h, 500)
    up = s.finish()
    t = s.tiers()
    assert t["register"] == 0 and t["set"] == 0 and t["fallen_back"] + t["dead"] == 8, t
    assert up.n_deferred == t["fallen_back"] >= 1
    res = s.results()
    for f in ("valid", "cause", "fail_event"):
        assert np.array_equal(getattr(res, f), getattr(want, f)), f
    st = s.set_stats()
    migrated = sum(s.key_events(i)["deferred_at"] >= 0 for i in range(8))
    assert migrated == 8 and st["pool_in_use"] == 0 and 1 <= st["pool_peak"] < migrated, st
    s.close()


# ---------------------------------------------------------------- 5. option off
def test_option_off_is_the_stream_as_it_was(dev):
    h, keys, orc, rs = case("B")
    s = Stream(dev)
    S.feed(s, h, 50)
    assert s.tiers()["set"] == 0 and s.set_stats()["pool_slots"] == 0
    up = s.finish()
    assert up.n_deferred == 1
    t = s.tiers()
    # the two invalid keys were found online, the deferred key is valid: checked at finish
    assert t == {"register": len(keys) - 3, "set": 0, "fallen_back": 1, "dead": int((orc["valid"] == 0).sum())} and t["dead"] == 2, t
    with pytest.raises(N.LincheckError, match="invalid"):
        s.set_record(0)
    final_equal(s, keys, orc, "B, option off")
    s.close()


# ---------------------------------------------------------------- 6. one context
def test_a_migrated_stream_a_second_stream_and_a_batch_check_share_a_context(dev):
    h, keys, orc, _rs = case("long12")
    hi, keysi, orci, _ = case("I")
    hb, keysb, orcb, _ = case("B")
    pk = Packed(hb)
    a, b = Stream(dev, set_tier=True), Stream(dev)
    for lo in range(0, max(len(h), len(hi)), 400):
        if lo < len(h):
            a.append(S.rows(h, lo, min(len(h), lo + 400)))
        r = dev.check(pk, verdicts_only=True)
        assert np.array_equal(r.valid, orcb["valid"]) and np.array_equal(r.fail_event, orcb["fail_event"])
        if lo < len(hi):
            b.append(S.rows(hi, lo, min(len(hi), lo + 400)))
    assert a.tiers()["set"] + a.tiers()["dead"] >= 1 and a.set_stats()["pool_peak"] >= 1
    a.finish(), b.finish()
    final_equal(a, keys, orc, "the migrated stream")
    final_equal(b, keysi, orci, "the second stream")
    a.close(), b.close()
