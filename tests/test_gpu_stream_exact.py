"""The exact mode of a stream on the device (LC_STREAM_EXACT: k_stream_exact and
k_stream_final in device_stream_exact.hip, csrc/host_stream.cpp).  Expected
values come from the oracle (oracle/linear_ref.c through cref: valid, cause,
fail_event, peak) and from the one-shot Device.check with peaks and final
configs (final, n_final), which test_gpu_parity.py / test_gpu_configs.py pin
against the oracle.  The batches are tests/test_gpu_stream.py's.

Final configs carry state ids.  In events mode the stream searches lc_pack's
own words, so its records are the one-shot's word for word.  In rows mode the
stream's packer numbers a key's states itself (every value an op names, per
key) while lc_pack shares one numbering over the batch, so there the configs
are compared decoded to register values: write_final_mem orders by (slot mask,
state id), so the masks come in the same order in both, each mask's values are
the same set, and only a mask group cut by max_final may hold other members of
the same group."""
import ctypes as C

import numpy as np
import pytest

import edgegen as E
import linear_ref as LR
import stream_helpers as S
from helpers import config_tuple, path_tuple
from lincheck import _native as N
from lincheck import checker as CK
from lincheck import model
from lincheck.checker import Device, Packed
from lincheck.stream import Stream
from test_gpu_budget_edges import REG_BY_S, REG_BY_S_PENDING, REG_P, band, register_target
from test_gpu_stream import WANTED, failing, rows_case, seams, source

pytestmark = pytest.mark.gpu

BUDGET = 2  # LC_CAUSE_BUDGET
FIELDS = ("valid", "cause", "fail_event", "peak")


@pytest.fixture(scope="module")
def dev():
    return Device(0)


_one = {}


def one_shot(dev, name, pk):
    """Device.check with peaks and final configs, once per batch."""
    if name not in _one:
        _one[name] = dev.check(pk)
    return _one[name]


def same_record(res, i, orc, one, k, label):
    """Key index i of a stream's results against batch key k: the oracle's
    verdict and peak, the one-shot check's final configs, word for word."""
    got = tuple(int(getattr(res, f)[i]) for f in FIELDS)
    want = tuple(int(orc[f][k]) for f in FIELDS)
    assert got == want, f"{label}: (valid, cause, fail_event, peak) {got}, oracle {want}"
    assert int(res.n_final[i]) == int(one.n_final[k]), f"{label}: n_final {res.n_final[i]}, one-shot {one.n_final[k]}"
    n = int(one.n_final[k])
    assert res.final[i, :n].tolist() == one.final[k, :n].tolist(), f"{label}: final configs"
    assert not res.final[i, n:].any(), f"{label}: words past n_final"


def push_exact(dev, src, one, cuts, label, words16=False, first_call=None, budget_dead=None):
    """test_gpu_stream.push_schedule on an exact stream: after every call the
    invalid keys are exactly those whose pushed prefix passes the oracle's
    failing event, a key that just died has its whole one-shot record, and a
    live key has a peak no larger than its final one and no configs yet.
    budget_dead: {key: event} of the keys the oracle gives up on at the
    stream's budget (:unknown, never on the invalid list)."""
    K = src.pk.n_keys
    budget_dead = budget_dead or {}
    s = Stream(dev, exact=True)
    pushed = np.zeros(K, np.int64)
    pos = [0] * K
    invalid, dead = set(), set()
    n_calls = max(len(c) - 1 + (first_call or {}).get(k, 0) for k, c in enumerate(cuts))
    for j in range(n_calls):
        parts = []
        for k in range(K):
            if j < (first_call or {}).get(k, 0) or pos[k] + 1 >= len(cuts[k]):
                continue
            lo, hi = cuts[k][pos[k]], cuts[k][pos[k] + 1]
            pos[k] += 1
            parts.append((k, lo, hi))
            pushed[k] = hi
        b, ids = src.chunk(parts, words16)
        up = s.push(b, ids)
        index = {key: i for i, key in enumerate(s.keys)}
        turned = {src.pk.keys.index(s.keys[i]) for i in up.invalid}
        assert not (turned & invalid), f"{label}, call {j}: a key turned invalid twice"
        invalid |= turned
        want = {k for k in range(K) if pushed[k] > src.fev[k] and k not in budget_dead}
        assert invalid == want, f"{label}, call {j}: invalid {sorted(invalid)}, oracle says {sorted(want)}"
        gave_up = {k for k, e in budget_dead.items() if pushed[k] > e}
        res = s.results()
        for k in (turned | gave_up) - dead:
            same_record(res, index[src.pk.keys[k]], src.orc, one, k, f"{label}, call {j}, key {k} just died")
            assert s.key_tier(index[src.pk.keys[k]]) == "dead"
        dead |= turned | gave_up
        for key, i in index.items():
            k = src.pk.keys.index(key)
            if k not in dead:
                assert (res.valid[i], res.n_final[i]) == (1, 0) and 1 <= res.peak[i] <= src.orc["peak"][k], f"{label}, live key {k}"
    return s


def final_equal(s, src, one, label, skip_empty=False):
    s.finish()
    res = s.results()
    if not skip_empty:
        assert sorted(res.keys) == sorted(src.pk.keys)  # (in order of first appearance in the stream)
    for i, key in enumerate(res.keys):
        k = src.pk.keys.index(key)
        same_record(res, i, src.orc, one, k, f"{label}, finished, key {k}")
    if skip_empty:  # keys without events never reach a stream in events mode
        assert set(src.pk.keys) - set(res.keys) == {src.pk.keys[k] for k in range(src.pk.n_keys) if src.nev[k] == 0}


# ---------------------------------------------------------------- seams
@pytest.mark.parametrize("name", ["profiles", "anomalies", "states32"])
def test_cuts_at_every_seam_of_the_walk(dev, name):
    src = source(name)
    one = one_shot(dev, name, src.pk)
    cuts, seen = [], set()
    for k in range(src.pk.n_keys):
        c = E.pending_before(src.pk, k).tolist()
        sm = seams(c, int(src.fev[k]) if src.fev[k] < (1 << 40) else len(c))
        seen |= set(sm)
        cuts.append(sorted({0, len(c) - 1} | set(sm.values())))
    if name == "profiles":
        assert not set(WANTED) - seen, f"no key is cut at: {sorted(set(WANTED) - seen)}"
    s = push_exact(dev, src, one, cuts, name)
    final_equal(s, src, one, name)
    s.close()


# ---------------------------------------------------------------- cursor
@pytest.mark.parametrize("size", [63, 64, 65, 128, 129, 200])
def test_chunk_sizes_around_the_cursor(dev, size):
    src = source("profiles")
    one = one_shot(dev, "profiles", src.pk)
    cuts = [sorted(set(range(0, n, size)) | {int(n)}) for n in src.nev]
    s = push_exact(dev, src, one, cuts, f"chunks of {size}", words16=size % 2 == 0, first_call={3: 4})
    assert s.keys[-1] == src.pk.keys[3], "key 3 joins the stream last, in its fifth call"
    final_equal(s, src, one, f"chunks of {size}")
    s.close()


def test_one_event_per_push(dev):
    src = source("small")
    one = one_shot(dev, "small", src.pk)
    assert 60 in src.nev
    cuts = [list(range(int(n) + 1)) for n in src.nev]
    s = push_exact(dev, src, one, cuts, "one event per push")
    final_equal(s, src, one, "one event per push", skip_empty=True)
    s.close()


# ---------------------------------------------------------------- budget edges
def budget_targets():
    return [("register", P) for P in REG_P] + [("register_by_S", n) for n in range(len(REG_BY_S))]


@pytest.mark.parametrize("which,arg", budget_targets())
def test_budget_edges(which, arg):
    """A register-tier key whose largest set is need: at need - 1 it is
    :unknown / budget at the oracle's event, in the call that reaches it --
    cuts before, at and after the deciding event -- and at need it gets its
    unbounded record.  Targets decided by |I| (at the failing :ok for 6-10
    pending), and by |S'| at 9, 7 and 4 pending.  Every other key of the band
    is checked against the oracle at the same budget beside it."""
    from test_gpu_stream import Source
    b = band(which)
    if which == "register":
        i, _at_fail = register_target(b, arg)
        e, nI, _nS, pend = b.deciding(i)
        assert pend == arg and nI == b.need[i], f"{b.names[i]}: {pend} pending, |I| {nI} at the deciding :ok"
    else:
        i = arg
        e, _nI, nS, pend = b.deciding(i)
        assert pend == REG_BY_S_PENDING[arg] and nS == b.need[i] and b.sizes[i][0].max() < b.need[i], b.describe(i)
    assert b.pend[i].max() <= E.T0_MAX_WIDTH
    need = b.need[i]
    sI, sS = b.sizes[i]
    first = int(np.flatnonzero((sI > need - 1) | (sS > need - 1))[0])
    assert first == e and 1 < need < 16 * 64 * 32
    full = b.oracle(1 << 40)
    for budget in (need - 1, need):
        d = Device(0, budget=budget)
        with pytest.raises(N.LincheckError, match="unsupported"):
            Stream(d)  # without the flag such a budget is still refused
        src = Source(b.hist, b.pk)
        src.orc = b.oracle(budget)
        src.fev = failing(src.orc)
        one = d.check(b.pk)
        gave_up = {k: int(src.orc["fail_event"][k]) for k in np.flatnonzero(src.orc["cause"] == BUDGET)}
        # (the oracle's peak of a key it gave up on is not the device's business: test_gpu_budget_edges.same_as_oracle)
        src.orc = src.orc.copy()
        src.orc["peak"][list(gave_up)] = one.peak[list(gave_up)]
        cuts = [sorted({0, min(first, int(n)), min(first + 1, int(n)), int(n)}) for n in src.nev]
        s = push_exact(d, src, one, cuts, f"{b.names[i]} at {budget}", budget_dead=gave_up)
        final_equal(s, src, one, f"{b.names[i]} at {budget}")
        res = s.results()
        got = (int(res.valid[i]), int(res.cause[i]), int(res.fail_event[i]))
        if budget == need - 1:
            assert got == (-1, BUDGET, first), f"{b.names[i]} at need - 1: {got}"
            assert s.key_tier(i) == "dead"
        else:
            assert got + (int(res.peak[i]),) == tuple(int(full[f][i]) for f in FIELDS), f"{b.names[i]} at need: {got}"
        s.close()


# ---------------------------------------------------------------- rows mode
def decoded(final, n, value):
    return [(int(final[c, 0]), int(final[c, 1]) & ((1 << 48) - 1), value(int(final[c, 1]) >> 48)) for c in range(n)]


def same_configs(got, want, max_final, label):
    """Two final-config lists decoded to register values (module docstring)."""
    assert len(got) == len(want), f"{label}: n_final {len(got)}, one-shot {len(want)}"
    assert [c[:2] for c in got] == [c[:2] for c in want], f"{label}: slot masks"
    masks = list(dict.fromkeys(c[:2] for c in want))
    for m in masks:
        if len(want) == max_final and m == masks[-1]:
            continue  # perhaps cut by max_final: its members may differ, their count (above) may not
        assert {c[2] for c in got if c[:2] == m} == {c[2] for c in want if c[:2] == m}, f"{label}: values under mask {m}"


def run_rows(dev, name, step, deferred=0):
    h, keys, orc, rs = rows_case(name)
    pk = Packed(h)
    one = one_shot(dev, "rows " + name, pk)
    fev = failing(orc)
    s = Stream(dev, exact=True)
    invalid = set()

    def after(n_rows, up):
        invalid.update(up.invalid)
        searched = [min(rs.emitted(k, n_rows), rs.defer_at[k] if rs.defer_at[k] >= 0 else 1 << 40) for k in keys[:up.n_keys]]
        want = {i for i, e in enumerate(searched) if e > fev[i]}
        assert invalid == want, f"{name}, {n_rows} rows: invalid {sorted(invalid)}, oracle says {sorted(want)}"

    S.feed(s, h, step or len(h), after)
    up = s.finish()
    assert up.n_deferred == deferred
    res = s.results()
    assert res.keys == keys == pk.keys
    for f in FIELDS:
        assert np.array_equal(getattr(res, f), orc[f]), f"{name}, step {step}: {f}"
    assert np.array_equal(res.n_final, one.n_final), f"{name}, step {step}: n_final"
    for i in range(len(keys)):
        same_configs(decoded(res.final[i], int(res.n_final[i]), lambda st: s.state_value(i, st)),
                     decoded(one.final[i], int(one.n_final[i]), lambda st: pk.state_value(i, st)),
                     dev.max_final, f"{name}, step {step}, key {i}")
    return s, orc


@pytest.mark.parametrize("step", [7, 64, 640, 0])
@pytest.mark.parametrize("name", ["A", "A-merged", "I"])
def test_rows_mode_final_records(dev, name, step):
    s, orc = run_rows(dev, name, step)
    assert (orc["valid"] == 0).sum() == {"A": 8, "A-merged": 8, "I": 3}[name]
    s.close()


def test_deferred_key_gets_its_record_from_the_batch_path(dev):
    """B: one key passes 10 pending ops (window slot 10) and is checked at
    finish through lc_check_batch, peaks and final configs requested."""
    s, orc = run_rows(dev, "B", 50, deferred=1)
    deferred = [i for i in range(len(orc)) if s.key_events(i)["deferred_at"] >= 0]
    assert len(deferred) == 1
    res = s.results()
    assert res.peak[deferred[0]] == orc["peak"][deferred[0]] > 1 and res.n_final[deferred[0]] >= 1
    s.close()


# ---------------------------------------------------------------- analysis
def test_analysis_right_after_the_append_that_reports_the_key(dev):
    """Every invalid key of the anomalous history: Stream.analysis taken in the
    call that reports it equals the ordinary checker's analysis of the key's
    whole sub-history -- :valid?, :op, :previous-ok, :last-op as they are,
    :configs and :final-paths as sets -- and oracle/linear_ref.py's, as
    test_gpu_parity.test_counterexamples compares them.  (A key with more than
    10 final configs: both renderings hold 10 of the restatement's, and the two
    may differ inside the mask group max_final cuts.)"""
    h, keys, orc, _rs = rows_case("A")
    ops = h.to_ops()
    lin = CK.linearizable({"model": model.cas_register(), "algorithm": "linear"})
    s = Stream(dev, exact=True)
    seen = []

    def after(n_rows, up):
        for i in up.invalid:
            k = keys[i]
            m = s.analysis(i, S.rows(h, 0, n_rows))
            sub = LR.subhistory(ops, k)
            want = lin.check({}, sub)
            a = LR.analysis(sub, model="cas-register")
            assert a.valid is False and a.fail_event == orc["fail_event"][i]
            assert m["valid?"] is False and want["valid?"] is False
            for f in ("op", "previous-ok", "last-op"):
                assert m[f] == want[f], f"key {k}: {f}: {m[f]}, the checker's {want[f]}"
            exp_cfgs = {(st, frozenset(sub[a.ops[q].invoke_pos]["index"] for q in L)) for st, L in a.final_configs}
            got_cfgs, want_cfgs = ([config_tuple(c, "cas-register") for c in x["configs"]] for x in (m, want))
            assert len(set(got_cfgs)) == len(got_cfgs) == len(want_cfgs) == min(10, len(exp_cfgs)), f"key {k}"
            assert set(got_cfgs) <= exp_cfgs
            exp_paths = LR.final_paths(a, sub, "cas-register")
            got_paths, want_paths = ({path_tuple(p, "cas-register") for p in x["final-paths"]} for x in (m, want))
            assert len(got_paths) == len(m["final-paths"]) > 0
            if len(exp_cfgs) <= 10:
                assert set(got_cfgs) == set(want_cfgs) == exp_cfgs, f"key {k}: configs"
                assert m["configs"][0]["last-op"] == want["configs"][0]["last-op"]
                assert got_paths == want_paths, f"key {k}: final-paths"
            if exp_paths is not None:
                assert got_paths <= exp_paths
                if len(exp_cfgs) <= 10 and len(exp_paths) <= 10:
                    assert got_paths == exp_paths
            seen.append(i)

    S.feed(s, h, 64, after)
    assert sorted(seen) == np.flatnonzero(orc["valid"] == 0).tolist() and len(seen) == 8
    s.close()


def test_events_mode_has_no_rows_to_report(dev):
    src = source("anomalies")
    s = Stream(dev, exact=True)
    b, ids = src.chunk([(k, 0, int(src.nev[k])) for k in range(src.pk.n_keys)])
    up = s.push(b, ids)
    assert up.invalid
    res = s.results()
    i = up.invalid[0]
    buf = np.zeros(64, np.int64)
    rc = N.lib().lc_stream_report(s.handle, i, 0, int(res.fail_event[i]), N.ptr(np.ascontiguousarray(res.final[i]), C.c_uint64),
                                  int(res.n_final[i]), 10, N.ptr(buf, C.c_int64), 64)
    assert rc == -5 and b"events mode" in N.lib().lc_last_error()  # LC_E_UNSUPPORTED
    s.close()


# ---------------------------------------------------------------- beside each other
def test_exact_and_plain_streams_and_a_batch_check_share_a_context(dev):
    h, keys, orc, _rs = rows_case("A")
    hi, keysi, orci, _ = rows_case("I")
    pk, pki = Packed(h), Packed(hi)
    one, onei = one_shot(dev, "rows A", pk), one_shot(dev, "rows I", pki)
    a, b = Stream(dev, exact=True), Stream(dev)
    for lo in range(0, max(len(h), len(hi)), 2000):
        if lo < len(h):
            a.append(S.rows(h, lo, min(len(h), lo + 2000)))
        r = dev.check(pki)
        for f in FIELDS:
            assert np.array_equal(getattr(r, f), orci[f]), f
        assert np.array_equal(r.n_final, onei.n_final)
        assert all(r.final[k, :r.n_final[k]].tolist() == onei.final[k, :r.n_final[k]].tolist() for k in range(len(keysi)))
        if lo < len(hi):
            b.append(S.rows(hi, lo, min(len(hi), lo + 2000)))
    a.finish(), b.finish()
    res = a.results()
    for f in FIELDS:
        assert np.array_equal(getattr(res, f), orc[f]), f
    assert np.array_equal(res.n_final, one.n_final)
    # the plain stream: its own verdicts, and nothing else of the result touched
    resb = b.results()
    assert resb.peak is None and resb.final is None and resb.n_final is None
    for f in ("valid", "cause", "fail_event"):
        assert np.array_equal(getattr(resb, f), orci[f]), f
    n = len(keysi)
    valid, fev, cause = np.zeros(n, np.int8), np.zeros(n, np.int32), np.zeros(n, np.uint8)
    peak, n_final = np.full(n, 0xABCD, np.uint32), np.full(n, 0xABCD, np.uint32)
    final = np.full((n, dev.max_final, 2), 0xABCD, np.uint64)
    r = N.LcResult()
    r.valid, r.fail_event, r.cause = N.ptr(valid, C.c_int8), N.ptr(fev, C.c_int32), N.ptr(cause, C.c_uint8)
    r.peak_configs, r.n_final, r.final_configs = N.ptr(peak, C.c_uint32), N.ptr(n_final, C.c_uint32), N.ptr(final, C.c_uint64)
    N.check(N.lib().lc_stream_results(b.handle, C.byref(r)))
    assert np.array_equal(valid, orci["valid"])
    assert (peak == 0xABCD).all() and (n_final == 0xABCD).all() and (final == 0xABCD).all()
    a.close(), b.close()
