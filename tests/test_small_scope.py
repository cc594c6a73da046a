"""The oracle on every small history (tests/small_scope.py): the C restatement
(oracle/linear_ref.c through cref) and the Python one (oracle/linear_ref.py)
against the definitional checker (oracle/brute.py) on every key of every
scope -- verdict and failing event -- and lc_pack on the two row orders the
GPU module feeds the device.  No key is sampled out.  The valid / invalid
counts are the oracle's own output recorded in small_scope.SCOPES, so a scope
cannot silently degenerate."""
import numpy as np
import pytest

import brute
import cref
import linear_ref as LR
import small_scope as SS
from lincheck import _native as N
from lincheck.checker import Packed


@pytest.fixture(scope="module", params=SS.ORDER)
def built(request):
    return SS.scope(request.param)


def test_counts_and_columns(built):
    """The rule's key and row counts, distinct keys (asserted by
    small_scope.Built), and columns that say what the event tuples say."""
    sc, h = built.scope, built.hist
    assert (built.n_keys, len(h)) == (sc.keys, sc.rows)
    assert sc.valid + sc.invalid == sc.keys
    for k in (0, built.n_keys // 2, built.n_keys - 1):
        lo, hi = int(built.off[k]), int(built.off[k + 1])
        got = [h.sub_op(r) for r in range(lo, hi)]
        want = SS.key_ops(built.events[k])
        for g, w, r in zip(got, want, range(lo, hi)):
            assert g["process"] == SS.PROCS_PER_KEY * k + w["process"] and h.key[r] == k
            assert (g["type"], g["f"], g["value"], g["index"]) == (w["type"], w["f"], w["value"], r)
    assert np.array_equal(h.process // SS.PROCS_PER_KEY, h.key)  # no process is shared between keys


def test_c_restatement_equals_the_definition(built):
    sc = built.scope
    keys, orc = cref.check_history(built.hist.as_c(), model=sc.model, threads=8)
    assert keys.tolist() == list(range(built.n_keys))
    assert ((orc["valid"] == 1).sum(), (orc["valid"] == 0).sum()) == (sc.valid, sc.invalid)
    assert orc["peak"].max() == sc.peak
    valid, fev = orc["valid"].tolist(), orc["fail_event"].tolist()
    bad = []
    for k in range(built.n_keys):
        ok, fe = brute.brute_check(built.ops(k), model=sc.model)
        if (valid[k], fev[k]) != (int(ok), -1 if fe is None else fe):
            bad.append(k)
    assert not bad, (f"{len(bad)} keys: cref {(valid[bad[0]], fev[bad[0]])}, brute "
                     f"{brute.brute_check(built.ops(bad[0]), model=sc.model)} on {built.describe(bad[0])}")
    assert (orc["cause"] == np.where(orc["valid"] == 0, 1, 0)).all()


@pytest.mark.parametrize("name", ["cas2", "cas3"])
def test_python_restatement_equals_the_definition(name):
    b = SS.scope(name)
    n_valid = 0
    for k in range(b.n_keys):
        ops = b.ops(k)
        a = LR.analysis(ops, model=b.scope.model)
        ok, fe = brute.brute_check(ops, model=b.scope.model)
        assert a.valid is ok and a.fail_event == fe, b.describe(k)
        n_valid += ok
    assert (n_valid, b.n_keys - n_valid) == (b.scope.valid, b.scope.invalid)


def pack_same(a, b):
    """Two Packed of the same keys: the same event words, descriptors, widths and key_error."""
    assert a.keys == b.keys
    assert np.array_equal(a.ev_off, b.ev_off)
    wa, wb = a.all_events(), b.all_events()
    assert np.array_equal(wa, wb)
    assert bool(a.view.trans_off) == bool(b.view.trans_off)
    n = int(a.view.n_trans)
    assert n == int(b.view.n_trans)
    ta, tb = N.carray(a.view.trans, n, np.uint32), N.carray(b.view.trans, n, np.uint32)
    if a.view.trans_off:
        oa, ob = (N.carray(p.view.trans_off, p.n_keys, np.uint32) for p in (a, b))
        key = np.repeat(np.arange(a.n_keys), np.diff(a.ev_off).astype(np.int64))
        inv = (wa >> 31) == 0
        assert np.array_equal(ta[oa[key[inv]] + (wa[inv] & 0xFFFFFF)], tb[ob[key[inv]] + (wb[inv] & 0xFFFFFF)])
    else:
        assert np.array_equal(ta, tb)
    assert np.array_equal(np.ctypeslib.as_array(a.view.key_width, shape=(a.n_keys,)),
                          np.ctypeslib.as_array(b.view.key_width, shape=(b.n_keys,)))
    assert [a.key_error(i) for i in range(a.n_keys)] == [b.key_error(i) for i in range(b.n_keys)]


def test_row_orders_pack_alike(built):
    """Key-major and one-row-of-each-key-in-turn: the same keys, event words,
    descriptors and key_error, key by key."""
    mdl = built.scope.model_obj()
    a, b = Packed(built.hist, mdl), Packed(built.round_robin(), mdl)
    assert a.keys == list(range(built.n_keys))
    pack_same(a, b)
    # every event of every key is an event of the reduced sub-history
    ops, events = LR.complete(built.ops(built.n_keys - 1), built.scope.model)
    assert a.n_events(built.n_keys - 1) == len(events)


# ---------------------------------------------------------------- widened scopes
# small_scope.widened: inert ops take every key out of the register tier (11)
# and past the narrow config's window (62) without changing a record.  Here the
# construction is held to the definition; tests/test_gpu_small_scope.py runs it.
WIDE_SCOPES = ("cas2", "cas3", "cas4p2", "reg4")
WIDTHS = (11, 62)
_base = {}


def base_records(name):
    """The unwidened scope's records (test_c_restatement_equals_the_definition
    holds them to brute.py)."""
    if name not in _base:
        b = SS.scope(name)
        _base[name] = cref.check_history(b.hist.as_c(), model=b.scope.model, threads=8)[1]
    return _base[name]


@pytest.mark.parametrize("place", SS.PLACES)
@pytest.mark.parametrize("n_inert", WIDTHS)
@pytest.mark.parametrize("name", WIDE_SCOPES)
def test_widened_records_and_words(name, n_inert, place):
    """The C restatement on the widened scope: valid, peak and probes are the
    unwidened key's, the failing event moves by the inert invokes before it;
    and lc_pack: every key past the register tier (11) / past the narrow
    window (62), none refused, both row orders the same words."""
    b = SS.scope(name)
    sc, base = b.scope, base_records(name)
    w = SS.widened(b, n_inert, place)
    # the columns: the scope's rows in order around one block of 2 * n_inert inert rows, processes disjoint
    h = w.hist
    assert len(h) == sc.rows + 2 * n_inert * sc.keys and np.array_equal(h.index, np.arange(len(h)))
    assert np.array_equal(np.repeat(np.arange(sc.keys), np.diff(w.off)), h.key)
    inert = h.process >= SS.INERT_PROC_BASE
    assert inert.sum() == 2 * n_inert * sc.keys and b.hist.process.max() < SS.INERT_PROC_BASE
    for a in ("type", "f", "process", "v0", "v1"):
        assert np.array_equal(getattr(h, a)[~inert], getattr(b.hist, a))
    assert (np.unique(h.process[inert], return_counts=True)[1] == 2).all()  # one op per inert process
    assert (h.v0[inert] == SS.INERT).all() and not (b.hist.v0 == SS.INERT).any() and not (b.hist.v1 == SS.INERT).any()
    first = np.flatnonzero(inert)[::2 * n_inert]
    assert np.array_equal(first, w.off[:-1] + w.at) and inert[first[-1]:first[-1] + 2 * n_inert].all()
    keys, orc = cref.check_history(h.as_c(), model=sc.model, threads=8)
    assert keys.tolist() == list(range(sc.keys))
    for f in ("valid", "cause", "peak", "probes"):
        bad = np.flatnonzero(orc[f] != base[f])
        assert not len(bad), f"{f}: {orc[f][bad[0]]}, unwidened {base[f][bad[0]]} on {w.describe(int(bad[0]))}"
    want = w.expected_fail_event(base["fail_event"])
    bad = np.flatnonzero(orc["fail_event"] != want)
    assert not len(bad), f"fail_event {orc['fail_event'][bad[0]]}, expected {want[bad[0]]} on {w.describe(int(bad[0]))}"
    moved = want != base["fail_event"]
    assert (want[moved] == base["fail_event"][moved] + n_inert).all()
    assert moved[base["valid"] == 0].all() if place == "head" else (moved.any() and not moved[base["valid"] == 0].all())
    mdl = sc.model_obj()
    pk = Packed(h, mdl)
    width = np.ctypeslib.as_array(pk.view.key_width, shape=(pk.n_keys,))
    assert n_inert <= width.min() and width.max() <= n_inert + sc.n_ops
    assert width.min() > (10 if n_inert == 11 else 56) and width.max() <= 112
    assert all(pk.key_error(i) is None for i in range(pk.n_keys))
    pack_same(pk, Packed(w.round_robin(), mdl))
    if place == "head":
        # the inert invokes come first and hold slots 0 .. n_inert - 1: every live event is the
        # unwidened key's with its slot + n_inert (event word: :ok bit 31, slot bits 24 .. 30)
        pk0 = Packed(b.hist, mdl)
        words, words0 = pk.all_events(), pk0.all_events()
        ev_off = pk.ev_off.astype(np.int64)
        assert np.array_equal(ev_off, pk0.ev_off.astype(np.int64) + n_inert * np.arange(pk.n_keys + 1))
        first = np.zeros(len(words), bool)
        first[(ev_off[:-1, None] + np.arange(n_inert)[None, :]).ravel()] = True
        assert np.array_equal(words[first] >> 24, np.tile(np.arange(n_inert, dtype=np.uint32), pk.n_keys))
        assert np.array_equal(words[~first] >> 24, (words0 >> 24) + np.uint32(n_inert))


@pytest.mark.parametrize("name,n_inert,place", [("cas2", n, p) for n in WIDTHS for p in SS.PLACES] + [("cas3", 11, "mid")])
def test_widened_wgl_records(name, n_inert, place):
    b = SS.scope(name)
    w = SS.widened(b, n_inert, place)
    for budget in (1 << 20, 3):
        _, base, _, _ = cref.check_history_wgl(b.hist.as_c(), budget=budget, threads=8, model=b.scope.model)
        keys, orc, _, _ = cref.check_history_wgl(w.hist.as_c(), budget=budget, threads=8, model=b.scope.model)
        assert keys.tolist() == list(range(b.n_keys))
        for f in ("valid", "peak"):
            bad = np.flatnonzero(orc[f] != base[f])
            assert not len(bad), f"budget {budget}, {f}: {orc[f][bad[0]]}, unwidened {base[f][bad[0]]} on {w.describe(int(bad[0]))}"


@pytest.mark.parametrize("place", ["head", "tail"])
def test_widened_by_the_definition(place):
    """brute.py itself on cas2 + 11: an op that can never be scheduled changes
    no verdict and moves the failing event by the invokes before it."""
    b = SS.scope("cas2")
    w = SS.widened(b, 11, place)
    base = base_records("cas2")
    want = w.expected_fail_event(base["fail_event"])
    for k in range(b.n_keys):
        ok, fe = brute.brute_check(w.ops(k), model=b.scope.model)
        assert (int(ok), -1 if fe is None else fe) == (base["valid"][k], want[k]), w.describe(k)


@pytest.mark.parametrize("place", SS.PLACES)
def test_widened_keys_leave_the_register_tier_in_their_inert_block(place):
    """stream_helpers.Restated on the round-robin order of cas2 + 11: every
    key is deferred, at the reduced event of the invoke that takes window
    slot 10."""
    import stream_helpers as S
    b = SS.scope("cas2")
    w = SS.widened(b, 11, place)
    rr = w.round_robin()
    rs = S.Restated(rr, 0)
    assert rs.keys == list(range(b.n_keys)) and not rs.error
    proc = rr.process.tolist()
    for k in range(b.n_keys):
        d = rs.defer_at[k]
        assert d >= 0, w.describe(k)
        is_ok, slot, _op, row = rs.events[k][d]
        assert not is_ok and slot == S.MAX_WIDTH and proc[row] >= SS.INERT_PROC_BASE, w.describe(k)
        assert all(s < S.MAX_WIDTH for ok_, s, _o, _r in rs.events[k][:d] if not ok_)
