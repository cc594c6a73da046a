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


def test_row_orders_pack_alike(built):
    """Key-major and one-row-of-each-key-in-turn: the same keys, event words,
    descriptors and key_error, key by key."""
    mdl = built.scope.model_obj()
    a, b = Packed(built.hist, mdl), Packed(built.round_robin(), mdl)
    assert a.keys == b.keys == list(range(built.n_keys))
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
    # every event of every key is an event of the reduced sub-history
    ops, events = LR.complete(built.ops(built.n_keys - 1), built.scope.model)
    assert a.n_events(built.n_keys - 1) == len(events)
