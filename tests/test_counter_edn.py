"""lc_edn_read_counter / lc_edn_parse_counter: a history written as EDN by
tests/counter_helpers.py reads back as the same columns, for tuple values and
plain ones, and the result maps of the text equal those of the ops."""
import numpy as np
import pytest

import counter_helpers as H
from lincheck import _native as N
from lincheck import checker as ck
from lincheck import counter as CT
from lincheck import independent


def same_columns(a, b):
    for name in ("type", "f", "process", "value"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    ka = np.full(a.n, N.LC_NO_KEY, np.int64) if a.key is None else a.key
    kb = np.full(b.n, N.LC_NO_KEY, np.int64) if b.key is None else b.key
    assert np.array_equal(ka, kb)


@pytest.mark.parametrize("n_keys", [0, 4])
def test_write_then_read_gives_the_same_columns(tmp_path, n_keys):
    ops = H.random_history(H.rng_of(5 + n_keys), 600, n_keys=n_keys, p_bad=0.02)
    want = CT.CounterHistory.from_ops(ops)
    text = H.write_edn(ops)
    got = CT.CounterHistory.parse_edn(text)
    same_columns(got, want)
    assert got.index.tolist() == list(range(len(ops)))
    path = tmp_path / "history.edn"
    path.write_text(text)
    same_columns(CT.CounterHistory.read_edn(str(path)), want)
    # a vector of op maps reads the same
    same_columns(CT.CounterHistory.parse_edn("[" + text + "]"), want)
    # and checks the same
    r = independent.checker(ck.counter({"host": True})).check({}, got, {}) if n_keys else ck.counter({"host": True}).check({}, got, {})
    maps = H.restate_independent(ops)
    if n_keys:
        assert all(H.same(r["results"][k], maps[k]) for k in maps)
    else:
        assert H.same(r, maps[None])


def test_values_that_are_no_integers_read_as_nil():
    text = """{:type :invoke, :f :add, :value "x", :process 0}
{:type :ok, :f :add, :value 1.5, :process 0}
{:type :invoke, :f :read, :value nil, :process 1, :time 5}
{:type :ok, :f :read, :value [7 12], :process 1}
{:type :ok, :f :read, :value [7 nil], :process :nemesis}
{:type :info, :f :start, :value [1 2], :process :nemesis}
{:type :invoke, :f :add, :value [1 2 3], :process 2}
{:type :invoke, :f :add, :value -4, :process 3, :index 99}
"""
    h = CT.CounterHistory.parse_edn(text)
    nil, nok, nop = N.LC_NIL, N.LC_NO_KEY, N.LC_NO_PROCESS
    assert h.value.tolist() == [nil, nil, nil, 12, nil, nil, nil, -4]
    assert h.key.tolist() == [nok, nok, nok, 7, 7, nok, nok, nok]
    assert h.process.tolist() == [0, 0, 1, 1, nop, nop, 2, 3]
    assert h.f.tolist() == [0, 0, 1, 1, 1, 2, 0, 0] and h.type.tolist() == [0, 1, 0, 1, 1, 3, 0, 0]
    assert h.index.tolist() == [-1] * 7 + [99]


def test_errors_are_reported():
    with pytest.raises(N.LincheckError, match="parse"):
        CT.CounterHistory.parse_edn("{:type :invoke, :f :add, :value 1")
    with pytest.raises(N.LincheckError, match="parse"):
        CT.CounterHistory.parse_edn("{:f :add, :value 1}")
    with pytest.raises(N.LincheckError, match="io"):
        CT.CounterHistory.read_edn("/nonexistent/history.edn")
