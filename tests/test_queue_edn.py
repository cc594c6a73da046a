"""lc_edn_read_queue / lc_edn_parse_queue: a history written as EDN by
tests/queue_helpers.py reads back as the same columns, for tuple values and
plain ones, drains' vectors inside tuples included; values of any other shape
are refused; every other :f is skipped with its value."""
import numpy as np
import pytest

import queue_helpers as H
from lincheck import _native as N
from lincheck import checker as ck
from lincheck import independent
from lincheck import queue as Q


def same_columns(a, b):
    for name in ("type", "f", "value", "drain_off", "drain_val"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    ka = np.full(a.n, N.LC_NO_KEY, np.int64) if a.key is None else a.key
    kb = np.full(b.n, N.LC_NO_KEY, np.int64) if b.key is None else b.key
    assert np.array_equal(ka, kb)


@pytest.mark.parametrize("n_keys", [0, 4])
def test_write_then_read_gives_the_same_columns(tmp_path, n_keys):
    ops = H.random_history(H.rng_of(5 + n_keys), 600, n_keys=n_keys, domain=5, p_crash=0.01)
    for o in ops:
        # as text, a drain's [int nil] is the tuple [k nil] (include/lincheck_queue.h): keep such a pair of
        # drained elements out of the text
        if o["f"] == "drain" and isinstance(o["value"], list) and len(o["value"]) == 2 and o["value"][1] is None:
            o["value"].reverse()
    want = Q.QueueHistory.from_ops(ops)
    assert int(want.drain_off[-1]) > 20
    text = H.write_edn(ops)
    got = Q.QueueHistory.parse_edn(text)
    same_columns(got, want)
    path = tmp_path / "history.edn"
    path.write_text(text)
    same_columns(Q.QueueHistory.read_edn(str(path)), want)
    # a vector of op maps reads the same
    same_columns(Q.QueueHistory.parse_edn("[" + text + "]"), want)
    # and checks the same
    for checker, restate in ((ck.total_queue, H.restate_queue), (ck.unique_ids, H.restate_ids)):
        maps = H.restate_independent(ops, restate)
        if n_keys:
            assert independent.checker(checker({"host": True})).check({}, got, {})["results"] == maps
        else:
            assert checker({"host": True}).check({}, got, {}) == maps[None]


def test_tuples_drains_and_skipped_rows():
    text = """{:type :invoke, :f :enqueue, :value 5, :process 0}
{:type :ok, :f :enqueue, :value [7 12], :process 0}
{:type :invoke, :f :dequeue, :value nil, :process 1, :time 5}
{:type :ok, :f :dequeue, :value [7 nil], :process 1}
{:type :info, :f :start, :value [1 2 "x" {:a 1}], :process :nemesis}
{:type :invoke, :f :drain, :value [7 nil], :process 2}
{:type :ok, :f :drain, :value [7 [3 nil -4]], :process 2}
{:type :ok, :f :drain, :value [1 2 3], :process 2}
{:type :ok, :f :drain, :value [8 9], :process 2}
{:type :ok, :f :drain, :value [], :process 2}
{:type :ok, :f :drain, :value [8 []], :process 2}
{:type :ok, :f :generate, :value -9223372036854775807, :process 3}
{:type :ok, :f :read, :value "anything", :process 3}
{:type :ok, :value 1.5}
"""
    h = Q.QueueHistory.parse_edn(text)
    nil, nok = N.LC_NIL, N.LC_NO_KEY
    E, D, R, G, O = N.LC_QF_ENQUEUE, N.LC_QF_DEQUEUE, N.LC_QF_DRAIN, N.LC_QF_GENERATE, N.LC_QF_OTHER
    assert h.f.tolist() == [E, E, D, D, O, R, R, R, R, R, R, G, O, O]
    assert h.type.tolist() == [0, 1, 0, 1, 3, 0, 1, 1, 1, 1, 1, 1, 1, 1]
    assert h.value.tolist() == [5, 12, nil, nil, nil, nil, nil, nil, nil, nil, nil, -(2**63 - 1), nil, nil]
    assert h.key.tolist() == [nok, 7, nok, 7, nok, 7, 7, nok, nok, nok, 8, nok, nok, nok]
    # [8 9] on a drain row is two drained elements: a tuple's second element there is nil or a vector
    assert h.drain_off.tolist() == [0, 0, 0, 0, 0, 0, 0, 3, 6, 8, 8, 8, 8, 8, 8]
    assert h.drain_val.tolist() == [3, nil, -4, 1, 2, 3, 8, 9]
    assert h.to_ops()[6]["value"] == independent.tuple(7, [3, None, -4])


@pytest.mark.parametrize("value", ['"x"', "1.5", ":kw", "[1 2 3]", '[7 "x"]', "[7 [1 2]]", "{:a 1}", "[nil 3]", "12345678901234567890N"])
def test_a_value_that_is_neither_an_integer_nor_nil_is_refused(value):
    with pytest.raises((ValueError, N.LincheckError)) as e:
        Q.QueueHistory.parse_edn("{:type :ok, :f :dequeue, :value 1}\n{:type :ok, :f :enqueue, :value %s, :process 0}" % value)
    if isinstance(e.value, N.LincheckError):  # out of range is a parse error, as everywhere in the reader
        assert "N" in value and e.value.code == -4
    else:
        assert "line 2" in str(e.value)
    assert N.lib().lc_edn_parse_queue(b"{:type :ok, :f :enqueue, :value 2.5}", 36, None) == -1


@pytest.mark.parametrize("value", ['"x"', "7", '[1 "x"]', "[7 [1 [2]]]", "[[1] [2]]", "[7 [1 2] 3]", "#{1 2}"])
def test_a_drain_that_is_no_vector_of_integers_is_refused(value):
    with pytest.raises(ValueError, match="drain"):
        Q.QueueHistory.parse_edn("{:type :ok, :f :drain, :value %s}" % value)


def test_from_ops_refuses_the_same():
    for bad in ("x", 1.5, True, [1, 2], 2**63):
        with pytest.raises(ValueError):
            Q.QueueHistory.from_ops([H.op("ok", "enqueue", bad)])
    for bad in (7, "x", [1, "x"], [[1]]):
        with pytest.raises(ValueError):
            Q.QueueHistory.from_ops([H.op("ok", "drain", bad)])
    # but not on rows that are skipped
    h = Q.QueueHistory.from_ops([{"type": "info", "f": "start", "value": "x", "process": "nemesis"}, H.op("ok", "read", "y")])
    assert h.f.tolist() == [N.LC_QF_OTHER] * 2


def test_errors_are_reported():
    with pytest.raises(N.LincheckError, match="parse"):
        Q.QueueHistory.parse_edn("{:type :invoke, :f :enqueue, :value 1")
    with pytest.raises(N.LincheckError, match="parse"):
        Q.QueueHistory.parse_edn("{:f :enqueue, :value 1}")
    with pytest.raises(N.LincheckError, match="parse"):
        Q.QueueHistory.parse_edn("{:type :ok, :f :drain, :value [1 2}")
    with pytest.raises(N.LincheckError, match="io"):
        Q.QueueHistory.read_edn("/nonexistent/history.edn")
