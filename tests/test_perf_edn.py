"""lc_edn_read_perf / lc_edn_parse_perf: :type :f :process :time kept, :f
names interned in order of first appearance, every :value skipped.  No GPU."""
import os

import pytest

import perf_helpers as PH
from lincheck import _native as N
from lincheck import perf as P

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "perf_demo_history.edn")


def test_columns_and_names_in_order_of_first_appearance():
    ops = PH.hand_ops()
    h = P.PerfHistory.parse_edn(PH.edn_of(ops))
    assert h.names == ["read", "write", "start", "stop", "cas"]
    assert h.to_ops() == ops
    assert h.time.tolist() == [o["time"] for o in ops]
    assert (h.process == N.LC_NO_PROCESS).tolist() == [o["process"] == "nemesis" for o in ops]
    c = h.as_c()
    assert (c.n_f, c.f_start, c.f_stop) == (5, 2, 3)


def test_same_as_from_ops():
    ops = PH.hand_ops()
    a, b = P.PerfHistory.parse_edn(PH.edn_of(ops)), P.PerfHistory.from_ops(ops)
    assert a.names == b.names
    for col in ("type", "f", "process", "time"):
        assert getattr(a, col).tolist() == getattr(b, col).tolist()


def test_vector_file_and_line_file(tmp_path):
    ops = PH.hand_ops()
    lines = PH.edn_of(ops)
    vec = "[" + lines.replace("\n", " ") + "]"
    for name, text in (("lines.edn", lines), ("vector.edn", vec)):
        p = tmp_path / name
        p.write_text(text)
        assert P.PerfHistory.read_edn(str(p)).to_ops() == ops


def test_set_workload_file_values_skipped():
    text = """{:type :invoke, :f :add, :value 0, :time 100, :process 0}
{:type :ok, :f :add, :value 0, :time 150, :process 0}
{:type :info, :f :start, :value {:isolated {"n1" #{"n2"}}}, :time 160, :process :nemesis}
{:type :invoke, :f :read, :value nil, :time 200, :process 1}
{:type :ok, :f :read, :value #{0 1 2 #_ 9 3}, :time 260, :process 1, :error "x } y"}
"""
    h = P.PerfHistory.parse_edn(text)
    assert h.names == ["add", "start", "read"]
    want = PH.restate(h.to_ops())
    assert want["points"] == [("add", "ok", 100, 50), ("read", "ok", 200, 60)]
    packed = P.PackedPerf(h)
    assert (packed.matched, packed.orphans, packed.intervals.tolist()) == (2, 0, [[160, 260]])


def test_golden_fixture_is_the_generators():
    h = P.PerfHistory.read_edn(GOLDEN)
    assert 500 <= h.n <= 800 and set(h.names) == {"read", "write", "cas", "start", "stop"}
    t = h.time.tolist()
    assert t != sorted(t)  # log order is not time order
    want = PH.restate(h.to_ops())
    assert {ty for _, ty, _ in want["rate"]} == {"ok", "fail", "info"} and len(want["nemesis"]) == 3


def test_f_that_is_no_keyword_and_missing_f():
    h = P.PerfHistory.parse_edn('{:type :ok :f "odd" :process 1 :time 3}{:type :ok :process 1 :time 4}')
    assert h.names == ['"odd"', "nil"]


@pytest.mark.parametrize("text,what", [
    ("{:type :ok, :f :read, :process 0}", "without :time"),
    ("{:type :ok, :f :read, :process 0, :time 1.5}", ":time is not an integer"),
    ("{:f :read, :process 0, :time 1}", "without :type"),
    ("{:type :okay, :f :read, :process 0, :time 1}", "unknown :type"),
    ("{:type :ok, :f :read, :process 0, :time 1", "unterminated"),
    ("[{:type :ok, :f :read, :process 0, :time 1}", "unterminated history vector"),
    ("{:type :ok, :f :read, :time 1}\n{:type :ok, :time 99999999999999999999}", "out of range"),
    ("7", "expected an op map"),
])
def test_parse_errors(text, what):
    with pytest.raises(N.LincheckError, match="parse") as e:
        P.PerfHistory.parse_edn(text)
    assert what in str(e.value)


def test_error_names_the_line():
    text = PH.edn_of(PH.hand_ops()[:3]) + "{:type :ok, :f :read, :process 0}\n"
    with pytest.raises(N.LincheckError, match="line 4"):
        P.PerfHistory.parse_edn(text)


def test_missing_file():
    with pytest.raises(N.LincheckError, match="io"):
        P.PerfHistory.read_edn("/nonexistent/history.edn")
