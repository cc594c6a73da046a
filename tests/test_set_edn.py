"""lc_edn_read_set / lc_edn_parse_set: a set-workload history.edn becomes the
columns SetHistory.from_ops makes of the same ops."""
import random

import numpy as np
import pytest

import set_helpers as SH
from lincheck import _native as N
from lincheck.independent import Tuple
from lincheck.setcheck import PackedSet, SetHistory

NEMESIS = [
    {"type": "info", "f": "start", "process": "nemesis", "value": None, "edn": "nil"},
    {"type": "info", "f": "start", "process": "nemesis", "value": None,
     "edn": '[:isolated {"n1" #{"n2" "n3"}, "n2" #{"n1"}, "n3" #{"n1"}}]'},
    {"type": "info", "f": "stop", "process": "nemesis", "value": None, "edn": ":network-healed"},
]


def same_columns(a: SetHistory, b: SetHistory):
    assert a.n == b.n
    for name in ("type", "f", "key", "elem", "read_off", "index"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert np.array_equal(a.read_elem[:int(a.read_off[-1])], b.read_elem[:int(b.read_off[-1])])


def with_nemesis(ops):
    out = list(ops)
    for i, row in enumerate(NEMESIS):
        out.insert(min(len(out), 3 + 4 * i), dict(row))
    for i, op in enumerate(out):
        op["index"] = i
    return out


def test_plain_history(tmp_path):
    ops = with_nemesis(SH.hand_ops())
    path = tmp_path / "history.edn"
    path.write_text(SH.edn_lines(ops))
    h = SetHistory.read_edn(str(path))
    same_columns(h, SetHistory.from_ops(ops))
    assert (h.key == N.LC_NO_KEY).all() and (h.f == N.LC_SF_OTHER).sum() == 3


def test_tuple_history_lists_and_vectors():
    ops = []
    for k in (3, 9):
        for e in (5, 6, -2):
            ops.append({"type": "invoke", "f": "add", "value": Tuple(k, e)})
            ops.append({"type": "ok", "f": "add", "value": Tuple(k, e)})
        ops.append({"type": "invoke", "f": "read", "value": Tuple(k, None)})
    ops.append({"type": "ok", "f": "read", "value": Tuple(3, [5, 5, 6])})
    ops.append({"type": "ok", "f": "read", "value": Tuple(9, {-2, 6})})
    ops.append({"type": "ok", "f": "read", "value": Tuple(9, []), "edn": "[9 ()]"})
    ops = with_nemesis(ops)
    text = SH.edn_lines(ops)
    h = SetHistory.parse_edn(text)
    same_columns(h, SetHistory.from_ops(ops))
    assert set(h.key.tolist()) == {3, 9, N.LC_NO_KEY}
    # the same ops as one vector of maps, commas and all
    same_columns(SetHistory.parse_edn("[" + text.replace("\n", " ") + "]"), h)
    assert PackedSet(h).keys == [3, 9]


def test_plain_vector_read_of_two_elements_is_no_tuple():
    ops = [{"type": "invoke", "f": "read", "value": None, "index": 0}, {"type": "ok", "f": "read", "value": [1, 2], "index": 1}]
    h = SetHistory.parse_edn(SH.edn_lines(ops))
    assert (h.key == N.LC_NO_KEY).all() and h.read_elem[:2].tolist() == [1, 2]


@pytest.mark.parametrize("seed", range(5))
def test_random_histories_round_trip(seed):
    ops = SH.random_history(random.Random(seed))
    same_columns(SetHistory.parse_edn(SH.edn_lines(ops)), SetHistory.from_ops(ops))


def test_non_integer_element_is_reported_not_crashed_on():
    ops = [{"type": "invoke", "f": "add", "value": 1}, {"type": "ok", "f": "add", "value": 1},
           {"type": "invoke", "f": "add", "value": None, "edn": ":x"}, {"type": "invoke", "f": "add", "value": None, "edn": "1.5"},
           {"type": "ok", "f": "read", "value": [1, None], "edn": '#{1 "two"}'}]
    for i, op in enumerate(ops):
        op["index"] = i
    h = SetHistory.parse_edn(SH.edn_lines(ops))
    same_columns(h, SetHistory.from_ops(ops))
    assert h.elem[2] == N.LC_NIL and h.elem[3] == N.LC_NIL and N.LC_NIL in h.read_elem.tolist()
    p = PackedSet(h)
    assert p.status[0] == N.LC_SET_KEY_ERROR and "not an integer" in p.key_error(0)


def test_syntax_error_names_the_line():
    with pytest.raises(N.LincheckError, match="line 2"):
        SetHistory.parse_edn("{:type :ok, :f :add, :value 1}\n{:type :ok, :f :add, :value #{1 2")

