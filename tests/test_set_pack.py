"""lc_set_pack (csrc/host_set.cpp) against jepsen.checker/set restated with
Python sets (tests/set_helpers.py), on the CPU: the packed view alone -- key
order, per-key status, and ids that give back every element -- decides each
key's result map, which is recomputed here from the view and compared."""
import random

import numpy as np
import pytest

import set_helpers as SH
from lincheck import _native as N
from lincheck.setcheck import PackedSet, SetHistory


def elements(a, k, ids):
    """The elements ids of key k stand for: min + id, or vals[id]."""
    if a["rank"][k]:
        vals = a["vals"][int(a["vals_off"][k]):int(a["vals_off"][k + 1])]
        assert len(vals) == a["span"][k] and all(int(x) < int(y) for x, y in zip(vals, vals[1:]))
        return [int(vals[i]) for i in ids]
    return [int(a["min"][k]) + int(i) for i in ids]


def from_view(packed, a, k):
    """The result map the packed arrays of key k imply."""
    if a["status"][k] != N.LC_SET_KEY_OK:
        return {"valid?": "unknown", "error": packed.key_error(k)}
    ab, ae = int(a["add_off"][k]), int(a["add_off"][k + 1])
    rb, re_ = int(a["read_off"][k]), int(a["read_off"][k + 1])
    ids, cls = a["add_id"][ab:ae], a["add_cls"][ab:ae]
    assert all(int(i) < int(a["span"][k]) for i in ids) and all(int(i) < int(a["span"][k]) for i in a["read_id"][rb:re_])
    el = elements(a, k, ids)
    ops = [{"type": "invoke" if c == N.LC_SET_ATTEMPT else "ok", "f": "add", "value": e} for e, c in zip(el, cls)]
    ops.append({"type": "ok", "f": "read", "value": elements(a, k, a["read_id"][rb:re_])})
    return SH.restate(ops)


def check_history(ops):
    want = SH.restate_independent(ops)
    packed = PackedSet(SetHistory.from_ops(ops))
    a = packed.arrays()
    assert packed.keys == list(want), "keys in order of first appearance"
    base_end = 0
    for k, key in enumerate(packed.keys):
        got = from_view(packed, a, k)
        assert SH.same(got, want[key]), (key, got, want[key])
        if a["status"][k] == N.LC_SET_KEY_OK:
            # every key on a fresh, even 64-bit word, disjoint from the one before
            assert int(a["base"][k]) % 2 == 0 and int(a["base"][k]) >= base_end
            base_end = int(a["base"][k]) + -(-int(a["span"][k]) // 64)
    assert base_end <= a["n_words"] and a["n_words"] % 2 == 0
    return packed, a


def test_hand_example():
    packed, a = check_history(SH.hand_ops())
    assert SH.restate(SH.hand_ops()) == SH.HAND_WANT
    assert packed.keys == [None] and a["span"][0] == 31 and a["min"][0] == 0 and a["rank"][0] == 0
    assert list(a["add_cls"]).count(N.LC_SET_ATTEMPT) == 11 and list(a["add_cls"]).count(N.LC_SET_ACK) == 9
    assert N.lib().lc_set_batch_max_runs(packed.view) == 9 + 2 * 9


@pytest.mark.parametrize("block", range(10))
def test_random_histories(block):
    rng = random.Random(1000 + block)
    for _ in range(20):
        check_history(SH.random_history(rng))


def test_nil_read_after_a_real_one_is_never_read():
    ops = [{"type": "invoke", "f": "add", "value": 1}, {"type": "ok", "f": "add", "value": 1},
           {"type": "ok", "f": "read", "value": {1}}, {"type": "ok", "f": "read", "value": None}]
    packed, a = check_history(ops)
    assert a["status"][0] == N.LC_SET_KEY_NEVER_READ and packed.key_error(0) == "Set was never read"


def test_extreme_elements_and_wide_keys():
    big = SH.I64_MAX
    ops = [{"type": t, "f": "add", "value": e} for e in (-1, big, -big, 0) for t in ("invoke", "ok")]
    ops.append({"type": "ok", "f": "read", "value": [big, -big, -1, -1]})
    packed, a = check_history(ops)
    assert a["rank"][0] == 1 and a["span"][0] == 4 and list(a["vals"]) == [-big, -1, 0, big]
    # {-5, 10^12}: two ids, not 10^12 bits
    ops = [{"type": "invoke", "f": "add", "value": -5}, {"type": "invoke", "f": "add", "value": 10 ** 12},
           {"type": "ok", "f": "read", "value": set()}]
    packed, a = check_history(ops)
    assert a["rank"][0] == 1 and a["span"][0] == 2 and a["n_words"] == 2


def test_nil_element_is_an_error_key_beside_good_ones():
    from lincheck.independent import Tuple
    ops = [{"type": "invoke", "f": "add", "value": Tuple(1, None)}, {"type": "ok", "f": "read", "value": Tuple(1, {3})},
           {"type": "invoke", "f": "add", "value": Tuple(2, 3)}, {"type": "ok", "f": "read", "value": Tuple(2, {3})},
           {"type": "ok", "f": "read", "value": Tuple(3, ["x"])}]
    packed, a = check_history(ops)
    assert list(a["status"]) == [N.LC_SET_KEY_ERROR, N.LC_SET_KEY_OK, N.LC_SET_KEY_ERROR]
    assert int(a["add_off"][-1]) == 1 and int(a["read_off"][-1]) == 1, "rows of keys that are not checked are not uploaded"


def test_large_history_takes_the_threaded_passes():
    """Above 2^17 rows the row passes are split over threads: same arrays."""
    from lincheck.setcheck import synth_set
    h = synth_set(n_keys=3, adds_per_key=60000, concurrency=10, info_rate=0.05, lost_rate=0.01, seed=5)
    a = PackedSet(h).arrays()
    for k in range(3):
        rows = h.key == k
        inv = rows & (h.f == N.LC_SF_ADD) & ((h.type == N.LC_INVOKE) | (h.type == N.LC_OK_T))
        ab, ae = int(a["add_off"][k]), int(a["add_off"][k + 1])
        assert np.array_equal(a["add_id"][ab:ae].astype(np.int64) + a["min"][k], h.elem[inv])
        assert np.array_equal(a["add_cls"][ab:ae] == N.LC_SET_ATTEMPT, h.type[inv] == N.LC_INVOKE)


def test_bad_codes_rejected():
    h = SetHistory.from_ops(SH.hand_ops())
    h.f[3] = 9
    with pytest.raises(N.LincheckError, match="row 3"):
        PackedSet(h)
