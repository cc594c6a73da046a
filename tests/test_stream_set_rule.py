"""The resident set tier's resume rule on the CPU: "closed start, then exact
JIT" (tests/stream_set_rule.py) against the oracle (oracle/linear_ref.c through
cref, the C build of linear_ref.analysis: valid and fail_event) on every key
of three histories whose keys leave the register tier -- a crashed op on a key
with 10 ops in flight -- and on rows_case "B" of tests/test_gpu_stream.py.

The rule closes S at the first invoke that takes window slot >= 10; since the
register tier's lattice may have been closed long before the key leaves, it is
also closed at a few earlier invokes.  Either way the verdict and the failing
event must be the oracle's ("emptiness")."""
import numpy as np
import pytest

import cref
import stream_helpers as S
import stream_set_rule as R
from lincheck import history as H

HISTORIES = {
    # name: (synth arguments, keys leaving the register tier, largest I, most ops pending, keys past the cap)
    "info2": (dict(n_keys=100, ops_per_key=100, concurrency=10, interleave=True, nemesis_period=5.0, info_rate=0.02,
                   anomaly_rate=0.1, seed=11), 3, 6480, 12, 0),
    "info5": (dict(n_keys=100, ops_per_key=100, concurrency=10, interleave=True, nemesis_period=5.0, info_rate=0.05,
                   anomaly_rate=0.1, seed=12), 31, 75712, 18, 1),
    "long": (dict(n_keys=60, ops_per_key=300, concurrency=10, info_rate=0.02, anomaly_rate=0.2, seed=13),
             32, 43520, 16, 1),
    "B": (dict(n_keys=12, ops_per_key=150, concurrency=10, interleave=True, nemesis_period=5.0, anomaly_rate=0.3,
               info_rate=0.02, seed=3), 1, None, None, 0),
}
LARGEST_S = {"info5": 41216, "long": 12288}  # largest closed S' after leaving

_case = {}


def case(name):
    if name not in _case:
        h = H.synth(**HISTORIES[name][0])
        keys, orc = cref.check_history(h.as_c(), budget=1 << 20, threads=8)
        rs = S.Restated(h)
        runs = [R.Run(rs.events[k]) for k in keys]
        _case[name] = (h, list(keys), orc, rs, runs)
    return _case[name]


def verdict(run):
    return int(run.valid), -1 if run.fail_event is None else run.fail_event


@pytest.mark.parametrize("name", list(HISTORIES))
def test_closed_start_gives_the_oracle_s_verdict_on_every_key(name):
    _h, keys, orc, rs, runs = case(name)
    assert (orc["cause"][orc["valid"] != 0] == 0).all(), "the oracle gives up on no key at budget 2^20"
    for i, k in enumerate(keys):
        assert verdict(runs[i]) == (int(orc["valid"][i]), int(orc["fail_event"][i])), f"{name}, key {k}"
        # the rule leaves where the stream defers (a key that failed earlier never gets there)
        if runs[i].left_at is not None:
            assert runs[i].left_at == rs.defer_at[k]
        else:
            assert rs.defer_at[k] < 0 or not runs[i].valid


@pytest.mark.parametrize("name", ["info2", "B", "long"])
def test_closing_at_earlier_events_changes_no_verdict(name):
    """The lattice is closed at every :ok of the lane phase, long before the
    key leaves: close at every 7th invoke, at the first 3, at every invoke."""
    _h, keys, orc, rs, runs = case(name)
    picked = [i for i in range(len(keys)) if name != "long" or runs[i].left_at is not None][:12 if name != "long" else 4]
    if name == "long":
        picked.append(next(i for i in range(len(keys)) if orc["valid"][i] == 0 and runs[i].left_at is not None))
    for i in picked:
        ev = rs.events[keys[i]]
        inv = [e for e, x in enumerate(ev) if not x[0]]
        for close_at in (set(inv[::7]), set(inv[:3]), set(inv)):
            assert verdict(R.Run(ev, close_at=close_at)) == (int(orc["valid"][i]), int(orc["fail_event"][i])), (name, i)


def test_a_key_is_invalid_only_after_leaving_the_tier():
    """From the oracle: in the long history at least one key's failing :ok
    lies past the invoke that takes window slot 10 -- the verdict a stream
    without the set tier reports at finish only."""
    _h, keys, orc, rs, _runs = case("long")
    late = [i for i, k in enumerate(keys) if orc["valid"][i] == 0 and 0 <= rs.defer_at[k] < orc["fail_event"][i]]
    assert late, "no key fails after leaving the register tier"


@pytest.mark.parametrize("name", ["info2", "info5", "long"])
def test_closed_sets_sizes_against_the_cap(name):
    """What the cap rule (stream_plan.hpp stream_set_falls_back) makes of the
    closed sets: a few leaving keys are past the larger LDS tier's capacities
    (S 4,096 / I 16,384), a cap of 32,768 covers all but one per history, and
    exact sets (no closing) are never larger."""
    _h, keys, _orc, rs, runs = case(name)
    _args, n_left, largest_i, most_pending, n_past_cap = HISTORIES[name]
    left = [r for r in runs if r.left_at is not None]
    assert len(left) == n_left
    assert max(r.max_i for r in left) == largest_i and max(r.max_pending for r in left) == most_pending
    if name in LARGEST_S:
        assert max(r.max_s for r in left) == LARGEST_S[name]
    assert sum(r.falls_back for r in left) == n_past_cap
    assert all(r.falls_back == (r.max_s > R.CAP or r.max_i > R.CAP) for r in left)
    if name != "info2":
        assert sum(r.max_s > 4096 or r.max_i > 16384 for r in left) == 4
    for i, r in enumerate(runs):
        if r.left_at is not None and i % 4 == 0:
            x = R.Run(rs.events[keys[i]], closed=False)
            assert x.max_s <= r.max_s and x.max_i <= r.max_i and verdict(x) == verdict(r)
