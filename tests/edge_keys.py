"""Keys on the set tiers' capacity edges, pinned.

need(key) = max(max |I|, max |S'|) over the events the unbounded :linear
search walks (cref.key_sizes / cref.need) is the least budget that decides a
key; a key whose largest |S'| or |I| is exactly a tier's capacity fills that
tier's arrays to the last slot and its hash tables to their designed load, and
one whose largest set is a few entries more leaves the tier inside one 64-lane
batch, where only the `r < CAP` guards stand between it and the next array.
Random batches meet neither except by luck, so the keys are searched for once
(tests/tools/find_edge_keys.py, CPU only) and pinned here as (synth arguments,
key) literals.  No search runs at test time: batch() rebuilds each key from
its seed and asserts, from cref.key_sizes and the packed words, that it is
still the edge it is listed as.

The capacities restate the kernels' (jepsen-etcd-demo_amd/csrc); they place
cases and state preconditions only.  Expected results always come from the
oracle."""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache
from typing import Dict, List

import numpy as np

import cref
from edgegen import pending_before
from lincheck import history as H
from lincheck.checker import Packed

UNBOUNDED = 1 << 40
LEAVES_REGISTER_TIER = 11        # lattice_core.hpp LC_T0_MAX_WIDTH + 1 ops pending
T1_S, T1_I = 256, 512            # device_search.hip T1_S, T1_I
T2_S, T2_I = 1024, 4096          # device_search.hip T2_S, T2_I
HBM_LIM_S, HBM_LIM_I = 2048, 4096  # device_hbm.hip LIM_S, LIM_I (the LDS pass's limits; past them: PASS_REDO)
BATCH = 64                       # one wave's batch: "over" means by at most this much

RERUN = "rerun tests/tools/find_edge_keys.py and replace tests/edge_keys.py TABLE"

# (synth kwargs, key, class, most pending, peak = max |S'|, max |I|, valid)
TABLE: List[tuple] = [
    ({'n_keys': 3000, 'ops_per_key': 60, 'concurrency': 12, 'anomaly_rate': 0.15, 'seed': 20}, 762, 't1_fit', 11, 256, 512, 1),
    ({'n_keys': 3000, 'ops_per_key': 40, 'concurrency': 13, 'anomaly_rate': 0.15, 'seed': 21}, 2653, 't1_fit', 11, 160, 512, 1),
    ({'n_keys': 3000, 'ops_per_key': 60, 'concurrency': 13, 'anomaly_rate': 0.15, 'seed': 21}, 2653, 't1_fit', 11, 256, 512, 1),
    ({'n_keys': 3000, 'ops_per_key': 40, 'concurrency': 13, 'anomaly_rate': 0.15, 'seed': 20}, 686, 't1_over_S', 11, 290, 384, 1),
    ({'n_keys': 3000, 'ops_per_key': 40, 'concurrency': 13, 'anomaly_rate': 0.15, 'seed': 21}, 588, 't1_over_S', 11, 320, 384, 1),
    ({'n_keys': 3000, 'ops_per_key': 40, 'concurrency': 13, 'anomaly_rate': 0.15, 'seed': 21}, 889, 't1_over_S', 11, 264, 480, 1),
    ({'n_keys': 3000, 'ops_per_key': 60, 'concurrency': 12, 'anomaly_rate': 0.15, 'seed': 27}, 1888, 't1_over_I', 11, 112, 528, 0),
    ({'n_keys': 3000, 'ops_per_key': 40, 'concurrency': 12, 'anomaly_rate': 0.15, 'seed': 21}, 1895, 't1_over_I', 11, 160, 544, 1),
    ({'n_keys': 3000, 'ops_per_key': 40, 'concurrency': 12, 'anomaly_rate': 0.15, 'seed': 21}, 2272, 't1_over_I', 11, 252, 568, 1),
    ({'n_keys': 300, 'ops_per_key': 200, 'concurrency': 11, 'info_rate': 0.005, 'anomaly_rate': 0.15, 'seed': 4}, 293, 't2_fit', 11, 1024, 2144, 1),
    ({'n_keys': 300, 'ops_per_key': 200, 'concurrency': 15, 'info_rate': 0.0, 'anomaly_rate': 0.15, 'seed': 2}, 89, 't2_fit', 11, 1024, 2528, 0),
    ({'n_keys': 300, 'ops_per_key': 200, 'concurrency': 16, 'info_rate': 0.0, 'anomaly_rate': 0.15, 'seed': 3}, 164, 't2_fit', 12, 280, 4096, 1),
    ({'n_keys': 300, 'ops_per_key': 200, 'concurrency': 13, 'info_rate': 0.005, 'anomaly_rate': 0.15, 'seed': 1}, 83, 't2_over_S', 12, 1072, 2680, 0),
    ({'n_keys': 300, 'ops_per_key': 200, 'concurrency': 11, 'info_rate': 0.01, 'anomaly_rate': 0.15, 'seed': 1}, 43, 't2_over_S', 11, 1088, 2622, 1),
    ({'n_keys': 300, 'ops_per_key': 200, 'concurrency': 11, 'info_rate': 0.01, 'anomaly_rate': 0.15, 'seed': 3}, 171, 't2_over_S', 11, 1072, 2096, 1),
    ({'n_keys': 300, 'ops_per_key': 200, 'concurrency': 13, 'info_rate': 0.01, 'anomaly_rate': 0.15, 'seed': 1}, 43, 't2_over_I', 12, 896, 4160, 0),
    ({'n_keys': 300, 'ops_per_key': 200, 'concurrency': 16, 'info_rate': 0.005, 'anomaly_rate': 0.15, 'seed': 4}, 109, 't2_over_I', 12, 768, 4129, 1),
    ({'n_keys': 300, 'ops_per_key': 300, 'concurrency': 11, 'info_rate': 0.01, 'anomaly_rate': 0.15, 'seed': 4}, 260, 't2_over_I', 11, 1024, 4120, 1),
    ({'n_keys': 400, 'ops_per_key': 300, 'concurrency': 16, 'info_rate': 0.01, 'anomaly_rate': 0.15, 'seed': 2}, 219, 'hbm_narrow', 12, 2048, 2176, 1),
    ({'n_keys': 400, 'ops_per_key': 300, 'concurrency': 16, 'info_rate': 0.01, 'anomaly_rate': 0.15, 'seed': 2}, 228, 'hbm_narrow', 12, 2066, 3530, 1),
    ({'n_keys': 400, 'ops_per_key': 300, 'concurrency': 16, 'info_rate': 0.01, 'anomaly_rate': 0.15, 'seed': 1}, 78, 'hbm_narrow', 12, 2304, 4096, 1),
    ({'n_keys': 400, 'ops_per_key': 300, 'concurrency': 16, 'info_rate': 0.01, 'anomaly_rate': 0.15, 'seed': 1}, 84, 'hbm_narrow', 12, 1696, 4120, 1),
    ({'n_keys': 400, 'ops_per_key': 300, 'concurrency': 16, 'info_rate': 0.01, 'anomaly_rate': 0.15, 'seed': 1}, 113, 'hbm_narrow', 15, 7552, 28576, 0),
]

# The grids searched are find_edge_keys.py's T1_GRID, T2_GRID and HBM_GRID.
CLASSES = ("t1_fit", "t1_over_S", "t1_over_I", "t2_fit", "t2_over_S", "t2_over_I", "hbm_narrow")


def _tier_class(name: str, maxS: int, maxI: int, cap_s: int, cap_i: int):
    if maxS <= cap_s and maxI <= cap_i:
        return f"{name}_fit" if (maxS == cap_s or maxI == cap_i) else None
    if cap_s < maxS <= cap_s + BATCH and maxI <= cap_i:
        return f"{name}_over_S"
    if cap_i < maxI <= cap_i + BATCH and maxS <= cap_s:
        return f"{name}_over_I"
    return None


def classify(sizeI: np.ndarray, sizeS: np.ndarray):
    """The edge class of a key with these unbounded sizes, or None."""
    maxS, maxI = int(sizeS.max(initial=1)), int(sizeI.max(initial=1))
    if maxS <= T1_S + BATCH and maxI <= T1_I + BATCH:
        return _tier_class("t1", maxS, maxI, T1_S, T1_I)
    if maxS <= T2_S + BATCH and maxI <= T2_I + BATCH:
        c = _tier_class("t2", maxS, maxI, T2_S, T2_I)
        if c is not None:
            return c
    if maxS > T2_S or maxI > T2_I:  # beyond T2: an :ok on or just past the HBM tier's LDS-pass limits
        onS = ((sizeS >= HBM_LIM_S) & (sizeS <= HBM_LIM_S + BATCH)).any()
        onI = ((sizeI >= HBM_LIM_I) & (sizeI <= HBM_LIM_I + BATCH)).any()
        if onS or onI:
            return "hbm_narrow"
    return None


def features(cls: str, sizeI: np.ndarray, sizeS: np.ndarray, valid: int) -> frozenset:
    """What a key of class cls adds to its class's cases (find_edge_keys.py
    picks keys so that each feature found is pinned once)."""
    f = set()
    if valid == 0:
        f.add("invalid")
    if cls == "hbm_narrow":
        for name, a, lim in (("S'", sizeS, HBM_LIM_S), ("I", sizeI, HBM_LIM_I)):
            if (a == lim).any():
                f.add(f"|{name}| == {lim}")
            if ((a > lim) & (a <= lim + BATCH)).any():
                f.add(f"|{name}| just past {lim}")
    elif cls.endswith("_fit"):
        cap_s, cap_i = (T1_S, T1_I) if cls.startswith("t1") else (T2_S, T2_I)
        if sizeS.max(initial=1) == cap_s:
            f.add("|S'| == CAP_S")
        if sizeI.max(initial=1) == cap_i:
            f.add("|I| == CAP_I")
    return frozenset(f)


@lru_cache(maxsize=4)
def _synth(items: tuple) -> H.History:
    return H.synth(**dict(items))


@dataclass
class EdgeBatch:
    cls: str
    rows: List[tuple]         # the TABLE rows, batch order (key i of the batch is rows[i])
    hist: H.History
    pk: Packed
    sizeI: List[np.ndarray]   # unbounded sizes per key
    sizeS: List[np.ndarray]
    need: List[int]

    def describe(self, i: int) -> str:
        kw, k, cls, pend, peak, maxI, valid = self.rows[i]
        return (f"{cls} key {i} (seed {kw['seed']} conc {kw['concurrency']} ops {kw['ops_per_key']} key {k}): "
                f"pending {pend}, max |S'| {peak}, max |I| {maxI}, need {self.need[i]}, "
                f"{'valid' if valid == 1 else 'invalid'}")


def renumbered(hist: H.History, key: int, new_key: int) -> H.History:
    """Key `key` of hist alone, renumbered to new_key."""
    part = hist.select_keys([key])
    assert len(part) > 0, f"no key {key}"
    part.key = np.full(len(part), new_key, np.int64)
    return part


def one_key(kw: Dict, key: int, new_key: int) -> H.History:
    """Key `key` of synth(**kw) alone, renumbered to new_key."""
    return renumbered(_synth(tuple(sorted(kw.items()))), key, new_key)


def merge(parts: List[H.History]) -> H.History:
    return H.History.concat(parts)


_built: Dict[str, EdgeBatch] = {}


def build(name: str, rows: List[tuple]) -> EdgeBatch:
    """The rows' keys as one batch (keys 0, 1, ... in order), every
    precondition asserted: sizes and verdict as pinned, the key's class still
    the row's (None: a budget target of no capacity class), and (T1, T2
    classes) 11 ops pending somewhere."""
    hist = merge([one_key(r[0], r[1], i) for i, r in enumerate(rows)])
    pk = Packed(hist)
    assert pk.keys == list(range(len(rows)))
    hc = hist.as_c()
    sI, sS, need = [], [], []
    for i, (kw, k, cls, pend, peak, maxI, valid) in enumerate(rows):
        a, b, res = cref.key_sizes(hc, i, budget=UNBOUNDED, result=True)
        got = (int(pending_before(pk, i).max()), int(b.max(initial=1)), int(a.max(initial=1)), int(res.valid))
        assert got == (pend, peak, maxI, valid), f"{cls} key {k} of synth({kw}): {got}, pinned {(pend, peak, maxI, valid)}: {RERUN}"
        if cls is not None:
            assert classify(a, b) == cls, f"{cls} key {k} of synth({kw}) is now {classify(a, b)}: {RERUN}"
        if cls is not None and cls != "hbm_narrow":
            assert pend >= LEAVES_REGISTER_TIER, f"{cls} key {k} stays in the register tier: {RERUN}"
        sI.append(a)
        sS.append(b)
        need.append(int(max(a.max(initial=1), b.max(initial=1))))
    return EdgeBatch(name, rows, hist, pk, sI, sS, need)


def batch(cls: str) -> EdgeBatch:
    """The class's pinned keys as one batch, in TABLE order."""
    if cls not in _built:
        rows = [r for r in TABLE if r[2] == cls]
        assert len(rows) >= 2, f"{cls}: fewer than 2 keys pinned"
        _built[cls] = build(cls, rows)
    return _built[cls]


def rows_of(cls: str) -> List[tuple]:
    return [r for r in TABLE if r[2] == cls]
