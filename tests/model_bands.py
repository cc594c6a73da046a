"""Batches that take (model/multi-register), (model/register) and (model/mutex)
through every set tier, pinned.

A band is a batch of at most 12 keys of one model.  Each key is a key of one
generator call (tests/histgen.py), named by that call and not by its ops; the
calls and keys below were chosen once by a search on the CPU (seeds 1-40 of the
shapes listed at each band, every key classified from the oracle's unbounded
set sizes) and are rebuilt from their seeds.  ModelBand asserts that every key
still has the class, need and verdict it is listed with, so a change to a
generator or to a capacity cannot quietly turn a deep key into a shallow one.

need(key) = max(max |I|, max |S'|) over the events the unbounded :linear search
walks.  For register and mutex the sizes and records are the C restatement's
(cref.key_sizes / cref.check_history); for multi-register, which the C
restatement does not know, they are oracle/linear_ref.py's (Analysis.size_I,
size_S, peak_configs, probes) and, for WGL, oracle/wgl_ref.py's.

The tier classes restate the kernels' capacities (edge_keys.py: T1 256 / 512,
T2 1024 / 4096, the HBM tier's LDS pass 2048 / 4096, as CAP_S / CAP_I); they
place keys only, expected results always come from an oracle:
  t1           the key never passes T1
  t2           it passes T1 but not T2
  hbm_lds      it is past T2, and every :ok fits the HBM tier's LDS pass
  hbm_hbm      some :ok is past the LDS pass
  wide_states  more than 255 states (wide configs) and a need of at least 500
  wide_small   more than 255 states, smaller sets"""
from __future__ import annotations

from typing import Dict, List

import numpy as np

import cref
import edgegen
import histgen
import linear_ref as LR
import wgl_ref as W
from edge_keys import HBM_LIM_I, HBM_LIM_S, T1_I, T1_S, T2_I, T2_S
from lincheck import _native as N
from lincheck import history as H
from lincheck import model
from lincheck.checker import Packed
from lincheck.independent import Tuple

UNBOUNDED = 1 << 40
NARROW_MAX_STATES = 255          # include/lincheck.h LC_NARROW_MAX_STATES
WIDE_MIN_NEED = 500
BUDGET_CAUSE = 2
CAUSE = {"none": 0, "nonlin": 1, "budget": 2, "window": 3, "states": 4}
VALID = {True: 1, False: 0, "unknown": -1}
MAX_KEYS = 12
RERUN = "search again (the module docstring names the shapes) and replace the band's rows"

MODELS = {"multi-register": model.multi_register, "register": model.register, "mutex": model.mutex,
          "cas-register": model.cas_register}
RECORD = np.dtype([("valid", np.int8), ("cause", np.uint8), ("fail_event", np.int32), ("peak", np.uint32),
                   ("probes", np.uint64)])

# ------------------------------------------------------------------ the generator calls
MR2 = dict(n_keys=8, n_ops=60, regs=("x", "y"), values=(0, 1, 2), corrupt=0.4)        # 16 maps
MR4 = dict(n_keys=8, n_ops=60, regs=(1, 2, 3, 4), values=(0, 1, 2, 3, 4), corrupt=0.4)  # up to 6^4 maps
CALLS = {
    "mr_p12w6_s31": ("multi_register_history", dict(seed=31, procs=12, width=6.0, **MR2)),
    "mr_p12w6_s32": ("multi_register_history", dict(seed=32, procs=12, width=6.0, **MR2)),
    "mr_p12w6_s34": ("multi_register_history", dict(seed=34, procs=12, width=6.0, **MR2)),
    "mr_p14w7_s31": ("multi_register_history", dict(seed=31, procs=14, width=7.0, **MR2)),
    "mr4_p12w6_s31": ("multi_register_history", dict(seed=31, procs=12, width=6.0, **MR4)),
    "reg7_s1": ("register_history", dict(seed=1, n_keys=12, n_ops=70, procs=10, n_values=7, p_info=0.08, corrupt=0.4)),
    "reg7_s2": ("register_history", dict(seed=2, n_keys=12, n_ops=70, procs=10, n_values=7, p_info=0.08, corrupt=0.4)),
    "reg12_s2": ("register_history", dict(seed=2, n_keys=12, n_ops=70, procs=10, n_values=12, p_info=0.08, corrupt=0.4)),
    "reg12_s5": ("register_history", dict(seed=5, n_keys=12, n_ops=70, procs=10, n_values=12, p_info=0.08, corrupt=0.4)),
    "reg1000_s1": ("register_history", dict(seed=1, n_keys=6, n_ops=700, procs=8, n_values=1000, p_info=0.012,
                                            corrupt=0.4, p_write=0.6)),
    "reg1000_s3": ("register_history", dict(seed=3, n_keys=6, n_ops=700, procs=8, n_values=1000, p_info=0.012,
                                            corrupt=0.4, p_write=0.6)),
    "mutex_s7": ("mutex_crash_history", dict(seed=7, n_keys=12, rounds=60, procs=6, p_info=0.2, corrupt=0.4)),
    "mutex_s11": ("mutex_crash_history", dict(seed=11, n_keys=12, rounds=60, procs=6, p_info=0.2, corrupt=0.4)),
    "mutex_s26": ("mutex_crash_history", dict(seed=26, n_keys=12, rounds=60, procs=6, p_info=0.2, corrupt=0.4)),
    "mutex_s33": ("mutex_crash_history", dict(seed=33, n_keys=12, rounds=60, procs=6, p_info=0.2, corrupt=0.4)),
}

# band -> (model, [(call, key, class, max |I|, max |S'|, valid)])
ROWS: Dict[str, tuple] = {
    # two registers x three values, 12 / 14 processes, intervals 6 / 7 wide (seeds 31-34 searched)
    "mr_narrow": ("multi-register", [
        ("mr_p12w6_s32", 0, "t2", 736, 440, 0),
        ("mr_p12w6_s32", 1, "t1", 186, 102, 0),
        ("mr_p12w6_s32", 2, "t2", 1176, 688, 1),
        ("mr_p12w6_s32", 3, "hbm_hbm", 4000, 3092, 1),
        ("mr_p12w6_s32", 4, "t2", 532, 248, 1),
        ("mr_p12w6_s32", 5, "t1", 312, 224, 1),
        ("mr_p12w6_s32", 6, "hbm_lds", 1974, 1200, 1),
        ("mr_p12w6_s32", 7, "t2", 592, 448, 1),
        ("mr_p12w6_s34", 1, "t2", 848, 864, 1),
        ("mr_p14w7_s31", 1, "hbm_hbm", 4543, 2672, 1),
        ("mr_p12w6_s31", 5, "t2", 1295, 700, 0),
    ]),
    # four registers x five values (up to 6^4 maps): wide configs
    "mr_wide": ("multi-register", [
        ("mr4_p12w6_s31", 0, "wide_states", 1728, 1232, 0),
        ("mr4_p12w6_s31", 1, "wide_states", 1352, 744, 1),
        ("mr4_p12w6_s31", 3, "wide_states", 529, 473, 1),
        ("mr4_p12w6_s31", 7, "wide_states", 2422, 2422, 1),
    ]),
    # 7 values: 8 states with nil, the most the layered tier takes
    "reg7": ("register", [
        ("reg7_s1", 10, "hbm_lds", 2560, 1536, 1),
        ("reg7_s1", 8, "t2", 1536, 512, 1),
        ("reg7_s1", 1, "t2", 1408, 768, 0),
        ("reg7_s1", 4, "t2", 1152, 512, 0),
        ("reg7_s1", 2, "t1", 448, 192, 0),
        ("reg7_s2", 1, "hbm_hbm", 5216, 1408, 1),
        ("reg7_s2", 7, "t2", 2560, 1024, 1),
    ]),
    # 12 values: 13 states, the layered tier hands the key on
    "reg12": ("register", [
        ("reg12_s2", 6, "hbm_hbm", 4160, 1536, 0),
        ("reg12_s2", 4, "hbm_hbm", 4544, 768, 1),
        ("reg12_s2", 11, "t2", 2640, 896, 1),
        ("reg12_s2", 7, "t2", 1824, 640, 0),
        ("reg12_s5", 2, "hbm_lds", 3072, 1280, 1),
    ]),
    # 1000 values drawn, 300+ written per key: wide by state count
    "reg_wide": ("register", [
        ("reg1000_s1", 5, "wide_states", 2176, 832, 1),
        ("reg1000_s1", 3, "wide_states", 576, 192, 0),
        ("reg1000_s1", 2, "wide_small", 170, 60, 1),
        ("reg1000_s3", 3, "wide_states", 3584, 1088, 0),
    ]),
    # 60 rounds, one op in five crashed (seeds 1-40 searched)
    "mutex": ("mutex", [
        ("mutex_s11", 6, "hbm_lds", 1871, 1659, 1),
        ("mutex_s11", 7, "t2", 1156, 545, 0),
        ("mutex_s11", 4, "t1", 10, 6, 0),
        ("mutex_s26", 1, "hbm_hbm", 4025, 2611, 1),
        ("mutex_s33", 11, "hbm_lds", 2811, 1130, 1),
        ("mutex_s7", 6, "t2", 2687, 816, 1),
    ]),
}

_calls: Dict[str, list] = {}


def call_ops(call: str) -> list:
    if call not in _calls:
        gen, kw = CALLS[call]
        _calls[call] = getattr(histgen, gen)(**kw)
    return _calls[call]


def key_ops(call: str, key: int, new_key: int) -> list:
    """Key `key` of a generator call, renumbered to new_key, with processes of its own."""
    out = []
    procs: Dict[int, int] = {}
    for op in call_ops(call):
        if op["value"][0] != key:
            continue
        p = procs.setdefault(op["process"], 10_000 * (new_key + 1) + len(procs))
        out.append({"type": op["type"], "f": op["f"], "value": Tuple(new_key, op["value"][1]), "process": p})
    assert out, f"{call} has no key {key}"
    return out


def tier_class(sI: np.ndarray, sS: np.ndarray, states: int) -> str:
    maxI, maxS = int(sI.max(initial=1)), int(sS.max(initial=1))
    if states > NARROW_MAX_STATES:
        return "wide_states" if max(maxI, maxS) >= WIDE_MIN_NEED else "wide_small"
    if maxS <= T1_S and maxI <= T1_I:
        return "t1"
    if maxS <= T2_S and maxI <= T2_I:
        return "t2"
    if maxS <= HBM_LIM_S and maxI <= HBM_LIM_I:
        return "hbm_lds"
    return "hbm_hbm"


def sizes_of(a: LR.Analysis):
    """linear_ref's per-event sizes as cref.key_sizes gives them: one entry
    per event walked, 0 at an :invoke."""
    n = max(list(a.size_I) + list(a.size_S) + [-1]) + 1
    if a.valid is True:
        n = len(a.events)
    sI, sS = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    for e, v in a.size_I.items():
        sI[e] = v
    for e, v in a.size_S.items():
        sS[e] = v
    return sI, sS


def record_of(a) -> tuple:
    fe = getattr(a, "fail_event", None)
    return (VALID[a.valid], CAUSE[a.cause], -1 if fe is None else fe, getattr(a, "peak_configs", 0),
            getattr(a, "probes", 0))


class ModelBand:
    """A batch of one model, its unbounded sizes per key and the oracles'
    records per budget.  `table`: the model the C restatement does not know."""

    def __init__(self, name: str):
        self.name = name
        self.model_name, self.rows = ROWS[name]
        assert len(self.rows) <= MAX_KEYS
        self.table = self.model_name == "multi-register"
        self.ops: List[dict] = []
        for i, r in enumerate(self.rows):
            self.ops += key_ops(r[0], r[1], i)
        for i, op in enumerate(self.ops):
            op["index"] = i
        self.hist = H.History.from_ops(self.ops)
        self.model = MODELS[self.model_name]()
        self.pk = Packed(self.hist, self.model)
        self.hc = self.hist.as_c()
        K = self.pk.n_keys
        assert self.pk.keys == list(range(len(self.rows)))
        self.subs = [LR.subhistory(self.ops, k) for k in range(K)]
        self._lin: Dict[int, list] = {}
        self._wgl: Dict[int, list] = {}
        self._orc: Dict[int, np.ndarray] = {}
        self._full: Dict[int, LR.Analysis] = {}
        if self.table:
            self.states = [int(x) for x in N.carray(self.pk.view.key_states, K, np.uint16)]
            self.sizes = [sizes_of(a) for a in self.linear(UNBOUNDED)]
        else:
            self.states = [int(x) for x in edgegen.batch_states(self.pk)] if K else []
            self.sizes = [cref.key_sizes(self.hc, k, budget=UNBOUNDED, model=self.model_name) for k in range(K)]
        self.need = [int(max(a.max(initial=1), b.max(initial=1))) for a, b in self.sizes]
        self.cls = [tier_class(a, b, s) for (a, b), s in zip(self.sizes, self.states)]
        self.names = [f"{c}:{r[0]}/key{r[1]}" for c, r in zip(self.cls, self.rows)]
        full = self.oracle(UNBOUNDED)
        for i, (call, key, cls, maxI, maxS, valid) in enumerate(self.rows):
            sI, sS = self.sizes[i]
            got = (self.cls[i], int(sI.max(initial=1)), int(sS.max(initial=1)), int(full["valid"][i]))
            want = (cls, got[1] if maxI is None else maxI, got[2] if maxS is None else maxS, valid)
            assert got == want, f"{name}: key {key} of {call} is {got}, pinned {want}: {RERUN}"

    # -- oracles
    def linear(self, budget: int) -> list:
        """linear_ref's analysis of every key at this budget.  The budget
        enters linear_ref only through its two `len(...) > budget` tests, so a
        key whose need is within the budget has its unbounded analysis."""
        if budget not in self._lin:
            out = []
            for i, sub in enumerate(self.subs):
                if budget != UNBOUNDED and self.need[i] <= budget:
                    out.append(self.linear(UNBOUNDED)[i])
                else:
                    out.append(LR.analysis(sub, budget=budget, model=self.model_name))
            self._lin[budget] = out
        return self._lin[budget]

    def wgl(self, budget: int) -> list:
        """wgl_ref's analysis of every key at this budget (the budget bounds
        Lowe's cache, tested as `len(cache) > budget` alone)."""
        if budget not in self._wgl:
            out = []
            for i, sub in enumerate(self.subs):
                full = self._wgl.get(UNBOUNDED)
                if full is not None and full[i].cause != "budget" and full[i].cache_size <= budget:
                    out.append(full[i])
                else:
                    out.append(W.analysis(sub, budget=budget, model=self.model_name))
            self._wgl[budget] = out
        return self._wgl[budget]

    def oracle(self, budget: int) -> np.ndarray:
        """The :linear records at this budget: valid, cause, fail_event, peak, probes."""
        if budget not in self._orc:
            if self.table:
                self._orc[budget] = np.array([record_of(a) for a in self.linear(budget)], RECORD)
            else:
                keys, orc = cref.check_history(self.hc, budget=budget, threads=8, model=self.model_name)
                assert list(keys) == self.pk.keys
                self._orc[budget] = orc
        return self._orc[budget]

    def analysis(self, i: int) -> LR.Analysis:
        """linear_ref's unbounded analysis of key i (any model): the final configs."""
        if self.table:
            return self.linear(UNBOUNDED)[i]
        if i not in self._full:
            self._full[i] = LR.analysis(self.subs[i], budget=UNBOUNDED, model=self.model_name)
        return self._full[i]

    # -- what a key is
    def past_t2(self, i: int) -> bool:
        return self.cls[i] in ("hbm_lds", "hbm_hbm")

    def deep(self, i: int) -> bool:
        """Searched by an HBM tier at an ample budget: past T2, or wide configs."""
        return self.past_t2(i) or self.cls[i].startswith("wide")

    def deciding(self, i: int):
        """(event, |I|, |S'|) where key i's sets first reach its need."""
        sI, sS = self.sizes[i]
        e = int(np.flatnonzero((sI == self.need[i]) | (sS == self.need[i]))[0])
        return e, int(sI[e]), int(sS[e])

    def first_past(self, i: int, budget: int) -> int:
        sI, sS = self.sizes[i]
        return int(np.flatnonzero((sI > budget) | (sS > budget))[0])

    def first_ok(self, i: int) -> int:
        return int(np.flatnonzero(self.pk.events(i) >> 31)[0])

    def describe(self, i: int) -> str:
        e, nI, nS = self.deciding(i)
        full = self.oracle(UNBOUNDED)[i]
        by = "|S'|" if nI < self.need[i] else "|I|"
        return (f"{self.name} / {self.names[i]}: {self.states[i]} states, need {self.need[i]} by {by} at event {e} "
                f"(|I| {nI}, |S'| {nS}); unbounded verdict {int(full['valid'])}, fails at {int(full['fail_event'])}")


def slots_of(events) -> Dict[int, int]:
    """Window slot of every op (lowest free at :invoke, freed at :ok), as lc_pack assigns them."""
    free, slot = list(range(128)), {}
    for kind, oid, _ in events:
        if kind == "invoke":
            slot[oid] = min(free)
            free.remove(slot[oid])
        else:
            free.append(slot[oid])
    return slot


def oracle_state(st, model_name: str):
    """An oracle's model state in the form device_state() decodes to."""
    if model_name == "multi-register":
        return tuple(st)
    if model_name == "mutex":
        return 1 if st else None  # helpers.oracle_state_value: lc_pack interns locked as 1
    return st


def device_state(pk: Packed, i: int, st: int, model_name: str):
    """State id st of key i as the model's value: the map (sorted as
    linear_ref sorts it) of a multi-register key, else the interned value."""
    if model_name == "multi-register":
        return tuple(sorted(pk.state_map(i, st), key=LR._reg_order))
    return pk.state_value(i, st)


def record_configs(rec: np.ndarray, n: int):
    """Final / frontier records as [(state id, slot mask)] (lo = slots 0..63,
    hi = slots 64..111 | state << 48)."""
    out = []
    for j in range(int(n)):
        lo, hi = (int(x) for x in rec[j])
        out.append(((hi >> 48) & 0x7FFF, lo | ((hi & ((1 << 48) - 1)) << 64)))
    return out


def oracle_configs(configs, slot: Dict[int, int], model_name: str) -> set:
    """An oracle's (state, linearized op ids) configs as {(state, slot mask)}."""
    out = set()
    for st, lin in configs:
        m = 0
        for q in lin:
            m |= 1 << slot[q]
        out.add((oracle_state(st, model_name), m))
    return out


_maps_memo: Dict[tuple, int] = {}
_reachable_maps = LR.reachable_maps


def memoised_reachable_maps(ops, initial, cap: int) -> int:
    """LR.reachable_maps, counted once per (distinct :txn values, initial map,
    cap): the count of a key with 32,767 maps takes ten seconds, and the
    :linear and the WGL restatement both begin with it."""
    ops = list(ops)
    key = (tuple(sorted({repr(o.value) for o in ops if not o.failed})), initial, cap)
    if key not in _maps_memo:
        _maps_memo[key] = _reachable_maps(ops, initial, cap)
    return _maps_memo[key]


_bands: Dict[str, ModelBand] = {}


def band(name: str) -> ModelBand:
    if name not in _bands:
        _bands[name] = ModelBand(name)
    return _bands[name]


# ------------------------------------------------------------------ targets pinned for the GPU tests
# knossos.competition on the table model: at this budget linear_ref gives up on keys 2, 3, 6, 9 and 10 of
# mr_narrow (needs 1176 - 4543); wgl_ref decides 2, 3, 6 and 9 (caches of 88 - 313) and gives up on 10 as well
COMPETITION_BUDGET = 1024
WGL_MIGRATE = 2048               # device_wgl.hip: the cache moves from LDS to HBM past lds_tab / 2 = 2048 pairs
WGL_SMALL_SPILL = (1 << 14) // 2  # LC_PATH_WGL_SMALL: a key spills once its cache would reach this
# mr_narrow keys by Lowe's cache at the end of the unbounded walk (test_model_bands pins them)
WGL_ABOVE_MIGRATE = (0, 1, 10)   # 2688, 2190, 9653 pairs
WGL_BELOW_MIGRATE = (2, 3, 4, 5, 6, 7, 8, 9)
WGL_SPILLS = (10,)               # 9653 >= 8192


# ------------------------------------------------------------------ the state-count limit
def sequential(ops_of_key: list, key: int, process: int) -> list:
    """(f, invoke value, ok value) triples as a sequential key: every set has one config."""
    out = []
    for f, v, done in ops_of_key:
        out.append({"type": "invoke", "f": f, "value": Tuple(key, v), "process": process})
        out.append({"type": "ok", "f": f, "value": Tuple(key, done), "process": process})
    return out


def map_limit_txns(counts, bad_last_read: bool) -> list:
    """Sequential :txn ops writing counts[r] distinct values (1 ..) to register
    r, one write per op, then a read of every register's last value.  With the
    empty initial map the reachable maps are prod(counts[r] + 1): a register
    is absent or holds one of its values.  bad_last_read: the read sees 0 in
    the last register, a value nothing writes."""
    out = []
    for r, n in enumerate(counts):
        for v in range(1, n + 1):
            w = [["write", r, v]]
            out.append(("txn", w, w))
    rd = [["read", r, None] for r in range(len(counts))]
    seen = [["read", r, n] for r, n in enumerate(counts)]
    if bad_last_read:
        seen[-1][2] = 0
    out.append(("txn", rd, seen))
    return out


MAPS_AT_LIMIT = (6, 30, 150)     # 7 x 31 x 151 = 32,767 = LC_WIDE_MAX_STATES maps
MAPS_PAST_LIMIT = (7, 7, 7, 63)  # 8 x 8 x 8 x 64 = 32,768


def ordinary_txn_key(seed: int, corrupt: float) -> list:
    ops = histgen.multi_register_history(seed, n_keys=1, n_ops=20, procs=4, regs=(0, 1), values=(1, 2, 3), corrupt=corrupt)
    return [(op["type"], op["f"], op["value"][1], op["process"]) for op in ops]


def map_limit_ops() -> list:
    """Keys 0 (invalid) and 3 (valid) ordinary, key 1 with exactly 32,767
    reachable maps and an impossible last read, key 2 with 32,768."""
    ops = []
    for k, seed, corrupt in ((0, 5, 1.0), (3, 6, 0.0)):
        if k == 3:
            ops += sequential(map_limit_txns(MAPS_AT_LIMIT, True), 1, 100)
            ops += sequential(map_limit_txns(MAPS_PAST_LIMIT, False), 2, 200)
        ops += [{"type": t, "f": f, "value": Tuple(k, v), "process": 1000 * (k + 1) + p}
                for t, f, v, p in ordinary_txn_key(seed, corrupt)]
    for i, op in enumerate(ops):
        op["index"] = i
    return ops


VALUES_AT_LIMIT = 32766          # + nil = 32,767 states
VALUES_PAST_LIMIT = 32767


def value_limit_ops() -> list:
    """cas-register: keys 0 and 3 ordinary, key 1 writing 32,766 distinct
    values and reading the last (the highest state id), key 2 writing 32,767."""
    def writes(n):
        return [("write", v, v) for v in range(1, n + 1)] + [("read", None, n)]
    ops = []
    for k, seed in ((0, 7), (3, 8)):
        if k == 3:
            ops += sequential(writes(VALUES_AT_LIMIT), 1, 100)
            ops += sequential(writes(VALUES_PAST_LIMIT), 2, 200)
        for op in histgen.random_history(seed, n_keys=1, max_ops=12, procs=3, p_nemesis=0.0):
            ops.append({"type": op["type"], "f": op["f"], "value": Tuple(k, op["value"][1]),
                        "process": 1000 * (k + 1) + op["process"]})
    for i, op in enumerate(ops):
        op["index"] = i
    return ops
