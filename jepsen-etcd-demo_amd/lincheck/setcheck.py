"""Mirror of jepsen.checker/set for the demo's set workload (set.clj:42-49).

    checker.set_()        (checker/set) on the device: every acknowledged :add
                          must be in the final :read, and the read may hold only
                          attempted elements.  Result map, Jepsen's keys as strings:
                          {"valid?", "attempt-count", "acknowledged-count",
                           "ok-count", "lost-count", "recovered-count",
                           "unexpected-count", "ok", "lost", "unexpected",
                           "recovered"}, the four sets as interval strings
                          (jepsen.util/integer-interval-set-str: "#{0..2 4 7..9}").

The path is its own: SetHistory (lc_set_history) -> PackedSet (lc_set_pack) ->
lc_set_check -> result maps rendered from the run lists.  Under
independent.checker every key is checked in one lc_set_check call.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence

import numpy as np

from . import _native as N
from .independent import Tuple, is_tuple

I64_MAX = (1 << 63) - 1
COUNT_KEYS = ("attempt-count", "acknowledged-count", "ok-count", "lost-count", "recovered-count", "unexpected-count")
RUN_KEYS = ("ok", "lost", "unexpected", "recovered")  # lc_set_result.runs' class order
TYPES = {"invoke": N.LC_INVOKE, "ok": N.LC_OK_T, "fail": N.LC_FAIL, "info": N.LC_INFO}
TYPE_NAMES = {v: k for k, v in TYPES.items()}


def _name(x) -> str:
    return str(x).lstrip(":")


def _elem(v) -> int:
    """An element as the C ABI holds it: LC_NIL for nil or anything that is
    no 64-bit integer."""
    if isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) and -I64_MAX <= int(v) <= I64_MAX:
        return int(v)
    return N.LC_NIL


class SetHistory:
    """A raw set-workload history as struct-of-arrays (lc_set_history)."""

    def __init__(self, type_, f, key, elem, read_off, read_elem, index=None):
        self.type = np.ascontiguousarray(type_, np.uint8)
        self.f = np.ascontiguousarray(f, np.uint8)
        self.key = None if key is None else np.ascontiguousarray(key, np.int64)
        self.elem = np.ascontiguousarray(elem, np.int64)
        self.read_off = np.ascontiguousarray(read_off, np.int64)
        self.read_elem = np.ascontiguousarray(read_elem if len(read_elem) else [0], np.int64)
        self.index = None if index is None else np.ascontiguousarray(index, np.int64)
        self.n = len(self.type)

    @classmethod
    def from_ops(cls, ops: Sequence[dict]) -> "SetHistory":
        """Op maps ({"type", "f", "value", "index"}; independent tuples as
        lincheck.independent.tuple) to columns, by the rules of lc_edn_read_set."""
        n = len(ops)
        type_, f = np.zeros(n, np.uint8), np.full(n, N.LC_SF_OTHER, np.uint8)
        key, elem, index = np.full(n, N.LC_NO_KEY, np.int64), np.zeros(n, np.int64), np.full(n, -1, np.int64)
        read_off, read_elem = np.zeros(n + 1, np.int64), []
        for r, op in enumerate(ops):
            type_[r] = TYPES[_name(op["type"])]
            fn = _name(op.get("f"))
            if op.get("index") is not None:
                index[r] = int(op["index"])
            if fn in ("add", "read"):
                v = op.get("value")
                if is_tuple(v):
                    k, v = v[0], v[1]
                    if _elem(k) == N.LC_NIL:
                        raise ValueError(f"op {r}: tuple key is not an integer")
                    key[r] = int(k)
                if fn == "add":
                    f[r] = N.LC_SF_ADD
                    elem[r] = _elem(v)
                else:
                    f[r] = N.LC_SF_READ
                    if v is None:
                        elem[r] = N.LC_NIL
                    elif isinstance(v, (set, frozenset, list, tuple)):
                        read_elem.extend(_elem(x) for x in v)
                    else:
                        read_elem.append(N.LC_NIL)
            read_off[r + 1] = len(read_elem)
        return cls(type_, f, key, elem, read_off, np.array(read_elem, np.int64), index)

    @classmethod
    def read_edn(cls, path: str) -> "SetHistory":
        """lc_edn_read_set: a set-workload history.edn."""
        h = C.c_void_p()
        N.check(N.lib().lc_edn_read_set(str(path).encode(), C.byref(h)))
        try:
            return cls._from_handle(h)
        finally:
            N.lib().lc_set_hist_free(h)

    @classmethod
    def parse_edn(cls, text: str) -> "SetHistory":
        data = text.encode()
        h = C.c_void_p()
        N.check(N.lib().lc_edn_parse_set(data, len(data), C.byref(h)))
        try:
            return cls._from_handle(h)
        finally:
            N.lib().lc_set_hist_free(h)

    @classmethod
    def _from_handle(cls, h) -> "SetHistory":
        v = N.LcSetHistory()
        N.check(N.lib().lc_set_hist_view(h, C.byref(v)))
        n = int(v.n)
        read_off = N.carray(v.read_off, n + 1, np.int64)
        return cls(N.carray(v.type, n, np.uint8), N.carray(v.f, n, np.uint8), N.carray(v.key, n, np.int64),
                   N.carray(v.elem, n, np.int64), read_off, N.carray(v.read_elem, int(read_off[-1]), np.int64),
                   N.carray(v.index, n, np.int64))

    def as_c(self) -> N.LcSetHistory:
        null64 = C.POINTER(C.c_int64)()
        return N.LcSetHistory(self.n, N.ptr(self.type, C.c_uint8), N.ptr(self.f, C.c_uint8),
                              null64 if self.key is None else N.ptr(self.key, C.c_int64), N.ptr(self.elem, C.c_int64),
                              N.ptr(self.read_off, C.c_int64), N.ptr(self.read_elem, C.c_int64),
                              null64 if self.index is None else N.ptr(self.index, C.c_int64))

    def to_ops(self) -> List[dict]:
        """The rows as op maps again (tests; small histories)."""
        out = []
        fs = {N.LC_SF_ADD: "add", N.LC_SF_READ: "read", N.LC_SF_OTHER: "other"}
        for r in range(self.n):
            fn = fs[int(self.f[r])]
            v: Any = None
            if fn == "add":
                v = None if self.elem[r] == N.LC_NIL else int(self.elem[r])
            elif fn == "read" and self.elem[r] != N.LC_NIL:
                v = [None if x == N.LC_NIL else int(x) for x in self.read_elem[self.read_off[r]:self.read_off[r + 1]]]
            if fn != "other" and self.key is not None and self.key[r] != N.LC_NO_KEY:
                v = Tuple(int(self.key[r]), v)
            out.append({"type": TYPE_NAMES[int(self.type[r])], "f": fn, "value": v,
                        "index": r if self.index is None else int(self.index[r])})
        return out


def synth_set(n_keys: int = 1, adds_per_key: int = 1000, concurrency: int = 10, info_rate: float = 0.02,
              lost_rate: float = 0.0, unexpected_rate: float = 0.0, seed: int = 1, shuffle: bool = False) -> SetHistory:
    """A synthetic set-workload history of the demo's shape (set.clj:25-35, for
    tests and timing only): per key the elements 0 .. adds_per_key - 1 from
    (range), added by `concurrency` clients at a time (that many :invoke rows,
    then their completions, :info at info_rate, else :ok), then one final
    read: the acknowledged elements less lost_rate of them, half of the :info
    ones, and unexpected_rate * adds_per_key elements nobody added.  Keys are
    laid out one after the other; several keys make tuple values.  shuffle:
    the elements in random order.  Built with numpy, no op maps."""
    rng = np.random.default_rng(seed)
    A, c = int(adds_per_key), max(1, int(concurrency))
    cols = dict(type=[], f=[], key=[], elem=[], read_len=[])
    reads = []
    for k in range(n_keys):
        el = np.arange(A, dtype=np.int64)
        if shuffle:
            rng.shuffle(el)
        info = rng.random(A) < info_rate
        # rows: groups of c invokes, then their c completions
        g = np.arange(A) // c
        pos = np.arange(A) - g * c
        size = np.minimum(c, A - g * c)
        inv_row = 2 * g * c + pos
        done_row = 2 * g * c + size + pos
        t = np.zeros(2 * A + 2, np.uint8)
        e = np.zeros(2 * A + 2, np.int64)
        t[inv_row] = N.LC_INVOKE
        t[done_row] = np.where(info, N.LC_INFO, N.LC_OK_T)
        e[inv_row] = el
        e[done_row] = el
        f = np.full(2 * A + 2, N.LC_SF_ADD, np.uint8)
        f[-2:] = N.LC_SF_READ
        t[-2], t[-1] = N.LC_INVOKE, N.LC_OK_T
        e[-2], e[-1] = N.LC_NIL, 0
        acked = el[~info]
        keep = acked[rng.random(len(acked)) >= lost_rate] if lost_rate > 0 else acked
        crashed = el[info]
        recovered = crashed[rng.random(len(crashed)) < 0.5]
        extra = A + 10 + 2 * np.arange(int(round(unexpected_rate * A)), dtype=np.int64)
        rd = np.concatenate([keep, recovered, extra])
        rl = np.zeros(2 * A + 2, np.int64)
        rl[-1] = len(rd)
        reads.append(rd)
        cols["type"].append(t); cols["f"].append(f); cols["elem"].append(e); cols["read_len"].append(rl)
        cols["key"].append(np.full(2 * A + 2, k, np.int64))
    cat = {name: np.concatenate(v) for name, v in cols.items()}
    read_off = np.zeros(len(cat["type"]) + 1, np.int64)
    np.cumsum(cat["read_len"], out=read_off[1:])
    return SetHistory(cat["type"], cat["f"], cat["key"] if n_keys > 1 else None, cat["elem"], read_off,
                      np.concatenate(reads) if reads else np.zeros(0, np.int64))


class PackedSet:
    """lc_set_pack output: the per-key id arrays lc_set_check reads."""

    def __init__(self, hist: SetHistory):
        self.hist = hist
        self._c = hist.as_c()
        h = C.c_void_p()
        N.check(N.lib().lc_set_pack(C.byref(self._c), C.byref(h)))
        self.handle = h
        v = N.LcSetBatch()
        N.check(N.lib().lc_set_packed_view(h, C.byref(v)))
        self.view = v
        self.n_keys = int(v.n_keys)
        keys = np.zeros(max(self.n_keys, 1), np.int64)
        N.check(N.lib().lc_set_packed_keys(h, N.ptr(keys, C.c_int64)))
        self.keys = [None if k == N.LC_NO_KEY else int(k) for k in keys[:self.n_keys]]
        self.status = N.carray(v.status, self.n_keys, np.uint8)

    def __del__(self):
        h = getattr(self, "handle", None)
        if h:
            N.lib().lc_set_packed_free(h)
            self.handle = None

    def key_error(self, i: int) -> Optional[str]:
        msg = N.lib().lc_set_packed_key_error(self.handle, i)
        return None if msg is None else msg.decode(errors="replace")

    def arrays(self) -> Dict[str, np.ndarray]:
        """Copies of every array of the view (tests, caller-built batches)."""
        v, K = self.view, self.n_keys
        add_off, read_off = N.carray(v.add_off, K + 1, np.uint64), N.carray(v.read_off, K + 1, np.uint64)
        vals_off = N.carray(v.vals_off, K + 1, np.uint64)
        return dict(add_off=add_off, add_id=N.carray(v.add_id, int(add_off[-1]), np.uint32),
                    add_cls=N.carray(v.add_cls, int(add_off[-1]), np.uint8), read_off=read_off,
                    read_id=N.carray(v.read_id, int(read_off[-1]), np.uint32), base=N.carray(v.base, K, np.uint64),
                    span=N.carray(v.span, K, np.uint32), min=N.carray(v.min, K, np.int64),
                    rank=N.carray(v.rank, K, np.uint8), vals_off=vals_off,
                    vals=N.carray(v.vals, int(vals_off[-1]), np.int64), status=N.carray(v.status, K, np.uint8),
                    n_words=int(v.n_words))


def batch_of(arrs: Dict[str, Any]) -> N.LcSetBatch:
    """An lc_set_batch over numpy arrays (PackedSet.arrays(), or a caller's
    own).  The arrays must outlive the call that reads the batch."""
    pad = {k: (np.ascontiguousarray(v if len(v) else np.zeros(1, v.dtype)) if isinstance(v, np.ndarray) else v)
           for k, v in arrs.items()}
    arrs["_keep"] = pad
    return N.LcSetBatch(len(arrs["span"]), N.ptr(pad["add_off"], C.c_uint64), N.ptr(pad["add_id"], C.c_uint32),
                        N.ptr(pad["add_cls"], C.c_uint8), N.ptr(pad["read_off"], C.c_uint64),
                        N.ptr(pad["read_id"], C.c_uint32), N.ptr(pad["base"], C.c_uint64), N.ptr(pad["span"], C.c_uint32),
                        N.ptr(pad["min"], C.c_int64), N.ptr(pad["rank"], C.c_uint8), N.ptr(pad["vals_off"], C.c_uint64),
                        N.ptr(pad["vals"], C.c_int64), N.ptr(pad["status"], C.c_uint8), int(arrs["n_words"]))


@dataclass
class SetResults:
    valid: np.ndarray    # int8 [K]: 1 / 0 / -1
    counts: np.ndarray   # uint64 [K, 6]: attempt, acknowledged, ok, lost, recovered, unexpected
    run_off: np.ndarray  # uint64 [4 K + 1]
    runs: np.ndarray     # int64 [n_runs, 2]: first and last element of every run
    timing: Dict[str, float]


def check_batch(dev, batch: N.LcSetBatch, run_cap: Optional[int] = None) -> SetResults:
    """lc_set_check on a checker.Device.  run_cap None: a small capacity
    first, and on LC_E_NOMEM once more with the capacity the library names
    (lc_set_batch_max_runs always suffices but is far above what a history
    that is mostly runs needs)."""
    K = int(batch.n_keys)
    valid, counts = np.zeros(max(K, 1), np.int8), np.zeros(max(6 * K, 1), np.uint64)
    run_off = np.zeros(4 * K + 1, np.uint64)
    cap = 4096 if run_cap is None else int(run_cap)
    while True:
        runs = np.zeros(max(2 * cap, 2), np.int64)
        r = N.LcSetResult(N.ptr(valid, C.c_int8), N.ptr(counts, C.c_uint64), N.ptr(run_off, C.c_uint64),
                          N.ptr(runs, C.c_int64), cap, 0)
        rc = N.lib().lc_set_check(dev.handle, C.byref(batch), C.byref(r))
        if rc == -2 and run_cap is None and int(r.n_runs) > cap:
            cap = int(r.n_runs)
            continue
        N.check(rc)
        break
    ms = (C.c_double * 4)()
    N.check(N.lib().lc_set_last_timing(dev.handle, ms))
    n = int(r.n_runs)
    return SetResults(valid[:K], counts[:6 * K].reshape(K, 6), run_off, runs[:2 * n].reshape(n, 2),
                      dict(upload_ms=ms[0], kernel_ms=ms[1], download_ms=ms[2], total_ms=ms[3]))


def interval_str(runs) -> str:
    """jepsen.util/integer-interval-set-str from a key's ascending (first,
    last) runs: a run of one prints as n, a longer one as a..b."""
    return "#{" + " ".join(str(int(a)) if a == b else f"{int(a)}..{int(b)}" for a, b in runs) + "}"


def result_map(packed: PackedSet, res: SetResults, i: int) -> Dict:
    """jepsen.checker/set's result map of packed key i."""
    if packed.status[i] != N.LC_SET_KEY_OK:
        return {"valid?": "unknown", "error": packed.key_error(i) or "error"}
    out: Dict[str, Any] = {"valid?": bool(res.valid[i] == N.LC_VALID)}
    for name, c in zip(COUNT_KEYS, res.counts[i].tolist()):
        out[name] = int(c)
    off = res.run_off[4 * i:4 * i + 5].tolist()
    for j, name in enumerate(RUN_KEYS):
        out[name] = interval_str(res.runs[int(off[j]):int(off[j + 1])].tolist())
    return out


class SetChecker:
    """jepsen.checker/set (set.clj:46) on the device."""

    def __init__(self, opts: Optional[Dict] = None):
        self.device = int((opts or {}).get("device", 0))
        self.path_flags = int((opts or {}).get("path-flags", 0))  # tests: LC_PATH_SET_HBM
        self._dev = None

    def dev(self):
        from . import checker as ck
        if self.path_flags:
            if self._dev is None:
                self._dev = ck.Device(self.device, path_flags=self.path_flags)
            return self._dev
        return ck.device_for(self.device)

    def _check(self, history):
        hist = history if isinstance(history, SetHistory) else SetHistory.from_ops(history)
        packed = PackedSet(hist)
        return packed, check_batch(self.dev(), packed.view)

    def check(self, test: Optional[Dict], history, opts: Optional[Dict] = None) -> Dict:
        """One (unwrapped) history, as at set.clj:46: rows without a key are
        one set; of a keyed history, the first key's."""
        packed, res = self._check(history)
        return result_map(packed, res, 0)

    # batched form, used by independent.checker
    def check_independent(self, test, history, opts, inner) -> Dict:
        from . import checker as ck
        from .independent import merge_results, subhistory
        packed, res = self._check(history)
        results: Dict[Any, Dict] = {}
        parts = [] if inner is self else list(inner.checkers.items())
        ops = None
        for i, k in enumerate(packed.keys):
            if k is None:
                continue  # no tuples: independent/history-keys finds no key
            mine = result_map(packed, res, i)
            if inner is self:
                results[k] = mine
                continue
            r = {}
            for name, ch in parts:
                if ch is self:
                    r[name] = mine
                    continue
                if ops is None:
                    ops = history.to_ops() if isinstance(history, SetHistory) else history
                r[name] = ck.check_safe(ch, test, subhistory(ops, k), dict(opts or {}, **{"history-key": k}))
            r["valid?"] = ck.merge_valid([x.get("valid?") for x in r.values()])
            results[k] = r
        return merge_results(results)


def set_(opts: Optional[Dict] = None) -> SetChecker:
    return SetChecker(opts)
