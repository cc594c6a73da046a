"""Mirror of jepsen.checker/counter for counter workloads.

    checker.counter()
        (checker/counter) on the device: every :ok :read's value must lie
        between the sum of the adds acknowledged when the read was invoked and
        the sum of the adds attempted when it completed
        (include/lincheck_counter.h has the rules; this library's reading of
        the public Jepsen 0.2.x source, parity unpinned).  Result map,
        Jepsen's keys as strings: {"valid?", "reads" ([[lower value upper]
        ...] in the order of the :ok :read rows), "errors" (those of them out
        of bounds)}; a key that breaks a pairing or value rule is
        {"valid?": "unknown", "error": ...}.

The path is its own: CounterHistory (lc_counter_history) -> PackedCounter
(lc_counter_pack) -> lc_counter_check -> result maps.  The device returns each
read's two bounds and the ordered indices of the reads out of bounds.  Under
independent.checker every key is checked in one lc_counter_check call.
{"host": True} runs lc_counter_check_host instead: the same fold in plain C++
on one thread, no device (tests, and the timing's baseline).
{"pack": "device"} takes CounterHistory -> CheckedCounter
(lc_counter_check_history) instead: the raw columns are uploaded, the device
groups, pairs and packs them and checks the batch where it lies, and only
results come back; the result maps are the default path's.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence

import numpy as np

from . import _native as N
from .independent import Tuple, is_tuple
from .setcheck import TYPE_NAMES, TYPES, _elem, _name

F_NAMES = {N.LC_CF_ADD: "add", N.LC_CF_READ: "read", N.LC_CF_OTHER: "other"}
FIRST_ERR_CAP = 1024  # check_batch's first err_idx capacity; a batch with more is checked once more


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


class CounterHistory:
    """A raw counter history as columns (lc_counter_history)."""

    def __init__(self, type_, f, process, key, value, index=None):
        self.type = np.ascontiguousarray(type_, np.uint8)
        self.f = np.ascontiguousarray(f, np.uint8)
        self.n = len(self.type)
        self.process = None if process is None else np.ascontiguousarray(process, np.int64)  # None: every row is process 0
        self.key = None if key is None else np.ascontiguousarray(key, np.int64)
        self.value = np.ascontiguousarray(value, np.int64)
        self.index = None if index is None else np.ascontiguousarray(index, np.int64)

    @classmethod
    def from_ops(cls, ops: Sequence[dict]) -> "CounterHistory":
        """Op maps ({"type", "f", "value", "process", "index"}; independent
        tuples as lincheck.independent.tuple) to columns, by the rules of
        lc_edn_read_counter: a :process that is no integer is LC_NO_PROCESS, a
        value that is no 64-bit integer is LC_NIL."""
        n = len(ops)
        type_, f = np.zeros(n, np.uint8), np.full(n, N.LC_CF_OTHER, np.uint8)
        process, key = np.full(n, N.LC_NO_PROCESS, np.int64), np.full(n, N.LC_NO_KEY, np.int64)
        value, index = np.full(n, N.LC_NIL, np.int64), np.full(n, -1, np.int64)
        for r, op in enumerate(ops):
            type_[r] = TYPES[_name(op["type"])]
            fn = _name(op.get("f"))
            if _is_int(op.get("process")):
                process[r] = int(op["process"])
            if op.get("index") is not None:
                index[r] = int(op["index"])
            if fn in ("add", "read"):
                f[r] = N.LC_CF_ADD if fn == "add" else N.LC_CF_READ
                v = op.get("value")
                if is_tuple(v):
                    k, v = v[0], v[1]
                    if _elem(k) == N.LC_NIL:
                        raise ValueError(f"op {r}: tuple key is not an integer")
                    key[r] = int(k)
                value[r] = _elem(v)
        return cls(type_, f, process, key, value, index)

    @classmethod
    def read_edn(cls, path: str) -> "CounterHistory":
        """lc_edn_read_counter: a counter run's history.edn."""
        h = C.c_void_p()
        N.check(N.lib().lc_edn_read_counter(str(path).encode(), C.byref(h)))
        try:
            return cls._from_handle(h)
        finally:
            N.lib().lc_counter_hist_free(h)

    @classmethod
    def parse_edn(cls, text: str) -> "CounterHistory":
        data = text.encode()
        h = C.c_void_p()
        N.check(N.lib().lc_edn_parse_counter(data, len(data), C.byref(h)))
        try:
            return cls._from_handle(h)
        finally:
            N.lib().lc_counter_hist_free(h)

    @classmethod
    def _from_handle(cls, h) -> "CounterHistory":
        v = N.LcCounterHistory()
        N.check(N.lib().lc_counter_hist_view(h, C.byref(v)))
        n = int(v.n)
        return cls(N.carray(v.type, n, np.uint8), N.carray(v.f, n, np.uint8), N.carray(v.process, n, np.int64),
                   N.carray(v.key, n, np.int64), N.carray(v.value, n, np.int64), N.carray(v.index, n, np.int64))

    def as_c(self) -> N.LcCounterHistory:
        null64 = C.POINTER(C.c_int64)()
        return N.LcCounterHistory(self.n, N.ptr(self.type, C.c_uint8), N.ptr(self.f, C.c_uint8),
                                  null64 if self.process is None else N.ptr(self.process, C.c_int64),
                                  null64 if self.key is None else N.ptr(self.key, C.c_int64), N.ptr(self.value, C.c_int64),
                                  null64 if self.index is None else N.ptr(self.index, C.c_int64))

    def op_at(self, r: int, unwrap: bool = True) -> dict:
        """Row r as an op map: its own :index where it has one, else its
        position; the value of a keyed op unwrapped (a key's sub-history)."""
        fn = F_NAMES[int(self.f[r])]
        v: Any = None if fn == "other" or self.value[r] == N.LC_NIL else int(self.value[r])
        if not unwrap and fn != "other" and self.key is not None and self.key[r] != N.LC_NO_KEY:
            v = Tuple(int(self.key[r]), v)
        idx = r if self.index is None or self.index[r] < 0 else int(self.index[r])
        return {"type": TYPE_NAMES[int(self.type[r])], "f": fn, "value": v,
                "process": 0 if self.process is None else "nemesis" if self.process[r] == N.LC_NO_PROCESS else int(self.process[r]),
                "index": idx}

    def to_ops(self) -> List[dict]:
        """The rows as op maps again (tests; small histories)."""
        return [self.op_at(r, unwrap=False) for r in range(self.n)]


def synth_counter(n_keys: int = 1, ops_per_key: int = 1000, concurrency: int = 5, info_rate: float = 0.0,
                  fail_rate: float = 0.0, stale_rate: float = 0.0, seed: int = 1) -> CounterHistory:
    """A synthetic counter history (tests and timing only).  Per key the ops
    run in rounds: each of `concurrency` processes invokes an op -- an add of
    1..5 or a read, half each -- then all complete in a random order.  An add
    completes :ok, :info at info_rate or :fail at fail_rate; a read completes
    :ok, or :fail at fail_rate.  An :ok read returns the acknowledged sum at
    its completion, which is in bounds, except a stale_rate share that returns
    one less than the acknowledged sum at its invocation, which is not.  Keys
    are laid out one after the other; several keys make tuple values.  Built
    with numpy, no op maps."""
    rng = np.random.default_rng(seed)
    c = max(1, int(concurrency))
    rounds = max(1, -(-int(ops_per_key) // c))
    cols = dict(type=[], f=[], process=[], key=[], value=[])
    for k in range(n_keys):
        shape = (rounds, c)
        is_add = rng.random(shape) < 0.5
        amount = rng.integers(1, 6, shape).astype(np.int64)
        u = rng.random(shape)
        comp = np.where(u < fail_rate, N.LC_FAIL, np.where(is_add & (u < fail_rate + info_rate), N.LC_INFO, N.LC_OK_T))
        stale = ~is_add & (comp == N.LC_OK_T) & (rng.random(shape) < stale_rate)
        order = np.argsort(rng.random(shape), axis=1)  # order[r, j]: the process that completes j-th in round r
        slot = np.empty(shape, np.int64)
        np.put_along_axis(slot, order, np.broadcast_to(np.arange(c), shape), axis=1)
        base = np.arange(rounds, dtype=np.int64)[:, None] * (2 * c)
        inv_row = base + np.arange(c)[None, :]
        comp_row = base + c + slot
        n_rows = rounds * 2 * c
        t = np.zeros(n_rows, np.uint8)
        f = np.zeros(n_rows, np.uint8)
        p = np.zeros(n_rows, np.int64)
        v = np.full(n_rows, N.LC_NIL, np.int64)
        t[inv_row], t[comp_row] = N.LC_INVOKE, comp
        f[inv_row] = f[comp_row] = np.where(is_add, N.LC_CF_ADD, N.LC_CF_READ)
        p[inv_row] = p[comp_row] = np.broadcast_to(np.arange(c), shape)
        v[inv_row[is_add]] = v[comp_row[is_add]] = amount[is_add]
        live = np.arange(rounds * c).reshape(shape) < ops_per_key  # the first ops_per_key ops, by invocation
        low = np.zeros(n_rows, np.int64)
        ok_add = is_add & (comp == N.LC_OK_T) & live
        low[comp_row[ok_add]] = amount[ok_add]
        lower = np.cumsum(low)
        ok_read = ~is_add & (comp == N.LC_OK_T)
        v[comp_row[ok_read]] = np.where(stale, lower[inv_row] - 1, lower[comp_row])[ok_read]
        keep = np.zeros(n_rows, bool)
        keep[inv_row[live]] = keep[comp_row[live]] = True
        cols["type"].append(t[keep]); cols["f"].append(f[keep]); cols["process"].append(p[keep]); cols["value"].append(v[keep])
        cols["key"].append(np.full(int(keep.sum()), k, np.int64))
    cat = {name: np.concatenate(a) for name, a in cols.items()}
    return CounterHistory(cat["type"], cat["f"], cat["process"], cat["key"] if n_keys > 1 else None, cat["value"], None)


BATCH_ARRAYS = (("ev_off", np.uint64), ("ev_kind", np.uint8), ("ev_val", np.int64), ("read_off", np.uint64),
                ("read_val", np.int64), ("status", np.uint8))
_CTYPES = {np.uint64: C.c_uint64, np.int64: C.c_int64, np.uint8: C.c_uint8}


class PackedCounter:
    """lc_counter_pack output: the per-key event lists lc_counter_check reads."""

    def __init__(self, hist: CounterHistory):
        self.hist = hist
        self._c = hist.as_c()
        h = C.c_void_p()
        N.check(N.lib().lc_counter_pack(C.byref(self._c), C.byref(h)))
        self.handle = h
        v = N.LcCounterBatch()
        N.check(N.lib().lc_counter_packed_view(h, C.byref(v)))
        self.view = v
        self.n_keys = int(v.n_keys)
        keys = np.zeros(max(self.n_keys, 1), np.int64)
        N.check(N.lib().lc_counter_packed_keys(h, N.ptr(keys, C.c_int64)))
        self.keys = [None if k == N.LC_NO_KEY else int(k) for k in keys[:self.n_keys]]
        self.status = N.carray(v.status, self.n_keys, np.uint8)
        self.read_off = N.carray(v.read_off, self.n_keys + 1, np.uint64).astype(np.int64)
        self.n_events = int(v.ev_off[self.n_keys]) if self.n_keys else 0
        self.n_reads = int(self.read_off[-1]) if self.n_keys else 0
        self._read_val: Optional[np.ndarray] = None

    def __del__(self):
        h = getattr(self, "handle", None)
        if h:
            N.lib().lc_counter_packed_free(h)
            self.handle = None

    def key_error(self, i: int) -> Optional[str]:
        msg = N.lib().lc_counter_packed_key_error(self.handle, i)
        return None if msg is None else msg.decode(errors="replace")

    def read_val(self) -> np.ndarray:
        if self._read_val is None:
            self._read_val = N.carray(self.view.read_val, self.n_reads, np.int64)
        return self._read_val

    def arrays(self) -> Dict[str, np.ndarray]:
        """Copies of every array of the view (tests, caller-built batches)."""
        v, K = self.view, self.n_keys
        sizes = dict(ev_off=K + 1, ev_kind=self.n_events, ev_val=self.n_events, read_off=K + 1, read_val=self.n_reads, status=K)
        return {name: N.carray(getattr(v, name), sizes[name], dt) for name, dt in BATCH_ARRAYS}


def batch_of(arrs: Dict[str, Any]) -> N.LcCounterBatch:
    """An lc_counter_batch over numpy arrays (PackedCounter.arrays(), or a
    caller's own).  The arrays must outlive the call that reads the batch."""
    pad = {}
    for name, dt in BATCH_ARRAYS:
        a = np.ascontiguousarray(arrs[name], dt)
        pad[name] = a if len(a) else np.zeros(1, dt)
    arrs["_keep"] = pad
    return N.LcCounterBatch(len(arrs["status"]), *[N.ptr(pad[name], _CTYPES[dt]) for name, dt in BATCH_ARRAYS])


@dataclass
class CounterResults:
    valid: np.ndarray     # int8 [K]: 1 / 0 / -1
    n_errors: np.ndarray  # uint64 [K]
    lower: np.ndarray     # int64 [R]
    upper: np.ndarray     # int64 [R]
    err_off: np.ndarray   # uint64 [K + 1]
    err_idx: np.ndarray   # uint64 [n_err] read indices of the batch, ascending
    timing: Dict[str, float]
    retried: bool = False  # the first err_cap was too small


def check_batch(dev, batch: N.LcCounterBatch, tile: int = 0, err_cap: Optional[int] = None, host: bool = False) -> CounterResults:
    """lc_counter_check on a checker.Device (host: lc_counter_check_host, dev
    unused).  err_cap: the first capacity of err_idx; when the batch has more
    reads out of bounds the call says how many and is made once more."""
    K = int(batch.n_keys)
    R = int(batch.read_off[K]) if K else 0
    valid, n_errors = np.zeros(max(K, 1), np.int8), np.zeros(max(K, 1), np.uint64)
    lower, upper = np.zeros(max(R, 1), np.int64), np.zeros(max(R, 1), np.int64)
    err_off = np.zeros(K + 1, np.uint64)
    cap = min(R, FIRST_ERR_CAP) if err_cap is None else int(err_cap)
    o = N.LcCounterOpts(int(tile), 0)
    retried = False
    while True:
        err_idx = np.zeros(max(cap, 1), np.uint64)
        r = N.LcCounterResult(N.ptr(valid, C.c_int8), N.ptr(n_errors, C.c_uint64), N.ptr(lower, C.c_int64),
                              N.ptr(upper, C.c_int64), N.ptr(err_off, C.c_uint64), N.ptr(err_idx, C.c_uint64), cap, 0)
        if host:
            rc = N.lib().lc_counter_check_host(C.byref(batch), C.byref(r))
        else:
            rc = N.lib().lc_counter_check(dev.handle, C.byref(batch), C.byref(o), C.byref(r))
        if rc == -2 and int(r.n_err) > cap and not retried:  # LC_E_NOMEM: err_idx was too small
            cap, retried = int(r.n_err), True
            continue
        N.check(rc)
        break
    ms = (C.c_double * 4)()
    if not host:
        N.check(N.lib().lc_counter_last_timing(dev.handle, ms))
    return CounterResults(valid[:K], n_errors[:K], lower[:R], upper[:R], err_off, err_idx[:int(r.n_err)],
                          dict(upload_ms=ms[0], kernel_ms=ms[1], download_ms=ms[2], total_ms=ms[3]), retried)


class CheckedCounter:
    """lc_counter_check_history output: a history packed and checked on the
    device.  It stands where a PackedCounter stands in result_map, and `res`
    is the CounterResults of the same call."""

    def __init__(self, dev, hist: CounterHistory, tile: int = 0):
        self.hist = hist
        self.dev = dev
        self._c = hist.as_c()
        h = C.c_void_p()
        o = N.LcCounterOpts(int(tile), 0)
        N.check(N.lib().lc_counter_check_history(dev.handle, C.byref(self._c), C.byref(o), C.byref(h)))
        self.handle = h
        v, r = N.LcCounterBatch(), N.LcCounterResult()
        N.check(N.lib().lc_counter_checked_view(h, C.byref(v), C.byref(r)))
        K = self.n_keys = int(v.n_keys)
        keys = np.zeros(max(K, 1), np.int64)
        N.check(N.lib().lc_counter_checked_keys(h, N.ptr(keys, C.c_int64)))
        self.keys = [None if k == N.LC_NO_KEY else int(k) for k in keys[:K]]
        self.status = N.carray(v.status, K, np.uint8)
        self.ev_off = N.carray(v.ev_off, K + 1, np.uint64)
        self.read_off = N.carray(v.read_off, K + 1, np.uint64).astype(np.int64)
        self.n_events = int(self.ev_off[-1])
        R = self.n_reads = int(self.read_off[-1])
        self._read_val = np.zeros(max(R, 1), np.int64)
        N.check(N.lib().lc_counter_checked_read_vals(h, N.ptr(self._read_val, C.c_int64)))
        self._read_val = self._read_val[:R]
        ms = (C.c_double * 6)()
        N.check(N.lib().lc_counter_history_timing(dev.handle, ms))
        names = ("upload_ms", "group_ms", "build_ms", "kernel_ms", "download_ms", "total_ms")
        self.res = CounterResults(N.carray(r.valid, K, np.int8), N.carray(r.n_errors, K, np.uint64), N.carray(r.lower, R, np.int64),
                                  N.carray(r.upper, R, np.int64), N.carray(r.err_off, K + 1, np.uint64),
                                  N.carray(r.err_idx, int(r.n_err), np.uint64), dict(zip(names, ms)))

    def __del__(self):
        h = getattr(self, "handle", None)
        if h:
            N.lib().lc_counter_checked_free(h)
            self.handle = None

    def key_error(self, i: int) -> Optional[str]:
        msg = N.lib().lc_counter_checked_key_error(self.handle, i)
        return None if msg is None else msg.decode(errors="replace")

    def key_error_row(self, i: int) -> int:
        return int(N.lib().lc_counter_checked_key_error_row(self.handle, i))

    def read_val(self) -> np.ndarray:
        return self._read_val

    def arrays(self) -> Dict[str, np.ndarray]:
        """The batch the device built, downloaded (lc_counter_checked_batch):
        PackedCounter.arrays()'s names.  Only for the device's latest check."""
        v, K = N.LcCounterBatch(), self.n_keys
        N.check(N.lib().lc_counter_checked_batch(self.dev.handle, self.handle, C.byref(v)))
        sizes = dict(ev_off=K + 1, ev_kind=self.n_events, ev_val=self.n_events, read_off=K + 1, read_val=self.n_reads, status=K)
        return {name: N.carray(getattr(v, name), sizes[name], dt) for name, dt in BATCH_ARRAYS}


def result_map(packed, res: CounterResults, i: int) -> Dict:
    """jepsen.checker/counter's result map of packed key i."""
    if packed.status[i] != N.LC_COUNTER_KEY_OK:
        return {"valid?": "unknown", "error": packed.key_error(i) or "error"}
    b, e = int(packed.read_off[i]), int(packed.read_off[i + 1])
    val = packed.read_val()
    triples = np.stack([res.lower[b:e], val[b:e], res.upper[b:e]], axis=1) if e > b else np.zeros((0, 3), np.int64)
    bad = res.err_idx[int(res.err_off[i]):int(res.err_off[i + 1])].astype(np.int64) - b
    return {"valid?": int(res.valid[i]) == N.LC_VALID, "reads": triples.tolist(), "errors": triples[bad].tolist()}


class CounterChecker:
    """jepsen.checker/counter on the device."""

    def __init__(self, opts: Optional[Dict] = None):
        opts = opts or {}
        self.device = int(opts.get("device", 0))
        self.tile = int(opts.get("tile", 0))
        self.host = bool(opts.get("host", False))  # lc_counter_check_host: no device
        self.err_cap = opts.get("err-cap")         # tests: the first err_idx capacity
        self.pack = opts.get("pack", "host")       # "device": lc_counter_check_history packs on the device
        if self.pack not in ("host", "device"):
            raise ValueError(f'counter: "pack" is "host" or "device", not {self.pack!r}')
        if self.pack == "device" and self.host:
            raise ValueError('counter: {"pack": "device"} runs on the device; it cannot go with {"host": True}')

    def dev(self):
        if self.host:
            return None
        from . import checker as ck
        return ck.device_for(self.device)

    def stream(self, dev=None):
        """A streaming check by this checker's rules
        (lincheck.counter_stream.CounterStream): rows are appended while the
        test runs, and after every append the results are those of check() on
        everything appended so far.  {"host": True} or no device: the host
        stream."""
        from .counter_stream import CounterStream
        return CounterStream(None if self.host else dev, {"tile": self.tile, "err-cap": self.err_cap})

    def _check(self, history):
        hist = history if isinstance(history, CounterHistory) else CounterHistory.from_ops(history)
        if self.pack == "device":
            checked = CheckedCounter(self.dev(), hist, self.tile)
            return checked, checked.res
        packed = PackedCounter(hist)
        return packed, check_batch(self.dev(), packed.view, self.tile, self.err_cap, self.host)

    def check(self, test: Optional[Dict], history, opts: Optional[Dict] = None) -> Dict:
        """One (unwrapped) history: rows without a key are one counter; of a
        keyed history, the first key's."""
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
                    ops = history.to_ops() if isinstance(history, CounterHistory) else history
                r[name] = ck.check_safe(ch, test, subhistory(ops, k), dict(opts or {}, **{"history-key": k}))
            r["valid?"] = ck.merge_valid([x.get("valid?") for x in r.values()])
            results[k] = r
        return merge_results(results)


def counter(opts: Optional[Dict] = None) -> CounterChecker:
    return CounterChecker(opts)
