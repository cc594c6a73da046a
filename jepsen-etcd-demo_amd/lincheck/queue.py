"""Mirrors of jepsen.checker/total-queue and jepsen.checker/unique-ids.

    checker.total_queue()
        (checker/total-queue) on the device: what goes into a queue must come
        out.  Per key three multisets -- the enqueues attempted, the enqueues
        acknowledged, the dequeues (an :ok :drain's elements included) -- and
        every distinct value classified from its three counts
        (include/lincheck_queue.h has the rules; this library's reading of the
        public Jepsen 0.2.x source, parity unpinned).  Result map, Jepsen's
        keys as strings: {"valid?", "attempt-count", "acknowledged-count",
        "ok-count", "unexpected-count", "duplicated-count", "lost-count",
        "recovered-count", "lost", "unexpected", "duplicated", "recovered"
        (sorted lists with repeats, nil first)}; a key with a crashed drain is
        {"valid?": "unknown", "error": ...}.
    checker.unique_ids()
        (checker/unique-ids): {"valid?", "attempted-count",
        "acknowledged-count", "duplicated-count", "duplicated" ({value: count}
        of the 48 most frequent duplicates), "range" ([min, max])}.

The path is its own: QueueHistory (lc_queue_history) -> PackedQueue
(lc_queue_pack) -> lc_queue_check -> result maps.  The device tallies every
(key, value) in a hash table and returns the per-key counts and one entry per
anomalous value.  Under independent.checker every key is checked in one
lc_queue_check call.  {"host": True} runs lc_queue_check_host instead: the same
fold in plain C++ on one thread, no device (tests, and the timing's baseline).
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence

import numpy as np

from . import _native as N
from .independent import Tuple, is_tuple
from .setcheck import I64_MAX, TYPE_NAMES, TYPES, _name

F_CODES = {"enqueue": N.LC_QF_ENQUEUE, "dequeue": N.LC_QF_DEQUEUE, "drain": N.LC_QF_DRAIN, "generate": N.LC_QF_GENERATE}
F_NAMES = {v: k for k, v in F_CODES.items()}
F_NAMES[N.LC_QF_OTHER] = "other"
FIRST_ENT_CAP = 1024  # check_batch's first entry capacity; a batch with more is checked once more
TOP_DUPLICATES = 48   # unique-ids' "duplicated" holds this many
COUNT_NAMES = ("attempt-count", "acknowledged-count", "ok-count", "unexpected-count", "duplicated-count", "lost-count",
               "recovered-count")
CLASS_NAMES = ("lost", "unexpected", "duplicated", "recovered")  # in the order of N.LC_QC_*


def _value(v, what: str) -> int:
    """An integer or nil as the C ABI holds it; anything else is refused, as
    lc_edn_read_queue refuses it."""
    if v is None:
        return N.LC_NIL
    if isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) and -I64_MAX <= int(v) <= I64_MAX:
        return int(v)
    raise ValueError(f"{what}: a value that is neither a 64-bit integer nor nil: {v!r}")


def _unsupported(call, *args):
    rc = call(*args)
    if rc == -5:  # LC_E_UNSUPPORTED
        raise ValueError(N.lib().lc_last_error().decode(errors="replace"))
    N.check(rc)


class QueueHistory:
    """A raw queue or id-generator history as columns (lc_queue_history)."""

    def __init__(self, type_, f, key, value, drain_off=None, drain_val=None):
        self.type = np.ascontiguousarray(type_, np.uint8)
        self.f = np.ascontiguousarray(f, np.uint8)
        self.n = len(self.type)
        self.key = None if key is None else np.ascontiguousarray(key, np.int64)
        self.value = np.ascontiguousarray(value, np.int64)
        self.drain_off = None if drain_off is None else np.ascontiguousarray(drain_off, np.uint64)
        self.drain_val = np.ascontiguousarray(drain_val if drain_val is not None else [], np.int64)
        if len(self.drain_val) == 0:
            self.drain_val = np.zeros(1, np.int64)[:0]

    @classmethod
    def from_ops(cls, ops: Sequence[dict]) -> "QueueHistory":
        """Op maps ({"type", "f", "value"}; independent tuples as
        lincheck.independent.tuple; a drain's value a list) to columns, by the
        rules of lc_edn_read_queue."""
        n = len(ops)
        type_, f = np.zeros(n, np.uint8), np.full(n, N.LC_QF_OTHER, np.uint8)
        key, value = np.full(n, N.LC_NO_KEY, np.int64), np.full(n, N.LC_NIL, np.int64)
        drain_off, drain_val = np.zeros(n + 1, np.uint64), []
        for r, op in enumerate(ops):
            type_[r] = TYPES[_name(op["type"])]
            code = F_CODES.get(_name(op.get("f")))
            if code is not None:
                f[r] = code
                v = op.get("value")
                if is_tuple(v):
                    k, v = v[0], v[1]
                    if k is None:
                        raise ValueError(f"op {r}: tuple key is not an integer")
                    key[r] = _value(k, f"op {r}: tuple key")
                if code == N.LC_QF_DRAIN:
                    if v is not None:
                        if not isinstance(v, (list, tuple)) or is_tuple(v):
                            raise ValueError(f"op {r}: a :drain's value is neither nil nor a vector of integers: {v!r}")
                        drain_val.extend(_value(e, f"op {r}") for e in v)
                else:
                    value[r] = _value(v, f"op {r}")
            drain_off[r + 1] = len(drain_val)
        return cls(type_, f, key, value, drain_off, drain_val)

    @classmethod
    def read_edn(cls, path: str) -> "QueueHistory":
        """lc_edn_read_queue: a queue or id-generator run's history.edn."""
        h = C.c_void_p()
        _unsupported(N.lib().lc_edn_read_queue, str(path).encode(), C.byref(h))
        try:
            return cls._from_handle(h)
        finally:
            N.lib().lc_queue_hist_free(h)

    @classmethod
    def parse_edn(cls, text: str) -> "QueueHistory":
        data = text.encode()
        h = C.c_void_p()
        _unsupported(N.lib().lc_edn_parse_queue, data, len(data), C.byref(h))
        try:
            return cls._from_handle(h)
        finally:
            N.lib().lc_queue_hist_free(h)

    @classmethod
    def _from_handle(cls, h) -> "QueueHistory":
        v = N.LcQueueHistory()
        N.check(N.lib().lc_queue_hist_view(h, C.byref(v)))
        n = int(v.n)
        off = N.carray(v.drain_off, n + 1, np.uint64)
        return cls(N.carray(v.type, n, np.uint8), N.carray(v.f, n, np.uint8), N.carray(v.key, n, np.int64),
                   N.carray(v.value, n, np.int64), off, N.carray(v.drain_val, int(off[-1]), np.int64))

    def as_c(self) -> N.LcQueueHistory:
        return N.LcQueueHistory(self.n, N.ptr(self.type, C.c_uint8), N.ptr(self.f, C.c_uint8),
                                C.POINTER(C.c_int64)() if self.key is None else N.ptr(self.key, C.c_int64),
                                N.ptr(self.value, C.c_int64),
                                C.POINTER(C.c_uint64)() if self.drain_off is None else N.ptr(self.drain_off, C.c_uint64),
                                N.ptr(self.drain_val, C.c_int64) if len(self.drain_val) else C.POINTER(C.c_int64)())

    def op_at(self, r: int, unwrap: bool = True) -> dict:
        """Row r as an op map; the value of a keyed op unwrapped (a key's
        sub-history) unless unwrap is False."""
        code = int(self.f[r])
        fn = F_NAMES[code]
        v: Any = None
        if code == N.LC_QF_DRAIN:
            if int(self.type[r]) == N.LC_OK_T:
                b, e = (int(self.drain_off[r]), int(self.drain_off[r + 1])) if self.drain_off is not None else (0, 0)
                v = [None if x == N.LC_NIL else int(x) for x in self.drain_val[b:e]]
        elif code != N.LC_QF_OTHER and self.value[r] != N.LC_NIL:
            v = int(self.value[r])
        if not unwrap and code != N.LC_QF_OTHER and self.key is not None and self.key[r] != N.LC_NO_KEY:
            v = Tuple(int(self.key[r]), v)
        return {"type": TYPE_NAMES[int(self.type[r])], "f": fn, "value": v, "process": 0, "index": r}

    def to_ops(self) -> List[dict]:
        """The rows as op maps again (tests; small histories)."""
        return [self.op_at(r, unwrap=False) for r in range(self.n)]


def _pairs(f, first, second, values):
    """Two rows per value: (first, f, v) then (second[i], f, v)."""
    n = len(values)
    t = np.empty(2 * n, np.uint8)
    t[0::2], t[1::2] = first, second
    return t, np.full(2 * n, f, np.uint8), np.repeat(np.asarray(values, np.int64), 2)


def synth_queue(n_keys: int = 1, n_values: int = 1000, lost: int = 0, duplicated: int = 0, unexpected: int = 0,
                recovered: int = 0, drain: int = 0, seed: int = 1) -> QueueHistory:
    """A synthetic queue history (tests and timing only).  Per key the values
    0 .. n_values - 1 are each enqueued (:invoke then :ok) and then dequeued
    once (:invoke then :ok, in a shuffled order), except that `lost` of them
    are never dequeued, `duplicated` others are dequeued twice, `recovered`
    others have an enqueue that completes :info, and `unexpected` values from
    n_values up are dequeued without ever being enqueued.  The last `drain`
    dequeues of a key come as one :ok :drain instead.  Keys are laid out one
    after the other; several keys make tuple values.  Built with numpy, no op
    maps."""
    rng = np.random.default_rng(seed)
    n = int(n_values)
    assert lost + duplicated + recovered <= n
    cols = dict(type=[], f=[], key=[], value=[], dn=[], dv=[])
    for k in range(n_keys):
        perm = rng.permutation(n)
        done = np.full(n, N.LC_OK_T, np.uint8)
        done[perm[lost + duplicated:lost + duplicated + recovered]] = N.LC_INFO
        deq = np.concatenate([perm[lost:], perm[lost:lost + duplicated], np.arange(n, n + unexpected)]).astype(np.int64)
        rng.shuffle(deq)
        nd = min(int(drain), len(deq))
        single = deq[:len(deq) - nd]
        t1, f1, v1 = _pairs(N.LC_QF_ENQUEUE, N.LC_INVOKE, done, np.arange(n))
        t2, f2, v2 = _pairs(N.LC_QF_DEQUEUE, N.LC_INVOKE, N.LC_OK_T, single)
        v2[0::2] = N.LC_NIL  # a dequeue's invocation has no value
        t, f, v = [t1, t2], [f1, f2], [v1, v2]
        dn = [np.zeros(len(t1) + len(t2), np.uint64)]
        if nd:
            t.append(np.array([N.LC_INVOKE, N.LC_OK_T], np.uint8))
            f.append(np.full(2, N.LC_QF_DRAIN, np.uint8))
            v.append(np.full(2, N.LC_NIL, np.int64))
            dn.append(np.array([0, nd], np.uint64))
            cols["dv"].append(deq[len(deq) - nd:])
        rows = sum(len(x) for x in t)
        cols["type"] += t; cols["f"] += f; cols["value"] += v; cols["dn"] += dn
        cols["key"].append(np.full(rows, k, np.int64))
    cat = {name: np.concatenate(a) if a else np.zeros(0, np.int64) for name, a in cols.items()}
    off = np.zeros(len(cat["type"]) + 1, np.uint64)
    np.cumsum(cat["dn"], out=off[1:])
    return QueueHistory(cat["type"], cat["f"], cat["key"] if n_keys > 1 else None, cat["value"], off, cat["dv"])


def synth_ids(n_keys: int = 1, n_values: int = 1000, dup_rate: float = 0.0, seed: int = 1) -> QueueHistory:
    """A synthetic id-generator history (tests and timing only): per key
    n_values :generate ops (:invoke then :ok) that return 0 .. n_values - 1 in
    a shuffled order, except a dup_rate share that return an id drawn at random
    from that range again."""
    rng = np.random.default_rng(seed)
    n = int(n_values)
    cols = dict(type=[], f=[], key=[], value=[])
    for k in range(n_keys):
        ids = rng.permutation(n).astype(np.int64)
        again = rng.random(n) < dup_rate
        ids[again] = rng.integers(0, max(n, 1), int(again.sum()))
        t, f, v = _pairs(N.LC_QF_GENERATE, N.LC_INVOKE, N.LC_OK_T, ids)
        v[0::2] = N.LC_NIL
        cols["type"].append(t); cols["f"].append(f); cols["value"].append(v)
        cols["key"].append(np.full(2 * n, k, np.int64))
    cat = {name: np.concatenate(a) for name, a in cols.items()}
    return QueueHistory(cat["type"], cat["f"], cat["key"] if n_keys > 1 else None, cat["value"])


BATCH_ARRAYS = (("row_key", np.uint32), ("row_kind", np.uint8), ("row_val", np.int64), ("status", np.uint8),
                ("attempted", np.uint64))
_CTYPES = {np.uint64: C.c_uint64, np.int64: C.c_int64, np.uint8: C.c_uint8, np.uint32: C.c_uint32}


class PackedQueue:
    """lc_queue_pack output: one row per value that counts, with its dense key id."""

    def __init__(self, hist: QueueHistory, mode: int):
        self.hist = hist
        self.mode = int(mode)
        self._c = hist.as_c()
        h = C.c_void_p()
        N.check(N.lib().lc_queue_pack(C.byref(self._c), self.mode, C.byref(h)))
        self.handle = h
        v = N.LcQueueBatch()
        N.check(N.lib().lc_queue_packed_view(h, C.byref(v)))
        self.view = v
        self.n_keys, self.n_rows = int(v.n_keys), int(v.n_rows)
        keys = np.zeros(max(self.n_keys, 1), np.int64)
        N.check(N.lib().lc_queue_packed_keys(h, N.ptr(keys, C.c_int64)))
        self.keys = [None if k == N.LC_NO_KEY else int(k) for k in keys[:self.n_keys]]
        self.status = N.carray(v.status, self.n_keys, np.uint8)

    def __del__(self):
        h = getattr(self, "handle", None)
        if h:
            N.lib().lc_queue_packed_free(h)
            self.handle = None

    def key_error(self, i: int) -> Optional[str]:
        msg = N.lib().lc_queue_packed_key_error(self.handle, i)
        return None if msg is None else msg.decode(errors="replace")

    def arrays(self) -> Dict[str, np.ndarray]:
        """Copies of every array of the view (tests, caller-built batches)."""
        v, K, n = self.view, self.n_keys, self.n_rows
        sizes = dict(row_key=n, row_kind=n, row_val=n, status=K, attempted=K)
        return {name: N.carray(getattr(v, name), sizes[name], dt) for name, dt in BATCH_ARRAYS}


def batch_of(arrs: Dict[str, Any], mode: int) -> N.LcQueueBatch:
    """An lc_queue_batch over numpy arrays (PackedQueue.arrays(), or a caller's
    own; "attempted" may be missing).  The arrays must outlive the call that
    reads the batch."""
    K = len(arrs["status"])
    pad = {}
    for name, dt in BATCH_ARRAYS:
        a = np.ascontiguousarray(arrs.get(name, np.zeros(K, dt)), dt)
        pad[name] = a if len(a) else np.zeros(1, dt)
    arrs["_keep"] = pad
    return N.LcQueueBatch(K, len(arrs["row_key"]), int(mode), 0, *[N.ptr(pad[name], _CTYPES[dt]) for name, dt in BATCH_ARRAYS])


@dataclass
class QueueResults:
    valid: np.ndarray      # int8 [K]: 1 / 0 / -1
    counts: np.ndarray     # uint64 [K, 7]
    lo: np.ndarray         # int64 [K], meaningful where has_range
    hi: np.ndarray
    has_range: np.ndarray  # uint8 [K]
    ent_key: np.ndarray    # uint32 [n_ent], sorted by (key, class, value)
    ent_class: np.ndarray  # uint8
    ent_val: np.ndarray    # int64
    ent_mult: np.ndarray   # uint64
    timing: Dict[str, float]
    retried: bool = False  # the first ent_cap was too small


def check_batch(dev, batch: N.LcQueueBatch, slots: int = 0, ent_cap: Optional[int] = None, host: bool = False) -> QueueResults:
    """lc_queue_check on a checker.Device (host: lc_queue_check_host, dev
    unused).  ent_cap: the first capacity of the entry arrays; when the batch
    has more entries the call says how many and is made once more."""
    K, n = int(batch.n_keys), int(batch.n_rows)
    valid, counts = np.zeros(max(K, 1), np.int8), np.zeros((max(K, 1), N.LC_QN_COUNTS), np.uint64)
    lo, hi, has = np.zeros(max(K, 1), np.int64), np.zeros(max(K, 1), np.int64), np.zeros(max(K, 1), np.uint8)
    cap = min(2 * n, FIRST_ENT_CAP) if ent_cap is None else int(ent_cap)
    o = N.LcQueueOpts(int(slots), 0)
    retried = False
    while True:
        m = max(cap, 1)
        ek, ec, ev, em = np.zeros(m, np.uint32), np.zeros(m, np.uint8), np.zeros(m, np.int64), np.zeros(m, np.uint64)
        r = N.LcQueueResult(N.ptr(valid, C.c_int8), N.ptr(counts, C.c_uint64), N.ptr(lo, C.c_int64), N.ptr(hi, C.c_int64),
                            N.ptr(has, C.c_uint8), N.ptr(ek, C.c_uint32), N.ptr(ec, C.c_uint8), N.ptr(ev, C.c_int64),
                            N.ptr(em, C.c_uint64), cap, 0)
        if host:
            rc = N.lib().lc_queue_check_host(C.byref(batch), C.byref(r))
        else:
            rc = N.lib().lc_queue_check(dev.handle, C.byref(batch), C.byref(o), C.byref(r))
        if rc == -2 and int(r.n_ent) > cap and not retried:  # LC_E_NOMEM: the entry arrays were too small
            cap, retried = int(r.n_ent), True
            continue
        N.check(rc)
        break
    ms = (C.c_double * 4)()
    if not host:
        N.check(N.lib().lc_queue_last_timing(dev.handle, ms))
    ne = int(r.n_ent)
    return QueueResults(valid[:K], counts[:K], lo[:K], hi[:K], has[:K], ek[:ne], ec[:ne], ev[:ne], em[:ne],
                        dict(upload_ms=ms[0], kernel_ms=ms[1], download_ms=ms[2], total_ms=ms[3]), retried)


def _nil(v: int):
    return None if v == N.LC_NIL else int(v)


def result_map(packed: PackedQueue, res: QueueResults, i: int) -> Dict:
    """The checker's result map of packed key i."""
    if packed.status[i] != N.LC_QUEUE_KEY_OK:
        return {"valid?": "unknown", "error": packed.key_error(i) or "error"}
    b, e = np.searchsorted(res.ent_key, [i, i + 1])
    cls, val, mult = res.ent_class[b:e], res.ent_val[b:e], res.ent_mult[b:e]
    c = res.counts[i]
    out: Dict[str, Any] = {"valid?": int(res.valid[i]) == N.LC_VALID}
    if packed.mode == N.LC_QM_UNIQUE_IDS:
        out.update({"attempted-count": int(c[N.LC_QN_ATTEMPT]), "acknowledged-count": int(c[N.LC_QN_ACKNOWLEDGED]),
                    "duplicated-count": int(c[N.LC_QN_OK])})
        # sort-by val, reverse, take 48, into a sorted map: the highest counts, ties towards the larger value
        top = np.lexsort((val, mult))[::-1][:TOP_DUPLICATES]
        out["duplicated"] = {_nil(val[j]): int(mult[j]) for j in np.sort(top)}
        out["range"] = [_nil(res.lo[i]), _nil(res.hi[i])] if res.has_range[i] else [None, None]
        return out
    for j, name in enumerate(COUNT_NAMES):
        out[name] = int(c[j])
    for code, name in enumerate(CLASS_NAMES):
        pick = cls == code
        out[name] = [_nil(x) for x in np.repeat(val[pick], mult[pick].astype(np.int64))]
    return out


class _QueueChecker:
    """The shared shape of the two checkers: pack, one call, result maps."""

    mode = N.LC_QM_TOTAL_QUEUE

    def __init__(self, opts: Optional[Dict] = None):
        opts = opts or {}
        self.device = int(opts.get("device", 0))
        self.slots = int(opts.get("slots", 0))
        self.host = bool(opts.get("host", False))  # lc_queue_check_host: no device
        self.ent_cap = opts.get("ent-cap")         # tests: the first entry capacity

    def dev(self):
        if self.host:
            return None
        from . import checker as ck
        return ck.device_for(self.device)

    def stream(self, dev=None):
        """A streaming check by this checker's rules
        (lincheck.queue_stream.QueueStream): rows are appended while the test
        runs, and after every append the results are those of check() on
        everything appended so far.  {"host": True}: the host stream."""
        from .queue_stream import QueueStream
        opts = {"slots": self.slots, "ent-cap": self.ent_cap}
        return QueueStream(None if self.host else dev if dev is not None else self.dev(), self.mode, opts)

    def _check(self, history):
        hist = history if isinstance(history, QueueHistory) else QueueHistory.from_ops(history)
        packed = PackedQueue(hist, self.mode)
        return packed, check_batch(self.dev(), packed.view, self.slots, self.ent_cap, self.host)

    def check(self, test: Optional[Dict], history, opts: Optional[Dict] = None) -> Dict:
        """One (unwrapped) history: rows without a key are one queue; of a
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
                    ops = history.to_ops() if isinstance(history, QueueHistory) else history
                r[name] = ck.check_safe(ch, test, subhistory(ops, k), dict(opts or {}, **{"history-key": k}))
            r["valid?"] = ck.merge_valid([x.get("valid?") for x in r.values()])
            results[k] = r
        return merge_results(results)


class TotalQueueChecker(_QueueChecker):
    """jepsen.checker/total-queue on the device."""
    mode = N.LC_QM_TOTAL_QUEUE


class UniqueIdsChecker(_QueueChecker):
    """jepsen.checker/unique-ids on the device."""
    mode = N.LC_QM_UNIQUE_IDS


def total_queue(opts: Optional[Dict] = None) -> TotalQueueChecker:
    return TotalQueueChecker(opts)


def unique_ids(opts: Optional[Dict] = None) -> UniqueIdsChecker:
    return UniqueIdsChecker(opts)
