"""Mirror of jepsen.checker/set-full for the set workload with intermediate reads.

    checker.set_full({"linearizable?": True})
        (checker/set-full {:linearizable? true}) on the device: every :ok :read
        is examined and every element classified :stable, :lost or :never-read
        (include/lincheck.h has the rules; restated from memory of the public
        Jepsen 0.2.x source, parity unpinned).  Result map, Jepsen's keys as
        strings: {"valid?", "attempt-count", "stable-count", "lost-count",
        "never-read-count", "stale-count", "duplicated-count", "lost",
        "never-read", "stale" (ascending element vectors), "duplicated"
        ({element: largest multiplicity in one read}), "worst-stale",
        "stable-latencies", "lost-latencies" ({0, 0.5, 0.95, 0.99, 1: ms})}.

The path is its own: SetFullHistory (lc_setfull_history) -> PackedSetFull
(lc_setfull_pack) -> lc_setfull_check -> result maps.  The device returns
outcome, latency, known and last-absent per element; the order statistics
(quantiles, worst-stale) and the multiplicities of the elements the device
flagged as duplicated are computed here from those arrays.  Under
independent.checker every key is checked in one lc_setfull_check call.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence

import numpy as np

from . import _native as N
from .independent import Tuple
from .setcheck import TYPE_NAMES, SetHistory

COUNT_KEYS = ("attempt-count", "stable-count", "lost-count", "never-read-count", "stale-count", "duplicated-count")
QUANTILES = (0, 0.5, 0.95, 0.99, 1)
WORST_STALE = 8
OUTCOMES = {N.LC_SETFULL_STABLE: "stable", N.LC_SETFULL_LOST: "lost", N.LC_SETFULL_NEVER_READ: "never-read"}


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


class SetFullHistory(SetHistory):
    """A raw set-workload history with :process and :time (lc_setfull_history)."""

    def __init__(self, type_, f, key, elem, read_off, read_elem, index=None, process=None, time=None):
        super().__init__(type_, f, key, elem, read_off, read_elem, index)
        self.process = np.zeros(self.n, np.int64) if process is None else np.ascontiguousarray(process, np.int64)
        self.time = np.zeros(self.n, np.int64) if time is None else np.ascontiguousarray(time, np.int64)

    @classmethod
    def from_ops(cls, ops: Sequence[dict]) -> "SetFullHistory":
        """Op maps ({"type", "f", "value", "process", "time", "index"}) to
        columns, by the rules of lc_edn_read_setfull: a :process that is no
        integer is LC_NO_PROCESS, a missing :time is 0."""
        b = SetHistory.from_ops(ops)
        process = np.array([int(op["process"]) if _is_int(op.get("process")) else N.LC_NO_PROCESS for op in ops], np.int64)
        time = np.array([int(op["time"]) if _is_int(op.get("time")) else 0 for op in ops], np.int64)
        return cls(b.type, b.f, b.key, b.elem, b.read_off, b.read_elem[:int(b.read_off[-1])], b.index, process, time)

    @classmethod
    def read_edn(cls, path: str) -> "SetFullHistory":
        """lc_edn_read_setfull: a set-workload history.edn with :process and :time."""
        h = C.c_void_p()
        N.check(N.lib().lc_edn_read_setfull(str(path).encode(), C.byref(h)))
        try:
            return cls._from_handle(h)
        finally:
            N.lib().lc_setfull_hist_free(h)

    @classmethod
    def parse_edn(cls, text: str) -> "SetFullHistory":
        data = text.encode()
        h = C.c_void_p()
        N.check(N.lib().lc_edn_parse_setfull(data, len(data), C.byref(h)))
        try:
            return cls._from_handle(h)
        finally:
            N.lib().lc_setfull_hist_free(h)

    @classmethod
    def _from_handle(cls, h) -> "SetFullHistory":
        v = N.LcSetFullHistory()
        N.check(N.lib().lc_setfull_hist_view(h, C.byref(v)))
        n = int(v.n)
        read_off = N.carray(v.read_off, n + 1, np.int64)
        return cls(N.carray(v.type, n, np.uint8), N.carray(v.f, n, np.uint8), N.carray(v.key, n, np.int64),
                   N.carray(v.elem, n, np.int64), read_off, N.carray(v.read_elem, int(read_off[-1]), np.int64),
                   N.carray(v.index, n, np.int64), N.carray(v.process, n, np.int64), N.carray(v.time, n, np.int64))

    def as_c(self) -> N.LcSetFullHistory:
        null64 = C.POINTER(C.c_int64)()
        return N.LcSetFullHistory(self.n, N.ptr(self.type, C.c_uint8), N.ptr(self.f, C.c_uint8),
                                  null64 if self.key is None else N.ptr(self.key, C.c_int64), N.ptr(self.elem, C.c_int64),
                                  N.ptr(self.read_off, C.c_int64), N.ptr(self.read_elem, C.c_int64),
                                  null64 if self.index is None else N.ptr(self.index, C.c_int64),
                                  N.ptr(self.process, C.c_int64), N.ptr(self.time, C.c_int64))

    def op_at(self, r: int, unwrap: bool = True) -> dict:
        """Row r as an op map: its own :index where it has one, else its
        position; the value of a keyed op unwrapped (a key's sub-history)."""
        fs = {N.LC_SF_ADD: "add", N.LC_SF_READ: "read", N.LC_SF_OTHER: "other"}
        fn = fs[int(self.f[r])]
        v: Any = None
        if fn == "add":
            v = None if self.elem[r] == N.LC_NIL else int(self.elem[r])
        elif fn == "read" and self.elem[r] != N.LC_NIL:
            v = [None if x == N.LC_NIL else int(x) for x in self.read_elem[self.read_off[r]:self.read_off[r + 1]]]
        if not unwrap and fn != "other" and self.key is not None and self.key[r] != N.LC_NO_KEY:
            v = Tuple(int(self.key[r]), v)
        idx = r if self.index is None or self.index[r] < 0 else int(self.index[r])
        return {"type": TYPE_NAMES[int(self.type[r])], "f": fn, "value": v,
                "process": "nemesis" if self.process[r] == N.LC_NO_PROCESS else int(self.process[r]),
                "time": int(self.time[r]), "index": idx}

    def to_ops(self) -> List[dict]:
        """The rows as op maps again (tests; small histories)."""
        return [self.op_at(r, unwrap=False) for r in range(self.n)]


def synth_set_full(n_keys: int = 1, adds_per_key: int = 1000, read_every: int = 100, stale_window: int = 0,
                   lost_rate: float = 0.0, overlap: bool = False, info_rate: float = 0.0, seed: int = 1,
                   step_ns: int = 1_000_000) -> SetFullHistory:
    """A synthetic set-workload history with intermediate reads (tests and
    timing only).  Per key the elements 0 .. adds_per_key - 1 are added one
    after the other (:invoke, then :ok, or :info at info_rate) by processes
    0..4, and after every read_every adds, and once at the end, process 5 reads:
    every element acknowledged so far except the last stale_window of them (they
    turn up one read late: stale) and except a lost_rate share that no read ever
    holds (lost).  overlap: process 6 invokes a read just before process 5's and
    completes just after it, with the same value.  Row r has :time r * step_ns.
    Keys are laid out one after the other; several keys make tuple values.
    Built with numpy, no op maps."""
    rng = np.random.default_rng(seed)
    A, every = int(adds_per_key), max(1, int(read_every))
    cols = dict(type=[], f=[], key=[], elem=[], process=[], read_len=[])
    reads = []
    for k in range(n_keys):
        info = rng.random(A) < info_rate
        lost = (rng.random(A) < lost_rate) & ~info
        points = list(range(every, A + 1, every))
        if not points or points[-1] != A:
            points.append(A)
        per_read = 4 if overlap else 2
        n_rows = 2 * A + per_read * len(points)
        t = np.zeros(n_rows, np.uint8)
        f = np.full(n_rows, N.LC_SF_ADD, np.uint8)
        e = np.zeros(n_rows, np.int64)
        p = np.zeros(n_rows, np.int64)
        rl = np.zeros(n_rows, np.int64)
        # adds: element i's two rows come after the reads of the points <= i
        el = np.arange(A, dtype=np.int64)
        before = np.searchsorted(np.asarray(points), el, side="right")
        inv_row = 2 * el + per_read * before
        t[inv_row], t[inv_row + 1] = N.LC_INVOKE, np.where(info, N.LC_INFO, N.LC_OK_T)
        e[inv_row], e[inv_row + 1] = el, el
        p[inv_row] = p[inv_row + 1] = el % 5
        visible = ~info & ~lost
        for j, pt in enumerate(points):
            r = 2 * pt + per_read * j
            shown = np.flatnonzero(visible[:max(0, pt - stale_window) if pt < A else pt])
            rows = [(r, N.LC_INVOKE, 6), (r + 1, N.LC_INVOKE, 5), (r + 2, N.LC_OK_T, 5), (r + 3, N.LC_OK_T, 6)] if overlap \
                else [(r, N.LC_INVOKE, 5), (r + 1, N.LC_OK_T, 5)]
            for row, ty, proc in rows:
                t[row], f[row], p[row] = ty, N.LC_SF_READ, proc
                e[row] = N.LC_NIL if ty == N.LC_INVOKE else 0
                if ty == N.LC_OK_T:
                    rl[row] = len(shown)
                    reads.append(shown)
        cols["type"].append(t); cols["f"].append(f); cols["elem"].append(e); cols["process"].append(p)
        cols["read_len"].append(rl)
        cols["key"].append(np.full(n_rows, k, np.int64))
    cat = {name: np.concatenate(v) for name, v in cols.items()}
    n = len(cat["type"])
    read_off = np.zeros(n + 1, np.int64)
    np.cumsum(cat["read_len"], out=read_off[1:])
    return SetFullHistory(cat["type"], cat["f"], cat["key"] if n_keys > 1 else None, cat["elem"], read_off,
                          np.concatenate(reads) if reads else np.zeros(0, np.int64), None, cat["process"],
                          np.arange(n, dtype=np.int64) * int(step_ns))


BATCH_ARRAYS = (("id_off", np.uint64), ("span", np.uint32), ("min", np.int64), ("rank", np.uint8), ("vals_off", np.uint64),
                ("vals", np.int64), ("status", np.uint8), ("inv_pos", np.int64), ("ack_pos", np.int64),
                ("ack_time", np.int64), ("row_off", np.uint64), ("row_pos", np.int64), ("row_time", np.int64),
                ("row_inv_pos", np.int64), ("row_inv_time", np.int64), ("el_off", np.uint64), ("read_id", np.uint32))
_CTYPES = {np.uint64: C.c_uint64, np.uint32: C.c_uint32, np.int64: C.c_int64, np.uint8: C.c_uint8}


class PackedSetFull:
    """lc_setfull_pack output: the per-key arrays lc_setfull_check reads."""

    def __init__(self, hist: SetFullHistory):
        self.hist = hist
        self._c = hist.as_c()
        h = C.c_void_p()
        N.check(N.lib().lc_setfull_pack(C.byref(self._c), C.byref(h)))
        self.handle = h
        v = N.LcSetFullBatch()
        N.check(N.lib().lc_setfull_packed_view(h, C.byref(v)))
        self.view = v
        self.n_keys = int(v.n_keys)
        keys = np.zeros(max(self.n_keys, 1), np.int64)
        N.check(N.lib().lc_setfull_packed_keys(h, N.ptr(keys, C.c_int64)))
        self.keys = [None if k == N.LC_NO_KEY else int(k) for k in keys[:self.n_keys]]
        self.status = N.carray(v.status, self.n_keys, np.uint8)
        self._arrays: Optional[Dict[str, np.ndarray]] = None

    def __del__(self):
        h = getattr(self, "handle", None)
        if h:
            N.lib().lc_setfull_packed_free(h)
            self.handle = None

    def key_error(self, i: int) -> Optional[str]:
        msg = N.lib().lc_setfull_packed_key_error(self.handle, i)
        return None if msg is None else msg.decode(errors="replace")

    def arrays(self) -> Dict[str, np.ndarray]:
        """Copies of every array of the view (tests, caller-built batches)."""
        return {name: a.copy() for name, a in self._view_arrays().items()}

    def _view_arrays(self) -> Dict[str, np.ndarray]:
        """The view's arrays, copied out once and shared (result maps: read only)."""
        if self._arrays is None:
            v, K = self.view, self.n_keys
            id_off, row_off = N.carray(v.id_off, K + 1, np.uint64), N.carray(v.row_off, K + 1, np.uint64)
            vals_off = N.carray(v.vals_off, K + 1, np.uint64)
            n_ids, n_rows = int(id_off[-1]), int(row_off[-1])
            el_off = N.carray(v.el_off, n_rows + 1, np.uint64)
            sizes = dict(id_off=K + 1, span=K, min=K, rank=K, vals_off=K + 1, vals=int(vals_off[-1]), status=K,
                         inv_pos=n_ids, ack_pos=n_ids, ack_time=n_ids, row_off=K + 1, row_pos=n_rows, row_time=n_rows,
                         row_inv_pos=n_rows, row_inv_time=n_rows, el_off=n_rows + 1, read_id=int(el_off[-1]))
            self._arrays = {name: N.carray(getattr(v, name), sizes[name], dt) for name, dt in BATCH_ARRAYS}
        return self._arrays


def batch_of(arrs: Dict[str, Any]) -> N.LcSetFullBatch:
    """An lc_setfull_batch over numpy arrays (PackedSetFull.arrays(), or a
    caller's own).  The arrays must outlive the call that reads the batch."""
    pad = {}
    for name, dt in BATCH_ARRAYS:
        a = np.ascontiguousarray(arrs[name], dt)
        pad[name] = a if len(a) else np.zeros(1, dt)
    arrs["_keep"] = pad
    return N.LcSetFullBatch(len(arrs["span"]), *[N.ptr(pad[name], _CTYPES[dt]) for name, dt in BATCH_ARRAYS])


@dataclass
class SetFullResults:
    valid: np.ndarray        # int8 [K]: 1 / 0 / -1
    counts: np.ndarray       # uint64 [K, 6]: attempt, stable, lost, never-read, stale, duplicated
    outcome: np.ndarray      # uint8 [n_ids] LC_SETFULL_*
    latency: np.ndarray      # int64 [n_ids] ms, -1 where there is none
    known: np.ndarray        # int64 [n_ids] positions, -1 for nil
    last_absent: np.ndarray  # int64 [n_ids]
    duplicated: np.ndarray   # uint8 [n_ids]
    timing: Dict[str, float]


def check_batch(dev, batch: N.LcSetFullBatch, linearizable: bool = False, max_matrix_bytes: int = 0,
                flags: int = 0) -> SetFullResults:
    """lc_setfull_check on a checker.Device."""
    K = int(batch.n_keys)
    n_ids = int(batch.id_off[K]) if K else 0
    valid, counts = np.zeros(max(K, 1), np.int8), np.zeros(max(6 * K, 1), np.uint64)
    m = max(n_ids, 1)
    outcome, dup = np.zeros(m, np.uint8), np.zeros(m, np.uint8)
    latency, known, la = np.zeros(m, np.int64), np.zeros(m, np.int64), np.zeros(m, np.int64)
    r = N.LcSetFullResult(N.ptr(valid, C.c_int8), N.ptr(counts, C.c_uint64), N.ptr(outcome, C.c_uint8),
                          N.ptr(latency, C.c_int64), N.ptr(known, C.c_int64), N.ptr(la, C.c_int64), N.ptr(dup, C.c_uint8))
    o = N.LcSetFullOpts(int(bool(linearizable)), int(flags), int(max_matrix_bytes))
    N.check(N.lib().lc_setfull_check(dev.handle, C.byref(batch), C.byref(o), C.byref(r)))
    ms = (C.c_double * 8)()
    N.check(N.lib().lc_setfull_last_timing(dev.handle, ms))
    return SetFullResults(valid[:K], counts[:6 * K].reshape(K, 6), outcome[:n_ids], latency[:n_ids], known[:n_ids],
                          la[:n_ids], dup[:n_ids],
                          dict(upload_ms=ms[0], mark_ms=ms[1], scan_ms=ms[2], download_ms=ms[3], total_ms=ms[4],
                               zero_ms=ms[5], passes=int(ms[6]), matrix_bytes=int(ms[7])))


def elements_of(arrs: Dict[str, np.ndarray], i: int, ids) -> List[int]:
    """The elements of key i's ids (ascending ids are ascending elements in both id forms)."""
    if arrs["rank"][i]:
        v0 = int(arrs["vals_off"][i])
        return [int(arrs["vals"][v0 + int(x)]) for x in ids]
    mn = int(arrs["min"][i])
    return [mn + int(x) for x in ids]


def multiplicities(arrs: Dict[str, np.ndarray], i: int, ids: np.ndarray) -> Dict[int, int]:
    """The largest number of times one of key i's reads holds each of `ids`
    (the ids the device flagged): counted here, from the packed read lists."""
    r0, r1 = int(arrs["row_off"][i]), int(arrs["row_off"][i + 1])
    off = arrs["el_off"][r0:r1 + 1].astype(np.int64)
    seg = arrs["read_id"][int(off[0]):int(off[-1])] if r1 > r0 else np.zeros(0, np.uint32)
    rows = np.repeat(np.arange(r1 - r0, dtype=np.uint64), np.diff(off))
    m = np.isin(seg, ids)
    pairs, cnt = np.unique(rows[m] << np.uint64(32) | seg[m].astype(np.uint64), return_counts=True)
    out: Dict[int, int] = {}
    for pid, c in zip((pairs & np.uint64(0xFFFFFFFF)).tolist(), cnt.tolist()):
        out[pid] = max(out.get(pid, 0), c)
    return out


def quantile_map(lat: np.ndarray) -> Dict:
    """{0, 0.5, 0.95, 0.99, 1} -> sorted[min(n - 1, floor(n * p))]."""
    s = np.sort(lat)
    n = len(s)
    return {q: int(s[min(n - 1, int(np.floor(n * q)))]) for q in QUANTILES}


def result_map(packed: PackedSetFull, res: SetFullResults, i: int) -> Dict:
    """jepsen.checker/set-full's result map of packed key i."""
    if packed.status[i] != N.LC_SET_KEY_OK:
        return {"valid?": "unknown", "error": packed.key_error(i) or "error"}
    arrs = packed._view_arrays()
    v = int(res.valid[i])
    out: Dict[str, Any] = {"valid?": True if v == N.LC_VALID else False if v == N.LC_INVALID else "unknown"}
    for name, c in zip(COUNT_KEYS, res.counts[i].tolist()):
        out[name] = int(c)
    b, e = int(arrs["id_off"][i]), int(arrs["id_off"][i]) + int(arrs["span"][i])
    oc, lat = res.outcome[b:e], res.latency[b:e]
    stable, lost = oc == N.LC_SETFULL_STABLE, oc == N.LC_SETFULL_LOST
    stale = np.flatnonzero(stable & (lat > 0))
    out["lost"] = elements_of(arrs, i, np.flatnonzero(lost))
    out["never-read"] = elements_of(arrs, i, np.flatnonzero(oc == N.LC_SETFULL_NEVER_READ))
    out["stale"] = elements_of(arrs, i, stale)
    flagged = np.flatnonzero(res.duplicated[b:e])
    mult = multiplicities(arrs, i, flagged.astype(np.uint32)) if len(flagged) else {}
    out["duplicated"] = dict(zip(elements_of(arrs, i, sorted(mult)), (mult[k] for k in sorted(mult))))
    worst = stale[np.lexsort((stale, -lat[stale]))][:WORST_STALE]  # latency descending, then element ascending
    hist = packed.hist

    def op(pos: int):
        return None if pos < 0 else hist.op_at(int(pos))

    out["worst-stale"] = [{"element": el, "outcome": "stable", "stable-latency": int(lat[x]), "lost-latency": None,
                           "known": op(res.known[b + x]), "last-absent": op(res.last_absent[b + x])}
                          for x, el in zip(worst.tolist(), elements_of(arrs, i, worst))]
    if stable.any():
        out["stable-latencies"] = quantile_map(lat[stable])
    if lost.any():
        out["lost-latencies"] = quantile_map(lat[lost])
    return out


class SetFullChecker:
    """jepsen.checker/set-full on the device."""

    def __init__(self, opts: Optional[Dict] = None):
        opts = opts or {}
        self.linearizable = bool(opts.get("linearizable?", False))
        self.device = int(opts.get("device", 0))
        self.max_matrix_bytes = int(opts.get("max-matrix-bytes", 0))
        self.flags = int(opts.get("flags", 0))  # tests: LC_SETFULL_MARK_DIRECT

    def dev(self):
        from . import checker as ck
        return ck.device_for(self.device)

    def stream(self, dev=None):
        """A streaming check under this checker's options
        (lincheck.setfull_stream.SetFullStream): rows are appended while the
        test runs, and after every append the results are those of check() on
        everything appended so far."""
        from .setfull_stream import SetFullStream
        return SetFullStream(dev if dev is not None else self.dev(),
                             {"linearizable?": self.linearizable, "max-matrix-bytes": self.max_matrix_bytes})

    def _check(self, history):
        hist = history if isinstance(history, SetFullHistory) else SetFullHistory.from_ops(history)
        packed = PackedSetFull(hist)
        return packed, check_batch(self.dev(), packed.view, self.linearizable, self.max_matrix_bytes, self.flags)

    def check(self, test: Optional[Dict], history, opts: Optional[Dict] = None) -> Dict:
        """One (unwrapped) history: rows without a key are one set; of a keyed
        history, the first key's."""
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
                    ops = history.to_ops() if isinstance(history, SetFullHistory) else history
                r[name] = ck.check_safe(ch, test, subhistory(ops, k), dict(opts or {}, **{"history-key": k}))
            r["valid?"] = ck.merge_valid([x.get("valid?") for x in r.values()])
            results[k] = r
        return merge_results(results)


def set_full(opts: Optional[Dict] = None) -> SetFullChecker:
    return SetFullChecker(opts)
