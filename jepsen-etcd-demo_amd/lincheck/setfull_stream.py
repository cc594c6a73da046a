"""Streaming checker/set-full: per-element verdicts while the set test runs.

    with checker.set_full({"linearizable?": True}).stream(dev) as s:
        for rows in slices_of_the_history:        # op maps or a SetFullHistory
            u = s.append(rows)                    # Update: keys whose :valid? changed
            ...
        s.result_map(0)                           # what SetFullChecker.check returns

include/lincheck_setfull_stream.h has the contract: after every append the
per-key :valid? and counts and the per-element records equal the one-shot
check (lincheck.setfull) of everything appended so far.  The element records
stay on the device between calls; an append uploads only its own rows and
folds only its own :ok reads.  Element ids are per key, in
order of first appearance -- not PackedSetFull's numbering -- so everything
here is keyed by element value.
"""

from __future__ import annotations

import bisect
import ctypes as C
from dataclasses import dataclass
from typing import Any, Dict, List, Optional

import numpy as np

from . import _native as N
from .setfull import COUNT_KEYS, WORST_STALE, SetFullHistory, quantile_map


@dataclass
class Update:
    n_keys: int
    rows: int           # rows appended so far
    reads: int          # :ok reads folded by this append
    ids: int            # element ids resident, all checked keys
    changed: List[int]  # keys whose valid differs from before this append


@dataclass
class StreamResults:
    valid: np.ndarray        # int8 [K]
    counts: np.ndarray       # uint64 [K, 6]
    id_off: np.ndarray       # int64 [K + 1]: key i's ids are id_off[i] .. id_off[i + 1] of the arrays below
    elems: np.ndarray        # int64 [n_ids]: the element of every id
    outcome: np.ndarray      # uint8 [n_ids] LC_SETFULL_*
    latency: np.ndarray      # int64 [n_ids]
    known: np.ndarray        # int64 [n_ids] positions, -1 for nil
    last_absent: np.ndarray  # int64 [n_ids]
    duplicated: np.ndarray   # uint8 [n_ids]
    multiplicity: np.ndarray  # uint32 [n_ids]: the largest multiplicity in one read (0 or 1: never twice)


def rows_of(hist: SetFullHistory, lo: int, hi: int) -> SetFullHistory:
    """Rows lo .. hi of a history as a history of their own (an append's rows
    from columns, no op maps)."""
    hi = min(hi, hist.n)
    off = hist.read_off[lo:hi + 1]
    return SetFullHistory(hist.type[lo:hi], hist.f[lo:hi], None if hist.key is None else hist.key[lo:hi], hist.elem[lo:hi],
                          off - off[0], hist.read_elem[int(off[0]):int(off[-1])],
                          None if hist.index is None else hist.index[lo:hi], hist.process[lo:hi], hist.time[lo:hi])


CHUNK_ARRAYS = (("tk_key", np.int64, "T"), ("tk_n_ids", np.uint32, "T"), ("tk_row_off", np.uint64, "T1"),
                ("tk_blk_off", np.uint64, "T1"), ("blk", np.uint32, "B"), ("en_t", np.uint32, "E"), ("en_id", np.uint32, "E"),
                ("en_flags", np.uint32, "E"), ("en_inv_pos", np.int64, "E"), ("en_ack_pos", np.int64, "E"),
                ("en_ack_time", np.int64, "E"), ("row_pos", np.int64, "R"), ("row_time", np.int64, "R"),
                ("row_inv_pos", np.int64, "R"), ("row_inv_time", np.int64, "R"), ("el_off", np.uint64, "R1"),
                ("read_id", np.uint32, "L"))


class SetFullStream:
    """lc_setfull_stream_*.  dev: a checker.Device, or None for a packer-only
    stream (chunks and accessors, no results)."""

    def __init__(self, dev, opts: Optional[Dict] = None):
        opts = opts or {}
        self.dev = dev
        self.linearizable = bool(opts.get("linearizable?", False))
        o = N.LcSetFullOpts(int(self.linearizable), 0, int(opts.get("max-matrix-bytes", 0)))
        h = C.c_void_p()
        N.check(N.lib().lc_setfull_stream_open(dev.handle if dev is not None else None, C.byref(o), C.byref(h)))
        self.handle: Optional[C.c_void_p] = h
        self._slices: List[SetFullHistory] = []
        self._starts: List[int] = []
        self.rows = 0
        self._results: Optional[StreamResults] = None

    # -- lifetime
    def close(self) -> None:
        if self.handle:
            N.lib().lc_setfull_stream_close(self.handle)
            self.handle = None

    def __enter__(self) -> "SetFullStream":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- appends
    def append(self, rows) -> Update:
        """The next rows of the history: op maps or a SetFullHistory.  A
        refused append (LincheckError) leaves the stream as it was."""
        hist = rows if isinstance(rows, SetFullHistory) else SetFullHistory.from_ops(rows)
        c = hist.as_c()
        u = N.LcSetFullStreamUpdate()
        N.check(N.lib().lc_setfull_stream_append(self.handle, C.byref(c), C.byref(u)))
        self._starts.append(self.rows)
        self._slices.append(hist)
        self.rows = int(u.rows)
        self._results = None
        return Update(int(u.n_keys), int(u.rows), int(u.reads), int(u.ids), N.carray(u.changed, int(u.n_changed), np.int64).tolist())

    # -- accessors
    def keys(self) -> List[Optional[int]]:
        n = int(N.lib().lc_setfull_stream_keys(self.handle, None))
        out = np.zeros(max(n, 1), np.int64)
        N.lib().lc_setfull_stream_keys(self.handle, N.ptr(out, C.c_int64))
        return [None if k == N.LC_NO_KEY else int(k) for k in out[:n]]

    def key_error(self, i: int) -> Optional[str]:
        msg = N.lib().lc_setfull_stream_key_error(self.handle, i)
        return None if msg is None else msg.decode(errors="replace")

    def ids(self, i: int) -> np.ndarray:
        """Key i's elements by id (none for an error key)."""
        n = int(N.check(N.lib().lc_setfull_stream_ids(self.handle, i, None, 0)))
        out = np.zeros(max(n, 1), np.int64)
        N.check(N.lib().lc_setfull_stream_ids(self.handle, i, N.ptr(out, C.c_int64), n))
        return out[:n]

    def multiplicity(self, i: int) -> np.ndarray:
        n = len(self.ids(i))
        out = np.zeros(max(n, 1), np.uint32)
        N.check(N.lib().lc_setfull_stream_multiplicity(self.handle, i, N.ptr(out, C.c_uint32), n))
        return out[:n]

    def last_timing(self) -> Dict[str, float]:
        ms = (C.c_double * 6)()
        N.check(N.lib().lc_setfull_stream_last_timing(self.handle, ms))
        return dict(pack_ms=ms[0], upload_ms=ms[1], mark_ms=ms[2], fold_ms=ms[3], readback_ms=ms[4], passes=int(ms[5]))

    def chunk(self) -> Dict[str, np.ndarray]:
        """Copies of the last append's chunk arrays (lc_setfull_stream_chunk)."""
        v = N.LcSetFullStreamChunk()
        N.check(N.lib().lc_setfull_stream_last_chunk(self.handle, C.byref(v)))
        T, E = int(v.n_touched), int(v.n_entries)
        row_off = N.carray(v.tk_row_off, T + 1, np.uint64)
        blk_off = N.carray(v.tk_blk_off, T + 1, np.uint64)
        R = int(row_off[-1])
        el_off = N.carray(v.el_off, R + 1, np.uint64)
        sizes = {"T": T, "T1": T + 1, "B": int(blk_off[-1]), "E": E, "R": R, "R1": R + 1, "L": int(el_off[-1])}
        return {name: N.carray(getattr(v, name), sizes[sz], dt) for name, dt, sz in CHUNK_ARRAYS}

    # -- results
    def counts(self):
        """(valid int8 [K], counts uint64 [K, 6]) of every key so far."""
        K = len(self.keys())
        valid, counts = np.zeros(max(K, 1), np.int8), np.zeros(max(6 * K, 1), np.uint64)
        N.check(N.lib().lc_setfull_stream_counts(self.handle, N.ptr(valid, C.c_int8), N.ptr(counts, C.c_uint64)))
        return valid[:K], counts[:6 * K].reshape(K, 6)

    def results(self) -> StreamResults:
        if self._results is not None:
            return self._results
        K = len(self.keys())
        per_key = [self.ids(i) for i in range(K)]
        id_off = np.zeros(K + 1, np.int64)
        np.cumsum([len(e) for e in per_key], out=id_off[1:])
        n = int(id_off[-1])
        m = max(n, 1)
        valid, counts = np.zeros(max(K, 1), np.int8), np.zeros(max(6 * K, 1), np.uint64)
        outcome, dup = np.zeros(m, np.uint8), np.zeros(m, np.uint8)
        latency, known, la = np.zeros(m, np.int64), np.zeros(m, np.int64), np.zeros(m, np.int64)
        r = N.LcSetFullResult(N.ptr(valid, C.c_int8), N.ptr(counts, C.c_uint64), N.ptr(outcome, C.c_uint8),
                              N.ptr(latency, C.c_int64), N.ptr(known, C.c_int64), N.ptr(la, C.c_int64), N.ptr(dup, C.c_uint8))
        N.check(N.lib().lc_setfull_stream_results(self.handle, C.byref(r)))
        mult = [self.multiplicity(i) for i in range(K)]
        self._results = StreamResults(valid[:K], counts[:6 * K].reshape(K, 6), id_off,
                                      np.concatenate(per_key) if n else np.zeros(0, np.int64), outcome[:n], latency[:n],
                                      known[:n], la[:n], dup[:n], np.concatenate(mult) if n else np.zeros(0, np.uint32))
        return self._results

    def op_at(self, pos: int) -> Optional[dict]:
        """The row at position pos as an op map (its own :index where it has one, else its position)."""
        if pos < 0:
            return None
        j = bisect.bisect_right(self._starts, pos) - 1
        h, r = self._slices[j], pos - self._starts[j]
        op = h.op_at(r)
        if h.index is None or h.index[r] < 0:
            op["index"] = int(pos)
        return op

    def result_map(self, i: int) -> Dict:
        """jepsen.checker/set-full's result map of key i for everything
        appended so far: what lincheck.setfull.result_map builds."""
        err = self.key_error(i)
        if err is not None:
            return {"valid?": "unknown", "error": err or "error"}
        res = self.results()
        v = int(res.valid[i])
        out: Dict[str, Any] = {"valid?": True if v == N.LC_VALID else False if v == N.LC_INVALID else "unknown"}
        for name, c in zip(COUNT_KEYS, res.counts[i].tolist()):
            out[name] = int(c)
        b, e = int(res.id_off[i]), int(res.id_off[i + 1])
        order = np.argsort(res.elems[b:e], kind="stable")  # ascending elements, as the one-shot map's ids
        els, oc, lat = res.elems[b:e][order], res.outcome[b:e][order], res.latency[b:e][order]
        known, la = res.known[b:e][order], res.last_absent[b:e][order]
        dup, mult = res.duplicated[b:e][order], res.multiplicity[b:e][order]
        stable, lost = oc == N.LC_SETFULL_STABLE, oc == N.LC_SETFULL_LOST
        stale = np.flatnonzero(stable & (lat > 0))
        out["lost"] = els[lost].tolist()
        out["never-read"] = els[oc == N.LC_SETFULL_NEVER_READ].tolist()
        out["stale"] = els[stale].tolist()
        out["duplicated"] = {int(x): int(m) for x, m in zip(els[dup != 0].tolist(), mult[dup != 0].tolist())}
        worst = stale[np.lexsort((stale, -lat[stale]))][:WORST_STALE]  # latency descending, then element ascending
        out["worst-stale"] = [{"element": int(els[x]), "outcome": "stable", "stable-latency": int(lat[x]), "lost-latency": None,
                               "known": self.op_at(int(known[x])), "last-absent": self.op_at(int(la[x]))}
                              for x in worst.tolist()]
        if stable.any():
            out["stable-latencies"] = quantile_map(lat[stable])
        if lost.any():
            out["lost-latencies"] = quantile_map(lat[lost])
        return out
