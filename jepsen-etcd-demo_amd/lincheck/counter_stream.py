"""Streaming checker/counter: every key's running sums and every read's bounds
stay resident, verdicts after every append.

    with checker.counter().stream(dev) as s:
        for rows in slices_of_the_history:        # op maps or a CounterHistory
            u = s.append(rows)                    # Update: keys whose :valid? changed
            ...
        s.result_maps()                           # what CounterChecker returns, per key

include/lincheck_counter_stream.h has the contract: after every append the
keys, per-key :valid? and error counts, every read's bounds and the reads out
of bounds equal the one-shot check (lincheck.counter) of everything appended so
far.  Past answers are revised: a :fail that arrives later takes its
:invoke :add out of the upper bound of every read completed since, so :valid?
moves in either direction, and a key that is :unknown because of a nil add
still open comes back when that add completes.  dev None opens
the host stream: the same contract by an incremental fold in plain C++ on one
thread.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Optional

import numpy as np

from . import _native as N
from .counter import FIRST_ERR_CAP, CounterHistory, CounterResults, result_map


@dataclass
class Update:
    n_keys: int
    rows: int           # history rows appended so far
    events: int         # packed events of this append
    reads: int          # :ok reads of this append
    reads_total: int    # reads resident
    patched: int        # invocations of earlier appends this one revised
    revisited: int      # resident reads looked at again because of them
    grew: bool          # this append grew the reads array first
    changed: List[int]  # keys whose valid differs from before this append


def rows_of(hist: CounterHistory, lo: int, hi: int) -> CounterHistory:
    """Rows lo .. hi of a history as a history of their own (an append's rows
    from columns, no op maps)."""
    hi = min(hi, hist.n)
    return CounterHistory(hist.type[lo:hi], hist.f[lo:hi], hist.process[lo:hi], None if hist.key is None else hist.key[lo:hi],
                          hist.value[lo:hi], None if hist.index is None else hist.index[lo:hi])


def launch_info() -> Dict[str, int]:
    out = np.zeros(6, np.int64)
    N.check(N.lib().lc_counter_stream_launch_info(N.ptr(out, C.c_int64)))
    names = ("block", "default_tile", "read_bytes", "max_bytes", "default_reads", "launch_events")
    return dict(zip(names, out.tolist()))


class _View:
    """What lincheck.counter.result_map reads of a PackedCounter, from a stream."""

    def __init__(self, stream: "CounterStream", n_reads: np.ndarray, value: np.ndarray):
        self._stream = stream
        K = len(n_reads)
        self.status = np.array([N.LC_COUNTER_KEY_OK if stream.key_error(i) is None else N.LC_COUNTER_KEY_ERROR for i in range(K)],
                               np.uint8)
        self.read_off = np.concatenate([[0], np.cumsum(n_reads.astype(np.int64))]).astype(np.int64)
        self._value = value

    def key_error(self, i: int) -> Optional[str]:
        return self._stream.key_error(i)

    def read_val(self) -> np.ndarray:
        return self._value


class CounterStream:
    """lc_counter_stream_*.  dev: a checker.Device, or None for the host
    stream.  opts: {"tile": 256 | 2048 (0: the default), "reads": the reads
    array's first capacity, "launch-events": the events of one launch,
    "err-cap": results()' first err_idx capacity}."""

    def __init__(self, dev, opts: Optional[Dict] = None):
        opts = opts or {}
        self.dev = dev
        self.err_cap = opts.get("err-cap")
        o = N.LcCounterStreamOpts(int(opts.get("tile") or 0), int(opts.get("reads") or 0), int(opts.get("launch-events") or 0), 0)
        h = C.c_void_p()
        N.check(N.lib().lc_counter_stream_open(dev.handle if dev is not None else None, C.byref(o), C.byref(h)))
        self.handle: Optional[C.c_void_p] = h
        self.rows = 0
        self._results: Optional[CounterResults] = None
        self._value: Optional[np.ndarray] = None

    # -- lifetime
    def close(self) -> None:
        if self.handle:
            N.lib().lc_counter_stream_close(self.handle)
            self.handle = None

    def __enter__(self) -> "CounterStream":
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
        """The next rows of the history: op maps or a CounterHistory.  A
        refused append (LincheckError) leaves the stream as it was."""
        hist = rows if isinstance(rows, CounterHistory) else CounterHistory.from_ops(rows)
        c = hist.as_c()
        u = N.LcCounterStreamUpdate()
        N.check(N.lib().lc_counter_stream_append(self.handle, C.byref(c), C.byref(u)))
        self.rows = int(u.rows)
        self._results = None
        return Update(int(u.n_keys), int(u.rows), int(u.events), int(u.reads), int(u.reads_total), int(u.patched),
                      int(u.revisited), bool(u.grew), N.carray(u.changed, int(u.n_changed), np.int64).tolist())

    # -- accessors
    def keys(self) -> List[Optional[int]]:
        n = int(N.lib().lc_counter_stream_keys(self.handle, None))
        out = np.zeros(max(n, 1), np.int64)
        N.lib().lc_counter_stream_keys(self.handle, N.ptr(out, C.c_int64))
        return [None if k == N.LC_NO_KEY else int(k) for k in out[:n]]

    def key_error(self, i: int) -> Optional[str]:
        msg = N.lib().lc_counter_stream_key_error(self.handle, i)
        return None if msg is None else msg.decode(errors="replace")

    def last_timing(self) -> Dict[str, float]:
        ms = (C.c_double * 6)()
        N.check(N.lib().lc_counter_stream_last_timing(self.handle, ms))
        return dict(pack_ms=ms[0], upload_ms=ms[1], kernel_ms=ms[2], readback_ms=ms[3], grow_ms=ms[4], total_ms=ms[5])

    # -- results
    def counts(self):
        """(valid int8 [K], n_errors uint64 [K], n_reads uint64 [K]) of every
        key so far; reads nothing from the device."""
        K = len(self.keys())
        m = max(K, 1)
        valid, n_errors, n_reads = np.zeros(m, np.int8), np.zeros(m, np.uint64), np.zeros(m, np.uint64)
        N.check(N.lib().lc_counter_stream_counts(self.handle, N.ptr(valid, C.c_int8), N.ptr(n_errors, C.c_uint64),
                                                 N.ptr(n_reads, C.c_uint64)))
        return valid[:K], n_errors[:K], n_reads[:K]

    def results(self, err_cap: Optional[int] = None) -> CounterResults:
        """Everything appended so far as lincheck.counter.check_batch returns
        it.  err_cap: the first capacity of err_idx; with more reads out of
        bounds the call says how many and is made once more."""
        if self._results is not None and err_cap is None:
            return self._results
        valid, _, n_reads = self.counts()
        K, R = len(valid), int(n_reads.sum())
        valid, n_errors = np.zeros(max(K, 1), np.int8), np.zeros(max(K, 1), np.uint64)
        lower, upper, value = (np.zeros(max(R, 1), np.int64) for _ in range(3))
        err_off = np.zeros(K + 1, np.uint64)
        cap = err_cap if err_cap is not None else self.err_cap if self.err_cap is not None else min(R, FIRST_ERR_CAP)
        cap, retried = int(cap), False
        while True:
            err_idx = np.zeros(max(cap, 1), np.uint64)
            r = N.LcCounterResult(N.ptr(valid, C.c_int8), N.ptr(n_errors, C.c_uint64), N.ptr(lower, C.c_int64),
                                  N.ptr(upper, C.c_int64), N.ptr(err_off, C.c_uint64), N.ptr(err_idx, C.c_uint64), cap, 0)
            rc = N.lib().lc_counter_stream_results(self.handle, C.byref(r), N.ptr(value, C.c_int64))
            if rc == -2 and int(r.n_err) > cap and not retried:  # LC_E_NOMEM: err_idx was too small
                cap, retried = int(r.n_err), True
                continue
            N.check(rc)
            break
        t = self.last_timing()
        self._value = value[:R]
        self._n_reads = n_reads
        self._results = CounterResults(valid[:K], n_errors[:K], lower[:R], upper[:R], err_off, err_idx[:int(r.n_err)],
                                       dict(upload_ms=t["upload_ms"], kernel_ms=t["kernel_ms"], download_ms=t["readback_ms"],
                                            total_ms=t["total_ms"]), retried)
        return self._results

    def read_values(self) -> np.ndarray:
        """The reads' values in results()' order."""
        self.results()
        return self._value

    def _view(self) -> _View:
        self.results()
        return _View(self, self._n_reads, self._value)

    def result_map(self, i: int) -> Dict:
        """The checker's result map of key i for everything appended so far:
        what lincheck.counter.result_map builds of the one-shot check."""
        return result_map(self._view(), self.results(), i)

    def result_maps(self) -> Dict:
        """{key: result map} of every key so far (a stream without tuples: {None: map})."""
        res, view = self.results(), self._view()
        return {k: result_map(view, res, i) for i, k in enumerate(self.keys())}
