"""Streaming checker/total-queue and checker/unique-ids: a tally that stays on
the device, verdicts after every append.

    with checker.total_queue().stream(dev) as s:
        for rows in slices_of_the_history:        # op maps or a QueueHistory
            u = s.append(rows)                    # Update: keys whose :valid? changed
            ...
        s.result_map(0)                           # what TotalQueueChecker.check returns

include/lincheck_queue_stream.h has the contract: after every append the keys,
per-key :valid?, counts, range and the anomalous values equal the one-shot
check (lincheck.queue) of everything appended so far.  :valid? is not monotone:
a value that is lost now may be dequeued by a later append.  The hash table
stays on the device between calls and grows as values arrive; an append uploads
only its own rows.  dev None opens the host stream: the same
contract by an incremental fold in plain C++ on one thread.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Optional

import numpy as np

from . import _native as N
from .queue import FIRST_ENT_CAP, QueueHistory, QueueResults, result_map


@dataclass
class Update:
    n_keys: int
    rows: int           # history rows appended so far
    packed: int         # values that count in this append
    distinct: int       # distinct (key, value) resident
    slots: int          # the table's slots
    grew: bool          # this append grew the table first
    changed: List[int]  # keys whose valid differs from before this append


def rows_of(hist: QueueHistory, lo: int, hi: int) -> QueueHistory:
    """Rows lo .. hi of a history as a history of their own (an append's rows
    from columns, no op maps)."""
    hi = min(hi, hist.n)
    if hist.drain_off is None:
        off, dv = None, None
    else:
        off = hist.drain_off[lo:hi + 1]
        dv = hist.drain_val[int(off[0]):int(off[-1])]
        off = off - off[0]
    return QueueHistory(hist.type[lo:hi], hist.f[lo:hi], None if hist.key is None else hist.key[lo:hi], hist.value[lo:hi], off, dv)


def launch_info() -> Dict[str, int]:
    out = np.zeros(6, np.int64)
    N.check(N.lib().lc_queue_stream_launch_info(N.ptr(out, C.c_int64)))
    names = ("block", "slots_per_value", "slot_bytes", "max_bytes", "default_slots", "launch_rows")
    return dict(zip(names, out.tolist()))


class _View:
    """What lincheck.queue.result_map reads of a PackedQueue, from a stream."""

    def __init__(self, stream: "QueueStream", n_keys: int):
        self.mode = stream.mode
        self._stream = stream
        self.status = np.array([N.LC_QUEUE_KEY_OK if stream.key_error(i) is None else N.LC_QUEUE_KEY_ERROR
                                for i in range(n_keys)], np.uint8)

    def key_error(self, i: int) -> Optional[str]:
        return self._stream.key_error(i)


class QueueStream:
    """lc_queue_stream_*.  dev: a checker.Device, or None for the host stream.
    opts: {"slots": the table's first size, a power of two (0: the default),
    "ent-cap": results()' first entry capacity}."""

    def __init__(self, dev, mode: int, opts: Optional[Dict] = None):
        opts = opts or {}
        self.dev = dev
        self.mode = int(mode)
        self.ent_cap = opts.get("ent-cap")
        o = N.LcQueueStreamOpts(int(opts.get("slots", 0)), 0)
        h = C.c_void_p()
        N.check(N.lib().lc_queue_stream_open(dev.handle if dev is not None else None, self.mode, C.byref(o), C.byref(h)))
        self.handle: Optional[C.c_void_p] = h
        self.rows = 0
        self._results: Optional[QueueResults] = None

    # -- lifetime
    def close(self) -> None:
        if self.handle:
            N.lib().lc_queue_stream_close(self.handle)
            self.handle = None

    def __enter__(self) -> "QueueStream":
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
        """The next rows of the history: op maps or a QueueHistory.  A refused
        append (LincheckError) leaves the stream as it was."""
        hist = rows if isinstance(rows, QueueHistory) else QueueHistory.from_ops(rows)
        c = hist.as_c()
        u = N.LcQueueStreamUpdate()
        N.check(N.lib().lc_queue_stream_append(self.handle, C.byref(c), C.byref(u)))
        self.rows = int(u.rows)
        self._results = None
        return Update(int(u.n_keys), int(u.rows), int(u.packed), int(u.distinct), int(u.slots), bool(u.grew),
                      N.carray(u.changed, int(u.n_changed), np.int64).tolist())

    # -- accessors
    def keys(self) -> List[Optional[int]]:
        n = int(N.lib().lc_queue_stream_keys(self.handle, None))
        out = np.zeros(max(n, 1), np.int64)
        N.lib().lc_queue_stream_keys(self.handle, N.ptr(out, C.c_int64))
        return [None if k == N.LC_NO_KEY else int(k) for k in out[:n]]

    def key_error(self, i: int) -> Optional[str]:
        msg = N.lib().lc_queue_stream_key_error(self.handle, i)
        return None if msg is None else msg.decode(errors="replace")

    def last_timing(self) -> Dict[str, float]:
        ms = (C.c_double * 6)()
        N.check(N.lib().lc_queue_stream_last_timing(self.handle, ms))
        return dict(pack_ms=ms[0], upload_ms=ms[1], kernel_ms=ms[2], readback_ms=ms[3], grow_ms=ms[4], total_ms=ms[5])

    # -- results
    def _arrays(self, K: int):
        m = max(K, 1)
        return (np.zeros(m, np.int8), np.zeros((m, N.LC_QN_COUNTS), np.uint64), np.zeros(m, np.int64), np.zeros(m, np.int64),
                np.zeros(m, np.uint8))

    def counts(self):
        """(valid int8 [K], counts uint64 [K, 7], lo, hi int64 [K], has_range
        uint8 [K]) of every key so far; reads nothing from the table."""
        K = len(self.keys())
        valid, counts, lo, hi, has = self._arrays(K)
        N.check(N.lib().lc_queue_stream_counts(self.handle, N.ptr(valid, C.c_int8), N.ptr(counts, C.c_uint64), N.ptr(lo, C.c_int64),
                                               N.ptr(hi, C.c_int64), N.ptr(has, C.c_uint8)))
        return valid[:K], counts[:K], lo[:K], hi[:K], has[:K]

    def results(self, ent_cap: Optional[int] = None) -> QueueResults:
        """Everything appended so far as lincheck.queue.check_batch returns it.
        ent_cap: the first capacity of the entry arrays; with more entries the
        call says how many and is made once more."""
        if self._results is not None and ent_cap is None:
            return self._results
        K = len(self.keys())
        valid, counts, lo, hi, has = self._arrays(K)
        cap = ent_cap if ent_cap is not None else self.ent_cap if self.ent_cap is not None else FIRST_ENT_CAP
        cap, retried = int(cap), False
        while True:
            m = max(cap, 1)
            ek, ec, ev, em = np.zeros(m, np.uint32), np.zeros(m, np.uint8), np.zeros(m, np.int64), np.zeros(m, np.uint64)
            r = N.LcQueueResult(N.ptr(valid, C.c_int8), N.ptr(counts, C.c_uint64), N.ptr(lo, C.c_int64), N.ptr(hi, C.c_int64),
                                N.ptr(has, C.c_uint8), N.ptr(ek, C.c_uint32), N.ptr(ec, C.c_uint8), N.ptr(ev, C.c_int64),
                                N.ptr(em, C.c_uint64), cap, 0)
            rc = N.lib().lc_queue_stream_results(self.handle, C.byref(r))
            if rc == -2 and int(r.n_ent) > cap and not retried:  # LC_E_NOMEM: the entry arrays were too small
                cap, retried = int(r.n_ent), True
                continue
            N.check(rc)
            break
        ne = int(r.n_ent)
        self._results = QueueResults(valid[:K], counts[:K], lo[:K], hi[:K], has[:K], ek[:ne], ec[:ne], ev[:ne], em[:ne],
                                     self.last_timing(), retried)
        return self._results

    def result_map(self, i: int) -> Dict:
        """The checker's result map of key i for everything appended so far:
        what lincheck.queue.result_map builds of the one-shot check."""
        res = self.results()
        return result_map(_View(self, len(res.valid)), res, i)

    def result_maps(self) -> Dict:
        """{key: result map} of every key so far (a stream without tuples: {None: map})."""
        res = self.results()
        view = _View(self, len(res.valid))
        return {k: result_map(view, res, i) for i, k in enumerate(self.keys())}
