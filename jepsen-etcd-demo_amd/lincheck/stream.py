"""Incremental check: a search that stays on the device while the history grows
(lc_stream_*, include/lincheck.h).

    s = Stream(dev)                  # or checker.linearizable(opts).stream(dev)
    for rows in pieces_of_the_history:
        up = s.append(rows)          # History columns, or a list of op maps
        if up.invalid:               # keys whose decided prefix is not linearizable
            stop_the_test()
    s.finish()
    res = s.results()                # valid / cause / fail_event per key

Each call searches only the events that are new; a key's verdict after
`finish` equals `Packed` + `Device.check` on the whole history.  By default a
stream returns verdicts and failing events only, no final configs: to render
the counterexample of a key found invalid, run the ordinary checker
(`checker.linearizable(...).check`) on that key's sub-history.
`failing_row(i)` names the history row of the :ok that could not be linearized.

`Stream(dev, exact=True)` keeps Knossos's exact config set of every
register-tier key on the device (LC_STREAM_EXACT): any budget is accepted and
a key that passes it turns :unknown in the append that reaches the event;
`results()` also carries `peak`, `final` and `n_final` -- a dead key's at
once, every key's after `finish`, equal to the one-shot check's -- and
`analysis(i, history)` renders a key's counterexample (:op, :previous-ok,
:configs, :final-paths) right after the append that reported it.

`Stream(dev, set_tier=True)` keeps a key that passes 10 pending ops or 32
register values on the device too (the resident set tier): it is reported
online like the others instead of at `finish`; `tiers()` / `key_tier(i)` say
where each key is searched.  With `exact=True` as well the set tier keeps the
exact sets too: a key that is invalid, or past the budget, only after leaving
the register tier is reported -- and `analysis` renders it -- in the append
that reaches the event, and only keys whose sets pass 32,768 configs within
the budget wait for `finish`.

Models: cas-register, register and mutex.  (model/multi-register) and
:algorithm :wgl have no register-tier search to resume and raise.
"""

from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from . import _native as N
from .history import History
from .model import CASRegister, MultiRegister


class Update:
    """What one call changed (lc_stream_update)."""

    def __init__(self, u: N.LcStreamUpdate):
        self.n_keys = int(u.n_keys)
        self.events = int(u.events)
        self.rows_held = int(u.rows_held)
        self.n_deferred = int(u.n_deferred)
        self.invalid = [int(u.invalid[i]) for i in range(int(u.n_invalid))]  # key indices, ascending

    def __repr__(self):
        return (f"Update(n_keys={self.n_keys}, events={self.events}, rows_held={self.rows_held}, "
                f"n_deferred={self.n_deferred}, invalid={self.invalid})")


class StreamResults:
    """valid / fail_event / cause per key; of an exact stream also peak,
    final ([key][max_final][2] words as Device.check's) and n_final (else None)."""

    def __init__(self, keys, valid, fail_event, cause, peak=None, final=None, n_final=None):
        self.keys, self.valid, self.fail_event, self.cause = keys, valid, fail_event, cause
        self.peak, self.final, self.n_final = peak, final, n_final


class Stream:
    """A resident search on `dev` (a checker.Device), or a packer-only stream
    (dev None: no device is needed, only the accessors work)."""

    TIERS = ("register", "set", "fallen_back", "dead")

    def __init__(self, dev=None, model=None, set_tier=False, exact=False):
        """set_tier: a key that leaves the register tier (10 ops pending, 32
        states) migrates to the resident set tier and keeps being searched
        online, instead of waiting for `finish` (LC_STREAM_SET_TIER).
        exact: the register tier keeps Knossos's exact sets (LC_STREAM_EXACT).
        Both: the set that migrates is exact too, so a key in the set tier
        also meets any budget at the oracle's event and brings its peak and
        final configs (a packer-only stream, dev None, refuses the pair)."""
        self.model = model if model is not None else CASRegister()
        if isinstance(self.model, MultiRegister):
            raise NotImplementedError("a stream checks (model/cas-register), (model/register) and (model/mutex)")
        self.dev = dev  # keeps the context alive
        opts = N.LcPackOpts(self.model.code)
        h = C.c_void_p()
        self.exact = bool(exact)
        sopts = N.LcStreamOpts((N.LC_STREAM_SET_TIER if set_tier else 0) | (N.LC_STREAM_EXACT if exact else 0))
        N.check(N.lib().lc_stream_open_opts(dev.handle if dev is not None else None, C.byref(opts), C.byref(sopts),
                                            C.byref(h)))
        self.handle = h

    def close(self):
        h = getattr(self, "handle", None)
        if h:
            N.lib().lc_stream_close(h)
            self.handle = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- feeding ------------------------------------------------------------
    def append(self, rows) -> Update:
        """History rows in history order: a History, or a list of op maps."""
        hist = rows if isinstance(rows, History) else History.from_ops(rows)
        c = hist.as_c()
        u = N.LcStreamUpdate()
        N.check(N.lib().lc_stream_append(self.handle, C.byref(c), C.byref(u)))
        return Update(u)

    def push(self, chunk: N.LcBatch, key_ids: Sequence[int]) -> Update:
        """A caller-packed chunk (events mode): chunk key k continues stream
        key key_ids[k].  Raises LincheckError (invalid) naming a key whose
        words are malformed; the other keys have advanced."""
        ids = np.ascontiguousarray(key_ids, dtype=np.int64)
        if len(ids) != int(chunk.n_keys):
            raise ValueError("one key id per chunk key")
        u = N.LcStreamUpdate()
        N.check(N.lib().lc_stream_push(self.handle, C.byref(chunk), N.ptr(ids if len(ids) else np.zeros(1, np.int64),
                                                                          C.c_int64), C.byref(u)))
        return Update(u)

    def finish(self) -> Update:
        u = N.LcStreamUpdate()
        N.check(N.lib().lc_stream_finish(self.handle, C.byref(u)))
        return Update(u)

    # -- reading ------------------------------------------------------------
    @property
    def keys(self) -> list:
        n = int(N.check(N.lib().lc_stream_keys(self.handle, None)))
        out = np.zeros(max(n, 1), np.int64)
        N.check(N.lib().lc_stream_keys(self.handle, N.ptr(out, C.c_int64)))
        return [int(k) for k in out[:n]]

    def results(self) -> StreamResults:
        keys = self.keys
        n = max(len(keys), 1)
        valid, fev, cause = np.zeros(n, np.int8), np.zeros(n, np.int32), np.zeros(n, np.uint8)
        r = N.LcResult()
        r.valid, r.fail_event, r.cause = N.ptr(valid, C.c_int8), N.ptr(fev, C.c_int32), N.ptr(cause, C.c_uint8)
        k = len(keys)
        if not self.exact or self.dev is None:  # (a packer-only stream: the call says so)
            N.check(N.lib().lc_stream_results(self.handle, C.byref(r)))
            return StreamResults(keys, valid[:k], fev[:k], cause[:k])
        mf = self.dev.max_final
        peak, n_final = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        final = np.zeros((n, mf, 2), np.uint64)
        r.peak_configs, r.n_final = N.ptr(peak, C.c_uint32), N.ptr(n_final, C.c_uint32)
        r.final_configs = N.ptr(final, C.c_uint64)
        N.check(N.lib().lc_stream_results(self.handle, C.byref(r)))
        return StreamResults(keys, valid[:k], fev[:k], cause[:k], peak[:k], final[:k], n_final[:k])

    def analysis(self, i: int, history, res: Optional[StreamResults] = None) -> dict:
        """Knossos's analysis of key i as the ordinary checker renders it
        (:valid?, :op, :previous-ok, :last-op, :configs, :final-paths), from an
        exact stream in rows mode.  `history` is the caller's concatenation of
        everything appended so far (a History, or a list of op maps): the
        stream keeps no copy of the rows.  res: a `results()` taken since the
        key's verdict, to spare the call."""
        from .checker import TRUNCATE, _render_words
        if not self.exact:
            raise ValueError("analysis needs Stream(dev, exact=True): a plain stream keeps no final configs")
        res = res if res is not None else self.results()
        v, c = int(res.valid[i]), int(res.cause[i])
        if v == N.LC_UNKNOWN and c == N.LC_CAUSE_ERROR:
            return {"valid?": "unknown", "error": self.key_error(i) or "error"}
        if v == N.LC_VALID:
            return {"analyzer": "linear", "configs": [], "final-paths": [], "valid?": True}
        hist = history if isinstance(history, History) else History.from_ops(history)
        fin = np.ascontiguousarray(res.final[i], dtype=np.uint64)
        cap = 4096
        while True:
            buf = np.empty(cap, np.int64)
            n = N.check(N.lib().lc_stream_report(self.handle, i, v, int(res.fail_event[i]), N.ptr(fin, C.c_uint64),
                                                 int(res.n_final[i]), TRUNCATE, N.ptr(buf, C.c_int64), cap))
            if n <= cap:
                break
            cap = n
        return _render_words(buf[:n].tolist(), v, N.CAUSES.get(c, "error"), "linear", hist, self.model)

    def key_events(self, i: int) -> dict:
        out = np.zeros(4, np.int64)
        N.check(N.lib().lc_stream_key_events(self.handle, i, N.ptr(out, C.c_int64)))
        return {"emitted": int(out[0]), "held": int(out[1]), "deferred_at": int(out[2]), "searched": int(out[3])}

    def event_row(self, i: int, j: int) -> int:
        return int(N.check(N.lib().lc_stream_event_row(self.handle, i, j)))

    def failing_row(self, i: int) -> Optional[int]:
        """History row of the :ok key i could not linearize (rows mode), or None."""
        res = self.results()
        if res.valid[i] != N.LC_INVALID or res.fail_event[i] < 0:
            return None
        return self.event_row(i, int(res.fail_event[i]))

    def words(self, i: int) -> np.ndarray:
        n = int(N.check(N.lib().lc_stream_key_words(self.handle, i, None, 0)))
        out = np.zeros(max(n, 1), np.uint32)
        N.check(N.lib().lc_stream_key_words(self.handle, i, N.ptr(out, C.c_uint32), n))
        return out[:n]

    def trans(self, i: int) -> np.ndarray:
        n = int(N.check(N.lib().lc_stream_key_trans(self.handle, i, None, 0)))
        out = np.zeros(max(n, 1), np.uint32)
        N.check(N.lib().lc_stream_key_trans(self.handle, i, N.ptr(out, C.c_uint32), n))
        return out[:n]

    def state_value(self, i: int, s: int):
        v = C.c_int64(); nil = C.c_int()
        N.check(N.lib().lc_stream_state_value(self.handle, i, s, C.byref(v), C.byref(nil)))
        return None if nil.value else int(v.value)

    def key_error(self, i: int) -> Optional[str]:
        msg = N.lib().lc_stream_key_error(self.handle, i)
        return None if msg is None else msg.decode(errors="replace")

    def record(self, i: int) -> np.ndarray:
        """Key i's device record (diagnostics; layout: csrc/stream_plan.hpp)."""
        out = np.zeros(N.LC_STREAM_REC_WORDS, np.uint32)
        N.check(N.lib().lc_stream_record(self.handle, i, N.ptr(out, C.c_uint32)))
        return out

    def key_tier(self, i: int) -> str:
        """Where key i is searched: "register", "set", "fallen_back" (checked
        at `finish`, from its first event) or "dead" (invalid or in error)."""
        return self.TIERS[int(N.check(N.lib().lc_stream_key_tier(self.handle, i)))]

    def tiers(self) -> dict:
        """Keys in each tier."""
        out = np.zeros(4, np.int64)
        N.check(N.lib().lc_stream_tiers(self.handle, N.ptr(out, C.c_int64)))
        return dict(zip(self.TIERS, map(int, out)))

    def set_record(self, i: int) -> dict:
        """Key i's set record (diagnostics; layout: csrc/stream_plan.hpp): the
        header words, the descriptors by window slot and the current configs
        (state << 56 | window-slot bits)."""
        n = int(N.check(N.lib().lc_stream_set_record(self.handle, i, None, 0)))
        out = np.zeros(n, np.uint32)
        N.check(N.lib().lc_stream_set_record(self.handle, i, N.ptr(out, C.c_uint32), n))
        hw = N.LC_STREAM_SET_HEAD_WORDS
        cfg = out[hw:].astype(np.uint64)
        return {"header": out[:16], "descs": out[16:hw], "configs": cfg[0::2] | (cfg[1::2] << np.uint64(32))}

    def set_stats(self) -> dict:
        """The last call's set-tier device times and the set-record pool."""
        out = np.zeros(6, np.float64)
        N.check(N.lib().lc_stream_set_stats(self.handle, N.ptr(out, C.c_double)))
        return {"migrate_ms": float(out[0]), "set_kernel_ms": float(out[1]), "pool_slots": int(out[2]),
                "pool_in_use": int(out[3]), "pool_peak": int(out[4]), "slot_bytes": int(out[5])}

    def exact_stats(self) -> dict:
        """Exact mode: k_stream_final's device time at `finish`, ms."""
        out = np.zeros(2, np.float64)
        N.check(N.lib().lc_stream_exact_stats(self.handle, N.ptr(out, C.c_double)))
        return {"final_kernel_ms": float(out[0]), "final_keys": int(out[1])}

    def last_timing(self) -> dict:
        out = np.zeros(4, np.float64)
        N.check(N.lib().lc_stream_last_timing(self.handle, N.ptr(out, C.c_double)))
        return dict(zip(("pack_ms", "upload_ms", "kernel_ms", "readback_ms"), map(float, out)))
