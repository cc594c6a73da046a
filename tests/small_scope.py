"""Every small history of a model, enumerated without duplicates.

A sampler over 1,000-op keys meets the event rules' corner cases -- a cas
whose old and new value are equal, a read of nil after a crashed write, an op
left open at the end of the key, a process reused after an :ok and retired
after an :info, the first :ok of a key being the failing event -- by luck.
Here they are all present: a scope is every key sub-history of a model with a
fixed number of invocations over the values {0, 1}, given completion types and
a bound on the ops pending at once.

enumerate_scope(name) walks a tree whose node is (events so far, pending ops
in invocation order, invocations left, crashed processes); from every node,
in this order:

 1. emit   -- no invocation left, and nothing pending or the scope allows
              `open`: the events so far are one key (ops still pending stay
              open);
 2. invoke -- an invocation left and fewer than `most pending` ops pending:
              the lowest process id neither pending nor crashed invokes each
              op of the model in turn (cas-register: read, write 0, write 1,
              cas [a b] for the four pairs; register: read, write 0, write 1;
              mutex: acquire, release);
 3. complete -- each pending op in list order, with each completion type of
              the scope other than `open`: an :ok of a read once per read
              value (0, 1, nil), anything else once with the invocation's
              value; an :info retires the process.

Every key's peak is at most 11 configs and at most 4 of its ops are pending at
once, so as enumerated all of them live in the register tier.  widened() takes
them out of it without changing a record: it inserts n inert ops into every
key -- a crashed op whose precondition names INERT, a value no op of a scope
ever writes (cas-register: {:invoke :cas [7 7]} {:info :cas [7 7]}; register:
{:invoke :read 7} {:info :read 7}), each on a process of its own.  Such an op
can never be linearized, so it multiplies no config set, but it stays pending
for good and holds a window slot: 11 of them put every key past the register
tier's 10 pending ops (the set tier T1, the stream's resident set tier), 62
put the live ops past the narrow config's 56 slots (the wide HBM tier, window
slots 62..65 across the two words of a wide config).  valid, peak and probes
stay the unwidened key's; the failing event moves by the inert invokes before
it (Widened.expected_fail_event).  Still out of reach: T2, the narrow HBM tier
and the layered tier (reached only by outgrowing T1, which no small history
does), mutex4 (a crashed acquire or release is legal in some state: the model
has no inert op) and table models.

SCOPES[name].keys / .rows / .valid / .invalid are the counts the rule gives
and the oracle's split (oracle/brute.py = oracle/linear_ref.c on every key);
scope() checks the first two and that the keys are distinct.
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache
from itertools import chain
from typing import Iterator, Tuple

import numpy as np

from lincheck import history as H
from lincheck import model as M

VALUES = (0, 1)
INERT = 7  # the value widened()'s inert ops name: no op of a scope writes it
READ_VALUES = (0, 1, None)
OPS = {
    "cas-register": [("read", None), ("write", 0), ("write", 1)] + [("cas", (a, b)) for a in VALUES for b in VALUES],
    "register": [("read", None), ("write", 0), ("write", 1)],
    "mutex": [("acquire", None), ("release", None)],
}
PROCS_PER_KEY = 8  # process of key k, enumeration process p: 8 * k + p (a key invokes at most 4 ops)
INERT_PROC_BASE = 1 << 40  # inert op i of key k: INERT_PROC_BASE + n_inert * k + i (live ones stay below 8 * 177,147)
PLACES = ("head", "mid", "tail")


@dataclass(frozen=True)
class Scope:
    name: str
    model: str
    n_ops: int
    completions: Tuple[str, ...]   # of "ok", "fail", "info", "open"
    most_pending: int
    keys: int
    rows: int
    valid: int
    invalid: int
    peak: int                      # the largest oracle peak of a key

    def model_obj(self):
        return {"cas-register": M.cas_register, "register": M.register, "mutex": M.mutex}[self.model]()


SCOPES = {s.name: s for s in (
    Scope("cas2", "cas-register", 2, ("ok", "fail", "info", "open"), 2, 2_119, 7_895, 1_345, 774, 2),
    Scope("cas3", "cas-register", 3, ("ok", "info", "open"), 3, 93_367, 522_885, 43_411, 49_956, 5),
    Scope("cas4p2", "cas-register", 4, ("ok",), 2, 177_147, 1_417_176, 24_773, 152_374, 4),
    Scope("reg4", "register", 4, ("ok",), 4, 65_625, 525_000, 29_247, 36_378, 11),
    Scope("mutex4", "mutex", 4, ("ok", "info", "open"), 4, 43_536, 328_064, 31_286, 12_250, 3),
)}
ORDER = tuple(SCOPES)


def enumerate_scope(name: str) -> Iterator[tuple]:
    """Each key of the scope as a tuple of events (type, f, value, process)."""
    sc = SCOPES[name]
    invocations = OPS[sc.model]
    done_types = [t for t in sc.completions if t != "open"]
    allow_open = "open" in sc.completions

    def walk(events, pending, left, crashed):
        if left == 0 and (allow_open or not pending):
            yield events
        if left > 0 and len(pending) < sc.most_pending:
            busy = {p for p, _, _ in pending} | crashed
            proc = next(p for p in range(PROCS_PER_KEY) if p not in busy)
            for f, v in invocations:
                yield from walk(events + (("invoke", f, v, proc),), pending + ((proc, f, v),), left - 1, crashed)
        for i, (proc, f, v) in enumerate(pending):
            rest = pending[:i] + pending[i + 1:]
            for t in done_types:
                for value in (READ_VALUES if t == "ok" and f == "read" else (v,)):
                    yield from walk(events + ((t, f, value, proc),), rest, left,
                                    crashed | {proc} if t == "info" else crashed)

    yield from walk((), (), sc.n_ops, frozenset())


def key_ops(events, key=None) -> list:
    """One key's events as op maps (an unwrapped sub-history; with `key`, the
    values wrapped in independent tuples and the processes made distinct)."""
    from lincheck.independent import Tuple as T
    out = []
    for i, (t, f, v, p) in enumerate(events):
        v = list(v) if isinstance(v, tuple) else v
        if key is not None:
            v, p = T(key, v), PROCS_PER_KEY * key + p
        out.append({"type": t, "f": f, "value": v, "process": p, "index": i})
    return out


def round_robin_of(h: H.History, off) -> H.History:
    """A key-major history's rows (row offsets per key: off), one row of each
    key in turn (as stream_helpers.merged_round_robin orders them), :index
    renumbered."""
    off = np.asarray(off, np.int64)
    pos = np.arange(len(h), dtype=np.int64) - np.repeat(off[:-1], np.diff(off))
    perm = np.lexsort((h.key, pos))
    return H.History(h.type[perm], h.f[perm], h.process[perm], h.key[perm], h.v0[perm], h.v1[perm],
                     np.arange(len(perm), dtype=np.int64))


class Built:
    """A scope enumerated: .events (the key tuples), .hist (key-major History,
    key = enumeration index), .off (row offsets per key, K + 1)."""

    def __init__(self, name: str):
        self.scope = SCOPES[name]
        self.events = list(enumerate_scope(name))
        sc = self.scope
        assert len(self.events) == sc.keys, f"{name}: {len(self.events)} keys, the rule gives {sc.keys}"
        assert len(set(self.events)) == len(self.events), f"{name}: a key is enumerated twice"
        # the distinct events are a few dozen: columns by table lookup
        code = {}
        for ev in chain.from_iterable(self.events):
            if ev not in code:
                code[ev] = len(code)
        table = np.zeros((len(code), 5), np.int64)  # type, f, v0, v1, process
        for (t, f, v, p), c in code.items():
            a, b = (v if isinstance(v, tuple) else (v, None))
            table[c] = (H.TYPES[t], H.FS[f], H.NIL if a is None else a, H.NIL if b is None else b, p)
        lens = np.fromiter((len(e) for e in self.events), np.int64, len(self.events))
        n = int(lens.sum())
        assert n == sc.rows, f"{name}: {n} rows, the rule gives {sc.rows}"
        idx = np.fromiter((code[ev] for ev in chain.from_iterable(self.events)), np.int64, n)
        self.off = np.concatenate([[0], np.cumsum(lens)])
        key = np.repeat(np.arange(len(self.events), dtype=np.int64), lens)
        col = table[idx]
        self.hist = H.History(col[:, 0], col[:, 1], PROCS_PER_KEY * key + col[:, 4], key, col[:, 2], col[:, 3],
                              np.arange(n, dtype=np.int64))

    @property
    def n_keys(self) -> int:
        return len(self.events)

    def slice(self, lo: int, hi: int) -> H.History:
        """Keys lo .. hi as a key-major history of their own (:index kept)."""
        a, b = int(self.off[lo]), int(self.off[hi])
        h = self.hist
        return H.History(h.type[a:b], h.f[a:b], h.process[a:b], h.key[a:b], h.v0[a:b], h.v1[a:b], h.index[a:b])

    def round_robin(self) -> H.History:
        """The same rows, one row of each key in turn (as
        stream_helpers.merged_round_robin orders them), :index renumbered."""
        return round_robin_of(self.hist, self.off)

    def ops(self, k: int) -> list:
        """Key k's unwrapped sub-history as op maps."""
        return key_ops(self.events[k])

    def describe(self, k: int) -> str:
        return f"{self.scope.name} key {k}: " + " ".join(
            f"[p{p} :{t} :{f} {list(v) if isinstance(v, tuple) else 'nil' if v is None else v}]"
            for t, f, v, p in self.events[k])


@lru_cache(maxsize=None)
def scope(name: str) -> Built:
    return Built(name)


class Widened:
    """A scope with n_inert inert ops in every key (module docstring): .hist
    (key-major, :index renumbered), .off (row offsets per key), .at (the row of
    the unwidened key the inert block stands before), and per reduced event of
    the unwidened keys -- offsets .ev_off, K + 1 -- .ev_shift: the inert invokes
    placed before it (0 or n_inert)."""

    def __init__(self, built: Built, n_inert: int, place: str):
        sc, h, off = built.scope, built.hist, built.off
        if sc.model == "mutex":
            raise ValueError("mutex has no inert op: a crashed acquire or release is legal in some state")
        self.built, self.scope, self.n_inert, self.place = built, sc, n_inert, place
        K, m = built.n_keys, n_inert
        n = np.diff(off)
        self.at = {"head": np.zeros(K, np.int64), "mid": n // 2, "tail": np.maximum(n - 1, 0)}[place]
        self.off = off + 2 * m * np.arange(K + 1, dtype=np.int64)
        total = int(self.off[-1])
        pos = np.arange(len(h), dtype=np.int64) - np.repeat(off[:-1], n)
        after = pos >= np.repeat(self.at, n)
        old = np.repeat(self.off[:-1], n) + pos + 2 * m * after                        # where the scope's rows go
        i = np.tile(np.arange(2 * m, dtype=np.int64), K)
        k = np.repeat(np.arange(K, dtype=np.int64), 2 * m)
        new = np.repeat(self.off[:-1] + self.at, 2 * m) + i                            # where the inert rows go
        cas = sc.model == "cas-register"
        col = {a: np.empty(total, getattr(h, a).dtype) for a in ("type", "f", "process", "key", "v0", "v1")}
        for a in col:
            col[a][old] = getattr(h, a)
        col["type"][new] = np.where(i % 2 == 0, H.TYPES["invoke"], H.TYPES["info"])
        col["f"][new] = H.FS["cas" if cas else "read"]
        col["process"][new] = INERT_PROC_BASE + m * k + i // 2
        col["key"][new] = k
        col["v0"][new] = INERT
        col["v1"][new] = INERT if cas else H.NIL
        self.hist = H.History(col["type"], col["f"], col["process"], col["key"], col["v0"], col["v1"],
                              np.arange(total, dtype=np.int64))
        # The unwidened keys' reduced events: every :ok row, and every :invoke
        # row but those a :fail answers.  A key's processes alternate :invoke
        # and completion, so by (process, row) an :invoke's completion, if it
        # has one, is the next row.
        order = np.lexsort((np.arange(len(h)), h.process))
        t, p = h.type[order], h.process[order]
        failed = np.zeros(len(h), bool)
        failed[:-1] = (t[:-1] == H.TYPES["invoke"]) & (p[1:] == p[:-1]) & (t[1:] == H.TYPES["fail"])
        is_event = np.zeros(len(h), bool)
        is_event[order] = ((t == H.TYPES["invoke"]) & ~failed) | (t == H.TYPES["ok"])
        self.ev_off = np.concatenate([[0], np.cumsum(is_event)])[off]
        self.ev_shift = np.where(after[is_event], m, 0).astype(np.int64)

    @property
    def n_keys(self) -> int:
        return self.built.n_keys

    def expected_fail_event(self, fail_event) -> np.ndarray:
        """The widened keys' failing events from the unwidened ones (-1 stays)."""
        fe = np.asarray(fail_event, np.int64)
        bad = fe >= 0
        out = fe.copy()
        out[bad] += self.ev_shift[self.ev_off[:-1][bad] + fe[bad]]
        return out

    def slice(self, lo: int, hi: int) -> H.History:
        a, b = int(self.off[lo]), int(self.off[hi])
        h = self.hist
        return H.History(h.type[a:b], h.f[a:b], h.process[a:b], h.key[a:b], h.v0[a:b], h.v1[a:b], h.index[a:b])

    def round_robin(self, lo: int = 0, hi: int = None) -> H.History:
        """Keys lo .. hi, one row of each key in turn, by Built.round_robin's rule."""
        hi = self.n_keys if hi is None else hi
        return round_robin_of(self.slice(lo, hi), self.off[lo:hi + 1] - self.off[lo])

    def ops(self, k: int) -> list:
        """Key k's unwrapped sub-history as op maps (:index from 0)."""
        lo, hi = int(self.off[k]), int(self.off[k + 1])
        out = [self.hist.sub_op(r) for r in range(lo, hi)]
        for i, o in enumerate(out):
            o["index"] = i
        return out

    def describe(self, k: int) -> str:
        return (f"{self.built.describe(k)} + {self.n_inert} inert ops before row {int(self.at[k])} "
                f"({self.place})")


def widened(built: Built, n_inert: int, place: str) -> Widened:
    return Widened(built, n_inert, place)
