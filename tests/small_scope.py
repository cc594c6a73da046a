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

Every key's peak is at most 11 configs, so all of them live in the register
tier; the set tiers (T1, T2, HBM) are out of these scopes' reach and keep
their own edge suites.

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
READ_VALUES = (0, 1, None)
OPS = {
    "cas-register": [("read", None), ("write", 0), ("write", 1)] + [("cas", (a, b)) for a in VALUES for b in VALUES],
    "register": [("read", None), ("write", 0), ("write", 1)],
    "mutex": [("acquire", None), ("release", None)],
}
PROCS_PER_KEY = 8  # process of key k, enumeration process p: 8 * k + p (a key invokes at most 4 ops)


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
        h = self.hist
        pos = np.arange(len(h), dtype=np.int64) - np.repeat(self.off[:-1], np.diff(self.off))
        perm = np.lexsort((h.key, pos))
        return H.History(h.type[perm], h.f[perm], h.process[perm], h.key[perm], h.v0[perm], h.v1[perm],
                         np.arange(len(perm), dtype=np.int64))

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
