"""Helpers of the stream tests (tests/test_stream_pack.py, tests/test_gpu_stream.py).

`Restated` is the decided-prefix rule of the incremental check (include/
lincheck.h "incremental check") written down a second time, in Python, from
the whole history at once: per key, an invoke row's fate is known at the row
that completes it (:ok, :fail, :info) or supersedes it (the same process
invoking again in the key), else only at `finish`; an event is in the decided
prefix once every invoke row at or before it has its fate.  So each event has
the row count at which it is emitted, and the emitted count after any number
of rows is a bisection -- no incremental state shared with the library's
packer (csrc/host_stream.cpp)."""
from __future__ import annotations

import bisect

import numpy as np

from lincheck import _native as N
from lincheck import history as H

NEVER = 1 << 62  # decided at finish only
CLIENT_F = {0: (N.LC_F_READ, N.LC_F_WRITE, N.LC_F_CAS), 1: (N.LC_F_READ, N.LC_F_WRITE), 2: (N.LC_F_ACQUIRE, N.LC_F_RELEASE)}
MAX_WIDTH, MAX_STATES = 10, 32


class Restated:
    def __init__(self, hist: H.History, model: int = 0):
        t, f, p, k = hist.type.tolist(), hist.f.tolist(), hist.process.tolist(), hist.key.tolist()
        v0, v1 = hist.v0.tolist(), hist.v1.tolist()
        self.keys = []            # order of first appearance
        rows_of = {}
        for r in range(len(t)):
            if k[r] == N.LC_NO_KEY:
                continue
            if p[r] == N.LC_NO_PROCESS and t[r] == N.LC_INFO:
                continue
            if k[r] not in rows_of:
                rows_of[k[r]] = []
                self.keys.append(k[r])
            rows_of[k[r]].append(r)
        self.error = {}           # key -> the row its error shows at
        self.events = {}          # key -> [(is_ok, slot, op triple or None, row)]
        self.ready = {}           # key -> rows appended when event j is emitted (ascending)
        self.items = {}           # key -> [(row, rows appended when it stops being held)] of invoke / :ok rows
        self.defer_at = {}        # key -> event ordinal or -1
        for key in self.keys:
            self._key(key, rows_of[key], t, f, p, v0, v1, model)

    def _key(self, key, rows, t, f, p, v0, v1, model):
        ops = {}                  # invoke row -> [f, v0, v1, fate, decided_at]
        open_of = {}
        ok_of = {}                # :ok row -> invoke row
        err = None
        for r in rows:
            if t[r] == N.LC_INVOKE:
                if f[r] not in CLIENT_F[model]:
                    err = r
                    break
                if p[r] in open_of:
                    o = ops[open_of[p[r]]]
                    o[3], o[4] = "forever", r + 1
                ops[r] = [f[r], v0[r], v1[r], None, NEVER]
                open_of[p[r]] = r
            elif t[r] in (N.LC_OK_T, N.LC_FAIL):
                if p[r] not in open_of:
                    err = r
                    break
                o = ops[open_of.pop(p[r])]
                o[4] = r + 1
                if t[r] == N.LC_OK_T:
                    o[3] = "ok"
                    if o[0] == N.LC_F_CAS:
                        if o[1] == N.LC_NIL and o[2] == N.LC_NIL:
                            o[1], o[2] = v0[r], v1[r]
                    elif o[1] == N.LC_NIL:
                        o[1] = v0[r]
                    ok_of[r] = o
                else:
                    o[3] = "fail"
            elif p[r] in open_of:
                o = ops[open_of.pop(p[r])]
                o[3], o[4] = "forever", r + 1
        if err is not None:
            self.error[key] = err
        ev, ready, items = [], [], []
        block, free, slot_of = 0, list(range(128)), {}
        states = {N.LC_NIL, 1} if model == 2 else {N.LC_NIL}  # mutex: unlocked, locked
        defer = -1
        for r in rows:
            if err is not None and r >= err:
                break
            if t[r] == N.LC_INVOKE:
                o = ops[r]
                block = max(block, o[4])
                items.append((r, block))
                if o[3] == "fail":
                    continue
                s = free.pop(0)
                slot_of[id(o)] = s
                if model != 2:
                    states |= {v for v in ((o[1],) if o[0] != N.LC_F_CAS else (o[1], o[2]))}
                if defer < 0 and (s >= MAX_WIDTH or len(states) > MAX_STATES):
                    defer = len(ev)
                ev.append((False, s, (o[0], o[1], o[2]), r))
                ready.append(block)
            elif r in ok_of:
                o = ok_of[r]
                block = max(block, r + 1)
                items.append((r, block))
                s = slot_of[id(o)]
                bisect.insort(free, s)
                ev.append((True, s, None, r))
                ready.append(block)
        self.events[key], self.ready[key], self.items[key], self.defer_at[key] = ev, ready, items, defer

    def emitted(self, key, n_rows, finished=False) -> int:
        """Events of the key's decided prefix once n_rows rows were appended."""
        if key in self.error and (finished or self.error[key] < n_rows):
            return None  # in error: the count no longer matters
        if finished:
            return len(self.events[key])
        return bisect.bisect_right(self.ready[key], n_rows)

    def held(self, key, n_rows) -> int:
        return sum(1 for r, until in self.items[key] if r < n_rows < until)


def rows(hist: H.History, lo: int, hi: int) -> H.History:
    """Rows lo .. hi of a history, as a history of their own."""
    return H.History(hist.type[lo:hi], hist.f[lo:hi], hist.process[lo:hi], hist.key[lo:hi], hist.v0[lo:hi],
                     hist.v1[lo:hi], hist.index[lo:hi])


def merged_round_robin(hist: H.History) -> H.History:
    """A key-major history's rows, one row of each key in turn."""
    key = hist.key
    order_keys = list(dict.fromkeys(key.tolist()))
    per = {k: np.flatnonzero(key == k) for k in order_keys}
    longest = max(len(v) for v in per.values())
    perm = np.array([per[k][i] for i in range(longest) for k in order_keys if i < len(per[k])], np.int64)
    h = H.History(hist.type[perm], hist.f[perm], hist.process[perm], hist.key[perm], hist.v0[perm], hist.v1[perm],
                  np.arange(len(perm), dtype=np.int64))
    return h


def decode_desc(d: int, state_value):
    """A descriptor as (kind, values): state ids through state_value (None:
    nil); LC_STATE_NONE -- a value no op installs -- as "none"."""
    f, a, b = d & 3, (d >> 2) & 0x7FFF, d >> 17
    sv = lambda s: "none" if s == N.LC_STATE_NONE else state_value(s)
    if f == N.LC_T_READ_ANY:
        return ("read", None)
    if f == N.LC_T_READ:
        return ("read", sv(a))
    if f == N.LC_T_WRITE:
        return ("write", sv(b))
    return ("cas", sv(a), sv(b))


def same_op(stream_op, packed_op, installed) -> bool:
    """The stream's decoded descriptor against lc_pack's: equal, or lc_pack
    names a value nothing in the batch installs ("none") where the stream,
    which interns every value an op names, names a value the key never
    installs."""
    if stream_op[0] != packed_op[0] or len(stream_op) != len(packed_op):
        return False
    for a, b in zip(stream_op[1:], packed_op[1:]):
        if a != b and not (b == "none" and a not in installed):
            return False
    return True


def compare_with_packed(stream, pk, restated=None):
    """Every key's final words against lc_pack's: ok bits, slots, descriptors
    decoded to register values; event rows too."""
    assert stream.keys == pk.keys
    for i, key in enumerate(pk.keys):
        if pk.key_error(i) is not None:
            assert stream.key_error(i) is not None, f"key {key}: lc_pack refuses it, the stream does not"
            continue
        assert stream.key_error(i) is None, f"key {key}: {stream.key_error(i)}"
        w, e = stream.words(i), pk.events(i)
        assert len(w) == len(e), f"key {key}: {len(w)} words, lc_pack {len(e)}"
        assert np.array_equal(w >> 24, e >> 24), f"key {key}: ok bits or slots differ"
        tr = stream.trans(i)
        inv = np.flatnonzero((e >> 31) == 0)
        ops_s = [decode_desc(int(tr[int(w[j]) & 0xFFFFFF]), lambda s: stream.state_value(i, s)) for j in inv]
        ops_p = [decode_desc(pk.desc(i, int(e[j]) & 0xFFFFFF), lambda s: pk.state_value(i, s)) for j in inv]
        installed = {o[-1] for o in ops_s if o[0] in ("write", "cas")}
        for j, a, b in zip(inv, ops_s, ops_p):
            assert same_op(a, b, installed), f"key {key}, event {j}: stream {a}, lc_pack {b}"
        for j in (0, len(e) // 2, len(e) - 1):
            if 0 <= j < len(e):
                assert stream.event_row(i, j) == pk.event_row(i, j)


def feed(stream, hist: H.History, step: int, after=None):
    """Append hist `step` rows at a time; after(n_rows, update) follows each call."""
    n = len(hist)
    for lo in range(0, n, step):
        hi = min(n, lo + step)
        up = stream.append(rows(hist, lo, hi))
        if after is not None:
            after(hi, up)
