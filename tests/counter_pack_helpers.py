"""What the tests of lc_counter_check_history share: lc_counter_pack's serial
fold restated LOCALLY, the way the device builds the batch,
raw-column generators, and the host path's answer (lc_counter_pack +
lc_counter_check_host) as plain arrays.

local_pack restates csrc/counter_pack_plan.hpp's claim in plain Python: with a
key's client rows grouped by process in history order, every row judges itself
from the row before it in its group and knows what it yields from the row after
it; the key's error is the offence at its lowest row; rule 3 is the first
offence among the surviving add events.  tests/test_counter_pack_local.py holds
it against lc_counter_pack on the CPU; the kernels rest on the same claim."""
import itertools
import random

import numpy as np

from lincheck import _native as N
from lincheck import counter as CT

INVOKE, OK, FAIL, INFO = N.LC_INVOKE, N.LC_OK_T, N.LC_FAIL, N.LC_INFO
ADD, READ, OTHER = N.LC_CF_ADD, N.LC_CF_READ, N.LC_CF_OTHER
NIL = N.LC_NIL
I64_MAX = (1 << 63) - 1

SECOND_INVOKE = "a second invocation by a process that has one open"
NO_OPEN = "a completion by a process with no open invocation"
OTHER_F = "a completion whose :f is not its invocation's"
READ_NIL = "an :ok :read whose value is nil or not an integer"
ADD_NIL = "an :add whose value is nil or not an integer"
ADD_NEGATIVE = "an :add of a negative value"
SUM = "the adds sum past the largest 64-bit integer"
MESSAGES = (SECOND_INVOKE, NO_OPEN, OTHER_F, READ_NIL, ADD_NIL, ADD_NEGATIVE, SUM)


def hist(rows, keyed=True, with_process=True):
    """rows: (type, f, process, key, value) tuples; None is the sentinel of its column."""
    t = [r[0] for r in rows]
    f = [r[1] for r in rows]
    p = [NIL if r[2] is None else r[2] for r in rows]
    k = [NIL if r[3] is None else r[3] for r in rows]
    v = [NIL if r[4] is None else r[4] for r in rows]
    return CT.CounterHistory(np.array(t, np.uint8), np.array(f, np.uint8), np.array(p, np.int64) if with_process else None,
                             np.array(k, np.int64) if keyed else None, np.array(v, np.int64))


def local_pack(h):
    """The batch of CounterHistory h by the local rules.  Returns PackedCounter.arrays()'s
    names plus keys, error (text or None per key) and error_row."""
    n = h.n
    proc = h.process if h.process is not None else np.zeros(n, np.int64)
    keyed = h.key is not None and bool((h.key != NIL).any())
    keys, index = [], {}
    if keyed:
        for r in range(n):
            k = int(h.key[r])
            if k != NIL and k not in index:
                index[k] = len(keys)
                keys.append(k)
    else:
        keys = [NIL]
    K = len(keys)
    groups = {}
    for r in range(n):
        if h.f[r] == OTHER or proc[r] == NIL or (keyed and h.key[r] == NIL):
            continue
        ki = index[int(h.key[r])] if keyed else 0
        groups.setdefault((ki, int(proc[r])), []).append(r)
    err1 = [None] * K      # (row, text), the lowest
    event = {}             # row -> [kind, value]; an RINV's value: the row of its :ok
    for (ki, _), rows in groups.items():
        for i, r in enumerate(rows):
            pr = rows[i - 1] if i else None
            nx = rows[i + 1] if i + 1 < len(rows) else None
            t, f, v = int(h.type[r]), int(h.f[r]), int(h.value[r])
            why = None
            if t == INVOKE:
                if pr is not None and h.type[pr] == INVOKE:
                    why = SECOND_INVOKE
                tn = int(h.type[nx]) if nx is not None else INVOKE
                if f == ADD:
                    if tn != FAIL:
                        event[r] = [N.LC_CE_UP, int(h.value[nx]) if tn == OK else v]
                elif tn == OK:
                    event[r] = [N.LC_CE_RINV, nx]
            else:
                if pr is None or h.type[pr] != INVOKE:
                    why = NO_OPEN
                elif h.f[pr] != f:
                    why = OTHER_F
                elif f == READ and t == OK and v == NIL:
                    why = READ_NIL
                if t == OK:
                    event[r] = [N.LC_CE_LOW if f == ADD else N.LC_CE_ROK, v]
            if why and (err1[ki] is None or r < err1[ki][0]):
                err1[ki] = (r, why)
    key_of = {}
    for (ki, _), rows in groups.items():
        for r in rows:
            key_of[r] = ki
    per_key = [[] for _ in range(K)]
    for r in sorted(event):
        per_key[key_of[r]].append(r)
    err = list(err1)
    for ki in range(K):
        if err[ki] is not None:
            continue
        up = 0
        for r in per_key[ki]:
            kind, v = event[r]
            if kind not in (N.LC_CE_UP, N.LC_CE_LOW):
                continue
            why = None
            if v == NIL:
                why = ADD_NIL
            elif v < 0:
                why = ADD_NEGATIVE
            elif kind == N.LC_CE_UP:
                up += v
                if up > I64_MAX:
                    why = SUM
            if why:
                err[ki] = (r, why)
                break
    ev_off, read_off, ev_kind, ev_val, read_val = [0], [0], [], [], []
    for ki in range(K):
        if err[ki] is None:
            number = {}
            for r in per_key[ki]:
                if event[r][0] == N.LC_CE_ROK:
                    number[r] = len(read_val)
                    read_val.append(event[r][1])
            for r in per_key[ki]:
                kind, v = event[r]
                ev_kind.append(kind)
                ev_val.append(number[v] if kind == N.LC_CE_RINV else number[r] if kind == N.LC_CE_ROK else v)
        ev_off.append(len(ev_kind))
        read_off.append(len(read_val))
    return dict(keys=[None if k == NIL else k for k in keys], error=[e and e[1] for e in err], error_row=[-1 if e is None else e[0] for e in err],
                ev_off=np.array(ev_off, np.uint64), ev_kind=np.array(ev_kind, np.uint8), ev_val=np.array(ev_val, np.int64),
                read_off=np.array(read_off, np.uint64), read_val=np.array(read_val, np.int64),
                status=np.array([e is not None for e in err], np.uint8))


BATCH = ("ev_off", "ev_kind", "ev_val", "read_off", "read_val", "status")
RESULT = ("valid", "n_errors", "lower", "upper", "err_off", "err_idx")


def host_pack(h):
    """lc_counter_pack's answer in local_pack's shape (no error_row: the host keeps none)."""
    p = CT.PackedCounter(h)
    out = p.arrays()
    out["keys"] = p.keys
    out["error"] = [p.key_error(i) for i in range(p.n_keys)]
    return out, p


def host_answer(h):
    """lc_counter_pack + lc_counter_check_host: the batch and the results, array by array."""
    out, p = host_pack(h)
    res = CT.check_batch(None, p.view, host=True, err_cap=max(p.n_reads, 1))
    for name in RESULT:
        out[name] = getattr(res, name)
    return out, p, res


def same_batch(got, want, names=BATCH + ("keys", "error")):
    for name in names:
        g, w = got[name], want[name]
        if isinstance(w, np.ndarray):
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (name, g[:16], w[:16])
        else:
            assert g == w, (name, g, w)


# ---- generators of raw columns ------------------------------------------------------------------

VALUES = (None, -1, 0, 1, 2, 7, I64_MAX, I64_MAX // 2 + 1)


def random_rows(rng, n_rows, n_keys, n_procs, p_wild=0.05, p_other=0.05, values=VALUES):
    """Rows of well-paired operations on n_procs processes over n_keys keys (0: no
    key column's worth: every key None), with at p_wild per row a row drawn blind
    (any type, any f, any value), which is what makes offences.  p_wild = 0 gives
    a history without a rule-1 offence."""
    open_ = {}
    rows = []
    keys = list(range(n_keys)) or [None]
    for _ in range(n_rows):
        k = rng.choice(keys)
        p = rng.randrange(n_procs)
        u = rng.random()
        if u < p_other:
            rows.append((rng.choice((INVOKE, OK, FAIL, INFO)), OTHER, rng.choice((None, p)), rng.choice((None, k)), None))
            continue
        if u < p_other + p_wild:
            rows.append((rng.choice((INVOKE, OK, FAIL, INFO)), rng.choice((ADD, READ)), p, k, rng.choice(values)))
            open_.pop((k, p), None)
            continue
        if (k, p) in open_:
            f, v = open_.pop((k, p))
            t = rng.choice((OK, OK, OK, FAIL, INFO))
            rows.append((t, f, p, k, v if f == ADD else rng.randrange(0, 20) if t == OK else None))
        else:
            f = rng.choice((ADD, READ))
            v = rng.randrange(0, 6) if f == ADD else None
            open_[(k, p)] = (f, v)
            rows.append((INVOKE, f, p, k, v))
    return rows


SMALL_ALPHABET = list(itertools.product((INVOKE, OK, FAIL, INFO), (ADD, READ), (0, 1), (None,), (None, -1, 1)))


def small_history(n_rows, index):
    """History number `index` of the len(SMALL_ALPHABET) ** n_rows histories of n_rows client rows
    over 2 processes x {add, read} x 4 types x values {nil, -1, 1}, one key."""
    rows = []
    for _ in range(n_rows):
        index, d = divmod(index, len(SMALL_ALPHABET))
        rows.append(SMALL_ALPHABET[d])
    return rows


def rng_of(seed):
    return random.Random(seed)
