"""The resident set tier's resume rule, restated in Python for the tests
(tests/test_stream_set_rule.py, tests/test_gpu_stream_set.py): "closed start,
then exact JIT".

A key's search is knossos.linear's (oracle/linear_ref.py `analysis`): a config
is (register value, ops linearized and still pending).  At the invoke that
takes the key out of the register tier -- and, to model a lattice that was
closed earlier, at any other invoke the caller names -- the config set S is
replaced by its closure under the ops then pending; every :ok after that is
the oracle's exact step (partition on p, JIT closure over the other pending
ops, apply p).  Ops are named by window slot, a config is (value, slot mask);
the model's step is linear_ref's own, tabulated per op.

Events come from stream_helpers.Restated: (is_ok, slot, (f, v0, v1), row)."""
from __future__ import annotations

import linear_ref as LR
from lincheck import _native as N

REGISTER_SLOTS = 10     # the register tier's reach (csrc/stream_plan.hpp STREAM_MAX_WIDTH)
CAP = 32768             # STREAM_SET_CAP
F_NAME = {N.LC_F_READ: "read", N.LC_F_WRITE: "write", N.LC_F_CAS: "cas"}


def op_value(op):
    f, v0, v1 = op
    nil = lambda v: None if v == N.LC_NIL else v
    return [nil(v0), nil(v1)] if f == N.LC_F_CAS else nil(v0)


class Stepper:
    """linear_ref.cas_register_step of one op, remembered per state."""

    def __init__(self, op):
        self.f, self.value, self.memo = F_NAME[op[0]], op_value(op), {}

    def __call__(self, st):
        if st not in self.memo:
            s2 = LR.cas_register_step(st, self.f, self.value)
            self.memo[st] = (s2 is not LR.INCONSISTENT, s2)
        return self.memo[st]


def close(S, pend, skip=-1):
    """Closure of S under linearizing the pending ops (slot -> Stepper) other than `skip`."""
    out = set(S)
    frontier = list(S)
    qs = [(1 << q, stp) for q, stp in pend.items() if q != skip]
    while frontier:
        nxt = []
        for st, L in frontier:
            for bit, stp in qs:
                if L & bit:
                    continue
                ok, s2 = stp(st)
                if ok:
                    c = (s2, L | bit)
                    if c not in out:
                        out.add(c)
                        nxt.append(c)
        frontier = nxt
    return out


class Run:
    """One key under the rule.  close_at: event ordinals (of invokes) at which S
    is closed besides the leaving invoke.  stop: search no event from there on.
    closed=False: S stays exact at the leaving invoke too (the oracle's own sets:
    the sizes below are then the least any resumed search can have)."""

    def __init__(self, events, close_at=(), stop=None, closed=True):
        self.valid, self.fail_event = True, None
        self.left_at = None            # the invoke that took window slot >= 10
        self.max_s = self.max_i = 0    # largest S' / I at an :ok after leaving
        self.max_pending = 0
        self.closed_size = None        # |S*| at the leaving invoke
        S = {(None, 0)}
        pend = {}
        for ei, (is_ok, slot, op, _row) in enumerate(events):
            if stop is not None and ei >= stop:
                break
            if not is_ok:
                leaving = self.left_at is None and slot >= REGISTER_SLOTS
                if (leaving and closed) or ei in close_at:
                    S = close(S, pend)
                if leaving:
                    self.left_at, self.closed_size = ei, len(S)
                pend[slot] = Stepper(op)
                self.max_pending = max(self.max_pending, len(pend))
                continue
            pbit = 1 << slot
            Sn = {(st, L & ~pbit) for st, L in S if L & pbit}
            I = close({c for c in S if not c[1] & pbit}, pend, skip=slot)
            stp = pend[slot]
            for st, L in I:
                ok, s2 = stp(st)
                if ok:
                    Sn.add((s2, L))
            if self.left_at is not None:
                self.max_s, self.max_i = max(self.max_s, len(Sn)), max(self.max_i, len(I))
            if not Sn:
                self.valid, self.fail_event = False, ei
                break
            S = Sn
            del pend[slot]
        self.S, self.pend = S, pend

    @property
    def falls_back(self):
        return self.max_s > CAP or self.max_i > CAP
