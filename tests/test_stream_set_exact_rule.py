"""The exact set tier's rule on the CPU: tests/stream_set_rule.py's
Run(events, closed=False) -- the oracle's own sets, nothing closed at the
leaving invoke -- extended here with a budget and a peak in the order
csrc/stream_plan.hpp stream_set_exact_decide states (|I| against the budget,
|S'| = 0, |S'| against the budget; the peak moves only past all three), against
the oracle (oracle/linear_ref.c through cref) on every key of "long" that leaves
the register tier: at budget 2^20, and at need - 1 and need, where need is the
least budget at which the oracle decides the key.  This is the rule
k_stream_set_exact must follow; the cap's fallback changes who answers, never
the answer."""
import numpy as np
import pytest

import cref
import stream_helpers as S
import stream_set_rule as R
from lincheck import history as H
from test_stream_set_rule import HISTORIES

NONLIN, BUDGET = 1, 2  # LC_CAUSE_*


class ExactRun:
    """R.Run(events, closed=False) with a budget and a peak: (valid, cause,
    fail_event, peak) as the oracle's record has them, and the largest |I| and
    |S'| met at an :ok from the leaving invoke on (R.Run's falls_back)."""

    def __init__(self, events, budget):
        self.valid, self.cause, self.fail_event, self.peak = 1, 0, -1, 1
        self.left_at, self.max_s, self.max_i = None, 0, 0
        Sset, pend = {(None, 0)}, {}
        for ei, (is_ok, slot, op, _row) in enumerate(events):
            if not is_ok:
                if self.left_at is None and slot >= R.REGISTER_SLOTS:
                    self.left_at = ei
                pend[slot] = R.Stepper(op)
                continue
            pbit = 1 << slot
            Sn = {(st, L & ~pbit) for st, L in Sset if L & pbit}
            I = R.close({c for c in Sset if not c[1] & pbit}, pend, skip=slot)
            for st, L in I:
                ok, s2 = pend[slot](st)
                if ok:
                    Sn.add((s2, L))
            if self.left_at is not None:
                self.max_s, self.max_i = max(self.max_s, len(Sn)), max(self.max_i, len(I))
            if len(I) > budget:
                self.valid, self.cause, self.fail_event = -1, BUDGET, ei
                break
            if not Sn:
                self.valid, self.cause, self.fail_event = 0, NONLIN, ei
                break
            if len(Sn) > budget:
                self.valid, self.cause, self.fail_event = -1, BUDGET, ei
                break
            Sset = Sn
            self.peak = max(self.peak, len(Sn))
            del pend[slot]

    @property
    def record(self):
        return self.valid, self.cause, self.fail_event, self.peak


@pytest.fixture(scope="module")
def long_case():
    h = H.synth(**HISTORIES["long"][0])
    keys, orc = cref.check_history(h.as_c(), budget=1 << 20, threads=8)
    rs = S.Restated(h)
    leaving = [i for i, k in enumerate(keys) if rs.defer_at[k] >= 0]
    assert len(leaving) >= HISTORIES["long"][1]
    return h, list(keys), orc, rs, leaving


def oracle_record(orc, i=0):
    return tuple(int(orc[f][i]) for f in ("valid", "cause", "fail_event", "peak"))


def test_the_rule_gives_the_oracle_s_record_at_the_default_budget(long_case):
    _h, keys, orc, rs, leaving = long_case
    past_cap = []
    for i in leaving:
        run = ExactRun(rs.events[keys[i]], 1 << 20)
        assert run.record == oracle_record(orc, i), f"key {keys[i]}: {run.record}, oracle {oracle_record(orc, i)}"
        assert run.left_at is None or run.left_at == rs.defer_at[keys[i]]
        # the sizes are stream_set_rule's exact ones, so the same keys fall back
        plain = R.Run(rs.events[keys[i]], closed=False)
        assert (run.max_s, run.max_i) == (plain.max_s, plain.max_i)
        if plain.falls_back:
            past_cap.append(keys[i])
    assert past_cap == [8], past_cap


def test_the_rule_meets_every_budget_edge_where_the_oracle_does(long_case):
    h, keys, orc, rs, leaving = long_case
    for i in leaving:
        k = keys[i]
        hk = h.select_keys([k])
        need = cref.need(hk.as_c(), k)
        sI, sS = cref.key_sizes(hk.as_c(), k, budget=1 << 62)
        assert need == max(int(sI.max(initial=1)), int(sS.max(initial=1))) > 1
        first = int(np.flatnonzero((sI > need - 1) | (sS > need - 1))[0])
        for budget in (need - 1, need):
            want = oracle_record(cref.check_history(hk.as_c(), budget=budget, threads=1)[1])
            got = ExactRun(rs.events[k], budget).record
            assert got == want, f"key {k} at budget {budget}: {got}, oracle {want}"
            if budget == need - 1:
                assert got[:3] == (-1, BUDGET, first)
            else:
                assert got == oracle_record(orc, i)  # at need: the unbounded record
