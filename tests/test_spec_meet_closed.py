"""k_spec's meeting test by set size and its closed sets at 7-10 ops pending,
on the lane-level model (emu_spec): no GPU.

Meeting by size: a segment's TOP run and its true run (from the set the
walk before it ended with) use one op-index assignment, the TOP run starts
from a superset, and the :ok transfer and the closure are monotone, so after
every lane-phase :ok the TOP lattice contains the true one bit by bit -- and
two nested sets are equal exactly when they have as many configs.

Closed dense sets: "close if dirty, project on p, relocate last" at 7-10
pending gives the verdicts and failing events of the exact :oks, and the
closed set on return to 6 pending that the exact walk's forced re-closure
gives."""
import copy
import os

import numpy as np
import pytest

import cref
import edgegen
import emu_spec as S
from lincheck import history as H
from lincheck.checker import Packed

# C2- and C5-shaped keys (concurrency 10, cas-register values 0..4), short
# enough for the lane-level model, with crashed ops (they keep their slots:
# 7-10 pending occurs) and a short think time (more ops in flight)
SHAPES = {
    "c2": dict(n_keys=2, ops_per_key=160, concurrency=10, info_rate=0.01, mean_think=0.5),
    "c5": dict(n_keys=2, ops_per_key=160, concurrency=10, info_rate=0.01, mean_think=0.5, anomaly_rate=0.5),
}
SEEDS = (2, 5, 11, 12, 13, 14)
AFTER_CUT = 64  # events both runs walk past a cut (runs meet within 25 on C2-shaped keys)


class _Trans:
    def __init__(self, pk, k):
        self.pk, self.k = pk, k

    def __getitem__(self, t):
        return self.pk.desc(self.k, int(t))


@pytest.fixture(scope="module")
def walked():
    """Every key walked once: (shape, seed, key, oracle verdict, exact walk, closed walk, per-cut run pairs)."""
    out = []
    for shape, kw in SHAPES.items():
        for seed in SEEDS:
            h = H.synth(seed=seed, **kw)
            pk = Packed(h)
            _, orc = cref.check_history(h.as_c(), budget=1 << 20, threads=4)
            nstates = edgegen.batch_states(pk)
            for k in range(pk.n_keys):
                ev, tr = pk.events(k), _Trans(pk, k)
                nev = len(ev)
                init = S.State()
                init.W0[0] = 1 << int(pk.view.init_state)
                whole = {}
                for closed in (False, True):
                    whole[closed] = S.walk(ev, tr, 0, nev, copy.deepcopy(init), closed)
                if whole[True][0] == 3 and whole[False][0] == 3:
                    continue  # more than 10 ops pending: not the register tier's key
                # the true run segment by segment, a TOP run and a true run past each cut
                c = edgegen.pending_before(pk, k)
                # cuts: k_spec's own, and every further boundary with at most 6
                # ops pending that lies 48 events past the last one
                cuts = sorted({x for x in edgegen.spec_cuts(c, nev, 8) if x is not None})
                for b in range(16, nev - 16):
                    if c[b] <= edgegen.SPEC_MAX_PEND and all(abs(b - x) >= 48 for x in cuts):
                        cuts.append(b)
                cuts.sort()
                pairs, st, at = [], copy.deepcopy(init), 0
                for cut in cuts:
                    status, _, _ = S.walk(ev, tr, at, cut, st, True)
                    if status:
                        break
                    at = cut
                    end = min(nev, cut + AFTER_CUT)
                    top = S.walk(ev, tr, cut, end, S.start_top(ev, tr, cut, int(nstates[k])), True)
                    true = S.walk(ev, tr, cut, end, S.start_from(ev, tr, cut, st), True)
                    pairs.append((cut, top, true))
                out.append((shape, seed, k, (int(orc["valid"][k]), int(orc["fail_event"][k])), whole[False],
                            whole[True], pairs, c))
    return out


def test_meeting_wait_keeps_a_fixed_trip_count():
    """tests/test_kernel_lint.py's rules for the LDS-flag waits, on the new one
    (spec_meet_entry): one loop, a fixed trip count, every flag read a spec_load."""
    import re
    from test_kernel_lint import CSRC, OPEN_LOOP, _body, _code
    src = _code(open(os.path.join(CSRC, "device_spec.hip")).read())
    body = _body(src, "__device__ __forceinline__ int32_t spec_meet_entry(")
    assert not re.search(OPEN_LOOP, body)
    assert len(re.findall(r"\b(for|while|do)\b", body)) == 1
    at = re.search(r"for \(uint32_t it = 0; it < SPEC_WAIT_MAX; \+\+it\) ", body)
    assert at, "the wait lost its fixed trip count"
    rest, n_loads = re.subn(r"\bspec_load\([^()]*\)", "", _body(body[at.start():], at.group(0)))
    assert n_loads >= 2 and "__hip_atomic_load" not in rest
    for flag in ("mt", "top_done"):
        assert not re.search(r"\b%s\b" % flag, rest), f"{flag} read without spec_load"


def test_batches_cover_the_dense_phase(walked):
    """:oks at 7, 8, 9 and 10 pending, clean ones (no invoke since the last :ok) among them."""
    seen, clean = set(), 0
    for _shape, _seed, _k, _orc, _exact, closed, _pairs, c in walked:
        oks = closed[2]
        for i, (j, n, _w, _b) in enumerate(oks):
            seen.add(n)
            if n >= 7 and i > 0 and oks[i - 1][0] == j - 1:
                clean += 1
    assert {7, 8, 9, 10} <= seen, sorted(seen)
    assert clean > 0
    assert len({seed for _s, seed, *_ in walked}) >= 6 and len(walked) >= 16


def test_closed_dense_oks_give_the_exact_verdicts(walked):
    for shape, seed, k, orc, exact, closed, _pairs, _c in walked:
        what = f"{shape} seed {seed} key {k}"
        assert exact[0] != 3 and closed[0] != 3, what
        for name, w in (("exact", exact), ("closed", closed)):
            got = (0, w[1]) if w[0] == 1 else (1, -1)
            assert got == orc, f"{what}: {name} dense :oks give {got}, the oracle {orc}"
        assert len(exact[2]) == len(closed[2]), what
        for (j0, n0, w0, b0), (j1, n1, w1, b1) in zip(exact[2], closed[2]):
            assert (j0, n0) == (j1, n1), what
            if w0 is not None:  # a lane-phase :ok: the canonical closed set
                assert np.array_equal(w0, w1), f"{what}: sets differ after the :ok at event {j0}"
            if b0 is not None:  # back at 6 pending
                assert np.array_equal(b1[0], b1[1]), f"{what}: event {j0}: the closed walk's set is not closed"
                assert np.array_equal(b0[1], b1[0]), f"{what}: event {j0}: closed sets differ on return to 6 pending"


def test_top_run_contains_the_true_run_and_counts_tell_equality(walked):
    n_pairs = met_early = 0
    for shape, seed, k, _orc, _exact, _closed, pairs, _c in walked:
        for cut, top, true in pairs:
            what = f"{shape} seed {seed} key {k} cut {cut}"
            n_pairs += 1
            # a superset dies no earlier
            if top[0] == 1:
                assert true[0] == 1 and true[1] <= top[1], what
            met = None
            for i, ((jt, nt, wt, _bt), (jr, nr, wr, _br)) in enumerate(zip(top[2], true[2])):
                assert (jt, nt) == (jr, nr), what
                if wt is None:
                    continue  # a dense-phase :ok: no compare
                assert np.array_equal(wt & wr, wr), f"{what}: event {jt}: the TOP set does not contain the true set"
                same = np.array_equal(wt, wr)
                assert (S.popc(wt) == S.popc(wr)) == same, f"{what}: event {jt}: counts {S.popc(wt)}, {S.popc(wr)}"
                assert S.popc(wt) <= 2048
                if met is not None:
                    assert same, f"{what}: event {jt}: runs that met at {met} differ again"
                elif same:
                    met = jt
                    met_early += i < 16
    assert n_pairs >= 12
    assert met_early >= n_pairs // 2, (met_early, n_pairs)  # (most pairs meet within the ring's 16 :oks)
