"""A check on the checker: the batches of tests/edgegen.py that
test_gpu_register_edges.py runs on the device are what they are built to be.
Everything here comes from the packed event words, the restated constants and
the C oracle (no GPU): event counts, the pending count at every cut window,
the kept cuts, the oracle's failing event at every directed anomaly -- so a
later change to a kernel constant or to the generator cannot quietly turn the
edge cases into ordinary ones.  The constants themselves are compared with
the sources they cite."""
import os
import re

import numpy as np
import pytest

import cref
import edgegen as E
import emu_t0
from lincheck import _native as N
from lincheck import history as H
from lincheck.checker import Packed

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "jepsen-etcd-demo_amd", "csrc")
_orc = {}


def oracle(name):
    if name not in _orc:
        b = E.get(name)
        keys, orc = cref.check_history(b.hist.as_c(), budget=1 << 20, threads=8)
        assert list(keys) == b.pk.keys
        _orc[name] = orc
    return _orc[name]


def pending(b, name):
    return E.pending_before(b.pk, b.index(name)).tolist()


def oks(b, name):
    """Events of the key that are :oks, from the packed words."""
    return np.flatnonzero(b.pk.events(b.index(name)) >> 31).tolist()


# ---------------------------------------------------------------- the constants
@pytest.mark.parametrize("file,pattern,value", [
    ("device_spec.hip", r"constexpr uint32_t SPEC_MIN_LEN = (\d+);", E.SPEC_MIN_LEN),
    ("device_spec.hip", r"constexpr uint32_t SPEC_MAX_PEND = (\d+);", E.SPEC_MAX_PEND),
    ("lattice_core.hpp", r"#define LC_T0_MAX_WIDTH (\d+)", E.T0_MAX_WIDTH),
    ("lattice_core.hpp", r"constexpr uint32_t T0_MAX_STATES = (\d+);", E.T0_MAX_STATES),
    ("device_spec.hip", r"spec_ev_lds\(\) \{ return .* \? (\d+)u : \d+u\) : 0u; \}", E.SPEC_EV_LDS[0]),
    ("device_spec.hip", r"spec_ev_lds\(\) \{ return .* \? \d+u : (\d+)u\) : 0u; \}", E.SPEC_EV_LDS[1]),
    ("device_spec.hip", r"SPEC_W_EV = (\d+), SPEC_W_MID = \d+, SPEC_W_HEAVY = \d+;", E.SPEC_W_EV),
    ("device_spec.hip", r"SPEC_W_EV = \d+, SPEC_W_MID = (\d+), SPEC_W_HEAVY = \d+;", E.SPEC_W_MID),
    ("device_spec.hip", r"SPEC_W_EV = \d+, SPEC_W_MID = \d+, SPEC_W_HEAVY = (\d+);", E.SPEC_W_HEAVY),
    ("device_spec.hip", r"of the boundaries t\s*\n?//\s*\.\. t \+ (\d+) ", E.SPEC_CUT_WINDOW),
    ("device_api.hip", r"l\.ck1 = o\.spec_ck \? .* : (\d+)u;", E.SPEC_CK_DEFAULT[0]),
    ("device_api.hip", r"l\.ck2 = o\.spec_ck \? .* : (\d+)u;", E.SPEC_CK_DEFAULT[1]),
    ("device_api.hip", r"s\.taggable = !b->trans_off && s\.shared_states <= (\d+) ", E.TAGGABLE_MAX_STATES),
])
def test_restated_constant(file, pattern, value):
    """The constants the cases are placed by are the sources'."""
    src = open(os.path.join(CSRC, file)).read()
    m = re.search(pattern, src)
    assert m, f"{file}: {pattern!r} not found (the restated constant has lost its source)"
    assert int(m.group(1)) == value


def test_restated_segment_rules():
    """eff, the equal-count targets and the cut window as the kernel states them."""
    src = open(os.path.join(CSRC, "device_spec.hip")).read()
    assert "nev < 2 * SPEC_MIN_LEN;" in src and "min((uint32_t)S, nev / SPEC_MIN_LEN)" in src
    assert "const uint32_t t = (uint32_t)((uint64_t)nev * s / eff);" in src
    assert "if (c2 >= 0 && c2 <= last) c2 = -1;" in src
    assert E.spec_eff(255, 8) == 1 and E.spec_eff(256, 8) == 2 and E.spec_eff(1024, 8) == 8 and E.spec_eff(4097, 4) == 4
    assert E.spec_targets(1024, 8) == [128 * s for s in range(1, 8)] == E.TARGETS
    assert list(E.cut_window(128)) == list(range(128, 193))


# ---------------------------------------------------------------- every batch
@pytest.mark.parametrize("name", sorted(E.BATCHES))
def test_batch_counts_and_verdicts(name):
    """Every key packs to its stated event count and pending counts; the
    oracle fails each anomalous key at its (earliest) directed anomaly, finds
    every other key valid and ends none on the budget; both verdicts occur."""
    b = E.get(name)
    orc = oracle(name)
    assert (orc["valid"] != N.LC_UNKNOWN).all(), "a key ended on the budget"
    assert (orc["valid"] == 1).any() and (orc["valid"] == 0).any()
    for i, (case, plan) in enumerate(zip(b.names, b.plans)):
        assert b.pk.n_events(i) == plan.nev, case
        assert E.pending_before(b.pk, i).tolist() == plan.c, case
        assert orc["n_events"][i] == plan.nev or not orc["valid"][i], case
        if not b.anomalies[i]:
            assert orc["valid"][i] == 1 and orc["fail_event"][i] == -1, case
            continue
        ev = b.pk.events(i)
        assert all(ev[e] >> 31 for e in b.anomalies[i]), f"{case}: an anomaly is not at an :ok"
        assert orc["valid"][i] == 0 and orc["fail_event"][i] == min(b.anomalies[i]), case
        if len(b.anomalies[i]) > 1:
            assert sorted(set(b.anomalies[i])) == sorted(b.anomalies[i]), case
            assert orc["fail_event"][i] != max(b.anomalies[i]), case


# ---------------------------------------------------------------- (a), (b)
def test_ragged_lengths_and_places():
    """(a): lengths on both sides of nev < 2 * SPEC_MIN_LEN, of eff = nev /
    SPEC_MIN_LEN, of the 64-event chunks and of both spec_ev_lds() sizes; the
    first and the last :ok fail; empty and one-event keys first, mid, last."""
    b = E.get("ragged")
    want = [0, 1, 2] + [L + d for L in (64, 128, 256, 384, 512, 768, 1024) + E.SPEC_EV_LDS for d in (-1, 0, 1)]
    assert E.RAGGED_LENGTHS == want
    assert {2 * E.SPEC_MIN_LEN - 1, 2 * E.SPEC_MIN_LEN} <= set(want)
    for nev in want:
        i = b.index(f"len{nev}-valid")
        assert b.pk.n_events(i) == nev
        if nev < 2:
            continue
        if nev > 2:
            assert 3 <= max(b.plans[i].c) <= 6  # concurrency 3-6: every boundary could be a cut (SPEC_MAX_PEND)
        assert b.anomalies[b.index(f"len{nev}-first_ok")] == [oks(b, f"len{nev}-first_ok")[0]]
        assert b.anomalies[b.index(f"len{nev}-last_ok")] == [oks(b, f"len{nev}-last_ok")[-1]]
        assert oks(b, f"len{nev}-last_ok")[-1] == nev - 1
    n = len(b.names)
    assert b.names[:2] == ["empty-first", "one-first"] and b.names[-2:] == ["empty-last", "one-last"]
    assert n // 3 < b.index("empty-mid") < 2 * n // 3 and b.index("one-mid") == b.index("empty-mid") + 1
    for place in ("first", "mid", "last"):
        assert b.pk.n_events(b.index(f"empty-{place}")) == 0 and b.pk.n_events(b.index(f"one-{place}")) == 1


def test_compact_is_past_the_wide_build():
    """(b): more keys than the 16-register build holds (step_plan.hpp:134,
    t0_wide = K <= cu_count * 8 with 256 CUs), (a)'s keys among them."""
    b = E.get("compact")
    assert "p.t0_wide = K <= (int64_t)in.cu_count * 8;" in open(os.path.join(CSRC, "step_plan.hpp")).read()
    assert b.pk.n_keys == 2600 > 256 * 8
    a = E.get("ragged")
    assert b.names[:len(a.names)] == a.names
    assert all(2 <= p.nev <= 6 for p in b.plans[len(a.names):])


# ---------------------------------------------------------------- (c)
NO_CUT = [None] * 7


def only(s, cut):
    return [cut if q == s else None for q in range(1, 8)]


# the kept cuts of segments 1..7 at 8 segments (targets 128 s, windows 128 s .. 128 s + 64)
PROFILE_CUTS = {
    "rolling7": NO_CUT, "rolling8": NO_CUT, "rolling9": NO_CUT, "rolling10": NO_CUT,
    "rolling7_touching6": E.TARGETS,
    # a dip to d asked for at an odd distance in parity lies one boundary later (edgegen.dip_boundary)
    "dip0_at+0": only(5, 640), "dip0_at+32": only(5, 672), "dip0_at+64": only(5, 704),
    "dip0_at+65": only(5, 704),   # the dip is at 706; its flank has 2 pending at the window's last boundary
    "dip3_at+0": only(5, 641), "dip3_at+32": only(5, 673),
    "dip3_at+64": only(5, 704),   # the dip is at 705: 4 pending at the window's last boundary
    "dip3_at+65": only(5, 704),
    "dip6_at+0": only(5, 640), "dip6_at+32": only(5, 672),
    "dip6_at+64": only(5, 704),   # the window's last boundary
    "dip6_at+65": NO_CUT,         # the dip is at 706, past the window
    "dip7_at+0": NO_CUT, "dip7_at+32": NO_CUT, "dip7_at+64": NO_CUT, "dip7_at+65": NO_CUT,  # 7 > SPEC_MAX_PEND
    "dip6_every_target": E.TARGETS,
    "burst_same_boundary": [128, 256, 384, 526, 640, 768, 896],
    "long_lived_slot0": E.TARGETS, "long_lived_slot9": E.TARGETS, "crashed_write_read_late": E.TARGETS,
}


def test_profile_names():
    b = E.get("profiles")
    assert sorted(b.names) == sorted(f"{p}-{v}" for p in PROFILE_CUTS for v in ("valid", "garbage_seg5"))


@pytest.mark.parametrize("profile", sorted(PROFILE_CUTS))
def test_profile_cuts(profile):
    """The cuts spec_cut_at would keep (SPEC_MAX_PEND, the 65-boundary window,
    the earliest minimum), from the packed words; the garbage read lies in
    segment 5."""
    b = E.get("profiles")
    for v in ("valid", "garbage_seg5"):
        c = pending(b, f"{profile}-{v}")
        assert len(c) == E.NEV + 1
        assert E.spec_cuts(c, E.NEV, 8) == PROFILE_CUTS[profile]
        assert max(c) <= E.T0_MAX_WIDTH
    cuts = [0] + [x for x in PROFILE_CUTS[profile] if x is not None] + [E.NEV]
    (bad,) = b.anomalies[b.index(f"{profile}-garbage_seg5")]
    assert 5 * 128 + E.SPEC_CUT_WINDOW < bad < 6 * 128, "past every cut of segment 5, before every cut of segment 6"
    assert max(x for x in cuts if x <= bad) in (0, PROFILE_CUTS[profile][4])


@pytest.mark.parametrize("P", [7, 8, 9, 10])
def test_rolling_never_cuts(P):
    """rolling(P): never below 7 > SPEC_MAX_PEND anywhere past warm-up, P
    pending at every other boundary; P = 10 = T0_MAX_WIDTH: :oks at 9 and 10."""
    c = pending(E.get("profiles"), f"rolling{P}-valid")
    warm = c.index(max(c))
    assert min(c[warm:]) >= 7 > E.SPEC_MAX_PEND
    assert set(c[warm:]) == ({7, 8} if P == 7 else {P - 1, P})
    assert all(E.spec_cut(c, E.NEV, t) is None for t in range(warm, E.NEV))


def test_rolling7_complete_first_touches_six():
    c = pending(E.get("profiles"), "rolling7_touching6-valid")
    assert set(c[7:]) == {6, 7} and all(c[t] == E.SPEC_MAX_PEND for t in E.TARGETS)


@pytest.mark.parametrize("d,off,at,n_at", [
    (0, 0, 640, 0), (0, 32, 672, 0), (0, 64, 704, 0), (0, 65, 706, 0),
    (3, 0, 641, 3), (3, 32, 673, 3), (3, 64, 705, 3), (3, 65, 705, 3),
    (6, 0, 640, 6), (6, 32, 672, 6), (6, 64, 704, 6), (6, 65, 706, 6),
    (7, 0, 641, 7), (7, 32, 673, 7), (7, 64, 705, 7), (7, 65, 705, 7),
])
def test_dip_windows(d, off, at, n_at):
    """dips(10, d, target + off): d pending at `at` and only there; 9-10
    pending outside the dip; what the window of target 640 holds."""
    c = pending(E.get("profiles"), f"dip{d}_at+{off}-valid")
    assert c[at] == n_at and [x for x in range(20, E.NEV - 20) if c[x] <= d] == [at]
    assert all(c[x] >= 9 for x in range(20, E.NEV - 20) if abs(x - at) > 10 - d)
    w = [c[x] for x in E.cut_window(E.DIP_TARGET)]
    if d == 6 and off == 64:
        assert min(w) == E.SPEC_MAX_PEND and w.index(min(w)) == E.SPEC_CUT_WINDOW and w.count(6) == 1
    if d == 7 or (d == 6 and off == 65):
        assert min(w) > E.SPEC_MAX_PEND
    if d < 6 and off >= 64:
        assert w.index(min(w)) == E.SPEC_CUT_WINDOW and min(w) == d + (at - 704)


@pytest.mark.parametrize("segs", [2, 4, 8])
def test_every_segment_has_heavy_oks(segs):
    """dips(10, 6, every target): a cut with SPEC_MAX_PEND pending at every
    target of 2, 4 and 8 segments, and :oks with 9 and with 10 pending in
    every segment (the 9-10-pending workspaces, spec_lds_ws: fewer than
    waves)."""
    b = E.get("profiles")
    c = pending(b, "dip6_every_target-valid")
    ok = set(oks(b, "dip6_every_target-valid"))
    cuts = E.spec_cuts(c, E.NEV, segs)
    assert cuts == E.spec_targets(E.NEV, segs) and all(c[x] == E.SPEC_MAX_PEND for x in cuts)
    edges = [0] + cuts + [E.NEV]
    for lo, hi in zip(edges, edges[1:]):
        for n in (9, 10):
            assert sum(1 for e in range(lo, hi) if e in ok and c[e] == n) >= 10, f"segment {lo}..{hi}: :oks at {n}"


def test_burst_drops_a_cut():
    """Equal-cost targets (LC_PATH_SPEC_COST, 4 segments) 2 and 3 lie in the
    burst of 9-10-pending :oks and find the same boundary right after it: the
    second cut is at the last kept one and is dropped (device_spec.hip k_spec)."""
    c = pending(E.get("profiles"), "burst_same_boundary-valid")
    t = E.spec_targets_cost(c, E.NEV, 4)
    assert len(t) == 3 and t[2] - t[1] < E.SPEC_CUT_WINDOW
    assert [E.spec_cut(c, E.NEV, x) for x in t] == [None, 526, 526]
    t8 = E.spec_targets_cost(c, E.NEV, 8)
    found = [E.spec_cut(c, E.NEV, x) for x in t8]
    assert found.count(526) >= 2


@pytest.mark.parametrize("profile,slot", [("long_lived_slot0", 0), ("long_lived_slot9", 9),
                                          ("crashed_write_read_late", 3)])
def test_long_lived_op_is_pending_at_every_cut(profile, slot):
    """The op in `slot` is invoked during warm-up (slot 0: event 0) and returns
    at the key's last event (crashed: never), so spec_pending walks back from
    every cut to the key's first chunk for it."""
    b = E.get("profiles")
    for v in ("valid", "garbage_seg5"):
        ev = b.pk.events(b.index(f"{profile}-{v}"))
        mine = [j for j in range(len(ev)) if ((int(ev[j]) >> 24) & 0x7F) == slot]
        assert mine[0] == slot and not ev[slot] >> 31
        desc = b.pk.desc(b.index(f"{profile}-{v}"), int(ev[slot]) & 0xFFFFFF)
        assert desc & 3 == N.LC_T_WRITE
        if profile.startswith("long"):
            assert mine == [slot, E.NEV - 1] and ev[E.NEV - 1] >> 31
        else:
            assert mine == [slot]
    rows = [op for op in b.hist.to_ops() if op["value"][0] == b.index("crashed_write_read_late-valid")]
    info = [op for op in rows if op["type"] == "info"]
    assert len(info) == 1 and info[0]["f"] == "write"


# ---------------------------------------------------------------- (d)
def test_anomaly_places():
    """(d): the cuts are the quiescent points (0 pending at every target, so
    spec_cut_at keeps the target itself, and a write precedes each: the
    cuts of k_search_segments too); each failing :ok is where its name says,
    against the cut at 512 and the default checkpoints."""
    for name in ("anomalies", "values5", "values6"):
        b = E.get(name)
        ck1, ck2 = E.SPEC_CK_DEFAULT
        cut = E.ANOMALY_CUT
        for i, case in enumerate(b.names):
            c = E.pending_before(b.pk, i).tolist()
            assert E.spec_cuts(c, E.NEV, 8) == E.TARGETS and all(c[t] == 0 for t in E.TARGETS), case
            assert [x for x in range(1, E.NEV) if c[x] == 0] == E.TARGETS, case
        first_ok = lambda case, pos: next(e for e in oks(b, case) if e >= pos)
        for s, t in enumerate(E.TARGETS, 1):
            case = f"first_ok_after_cut{s}-stale"
            assert b.anomalies[b.index(case)] == [first_ok(case, t)]
            assert first_ok(case, t) - t <= E.ANOMALY_FLOOR  # only invokes between the cut and it
        for kind in ("garbage", "stale"):
            assert b.anomalies[b.index(f"last_ok_before_cut-{kind}")] == [cut - 1]
            assert b.anomalies[b.index(f"at_ck1-{kind}")] == [first_ok(f"at_ck1-{kind}", cut + ck1)]
            assert b.anomalies[b.index(f"at_ck2-{kind}")] == [first_ok(f"at_ck2-{kind}", cut + ck2)]
            assert cut + ck2 <= b.anomalies[b.index(f"at_ck2-{kind}")][0] < cut + 128
            assert b.anomalies[b.index(f"last_event-{kind}")] == [E.NEV - 1]
            assert b.anomalies[b.index(f"segment0_only-{kind}")][0] < 128
        for case in ("two-garbage_seg2-stale_seg5", "two-stale_seg2-garbage_seg5"):
            a = b.anomalies[b.index(case)]
            assert 256 <= a[0] < 384 and 640 <= a[1] < 768
        a = b.anomalies[b.index("every_segment")]
        assert [x // 128 for x in a] == list(range(8))


@pytest.mark.parametrize("s", range(1, 8))
def test_top_run_survives_the_stale_read(s):
    """The case the verifying run exists for: the stale value is a state of
    the table, so a run from TOP passes the first :ok after the cut.  Shown
    with the oracle alone: the key's prefix before the cut replaced by one
    completed write of the stale value, the stale read does not fail."""
    b = E.get("anomalies")
    k = b.index(f"first_ok_after_cut{s}-stale")
    cut = E.TARGETS[s - 1]
    (bad,) = b.anomalies[k]
    assert oracle("anomalies")["fail_event"][k] == bad
    rows = [op for op in b.hist.to_ops() if op["value"][0] == k]
    n_ev, at = 0, None
    for j, op in enumerate(rows):
        if n_ev == cut:
            at = j
            break
        n_ev += op["type"] in ("invoke", "ok")
    suffix = rows[at:]
    stale = next(op["value"][1] for op in suffix if op["type"] == "ok" and op["f"] == "read"
                 and op is [o for o in suffix if o["type"] == "ok"][0])
    assert stale == rows[0]["value"][1] and rows[0]["f"] == "write"  # the key's first write, long overwritten
    from lincheck.independent import Tuple
    ops = [{"type": "invoke", "f": "write", "value": Tuple(k, stale), "process": 999_999},
           {"type": "ok", "f": "write", "value": Tuple(k, stale), "process": 999_999}] + suffix
    for i, op in enumerate(ops):
        op["index"] = i
    h = H.History.from_ops(ops)
    assert Packed(h).n_events(0) == 2 + E.NEV - cut
    _, orc = cref.check_history(h.as_c(), budget=1 << 20)
    read_at = 2 + bad - cut
    assert orc["valid"][0] == 1 or orc["fail_event"][0] > read_at, "a run from the stale state dies at the read too"


# ---------------------------------------------------------------- (e)
def test_limits():
    """(e): exactly T0_MAX_STATES states, one more, both (per-key tables);
    T0_MAX_WIDTH + 1 pending once in one key; TAGGABLE_MAX_STATES and one more."""
    st = {n: E.batch_states(E.get(n).pk) for n in ("states32", "states33", "states32_33_mixed", "values5", "values6")}
    assert (st["states32"] == E.T0_MAX_STATES).all() and not E.get("states32").pk.view.trans_off
    assert (st["states33"] == E.T0_MAX_STATES + 1).all() and not E.get("states33").pk.view.trans_off
    assert E.get("states32_33_mixed").pk.view.trans_off
    assert st["states32_33_mixed"].tolist() == [E.T0_MAX_STATES + k % 2 for k in range(12)]
    for n in ("states32", "states33", "states32_33_mixed"):
        b = E.get(n)
        assert all(max(p.c) <= E.T0_MAX_WIDTH and E.spec_cuts(p.c, E.NEV, 8) == E.TARGETS for p in b.plans)
    assert (st["values5"] == E.TAGGABLE_MAX_STATES).all() and (st["values6"] == E.TAGGABLE_MAX_STATES + 1).all()
    for n in ("values5", "values6"):
        pk = E.get(n).pk
        trans = N.carray(pk.view.trans, int(pk.view.n_trans), np.uint32)
        assert not pk.view.trans_off and pk.view.init_state == 0
        assert not any((t & 3) >= N.LC_T_WRITE and (t >> 17) == 0 for t in trans.tolist()), "an op installs nil"
    b = E.get("width11")
    for case, p in zip(b.names, b.plans):
        if case.startswith("reaches11"):
            assert max(p.c) == E.T0_MAX_WIDTH + 1 and p.c.count(E.T0_MAX_WIDTH + 1) == 1
        else:
            assert max(p.c) == E.T0_MAX_WIDTH
    assert sum(c.startswith("reaches11") for c in b.names) == 1


# ---------------------------------------------------------------- the lane-level model
def small_cases():
    t = [128]
    return [
        ("rolling7", E.rolling(300, 7, first="invoke")), ("rolling8", E.rolling(300, 8)),
        ("rolling9", E.rolling(160, 9)), ("rolling10", E.rolling(160, 10)),
        ("rolling10-garbage", E.rolling(160, 10).with_anomalies((120, "garbage"))),
        ("dip6_wide", E.dips(200, 10, 6, t, wide=True)),
        ("dip6-garbage", E.dips(200, 10, 6, t).with_anomalies((150, "garbage"))),
        ("dip0-stale", E.dips(200, 8, 0, t).with_anomalies((128, "stale"))),
        ("quiescent", E.quiescent_at(256, t)), ("quiescent-stale", E.quiescent_at(256, t).with_anomalies((128, "stale"))),
        ("long_lived_slot0", E.long_lived(200, 0, floor=8, where=t)), ("long_lived_slot9", E.long_lived(200, 9, where=t)),
        ("long_lived_slot9-garbage", E.long_lived(200, 9, where=t).with_anomalies((170, "garbage"))),
        ("crashed_late", E.crashed_late(300, 3, floor=8, where=t)),
        ("crashed_late-garbage", E.crashed_late(200, 3, where=t).with_anomalies((190, "garbage"))),
        ("burst", E.burst(300, 5, 10, 100, 140)),
        ("ragged65-last_ok", E.Plan(65, E.counts(65, 4, drain=True)).with_anomalies((63, "garbage"))),
    ]


_small = []


def small_batch():
    if not _small:
        b = E.batch(small_cases(), seed=21)
        _, orc = cref.check_history(b.hist.as_c(), budget=1 << 20)
        _small.extend([b, orc])
    return _small


@pytest.mark.parametrize("closed", [False, True], ids=["exact", "closed"])
@pytest.mark.parametrize("case", [c for c, _ in small_cases()])
def test_lattice_model_on_profiles(case, closed):
    """Keys of every profile, 300 events or fewer, through the lane-level
    model of the register tier (emu_t0), exact and closed: it agrees with the
    oracle on them, and with the directed anomaly."""
    b, orc = small_batch()
    i = b.index(case)
    assert b.plans[i].nev <= 300
    trans = N.carray(b.pk.view.trans, int(b.pk.view.n_trans), np.uint32)
    want = (0, min(b.anomalies[i])) if b.anomalies[i] else (1, -1)
    assert (int(orc["valid"][i]), int(orc["fail_event"][i])) == want
    assert emu_t0.check_key(b.pk.events(i), trans, closed=closed) == want
