"""A check on the checker: the bands of tests/model_bands.py that
test_gpu_model_tiers.py runs on the device are what they are named for.
Everything here comes from the oracles and the packed batches (no GPU): each
key's tier class from its unbounded set sizes, the verdict mix, the pinned
competition budget, the WGL caches on both sides of the move from LDS to HBM,
and the state counts at the 15-bit limit -- so a later change to a generator,
an oracle or a capacity cannot quietly turn the deep keys into shallow ones.

Measured here (one core, the C oracle on 8 threads): building a band with its
unbounded sizes and records takes 2.0 s (mr_narrow), 0.8 s (mr_wide) and 0.06
- 0.25 s (the register and mutex bands, which use the C oracle); wgl_ref adds
0.3 s (mr_narrow) and 0.6 s (mr_wide).  The two keys at the map limit are the
slow ones: LR.reachable_maps takes 11 s for the key with 32,767 maps (187 :txn
values stepped from every map) and 1.7 s for the one with 32,768, so
test_map_counts_at_the_limit takes 14 s; the rest of this module takes 4 s."""
import os
import re
import time

import numpy as np
import pytest

import cref
import histgen
import linear_ref as LR
import model_bands as MB
from lincheck import _native as N
from lincheck import history as H
from lincheck import model
from lincheck.checker import Packed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jepsen-etcd-demo_amd", "csrc")
BAND_SECONDS = 30  # a band and its records: measured at 2.0 s at the most (module docstring)

# band -> the classes it must hold (ISSUE: what each band is for)
MUST_HOLD = {
    "mr_narrow": {"t1", "t2", "hbm_lds", "hbm_hbm"},
    "mr_wide": {"wide_states"},
    "reg7": {"t2", "hbm_lds", "hbm_hbm"},
    "reg12": {"hbm_lds", "hbm_hbm"},
    "reg_wide": {"wide_states"},
    "mutex": {"t2", "hbm_lds", "hbm_hbm"},
}


@pytest.mark.parametrize("file,pattern,value", [
    ("device_search.hip", r"T1_S = (\d+)", MB.T1_S), ("device_search.hip", r"T1_I = (\d+)", MB.T1_I),
    ("device_search.hip", r"T2_S = (\d+)", MB.T2_S), ("device_search.hip", r"T2_I = (\d+)", MB.T2_I),
    ("device_hbm.hip", r"LDS_ES = (\d+), LDS_EI = \d+, LIM_S = LDS_ES / 2, LIM_I = LDS_EI / 2;", 2 * MB.HBM_LIM_S),
    ("device_hbm.hip", r"LDS_ES = \d+, LDS_EI = (\d+), LIM_S = LDS_ES / 2, LIM_I = LDS_EI / 2;", 2 * MB.HBM_LIM_I),
    ("../../include/lincheck.h", r"#define LC_NARROW_MAX_STATES (\d+)", MB.NARROW_MAX_STATES),
    ("../../include/lincheck.h", r"#define LC_WIDE_MAX_STATES +(\d+)", LR.WIDE_MAX_STATES),
])
def test_restated_capacity(file, pattern, value):
    """The capacities the classes are placed by are the sources'."""
    m = re.search(pattern, open(os.path.join(CSRC, file)).read())
    assert m, f"{file}: {pattern!r} not found (the restated constant has lost its source)"
    assert int(m.group(1)) == value


@pytest.mark.parametrize("name", sorted(MB.ROWS))
def test_band_is_what_it_is_named_for(name):
    """Every key has its pinned class, sizes and verdict (ModelBand asserts
    them while building) and a need above 1; the band holds the classes it is
    for, valid keys, and an invalid key past T1 whose failing :ok is not its
    first; it is built, records included, in bounded time."""
    t0 = time.time()
    b = MB.band(name)
    full = b.oracle(MB.UNBOUNDED)
    took = time.time() - t0
    for i in range(b.pk.n_keys):
        print(b.describe(i))
    assert b.pk.n_keys <= MB.MAX_KEYS and took < BAND_SECONDS
    assert all(n > 1 for n in b.need)
    assert MUST_HOLD[name] <= set(b.cls)
    assert (full["cause"] != MB.BUDGET_CAUSE).all()
    assert (full["valid"] == 1).any()
    bad = [i for i in range(b.pk.n_keys) if full["valid"][i] == 0 and b.cls[i] != "t1"]
    assert bad and all(full["fail_event"][i] > b.first_ok(i) for i in bad)
    if name == "mr_wide":
        assert b.cls.count("wide_states") >= 2
    if name == "mr_narrow":
        assert max(b.need[i] for i in range(b.pk.n_keys) if b.cls[i] == "hbm_hbm") < 5000
        assert b.table and b.pk.view.table
    if name == "reg7":
        assert set(b.states) == {8}
    if name == "reg12":
        assert set(b.states) == {13}
    if name in ("reg_wide", "mr_wide"):
        assert min(b.states) > MB.NARROW_MAX_STATES
    if name == "mutex":
        assert set(b.states) == {2}


def test_register_and_mutex_bands_hold_deep_invalid_keys():
    """An invalid key past T2 among the register bands (reg12 key 0, |I| 4160)."""
    b = MB.band("reg12")
    assert b.cls[0] == "hbm_hbm" and b.oracle(MB.UNBOUNDED)["valid"][0] == 0


def test_table_target_decided_by_S():
    """mr_narrow key 8: max |S'| > max |I| (the budget flip decided by |S'|)."""
    b = MB.band("mr_narrow")
    sI, sS = b.sizes[8]
    assert b.cls[8] == "t2" and sS.max() == b.need[8] == 864 > sI.max()


def test_linear_ref_sizes_are_the_c_oracles_on_a_register_band():
    """sizes_of(linear_ref.analysis) is what cref.key_sizes gives (the form
    the table bands' sizes take), checked on a band both oracles know."""
    b = MB.band("mutex")
    for i in (1, 2, 5):
        sI, sS = MB.sizes_of(b.analysis(i))
        np.testing.assert_array_equal(sI, b.sizes[i][0])
        np.testing.assert_array_equal(sS, b.sizes[i][1])
        a = b.analysis(i)
        rec = b.oracle(MB.UNBOUNDED)[i]
        assert MB.record_of(a) == (rec["valid"], rec["cause"], rec["fail_event"], rec["peak"], rec["probes"])


@pytest.mark.parametrize("gen,kw,mdl", [
    ("register_history", dict(n_keys=20, n_ops=40, procs=6, n_values=4), "register"),
    ("register_history", dict(n_keys=20, n_ops=40, procs=6, n_values=4, p_info=0.1), "register"),
    ("mutex_crash_history", dict(n_keys=20, rounds=20, procs=5, p_info=0.0), "mutex"),
    ("mutex_crash_history", dict(n_keys=20, rounds=20, procs=5, p_info=0.15), "mutex"),
])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_uncorrupted_keys_are_valid(gen, kw, mdl, seed):
    """Linearizable by construction: without corruption every key is valid,
    with crashed ops (effect applied or not) as without."""
    ops = getattr(histgen, gen)(seed, corrupt=0.0, **kw)
    _keys, orc = cref.check_history(H.History.from_ops(ops).as_c(), budget=1 << 20, threads=8, model=mdl)
    assert len(orc) == kw["n_keys"] and (orc["valid"] == 1).all()
    if kw.get("p_info"):
        assert any(op["type"] == "info" for op in ops)


@pytest.mark.parametrize("p_info", [0.0, 0.1])
def test_uncorrupted_table_keys_are_valid(p_info):
    """The same for multi_register_history at the bands' widths, by linear_ref."""
    ops = histgen.multi_register_history(3, n_keys=10, n_ops=30, procs=8, regs=("x", "y"), values=(0, 1, 2), width=4.0,
                                         corrupt=0.0, p_info=p_info)
    orc = LR.check_independent(ops, model="multi-register")
    assert len(orc) == 10 and all(a.valid is True for a in orc.values())


@pytest.mark.parametrize("gen,mdl", [("register_history", "register"), ("mutex_crash_history", "mutex")])
def test_corrupted_keys(gen, mdl):
    """Corruption makes invalid keys (a crashed op may still stand in for
    the lost effect, so not every corrupted key is one)."""
    ops = getattr(histgen, gen)(4, n_keys=30, corrupt=1.0, p_info=0.02)
    _keys, orc = cref.check_history(H.History.from_ops(ops).as_c(), budget=1 << 20, threads=8, model=mdl)
    assert (orc["valid"] == 0).sum() >= 10


def test_mutex_generator_crashes_both_kinds_of_op():
    """Crashed acquires and crashed releases both occur, some keys end early
    (the lock held for good after a crashed release without effect: at most
    `tail` crashed ops follow), and every key is still valid."""
    ops = histgen.mutex_crash_history(3, n_keys=40, rounds=30, p_info=0.25, corrupt=0.0, tail=4)
    crashed = {op["f"] for op in ops if op["type"] == "info"}
    assert crashed == {"acquire", "release"}
    lengths = [sum(1 for op in ops if op["value"][0] == k and op["type"] == "ok" and op["f"] == "acquire") for k in range(40)]
    assert min(lengths) < 10 and max(lengths) >= 20
    _keys, orc = cref.check_history(H.History.from_ops(ops).as_c(), budget=1 << 20, threads=8, model="mutex")
    assert (orc["valid"] == 1).all()


def test_competition_budget():
    """At COMPETITION_BUDGET linear_ref gives up on keys of mr_narrow and
    wgl_ref decides every one of them."""
    b = MB.band("mr_narrow")
    left = np.flatnonzero(b.oracle(MB.COMPETITION_BUDGET)["cause"] == MB.BUDGET_CAUSE).tolist()
    assert left == [2, 3, 6, 9, 10]
    wgl = b.wgl(MB.COMPETITION_BUDGET)
    decided = [i for i in left if wgl[i].valid != "unknown"]
    print("wgl at the competition budget:", [(i, str(wgl[i].valid), wgl[i].cache_size) for i in left])
    assert decided == [2, 3, 6, 9]  # key 10's cache (9,653) passes the budget too: WGL's :unknown is the answer


def test_wgl_caches_on_both_sides_of_the_migration():
    """Lowe's cache at the end of the unbounded walk, per key of mr_narrow."""
    b = MB.band("mr_narrow")
    caches = [w.cache_size for w in b.wgl(MB.UNBOUNDED)]
    assert caches == [2688, 2190, 88, 270, 987, 108, 313, 370, 178, 255, 9653]
    assert tuple(i for i, c in enumerate(caches) if c > MB.WGL_MIGRATE) == MB.WGL_ABOVE_MIGRATE
    assert tuple(i for i, c in enumerate(caches) if c <= MB.WGL_MIGRATE) == MB.WGL_BELOW_MIGRATE
    assert tuple(i for i, c in enumerate(caches) if c >= MB.WGL_SMALL_SPILL) == MB.WGL_SPILLS
    src = open(os.path.join(CSRC, "device_wgl.hip")).read()
    assert "a.lds_tab / 2" in src, "the migration point has lost its source"


def test_map_counts_at_the_limit():
    """7 x 31 x 151 = 32,767 and 8 x 8 x 8 x 64 = 32,768 reachable maps, by
    LR.reachable_maps and by lc_pack; the last map of the decided key is the
    state the failing read stands in."""
    ops = MB.map_limit_ops()
    pk = Packed(H.History.from_ops(ops), model.multi_register())
    assert pk.keys == [0, 1, 2, 3]
    states = [int(x) for x in N.carray(pk.view.key_states, 4, np.uint16)]
    assert states[1:3] == [LR.WIDE_MAX_STATES, LR.WIDE_MAX_STATES + 1] and max(states[0], states[3]) <= 16
    for k, want in ((1, 32767), (2, 32768)):
        o, events = LR.complete(LR.subhistory(ops, k), "multi-register")
        assert LR.reachable_maps(o, LR.multi_register_init(), LR.WIDE_MAX_STATES) == want
        assert max(MB.slots_of(events).values()) == 0  # sequential: every set has one config
    a0 = LR.analysis(LR.subhistory(ops, 0), model="multi-register")
    a3 = LR.analysis(LR.subhistory(ops, 3), model="multi-register")
    assert a0.valid is False and a3.valid is True


def test_value_counts_at_the_limit():
    """32,766 and 32,767 distinct written values: the C oracle decides the
    first and gives :unknown / states for the second."""
    ops = MB.value_limit_ops()
    hist = H.History.from_ops(ops)
    for k, n in ((1, MB.VALUES_AT_LIMIT), (2, MB.VALUES_PAST_LIMIT)):
        vals = {op["value"][1] for op in ops if op["value"][0] == k and op["f"] == "write"}
        assert len(vals) == n
    _keys, orc = cref.check_history(hist.as_c(), budget=1 << 20, threads=8)
    assert orc["valid"].tolist()[1:3] == [1, -1] and orc["cause"].tolist()[1:3] == [0, 4]
    assert orc["fail_event"][2] == -1 and orc["peak"][1] == 1
    pk = Packed(hist)
    assert pk.state_value(1, MB.VALUES_AT_LIMIT) == MB.VALUES_AT_LIMIT
