"""Every tier's budget test at its edge.  need(key) = max(max |I|, max |S'|)
over the events the unbounded :linear search walks (cref.key_sizes;
tests/test_oracle_sizes.py) is the least budget that decides a key: at
B = need the key has its unbounded record, at B = need - 1 it is :unknown /
budget at the first event whose |I| or |S'| passes B.  A budget test written
`>=`, or placed behind the emptiness test, or applied to the wrong set, fails
one of the two runs of a target; budgets that merely lie near a key's sizes
(the rest of the suite) do not notice.

For each band a batch of at most 32 keys with a few targets; each target is run
at need - 1 and at need, the whole batch compared with the oracle at the same
budget (verdict, cause, failing event; peak where the oracle finishes the
key), and the target's flip asserted explicitly.  The bands: the register tier
(one target per pending count 4..10 at the deciding :ok), T1 / T2, the
config-keyed HBM tier (LC_PATH_LAYERS_OFF), the layered tier and what it
hands on, the wide tier (entered by state count and by window slot), WGL (the
budget bounds Lowe's cache) and knossos.competition.

One batch is larger on purpose: the register band runs a second time inside
2,600 keys (fillers of 2-6 events), because k_search_lattice's 4-register
build -- the only one with ok_lane<4>, ok_lane<5> and ok_event_mem<8/16> --
is chosen only above 8 keys per CU.  It costs about as much as a 32-key run.

The wide-window keys are built, not found: synth's crashed ops (conc 30,
info_rate 0.05-0.15, 300-600 ops, seeds 1-4) each multiply the closure, and no
key with 50 ops pending had a need below 2^16; 56 crashed cas ops from a value
never written are inert and hold the slots just the same.

Not covered, and why:
  * a layered-tier target whose deciding layer is larger than the LDS table:
    the oracle reports set sizes, not layer sizes, so such a key cannot be
    chosen on the CPU; test_gpu_layers.test_layers_large_layers_multi_pass
    runs such layers, at budgets that are no key's need.
  * WGL caches ending exactly at 8190 / 8191: the search (300-key batches of
    200 and 300 ops, 10-14 clients, seeds 1-40) found 8185, 8193 and 8206."""
import numpy as np
import pytest

import cref
import edge_keys as EK
import edgegen as E
from lincheck import _native as N
from lincheck import history as H
from lincheck.checker import Device, Packed
from lincheck.independent import Tuple
from test_gpu_wgl import wgl_vs_oracle

pytestmark = pytest.mark.gpu

BUDGET_CAUSE = 2
WGL_LDS_TAB = 4096                 # device_api.hip run_wgl: w.lds_tab for narrow keys
WGL_MIGRATE = WGL_LDS_TAB // 2     # device_wgl.hip: cache_n > a.lds_tab / 2 -> migrate() to the HBM table
WGL_SMALL_SPILL = (1 << 14) // 2   # LC_PATH_WGL_SMALL: spill_at = 2^14 / 2 - 1, a key spills once its cache would reach this


# ------------------------------------------------------------------ bands
class Band:
    """A batch, its unbounded sizes per key and the oracle's records per budget."""

    def __init__(self, name, hist, pk, names, max_keys=32):
        self.name, self.hist, self.pk, self.names = name, hist, pk, names
        self.hc = hist.as_c()
        self.sizes = [cref.key_sizes(self.hc, k, budget=EK.UNBOUNDED) for k in pk.keys]
        self.need = [int(max(a.max(initial=1), b.max(initial=1))) for a, b in self.sizes]
        self.pend = [E.pending_before(pk, i) for i in range(pk.n_keys)]
        self._orc = {}
        assert pk.n_keys <= max_keys and len(names) == pk.n_keys

    def oracle(self, budget):
        if budget not in self._orc:
            keys, orc = cref.check_history(self.hc, budget=budget, threads=8)
            assert list(keys) == self.pk.keys
            self._orc[budget] = orc
        return self._orc[budget]

    def deciding(self, i):
        """(event, |I|, |S'|, ops pending) where key i's sets first reach need."""
        sI, sS = self.sizes[i]
        e = int(np.flatnonzero((sI == self.need[i]) | (sS == self.need[i]))[0])
        return e, int(sI[e]), int(sS[e]), int(self.pend[i][e])

    def describe(self, i):
        e, nI, nS, pend = self.deciding(i)
        full = self.oracle(EK.UNBOUNDED)[i]
        by = "|S'|" if nI < self.need[i] else "|I|"
        at_fail = full["valid"] == 0 and full["fail_event"] == e
        return (f"{self.name} / {self.names[i]}: need {self.need[i]} by {by} at event {e} ({pend} pending, |I| {nI}, "
                f"|S'| {nS}){', the failing :ok' if at_fail else ''}; unbounded verdict {int(full['valid'])}")


def same_as_oracle(band, r, budget, what):
    orc = band.oracle(budget)
    fields = ["valid", "cause", "fail_event"]
    for f in fields:
        bad = np.flatnonzero(getattr(r, f) != orc[f])
        assert not len(bad), (f"{what}, budget {budget}: {f} differs on " + "; ".join(
            f"{band.names[i]} (device {getattr(r, f)[i]}, oracle {orc[f][i]}, need {band.need[i]})" for i in bad[:6]))
    done = orc["cause"] != BUDGET_CAUSE
    bad = np.flatnonzero(done & (r.peak != orc["peak"]))
    assert not len(bad), f"{what}, budget {budget}: peak differs on {[band.names[i] for i in bad[:6]]}"
    return orc


def flip(band, i, tier, **dev_kw):
    """Target i at need - 1 and at need: the whole batch against the oracle,
    and the target's flip.  Returns the two results."""
    need = band.need[i]
    sI, sS = band.sizes[i]
    full = band.oracle(EK.UNBOUNDED)[i]
    assert full["cause"] != BUDGET_CAUSE and need > 1
    print(f"{band.describe(i)}; tier: {tier}")
    below = Device(0, budget=need - 1, **dev_kw).check(band.pk)
    same_as_oracle(band, below, need - 1, f"{band.names[i]} at need - 1")
    first = int(np.flatnonzero((sI > need - 1) | (sS > need - 1))[0])
    got = (int(below.valid[i]), int(below.cause[i]), int(below.fail_event[i]))
    assert got == (-1, BUDGET_CAUSE, first), f"{band.names[i]} at need - 1 = {need - 1}: {got}, expected :unknown / budget at {first}"
    at = Device(0, budget=need, **dev_kw).check(band.pk)
    same_as_oracle(band, at, need, f"{band.names[i]} at need")
    got = (int(at.valid[i]), int(at.cause[i]), int(at.fail_event[i]), int(at.peak[i]))
    want = (int(full["valid"]), int(full["cause"]), int(full["fail_event"]), int(full["peak"]))
    assert got == want, f"{band.names[i]} at need = {need}: {got}, unbounded {want}"
    return below, at


def synth_band(name, rows):
    b = EK.build(name, rows)
    return Band(name, b.hist, b.pk, [f"{r[2] or 'target'}:seed{r[0]['seed']}/ops{r[0]['ops_per_key']}/key{r[1]}" for r in rows])


_bands = {}


def band(name):
    if name not in _bands:
        _bands[name] = BANDS[name]()
    return _bands[name]


# -- the register tier: keys that never pass 10 pending
REG_NEV = 120
REG_P = (4, 5, 6, 7, 8, 9, 10)
REG_BAD_READS = (("garbage", 30), ("garbage", 60), ("stale", 90))


def register_cases():
    """rolling(120, P): every :ok of such a key has P ops pending.  Per P a
    valid key, two with a garbage read (at event 30, at 60) and one with a
    stale read at 90 (edgegen seed 2: for P = 6 .. 10 one of the bad reads'
    |I| is its key's largest set; test_register_tier_targets_cover_the_orderings)."""
    cases = []
    for P in REG_P:
        pl = E.rolling(REG_NEV, P)
        cases += [(f"rolling{P}-valid", pl)] + [(f"rolling{P}-{kind}{pos}", pl.with_anomalies((pos, kind)))
                                                 for kind, pos in REG_BAD_READS]
    return cases


def register_band():
    b = E.batch(register_cases(), seed=2)
    assert max(max(p.c) for p in b.plans) <= E.T0_MAX_WIDTH
    return Band("register", b.hist, b.pk, b.names)


# k_search_lattice has two builds (step_plan.hpp plan_step, t0_wide): up to 8 keys per CU the 16-register
# one (RM = T0_RBIG), which sends every :ok of at most 6 pending to ok_lane<6> and 9 / 10 pending to
# ok_reg<8> / ok_reg<16>; above that the 4-register one (RM = T0_RSMALL), which alone reaches ok_lane<4>,
# ok_lane<5>, ok_event_mem<8> / <16> and its own ok_reg<2> / <4>.  lc_stats names the kernel, not the
# build, so the build is chosen here by the batch's size, as the library chooses it.
CU_COUNT = 256                     # the MI355X's
COMPACT_KEYS = 2600                # > 8 keys per CU: the 4-register build
BUILDS = ("16reg", "4reg")
UNSEGMENTED = N.LC_PATH_SPLIT_OFF | N.LC_PATH_SPEC_OFF  # k_search_lattice whatever the batch (as test_gpu_register_edges)


def register_compact_band():
    """The register band's 28 keys and the three |S'| targets inside a batch
    of 2,600 keys: fillers of 2-6 events, every seventh with a garbage read
    (as edgegen.compact_cases pads), so that the 4-register build runs."""
    cases = register_cases()
    by_s = synth_band("register_by_S", REG_BY_S)
    n = 0
    while len(cases) < COMPACT_KEYS - len(REG_BY_S):
        nev = 2 + n % 5
        plan = E.Plan(nev, E.counts(nev, 2 + n % 2, drain=True))
        cases.append((f"filler{n}", plan.with_anomalies((0, "garbage")) if n % 7 == 3 else plan))
        n += 1
    b = E.batch(cases, seed=2)
    hist = EK.merge([b.hist] + [EK.renumbered(by_s.hist, i, len(cases) + i) for i in range(len(REG_BY_S))])
    pk = Packed(hist)
    assert pk.keys == list(range(COMPACT_KEYS)) and pk.n_keys > CU_COUNT * 8
    out = Band("register_compact", hist, pk, b.names + by_s.names, max_keys=COMPACT_KEYS)
    small = band("register")  # the same keys, seed for seed, as the 32-key band's
    assert out.need[:len(small.need)] == small.need and out.need[-len(REG_BY_S):] == by_s.need
    return out


def register_bands(build):
    """(the band holding the rolling keys, the band holding the |S'| targets) of a build."""
    if build == "4reg":
        return band("register_compact"), band("register_compact")
    return band("register"), band("register_by_S")


# register-tier keys whose largest set is an |S'| (max |S'| > max |I|): rare (about one synth key in 50 at
# 6-10 clients); found by scanning synth(n_keys=300, ops_per_key=60, anomaly_rate=0.15) at 6, 8, 10 clients
REG_BY_S = [
    ({'n_keys': 300, 'ops_per_key': 60, 'concurrency': 10, 'anomaly_rate': 0.15, 'seed': 1}, 279, None, 9, 200, 192, 0),
    ({'n_keys': 300, 'ops_per_key': 60, 'concurrency': 8, 'anomaly_rate': 0.15, 'seed': 2}, 39, None, 7, 52, 50, 1),
    ({'n_keys': 300, 'ops_per_key': 60, 'concurrency': 6, 'anomaly_rate': 0.15, 'seed': 5}, 56, None, 5, 12, 10, 1),
]

# -- T1 / T2: the fit classes and T1's over-by-S' class (need below T1's |I| capacity)
SET_ROWS = EK.rows_of("t1_fit") + EK.rows_of("t1_over_S") + EK.rows_of("t2_fit")
SET_TARGETS = {  # index in SET_ROWS -> what the target is
    0: "T1: need 512 = CAP_I, |S'| 256 = CAP_S",
    5: "T1: need 480 by |I| (the key later leaves T1 by |S'| 264)",
    6: "T2: need 2144 by |I| after |S'| has fitted 1024 = CAP_S",
    8: "T2: need 4096 = CAP_I",
}

# -- beyond T2: the HBM tiers
HBM_EXTRA = [  # beyond T2 by |S'|, largest set below the LDS pass's limits
    ({'n_keys': 300, 'ops_per_key': 200, 'concurrency': 11, 'info_rate': 0.01, 'anomaly_rate': 0.15, 'seed': 3}, 141, None, 11, 1160, 2016, 1),
    ({'n_keys': 300, 'ops_per_key': 200, 'concurrency': 11, 'info_rate': 0.01, 'anomaly_rate': 0.15, 'seed': 3}, 180, None, 13, 1536, 1696, 1),
]
HBM_ROWS = EK.rows_of("hbm_narrow")[:4] + HBM_EXTRA
HBM_TARGETS = {
    4: "need 2016 inside an LDS pass (|S'| <= 2048, |I| <= 4096 at every :ok)",
    5: "need 1696 inside an LDS pass",
    0: "need 2176 at an :ok whose |S'| is 2048 = LIM_S",
    3: "need 4120: the LDS pass is redone on the HBM tables (|I| passes 4096 = LIM_I), then the budget",
}
# 12 register values (13 states > 8: the layered tier hands the key on to the config-keyed tier)
MANY_VALUES = [
    ({'n_keys': 64, 'ops_per_key': 300, 'concurrency': 14, 'info_rate': 0.01, 'n_values': 12, 'anomaly_rate': 0.15, 'seed': 43}, 40, None, 12, 1536, 5248, 1),
]
WIDE_NEV = 1000


def wide_band():
    """Keys with 401 register states (> LC_NARROW_MAX_STATES = 255: wide
    configs, the wide HBM tier): rolling(1000, P) with two ops in three a
    write of a value of its own, 500 ops per key.  P = 10: need ~3,000."""
    def plan(P):
        pl = E.rolling(WIDE_NEV, P)
        n_inv = sum(1 for b in range(WIDE_NEV) if pl.c[b + 1] > pl.c[b])
        return E.Plan(pl.nev, pl.c, kinds={o: "write" for o in range(n_inv) if o % 3 != 2})
    cases = [(f"wide{P}", plan(P)) for P in (8, 9, 10)] + [("wide9-garbage", plan(9).with_anomalies((900, "garbage")))]
    b = E.batch(cases, seed=1, values=range(400), stale=None, garbage=9999, per_key_values=True)
    assert (E.batch_states(b.pk) > 255).all()
    return Band("wide", b.hist, b.pk, b.names)


WINDOW_INERT = 56  # crashed ops holding window slots 0 .. 55 for good: the next invoke gets a slot >= LC_NARROW_MAX_SLOTS


def wide_window_band():
    """Keys with 57-66 ops pending and a need of about a thousand: 56
    crashed cas ops from a value no op ever writes (they can never take
    effect, so they add nothing to a closure) under rolling(300, 10) keys
    (edgegen seeds 1, 2; one with a garbage read).  Every live op then has a
    window slot >= 56: the keys leave the register tier, and T1 at their
    first live :invoke (device_search.hip search_key_lds, slot >=
    LC_NARROW_MAX_SLOTS: K_WIDE), for the wide HBM tier."""
    parts, names = [], []
    for k, (seed, anomaly) in enumerate(((1, None), (2, None), (1, (200, "garbage")))):
        pl = E.rolling(300, 10)
        b = E.batch([("w", pl.with_anomalies(anomaly) if anomaly else pl)], seed=seed)
        inert = []
        for p in range(WINDOW_INERT):
            for t in ("invoke", "info"):
                inert.append({"type": t, "f": "cas", "value": Tuple(0, [99, 1]), "process": 5000 + p})
        ops = inert + b.hist.to_ops()
        for i, o in enumerate(ops):
            o["index"] = i
        parts.append(EK.renumbered(H.History.from_ops(ops), 0, k))
        names.append(f"window57-seed{seed}" + ("-garbage200" if anomaly else ""))
    hist = EK.merge(parts)
    pk = Packed(hist)
    assert pk.keys == [0, 1, 2]
    for i in range(3):
        assert E.pending_before(pk, i).max() >= WINDOW_INERT + 10
    return Band("wide_window", hist, pk, names)


BANDS = {
    "register": register_band,
    "register_by_S": lambda: synth_band("register_by_S", REG_BY_S),
    "register_compact": register_compact_band,
    "wide_window": wide_window_band,
    "set_tiers": lambda: synth_band("set_tiers", SET_ROWS),
    "hbm": lambda: synth_band("hbm", HBM_ROWS),
    "many_values": lambda: synth_band("many_values", MANY_VALUES + EK.rows_of("t2_over_S")[:2]),
    "wide": wide_band,
}


# ------------------------------------------------------------------ :linear
def register_target(b, P):
    """The key of rolling(P) to flip: the one whose largest set is its failing
    :ok's |I| if there is one, else the valid key."""
    full = b.oracle(EK.UNBOUNDED)
    for kind, pos in REG_BAD_READS:
        i = b.names.index(f"rolling{P}-{kind}{pos}")
        e, nI, _nS, _ = b.deciding(i)
        if full["valid"][i] == 0 and full["fail_event"][i] == e and nI == b.need[i]:
            return i, True
    return b.names.index(f"rolling{P}-valid"), False


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("P", REG_P)
def test_register_tier(P, build):
    """One target per pending count at the deciding :ok, in both builds of
    k_search_lattice.  16reg (the 32-key batch): ok_lane<6> (4-6 pending),
    ok_reg<2> / <4> (7, 8), ok_reg<8> / <16> (9, 10).  4reg (the same keys
    among 2,600): ok_lane<4> / <5> / <6> by the highest live op index,
    its ok_reg<2> / <4>, ok_event_mem<8> / <16> (9, 10)."""
    b, _ = register_bands(build)
    i, at_fail = register_target(b, P)
    e, _nI, _nS, pend = b.deciding(i)
    assert pend == P, f"{b.names[i]}: {pend} pending at the deciding :ok"
    below, at = flip(b, i, f"register tier, {build} build", path_flags=UNSEGMENTED)
    assert below.stats["t0_path"] == at.stats["t0_path"] == "k_search_lattice"
    assert below.stats["deep_keys"] == 0
    if at_fail:  # |I| is tested before emptiness: :unknown, not :invalid, at the same event
        assert int(at.valid[i]) == 0 and int(below.fail_event[i]) == int(at.fail_event[i])


def test_register_tier_targets_cover_the_orderings():
    """Of the register tier's targets some are decided by |I| at the failing
    :ok -- at 7 or 8 pending (ok_reg) among them -- and the others by |I|
    before the key's end; the |S'| ones are test_register_tier_by_S's."""
    b = band("register")
    at_fail = {P for P in REG_P if register_target(b, P)[1]}
    assert at_fail == {6, 7, 8, 9, 10}, at_fail  # ok_lane, ok_reg<2>, <4>, and both 9- and 10-pending forms


REG_BY_S_PENDING = (9, 7, 4)  # ops pending at each REG_BY_S target's deciding :ok


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("n", range(len(REG_BY_S)))
def test_register_tier_by_S(n, build):
    """Targets whose largest set is an |S'| (the |I| test passes at need - 1;
    the |S'| test, behind the emptiness test, decides), with 9, 7 and 4 ops
    pending at the deciding :ok, in both builds."""
    _, b = register_bands(build)
    i = b.names.index(band("register_by_S").names[n])
    e, nI, nS, pend = b.deciding(i)
    assert pend == REG_BY_S_PENDING[n], f"{b.names[i]}: {pend} pending at the deciding :ok"
    assert nS == b.need[i] and b.sizes[i][0].max() < b.need[i] and b.pend[i].max() <= E.T0_MAX_WIDTH
    below, at = flip(b, i, f"register tier, {build} build", path_flags=UNSEGMENTED)
    assert below.stats["t0_path"] == at.stats["t0_path"] == "k_search_lattice"


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("budget", [2047, 2048, 4095, 4096])
def test_register_tier_counting_thresholds(budget, build):
    """budget < 64 x 32 compiles ok_lane's size reductions in, budget <
    RL x 64 x 32 those of ok_reg<RL> / ok_event_mem<RL>: on both sides of the
    first two thresholds the records are the oracle's, in both builds."""
    for b in dict.fromkeys(register_bands(build)):
        r = Device(0, budget=budget, path_flags=UNSEGMENTED).check(b.pk)
        same_as_oracle(b, r, budget, f"{b.name}, {build} build")
        assert r.stats["t0_path"] == "k_search_lattice"


@pytest.mark.parametrize("i", sorted(SET_TARGETS))
def test_set_tiers(i):
    b = band("set_tiers")
    below, at = flip(b, i, SET_TARGETS[i])
    assert below.stats["deep_keys"] == 0 and at.stats["deep_keys"] == 0  # decided in T1 / T2 both times


@pytest.mark.parametrize("path", ["layers_off", "default"])
@pytest.mark.parametrize("i", sorted(HBM_TARGETS))
def test_hbm_tiers(i, path):
    """The config-keyed narrow tier (LC_PATH_LAYERS_OFF) and the layered tier
    (the default path) on the same targets."""
    b = band("hbm")
    e, nI, nS, _ = b.deciding(i)
    sI, sS = b.sizes[i]
    beyond = np.flatnonzero((sS > EK.T2_S) | (sI > EK.T2_I))
    assert len(beyond) and beyond[0] <= e, f"{b.names[i]} is decided before it leaves T2"
    if i in (4, 5):
        assert sS.max() <= EK.HBM_LIM_S and sI.max() <= EK.HBM_LIM_I
    if i == 0:
        assert nS == EK.HBM_LIM_S
    if i == 3:
        assert nI > EK.HBM_LIM_I
    flags = N.LC_PATH_LAYERS_OFF if path == "layers_off" else 0
    tier = "config-keyed HBM tier" if flags else "layered HBM tier"
    below, at = flip(b, i, f"{tier}; {HBM_TARGETS[i]}", path_flags=flags)
    assert at.stats["deep_keys"] > 0


@pytest.mark.parametrize("path", ["layers_off", "default"])
def test_key_with_more_than_8_register_values(path):
    """13 states: the layered tier hands the key to the config-keyed tier."""
    b = band("many_values")
    flags = N.LC_PATH_LAYERS_OFF if path == "layers_off" else 0
    flip(b, 0, "config-keyed HBM tier" + ("" if flags else ", handed on by the layered tier"), path_flags=flags)


@pytest.mark.parametrize("name", ["wide10", "wide9-garbage"])
def test_wide_configs(name):
    """Wide configs by state count (key_states > 255: K_WIDE at the key's start)."""
    b = band("wide")
    below, at = flip(b, b.names.index(name), "wide HBM tier (401 states)")
    assert at.stats["deep_keys"] == b.pk.n_keys


@pytest.mark.parametrize("path", ["layers_off", "default"])
@pytest.mark.parametrize("name", ["window57-seed1", "window57-seed1-garbage200"])
def test_wide_window(name, path):
    """Wide configs by window slot (an :invoke with slot >= 56: K_WIDE in mid
    key), with 57-66 ops pending and a need of about a thousand."""
    b = band("wide_window")
    flags = N.LC_PATH_LAYERS_OFF if path == "layers_off" else 0
    below, at = flip(b, b.names.index(name), "wide HBM tier (window slots >= 56)", path_flags=flags)
    assert at.stats["deep_keys"] == b.pk.n_keys


# ------------------------------------------------------------------ WGL
# (synth kwargs, key, Lowe's cache size at the end of the unbounded walk, valid)
WGL_ROWS = [
    ({'n_keys': 300, 'ops_per_key': 300, 'concurrency': 12, 'info_rate': 0.01, 'anomaly_rate': 0.1, 'seed': 5}, 16, 2046, 1),
    ({'n_keys': 300, 'ops_per_key': 150, 'concurrency': 14, 'info_rate': 0.01, 'anomaly_rate': 0.1, 'seed': 1}, 45, 2047, 1),
    ({'n_keys': 300, 'ops_per_key': 300, 'concurrency': 14, 'info_rate': 0.01, 'anomaly_rate': 0.1, 'seed': 4}, 143, 2050, 1),
    ({'n_keys': 300, 'ops_per_key': 150, 'concurrency': 12, 'info_rate': 0.01, 'anomaly_rate': 0.1, 'seed': 4}, 266, 2051, 0),
    ({'n_keys': 300, 'ops_per_key': 300, 'concurrency': 12, 'info_rate': 0.01, 'anomaly_rate': 0.1, 'seed': 4}, 143, 1023, 1),
    ({'n_keys': 300, 'ops_per_key': 300, 'concurrency': 12, 'info_rate': 0.01, 'anomaly_rate': 0.1, 'seed': 1}, 59, 1025, 1),
]
WGL_SPILL_ROWS = [  # the nearest to 8190 / 8191 / 8192 found (module docstring)
    ({'n_keys': 300, 'ops_per_key': 200, 'concurrency': 14, 'info_rate': 0.01, 'anomaly_rate': 0.1, 'seed': 25}, 207, 8185, 0),
    ({'n_keys': 300, 'ops_per_key': 200, 'concurrency': 14, 'info_rate': 0.01, 'anomaly_rate': 0.1, 'seed': 18}, 78, 8193, 0),
    ({'n_keys': 300, 'ops_per_key': 200, 'concurrency': 14, 'info_rate': 0.01, 'anomaly_rate': 0.1, 'seed': 37}, 111, 8206, 0),
]
_wgl = {}


def wgl_batch(name, rows):
    """The rows' keys as one batch; the cache sizes pinned are the oracle's."""
    if name not in _wgl:
        hist = EK.merge([EK.one_key(kw, k, i) for i, (kw, k, _c, _v) in enumerate(rows)])
        keys, orc, _fin, _nf = cref.check_history_wgl(hist.as_c(), budget=1 << 20, threads=8)
        got = [(int(r["peak"]), int(r["valid"])) for r in orc]
        assert got == [(c, v) for _kw, _k, c, v in rows], f"{name}: cache sizes {got}: choose the keys again"
        _wgl[name] = (hist, orc)
    return _wgl[name]


@pytest.mark.parametrize("i", range(len(WGL_ROWS)))
def test_wgl_cache_budget(i):
    """need = the unbounded walk's cache size: below and above the LDS
    table's migration point (2048; 1024 should the launch halve the table)."""
    hist, full = wgl_batch("wgl", WGL_ROWS)
    need = WGL_ROWS[i][2]
    side = "below" if need <= WGL_MIGRATE else "above"
    print(f"wgl key {i}: cache {need}, {side} the migration point {WGL_MIGRATE}; unbounded verdict {int(full['valid'][i])}")
    _, below, orc = wgl_vs_oracle(hist, need - 1)
    assert (int(orc["valid"][i]), int(orc["cause"][i])) == (-1, BUDGET_CAUSE)
    assert (int(below.valid[i]), int(below.cause[i]), int(below.peak[i])) == (-1, BUDGET_CAUSE, int(orc["peak"][i]))
    _, at, orc = wgl_vs_oracle(hist, need)
    for f in ("valid", "cause", "fail_event", "peak"):
        assert int(getattr(at, f)[i]) == int(orc[f][i]) == int(full[f][i]), f


def test_wgl_small_tables_spill_threshold():
    """LC_PATH_WGL_SMALL at 2^16: a key is searched again with the budget's
    table exactly when its cache would reach 8192 (spill_at = 2^14 / 2 - 1,
    tested as cache_n + 1 > spill_at before the entry is made)."""
    hist, full = wgl_batch("wgl_spill", WGL_SPILL_ROWS)
    _, res, orc = wgl_vs_oracle(hist, 1 << 16, path_flags=N.LC_PATH_WGL_SMALL)
    want = int((orc["peak"] >= WGL_SMALL_SPILL).sum())
    print(f"wgl spill: caches {orc['peak'].tolist()}, spilled {res.stats['wgl_spilled']}, expected {want}")
    assert want == 2
    assert res.stats["wgl_spilled"] == want


# ------------------------------------------------------------------ competition
def test_competition_hands_over_exactly_the_budget_keys():
    """knossos.competition at B = need - 1 of a T2 target: WGL answers exactly
    the keys the :linear oracle leaves at the budget, with its own oracle's
    verdicts; the others keep :linear's records."""
    b = band("set_tiers")
    i = 6
    B = b.need[i] - 1
    lin = b.oracle(B)
    keys, wgl, _fin, _nf = cref.check_history_wgl(b.hc, budget=B, threads=8)
    left = lin["cause"] == BUDGET_CAUSE
    assert left[i] and wgl["valid"][i] != -1, "WGL does not decide the target at this budget: choose another"
    assert not left.all()
    r = Device(0, budget=B, algorithm=N.LC_ALGO_COMPETITION).check(b.pk)
    print(f"competition at {B}: :linear leaves {np.flatnonzero(left).tolist()}, analyzer {r.analyzer.tolist()}")
    np.testing.assert_array_equal(r.analyzer == N.LC_ALGO_WGL, left)
    for f in ("valid", "cause", "fail_event"):
        np.testing.assert_array_equal(getattr(r, f)[left], wgl[f][left], err_msg=f"wgl keys: {f}")
        np.testing.assert_array_equal(getattr(r, f)[~left], lin[f][~left], err_msg=f":linear keys: {f}")
