"""Every small history (tests/small_scope.py: cas2, cas3, cas4p2, reg4, mutex4 --
381,794 keys of at most 8 events) through the register tier's paths, WGL, the
node records and the streams, against the C restatement (cref), which
tests/test_small_scope.py pins to the definition on the same keys.  Every leg
runs every key of the scopes it names; k_spec and the quiescent-point segments
take a scope in batches (their plan has a workspace cap / a key limit), and
every batched call asserts the path it ran on.

  (a) test_unsegmented         k_search_lattice, 16- and 32-bit words, exact sets, final configs
  (b) test_spec*               k_spec: 2/4/8 segments, checkpoints, NOSTAGE / COST / NOPRIO, exact builds
  (c) test_segments            k_search_segments, seg_len 0 and 1 (cas2, cas3)
  (d) test_default_path        whatever Device(0) chooses
  (e) test_budgets             budgets 1..12 on (a)'s path
  (f) test_wgl*, test_competition
  (g) test_node_records        upload + check_node, check_node_async through three pinned buffers
  (h) test_stream              cas3, one row of each key in turn: plain, exact, set_tier, both
  (i) test_row_order           the one-shot check of that row order

As enumerated every key stays in the register tier (peaks of at most 11
configs, at most 4 ops pending), so in leg (h) no key migrates: its set_tier
runs prove only that nothing migrates needlessly.  small_scope.widened takes
every key of cas2, cas3, cas4p2 and reg4 out of the register tier with inert
ops -- crashed ops that can never be linearized, 11 or 62 a key, before the
key's first row (head), its middle row (mid) or its last row (tail) -- and the
records stay the unwidened key's (tests/test_small_scope.py); the oracle here
is cref on the widened history.  Each leg asserts the tier that answered:

  (j) test_t1*                 + 11: k_search_lds (T1), every placement; probes, verdicts only, no peaks, node
                               records, final configs (cas2; cas3 head: the unwidened configs << 11), budgets
                               1 .. 12 (cas3 mid).  Every key_width is above the register tier's 10 and no key
                               is handed past T2 (deep_keys 0)
  (k) test_wide_hbm*           + 62: launch_t3_wide, the live ops in window slots 62 .. 65; probes, final
                               configs (cas2; cas3 head: the unwidened configs << 62, slot bits in both words),
                               budgets 1 .. 3.  Every key passes slot 55; deep_keys = keys
  (l) test_wgl_widened, test_competition_widened
  (m) test_stream_set_*        + 11, one row of each key in turn: k_stream_migrate, then k_stream_set /
                               k_stream_set_exact on every key (cas2 in one stream, cas3 mid in streams of
                               2,048 keys); reports in the append the decided-prefix rule names, key_tier
                               set / dead, deferred_at, nothing deferred or fallen back, exact: peaks and
                               final configs against (j)'s one-shot run
  (n) test_stream_without_the_set_tier   cas2 + 11 mid: dead before the inert block or answered by finish

lc_stats.lds_keys (keys_done in Device.check's stats) counts the keys finished
in any tier, the HBM tiers included, so it says that every key was answered,
not where: the tier follows from key_width -- the register tier's kernels
return K_SPILL above 10, every narrow tier K_WIDE at an invoke into slot 56 or
higher -- together with deep_keys.

Out of these scopes' reach still: T2, the narrow HBM tier and the layered tier
(reached only by outgrowing T1, which no small history does), mutex4 (no inert
op: a crashed acquire or release is legal in some state) and table models.

A key the device gets wrong is printed as op maps (Loaded.same)."""
import time

import numpy as np
import pytest

import cref
import linear_ref as LR
import small_scope as SS
import stream_helpers as S
from helpers import oracle_state_value
from lincheck import _native as N
from lincheck import parallel as P
from lincheck.checker import Device, Packed, PinnedRecords
from lincheck.stream import Stream

pytestmark = pytest.mark.gpu

BUDGET = 1 << 20
BUDGET_CAUSE = 2
OFF = N.LC_PATH_SPLIT_OFF | N.LC_PATH_SPEC_OFF
# k_spec's workspaces are 3 * 16 * 64 words per key and segment (the exact
# builds: 2 * 18 * 64 more) and plan_step drops k_spec past 8 GiB of them:
# 8 segments hold 87,381 keys (exact: 49,932).  16,384 keys a call stay far
# below it, at 1.5 GiB (exact: 2.6 GiB) of workspace.
SPEC_BATCH = 16384
# plan_step cuts at quiescent points only batches of at most cu_count * 8 keys
# (256 CUs on the MI355X)
SEG_BATCH = 256 * 8
MASK48 = (1 << 48) - 1

_devs = {}


def dev(**kw) -> Device:
    """One context per option set for the whole module (lc_create allocates)."""
    key = tuple(sorted(kw.items()))
    if key not in _devs:
        _devs[key] = Device(0, **kw)
    return _devs[key]


class Loaded:
    """A scope -- or, with n_inert and place, small_scope.widened of it --
    packed, with its oracle records; prep times in .prep (s)."""

    def __init__(self, name, n_inert=0, place=None):
        t0 = time.perf_counter()
        self.b = SS.widened(SS.scope(name), n_inert, place) if n_inert else SS.scope(name)
        self.scope_name, self.n_inert, self.place = name, n_inert, place
        name = f"{name} + {n_inert} {place}" if n_inert else name
        self.name, self.model, self.mdl = name, self.b.scope.model, self.b.scope.model_obj()
        t1 = time.perf_counter()
        self.pk = Packed(self.b.hist, self.mdl)
        t2 = time.perf_counter()
        self._orc = {}
        self.orc = self.oracle(BUDGET)
        t3 = time.perf_counter()
        self.prep = {"enumerate+columns": t1 - t0, "pack": t2 - t1, "cref": t3 - t2}
        print(f"{name}: {self.pk.n_keys} keys, {len(self.b.hist)} rows; prep " +
              ", ".join(f"{k} {v:.2f} s" for k, v in self.prep.items()))
        assert self.pk.keys == list(range(self.b.n_keys))
        sc = self.b.scope
        assert ((self.orc["valid"] == 1).sum(), (self.orc["valid"] == 0).sum()) == (sc.valid, sc.invalid)
        assert not self.pk.view.trans_off  # one state numbering for the batch (state_values)
        self._batches = {}
        self._finals = None
        self.width = np.ctypeslib.as_array(self.pk.view.key_width, shape=(self.pk.n_keys,))

    def oracle(self, budget):
        if budget not in self._orc:
            keys, orc = cref.check_history(self.b.hist.as_c(), budget=budget, threads=8, model=self.model)
            assert keys.tolist() == list(range(self.b.n_keys))
            self._orc[budget] = orc
        return self._orc[budget]

    def batches(self, size):
        """[(lo, hi, Packed of keys lo .. hi)]: every key, in order."""
        if size not in self._batches:
            K = self.b.n_keys
            self._batches[size] = [(lo, min(K, lo + size), Packed(self.b.slice(lo, min(K, lo + size)), self.mdl))
                                   for lo in range(0, K, size)]
            assert sum(pk.n_keys for _, _, pk in self._batches[size]) == K
        return self._batches[size]

    def same(self, what, r, lo=0, hi=None, peak=False, budget=BUDGET):
        """r's valid / cause / fail_event (peak: and peak, but where the oracle
        gave up at the budget) equal the oracle's for keys lo .. hi."""
        orc = self.oracle(budget)[lo:hi]
        for f in ("valid", "cause", "fail_event") + (("peak",) if peak else ()):
            got = np.asarray(getattr(r, f))
            ok = got == orc[f]
            if f == "peak":
                ok |= orc["cause"] == BUDGET_CAUSE
            bad = np.flatnonzero(~ok)
            assert not len(bad), (f"{self.name}, {what}: {f} differs on {len(bad)} keys; device {got[bad[0]]}, oracle "
                                  f"{orc[f][bad[0]]} on {self.b.describe(lo + int(bad[0]))}\n"
                                  f"{self.b.ops(lo + int(bad[0]))}")

    def state_values(self, pk=None):
        """State id -> the restatement's state, of a batch with one shared table."""
        pk = pk or self.pk
        out = []
        for s in range(1 << 15):
            try:
                out.append(pk.state_value(0, s))
            except N.LincheckError:
                break
        return out

    def oracle_finals(self):
        """{key: set of (lo, hi) records} of every invalid key by
        oracle/linear_ref.py, in the device's layout (helpers.encode_finals)."""
        if self._finals is None:
            ids = {v: s for s, v in enumerate(self.state_values())}
            self._finals = {}
            for k in np.flatnonzero(self.orc["valid"] == 0).tolist():
                a = LR.analysis(self.b.ops(k), model=self.model)
                assert a.valid is False and a.fail_event == self.orc["fail_event"][k]
                recs = set()
                for st, L in a.final_configs:
                    mask = 0
                    for q in L:
                        mask |= 1 << a.final_slots[q]
                    # (lo = slots 0..63, hi = slots 64..111 | state << 48: helpers.encode_finals)
                    recs.add((mask & ((1 << 64) - 1), mask >> 64 | ids[oracle_state_value(st, self.model)] << 48))
                assert len(recs) == len(a.final_configs) <= 10
                self._finals[k] = recs
        return self._finals


_loaded = {}
KEEP_WIDENED = 3  # widened scopes kept at once (cas4p2 + 11 is 5.3 M rows): the tests below use them in groups


@pytest.fixture(scope="module")
def scopes():
    def load(name, n_inert=0, place=None) -> Loaded:
        key = (name, n_inert, place)
        if key not in _loaded:
            wide = [k for k in _loaded if k[1]]
            if n_inert and len(wide) >= KEEP_WIDENED:
                del _loaded[wide[0]]
            _loaded[key] = Loaded(name, n_inert, place)
        return _loaded[key]
    yield load
    _loaded.clear()
    _one.clear()
    _expect.clear()
    _devs.clear()
    SS.scope.cache_clear()


def same_finals(what, r, ref, ordered=True):
    """n_final and the records written, key by key (ordered=False: as sets --
    no key here has more than max_final configs, so none is cut)."""
    np.testing.assert_array_equal(r.n_final, ref.n_final, err_msg=f"{what}: n_final")
    assert r.n_final.max(initial=0) <= r.final.shape[1]
    live = np.arange(r.final.shape[1])[None, :] < r.n_final[:, None]
    bad = np.flatnonzero(((r.final != ref.final).any(axis=2) & live).any(axis=1)).tolist()
    if not ordered:
        bad = [k for k in bad if sorted(map(tuple, r.final[k, :r.n_final[k]].tolist())) !=
               sorted(map(tuple, ref.final[k, :r.n_final[k]].tolist()))]
    assert not bad, f"{what}: final configs differ on keys {bad[:8]}"


# ---------------------------------------------------------------- (a)
@pytest.mark.parametrize("name", SS.ORDER)
def test_unsegmented(scopes, name):
    L = scopes(name)
    r = dev(path_flags=OFF, count_probes=True).check(L.pk)
    assert r.stats["t0_path"] == "k_search_lattice"
    L.same("unsegmented, probes counted", r, peak=True)
    assert r.stats["probes"] == int(L.orc["probes"].sum())
    full = None
    for flags in (OFF, OFF | N.LC_PATH_EV32):
        d = dev(path_flags=flags)
        r = d.check(L.pk)
        assert r.stats["t0_path"] == "k_search_lattice"
        assert r.stats["ev_word_bytes"] == 4
        L.same(f"unsegmented {flags:#x}", r, peak=True)
        full = full or r
        same_finals(f"unsegmented {flags:#x} against {OFF:#x}", r, full)
        L.same(f"unsegmented {flags:#x}, verdicts only", d.check(L.pk, verdicts_only=True))
        x = dev(path_flags=flags, max_final=10).check(L.pk, peaks=False)
        assert x.stats["t0_path"] == "k_search_lattice"
        L.same(f"unsegmented {flags:#x}, exact", x)
        same_finals(f"unsegmented {flags:#x}, exact", x, full, ordered=False)
    if name in ("cas2", "cas3"):
        want = L.oracle_finals()
        fin = full.final.tolist()
        for k, recs in want.items():
            assert full.n_final[k] == len(recs), L.b.describe(k)
            assert {tuple(x) for x in fin[k][:len(recs)]} == recs, L.b.describe(k)


# ---------------------------------------------------------------- (b)
SPEC_RUNS = ([(f"segs {s}, ck {ck}", dict(spec_segs=s, **({"spec_ck": ck} if ck else {})))
              for s in (2, 4, 8) for ck in (None, (0, 0))] +
             [(f"segs 4, {what}", dict(spec_segs=4, path_flags=N.LC_PATH_SPLIT_OFF | f))
              for what, f in (("NOSTAGE", N.LC_PATH_SPEC_NOSTAGE), ("COST", N.LC_PATH_SPEC_COST),
                              ("NOPRIO", N.LC_PATH_SPEC_NOPRIO))])


@pytest.mark.parametrize("name", SS.ORDER)
def test_spec(scopes, name):
    L = scopes(name)
    for what, kw in SPEC_RUNS:
        d = dev(**dict(dict(path_flags=N.LC_PATH_SPLIT_OFF), **kw))
        for lo, hi, pk in L.batches(SPEC_BATCH):
            r = d.check(pk, verdicts_only=True)
            assert r.stats["t0_path"] == "k_spec", f"{name}, {what}, keys {lo}..{hi}"
            L.same(f"k_spec, {what}", r, lo, hi)


@pytest.mark.parametrize("name", SS.ORDER)
def test_spec_exact(scopes, name):
    L = scopes(name)
    ref_dev = dev(path_flags=OFF, max_final=10)
    for lo, hi, pk in L.batches(SPEC_BATCH):
        ref = ref_dev.check(pk, peaks=False)
        assert ref.stats["t0_path"] == "k_search_lattice"
        L.same("unsegmented, exact", ref, lo, hi)
        for segs in (2, 8):
            r = dev(path_flags=N.LC_PATH_SPLIT_OFF, spec_segs=segs, max_final=10).check(pk, peaks=False)
            assert r.stats["t0_path"] == "k_spec", f"{name}, exact, segs {segs}, keys {lo}..{hi}"
            L.same(f"k_spec exact, segs {segs}", r, lo, hi)
            same_finals(f"{name}, k_spec exact, segs {segs}, keys {lo}..{hi}", r, ref)


# ---------------------------------------------------------------- (c)
def taggable(pk) -> bool:
    """device_api.hip's rule for a batch the segments kernel can tag: one shared
    table of at most 6 states, nil first, and no op that installs nil."""
    if pk.view.trans_off or pk.view.init_state != 0:
        return False
    trans = N.carray(pk.view.trans, int(pk.view.n_trans), np.uint32)
    installs_nil = (((trans & 3) >= N.LC_T_WRITE) & ((trans >> 17) == 0)).any()
    n_states = 0
    try:
        while True:
            pk.state_value(0, n_states)
            n_states += 1
    except N.LincheckError:
        pass
    return n_states <= 6 and not installs_nil


@pytest.mark.parametrize("name", ["cas2", "cas3"])
def test_segments(scopes, name):
    L = scopes(name)
    tagged = 0
    for seg_len in (0, 1):
        d = dev(path_flags=N.LC_PATH_SPLIT_ON, seg_len=seg_len)
        for lo, hi, pk in L.batches(SEG_BATCH):
            r = d.check(pk, verdicts_only=True)
            if taggable(pk):
                tagged += 1
                assert r.stats["t0_path"] == "k_search_segments", f"{name}, seg_len {seg_len}, keys {lo}..{hi}"
            L.same(f"segments, seg_len {seg_len}, path {r.stats['t0_path']}", r, lo, hi)
    # {nil, 0, 1} and no write of nil: every batch is taggable
    assert tagged == 2 * len(L.batches(SEG_BATCH))


# ---------------------------------------------------------------- (d)
@pytest.mark.parametrize("name", SS.ORDER)
def test_default_path(scopes, name):
    L = scopes(name)
    d = dev()
    r = d.check(L.pk)
    L.same(f"default, path {r.stats['t0_path']}", r, peak=True)
    r = d.check(L.pk, verdicts_only=True)
    L.same(f"default, verdicts only, path {r.stats['t0_path']}", r)
    r = d.check(L.pk, peaks=False)
    L.same(f"default, no peaks, path {r.stats['t0_path']}", r)


# ---------------------------------------------------------------- (e)
@pytest.mark.parametrize("name", SS.ORDER)
def test_budgets(scopes, name):
    L = scopes(name)
    assert L.orc["peak"].max() <= 11
    for budget in range(1, 13):
        orc = L.oracle(budget)
        r = dev(path_flags=OFF, budget=budget).check(L.pk)
        L.same(f"budget {budget}", r, peak=True, budget=budget)
        unknown = orc["valid"] == -1
        assert (r.cause[r.valid == -1] == BUDGET_CAUSE).all() and (unknown == (orc["cause"] == BUDGET_CAUSE)).all()
        assert (r.fail_event[unknown] >= 0).all()
    assert not unknown.any()  # 12 is past every key's need: the largest |I| and |S'|
    assert (L.oracle(1)["valid"] == -1).any()


# ---------------------------------------------------------------- (f)
def wgl_same(L, budget, path_flags=0):
    """test_gpu_wgl.wgl_vs_oracle on a whole scope (its frontier loop as array
    operations): verdict, cause, failing event, cache size, frontier records."""
    what = f"{L.name}, wgl, budget {budget}, path_flags {path_flags:#x}"
    res = dev(budget=budget, algorithm=N.LC_ALGO_WGL, path_flags=path_flags).check(L.pk)
    keys, orc, fin, nf = cref.check_history_wgl(L.b.hist.as_c(), budget=budget, threads=8, model=L.model)
    assert keys.tolist() == L.pk.keys
    for f in ("valid", "cause", "fail_event"):
        bad = np.flatnonzero(getattr(res, f) != orc[f])
        assert not len(bad), (f"{what}: {f} differs on {len(bad)} keys; device {getattr(res, f)[bad[0]]}, oracle "
                              f"{orc[f][bad[0]]} on {L.b.describe(int(bad[0]))}\n{L.b.ops(int(bad[0]))}")
    done = np.isin(orc["cause"], [0, 1, 2])
    np.testing.assert_array_equal(res.peak[done], orc["peak"][done], err_msg=f"{what}: cache size")
    assert (res.analyzer == N.LC_ALGO_WGL).all()
    bad = orc["valid"] == 0
    np.testing.assert_array_equal(res.n_final[bad], nf[bad], err_msg=f"{what}: frontier size")
    assert nf.max() <= res.final.shape[1]
    live = bad[:, None] & (np.arange(res.final.shape[1])[None, :] < nf[:, None])
    lo, hi = res.final[..., 0][live], res.final[..., 1][live]
    want = fin[:, :res.final.shape[1]][live]
    sv = L.state_values()
    if L.model == "mutex":
        sv = [1 if v else None for v in sv]  # lc_pack interns locked as 1
    value = np.array([N.LC_NIL if v is None else v for v in sv], np.int64)
    assert np.array_equal(value[((hi >> np.uint64(48)) & np.uint64(0x7FFF)).astype(np.int64)], want[:, 2]), what
    assert np.array_equal(lo, want[:, 0].astype(np.uint64)), what
    assert np.array_equal(hi & np.uint64(MASK48), want[:, 1].astype(np.uint64) & np.uint64(MASK48)), what
    return res, orc


WGL_RUNS = [(1 << 20, 0), (1, 0), (2, 0), (3, 0), (5, 0), (1 << 20, N.LC_PATH_WGL_EV_HBM)]


@pytest.mark.parametrize("budget,path_flags", WGL_RUNS, ids=[f"budget{b}-{f:#x}" for b, f in WGL_RUNS])
@pytest.mark.parametrize("name", SS.ORDER)
def test_wgl(scopes, name, budget, path_flags):
    L = scopes(name)
    _, orc = wgl_same(L, budget, path_flags)
    if budget == 1 << 20:
        sc = L.b.scope
        assert ((orc["valid"] == 1).sum(), (orc["valid"] == 0).sum()) == (sc.valid, sc.invalid)
    elif budget == 1:
        assert (orc["valid"] == -1).any()  # the budget is met, on every scope


def competition_same(L):
    """test_gpu_wgl.test_competition_answers_budget_keys_with_wgl's rule at a
    budget of 1: :linear's record where it has one, WGL's verdict (analyzer
    :wgl) for the keys :linear gives up on at the budget."""
    name = L.name
    budget = 1
    lin = L.oracle(budget)
    _, wgl, _, _ = cref.check_history_wgl(L.b.hist.as_c(), budget=budget, threads=8, model=L.model)
    r = dev(budget=budget, algorithm=N.LC_ALGO_COMPETITION).check(L.pk)
    gave_up = (lin["valid"] == -1) & (lin["cause"] == BUDGET_CAUSE)
    assert gave_up.any() and (gave_up & (wgl["valid"] != -1)).any() and not gave_up.all()
    want_an = np.where(gave_up, N.LC_ALGO_WGL, N.LC_ALGO_LINEAR)
    bad = np.flatnonzero(r.analyzer != want_an)
    assert not len(bad), f"{name}: analyzer {r.analyzer[bad[0]]} on {L.b.describe(int(bad[0]))}"
    for f in ("valid", "cause", "fail_event"):
        # (the rule pins a :wgl key's verdict; its cause and event are test_wgl's business)
        want = np.where(gave_up, wgl[f] if f == "valid" else getattr(r, f), lin[f])
        bad = np.flatnonzero(getattr(r, f) != want)
        assert not len(bad), (f"{name}, competition: {f} differs on {len(bad)} keys; device {getattr(r, f)[bad[0]]}, "
                              f"oracles {want[bad[0]]} on {L.b.describe(int(bad[0]))}")


@pytest.mark.parametrize("name", SS.ORDER)
def test_competition(scopes, name):
    competition_same(scopes(name))


# ---------------------------------------------------------------- (g)
class Records:
    def __init__(self, rec):
        self.valid, self.cause, self.fail_event = P.unpack_records(np.asarray(rec).astype(np.int64))


@pytest.mark.parametrize("name", SS.ORDER)
def test_node_records(scopes, name):
    L = scopes(name)
    K = L.pk.n_keys
    d = dev()
    db = d.upload(L.pk)
    db.check_node(K)
    L.same("upload + check_node", Records(d.node_records(K)))
    rec, _st = d.check_node(L.pk, K)
    L.same("check_node from the host", Records(rec))
    bufs = [PinnedRecords(K) for _ in range(3)]
    for b in bufs:
        d.check_node_async(L.pk, K, b)
    d.wait()
    for i, b in enumerate(bufs):
        L.same(f"check_node_async, buffer {i}", Records(b))


# ---------------------------------------------------------------- (h), (i)
@pytest.fixture(scope="module")
def merged(scopes):
    """cas3, one row of each key in turn; when each key's events are decided
    (stream_helpers.Restated) and leg (a)'s one-shot records."""
    L = scopes("cas3")
    t0 = time.perf_counter()
    rr = L.b.round_robin()
    rs = S.Restated(rr, 0)
    print(f"cas3 merged: round robin + Restated {time.perf_counter() - t0:.2f} s")
    one = dev(path_flags=OFF).check(L.pk)
    L.same("one shot", one, peak=True)
    # the one-shot final configs of every invalid key with register values for state ids
    sv = [-1 if v is None else v for v in L.state_values()]
    one.by_value = {k: sorted((lo, hi & MASK48, sv[hi >> 48]) for lo, hi in one.final[k, :one.n_final[k]].tolist())
                    for k in np.flatnonzero(L.orc["valid"] == 0).tolist()}
    return L, rr, rs, one


@pytest.mark.parametrize("exact,set_tier", [(False, False), (True, False), (False, True), (True, True)],
                         ids=["plain", "exact", "set_tier", "exact+set_tier"])
def test_stream(merged, exact, set_tier):
    """Appended n_keys rows at a time.  A key is reported by the append that
    decides its failing :ok -- the append that holds the failing row when every
    op invoked before it has completed or crashed by then, else the one that
    brings the last such completion, or `finish` for an op left open (the
    decided-prefix rule, stream_helpers.Restated) -- and never earlier or
    later; a valid key is never reported."""
    L, rr, rs, one = merged
    K, orc = L.pk.n_keys, L.orc
    step = K
    bad = np.flatnonzero(orc["valid"] == 0)
    ready = np.array([rs.ready[int(k)][int(orc["fail_event"][k])] for k in bad])
    row = np.array([rs.events[int(k)][int(orc["fail_event"][k])][3] for k in bad])
    n_calls = -(-len(rr) // step)
    due = np.where(ready >= S.NEVER, n_calls, (np.minimum(ready, len(rr)) - 1) // step)  # n_calls: at finish
    assert (due[ready == row + 1] == row[ready == row + 1] // step).all()
    assert (ready == row + 1).sum() > 10_000 and (ready >= S.NEVER).sum() > 1_000 and (due > row // step).sum() > 10_000
    s = Stream(dev(), L.mdl, set_tier=set_tier, exact=exact)
    reported = {}

    def after(n_rows, up):
        call = (n_rows - 1) // step
        for i in up.invalid:
            assert i not in reported, f"key {i} reported twice"
            reported[i] = call

    S.feed(s, rr, step, after)
    up = s.finish()
    for i in up.invalid:
        assert i not in reported, f"key {i} reported twice"
        reported[i] = n_calls
    assert s.keys == L.pk.keys
    assert up.n_deferred == 0
    got = np.array([reported.get(int(k), -1) for k in bad])
    wrong = np.flatnonzero(got != due)
    assert not len(wrong), (f"{len(wrong)} keys reported in another call: call {got[wrong[0]]}, due {due[wrong[0]]} "
                            f"({n_calls}: finish) on {L.b.describe(int(bad[wrong[0]]))}")
    assert set(reported) == set(bad.tolist()), "a valid key was reported"
    res = s.results()
    L.same(f"stream exact={exact} set_tier={set_tier}", res, peak=exact)
    if exact:
        np.testing.assert_array_equal(res.n_final, one.n_final)
        # the stream numbers a key's states itself: configs compared by register value
        fin_s = res.final[bad].tolist()
        for k, fin in zip(bad.tolist(), fin_s):
            value = {}
            for _lo, hi in fin[:len(one.by_value[k])]:
                if hi >> 48 not in value:
                    v = s.state_value(k, hi >> 48)
                    value[hi >> 48] = -1 if v is None else v
            got_k = sorted((lo, hi & MASK48, value[hi >> 48]) for lo, hi in fin[:len(one.by_value[k])])
            assert got_k == one.by_value[k], L.b.describe(k)
    else:
        assert res.peak is None and res.final is None
    s.close()


def test_row_order(merged):
    L, rr, _rs, one = merged
    pk = Packed(rr, L.mdl)
    assert pk.keys == L.pk.keys
    r = dev(path_flags=OFF).check(pk)
    L.same("round robin, unsegmented", r, peak=True)
    same_finals("round robin against key-major", r, one)
    r = dev().check(pk, verdicts_only=True)
    L.same(f"round robin, default, path {r.stats['t0_path']}", r)


# ---------------------------------------------------------------- (j) .. (n): the set tiers
# small_scope.widened: 11 inert ops put every key past the register tier's 10
# pending ops, 62 past the narrow config's 56 window slots; the records stay
# the unwidened key's (tests/test_small_scope.py), the oracle here is cref on
# the widened history itself.
T0_MAX_WIDTH = 10          # lattice_core.hpp: a key_width above it is K_SPILL before the first event
DIRECT_T3_WIDTH = 28       # device_search.hpp LC_DIRECT_T3_WIDTH: wider keys skip T1 / T2
NARROW_MAX_SLOTS = 56      # an :invoke with a window slot >= 56 is K_WIDE in every narrow tier
# The wide tier's per-block workspace is sized from the budget (ensure_ws):
# 2^20 would reserve tables for a million configs a block where every set here
# has at most 11 (|I| at most 12: leg (e)).  4096 is a power of two far above
# both and small for the workspace; the oracle runs at the same budget.
WIDE_BUDGET = 4096
WIDE_SCOPES = ("cas2", "cas3", "cas4p2", "reg4")


def took(what, L, t0):
    print(f"{L.name}, {what}: {L.pk.n_keys} keys, {time.perf_counter() - t0:.2f} s")


def in_t1(L, r, what):
    """The set tier T1 answered every key: none fits the register tier (its
    kernels return K_SPILL on key_width alone), none is wide enough to skip
    T1, every key was finished (lc_stats.lds_keys, which Device.check names
    keys_done, counts the keys finished in any tier) and none was handed past
    T2 (deep_keys)."""
    assert L.width.min() > T0_MAX_WIDTH and L.width.max() <= DIRECT_T3_WIDTH, what
    print(f"{L.name}, {what}: keys_done {r.stats['keys_done']}, deep_keys {r.stats['deep_keys']}, t0_path {r.stats['t0_path']}")
    assert r.stats["keys_done"] == L.pk.n_keys and r.stats["deep_keys"] == 0, what


def in_wide(L, r, what):
    """The wide HBM tier answered every key: every key's window passes slot
    55, where each narrow tier returns K_WIDE, and all of them went to the
    HBM tier (deep_keys)."""
    assert L.width.min() > NARROW_MAX_SLOTS and L.width.max() <= 112, what
    print(f"{L.name}, {what}: keys_done {r.stats['keys_done']}, deep_keys {r.stats['deep_keys']}, t3_bytes {r.stats['t3_bytes']}")
    assert r.stats["deep_keys"] == L.pk.n_keys and r.stats["keys_done"] == L.pk.n_keys, what


def finals_same(L, r, what, want=None):
    """n_final and the records of every invalid key, both words, against
    linear_ref.analysis on the widened ops (want: against those records).  (A
    key of two ops fails with no pending op linearized, so cas2's masks are all
    0 and its records differ by state alone.)"""
    want = L.oracle_finals() if want is None else want
    assert len(want) == L.b.scope.invalid
    fin = r.final.tolist()
    for k, recs in want.items():
        assert r.n_final[k] == len(recs), f"{what}: {L.b.describe(k)}"
        assert {tuple(x) for x in fin[k][:len(recs)]} == recs, f"{what}: {L.b.describe(k)}\n{L.b.ops(k)}"


def shifted_finals(L0, L):
    """The final configs of a scope widened at `head`, from the unwidened
    scope's (Loaded.oracle_finals, linear_ref.analysis): the inert invokes come
    first and hold slots 0 .. n_inert - 1 for good, so every live op has its
    unwidened slot + n_inert (tests/test_small_scope.py asserts it from the
    packed words of every key) and a config its unwidened mask << n_inert, with
    the same register value.  Returns the records and the highest bit set."""
    assert L.place == "head"
    n = L.n_inert
    value = L0.state_values()
    ids = {v: s for s, v in enumerate(L.state_values())}
    out, top = {}, 0
    for k, recs in L0.oracle_finals().items():
        out[k] = set()
        for lo, hi in recs:
            assert hi & MASK48 == 0
            mask = lo << n
            top = max(top, mask.bit_length())
            out[k].add((mask & ((1 << 64) - 1), mask >> 64 | ids[value[hi >> 48]] << 48))
        assert len(out[k]) == len(recs)
    return out, top


def budget_leg(L, r, budget, what):
    """Leg (e)'s assertions at one budget; returns the oracle's unknown keys."""
    orc = L.oracle(budget)
    L.same(what, r, peak=True, budget=budget)
    unknown = orc["valid"] == -1
    assert (r.cause[r.valid == -1] == BUDGET_CAUSE).all() and (unknown == (orc["cause"] == BUDGET_CAUSE)).all()
    assert (r.fail_event[unknown] >= 0).all()
    return unknown


# ---------------------------------------------------------------- (j)
@pytest.mark.parametrize("place", SS.PLACES)
@pytest.mark.parametrize("name", WIDE_SCOPES)
def test_t1(scopes, name, place):
    L = scopes(name, 11, place)
    K = L.pk.n_keys
    t0 = time.perf_counter()
    d = dev(count_probes=True)
    r = d.check(L.pk)
    in_t1(L, r, "T1")
    L.same("T1, probes counted", r, peak=True)
    assert r.stats["probes"] == int(L.orc["probes"].sum())
    if place == "mid":
        x = d.check(L.pk, verdicts_only=True)
        in_t1(L, x, "T1, verdicts only")
        L.same("T1, verdicts only", x)
        x = d.check(L.pk, peaks=False)
        in_t1(L, x, "T1, no peaks")
        L.same("T1, no peaks", x)
        same_finals(f"{L.name}, T1, no peaks", x, r, ordered=False)
    if name == "cas3" and place == "mid":
        dn = dev()
        db = dn.upload(L.pk)
        db.check_node(K)
        L.same("T1, upload + check_node", Records(dn.node_records(K)))
    if name == "cas2" and place != "mid":
        finals_same(L, r, "T1")
    if name == "cas3" and place == "head":  # configs with pending ops linearized: slot bits 11 .. 13
        want, top = shifted_finals(scopes("cas3"), L)
        assert top == 11 + 3
        finals_same(L, r, "T1, against the unwidened configs << 11", want)
    took("T1", L, t0)


@pytest.mark.parametrize("budget", [1, 2, 3, 5, 12])
def test_t1_budgets(scopes, budget):
    L = scopes("cas3", 11, "mid")
    t0 = time.perf_counter()
    r = dev(budget=budget).check(L.pk)
    in_t1(L, r, f"T1, budget {budget}")
    unknown = budget_leg(L, r, budget, f"T1, budget {budget}")
    assert unknown.any() if budget == 1 else not unknown.any() if budget == 12 else True
    took(f"T1, budget {budget}", L, t0)


# ---------------------------------------------------------------- (k)
WIDE_RUNS = [("cas2", p) for p in SS.PLACES] + [("cas3", "head"), ("cas3", "tail"), ("reg4", "head")]


@pytest.mark.parametrize("name,place", WIDE_RUNS)
def test_wide_hbm(scopes, name, place):
    L = scopes(name, 62, place)
    t0 = time.perf_counter()
    orc = L.oracle(WIDE_BUDGET)
    assert not (orc["valid"] == -1).any()
    r = dev(count_probes=True, budget=WIDE_BUDGET).check(L.pk)
    in_wide(L, r, "wide HBM tier")
    L.same("wide HBM tier", r, peak=True, budget=WIDE_BUDGET)
    assert r.stats["probes"] == int(orc["probes"].sum())
    if name == "cas2" and place != "mid":
        finals_same(L, r, "wide HBM tier")
    if name == "cas3" and place == "head":  # slot bits 62 .. 64: both words of a wide config
        want, top = shifted_finals(scopes("cas3"), L)
        assert top == 62 + 3
        finals_same(L, r, "wide HBM tier, against the unwidened configs << 62", want)
    took("wide HBM tier", L, t0)


@pytest.mark.parametrize("budget", [1, 2, 3])
def test_wide_hbm_budgets(scopes, budget):
    L = scopes("cas2", 62, "head")
    t0 = time.perf_counter()
    r = dev(budget=budget).check(L.pk)
    in_wide(L, r, f"wide HBM tier, budget {budget}")
    unknown = budget_leg(L, r, budget, f"wide HBM tier, budget {budget}")
    assert unknown.any() or budget > 1
    took(f"wide HBM tier, budget {budget}", L, t0)


# ---------------------------------------------------------------- (l)
@pytest.mark.parametrize("name,n_inert,place", [("cas2", 11, "head"), ("cas2", 62, "head"), ("cas3", 11, "mid")])
def test_wgl_widened(scopes, name, n_inert, place):
    L = scopes(name, n_inert, place)
    for budget, path_flags in ((1 << 20, 0), (3, 0), (1 << 20, N.LC_PATH_WGL_EV_HBM)):
        t0 = time.perf_counter()
        _, orc = wgl_same(L, budget, path_flags)
        if budget == 1 << 20:
            sc = L.b.scope
            assert ((orc["valid"] == 1).sum(), (orc["valid"] == 0).sum()) == (sc.valid, sc.invalid)
        took(f"wgl, budget {budget}, path_flags {path_flags:#x}", L, t0)


def test_competition_widened(scopes):
    L = scopes("cas3", 11, "mid")
    t0 = time.perf_counter()
    competition_same(L)
    took("competition, budget 1", L, t0)


# ---------------------------------------------------------------- (m), (n)
# A set record is STREAM_SET_REC_WORDS * 4 = 524,608 bytes and the pool grows
# by chunks of 4 << c slots: a stream in which 2,048 keys migrate holds at most
# 4,092 slots, 2.15 GB; all of cas3 at once would be about 49 GB.
STREAM_BATCH = 2048
_one, _expect = {}, {}


def one_shot(L):
    """The one-shot T1 records of a scope + 11, and every invalid key's final
    configs with register values for state ids (as the fixture `merged`)."""
    if L.name not in _one:
        one = dev(count_probes=True).check(L.pk)
        in_t1(L, one, "one shot")
        L.same("one shot", one, peak=True)
        sv = [-1 if v is None else v for v in L.state_values()]
        one.by_value = {k: sorted((lo, hi & MASK48, sv[hi >> 48]) for lo, hi in one.final[k, :one.n_final[k]].tolist())
                        for k in np.flatnonzero(L.orc["valid"] == 0).tolist()}
        _one[L.name] = one
    return _one[L.name]


def stream_expect(L, lo, hi):
    """Keys lo .. hi, one row of each in turn, and from stream_helpers.Restated
    on those rows: the append that decides each invalid key's failing :ok
    (n_calls: finish), each key's defer_at and event count."""
    if (L.name, lo, hi) not in _expect:
        rr = L.b.round_robin(lo, hi)
        rs = S.Restated(rr, 0)
        assert rs.keys == list(range(lo, hi)) and not rs.error
        orc, step = L.orc[lo:hi], hi - lo
        bad = np.flatnonzero(orc["valid"] == 0)
        ready = np.array([rs.ready[lo + int(k)][int(orc["fail_event"][k])] for k in bad], np.int64)
        row = np.array([rs.events[lo + int(k)][int(orc["fail_event"][k])][3] for k in bad], np.int64)
        n_calls = -(-len(rr) // step)
        due = np.where(ready >= S.NEVER, n_calls, (np.minimum(ready, len(rr)) - 1) // step)
        assert (due[ready == row + 1] == row[ready == row + 1] // step).all()
        defer_at = np.array([rs.defer_at[k] for k in range(lo, hi)], np.int64)
        n_ev = np.array([len(rs.events[k]) for k in range(lo, hi)], np.int64)
        assert (defer_at >= 0).all()  # every key takes window slot 10 in its inert block
        _expect[L.name, lo, hi] = (rr, n_calls, bad, due, defer_at, n_ev)
    return _expect[L.name, lo, hi]


def stream_leg(L, lo, hi, exact, set_tier, one=None):
    """One stream over keys lo .. hi, appended as many rows at a time as it has
    keys; test_stream's assertions, and where each key was searched."""
    rr, n_calls, bad, due, defer_at, n_ev = stream_expect(L, lo, hi)
    K, step, orc = hi - lo, hi - lo, L.orc[lo:hi]
    what = f"{L.name}, keys {lo}..{hi}, stream exact={exact} set_tier={set_tier}"
    # alive when its migrating invoke is searched: valid, or failing at or after it
    reaches = (orc["valid"] != 0) | (orc["fail_event"].astype(np.int64) >= defer_at)
    if not set_tier:  # past the register tier a key waits for finish
        due = np.where(reaches[bad], n_calls, due)
    s = Stream(dev(), L.mdl, set_tier=set_tier, exact=exact)
    try:
        reported = {}

        def after(n_rows, up):
            call = (n_rows - 1) // step
            for i in up.invalid:
                assert i not in reported, f"{what}: key {lo + i} reported twice"
                reported[i] = call

        S.feed(s, rr, step, after)
        up = s.finish()
        for i in up.invalid:
            assert i not in reported, f"{what}: key {lo + i} reported twice"
            reported[i] = n_calls
        assert s.keys == list(range(lo, hi))
        got = np.array([reported.get(int(k), -1) for k in bad])
        wrong = np.flatnonzero(got != due)
        assert not len(wrong), (f"{what}: {len(wrong)} keys reported in another call: call {got[wrong[0]]}, due "
                                f"{due[wrong[0]]} ({n_calls}: finish) on {L.b.describe(lo + int(bad[wrong[0]]))}")
        assert set(reported) == set(bad.tolist()), f"{what}: a valid key was reported"
        t = s.tiers()
        tier = [s.key_tier(i) for i in range(K)]
        assert sum(t.values()) == K and all(t[name] == tier.count(name) for name in t)
        if set_tier:
            assert up.n_deferred == 0 and t["fallen_back"] == 0, f"{what}: {up}, {t}"
            at = np.array([s.key_events(i)["deferred_at"] for i in range(K)], np.int64)
            moved = np.flatnonzero(reaches & (defer_at < n_ev - 1))
            wrong = [int(i) for i in moved if tier[i] not in ("set", "dead") or at[i] != defer_at[i]]
            assert not wrong, (f"{what}: {len(wrong)} keys not in the set tier: tier {tier[wrong[0]]}, deferred_at "
                               f"{at[wrong[0]]}, expected {defer_at[wrong[0]]} on {L.b.describe(lo + wrong[0])}")
            # every invalid key is dead, every valid one that migrated is still in the set tier
            assert t["dead"] == len(bad) and t["set"] >= int((orc["valid"][moved] == 1).sum())
            st = s.set_stats()
            assert st["pool_in_use"] == t["set"] and st["pool_peak"] >= t["set"]
        else:
            # The packer counts a key as deferred when it emits the invoke that takes slot 10
            # (host_stream.cpp drain), and every key's rows hold one.  A key is dead iff it was
            # reported online, before that invoke; every other key is checked at finish.
            assert up.n_deferred == K, f"{what}: {up}"
            assert t == {"register": 0, "set": 0, "fallen_back": int(reaches.sum()), "dead": K - int(reaches.sum())}, t
            assert s.set_stats()["pool_slots"] == 0
        res = s.results()
        L.same(what, res, lo, hi, peak=exact)
        if exact:
            np.testing.assert_array_equal(res.n_final, one.n_final[lo:hi])
            fin_s = res.final[bad].tolist()
            for k, fin in zip(bad.tolist(), fin_s):
                want = one.by_value[lo + k]
                value = {}
                for _lo, hi_w in fin[:len(want)]:
                    if hi_w >> 48 not in value:
                        v = s.state_value(k, hi_w >> 48)
                        value[hi_w >> 48] = -1 if v is None else v
                got_k = sorted((lo_w, hi_w & MASK48, value[hi_w >> 48]) for lo_w, hi_w in fin[:len(want)])
                assert got_k == want, f"{what}: {L.b.describe(lo + k)}"
        else:
            assert res.peak is None and res.final is None
        return dict(t, n_deferred=up.n_deferred, reaches=int(reaches.sum()), online=int((due < n_calls).sum()),
                    at_finish=int((due == n_calls).sum()))
    finally:
        s.close()


MODES = [(False, True), (True, True)]
MODE_IDS = ["set_tier", "exact+set_tier"]


@pytest.mark.parametrize("exact,set_tier", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("place", SS.PLACES)
def test_stream_set_cas2(scopes, place, exact, set_tier):
    """cas2 + 11, all 2,119 keys in one stream: every key migrates
    (k_stream_migrate) and is searched on in the resident set tier
    (k_stream_set, exact: k_stream_set_exact)."""
    L = scopes("cas2", 11, place)
    t0 = time.perf_counter()
    got = stream_leg(L, 0, L.pk.n_keys, exact, set_tier, one_shot(L) if exact else None)
    assert got["online"] > 100
    print(got)
    took(f"stream exact={exact} set_tier={set_tier}", L, t0)


@pytest.mark.parametrize("exact,set_tier", MODES, ids=MODE_IDS)
def test_stream_set_cas3(scopes, exact, set_tier):
    """cas3 + 11 mid, all 93,367 keys, 2,048 keys a stream (the pool's memory:
    STREAM_BATCH), each stream closed before the next opens."""
    L = scopes("cas3", 11, "mid")
    K = L.pk.n_keys
    one = one_shot(L) if exact else None
    t0 = time.perf_counter()
    total = {}
    for lo in range(0, K, STREAM_BATCH):
        got = stream_leg(L, lo, min(K, lo + STREAM_BATCH), exact, set_tier, one)
        for k, v in got.items():
            total[k] = total.get(k, 0) + v
    print(total)
    assert total["dead"] == L.b.scope.invalid and total["fallen_back"] == 0
    assert total["online"] > 10_000 and total["at_finish"] > 1_000
    took(f"stream exact={exact} set_tier={set_tier}, {-(-K // STREAM_BATCH)} streams", L, t0)


@pytest.mark.parametrize("exact", [False, True], ids=["plain", "exact"])
def test_stream_without_the_set_tier(scopes, exact):
    """cas2 + 11 mid with the set tier off: a key whose failing :ok is decided
    before its inert block is reported online, every other key waits for
    `finish` and is answered there through the batch path."""
    L = scopes("cas2", 11, "mid")
    t0 = time.perf_counter()
    got = stream_leg(L, 0, L.pk.n_keys, exact, False, one_shot(L) if exact else None)
    print(got)
    assert got["online"] > 100 and got["at_finish"] > 100
    took(f"stream exact={exact} set_tier=False", L, t0)
