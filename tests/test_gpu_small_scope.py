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
    """A scope, packed, with its oracle records; prep times in .prep (s)."""

    def __init__(self, name):
        t0 = time.perf_counter()
        self.b = SS.scope(name)
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
                    recs.add((mask, ids[oracle_state_value(st, self.model)] << 48))
                assert len(recs) == len(a.final_configs) <= 10
                self._finals[k] = recs
        return self._finals


_loaded = {}


@pytest.fixture(scope="module")
def scopes():
    def load(name) -> Loaded:
        if name not in _loaded:
            _loaded[name] = Loaded(name)
        return _loaded[name]
    yield load
    _loaded.clear()
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


@pytest.mark.parametrize("name", SS.ORDER)
def test_competition(scopes, name):
    """test_gpu_wgl.test_competition_answers_budget_keys_with_wgl's rule at a
    budget of 1: :linear's record where it has one, WGL's verdict (analyzer
    :wgl) for the keys :linear gives up on at the budget."""
    L = scopes(name)
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
