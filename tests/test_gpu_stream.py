"""The incremental check on the device (lc_stream_*: k_stream in
device_stream_lattice.hip, csrc/host_stream.cpp).  Expected values always come from
the oracle (oracle/linear_ref.c through cref) or from Device.check one-shot:
a stream fed a history in pieces must end with the records of the one-shot
check, and after every call the set of invalid keys must be exactly the keys
whose searched prefix holds the oracle's failing :ok.

Kernel edges go through `push` (events mode): slices of an lc_pack'ed
tests/edgegen.py batch, cut where edgegen.pending_before says the walk's
state is at one of its seams."""
import ctypes as C

import numpy as np
import pytest

import cref
import edgegen as E
import stream_helpers as S
from lincheck import _native as N
from lincheck import history as H
from lincheck.checker import Device, Packed
from lincheck.stream import Stream

pytestmark = pytest.mark.gpu

INVALID, ERROR = 1, 2          # a record's status word (csrc/stream_plan.hpp)
H_STATUS, H_N, H_DONE, H_FAIL = 0, 1, 5, 6


NEVER = np.int64(1) << 40


def failing(orc):
    """The oracle's failing event of every invalid key, NEVER for the others."""
    return np.where(orc["valid"] == 0, orc["fail_event"].astype(np.int64), NEVER)


@pytest.fixture(scope="module")
def dev():
    return Device(0)


class Source:
    """An lc_pack'ed batch to cut chunks from, and the oracle's records for it."""

    def __init__(self, hist, pk):
        self.pk = pk
        keys, self.orc = cref.check_history(hist.as_c(), budget=1 << 20, threads=8)
        assert list(keys) == pk.keys
        v = pk.view
        K = pk.n_keys
        self.ev = [pk.events(i) for i in range(K)]
        self.nev = np.array([len(e) for e in self.ev], np.int64)
        self.width = N.carray(v.key_width, K, np.uint8)
        self.states = N.carray(v.key_states, K, np.uint16)
        self.trans = N.carray(v.trans, int(v.n_trans), np.uint32)
        self.trans_off = N.carray(v.trans_off, K, np.uint32) if v.trans_off else None
        self.init_state = int(v.init_state)
        # no key may be deferred or refused: all of them fit the register tier
        assert (self.width <= 10).all() and (self.states <= 32).all() and (E.batch_states(pk) <= 32).all()
        self.fev = failing(self.orc)

    def chunk(self, parts, words16=False, patch=None):
        """parts: [(key index, lo, hi)]; an LcBatch of those keys' words lo .. hi and its key ids."""
        ks = [k for k, _lo, _hi in parts]
        words = [self.ev[k][lo:hi] for k, lo, hi in parts]
        if patch:
            words = patch(words)
        off = np.concatenate([[0], np.cumsum([len(w) for w in words])]).astype(np.uint64)
        ev = np.ascontiguousarray(np.concatenate(words + [np.zeros(1, np.uint32)]), np.uint32)
        b = N.LcBatch()
        b.n_keys = len(parts)
        b.ev_off = N.ptr(off, C.c_uint64)
        keep = [off, ev]
        if words16:
            e16 = np.ascontiguousarray(((ev >> 16) & 0x8000) | (((ev >> 24) & 0x7F) << 11) | (ev & 0xFFFFFF), np.uint16)
            b.events16 = N.ptr(e16, C.c_uint16)
            keep.append(e16)
        else:
            b.events = N.ptr(ev, C.c_uint32)
        b.trans, b.n_trans = N.ptr(self.trans, C.c_uint32), len(self.trans)
        kw = np.ascontiguousarray(self.width[ks] if ks else np.zeros(1, np.uint8))
        kst = np.ascontiguousarray(self.states[ks] if ks else np.zeros(1, np.uint16))
        b.key_width, b.key_states = N.ptr(kw, C.c_uint8), N.ptr(kst, C.c_uint16)
        keep += [kw, kst]
        if self.trans_off is not None:
            to = np.ascontiguousarray(self.trans_off[ks] if ks else np.zeros(1, np.uint32))
            b.trans_off = N.ptr(to, C.c_uint32)
            keep.append(to)
        b.init_state = self.init_state
        b._keep = keep
        return b, [self.pk.keys[k] for k in ks]


_src = {}


def source(name):
    if name not in _src:
        if name == "small":  # whole keys pushed one event at a time
            cases = [("k60-7-valid", E.rolling(60, 7)), ("k60-9-garbage", E.rolling(60, 9).with_anomalies((40, "garbage"))),
                     ("k60-5-stale", E.dips(60, 5, 1, [30]).with_anomalies((45, "stale"))),
                     ("k61-10-valid", E.rolling(61, 10)), ("k2", E.tiny(2)), ("k0", E.tiny(0))]
            b = E.batch(cases, seed=21)
        else:
            b = E.get(name)
        _src[name] = Source(b.hist, b.pk)
    return _src[name]


def final_equal(s, src, label):
    res = s.results()
    assert res.keys == src.pk.keys
    for f in ("valid", "cause", "fail_event"):
        got, want = getattr(res, f), src.orc[f]
        bad = np.flatnonzero(got != want)
        assert not len(bad), f"{label}: {f} differs at keys {bad[:8]}: stream {got[bad[:8]]}, oracle {want[bad[:8]]}"


def push_schedule(dev, src, cuts, label, words16=False, first_call=None):
    """cuts[k]: ascending boundaries of key k; call j pushes key k's words
    cuts[k][j] .. cuts[k][j + 1] (nothing once its cuts are used up).
    first_call[k]: the call key k first appears in.  After every call the
    invalid keys are exactly those whose pushed prefix passes the oracle's
    failing event."""
    K = src.pk.n_keys
    s = Stream(dev)
    pushed = np.zeros(K, np.int64)
    pos = [0] * K
    invalid = set()
    n_calls = max(len(c) - 1 + (first_call or {}).get(k, 0) for k, c in enumerate(cuts))
    for j in range(n_calls):
        parts = []
        for k in range(K):
            if j < (first_call or {}).get(k, 0) or pos[k] + 1 >= len(cuts[k]):
                continue
            lo, hi = cuts[k][pos[k]], cuts[k][pos[k] + 1]
            pos[k] += 1
            parts.append((k, lo, hi))
            pushed[k] = hi
        b, ids = src.chunk(parts, words16)
        up = s.push(b, ids)
        index = {key: i for i, key in enumerate(s.keys)}
        turned = {src.pk.keys.index(s.keys[i]) for i in up.invalid}
        assert not (turned & invalid), f"{label}, call {j}: a key turned invalid twice"
        invalid |= turned
        want = {k for k in range(K) if pushed[k] > src.fev[k]}
        assert invalid == want, f"{label}, call {j}: invalid {sorted(invalid)}, oracle says {sorted(want)}"
        res = s.results()
        for k in turned:
            assert res.fail_event[index[src.pk.keys[k]]] == src.orc["fail_event"][k]
    return s


# ---------------------------------------------------------------- kernel edges
def seams(c, fev):
    """Boundaries of a key at the walk's seams, by name (the first of each)."""
    n = len(c) - 1
    out = {}

    def first(name, pred):
        for b in range(1, n):
            if pred(b):
                out.setdefault(name, b)
                return

    for p in range(1, 11):
        first(f"n={p}", lambda b, p=p: c[b] == p)
    first("n=0 again", lambda b: c[b] == 0)
    first("n=6, invoke next", lambda b: c[b] == 6 and c[b + 1] == 7)
    first("after the :ok back to 6", lambda b: c[b - 1] == 7 and c[b] == 6)
    first("n=9, first :ok back to registers", lambda b: c[b] == 9 and c[b + 1] == 8)
    first("n=10, :ok next", lambda b: c[b] == 10 and c[b + 1] == 9)
    first("lane :ok, :ok next", lambda b: c[b - 1] <= 6 and c[b] == c[b - 1] - 1 and c[b + 1] == c[b] - 1)
    first("holes in live", lambda b: 1 <= c[b] <= 5 and c[b - 1] == c[b] + 1 and max(c[:b]) >= c[b] + 2)
    if fev < n:
        out["before the failing :ok"] = fev
        if fev + 1 < n:
            out["after the failing :ok"] = fev + 1
    return out


WANTED = [f"n={p}" for p in range(1, 11)] + ["n=0 again", "n=6, invoke next", "after the :ok back to 6",
                                             "n=9, first :ok back to registers", "n=10, :ok next", "lane :ok, :ok next",
                                             "holes in live", "before the failing :ok", "after the failing :ok"]


@pytest.mark.parametrize("name", ["profiles", "anomalies", "states32"])
def test_cuts_at_every_seam_of_the_walk(dev, name):
    src = source(name)
    cuts, seen = [], set()
    for k in range(src.pk.n_keys):
        c = E.pending_before(src.pk, k).tolist()
        sm = seams(c, int(src.fev[k]) if src.fev[k] < (1 << 40) else len(c))
        seen |= set(sm)
        cuts.append(sorted({0, len(c) - 1} | set(sm.values())))
    if name == "profiles":
        assert not set(WANTED) - seen, f"no key is cut at: {sorted(set(WANTED) - seen)}"
    s = push_schedule(dev, src, cuts, name)
    final_equal(s, src, name)
    s.close()


@pytest.mark.parametrize("size", [63, 64, 65, 128, 129, 200])
def test_chunk_sizes_around_the_cursor(dev, size):
    """The walk's cursor keeps three 64-event chunks in flight.  One key first
    appears in the fifth call; 16-bit words in place for the even sizes."""
    src = source("profiles")
    cuts = [sorted(set(range(0, n, size)) | {int(n)}) for n in src.nev]
    s = push_schedule(dev, src, cuts, f"chunks of {size}", words16=size % 2 == 0, first_call={3: 4})
    assert s.keys[-1] == src.pk.keys[3], "key 3 joins the stream last, in its fifth call"
    res = s.results()
    order = [src.pk.keys.index(k) for k in s.keys]
    for f in ("valid", "cause", "fail_event"):
        assert np.array_equal(getattr(res, f), src.orc[f][order]), f
    s.close()


def test_one_event_per_push(dev):
    src = source("small")
    assert 60 in src.nev
    cuts = [list(range(int(n) + 1)) for n in src.nev]
    s = push_schedule(dev, src, cuts, "one event per push")
    final_equal_except_empty(s, src)
    s.close()


def final_equal_except_empty(s, src):
    """Keys without events never reach a stream in events mode."""
    res = s.results()
    for i, key in enumerate(res.keys):
        k = src.pk.keys.index(key)
        assert (res.valid[i], res.cause[i], res.fail_event[i]) == (src.orc["valid"][k], src.orc["cause"][k],
                                                                   src.orc["fail_event"][k]), key
    assert set(src.pk.keys) - set(res.keys) == {src.pk.keys[k] for k in range(src.pk.n_keys) if src.nev[k] == 0}


def test_records_follow_the_plan_and_a_dead_key_keeps_its_record(dev):
    src = source("profiles")
    dead = int(np.flatnonzero(src.fev < (1 << 40))[0])
    live = int(np.flatnonzero(src.orc["valid"] == 1)[0])
    f = int(src.fev[dead])
    s = Stream(dev)
    c_live = E.pending_before(src.pk, live)
    b, ids = src.chunk([(dead, 0, f + 1), (live, 0, 300)])
    up = s.push(b, ids)
    assert up.invalid == [0] and up.events == f + 1 + 300
    rec = s.record(0)
    assert (rec[H_STATUS], rec[H_FAIL], rec[H_DONE]) == (INVALID, f, f)
    r1 = s.record(1)
    assert (r1[H_STATUS], r1[H_N], r1[H_DONE]) == (0, c_live[300], 300)
    # more words for the dead key (and a key without new words beside it): nothing of its record moves
    b, ids = src.chunk([(dead, f + 1, f + 200), (live, 300, 300)])
    up = s.push(b, ids)
    assert up.invalid == [] and up.events == 0
    assert np.array_equal(s.record(0), rec) and np.array_equal(s.record(1), r1)
    b, ids = src.chunk([(live, 300, int(src.nev[live]))])
    s.push(b, ids)
    res = s.results()
    assert (res.valid[0], res.fail_event[0], res.valid[1]) == (0, f, 1)
    s.close()


# ---------------------------------------------------------------- rows mode
_hist = {}


def rows_case(name):
    if name not in _hist:
        if name == "A":
            h = H.synth(64, 200, concurrency=10, anomaly_rate=0.3, seed=7)
        elif name == "A-merged":
            h = S.merged_round_robin(rows_case("A")[0])
        elif name == "I":
            h = H.synth(24, 120, concurrency=10, interleave=True, nemesis_period=5.0, anomaly_rate=0.3, seed=3)
        elif name == "B":
            h = H.synth(12, 150, concurrency=10, interleave=True, nemesis_period=5.0, anomaly_rate=0.3, info_rate=0.02,
                        seed=3)
        keys, orc = cref.check_history(h.as_c(), budget=1 << 20, threads=8)
        _hist[name] = (h, list(keys), orc, S.Restated(h))
    return _hist[name]


def run_rows(dev, name, step, deferred=0):
    h, keys, orc, rs = rows_case(name)
    fev = failing(orc)
    s = Stream(dev)
    invalid = set()

    def after(n_rows, up):
        invalid.update(up.invalid)
        searched = [min(rs.emitted(k, n_rows), rs.defer_at[k] if rs.defer_at[k] >= 0 else 1 << 40) for k in keys[:up.n_keys]]
        want = {i for i, e in enumerate(searched) if e > fev[i]}
        assert invalid == want, f"{name}, {n_rows} rows: invalid {sorted(invalid)}, oracle says {sorted(want)}"

    S.feed(s, h, step or len(h), after)
    online = set(invalid)
    up = s.finish()
    assert up.n_deferred == deferred
    res = s.results()
    assert res.keys == keys
    for f in ("valid", "cause", "fail_event"):
        assert np.array_equal(getattr(res, f), orc[f]), f"{name}, step {step}: {f}"
    for i in np.flatnonzero(orc["valid"] == 0):
        assert s.failing_row(int(i)) == s.event_row(int(i), int(orc["fail_event"][i]))
    return s, online, orc


@pytest.mark.parametrize("step", [7, 64, 640, 0])
@pytest.mark.parametrize("name", ["A", "A-merged", "I"])
def test_rows_mode_online_and_final(dev, name, step):
    s, online, orc = run_rows(dev, name, step)
    n_bad = {"A": 8, "A-merged": 8, "I": 3}[name]
    assert (orc["valid"] == 0).sum() == n_bad and (orc["valid"] == 1).sum() == len(orc) - n_bad
    s.close()


def test_rows_mode_one_row_per_append(dev):
    s, _online, _orc = run_rows(dev, "I", 1)
    s.close()


def test_deferred_key_beside_online_verdicts(dev):
    """B: one key passes 10 pending ops and is checked at finish through the
    batch path; the two invalid keys are found online, and are not that key."""
    s, online, orc = run_rows(dev, "B", 50, deferred=1)
    deferred = [i for i in range(len(orc)) if s.key_events(i)["deferred_at"] >= 0]
    assert len(deferred) == 1 and len(online) == 2 and deferred[0] not in online
    assert online == set(np.flatnonzero(orc["valid"] == 0).tolist())
    s.close()


def test_every_key_deferred_at_a_small_budget():
    """D at budget 65,536: concurrency 30 defers all 8 keys; the final records
    are Device.check's at the same budget (some keys give up at it)."""
    h = H.synth(8, 300, concurrency=30, info_rate=0.02, anomaly_rate=0.5, seed=4)
    dev = Device(0, budget=65536)
    want = dev.check(Packed(h), verdicts_only=True)
    s = Stream(dev)
    S.feed(s, h, 500)
    up = s.finish()
    assert up.n_deferred == 8
    res = s.results()
    for f in ("valid", "cause", "fail_event"):
        assert np.array_equal(getattr(res, f), getattr(want, f)), f
    s.close()


# ---------------------------------------------------------------- refusals, malformed words, two streams
def test_malformed_push_costs_one_key(dev):
    """An :ok of a slot that is not pending: that key is ERROR, the call says
    LC_E_INVALID naming it, and the other keys are exact."""
    src = source("anomalies")
    K = src.pk.n_keys
    bad = 1

    def patch(words):
        w = words[bad].copy()
        free = (set(range(16)) - set(((w[:40] >> 24) & 0x7F).tolist())).pop()
        w[40] = 0x80000000 | (free << 24)
        words[bad] = w
        return words

    s = Stream(dev)
    b, ids = src.chunk([(k, 0, 500) for k in range(K)], patch=patch)
    with pytest.raises(N.LincheckError, match=r"invalid: .*key index 1 .*malformed"):
        s.push(b, ids)
    assert s.record(bad)[H_STATUS] == ERROR
    b, ids = src.chunk([(k, 500, int(src.nev[k])) for k in range(K)])
    s.push(b, ids)
    res = s.results()
    assert (res.valid[bad], res.cause[bad], res.fail_event[bad]) == (N.LC_UNKNOWN, N.LC_CAUSE_ERROR, -1)
    rest = [k for k in range(K) if k != bad]
    for f in ("valid", "cause", "fail_event"):
        assert np.array_equal(getattr(res, f)[rest], src.orc[f][rest]), f
    s.close()


def test_refusals(dev):
    with pytest.raises(N.LincheckError, match="unsupported"):
        Stream(Device(0, budget=16 * 64 * 32 - 1))
    src = source("anomalies")
    s = Stream(dev)
    b, ids = src.chunk([(0, 0, 10), (1, 0, 10)])
    wide = np.array([10, 11], np.uint8)
    b.key_width = N.ptr(wide, C.c_uint8)
    with pytest.raises(N.LincheckError, match="unsupported"):
        s.push(b, ids)
    assert s.keys == []
    b, ids = src.chunk([(0, 0, 10)])
    s.push(b, ids)
    with pytest.raises(N.LincheckError, match="events mode"):
        s.append(S.rows(rows_case("I")[0], 0, 5))
    s.close()


def test_two_streams_and_a_batch_check_share_a_context(dev):
    h, keys, orc, _rs = rows_case("A")
    hi, keysi, orci, _ = rows_case("I")
    pk = Packed(h)
    a, b = Stream(dev), Stream(dev)
    for lo in range(0, max(len(h), len(hi)), 2000):
        if lo < len(h):
            a.append(S.rows(h, lo, min(len(h), lo + 2000)))
        r = dev.check(pk, verdicts_only=True)
        assert np.array_equal(r.valid, orc["valid"]) and np.array_equal(r.fail_event, orc["fail_event"])
        if lo < len(hi):
            b.append(S.rows(hi, lo, min(len(hi), lo + 2000)))
    a.finish(), b.finish()
    for s, o in ((a, orc), (b, orci)):
        res = s.results()
        for f in ("valid", "cause", "fail_event"):
            assert np.array_equal(getattr(res, f), o[f]), f
        s.close()
