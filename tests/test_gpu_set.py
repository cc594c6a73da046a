"""lc_set_check on the GPU: every case compares each key's full result map
(:valid?, the six counts, the four interval strings) with jepsen.checker/set
restated with Python sets (tests/set_helpers.py), on every path the key can
take: the LDS tier (spans up to 65,536 ids) and the HBM tier (wider keys, and
every key under LC_PATH_SET_HBM), the latter with k_set_mark's LDS tile and
without it (LC_PATH_SET_DIRECT)."""
import ctypes as C
import random

import numpy as np
import pytest

import set_helpers as SH
from lincheck import _native as N
from lincheck import checker as ck
from lincheck import independent
from lincheck import setcheck as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def devs(device):
    """The paths by name: the library's own choice, every key through HBM, and
    both with the mark kernel's tile form off."""
    return {"auto": ck.Device(0), "hbm": ck.Device(0, path_flags=N.LC_PATH_SET_HBM),
            "direct": ck.Device(0, path_flags=N.LC_PATH_SET_DIRECT),
            "hbm-direct": ck.Device(0, path_flags=N.LC_PATH_SET_HBM | N.LC_PATH_SET_DIRECT)}


@pytest.fixture(scope="module")
def info():
    out = np.zeros(7, np.int64)
    N.check(N.lib().lc_set_launch_info(N.ptr(out, C.c_int64)))
    return dict(zip("lane wave block lds floor mark_rows mark_tile".split(), out.tolist()))


def maps(dev, hist):
    packed = S.PackedSet(hist)
    res = S.check_batch(dev, packed.view)
    return packed, res, {k: S.result_map(packed, res, i) for i, k in enumerate(packed.keys)}


def agree(devs, hist, want, paths=("auto", "hbm", "hbm-direct")):
    out = None
    for p in paths:
        packed, res, got = maps(devs[p], hist)
        assert list(got) == list(want)
        for k in want:
            assert SH.same(got[k], want[k]), (p, k, got[k], want[k])
        out = (packed, res)
    return out


def ranges(*rs):
    return [x for a, b in rs for x in range(a, b + 1)]


def test_hand_example(devs):
    ops = SH.hand_ops()
    agree(devs, S.SetHistory.from_ops(ops), {None: SH.HAND_WANT})
    assert SH.restate(ops) == SH.HAND_WANT


def test_random_keys_one_batch(devs):
    """300 keys x up to 64 adds, with never-read, empty-read and error keys."""
    rng = random.Random(77)
    ops = []
    for i in range(60):
        ops += SH.random_history(rng, max_keys=5, max_adds=64, keyed=True, key_base=1000 * i)
    while len(SH.keys_of(ops)) < 300:
        ops += SH.random_history(rng, max_keys=5, max_adds=64, keyed=True, key_base=1000 * (100 + len(ops)))
    want = SH.restate_independent(ops)
    kinds = {(w.get("valid?"), w.get("error")) for w in want.values()}
    assert {True, False, "unknown"} <= {k[0] for k in kinds} and len([k for k in kinds if k[0] == "unknown"]) == 2
    agree(devs, S.SetHistory.from_ops(ops), want)


def boundary_sets(bounds, shift, low):
    """Two keys: runs that cross each boundary, and runs of one class that end
    on the bit before it with a run of another class starting on it.  low:
    the key's least element (ids are offsets from it).  The attempts repeat
    one element often enough for the keys to keep offset ids (set_plan.hpp)."""
    pad = [low] * (5 * (shift + max(bounds)) // 64 + 100)
    cross = ranges(*[(shift + b - 3, shift + b + 2) for b in bounds])
    a1 = (cross + pad, cross, cross + [low])  # ok runs across every boundary
    ok = ranges(*[(shift + b - 3, shift + b - 1) for b in bounds])
    lost = ranges(*[(shift + b, shift + b + 2) for b in bounds])
    unexpected = ranges(*[(shift + b + 3, shift + b + 4) for b in bounds])
    recovered = ranges(*[(shift + b + 5, shift + b + 5) for b in bounds])
    a2 = (ok + lost + recovered + pad, ok + lost, ok + unexpected + recovered + [low])
    return a1, a2


def test_run_boundaries(devs, info):
    """Bits 31|32, 63|64, 127|128, a lane's 16-byte chunk, a wave's and a
    workgroup's chunk of k_set_classify: a run across each is one run, and
    runs of different classes that meet there stay two."""
    bounds = sorted({32, 64, 128, info["lane"], 2 * info["lane"], info["wave"], info["block"]})
    assert info["block"] + 64 < info["lds"]
    small = boundary_sets(bounds, 0, 0)                   # fits the LDS tier
    large = boundary_sets(bounds, 2 * info["block"], 0)   # 3 workgroups of the HBM tier
    hist = SH.hist_of_sets(list(small) + list(large))
    want = SH.restate_hist(hist)
    assert want[0]["ok"].count("..") == len(bounds) and want[0]["ok-count"] == 6 * len(bounds) + 1
    assert want[1]["lost"].count("..") == len(bounds) and want[1]["recovered-count"] == len(bounds) + 1
    packed, _ = agree(devs, hist, want)
    a = packed.arrays()
    assert a["rank"].tolist() == [0, 0, 0, 0] and a["min"].tolist() == [0, 0, 0, 0]
    assert all(s <= info["lds"] for s in a["span"][:2]) and all(s > info["lds"] for s in a["span"][2:])


def test_one_run_over_three_workgroups(devs, info):
    n = 3 * info["block"] + 100
    el = list(range(n))
    hist = SH.hist_of_sets([(el, el, el)])
    want = SH.restate_hist(hist)
    assert want[None]["ok"] == f"#{{0..{n - 1}}}" and want[None]["valid?"] is True
    _, res = agree(devs, hist, want)
    assert len(res.runs) == 1


def test_alternating_bits_scan(devs, info):
    """Every other element: as many runs as the span allows (the scan's and
    the capacity protocol's worst case)."""
    n = 3 * info["block"] + 100
    ev = list(range(0, n, 2))
    hist = SH.hist_of_sets([(ev, ev[: len(ev) // 2], ev)])
    want = SH.restate_hist(hist)
    _, res = agree(devs, hist, want)
    assert len(res.runs) == len(ev) + len(ev) - len(ev) // 2  # ok + recovered


def test_adjacent_keys_do_not_bridge(devs):
    k0 = ranges((0, 0), (100, 127))  # span 128: the last bit of the key's last word
    k1 = ranges((0, 5))              # bit 0 of the next key's first word
    hist = SH.hist_of_sets([(k0, k0, k0), (k1, k1, k1)])
    want = SH.restate_hist(hist)
    assert want[0]["ok"] == "#{0 100..127}" and want[1]["ok"] == "#{0..5}"
    packed, res = agree(devs, hist, want)
    a = packed.arrays()
    assert a["span"].tolist() == [128, 6] and a["base"].tolist() == [0, 2]


def test_rank_keys(devs):
    big = SH.I64_MAX
    wide = [-5, 0, 1, 2, 10 ** 12, 10 ** 12 + 1, big - 1, big]
    # the plan boundary: 1,000 attempt rows are 5,000 bytes = 208 bitmap words = 13,312 ids
    inside = list(range(999)) + [13311]
    outside = list(range(999)) + [13312]
    plain = list(range(50))
    hist = SH.hist_of_sets([(wide, wide[:-1], wide[1:]), (inside, [], [5, 13311]), (outside, [], [5, 13312]),
                            (plain, plain, plain)])
    want = SH.restate_hist(hist)
    assert want[0]["ok"] == f"#{{0..2 {10 ** 12}..{10 ** 12 + 1} {big - 1}..{big}}}" and want[0]["lost"] == "#{-5}"
    packed, _ = agree(devs, hist, want)
    assert packed.arrays()["rank"].tolist() == [1, 0, 1, 0]


def test_rank_key_wider_than_the_lds_tier(devs, info):
    """A rank key of more ids than the LDS tier takes: adjacency from vals
    across lanes and workgroups of k_set_classify."""
    n = info["lds"] + info["block"]
    el = sorted([1000 * i for i in range(n)] + [1000 * i + 1 for i in range(0, n, 2)])  # runs of two and of one
    hist = SH.hist_of_sets([(el, el[::2], el[1:])])
    want = SH.restate_hist(hist)
    packed, _ = agree(devs, hist, want, paths=("auto",))
    a = packed.arrays()
    assert a["rank"].tolist() == [1] and a["span"][0] > info["lds"]


def test_mark_monotone_and_shuffled(devs, info):
    """About 100,000 adds from (range), in order and shuffled, and a read in
    another order: the same records."""
    n = 100_000
    rng = np.random.default_rng(5)
    el = np.arange(n)
    lost = set(rng.choice(n, 7, replace=False).tolist())
    final = [x for x in el.tolist() if x not in lost] + [n + 3, n + 4]
    sh = rng.permutation(el).tolist()
    h1 = SH.hist_of_sets([(el.tolist(), el.tolist(), final)])
    h2 = SH.hist_of_sets([(sh, sh[::-1], final[::-1])])
    want = SH.restate_hist(h1)
    assert want == SH.restate_hist(h2) and want[None]["lost-count"] == 7 and want[None]["unexpected"] == f"#{{{n + 3}..{n + 4}}}"
    _, r1 = agree(devs, h1, want, paths=("auto", "direct"))   # the tile form, the lanes' own atomics
    _, r2 = agree(devs, h2, want, paths=("direct", "auto"))   # no chunk fits a tile: the fallback inside the tile build
    assert np.array_equal(r1.runs, r2.runs) and np.array_equal(r1.counts, r2.counts)


def test_mark_chunks_at_the_tile_limit(devs, info):
    """Workgroups of k_set_mark whose ids span exactly a tile, one word more,
    and far more, in one key: the same records with and without the tile."""
    rows, tile = info["mark_rows"], info["mark_tile"]
    chunks = []
    for base, width in ((0, tile), (3 * tile, tile + 32), (8 * tile + 5, tile - 5), (12 * tile, 4 * tile)):
        ids = [base, base + width - 1] + [base + (7 * i) % width for i in range(rows - 2)]
        chunks.append(ids)
    attempts = [x for c in chunks for x in c]
    assert len(attempts) == 4 * rows
    acks = attempts[::3]
    final = sorted(set(attempts))[::2] + [16 * tile + 1]
    hist = SH.hist_of_sets([(attempts, acks, final)])
    want = SH.restate_hist(hist)
    packed, _ = agree(devs, hist, want, paths=("hbm", "hbm-direct", "auto"))
    assert packed.arrays()["rank"].tolist() == [0]


def test_run_cap_too_small(devs):
    hist = S.SetHistory.from_ops(SH.hand_ops())
    packed = S.PackedSet(hist)
    for dev in devs.values():
        K = 1
        valid, counts, run_off = np.zeros(K, np.int8), np.zeros(6 * K, np.uint64), np.zeros(4 * K + 1, np.uint64)
        runs = np.full(2 * 8, -7, np.int64)
        r = N.LcSetResult(N.ptr(valid, C.c_int8), N.ptr(counts, C.c_uint64), N.ptr(run_off, C.c_uint64),
                          N.ptr(runs, C.c_int64), 3, 0)
        rc = N.lib().lc_set_check(dev.handle, C.byref(packed.view), C.byref(r))
        assert rc == -2 and r.n_runs == 6 and b"run_cap >= 6" in N.lib().lc_last_error()
        assert (runs == -7).all(), "no runs written"
        r.run_cap = r.n_runs
        N.check(N.lib().lc_set_check(dev.handle, C.byref(packed.view), C.byref(r)))
        assert runs[:12].reshape(6, 2).tolist() == [[0, 2], [4, 8], [3, 3], [20, 20], [30, 30], [8, 8]]
        assert run_off.tolist() == [0, 2, 4, 5, 6] and counts.tolist() == [11, 9, 8, 2, 1, 1] and valid[0] == 0


def test_bad_id_in_a_caller_built_batch(devs):
    ops = SH.random_history(random.Random(3), max_keys=4, max_adds=40, keyed=True)
    while len(SH.keys_of(ops)) < 3:
        ops = SH.random_history(random.Random(len(ops)), max_keys=4, max_adds=40, keyed=True)
    hist = S.SetHistory.from_ops(ops)
    packed = S.PackedSet(hist)
    want = SH.restate_independent(ops)
    for name, dev in devs.items():
        a = packed.arrays()
        k = next(i for i in range(packed.n_keys) if a["add_off"][i + 1] > a["add_off"][i])
        a["add_id"][int(a["add_off"][k])] = a["span"][k]  # one id past the key's span
        with pytest.raises(N.LincheckError, match=f"invalid.*key {k}:"):
            S.check_batch(dev, S.batch_of(a))
        res = S.check_batch(dev, packed.view)  # the context is fine afterwards
        for i, key in enumerate(packed.keys):
            assert SH.same(S.result_map(packed, res, i), want[key]), (name, key)
    # the host's own checks: offsets that go back, a key's words past the batch's
    a = packed.arrays()
    a["read_off"][1] = a["read_off"][-1] + 5
    with pytest.raises(N.LincheckError, match="offsets not ascending"):
        S.check_batch(devs["auto"], S.batch_of(a))
    a = packed.arrays()
    a["n_words"] = 0
    with pytest.raises(N.LincheckError, match="bitmap words"):
        S.check_batch(devs["auto"], S.batch_of(a))


def test_interleaved_with_a_register_check(devs):
    from lincheck import history as H
    dev = devs["auto"]
    h1 = S.synth_set(n_keys=5, adds_per_key=300, info_rate=0.05, lost_rate=0.02, unexpected_rate=0.01, seed=1)
    h2 = S.synth_set(n_keys=3, adds_per_key=500, info_rate=0.1, seed=2, shuffle=True)
    reg = ck.Packed(H.synth(n_keys=16, ops_per_key=100, concurrency=5, anomaly_rate=0.2, seed=3))
    before = dev.check(reg)
    _, _, got1 = maps(dev, h1)
    mid = dev.check(reg)
    _, _, got2 = maps(dev, h2)
    assert got1 == SH.restate_hist(h1) and got2 == SH.restate_hist(h2)
    assert np.array_equal(before.valid, mid.valid) and np.array_equal(before.fail_event, mid.fail_event)
    assert (mid.valid == 0).any()


def test_demo_end_to_end(tmp_path, devs):
    """The demo's call: history.edn of a single-key set run -> read_edn ->
    checker.set_().check -> the result map."""
    h = S.synth_set(n_keys=1, adds_per_key=3000, concurrency=10, info_rate=0.02, lost_rate=0.002, unexpected_rate=0.001,
                    seed=11)
    ops = h.to_ops()
    path = tmp_path / "history.edn"
    path.write_text(SH.edn_lines(ops))
    want = SH.restate(ops)
    assert want["valid?"] is False and want["lost-count"] > 0 and want["unexpected-count"] == 3
    hist = S.SetHistory.read_edn(str(path))
    assert ck.set_().check({}, hist, {}) == want
    assert ck.set is ck.set_ and ck.set_({"path-flags": N.LC_PATH_SET_HBM}).check({}, ops, {}) == want


def test_independent_checker_batches_the_set_checker(devs):
    h = S.synth_set(n_keys=6, adds_per_key=200, info_rate=0.05, lost_rate=0.01, seed=4)
    ops = h.to_ops()
    want = SH.restate_independent(ops)
    out = independent.checker(ck.set_()).check({}, ops, {})
    assert out["results"] == want
    assert out["failures"] == [k for k, w in want.items() if w["valid?"] is False]
    assert out["valid?"] == ck.merge_valid([w["valid?"] for w in want.values()])
    comp = independent.checker(ck.compose({"set": ck.set_(), "optimism": ck.unbridled_optimism()})).check({}, ops, {})
    for k, w in want.items():
        assert comp["results"][k]["set"] == w and comp["results"][k]["optimism"] == {"valid?": True}
        assert comp["results"][k]["valid?"] == w["valid?"]
