"""lc_setfull_check on the GPU: every case compares each key's full result map
and every per-id field (outcome, latency, known, last-absent) exactly with the
fold of tests/setfull_helpers.py (jepsen.checker/set-full restated; parity
unpinned), on both forms of the mark kernel and under caps that band the keys."""
import ctypes as C
import random

import numpy as np
import pytest

import setfull_helpers as H
from lincheck import _native as N
from lincheck import checker as ck
from lincheck import independent
from lincheck import setfull as F
from lincheck.independent import Tuple

pytestmark = pytest.mark.gpu

DIRECT = N.LC_SETFULL_MARK_DIRECT


@pytest.fixture(scope="module")
def dev(device):
    return ck.Device(0)


@pytest.fixture(scope="module")
def info():
    out = np.zeros(6, np.int64)
    N.check(N.lib().lc_setfull_launch_info(N.ptr(out, C.c_int64)))
    return dict(zip("wave block mark_els lane_els tile cap".split(), out.tolist()))


def run(dev, ops, lin=False, cap=0, flags=0):
    packed = F.PackedSetFull(F.SetFullHistory.from_ops(ops))
    return packed, F.check_batch(dev, packed.view, lin, cap, flags)


def agree(dev, ops, lin=False, cap=0, flags=0, want=None):
    """Device = fold for every key: the result map and every per-id field."""
    want = want or H.restate_independent(ops, lin)
    packed, res = run(dev, ops, lin, cap, flags)
    assert packed.keys == list(want)
    for i, k in enumerate(packed.keys):
        r, per = want[k]
        got = F.result_map(packed, res, i)
        assert H.same(got, r), (k, got, r)
        if "error" not in r:
            assert H.per_element(packed, res, i) == per, k
    return packed, res, want


def keyed(groups):
    """Several keys' ops (key, ops) one after the other as one tuple history."""
    out = []
    for k, ops in groups:
        out += [dict(o, value=Tuple(k, o["value"])) if o["f"] in ("add", "read") else dict(o) for o in ops]
    return out


def grid_key(rng, n_el, n_reads, elements=None, p_hold=0.8):
    """n_el acknowledged adds with n_reads reads spread between and after
    them, each holding a random share of what was added so far."""
    els = list(range(n_el)) if elements is None else list(elements)
    at = sorted(rng.randint(0, n_el) for _ in range(n_reads))
    ops, t = [], 0
    for i in range(n_el + 1):
        for _ in range(at.count(i)):
            ops.append(H.op("invoke", "read", None, 5, t))
            ops.append(H.op("ok", "read", [e for e in els[:i] if rng.random() < p_hold], 5, t + 2))
            t += 3
        if i < n_el:
            ops.append(H.op("invoke", "add", els[i], i % 5, t))
            ops.append(H.op("ok", "add", els[i], i % 5, t + 1))
            t += 2
    return ops


def test_hand_example(dev):
    ops = H.hand_ops()
    packed, res, want = agree(dev, ops, lin=True)
    got = F.result_map(packed, res, 0)
    assert {k: got[k] for k in H.HAND_WANT} == H.HAND_WANT
    assert [w["element"] for w in got["worst-stale"]] == H.HAND_WORST
    assert H.per_element(packed, res, 0) == H.HAND_PER
    assert res.counts[0].tolist() == [7, 4, 1, 2, 2, 1] and res.valid.tolist() == [N.LC_INVALID]
    assert ck.set_full({"linearizable?": True}).check({}, ops, {}) == got


def test_hand_example_under_independent(dev):
    ops = keyed([(3, H.hand_ops()), (4, H.hand_ops()[:14])])
    out = independent.checker(ck.set_full({"linearizable?": True})).check({}, ops, {})
    want = H.restate_independent(ops, True)
    assert list(out["results"]) == [3, 4]
    for k in (3, 4):
        assert H.same(out["results"][k], want[k][0]), k
    assert {k: out["results"][3][k] for k in H.HAND_WANT} == H.HAND_WANT
    assert out["failures"] == [3, 4] and out["valid?"] is False  # key 4 holds 3 twice
    comp = independent.checker(ck.compose({"set": ck.set_full(), "optimism": ck.unbridled_optimism()})).check({}, ops, {})
    assert H.same(comp["results"][3]["set"], H.restate_independent(ops, False)[3][0])
    assert comp["results"][3]["optimism"] == {"valid?": True} and comp["results"][3]["valid?"] is False


@pytest.fixture(scope="module")
def many_keys():
    """At least 300 random keys as one tuple history, and the fold's answers."""
    rng = random.Random(2024)
    ops = []
    for j in range(125):
        ops += H.random_history(rng, max_keys=5, keyed=True, key_base=1000 * j)
    return ops, {lin: H.restate_independent(ops, lin) for lin in (False, True)}


@pytest.mark.parametrize("lin", [False, True])
def test_random_keys_one_batch(dev, many_keys, lin):
    ops, want = many_keys
    checked = [k for k, (r, _) in want[lin].items() if "error" not in r]
    assert len(checked) >= 0.9 * len(want[lin]) and len(checked) >= 300
    packed, res, _ = agree(dev, ops, lin, want=want[lin])
    assert res.timing["passes"] == 1
    if lin:  # some key is invalid only because it is stale
        flipped = [k for k in checked if want[True][k][0]["valid?"] is False and want[False][k][0]["valid?"] is True]
        assert flipped


def test_id_and_row_edges(dev, info):
    """E around one wave's and one workgroup's ids, R around 64 rows, all in one
    batch: keys adjacent in the batch do not bleed into each other's words."""
    assert (info["wave"], info["block"]) == (64, 256)
    rng = random.Random(5)
    sizes = [1, 63, 64, 65, 129, info["block"] - 1, info["block"], info["block"] + 1]
    groups = [(100 * e + r, grid_key(rng, e, r)) for e in sizes for r in (0, 1, 2, 63, 64, 65)]
    ops = keyed(groups)
    want = H.restate_independent(ops, True, H.restate_matrix)
    agree(dev, ops, True, want=want)
    agree(dev, ops, True, flags=DIRECT, want=want)
    assert H.restate_independent(keyed(groups[:12]), True) == H.restate_independent(keyed(groups[:12]), True, H.restate_matrix)


def test_walk_stop_rule(dev):
    """The downward walk must not stop before an older row that was invoked
    later than it completed relative to the others."""
    def adds(els, t=0):
        out = []
        for e in els:
            out += [H.op("invoke", "add", e, 0, t), H.op("ok", "add", e, 0, t + 1)]
            t += 2
        return out, t
    base, t = adds([1, 2, 3, 4])
    # a read invoked first and completed last that alone holds 1 and alone misses 2; 3 is in every read, 4 in none
    ops = base + [H.op("invoke", "read", None, 5, t)]
    for j in range(70):
        ops += [H.op("invoke", "read", None, 6, t + 1 + 2 * j), H.op("ok", "read", [2, 3], 6, t + 2 + 2 * j)]
    ops += [H.op("ok", "read", [1, 3], 5, t + 200)]
    # 5: its first eligible row is the last row; 6: no eligible row
    tail = [H.op("invoke", "read", None, 7, t + 201), H.op("invoke", "add", 5, 1, t + 202), H.op("ok", "add", 5, 1, t + 203),
            H.op("ok", "read", [1, 2, 3, 5], 7, t + 204), H.op("invoke", "add", 6, 1, t + 205), H.op("ok", "add", 6, 1, t + 206)]
    _, _, want = agree(dev, ops + tail, True)
    per = want[None][1]
    assert per[1][0] == "stable" and per[2][0] == "stable" and per[3][0] == "stable" and per[4][0] == "lost"
    assert per[5] == ("stable", 0, len(ops) + 2, -1) and per[6] == ("never-read", -1, len(ops) + 5, -1)
    # without the tail the slow read decides: 1 is lost (every later invocation misses it), 2 is stable and stale
    _, _, want = agree(dev, ops, True)
    per = want[None][1]
    assert per[1][0] == "lost" and per[1][3] == len(ops) - 3
    assert per[2][0] == "stable" and per[2][1] > 0 and per[2][3] == len(base)
    assert per[3] == ("stable", 0, 5, -1) and per[4][0] == "lost"


def test_known_from_read_ack_or_neither(dev):
    ops = [H.op("invoke", "add", 1, 0, 0), H.op("invoke", "add", 2, 1, 1), H.op("invoke", "add", 3, 2, 2),
           H.op("invoke", "read", None, 5, 3), H.op("ok", "read", [1], 5, 4),  # 1 known by this read ...
           H.op("ok", "add", 1, 0, 5),                                          # ... before its ack
           H.op("ok", "add", 2, 1, 6),                                          # 2 known by its ack, read later
           H.op("info", "add", 3, 2, 7),                                        # 3 never known
           H.op("invoke", "read", None, 5, 8), H.op("ok", "read", [1, 2], 5, 9)]
    _, _, want = agree(dev, ops)
    per = want[None][1]
    assert per[1][2] == 4 and per[2][2] == 6 and per[3] == ("never-read", -1, -1, 8)


def test_bands_give_identical_results(dev, info):
    rng = random.Random(9)
    groups = [(1, grid_key(rng, 1500, 20)), (2, grid_key(rng, 70, 3)), (3, grid_key(rng, 600, 20, p_hold=0.97))]
    # a duplicate in a high band of key 1, and one in key 3
    groups[0][1].extend([H.op("invoke", "read", None, 6, 10 ** 6), H.op("ok", "read", [1400, 7, 1400, 1400], 6, 10 ** 6 + 1)])
    groups[2][1].extend([H.op("invoke", "read", None, 6, 10 ** 6), H.op("ok", "read", [599, 599], 6, 10 ** 6 + 1)])
    ops = keyed(groups)
    want = H.restate_independent(ops, True, H.restate_matrix)
    assert want[1][0]["duplicated"] == {1400: 3} and want[3][0]["duplicated"] == {599: 2}
    rows = 21
    seen = []
    for cap, passes in ((0, 1), (rows * 8 * 8, None), (rows * 4 * 8, None), (8, None)):
        packed, res, _ = agree(dev, ops, True, cap=cap, want=want)
        seen.append((res.timing["passes"], res))
        if passes:
            assert res.timing["passes"] == passes
    assert [p for p, _ in seen][0] == 1 and seen[1][0] >= 3 and seen[2][0] >= 5 and seen[3][0] >= seen[2][0]
    first = seen[0][1]
    for _, res in seen[1:]:
        for name in ("valid", "counts", "outcome", "latency", "known", "last_absent", "duplicated"):
            assert np.array_equal(getattr(res, name), getattr(first, name)), name


def big_key(reads, n=8300):
    """n acknowledged adds 0..n-1 (offset ids), then the given reads."""
    ops, t = [], 0
    for e in range(n):
        ops += [H.op("invoke", "add", e, e % 5, t), H.op("ok", "add", e, e % 5, t + 1)]
        t += 2
    for r in reads:
        ops += [H.op("invoke", "read", None, 5, t), H.op("ok", "read", r, 5, t + 1)]
        t += 2
    return ops


def test_mark_forms_at_the_tile_limit(dev, info):
    """Both forms of k_setfull_mark on monotone and shuffled ids, with one
    workgroup's ids spanning the LDS tile exactly, one id less and one more."""
    tile, els = info["tile"], info["mark_els"]
    assert (tile, els) == (8192, 4096)
    rng = random.Random(4)
    every_other = list(range(0, tile, 2))  # 4,096 elements over exactly the tile's ids
    shuffled = list(range(8300))
    rng.shuffle(shuffled)
    reads = [list(range(8300)), shuffled, every_other, every_other[:-1] + [tile - 1], every_other[:-1] + [tile],
             every_other[:-1] + [tile + 31], rng.sample(range(8300), 3000), list(range(100, 4196))]
    ops = big_key(reads)
    want = H.restate_independent(ops, True, H.restate_matrix)
    _, tiled, _ = agree(dev, ops, True, want=want)
    _, direct, _ = agree(dev, ops, True, flags=DIRECT, want=want)
    assert want[None][0]["attempt-count"] == 8300 and not want[None][0]["duplicated"]
    for name in ("valid", "counts", "outcome", "latency", "known", "last_absent", "duplicated"):
        assert np.array_equal(getattr(tiled, name), getattr(direct, name)), name
    packed = F.PackedSetFull(F.SetFullHistory.from_ops(ops))
    assert packed.arrays()["rank"].tolist() == [0] and packed.arrays()["span"].tolist() == [8300]


def test_rank_keys(dev):
    big = (1 << 63) - 1
    els = [-5, 10 ** 12, big]
    ops = keyed([(1, grid_key(random.Random(1), 3, 4, elements=els)),
                 (2, grid_key(random.Random(2), 40, 6, elements=[-big + 7 * i * 10 ** 15 for i in range(40)]))])
    ops += [dict(H.op("invoke", "read", None, 6, 10 ** 5), value=Tuple(1, None)),
            dict(H.op("ok", "read", [big, -5, big, 77], 6, 10 ** 5 + 1), value=Tuple(1, [big, -5, big, 77]))]
    packed, res, want = agree(dev, ops, True)
    assert packed.arrays()["rank"].tolist() == [1, 1] and packed.arrays()["span"].tolist() == [4, 40]
    assert want[1][0]["duplicated"] == {big: 2} and want[1][0]["attempt-count"] == 3


def test_duplicates_in_one_load_and_across_workgroups(dev, info):
    n = info["mark_els"] + 904
    reads = [[7, 7, 8, 9, 9, 9, 10],                  # inside one 16-byte load, and across two
             list(range(n)) + [7, 4100, 11],          # 7 and 11 again in the row's second workgroup, 4100 inside it
             list(range(n)),
             [20000, 3, 20000]]                       # an element nobody added
    ops = big_key(reads, n=5000)
    want = H.restate_independent(ops, False, H.restate_matrix)
    assert want[None][0]["duplicated"] == {7: 2, 9: 3, 11: 2, 4100: 2, 20000: 2}
    for flags in (0, DIRECT):
        packed, res, _ = agree(dev, ops, flags=flags, want=want)
        assert res.counts[0, 5] == 5 and res.valid[0] == N.LC_INVALID
        assert int(res.duplicated.sum()) == 5


def test_bad_id_in_a_caller_built_batch(dev):
    rng = random.Random(8)
    ops = keyed([(k, grid_key(rng, 30, 4)) for k in (1, 2, 3)])
    packed = F.PackedSetFull(F.SetFullHistory.from_ops(ops))
    want = H.restate_independent(ops)
    for flags in (0, DIRECT):
        a = packed.arrays()
        r = int(a["row_off"][1]) + 3
        a["read_id"][int(a["el_off"][r])] = a["span"][1]  # one id past key 1's span
        with pytest.raises(N.LincheckError, match="invalid.*key 1:"):
            F.check_batch(dev, F.batch_of(a), flags=flags)
        good = packed.arrays()  # (kept alive: the batch points into it)
        res = F.check_batch(dev, F.batch_of(good), flags=flags)  # the context is fine afterwards
        for i, k in enumerate(packed.keys):
            assert H.same(F.result_map(packed, res, i), want[k][0]) and H.per_element(packed, res, i) == want[k][1]
    # the host's own checks
    a = packed.arrays()
    a["row_off"][1] = a["row_off"][-1] + 5
    with pytest.raises(N.LincheckError, match="offsets not ascending"):
        F.check_batch(dev, F.batch_of(a))
    a = packed.arrays()
    a["row_pos"][1], a["row_pos"][2] = a["row_pos"][2], a["row_pos"][1]
    with pytest.raises(N.LincheckError, match="completion order"):
        F.check_batch(dev, F.batch_of(a))
    a = packed.arrays()
    a["id_off"][1:] -= 1
    with pytest.raises(N.LincheckError, match="fewer per-id entries"):
        F.check_batch(dev, F.batch_of(a))


def test_interleaved_with_register_and_set_checks(dev):
    from lincheck import history as Hist
    from lincheck import setcheck as S
    import set_helpers as SH
    h1 = F.synth_set_full(n_keys=4, adds_per_key=300, read_every=50, stale_window=5, lost_rate=0.02, overlap=True, seed=1)
    h2 = F.synth_set_full(n_keys=2, adds_per_key=500, read_every=100, info_rate=0.05, seed=2)
    hs = S.synth_set(n_keys=3, adds_per_key=400, info_rate=0.05, lost_rate=0.02, seed=3)
    reg = ck.Packed(Hist.synth(n_keys=16, ops_per_key=100, concurrency=5, anomaly_rate=0.2, seed=3))
    before = dev.check(reg)
    agree(dev, h1.to_ops(), True, want=H.restate_independent(h1.to_ops(), True, H.restate_matrix))
    packed = S.PackedSet(hs)
    res = S.check_batch(dev, packed.view)
    assert {k: S.result_map(packed, res, i) for i, k in enumerate(packed.keys)} == SH.restate_hist(hs)
    mid = dev.check(reg)
    agree(dev, h2.to_ops(), False, want=H.restate_independent(h2.to_ops(), False, H.restate_matrix))
    assert np.array_equal(before.valid, mid.valid) and np.array_equal(before.fail_event, mid.fail_event)
    assert (mid.valid == 0).any()


def test_history_edn_end_to_end(tmp_path, dev):
    """history.edn of a set run with intermediate reads -> read_edn ->
    compose({"perf": perf(), "set": set_full({"linearizable?": true})})."""
    h = F.synth_set_full(n_keys=1, adds_per_key=2000, read_every=100, stale_window=3, lost_rate=0.002, overlap=True, seed=11)
    ops = h.to_ops()
    path = tmp_path / "history.edn"
    path.write_text(H.edn_lines(ops))
    want, _ = H.restate_independent(ops, True, H.restate_matrix)[None]
    assert want["valid?"] is False and want["lost-count"] > 0 and want["stale-count"] > 0
    hist = F.SetFullHistory.read_edn(str(path))
    out = ck.compose({"perf": ck.perf(), "set": ck.set_full({"linearizable?": True})}).check({}, hist.to_ops(), {})
    assert out["perf"] == {"valid?": True} and out["valid?"] is False
    assert H.same(out["set"], want)
    assert H.same(ck.set_full({"linearizable?": True, "max-matrix-bytes": 4096, "flags": DIRECT}).check({}, hist, {}), want)
