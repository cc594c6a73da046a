"""lc_setfull_stream_* on the GPU.  After EVERY append each case compares the
stream -- per-key valid and counts, per element (by value) outcome, latency,
known, last-absent and the duplicated multiplicities -- with the one-shot
device check (lc_setfull_pack + lc_setfull_check) of the prefix AND with the
fold of tests/setfull_helpers.py.  Shapes are the smallest that cross the
kernels' edges: a wave's 64 ids, a block's 256, a mark workgroup's 1,024 read
elements, the records' first capacity of 64 blocks."""
import random

import numpy as np
import pytest

import setfull_helpers as H
import setfull_stream_helpers as SH
from lincheck import _native as N
from lincheck import checker as ck
from lincheck import setfull as F
from lincheck.setfull_stream import SetFullStream, rows_of
from test_gpu_setfull import grid_key, keyed

pytestmark = pytest.mark.gpu

ARRAYS = ("valid", "counts", "id_off", "elems", "outcome", "latency", "known", "last_absent", "duplicated", "multiplicity")


@pytest.fixture(scope="module")
def dev(device):
    return ck.Device(0)


def one_shot(dev, prefix, lin):
    """{key: (valid, counts, per element, duplicated)} from lc_setfull_check of the prefix."""
    packed = F.PackedSetFull(F.SetFullHistory.from_ops(prefix))
    res = F.check_batch(dev, packed.view, lin)
    out = {}
    for i, k in enumerate(packed.keys):
        if packed.status[i] != N.LC_SET_KEY_OK:
            out[k] = None
            continue
        out[k] = (int(res.valid[i]), res.counts[i].tolist(), H.per_element(packed, res, i), F.result_map(packed, res, i)["duplicated"])
    return out


def follow(dev, parts, lin=False, cap=0, compare=True):
    """Append the parts one after the other; after each, the stream against
    the one-shot check and the fold of the prefix.  Returns the final arrays,
    the updates and the stream's last result maps."""
    done, ups = [], []
    with SetFullStream(dev, {"linearizable?": lin, "max-matrix-bytes": cap}) as s:
        for part in parts:
            u = s.append(part)
            ups.append(u)
            done = done + list(part)
            if not compare:
                continue
            res = s.results()
            valid, counts = s.counts()
            assert np.array_equal(valid, res.valid) and np.array_equal(counts, res.counts)
            assert u.ids == len(res.elems) and u.rows == len(done)
            SH.check_prefix(s, done, lin, lambda i: SH.stream_per_element(res, i), valid, counts)
            if not s.keys():
                continue
            ref = one_shot(dev, done, lin)
            assert list(ref) == s.keys()
            for i, k in enumerate(s.keys()):
                if ref[k] is None:
                    assert s.key_error(i) and valid[i] == N.LC_UNKNOWN and not counts[i].any()
                    continue
                per, dups = SH.stream_per_element(res, i)
                assert (int(valid[i]), counts[i].tolist(), per, dups) == ref[k], (k, len(done))
        res = s.results()
        maps = [s.result_map(i) for i in range(len(s.keys()))]
        timing = s.last_timing()
    return {name: getattr(res, name).copy() for name in ARRAYS}, ups, maps, timing


def same_arrays(a, b):
    for name in ARRAYS:
        assert np.array_equal(a[name], b[name]), name


def adds(els, t, procs=5):
    out = []
    for e in els:
        out += [H.op("invoke", "add", e, e % procs, t), H.op("ok", "add", e, e % procs, t + 1)]
        t += 2
    return out, t


def read(vals, t, p=5):
    return [H.op("invoke", "read", None, p, t), H.op("ok", "read", vals, p, t + 1)]


def test_hand_example_one_row_per_append(dev):
    ops = H.hand_ops()
    arrs, ups, maps, _ = follow(dev, SH.slices(ops, 1), lin=True)
    assert {k: maps[0][k] for k in H.HAND_WANT} == H.HAND_WANT
    assert [w["element"] for w in maps[0]["worst-stale"]] == H.HAND_WORST
    assert arrs["counts"][0].tolist() == [7, 4, 1, 2, 2, 1] and arrs["valid"].tolist() == [N.LC_INVALID]
    # :valid? over the appends: unknown until the first read (row 6), which misses the acknowledged 1: false from there on
    assert [i for i, u in enumerate(ups) if u.changed] == [6] and ups[6].changed == [0]
    # under independent: two keys, the second one a prefix of the example
    k_ops = keyed([(3, ops), (4, ops[:14])])
    arrs, _, maps, _ = follow(dev, SH.slices(k_ops, 1), lin=True)
    assert {k: maps[0][k] for k in H.HAND_WANT} == H.HAND_WANT and maps[1]["duplicated"] == {3: 2}


@pytest.mark.parametrize("lin", [False, True])
def test_random_histories_any_split(dev, lin):
    """Appends of 1, 7 and 64 rows and all at once: equal to the one-shot check
    after every append, and identical final arrays."""
    n_err = 0
    for seed in range(4):
        ops = H.random_history(random.Random(100 * seed + lin), max_keys=5, max_adds=40 if seed else 12, error_rate=0.12)
        n_err += sum("error" in r for r, _ in H.restate_independent(ops, lin).values())
        finals = [follow(dev, SH.slices(ops, step), lin, compare=(step != 1 or seed == 0))[0] for step in (1, 7, 64, 0)]
        for other in finals[1:]:
            same_arrays(finals[0], other)
    assert n_err > 0  # error keys are in


def test_id_edges(dev):
    """Keys of 63 .. 257 elements in one stream; every key's last wave and block are partly used."""
    rng = random.Random(5)
    groups = [(1000 + e, grid_key(rng, e, 5)) for e in (63, 64, 65, 255, 256, 257)]
    ops = keyed(groups)
    # (keys one after the other: appends of 300 rows cut inside the keys)
    arrs, _, maps, _ = follow(dev, SH.slices(ops, 300), lin=True)
    assert np.diff(arrs["id_off"]).tolist() == [63, 64, 65, 255, 256, 257]
    same_arrays(arrs, follow(dev, [ops], lin=True, compare=False)[0])


def test_growth_and_a_late_key(dev):
    """A key grows from 200 to 600 ids across appends while 70 other keys take
    the blocks around it: past the records' first capacity of 64 blocks
    (doubled, copied device to device), the key's blocks not adjacent; then a
    key nobody saw before."""
    rng = random.Random(6)
    a1, t = adds(range(200), 0)
    part1 = keyed([(1, a1 + read([e for e in range(200) if e % 7], t))])
    small = keyed([(100 + j, grid_key(rng, 3, 2)) for j in range(70)])
    a2, t2 = adds(range(200, 600), t + 10)
    part3 = keyed([(1, a2 + read([e for e in range(600) if e % 5], t2) + read(list(range(0, 600, 2)), t2 + 2))])
    late = keyed([(7, grid_key(rng, 20, 3))])
    arrs, ups, maps, _ = follow(dev, [part1, small, part3, late, keyed([(1, read(list(range(600)), t2 + 10))])], lin=True)
    assert [u.n_keys for u in ups] == [1, 71, 71, 72, 72] and ups[-1].ids == 600 + 70 * 3 + 20
    assert maps[0]["attempt-count"] == 600 and maps[0]["valid?"] is False and maps[0]["stale-count"] > 0


def test_row_edges(dev):
    parts = [
        # 0: adds only (1 is never acknowledged)
        adds([0], 0)[0] + [H.op("invoke", "add", 1, 1, 2), H.op("invoke", "add", 2, 2, 3), H.op("ok", "add", 2, 2, 4),
                          H.op("invoke", "add", 3, 3, 5), H.op("ok", "add", 3, 3, 6), H.op("invoke", "add", 9, 4, 7),
                          H.op("ok", "add", 9, 4, 8)],
        # 1: reads only; process 6's is invoked here and completes in append 3; 2 is in every read, 9 in none
        [H.op("invoke", "read", None, 6, 10)] + read([0, 1, 2], 11) + read([2], 13),
        # 2: 1's ack arrives after the read that held it (known is that read); an empty (nil) read
        [H.op("ok", "add", 1, 1, 20)] + read(None, 21),
        # 3: the read of append 1 completes; 3 is read, re-invoked and read again in one append
        read([2, 3], 30) + [H.op("ok", "read", [0, 2], 6, 32), H.op("invoke", "add", 3, 3, 33)] + read([0, 2, 3], 34),
        # 4: 0 was lost after append 3's last read?  no: held again -- and 1 comes back here
        read([0, 1, 2, 3], 40),
        # 5: 3's second invocation is acknowledged late
        [H.op("ok", "add", 3, 3, 50)],
    ]
    arrs, ups, maps, _ = follow(dev, parts, lin=True)
    assert [u.reads for u in ups] == [0, 2, 1, 3, 1, 0]
    els = arrs["elems"].tolist()
    known = dict(zip(els, arrs["known"].tolist()))
    assert known[1] == 11 and known[3] == 22 and known[2] == 4  # 1: the read at position 11; 3: the read after its re-invocation
    assert maps[0]["lost"] == [9] and maps[0]["valid?"] is False
    # lost after one append and stable again after a later one
    base, t = adds([1, 2], 0)
    parts = [base + read([1, 2], t), read([2], t + 2), read([2], t + 4), read([1, 2], t + 6)]
    _, ups, maps, _ = follow(dev, parts)
    assert [u.changed for u in ups] == [[0], [0], [], [0]] and maps[0]["valid?"] is True and maps[0]["stale"] == [1]


def test_row_passes_give_identical_results(dev):
    """One chunk of 40 reads x 600 ids (3 blocks: 96 bytes a row) under caps that
    force 3, 14 and 40 passes of whole rows."""
    rng = random.Random(9)
    a, t = adds(range(600), 0)
    ops = list(a)
    for j in range(40):
        ops += read([e for e in range(600) if rng.random() < 0.9] + ([17, 17] if j == 33 else []), t + 2 * j, p=5 + j % 3)
    whole, _, maps, timing = follow(dev, [a, ops[len(a):]], lin=True)
    assert timing["passes"] == 1 and maps[0]["duplicated"] == {17: 3}
    for cap, passes in ((15 * 96, 3), (3 * 96, 14), (8, 40)):
        got, _, _, timing = follow(dev, [a, ops[len(a):]], lin=True, cap=cap, compare=False)
        assert timing["passes"] == passes
        same_arrays(whole, got)
    # and the same under a cap when the adds come with the reads
    same_arrays(whole, follow(dev, [ops], lin=True, cap=3 * 96, compare=False)[0])


def test_duplicates(dev):
    n = 1024 + 300
    a, t = adds(range(1400), 0)
    parts = [a,
             read([7, 7, 8, 9, 9, 9, 10], t),               # twice inside one 16-byte load, and across two
             read(list(range(n)) + [7, 1100, 11], t + 2),   # 7 and 11 again in the row's second workgroup, 1100 inside it
             read([20000, 3, 20000], t + 4),                # an element nobody added
             read(list(range(n)), t + 6), read([1, 2], t + 8)]  # none afterwards: flags and multiplicities persist
    arrs, ups, maps, _ = follow(dev, parts)
    want = {7: 2, 9: 3, 11: 2, 1100: 2, 20000: 2}
    assert maps[0]["duplicated"] == want and maps[0]["duplicated-count"] == 5 and maps[0]["valid?"] is False
    assert int(arrs["duplicated"].sum()) == 5 and ups[1].changed == [0]
    els = arrs["elems"].tolist()
    assert arrs["outcome"][els.index(20000)] == N.LC_SETFULL_UNTRACKED


def test_refusals(dev):
    keyed_ops = keyed([(3, H.hand_ops())])
    with SetFullStream(dev, {"linearizable?": True}) as s:
        s.append(keyed_ops[:10])
        before = (s.keys(), s.counts()[1].tolist(), s.results().elems.tolist(), s.rows)
        with pytest.raises(N.LincheckError, match="invalid.*keyed"):
            s.append(H.hand_ops()[10:14])
        bad = F.SetFullHistory.from_ops(keyed_ops[10:14])
        bad.f[1] = 5
        with pytest.raises(N.LincheckError, match="bad :type / :f code"):
            s.append(bad)
        s._results = None
        assert (s.keys(), s.counts()[1].tolist(), s.results().elems.tolist(), s.rows) == before
        s.append(keyed_ops[10:])
        assert {k: s.result_map(0)[k] for k in H.HAND_WANT} == H.HAND_WANT
    with pytest.raises(N.LincheckError, match="unsupported.*one device"):
        SetFullStream(ck.Device(0, devices=[0, 0]))


def test_interleaved_with_the_other_checks(dev):
    from lincheck import history as Hist
    from lincheck import model
    from lincheck import setcheck as S
    import set_helpers as SetH
    import stream_helpers as StH
    h1 = F.synth_set_full(n_keys=3, adds_per_key=300, read_every=50, stale_window=5, lost_rate=0.02, overlap=True, seed=1)
    ops = h1.to_ops()
    want = H.restate_independent(ops, True, H.restate_matrix)
    hs = S.synth_set(n_keys=3, adds_per_key=400, info_rate=0.05, lost_rate=0.02, seed=3)
    reg_h = Hist.synth(n_keys=16, ops_per_key=100, concurrency=5, anomaly_rate=0.2, seed=3)
    reg = ck.Packed(reg_h)
    before = dev.check(reg)
    full = F.PackedSetFull(h1)
    full_res = F.check_batch(dev, full.view, True)
    lin_stream = ck.linearizable({"model": model.cas_register()}).stream(dev)
    cuts = [len(reg_h.type) * j // 4 for j in range(5)]
    with ck.set_full({"linearizable?": True}).stream(dev) as s:
        parts = SH.slices(ops, len(ops) // 4 + 1)
        assert len(parts) == 4
        for j, part in enumerate(parts):
            s.append(part)
            lin_stream.append(StH.rows(reg_h, cuts[j], cuts[j + 1]))
            if j == 0:
                mid = dev.check(reg)
            elif j == 1:
                packed = S.PackedSet(hs)
                assert {k: S.result_map(packed, S.check_batch(dev, packed.view), i)
                        for i, k in enumerate(packed.keys)} == SetH.restate_hist(hs)
            elif j == 2:
                again = F.check_batch(dev, full.view, True)
                for name in ("valid", "counts", "outcome", "latency", "known", "last_absent", "duplicated"):
                    assert np.array_equal(getattr(again, name), getattr(full_res, name)), name
        for i, k in enumerate(s.keys()):
            assert H.same(s.result_map(i), want[k][0]), k
            assert SH.stream_per_element(s.results(), i)[0] == want[k][1]
    lin_stream.finish()
    lin_res = lin_stream.results()
    lin_stream.close()
    after = dev.check(reg)
    assert dict(zip(lin_res.keys, lin_res.valid.tolist())) == dict(zip(reg.keys, before.valid.tolist()))
    for r in (mid, after):
        assert np.array_equal(before.valid, r.valid) and np.array_equal(before.fail_event, r.fail_event)
    assert (after.valid == 0).any()


def test_result_map_equals_the_one_shot_checker(tmp_path, dev):
    """history.edn -> lc_edn_read_setfull rows fed in 5 slices: the stream's
    result map is checker.set_full's of the whole history, :worst-stale and
    both latency quantile maps included."""
    h = F.synth_set_full(n_keys=1, adds_per_key=1500, read_every=100, stale_window=3, lost_rate=0.004, overlap=True, seed=11)
    path = tmp_path / "history.edn"
    path.write_text(H.edn_lines(h.to_ops()))
    hist = F.SetFullHistory.read_edn(str(path))
    opts = {"linearizable?": True}
    want = ck.set_full(opts).check({}, hist, {})
    assert want["valid?"] is False and want["lost-count"] > 0 and len(want["worst-stale"]) == 8
    assert "stable-latencies" in want and "lost-latencies" in want
    ops = hist.to_ops()
    with ck.set_full(opts).stream(dev) as s:
        n = len(ops) // 5 + 1
        for part in SH.slices(ops, n):
            s.append(part)
        assert s.result_map(0) == want
    # columns in, not op maps: slices of the history itself, and an unkeyed random history with duplicates
    cols = [rows_of(hist, a, a + n) for a in range(0, hist.n, n)]
    with SetFullStream(dev, opts) as s:
        for c in cols:
            s.append(c)
        assert s.result_map(0) == want
    for seed in (3, 4, 5):
        ops = H.random_history(random.Random(seed), max_keys=1, keyed=False, error_rate=0)
        want = ck.set_full(opts).check({}, ops, {})
        with SetFullStream(dev, opts) as s:
            for part in SH.slices(ops, 9):
                s.append(part)
            assert H.norm(s.result_map(0)) == H.norm(want), seed
