"""The streaming checker/counter without a GPU: the host stream
(lc_counter_stream_open without a context) against lc_counter_pack +
lc_counter_check_host of the prefix and the restatement of
tests/counter_helpers.py after EVERY append -- array for array, map for map --
on the hand example row by row, on seeded random histories cut at random
places and on hand-built cases for every direction valid can move in; the
refusals that leave the stream as it was; and the packer and host fold under
AddressSanitizer and UBSan as a stand-alone program."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import counter_helpers as H
import counter_stream_helpers as S
from lincheck import _native as N
from lincheck import checker as ck
from lincheck import counter as CT
from lincheck import independent
from lincheck.counter_stream import CounterStream, rows_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jepsen-etcd-demo_amd", "csrc")
CXX = shutil.which("g++")
CASES = S.hand_cases()


def test_hand_example_row_by_row():
    out = S.follow(None, CASES["hand"])
    with CounterStream(None) as s:
        for o in H.hand_ops():
            s.append([o])
        assert s.result_map(0) == {"valid?": False, "reads": H.HAND_READS, "errors": H.HAND_ERRORS}
    # `fail add 0 4` revises nothing that was read
    assert sum(u.revisited for u, _ in out) == 0


def test_hand_example_with_a_read_before_the_fail():
    out = S.follow(None, CASES["hand-read-before-the-fail"])
    fail_at = next(j for j, part in enumerate(CASES["hand-read-before-the-fail"]) if part[0]["type"] == "fail" and part[0]["f"] == "add")
    u = out[fail_at][0]
    # the read [1 6 7] completed since the invocation is looked at again: its upper bound 7 becomes 3
    assert (u.patched, u.revisited, u.changed) == (1, 1, [0])


@pytest.mark.parametrize("seed", range(8))
def test_random_histories_without_bad_rows(seed):
    parts = S.random_case(seed, 0)
    assert len(parts) == 13
    seen, late_fails = S.transitions(parts)
    assert not any(v == -1 for d in seen for v in d.values())
    assert 1 <= late_fails <= 9, late_fails
    flat = [{}] + seen
    assert sum(1 for a, b in zip(flat, flat[1:]) for k in b if a.get(k, 1) == 1 and b[k] == 0) == 3
    out = S.follow(None, parts)
    assert [v for _, v in out] == seen
    assert sum(u.patched for u, _ in out) >= late_fails


@pytest.mark.parametrize("seed", range(8))
def test_random_histories_with_bad_rows(seed):
    parts = S.random_case(seed, 0.002)
    seen, _ = S.transitions(parts)
    share = sum(v == -1 for d in seen for v in d.values()) / sum(len(d) for d in seen)
    assert share <= 0.6, share   # (the test cannot pass on unknowns alone)
    out = S.follow(None, parts)
    assert [v for _, v in out] == seen


DIRECTIONS = {"invalid-to-valid": [1, 1, 0, 1, 1, 1], "valid-to-invalid-by-a-fail": [1, 1, 1, 0, 0, 0],
              "unknown-and-back-nil-ok-3": [-1, -1, -1, -1, 1, 0], "unknown-and-back-negative-fail": [-1, -1, -1, -1, 1, 1],
              "unknown-and-back-sum": [1, -1, -1, -1, -1, -1, -1, -1, -1, -1, 0, 0]}


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_built_cases(name):
    out = S.follow(None, CASES[name])
    if name in DIRECTIONS:
        assert [list(v.values())[0] for _, v in out] == DIRECTIONS[name]
    if name.startswith("permanent-"):
        # key 2 is :unknown from the third append on, and stays; key 1 goes on and turns invalid
        assert [v[2] for _, v in out] == [1, 1, -1, -1] and [v[1] for _, v in out] == [1, 1, 1, 0]


def test_a_key_that_came_back_has_all_its_reads():
    with CounterStream(None) as s:
        for part in CASES["unknown-and-back-nil-ok-3"][:4]:
            s.append(part)
        assert s.counts()[0].tolist() == [-1] and s.counts()[2].tolist() == [0] and s.key_error(0)
        assert s.result_map(0)["valid?"] == "unknown"
        u = s.append(CASES["unknown-and-back-nil-ok-3"][4])
        assert u.changed == [0] and s.key_error(0) is None
        assert s.result_map(0) == {"valid?": True, "reads": [[0, 2, 3]], "errors": []}


def snapshot(s):
    res = s.results()
    return s.keys(), [a.tolist() for a in s.counts()], [getattr(res, n).tolist() for n in ("lower", "upper", "err_off", "err_idx")]


def test_refused_appends_leave_the_stream_as_it_was():
    keyed = [S.kop(3, "invoke", "add", 0, 1), S.kop(3, "invoke", "read", 1), S.kop(3, "ok", "read", 1, 4)]
    more = [S.kop(3, "fail", "add", 0, 1), S.kop(8, "invoke", "add", 0, 2)]
    with CounterStream(None) as s:
        s.append(keyed)
        was = snapshot(s)
        assert was[1][0] == [0]
        with pytest.raises(N.LincheckError) as e:   # the other keyedness
            s.append([H.op("invoke", "add", 5, 1)])
        assert e.value.code == -1 and snapshot(s) == was
        bad = CT.CounterHistory.from_ops(more)
        for col, code in (("type", 4), ("f", 3)):
            h = CT.CounterHistory(bad.type.copy(), bad.f.copy(), bad.process, bad.key, bad.value)
            getattr(h, col)[1] = code
            with pytest.raises(N.LincheckError) as e:
                s.append(h)
            assert e.value.code == -1 and snapshot(s) == was   # key 8 is not there, the :fail has revised nothing
        u = s.append(more)
        assert u.n_keys == 2 and s.keys() == [3, 8] and u.patched == 1
        S.same_as_prefix(s, keyed + more)
    with CounterStream(None) as s:   # an unkeyed stream refuses keyed rows
        s.append([H.op("invoke", "add", 0, 1)])
        was = snapshot(s)
        with pytest.raises(N.LincheckError) as e:
            s.append(keyed)
        assert e.value.code == -1 and snapshot(s) == was and s.keys() == [None]


def test_before_any_client_row_the_stream_reads_as_an_empty_history():
    with CounterStream(None) as s:
        S.same_as_prefix(s, [])
        assert s.keys() == [None] and s.counts()[0].tolist() == [1]
        u = s.append([])
        assert (u.rows, u.n_keys, u.events, u.reads, u.patched, u.revisited, u.grew, u.changed) == (0, 1, 0, 0, 0, 0, False, [])
        nemesis = [{"type": "info", "f": "start", "value": "x", "process": "nemesis"}]
        s.append(nemesis)
        S.same_as_prefix(s, nemesis)
        u = s.append([S.kop(77, "invoke", "read", 0), S.kop(78, "invoke", "add", 0, None)])
        assert s.keys() == [77, 78] and u.n_keys == 2 and u.changed == [1]


def test_the_reads_array_grows_by_doubling():
    ops = S.events_exactly(2 * 600, read_every=1)   # 600 reads
    with CounterStream(None, {"reads": 256}) as s:
        grew = [s.append(ops[lo:lo + 200]).grew for lo in range(0, len(ops), 200)]   # 100 reads an append
        # 300 reads pass 256: 512; 600 pass 512: 1,024
        assert grew == [False, False, True, False, False, True]
        S.same_as_prefix(s, ops, maps=False)


def test_the_err_cap_protocol_and_columns():
    hist = CT.synth_counter(n_keys=3, ops_per_key=400, stale_rate=0.2, fail_rate=0.1, seed=4)
    with CounterStream(None) as s:
        for lo in range(0, hist.n, 77):
            s.append(rows_of(hist, lo, lo + 77))
        full = s.results()
        assert len(full.err_idx) > 10 and not full.retried
        again = s.results(err_cap=1)
        assert again.retried
        for name in ("valid", "n_errors", "lower", "upper", "err_off", "err_idx"):
            assert np.array_equal(getattr(full, name), getattr(again, name)), name
        S.same_as_prefix(s, hist, maps=False)


def test_the_checker_shapes():
    hist = CT.synth_counter(n_keys=4, ops_per_key=300, stale_rate=0.05, fail_rate=0.1, info_rate=0.1, seed=3)
    ops = hist.to_ops()
    c = ck.counter({"host": True})
    want = independent.checker(c).check({}, ops, {})["results"]
    with c.stream() as s:
        for lo in range(0, hist.n, 97):
            s.append(rows_of(hist, lo, lo + 97))
        assert s.dev is None and s.result_maps() == want
        for i, k in enumerate(s.keys()):
            assert s.result_map(i) == c.check({}, independent.subhistory(ops, k), {})
    with ck.counter().stream() as s:   # no device: the host stream
        assert s.dev is None


@pytest.mark.skipif(not CXX, reason="no g++")
def test_packer_and_host_fold_run_clean_under_asan_and_ubsan(tmp_path):
    out = str(tmp_path / "asan_main")
    subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "counter_stream_asan_main.cpp"), os.path.join(CSRC, "host_counter_stream.cpp"),
                    os.path.join(CSRC, "host_counter.cpp"), "-pthread", "-o", out], check=True, timeout=300)
    r = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, \
        r.stderr[-3000:]
