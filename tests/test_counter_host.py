"""checker/counter without a GPU: lc_counter_pack and lc_counter_check_host
against the two restatements of the rules in tests/counter_helpers.py (the
oracle; parity with Jepsen unpinned), the error rules key by key, the overflow
rule, the checker shapes with the host fold as the backend, and the packer and
host fold under AddressSanitizer and UBSan as a stand-alone program."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import counter_helpers as H
from lincheck import _native as N
from lincheck import checker as ck
from lincheck import counter as CT
from lincheck import independent

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jepsen-etcd-demo_amd", "csrc")
CXX = shutil.which("g++")
I64_MAX = H.I64_MAX


def host_maps(ops, err_cap=None):
    """{key: result map} through lc_counter_pack + lc_counter_check_host."""
    packed = CT.PackedCounter(CT.CounterHistory.from_ops(ops))
    res = CT.check_batch(None, packed.view, err_cap=err_cap, host=True)
    return {k: CT.result_map(packed, res, i) for i, k in enumerate(packed.keys)}, packed, res


def agree(ops):
    want = H.restate_independent(ops, H.restate)
    again = H.restate_independent(ops, H.restate_np)
    got, packed, res = host_maps(ops)
    assert list(got) == list(want) == list(again)
    for k in want:
        assert H.same(again[k], want[k]), (k, again[k], want[k])
        assert H.same(got[k], want[k]), (k, got[k], want[k])
    exp = H.expected_arrays(want)
    for name in ("valid", "n_errors", "lower", "upper", "err_off", "err_idx"):
        assert np.array_equal(getattr(res, name), exp[name]), name
    return want


def test_hand_example():
    got, packed, res = host_maps(H.hand_ops())
    assert got == {None: {"valid?": False, "reads": H.HAND_READS, "errors": H.HAND_ERRORS}}
    assert H.restate(H.hand_ops()) == got[None] and H.restate_np(H.hand_ops()) == got[None]
    # the packed events: only the rows that matter, a read event's value its read's index
    a = packed.arrays()
    UP, LOW, RI, RO = N.LC_CE_UP, N.LC_CE_LOW, N.LC_CE_RINV, N.LC_CE_ROK
    assert a["ev_kind"].tolist() == [UP, RI, LOW, UP, RO, RI, RO, RI, UP, LOW, RO, RI, RO]
    assert a["ev_val"].tolist() == [1, 0, 1, 2, 0, 1, 1, 2, 3, 3, 2, 3, 3]
    assert a["read_val"].tolist() == [1, 4, 0, 6] and a["ev_off"].tolist() == [0, 13] and a["read_off"].tolist() == [0, 4]


def test_a_failed_add_never_counts_and_an_ok_value_replaces_the_invocations():
    ops = [H.op("invoke", "add", 0, 4), H.op("fail", "add", 0, 4), H.op("invoke", "add", 1, 9), H.op("ok", "add", 1, 2),
           H.op("invoke", "read", 2), H.op("ok", "read", 2, 2)]
    assert host_maps(ops)[0][None] == {"valid?": True, "reads": [[2, 2, 2]], "errors": []}
    # an invocation of nil that its :ok fills in is no error; one that stays nil is
    ops = [H.op("invoke", "add", 0, None), H.op("ok", "add", 0, 3), H.op("invoke", "read", 1), H.op("ok", "read", 1, 3)]
    assert agree(ops)[None]["valid?"] is True
    assert agree(ops[:1] + [H.op("info", "add", 0, None)] + ops[2:])[None]["valid?"] == "unknown"


@pytest.mark.parametrize("block", range(4))
def test_small_random_histories(block):
    rng = H.rng_of(100 + block)
    for i in range(500):
        agree(H.random_history(rng, rng.randint(0, 40), n_keys=[0, 1, 3][i % 3], p_bad=0.03))


@pytest.mark.parametrize("block", range(4))
def test_long_random_histories(block):
    rng = H.rng_of(200 + block)
    for i in range(50):
        agree(H.random_history(rng, 2000, n_keys=[0, 5][i % 2], p_bad=0.0005 if i % 5 else 0.0))


@pytest.mark.parametrize("kind", H.BAD_KINDS)
def test_an_error_makes_exactly_its_own_key_unknown(kind):
    rng = H.rng_of(7)
    keys = [(k, H.exact_key(rng, 40)) for k in (10, 20, 30)]
    clean = agree(H.keyed(keys))
    assert all(r["valid?"] != "unknown" for r in clean.values())
    keys[1] = (20, H.break_key(rng, keys[1][1], kind))
    for ops in (H.keyed(keys), H.interleave(rng, keys)):
        want = agree(ops)
        got = host_maps(ops)[0]
        assert got[20]["valid?"] == "unknown" and got[20]["error"]
        assert got[10] == clean[10] and got[30] == clean[30] and want[10] == clean[10]


def test_the_sum_may_reach_int64_max_and_not_pass_it():
    big = 1 << 61
    adds = [big, big, big, big - 1]
    ops = []
    for v in adds:
        ops += [H.op("invoke", "add", 0, v), H.op("ok", "add", 0, v)]
    ops += [H.op("invoke", "read", 1), H.op("ok", "read", 1, I64_MAX)]
    assert agree(ops)[None] == {"valid?": True, "reads": [[I64_MAX, I64_MAX, I64_MAX]], "errors": []}
    more = ops + [H.op("invoke", "add", 0, 1)]
    assert agree(more)[None]["valid?"] == "unknown"
    # a failed add past the limit never counted
    assert agree(more + [H.op("fail", "add", 0, 1)])[None]["valid?"] is True


def test_err_cap_too_small_is_reported_and_the_retry_succeeds():
    ops = H.exact_key(H.rng_of(3), 400, p_wrong=0.5)
    want = H.restate(ops)
    assert len(want["errors"]) > 5
    packed = CT.PackedCounter(CT.CounterHistory.from_ops(ops))
    K, R = 1, packed.n_reads
    valid, n_errors, err_off = np.zeros(K, np.int8), np.zeros(K, np.uint64), np.zeros(K + 1, np.uint64)
    lower, upper, err_idx = np.zeros(R, np.int64), np.zeros(R, np.int64), np.zeros(1, np.uint64)
    r = N.LcCounterResult(N.ptr(valid, C.c_int8), N.ptr(n_errors, C.c_uint64), N.ptr(lower, C.c_int64),
                          N.ptr(upper, C.c_int64), N.ptr(err_off, C.c_uint64), N.ptr(err_idx, C.c_uint64), 1, 0)
    assert N.lib().lc_counter_check_host(C.byref(packed.view), C.byref(r)) == -2
    assert int(r.n_err) == len(want["errors"]) and b"needed" in N.lib().lc_last_error()
    res = CT.check_batch(None, packed.view, err_cap=1, host=True)
    assert res.retried and CT.result_map(packed, res, 0) == want


def test_caller_built_batches_are_validated():
    packed = CT.PackedCounter(CT.CounterHistory.from_ops(H.keyed([(1, H.hand_ops()), (2, H.hand_ops())])))
    a = packed.arrays()
    res = CT.check_batch(None, CT.batch_of(a), host=True)
    assert CT.result_map(packed, res, 1)["reads"] == H.HAND_READS
    for name, at, v in (("ev_val", 1, 4), ("ev_val", 1, -1), ("ev_kind", 0, 9), ("ev_off", 1, 99), ("status", 0, 1), ("status", 0, 3)):
        b = {k: x.copy() for k, x in a.items()}
        b[name][at] = v
        with pytest.raises(N.LincheckError, match="invalid"):
            CT.check_batch(None, CT.batch_of(b), host=True)


def test_bad_codes_and_null_arguments_are_refused():
    h = CT.CounterHistory.from_ops(H.hand_ops())
    h.type[3] = 9
    with pytest.raises(N.LincheckError, match="invalid"):
        CT.PackedCounter(h)
    assert N.lib().lc_counter_pack(None, None) == -1
    assert N.lib().lc_counter_check_host(None, None) == -1
    assert N.lib().lc_counter_packed_key_error(None, 0) is None


def test_checker_shapes():
    rng = H.rng_of(11)
    keys = [(k, H.exact_key(rng, 60)) for k in range(5)]
    keys[2] = (2, H.break_key(rng, keys[2][1], "nil-read"))
    ops = H.interleave(rng, keys)
    want = H.restate_independent(ops)
    counter = ck.counter({"host": True})
    # alone, on one key's sub-history
    assert counter.check({}, keys[0][1], {}) == want[0]
    # under independent.checker: every key in one call
    r = independent.checker(counter).check({}, ops, {})
    assert list(r["results"]) == [k for k in want] and all(H.same(r["results"][k], want[k]) for k in want)
    assert r["failures"] == [k for k in want if want[k]["valid?"] is False]
    assert r["valid?"] == ck.merge_valid([x["valid?"] for x in want.values()])
    # composed, alone and per key
    both = ck.compose({"optimism": ck.unbridled_optimism(), "counter": counter})
    one = both.check({}, keys[1][1], {})
    assert one["counter"] == want[1] and one["valid?"] == want[1]["valid?"]
    r = independent.checker(both).check({}, ops, {})
    for k in want:
        assert H.same(r["results"][k]["counter"], want[k]) and r["results"][k]["optimism"] == {"valid?": True}
    assert r["failures"] == [k for k in want if want[k]["valid?"] is False]
    # a CounterHistory goes in as it is
    r2 = independent.checker(counter).check({}, CT.CounterHistory.from_ops(ops), {})
    assert all(H.same(r2["results"][k], want[k]) for k in want)


def test_synth_counter_is_valid_unless_stale():
    clean = CT.synth_counter(n_keys=3, ops_per_key=203, concurrency=5, info_rate=0.1, fail_rate=0.1, seed=5)
    want = H.restate_independent(clean.to_ops())
    assert len(want) == 3 and all(r["valid?"] is True and r["reads"] for r in want.values())
    stale = CT.synth_counter(n_keys=3, ops_per_key=203, concurrency=5, info_rate=0.1, fail_rate=0.1, stale_rate=0.2, seed=5)
    ops = stale.to_ops()
    want = agree(ops)
    assert all(r["valid?"] is False for r in want.values())
    r = independent.checker(ck.counter({"host": True})).check({}, stale, {})
    assert r["results"] == want


def test_launch_info():
    out = np.zeros(4, np.int64)
    N.check(N.lib().lc_counter_launch_info(N.ptr(out, C.c_int64)))
    assert out.tolist() == [256, 2048, 256, 256]


@pytest.mark.skipif(not CXX, reason="no g++")
def test_pack_and_host_fold_run_clean_under_asan_and_ubsan(tmp_path):
    out = str(tmp_path / "asan_main")
    subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "counter_asan_main.cpp"), os.path.join(CSRC, "host_counter.cpp"),
                    "-o", out], check=True, timeout=300)
    r = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, \
        r.stderr[-3000:]
