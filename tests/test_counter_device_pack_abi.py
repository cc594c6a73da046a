"""include/lincheck_counter_pack.h against the ctypes binding, without a GPU:
every symbol the header declares is exported and has a prototype, it adds no
struct of its own and leaves include/lincheck_counter.h's names alone, null
arguments are LC_E_INVALID before any device is touched, the error texts are
lc_counter_pack's, and {"pack": "device"} does not go with {"host": True}."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import counter_pack_helpers as PH
from lincheck import _native as N
from lincheck import checker as ck

INCLUDE = os.path.join(os.path.dirname(__file__), "..", "include")
HEADER = os.path.join(INCLUDE, "lincheck_counter_pack.h")
NAMES = ("lc_counter_check_history", "lc_counter_checked_free", "lc_counter_checked_view", "lc_counter_checked_keys",
         "lc_counter_checked_key_error", "lc_counter_checked_key_error_row", "lc_counter_checked_read_vals",
         "lc_counter_checked_batch", "lc_counter_history_timing", "lc_counter_pack_launch_info", "lc_counter_pack_table_slots")


def declared(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(lc_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_exported_and_bound():
    L = C.CDLL(N.LIB_PATH)
    names = declared(HEADER)
    assert set(names) == set(NAMES) == set(N.COUNTER_PACK_SIGNATURES)
    for name in names:
        assert hasattr(L, name), name
        assert getattr(N.lib(), name).argtypes == N.COUNTER_PACK_SIGNATURES[name][1]
    others = (set(N.SIGNATURES) | set(N.COUNTER_SIGNATURES) | set(N.QUEUE_SIGNATURES) | set(N.SETFULL_STREAM_SIGNATURES)
              | set(N.QUEUE_STREAM_SIGNATURES) | set(N.COUNTER_STREAM_SIGNATURES))
    assert not set(names) & others


def test_the_abi_version_stays_13_and_the_header_adds_no_struct():
    assert N.LC_ABI_VERSION == 13 and N.lib().lc_abi_version() == 13
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.findall(r"typedef struct (\w+)", src) == ["lc_counter_checked"] and "{" not in src.replace('extern "C" {', "")
    # the structs it passes are lincheck_counter.h's, whose sizes tests/test_counter_abi.py holds against the compiler's
    assert set(declared(os.path.join(INCLUDE, "lincheck_counter.h"))) == set(N.COUNTER_SIGNATURES)


def test_null_arguments_are_invalid_without_a_device():
    L = N.lib()
    h = PH.hist([(PH.INVOKE, PH.ADD, 0, None, 1)]).as_c()
    o, out, fake = N.LcCounterOpts(0, 0), C.c_void_p(), C.c_void_p(1)   # (the context is not touched before the checks)
    assert L.lc_counter_check_history(None, C.byref(h), C.byref(o), C.byref(out)) == -1
    assert L.lc_counter_check_history(fake, None, C.byref(o), C.byref(out)) == -1
    assert L.lc_counter_check_history(fake, C.byref(h), None, C.byref(out)) == -1
    assert L.lc_counter_check_history(fake, C.byref(h), C.byref(o), None) == -1
    assert L.lc_counter_check_history(fake, C.byref(h), C.byref(N.LcCounterOpts(0, 1)), C.byref(out)) == -1
    assert L.lc_counter_check_history(fake, C.byref(h), C.byref(N.LcCounterOpts(100, 0)), C.byref(out)) == -1
    h.n = -1
    assert L.lc_counter_check_history(fake, C.byref(h), C.byref(o), C.byref(out)) == -1
    h.n = (1 << 31) - 15
    assert L.lc_counter_check_history(fake, C.byref(h), C.byref(o), C.byref(out)) == -5   # LC_E_UNSUPPORTED
    assert "2^31 - 16" in L.lc_last_error().decode()
    h.n, h.value = 1, None
    assert L.lc_counter_check_history(fake, C.byref(h), C.byref(o), C.byref(out)) == -1
    assert L.lc_counter_checked_view(None, None, None) == -1 and L.lc_counter_checked_keys(None, None) == -1
    assert L.lc_counter_checked_read_vals(None, None) == -1 and L.lc_counter_checked_batch(None, None, None) == -1
    assert L.lc_counter_history_timing(None, None) == -1 and L.lc_counter_pack_launch_info(None) == -1
    assert L.lc_counter_checked_key_error(None, 0) is None and L.lc_counter_checked_key_error_row(None, 0) == -1
    L.lc_counter_checked_free(None)


def test_a_history_of_no_rows_needs_no_device():
    L = N.lib()
    h, o, out = PH.hist([]).as_c(), N.LcCounterOpts(0, 0), C.c_void_p()
    assert L.lc_counter_check_history(C.c_void_p(1), C.byref(h), C.byref(o), C.byref(out)) == 0
    v, r, key = N.LcCounterBatch(), N.LcCounterResult(), (C.c_int64 * 1)()
    assert L.lc_counter_checked_view(out, C.byref(v), C.byref(r)) == 0 and L.lc_counter_checked_keys(out, key) == 0
    want, _, _ = PH.host_answer(PH.hist([]))
    assert v.n_keys == 1 and key[0] == N.LC_NO_KEY and r.valid[0] == 1 and r.n_err == 0 and want["keys"] == [None]
    assert [v.ev_off[0], v.ev_off[1], v.read_off[1], r.err_off[1]] == [0, 0, 0, 0]
    L.lc_counter_checked_free(out)


def test_launch_constants():
    out = (C.c_int64 * 3)()
    assert N.lib().lc_counter_pack_launch_info(out) == 0 and list(out) == [256, 2048, (1 << 31) - 16]
    assert [N.lib().lc_counter_pack_table_slots(n) for n in (-1, 0, 1, 128, 129, 1000)] == [0, 256, 256, 256, 512, 2048]


def test_the_error_texts_are_lc_counter_packs():
    """One tiny history per message, packed on the host: its text is the table's
    (csrc/counter_pack_plan.hpp, through tests/counter_pack_helpers.py and
    tests/test_counter_pack_plan.py, which holds the header against these constants)."""
    I, O, A, R = PH.INVOKE, PH.OK, PH.ADD, PH.READ
    tiny = {
        PH.SECOND_INVOKE: [(I, R, 0, None, None), (I, R, 0, None, None)],
        PH.NO_OPEN: [(O, A, 0, None, 1)],
        PH.OTHER_F: [(I, A, 0, None, 1), (O, R, 0, None, 1)],
        PH.READ_NIL: [(I, R, 0, None, None), (O, R, 0, None, None)],
        PH.ADD_NIL: [(I, A, 0, None, None)],
        PH.ADD_NEGATIVE: [(I, A, 0, None, -1)],
        PH.SUM: [(I, A, 0, None, PH.I64_MAX), (I, A, 1, None, 1)],
    }
    assert set(tiny) == set(PH.MESSAGES)
    for message, rows in tiny.items():
        want, _ = PH.host_pack(PH.hist(rows, keyed=False))
        assert want["error"] == [message]


def test_pack_device_does_not_go_with_host():
    with pytest.raises(ValueError):
        ck.counter({"pack": "device", "host": True})
    with pytest.raises(ValueError):
        ck.counter({"pack": "elsewhere"})
    assert ck.counter({"pack": "device"}).pack == "device" and ck.counter().pack == "host" and ck.counter({"host": True}).host


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jepsen-etcd-demo_amd", "csrc")
CXX = shutil.which("g++")


@pytest.mark.skipif(not CXX, reason="no g++")
def test_the_host_half_runs_clean_under_asan_and_ubsan(tmp_path):
    """tests/counter_pack_asan_main.cpp: the argument checks, the result object and what the host
    shapes from it, as a stand-alone program with the device half stubbed."""
    out = str(tmp_path / "asan_main")
    subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "counter_pack_asan_main.cpp"), os.path.join(CSRC, "host_counter_pack.cpp"),
                    os.path.join(CSRC, "host_counter.cpp"), "-o", out], check=True, timeout=300)
    r = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, \
        r.stdout + r.stderr[-3000:]
