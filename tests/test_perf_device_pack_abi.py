"""include/lincheck_perf_pack.h against the ctypes binding, without a GPU: every
symbol the header declares is exported and has a prototype, it adds no struct
of its own, null arguments are LC_E_INVALID before any device is touched, a
history of no rows is answered without one, the launch constants, the Python
option, and the host half as a stand-alone program under ASan and UBSan."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import perf_helpers as PH
from lincheck import _native as N
from lincheck import checker as ck
from lincheck import perf as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "lincheck_perf_pack.h")
CSRC = os.path.join(ROOT, "jepsen-etcd-demo_amd", "csrc")
NAMES = ("lc_perf_check_history", "lc_perf_checked_free", "lc_perf_checked_view", "lc_perf_checked_info",
         "lc_perf_checked_intervals", "lc_perf_checked_records", "lc_perf_history_timing", "lc_perf_pack_launch_info")


def declared(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(lc_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_exported_and_bound():
    L = C.CDLL(N.LIB_PATH)
    names = declared(HEADER)
    assert set(names) == set(NAMES) == set(N.PERF_PACK_SIGNATURES)
    for name in names:
        assert hasattr(L, name), name
        assert getattr(N.lib(), name).argtypes == N.PERF_PACK_SIGNATURES[name][1]
    others = (set(N.SIGNATURES) | set(N.COUNTER_SIGNATURES) | set(N.QUEUE_SIGNATURES) | set(N.SETFULL_STREAM_SIGNATURES)
              | set(N.QUEUE_STREAM_SIGNATURES) | set(N.COUNTER_STREAM_SIGNATURES) | set(N.COUNTER_PACK_SIGNATURES))
    assert not set(names) & others
    assert not set(names) & set(declared(os.path.join(INCLUDE, "lincheck.h")))


def test_the_abi_version_stays_13_and_the_header_adds_no_struct():
    assert N.LC_ABI_VERSION == 13 and N.lib().lc_abi_version() == 13
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.findall(r"typedef struct (\w+)", src) == ["lc_perf_checked"] and "{" not in src.replace('extern "C" {', "")


def one_row():
    return P.PerfHistory.from_ops([PH.op("invoke", "read", 0, 5)])


def test_null_arguments_are_invalid_without_a_device():
    L = N.lib()
    hist = one_row()
    h, o, out, fake = hist.as_c(), P.make_opts(), C.c_void_p(), C.c_void_p(1)  # (the context is not touched before the checks)
    assert L.lc_perf_check_history(None, C.byref(h), C.byref(o), C.byref(out)) == -1
    assert L.lc_perf_check_history(fake, None, C.byref(o), C.byref(out)) == -1
    assert L.lc_perf_check_history(fake, C.byref(h), None, C.byref(out)) == -1
    assert L.lc_perf_check_history(fake, C.byref(h), C.byref(o), None) == -1
    h.n = -1
    assert L.lc_perf_check_history(fake, C.byref(h), C.byref(o), C.byref(out)) == -1
    h.n = (1 << 31) - 15
    assert L.lc_perf_check_history(fake, C.byref(h), C.byref(o), C.byref(out)) == -5   # LC_E_UNSUPPORTED
    assert "2^31 - 16" in L.lc_last_error().decode()
    h.n, h.n_f = 1, 257
    assert L.lc_perf_check_history(fake, C.byref(h), C.byref(o), C.byref(out)) == -1
    h.n_f = N.LC_PERF_MAX_F + 1
    assert L.lc_perf_check_history(fake, C.byref(h), C.byref(o), C.byref(out)) == -5 and "33" in L.lc_last_error().decode()
    h.n_f, h.time = 1, None
    assert L.lc_perf_check_history(fake, C.byref(h), C.byref(o), C.byref(out)) == -1
    assert not out.value
    assert L.lc_perf_checked_view(None, None, None) == -1 and L.lc_perf_checked_info(None, None) == -1
    assert L.lc_perf_checked_intervals(None, None) == -1 and L.lc_perf_checked_records(None, None, None) == -1
    assert L.lc_perf_history_timing(None, None) == -1 and L.lc_perf_pack_launch_info(None) == -1
    L.lc_perf_checked_free(None)


def test_a_history_of_no_rows_needs_no_device():
    L = N.lib()
    hist = P.PerfHistory.from_ops([])
    h, o, out, fake = hist.as_c(), P.make_opts(), C.c_void_p(), C.c_void_p(1)
    assert L.lc_perf_check_history(fake, C.byref(h), C.byref(o), C.byref(out)) == 0
    v, r, info = N.LcPerfBatch(), N.LcPerfResult(), np.full(4, 9, np.int64)
    assert L.lc_perf_checked_view(out, C.byref(v), C.byref(r)) == 0 and L.lc_perf_checked_info(out, N.ptr(info, C.c_int64)) == 0
    assert (v.n, v.n_matched, v.n_f, v.t_min, v.t_max, v.x_min, v.x_max) == (0, 0, 0, 0, 0, 0, 0) and not v.t_comp
    assert (r.rate_first, r.rate_n, r.q_first, r.q_n, r.rate_cap, r.group_cap, r.quant_cap) == (0,) * 7 and info.tolist() == [0] * 4
    assert L.lc_perf_checked_intervals(out, None) == 0
    b = N.LcPerfBatch()
    assert L.lc_perf_checked_records(fake, out, C.byref(b)) == 0 and b.n == 0
    L.lc_perf_checked_free(out)
    # the host path's answer to the same history: lc_perf_pack's empty batch
    packed = P.PackedPerf(hist)
    assert (packed.n, packed.matched, packed.unmatched, packed.orphans, len(packed.intervals)) == (0, 0, 0, 0, 0)
    # lc_perf_check's refusals hold for it too
    out = C.c_void_p()
    for bad in ({"quantile-dt-ns": 0}, {"rate-dt-ns": -5}, {"quantiles": [1.5]}):
        assert L.lc_perf_check_history(fake, C.byref(h), C.byref(P.make_opts(bad)), C.byref(out)) == -1 and not out.value


def test_launch_constants():
    out = (C.c_int64 * 3)()
    assert N.lib().lc_perf_pack_launch_info(out) == 0 and list(out) == [256, 2048, (1 << 31) - 16]


def test_the_pack_option():
    for bad in ("elsewhere", "", None, 1):
        with pytest.raises(ValueError):
            ck.perf({"pack": bad})
        with pytest.raises(ValueError):
            P.analyze(None, [], {"pack": bad})
    assert ck.perf({"pack": "device"}).pack == "device" and ck.perf().pack == "host" and ck.perf({"pack": "host"}).pack == "host"


CXX = shutil.which("g++")


@pytest.mark.skipif(not CXX, reason="no g++")
def test_the_host_half_runs_clean_under_asan_and_ubsan(tmp_path):
    """tests/perf_pack_asan_main.cpp: the argument checks, the interval fold and the result object, as a
    stand-alone program; once with the device half stubbed, once without any (LC_E_DEVICE)."""
    for tag, flags in (("stub", []), ("none", ["-DPP_NO_DEVICE_HALF"])):
        out = str(tmp_path / f"asan_main_{tag}")
        subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", *flags, "-I", INCLUDE, "-I", CSRC,
                        os.path.join(ROOT, "tests", "perf_pack_asan_main.cpp"), os.path.join(CSRC, "host_perf_pack.cpp"),
                        os.path.join(CSRC, "host_perf.cpp"), "-o", out], check=True, timeout=300)
        r = subprocess.run([out], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.strip() == "ok" and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, \
            tag + r.stdout + r.stderr[-3000:]
