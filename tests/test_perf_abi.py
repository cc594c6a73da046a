"""ABI 13's additions: every lc_perf_* / lc_edn_*_perf symbol is exported and
bound, and the ctypes mirrors of the new structs have the C compiler's sizes
and offsets for include/lincheck.h (x86-64 LP64), as tests/test_abi.py checks
the older ones."""
import ctypes as C
import os
import re
import subprocess

from lincheck import _native as N

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "lincheck.h")
STRUCTS = {"lc_perf_history": N.LcPerfHistory, "lc_perf_batch": N.LcPerfBatch, "lc_perf_opts": N.LcPerfOpts,
           "lc_perf_result": N.LcPerfResult}
SYMBOLS = ["lc_perf_pack", "lc_perf_packed_free", "lc_perf_packed_view", "lc_perf_packed_info", "lc_perf_packed_intervals",
           "lc_perf_opts_default", "lc_perf_shape", "lc_perf_check", "lc_perf_last_timing", "lc_perf_launch_info",
           "lc_edn_read_perf", "lc_edn_parse_perf", "lc_perf_hist_view", "lc_perf_hist_name", "lc_perf_hist_free"]


def test_abi_is_13():
    assert N.LC_ABI_VERSION == 13 and N.lib().lc_abi_version() == 13
    assert re.search(r"#define LC_ABI_VERSION 13\b", open(HEADER).read())


def test_symbols_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(lc_[a-z0-9_]+)\s*\(", src))
    L = C.CDLL(N.LIB_PATH)
    for name in SYMBOLS:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in N.SIGNATURES, name
    assert {n for n in declared if "perf" in n} == set(SYMBOLS)


def test_struct_layouts_match_header(tmp_path):
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{os.path.abspath(HEADER)}"', "int main(void) {"]
    for cname, py in STRUCTS.items():
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        for fname, _ in py._fields_:
            lines.append(f'printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['printf("consts %d %d %d %d\\n", LC_PERF_MAX_F, LC_PERF_MAX_Q, LC_PERF_SELECT_HBM, LC_PERF_COUNT_DIRECT);',
              'printf("meta %u\\n", LC_PERF_META(3, 7, 2));', 'printf("noinv %d\\n", LC_PERF_NO_INVOKE == INT64_MIN);',
              "return 0; }"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {tuple(l.split()[:2]): int(l.split()[2]) for l in out if l and not l.startswith(("consts", "meta", "noinv"))}
    for cname, py in STRUCTS.items():
        assert got[(cname, "size")] == C.sizeof(py), cname
        for fname, _ in py._fields_:
            assert got[(cname, fname)] == getattr(py, fname).offset, (cname, fname)
    assert f"consts {N.LC_PERF_MAX_F} {N.LC_PERF_MAX_Q} {N.LC_PERF_SELECT_HBM} {N.LC_PERF_COUNT_DIRECT}" in out
    assert f"meta {3 | 7 << 8 | 2 << 16}" in out and "noinv 1" in out


def test_default_opts_are_jepsens():
    o = N.LcPerfOpts()
    N.lib().lc_perf_opts_default(C.byref(o))
    assert (o.quantile_dt_ns, o.rate_dt_ns, o.n_q, o.flags) == (30 * 10**9, 10 * 10**9, 4, 0)
    assert list(o.q)[:4] == [0.5, 0.95, 0.99, 1.0]
