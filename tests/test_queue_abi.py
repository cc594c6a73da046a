"""include/lincheck_queue.h against the ctypes binding: every symbol the header
declares is exported and has a prototype, struct sizes and field offsets equal
the C compiler's, the constants agree, and the ABI version is still 13."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from lincheck import _native as N

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "lincheck_queue.h")
STRUCTS = {"lc_queue_history": N.LcQueueHistory, "lc_queue_batch": N.LcQueueBatch, "lc_queue_opts": N.LcQueueOpts,
           "lc_queue_result": N.LcQueueResult}


def declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(lc_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_exported_and_bound():
    L = C.CDLL(N.LIB_PATH)
    names = declared()
    assert len(names) == 13
    for name in names:
        assert hasattr(L, name), name
    assert set(names) == set(N.QUEUE_SIGNATURES)
    assert not set(names) & (set(N.SIGNATURES) | set(N.COUNTER_SIGNATURES))


def test_the_abi_version_stays_13():
    assert N.LC_ABI_VERSION == 13 and N.lib().lc_abi_version() == 13
    assert "#define LC_ABI_VERSION 13" in open(os.path.join(os.path.dirname(HEADER), "lincheck.h")).read()


def test_struct_layouts_match_header(tmp_path):
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{os.path.abspath(HEADER)}"', "int main(void) {"]
    for cname, py in STRUCTS.items():
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        for fname, _ in py._fields_:
            lines.append(f'printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    consts = [c for c in dir(N) if re.match(r"LC_(Q[FMKNC]|QUEUE_KEY)_", c)]
    assert len(consts) == 24
    for c in consts:
        lines.append(f'printf("const {c} %d\\n", (int){c});')
    lines += ["return 0; }"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {tuple(l.split()[:2]): int(l.split()[2]) for l in out if l}
    for cname, py in STRUCTS.items():
        assert got[(cname, "size")] == C.sizeof(py), cname
        for fname, _ in py._fields_:
            assert got[(cname, fname)] == getattr(py, fname).offset, (cname, fname)
    for c in consts:
        assert got[("const", c)] == getattr(N, c), c


def test_launch_info():
    out = np.zeros(4, np.int64)
    N.check(N.lib().lc_queue_launch_info(N.ptr(out, C.c_int64)))
    assert out.tolist() == [256, 2, 16, 8 << 30]
    assert N.lib().lc_queue_launch_info(None) == -1
