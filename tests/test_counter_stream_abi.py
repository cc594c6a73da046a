"""include/lincheck_counter_stream.h against the ctypes binding: every symbol
the header declares is exported and has a prototype, struct sizes and field
offsets equal the C compiler's, the ABI version is still 13, and
include/lincheck_counter.h still declares exactly its names."""
import ctypes as C
import os
import re
import subprocess

from lincheck import _native as N

INCLUDE = os.path.join(os.path.dirname(__file__), "..", "include")
HEADER = os.path.join(INCLUDE, "lincheck_counter_stream.h")
STRUCTS = {"lc_counter_stream_opts": N.LcCounterStreamOpts, "lc_counter_stream_update": N.LcCounterStreamUpdate}
NAMES = ("open", "append", "counts", "results", "keys", "key_error", "last_timing", "launch_info", "close")


def declared(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(lc_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_exported_and_bound():
    L = C.CDLL(N.LIB_PATH)
    names = declared(HEADER)
    assert set(names) == {"lc_counter_stream_" + n for n in NAMES}
    for name in names:
        assert hasattr(L, name), name
    assert set(names) == set(N.COUNTER_STREAM_SIGNATURES)
    others = (set(N.SIGNATURES) | set(N.COUNTER_SIGNATURES) | set(N.QUEUE_SIGNATURES) | set(N.SETFULL_STREAM_SIGNATURES)
              | set(N.QUEUE_STREAM_SIGNATURES))
    assert not set(names) & others
    for name in names:   # the loaded library carries the prototypes
        assert getattr(N.lib(), name).argtypes == N.COUNTER_STREAM_SIGNATURES[name][1]


def test_the_abi_version_stays_13_and_the_one_shot_header_its_names():
    assert N.LC_ABI_VERSION == 13 and N.lib().lc_abi_version() == 13
    assert "#define LC_ABI_VERSION 13" in open(os.path.join(INCLUDE, "lincheck.h")).read()
    one_shot = declared(os.path.join(INCLUDE, "lincheck_counter.h"))
    assert set(one_shot) == set(N.COUNTER_SIGNATURES) and not [n for n in one_shot if "stream" in n]


def test_struct_layouts_match_header(tmp_path):
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{os.path.abspath(HEADER)}"', "int main(void) {"]
    for cname, py in STRUCTS.items():
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        for fname, _ in py._fields_:
            lines.append(f'printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
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
    # the header's structs field for field, in order
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for cname, py in STRUCTS.items():
        body = re.search(r"typedef struct %s \{(.*?)\}" % cname, src, flags=re.S).group(1)
        assert re.findall(r"(\w+);", body) == [f for f, _ in py._fields_], cname
