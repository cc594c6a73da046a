"""The streaming set-full's packer on the CPU: a packer-only stream
(lc_setfull_stream_open without a context) over random histories and the hand
example, split into appends of 1, 3 and 17 rows and all at once.  After EVERY
append the numpy emulation of the device half (tests/setfull_stream_helpers.py)
over the chunk arrays must give, for every key, exactly the fold
(setfull_helpers.restate through restate_independent) of the prefix: the
per-element tuples, counts, :valid? and the error text (the one-shot packer's).
Also here: the refusals and the ABI additions.  No GPU."""
import ctypes as C
import os
import random
import re
import subprocess

import pytest

import setfull_helpers as H
import setfull_stream_helpers as SH
from lincheck import _native as N
from lincheck.independent import Tuple
from lincheck.setfull import SetFullHistory
from lincheck.setfull_stream import SetFullStream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lincheck_setfull_stream.h")


def follow(ops, step, lin):
    """Append by append: the emulation over the chunks against the fold of every prefix."""
    emu = SH.Emu(lin)
    n_err = 0
    with SetFullStream(None, {"linearizable?": lin}) as s:
        done = 0
        for part in SH.slices(ops, step):
            u = s.append(part)
            done += len(part)
            assert u.rows == done and u.n_keys == len(s.keys()) and u.changed == []
            c = s.chunk()
            assert u.reads == len(c["row_pos"])
            emu.apply(c)
            K = len(s.keys())
            valid = [emu.valid.get(i, N.LC_UNKNOWN) if s.key_error(i) is None else N.LC_UNKNOWN for i in range(K)]
            counts = [emu.counts.get(i, [0] * 6) if s.key_error(i) is None else [0] * 6 for i in range(K)]

            def per_of(i):
                per, dup = emu.per_element(i, s.ids(i))
                mult = s.multiplicity(i)
                els = s.ids(i).tolist()
                return per, {e: int(mult[els.index(e)]) for e in dup}

            want = SH.check_prefix(s, ops[:done], lin, per_of, valid, counts)
            assert u.ids == sum(len(s.ids(i)) for i in range(K))
        n_err = sum("error" in r for r, _ in want.values())
        with pytest.raises(N.LincheckError, match="packer-only"):
            s.counts()
        with pytest.raises(N.LincheckError, match="packer-only"):
            s.results()
    return n_err


@pytest.mark.parametrize("step", [1, 3, 17, 0])
def test_hand_example(step):
    follow(H.hand_ops(), step, True)
    follow([dict(o, value=Tuple(9, o["value"])) if o["f"] in ("add", "read") else o for o in H.hand_ops()], step, False)


@pytest.mark.parametrize("step,seeds", [(1, range(0, 12)), (3, range(12, 30)), (17, range(30, 60)), (0, range(60, 120))])
def test_random_histories(step, seeds):
    """(Appends of one row re-fold every prefix: fewer and shorter histories there.)"""
    for seed in seeds:
        rng = random.Random(seed)
        ops = H.random_history(rng, max_keys=5, max_adds=20 if step == 1 else 40, error_rate=0.05 if step else 0.015)
        follow(ops, step, seed % 2 == 0)


def test_error_keys_are_followed_too():
    """Every error rule, in the middle of a keyed history, one row per append."""
    from test_setfull_host import bad_key
    n = 0
    for kind in ("nil-add", "string-add", "nil-ok-add", "ok-without-invoke", "read-without-invoke", "read-after-fail",
                 "read-not-collection", "nil-in-read"):
        good = bad_key("nil-add")[:4]
        ops = [dict(o, value=Tuple(10, o["value"])) for o in good] + [dict(o, value=Tuple(11, o["value"])) for o in bad_key(kind)] + \
              [dict(o, value=Tuple(12, o["value"])) for o in good]
        for step in (1, 5):
            n += follow(ops, step, False)
    assert n == 16


def test_read_invoked_two_appends_earlier_and_reinvocation():
    ops = [H.op("invoke", "add", 1, 0, 0), H.op("invoke", "read", None, 5, 1),              # append 0
           H.op("ok", "add", 1, 0, 2), H.op("invoke", "add", 2, 1, 3),                      # append 1
           H.op("ok", "read", [1], 5, 4), H.op("invoke", "add", 1, 0, 5),                   # append 2: read from append 0; 1 starts over
           H.op("invoke", "read", None, 5, 6), H.op("ok", "read", [1, 2, 2], 5, 7)]         # append 3
    with SetFullStream(None) as s:
        for i in range(0, 8, 2):
            s.append(ops[i:i + 2])
            c = s.chunk()
            if i == 4:
                assert c["row_inv_pos"].tolist() == [1] and c["row_inv_time"].tolist() == [10 ** 6] and c["row_pos"].tolist() == [4]
                assert c["en_flags"].tolist() == [N.LC_SFS_FRESH] and c["en_inv_pos"].tolist() == [5]
        assert s.ids(0).tolist() == [1, 2] and s.multiplicity(0).tolist() == [0, 2]  # (0: never twice in one read)
    follow(ops, 2, True)


def make(ops):
    return SetFullHistory.from_ops(ops)


def state(s):
    return (s.keys(), [s.ids(i).tolist() for i in range(len(s.keys()))], s.rows)


def test_refusals_leave_the_stream_unchanged():
    keyed = [dict(o, value=Tuple(3, o["value"])) if o["f"] in ("add", "read") else o for o in H.hand_ops()]
    plain = H.hand_ops()
    for first, other in ((keyed, plain), (plain, keyed)):
        with SetFullStream(None) as s:
            s.append(first[:10])
            before = state(s)
            with pytest.raises(N.LincheckError, match="invalid.*keyed"):
                s.append(other[10:14])
            assert state(s) == before
            bad = make(first[10:14])
            bad.type[2] = 9
            with pytest.raises(N.LincheckError, match="invalid.*bad :type / :f code"):
                s.append(bad)
            bad = make(first[10:14])
            bad.f[0] = 3
            with pytest.raises(N.LincheckError, match="bad :type / :f code"):
                s.append(bad)
            assert state(s) == before
            # and the stream goes on as if nothing had happened
            s.append(first[10:])
            assert s.rows == len(first)
        follow(first, 10, True)
    # rows without a client row fix nothing: nemesis rows first, then either kind
    nem = [H.hand_ops()[14]] * 3
    for rest in (keyed, plain):
        with SetFullStream(None) as s:
            s.append(nem)
            assert s.keys() == []
            s.append(rest[:4])
            assert s.keys() == ([3] if rest is keyed else [None]) and s.chunk()["en_inv_pos"].tolist() == [3, 5]


def test_null_arguments():
    L = N.lib()
    assert L.lc_setfull_stream_open(None, None, None) == -1
    h = C.c_void_p()
    o = N.LcSetFullOpts(0, 7, 0)
    assert L.lc_setfull_stream_open(None, C.byref(o), C.byref(h)) == -1 and b"flags" in L.lc_last_error()
    assert L.lc_setfull_stream_append(None, None, None) == -1
    assert L.lc_setfull_stream_key_error(None, 0) is None
    L.lc_setfull_stream_close(None)


# ---- the ABI additions ----------------------------------------------------------

SYMBOLS = sorted(N.SETFULL_STREAM_SIGNATURES)
STRUCTS = {"lc_setfull_stream_update": N.LcSetFullStreamUpdate, "lc_setfull_stream_chunk": N.LcSetFullStreamChunk}


def test_symbols_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(lc_[a-z0-9_]+)\s*\(", src))
    L = C.CDLL(N.LIB_PATH)
    assert declared == set(SYMBOLS) and len(SYMBOLS) == 11
    for name in SYMBOLS:
        assert name.startswith("lc_setfull_stream_") and hasattr(L, name), name
    assert N.LC_ABI_VERSION == 13 and N.lib().lc_abi_version() == 13  # additive: the version stays


def test_struct_layouts_match_header(tmp_path):
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{os.path.abspath(HEADER)}"', "int main(void) {"]
    for cname, py in STRUCTS.items():
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        for fname, _ in py._fields_:
            lines.append(f'printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['printf("consts %u %u\\n", LC_SFS_FRESH, LC_SFS_ACK);', "return 0; }"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {tuple(l.split()[:2]): int(l.split()[2]) for l in out if l and not l.startswith("consts")}
    for cname, py in STRUCTS.items():
        assert got[(cname, "size")] == C.sizeof(py), cname
        for fname, _ in py._fields_:
            assert got[(cname, fname)] == getattr(py, fname).offset, (cname, fname)
    assert f"consts {N.LC_SFS_FRESH} {N.LC_SFS_ACK}" in out
