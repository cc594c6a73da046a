"""checker/set-full on the CPU: the two oracles of tests/setfull_helpers.py
against each other and against the hand example, lc_setfull_pack's arrays
decoded back against the fold's inputs, the error rules, the EDN reader, the
ABI additions and the new kernels' resources.  No GPU."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

import setfull_helpers as H
from lincheck import _native as N
from lincheck.independent import Tuple
from lincheck.setfull import (PackedSetFull, SetFullHistory, elements_of, multiplicities, quantile_map, result_map,
                              synth_set_full)
from set_helpers import is_int, keys_of
from test_occupancy import LDS_PER_CU, LLVM, SO

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "lincheck.h")
SEEDS = range(200)


@pytest.fixture(scope="module")
def histories():
    """The random histories and the fold's answer for each key, computed once."""
    out = []
    for seed in SEEDS:
        ops = H.random_history(random.Random(seed))
        out.append((ops, H.restate_independent(ops, linearizable=True)))
    return out


def test_most_random_keys_are_checked(histories):
    """The fold alone decides: at least 90 % of the generated keys are
    checked, not error, keys -- and there are at least 500 of them."""
    keys = [r for _, want in histories for r, _ in want.values()]
    checked = [r for r in keys if "error" not in r]
    assert len(checked) >= 0.9 * len(keys), (len(checked), len(keys))
    assert len(checked) >= 500
    assert len(checked) < len(keys)  # the error rules are exercised too
    seen = {str(r["valid?"]) for r in checked}
    assert seen == {"True", "False", "unknown"}
    assert any(r["stale"] for r in checked) and any(r["lost"] for r in checked) and any(r["duplicated"] for r in checked)


def test_fold_equals_matrix(histories):
    test_most_random_keys_are_checked(histories)
    n = 0
    for ops, want in histories:
        pos = H.with_pos(ops)
        for k, (r, per) in want.items():
            if "error" in r:
                continue
            mine = pos if k is None else H.sub(pos, k)
            for lin in (True, False):
                r2, per2 = H.restate_matrix(mine, lin)
                r1 = r if lin else H.restate(mine, False)[0]
                assert H.norm(r2) == H.norm(r1), (k, r1, r2)
                assert per2 == per
            n += 1
    assert n >= 500


def test_hand_example_literally():
    ops = H.with_pos(H.hand_ops())
    for how in (H.restate, H.restate_matrix):
        r, per = how(ops, True)
        assert per == H.HAND_PER
        assert {k: r[k] for k in H.HAND_WANT} == H.HAND_WANT
        assert [w["element"] for w in r["worst-stale"]] == H.HAND_WORST
        assert r["worst-stale"][0]["known"]["index"] == 7 and r["worst-stale"][0]["last-absent"]["index"] == 12
        assert how(ops, False)[0]["valid?"] is False  # element 4 is lost either way


def decode(ops, k):
    """What lc_setfull_pack should hold of one checked key, from its ops."""
    last_inv, ack, open_read, rows = {}, {}, {}, []
    for op in ops:
        if not is_int(op.get("process")):
            continue
        if op["f"] == "add" and op["type"] == "invoke":
            last_inv[op["value"]] = op["pos"]
            ack.pop(op["value"], None)
        elif op["f"] == "add" and op["type"] == "ok":
            ack.setdefault(op["value"], (op["pos"], op["time"]))
        elif op["f"] == "read" and op["type"] == "invoke":
            open_read[op["process"]] = op
        elif op["f"] == "read" and op["type"] == "fail":
            open_read.pop(op["process"], None)
        elif op["f"] == "read" and op["type"] == "ok":
            inv = open_read[op["process"]]
            rows.append((op["pos"], op["time"], inv["pos"], inv["time"], list(op["value"] or [])))
    return last_inv, ack, rows


def test_pack_decodes_to_the_folds_inputs(histories):
    forms = set()
    for ops, want in histories[:120]:
        packed = PackedSetFull(SetFullHistory.from_ops(ops))
        a = packed.arrays()
        pos = H.with_pos(ops)
        assert packed.keys == (keys_of(ops) or [None])
        for i, k in enumerate(packed.keys):
            r, _ = want[k]
            assert (packed.status[i] == N.LC_SET_KEY_OK) == ("error" not in r), (k, r, packed.key_error(i))
            if "error" in r:
                assert packed.key_error(i)
                assert a["span"][i] == 0 and a["row_off"][i] == a["row_off"][i + 1]
                continue
            last_inv, ack, rows = decode(pos if k is None else H.sub(pos, k), k)
            forms.add(int(a["rank"][i]))
            b, n = int(a["id_off"][i]), int(a["span"][i])
            els = elements_of(a, i, range(n))
            assert els == sorted(els) and len(set(els)) == n
            got_inv = {e: int(a["inv_pos"][b + x]) for x, e in enumerate(els) if a["inv_pos"][b + x] >= 0}
            assert got_inv == last_inv
            got_ack = {e: (int(a["ack_pos"][b + x]), int(a["ack_time"][b + x])) for x, e in enumerate(els) if a["ack_pos"][b + x] >= 0}
            assert got_ack == ack
            r0, r1 = int(a["row_off"][i]), int(a["row_off"][i + 1])
            got_rows = [(int(a["row_pos"][r]), int(a["row_time"][r]), int(a["row_inv_pos"][r]), int(a["row_inv_time"][r]),
                         [els[x] for x in a["read_id"][int(a["el_off"][r]):int(a["el_off"][r + 1])]]) for r in range(r0, r1)]
            assert got_rows == rows
    assert forms == {0, 1}  # offset ids and rank ids


def bad_key(kind):
    base = [H.op("invoke", "add", 1, 0, 0), H.op("ok", "add", 1, 0, 1), H.op("invoke", "read", None, 5, 2),
            H.op("ok", "read", [1], 5, 3)]
    extra = {"nil-add": [H.op("invoke", "add", None, 1, 4)],
             "string-add": [H.op("invoke", "add", "x", 1, 4)],
             "nil-ok-add": [H.op("ok", "add", None, 1, 4)],
             "ok-without-invoke": [H.op("ok", "add", 2, 1, 4)],
             "read-without-invoke": [H.op("ok", "read", [1], 6, 4)],
             "read-after-fail": [H.op("invoke", "read", None, 6, 4), H.op("fail", "read", None, 6, 5), H.op("ok", "read", [1], 6, 6)],
             "read-not-collection": [H.op("invoke", "read", None, 6, 4), H.op("ok", "read", 7, 6, 5)],
             "nil-in-read": [H.op("invoke", "read", None, 6, 4), H.op("ok", "read", [1, None], 6, 5)]}[kind]
    return base + extra


@pytest.mark.parametrize("kind", ["nil-add", "string-add", "nil-ok-add", "ok-without-invoke", "read-without-invoke",
                                  "read-after-fail", "read-not-collection", "nil-in-read"])
def test_error_rules(kind):
    """Each error rule makes its key :unknown with an :error -- in the fold
    and in the pack -- and leaves the keys around it alone."""
    good = bad_key("nil-add")[:4]
    ops = [dict(o, value=Tuple(10, o["value"])) for o in good] + [dict(o, value=Tuple(11, o["value"])) for o in bad_key(kind)] + \
          [dict(o, value=Tuple(12, o["value"])) for o in good]
    want = H.restate_independent(ops)
    assert want[11][0]["valid?"] == "unknown" and "error" in want[11][0]
    assert "error" not in want[10][0] and "error" not in want[12][0]
    packed = PackedSetFull(SetFullHistory.from_ops(ops))
    assert packed.keys == [10, 11, 12] and packed.status.tolist() == [0, N.LC_SET_KEY_ERROR, 0]
    got = result_map(packed, None, 1)
    assert got["valid?"] == "unknown" and got["error"] == packed.key_error(1) and len(got["error"]) > 10
    assert packed.key_error(0) is None and packed.key_error(2) is None
    a = packed.arrays()
    assert a["span"].tolist() == [1, 0, 1] and a["row_off"].tolist() == [0, 1, 1, 2]
    assert a["inv_pos"].tolist() == [0, len(ops) - 4] and a["read_id"].tolist() == [0, 0]


def test_ignored_rows_are_no_errors():
    """:fail / :info adds of nil, an :invoke :read's value, nemesis rows with
    anything in them and an :info :read without an invocation change nothing."""
    ops = bad_key("nil-add")[:4] + [H.op("fail", "add", None, 1, 4), H.op("info", "add", None, 1, 5),
                                    dict(H.op("ok", "add", 99, 0, 6), process="nemesis"),
                                    dict(H.op("ok", "read", 7, 0, 7), process="nemesis"), H.op("info", "read", None, 9, 8)]
    assert "error" not in H.restate(H.with_pos(ops))[0]
    packed = PackedSetFull(SetFullHistory.from_ops(ops))
    assert packed.status.tolist() == [0] and packed.arrays()["span"].tolist() == [1]


def test_edn_reader_equals_from_ops(tmp_path, histories):
    n = 0
    for ops, _ in histories[:60]:
        # (a keyed read of a bare integer, [k 7], reads as a plain two-element read: lc_edn_read_set's rule)
        if any(o["f"] == "read" and isinstance(o["value"], Tuple) and is_int(o["value"][1]) for o in ops):
            continue
        n += 1
        text = H.edn_lines(ops)
        a, b = SetFullHistory.parse_edn(text), SetFullHistory.from_ops(ops)
        for name in ("type", "f", "elem", "read_off", "index", "process", "time"):
            assert np.array_equal(getattr(a, name), getattr(b, name)), name
        assert np.array_equal(a.read_elem[:a.read_off[-1]], b.read_elem[:b.read_off[-1]])
        keyed = b.key is not None and (b.key != N.LC_NO_KEY).any()
        assert np.array_equal(a.key, b.key) if keyed else (a.key == N.LC_NO_KEY).all()
    assert n >= 40
    path = tmp_path / "history.edn"
    path.write_text(H.edn_lines(H.hand_ops()))
    h = SetFullHistory.read_edn(str(path))
    assert h.process.tolist()[14] == N.LC_NO_PROCESS and h.time.tolist()[13] == 20 * 10 ** 6
    want = [dict(o, index=i) for i, o in enumerate(H.hand_ops())]
    want[14]["f"] = "other"  # the nemesis row: the set reader keeps no other :f
    assert want == h.to_ops()


def test_host_side_statistics():
    assert quantile_map(np.array([5, 0, 1, 0])) == {0: 0, 0.5: 1, 0.95: 5, 0.99: 5, 1: 5}
    assert quantile_map(np.array([13])) == {q: 13 for q in (0, 0.5, 0.95, 0.99, 1)}
    packed = PackedSetFull(SetFullHistory.from_ops(H.hand_ops()))
    a = packed.arrays()
    assert a["span"].tolist() == [7] and a["rank"].tolist() == [0]
    assert multiplicities(a, 0, np.array([3], np.uint32)) == {3: 2}
    assert multiplicities(a, 0, np.array([0, 3], np.uint32)) == {0: 1, 3: 2}


def test_synth_is_what_it_says():
    h = synth_set_full(n_keys=2, adds_per_key=60, read_every=10, stale_window=3, lost_rate=0.1, overlap=True, seed=3)
    want = H.restate_independent(h.to_ops(), linearizable=True)
    assert set(want) == {0, 1}
    for r, per in want.values():
        assert r["attempt-count"] == 60 and r["lost-count"] > 0 and r["stale-count"] > 0 and not r["duplicated"]
        assert r["stable-count"] + r["lost-count"] == 60 and r["valid?"] is False
    r, _ = H.restate_independent(synth_set_full(adds_per_key=50, read_every=7).to_ops(), linearizable=True)[None]
    assert r["valid?"] is True and r["stable-count"] == 50 and r["stale-count"] == 0


# ---- the ABI additions ----------------------------------------------------------

STRUCTS = {"lc_setfull_history": N.LcSetFullHistory, "lc_setfull_batch": N.LcSetFullBatch,
           "lc_setfull_opts": N.LcSetFullOpts, "lc_setfull_result": N.LcSetFullResult}
SYMBOLS = ["lc_setfull_pack", "lc_setfull_packed_free", "lc_setfull_packed_view", "lc_setfull_packed_keys",
           "lc_setfull_packed_key_error", "lc_setfull_check", "lc_setfull_last_timing", "lc_setfull_launch_info",
           "lc_edn_read_setfull", "lc_edn_parse_setfull", "lc_setfull_hist_view", "lc_setfull_hist_free"]


def test_symbols_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(lc_[a-z0-9_]+)\s*\(", src))
    L = C.CDLL(N.LIB_PATH)
    for name in SYMBOLS:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in N.SIGNATURES, name
    assert {n for n in declared if "setfull" in n} == set(SYMBOLS)
    assert not any("perf" in n for n in SYMBOLS)
    assert N.LC_ABI_VERSION == 13 and N.lib().lc_abi_version() == 13


def test_struct_layouts_match_header(tmp_path):
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{os.path.abspath(HEADER)}"', "int main(void) {"]
    for cname, py in STRUCTS.items():
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        for fname, _ in py._fields_:
            lines.append(f'printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['printf("consts %d %d %d %d %d %u\\n", LC_SETFULL_NONE, LC_SETFULL_UNTRACKED, LC_SETFULL_STABLE, '
              'LC_SETFULL_LOST, LC_SETFULL_NEVER_READ, LC_SETFULL_MARK_DIRECT);', "return 0; }"]
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
    assert (f"consts {N.LC_SETFULL_NONE} {N.LC_SETFULL_UNTRACKED} {N.LC_SETFULL_STABLE} {N.LC_SETFULL_LOST} "
            f"{N.LC_SETFULL_NEVER_READ} {N.LC_SETFULL_MARK_DIRECT}") in out


def test_bad_batches_are_refused_before_any_device_work():
    """lc_setfull_check's null checks come first (no context needed to fail)."""
    assert N.lib().lc_setfull_check(None, None, None, None) == -1
    assert b"lc_setfull_check" in N.lib().lc_last_error()


# ---- the new kernels' resources (from the code object, no GPU) ---------------------

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
KERNEL_LIB = os.path.join(os.path.dirname(SO), "libsetfull_kernels.so")  # liblincheck.so links it (the Makefile says why)


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """The kernel descriptors of the set-full kernels' library (as tests/test_set_kernels.py reads k_set_*)."""
    for tool in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"):
        if not os.path.exists(os.path.join(LLVM, tool)):
            pytest.skip(f"{tool} not in {LLVM}")
    tmp = tmp_path_factory.mktemp("setfull_kernels")
    fat = str(tmp / "fat.bin")
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", KERNEL_LIB, str(tmp / "x")],
                   check=True, capture_output=True)
    data = open(fat, "rb").read()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), data)]
    out = {}
    for i, b in enumerate(starts):
        part, co = str(tmp / f"bundle{i}.bin"), str(tmp / f"k{i}.co")
        with open(part, "wb") as f:
            f.write(data[b:starts[i + 1] if i + 1 < len(starts) else len(data)])
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={part}",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True, capture_output=True)
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True,
                               text=True).stdout
        for block in re.split(r"\n  - \.agpr_count:", notes):
            m = re.search(r"\.name:\s+(\S+)", block)
            if m:
                out[m.group(1)] = {k: int(v) for k, v in re.findall(
                    r"\.(vgpr_count|group_segment_fixed_size|private_segment_fixed_size):\s+(\d+)", block)}
    return out


@pytest.mark.parametrize("stem", ["k_setfull_mark", "k_setfull_scan", "k_setfull_finish"])
def test_kernel_resources(kernels, stem):
    """No scratch, and what DESIGN 3.12's occupancy needs: eight workgroups of
    four waves per CU -- at most 64 VGPRs (8 waves per SIMD) and an eighth of
    the CU's LDS per workgroup."""
    mine = {n: k for n, k in kernels.items() if stem in n}
    assert len(mine) == 1 and len(kernels) == 3, sorted(kernels)
    for name, k in mine.items():
        assert k["private_segment_fixed_size"] == 0, f"{name}: {k}"
        assert k["vgpr_count"] <= 64, f"{name}: {k}"
        assert 8 * k["group_segment_fixed_size"] <= LDS_PER_CU, f"{name}: {k}"
