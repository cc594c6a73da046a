"""The streaming packer (csrc/host_stream.cpp) without a GPU: a packer-only
stream (lc_stream_open with no context) must emit, for any split of the rows
into appends, the words lc_pack gives for the whole history -- ok bits, slots
and descriptors decoded to register values -- and after every append exactly
the decided prefix the Python restatement (tests/stream_helpers.py) computes.
Deferral, refusals, the ABI and k_stream's code object are pinned here too."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import stream_helpers as S
from lincheck import _native as N
from lincheck import history as H
from lincheck import model
from lincheck.checker import Packed
from lincheck.independent import Tuple
from lincheck.stream import Stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "kat.json")

_hists = {}


def hist(name):
    if name not in _hists:
        if name == "A":
            h = H.synth(64, 200, concurrency=10, anomaly_rate=0.3, seed=7)
        elif name == "A-merged":
            h = S.merged_round_robin(hist("A")[0])
        elif name == "I":
            h = H.synth(24, 120, concurrency=10, interleave=True, nemesis_period=5.0, anomaly_rate=0.3, seed=3)
        elif name == "B":
            h = H.synth(12, 150, concurrency=10, interleave=True, nemesis_period=5.0, anomaly_rate=0.3, info_rate=0.02,
                        seed=3)
        elif name == "D":
            h = H.synth(8, 300, concurrency=30, info_rate=0.02, anomaly_rate=0.5, seed=4)
        _hists[name] = (h, Packed(h), S.Restated(h))
    return _hists[name]


def run(name, step):
    h, pk, rs = hist(name)
    s = Stream(None)
    index = {k: i for i, k in enumerate(rs.keys)}
    seen = [0]

    def after(n_rows, up):
        # the keys of this append's rows (every key when the append is large)
        ks = set(h.key[seen[0]:n_rows].tolist()) - {N.LC_NO_KEY} if n_rows - seen[0] <= 64 else set(rs.keys[:up.n_keys])
        seen[0] = n_rows
        assert s.keys == rs.keys[:up.n_keys]
        for k in ks:
            got = s.key_events(index[k])
            assert got["emitted"] == rs.emitted(k, n_rows), f"{name}, {n_rows} rows, key {k}"
            assert got["held"] == rs.held(k, n_rows), f"{name}, {n_rows} rows, key {k}: held"
        if len(ks) == up.n_keys:
            assert up.rows_held == sum(rs.held(k, n_rows) for k in ks)

    S.feed(s, h, step, after)
    held_max = max(s.key_events(i)["held"] for i in range(len(rs.keys)))
    s.finish()
    for i, k in enumerate(rs.keys):
        assert s.key_events(i) == {"emitted": rs.emitted(k, len(h), True), "held": 0, "deferred_at": rs.defer_at[k],
                                   "searched": 0}
    S.compare_with_packed(s, pk)
    s.close()
    return held_max


@pytest.mark.parametrize("step", [7, 64, 640, 0])
@pytest.mark.parametrize("name", ["A", "A-merged", "I", "B"])
def test_final_words_equal_lc_pack(name, step):
    run(name, step or len(hist(name)[0]))


@pytest.mark.parametrize("name", ["I", "B"])
def test_one_row_per_append(name):
    run(name, 1)


def test_restatement_matches_lc_pack_on_its_own():
    """The restatement's events (all rows appended, finished) are lc_pack's:
    the yardstick is checked against the packer it restates before it judges
    the stream."""
    for name in ("A", "I", "B", "D"):
        h, pk, rs = hist(name)
        assert rs.keys == pk.keys
        for i, k in enumerate(pk.keys):
            e = pk.events(i)
            want = np.array([(1 << 31 if ok else 0) | slot << 24 for ok, slot, _op, _r in rs.events[k]], np.uint32)
            assert np.array_equal(e & 0xFF000000, want), f"{name}, key {k}"


def first_wide_invoke(pk, i):
    e = pk.events(i)
    at = np.flatnonzero(((e >> 31) == 0) & (((e >> 24) & 0x7F) >= 10))
    return int(at[0]) if len(at) else -1


@pytest.mark.parametrize("name,n_deferred", [("A", 0), ("I", 0), ("B", 1), ("D", 8)])
def test_deferral_at_the_first_invoke_of_slot_10(name, n_deferred):
    h, pk, rs = hist(name)
    s = Stream(None)
    ups = []
    S.feed(s, h, 97, lambda n, up: ups.append(up.n_deferred))
    up = s.finish()
    want = [first_wide_invoke(pk, i) for i in range(pk.n_keys)]
    assert [s.key_events(i)["deferred_at"] for i in range(pk.n_keys)] == want
    assert sum(w >= 0 for w in want) == n_deferred == up.n_deferred
    assert ups == sorted(ups), "a deferred key stays deferred"
    s.close()


def test_33rd_state_defers():
    """32 states (nil and 31 values) stay; the invoke that interns the 33rd is the deferral point."""
    ops = []
    for v in range(40):
        ops += [{"type": "invoke", "f": "write", "value": Tuple(5, v), "process": 0},
                {"type": "ok", "f": "write", "value": Tuple(5, v), "process": 0}]
    s = Stream(None)
    s.append(ops)
    assert s.key_events(0)["deferred_at"] == 2 * 31
    assert S.Restated(H.History.from_ops(ops)).defer_at[5] == 2 * 31
    s.close()


# ---------------------------------------------------------------- the known-answer corpus
def kats():
    cases = json.load(open(GOLDEN))
    for c in cases:
        for op in c["history"]:
            v = op["value"]
            if isinstance(v, dict) and "tuple" in v:
                op["value"] = Tuple(*v["tuple"])
    return cases


MODELS = {"cas-register": model.cas_register, "register": model.register, "mutex": model.mutex}
KEYLESS_CLIENT = {"non-tuple-op-in-every-key"}


@pytest.mark.parametrize("case", kats(), ids=lambda c: c["name"])
@pytest.mark.parametrize("step", [1, 3, 0])
def test_kat_corpus_through_the_packer(case, step):
    ops = case["history"]
    m = MODELS[case["model"]]()
    h = H.History.from_ops(ops)
    s = Stream(None, m)
    if case["name"] in KEYLESS_CLIENT:
        with pytest.raises(N.LincheckError, match="unsupported"):
            s.append(h)
        assert s.keys == []
        return
    pk = Packed(h, m)
    S.feed(s, h, step or max(len(h), 1))
    s.finish()
    S.compare_with_packed(s, pk)
    s.close()


def test_corpus_covers_every_fate():
    """:fail, :info, an orphan completion (a key error) and ops open at finish
    are in the corpus; a superseded invoke is added below."""
    cases = {c["name"]: c for c in kats()}
    types = lambda n: [op["type"] for op in cases[n]["history"]]
    assert "fail" in types("failed-cas-dropped") and "info" in types("crashed-write-late")
    assert types("unmatched-invoke").count("invoke") > types("unmatched-invoke").count("ok")
    h = H.History.from_ops(cases["malformed-key-isolated"]["history"])
    assert any(Packed(h).key_error(i) for i in range(Packed(h).n_keys))


@pytest.mark.parametrize("step", [1, 2, 0])
def test_superseded_invoke_stays_pending_forever(step):
    ops = [{"type": "invoke", "f": "write", "value": Tuple(0, 1), "process": 0},
           {"type": "invoke", "f": "read", "value": Tuple(0, None), "process": 1},
           {"type": "invoke", "f": "write", "value": Tuple(0, 2), "process": 0},   # supersedes the first
           {"type": "ok", "f": "read", "value": Tuple(0, 1), "process": 1},
           {"type": "ok", "f": "write", "value": Tuple(0, 2), "process": 0},
           {"type": "invoke", "f": "read", "value": Tuple(0, None), "process": 1}]  # open at finish
    h = H.History.from_ops(ops)
    s = Stream(None)
    counts = []
    S.feed(s, h, step or len(h), lambda n, up: counts.append((n, s.key_events(0)["emitted"])))
    rs = S.Restated(h)
    assert counts == [(n, rs.emitted(0, n)) for n, _ in counts]
    if step == 1:
        # the first write is decided by the row that supersedes it; the read only by its :ok
        assert [c for _, c in counts] == [0, 0, 1, 2, 5, 5]
    s.finish()
    assert s.key_events(0)["emitted"] == 6
    S.compare_with_packed(s, Packed(h))
    assert (s.words(0)[2] >> 24) == 2  # the superseded write keeps slot 0, the read slot 1
    s.close()


def test_orphan_completion_is_a_key_error_from_then_on():
    ops = [{"type": "invoke", "f": "write", "value": Tuple(0, 1), "process": 0},
           {"type": "ok", "f": "write", "value": Tuple(0, 1), "process": 0},
           {"type": "invoke", "f": "write", "value": Tuple(1, 1), "process": 1},
           {"type": "ok", "f": "write", "value": Tuple(0, 3), "process": 7},     # no invocation
           {"type": "ok", "f": "write", "value": Tuple(1, 1), "process": 1}]
    s = Stream(None)
    s.append(ops[:3])
    assert s.key_error(0) is None and s.key_events(0)["emitted"] == 2
    s.append(ops[3:])
    assert "without a prior invocation" in s.key_error(0) and "row 3" in s.key_error(0)
    assert s.key_error(1) is None and s.key_events(1)["emitted"] == 2
    s.close()


# ---------------------------------------------------------------- refusals
def snapshot(s):
    return [(k, s.key_events(i), s.words(i).tolist(), s.trans(i).tolist()) for i, k in enumerate(s.keys)]


def test_refused_appends_leave_the_stream_unchanged():
    h, _pk, _rs = hist("I")
    s = Stream(None)
    s.append(S.rows(h, 0, 500))
    before = snapshot(s)
    good = [{"type": "invoke", "f": "write", "value": Tuple(99, 1), "process": 0}]
    bad_rows = {
        "keyless client row": ({"type": "invoke", "f": "write", "value": 3, "process": 4}, "unsupported"),
        ":txn row": ({"type": "invoke", "f": "txn", "value": Tuple(0, [["read", 1, None]]), "process": 4}, "unsupported"),
    }
    for why, (row, code) in bad_rows.items():
        with pytest.raises(N.LincheckError, match=code):
            s.append(H.History.from_ops(good + [row]))
        assert snapshot(s) == before, why
    for col, val in (("type", 4), ("f", 7)):
        hb = H.History.from_ops(good + good)
        getattr(hb, col)[1] = val
        with pytest.raises(N.LincheckError, match="invalid"):
            s.append(hb)
        assert snapshot(s) == before, col
    s.append(S.rows(h, 500, len(h)))   # and it goes on as if nothing had been refused
    s.finish()
    S.compare_with_packed(s, hist("I")[1])
    s.close()


def test_modes_do_not_mix_and_a_finished_stream_is_closed_to_rows():
    s = Stream(None)
    s.append(S.rows(hist("I")[0], 0, 10))
    b = N.LcBatch()
    with pytest.raises(N.LincheckError, match="rows mode"):
        s.push(b, [])
    s.finish()
    with pytest.raises(N.LincheckError, match="finished"):
        s.append(S.rows(hist("I")[0], 10, 20))
    s.close()
    s = Stream(None)
    with pytest.raises(N.LincheckError, match="no device"):
        s.push(b, [])
    with pytest.raises(N.LincheckError, match="searches nothing"):
        s.results()
    s.close()


def test_models_a_stream_takes():
    with pytest.raises(NotImplementedError):
        Stream(None, model.multi_register({}))
    o = N.LcPackOpts(N.LC_MODEL_MULTI_REGISTER)
    h = C.c_void_p()
    assert N.lib().lc_stream_open(None, C.byref(o), C.byref(h)) == -5
    from lincheck import checker
    with pytest.raises(NotImplementedError):
        checker.linearizable({"model": model.cas_register(), "algorithm": "wgl"}).stream()
    # (model/register) refuses a cas per key, as lc_pack does
    s = Stream(None, model.register())
    s.append([{"type": "invoke", "f": "cas", "value": Tuple(0, [1, 2]), "process": 0},
              {"type": "invoke", "f": "write", "value": Tuple(1, 2), "process": 1}])
    assert "cannot step" in s.key_error(0) and s.key_error(1) is None
    s.close()


# ---------------------------------------------------------------- ABI
STREAM_NAMES = ["lc_stream_open", "lc_stream_append", "lc_stream_push", "lc_stream_finish", "lc_stream_results",
                "lc_stream_keys", "lc_stream_key_events", "lc_stream_event_row", "lc_stream_close"]


def test_abi_lists_the_stream_and_stays_13():
    src = open(os.path.join(ROOT, "include", "lincheck.h")).read()
    assert re.search(r"#define LC_ABI_VERSION 13\b", src) and N.LC_ABI_VERSION == 13 and N.lib().lc_abi_version() == 13
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in STREAM_NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in N.SIGNATURES and hasattr(N.lib(), name)
    assert int(re.search(r"#define LC_STREAM_REC_WORDS (\d+)", src).group(1)) == N.LC_STREAM_REC_WORDS


def test_update_struct_layout(tmp_path):
    import subprocess
    fields = [f for f, _ in N.LcStreamUpdate._fields_]
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{os.path.join(ROOT, "include", "lincheck.h")}"',
             "int main(void) {", 'printf("%zu\\n", sizeof(lc_stream_update));']
    lines += [f'printf("%zu\\n", offsetof(lc_stream_update, {f}));' for f in fields] + ["return 0; }"]
    (tmp_path / "l.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-o", str(tmp_path / "l"), str(tmp_path / "l.c")], check=True)
    out = [int(x) for x in subprocess.run([str(tmp_path / "l")], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [C.sizeof(N.LcStreamUpdate)] + [getattr(N.LcStreamUpdate, f).offset for f in fields]


# ---------------------------------------------------------------- k_stream's code object
def test_k_stream_keeps_the_compact_build_s_footprint(tmp_path):
    """k_stream is the compact FAST walk plus a record's load and store.  The
    parent's k_search_lattice<4> is 109 VGPRs, 12,288 B of LDS and no scratch;
    at 12 KB per wave LDS caps residency at 3.25 waves per SIMD, which 128
    VGPRs (4 waves) do not lower.  So: no private segment, at most 128 VGPRs,
    the 12 KB workspace."""
    from test_occupancy import _kernels
    ks = _kernels(tmp_path)
    name = "_ZN3lcd8k_streamENS_10StreamArgsE"
    assert name in ks, "k_stream is not in the code object"
    k = ks[name]
    assert k["private_segment_fixed_size"] == 0, k
    assert k["vgpr_count"] <= 128, k
    assert k["group_segment_fixed_size"] == 12288, k
