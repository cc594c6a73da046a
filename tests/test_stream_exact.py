"""The exact mode of a stream (LC_STREAM_EXACT) without a GPU: the ABI, the
refusals, a packer-only stream taking the flag, lc_stream_report against
lc_report -- the same verdict and the same final configs, built from
oracle/linear_ref.py, must render to the same words whatever the split into
appends -- and the two new kernels' code objects."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import cref
import linear_ref as LR
import stream_helpers as S
from helpers import encode_finals, oracle_state_value
from lincheck import _native as N
from lincheck import history as H
from lincheck import model
from lincheck.checker import TRUNCATE, Packed
from lincheck.independent import Tuple
from lincheck.stream import Stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "kat.json")
HEADER = os.path.join(ROOT, "include", "lincheck.h")
E_INVALID, E_UNSUPPORTED = -1, -5  # include/lincheck.h LC_E_*
MODELS = {"cas-register": model.cas_register, "register": model.register, "mutex": model.mutex}


# ---------------------------------------------------------------- ABI
def test_flag_and_report_in_header_bindings_and_library():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"#define\s+LC_STREAM_EXACT\s+2u\b", src)
    assert N.LC_STREAM_EXACT == 2 and N.LC_STREAM_EXACT & N.LC_STREAM_SET_TIER == 0
    assert re.search(r"\blc_stream_report\s*\(", src)
    assert "lc_stream_report" in N.SIGNATURES
    assert hasattr(C.CDLL(N.LIB_PATH), "lc_stream_report")
    assert N.lib().lc_abi_version() == N.LC_ABI_VERSION == 13
    m = re.search(r"#define\s+LC_STREAM_REC_WORDS\s+(\d+)", src)
    assert int(m.group(1)) == N.LC_STREAM_REC_WORDS == 1360


def open_with(flags, ctx=None):
    opts, sopts, h = N.LcPackOpts(0), N.LcStreamOpts(flags), C.c_void_p()
    rc = N.lib().lc_stream_open_opts(ctx, C.byref(opts), C.byref(sopts), C.byref(h))
    return rc, h, N.lib().lc_last_error().decode()


def test_exact_with_the_set_tier_is_refused():
    rc, h, msg = open_with(N.LC_STREAM_EXACT | N.LC_STREAM_SET_TIER)
    assert rc == E_UNSUPPORTED and not h.value
    assert "LC_STREAM_EXACT" in msg and "LC_STREAM_SET_TIER" in msg
    with pytest.raises(N.LincheckError, match="unsupported"):
        Stream(None, exact=True, set_tier=True)
    rc, h, msg = open_with(4)
    assert rc == E_INVALID and "unknown flags" in msg


def test_a_packer_only_stream_accepts_the_flag():
    rc, h, _ = open_with(N.LC_STREAM_EXACT)
    assert rc == 0 and h.value
    N.lib().lc_stream_close(h)
    h = H.synth(4, 40, concurrency=5, seed=1)
    pk = Packed(h)
    s = Stream(None, exact=True)
    S.feed(s, h, 11)
    s.finish()
    S.compare_with_packed(s, pk)
    with pytest.raises(N.LincheckError, match="packer-only"):
        s.results()
    s.close()


# ---------------------------------------------------------------- lc_stream_report against lc_report
def stream_state_ids(s, i):
    out = {}
    for st in range(1 << 16):
        try:
            out[s.state_value(i, st)] = st
        except N.LincheckError:
            break
    return out


def report(fn, handle, i, valid, fev, fin, n):
    cap = 1 << 14
    buf = np.empty(cap, np.int64)
    got = N.check(fn(handle, i, valid, fev, N.ptr(np.ascontiguousarray(fin), C.c_uint64), n, TRUNCATE,
                     N.ptr(buf, C.c_int64), cap))
    assert got <= cap
    return buf[:got].tolist()


class Case:
    """A history, lc_pack's batch of it, and for every invalid key the
    restatement's analysis with its final configs in both state numberings'
    terms (lc_pack shares one over the batch; a stream numbers per key)."""

    def __init__(self, h, model_name="cas-register", ops=None):
        self.h, self.model_name, self.mdl = h, model_name, MODELS[model_name]()
        self.pk = Packed(h, self.mdl)
        ops = ops if ops is not None else h.to_ops()
        keys, orc = cref.check_history(h.as_c(), model=model_name, threads=4)
        assert list(keys) == self.pk.keys
        self.bad = {}
        for i in np.flatnonzero(orc["valid"] == 0):
            a = LR.analysis(LR.subhistory(ops, self.pk.keys[int(i)]), model=model_name)
            assert a.valid is False and a.fail_event == orc["fail_event"][i]
            self.bad[int(i)] = a

    def finals_for_stream(self, s, i, a):
        ids = stream_state_ids(s, i)
        out = np.zeros((TRUNCATE, 2), np.uint64)
        n = 0
        for st, L in a.final_configs[:TRUNCATE]:
            mask = 0
            for q in L:
                mask |= 1 << a.final_slots[q]
            out[n, 0] = mask & ((1 << 64) - 1)
            out[n, 1] = (mask >> 64) | (ids[oracle_state_value(st, self.model_name)] << 48)
            n += 1
        return out, n

    def compare(self, s, i, label):
        a = self.bad[i]
        fin, n = encode_finals(self.pk, i, a, self.model_name)
        want = report(N.lib().lc_report, self.pk.handle, i, 0, a.fail_event, fin, n)
        fin_s, n_s = self.finals_for_stream(s, i, a)
        assert n_s == n
        got = report(N.lib().lc_stream_report, s.handle, i, 0, a.fail_event, fin_s, n_s)
        assert got == want, f"{label}, key index {i}"
        assert want[2] == n and (want[3] > 0 or not a.final_configs)

    def run(self, step, label):
        """Every invalid key's words right after the append that emits its
        failing :ok (every op of that prefix has its fate, so the words are
        final), and again after finish."""
        s = Stream(None, self.mdl, exact=True)
        assert s.exact
        done = set()

        def after(n_rows, up):
            for i, a in self.bad.items():
                if i not in done and i < up.n_keys and s.key_events(i)["emitted"] > a.fail_event:
                    done.add(i)
                    self.compare(s, i, f"{label}, {n_rows} rows")

        S.feed(s, self.h, step or max(len(self.h), 1), after)
        s.finish()
        assert s.keys == self.pk.keys
        for i in self.bad:
            self.compare(s, i, f"{label}, finished")
        s.close()
        return len(self.bad)


_cases = {}


def synth_case(name):
    if name not in _cases:
        if name == "A":
            h = H.synth(64, 200, concurrency=10, anomaly_rate=0.3, seed=7)
        elif name == "A-merged":
            h = S.merged_round_robin(synth_case("A").h)
        elif name == "I":
            h = H.synth(24, 120, concurrency=10, interleave=True, nemesis_period=5.0, anomaly_rate=0.3, seed=3)
        else:
            h = H.synth(12, 150, concurrency=10, interleave=True, nemesis_period=5.0, anomaly_rate=0.3, info_rate=0.02,
                        seed=3)
        _cases[name] = Case(h)
    return _cases[name]


@pytest.mark.parametrize("step", [1, 7, 64, 0])
@pytest.mark.parametrize("name", ["A", "A-merged", "I", "B"])
def test_report_words_equal_lc_report_on_the_anomalous_histories(name, step):
    n_bad = synth_case(name).run(step, f"{name}, step {step}")
    assert n_bad == {"A": 8, "A-merged": 8, "I": 3, "B": 2}[name]


KEYLESS_CLIENT = {"non-tuple-op-in-every-key"}  # (tests/test_stream_pack.py)


def kats():
    cases = json.load(open(GOLDEN))
    for c in cases:
        for op in c["history"]:
            v = op["value"]
            if isinstance(v, dict) and "tuple" in v:
                op["value"] = Tuple(*v["tuple"])
    return cases


def test_report_words_equal_lc_report_on_the_known_answers():
    n_bad = 0
    for c in kats():
        if not any(e["valid?"] is False for e in c["expect"].values()):
            continue
        if c["name"] in KEYLESS_CLIENT:  # a client row of every key's sub-history: no stream holds it
            with pytest.raises(N.LincheckError, match="unsupported"):
                Stream(None, MODELS[c.get("model", "cas-register")](), exact=True).append(H.History.from_ops(c["history"]))
            continue
        case = Case(H.History.from_ops(c["history"]), c.get("model", "cas-register"), c["history"])
        assert sorted(case.bad) == sorted(i for i, k in enumerate(case.pk.keys) if c["expect"][str(k)]["valid?"] is False), c["name"]
        for step in (1, 7, 64, 0):
            n_bad += case.run(step, f"{c['name']}, step {step}")
    assert n_bad >= 4 * 5


def test_report_refuses_what_it_cannot_name():
    s = Stream(None, exact=True)
    buf = np.zeros(8, np.int64)
    fin = np.zeros(2, np.uint64)
    rc = N.lib().lc_stream_report(s.handle, 0, 0, 0, N.ptr(fin, C.c_uint64), 0, 10, N.ptr(buf, C.c_int64), 8)
    assert rc == E_INVALID and b"no such key" in N.lib().lc_last_error()
    s.append([{"type": "invoke", "f": "write", "value": Tuple(1, 3), "process": 0},
              {"type": "ok", "f": "write", "value": Tuple(1, 3), "process": 0}])
    rc = N.lib().lc_stream_report(s.handle, 0, 0, 2, N.ptr(fin, C.c_uint64), 0, 10, N.ptr(buf, C.c_int64), 8)
    assert rc == E_INVALID and b"fail_event" in N.lib().lc_last_error()
    with pytest.raises(ValueError, match="exact=True"):
        Stream(None).analysis(0, [])
    s.close()


# ---------------------------------------------------------------- the code objects
K_EXACT = "_ZN3lcd14k_stream_exactENS_15StreamExactArgsE"
K_FINAL = "_ZN3lcd14k_stream_finalENS_15StreamExactArgsE"
K_STREAM = "_ZN3lcd8k_streamENS_10StreamArgsE"


def test_exact_kernels_code_objects(tmp_path):
    """k_stream_exact is the compact exact walk (the one-shot k_search_lattice<4>:
    109 VGPRs, 12,288 B of LDS, no scratch) plus a record's load and store: no
    private segment, at most 128 VGPRs (4 waves per SIMD, which the 12 KB
    workspace caps at 3.25 anyway), the 12 KB workspace.  k_stream_final keeps
    no walk state: no private segment either.  k_stream, in its own module,
    stays what it was: 97 VGPRs, 12,288 B, no private segment."""
    from test_occupancy import _kernels
    ks = _kernels(tmp_path)
    assert K_EXACT in ks and K_FINAL in ks, sorted(k for k in ks if "stream" in k)
    k = ks[K_EXACT]
    assert k["private_segment_fixed_size"] == 0, k
    assert k["vgpr_count"] <= 128, k
    assert k["group_segment_fixed_size"] == 12288, k
    assert ks[K_FINAL]["private_segment_fixed_size"] == 0, ks[K_FINAL]
    k = ks[K_STREAM]
    assert (k["vgpr_count"], k["group_segment_fixed_size"], k["private_segment_fixed_size"]) == (97, 12288, 0), k
