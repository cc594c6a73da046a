"""Which register-tier kernel a step runs (csrc/step_plan.hpp plan_step, read
back through lc_stats.t0_path / ev_word_bytes).  Every path gives the oracle's
verdicts, so only the reported kernel name shows that a rule moved: the names
below are what the library chose for these batches before the rules were
gathered into plan_step, and what it must keep choosing."""
import numpy as np
import pytest

import cref
import linear_ref as LR
from histgen import multi_register_history
from lincheck import _native as N
from lincheck import history as H
from lincheck import model
from lincheck.checker import Device, Packed

pytestmark = pytest.mark.gpu

C5 = dict(n_keys=64, ops_per_key=1000, concurrency=10, anomaly_rate=0.2, seed=111)
# clients that think 20 x as long as an op takes: quiescent points are close
THINK = dict(n_keys=64, ops_per_key=1000, concurrency=10, mean_think=20.0, anomaly_rate=0.25, seed=112)


@pytest.fixture(scope="module")
def batches():
    out = {}
    for name, shape in (("c5", C5), ("think", THINK)):
        h = H.synth(**shape)
        _, orc = cref.check_history(h.as_c(), budget=1 << 20, threads=8)
        assert (orc["valid"] == 0).any() and (orc["valid"] == 1).any()
        out[name] = (Packed(h), orc)
    return out


def _same_as_oracle(r, orc, what):
    np.testing.assert_array_equal(r.valid, orc["valid"], err_msg=f"{what}: valid")
    np.testing.assert_array_equal(r.cause, orc["cause"], err_msg=f"{what}: cause")
    np.testing.assert_array_equal(r.fail_event, orc["fail_event"], err_msg=f"{what}: fail_event")


# (batch, Device arguments, check arguments) -> (kernel, bytes per event word read)
CASES = {
    "verdicts_only": ("c5", dict(), dict(verdicts_only=True), ("k_spec", 2)),
    "finals_no_peaks": ("c5", dict(), dict(peaks=False), ("k_spec", 2)),
    "peaks": ("c5", dict(), dict(), ("k_search_lattice", 4)),
    "split_off_spec_off": ("c5", dict(path_flags=N.LC_PATH_SPLIT_OFF | N.LC_PATH_SPEC_OFF), dict(verdicts_only=True),
                           ("k_search_lattice", 4)),
    "split_on": ("c5", dict(path_flags=N.LC_PATH_SPLIT_ON), dict(verdicts_only=True), ("k_search_segments", 4)),
    "ev32": ("c5", dict(path_flags=N.LC_PATH_EV32), dict(verdicts_only=True), ("k_spec", 4)),
    "think20_default": ("think", dict(), dict(verdicts_only=True), ("k_search_segments", 4)),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_register_tier_path(batches, case):
    batch, dev_kw, check_kw, want = CASES[case]
    pk, orc = batches[batch]
    r = Device(0, **dev_kw).check(pk, **check_kw)
    got = (r.stats["t0_path"], r.stats["ev_word_bytes"])
    print(f"{case}: t0_path {got[0]}, ev_word_bytes {got[1]}")
    _same_as_oracle(r, orc, case)
    assert got == want


def test_table_model_has_no_register_tier():
    """(model/multi-register) steps ops through lc_batch.table on the set
    tiers: no register-tier kernel, no event words read by one."""
    ops = multi_register_history(11, n_keys=40, n_ops=50, procs=5, regs=("x", "y", "z"), values=(0, 1, 2, 3),
                                 corrupt=0.3)
    pk = Packed(H.History.from_ops(ops), model.multi_register(None))
    assert pk.view.table
    r = Device(0).check(pk)
    print(f"table model: t0_path {r.stats['t0_path']}, ev_word_bytes {r.stats['ev_word_bytes']}")
    orc = LR.check_independent(ops, budget=1 << 20, model="multi-register", initial=LR.multi_register_init(None))
    want_v = {True: 1, False: 0, "unknown": -1}
    assert [int(v) for v in r.valid] == [want_v[orc[k].valid] for k in pk.keys]
    assert (r.stats["t0_path"], r.stats["ev_word_bytes"]) == ("none", 0)


def test_resident_async_node_step_path(batches):
    """An enqueued step reports its kernel at once (its times come from wait)."""
    pk, orc = batches["c5"]
    dev = Device(0)
    db = dev.upload(pk)
    st = db.check_node(pk.n_keys, asynchronous=True)
    got = (N.T0_PATH_NAMES[st.t0_path], st.ev_word_bytes)
    print(f"async node step: t0_path {got[0]}, ev_word_bytes {got[1]}")
    assert dev.wait()[0] == 1
    rec = dev.node_records(pk.n_keys).astype(np.int64)
    np.testing.assert_array_equal((rec & 0xFF) - 1, orc["valid"])
    np.testing.assert_array_equal((rec >> 8) & 0xFF, orc["cause"])
    np.testing.assert_array_equal((rec >> 16) - 1, orc["fail_event"])
    assert got == ("k_spec", 2)
