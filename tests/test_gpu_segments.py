"""Key segments (device_segments.hip): verdict-only
register-tier steps over about one key per SIMD cut each key at quiescent
points, search every segment from all start states at once (tagged lattice
words) and compose per key; a key that dies is searched again, untagged, in
the segment it died in.  Verdicts, causes and failing events must equal the
oracle's and the unsplit search's, whatever the segment length."""
import numpy as np
import pytest

import cref
from lincheck import _native as N
from lincheck import history as H
from lincheck.checker import Device, Packed

pytestmark = pytest.mark.gpu

SHAPES = {
    "c2": dict(n_keys=400, ops_per_key=1000, concurrency=10, seed=81),
    "c5": dict(n_keys=400, ops_per_key=1000, concurrency=10, anomaly_rate=0.2, seed=82),
    "late_anomalies": dict(n_keys=200, ops_per_key=2000, concurrency=8, anomaly_rate=0.5, seed=83),
    "low_concurrency": dict(n_keys=300, ops_per_key=800, concurrency=3, anomaly_rate=0.2, seed=84),
    "crashed": dict(n_keys=300, ops_per_key=800, concurrency=6, info_rate=0.002, anomaly_rate=0.2, seed=85),
    "two_values": dict(n_keys=300, ops_per_key=800, concurrency=9, n_values=2, anomaly_rate=0.2, seed=86),
}


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("seg_len", [0, 64, 1])
def test_segments_match_oracle(shape, seg_len):
    h = H.synth(**SHAPES[shape])
    pk = Packed(h)
    got = Device(0, path_flags=N.LC_PATH_SPLIT_ON, seg_len=seg_len).check(pk, verdicts_only=True)
    ref = Device(0, path_flags=N.LC_PATH_SPLIT_OFF).check(pk, verdicts_only=True)
    _, orc = cref.check_history(h.as_c(), budget=1 << 20, threads=8)
    for name, r in (("split", got), ("unsplit", ref)):
        np.testing.assert_array_equal(r.valid, orc["valid"], err_msg=f"{name} valid")
        np.testing.assert_array_equal(r.cause, orc["cause"], err_msg=f"{name} cause")
        np.testing.assert_array_equal(r.fail_event, orc["fail_event"], err_msg=f"{name} fail_event")
    if SHAPES[shape].get("anomaly_rate"):
        assert (orc["valid"] == 0).any()


# seed: chosen on the CPU for test_segments_dense_arms's preconditions
DENSE_SHAPE = dict(n_keys=32, ops_per_key=600, concurrency=10, anomaly_rate=0.2, seed=91)


def first_cut_and_pending(pk, i):
    """Key i's first possible cut -- the first position after which nothing is
    pending and a write or cas has been invoked (None: no such position
    inside the key) -- and the ops pending before each event, both from the
    packed event words (bit 31: an :ok) and the shared transition table."""
    trans = N.carray(pk.view.trans, int(pk.view.n_trans), np.uint32)
    ev = pk.events(i)
    ok = (ev >> 31).astype(bool)
    step = np.where(ok, -1, 1)
    after = np.cumsum(step)
    wrote = np.cumsum(~ok & ((trans[ev & 0xFFFFFF] & 3) >= N.LC_T_WRITE)) > 0
    cuts = np.flatnonzero((after == 0) & wrote)[:1] + 1
    cut = int(cuts[0]) if len(cuts) and cuts[0] < len(ev) else None
    return cut, after - step, ok


def test_segments_dense_arms():
    """The shared walk's dense arms (:ok with 7, 8, 9, 10 ops pending) through
    both segment kernels: tagged segments in k_search_segments, the untagged
    search of the segment a key died in in k_seg_rerun."""
    h = H.synth(**DENSE_SHAPE)
    pk = Packed(h)
    _, orc = cref.check_history(h.as_c(), budget=1 << 20, threads=8)
    # preconditions on the input (the oracle's own data, no device involved)
    assert not pk.view.trans_off  # one shared table: the batch is taggable
    reached, rerun_past_cut = set(), False
    for i in range(pk.n_keys):
        cut, pending, ok = first_cut_and_pending(pk, i)
        if cut is None:
            continue
        reached |= set(pending[cut:][ok[cut:]].tolist())
        rerun_past_cut |= orc["valid"][i] == 0 and orc["fail_event"][i] >= cut
    assert {7, 8, 9, 10} <= reached
    assert rerun_past_cut
    got = Device(0, path_flags=N.LC_PATH_SPLIT_ON, seg_len=1).check(pk, verdicts_only=True)
    ref = Device(0, path_flags=N.LC_PATH_SPLIT_OFF).check(pk, verdicts_only=True)
    for name, r in (("split", got), ("unsplit", ref)):
        np.testing.assert_array_equal(r.valid, orc["valid"], err_msg=f"{name} valid")
        np.testing.assert_array_equal(r.cause, orc["cause"], err_msg=f"{name} cause")
        np.testing.assert_array_equal(r.fail_event, orc["fail_event"], err_msg=f"{name} fail_event")


def test_segments_resident_async():
    """The bench's resident steps (node records, asynchronous) on the split path."""
    h = H.synth(n_keys=1000, ops_per_key=1000, concurrency=10, anomaly_rate=0.05, seed=87)
    pk = Packed(h)
    dev = Device(0, path_flags=N.LC_PATH_SPLIT_ON)
    db = dev.upload(pk)
    for _ in range(5):
        db.check_node(pk.n_keys, asynchronous=True)
    dev.wait()
    rec = dev.node_records(pk.n_keys).astype(np.int64)
    _, orc = cref.check_history(h.as_c(), budget=dev.budget, threads=8)
    np.testing.assert_array_equal((rec & 0xFF) - 1, orc["valid"])
    np.testing.assert_array_equal((rec >> 16) - 1, orc["fail_event"])


def test_low_overlap_split_by_default():
    """Clients that think longer than an op takes (the demo's 10 Hz per
    thread against millisecond latencies): quiescent points are frequent,
    the default choice cuts the keys, and the verdicts equal the oracle's."""
    h = H.synth(n_keys=64, ops_per_key=4000, concurrency=10, mean_think=20.0, anomaly_rate=0.25, seed=88)
    pk = Packed(h)
    dev = Device(0)
    got = dev.check(pk, verdicts_only=True)
    _, orc = cref.check_history(h.as_c(), budget=dev.budget, threads=8)
    np.testing.assert_array_equal(got.valid, orc["valid"])
    np.testing.assert_array_equal(got.fail_event, orc["fail_event"])
    assert (orc["valid"] == 0).any()
