"""k_spec_rerun as one-wave workgroups on the lane's own k_spec workspaces
(device_spec.hip, StepPlan::rerun_grid).  Checkpoints at the cut (spec_ck
(0, 0)) leave most cut keys to the rerun launch: nine alternating
lc_check_node_async steps on the two lanes, a buffer each, over a batch with
more rerun keys than the rerun grid has waves (600 keys x 300 ops: the
grid-stride loop), and over a batch whose reruns cross 9-10 ops pending
(concurrency 10, mean_think 0.3: the lattice in the wave's global workspace
slot, which belongs to the same lane's k_spec until that launch has ended).
Every step's bytes must equal lc_check_node's on a fresh context."""
import numpy as np
import pytest

from lincheck import _native as N
from lincheck import history as H
from lincheck import parallel as P
from lincheck.checker import Device, Packed, PinnedRecords

pytestmark = pytest.mark.gpu

PAD = 3
SHAPES = {
    "A": dict(n_keys=600, ops_per_key=300, concurrency=10, anomaly_rate=0.2, seed=401),
    "W": dict(n_keys=100, ops_per_key=600, concurrency=10, mean_think=0.3, anomaly_rate=0.2, seed=402),
}


class Case:
    def __init__(self, name):
        self.hist = H.synth(**SHAPES[name])
        self.pk = Packed(self.hist)
        self.block = self.pk.n_keys + PAD
        self.ref = Device(0).check_node(self.pk, self.block)[0].copy()  # a fresh context, synchronous


@pytest.fixture(scope="module")
def cases():
    cs = {name: Case(name) for name in SHAPES}
    for c in cs.values():
        assert c.ref.size == c.block and not c.ref[-PAD:].any()
        valid = P.unpack_records(c.ref.astype(np.int64))[0][:c.pk.n_keys]
        assert valid.min() == 0 and valid.max() == 1  # invalid and valid keys in each
    # keys long enough to be cut (so that they can miss and rerun), 9-10 ops pending in W
    for c in cs.values():
        assert min(c.pk.n_events(i) for i in range(c.pk.n_keys)) >= 256
    width = np.ctypeslib.as_array(cs["W"].pk.view.key_width, shape=(cs["W"].pk.n_keys,))
    assert (width >= 9).sum() >= 50
    return cs


@pytest.mark.parametrize("segs", [8, 4, 2])
def test_nine_steps_of_reruns_on_two_lanes(cases, segs):
    dev = Device(0, path_flags=N.LC_PATH_SPLIT_OFF, spec_segs=segs, spec_ck=(0, 0))
    names = ["A", "W"] * 4 + ["A"]
    bufs = [PinnedRecords(cases[name].block) for name in names]
    for name, b in zip(names, bufs):
        enq, _ = dev.check_node_async(cases[name].pk, cases[name].block, b)
        assert enq
    assert dev.wait()[0] == len(names)
    for i, (name, b) in enumerate(zip(names, bufs)):
        np.testing.assert_array_equal(np.asarray(b), cases[name].ref, err_msg=f"step {i} ({name})")


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_same_batch_on_both_lanes(cases, name):
    """The same batch nine times: both lanes' rerun lists and workspace slots
    in use at once for equal work."""
    dev = Device(0, path_flags=N.LC_PATH_SPLIT_OFF, spec_ck=(0, 0))
    bufs = [PinnedRecords(cases[name].block) for _ in range(9)]
    for b in bufs:
        enq, _ = dev.check_node_async(cases[name].pk, cases[name].block, b)
        assert enq
    assert dev.wait()[0] == 9
    for i, b in enumerate(bufs):
        np.testing.assert_array_equal(np.asarray(b), cases[name].ref, err_msg=f"step {i}")
