"""k_spec decides every key it can (device_spec.hip): a key of fewer than
2 * SPEC_MIN_LEN events is one segment, walked exactly from the initial state
by wave 0; a key the packer marked with an error is finished in the verdict
step.  Only keys whose runs never met go to k_spec_rerun.  The batch
(tests/short_keys.py) straddles both length thresholds -- 0, 1, 2, 127, 128,
129, 255, 256, 257 events -- beside concurrency-10 keys of ~600 events with
9-10 ops pending, anomalies among the short and the long keys, and one
key_error key.  Verdicts, causes and failing events must equal the oracle's
and the unsegmented search's for 2, 4 and 8 segments, with the default
checkpoints and with checkpoints at the cut (so that the long keys still
rerun); with final configs asked for (the EX builds), the counts and records
must equal the unsegmented search's."""
import numpy as np
import pytest

import cref
import short_keys
from lincheck import _native as N
from lincheck.checker import Device, Packed

pytestmark = pytest.mark.gpu

OFF = N.LC_PATH_SPLIT_OFF | N.LC_PATH_SPEC_OFF
RUNS = [(segs, ck) for segs in (2, 4, 8) for ck in (None, (0, 0))]


class Batch:
    def __init__(self):
        self.hist, self.lengths = short_keys.build()
        self.pk = Packed(self.hist)
        keys, self.orc = cref.check_history(self.hist.as_c(), budget=1 << 20, threads=8)
        assert list(keys) == self.pk.keys
        self.nev = np.array([self.pk.n_events(i) for i in range(self.pk.n_keys)])
        self.plain = Device(0, path_flags=OFF).check(self.pk, verdicts_only=True)
        self.plain_fin = Device(0, path_flags=OFF, max_final=10).check(self.pk, peaks=False)


@pytest.fixture(scope="module")
def batch():
    return Batch()


def _dev(segs, ck, **kw):
    if ck is not None:
        kw["spec_ck"] = ck
    kw.setdefault("path_flags", N.LC_PATH_SPLIT_OFF)
    return Device(0, spec_segs=segs, **kw)


def test_batch_holds_what_it_should(batch):
    """Every length at the thresholds, invalid keys among the one-segment and
    the cut keys, 9-10 ops pending, the error key -- by the oracle, and the
    unsegmented search agrees with it."""
    for i, k in enumerate(batch.pk.keys):
        if k in batch.lengths:
            assert batch.nev[i] == batch.lengths[k]
    for n in short_keys.LENGTHS:
        assert (batch.nev == n).sum() >= 2, n
    assert 180 <= batch.pk.n_keys <= 230
    v = batch.orc["valid"]
    assert ((v == 0) & (batch.nev < 128)).any() and ((v == 0) & (batch.nev >= 128) & (batch.nev < 256)).any()
    assert ((v == 0) & (batch.nev >= 256) & (batch.nev < 300)).any() and ((v == 0) & (batch.nev >= 500)).any()
    assert ((v == 1) & (batch.nev < 128) & (batch.nev > 4)).any()
    width = np.ctypeslib.as_array(batch.pk.view.key_width, shape=(batch.pk.n_keys,))
    assert (width >= 9).sum() >= 50
    e = batch.pk.keys.index(short_keys.ERROR_KEY)
    assert batch.pk.key_error(e) and v[e] == -1 and batch.orc["cause"][e] == N.LC_CAUSE_ERROR
    for f in ("valid", "cause", "fail_event"):
        np.testing.assert_array_equal(getattr(batch.plain, f), batch.orc[f], err_msg=f"unsegmented: {f}")
        np.testing.assert_array_equal(getattr(batch.plain_fin, f), batch.orc[f], err_msg=f"unsegmented, finals: {f}")


@pytest.mark.parametrize("segs,ck", RUNS, ids=[f"segs{s}-{'ck0' if c else 'default'}" for s, c in RUNS])
def test_verdicts(batch, segs, ck):
    r = _dev(segs, ck).check(batch.pk, verdicts_only=True)
    assert r.stats["t0_path"] == "k_spec"
    for f in ("valid", "cause", "fail_event"):
        np.testing.assert_array_equal(getattr(r, f), batch.orc[f], err_msg=f"oracle: {f}")
        np.testing.assert_array_equal(getattr(r, f), getattr(batch.plain, f), err_msg=f"unsegmented: {f}")
    if (segs, ck) == (4, None):
        # no staging: every key's event words read from HBM, every key validated by the validation blocks
        r = _dev(segs, ck, path_flags=N.LC_PATH_SPLIT_OFF | N.LC_PATH_SPEC_NOSTAGE).check(batch.pk, verdicts_only=True)
        assert r.stats["t0_path"] == "k_spec"
        for f in ("valid", "cause", "fail_event"):
            np.testing.assert_array_equal(getattr(r, f), batch.orc[f], err_msg=f"NOSTAGE, oracle: {f}")


@pytest.mark.parametrize("segs,ck", RUNS, ids=[f"segs{s}-{'ck0' if c else 'default'}" for s, c in RUNS])
def test_final_configs(batch, segs, ck):
    ref = batch.plain_fin
    r = _dev(segs, ck, max_final=10).check(batch.pk, peaks=False)
    assert r.stats["t0_path"] == "k_spec"
    for f in ("valid", "cause", "fail_event"):
        np.testing.assert_array_equal(getattr(r, f), batch.orc[f], err_msg=f"oracle: {f}")
    for f in ("valid", "cause", "fail_event", "n_final"):
        np.testing.assert_array_equal(getattr(r, f), getattr(ref, f), err_msg=f"unsegmented: {f}")
    bad = [k for k in range(batch.pk.n_keys)
           if r.final[k, :min(int(r.n_final[k]), r.final.shape[1])].tolist() !=
           ref.final[k, :min(int(ref.n_final[k]), ref.final.shape[1])].tolist()]
    assert not bad, f"final configs differ on keys {bad[:8]} (events {batch.nev[bad[:8]].tolist()})"
