"""k_spec with meeting by set size and closed sets at 7-10 ops pending
(device_spec.hip, lattice_core.hpp ok_reg_closed / ok_event_mem_closed):
verdicts, causes and failing events equal the oracle's, exactly, on small
batches built so that the new paths run -- :oks at 7, 8, 9 and 10 pending,
clean ones (no invoke since the last :ok) among them, failing :oks before and
after the runs' meeting points, keys of 2 x SPEC_MIN_LEN events (the shortest
k_spec cuts in two) and keys with all 8 segments.  The same batches through
the exact-set path (final configs, k_spec<.., EX>) keep its records."""
import numpy as np
import pytest

import cref
import edgegen
from edgegen import NEV, TARGETS, Plan, counts, crashed_late, dips, long_lived, rolling
from lincheck import _native as N
from lincheck import history as H
from lincheck.checker import Device, Packed

pytestmark = pytest.mark.gpu

SHORT = 2 * edgegen.SPEC_MIN_LEN  # events of the shortest key cut in two

SYNTH = {
    # (about 1,150 events per key: 8 segments; the short think time keeps more ops in flight)
    "clean": dict(n_keys=48, ops_per_key=800, concurrency=10, mean_think=0.5, seed=3),
    # (every key anomalous: about half of them detectably so)
    "half_invalid": dict(n_keys=48, ops_per_key=800, concurrency=10, mean_think=0.5, anomaly_rate=1.0, seed=4),
    "lingering": dict(n_keys=48, ops_per_key=800, concurrency=10, info_rate=0.003, anomaly_rate=0.2, seed=6),
}


def _edge_cases():
    """tests/edgegen.py's 7-10-pending profiles (8 segments each), and keys of
    SHORT events (two segments) and one event fewer (none)."""
    cases = []
    for P in (7, 8, 9, 10):
        cases += edgegen.both(f"rolling{P}", rolling(NEV, P))
    cases += edgegen.both("rolling7_invoke_first", rolling(NEV, 7, first="invoke"))
    cases += edgegen.both("dip6_every_target", dips(NEV, 10, 6, TARGETS, wide=True))
    cases += edgegen.both("dip3_every_target", dips(NEV, 9, 3, TARGETS, wide=True))
    cases += edgegen.both("long_lived_slot0", long_lived(NEV, 0, where=TARGETS))
    cases += edgegen.both("crashed_write_read_late", crashed_late(NEV, 3, where=TARGETS))
    for nev in (SHORT, SHORT - 2):
        mid = nev // 2
        for hi in (8, 10):
            plan = Plan(nev, counts(nev, hi, [(edgegen.dip_boundary(mid, 4), 4)], drain=True, wide=True))
            cases.append((f"len{nev}_hi{hi}-valid", plan))
            # a failing :ok right after the cut (before any meeting point) and well past it
            cases.append((f"len{nev}_hi{hi}-stale_after_cut", plan.with_anomalies((mid + 2, "stale"))))
            cases.append((f"len{nev}_hi{hi}-garbage_late", plan.with_anomalies((mid + 60, "garbage"))))
    return cases


def _batches():
    out = {name: Packed(H.synth(**kw)) for name, kw in SYNTH.items()}
    hists = {name: H.synth(**kw) for name, kw in SYNTH.items()}
    b = edgegen.batch(_edge_cases(), seed=21)
    out["edges"], hists["edges"] = b.pk, b.hist
    return out, hists


def _ok_histogram(pk):
    """From the packed words: :oks by ops pending before them, and the clean
    ones (the event before is an :ok too) at 7 or more pending."""
    by_pending, clean_dense = {}, 0
    for k in range(pk.n_keys):
        c = edgegen.pending_before(pk, k)
        ok = c[1:] < c[:-1]
        for b in np.nonzero(ok)[0]:
            by_pending[int(c[b])] = by_pending.get(int(c[b]), 0) + 1
            if c[b] >= 7 and b > 0 and ok[b - 1]:
                clean_dense += 1
    return by_pending, clean_dense


@pytest.fixture(scope="module")
def batches():
    pks, hists = _batches()
    out = {}
    for name, pk in pks.items():
        _, orc = cref.check_history(hists[name].as_c(), budget=1 << 20, threads=8)
        out[name] = (pk, orc)
    return out


@pytest.mark.parametrize("name", ["clean", "half_invalid", "lingering", "edges"])
def test_batch_runs_the_new_paths(batches, name):
    """The precondition on the inputs, from the packed words alone."""
    pk, orc = batches[name]
    by_pending, clean_dense = _ok_histogram(pk)
    for n in (7, 8, 9, 10):
        assert by_pending.get(n, 0) > 0, f"{name}: no :ok at {n} pending ({by_pending})"
    assert clean_dense > 0, f"{name}: no clean :ok at 7 or more pending"
    nev = np.diff(np.asarray(pk.ev_off)).astype(np.int64)
    assert (nev >= 8 * edgegen.SPEC_MIN_LEN).any(), "no key with all 8 segments"
    if name == "edges":
        assert (nev == SHORT).any() and (nev == SHORT - 2).any()
    if name == "half_invalid":
        bad = int((orc["valid"] == 0).sum())
        assert pk.n_keys // 4 <= bad <= 3 * pk.n_keys // 4, f"{bad} of {pk.n_keys} keys invalid"
    if name == "clean":
        assert (orc["valid"] == 1).all()


@pytest.mark.parametrize("name", ["clean", "half_invalid", "lingering", "edges"])
def test_verdict_records_equal_the_oracle(batches, name):
    pk, orc = batches[name]
    runs = [("default", dict())]
    runs += [(f"segs {s}", dict(path_flags=N.LC_PATH_SPLIT_OFF, spec_segs=s)) for s in (2, 3, 4, 6, 8)]
    runs += [("segs 8, ck (1, 2)", dict(path_flags=N.LC_PATH_SPLIT_OFF, spec_segs=8, spec_ck=(1, 2))),
             ("segs 8, 32-bit words", dict(path_flags=N.LC_PATH_SPLIT_OFF | N.LC_PATH_EV32, spec_segs=8))]
    for what, kw in runs:
        r = Device(0, **kw).check(pk, verdicts_only=True)
        for f in ("valid", "cause", "fail_event"):
            np.testing.assert_array_equal(getattr(r, f), orc[f], err_msg=f"{name}, {what}: {f}")


@pytest.mark.parametrize("name", ["clean", "half_invalid", "lingering", "edges"])
def test_exact_path_records_unchanged(batches, name):
    """lc_check_batch with final configs (k_spec<.., EX>: exact sets, no
    meeting entries): the unsegmented exact search's records."""
    pk, orc = batches[name]
    ref = Device(0, path_flags=N.LC_PATH_SPLIT_OFF | N.LC_PATH_SPEC_OFF).check(pk, peaks=False)
    for f in ("valid", "cause", "fail_event"):
        np.testing.assert_array_equal(getattr(ref, f), orc[f], err_msg=f"{name}, unsegmented: {f}")
    for what, kw in [("default", dict()), ("segs 8", dict(path_flags=N.LC_PATH_SPLIT_OFF, spec_segs=8))]:
        r = Device(0, **kw).check(pk, peaks=False)
        for f in ("valid", "cause", "fail_event", "n_final"):
            np.testing.assert_array_equal(getattr(r, f), getattr(ref, f), err_msg=f"{name}, {what}: {f}")
        bad = [k for k in range(pk.n_keys) if r.final[k, :r.n_final[k]].tolist() != ref.final[k, :ref.n_final[k]].tolist()]
        assert not bad, f"{name}, {what}: final configs differ on keys {bad[:8]}"
