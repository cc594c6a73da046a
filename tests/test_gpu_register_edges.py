"""The register tier (lattice_core.hpp, device_lattice.hip, device_spec.hip) on
histories built to a schedule
(tests/edgegen.py): ragged batches with keys on both sides of every length
threshold, chosen pending counts at the cut windows of the speculative
segments, several waves in the 9-10-pending workspaces at once, failing :oks
placed against cuts and checkpoints, more than one anomaly per key, and
batches at the state and width limits.  Every batch goes through every
register-tier path; verdicts, causes and failing events (and peaks, final
configs where the path gives them) must equal the oracle's bit for bit, and a
pinned path must be the one reported.  tests/test_edgegen.py asserts, without
a GPU, that each batch is the edge case it is named for."""
from types import SimpleNamespace

import numpy as np
import pytest

import cref
import edgegen as E
from lincheck import _native as N
from lincheck import parallel as P
from lincheck.checker import Device

pytestmark = pytest.mark.gpu

OFF = N.LC_PATH_SPLIT_OFF | N.LC_PATH_SPEC_OFF
CU_COUNT = 256  # the MI355X's; k_search_segments takes at most 8 keys per CU (step_plan.hpp:82)

# groups of runs per batch; "compact" (2,600 keys) takes the unsegmented paths and the default
GROUPS = ("unsegmented", "spec", "spec_flags", "exact", "split", "node")
BATCH_GROUPS = {name: (("unsegmented", "node") if name == "compact" else GROUPS) for name in sorted(E.BATCHES)}


class Loaded:
    """A batch, the oracle's records for it, and the runs made so far."""

    def __init__(self, name):
        self.name = name
        self.b = E.get(name)
        keys, self.orc = cref.check_history(self.b.hist.as_c(), budget=1 << 20, threads=8)
        assert list(keys) == self.b.pk.keys
        pk = self.b.pk
        width = max(max(p.c) for p in self.b.plans)
        states = E.batch_states(pk)
        # what dev_search's rules (step_plan.hpp, device_api.hip batch_shape) make of the batch
        self.t0_only = bool(width <= E.T0_MAX_WIDTH and (states <= E.T0_MAX_STATES).all())
        trans = N.carray(pk.view.trans, int(pk.view.n_trans), np.uint32).tolist()
        installs_nil = any((t & 3) >= N.LC_T_WRITE and (t >> 17) == 0 for t in trans)
        self.taggable = bool(not pk.view.trans_off and states.max() <= E.TAGGABLE_MAX_STATES and not installs_nil)
        self.runs = {}  # group -> [(label, KeyResults, fields compared with the oracle)]
        self.ref = None

    def spec_path(self):
        return "k_spec" if self.t0_only else "k_search_lattice"

    def check(self, label, r, path=None, peak=False):
        if path is not None:
            assert r.stats["t0_path"] == path, f"{self.name}, {label}: reported {r.stats['t0_path']}, pinned {path}"
        for f in ("valid", "cause", "fail_event") + (("peak",) if peak else ()):
            got, want = getattr(r, f), self.orc[f]
            bad = np.flatnonzero(got != want)
            assert not len(bad), (f"{self.name}, {label}: {f} differs on " +
                                  ", ".join(f"{self.b.names[i]} (device {got[i]}, oracle {want[i]})" for i in bad[:6]))

    def exact_ref(self):
        if self.ref is None:
            self.ref = Device(0, path_flags=OFF, max_final=10).check(self.b.pk, peaks=False)
            assert self.ref.stats["t0_path"] == "k_search_lattice"
            self.check("unsegmented, peaks=False", self.ref)
        return self.ref

    def run(self, group):
        """Run the group's paths once; every run is checked against the
        oracle as a whole here and kept for the per-key tests."""
        if group in self.runs:
            return self.runs[group]
        pk, out = self.b.pk, []
        self.runs[group] = out
        if group == "unsegmented":
            r = Device(0, path_flags=OFF).check(pk, verdicts_only=True)
            out.append(("unsegmented, verdicts only", r))
            self.check(out[-1][0], r, "k_search_lattice")
            r = Device(0, path_flags=OFF).check(pk)
            out.append(("unsegmented, peaks", r))
            self.check(out[-1][0], r, "k_search_lattice", peak=True)
            out.append(("unsegmented, peaks=False", self.exact_ref()))
        elif group == "spec":
            for segs in (2, 3, 4, 6, 8):
                for ck in ((32, 160), (1, 2), (0, 0)):
                    r = Device(0, path_flags=N.LC_PATH_SPLIT_OFF, spec_segs=segs, spec_ck=ck).check(pk, verdicts_only=True)
                    out.append((f"k_spec segs {segs} ck {ck}", r))
                    self.check(out[-1][0], r, self.spec_path())
        elif group == "spec_flags":
            for flag, what in ((N.LC_PATH_SPEC_COST, "SPEC_COST"), (N.LC_PATH_EV32, "EV32"),
                               (N.LC_PATH_SPEC_NOPRIO, "SPEC_NOPRIO")):
                r = Device(0, path_flags=N.LC_PATH_SPLIT_OFF | flag, spec_segs=4).check(pk, verdicts_only=True)
                out.append((f"k_spec segs 4 {what}", r))
                self.check(out[-1][0], r, self.spec_path())
        elif group == "exact":
            ref = self.exact_ref()
            for segs, ck in ((2, None), (4, None), (8, None), (4, (1, 2))):
                r = Device(0, path_flags=N.LC_PATH_SPLIT_OFF, spec_segs=segs, spec_ck=ck, max_final=10).check(pk, peaks=False)
                label = f"exact k_spec segs {segs} ck {ck}"
                out.append((label, r))
                self.check(label, r, self.spec_path())
                np.testing.assert_array_equal(r.n_final, ref.n_final, err_msg=f"{self.name}, {label}: n_final")
                bad = [self.b.names[k] for k in range(pk.n_keys)
                       if r.final[k, :r.n_final[k]].tolist() != ref.final[k, :ref.n_final[k]].tolist()]
                assert not bad, f"{self.name}, {label}: final configs differ on {bad[:6]}"
        elif group == "split":
            # k_search_segments takes a taggable register-tier batch of at most 8 keys per CU
            # (step_plan.hpp:82); any other batch must say so in the path it reports
            split = self.taggable and self.t0_only and pk.n_keys <= CU_COUNT * 8
            for seg_len in (0, 64, 1):
                r = Device(0, path_flags=N.LC_PATH_SPLIT_ON, seg_len=seg_len).check(pk, verdicts_only=True)
                out.append((f"SPLIT_ON seg_len {seg_len}", r))
                self.check(out[-1][0], r, "k_search_segments" if split else self.spec_path())
        elif group == "node":
            dev = Device(0)
            rec, _st = dev.check_node(pk, pk.n_keys)
            v, cause, fe = P.unpack_records(rec)
            r = SimpleNamespace(valid=v, cause=cause, fail_event=fe, stats={})
            out.append(("check_node, the library's choice", r))
            self.check(out[-1][0], r)
            r = dev.check(pk, verdicts_only=True)
            out.append(("the library's choice, verdicts only", r))
            self.check(out[-1][0], r)
        return out


@pytest.fixture(scope="module")
def loaded():
    """Batches by name, built once, with their oracle records and device runs."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Loaded(name)
        return cache[name]
    yield get
    cache.clear()


@pytest.mark.parametrize("name,group", [(n, g) for n in sorted(BATCH_GROUPS) for g in BATCH_GROUPS[n]])
def test_paths(loaded, name, group):
    """One batch through one group of register-tier paths: every record
    equals the oracle's, every pinned path is the one reported."""
    L = loaded(name)
    assert L.run(group)
    assert (L.orc["valid"] == 0).any() and (L.orc["valid"] == 1).any()


def test_expected_paths(loaded):
    """Which batches the register tier takes alone and which are taggable, as
    the cases of (e) are built: 32 states stay on k_spec, 33 states (shared or
    one key in two) and one key of 11 pending do not; 5 values are taggable,
    6 are not."""
    want = {"ragged": (True, True), "compact": (True, True), "profiles": (True, True), "anomalies": (True, True),
            "states32": (True, False), "states33": (False, False), "states32_33_mixed": (False, False),
            "width11": (False, True), "values5": (True, True), "values6": (True, False)}
    for name, (t0_only, taggable) in want.items():
        L = loaded(name)
        assert (L.t0_only, L.taggable) == (t0_only, taggable), name


KEYED = [n for n in sorted(E.BATCHES) if n != "compact"]  # (compact: (a)'s keys again, and fillers)


def _case_ids():
    # the names only (plans are cheap; no history is built at collection)
    return [(n, case) for n in KEYED for case, _plan in E.BATCHES[n][0]()]


@pytest.mark.parametrize("name,case", _case_ids(), ids=lambda x: x)
def test_key(loaded, name, case):
    """One named key on every path (the runs are shared with test_paths):
    its record is the oracle's everywhere."""
    L = loaded(name)
    i = L.b.index(case)
    for group in BATCH_GROUPS[name]:
        try:
            runs = L.run(group)
        except AssertionError:
            runs = L.runs[group]  # the whole-batch failure is test_paths'; this key is judged on its own
        assert runs, f"{name}, {group}: nothing ran"
        for label, r in runs:
            got = (int(r.valid[i]), int(r.cause[i]), int(r.fail_event[i]))
            want = (int(L.orc["valid"][i]), int(L.orc["cause"][i]), int(L.orc["fail_event"][i]))
            assert got == want, f"{label}: (valid, cause, fail_event) {got}, oracle {want}"
            if label == "unsegmented, peaks":
                assert int(r.peak[i]) == int(L.orc["peak"][i]), label
