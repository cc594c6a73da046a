"""The set tiers at their capacity edges (device_search.hip T1 256/512 and T2
1024/4096, device_hbm.hip's LDS pass 2048/4096): keys whose largest |S'| or
|I| is exactly a tier's capacity -- the last array slot written, the hash
table at its designed load -- and keys at most one 64-lane batch past it,
where the `r < CAP` guards are all that keeps the overshoot out of the next
LDS array.  The keys are pinned in tests/edge_keys.py (found by
tests/tools/find_edge_keys.py); every test starts from edge_keys.batch(),
which asserts that each key still is the edge it is listed as.

Every record (verdict, cause, failing event, peak) and the probe total must be
the oracle's, on every way into the search; the tier each class ends in is
asserted from lc_stats, so that a tier that gives keys up early (and so no
longer meets its edge) shows: lc_stats.deep_keys is the number of keys T2
handed to the HBM tier, exactly the keys past T2's capacity (lds_keys counts
every key finished, in whichever tier; T1 -> T2 hand-overs have no counter).

No case puts an exact-fit key and a second key on one wave's tables: T1
launches min(K, 7 x CUs) blocks and T2 one per CU (device_api.hip
run_set_tiers), so that takes more than 1,792 (256) keys that leave the
register tier, and search_key_lds clears both hash tables in full at every
key's start in any case.

What a record comparison cannot see, from reading device_search.hip and
device_hbm.hip: without the `r < CAP_I` / `r < CAP_S` guards the overshoot of
at most 63 entries lands in the tier's own next LDS array (hS after I), and the
loop leaves the key (`nI > CAP_I`: K_SPILL) in the same iteration, before
anything reads it; and the HBM tier's LDS pass one entry past LIM_I (`r >`
for `r >=` in take_pos) only loads its 8192-slot table to 4097.  Neither
changes a record, so neither is claimed as covered here."""
import numpy as np
import pytest

import cref
import edge_keys as EK
import linear_ref as LR
from helpers import encode_finals
from lincheck import _native as N
from lincheck import parallel as P
from lincheck.checker import Device

pytestmark = pytest.mark.gpu

BUDGET = 1 << 20
BEYOND_T2 = ("t2_over_S", "t2_over_I", "hbm_narrow")          # classes the HBM tier searches


class Loaded:
    def __init__(self, cls):
        self.b = EK.batch(cls)
        keys, self.orc = cref.check_history(self.b.hist.as_c(), budget=BUDGET, threads=8)
        assert list(keys) == self.b.pk.keys
        assert (self.orc["cause"] != 2).all(), "a pinned key does not finish at 2^20"

    def same(self, what, valid, cause, fail_event, peak=None):
        for f, got in (("valid", valid), ("cause", cause), ("fail_event", fail_event), ("peak", peak)):
            if got is None:
                continue
            bad = np.flatnonzero(np.asarray(got) != self.orc[f])
            assert not len(bad), (f"{what}: {f} differs on " + "; ".join(
                f"{self.b.describe(i)} (device {got[i]}, oracle {self.orc[f][i]})" for i in bad))


@pytest.fixture(scope="module")
def loaded():
    cache = {}

    def get(cls):
        if cls not in cache:
            cache[cls] = Loaded(cls)
        return cache[cls]
    yield get
    cache.clear()


def paths_of(cls):
    """The default path (the layered HBM tier) and, for the classes that
    reach the HBM tier, LC_PATH_LAYERS_OFF (the config-keyed tier, whose LDS
    pass has the 2048 / 4096 limits)."""
    return (("default", 0),) + ((("LAYERS_OFF", N.LC_PATH_LAYERS_OFF),) if cls in BEYOND_T2 else ())


def tier_of(cls):
    """The tier a class's keys are expected to end in, from their sizes (the
    device reports the T2 -> HBM hand-over only: deep_keys)."""
    return "T1" if cls in ("t1_fit",) else "T2" if cls in ("t1_over_S", "t1_over_I", "t2_fit") else "HBM"


@pytest.mark.parametrize("cls", EK.CLASSES)
def test_records_probes_and_routing(loaded, cls):
    """lc_check_batch with peaks and probe counts: the oracle's records and
    probe total; the HBM tier searches exactly the keys past T2."""
    L = loaded(cls)
    pk = L.b.pk
    n_deep = pk.n_keys if cls in BEYOND_T2 else 0
    for i in range(pk.n_keys):
        print(f"{L.b.describe(i)}; expected to end in {tier_of(cls)}")
    for what, flags in paths_of(cls):
        r = Device(0, budget=BUDGET, count_probes=True, path_flags=flags).check(pk)
        print(f"{cls}, {what}: keys finished {r.stats['keys_done']}, deep_keys {r.stats['deep_keys']}, "
              f"probes {r.stats['probes']}")
        L.same(f"{cls}, {what}", r.valid, r.cause, r.fail_event, r.peak)
        assert r.stats["probes"] == int(L.orc["probes"].sum())
        # |S'| == CAP_S and |I| == CAP_I stay in the tier; one entry more leaves it.  (lc_stats.lds_keys
        # counts the keys finished in any tier; deep_keys the keys handed past T2.)
        assert r.stats["deep_keys"] == n_deep, f"{cls}: {r.stats['deep_keys']} keys reached the HBM tier, {n_deep} are past T2"
        assert r.stats["keys_done"] == pk.n_keys


PY_ORACLE_MAX_NEED = 5000  # linear_ref.py enumerates the final configs of keys up to this size in well under a second


@pytest.mark.parametrize("cls", [c for c in EK.CLASSES if any(r[2] == c and r[6] == 0 for r in EK.TABLE)])
def test_final_configs_of_invalid_keys(loaded, cls):
    """Invalid keys (of the classes the search found one for): the final
    configs returned are configs of the set standing before the failing :ok as
    linear_ref.py enumerates it -- all of it when it has fewer than max_final
    = 10 configs, 10 of it otherwise -- on every path of the class.  The one
    invalid key too large for the Python restatement (hbm_narrow, max |I|
    28,576) is compared between the layered and the config-keyed tier instead,
    as test_gpu_layers.test_layers_final_configs does."""
    L = loaded(cls)
    bad = np.flatnonzero(L.orc["valid"] == 0)
    assert len(bad)
    pk = L.b.pk
    ops = L.b.hist.to_ops()
    runs = {what: Device(0, budget=BUDGET, path_flags=flags).check(pk) for what, flags in paths_of(cls)}
    for what, r in runs.items():
        L.same(f"{cls}, {what}", r.valid, r.cause, r.fail_event, r.peak)
    for i in bad:
        if L.b.need[i] <= PY_ORACLE_MAX_NEED:
            a = LR.analysis(LR.subhistory(ops, int(pk.keys[i])))
            assert a.valid is False and a.fail_event == L.orc["fail_event"][i]
            fin, n = encode_finals(pk, int(i), a, "cas-register", limit=len(a.final_configs))
            want = {tuple(x) for x in fin[:n].tolist()}
            for what, r in runs.items():
                got = [tuple(x) for x in r.final[i][:int(r.n_final[i])].tolist()]
                print(f"{L.b.describe(i)}, {what}: {len(got)} of {len(want)} final configs")
                assert len(got) == min(len(want), 10) == len(set(got)), (what, L.b.describe(i))
                assert set(got) <= want, (what, L.b.describe(i))
        else:
            assert len(runs) == 2, L.b.describe(i)
            ra, rb = runs.values()
            na, nb = int(ra.n_final[i]), int(rb.n_final[i])
            assert na == nb and na > 0, L.b.describe(i)
            if na < 10:  # the whole set
                assert {tuple(x) for x in ra.final[i][:na].tolist()} == {tuple(x) for x in rb.final[i][:nb].tolist()}


@pytest.mark.parametrize("cls", EK.CLASSES)
def test_other_entries(loaded, cls):
    """verdicts_only, and a resident batch's node step: the same records."""
    L = loaded(cls)
    pk = L.b.pk
    for what, flags in paths_of(cls):
        r = Device(0, budget=BUDGET, path_flags=flags).check(pk, verdicts_only=True)
        L.same(f"{cls}, {what}, verdicts_only", r.valid, r.cause, r.fail_event)
        dev = Device(0, budget=BUDGET, path_flags=flags)
        db = dev.upload(pk)
        db.check_node(pk.n_keys)
        v, cause, fe = P.unpack_records(dev.node_records(pk.n_keys).astype(np.int64))
        L.same(f"{cls}, {what}, upload / check_node", v, cause, fe)
        rec, _st = dev.check_node(pk, pk.n_keys)
        v, cause, fe = P.unpack_records(rec.astype(np.int64))
        L.same(f"{cls}, {what}, check_node", v, cause, fe)
