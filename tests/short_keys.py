"""A batch whose keys' event counts straddle k_spec's two length thresholds
(SPEC_MIN_LEN = 128 events: below it a key is one segment; from 256 on it is
cut), for tests/test_gpu_spec_short_keys.py.

lc_synth_generate fixes ops per key, not events (a failed cas packs to no
event, a truncated op to one), so the keys are prefixes of generated keys cut
where the packer's own event -> row map says the wanted event sits, and a
prefix is kept only if it packs to exactly the wanted count."""
import numpy as np

from lincheck import history as H
from lincheck.checker import Packed
from lincheck.history import Tuple

LENGTHS = (0, 1, 2, 127, 128, 129, 255, 256, 257)
EXTRA = (90, 110)  # one-segment keys long enough to hold an anomaly
PER_LENGTH = 12   # keys wanted of each exact length (fewer are accepted, at least 2)
LONG_OPS = 400    # ~600 events
N_LONG = 80
ERROR_KEY = 999_000


def _prefixes(src, pk, want_events):
    """The rows of a history whose key i is src's key i cut after its event
    want_events[i] - 1 (no rows for 0)."""
    keep = np.zeros(len(src), bool)
    pos = {k: i for i, k in enumerate(pk.keys)}
    idx = np.array([pos.get(int(k), -1) for k in src.key])
    for i, n in enumerate(want_events):
        if n == 0:
            continue
        last = pk.event_row(i, n - 1)
        rows = np.flatnonzero(idx == i)
        keep[rows[rows <= last]] = True
    rows = np.flatnonzero(keep)
    return H.History(src.type[rows], src.f[rows], src.process[rows], src.key[rows], src.v0[rows], src.v1[rows],
                     np.arange(rows.size, dtype=np.int64))


def build():
    """(history, {key: wanted events}) -- about 200 keys: prefixes of every
    length in LENGTHS, concurrency-10 keys of ~600 events that reach 9-10 ops
    pending, an anomaly somewhere in every generated short key's source (so in
    many of the prefixes) and in a third of the long keys, and one key the
    packer marks with an error."""
    all_len = LENGTHS + EXTRA
    n_src = len(all_len) * PER_LENGTH * 10
    src = H.synth(n_keys=n_src, ops_per_key=220, concurrency=10, mean_think=0.3, anomaly_rate=1.0, seed=311)
    pk = Packed(src)
    want = [all_len[i % len(all_len)] for i in range(n_src)]
    cut = _prefixes(src, pk, want)
    pc = Packed(cut)
    got = {k: pc.n_events(i) for i, k in enumerate(pc.keys)}
    by_len = {n: [] for n in all_len}
    for i, k in enumerate(pk.keys):
        n = want[i]
        if n and got.get(k) == n and len(by_len[n]) < PER_LENGTH:
            by_len[n].append(k)
    for n in all_len:
        if n:
            assert len(by_len[n]) >= 2, f"only {len(by_len[n])} prefixes pack to {n} events"
    short = cut.select_keys([k for ks in by_len.values() for k in ks])
    # 0 events: keys whose only op failed (Knossos drops the pair)
    zero_keys = [998_000 + i for i in range(3)]
    zero = H.History.from_ops([op for k in zero_keys for op in (
        {"type": "invoke", "f": "cas", "value": Tuple(k, [3, 4]), "process": 0},
        {"type": "fail", "f": "cas", "value": Tuple(k, [3, 4]), "process": 0})])
    # 4 events, not linearizable: a read of a value nobody wrote
    tiny_keys = [997_000 + i for i in range(3)]
    tiny = H.History.from_ops([op for k in tiny_keys for op in (
        {"type": "invoke", "f": "write", "value": Tuple(k, 1), "process": 0},
        {"type": "ok", "f": "write", "value": Tuple(k, 1), "process": 0},
        {"type": "invoke", "f": "read", "value": Tuple(k, None), "process": 1},
        {"type": "ok", "f": "read", "value": Tuple(k, 2), "process": 1})])
    # the packer refuses this one: a completion without an invocation
    err = H.History.from_ops([{"type": "ok", "f": "write", "value": Tuple(ERROR_KEY, 1), "process": 0}])
    long_ = H.synth(n_keys=N_LONG, ops_per_key=LONG_OPS, concurrency=10, mean_think=0.3, anomaly_rate=0.3, seed=312,
                    key_base=500_000)
    lengths = {k: n for n, ks in by_len.items() for k in ks}
    lengths.update({k: 0 for k in zero_keys})
    lengths.update({k: 4 for k in tiny_keys})
    return H.History.concat([short, zero, tiny, err, long_]), lengths
