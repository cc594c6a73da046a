"""Helpers of the streaming set-full tests (lc_setfull_stream_*).

Emu is a small numpy restatement of what the device does with a chunk of the
packer -- reset, mark, fold, finish over resident per-slot records -- so the
CPU suite can hold the packer's chunks against the fold of
tests/setfull_helpers.py after every append without a GPU.  It is written from
the record's definition (include/lincheck_setfull_stream.h and lincheck.h's
set-full rules), row by row, not from the kernels.

check_prefix compares one stream's state with the fold of the prefix, key by
key, error keys included; slices() cuts a history into appends."""
import numpy as np

import setfull_helpers as H
from lincheck import _native as N
from lincheck.setfull import OUTCOMES, PackedSetFull, SetFullHistory
from set_helpers import keys_of

NONE = N.LC_SETFULL_NONE
FIELDS = ("inv", "ack", "ack_t", "kn", "kn_t", "lp", "lp_t", "la", "la_t", "ms")


def slices(ops, step):
    """The history in appends of `step` rows (0: all at once)."""
    if not step:
        return [ops]
    return [ops[i:i + step] for i in range(0, len(ops), step)]


class Emu:
    """The device half in numpy: records by slot, a chunk at a time."""

    def __init__(self, linearizable=False):
        self.lin = linearizable
        self.rec = {f: np.full(0, NONE, np.int64) for f in FIELDS}
        self.outcome = np.zeros(0, np.uint8)
        self.dup = np.zeros(0, np.uint8)
        self.valid, self.counts = {}, {}   # by key index
        self.slots = {}                    # key index -> slot of every id

    def _grow(self, n):
        have = len(self.outcome)
        if n <= have:
            return
        for f in FIELDS:
            self.rec[f] = np.concatenate([self.rec[f], np.full(n - have, NONE, np.int64)])
        self.outcome = np.concatenate([self.outcome, np.zeros(n - have, np.uint8)])
        self.dup = np.concatenate([self.dup, np.zeros(n - have, np.uint8)])

    def apply(self, c):
        """Fold one chunk (SetFullStream.chunk()); returns the touched keys."""
        T = len(c["tk_key"])
        if len(c["blk"]):
            self._grow(256 * (int(c["blk"].max()) + 1))
        rec = self.rec
        slot_of = []
        for t in range(T):
            blocks = c["blk"][int(c["tk_blk_off"][t]):int(c["tk_blk_off"][t + 1])].astype(np.int64)
            n = int(c["tk_n_ids"][t])
            assert len(blocks) == (n + 255) // 256, "a key owns whole blocks of 256 ids, no more than it needs"
            ids = np.arange(n)
            slot_of.append(blocks[ids // 256] * 256 + ids % 256 if n else np.zeros(0, np.int64))
        # reset
        seen = set()
        for e in range(len(c["en_t"])):
            t, i, fl = int(c["en_t"][e]), int(c["en_id"][e]), int(c["en_flags"][e])
            assert (t, i) not in seen, "one entry per touched id"
            seen.add((t, i))
            s = slot_of[t][i]
            if fl & N.LC_SFS_FRESH:
                for f in FIELDS[:-1]:
                    rec[f][s] = NONE
                rec["inv"][s] = c["en_inv_pos"][e]
            if fl & N.LC_SFS_ACK:
                assert rec["ack"][s] == NONE and rec["inv"][s] >= 0 and c["en_ack_pos"][e] > rec["inv"][s]
                rec["ack"][s], rec["ack_t"][s] = c["en_ack_pos"][e], c["en_ack_time"][e]
        for t in range(T):
            sl = slot_of[t]
            n = len(sl)
            r0, r1 = int(c["tk_row_off"][t]), int(c["tk_row_off"][t + 1])
            inv = rec["inv"][sl]
            tracked = inv >= 0
            kn, kn_t = rec["kn"][sl].copy(), rec["kn_t"][sl].copy()
            use_ack = tracked & (rec["ack"][sl] >= 0) & ((kn < 0) | (rec["ack"][sl] < kn))
            kn[use_ack], kn_t[use_ack] = rec["ack"][sl][use_ack], rec["ack_t"][sl][use_ack]
            lp, lp_t, la, la_t = (rec[f][sl].copy() for f in ("lp", "lp_t", "la", "la_t"))
            for r in range(r0, r1):
                ids = c["read_id"][int(c["el_off"][r]):int(c["el_off"][r + 1])].astype(np.int64)
                assert (ids < n).all()
                # mark: a bit already set when the same row marks it again is a duplicate
                uniq, cnt = np.unique(ids, return_counts=True)
                self.dup[sl[uniq[cnt > 1]]] = 1
                held = np.zeros(n, bool)
                held[uniq] = True
                # fold: only rows that completed after the element's invocation
                pos, tm, ipos, itm = (int(c[f][r]) for f in ("row_pos", "row_time", "row_inv_pos", "row_inv_time"))
                el = tracked & (pos > inv)
                p = el & held & (ipos > lp)
                lp[p], lp_t[p] = ipos, itm
                k = el & held & ((kn < 0) | (pos < kn))
                kn[k], kn_t[k] = pos, tm
                a = el & ~held & (ipos > la)
                la[a], la_t[a] = ipos, itm
            for f, v in (("kn", kn), ("kn_t", kn_t), ("lp", lp), ("lp_t", lp_t), ("la", la), ("la_t", la_t)):
                rec[f][sl[tracked]] = v[tracked]
            stable = tracked & (lp >= 0) & (la < lp)
            lost = tracked & ~stable & (kn >= 0) & (la >= 0) & (lp < la) & (kn < la)
            until = np.where(stable, np.where(la >= 0, la_t + 1, 0), np.where(lp >= 0, lp_t + 1, 0))
            ms = np.where(stable | lost, np.maximum(0, until - kn_t) // 10 ** 6, NONE)
            rec["ms"][sl] = ms
            self.outcome[sl] = np.where(~tracked, N.LC_SETFULL_UNTRACKED, np.where(stable, N.LC_SETFULL_STABLE, np.where(
                lost, N.LC_SETFULL_LOST, N.LC_SETFULL_NEVER_READ)))
            # finish
            counts = [int(tracked.sum()), int(stable.sum()), int(lost.sum()), int((tracked & ~stable & ~lost).sum()),
                      int((stable & (ms > 0)).sum()), int(self.dup[sl].sum())]
            v = N.LC_INVALID if counts[2] else N.LC_UNKNOWN if not counts[1] else \
                N.LC_INVALID if self.lin and counts[4] else N.LC_VALID
            if counts[5]:
                v = N.LC_INVALID
            ki = int(c["tk_key"][t])
            self.valid[ki], self.counts[ki], self.slots[ki] = v, counts, sl
        return [int(k) for k in c["tk_key"]]

    def per_element(self, ki, elems):
        """{element: (outcome, latency, known, last-absent)} of key ki's tracked ids, and its duplicated elements."""
        sl = self.slots.get(ki, np.zeros(0, np.int64))
        assert len(sl) == len(elems)
        per = {int(e): (OUTCOMES[int(self.outcome[s])], int(self.rec["ms"][s]), int(self.rec["kn"][s]), int(self.rec["la"][s]))
               for e, s in zip(elems, sl) if self.outcome[s] != N.LC_SETFULL_UNTRACKED}
        return per, {int(e) for e, s in zip(elems, sl) if self.dup[s]}


def stream_per_element(res, i):
    """The same from a device stream's StreamResults."""
    b, e = int(res.id_off[i]), int(res.id_off[i + 1])
    per = {int(res.elems[x]): (OUTCOMES[int(res.outcome[x])], int(res.latency[x]), int(res.known[x]), int(res.last_absent[x]))
           for x in range(b, e) if res.outcome[x] != N.LC_SETFULL_UNTRACKED}
    dups = {int(res.elems[x]): int(res.multiplicity[x]) for x in range(b, e) if res.duplicated[x]}
    return per, dups


def want_counts(r):
    return [r[k] for k in ("attempt-count", "stable-count", "lost-count", "never-read-count", "stale-count", "duplicated-count")]


def valid_code(v):
    return N.LC_VALID if v is True else N.LC_INVALID if v is False else N.LC_UNKNOWN


def check_prefix(stream, prefix, lin, per_of, valid, counts):
    """The stream's state against the fold of `prefix` for EVERY key.
    per_of(i) -> ({element: tuple}, {element: multiplicity}); valid / counts by key index."""
    want = H.restate_independent(prefix, lin)
    keys = stream.keys()
    if not keys:  # no client row yet: the fold's single key has nothing in it either
        assert list(want) == [None] and want[None][0].get("attempt-count") == 0 and not want[None][0]["duplicated"]
        return want
    assert keys == (keys_of(prefix) or [None])
    assert keys == list(want)
    packed = PackedSetFull(SetFullHistory.from_ops(prefix))  # the one-shot packer: the error texts
    for i, k in enumerate(keys):
        r, per = want[k]
        if "error" in r:
            assert stream.key_error(i) and stream.key_error(i) == packed.key_error(i), (k, r)
            assert len(stream.ids(i)) == 0
            if valid is not None:
                assert valid[i] == N.LC_UNKNOWN and list(counts[i]) == [0] * 6, k
            continue
        assert stream.key_error(i) is None, (k, stream.key_error(i))
        got, dups = per_of(i)
        assert got == per, (k, got, per)
        assert dups == r["duplicated"], (k, dups, r["duplicated"])
        assert valid[i] == valid_code(r["valid?"]), (k, valid[i], r["valid?"])
        assert [int(x) for x in counts[i]] == want_counts(r), (k, counts[i], r)
    return want
