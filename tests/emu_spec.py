"""Lane-level CPU model of a speculative segment's walk (device_spec.hip
spec_walk, verdict builds), on top of emu_t0's steps: the lane phase on closed
sets, the dense phase (7-10 ops pending) on exact sets (ok_reg,
ok_event_mem) or on closed ones (ok_reg_closed, ok_event_mem_closed), `dirty`
carried as the kernel carries it, and the start of a run at a cut -- from TOP,
or from the set another walk ended with, relabelled to the cut's op indices.

Test infrastructure, as emu_t0 is: it never stands in for the device."""
from __future__ import annotations

import numpy as np

import emu_t0 as E

LANES = E.LANES
OK_BIT = E.OK_BIT


def popc(W) -> int:
    """Configs in one lattice register (the kernel's wave sum of popc(W0))."""
    return int(sum(bin(int(x)).count("1") for x in W))


def ok_dense_closed(W, p, n, ops, dirty):
    """ok_reg_closed / ok_event_mem_closed: close W (RL = 2^(n-6) lane arrays)
    under all n pending ops when dirty; keep the part with bit p, that bit
    moved down; `last` = n - 1 takes index p.  Returns (status, W')."""
    RL, NB, NR = 1 << (n - 6), n, n - 6
    rl = NR - 1
    C = [w.copy() for w in W]
    if dirty:
        vp, vk, sb = E.lane_masks(ops, NB, -1)  # (no op left out)
        rp = [ops.pas[6 + r] for r in range(NR)]
        rk = [ops.keep[6 + r] for r in range(NR)]
        for _s in range(NB):
            nv = [E.sweep_lanes(C[k], vp, vk, sb, NB) for k in range(RL)]
            for r in range(NR):
                for k in range(RL):
                    if (k >> r) & 1:
                        nv[k] = E.xacc(nv[k], nv[k ^ (1 << r)], rp[r], rk[r], sb[6 + r])
            ch = any((nv[k] != C[k]).any() for k in range(RL))
            C = nv
            if not ch:
                break
    last = n - 1
    zero = np.zeros(64, np.uint32)
    Wn = [None] * RL
    for k in range(RL):
        if (k >> rl) & 1:
            Wn[k] = zero.copy()
        elif p == last:
            Wn[k] = C[k | (1 << rl)].copy()
        elif p < 6:
            hp = (LANES >> p) & 1 == 1
            Wn[k] = np.where(hp, C[k | (1 << rl)], E.gup(C[k], p)).astype(np.uint32)
        else:
            r = p - 6
            Wn[k] = (C[k | (1 << rl)] if (k >> r) & 1 else C[k | (1 << r)]).copy()
    if not any(w.any() for w in Wn):
        return 1, C
    return 0, Wn


class State:
    """spec_walk's SpecState: W0, the ops by index, slots, live indices."""

    def __init__(self):
        self.W0 = np.zeros(64, np.uint32)
        self.ops = E.Ops()
        self.slot_v = [0] * 64
        self.dense = [0] * 128
        self.n = 0
        self.live = 0


def pending_at(events, cut):
    """The ops pending at boundary `cut`: {slot: invoke word}, as spec_pending finds them."""
    pend = {}
    for ev in events[:cut]:
        ev = int(ev)
        slot = (ev >> 24) & 0x7F
        if ev & OK_BIT:
            pend.pop(slot, None)
        else:
            pend[slot] = ev
    return pend


def setup(events, trans, cut) -> State:
    """spec_setup: the ops pending at the cut take op indices 0 .. n-1 in slot order."""
    st = State()
    for j, (slot, ev) in enumerate(sorted(pending_at(events, cut).items())):
        st.ops.pas[j], st.ops.keep[j], st.ops.b[j] = E.xfer_of(int(trans[ev & 0xFFFFFF]))
        st.slot_v[j] = slot
        st.dense[slot] = j
        st.n += 1
    st.live = (1 << st.n) - 1
    return st


def start_top(events, trans, cut, nstates) -> State:
    st = setup(events, trans, cut)
    st.W0 = np.where(LANES < (1 << st.n), np.uint32((1 << nstates) - 1), np.uint32(0)).astype(np.uint32)
    return st


def start_from(events, trans, cut, prev: State) -> State:
    """k_spec's relabelling: the set walk `prev` ended with (at `cut`), from
    its op indices to the cut's."""
    st = setup(events, trans, cut)
    assert prev.n == st.n <= 6
    at = {prev.slot_v[q]: q for q in range(6) if (prev.live >> q) & 1}
    src = np.zeros(64, np.int64)
    for j in range(st.n):
        src |= ((LANES >> j) & 1) << at[st.slot_v[j]]
    st.W0 = np.where(LANES < (1 << st.n), prev.W0[src], np.uint32(0)).astype(np.uint32)
    return st


def walk(events, trans, b, e_end, st: State, closed_dense: bool):
    """Events [b, e_end) from st (changed in place).  Returns (status, fev,
    oks): status 0 alive / 1 dead at event fev / 3 does not fit; oks: one
    (event, pending before, W0, back) per successful :ok -- W0 the lane
    lattice after a lane-phase :ok (None in the dense phase); back, for the
    dense :ok that returns to 6 pending, the lattice as it stands and closed
    under the 6 ops (else None)."""
    ops = st.ops
    W = [st.W0] + [np.zeros(64, np.uint32) for _ in range(15)]
    dirty = True
    oks = []
    for j in range(b, e_end):
        ev = int(events[j])
        slot = (ev >> 24) & 0x7F
        n = st.n
        if not ev & OK_BIT:
            if n >= 10 or slot >= 64:
                return 3, j, oks
            idx = (~st.live & -~st.live).bit_length() - 1 if n < 6 else n  # lowest free / dense
            ops.pas[idx], ops.keep[idx], ops.b[idx] = E.xfer_of(int(trans[ev & 0xFFFFFF]))
            st.slot_v[idx] = slot
            st.dense[slot] = idx
            st.live |= 1 << idx
            st.n += 1
            dirty = True
            continue
        p = st.dense[slot]
        if n <= 6:
            r, W0 = E.ok_lane_closed(W[0], p, st.live, ops, dirty)
            dirty = False
            if r:
                return 1, j, oks
            W[0] = st.W0 = W0
            st.live &= ~(1 << p)
            st.n -= 1
            oks.append((j, n, W0.copy(), None))
            continue
        RL = 1 << (n - 6)
        if closed_dense:
            r, Wn = ok_dense_closed(W[:RL], p, n, ops, dirty)
            dirty = False
        else:
            r, Wn = (E.ok_event_mem if n >= 9 else E.ok_event)(W[:RL], p, n, ops)
            dirty = True  # exact sets: closed again at the next lane-phase :ok
        if r:
            return 1, j, oks
        for k in range(RL):
            W[k] = Wn[k]
        last = n - 1
        if p != last:
            s_last = st.slot_v[last]
            ops.pas[p], ops.keep[p], ops.b[p] = ops.pas[last], ops.keep[last], ops.b[last]
            st.slot_v[p] = s_last
            st.dense[s_last] = p
        st.n -= 1
        st.live = (1 << st.n) - 1
        st.W0 = W[0]
        oks.append((j, n, None, (W[0].copy(), close_lane(W[0], st.live, ops)) if st.n == 6 else None))
    return 0, -1, oks


def close_lane(W0, live, ops):
    """W0 closed under the live ops (ok_lane_closed's closure alone)."""
    C = W0
    vp, vk = [], []
    for q in range(6):
        on = ((LANES >> q) & 1 == 1) & bool((live >> q) & 1)
        vp.append(np.where(on, np.uint32(ops.pas[q]), np.uint32(0)).astype(np.uint32))
        vk.append(np.where(on, np.uint32(ops.keep[q]), np.uint32(0)).astype(np.uint32))
    sb = [ops.b[q] for q in range(6)]
    for _s in range(7):
        nv = E.sweep_lanes(C, vp, vk, sb, 6)
        if not (nv != C).any():
            break
        C = nv
    return C
