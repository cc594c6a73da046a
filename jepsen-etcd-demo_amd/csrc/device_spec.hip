// device_spec.hip -- speculative key segments: k_spec (one workgroup per key,
// one wave per segment) and k_spec_rerun.

#include "lattice_core.hpp"
#include "lattice_validate.hpp"

namespace lcd {

// ---- Speculative key segments -----------------------------------------------
//
// The other way to cut a serial key (no quiescent point needed).  The search
// is monotone: from a larger config set every later set is at least as large.
// So segment s of a key (s >= 1, cut where at most 6 ops are pending) is
// searched from TOP = every register state with every subset of the ops
// pending at the cut linearized -- a superset of the real set there, whatever
// came before.  Runs from different start sets through the same events meet
// quickly (a completed write collapses the register; measured on C2-shaped
// keys with tools/spec_conv.py: within 8 events at the median, 25 at most),
// and once two runs hold equal sets they stay equal.  One workgroup per key,
// one wave per segment:
//   1. every wave searches its segment from TOP (segment 0 from the initial
//      state, exactly), recording the set after the first :ok past cut + ck1
//      and past cut + ck2 (checkpoints), its failing event if it dies, and its
//      set at the segment's end;
//   2. every wave s >= 1 then searches its segment again from the set segment
//      s - 1 ended with, until the two runs meet: at one of the first :oks,
//      by set size alone (the TOP run's set contains the other's, so equal
//      config counts are equal sets: spec_meet_word), else at a checkpoint.
//      Inductively every set is then exact: where they meet, the TOP run IS
//      the real run from there on, so its death (or survival) is the
//      segment's;
//   3. wave 0 walks the segments in order: the key fails in the first
//      segment whose real run dies.  A pair of runs that never met (not seen
//      on any measured history) sends the key to the unsegmented search.
// Compared sets are the closed sets the FAST path keeps, taken right after an
// :ok, where they are canonical (ok_lane_closed); both runs of a segment start
// from the same op-index assignment (slot order at the cut), so the
// assignments stay equal event by event.  Verdicts only.

constexpr uint32_t SPEC_NONE = 0xFFFFFFFFu;
constexpr uint32_t SPEC_MIN_LEN = 128;  // events per segment at least
constexpr uint32_t SPEC_MAX_PEND = 6;   // ops pending at a cut at most (the lane phase)

// Ops invoked minus ops completed over events [b, e) of a key (the change in
// the pending count across them): one ballot pair per 64 events, 8 chunks'
// loads in flight.
template <class EvT>
__device__ __forceinline__ int32_t spec_net(EvT evp, uint32_t b, uint32_t e) {
    constexpr uint32_t G = 8;
    const uint32_t lane = lane_id();
    int32_t cnt = 0;
    for (uint32_t gb = b; gb < e; gb += 64 * G) {
        uint32_t wg[G];
#pragma unroll
        for (uint32_t g = 0; g < G; ++g) {
            const uint32_t j = gb + 64 * g + lane;
            wg[g] = j < e ? evp[j] : 0u;
        }
#pragma unroll
        for (uint32_t g = 0; g < G; ++g) {
            const uint32_t base = gb + 64 * g;
            if (base >= e) continue;
            const bool in = base + lane < e;
            cnt += __popcll(__ballot(in && !(wg[g] >> 31))) - __popcll(__ballot(in && (wg[g] >> 31)));
        }
    }
    return cnt;
}

// Estimated cost of an event, in 1/8 of a lane-phase event: the per-event fit
// of DESIGN.md section 3 (707 cycles per event, +171 per :ok with 7-8 ops
// pending, ~21k per :ok with 9-10 pending -- the last in the LDS workspace).
constexpr uint32_t SPEC_W_EV = 8, SPEC_W_MID = 2, SPEC_W_HEAVY = 240;

// One 64-event chunk's classes (w: lane i holds event base + i; cnt: ops
// pending before the chunk): the lanes that are events, :oks with 7-8 and
// with 9-10 ops pending, each lane's pending count before its event, and the
// chunk's cost.  Pending counts come from two ballots and mbcnt (no scan).
struct ChunkCost {
    uint64_t in, inv, oks, mid, heavy;
    int32_t pend;   // per lane: ops pending before the lane's event
    uint32_t cost;  // the chunk's, uniform
};
__device__ __forceinline__ ChunkCost chunk_cost(uint32_t w, uint32_t base, uint32_t nev, int32_t cnt) {
    const uint32_t lane = lane_id();
    ChunkCost c;
    const bool in = base + lane < nev;
    const bool ok = in && (w >> 31);
    c.in = __ballot(in);
    c.inv = __ballot(in && !ok);
    c.oks = __ballot(ok);
    c.pend = cnt + (int32_t)rank_of(c.inv) - (int32_t)rank_of(c.oks);
    c.mid = __ballot(ok && c.pend >= 7 && c.pend <= 8);
    c.heavy = __ballot(ok && c.pend >= 9);
    c.cost = SPEC_W_EV * (uint32_t)__popcll(c.in) + SPEC_W_MID * (uint32_t)__popcll(c.mid) +
             SPEC_W_HEAVY * (uint32_t)__popcll(c.heavy);
    return c;
}

// Segment boundaries at equal estimated cost: target s (1 .. eff-1) at
// s/eff of the key's total cost (chunk_cost), lane s of pos_v, with the ops
// pending there in lane s of pend_v.  Two passes of ballots over the key's
// events (the total, then the targets), 8 chunks' loads in flight.  A
// segment's walk time is its events plus its 9-10-pending :oks (~30 events'
// time each, 2-5 of them in the slowest walks): equal event counts left the
// slowest of C2's 4,000 walks at 1.65x the median.
template <class EvT>
__device__ __forceinline__ void spec_targets_cost(EvT evp, uint32_t nev, uint32_t eff, uint32_t &pos_v,
                                                  int32_t &pend_v) {
    constexpr uint32_t G = 8;
    const uint32_t lane = lane_id();
    uint32_t total = 0;
    int32_t cnt = 0;
    for (uint32_t gb = 0; gb < nev; gb += 64 * G) {
        uint32_t wg[G];
#pragma unroll
        for (uint32_t g = 0; g < G; ++g) {
            const uint32_t j = gb + 64 * g + lane;
            wg[g] = j < nev ? evp[j] : 0u;
        }
#pragma unroll
        for (uint32_t g = 0; g < G; ++g) {
            const uint32_t base = gb + 64 * g;
            if (base >= nev) continue;
            const ChunkCost c = chunk_cost(wg[g], base, nev, cnt);
            total += c.cost;
            cnt += __popcll(c.inv) - __popcll(c.oks);
        }
    }
    pos_v = 0;
    pend_v = 0;
    uint32_t next = 1, acc = 0;
    uint32_t t_next = (uint32_t)((uint64_t)total / eff);
    cnt = 0;
    for (uint32_t gb = 0; gb < nev && next < eff; gb += 64 * G) {
        uint32_t wg[G];
#pragma unroll
        for (uint32_t g = 0; g < G; ++g) {
            const uint32_t j = gb + 64 * g + lane;
            wg[g] = j < nev ? evp[j] : 0u;
        }
#pragma unroll
        for (uint32_t g = 0; g < G; ++g) {
            const uint32_t base = gb + 64 * g;
            if (base >= nev || next >= eff) continue;
            const ChunkCost c = chunk_cost(wg[g], base, nev, cnt);
            if (acc + c.cost >= t_next) {
                // each lane's cost up to and including its event
                const uint64_t me = 1ull << lane;
                const uint32_t incl = SPEC_W_EV * (rank_of(c.in) + 1u) +
                                      SPEC_W_MID * (rank_of(c.mid) + ((c.mid & me) ? 1u : 0u)) +
                                      SPEC_W_HEAVY * (rank_of(c.heavy) + ((c.heavy & me) ? 1u : 0u));
                const bool in = (c.in & me) != 0;
                while (next < eff && acc + c.cost >= t_next) {
                    const uint64_t hit = __ballot(in && acc + incl >= t_next);
                    const uint32_t l = (uint32_t)__builtin_ctzll(hit);
                    const int32_t at = __builtin_amdgcn_readlane(c.pend, l);
                    pos_v = lane == next ? base + l : pos_v;
                    pend_v = lane == next ? at : pend_v;
                    ++next;
                    t_next = (uint32_t)((uint64_t)total * next / eff);
                }
            }
            acc += c.cost;
            cnt += __popcll(c.inv) - __popcll(c.oks);
        }
    }
}

// The cut for target position t (c_t ops pending there): of the boundaries t
// .. t + 64 (t + i = before event t + i), the one with the fewest ops pending,
// the earliest of those, if that is at most SPEC_MAX_PEND and it lies inside
// the key; else SPEC_NONE.  n_at: ops pending at the cut.
// w: lane i holds event t + i (0 past the key).
__device__ __forceinline__ uint32_t spec_cut_at(uint32_t w, uint32_t nev, uint32_t t, int32_t c_t, uint32_t &n_at) {
    const uint32_t lane = lane_id();
    const uint32_t j = t + lane;  // event j; boundary j + 1 after it
    const int32_t d = j < nev ? 1 - 2 * (int32_t)(w >> 31) : 0;
    const int32_t cnt = c_t + wave_scan(d);
    uint32_t key = (j + 1u < nev && cnt >= 0 && cnt <= (int32_t)SPEC_MAX_PEND) ? ((uint32_t)cnt << 7) | (lane + 1u)
                                                                               : ~0u;
    if (lane == 0 && t < nev && c_t >= 0 && c_t <= (int32_t)SPEC_MAX_PEND) key = min(key, (uint32_t)c_t << 7);
    const uint32_t best = uni(__ockl_wfred_min_u32(key));
    if (best == ~0u) return SPEC_NONE;
    n_at = best >> 7;
    return t + (best & 127u);
}

// The ops pending at boundary c (n expected, n <= 6): each slot is decided by
// its last event before c, walking back.  Returns their :invoke words in slot
// order, word j in lane j; found = how many.
template <class EvT>
__device__ __forceinline__ uint32_t spec_pending(EvT evp, uint32_t c, uint32_t n, uint32_t &found) {
    const uint32_t lane = lane_id();
    uint64_t seen = 0, pm = 0;
    uint32_t byslot = 0;
    found = 0;
    n = min(n, SPEC_MAX_PEND);
    for (uint32_t j = c; found < n && j > 0;) {
        const uint32_t base = j > 64u ? j - 64u : 0u, cnt = j - base;
        const uint32_t w = lane < cnt ? evp[base + lane] : 0u;
        for (int32_t i = (int32_t)cnt - 1; i >= 0 && found < n; --i) {
            const uint32_t wi = __builtin_amdgcn_readlane(w, i);
            const uint32_t sl = LC_EV_SLOT(wi) & 63u;
            if (!((seen >> sl) & 1ull)) {
                seen |= 1ull << sl;
                if (!(wi & LC_EV_OK_BIT)) {
                    pm |= 1ull << sl;
                    byslot = lane == sl ? wi : byslot;
                    ++found;
                }
            }
        }
        j = base;
    }
    uint32_t words = 0;
    for (uint32_t k = 0; k < found; ++k) {
        const uint32_t sl = (uint32_t)__builtin_ctzll(pm);
        pm &= pm - 1;
        const uint32_t wi = __builtin_amdgcn_readlane(byslot, sl);
        words = lane == k ? wi : words;
    }
    return words;
}

// Register-tier state of a walk (the lane phase's registers).
struct SpecState {
    uint32_t W0, k_v, cap_v, b_v, slot_v, dense_v, n, live;
};

// The ops pending at a cut (words in lanes 0 .. n-1, slot order) take op
// indices 0 .. n-1.
__device__ __forceinline__ void spec_setup(SpecState &st, uint32_t words, uint32_t n, const uint32_t *trp,
                                           uint32_t ntr) {
    const uint32_t lane = lane_id();
    const bool me = lane < n;
    const uint32_t t = LC_EV_TRANS(words);
    const Xfer x = xfer_of((me && t < ntr) ? trp[t] : 0u);
    st.k_v = me ? x.k : 0u;
    st.cap_v = me ? x.cap : 0u;
    st.b_v = me ? x.b : 0u;
    st.slot_v = me ? (LC_EV_SLOT(words) & 63u) : 0u;
    st.dense_v = 0;
    for (uint32_t j = 0; j < n; ++j) {
        const uint32_t sl = __builtin_amdgcn_readlane(st.slot_v, j);
        st.dense_v = lane == sl ? j : st.dense_v;
    }
    st.n = n;
    st.live = (1u << n) - 1u;
}

// Events [b, e_end) of a key from st, on the compact lattice with closed sets
// (the register tier's FAST path).  MODE 0 (TOP run): records the set after
// the first lane-phase :ok at or past b + ck1 and past b + ck2 into ck_w /
// ck_e.  MODE 1 (verifying run): compares with them at those events.
// `meet` (verdict builds, may be null): the segment's meeting entries, which
// MODE 0 publishes and MODE 1 compares with before the first checkpoint.
// Returns 0 alive at e_end (st: the walk's state there; st.W0 the lattice if
// st.n <= 6), 1 dead at fev, 3 the key does not fit the register tier,
// 4 (MODE 1) met the TOP run, 5 (MODE 1) passed both checkpoints unmet.
// The 9-10-pending workspace: one of the workgroup's NWS LDS slots while one
// is free (busy flags in LDS), else the wave's global slot (an :ok there costs
// ~40k cycles against ~2k in LDS).  NWS = 1, 2, 3 slots for 2, 4, 8 waves
// keep 4 waves per SIMD within the CU's LDS; the 8-wave build held to 8
// waves per SIMD (LC_SPEC8_WAVES) has 2, so that 4 of its workgroups fit.
#ifndef LC_SPEC8_NWS
#define LC_SPEC8_NWS (LC_SPEC8_WAVES >= 8 ? 2 : 3)
#endif
// The 2-wave build keeps no LDS workspace (its 9-10-pending :oks use the
// waves' global ones): 12 KB of LDS per workgroup held it to 5.5 waves per
// SIMD, and the occupancy is worth more to the many-key batches it runs
// than the rare 9-10-pending :ok (LC_SPEC2_WAVES below).
#ifndef LC_SPEC2_NWS
#define LC_SPEC2_NWS 0
#endif
template <int S>
constexpr int spec_lds_ws() { return S <= 2 ? LC_SPEC2_NWS : S <= 3 ? 1 : S <= 6 ? 2 : LC_SPEC8_NWS; }
// Issue priority of a TOP walk by progress (MODE 0, prio): the SIMD's
// arbiter favours the higher s_setprio, then the older wave, so with age
// alone the last-dispatched blocks' walks trail by up to a quarter of a walk
// and end running alone on their SIMDs.  A walk in its first quarter runs at
// priority 3, its last quarter at 0: the four walks a SIMD holds advance
// together and keep it busy to the end.
#ifndef LC_SPEC_PRIO_TOP
#define LC_SPEC_PRIO_TOP 3
#endif
__device__ __forceinline__ void spec_prio(uint32_t quarter) {
    const int lv = LC_SPEC_PRIO_TOP - (int)quarter;
    if (lv >= 3) __builtin_amdgcn_s_setprio(3);
    else if (lv == 2) __builtin_amdgcn_s_setprio(2);
    else if (lv == 1) __builtin_amdgcn_s_setprio(1);
    else __builtin_amdgcn_s_setprio(0);
}

// Words of a run's saved set (EX): T0_RMEM lattice rows, the slot of each op
// index (one row), the live op indices.
constexpr uint32_t SPEC_SAVE_WORDS = (T0_RMEM + 2) * 64;

// EX: Knossos's exact sets (ok_lane) instead of closed ones in the lane
// phase, for steps that report final configs; `save` (EX, may be null)
// receives the run's set at its end or before its failing :ok, in the
// LatMem row layout write_final_mem reads, with its slots and live indices.
// Checkpoints of a TOP run: at ck1, ck2 and evenly between (a verifying run
// compares its set at each and stops at the first match; one that passes
// them all unmet sends the key to the unsegmented search).  A third one
// between measured no faster in round 5 (C2 0.2472 ms with two, 0.2492
// with three; A/B: make variant VFLAGS=-DLC_SPEC_NCK=n).
#ifndef LC_SPEC_NCK
#define LC_SPEC_NCK 2
#endif
constexpr uint32_t SPEC_NCK = LC_SPEC_NCK;
// With three (a diagnostic build): an early one at ck1 / 4 before them
// (LC_SPEC_CK_EARLY), where most pairs of runs have already met; one that
// has not goes on to ck1 and ck2 as with two.  Measured in round 6
// (profiles/r06_segments_seeds.txt): (8, 32, 120) no faster than (32, 120) on
// C2 or C5.
#ifndef LC_SPEC_CK_EARLY
#define LC_SPEC_CK_EARLY 1
#endif
__device__ __forceinline__ uint32_t spec_ck_target(uint32_t i, uint32_t ck1, uint32_t ck2) {
    if (LC_SPEC_CK_EARLY && SPEC_NCK == 3) return i == 0 ? max(ck1 / 4u, 4u) : i == 1 ? ck1 : ck2;
    return i == 0 ? ck1 : i + 1 >= SPEC_NCK ? ck2 : ck1 + (ck2 - ck1) * i / (SPEC_NCK - 1);
}
// Flags between the waves of one k_spec workgroup (LDS, workgroup scope).  A
// wave publishes after its stores (a release fence for the whole wave, then
// lane 0's store); a waiter polls with an acquire load and sleeps between
// polls, a fixed trip count over a uniform value (k_spec's INVARIANT
// below).  The wait is bounded: a waiter that gives up takes the exact path
// (the key is searched unsegmented), so a timeout costs time, never a result.
constexpr uint32_t SPEC_WAIT_MAX = 1u << 22;
__device__ __forceinline__ void spec_publish(int32_t *f, int32_t v = 1) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    if (lane_id() == 0) __hip_atomic_store(f, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ int32_t spec_load(const int32_t *f) {
    return uni(__hip_atomic_load(f, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP));
}
__device__ __forceinline__ bool spec_wait(const int32_t *f) {
#pragma unroll 1
    for (uint32_t it = 0; it < SPEC_WAIT_MAX; ++it) {
        if (spec_load(f) != 0) return true;
        __builtin_amdgcn_s_sleep(2);
    }
    return false;
}
// A verifying run's checkpoint event i (relative to nothing: the event
// index), read while the TOP run it compares with may still be walking:
// waits until that run has recorded it or has ended
// without it (-1: no such checkpoint); -1 on a timeout too.
__device__ __forceinline__ int32_t spec_ck_event(const int32_t *ck_e, uint32_t i, const int32_t *top_done) {
    if (!top_done) return uni(ck_e[i]);
#pragma unroll 1
    for (uint32_t it = 0; it < SPEC_WAIT_MAX; ++it) {
        const int32_t e = spec_load(ck_e + i);
        if (e >= 0) return e;
        if (spec_load(top_done) != 0) return spec_load(ck_e + i);
        __builtin_amdgcn_s_sleep(2);
    }
    return -1;
}

// Meeting by set size (verdict builds).  Both runs of a segment use the same
// op-index assignment and the TOP run starts from a superset, so after every
// lane-phase :ok its closed set contains the verifying run's bit by bit, and
// the two are equal exactly when their config counts are (DESIGN.md,
// "Speculative key segments").  The TOP run publishes, for each of its first
// SPEC_MEET_N successful :oks before its first checkpoint, one word: the :ok's
// ordinal in the segment << 16 | the wave sum of popc(W0) (at most 2,048), or
// SPEC_MEET_NOCMP for an :ok taken in the dense phase (so ordinals stay
// aligned).  The verifying run computes the same word and has met the TOP run
// where they are equal.  Past the ring, or where the TOP run ended without
// the entry or the wait gave up, it goes on to the checkpoints.
// A/B: make variant VFLAGS=-DLC_SPEC_MEET=0.
#ifndef LC_SPEC_MEET
#define LC_SPEC_MEET 1
#endif
// Closed sets at 7-10 ops pending as in the lane phase (ok_reg_closed,
// ok_event_mem_closed), `dirty` carried across the phase switches.
// A/B: make variant VFLAGS=-DLC_SPEC_CLOSED=0.
#ifndef LC_SPEC_CLOSED
#define LC_SPEC_CLOSED 1
#endif
constexpr uint32_t SPEC_MEET_N = 16;  // ck1 = 32 events hold about 16 :oks
constexpr uint32_t SPEC_MEET_NOCMP = 0xFFFFu;
__device__ __forceinline__ int32_t spec_meet_word(uint32_t ord, uint32_t W0) {
    const uint32_t cnt = (uint32_t)__builtin_amdgcn_readlane(wave_scan((int32_t)__popc(W0)), 63);
    return (int32_t)((ord << 16) | cnt);
}
// The TOP run's meeting entry i, as spec_ck_event waits for a checkpoint:
// until that run has published it or has ended without it (-1; -1 on a
// timeout too).
__device__ __forceinline__ int32_t spec_meet_entry(const int32_t *mt, uint32_t i, const int32_t *top_done) {
#pragma unroll 1
    for (uint32_t it = 0; it < SPEC_WAIT_MAX; ++it) {
        const int32_t v = spec_load(mt + i);
        if (v >= 0) return v;
        if (spec_load(top_done) != 0) return spec_load(mt + i);
        __builtin_amdgcn_s_sleep(2);
    }
    return -1;
}

template <int MODE, int NWS, class EvT, bool EX = false>
__device__ __forceinline__ int spec_walk(EvT evp, const uint32_t *trp, uint32_t ntr, uint32_t b,
                                         uint32_t e_end, SpecState &st, uint32_t *ws, uint32_t *lds_ws,
                                         int32_t *lds_busy, uint32_t (*ck_w)[64], int32_t *ck_e, uint32_t ck1,
                                         uint32_t ck2, uint32_t &fev_out, bool prio = false,
                                         uint32_t *save = nullptr, const int32_t *top_done = nullptr,
                                         int32_t *meet = nullptr) {
    constexpr int RM = T0_RSMALL;
    constexpr bool MEETC = LC_SPEC_MEET && !EX, CLOSED = LC_SPEC_CLOSED && !EX;
    const uint32_t lane = lane_id();
    LatMem m{ws, ws + T0_RMEM * 64, ws + 2 * T0_RMEM * 64};
    int32_t held = -1;  // LDS slot held
    const EvT ep = evp + b;
    const uint32_t nev = e_end - b;
    auto ldesc = [&](uint32_t w, bool have) -> uint32_t {
        const uint32_t t = LC_EV_TRANS(w);
        return (have && !(w & LC_EV_OK_BIT) && t < ntr) ? trp[t] : 0u;
    };
    uint32_t W[RM];
#pragma unroll
    for (int k = 0; k < RM; ++k) W[k] = 0;
    bool in_mem = false;
    uint32_t k_v = st.k_v, cap_v = st.cap_v, b_v = st.b_v, slot_v = st.slot_v, dense_v = st.dense_v;
    uint32_t n = st.n, live = st.live;
    uint32_t lm[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) lm[q] = (uint32_t)__builtin_amdgcn_sbfe((int)lane, q, 1);
    int status = 0;
    uint32_t fev = 0;
    uint32_t ev = lane < nev ? ep[lane] : 0u;
    uint32_t dsc = ldesc(ev, lane < nev);
    uint32_t ev_n = 64 + lane < nev ? ep[64 + lane] : 0u;
    uint32_t dsc_n = ldesc(ev_n, 64 + lane < nev);
    uint32_t ev_nn = 128 + lane < nev ? ep[128 + lane] : 0u;
    Xfer xc = xfer_of(dsc);
    uint32_t e = 0, i = 0, base = 0, lim = nev;
    // progress steps of the walk (its priority steps down at each): its
    // quarters; steps at 1/2, 3/4 and 7/8 measured no different (DESIGN.md,
    // "Issue priority by progress")
    const uint32_t q1 = nev / 4u, q2 = nev / 2u, q3 = nev - nev / 4u;
    if (MODE == 0 && prio) spec_prio(0);
    auto advance = [&]() {
        ++e;
        if (++i == 64u) {
            i = 0; base += 64;
            ev = ev_n; dsc = dsc_n; ev_n = ev_nn;
            xc = xfer_of(dsc);
            dsc_n = ldesc(ev_n, base + 64 + lane < nev);
            ev_nn = base + 128 + lane < nev ? ep[base + 128 + lane] : 0u;
            if (MODE == 0 && prio) spec_prio(base >= q3 ? 3u : base >= q2 ? 2u : base >= q1 ? 1u : 0u);
        }
    };
    // next checkpoint (relative event; ~0u: none)
    uint32_t ck_i = 0;
    uint32_t ck_at = ck1;
    if constexpr (MODE != 0) {
        const int32_t e0 = spec_ck_event(ck_e, 0, top_done);
        ck_at = e0 >= 0 ? (uint32_t)e0 - b : ~0u;
    }
    uint32_t W0 = st.W0;
    bool dirty = true;
    // meeting entries (MEETC): the next :ok's ordinal; on while the ring lasts
    // and no checkpoint has been recorded / compared
    uint32_t mt_ord = 0;
    auto mt_on = [&]() -> bool { return MEETC && meet != nullptr && mt_ord < SPEC_MEET_N && ck_i == 0; };
    // One lane-phase event (<= 6 pending); true: an :invoke with 6 pending,
    // for the dense phase.  CK: the event may be a checkpoint's :ok.  The
    // events before the next checkpoint run the body without that test, so
    // the checkpoint words stay out of the hot loop (one body for both
    // measured C2 0.2655 against 0.2596 ms: DESIGN.md, "The lane phase split
    // at the checkpoints").
    auto lane_event = [&](auto ck_t) -> bool {
        constexpr bool CK = decltype(ck_t)::value;
        const uint32_t evi = __builtin_amdgcn_readlane(ev, i);
        const uint32_t slot = LC_EV_SLOT(evi);
        if (!(evi & LC_EV_OK_BIT)) {
            if (n == 6) return true;
            // (n >= T0_MAX_WIDTH || slot >= 64 as one compare)
            if ((n | (slot & ~63u)) >= T0_MAX_WIDTH) {
                status = 3;
            } else {
                const uint32_t idx = (uint32_t)__builtin_ctz(~live);
                // the op's transfer read out first, then written: no wait
                // states between a v_readlane and the v_writelane of its value
                const uint32_t xk = (uint32_t)__builtin_amdgcn_readlane(xc.k, i),
                               xcap = (uint32_t)__builtin_amdgcn_readlane(xc.cap, i),
                               xb = (uint32_t)__builtin_amdgcn_readlane(xc.b, i);
                slot_v = setl(slot_v, idx, slot);
                k_v = setl(k_v, idx, xk);
                cap_v = setl(cap_v, idx, xcap);
                b_v = setl(b_v, idx, xb);
                dense_v = setl(dense_v, slot, idx);
                live |= 1u << idx;
                ++n;
                dirty = true;
            }
        } else {
            const uint32_t p = __builtin_amdgcn_readlane(dense_v, slot & 63u);
            int r;
            // closed sets: exact ones (ok_lane, as the wide T0 keeps
            // them) measured 10 % slower per event here
            // sweeps specialised to the highest live index (one body for
            // every live set measured 4 % slower per event here)
            const uint32_t top = 32u - (uint32_t)__builtin_clz(live);
            if constexpr (EX) {
                // exact sets: p's transfer, then its lane cleared (as in lattice_key)
                const uint32_t pk = __builtin_amdgcn_readlane(k_v, p), pc = __builtin_amdgcn_readlane(cap_v, p),
                               pb = __builtin_amdgcn_readlane(b_v, p);
                k_v = setl(k_v, p, 0u);
                uint32_t probes = 0, nSn = 0;
                if (top >= 6)
                    r = ok_lane<6>(W0, p, live, k_v, cap_v, b_v, pk, pc, pb, lane, lm, ~0ull, false, probes, nSn,
                                   false);
                else if (top == 5)
                    r = ok_lane<5>(W0, p, live, k_v, cap_v, b_v, pk, pc, pb, lane, lm, ~0ull, false, probes, nSn,
                                   false);
                else
                    r = ok_lane<4>(W0, p, live, k_v, cap_v, b_v, pk, pc, pb, lane, lm, ~0ull, false, probes, nSn,
                                   false);
            } else {
                if (top >= 6) r = ok_lane_closed<6>(W0, p, live, k_v, cap_v, b_v, lane, lm, dirty);
                else if (top == 5) r = ok_lane_closed<5>(W0, p, live, k_v, cap_v, b_v, lane, lm, dirty);
                else r = ok_lane_closed<4>(W0, p, live, k_v, cap_v, b_v, lane, lm, dirty);
                dirty = false;
                k_v = setl(k_v, p, 0u);
            }
            live = r ? live : live & ~(1u << p);
            n = r ? n : n - 1;
            status = r;
            fev = e;
            if (CK && !r && e >= ck_at) {  // a checkpoint (a lane-phase :ok: the set is canonical)
                if constexpr (MODE == 0) {
                    ck_w[ck_i][lane] = W0;
                    spec_publish(&ck_e[ck_i], (int32_t)(b + e));  // (after the set: a verifier may be waiting)
                    ++ck_i;
                    ck_at = ck_i < SPEC_NCK ? max(spec_ck_target(ck_i, ck1, ck2), e + 1u) : ~0u;
                } else {
                    if (!__any(W0 != ck_w[ck_i][lane])) {
                        status = 4;
                    } else {
                        ++ck_i;
                        const int32_t nx = ck_i < SPEC_NCK ? spec_ck_event(ck_e, ck_i, top_done) : -1;
                        ck_at = nx >= 0 ? (uint32_t)nx - b : ~0u;
                        if (ck_i == SPEC_NCK) status = 5;
                    }
                }
            } else if (CK && !r && mt_on()) {  // a meeting entry (before the first checkpoint)
                const int32_t mine = spec_meet_word(mt_ord, W0);
                if constexpr (MODE == 0) {
                    spec_publish(&meet[mt_ord], mine);
                    ++mt_ord;
                } else {
                    const int32_t theirs = spec_meet_entry(meet, mt_ord, top_done);
                    if (theirs == mine) status = 4;
                    mt_ord = theirs < 0 ? SPEC_MEET_N : mt_ord + 1u;
                }
            }
        }
        lim = status ? 0u : lim;
        advance();
        return false;
    };
    for (uint32_t phase = 0; phase <= nev && e < lim; ++phase) {
        bool dense = false;
        while (e < lim) {  // lane phase: <= 6 pending
            // (while meeting entries are due, every event runs the CK body)
            uint32_t stop = mt_on() ? e : min(lim, ck_at);
            while (e < stop) {
                if (lane_event(std::false_type{})) { dense = true; break; }
                stop = min(stop, lim);
            }
            if (dense || e >= lim) break;
            if (lane_event(std::true_type{})) { dense = true; break; }
        }
        (void)dense;
        if (e >= lim) break;
        W[0] = W0;
#pragma unroll
        for (int k = 1; k < RM; ++k) W[k] = 0u;
        while (e < lim) {  // dense phase: 7-10 pending
            const uint32_t evi = __builtin_amdgcn_readlane(ev, i);
            const uint32_t slot = LC_EV_SLOT(evi);
            if (!(evi & LC_EV_OK_BIT)) {
                if (n >= T0_MAX_WIDTH || slot >= 64) {
                    status = 3;
                } else {
                    if (n == 8) {  // 9 pending: the lattice moves to the workspace
                        int32_t got = -1;
                        if (lane == 0) {
                            for (int q = 0; q < NWS && got < 0; ++q)
                                if (atomicCAS(&lds_busy[q], 0, 1) == 0) got = q;
                        }
                        held = uni(got);
                        uint32_t *const mb = held >= 0 ? lds_ws + (size_t)held * (3 * T0_RMEM * 64) : ws;
                        m = LatMem{mb, mb + T0_RMEM * 64, mb + 2 * T0_RMEM * 64};
                        uint32_t *const mW = m.W + opq_lane(lane);
#pragma unroll
                        for (int k = 0; k < T0_RMEM; ++k) mW[k * 64] = k < RM ? W[k < RM ? k : 0] : 0u;
                        in_mem = true;
                    }
                    const uint32_t idx = n;
                    slot_v = setl(slot_v, idx, slot);
                    k_v = setl(k_v, idx, (uint32_t)__builtin_amdgcn_readlane(xc.k, i));
                    cap_v = setl(cap_v, idx, (uint32_t)__builtin_amdgcn_readlane(xc.cap, i));
                    b_v = setl(b_v, idx, (uint32_t)__builtin_amdgcn_readlane(xc.b, i));
                    dense_v = setl(dense_v, slot, idx);
                    live |= 1u << idx;
                    ++n;
                    dirty = true;
                }
            } else {
                const uint32_t p = __builtin_amdgcn_readlane(dense_v, slot & 63u);
                uint32_t nSn = 0, probes = 0;
                int r;
                if constexpr (CLOSED) {
                    if (n == 7) r = ok_reg_closed<2, RM>(W, p, k_v, cap_v, b_v, lane, dirty);
                    else if (n == 8) r = ok_reg_closed<4, RM>(W, p, k_v, cap_v, b_v, lane, dirty);
                    else if (n == 9) r = ok_event_mem_closed<8>(m, p, k_v, cap_v, b_v, lane, dirty);
                    else r = ok_event_mem_closed<16>(m, p, k_v, cap_v, b_v, lane, dirty);
                    dirty = false;
                } else {
                    if (n == 7) r = ok_reg<2, RM>(W, p, k_v, cap_v, b_v, lane, ~0ull, false, probes, nSn, false);
                    else if (n == 8) r = ok_reg<4, RM>(W, p, k_v, cap_v, b_v, lane, ~0ull, false, probes, nSn, false);
                    else if (n == 9) r = ok_event_mem_gs<8>(m, p, n, k_v, cap_v, b_v, lane);
                    else r = ok_event_mem_gs<16>(m, p, n, k_v, cap_v, b_v, lane);
                }
                if constexpr (MEETC) {
                    if (!r && mt_on()) {  // no compare here: the ordinals stay aligned
                        if constexpr (MODE == 0)
                            spec_publish(&meet[mt_ord], (int32_t)((mt_ord << 16) | SPEC_MEET_NOCMP));
                        ++mt_ord;
                    }
                }
                const uint32_t last = n - 1;
                const uint32_t s_last = __builtin_amdgcn_readlane(slot_v, last);
                const uint32_t x0 = __builtin_amdgcn_readlane(k_v, last), x1 = __builtin_amdgcn_readlane(cap_v, last),
                               x2 = __builtin_amdgcn_readlane(b_v, last);
                if (!r) {
                    slot_v = setl(slot_v, p, s_last);
                    k_v = setl(k_v, p, x0);
                    cap_v = setl(cap_v, p, x1);
                    b_v = setl(b_v, p, x2);
                    dense_v = setl(dense_v, s_last & 63u, p);
                    k_v = setl(k_v, last, 0u);
                }
                live = r ? live : (1u << last) - 1u;
                if (in_mem && n == 9 && !r) {
                    const uint32_t *const mW = m.W + opq_lane(lane);
#pragma unroll
                    for (int k = 0; k < RM; ++k) W[k] = mW[k * 64];
                    in_mem = false;
                    if (held >= 0 && lane == 0) atomicExch(&lds_busy[held], 0);
                    held = -1;
                }
                n = r ? n : n - 1;
                status = r;
                fev = e;
            }
            lim = status ? 0u : lim;
            advance();
            if (n <= 6) break;
        }
        W0 = W[0];
        // (closed dense sets: the set is as clean as the last event left it)
        if constexpr (!CLOSED) dirty = true;
    }
    if constexpr (EX) {
        if (save) {
            // the set standing at the end (or before the failing :ok): the
            // dense lattice (registers or the workspace) from 7 ops pending on
            if (n > 6) {
#pragma unroll 1
                for (int k = 0; k < T0_RMEM; ++k) {
                    uint32_t x = 0;
                    if (in_mem) x = m.W[k * 64 + opq_lane(lane)];
                    else {
#pragma unroll
                        for (int q = 0; q < RM; ++q)
                            if (q == k) x = W[q];
                    }
                    save[k * 64 + lane] = x;
                }
            } else {
                save[lane] = W0;
            }
            save[T0_RMEM * 64 + lane] = slot_v;
            if (lane == 0) save[(T0_RMEM + 1) * 64] = live;
        }
    }
    if (held >= 0 && lane == 0) atomicExch(&lds_busy[held], 0);
    if (MODE == 0 && prio) __builtin_amdgcn_s_setprio(0);
    st.W0 = W0;
    st.k_v = k_v; st.cap_v = cap_v; st.b_v = b_v; st.slot_v = slot_v; st.dense_v = dense_v;
    st.n = n; st.live = live;
    fev_out = b + fev;
    return status;
}

#ifdef LC_SPEC_STAMPS
// Diagnostic build only: per (block, wave) clock stamps of the phases.
__device__ unsigned long long lc_spec_stamps[4096 * 8 * 12];
extern "C" int lc_debug_spec_stamps(unsigned long long *host, int n) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(lc_spec_stamps), (size_t)n * 8 * 12 * 8, 0, hipMemcpyDeviceToHost);
}
#define SPEC_STAMP(s, k, v) \
    if (lane == 0 && blk < 4096 && (s) < 8) lc_spec_stamps[((size_t)blk * 8 + (s)) * 12 + (k)] = (v);
#else
#define SPEC_STAMP(s, k, v)
#endif

// One workgroup per key (blockIdx = LPT position), the key cut into up to S
// segments, one wave per segment: wave w walks segment w from TOP, then
// verifies the next kept segment from the set its walk ended with, and wave 0
// gives the key's verdict ("Speculative key segments").  Results go
// through a.full like T0's; a.lat_ws holds each wave's 9-10-pending fallback
// workspace (global memory: the workgroup's LDS workspaces are shared, NWS of
// them).
// 16-bit event words of a key k_spec stages in LDS: none for 2-segment
// workgroups (the many-key batches, where 6 KB more per block would cost
// occupancy), 4,096 (8 KB) otherwise -- C2's keys have ~1,470.  (The 8-wave
// build's 4 workgroups per CU, 8 waves per SIMD, fit the CU's 160 KB with
// these and 2 checkpoint sets per segment; a third set needs 3,072 here.)
template <int S, bool E16>
constexpr uint32_t spec_ev_lds() { return (E16 && S > 2) ? (S >= 8 && SPEC_NCK > 2 ? 3072u : 4096u) : 0u; }

// The 2-wave build (the many-key batches: C3's shards, throughput-bound) is
// held to 8 waves per SIMD: 64 VGPRs, 140 B per lane spilled to scratch, and
// no LDS workspace (LC_SPEC2_NWS) so that 8 fit.  A/B on one box, the C3
// shard (12,500 x 2,000), two rounds each (round 5): 6 waves per SIMD with
// the LDS workspace (5.5 resident) 3.881 ms per step, kernel 3.694; 6
// without it 3.814 / 3.650; 7 3.607 / 3.421; 8 3.601 / 3.427.  Records
// identical.  (Before: 84 VGPRs, 4 waves, 4.04 ms per step.)
#ifndef LC_SPEC2_WAVES
#define LC_SPEC2_WAVES 8
#endif
template <int S, bool E16, bool EX = false>
__global__ __launch_bounds__(64 * S, (S == 2 ? LC_SPEC2_WAVES : S == 8 ? LC_SPEC8_WAVES : 1)) void k_spec(T0Args a) {
// a's fields, read through the kernarg segment at each use (t0k): no faster
// than reading `a` (C2 0.2739 / 0.2732 ms), but half the scalar spills
// ("k_spec's arguments through the kernarg segment").
#define KA t0k()
    constexpr uint32_t EVC = spec_ev_lds<S, E16>();
    __shared__ uint16_t s_ev[EVC ? EVC : 1];  // the key's event words (EvStaged)
    __shared__ uint32_t s_end[S][64];     // TOP run's set at the segment's end
    __shared__ uint32_t s_ck[S][SPEC_NCK][64];  // TOP run's checkpoint sets
    __shared__ uint32_t s_pend[S][8];     // ops pending at the cut ([0..5] words, [6] count)
    __shared__ uint64_t s_map[S];         // end: byte i = 0x80 | slot of live op index i
    __shared__ int32_t s_ck_e[S][SPEC_NCK];  // checkpoint events (-1: none)
    __shared__ int32_t s_cut[S], s_segend[S];  // segment [cut, end); cut -1: no segment
    __shared__ int32_t s_top[S];          // TOP run: -1 alive, -2 does not fit, -3 lost, else its failing event
    __shared__ int32_t s_ver[S], s_vfev[S];
    __shared__ int32_t s_net[S];          // cut search: pending-count change over each part
    __shared__ int32_t s_cand[S], s_ncand[S];  // each target's cut (-1: none) and ops pending there
    __shared__ int32_t s_prdy[S], s_done[S];  // flags a verifying wave waits on: s_pend / s_top -3 of s out; TOP run of s ended
    __shared__ uint32_t s_vx[S][2];       // self-validation: each wave's part, XOR of its slots' one-hots
    constexpr bool MEETC = LC_SPEC_MEET && !EX;
    __shared__ int32_t s_meet[MEETC ? S : 1][SPEC_MEET_N];  // TOP run's meeting entries (-1: not published)
    constexpr int NWS = spec_lds_ws<S>();
    __shared__ uint32_t s_ws[NWS ? NWS * 3 * T0_RMEM * 64 : 1];  // 9-10-pending workspaces (12 KB each)
    __shared__ int32_t s_ws_busy[NWS ? NWS : 1];
    const uint32_t lane = lane_id(), wv = uni((uint32_t)threadIdx.x >> 6);  // uniform per wave
    // T0_STRICT steps: the event-by-event validation, in nb blocks after the
    // keys' (no second stream, no cross-stream waits around the step), or
    // before them (T0_SPEC_VFIRST)
    const uint32_t nb = gridDim.x - (uint32_t)KA.n_order;
    const bool vfirst = (KA.flags & T0_SPEC_VFIRST) != 0;
    const uint32_t blk = vfirst ? blockIdx.x - nb : blockIdx.x;  // the key block's LPT position
    if (vfirst ? blockIdx.x < nb : blockIdx.x >= (uint32_t)KA.n_order) {
        const uint32_t vb = vfirst ? blockIdx.x : blockIdx.x - (uint32_t)KA.n_order;
        for (int64_t k = (int64_t)vb * S + wv; k < KA.n_order; k += (int64_t)nb * S) {
            // (a key whose words its own block stages whole is validated
            // there, from LDS: see below)
            if (EVC > 0 && !(KA.flags & T0_SPEC_NOSTAGE) && KA.ev_off[k + 1] - KA.ev_off[k] <= EVC) continue;
            validate_key<false, E16>(a, k);
        }
        return;  // the whole block: no barrier below is reached by half of it
    }
    // (The block's set-up -- staging, validation, the cuts -- runs at issue
    // priority 0: at a TOP walk's first-quarter priority it measured -0.3 % on
    // C2 / C5 and other seeds, within noise, profiles/r06_segments_seeds.txt.)
    // (scalar: as a VGPR it was the 64-VGPR builds' last spill to scratch)
    const int32_t key = (int32_t)uni((uint32_t)KA.order[blk]);
    uint32_t *ws = KA.lat_ws + ((size_t)blk * S + wv) * (3 * T0_RMEM * 64);
    const uint64_t eb = KA.ev_off[key];
    const uint32_t nev = (uint32_t)(KA.ev_off[key + 1] - eb);
    // the key's words: staged in LDS (8 loads in flight per thread, then the
    // stores; made visible by the barrier below), else read from HBM
    uint32_t n_lds = 0;
    if constexpr (EVC > 0) {
        if (!(KA.flags & T0_SPEC_NOSTAGE)) {
            n_lds = nev < EVC ? nev : EVC;
            const uint16_t *g = KA.events16 + eb;
            for (uint32_t base = 0; base < n_lds; base += 64u * S * 8u) {
                uint16_t v[8];
#pragma unroll
                for (uint32_t q = 0; q < 8; ++q) {
                    const uint32_t j = base + q * 64u * S + threadIdx.x;
                    v[q] = j < n_lds ? g[j] : (uint16_t)0;
                }
#pragma unroll
                for (uint32_t q = 0; q < 8; ++q) {
                    const uint32_t j = base + q * 64u * S + threadIdx.x;
                    if (j < n_lds) s_ev[j] = v[q];
                }
            }
        }
    }
    using EvK = typename std::conditional<(EVC > 0), EvStaged, EvSrc<E16>>::type;
    EvK evp;
    if constexpr (EVC > 0) evp = EvStaged{(LdsU16 *)s_ev, KA.events16 + eb, n_lds};
    else evp = ev_src<E16>(KA) + eb;
    const uint32_t tb = KA.trans_off ? KA.trans_off[key] : 0u;
    const uint32_t ntr = KA.n_trans > tb ? KA.n_trans - tb : 0u;
    const uint32_t *const trp = KA.trans + (ntr ? tb : 0u);
    const uint32_t nstates = KA.trans_off ? (KA.key_states ? KA.key_states[key] : 0xFFFFu) : KA.shared_states;
    const uint32_t width = KA.key_width ? KA.key_width[key] : 0xFFu;
    // keys no wave walks: errors and keys outside the tier, which the verdict
    // step finishes as lattice_key's prologue does
    const bool plain = (KA.key_error && KA.key_error[key]) ||
                       (KA.key_states && KA.key_states[key] > LC_WIDE_MAX_STATES) || nstates > T0_MAX_STATES ||
                       width > T0_MAX_WIDTH || KA.init_state >= T0_MAX_STATES;
    // a key too short to cut is one segment: wave 0's exact walk of segment 0
    // from the initial state is the key's verdict (eff = max(1, min(S, nev /
    // SPEC_MIN_LEN)) for every key that is walked)
    const bool whole = plain || nstates == 0 || nev < 2 * SPEC_MIN_LEN;
    const uint32_t eff = whole ? 1u : min((uint32_t)S, nev / SPEC_MIN_LEN);
    const uint32_t topmask = nstates >= 32 ? ~0u : (1u << nstates) - 1u;

    if (threadIdx.x < NWS) s_ws_busy[threadIdx.x] = 0;
    if (MEETC && threadIdx.x < S * SPEC_MEET_N) s_meet[threadIdx.x / SPEC_MEET_N][threadIdx.x % SPEC_MEET_N] = -1;
    __syncthreads();
    // T0_STRICT batches whose key the block staged whole: the key's
    // validation here, from LDS, its 64-event chunks split over the S waves
    // (the slot protocol's state at a wave's first chunk is the XOR of the
    // earlier waves' slot parities, exchanged at the cut search's barrier),
    // instead of a second HBM read of the words in the validation blocks.
    bool self_val = false;
    uint32_t vc0 = 0, vc1 = 0;
    if constexpr (EVC > 0) {
        self_val = (KA.flags & T0_STRICT) && !(KA.flags & T0_SPEC_NOSTAGE) && n_lds == nev &&
                   !(KA.key_error && KA.key_error[key]);
        const uint32_t nch = (nev + 63u) / 64u;
        vc0 = nch * wv / S;
        vc1 = nch * (wv + 1u) / S;
        if (self_val) {
            uint32_t x0 = 0, x1 = 0;
            for (uint32_t ch = vc0; ch < vc1; ++ch) {
                const uint32_t j = ch * 64u + lane;
                if (j < nev) {
                    const uint32_t sl = LC_EV_SLOT(LC_EV16_WIDE(s_ev[j]));
                    x0 ^= sl < 32u ? 1u << sl : 0u;
                    x1 ^= (sl >= 32u && sl < 64u) ? 1u << (sl - 32u) : 0u;
                }
            }
            x0 = uni(__ockl_wfred_xor_u32(x0));
            x1 = uni(__ockl_wfred_xor_u32(x1));
            if (lane == 0) { s_vx[wv][0] = x0; s_vx[wv][1] = x1; }
        }
    }
    if (wv == 0) {
        for (uint32_t s = 0; s < (uint32_t)S; ++s) { SPEC_STAMP(s, 0, __builtin_amdgcn_s_memtime()) }
    }
    // 0. the cuts.  Targets at s/eff of the key's events (T0_SPEC_COST: of its
    // estimated cost, each wave computing every target); each moved to the
    // boundary with the fewest ops pending within 64 events.  Equal event
    // counts: the waves count the pending-count change over the parts
    // [t_p, t_p+1) (part p on wave p mod S), the parts' prefix gives the count
    // at each target, and the waves place the cuts likewise -- two barriers.
    const bool cost = (KA.flags & T0_SPEC_COST) != 0;
    if (!plain && !cost) {
        for (uint32_t p = wv; p + 1 < eff; p += S) {
            const uint32_t t0 = (uint32_t)((uint64_t)nev * p / eff), t1 = (uint32_t)((uint64_t)nev * (p + 1) / eff);
            const int32_t d = spec_net(evp, t0, t1);
            if (lane == 0) s_net[p] = d;
        }
    }
    __syncthreads();
    if constexpr (EVC > 0) {
        if (self_val) {
            // (the states a transition may install: as validate_key reads them)
            const uint32_t vns = KA.trans_off ? (KA.key_states ? KA.key_states[key] : 0u) : KA.shared_states;
            uint32_t pend[2] = {0u, 0u};
            for (uint32_t q = 0; q < wv; ++q) { pend[0] ^= uni(s_vx[q][0]); pend[1] ^= uni(s_vx[q][1]); }
            int32_t why = 0;
            for (uint32_t ch = vc0; ch < vc1 && !why; ++ch) {
                const uint32_t j = ch * 64u + lane;
                const bool in = j < nev;
                const uint32_t w = in ? LC_EV16_WIDE(s_ev[j]) : 0u;
                why = validate_chunk<false, 2>(w, in, trp, ntr, vns, 64u, pend);
            }
            if (why && lane == 0) {
                atomicOr(&KA.err[0], why);
                atomicMax(&KA.err[1], KA.err_base + key + 1);
            }
        }
    }
    if (!plain && !cost) {
        for (uint32_t s = wv; s < eff; s += S) {
            if (s == 0) continue;
            int32_t pend = 0;
            for (uint32_t q = 0; q < s; ++q) pend += uni(s_net[q]);
            const uint32_t t = (uint32_t)((uint64_t)nev * s / eff);
            const uint32_t w = t + lane < nev ? evp[t + lane] : 0u;
            uint32_t n2 = 0;
            const uint32_t c2 = spec_cut_at(w, nev, t, pend, n2);
            if (lane == 0) {
                s_cand[s] = c2 == SPEC_NONE ? -1 : (int32_t)c2;
                s_ncand[s] = (int32_t)n2;
            }
        }
    }
    if (!plain && cost && wv < eff) {
        uint32_t pos_v;
        int32_t pend_v;
        spec_targets_cost(evp, nev, eff, pos_v, pend_v);
        for (uint32_t s = wv; s < eff; s += S) {  // every wave has every target: each places its own cuts
            if (s == 0) continue;
            const uint32_t t = uni(__builtin_amdgcn_readlane(pos_v, s));
            const uint32_t w = t + lane < nev ? evp[t + lane] : 0u;
            uint32_t n2 = 0;
            const uint32_t c2 = spec_cut_at(w, nev, t, uni(__builtin_amdgcn_readlane(pend_v, s)), n2);
            if (lane == 0) {
                s_cand[s] = c2 == SPEC_NONE ? -1 : (int32_t)c2;
                s_ncand[s] = (int32_t)n2;
            }
        }
    }
    __syncthreads();
    // the kept cuts (each past the last kept one; a segment ends at the next
    // kept cut), by one thread
    if (threadIdx.x == 0 && !plain) {
        int32_t last = 0;
        s_cut[0] = 0;
        for (uint32_t s = 1; s < eff; ++s) {
            int32_t c2 = s_cand[s];
            if (c2 >= 0 && c2 <= last) c2 = -1;
            if (c2 >= 0) last = c2;
            s_cut[s] = c2;
        }
        int32_t end = (int32_t)nev;
        for (uint32_t s = eff; s-- > 0;) {
            s_segend[s] = end;
            if (s_cut[s] >= 0) end = s_cut[s];
            for (uint32_t q = 0; q < SPEC_NCK; ++q) s_ck_e[s][q] = -1;
            s_top[s] = -1;
        }
        for (uint32_t s = 0; s < (uint32_t)S; ++s) {
            s_prdy[s] = 0;
            s_done[s] = 0;
            s_ver[s] = 0;
            s_vfev[s] = -1;
        }
    }
    __syncthreads();
    // 1 + 2. wave w walks segment w from TOP (segment 0 exactly), then at
    // once verifies the next kept segment from the set its own walk ended
    // with; no barrier stands between the two.  The verifying run compares
    // with that segment's TOP run at its checkpoints, which that run publishes
    // as it passes them (spec_ck_event waits for one not reached yet), and
    // with its end set once it has ended.  A block takes about its slowest
    // TOP walk, not its slowest TOP walk plus its slowest verifying run.
    // INVARIANT: no open loop (`for (;;) ... break` compiles into an
    // exec-masked loop whose exit can hang the wave), and every branch on a
    // segment index or an LDS flag is on a uni() value; the flag waits
    // (spec_wait, spec_ck_event) have a fixed trip count.
    // tests/test_kernel_lint.py checks these shapes in this file.
    if (!plain) {
        const uint32_t s = wv;
        const bool kept = s < eff && uni(s_cut[s]) >= 0;
        int32_t top_s = -1;
        if (kept) {
            const int32_t cut_i = uni(s_cut[s]);
            const uint32_t cut = (uint32_t)cut_i, end = (uint32_t)uni(s_segend[s]);
            const uint32_t n0 = s == 0 ? 0u : (uint32_t)uni(s_ncand[s]);
            SPEC_STAMP(s, 1, __builtin_amdgcn_s_memtime())
            SPEC_STAMP(s, 6, ((unsigned long long)end << 32) | cut)
            SPEC_STAMP(s, 8, (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) |
                                 ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32))
            SPEC_STAMP(s, 9, (unsigned long long)key)
            SpecState st{};
            uint32_t words = 0, np = 0;
            if (s == 0) {
                st.W0 = lane == 0 ? 1u << KA.init_state : 0u;
            } else {
                words = spec_pending(evp, cut, n0, np);
                spec_setup(st, words, np, trp, ntr);
                st.W0 = lane < (1u << np) ? topmask : 0u;
            }
            if (lane < 6) s_pend[s][lane] = words;
            if (lane == 6) s_pend[s][6] = np;
            // the ops found pending must be as many as the count says (else
            // the event stream is malformed): the key is searched unsegmented
            const bool lost = s != 0 && np != n0;
            if (lost && lane == 0) s_top[s] = -3;
            spec_publish(&s_prdy[s]);
            uint32_t fev = 0;
            uint32_t *const sv = EX ? KA.spec_fin + ((size_t)blk * S + s) * 2 * SPEC_SAVE_WORDS : nullptr;
            const int r = lost ? 6
                               : spec_walk<0, NWS, EvK, EX>(evp, trp, ntr, cut, end, st, ws, s_ws, s_ws_busy,
                                                                   s_ck[s], s_ck_e[s], KA.spec_ck1, KA.spec_ck2,
                                                                   fev, !(KA.flags & T0_SPEC_NOPRIO), sv, nullptr,
                                                                   (MEETC && s != 0) ? s_meet[s] : nullptr);
            s_end[s][lane] = st.W0;
            uint64_t map = 0;
            for (uint32_t q = 0; q < 6; ++q) {
                const uint32_t sl = __builtin_amdgcn_readlane(st.slot_v, q);
                if ((st.live >> q) & 1u) map |= (uint64_t)(0x80u | sl) << (8 * q);
            }
            SPEC_STAMP(s, 2, __builtin_amdgcn_s_memtime())
            top_s = r == 1 ? (int32_t)fev : r == 3 ? -2 : r == 6 ? -3 : -1;
            if (lane == 0) {
                s_map[s] = map;
                s_top[s] = top_s;
            }
            spec_publish(&s_done[s]);
        }
        // the next kept segment (its predecessor is this one)
        uint32_t v = s + 1;
        while (v < eff && uni(s_cut[v]) < 0) ++v;
        if (kept && top_s == -1 && v < eff) {
            SPEC_STAMP(v, 3, __builtin_amdgcn_s_memtime())
            int32_t ver = 3, vfev = -1;  // (a wait that gives up: the key goes unsegmented)
            uint32_t fev = 0;
            if (spec_wait(&s_prdy[v]) && spec_load(&s_top[v]) != -3) {
                const uint32_t cut = (uint32_t)uni(s_cut[v]), end = (uint32_t)uni(s_segend[v]);
                const uint32_t np = uni(s_pend[v][6]);
                SpecState st{};
                spec_setup(st, lane < 6 ? s_pend[v][lane] : 0u, np, trp, ntr);
                // this walk's end set, relabelled from its op indices to v's
                const uint64_t map = uni(s_map[s]);
                uint32_t src = 0;
                for (uint32_t j = 0; j < np; ++j) {
                    const uint32_t sl = __builtin_amdgcn_readlane(st.slot_v, j);
                    uint32_t at = 31;
                    for (uint32_t q = 0; q < 6; ++q)
                        if (((map >> (8 * q)) & 0xFFu) == (0x80u | sl)) at = q;
                    src |= ((lane >> j) & 1u) << at;
                }
                const uint32_t E = (uint32_t)__shfl((int)s_end[s][lane], (int)(src & 63u));
                st.W0 = lane < (1u << np) ? E : 0u;
                uint32_t *const sv =
                    EX ? KA.spec_fin + ((size_t)blk * S + v) * 2 * SPEC_SAVE_WORDS + SPEC_SAVE_WORDS : nullptr;
                // (the verifying runs stay at issue priority 0: 2 and 3 measured
                // slower on C2 and most seeds, profiles/r06_segments_seeds.txt)
                const int r = spec_walk<1, NWS, EvK, EX>(evp, trp, ntr, cut, end, st, ws, s_ws, s_ws_busy,
                                                                s_ck[v], s_ck_e[v], 0, 0, fev, false, sv,
                                                                &s_done[v], MEETC ? s_meet[v] : nullptr);
                bool last = true;
                for (uint32_t q = v + 1; q < eff; ++q) last = last && uni(s_cut[q]) < 0;
                if (r == 4) ver = 1;                        // met the TOP run
                else if (r == 1) { ver = 2; vfev = (int32_t)fev; }  // died before meeting it
                else if (r == 3) ver = 6;                   // does not fit
                else if (r == 5) ver = 3;                   // never met
                else if (last) ver = 5;                     // the last segment, searched exactly to its end
                else if (spec_wait(&s_done[v])) ver = (st.n <= 6 && !__any(st.W0 != s_end[v][lane])) ? 1 : 3;
            }
            SPEC_STAMP(v, 7, ((unsigned long long)ver << 32) | (fev - (uint32_t)uni(s_cut[v])))
            SPEC_STAMP(v, 4, __builtin_amdgcn_s_memtime())
            if (lane == 0) {
                s_ver[v] = ver;
                s_vfev[v] = vfev;
            }
        }
    }
    __syncthreads();
    if (wv == 0) {
        for (uint32_t s = 0; s < (uint32_t)S; ++s) { SPEC_STAMP(s, 5, __builtin_amdgcn_s_memtime()) }
    }
    // 3. the key's verdict: the first segment whose real run dies
    if (wv == 0) {
        const Args &f = *KA.full;
        bool rerun = false, bad = false;
        int32_t fv = -1;
        // EX: the run whose set is the key's final one -- 2 x segment, + 1 for
        // the verifying run: the run that truly died, or the last segment's
        // true run
        uint32_t fin_run = 0;
        if (!plain) {
            for (uint32_t s = 0; s < eff && fv < 0 && !rerun && !bad; ++s) {
                if (uni(s_cut[s]) < 0) continue;
                const int32_t top = uni(s_top[s]);
                if (top == -2) { bad = true; break; }
                if (top == -3) { rerun = true; break; }
                fin_run = 2 * s;
                if (s == 0) { fv = top; continue; }
                const int32_t ver = uni(s_ver[s]);
                if (ver == 1) fv = top;
                else if (ver == 2) { fv = uni(s_vfev[s]); fin_run = 2 * s + 1; }
                else if (ver == 5) fin_run = 2 * s + 1;
                else if (ver == 6) bad = true;
                else rerun = true;  // never met (or nothing to start from): unsegmented
            }
        }
        int kr = K_DONE;
        // the unsegmented search runs in a launch of its own (k_spec_rerun):
        // inlined here it cost this kernel 27 VGPRs, 6 -> 4 waves per SIMD
        if (plain) {  // in lattice_key's order: the packer's mark, the states, the tier
            if (KA.key_error && KA.key_error[key]) finish_key(f, key, LC_UNKNOWN, LC_CAUSE_ERROR, -1, 0, 0, 0);
            else if (KA.key_states && KA.key_states[key] > LC_WIDE_MAX_STATES)
                finish_key(f, key, LC_UNKNOWN, LC_CAUSE_STATES, -1, 1, 0, 0);
            else kr = K_SPILL;
        } else if (rerun) {
            if (lane == 0) KA.spec_rr[atomicAdd(KA.spec_nrr, 1)] = key;
        } else if (bad) kr = K_SPILL;
        else if (fv >= 0) finish_key(f, key, LC_INVALID, LC_CAUSE_NONLIN, fv, 0, 0, (uint64_t)fv + 1u);
        else finish_key(f, key, LC_VALID, LC_CAUSE_NONE, -1, 0, 0, nev);
        if constexpr (EX) {
            if (!plain && !rerun && !bad) {
                uint32_t *const sv = KA.spec_fin + ((size_t)blk * S * 2 + fin_run) * SPEC_SAVE_WORDS;
                const LatMem fm{sv, sv, sv};
                write_final_mem(f, key, fm, lane, sv[T0_RMEM * 64 + lane], uni(sv[(T0_RMEM + 1) * 64]));
            }
        }
        if (kr == K_SPILL) {
            if (KA.flags & T0_STRICT) {
                t0_malformed(KA, key, LC_BATCH_E_FIT);
                finish_key(f, key, LC_UNKNOWN, LC_CAUSE_ERROR, -1, 0, 0, 0);
            } else {
                const bool deep = f.deep && KA.key_width && KA.key_width[key] > LC_DIRECT_T3_WIDTH;
                push_list(deep ? f.deep : f.spill, deep ? f.n_deep : f.n_spill, key, f.list_cap);
            }
        }
    }
}
#undef KA

// The keys k_spec left to the unsegmented search (compact T0, FAST): runs
// that never met, lost their pending set or gave up a wait.  One wave per
// workgroup, no LDS and at most 128 VGPRs (tests/test_rerun_metadata.py), so
// a block fits wherever one k_spec<8> workgroup of the other lane's launch
// has ended (4 of them fill a CU's LDS, 8 of their 64-VGPR waves a SIMD): the
// launch is in every step and usually finds no key, so its dispatch is what
// it costs.  Wave b's 9-10-pending workspace is slot b of the lane's own
// k_spec workspaces (a.lat_ws), free once that k_spec has ended -- this
// launch follows it in stream order -- so an :ok there takes ~40k cycles
// against ~2k in LDS (spec_walk's note): accepted on a path no measured
// history takes.  The grid is StepPlan::rerun_grid, at most the slots.
template <bool E16, bool EX = false>
__global__ __launch_bounds__(64) void k_spec_rerun(T0Args a) {
    uint32_t *const ws = a.lat_ws + (size_t)blockIdx.x * (3 * T0_RMEM * 64);
    const int32_t n = *a.spec_nrr;
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.spec_nrr_next = 0;  // two counters in turn: no memset per step
    for (int32_t w = (int32_t)blockIdx.x; w < n; w += (int32_t)gridDim.x) {
        const int32_t key = a.spec_rr[w];
        const int kr = lattice_key<T0_RSMALL, !EX, E16>(a, key, ws);
        if (kr == K_SPILL) t0_spill(a, key);
    }
}

#ifdef LC_T0_COUNT_SWEEPS
// Diagnostic build only: this unit's share of lc_debug_sweep_hist (device_lattice.hip).
int spec_sweep_hist(unsigned long long *host) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(lc_sweep_hist), sizeof(lc_sweep_hist), 0, hipMemcpyDeviceToHost);
}
#endif

size_t spec_ws_words(int64_t n_keys, int segs) { return (size_t)std::max<int64_t>(n_keys, 1) * segs * lat_ws_words(); }

size_t spec_fin_words(int64_t n_keys, int segs) {
    return (size_t)std::max<int64_t>(n_keys, 1) * segs * 2 * SPEC_SAVE_WORDS;
}
// Keys order[0 .. n_order) in workgroups of l.segs segments, then the rerun
// launch (device_search.hpp SpecLaunch).
hipError_t launch_spec(const Args &a, const Args *a_dev, const SpecLaunch &l, hipStream_t s) {
    const int segs = l.segs;
    const uint16_t *const events16 = l.events16;
    uint32_t *const fin = l.fin;
    T0Args t = make_t0(a, a_dev);
    t.events16 = events16;
    if (l.cost_cuts) t.flags |= T0_SPEC_COST;
    if (!l.stage) t.flags |= T0_SPEC_NOSTAGE;
    if (l.vfirst && l.validate_blocks > 0) t.flags |= T0_SPEC_VFIRST;
    if (!l.prio) t.flags |= T0_SPEC_NOPRIO;
    t.lat_ws = l.ws;
    t.spec_ck1 = l.ck1;
    t.spec_ck2 = l.ck2;
    t.spec_nrr = l.rr + (l.parity & 1);
    t.spec_nrr_next = l.rr + ((l.parity & 1) ^ 1);
    t.spec_rr = l.rr + 2;
    t.spec_fin = fin;
    const dim3 grid((unsigned)std::max(1, a.n_order + std::max(0, l.validate_blocks)));
    // (one wave each, wave b on workspace slot b: never more than the slots)
    const dim3 rgrid((unsigned)std::max(1, std::min(a.n_order * segs, l.rerun_grid)));
    // one wave per segment: more segments than waves (8, 12 or 16 on 4
    // waves, 4 or 8 on 2) measured slower (step_plan.hpp)
#define LC_SPEC_L(SS, E, X) hipLaunchKernelGGL((k_spec<SS, E, X>), grid, dim3(64 * SS), 0, s, t)
#define LC_SPEC_ALL(E)                                      \
    if (fin) {                                              \
        if (segs >= 8) LC_SPEC_L(8, E, true);               \
        else if (segs >= 4) LC_SPEC_L(4, E, true);          \
        else LC_SPEC_L(2, E, true);                         \
    } else if (segs >= 8) LC_SPEC_L(8, E, false);           \
    else if (segs >= 6) LC_SPEC_L(6, E, false);             \
    else if (segs >= 4) LC_SPEC_L(4, E, false);             \
    else if (segs >= 3) LC_SPEC_L(3, E, false);             \
    else LC_SPEC_L(2, E, false);
    if (events16) { LC_SPEC_ALL(true) } else { LC_SPEC_ALL(false) }
#undef LC_SPEC_ALL
#undef LC_SPEC_L
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (events16) {
        if (fin) hipLaunchKernelGGL((k_spec_rerun<true, true>), rgrid, dim3(64), 0, s, t);
        else hipLaunchKernelGGL((k_spec_rerun<true, false>), rgrid, dim3(64), 0, s, t);
    } else {
        if (fin) hipLaunchKernelGGL((k_spec_rerun<false, true>), rgrid, dim3(64), 0, s, t);
        else hipLaunchKernelGGL((k_spec_rerun<false, false>), rgrid, dim3(64), 0, s, t);
    }
    return hipGetLastError();
}

}  // namespace lcd
