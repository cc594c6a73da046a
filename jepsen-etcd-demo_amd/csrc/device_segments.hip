// device_segments.hip -- key segments: a serial key cut at quiescent points,
// its segments searched on waves of their own (k_seg_prep, k_search_segments,
// k_seg_compose, k_seg_rerun).

#include "lattice_core.hpp"

namespace lcd {

// ---- Key segments ------------------------------------------------------------
//
// With every key's events strictly serial, a batch of about one key per SIMD
// (C2: 1,000 keys on 1,024 SIMDs) leaves each SIMD one wave whose dependency
// chains are all exposed.  The search distributes over initial states: the
// set after any event, from an initial set S, is the union of the sets
// reached from each s in S.  So a key is cut at quiescent points (no op
// pending: the config set is a plain set of register states) and each
// segment is searched on a wave of its own from every start state at once:
// the lattice word holds one 6-bit group per start state (xfer_tag), valid
// where the key's values are interned as states 1..5 and no op installs nil
// (state 0): a cut is placed only after a write or cas has been invoked
// (and, the point being quiescent, completed), so nil cannot be a start
// state.  Segment 0 starts from the initial state alone and is searched
// untagged.  A per-key composition then walks the segments: the states
// after segment s are the union, over the states standing before it, of
// their groups in its final word; the key dies in the first segment whose
// union is empty, and only that segment is searched again, untagged, from
// the states before it, for the failing event.  Verdicts only (the FAST
// path): no set sizes, probes or final configs.

// Cut points of one key per wave: a chunk of 64 events per pass (the next
// chunk's words in flight), the pending count as a wave prefix sum, a cut
// after an event that leaves nothing pending once a write / cas has been
// invoked, at least seg_len events past the previous cut (longer for a key
// that would otherwise need more than max_seg segments).
__global__ __launch_bounds__(64) void k_seg_prep(SegArgs a) {
    const uint32_t lane = lane_id();
    for (int32_t key = blockIdx.x; key < a.n_keys; key += gridDim.x) {
        uint32_t *ends = a.seg_end + (size_t)key * a.max_seg;
        if (a.key_error && a.key_error[key]) {
            if (lane == 0) a.seg_cnt[key] = 0;
            continue;
        }
        const uint64_t eb = a.ev_off[key];
        const uint32_t nev = (uint32_t)(a.ev_off[key + 1] - eb);
        const uint32_t seg_len = max(a.seg_len, (nev + a.max_seg - 2) / (a.max_seg - 1));
        int32_t count = 0;   // ops pending before this chunk
        bool wseen = false;  // a write / cas invoked before this chunk
        uint32_t last = 0, nseg = 0;
        uint32_t w_next = lane < nev ? a.events[eb + lane] : LC_EV_OK_BIT;
        for (uint32_t base = 0; base < nev; base += 64) {
            const uint32_t j = base + lane;
            const bool in = j < nev;
            const uint32_t w = w_next;
            w_next = j + 64 < nev ? a.events[eb + j + 64] : LC_EV_OK_BIT;
            const bool ok = (w & LC_EV_OK_BIT) != 0;
            const uint32_t t = LC_EV_TRANS(w);
            const uint32_t d = (in && !ok && t < a.n_trans) ? a.trans[t] : 0u;
            const int32_t x = wave_scan(in ? (ok ? -1 : 1) : 0);
            const int32_t cnt = count + x;  // ops pending after event j
            const uint64_t wb = __ballot(in && !ok && (d & 3u) >= LC_T_WRITE);
            const uint64_t upto = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
            const bool wsj = wseen || (wb & upto) != 0;
            uint64_t cand = __ballot(in && cnt == 0 && wsj && j + 1 < nev);
            while (cand && nseg + 1 < a.max_seg) {
                const uint32_t l = (uint32_t)__builtin_ctzll(cand);
                cand &= cand - 1;
                const uint32_t pos = base + l + 1;
                if (pos - last >= seg_len) {
                    if (lane == 0) ends[nseg] = pos;
                    ++nseg;
                    last = pos;
                }
            }
            count = __shfl(cnt, 63);
            wseen = wseen || wb != 0;
        }
        if (lane == 0) {
            ends[nseg] = nev;
            ++nseg;
            a.seg_cnt[key] = nseg;
            const int32_t at = atomicAdd(&a.ctl[0], (int32_t)nseg);
            for (uint32_t s = 0; s < nseg; ++s) a.work[at + (int32_t)s] = ((uint32_t)key << 8) | s;
        }
    }
}

// One segment [sb, se) of a key from the start word `init` (untagged: a
// state mask; tagged: TAG_ID), on the compact lattice with closed sets (the
// register tier's FAST path).  status 0: fin = the OR of every config word
// left (for a quiescent end, lane 0's word); 1: every start died at event
// fev (key-relative); 3: the key does not fit the register tier.
template <bool TAG>
__device__ __forceinline__ void segment_search(const SegArgs &a, int32_t key, uint32_t sb, uint32_t se,
                                               uint32_t init, uint32_t *ws, int &status_out, uint32_t &fev_out,
                                               uint32_t &fin_out) {
    constexpr int RM = T0_RSMALL;
    const uint32_t lane = lane_id();
    const LatMem m{ws, ws + T0_RMEM * 64, ws + 2 * T0_RMEM * 64};
    uint32_t W[RM];
    LatWalk w;
    lattice_walk<RM, true, TAG>(W, w, ev_src<false>(a) + (a.ev_off[key] + sb), se - sb, a.trans, a.n_trans, init, m,
                                ~0ull, false, false);
    uint32_t f = 0;
    if (w.in_mem) {
#pragma unroll 1
        for (int k = 0; k < T0_RMEM; ++k) f |= m.W[k * 64 + lane];
    } else {
#pragma unroll
        for (int k = 0; k < RM; ++k) f |= W[k];
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) f |= (uint32_t)__shfl_xor((int)f, o);
    status_out = w.status;
    fev_out = sb + w.fev;
    fin_out = w.status ? 0u : f;
}

// Every segment of the work list, one wave each (persistent grid, tickets).
__global__ __launch_bounds__(64) void k_search_segments(SegArgs a) {
    __shared__ uint32_t ws[3 * T0_RMEM * 64];
    const int32_t nwork = a.ctl[0];
    for (int32_t guard = 0; guard <= nwork; ++guard) {
        int32_t w = 0;
        if (lane_id() == 0) w = atomicAdd(&a.ctl[1], 1);
        w = __builtin_amdgcn_readfirstlane(w);
        if (w >= nwork) break;
        const uint32_t item = a.work[w];
        const int32_t key = (int32_t)(item >> 8);
        const uint32_t s = item & 0xFFu;
        const uint32_t *ends = a.seg_end + (size_t)key * a.max_seg;
        const uint32_t sb = s ? ends[s - 1] : 0u, se = ends[s];
        int status;
        uint32_t fev, fin;
        if (s == 0) segment_search<false>(a, key, sb, se, 1u, ws, status, fev, fin);  // from nil (state 0)
        else segment_search<true>(a, key, sb, se, TAG_ID, ws, status, fev, fin);
        if (lane_id() == 0) {
            a.seg_out[(size_t)key * a.max_seg + s] = fin;
            if (s == 0) a.seg0_fev[key] = status == 1 ? (int32_t)fev : -1;
        }
        if (status == 3) t0_malformed(a, key, LC_BATCH_E_FIT);  // declared to fit the register tier, and it does not
    }
}

// A segmented key's verdict (and its LC_REC_* record when asked for).
__device__ __forceinline__ void seg_verdict(const SegArgs &a, int32_t key, int v, int cause, int32_t fev) {
    a.valid[key] = (int8_t)v; a.cause[key] = (uint8_t)cause; a.fail_event[key] = fev;
    if (a.rec)
        a.rec[key] = (uint64_t)(uint8_t)(v + 1) | (uint64_t)(uint8_t)cause << 8 | (uint64_t)(uint32_t)(fev + 1) << 16;
}

// Per key (one thread each): compose the segments' final words.
__global__ __launch_bounds__(256) void k_seg_compose(SegArgs a) {
    for (int32_t key = blockIdx.x * blockDim.x + threadIdx.x; key < a.n_keys; key += gridDim.x * blockDim.x) {
        if (a.key_error && a.key_error[key]) {
            seg_verdict(a, key, LC_UNKNOWN, LC_CAUSE_ERROR, -1);
            continue;
        }
        const uint32_t n = a.seg_cnt[key];
        const uint32_t *out = a.seg_out + (size_t)key * a.max_seg;
        if (out[0] == 0u) {  // segment 0 is searched from the initial state itself
            seg_verdict(a, key, LC_INVALID, LC_CAUSE_NONLIN, a.seg0_fev[key]);
            continue;
        }
        uint32_t S = (out[0] >> 1) & 0x1Fu;  // state ids 1..5 -> start groups 0..4
        bool dead = false;
        for (uint32_t s = 1; s < n && !dead; ++s) {
            const uint32_t F = out[s];
            uint32_t S2 = 0;
#pragma unroll
            for (uint32_t t = 0; t < 5; ++t)
                if ((S >> t) & 1u) S2 |= (F >> (6u * t)) & 0x1Fu;
            if (!S2) {
                const int32_t at = atomicAdd(&a.ctl[2], 1);
                a.rerun[at] = ((uint32_t)key << 8) | s;
                a.rerun_init[at] = S << 1;  // back to state ids
                dead = true;
            }
            S = S2;
        }
        if (!dead) {
            seg_verdict(a, key, LC_VALID, LC_CAUSE_NONE, -1);
        }
    }
}

// The segment each dead key died in, searched again untagged from the states
// standing before it: the failing event.
__global__ __launch_bounds__(64) void k_seg_rerun(SegArgs a) {
    __shared__ uint32_t ws[3 * T0_RMEM * 64];
    const int32_t nr = a.ctl[2];
    for (int32_t guard = 0; guard <= nr; ++guard) {
        int32_t w = 0;
        if (lane_id() == 0) w = atomicAdd(&a.ctl[3], 1);
        w = __builtin_amdgcn_readfirstlane(w);
        if (w >= nr) break;
        const uint32_t item = a.rerun[w];
        const int32_t key = (int32_t)(item >> 8);
        const uint32_t s = item & 0xFFu;
        const uint32_t *ends = a.seg_end + (size_t)key * a.max_seg;
        int status;
        uint32_t fev, fin;
        segment_search<false>(a, key, ends[s - 1], ends[s], a.rerun_init[w], ws, status, fev, fin);
        if (status == 1) {
            if (lane_id() == 0) seg_verdict(a, key, LC_INVALID, LC_CAUSE_NONLIN, (int32_t)fev);
        } else {  // cannot happen for a consistent batch: report it as malformed
            if (lane_id() == 0) seg_verdict(a, key, LC_UNKNOWN, LC_CAUSE_ERROR, -1);
            t0_malformed(a, key, LC_BATCH_E_FIT);
        }
    }
}

hipError_t launch_segments(const SegArgs &a, int grid, hipStream_t s) {
    hipLaunchKernelGGL(k_seg_prep, dim3((unsigned)std::max(1, a.n_keys)), dim3(64), 0, s, a);
    hipLaunchKernelGGL(k_search_segments, dim3((unsigned)grid), dim3(64), 0, s, a);
    hipLaunchKernelGGL(k_seg_compose, dim3((unsigned)std::max(1, (a.n_keys + 255) / 256)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_seg_rerun, dim3(256), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace lcd
