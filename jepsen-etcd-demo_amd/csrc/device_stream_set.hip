// device_stream_set.hip -- the resident set tier of a stream (lc_stream_* with
// LC_STREAM_SET_TIER).
//
// A key whose next invoke would leave the register tier (k_stream,
// device_stream_lattice.hip: 10 ops pending, 32 states) is not restarted at
// lc_stream_finish: its lattice is written out once as a config set
// (k_stream_migrate) and from then on each call searches the key's new words
// from that set (k_stream_set), event by event as search_key_lds
// (device_search.hip) does: partition S on p, JIT closure I over the other
// pending ops, apply p, deduplicate in hash sets.  The set record's layout and
// the fallback rule are stream_plan.hpp's.
//
// Geometry.  k_stream_migrate: one wave per migrating key, no LDS.
// k_stream_set: one workgroup of 256 threads per key with new words, at most
// SET_GRID workgroups per launch.  S ping-pongs between the record's two
// arrays; I, both hash sets (2 x STREAM_SET_CAP slots each, load <= 1/2) and
// the positions their entries took live in a 1.5 MB workspace per resident
// workgroup in device memory -- no set of a key this far fits LDS -- and LDS
// holds ~0.8 KB of descriptors and counters.  The kernel needs few registers,
// so a CU could hold 8 such workgroups; the grid (<= 64 on 256 CUs) is what
// bounds residency, one workgroup per CU.
//
// Control is bounded: probe loops run at most one pass over their table,
// nothing waits on memory another workgroup writes, phases of an event are
// separated by __syncthreads, launches by their order on one HIP stream.

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/lincheck.h"
#include "device_common.hpp"
#include "device_search.hpp"
#include "stream_plan.hpp"

namespace lcd {

constexpr int SET_WG = 256;
constexpr uint32_t SET_CAP = lc::STREAM_SET_CAP;
constexpr uint32_t SET_HSLOTS = 2 * SET_CAP;
static_assert((SET_HSLOTS & (SET_HSLOTS - 1)) == 0, "hash slots: a power of two");

// reason bit of an ERROR beside LC_BATCH_E_*: a hash set took no more entries
constexpr uint32_t SET_E_TABLE = 8;

struct StreamSetShared {
    uint32_t desc[64];      // descriptor of the op pending in each window slot
    uint32_t slotlist[64];  // the :ok's closure candidates: slots, descriptors
    uint32_t desclist[64];
    uint32_t cnt[2];        // entries of S' / of I
    uint32_t err;
};

// Insert key into a hash set in device memory; true if it was not there.  At
// most one pass over the table (it is never more than half full).
__device__ __forceinline__ bool set_insert(uint64_t *tab, uint64_t key, bool active, uint32_t &pos, uint32_t *err) {
    bool isnew = false, done = !active;
    uint32_t h = hash64(key) & (SET_HSLOTS - 1);
    for (uint32_t t = 0; t < SET_HSLOTS && !done; ++t) {
        const unsigned long long old =
            atomicCAS((unsigned long long *)&tab[h], (unsigned long long)EMPTY, (unsigned long long)key);
        if (old == EMPTY) { isnew = true; done = true; }
        else if (old == key) { done = true; }
        else { h = (h + 1) & (SET_HSLOTS - 1); }
    }
    if (!done) atomicOr(err, 1u);
    pos = h;
    return isnew;
}

// Array position of this thread's new entry: one LDS add per wave.
__device__ __forceinline__ uint32_t set_reserve(uint32_t *ctr, bool flag) {
    const uint64_t m = __ballot(flag);
    uint32_t base = 0;
    if (lane_id() == 0 && m) base = atomicAdd(ctr, (uint32_t)__popcll(m));
    base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
    return base + rank_of(m);
}

__device__ __forceinline__ void set_report(const StreamSetArgs &a, int32_t key, uint32_t status, uint32_t fail, uint32_t why) {
    const uint32_t i = atomicAdd(&a.out[0], 1u);
    if (i < (uint32_t)a.n_items) {
        uint32_t *o = a.out + 1 + 4 * (size_t)i;
        o[0] = (uint32_t)key; o[1] = status; o[2] = fail; o[3] = why;
    }
}

// ---- migration ---------------------------------------------------------------
// Every set bit s of lattice word W[L] is the config (state s, ops L
// linearized and pending); op indices become window slots as write_final_mem
// (lattice_core.hpp) translates them.  The lattice may be closed over the
// pending ops or, when the record is dirty, closed over all but the ops
// invoked last: either is a set between S and its closure, which is all the
// search needs.
__device__ __forceinline__ void migrate_key(const StreamSetArgs &a, int32_t w) {
    using namespace lc;
    const uint32_t lane = lane_id();
    const StreamMigItem it = a.mig[w];
    const uint32_t *const r = a.rec + (size_t)it.key * STREAM_REC_WORDS;
    uint32_t *const sr = it.set_rec;
    uint64_t *const S0 = (uint64_t *)(sr + STREAM_SET_OFF_S0);
    const uint32_t hv = lane < STREAM_HDR_WORDS ? r[lane] : 0u;
    auto H = [&](uint32_t i) { return (uint32_t)__builtin_amdgcn_readlane((int)hv, (int)i); };
    uint32_t status = H(STREAM_H_STATUS);
    uint32_t nS = 0;
    if (status == STREAM_LIVE && !H(STREAM_H_STARTED)) {  // no event searched yet: the initial state
        if (lane == 0) S0[0] = (uint64_t)(a.init_state & 31u) << 56;
        nS = 1;
    } else if (status == STREAM_LIVE) {
        const uint32_t n0 = H(STREAM_H_N);
        const uint32_t n = n0 < STREAM_MAX_WIDTH ? n0 : STREAM_MAX_WIDTH;
        const uint32_t live = H(STREAM_H_LIVE) & ((1u << STREAM_MAX_WIDTH) - 1u);
        const uint32_t slot_v = r[STREAM_OFF_LANES + 3 * 64 + lane] & 63u;
        const uint32_t rows = stream_lattice_words(n) / 64;
        const uint32_t top = live ? 32u - (uint32_t)__clz(live) : 0u;
        uint64_t lo = 0;
        for (uint32_t j = 0; j < top && j < 6u; ++j) {
            const uint32_t sj = (uint32_t)__builtin_amdgcn_readlane((int)slot_v, (int)j);
            if (((lane & live) >> j) & 1u) lo |= 1ull << sj;
        }
        for (uint32_t k = 0; k < rows; ++k) {
            uint64_t hi = 0;
            for (uint32_t j = 6; j < top; ++j)
                if ((((k << 6) & live) >> j) & 1u) hi |= 1ull << (uint32_t)__builtin_amdgcn_readlane((int)slot_v, (int)j);
            const uint32_t wd = r[STREAM_OFF_LATTICE + k * 64 + lane];
            const uint64_t sm = lo | hi;
            for (uint32_t s = 0; s < STREAM_MAX_STATES; ++s) {
                const bool flag = (wd >> s) & 1u;
                const uint64_t m = __ballot(flag);
                const uint32_t pos = nS + rank_of(m);
                if (flag && pos < SET_CAP) S0[pos] = ((uint64_t)s << 56) | sm;
                nS += (uint32_t)__popcll(m);
            }
        }
        if (nS > SET_CAP) status = STREAM_SET_FALLBACK;  // (a lattice holds at most the cap)
    }
    uint32_t h = 0;
    h = lane == STREAM_SET_H_STATUS ? status : h;
    h = lane == STREAM_SET_H_NS ? nS : h;
    h = lane == STREAM_SET_H_PEND0 ? H(STREAM_H_PEND0) : h;
    h = lane == STREAM_SET_H_PEND1 ? H(STREAM_H_PEND1) : h;
    h = lane == STREAM_SET_H_DONE ? H(STREAM_H_DONE) : h;
    h = lane == STREAM_SET_H_FAIL ? H(STREAM_H_FAIL) : h;
    if (lane < STREAM_SET_HDR_WORDS) sr[lane] = h;
    sr[STREAM_SET_OFF_DESC + lane] = a.descs[it.desc_b + lane];
}

__global__ __launch_bounds__(64) void k_stream_migrate(StreamSetArgs a) {
    for (int32_t w = blockIdx.x; w < a.n_mig; w += gridDim.x) migrate_key(a, w);
}

// ---- the search ----------------------------------------------------------------
__device__ __forceinline__ void set_key(const StreamSetArgs &a, int32_t w, StreamSetShared &sh, char *ws) {
    using namespace lc;
    const uint32_t tid = threadIdx.x;
    const StreamSetItem it = a.items[w];
    uint32_t *const sr = it.set_rec;
    if (sr[STREAM_SET_H_STATUS] != STREAM_LIVE) return;  // it died in the register tier, in this very call
    const uint32_t nev = it.ev_e - it.ev_b;
    if (!nev) return;
    uint64_t *const Sa[2] = {(uint64_t *)(sr + STREAM_SET_OFF_S0), (uint64_t *)(sr + STREAM_SET_OFF_S1)};
    uint64_t *const I = (uint64_t *)(ws + a.ws.off_I);
    uint64_t *const hS = (uint64_t *)(ws + a.ws.off_hS);
    uint64_t *const hI = (uint64_t *)(ws + a.ws.off_hI);
    uint32_t *const pS = (uint32_t *)(ws + a.ws.off_pS);
    uint32_t *const pI = (uint32_t *)(ws + a.ws.off_pI);
    const uint32_t *const trp = a.trans + it.tr_b;
    const uint32_t *const evp = a.events32 + it.ev_b;

    uint32_t nS = sr[STREAM_SET_H_NS];
    nS = nS < SET_CAP ? nS : SET_CAP;
    uint64_t pending = (uint64_t)sr[STREAM_SET_H_PEND0] | (uint64_t)sr[STREAM_SET_H_PEND1] << 32;
    const uint32_t done = sr[STREAM_SET_H_DONE];
    uint32_t cur = sr[STREAM_SET_H_CUR] & 1u;
    if (tid < 64) sh.desc[tid] = sr[STREAM_SET_OFF_DESC + tid];
    if (tid == 0) sh.err = 0;
    __syncthreads();

    uint32_t status = STREAM_LIVE, fail = 0, why = 0;
    for (uint32_t i = 0; i < nev; ++i) {
        const uint32_t evi = evp[i];
        const uint32_t slot = LC_EV_SLOT(evi);
        if (!(evi & LC_EV_OK_BIT)) {  // :invoke
            if (slot >= STREAM_SET_MAX_SLOTS) { status = STREAM_SET_FALLBACK; fail = done + i; break; }
            if ((pending >> slot) & 1ull) { status = STREAM_ERROR; why = LC_BATCH_E_SLOTS; break; }
            if (LC_EV_TRANS(evi) >= it.ntr) { status = STREAM_ERROR; why = LC_BATCH_E_TRANS; break; }
            if (tid == 0) sh.desc[slot] = trp[LC_EV_TRANS(evi)];
            pending |= 1ull << slot;
            continue;
        }
        // ---- :ok of the op in `slot` ----
        if (slot >= STREAM_SET_MAX_SLOTS || !((pending >> slot) & 1ull)) { status = STREAM_ERROR; why = LC_BATCH_E_SLOTS; break; }
        const uint32_t p = slot;
        const uint64_t pbit = 1ull << p;
        if (tid == 0) { sh.cnt[0] = 0; sh.cnt[1] = 0; }
        __syncthreads();
        const uint32_t dp = sh.desc[p];
        const uint64_t *const S = Sa[cur];
        uint64_t *const Sn = Sa[cur ^ 1u];
        // -- partition S: p already linearized -> S' (p returns); else seed I
        for (uint32_t j = 0; j < nS; j += SET_WG) {
            const uint32_t idx = j + tid;
            const bool act = idx < nS;
            const uint64_t c = act ? S[idx] : 0;
            const bool hasp = act && (c & pbit);
            const bool toI = act && !hasp;
            uint32_t posa = 0, posb = 0;
            const bool ns = set_insert(hS, c & ~pbit, hasp, posa, &sh.err);
            const bool ni = set_insert(hI, c, toI, posb, &sh.err);
            const uint32_t ra = set_reserve(&sh.cnt[0], ns), rb = set_reserve(&sh.cnt[1], ni);
            if (ns) { Sn[ra] = c & ~pbit; pS[ra] = posa; }  // (at most nS <= the cap of them)
            if (ni) { I[rb] = c; pI[rb] = posb; }
        }
        // -- JIT closure over the other pending ops
        const uint64_t cand = pending & ~pbit;
        const uint32_t nc = (uint32_t)__popcll(cand);
        if (tid < 64 && ((cand >> tid) & 1ull)) {
            const uint32_t r = (uint32_t)__popcll(cand & ((1ull << tid) - 1ull));
            sh.slotlist[r] = tid;
            sh.desclist[r] = sh.desc[tid];
        }
        __syncthreads();
        uint32_t nI = sh.cnt[1];
        __syncthreads();
        bool overflow = false;
        uint32_t head = 0;
        while (nc && head < nI && !overflow) {
            const uint32_t end = nI;
            const uint32_t total = (end - head) * nc;
            for (uint32_t t0 = 0; t0 < total; t0 += SET_WG) {
                const uint32_t item = t0 + tid;
                bool act = item < total;
                const uint32_t ci = head + (act ? item / nc : 0u);
                const uint32_t k = act ? item % nc : 0u;
                const uint64_t c = I[ci];
                const uint32_t q = sh.slotlist[k];
                const uint32_t dq = sh.desclist[k];
                uint32_t s2 = 0;
                act = act && !((c >> q) & 1ull) && step(nullptr, (uint32_t)(c >> 56), dq, s2);
                const uint64_t c2 = ((uint64_t)s2 << 56) | (c & LMASK) | (1ull << q);
                uint32_t pos = 0;
                const bool nw = set_insert(hI, c2, act, pos, &sh.err);
                const uint32_t r = set_reserve(&sh.cnt[1], nw);
                if (nw) {
                    if (r < SET_CAP) { I[r] = c2; pI[r] = pos; }
                    else hI[pos] = EMPTY;  // past the cap: the key falls back, the table stays clean
                }
            }
            __syncthreads();
            nI = sh.cnt[1];
            __syncthreads();
            overflow = nI > SET_CAP;
            head = end;
        }
        // -- apply p to every config of the closure
        if (!overflow) {
            for (uint32_t j = 0; j < nI; j += SET_WG) {
                const uint32_t idx = j + tid;
                const uint64_t c = idx < nI ? I[idx] : 0;
                uint32_t s2 = 0;
                const bool act = idx < nI && step(nullptr, (uint32_t)(c >> 56), dp, s2);
                const uint64_t c2 = ((uint64_t)s2 << 56) | (c & LMASK);
                uint32_t pos = 0;
                const bool nw = set_insert(hS, c2, act, pos, &sh.err);
                const uint32_t r = set_reserve(&sh.cnt[0], nw);
                if (nw) {
                    if (r < SET_CAP) { Sn[r] = c2; pS[r] = pos; }
                    else hS[pos] = EMPTY;
                }
            }
        }
        __syncthreads();
        const uint32_t nSn = sh.cnt[0];
        // both hash sets empty again, by the entries they hold
        const uint32_t kS = nSn < SET_CAP ? nSn : SET_CAP, kI = nI < SET_CAP ? nI : SET_CAP;
        for (uint32_t j = tid; j < kS; j += SET_WG) hS[pS[j]] = EMPTY;
        for (uint32_t j = tid; j < kI; j += SET_WG) hI[pI[j]] = EMPTY;
        const bool table_full = sh.err != 0;
        __syncthreads();
        if (table_full) { status = STREAM_ERROR; why = SET_E_TABLE; break; }
        if (stream_set_falls_back(nSn, nI, 0, 0)) { status = STREAM_SET_FALLBACK; fail = done + i; break; }
        if (nSn == 0) { status = STREAM_INVALID; fail = done + i; break; }
        cur ^= 1u;
        nS = nSn;
        pending &= ~pbit;
    }
    __syncthreads();
    if (tid == 0) {
        sr[STREAM_SET_H_STATUS] = status;
        sr[STREAM_SET_H_NS] = nS;
        sr[STREAM_SET_H_PEND0] = (uint32_t)pending;
        sr[STREAM_SET_H_PEND1] = (uint32_t)(pending >> 32);
        sr[STREAM_SET_H_DONE] = status == STREAM_LIVE ? done + nev : status == STREAM_ERROR ? done : fail;
        sr[STREAM_SET_H_FAIL] = fail;
        sr[STREAM_SET_H_CUR] = cur;
        if (status != STREAM_LIVE) set_report(a, it.key, status, fail, why);
    }
    if (status == STREAM_LIVE && tid < 64) sr[STREAM_SET_OFF_DESC + tid] = sh.desc[tid];
    __syncthreads();
}

__global__ __launch_bounds__(SET_WG) void k_stream_set(StreamSetArgs a) {
    __shared__ StreamSetShared sh;
    char *const ws = a.ws.base + (size_t)blockIdx.x * a.ws.slot_bytes;
    for (int32_t w = blockIdx.x; w < a.n_items; w += gridDim.x) set_key(a, w, sh, ws);
}

StreamSetWs stream_set_ws_layout() {
    StreamSetWs w{};
    w.hmask = SET_HSLOTS - 1;
    w.off_I = 0;
    w.off_hS = w.off_I + (size_t)SET_CAP * 8;
    w.off_hI = w.off_hS + (size_t)SET_HSLOTS * 8;
    w.off_pS = w.off_hI + (size_t)SET_HSLOTS * 8;
    w.off_pI = w.off_pS + (size_t)SET_CAP * 4;
    w.slot_bytes = w.off_pI + (size_t)SET_CAP * 4;
    return w;
}

hipError_t launch_stream_migrate(const StreamSetArgs &a, int grid, hipStream_t s) {
    hipLaunchKernelGGL(k_stream_migrate, dim3(grid), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_stream_set(const StreamSetArgs &a, int grid, hipStream_t s) {
    hipLaunchKernelGGL(k_stream_set, dim3(grid), dim3(SET_WG), 0, s, a);
    return hipGetLastError();
}

}  // namespace lcd
