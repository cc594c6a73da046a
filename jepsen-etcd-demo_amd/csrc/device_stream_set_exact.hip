// device_stream_set_exact.hip -- the exact mode of a stream's resident set tier
// (LC_STREAM_EXACT | LC_STREAM_SET_TIER):
// k_stream_set_exact and k_stream_set_final.  The plain form is
// device_stream_set.hip's k_stream_set; the host half is device_stream.hip.  A
// translation unit of its own, as device_stream_exact.hip is: which kernels
// share a module changes their register allocation.
//
// An exact register record (k_stream_exact) holds Knossos's own S, so
// k_stream_migrate writes out S itself, and k_stream_set's step -- partition on
// p, JIT closure, apply p -- is the oracle's.  Every |I| and |S'| here is then
// the oracle's, and what this unit adds is the accounting: the sizes against the
// context's budget in the oracle's order (stream_plan.hpp
// stream_set_exact_decide), the running peak (in the key's register record's
// STREAM_H_PEAK, which the key's time in the register tier left there), and
// the final configs of a key that dies at an event: the max_final smallest of
// the set standing before it, in (slot mask, state id) order.
//
// Geometry: k_stream_set's.  One workgroup of 256 threads per key with new
// words, at most 64 per launch, the same workspace, 32-bit event words; ~0.8 KB
// of LDS.  k_stream_set_final: one workgroup per set-tier key still live.
// Control is bounded as in k_stream_set: nothing waits on another workgroup.

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/lincheck.h"
#include "device_common.hpp"
#include "device_search.hpp"
#include "stream_plan.hpp"

namespace lcd {
namespace {

constexpr int SETX_WG = 256;
constexpr uint32_t SETX_CAP = lc::STREAM_SET_CAP;
constexpr uint32_t SETX_HSLOTS = 2 * SETX_CAP;  // stream_set_ws_layout's tables
static_assert((SETX_HSLOTS & (SETX_HSLOTS - 1)) == 0, "hash slots: a power of two");

// reason bit of an ERROR beside LC_BATCH_E_*: a hash set took no more entries
constexpr uint32_t SETX_E_TABLE = 8;

struct StreamSetExactShared {
    uint32_t desc[64];      // descriptor of the op pending in each window slot
    uint32_t slotlist[64];  // the :ok's closure candidates: slots, descriptors
    uint32_t desclist[64];
    uint32_t cnt[2];        // entries of S' / of I
    uint32_t err;
    uint64_t wmin[SETX_WG / 64];  // the final configs' selection: one minimum per wave
};

// Insert key into a hash set in device memory; true if it was not there.  At
// most one pass over the table (it is never more than half full).
__device__ __forceinline__ bool setx_insert(uint64_t *tab, uint64_t key, bool active, uint32_t &pos, uint32_t *err) {
    bool isnew = false, done = !active;
    uint32_t h = hash64(key) & (SETX_HSLOTS - 1);
    for (uint32_t t = 0; t < SETX_HSLOTS && !done; ++t) {
        const unsigned long long old =
            atomicCAS((unsigned long long *)&tab[h], (unsigned long long)EMPTY, (unsigned long long)key);
        if (old == EMPTY) { isnew = true; done = true; }
        else if (old == key) { done = true; }
        else { h = (h + 1) & (SETX_HSLOTS - 1); }
    }
    if (!done) atomicOr(err, 1u);
    pos = h;
    return isnew;
}

// Array position of this thread's new entry: one LDS add per wave.
__device__ __forceinline__ uint32_t setx_reserve(uint32_t *ctr, bool flag) {
    const uint64_t m = __ballot(flag);
    uint32_t base = 0;
    if (lane_id() == 0 && m) base = atomicAdd(ctr, (uint32_t)__popcll(m));
    base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
    return base + rank_of(m);
}

// The max_final smallest configs of S[0 .. nS) in (slot mask, state id) order
// into the stream's arrays, in write_final_mem's record form, and their count.
// max_final rounds of a workgroup minimum over the sort keys above the last one
// taken: a wave reduction, then one LDS word per wave.  nS is uniform.
__device__ __forceinline__ void setx_write_final(const StreamSetExactArgs &a, int32_t key, const uint64_t *S, uint32_t nS,
                                                 uint64_t *wmin) {
    using namespace lc;
    if (!a.final_cfg) return;
    const uint32_t tid = threadIdx.x;
    const uint32_t mf = a.max_final > 0 ? (uint32_t)a.max_final : 0u;
    const uint32_t nw = nS < mf ? nS : mf;
    uint64_t lo = 0;  // sort keys below it are taken
    for (uint32_t r = 0; r < nw; ++r) {
        uint64_t mn = ~0ull;
        for (uint32_t j = tid; j < nS; j += SETX_WG) {
            const uint64_t k = stream_set_sort_key(S[j]);
            mn = k >= lo && k < mn ? k : mn;
        }
        for (int o = 32; o >= 1; o >>= 1) {
            const uint32_t l2 = (uint32_t)__shfl_xor((int)(uint32_t)mn, o), h2 = (uint32_t)__shfl_xor((int)(uint32_t)(mn >> 32), o);
            const uint64_t v = ((uint64_t)h2 << 32) | l2;
            mn = v < mn ? v : mn;
        }
        if (lane_id() == 0) wmin[tid >> 6] = mn;
        __syncthreads();
#pragma unroll
        for (int wv = 0; wv < SETX_WG / 64; ++wv) mn = wmin[wv] < mn ? wmin[wv] : mn;
        __syncthreads();
        if (tid == 0) {
            const uint64_t c = stream_set_sort_key_cfg(mn);
            uint64_t *const o = a.final_cfg + stream_final_off64((uint64_t)key, mf, r);
            o[0] = c & LMASK;
            o[1] = (c >> 56) << 48;
        }
        lo = mn + 1;
    }
    if (tid == 0 && a.n_final) a.n_final[key] = nw;
}

__device__ __forceinline__ void setx_report(const StreamSetArgs &a, int32_t key, uint32_t status, uint32_t fail, uint32_t why) {
    const uint32_t i = atomicAdd(&a.out[0], 1u);
    if (i < (uint32_t)a.n_items) {
        uint32_t *o = a.out + 1 + 4 * (size_t)i;
        o[0] = (uint32_t)key; o[1] = status; o[2] = fail; o[3] = why;
    }
}

// k_stream_set's set_key with the oracle's accounting.
__device__ __forceinline__ void setx_key(const StreamSetExactArgs &x, int32_t w, StreamSetExactShared &sh, char *ws) {
    using namespace lc;
    const StreamSetArgs &a = x.set;
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
    uint32_t *const peakp = x.rec + (size_t)it.key * STREAM_REC_WORDS + STREAM_H_PEAK;

    uint32_t nS = sr[STREAM_SET_H_NS];
    nS = nS < SETX_CAP ? nS : SETX_CAP;
    uint64_t pending = (uint64_t)sr[STREAM_SET_H_PEND0] | (uint64_t)sr[STREAM_SET_H_PEND1] << 32;
    const uint32_t done = sr[STREAM_SET_H_DONE];
    uint32_t cur = sr[STREAM_SET_H_CUR] & 1u;
    uint32_t peak = *peakp;
    peak = peak ? peak : 1u;  // a fresh record counts as 1
    const uint32_t stop = stream_set_closure_stop(x.budget);
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
        for (uint32_t j = 0; j < nS; j += SETX_WG) {
            const uint32_t idx = j + tid;
            const bool act = idx < nS;
            const uint64_t c = act ? S[idx] : 0;
            const bool hasp = act && (c & pbit);
            const bool toI = act && !hasp;
            uint32_t posa = 0, posb = 0;
            const bool ns = setx_insert(hS, c & ~pbit, hasp, posa, &sh.err);
            const bool ni = setx_insert(hI, c, toI, posb, &sh.err);
            const uint32_t ra = setx_reserve(&sh.cnt[0], ns), rb = setx_reserve(&sh.cnt[1], ni);
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
        bool overflow = false;  // |I| is past the budget or the cap: the event is decided
        uint32_t head = 0;
        while (nc && head < nI && !overflow) {
            const uint32_t end = nI;
            const uint32_t total = (end - head) * nc;
            for (uint32_t t0 = 0; t0 < total; t0 += SETX_WG) {
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
                const bool nw = setx_insert(hI, c2, act, pos, &sh.err);
                const uint32_t r = setx_reserve(&sh.cnt[1], nw);
                if (nw) {
                    if (r < SETX_CAP) { I[r] = c2; pI[r] = pos; }
                    else hI[pos] = EMPTY;  // past the cap: the table stays clean
                }
            }
            __syncthreads();
            nI = sh.cnt[1];
            __syncthreads();
            overflow = nI > stop;
            head = end;
        }
        // -- apply p to every config of the closure
        if (!overflow) {
            for (uint32_t j = 0; j < nI; j += SETX_WG) {
                const uint32_t idx = j + tid;
                const uint64_t c = idx < nI ? I[idx] : 0;
                uint32_t s2 = 0;
                const bool act = idx < nI && step(nullptr, (uint32_t)(c >> 56), dp, s2);
                const uint64_t c2 = ((uint64_t)s2 << 56) | (c & LMASK);
                uint32_t pos = 0;
                const bool nw = setx_insert(hS, c2, act, pos, &sh.err);
                const uint32_t r = setx_reserve(&sh.cnt[0], nw);
                if (nw) {
                    if (r < SETX_CAP) { Sn[r] = c2; pS[r] = pos; }
                    else hS[pos] = EMPTY;
                }
            }
        }
        __syncthreads();
        const uint32_t nSn = sh.cnt[0];
        // both hash sets empty again, by the entries they hold
        const uint32_t kS = nSn < SETX_CAP ? nSn : SETX_CAP, kI = nI < SETX_CAP ? nI : SETX_CAP;
        for (uint32_t j = tid; j < kS; j += SETX_WG) hS[pS[j]] = EMPTY;
        for (uint32_t j = tid; j < kI; j += SETX_WG) hI[pI[j]] = EMPTY;
        const bool table_full = sh.err != 0;
        __syncthreads();
        const uint32_t dec =
            stream_set_exact_decide(table_full, stream_set_exact_count(nI), stream_set_exact_count(nSn), x.budget);
        if (dec != STREAM_LIVE) {
            status = dec;
            if (dec == STREAM_ERROR) why = SETX_E_TABLE;
            else fail = done + i;
            break;
        }
        cur ^= 1u;
        nS = nSn;
        peak = nSn > peak ? nSn : peak;
        pending &= ~pbit;
    }
    __syncthreads();
    // S (the current array) is the set standing before the failing event: the partition only read it
    if (status == STREAM_INVALID || status == STREAM_BUDGET) setx_write_final(x, it.key, Sa[cur], nS, sh.wmin);
    if (tid == 0) {
        sr[STREAM_SET_H_STATUS] = status;
        sr[STREAM_SET_H_NS] = nS;
        sr[STREAM_SET_H_PEND0] = (uint32_t)pending;
        sr[STREAM_SET_H_PEND1] = (uint32_t)(pending >> 32);
        sr[STREAM_SET_H_DONE] = status == STREAM_LIVE ? done + nev : status == STREAM_ERROR ? done : fail;
        sr[STREAM_SET_H_FAIL] = fail;
        sr[STREAM_SET_H_CUR] = cur;
        *peakp = peak;
        if (status != STREAM_LIVE) setx_report(a, it.key, status, fail, why);
    }
    if (status == STREAM_LIVE && tid < 64) sr[STREAM_SET_OFF_DESC + tid] = sh.desc[tid];
    __syncthreads();
}

}  // namespace

__global__ __launch_bounds__(SETX_WG) void k_stream_set_exact(StreamSetExactArgs a) {
    __shared__ StreamSetExactShared sh;
    char *const ws = a.set.ws.base + (size_t)blockIdx.x * a.set.ws.slot_bytes;
    for (int32_t w = blockIdx.x; w < a.set.n_items; w += gridDim.x) setx_key(a, w, sh, ws);
}

// lc_stream_finish: the end set of a set-tier key that is still live, from its
// set record.  Keys that died wrote theirs; keys that fell back get theirs
// from the batch path.
__global__ __launch_bounds__(SETX_WG) void k_stream_set_final(StreamSetExactArgs a) {
    using namespace lc;
    __shared__ uint64_t wmin[SETX_WG / 64];
    for (int32_t w = blockIdx.x; w < a.set.n_items; w += gridDim.x) {
        const StreamSetItem it = a.set.items[w];
        const uint32_t *const sr = it.set_rec;
        if (sr[STREAM_SET_H_STATUS] != STREAM_LIVE) continue;
        const uint32_t n0 = sr[STREAM_SET_H_NS];
        const uint32_t nS = n0 < SETX_CAP ? n0 : SETX_CAP;
        const uint64_t *const S = (const uint64_t *)(sr + stream_set_off_s(sr[STREAM_SET_H_CUR] & 1u));
        setx_write_final(a, it.key, S, nS, wmin);
    }
}

hipError_t launch_stream_set_exact(const StreamSetExactArgs &a, int grid, hipStream_t s) {
    hipLaunchKernelGGL(k_stream_set_exact, dim3(grid), dim3(SETX_WG), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_stream_set_final(const StreamSetExactArgs &a, int grid, hipStream_t s) {
    hipLaunchKernelGGL(k_stream_set_final, dim3(grid), dim3(SETX_WG), 0, s, a);
    return hipGetLastError();
}

}  // namespace lcd
