// device_stream_exact.hip -- the exact mode of a resident search
// (LC_STREAM_EXACT): k_stream_exact and k_stream_final.  The FAST form is
// device_stream_lattice.hip's k_stream; the host half is device_stream.hip.
// A translation unit of its own: which kernels share a module changes their
// register allocation.

#include "lattice_core.hpp"
#include "lattice_validate.hpp"

namespace lcd {

// ---- A resident search on Knossos's own sets ------------------------------------
//
// k_stream keeps closed supersets in the lane phase: enough for emptiness,
// nothing else.  Here a key's record holds the exact walk's state -- the same
// record without `dirty`, plus the running peak (STREAM_H_PEAK) -- so every
// set size is the oracle's: a budget of any size is honoured at the event the
// oracle names, and the set standing before a failing event is the one the
// one-shot check reports.  One wave per key with new words, as k_stream: load
// the record, validate the new words, resume the exact walk, store the record.
// A key that dies -- invalid, or past the budget -- writes that set's
// max_final smallest configs (write_final_mem) to the stream's own arrays,
// then its header, and goes on the launch's list.  Nothing waits on anything.

// write_final_mem's view of the stream's arrays (only these fields are read).
__device__ __forceinline__ Args final_args(const StreamExactArgs &a) {
    Args f{};
    f.final_cfg = a.final_cfg;
    f.n_final = a.n_final;
    f.max_final = a.max_final;
    return f;
}

__device__ __forceinline__ void stream_exact_key(const StreamExactArgs &a, int32_t w, uint32_t *ws) {
    using namespace lc;
    const uint32_t lane = lane_id();
    const LatMem m{ws, ws + T0_RMEM * 64, ws + 2 * T0_RMEM * 64};
    const StreamItem it = a.items[w];
    uint32_t *const r = a.rec + (size_t)it.key * STREAM_REC_WORDS;
    const uint32_t hv = lane < STREAM_HDR_WORDS ? r[lane] : 0u;
    auto H = [&](uint32_t i) { return (uint32_t)__builtin_amdgcn_readlane((int)hv, (int)i); };
    if (H(STREAM_H_STATUS) != STREAM_LIVE) return;  // dead: the record stays as it is
    const uint32_t nev = it.ev_e - it.ev_b;
    if (!nev) return;
    const uint32_t *const trp = a.trans + it.tr_b;
    const EvSrc<true> evp{a.events16 + it.ev_b};
    const uint32_t done = H(STREAM_H_DONE);

    uint32_t pend[2] = {H(STREAM_H_PEND0), H(STREAM_H_PEND1)};
    int32_t why = 0;
    for (uint32_t base = 0; base < nev && !why; base += 64) {
        const bool in = base + lane < nev;
        const uint32_t wd = in ? evp[base + lane] : 0u;
        why = validate_chunk<false, 2>(wd, in, trp, it.ntr, it.ns, 64u, pend);
    }

    uint32_t status = STREAM_LIVE, fail = 0;
    LatResume rs{};
    rs.peak = 1;
    if (why) {
        status = STREAM_ERROR;
    } else {
        uint32_t W[T0_RSMALL];
        uint32_t *const la = r + STREAM_OFF_LANES, *const lat = r + STREAM_OFF_LATTICE;
        if (H(STREAM_H_STARTED)) {
            const uint32_t n0 = H(STREAM_H_N);
            rs.n = n0 < T0_MAX_WIDTH ? n0 : T0_MAX_WIDTH;
            rs.live = H(STREAM_H_LIVE);
            rs.in_mem = stream_in_workspace(rs.n);
            rs.peak = H(STREAM_H_PEAK);
            rs.k_v = la[lane]; rs.cap_v = la[64 + lane]; rs.b_v = la[128 + lane];
            rs.slot_v = la[192 + lane]; rs.dense_v = la[256 + lane];
            const uint32_t rows = stream_lattice_words(rs.n) / 64;
            if (rs.in_mem) {
#pragma unroll
                for (int k = 0; k < T0_RMEM; ++k) m.W[k * 64 + lane] = (uint32_t)k < rows ? lat[k * 64 + lane] : 0u;
#pragma unroll
                for (int k = 0; k < T0_RSMALL; ++k) W[k] = 0u;
            } else {
#pragma unroll
                for (int k = 0; k < T0_RSMALL; ++k) W[k] = (uint32_t)k < rows ? lat[k * 64 + lane] : 0u;
            }
        } else {  // a fresh record: the model's initial state, nothing pending, a set of one
#pragma unroll
            for (int k = 0; k < T0_RSMALL; ++k) W[k] = 0u;
            if (lane == 0) W[0] = 1u << (a.init_state & 31u);
        }
        LatWalk lw;
        lattice_walk<T0_RSMALL, false, false, EvSrc<true>, true>(W, lw, evp, nev, trp, it.ntr, 0u, m, a.budget, true,
                                                                 false, &rs);
        if (lw.status == 1 || lw.status == 2) {
            // W / live hold the set before the failing event: that set's configs
            status = lw.status == 1 ? STREAM_INVALID : STREAM_BUDGET;
            fail = done + lw.fev;
            if (!lw.in_mem) {
#pragma unroll
                for (int k = 0; k < T0_RSMALL; ++k) m.W[k * 64 + lane] = W[k];
            }
            write_final_mem(final_args(a), it.key, m, lane, lw.slot_v, lw.live);
        } else if (lw.status) {  // more ops pending than the tier holds: the words lied about the key's width
            status = STREAM_ERROR;
            why = LC_BATCH_E_FIT;
        } else {
            la[lane] = rs.k_v; la[64 + lane] = rs.cap_v; la[128 + lane] = rs.b_v;
            la[192 + lane] = rs.slot_v; la[256 + lane] = rs.dense_v;
            const uint32_t rows = stream_lattice_words(rs.n) / 64;
            if (rs.in_mem) {
#pragma unroll
                for (int k = 0; k < T0_RMEM; ++k)
                    if ((uint32_t)k < rows) lat[k * 64 + lane] = m.W[k * 64 + lane];
            } else {
#pragma unroll
                for (int k = 0; k < T0_RSMALL; ++k)
                    if ((uint32_t)k < rows) lat[k * 64 + lane] = W[k];
            }
        }
    }
    const bool at_event = status == STREAM_INVALID || status == STREAM_BUDGET;
    uint32_t h = 0;
    h = lane == STREAM_H_STATUS ? status : h;
    h = lane == STREAM_H_N ? rs.n : h;
    h = lane == STREAM_H_LIVE ? rs.live : h;
    h = lane == STREAM_H_IN_MEM ? (uint32_t)rs.in_mem : h;
    h = lane == STREAM_H_DONE ? (status == STREAM_LIVE ? done + nev : at_event ? fail : done) : h;
    h = lane == STREAM_H_FAIL ? fail : h;
    h = lane == STREAM_H_PEND0 ? pend[0] : h;
    h = lane == STREAM_H_PEND1 ? pend[1] : h;
    h = lane == STREAM_H_STARTED ? 1u : h;
    h = lane == STREAM_H_PEAK ? rs.peak : h;
    if (lane < STREAM_HDR_WORDS) r[lane] = h;
    if (status != STREAM_LIVE && lane == 0) {
        const uint32_t i = atomicAdd(&a.out[0], 1u);
        if (i < (uint32_t)a.n_items) {
            uint32_t *o = a.out + 1 + 4 * (size_t)i;
            o[0] = (uint32_t)it.key; o[1] = status; o[2] = fail; o[3] = (uint32_t)why;
        }
    }
}

__global__ __launch_bounds__(64) void k_stream_exact(StreamExactArgs a) {
    __shared__ uint32_t ws[3 * T0_RMEM * 64];  // lattices of 9-10 pending ops (12 KB)
    for (int32_t w = blockIdx.x; w < a.n_items; w += gridDim.x) stream_exact_key(a, w, ws);
}

// lc_stream_finish: the end set of a key that is still live, from its record
// (a fresh record: the initial state alone).  Keys that died wrote theirs.
__global__ __launch_bounds__(64) void k_stream_final(StreamExactArgs a) {
    using namespace lc;
    __shared__ uint32_t ws[T0_RMEM * 64];
    const uint32_t lane = lane_id();
    const LatMem m{ws, ws, ws};
    for (int32_t w = blockIdx.x; w < a.n_items; w += gridDim.x) {
        const int32_t key = a.keys[w];
        const uint32_t *const r = a.rec + (size_t)key * STREAM_REC_WORDS;
        const uint32_t hv = lane < STREAM_HDR_WORDS ? r[lane] : 0u;
        auto H = [&](uint32_t i) { return (uint32_t)__builtin_amdgcn_readlane((int)hv, (int)i); };
        if (H(STREAM_H_STATUS) != STREAM_LIVE) continue;
        uint32_t slot_v = 0, live = 0;
        if (H(STREAM_H_STARTED)) {
            const uint32_t n0 = H(STREAM_H_N);
            const uint32_t rows = stream_lattice_words(n0 < T0_MAX_WIDTH ? n0 : T0_MAX_WIDTH) / 64;
            live = H(STREAM_H_LIVE) & ((1u << T0_MAX_WIDTH) - 1u);
            slot_v = r[STREAM_OFF_LANES + 192 + lane];
#pragma unroll
            for (int k = 0; k < T0_RMEM; ++k)
                m.W[k * 64 + lane] = (uint32_t)k < rows ? r[STREAM_OFF_LATTICE + k * 64 + lane] : 0u;
        } else {
#pragma unroll
            for (int k = 0; k < T0_RMEM; ++k) m.W[k * 64 + lane] = 0u;
            if (lane == 0) m.W[0] = 1u << (a.init_state & 31u);
        }
        write_final_mem(final_args(a), key, m, lane, slot_v, live);
    }
}

hipError_t launch_stream_exact(const StreamExactArgs &a, int grid, hipStream_t s) {
    hipLaunchKernelGGL(k_stream_exact, dim3(grid), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_stream_final(const StreamExactArgs &a, int grid, hipStream_t s) {
    hipLaunchKernelGGL(k_stream_final, dim3(grid), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace lcd
