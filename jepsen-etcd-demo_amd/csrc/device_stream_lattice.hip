// device_stream_lattice.hip -- the register tier's resident search (k_stream)
// of lc_stream_*.  Its host half: device_stream.hip; the set tier's kernels:
// device_stream_set.hip.

#include "lattice_core.hpp"
#include "lattice_validate.hpp"

namespace lcd {

// ---- A resident search (lc_stream_*) -------------------------------------------
//
// A history that is still being written is checked as it grows: each key's
// walk state lives in a record in device memory (stream_plan.hpp) between
// calls, and a call searches only the event words that are new.  One wave
// per key with new words: load the record, validate the new words with the
// slot-protocol words the record carries (the walk stays in bounds on any
// input, but its verdict over malformed words means nothing), resume the
// compact FAST walk where it stopped, store the record.  A key that died --
// its set empty at an :ok, or its words malformed -- stores its header alone
// and is appended to the launch's list; later launches leave it untouched.
// Nothing waits on anything: the host reads the list back after the launch.
__device__ __forceinline__ void stream_key(const StreamArgs &a, int32_t w, uint32_t *ws) {
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
            rs.dirty = H(STREAM_H_DIRTY) != 0;
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
        } else {  // a fresh record: the model's initial state, nothing pending
#pragma unroll
            for (int k = 0; k < T0_RSMALL; ++k) W[k] = 0u;
            if (lane == 0) W[0] = 1u << (a.init_state & 31u);
            rs.dirty = true;
        }
        LatWalk lw;
        lattice_walk<T0_RSMALL, true, false, EvSrc<true>, true>(W, lw, evp, nev, trp, it.ntr, 0u, m, ~0ull, false,
                                                                false, &rs);
        if (lw.status == 1) {
            status = STREAM_INVALID;
            fail = done + lw.fev;
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
    uint32_t h = 0;
    h = lane == STREAM_H_STATUS ? status : h;
    h = lane == STREAM_H_N ? rs.n : h;
    h = lane == STREAM_H_LIVE ? rs.live : h;
    h = lane == STREAM_H_IN_MEM ? (uint32_t)rs.in_mem : h;
    h = lane == STREAM_H_DIRTY ? (uint32_t)rs.dirty : h;
    h = lane == STREAM_H_DONE ? (status == STREAM_LIVE ? done + nev : status == STREAM_INVALID ? fail : done) : h;
    h = lane == STREAM_H_FAIL ? fail : h;
    h = lane == STREAM_H_PEND0 ? pend[0] : h;
    h = lane == STREAM_H_PEND1 ? pend[1] : h;
    h = lane == STREAM_H_STARTED ? 1u : h;
    if (lane < STREAM_HDR_WORDS) r[lane] = h;
    if (status != STREAM_LIVE && lane == 0) {
        const uint32_t i = atomicAdd(&a.out[0], 1u);
        if (i < (uint32_t)a.n_items) {
            uint32_t *o = a.out + 1 + 4 * (size_t)i;
            o[0] = (uint32_t)it.key; o[1] = status; o[2] = fail; o[3] = (uint32_t)why;
        }
    }
}

__global__ __launch_bounds__(64) void k_stream(StreamArgs a) {
    __shared__ uint32_t ws[3 * T0_RMEM * 64];  // lattices of 9-10 pending ops (12 KB)
    for (int32_t w = blockIdx.x; w < a.n_items; w += gridDim.x) stream_key(a, w, ws);
}

hipError_t launch_stream(const StreamArgs &a, int grid, hipStream_t s) {
    hipLaunchKernelGGL(k_stream, dim3(grid), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace lcd
