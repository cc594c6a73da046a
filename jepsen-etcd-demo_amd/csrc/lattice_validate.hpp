// lattice_validate.hpp -- the validation pass over a key's event words: the
// slot protocol by XOR scans, 64 events per pass.  k_validate
// (device_lattice.hip), k_spec's validation blocks (device_spec.hip) and the
// resident search (device_stream_lattice.hip) run it.  Device code: included
// by .hip files only.
#pragma once

#include "lattice_core.hpp"

namespace lcd {

// Inclusive XOR prefix over the wave's lanes (DPP row shifts, then the
// row broadcasts across the wave's four rows).
__device__ __forceinline__ uint32_t wave_xor_scan(uint32_t x) {
    x ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xF, 0xF, true);  // row_shr:1
    x ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xF, 0xF, true);  // row_shr:2
    x ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xF, 0xF, true);  // row_shr:4
    x ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xF, 0xF, true);  // row_shr:8
    x ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xA, 0xF, false);  // row_bcast:15 -> rows 1, 3
    x ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xC, 0xF, false);  // row_bcast:31 -> rows 2, 3
    return x;
}

// The slot protocol of one 64-event chunk, all slots at once: the events of a
// slot alternate :invoke, :ok, :invoke ... from its state at the chunk's
// start.  Each lane's slot as a one-hot bit over NW 32-bit words, XOR-scanned
// over the lanes: bit s of the exclusive prefix is the parity of slot s's
// earlier events in the chunk, so an event is an :ok exactly when its slot was
// pending at the chunk's start XOR that parity.  pend: the slots pending at
// the chunk's start (NW words, wave-uniform), updated to its end.  Returns
// whether any tracked lane breaks the protocol.
template <int NW>
__device__ __forceinline__ bool slot_protocol(bool tracked, bool ok, uint32_t s, uint32_t (&pend)[NW]) {
    const uint32_t q = s >> 5, bit = 1u << (s & 31u);
    uint32_t par = 0, b = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        const uint32_t oh = (tracked && q == (uint32_t)w) ? bit : 0u;
        const uint32_t x = wave_xor_scan(oh);
        par = q == (uint32_t)w ? (x ^ oh) : par;  // the exclusive prefix of the lane's word
        b = q == (uint32_t)w ? pend[w] : b;
        pend[w] ^= (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
    }
    const bool pending = (((par ^ b) & bit) != 0);
    return __any(tracked && ok != pending);
}

// Validation of a batch the host did not check event by event (T0_STRICT
// steps): a kernel of its own on a second stream, running beside the search
// (which stays in bounds on any input).  One wave per key, 64 events per
// pass: every transition id in range and installing only states the key
// has, every slot below 64, and the slot protocol (slot_protocol: one XOR
// scan per 32 slots and chunk, all slots at once).  Violations set the
// batch's error words (the call then returns LC_E_INVALID).
// GEN (a batch of any width whose events the host did not walk either):
// window slots up to 126, the slot-127 marker of ops beyond the encodable
// window exempt from the slot protocol (the search stops before it follows
// one), and every :invoke's slot below the key's key_width.
// One 64-event chunk of a key's validation (w: lane i holds event i of the
// chunk, in: it is one): transition ids, window slots, the slot protocol.
// Returns the LC_BATCH_E_* reasons found (0: none; pend is then advanced).
template <bool GEN, int NW>
__device__ __forceinline__ int32_t validate_chunk(uint32_t w, bool in, const uint32_t *trp, uint32_t ntr, uint32_t ns,
                                                  uint32_t width, uint32_t (&pend)[NW]) {
    int32_t why = 0;
    const bool ok = (w & LC_EV_OK_BIT) != 0;
    const uint32_t s = LC_EV_SLOT(w), t = LC_EV_TRANS(w);
    const uint32_t d = (in && !ok && t < ntr) ? trp[t] : 0u;
    if (__any(in && !ok && (t >= ntr || ((d & 3u) >= LC_T_WRITE && (d >> 17) >= ns)))) why |= LC_BATCH_E_TRANS;
    const bool beyond = GEN && s == 127u;  // past the encodable window: no slot to track
    if (__any(in && !beyond && (GEN ? (!ok && s >= width) : s >= 64u))) why |= LC_BATCH_E_FIT;
    if (why) return why;
    if (slot_protocol<NW>(in && !beyond, ok, s, pend)) why |= LC_BATCH_E_SLOTS;
    return why;
}

template <bool GEN, bool E16 = false>
__device__ __forceinline__ void validate_key(const T0Args &a, int64_t k) {
    const uint32_t lane = lane_id();
    if (a.key_error && a.key_error[k]) return;
    const uint64_t eb = a.ev_off[k], ee = a.ev_off[k + 1];
    const uint32_t tb = a.trans_off ? a.trans_off[k] : 0u;
    const uint32_t ntr = a.n_trans > tb ? a.n_trans - tb : 0u;
    const uint32_t ns = a.trans_off ? (a.key_states ? a.key_states[k] : 0u) : a.shared_states;
    const uint32_t width = GEN ? (a.key_width ? a.key_width[k] : 127u) : 64u;
    constexpr int NW = GEN ? 4 : 2;
    uint32_t pend[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) pend[w] = 0;
    int32_t why = 0;
    uint32_t w_next = lane < ee - eb ? (E16 ? LC_EV16_WIDE(a.events16[eb + lane]) : a.events[eb + lane]) : 0u;
    for (uint64_t base = eb; base < ee && !why; base += 64) {
        const uint64_t j = base + lane;
        const bool in = j < ee;
        const uint32_t w = w_next;
        const uint64_t jn = j + 64;
        w_next = jn < ee ? (E16 ? LC_EV16_WIDE(a.events16[jn]) : a.events[jn]) : 0u;  // the next chunk, in flight
        why = validate_chunk<GEN, NW>(w, in, a.trans + (ntr ? tb : 0u), ntr, ns, width, pend);
    }
    if (why && lane == 0) {
        atomicOr(&a.err[0], why);
        atomicMax(&a.err[1], a.err_base + (int32_t)k + 1);
    }
}

}  // namespace lcd
