// lattice_core.hpp -- T0: the JIT linearization search with the config set
// held as a subset lattice in registers (one wavefront per key).
//
// Same sets as every other tier (semantics: oracle/linear_ref.py).  The
// representation exploits two facts of the packed form:
//   * a config is (register state, set L of linearized pending ops), and the
//     pending ops are numbered densely 0..n-1 (n = ops pending; when op j
//     returns, op n-1 takes number j), so L is a subset of {0 .. n-1} and
//     n <= the key's concurrency (10 for the demo's 10 client threads);
//   * the register has few states (6 for the demo's values 0..4 + nil).
// So S is stored as W[L] = bitmask of states s with (s, L) in S, one 32-bit
// mask per subset L, subset index = lane + 64 * register.
//
// Per :ok(p) event:
//   Ret[L]  = W[L u {p}]              (configs that already linearized p)
//   I[L]    = W[L]          for p not in L; then the JIT closure
//   I[L u {q}] |= T_q(I[L]) for every pending q != p, to a fixpoint,
//   S'[L]   = Ret[L] | T_p(I[L])
// where T_q maps a state mask through op q's cas-register step, branch-free:
//   T(M) = min(M & k, cap) << b
//   (k = the states the op accepts, cap = ~0 for reads (T(M) = M & k, b = 0)
//    and 1 for writes / cas (T(M) = {b} if M & k is not empty):
//    read nil: k = all; read a: k = {a}; write b: k = all, cap = 1;
//    cas a->b: k = {a}, cap = 1).
// The closure runs as Gauss-Seidel sweeps over the subset-bit positions:
// lanes (subsets) WITH bit q gather I from the subset without it -- one
// DPP / permlane instruction for a lane bit, a register for a register bit --
// and positions are applied in place, so one sweep follows every path that
// adds ops in increasing index order.  A sweep that changes nothing ends the
// closure, and n - 1 sweeps always suffice (a path has at most n - 1 steps).
// Accept masks are lane-masked once per event (zero on lanes without bit q
// and for q = p), so a sweep position is 3 VALU instructions (v_and_b32_dpp
// with the gather folded in, v_min_u32, v_lshl_or_b32).
//
// Set sizes (budget, peak) are wave popcount reductions and the probe count
// (LC_OPT_COUNT_PROBES) is accumulated per lane, so every number reported
// equals the oracle's.  Keys outside T0's reach (more than 10 ops pending,
// more than 32 register states) go to the hash-set tiers.
//
// This header is the register lattice itself -- transfers, gathers, the :ok
// steps, the event walk (lattice_walk) and the unsegmented key (lattice_key) --
// as inlined device code; the kernels built on it are in device_lattice.hip
// (unsegmented tier), device_segments.hip, device_spec.hip and
// device_stream_lattice.hip.  Device code: included by .hip files only.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include <algorithm>
#include <cstdint>

#include "../../include/lincheck.h"
#include "device_common.hpp"
#include "device_search.hpp"
#include "stream_plan.hpp"

extern "C" __device__ uint32_t __ockl_wfred_add_u32(uint32_t);
extern "C" __device__ int32_t __ockl_wfred_add_i32(int32_t);
extern "C" __device__ uint32_t __ockl_wfred_min_u32(uint32_t);
extern "C" __device__ uint32_t __ockl_wfred_xor_u32(uint32_t);

namespace lcd {

// Lattice registers per lane: the compact build holds n <= 8 pending ops in
// 4 registers (9-10 in the LDS workspace) and fits 4 waves per SIMD; the
// wide build holds n <= 10 in 16 registers (2 waves per SIMD) and is used
// when every key can be resident at once (launch_t0).
constexpr int T0_RSMALL = 4, T0_RBIG = 16;
constexpr int T0_RMEM = 16;            // workspace lattice (global memory): n <= 10
#ifndef LC_T0_MAX_WIDTH
#define LC_T0_MAX_WIDTH 10
#endif
constexpr uint32_t T0_MAX_WIDTH = LC_T0_MAX_WIDTH;  // <= 6 + log2(T0_RMEM)
constexpr uint32_t T0_MAX_STATES = 32;

struct Xfer { uint32_t k, cap, b, m; };

// A key's event words as the register tier reads them: the 32-bit form, or
// the 16-bit form lc_pack emits when every word fits (lc_batch.events16,
// LC_EV16_WIDE), read in place -- half the bytes per event and no widening
// pass over the batch before the search.
template <bool E16> struct EvSrc;
template <> struct EvSrc<false> {
    const uint32_t *p;
    __device__ __forceinline__ uint32_t operator[](uint64_t j) const { return p[j]; }
    __device__ __forceinline__ EvSrc operator+(uint64_t o) const { return {p + o}; }
};
template <> struct EvSrc<true> {
    const uint16_t *p;
    __device__ __forceinline__ uint32_t operator[](uint64_t j) const { return LC_EV16_WIDE(p[j]); }
    __device__ __forceinline__ EvSrc operator+(uint64_t o) const { return {p + o}; }
};
// A key's 16-bit event words staged in its workgroup's LDS (k_spec): the
// first n_lds words from there, the rest from HBM.  The cut search, every
// segment's TOP walk and its verifying run then read HBM once between them.
// (The LDS copy is held as an LDS-typed pointer: a generic one made every
// read a select between the two pointers and a flat load, waited on for both
// counters at once -- C2 / C5 / C3-shard times equal either way, tools/
// gpu_r4s.sh, but the window refill is a ds_read again.)
using LdsU16 = __attribute__((address_space(3))) const uint16_t;
struct EvStaged {
    LdsU16 *l;          // the LDS copy
    const uint16_t *g;  // the words in HBM
    uint32_t n_lds;
    __device__ __forceinline__ uint32_t operator[](uint64_t j) const {
        uint32_t w;
        if (j < n_lds) w = l[j];
        else w = g[j];
        return LC_EV16_WIDE(w);
    }
    __device__ __forceinline__ EvStaged operator+(uint64_t o) const {
        return {l + o, g + o, n_lds > o ? n_lds - (uint32_t)o : 0u};
    }
};

__device__ __forceinline__ Xfer xfer_of(uint32_t d) {
    const uint32_t f = d & 3u, a = (d >> 2) & 0x7FFFu, b = d >> 17;
    const uint32_t abit = a < 32u ? 1u << (a & 31u) : 0u;
    Xfer x;
    x.k = (f == LC_T_READ || f == LC_T_CAS) ? abit : 0xFFFFFFFFu;
    x.cap = f >= LC_T_WRITE ? 1u : 0xFFFFFFFFu;
    x.b = f >= LC_T_WRITE ? (b & 31u) : 0u;
    x.m = ~0u;
    return x;
}

// Tagged transfers (key segments, see k_search_segments): the lattice word
// holds 5 groups of 6 bits, group t = the states reachable from initial
// state t + 1 (register states 1..5, bit s - 1 of a group; bit 5 spare, 0).
// An op's transfer on a word is
//   T(M) = (((M & K) + C) >> s) & Mb
// with K = the accepted states in every group, and for a write / cas of
// state b: C = 31 in every group (a nonempty group carries into its bit 5),
// s = 6 - b (that bit lands on bit b - 1), Mb = bit b - 1 in every group;
// for a read C = 0, s = 0, Mb = ~0 (T(M) = M & K).  K = 0 gives 0 in every
// case (31 >> s never reaches bit b - 1), as the untagged form's does.
constexpr uint32_t TAG_REP = 0x1041041u;  // 1 in each 6-bit group
constexpr uint32_t TAG_ID = 0x10204081u;  // group t holds state t + 1: the identity start

__device__ __forceinline__ Xfer xfer_tag(uint32_t d) {
    const uint32_t f = d & 3u, a = (d >> 2) & 0x7FFFu, b = d >> 17;
    const uint32_t abit = (a >= 1u && a <= 5u) ? 1u << (a - 1u) : 0u;
    Xfer x;
    x.k = (f == LC_T_READ || f == LC_T_CAS) ? abit * TAG_REP : 0x1Fu * TAG_REP;
    const bool inst = f >= LC_T_WRITE && b >= 1u && b <= 5u;
    x.cap = inst ? 31u * TAG_REP : 0u;            // C
    x.b = inst ? 6u - b : 0u;                     // s
    x.m = inst ? (1u << (b - 1u)) * TAG_REP : ~0u;  // Mb
    if (f >= LC_T_WRITE && !inst) x.k = 0u;       // installs a state outside the tags: never taken
    return x;
}

// v with lane l (uniform, < 64) set to x: one v_writelane_b32.  Written as
// `lane == l ? x : v` the compiler masks EXEC around a move per value.
extern "C" __device__ int lc_writelane(int x, int l, int v) __asm("llvm.amdgcn.writelane.i32");
__device__ __forceinline__ uint32_t setl(uint32_t v, uint32_t l, uint32_t x) {
    return (uint32_t)lc_writelane((int)x, (int)l, (int)v);
}

// x from lane (lane ^ 2^q), q < 6 uniform: one ds_bpermute on an address
// (lane * 4) ^ (4 << q).  __shfl_xor adds a width check (a compare and a
// select) and the shift of the lane index on every call.
__device__ __forceinline__ uint32_t xor_lane(uint32_t x, uint32_t q, uint32_t lane) {
    return (uint32_t)__builtin_amdgcn_ds_bpermute((int)((lane << 2) ^ (4u << q)), (int)x);
}

// s & v as one v_and_b32 (kept opaque: the compiler would turn an AND with a
// 0/~0 lane mask into a select through an SGPR pair)
__device__ __forceinline__ uint32_t vand(uint32_t s, uint32_t v) {
    uint32_t r;
    asm("v_and_b32 %0, %1, %2" : "=v"(r) : "s"(s), "v"(v));
    return r;
}

// acc | T(x) = acc | (min(x & k, cap) << b): v_and_b32, v_min_u32, v_lshl_or_b32
// (tagged: acc | ((((x & K) + C) >> s) & Mb): v_and, v_add, v_lshrrev, v_and_or)
template <bool TAG = false>
__device__ __forceinline__ uint32_t xacc(uint32_t acc, uint32_t x, uint32_t k, uint32_t cap, uint32_t b,
                                         uint32_t mb = ~0u) {
    if constexpr (TAG) return ((((x & k) + cap) >> b) & mb) | acc;
    else return (__builtin_elementwise_min(x & k, cap) << b) | acc;
}

// One-directional gathers along subset bit q < 6 (a lane-index bit):
//   gdown<q>(x)[L] = x[L - 2^q]   (meaningful on lanes WITH bit q)
//   gup<q>(x)[L]   = x[L + 2^q]   (meaningful on lanes WITHOUT bit q)
// One VALU instruction each: DPP quad_perm (q = 0, 1), DPP row_shr / row_shl
// (q = 2, 3; lanes whose source leaves the row read 0), gfx950
// v_permlane16_swap / v_permlane32_swap (q = 4, 5; the other half of the
// lanes reads garbage, which every caller masks).
// A DPP move whose lanes without a source read 0 (bound_ctrl) is written as
// update_dpp(0, x), so the compiler folds it into the single VALU op that
// consumes it (v_and_b32_dpp in a sweep).
template <int CTRL>
__device__ __forceinline__ uint32_t dpp0(uint32_t x) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xF, 0xF, true);
}
template <int Q>
__device__ __forceinline__ uint32_t gdown(uint32_t x) {
    if constexpr (Q == 0) return dpp0<0xA0>(x);        // quad_perm [0,0,2,2]
    else if constexpr (Q == 1) return dpp0<0x44>(x);   // quad_perm [0,1,0,1]
    else if constexpr (Q == 2) return dpp0<0x114>(x);  // row_shr:4
    else if constexpr (Q == 3) return dpp0<0x118>(x);  // row_shr:8
    else if constexpr (Q == 4) return __builtin_amdgcn_permlane16_swap(x, x, false, false)[0];
    else return __builtin_amdgcn_permlane32_swap(x, x, false, false)[0];
}
// gdown with a dead register as the permlane's other operand: the swap
// clobbers both, so this saves one copy of x
template <int Q>
__device__ __forceinline__ uint32_t gdown_j(uint32_t x, uint32_t junk) {
    if constexpr (Q == 4) return __builtin_amdgcn_permlane16_swap(junk, x, false, false)[0];
    else if constexpr (Q == 5) return __builtin_amdgcn_permlane32_swap(junk, x, false, false)[0];
    else return gdown<Q>(x);
}
template <int Q>
__device__ __forceinline__ uint32_t gup(uint32_t x) {
    if constexpr (Q == 0) return dpp0<0xF5>(x);        // quad_perm [1,1,3,3]
    else if constexpr (Q == 1) return dpp0<0xEE>(x);   // quad_perm [2,3,2,3]
    else if constexpr (Q == 2) return dpp0<0x104>(x);  // row_shl:4
    else if constexpr (Q == 3) return dpp0<0x108>(x);  // row_shl:8
    else if constexpr (Q == 4) return __builtin_amdgcn_permlane16_swap(x, x, false, false)[1];
    else return __builtin_amdgcn_permlane32_swap(x, x, false, false)[1];
}
// Run-time bit (uniform q < 6): a scalar branch to one of the above.
__device__ __forceinline__ uint32_t gdown_rt(uint32_t x, uint32_t q) {
    switch (q) {
        case 0: return gdown<0>(x);
        case 1: return gdown<1>(x);
        case 2: return gdown<2>(x);
        case 3: return gdown<3>(x);
        case 4: return gdown<4>(x);
        default: return gdown<5>(x);
    }
}
__device__ __forceinline__ uint32_t gup_rt(uint32_t x, uint32_t q) {
    switch (q) {
        case 0: return gup<0>(x);
        case 1: return gup<1>(x);
        case 2: return gup<2>(x);
        case 3: return gup<3>(x);
        case 4: return gup<4>(x);
        default: return gup<5>(x);
    }
}

// x from lane (lane ^ 2^Q), both directions (workspace path).  Both gathers
// are evaluated unconditionally: a cross-lane op written inside `c ? a : b`
// would run under a divergent EXEC mask and read inactive source lanes.
template <int Q>
__device__ __forceinline__ uint32_t xv(uint32_t x, uint32_t lane) {
    const uint32_t d = gdown<Q>(x), u = gup<Q>(x);
    return ((lane >> Q) & 1u) ? d : u;
}

template <bool TAG = false>
__device__ __forceinline__ uint32_t xapply(uint32_t M, uint32_t k, uint32_t cap, uint32_t b, uint32_t mb = ~0u) {
    if constexpr (TAG) return (((M & k) + cap) >> b) & mb;
    else return __builtin_elementwise_min(M & k, cap) << b;
}

__device__ __forceinline__ bool idx_has(uint32_t lane, int k, uint32_t q) {
    return q < 6 ? ((lane >> q) & 1u) : (((uint32_t)k >> (q - 6)) & 1u);
}

template <int RL>
constexpr int lat_bits() { return RL == 1 ? 6 : RL == 2 ? 7 : RL == 4 ? 8 : RL == 8 ? 9 : 10; }

using Lat = uint32_t[T0_RBIG];

// T0's kernel arguments: only what the event loop reads, so the loop keeps
// its scalar registers (the full Args would spill SGPRs into VGPR lanes).
constexpr uint32_t T0_COUNT = 1, T0_WANT_PEAK = 2, T0_DBG_NOEVENTS = 4, T0_DBG_NOFINAL = 8, T0_WANT_FINAL = 16;
// T0_STRICT: the host skipped its per-event validation (a T0-only step: every
// key declared to fit the lattice).  T0 then checks the event stream itself
// as it walks it, and a key that would leave T0 is an error, not a spill (no
// later tier is launched to take it).
constexpr uint32_t T0_STRICT = 32;
// k_spec: cuts at equal estimated cost (spec_targets_cost) instead of equal
// event counts
constexpr uint32_t T0_SPEC_COST = 64;
// k_spec: TOP walks leave issue priority to age alone (no progress priority)
constexpr uint32_t T0_SPEC_NOPRIO = 128;
// k_spec: the T0_STRICT validation blocks come first in the grid (batches of
// more keys than the chip holds at once: dispatched last, they would run
// after the last round of keys, alone)
constexpr uint32_t T0_SPEC_VFIRST = 256;
// k_spec: events read from HBM, not staged in LDS (A/B)
constexpr uint32_t T0_SPEC_NOSTAGE = 512;
struct T0Args {
    const uint64_t *ev_off;
    const uint32_t *events;
    const uint16_t *events16;    // the same words in 16 bits, or null (E16 kernels read these)
    const uint32_t *trans;
    const uint32_t *trans_off;   // may be null
    const uint8_t *key_width;    // may be null
    const uint16_t *key_states;  // may be null
    const uint8_t *key_error;    // may be null
    const int32_t *order;
    int32_t *ticket;
    int32_t *err;                // [0] LC_BATCH_E_* bits, [1] 1 + largest malformed key
    int32_t err_base;            // that key's index in the caller's batch = err_base + key
    uint32_t *lat_ws;            // k_spec, k_spec_rerun: the waves' 9-10-pending workspaces in global
                                 // memory (k_search_lattice keeps its own in LDS)
    const Args *full;            // device copy: results, counters, spill list
    uint64_t budget;
    int32_t n_order;
    uint32_t init_state, shared_states, flags;
    uint32_t n_trans;            // entries of trans[]
    uint32_t ticket_base;        // ticket value this launch starts from (see launch_t0)
    uint32_t spec_ck1, spec_ck2; // speculative segments: checkpoint distances past a cut
    int32_t *spec_rr;            // speculative segments: keys left to the unsegmented search,
    int32_t *spec_nrr;           //   their count (zero at the launch)
    int32_t *spec_nrr_next;      //   and the next launch's count (zeroed by k_spec_rerun)
    uint32_t *spec_fin;          // exact segments: each run's saved set (2 per segment, SPEC_SAVE_WORDS each)
};

// T0Args read through the kernarg segment where a field is used (k_spec's
// KA): a kernel that takes its arguments by value loads every field
// it uses anywhere at its entry and holds it in a scalar register for its
// whole life; with the walk's own scalars the file overflows into VGPR lanes
// and uniform loop words are kept in VGPRs (copied at every event).  The empty
// asm makes each use's pointer opaque, so no load is hoisted or shared.
using KT0 = const __attribute__((address_space(4))) T0Args;
__device__ __forceinline__ KT0 &t0k() {
    KT0 *p = (KT0 *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return *p;
}

template <bool E16, class A = T0Args>
__device__ __forceinline__ EvSrc<E16> ev_src(const A &a) {
    if constexpr (E16) return {a.events16};
    else return {a.events};
}

template <class A = T0Args>
__device__ __forceinline__ void t0_malformed(const A &a, int32_t key, uint32_t why) {
    if (lane_id() == 0) {
        atomicOr(&a.err[0], (int32_t)why);
        atomicMax(&a.err[1], a.err_base + key + 1);
    }
}

// The lane index made opaque where it is used (workspace rows, lane masks).
// For the workspace: a row array's lane column, its address formed where
// used: with a plain m.W[k * 64 + lane] the compiler hoisted the 16 rows'
// 64-bit addresses out of the walk's event loop and kept them for its whole
// life -- 16 VGPR pairs, spilled to scratch in the 64-VGPR k_spec builds and
// rewritten there at every walk's start (round 5's 29.8x traffic).  The empty
// asm makes the lane index opaque, so each use site rebuilds one address and
// the rows are immediate offsets from it.
__device__ __forceinline__ uint32_t opq_lane(uint32_t lane) {
    asm volatile("" : "+v"(lane));
    return lane;
}

// A wave-uniform value the compiler cannot prove uniform (a reduction's
// result, an LDS read): into a scalar register, so control flow on it stays
// scalar (no EXEC masking).
__device__ __forceinline__ uint32_t uni(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
__device__ __forceinline__ int32_t uni(int32_t x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ uint64_t uni(uint64_t x) {
    return (uint64_t)uni((uint32_t)x) | ((uint64_t)uni((uint32_t)(x >> 32)) << 32);
}

// Inclusive prefix sum over the wave's lanes, by DPP: Hillis-Steele within
// each row of 16 (row_shr 1, 2, 4, 8), then row_bcast 15 and 31 carry each
// row's total into the rows above it.
__device__ __forceinline__ int32_t wave_scan(int32_t x) {
    x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xF, 0xF, true);  // row_shr:1
    x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xF, 0xF, true);  // row_shr:2
    x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xF, 0xF, true);  // row_shr:4
    x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xF, 0xF, true);  // row_shr:8
    x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xA, 0xF, false);  // row_bcast:15 -> rows 1, 3
    x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xC, 0xF, false);  // row_bcast:31 -> rows 2, 3
    return x;
}

// Transfer masks of one event: vk[q] = op q's accept mask on lanes with bit
// q (0 elsewhere and for q = p); sc[q] / sb[q] = op q's cap / shift.
struct LaneMasks {
    uint32_t vk[6], sc[10], sb[10], sm[10];
};

template <int N, bool TAG = false>
__device__ __forceinline__ void lane_masks(LaneMasks &m, uint32_t p, uint32_t k_v, uint32_t cap_v, uint32_t b_v,
                                           uint32_t lane, uint32_t m_v = 0) {
#pragma unroll
    for (int q = 0; q < 6; ++q) m.vk[q] = 0u;
#pragma unroll
    for (int q = 0; q < 10; ++q) { m.sc[q] = 0u; m.sb[q] = 0u; }
    // (lane bit q as a 0 / ~0 word from an opaque lane index, p's mask
    // cleared in the scalar: written as `lane bit q && q != p ? sk : 0`, the
    // six lane conditions became loop-invariant 64-bit scalar masks, hoisted
    // out of the walk and spilled into VGPR lanes -- 12 v_readlane and 12
    // scalar selects at every 7-10-pending :ok of the 64-VGPR k_spec builds)
    const uint32_t ol = opq_lane(lane);
#pragma unroll
    for (int q = 0; q < (N < 6 ? N : 6); ++q) {
        const uint32_t sk = (uint32_t)q != p ? (uint32_t)__builtin_amdgcn_readlane(k_v, q) : 0u;
        m.vk[q] = sk & (uint32_t)__builtin_amdgcn_sbfe((int)ol, q, 1);
    }
#pragma unroll
    for (int q = 0; q < (N < 10 ? N : 10); ++q) {
        m.sc[q] = __builtin_amdgcn_readlane(cap_v, q);
        m.sb[q] = __builtin_amdgcn_readlane(b_v, q);
        if constexpr (TAG) m.sm[q] = __builtin_amdgcn_readlane(m_v, q);
    }
}

// One Gauss-Seidel pass over lane-bit positions Q .. min(N, 6) - 1.  A
// position is T_Q applied to the gathered word: min(x & k, cap) << b, OR-ed
// into cur.  The DPP gathers (Q < 4) have a single use and fold into the
// v_and_b32 (v_and_b32_dpp); the permlane swaps (Q = 4, 5) clobber both
// operands, so their other operand is `prev`, the previous position's min()
// result, dead once it has been shifted into cur -- one copy of cur per swap.
template <int Q, int N, bool TAG = false>
__device__ __forceinline__ uint32_t sweep_lanes(uint32_t cur, const LaneMasks &m, uint32_t prev = 0) {
    if constexpr (Q >= N || Q >= 6) {
        return cur;
    } else if constexpr (TAG) {
        const uint32_t x = gdown_j<Q>(cur, prev);
        const uint32_t t = (x & m.vk[Q]) + m.sc[Q];
        return sweep_lanes<Q + 1, N, TAG>(((t >> m.sb[Q]) & m.sm[Q]) | cur, m, t);
    } else {
        const uint32_t x = gdown_j<Q>(cur, prev);
        const uint32_t t = __builtin_elementwise_min(x & m.vk[Q], m.sc[Q]);
        return sweep_lanes<Q + 1, N>((t << m.sb[Q]) | cur, m, t);
    }
}

// Probe count of the oracle for one event (LC_OPT_COUNT_PROBES only): legal
// successors over I plus legal applications of p.
template <int RL, int NB>
__device__ __forceinline__ uint32_t event_probes(const uint32_t *I, uint32_t p, uint32_t cand, uint32_t k_v,
                                                 uint32_t lane, uint32_t pm) {
    uint32_t pr = 0;  // pm: p's accept mask
#pragma unroll
    for (int q = 0; q < NB; ++q) {
        const uint32_t m = ((cand >> q) & 1u) ? __builtin_amdgcn_readlane(k_v, q) : 0u;
#pragma unroll
        for (int k = 0; k < RL; ++k)
            if (!idx_has(lane, k, (uint32_t)q)) pr += (uint32_t)__popc(I[k] & m);
    }
#pragma unroll
    for (int k = 0; k < RL; ++k) pr += (uint32_t)__popc(I[k] & pm);
    return pr;
}

#ifdef LC_T0_COUNT_SWEEPS
// Diagnostic build only: histogram of (closure width nc, sweeps run), one per
// translation unit; lc_debug_sweep_hist (device_lattice.hip) sums them.
[[maybe_unused]] static __device__ unsigned long long lc_sweep_hist[8 * 8];
#endif

// One :ok(p) event while every live op index is < 6: the whole lattice is
// one register and every subset bit is a lane bit.  Op indices are assigned
// lowest-free at invoke (not compacted), so an :ok only frees index p -- no
// relocation: S' lands on the lanes without bit p and lanes with bit p stay
// empty, which is exactly the state a later invoke into index p needs.  One
// code path for every live set (free positions and p carry zero masks), so an
// event costs no dispatch branches; the gather along the run-time bit p is one
// ds_bpermute, issued first so its latency hides under the mask setup.
// lm[q] (0 / ~0) is lane bit q as a VGPR mask.  W = S on entry, S' on a
// normal return.  Returns 0 normal, 1 invalid, 2 budget exceeded.
// The closure sweeps run until one changes nothing, without a trip counter
// (the sweeps only grow the set inside its closure, a finite lattice): the
// loop is the sweep, one v_cmp and a vcc branch -- six scalar instructions
// and a counter fewer per sweep than `for (s < nc) ... if (!__any) break`.
// C2 k_spec 0.2786 -> 0.2754 ms, C5 0.2834 -> 0.2808 (A/B on one box,
// tools/gpu_r4o.sh); LC_T0_SWEEP_DO=0 keeps the counted loop.
#ifndef LC_T0_SWEEP_DO
#define LC_T0_SWEEP_DO 1
#endif
template <int T>  // T = 1 + the highest live index (positions T.. are empty)
__device__ __forceinline__ int ok_lane(uint32_t &W, uint32_t p, uint32_t live, uint32_t k_v, uint32_t cap_v,
                                       uint32_t b_v, uint32_t pk, uint32_t pc, uint32_t pb, uint32_t lane,
                                       const uint32_t (&lm)[6], uint64_t budget, bool count, uint32_t &probes,
                                       uint32_t &nSn_out, bool want_size) {
    const uint32_t cand = live & ~(1u << p);
    const uint32_t wup = xor_lane(W, p, lane);
    // free indices and p hold zero accept masks in k_v (the caller cleared
    // lane p), so a position's masks need no gating by `cand`
    LaneMasks m;
#pragma unroll
    for (int q = 0; q < T; ++q) {
        m.vk[q] = vand(__builtin_amdgcn_readlane(k_v, q), lm[q]);
        m.sc[q] = __builtin_amdgcn_readlane(cap_v, q);
        m.sb[q] = __builtin_amdgcn_readlane(b_v, q);
    }
    const bool hp = (lane >> p) & 1u;
    if (count) probes += (uint32_t)__popc(W);
    uint32_t Ret = hp ? 0u : wup;
    uint32_t I = hp ? 0u : W;
    const uint32_t nc = (uint32_t)__popc(cand);  // a closure path has at most nc steps
#ifdef LC_T0_COUNT_SWEEPS
    uint32_t done_s = nc;
#endif
#if LC_T0_SWEEP_DO && !defined(LC_T0_COUNT_SWEEPS)
    // until a sweep changes nothing (see ok_lane_closed)
    (void)nc;
    bool ch;
    do {
        const uint32_t nv = sweep_lanes<0, T>(I, m);
        ch = nv != I;
        I = nv;
    } while (__any(ch));
#else
#pragma unroll 1
    for (uint32_t s = 0; s < nc; ++s) {
        const uint32_t nv = sweep_lanes<0, T>(I, m);
        const bool ch = nv != I;
        I = nv;
        if (!__any(ch)) {
#ifdef LC_T0_COUNT_SWEEPS
            done_s = s + 1;
#endif
            break;
        }
    }
#endif
#ifdef LC_T0_COUNT_SWEEPS
    if (lane == 0) atomicAdd(&lc_sweep_hist[nc * 8 + (done_s < 7 ? done_s : 7)], 1ull);
#endif
    if (count) probes += event_probes<1, 6>(&I, p, cand, k_v, lane, pk);
    Ret = xacc(Ret, I, pk, pc, pb);
    // One register holds at most 64 x 32 configs: with a larger budget only
    // emptiness matters (a ballot); exact sizes only when asked for (peak).
    if (__builtin_expect(budget < 64u * 32u, 0)) {
        const uint32_t nI = __ockl_wfred_add_u32((uint32_t)__popc(I));
        if (nI > budget) return 2;
    }
    if (!__any(Ret != 0u)) { nSn_out = 0; return 1; }
    if (__builtin_expect(budget < 64u * 32u || want_size, 0)) {
        const uint32_t nSn = __ockl_wfred_add_u32((uint32_t)__popc(Ret));
        nSn_out = nSn;
        if (nSn > budget) return 2;
    }
    W = Ret;
    return 0;
}

// Fast path (verdicts only): the lane lattice is kept CLOSED under every
// pending op instead of holding exactly Knossos's set S.  With C(S) the
// closure of S under the pending ops, the projection
//     { (s, L \ p) : (s, L) in C(S_k), p in L }  =  C(S_{k+1}),
// so an :ok(p) is "close W, then keep the lanes with bit p, shifted down":
// S_{k+1} is empty iff that projection is.  Any W with S <= W <= C(S) closes
// to C(S), and W is already closed when no op was invoked since the last
// :ok (`dirty` false): then the :ok is the projection alone.  Sets are
// supersets of Knossos's, so this path is used only when no set size, probe
// count or config list is asked for (FAST in lattice_walk).
// Returns 0 normal, 1 invalid (W unchanged).
template <int T, bool TAG = false>
__device__ __forceinline__ int ok_lane_closed(uint32_t &W, uint32_t p, uint32_t live, uint32_t k_v, uint32_t cap_v,
                                              uint32_t b_v, uint32_t lane, const uint32_t (&lm)[6], bool dirty,
                                              uint32_t m_v = 0) {
    uint32_t C = W;
    if (dirty) {
        LaneMasks m;
#pragma unroll
        for (int q = 0; q < T; ++q) {
            m.vk[q] = vand(__builtin_amdgcn_readlane(k_v, q), lm[q]);
            m.sc[q] = __builtin_amdgcn_readlane(cap_v, q);
            m.sb[q] = __builtin_amdgcn_readlane(b_v, q);
            if constexpr (TAG) m.sm[q] = __builtin_amdgcn_readlane(m_v, q);
        }
#if LC_T0_SWEEP_DO
        // until a sweep changes nothing: the sweeps only grow C inside the
        // closure, a finite lattice, so the loop ends (no trip counter)
        bool ch;
        do {
            const uint32_t nv = sweep_lanes<0, T, TAG>(C, m);
            ch = nv != C;
            C = nv;
        } while (__any(ch));
#else
        const uint32_t nc = (uint32_t)__popc(live);  // a path has at most nc steps
#pragma unroll 1
        for (uint32_t s = 0; s < nc; ++s) {
            const uint32_t nv = sweep_lanes<0, T, TAG>(C, m);
            const bool ch = nv != C;
            C = nv;
            if (!__any(ch)) break;
        }
#endif
    }
    // (a DPP switch on p measured slower, in the compact T0 and in the
    // speculative segments' walk: 1,224 against 1,142 cycles per event)
    const uint32_t up = xor_lane(C, p, lane);
    // (lane bit p as a 0 / ~0 word: one v_bfe, and the select a v_bfi)
    const uint32_t Wn = up & ~(uint32_t)__builtin_amdgcn_sbfe((int)lane, (int)p, 1);
    if (!__any(Wn != 0u)) return 1;
    W = Wn;
    return 0;
}

// One :ok(p) event on a lattice of RL registers (N = 7 or 8 ops pending):
// lane bits 0..5 as in ok_lane, register bits 6.. through register pairs.
template <int RL, int RM, bool TAG = false>
__device__ __forceinline__ int ok_reg(uint32_t (&W)[RM], uint32_t p, uint32_t k_v, uint32_t cap_v, uint32_t b_v,
                                      uint32_t lane, uint64_t budget, bool count, uint32_t &probes,
                                      uint32_t &nSn_out, bool want_size, uint32_t m_v = 0) {
    constexpr int NB = lat_bits<RL>();  // = ops pending
    constexpr int NR = NB - 6;          // register bits
    LaneMasks m;
    lane_masks<NB, TAG>(m, p, k_v, cap_v, b_v, lane, m_v);
    uint32_t rk[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const bool on = (uint32_t)(6 + r) != p;
        const uint32_t sk = __builtin_amdgcn_readlane(k_v, 6 + r);
        rk[r] = on ? sk : 0u;
    }
    const uint32_t pk = __builtin_amdgcn_readlane(k_v, p), pc = __builtin_amdgcn_readlane(cap_v, p),
                   pb = __builtin_amdgcn_readlane(b_v, p);
    const uint32_t pm = TAG ? __builtin_amdgcn_readlane(m_v, p) : ~0u;
    uint32_t Ret[RL], I[RL];
    if (count) {
#pragma unroll
        for (int k = 0; k < RL; ++k) probes += (uint32_t)__popc(W[k]);
    }
    if (p < 6) {
        const bool hp = (lane >> p) & 1u;
#pragma unroll
        for (int k = 0; k < RL; ++k) {
            const uint32_t u = gup_rt(W[k], p);
            Ret[k] = hp ? 0u : u;
            I[k] = hp ? 0u : W[k];
        }
    } else {
        const uint32_t r = p - 6;
#pragma unroll
        for (int k = 0; k < RL; ++k) {
            uint32_t src = W[k];
#pragma unroll
            for (int rr = 0; rr < NR; ++rr)
                if (r == (uint32_t)rr) src = W[k | (1 << rr)];
            const bool hk = ((uint32_t)k >> r) & 1u;
            Ret[k] = hk ? 0u : src;
            I[k] = hk ? 0u : W[k];
        }
    }
#pragma unroll 1
    for (int s = 1; s < NB; ++s) {
        uint32_t nv[RL];
#pragma unroll
        for (int k = 0; k < RL; ++k) nv[k] = sweep_lanes<0, 6, TAG>(I[k], m);
#pragma unroll
        for (int r = 0; r < NR; ++r)
#pragma unroll
            for (int k = 0; k < RL; ++k)
                if ((k >> r) & 1)
                    nv[k] = xacc<TAG>(nv[k], nv[k ^ (1 << r)], rk[r], m.sc[6 + r], m.sb[6 + r], TAG ? m.sm[6 + r] : ~0u);
        bool ch = false;
#pragma unroll
        for (int k = 0; k < RL; ++k) { ch |= nv[k] != I[k]; I[k] = nv[k]; }
        if (!__any(ch)) break;
    }
    if (count)
        probes += event_probes<RL, NB>(I, p, ((1u << NB) - 1u) & ~(1u << p), k_v, lane, pk);
    uint32_t cI = 0, cS = 0;
#pragma unroll
    for (int k = 0; k < RL; ++k) {
        Ret[k] = xacc<TAG>(Ret[k], I[k], pk, pc, pb, pm);
        cI += (uint32_t)__popc(I[k]);
        cS += (uint32_t)__popc(Ret[k]);
    }
    if (budget < (uint64_t)RL * 64u * 32u) {
        const uint32_t nI = __ockl_wfred_add_u32(cI);
        if (nI > budget) return 2;
    }
    if (!__any(cS != 0u)) { nSn_out = 0; return 1; }
    if (budget < (uint64_t)RL * 64u * 32u || want_size) {
        const uint32_t nSn = __ockl_wfred_add_u32(cS);
        nSn_out = nSn;
        if (nSn > budget) return 2;
    }
    constexpr int rl = NR - 1;  // `last` = NB - 1 is register bit rl
    if (p == (uint32_t)(NB - 1)) {
#pragma unroll
        for (int k = 0; k < RL; ++k) W[k] = Ret[k];
        return 0;
    }
    if (p < 6) {
        const bool hp = (lane >> p) & 1u;
#pragma unroll
        for (int k = 0; k < RL; ++k) {
            if ((k >> rl) & 1) { W[k] = 0u; continue; }
            const uint32_t z = gdown_rt(Ret[k | (1 << rl)], p);
            W[k] = hp ? z : Ret[k];
        }
    } else {
        const uint32_t r = p - 6;
#pragma unroll
        for (int k = 0; k < RL; ++k) {
            if ((k >> rl) & 1) { W[k] = 0u; continue; }
            uint32_t src = Ret[k];
#pragma unroll
            for (int rr = 0; rr < NR; ++rr)
                if (r == (uint32_t)rr) src = Ret[(k ^ (1 << rr)) | (1 << rl)];
            W[k] = (((uint32_t)k >> r) & 1u) ? src : Ret[k];
        }
    }
    return 0;
}

// ok_reg on CLOSED sets (verdicts only; ok_lane_closed's identity at 7 or 8
// ops pending): W is closed under every pending op when dirty (an op was
// invoked since the last closure), the lanes / registers with bit p are kept
// with that bit moved down, and `last` takes index p as in ok_reg.  A clean
// :ok is the projection alone: no masks, no sweeps.
// Returns 0 normal, 1 invalid (W then holds the closure).
template <int RL, int RM>
__device__ __forceinline__ int ok_reg_closed(uint32_t (&W)[RM], uint32_t p, uint32_t k_v, uint32_t cap_v,
                                             uint32_t b_v, uint32_t lane, bool dirty) {
    constexpr int NB = lat_bits<RL>();  // = ops pending
    constexpr int NR = NB - 6;          // register bits
    constexpr int rl = NR - 1;          // `last` = NB - 1 is register bit rl
    if (dirty) {
        LaneMasks m;
        lane_masks<NB>(m, ~0u, k_v, cap_v, b_v, lane);  // (no op left out: p's steps belong to the closure)
        uint32_t rk[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) rk[r] = __builtin_amdgcn_readlane(k_v, 6 + r);
#pragma unroll 1
        for (int s = 0; s < NB; ++s) {  // a path has at most NB steps
            uint32_t nv[RL];
#pragma unroll
            for (int k = 0; k < RL; ++k) nv[k] = sweep_lanes<0, 6>(W[k], m);
#pragma unroll
            for (int r = 0; r < NR; ++r)
#pragma unroll
                for (int k = 0; k < RL; ++k)
                    if ((k >> r) & 1) nv[k] = xacc(nv[k], nv[k ^ (1 << r)], rk[r], m.sc[6 + r], m.sb[6 + r]);
            bool ch = false;
#pragma unroll
            for (int k = 0; k < RL; ++k) { ch |= nv[k] != W[k]; W[k] = nv[k]; }
            if (!__any(ch)) break;
        }
    }
    // the new set over indices 0 .. NB-2, index p now the op that was `last`:
    // L with p comes from L + last, L without p from L + p (without last)
    uint32_t Wn[RL];
    uint32_t any = 0;
    if (p == (uint32_t)(NB - 1)) {
#pragma unroll
        for (int k = 0; k < RL; ++k) Wn[k] = ((k >> rl) & 1) ? 0u : W[k | (1 << rl)];
    } else if (p < 6) {
        const uint32_t hp = (uint32_t)__builtin_amdgcn_sbfe((int)lane, (int)p, 1);  // lane bit p as 0 / ~0
#pragma unroll
        for (int k = 0; k < RL; ++k) {
            if ((k >> rl) & 1) { Wn[k] = 0u; continue; }
            const uint32_t u = gup_rt(W[k], p);
            Wn[k] = (W[k | (1 << rl)] & hp) | (u & ~hp);
        }
    } else {
        const uint32_t r = p - 6;
#pragma unroll
        for (int k = 0; k < RL; ++k) {
            if ((k >> rl) & 1) { Wn[k] = 0u; continue; }
            uint32_t src = W[k | (1 << rl)];
#pragma unroll
            for (int rr = 0; rr < rl; ++rr)
                if (r == (uint32_t)rr && !((k >> rr) & 1)) src = W[k | (1 << rr)];
            Wn[k] = src;
        }
    }
#pragma unroll
    for (int k = 0; k < RL; ++k) any |= Wn[k];
    if (!__any(any != 0u)) return 1;
#pragma unroll
    for (int k = 0; k < RL; ++k) W[k] = Wn[k];
    return 0;
}

// Lattice of a key with 9 or 10 ops pending: 16 x 64 words per array in the
// block's LDS workspace, index k * 64 + lane.  Every lane reads and writes
// only its own column (register-bit partners are in the same lane; lane-bit
// partners are exchanged in registers), so no cross-lane memory ordering is
// involved.  Such events are rare (< 0.2 % of C2's); keeping them out of
// registers keeps T0's register budget small.
struct LatMem {
    uint32_t *W, *R, *I;
};


template <int RL, bool TAG = false>
__device__ __forceinline__ int ok_event_mem(const LatMem &m, uint32_t p, uint32_t n, uint32_t k_v,
                                            uint32_t cap_v, uint32_t b_v, uint32_t lane, uint64_t budget,
                                            bool count, uint32_t &probes, uint32_t &nSn_out, bool want_size,
                                            uint32_t m_v = 0) {
    constexpr int NB = lat_bits<RL>();
    const uint32_t cand = ((1u << n) - 1u) & ~(1u << p);
    // transfer of candidate q: lane q of k_v/cap_v/b_v, read at use
    // (not hoisted: 3 x NB scalars would spill SGPRs into the VGPR budget)
    const uint32_t ck = k_v & (((cand >> lane) & 1u) ? ~0u : 0u);
#define KK(Q) __builtin_amdgcn_readlane(ck, Q)
#define CP(Q) __builtin_amdgcn_readlane(cap_v, Q)
#define SB(Q) __builtin_amdgcn_readlane(b_v, Q)
#define SM(Q) (TAG ? __builtin_amdgcn_readlane(m_v, Q) : ~0u)
    const uint32_t pk = __builtin_amdgcn_readlane(k_v, p), pc = __builtin_amdgcn_readlane(cap_v, p),
                   pb = __builtin_amdgcn_readlane(b_v, p), pm = SM(p);
    const uint32_t plm = p < 6 ? 1u << p : 0u, prm = p >= 6 ? 1u << (p - 6) : 0u;
#pragma unroll 1
    for (int k = 0; k < RL; ++k) {
        const uint32_t w = m.W[k * 64 + lane];
        if (count) probes += (uint32_t)__popc(w);
        const uint32_t src = (uint32_t)__shfl_xor((int)m.W[(k ^ prm) * 64 + lane], (int)plm);
        const bool hp = (lane & plm) || ((uint32_t)k & prm);
        m.R[k * 64 + lane] = hp ? 0u : src;
        m.I[k * 64 + lane] = hp ? 0u : w;
    }
    for (;;) {  // sweeps in place (monotone: any order reaches the fixpoint)
        bool ch = false;
#pragma unroll 1
        for (int k = 0; k < RL; ++k) {
            const uint32_t x = m.I[k * 64 + lane];
            uint32_t acc = x;
#define LC_LANEBIT(Q)                                                                  \
            {                                                                          \
                const uint32_t y = xv<Q>(x, lane);                                     \
                acc |= ((lane >> Q) & 1u) ? xapply<TAG>(y, KK(Q), CP(Q), SB(Q), SM(Q)) : 0u; \
            }
            LC_LANEBIT(0) LC_LANEBIT(1) LC_LANEBIT(2) LC_LANEBIT(3) LC_LANEBIT(4) LC_LANEBIT(5)
#undef LC_LANEBIT
#pragma unroll
            for (int q = 6; q < NB; ++q)
                if ((k >> (q - 6)) & 1)
                    acc |= xapply<TAG>(m.I[(k ^ (1 << (q - 6))) * 64 + lane], KK(q), CP(q), SB(q), SM(q));
            if (acc != x) { m.I[k * 64 + lane] = acc; ch = true; }
        }
        if (!__any(ch)) break;
    }
    uint32_t cI = 0, cS = 0;
#pragma unroll 1
    for (int k = 0; k < RL; ++k) {
        const uint32_t x = m.I[k * 64 + lane];
        if (count) {
#pragma unroll
            for (int q = 0; q < NB; ++q)
                if (!idx_has(lane, k, (uint32_t)q)) probes += (uint32_t)__popc(x & KK(q));
            probes += (uint32_t)__popc(x & pk);
        }
        const uint32_t r = m.R[k * 64 + lane] | xapply<TAG>(x, pk, pc, pb, pm);
        m.R[k * 64 + lane] = r;
        cI += (uint32_t)__popc(x);
        cS += (uint32_t)__popc(r);
    }
    if (budget < (uint64_t)RL * 64u * 32u) {
        const uint32_t nI = __ockl_wfred_add_u32(cI);
        if (nI > budget) return 2;
    }
    if (!__any(cS != 0u)) { nSn_out = 0; return 1; }
    if (budget < (uint64_t)RL * 64u * 32u || want_size) {
        const uint32_t nSn = __ockl_wfred_add_u32(cS);
        nSn_out = nSn;
        if (nSn > budget) return 2;
    }
#undef KK
#undef CP
#undef SB
#undef SM
    // relocation: the op at index `last` moves to index p
    const uint32_t last = n - 1;
    const uint32_t llm = last < 6 ? 1u << last : 0u, lrm = last >= 6 ? 1u << (last - 6) : 0u;
#pragma unroll 1
    for (int k = 0; k < RL; ++k) {
        const uint32_t r = m.R[k * 64 + lane];
        const uint32_t src = (uint32_t)__shfl_xor((int)m.R[(k ^ (prm | lrm)) * 64 + lane], (int)(plm | llm));
        const bool hp = (lane & plm) || ((uint32_t)k & prm);
        const bool hl = (lane & llm) || ((uint32_t)k & lrm);
        m.W[k * 64 + lane] = p == last ? r : (hl ? 0u : (hp ? src : r));
    }
    return 0;
}

// ok_event_mem's closure as Gauss-Seidel sweeps (verdicts only: no sizes or
// probes): each row a one-directional lane sweep (sweep_lanes, 3 VALU per
// position), then the register bits from the rows below it, already updated
// in this sweep.  The bidirectional per-row form above needs about twice the
// instructions per sweep and more sweeps.
template <int RL>
__device__ __forceinline__ int ok_event_mem_gs(const LatMem &m, uint32_t p, uint32_t n, uint32_t k_v, uint32_t cap_v,
                                               uint32_t b_v, uint32_t lane) {
    constexpr int NB = lat_bits<RL>();
    constexpr int NR = NB - 6;
    LaneMasks lmk;
    lane_masks<NB>(lmk, p, k_v, cap_v, b_v, lane);
    uint32_t rk[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) rk[r] = (uint32_t)(6 + r) != p ? __builtin_amdgcn_readlane(k_v, 6 + r) : 0u;
    const uint32_t pk = __builtin_amdgcn_readlane(k_v, p), pc = __builtin_amdgcn_readlane(cap_v, p),
                   pb = __builtin_amdgcn_readlane(b_v, p);
    const uint32_t plm = p < 6 ? 1u << p : 0u, prm = p >= 6 ? 1u << (p - 6) : 0u;
    const uint32_t ol = opq_lane(lane);
    uint32_t *const mW = m.W + ol, *const mR = m.R + ol, *const mI = m.I + ol;
#pragma unroll 1
    for (int k = 0; k < RL; ++k) {
        const uint32_t w = mW[k * 64];
        const uint32_t src = (uint32_t)__shfl_xor((int)mW[(k ^ prm) * 64], (int)plm);
        const bool hp = (lane & plm) || ((uint32_t)k & prm);
        mR[k * 64] = hp ? 0u : src;
        mI[k * 64] = hp ? 0u : w;
    }
#pragma unroll 1
    for (int s = 0; s < NB; ++s) {
        bool ch = false;
#pragma unroll 1
        for (int k = 0; k < RL; ++k) {
            const uint32_t x = mI[k * 64];
            uint32_t nv = sweep_lanes<0, 6>(x, lmk);
#pragma unroll
            for (int r = 0; r < NR; ++r)
                if ((k >> r) & 1) nv = xacc(nv, mI[(k ^ (1 << r)) * 64], rk[r], lmk.sc[6 + r], lmk.sb[6 + r]);
            if (nv != x) {
                mI[k * 64] = nv;
                ch = true;
            }
        }
        if (!__any(ch)) break;
    }
    uint32_t cS = 0;
#pragma unroll 1
    for (int k = 0; k < RL; ++k) {
        const uint32_t r = mR[k * 64] | xapply(mI[k * 64], pk, pc, pb);
        mR[k * 64] = r;
        cS |= r;
    }
    if (!__any(cS != 0u)) return 1;
    const uint32_t last = n - 1;
    const uint32_t llm = last < 6 ? 1u << last : 0u, lrm = last >= 6 ? 1u << (last - 6) : 0u;
#pragma unroll 1
    for (int k = 0; k < RL; ++k) {
        const uint32_t r = mR[k * 64];
        const uint32_t src = (uint32_t)__shfl_xor((int)mR[(k ^ (prm | lrm)) * 64], (int)(plm | llm));
        const bool hp = (lane & plm) || ((uint32_t)k & prm);
        const bool hl = (lane & llm) || ((uint32_t)k & lrm);
        mW[k * 64] = p == last ? r : (hl ? 0u : (hp ? src : r));
    }
    return 0;
}

// ok_event_mem_gs on CLOSED sets (verdicts only; see ok_reg_closed): m.W is
// closed in place when dirty, its part with bit p goes to m.R with that bit
// moved down and `last` (a row bit: n >= 9) relocated to p, and back to m.W.
// Returns 0 normal, 1 invalid (m.W then holds the closure).
template <int RL>
__device__ __forceinline__ int ok_event_mem_closed(const LatMem &m, uint32_t p, uint32_t k_v, uint32_t cap_v,
                                                   uint32_t b_v, uint32_t lane, bool dirty) {
    constexpr int NB = lat_bits<RL>();  // = ops pending (9 or 10)
    constexpr int NR = NB - 6;
    constexpr uint32_t lrm = 1u << (NR - 1);  // `last` = NB - 1 as a row bit
    const uint32_t ol = opq_lane(lane);
    uint32_t *const mW = m.W + ol, *const mR = m.R + ol;
    if (dirty) {
        LaneMasks lmk;
        lane_masks<NB>(lmk, ~0u, k_v, cap_v, b_v, lane);
        uint32_t rk[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) rk[r] = __builtin_amdgcn_readlane(k_v, 6 + r);
#pragma unroll 1
        for (int s = 0; s < NB; ++s) {
            bool ch = false;
#pragma unroll 1
            for (int k = 0; k < RL; ++k) {
                const uint32_t x = mW[k * 64];
                uint32_t nv = sweep_lanes<0, 6>(x, lmk);
#pragma unroll
                for (int r = 0; r < NR; ++r)
                    if ((k >> r) & 1) nv = xacc(nv, mW[(k ^ (1 << r)) * 64], rk[r], lmk.sc[6 + r], lmk.sb[6 + r]);
                if (nv != x) {
                    mW[k * 64] = nv;
                    ch = true;
                }
            }
            if (!__any(ch)) break;
        }
    }
    const uint32_t plm = p < 6 ? 1u << p : 0u, prm = p >= 6 ? 1u << (p - 6) : 0u;
    const bool p_last = p == (uint32_t)(NB - 1);
    uint32_t cS = 0;
#pragma unroll 1
    for (int k = 0; k < RL; ++k) {
        // L with p: from L + last, same lane; L without p: from L + p.  (The
        // gather runs on every lane: no cross-lane op under a divergent mask.)
        const uint32_t up = (uint32_t)__shfl_xor((int)mW[(k ^ prm) * 64], (int)plm);
        const uint32_t wl = mW[(k | lrm) * 64];
        const bool hp = (lane & plm) || ((uint32_t)k & prm);
        const uint32_t r = ((uint32_t)k & lrm) ? 0u : (p_last || hp) ? wl : up;
        mR[k * 64] = r;
        cS |= r;
    }
    if (!__any(cS != 0u)) return 1;
#pragma unroll 1
    for (int k = 0; k < RL; ++k) mW[k * 64] = mR[k * 64];
    return 0;
}

// The max_final smallest configs of the lattice held in m.W (register
// lattices are stored there first) in (slot mask, state) order, op indices
// translated back to window slots (slot_v: lane j holds the slot of the op
// at index j; `live` = the occupied indices).  The order is the window's, not
// the op indices', so every run that holds the same set -- the unsegmented
// search, a speculative segment's that assigned its own indices -- writes
// the same records (Knossos's truncation to 10 is of an unordered set; any
// fixed choice matches it).  Selection: max_final rounds of a wave minimum.
__device__ __forceinline__ void write_final_mem(const Args &a, int32_t key, const LatMem &m, uint32_t lane,
                                                uint32_t slot_v, uint32_t live_ops) {
    if (!a.final_cfg) return;
    const uint32_t mf = (uint32_t)a.max_final;
    const uint32_t top = live_ops ? 32u - (uint32_t)__clz(live_ops) : 0u;  // index bits in use
    const int live = top <= 6 ? 1 : (1 << (top - 6));
    // slot mask of subset L = lane + 64 k: the lane's bits (indices 0..5)
    // and the row's (6..), the latter uniform
    uint64_t lo = 0;
    uint32_t cnt = 0;
    for (uint32_t j = 0; j < top && j < 6u; ++j) {
        const uint32_t sj = __builtin_amdgcn_readlane(slot_v, j);
        if (((lane & live_ops) >> j) & 1u) lo |= 1ull << sj;
    }
#pragma unroll 1
    for (int k = 0; k < live; ++k) cnt += (uint32_t)__popc(m.W[k * 64 + lane]);
    const uint32_t tot = __ockl_wfred_add_u32(cnt);
    const uint32_t nw = tot < mf ? tot : mf;
    uint64_t last_m = 0;
    int last_s = -1;
#pragma unroll 1
    for (uint32_t r = 0; r < nw; ++r) {
        const uint32_t above = last_s < 0 ? ~0u : last_s >= 31 ? 0u : ~((2u << last_s) - 1u);
        uint64_t bm = ~0ull;
        uint32_t bs = 32;
#pragma unroll 1
        for (int k = 0; k < live; ++k) {
            uint32_t w = m.W[k * 64 + lane];
            uint64_t hi = 0;
            for (uint32_t j = 6; j < top; ++j)
                if ((((uint32_t)k << 6) & live_ops) >> j & 1u) hi |= 1ull << __builtin_amdgcn_readlane(slot_v, j);
            const uint64_t sm = lo | hi;
            if (sm == last_m) w &= above;
            if (w && sm >= last_m && sm < bm) {
                bm = sm;
                bs = (uint32_t)__ffs(w) - 1;
            }
        }
        uint64_t mn = bm;
        for (int o = 32; o >= 1; o >>= 1) {
            const uint32_t l2 = (uint32_t)__shfl_xor((int)(uint32_t)mn, o), h2 = (uint32_t)__shfl_xor((int)(uint32_t)(mn >> 32), o);
            const uint64_t v = ((uint64_t)h2 << 32) | l2;
            mn = v < mn ? v : mn;
        }
        uint32_t st = bm == mn ? bs : 32u;
        for (int o = 32; o >= 1; o >>= 1) {
            const uint32_t v = (uint32_t)__shfl_xor((int)st, o);
            st = v < st ? v : st;
        }
        if (lane == 0) {
            a.final_cfg[((size_t)key * a.max_final + r) * 2 + 0] = mn;
            a.final_cfg[((size_t)key * a.max_final + r) * 2 + 1] = (uint64_t)st << 48;
        }
        last_m = mn;
        last_s = (int)st;
    }
    if (lane == 0 && a.n_final) a.n_final[key] = nw;
}

// Op indices: an invoke takes the lowest free index.  While at most 6 ops are
// pending every live index is < 6 and an :ok just frees its index (ok_lane);
// from 7 pending on the indices are dense (0..n-1) and an :ok refills the
// freed index p with the op at index n-1 (a two-bit exchange of the lattice),
// so the lattice spans 2^n subsets.
//
// The event loop has one exit test per event and no early returns: the
// compiler then keeps one flat loop (no state-machine phi copies), and with
// the 9-10-pending workspace in LDS there are no global stores in the loop,
// so the prefetch of the next chunk is never waited for early.
//
// Register budget: the loop only touches the T0Args fields it needs; result
// pointers, counters and work lists are read through `full` (a copy of the
// tier's Args in device memory) once per key.

// What a walk leaves behind for its caller's ending, beside the lattice W.
struct LatWalk {
    bool in_mem;      // the lattice lives in m.W (9 or 10 ops pending)
    uint32_t slot_v;  // lane j: window slot of the op at index j
    uint32_t live;    // occupied op indices
    uint32_t n;       // ops pending
    int status;       // 0, or 1 invalid, 2 budget, 3 spill: at event fev, W / live the set before it
    uint32_t fev;
    uint32_t peak, probes;
};

// A walk's state between two events, for the resume form (k_stream; the
// record's layout: stream_plan.hpp): in, where the walk starts; out, where
// it stopped.  The lattice itself is W, or m.W when in_mem.  `dirty` belongs
// to the FAST walk's closed sets and `peak` (the largest set so far) to the
// exact walk: neither reads or writes the other's.
struct LatResume {
    uint32_t k_v, cap_v, b_v, slot_v, dense_v;  // per-op lanes, as in lattice_walk
    uint32_t n, live;
    bool in_mem, dirty;
    uint32_t peak;
};

// The register tier's event walk: events evp[0 .. nev) from the start word
// `init` in lane 0 (a state mask; TAG: one 6-bit group per start state,
// xfer_tag), transitions trp[t], t < ntr.  The unsegmented search
// (lattice_key) and the key segments (segment_search) both run it; the
// speculative segments have a walk of their own (spec_walk).
// FAST: no probe counting, no peak sizes and a budget no lattice can exceed
// (>= 16 x 64 x 32 configs), so every size reduction and budget test folds
// away -- the common case, and the bench's.
// RESUME: the walk starts from *rs and the lattice the caller loaded (W, or
// m.W when rs->in_mem) instead of `init`, in the phase its pending count
// belongs to (7 or more pending: the dense phase), and leaves its state in
// *rs.  Event ordinals (fev) count from evp[0].  On the compact build, FAST
// (k_stream) or exact (k_stream_exact: Knossos's own sets, so sizes, budgets
// and final configs carry across calls).
template <int RM, bool FAST, bool TAG, class EvT, bool RESUME = false>
__device__ __forceinline__ void lattice_walk(uint32_t (&W)[RM], LatWalk &out, const EvT evp, const uint32_t nev,
                                             const uint32_t *const trp, const uint32_t ntr, uint32_t init,
                                             const LatMem &m, uint64_t budget, bool want_peak, bool count,
                                             LatResume *rs = nullptr) {
    static_assert(!TAG || (FAST && RM == T0_RSMALL), "tagged words: closed sets on the compact lattice only");
    static_assert(!RESUME || (!TAG && RM == T0_RSMALL), "resume: the compact untagged build only");
    const uint32_t lane = lane_id();
    auto ldesc = [&](uint32_t w, bool have) -> uint32_t {
        const uint32_t t = LC_EV_TRANS(w);
        return (have && !(w & LC_EV_OK_BIT) && t < ntr) ? trp[t] : 0u;
    };
    auto decode = [](uint32_t d) -> Xfer {
        if constexpr (TAG) return xfer_tag(d);
        else return xfer_of(d);
    };

    if constexpr (!RESUME) {
#pragma unroll
        for (int k = 0; k < RM; ++k) W[k] = 0;
        if (lane == 0) W[0] = init;
    }
    bool in_mem = false;   // lattice lives in m.W (9 or 10 ops pending)
    uint32_t k_v = 0, cap_v = 0, b_v = 0;  // lane j: transfer (k, cap, b) of the op at index j
    uint32_t m_v = 0;      // TAG: and its mask Mb
    uint32_t slot_v = 0;   // lane j: window slot of the op at index j
    uint32_t dense_v = 0;  // lane s: index of the op in window slot s
    uint32_t n = 0;        // ops pending
    uint32_t live = 0;     // occupied op indices (all < 6 while n <= 6; 0..n-1 beyond)
    uint32_t lm[6];        // lane bit q as a 0 / ~0 mask
#pragma unroll
    for (int q = 0; q < 6; ++q) lm[q] = (uint32_t)__builtin_amdgcn_sbfe((int)lane, q, 1);
    uint32_t peak = 1, probes = 0;
    int status = 0;        // 1 invalid, 2 budget, 3 spill
    uint32_t fev = 0;
    if constexpr (RESUME) {
        in_mem = rs->in_mem;
        k_v = rs->k_v; cap_v = rs->cap_v; b_v = rs->b_v; slot_v = rs->slot_v; dense_v = rs->dense_v;
        n = rs->n; live = rs->live;
        if constexpr (!FAST) peak = rs->peak;
    }

    // Event cursor: events arrive 64 at a time, one per lane; the next
    // chunk's words and descriptors are in flight while this one is searched.
    uint32_t ev = lane < nev ? evp[lane] : 0u;
    uint32_t dsc = ldesc(ev, lane < nev);
    uint32_t ev_n = 64 + lane < nev ? evp[64 + lane] : 0u;
    uint32_t dsc_n = ldesc(ev_n, 64 + lane < nev);
    uint32_t ev_nn = 128 + lane < nev ? evp[128 + lane] : 0u;
    // each lane decodes its event's transition once per chunk (VALU, all 64
    // at a time), so an invoke only reads three lanes
    Xfer xc = decode(dsc);
    uint32_t e = 0, i = 0, base = 0;
    uint32_t lim = nev;  // 0 once the key has a verdict: each loop's only exit is its head
    auto advance = [&]() {
        ++e;
        if (++i == 64u) {
            i = 0; base += 64;
            ev = ev_n; dsc = dsc_n; ev_n = ev_nn;
            xc = decode(dsc);
            dsc_n = ldesc(ev_n, base + 64 + lane < nev);
            ev_nn = base + 128 + lane < nev ? evp[base + 128 + lane] : 0u;
        }
    };
// LC_T0_PROFILE: device_lattice.hip, whose kernel flushes the counters,
// defines the two before it includes this header
#ifndef T0_PROF_BEGIN
#define T0_PROF_BEGIN
#define T0_PROF_END(evi)
#endif

    // Two phases, each a loop of its own, so that neither carries the
    // other's values through its back edge (one loop for both made the
    // register allocator copy every loop-carried value twice per event):
    //   lane phase  -- at most 6 ops pending, every live index < 6, the
    //                  lattice in one register (W0);
    //   dense phase -- 7 to 10 pending, dense indices, W[0..3] or the LDS
    //                  workspace; left after the :ok that brings n back to 6.
    uint32_t W0 = W[0];
    bool dirty = true;  // FAST: an op was invoked since the lattice was last closed
    // RESUME with 7 or more pending: the first round skips the lane phase
    // (stream_plan.hpp stream_resume_phase) and keeps the loaded lattice
    [[maybe_unused]] bool dense_first = false;
    if constexpr (RESUME) {
        if constexpr (FAST) dirty = rs->dirty;
        dense_first = n >= 7;
    }
    for (uint32_t phase = 0; phase <= nev && e < lim; ++phase) {
        while (e < lim && !(RESUME && dense_first)) {
            T0_PROF_BEGIN
            const uint32_t evi = __builtin_amdgcn_readlane(ev, i);
            const uint32_t slot = LC_EV_SLOT(evi);
            if (!(evi & LC_EV_OK_BIT)) {
                if (n == 6) break;  // a 7th pending op: the dense phase takes this invoke
                if (n >= T0_MAX_WIDTH || slot >= 64) {
                    status = 3;
                } else {
                    const Xfer x{(uint32_t)__builtin_amdgcn_readlane(xc.k, i),
                                 (uint32_t)__builtin_amdgcn_readlane(xc.cap, i),
                                 (uint32_t)__builtin_amdgcn_readlane(xc.b, i)};
                    const uint32_t idx = (uint32_t)__builtin_ctz(~live);  // lowest free index
                    slot_v = setl(slot_v, idx, slot);
                    k_v = setl(k_v, idx, x.k);
                    cap_v = setl(cap_v, idx, x.cap);
                    b_v = setl(b_v, idx, x.b);
                    if constexpr (TAG) m_v = setl(m_v, idx, (uint32_t)__builtin_amdgcn_readlane(xc.m, i));
                    dense_v = setl(dense_v, slot, idx);
                    live |= 1u << idx;
                    ++n;
                    dirty = true;
                }
            } else {
                const uint32_t p = __builtin_amdgcn_readlane(dense_v, slot & 63u);
                uint32_t nSn = 0;
                int r;
                if constexpr (FAST && RM == T0_RSMALL) {
                    // closed sets (compact build only: on C2's lone waves the
                    // projection's exposed bpermute ate the saved sweeps)
                    const uint32_t top = 32u - (uint32_t)__builtin_clz(live);
                    if (top >= 6) r = ok_lane_closed<6, TAG>(W0, p, live, k_v, cap_v, b_v, lane, lm, dirty, m_v);
                    else if (top == 5) r = ok_lane_closed<5, TAG>(W0, p, live, k_v, cap_v, b_v, lane, lm, dirty, m_v);
                    else r = ok_lane_closed<4, TAG>(W0, p, live, k_v, cap_v, b_v, lane, lm, dirty, m_v);
                    dirty = false;
                    k_v = setl(k_v, p, 0u);
                } else {
                // p's transfer, then p's lane cleared for good: its index is
                // free after this :ok (and an invalid key stops here)
                const uint32_t pk = __builtin_amdgcn_readlane(k_v, p), pc = __builtin_amdgcn_readlane(cap_v, p),
                               pb = __builtin_amdgcn_readlane(b_v, p);
                k_v = setl(k_v, p, 0u);
                // Compact build (many keys per SIMD, throughput): sweeps cover
                // the positions below the highest live index only.  Wide build
                // (one key per SIMD, latency): one sweep body for every event --
                // the specialised copies cost more in instruction-cache misses
                // across a CU's four lone waves than they save.
                const uint32_t top = 32u - (uint32_t)__builtin_clz(live);
                if (RM == T0_RBIG || top >= 6)
                    r = ok_lane<6>(W0, p, live, k_v, cap_v, b_v, pk, pc, pb, lane, lm, budget, count, probes, nSn,
                                   want_peak);
                else if (top == 5)
                    r = ok_lane<5>(W0, p, live, k_v, cap_v, b_v, pk, pc, pb, lane, lm, budget, count, probes, nSn,
                                   want_peak);
                else
                    r = ok_lane<4>(W0, p, live, k_v, cap_v, b_v, pk, pc, pb, lane, lm, budget, count, probes, nSn,
                                   want_peak);
                }
                live = r ? live : live & ~(1u << p);
                n = r ? n : n - 1;
                peak = nSn > peak ? nSn : peak;
                status = r;
                fev = e;
            }
            T0_PROF_END(evi)
            lim = status ? 0u : lim;
            advance();
        }
        if (e >= lim) break;
        if (!(RESUME && dense_first)) {
            W[0] = W0;
#pragma unroll
            for (int k = 1; k < RM; ++k) W[k] = 0u;
        }
        if constexpr (RESUME) dense_first = false;
        while (e < lim) {
            T0_PROF_BEGIN
            const uint32_t evi = __builtin_amdgcn_readlane(ev, i);
            const uint32_t slot = LC_EV_SLOT(evi);
            if (!(evi & LC_EV_OK_BIT)) {
                if (n >= T0_MAX_WIDTH || slot >= 64) {
                    status = 3;
                } else {
                    if (RM < 16 && n == 8) {  // 9 pending: move the lattice to the workspace
                        // (rows from one opaque lane column, as in spec_walk: a
                        // workspace in global memory kept 30 VGPRs of row
                        // addresses alive in k_spec_rerun otherwise)
                        uint32_t *const mW = m.W + opq_lane(lane);
#pragma unroll
                        for (int k = 0; k < T0_RMEM; ++k) mW[k * 64] = k < RM ? W[k < RM ? k : 0] : 0u;
                        in_mem = true;
                    }
                    const Xfer x{(uint32_t)__builtin_amdgcn_readlane(xc.k, i),
                                 (uint32_t)__builtin_amdgcn_readlane(xc.cap, i),
                                 (uint32_t)__builtin_amdgcn_readlane(xc.b, i)};
                    const uint32_t idx = n;  // dense: every index below n is taken
                    slot_v = setl(slot_v, idx, slot);
                    k_v = setl(k_v, idx, x.k);
                    cap_v = setl(cap_v, idx, x.cap);
                    b_v = setl(b_v, idx, x.b);
                    if constexpr (TAG) m_v = setl(m_v, idx, (uint32_t)__builtin_amdgcn_readlane(xc.m, i));
                    dense_v = setl(dense_v, slot, idx);
                    live |= 1u << idx;
                    ++n;
                }
            } else {
                const uint32_t p = __builtin_amdgcn_readlane(dense_v, slot & 63u);
                uint32_t nSn = 0;
                int r;
                if (n == 7)
                    r = ok_reg<2, RM, TAG>(W, p, k_v, cap_v, b_v, lane, budget, count, probes, nSn, want_peak, m_v);
                else if (n == 8)
                    r = ok_reg<4, RM, TAG>(W, p, k_v, cap_v, b_v, lane, budget, count, probes, nSn, want_peak, m_v);
                else if constexpr (RM < 16) {
                    if (n == 9)
                        r = ok_event_mem<8, TAG>(m, p, n, k_v, cap_v, b_v, lane, budget, count, probes, nSn, want_peak,
                                                 m_v);
                    else
                        r = ok_event_mem<16, TAG>(m, p, n, k_v, cap_v, b_v, lane, budget, count, probes, nSn, want_peak,
                                                  m_v);
                } else {
                    if (n == 9) r = ok_reg<8>(W, p, k_v, cap_v, b_v, lane, budget, count, probes, nSn, want_peak);
                    else r = ok_reg<16>(W, p, k_v, cap_v, b_v, lane, budget, count, probes, nSn, want_peak);
                }
                // the op at index `last` takes index p (a no-op when p == last)
                const uint32_t last = n - 1;
                const uint32_t s_last = __builtin_amdgcn_readlane(slot_v, last);
                const uint32_t x0 = __builtin_amdgcn_readlane(k_v, last),
                               x1 = __builtin_amdgcn_readlane(cap_v, last), x2 = __builtin_amdgcn_readlane(b_v, last);
                if (!r) {
                    slot_v = setl(slot_v, p, s_last);
                    k_v = setl(k_v, p, x0);
                    cap_v = setl(cap_v, p, x1);
                    b_v = setl(b_v, p, x2);
                    if constexpr (TAG) m_v = setl(m_v, p, (uint32_t)__builtin_amdgcn_readlane(m_v, last));
                    dense_v = setl(dense_v, s_last & 63u, p);
                    // index `last` is free now: zero transfer (the lane phase relies on it)
                    k_v = setl(k_v, last, 0u);
                }
                live = r ? live : (1u << last) - 1u;
                if (RM < 16 && in_mem && n == 9 && !r) {  // back to registers: no config holds index 8 or 9
                    const uint32_t *const mW = m.W + opq_lane(lane);
#pragma unroll
                    for (int k = 0; k < RM; ++k) W[k] = mW[k * 64];
                    in_mem = false;
                }
                n = r ? n : n - 1;
                peak = nSn > peak ? nSn : peak;
                status = r;
                fev = e;
            }
            T0_PROF_END(evi)
            lim = status ? 0u : lim;
            advance();
            if (n <= 6) break;  // dense indices 0..5: the lane phase's invariant holds
        }
        W0 = W[0];
        dirty = true;  // the dense phase keeps exact sets, not closed ones
    }
#undef T0_PROF_BEGIN
#undef T0_PROF_END
    W[0] = W0;
    out.in_mem = in_mem; out.slot_v = slot_v; out.live = live; out.n = n;
    out.status = status; out.fev = fev; out.peak = peak; out.probes = probes;
    if constexpr (RESUME) {
        rs->in_mem = in_mem;
        rs->k_v = k_v; rs->cap_v = cap_v; rs->b_v = b_v; rs->slot_v = slot_v; rs->dense_v = dense_v;
        rs->n = n; rs->live = live;
        if constexpr (FAST) rs->dirty = dirty;
        else rs->peak = peak;
    }
}

// One key, unsegmented: K_DONE with its results written, or K_SPILL.
template <int RM, bool FAST, bool E16 = false>
__device__ __forceinline__ int lattice_key(const T0Args &a, int32_t key, uint32_t *ws) {
    const uint32_t lane = lane_id();
    const LatMem m{ws, ws + T0_RMEM * 64, ws + 2 * T0_RMEM * 64};
    const uint64_t eb = a.ev_off[key], ee = a.ev_off[key + 1];
    const uint32_t tb = a.trans_off ? a.trans_off[key] : 0u;
    if (a.key_error && a.key_error[key]) {  // lc_pack could not prepare it (check-safe)
        finish_key(*a.full, key, LC_UNKNOWN, LC_CAUSE_ERROR, -1, 0, 0, 0);
        return K_DONE;
    }
    if (a.key_states && a.key_states[key] > LC_WIDE_MAX_STATES) {
        finish_key(*a.full, key, LC_UNKNOWN, LC_CAUSE_STATES, -1, 1, 0, 0);
        return K_DONE;
    }
    const uint32_t nstates = a.trans_off ? (a.key_states ? a.key_states[key] : 0xFFFFu) : a.shared_states;
    const uint32_t width = a.key_width ? a.key_width[key] : 0xFFu;  // = max ops pending at once
    if (nstates > T0_MAX_STATES || width > T0_MAX_WIDTH || a.init_state >= T0_MAX_STATES) return K_SPILL;
    const uint64_t budget = FAST ? ~0ull : a.budget;
    const bool want_peak = !FAST && (a.flags & T0_WANT_PEAK) != 0;
    const bool count = !FAST && (a.flags & T0_COUNT) != 0;
    // The key may name transitions trans[tb + t], t < ntr.  A batch the host
    // did not validate may hold larger ids: they load nothing (the event is
    // then a read of nil), and the batch's validation waves report them.
    // Every other malformation (an :ok of a slot that is not pending, an
    // :invoke into an occupied one) leaves T0 in bounds -- indices stay below
    // T0_MAX_WIDTH and lanes below 64 -- with a verdict the failed call
    // does not return.
    const uint32_t ntr = a.n_trans > tb ? a.n_trans - tb : 0u;
    const uint32_t nev = (a.flags & T0_DBG_NOEVENTS) ? 0u : (uint32_t)(ee - eb);
    uint32_t W[RM];
    LatWalk w;
    lattice_walk<RM, FAST, false>(W, w, ev_src<E16>(a) + eb, nev, a.trans + (ntr ? tb : 0u), ntr, 1u << a.init_state, m,
                                  budget, want_peak, count);
    if (w.status == 3) return K_SPILL;
    // per-key epilogue (results through `full`); on a failure W / live still
    // hold the set before the failing event, which is what is reported
    const Args &f = *a.full;

    if (!w.in_mem) {
        uint32_t *const mW = m.W + opq_lane(lane);
#pragma unroll
        for (int k = 0; k < RM; ++k) mW[k * 64] = W[k];
    }
    if (!(a.flags & T0_DBG_NOFINAL)) write_final_mem(f, key, m, lane, w.slot_v, w.live);
    const uint32_t pr = __ockl_wfred_add_u32(w.probes);
    if (w.status)
        finish_key(f, key, w.status == 1 ? LC_INVALID : LC_UNKNOWN,
                   w.status == 1 ? LC_CAUSE_NONLIN : LC_CAUSE_BUDGET, (int32_t)w.fev, w.peak, pr,
                   (uint64_t)w.fev + (w.status == 1 ? 1u : 0u));
    else
        finish_key(f, key, LC_VALID, LC_CAUSE_NONE, -1, w.peak, pr, nev);
    return K_DONE;
}

// A key the register tier cannot hold: to the deep or the spill list -- or,
// in a step declared to fit T0 (T0_STRICT), malformed: no later tier runs.
__device__ __forceinline__ void t0_spill(const T0Args &a, int32_t key) {
    const Args &f = *a.full;
    if (a.flags & T0_STRICT) {
        t0_malformed(a, key, LC_BATCH_E_FIT);
        finish_key(f, key, LC_UNKNOWN, LC_CAUSE_ERROR, -1, 0, 0, 0);
    } else {
        const bool deep = f.deep && a.key_width && a.key_width[key] > LC_DIRECT_T3_WIDTH;
        push_list(deep ? f.deep : f.spill, deep ? f.n_deep : f.n_spill, key, f.list_cap);
    }
}

// T0's arguments from a tier's Args (launch_t0, launch_spec).
static T0Args make_t0(const Args &a, const Args *a_dev) {
    T0Args t{};
    t.ev_off = a.ev_off; t.events = a.events; t.trans = a.trans; t.trans_off = a.trans_off;
    t.key_width = a.key_width; t.key_states = a.key_states; t.key_error = a.key_error; t.order = a.order;
    t.ticket = a.ticket;
    t.err = a.err;
    t.err_base = a.err_base;
    t.n_trans = a.n_trans;
    t.lat_ws = a.lat_ws; t.full = a_dev; t.budget = a.budget; t.n_order = a.n_order;
    t.init_state = a.init_state; t.shared_states = a.shared_states;
    t.flags = (a.count_probes ? T0_COUNT : 0u) | (a.peak ? T0_WANT_PEAK : 0u) | (a.final_cfg ? T0_WANT_FINAL : 0u) |
              (a.debug_mode == 2 ? T0_DBG_NOEVENTS : 0u) | (a.debug_mode == 3 ? T0_DBG_NOFINAL : 0u) |
              (a.strict ? T0_STRICT : 0u);
    return t;
}

}  // namespace lcd
