// A resident, resumable register-tier search (lc_stream_*):
// the per-key state record k_stream (device_stream_lattice.hip) loads and stores,
// which of its words a load or a save touches, the phase a resumed walk
// enters, and when a key leaves the stream for the batch path -- as pure
// functions of plain values, tested without a GPU (tests/test_stream_plan.py).
// No HIP here.
//
// A record is lattice_walk's state between two events of a key: the ops
// pending (their transfers and window slots, one lane per op index), the
// lattice W[L] over the subsets of those ops, and the two words of the slot
// protocol (validate_chunk) carried from chunk to chunk.
#pragma once

#include <cstdint>

namespace lc {

// ---- record layout, in 32-bit words -------------------------------------------
constexpr uint32_t STREAM_HDR_WORDS = 16;
// header words
constexpr uint32_t STREAM_H_STATUS = 0;   // STREAM_LIVE / _INVALID / _ERROR
constexpr uint32_t STREAM_H_N = 1;        // ops pending
constexpr uint32_t STREAM_H_LIVE = 2;     // occupied op indices
constexpr uint32_t STREAM_H_IN_MEM = 3;   // the lattice is wider than the compact build's 4 registers
constexpr uint32_t STREAM_H_DIRTY = 4;    // an op was invoked since the lattice was last closed
constexpr uint32_t STREAM_H_DONE = 5;     // events searched so far
constexpr uint32_t STREAM_H_FAIL = 6;     // STREAM_INVALID: ordinal of the failing :ok in the key's stream
constexpr uint32_t STREAM_H_PEND0 = 7;    // window slots 0..31 pending (the slot protocol)
constexpr uint32_t STREAM_H_PEND1 = 8;    // window slots 32..63
constexpr uint32_t STREAM_H_STARTED = 9;  // 0: a fresh (zero-filled) record, the walk starts from the initial state
constexpr uint32_t STREAM_H_PEAK = 10;    // exact mode: the largest config set so far (a fresh record counts as 1)
static_assert(STREAM_H_PEAK < STREAM_HDR_WORDS, "the header's spare words hold the peak");
// per-op lane arrays of the walk, 64 lanes each, in this order
constexpr uint32_t STREAM_LANE_ARRAYS = 5;  // k_v, cap_v, b_v, slot_v, dense_v
constexpr uint32_t STREAM_OFF_LANES = STREAM_HDR_WORDS;
constexpr uint32_t STREAM_OFF_LATTICE = STREAM_OFF_LANES + STREAM_LANE_ARRAYS * 64;
constexpr uint32_t STREAM_LATTICE_MAX = 1024;  // 10 ops pending: 16 registers x 64 lanes
constexpr uint32_t STREAM_REC_WORDS = STREAM_OFF_LATTICE + STREAM_LATTICE_MAX;

constexpr uint32_t STREAM_LIVE = 0, STREAM_INVALID = 1, STREAM_ERROR = 2;
// exact mode (LC_STREAM_EXACT): a set or a closure passed the context's budget
// at event STREAM_H_FAIL.  (3 is the set record's STREAM_SET_FALLBACK.)
constexpr uint32_t STREAM_BUDGET = 4;

// the register tier's reach (lattice_core.hpp T0_MAX_WIDTH / T0_MAX_STATES)
constexpr uint32_t STREAM_MAX_WIDTH = 10;
constexpr uint32_t STREAM_MAX_STATES = 32;
// the least budget at which the FAST walk's sets are exact: no lattice holds
// more than 16 registers x 64 lanes x 32 states
constexpr uint64_t STREAM_MIN_BUDGET = 16ull * 64 * 32;
// Budgets a stream accepts: the exact walk holds Knossos's own sets and counts
// them, so any; the FAST walk's closed sets only where no set can pass it.
constexpr bool stream_budget_ok(uint64_t budget, bool exact) { return exact || budget >= STREAM_MIN_BUDGET; }

// ---- exact mode: the final configs of a stream's keys --------------------------
// Two arrays in device memory beside the records, grown with them: max_final
// configs of two 64-bit words per key (write_final_mem's record: the slot
// mask's low word; state << 48 | its high bits), and a count per key.
constexpr uint32_t STREAM_MAX_FINAL = 16;  // lc_opts.max_final at most
constexpr uint64_t stream_final_words64(uint32_t max_final) { return 2ull * max_final; }  // per key
constexpr uint64_t stream_final_off64(uint64_t key, uint32_t max_final, uint32_t cfg) {
    return (key * max_final + cfg) * 2;
}
constexpr uint64_t stream_final_bytes(uint64_t keys, uint32_t max_final) { return keys * stream_final_words64(max_final) * 8; }
constexpr uint64_t stream_nfinal_bytes(uint64_t keys) { return keys * 4; }

// Lattice words of a key with n ops pending: one register (64 lanes) up to 6,
// doubling with every op beyond; word k * 64 + lane = register k of the lane.
constexpr uint32_t stream_lattice_words(uint32_t n) { return 64u << (n > 6 ? (n > 10 ? 4 : n - 6) : 0); }

// Words a wave reads when it loads a record whose header says n ops pending
// (the header is read first, then the lane arrays and the lattice rows in
// use), and the words it writes when it stores one.  A key that died in this
// call stores its header alone: its set is no longer followed.
constexpr uint32_t stream_load_words(uint32_t n, bool started) {
    return STREAM_HDR_WORDS + (started ? STREAM_LANE_ARRAYS * 64 + stream_lattice_words(n) : 0);
}
constexpr uint32_t stream_save_words(uint32_t n, bool dead) {
    return STREAM_HDR_WORDS + (dead ? 0 : STREAM_LANE_ARRAYS * 64 + stream_lattice_words(n));
}

// The phase of lattice_walk a resume enters: the lane phase (0) with at most
// 6 ops pending -- a 7th invoke then moves it to the dense phase as in an
// unbroken walk -- and the dense phase (1) from 7 up, where op indices are
// dense and the lattice is in registers 0..3 (7, 8) or the workspace (9, 10).
constexpr int stream_resume_phase(uint32_t n) { return n >= 7 ? 1 : 0; }
constexpr bool stream_in_workspace(uint32_t n) { return n >= 9; }

// Deferral: an invoke that would take window slot `slot` or intern the key's
// `states`-th state (nil included) ends the key's time on the device; from
// that event on its words stay on the host and lc_stream_finish checks the
// key once through the batch path.
constexpr bool stream_defers(uint32_t slot, uint32_t states) {
    return slot >= STREAM_MAX_WIDTH || states > STREAM_MAX_STATES;
}

// A register-tier key's descriptors at most: the read of anything, reads,
// writes and cas pairs over 32 states (the streaming packer interns every
// value an op names, so none carries LC_STATE_NONE) -- all below the 2,048 of
// a 16-bit event word.
constexpr uint32_t STREAM_MAX_DESC = 1 + 32 + 32 + 32 * 32;

// ---- the resident set tier (LC_STREAM_SET_TIER; device_stream_set.hip) ---------
// A key that leaves the register tier keeps being searched from a set record
// in device memory: the JIT search's config set S between two events, in the
// narrow form of device_search.hip (state << 56 | window-slot bits of the ops
// linearized and still pending), and each pending op's descriptor by window
// slot.  The record, in 32-bit words: a header, 64 descriptors, two S arrays
// of STREAM_SET_CAP u64 configs that an :ok reads and writes in turn.
constexpr uint32_t STREAM_SET_HDR_WORDS = 16;
constexpr uint32_t STREAM_SET_H_STATUS = 0;  // STREAM_LIVE / _INVALID / _ERROR / STREAM_SET_FALLBACK
constexpr uint32_t STREAM_SET_H_NS = 1;      // configs in the current S array
constexpr uint32_t STREAM_SET_H_PEND0 = 2;   // window slots 0..31 pending
constexpr uint32_t STREAM_SET_H_PEND1 = 3;   // window slots 32..63
constexpr uint32_t STREAM_SET_H_DONE = 4;    // events searched so far (register tier's included)
constexpr uint32_t STREAM_SET_H_FAIL = 5;    // STREAM_INVALID: ordinal of the failing :ok in the key's stream
constexpr uint32_t STREAM_SET_H_CUR = 6;     // which S array is current (0 / 1)
constexpr uint32_t STREAM_SET_FALLBACK = 3;  // status: the key left the set tier for lc_stream_finish

constexpr uint32_t STREAM_SET_SLOTS = 64;    // descriptors, one per window slot
// Configs per S array, and the most the closure I of one :ok may hold.  At
// most the smallest budget a stream accepts, so that a one-shot check that
// gives up at its budget is never answered by the set tier;
// at least a full register-tier lattice, so that every migration fits.
constexpr uint32_t STREAM_SET_CAP = 32768;
static_assert(STREAM_SET_CAP <= STREAM_MIN_BUDGET, "the set tier's cap is at most the least budget of a stream");
static_assert(STREAM_SET_CAP >= STREAM_LATTICE_MAX * STREAM_MAX_STATES, "a full lattice migrates without loss");

constexpr uint32_t STREAM_SET_OFF_DESC = STREAM_SET_HDR_WORDS;
constexpr uint32_t STREAM_SET_OFF_S0 = STREAM_SET_OFF_DESC + STREAM_SET_SLOTS;
constexpr uint32_t STREAM_SET_OFF_S1 = STREAM_SET_OFF_S0 + 2 * STREAM_SET_CAP;
constexpr uint32_t STREAM_SET_REC_WORDS = STREAM_SET_OFF_S1 + 2 * STREAM_SET_CAP;
static_assert(STREAM_SET_OFF_S0 % 2 == 0 && STREAM_SET_REC_WORDS % 2 == 0, "the S arrays are 8-byte aligned");
constexpr uint32_t stream_set_off_s(uint32_t which) { return which ? STREAM_SET_OFF_S1 : STREAM_SET_OFF_S0; }
// One slot of the set-record pool, bytes.
constexpr uint64_t stream_set_slot_bytes() { return (uint64_t)STREAM_SET_REC_WORDS * 4; }

// The narrow config's reach (include/lincheck.h LC_NARROW_MAX_SLOTS / _STATES).
constexpr uint32_t STREAM_SET_MAX_SLOTS = 56;
constexpr uint32_t STREAM_SET_MAX_STATES = 255;

// Fallback: a migrated key returns to deferral -- its record is released and
// lc_stream_finish checks it once, from its first event -- when an :ok's S'
// (n_s) or closure I (n_i) would pass the cap, an invoke takes window slot
// `slot` at or past the narrow form's, or the key has interned `states`
// states, more than a narrow config's state field holds.
constexpr bool stream_set_falls_back(uint64_t n_s, uint64_t n_i, uint32_t slot, uint32_t states) {
    return n_s > STREAM_SET_CAP || n_i > STREAM_SET_CAP || slot >= STREAM_SET_MAX_SLOTS || states > STREAM_SET_MAX_STATES;
}

// ---- the exact set tier (LC_STREAM_EXACT | LC_STREAM_SET_TIER; device_stream_set_exact.hip)
// An exact register record holds Knossos's own S, so the set that migrates is
// S itself and every |I| and |S'| of k_stream_set's step is the oracle's.  The
// set record keeps its layout and gains no word: the key's running peak stays
// where k_stream_exact left it, in its register record's STREAM_H_PEAK -- the
// register record is idle once the key has migrated -- and k_stream_set_exact
// reads it before a key's new words and stores it after them, so
// stream_dev_peaks and a dead key's Final read one place for both tiers.
//
// What an :ok at event e decides, in the oracle's order (table_full: a hash
// set took no more entries; n_i = |I|, n_s = |S'|).  The kernel's counts are
// exact while they are at most the cap; past it they only say "past the cap"
// (an entry beyond an array's end leaves its hash set again and may be counted
// twice, and the closure stops past stream_set_closure_stop), so the kernel
// passes stream_set_exact_count of each.  A budget above the cap thus meets the
// cap first: the key falls back and the batch path meets the budget.
constexpr uint64_t stream_set_exact_count(uint64_t counted) {
    return counted > STREAM_SET_CAP ? (uint64_t)STREAM_SET_CAP + 1 : counted;
}
constexpr uint32_t stream_set_exact_decide(bool table_full, uint64_t n_i, uint64_t n_s, uint64_t budget) {
    return table_full                ? STREAM_ERROR
           : n_i > budget            ? STREAM_BUDGET
           : n_i > STREAM_SET_CAP    ? STREAM_SET_FALLBACK
           : n_s == 0                ? STREAM_INVALID
           : n_s > budget            ? STREAM_BUDGET
           : n_s > STREAM_SET_CAP    ? STREAM_SET_FALLBACK
                                     : STREAM_LIVE;
}
// |I| past which the closure need not go on: the decision is made either way.
constexpr uint32_t stream_set_closure_stop(uint64_t budget) {
    return budget < STREAM_SET_CAP ? (uint32_t)budget : STREAM_SET_CAP;
}
// Final configs of a set-tier key: the max_final smallest in (slot mask, state
// id) order, write_final_mem's canonical choice.  A narrow config is
// state << 56 | mask, so that order is the config's rotated left by 8 bits.
constexpr uint64_t stream_set_sort_key(uint64_t cfg) { return cfg << 8 | cfg >> 56; }
constexpr uint64_t stream_set_sort_key_cfg(uint64_t key) { return key >> 8 | key << 56; }

}  // namespace lc
