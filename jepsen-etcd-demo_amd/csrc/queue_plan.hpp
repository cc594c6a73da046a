// queue_plan.hpp -- the sizing rules of lc_queue_check's hash table, as pure
// functions of a batch's row count.  Host C++ only (no HIP): pinned on the CPU
// by tests/test_queue_plan.py through tests/queue_plan_main.cpp.
//
// The table is open-addressed with linear probing, QP_SLOT_BYTES per slot: the
// index of a representative row and three 32-bit tallies.  Its slot count is a
// power of two, so that a hash is reduced by a mask, and at least the batch's
// row count, so that it can never overflow: a batch has at most one distinct
// (key, value) per row.
//   qp_default_slots  the next power of two at or above 2 x n_rows (a load
//                     factor of at most 1/2), and at least one workgroup's
//                     worth
//   qp_slots_of       lc_queue_opts.slots to the slots used: 0 is the default;
//                     otherwise a power of two >= n_rows, else QP_BAD_SLOTS
//   qp_bytes          slots x QP_SLOT_BYTES; a table above QP_MAX_BYTES is
//                     refused
#pragma once

#include <cstdint>

namespace lcq {

constexpr uint32_t QP_BLOCK = 256;             // threads per workgroup, every queue kernel
constexpr uint32_t QP_SLOT_BYTES = 16;         // {rep, tally[3]}: one 16-byte store resets a slot
constexpr uint32_t QP_SLOTS_PER_ROW = 2;       // the default: load factor <= 1/2
constexpr uint64_t QP_MAX_BYTES = 8ull << 30;  // the table's byte cap: 2^29 slots
constexpr uint64_t QP_MAX_SLOTS = QP_MAX_BYTES / QP_SLOT_BYTES;
constexpr uint64_t QP_BAD_SLOTS = 0;
constexpr uint32_t QP_EMPTY = 0xFFFFFFFFu;     // a slot's word before a row claims it

inline uint64_t qp_pow2_at_least(uint64_t x) {
    uint64_t p = 1;
    while (p < x) p <<= 1;  // (callers keep x at or below 2^63)
    return p;
}

inline uint64_t qp_default_slots(uint64_t n_rows) {
    if (n_rows > (1ull << 61)) return 1ull << 63;
    const uint64_t s = qp_pow2_at_least(QP_SLOTS_PER_ROW * n_rows);
    return s < QP_BLOCK ? QP_BLOCK : s;
}

inline uint64_t qp_slots_of(uint32_t asked, uint64_t n_rows) {
    if (asked == 0) return qp_default_slots(n_rows);
    if ((asked & (asked - 1)) != 0 || asked < n_rows) return QP_BAD_SLOTS;
    return asked;
}

inline uint64_t qp_bytes(uint64_t slots) { return slots > (~0ull) / QP_SLOT_BYTES ? ~0ull : slots * QP_SLOT_BYTES; }
inline bool qp_fits(uint64_t slots) { return slots <= QP_MAX_SLOTS; }

// One lane per row, one lane per slot.
inline uint64_t qp_blocks(uint64_t n) { return n / QP_BLOCK + (n % QP_BLOCK != 0); }

}  // namespace lcq
