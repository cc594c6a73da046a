// queue_stream_plan.hpp -- the sizing rules of a streaming total-queue /
// unique-ids' resident hash table (lc_queue_stream_*), as pure functions.  Host
// C++ only (no HIP): pinned on the CPU by tests/test_queue_stream_plan.py
// through tests/queue_stream_plan_main.cpp.
//
// The table is open-addressed with linear probing and a power-of-two slot
// count, QSP_SLOT_BYTES per slot (device_queue_stream.hpp has the slot).  An
// append of `rows` packed rows adds at most `rows` distinct (key, value) to
// the `resident` ones the table holds.
//   qsp_first_slots   lc_queue_stream_opts.slots to the table's first size: 0
//                     is QSP_DEFAULT_SLOTS; otherwise a power of two, else
//                     QSP_BAD_SLOTS
//   qsp_must_grow     before an append: slots < resident + rows (the append
//                     could overflow the table), or slots < 2 x resident (what
//                     the table holds already passes the load factor of 1/2
//                     that queue_plan.hpp's QP_SLOTS_PER_ROW stands for).  A
//                     table with room for the append at no more than half full
//                     BEFORE it is left alone: an append may fill it to the
//                     last slot, and the next one grows it
//   qsp_grown_slots   the next power of two at or above 2 x (resident + rows):
//                     the bound restored for the append at its worst.  Where
//                     that passes the byte cap, the largest table the cap
//                     admits if the append cannot overflow it; else
//                     QSP_BAD_SLOTS: the append is refused (LC_E_NOMEM)
//   qsp_pieces        an append of more than QSP_LAUNCH_ROWS packed rows is
//                     tallied and settled in pieces of at most that many: a
//                     slot's state word names a row of the piece in flight.
//                     Pieces are equal but for the last: piece i holds rows
//                     [i x QSP_LAUNCH_ROWS, min(rows, (i + 1) x QSP_LAUNCH_ROWS))
//   qsp_key_cap       the capacity of the per-key words, doubled as keys appear
#pragma once

#include <cstdint>

namespace lcqs {

constexpr uint32_t QSP_BLOCK = 256;                // threads per workgroup, every kernel
constexpr uint32_t QSP_SLOT_BYTES = 48;            // three 16-byte words
constexpr uint32_t QSP_SLOTS_PER_VALUE = 2;        // load factor <= 1/2 after a grow
constexpr uint64_t QSP_MAX_BYTES = 8ull << 30;     // the table's byte cap
constexpr uint64_t QSP_MAX_SLOTS = 1ull << 27;     // the largest power of two within it (6 GiB)
constexpr uint64_t QSP_DEFAULT_SLOTS = 1ull << 16; // 3 MiB
constexpr uint64_t QSP_LAUNCH_ROWS = 1ull << 24;   // packed rows of one tally launch (and of its staging)
constexpr uint64_t QSP_MAX_ROWS = 0xFFFFFFFFull;   // a stream's packed rows stay below 2^32
constexpr uint64_t QSP_BAD_SLOTS = 0;

static_assert(QSP_MAX_SLOTS * QSP_SLOT_BYTES <= QSP_MAX_BYTES && 2 * QSP_MAX_SLOTS * QSP_SLOT_BYTES > QSP_MAX_BYTES, "the cap");

inline uint64_t qsp_pow2_at_least(uint64_t x) {
    uint64_t p = 1;
    while (p < x) p <<= 1;  // (callers keep x at or below 2^63)
    return p;
}

inline uint64_t qsp_bytes(uint64_t slots) { return slots * QSP_SLOT_BYTES; }

inline uint64_t qsp_first_slots(uint32_t asked) {
    if (asked == 0) return QSP_DEFAULT_SLOTS;
    if ((asked & (asked - 1)) != 0 || asked > QSP_MAX_SLOTS) return QSP_BAD_SLOTS;
    return asked;
}

// resident, rows < 2^32 each (the stream's size rule), so nothing here overflows.
inline bool qsp_must_grow(uint64_t slots, uint64_t resident, uint64_t rows) {
    return slots < resident + rows || slots < QSP_SLOTS_PER_VALUE * resident;
}

inline uint64_t qsp_grown_slots(uint64_t resident, uint64_t rows) {
    const uint64_t need = resident + rows;
    const uint64_t want = qsp_pow2_at_least(QSP_SLOTS_PER_VALUE * need);
    if (want <= QSP_MAX_SLOTS) return want;
    return need <= QSP_MAX_SLOTS ? QSP_MAX_SLOTS : QSP_BAD_SLOTS;
}

inline uint64_t qsp_pieces(uint64_t rows, uint64_t limit = QSP_LAUNCH_ROWS) { return rows / limit + (rows % limit != 0); }
inline uint64_t qsp_piece_begin(uint64_t i, uint64_t rows, uint64_t limit = QSP_LAUNCH_ROWS) {
    const uint64_t b = i * limit;
    return b < rows ? b : rows;
}

// The per-key words on the device hold `have` keys (0: none yet) and `need`
// are wanted: QSP_KEYS0 at first, then doubled until they fit.
constexpr uint64_t QSP_KEYS0 = 64;
inline uint64_t qsp_key_cap(uint64_t have, uint64_t need) {
    uint64_t c = have ? have : QSP_KEYS0;
    while (c < need) c <<= 1;
    return c;
}

// One lane per row, per slot, per word.
inline uint64_t qsp_blocks(uint64_t n) { return n / QSP_BLOCK + (n % QSP_BLOCK != 0); }

}  // namespace lcqs
