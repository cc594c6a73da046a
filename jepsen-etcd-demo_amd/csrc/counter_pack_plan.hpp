// counter_pack_plan.hpp -- what the host and the device half of
// lc_counter_check_history share: the codes and texts of a key's error and the
// word a key's lowest offence is kept in.  Host C++ only (no HIP): pinned on the
// CPU by tests/test_counter_pack_plan.py through tests/counter_pack_plan_main.cpp,
// and the texts against lc_counter_pack's by tests/test_counter_device_pack_abi.py.
//
// lc_counter_pack's serial fold, made local: with a
// key's client rows grouped by process in history order, what the fold knows
// of a process before a row is decided by the row before it in its group -- an
// invocation is open exactly when that row is an invocation -- as long as no
// earlier row of the key was an offence.  So every row judges itself from its
// predecessor, and the key's error is the offence at its lowest row: the fold
// stops at that row and never sees the later ones.  An offence is the word
// (row << CP_CODE_BITS) | code, and a key's error the minimum of its words.
#pragma once

#include <cstdint>

namespace lccp {

// rule 1 (pairing), then rule 3 (values), in the order lc_counter_pack tests them
enum : uint32_t {
    CP_SECOND_INVOKE = 1,
    CP_NO_OPEN = 2,
    CP_OTHER_F = 3,
    CP_READ_NIL = 4,
    CP_ADD_NIL = 5,
    CP_ADD_NEGATIVE = 6,
    CP_SUM = 7,
    CP_CODES = 8,
};

constexpr uint32_t CP_CODE_BITS = 3;
constexpr uint64_t CP_NO_ERROR = ~0ull;
constexpr uint8_t CP_NO_EVENT = 0xFF;  // a position that yields no event

constexpr uint64_t cp_word(uint64_t row, uint32_t code) { return (row << CP_CODE_BITS) | code; }
inline uint64_t cp_word_row(uint64_t w) { return w >> CP_CODE_BITS; }
inline uint32_t cp_word_code(uint64_t w) { return (uint32_t)(w & ((1u << CP_CODE_BITS) - 1)); }

// lc_counter_pack's messages, word for word (csrc/host_counter.cpp).
inline const char *cp_error_text(uint32_t code) {
    switch (code) {
        case CP_SECOND_INVOKE: return "a second invocation by a process that has one open";
        case CP_NO_OPEN: return "a completion by a process with no open invocation";
        case CP_OTHER_F: return "a completion whose :f is not its invocation's";
        case CP_READ_NIL: return "an :ok :read whose value is nil or not an integer";
        case CP_ADD_NIL: return "an :add whose value is nil or not an integer";
        case CP_ADD_NEGATIVE: return "an :add of a negative value";
        case CP_SUM: return "the adds sum past the largest 64-bit integer";
        default: return nullptr;
    }
}

// The running sum of a key's LC_CE_UP values is scanned as two plain sums, of
// the values' low 32 bits and of their high 31 (each below 2^63 over a batch
// of fewer than 2^31 rows).  The key's sum up to an event is d_hi * 2^32 +
// d_lo from the differences against the key's start: it passes INT64_MAX
// exactly when d_hi + (d_lo >> 32) reaches 2^31.
constexpr bool cp_sum_past_int64(uint64_t d_lo, uint64_t d_hi) { return d_hi + (d_lo >> 32) >= (1ull << 31); }

}  // namespace lccp
