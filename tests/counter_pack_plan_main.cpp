// The sizing rules of lc_counter_check_history's device pack on the CPU
// (tests/test_counter_pack_plan.py): csrc/rows_plan.hpp and
// csrc/counter_pack_plan.hpp, which are host C++ without HIP.  Reads commands
// from standard input, one per line, and answers each with one line:
//   rows N        slots, blocks of rows, tiles, blocks of slots
//   bits MAX      rp_bits(MAX)
//   hash KEY      rp_hash(KEY) (decimal, unsigned)
//   sort N        bits of the key sort and of the process sort when every row
//                 of N is a key and a process of its own, and the limit
//   word ROW CODE the error word, and the row and code read back from it
//   sum LO HI     cp_sum_past_int64
//   text CODE     the message, or "-"
//   consts        block, items per thread, tile, largest n, slot bytes, none, codes
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "counter_pack_plan.hpp"
#include "rows_plan.hpp"

int main() {
    char cmd[32];
    while (std::scanf("%31s", cmd) == 1) {
        uint64_t a = 0, b = 0;
        if (!std::strcmp(cmd, "rows")) {
            if (std::scanf("%" SCNu64, &a) != 1) return 1;
            const uint64_t s = lcr::rp_slots(a);
            std::printf("%" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", s, lcr::rp_blocks(a), lcr::rp_tiles(a), lcr::rp_blocks(s));
        } else if (!std::strcmp(cmd, "bits")) {
            if (std::scanf("%" SCNu64, &a) != 1) return 1;
            std::printf("%u\n", lcr::rp_bits(a));
        } else if (!std::strcmp(cmd, "hash")) {
            if (std::scanf("%" SCNu64, &a) != 1) return 1;
            std::printf("%" PRIu64 "\n", lcr::rp_hash(a));
        } else if (!std::strcmp(cmd, "sort")) {
            if (std::scanf("%" SCNu64, &a) != 1) return 1;
            // key indices run 0 .. K (K: takes no part) with K <= n; process indices 0 .. P - 1 with P <= n
            std::printf("%u %u %u\n", lcr::rp_bits(a), lcr::rp_bits(a ? a - 1 : 0), lcr::RP_SORT_BITS_MAX);
        } else if (!std::strcmp(cmd, "word")) {
            if (std::scanf("%" SCNu64 " %" SCNu64, &a, &b) != 2) return 1;
            const uint64_t w = lccp::cp_word(a, (uint32_t)b);
            std::printf("%" PRIu64 " %" PRIu64 " %u %d\n", w, lccp::cp_word_row(w), lccp::cp_word_code(w), w < lccp::CP_NO_ERROR);
        } else if (!std::strcmp(cmd, "sum")) {
            if (std::scanf("%" SCNu64 " %" SCNu64, &a, &b) != 2) return 1;
            std::printf("%d\n", lccp::cp_sum_past_int64(a, b) ? 1 : 0);
        } else if (!std::strcmp(cmd, "text")) {
            if (std::scanf("%" SCNu64, &a) != 1) return 1;
            const char *t = lccp::cp_error_text((uint32_t)a);
            std::printf("%s\n", t ? t : "-");
        } else if (!std::strcmp(cmd, "consts")) {
            std::printf("%u %u %u %" PRIu64 " %u %u %u\n", lcr::RP_BLOCK, lcr::RP_IPT, lcr::RP_TILE, lcr::RP_MAX_ROWS, lcr::RP_SLOT_BYTES,
                        lcr::RP_NONE, (unsigned)lccp::CP_CODES);
        } else {
            return 2;
        }
    }
    return 0;
}
