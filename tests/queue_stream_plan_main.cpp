// qsp_first_slots / qsp_must_grow / qsp_grown_slots / qsp_pieces / qsp_key_cap
// (csrc/queue_stream_plan.hpp) from the command line, for
// tests/test_queue_stream_plan.py.  stdin, one request per line:
//   first asked                 -> "slots"            (0: refused)
//   grow slots resident rows    -> "must_grow grown"  (grown 0: past the byte cap, refused)
//   pieces rows limit           -> "n b0 b1 ... bn"   (the pieces' bounds)
//   keys have need              -> "capacity"
//   consts                      -> "block slot_bytes slots_per_value max_bytes max_slots default_slots launch_rows max_rows keys0"
#include <cstdio>
#include <iostream>
#include <string>

#include "queue_stream_plan.hpp"

int main() {
    using namespace lcqs;
    std::string what;
    while (std::cin >> what) {
        if (what == "first") {
            unsigned asked;
            std::cin >> asked;
            std::printf("%llu\n", (unsigned long long)qsp_first_slots(asked));
        } else if (what == "grow") {
            unsigned long long slots, resident, rows;
            std::cin >> slots >> resident >> rows;
            std::printf("%d %llu\n", (int)qsp_must_grow(slots, resident, rows), (unsigned long long)qsp_grown_slots(resident, rows));
        } else if (what == "pieces") {
            unsigned long long rows, limit;
            std::cin >> rows >> limit;
            const uint64_t n = qsp_pieces(rows, limit);
            std::printf("%llu", (unsigned long long)n);
            for (uint64_t i = 0; i <= n; ++i) std::printf(" %llu", (unsigned long long)qsp_piece_begin(i, rows, limit));
            std::printf("\n");
        } else if (what == "keys") {
            unsigned long long have, need;
            std::cin >> have >> need;
            std::printf("%llu\n", (unsigned long long)qsp_key_cap(have, need));
        } else if (what == "consts") {
            std::printf("%u %u %u %llu %llu %llu %llu %llu %llu\n", QSP_BLOCK, QSP_SLOT_BYTES, QSP_SLOTS_PER_VALUE,
                        (unsigned long long)QSP_MAX_BYTES, (unsigned long long)QSP_MAX_SLOTS, (unsigned long long)QSP_DEFAULT_SLOTS,
                        (unsigned long long)QSP_LAUNCH_ROWS, (unsigned long long)QSP_MAX_ROWS, (unsigned long long)QSP_KEYS0);
        } else {
            return 1;
        }
        if (!std::cin) return 1;
    }
    return 0;
}
