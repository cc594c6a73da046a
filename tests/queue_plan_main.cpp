// qp_default_slots / qp_slots_of / qp_bytes / qp_fits / qp_blocks
// (csrc/queue_plan.hpp) from the command line, for tests/test_queue_plan.py.
// stdin, one request per line:
//   default n_rows      -> "slots bytes fits blocks"
//   slots asked n_rows  -> "slots fits"   (slots 0: refused)
//   consts              -> "block slot_bytes slots_per_row max_bytes"
#include <cstdio>
#include <iostream>
#include <string>

#include "queue_plan.hpp"

int main() {
    std::string what;
    while (std::cin >> what) {
        if (what == "default") {
            unsigned long long n;
            std::cin >> n;
            const uint64_t s = lcq::qp_default_slots(n);
            std::printf("%llu %llu %d %llu\n", (unsigned long long)s, (unsigned long long)lcq::qp_bytes(s), (int)lcq::qp_fits(s),
                        (unsigned long long)lcq::qp_blocks(s));
        } else if (what == "slots") {
            unsigned asked;
            unsigned long long n;
            std::cin >> asked >> n;
            const uint64_t s = lcq::qp_slots_of(asked, n);
            std::printf("%llu %d\n", (unsigned long long)s, (int)(s != lcq::QP_BAD_SLOTS && lcq::qp_fits(s)));
        } else if (what == "consts") {
            std::printf("%u %u %u %llu\n", lcq::QP_BLOCK, lcq::QP_SLOT_BYTES, lcq::QP_SLOTS_PER_ROW, (unsigned long long)lcq::QP_MAX_BYTES);
        } else {
            return 1;
        }
        if (!std::cin) return 1;
    }
    return 0;
}
