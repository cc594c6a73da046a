// The exact mode's rules (csrc/stream_plan.hpp) from the command line, for
// tests/test_stream_exact_plan.py: the constants on the first line, then one
// line per query read from stdin:
//   b <budget> <exact>               -> the stream accepts the budget
//   f <keys> <max_final> <key> <cfg> -> words per key, offset of the config (64-bit words), array bytes, count bytes
#include <cstdio>
#include <iostream>
#include <string>

#include "stream_plan.hpp"

int main() {
    std::printf("%u %u %u %u %u %u %u %u %llu %u\n", lc::STREAM_HDR_WORDS, lc::STREAM_REC_WORDS, lc::STREAM_H_PEAK,
                lc::STREAM_H_STARTED, lc::STREAM_LIVE, lc::STREAM_INVALID, lc::STREAM_ERROR, lc::STREAM_BUDGET,
                (unsigned long long)lc::STREAM_MIN_BUDGET, lc::STREAM_MAX_FINAL);
    std::printf("%u %u %u %u %u %u %u %u %u %u %u %u\n", lc::STREAM_H_STATUS, lc::STREAM_H_N, lc::STREAM_H_LIVE,
                lc::STREAM_H_IN_MEM, lc::STREAM_H_DIRTY, lc::STREAM_H_DONE, lc::STREAM_H_FAIL, lc::STREAM_H_PEND0,
                lc::STREAM_H_PEND1, lc::STREAM_H_STARTED, lc::STREAM_H_PEAK, lc::STREAM_SET_FALLBACK);
    std::string what;
    while (std::cin >> what) {
        unsigned long long a, b, c, d;
        if (what == "b") {
            if (!(std::cin >> a >> b)) return 1;
            std::printf("%d\n", (int)lc::stream_budget_ok(a, b != 0));
        } else if (what == "f") {
            if (!(std::cin >> a >> b >> c >> d)) return 1;
            std::printf("%llu %llu %llu %llu\n", (unsigned long long)lc::stream_final_words64((uint32_t)b),
                        (unsigned long long)lc::stream_final_off64(c, (uint32_t)b, (uint32_t)d),
                        (unsigned long long)lc::stream_final_bytes(a, (uint32_t)b),
                        (unsigned long long)lc::stream_nfinal_bytes(a));
        } else {
            return 1;
        }
    }
    return 0;
}
