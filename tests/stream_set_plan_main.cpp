// The resident set tier's rules (csrc/stream_plan.hpp) from the command line,
// for tests/test_stream_set_plan.py: the layout constants on the first line,
// the header words on the second, then one line per query read from stdin:
//   f <n_s> <n_i> <slot> <states>  -> falls back
//   o <which>                      -> word offset of S array `which`
#include <cstdio>
#include <iostream>
#include <string>

#include "stream_plan.hpp"

int main() {
    std::printf("%u %u %u %u %u %u %u %llu %llu %u %u\n", lc::STREAM_SET_HDR_WORDS, lc::STREAM_SET_SLOTS, lc::STREAM_SET_OFF_DESC,
                lc::STREAM_SET_OFF_S0, lc::STREAM_SET_OFF_S1, lc::STREAM_SET_REC_WORDS, lc::STREAM_SET_CAP,
                (unsigned long long)lc::STREAM_MIN_BUDGET, (unsigned long long)lc::stream_set_slot_bytes(),
                lc::STREAM_SET_MAX_SLOTS, lc::STREAM_SET_MAX_STATES);
    std::printf("%u %u %u %u %u %u %u %u\n", lc::STREAM_SET_H_STATUS, lc::STREAM_SET_H_NS, lc::STREAM_SET_H_PEND0,
                lc::STREAM_SET_H_PEND1, lc::STREAM_SET_H_DONE, lc::STREAM_SET_H_FAIL, lc::STREAM_SET_H_CUR,
                lc::STREAM_SET_FALLBACK);
    std::string what;
    while (std::cin >> what) {
        unsigned long long a, b;
        unsigned c, d;
        if (what == "f") {
            if (!(std::cin >> a >> b >> c >> d)) return 1;
            std::printf("%d\n", (int)lc::stream_set_falls_back(a, b, c, d));
        } else if (what == "o") {
            if (!(std::cin >> c)) return 1;
            std::printf("%u\n", lc::stream_set_off_s(c));
        } else {
            return 1;
        }
    }
    return 0;
}
