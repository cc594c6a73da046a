// The stream rules (csrc/stream_plan.hpp) from the command line, for
// tests/test_stream_plan.py: the layout constants on the first line, then one
// line per query read from stdin:
//   n <pending> <started> <dead>   -> lattice words, load words, save words, resume phase, in workspace
//   d <slot> <states>              -> defers
#include <cstdio>
#include <iostream>
#include <string>

#include "stream_plan.hpp"

int main() {
    std::printf("%u %u %u %u %u %u %u %u %llu %u\n", lc::STREAM_HDR_WORDS, lc::STREAM_LANE_ARRAYS, lc::STREAM_OFF_LANES,
                lc::STREAM_OFF_LATTICE, lc::STREAM_LATTICE_MAX, lc::STREAM_REC_WORDS, lc::STREAM_MAX_WIDTH,
                lc::STREAM_MAX_STATES, (unsigned long long)lc::STREAM_MIN_BUDGET, lc::STREAM_MAX_DESC);
    std::printf("%u %u %u %u %u %u %u %u %u %u\n", lc::STREAM_H_STATUS, lc::STREAM_H_N, lc::STREAM_H_LIVE,
                lc::STREAM_H_IN_MEM, lc::STREAM_H_DIRTY, lc::STREAM_H_DONE, lc::STREAM_H_FAIL, lc::STREAM_H_PEND0,
                lc::STREAM_H_PEND1, lc::STREAM_H_STARTED);
    std::string what;
    while (std::cin >> what) {
        unsigned a, b, c;
        if (what == "n") {
            if (!(std::cin >> a >> b >> c)) return 1;
            std::printf("%u %u %u %d %d\n", lc::stream_lattice_words(a), lc::stream_load_words(a, b != 0),
                        lc::stream_save_words(a, c != 0), lc::stream_resume_phase(a), (int)lc::stream_in_workspace(a));
        } else if (what == "d") {
            if (!(std::cin >> a >> b)) return 1;
            std::printf("%d\n", (int)lc::stream_defers(a, b));
        } else {
            return 1;
        }
    }
    return 0;
}
