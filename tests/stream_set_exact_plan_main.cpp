// The exact set tier's rules (csrc/stream_plan.hpp) from the command line, for
// tests/test_stream_set_exact_plan.py.  First line: the set record's header
// words, its size, the cap, the register record's peak word and header size,
// and the five statuses (live, invalid, error, fallback, budget).  Then one
// line per query read from stdin:
//   d <table_full> <n_i> <n_s> <budget>  -> the :ok's decision (a status)
//   c <budget>                           -> |I| past which the closure may stop
//   n <counted>                          -> the size the kernel may claim from a count
//   k <config>                           -> its sort key
//   u <sort key>                         -> the config back
#include <cstdio>
#include <iostream>
#include <string>

#include "stream_plan.hpp"

int main() {
    std::printf("%u %u %u %u %u %u %u %u %u %u %u\n", lc::STREAM_SET_HDR_WORDS, lc::STREAM_SET_H_CUR, lc::STREAM_SET_REC_WORDS,
                lc::STREAM_SET_CAP, lc::STREAM_H_PEAK, lc::STREAM_HDR_WORDS, lc::STREAM_LIVE, lc::STREAM_INVALID,
                lc::STREAM_ERROR, lc::STREAM_SET_FALLBACK, lc::STREAM_BUDGET);
    std::string what;
    while (std::cin >> what) {
        unsigned long long a, b, c;
        unsigned t;
        if (what == "d") {
            if (!(std::cin >> t >> a >> b >> c)) return 1;
            std::printf("%u\n", lc::stream_set_exact_decide(t != 0, a, b, c));
        } else if (what == "c") {
            if (!(std::cin >> a)) return 1;
            std::printf("%u\n", lc::stream_set_closure_stop(a));
        } else if (what == "n") {
            if (!(std::cin >> a)) return 1;
            std::printf("%llu\n", (unsigned long long)lc::stream_set_exact_count(a));
        } else if (what == "k") {
            if (!(std::cin >> a)) return 1;
            std::printf("%llu\n", (unsigned long long)lc::stream_set_sort_key(a));
        } else if (what == "u") {
            if (!(std::cin >> a)) return 1;
            std::printf("%llu\n", (unsigned long long)lc::stream_set_sort_key_cfg(a));
        } else {
            return 1;
        }
    }
    return 0;
}
