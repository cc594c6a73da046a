// csp_first_reads / csp_reads_cap / csp_refuses / csp_launch_events /
// csp_pieces / csp_patch_threads (csrc/counter_stream_plan.hpp) from the
// command line, for tests/test_counter_stream_plan.py.  stdin, one request per
// line:
//   first asked                        -> "capacity"         (0: refused)
//   cap have need                      -> "capacity"         (0: past the byte cap, refused)
//   refuses reads events ok_reads rows -> "0 | 1 | 2"
//   launch asked tile                  -> "events"
//   pieces events limit                -> "n b0 b1 ... bn"   (the pieces' bounds)
//   patch reads min_r0 patches         -> "threads blocks"
//   consts                             -> "block read_bytes max_bytes max_reads default_reads launch_events limit"
#include <cstdio>
#include <iostream>
#include <string>

#include "counter_stream_plan.hpp"

int main() {
    using namespace lccs;
    typedef unsigned long long ull;
    std::string what;
    while (std::cin >> what) {
        if (what == "first") {
            unsigned asked;
            std::cin >> asked;
            std::printf("%llu\n", (ull)csp_first_reads(asked));
        } else if (what == "cap") {
            ull have, need;
            std::cin >> have >> need;
            std::printf("%llu\n", (ull)csp_reads_cap(have, need));
        } else if (what == "refuses") {
            ull reads, events, oks, rows;
            std::cin >> reads >> events >> oks >> rows;
            std::printf("%d\n", csp_refuses(reads, events, oks, rows));
        } else if (what == "launch") {
            unsigned asked, tile;
            std::cin >> asked >> tile;
            std::printf("%llu\n", (ull)csp_launch_events(asked, tile));
        } else if (what == "pieces") {
            ull events, limit;
            std::cin >> events >> limit;
            const uint64_t n = csp_pieces(events, limit);
            std::printf("%llu", (ull)n);
            for (uint64_t i = 0; i <= n; ++i) std::printf(" %llu", (ull)csp_piece_begin(i, events, limit));
            std::printf("\n");
        } else if (what == "patch") {
            ull reads, min_r0, patches;
            std::cin >> reads >> min_r0 >> patches;
            const uint64_t t = csp_patch_threads(reads, min_r0, patches);
            std::printf("%llu %llu\n", (ull)t, (ull)csp_blocks(t));
        } else if (what == "consts") {
            std::printf("%u %u %llu %llu %llu %llu %llu\n", CSP_BLOCK, CSP_READ_BYTES, (ull)CSP_MAX_BYTES, (ull)CSP_MAX_READS,
                        (ull)CSP_DEFAULT_READS, (ull)CSP_LAUNCH_EVENTS, (ull)CSP_LIMIT);
        } else {
            return 1;
        }
        if (!std::cin) return 1;
    }
    return 0;
}
