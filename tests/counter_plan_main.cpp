// ct_tile_of / ct_tiles / ct_chunks / ct_first_key / ct_tile_heads
// (csrc/counter_plan.hpp) from the command line, for tests/test_counter_plan.py.
// stdin, one request per line:
//   tile asked                 -> "tile"
//   series tile K  then K item counts
//       -> "n tiles chunks"  then per tile "first heads"  then the closing "first"
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "counter_plan.hpp"

int main() {
    std::string what;
    while (std::cin >> what) {
        if (what == "tile") {
            unsigned asked;
            std::cin >> asked;
            std::printf("%u\n", lcc::ct_tile_of(asked));
        } else if (what == "series") {
            unsigned tile;
            long long K;
            std::cin >> tile >> K;
            std::vector<uint64_t> off(K + 1, 0);
            for (long long k = 0; k < K; ++k) {
                unsigned long long n;
                std::cin >> n;
                off[k + 1] = off[k] + n;
            }
            const uint64_t n = off[K], T = lcc::ct_tiles(n, tile);
            const std::vector<uint32_t> first = lcc::ct_first_key(off.data(), K, n, tile);
            std::printf("%llu %llu %llu\n", (unsigned long long)n, (unsigned long long)T, (unsigned long long)lcc::ct_chunks(T));
            for (uint64_t t = 0; t < T; ++t)
                std::printf("%u %u\n", first[t], (unsigned)lcc::ct_tile_heads(off.data(), K, n, tile, first, t));
            std::printf("%u\n", first[T]);
        } else {
            return 1;
        }
        if (!std::cin) return 1;
    }
    return 0;
}
