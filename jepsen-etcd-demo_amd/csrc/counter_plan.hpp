// counter_plan.hpp -- the tile arithmetic and launch shapes of lc_counter_check,
// as pure functions of a batch's offsets.  Host C++ only (no HIP): pinned on the
// CPU by tests/test_counter_plan.py through tests/counter_plan_main.cpp.
//
// A SERIES is either the batch's events (ev_off) or its reads (read_off): n
// items, key k's at off[k] .. off[k + 1].  It is cut into TILES of `tile`
// consecutive items, one workgroup of CT_BLOCK threads each, every thread
// holding tile / CT_BLOCK consecutive items.  A key HEAD is the first item of a
// key that has items; a running sum starts over at a head.
//   ct_first_key   per tile the first entry j of off[0 .. K] with off[j] at or
//                  past the tile's first item, and K + 1 after the last tile:
//                  the entries first_key[t] .. first_key[t + 1] are those that
//                  fall into tile t (the last tile also takes the entries that
//                  equal n).  A workgroup marks its heads from them: entry j is
//                  a head when j < K and off[j] < n (an empty key's entry
//                  marks the next key's head once more, which changes nothing).
//   ct_tile_heads  what k_counter_tile records of a tile's heads: bit 0 some
//                  head, bit 1 a head at the tile's first item.
// k_counter_carry walks the tile records in CHUNKS of CT_CARRY_CHUNK tiles, one
// per thread, with a running carry from chunk to chunk.
#pragma once

#include <cstdint>
#include <vector>

namespace lcc {

constexpr uint32_t CT_BLOCK = 256;          // threads per workgroup, every counter kernel
constexpr uint32_t CT_TILE_MIN = 256;       // one item per thread (tests)
constexpr uint32_t CT_TILE_DEFAULT = 2048;  // eight per thread: kinds as one 8-byte load, values as four 16-byte loads
constexpr uint32_t CT_CARRY_CHUNK = CT_BLOCK;
constexpr uint64_t CT_MAX_TILES = 0x7FFFFFF0ull;  // one launch's workgroups

constexpr uint8_t CT_HEAD_ANY = 1, CT_HEAD_FIRST = 2;

// lc_counter_opts.tile to the tile used; 0 when it is not one the kernels are built for.
inline uint32_t ct_tile_of(uint32_t asked) {
    if (asked == 0) return CT_TILE_DEFAULT;
    return asked == CT_TILE_MIN || asked == CT_TILE_DEFAULT ? asked : 0;
}

inline uint64_t ct_tiles(uint64_t n, uint32_t tile) { return n / tile + (n % tile != 0); }
inline uint64_t ct_chunks(uint64_t n_tiles) { return n_tiles / CT_CARRY_CHUNK + (n_tiles % CT_CARRY_CHUNK != 0); }

// off: [K + 1], ascending from 0 to n.  Returns [ct_tiles(n, tile) + 1].
inline std::vector<uint32_t> ct_first_key(const uint64_t *off, int64_t K, uint64_t n, uint32_t tile) {
    const uint64_t T = ct_tiles(n, tile);
    std::vector<uint32_t> first((size_t)T + 1);
    uint64_t j = 0;
    for (uint64_t t = 0; t < T; ++t) {
        while (j <= (uint64_t)K && off[j] < t * tile) ++j;
        first[(size_t)t] = (uint32_t)j;
    }
    first[(size_t)T] = (uint32_t)K + 1;
    return first;
}

// Tile t's head byte, from ct_first_key's output.
inline uint8_t ct_tile_heads(const uint64_t *off, int64_t K, uint64_t n, uint32_t tile, const std::vector<uint32_t> &first,
                             uint64_t t) {
    uint8_t h = 0;
    for (uint64_t j = first[(size_t)t]; j < first[(size_t)t + 1]; ++j) {
        if (j >= (uint64_t)K || off[j] >= n) continue;
        h |= CT_HEAD_ANY;
        if (off[j] == t * tile) h |= CT_HEAD_FIRST;
    }
    return h;
}

}  // namespace lcc
