// counter_stream_plan.hpp -- the sizing rules of a streaming checker/counter
// (lc_counter_stream_*), as pure functions.  Host C++ only (no HIP): pinned on
// the CPU by tests/test_counter_stream_plan.py through
// tests/counter_stream_plan_main.cpp.
//
// Resident per read: CSP_READ_BYTES (key id, rank within the key, lower, value,
// upper, flag).  The reads array holds `cap` reads and grows by doubling.
//   csp_first_reads    lc_counter_stream_opts.reads to the first capacity: 0
//                      is CSP_DEFAULT_READS; anything from 1 to CSP_MAX_READS
//                      is taken as it is
//   csp_reads_cap      the capacity that holds `need` reads from one of
//                      `have`: doubled until it fits, cut at CSP_MAX_READS;
//                      CSP_BAD when need passes CSP_MAX_READS (LC_E_NOMEM)
//   csp_refuses        an append is judged BEFORE it is folded, by what it can
//                      add at most: `ok_reads` :ok :read rows and `client`
//                      :add / :read rows.  Reads or events that could reach
//                      2^32 over the stream refuse it (LC_E_UNSUPPORTED)
//   csp_launch_events  lc_counter_stream_opts.launch_events to the events of
//                      one launch: 0 is CSP_LAUNCH_EVENTS; else rounded up to
//                      a multiple of the tile, at most CSP_LAUNCH_EVENTS
//   csp_pieces         an append of more events is scanned in pieces of that
//                      many, each a scan of its own that starts from the sums
//                      the piece before left
//   csp_patch_threads  k_cs_patch's lanes: one per resident read from the
//                      oldest revised invocation's r0 on, and at least one per
//                      patch
#pragma once

#include <cstdint>

namespace lccs {

constexpr uint32_t CSP_BLOCK = 256;                  // threads per workgroup, every kernel
constexpr uint32_t CSP_READ_BYTES = 33;              // 4 + 4 + 8 + 8 + 8 + 1
constexpr uint64_t CSP_MAX_BYTES = 8ull << 30;       // the reads array's byte cap
constexpr uint64_t CSP_MAX_READS = CSP_MAX_BYTES / CSP_READ_BYTES;
constexpr uint64_t CSP_DEFAULT_READS = 1ull << 16;
constexpr uint64_t CSP_LAUNCH_EVENTS = 1ull << 24;   // events of one launch (and of its staging)
constexpr uint64_t CSP_LIMIT = 0xFFFFFFFFull;        // a stream's reads and events stay below 2^32
constexpr uint64_t CSP_BAD = 0;

inline uint64_t csp_first_reads(uint32_t asked) {
    if (asked == 0) return CSP_DEFAULT_READS;
    return asked <= CSP_MAX_READS ? asked : CSP_BAD;
}

inline uint64_t csp_reads_cap(uint64_t have, uint64_t need) {
    if (need > CSP_MAX_READS) return CSP_BAD;
    uint64_t c = have ? have : 1;
    while (c < need) c <<= 1;
    return c < CSP_MAX_READS ? c : CSP_MAX_READS;
}

// reads, events: the stream's so far.  0: taken; 1: the reads, 2: the events could reach 2^32.
inline int csp_refuses(uint64_t reads, uint64_t events, uint64_t ok_reads, uint64_t client) {
    if (reads + ok_reads > CSP_LIMIT) return 1;
    if (events + client > CSP_LIMIT) return 2;
    return 0;
}

inline uint64_t csp_launch_events(uint32_t asked, uint32_t tile) {
    if (asked == 0) return CSP_LAUNCH_EVENTS;
    const uint64_t up = ((uint64_t)asked + tile - 1) / tile * tile;
    return up < CSP_LAUNCH_EVENTS ? up : CSP_LAUNCH_EVENTS;
}

inline uint64_t csp_pieces(uint64_t events, uint64_t limit) { return events / limit + (events % limit != 0); }
inline uint64_t csp_piece_begin(uint64_t i, uint64_t events, uint64_t limit) {
    const uint64_t b = i * limit;
    return b < events ? b : events;
}

inline uint64_t csp_patch_threads(uint64_t reads, uint64_t min_r0, uint64_t patches) {
    const uint64_t span = reads > min_r0 ? reads - min_r0 : 0;
    return span > patches ? span : patches;
}

inline uint64_t csp_blocks(uint64_t n) { return n / CSP_BLOCK + (n % CSP_BLOCK != 0); }

}  // namespace lccs
