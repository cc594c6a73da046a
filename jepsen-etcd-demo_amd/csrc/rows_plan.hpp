// rows_plan.hpp -- the sizing rules of the device's row front end
// (device_rows.hip): grouping raw history rows by independent key and pairing
// them by (key, process) on the device.  Host C++ only (no HIP): pinned on the
// CPU by tests/test_counter_pack_plan.py through tests/counter_pack_plan_main.cpp.
//
//   rp_slots      slots of a hash table (keys, or processes) for n rows: the
//                 next power of two at or above 2 x n (a load factor of at most
//                 1/2: a batch has at most one distinct key per row, so a probe
//                 always ends at an empty slot), and at least one workgroup's
//                 worth.  A probe loop runs at most rp_slots steps.
//   rp_hash       a key's (a process's) first slot, before the mask: the
//                 64-bit finaliser of MurmurHash3, so that keys that differ in
//                 few bits (0, 1, 2, ...; multiples of a power of two) spread
//   rp_bits       the bits a stable LSD radix sort needs for values 0 .. max
//   rp_tiles      tiles of RP_TILE consecutive items of a scan, one workgroup each
// Rows and positions are 32-bit on the device: a batch has at most RP_MAX_ROWS
// rows, and byte offsets (n x something) are 64-bit everywhere.
#pragma once

#include <cstdint>

namespace lcr {

constexpr uint32_t RP_BLOCK = 256;              // threads per workgroup, every kernel of the front end
constexpr uint32_t RP_IPT = 8;                  // a scan's items per thread
constexpr uint32_t RP_TILE = RP_BLOCK * RP_IPT; // a scan's tile
constexpr uint64_t RP_MAX_ROWS = 0x7FFFFFF0ull; // 2^31 - 16
constexpr uint32_t RP_SLOT_BYTES = 16;          // {key, first row}
constexpr uint32_t RP_SLOTS_PER_ROW = 2;
constexpr uint32_t RP_NONE = 0xFFFFFFFFu;       // no row / no position
constexpr uint32_t RP_SORT_BITS_MAX = 32;       // each sort's keys are 32-bit

inline uint64_t rp_pow2_at_least(uint64_t x) {
    uint64_t p = 1;
    while (p < x) p <<= 1;  // (callers keep x at or below 2^63)
    return p;
}

inline uint64_t rp_slots(uint64_t n_rows) {
    if (n_rows > RP_MAX_ROWS) return 0;
    const uint64_t s = rp_pow2_at_least(RP_SLOTS_PER_ROW * n_rows);
    return s < RP_BLOCK ? RP_BLOCK : s;
}

constexpr uint64_t rp_hash(uint64_t k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return k;
}

// Bits of a sort over values 0 .. max, at least 1 (a sort of no bits is a copy; one bit costs a pass and keeps one code path).
inline uint32_t rp_bits(uint64_t max) {
    uint32_t b = 1;
    while (b < 64 && (max >> b) != 0) ++b;
    return b;
}

inline uint64_t rp_blocks(uint64_t n) { return n / RP_BLOCK + (n % RP_BLOCK != 0); }
inline uint64_t rp_tiles(uint64_t n) { return n / RP_TILE + (n % RP_TILE != 0); }

}  // namespace lcr
