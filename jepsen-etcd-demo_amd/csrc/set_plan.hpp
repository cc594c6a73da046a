// set_plan.hpp -- what a set-workload check (lc_set_pack, lc_set_check) does
// with each key and each step, as pure functions of the key's shape and the
// batch.  Host C++ only (no HIP): pinned on the CPU by tests/test_set_plan.py
// through tests/set_plan_main.cpp.
//
// Per key (plan_set_key): how elements become bitmap ids.
//   offset ids  id = element - min, span = max - min + 1 (unsigned 64-bit).
//               Taken when span <= SET_OFFSET_FLOOR_BITS, or when the key's three
//               bitmaps are no larger than its own input columns:
//                   24 * ceil(span / 64)  <=  5 * n_add + 4 * n_read      (bytes)
//               (three bitmaps of 8-byte words against a 4-byte id and a 1-byte
//               class per add row and a 4-byte id per read element).
//   rank ids    otherwise: the host sorts the key's distinct values, id = rank,
//               span = their count.  A key {-5, 10^12} costs two bits, not 10^12.
// Per step (plan_set_step): the tier of every key and the launch lists.
//   LDS tier    keys of span <= SET_LDS_MAX_BITS (and every key that is not
//               checked): one workgroup per key, the three bitmaps in LDS.
//               3 x 8 KiB = 24 KiB per workgroup, so six workgroups (24 of 32
//               waves) share a CU's 160 KiB.
//   HBM tier    wider keys: k_set_mark over chunks of SET_MARK_ROWS rows, then
//               k_set_classify over chunks of SET_BLOCK_WORDS bitmap words.
// Every key owns at least one "item"; an HBM key one per classify chunk.  The
// run counts of (key, class, chunk) are laid out in exactly that order --
// cnt[4 * item_base[k] + class * chunks(k) + chunk] -- so one linear exclusive
// scan gives every workgroup the place of its runs in the ascending output.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/lincheck.h"

namespace lcs {

constexpr uint32_t SET_BLOCK = 256;             // threads per workgroup, every set kernel
constexpr uint32_t SET_LANE_WORDS = 2;          // k_set_classify: one 16-byte load per bitmap and lane
constexpr uint32_t SET_WAVE_WORDS = 64 * SET_LANE_WORDS;
constexpr uint32_t SET_BLOCK_WORDS = SET_BLOCK * SET_LANE_WORDS;  // 512 words = 32,768 ids
constexpr uint32_t SET_LDS_MAX_BITS = 65536;    // LDS tier: 3 x 8 KiB
constexpr uint32_t SET_LDS_MAX_WORDS = SET_LDS_MAX_BITS / 64;
constexpr uint32_t SET_MARK_LANE_ROWS = 16;     // k_set_mark: consecutive rows per lane
constexpr uint32_t SET_MARK_ROWS = SET_BLOCK * SET_MARK_LANE_ROWS;
constexpr uint32_t SET_MARK_TILE_WORDS = SET_BLOCK;  // k_set_mark's LDS tile: 256 32-bit words per bitmap = 8,192 ids
constexpr uint64_t SET_OFFSET_FLOOR_BITS = 1024;
constexpr uint64_t SET_MAX_SPAN = 0xFFFFFFC0ull;  // ids are 32-bit
// Most device memory the HBM tier's three bitmaps may take.
constexpr uint64_t SET_BM_MAX_BYTES = 8ull << 30;

inline uint64_t set_words(uint64_t span) { return span / 64 + (span % 64 != 0); }
// a key's words in the shared bitmaps: rounded up to even (16-byte loads)
inline uint64_t set_words_padded(uint64_t span) { return (set_words(span) + 1) & ~1ull; }

struct SetKeyPlan {
    bool rank = false;
    uint64_t span = 0;  // offset ids: the span; rank ids: 0 (the distinct count, known after the sort)
};

// any: the key has at least one element (else min / max are ignored).
inline SetKeyPlan plan_set_key(bool any, int64_t mn, int64_t mx, uint64_t n_add, uint64_t n_read) {
    SetKeyPlan p;
    if (!any) return p;
    const uint64_t span = (uint64_t)mx - (uint64_t)mn + 1;  // <= 2^64 - 1: LC_NIL is no element
    const uint64_t input = 5 * n_add + 4 * n_read;
    if (span <= SET_OFFSET_FLOOR_BITS || set_words(span) <= input / 24) {
        p.span = span;
        return p;
    }
    p.rank = true;
    return p;
}

struct SetItem {       // one k_set_classify workgroup
    uint32_t key, chunk;
};
struct SetMarkItem {   // one k_set_mark workgroup: rows [row, min(row + SET_MARK_ROWS, end of the key))
    uint32_t key, is_read;
    uint64_t row;
};

struct SetStepIn {
    int64_t n_keys = 0;
    const uint32_t *span = nullptr;
    const uint8_t *status = nullptr;    // or null
    const uint64_t *add_off = nullptr, *read_off = nullptr;
    uint64_t n_words = 0;               // the batch's bitmap words
    bool force_hbm = false;             // LC_PATH_SET_HBM
    uint64_t bm_max_bytes = SET_BM_MAX_BYTES;
};

struct SetStepPlan {
    int rc = LC_OK;                      // LC_E_NOMEM: the bitmaps pass bm_max_bytes
    std::vector<uint32_t> small_keys;    // LDS tier, one workgroup each
    std::vector<SetItem> items;          // HBM tier classify workgroups
    std::vector<SetMarkItem> marks;      // HBM tier mark workgroups
    std::vector<uint32_t> item_base;     // [n_keys + 1]
    uint64_t n_items = 0;
    uint64_t bm_words = 0;               // words to allocate and zero: 3 * n_words, or 0 with no HBM key
};

inline bool set_key_hbm(uint32_t span, uint8_t status, bool force_hbm) {
    if (status != LC_SET_KEY_OK || span == 0) return false;
    return force_hbm || span > SET_LDS_MAX_BITS;
}
inline uint32_t set_key_chunks(uint32_t span, bool hbm) {
    return hbm ? (uint32_t)((set_words(span) + SET_BLOCK_WORDS - 1) / SET_BLOCK_WORDS) : 1u;
}

inline SetStepPlan plan_set_step(const SetStepIn &in) {
    SetStepPlan p;
    p.item_base.resize((size_t)in.n_keys + 1);
    bool any_hbm = false;
    for (int64_t k = 0; k < in.n_keys; ++k) {
        const uint8_t st = in.status ? in.status[k] : (uint8_t)LC_SET_KEY_OK;
        const bool hbm = set_key_hbm(in.span[k], st, in.force_hbm);
        p.item_base[(size_t)k] = (uint32_t)p.n_items;
        if (!hbm) {
            p.small_keys.push_back((uint32_t)k);
            p.n_items += 1;
            continue;
        }
        any_hbm = true;
        const uint32_t chunks = set_key_chunks(in.span[k], true);
        for (uint32_t j = 0; j < chunks; ++j) p.items.push_back({(uint32_t)k, j});
        p.n_items += chunks;
        for (uint64_t r = in.add_off[k]; r < in.add_off[k + 1]; r += SET_MARK_ROWS) p.marks.push_back({(uint32_t)k, 0u, r});
        for (uint64_t r = in.read_off[k]; r < in.read_off[k + 1]; r += SET_MARK_ROWS) p.marks.push_back({(uint32_t)k, 1u, r});
    }
    p.item_base[(size_t)in.n_keys] = (uint32_t)p.n_items;
    if (any_hbm) {
        p.bm_words = 3 * in.n_words;
        if (in.n_words > in.bm_max_bytes / 24) p.rc = LC_E_NOMEM;
    }
    return p;
}

}  // namespace lcs
