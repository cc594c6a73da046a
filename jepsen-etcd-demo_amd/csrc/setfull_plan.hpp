// setfull_plan.hpp -- what lc_setfull_check does with each key of a batch, as
// pure functions of the batch's shape.  Host C++ only (no HIP): pinned on the
// CPU by tests/test_setfull_plan.py through tests/setfull_plan_main.cpp.
//
// A key's presence matrix has one row per :ok read and one bit per id, rows
// of whole 64-bit words.  A step runs in PASSES: each pass zeroes one matrix
// buffer of at most `cap` bytes, marks it (k_setfull_mark) and scans it
// (k_setfull_scan).  The keys are laid into passes in batch order, each as one
// or more BANDS of consecutive ids (a "segment": key, first id, ids, words per
// row, place in the pass's buffer):
//   * a key whose rows x ceil(ids / 64) words fit what is left of the pass is
//     one band there (a batch of small keys is one pass);
//   * otherwise it takes the widest band that fits, a multiple of
//     SF_BLOCK_IDS ids (whole scan workgroups, so the per-workgroup counts of
//     different bands never share a slot), and goes on in the next pass;
//   * a band narrower than SF_BLOCK_IDS is never made: when not even that
//     fits an empty pass, the band is SF_BLOCK_IDS ids wide and that pass is
//     larger than the cap (rows x 32 bytes; a million reads are 32 MB).
// Every band of a key re-reads the key's read lists once and marks only its
// own ids, so the records are the same for any cap.
//
// The default cap is 128 MiB.  Every band re-reads the key's read lists, so
// fewer and wider bands are cheaper (measured, DESIGN.md 3.12: 2^20 ids x 256
// reads in 1, 4 and 32 bands mark in 0.13, 0.47 and 3.6 ms), and the cap
// should be as large as it can be while a pass's matrix, which mark writes
// with atomics and scan then reads once, still fits the 256 MiB Infinity
// Cache beside the read lists streaming past it: half of it.
//
// Mark workgroups: one per (band, row, SF_MARK_ELS read elements), starting
// at the row's first element rounded down to four (16-byte loads; the lanes
// mask what is not the row's).  Scan workgroups: one per (band, SF_BLOCK_IDS
// ids), one wave per 64 ids, one lane per id.  A key owns one count slot per
// SF_BLOCK_IDS ids of its span, item_base[k] + id / SF_BLOCK_IDS.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/lincheck.h"

namespace lcf {

constexpr uint32_t SF_BLOCK = 256;           // threads per workgroup, every set-full kernel
constexpr uint32_t SF_WAVE_IDS = 64;         // k_setfull_scan: one wave per matrix word
constexpr uint32_t SF_BLOCK_IDS = SF_BLOCK;  // one lane per id
constexpr uint32_t SF_BLOCK_WORDS = SF_BLOCK_IDS / 64;
constexpr uint32_t SF_MARK_LANE_ELS = 16;    // k_setfull_mark: consecutive read elements per lane (four 16-byte loads)
constexpr uint32_t SF_MARK_ELS = SF_BLOCK * SF_MARK_LANE_ELS;
constexpr uint32_t SF_MARK_TILE_WORDS = SF_BLOCK;  // mark's LDS tile: 256 32-bit words = 8,192 ids
constexpr uint64_t SF_MATRIX_MAX_BYTES = 128ull << 20;
constexpr uint64_t SF_MAX_SPAN = 0xFFFFFFC0ull;    // ids are 32-bit (as SET_MAX_SPAN)

inline uint64_t sf_words(uint64_t ids) { return ids / 64 + (ids % 64 != 0); }

// The ids of the next band of a key with `rows` rows and ids_left ids still
// to place, in a pass with words_left 64-bit words free.  0: start a new pass.
inline uint64_t sf_band_ids(uint64_t rows, uint64_t ids_left, uint64_t words_left, bool pass_empty) {
    if (ids_left == 0) return 0;
    if (rows == 0) return ids_left;  // no matrix at all
    const uint64_t max_bw = words_left / rows;
    if (sf_words(ids_left) <= max_bw) return ids_left;
    const uint64_t whole = max_bw / SF_BLOCK_WORDS * SF_BLOCK_IDS;
    if (whole) return whole;
    return pass_empty ? std::min<uint64_t>(ids_left, SF_BLOCK_IDS) : 0;
}

struct SfSeg {        // a band of one key in one pass
    uint32_t key, lo, n_ids, bw;  // first id, ids, 64-bit words per row
    uint64_t mbase;               // word offset of its rows in the pass's matrix
};
struct SfMarkItem {   // one k_setfull_mark workgroup
    uint32_t seg, pad;
    uint64_t row;     // the batch's row number
    uint64_t start;   // first element (a multiple of four) of its SF_MARK_ELS
};
struct SfScanItem {   // one k_setfull_scan workgroup: ids lo + chunk * SF_BLOCK_IDS ...
    uint32_t seg, chunk;
};
struct SfPass {
    uint64_t mark0 = 0, mark1 = 0, scan0 = 0, scan1 = 0, words = 0;
};

struct SfStepIn {
    int64_t n_keys = 0;
    const uint32_t *span = nullptr;
    const uint8_t *status = nullptr;  // or null
    const uint64_t *row_off = nullptr, *el_off = nullptr;
    uint64_t cap_bytes = SF_MATRIX_MAX_BYTES;
};

struct SfStepPlan {
    std::vector<SfSeg> segs;
    std::vector<SfMarkItem> marks;
    std::vector<SfScanItem> scans;
    std::vector<SfPass> passes;
    std::vector<uint32_t> item_base;  // [n_keys + 1] count slots
    uint64_t n_items = 0;
    uint64_t max_words = 0;           // the largest pass
    uint64_t total_words = 0;         // zeroed in all
};

inline SfStepPlan plan_setfull_step(const SfStepIn &in) {
    SfStepPlan p;
    const uint64_t cap_words = std::max<uint64_t>(1, (in.cap_bytes ? in.cap_bytes : SF_MATRIX_MAX_BYTES) / 8);
    p.item_base.resize((size_t)in.n_keys + 1);
    SfPass cur;
    auto close = [&]() {
        cur.mark1 = p.marks.size();
        cur.scan1 = p.scans.size();
        if (cur.mark1 > cur.mark0 || cur.scan1 > cur.scan0) {
            p.passes.push_back(cur);
            p.max_words = std::max(p.max_words, cur.words);
            p.total_words += cur.words;
        }
        cur = SfPass();
        cur.mark0 = p.marks.size();
        cur.scan0 = p.scans.size();
    };
    for (int64_t k = 0; k < in.n_keys; ++k) {
        p.item_base[(size_t)k] = (uint32_t)p.n_items;
        const uint8_t st = in.status ? in.status[k] : (uint8_t)LC_SET_KEY_OK;
        const uint64_t span = st == LC_SET_KEY_OK ? in.span[k] : 0;
        p.n_items += std::max<uint64_t>(1, (span + SF_BLOCK_IDS - 1) / SF_BLOCK_IDS);
        const uint64_t r0 = in.row_off[k], r1 = st == LC_SET_KEY_OK ? in.row_off[k + 1] : r0, rows = r1 - r0;
        for (uint64_t lo = 0; lo < span;) {
            const bool empty = cur.words == 0 && cur.scan0 == p.scans.size();
            const uint64_t left = cur.words < cap_words ? cap_words - cur.words : 0;
            const uint64_t n = sf_band_ids(rows, span - lo, left, empty);
            if (n == 0) {
                close();
                continue;
            }
            const uint32_t bw = rows ? (uint32_t)sf_words(n) : 0u;
            const uint32_t seg = (uint32_t)p.segs.size();
            p.segs.push_back({(uint32_t)k, (uint32_t)lo, (uint32_t)n, bw, cur.words});
            cur.words += rows * bw;
            for (uint64_t r = r0; r < r1; ++r) {
                if (in.el_off[r] == in.el_off[r + 1]) continue;  // an empty read: a row of zeros
                for (uint64_t s = in.el_off[r] & ~3ull; s < in.el_off[r + 1]; s += SF_MARK_ELS) p.marks.push_back({seg, 0u, r, s});
            }
            for (uint64_t c = 0; c * SF_BLOCK_IDS < n; ++c) p.scans.push_back({seg, (uint32_t)c});
            lo += n;
        }
    }
    close();
    p.item_base[(size_t)in.n_keys] = (uint32_t)p.n_items;
    return p;
}

}  // namespace lcf
