// setfull_stream_plan.hpp -- the capacity and pass rules of a streaming
// set-full (lc_setfull_stream_*), as pure functions.  Host
// C++ only (no HIP): pinned on the CPU by tests/test_setfull_stream_plan.py
// through tests/setfull_stream_plan_main.cpp.
//
// CAPACITY.  The records live in BLOCKS of SFS_BLOCK_IDS ids, one fold
// workgroup each.  A key owns whole blocks: its id capacity grows by one
// block at a time (sfs_blocks), and a block belongs to one key for the
// stream's life, so no record ever moves between blocks.  The device arrays
// hold a number of blocks that grows by doubling from SFS_MIN_BLOCKS
// (sfs_grow_blocks), the old contents copied device to device.
//
// PASSES.  An append's chunk has, per touched key, its new :ok reads (rows)
// and a presence matrix rows x (4 words per block of the key).  The chunk is
// folded in passes of WHOLE ROWS: the touched keys are laid into passes in
// order, each taking as many of its remaining rows as fit what is left of the
// pass's matrix (cap_bytes); a key whose single row is wider than an empty
// pass takes that one row above the cap.  A key without new rows is one
// segment of no rows in the pass that is open when its turn comes (its
// records are re-classified: adds alone change the counts).  Every update of
// the fold is a max or a first by position, so row passes compose and the
// records are the same for any cap.
// Per segment: one mark workgroup per (non-empty row, SFS_MARK_ELS read
// elements from the row's start rounded down to four), one fold workgroup
// per block of the key.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace lcfs {

constexpr uint32_t SFS_BLOCK = 256;              // threads per workgroup, every kernel
constexpr uint32_t SFS_BLOCK_IDS = SFS_BLOCK;    // k_sfs_fold: one lane per id, one wave per 64 ids
constexpr uint32_t SFS_BLOCK_WORDS = SFS_BLOCK_IDS / 64;
constexpr uint32_t SFS_MARK_LANE_ELS = 4;        // k_sfs_mark: one 16-byte load per lane
constexpr uint32_t SFS_MARK_ELS = SFS_BLOCK * SFS_MARK_LANE_ELS;
constexpr uint64_t SFS_MIN_BLOCKS = 64;          // the device arrays' first capacity (16,384 ids)
constexpr uint64_t SFS_MAX_BLOCKS = 1ull << 24;  // 2^32 ids in all: slots are 32-bit
constexpr uint64_t SFS_MATRIX_MAX_BYTES = 128ull << 20;  // as the one-shot check's cap (setfull_plan.hpp)

// Blocks a key of `ids` ids owns.
inline uint64_t sfs_blocks(uint64_t ids) { return ids / SFS_BLOCK_IDS + (ids % SFS_BLOCK_IDS != 0); }

// The device arrays' capacity in blocks once `need` blocks are in use.
inline uint64_t sfs_grow_blocks(uint64_t have, uint64_t need) {
    uint64_t cap = std::max(have, SFS_MIN_BLOCKS);
    while (cap < need) cap *= 2;
    return cap;
}

struct SfsSeg {       // rows [row0, row0 + n_rows) of the chunk (one touched key's) in one pass
    uint32_t t;       // the touched key
    uint32_t n_rows;
    uint32_t bw;      // 64-bit words per matrix row: SFS_BLOCK_WORDS x the key's blocks
    uint32_t n_ids;
    uint64_t row0;    // the chunk's row number of its first row
    uint64_t mbase;   // word offset of its rows in the pass's matrix
    uint64_t blk_off; // the key's blocks in the chunk's block list
};
struct SfsMarkItem {  // one k_sfs_mark workgroup
    uint32_t seg, pad;
    uint64_t row;     // the chunk's row number
    uint64_t start;   // first element (a multiple of four) of its SFS_MARK_ELS
};
struct SfsFoldItem {  // one k_sfs_fold workgroup: block j of the segment's key
    uint32_t seg, j;
};
struct SfsPass {
    uint64_t mark0 = 0, mark1 = 0, fold0 = 0, fold1 = 0, words = 0;
};

struct SfsChunkIn {
    int64_t n_touched = 0;
    const uint32_t *n_ids = nullptr;    // [n_touched]
    const uint64_t *row_off = nullptr;  // [n_touched + 1]
    const uint64_t *blk_off = nullptr;  // [n_touched + 1]
    const uint64_t *el_off = nullptr;   // [rows + 1]
    uint64_t cap_bytes = SFS_MATRIX_MAX_BYTES;
};

struct SfsChunkPlan {
    std::vector<SfsSeg> segs;
    std::vector<SfsMarkItem> marks;
    std::vector<SfsFoldItem> folds;
    std::vector<SfsPass> passes;
    uint64_t max_words = 0;    // the largest pass
    uint64_t total_words = 0;  // zeroed in all
};

inline SfsChunkPlan plan_sfs_chunk(const SfsChunkIn &in) {
    SfsChunkPlan p;
    const uint64_t cap_words = std::max<uint64_t>(1, (in.cap_bytes ? in.cap_bytes : SFS_MATRIX_MAX_BYTES) / 8);
    SfsPass cur;
    auto close = [&]() {
        cur.mark1 = p.marks.size();
        cur.fold1 = p.folds.size();
        if (cur.fold1 > cur.fold0) {
            p.passes.push_back(cur);
            p.max_words = std::max(p.max_words, cur.words);
            p.total_words += cur.words;
        }
        cur = SfsPass();
        cur.mark0 = p.marks.size();
        cur.fold0 = p.folds.size();
    };
    for (int64_t t = 0; t < in.n_touched; ++t) {
        const uint64_t blocks = in.blk_off[t + 1] - in.blk_off[t];
        const uint64_t r0 = in.row_off[t], r1 = in.row_off[t + 1];
        const uint64_t bw = blocks * SFS_BLOCK_WORDS;
        uint64_t r = r0;
        do {
            uint64_t n = 0;
            if (r < r1 && bw) {
                const uint64_t left = cur.words < cap_words ? cap_words - cur.words : 0;
                n = std::min(r1 - r, left / bw);
                if (n == 0) {
                    if (cur.fold0 != p.folds.size()) {  // the pass is in use: a new one
                        close();
                        continue;
                    }
                    n = 1;  // one row is wider than an empty pass
                }
            } else {
                n = r1 - r;  // no rows, or a key without ids: no matrix
            }
            const uint32_t seg = (uint32_t)p.segs.size();
            p.segs.push_back({(uint32_t)t, (uint32_t)n, (uint32_t)bw, in.n_ids[t], r, cur.words, in.blk_off[t]});
            cur.words += n * bw;
            if (bw)
                for (uint64_t q = r; q < r + n; ++q) {
                    if (in.el_off[q] == in.el_off[q + 1]) continue;  // an empty read: a row of zeros
                    for (uint64_t s = in.el_off[q] & ~3ull; s < in.el_off[q + 1]; s += SFS_MARK_ELS) p.marks.push_back({seg, 0u, q, s});
                }
            for (uint64_t j = 0; j < blocks; ++j) p.folds.push_back({seg, (uint32_t)j});
            r += n;
        } while (r < r1);
    }
    close();
    return p;
}

}  // namespace lcfs
