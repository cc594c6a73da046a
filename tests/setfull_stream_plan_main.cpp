// sfs_blocks / sfs_grow_blocks / plan_sfs_chunk (csrc/setfull_stream_plan.hpp)
// from the command line, for tests/test_setfull_stream_plan.py.  stdin, one
// request per line:
//   blocks ids                 -> "blocks"
//   grow have need             -> "capacity in blocks"
//   chunk T cap_bytes  then T x "n_ids rows els_per_row"  (first_el_gap 0; a
//       key's blocks are sfs_blocks(n_ids))
//       -> "passes segs marks folds max_words total_words"
//          then per pass "mark0 mark1 fold0 fold1 words"
//          then per segment "t n_rows bw row0 mbase"
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "setfull_stream_plan.hpp"

int main() {
    std::string what;
    while (std::cin >> what) {
        if (what == "blocks") {
            unsigned long long ids;
            std::cin >> ids;
            std::printf("%llu\n", (unsigned long long)lcfs::sfs_blocks(ids));
        } else if (what == "grow") {
            unsigned long long have, need;
            std::cin >> have >> need;
            std::printf("%llu\n", (unsigned long long)lcfs::sfs_grow_blocks(have, need));
        } else if (what == "chunk") {
            long long T;
            unsigned long long cap;
            std::cin >> T >> cap;
            std::vector<uint32_t> n_ids(T);
            std::vector<uint64_t> row_off(T + 1, 0), blk_off(T + 1, 0), el_off(1, 0);
            for (long long t = 0; t < T; ++t) {
                unsigned long long ids, rows, per;
                std::cin >> ids >> rows >> per;
                n_ids[t] = (uint32_t)ids;
                row_off[t + 1] = row_off[t] + rows;
                blk_off[t + 1] = blk_off[t] + lcfs::sfs_blocks(ids);
                for (unsigned long long r = 0; r < rows; ++r) el_off.push_back(el_off.back() + per);
            }
            lcfs::SfsChunkIn in;
            in.n_touched = T; in.n_ids = n_ids.data(); in.row_off = row_off.data(); in.blk_off = blk_off.data();
            in.el_off = el_off.data(); in.cap_bytes = cap;
            const lcfs::SfsChunkPlan p = lcfs::plan_sfs_chunk(in);
            std::printf("%zu %zu %zu %zu %llu %llu\n", p.passes.size(), p.segs.size(), p.marks.size(), p.folds.size(),
                        (unsigned long long)p.max_words, (unsigned long long)p.total_words);
            for (const lcfs::SfsPass &q : p.passes)
                std::printf("%llu %llu %llu %llu %llu\n", (unsigned long long)q.mark0, (unsigned long long)q.mark1,
                            (unsigned long long)q.fold0, (unsigned long long)q.fold1, (unsigned long long)q.words);
            for (const lcfs::SfsSeg &s : p.segs)
                std::printf("%u %u %u %llu %llu\n", s.t, s.n_rows, s.bw, (unsigned long long)s.row0, (unsigned long long)s.mbase);
        } else {
            return 1;
        }
        if (!std::cin) return 1;
    }
    return 0;
}
