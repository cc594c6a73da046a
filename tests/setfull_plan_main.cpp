// sf_band_ids / plan_setfull_step (csrc/setfull_plan.hpp) from the command
// line, for tests/test_setfull_plan.py.  stdin, one request per line:
//   band rows ids_left words_left pass_empty   -> "ids"
//   step K cap_bytes  then K x "span status rows els_per_row first_el_gap"
//       -> "passes segs marks scans n_items max_words total_words"
//          then per pass "mark0 mark1 scan0 scan1 words"
//          then per segment "key lo n_ids bw mbase"
//          then per key "item_base"
// A step's rows hold els_per_row elements each, laid out one after the other
// from first_el_gap of the first key on (so row starts need not be multiples
// of four); first_el_gap of later keys is ignored.
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "setfull_plan.hpp"

int main() {
    std::string what;
    while (std::cin >> what) {
        if (what == "band") {
            unsigned long long rows, ids, words;
            int empty;
            std::cin >> rows >> ids >> words >> empty;
            std::printf("%llu\n", (unsigned long long)lcf::sf_band_ids(rows, ids, words, empty != 0));
        } else if (what == "step") {
            long long K;
            unsigned long long cap;
            std::cin >> K >> cap;
            std::vector<uint32_t> span(K);
            std::vector<uint8_t> status(K);
            std::vector<uint64_t> row_off(K + 1, 0), el_off;
            uint64_t el = 0;
            for (long long k = 0; k < K; ++k) {
                unsigned long long s, st, rows, per, gap;
                std::cin >> s >> st >> rows >> per >> gap;
                span[k] = (uint32_t)s; status[k] = (uint8_t)st;
                row_off[k + 1] = row_off[k] + rows;
                if (k == 0) el = gap;
                for (unsigned long long r = 0; r < rows; ++r) {
                    el_off.push_back(el);
                    el += per;
                }
            }
            el_off.push_back(el);
            lcf::SfStepIn in;
            in.n_keys = K; in.span = span.data(); in.status = status.data(); in.row_off = row_off.data();
            in.el_off = el_off.data(); in.cap_bytes = cap;
            const lcf::SfStepPlan p = lcf::plan_setfull_step(in);
            std::printf("%zu %zu %zu %zu %llu %llu %llu\n", p.passes.size(), p.segs.size(), p.marks.size(), p.scans.size(),
                        (unsigned long long)p.n_items, (unsigned long long)p.max_words, (unsigned long long)p.total_words);
            for (const lcf::SfPass &q : p.passes)
                std::printf("%llu %llu %llu %llu %llu\n", (unsigned long long)q.mark0, (unsigned long long)q.mark1,
                            (unsigned long long)q.scan0, (unsigned long long)q.scan1, (unsigned long long)q.words);
            for (const lcf::SfSeg &s : p.segs)
                std::printf("%u %u %u %u %llu\n", s.key, s.lo, s.n_ids, s.bw, (unsigned long long)s.mbase);
            for (long long k = 0; k <= K; ++k) std::printf("%u\n", p.item_base[k]);
        } else {
            return 1;
        }
        if (!std::cin) return 1;
    }
    return 0;
}
