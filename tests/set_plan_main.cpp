// plan_set_key / plan_set_step (csrc/set_plan.hpp) from the command line, for
// tests/test_set_plan.py.  stdin, one request per line:
//   key any min max n_add n_read          -> "rank span"
//   step K force_hbm bm_max_bytes  then K x "span status n_add n_read"
//                                         -> "rc n_small n_items n_marks bm_words n_words"
//                                            then per key "base item_base chunks hbm"
// A step's bases are laid out as lc_set_pack does: each checked key's words
// rounded up to even, one key after the other.
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "set_plan.hpp"

int main() {
    std::string what;
    while (std::cin >> what) {
        if (what == "key") {
            int any;
            long long mn, mx;
            unsigned long long n_add, n_read;
            std::cin >> any >> mn >> mx >> n_add >> n_read;
            const lcs::SetKeyPlan p = lcs::plan_set_key(any != 0, mn, mx, n_add, n_read);
            std::printf("%d %llu\n", (int)p.rank, (unsigned long long)p.span);
        } else if (what == "step") {
            long long K;
            int force;
            unsigned long long cap;
            std::cin >> K >> force >> cap;
            std::vector<uint32_t> span(K);
            std::vector<uint8_t> status(K);
            std::vector<uint64_t> add_off(K + 1, 0), read_off(K + 1, 0), base(K);
            uint64_t words = 0;
            for (long long k = 0; k < K; ++k) {
                unsigned long long s, st, a, r;
                std::cin >> s >> st >> a >> r;
                span[k] = (uint32_t)s; status[k] = (uint8_t)st;
                add_off[k + 1] = add_off[k] + a; read_off[k + 1] = read_off[k] + r;
                base[k] = words;
                if (st == LC_SET_KEY_OK) words += lcs::set_words_padded(s);
            }
            lcs::SetStepIn in;
            in.n_keys = K; in.span = span.data(); in.status = status.data(); in.add_off = add_off.data();
            in.read_off = read_off.data(); in.n_words = words; in.force_hbm = force != 0; in.bm_max_bytes = cap;
            const lcs::SetStepPlan p = lcs::plan_set_step(in);
            std::printf("%d %zu %llu %zu %llu %llu\n", p.rc, p.small_keys.size(), (unsigned long long)p.n_items, p.marks.size(),
                        (unsigned long long)p.bm_words, (unsigned long long)words);
            for (long long k = 0; k < K; ++k) {
                const bool hbm = lcs::set_key_hbm(span[k], status[k], in.force_hbm);
                std::printf("%llu %u %u %d\n", (unsigned long long)base[k], p.item_base[k], lcs::set_key_chunks(span[k], hbm), (int)hbm);
            }
        } else {
            return 1;
        }
        if (!std::cin) return 1;
    }
    return 0;
}
