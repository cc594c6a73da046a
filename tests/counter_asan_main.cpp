// A stand-alone driver of checker/counter's packer and host fold for the
// sanitizer test (tests/test_counter_host.py): built with
// -fsanitize=address,undefined together with csrc/host_counter.cpp and nothing
// else.  No device function is reached; the few helpers of csrc/common.cpp that
// host_counter.cpp uses are given here, since common.cpp itself needs the HIP
// runtime.
//
// Feeds lc_counter_pack + lc_counter_check_host the hand example (and requires
// its triples), every malformed case beside a clean key, the overflow edge, an
// err_cap that is too small, caller-built batches that must be refused, and a
// 10,000-row random keyed history with every kind of row in it.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "common.hpp"
#include "../include/lincheck_counter.h"

namespace lc {
static std::string g_err;
void set_error(const std::string &m) { g_err = m; }
int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
void range_push(const char *) {}
void range_pop() {}
void *pinned_alloc(size_t bytes) { return std::malloc(bytes ? bytes : 1); }
void pinned_free(void *p) { std::free(p); }
}  // namespace lc

struct Rows {
    std::vector<uint8_t> type, f;
    std::vector<int64_t> process, key, value;
    void add(uint8_t t, uint8_t fn, int64_t p, int64_t v, int64_t k = LC_NO_KEY) {
        type.push_back(t); f.push_back(fn); process.push_back(p); key.push_back(k); value.push_back(v);
    }
    lc_counter_history view(bool keyed) const {
        lc_counter_history h{};
        h.n = (int64_t)type.size();
        h.type = type.data(); h.f = f.data(); h.process = process.data(); h.key = keyed ? key.data() : nullptr;
        h.value = value.data(); h.index = nullptr;
        return h;
    }
};

struct Out {
    std::vector<int8_t> valid;
    std::vector<uint64_t> n_errors, err_off, err_idx;
    std::vector<int64_t> lower, upper;
    lc_counter_result r{};
    Out(const lc_counter_batch &b, uint64_t cap) {
        const size_t K = (size_t)b.n_keys, R = K ? (size_t)b.read_off[K] : 0;
        valid.resize(K + 1); n_errors.resize(K + 1); err_off.resize(K + 1); err_idx.resize(cap + 1);
        lower.resize(R + 1); upper.resize(R + 1);
        r.valid = valid.data(); r.n_errors = n_errors.data(); r.lower = lower.data(); r.upper = upper.data();
        r.err_off = err_off.data(); r.err_idx = err_idx.data(); r.err_cap = cap; r.n_err = 0;
    }
};

#define REQUIRE(c)                                                          \
    do {                                                                    \
        if (!(c)) {                                                         \
            std::fprintf(stderr, "line %d: %s (%s)\n", __LINE__, #c, lc::g_err.c_str()); \
            return 1;                                                       \
        }                                                                   \
    } while (0)

static void hand(Rows &R, int64_t k) {
    const int64_t nil = LC_NIL;
    R.add(LC_INVOKE, LC_CF_ADD, 0, 1, k); R.add(LC_INVOKE, LC_CF_READ, 1, nil, k); R.add(LC_OK_T, LC_CF_ADD, 0, 1, k);
    R.add(LC_INVOKE, LC_CF_ADD, 2, 2, k); R.add(LC_OK_T, LC_CF_READ, 1, 1, k);
    R.add(LC_INVOKE, LC_CF_ADD, 0, 4, k); R.add(LC_FAIL, LC_CF_ADD, 0, 4, k); R.add(LC_INFO, LC_CF_ADD, 2, 2, k);
    R.add(LC_INVOKE, LC_CF_READ, 1, nil, k); R.add(LC_OK_T, LC_CF_READ, 1, 4, k);
    R.add(LC_INVOKE, LC_CF_READ, 3, nil, k); R.add(LC_INVOKE, LC_CF_ADD, 0, 3, k); R.add(LC_OK_T, LC_CF_ADD, 0, 3, k);
    R.add(LC_OK_T, LC_CF_READ, 3, 0, k);
    R.add(LC_INVOKE, LC_CF_READ, 1, nil, k); R.add(LC_FAIL, LC_CF_READ, 1, nil, k);
    R.add(LC_INVOKE, LC_CF_READ, 1, nil, k); R.add(LC_OK_T, LC_CF_READ, 1, 6, k);
}

// The hand example's results at key `k` of a checked batch.
static bool hand_ok(const lc_counter_batch &b, const Out &o, int64_t k) {
    const int64_t lo[4] = {0, 1, 1, 4}, up[4] = {3, 3, 6, 6};
    const uint64_t r0 = b.read_off[k];
    if (b.read_off[k + 1] - r0 != 4 || o.valid[(size_t)k] != LC_INVALID || o.n_errors[(size_t)k] != 2) return false;
    for (int i = 0; i < 4; ++i)
        if (o.lower[r0 + i] != lo[i] || o.upper[r0 + i] != up[i]) return false;
    const uint64_t e0 = o.err_off[(size_t)k];
    return o.err_off[(size_t)k + 1] == e0 + 2 && o.err_idx[e0] == r0 + 1 && o.err_idx[e0 + 1] == r0 + 2;
}

int main() {
    // the hand example, one key without tuples
    {
        Rows R;
        hand(R, LC_NO_KEY);
        lc_counter_history h = R.view(false);
        lc_counter_packed *p = nullptr;
        REQUIRE(lc_counter_pack(&h, &p) == LC_OK);
        lc_counter_batch b{};
        REQUIRE(lc_counter_packed_view(p, &b) == LC_OK && b.n_keys == 1 && b.ev_off[1] == 13);
        Out o(b, 4);
        REQUIRE(lc_counter_check_host(&b, &o.r) == LC_OK && o.r.n_err == 2 && hand_ok(b, o, 0));
        Out small(b, 1);
        REQUIRE(lc_counter_check_host(&b, &small.r) == LC_E_NOMEM && small.r.n_err == 2);
        int64_t key = 0;
        REQUIRE(lc_counter_packed_keys(p, &key) == LC_OK && key == LC_NO_KEY && !lc_counter_packed_key_error(p, 0));
        lc_counter_packed_free(p);
    }
    // every malformed case as key 1 between two hand examples
    for (int bad = 0; bad < 8; ++bad) {
        Rows R;
        hand(R, 0);
        const int64_t nil = LC_NIL;
        switch (bad) {
            case 0: R.add(LC_OK_T, LC_CF_ADD, 5, 1, 1); break;                                      // no open invocation
            case 1: R.add(LC_INVOKE, LC_CF_READ, 5, nil, 1); R.add(LC_INVOKE, LC_CF_ADD, 5, 1, 1); break;  // a second one
            case 2: R.add(LC_INVOKE, LC_CF_ADD, 5, nil, 1); break;                                  // an add of nil
            case 3: R.add(LC_INVOKE, LC_CF_ADD, 5, 1, 1); R.add(LC_OK_T, LC_CF_ADD, 5, -7, 1); break;      // a negative add
            case 4: R.add(LC_INVOKE, LC_CF_READ, 5, nil, 1); R.add(LC_OK_T, LC_CF_READ, 5, nil, 1); break; // a read of nil
            case 5: R.add(LC_INVOKE, LC_CF_ADD, 5, INT64_MAX, 1); R.add(LC_INVOKE, LC_CF_ADD, 6, 1, 1); break;  // past INT64_MAX
            case 6: R.add(LC_INVOKE, LC_CF_ADD, 5, 1, 1); R.add(LC_OK_T, LC_CF_READ, 5, 1, 1); break;      // another :f
            default: R.add(LC_FAIL, LC_CF_READ, 5, nil, 1); break;                                  // a :fail nobody invoked
        }
        R.add(LC_INFO, LC_CF_OTHER, LC_NO_PROCESS, nil, LC_NO_KEY);  // a nemesis row
        hand(R, 2);
        lc_counter_history h = R.view(true);
        lc_counter_packed *p = nullptr;
        REQUIRE(lc_counter_pack(&h, &p) == LC_OK);
        lc_counter_batch b{};
        REQUIRE(lc_counter_packed_view(p, &b) == LC_OK && b.n_keys == 3);
        REQUIRE(b.status[1] == LC_COUNTER_KEY_ERROR && lc_counter_packed_key_error(p, 1) && b.ev_off[1] == b.ev_off[2]);
        Out o(b, 8);
        REQUIRE(lc_counter_check_host(&b, &o.r) == LC_OK && o.r.n_err == 4);
        REQUIRE(hand_ok(b, o, 0) && hand_ok(b, o, 2) && o.valid[1] == LC_UNKNOWN && o.n_errors[1] == 0);
        lc_counter_packed_free(p);
    }
    // exactly INT64_MAX passes
    {
        Rows R;
        R.add(LC_INVOKE, LC_CF_ADD, 0, INT64_MAX - 5, LC_NO_KEY); R.add(LC_OK_T, LC_CF_ADD, 0, INT64_MAX - 5, LC_NO_KEY);
        R.add(LC_INVOKE, LC_CF_ADD, 0, 5, LC_NO_KEY);
        R.add(LC_INVOKE, LC_CF_READ, 1, LC_NIL, LC_NO_KEY); R.add(LC_OK_T, LC_CF_READ, 1, INT64_MAX, LC_NO_KEY);
        lc_counter_history h = R.view(false);
        lc_counter_packed *p = nullptr;
        REQUIRE(lc_counter_pack(&h, &p) == LC_OK);
        lc_counter_batch b{};
        REQUIRE(lc_counter_packed_view(p, &b) == LC_OK && b.status[0] == LC_COUNTER_KEY_OK);
        Out o(b, 1);
        REQUIRE(lc_counter_check_host(&b, &o.r) == LC_OK && o.valid[0] == LC_VALID && o.upper[0] == INT64_MAX &&
                o.lower[0] == INT64_MAX - 5);
        // caller-built batches that must be refused
        std::vector<int64_t> val(b.ev_val, b.ev_val + b.ev_off[1]);
        std::vector<uint8_t> kind(b.ev_kind, b.ev_kind + b.ev_off[1]);
        lc_counter_batch c = b;
        c.ev_val = val.data(); c.ev_kind = kind.data();
        val[3] = 1;  // a read that is not the batch's
        REQUIRE(lc_counter_check_host(&c, &o.r) == LC_E_INVALID);
        val[3] = 0; kind[0] = 200;
        REQUIRE(lc_counter_check_host(&c, &o.r) == LC_E_INVALID);
        kind[0] = LC_CE_UP;
        REQUIRE(lc_counter_check_host(&c, &o.r) == LC_OK);
        lc_counter_packed_free(p);
    }
    // bad codes, nulls, the empty history
    {
        Rows R;
        hand(R, LC_NO_KEY);
        R.type[2] = 7;
        lc_counter_history h = R.view(false);
        lc_counter_packed *p = nullptr;
        REQUIRE(lc_counter_pack(&h, &p) == LC_E_INVALID && !p);
        REQUIRE(lc_counter_pack(nullptr, &p) == LC_E_INVALID);
        lc_counter_history e{};
        REQUIRE(lc_counter_pack(&e, &p) == LC_OK);
        lc_counter_batch b{};
        REQUIRE(lc_counter_packed_view(p, &b) == LC_OK && b.n_keys == 1 && b.ev_off[1] == 0 && b.read_off[1] == 0);
        Out o(b, 0);
        REQUIRE(lc_counter_check_host(&b, &o.r) == LC_OK && o.valid[0] == LC_VALID && o.r.n_err == 0);
        lc_counter_packed_free(p);
        int64_t info[4];
        REQUIRE(lc_counter_launch_info(info) == LC_OK && info[0] == 256);
    }
    // 10,000 random rows over 7 interleaved keys
    {
        Rows R;
        uint64_t x = 88172645463325252ull;
        auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
        for (int i = 0; i < 10000; ++i) {
            const int64_t k = (int64_t)(rnd() % 7), p = (int64_t)(rnd() % 5);
            const uint64_t what = rnd() % 100;
            if (what < 3) { R.add(LC_INFO, LC_CF_OTHER, LC_NO_PROCESS, LC_NIL, LC_NO_KEY); continue; }
            const uint8_t t = (uint8_t)(rnd() % 4), f = (uint8_t)(rnd() % 2);
            int64_t v = (int64_t)(rnd() % 50);
            if (what == 3) v = LC_NIL;
            if (what == 4) v = -v;
            // keys 0..3 mostly alternate per process by construction of the walk below; the others are free-form
            R.add(k < 4 ? (uint8_t)(i % 2 ? LC_OK_T : LC_INVOKE) : t, f, k < 4 ? (int64_t)(i / 2 % 3) : p, v, k);
        }
        lc_counter_history h = R.view(true);
        lc_counter_packed *p = nullptr;
        REQUIRE(lc_counter_pack(&h, &p) == LC_OK);
        lc_counter_batch b{};
        REQUIRE(lc_counter_packed_view(p, &b) == LC_OK && b.n_keys == 7);
        Out o(b, b.read_off[7]);
        REQUIRE(lc_counter_check_host(&b, &o.r) == LC_OK);
        for (int64_t k = 0; k < 7; ++k) {
            REQUIRE((b.status[k] == LC_COUNTER_KEY_ERROR) == (o.valid[(size_t)k] == LC_UNKNOWN));
            REQUIRE((b.status[k] == LC_COUNTER_KEY_ERROR) == (lc_counter_packed_key_error(p, k) != nullptr));
        }
        lc_counter_packed_free(p);
    }
    // a well-formed long key: 10,000 rows of overlapping adds and reads
    {
        Rows R;
        uint64_t x = 1234567ull;
        auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
        int open[4] = {0, 0, 0, 0};  // 0 free, 1 add, 2 read
        int64_t val[4] = {0, 0, 0, 0}, lower = 0;
        for (int i = 0; i < 10000; ++i) {
            const int p = (int)(rnd() % 4);
            if (!open[p]) {
                open[p] = 1 + (int)(rnd() % 2);
                val[p] = (int64_t)(rnd() % 9);
                R.add(LC_INVOKE, open[p] == 1 ? LC_CF_ADD : LC_CF_READ, p, open[p] == 1 ? val[p] : LC_NIL);
            } else {
                const uint8_t t = (uint8_t)(1 + rnd() % 3);
                if (open[p] == 1) {
                    if (t == LC_OK_T) lower += val[p];
                    R.add(t, LC_CF_ADD, p, val[p]);
                } else {
                    R.add(t, LC_CF_READ, p, t == LC_OK_T ? lower : LC_NIL);
                }
                open[p] = 0;
            }
        }
        lc_counter_history h = R.view(false);
        lc_counter_packed *p = nullptr;
        REQUIRE(lc_counter_pack(&h, &p) == LC_OK);
        lc_counter_batch b{};
        REQUIRE(lc_counter_packed_view(p, &b) == LC_OK && b.n_keys == 1 && b.status[0] == LC_COUNTER_KEY_OK);
        REQUIRE(b.read_off[1] > 500);
        Out o(b, b.read_off[1]);
        REQUIRE(lc_counter_check_host(&b, &o.r) == LC_OK && o.valid[0] == LC_VALID && o.r.n_err == 0);
        lc_counter_packed_free(p);
    }
    std::printf("ok\n");
    return 0;
}
