// A stand-alone driver of the streaming counter's packer and host fold for the
// sanitizer test (tests/test_counter_stream_host.py): built with
// -fsanitize=address,undefined together with csrc/host_counter_stream.cpp and
// csrc/host_counter.cpp and nothing else.  The streams are host streams (no
// context), so no device function is reached -- the device half's functions
// are weak and absent here; the few helpers of csrc/common.cpp that those
// files use are given here, since common.cpp itself needs the HIP runtime.
//
// Appends 20,000 random rows (three keys or none; adds and reads on
// overlapping processes completing :ok, :fail or :info; now and then a nil or
// negative add that is failed later, a huge add, an orphan completion, a nil
// read; nemesis rows) cut at random points, with empty appends, and after
// EVERY append requires the stream's keys, counts, bounds and error indices to
// equal lc_counter_pack + lc_counter_check_host of the prefix; then the
// refusals (bad codes, the other keyedness, bad options) that must leave a
// stream as it was, and an err_idx capacity that is too small.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "common.hpp"
#include "../include/lincheck_counter_stream.h"

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
void *big_alloc(size_t bytes) { return std::malloc(bytes ? bytes : 1); }
void big_free(void *p, size_t) { std::free(p); }
}  // namespace lc

#define REQUIRE(c)                                                                              \
    do {                                                                                        \
        if (!(c)) {                                                                             \
            std::fprintf(stderr, "line %d: %s (%s)\n", __LINE__, #c, lc::g_err.c_str());        \
            return 1;                                                                           \
        }                                                                                       \
    } while (0)

struct Rows {
    std::vector<uint8_t> type, f;
    std::vector<int64_t> process, key, value;
    void add(uint8_t t, uint8_t fn, int64_t p, int64_t v, int64_t k = LC_NO_KEY) {
        type.push_back(t); f.push_back(fn); process.push_back(p); key.push_back(k); value.push_back(v);
    }
    size_t n() const { return type.size(); }
    lc_counter_history view(bool keyed, size_t lo, size_t hi) const {
        lc_counter_history h{};
        h.n = (int64_t)(hi - lo);
        h.type = type.data() + lo; h.f = f.data() + lo; h.process = process.data() + lo; h.key = keyed ? key.data() + lo : nullptr;
        h.value = value.data() + lo; h.index = nullptr;
        return h;
    }
};

struct Out {
    std::vector<int8_t> valid;
    std::vector<uint64_t> n_errors, err_off, err_idx;
    std::vector<int64_t> lower, upper;
    lc_counter_result r{};
    Out(size_t K, size_t R, uint64_t cap) {
        valid.assign(K + 1, 9); n_errors.assign(K + 1, 99); err_off.assign(K + 2, 99); err_idx.assign(cap + 1, 99);
        lower.assign(R + 1, -7); upper.assign(R + 1, -7);
        r.valid = valid.data(); r.n_errors = n_errors.data(); r.lower = lower.data(); r.upper = upper.data();
        r.err_off = err_off.data(); r.err_idx = err_idx.data(); r.err_cap = cap; r.n_err = 0;
    }
};

static uint64_t g_rng = 88172645463325252ull;
static uint64_t rnd() {
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return g_rng;
}
static bool chance(unsigned per_mille) { return rnd() % 1000 < per_mille; }

// The stream against the one-shot check of rows [0, upto).
static int same(lc_counter_stream *s, const Rows &R, bool keyed, size_t upto) {
    lc_counter_history h = R.view(keyed, 0, upto);
    lc_counter_packed *p = nullptr;
    REQUIRE(lc_counter_pack(&h, &p) == LC_OK);
    lc_counter_batch b{};
    REQUIRE(lc_counter_packed_view(p, &b) == LC_OK);
    const size_t K = (size_t)b.n_keys, NR = (size_t)b.read_off[K];
    REQUIRE(lc_counter_stream_keys(s, nullptr) == (int64_t)K);
    std::vector<int64_t> k1(K + 1), k2(K + 1);
    REQUIRE(lc_counter_stream_keys(s, k1.data()) == (int64_t)K && lc_counter_packed_keys(p, k2.data()) == LC_OK);
    REQUIRE(std::memcmp(k1.data(), k2.data(), K * 8) == 0);
    Out want(K, NR, NR), got(K, NR, NR);
    REQUIRE(lc_counter_check_host(&b, &want.r) == LC_OK);
    std::vector<int8_t> valid(K + 1);
    std::vector<uint64_t> n_errors(K + 1), n_reads(K + 1);
    std::vector<int64_t> value(NR + 1);
    REQUIRE(lc_counter_stream_counts(s, valid.data(), n_errors.data(), n_reads.data()) == LC_OK);
    REQUIRE(lc_counter_stream_results(s, &got.r, value.data()) == LC_OK && got.r.n_err == want.r.n_err);
    for (size_t k = 0; k < K; ++k) {
        REQUIRE(valid[k] == want.valid[k] && got.valid[k] == want.valid[k]);
        REQUIRE(n_errors[k] == want.n_errors[k] && got.n_errors[k] == want.n_errors[k]);
        REQUIRE(n_reads[k] == b.read_off[k + 1] - b.read_off[k]);
        REQUIRE(got.err_off[k] == want.err_off[k]);
        REQUIRE((lc_counter_stream_key_error(s, (int64_t)k) != nullptr) == (lc_counter_packed_key_error(p, (int64_t)k) != nullptr));
    }
    REQUIRE(got.err_off[K] == want.err_off[K]);
    for (size_t i = 0; i < NR; ++i) REQUIRE(got.lower[i] == want.lower[i] && got.upper[i] == want.upper[i] && value[i] == b.read_val[i]);
    for (size_t i = 0; i < (size_t)want.r.n_err; ++i) REQUIRE(got.err_idx[i] == want.err_idx[i]);
    if (want.r.n_err) {  // a capacity one too small: the count comes back, the rest is written
        Out small(K, NR, want.r.n_err - 1);
        REQUIRE(lc_counter_stream_results(s, &small.r, nullptr) == LC_E_NOMEM && small.r.n_err == want.r.n_err);
        for (size_t k = 0; k <= K; ++k) REQUIRE(small.err_off[k] == want.err_off[k]);
        for (size_t i = 0; i < NR; ++i) REQUIRE(small.lower[i] == want.lower[i] && small.upper[i] == want.upper[i]);
    }
    lc_counter_packed_free(p);
    return 0;
}

// Random rows: per key a few processes with open invocations.
static void generate(Rows &R, size_t n, int n_keys) {
    struct Op { uint8_t f; int64_t v; };
    std::vector<std::map<int64_t, Op>> open((size_t)(n_keys ? n_keys : 1));
    std::vector<int64_t> lower(open.size(), 0), upper(open.size(), 0);
    while (R.n() < n) {
        if (chance(40)) {
            R.add(LC_INFO, LC_CF_OTHER, LC_NO_PROCESS, LC_NIL);
            continue;
        }
        const size_t ki = (size_t)(rnd() % open.size());
        const int64_t k = n_keys ? (int64_t)(10 + ki) : LC_NO_KEY;
        auto &o = open[ki];
        if (R.n() > n / 2 && rnd() % 4000 == 0) {  // a permanent error, late
            if (chance(500)) R.add(LC_OK_T, LC_CF_ADD, 90, 1, k);
            else { R.add(LC_INVOKE, LC_CF_READ, 91, LC_NIL, k); R.add(LC_OK_T, LC_CF_READ, 91, LC_NIL, k); }
            continue;
        }
        const int64_t p = (int64_t)(rnd() % 5);
        if (!o.count(p)) {
            if (chance(500)) {
                int64_t v = (int64_t)(rnd() % 10);
                if (chance(15)) v = LC_NIL;
                else if (chance(15)) v = -3;
                else if (chance(10)) v = INT64_MAX - (int64_t)(rnd() % 3);
                o[p] = Op{LC_CF_ADD, v};
                if (v >= 0) upper[ki] += v < 1000 ? v : 0;
                R.add(LC_INVOKE, LC_CF_ADD, p, v, k);
            } else {
                o[p] = Op{LC_CF_READ, 0};
                R.add(LC_INVOKE, LC_CF_READ, p, LC_NIL, k);
            }
            continue;
        }
        const Op op = o[p];
        o.erase(p);
        const unsigned c = (unsigned)(rnd() % 10);
        uint8_t t = c < 6 ? LC_OK_T : c < 9 ? LC_FAIL : LC_INFO;
        if (op.f == LC_CF_ADD) {
            int64_t v = op.v;
            if (v == LC_NIL || v < 0 || v > 1000) {  // a bad or huge add: mostly failed, sometimes replaced by a good value
                t = chance(700) ? LC_FAIL : chance(980) ? LC_OK_T : LC_INFO;
                if (t == LC_OK_T) v = 4;
            } else if (t == LC_OK_T && chance(100)) {
                v += 2;  // the :ok's value replaces the invocation's
            }
            if (t == LC_OK_T) lower[ki] += v;
            R.add(t, LC_CF_ADD, p, v, k);
        } else {
            const int64_t span = upper[ki] - lower[ki] + 3;
            R.add(t, LC_CF_READ, p, t == LC_OK_T ? lower[ki] - 1 + (int64_t)(rnd() % (uint64_t)span) : LC_NIL, k);
        }
    }
}

static int64_t g_patched, g_revisited, g_changed;

static int run(bool keyed, uint32_t reads0) {
    Rows R;
    generate(R, 20000, keyed ? 3 : 0);
    lc_counter_stream *s = nullptr;
    lc_counter_stream_opts o{256, reads0, 0, 0};
    REQUIRE(lc_counter_stream_open(nullptr, &o, &s) == LC_OK && s);
    REQUIRE(same(s, R, keyed, 0) == 0);
    size_t at = 0;
    int64_t patched = 0, revisited = 0, changed = 0;
    while (at < R.n()) {
        size_t step = chance(100) ? 0 : (size_t)(rnd() % (chance(200) ? 2000 : 40));
        if (at + step > R.n()) step = R.n() - at;
        lc_counter_history h = R.view(keyed, at, at + step);
        lc_counter_stream_update u{};
        REQUIRE(lc_counter_stream_append(s, &h, &u) == LC_OK);
        at += step;
        REQUIRE(u.rows == (int64_t)at);
        patched += u.patched; revisited += u.revisited; changed += u.n_changed;
        if (same(s, R, keyed, at)) return 1;
    }
    g_patched += patched; g_revisited += revisited; g_changed += changed;
    double ms[6];
    REQUIRE(lc_counter_stream_last_timing(s, ms) == LC_OK && ms[5] >= ms[0]);
    lc_counter_stream_close(s);
    return 0;
}

int main() {
    if (run(true, 16) || run(false, 0)) return 1;
    // the histories did revise earlier answers
    REQUIRE(g_patched > 100 && g_revisited > 100 && g_changed > 3);
    {   // refusals leave the stream as it was
        Rows R;
        R.add(LC_INVOKE, LC_CF_ADD, 0, 3, 7); R.add(LC_INVOKE, LC_CF_READ, 1, LC_NIL, 7); R.add(LC_OK_T, LC_CF_READ, 1, 9, 7);
        R.add(LC_OK_T, LC_CF_ADD, 0, 3);                       // row 3: no key
        R.add(LC_FAIL, LC_CF_ADD, 0, 3, 8);                    // row 4: another key, an orphan
        lc_counter_stream *s = nullptr;
        REQUIRE(lc_counter_stream_open(nullptr, nullptr, &s) == LC_OK);
        lc_counter_history h = R.view(true, 0, 3);
        REQUIRE(lc_counter_stream_append(s, &h, nullptr) == LC_OK);
        REQUIRE(same(s, R, true, 3) == 0);
        lc_counter_history hu = R.view(false, 3, 4);           // unkeyed rows to a keyed stream
        REQUIRE(lc_counter_stream_append(s, &hu, nullptr) == LC_E_INVALID);
        REQUIRE(same(s, R, true, 3) == 0);
        Rows B = R;
        B.type[4] = 4;
        lc_counter_history hb = B.view(true, 4, 5);
        REQUIRE(lc_counter_stream_append(s, &hb, nullptr) == LC_E_INVALID);
        B.type[4] = LC_FAIL; B.f[4] = 3;
        REQUIRE(lc_counter_stream_append(s, &hb, nullptr) == LC_E_INVALID);
        hb.n = -1;
        REQUIRE(lc_counter_stream_append(s, &hb, nullptr) == LC_E_INVALID);
        hb.n = 1; hb.type = nullptr;
        REQUIRE(lc_counter_stream_append(s, &hb, nullptr) == LC_E_INVALID);
        REQUIRE(lc_counter_stream_append(s, nullptr, nullptr) == LC_E_INVALID && lc_counter_stream_append(nullptr, &h, nullptr) == LC_E_INVALID);
        REQUIRE(lc_counter_stream_keys(s, nullptr) == 1 && same(s, R, true, 3) == 0);
        lc_counter_history h2 = R.view(true, 3, 5);            // (row 3 has no key: ignored)
        lc_counter_stream_update u{};
        REQUIRE(lc_counter_stream_append(s, &h2, &u) == LC_OK && u.n_keys == 2 && u.n_changed == 1 && u.changed[0] == 1);
        REQUIRE(same(s, R, true, 5) == 0);
        REQUIRE(lc_counter_stream_key_error(s, 1) && !lc_counter_stream_key_error(s, 0) && !lc_counter_stream_key_error(s, 2));
        lc_counter_stream_close(s);
        lc_counter_stream_close(nullptr);
    }
    {
        lc_counter_stream *s = nullptr;
        lc_counter_stream_opts o{100, 0, 0, 0};
        REQUIRE(lc_counter_stream_open(nullptr, &o, &s) == LC_E_INVALID && !s);
        o = lc_counter_stream_opts{0, 0, 0, 2};
        REQUIRE(lc_counter_stream_open(nullptr, &o, &s) == LC_E_INVALID && !s);
        REQUIRE(lc_counter_stream_open(nullptr, nullptr, nullptr) == LC_E_INVALID);
        int64_t info[6];
        REQUIRE(lc_counter_stream_launch_info(info) == LC_OK && info[0] == 256 && info[2] == 33 && lc_counter_stream_launch_info(nullptr) == LC_E_INVALID);
    }
    std::printf("ok\n");
    return 0;
}
