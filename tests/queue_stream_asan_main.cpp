// A stand-alone driver of the streaming total-queue / unique-ids' packer and
// host fold for the sanitizer test (tests/test_queue_stream_host.py): built
// with -fsanitize=address,undefined together with csrc/host_queue_stream.cpp
// and csrc/host_queue.cpp and nothing else.  The streams are host streams
// (no context), so no device function is reached -- the device half's
// functions are weak and absent here; the few helpers of csrc/common.cpp that
// those files use are given here, since common.cpp itself needs the HIP
// runtime.
//
// Appends the hand example row by row, 30,000 random rows (three keys or none,
// drains, crashed drains late in the history, nil values, nemesis rows) cut at
// random points, empty appends and appends of ignored rows, in both modes, and
// after EVERY append requires the stream's keys, counts and sorted entries to
// equal lc_queue_pack + lc_queue_check_host of the prefix; then the refusals
// (bad codes, the other kind, bad options) that must leave a stream as it was,
// and an entry capacity that is too small.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "common.hpp"
#include "../include/lincheck_queue_stream.h"

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

struct Rows {
    std::vector<uint8_t> type, f;
    std::vector<int64_t> key, value, drain_val;
    std::vector<uint64_t> drain_off{0};
    void add(uint8_t t, uint8_t fn, int64_t v, int64_t k = LC_NO_KEY, std::vector<int64_t> drained = {}) {
        type.push_back(t); f.push_back(fn); key.push_back(k); value.push_back(v);
        drain_val.insert(drain_val.end(), drained.begin(), drained.end());
        drain_off.push_back(drain_val.size());
    }
    size_t n() const { return type.size(); }
    // rows [lo, hi) as a history of their own (drain_off is not rebased: the library reads differences)
    lc_queue_history view(bool keyed, size_t lo, size_t hi) const {
        lc_queue_history h{};
        h.n = (int64_t)(hi - lo);
        h.type = type.data() + lo; h.f = f.data() + lo; h.key = keyed ? key.data() + lo : nullptr; h.value = value.data() + lo;
        h.drain_off = drain_off.data() + lo; h.drain_val = drain_val.data();
        return h;
    }
};

struct Out {
    std::vector<int8_t> valid;
    std::vector<uint64_t> counts, mult;
    std::vector<int64_t> lo, hi, val;
    std::vector<uint8_t> has, cls;
    std::vector<uint32_t> key;
    lc_queue_result r{};
    Out(size_t K, uint64_t cap) {
        valid.assign(K + 1, 9); counts.assign(K * LC_QN_COUNTS + 1, 99); lo.assign(K + 1, 0); hi.assign(K + 1, 0); has.assign(K + 1, 9);
        key.resize(cap + 1); cls.resize(cap + 1); val.resize(cap + 1); mult.resize(cap + 1);
        r.valid = valid.data(); r.counts = counts.data(); r.lo = lo.data(); r.hi = hi.data(); r.has_range = has.data();
        r.ent_key = key.data(); r.ent_class = cls.data(); r.ent_val = val.data(); r.ent_mult = mult.data();
        r.ent_cap = cap; r.n_ent = 0;
    }
};

#define REQUIRE(c)                                                          \
    do {                                                                    \
        if (!(c)) {                                                         \
            std::fprintf(stderr, "line %d: %s (%s)\n", __LINE__, #c, lc::g_err.c_str()); \
            return 1;                                                       \
        }                                                                   \
    } while (0)

static uint64_t g_rng = 0x243F6A8885A308D3ull;
static uint64_t rnd() {
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return g_rng;
}

// The stream equals the one-shot host check of rows [0, upto).
static int same(lc_queue_stream *s, const Rows &R, bool keyed, size_t upto, uint32_t mode) {
    lc_queue_history h = R.view(keyed, 0, upto);
    lc_queue_packed *p = nullptr;
    REQUIRE(lc_queue_pack(&h, mode, &p) == LC_OK);
    lc_queue_batch b{};
    REQUIRE(lc_queue_packed_view(p, &b) == LC_OK);
    const size_t K = (size_t)b.n_keys;
    const uint64_t cap = 2 * (uint64_t)b.n_rows + 1;
    Out want(K, cap), got(K, cap), cheap(K, 0);
    REQUIRE(lc_queue_check_host(&b, &want.r) == LC_OK);
    REQUIRE(lc_queue_stream_keys(s, nullptr) == (int64_t)K);
    std::vector<int64_t> k1(K + 1), k2(K + 1);
    REQUIRE(lc_queue_stream_keys(s, k1.data()) == (int64_t)K && lc_queue_packed_keys(p, k2.data()) == LC_OK);
    REQUIRE(std::memcmp(k1.data(), k2.data(), K * 8) == 0);
    REQUIRE(lc_queue_stream_results(s, &got.r) == LC_OK && got.r.n_ent == want.r.n_ent);
    REQUIRE(lc_queue_stream_counts(s, cheap.valid.data(), cheap.counts.data(), cheap.lo.data(), cheap.hi.data(), cheap.has.data()) == LC_OK);
    for (const Out *o : {&got, &cheap}) {
        REQUIRE(std::memcmp(o->valid.data(), want.valid.data(), K) == 0);
        REQUIRE(std::memcmp(o->counts.data(), want.counts.data(), K * LC_QN_COUNTS * 8) == 0);
        REQUIRE(std::memcmp(o->has.data(), want.has.data(), K) == 0);
        for (size_t k = 0; k < K; ++k) REQUIRE(!want.has[k] || (o->lo[k] == want.lo[k] && o->hi[k] == want.hi[k]));
    }
    const size_t ne = (size_t)want.r.n_ent;
    REQUIRE(std::memcmp(got.key.data(), want.key.data(), ne * 4) == 0 && std::memcmp(got.cls.data(), want.cls.data(), ne) == 0);
    REQUIRE(std::memcmp(got.val.data(), want.val.data(), ne * 8) == 0 && std::memcmp(got.mult.data(), want.mult.data(), ne * 8) == 0);
    for (size_t k = 0; k < K; ++k) {
        const char *e1 = lc_queue_stream_key_error(s, (int64_t)k), *e2 = lc_queue_packed_key_error(p, (int64_t)k);
        REQUIRE(!e1 == !e2 && (!e1 || std::strcmp(e1, e2) == 0));
    }
    if (ne > 1) {  // an entry capacity that is too small: the count comes back, the rest is written
        Out small(K, ne - 1);
        REQUIRE(lc_queue_stream_results(s, &small.r) == LC_E_NOMEM && small.r.n_ent == ne);
        REQUIRE(std::memcmp(small.counts.data(), want.counts.data(), K * LC_QN_COUNTS * 8) == 0);
    }
    lc_queue_packed_free(p);
    return 0;
}

static void hand(Rows &R, int64_t k) {
    const int64_t nil = LC_NIL;
    R.add(LC_INVOKE, LC_QF_ENQUEUE, 1, k); R.add(LC_OK_T, LC_QF_ENQUEUE, 1, k);
    R.add(LC_INVOKE, LC_QF_ENQUEUE, 2, k); R.add(LC_OK_T, LC_QF_ENQUEUE, 2, k);
    R.add(LC_INVOKE, LC_QF_ENQUEUE, 3, k); R.add(LC_INFO, LC_QF_ENQUEUE, 3, k);
    R.add(LC_INVOKE, LC_QF_ENQUEUE, 4, k); R.add(LC_FAIL, LC_QF_ENQUEUE, 4, k);
    R.add(LC_INVOKE, LC_QF_DEQUEUE, nil, k); R.add(LC_OK_T, LC_QF_DEQUEUE, 1, k);
    R.add(LC_INVOKE, LC_QF_GENERATE, nil, k); R.add(LC_OK_T, LC_QF_GENERATE, 7, k);
    R.add(LC_OK_T, LC_QF_DEQUEUE, 1, k); R.add(LC_OK_T, LC_QF_GENERATE, 7, k);
    R.add(LC_INFO, LC_QF_OTHER, nil, LC_NO_KEY);
    R.add(LC_INVOKE, LC_QF_DRAIN, nil, k); R.add(LC_OK_T, LC_QF_DRAIN, nil, k, {3, 9, nil});
    R.add(LC_OK_T, LC_QF_GENERATE, nil, k); R.add(LC_OK_T, LC_QF_GENERATE, INT64_MAX, k);
}

static void random_rows(Rows &R, size_t n, bool keyed, bool crash) {
    for (size_t i = 0; i < n; ++i) {
        const int64_t k = keyed ? (int64_t)(rnd() % 3) * 7 - 3 : LC_NO_KEY;
        const int64_t v = rnd() % 12 == 0 ? LC_NIL : (int64_t)(rnd() % 40) + 1;
        const uint64_t u = rnd() % 100;
        const uint8_t t = (uint8_t)(rnd() % 4);
        if (u < 5) R.add(LC_INFO, LC_QF_OTHER, LC_NIL, LC_NO_KEY);
        else if (u < 45) R.add(t, LC_QF_ENQUEUE, v, k);
        else if (u < 70) R.add(t == LC_INFO ? LC_OK_T : t, LC_QF_DEQUEUE, v, k);
        else if (u < 80) {
            const bool info = crash && i > n / 2 && rnd() % 400 == 0;
            std::vector<int64_t> d;
            for (uint64_t j = rnd() % 4; j > 0; --j) d.push_back((int64_t)(rnd() % 40) + 1);
            const uint8_t dt = info ? LC_INFO : t == LC_INFO ? LC_OK_T : t;
            R.add(dt, LC_QF_DRAIN, LC_NIL, k, dt == LC_OK_T ? d : std::vector<int64_t>{});
        } else R.add(t, LC_QF_GENERATE, v, k);
    }
}

static int stream_through(const Rows &R, bool keyed, uint32_t mode, size_t max_step) {
    lc_queue_stream *s = nullptr;
    lc_queue_stream_opts o{256, 0};
    REQUIRE(lc_queue_stream_open(nullptr, mode, &o, &s) == LC_OK && s);
    if (same(s, R, keyed, 0, mode)) return 1;
    size_t at = 0;
    int64_t packed = 0;
    while (at < R.n()) {
        const size_t step = max_step == 1 ? 1 : (size_t)(rnd() % max_step);  // (0: an empty append)
        const size_t to = std::min(R.n(), at + step);
        lc_queue_history h = R.view(keyed, at, to);
        lc_queue_stream_update u{};
        REQUIRE(lc_queue_stream_append(s, &h, &u) == LC_OK);
        at = to;
        packed += u.packed;
        REQUIRE(u.rows == (int64_t)at && u.slots >= u.distinct && u.distinct <= packed && (u.slots & (u.slots - 1)) == 0);
        if (same(s, R, keyed, at, mode)) return 1;
    }
    double ms[6];
    REQUIRE(lc_queue_stream_last_timing(s, ms) == LC_OK && ms[5] >= ms[0]);
    lc_queue_stream_close(s);
    return 0;
}

int main() {
    for (uint32_t mode : {(uint32_t)LC_QM_TOTAL_QUEUE, (uint32_t)LC_QM_UNIQUE_IDS}) {
        for (int keyed = 0; keyed < 2; ++keyed) {
            Rows R;
            hand(R, keyed ? 5 : LC_NO_KEY);
            if (keyed) hand(R, -8);
            if (stream_through(R, keyed != 0, mode, 1)) return 1;
            Rows big;
            random_rows(big, 30000, keyed != 0, true);
            if (stream_through(big, keyed != 0, mode, 6000)) return 1;
            Rows small;
            random_rows(small, 300, keyed != 0, false);
            if (stream_through(small, keyed != 0, mode, 9)) return 1;
        }
    }
    // refusals leave the stream as it was
    {
        Rows R;
        hand(R, 5);
        lc_queue_stream *s = nullptr;
        REQUIRE(lc_queue_stream_open(nullptr, LC_QM_TOTAL_QUEUE, nullptr, &s) == LC_OK);
        lc_queue_history h = R.view(true, 0, R.n());
        REQUIRE(lc_queue_stream_append(s, &h, nullptr) == LC_OK);
        Rows U;
        hand(U, LC_NO_KEY);
        lc_queue_history hu = U.view(false, 0, U.n());
        REQUIRE(lc_queue_stream_append(s, &hu, nullptr) == LC_E_INVALID);
        if (same(s, R, true, R.n(), LC_QM_TOTAL_QUEUE)) return 1;
        Rows B;
        B.add(LC_OK_T, LC_QF_ENQUEUE, 1, 77); B.add(LC_INFO, LC_QF_DRAIN, LC_NIL, 5); B.add(7, LC_QF_ENQUEUE, 1, 5);
        lc_queue_history hb = B.view(true, 0, B.n());
        REQUIRE(lc_queue_stream_append(s, &hb, nullptr) == LC_E_INVALID);
        B.type[2] = LC_OK_T; B.f[2] = LC_QF_OTHER + 1;
        REQUIRE(lc_queue_stream_append(s, &hb, nullptr) == LC_E_INVALID);
        B.f[2] = LC_QF_ENQUEUE; B.drain_off[2] = 5;
        REQUIRE(lc_queue_stream_append(s, &hb, nullptr) == LC_E_INVALID);
        if (same(s, R, true, R.n(), LC_QM_TOTAL_QUEUE)) return 1;
        REQUIRE(lc_queue_stream_keys(s, nullptr) == 1 && !lc_queue_stream_key_error(s, 0));
        hb.n = -1;
        REQUIRE(lc_queue_stream_append(s, &hb, nullptr) == LC_E_INVALID);
        REQUIRE(lc_queue_stream_append(s, nullptr, nullptr) == LC_E_INVALID && lc_queue_stream_append(nullptr, &h, nullptr) == LC_E_INVALID);
        // the same rows made good are taken: key 77 appears, key 5 goes :unknown
        B.drain_off[2] = 0;
        hb.n = 3;
        lc_queue_stream_update u{};
        REQUIRE(lc_queue_stream_append(s, &hb, &u) == LC_OK && u.n_keys == 2 && u.n_changed == 2 && u.changed[0] == 0 && u.changed[1] == 1);
        REQUIRE(lc_queue_stream_key_error(s, 0) && std::strstr(lc_queue_stream_key_error(s, 0), "crashed drain"));
        lc_queue_stream_close(s);
        lc_queue_stream_close(nullptr);
    }
    // bad options; launch constants
    {
        lc_queue_stream *s = nullptr;
        lc_queue_stream_opts o{3, 0};
        REQUIRE(lc_queue_stream_open(nullptr, LC_QM_TOTAL_QUEUE, &o, &s) == LC_E_INVALID && !s);
        o.slots = 0; o.flags = 1;
        REQUIRE(lc_queue_stream_open(nullptr, LC_QM_TOTAL_QUEUE, &o, &s) == LC_E_INVALID && !s);
        o.flags = 0;
        REQUIRE(lc_queue_stream_open(nullptr, 2, &o, &s) == LC_E_INVALID && lc_queue_stream_open(nullptr, 0, &o, nullptr) == LC_E_INVALID);
        int64_t info[6];
        REQUIRE(lc_queue_stream_launch_info(info) == LC_OK && info[0] == 256 && info[2] == 48 && lc_queue_stream_launch_info(nullptr) == LC_E_INVALID);
    }
    std::printf("ok\n");
    return 0;
}
