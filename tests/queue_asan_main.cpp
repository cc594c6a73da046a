// A stand-alone driver of checker/total-queue's and /unique-ids' packer, host
// fold and EDN reader for the sanitizer test (tests/test_queue_host.py): built
// with -fsanitize=address,undefined together with csrc/host_queue.cpp and
// csrc/host_edn.cpp and nothing else.  No device function is reached; the few
// helpers of csrc/common.cpp that those files use are given here, since
// common.cpp itself needs the HIP runtime.
//
// Feeds lc_queue_pack + lc_queue_check_host the hand example (and requires its
// counts and entries), a crashed drain beside healthy keys, an ent_cap that is
// too small, caller-built batches that must be refused, the empty history,
// unique-ids with its range, 20,000 random keyed rows with every kind of row in
// them, and lc_edn_parse_queue texts: tuples, drains, refused values, broken
// syntax cut at every length.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "common.hpp"
#include "../include/lincheck_queue.h"

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
    lc_queue_history view(bool keyed) const {
        lc_queue_history h{};
        h.n = (int64_t)type.size();
        h.type = type.data(); h.f = f.data(); h.key = keyed ? key.data() : nullptr; h.value = value.data();
        h.drain_off = drain_off.data(); h.drain_val = drain_val.data();
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
    Out(const lc_queue_batch &b, uint64_t cap) {
        const size_t K = (size_t)b.n_keys;
        valid.resize(K + 1); counts.resize(K * LC_QN_COUNTS + 1); lo.resize(K + 1); hi.resize(K + 1); has.resize(K + 1);
        key.resize(cap + 1); cls.resize(cap + 1); val.resize(cap + 1); mult.resize(cap + 1);
        r.valid = valid.data(); r.counts = counts.data(); r.lo = lo.data(); r.hi = hi.data(); r.has_range = has.data();
        r.ent_key = key.data(); r.ent_class = cls.data(); r.ent_val = val.data(); r.ent_mult = mult.data();
        r.ent_cap = cap; r.n_ent = 0;
    }
    const uint64_t *of(int64_t k) const { return counts.data() + (size_t)k * LC_QN_COUNTS; }
};

#define REQUIRE(c)                                                          \
    do {                                                                    \
        if (!(c)) {                                                         \
            std::fprintf(stderr, "line %d: %s (%s)\n", __LINE__, #c, lc::g_err.c_str()); \
            return 1;                                                       \
        }                                                                   \
    } while (0)

// tests/queue_helpers.py's HAND_QUEUE at key k.
static void hand(Rows &R, int64_t k) {
    const int64_t nil = LC_NIL;
    R.add(LC_INVOKE, LC_QF_ENQUEUE, 1, k); R.add(LC_OK_T, LC_QF_ENQUEUE, 1, k);
    R.add(LC_INVOKE, LC_QF_ENQUEUE, 2, k); R.add(LC_OK_T, LC_QF_ENQUEUE, 2, k);
    R.add(LC_INVOKE, LC_QF_ENQUEUE, 3, k); R.add(LC_INFO, LC_QF_ENQUEUE, 3, k);
    R.add(LC_INVOKE, LC_QF_ENQUEUE, 4, k); R.add(LC_FAIL, LC_QF_ENQUEUE, 4, k);
    R.add(LC_INVOKE, LC_QF_DEQUEUE, nil, k); R.add(LC_OK_T, LC_QF_DEQUEUE, 1, k);
    R.add(LC_INVOKE, LC_QF_DEQUEUE, nil, k); R.add(LC_OK_T, LC_QF_DEQUEUE, 1, k);
    R.add(LC_INVOKE, LC_QF_DEQUEUE, nil, k); R.add(LC_FAIL, LC_QF_DEQUEUE, nil, k);
    R.add(LC_INFO, LC_QF_OTHER, nil, LC_NO_KEY);
    R.add(LC_INVOKE, LC_QF_DRAIN, nil, k); R.add(LC_OK_T, LC_QF_DRAIN, nil, k, {3, 9, nil});
}

// The hand example's counts at key k, and its five entries from `e` on.
static bool hand_ok(const Out &o, int64_t k, uint64_t e) {
    const uint64_t want[LC_QN_COUNTS] = {4, 2, 2, 2, 1, 1, 1};
    if (o.valid[(size_t)k] != LC_INVALID || std::memcmp(o.of(k), want, sizeof want) != 0) return false;
    const uint8_t cls[5] = {LC_QC_LOST, LC_QC_UNEXPECTED, LC_QC_UNEXPECTED, LC_QC_DUPLICATED, LC_QC_RECOVERED};
    const int64_t val[5] = {2, LC_NIL, 9, 1, 3};
    for (int i = 0; i < 5; ++i)
        if (o.key[e + i] != (uint32_t)k || o.cls[e + i] != cls[i] || o.val[e + i] != val[i] || o.mult[e + i] != 1) return false;
    return true;
}

static int parse(const std::string &s, lc_queue_hist **h) { return lc_edn_parse_queue(s.data(), (int64_t)s.size(), h); }

int main() {
    // the hand example, one key without tuples
    {
        Rows R;
        hand(R, LC_NO_KEY);
        lc_queue_history h = R.view(false);
        lc_queue_packed *p = nullptr;
        REQUIRE(lc_queue_pack(&h, LC_QM_TOTAL_QUEUE, &p) == LC_OK);
        lc_queue_batch b{};
        REQUIRE(lc_queue_packed_view(p, &b) == LC_OK && b.n_keys == 1 && b.n_rows == 11 && b.mode == LC_QM_TOTAL_QUEUE);
        Out o(b, 5);
        REQUIRE(lc_queue_check_host(&b, &o.r) == LC_OK && o.r.n_ent == 5 && hand_ok(o, 0, 0));
        Out small(b, 4);
        REQUIRE(lc_queue_check_host(&b, &small.r) == LC_E_NOMEM && small.r.n_ent == 5 && small.of(0)[LC_QN_LOST] == 1);
        Out none(b, 0);
        none.r.ent_key = nullptr; none.r.ent_class = nullptr; none.r.ent_val = nullptr; none.r.ent_mult = nullptr;
        REQUIRE(lc_queue_check_host(&b, &none.r) == LC_E_NOMEM && none.r.n_ent == 5);
        int64_t key = 0;
        REQUIRE(lc_queue_packed_keys(p, &key) == LC_OK && key == LC_NO_KEY && !lc_queue_packed_key_error(p, 0));
        lc_queue_packed_free(p);
        // the same rows as ids: nothing is a :generate
        REQUIRE(lc_queue_pack(&h, LC_QM_UNIQUE_IDS, &p) == LC_OK);
        REQUIRE(lc_queue_packed_view(p, &b) == LC_OK && b.n_keys == 1 && b.n_rows == 0);
        Out ids(b, 0);
        REQUIRE(lc_queue_check_host(&b, &ids.r) == LC_OK && ids.valid[0] == LC_VALID && ids.has[0] == 0);
        lc_queue_packed_free(p);
    }
    // a crashed drain as key 1 between two hand examples
    {
        Rows R;
        hand(R, 0);
        R.add(LC_OK_T, LC_QF_DEQUEUE, 5, 1); R.add(LC_INFO, LC_QF_DRAIN, LC_NIL, 1); R.add(LC_OK_T, LC_QF_DRAIN, LC_NIL, 1, {1, 2});
        hand(R, 2);
        lc_queue_history h = R.view(true);
        lc_queue_packed *p = nullptr;
        REQUIRE(lc_queue_pack(&h, LC_QM_TOTAL_QUEUE, &p) == LC_OK);
        lc_queue_batch b{};
        REQUIRE(lc_queue_packed_view(p, &b) == LC_OK && b.n_keys == 3 && b.n_rows == 22);
        REQUIRE(b.status[1] == LC_QUEUE_KEY_ERROR && lc_queue_packed_key_error(p, 1) && !lc_queue_packed_key_error(p, 2));
        REQUIRE(std::strstr(lc_queue_packed_key_error(p, 1), "crashed drain"));
        Out o(b, 10);
        REQUIRE(lc_queue_check_host(&b, &o.r) == LC_OK && o.r.n_ent == 10);
        REQUIRE(hand_ok(o, 0, 0) && hand_ok(o, 2, 5) && o.valid[1] == LC_UNKNOWN && o.of(1)[LC_QN_UNEXPECTED] == 0);
        // caller-built batches that must be refused
        std::vector<uint32_t> rk(b.row_key, b.row_key + b.n_rows);
        std::vector<uint8_t> kind(b.row_kind, b.row_kind + b.n_rows);
        lc_queue_batch c = b;
        c.row_key = rk.data(); c.row_kind = kind.data();
        rk[21] = 3;
        REQUIRE(lc_queue_check_host(&c, &o.r) == LC_E_INVALID);
        rk[21] = 2; kind[0] = 3;
        REQUIRE(lc_queue_check_host(&c, &o.r) == LC_E_INVALID);
        kind[0] = LC_QK_ATTEMPT; c.mode = LC_QM_UNIQUE_IDS;
        REQUIRE(lc_queue_check_host(&c, &o.r) == LC_E_INVALID);
        c.mode = 2;
        REQUIRE(lc_queue_check_host(&c, &o.r) == LC_E_INVALID);
        c.mode = LC_QM_TOTAL_QUEUE; c.n_rows = -1;
        REQUIRE(lc_queue_check_host(&c, &o.r) == LC_E_INVALID);
        c.n_rows = b.n_rows;
        rk[0] = 1;  // a row of the error key contributes nothing
        REQUIRE(lc_queue_check_host(&c, &o.r) == LC_OK && o.of(0)[LC_QN_ATTEMPT] == 3 && o.of(1)[LC_QN_ATTEMPT] == 0);
        lc_queue_packed_free(p);
    }
    // bad codes, nulls, the empty history
    {
        Rows R;
        hand(R, LC_NO_KEY);
        R.type[2] = 7;
        lc_queue_history h = R.view(false);
        lc_queue_packed *p = nullptr;
        REQUIRE(lc_queue_pack(&h, LC_QM_TOTAL_QUEUE, &p) == LC_E_INVALID && !p);
        R.type[2] = LC_INVOKE; R.f[3] = LC_QF_OTHER + 1;
        REQUIRE(lc_queue_pack(&h, LC_QM_TOTAL_QUEUE, &p) == LC_E_INVALID && !p);
        R.f[3] = LC_QF_ENQUEUE;
        REQUIRE(lc_queue_pack(&h, 2, &p) == LC_E_INVALID && lc_queue_pack(nullptr, 0, &p) == LC_E_INVALID);
        R.drain_off[5] = 9;
        REQUIRE(lc_queue_pack(&h, LC_QM_TOTAL_QUEUE, &p) == LC_E_INVALID && !p);
        lc_queue_history e{};
        REQUIRE(lc_queue_pack(&e, LC_QM_TOTAL_QUEUE, &p) == LC_OK);
        lc_queue_batch b{};
        REQUIRE(lc_queue_packed_view(p, &b) == LC_OK && b.n_keys == 1 && b.n_rows == 0);
        Out o(b, 0);
        REQUIRE(lc_queue_check_host(&b, &o.r) == LC_OK && o.valid[0] == LC_VALID && o.r.n_ent == 0);
        lc_queue_packed_free(p);
        int64_t info[4];
        REQUIRE(lc_queue_launch_info(info) == LC_OK && info[0] == 256 && info[2] == 16);
    }
    // unique-ids: counts, the range with nil and INT64_MAX, a key without acks
    {
        Rows R;
        for (int64_t v : {(int64_t)5, (int64_t)INT64_MAX, (int64_t)LC_NIL, (int64_t)5, (int64_t)-3, (int64_t)5}) {
            R.add(LC_INVOKE, LC_QF_GENERATE, LC_NIL, 10);
            R.add(LC_OK_T, LC_QF_GENERATE, v, 10);
        }
        R.add(LC_INVOKE, LC_QF_GENERATE, LC_NIL, 20); R.add(LC_FAIL, LC_QF_GENERATE, LC_NIL, 20);
        lc_queue_history h = R.view(true);
        lc_queue_packed *p = nullptr;
        REQUIRE(lc_queue_pack(&h, LC_QM_UNIQUE_IDS, &p) == LC_OK);
        lc_queue_batch b{};
        REQUIRE(lc_queue_packed_view(p, &b) == LC_OK && b.n_keys == 2 && b.n_rows == 6 && b.attempted[0] == 6 && b.attempted[1] == 1);
        Out o(b, 2);
        o.lo[1] = o.hi[1] = 77;
        REQUIRE(lc_queue_check_host(&b, &o.r) == LC_OK && o.r.n_ent == 1 && o.valid[0] == LC_INVALID && o.valid[1] == LC_VALID);
        REQUIRE(o.of(0)[0] == 6 && o.of(0)[1] == 6 && o.of(0)[2] == 1 && o.of(1)[0] == 1 && o.of(1)[1] == 0);
        REQUIRE(o.has[0] == 1 && o.lo[0] == LC_NIL && o.hi[0] == INT64_MAX && o.has[1] == 0 && o.lo[1] == 77 && o.hi[1] == 77);
        REQUIRE(o.key[0] == 0 && o.cls[0] == LC_QC_DUPLICATED && o.val[0] == 5 && o.mult[0] == 3);
        lc_queue_packed_free(p);
    }
    // 20,000 random rows over 7 interleaved keys, both modes; the totals are those of a direct count
    for (uint32_t mode = 0; mode < 2; ++mode) {
        Rows R;
        uint64_t x = 88172645463325252ull;
        auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
        uint64_t attempts = 0, acks = 0, deqs = 0, gen_ok = 0;
        for (int i = 0; i < 20000; ++i) {
            const int64_t k = (int64_t)(rnd() % 7);
            const uint64_t what = rnd() % 100;
            if (what < 3) { R.add(LC_INFO, LC_QF_OTHER, LC_NIL, LC_NO_KEY); continue; }
            const uint8_t t = (uint8_t)(rnd() % 4), f = (uint8_t)(rnd() % 4);
            const int64_t v = what == 3 ? LC_NIL : (int64_t)(rnd() % 50) - 25;
            if (f == LC_QF_DRAIN) {
                if (t == LC_INFO) continue;  // (no crashed drains here: every key is checked)
                std::vector<int64_t> d;
                for (uint64_t j = rnd() % 4; j > 0; --j) d.push_back((int64_t)(rnd() % 50) - 25);
                if (t == LC_OK_T) deqs += d.size();
                R.add(t, f, LC_NIL, k, t == LC_OK_T ? d : std::vector<int64_t>{});
                continue;
            }
            attempts += f == LC_QF_ENQUEUE && t == LC_INVOKE;
            acks += f == LC_QF_ENQUEUE && t == LC_OK_T;
            deqs += f == LC_QF_DEQUEUE && t == LC_OK_T;
            gen_ok += f == LC_QF_GENERATE && t == LC_OK_T;
            R.add(t, f, v, k);
        }
        lc_queue_history h = R.view(true);
        lc_queue_packed *p = nullptr;
        REQUIRE(lc_queue_pack(&h, mode, &p) == LC_OK);
        lc_queue_batch b{};
        REQUIRE(lc_queue_packed_view(p, &b) == LC_OK && b.n_keys == 7);
        REQUIRE((uint64_t)b.n_rows == (mode ? gen_ok : attempts + acks + deqs));
        Out o(b, 2 * (uint64_t)b.n_rows);
        REQUIRE(lc_queue_check_host(&b, &o.r) == LC_OK);
        uint64_t sum[LC_QN_COUNTS] = {};
        for (int64_t k = 0; k < 7; ++k)
            for (int i = 0; i < LC_QN_COUNTS; ++i) sum[i] += o.of(k)[i];
        if (mode) {
            REQUIRE(sum[LC_QN_ACKNOWLEDGED] == gen_ok && sum[LC_QN_OK] == o.r.n_ent && o.r.n_ent > 0);
        } else {
            REQUIRE(sum[LC_QN_ATTEMPT] == attempts && sum[LC_QN_ACKNOWLEDGED] == acks);
            REQUIRE(sum[LC_QN_OK] + sum[LC_QN_UNEXPECTED] + sum[LC_QN_DUPLICATED] == deqs);  // every dequeue is one of the three
        }
        for (uint64_t e = 1; e < o.r.n_ent; ++e) {  // sorted by (key, class, value)
            const bool up = o.key[e - 1] != o.key[e] ? o.key[e - 1] < o.key[e]
                          : o.cls[e - 1] != o.cls[e] ? o.cls[e - 1] < o.cls[e] : o.val[e - 1] < o.val[e];
            REQUIRE(up);
        }
        lc_queue_packed_free(p);
    }
    // the EDN reader
    {
        const std::string text =
            "{:type :invoke, :f :enqueue, :value [7 12], :process 0}\n"
            "{:type :ok, :f :enqueue, :value [7 12], :process 0}\n"
            "; a comment\n"
            "{:type :info, :f :start, :value [1 \"x\" {:a #{1 2}}], :process :nemesis}\n"
            "{:type :ok, :f :drain, :value [7 [12 nil -4]], :process 1}\n"
            "{:type :ok, :f :drain, :value [1 2 3], :process 1}\n"
            "{:type :ok, :f :generate, :value 9223372036854775807}\n";
        lc_queue_hist *h = nullptr;
        REQUIRE(parse(text, &h) == LC_OK);
        lc_queue_history v{};
        REQUIRE(lc_queue_hist_view(h, &v) == LC_OK && v.n == 6 && v.drain_off[6] == 6 && v.drain_off[4] == 3);
        REQUIRE(v.key[0] == 7 && v.value[1] == 12 && v.f[2] == LC_QF_OTHER && v.key[3] == 7 && v.key[4] == LC_NO_KEY);
        REQUIRE(v.drain_val[1] == LC_NIL && v.drain_val[5] == 3 && v.value[5] == INT64_MAX);
        lc_queue_packed *p = nullptr;
        REQUIRE(lc_queue_pack(&v, LC_QM_TOTAL_QUEUE, &p) == LC_OK);
        lc_queue_batch b{};
        REQUIRE(lc_queue_packed_view(p, &b) == LC_OK && b.n_keys == 1 && b.n_rows == 5);
        lc_queue_packed_free(p);
        lc_queue_hist_free(h);
        // every prefix of the text either reads or fails cleanly
        for (size_t n = 0; n <= text.size(); ++n) {
            h = nullptr;
            const int rc = parse(text.substr(0, n), &h);
            REQUIRE(rc == LC_OK || rc == LC_E_PARSE || rc == LC_E_UNSUPPORTED);
            REQUIRE((rc == LC_OK) == (h != nullptr));
            lc_queue_hist_free(h);
        }
        const char *refused[] = {"{:type :ok, :f :enqueue, :value \"x\"}", "{:type :ok, :f :dequeue, :value [1 2 3]}",
                                 "{:type :ok, :f :drain, :value 7}", "{:type :ok, :f :drain, :value [7 [1 [2]]]}",
                                 "{:type :ok, :f :generate, :value 1.5}", "[{:type :ok, :f :enqueue, :value [7 :x]}]"};
        for (const char *t : refused) {
            h = nullptr;
            REQUIRE(parse(t, &h) == LC_E_UNSUPPORTED && !h);
        }
        REQUIRE(parse("{:f :enqueue, :value 1}", &h) == LC_E_PARSE && parse("{:type :ok, :f :drain, :value [1 2}", &h) == LC_E_PARSE);
        REQUIRE(lc_edn_read_queue("/nonexistent/history.edn", &h) == LC_E_IO);
    }
    std::printf("ok\n");
    return 0;
}
