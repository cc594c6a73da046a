// A stand-alone driver of the streaming set-full's packer for the sanitizer
// test (tests/test_setfull_stream_host.py): built with -fsanitize=address,
// undefined together with csrc/host_setfull_stream.cpp and nothing else.  The
// stream is packer-only (no context), so no device function is reached; the
// few helpers of csrc/common.cpp the packer uses are given here, since
// common.cpp itself needs the HIP runtime.
//
// Drives lc_setfull_stream_append over a few thousand rows of a keyed history
// in appends of uneven sizes: re-invoked elements, reads invoked in one append
// and completed in a later one, duplicates, empty reads, keys that grow past
// one block of ids, an error key, refused appends; then every accessor.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "common.hpp"
#include "../include/lincheck_setfull_stream.h"

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
}  // namespace lc

struct Rows {
    std::vector<uint8_t> type, f;
    std::vector<int64_t> key, elem, process, time, read_off{0}, read_elem;
    void add(uint8_t t, uint8_t fn, int64_t k, int64_t e, int64_t p, const std::vector<int64_t> &vals = {}) {
        type.push_back(t); f.push_back(fn); key.push_back(k); elem.push_back(e); process.push_back(p);
        time.push_back((int64_t)type.size() * 1000000);
        read_elem.insert(read_elem.end(), vals.begin(), vals.end());
        read_off.push_back((int64_t)read_elem.size());
    }
    lc_setfull_history slice(size_t b, size_t e, std::vector<int64_t> &off) const {
        off.assign(read_off.begin() + (long)b, read_off.begin() + (long)e + 1);
        lc_setfull_history h{};
        h.n = (int64_t)(e - b);
        h.type = type.data() + b; h.f = f.data() + b; h.key = key.data() + b; h.elem = elem.data() + b;
        h.read_off = off.data(); h.read_elem = read_elem.data();
        h.index = nullptr; h.process = process.data() + b; h.time = time.data() + b;
        return h;
    }
};

#define REQUIRE(c)                                                          \
    do {                                                                    \
        if (!(c)) {                                                         \
            std::fprintf(stderr, "line %d: %s (%s)\n", __LINE__, #c, lc::g_err.c_str()); \
            return 1;                                                       \
        }                                                                   \
    } while (0)

int main() {
    Rows R;
    uint64_t x = 88172645463325252ull;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    std::vector<std::vector<int64_t>> added(3);
    for (int i = 0; i < 2600; ++i) {
        const int64_t k = 10 + (int64_t)(rnd() % 3);
        auto &a = added[(size_t)(k - 10)];
        const uint64_t what = rnd() % 10;
        if (what < 6) {
            const int64_t e = (rnd() % 8 == 0 && !a.empty()) ? a[rnd() % a.size()] : (int64_t)(rnd() % 5000) - 50;
            R.add(LC_INVOKE, LC_SF_ADD, k, e, (int64_t)(rnd() % 5));
            if (rnd() % 4) R.add(rnd() % 6 ? LC_OK_T : LC_INFO, LC_SF_ADD, k, e, 0);
            a.push_back(e);
        } else if (what < 8) {
            R.add(LC_INVOKE, LC_SF_READ, k, LC_NIL, 5 + (int64_t)(rnd() % 3));
        } else {
            std::vector<int64_t> vals;
            for (int64_t e : a)
                if (rnd() % 5) vals.push_back(e);
            if (rnd() % 3 == 0 && !vals.empty()) vals.push_back(vals[rnd() % vals.size()]);
            if (rnd() % 7 == 0) vals.clear();
            R.add(LC_INVOKE, LC_SF_READ, k, LC_NIL, 9);
            R.add(LC_OK_T, LC_SF_READ, k, 0, 9, vals);
        }
        if (rnd() % 20 == 0) R.add(LC_INFO, LC_SF_OTHER, LC_NO_KEY, 0, LC_NO_PROCESS);
    }
    R.add(LC_OK_T, LC_SF_ADD, 12, 123456789, 0);  // no earlier :invoke :add: key 12 is an error key from here
    R.add(LC_INVOKE, LC_SF_ADD, 12, 5, 0);
    const size_t n = R.type.size();

    lc_setfull_stream *s = nullptr;
    lc_setfull_opts o{};
    o.linearizable = 1;
    REQUIRE(lc_setfull_stream_open(nullptr, &o, &s) == LC_OK && s);
    std::vector<int64_t> off;
    size_t at = 0, step = 1;
    bool refused = false;
    while (at < n) {
        const size_t e = std::min(n, at + step);
        lc_setfull_history h = R.slice(at, e, off);
        lc_setfull_stream_update u{};
        REQUIRE(lc_setfull_stream_append(s, &h, &u) == LC_OK);
        REQUIRE(u.rows == (int64_t)e && u.n_changed == 0);
        lc_setfull_stream_chunk c{};
        REQUIRE(lc_setfull_stream_last_chunk(s, &c) == LC_OK);
        // touch every array of the chunk
        uint64_t sum = 0;
        for (int64_t t = 0; t < c.n_touched; ++t) {
            sum += (uint64_t)c.tk_key[t] + c.tk_n_ids[t];
            for (uint64_t j = c.tk_blk_off[t]; j < c.tk_blk_off[t + 1]; ++j) sum += c.blk[j];
            for (uint64_t r = c.tk_row_off[t]; r < c.tk_row_off[t + 1]; ++r) {
                sum += (uint64_t)(c.row_pos[r] + c.row_time[r] + c.row_inv_pos[r] + c.row_inv_time[r]);
                for (uint64_t i = c.el_off[r]; i < c.el_off[r + 1]; ++i) {
                    REQUIRE(c.read_id[i] < c.tk_n_ids[t]);
                    sum += c.read_id[i];
                }
            }
        }
        for (int64_t i = 0; i < c.n_entries; ++i)
            sum += c.en_t[i] + c.en_id[i] + c.en_flags[i] + (uint64_t)(c.en_inv_pos[i] + c.en_ack_pos[i] + c.en_ack_time[i]);
        if (sum == 0x1234567) std::puts("");
        bool client = false;
        for (size_t q = at; q < e; ++q) client |= R.f[q] != LC_SF_OTHER;
        if (at >= 100 && client && !refused) {  // refused appends change nothing
            refused = true;
            std::vector<uint8_t> bad(R.type.begin() + (long)at, R.type.begin() + (long)e);
            lc_setfull_history hb = h;
            bad[0] = 7;
            hb.type = bad.data();
            REQUIRE(lc_setfull_stream_append(s, &hb, nullptr) == LC_E_INVALID);
            hb = h;
            hb.key = nullptr;
            REQUIRE(lc_setfull_stream_append(s, &hb, nullptr) == LC_E_INVALID);
            REQUIRE(lc_setfull_stream_keys(s, nullptr) == u.n_keys);
        }
        at = e;
        step = step % 37 + 3;
    }
    REQUIRE(refused);
    int64_t keys[8];
    REQUIRE(lc_setfull_stream_keys(s, keys) == 3);
    int n_bad = 0;
    for (int64_t i = 0; i < 3; ++i) {
        const int64_t ids = lc_setfull_stream_ids(s, i, nullptr, 0);
        REQUIRE(ids >= 0);
        std::vector<int64_t> el((size_t)ids + 1);
        std::vector<uint32_t> mult((size_t)ids + 1);
        REQUIRE(lc_setfull_stream_ids(s, i, el.data(), ids) == ids);
        REQUIRE(lc_setfull_stream_multiplicity(s, i, mult.data(), ids) == LC_OK);
        const char *err = lc_setfull_stream_key_error(s, i);
        n_bad += err != nullptr;
        REQUIRE((err != nullptr) == (keys[i] == 12) && (err == nullptr || ids == 0));
    }
    REQUIRE(n_bad == 1);
    REQUIRE(lc_setfull_stream_ids(s, 0, nullptr, 0) > 256 || lc_setfull_stream_ids(s, 1, nullptr, 0) > 256);  // a key past one block of ids
    double ms[6];
    REQUIRE(lc_setfull_stream_last_timing(s, ms) == LC_OK);
    lc_setfull_result r{};
    REQUIRE(lc_setfull_stream_results(s, &r) == LC_E_UNSUPPORTED);
    lc_setfull_stream_close(s);
    std::puts("ok");
    return 0;
}
