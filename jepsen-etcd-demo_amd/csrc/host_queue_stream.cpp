// host_queue_stream.cpp -- lc_queue_stream_*: the packer of a streaming
// total-queue / unique-ids, its entry points and the host stream's fold
// (include/lincheck_queue_stream.h has the contract).
// Single-threaded, as host_setfull_stream.cpp.
//
// The packer carries what of the two checkers is not per value: the key ids in
// order of first appearance, which keys a crashed drain has made :unknown, and
// unique-ids' :invoke rows per key.  Each append becomes one CHUNK: row_key,
// row_kind, row_val of the rows that count (lc_queue_pack's drop and expansion
// rules) and the list of the keys they touch.  An append is taken in three
// steps, so that a refused one leaves the stream as it was:
//   look     codes, columns, keyedness; then every row's key id (new keys get
//            theirs), the crashed drains, and the count of the rows to pack
//   decide   the size rule and the plan's grow rule (queue_stream_plan.hpp); a
//            refusal takes the new keys and :unknown marks back.  With a
//            device the table is grown here, the last step that may refuse
//   commit   the chunk's rows, the :invoke counts, then the fold: the device
//            half (device_queue_stream.hpp), or for a stream opened without a
//            context an incremental fold over lc_queue_check_host's
//            std::unordered_map, kept between appends: per row the class
//            vector of its value's tallies before and after, the difference
//            into the key's words.  It mirrors the plan's slot count too, so
//            that its updates equal a device stream's field for field.
// Per key the stream keeps QS_KEY_WORDS words in the device's format (seven
// counts, the range as two unsigned maxima); valid, lo, hi and has_range are
// derived from them.  No HIP here.

#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "common.hpp"
#include "device_queue_stream.hpp"
#include "queue_stream_plan.hpp"

namespace lcq {
// host_queue.cpp's (device_queue.hpp declares it beside HIP types, which this file stays clear of)
void queue_sort_entries(lc_queue_result *r, uint64_t n, const uint32_t *key, const uint8_t *cls, const int64_t *val,
                        const unsigned long long *mult);
}  // namespace lcq

namespace {

const char *const CRASHED_DRAIN = "Not sure how to handle a crashed drain operation";
constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr uint64_t SIGN = 1ull << 63;

struct Ident {
    uint32_t key;
    int64_t val;
    bool operator==(const Ident &o) const { return key == o.key && val == o.val; }
};
struct IdentHash {
    size_t operator()(const Ident &i) const {
        uint64_t x = (uint64_t)i.val ^ ((uint64_t)i.key * 0x9E3779B97F4A7C15ull);
        x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
        x ^= x >> 27;
        return (size_t)x;
    }
};
struct Tally { uint32_t t[3] = {0, 0, 0}; };

// The seven counts' share of one value with tallies t, and its multiplicity in the four listed classes.
void classes(uint32_t mode, const uint32_t *t, uint64_t *v, uint64_t *m) {
    const uint64_t at = t[LC_QK_ATTEMPT], en = t[LC_QK_ACK], de = t[LC_QK_DEQUEUE];
    for (int i = 0; i < LC_QN_COUNTS; ++i) v[i] = 0;
    m[0] = m[1] = m[2] = m[3] = 0;
    if (mode == LC_QM_UNIQUE_IDS) {
        v[LC_QN_ACKNOWLEDGED] = en;
        v[LC_QN_OK] = en > 1;
        m[LC_QC_DUPLICATED] = en > 1 ? en : 0;
        return;
    }
    const uint64_t ok = std::min(de, at);
    v[LC_QN_ATTEMPT] = at;
    v[LC_QN_ACKNOWLEDGED] = en;
    v[LC_QN_OK] = ok;
    v[LC_QN_UNEXPECTED] = m[LC_QC_UNEXPECTED] = at == 0 ? de : 0;
    v[LC_QN_DUPLICATED] = m[LC_QC_DUPLICATED] = at > 0 && de > at ? de - at : 0;
    v[LC_QN_LOST] = m[LC_QC_LOST] = en > de ? en - de : 0;
    v[LC_QN_RECOVERED] = m[LC_QC_RECOVERED] = ok > en ? ok - en : 0;
}

}  // namespace

struct lc_queue_stream {
    lc_ctx *ctx = nullptr;
    lcqs::QsDev *dev = nullptr;
    uint32_t mode = 0;
    int keyed = -1;       // -1: no row with a key or a queue :f yet
    bool broken = false;  // a device step failed half way: the table is not what the packer thinks
    int64_t rows = 0;
    uint64_t packed = 0, distinct = 0, slots = 0, appends = 0;
    std::vector<int64_t> keys;
    std::unordered_map<int64_t, uint32_t> ids;
    std::vector<uint8_t> status;
    std::vector<uint64_t> attempted;
    std::vector<uint64_t> words;   // [K][QS_KEY_WORDS]
    std::vector<int8_t> valid;
    std::vector<uint64_t> seen_in;  // per key: the append that last put it on `look`
    std::vector<int64_t> changed;
    // the current append
    std::vector<uint32_t> kid, look, new_bad, touched;
    std::vector<uint8_t> in_touched;
    lc::pinned_vector<uint32_t> row_key;
    lc::pinned_vector<uint8_t> row_kind;
    lc::pinned_vector<int64_t> row_val;
    std::vector<uint64_t> t_words;
    // the host stream's table
    std::unordered_map<Ident, Tally, IdentHash> tab;
    double ms[6] = {0, 0, 0, 0, 0, 0};
};

namespace {

using lcqs::QS_HI;
using lcqs::QS_KEY_WORDS;
using lcqs::QS_LO;

void add_key(lc_queue_stream *s, int64_t k) {
    s->ids.emplace(k, (uint32_t)s->keys.size());
    s->keys.push_back(k);
    s->status.push_back(LC_QUEUE_KEY_OK);
    s->attempted.push_back(0);
    s->words.insert(s->words.end(), QS_KEY_WORDS, 0);
    s->valid.push_back(LC_VALID);
    s->seen_in.push_back(0);
    s->in_touched.push_back(0);
}

void drop_keys_from(lc_queue_stream *s, size_t K0) {
    for (size_t k = K0; k < s->keys.size(); ++k) s->ids.erase(s->keys[k]);
    s->keys.resize(K0); s->status.resize(K0); s->attempted.resize(K0); s->words.resize(K0 * QS_KEY_WORDS);
    s->valid.resize(K0); s->seen_in.resize(K0); s->in_touched.resize(K0);
}

int8_t valid_of(const lc_queue_stream *s, size_t k) {
    if (s->status[k] != LC_QUEUE_KEY_OK) return LC_UNKNOWN;
    const uint64_t *c = s->words.data() + k * QS_KEY_WORDS;
    if (s->mode == LC_QM_UNIQUE_IDS) return c[LC_QN_OK] ? LC_INVALID : LC_VALID;
    return c[LC_QN_LOST] || c[LC_QN_UNEXPECTED] ? LC_INVALID : LC_VALID;
}

// Key k as lc_queue_result's arrays hold it.
void key_out(const lc_queue_stream *s, size_t k, int8_t *valid, uint64_t *counts, int64_t *lo, int64_t *hi, uint8_t *has) {
    const uint64_t *w = s->words.data() + k * QS_KEY_WORDS;
    const bool ok = s->status[k] == LC_QUEUE_KEY_OK, ids = s->mode == LC_QM_UNIQUE_IDS;
    valid[k] = s->valid[k];
    for (int i = 0; i < LC_QN_COUNTS; ++i) counts[k * LC_QN_COUNTS + i] = ok ? w[i] : 0;
    if (ok && ids) counts[k * LC_QN_COUNTS + LC_QN_ATTEMPT] = s->attempted[k];
    has[k] = ok && ids && w[LC_QN_ACKNOWLEDGED] != 0;
    if (has[k]) {
        lo[k] = (int64_t)(~w[QS_LO] ^ SIGN);
        hi[k] = (int64_t)(w[QS_HI] ^ SIGN);
    }
}

// Refusals that need no look at the keys: nothing of the stream has changed when one fires.
int refuse(const lc_queue_stream *s, const lc_queue_history *h, int *kind) {
    const int64_t n = h->n;
    if (n < 0) return lc::fail(LC_E_INVALID, "lc_queue_stream_append: n < 0");
    if (n > 0 && (!h->type || !h->f || !h->value)) return lc::fail(LC_E_INVALID, "lc_queue_stream_append: null column");
    bool client = false, has_key = false;
    for (int64_t r = 0; r < n; ++r) {
        if (h->type[r] > LC_INFO || h->f[r] > LC_QF_OTHER)
            return lc::fail(LC_E_INVALID, "lc_queue_stream_append: row %lld: bad :type / :f code", (long long)r);
        if (h->drain_off && h->drain_off[r + 1] < h->drain_off[r])
            return lc::fail(LC_E_INVALID, "lc_queue_stream_append: row %lld: drain_off not ascending", (long long)r);
        client |= h->f[r] != LC_QF_OTHER;
        has_key |= h->key && h->key[r] != LC_NO_KEY;
    }
    if (h->drain_off && n && h->drain_off[n] > h->drain_off[0] && !h->drain_val)
        return lc::fail(LC_E_INVALID, "lc_queue_stream_append: null drain_val");
    *kind = has_key ? 1 : client ? 0 : -1;
    if (*kind >= 0 && s->keyed >= 0 && *kind != s->keyed)
        return lc::fail(LC_E_INVALID, "lc_queue_stream_append: %s rows appended to a stream of %s rows", *kind ? "keyed" : "unkeyed",
                        s->keyed ? "keyed" : "unkeyed");
    return LC_OK;
}

// What row r packs to: calls put(kind, value) once per value that counts.
template <class F>
inline void pack_row(const lc_queue_history *h, uint32_t mode, int64_t r, F &&put) {
    const uint8_t t = h->type[r], f = h->f[r];
    if (mode == LC_QM_UNIQUE_IDS) {
        if (f == LC_QF_GENERATE && t == LC_OK_T) put(LC_QK_ACK, h->value[r]);
    } else if (f == LC_QF_DRAIN) {
        if (t == LC_OK_T && h->drain_off)
            for (uint64_t i = h->drain_off[r]; i < h->drain_off[r + 1]; ++i) put(LC_QK_DEQUEUE, h->drain_val[i]);
    } else if (f == LC_QF_ENQUEUE) {
        if (t == LC_INVOKE) put(LC_QK_ATTEMPT, h->value[r]);
        else if (t == LC_OK_T) put(LC_QK_ACK, h->value[r]);
    } else if (f == LC_QF_DEQUEUE && t == LC_OK_T) {
        put(LC_QK_DEQUEUE, h->value[r]);
    }
}

// The host stream's fold of the chunk; the touched keys' words are updated in place.
void fold_host(lc_queue_stream *s) {
    const size_t n = s->row_key.size();
    uint64_t a[LC_QN_COUNTS], b[LC_QN_COUNTS], m[4];
    for (size_t i = 0; i < n; ++i) {
        const uint32_t k = s->row_key[i];
        const uint8_t kind = s->row_kind[i];
        const int64_t v = s->row_val[i];
        Tally &t = s->tab[Ident{k, v}];
        uint64_t *w = s->words.data() + (size_t)k * QS_KEY_WORDS;
        classes(s->mode, t.t, b, m);
        ++t.t[kind];
        classes(s->mode, t.t, a, m);
        for (int j = 0; j < LC_QN_COUNTS; ++j) w[j] += a[j] - b[j];
        if (s->mode == LC_QM_UNIQUE_IDS) {
            const uint64_t u = (uint64_t)v ^ SIGN;
            w[QS_LO] = std::max(w[QS_LO], ~u);
            w[QS_HI] = std::max(w[QS_HI], u);
        }
    }
    s->distinct = s->tab.size();
}

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

int append(lc_queue_stream *s, const lc_queue_history *h, lc_queue_stream_update *u) {
    const auto t0 = std::chrono::steady_clock::now();
    if (s->broken) return lc::fail(LC_E_INVALID, "lc_queue_stream_append: an earlier append failed on the device; close the stream");
    int kind = -1;
    if (int rc = refuse(s, h, &kind)) return rc;
    const int64_t n = h->n;
    const bool tq = s->mode == LC_QM_TOTAL_QUEUE;

    // ---- look
    const int keyed0 = s->keyed;
    size_t K0 = s->keys.size();
    const bool decides_keyed = s->keyed < 0 && kind == 1;
    if (decides_keyed) drop_keys_from(s, 0);  // the placeholder LC_NO_KEY, which nothing has touched
    if (s->keyed < 0) s->keyed = kind;
    if (decides_keyed) K0 = 0;
    auto take_back = [&]() {
        for (uint32_t k : s->new_bad) s->status[k] = LC_QUEUE_KEY_OK;
        drop_keys_from(s, K0);
        s->keyed = keyed0;
        if (decides_keyed) add_key(s, LC_NO_KEY);
    };
    ++s->appends;  // (a stamp only: a refused append keeps its number)
    s->new_bad.clear();
    s->look.clear();
    s->kid.assign((size_t)n, 0u);
    const bool keyed = s->keyed == 1;
    if (keyed) {
        int64_t last = LC_NO_KEY;
        uint32_t last_i = NONE;
        for (int64_t r = 0; r < n; ++r) {
            const int64_t k = h->key ? h->key[r] : LC_NO_KEY;
            if (k != last) {
                last = k;
                if (k == LC_NO_KEY) {
                    last_i = NONE;
                } else {
                    auto it = s->ids.find(k);
                    if (it == s->ids.end()) {
                        if (s->keys.size() >= 0x7FFFFFF0u) {
                            take_back();
                            return lc::fail(LC_E_INVALID, "lc_queue_stream_append: more than 2^31 keys");
                        }
                        last_i = (uint32_t)s->keys.size();
                        add_key(s, k);
                    } else {
                        last_i = it->second;
                    }
                    if (s->seen_in[last_i] != s->appends) {
                        s->seen_in[last_i] = s->appends;
                        s->look.push_back(last_i);
                    }
                }
            }
            s->kid[(size_t)r] = last_i;
        }
    } else if (n) {
        s->look.push_back(0);
    }
    if (tq)
        for (int64_t r = 0; r < n; ++r) {
            const uint32_t k = s->kid[(size_t)r];
            if (k != NONE && h->f[r] == LC_QF_DRAIN && h->type[r] == LC_INFO && s->status[k] == LC_QUEUE_KEY_OK) {
                s->status[k] = LC_QUEUE_KEY_ERROR;
                s->new_bad.push_back(k);
            }
        }
    uint64_t n_pack = 0;
    for (int64_t r = 0; r < n; ++r) {
        const uint32_t k = s->kid[(size_t)r];
        if (k == NONE || s->status[k] != LC_QUEUE_KEY_OK) continue;
        pack_row(h, s->mode, r, [&](uint8_t, int64_t) { ++n_pack; });
    }

    // ---- decide
    if (s->packed + n_pack > lcqs::QSP_MAX_ROWS) {
        take_back();
        return lc::fail(LC_E_UNSUPPORTED, "lc_queue_stream_append: %llu values after %llu: a stream's stay below 2^32",
                        (unsigned long long)n_pack, (unsigned long long)s->packed);
    }
    bool grew = false;
    double grow_ms = 0;
    if (lcqs::qsp_must_grow(s->slots, s->distinct, n_pack)) {
        const uint64_t to = lcqs::qsp_grown_slots(s->distinct, n_pack);
        if (to == lcqs::QSP_BAD_SLOTS) {
            take_back();
            return lc::fail(LC_E_NOMEM, "lc_queue_stream_append: %llu values beside %llu resident need more than the table's cap of %llu bytes",
                            (unsigned long long)n_pack, (unsigned long long)s->distinct, (unsigned long long)lcqs::QSP_MAX_BYTES);
        }
        if (to > s->slots) {
            if (s->dev)
                if (int rc = lcqs::qs_dev_grow(s->dev, to, &grow_ms)) {
                    if (rc == LC_E_NOMEM) take_back();
                    else s->broken = true;
                    return rc;
                }
            s->slots = to;
            grew = true;
        }
    }

    // ---- commit
    s->row_key.resize((size_t)n_pack); s->row_kind.resize((size_t)n_pack); s->row_val.resize((size_t)n_pack);
    s->touched.clear();
    size_t w = 0;
    for (int64_t r = 0; r < n; ++r) {
        const uint32_t k = s->kid[(size_t)r];
        if (k == NONE || s->status[k] != LC_QUEUE_KEY_OK) continue;
        if (!tq && h->f[r] == LC_QF_GENERATE && h->type[r] == LC_INVOKE) ++s->attempted[k];
        const size_t w0 = w;
        pack_row(h, s->mode, r, [&](uint8_t kd, int64_t v) {
            s->row_key[w] = k; s->row_kind[w] = kd; s->row_val[w] = v;
            ++w;
        });
        if (w != w0 && !s->in_touched[k]) {
            s->in_touched[k] = 1;
            s->touched.push_back(k);
        }
    }
    for (uint32_t k : s->touched) s->in_touched[k] = 0;
    s->rows += n;
    s->packed += n_pack;
    std::fill(s->ms, s->ms + 6, 0.0);
    s->ms[0] = ms_since(t0);
    s->ms[4] = grow_ms;
    if (s->dev) {
        if (n_pack) {
            lcqs::QsChunk c;
            c.n_rows = n_pack; c.row_key = s->row_key.data(); c.row_kind = s->row_kind.data(); c.row_val = s->row_val.data();
            c.n_touched = s->touched.size(); c.touched = s->touched.data(); c.n_keys = s->keys.size();
            s->t_words.assign(s->touched.size() * QS_KEY_WORDS, 0);
            if (int rc = lcqs::qs_dev_append(s->dev, &c, s->t_words.data(), &s->distinct, s->ms + 1)) {
                s->broken = true;
                return rc;
            }
            for (size_t t = 0; t < s->touched.size(); ++t)
                std::copy_n(s->t_words.begin() + t * QS_KEY_WORDS, (size_t)QS_KEY_WORDS, s->words.begin() + (size_t)s->touched[t] * QS_KEY_WORDS);
        }
    } else {
        const auto t1 = std::chrono::steady_clock::now();
        fold_host(s);
        s->ms[2] = ms_since(t1);
    }
    // valid: every key this append has looked at (touched, made :unknown or new)
    s->changed.clear();
    for (uint32_t k : s->look) {
        const int8_t v = valid_of(s, k);
        if (v != s->valid[k]) s->changed.push_back((int64_t)k);
        s->valid[k] = v;
    }
    std::sort(s->changed.begin(), s->changed.end());
    s->ms[5] = ms_since(t0);
    if (u) {
        u->n_keys = (int64_t)s->keys.size();
        u->rows = s->rows;
        u->packed = (int64_t)n_pack;
        u->distinct = (int64_t)s->distinct;
        u->slots = (int64_t)s->slots;
        u->grew = grew;
        u->n_changed = (int64_t)s->changed.size();
        u->changed = s->changed.data();
    }
    return LC_OK;
}

int results(lc_queue_stream *s, lc_queue_result *r) {
    const size_t K = s->keys.size();
    if (!r->valid || !r->counts || !r->lo || !r->hi || !r->has_range)
        return lc::fail(LC_E_INVALID, "lc_queue_stream_results: null result array");
    if (r->ent_cap && (!r->ent_key || !r->ent_class || !r->ent_val || !r->ent_mult))
        return lc::fail(LC_E_INVALID, "lc_queue_stream_results: null entry array");
    for (size_t k = 0; k < K; ++k) key_out(s, k, r->valid, r->counts, r->lo, r->hi, r->has_range);
    r->n_ent = 0;
    std::vector<uint32_t> ek;
    std::vector<uint8_t> ec;
    std::vector<int64_t> ev;
    std::vector<unsigned long long> em;
    uint64_t n_ent = 0;
    if (s->dev) {
        if (s->distinct == 0) return LC_OK;
        const uint64_t cap = std::min<uint64_t>(r->ent_cap, 2 * s->distinct);  // (a distinct value makes at most two entries)
        const size_t m = (size_t)std::max<uint64_t>(cap, 1);
        ek.resize(m); ec.resize(m); ev.resize(m); em.resize(m);
        static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "entry multiplicities");
        if (int rc = lcqs::qs_dev_entries(s->dev, s->status.data(), K, cap, ek.data(), ec.data(), ev.data(), (uint64_t *)em.data(), &n_ent))
            return rc;
    } else {
        uint64_t v[LC_QN_COUNTS], m[4];
        for (const auto &p : s->tab) {
            if (s->status[p.first.key] != LC_QUEUE_KEY_OK) continue;
            classes(s->mode, p.second.t, v, m);
            for (int c = 0; c < 4; ++c)
                if (m[c]) {
                    ek.push_back(p.first.key); ec.push_back((uint8_t)c); ev.push_back(p.first.val); em.push_back(m[c]);
                }
        }
        n_ent = ek.size();
    }
    r->n_ent = n_ent;
    if (n_ent > r->ent_cap)
        return lc::fail(LC_E_NOMEM, "lc_queue_stream_results: ent_cap %llu, %llu needed", (unsigned long long)r->ent_cap,
                        (unsigned long long)n_ent);
    lcq::queue_sort_entries(r, n_ent, ek.data(), ec.data(), ev.data(), em.data());
    return LC_OK;
}

template <class F>
int guarded(const char *who, F &&f) {
    try {
        return f();
    } catch (const std::bad_alloc &) {
        return lc::fail(LC_E_NOMEM, "%s: out of memory", who);
    } catch (const std::exception &e) {
        return lc::fail(LC_E_NOMEM, "%s: %s", who, e.what());
    }
}

}  // namespace

extern "C" int lc_queue_stream_open(lc_ctx *ctx, uint32_t mode, const lc_queue_stream_opts *o, lc_queue_stream **out) {
    if (!out) return lc::fail(LC_E_INVALID, "lc_queue_stream_open: null out");
    *out = nullptr;
    if (mode > LC_QM_UNIQUE_IDS) return lc::fail(LC_E_INVALID, "lc_queue_stream_open: mode %u", mode);
    if (o && o->flags) return lc::fail(LC_E_INVALID, "lc_queue_stream_open: unknown flags 0x%x", o->flags);
    const uint64_t slots = lcqs::qsp_first_slots(o ? o->slots : 0);
    if (slots == lcqs::QSP_BAD_SLOTS)
        return lc::fail(LC_E_INVALID, "lc_queue_stream_open: slots %u (a power of two, at most 2^27)", o->slots);
    return guarded("lc_queue_stream_open", [&]() -> int {
        lc_queue_stream *s = new lc_queue_stream;
        s->ctx = ctx;
        s->mode = mode;
        s->slots = slots;
        add_key(s, LC_NO_KEY);
        if (ctx) {
            int rc = lcqs::qs_dev_open ? lcqs::qs_dev_open(ctx, mode, &s->dev)
                                       : lc::fail(LC_E_UNSUPPORTED, "lc_queue_stream_open: this build has no device half");
            double ms = 0;
            if (!rc) rc = lcqs::qs_dev_grow(s->dev, slots, &ms);
            if (rc) {
                if (s->dev) lcqs::qs_dev_close(s->dev);
                delete s;
                return rc;
            }
        }
        *out = s;
        return LC_OK;
    });
}

extern "C" void lc_queue_stream_close(lc_queue_stream *s) {
    if (!s) return;
    if (s->dev) lcqs::qs_dev_close(s->dev);
    delete s;
}

extern "C" int lc_queue_stream_append(lc_queue_stream *s, const lc_queue_history *rows, lc_queue_stream_update *u) {
    lc::Range range("lc_queue_stream_append");
    if (!s || !rows) return lc::fail(LC_E_INVALID, "lc_queue_stream_append: null argument");
    return guarded("lc_queue_stream_append", [&]() -> int { return append(s, rows, u); });
}

extern "C" int lc_queue_stream_counts(lc_queue_stream *s, int8_t *valid, uint64_t *counts, int64_t *lo, int64_t *hi, uint8_t *has_range) {
    if (!s || !valid || !counts || !lo || !hi || !has_range) return lc::fail(LC_E_INVALID, "lc_queue_stream_counts: null argument");
    for (size_t k = 0; k < s->keys.size(); ++k) key_out(s, k, valid, counts, lo, hi, has_range);
    return LC_OK;
}

extern "C" int lc_queue_stream_results(lc_queue_stream *s, lc_queue_result *r) {
    if (!s || !r) return lc::fail(LC_E_INVALID, "lc_queue_stream_results: null argument");
    if (s->broken) return lc::fail(LC_E_INVALID, "lc_queue_stream_results: an earlier append failed on the device");
    return guarded("lc_queue_stream_results", [&]() -> int { return results(s, r); });
}

extern "C" int64_t lc_queue_stream_keys(const lc_queue_stream *s, int64_t *out) {
    if (!s) return lc::fail(LC_E_INVALID, "lc_queue_stream_keys: null stream");
    if (out) std::copy(s->keys.begin(), s->keys.end(), out);
    return (int64_t)s->keys.size();
}

extern "C" const char *lc_queue_stream_key_error(const lc_queue_stream *s, int64_t i) {
    if (!s || i < 0 || (size_t)i >= s->keys.size() || s->status[(size_t)i] == LC_QUEUE_KEY_OK) return nullptr;
    return CRASHED_DRAIN;
}

extern "C" int lc_queue_stream_last_timing(const lc_queue_stream *s, double *out6) {
    if (!s || !out6) return lc::fail(LC_E_INVALID, "lc_queue_stream_last_timing: null argument");
    std::copy(s->ms, s->ms + 6, out6);
    return LC_OK;
}

extern "C" int lc_queue_stream_launch_info(int64_t *out6) {
    if (!out6) return lc::fail(LC_E_INVALID, "lc_queue_stream_launch_info: null out");
    out6[0] = lcqs::QSP_BLOCK;
    out6[1] = lcqs::QSP_SLOTS_PER_VALUE;
    out6[2] = lcqs::QSP_SLOT_BYTES;
    out6[3] = (int64_t)lcqs::QSP_MAX_BYTES;
    out6[4] = (int64_t)lcqs::QSP_DEFAULT_SLOTS;
    out6[5] = (int64_t)lcqs::QSP_LAUNCH_ROWS;
    return LC_OK;
}
