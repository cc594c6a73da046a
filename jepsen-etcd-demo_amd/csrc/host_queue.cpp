// host_queue.cpp -- checker/total-queue and checker/unique-ids on the host:
// lc_queue_pack (a raw history, lc_queue_history, to what lc_queue_check
// reads, lc_queue_batch) and lc_queue_check_host, the same fold as the
// device's in plain C++ on one thread (include/lincheck_queue.h has the rules;
// parity with Jepsen unpinned).  No HIP in this file.
//
// The pack is deliberately thin: independent/checker's split (key -> dense
// id), the drop and expansion rules of the drains, and nothing per value.
// Interning values here would be the whole check done on one thread.

#include <algorithm>
#include <cstring>
#include <numeric>
#include <string>
#include <unordered_map>
#include <vector>

#include "common.hpp"
#include "queue_plan.hpp"
#include "../../include/lincheck_queue.h"

struct lc_queue_packed {
    uint32_t mode = 0;
    std::vector<int64_t> keys;
    std::vector<uint8_t> status;
    std::vector<uint64_t> attempted;
    std::vector<std::string> error;
    lc::pinned_vector<uint32_t> row_key;
    lc::pinned_vector<uint8_t> row_kind;
    lc::pinned_vector<int64_t> row_val;
};

namespace lcq {

int queue_validate(const lc_queue_batch *b, const lc_queue_result *r, const char *who) {
    const int64_t K = b->n_keys, n = b->n_rows;
    if (K < 0 || K > 0x7FFFFFF0) return lc::fail(LC_E_INVALID, "%s: n_keys %lld", who, (long long)K);
    if (n < 0 || (uint64_t)n > QP_MAX_SLOTS) return lc::fail(LC_E_INVALID, "%s: n_rows %lld (at most 2^29)", who, (long long)n);
    if (b->mode > LC_QM_UNIQUE_IDS || b->reserved) return lc::fail(LC_E_INVALID, "%s: bad mode", who);
    if (n && (!b->row_key || !b->row_kind || !b->row_val)) return lc::fail(LC_E_INVALID, "%s: null row array", who);
    if (b->status)
        for (int64_t k = 0; k < K; ++k)
            if (b->status[k] > LC_QUEUE_KEY_ERROR) return lc::fail(LC_E_INVALID, "%s: key %lld: bad status code", who, (long long)k);
    if (K && (!r->valid || !r->counts || !r->lo || !r->hi || !r->has_range))
        return lc::fail(LC_E_INVALID, "%s: null result array", who);
    if (r->ent_cap && (!r->ent_key || !r->ent_class || !r->ent_val || !r->ent_mult))
        return lc::fail(LC_E_INVALID, "%s: null entry array", who);
    return LC_OK;
}

void queue_finish(const lc_queue_batch *b, lc_queue_result *r) {
    const bool ids = b->mode == LC_QM_UNIQUE_IDS;
    for (int64_t k = 0; k < b->n_keys; ++k) {
        uint64_t *c = r->counts + k * LC_QN_COUNTS;
        if (b->status && b->status[k] != LC_QUEUE_KEY_OK) {
            r->valid[k] = LC_UNKNOWN;
            r->has_range[k] = 0;
            continue;
        }
        if (ids) {
            c[LC_QN_ATTEMPT] = b->attempted ? b->attempted[k] : 0;
            r->valid[k] = c[LC_QN_OK] ? LC_INVALID : LC_VALID;
            r->has_range[k] = c[LC_QN_ACKNOWLEDGED] != 0;
        } else {
            r->valid[k] = c[LC_QN_LOST] || c[LC_QN_UNEXPECTED] ? LC_INVALID : LC_VALID;
            r->has_range[k] = 0;
        }
    }
}

void queue_sort_entries(lc_queue_result *r, uint64_t n, const uint32_t *key, const uint8_t *cls, const int64_t *val,
                        const unsigned long long *mult) {
    std::vector<uint64_t> at((size_t)n);
    std::iota(at.begin(), at.end(), (uint64_t)0);
    std::sort(at.begin(), at.end(), [&](uint64_t x, uint64_t y) {
        if (key[x] != key[y]) return key[x] < key[y];
        if (cls[x] != cls[y]) return cls[x] < cls[y];
        return val[x] < val[y];
    });
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t j = at[(size_t)i];
        r->ent_key[i] = key[j];
        r->ent_class[i] = cls[j];
        r->ent_val[i] = val[j];
        r->ent_mult[i] = mult[j];
    }
}

}  // namespace lcq

namespace {

const char *const CRASHED_DRAIN = "Not sure how to handle a crashed drain operation";

int pack(const lc_queue_history *h, uint32_t mode, lc_queue_packed &P) {
    const int64_t n = h->n;
    P.mode = mode;
    for (int64_t r = 0; r < n; ++r) {
        if (h->type[r] > LC_INFO || h->f[r] > LC_QF_OTHER)
            return lc::fail(LC_E_INVALID, "lc_queue_pack: row %lld: bad :type / :f code", (long long)r);
        if (h->drain_off && h->drain_off[r + 1] < h->drain_off[r])
            return lc::fail(LC_E_INVALID, "lc_queue_pack: row %lld: drain_off not ascending", (long long)r);
    }
    if (h->drain_off && n && h->drain_off[n] && !h->drain_val) return lc::fail(LC_E_INVALID, "lc_queue_pack: null drain_val");
    bool keyed = false;
    if (h->key)
        for (int64_t r = 0; r < n && !keyed; ++r) keyed = h->key[r] != LC_NO_KEY;
    std::unordered_map<int64_t, uint32_t> ids;
    if (!keyed) P.keys.push_back(LC_NO_KEY);
    // pass 1: every row's dense key id (NONE: ignored), the crashed drains, the row count
    constexpr uint32_t NONE = 0xFFFFFFFFu;
    std::vector<uint32_t> kid((size_t)n, 0u);
    std::vector<uint8_t> bad(keyed ? 0 : 1, 0);
    int64_t last = LC_NO_KEY;
    uint32_t last_i = NONE;
    for (int64_t r = 0; r < n; ++r) {
        if (!keyed) continue;
        const int64_t k = h->key[r];
        if (k != last) {
            last = k;
            if (k == LC_NO_KEY) {
                last_i = NONE;
            } else {
                auto it = ids.find(k);
                if (it == ids.end()) {
                    if (P.keys.size() >= 0x7FFFFFF0u) return lc::fail(LC_E_INVALID, "lc_queue_pack: more than 2^31 keys");
                    it = ids.emplace(k, (uint32_t)P.keys.size()).first;
                    P.keys.push_back(k);
                    bad.push_back(0);
                }
                last_i = it->second;
            }
        }
        kid[(size_t)r] = last_i;
    }
    const size_t K = P.keys.size();
    P.attempted.assign(K, 0);
    uint64_t rows = 0;
    for (int64_t r = 0; r < n; ++r) {
        const uint32_t k = kid[(size_t)r];
        if (k == NONE) continue;
        const uint8_t t = h->type[r], f = h->f[r];
        if (mode == LC_QM_UNIQUE_IDS) {
            if (f != LC_QF_GENERATE) continue;
            if (t == LC_INVOKE) ++P.attempted[k];
            else if (t == LC_OK_T) ++rows;
        } else if (f == LC_QF_DRAIN) {
            if (t == LC_INFO) bad[k] = 1;
            else if (t == LC_OK_T && h->drain_off) rows += h->drain_off[r + 1] - h->drain_off[r];
        } else if ((f == LC_QF_ENQUEUE && (t == LC_INVOKE || t == LC_OK_T)) || (f == LC_QF_DEQUEUE && t == LC_OK_T)) {
            ++rows;
        }
    }
    if (rows > lcq::QP_MAX_SLOTS) return lc::fail(LC_E_INVALID, "lc_queue_pack: %llu values (at most 2^29)", (unsigned long long)rows);
    P.status.assign(K, LC_QUEUE_KEY_OK);
    P.error.assign(K, std::string());
    for (size_t k = 0; k < K; ++k)
        if (bad[k]) {
            P.status[k] = LC_QUEUE_KEY_ERROR;
            P.error[k] = CRASHED_DRAIN;
        }
    // pass 2: the rows (an error key has none; its upper bound above only over-reserves)
    P.row_key.resize((size_t)rows); P.row_kind.resize((size_t)rows); P.row_val.resize((size_t)rows);
    uint64_t w = 0;
    auto put = [&](uint32_t k, uint8_t kind, int64_t v) {
        P.row_key[(size_t)w] = k; P.row_kind[(size_t)w] = kind; P.row_val[(size_t)w] = v;
        ++w;
    };
    for (int64_t r = 0; r < n; ++r) {
        const uint32_t k = kid[(size_t)r];
        if (k == NONE || bad[k]) continue;
        const uint8_t t = h->type[r], f = h->f[r];
        if (mode == LC_QM_UNIQUE_IDS) {
            if (f == LC_QF_GENERATE && t == LC_OK_T) put(k, LC_QK_ACK, h->value[r]);
        } else if (f == LC_QF_DRAIN) {
            if (t == LC_OK_T && h->drain_off)
                for (uint64_t i = h->drain_off[r]; i < h->drain_off[r + 1]; ++i) put(k, LC_QK_DEQUEUE, h->drain_val[i]);
        } else if (f == LC_QF_ENQUEUE) {
            if (t == LC_INVOKE) put(k, LC_QK_ATTEMPT, h->value[r]);
            else if (t == LC_OK_T) put(k, LC_QK_ACK, h->value[r]);
        } else if (f == LC_QF_DEQUEUE && t == LC_OK_T) {
            put(k, LC_QK_DEQUEUE, h->value[r]);
        }
    }
    P.row_key.resize((size_t)w); P.row_kind.resize((size_t)w); P.row_val.resize((size_t)w);
    return LC_OK;
}

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
struct Tally { uint64_t t[3] = {0, 0, 0}; };

int check_host(const lc_queue_batch *b, lc_queue_result *r) {
    const int64_t K = b->n_keys, n = b->n_rows;
    const bool ids = b->mode == LC_QM_UNIQUE_IDS;
    r->n_ent = 0;
    if (K) std::memset(r->counts, 0, (size_t)K * LC_QN_COUNTS * 8);
    std::unordered_map<Ident, Tally, IdentHash> tab;
    tab.reserve((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const uint32_t k = b->row_key[i];
        const uint8_t kind = b->row_kind[i];
        if ((int64_t)k >= K) return lc::fail(LC_E_INVALID, "lc_queue_check_host: row %lld: row_key %u of %lld keys", (long long)i, k, (long long)K);
        if (ids ? kind != LC_QK_ACK : kind > LC_QK_DEQUEUE)
            return lc::fail(LC_E_INVALID, "lc_queue_check_host: row %lld: bad row_kind %u", (long long)i, (unsigned)kind);
        if (b->status && b->status[k] != LC_QUEUE_KEY_OK) continue;
        ++tab[Ident{k, b->row_val[i]}].t[kind];
    }
    std::vector<uint32_t> ek;
    std::vector<uint8_t> ec;
    std::vector<int64_t> ev;
    std::vector<unsigned long long> em;
    auto entry = [&](uint32_t k, uint8_t c, int64_t v, uint64_t m) {
        if (!m) return;
        ek.push_back(k); ec.push_back(c); ev.push_back(v); em.push_back(m);
    };
    for (const auto &p : tab) {
        const uint32_t k = p.first.key;
        const int64_t v = p.first.val;
        const uint64_t at = p.second.t[0], en = p.second.t[1], de = p.second.t[2];
        uint64_t *c = r->counts + (size_t)k * LC_QN_COUNTS;
        if (ids) {
            c[LC_QN_ACKNOWLEDGED] += en;
            c[LC_QN_OK] += en > 1;
            if (c[LC_QN_ACKNOWLEDGED] == en) r->lo[k] = r->hi[k] = v;  // the key's first
            r->lo[k] = std::min(r->lo[k], v);
            r->hi[k] = std::max(r->hi[k], v);
            entry(k, LC_QC_DUPLICATED, v, en > 1 ? en : 0);
            continue;
        }
        const uint64_t ok = std::min(de, at);
        const uint64_t unexpected = at == 0 ? de : 0, duplicated = at > 0 && de > at ? de - at : 0;
        const uint64_t lost = en > de ? en - de : 0, recovered = ok > en ? ok - en : 0;
        c[LC_QN_ATTEMPT] += at; c[LC_QN_ACKNOWLEDGED] += en; c[LC_QN_OK] += ok; c[LC_QN_UNEXPECTED] += unexpected;
        c[LC_QN_DUPLICATED] += duplicated; c[LC_QN_LOST] += lost; c[LC_QN_RECOVERED] += recovered;
        entry(k, LC_QC_LOST, v, lost); entry(k, LC_QC_UNEXPECTED, v, unexpected);
        entry(k, LC_QC_DUPLICATED, v, duplicated); entry(k, LC_QC_RECOVERED, v, recovered);
    }
    lcq::queue_finish(b, r);
    r->n_ent = ek.size();
    if (r->n_ent > r->ent_cap)
        return lc::fail(LC_E_NOMEM, "lc_queue_check_host: ent_cap %llu, %llu needed", (unsigned long long)r->ent_cap,
                        (unsigned long long)r->n_ent);
    lcq::queue_sort_entries(r, r->n_ent, ek.data(), ec.data(), ev.data(), em.data());
    return LC_OK;
}

}  // namespace

extern "C" int lc_queue_pack(const lc_queue_history *h, uint32_t mode, lc_queue_packed **out) {
    lc::Range range("lc_queue_pack");
    if (!h || !out || h->n < 0) return lc::fail(LC_E_INVALID, "lc_queue_pack: null argument");
    if (mode > LC_QM_UNIQUE_IDS) return lc::fail(LC_E_INVALID, "lc_queue_pack: mode %u", mode);
    if (h->n > 0 && (!h->type || !h->f || !h->value)) return lc::fail(LC_E_INVALID, "lc_queue_pack: null column");
    try {
        auto *p = new lc_queue_packed();
        const int rc = pack(h, mode, *p);
        if (rc) { delete p; return rc; }
        *out = p;
        return LC_OK;
    } catch (const std::bad_alloc &) {
        return lc::fail(LC_E_NOMEM, "lc_queue_pack: out of memory");
    } catch (const std::exception &e) {
        return lc::fail(LC_E_NOMEM, "lc_queue_pack: %s", e.what());
    }
}

extern "C" void lc_queue_packed_free(lc_queue_packed *p) { delete p; }

extern "C" int lc_queue_packed_view(const lc_queue_packed *p, lc_queue_batch *out) {
    if (!p || !out) return lc::fail(LC_E_INVALID, "lc_queue_packed_view: null argument");
    out->n_keys = (int64_t)p->keys.size();
    out->n_rows = (int64_t)p->row_key.size();
    out->mode = p->mode; out->reserved = 0;
    out->row_key = p->row_key.data(); out->row_kind = p->row_kind.data(); out->row_val = p->row_val.data();
    out->status = p->status.data(); out->attempted = p->attempted.data();
    return LC_OK;
}

extern "C" int lc_queue_packed_keys(const lc_queue_packed *p, int64_t *out) {
    if (!p || !out) return lc::fail(LC_E_INVALID, "lc_queue_packed_keys: null argument");
    std::copy(p->keys.begin(), p->keys.end(), out);
    return LC_OK;
}

extern "C" const char *lc_queue_packed_key_error(const lc_queue_packed *p, int64_t i) {
    if (!p || i < 0 || (size_t)i >= p->keys.size() || p->status[(size_t)i] == LC_QUEUE_KEY_OK) return nullptr;
    return p->error[(size_t)i].c_str();
}

extern "C" int lc_queue_check_host(const lc_queue_batch *b, lc_queue_result *r) {
    if (!b || !r) return lc::fail(LC_E_INVALID, "lc_queue_check_host: null argument");
    if (int rc = lcq::queue_validate(b, r, "lc_queue_check_host")) return rc;
    try {
        return check_host(b, r);
    } catch (const std::bad_alloc &) {
        return lc::fail(LC_E_NOMEM, "lc_queue_check_host: out of memory");
    }
}

extern "C" int lc_queue_launch_info(int64_t *out4) {
    if (!out4) return lc::fail(LC_E_INVALID, "lc_queue_launch_info: null out");
    out4[0] = lcq::QP_BLOCK;
    out4[1] = lcq::QP_SLOTS_PER_ROW;
    out4[2] = lcq::QP_SLOT_BYTES;
    out4[3] = (int64_t)lcq::QP_MAX_BYTES;
    return LC_OK;
}
