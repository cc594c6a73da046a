// host_set.cpp -- lc_set_pack: a raw set-workload history (lc_set_history) to
// the per-key id arrays lc_set_check reads (lc_set_batch).  Stands behind
// jepsen.independent/checker's split and the three `into #{}` reductions of
// jepsen.checker/set (set.clj:46).
//
// Three passes over the rows, the two long ones split into contiguous row
// ranges over up to 16 threads (lc::run_threads):
//   1. keys in order of first appearance (serial: one hash lookup per change
//      of key);
//   2. per thread and key: add rows kept (:invoke / :ok), element minimum and
//      maximum, a nil or non-integer element, the last :ok :read.  Merged,
//      this gives each key's status, its id form (plan_set_key) and the layout;
//   3. per thread: the kept add rows scattered to their key's range, in
//      history order, as (id, class).
// The final read's ids and a rank key's sorted values are made per key
// between 2 and 3.

#include <algorithm>
#include <cstring>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "common.hpp"
#include "set_plan.hpp"

struct lc_set_packed {
    std::vector<int64_t> keys;
    lc::pinned_vector<uint32_t> add_id, read_id;
    lc::pinned_vector<uint8_t> add_cls;
    lc::pinned_vector<int64_t> vals;
    std::vector<uint64_t> add_off, read_off, base, vals_off;
    std::vector<uint32_t> span;
    std::vector<int64_t> mn;
    std::vector<uint8_t> rank, status;
    std::vector<std::string> error;
    uint64_t n_words = 0;
};

namespace {

struct ThreadAcc {
    std::vector<uint64_t> cnt;
    std::vector<int64_t> mn, mx, last_read;
    std::vector<uint8_t> any, bad;
    void init(size_t K) {
        cnt.assign(K, 0); mn.assign(K, 0); mx.assign(K, 0); last_read.assign(K, -1);
        any.assign(K, 0); bad.assign(K, 0);
    }
};

inline bool kept_add(const lc_set_history *h, int64_t r) {
    return h->f[r] == LC_SF_ADD && (h->type[r] == LC_INVOKE || h->type[r] == LC_OK_T);
}

int pack(const lc_set_history *h, lc_set_packed &P) {
    const int64_t n = h->n;
    for (int64_t r = 0; r < n; ++r)
        if (h->type[r] > LC_INFO || h->f[r] > LC_SF_OTHER)
            return lc::fail(LC_E_INVALID, "lc_set_pack: row %lld: bad :type / :f code", (long long)r);
    if (h->read_off) {
        if (h->read_off[0] < 0) return lc::fail(LC_E_INVALID, "lc_set_pack: read_off[0] < 0");
        for (int64_t r = 0; r < n; ++r)
            if (h->read_off[r + 1] < h->read_off[r])
                return lc::fail(LC_E_INVALID, "lc_set_pack: read_off not ascending at row %lld", (long long)r);
        if (h->read_off[n] > 0 && !h->read_elem) return lc::fail(LC_E_INVALID, "lc_set_pack: read_elem is null");
    }
    // 1. keys
    bool keyed = false;
    if (h->key)
        for (int64_t r = 0; r < n && !keyed; ++r) keyed = h->key[r] != LC_NO_KEY;
    std::vector<int32_t> kidx;  // keyed: the key index of each row, -1 for rows without a key
    if (keyed) {
        kidx.resize((size_t)n);
        std::unordered_map<int64_t, int32_t> ids;
        int64_t last = LC_NO_KEY;
        int32_t last_i = -1;
        for (int64_t r = 0; r < n; ++r) {
            const int64_t k = h->key[r];
            if (k != last) {
                last = k;
                if (k == LC_NO_KEY) {
                    last_i = -1;
                } else {
                    auto it = ids.find(k);
                    if (it == ids.end()) {
                        if (P.keys.size() >= 0x7FFFFFFFu) return lc::fail(LC_E_INVALID, "lc_set_pack: more than 2^31 keys");
                        it = ids.emplace(k, (int32_t)P.keys.size()).first;
                        P.keys.push_back(k);
                    }
                    last_i = it->second;
                }
            }
            kidx[(size_t)r] = last_i;
        }
    } else {
        P.keys.push_back(LC_NO_KEY);
    }
    const size_t K = P.keys.size();
    auto key_of = [&](int64_t r) -> int64_t { return keyed ? kidx[(size_t)r] : 0; };

    // 2. per thread and key
    unsigned T = (unsigned)std::min<int64_t>({16, (int64_t)std::max(1u, std::thread::hardware_concurrency()), n >> 16});
    if (T > 1 && (uint64_t)K * T > (1ull << 24)) T = (unsigned)std::max<uint64_t>(1, (1ull << 24) / K);
    T = std::max(1u, T);
    std::vector<ThreadAcc> acc(T);
    auto range = [&](unsigned t, int64_t &b, int64_t &e) { b = n * t / T; e = n * (t + 1) / T; };
    lc::run_threads(T, [&](unsigned t) {
        ThreadAcc &a = acc[t];
        a.init(K);
        int64_t b, e;
        range(t, b, e);
        for (int64_t r = b; r < e; ++r) {
            const int64_t k = key_of(r);
            if (k < 0) continue;
            if (kept_add(h, r)) {
                const int64_t v = h->elem[r];
                ++a.cnt[k];
                if (v == LC_NIL) { a.bad[k] = 1; continue; }
                if (!a.any[k]) { a.any[k] = 1; a.mn[k] = a.mx[k] = v; }
                else { a.mn[k] = std::min(a.mn[k], v); a.mx[k] = std::max(a.mx[k], v); }
            } else if (h->f[r] == LC_SF_READ && h->type[r] == LC_OK_T) {
                a.last_read[k] = r;
            }
        }
    });
    P.add_off.assign(K + 1, 0); P.read_off.assign(K + 1, 0); P.vals_off.assign(K + 1, 0);
    P.base.assign(K, 0); P.span.assign(K, 0); P.mn.assign(K, 0); P.rank.assign(K, 0); P.status.assign(K, 0);
    P.error.assign(K, std::string());
    std::vector<int64_t> final_read(K, -1);
    std::vector<uint64_t> n_add(K, 0);
    uint64_t add_total = 0, read_total = 0, words = 0;
    std::vector<size_t> rank_keys;
    for (size_t k = 0; k < K; ++k) {
        bool any = false, bad = false;
        int64_t mn = 0, mx = 0, last = -1;
        for (unsigned t = 0; t < T; ++t) {
            const ThreadAcc &a = acc[t];
            n_add[k] += a.cnt[k];
            bad |= a.bad[k] != 0;
            if (a.last_read[k] >= 0) last = a.last_read[k];
            if (a.any[k]) {
                mn = any ? std::min(mn, a.mn[k]) : a.mn[k];
                mx = any ? std::max(mx, a.mx[k]) : a.mx[k];
                any = true;
            }
        }
        uint64_t n_read = 0;
        if (last < 0 || h->elem[last] == LC_NIL) {
            // the reduce over the :ok :read values keeps the last one, nil included
            P.status[k] = LC_SET_KEY_NEVER_READ;
            P.error[k] = "Set was never read";
        } else {
            const int64_t rb = h->read_off ? h->read_off[last] : 0, re = h->read_off ? h->read_off[last + 1] : 0;
            for (int64_t i = rb; i < re; ++i) {
                const int64_t v = h->read_elem[i];
                if (v == LC_NIL) { bad = true; break; }
                mn = any ? std::min(mn, v) : v;
                mx = any ? std::max(mx, v) : v;
                any = true;
            }
            n_read = (uint64_t)(re - rb);
            if (bad) {
                P.status[k] = LC_SET_KEY_ERROR;
                P.error[k] = "a set element is nil or not an integer";
            }
        }
        if (P.status[k] == LC_SET_KEY_OK) {
            const lcs::SetKeyPlan kp = lcs::plan_set_key(any, mn, mx, n_add[k], n_read);
            if (!kp.rank && kp.span > lcs::SET_MAX_SPAN) {
                P.status[k] = LC_SET_KEY_ERROR;
                P.error[k] = "the key's elements span more than 2^32 ids";
            } else {
                final_read[k] = last;
                P.rank[k] = kp.rank;
                P.span[k] = (uint32_t)kp.span;
                P.mn[k] = any ? mn : 0;
                if (kp.rank) rank_keys.push_back(k);
            }
        }
        if (P.status[k] != LC_SET_KEY_OK) { n_add[k] = 0; n_read = 0; }
        P.add_off[k] = add_total;
        P.read_off[k] = read_total;
        add_total += n_add[k];
        read_total += n_read;
    }
    P.add_off[K] = add_total;
    P.read_off[K] = read_total;

    // a rank key's sorted distinct values (one more pass over the rows when there is such a key)
    std::vector<std::vector<int64_t>> kv(K);
    if (!rank_keys.empty()) {
        for (int64_t r = 0; r < n; ++r) {
            const int64_t k = key_of(r);
            if (k >= 0 && P.rank[k] && P.status[k] == LC_SET_KEY_OK && kept_add(h, r)) kv[k].push_back(h->elem[r]);
        }
        for (size_t k : rank_keys) {
            const int64_t last = final_read[k];
            if (h->read_off)
                for (int64_t i = h->read_off[last]; i < h->read_off[last + 1]; ++i) kv[k].push_back(h->read_elem[i]);
            std::sort(kv[k].begin(), kv[k].end());
            kv[k].erase(std::unique(kv[k].begin(), kv[k].end()), kv[k].end());
            if (kv[k].size() > lcs::SET_MAX_SPAN) return lc::fail(LC_E_INVALID, "lc_set_pack: a key has more than 2^32 distinct elements");
            P.span[k] = (uint32_t)kv[k].size();
        }
    }
    uint64_t vals_total = 0;
    for (size_t k = 0; k < K; ++k) {
        P.base[k] = words;
        if (P.status[k] == LC_SET_KEY_OK) words += lcs::set_words_padded(P.span[k]);
        P.vals_off[k] = vals_total;
        vals_total += kv[k].size();
    }
    P.vals_off[K] = vals_total;
    P.n_words = words;
    P.vals.resize(vals_total);
    for (size_t k : rank_keys) std::copy(kv[k].begin(), kv[k].end(), P.vals.begin() + (ptrdiff_t)P.vals_off[k]);

    auto id_of = [&](size_t k, int64_t v) -> uint32_t {
        if (!P.rank[k]) return (uint32_t)((uint64_t)v - (uint64_t)P.mn[k]);
        const int64_t *b = P.vals.data() + P.vals_off[k];
        return (uint32_t)(std::lower_bound(b, b + P.span[k], v) - b);
    };
    P.read_id.resize(read_total);
    for (size_t k = 0; k < K; ++k) {
        if (final_read[k] < 0) continue;
        uint64_t at = P.read_off[k];
        for (int64_t i = h->read_off ? h->read_off[final_read[k]] : 0; at < P.read_off[k + 1]; ++i) P.read_id[at++] = id_of(k, h->read_elem[i]);
    }

    // 3. scatter the kept add rows (each thread's cursor per key: where its range starts)
    P.add_id.resize(add_total);
    P.add_cls.resize(add_total);
    {
        std::vector<uint64_t> cur(K);
        for (size_t k = 0; k < K; ++k) cur[k] = P.add_off[k];
        for (unsigned t = 0; t < T; ++t)
            for (size_t k = 0; k < K; ++k) {
                const uint64_t c = acc[t].cnt[k];
                acc[t].cnt[k] = cur[k];
                cur[k] += P.status[k] == LC_SET_KEY_OK ? c : 0;
            }
    }
    lc::run_threads(T, [&](unsigned t) {
        std::vector<uint64_t> &cur = acc[t].cnt;
        int64_t b, e;
        range(t, b, e);
        for (int64_t r = b; r < e; ++r) {
            const int64_t k = key_of(r);
            if (k < 0 || P.status[k] != LC_SET_KEY_OK || !kept_add(h, r)) continue;
            const uint64_t at = cur[k]++;
            P.add_id[at] = id_of((size_t)k, h->elem[r]);
            P.add_cls[at] = h->type[r] == LC_INVOKE ? LC_SET_ATTEMPT : LC_SET_ACK;
        }
    });
    return LC_OK;
}

}  // namespace

extern "C" int lc_set_pack(const lc_set_history *h, lc_set_packed **out) {
    lc::Range range("lc_set_pack");
    if (!h || !out || h->n < 0) return lc::fail(LC_E_INVALID, "lc_set_pack: null argument");
    if (h->n > 0 && (!h->type || !h->f || !h->elem)) return lc::fail(LC_E_INVALID, "lc_set_pack: null column");
    try {
        auto *p = new lc_set_packed();
        const int rc = pack(h, *p);
        if (rc) { delete p; return rc; }
        *out = p;
        return LC_OK;
    } catch (const std::bad_alloc &) {
        return lc::fail(LC_E_NOMEM, "lc_set_pack: out of memory");
    } catch (const std::exception &e) {
        return lc::fail(LC_E_NOMEM, "lc_set_pack: %s", e.what());
    }
}

extern "C" void lc_set_packed_free(lc_set_packed *p) { delete p; }

extern "C" int lc_set_packed_view(const lc_set_packed *p, lc_set_batch *out) {
    if (!p || !out) return lc::fail(LC_E_INVALID, "lc_set_packed_view: null argument");
    out->n_keys = (int64_t)p->keys.size();
    out->add_off = p->add_off.data(); out->add_id = p->add_id.data(); out->add_cls = p->add_cls.data();
    out->read_off = p->read_off.data(); out->read_id = p->read_id.data();
    out->base = p->base.data(); out->span = p->span.data(); out->min = p->mn.data(); out->rank = p->rank.data();
    out->vals_off = p->vals_off.data(); out->vals = p->vals.data(); out->status = p->status.data();
    out->n_words = p->n_words;
    return LC_OK;
}

extern "C" int lc_set_packed_keys(const lc_set_packed *p, int64_t *out) {
    if (!p || !out) return lc::fail(LC_E_INVALID, "lc_set_packed_keys: null argument");
    std::copy(p->keys.begin(), p->keys.end(), out);
    return LC_OK;
}

extern "C" const char *lc_set_packed_key_error(const lc_set_packed *p, int64_t i) {
    if (!p || i < 0 || (size_t)i >= p->keys.size() || p->status[(size_t)i] == LC_SET_KEY_OK) return nullptr;
    return p->error[(size_t)i].c_str();
}

extern "C" int64_t lc_set_batch_max_runs(const lc_set_batch *b) {
    if (!b || b->n_keys < 0) return lc::fail(LC_E_INVALID, "lc_set_batch_max_runs: null argument");
    uint64_t total = 0;
    for (int64_t k = 0; k < b->n_keys; ++k) {
        if (b->status && b->status[k] != LC_SET_KEY_OK) continue;
        if (b->add_off[k + 1] < b->add_off[k] || b->read_off[k + 1] < b->read_off[k])
            return lc::fail(LC_E_INVALID, "lc_set_batch_max_runs: offsets of key %lld not ascending", (long long)k);
        for (uint64_t i = b->add_off[k]; i < b->add_off[k + 1]; ++i) total += b->add_cls[i] == LC_SET_ACK;
        total += 2 * (b->read_off[k + 1] - b->read_off[k]);
    }
    return (int64_t)total;
}

extern "C" int lc_set_launch_info(int64_t *out7) {
    if (!out7) return lc::fail(LC_E_INVALID, "lc_set_launch_info: null out");
    out7[0] = 64 * lcs::SET_LANE_WORDS;
    out7[1] = 64 * lcs::SET_WAVE_WORDS;
    out7[2] = 64 * lcs::SET_BLOCK_WORDS;
    out7[3] = lcs::SET_LDS_MAX_BITS;
    out7[4] = (int64_t)lcs::SET_OFFSET_FLOOR_BITS;
    out7[5] = lcs::SET_MARK_ROWS;
    out7[6] = 32 * lcs::SET_MARK_TILE_WORDS;
    return LC_OK;
}
