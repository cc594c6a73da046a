// host_setfull.cpp -- lc_setfull_pack: a raw set-workload history with
// :process and :time (lc_setfull_history) to what lc_setfull_check reads
// (lc_setfull_batch).  Stands behind jepsen.independent/checker's split and
// the bookkeeping of jepsen.checker/set-full's fold that is not per (read,
// element): which :ok :read belongs to which invocation, which :invoke :add
// of an element is its last one and which :ok :add acknowledged it, and the
// error rules (include/lincheck.h has the semantics; parity unpinned).
//
// Two serial passes over the rows (the fold's state -- open reads by process,
// invoked elements -- follows history order):
//   1. keys in order of first appearance; per key the rows that count (kept
//      adds, :ok reads with their invocation), element minimum and maximum,
//      the first error;
//   2. per key: the id form (plan_set_key, as lc_set_pack), a rank key's
//      sorted values, then the per-id and per-row arrays.
// Every value of an :ok :read gets an id, invoked or not: the device flags
// duplicates per id, and a duplicate of an element nobody added counts.

#include <algorithm>
#include <cstring>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "common.hpp"
#include "set_plan.hpp"
#include "setfull_plan.hpp"

struct lc_setfull_packed {
    std::vector<int64_t> keys;
    std::vector<uint64_t> id_off, vals_off, row_off;
    std::vector<uint32_t> span;
    std::vector<int64_t> mn;
    std::vector<uint8_t> rank, status;
    std::vector<std::string> error;
    lc::pinned_vector<int64_t> vals, inv_pos, ack_pos, ack_time, row_pos, row_time, row_inv_pos, row_inv_time;
    lc::pinned_vector<uint64_t> el_off;
    lc::pinned_vector<uint32_t> read_id;
};

namespace {

struct KeyAcc {
    std::vector<int64_t> adds;                // rows of :invoke / :ok :add, in order
    std::vector<std::pair<int64_t, int64_t>> reads;  // (:ok :read row, its invocation's row), in order
    std::unordered_map<int64_t, int64_t> open;       // process -> its open :read invocation's row
    std::unordered_set<int64_t> invoked;
    bool any = false, bad = false;
    int64_t mn = 0, mx = 0;
    uint64_t n_read = 0;
    std::string error;
    void see(int64_t v) {
        if (!any) { any = true; mn = mx = v; }
        else { mn = std::min(mn, v); mx = std::max(mx, v); }
    }
    void fail(const char *why) {
        if (!bad) error = why;
        bad = true;
    }
};

int pack(const lc_setfull_history *h, lc_setfull_packed &P) {
    const int64_t n = h->n;
    for (int64_t r = 0; r < n; ++r)
        if (h->type[r] > LC_INFO || h->f[r] > LC_SF_OTHER)
            return lc::fail(LC_E_INVALID, "lc_setfull_pack: row %lld: bad :type / :f code", (long long)r);
    if (h->read_off) {
        if (h->read_off[0] < 0) return lc::fail(LC_E_INVALID, "lc_setfull_pack: read_off[0] < 0");
        for (int64_t r = 0; r < n; ++r)
            if (h->read_off[r + 1] < h->read_off[r])
                return lc::fail(LC_E_INVALID, "lc_setfull_pack: read_off not ascending at row %lld", (long long)r);
        if (h->read_off[n] > 0 && !h->read_elem) return lc::fail(LC_E_INVALID, "lc_setfull_pack: read_elem is null");
    }
    // 1. keys, and each key's fold bookkeeping
    bool keyed = false;
    if (h->key)
        for (int64_t r = 0; r < n && !keyed; ++r) keyed = h->key[r] != LC_NO_KEY;
    std::unordered_map<int64_t, int32_t> ids;
    std::vector<KeyAcc> acc;
    if (!keyed) {
        P.keys.push_back(LC_NO_KEY);
        acc.emplace_back();
    }
    int64_t last = LC_NO_KEY;
    int32_t last_i = -1;
    for (int64_t r = 0; r < n; ++r) {
        int32_t ki = 0;
        if (keyed) {
            const int64_t k = h->key[r];
            if (k != last) {
                last = k;
                if (k == LC_NO_KEY) {
                    last_i = -1;
                } else {
                    auto it = ids.find(k);
                    if (it == ids.end()) {
                        if (P.keys.size() >= 0x7FFFFFF0u) return lc::fail(LC_E_INVALID, "lc_setfull_pack: more than 2^31 keys");
                        it = ids.emplace(k, (int32_t)P.keys.size()).first;
                        P.keys.push_back(k);
                        acc.emplace_back();
                    }
                    last_i = it->second;
                }
            }
            ki = last_i;
            if (ki < 0) continue;
        }
        KeyAcc &a = acc[(size_t)ki];
        if (a.bad || h->f[r] == LC_SF_OTHER) continue;
        const int64_t proc = h->process ? h->process[r] : 0;
        if (proc == LC_NO_PROCESS) continue;
        const uint8_t t = h->type[r];
        if (h->f[r] == LC_SF_ADD) {
            if (t != LC_INVOKE && t != LC_OK_T) continue;
            const int64_t v = h->elem[r];
            if (v == LC_NIL) { a.fail("a set element is nil or not an integer"); continue; }
            if (t == LC_INVOKE) a.invoked.insert(v);
            else if (!a.invoked.count(v)) { a.fail("an :ok :add of an element with no earlier :invoke :add"); continue; }
            a.see(v);
            a.adds.push_back(r);
        } else if (t == LC_INVOKE) {
            a.open[proc] = r;
        } else if (t == LC_FAIL) {
            a.open.erase(proc);
        } else if (t == LC_OK_T) {
            auto it = a.open.find(proc);
            if (it == a.open.end()) { a.fail("an :ok :read by a process with no open :read invocation"); continue; }
            const int64_t rb = h->read_off ? h->read_off[r] : 0, re = h->read_off ? h->read_off[r + 1] : 0;
            bool nil = false;
            for (int64_t i = rb; i < re && !nil; ++i) {
                nil = h->read_elem[i] == LC_NIL;
                if (!nil) a.see(h->read_elem[i]);
            }
            if (nil) { a.fail("a :read value is no collection, or holds nil or a non-integer"); continue; }
            a.n_read += (uint64_t)(re - rb);
            a.reads.emplace_back(r, it->second);
        }
    }
    // 2. layout and arrays
    const size_t K = P.keys.size();
    P.id_off.assign(K + 1, 0); P.vals_off.assign(K + 1, 0); P.row_off.assign(K + 1, 0);
    P.span.assign(K, 0); P.mn.assign(K, 0); P.rank.assign(K, 0); P.status.assign(K, 0);
    P.error.assign(K, std::string());
    std::vector<std::vector<int64_t>> kv(K);
    uint64_t n_ids = 0, n_rows = 0, n_el = 0, n_vals = 0;
    for (size_t k = 0; k < K; ++k) {
        KeyAcc &a = acc[k];
        if (!a.bad) {
            const lcs::SetKeyPlan kp = lcs::plan_set_key(a.any, a.mn, a.mx, a.adds.size(), a.n_read);
            if (!kp.rank && kp.span > lcf::SF_MAX_SPAN) a.fail("the key's elements span more than 2^32 ids");
            else if (kp.rank) {
                std::vector<int64_t> &v = kv[k];
                for (int64_t r : a.adds) v.push_back(h->elem[r]);
                for (const auto &rd : a.reads)
                    for (int64_t i = h->read_off ? h->read_off[rd.first] : 0; h->read_off && i < h->read_off[rd.first + 1]; ++i)
                        v.push_back(h->read_elem[i]);
                std::sort(v.begin(), v.end());
                v.erase(std::unique(v.begin(), v.end()), v.end());
                if (v.size() > lcf::SF_MAX_SPAN) return lc::fail(LC_E_INVALID, "lc_setfull_pack: a key has more than 2^32 distinct elements");
                P.rank[k] = 1;
                P.span[k] = (uint32_t)v.size();
                P.mn[k] = a.mn;
            } else {
                P.span[k] = (uint32_t)kp.span;
                P.mn[k] = a.any ? a.mn : 0;
            }
        }
        if (a.bad) {
            P.status[k] = LC_SET_KEY_ERROR;
            P.error[k] = a.error;
            P.span[k] = 0; P.rank[k] = 0; P.mn[k] = 0;
            kv[k].clear();
            a.adds.clear(); a.reads.clear(); a.n_read = 0;
        }
        P.id_off[k] = n_ids; P.vals_off[k] = n_vals; P.row_off[k] = n_rows;
        n_ids += P.span[k]; n_vals += kv[k].size(); n_rows += a.reads.size(); n_el += a.n_read;
    }
    P.id_off[K] = n_ids; P.vals_off[K] = n_vals; P.row_off[K] = n_rows;
    P.vals.resize(n_vals);
    P.inv_pos.assign(n_ids, LC_SETFULL_NONE); P.ack_pos.assign(n_ids, LC_SETFULL_NONE); P.ack_time.assign(n_ids, 0);
    P.row_pos.resize(n_rows); P.row_time.resize(n_rows); P.row_inv_pos.resize(n_rows); P.row_inv_time.resize(n_rows);
    P.el_off.assign(n_rows + 1, 0);
    P.read_id.resize(n_el);
    auto time_of = [&](int64_t r) -> int64_t { return h->time ? h->time[r] : 0; };
    uint64_t el = 0;
    for (size_t k = 0; k < K; ++k) {
        const KeyAcc &a = acc[k];
        std::copy(kv[k].begin(), kv[k].end(), P.vals.begin() + (ptrdiff_t)P.vals_off[k]);
        const int64_t *vb = P.vals.data() + P.vals_off[k];
        const uint32_t span = P.span[k];
        const bool rank = P.rank[k] != 0;
        const int64_t mn = P.mn[k];
        auto id_of = [&](int64_t v) -> uint32_t {
            if (!rank) return (uint32_t)((uint64_t)v - (uint64_t)mn);
            return (uint32_t)(std::lower_bound(vb, vb + span, v) - vb);
        };
        for (int64_t r : a.adds) {
            const uint64_t g = P.id_off[k] + id_of(h->elem[r]);
            if (h->type[r] == LC_INVOKE) {
                P.inv_pos[g] = r;
                P.ack_pos[g] = LC_SETFULL_NONE;
                P.ack_time[g] = 0;
            } else if (P.ack_pos[g] == LC_SETFULL_NONE) {
                P.ack_pos[g] = r;
                P.ack_time[g] = time_of(r);
            }
        }
        uint64_t row = P.row_off[k];
        for (const auto &rd : a.reads) {
            P.row_pos[row] = rd.first; P.row_time[row] = time_of(rd.first);
            P.row_inv_pos[row] = rd.second; P.row_inv_time[row] = time_of(rd.second);
            P.el_off[row] = el;
            if (h->read_off)
                for (int64_t i = h->read_off[rd.first]; i < h->read_off[rd.first + 1]; ++i) P.read_id[el++] = id_of(h->read_elem[i]);
            ++row;
        }
    }
    P.el_off[n_rows] = el;
    return LC_OK;
}

}  // namespace

extern "C" int lc_setfull_pack(const lc_setfull_history *h, lc_setfull_packed **out) {
    lc::Range range("lc_setfull_pack");
    if (!h || !out || h->n < 0) return lc::fail(LC_E_INVALID, "lc_setfull_pack: null argument");
    if (h->n > 0 && (!h->type || !h->f || !h->elem)) return lc::fail(LC_E_INVALID, "lc_setfull_pack: null column");
    try {
        auto *p = new lc_setfull_packed();
        const int rc = pack(h, *p);
        if (rc) { delete p; return rc; }
        *out = p;
        return LC_OK;
    } catch (const std::bad_alloc &) {
        return lc::fail(LC_E_NOMEM, "lc_setfull_pack: out of memory");
    } catch (const std::exception &e) {
        return lc::fail(LC_E_NOMEM, "lc_setfull_pack: %s", e.what());
    }
}

extern "C" void lc_setfull_packed_free(lc_setfull_packed *p) { delete p; }

extern "C" int lc_setfull_packed_view(const lc_setfull_packed *p, lc_setfull_batch *out) {
    if (!p || !out) return lc::fail(LC_E_INVALID, "lc_setfull_packed_view: null argument");
    out->n_keys = (int64_t)p->keys.size();
    out->id_off = p->id_off.data(); out->span = p->span.data(); out->min = p->mn.data(); out->rank = p->rank.data();
    out->vals_off = p->vals_off.data(); out->vals = p->vals.data(); out->status = p->status.data();
    out->inv_pos = p->inv_pos.data(); out->ack_pos = p->ack_pos.data(); out->ack_time = p->ack_time.data();
    out->row_off = p->row_off.data(); out->row_pos = p->row_pos.data(); out->row_time = p->row_time.data();
    out->row_inv_pos = p->row_inv_pos.data(); out->row_inv_time = p->row_inv_time.data();
    out->el_off = p->el_off.data(); out->read_id = p->read_id.data();
    return LC_OK;
}

extern "C" int lc_setfull_packed_keys(const lc_setfull_packed *p, int64_t *out) {
    if (!p || !out) return lc::fail(LC_E_INVALID, "lc_setfull_packed_keys: null argument");
    std::copy(p->keys.begin(), p->keys.end(), out);
    return LC_OK;
}

extern "C" const char *lc_setfull_packed_key_error(const lc_setfull_packed *p, int64_t i) {
    if (!p || i < 0 || (size_t)i >= p->keys.size() || p->status[(size_t)i] == LC_SET_KEY_OK) return nullptr;
    return p->error[(size_t)i].c_str();
}

extern "C" int lc_setfull_launch_info(int64_t *out6) {
    if (!out6) return lc::fail(LC_E_INVALID, "lc_setfull_launch_info: null out");
    out6[0] = lcf::SF_WAVE_IDS;
    out6[1] = lcf::SF_BLOCK_IDS;
    out6[2] = lcf::SF_MARK_ELS;
    out6[3] = lcf::SF_MARK_LANE_ELS;
    out6[4] = 32 * lcf::SF_MARK_TILE_WORDS;
    out6[5] = (int64_t)lcf::SF_MATRIX_MAX_BYTES;
    return LC_OK;
}
