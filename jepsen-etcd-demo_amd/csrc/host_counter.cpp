// host_counter.cpp -- checker/counter on the host: lc_counter_pack (a raw
// counter history, lc_counter_history, to what lc_counter_check reads,
// lc_counter_batch) and lc_counter_check_host, the same fold as the device's
// in plain C++ on one thread (include/lincheck_counter.h has the rules;
// parity with Jepsen unpinned).  No HIP in this file.
//
// The pack stands behind jepsen.independent/checker's split and
// knossos.history/complete: one serial pass over the rows (pairing follows
// history order) that keeps per key an event list with only the rows that
// matter --
//   :invoke :add   an LC_CE_UP event; its value becomes the :ok's when one
//                  comes, and a :fail takes the event out again
//   :ok :add       an LC_CE_LOW event
//   :invoke :read  an LC_CE_RINV event, taken out again unless an :ok comes
//   :ok :read      an LC_CE_ROK event and the read's value
// -- then the value rules over what survived, and one copy into the batch's
// arrays, key after key, with the read events' indices made the batch's.

#include <algorithm>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "common.hpp"
#include "counter_plan.hpp"
#include "../../include/lincheck_counter.h"

struct lc_counter_packed {
    std::vector<int64_t> keys;
    std::vector<uint64_t> ev_off, read_off;
    std::vector<uint8_t> status;
    std::vector<std::string> error;
    lc::pinned_vector<uint8_t> ev_kind;
    lc::pinned_vector<int64_t> ev_val, read_val;
};

namespace lcc {

// The offset arrays and the status codes of a batch (a caller may have built it).
int counter_validate(const lc_counter_batch *b, const char *who) {
    const int64_t K = b->n_keys;
    if (K < 0 || K > 0x7FFFFFF0) return lc::fail(LC_E_INVALID, "%s: n_keys %lld", who, (long long)K);
    if (K == 0) return LC_OK;
    if (!b->ev_off || !b->read_off) return lc::fail(LC_E_INVALID, "%s: null offset array", who);
    if (b->ev_off[0] != 0 || b->read_off[0] != 0) return lc::fail(LC_E_INVALID, "%s: offsets do not start at 0", who);
    for (int64_t k = 0; k < K; ++k) {
        if (b->ev_off[k + 1] < b->ev_off[k] || b->read_off[k + 1] < b->read_off[k])
            return lc::fail(LC_E_INVALID, "%s: key %lld: offsets not ascending", who, (long long)k);
        const uint8_t st = b->status ? b->status[k] : (uint8_t)LC_COUNTER_KEY_OK;
        if (st > LC_COUNTER_KEY_ERROR) return lc::fail(LC_E_INVALID, "%s: key %lld: bad status code", who, (long long)k);
        if (st == LC_COUNTER_KEY_ERROR && (b->ev_off[k + 1] != b->ev_off[k] || b->read_off[k + 1] != b->read_off[k]))
            return lc::fail(LC_E_INVALID, "%s: key %lld: an error key with events or reads", who, (long long)k);
    }
    if (b->ev_off[K] && (!b->ev_kind || !b->ev_val)) return lc::fail(LC_E_INVALID, "%s: null event array", who);
    if (b->read_off[K] && !b->read_val) return lc::fail(LC_E_INVALID, "%s: null read_val", who);
    return LC_OK;
}

}  // namespace lcc

namespace {

constexpr uint8_t GONE = 0xFF;  // an event taken out again

struct Open {
    uint8_t f;
    uint64_t ev;  // its event in the key's list
};

struct KeyAcc {
    std::vector<uint8_t> kind;
    std::vector<int64_t> val, rval;
    std::unordered_map<int64_t, Open> open;  // process -> its open invocation
    bool bad = false;
    std::string error;
    void fail(const char *why) {
        if (!bad) error = why;
        bad = true;
    }
    uint64_t push(uint8_t k, int64_t v) {
        kind.push_back(k);
        val.push_back(v);
        return kind.size() - 1;
    }
};

void fold_row(KeyAcc &a, uint8_t t, uint8_t f, int64_t proc, int64_t v) {
    if (t == LC_INVOKE) {
        if (a.open.count(proc)) return a.fail("a second invocation by a process that has one open");
        a.open[proc] = Open{f, a.push(f == LC_CF_ADD ? LC_CE_UP : LC_CE_RINV, v)};
        return;
    }
    auto it = a.open.find(proc);
    if (it == a.open.end()) return a.fail("a completion by a process with no open invocation");
    const Open o = it->second;
    if (o.f != f) return a.fail("a completion whose :f is not its invocation's");
    a.open.erase(it);
    if (f == LC_CF_ADD) {
        if (t == LC_OK_T) {
            a.val[o.ev] = v;  // knossos.history/complete: the :ok's value is the invocation's
            a.push(LC_CE_LOW, v);
        } else if (t == LC_FAIL) {
            a.kind[o.ev] = GONE;
        }
    } else {
        if (t == LC_OK_T) {
            if (v == LC_NIL) return a.fail("an :ok :read whose value is nil or not an integer");
            a.val[o.ev] = (int64_t)a.rval.size();
            a.push(LC_CE_ROK, (int64_t)a.rval.size());
            a.rval.push_back(v);
        } else {
            a.kind[o.ev] = GONE;  // :fail removes it; after an :info no :ok can come: it yields nothing
        }
    }
}

// What survived: reads still open yield nothing; the adds' values and their sum.
void finish_key(KeyAcc &a) {
    for (const auto &p : a.open)
        if (p.second.f == LC_CF_READ) a.kind[p.second.ev] = GONE;
    a.open.clear();
    uint64_t up = 0;
    for (size_t e = 0; e < a.kind.size() && !a.bad; ++e) {
        if (a.kind[e] != LC_CE_UP && a.kind[e] != LC_CE_LOW) continue;
        const int64_t v = a.val[e];
        if (v == LC_NIL) a.fail("an :add whose value is nil or not an integer");
        else if (v < 0) a.fail("an :add of a negative value");
        else if (a.kind[e] == LC_CE_UP) {
            up += (uint64_t)v;
            if (up > (uint64_t)INT64_MAX) a.fail("the adds sum past the largest 64-bit integer");
        }
    }
}

int pack(const lc_counter_history *h, lc_counter_packed &P) {
    const int64_t n = h->n;
    for (int64_t r = 0; r < n; ++r)
        if (h->type[r] > LC_INFO || h->f[r] > LC_CF_OTHER)
            return lc::fail(LC_E_INVALID, "lc_counter_pack: row %lld: bad :type / :f code", (long long)r);
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
                        if (P.keys.size() >= 0x7FFFFFF0u) return lc::fail(LC_E_INVALID, "lc_counter_pack: more than 2^31 keys");
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
        if (a.bad || h->f[r] == LC_CF_OTHER) continue;
        const int64_t proc = h->process ? h->process[r] : 0;
        if (proc == LC_NO_PROCESS) continue;
        fold_row(a, h->type[r], h->f[r], proc, h->value[r]);
    }
    const size_t K = P.keys.size();
    P.ev_off.assign(K + 1, 0); P.read_off.assign(K + 1, 0);
    P.status.assign(K, LC_COUNTER_KEY_OK);
    P.error.assign(K, std::string());
    uint64_t E = 0, R = 0;
    for (size_t k = 0; k < K; ++k) {
        KeyAcc &a = acc[k];
        if (!a.bad) finish_key(a);
        P.ev_off[k] = E; P.read_off[k] = R;
        if (a.bad) {
            P.status[k] = LC_COUNTER_KEY_ERROR;
            P.error[k] = a.error;
            a.kind.clear(); a.val.clear(); a.rval.clear();
            continue;
        }
        E += (uint64_t)(a.kind.size() - (size_t)std::count(a.kind.begin(), a.kind.end(), GONE));
        R += a.rval.size();
    }
    P.ev_off[K] = E; P.read_off[K] = R;
    P.ev_kind.resize(E); P.ev_val.resize(E); P.read_val.resize(R);
    for (size_t k = 0; k < K; ++k) {
        const KeyAcc &a = acc[k];
        uint64_t e = P.ev_off[k];
        const int64_t r0 = (int64_t)P.read_off[k];
        for (size_t i = 0; i < a.kind.size(); ++i) {
            if (a.kind[i] == GONE) continue;
            P.ev_kind[e] = a.kind[i];
            P.ev_val[e] = a.kind[i] >= LC_CE_RINV ? r0 + a.val[i] : a.val[i];
            ++e;
        }
        if (!a.rval.empty()) std::copy(a.rval.begin(), a.rval.end(), P.read_val.begin() + (ptrdiff_t)r0);
    }
    return LC_OK;
}

}  // namespace

extern "C" int lc_counter_pack(const lc_counter_history *h, lc_counter_packed **out) {
    lc::Range range("lc_counter_pack");
    if (!h || !out || h->n < 0) return lc::fail(LC_E_INVALID, "lc_counter_pack: null argument");
    if (h->n > 0 && (!h->type || !h->f || !h->value)) return lc::fail(LC_E_INVALID, "lc_counter_pack: null column");
    try {
        auto *p = new lc_counter_packed();
        const int rc = pack(h, *p);
        if (rc) { delete p; return rc; }
        *out = p;
        return LC_OK;
    } catch (const std::bad_alloc &) {
        return lc::fail(LC_E_NOMEM, "lc_counter_pack: out of memory");
    } catch (const std::exception &e) {
        return lc::fail(LC_E_NOMEM, "lc_counter_pack: %s", e.what());
    }
}

extern "C" void lc_counter_packed_free(lc_counter_packed *p) { delete p; }

extern "C" int lc_counter_packed_view(const lc_counter_packed *p, lc_counter_batch *out) {
    if (!p || !out) return lc::fail(LC_E_INVALID, "lc_counter_packed_view: null argument");
    out->n_keys = (int64_t)p->keys.size();
    out->ev_off = p->ev_off.data(); out->ev_kind = p->ev_kind.data(); out->ev_val = p->ev_val.data();
    out->read_off = p->read_off.data(); out->read_val = p->read_val.data(); out->status = p->status.data();
    return LC_OK;
}

extern "C" int lc_counter_packed_keys(const lc_counter_packed *p, int64_t *out) {
    if (!p || !out) return lc::fail(LC_E_INVALID, "lc_counter_packed_keys: null argument");
    std::copy(p->keys.begin(), p->keys.end(), out);
    return LC_OK;
}

extern "C" const char *lc_counter_packed_key_error(const lc_counter_packed *p, int64_t i) {
    if (!p || i < 0 || (size_t)i >= p->keys.size() || p->status[(size_t)i] == LC_COUNTER_KEY_OK) return nullptr;
    return p->error[(size_t)i].c_str();
}

extern "C" int lc_counter_check_host(const lc_counter_batch *b, lc_counter_result *r) {
    if (!b || !r) return lc::fail(LC_E_INVALID, "lc_counter_check_host: null argument");
    if (int rc = lcc::counter_validate(b, "lc_counter_check_host")) return rc;
    const int64_t K = b->n_keys;
    r->n_err = 0;
    if (K == 0) return LC_OK;
    const uint64_t R = b->read_off[K];
    if (!r->valid || !r->n_errors || !r->err_off || (R && (!r->lower || !r->upper)) || (r->err_cap && !r->err_idx))
        return lc::fail(LC_E_INVALID, "lc_counter_check_host: null result array");
    if (R) {
        std::memset(r->lower, 0, R * 8);
        std::memset(r->upper, 0, R * 8);
    }
    uint64_t n_err = 0;
    for (int64_t k = 0; k < K; ++k) {
        r->err_off[k] = n_err;
        r->n_errors[k] = 0;
        if (b->status && b->status[k] != LC_COUNTER_KEY_OK) {
            r->valid[k] = LC_UNKNOWN;
            continue;
        }
        const uint64_t r0 = b->read_off[k], r1 = b->read_off[k + 1];
        uint64_t lower = 0, upper = 0;  // (unsigned: a caller-built batch's sums may wrap)
        for (uint64_t e = b->ev_off[k]; e < b->ev_off[k + 1]; ++e) {
            const uint64_t v = (uint64_t)b->ev_val[e];
            switch (b->ev_kind[e]) {
                case LC_CE_UP: upper += v; break;
                case LC_CE_LOW: lower += v; break;
                case LC_CE_RINV:
                case LC_CE_ROK:
                    if (v < r0 || v >= r1)
                        return lc::fail(LC_E_INVALID, "lc_counter_check_host: key %lld: a read event names a read that is not the key's",
                                        (long long)k);
                    if (b->ev_kind[e] == LC_CE_RINV) r->lower[v] = (int64_t)lower;
                    else r->upper[v] = (int64_t)upper;
                    break;
                default:
                    return lc::fail(LC_E_INVALID, "lc_counter_check_host: key %lld: bad event kind", (long long)k);
            }
        }
        for (uint64_t i = r0; i < r1; ++i) {
            const int64_t v = b->read_val[i];
            if (r->lower[i] <= v && v <= r->upper[i]) continue;
            if (n_err < r->err_cap) r->err_idx[n_err] = i;
            ++n_err;
        }
        r->n_errors[k] = n_err - r->err_off[k];
        r->valid[k] = r->n_errors[k] ? LC_INVALID : LC_VALID;
    }
    r->err_off[K] = n_err;
    r->n_err = n_err;
    if (n_err > r->err_cap) return lc::fail(LC_E_NOMEM, "lc_counter_check_host: err_cap %llu, %llu needed",
                                            (unsigned long long)r->err_cap, (unsigned long long)n_err);
    return LC_OK;
}

extern "C" int lc_counter_launch_info(int64_t *out4) {
    if (!out4) return lc::fail(LC_E_INVALID, "lc_counter_launch_info: null out");
    out4[0] = lcc::CT_BLOCK;
    out4[1] = lcc::CT_TILE_DEFAULT;
    out4[2] = lcc::CT_TILE_MIN;
    out4[3] = lcc::CT_CARRY_CHUNK;
    return LC_OK;
}
