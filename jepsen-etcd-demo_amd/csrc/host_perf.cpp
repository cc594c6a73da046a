// host_perf.cpp -- lc_perf_pack: a whole history (lc_perf_history) to the
// completion records lc_perf_check reads (lc_perf_batch), and the nemesis
// intervals.  Stands behind jepsen.util/history->latencies and
// nemesis-intervals.
//
// One pass over the rows, in history order:
//   a client :invoke becomes its process's pending invocation (an earlier
//     pending one is then unmatched);
//   a client :ok / :fail / :info is one record: it completes and clears the
//     pending invocation of its process, or is an orphan;
//   among the other rows, :start opens an interval if none is open and the
//     next :stop closes it; one still open at the end runs to the largest time.
// Processes are looked up in a flat table while they are small non-negative
// integers (Jepsen's are), else in a hash map.

#include <algorithm>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "common.hpp"
#include "perf_plan.hpp"

struct lc_perf_packed {
    lc::pinned_vector<int64_t> t_comp, t_inv;
    lc::pinned_vector<uint32_t> meta;
    std::vector<int64_t> intervals;  // (t0, t1) pairs
    int64_t matched = 0, unmatched = 0, orphans = 0;
    int64_t t_min = 0, t_max = 0, x_min = 0, x_max = 0;
    int32_t n_f = 0;
};

namespace {

constexpr int64_t FLAT_PROCESSES = 1 << 16;

int pack(const lc_perf_history *h, lc_perf_packed &P) {
    const int64_t n = h->n;
    if (h->n_f < 0 || h->n_f > 256) return lc::fail(LC_E_INVALID, "lc_perf_pack: n_f %d", h->n_f);
    if (h->n_f > LC_PERF_MAX_F)
        return lc::fail(LC_E_UNSUPPORTED, "lc_perf_pack: %d distinct :f, at most %d are supported", h->n_f, LC_PERF_MAX_F);
    int64_t clients = 0;
    for (int64_t r = 0; r < n; ++r) {
        if (h->type[r] > LC_INFO) return lc::fail(LC_E_INVALID, "lc_perf_pack: row %lld: bad :type code", (long long)r);
        if ((int32_t)h->f[r] >= h->n_f) return lc::fail(LC_E_INVALID, "lc_perf_pack: row %lld: f %u is not below n_f %d", (long long)r, h->f[r], h->n_f);
        clients += h->process[r] != LC_NO_PROCESS && h->type[r] != LC_INVOKE;
    }
    P.n_f = h->n_f;
    P.t_comp.reserve((size_t)clients);
    P.t_inv.reserve((size_t)clients);
    P.meta.reserve((size_t)clients);
    // pending invocation (a row) of each process, -1 for none
    std::vector<int64_t> flat;
    std::unordered_map<int64_t, int64_t> sparse;
    auto pending = [&](int64_t p) -> int64_t & {
        if (p >= 0 && p < FLAT_PROCESSES) {
            if ((size_t)p >= flat.size()) flat.resize((size_t)p + 1, -1);
            return flat[(size_t)p];
        }
        return sparse.emplace(p, -1).first->second;
    };
    bool any_t = false, any_x = false, open = false;
    int64_t open_t = 0, hist_max = 0;
    for (int64_t r = 0; r < n; ++r) {
        const int64_t t = h->time[r], p = h->process[r];
        hist_max = r == 0 ? t : std::max(hist_max, t);
        if (p == LC_NO_PROCESS) {
            if ((int32_t)h->f[r] == h->f_start && !open) {
                open = true;
                open_t = t;
            } else if ((int32_t)h->f[r] == h->f_stop && open) {
                open = false;
                P.intervals.push_back(open_t);
                P.intervals.push_back(t);
            }
            continue;
        }
        int64_t &pend = pending(p);
        if (h->type[r] == LC_INVOKE) {
            if (pend >= 0) ++P.unmatched;
            pend = r;
            continue;
        }
        uint32_t f_inv = h->f[r];
        int64_t t_inv = LC_PERF_NO_INVOKE;
        if (pend >= 0) {
            f_inv = h->f[pend];
            t_inv = h->time[pend];
            if (t_inv == LC_PERF_NO_INVOKE)
                return lc::fail(LC_E_INVALID, "lc_perf_pack: row %lld: :time INT64_MIN is reserved", (long long)pend);
            pend = -1;
            ++P.matched;
            P.x_min = any_x ? std::min(P.x_min, t_inv) : t_inv;
            P.x_max = any_x ? std::max(P.x_max, t_inv) : t_inv;
            any_x = true;
        } else {
            ++P.orphans;
        }
        P.t_min = any_t ? std::min(P.t_min, t) : t;
        P.t_max = any_t ? std::max(P.t_max, t) : t;
        any_t = true;
        P.t_comp.push_back(t);
        P.t_inv.push_back(t_inv);
        P.meta.push_back(LC_PERF_META(f_inv, h->f[r], h->type[r]));
    }
    for (int64_t v : flat) P.unmatched += v >= 0;
    for (const auto &kv : sparse) P.unmatched += kv.second >= 0;
    if (open) {
        P.intervals.push_back(open_t);
        P.intervals.push_back(hist_max);
    }
    return LC_OK;
}

}  // namespace

extern "C" int lc_perf_pack(const lc_perf_history *h, lc_perf_packed **out) {
    lc::Range range("lc_perf_pack");
    if (!h || !out || h->n < 0) return lc::fail(LC_E_INVALID, "lc_perf_pack: null argument");
    if (h->n > 0 && (!h->type || !h->f || !h->process || !h->time)) return lc::fail(LC_E_INVALID, "lc_perf_pack: null column");
    lc_perf_packed *P = nullptr;
    try {
        P = new lc_perf_packed();
        if (int rc = pack(h, *P)) {
            delete P;
            return rc;
        }
    } catch (const std::bad_alloc &) {
        delete P;
        return lc::fail(LC_E_NOMEM, "lc_perf_pack: out of memory");
    }
    *out = P;
    return LC_OK;
}

extern "C" void lc_perf_packed_free(lc_perf_packed *p) { delete p; }

extern "C" int lc_perf_packed_view(const lc_perf_packed *p, lc_perf_batch *out) {
    if (!p || !out) return lc::fail(LC_E_INVALID, "lc_perf_packed_view: null argument");
    std::memset(out, 0, sizeof *out);
    out->n = (int64_t)p->t_comp.size();
    out->t_comp = p->t_comp.data(); out->t_inv = p->t_inv.data(); out->meta = p->meta.data();
    out->n_matched = p->matched;
    out->t_min = p->t_min; out->t_max = p->t_max; out->x_min = p->x_min; out->x_max = p->x_max;
    out->n_f = p->n_f;
    return LC_OK;
}

extern "C" int lc_perf_packed_info(const lc_perf_packed *p, int64_t *out4) {
    if (!p || !out4) return lc::fail(LC_E_INVALID, "lc_perf_packed_info: null argument");
    out4[0] = p->matched; out4[1] = p->unmatched; out4[2] = p->orphans; out4[3] = (int64_t)p->intervals.size() / 2;
    return LC_OK;
}

extern "C" int lc_perf_packed_intervals(const lc_perf_packed *p, int64_t *out) {
    if (!p || (!out && !p->intervals.empty())) return lc::fail(LC_E_INVALID, "lc_perf_packed_intervals: null argument");
    if (!p->intervals.empty()) std::memcpy(out, p->intervals.data(), p->intervals.size() * 8);
    return LC_OK;
}

extern "C" void lc_perf_opts_default(lc_perf_opts *o) {
    if (!o) return;
    std::memset(o, 0, sizeof *o);
    o->quantile_dt_ns = 30000000000ll;
    o->rate_dt_ns = 10000000000ll;
    o->n_q = 4;
    o->q[0] = 0.5; o->q[1] = 0.95; o->q[2] = 0.99; o->q[3] = 1.0;
}

extern "C" int lc_perf_shape(const lc_perf_batch *b, const lc_perf_opts *o, int64_t *out4) {
    if (!b || !o || !out4) return lc::fail(LC_E_INVALID, "lc_perf_shape: null argument");
    if (b->n < 0 || b->n_matched < 0 || b->n_matched > b->n || b->n_f < 0)
        return lc::fail(LC_E_INVALID, "lc_perf_shape: bad record counts");
    if (b->n > 0 && b->t_max < b->t_min) return lc::fail(LC_E_INVALID, "lc_perf_shape: t_max below t_min");
    if (b->n_matched > 0 && b->x_max < b->x_min) return lc::fail(LC_E_INVALID, "lc_perf_shape: x_max below x_min");
    const lcp::PerfShape s = lcp::perf_shape(b, o->rate_dt_ns, o->quantile_dt_ns);
    if (s.rc == LC_E_INVALID) return lc::fail(LC_E_INVALID, "lc_perf: a bucket width is not positive");
    if (s.rc) return lc::fail(s.rc, "lc_perf: the tables pass %llu entries: widen the buckets", (unsigned long long)lcp::PERF_MAX_TABLE);
    out4[0] = s.rate_first; out4[1] = s.rate_n; out4[2] = s.q_first; out4[3] = s.q_n;
    return LC_OK;
}

int lcp::perf_opts_check(const lc_perf_batch *b, const lc_perf_opts *o, int64_t *shape4) {
    if (o->n_q < 1 || o->n_q > LC_PERF_MAX_Q) return lc::fail(LC_E_INVALID, "lc_perf_check: n_q %d is not in 1..%d", o->n_q, LC_PERF_MAX_Q);
    for (int j = 0; j < o->n_q; ++j)
        if (!(o->q[j] >= 0.0 && o->q[j] <= 1.0)) return lc::fail(LC_E_INVALID, "lc_perf_check: quantile %d is not in [0, 1]", j);
    if (b->n_f > LC_PERF_MAX_F)
        return lc::fail(LC_E_UNSUPPORTED, "lc_perf_check: %d distinct :f, at most %d are supported", b->n_f, LC_PERF_MAX_F);
    return lc_perf_shape(b, o, shape4);
}

extern "C" int lc_perf_launch_info(int64_t *out4) {
    if (!out4) return lc::fail(LC_E_INVALID, "lc_perf_launch_info: null argument");
    out4[0] = lcp::PERF_WG_RECORDS; out4[1] = lcp::PERF_TILE_BUCKETS; out4[2] = lcp::PERF_LDS_MAX; out4[3] = lcp::PERF_DIGIT_BITS;
    return LC_OK;
}
