// host_perf_pack.cpp -- lc_perf_check_history's host half
// (include/lincheck_perf_pack.h): the argument checks,
// the fold of the compacted nemesis rows into intervals, and the library-owned
// result object.  Nothing here runs per row of the history.  The device half is
// device_perf_pack.hpp's.  No HIP in this file.

#include <cstring>

#include "common.hpp"
#include "device_perf_pack.hpp"
#include "perf_plan.hpp"
#include "rows_plan.hpp"

struct lc_perf_checked {
    lcpp::PpOut o;
    std::vector<int64_t> intervals;  // (t0, t1) pairs
    bool has_records = false;
};

void lcpp::pp_fold_intervals(const std::vector<int64_t> &nem, int32_t f_start, int32_t f_stop, int64_t hist_max,
                             std::vector<int64_t> &out) {
    bool open = false;
    int64_t open_t = 0;
    for (size_t i = 0; i + 1 < nem.size(); i += 2) {
        const int32_t f = (int32_t)nem[i];
        const int64_t t = nem[i + 1];
        if (f == f_start && !open) {
            open = true;
            open_t = t;
        } else if (f == f_stop && open) {
            open = false;
            out.push_back(open_t);
            out.push_back(t);
        }
    }
    if (open) {
        out.push_back(open_t);
        out.push_back(hist_max);
    }
}

namespace {

lc_perf_batch sizes_of(const lcpp::PpOut &o) {
    lc_perf_batch b{};
    b.n = o.n_rec;
    b.n_matched = o.matched;
    b.t_min = o.t_min; b.t_max = o.t_max; b.x_min = o.x_min; b.x_max = o.x_max;
    b.n_f = o.n_f;
    return b;
}

}  // namespace

extern "C" int lc_perf_check_history(lc_ctx *ctx, const lc_perf_history *h, const lc_perf_opts *o, lc_perf_checked **out) {
    if (!ctx || !h || !o || !out || h->n < 0) return lc::fail(LC_E_INVALID, "lc_perf_check_history: null argument");
    if (h->n > 0 && (!h->type || !h->f || !h->process || !h->time)) return lc::fail(LC_E_INVALID, "lc_perf_check_history: null column");
    if (h->n_f < 0 || h->n_f > 256) return lc::fail(LC_E_INVALID, "lc_perf_check_history: n_f %d", h->n_f);
    if (h->n_f > LC_PERF_MAX_F)
        return lc::fail(LC_E_UNSUPPORTED, "lc_perf_check_history: %d distinct :f, at most %d are supported", h->n_f, LC_PERF_MAX_F);
    if ((uint64_t)h->n > lcr::RP_MAX_ROWS)
        return lc::fail(LC_E_UNSUPPORTED, "lc_perf_check_history: %lld rows (at most 2^31 - 16)", (long long)h->n);
    lc::Range range("lc_perf_check_history");
    try {
        auto *c = new lc_perf_checked();
        c->o.n_f = h->n_f;
        int rc = LC_OK;
        if (h->n == 0) {  // lc_perf_check on a batch of no records: its checks, no table
            const lc_perf_batch b = sizes_of(c->o);
            rc = lcp::perf_opts_check(&b, o, c->o.shape);
            c->has_records = true;
        } else if (!lcpp::pp_dev_check) {
            rc = lc::fail(LC_E_DEVICE, "lc_perf_check_history: built without its device half");
        } else {
            rc = lcpp::pp_dev_check(ctx, h, o, &c->o);
        }
        if (rc) {
            delete c;
            return rc;
        }
        if (c->o.n_rec == 0) c->has_records = true;
        lcpp::pp_fold_intervals(c->o.nem, h->f_start, h->f_stop, c->o.hist_max, c->intervals);
        *out = c;
        return LC_OK;
    } catch (const std::bad_alloc &) {
        return lc::fail(LC_E_NOMEM, "lc_perf_check_history: out of memory");
    }
}

extern "C" void lc_perf_checked_free(lc_perf_checked *c) { delete c; }

extern "C" int lc_perf_checked_view(const lc_perf_checked *c, lc_perf_batch *sizes, lc_perf_result *result) {
    if (!c || !sizes || !result) return lc::fail(LC_E_INVALID, "lc_perf_checked_view: null argument");
    const lcpp::PpOut &o = c->o;
    *sizes = sizes_of(o);
    *result = lc_perf_result{};
    result->rate = const_cast<uint64_t *>(o.rate.data());
    result->group = const_cast<uint64_t *>(o.group.data());
    result->quant = const_cast<int64_t *>(o.quant.data());
    result->rate_cap = o.rate.size(); result->group_cap = o.group.size(); result->quant_cap = o.quant.size();
    result->rate_first = o.shape[0]; result->rate_n = o.shape[1]; result->q_first = o.shape[2]; result->q_n = o.shape[3];
    return LC_OK;
}

extern "C" int lc_perf_checked_info(const lc_perf_checked *c, int64_t *out4) {
    if (!c || !out4) return lc::fail(LC_E_INVALID, "lc_perf_checked_info: null argument");
    out4[0] = c->o.matched; out4[1] = c->o.unmatched; out4[2] = c->o.orphans; out4[3] = (int64_t)c->intervals.size() / 2;
    return LC_OK;
}

extern "C" int lc_perf_checked_intervals(const lc_perf_checked *c, int64_t *out) {
    if (!c || (!out && !c->intervals.empty())) return lc::fail(LC_E_INVALID, "lc_perf_checked_intervals: null argument");
    if (!c->intervals.empty()) std::memcpy(out, c->intervals.data(), c->intervals.size() * 8);
    return LC_OK;
}

extern "C" int lc_perf_checked_records(lc_ctx *ctx, lc_perf_checked *c, lc_perf_batch *out) {
    if (!ctx || !c || !out) return lc::fail(LC_E_INVALID, "lc_perf_checked_records: null argument");
    if (!c->has_records) {
        if (!lcpp::pp_dev_records) return lc::fail(LC_E_DEVICE, "lc_perf_checked_records: built without its device half");
        try {
            if (int rc = lcpp::pp_dev_records(ctx, &c->o)) return rc;
        } catch (const std::bad_alloc &) {
            return lc::fail(LC_E_NOMEM, "lc_perf_checked_records: out of memory");
        }
        c->has_records = true;
    }
    *out = sizes_of(c->o);
    out->t_comp = c->o.t_comp.data(); out->t_inv = c->o.t_inv.data(); out->meta = c->o.meta.data();
    return LC_OK;
}

extern "C" int lc_perf_history_timing(lc_ctx *ctx, double *out6) {
    if (!ctx || !out6) return lc::fail(LC_E_INVALID, "lc_perf_history_timing: null argument");
    if (!lcpp::pp_dev_timing) {
        std::memset(out6, 0, 6 * sizeof(double));
        return LC_OK;
    }
    return lcpp::pp_dev_timing(ctx, out6);
}

extern "C" int lc_perf_pack_launch_info(int64_t *out3) {
    if (!out3) return lc::fail(LC_E_INVALID, "lc_perf_pack_launch_info: null out");
    out3[0] = lcr::RP_BLOCK;
    out3[1] = lcr::RP_TILE;
    out3[2] = (int64_t)lcr::RP_MAX_ROWS;
    return LC_OK;
}
