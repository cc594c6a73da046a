// host_counter_pack.cpp -- lc_counter_check_history's host half
// (include/lincheck_counter_pack.h): the argument
// checks, the library-owned result object and what is shaped from it on the
// host -- per key, never per row: valid and n_errors from err_off, an error
// key's text from its code.  The device half is device_counter_pack.hpp's.  No
// HIP in this file.

#include <cstring>
#include <string>

#include "common.hpp"
#include "counter_pack_plan.hpp"
#include "counter_plan.hpp"
#include "device_counter_pack.hpp"
#include "rows_plan.hpp"

struct lc_counter_checked {
    lccp::CpOut o;
    std::vector<int8_t> valid;
    std::vector<uint64_t> n_errors;
    bool has_batch = false;
};

namespace {

// A history of no rows: lc_counter_pack's one key LC_NO_KEY without events, valid.
void fill_empty(lc_counter_checked &c) {
    lccp::CpOut &o = c.o;
    o.n_keys = 1;
    o.keys.assign(1, LC_NO_KEY);
    o.status.assign(1, LC_COUNTER_KEY_OK);
    o.error.assign(1, lccp::CP_NO_ERROR);
    o.ev_off.assign(2, 0); o.read_off.assign(2, 0); o.err_off.assign(2, 0);
    c.has_batch = true;
}

void shape(lc_counter_checked &c) {
    const lccp::CpOut &o = c.o;
    const size_t K = (size_t)o.n_keys;
    c.valid.resize(K);
    c.n_errors.resize(K);
    for (size_t k = 0; k < K; ++k) {
        c.n_errors[k] = o.err_off[k + 1] - o.err_off[k];
        c.valid[k] = o.status[k] != LC_COUNTER_KEY_OK ? LC_UNKNOWN : c.n_errors[k] ? LC_INVALID : LC_VALID;
    }
}

}  // namespace

extern "C" int lc_counter_check_history(lc_ctx *ctx, const lc_counter_history *h, const lc_counter_opts *o, lc_counter_checked **out) {
    if (!ctx || !h || !o || !out || h->n < 0) return lc::fail(LC_E_INVALID, "lc_counter_check_history: null argument");
    if (h->n > 0 && (!h->type || !h->f || !h->value)) return lc::fail(LC_E_INVALID, "lc_counter_check_history: null column");
    if (o->flags) return lc::fail(LC_E_INVALID, "lc_counter_check_history: unknown flags 0x%x", o->flags);
    const uint32_t tile = lcc::ct_tile_of(o->tile);
    if (!tile) return lc::fail(LC_E_INVALID, "lc_counter_check_history: tile %u (256 or 2048)", o->tile);
    if ((uint64_t)h->n > lcr::RP_MAX_ROWS)
        return lc::fail(LC_E_UNSUPPORTED, "lc_counter_check_history: %lld rows (at most 2^31 - 16)", (long long)h->n);
    lc::Range range("lc_counter_check_history");
    try {
        auto *c = new lc_counter_checked();
        int rc = LC_OK;
        if (h->n == 0) fill_empty(*c);
        else if (!lccp::cp_dev_check) rc = lc::fail(LC_E_DEVICE, "lc_counter_check_history: built without its device half");
        else rc = lccp::cp_dev_check(ctx, h, tile, &c->o);
        if (rc) {
            delete c;
            return rc;
        }
        shape(*c);
        *out = c;
        return LC_OK;
    } catch (const std::bad_alloc &) {
        return lc::fail(LC_E_NOMEM, "lc_counter_check_history: out of memory");
    }
}

extern "C" void lc_counter_checked_free(lc_counter_checked *c) { delete c; }

extern "C" int lc_counter_checked_view(const lc_counter_checked *c, lc_counter_batch *sizes, lc_counter_result *result) {
    if (!c || !sizes || !result) return lc::fail(LC_E_INVALID, "lc_counter_checked_view: null argument");
    const lccp::CpOut &o = c->o;
    *sizes = lc_counter_batch{};
    sizes->n_keys = o.n_keys;
    sizes->ev_off = o.ev_off.data(); sizes->read_off = o.read_off.data(); sizes->status = o.status.data();
    *result = lc_counter_result{};
    result->valid = const_cast<int8_t *>(c->valid.data());
    result->n_errors = const_cast<uint64_t *>(c->n_errors.data());
    result->lower = const_cast<int64_t *>(o.lower.data());
    result->upper = const_cast<int64_t *>(o.upper.data());
    result->err_off = const_cast<uint64_t *>(o.err_off.data());
    result->err_idx = const_cast<uint64_t *>(o.err_idx.data());
    result->err_cap = o.n_err;
    result->n_err = o.n_err;
    return LC_OK;
}

extern "C" int lc_counter_checked_keys(const lc_counter_checked *c, int64_t *out) {
    if (!c || !out) return lc::fail(LC_E_INVALID, "lc_counter_checked_keys: null argument");
    std::copy(c->o.keys.begin(), c->o.keys.end(), out);
    return LC_OK;
}

extern "C" const char *lc_counter_checked_key_error(const lc_counter_checked *c, int64_t i) {
    if (!c || i < 0 || i >= c->o.n_keys || c->o.status[(size_t)i] == LC_COUNTER_KEY_OK) return nullptr;
    return lccp::cp_error_text(lccp::cp_word_code(c->o.error[(size_t)i]));
}

extern "C" int64_t lc_counter_checked_key_error_row(const lc_counter_checked *c, int64_t i) {
    if (!c || i < 0 || i >= c->o.n_keys || c->o.status[(size_t)i] == LC_COUNTER_KEY_OK) return -1;
    return (int64_t)lccp::cp_word_row(c->o.error[(size_t)i]);
}

extern "C" int lc_counter_checked_read_vals(const lc_counter_checked *c, int64_t *out) {
    if (!c || !out) return lc::fail(LC_E_INVALID, "lc_counter_checked_read_vals: null argument");
    std::copy(c->o.read_val.begin(), c->o.read_val.end(), out);
    return LC_OK;
}

extern "C" int lc_counter_checked_batch(lc_ctx *ctx, lc_counter_checked *c, lc_counter_batch *out) {
    if (!ctx || !c || !out) return lc::fail(LC_E_INVALID, "lc_counter_checked_batch: null argument");
    if (!c->has_batch) {
        if (!lccp::cp_dev_batch) return lc::fail(LC_E_DEVICE, "lc_counter_checked_batch: built without its device half");
        if (int rc = lccp::cp_dev_batch(ctx, &c->o)) return rc;
        c->has_batch = true;
    }
    const lccp::CpOut &o = c->o;
    out->n_keys = o.n_keys;
    out->ev_off = o.ev_off.data(); out->ev_kind = o.ev_kind.data(); out->ev_val = o.ev_val.data();
    out->read_off = o.read_off.data(); out->read_val = o.read_val.data(); out->status = o.status.data();
    return LC_OK;
}

extern "C" int lc_counter_history_timing(lc_ctx *ctx, double *out6) {
    if (!ctx || !out6) return lc::fail(LC_E_INVALID, "lc_counter_history_timing: null argument");
    if (!lccp::cp_dev_timing) {
        std::memset(out6, 0, 6 * sizeof(double));
        return LC_OK;
    }
    return lccp::cp_dev_timing(ctx, out6);
}

extern "C" int lc_counter_pack_launch_info(int64_t *out3) {
    if (!out3) return lc::fail(LC_E_INVALID, "lc_counter_pack_launch_info: null out");
    out3[0] = lcr::RP_BLOCK;
    out3[1] = lcr::RP_TILE;
    out3[2] = (int64_t)lcr::RP_MAX_ROWS;
    return LC_OK;
}

extern "C" int64_t lc_counter_pack_table_slots(int64_t n) { return n < 0 ? 0 : (int64_t)lcr::rp_slots((uint64_t)n); }
