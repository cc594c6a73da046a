// A stand-alone driver of lc_perf_check_history's HOST half for the sanitizer
// test (tests/test_perf_device_pack_abi.py): built with
// -fsanitize=address,undefined together with csrc/host_perf_pack.cpp and
// csrc/host_perf.cpp and nothing else.  Built with -DPP_NO_DEVICE_HALF the
// device half is absent, as in a build of the host files alone: the refusals
// run, the device call answers LC_E_DEVICE, a history of no rows is answered.
// Built without it the device half is stubbed: it fills the
// counts and bounds from lc_perf_pack and compacts the nemesis rows as the
// device does.  So what runs is the argument checks, the fold of the compacted
// nemesis rows into intervals (held against lc_perf_pack's own intervals and
// against answers written out here) and the library-owned result object.  The
// few helpers of csrc/common.cpp that the two files use are given here, since
// common.cpp itself needs the HIP runtime.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "common.hpp"
#include "device_perf_pack.hpp"
#include "perf_plan.hpp"

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
}  // namespace lc

#define REQUIRE(x)                                                          \
    do {                                                                    \
        if (!(x)) {                                                         \
            std::printf("line %d: %s (%s)\n", __LINE__, #x, lc::g_err.c_str()); \
            return 1;                                                       \
        }                                                                   \
    } while (0)

#ifndef PP_NO_DEVICE_HALF
namespace lcpp {

static uint64_t g_generation = 0;
static double g_ms[6] = {1, 2, 3, 4, 5, 6};

int pp_dev_check(lc_ctx *, const lc_perf_history *h, const lc_perf_opts *o, PpOut *out) {
    lc_perf_packed *p = nullptr;
    if (int rc = lc_perf_pack(h, &p)) return rc;
    lc_perf_batch b{};
    int64_t info[4];
    lc_perf_packed_view(p, &b);
    lc_perf_packed_info(p, info);
    out->n_rec = b.n; out->matched = info[0]; out->unmatched = info[1]; out->orphans = info[2];
    out->t_min = b.t_min; out->t_max = b.t_max; out->x_min = b.x_min; out->x_max = b.x_max;
    out->t_comp.assign(b.t_comp, b.t_comp + b.n); out->t_inv.assign(b.t_inv, b.t_inv + b.n); out->meta.assign(b.meta, b.meta + b.n);
    out->hist_max = h->time[0];
    for (int64_t r = 0; r < h->n; ++r) {
        if (h->time[r] > out->hist_max) out->hist_max = h->time[r];
        if (h->process[r] == LC_NO_PROCESS && ((int32_t)h->f[r] == h->f_start || (int32_t)h->f[r] == h->f_stop)) {
            out->nem.push_back(h->f[r]);
            out->nem.push_back(h->time[r]);
        }
    }
    b.t_comp = nullptr;
    const int rc = lcp::perf_opts_check(&b, o, out->shape);
    if (!rc) {
        out->rate.assign((size_t)(b.n_f * 3 * out->shape[1]), 0);
        out->group.assign((size_t)(b.n_f * out->shape[3]), 0);
        out->quant.assign((size_t)(b.n_f * out->shape[3] * o->n_q), 0);
    }
    out->generation = ++g_generation;
    lc_perf_packed_free(p);
    return rc;
}

int pp_dev_records(lc_ctx *, PpOut *o) { return o->generation == g_generation ? LC_OK : lc::fail(LC_E_INVALID, "not the latest"); }

int pp_dev_timing(lc_ctx *, double *out6) {
    std::memcpy(out6, g_ms, sizeof g_ms);
    return LC_OK;
}

}  // namespace lcpp

namespace {

// The intervals of one history through lc_perf_check_history, held against lc_perf_pack's.
int intervals_of(lc_ctx *ctx, const lc_perf_history &h, std::vector<int64_t> &iv) {
    lc_perf_opts o;
    lc_perf_opts_default(&o);
    lc_perf_checked *c = nullptr;
    REQUIRE(lc_perf_check_history(ctx, &h, &o, &c) == LC_OK);
    int64_t info[4], want_info[4];
    REQUIRE(lc_perf_checked_info(c, info) == LC_OK);
    iv.assign((size_t)info[3] * 2, 0);
    REQUIRE(lc_perf_checked_intervals(c, iv.data()) == LC_OK);
    lc_perf_packed *p = nullptr;
    REQUIRE(lc_perf_pack(&h, &p) == LC_OK && lc_perf_packed_info(p, want_info) == LC_OK);
    std::vector<int64_t> want((size_t)want_info[3] * 2);
    REQUIRE(lc_perf_packed_intervals(p, want.data()) == LC_OK);
    REQUIRE(!std::memcmp(info, want_info, sizeof info) && iv == want);
    lc_perf_packed_free(p);
    lc_perf_checked_free(c);
    return 0;
}

}  // namespace
#endif

int main() {
    lc_ctx *ctx = (lc_ctx *)(uintptr_t)16;  // never dereferenced: the stub takes no context
    // f: 0 read, 1 start, 2 stop.  A matched read, starts logged twice, a stop, a start left open; the largest time is an :invoke's
    const uint8_t type[] = {LC_INVOKE, LC_INFO, LC_INFO, LC_OK_T, LC_INFO, LC_INFO, LC_INFO, LC_INVOKE};
    const uint8_t f[] = {0, 1, 1, 0, 2, 2, 1, 0};
    const int64_t process[] = {3, LC_NO_PROCESS, LC_NO_PROCESS, 3, LC_NO_PROCESS, LC_NO_PROCESS, LC_NO_PROCESS, 4};
    const int64_t time[] = {10, 20, 21, 30, 40, 41, 50, 90};
    lc_perf_history h{8, type, f, process, time, 3, 1, 2};
    lc_perf_opts o;
    lc_perf_opts_default(&o);
    lc_perf_checked *c = nullptr;
    // refusals, none of which asks the device half
    REQUIRE(lc_perf_check_history(nullptr, &h, &o, &c) == LC_E_INVALID);
    REQUIRE(lc_perf_check_history(ctx, nullptr, &o, &c) == LC_E_INVALID);
    REQUIRE(lc_perf_check_history(ctx, &h, nullptr, &c) == LC_E_INVALID);
    REQUIRE(lc_perf_check_history(ctx, &h, &o, nullptr) == LC_E_INVALID);
    lc_perf_history bad = h;
    bad.n = -1;
    REQUIRE(lc_perf_check_history(ctx, &bad, &o, &c) == LC_E_INVALID);
    bad = h; bad.time = nullptr;
    REQUIRE(lc_perf_check_history(ctx, &bad, &o, &c) == LC_E_INVALID);
    bad = h; bad.n_f = 257;
    REQUIRE(lc_perf_check_history(ctx, &bad, &o, &c) == LC_E_INVALID);
    bad.n_f = -1;
    REQUIRE(lc_perf_check_history(ctx, &bad, &o, &c) == LC_E_INVALID);
    bad.n_f = LC_PERF_MAX_F + 1;
    REQUIRE(lc_perf_check_history(ctx, &bad, &o, &c) == LC_E_UNSUPPORTED);
    bad = h; bad.n = 0x7FFFFFF1ll;
    REQUIRE(lc_perf_check_history(ctx, &bad, &o, &c) == LC_E_UNSUPPORTED);
#ifdef PP_NO_DEVICE_HALF
    REQUIRE(lc_perf_check_history(ctx, &h, &o, &c) == LC_E_DEVICE && c == nullptr);
#endif
    // no rows: no device half is asked; lc_perf_check's own refusals hold
    lc_perf_history none{};
    none.n_f = 2; none.f_start = -1; none.f_stop = -1;
    REQUIRE(lc_perf_check_history(ctx, &none, &o, &c) == LC_OK);
    lc_perf_batch b{};
    lc_perf_result r{};
    int64_t info[4] = {9, 9, 9, 9};
    REQUIRE(lc_perf_checked_view(c, &b, &r) == LC_OK && b.n == 0 && b.n_matched == 0 && b.n_f == 2 && !b.t_comp);
    REQUIRE(r.rate_n == 0 && r.q_n == 0 && r.rate_cap == 0 && r.group_cap == 0 && r.quant_cap == 0);
    REQUIRE(lc_perf_checked_info(c, info) == LC_OK && !info[0] && !info[1] && !info[2] && !info[3]);
    REQUIRE(lc_perf_checked_intervals(c, nullptr) == LC_OK);
    REQUIRE(lc_perf_checked_records(ctx, c, &b) == LC_OK && b.n == 0);
    lc_perf_checked_free(c);
    c = nullptr;
    lc_perf_opts bad_o = o;
    bad_o.n_q = 0;
    REQUIRE(lc_perf_check_history(ctx, &none, &bad_o, &c) == LC_E_INVALID && c == nullptr);
    bad_o = o; bad_o.rate_dt_ns = 0;
    REQUIRE(lc_perf_check_history(ctx, &none, &bad_o, &c) == LC_E_INVALID);
    bad_o = o; bad_o.q[1] = 1.5;
    REQUIRE(lc_perf_check_history(ctx, &none, &bad_o, &c) == LC_E_INVALID);

#ifdef PP_NO_DEVICE_HALF
    double none_ms[6] = {7, 7, 7, 7, 7, 7};
    REQUIRE(lc_perf_history_timing(ctx, none_ms) == LC_OK && none_ms[0] == 0.0 && none_ms[5] == 0.0);
#else
    // the fold: starts logged twice open once; the second stop closes nothing; the last start runs to the :invoke at 90
    std::vector<int64_t> iv;
    if (intervals_of(ctx, h, iv)) return 1;
    REQUIRE((iv == std::vector<int64_t>{20, 40, 50, 90}));
    // f_start == f_stop: every other such row closes what the one before opened
    lc_perf_history same = h;
    same.f_start = 1; same.f_stop = 1;
    if (intervals_of(ctx, same, iv)) return 1;
    REQUIRE((iv == std::vector<int64_t>{20, 21, 50, 90}));
    // both -1: no row is a nemesis row
    lc_perf_history neither = h;
    neither.f_start = -1; neither.f_stop = -1;
    if (intervals_of(ctx, neither, iv)) return 1;
    REQUIRE(iv.empty());
    // no :start: stops alone open nothing; no :stop: one interval to the end
    lc_perf_history only = h;
    only.f_start = -1;
    if (intervals_of(ctx, only, iv)) return 1;
    REQUIRE(iv.empty());
    only = h; only.f_stop = -1;
    if (intervals_of(ctx, only, iv)) return 1;
    REQUIRE((iv == std::vector<int64_t>{20, 90}));
    // the largest time on a nemesis row, and a history of nemesis rows alone
    const int64_t time2[] = {10, 20, 21, 30, 40, 41, 95, 90};
    lc_perf_history late = h;
    late.time = time2;
    if (intervals_of(ctx, late, iv)) return 1;
    REQUIRE((iv == std::vector<int64_t>{20, 40, 95, 95}));
    lc_perf_history nem{3, type + 4, f + 4, process + 4, time + 4, 3, 1, 2};
    if (intervals_of(ctx, nem, iv)) return 1;
    REQUIRE((iv == std::vector<int64_t>{50, 50}));
    lcpp::pp_fold_intervals(std::vector<int64_t>(), 1, 2, 7, iv);  // no nemesis row: nothing is added
    REQUIRE(iv.size() == 2);

    // the result object
    REQUIRE(lc_perf_check_history(ctx, &h, &o, &c) == LC_OK);
    REQUIRE(lc_perf_checked_view(c, &b, &r) == LC_OK && b.n == 1 && b.n_matched == 1 && !b.t_comp && !b.t_inv && !b.meta);
    REQUIRE(b.t_min == 30 && b.t_max == 30 && b.x_min == 10 && b.x_max == 10 && b.n_f == 3);
    REQUIRE(r.rate_n == 1 && r.q_n == 1 && r.rate_cap == 9 && r.group_cap == 3 && r.quant_cap == 12 && r.rate && r.group && r.quant);
    REQUIRE(lc_perf_checked_info(c, info) == LC_OK && info[0] == 1 && info[1] == 1 && info[2] == 0 && info[3] == 2);
    REQUIRE(lc_perf_checked_records(ctx, c, &b) == LC_OK && b.n == 1 && b.t_comp[0] == 30 && b.t_inv[0] == 10);
    REQUIRE(b.meta[0] == LC_PERF_META(0, 0, LC_OK_T));
    // an older object is refused its records once a later call has run; one whose records are down keeps them
    lc_perf_checked *older = nullptr, *fresh = nullptr;
    REQUIRE(lc_perf_check_history(ctx, &h, &o, &older) == LC_OK && lc_perf_check_history(ctx, &h, &o, &fresh) == LC_OK);
    REQUIRE(lc_perf_checked_records(ctx, older, &b) == LC_E_INVALID && lc_perf_checked_records(ctx, fresh, &b) == LC_OK);
    REQUIRE(lc_perf_checked_records(ctx, c, &b) == LC_OK && b.t_comp[0] == 30);
    // a bad row and a bad option come back as the host path's
    uint8_t bad_type[8];
    std::memcpy(bad_type, type, 8);
    bad_type[5] = 9;
    bad = h; bad.type = bad_type;
    lc_perf_checked *none_c = nullptr;
    REQUIRE(lc_perf_check_history(ctx, &bad, &o, &none_c) == LC_E_INVALID && none_c == nullptr);
    bad_o = o; bad_o.quantile_dt_ns = -1;
    REQUIRE(lc_perf_check_history(ctx, &h, &bad_o, &none_c) == LC_E_INVALID && none_c == nullptr);
    double ms[6];
    REQUIRE(lc_perf_history_timing(ctx, ms) == LC_OK && ms[5] == 6.0 && lc_perf_history_timing(ctx, nullptr) == LC_E_INVALID);
    int64_t li[3];
    REQUIRE(lc_perf_pack_launch_info(li) == LC_OK && li[0] == 256 && li[1] == 2048 && li[2] == 0x7FFFFFF0ll);
    REQUIRE(lc_perf_pack_launch_info(nullptr) == LC_E_INVALID);
    REQUIRE(lc_perf_checked_view(nullptr, &b, &r) == LC_E_INVALID && lc_perf_checked_info(c, nullptr) == LC_E_INVALID);
    REQUIRE(lc_perf_checked_intervals(c, nullptr) == LC_E_INVALID && lc_perf_checked_records(ctx, nullptr, &b) == LC_E_INVALID);
    lc_perf_checked_free(c); lc_perf_checked_free(older); lc_perf_checked_free(fresh);
    lc_perf_checked_free(nullptr);
#endif
    std::printf("ok\n");
    return 0;
}
