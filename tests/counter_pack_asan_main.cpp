// A stand-alone driver of lc_counter_check_history's HOST half for the
// sanitizer test (tests/test_counter_device_pack_abi.py): built with
// -fsanitize=address,undefined together with csrc/host_counter_pack.cpp and
// csrc/host_counter.cpp and nothing else.  The device half is stubbed here: it
// fills the result arrays from lc_counter_pack + lc_counter_check_host, with
// the error words a device would write.  So what runs is the argument checks,
// the library-owned result object and what the host shapes from it.  The few
// helpers of csrc/common.cpp that the two files use are given here, since
// common.cpp itself needs the HIP runtime.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "common.hpp"
#include "counter_pack_plan.hpp"
#include "device_counter_pack.hpp"

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

namespace lccp {

static uint64_t g_generation = 0;
static double g_ms[6] = {1, 2, 3, 4, 5, 6};

int cp_dev_check(lc_ctx *, const lc_counter_history *h, uint32_t, CpOut *o) {
    lc_counter_packed *p = nullptr;
    if (int rc = lc_counter_pack(h, &p)) return rc;
    lc_counter_batch b{};
    lc_counter_packed_view(p, &b);
    const size_t K = (size_t)b.n_keys, E = (size_t)b.ev_off[K], R = (size_t)b.read_off[K];
    o->n_keys = b.n_keys; o->E = E; o->R = R;
    o->keys.resize(K); lc_counter_packed_keys(p, o->keys.data());
    o->status.assign(b.status, b.status + K);
    o->error.assign(K, CP_NO_ERROR);
    for (size_t k = 0; k < K; ++k) {
        const char *why = lc_counter_packed_key_error(p, (int64_t)k);
        for (uint32_t c = 1; why && c < CP_CODES; ++c)
            if (!std::strcmp(why, cp_error_text(c))) o->error[k] = cp_word(k + 7, c);
    }
    o->ev_off.assign(b.ev_off, b.ev_off + K + 1); o->read_off.assign(b.read_off, b.read_off + K + 1);
    o->err_off.resize(K + 1); o->lower.resize(R); o->upper.resize(R); o->err_idx.resize(R);
    o->read_val.assign(b.read_val, b.read_val + R);
    o->ev_kind.assign(b.ev_kind, b.ev_kind + E); o->ev_val.assign(b.ev_val, b.ev_val + E);
    std::vector<int8_t> valid(K);
    std::vector<uint64_t> n_errors(K);
    lc_counter_result r{valid.data(), n_errors.data(), o->lower.data(), o->upper.data(), o->err_off.data(), o->err_idx.data(), R, 0};
    const int rc = lc_counter_check_host(&b, &r);
    o->n_err = r.n_err;
    o->err_idx.resize(r.n_err);
    o->generation = ++g_generation;
    lc_counter_packed_free(p);
    return rc;
}

int cp_dev_batch(lc_ctx *, CpOut *o) {
    return o->generation == g_generation ? LC_OK : lc::fail(LC_E_INVALID, "not the latest");
}

int cp_dev_timing(lc_ctx *, double *out6) {
    std::memcpy(out6, g_ms, sizeof g_ms);
    return LC_OK;
}

}  // namespace lccp

int main() {
    lc_ctx *ctx = (lc_ctx *)(uintptr_t)16;  // never dereferenced: the stub takes no context
    // invoke add 2 / ok add 2 / invoke read / ok read 5 (out of bounds) on key 4; an orphan completion on key 9; a clean key 1
    const uint8_t type[] = {LC_INVOKE, LC_OK_T, LC_INVOKE, LC_OK_T, LC_OK_T, LC_INVOKE, LC_INVOKE, LC_OK_T};
    const uint8_t f[] = {LC_CF_ADD, LC_CF_ADD, LC_CF_READ, LC_CF_READ, LC_CF_ADD, LC_CF_ADD, LC_CF_READ, LC_CF_READ};
    const int64_t process[] = {0, 0, 1, 1, 0, 0, 1, 1};
    const int64_t key[] = {4, 4, 4, 4, 9, 1, 1, 1};
    const int64_t value[] = {2, 2, LC_NIL, 5, 1, 3, LC_NIL, 2};
    lc_counter_history h{8, type, f, process, key, value, nullptr};
    lc_counter_opts o{0, 0};
    lc_counter_checked *c = nullptr;
    // refusals
    REQUIRE(lc_counter_check_history(nullptr, &h, &o, &c) == LC_E_INVALID);
    REQUIRE(lc_counter_check_history(ctx, nullptr, &o, &c) == LC_E_INVALID);
    REQUIRE(lc_counter_check_history(ctx, &h, nullptr, &c) == LC_E_INVALID);
    REQUIRE(lc_counter_check_history(ctx, &h, &o, nullptr) == LC_E_INVALID);
    lc_counter_opts bad{100, 0}, flags{0, 2};
    REQUIRE(lc_counter_check_history(ctx, &h, &bad, &c) == LC_E_INVALID);
    REQUIRE(lc_counter_check_history(ctx, &h, &flags, &c) == LC_E_INVALID);
    lc_counter_history big = h;
    big.n = 0x7FFFFFF1ll;
    REQUIRE(lc_counter_check_history(ctx, &big, &o, &c) == LC_E_UNSUPPORTED);
    big.n = -1;
    REQUIRE(lc_counter_check_history(ctx, &big, &o, &c) == LC_E_INVALID);
    big = h; big.value = nullptr;
    REQUIRE(lc_counter_check_history(ctx, &big, &o, &c) == LC_E_INVALID);
    uint8_t bad_type[8];
    std::memcpy(bad_type, type, 8);
    bad_type[3] = 9;
    big = h; big.type = bad_type;
    REQUIRE(lc_counter_check_history(ctx, &big, &o, &c) == LC_E_INVALID && c == nullptr);
    // no rows: no device half is asked
    lc_counter_history none{};
    REQUIRE(lc_counter_check_history(ctx, &none, &o, &c) == LC_OK);
    lc_counter_batch b{};
    lc_counter_result r{};
    int64_t keys[3];
    REQUIRE(lc_counter_checked_view(c, &b, &r) == LC_OK && b.n_keys == 1 && r.valid[0] == LC_VALID && r.n_err == 0);
    REQUIRE(lc_counter_checked_keys(c, keys) == LC_OK && keys[0] == LC_NO_KEY && !lc_counter_checked_key_error(c, 0));
    REQUIRE(lc_counter_checked_batch(ctx, c, &b) == LC_OK && b.ev_off[1] == 0);
    lc_counter_checked_free(c);
    // the three keys
    REQUIRE(lc_counter_check_history(ctx, &h, &o, &c) == LC_OK);
    REQUIRE(lc_counter_checked_view(c, &b, &r) == LC_OK && b.n_keys == 3 && !b.ev_kind && !b.ev_val && !b.read_val);
    REQUIRE(lc_counter_checked_keys(c, keys) == LC_OK && keys[0] == 4 && keys[1] == 9 && keys[2] == 1);
    REQUIRE(r.valid[0] == LC_INVALID && r.valid[1] == LC_UNKNOWN && r.valid[2] == LC_VALID);
    REQUIRE(r.n_errors[0] == 1 && r.n_errors[1] == 0 && r.n_err == 1 && r.err_cap == 1 && r.err_idx[0] == 0);
    REQUIRE(r.lower[0] == 2 && r.upper[0] == 2 && r.lower[1] == 0 && r.upper[1] == 3);
    REQUIRE(b.status[1] == LC_COUNTER_KEY_ERROR && b.ev_off[3] == 7 && b.read_off[3] == 2);
    REQUIRE(!lc_counter_checked_key_error(c, 0) && lc_counter_checked_key_error_row(c, 0) == -1);
    REQUIRE(!std::strcmp(lc_counter_checked_key_error(c, 1), lccp::cp_error_text(lccp::CP_NO_OPEN)));
    REQUIRE(lc_counter_checked_key_error_row(c, 1) == 8 && !lc_counter_checked_key_error(c, 3) && !lc_counter_checked_key_error(c, -1));
    int64_t vals[2];
    REQUIRE(lc_counter_checked_read_vals(c, vals) == LC_OK && vals[0] == 5 && vals[1] == 2);
    REQUIRE(lc_counter_checked_batch(ctx, c, &b) == LC_OK && b.ev_kind[0] == LC_CE_UP && b.ev_val[3] == 0 && b.read_val[1] == 2);
    // an older object is refused its batch once a later call has run
    lc_counter_checked *later = nullptr;
    REQUIRE(lc_counter_check_history(ctx, &h, &o, &later) == LC_OK);
    lc_counter_checked *older = nullptr;
    lccp::g_generation += 0;
    REQUIRE(lc_counter_checked_batch(ctx, later, &b) == LC_OK);
    REQUIRE(lc_counter_check_history(ctx, &h, &o, &older) == LC_OK);
    lc_counter_checked *fresh = nullptr;
    REQUIRE(lc_counter_check_history(ctx, &h, &o, &fresh) == LC_OK);
    REQUIRE(lc_counter_checked_batch(ctx, older, &b) == LC_E_INVALID && lc_counter_checked_batch(ctx, fresh, &b) == LC_OK);
    double ms[6];
    REQUIRE(lc_counter_history_timing(ctx, ms) == LC_OK && ms[5] == 6.0 && lc_counter_history_timing(ctx, nullptr) == LC_E_INVALID);
    int64_t info[3];
    REQUIRE(lc_counter_pack_launch_info(info) == LC_OK && info[0] == 256 && info[1] == 2048 && info[2] == 0x7FFFFFF0ll);
    REQUIRE(lc_counter_pack_table_slots(129) == 512 && lc_counter_pack_table_slots(-1) == 0);
    REQUIRE(lc_counter_checked_view(nullptr, &b, &r) == LC_E_INVALID && lc_counter_checked_keys(c, nullptr) == LC_E_INVALID);
    lc_counter_checked_free(c); lc_counter_checked_free(later); lc_counter_checked_free(older); lc_counter_checked_free(fresh);
    lc_counter_checked_free(nullptr);
    std::printf("ok\n");
    return 0;
}
