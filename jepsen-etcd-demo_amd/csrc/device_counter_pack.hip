// device_counter_pack.hip -- lc_counter_check_history's device half: a raw
// counter history becomes lc_counter_pack's batch in HBM, and the scan kernels
// of device_counter.hip run on it where it lies (DESIGN.md section 3.18;
// counter_pack_plan.hpp has the rules made local, device_rows.hpp the front end
// that groups and pairs the rows).
//
// A POSITION is a row's place in key-major history order (device_rows.hpp).
// One lane per position or per key in every kernel:
//   k_cp_takes     per row: f is :add or :read; the lowest row with a bad
//                  :type / :f code
//   k_cp_classify  a position judges itself from its predecessor (rule 1) and
//                  lowers its key's error word to its own offence; from its
//                  successor it knows what it yields: an :invoke :add an
//                  LC_CE_UP unless a :fail follows, with the :ok's value when
//                  one does; an :ok :add an LC_CE_LOW; an :invoke :read an
//                  LC_CE_RINV when an :ok follows; an :ok :read an LC_CE_ROK.
//                  An LC_CE_UP's value goes into the scan as two halves.
//   k_cp_kstart    every key's first position, by bisection
//   k_cp_rule3     an add event's value nil or negative, or the key's
//                  LC_CE_UP sum up to it past INT64_MAX: the key's second
//                  error word, read only when rule 1 left the key alone
//   k_cp_flags     "yields an event" and "is an :ok :read", zero in error
//                  keys, for the scan that places events and reads
//   k_cp_offsets   ev_off, read_off, status and the error word of every key
//   k_cp_scatter   ev_kind, ev_val, read_val; a read's two events carry the
//                  :ok row's rank among the batch's reads
//   k_cp_first     a series' first[] entries (counter_plan.hpp), by bisection
// Nobody waits for anybody: error words are 64-bit atomicMin, skipped when the
// word read is already lower.  Ordering is by kernel boundaries on one stream.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>

#include "common.hpp"
#include "counter_pack_plan.hpp"
#include "counter_plan.hpp"
#include "device_counter.hpp"
#include "device_counter_pack.hpp"
#include "device_ctx.hpp"
#include "device_rows.hpp"
#include "rows_plan.hpp"

namespace lccp {

namespace {

typedef unsigned long long u64;
using lcr::RP_BLOCK;
using lcr::RP_NONE;

constexpr int64_t NIL = INT64_MIN;

struct BuildArgs {
    lcr::RowsView v;
    const uint8_t *type, *f;
    const int64_t *value;
    uint8_t *evk;      // [n] what a position yields: LC_CE_*, or CP_NO_EVENT
    int64_t *evv;      // [n] its value; an LC_CE_RINV's: the position of its :ok
    ulonglong2 *sc;    // [n + 1]
    u64 *err1, *err3;  // [n_keys]
    uint32_t *kstart;  // [n_keys + 1]
    u64 *ev_off, *read_off, *errw;
    uint8_t *status;
    uint8_t *ev_kind;
    int64_t *ev_val, *read_val;
};

__device__ inline void lower_word(u64 *w, u64 mine) {
    if (__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > mine) atomicMin(w, mine);
}

__global__ __launch_bounds__(RP_BLOCK) void k_cp_takes(const uint8_t *type, const uint8_t *f, uint32_t n, uint8_t *takes,
                                                      uint32_t *bad_row) {
    const u64 r = (u64)blockIdx.x * RP_BLOCK + threadIdx.x;
    if (r >= n) return;
    const uint8_t t = type[r], ff = f[r];
    takes[r] = ff != LC_CF_OTHER;
    if (t > LC_INFO || ff > LC_CF_OTHER)
        if (__hip_atomic_load(bad_row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > (uint32_t)r) atomicMin(bad_row, (uint32_t)r);
}

__global__ __launch_bounds__(RP_BLOCK) void k_cp_classify(BuildArgs a) {
    const u64 j = (u64)blockIdx.x * RP_BLOCK + threadIdx.x;
    if (j >= a.v.n) return;
    const uint32_t k = a.v.pos_key[j];
    uint8_t kind = CP_NO_EVENT;
    int64_t val = 0;
    u64 lo = 0, hi = 0;
    if (k != a.v.n_keys) {
        const uint32_t r = a.v.pos_row[j], pj = a.v.prev[j], nj = a.v.next[j];
        const uint8_t t = a.type[r], ff = a.f[r];
        const int64_t v = a.value[r];
        uint32_t code = 0;
        if (t == LC_INVOKE) {
            if (pj != RP_NONE && a.type[a.v.pos_row[pj]] == LC_INVOKE) code = CP_SECOND_INVOKE;
            const uint32_t rn = nj != RP_NONE ? a.v.pos_row[nj] : 0;
            const uint8_t tn = nj != RP_NONE ? a.type[rn] : (uint8_t)LC_INVOKE;  // (an invocation: no completion)
            if (ff == LC_CF_ADD) {
                if (tn != LC_FAIL) {
                    kind = LC_CE_UP;
                    val = tn == LC_OK_T ? a.value[rn] : v;
                }
            } else if (tn == LC_OK_T) {
                kind = LC_CE_RINV;
                val = (int64_t)nj;
            }
        } else {
            if (pj == RP_NONE) {
                code = CP_NO_OPEN;
            } else {
                const uint32_t rp = a.v.pos_row[pj];
                if (a.type[rp] != LC_INVOKE) code = CP_NO_OPEN;
                else if (a.f[rp] != ff) code = CP_OTHER_F;
                else if (ff == LC_CF_READ && t == LC_OK_T && v == NIL) code = CP_READ_NIL;
            }
            if (t == LC_OK_T) {
                kind = ff == LC_CF_ADD ? LC_CE_LOW : LC_CE_ROK;
                val = v;
            }
        }
        if (code) lower_word(&a.err1[k], cp_word(r, code));
        if (kind == LC_CE_UP && val >= 0) {  // (nil is negative)
            lo = (u64)val & 0xFFFFFFFFull;
            hi = (u64)val >> 32;
        }
    }
    a.evk[j] = kind;
    a.evv[j] = val;
    a.sc[j] = make_ulonglong2(lo, hi);
}

// The first of pos_key[0 .. n) at or above k (n when none is).
__global__ __launch_bounds__(RP_BLOCK) void k_cp_kstart(BuildArgs a) {
    const u64 k = (u64)blockIdx.x * RP_BLOCK + threadIdx.x;
    if (k > a.v.n_keys) return;
    uint32_t lo = 0, hi = a.v.n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a.v.pos_key[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    a.kstart[k] = lo;
}

__global__ __launch_bounds__(RP_BLOCK) void k_cp_rule3(BuildArgs a) {
    const u64 j = (u64)blockIdx.x * RP_BLOCK + threadIdx.x;
    if (j >= a.v.n) return;
    const uint8_t kind = a.evk[j];
    if (kind != LC_CE_UP && kind != LC_CE_LOW) return;
    const uint32_t k = a.v.pos_key[j];
    const int64_t v = a.evv[j];
    uint32_t code = 0;
    if (v == NIL) {
        code = CP_ADD_NIL;
    } else if (v < 0) {
        code = CP_ADD_NEGATIVE;
    } else if (kind == LC_CE_UP) {
        const ulonglong2 s0 = a.sc[a.kstart[k]], s = a.sc[j];
        if (cp_sum_past_int64(s.x + ((u64)v & 0xFFFFFFFFull) - s0.x, s.y + ((u64)v >> 32) - s0.y)) code = CP_SUM;
    }
    if (code) lower_word(&a.err3[k], cp_word(a.v.pos_row[j], code));
}

__global__ __launch_bounds__(RP_BLOCK) void k_cp_flags(BuildArgs a) {
    const u64 j = (u64)blockIdx.x * RP_BLOCK + threadIdx.x;
    if (j >= a.v.n) return;
    const uint8_t kind = a.evk[j];
    u64 ev = 0, rd = 0;
    if (kind != CP_NO_EVENT) {
        const uint32_t k = a.v.pos_key[j];
        if (a.err1[k] == CP_NO_ERROR && a.err3[k] == CP_NO_ERROR) {
            ev = 1;
            rd = kind == LC_CE_ROK;
        }
    }
    a.sc[j] = make_ulonglong2(ev, rd);
}

__global__ __launch_bounds__(RP_BLOCK) void k_cp_offsets(BuildArgs a) {
    const u64 k = (u64)blockIdx.x * RP_BLOCK + threadIdx.x;
    if (k > a.v.n_keys) return;
    const ulonglong2 s = a.sc[a.kstart[k]];
    a.ev_off[k] = s.x;
    a.read_off[k] = s.y;
    if (k == a.v.n_keys) return;
    const u64 w = a.err1[k] != CP_NO_ERROR ? a.err1[k] : a.err3[k];
    a.errw[k] = w;
    a.status[k] = w != CP_NO_ERROR ? LC_COUNTER_KEY_ERROR : LC_COUNTER_KEY_OK;
}

__global__ __launch_bounds__(RP_BLOCK) void k_cp_scatter(BuildArgs a) {
    const u64 j = (u64)blockIdx.x * RP_BLOCK + threadIdx.x;
    if (j >= a.v.n) return;
    const ulonglong2 s = a.sc[j];
    if (a.sc[j + 1].x == s.x) return;
    const uint8_t kind = a.evk[j];
    int64_t val = a.evv[j];
    if (kind == LC_CE_RINV) {
        val = (int64_t)a.sc[(uint32_t)val].y;
    } else if (kind == LC_CE_ROK) {
        a.read_val[s.y] = val;
        val = (int64_t)s.y;
    }
    a.ev_kind[s.x] = kind;
    a.ev_val[s.x] = val;
}

// first[t], t < tiles: the first entry of off[0 .. K] at or past t * tile; first[tiles] = K + 1 (ct_first_key).
__global__ __launch_bounds__(RP_BLOCK) void k_cp_first(const u64 *off, uint32_t K, uint32_t tile, u64 tiles, uint32_t *first) {
    const u64 t = (u64)blockIdx.x * RP_BLOCK + threadIdx.x;
    if (t > tiles) return;
    if (t == tiles) {
        first[t] = K + 1;
        return;
    }
    const u64 at = t * tile;
    uint32_t lo = 0, hi = K + 1;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (off[mid] < at) lo = mid + 1;
        else hi = mid;
    }
    first[t] = lo;
}

struct PackDev {
    enum { TYPE, F, PROC, KEY, VAL, TAKES, SC, EVK, EVV, ERR1, ERR3, KSTART, EV_OFF, READ_OFF, STATUS, ERRW, EV_KIND, EV_VAL, READ_VAL,
           LOWER, UPPER, FIRST_EV, FIRST_RD, TILES, ERR_OFF, ERR_IDX, OUT, N_MEM };
    lcx::DevBatch::Mem mem[N_MEM];
    lcr::Rows *rows = nullptr;
    char *hstage = nullptr;  // pinned staging of the columns of a caller whose arrays are not page-locked
    size_t hstage_cap = 0;
    unsigned long long *hout = nullptr;  // pinned landing: out (4 words), then E and R
    size_t hout_cap = 0;
    hipEvent_t ev[6] = {};
    double ms[6] = {0, 0, 0, 0, 0, 0};
    uint64_t generation = 0, E = 0;  // the batch the arrays hold
    ~PackDev() {
        lcr::rows_close(rows);
        for (lcx::DevBatch::Mem &m : mem)
            if (m.p) (void)hipFree(m.p);
        if (hstage) (void)hipHostFree(hstage);
        if (hout) (void)hipHostFree(hout);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

void pack_dev_free(void *p) { delete (PackDev *)p; }

int pack_dev_of(lcx::Dev *d, PackDev **out) {
    if (!d->cpackdev) {
        PackDev *D = new (std::nothrow) PackDev();
        if (!D) return lc::fail(LC_E_NOMEM, "lc_counter_check_history: out of memory");
        if (int rc = lcr::rows_open(&D->rows)) {
            delete D;
            return rc;
        }
        d->cpackdev = D;
        d->cpackdev_free = pack_dev_free;
    }
    *out = (PackDev *)d->cpackdev;
    return LC_OK;
}

// One column to the device: straight from a page-locked array, else through its section of the staging block.
int upload(hipStream_t stream, void *dst, const void *src, size_t bytes, char *stage) {
    if (!lcx::pinned(src)) {
        std::memcpy(stage, src, bytes);
        src = stage;
    }
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream));
    return LC_OK;
}

size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }

int check(PackDev &D, hipStream_t stream, const lc_counter_history *h, uint32_t tile, CpOut *out) {
    const auto wall0 = std::chrono::steady_clock::now();
    const size_t n = (size_t)h->n;
    const uint32_t blocks = (uint32_t)lcr::rp_blocks(n);
    for (hipEvent_t &e : D.ev)
        if (!e) HIPCHK(hipEventCreate(&e));
    D.generation++;
    D.E = 0;
    BuildArgs a{};
    uint8_t *type, *f, *takes;
    int64_t *proc = nullptr, *key = nullptr, *value;
    unsigned long long *dout;
    HIPCHK(lcx::grow(D.mem[PackDev::TYPE], type, n));
    HIPCHK(lcx::grow(D.mem[PackDev::F], f, n));
    if (h->process) HIPCHK(lcx::grow(D.mem[PackDev::PROC], proc, n));
    if (h->key) HIPCHK(lcx::grow(D.mem[PackDev::KEY], key, n));
    HIPCHK(lcx::grow(D.mem[PackDev::VAL], value, n));
    HIPCHK(lcx::grow(D.mem[PackDev::TAKES], takes, n));
    HIPCHK(lcx::grow(D.mem[PackDev::OUT], dout, (size_t)4));
    HIPCHK(lcx::grow_pinned(D.hout, D.hout_cap, (size_t)8));
    const size_t s_f = align16(n), s_proc = s_f + align16(n), s_key = s_proc + n * 8, s_val = s_key + n * 8;
    HIPCHK(lcx::grow_pinned(D.hstage, D.hstage_cap, s_val + n * 8));

    HIPCHK(hipEventRecord(D.ev[0], stream));
    LCCHK(upload(stream, type, h->type, n, D.hstage));
    LCCHK(upload(stream, f, h->f, n, D.hstage + s_f));
    if (proc) LCCHK(upload(stream, proc, h->process, n * 8, D.hstage + s_proc));
    if (key) LCCHK(upload(stream, key, h->key, n * 8, D.hstage + s_key));
    LCCHK(upload(stream, value, h->value, n * 8, D.hstage + s_val));
    HIPCHK(hipEventRecord(D.ev[1], stream));
    // out: [0] the reads out of bounds, [1] the scan kernels' error word, [2] the lowest row with a bad code
    HIPCHK(hipMemsetAsync(dout, 0, 16, stream));
    HIPCHK(hipMemsetAsync(dout + 2, 0xFF, 8, stream));
    k_cp_takes<<<blocks, RP_BLOCK, 0, stream>>>(type, f, (uint32_t)n, takes, (uint32_t *)(dout + 2));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(D.hout + 2, dout + 2, 8, hipMemcpyDeviceToHost, stream));
    uint64_t n_keys = 0, n_procs = 0;
    LCCHK(lcr::rows_group(D.rows, stream, lcr::RowsIn{(uint32_t)n, takes, proc, key}, &n_keys, &n_procs));
    if ((uint32_t)D.hout[2] != RP_NONE)
        return lc::fail(LC_E_INVALID, "lc_counter_check_history: row %lld: bad :type / :f code", (long long)(uint32_t)D.hout[2]);
    LCCHK(lcr::rows_pair(D.rows, stream, &a.v));
    HIPCHK(hipEventRecord(D.ev[2], stream));

    const size_t K = a.v.n_keys;
    a.type = type; a.f = f; a.value = value;
    HIPCHK(lcx::grow(D.mem[PackDev::SC], a.sc, n + 1));
    HIPCHK(lcx::grow(D.mem[PackDev::EVK], a.evk, n));
    HIPCHK(lcx::grow(D.mem[PackDev::EVV], a.evv, n));
    HIPCHK(lcx::grow(D.mem[PackDev::ERR1], a.err1, K));
    HIPCHK(lcx::grow(D.mem[PackDev::ERR3], a.err3, K));
    HIPCHK(lcx::grow(D.mem[PackDev::KSTART], a.kstart, K + 1));
    HIPCHK(lcx::grow(D.mem[PackDev::EV_OFF], a.ev_off, K + 1));
    HIPCHK(lcx::grow(D.mem[PackDev::READ_OFF], a.read_off, K + 1));
    HIPCHK(lcx::grow(D.mem[PackDev::STATUS], a.status, K));
    HIPCHK(lcx::grow(D.mem[PackDev::ERRW], a.errw, K));
    try {
        out->keys.resize(K); out->status.resize(K); out->error.resize(K);
        out->ev_off.resize(K + 1); out->read_off.resize(K + 1); out->err_off.resize(K + 1);
    } catch (const std::bad_alloc &) {
        return lc::fail(LC_E_NOMEM, "lc_counter_check_history: out of memory");
    }
    const uint32_t kblocks = (uint32_t)lcr::rp_blocks(K + 1);
    HIPCHK(hipMemsetAsync(a.err1, 0xFF, K * 8, stream));
    HIPCHK(hipMemsetAsync(a.err3, 0xFF, K * 8, stream));
    k_cp_classify<<<blocks, RP_BLOCK, 0, stream>>>(a);
    HIPCHK(hipGetLastError());
    LCCHK(lcr::rows_scan2(D.rows, stream, a.sc, n));
    k_cp_kstart<<<kblocks, RP_BLOCK, 0, stream>>>(a);
    k_cp_rule3<<<blocks, RP_BLOCK, 0, stream>>>(a);
    k_cp_flags<<<blocks, RP_BLOCK, 0, stream>>>(a);
    HIPCHK(hipGetLastError());
    LCCHK(lcr::rows_scan2(D.rows, stream, a.sc, n));
    k_cp_offsets<<<kblocks, RP_BLOCK, 0, stream>>>(a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(D.hout + 4, a.sc + n, 16, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(out->keys.data(), a.v.keys, K * 8, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(out->status.data(), a.status, K, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(out->error.data(), a.errw, K * 8, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(out->ev_off.data(), a.ev_off, (K + 1) * 8, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(out->read_off.data(), a.read_off, (K + 1) * 8, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));

    const uint64_t E = D.hout[4], R = D.hout[5];
    const uint64_t te = lcc::ct_tiles(E, tile), tr = lcc::ct_tiles(R, tile), tmax = std::max(te, tr);
    uint32_t *first_ev, *first_rd;
    char *tiles;
    int64_t *lower, *upper;
    unsigned long long *err_off, *err_idx;
    HIPCHK(lcx::grow(D.mem[PackDev::EV_KIND], a.ev_kind, (size_t)E));
    HIPCHK(lcx::grow(D.mem[PackDev::EV_VAL], a.ev_val, (size_t)E));
    HIPCHK(lcx::grow(D.mem[PackDev::READ_VAL], a.read_val, (size_t)R));
    HIPCHK(lcx::grow(D.mem[PackDev::LOWER], lower, (size_t)R));
    HIPCHK(lcx::grow(D.mem[PackDev::UPPER], upper, (size_t)R));
    HIPCHK(lcx::grow(D.mem[PackDev::FIRST_EV], first_ev, (size_t)te + 1));
    HIPCHK(lcx::grow(D.mem[PackDev::FIRST_RD], first_rd, (size_t)tr + 1));
    const size_t o_sb = align16(tmax * 8), o_ca = 2 * o_sb, o_cb = 3 * o_sb, o_hd = 4 * o_sb;
    HIPCHK(lcx::grow(D.mem[PackDev::TILES], tiles, o_hd + align16(tmax)));
    HIPCHK(lcx::grow(D.mem[PackDev::ERR_OFF], err_off, K + 1));
    HIPCHK(lcx::grow(D.mem[PackDev::ERR_IDX], err_idx, (size_t)R));
    try {
        out->lower.resize(R); out->upper.resize(R); out->read_val.resize(R);
    } catch (const std::bad_alloc &) {
        return lc::fail(LC_E_NOMEM, "lc_counter_check_history: out of memory");
    }
    if (E) {
        k_cp_scatter<<<blocks, RP_BLOCK, 0, stream>>>(a);
        k_cp_first<<<(uint32_t)lcr::rp_blocks(te + 1), RP_BLOCK, 0, stream>>>(a.ev_off, (uint32_t)K, tile, te, first_ev);
    }
    if (R) k_cp_first<<<(uint32_t)lcr::rp_blocks(tr + 1), RP_BLOCK, 0, stream>>>(a.read_off, (uint32_t)K, tile, tr, first_rd);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(D.ev[3], stream));
    HIPCHK(hipMemsetAsync(err_off, 0, (K + 1) * 8, stream));
    if (R) {
        HIPCHK(hipMemsetAsync(lower, 0, R * 8, stream));
        HIPCHK(hipMemsetAsync(upper, 0, R * 8, stream));
    }
    lcc::CtTiles ct{(unsigned long long *)tiles, (unsigned long long *)(tiles + o_sb), (unsigned long long *)(tiles + o_ca),
                    (unsigned long long *)(tiles + o_cb), (uint8_t *)(tiles + o_hd)};
    if (E) {
        lcc::CtEvents e{};
        e.s = lcc::CtSeries{(const uint64_t *)a.ev_off, first_ev, (int64_t)K, E, te};
        e.t = ct;
        e.kind = a.ev_kind; e.val = a.ev_val; e.lower = lower; e.upper = upper; e.R = R;
        e.err = (uint32_t *)(dout + 1);
        HIPCHK(lcc::counter_launch_events(stream, tile, e));
    }
    if (R) {
        lcc::CtJudge g{};
        g.s = lcc::CtSeries{(const uint64_t *)a.read_off, first_rd, (int64_t)K, R, tr};
        g.t = ct;
        g.val = a.read_val; g.lower = lower; g.upper = upper;
        g.err_off = err_off; g.err_idx = err_idx; g.err_cap = R; g.n_err = dout;
        HIPCHK(lcc::counter_launch_judge(stream, tile, g));
    }
    HIPCHK(hipEventRecord(D.ev[4], stream));
    HIPCHK(hipMemcpyAsync(D.hout, dout, 16, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(out->err_off.data(), err_off, (K + 1) * 8, hipMemcpyDeviceToHost, stream));
    if (R) {
        HIPCHK(hipMemcpyAsync(out->lower.data(), lower, R * 8, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipMemcpyAsync(out->upper.data(), upper, R * 8, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipMemcpyAsync(out->read_val.data(), a.read_val, R * 8, hipMemcpyDeviceToHost, stream));
    }
    HIPCHK(hipStreamSynchronize(stream));
    if ((uint32_t)D.hout[1]) return lc::fail(LC_E_DEVICE, "lc_counter_check_history: the batch built on the device is malformed");
    const uint64_t n_err = D.hout[0];
    try {
        out->err_idx.resize(n_err);
    } catch (const std::bad_alloc &) {
        return lc::fail(LC_E_NOMEM, "lc_counter_check_history: out of memory");
    }
    if (n_err) HIPCHK(hipMemcpyAsync(out->err_idx.data(), err_idx, n_err * 8, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipEventRecord(D.ev[5], stream));
    HIPCHK(hipStreamSynchronize(stream));
    out->n_keys = (int64_t)K; out->E = E; out->R = R; out->n_err = n_err;
    out->generation = D.generation;
    D.E = E;
    float ms = 0;
    for (int i = 0; i < 5; ++i) {
        HIPCHK(hipEventElapsedTime(&ms, D.ev[i], D.ev[i + 1]));
        D.ms[i] = ms;
    }
    D.ms[5] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    return LC_OK;
}

}  // namespace

int cp_dev_check(lc_ctx *c, const lc_counter_history *h, uint32_t tile, CpOut *out) {
    if (c->n_dev != 1 || c->comm)
        return lc::fail(LC_E_UNSUPPORTED, "lc_counter_check_history: needs a context of one device and no communicator");
    lcx::CtxCall x(c);
    LCCHK(x.enter());
    PackDev *D;
    LCCHK(pack_dev_of(x.d, &D));
    return check(*D, x.d->stream, h, tile, out);
}

int cp_dev_batch(lc_ctx *c, CpOut *out) {
    lcx::CtxCall x(c);
    LCCHK(x.enter());
    PackDev *D = (PackDev *)x.d->cpackdev;
    if (!D || D->generation != out->generation || D->E != out->E)
        return lc::fail(LC_E_INVALID, "lc_counter_checked_batch: not the context's latest lc_counter_check_history");
    const size_t E = (size_t)out->E;
    try {
        out->ev_kind.resize(E); out->ev_val.resize(E);
    } catch (const std::bad_alloc &) {
        return lc::fail(LC_E_NOMEM, "lc_counter_checked_batch: out of memory");
    }
    if (!E) return LC_OK;
    HIPCHK(hipMemcpyAsync(out->ev_kind.data(), D->mem[PackDev::EV_KIND].p, E, hipMemcpyDeviceToHost, x.d->stream));
    HIPCHK(hipMemcpyAsync(out->ev_val.data(), D->mem[PackDev::EV_VAL].p, E * 8, hipMemcpyDeviceToHost, x.d->stream));
    HIPCHK(hipStreamSynchronize(x.d->stream));
    return LC_OK;
}

int cp_dev_timing(lc_ctx *c, double *out6) {
    std::lock_guard<std::mutex> g(c->mu);
    const PackDev *D = (const PackDev *)c->dev[0]->cpackdev;
    for (int i = 0; i < 6; ++i) out6[i] = D ? D->ms[i] : 0.0;
    return LC_OK;
}

}  // namespace lccp
