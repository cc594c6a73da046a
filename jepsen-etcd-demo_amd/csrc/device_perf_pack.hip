// device_perf_pack.hip -- lc_perf_check_history's device half: a raw perf
// history becomes lc_perf_pack's batch in HBM, written straight into the record
// columns of lc_perf_check's device state, and device_perf.hip's kernels run on
// it where it lies (device_rows.hpp is the front end
// that pairs the rows).
//
// The batch is unkeyed: every row with a process takes part, and a POSITION is
// such a row's place in history order (device_rows.hpp).  One lane per row or
// per position in every kernel:
//   k_pp_takes     per row: has it a process; is it a record (a client row that
//                  is no :invoke) and is it a nemesis row (no process, f is
//                  f_start or f_stop) -- the pair of flags rows_scan2 turns into
//                  the record's number and the nemesis row's number; the lowest
//                  row with a bad :type / :f code; the largest :time of all rows
//   k_pp_nemesis   per row: a nemesis row's (f, time) to its number
//   k_pp_build     per position: a record is matched when its predecessor is an
//                  :invoke, and writes t_comp, t_inv and meta at its number; an
//                  :invoke is unmatched when its successor is none or an
//                  :invoke; the three counts, the four bounds and the lowest
//                  (completion row, invocation row) whose invocation's :time is
//                  the reserved INT64_MIN
// Nobody waits for anybody.  Counts and bounds are reduced in each wave, then
// across the workgroup's four waves in LDS, and leave with one atomic per
// workgroup and quantity, skipped when it would change nothing.  Ordering is by
// kernel boundaries on one stream.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>

#include "common.hpp"
#include "device_ctx.hpp"
#include "device_perf.hpp"
#include "device_perf_pack.hpp"
#include "device_rows.hpp"
#include "perf_plan.hpp"
#include "rows_plan.hpp"

namespace lcpp {

namespace {

typedef unsigned long long u64;
using lcr::RP_BLOCK;
using lcr::RP_NONE;

constexpr uint32_t WAVES = RP_BLOCK / 64;
constexpr u64 SIGN = 1ull << 63;  // t ^ SIGN keeps int64 order among unsigned words
constexpr u64 NO_WORD = ~0ull;

// The control words.  k_pp_build reduces words W_BUILD .. W_WORDS - 1 in this order: sums, then minima, then maxima.
enum { W_BAD, W_HMAX, W_BUILD, W_MATCHED = W_BUILD, W_UNMATCHED, W_ORPHANS, W_RESERVED, W_TMIN, W_XMIN, W_TMAX, W_XMAX, W_WORDS };
constexpr uint32_t N_SUM = 3, N_MIN = 3, N_MAX = 2, N_BUILD = N_SUM + N_MIN + N_MAX;
static_assert(W_BUILD + N_BUILD == W_WORDS, "control words");
// a bad code's word: the row, then which code (0 :type, 1 :f), then the f
__host__ __device__ inline u64 bad_word(u64 row, uint32_t is_f, uint32_t f) { return row << 16 | (u64)is_f << 8 | f; }

__device__ inline u64 wave_min(u64 v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const u64 o = __shfl_xor(v, d, 64);
        v = o < v ? o : v;
    }
    return v;
}

__device__ inline u64 wave_max(u64 v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const u64 o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

__device__ inline u64 wave_count(bool flag) { return (u64)__popcll(__ballot(flag)); }

__device__ inline void lower_word(u64 *w, u64 mine) {
    if (mine != NO_WORD && __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > mine) atomicMin(w, mine);
}

__device__ inline void raise_word(u64 *w, u64 mine) {
    if (mine != 0 && __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < mine) atomicMax(w, mine);
}

__global__ __launch_bounds__(RP_BLOCK) void k_pp_takes(const uint8_t *type, const uint8_t *f, const int64_t *process, const int64_t *time,
                                                      uint32_t n, int32_t n_f, int32_t f_start, int32_t f_stop, uint8_t *takes,
                                                      ulonglong2 *sc, u64 *words) {
    __shared__ u64 sh[2][WAVES];
    const u64 r = (u64)blockIdx.x * RP_BLOCK + threadIdx.x;
    u64 bad = NO_WORD, hmax = 0;
    if (r < n) {
        const uint8_t t = type[r], ff = f[r];
        const bool client = process[r] != LC_NO_PROCESS;
        takes[r] = client;
        const bool rec = client && t != LC_INVOKE;
        const bool nem = !client && ((int32_t)ff == f_start || (int32_t)ff == f_stop);
        sc[r] = make_ulonglong2(rec, nem);
        if (t > LC_INFO) bad = bad_word(r, 0, 0);
        else if ((int32_t)ff >= n_f) bad = bad_word(r, 1, ff);
        hmax = (u64)time[r] ^ SIGN;
    }
    bad = wave_min(bad);
    hmax = wave_max(hmax);
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
        sh[0][w] = bad;
        sh[1][w] = hmax;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 v = sh[0][0];
        for (uint32_t i = 1; i < WAVES; ++i) v = sh[0][i] < v ? sh[0][i] : v;
        lower_word(&words[W_BAD], v);
    } else if (threadIdx.x == 1) {
        u64 v = sh[1][0];
        for (uint32_t i = 1; i < WAVES; ++i) v = sh[1][i] > v ? sh[1][i] : v;
        raise_word(&words[W_HMAX], v);
    }
}

// sc: the exclusive scan of k_pp_takes' flags, [n] the totals.  nem: [2 x sc[n].y].
__global__ __launch_bounds__(RP_BLOCK) void k_pp_nemesis(const uint8_t *f, const int64_t *time, uint32_t n, const ulonglong2 *sc,
                                                        int64_t *nem) {
    const u64 r = (u64)blockIdx.x * RP_BLOCK + threadIdx.x;
    if (r >= n) return;
    const u64 at = sc[r].y;
    if (sc[r + 1].y == at) return;
    nem[2 * at] = (int64_t)f[r];
    nem[2 * at + 1] = time[r];
}

struct BuildArgs {
    lcr::RowsView v;
    const uint8_t *type, *f;
    const int64_t *time;
    const ulonglong2 *sc;  // [n + 1] per row: .x the number of the records before it
    u64 n_rec;
    int64_t *t_comp, *t_inv;  // [n_rec]
    uint32_t *meta;
    u64 *words;
};

__global__ __launch_bounds__(RP_BLOCK) void k_pp_build(BuildArgs a) {
    __shared__ u64 sh[N_BUILD][WAVES];
    const u64 j = (u64)blockIdx.x * RP_BLOCK + threadIdx.x;
    bool matched = false, unmatched = false, orphan = false;
    u64 reserved = NO_WORD, tmin = NO_WORD, xmin = NO_WORD, tmax = 0, xmax = 0;
    if (j < a.v.n && a.v.pos_key[j] != a.v.n_keys) {
        const uint32_t r = a.v.pos_row[j];
        const uint8_t t = a.type[r];
        if (t == LC_INVOKE) {
            const uint32_t nj = a.v.next[j];
            unmatched = nj == RP_NONE || a.type[a.v.pos_row[nj]] == LC_INVOKE;
        } else {
            const uint32_t pj = a.v.prev[j];
            const uint32_t rp = pj != RP_NONE ? a.v.pos_row[pj] : r;
            matched = pj != RP_NONE && a.type[rp] == LC_INVOKE;
            orphan = !matched;
            const uint8_t ff = a.f[r];
            const int64_t tc = a.time[r];
            int64_t ti = LC_PERF_NO_INVOKE;
            uint32_t f_inv = ff;
            if (matched) {
                ti = a.time[rp];
                f_inv = a.f[rp];
                if (ti == LC_PERF_NO_INVOKE) reserved = (u64)r << 32 | rp;
                xmin = xmax = (u64)ti ^ SIGN;
            }
            tmin = tmax = (u64)tc ^ SIGN;
            const u64 at = a.sc[r].x;
            if (at < a.n_rec) {
                a.t_comp[at] = tc;
                a.t_inv[at] = ti;
                a.meta[at] = LC_PERF_META(f_inv, ff, t);
            }
        }
    }
    const u64 c0 = wave_count(matched), c1 = wave_count(unmatched), c2 = wave_count(orphan);
    reserved = wave_min(reserved);
    tmin = wave_min(tmin);
    xmin = wave_min(xmin);
    tmax = wave_max(tmax);
    xmax = wave_max(xmax);
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {  // (the order of the control words)
        sh[0][w] = c0; sh[1][w] = c1; sh[2][w] = c2;
        sh[3][w] = reserved; sh[4][w] = tmin; sh[5][w] = xmin;
        sh[6][w] = tmax; sh[7][w] = xmax;
    }
    __syncthreads();
    const uint32_t q = threadIdx.x;
    if (q >= N_BUILD) return;
    u64 v = sh[q][0];
    for (uint32_t i = 1; i < WAVES; ++i) {
        const u64 o = sh[q][i];
        v = q < N_SUM ? v + o : q < N_SUM + N_MIN ? (o < v ? o : v) : (o > v ? o : v);
    }
    u64 *word = &a.words[W_BUILD + q];
    if (q < N_SUM) {
        if (v) atomicAdd(word, v);
    } else if (q < N_SUM + N_MIN) {
        lower_word(word, v);
    } else {
        raise_word(word, v);
    }
}

struct PackDev {
    enum { TYPE, F, PROC, TIME, TAKES, SC, NEM, WORDS, N_MEM };
    lcx::DevBatch::Mem mem[N_MEM];
    lcr::Rows *rows = nullptr;
    char *hstage = nullptr;  // pinned staging of the columns of a caller whose arrays are not page-locked
    size_t hstage_cap = 0;
    unsigned long long *hout = nullptr;  // pinned landing: the control words, then the scan's two totals
    size_t hout_cap = 0;
    int64_t *hnem = nullptr;  // pinned landing of the nemesis rows
    size_t hnem_cap = 0;
    hipEvent_t ev[4] = {};
    double ms[6] = {0, 0, 0, 0, 0, 0};
    ~PackDev() {
        lcr::rows_close(rows);
        for (lcx::DevBatch::Mem &m : mem)
            if (m.p) (void)hipFree(m.p);
        if (hstage) (void)hipHostFree(hstage);
        if (hout) (void)hipHostFree(hout);
        if (hnem) (void)hipHostFree(hnem);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

void pack_dev_free(void *p) { delete (PackDev *)p; }

int pack_dev_of(lcx::Dev *d, PackDev **out) {
    if (!d->ppackdev) {
        PackDev *D = new (std::nothrow) PackDev();
        if (!D) return lc::fail(LC_E_NOMEM, "lc_perf_check_history: out of memory");
        if (int rc = lcr::rows_open(&D->rows)) {
            delete D;
            return rc;
        }
        d->ppackdev = D;
        d->ppackdev_free = pack_dev_free;
    }
    *out = (PackDev *)d->ppackdev;
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

int64_t unbiased(u64 w) { return (int64_t)(w ^ SIGN); }

int check(PackDev &D, lcx::Dev *d, const lc_perf_history *h, const lc_perf_opts *o, PpOut *out) {
    const auto wall0 = std::chrono::steady_clock::now();
    hipStream_t stream = d->stream;
    const size_t n = (size_t)h->n;
    const uint32_t blocks = (uint32_t)lcr::rp_blocks(n);
    for (hipEvent_t &e : D.ev)
        if (!e) HIPCHK(hipEventCreate(&e));
    uint8_t *type, *f, *takes;
    int64_t *proc, *time;
    ulonglong2 *sc;
    u64 *words;
    HIPCHK(lcx::grow(D.mem[PackDev::TYPE], type, n));
    HIPCHK(lcx::grow(D.mem[PackDev::F], f, n));
    HIPCHK(lcx::grow(D.mem[PackDev::PROC], proc, n));
    HIPCHK(lcx::grow(D.mem[PackDev::TIME], time, n));
    HIPCHK(lcx::grow(D.mem[PackDev::TAKES], takes, n));
    HIPCHK(lcx::grow(D.mem[PackDev::SC], sc, n + 1));
    HIPCHK(lcx::grow(D.mem[PackDev::WORDS], words, (size_t)W_WORDS));
    HIPCHK(lcx::grow_pinned(D.hout, D.hout_cap, (size_t)W_WORDS + 2));
    const size_t s_f = align16(n), s_proc = s_f + align16(n), s_time = s_proc + n * 8;
    HIPCHK(lcx::grow_pinned(D.hstage, D.hstage_cap, s_time + n * 8));

    HIPCHK(hipEventRecord(D.ev[0], stream));
    LCCHK(upload(stream, type, h->type, n, D.hstage));
    LCCHK(upload(stream, f, h->f, n, D.hstage + s_f));
    LCCHK(upload(stream, proc, h->process, n * 8, D.hstage + s_proc));
    LCCHK(upload(stream, time, h->time, n * 8, D.hstage + s_time));
    HIPCHK(hipEventRecord(D.ev[1], stream));
    HIPCHK(hipMemsetAsync(words, 0, W_WORDS * 8, stream));
    HIPCHK(hipMemsetAsync(words + W_BAD, 0xFF, 8, stream));
    HIPCHK(hipMemsetAsync(words + W_RESERVED, 0xFF, N_MIN * 8, stream));
    k_pp_takes<<<blocks, RP_BLOCK, 0, stream>>>(type, f, proc, time, (uint32_t)n, h->n_f, h->f_start, h->f_stop, takes, sc, words);
    HIPCHK(hipGetLastError());
    LCCHK(lcr::rows_scan2(D.rows, stream, sc, n));
    HIPCHK(hipMemcpyAsync(D.hout, words, 2 * 8, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(D.hout + W_WORDS, sc + n, 16, hipMemcpyDeviceToHost, stream));
    uint64_t n_keys = 0, n_procs = 0;
    LCCHK(lcr::rows_group(D.rows, stream, lcr::RowsIn{(uint32_t)n, takes, proc, nullptr}, &n_keys, &n_procs));  // (synchronises)
    if (D.hout[W_BAD] != NO_WORD) {
        const u64 w = D.hout[W_BAD];
        const long long row = (long long)(w >> 16);
        if (!(w >> 8 & 1)) return lc::fail(LC_E_INVALID, "lc_perf_check_history: row %lld: bad :type code", row);
        return lc::fail(LC_E_INVALID, "lc_perf_check_history: row %lld: f %u is not below n_f %d", row, (unsigned)(w & 0xFF), h->n_f);
    }
    const uint64_t n_rec = D.hout[W_WORDS], n_nem = D.hout[W_WORDS + 1];
    if (n_rec > n || n_nem > n) return lc::fail(LC_E_DEVICE, "lc_perf_check_history: the scan's totals pass the row count");
    BuildArgs a{};
    LCCHK(lcr::rows_pair(D.rows, stream, &a.v));
    HIPCHK(hipEventRecord(D.ev[2], stream));

    a.type = type; a.f = f; a.time = time; a.sc = sc; a.n_rec = n_rec; a.words = words;
    LCCHK(lcp::perf_records_device(&d->perfdev, n_rec, &a.t_comp, &a.t_inv, &a.meta));
    int64_t *nem;
    HIPCHK(lcx::grow(D.mem[PackDev::NEM], nem, (size_t)n_nem * 2));
    HIPCHK(lcx::grow_pinned(D.hnem, D.hnem_cap, std::max<size_t>((size_t)n_nem * 2, 2)));
    if (n_nem) k_pp_nemesis<<<blocks, RP_BLOCK, 0, stream>>>(f, time, (uint32_t)n, sc, nem);
    k_pp_build<<<blocks, RP_BLOCK, 0, stream>>>(a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(D.ev[3], stream));
    HIPCHK(hipMemcpyAsync(D.hout, words, W_WORDS * 8, hipMemcpyDeviceToHost, stream));
    if (n_nem) HIPCHK(hipMemcpyAsync(D.hnem, nem, n_nem * 16, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));

    const unsigned long long *w = D.hout;
    if (w[W_RESERVED] != NO_WORD)
        return lc::fail(LC_E_INVALID, "lc_perf_check_history: row %lld: :time INT64_MIN is reserved", (long long)(w[W_RESERVED] & 0xFFFFFFFFull));
    out->n_rec = (int64_t)n_rec;
    out->matched = (int64_t)w[W_MATCHED]; out->unmatched = (int64_t)w[W_UNMATCHED]; out->orphans = (int64_t)w[W_ORPHANS];
    if (w[W_MATCHED] + w[W_ORPHANS] != n_rec)
        return lc::fail(LC_E_DEVICE, "lc_perf_check_history: %llu matched and %llu orphans, %llu records", w[W_MATCHED], w[W_ORPHANS],
                        (unsigned long long)n_rec);
    out->t_min = n_rec ? unbiased(w[W_TMIN]) : 0;
    out->t_max = n_rec ? unbiased(w[W_TMAX]) : 0;
    out->x_min = out->matched ? unbiased(w[W_XMIN]) : 0;
    out->x_max = out->matched ? unbiased(w[W_XMAX]) : 0;
    out->hist_max = unbiased(w[W_HMAX]);
    out->nem.assign(D.hnem, D.hnem + n_nem * 2);

    lc_perf_batch sizes{};
    sizes.n = out->n_rec; sizes.n_matched = out->matched;
    sizes.t_min = out->t_min; sizes.t_max = out->t_max; sizes.x_min = out->x_min; sizes.x_max = out->x_max;
    sizes.n_f = h->n_f;
    LCCHK(lcp::perf_opts_check(&sizes, o, out->shape));
    const uint64_t F = (uint64_t)h->n_f, R = F * 3 * (uint64_t)out->shape[1], G = F * (uint64_t)out->shape[3];
    out->rate.assign(R, 0); out->group.assign(G, 0); out->quant.assign(G * (uint64_t)o->n_q, 0);
    lc_perf_result r{};
    r.rate = out->rate.data(); r.group = out->group.data(); r.quant = out->quant.data();
    r.rate_cap = R; r.group_cap = G; r.quant_cap = G * (uint64_t)o->n_q;
    LCCHK(lcp::perf_check_device(&d->perfdev, stream, &sizes, o, &r));
    out->generation = lcp::perf_generation(d->perfdev);

    float ms = 0;
    for (int i = 0; i < 3; ++i) {
        HIPCHK(hipEventElapsedTime(&ms, D.ev[i], D.ev[i + 1]));
        D.ms[i] = ms;
    }
    double perf_ms[4] = {0, 0, 0, 0};
    if (n_rec) lcp::perf_last_timing(d->perfdev, perf_ms);
    D.ms[3] = perf_ms[1];
    D.ms[4] = perf_ms[2];
    D.ms[5] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    return LC_OK;
}

}  // namespace

int pp_dev_check(lc_ctx *c, const lc_perf_history *h, const lc_perf_opts *o, PpOut *out) {
    if (c->n_dev != 1 || c->comm)
        return lc::fail(LC_E_UNSUPPORTED, "lc_perf_check_history: needs a context of one device and no communicator");
    lcx::CtxCall x(c);
    LCCHK(x.enter());
    PackDev *D;
    LCCHK(pack_dev_of(x.d, &D));
    return check(*D, x.d, h, o, out);
}

int pp_dev_records(lc_ctx *c, PpOut *out) {
    lcx::CtxCall x(c);
    LCCHK(x.enter());
    if (!x.d->perfdev || lcp::perf_generation(x.d->perfdev) != out->generation)
        return lc::fail(LC_E_INVALID, "lc_perf_checked_records: not the context's latest lc_perf_check_history");
    const size_t n = (size_t)out->n_rec;
    out->t_comp.resize(n); out->t_inv.resize(n); out->meta.resize(n);
    return lcp::perf_records_download(x.d->perfdev, x.d->stream, n, out->t_comp.data(), out->t_inv.data(), out->meta.data());
}

int pp_dev_timing(lc_ctx *c, double *out6) {
    std::lock_guard<std::mutex> g(c->mu);
    const PackDev *D = (const PackDev *)c->dev[0]->ppackdev;
    for (int i = 0; i < 6; ++i) out6[i] = D ? D->ms[i] : 0.0;
    return LC_OK;
}

}  // namespace lcpp
