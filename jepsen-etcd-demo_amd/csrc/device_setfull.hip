// device_setfull.hip -- jepsen.checker/set-full on the device: the kernels and
// the step that runs them (lc_setfull_check; include/lincheck.h has the
// semantics, restated from memory of the public Jepsen 0.2.x source; parity
// unpinned).
//
// Per key a PRESENCE MATRIX: one row per :ok :read in completion order, one
// bit per element id.  Jepsen's fold updates every tracked element at every
// read; here every element looks at its own column of the matrix instead.
// An element invoked at position I sees the rows that completed after I --
// a suffix of the rows -- and needs of them
//     last-present  the largest invocation position among the rows holding it
//     last-absent   the largest one among the rows missing it
//     known         the first of: its :ok :add, the first such row holding it
// from which outcome and latency follow with integer arithmetic.
//
// Kernels (csrc/setfull_plan.hpp lays the keys into passes and bands):
//   k_setfull_mark    read lists to bits.  One workgroup per (band, row, 4,096
//                     read elements), 16-byte loads of ids.  When the
//                     workgroup's ids span no more than its LDS tile (8,192
//                     ids) they are marked there (ds_or) and the tile's
//                     nonzero words leave with one atomicOr each; otherwise,
//                     and under LC_SETFULL_MARK_DIRECT, each lane merges the
//                     bits that fall into one 32-bit word and issues its own
//                     atomics.  A bit that is already set when the same row
//                     marks it again flags the id as duplicated.  An id at or
//                     past the key's span marks nothing and names its key in
//                     the error word (the call returns LC_E_INVALID); an id
//                     outside the band is another band's.
//   k_setfull_scan    one wave per 64 consecutive ids (one matrix word per
//                     row), one lane per id.  All 64 lanes read the same word
//                     of a row, so the row loops issue wave-uniform loads and
//                     each lane tests its own bit.  Down from the newest row:
//                     last-present / last-absent, each settled once a row's
//                     completion position is below the invocation position it
//                     holds (rows are in completion order and a read is
//                     invoked before it completes: no older row was invoked
//                     later).  Both must be exact -- last-absent's time is the
//                     stable latency, last-present's the lost latency -- so a
//                     lane is done when both are settled or its first
//                     eligible row is passed, and the wave's loop ends when
//                     every lane is done.  Then up from the first eligible
//                     row to the first one present, stopping at the add's :ok.
//   k_setfull_finish  one workgroup per key: the key's counts summed over its
//                     scan workgroups' own six sums (no atomics: section 3.9's
//                     note on per-wave adds), then :valid?.
// Ordering is by kernel boundaries on one stream; nothing spins.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "device_setfull.hpp"
#include "setfull_plan.hpp"

#define HIPCHK(expr)                                                                       \
    do {                                                                                   \
        hipError_t _e = (expr);                                                            \
        if (_e != hipSuccess)                                                              \
            return lc::fail(LC_E_DEVICE, "%s failed: %s", #expr, hipGetErrorString(_e));  \
    } while (0)

namespace lcf {

namespace {

struct SfArgs {
    const SfSeg *segs;
    const uint64_t *id_off;     // [n_keys + 1]
    const uint64_t *row_off;    // [n_keys + 1]
    const uint32_t *span;
    const uint8_t *status;
    const uint32_t *item_base;  // [n_keys + 1]
    const int64_t *inv_pos, *ack_pos, *ack_time;                  // per id
    const int64_t *row_pos, *row_time, *row_inv_pos, *row_inv_time;  // per row
    const uint64_t *el_off;
    const uint32_t *read_id;
    uint64_t *mat;              // the pass's matrix
    uint32_t *part;             // [6 * n_items] each scan workgroup's own six counts
    uint8_t *outcome, *dup;     // per id
    int64_t *latency, *known, *last_absent;
    unsigned long long *counts; // [6 * n_keys]
    int8_t *valid;
    int32_t *err;               // 1 + a key with a bad id, or 0
    uint32_t direct;            // LC_SETFULL_MARK_DIRECT
    uint32_t linearizable;
};

// The ids of `bits` of 32-bit word w of a band are duplicated.
__device__ inline void flag_dups(uint8_t *dup, uint32_t lo, uint32_t w, uint32_t bits) {
    while (bits) {
        const int b = __ffs((int)bits) - 1;
        bits &= bits - 1;
        dup[lo + 32u * w + (uint32_t)b] = 1;
    }
}

__global__ __launch_bounds__(SF_BLOCK) void k_setfull_mark(SfArgs a, const SfMarkItem *items) {
    const SfMarkItem it = items[blockIdx.x];
    const SfSeg sg = a.segs[it.seg];
    const uint32_t k = sg.key, span = a.span[k];
    const uint64_t row_b = a.el_off[it.row], row_e = a.el_off[it.row + 1];
    const uint64_t r0 = it.start + (uint64_t)threadIdx.x * SF_MARK_LANE_ELS;
    uint32_t *M = reinterpret_cast<uint32_t *>(a.mat + sg.mbase + (it.row - a.row_off[k]) * (uint64_t)sg.bw);
    uint8_t *dup = a.dup + a.id_off[k];
    // the lane's elements, read once: 16-byte loads (r0 is a multiple of four; the array is padded past its end)
    uint32_t ids[SF_MARK_LANE_ELS];
#pragma unroll
    for (uint32_t q = 0; q < SF_MARK_LANE_ELS / 4; ++q) {
        const uint64_t at = r0 + 4 * q;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (at < row_e && at + 4 > row_b) v = *reinterpret_cast<const uint4 *>(a.read_id + at);
        ids[4 * q] = v.x; ids[4 * q + 1] = v.y; ids[4 * q + 2] = v.z; ids[4 * q + 3] = v.w;
    }
    // which of them are the row's, and of those which are this band's (rel: the id inside the band)
    uint32_t mine = 0;
    bool bad = false;
#pragma unroll
    for (uint32_t j = 0; j < SF_MARK_LANE_ELS; ++j) {
        const uint64_t at = r0 + j;
        if (at < row_b || at >= row_e) continue;
        if (ids[j] >= span) {
            bad = true;
            continue;
        }
        ids[j] -= sg.lo;  // (wraps above n_ids for an id below the band)
        if (ids[j] < sg.n_ids) mine |= 1u << j;
    }
    if (bad) atomicMax(a.err, (int32_t)k + 1);
    // the tile form: the workgroup's ids within SF_MARK_TILE_WORDS words of their least one
    __shared__ uint32_t tile[SF_MARK_TILE_WORDS];
    __shared__ uint32_t red[2][SF_BLOCK / 64];
    bool tiled = false;
    uint32_t lo = 0;
    if (!a.direct) {
        uint32_t mn = 0xFFFFFFFFu, mx = 0;
#pragma unroll
        for (uint32_t j = 0; j < SF_MARK_LANE_ELS; ++j)
            if (mine >> j & 1) {
                mn = min(mn, ids[j]);
                mx = max(mx, ids[j]);
            }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            mn = min(mn, (uint32_t)__shfl_xor(mn, d, 64));
            mx = max(mx, (uint32_t)__shfl_xor(mx, d, 64));
        }
        if ((threadIdx.x & 63) == 0) {
            red[0][threadIdx.x >> 6] = mn;
            red[1][threadIdx.x >> 6] = mx;
        }
        tile[threadIdx.x] = 0;
        __syncthreads();
#pragma unroll
        for (uint32_t w = 0; w < SF_BLOCK / 64; ++w) {
            mn = min(mn, red[0][w]);
            mx = max(mx, red[1][w]);
        }
        lo = mn >> 5;
        tiled = mn <= mx && (mx >> 5) - lo < SF_MARK_TILE_WORDS;  // the same in every lane
    }
    // the lanes' own atomics: the bits of consecutive elements that share a 32-bit word leave in one
    uint32_t w1 = 0, m1 = 0;
#pragma unroll
    for (uint32_t j = 0; j < SF_MARK_LANE_ELS; ++j) {
        if (!(mine >> j & 1)) continue;
        const uint32_t rel = ids[j], w = rel >> 5, bit = 1u << (rel & 31);
        if (tiled) {
            if (atomicOr(&tile[w - lo], bit) & bit) dup[sg.lo + rel] = 1;
            continue;
        }
        if (w != w1 && m1) {
            flag_dups(dup, sg.lo, w1, atomicOr(M + w1, m1) & m1);
            m1 = 0;
        }
        w1 = w;
        if (m1 & bit) dup[sg.lo + rel] = 1;
        m1 |= bit;
    }
    if (m1) flag_dups(dup, sg.lo, w1, atomicOr(M + w1, m1) & m1);
    if (tiled) {
        __syncthreads();
        const uint32_t t = tile[threadIdx.x];
        if (t) flag_dups(dup, sg.lo, lo + threadIdx.x, atomicOr(M + lo + threadIdx.x, t) & t);
    }
}

// The workgroup's sum of each of six counters, in every thread.
__device__ inline void block_sum6(const uint32_t v[6], uint64_t out[6], uint64_t (*sh)[6]) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        unsigned long long x = v[i];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) x += __shfl_down(x, d, 64);
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6][i] = x;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 6; ++i) out[i] = sh[0][i] + sh[1][i] + sh[2][i] + sh[3][i];
    __syncthreads();
}

__global__ __launch_bounds__(SF_BLOCK) void k_setfull_scan(SfArgs a, const SfScanItem *items) {
    __shared__ uint64_t s6[SF_BLOCK / 64][6];
    const SfScanItem it = items[blockIdx.x];
    const SfSeg sg = a.segs[it.seg];
    const uint32_t k = sg.key, tid = threadIdx.x, lane = tid & 63;
    const uint32_t rel = it.chunk * SF_BLOCK_IDS + tid;
    const bool have = rel < sg.n_ids;
    const uint64_t g = a.id_off[k] + sg.lo + (have ? rel : 0u);
    const uint64_t R0 = a.row_off[k];
    const int64_t R = (int64_t)(a.row_off[k + 1] - R0);
    const int64_t *row_pos = a.row_pos + R0, *row_time = a.row_time + R0;
    const int64_t *row_inv = a.row_inv_pos + R0, *row_inv_time = a.row_inv_time + R0;
    const int64_t I = have ? a.inv_pos[g] : (int64_t)LC_SETFULL_NONE;
    const bool tracked = I >= 0;
    const int64_t A = tracked ? a.ack_pos[g] : (int64_t)LC_SETFULL_NONE;
    // the first eligible row: the first one that completed after the add's invocation
    int64_t fe = R;
    if (tracked) {
        int64_t b = 0, e = R;
        while (b < e) {
            const int64_t m = b + (e - b) / 2;
            if (row_pos[m] > I) e = m;
            else b = m + 1;
        }
        fe = b;
    }
    int64_t fe_min = fe;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int64_t other = (int64_t)__shfl_xor((long long)fe_min, d, 64);
        fe_min = other < fe_min ? other : fe_min;
    }
    // the wave's word of every row (the same in all 64 lanes)
    const uint32_t wv = __builtin_amdgcn_readfirstlane(it.chunk * SF_BLOCK_WORDS + (tid >> 6));
    const uint64_t *W = a.mat + sg.mbase + wv;
    const uint64_t bw = sg.bw;
    // down: last-present and last-absent
    int64_t lp = LC_SETFULL_NONE, la = LC_SETFULL_NONE, lpt = 0, lat = 0;
    bool done = fe >= R;
    for (int64_t r = R - 1; r >= fe_min; --r) {
        if (__all(done)) break;
        const int64_t c = row_pos[r], i = row_inv[r], t = row_inv_time[r];
        const uint64_t w = W[(uint64_t)r * bw];
        if (done) continue;
        if (r < fe || (lp >= 0 && la >= 0 && c < (lp < la ? lp : la))) {
            done = true;
        } else if (w >> lane & 1) {
            if (i > lp) { lp = i; lpt = t; }
        } else {
            if (i > la) { la = i; lat = t; }
        }
    }
    // up: known, when some eligible row holds the element at all
    int64_t kp = LC_SETFULL_NONE, kt = 0;
    bool kdone = lp < 0;
    for (int64_t r = fe_min; r < R; ++r) {
        if (__all(kdone)) break;
        const int64_t c = row_pos[r], t = row_time[r];
        const uint64_t w = W[(uint64_t)r * bw];
        if (kdone || r < fe) continue;
        if (A >= 0 && c > A) {
            kdone = true;  // the :ok :add came first
        } else if (w >> lane & 1) {
            kp = c;
            kt = t;
            kdone = true;
        }
    }
    if (kp < 0 && A >= 0) {
        kp = A;
        kt = a.ack_time[g];
    }
    const bool stable = lp >= 0 && la < lp;
    const bool lost = !stable && kp >= 0 && la >= 0 && lp < la && kp < la;
    const int64_t until = stable ? (la >= 0 ? lat + 1 : 0) : (lp >= 0 ? lpt + 1 : 0);
    int64_t ms = LC_SETFULL_NONE;
    if (stable || lost) ms = (until > kt ? until - kt : 0) / 1000000;
    uint32_t v[6] = {0, 0, 0, 0, 0, 0};
    if (have) {
        a.outcome[g] = !tracked ? LC_SETFULL_UNTRACKED : stable ? LC_SETFULL_STABLE : lost ? LC_SETFULL_LOST : LC_SETFULL_NEVER_READ;
        a.latency[g] = ms;
        a.known[g] = kp;
        a.last_absent[g] = la;
        v[0] = tracked;
        v[1] = stable;
        v[2] = lost;
        v[3] = tracked && !stable && !lost;
        v[4] = stable && ms > 0;
        v[5] = a.dup[g] != 0;
    }
    uint64_t tot[6];
    block_sum6(v, tot, s6);
    const uint64_t slot = (uint64_t)a.item_base[k] + sg.lo / SF_BLOCK_IDS + it.chunk;
    if (tid < 6) a.part[6 * slot + tid] = (uint32_t)tot[tid];
}

__global__ __launch_bounds__(SF_BLOCK) void k_setfull_finish(SfArgs a) {
    __shared__ uint64_t s6[SF_BLOCK / 64][6];
    const uint32_t k = blockIdx.x;
    const bool checked = a.status[k] == LC_SET_KEY_OK;
    uint32_t acc[6] = {0, 0, 0, 0, 0, 0};
    uint64_t tot[6] = {0, 0, 0, 0, 0, 0};
    if (checked) {
        // (a slot holds at most SF_BLOCK_IDS; a thread's share of 2^32 ids fits 32 bits)
        for (uint64_t j = (uint64_t)a.item_base[k] + threadIdx.x; j < a.item_base[k + 1]; j += SF_BLOCK)
#pragma unroll
            for (int i = 0; i < 6; ++i) acc[i] += a.part[6 * j + i];
    }
    block_sum6(acc, tot, s6);
    if (threadIdx.x < 6) a.counts[6ull * k + threadIdx.x] = tot[threadIdx.x];
    if (threadIdx.x == 0) {
        int8_t v = LC_VALID;
        if (!checked) v = LC_UNKNOWN;
        else if (tot[2]) v = LC_INVALID;
        else if (!tot[1]) v = LC_UNKNOWN;
        else if (a.linearizable && tot[4]) v = LC_INVALID;
        if (checked && tot[5]) v = LC_INVALID;
        a.valid[k] = v;
    }
}

struct Buf {
    void *p = nullptr;
    size_t cap = 0;
    hipError_t grow(size_t bytes) {
        bytes = std::max<size_t>(bytes, 256);
        if (bytes <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        hipError_t e = hipMalloc(&p, bytes + bytes / 4);
        if (e == hipSuccess) cap = bytes + bytes / 4;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};
struct HostBuf {
    char *p = nullptr;
    size_t cap = 0;
    hipError_t grow(size_t bytes) {
        bytes = std::max<size_t>(bytes, 256);
        if (bytes <= cap) return hipSuccess;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        hipError_t e = hipHostMalloc((void **)&p, bytes + bytes / 4, hipHostMallocDefault);
        if (e == hipSuccess) cap = bytes + bytes / 4;
        return e;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
};

// Sections of a block, each 16-byte aligned.
struct Layout {
    size_t at = 0;
    size_t take(size_t bytes) {
        const size_t o = at;
        at += (bytes + 15) & ~(size_t)15;
        return o;
    }
};

}  // namespace

struct SetFullDev {
    Buf meta, ids, rows, el_off, read_id, mat, part, out;
    HostBuf hmeta, hout;
    std::vector<hipEvent_t> ev;  // 3 fixed, then 3 per pass
    double ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

void setfull_dev_free(SetFullDev *d) {
    if (!d) return;
    for (Buf *b : {&d->meta, &d->ids, &d->rows, &d->el_off, &d->read_id, &d->mat, &d->part, &d->out}) b->release();
    d->hmeta.release();
    d->hout.release();
    for (hipEvent_t e : d->ev)
        if (e) (void)hipEventDestroy(e);
    delete d;
}

int setfull_last_timing(const SetFullDev *d, double *out8) {
    for (int i = 0; i < 8; ++i) out8[i] = d ? d->ms[i] : 0.0;
    return LC_OK;
}

// The offset arrays of a batch (a caller may have built it) and the rows'
// order, which the scan's suffix rule and stop rule rest on.  The ids
// themselves are the mark kernel's to check.
static int validate(const lc_setfull_batch *b) {
    const int64_t K = b->n_keys;
    if (K < 0 || K > 0x7FFFFFF0) return lc::fail(LC_E_INVALID, "lc_setfull_check: n_keys %lld", (long long)K);
    if (K == 0) return LC_OK;
    if (!b->id_off || !b->span || !b->row_off) return lc::fail(LC_E_INVALID, "lc_setfull_check: null per-key array");
    if (b->id_off[0] != 0 || b->row_off[0] != 0) return lc::fail(LC_E_INVALID, "lc_setfull_check: offsets do not start at 0");
    for (int64_t k = 0; k < K; ++k) {
        if (b->id_off[k + 1] < b->id_off[k] || b->row_off[k + 1] < b->row_off[k])
            return lc::fail(LC_E_INVALID, "lc_setfull_check: key %lld: offsets not ascending", (long long)k);
        const uint8_t st = b->status ? b->status[k] : (uint8_t)LC_SET_KEY_OK;
        if (st != LC_SET_KEY_OK && st != LC_SET_KEY_ERROR) return lc::fail(LC_E_INVALID, "lc_setfull_check: key %lld: bad status code", (long long)k);
        if (st != LC_SET_KEY_OK) continue;
        if (b->span[k] > SF_MAX_SPAN) return lc::fail(LC_E_INVALID, "lc_setfull_check: key %lld: span above 2^32 - 64", (long long)k);
        if (b->id_off[k + 1] - b->id_off[k] < b->span[k])
            return lc::fail(LC_E_INVALID, "lc_setfull_check: key %lld: fewer per-id entries than its span", (long long)k);
        if (b->row_off[k + 1] - b->row_off[k] > 0x7FFFFFF0ull) return lc::fail(LC_E_INVALID, "lc_setfull_check: key %lld: more than 2^31 reads", (long long)k);
    }
    const uint64_t n_ids = b->id_off[K], n_rows = b->row_off[K];
    if (n_ids && (!b->inv_pos || !b->ack_pos || !b->ack_time)) return lc::fail(LC_E_INVALID, "lc_setfull_check: null per-id array");
    if (n_rows && (!b->row_pos || !b->row_time || !b->row_inv_pos || !b->row_inv_time || !b->el_off))
        return lc::fail(LC_E_INVALID, "lc_setfull_check: null per-row array");
    if (n_rows) {
        if (b->el_off[0] != 0) return lc::fail(LC_E_INVALID, "lc_setfull_check: el_off[0] is not 0");
        for (uint64_t r = 0; r < n_rows; ++r)
            if (b->el_off[r + 1] < b->el_off[r]) return lc::fail(LC_E_INVALID, "lc_setfull_check: el_off not ascending at row %llu", (unsigned long long)r);
        if (b->el_off[n_rows] && !b->read_id) return lc::fail(LC_E_INVALID, "lc_setfull_check: null read_id");
        for (int64_t k = 0; k < K; ++k)
            for (uint64_t r = b->row_off[k]; r < b->row_off[k + 1]; ++r)
                if (b->row_pos[r] < 0 || b->row_inv_pos[r] < 0 || b->row_inv_pos[r] >= b->row_pos[r] ||
                    (r > b->row_off[k] && b->row_pos[r] <= b->row_pos[r - 1]))
                    return lc::fail(LC_E_INVALID, "lc_setfull_check: key %lld: reads not in completion order, or one invoked after it completed",
                                    (long long)k);
    }
    return LC_OK;
}

int setfull_check(SetFullDev **dev, hipStream_t stream, const lc_setfull_batch *b, const lc_setfull_opts *o,
                  lc_setfull_result *r) {
    lc::Range range("lc_setfull_check");
    const auto wall0 = std::chrono::steady_clock::now();
    if (int rc = validate(b)) return rc;
    if (o->flags & ~LC_SETFULL_MARK_DIRECT) return lc::fail(LC_E_INVALID, "lc_setfull_check: unknown flags 0x%x", o->flags);
    const int64_t K = b->n_keys;
    if (K == 0) return LC_OK;
    const size_t nk = (size_t)K;
    const uint64_t n_ids = b->id_off[K], n_rows = b->row_off[K], n_el = n_rows ? b->el_off[n_rows] : 0;
    if (!r->valid || !r->counts) return lc::fail(LC_E_INVALID, "lc_setfull_check: null result array");
    if (n_ids && (!r->outcome || !r->latency || !r->known || !r->last_absent || !r->duplicated))
        return lc::fail(LC_E_INVALID, "lc_setfull_check: null per-id result array");
    if (!*dev) {
        *dev = new (std::nothrow) SetFullDev();
        if (!*dev) return lc::fail(LC_E_NOMEM, "lc_setfull_check: out of memory");
    }
    SetFullDev &D = **dev;

    SfStepIn in;
    in.n_keys = K; in.span = b->span; in.status = b->status; in.row_off = b->row_off; in.el_off = b->el_off;
    in.cap_bytes = o->max_matrix_bytes ? o->max_matrix_bytes : SF_MATRIX_MAX_BYTES;
    SfStepPlan plan;
    try {
        plan = plan_setfull_step(in);
    } catch (const std::bad_alloc &) {
        return lc::fail(LC_E_NOMEM, "lc_setfull_check: out of memory");
    }
    if (plan.n_items > 0x7FFFFFF0ull) return lc::fail(LC_E_INVALID, "lc_setfull_check: more than 2^31 count slots");
    for (const SfPass &p : plan.passes)
        if (p.mark1 - p.mark0 > 0x7FFFFFF0ull || p.scan1 - p.scan0 > 0x7FFFFFF0ull)
            return lc::fail(LC_E_INVALID, "lc_setfull_check: more than 2^31 workgroups in one pass");
    while (D.ev.size() < 3 + 3 * plan.passes.size() + 1) {
        hipEvent_t e = nullptr;
        HIPCHK(hipEventCreate(&e));
        D.ev.push_back(e);
    }

    // one metadata block, one copy
    Layout L;
    const size_t o_id_off = L.take((nk + 1) * 8), o_row_off = L.take((nk + 1) * 8);
    const size_t o_segs = L.take(plan.segs.size() * sizeof(SfSeg)), o_marks = L.take(plan.marks.size() * sizeof(SfMarkItem));
    const size_t o_scans = L.take(plan.scans.size() * sizeof(SfScanItem));
    const size_t o_span = L.take(nk * 4), o_item_base = L.take((nk + 1) * 4), o_status = L.take(nk);
    HIPCHK(D.hmeta.grow(L.at));
    HIPCHK(D.meta.grow(L.at));
    char *hm = D.hmeta.p;
    std::memcpy(hm + o_id_off, b->id_off, (nk + 1) * 8);
    std::memcpy(hm + o_row_off, b->row_off, (nk + 1) * 8);
    if (!plan.segs.empty()) std::memcpy(hm + o_segs, plan.segs.data(), plan.segs.size() * sizeof(SfSeg));
    if (!plan.marks.empty()) std::memcpy(hm + o_marks, plan.marks.data(), plan.marks.size() * sizeof(SfMarkItem));
    if (!plan.scans.empty()) std::memcpy(hm + o_scans, plan.scans.data(), plan.scans.size() * sizeof(SfScanItem));
    std::memcpy(hm + o_span, b->span, nk * 4);
    std::memcpy(hm + o_item_base, plan.item_base.data(), (nk + 1) * 4);
    if (b->status) std::memcpy(hm + o_status, b->status, nk);
    else std::memset(hm + o_status, 0, nk);

    // per-id inputs (three arrays), per-row inputs (four), the CSR
    HIPCHK(D.ids.grow(n_ids * 24));
    HIPCHK(D.rows.grow(n_rows * 32));
    HIPCHK(D.el_off.grow((n_rows + 1) * 8));
    HIPCHK(D.read_id.grow(n_el * 4 + 16));  // (mark's last 16-byte load may pass the end)
    HIPCHK(D.mat.grow(plan.max_words * 8));
    HIPCHK(D.part.grow(plan.n_items * 24));
    // out: error word (16 bytes), counts, valid, then per id: latency, known, last_absent, outcome, dup
    Layout O;
    const size_t o_err = O.take(16), o_counts = O.take(nk * 48), o_valid = O.take(nk);
    const size_t head_bytes = O.at;
    const size_t o_lat = O.take(n_ids * 8), o_known = O.take(n_ids * 8), o_la = O.take(n_ids * 8);
    const size_t o_outcome = O.take(n_ids), o_dup = O.take(n_ids);
    HIPCHK(D.out.grow(O.at));
    HIPCHK(D.hout.grow(head_bytes));

    size_t e = 0;
    HIPCHK(hipEventRecord(D.ev[e++], stream));
    HIPCHK(hipMemcpyAsync(D.meta.p, hm, L.at, hipMemcpyHostToDevice, stream));
    char *dids = (char *)D.ids.p, *drows = (char *)D.rows.p;
    if (n_ids) {
        HIPCHK(hipMemcpyAsync(dids, b->inv_pos, n_ids * 8, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(dids + n_ids * 8, b->ack_pos, n_ids * 8, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(dids + n_ids * 16, b->ack_time, n_ids * 8, hipMemcpyHostToDevice, stream));
    }
    if (n_rows) {
        HIPCHK(hipMemcpyAsync(drows, b->row_pos, n_rows * 8, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(drows + n_rows * 8, b->row_time, n_rows * 8, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(drows + n_rows * 16, b->row_inv_pos, n_rows * 8, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(drows + n_rows * 24, b->row_inv_time, n_rows * 8, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(D.el_off.p, b->el_off, (n_rows + 1) * 8, hipMemcpyHostToDevice, stream));
    }
    if (n_el) HIPCHK(hipMemcpyAsync(D.read_id.p, b->read_id, n_el * 4, hipMemcpyHostToDevice, stream));
    HIPCHK(hipEventRecord(D.ev[e++], stream));
    HIPCHK(hipMemsetAsync(D.out.p, 0, O.at, stream));
    HIPCHK(hipMemsetAsync(D.part.p, 0, std::max<size_t>(plan.n_items * 24, 24), stream));

    char *dm = (char *)D.meta.p, *dout = (char *)D.out.p;
    SfArgs a{};
    a.segs = (const SfSeg *)(dm + o_segs);
    a.id_off = (const uint64_t *)(dm + o_id_off); a.row_off = (const uint64_t *)(dm + o_row_off);
    a.span = (const uint32_t *)(dm + o_span); a.status = (const uint8_t *)(dm + o_status);
    a.item_base = (const uint32_t *)(dm + o_item_base);
    a.inv_pos = (const int64_t *)dids; a.ack_pos = (const int64_t *)(dids + n_ids * 8); a.ack_time = (const int64_t *)(dids + n_ids * 16);
    a.row_pos = (const int64_t *)drows; a.row_time = (const int64_t *)(drows + n_rows * 8);
    a.row_inv_pos = (const int64_t *)(drows + n_rows * 16); a.row_inv_time = (const int64_t *)(drows + n_rows * 24);
    a.el_off = (const uint64_t *)D.el_off.p; a.read_id = (const uint32_t *)D.read_id.p;
    a.mat = (uint64_t *)D.mat.p; a.part = (uint32_t *)D.part.p;
    a.outcome = (uint8_t *)(dout + o_outcome); a.dup = (uint8_t *)(dout + o_dup);
    a.latency = (int64_t *)(dout + o_lat); a.known = (int64_t *)(dout + o_known); a.last_absent = (int64_t *)(dout + o_la);
    a.counts = (unsigned long long *)(dout + o_counts); a.valid = (int8_t *)(dout + o_valid); a.err = (int32_t *)(dout + o_err);
    a.direct = (o->flags & LC_SETFULL_MARK_DIRECT) ? 1u : 0u;
    a.linearizable = o->linearizable ? 1u : 0u;
    const SfMarkItem *d_marks = (const SfMarkItem *)(dm + o_marks);
    const SfScanItem *d_scans = (const SfScanItem *)(dm + o_scans);

    for (const SfPass &p : plan.passes) {
        HIPCHK(hipEventRecord(D.ev[e++], stream));
        if (p.words) HIPCHK(hipMemsetAsync(D.mat.p, 0, p.words * 8, stream));
        HIPCHK(hipEventRecord(D.ev[e++], stream));
        if (p.mark1 > p.mark0) k_setfull_mark<<<(uint32_t)(p.mark1 - p.mark0), SF_BLOCK, 0, stream>>>(a, d_marks + p.mark0);
        HIPCHK(hipEventRecord(D.ev[e++], stream));
        if (p.scan1 > p.scan0) k_setfull_scan<<<(uint32_t)(p.scan1 - p.scan0), SF_BLOCK, 0, stream>>>(a, d_scans + p.scan0);
    }
    k_setfull_finish<<<(uint32_t)K, SF_BLOCK, 0, stream>>>(a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(D.ev[e++], stream));
    const size_t e_kernels = e - 1;
    HIPCHK(hipMemcpyAsync(D.hout.p, D.out.p, head_bytes, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    const char *ho = D.hout.p;
    int32_t bad_key;
    std::memcpy(&bad_key, ho + o_err, 4);
    if (bad_key) return lc::fail(LC_E_INVALID, "lc_setfull_check: key %d: an id at or past the key's span", bad_key - 1);
    std::memcpy(r->counts, ho + o_counts, nk * 48);
    std::memcpy(r->valid, ho + o_valid, nk);
    if (n_ids) {
        HIPCHK(hipMemcpyAsync(r->latency, dout + o_lat, n_ids * 8, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipMemcpyAsync(r->known, dout + o_known, n_ids * 8, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipMemcpyAsync(r->last_absent, dout + o_la, n_ids * 8, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipMemcpyAsync(r->outcome, dout + o_outcome, n_ids, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipMemcpyAsync(r->duplicated, dout + o_dup, n_ids, hipMemcpyDeviceToHost, stream));
    }
    HIPCHK(hipEventRecord(D.ev[e++], stream));
    HIPCHK(hipStreamSynchronize(stream));
    float f = 0;
    double zero = 0, mark = 0, scan = 0;
    for (size_t p = 0; p < plan.passes.size(); ++p) {
        HIPCHK(hipEventElapsedTime(&f, D.ev[2 + 3 * p], D.ev[3 + 3 * p]));
        zero += f;
        HIPCHK(hipEventElapsedTime(&f, D.ev[3 + 3 * p], D.ev[4 + 3 * p]));
        mark += f;
        HIPCHK(hipEventElapsedTime(&f, D.ev[4 + 3 * p], D.ev[5 + 3 * p]));
        scan += f;
    }
    HIPCHK(hipEventElapsedTime(&f, D.ev[0], D.ev[1]));
    D.ms[0] = f;
    D.ms[1] = mark;
    D.ms[2] = scan;
    HIPCHK(hipEventElapsedTime(&f, D.ev[e_kernels], D.ev[e_kernels + 1]));
    D.ms[3] = f;
    D.ms[5] = zero;
    D.ms[6] = (double)plan.passes.size();
    D.ms[7] = (double)plan.total_words * 8.0;
    D.ms[4] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    return LC_OK;
}

}  // namespace lcf
