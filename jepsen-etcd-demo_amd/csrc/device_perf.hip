// device_perf.hip -- jepsen.checker.perf's analysis on the device: the kernels
// and the step that runs them (lc_perf_check; include/lincheck.h, ABI 13).
//
// Input is one record per client completion (lc_perf_batch).  The step:
//   k_perf_count    one pass over the records, four per lane with 16-byte
//                   loads: latency, rate bucket, quantile bucket.  Counts go to
//                   the rate table [f][type][bucket] and the group table
//                   [f][bucket] through a per-workgroup LDS tile that covers
//                   PERF_TILE_BUCKETS buckets from the workgroup's smallest one
//                   (histories are nearly time-ordered); the tile's nonzero
//                   words leave with one atomic each, a record outside it with
//                   its own.  LC_PERF_COUNT_DIRECT: every record its own
//                   atomic.  Also the batch's largest latency magnitude.
//   k_perf_scan     one workgroup: the exclusive scan of the group counts
//                   (segment offsets) and the HBM tier's slots.
//   k_perf_scatter  every matched record's (x, latency) pair into its group's
//                   segment; places are taken per workgroup and group (LDS
//                   ranks, one global atomic per tile word), order inside a
//                   segment is free.
//   select          per non-empty group the n_q order statistics under
//                   (x, latency) order (csrc/perf_plan.hpp):
//     k_perf_select_lds  one workgroup per group of up to PERF_LDS_MAX points:
//                   staged once, sorted in LDS (bitonic), read at the indices.
//     k_perf_hbm_hist / k_perf_hbm_pick  larger groups: digit passes from the
//                   most significant byte of the 128-bit key (x - bucket
//                   start, latency + bias).  The histogram kernel runs over
//                   the elements of all large groups at once; an element
//                   counts for a quantile when it carries the quantile's
//                   prefix.  Quantiles that still share a prefix share one
//                   histogram.  The pick kernel extends every prefix by the
//                   digit that holds its rank and clears the histograms.
//                   Digits that are zero in every key are skipped: those above
//                   the bucket width on the host, those above the largest
//                   latency magnitude by the kernels themselves.
// Ordering is by kernel boundaries on one stream; no kernel waits for another
// workgroup.  All arithmetic is integer but the quantile index's one double
// product; counts use integer atomics, so results are bit-reproducible.
//
// Every record is checked (type, f ids, times inside the batch's bounds) before
// it addresses a table; a bad one counts nowhere, leaves its row in the error
// word, and the call returns LC_E_INVALID.
//
// The step has two entries over one body (perf_run): perf_check uploads the
// batch's three columns; perf_check_device runs the same launches on a batch
// that lc_perf_check_history (device_perf_pack.hip) has written into the
// device's own columns.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>

#include "common.hpp"
#include "device_perf.hpp"
#include "perf_plan.hpp"

#define HIPCHK(expr)                                                                       \
    do {                                                                                   \
        hipError_t _e = (expr);                                                            \
        if (_e != hipSuccess)                                                              \
            return lc::fail(LC_E_DEVICE, "%s failed: %s", #expr, hipGetErrorString(_e));  \
    } while (0)

#define LCP_CHK(expr)          \
    do {                       \
        int _rc = (expr);      \
        if (_rc) return _rc;   \
    } while (0)

namespace lcp {

namespace {

constexpr uint32_t NO_SLOT = 0xFFFFFFFFu;
constexpr uint32_t NONE32 = 0xFFFFFFFFu;

struct Pair {
    int64_t x, lat;
};

// One quantile of one HBM-tier group: the key prefix fixed so far (digits not
// yet decided are zero), the rank left among the keys that carry it, and the
// lowest quantile of the group with the same prefix (whose histogram it reads).
struct SelState {
    uint64_t phi, plo, k;
    uint32_t rep, pad;
};

enum { CTL_MAXMAG = 0, CTL_ERR = 1, CTL_LARGE = 2, CTL_TOTAL = 3, CTL_WORDS = 4 };

struct PerfArgs {
    const int64_t *t_comp, *t_inv;
    const uint32_t *meta;
    uint64_t n;
    uint32_t n_f, n_q, direct, force_hbm;
    int64_t rate_dt, q_dt, rate_first, q_first;
    uint64_t nr, nq, G;
    int64_t t_min, t_max, x_min, x_max;
    unsigned long long *ctl;     // [CTL_WORDS]
    unsigned long long *rate;    // [n_f * 3 * nr]
    unsigned long long *group;   // [G]
    int64_t *quant;              // [G * n_q]
    uint64_t *off;               // [G + 1]
    unsigned long long *cursor;  // [G]
    uint32_t *slot;              // [G] the group's HBM slot, or NO_SLOT
    uint32_t *large;             // [slots_cap] the group of each slot
    Pair *pairs;                 // [pair_cap]
    uint64_t pair_cap, slots_cap;
    uint32_t *hist;              // [slots_cap][n_q][PERF_DIGITS]
    SelState *state;             // [slots_cap][n_q]
    double q[LC_PERF_MAX_Q];
};

struct Rec {
    int64_t tc, ti;
    uint32_t m;
};

// The lane's PERF_LANE_RECORDS consecutive records; returns how many exist.
__device__ inline uint32_t load_records(const PerfArgs &a, uint64_t r0, Rec rec[PERF_LANE_RECORDS]) {
    if (r0 >= a.n) return 0;
    const uint32_t cnt = (uint32_t)std::min<uint64_t>(PERF_LANE_RECORDS, a.n - r0);
    if (cnt == PERF_LANE_RECORDS) {  // r0 is a multiple of 4: 16-byte aligned in every column
        const ulonglong2 c0 = *reinterpret_cast<const ulonglong2 *>(a.t_comp + r0);
        const ulonglong2 c1 = *reinterpret_cast<const ulonglong2 *>(a.t_comp + r0 + 2);
        const ulonglong2 i0 = *reinterpret_cast<const ulonglong2 *>(a.t_inv + r0);
        const ulonglong2 i1 = *reinterpret_cast<const ulonglong2 *>(a.t_inv + r0 + 2);
        const uint4 m = *reinterpret_cast<const uint4 *>(a.meta + r0);
        rec[0] = Rec{(int64_t)c0.x, (int64_t)i0.x, m.x};
        rec[1] = Rec{(int64_t)c0.y, (int64_t)i0.y, m.y};
        rec[2] = Rec{(int64_t)c1.x, (int64_t)i1.x, m.z};
        rec[3] = Rec{(int64_t)c1.y, (int64_t)i1.y, m.w};
    } else {
#pragma unroll
        for (uint32_t j = 0; j < PERF_LANE_RECORDS; ++j)
            rec[j] = j < cnt ? Rec{a.t_comp[r0 + j], a.t_inv[r0 + j], a.meta[r0 + j]} : Rec{0, 0, 0};
    }
    return cnt;
}

struct Place {
    bool ok, matched;
    uint32_t f_inv, f_comp, type;
    uint32_t rrel, qrel;  // buckets relative to rate_first / q_first
};

// Where a record counts, after every check that keeps it inside the tables.
__device__ inline Place place_of(const PerfArgs &a, const Rec &r) {
    Place p{};
    p.f_inv = r.m & 0xFFu;
    p.f_comp = (r.m >> 8) & 0xFFu;
    p.type = (r.m >> 16) & 0xFFu;
    p.matched = r.ti != LC_PERF_NO_INVOKE;
    if ((r.m >> 24) || p.type < LC_OK_T || p.type > LC_INFO || p.f_inv >= a.n_f || p.f_comp >= a.n_f) return p;
    if (r.tc < a.t_min || r.tc > a.t_max) return p;
    const uint64_t rr = (uint64_t)perf_bucket(r.tc, a.rate_dt) - (uint64_t)a.rate_first;
    if (rr >= a.nr) return p;
    p.rrel = (uint32_t)rr;
    if (p.matched) {
        if (r.ti < a.x_min || r.ti > a.x_max) return p;
        const uint64_t qr = (uint64_t)perf_bucket(r.ti, a.q_dt) - (uint64_t)a.q_first;
        if (qr >= a.nq) return p;
        p.qrel = (uint32_t)qr;
    }
    p.ok = true;
    return p;
}

__device__ inline uint32_t block_min(uint32_t v, uint32_t *sh) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = min(v, (uint32_t)__shfl_xor(v, d, 64));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    v = min(min(sh[0], sh[1]), min(sh[2], sh[3]));
    __syncthreads();
    return v;
}

__device__ inline uint64_t block_max64(uint64_t v, uint64_t *sh) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint64_t o = (uint64_t)__shfl_xor((unsigned long long)v, d, 64);
        v = o > v ? o : v;
    }
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    v = std::max(std::max(sh[0], sh[1]), std::max(sh[2], sh[3]));
    __syncthreads();
    return v;
}

__global__ __launch_bounds__(PERF_BLOCK) void k_perf_count(PerfArgs a) {
    __shared__ uint32_t tile_r[PERF_TILE_RATE_WORDS];
    __shared__ uint32_t tile_g[PERF_TILE_GROUP_WORDS];
    __shared__ uint32_t red[4];
    __shared__ uint64_t red64[4];
    const uint32_t tid = threadIdx.x;
    const uint64_t r0 = (uint64_t)blockIdx.x * PERF_WG_RECORDS + (uint64_t)tid * PERF_LANE_RECORDS;
    Rec rec[PERF_LANE_RECORDS];
    Place pl[PERF_LANE_RECORDS];
    const uint32_t cnt = load_records(a, r0, rec);
    uint32_t rmin = NONE32, qmin = NONE32;
    uint64_t mag = 0;
    uint64_t bad = 0;
#pragma unroll
    for (uint32_t j = 0; j < PERF_LANE_RECORDS; ++j) {
        pl[j] = Place{};
        if (j >= cnt) continue;
        pl[j] = place_of(a, rec[j]);
        if (!pl[j].ok) {
            bad = r0 + j + 1;
            continue;
        }
        rmin = min(rmin, pl[j].rrel);
        if (pl[j].matched) {
            qmin = min(qmin, pl[j].qrel);
            const int64_t lat = (int64_t)((uint64_t)rec[j].tc - (uint64_t)rec[j].ti);
            const uint64_t m = lat < 0 ? ~(uint64_t)lat : (uint64_t)lat;
            mag = m > mag ? m : mag;
        }
    }
    if (bad) atomicMax(&a.ctl[CTL_ERR], (unsigned long long)bad);
    mag = block_max64(mag, red64);
    if (tid == 0 && mag) atomicMax(&a.ctl[CTL_MAXMAG], (unsigned long long)mag);
    const bool tiled = !a.direct;
    if (tiled) {
        for (uint32_t i = tid; i < PERF_TILE_RATE_WORDS; i += PERF_BLOCK) tile_r[i] = 0;
        tile_g[tid] = 0;
        rmin = block_min(rmin, red);  // (its barriers also order the zeroing)
        qmin = block_min(qmin, red);
    }
#pragma unroll
    for (uint32_t j = 0; j < PERF_LANE_RECORDS; ++j) {
        const Place &p = pl[j];
        if (!p.ok) continue;
        const uint32_t ft = p.f_comp * 3 + (p.type - 1);
        const int rs = tiled ? perf_tile_slot(p.rrel, rmin) : -1;
        if (rs >= 0) atomicAdd(&tile_r[ft * PERF_TILE_BUCKETS + rs], 1u);
        else atomicAdd(&a.rate[perf_rate_index(p.f_comp, p.type, p.rrel, a.nr)], 1ull);
        if (!p.matched) continue;
        const int qs = tiled ? perf_tile_slot(p.qrel, qmin) : -1;
        if (qs >= 0) atomicAdd(&tile_g[p.f_inv * PERF_TILE_BUCKETS + qs], 1u);
        else atomicAdd(&a.group[perf_group_index(p.f_inv, p.qrel, a.nq)], 1ull);
    }
    if (!tiled) return;
    __syncthreads();
    for (uint32_t i = tid; i < PERF_TILE_RATE_WORDS; i += PERF_BLOCK) {
        const uint32_t v = tile_r[i];
        if (v) atomicAdd(&a.rate[(uint64_t)(i / PERF_TILE_BUCKETS) * a.nr + rmin + i % PERF_TILE_BUCKETS], (unsigned long long)v);
    }
    const uint32_t v = tile_g[tid];
    if (v) atomicAdd(&a.group[(uint64_t)(tid / PERF_TILE_BUCKETS) * a.nq + qmin + tid % PERF_TILE_BUCKETS], (unsigned long long)v);
}

// One workgroup: off[] = exclusive scan of group[], cursor[] = off[], and the
// HBM tier's slots in group order.  Each thread a contiguous slice.
constexpr uint32_t SCAN_BLOCK = 1024;
__global__ __launch_bounds__(SCAN_BLOCK) void k_perf_scan(PerfArgs a) {
    __shared__ uint64_t sh[SCAN_BLOCK];
    __shared__ uint32_t shl[SCAN_BLOCK];
    const uint32_t tid = threadIdx.x;
    const uint64_t n = a.G, per = (n + SCAN_BLOCK - 1) / SCAN_BLOCK;
    const uint64_t b = std::min(n, (uint64_t)tid * per), e = std::min(n, b + per);
    uint64_t sum = 0;
    uint32_t nl = 0;
    for (uint64_t i = b; i < e; ++i) {
        const uint64_t c = a.group[i];
        sum += c;
        nl += perf_tier(c, a.force_hbm != 0) == 2;
    }
    sh[tid] = sum;
    shl[tid] = nl;
    __syncthreads();
    for (uint32_t d = 1; d < SCAN_BLOCK; d <<= 1) {
        const uint64_t v = tid >= d ? sh[tid - d] : 0;
        const uint32_t w = tid >= d ? shl[tid - d] : 0;
        __syncthreads();
        sh[tid] += v;
        shl[tid] += w;
        __syncthreads();
    }
    uint64_t run = sh[tid] - sum;
    uint32_t s = shl[tid] - nl;
    for (uint64_t i = b; i < e; ++i) {
        const uint64_t c = a.group[i];
        a.off[i] = run;
        a.cursor[i] = run;
        run += c;
        if (perf_tier(c, a.force_hbm != 0) == 2 && s < a.slots_cap) {
            a.slot[i] = s;
            a.large[s] = (uint32_t)i;
            ++s;
        } else {
            a.slot[i] = NO_SLOT;
        }
    }
    if (tid == SCAN_BLOCK - 1) {
        a.off[n] = sh[tid];
        a.ctl[CTL_TOTAL] = sh[tid];
        a.ctl[CTL_LARGE] = std::min<uint64_t>(shl[tid], a.slots_cap);
    }
}

__global__ __launch_bounds__(PERF_BLOCK) void k_perf_scatter(PerfArgs a) {
    __shared__ uint32_t tile_g[PERF_TILE_GROUP_WORDS];
    __shared__ uint64_t base_g[PERF_TILE_GROUP_WORDS];
    __shared__ uint32_t red[4];
    if (a.ctl[CTL_ERR]) return;
    const uint32_t tid = threadIdx.x;
    const uint64_t r0 = (uint64_t)blockIdx.x * PERF_WG_RECORDS + (uint64_t)tid * PERF_LANE_RECORDS;
    Rec rec[PERF_LANE_RECORDS];
    Place pl[PERF_LANE_RECORDS];
    uint32_t rank[PERF_LANE_RECORDS];
    const uint32_t cnt = load_records(a, r0, rec);
    uint32_t qmin = NONE32;
#pragma unroll
    for (uint32_t j = 0; j < PERF_LANE_RECORDS; ++j) {
        pl[j] = Place{};
        if (j >= cnt) continue;
        pl[j] = place_of(a, rec[j]);
        if (pl[j].ok && pl[j].matched) qmin = min(qmin, pl[j].qrel);
    }
    const bool tiled = !a.direct;
    if (tiled) {
        tile_g[tid] = 0;
        qmin = block_min(qmin, red);
    }
#pragma unroll
    for (uint32_t j = 0; j < PERF_LANE_RECORDS; ++j) {
        const Place &p = pl[j];
        rank[j] = NONE32;
        if (!p.ok || !p.matched) continue;
        const int qs = tiled ? perf_tile_slot(p.qrel, qmin) : -1;
        if (qs >= 0) {
            rank[j] = atomicAdd(&tile_g[p.f_inv * PERF_TILE_BUCKETS + qs], 1u);
        } else {
            const uint64_t at = atomicAdd(&a.cursor[perf_group_index(p.f_inv, p.qrel, a.nq)], 1ull);
            const int64_t lat = (int64_t)((uint64_t)rec[j].tc - (uint64_t)rec[j].ti);
            if (at < a.pair_cap) a.pairs[at] = Pair{rec[j].ti, lat};
        }
    }
    if (!tiled) return;
    __syncthreads();
    {
        const uint32_t c = tile_g[tid];
        if (c) base_g[tid] = atomicAdd(&a.cursor[(uint64_t)(tid / PERF_TILE_BUCKETS) * a.nq + qmin + tid % PERF_TILE_BUCKETS],
                                       (unsigned long long)c);
    }
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < PERF_LANE_RECORDS; ++j) {
        if (rank[j] == NONE32) continue;
        const Place &p = pl[j];
        const uint64_t at = base_g[p.f_inv * PERF_TILE_BUCKETS + (p.qrel - qmin)] + rank[j];
        const int64_t lat = (int64_t)((uint64_t)rec[j].tc - (uint64_t)rec[j].ti);
        if (at < a.pair_cap) a.pairs[at] = Pair{rec[j].ti, lat};
    }
}

__device__ inline bool pair_less(const Pair &p, const Pair &q) { return p.x < q.x || (p.x == q.x && p.lat < q.lat); }

// LDS tier: one workgroup per group of up to PERF_LDS_MAX points.
__global__ __launch_bounds__(PERF_BLOCK) void k_perf_select_lds(PerfArgs a) {
    __shared__ Pair s[PERF_LDS_MAX];
    if (a.ctl[CTL_ERR]) return;
    const uint64_t g = blockIdx.x;
    const uint64_t n = a.group[g];
    if (perf_tier(n, a.force_hbm != 0) != 1) return;
    const uint64_t o = a.off[g];
    if (o + n > a.pair_cap) return;
    const uint32_t tid = threadIdx.x;
    uint32_t m = 1;
    while (m < n) m <<= 1;
    for (uint32_t i = tid; i < m; i += PERF_BLOCK) s[i] = i < n ? a.pairs[o + i] : Pair{INT64_MAX, INT64_MAX};
    __syncthreads();
    for (uint32_t k = 2; k <= m; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t i = tid; i < m; i += PERF_BLOCK) {
                const uint32_t x = i ^ j;
                if (x <= i) continue;
                const Pair p = s[i], q = s[x];
                const bool up = (i & k) == 0;
                if (up ? pair_less(q, p) : pair_less(p, q)) {
                    s[i] = q;
                    s[x] = p;
                }
            }
            __syncthreads();
        }
    if (tid < a.n_q) a.quant[g * a.n_q + tid] = s[perf_quantile_index(n, a.q[tid])].lat;
}

// ---- HBM tier -----------------------------------------------------------------

// Digit d (0 = most significant) of the key (hi, lo).
__device__ inline uint32_t key_digit(uint64_t hi, uint64_t lo, uint32_t d) {
    return (uint32_t)((d < 8 ? hi >> (56 - 8 * d) : lo >> (56 - 8 * (d - 8))) & 0xFFu);
}
// The masks of the d digits above digit d.
__device__ inline void prefix_masks(uint32_t d, uint64_t &mhi, uint64_t &mlo) {
    mhi = d == 0 ? 0ull : (d >= 8 ? ~0ull : ~0ull << (64 - 8 * d));
    mlo = d <= 8 ? 0ull : ~0ull << (64 - 8 * (d - 8));
}
// Whether pass d is skipped: no large group, or a digit of the latency half
// above the largest magnitude (zero in every key).
__device__ inline bool pass_skipped(const PerfArgs &a, uint32_t d, uint64_t &bias) {
    const uint32_t k = perf_mag_bits(a.ctl[CTL_MAXMAG]);
    bias = perf_bias(k);
    if (a.ctl[CTL_ERR] || a.ctl[CTL_LARGE] == 0) return true;
    return d >= 8 && d - 8 < 8 - perf_live_digits(k + 1);
}
// The group that holds position p of the pair array: off[g] <= p < off[g + 1].
__device__ inline uint64_t group_of(const PerfArgs &a, uint64_t p) {
    uint64_t lo = 0, hi = a.G;  // first index in (0, G] whose offset is above p, less one
    while (lo < hi) {
        const uint64_t mid = (lo + hi) / 2;
        if (a.off[mid + 1] > p) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}
__device__ inline uint64_t group_start(const PerfArgs &a, uint64_t g) {
    return (uint64_t)(a.q_first + (int64_t)(g % a.nq)) * (uint64_t)a.q_dt;
}

__global__ __launch_bounds__(PERF_BLOCK) void k_perf_hbm_init(PerfArgs a) {
    if (a.ctl[CTL_ERR]) return;
    const uint64_t total = a.ctl[CTL_LARGE] * a.n_q;
    for (uint64_t i = (uint64_t)blockIdx.x * PERF_BLOCK + threadIdx.x; i < total; i += (uint64_t)gridDim.x * PERF_BLOCK) {
        const uint64_t s = i / a.n_q, j = i % a.n_q;
        const uint64_t n = a.group[a.large[s]];
        a.state[i] = SelState{0, 0, perf_quantile_index(n, a.q[j]), 0, 0};
    }
}

__global__ __launch_bounds__(PERF_BLOCK) void k_perf_hbm_hist(PerfArgs a, uint32_t d) {
    __shared__ uint32_t lh[LC_PERF_MAX_Q][PERF_DIGITS];
    uint64_t bias;
    if (pass_skipped(a, d, bias)) return;
    const uint64_t total = std::min<uint64_t>(a.ctl[CTL_TOTAL], a.pair_cap);
    const uint64_t p0 = (uint64_t)blockIdx.x * PERF_WG_RECORDS;
    if (p0 >= total) return;
    const uint64_t pend = std::min(total, p0 + PERF_WG_RECORDS);
    const uint32_t tid = threadIdx.x;
    uint64_t mhi, mlo;
    prefix_masks(d, mhi, mlo);
    const uint64_t gA = group_of(a, p0), gB = group_of(a, pend - 1);
    const uint64_t pa = p0 + (uint64_t)tid * PERF_LANE_RECORDS;
    if (gA == gB) {  // the whole chunk in one group: its histograms in LDS
        const uint32_t sl = a.slot[gA];
        if (sl == NO_SLOT) return;
        for (uint32_t q = 0; q < a.n_q; ++q) lh[q][tid] = 0;
        __syncthreads();
        const uint64_t start = group_start(a, gA);
        const SelState *st = a.state + (uint64_t)sl * a.n_q;
#pragma unroll
        for (uint32_t j = 0; j < PERF_LANE_RECORDS; ++j) {
            if (pa + j >= pend) continue;
            const Pair e = a.pairs[pa + j];
            const uint64_t hi = (uint64_t)e.x - start, lo = (uint64_t)e.lat + bias;
            const uint32_t dig = key_digit(hi, lo, d);
            for (uint32_t q = 0; q < a.n_q; ++q) {
                const SelState s = st[q];
                if (s.rep == q && ((hi ^ s.phi) & mhi) == 0 && ((lo ^ s.plo) & mlo) == 0) atomicAdd(&lh[q][dig], 1u);
            }
        }
        __syncthreads();
        for (uint32_t q = 0; q < a.n_q; ++q) {
            const uint32_t v = lh[q][tid];
            if (v) atomicAdd(&a.hist[((uint64_t)sl * a.n_q + q) * PERF_DIGITS + tid], v);
        }
        return;
    }
    // several groups in the chunk: each element to its own group's histograms
    if (pa >= pend) return;
    uint64_t g = group_of(a, pa);
#pragma unroll
    for (uint32_t j = 0; j < PERF_LANE_RECORDS; ++j) {
        if (pa + j >= pend) continue;
        while (g < a.G && a.off[g + 1] <= pa + j) ++g;
        if (g >= a.G) break;
        const uint32_t sl = a.slot[g];
        if (sl == NO_SLOT) continue;
        const Pair e = a.pairs[pa + j];
        const uint64_t hi = (uint64_t)e.x - group_start(a, g), lo = (uint64_t)e.lat + bias;
        const uint32_t dig = key_digit(hi, lo, d);
        const SelState *st = a.state + (uint64_t)sl * a.n_q;
        for (uint32_t q = 0; q < a.n_q; ++q) {
            const SelState s = st[q];
            if (s.rep == q && ((hi ^ s.phi) & mhi) == 0 && ((lo ^ s.plo) & mlo) == 0)
                atomicAdd(&a.hist[((uint64_t)sl * a.n_q + q) * PERF_DIGITS + dig], 1u);
        }
    }
}

// One workgroup per slot in turn; wave w takes quantiles w and w + 4.
__global__ __launch_bounds__(PERF_BLOCK) void k_perf_hbm_pick(PerfArgs a, uint32_t d) {
    __shared__ SelState ns[LC_PERF_MAX_Q];
    uint64_t bias;
    if (pass_skipped(a, d, bias)) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t n_large = a.ctl[CTL_LARGE];
    for (uint64_t sl = blockIdx.x; sl < n_large; sl += gridDim.x) {
        for (uint32_t q = wave; q < a.n_q; q += PERF_BLOCK / 64) {
            SelState s = a.state[sl * a.n_q + q];
            const uint4 h = *reinterpret_cast<const uint4 *>(a.hist + (sl * a.n_q + s.rep) * PERF_DIGITS + 4 * lane);
            const uint64_t mine = (uint64_t)h.x + h.y + h.z + h.w;
            uint64_t inc = mine;
#pragma unroll
            for (int sft = 1; sft < 64; sft <<= 1) {
                const uint64_t y = (uint64_t)__shfl_up((unsigned long long)inc, sft, 64);
                if ((int)lane >= sft) inc += y;
            }
            const uint64_t excl = inc - mine;
            const bool here = excl <= s.k && s.k < inc;
            if (here) {
                uint64_t before = excl;
                uint32_t dig = 4 * lane;
                if (s.k >= before + h.x) {
                    before += h.x;
                    ++dig;
                    if (s.k >= before + h.y) {
                        before += h.y;
                        ++dig;
                        if (s.k >= before + h.z) {
                            before += h.z;
                            ++dig;
                        }
                    }
                }
                s.k -= before;
                if (d < 8) s.phi |= (uint64_t)dig << (56 - 8 * d);
                else s.plo |= (uint64_t)dig << (56 - 8 * (d - 8));
                ns[q] = s;
            }
            if (__ballot(here) == 0 && lane == 0) {  // the rank is not among the counted keys
                atomicMax(&a.ctl[CTL_ERR], ~0ull);
                ns[q] = s;
            }
        }
        __syncthreads();
        for (uint32_t q = 0; q < a.n_q; ++q) a.hist[(sl * a.n_q + q) * PERF_DIGITS + tid] = 0;
        if (tid < a.n_q) {
            SelState s = ns[tid];
            uint32_t rep = tid;
            for (uint32_t q = 0; q < tid; ++q)
                if (ns[q].phi == s.phi && ns[q].plo == s.plo) {
                    rep = q;
                    break;
                }
            s.rep = rep;
            a.state[sl * a.n_q + tid] = s;
            a.quant[(uint64_t)a.large[sl] * a.n_q + tid] = (int64_t)(s.plo - bias);
        }
        __syncthreads();
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

}  // namespace

struct PerfDev {
    Buf t_comp, t_inv, meta, out, off, cursor, slot, large, pairs, hist, state;
    HostBuf hout;
    hipEvent_t ev[4] = {};
    double ms[4] = {0, 0, 0, 0};
    uint64_t generation = 0;  // bumped whenever the record columns are about to be rewritten
};

namespace {

int perf_dev_of(PerfDev **dev) {
    if (*dev) return LC_OK;
    PerfDev *d = new (std::nothrow) PerfDev();
    if (!d) return lc::fail(LC_E_NOMEM, "lc_perf_check: out of memory");
    *dev = d;  // (owned by the context from here on: a failed event is freed with it)
    for (hipEvent_t &e : d->ev) HIPCHK(hipEventCreate(&e));
    return LC_OK;
}

}  // namespace

void perf_dev_free(PerfDev *d) {
    if (!d) return;
    for (Buf *b : {&d->t_comp, &d->t_inv, &d->meta, &d->out, &d->off, &d->cursor, &d->slot, &d->large, &d->pairs, &d->hist, &d->state})
        b->release();
    d->hout.release();
    for (hipEvent_t e : d->ev)
        if (e) (void)hipEventDestroy(e);
    delete d;
}

int perf_last_timing(const PerfDev *d, double *out_ms) {
    for (int i = 0; i < 4; ++i) out_ms[i] = d ? d->ms[i] : 0.0;
    return LC_OK;
}

int perf_records_device(PerfDev **dev, uint64_t n, int64_t **t_comp, int64_t **t_inv, uint32_t **meta) {
    LCP_CHK(perf_dev_of(dev));
    PerfDev &D = **dev;
    D.generation++;
    HIPCHK(D.t_comp.grow(n * 8));
    HIPCHK(D.t_inv.grow(n * 8));
    HIPCHK(D.meta.grow(n * 4));
    *t_comp = (int64_t *)D.t_comp.p; *t_inv = (int64_t *)D.t_inv.p; *meta = (uint32_t *)D.meta.p;
    return LC_OK;
}

uint64_t perf_generation(const PerfDev *d) { return d ? d->generation : 0; }

int perf_records_download(PerfDev *d, hipStream_t stream, uint64_t n, int64_t *t_comp, int64_t *t_inv, uint32_t *meta) {
    if (!d || d->t_comp.cap < n * 8 || d->t_inv.cap < n * 8 || d->meta.cap < n * 4)
        return lc::fail(LC_E_INVALID, "lc_perf_checked_records: the device holds no such batch");
    if (!n) return LC_OK;
    HIPCHK(hipMemcpyAsync(t_comp, d->t_comp.p, n * 8, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(t_inv, d->t_inv.p, n * 8, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(meta, d->meta.p, n * 4, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    return LC_OK;
}

namespace {

// lc_perf_check's step.  resident: the record columns already lie in the
// device's own arrays (perf_records_device), b's column pointers are not read
// and nothing is uploaded.
int perf_run(PerfDev **dev, hipStream_t stream, const lc_perf_batch *b, const lc_perf_opts *o, lc_perf_result *r, bool resident) {
    lc::Range range("lc_perf_check");
    const auto wall0 = std::chrono::steady_clock::now();
    // everything the host can check, before any kernel
    int64_t shape[4];
    if (int rc = perf_opts_check(b, o, shape)) return rc;
    if (!resident && b->n > 0 && (!b->t_comp || !b->t_inv || !b->meta)) return lc::fail(LC_E_INVALID, "lc_perf_check: null record column");
    if (b->n > 0 && b->n_f < 1) return lc::fail(LC_E_INVALID, "lc_perf_check: records but no :f names");
    if ((uint64_t)b->n > 0xFFFFFFFFull * 256) return lc::fail(LC_E_INVALID, "lc_perf_check: too many records for one call");
    const uint64_t F = (uint64_t)b->n_f, nr = (uint64_t)shape[1], nq = (uint64_t)shape[3], n_q = (uint64_t)o->n_q;
    const uint64_t R = F * 3 * nr, G = F * nq;
    if (r->rate_cap < R || r->group_cap < G || r->quant_cap < G * n_q)
        return lc::fail(LC_E_INVALID, "lc_perf_check: result arrays too small: %llu rate, %llu group, %llu quantile entries needed",
                        (unsigned long long)R, (unsigned long long)G, (unsigned long long)(G * n_q));
    if ((R && !r->rate) || (G && (!r->group || !r->quant))) return lc::fail(LC_E_INVALID, "lc_perf_check: null result array");
    r->rate_first = shape[0]; r->rate_n = shape[1]; r->q_first = shape[2]; r->q_n = shape[3];
    if (b->n == 0) return LC_OK;

    const bool force = (o->flags & LC_PERF_SELECT_HBM) != 0;
    const uint64_t nm = (uint64_t)b->n_matched;
    const bool hbm = nm > 0 && (force || nm > PERF_LDS_MAX);
    const uint64_t slots_cap = !hbm ? 0 : (force ? std::min(G, nm) : nm / (PERF_LDS_MAX + 1));
    if (slots_cap * n_q * PERF_DIGITS * 4 > PERF_HIST_MAX_BYTES)
        return lc::fail(LC_E_NOMEM, "lc_perf_check: the digit histograms of %llu groups pass %llu bytes",
                        (unsigned long long)slots_cap, (unsigned long long)PERF_HIST_MAX_BYTES);

    LCP_CHK(perf_dev_of(dev));
    PerfDev &D = **dev;
    const uint64_t n = (uint64_t)b->n;
    if (!resident) {
        D.generation++;
        HIPCHK(D.t_comp.grow(n * 8));
        HIPCHK(D.t_inv.grow(n * 8));
        HIPCHK(D.meta.grow(n * 4));
    } else if (D.t_comp.cap < n * 8 || D.t_inv.cap < n * 8 || D.meta.cap < n * 4) {
        return lc::fail(LC_E_INVALID, "lc_perf_check: the device holds no batch of %llu records", (unsigned long long)n);
    }
    // out: control words, rate, group, quantiles
    const size_t o_ctl = 0, o_rate = CTL_WORDS * 8, o_group = o_rate + R * 8, o_quant = o_group + G * 8;
    const size_t out_bytes = o_quant + G * n_q * 8;
    HIPCHK(D.out.grow(out_bytes));
    HIPCHK(D.hout.grow(out_bytes));
    HIPCHK(D.off.grow((G + 1) * 8));
    HIPCHK(D.cursor.grow(G * 8));
    HIPCHK(D.slot.grow(G * 4));
    HIPCHK(D.large.grow(slots_cap * 4));
    HIPCHK(D.pairs.grow(nm * sizeof(Pair)));
    HIPCHK(D.hist.grow(slots_cap * n_q * PERF_DIGITS * 4));
    HIPCHK(D.state.grow(slots_cap * n_q * sizeof(SelState)));

    HIPCHK(hipEventRecord(D.ev[0], stream));
    if (!resident) {
        HIPCHK(hipMemcpyAsync(D.t_comp.p, b->t_comp, n * 8, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(D.t_inv.p, b->t_inv, n * 8, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(D.meta.p, b->meta, n * 4, hipMemcpyHostToDevice, stream));
    }
    HIPCHK(hipEventRecord(D.ev[1], stream));
    HIPCHK(hipMemsetAsync(D.out.p, 0, out_bytes, stream));
    if (slots_cap) HIPCHK(hipMemsetAsync(D.hist.p, 0, slots_cap * n_q * PERF_DIGITS * 4, stream));

    char *dout = (char *)D.out.p;
    PerfArgs a{};
    a.t_comp = (const int64_t *)D.t_comp.p; a.t_inv = (const int64_t *)D.t_inv.p; a.meta = (const uint32_t *)D.meta.p;
    a.n = n; a.n_f = (uint32_t)F; a.n_q = (uint32_t)n_q;
    a.direct = (o->flags & LC_PERF_COUNT_DIRECT) ? 1u : 0u; a.force_hbm = force ? 1u : 0u;
    a.rate_dt = o->rate_dt_ns; a.q_dt = o->quantile_dt_ns; a.rate_first = shape[0]; a.q_first = shape[2];
    a.nr = nr; a.nq = nq; a.G = G;
    a.t_min = b->t_min; a.t_max = b->t_max; a.x_min = b->x_min; a.x_max = b->x_max;
    if (nm == 0) {  // no matched record is legal: none may claim to be one
        a.x_min = 0;
        a.x_max = -1;
    }
    a.ctl = (unsigned long long *)(dout + o_ctl); a.rate = (unsigned long long *)(dout + o_rate);
    a.group = (unsigned long long *)(dout + o_group); a.quant = (int64_t *)(dout + o_quant);
    a.off = (uint64_t *)D.off.p; a.cursor = (unsigned long long *)D.cursor.p; a.slot = (uint32_t *)D.slot.p;
    a.large = (uint32_t *)D.large.p; a.pairs = (Pair *)D.pairs.p; a.pair_cap = nm; a.slots_cap = slots_cap;
    a.hist = (uint32_t *)D.hist.p; a.state = (SelState *)D.state.p;
    for (int j = 0; j < o->n_q; ++j) a.q[j] = o->q[j];

    const uint32_t g_rec = (uint32_t)((n + PERF_WG_RECORDS - 1) / PERF_WG_RECORDS);
    k_perf_count<<<g_rec, PERF_BLOCK, 0, stream>>>(a);
    if (nm > 0) {
        k_perf_scan<<<1, SCAN_BLOCK, 0, stream>>>(a);
        k_perf_scatter<<<g_rec, PERF_BLOCK, 0, stream>>>(a);
        k_perf_select_lds<<<(uint32_t)G, PERF_BLOCK, 0, stream>>>(a);
        if (hbm) {
            const uint32_t g_pair = (uint32_t)((nm + PERF_WG_RECORDS - 1) / PERF_WG_RECORDS);
            const uint32_t g_slot = (uint32_t)std::min<uint64_t>(slots_cap, 1024);
            k_perf_hbm_init<<<g_slot, PERF_BLOCK, 0, stream>>>(a);
            const uint32_t hi_live = perf_live_digits(perf_dt_bits(o->quantile_dt_ns));
            for (uint32_t d = 8 - hi_live; d < PERF_KEY_DIGITS; ++d) {
                k_perf_hbm_hist<<<g_pair, PERF_BLOCK, 0, stream>>>(a, d);
                k_perf_hbm_pick<<<g_slot, PERF_BLOCK, 0, stream>>>(a, d);
            }
        }
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(D.ev[2], stream));
    HIPCHK(hipMemcpyAsync(D.hout.p, D.out.p, out_bytes, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipEventRecord(D.ev[3], stream));
    HIPCHK(hipStreamSynchronize(stream));
    const char *ho = D.hout.p;
    uint64_t ctl[CTL_WORDS];
    std::memcpy(ctl, ho + o_ctl, sizeof ctl);
    float f = 0;
    for (int i = 0; i < 3; ++i) {
        HIPCHK(hipEventElapsedTime(&f, D.ev[i], D.ev[i + 1]));
        D.ms[i] = f;
    }
    if (ctl[CTL_ERR] == ~0ull) return lc::fail(LC_E_DEVICE, "lc_perf_check: the HBM select lost a rank (internal error)");
    if (ctl[CTL_ERR])
        return lc::fail(LC_E_INVALID, "lc_perf_check: record %llu: a bad :type / :f code, or a time outside the batch's bounds",
                        (unsigned long long)(ctl[CTL_ERR] - 1));
    if (nm > 0 && ctl[CTL_TOTAL] != nm)
        return lc::fail(LC_E_INVALID, "lc_perf_check: %llu matched records, n_matched says %llu", (unsigned long long)ctl[CTL_TOTAL],
                        (unsigned long long)nm);
    if (R) std::memcpy(r->rate, ho + o_rate, R * 8);
    if (G) std::memcpy(r->group, ho + o_group, G * 8);
    if (G) std::memcpy(r->quant, ho + o_quant, G * n_q * 8);
    D.ms[3] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    return LC_OK;
}

}  // namespace

int perf_check(PerfDev **dev, hipStream_t stream, const lc_perf_batch *b, const lc_perf_opts *o, lc_perf_result *r) {
    return perf_run(dev, stream, b, o, r, false);
}

int perf_check_device(PerfDev **dev, hipStream_t stream, const lc_perf_batch *sizes, const lc_perf_opts *o, lc_perf_result *r) {
    return perf_run(dev, stream, sizes, o, r, true);
}

}  // namespace lcp
