// perf_plan.hpp -- the pure rules of the perf path (lc_perf_pack,
// lc_perf_check): bucket index, quantile index, which
// groups take the LDS select, the histogram tile window, the offset layout of
// the tables.  No HIP types: the kernels (device_perf.hip) and the host call
// the same functions, and tests/perf_plan_main.cpp pins them on the CPU.
//
// Tables.  With F = n_f names, NR rate buckets and NQ quantile buckets:
//   rate   [F][3][NR]   index (f * 3 + (type - 1)) * NR + (bucket - rate_first)
//   group  [F][NQ]      index f * NQ + (bucket - q_first)
//   quant  [F][NQ][n_q] index group * n_q + j
// A group's points lie in one segment of the pair array, at the exclusive scan
// of the group counts in group-index order.
//
// Select tiers.
//   LDS tier   groups of at most PERF_LDS_MAX points: one workgroup stages the
//              group's (x, latency) pairs once and sorts them there.  16 bytes
//              a point: 2,048 points = 32 KiB a workgroup, so five workgroups
//              (20 of 32 waves) share a CU's 160 KiB.
//   HBM tier   larger groups (every non-empty group under LC_PERF_SELECT_HBM):
//              a most-significant-digit-first radix select with
//              PERF_DIGIT_BITS-bit digits over the 128-bit key
//              (x - bucket start, latency + bias), all groups and quantiles in
//              one grid per digit.
// Histogram tile.  A workgroup of the streaming kernels takes PERF_WG_RECORDS
// records; its LDS tile covers the PERF_TILE_BUCKETS buckets of each width
// starting at the workgroup's smallest one, for every f (and type).
#pragma once

#include <cstdint>

#include "../../include/lincheck.h"

#if defined(__HIPCC__)
#define LC_PERF_HD __host__ __device__
#else
#define LC_PERF_HD
#endif

namespace lcp {

constexpr uint32_t PERF_BLOCK = 256;            // threads per workgroup of the streaming kernels
constexpr uint32_t PERF_LANE_RECORDS = 4;       // consecutive records per lane: two 16-byte loads per time column
constexpr uint32_t PERF_WG_RECORDS = PERF_BLOCK * PERF_LANE_RECORDS;
constexpr uint32_t PERF_TILE_BUCKETS = 8;
constexpr uint32_t PERF_TILE_RATE_WORDS = LC_PERF_MAX_F * 3 * PERF_TILE_BUCKETS;   // 768
constexpr uint32_t PERF_TILE_GROUP_WORDS = LC_PERF_MAX_F * PERF_TILE_BUCKETS;      // 256
constexpr uint32_t PERF_LDS_BYTES_PER_CU = 160 * 1024;
constexpr uint32_t PERF_LDS_MAX = 2048;         // points: 32 KiB of pairs
constexpr uint32_t PERF_LDS_SHARE = PERF_LDS_BYTES_PER_CU / (PERF_LDS_MAX * 16);   // 5 workgroups a CU
constexpr uint32_t PERF_DIGIT_BITS = 8;
constexpr uint32_t PERF_DIGITS = 1u << PERF_DIGIT_BITS;
constexpr uint32_t PERF_KEY_DIGITS = 128 / PERF_DIGIT_BITS;  // digit 0 is the most significant
// Most table entries (rate + group) one call may ask for.
constexpr uint64_t PERF_MAX_TABLE = 1ull << 26;
// Most device memory the HBM select's digit histograms may take.
constexpr uint64_t PERF_HIST_MAX_BYTES = 1ull << 30;

// floor(t / dt) for dt > 0, any sign of t.
LC_PERF_HD inline int64_t perf_bucket(int64_t t, int64_t dt) {
    const int64_t q = t / dt;
    return (t % dt != 0 && t < 0) ? q - 1 : q;
}
// A bucket's plotted time: its midpoint.
LC_PERF_HD inline int64_t perf_bucket_mid(int64_t b, int64_t dt) { return b * dt + dt / 2; }

// min(n - 1, (long) floor((double) n * q)), n >= 1; the product in IEEE double
// as written.  A q below 0 selects the first point.
LC_PERF_HD inline uint64_t perf_quantile_index(uint64_t n, double q) {
    const double x = (double)n * q;
    if (!(x > 0.0)) return 0;
    if (x >= (double)n) return n - 1;
    const uint64_t i = (uint64_t)x;  // truncation = floor for x >= 0
    return i < n - 1 ? i : n - 1;
}

// Which select a group of n points takes: 0 none (empty), 1 LDS, 2 HBM.
LC_PERF_HD inline int perf_tier(uint64_t n, bool force_hbm) {
    if (n == 0) return 0;
    return (force_hbm || n > PERF_LDS_MAX) ? 2 : 1;
}

// The tile slot of bucket b in a workgroup whose smallest bucket is b0, or -1.
LC_PERF_HD inline int perf_tile_slot(int64_t b, int64_t b0) {
    const uint64_t d = (uint64_t)b - (uint64_t)b0;
    return (b >= b0 && d < PERF_TILE_BUCKETS) ? (int)d : -1;
}

LC_PERF_HD inline uint64_t perf_rate_index(uint32_t f, uint32_t type, uint64_t rel, uint64_t nr) {
    return ((uint64_t)f * 3 + (type - 1)) * nr + rel;
}
LC_PERF_HD inline uint64_t perf_group_index(uint32_t f, uint64_t rel, uint64_t nq) { return (uint64_t)f * nq + rel; }

// The bit length of the largest latency magnitude (mag = lat < 0 ? ~lat : lat):
// every latency lies in [-2^k, 2^k), so latency + 2^k (mod 2^64) is below
// 2^(k + 1) and keeps signed order.  k = 63 is the plain sign-bit flip.
LC_PERF_HD inline uint32_t perf_mag_bits(uint64_t maxmag) {
    uint32_t k = 0;
    while (k < 63 && (maxmag >> k) != 0) ++k;
    return k;
}
LC_PERF_HD inline uint64_t perf_bias(uint32_t k) { return 1ull << k; }
// Key digits that can differ: a 64-bit half whose values are below 2^bits has
// zero digits above ceil(bits / PERF_DIGIT_BITS) (at least one is kept).
LC_PERF_HD inline uint32_t perf_live_digits(uint32_t bits) {
    const uint32_t d = (bits + PERF_DIGIT_BITS - 1) / PERF_DIGIT_BITS;
    return d == 0 ? 1 : (d > 8 ? 8 : d);
}
// Bits of x - bucket start, below dt.
LC_PERF_HD inline uint32_t perf_dt_bits(int64_t dt) {
    uint32_t k = 0;
    while (k < 63 && ((uint64_t)(dt - 1) >> k) != 0) ++k;
    return k;
}

struct PerfShape {
    int rc = LC_OK;  // LC_E_INVALID: a width that is not positive; LC_E_NOMEM: tables above PERF_MAX_TABLE
    int64_t rate_first = 0, rate_n = 0, q_first = 0, q_n = 0;
};

inline PerfShape perf_shape(const lc_perf_batch *b, int64_t rate_dt, int64_t q_dt) {
    PerfShape s;
    if (rate_dt <= 0 || q_dt <= 0) {
        s.rc = LC_E_INVALID;
        return s;
    }
    if (b->n > 0) {
        s.rate_first = perf_bucket(b->t_min, rate_dt);
        s.rate_n = (int64_t)((uint64_t)perf_bucket(b->t_max, rate_dt) - (uint64_t)s.rate_first + 1);
    }
    if (b->n_matched > 0) {
        s.q_first = perf_bucket(b->x_min, q_dt);
        s.q_n = (int64_t)((uint64_t)perf_bucket(b->x_max, q_dt) - (uint64_t)s.q_first + 1);
    }
    const uint64_t F = (uint64_t)b->n_f;
    if (s.rate_n < 0 || s.q_n < 0 || (uint64_t)s.rate_n > PERF_MAX_TABLE || (uint64_t)s.q_n > PERF_MAX_TABLE ||
        F * 3 * (uint64_t)s.rate_n + F * (uint64_t)s.q_n > PERF_MAX_TABLE)
        s.rc = LC_E_NOMEM;
    return s;
}

// What lc_perf_check refuses before it touches a device, in its order: n_q,
// the quantiles, n_f, then lc_perf_shape's checks; shape4 as lc_perf_shape's.
// Defined in host_perf.cpp (it sets the error text).
int perf_opts_check(const lc_perf_batch *b, const lc_perf_opts *o, int64_t *shape4);

}  // namespace lcp
