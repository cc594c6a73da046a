// device_set.hip -- jepsen.checker/set (set.clj:46) on the device: the kernels
// and the step that runs them (lc_set_check; include/lincheck.h, ABI 12).
//
// Per key three bitmaps over the key's ids: A (attempted), K (acknowledged),
// R (the final read).  The classes are word-wise
//     ok = R & A    lost = K & ~R    unexpected = R & ~A    recovered = ok & ~K
// and each class's interval string is its maximal runs of consecutive
// elements: a run starts at a set bit whose predecessor is clear (or, for
// rank ids, is not the element one below) and ends likewise on the other side.
//
// Two tiers (csrc/set_plan.hpp):
//   k_set_small     one workgroup per key, bitmaps in LDS (ds_or), never in HBM
//   k_set_mark      HBM tier: ids to bits, one lane per 16 consecutive rows.
//                   The demo's elements come from (range): neighbouring rows
//                   hit neighbouring bits.  When the ids of a workgroup's
//                   4,096 rows span no more than its LDS tile (8,192 ids) they
//                   are marked there (ds_or) and only the tile's nonzero words
//                   leave, one atomicOr each; otherwise, and under
//                   LC_PATH_SET_DIRECT, each lane merges the bits that fall
//                   into one 32-bit word and issues its own atomics
//   k_set_classify  HBM tier: 16-byte loads of A, K, R, classes, popcounts, runs
// Runs come out ascending per (key, class), so each pass runs twice: a count
// pass (popcounts and run starts per workgroup), one
// single-workgroup exclusive scan (k_set_scan), and a write pass that puts
// every run's first and last element at its scanned place.  Ordering is by
// kernel boundaries on one stream; no kernel waits for another workgroup.
// A run's end has the rank of its start, and the ends before any boundary
// are the starts before it less the run that is open across it, so only the
// starts are scanned.
// The six counts of a key are summed without atomics: every workgroup leaves
// its own six sums (part[]), and the key's first workgroup of the write pass
// adds them up.  (One atomic add per wave and key was measured first: on one
// key of 2^26 ids the 49,152 adds to the same six words took 0.46 of the
// count pass's 0.50 ms.)
//
// Every id is checked against its key's span before it addresses a bitmap;
// a bad id (or class byte) marks nothing, names its key in the error word,
// and the call returns LC_E_INVALID.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "device_set.hpp"
#include "set_plan.hpp"

#define HIPCHK(expr)                                                                       \
    do {                                                                                   \
        hipError_t _e = (expr);                                                            \
        if (_e != hipSuccess)                                                              \
            return lc::fail(LC_E_DEVICE, "%s failed: %s", #expr, hipGetErrorString(_e));  \
    } while (0)

namespace lcs {

namespace {

struct SetArgs {
    const uint64_t *add_off;
    const uint32_t *add_id;
    const uint8_t *add_cls;
    const uint64_t *read_off;
    const uint32_t *read_id;
    const uint64_t *base;
    const uint32_t *span;
    const int64_t *kmin;
    const uint8_t *rank;
    const uint64_t *vals_off;
    const int64_t *vals;
    const uint8_t *status;
    const uint32_t *item_base;  // [n_keys + 1]
    uint64_t *bm;               // A, K, R: n_words each
    uint64_t n_words;
    unsigned long long *counts; // [6 * n_keys]
    uint32_t *part;             // [6 * n_items] each workgroup's own six counts
    uint64_t *cnt;              // [4 * n_items] run starts, then their exclusive scan
    uint64_t *run_off;          // [4 * n_keys + 1]
    int64_t *runs;              // [2 * run_cap]
    uint64_t run_cap;
    int8_t *valid;
    int32_t *err;               // 1 + a key with a bad id, or 0
    const unsigned long long *total;  // runs in all (after k_set_scan)
    uint32_t direct;            // LC_PATH_SET_DIRECT
};

struct W3 {
    uint64_t a, k, r;
};
struct Masks {
    uint64_t c[4], s[4], e[4];  // class words, run starts, run ends: ok, lost, unexpected, recovered
};

__device__ inline void classes(const W3 &w, uint64_t c[4]) {
    c[0] = w.r & w.a;
    c[1] = w.k & ~w.r;
    c[2] = w.r & ~w.a;
    c[3] = w.r & w.a & ~w.k;
}

// Of the ids 64 * w + bit of cand (each with a predecessor), those whose
// element is one above the element of the id below.
__device__ inline uint64_t adjacent(const int64_t *vals, uint64_t w, uint64_t cand) {
    uint64_t out = 0;
    while (cand) {
        const int b = __ffsll((unsigned long long)cand) - 1;
        cand &= cand - 1;
        const uint64_t g = 64 * w + (uint64_t)b;
        if ((uint64_t)vals[g] - 1 == (uint64_t)vals[g - 1]) out |= 1ull << b;
    }
    return out;
}

// Word w of a key with its neighbours (0 beyond the key's ends).  vals: a
// rank key's values, or null for offset ids (neighbouring ids are
// neighbouring elements).
__device__ inline Masks word_masks(const W3 &prv, const W3 &cur, const W3 &nxt, const int64_t *vals, uint64_t w) {
    uint64_t adj = ~0ull, adj_next = 1;
    if (vals) {
        const uint64_t u = cur.a | cur.k | cur.r;
        const uint64_t up = (prv.a | prv.k | prv.r) >> 63, un = (nxt.a | nxt.k | nxt.r) & 1;
        adj = adjacent(vals, w, u & ((u << 1) | up));
        adj_next = ((u >> 63) & un) ? adjacent(vals, w + 1, 1) : 0;
    }
    Masks m;
    uint64_t p[4], n[4];
    classes(cur, m.c);
    classes(prv, p);
    classes(nxt, n);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        m.s[i] = m.c[i] & ~(((m.c[i] << 1) | (p[i] >> 63)) & adj);
        m.e[i] = m.c[i] & ~(((m.c[i] >> 1) | (n[i] << 63)) & ((adj >> 1) | (adj_next << 63)));
    }
    return m;
}

// Exclusive scan and total of four counters over the workgroup's 256 threads.
__device__ inline void block_scan4(const uint32_t v[4], uint32_t excl[4], uint32_t tot[4], uint32_t (*sh)[4]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        uint32_t x = v[c];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(x, d, 64);
            if (lane >= d) x += y;
        }
        inc[c] = x;
        if (lane == 63) sh[wave][c] = x;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        uint32_t before = 0, t = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const uint32_t s = sh[w][c];
            before += w < wave ? s : 0u;
            t += s;
        }
        excl[c] = before + inc[c] - v[c];
        tot[c] = t;
    }
    __syncthreads();
}

// The workgroup's sum of each of six counters, in every thread.
__device__ inline void block_sum6(const uint64_t v[6], uint64_t out[6], uint64_t (*sh)[6]) {
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

// Count pass: the workgroup's six counts to its item's place in part[].
__device__ inline void put_counts(const SetArgs &a, uint64_t item, const uint32_t pc[6], uint64_t (*sh)[6]) {
    uint64_t v[6], tot[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) v[i] = pc[i];
    block_sum6(v, tot, sh);
#pragma unroll
    for (int i = 0; i < 6; ++i)
        if (threadIdx.x == (uint32_t)i) a.part[6 * item + i] = (uint32_t)tot[i];
}

__device__ inline void count_word(const W3 &cur, const Masks &m, uint32_t ns[4], uint32_t pc[6]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) ns[i] += __popcll(m.s[i]);
    pc[0] += __popcll(cur.a);
    pc[1] += __popcll(cur.k);
    pc[2] += __popcll(m.c[0]);
    pc[3] += __popcll(m.c[1]);
    pc[4] += __popcll(m.c[3]);
    pc[5] += __popcll(m.c[2]);
}

// The runs that start / end in word w: first elements at pos, last ones at epos.
__device__ inline void emit_word(const SetArgs &a, const Masks &m, uint64_t w, int64_t kmin, const int64_t *vals,
                                 uint64_t pos[4], uint64_t epos[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        uint64_t s = m.s[i];
        while (s) {
            const uint64_t g = 64 * w + (uint64_t)(__ffsll((unsigned long long)s) - 1);
            s &= s - 1;
            if (pos[i] < a.run_cap) a.runs[2 * pos[i]] = vals ? vals[g] : (int64_t)((uint64_t)kmin + g);
            ++pos[i];
        }
        uint64_t e = m.e[i];
        while (e) {
            const uint64_t g = 64 * w + (uint64_t)(__ffsll((unsigned long long)e) - 1);
            e &= e - 1;
            if (epos[i] < a.run_cap) a.runs[2 * epos[i] + 1] = vals ? vals[g] : (int64_t)((uint64_t)kmin + g);
            ++epos[i];
        }
    }
}

// What a key's first workgroup leaves for the host in the write pass (every
// thread of it calls): the key's counts summed over its workgroups of the
// count pass, :valid?, and where its runs start.
__device__ inline void finish_key(const SetArgs &a, uint32_t k, uint64_t cbase, uint32_t chunks, bool checked,
                                  uint64_t (*sh)[6]) {
    if (threadIdx.x < 4) a.run_off[4ull * k + threadIdx.x] = a.cnt[cbase + (uint64_t)threadIdx.x * chunks];
    if (chunks == 1) {  // (the LDS tier: one workgroup's counts are the key's)
        const uint32_t *p = a.part + 6 * (cbase / 4);
        if (threadIdx.x < 6) a.counts[6ull * k + threadIdx.x] = checked ? p[threadIdx.x] : 0u;
        if (threadIdx.x == 0)
            a.valid[k] = !checked ? (int8_t)LC_UNKNOWN : (p[3] == 0 && p[5] == 0 ? (int8_t)LC_VALID : (int8_t)LC_INVALID);
        return;
    }
    uint64_t acc[6] = {0, 0, 0, 0, 0, 0}, tot[6];
    if (checked)
        for (uint32_t j = threadIdx.x; j < chunks; j += SET_BLOCK)
#pragma unroll
            for (int i = 0; i < 6; ++i) acc[i] += a.part[6 * (cbase / 4 + j) + i];
    block_sum6(acc, tot, sh);
#pragma unroll
    for (int i = 0; i < 6; ++i)
        if (threadIdx.x == (uint32_t)i) a.counts[6ull * k + i] = tot[i];
    if (threadIdx.x == 0)
        a.valid[k] = !checked ? (int8_t)LC_UNKNOWN : (tot[3] == 0 && tot[5] == 0 ? (int8_t)LC_VALID : (int8_t)LC_INVALID);
}

template <bool WRITE>
__global__ __launch_bounds__(SET_BLOCK) void k_set_small(SetArgs a, const uint32_t *small_keys) {
    __shared__ uint64_t sb[3][SET_LDS_MAX_WORDS];
    __shared__ uint32_t ssc[4][4];
    __shared__ uint64_t s6[4][6];
    const uint32_t k = small_keys[blockIdx.x];
    const uint32_t tid = threadIdx.x;
    const uint64_t cbase = 4ull * a.item_base[k];
    const bool checked = a.status[k] == LC_SET_KEY_OK;
    const uint32_t span = checked ? a.span[k] : 0u;
    if (span == 0 || span > SET_LDS_MAX_BITS) {  // nothing to mark (a wider key never comes here)
        if (!WRITE) {
            if (tid < 4) a.cnt[cbase + tid] = 0;
            if (tid < 6) a.part[6 * (cbase / 4) + tid] = 0;
        } else {
            finish_key(a, k, cbase, 1, checked, s6);
        }
        return;
    }
    const uint32_t kw = (span + 63) / 64;
    for (uint32_t i = tid; i < kw; i += SET_BLOCK) sb[0][i] = sb[1][i] = sb[2][i] = 0;
    __syncthreads();
    for (uint64_t i = a.add_off[k] + tid; i < a.add_off[k + 1]; i += SET_BLOCK) {
        const uint32_t id = a.add_id[i], cls = a.add_cls[i];
        if (id >= span || (cls != LC_SET_ATTEMPT && cls != LC_SET_ACK)) {
            atomicMax(a.err, (int32_t)k + 1);
            continue;
        }
        atomicOr(reinterpret_cast<uint32_t *>(sb[cls - 1]) + (id >> 5), 1u << (id & 31));
    }
    for (uint64_t i = a.read_off[k] + tid; i < a.read_off[k + 1]; i += SET_BLOCK) {
        const uint32_t id = a.read_id[i];
        if (id >= span) {
            atomicMax(a.err, (int32_t)k + 1);
            continue;
        }
        atomicOr(reinterpret_cast<uint32_t *>(sb[2]) + (id >> 5), 1u << (id & 31));
    }
    __syncthreads();
    const int64_t *vals = a.rank[k] ? a.vals + a.vals_off[k] : nullptr;
    const int64_t kmin = a.kmin[k];
    const uint32_t wpt = (kw + SET_BLOCK - 1) / SET_BLOCK;  // consecutive words per thread (<= 4)
    const uint32_t w0 = tid * wpt;
    auto load = [&](uint32_t w) -> W3 { return w < kw ? W3{sb[0][w], sb[1][w], sb[2][w]} : W3{0, 0, 0}; };
    uint32_t ns[4] = {0, 0, 0, 0}, pc[6] = {0, 0, 0, 0, 0, 0}, open_in[4] = {0, 0, 0, 0};
    for (uint32_t j = 0; j < wpt && w0 + j < kw; ++j) {
        const uint32_t w = w0 + j;
        const W3 cur = load(w);
        const Masks m = word_masks(w ? load(w - 1) : W3{0, 0, 0}, cur, load(w + 1), vals, w);
        count_word(cur, m, ns, pc);
        if (j == 0)
#pragma unroll
            for (int i = 0; i < 4; ++i) open_in[i] = (uint32_t)(m.c[i] & ~m.s[i] & 1);
    }
    uint32_t excl[4], tot[4];
    block_scan4(ns, excl, tot, ssc);
    if (!WRITE) {
        if (tid < 4) a.cnt[cbase + tid] = tot[tid];
        put_counts(a, cbase / 4, pc, s6);
        return;
    }
    finish_key(a, k, cbase, 1, true, s6);
    if (*a.total > a.run_cap || *a.err) return;
    uint64_t pos[4], epos[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        pos[i] = a.cnt[cbase + i] + excl[i];
        epos[i] = pos[i] - open_in[i];
    }
    for (uint32_t j = 0; j < wpt && w0 + j < kw; ++j) {
        const uint32_t w = w0 + j;
        const Masks m = word_masks(w ? load(w - 1) : W3{0, 0, 0}, load(w), load(w + 1), vals, w);
        emit_word(a, m, w, kmin, vals, pos, epos);
    }
}

// HBM tier: rows [row, row + SET_MARK_ROWS) of one key's add or read ids.
__global__ __launch_bounds__(SET_BLOCK) void k_set_mark(SetArgs a, const SetMarkItem *marks) {
    const SetMarkItem it = marks[blockIdx.x];
    const uint32_t k = it.key, span = a.span[k];
    const uint64_t end = std::min(it.is_read ? a.read_off[k + 1] : a.add_off[k + 1], it.row + SET_MARK_ROWS);
    const uint64_t r0 = it.row + (uint64_t)threadIdx.x * SET_MARK_LANE_ROWS;
    uint32_t *A = reinterpret_cast<uint32_t *>(a.bm + a.base[k]);
    uint32_t *K = reinterpret_cast<uint32_t *>(a.bm + a.n_words + a.base[k]);
    uint32_t *R = reinterpret_cast<uint32_t *>(a.bm + 2 * a.n_words + a.base[k]);
    // the lane's rows, read once: 16-byte loads when the lane has all 16 and they are aligned
    const uint32_t nrow = r0 < end ? (uint32_t)std::min<uint64_t>(SET_MARK_LANE_ROWS, end - r0) : 0u;
    const uint32_t *src = it.is_read ? a.read_id : a.add_id;
    uint32_t ids[SET_MARK_LANE_ROWS], cl[SET_MARK_LANE_ROWS];
    if (nrow == SET_MARK_LANE_ROWS && (r0 & 3) == 0) {
#pragma unroll
        for (uint32_t q = 0; q < SET_MARK_LANE_ROWS / 4; ++q) {
            const uint4 v = reinterpret_cast<const uint4 *>(src + r0)[q];
            ids[4 * q] = v.x; ids[4 * q + 1] = v.y; ids[4 * q + 2] = v.z; ids[4 * q + 3] = v.w;
        }
    } else {
#pragma unroll
        for (uint32_t j = 0; j < SET_MARK_LANE_ROWS; ++j) ids[j] = j < nrow ? src[r0 + j] : 0u;
    }
    if (it.is_read) {
#pragma unroll
        for (uint32_t j = 0; j < SET_MARK_LANE_ROWS; ++j) cl[j] = LC_SET_ATTEMPT;
    } else if (nrow == SET_MARK_LANE_ROWS && (r0 & 15) == 0) {
        const uint4 v = *reinterpret_cast<const uint4 *>(a.add_cls + r0);
        const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (uint32_t j = 0; j < SET_MARK_LANE_ROWS; ++j) cl[j] = (w4[j / 4] >> (8 * (j % 4))) & 0xFFu;
    } else {
#pragma unroll
        for (uint32_t j = 0; j < SET_MARK_LANE_ROWS; ++j) cl[j] = j < nrow ? (uint32_t)a.add_cls[r0 + j] : (uint32_t)LC_SET_ATTEMPT;
    }
    // the tile form: the workgroup's ids within SET_MARK_TILE_WORDS words of their least one
    __shared__ uint32_t tile[2][SET_MARK_TILE_WORDS];
    __shared__ uint32_t red[2][SET_BLOCK / 64];
    bool tiled = false;
    uint32_t lo = 0;
    if (!a.direct) {
        uint32_t mn = 0xFFFFFFFFu, mx = 0;
#pragma unroll
        for (uint32_t j = 0; j < SET_MARK_LANE_ROWS; ++j)
            if (j < nrow && ids[j] < span) {
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
        tile[0][threadIdx.x] = 0;
        tile[1][threadIdx.x] = 0;
        __syncthreads();
#pragma unroll
        for (uint32_t w = 0; w < SET_BLOCK / 64; ++w) {
            mn = min(mn, red[0][w]);
            mx = max(mx, red[1][w]);
        }
        lo = mn >> 5;
        tiled = mn <= mx && (mx >> 5) - lo < SET_MARK_TILE_WORDS;  // the same in every lane
    }
    // the lanes' own atomics: the bits of consecutive rows that share a 32-bit word leave in one
    uint32_t w1 = 0, m1 = 0, w2 = 0, m2 = 0;  // attempted (or read) / acknowledged
    bool bad = false;
#pragma unroll
    for (uint32_t j = 0; j < SET_MARK_LANE_ROWS; ++j) {
        if (j >= nrow) continue;
        const uint32_t id = ids[j], cls = cl[j];
        if (id >= span || (cls != LC_SET_ATTEMPT && cls != LC_SET_ACK)) {
            bad = true;
            continue;
        }
        const uint32_t w = id >> 5, bit = 1u << (id & 31);
        if (tiled) {
            atomicOr(&tile[cls == LC_SET_ACK][w - lo], bit);
        } else if (cls == LC_SET_ATTEMPT) {
            if (w != w1 && m1) {
                atomicOr((it.is_read ? R : A) + w1, m1);
                m1 = 0;
            }
            w1 = w;
            m1 |= bit;
        } else {
            if (w != w2 && m2) {
                atomicOr(K + w2, m2);
                m2 = 0;
            }
            w2 = w;
            m2 |= bit;
        }
    }
    if (m1) atomicOr((it.is_read ? R : A) + w1, m1);
    if (m2) atomicOr(K + w2, m2);
    if (bad) atomicMax(a.err, (int32_t)k + 1);
    if (tiled) {
        __syncthreads();
        const uint32_t t1 = tile[0][threadIdx.x], t2 = tile[1][threadIdx.x];
        if (t1) atomicOr((it.is_read ? R : A) + lo + threadIdx.x, t1);
        if (t2) atomicOr(K + lo + threadIdx.x, t2);
    }
}

template <bool WRITE>
__global__ __launch_bounds__(SET_BLOCK) void k_set_classify(SetArgs a, const SetItem *items) {
    __shared__ uint32_t ssc[4][4];
    __shared__ uint64_t s6[4][6];
    const SetItem it = items[blockIdx.x];
    const uint32_t k = it.key, tid = threadIdx.x;
    const uint64_t kw = ((uint64_t)a.span[k] + 63) / 64;
    const uint32_t chunks = (uint32_t)((kw + SET_BLOCK_WORDS - 1) / SET_BLOCK_WORDS);
    const uint64_t cbase = 4ull * a.item_base[k];
    const uint64_t *A = a.bm + a.base[k], *K = A + a.n_words, *R = K + a.n_words;
    const int64_t *vals = a.rank[k] ? a.vals + a.vals_off[k] : nullptr;
    const int64_t kmin = a.kmin[k];
    const uint64_t w0 = (uint64_t)it.chunk * SET_BLOCK_WORDS + (uint64_t)tid * SET_LANE_WORDS;
    const bool have = w0 < kw;  // (w0 even; the key's words are padded to even, so w0 + 1 is the key's own too)
    W3 prv{0, 0, 0}, c0{0, 0, 0}, c1{0, 0, 0}, nxt{0, 0, 0};
    if (have) {
        const ulonglong2 pa = *reinterpret_cast<const ulonglong2 *>(A + w0);
        const ulonglong2 pk = *reinterpret_cast<const ulonglong2 *>(K + w0);
        const ulonglong2 pr = *reinterpret_cast<const ulonglong2 *>(R + w0);
        c0 = W3{pa.x, pk.x, pr.x};
        c1 = W3{pa.y, pk.y, pr.y};
        if (w0 > 0) prv = W3{A[w0 - 1], K[w0 - 1], R[w0 - 1]};
        if (w0 + 2 < kw) nxt = W3{A[w0 + 2], K[w0 + 2], R[w0 + 2]};
    }
    Masks m0{}, m1{};
    uint32_t ns[4] = {0, 0, 0, 0}, pc[6] = {0, 0, 0, 0, 0, 0}, open_in[4] = {0, 0, 0, 0};
    if (have) {
        m0 = word_masks(prv, c0, c1, vals, w0);
        m1 = word_masks(c0, c1, nxt, vals, w0 + 1);
        count_word(c0, m0, ns, pc);
        count_word(c1, m1, ns, pc);
#pragma unroll
        for (int i = 0; i < 4; ++i) open_in[i] = (uint32_t)(m0.c[i] & ~m0.s[i] & 1);
    }
    uint32_t excl[4], tot[4];
    block_scan4(ns, excl, tot, ssc);
    if (!WRITE) {
        if (tid < 4) a.cnt[cbase + (uint64_t)tid * chunks + it.chunk] = tot[tid];
        put_counts(a, cbase / 4 + it.chunk, pc, s6);
        return;
    }
    if (it.chunk == 0) finish_key(a, k, cbase, chunks, true, s6);
    if (!have || *a.total > a.run_cap || *a.err) return;
    uint64_t pos[4], epos[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        pos[i] = a.cnt[cbase + (uint64_t)i * chunks + it.chunk] + excl[i];
        epos[i] = pos[i] - open_in[i];
    }
    emit_word(a, m0, w0, kmin, vals, pos, epos);
    emit_word(a, m1, w0 + 1, kmin, vals, pos, epos);
}

// Exclusive scan of cnt[0..n) in place by one workgroup: each thread a
// contiguous slice.  n = 4 * items <= 4 * (keys + bitmap words / 512): a
// million keys are 32 MB through one CU, well under a millisecond's worth of
// the step that made them.
constexpr uint32_t SCAN_BLOCK = 1024;
__global__ __launch_bounds__(SCAN_BLOCK) void k_set_scan(uint64_t *cnt, uint64_t n, unsigned long long *total,
                                                         uint64_t *run_off_end) {
    __shared__ uint64_t sh[SCAN_BLOCK];
    const uint32_t tid = threadIdx.x;
    const uint64_t per = (n + SCAN_BLOCK - 1) / SCAN_BLOCK;
    const uint64_t b = std::min(n, (uint64_t)tid * per), e = std::min(n, b + per);
    uint64_t sum = 0;
    for (uint64_t i = b; i < e; ++i) sum += cnt[i];
    sh[tid] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < SCAN_BLOCK; d <<= 1) {
        const uint64_t v = tid >= d ? sh[tid - d] : 0;
        __syncthreads();
        sh[tid] += v;
        __syncthreads();
    }
    uint64_t run = sh[tid] - sum;
    for (uint64_t i = b; i < e; ++i) {
        const uint64_t t = cnt[i];
        cnt[i] = run;
        run += t;
    }
    if (tid == SCAN_BLOCK - 1) {
        *total = sh[tid];
        *run_off_end = sh[tid];
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

// Sections of the per-step metadata block, each 16-byte aligned.
struct Layout {
    size_t at = 0;
    size_t take(size_t bytes) {
        const size_t o = at;
        at += (bytes + 15) & ~(size_t)15;
        return o;
    }
};

}  // namespace

struct SetDev {
    Buf add_id, add_cls, read_id, vals, meta, bm, out, cnt, part, runs;
    HostBuf hmeta, hout;
    hipEvent_t ev[4] = {};
    double ms[4] = {0, 0, 0, 0};
};

void set_dev_free(SetDev *d) {
    if (!d) return;
    for (Buf *b : {&d->add_id, &d->add_cls, &d->read_id, &d->vals, &d->meta, &d->bm, &d->out, &d->cnt, &d->part, &d->runs}) b->release();
    d->hmeta.release();
    d->hout.release();
    for (hipEvent_t e : d->ev)
        if (e) (void)hipEventDestroy(e);
    delete d;
}

int set_last_timing(const SetDev *d, double *out_ms) {
    for (int i = 0; i < 4; ++i) out_ms[i] = d ? d->ms[i] : 0.0;
    return LC_OK;
}

// The offset arrays of a batch (a caller may have built it): ascending, the
// key's bitmap words inside the batch's and before the next key's, a rank
// key's values at least its span.  The ids themselves are the kernels' to check.
static int validate(const lc_set_batch *b) {
    const int64_t K = b->n_keys;
    if (K < 0 || K > 0x7FFFFFF0) return lc::fail(LC_E_INVALID, "lc_set_check: n_keys %lld", (long long)K);
    if (K == 0) return LC_OK;
    if (!b->add_off || !b->read_off || !b->base || !b->span || !b->min || !b->rank || !b->vals_off)
        return lc::fail(LC_E_INVALID, "lc_set_check: null per-key array");
    if (b->n_words & 1) return lc::fail(LC_E_INVALID, "lc_set_check: n_words is odd");
    for (int64_t k = 0; k < K; ++k) {
        if (b->add_off[k + 1] < b->add_off[k] || b->read_off[k + 1] < b->read_off[k] || b->vals_off[k + 1] < b->vals_off[k])
            return lc::fail(LC_E_INVALID, "lc_set_check: key %lld: offsets not ascending", (long long)k);
        const uint8_t st = b->status ? b->status[k] : (uint8_t)LC_SET_KEY_OK;
        if (st > LC_SET_KEY_ERROR || b->rank[k] > 1) return lc::fail(LC_E_INVALID, "lc_set_check: key %lld: bad status / rank code", (long long)k);
        if (st != LC_SET_KEY_OK) continue;
        if (b->span[k] > SET_MAX_SPAN) return lc::fail(LC_E_INVALID, "lc_set_check: key %lld: span above 2^32 - 64", (long long)k);
        const uint64_t next = k + 1 < K ? b->base[k + 1] : b->n_words;
        if ((b->base[k] & 1) || b->base[k] > b->n_words || next > b->n_words || next < b->base[k] ||
            set_words_padded(b->span[k]) > next - b->base[k])
            return lc::fail(LC_E_INVALID, "lc_set_check: key %lld: bitmap words outside the batch's or into the next key's",
                            (long long)k);
        if (b->rank[k] && b->vals_off[k + 1] - b->vals_off[k] < b->span[k])
            return lc::fail(LC_E_INVALID, "lc_set_check: key %lld: fewer values than its span", (long long)k);
        if (!b->rank[k] && b->span[k] && (uint64_t)INT64_MAX - (uint64_t)b->min[k] < (uint64_t)b->span[k] - 1 && b->min[k] >= 0)
            return lc::fail(LC_E_INVALID, "lc_set_check: key %lld: min + span passes INT64_MAX", (long long)k);
    }
    if (b->add_off[K] && (!b->add_id || !b->add_cls)) return lc::fail(LC_E_INVALID, "lc_set_check: null add arrays");
    if (b->read_off[K] && !b->read_id) return lc::fail(LC_E_INVALID, "lc_set_check: null read_id");
    if (b->vals_off[K] && !b->vals) return lc::fail(LC_E_INVALID, "lc_set_check: null vals");
    return LC_OK;
}

int set_check(SetDev **dev, hipStream_t stream, int path_flags, const lc_set_batch *b, lc_set_result *r) {
    lc::Range range("lc_set_check");
    const auto wall0 = std::chrono::steady_clock::now();
    if (int rc = validate(b)) return rc;
    const int64_t K = b->n_keys;
    if (K > 0 && (!r->valid || !r->counts || !r->run_off)) return lc::fail(LC_E_INVALID, "lc_set_check: null result array");
    if (r->run_cap && !r->runs) return lc::fail(LC_E_INVALID, "lc_set_check: null runs");
    r->n_runs = 0;
    if (K == 0) {
        if (r->run_off) r->run_off[0] = 0;
        return LC_OK;
    }
    if (!*dev) {
        *dev = new (std::nothrow) SetDev();
        if (!*dev) return lc::fail(LC_E_NOMEM, "lc_set_check: out of memory");
        for (hipEvent_t &e : (*dev)->ev) HIPCHK(hipEventCreate(&e));
    }
    SetDev &D = **dev;

    SetStepIn in;
    in.n_keys = K; in.span = b->span; in.status = b->status; in.add_off = b->add_off; in.read_off = b->read_off;
    in.n_words = b->n_words;
    in.force_hbm = (path_flags & LC_PATH_SET_HBM) != 0;
    SetStepPlan plan;
    try {
        plan = plan_set_step(in);
    } catch (const std::bad_alloc &) {
        return lc::fail(LC_E_NOMEM, "lc_set_check: out of memory");
    }
    if (plan.rc == LC_E_NOMEM)
        return lc::fail(LC_E_NOMEM, "lc_set_check: the bitmaps need %llu bytes, above the cap of %llu",
                        (unsigned long long)(24 * b->n_words), (unsigned long long)in.bm_max_bytes);
    if (plan.n_items > 0x7FFFFFFFull || plan.marks.size() > 0x7FFFFFFFull)
        return lc::fail(LC_E_INVALID, "lc_set_check: more than 2^31 workgroups in one step");

    // one metadata block, one copy
    const size_t nk = (size_t)K;
    Layout L;
    const size_t o_add_off = L.take((nk + 1) * 8), o_read_off = L.take((nk + 1) * 8), o_base = L.take(nk * 8);
    const size_t o_min = L.take(nk * 8), o_vals_off = L.take((nk + 1) * 8);
    const size_t o_marks = L.take(plan.marks.size() * sizeof(SetMarkItem)), o_items = L.take(plan.items.size() * sizeof(SetItem));
    const size_t o_span = L.take(nk * 4), o_item_base = L.take((nk + 1) * 4), o_small = L.take(plan.small_keys.size() * 4);
    const size_t o_rank = L.take(nk), o_status = L.take(nk);
    HIPCHK(D.hmeta.grow(L.at));
    HIPCHK(D.meta.grow(L.at));
    char *hm = D.hmeta.p;
    std::memcpy(hm + o_add_off, b->add_off, (nk + 1) * 8);
    std::memcpy(hm + o_read_off, b->read_off, (nk + 1) * 8);
    std::memcpy(hm + o_base, b->base, nk * 8);
    std::memcpy(hm + o_min, b->min, nk * 8);
    std::memcpy(hm + o_vals_off, b->vals_off, (nk + 1) * 8);
    if (!plan.marks.empty()) std::memcpy(hm + o_marks, plan.marks.data(), plan.marks.size() * sizeof(SetMarkItem));
    if (!plan.items.empty()) std::memcpy(hm + o_items, plan.items.data(), plan.items.size() * sizeof(SetItem));
    std::memcpy(hm + o_span, b->span, nk * 4);
    std::memcpy(hm + o_item_base, plan.item_base.data(), (nk + 1) * 4);
    if (!plan.small_keys.empty()) std::memcpy(hm + o_small, plan.small_keys.data(), plan.small_keys.size() * 4);
    std::memcpy(hm + o_rank, b->rank, nk);
    if (b->status) std::memcpy(hm + o_status, b->status, nk);
    else std::memset(hm + o_status, 0, nk);

    const uint64_t n_add = b->add_off[K], n_read = b->read_off[K], n_vals = b->vals_off[K];
    HIPCHK(D.add_id.grow(n_add * 4));
    HIPCHK(D.add_cls.grow(n_add));
    HIPCHK(D.read_id.grow(n_read * 4));
    HIPCHK(D.vals.grow(n_vals * 8));
    HIPCHK(D.bm.grow(plan.bm_words * 8));
    HIPCHK(D.cnt.grow(plan.n_items * 4 * 8));
    HIPCHK(D.part.grow(plan.n_items * 6 * 4));
    HIPCHK(D.runs.grow(r->run_cap * 16));
    // out: error word (8 bytes), total, counts, run_off, valid
    const size_t o_err = 0, o_total = 8, o_counts = 16, o_run_off = o_counts + nk * 48, o_valid = o_run_off + (4 * nk + 1) * 8;
    const size_t out_bytes = o_valid + nk;
    HIPCHK(D.out.grow(out_bytes));
    HIPCHK(D.hout.grow(out_bytes));

    HIPCHK(hipEventRecord(D.ev[0], stream));
    HIPCHK(hipMemcpyAsync(D.meta.p, hm, L.at, hipMemcpyHostToDevice, stream));
    if (n_add) {
        HIPCHK(hipMemcpyAsync(D.add_id.p, b->add_id, n_add * 4, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(D.add_cls.p, b->add_cls, n_add, hipMemcpyHostToDevice, stream));
    }
    if (n_read) HIPCHK(hipMemcpyAsync(D.read_id.p, b->read_id, n_read * 4, hipMemcpyHostToDevice, stream));
    if (n_vals) HIPCHK(hipMemcpyAsync(D.vals.p, b->vals, n_vals * 8, hipMemcpyHostToDevice, stream));
    HIPCHK(hipEventRecord(D.ev[1], stream));
    HIPCHK(hipMemsetAsync(D.out.p, 0, out_bytes, stream));
    if (plan.bm_words) HIPCHK(hipMemsetAsync(D.bm.p, 0, plan.bm_words * 8, stream));

    char *dm = (char *)D.meta.p, *dout = (char *)D.out.p;
    SetArgs a{};
    a.add_off = (const uint64_t *)(dm + o_add_off); a.add_id = (const uint32_t *)D.add_id.p; a.add_cls = (const uint8_t *)D.add_cls.p;
    a.read_off = (const uint64_t *)(dm + o_read_off); a.read_id = (const uint32_t *)D.read_id.p;
    a.base = (const uint64_t *)(dm + o_base); a.span = (const uint32_t *)(dm + o_span); a.kmin = (const int64_t *)(dm + o_min);
    a.rank = (const uint8_t *)(dm + o_rank); a.vals_off = (const uint64_t *)(dm + o_vals_off); a.vals = (const int64_t *)D.vals.p;
    a.status = (const uint8_t *)(dm + o_status); a.item_base = (const uint32_t *)(dm + o_item_base);
    a.bm = (uint64_t *)D.bm.p; a.n_words = b->n_words;
    a.counts = (unsigned long long *)(dout + o_counts); a.cnt = (uint64_t *)D.cnt.p; a.part = (uint32_t *)D.part.p;
    a.run_off = (uint64_t *)(dout + o_run_off); a.runs = (int64_t *)D.runs.p; a.run_cap = r->run_cap;
    a.valid = (int8_t *)(dout + o_valid); a.err = (int32_t *)(dout + o_err);
    a.total = (const unsigned long long *)(dout + o_total);
    a.direct = (path_flags & LC_PATH_SET_DIRECT) ? 1u : 0u;
    const uint32_t *d_small = (const uint32_t *)(dm + o_small);
    const SetItem *d_items = (const SetItem *)(dm + o_items);
    const SetMarkItem *d_marks = (const SetMarkItem *)(dm + o_marks);
    const uint32_t g_small = (uint32_t)plan.small_keys.size(), g_items = (uint32_t)plan.items.size();
    const uint32_t g_marks = (uint32_t)plan.marks.size();

    if (g_marks) k_set_mark<<<g_marks, SET_BLOCK, 0, stream>>>(a, d_marks);
    if (g_small) k_set_small<false><<<g_small, SET_BLOCK, 0, stream>>>(a, d_small);
    if (g_items) k_set_classify<false><<<g_items, SET_BLOCK, 0, stream>>>(a, d_items);
    k_set_scan<<<1, SCAN_BLOCK, 0, stream>>>(a.cnt, plan.n_items * 4, (unsigned long long *)(dout + o_total),
                                             a.run_off + 4 * nk);
    if (g_small) k_set_small<true><<<g_small, SET_BLOCK, 0, stream>>>(a, d_small);
    if (g_items) k_set_classify<true><<<g_items, SET_BLOCK, 0, stream>>>(a, d_items);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(D.ev[2], stream));
    HIPCHK(hipMemcpyAsync(D.hout.p, D.out.p, out_bytes, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    const char *ho = D.hout.p;
    int32_t bad_key;
    uint64_t total;
    std::memcpy(&bad_key, ho + o_err, 4);
    std::memcpy(&total, ho + o_total, 8);
    if (bad_key) return lc::fail(LC_E_INVALID, "lc_set_check: key %d: an id at or past the key's span, or a bad class byte", bad_key - 1);
    std::memcpy(r->counts, ho + o_counts, nk * 48);
    std::memcpy(r->run_off, ho + o_run_off, (4 * nk + 1) * 8);
    std::memcpy(r->valid, ho + o_valid, nk);
    r->n_runs = total;
    if (total > r->run_cap)
        return lc::fail(LC_E_NOMEM, "lc_set_check: %llu runs, run_cap %llu: call again with run_cap >= %llu",
                        (unsigned long long)total, (unsigned long long)r->run_cap, (unsigned long long)total);
    if (total) HIPCHK(hipMemcpyAsync(r->runs, D.runs.p, total * 16, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipEventRecord(D.ev[3], stream));
    HIPCHK(hipStreamSynchronize(stream));
    float f = 0;
    for (int i = 0; i < 3; ++i) {
        HIPCHK(hipEventElapsedTime(&f, D.ev[i], D.ev[i + 1]));
        D.ms[i] = f;
    }
    D.ms[3] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    return LC_OK;
}

}  // namespace lcs
