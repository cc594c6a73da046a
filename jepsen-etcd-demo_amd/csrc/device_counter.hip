// device_counter.hip -- jepsen.checker/counter on the device: the kernels
// (include/lincheck_counter.h has the rules).
//
// Per key two running sums over its events in history order: `lower`, the
// :ok adds so far, and `upper`, the surviving :invoke adds so far.  A read's
// lower bound is `lower` at its :invoke, its upper bound `upper` at its :ok.
// Over the whole batch that is one SEGMENTED inclusive scan of two exact
// 64-bit sums (a segment per key) and a gather at the read events; then a
// plain scan over the reads counts those out of bounds and places their
// indices in order.
//
// Each scan is three launches (csrc/counter_plan.hpp has the tile arithmetic):
//   k_counter_tile    one workgroup per tile of events.  A thread holds
//                     consecutive events (eight at the default tile: their
//                     kinds one 8-byte load, their values four 16-byte loads);
//                     key heads are marked in an LDS bitmap from the offsets
//                     of the keys that start in the tile.  Writes the tile's
//                     two sums since its last head (or its start) and whether
//                     it holds a head, and one at its first event.
//   k_counter_carry   one workgroup: a segmented exclusive scan over the tile
//                     records, 256 tiles at a time with a running carry.
//                     Writes each tile's carry-in (zero where the tile starts
//                     a key).
//   k_counter_apply   per tile again, from the carry-in: stores lower at the
//                     read's index at an LC_CE_RINV event and upper at an
//                     LC_CE_ROK event.  No running sum leaves for any other
//                     event.
//   k_counter_judge_tile / k_counter_carry / k_counter_judge
//                     the same over the reads: the flag is
//                     !(lower <= value && value <= upper), the count series
//                     has no heads; k_counter_judge writes the flagged reads'
//                     indices at their ranks (ascending, so ascending inside
//                     every key) and err_off of the keys that start in its
//                     tile from the ranks in LDS.
// All sums are 64-bit integers: a wave's scan by shuffles, the four waves'
// through LDS.  Ordering is by kernel boundaries on one stream: no workgroup
// reads what another workgroup of the same launch writes.

#include <hip/hip_runtime.h>

#include "counter_plan.hpp"
#include "device_counter.hpp"

namespace lcc {

namespace {

typedef unsigned long long u64;

// (a, b, f): two sums and "a head lies in the span".  `p` before `x`.
__device__ inline void seg_join(u64 pa, u64 pb, uint32_t pf, u64 &a, u64 &b, uint32_t &f) {
    if (!f) {
        a += pa;
        b += pb;
    }
    f |= pf;
}

struct Scan {
    u64 ea, eb;   // exclusive: everything before this thread since the last head
    uint32_t ef;  // a head lies before this thread
    u64 ta, tb;   // the workgroup's
    uint32_t tf;
};

// The workgroup's segmented scan of one (a, b, f) per thread.  sh: 3 x 4 words of LDS.
__device__ inline Scan block_seg_scan(u64 a, u64 b, uint32_t f, u64 *sh_a, u64 *sh_b, uint32_t *sh_f) {
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u64 pa = __shfl_up(a, d, 64), pb = __shfl_up(b, d, 64);
        const uint32_t pf = __shfl_up(f, d, 64);
        if (lane >= (uint32_t)d) seg_join(pa, pb, pf, a, b, f);
    }
    if (lane == 63) {
        sh_a[w] = a;
        sh_b[w] = b;
        sh_f[w] = f;
    }
    // the wave's exclusive values: the lane before's inclusive ones
    u64 xa = __shfl_up(a, 1, 64), xb = __shfl_up(b, 1, 64);
    uint32_t xf = __shfl_up(f, 1, 64);
    if (lane == 0) {
        xa = 0;
        xb = 0;
        xf = 0;
    }
    __syncthreads();
    Scan s;
    u64 wa = 0, wb = 0;
    uint32_t wf = 0;
    s.ea = 0; s.eb = 0; s.ef = 0;
#pragma unroll
    for (uint32_t i = 0; i < CT_BLOCK / 64; ++i) {
        if (i == w) {  // the waves before this one
            s.ea = wa;
            s.eb = wb;
            s.ef = wf;
        }
        u64 na = sh_a[i], nb = sh_b[i];
        uint32_t nf = sh_f[i];
        seg_join(wa, wb, wf, na, nb, nf);
        wa = na;
        wb = nb;
        wf = nf;
    }
    s.ta = wa; s.tb = wb; s.tf = wf;
    seg_join(s.ea, s.eb, s.ef, xa, xb, xf);
    s.ea = xa; s.eb = xb; s.ef = xf;
    __syncthreads();  // sh is free again
    return s;
}

// The heads of tile t as an LDS bitmap of IPT * 256 bits; returns this thread's IPT bits.
template <int IPT>
__device__ inline uint32_t mark_heads(const CtSeries &s, uint64_t t, uint32_t *bits) {
    constexpr uint32_t TILE = IPT * CT_BLOCK;
    const uint64_t t0 = t * TILE;
    if (threadIdx.x < TILE / 32) bits[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t j1 = s.first[t + 1];
    for (uint64_t j = (uint64_t)s.first[t] + threadIdx.x; j < j1; j += CT_BLOCK) {
        if (j >= (uint64_t)s.K) continue;
        const uint64_t o = s.off[j];
        if (o >= s.n || o < t0 || o - t0 >= TILE) continue;
        atomicOr(&bits[(o - t0) >> 5], 1u << ((o - t0) & 31));
    }
    __syncthreads();
    const uint32_t at = threadIdx.x * IPT;
    return (bits[at >> 5] >> (at & 31)) & ((1u << IPT) - 1u);
}

// IPT consecutive values from `base`; `fill` at and past n.
template <int IPT>
__device__ inline void load_vals(const int64_t *p, uint64_t base, uint64_t n, int64_t fill, int64_t out[IPT]) {
    if (IPT % 2 == 0 && base + IPT <= n) {
#pragma unroll
        for (int q = 0; q < IPT / 2; ++q) {
            const longlong2 v = *reinterpret_cast<const longlong2 *>(p + base + 2 * q);
            out[2 * q] = v.x;
            out[2 * q + 1] = v.y;
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < IPT; ++j) out[j] = base + j < n ? p[base + j] : fill;
}

// IPT consecutive kinds from `base`; 0xFF (no event) at and past n.
template <int IPT>
__device__ inline void load_kinds(const uint8_t *p, uint64_t base, uint64_t n, uint8_t out[IPT]) {
    if (IPT == 8 && base + 8 <= n) {
        const uint64_t v = *reinterpret_cast<const uint64_t *>(p + base);
#pragma unroll
        for (int j = 0; j < IPT; ++j) out[j] = (uint8_t)(v >> (8 * j));
        return;
    }
#pragma unroll
    for (int j = 0; j < IPT; ++j) out[j] = base + j < n ? p[base + j] : (uint8_t)0xFF;
}

template <int IPT>
__global__ __launch_bounds__(CT_BLOCK) void k_counter_tile(CtEvents a) {
    __shared__ uint32_t bits[IPT * CT_BLOCK / 32];
    __shared__ u64 sh_a[CT_BLOCK / 64], sh_b[CT_BLOCK / 64];
    __shared__ uint32_t sh_f[CT_BLOCK / 64];
    const uint64_t t = blockIdx.x, base = t * (IPT * CT_BLOCK) + (uint64_t)threadIdx.x * IPT;
    const uint32_t hb = mark_heads<IPT>(a.s, t, bits);
    uint8_t kind[IPT];
    int64_t val[IPT];
    load_kinds<IPT>(a.kind, base, a.s.n, kind);
    load_vals<IPT>(a.val, base, a.s.n, 0, val);
    u64 lo = 0, up = 0;
#pragma unroll
    for (int j = 0; j < IPT; ++j) {
        if (hb >> j & 1) {
            lo = 0;
            up = 0;
        }
        if (kind[j] == LC_CE_UP) up += (u64)val[j];
        if (kind[j] == LC_CE_LOW) lo += (u64)val[j];
    }
    const Scan s = block_seg_scan(lo, up, hb != 0, sh_a, sh_b, sh_f);
    if (threadIdx.x == 0) {
        a.t.sum_a[t] = s.ta;
        a.t.sum_b[t] = s.tb;
        a.t.heads[t] = (uint8_t)((s.tf ? CT_HEAD_ANY : 0) | ((hb & 1) ? CT_HEAD_FIRST : 0));
    }
}

__global__ __launch_bounds__(CT_BLOCK) void k_counter_carry(CtTiles t, uint64_t tiles) {
    __shared__ u64 sh_a[CT_BLOCK / 64], sh_b[CT_BLOCK / 64];
    __shared__ uint32_t sh_f[CT_BLOCK / 64];
    u64 run_a = 0, run_b = 0;
    for (uint64_t c0 = 0; c0 < tiles; c0 += CT_CARRY_CHUNK) {
        const uint64_t i = c0 + threadIdx.x;
        const bool have = i < tiles;
        const u64 a = have ? t.sum_a[i] : 0, b = have ? t.sum_b[i] : 0;
        const uint8_t h = have ? t.heads[i] : (uint8_t)0;
        const Scan s = block_seg_scan(a, b, (h & CT_HEAD_ANY) != 0, sh_a, sh_b, sh_f);
        if (have) {
            const bool first = (h & CT_HEAD_FIRST) != 0;
            t.carry_a[i] = first ? 0 : s.ef ? s.ea : run_a + s.ea;
            t.carry_b[i] = first ? 0 : s.ef ? s.eb : run_b + s.eb;
        }
        run_a = s.tf ? s.ta : run_a + s.ta;
        run_b = s.tf ? s.tb : run_b + s.tb;
    }
}

template <int IPT>
__global__ __launch_bounds__(CT_BLOCK) void k_counter_apply(CtEvents a) {
    __shared__ uint32_t bits[IPT * CT_BLOCK / 32];
    __shared__ u64 sh_a[CT_BLOCK / 64], sh_b[CT_BLOCK / 64];
    __shared__ uint32_t sh_f[CT_BLOCK / 64];
    const uint64_t t = blockIdx.x, base = t * (IPT * CT_BLOCK) + (uint64_t)threadIdx.x * IPT;
    const uint32_t hb = mark_heads<IPT>(a.s, t, bits);
    uint8_t kind[IPT];
    int64_t val[IPT];
    load_kinds<IPT>(a.kind, base, a.s.n, kind);
    load_vals<IPT>(a.val, base, a.s.n, 0, val);
    u64 lo = 0, up = 0;
#pragma unroll
    for (int j = 0; j < IPT; ++j) {
        if (hb >> j & 1) {
            lo = 0;
            up = 0;
        }
        if (kind[j] == LC_CE_UP) up += (u64)val[j];
        if (kind[j] == LC_CE_LOW) lo += (u64)val[j];
    }
    const Scan s = block_seg_scan(lo, up, hb != 0, sh_a, sh_b, sh_f);
    // what reaches this thread's first event
    lo = s.ef ? s.ea : a.t.carry_a[t] + s.ea;
    up = s.ef ? s.eb : a.t.carry_b[t] + s.eb;
    bool bad = false;
#pragma unroll
    for (int j = 0; j < IPT; ++j) {
        if (hb >> j & 1) {
            lo = 0;
            up = 0;
        }
        const uint8_t k = kind[j];
        if (k == LC_CE_UP) {
            up += (u64)val[j];
        } else if (k == LC_CE_LOW) {
            lo += (u64)val[j];
        } else if (k == LC_CE_RINV || k == LC_CE_ROK) {
            const uint64_t idx = (uint64_t)val[j];
            if (idx >= a.R) bad = true;
            else if (k == LC_CE_RINV) a.lower[idx] = (int64_t)lo;
            else a.upper[idx] = (int64_t)up;
        } else if (base + j < a.s.n) {
            bad = true;
        }
    }
    if (bad) atomicOr(a.err, 1u);
}

// This thread's IPT reads of tile t: bit j set when read base + j is out of bounds.
template <int IPT>
__device__ inline uint32_t judge_flags(const CtJudge &a, uint64_t base) {
    int64_t v[IPT], lo[IPT], up[IPT];
    load_vals<IPT>(a.val, base, a.s.n, 0, v);
    load_vals<IPT>(a.lower, base, a.s.n, 0, lo);
    load_vals<IPT>(a.upper, base, a.s.n, 0, up);
    uint32_t fl = 0;
#pragma unroll
    for (int j = 0; j < IPT; ++j)
        if (base + j < a.s.n && !(lo[j] <= v[j] && v[j] <= up[j])) fl |= 1u << j;
    return fl;
}

template <int IPT>
__global__ __launch_bounds__(CT_BLOCK) void k_counter_judge_tile(CtJudge a) {
    __shared__ u64 sh_a[CT_BLOCK / 64], sh_b[CT_BLOCK / 64];
    __shared__ uint32_t sh_f[CT_BLOCK / 64];
    const uint64_t t = blockIdx.x, base = t * (IPT * CT_BLOCK) + (uint64_t)threadIdx.x * IPT;
    const uint32_t fl = judge_flags<IPT>(a, base);
    const Scan s = block_seg_scan((u64)__popc(fl), 0, 0, sh_a, sh_b, sh_f);
    if (threadIdx.x == 0) {
        a.t.sum_a[t] = s.ta;
        a.t.sum_b[t] = 0;
        a.t.heads[t] = 0;
    }
}

template <int IPT>
__global__ __launch_bounds__(CT_BLOCK) void k_counter_judge(CtJudge a) {
    constexpr uint32_t TILE = IPT * CT_BLOCK;
    __shared__ uint32_t rank[TILE + 1];  // flagged reads of the tile before each of its reads; [TILE]: all
    __shared__ u64 sh_a[CT_BLOCK / 64], sh_b[CT_BLOCK / 64];
    __shared__ uint32_t sh_f[CT_BLOCK / 64];
    const uint64_t t = blockIdx.x, t0 = t * TILE, base = t0 + (uint64_t)threadIdx.x * IPT;
    const uint32_t fl = judge_flags<IPT>(a, base);
    const Scan s = block_seg_scan((u64)__popc(fl), 0, 0, sh_a, sh_b, sh_f);
    const u64 before = a.t.carry_a[t];
    uint32_t r = (uint32_t)s.ea;
#pragma unroll
    for (int j = 0; j < IPT; ++j) {
        rank[threadIdx.x * IPT + j] = r;
        if (fl >> j & 1) {
            const u64 at = before + r;
            if (at < a.err_cap) a.err_idx[at] = base + j;
            ++r;
        }
    }
    if (threadIdx.x == 0) {
        rank[TILE] = (uint32_t)s.ta;
        if (t + 1 == a.s.tiles) *a.n_err = before + s.ta;
    }
    __syncthreads();
    // err_off of the offset entries of this tile (the last tile: those at n too, entry K among them)
    const uint64_t j1 = a.s.first[t + 1];
    for (uint64_t j = (uint64_t)a.s.first[t] + threadIdx.x; j < j1; j += CT_BLOCK) {
        if (j > (uint64_t)a.s.K) continue;
        const uint64_t o = a.s.off[j];
        if (o < t0 || o - t0 > TILE) continue;
        a.err_off[j] = before + rank[o - t0];
    }
}

}  // namespace

hipError_t counter_launch_events(hipStream_t stream, uint32_t tile, const CtEvents &a) {
    if (a.s.n == 0 || a.s.tiles == 0 || a.s.tiles > CT_MAX_TILES) return hipErrorInvalidValue;
    const dim3 grid((uint32_t)a.s.tiles), block(CT_BLOCK);
    if (tile == CT_TILE_DEFAULT) {
        k_counter_tile<8><<<grid, block, 0, stream>>>(a);
        k_counter_carry<<<1, block, 0, stream>>>(a.t, a.s.tiles);
        k_counter_apply<8><<<grid, block, 0, stream>>>(a);
    } else if (tile == CT_TILE_MIN) {
        k_counter_tile<1><<<grid, block, 0, stream>>>(a);
        k_counter_carry<<<1, block, 0, stream>>>(a.t, a.s.tiles);
        k_counter_apply<1><<<grid, block, 0, stream>>>(a);
    } else {
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t counter_launch_judge(hipStream_t stream, uint32_t tile, const CtJudge &a) {
    if (a.s.n == 0 || a.s.tiles == 0 || a.s.tiles > CT_MAX_TILES) return hipErrorInvalidValue;
    const dim3 grid((uint32_t)a.s.tiles), block(CT_BLOCK);
    if (tile == CT_TILE_DEFAULT) {
        k_counter_judge_tile<8><<<grid, block, 0, stream>>>(a);
        k_counter_carry<<<1, block, 0, stream>>>(a.t, a.s.tiles);
        k_counter_judge<8><<<grid, block, 0, stream>>>(a);
    } else if (tile == CT_TILE_MIN) {
        k_counter_judge_tile<1><<<grid, block, 0, stream>>>(a);
        k_counter_carry<<<1, block, 0, stream>>>(a.t, a.s.tiles);
        k_counter_judge<1><<<grid, block, 0, stream>>>(a);
    } else {
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace lcc
