// device_rows.hip -- raw history rows grouped by key and paired by (key,
// process) on the device: the kernels and the steps that run them
// (device_rows.hpp has the contract, rows_plan.hpp the sizes; DESIGN.md
// section 3.18).
//
//   k_rows_clear   every slot of both tables to {empty, no row}
//   k_rows_claim   one lane per row.  A row whose key differs from the row
//                  before it (a run of one key claims once) finds the key's
//                  slot by linear probing from rp_hash, claiming an empty slot
//                  by a compare-and-swap of its key word, and lowers the
//                  slot's row to its own by a 64-bit atomicMin, which it skips
//                  when the row it reads there is already lower.  The same for
//                  its process in the second table.  A slot's key never
//                  changes once set and nobody waits for anybody: a lane that
//                  loses a swap reads the winner's key from the swap itself.
//   k_rows_first   (the next launch, so every minimum is final) each row reads
//                  its key's and its process's first row; the row that is one
//                  flags itself for the scan that numbers them.
//   k_rows_ids     each row's key and process index from the scan at those
//                  first rows; the first rows write the key list.
//   k_rows_gather, k_rows_link
//                  around the second sort: the process index of each position;
//                  then predecessor and successor from the sorted neighbours.
//   k_scan_tile / k_scan_carry / k_scan_apply
//                  rows_scan2, three launches as the counter kernels' scans.
// Every probe loop ends after at most `slots` steps; one that found neither its
// key nor an empty slot sets the error word.  Ordering is by kernel boundaries
// on one stream.  The two stable radix sorts are rocPRIM's.

#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "common.hpp"
#include "device_ctx.hpp"
#include "device_rows.hpp"
#include "rows_plan.hpp"

namespace lcr {

namespace {

typedef unsigned long long u64;

constexpr u64 EMPTY = 0x8000000000000000ull;  // LC_NO_KEY = LC_NO_PROCESS: no row is inserted under it
constexpr u64 NO_ROW = ~0ull;

struct Slot {
    u64 key, row;
};
static_assert(sizeof(Slot) == RP_SLOT_BYTES, "slot size");

__global__ __launch_bounds__(RP_BLOCK) void k_rows_clear(Slot *a, Slot *b, u64 slots) {
    const u64 i = (u64)blockIdx.x * RP_BLOCK + threadIdx.x;
    if (i >= slots) return;
    const ulonglong2 e = make_ulonglong2(EMPTY, NO_ROW);
    *reinterpret_cast<ulonglong2 *>(a + i) = e;
    if (b) *reinterpret_cast<ulonglong2 *>(b + i) = e;
}

__device__ inline void claim(Slot *tab, u64 mask, u64 key, u64 row, uint32_t *err) {
    u64 s = rp_hash(key) & mask;
    for (u64 step = 0; step <= mask; ++step, s = (s + 1) & mask) {
        u64 cur = __hip_atomic_load(&tab[s].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == EMPTY) {
            cur = atomicCAS(&tab[s].key, EMPTY, key);
            if (cur == EMPTY) cur = key;
        }
        if (cur != key) continue;
        if (__hip_atomic_load(&tab[s].row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > row) atomicMin(&tab[s].row, row);
        return;
    }
    atomicOr(err, 1u);
}

// The first row of `key`, which k_rows_claim has inserted.
__device__ inline uint32_t first_row_of(const Slot *tab, u64 mask, u64 key, uint32_t *err) {
    u64 s = rp_hash(key) & mask;
    for (u64 step = 0; step <= mask; ++step, s = (s + 1) & mask) {
        const u64 cur = tab[s].key;
        if (cur == key) return (uint32_t)tab[s].row;
        if (cur == EMPTY) break;
    }
    atomicOr(err, 1u);
    return RP_NONE;
}

struct GroupArgs {
    RowsIn in;
    Slot *ktab, *ptab;
    u64 mask;
    uint32_t *kfrow, *pfrow;  // [n] first row of the row's key / process, or RP_NONE
    ulonglong2 *sc;           // [n + 1]
    uint32_t *err;
};

__global__ __launch_bounds__(RP_BLOCK) void k_rows_claim(GroupArgs a) {
    const u64 r = (u64)blockIdx.x * RP_BLOCK + threadIdx.x;
    if (r >= a.in.n) return;
    if (a.in.key) {
        const u64 k = (u64)a.in.key[r];
        if (k != EMPTY && (r == 0 || (u64)a.in.key[r - 1] != k)) claim(a.ktab, a.mask, k, r, a.err);
    }
    if (a.in.process) {
        const u64 p = (u64)a.in.process[r];
        if (p != EMPTY && (r == 0 || (u64)a.in.process[r - 1] != p)) claim(a.ptab, a.mask, p, r, a.err);
    }
}

__global__ __launch_bounds__(RP_BLOCK) void k_rows_first(GroupArgs a) {
    const u64 r = (u64)blockIdx.x * RP_BLOCK + threadIdx.x;
    if (r >= a.in.n) return;
    uint32_t kf = RP_NONE, pf = RP_NONE;
    if (a.in.key) {
        const u64 k = (u64)a.in.key[r];
        if (k != EMPTY) kf = first_row_of(a.ktab, a.mask, k, a.err);
    }
    if (a.in.process) {
        const u64 p = (u64)a.in.process[r];
        if (p != EMPTY) pf = first_row_of(a.ptab, a.mask, p, a.err);
    }
    a.kfrow[r] = kf;
    a.pfrow[r] = pf;
    a.sc[r] = make_ulonglong2(kf == (uint32_t)r, pf == (uint32_t)r);
}

struct IdsArgs {
    RowsIn in;
    const uint32_t *kfrow, *pfrow;
    const ulonglong2 *sc;
    uint32_t keyed, n_keys;
    uint32_t *kidx, *pidx, *rowid;  // [n]
    int64_t *keys;                  // [n_keys]
    uint32_t *first_row;            // [n_keys]
};

__global__ __launch_bounds__(RP_BLOCK) void k_rows_ids(IdsArgs a) {
    const u64 r = (u64)blockIdx.x * RP_BLOCK + threadIdx.x;
    if (r >= a.in.n) return;
    const uint32_t kf = a.kfrow[r], pf = a.pfrow[r];
    bool part = a.in.takes[r] != 0;
    if (a.in.process && pf == RP_NONE) part = false;
    if (a.keyed && kf == RP_NONE) part = false;
    uint32_t k = a.n_keys;
    if (part) k = a.keyed ? (uint32_t)a.sc[kf].x : 0u;
    a.kidx[r] = k;
    a.pidx[r] = pf == RP_NONE ? 0u : (uint32_t)a.sc[pf].y;
    a.rowid[r] = (uint32_t)r;
    if (a.keyed) {
        if (kf == (uint32_t)r) {
            const u64 i = a.sc[r].x;
            a.keys[i] = a.in.key[r];
            a.first_row[i] = (uint32_t)r;
        }
    } else if (r == 0) {
        a.keys[0] = (int64_t)EMPTY;
        a.first_row[0] = 0;
    }
}

__global__ __launch_bounds__(RP_BLOCK) void k_rows_gather(const uint32_t *pidx, const uint32_t *pos_row, uint32_t n, uint32_t *pkey,
                                                         uint32_t *pos) {
    const u64 j = (u64)blockIdx.x * RP_BLOCK + threadIdx.x;
    if (j >= n) return;
    pkey[j] = pidx[pos_row[j]];
    pos[j] = (uint32_t)j;
}

__global__ __launch_bounds__(RP_BLOCK) void k_rows_link(const uint32_t *sorted_p, const uint32_t *sorted_pos, const uint32_t *pos_key,
                                                       uint32_t n, uint32_t n_keys, uint32_t *prev, uint32_t *next) {
    const u64 i = (u64)blockIdx.x * RP_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t j = sorted_pos[i], k = pos_key[j], p = sorted_p[i];
    uint32_t pv = RP_NONE, nx = RP_NONE;
    if (k != n_keys) {
        if (i > 0 && sorted_p[i - 1] == p) {
            const uint32_t q = sorted_pos[i - 1];
            if (pos_key[q] == k) pv = q;
        }
        if (i + 1 < n && sorted_p[i + 1] == p) {
            const uint32_t q = sorted_pos[i + 1];
            if (pos_key[q] == k) nx = q;
        }
    }
    prev[j] = pv;
    next[j] = nx;
}

// The workgroup's exclusive scan of one pair per thread: (x, y) become the sums of the threads before, (tx, ty) the workgroup's.
__device__ inline void block_scan2(u64 &x, u64 &y, u64 &tx, u64 &ty, u64 *sh_x, u64 *sh_y) {
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    u64 ix = x, iy = y;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u64 px = __shfl_up(ix, d, 64), py = __shfl_up(iy, d, 64);
        if (lane >= (uint32_t)d) {
            ix += px;
            iy += py;
        }
    }
    if (lane == 63) {
        sh_x[w] = ix;
        sh_y[w] = iy;
    }
    __syncthreads();
    u64 bx = 0, by = 0;
    tx = 0;
    ty = 0;
#pragma unroll
    for (uint32_t i = 0; i < RP_BLOCK / 64; ++i) {
        if (i == w) {
            bx = tx;
            by = ty;
        }
        tx += sh_x[i];
        ty += sh_y[i];
    }
    x = bx + ix - x;
    y = by + iy - y;
    __syncthreads();  // sh is free again
}

__global__ __launch_bounds__(RP_BLOCK) void k_scan_tile(const ulonglong2 *a, u64 n, ulonglong2 *sums) {
    __shared__ u64 sh_x[RP_BLOCK / 64], sh_y[RP_BLOCK / 64];
    const u64 base = (u64)blockIdx.x * RP_TILE + (u64)threadIdx.x * RP_IPT;
    u64 x = 0, y = 0, tx, ty;
#pragma unroll
    for (uint32_t j = 0; j < RP_IPT; ++j)
        if (base + j < n) {
            const ulonglong2 v = a[base + j];
            x += v.x;
            y += v.y;
        }
    block_scan2(x, y, tx, ty, sh_x, sh_y);
    if (threadIdx.x == 0) sums[blockIdx.x] = make_ulonglong2(tx, ty);
}

// One workgroup: the tile sums to the sums of the tiles before, RP_BLOCK tiles at a time; the grand totals to *total.
__global__ __launch_bounds__(RP_BLOCK) void k_scan_carry(ulonglong2 *sums, u64 tiles, ulonglong2 *total) {
    __shared__ u64 sh_x[RP_BLOCK / 64], sh_y[RP_BLOCK / 64];
    u64 run_x = 0, run_y = 0;
    for (u64 c0 = 0; c0 < tiles; c0 += RP_BLOCK) {
        const u64 i = c0 + threadIdx.x;
        const bool have = i < tiles;
        const ulonglong2 v = have ? sums[i] : make_ulonglong2(0, 0);
        u64 x = v.x, y = v.y, tx, ty;
        block_scan2(x, y, tx, ty, sh_x, sh_y);
        if (have) sums[i] = make_ulonglong2(run_x + x, run_y + y);
        run_x += tx;
        run_y += ty;
    }
    if (threadIdx.x == 0) *total = make_ulonglong2(run_x, run_y);
}

__global__ __launch_bounds__(RP_BLOCK) void k_scan_apply(ulonglong2 *a, u64 n, const ulonglong2 *sums) {
    __shared__ u64 sh_x[RP_BLOCK / 64], sh_y[RP_BLOCK / 64];
    const u64 base = (u64)blockIdx.x * RP_TILE + (u64)threadIdx.x * RP_IPT;
    ulonglong2 v[RP_IPT];
    u64 x = 0, y = 0, tx, ty;
#pragma unroll
    for (uint32_t j = 0; j < RP_IPT; ++j) {
        v[j] = base + j < n ? a[base + j] : make_ulonglong2(0, 0);
        x += v[j].x;
        y += v[j].y;
    }
    block_scan2(x, y, tx, ty, sh_x, sh_y);
    const ulonglong2 c = sums[blockIdx.x];
    x += c.x;
    y += c.y;
#pragma unroll
    for (uint32_t j = 0; j < RP_IPT; ++j) {
        if (base + j < n) a[base + j] = make_ulonglong2(x, y);
        x += v[j].x;
        y += v[j].y;
    }
}

}  // namespace

struct Rows {
    enum { KTAB, PTAB, KFROW, PFROW, SC, KIDX, PIDX, ROWID, KEYS, FIRST, POS_KEY, POS_ROW, PKEY, POS, SORTED_P, SORTED_POS, PREV, NEXT,
           SORT_TMP, SUMS, ERR, N_MEM };
    lcx::DevBatch::Mem mem[N_MEM];
    unsigned long long *hout = nullptr;  // pinned landing: the totals (2 words), the error word
    size_t hout_cap = 0;
    // the batch of the last rows_group
    RowsIn in{};
    uint64_t n_keys = 0, n_procs = 0;
    uint32_t *kfrow = nullptr, *pfrow = nullptr, *err = nullptr;
    ulonglong2 *sc = nullptr;
    ~Rows() {
        for (lcx::DevBatch::Mem &m : mem)
            if (m.p) (void)hipFree(m.p);
        if (hout) (void)hipHostFree(hout);
    }
};

int rows_open(Rows **out) {
    *out = new (std::nothrow) Rows();
    return *out ? LC_OK : lc::fail(LC_E_NOMEM, "rows_open: out of memory");
}

void rows_close(Rows *r) { delete r; }

int rows_scan2(Rows *R, hipStream_t stream, ulonglong2 *a, uint64_t n) {
    const uint64_t tiles = rp_tiles(n);
    ulonglong2 *sums;
    HIPCHK(lcx::grow(R->mem[Rows::SUMS], sums, (size_t)tiles));
    if (tiles) k_scan_tile<<<(uint32_t)tiles, RP_BLOCK, 0, stream>>>(a, n, sums);
    k_scan_carry<<<1, RP_BLOCK, 0, stream>>>(sums, tiles, a + n);
    if (tiles) k_scan_apply<<<(uint32_t)tiles, RP_BLOCK, 0, stream>>>(a, n, sums);
    HIPCHK(hipGetLastError());
    return LC_OK;
}

int rows_group(Rows *R, hipStream_t stream, const RowsIn &in, uint64_t *n_keys, uint64_t *n_procs) {
    if (in.n == 0 || in.n > RP_MAX_ROWS) return lc::fail(LC_E_INVALID, "rows_group: %u rows", in.n);
    const size_t n = in.n;
    const uint64_t slots = rp_slots(n);
    const uint32_t blocks = (uint32_t)rp_blocks(n);
    GroupArgs a{};
    a.in = in;
    a.mask = slots - 1;
    HIPCHK(lcx::grow_pinned(R->hout, R->hout_cap, (size_t)4));
    if (in.key) HIPCHK(lcx::grow(R->mem[Rows::KTAB], a.ktab, (size_t)slots));
    if (in.process) HIPCHK(lcx::grow(R->mem[Rows::PTAB], a.ptab, (size_t)slots));
    HIPCHK(lcx::grow(R->mem[Rows::KFROW], a.kfrow, n));
    HIPCHK(lcx::grow(R->mem[Rows::PFROW], a.pfrow, n));
    HIPCHK(lcx::grow(R->mem[Rows::SC], a.sc, n + 1));
    HIPCHK(lcx::grow(R->mem[Rows::ERR], a.err, (size_t)1));
    HIPCHK(hipMemsetAsync(a.err, 0, 4, stream));
    if (a.ktab || a.ptab) {
        Slot *t0 = a.ktab ? a.ktab : a.ptab, *t1 = a.ktab ? a.ptab : nullptr;
        k_rows_clear<<<(uint32_t)rp_blocks(slots), RP_BLOCK, 0, stream>>>(t0, t1, slots);
        k_rows_claim<<<blocks, RP_BLOCK, 0, stream>>>(a);
    }
    k_rows_first<<<blocks, RP_BLOCK, 0, stream>>>(a);
    HIPCHK(hipGetLastError());
    LCCHK(rows_scan2(R, stream, a.sc, n));
    HIPCHK(hipMemcpyAsync(R->hout, a.sc + n, 16, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(R->hout + 2, a.err, 4, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    if ((uint32_t)R->hout[2]) return lc::fail(LC_E_DEVICE, "rows_group: a probe overran its table");
    R->in = in;
    R->n_keys = R->hout[0];
    R->n_procs = R->hout[1];
    R->kfrow = a.kfrow; R->pfrow = a.pfrow; R->sc = a.sc; R->err = a.err;
    *n_keys = R->n_keys;
    *n_procs = R->n_procs;
    return LC_OK;
}

namespace {

int sort_pairs(Rows *R, hipStream_t stream, const uint32_t *k_in, uint32_t *k_out, const uint32_t *v_in, uint32_t *v_out, size_t n,
               uint32_t bits) {
    size_t bytes = 0;
    HIPCHK(rocprim::radix_sort_pairs(nullptr, bytes, k_in, k_out, v_in, v_out, n, 0u, bits, stream));
    char *tmp;
    HIPCHK(lcx::grow(R->mem[Rows::SORT_TMP], tmp, bytes));
    HIPCHK(rocprim::radix_sort_pairs((void *)tmp, bytes, k_in, k_out, v_in, v_out, n, 0u, bits, stream));
    return LC_OK;
}

}  // namespace

int rows_pair(Rows *R, hipStream_t stream, RowsView *out) {
    const size_t n = R->in.n;
    const uint32_t blocks = (uint32_t)rp_blocks(n);
    const bool keyed = R->n_keys != 0;
    const uint32_t K = keyed ? (uint32_t)R->n_keys : 1u;
    const uint32_t key_bits = rp_bits(K), proc_bits = rp_bits(R->n_procs ? R->n_procs - 1 : 0);
    if (key_bits > RP_SORT_BITS_MAX || proc_bits > RP_SORT_BITS_MAX) return lc::fail(LC_E_INVALID, "rows_pair: sort bits");
    IdsArgs a{};
    a.in = R->in; a.kfrow = R->kfrow; a.pfrow = R->pfrow; a.sc = R->sc;
    a.keyed = keyed; a.n_keys = K;
    uint32_t *pos_key, *pos_row, *pkey, *pos, *sorted_p, *sorted_pos, *prev, *next;
    HIPCHK(lcx::grow(R->mem[Rows::KIDX], a.kidx, n));
    HIPCHK(lcx::grow(R->mem[Rows::PIDX], a.pidx, n));
    HIPCHK(lcx::grow(R->mem[Rows::ROWID], a.rowid, n));
    HIPCHK(lcx::grow(R->mem[Rows::KEYS], a.keys, (size_t)K));
    HIPCHK(lcx::grow(R->mem[Rows::FIRST], a.first_row, (size_t)K));
    HIPCHK(lcx::grow(R->mem[Rows::POS_KEY], pos_key, n));
    HIPCHK(lcx::grow(R->mem[Rows::POS_ROW], pos_row, n));
    HIPCHK(lcx::grow(R->mem[Rows::PKEY], pkey, n));
    HIPCHK(lcx::grow(R->mem[Rows::POS], pos, n));
    HIPCHK(lcx::grow(R->mem[Rows::SORTED_P], sorted_p, n));
    HIPCHK(lcx::grow(R->mem[Rows::SORTED_POS], sorted_pos, n));
    HIPCHK(lcx::grow(R->mem[Rows::PREV], prev, n));
    HIPCHK(lcx::grow(R->mem[Rows::NEXT], next, n));
    k_rows_ids<<<blocks, RP_BLOCK, 0, stream>>>(a);
    HIPCHK(hipGetLastError());
    LCCHK(sort_pairs(R, stream, a.kidx, pos_key, a.rowid, pos_row, n, key_bits));
    k_rows_gather<<<blocks, RP_BLOCK, 0, stream>>>(a.pidx, pos_row, (uint32_t)n, pkey, pos);
    HIPCHK(hipGetLastError());
    LCCHK(sort_pairs(R, stream, pkey, sorted_p, pos, sorted_pos, n, proc_bits));
    k_rows_link<<<blocks, RP_BLOCK, 0, stream>>>(sorted_p, sorted_pos, pos_key, (uint32_t)n, K, prev, next);
    HIPCHK(hipGetLastError());
    out->n = (uint32_t)n; out->n_keys = K; out->keyed = keyed;
    out->keys = a.keys; out->first_row = a.first_row;
    out->pos_key = pos_key; out->pos_row = pos_row; out->prev = prev; out->next = next;
    out->err = R->err;
    return LC_OK;
}

}  // namespace lcr
