// device_queue.hip -- jepsen.checker/total-queue and /unique-ids on the device:
// the kernels (include/lincheck_queue.h has the rules).
//
// Both checkers tally a multiset of values per key and classify every distinct
// value from its counts.  The tally is a concurrent hash table in HBM, open-
// addressed with linear probing, 16 bytes per slot: {rep, tally[3]}.
//
//   k_queue_reset     one slot per lane: rep = QP_EMPTY and the tallies 0 in
//                     one 16-byte store; the per-key counts, the range words
//                     and the out words in the same launch.
//   k_queue_tally     one row per lane.  A slot's word holds THE INDEX OF A
//                     REPRESENTATIVE ROW, not the value: a lane claims an
//                     empty slot with one returning compare-and-swap
//                     (QP_EMPTY -> its row index), and a lane that finds the
//                     slot taken compares its (key id, value) with
//                     row_key[rep] and row_val[rep].  Those are input arrays
//                     that no kernel writes, so plain loads are right and
//                     nothing has to be published between the claim and a
//                     payload: the 96-bit identity needs no wide atomic and no
//                     sentinel value, and every int64 is a legal value.  A
//                     failed swap returns the occupant, which is used without
//                     another load.  The slot word itself, which other CUs
//                     write, is read with a relaxed agent-scope atomic load (a
//                     plain load may be served from this CU's L1).  On a match
//                     or a claim: one no-return add on tally[kind].  THE PROBE
//                     LOOP IS BOUNDED BY `slots`: a lane that has visited
//                     every slot sets the error word and stops, so no input
//                     can spin a wave.  With slots >= n_rows, which the host
//                     enforces, that cannot happen: a batch has at most one
//                     distinct (key, value) per row.
//   k_queue_classify  one slot per lane.  An occupied slot computes its class
//                     multiplicities (total-queue) or count > 1 (unique-ids).
//                     The counts are reduced before they reach the key's
//                     global words: a wave whose occupied slots share one key
//                     sums by shuffles, a workgroup whose waves share it sums
//                     those through LDS and adds once per word; only a wave
//                     that holds several keys adds per lane.  The entries: a
//                     workgroup scan of the lanes' entry counts, one returning
//                     add per workgroup on the cursor, and the entries past
//                     ent_cap are counted and not written.
// Ordering is by kernel boundaries on one stream.

#include <hip/hip_runtime.h>

#include "device_queue.hpp"
#include "queue_plan.hpp"

namespace lcq {

namespace {

typedef unsigned long long u64;

constexpr int N_RED = LC_QN_COUNTS + 2;  // the seven counts, then the range's lo and hi
constexpr int WAVES = QP_BLOCK / 64;

__device__ inline uint32_t slot_hash(uint32_t key, int64_t val) {
    u64 x = (u64)val ^ ((u64)key * 0x9E3779B97F4A7C15ull);
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return (uint32_t)x ^ (uint32_t)(x >> 32);
}

__global__ __launch_bounds__(QP_BLOCK) void k_queue_reset(QueueArgs a) {
    const u64 gid = (u64)blockIdx.x * QP_BLOCK + threadIdx.x, total = (u64)gridDim.x * QP_BLOCK;
    if (gid < a.slots) a.table[gid] = make_uint4(QP_EMPTY, 0u, 0u, 0u);
    for (u64 k = gid; k < a.K; k += total) {
#pragma unroll
        for (int i = 0; i < LC_QN_COUNTS; ++i) a.counts[k * LC_QN_COUNTS + i] = 0;
        a.lo[k] = INT64_MAX;
        a.hi[k] = INT64_MIN;
    }
    if (gid < QO_WORDS) a.out[gid] = 0;
}

__global__ __launch_bounds__(QP_BLOCK) void k_queue_tally(QueueArgs a) {
    const u64 r = (u64)blockIdx.x * QP_BLOCK + threadIdx.x;
    if (r >= a.n_rows) return;
    const uint32_t key = a.row_key[r], kind = a.row_kind[r];
    const bool kind_ok = a.mode == LC_QM_UNIQUE_IDS ? kind == LC_QK_ACK : kind <= LC_QK_DEQUEUE;
    if (key >= a.K || !kind_ok) {
        atomicOr(&a.out[QO_ERR], QE_BAD_ROW);
        return;
    }
    if (a.status[key] != LC_QUEUE_KEY_OK) return;
    const int64_t val = a.row_val[r];
    const uint32_t mask = a.slots - 1, me = (uint32_t)r;
    uint32_t slot = slot_hash(key, val) & mask;
    for (uint32_t seen = 0; seen < a.slots; ++seen) {
        uint32_t *w = reinterpret_cast<uint32_t *>(a.table + slot);
        uint32_t rep = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (rep == QP_EMPTY) {
            rep = atomicCAS(w, QP_EMPTY, me);
            if (rep == QP_EMPTY) rep = me;
        }
        // rep is a row index of this batch: only those are ever swapped in
        if (rep == me || (a.row_key[rep] == key && a.row_val[rep] == val)) {
            __hip_atomic_fetch_add(w + 1 + kind, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        slot = (slot + 1) & mask;
    }
    atomicOr(&a.out[QO_ERR], QE_FULL);
}

__device__ inline u64 wave_sum(u64 v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ inline long long wave_min(long long v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const long long o = __shfl_xor(v, d, 64);
        v = o < v ? o : v;
    }
    return v;
}
__device__ inline long long wave_max(long long v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const long long o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

// Word i of key k's reduced record into the key's global words.
__device__ inline void add_word(const QueueArgs &a, uint32_t k, int i, u64 v) {
    if (i < LC_QN_COUNTS) {
        if (v) __hip_atomic_fetch_add(&a.counts[(u64)k * LC_QN_COUNTS + i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else if (a.mode == LC_QM_UNIQUE_IDS) {
        if (i == LC_QN_COUNTS) __hip_atomic_fetch_min(&a.lo[k], (long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else __hip_atomic_fetch_max(&a.hi[k], (long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(QP_BLOCK) void k_queue_classify(QueueArgs a) {
    __shared__ u64 sh_red[WAVES][N_RED];
    __shared__ uint32_t sh_key[WAVES], sh_flag[WAVES], sh_ent[WAVES];
    __shared__ u64 sh_base;
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const u64 gid = (u64)blockIdx.x * QP_BLOCK + threadIdx.x;

    uint4 s = make_uint4(QP_EMPTY, 0u, 0u, 0u);
    if (gid < a.slots) s = a.table[gid];
    const bool occ = s.x != QP_EMPTY;
    uint32_t key = 0;
    int64_t val = 0;
    if (occ) {
        key = a.row_key[s.x];
        val = a.row_val[s.x];
    }
    // this slot's record: the seven counts, and its multiplicity in the four listed classes
    u64 v[LC_QN_COUNTS] = {0, 0, 0, 0, 0, 0, 0};
    u64 m[4] = {0, 0, 0, 0};
    if (occ) {
        const u64 at = s.y, en = s.z, de = s.w;
        if (a.mode == LC_QM_UNIQUE_IDS) {
            v[LC_QN_ACKNOWLEDGED] = en;
            v[LC_QN_OK] = en > 1;
            m[LC_QC_DUPLICATED] = en > 1 ? en : 0;
        } else {
            const u64 ok = de < at ? de : at;
            v[LC_QN_ATTEMPT] = at;
            v[LC_QN_ACKNOWLEDGED] = en;
            v[LC_QN_OK] = ok;
            v[LC_QN_UNEXPECTED] = m[LC_QC_UNEXPECTED] = at == 0 ? de : 0;
            v[LC_QN_DUPLICATED] = m[LC_QC_DUPLICATED] = at > 0 && de > at ? de - at : 0;
            v[LC_QN_LOST] = m[LC_QC_LOST] = en > de ? en - de : 0;
            v[LC_QN_RECOVERED] = m[LC_QC_RECOVERED] = ok > en ? ok - en : 0;
        }
    }
    const uint32_t n_ent = (m[0] != 0) + (m[1] != 0) + (m[2] != 0) + (m[3] != 0);

    // the wave: do its occupied slots share one key?
    const u64 occ_mask = __ballot(occ);
    uint32_t flag = 0, wkey = 0;  // 0 nothing occupied, 1 one key, 2 several
    if (occ_mask) {
        wkey = __shfl(key, __ffsll((long long)occ_mask) - 1, 64);
        flag = __all(!occ || key == wkey) ? 1 : 2;
    }
    if (flag == 1) {
#pragma unroll
        for (int i = 0; i < LC_QN_COUNTS; ++i) {
            const u64 t = wave_sum(v[i]);
            if (lane == 0) sh_red[w][i] = t;
        }
        const long long lo = wave_min(occ ? (long long)val : INT64_MAX), hi = wave_max(occ ? (long long)val : INT64_MIN);
        if (lane == 0) {
            sh_red[w][LC_QN_COUNTS] = (u64)lo;
            sh_red[w][LC_QN_COUNTS + 1] = (u64)hi;
        }
    }
    // the wave's inclusive scan of the entry counts
    uint32_t inc = n_ent;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t p = __shfl_up(inc, d, 64);
        if (lane >= (uint32_t)d) inc += p;
    }
    if (lane == 63) sh_ent[w] = inc;
    if (lane == 0) {
        sh_key[w] = wkey;
        sh_flag[w] = flag;
    }
    __syncthreads();

    // the workgroup: do its waves share that key?
    bool have = false, mixed = false;
    uint32_t bkey = 0, ent_before = 0, ent_total = 0;
#pragma unroll
    for (int i = 0; i < WAVES; ++i) {
        if (sh_flag[i] == 2) mixed = true;
        else if (sh_flag[i] == 1) {
            if (have && sh_key[i] != bkey) mixed = true;
            if (!have) bkey = sh_key[i];
            have = true;
        }
        if (i < (int)w) ent_before += sh_ent[i];
        ent_total += sh_ent[i];
    }
    if (threadIdx.x == 0)
        sh_base = ent_total ? __hip_atomic_fetch_add(&a.out[QO_N_ENT], (u64)ent_total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
    if (!mixed) {
        if (have && threadIdx.x < N_RED) {
            const int i = (int)threadIdx.x;
            u64 t = 0;
            long long lo = INT64_MAX, hi = INT64_MIN;
#pragma unroll
            for (int j = 0; j < WAVES; ++j) {
                if (sh_flag[j] != 1) continue;
                const u64 x = sh_red[j][i];
                t += x;
                lo = (long long)x < lo ? (long long)x : lo;
                hi = (long long)x > hi ? (long long)x : hi;
            }
            add_word(a, bkey, i, i < LC_QN_COUNTS ? t : i == LC_QN_COUNTS ? (u64)lo : (u64)hi);
        }
    } else if (flag == 1) {
        if (lane < N_RED) add_word(a, wkey, (int)lane, sh_red[w][lane]);
    } else if (flag == 2 && occ) {
#pragma unroll
        for (int i = 0; i < LC_QN_COUNTS; ++i) add_word(a, key, i, v[i]);
        add_word(a, key, LC_QN_COUNTS, (u64)val);
        add_word(a, key, LC_QN_COUNTS + 1, (u64)val);
    }
    __syncthreads();

    if (n_ent) {
        u64 pos = sh_base + ent_before + (inc - n_ent);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (!m[c]) continue;
            if (pos < a.ent_cap) {
                a.ent_key[pos] = key;
                a.ent_class[pos] = (uint8_t)c;
                a.ent_val[pos] = val;
                a.ent_mult[pos] = m[c];
            }
            ++pos;
        }
    }
}

}  // namespace

hipError_t queue_launch(hipStream_t stream, const QueueArgs &a) {
    const uint32_t slot_blocks = (uint32_t)qp_blocks(a.slots);
    hipLaunchKernelGGL(k_queue_reset, dim3(slot_blocks), dim3(QP_BLOCK), 0, stream, a);
    if (a.n_rows) hipLaunchKernelGGL(k_queue_tally, dim3((uint32_t)qp_blocks(a.n_rows)), dim3(QP_BLOCK), 0, stream, a);
    hipLaunchKernelGGL(k_queue_classify, dim3(slot_blocks), dim3(QP_BLOCK), 0, stream, a);
    return hipGetLastError();
}

}  // namespace lcq
