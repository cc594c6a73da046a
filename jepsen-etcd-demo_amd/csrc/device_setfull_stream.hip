// device_setfull_stream.hip -- the device half of a streaming set-full
// (lc_setfull_stream_*; include/lincheck_setfull_stream.h has the contract,
// DESIGN.md section 3.13 the design).  A library of its own,
// lincheck/libsetfull_stream_kernels.so, which liblincheck.so links by its own
// directory (the Makefile says why); lc::fail and the context's lane join
// resolve from liblincheck.so.
//
// RESIDENT, per element id, one RECORD in HBM between calls: the position of
// the last :invoke :add (inv), of the first :ok :add since (ack, with its
// time), and the fold's three ops as (position, time) pairs -- known,
// last-present, last-absent -- with the outcome, latency and duplicated flag
// derived from them.  Records are struct-of-arrays over SLOTS; a block of 256
// slots belongs to one key and is one fold workgroup; each block has its own
// six partial counts.
//
// Per append (one chunk of the packer, host_setfull_stream.cpp):
//   k_sfs_reset   one lane per entry.  FRESH: the record starts over at the
//                 entry's invocation with known / last-present / last-absent
//                 nil.  ACK: the id's ack position and time (the packer sends
//                 only the first since the invocation).
//   k_sfs_mark    the chunk's read lists to bits of a presence matrix (new
//                 rows x the key's ids), one workgroup per (row, 1,024 read
//                 elements), one 16-byte load of ids per lane and an atomicOr
//                 per element, whose old value flags a duplicate.  An id at
//                 or past the key's count marks nothing and names its key in
//                 the error word.
//   k_sfs_fold    one lane per id, one wave per 64 ids: loads the record,
//                 merges the ack into known, walks the segment's rows reading
//                 one wave-uniform matrix word per row; a row counts when it
//                 completed after the invocation; bit set: last-present is
//                 the later invocation, known the earlier position; else
//                 last-absent.  Stores the record, classifies, and leaves the
//                 block's six counts in the block's own slot.
//   k_sfs_finish  one workgroup per touched key: its blocks' counts summed
//                 (no atomics), then :valid? by the one-shot rule order.
// A chunk above the matrix cap is folded in passes of whole rows
// (setfull_stream_plan.hpp): every update is a max or a first by position, so
// the passes compose.  Ordering is by kernel boundaries on the context's lane
// 0; nothing spins.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "device_ctx.hpp"
#include "device_setfull_stream.hpp"
#include "setfull_stream_plan.hpp"

namespace lcfs {

namespace {

constexpr int N_I64 = 10;  // inv, ack, ack_time, known (pos, time), last-present, last-absent, latency
enum { A_INV, A_ACK, A_ACKT, A_KN, A_KNT, A_LP, A_LPT, A_LA, A_LAT, A_MS };

struct SfsArgs {
    // resident
    int64_t *rec[N_I64];
    uint8_t *outcome, *dup;
    uint32_t *part;              // [6 * blocks]
    // the chunk
    const SfsSeg *segs;
    const uint32_t *blk;
    const uint64_t *tk_blk_off;  // [n_touched + 1]
    const uint32_t *en_slot, *en_flags;
    const int64_t *en_inv, *en_ack, *en_ackt;
    const int64_t *row_pos, *row_time, *row_inv_pos, *row_inv_time;
    const uint64_t *el_off;
    const uint32_t *read_id;
    const int64_t *tk_key;
    uint64_t *mat;
    unsigned long long *counts;  // [6 * n_touched]
    int8_t *valid;               // [n_touched]
    int32_t *err;                // 1 + a key with a bad id, or 0
    uint32_t n_entries;
    uint32_t linearizable;
};

__global__ __launch_bounds__(SFS_BLOCK) void k_sfs_reset(SfsArgs a) {
    const uint32_t i = blockIdx.x * SFS_BLOCK + threadIdx.x;
    if (i >= a.n_entries) return;
    const uint32_t slot = a.en_slot[i], fl = a.en_flags[i];
    if (fl & LC_SFS_FRESH) {
        a.rec[A_INV][slot] = a.en_inv[i];
        a.rec[A_ACK][slot] = LC_SETFULL_NONE;
        a.rec[A_ACKT][slot] = 0;
        a.rec[A_KN][slot] = LC_SETFULL_NONE;
        a.rec[A_KNT][slot] = 0;
        a.rec[A_LP][slot] = LC_SETFULL_NONE;
        a.rec[A_LPT][slot] = 0;
        a.rec[A_LA][slot] = LC_SETFULL_NONE;
        a.rec[A_LAT][slot] = 0;
    }
    if (fl & LC_SFS_ACK) {
        a.rec[A_ACK][slot] = a.en_ack[i];
        a.rec[A_ACKT][slot] = a.en_ackt[i];
    }
}

__global__ __launch_bounds__(SFS_BLOCK) void k_sfs_mark(SfsArgs a, const SfsMarkItem *items) {
    const SfsMarkItem it = items[blockIdx.x];
    const SfsSeg sg = a.segs[it.seg];
    const uint64_t row_b = a.el_off[it.row], row_e = a.el_off[it.row + 1];
    const uint64_t at = it.start + (uint64_t)threadIdx.x * SFS_MARK_LANE_ELS;
    uint32_t *M = reinterpret_cast<uint32_t *>(a.mat + sg.mbase + (it.row - sg.row0) * (uint64_t)sg.bw);
    // the lane's four elements in one 16-byte load (at is a multiple of four; the array is padded past its end)
    uint4 v = make_uint4(0, 0, 0, 0);
    if (at < row_e && at + SFS_MARK_LANE_ELS > row_b) v = *reinterpret_cast<const uint4 *>(a.read_id + at);
    const uint32_t ids[SFS_MARK_LANE_ELS] = {v.x, v.y, v.z, v.w};
    bool bad = false;
#pragma unroll
    for (uint32_t j = 0; j < SFS_MARK_LANE_ELS; ++j) {
        if (at + j < row_b || at + j >= row_e) continue;
        const uint32_t id = ids[j];
        if (id >= sg.n_ids) {
            bad = true;
            continue;
        }
        // (a lane's own atomics are ordered: the second of two equal ids in one load sees the first's bit)
        const uint32_t bit = 1u << (id & 31);
        if (atomicOr(M + (id >> 5), bit) & bit) a.dup[(uint64_t)a.blk[sg.blk_off + id / SFS_BLOCK_IDS] * SFS_BLOCK_IDS + id % SFS_BLOCK_IDS] = 1;
    }
    if (bad) atomicMax(a.err, (int32_t)a.tk_key[sg.t] + 1);
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

__global__ __launch_bounds__(SFS_BLOCK) void k_sfs_fold(SfsArgs a, const SfsFoldItem *items) {
    __shared__ uint64_t s6[SFS_BLOCK / 64][6];
    const SfsFoldItem it = items[blockIdx.x];
    const SfsSeg sg = a.segs[it.seg];
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t block = a.blk[sg.blk_off + it.j];
    const bool have = it.j * SFS_BLOCK_IDS + tid < sg.n_ids;
    const uint64_t slot = (uint64_t)block * SFS_BLOCK_IDS + tid;
    const int64_t I = have ? a.rec[A_INV][slot] : (int64_t)LC_SETFULL_NONE;
    const bool tracked = I >= 0;
    int64_t kn = LC_SETFULL_NONE, knt = 0, lp = LC_SETFULL_NONE, lpt = 0, la = LC_SETFULL_NONE, lat = 0;
    if (tracked) {
        kn = a.rec[A_KN][slot]; knt = a.rec[A_KNT][slot];
        lp = a.rec[A_LP][slot]; lpt = a.rec[A_LPT][slot];
        la = a.rec[A_LA][slot]; lat = a.rec[A_LAT][slot];
        const int64_t A = a.rec[A_ACK][slot];
        if (A >= 0 && (kn < 0 || A < kn)) {
            kn = A;
            knt = a.rec[A_ACKT][slot];
        }
    }
    // the wave's word of every row (the same in all 64 lanes)
    const uint32_t wv = __builtin_amdgcn_readfirstlane(it.j * SFS_BLOCK_WORDS + (tid >> 6));
    const uint64_t *W = a.mat + sg.mbase + wv;
    const uint64_t bw = sg.bw;
    const int64_t *row_pos = a.row_pos + sg.row0, *row_time = a.row_time + sg.row0;
    const int64_t *row_inv = a.row_inv_pos + sg.row0, *row_inv_time = a.row_inv_time + sg.row0;
    for (uint32_t r = 0; r < sg.n_rows; ++r) {
        const int64_t c = row_pos[r], i = row_inv[r];
        const uint64_t w = W[(uint64_t)r * bw];
        if (!tracked || c <= I) continue;  // the element was not tracked when the read completed
        if (w >> lane & 1) {
            if (i > lp) { lp = i; lpt = row_inv_time[r]; }
            if (kn < 0 || c < kn) { kn = c; knt = row_time[r]; }
        } else if (i > la) {
            la = i;
            lat = row_inv_time[r];
        }
    }
    const bool stable = lp >= 0 && la < lp;
    const bool lost = !stable && kn >= 0 && la >= 0 && lp < la && kn < la;
    const int64_t until = stable ? (la >= 0 ? lat + 1 : 0) : (lp >= 0 ? lpt + 1 : 0);
    int64_t ms = LC_SETFULL_NONE;
    if (stable || lost) ms = (until > knt ? until - knt : 0) / 1000000;
    uint32_t v[6] = {0, 0, 0, 0, 0, 0};
    if (have) {
        if (tracked) {
            a.rec[A_KN][slot] = kn; a.rec[A_KNT][slot] = knt;
            a.rec[A_LP][slot] = lp; a.rec[A_LPT][slot] = lpt;
            a.rec[A_LA][slot] = la; a.rec[A_LAT][slot] = lat;
        }
        a.outcome[slot] = !tracked ? LC_SETFULL_UNTRACKED : stable ? LC_SETFULL_STABLE : lost ? LC_SETFULL_LOST : LC_SETFULL_NEVER_READ;
        a.rec[A_MS][slot] = ms;
        v[0] = tracked;
        v[1] = stable;
        v[2] = lost;
        v[3] = tracked && !stable && !lost;
        v[4] = stable && ms > 0;
        v[5] = a.dup[slot] != 0;
    }
    uint64_t tot[6];
    block_sum6(v, tot, s6);
    if (tid < 6) a.part[6ull * block + tid] = (uint32_t)tot[tid];
}

__global__ __launch_bounds__(SFS_BLOCK) void k_sfs_finish(SfsArgs a) {
    __shared__ uint64_t s6[SFS_BLOCK / 64][6];
    const uint32_t t = blockIdx.x;
    uint32_t acc[6] = {0, 0, 0, 0, 0, 0};
    uint64_t tot[6] = {0, 0, 0, 0, 0, 0};
    // (a block's slot holds at most 256; a thread's share of 2^24 blocks fits 32 bits)
    for (uint64_t j = a.tk_blk_off[t] + threadIdx.x; j < a.tk_blk_off[t + 1]; j += SFS_BLOCK) {
        const uint64_t b = a.blk[j];
#pragma unroll
        for (int i = 0; i < 6; ++i) acc[i] += a.part[6 * b + i];
    }
    block_sum6(acc, tot, s6);
    if (threadIdx.x < 6) a.counts[6ull * t + threadIdx.x] = tot[threadIdx.x];
    if (threadIdx.x == 0) {
        int8_t v = LC_VALID;
        if (tot[2]) v = LC_INVALID;
        else if (!tot[1]) v = LC_UNKNOWN;
        else if (a.linearizable && tot[4]) v = LC_INVALID;
        if (tot[5]) v = LC_INVALID;
        a.valid[t] = v;
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

struct SfsDev {
    lc_ctx *ctx = nullptr;
    // resident: N_I64 arrays of cap_blocks * 256 int64, two of bytes, the blocks' counts
    uint64_t cap_blocks = 0;
    int64_t *rec = nullptr;
    uint8_t *bytes = nullptr;
    uint32_t *part = nullptr;
    // per chunk
    Buf in, mat, out;
    HostBuf hin, hout;
    std::vector<hipEvent_t> ev;
};

namespace {

// The resident arrays hold `need` blocks: grown by doubling, the old contents
// copied device to device, the new blocks' positions nil and flags 0.
int ensure_blocks(SfsDev &D, hipStream_t q, uint64_t need) {
    if (need <= D.cap_blocks) return LC_OK;
    const uint64_t cap = sfs_grow_blocks(D.cap_blocks, need);
    const size_t old_n = (size_t)D.cap_blocks * SFS_BLOCK_IDS, n = (size_t)cap * SFS_BLOCK_IDS;
    int64_t *rec = nullptr;
    uint8_t *bytes = nullptr;
    uint32_t *part = nullptr;
    hipError_t e = hipMalloc((void **)&rec, n * 8 * N_I64);
    if (e == hipSuccess) e = hipMalloc((void **)&bytes, n * 2);
    if (e == hipSuccess) e = hipMalloc((void **)&part, (size_t)cap * 24);
    for (int i = 0; i < N_I64 && e == hipSuccess; ++i) {
        if (old_n) e = hipMemcpyAsync(rec + (size_t)i * n, D.rec + (size_t)i * old_n, old_n * 8, hipMemcpyDeviceToDevice, q);
        if (e == hipSuccess) e = hipMemsetAsync(rec + (size_t)i * n + old_n, 0xFF, (n - old_n) * 8, q);
    }
    for (int i = 0; i < 2 && e == hipSuccess; ++i) {
        if (old_n) e = hipMemcpyAsync(bytes + (size_t)i * n, D.bytes + (size_t)i * old_n, old_n, hipMemcpyDeviceToDevice, q);
        if (e == hipSuccess) e = hipMemsetAsync(bytes + (size_t)i * n + old_n, 0, n - old_n, q);
    }
    if (e == hipSuccess && old_n) e = hipMemcpyAsync(part, D.part, (size_t)D.cap_blocks * 24, hipMemcpyDeviceToDevice, q);
    if (e == hipSuccess) e = hipMemsetAsync(part + 6 * (size_t)D.cap_blocks, 0, (size_t)(cap - D.cap_blocks) * 24, q);
    if (e == hipSuccess) e = hipStreamSynchronize(q);
    if (e != hipSuccess) {
        if (rec) (void)hipFree(rec);
        if (bytes) (void)hipFree(bytes);
        if (part) (void)hipFree(part);
        return lc::fail(LC_E_DEVICE, "lc_setfull_stream_append: growing the records to %llu blocks failed: %s",
                        (unsigned long long)cap, hipGetErrorString(e));
    }
    if (D.rec) (void)hipFree(D.rec);
    if (D.bytes) (void)hipFree(D.bytes);
    if (D.part) (void)hipFree(D.part);
    D.rec = rec; D.bytes = bytes; D.part = part;
    D.cap_blocks = cap;
    return LC_OK;
}

void fill_resident(const SfsDev &D, SfsArgs &a) {
    const size_t n = (size_t)D.cap_blocks * SFS_BLOCK_IDS;
    for (int i = 0; i < N_I64; ++i) a.rec[i] = D.rec + (size_t)i * n;
    a.outcome = D.bytes;
    a.dup = D.bytes + n;
    a.part = D.part;
}

}  // namespace

int sfs_dev_open(lc_ctx *c, SfsDev **out) {
    *out = nullptr;
    if (c->n_dev != 1 || c->comm)
        return lc::fail(LC_E_UNSUPPORTED, "lc_setfull_stream_open: a stream needs a context of one device and no communicator");
    SfsDev *d = new (std::nothrow) SfsDev();
    if (!d) return lc::fail(LC_E_NOMEM, "lc_setfull_stream_open: out of memory");
    d->ctx = c;
    *out = d;
    return LC_OK;
}

void sfs_dev_close(SfsDev *d) {
    if (!d) return;
    {
        std::lock_guard<std::mutex> g(d->ctx->mu);
        lcx::Dev *dev = d->ctx->dev[0];
        (void)hipSetDevice(dev->device);
        (void)hipStreamSynchronize(dev->stream);
        if (d->rec) (void)hipFree(d->rec);
        if (d->bytes) (void)hipFree(d->bytes);
        if (d->part) (void)hipFree(d->part);
        for (Buf *b : {&d->in, &d->mat, &d->out}) b->release();
        d->hin.release();
        d->hout.release();
        for (hipEvent_t e : d->ev)
            if (e) (void)hipEventDestroy(e);
    }
    delete d;
}

int sfs_dev_append(SfsDev *dp, const lc_setfull_stream_chunk *c, uint64_t n_blocks, int linearizable, uint64_t cap_bytes,
                   int8_t *valid, uint64_t *counts, double *ms5) {
    SfsDev &D = *dp;
    lcx::CtxCall x(D.ctx);
    LCCHK(x.enter());
    hipStream_t q = x.d->stream;
    const size_t T = (size_t)c->n_touched, n_en = (size_t)c->n_entries;
    const size_t n_rows = (size_t)c->tk_row_off[T], n_el = (size_t)c->el_off[n_rows], n_blk = (size_t)c->tk_blk_off[T];
    if (n_rows > 0x7FFFFFF0ull || n_en > 0x7FFFFFF0ull) return lc::fail(LC_E_INVALID, "lc_setfull_stream_append: more than 2^31 reads or adds in one append");
    LCCHK(ensure_blocks(D, q, n_blocks));

    SfsChunkIn in;
    in.n_touched = c->n_touched; in.n_ids = c->tk_n_ids; in.row_off = c->tk_row_off; in.blk_off = c->tk_blk_off;
    in.el_off = c->el_off; in.cap_bytes = cap_bytes ? cap_bytes : SFS_MATRIX_MAX_BYTES;
    SfsChunkPlan plan;
    try {
        plan = plan_sfs_chunk(in);
    } catch (const std::bad_alloc &) {
        return lc::fail(LC_E_NOMEM, "lc_setfull_stream_append: out of memory");
    }
    for (const SfsPass &p : plan.passes)
        if (p.mark1 - p.mark0 > 0x7FFFFFF0ull || p.fold1 - p.fold0 > 0x7FFFFFF0ull)
            return lc::fail(LC_E_INVALID, "lc_setfull_stream_append: more than 2^31 workgroups in one pass");
    while (D.ev.size() < 4 + 3 * plan.passes.size()) {
        hipEvent_t e = nullptr;
        HIPCHK(hipEventCreate(&e));
        D.ev.push_back(e);
    }

    // one input block, one copy
    Layout L;
    const size_t o_segs = L.take(plan.segs.size() * sizeof(SfsSeg)), o_marks = L.take(plan.marks.size() * sizeof(SfsMarkItem));
    const size_t o_folds = L.take(plan.folds.size() * sizeof(SfsFoldItem));
    const size_t o_blk_off = L.take((T + 1) * 8), o_tk_key = L.take(T * 8), o_blk = L.take(n_blk * 4);
    const size_t o_en_slot = L.take(n_en * 4), o_en_flags = L.take(n_en * 4);
    const size_t o_en_inv = L.take(n_en * 8), o_en_ack = L.take(n_en * 8), o_en_ackt = L.take(n_en * 8);
    const size_t o_rows = L.take(n_rows * 32), o_el_off = L.take((n_rows + 1) * 8);
    const size_t o_read_id = L.take(n_el * 4 + 16);  // (mark's last 16-byte load may pass the end)
    HIPCHK(D.hin.grow(L.at));
    HIPCHK(D.in.grow(L.at));
    char *hm = D.hin.p;
    auto put = [&](size_t off, const void *src, size_t bytes) {
        if (bytes) std::memcpy(hm + off, src, bytes);
    };
    put(o_segs, plan.segs.data(), plan.segs.size() * sizeof(SfsSeg));
    put(o_marks, plan.marks.data(), plan.marks.size() * sizeof(SfsMarkItem));
    put(o_folds, plan.folds.data(), plan.folds.size() * sizeof(SfsFoldItem));
    put(o_blk_off, c->tk_blk_off, (T + 1) * 8);
    put(o_tk_key, c->tk_key, T * 8);
    put(o_blk, c->blk, n_blk * 4);
    uint32_t *en_slot = reinterpret_cast<uint32_t *>(hm + o_en_slot);
    for (size_t i = 0; i < n_en; ++i) {
        const uint32_t t = c->en_t[i], id = c->en_id[i];
        if (t >= T || id >= c->tk_n_ids[t]) return lc::fail(LC_E_INVALID, "lc_setfull_stream_append: entry %zu is of no id", i);
        en_slot[i] = c->blk[c->tk_blk_off[t] + id / SFS_BLOCK_IDS] * SFS_BLOCK_IDS + id % SFS_BLOCK_IDS;
    }
    put(o_en_flags, c->en_flags, n_en * 4);
    put(o_en_inv, c->en_inv_pos, n_en * 8);
    put(o_en_ack, c->en_ack_pos, n_en * 8);
    put(o_en_ackt, c->en_ack_time, n_en * 8);
    put(o_rows, c->row_pos, n_rows * 8);
    put(o_rows + n_rows * 8, c->row_time, n_rows * 8);
    put(o_rows + n_rows * 16, c->row_inv_pos, n_rows * 8);
    put(o_rows + n_rows * 24, c->row_inv_time, n_rows * 8);
    put(o_el_off, c->el_off, (n_rows + 1) * 8);
    put(o_read_id, c->read_id, n_el * 4);
    std::memset(hm + o_read_id + n_el * 4, 0, 16);
    HIPCHK(D.mat.grow(plan.max_words * 8));
    Layout O;
    const size_t o_err = O.take(16), o_counts = O.take(T * 48), o_valid = O.take(T);
    HIPCHK(D.out.grow(O.at));
    HIPCHK(D.hout.grow(O.at));

    size_t e = 0;
    HIPCHK(hipEventRecord(D.ev[e++], q));
    HIPCHK(hipMemcpyAsync(D.in.p, hm, L.at, hipMemcpyHostToDevice, q));
    HIPCHK(hipMemsetAsync(D.out.p, 0, O.at, q));
    HIPCHK(hipEventRecord(D.ev[e++], q));

    const char *dm = (const char *)D.in.p;
    char *dout = (char *)D.out.p;
    SfsArgs a{};
    fill_resident(D, a);
    a.segs = (const SfsSeg *)(dm + o_segs);
    a.blk = (const uint32_t *)(dm + o_blk); a.tk_blk_off = (const uint64_t *)(dm + o_blk_off);
    a.tk_key = (const int64_t *)(dm + o_tk_key);
    a.en_slot = (const uint32_t *)(dm + o_en_slot); a.en_flags = (const uint32_t *)(dm + o_en_flags);
    a.en_inv = (const int64_t *)(dm + o_en_inv); a.en_ack = (const int64_t *)(dm + o_en_ack); a.en_ackt = (const int64_t *)(dm + o_en_ackt);
    a.row_pos = (const int64_t *)(dm + o_rows); a.row_time = (const int64_t *)(dm + o_rows + n_rows * 8);
    a.row_inv_pos = (const int64_t *)(dm + o_rows + n_rows * 16); a.row_inv_time = (const int64_t *)(dm + o_rows + n_rows * 24);
    a.el_off = (const uint64_t *)(dm + o_el_off); a.read_id = (const uint32_t *)(dm + o_read_id);
    a.mat = (uint64_t *)D.mat.p;
    a.counts = (unsigned long long *)(dout + o_counts); a.valid = (int8_t *)(dout + o_valid); a.err = (int32_t *)(dout + o_err);
    a.n_entries = (uint32_t)n_en;
    a.linearizable = linearizable ? 1u : 0u;
    const SfsMarkItem *d_marks = (const SfsMarkItem *)(dm + o_marks);
    const SfsFoldItem *d_folds = (const SfsFoldItem *)(dm + o_folds);

    if (n_en) k_sfs_reset<<<(uint32_t)((n_en + SFS_BLOCK - 1) / SFS_BLOCK), SFS_BLOCK, 0, q>>>(a);
    for (const SfsPass &p : plan.passes) {
        HIPCHK(hipEventRecord(D.ev[e++], q));
        if (p.words) HIPCHK(hipMemsetAsync(D.mat.p, 0, p.words * 8, q));
        if (p.mark1 > p.mark0) k_sfs_mark<<<(uint32_t)(p.mark1 - p.mark0), SFS_BLOCK, 0, q>>>(a, d_marks + p.mark0);
        HIPCHK(hipEventRecord(D.ev[e++], q));
        k_sfs_fold<<<(uint32_t)(p.fold1 - p.fold0), SFS_BLOCK, 0, q>>>(a, d_folds + p.fold0);
        HIPCHK(hipEventRecord(D.ev[e++], q));
    }
    if (T) k_sfs_finish<<<(uint32_t)T, SFS_BLOCK, 0, q>>>(a);
    HIPCHK(hipGetLastError());
    const size_t e_k = e;
    HIPCHK(hipEventRecord(D.ev[e++], q));
    HIPCHK(hipMemcpyAsync(D.hout.p, D.out.p, O.at, hipMemcpyDeviceToHost, q));
    HIPCHK(hipEventRecord(D.ev[e++], q));
    HIPCHK(hipStreamSynchronize(q));
    const char *ho = D.hout.p;
    int32_t bad_key;
    std::memcpy(&bad_key, ho + o_err, 4);
    if (bad_key) return lc::fail(LC_E_INVALID, "lc_setfull_stream_append: key %d: an id at or past the key's count", bad_key - 1);
    if (T) {
        std::memcpy(counts, ho + o_counts, T * 48);
        std::memcpy(valid, ho + o_valid, T);
    }
    float f = 0;
    double mark = 0;
    for (size_t p = 0; p < plan.passes.size(); ++p) {
        HIPCHK(hipEventElapsedTime(&f, D.ev[2 + 3 * p], D.ev[3 + 3 * p]));
        mark += f;
    }
    HIPCHK(hipEventElapsedTime(&f, D.ev[0], D.ev[1]));
    ms5[0] = f;
    ms5[1] = mark;
    HIPCHK(hipEventElapsedTime(&f, D.ev[1], D.ev[e_k]));
    ms5[2] = std::max(0.0, (double)f - mark);
    HIPCHK(hipEventElapsedTime(&f, D.ev[e_k], D.ev[e_k + 1]));
    ms5[3] = f;
    ms5[4] = (double)plan.passes.size();
    return LC_OK;
}

int sfs_dev_results(SfsDev *dp, uint64_t n_blocks, uint8_t *outcome, int64_t *latency, int64_t *known, int64_t *last_absent,
                    uint8_t *dup) {
    SfsDev &D = *dp;
    lcx::CtxCall x(D.ctx);
    LCCHK(x.enter());
    hipStream_t q = x.d->stream;
    if (n_blocks > D.cap_blocks) return lc::fail(LC_E_INVALID, "lc_setfull_stream_results: %llu blocks, %llu resident",
                                                 (unsigned long long)n_blocks, (unsigned long long)D.cap_blocks);
    const size_t n = (size_t)n_blocks * SFS_BLOCK_IDS;
    if (n == 0) return LC_OK;
    SfsArgs a{};
    fill_resident(D, a);
    HIPCHK(hipMemcpyAsync(outcome, a.outcome, n, hipMemcpyDeviceToHost, q));
    HIPCHK(hipMemcpyAsync(dup, a.dup, n, hipMemcpyDeviceToHost, q));
    HIPCHK(hipMemcpyAsync(latency, a.rec[A_MS], n * 8, hipMemcpyDeviceToHost, q));
    HIPCHK(hipMemcpyAsync(known, a.rec[A_KN], n * 8, hipMemcpyDeviceToHost, q));
    HIPCHK(hipMemcpyAsync(last_absent, a.rec[A_LA], n * 8, hipMemcpyDeviceToHost, q));
    HIPCHK(hipStreamSynchronize(q));
    return LC_OK;
}

}  // namespace lcfs
