// device_counter_stream.hip -- the device half of a streaming checker/counter
// (lc_counter_stream_*; include/lincheck_counter_stream.h has the contract,
// DESIGN.md section 3.17 the design).  A library of its own,
// lincheck/libcounter_stream_kernels.so, which liblincheck.so links by its own
// directory (the Makefile says why); lc::fail and the context's lane join
// resolve from liblincheck.so.
//
// RESIDENT between calls (events are not kept):
//   per key    the two running sums key_lo / key_up and n_err, the number of
//              its reads out of bounds
//   per slot   the `lower` stored at an open read's :invoke
//   per read   in arrival order: key id, rank within the key, lower, value,
//              upper, flag
// One append (device_counter_stream.hpp has the chunk):
//   k_cs_patch   over the resident reads [min r0, R), one per lane: binary
//                search of the patch list for the last entry of the read's
//                key with r0 <= r; its accumulated delta goes to `upper`, the
//                read is judged again, and where the flag changed n_err of the
//                key takes +1 or -1 (a wrapped add).  The lane of a key's last
//                patch adds its accumulated delta, the key's whole revision,
//                to key_up: one plain store a key.  Before the scan, so that
//                this append's reads start from the revised sum.
//   k_cs_tile / k_cs_carry / k_cs_apply
//                section 3.14's segmented scan over the append's events, a
//                segment per touched key.  A head event takes its key's
//                resident sums with it, so every segment starts from them.
//                apply stores `lower` into the slot at LC_CE_RINV, `upper`
//                into the read at LC_CE_ROK and, at a segment's last event,
//                the two sums into tail[segment].  An append of more than one
//                launch's events runs this once per piece.
//   k_cs_commit  tail[segment] to the key's sums, one segment per lane: a
//                launch of its own, because another workgroup of apply reads
//                those sums at the segment's head.
//   k_cs_judge   over the append's reads, after every piece: `lower` from the
//                slot (written by any workgroup of an earlier launch, of this
//                append or an older one), the flag, +1 to n_err where set.
//   k_cs_gather  n_err of the keys the packer names and the error word into
//                one small readback.
//   k_cs_results on demand: every read to read_off[key] + rank.
// Ordering is by kernel boundaries on the context's first stream; no lane or
// workgroup waits for another; atomics are adds and ors.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "counter_plan.hpp"
#include "counter_stream_plan.hpp"
#include "device_counter_stream.hpp"
#include "device_ctx.hpp"

namespace lccs {

namespace {

typedef unsigned long long u64;

constexpr uint32_t CE_BAD_EVENT = 1;  // a kind, segment, key, slot or read index out of range
constexpr uint8_t HEAD_ANY = 1, HEAD_FIRST = 2;

struct CsReads {
    uint32_t *key, *rank;
    int64_t *lower, *val, *upper;
    uint8_t *flag;
};

struct CsArgs {
    // resident
    u64 *key_lo, *key_up, *n_err;  // [K]
    u64 *slot_lo;                  // [n_slots]
    CsReads rd;                    // [cap]
    uint32_t K, n_slots;
    u64 R0;                        // reads resident before this append
    uint32_t n_new;                // this append's reads
    const uint32_t *new_slot;      // [n_new]
    // one piece's events
    uint32_t n;
    const uint8_t *kind;
    const uint32_t *seg, *aux;
    const int64_t *val;
    const uint32_t *seg_key;       // [n_seg]
    uint32_t n_seg, seg0, seg1;    // the piece's segments are seg0 .. seg1
    u64 *tail_lo, *tail_up;        // [n_seg]
    // the scan's tile records
    u64 *sum_a, *sum_b, *carry_a, *carry_b;
    uint8_t *heads;
    uint32_t tiles;
    // patches
    uint32_t n_patch;
    u64 min_r0;
    const uint32_t *p_key, *p_r0;
    const int64_t *p_acc;
    // readback
    const uint32_t *look;
    uint32_t n_look;
    u64 *out;                      // [1 + n_look]
    uint32_t *err;
};

__device__ inline uint8_t judged(int64_t lo, int64_t v, int64_t up) { return !(lo <= v && v <= up); }

__global__ __launch_bounds__(CSP_BLOCK) void k_cs_patch(CsArgs a) {
    const u64 gid = (u64)blockIdx.x * CSP_BLOCK + threadIdx.x;
    const u64 r = a.min_r0 + gid;
    if (r < a.R0) {
        const uint32_t k = a.rd.key[r];
        uint32_t lo = 0, hi = a.n_patch;
        while (lo < hi) {  // the first entry past (k, r)
            const uint32_t m = (lo + hi) >> 1;
            const uint32_t pk = a.p_key[m];
            if (pk < k || (pk == k && (u64)a.p_r0[m] <= r)) lo = m + 1;
            else hi = m;
        }
        if (lo && k < a.K && a.p_key[lo - 1] == k) {
            const int64_t up = (int64_t)((u64)a.rd.upper[r] + (u64)a.p_acc[lo - 1]);
            a.rd.upper[r] = up;
            const uint8_t fl = judged(a.rd.lower[r], a.rd.val[r], up);
            if (fl != a.rd.flag[r]) {
                a.rd.flag[r] = fl;
                __hip_atomic_fetch_add(&a.n_err[k], fl ? 1ull : ~0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    if (gid < a.n_patch) {
        const uint32_t k = a.p_key[gid];
        if (k >= a.K) atomicOr(a.err, CE_BAD_EVENT);
        else if (gid + 1 == a.n_patch || a.p_key[gid + 1] != k) a.key_up[k] += (u64)a.p_acc[gid];  // the key's last entry: its only writer
    }
}

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

constexpr int WAVES = CSP_BLOCK / 64;

// The workgroup's segmented scan of one (a, b, f) per thread (device_counter.hip's, restated).
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
    for (uint32_t i = 0; i < (uint32_t)WAVES; ++i) {
        if (i == w) {
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
    __syncthreads();
    return s;
}

// This thread's IPT consecutive events from `base`: kinds (0xFF past the end),
// values, and sg[j + 1] the segment of event base + j (sg[0] the event before,
// sg[IPT + 1] the one after; ~0 outside the piece, so that the piece's first
// event is a head and its last a tail).
template <int IPT>
__device__ __forceinline__ void load_events(const CsArgs &a, u64 base, uint8_t kind[IPT], int64_t val[IPT], uint32_t sg[IPT + 2]) {
#pragma unroll
    for (int j = 0; j < IPT; ++j) {
        const bool in = base + j < a.n;
        kind[j] = in ? a.kind[base + j] : (uint8_t)0xFF;
        val[j] = in ? a.val[base + j] : 0;
    }
#pragma unroll
    for (int j = 0; j < IPT + 2; ++j) {
        const u64 i = base + j;  // event i - 1
        sg[j] = i >= 1 && i - 1 < a.n ? a.seg[i - 1] : 0xFFFFFFFFu;
    }
}

// The thread's fold of its events: a head starts from its key's resident sums.
template <int IPT>
__device__ __forceinline__ uint32_t fold_events(const CsArgs &a, u64 base, const uint8_t kind[IPT], const int64_t val[IPT],
                                       const uint32_t sg[IPT + 2], u64 &lo, u64 &up, bool &bad) {
    uint32_t hb = 0;
#pragma unroll
    for (int j = 0; j < IPT; ++j) {
        if (base + j < a.n && sg[j + 1] != sg[j]) {
            hb |= 1u << j;
            const uint32_t s = sg[j + 1];
            const uint32_t k = s < a.n_seg ? a.seg_key[s] : 0xFFFFFFFFu;
            if (k < a.K) {
                lo = a.key_lo[k];
                up = a.key_up[k];
            } else {
                bad = true;
                lo = 0;
                up = 0;
            }
        }
        up += kind[j] == LC_CE_UP ? (u64)val[j] : 0;
        lo += kind[j] == LC_CE_LOW ? (u64)val[j] : 0;
    }
    return hb;
}

template <int IPT>
__global__ __launch_bounds__(CSP_BLOCK) void k_cs_tile(CsArgs a) {
    __shared__ u64 sh_a[WAVES], sh_b[WAVES];
    __shared__ uint32_t sh_f[WAVES];
    const u64 t = blockIdx.x, base = t * (IPT * CSP_BLOCK) + (u64)threadIdx.x * IPT;
    uint8_t kind[IPT];
    int64_t val[IPT];
    uint32_t sg[IPT + 2];
    load_events<IPT>(a, base, kind, val, sg);
    u64 lo = 0, up = 0;
    bool bad = false;
    const uint32_t hb = fold_events<IPT>(a, base, kind, val, sg, lo, up, bad);
    const Scan s = block_seg_scan(lo, up, hb != 0, sh_a, sh_b, sh_f);
    if (threadIdx.x == 0) {
        a.sum_a[t] = s.ta;
        a.sum_b[t] = s.tb;
        a.heads[t] = (uint8_t)((s.tf ? HEAD_ANY : 0) | ((hb & 1) ? HEAD_FIRST : 0));
    }
}

__global__ __launch_bounds__(CSP_BLOCK) void k_cs_carry(CsArgs t) {
    __shared__ u64 sh_a[WAVES], sh_b[WAVES];
    __shared__ uint32_t sh_f[WAVES];
    u64 run_a = 0, run_b = 0;
    for (uint32_t c0 = 0; c0 < t.tiles; c0 += CSP_BLOCK) {
        const uint32_t i = c0 + threadIdx.x;
        const bool have = i < t.tiles;
        const u64 a = have ? t.sum_a[i] : 0, b = have ? t.sum_b[i] : 0;
        const uint8_t h = have ? t.heads[i] : (uint8_t)0;
        const Scan s = block_seg_scan(a, b, (h & HEAD_ANY) != 0, sh_a, sh_b, sh_f);
        if (have) {
            const bool first = (h & HEAD_FIRST) != 0;
            t.carry_a[i] = first ? 0 : s.ef ? s.ea : run_a + s.ea;
            t.carry_b[i] = first ? 0 : s.ef ? s.eb : run_b + s.eb;
        }
        run_a = s.tf ? s.ta : run_a + s.ta;
        run_b = s.tf ? s.tb : run_b + s.tb;
    }
}

template <int IPT>
__global__ __launch_bounds__(CSP_BLOCK) void k_cs_apply(CsArgs a) {
    __shared__ u64 sh_a[WAVES], sh_b[WAVES];
    __shared__ uint32_t sh_f[WAVES];
    const u64 t = blockIdx.x, base = t * (IPT * CSP_BLOCK) + (u64)threadIdx.x * IPT;
    uint8_t kind[IPT];
    int64_t val[IPT];
    uint32_t sg[IPT + 2];
    load_events<IPT>(a, base, kind, val, sg);
    u64 lo = 0, up = 0;
    bool bad = false;
    const uint32_t hb = fold_events<IPT>(a, base, kind, val, sg, lo, up, bad);
    const Scan s = block_seg_scan(lo, up, hb != 0, sh_a, sh_b, sh_f);
    // what reaches this thread's first event
    lo = s.ef ? s.ea : a.carry_a[t] + s.ea;
    up = s.ef ? s.eb : a.carry_b[t] + s.eb;
#pragma unroll
    for (int j = 0; j < IPT; ++j) {
        const uint32_t sgj = sg[j + 1];
        if (hb >> j & 1) {
            const uint32_t k = sgj < a.n_seg ? a.seg_key[sgj] : 0xFFFFFFFFu;
            lo = k < a.K ? a.key_lo[k] : 0;
            up = k < a.K ? a.key_up[k] : 0;
        }
        const uint8_t kd = kind[j];
        if (kd == LC_CE_UP) {
            up += (u64)val[j];
        } else if (kd == LC_CE_LOW) {
            lo += (u64)val[j];
        } else if (kd == LC_CE_RINV || kd == LC_CE_ROK) {
            const uint32_t slot = a.aux[base + j];
            const u64 idx = (u64)val[j];
            if (slot >= a.n_slots) bad = true;
            else if (kd == LC_CE_RINV) a.slot_lo[slot] = lo;
            else if (idx >= a.n_new) bad = true;
            else a.rd.upper[a.R0 + idx] = (int64_t)up;
        } else if (base + j < a.n) {
            bad = true;
        }
        if (sg[j + 2] != sgj && sgj < a.n_seg) {  // the segment's last event in this piece
            a.tail_lo[sgj] = lo;
            a.tail_up[sgj] = up;
        }
    }
    if (bad) atomicOr(a.err, CE_BAD_EVENT);
}

__global__ __launch_bounds__(CSP_BLOCK) void k_cs_commit(CsArgs a) {
    const u64 s = (u64)a.seg0 + (u64)blockIdx.x * CSP_BLOCK + threadIdx.x;
    if (s > a.seg1 || s >= a.n_seg) return;
    const uint32_t k = a.seg_key[s];
    if (k >= a.K) return;  // (apply has set the error word)
    a.key_lo[k] = a.tail_lo[s];
    a.key_up[k] = a.tail_up[s];
}

__global__ __launch_bounds__(CSP_BLOCK) void k_cs_judge(CsArgs a) {
    const u64 gid = (u64)blockIdx.x * CSP_BLOCK + threadIdx.x;
    if (gid >= a.n_new) return;
    const u64 r = a.R0 + gid;
    const uint32_t k = a.rd.key[r], slot = a.new_slot[gid];
    if (k >= a.K || slot >= a.n_slots) {
        atomicOr(a.err, CE_BAD_EVENT);
        return;
    }
    const int64_t lo = (int64_t)a.slot_lo[slot];
    a.rd.lower[r] = lo;
    const uint8_t fl = judged(lo, a.rd.val[r], a.rd.upper[r]);
    a.rd.flag[r] = fl;
    if (fl) __hip_atomic_fetch_add(&a.n_err[k], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(CSP_BLOCK) void k_cs_gather(CsArgs a) {
    const u64 gid = (u64)blockIdx.x * CSP_BLOCK + threadIdx.x;
    if (gid < a.n_look) {
        const uint32_t k = a.look[gid];
        a.out[1 + gid] = k < a.K ? a.n_err[k] : 0;
    }
    if (gid == 0) {
        a.out[0] = *a.err;
        *a.err = 0;
    }
}

struct CsResArgs {
    CsReads rd;
    u64 R, total;
    const u64 *read_off;  // [K]
    uint32_t K;
    int64_t *lower, *upper, *value;
    uint8_t *flag;
};

__global__ __launch_bounds__(CSP_BLOCK) void k_cs_results(CsResArgs a) {
    const u64 r = (u64)blockIdx.x * CSP_BLOCK + threadIdx.x;
    if (r >= a.R) return;
    const uint32_t k = a.rd.key[r];
    if (k >= a.K) return;
    const u64 off = a.read_off[k];
    if (off == CS_NO_READS) return;
    const u64 at = off + a.rd.rank[r];
    if (at >= a.total) return;
    a.lower[at] = a.rd.lower[r];
    a.upper[at] = a.rd.upper[r];
    a.value[at] = a.rd.val[r];
    a.flag[at] = a.rd.flag[r];
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

size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }

// The reads arrays as one allocation of `cap` reads.
size_t reads_bytes(uint64_t cap) { return (size_t)cap * 8 * 3 + up16((size_t)cap * 4) * 2 + up16((size_t)cap); }
CsReads reads_at(void *p, uint64_t cap) {
    char *b = (char *)p;
    CsReads r;
    r.lower = (int64_t *)b; r.val = r.lower + cap; r.upper = r.val + cap;
    b += (size_t)cap * 24;
    r.key = (uint32_t *)b; b += up16((size_t)cap * 4);
    r.rank = (uint32_t *)b; b += up16((size_t)cap * 4);
    r.flag = (uint8_t *)b;
    return r;
}

// A resident array of 8-byte words that grows by doubling, the old words copied, the new ones 0.
struct Words {
    u64 *p = nullptr;
    uint64_t cap = 0;
    int ensure(hipStream_t q, uint64_t need, uint64_t first, const char *what) {
        if (need <= cap) return LC_OK;
        uint64_t c = cap ? cap : first;
        while (c < need) c <<= 1;
        u64 *n = nullptr;
        hipError_t e = hipMalloc((void **)&n, (size_t)c * 8);
        if (e == hipSuccess && cap) e = hipMemcpyAsync(n, p, (size_t)cap * 8, hipMemcpyDeviceToDevice, q);
        if (e == hipSuccess) e = hipMemsetAsync(n + cap, 0, (size_t)(c - cap) * 8, q);
        if (e == hipSuccess) e = hipStreamSynchronize(q);
        if (e != hipSuccess) {
            if (n) (void)hipFree(n);
            return lc::fail(LC_E_DEVICE, "lc_counter_stream_append: growing %s to %llu failed: %s", what, (unsigned long long)c,
                            hipGetErrorString(e));
        }
        if (p) (void)hipFree(p);
        p = n;
        cap = c;
        return LC_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

}  // namespace

struct CsDev {
    lc_ctx *ctx = nullptr;
    uint32_t tile = 0;
    uint64_t launch_events = 0;
    void *reads = nullptr;
    uint64_t cap = 0;
    Words key_lo, key_up, n_err, slot_lo;
    uint32_t *err = nullptr;
    Buf ev, segs, news, patch, look, tiles, out, res, off;
    HostBuf hout, hres;
    hipEvent_t evt[6] = {};
};

namespace {

int ensure_events(CsDev &D) {
    for (hipEvent_t &e : D.evt)
        if (!e) HIPCHK(hipEventCreate(&e));
    return LC_OK;
}

}  // namespace

int cs_dev_open(lc_ctx *c, uint32_t tile, uint64_t launch_events, CsDev **out) {
    *out = nullptr;
    if (c->n_dev != 1 || c->comm)
        return lc::fail(LC_E_UNSUPPORTED, "lc_counter_stream_open: a stream needs a context of one device and no communicator");
    if (tile != lcc::CT_TILE_MIN && tile != lcc::CT_TILE_DEFAULT) return lc::fail(LC_E_INVALID, "lc_counter_stream_open: tile %u", tile);
    if (launch_events == 0 || launch_events % tile || launch_events > CSP_LAUNCH_EVENTS)
        return lc::fail(LC_E_INVALID, "lc_counter_stream_open: %llu events a launch", (unsigned long long)launch_events);
    CsDev *d = new (std::nothrow) CsDev();
    if (!d) return lc::fail(LC_E_NOMEM, "lc_counter_stream_open: out of memory");
    d->ctx = c;
    d->tile = tile;
    d->launch_events = launch_events;
    *out = d;
    return LC_OK;
}

void cs_dev_close(CsDev *d) {
    if (!d) return;
    {
        std::lock_guard<std::mutex> g(d->ctx->mu);
        lcx::Dev *dev = d->ctx->dev[0];
        (void)hipSetDevice(dev->device);
        (void)hipStreamSynchronize(dev->stream);
        if (d->reads) (void)hipFree(d->reads);
        if (d->err) (void)hipFree(d->err);
        for (Words *w : {&d->key_lo, &d->key_up, &d->n_err, &d->slot_lo}) w->release();
        for (Buf *b : {&d->ev, &d->segs, &d->news, &d->patch, &d->look, &d->tiles, &d->out, &d->res, &d->off}) b->release();
        for (HostBuf *b : {&d->hout, &d->hres}) b->release();
        for (hipEvent_t e : d->evt)
            if (e) (void)hipEventDestroy(e);
    }
    delete d;
}

int cs_dev_reserve(CsDev *dp, uint64_t cap, uint64_t reads, double *ms) {
    CsDev &D = *dp;
    lcx::CtxCall x(D.ctx);
    LCCHK(x.enter());
    hipStream_t q = x.d->stream;
    *ms = 0;
    if (cap <= D.cap) return LC_OK;
    if (cap > CSP_MAX_READS || reads > D.cap) return lc::fail(LC_E_INVALID, "lc_counter_stream_append: a reads array of %llu", (unsigned long long)cap);
    LCCHK(ensure_events(D));
    if (!D.err) {
        HIPCHK(hipMalloc((void **)&D.err, 4));
        HIPCHK(hipMemsetAsync(D.err, 0, 4, q));
    }
    void *to = nullptr;
    if (hipMalloc(&to, reads_bytes(cap)) != hipSuccess) {
        (void)hipGetLastError();
        return lc::fail(LC_E_NOMEM, "lc_counter_stream_append: no device memory for %llu reads (%llu bytes)", (unsigned long long)cap,
                        (unsigned long long)reads_bytes(cap));
    }
    hipError_t e = hipEventRecord(D.evt[4], q);
    if (e == hipSuccess && reads) {
        const CsReads f = reads_at(D.reads, D.cap), t = reads_at(to, cap);
        const size_t n = (size_t)reads;
        const void *src[6] = {f.lower, f.val, f.upper, f.key, f.rank, f.flag};
        void *dst[6] = {t.lower, t.val, t.upper, t.key, t.rank, t.flag};
        const size_t bytes[6] = {n * 8, n * 8, n * 8, n * 4, n * 4, n};
        for (int i = 0; i < 6 && e == hipSuccess; ++i) e = hipMemcpyAsync(dst[i], src[i], bytes[i], hipMemcpyDeviceToDevice, q);
    }
    if (e == hipSuccess) e = hipEventRecord(D.evt[5], q);
    if (e == hipSuccess) e = hipStreamSynchronize(q);
    if (e != hipSuccess) {
        (void)hipFree(to);
        return lc::fail(LC_E_DEVICE, "lc_counter_stream_append: growing the reads array to %llu failed: %s", (unsigned long long)cap,
                        hipGetErrorString(e));
    }
    if (D.reads) (void)hipFree(D.reads);  // (the stream is idle here)
    D.reads = to;
    D.cap = cap;
    float f = 0;
    HIPCHK(hipEventElapsedTime(&f, D.evt[4], D.evt[5]));
    *ms = f;
    return LC_OK;
}

int cs_dev_append(CsDev *dp, const CsChunk *c, uint64_t *n_errors, double *ms3) {
    CsDev &D = *dp;
    lcx::CtxCall x(D.ctx);
    LCCHK(x.enter());
    hipStream_t q = x.d->stream;
    const uint64_t E = c->n_events, NR = c->n_reads, P = c->n_patch, L = c->n_look, S = c->n_seg, R0 = c->reads_before;
    if (!D.reads || c->n_keys == 0 || c->n_keys > 0x7FFFFFF0ull || R0 + NR > D.cap || c->n_slots > CSP_LIMIT || S > E || L > c->n_keys ||
        (P && c->min_r0 > R0))
        return lc::fail(LC_E_INVALID, "lc_counter_stream_append: a chunk that does not fit the stream");
    LCCHK(ensure_events(D));
    LCCHK(D.key_lo.ensure(q, c->n_keys, 64, "the per-key sums"));
    LCCHK(D.key_up.ensure(q, c->n_keys, 64, "the per-key sums"));
    LCCHK(D.n_err.ensure(q, c->n_keys, 64, "the per-key counts"));
    LCCHK(D.slot_lo.ensure(q, std::max<uint64_t>(c->n_slots, 1), 64, "the slots"));
    const size_t piece_max = (size_t)std::min<uint64_t>(E, D.launch_events);
    const uint64_t tiles_max = lcc::ct_tiles(piece_max, D.tile);
    // one piece's events: values, segments, slots, kinds
    const size_t o_seg = piece_max * 8, o_aux = o_seg + up16(piece_max * 4), o_kind = o_aux + up16(piece_max * 4);
    HIPCHK(D.ev.grow(o_kind + up16(piece_max)));
    // the segments' keys and tails
    const size_t o_tlo = up16((size_t)S * 4), o_tup = o_tlo + (size_t)S * 8;
    HIPCHK(D.segs.grow(o_tup + (size_t)S * 8));
    HIPCHK(D.news.grow((size_t)NR * 4));
    const size_t o_pkey = (size_t)P * 8, o_pr0 = o_pkey + up16((size_t)P * 4);
    HIPCHK(D.patch.grow(o_pr0 + up16((size_t)P * 4)));
    HIPCHK(D.look.grow((size_t)L * 4));
    const size_t o_heads = (size_t)tiles_max * 32;
    HIPCHK(D.tiles.grow(o_heads + up16((size_t)tiles_max)));
    HIPCHK(D.out.grow((1 + (size_t)L) * 8));
    HIPCHK(D.hout.grow((1 + (size_t)L) * 8));

    CsArgs a{};
    a.key_lo = D.key_lo.p; a.key_up = D.key_up.p; a.n_err = D.n_err.p; a.slot_lo = D.slot_lo.p;
    a.rd = reads_at(D.reads, D.cap);
    a.K = (uint32_t)c->n_keys; a.n_slots = (uint32_t)c->n_slots; a.R0 = R0; a.n_new = (uint32_t)NR;
    a.new_slot = (const uint32_t *)D.news.p;
    char *ev = (char *)D.ev.p;
    a.val = (const int64_t *)ev; a.seg = (const uint32_t *)(ev + o_seg); a.aux = (const uint32_t *)(ev + o_aux);
    a.kind = (const uint8_t *)(ev + o_kind);
    char *sg = (char *)D.segs.p;
    a.seg_key = (const uint32_t *)sg; a.n_seg = (uint32_t)S; a.tail_lo = (u64 *)(sg + o_tlo); a.tail_up = (u64 *)(sg + o_tup);
    u64 *tl = (u64 *)D.tiles.p;
    a.sum_a = tl; a.sum_b = tl + tiles_max; a.carry_a = tl + 2 * tiles_max; a.carry_b = tl + 3 * tiles_max;
    a.heads = (uint8_t *)D.tiles.p + o_heads;
    char *pp = (char *)D.patch.p;
    a.n_patch = (uint32_t)P; a.min_r0 = c->min_r0;
    a.p_acc = (const int64_t *)pp; a.p_key = (const uint32_t *)(pp + o_pkey);
    a.p_r0 = (const uint32_t *)(pp + o_pr0);
    a.look = (const uint32_t *)D.look.p; a.n_look = (uint32_t)L; a.out = (u64 *)D.out.p; a.err = D.err;

    HIPCHK(hipEventRecord(D.evt[0], q));
    if (S) HIPCHK(hipMemcpyAsync((void *)a.seg_key, c->seg_key, (size_t)S * 4, hipMemcpyHostToDevice, q));
    if (NR) {
        HIPCHK(hipMemcpyAsync(a.rd.key + R0, c->rd_key, (size_t)NR * 4, hipMemcpyHostToDevice, q));
        HIPCHK(hipMemcpyAsync(a.rd.rank + R0, c->rd_rank, (size_t)NR * 4, hipMemcpyHostToDevice, q));
        HIPCHK(hipMemcpyAsync(a.rd.val + R0, c->rd_val, (size_t)NR * 8, hipMemcpyHostToDevice, q));
        HIPCHK(hipMemcpyAsync((void *)a.new_slot, c->rd_slot, (size_t)NR * 4, hipMemcpyHostToDevice, q));
    }
    if (P) {
        HIPCHK(hipMemcpyAsync((void *)a.p_acc, c->p_acc, (size_t)P * 8, hipMemcpyHostToDevice, q));
        HIPCHK(hipMemcpyAsync((void *)a.p_key, c->p_key, (size_t)P * 4, hipMemcpyHostToDevice, q));
        HIPCHK(hipMemcpyAsync((void *)a.p_r0, c->p_r0, (size_t)P * 4, hipMemcpyHostToDevice, q));
    }
    if (L) HIPCHK(hipMemcpyAsync((void *)a.look, c->look, (size_t)L * 4, hipMemcpyHostToDevice, q));
    // the first piece's events go up before the patch launch, so that the upload is timed as one
    const uint64_t pieces = csp_pieces(E, D.launch_events);
    if (pieces == 0) {
        HIPCHK(hipEventRecord(D.evt[1], q));
        if (P) k_cs_patch<<<(uint32_t)csp_blocks(csp_patch_threads(R0, c->min_r0, P)), CSP_BLOCK, 0, q>>>(a);
    }
    for (uint64_t i = 0; i < pieces; ++i) {
        const uint64_t b = csp_piece_begin(i, E, D.launch_events), e = csp_piece_begin(i + 1, E, D.launch_events);
        const size_t n = (size_t)(e - b);
        HIPCHK(hipMemcpyAsync((void *)a.val, c->ev_val + b, n * 8, hipMemcpyHostToDevice, q));
        HIPCHK(hipMemcpyAsync((void *)a.seg, c->ev_seg + b, n * 4, hipMemcpyHostToDevice, q));
        HIPCHK(hipMemcpyAsync((void *)a.aux, c->ev_aux + b, n * 4, hipMemcpyHostToDevice, q));
        HIPCHK(hipMemcpyAsync((void *)a.kind, c->ev_kind + b, n, hipMemcpyHostToDevice, q));
        if (i == 0) {
            HIPCHK(hipEventRecord(D.evt[1], q));
            if (P) k_cs_patch<<<(uint32_t)csp_blocks(csp_patch_threads(R0, c->min_r0, P)), CSP_BLOCK, 0, q>>>(a);
        }
        a.n = (uint32_t)n;
        a.tiles = (uint32_t)lcc::ct_tiles(n, D.tile);
        a.seg0 = c->ev_seg[b];
        a.seg1 = c->ev_seg[e - 1];
        if (a.seg0 > a.seg1 || a.seg1 >= S) return lc::fail(LC_E_INVALID, "lc_counter_stream_append: the events' segments do not ascend");
        if (D.tile == lcc::CT_TILE_DEFAULT) {
            k_cs_tile<8><<<a.tiles, CSP_BLOCK, 0, q>>>(a);
            k_cs_carry<<<1, CSP_BLOCK, 0, q>>>(a);
            k_cs_apply<8><<<a.tiles, CSP_BLOCK, 0, q>>>(a);
        } else {
            k_cs_tile<1><<<a.tiles, CSP_BLOCK, 0, q>>>(a);
            k_cs_carry<<<1, CSP_BLOCK, 0, q>>>(a);
            k_cs_apply<1><<<a.tiles, CSP_BLOCK, 0, q>>>(a);
        }
        k_cs_commit<<<(uint32_t)csp_blocks((uint64_t)a.seg1 - a.seg0 + 1), CSP_BLOCK, 0, q>>>(a);
    }
    if (NR) k_cs_judge<<<(uint32_t)csp_blocks(NR), CSP_BLOCK, 0, q>>>(a);
    k_cs_gather<<<(uint32_t)std::max<uint64_t>(1, csp_blocks(L)), CSP_BLOCK, 0, q>>>(a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(D.evt[2], q));
    HIPCHK(hipMemcpyAsync(D.hout.p, D.out.p, (1 + (size_t)L) * 8, hipMemcpyDeviceToHost, q));
    HIPCHK(hipEventRecord(D.evt[3], q));
    HIPCHK(hipStreamSynchronize(q));
    const u64 *ho = (const u64 *)D.hout.p;
    if (ho[0]) return lc::fail(LC_E_INVALID, "lc_counter_stream_append: a chunk with a kind, key, slot or read index out of range");
    if (L) std::memcpy(n_errors, ho + 1, (size_t)L * 8);
    float f = 0;
    for (int i = 0; i < 3; ++i) {
        HIPCHK(hipEventElapsedTime(&f, D.evt[i], D.evt[i + 1]));
        ms3[i] = f;
    }
    return LC_OK;
}

int cs_dev_results(CsDev *dp, const uint64_t *read_off, uint64_t n_keys, uint64_t reads, uint64_t total, int64_t *lower, int64_t *upper,
                   int64_t *value, uint8_t *flag) {
    CsDev &D = *dp;
    lcx::CtxCall x(D.ctx);
    LCCHK(x.enter());
    hipStream_t q = x.d->stream;
    if (total == 0) return LC_OK;
    if (!D.reads || reads > D.cap || total > reads || n_keys == 0) return lc::fail(LC_E_INVALID, "lc_counter_stream_results: counts that do not fit the stream");
    const size_t T = (size_t)total, o_flag = T * 24, bytes = o_flag + up16(T);
    HIPCHK(D.res.grow(bytes));
    HIPCHK(D.hres.grow(bytes));
    HIPCHK(D.off.grow((size_t)n_keys * 8));
    CsResArgs a{};
    a.rd = reads_at(D.reads, D.cap);
    a.R = reads; a.total = total; a.read_off = (const u64 *)D.off.p; a.K = (uint32_t)n_keys;
    a.lower = (int64_t *)D.res.p; a.upper = a.lower + T; a.value = a.upper + T; a.flag = (uint8_t *)D.res.p + o_flag;
    HIPCHK(hipMemcpyAsync(D.off.p, read_off, (size_t)n_keys * 8, hipMemcpyHostToDevice, q));
    HIPCHK(hipStreamSynchronize(q));  // (read_off is the caller's pageable memory)
    k_cs_results<<<(uint32_t)csp_blocks(reads), CSP_BLOCK, 0, q>>>(a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(D.hres.p, D.res.p, bytes, hipMemcpyDeviceToHost, q));
    HIPCHK(hipStreamSynchronize(q));
    std::memcpy(lower, D.hres.p, T * 8);
    std::memcpy(upper, D.hres.p + T * 8, T * 8);
    if (value) std::memcpy(value, D.hres.p + T * 16, T * 8);
    std::memcpy(flag, D.hres.p + o_flag, T);
    return LC_OK;
}

}  // namespace lccs
