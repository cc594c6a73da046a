// device_queue_stream.hip -- the device half of a streaming total-queue /
// unique-ids (lc_queue_stream_*; include/lincheck_queue_stream.h has the
// contract, DESIGN.md section 3.16 the design).  A library of its own,
// lincheck/libqueue_stream_kernels.so, which liblincheck.so links by its own
// directory (the Makefile says why); lc::fail and the context's lane join
// resolve from liblincheck.so.
//
// RESIDENT between calls: the hash table (device_queue_stream.hpp has the
// slot), QS_KEY_WORDS words per key, and a control block: the distinct-value
// counter, the error word, the dirty cursor, the entry cursor.
//
// THE CLAIM keeps what makes k_queue_tally safe -- no lane ever waits for
// another lane's store -- with a state word of three kinds.  EMPTY is claimed
// with one returning compare-and-swap to QS_ROW0 + the claiming row's index.
// A lane that meets such a state compares with row_key / row_val of that row:
// input arrays that no kernel writes.  A lane that meets QS_SETTLED compares
// with the slot's own key and value, which an EARLIER kernel wrote (k_qs_settle
// or k_qs_rehash), so plain loads are right.  The state word itself, which
// other CUs write, is read with a relaxed agent-scope atomic load.  Every
// claimed slot is settled by the k_qs_settle that follows its tally, so a
// state never names a row of an older piece.
//
//   k_qs_tally    one packed row per lane: probe, claim or match; one
//                 no-return add on tally[kind]; the lane that turns the slot's
//                 dirty flag from 0 to 1 (a returning exchange, tried only
//                 while the flag reads 0) enters the slot into the dirty list
//                 at a position from one returning add on the cursor.  The
//                 list holds the piece's rows, which bounds it.  A new claim
//                 bumps the distinct-value counter.  The probe loop is bounded
//                 by `slots`; a lane that has seen every slot sets the error
//                 word and stops.
//   k_qs_settle   one dirty slot per lane: a slot in a row state takes that
//                 row's key and value and becomes SETTLED; the class vector of
//                 `tally` minus that of `applied` (k_queue_classify's
//                 formulas) goes to the key's count words, a wrapped unsigned
//                 add where negative; unique-ids folds the value into the
//                 key's range words; applied = tally, dirty = 0.  A wave whose
//                 dirty slots share one key sums by shuffles and adds once per
//                 word; a wave that holds several keys adds per lane.  (No
//                 workgroup stage: a dirty list is in arrival order, and the
//                 lists measured are short beside a table.)
//   k_qs_gather   the touched keys' words, the distinct counter, the error
//                 word and the dirty count into the readback block; resets the
//                 dirty cursor.
//   k_qs_rehash   on growth, one old slot per lane: every occupied slot is
//                 SETTLED between appends and identities are distinct, so each
//                 claims the first EMPTY slot of the new table from its hash
//                 with a compare-and-swap and stores its payload; no compare.
//                 Bounded by the new `slots`.
//   k_qs_entries  on demand, one slot per lane: the entry half of
//                 k_queue_classify.  Slots of :unknown keys are skipped.
// Ordering is by kernel boundaries on the context's lane 0; every loop is
// bounded by a launch argument; nothing spins.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "device_ctx.hpp"
#include "device_queue_stream.hpp"
#include "queue_stream_plan.hpp"

namespace lcqs {

namespace {

typedef unsigned long long u64;

// The slot as three 16-byte words.
struct QsSlot {
    uint32_t state, key;
    int64_t val;
    uint32_t tally[3], dirty;
    uint32_t applied[3], pad;
};
static_assert(sizeof(QsSlot) == QSP_SLOT_BYTES, "the slot");

enum { QC_DISTINCT = 0, QC_ERR = 1, QC_CURSOR = 2, QC_N_ENT = 3, QC_WORDS = 4 };
enum { QR_DISTINCT = 0, QR_ERR = 1, QR_DIRTY = 2, QR_HEAD = 4 };  // the readback block; the keys' words from QR_HEAD
constexpr u64 QE_BAD_ROW = 1;    // row_key >= n_keys, or a row_kind the mode has not
constexpr u64 QE_FULL = 2;       // a lane visited every slot and found no place
constexpr u64 QE_STATE = 4;      // a state that names no row of the piece, or a dirty list past its capacity
constexpr u64 SIGN = 1ull << 63;

struct QsArgs {
    QsSlot *table;
    uint32_t slots;  // a power of two
    uint32_t n_rows; // the piece's
    const uint32_t *row_key;
    const uint8_t *row_kind;
    const int64_t *row_val;
    uint32_t K, mode;
    u64 *keyst;      // [key capacity][QS_KEY_WORDS]
    uint32_t *dirty; // [n_rows]
    u64 *ctl;        // [QC_WORDS]
    const uint32_t *touched;
    uint32_t n_touched;
    u64 *out;        // [QR_HEAD + n_touched * QS_KEY_WORDS]
};

struct QsEntArgs {
    const QsSlot *table;
    uint32_t slots, K, mode;
    const uint8_t *status;
    uint32_t *ent_key;
    uint8_t *ent_class;
    int64_t *ent_val;
    u64 *ent_mult;
    u64 ent_cap;
    u64 *ctl;
};

__device__ inline uint32_t slot_hash(uint32_t key, int64_t val) {
    u64 x = (u64)val ^ ((u64)key * 0x9E3779B97F4A7C15ull);
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return (uint32_t)x ^ (uint32_t)(x >> 32);
}

__device__ inline void set_err(u64 *ctl, u64 bit) {
    __hip_atomic_fetch_or(&ctl[QC_ERR], bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(QSP_BLOCK) void k_qs_tally(QsArgs a) {
    const u64 r = (u64)blockIdx.x * QSP_BLOCK + threadIdx.x;
    if (r >= a.n_rows) return;
    const uint32_t key = a.row_key[r], kind = a.row_kind[r];
    const bool kind_ok = a.mode == LC_QM_UNIQUE_IDS ? kind == LC_QK_ACK : kind <= LC_QK_DEQUEUE;
    if (key >= a.K || !kind_ok) {
        set_err(a.ctl, QE_BAD_ROW);
        return;
    }
    const int64_t val = a.row_val[r];
    const uint32_t mask = a.slots - 1, me = QS_ROW0 + (uint32_t)r;
    uint32_t slot = slot_hash(key, val) & mask;
    for (uint32_t seen = 0; seen < a.slots; ++seen) {
        QsSlot *s = a.table + slot;
        uint32_t st = __hip_atomic_load(&s->state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        bool claimed = false;
        if (st == QS_EMPTY) {
            st = atomicCAS(&s->state, QS_EMPTY, me);
            if (st == QS_EMPTY) {
                st = me;
                claimed = true;
            }
        }
        bool match;
        if (st == me) {
            match = true;
        } else if (st == QS_SETTLED) {
            match = s->key == key && s->val == val;  // an earlier kernel's stores
        } else {
            const uint32_t rep = st - QS_ROW0;
            if (rep >= a.n_rows) {
                set_err(a.ctl, QE_STATE);
                return;
            }
            match = a.row_key[rep] == key && a.row_val[rep] == val;
        }
        if (match) {
            __hip_atomic_fetch_add(&s->tally[kind], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (__hip_atomic_load(&s->dirty, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0 &&
                __hip_atomic_exchange(&s->dirty, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) {
                const u64 at = __hip_atomic_fetch_add(&a.ctl[QC_CURSOR], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (at < a.n_rows) a.dirty[at] = slot;
                else set_err(a.ctl, QE_STATE);
            }
            if (claimed) __hip_atomic_fetch_add(&a.ctl[QC_DISTINCT], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        slot = (slot + 1) & mask;
    }
    set_err(a.ctl, QE_FULL);
}

// The seven counts' share of a value with tallies (at, en, de).
__device__ inline void class_counts(uint32_t mode, u64 at, u64 en, u64 de, u64 *v) {
#pragma unroll
    for (int i = 0; i < LC_QN_COUNTS; ++i) v[i] = 0;
    if (mode == LC_QM_UNIQUE_IDS) {
        v[LC_QN_ACKNOWLEDGED] = en;
        v[LC_QN_OK] = en > 1;
    } else {
        const u64 ok = de < at ? de : at;
        v[LC_QN_ATTEMPT] = at;
        v[LC_QN_ACKNOWLEDGED] = en;
        v[LC_QN_OK] = ok;
        v[LC_QN_UNEXPECTED] = at == 0 ? de : 0;
        v[LC_QN_DUPLICATED] = at > 0 && de > at ? de - at : 0;
        v[LC_QN_LOST] = en > de ? en - de : 0;
        v[LC_QN_RECOVERED] = ok > en ? ok - en : 0;
    }
}

__device__ inline u64 wave_sum(u64 v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ inline u64 wave_umax(u64 v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const u64 o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

// Word i of key k: a count's (wrapped) difference, or a range image.
__device__ inline void add_word(const QsArgs &a, uint32_t k, int i, u64 v) {
    u64 *w = a.keyst + (u64)k * QS_KEY_WORDS + i;
    if (i < LC_QN_COUNTS) {
        if (v) __hip_atomic_fetch_add(w, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else if (a.mode == LC_QM_UNIQUE_IDS) {
        if (v) __hip_atomic_fetch_max(w, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(QSP_BLOCK) void k_qs_settle(QsArgs a) {
    const uint32_t lane = threadIdx.x & 63;
    const u64 gid = (u64)blockIdx.x * QSP_BLOCK + threadIdx.x;
    const u64 n_dirty = a.ctl[QC_CURSOR] < a.n_rows ? a.ctl[QC_CURSOR] : a.n_rows;  // (the tally kernel's adds: an earlier kernel)
    const bool act = gid < n_dirty;
    uint32_t key = 0;
    u64 d[QS_KEY_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (act) {
        const uint32_t slot = a.dirty[gid];
        if (slot >= a.slots) {
            set_err(a.ctl, QE_STATE);
        } else {
            uint4 *p = reinterpret_cast<uint4 *>(a.table + slot);
            const uint4 w0 = p[0], w1 = p[1], w2 = p[2];
            int64_t val;
            bool ok = true;
            if (w0.x >= QS_ROW0) {
                const uint32_t rep = w0.x - QS_ROW0;
                if (rep >= a.n_rows) {
                    set_err(a.ctl, QE_STATE);
                    ok = false;
                    val = 0;
                } else {
                    key = a.row_key[rep];
                    val = a.row_val[rep];
                    p[0] = make_uint4(QS_SETTLED, key, (uint32_t)(u64)val, (uint32_t)((u64)val >> 32));
                }
            } else {
                key = w0.y;
                val = (int64_t)((u64)w0.z | ((u64)w0.w << 32));
            }
            if (ok && key < a.K) {
                u64 now[LC_QN_COUNTS], was[LC_QN_COUNTS];
                class_counts(a.mode, w1.x, w1.y, w1.z, now);
                class_counts(a.mode, w2.x, w2.y, w2.z, was);
#pragma unroll
                for (int i = 0; i < LC_QN_COUNTS; ++i) d[i] = now[i] - was[i];
                if (a.mode == LC_QM_UNIQUE_IDS && w1.y) {
                    const u64 u = (u64)val ^ SIGN;
                    d[QS_LO] = ~u;
                    d[QS_HI] = u;
                }
                p[1] = make_uint4(w1.x, w1.y, w1.z, 0u);
                p[2] = make_uint4(w1.x, w1.y, w1.z, 0u);
            } else if (ok) {
                set_err(a.ctl, QE_STATE);
                key = 0;
            }
        }
    }
    // the wave: do its dirty slots share one key?
    const u64 act_mask = __ballot(act);
    if (!act_mask) return;
    const uint32_t wkey = __shfl(key, __ffsll((long long)act_mask) - 1, 64);
    if (__all(!act || key == wkey)) {
        u64 t[QS_KEY_WORDS];
#pragma unroll
        for (int i = 0; i < LC_QN_COUNTS; ++i) t[i] = wave_sum(d[i]);
        t[QS_LO] = wave_umax(d[QS_LO]);
        t[QS_HI] = wave_umax(d[QS_HI]);
        // lane i adds word i (a select over registers, no indexed array)
        u64 mine = 0;
#pragma unroll
        for (int i = 0; i < QS_KEY_WORDS; ++i) mine = lane == (uint32_t)i ? t[i] : mine;
        if (lane < QS_KEY_WORDS) add_word(a, wkey, (int)lane, mine);
    } else if (act) {
#pragma unroll
        for (int i = 0; i < QS_KEY_WORDS; ++i) add_word(a, key, i, d[i]);
    }
}

__global__ __launch_bounds__(QSP_BLOCK) void k_qs_gather(QsArgs a) {
    const u64 gid = (u64)blockIdx.x * QSP_BLOCK + threadIdx.x;
    if (gid < (u64)a.n_touched * QS_KEY_WORDS) {
        const uint32_t k = a.touched[gid / QS_KEY_WORDS];
        a.out[QR_HEAD + gid] = k < a.K ? a.keyst[(u64)k * QS_KEY_WORDS + gid % QS_KEY_WORDS] : 0;
    }
    if (gid == 0) {
        a.out[QR_DISTINCT] = a.ctl[QC_DISTINCT];
        a.out[QR_ERR] = a.ctl[QC_ERR];
        a.out[QR_DIRTY] = a.ctl[QC_CURSOR];
        a.ctl[QC_CURSOR] = 0;
    }
}

__global__ __launch_bounds__(QSP_BLOCK) void k_qs_rehash(const QsSlot *from, uint32_t from_slots, QsSlot *to, uint32_t to_slots, u64 *ctl) {
    const u64 gid = (u64)blockIdx.x * QSP_BLOCK + threadIdx.x;
    if (gid >= from_slots) return;
    const uint4 *p = reinterpret_cast<const uint4 *>(from + gid);
    const uint4 w0 = p[0];
    if (w0.x == QS_EMPTY) return;
    if (w0.x != QS_SETTLED) {
        set_err(ctl, QE_STATE);
        return;
    }
    const uint4 w1 = p[1], w2 = p[2];
    const int64_t val = (int64_t)((u64)w0.z | ((u64)w0.w << 32));
    const uint32_t mask = to_slots - 1;
    uint32_t slot = slot_hash(w0.y, val) & mask;
    for (uint32_t seen = 0; seen < to_slots; ++seen) {
        QsSlot *s = to + slot;
        if (__hip_atomic_load(&s->state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == QS_EMPTY &&
            atomicCAS(&s->state, QS_EMPTY, QS_SETTLED) == QS_EMPTY) {
            // the slot is this lane's: no other lane reads its payload in this kernel
            s->key = w0.y;
            s->val = val;
            uint4 *q = reinterpret_cast<uint4 *>(s);
            q[1] = make_uint4(w1.x, w1.y, w1.z, 0u);
            q[2] = w2;
            return;
        }
        slot = (slot + 1) & mask;
    }
    set_err(ctl, QE_FULL);
}

constexpr int WAVES = QSP_BLOCK / 64;

__global__ __launch_bounds__(QSP_BLOCK) void k_qs_entries(QsEntArgs a) {
    __shared__ uint32_t sh_ent[WAVES];
    __shared__ u64 sh_base;
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const u64 gid = (u64)blockIdx.x * QSP_BLOCK + threadIdx.x;
    uint32_t key = 0;
    int64_t val = 0;
    u64 m[4] = {0, 0, 0, 0};
    if (gid < a.slots) {
        const uint4 *p = reinterpret_cast<const uint4 *>(a.table + gid);
        const uint4 w0 = p[0];
        if (w0.x == QS_SETTLED && w0.y < a.K && a.status[w0.y] == LC_QUEUE_KEY_OK) {
            const uint4 w1 = p[1];
            key = w0.y;
            val = (int64_t)((u64)w0.z | ((u64)w0.w << 32));
            const u64 at = w1.x, en = w1.y, de = w1.z;
            if (a.mode == LC_QM_UNIQUE_IDS) {
                m[LC_QC_DUPLICATED] = en > 1 ? en : 0;
            } else {
                const u64 ok = de < at ? de : at;
                m[LC_QC_UNEXPECTED] = at == 0 ? de : 0;
                m[LC_QC_DUPLICATED] = at > 0 && de > at ? de - at : 0;
                m[LC_QC_LOST] = en > de ? en - de : 0;
                m[LC_QC_RECOVERED] = ok > en ? ok - en : 0;
            }
        }
    }
    const uint32_t n_ent = (m[0] != 0) + (m[1] != 0) + (m[2] != 0) + (m[3] != 0);
    // the wave's inclusive scan of the entry counts
    uint32_t inc = n_ent;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t p = __shfl_up(inc, d, 64);
        if (lane >= (uint32_t)d) inc += p;
    }
    if (lane == 63) sh_ent[w] = inc;
    __syncthreads();
    uint32_t ent_before = 0, ent_total = 0;
#pragma unroll
    for (int i = 0; i < WAVES; ++i) {
        if (i < (int)w) ent_before += sh_ent[i];
        ent_total += sh_ent[i];
    }
    if (threadIdx.x == 0)
        sh_base = ent_total ? __hip_atomic_fetch_add(&a.ctl[QC_N_ENT], (u64)ent_total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
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

}  // namespace

struct QsDev {
    lc_ctx *ctx = nullptr;
    uint32_t mode = 0;
    QsSlot *table = nullptr;
    uint64_t slots = 0;
    u64 *keyst = nullptr;
    uint64_t cap_keys = 0;
    u64 *ctl = nullptr;
    Buf rows, dirty, touched, out, ent, status;
    HostBuf hin, hout, hent;
    hipEvent_t ev[6] = {};
};

namespace {

int ensure_events(QsDev &D) {
    for (hipEvent_t &e : D.ev)
        if (!e) HIPCHK(hipEventCreate(&e));
    return LC_OK;
}

// The per-key words hold `need` keys: grown by doubling, the old words copied
// device to device, the new keys' words 0.
int ensure_keys(QsDev &D, hipStream_t q, uint64_t need) {
    if (need <= D.cap_keys) return LC_OK;
    const uint64_t cap = qsp_key_cap(D.cap_keys, need);
    const size_t old_b = (size_t)D.cap_keys * QS_KEY_WORDS * 8, new_b = (size_t)cap * QS_KEY_WORDS * 8;
    u64 *p = nullptr;
    hipError_t e = hipMalloc((void **)&p, new_b);
    if (e == hipSuccess && old_b) e = hipMemcpyAsync(p, D.keyst, old_b, hipMemcpyDeviceToDevice, q);
    if (e == hipSuccess) e = hipMemsetAsync((char *)p + old_b, 0, new_b - old_b, q);
    if (e == hipSuccess) e = hipStreamSynchronize(q);
    if (e != hipSuccess) {
        if (p) (void)hipFree(p);
        return lc::fail(LC_E_DEVICE, "lc_queue_stream_append: growing the per-key words to %llu keys failed: %s",
                        (unsigned long long)cap, hipGetErrorString(e));
    }
    if (D.keyst) (void)hipFree(D.keyst);
    D.keyst = p;
    D.cap_keys = cap;
    return LC_OK;
}

}  // namespace

int qs_dev_open(lc_ctx *c, uint32_t mode, QsDev **out) {
    *out = nullptr;
    if (c->n_dev != 1 || c->comm)
        return lc::fail(LC_E_UNSUPPORTED, "lc_queue_stream_open: a stream needs a context of one device and no communicator");
    QsDev *d = new (std::nothrow) QsDev();
    if (!d) return lc::fail(LC_E_NOMEM, "lc_queue_stream_open: out of memory");
    d->ctx = c;
    d->mode = mode;
    *out = d;
    return LC_OK;
}

void qs_dev_close(QsDev *d) {
    if (!d) return;
    {
        std::lock_guard<std::mutex> g(d->ctx->mu);
        lcx::Dev *dev = d->ctx->dev[0];
        (void)hipSetDevice(dev->device);
        (void)hipStreamSynchronize(dev->stream);
        if (d->table) (void)hipFree(d->table);
        if (d->keyst) (void)hipFree(d->keyst);
        if (d->ctl) (void)hipFree(d->ctl);
        for (Buf *b : {&d->rows, &d->dirty, &d->touched, &d->out, &d->ent, &d->status}) b->release();
        for (HostBuf *b : {&d->hin, &d->hout, &d->hent}) b->release();
        for (hipEvent_t e : d->ev)
            if (e) (void)hipEventDestroy(e);
    }
    delete d;
}

int qs_dev_grow(QsDev *dp, uint64_t slots, double *ms) {
    QsDev &D = *dp;
    lcx::CtxCall x(D.ctx);
    LCCHK(x.enter());
    hipStream_t q = x.d->stream;
    *ms = 0;
    if (slots <= D.slots || slots > QSP_MAX_SLOTS || (slots & (slots - 1)))
        return lc::fail(LC_E_INVALID, "lc_queue_stream_append: a table of %llu slots after one of %llu", (unsigned long long)slots,
                        (unsigned long long)D.slots);
    LCCHK(ensure_events(D));
    if (!D.ctl) {
        HIPCHK(hipMalloc((void **)&D.ctl, QC_WORDS * 8));
        HIPCHK(hipMemsetAsync(D.ctl, 0, QC_WORDS * 8, q));
    }
    QsSlot *to = nullptr;
    if (hipMalloc((void **)&to, (size_t)qsp_bytes(slots)) != hipSuccess) {
        (void)hipGetLastError();
        return lc::fail(LC_E_NOMEM, "lc_queue_stream_append: no device memory for a table of %llu slots (%llu bytes)",
                        (unsigned long long)slots, (unsigned long long)qsp_bytes(slots));
    }
    hipError_t e = hipEventRecord(D.ev[4], q);
    if (e == hipSuccess) e = hipMemsetAsync(to, 0, (size_t)qsp_bytes(slots), q);
    if (e == hipSuccess && D.table) {
        k_qs_rehash<<<(uint32_t)qsp_blocks(D.slots), QSP_BLOCK, 0, q>>>(D.table, (uint32_t)D.slots, to, (uint32_t)slots, D.ctl);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(D.ev[5], q);
    if (e == hipSuccess) e = hipStreamSynchronize(q);
    if (e != hipSuccess) {
        (void)hipFree(to);
        return lc::fail(LC_E_DEVICE, "lc_queue_stream_append: growing the table to %llu slots failed: %s", (unsigned long long)slots,
                        hipGetErrorString(e));
    }
    // the old table goes behind the kernel that read it (the stream is idle here)
    if (D.table) (void)hipFree(D.table);
    D.table = to;
    D.slots = slots;
    float f = 0;
    HIPCHK(hipEventElapsedTime(&f, D.ev[4], D.ev[5]));
    *ms = f;
    return LC_OK;
}

int qs_dev_append(QsDev *dp, const QsChunk *c, uint64_t *words, uint64_t *distinct, double *ms3) {
    QsDev &D = *dp;
    lcx::CtxCall x(D.ctx);
    LCCHK(x.enter());
    hipStream_t q = x.d->stream;
    const size_t T = (size_t)c->n_touched;
    if (!D.table || c->n_keys > 0x7FFFFFF0ull || T > c->n_keys) return lc::fail(LC_E_INVALID, "lc_queue_stream_append: a chunk without a table or keys");
    LCCHK(ensure_events(D));
    LCCHK(ensure_keys(D, q, c->n_keys));
    const uint64_t pieces = qsp_pieces(c->n_rows);
    const size_t piece_max = (size_t)std::min<uint64_t>(c->n_rows, QSP_LAUNCH_ROWS);
    // one piece's rows on the device: values, key ids, kinds
    const size_t o_key = piece_max * 8, o_kind = o_key + up16(piece_max * 4), row_bytes = o_kind + up16(piece_max);
    HIPCHK(D.rows.grow(row_bytes));
    HIPCHK(D.dirty.grow(piece_max * 4));
    HIPCHK(D.touched.grow(T * 4));
    HIPCHK(D.hin.grow(T * 4));
    const size_t out_words = QR_HEAD + T * QS_KEY_WORDS;
    HIPCHK(D.out.grow(out_words * 8));
    HIPCHK(D.hout.grow(out_words * 8));
    if (T) std::memcpy(D.hin.p, c->touched, T * 4);

    QsArgs a{};
    a.table = D.table; a.slots = (uint32_t)D.slots;
    a.row_val = (const int64_t *)D.rows.p;
    a.row_key = (const uint32_t *)((const char *)D.rows.p + o_key);
    a.row_kind = (const uint8_t *)((const char *)D.rows.p + o_kind);
    a.K = (uint32_t)c->n_keys; a.mode = D.mode;
    a.keyst = D.keyst; a.dirty = (uint32_t *)D.dirty.p; a.ctl = D.ctl;
    a.touched = (const uint32_t *)D.touched.p; a.n_touched = (uint32_t)T;
    a.out = (u64 *)D.out.p;

    HIPCHK(hipEventRecord(D.ev[0], q));
    if (T) HIPCHK(hipMemcpyAsync(D.touched.p, D.hin.p, T * 4, hipMemcpyHostToDevice, q));
    for (uint64_t i = 0; i < pieces; ++i) {
        const uint64_t b = qsp_piece_begin(i, c->n_rows), e = qsp_piece_begin(i + 1, c->n_rows);
        const size_t n = (size_t)(e - b);
        if (i) HIPCHK(hipMemsetAsync(D.ctl + QC_CURSOR, 0, 8, q));  // (the first piece finds the last gather's reset)
        HIPCHK(hipMemcpyAsync((void *)a.row_val, c->row_val + b, n * 8, hipMemcpyHostToDevice, q));
        HIPCHK(hipMemcpyAsync((void *)a.row_key, c->row_key + b, n * 4, hipMemcpyHostToDevice, q));
        HIPCHK(hipMemcpyAsync((void *)a.row_kind, c->row_kind + b, n, hipMemcpyHostToDevice, q));
        if (i == 0) HIPCHK(hipEventRecord(D.ev[1], q));
        a.n_rows = (uint32_t)n;
        const uint32_t blocks = (uint32_t)qsp_blocks(n);
        k_qs_tally<<<blocks, QSP_BLOCK, 0, q>>>(a);
        k_qs_settle<<<blocks, QSP_BLOCK, 0, q>>>(a);
    }
    k_qs_gather<<<(uint32_t)std::max<uint64_t>(1, qsp_blocks(T * QS_KEY_WORDS)), QSP_BLOCK, 0, q>>>(a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(D.ev[2], q));
    HIPCHK(hipMemcpyAsync(D.hout.p, D.out.p, out_words * 8, hipMemcpyDeviceToHost, q));
    HIPCHK(hipEventRecord(D.ev[3], q));
    HIPCHK(hipStreamSynchronize(q));
    const u64 *ho = (const u64 *)D.hout.p;
    if (ho[QR_ERR] & QE_BAD_ROW)
        return lc::fail(LC_E_INVALID, "lc_queue_stream_append: a row_key that is not below n_keys, or a row_kind the mode has not");
    if (ho[QR_ERR])
        return lc::fail(LC_E_DEVICE, "lc_queue_stream_append: the table of %llu slots is inconsistent (error word 0x%llx)",
                        (unsigned long long)D.slots, (unsigned long long)ho[QR_ERR]);
    *distinct = ho[QR_DISTINCT];
    if (T) std::memcpy(words, ho + QR_HEAD, T * QS_KEY_WORDS * 8);
    float f = 0;
    for (int i = 0; i < 3; ++i) {
        HIPCHK(hipEventElapsedTime(&f, D.ev[i], D.ev[i + 1]));
        ms3[i] = f;
    }
    return LC_OK;
}

int qs_dev_entries(QsDev *dp, const uint8_t *status, uint64_t n_keys, uint64_t cap, uint32_t *ent_key, uint8_t *ent_class,
                   int64_t *ent_val, uint64_t *ent_mult, uint64_t *n_ent) {
    QsDev &D = *dp;
    lcx::CtxCall x(D.ctx);
    LCCHK(x.enter());
    hipStream_t q = x.d->stream;
    *n_ent = 0;
    if (!D.table || n_keys == 0) return LC_OK;
    const size_t ne = (size_t)cap;
    const size_t o_val = 0, o_mult = o_val + ne * 8, o_key = o_mult + ne * 8, o_cls = o_key + up16(ne * 4), bytes = o_cls + up16(ne);
    HIPCHK(D.ent.grow(bytes));
    HIPCHK(D.status.grow((size_t)n_keys));
    HIPCHK(D.hin.grow((size_t)n_keys));
    HIPCHK(D.hout.grow(QC_WORDS * 8));
    std::memcpy(D.hin.p, status, (size_t)n_keys);
    QsEntArgs a{};
    a.table = D.table; a.slots = (uint32_t)D.slots; a.K = (uint32_t)n_keys; a.mode = D.mode;
    a.status = (const uint8_t *)D.status.p;
    char *de = (char *)D.ent.p;
    a.ent_val = (int64_t *)(de + o_val); a.ent_mult = (u64 *)(de + o_mult); a.ent_key = (uint32_t *)(de + o_key);
    a.ent_class = (uint8_t *)(de + o_cls);
    a.ent_cap = cap; a.ctl = D.ctl;
    HIPCHK(hipMemcpyAsync(D.status.p, D.hin.p, (size_t)n_keys, hipMemcpyHostToDevice, q));
    HIPCHK(hipMemsetAsync(D.ctl + QC_N_ENT, 0, 8, q));
    k_qs_entries<<<(uint32_t)qsp_blocks(D.slots), QSP_BLOCK, 0, q>>>(a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(D.hout.p, D.ctl, QC_WORDS * 8, hipMemcpyDeviceToHost, q));
    HIPCHK(hipStreamSynchronize(q));
    const uint64_t n = ((const u64 *)D.hout.p)[QC_N_ENT];
    *n_ent = n;
    if (n == 0 || n > cap) return LC_OK;
    HIPCHK(D.hent.grow(bytes));
    HIPCHK(hipMemcpyAsync(D.hent.p, D.ent.p, bytes, hipMemcpyDeviceToHost, q));
    HIPCHK(hipStreamSynchronize(q));
    const size_t m = (size_t)n;
    std::memcpy(ent_val, D.hent.p + o_val, m * 8);
    std::memcpy(ent_mult, D.hent.p + o_mult, m * 8);
    std::memcpy(ent_key, D.hent.p + o_key, m * 4);
    std::memcpy(ent_class, D.hent.p + o_cls, m);
    return LC_OK;
}

}  // namespace lcqs
