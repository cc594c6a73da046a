// device_api.hip -- host orchestration of the device search (C ABI: lc_create,
// lc_upload, lc_check_device, lc_check_batch, lc_wait; include/lincheck.h).
// The context's types are in device_ctx.hpp, the node steps (lc_check_node*)
// in device_node.hip, the device half of lc_stream_* in device_stream.hip.
//
// This is the native side of the drop-in at etcdemo.clj:115-119: one call
// checks every key of a batch.  independent/checker's per-key pmap becomes
//   * across GPUs: contiguous key shards balanced by event count, one per
//     device of the context (one host driver thread per device), or one
//     shard per process with the verdict records all-gathered over RCCL
//     (lc_check_node);
//   * within a GPU: a work list walked by persistent kernels.
// Nothing a kernel follows is trusted unchecked: the host validates every
// index of a batch, except the per-event ones of a batch whose keys all fit
// the register tier, which T0 checks itself as it walks the events (a
// malformed event stops its key and the call returns LC_E_INVALID).

#include <dlfcn.h>

#include <atomic>
#include <chrono>
#include <cstring>
#include <functional>
#include <string>
#include <thread>

#include "device_ctx.hpp"
#include "counter_plan.hpp"
#include "queue_plan.hpp"

using namespace lcx;

const Rccl *lcx::rccl() {
    static Rccl r;
    static std::once_flag once;
    std::call_once(once, [] {
        void *h = nullptr;
        Dl_info info;
        if (dladdr((void *)&hipStreamCreateWithFlags, &info) && info.dli_fname) {
            std::string dir = info.dli_fname;
            dir = dir.substr(0, dir.find_last_of('/') + 1);
            for (const char *name : {"librccl.so.1", "librccl.so"})
                if (!h) h = dlopen((dir + name).c_str(), RTLD_NOW | RTLD_LOCAL);
        }
        if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!h) return;
        r.get_unique_id = (decltype(r.get_unique_id))dlsym(h, "ncclGetUniqueId");
        r.comm_init_rank = (decltype(r.comm_init_rank))dlsym(h, "ncclCommInitRank");
        r.comm_destroy = (decltype(r.comm_destroy))dlsym(h, "ncclCommDestroy");
        r.all_gather = (decltype(r.all_gather))dlsym(h, "ncclAllGather");
        r.error_string = (decltype(r.error_string))dlsym(h, "ncclGetErrorString");
        if (r.get_unique_id && r.comm_init_rank && r.comm_destroy && r.all_gather) r.h = h;
    });
    return r.h ? &r : nullptr;
}

namespace {

// 16-bit event words (lc_batch.events16) widened to the 32-bit form every
// kernel reads (LC_EV16_WIDE): 4 words per thread, 8-byte loads, 16-byte stores.
__global__ void k_widen16(const uint16_t *in, uint32_t *out, uint64_t n) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t n4 = n / 4;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const uint2 v = reinterpret_cast<const uint2 *>(in)[i];
        uint4 w;
        w.x = LC_EV16_WIDE(v.x & 0xFFFFu); w.y = LC_EV16_WIDE(v.x >> 16);
        w.z = LC_EV16_WIDE(v.y & 0xFFFFu); w.w = LC_EV16_WIDE(v.y >> 16);
        reinterpret_cast<uint4 *>(out)[i] = w;
    }
    for (uint64_t i = n4 * 4 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        out[i] = LC_EV16_WIDE(in[i]);
}

// Read and clear the error words of the ring slots in `mask` (one atomic
// exchange per word, so an error a still-running step raises meanwhile is
// never lost, only reported by the next read).
__global__ void k_take_err(int32_t *words, uint32_t mask, int32_t *out) {
    if (threadIdx.x != 0) return;
    for (int q = 0; q < 4; ++q) {
        const bool on = (mask >> q) & 1u;
        out[2 * q] = on ? atomicExch(&words[2 * q], 0) : 0;
        out[2 * q + 1] = on ? atomicExch(&words[2 * q + 1], 0) : 0;
    }
}

}  // namespace

using lc::HostPool;

constexpr size_t CTL_BYTES = 4 * sizeof(unsigned long long) + 16 * sizeof(int32_t);
// Beyond CTL_BYTES in the 256-byte control block: counters[16..19] the WGL
// step's, [20] the keys a competition step hands to WGL, [24..31] the error words of the last 4 LC_DEV_ASYNC steps (slot =
// the step's sequence number mod 4: a refusal is reported by the wait for
// that step), [32..39] where k_take_err leaves what it read.
constexpr int ERR_RING = 24, ERR_TAKEN = 32;
// Most device memory the speculative segments' per-key workspaces may take.
constexpr uint64_t SPEC_WS_MAX_BYTES = 8ull << 30;

// Lane 0 behind everything enqueued on lane 1: whatever follows on lane 0
// (any step but an overlapping one, a wait) sees all that was enqueued
// before it.  The next run of overlapping steps starts on lane 0 again.
namespace lcx {

int join_lanes(Dev *c) {
    if (c->lane1_live) {
        HIPCHK(hipEventRecord(c->lane[1].done, c->stream1));
        HIPCHK(hipStreamWaitEvent(c->stream, c->lane[1].done, 0));
        c->lane1_live = false;
    }
    c->run_n = 0;
    return LC_OK;
}

// The host behind both lanes (before a buffer their steps use is freed).
int drain_lanes(Dev *c) {
    HIPCHK(hipStreamSynchronize(c->stream1));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->lane1_live = c->lane1_wait_start = false;
    c->run_n = 0;
    return LC_OK;
}

int ensure_capacity(Dev *c, int64_t n_keys) {
    if (n_keys <= c->cap_keys) return LC_OK;
    int64_t cap = std::max<int64_t>(n_keys, 1024);
    if (c->n_async) LCCHK(drain_lanes(c));  // an enqueued step may still write what goes
    dfree(c->lists);
    dfree(c->peak); dfree(c->final_cfg); dfree(c->n_final); dfree(c->analyzer);
    HIPCHK(dalloc(&c->lists, (size_t)cap * 5));
    HIPCHK(dalloc(&c->analyzer, (size_t)cap));
    for (Lane &l : c->lane) {
        dfree(l.valid); dfree(l.fail_event); dfree(l.cause);
        HIPCHK(dalloc(&l.valid, (size_t)cap));
        HIPCHK(dalloc(&l.fail_event, (size_t)cap));
        HIPCHK(dalloc(&l.cause, (size_t)cap));
        for (bool &v : l.args_ok) v = false;
    }
    HIPCHK(dalloc(&c->peak, (size_t)cap));
    HIPCHK(dalloc(&c->final_cfg, (size_t)cap * (size_t)c->o->max_final * 2));
    HIPCHK(dalloc(&c->n_final, (size_t)cap));
    c->cap_keys = cap;
    return LC_OK;
}

}  // namespace lcx

// Lay out (and if needed allocate) the layered T3 workspace for `want`
// blocks: four arrays of budget + slack entries (8 B) per block.
static int ensure_lay_ws(Dev *c, int want, int *slots_out) {
    Dev::LWs &W = c->lws;
    const uint64_t cap = c->o->max_configs + (uint64_t)lcd::t3l_slack() + 64;
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    lcd::LayWs w{};
    size_t off = 0;
    w.off_S0 = off; off += al(cap * 8);
    w.off_S1 = off; off += al(cap * 8);
    w.off_I0 = off; off += al(cap * 8);
    w.off_I1 = off; off += al(cap * 8);
    w.slot_bytes = off;
    w.cap = (uint32_t)std::min<uint64_t>(cap, 0xFFFFFFFFull);
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    int slots = std::min(want, c->cu_count);
    const size_t limit = W.bytes + free_b / 2;
    while (slots > 1 && (size_t)slots * w.slot_bytes > limit) slots /= 2;
    if ((size_t)slots * w.slot_bytes > limit)
        return lc::fail(LC_E_NOMEM, "T3 workspace: one slot needs %zu bytes (budget %llu)", w.slot_bytes,
                        (unsigned long long)c->o->max_configs);
    if (!W.base || W.w.slot_bytes != w.slot_bytes || W.slots < slots) {
        dfree(W.base);
        W.bytes = 0; W.slots = 0;
        HIPCHK(hipMalloc((void **)&W.base, (size_t)slots * w.slot_bytes));
        W.bytes = (size_t)slots * w.slot_bytes;
        W.slots = slots;
    }
    w.base = W.base;
    W.w = w;
    *slots_out = std::min(slots, W.slots);
    return LC_OK;
}

// Lay out (and if needed allocate) a T3 workspace for `want` blocks.
static int ensure_ws(Dev *c, int wide, int want, int *slots_out) {
    Dev::Ws &W = c->ws[wide];
    const size_t cfg = wide ? lcd::cfg_bytes_wide() : lcd::cfg_bytes_narrow();
    const uint64_t cap = c->o->max_configs + (uint64_t)lcd::t3_block() + 64;
    uint64_t H = 1;
    while (H < 2 * cap) H <<= 1;
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    lcd::HbmWs w{};
    size_t off = 0;
    w.off_S0 = off; off += al(cap * cfg);
    w.off_S1 = off; off += al(cap * cfg);
    w.off_I = off; off += al(cap * cfg);
    w.off_hS = off; off += al(H * cfg);
    w.off_hI = off; off += al(H * cfg);
    w.off_pS0 = off; off += al(cap * 4);
    w.off_pS1 = off; off += al(cap * 4);
    w.off_pI = off; off += al(cap * 4);
    w.slot_bytes = off;
    w.cap = (uint32_t)cap;
    w.hmask = (uint32_t)(H - 1);
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    const int max_slots = c->o->deep_slots > 0 ? c->o->deep_slots : 2 * c->cu_count;
    int slots = std::min(want, max_slots);
    const size_t limit = (W.bytes ? W.bytes : 0) + free_b / 2;
    while (slots > 1 && (size_t)slots * w.slot_bytes > limit) slots /= 2;
    if ((size_t)slots * w.slot_bytes > limit)
        return lc::fail(LC_E_NOMEM, "T3 workspace: one slot needs %zu bytes (budget %llu)", w.slot_bytes,
                        (unsigned long long)c->o->max_configs);
    if (!W.base || W.w.slot_bytes != w.slot_bytes || W.slots < slots) {
        dfree(W.base);
        W.bytes = 0; W.slots = 0;
        HIPCHK(hipMalloc((void **)&W.base, (size_t)slots * w.slot_bytes));
        HIPCHK(hipMemsetAsync(W.base, 0xFF, (size_t)slots * w.slot_bytes, c->stream));  // EMPTY tables
        W.bytes = (size_t)slots * w.slot_bytes;
        W.slots = slots;
    }
    w.base = W.base;
    W.w = w;
    *slots_out = std::min(slots, W.slots);
    return LC_OK;
}

extern "C" int lc_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

static int dev_init(Dev *c, int device) {
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return lc::fail(LC_E_DEVICE, "lc_create: device %d is %s, this build targets gfx950", device, prop.gcnArchName);
    c->device = device;
    c->cu_count = prop.multiProcessorCount;
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    // (four streams, lane 1 doubling as the validation stream: a process
    // has four hardware queues by default, and a fifth stream would share
    // one with another and run behind it)
    HIPCHK(hipStreamCreateWithFlags(&c->stream1, hipStreamNonBlocking));
    c->lane[0].stream = c->stream;
    c->lane[1].stream = c->stream1;
    HIPCHK(hipStreamCreateWithFlags(&c->cstream, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&c->estream, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&c->vin, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->vdone, hipEventDisableTiming));
    for (hipEvent_t *e : {&c->e0, &c->e1, &c->et0, &c->et3a, &c->et3b, &c->ea0, &c->ea1}) HIPCHK(hipEventCreate(e));
    for (hipEvent_t &e : c->ring) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    HIPCHK(dalloc(&c->ctl, 32));
    c->acc = c->ctl;
    c->counters = (int32_t *)(c->ctl + 4);
    HIPCHK(hipMemset(c->ctl, 0, 32 * sizeof(unsigned long long)));
    HIPCHK(hipHostMalloc((void **)&c->hctl, 32 * sizeof(unsigned long long), hipHostMallocDefault));
    std::memset(c->hctl, 0, 32 * sizeof(unsigned long long));
    HIPCHK(hipEventCreateWithFlags(&c->run_start, hipEventDisableTiming));
    for (Lane &l : c->lane) {
        HIPCHK(dalloc(&l.dargs, Lane::ARGS_RING));
        HIPCHK(hipHostMalloc((void **)&l.hargs, sizeof(lcd::Args) * Lane::ARGS_RING, hipHostMallocDefault));
        for (hipEvent_t &e : l.args_ev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&l.done, hipEventDisableTiming));
    }
    return LC_OK;
}

extern "C" int lc_comm_id(uint8_t *out) {
    if (!out) return lc::fail(LC_E_INVALID, "lc_comm_id: null out");
    const Rccl *R = rccl();
    if (!R) return lc::fail(LC_E_DEVICE, "lc_comm_id: librccl.so.1 could not be loaded");
    ncclUniqueId id;
    RCCLCHK(R->get_unique_id(&id));
    std::memcpy(out, id.internal, LC_COMM_ID_BYTES);
    return LC_OK;
}

static std::atomic<int> g_live_ctx{0};

extern "C" int lc_create(const lc_opts *opts, lc_ctx **out) {
    if (!out) return lc::fail(LC_E_INVALID, "lc_create: null out");
    lc_opts o{};
    if (opts) o = *opts;
    if (o.algorithm < LC_ALGO_LINEAR || o.algorithm > LC_ALGO_COMPETITION)
        return lc::fail(LC_E_INVALID, "lc_create: algorithm must be LC_ALGO_LINEAR, _WGL or _COMPETITION");
    if (o.max_configs == 0) o.max_configs = 1ull << 20;
    if (o.max_configs > (1ull << 31)) return lc::fail(LC_E_INVALID, "lc_create: max_configs above 2^31");
    if (o.max_final <= 0) o.max_final = 10;
    if (o.max_final > 16) return lc::fail(LC_E_INVALID, "lc_create: max_final above 16");
    if (o.flags & ~LC_OPT_COUNT_PROBES) return lc::fail(LC_E_INVALID, "lc_create: unknown flags 0x%x", o.flags);
    if (o.path_flags & ~LC_PATH_ALL) return lc::fail(LC_E_INVALID, "lc_create: unknown path_flags 0x%x", o.path_flags);
    if ((o.path_flags & LC_PATH_SPLIT_ON) && (o.path_flags & LC_PATH_SPLIT_OFF))
        return lc::fail(LC_E_INVALID, "lc_create: LC_PATH_SPLIT_ON and _OFF together");
    if ((o.path_flags & LC_PATH_CHUNKS_ON) && (o.path_flags & LC_PATH_CHUNKS_OFF))
        return lc::fail(LC_E_INVALID, "lc_create: LC_PATH_CHUNKS_ON and _OFF together");
    if (o.spec_segs != 0 && o.spec_segs != 2 && o.spec_segs != 3 && o.spec_segs != 4 && o.spec_segs != 6 &&
        o.spec_segs != 8)
        return lc::fail(LC_E_INVALID, "lc_create: spec_segs must be 0, 2, 3, 4, 6 or 8");
    if (o.seg_len < 0) return lc::fail(LC_E_INVALID, "lc_create: seg_len < 0");
    // (a negative word is a ck2 past 32766 that wrapped: refused, not read as another value)
    if (o.spec_ck < 0 || (o.spec_ck && (((uint32_t)o.spec_ck & 0xFFFFu) == 0 || ((uint32_t)o.spec_ck >> 16) == 0)))
        return lc::fail(LC_E_INVALID, "lc_create: spec_ck must be 0 or (ck1 + 1) | (ck2 + 1) << 16, "
                                      "0 <= ck1 <= 65534, 0 <= ck2 <= 32766");
    if (o.n_devices < 0 || o.n_devices > MAX_DEV)
        return lc::fail(LC_E_INVALID, "lc_create: n_devices must be 0..%d", MAX_DEV);
    if (o.comm_size < 0 || o.comm_size > 4096 || (o.comm_size > 1 && (o.comm_rank < 0 || o.comm_rank >= o.comm_size)))
        return lc::fail(LC_E_INVALID, "lc_create: comm_rank %d of comm_size %d", o.comm_rank, o.comm_size);
    if (o.comm_size > 1 && o.n_devices > 1)
        return lc::fail(LC_E_INVALID, "lc_create: a rank of a multi-process node drives one device");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return lc::fail(LC_E_DEVICE, "lc_create: no HIP device visible");
    const int n = o.n_devices > 1 ? o.n_devices : 1;
    int list[MAX_DEV];
    for (int g = 0; g < n; ++g) {
        list[g] = o.n_devices > 1 ? o.devices[g] : o.device;
        if (list[g] < 0 || list[g] >= ndev) return lc::fail(LC_E_DEVICE, "lc_create: device %d of %d", list[g], ndev);
    }
    lc_ctx *c = new (std::nothrow) lc_ctx();
    if (!c) return lc::fail(LC_E_NOMEM, "lc_create: out of memory");
    c->o = o;
    for (int g = 0; g < n; ++g) {
        c->dev[g] = new (std::nothrow) Dev();
        if (!c->dev[g]) { delete c; return lc::fail(LC_E_NOMEM, "lc_create: out of memory"); }
        c->dev[g]->o = &c->o;
        c->n_dev = g + 1;
        int rc = dev_init(c->dev[g], list[g]);
        if (rc) { delete c; return rc; }
    }
    if (n > 1) c->drivers = new HostPool((unsigned)n - 1);
    // comm_size 1 with an id: a one-rank communicator (the exchange runs
    // through RCCL all the same)
    bool want_comm = o.comm_size > 1;
    for (uint8_t byte : o.comm_id) want_comm |= o.comm_size == 1 && byte != 0;
    if (want_comm) {
        const Rccl *R = rccl();
        if (!R) { delete c; return lc::fail(LC_E_DEVICE, "lc_create: librccl.so.1 could not be loaded"); }
        ncclUniqueId id;
        std::memcpy(id.internal, o.comm_id, LC_COMM_ID_BYTES);
        (void)hipSetDevice(list[0]);
        ncclResult_t r = R->comm_init_rank(&c->comm, o.comm_size, id, o.comm_rank);
        if (r != ncclSuccess) {
            c->comm = nullptr;
            delete c;
            return lc::fail(LC_E_DEVICE, "lc_create: ncclCommInitRank (rank %d of %d) failed: %s", o.comm_rank,
                            o.comm_size, R->error(r));
        }
        c->rank = o.comm_rank;
        c->size = o.comm_size;
    }
    *out = c;
    g_live_ctx.fetch_add(1);
    return LC_OK;
}

// The last context's destruction also gives back the host blocks the
// library keeps for reuse (page-locked memory is a limited resource; a JVM
// that checked once should not hold it for its life).  lc_trim does it
// at any time.
extern "C" void lc_destroy(lc_ctx *c) {
    if (!c) return;
    delete c;
    if (g_live_ctx.fetch_sub(1) == 1) lc::trim_host_caches();
}

// ---- validation -------------------------------------------------------------

// Per-event validation of a packed batch over the worker pool: every :ok
// names a pending slot, no :invoke lands in an occupied slot, every
// transition id is in range, no key uses more slots than its key_width says
// or (per-key tables) installs a state beyond its key_states.  Returns 0 or
// a reason code with the first bad key in *badkey; sets no error text.
// stage (optional): pinned host buffer that receives a copy of the event
// words; each thread copies the contiguous run of keys it validates, so the
// events are read once, in cache, on their way to the DMA engine.
// check = false: the copy alone (a batch T0 validates itself).
// Event word j of b: the 32-bit words, or the 16-bit ones widened (lc_pack
// gives only those when every word fits).
static inline uint32_t ev_at(const lc_batch *b, uint64_t j) {
    return b->events ? b->events[j] : LC_EV16_WIDE(b->events16[j]);
}

static int validate_events(const lc_batch *b, int64_t *badkey_out, uint32_t *stage, HostPool *hp, bool check = true) {
    const int64_t K = b->n_keys;
    unsigned nt = hp ? hp->size() : 1;
    if (K < 256) nt = 1;
    std::vector<int> bad((size_t)nt, 0);
    std::vector<int64_t> badkey((size_t)nt, -1);
    // contiguous key runs of about equal event counts
    const uint64_t n_ev = b->ev_off[K];
    std::vector<int64_t> cut((size_t)nt + 1, K);
    cut[0] = 0;
    for (unsigned t = 1; t < nt; ++t)
        cut[t] = std::upper_bound(b->ev_off, b->ev_off + K, n_ev * t / nt) - b->ev_off - 1;
    auto work = [&](unsigned t) {
        const int64_t k0 = std::max<int64_t>(cut[t], 0), k1 = std::max<int64_t>(cut[t + 1], k0);
        if (stage && k1 > k0) {
            if (b->events)
                std::memcpy(stage + b->ev_off[k0], b->events + b->ev_off[k0], (b->ev_off[k1] - b->ev_off[k0]) * 4);
            else
                for (uint64_t j = b->ev_off[k0]; j < b->ev_off[k1]; ++j) stage[j] = LC_EV16_WIDE(b->events16[j]);
        }
        if (!check) return;
        for (int64_t k = k0; k < k1 && !bad[t]; ++k) {
            if (b->key_error && b->key_error[k]) continue;  // not searched
            const uint64_t tb = b->trans_off ? b->trans_off[k] : 0;
            const uint32_t ns = (b->trans_off && b->key_states) ? b->key_states[k] : 0xFFFFFFFFu;
            // a table model: each op's row must lie in table[] and name only
            // states of the key (a key beyond LC_WIDE_MAX_STATES is never stepped)
            const bool rows = b->table && ns <= LC_WIDE_MAX_STATES;
            uint64_t tmax = 0;
            uint64_t pend[2] = {0, 0};
            uint32_t width = 0;
            for (uint64_t j = b->ev_off[k]; j < b->ev_off[k + 1]; ++j) {
                const uint32_t ev = ev_at(b, j);
                const uint32_t s = LC_EV_SLOT(ev);
                // slot 127 marks ops beyond the encodable window: the search
                // stops (LC_CAUSE_WINDOW) before it could follow one.
                if (ev & LC_EV_OK_BIT) {
                    if (s == 127) continue;
                    if (!((pend[s >> 6] >> (s & 63)) & 1)) { bad[t] = 1; break; }
                    pend[s >> 6] &= ~(1ull << (s & 63));
                } else {
                    const uint64_t ti = tb + LC_EV_TRANS(ev);
                    if (ti >= (uint64_t)b->n_trans) { bad[t] = 2; break; }
                    const uint32_t d = b->trans[ti], f = d & 3u;
                    if (b->table) tmax = std::max(tmax, ti + 1);
                    else if ((f == LC_T_WRITE || f == LC_T_CAS) && (d >> 17) >= ns) { bad[t] = 5; break; }
                    if (s == 127) continue;
                    if ((pend[s >> 6] >> (s & 63)) & 1) { bad[t] = 3; break; }
                    pend[s >> 6] |= 1ull << (s & 63);
                    width = std::max(width, s + 1);
                }
            }
            if (!bad[t] && b->key_width && width > b->key_width[k]) bad[t] = 4;
            for (uint64_t ti = tb; rows && !bad[t] && ti < tmax; ++ti) {
                const uint64_t r0 = b->trans[ti];
                if (r0 + ns > (uint64_t)b->n_table) { bad[t] = 5; break; }
                for (uint64_t j = 0; j < ns; ++j)
                    if (b->table[r0 + j] != LC_TABLE_NONE && b->table[r0 + j] >= ns) { bad[t] = 5; break; }
            }
            if (bad[t]) badkey[t] = k;
        }
    };
    if (hp && nt > 1) hp->run(nt, work);
    else work(0);
    for (size_t t = 0; t < bad.size(); ++t)
        if (bad[t]) { *badkey_out = badkey[t]; return bad[t]; }
    return 0;
}

static int events_error(int why, int64_t key) {
    static const char *text[] = {"", ":ok of a slot with no pending op", "transition id out of range",
                                 ":invoke into an occupied slot", "uses more window slots than key_width says",
                                 "installs a state beyond key_states"};
    return lc::fail(LC_E_INVALID, "batch: key %lld: %s", (long long)key, text[why]);
}

// Host validation of everything but the events: offsets, the transition
// table, init_state.  O(keys + transitions).
static int validate_batch(const lc_batch *b) {
    if (!b || b->n_keys < 0) return lc::fail(LC_E_INVALID, "batch: bad n_keys");
    if (b->n_keys == 0) return LC_OK;
    if (!b->ev_off || !b->trans || b->n_trans <= 0) return lc::fail(LC_E_INVALID, "batch: missing arrays");
    if (b->n_trans > 0xFFFFFFFFll) return lc::fail(LC_E_INVALID, "batch: more than 2^32 transitions");
    if (b->ev_off[0] != 0) return lc::fail(LC_E_INVALID, "batch: ev_off[0] != 0");
    for (int64_t k = 0; k < b->n_keys; ++k) {
        if (b->ev_off[k + 1] < b->ev_off[k]) return lc::fail(LC_E_INVALID, "batch: ev_off not monotone at key %lld", (long long)k);
        if (b->ev_off[k + 1] - b->ev_off[k] > 0x7FFFFFFFull) return lc::fail(LC_E_INVALID, "batch: key %lld has > 2^31 events", (long long)k);
    }
    if (b->ev_off[b->n_keys] && !b->events && !b->events16) return lc::fail(LC_E_INVALID, "batch: events missing");
    if (b->init_state >= LC_STATE_NONE) return lc::fail(LC_E_INVALID, "batch: bad init_state");
    if (b->table) {
        // rows of a table model: trans[] are offsets into table[], checked per
        // key against its state count with the events (validate_events)
        if (b->n_table <= 0 || b->n_table > 0xFFFFFFFFll || !b->trans_off || !b->key_states)
            return lc::fail(LC_E_INVALID, "batch: a table model needs n_table, trans_off and key_states");
        return LC_OK;
    }
    // Per-key tables with state counts: every install is checked against its
    // key's key_states with the events (validate_events, or T0's validation
    // on the device).  lc_pack gives the values past a key's LC_WIDE_MAX_STATES-th
    // state the id LC_STATE_NONE; such a key is never stepped (LC_CAUSE_STATES),
    // and the other keys of its batch are still searched.
    const bool per_key = b->trans_off && b->key_states;
    for (int64_t i = 0; i < b->n_trans && !per_key; ++i) {
        uint32_t d = b->trans[i];
        uint32_t f = d & 3u, bb = d >> 17;
        if ((f == LC_T_WRITE || f == LC_T_CAS) && bb >= LC_STATE_NONE)
            return lc::fail(LC_E_INVALID, "batch: transition %lld installs an invalid state", (long long)i);
    }
    return LC_OK;
}

// Would key segments pay?  A segment ends only at a quiescent point, so the
// longest stretch without one bounds the segmented search, as the whole key
// bounds the unsegmented one.  Up to 4 keys spread over the batch are
// scanned on the host (a few thousand events); segments pay when their
// longest stretch is at most a quarter of their length.
static bool segments_pay(const lc_batch *b) {
    const int64_t K = b->n_keys;
    if (K <= 0 || (!b->events && !b->events16)) return false;
    uint64_t len = 0, gap = 0;
    for (int s = 0; s < 4; ++s) {
        const int64_t k = K * s / 4;
        const uint64_t e0 = b->ev_off[k], e1 = b->ev_off[k + 1];
        int64_t pend = 0;
        uint64_t last = e0;
        for (uint64_t j = e0; j < e1; ++j) {
            pend += (ev_at(b, j) & LC_EV_OK_BIT) ? -1 : 1;
            if (pend == 0) {
                gap = std::max(gap, j + 1 - last);
                last = j + 1;
            }
        }
        gap = std::max(gap, e1 - last);
        len += e1 - e0;
    }
    return len >= 4 * 512 && gap * 4 * 4 <= len;
}

static Shape batch_shape(const lc_batch *b) {
    Shape s;
    if (b->table) return s;  // a table model: the set tiers only (no register lattice)
    uint32_t mx = b->init_state;
    for (int64_t i = 0; i < b->n_trans; ++i) {
        const uint32_t t = b->trans[i], f = t & 3u, a = (t >> 2) & 0x7FFFu, bb = t >> 17;
        if ((f == LC_T_READ || f == LC_T_CAS) && a != LC_STATE_NONE) mx = std::max(mx, a);
        if (f == LC_T_WRITE || f == LC_T_CAS) mx = std::max(mx, bb);
    }
    s.shared_states = mx + 1;
    bool installs_nil = false;
    for (int64_t i = 0; i < b->n_trans; ++i) {
        const uint32_t t = b->trans[i], f = t & 3u;
        installs_nil |= (f == LC_T_WRITE || f == LC_T_CAS) && (t >> 17) == 0;
    }
    s.taggable = !b->trans_off && s.shared_states <= 6 && b->init_state == 0 && !installs_nil;
    s.seg_pays = s.taggable && segments_pay(b);
    const int64_t K = b->n_keys;
    bool ok = K > 0 && b->key_width && b->init_state < lcd::t0_max_states();
    for (int64_t k = 0; ok && k < K; ++k) ok = b->key_width[k] <= lcd::t0_max_width();
    if (ok && b->trans_off) {
        ok = b->key_states != nullptr;
        for (int64_t k = 0; ok && k < K; ++k) ok = b->key_states[k] <= lcd::t0_max_states() && b->key_states[k] > 0;
    } else if (ok) {
        ok = s.shared_states <= lcd::t0_max_states();
    }
    s.t0_only = ok;
    return s;
}

namespace lcx {

// Is p page-locked host memory (a DMA source without a bounce)?
bool pinned(const void *p) {
    if (!p) return false;
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return at.type == hipMemoryTypeHost;
}

// Keys [k0, k1) of b as a batch of their own (ev_off rebased into `off`).
lc_batch sub_batch(const lc_batch *b, int64_t k0, int64_t k1, std::vector<uint64_t> &off) {
    lc_batch s = *b;
    s.n_keys = k1 - k0;
    off.resize((size_t)(k1 - k0) + 1);
    const uint64_t base = b->ev_off[k0];
    for (int64_t k = k0; k <= k1; ++k) off[(size_t)(k - k0)] = b->ev_off[k] - base;
    s.ev_off = off.data();
    s.events = b->events ? b->events + base : nullptr;
    if (b->trans_off) s.trans_off = b->trans_off + k0;
    if (b->key_width) s.key_width = b->key_width + k0;
    if (b->key_states) s.key_states = b->key_states + k0;
    if (b->key_error) s.key_error = b->key_error + k0;
    if (b->events16) s.events16 = b->events16 + base;
    return s;
}

// Contiguous key shards of about equal event counts, one per device.
void shard_keys(const lc_batch *b, int n, int64_t *key0) {
    const int64_t K = b->n_keys;
    const uint64_t tot = K ? b->ev_off[K] : 0;
    key0[0] = 0;
    for (int g = 1; g < n; ++g) {
        int64_t k = tot ? std::upper_bound(b->ev_off, b->ev_off + K + 1, tot * (uint64_t)g / (uint64_t)n) - b->ev_off - 1
                        : K * g / n;
        key0[g] = std::min(std::max(k, key0[g - 1]), K);
    }
    key0[n] = K;
}

// Copy a validated batch into d's device arrays (grown as needed).
// events_src: where the event words are copied from (b->events by default;
// lc_check_batch passes its pinned staging copy).  The per-key arrays and the
// transition table go through one pinned staging block and one copy; the
// event words are copied straight from the caller's (page-locked) memory.
// sync: wait for the copies (the caller may free its arrays on return);
// otherwise the caller keeps them alive until its stream has passed them.
int upload_into(Dev *c, const lc_batch *b, DevBatch *d, const Shape &sh, bool validated, const uint32_t *events_src,
                bool sync, hipStream_t stream) {
    lc::Range range("lincheck: upload");
    hipStream_t cs = stream ? stream : c->stream;
    const int64_t K = b->n_keys;
    d->device = c->device;
    d->n_keys = K;
    d->n_events = K ? b->ev_off[K] : 0;
    d->n_trans = b->n_trans > 0 ? b->n_trans : 1;
    d->init_state = b->init_state;
    d->has_trans_off = b->trans_off != nullptr;
    d->shared_states = sh.shared_states;
    d->t0_only = sh.t0_only;
    d->taggable = sh.taggable;
    d->seg_pays = sh.seg_pays;
    d->validated = validated;
    d->narrow_keys = 0;
    if (b->key_width && c->o->algorithm != LC_ALGO_LINEAR)
        for (int64_t k = 0; k < K; ++k) d->narrow_keys += b->key_width[k] <= 24;
    HIPCHK(hipSetDevice(c->device));
    // The event words first: their copy (the bulk of the bytes) runs while
    // the host stages the per-key arrays below.  A register-tier batch with
    // page-locked 16-bit words crosses the host link at 2 bytes per event and
    // is widened on the device (the register tier validates what it reads).
    HIPCHK(grow(d->mem[1], d->events, (size_t)d->n_events));
    // (a batch with no 32-bit words at all crosses as 16-bit words whatever
    // its tiers: prepare_batch widened them into events_src where the host
    // must, and the device widens them otherwise)
    const bool use16 = d->n_events && b->events16 &&
                       ((sh.t0_only && !(c->o->path_flags & LC_PATH_EV32) && (!events_src || events_src == b->events) &&
                         pinned(b->events16)) ||
                        (!b->events && !events_src));
    d->ev32_ready = !use16;
    if (use16) {
        // widened on the device only if a step's kernels need the 32-bit
        // words (dev_search); the speculative segments read these in place
        HIPCHK(grow(d->mem[3], d->events16, (size_t)d->n_events + 4));
        HIPCHK(hipMemcpyAsync(d->events16, b->events16, (size_t)d->n_events * 2, hipMemcpyHostToDevice, cs));
    } else if (d->n_events) {
        d->events16 = nullptr;
        HIPCHK(hipMemcpyAsync(d->events, events_src ? events_src : b->events, (size_t)d->n_events * 4,
                              hipMemcpyHostToDevice, cs));
    }
    // layout of the staging block (16-byte aligned pieces)
    auto al = [](size_t x) { return (x + 15) & ~(size_t)15; };
    const size_t Kz = (size_t)K;
    const size_t o_off = 0, o_order = al(o_off + (Kz + 1) * 8), o_trans = al(o_order + Kz * 4);
    const size_t o_toff = al(o_trans + (size_t)d->n_trans * 4);
    const size_t o_width = al(o_toff + (b->trans_off ? Kz * 4 : 0));
    const size_t o_states = al(o_width + (b->key_width ? Kz : 0));
    const size_t o_err = al(o_states + (b->key_states ? Kz * 2 : 0));
    const size_t bytes = al(o_err + (b->key_error ? Kz : 0));
    if (!d->hmeta_done) HIPCHK(hipEventCreateWithFlags(&d->hmeta_done, hipEventDisableTiming));
    HIPCHK(hipEventSynchronize(d->hmeta_done));  // the previous copy out of the block is done
    HIPCHK(grow_pinned(d->hmeta, d->hmeta_cap, bytes));
    char *h = d->hmeta;
    std::memcpy(h + o_off, b->ev_off, (Kz + 1) * 8);
    // LPT order: longest keys first (kept from the last upload when the
    // offsets are the same)
    int32_t *order = (int32_t *)(h + o_order);
    if (d->order_off.size() == Kz + 1 && std::memcmp(d->order_off.data(), b->ev_off, (Kz + 1) * 8) == 0) {
        std::memcpy(order, d->order_of.data(), Kz * 4);
    } else {
        std::vector<uint64_t> lk(Kz);  // (length << 32 | key), descending = LPT, ties by key
        for (size_t k = 0; k < Kz; ++k)
            lk[k] = (std::min<uint64_t>(b->ev_off[k + 1] - b->ev_off[k], 0xFFFFFFFFull) << 32) | (0xFFFFFFFFu - (uint32_t)k);
        std::sort(lk.begin(), lk.end(), std::greater<uint64_t>());
        for (size_t k = 0; k < Kz; ++k) order[k] = (int32_t)(0xFFFFFFFFu - (uint32_t)lk[k]);
        d->order_off.assign(b->ev_off, b->ev_off + Kz + 1);
        d->order_of.assign(order, order + Kz);
    }
    if (b->n_trans > 0) std::memcpy(h + o_trans, b->trans, (size_t)b->n_trans * 4);
    else std::memset(h + o_trans, 0, 4);
    if (b->trans_off) std::memcpy(h + o_toff, b->trans_off, Kz * 4);
    if (b->key_width) std::memcpy(h + o_width, b->key_width, Kz);
    if (b->key_states) std::memcpy(h + o_states, b->key_states, Kz * 2);
    if (b->key_error) std::memcpy(h + o_err, b->key_error, Kz);
    char *dm = nullptr;
    HIPCHK(grow(d->mem[0], dm, bytes));
    d->table = nullptr;
    d->n_table = b->table ? b->n_table : 0;
    if (b->table) {
        // a table model's rows (small next to the events; pageable source)
        HIPCHK(grow(d->mem[2], d->table, (size_t)b->n_table));
        HIPCHK(hipMemcpyAsync(d->table, b->table, (size_t)b->n_table * 2, hipMemcpyHostToDevice, cs));
    }
    d->ev_off = (uint64_t *)(dm + o_off);
    d->order = (int32_t *)(dm + o_order);
    d->trans = (uint32_t *)(dm + o_trans);
    d->trans_off = b->trans_off ? (uint32_t *)(dm + o_toff) : nullptr;
    d->key_width = b->key_width ? (uint8_t *)(dm + o_width) : nullptr;
    d->key_states = b->key_states ? (uint16_t *)(dm + o_states) : nullptr;
    d->key_error = b->key_error ? (uint8_t *)(dm + o_err) : nullptr;
    HIPCHK(hipMemcpyAsync(dm, h, bytes, hipMemcpyHostToDevice, cs));
    HIPCHK(hipEventRecord(d->hmeta_done, cs));
    if (sync) HIPCHK(hipStreamSynchronize(cs));
    return LC_OK;
}

}  // namespace lcx

// ---- one device's search ----------------------------------------------------

static int batch_error(int why, int64_t key) {
    return lc::fail(LC_E_INVALID, "batch: key %lld: %s", (long long)key,
                    (why & lcd::LC_BATCH_E_SLOTS)   ? "an :ok of a slot with no pending op, or an :invoke into an occupied slot"
                    : (why & lcd::LC_BATCH_E_TRANS) ? "transition id out of range, or a state beyond key_states"
                                                    : "key_width / key_states understate the key");
}

// After a readback of the control block: a malformed batch a synchronous
// step found.  The kernels name the key by its index in the caller's batch
// (Args::err_base).
static int take_error(Dev *c) {
    int32_t *cnt = (int32_t *)(c->hctl + 4);
    if (!cnt[4]) return LC_OK;
    const int why = cnt[4];
    const int64_t key = (int64_t)cnt[5] - 1;
    cnt[4] = cnt[5] = 0;
    HIPCHK(hipMemsetAsync(c->counters + 4, 0, 2 * sizeof(int32_t), c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return batch_error(why, key);
}

// The error words of the LC_DEV_ASYNC steps in ring slots `mask` (first
// `first`, when it is one of them), read and cleared on stream s.
// (enqueue, then ring_taken after the stream has passed it: dev_wait does
// both around its one synchronisation)
static int take_ring_enqueue(Dev *c, uint32_t mask, hipStream_t s) {
    hipLaunchKernelGGL(k_take_err, dim3(1), dim3(64), 0, s, c->counters + ERR_RING, mask, c->counters + ERR_TAKEN);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync((int32_t *)(c->hctl + 16), c->counters + ERR_TAKEN, 8 * sizeof(int32_t),
                          hipMemcpyDeviceToHost, s));
    return LC_OK;
}
static int ring_taken(Dev *c, int first) {
    const int32_t *h = (const int32_t *)(c->hctl + 16);
    int q = first >= 0 && h[2 * first] ? first : -1;
    for (int i = 0; i < 4 && q < 0; ++i)
        if (h[2 * i]) q = i;
    if (q < 0) return LC_OK;
    return batch_error(h[2 * q], (int64_t)h[2 * q + 1] - 1);
}
static int take_ring(Dev *c, uint32_t mask, int first, hipStream_t s) {
    const int rc = take_ring_enqueue(c, mask, s);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(s));
    return ring_taken(c, first);
}

// Segment arrays for n_keys keys (grown on demand).
static int ensure_segments(Dev *c, int64_t n_keys) {
    if (n_keys <= c->seg_keys && c->seg_ctl) return LC_OK;
    const int64_t cap = std::max<int64_t>(n_keys, 1024);
    const size_t per = (size_t)cap * lcd::SEG_MAX;
    dfree(c->seg_cnt); dfree(c->seg_end); dfree(c->seg_out); dfree(c->seg_work); dfree(c->seg_rerun);
    dfree(c->seg_rerun_init); dfree(c->seg0_fev); dfree(c->seg_ctl);
    HIPCHK(dalloc(&c->seg_cnt, (size_t)cap));
    HIPCHK(dalloc(&c->seg_end, per));
    HIPCHK(dalloc(&c->seg_out, per));
    HIPCHK(dalloc(&c->seg_work, per));
    HIPCHK(dalloc(&c->seg_rerun, (size_t)cap));
    HIPCHK(dalloc(&c->seg_rerun_init, (size_t)cap));
    HIPCHK(dalloc(&c->seg0_fev, (size_t)cap));
    HIPCHK(dalloc(&c->seg_ctl, 4));
    c->seg_keys = cap;
    return LC_OK;
}

// ---- knossos.wgl (device_wgl.hip) ---------------------------------------------

// Lowe's caches of the resident waves share at most this much of the free
// HBM (a third, and at most 96 GB); a key whose cache outgrows its share is
// searched again with a table the budget fits (fewer waves at once).  C4 at
// a budget of 2^22 (256 keys x a 2^23-entry table, 64 GB) then searches
// every key once; with a 4 GB share, 253 of its 256 keys outgrew their
// 2^19-entry tables and were searched twice (profiles/r05_c4_budget_sweep.json).
constexpr size_t WGL_SHARE_MAX = 96ull << 30;
constexpr uint64_t WGL_SPILL_ENTRIES = 1ull << 19;  // first tables when the budget's do not fit the share
constexpr uint32_t WGL_LDS_EVENTS = 8192;  // events (+ slot history) per key held in LDS

// Allocate (or reuse) WGL workspace `which` for `slots` waves of layout w.
// Contents written under another layout are cleared (a table entry is the
// key's by its stamp only where every earlier write was a table entry too).
static int ensure_wgl_ws(Dev *c, int which, const lcd::WglWs &w, int want, int *slots_out) {
    Dev::WWs &W = c->wws[which];
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    int slots = std::max(want, 1);
    const size_t limit = W.bytes + free_b / 2;
    while (slots > 1 && (size_t)slots * w.slot_bytes > limit) slots /= 2;
    if ((size_t)slots * w.slot_bytes > limit)
        return lc::fail(LC_E_NOMEM, "WGL workspace: one wave needs %zu bytes (budget %llu)", w.slot_bytes,
                        (unsigned long long)c->o->max_configs);
    const size_t need = (size_t)slots * w.slot_bytes;
    if (!W.base || W.bytes < need) {
        if (W.base) HIPCHK(hipStreamSynchronize(c->stream));
        dfree(W.base);
        W.bytes = 0; W.slots = 0; W.layout = lcd::WglWs{};
        HIPCHK(hipMalloc((void **)&W.base, need));
        HIPCHK(hipMemsetAsync(W.base, 0, need, c->stream));  // stamp 0: never a key's
        W.bytes = need;
    } else if (!W.layout.same_layout(w)) {
        HIPCHK(hipMemsetAsync(W.base, 0, W.bytes, c->stream));
    }
    W.layout = w;
    W.slots = (int)std::min<size_t>(W.bytes / w.slot_bytes, (size_t)INT32_MAX);
    *slots_out = std::min(slots, W.slots);
    return LC_OK;
}

// knossos.wgl over keys order[0 .. n): n = n_order, or *n_in (a device
// count) when n_in is given (n_hint bounds it).  Results through a's arrays;
// analyzer (device, may be null) gets LC_ALGO_WGL per key searched.
static int run_wgl(Dev *c, const DevBatch *d, const lcd::Args &a, const int32_t *order, int32_t n_order,
                   const int32_t *n_in, int64_t n_hint, uint8_t *analyzer, lc_stats *st) {
    if (n_hint <= 0 || d->n_keys == 0) return LC_OK;
    const lc_opts &o = *c->o;
    // the longest key (LPT order: the first), for the frame stack and slot history
    uint64_t max_ev = 1;
    if (!d->order_of.empty()) {
        const int32_t k0 = d->order_of[0];
        max_ev = std::max<uint64_t>(1, d->order_off[(size_t)k0 + 1] - d->order_off[(size_t)k0]);
    }
    if (max_ev > 0x7FFFFFFFull) return lc::fail(LC_E_INVALID, "WGL: a key with more than 2^31 events");
    const uint64_t need = lcd::wgl_table_entries(o.max_configs);
    const int slots_a = (int)std::min<int64_t>(n_hint, (int64_t)c->cu_count * 4);
    // Lowe's tables of the first launch: the budget's table for every resident
    // wave -- twice that (a quarter full at the budget) when the share holds
    // it -- if a third of the free HBM holds them (C4 at 2^22: 64 GB); else
    // 2^19 entries, and the keys that pass half of that are searched again
    // with the budget's table (early, so the walk repeated is short).  Both
    // measured in round 5 against tables that grow into a pool.
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    const uint64_t share = std::min<uint64_t>((c->wws[0].bytes + free_b) / 3, WGL_SHARE_MAX);
    const uint64_t per = 32ull * (uint64_t)slots_a;
    uint64_t t_a = need * per <= share ? need : std::min<uint64_t>(need, WGL_SPILL_ENTRIES);
    if (t_a == need && 2 * need * per <= share) t_a = 2 * need;
    if (o.path_flags & LC_PATH_WGL_SMALL) t_a = 1ull << 14;
    t_a = std::min(t_a, 2 * need);
    const lcd::WglWs wa = lcd::wgl_layout(o.max_configs, (uint32_t)max_ev, (uint32_t)t_a);
    int slots = 0;
    int rc = ensure_wgl_ws(c, 0, wa, slots_a, &slots);
    if (rc) return rc;
    int32_t *const ctl = c->counters + 16;  // [0] -, [1] ticket, [2] spill count, [3] spill ticket
    int32_t *const spill = c->lists + 4 * c->cap_keys;
    HIPCHK(hipMemsetAsync(ctl, 0, 4 * sizeof(int32_t), c->stream));
    lcd::WglArgs w{};
    w.ev_off = a.ev_off; w.events = a.events; w.trans = a.trans; w.trans_off = a.trans_off;
    w.key_states = a.key_states; w.key_error = a.key_error; w.table = a.table;
    w.init_state = a.init_state; w.n_trans = a.n_trans; w.budget = o.max_configs; w.max_final = o.max_final;
    // LDS per block: the first events of the key, their slot history and
    // descriptors (12 B per event), the LDS tier of the cache (8 B per entry; narrow keys), the
    // frame ring -- within a fourth of the CU's 160 KB when the launch has
    // four keys per CU (one wave each), up to 64 KB otherwise
    // (a key whose events do not all fit is searched from HBM; more than 64
    // KB per block when the launch has about one key per CU: C4's 10,000
    // events take 120 KB)
    const int64_t per_cu = std::min<int64_t>(4, std::max<int64_t>(1, (n_hint + c->cu_count - 1) / c->cu_count));
    size_t lds_cap = (160u << 10) / (size_t)per_cu - 1024;
    if (!lcd::wgl_allow_lds(lds_cap)) lds_cap = std::min<size_t>(lds_cap, 64u << 10);
    w.lds_events = (uint32_t)std::min<uint64_t>(max_ev, WGL_LDS_EVENTS);
    if (d->narrow_keys == 0) w.lds_events = (uint32_t)std::min<uint64_t>(max_ev, 3 * WGL_LDS_EVENTS / 2);
    if (o.path_flags & LC_PATH_WGL_EV_HBM) w.lds_events = 0;  // every key's events from HBM (tests)
    w.lds_tab = d->narrow_keys > 0 ? 4096u : 0u;
    w.lds_events = (w.lds_events + 1u) & ~1u;  // even: the cache tier after it is 8-byte aligned
    while (lcd::wgl_lds_bytes(w.lds_events, w.lds_tab) > lds_cap) {
        if (w.lds_tab > 1024) w.lds_tab /= 2;
        else w.lds_events = w.lds_events > 1024 ? w.lds_events - 256 : (w.lds_events / 2 + 1u) & ~1u;
    }
    w.key_width = a.key_width;
    w.order = order; w.n_order = n_order; w.n_in = n_in;
    w.ticket = ctl + 1;
    w.err = a.err;
    w.gen_base = (uint64_t)(++c->wgl_seq) << 32;
    w.spill_at = t_a < need ? (uint32_t)(t_a / 2 - 1) : 0u;
    w.spill = spill; w.n_spill = ctl + 2;
    w.ws = wa;
    w.ws.base = c->wws[0].base;
    w.valid = a.valid; w.fail_event = a.fail_event; w.cause = a.cause; w.peak = a.peak;
    w.final_cfg = a.final_cfg; w.n_final = a.n_final; w.analyzer = analyzer; w.rec = a.rec;
    w.ev_count = a.ev_count; w.keys_done = a.keys_done;
    w.probes = o.algorithm == LC_ALGO_WGL ? a.probes : nullptr;  // (competition: :linear's probe count)
    HIPCHK(hipEventRecord(c->et3a, c->stream));
    HIPCHK(lcd::launch_wgl(w, slots, c->stream));
    int32_t n_spill = 0;
    if (w.spill_at) {
        int32_t *h = (int32_t *)(c->hctl + 4) + 18;
        HIPCHK(hipMemcpyAsync(h, ctl + 2, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        n_spill = *h;
        if (n_spill > 0) {
            const lcd::WglWs wb = lcd::wgl_layout(o.max_configs, (uint32_t)max_ev, 0);
            rc = ensure_wgl_ws(c, 1, wb, (int)std::min<int64_t>(n_spill, (int64_t)c->cu_count * 4), &slots);
            if (rc) return rc;
            w.order = spill; w.n_order = 0; w.n_in = ctl + 2;
            w.ticket = ctl + 3;
            w.gen_base = (uint64_t)(++c->wgl_seq) << 32;
            w.spill_at = 0;
            w.ws = wb;
            w.ws.base = c->wws[1].base;
            HIPCHK(lcd::launch_wgl(w, slots, c->stream));
        }
    }
    HIPCHK(hipEventRecord(c->et3b, c->stream));
    if (st) st->wgl_spilled += (uint64_t)n_spill;
    return LC_OK;
}

// One search step, as dev_search's stages see it: where it runs, its plan
// (step_plan.hpp), the Args every launch of it shares, and what the tiers
// leave for fill_stats.
struct Step {
    Dev *c;
    const DevBatch *d;
    const lc_result *r;
    ResMode mode;
    int64_t K;
    std::chrono::steady_clock::time_point t0;
    lc::StepPlan p;
    lcd::Args a{};
    uint8_t *analyzer = nullptr;  // which analysis answered each key (lc_result.analyzer), or null
    uint32_t ticket_base = 0;
    bool t3 = false;
    unsigned long long probes_pre_t3 = 0;
    int32_t n_deep = 0, n_widek = 0;
    float ms = 0, ms0 = 0, ms3 = 0, msw = 0;
    uint64_t wgl_keys = 0, wgl_steps = 0, wgl_spilled = 0;
    Lane *L = nullptr;             // the lane whose scratch and result arrays the step uses
    hipStream_t q = nullptr;       // ... and its stream (lane 0's for every step but an overlapping one)
    const LaneUse *lu = nullptr;
};

// The work lists between the tiers (Dev::lists) and their counts (Dev::counters).
struct Lists {
    int32_t *spill0, *spill1, *spill2, *wide, *old_narrow;
    int32_t *n_spill0, *n_spill1, *n_spill2, *n_wide;
};
static Lists lists_of(const Dev *c) {
    return {c->lists, c->lists + c->cap_keys, c->lists + 2 * c->cap_keys, c->lists + 3 * c->cap_keys,
            c->lists + 4 * c->cap_keys, c->counters + 0, c->counters + 1, c->counters + 2, c->counters + 3};
}

// The Args every launch of the step shares (strict and, for an enqueued
// step, err follow the plan), and the step's analyzer array.
static void step_args(Step &s, int64_t key0, int64_t res_off) {
    Dev *c = s.c;
    const DevBatch *d = s.d;
    const lc_result *r = s.r;
    const ResMode mode = s.mode;
    const lc_opts &o = *c->o;
    lcd::Args &a = s.a;
    a.ev_off = d->ev_off; a.events = d->events; a.trans = d->trans; a.trans_off = d->trans_off;
    a.key_width = d->key_width; a.key_states = d->key_states; a.key_error = d->key_error;
    a.table = d->table;
    a.init_state = d->init_state; a.shared_states = d->shared_states;
    a.n_trans = (uint32_t)d->n_trans;
    a.budget = o.max_configs; a.max_final = o.max_final; a.debug_mode = o.debug_mode;
    a.count_probes = (o.flags & LC_OPT_COUNT_PROBES) ? 1 : 0;
    if (mode == RES_DEV) {
        a.valid = r->valid; a.fail_event = r->fail_event; a.cause = r->cause;
        a.peak = r->peak_configs; a.final_cfg = r->final_configs; a.n_final = r->n_final;
    } else {
        a.valid = s.L->valid + res_off; a.fail_event = s.L->fail_event + res_off; a.cause = s.L->cause + res_off;
        a.peak = (mode == RES_HOST && r->peak_configs) ? c->peak : nullptr;
        a.final_cfg = (mode == RES_HOST && r->final_configs) ? c->final_cfg : nullptr;
        a.n_final = (mode == RES_HOST && r->n_final) ? c->n_final : nullptr;
    }
    a.rec = c->rec_out ? c->rec_out + res_off : nullptr;
    a.probes = c->acc + 0; a.ev_count = c->acc + 1; a.keys_done = c->acc + 2; a.stream_bytes = c->acc + 3;
    a.err = c->counters + 4;
    a.err_base = (int32_t)key0;  // malformed keys are reported by their index in the caller's batch
    a.list_cap = (int32_t)c->cap_keys;
    s.analyzer = mode == RES_DEV ? r->analyzer : (mode == RES_HOST && r->analyzer) ? c->analyzer : nullptr;
}

// What plan_step decides from: the batch, the options, what s.a asks for.
static lc::StepIn step_in(const Step &s, bool allow_async) {
    const DevBatch *d = s.d;
    const lc_opts &o = *s.c->o;
    lc::StepIn in;
    in.K = s.K; in.n_events = d->n_events; in.cu_count = s.c->cu_count;
    in.t0_only = d->t0_only; in.table = d->table != nullptr; in.taggable = d->taggable; in.seg_pays = d->seg_pays;
    in.validated = d->validated; in.has_events16 = d->events16 != nullptr;
    in.algorithm = o.algorithm; in.flags = o.flags; in.path_flags = o.path_flags; in.spec_segs = o.spec_segs;
    in.max_configs = o.max_configs;
    in.want_peak = s.a.peak != nullptr; in.want_final = s.a.final_cfg != nullptr; in.want_n_final = s.a.n_final != nullptr;
    in.res_host = s.mode == RES_HOST; in.allow_async = allow_async;
    in.spec8_waves = LC_SPEC8_WAVES;
    in.ws_words = lcd::spec_ws_words(1, 1); in.fin_words = lcd::spec_fin_words(1, 1);
    in.ws_max_bytes = SPEC_WS_MAX_BYTES;
    return in;
}

// The 32-bit event words every kernel but k_spec reads, widened once per
// upload from a batch's 16-bit ones.
static int ensure_ev32(Dev *c, const DevBatch *d, hipStream_t q) {
    if (d->ev32_ready || !d->n_events) return LC_OK;
    const uint64_t n4 = (d->n_events + 3) / 4;
    const int blocks = (int)std::min<uint64_t>((n4 + 255) / 256, (uint64_t)c->cu_count * 8);
    hipLaunchKernelGGL(k_widen16, dim3(std::max(blocks, 1)), dim3(256), 0, q, d->events16, d->events,
                       d->n_events);
    HIPCHK(hipGetLastError());
    d->ev32_ready = true;
    return LC_OK;
}

// Zero the control block: everything but the error words (a malformed batch
// reported at the next wait keeps them until then).
static int zero_control(Dev *c, hipStream_t q) {
    HIPCHK(hipMemsetAsync(c->ctl, 0, 4 * sizeof(unsigned long long) + 4 * sizeof(int32_t), q));
    HIPCHK(hipMemsetAsync(c->counters + 6, 0, 10 * sizeof(int32_t), q));
    return LC_OK;
}

// The control block, and with RES_HOST the results, to the host; then the
// stream's end and the step's error words.
static int readback(const Step &s) {
    Dev *c = s.c;
    const lc_result *r = s.r;
    const size_t K = (size_t)s.K;
    HIPCHK(hipEventRecord(c->e1, c->stream));
    HIPCHK(hipMemcpyAsync(c->hctl, c->ctl, CTL_BYTES, hipMemcpyDeviceToHost, c->stream));
    if (s.mode == RES_HOST && K > 0) {
        HIPCHK(hipMemcpyAsync(r->valid, s.L->valid, K, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(r->fail_event, s.L->fail_event, K * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(r->cause, s.L->cause, K, hipMemcpyDeviceToHost, c->stream));
        if (r->peak_configs) HIPCHK(hipMemcpyAsync(r->peak_configs, c->peak, K * 4, hipMemcpyDeviceToHost, c->stream));
        if (r->final_configs)
            HIPCHK(hipMemcpyAsync(r->final_configs, c->final_cfg, K * c->o->max_final * 16, hipMemcpyDeviceToHost,
                                  c->stream));
        if (r->n_final) HIPCHK(hipMemcpyAsync(r->n_final, c->n_final, K * 4, hipMemcpyDeviceToHost, c->stream));
        if (r->analyzer) HIPCHK(hipMemcpyAsync(r->analyzer, c->analyzer, K, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return take_error(c);
}

// The :wgl-only step: knossos.wgl's own search (device_wgl.hip) for every key.
static int search_wgl(Step &s, lc_stats *st) {
    Dev *c = s.c;
    const DevBatch *d = s.d;
    const int64_t K = s.K;
    LCCHK(zero_control(c, c->stream));
    c->ticket_live = false;
    LCCHK(ensure_ev32(c, d, c->stream));
    if (s.a.n_final && K > 0) HIPCHK(hipMemsetAsync(s.a.n_final, 0, (size_t)K * 4, c->stream));
    HIPCHK(hipEventRecord(c->e0, c->stream));
    if (!d->validated && K > 0) {  // the per-event checks the host skipped, ahead of the walk
        lcd::Args av = s.a;
        av.n_order = (int32_t)K;
        HIPCHK(lcd::launch_validate(av, c->stream, true));
    }
    lc_stats ws{};
    LCCHK(run_wgl(c, d, s.a, d->order, (int32_t)K, nullptr, K, s.analyzer, &ws));
    LCCHK(readback(s));
    float ms = 0, msw = 0;
    HIPCHK(hipEventElapsedTime(&ms, c->e0, c->e1));
    if (K > 0) HIPCHK(hipEventElapsedTime(&msw, c->et3a, c->et3b));
    if (st) {
        *st = lc_stats{};
        st->kernel_ms = ms;
        st->wgl_ms = msw;
        st->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - s.t0).count();
        st->lds_keys = c->hctl[2];
        st->wgl_keys = c->hctl[2];
        st->wgl_steps = c->hctl[1];
        st->events = c->hctl[1];
        st->probes = c->hctl[0];  // Lowe's cache lookups
        st->wgl_spilled = ws.wgl_spilled;
    }
    return LC_OK;
}

// k_spec's per-key workspaces, the exact runs' saved sets, the rerun list:
// the step's lane's own.
static int ensure_spec_ws(const Step &s) {
    Dev *c = s.c;
    Lane &L = *s.L;
    LCCHK(grow_dev(c, L.spec_ws, L.spec_ws_words, lcd::spec_ws_words(s.K, s.p.segs)));
    LCCHK(grow_dev(c, L.spec_fin, L.spec_fin_words, s.p.exact ? lcd::spec_fin_words(s.K, s.p.segs) : (size_t)0));
    const int64_t rr_had = L.spec_rr_cap;
    LCCHK(grow_dev(c, L.spec_rr, L.spec_rr_cap, s.K + 2));
    if (L.spec_rr_cap != rr_had) HIPCHK(hipMemsetAsync(L.spec_rr, 0, 2 * sizeof(int32_t), s.q));
    return LC_OK;
}

// T0's Args -- every key, LPT order; keys outside the register lattice spill
// to T1 -- and the ticket the step starts from: a T0-only step continues the
// previous one's, any other zeroes the control block.
static int t0_args(Step &s, lcd::Args *a0) {
    Dev *c = s.c;
    if (s.p.t0_step && c->ticket_live && !s.p.competition) {
        s.ticket_base = c->ticket_next;
    } else {
        // (of a run of overlapping steps only the first comes here, on lane
        // 0, ahead of run_start: the later ones find the ticket live)
        LCCHK(zero_control(c, s.q));
    }
    c->ticket_live = false;
    if (s.a.n_final && s.K > 0) HIPCHK(hipMemsetAsync(s.a.n_final, 0, (size_t)s.K * 4, s.q));
    const Lists l = lists_of(c);
    *a0 = s.a;
    a0->order = s.d->order; a0->n_order = (int32_t)s.K; a0->n_in = nullptr; a0->ticket = c->counters + 8;
    a0->spill = l.spill0; a0->n_spill = l.n_spill0; a0->wide = l.wide; a0->n_wide = l.n_wide;
    a0->deep = l.spill2; a0->n_deep = l.n_spill2;  // very wide keys: straight to T3
    a0->lat_ws = nullptr;
    return LC_OK;
}

// T0 reads the result/counter/list pointers from a device copy of its
// Args: a ring slot holding these Args, else the next slot, refreshed
// (device copies are rewritten in stream order, after the launches that
// read them: the ring is the lane's own, whose stream every step of the lane
// runs on)
static int args_slot(Lane &L, const lcd::Args &a0, lcd::Args **dargs) {
    int aslot = -1;
    for (int q = 0; q < Lane::ARGS_RING && aslot < 0; ++q)
        if (L.args_ok[q] && std::memcmp(L.hargs + q, &a0, sizeof a0) == 0) aslot = q;
    if (aslot < 0) {
        aslot = (int)(L.args_next++ % Lane::ARGS_RING);
        HIPCHK(hipEventSynchronize(L.args_ev[aslot]));  // its staging copy has been read
        std::memcpy(L.hargs + aslot, &a0, sizeof a0);
        HIPCHK(hipMemcpyAsync(L.dargs + aslot, L.hargs + aslot, sizeof(lcd::Args), hipMemcpyHostToDevice, L.stream));
        HIPCHK(hipEventRecord(L.args_ev[aslot], L.stream));
        L.args_ok[aslot] = true;
    }
    *dargs = L.dargs + aslot;
    return LC_OK;
}

static lcd::SegArgs seg_args(const Step &s, int grid) {
    Dev *c = s.c;
    const DevBatch *d = s.d;
    const lcd::Args &a = s.a;
    lcd::SegArgs sa{};
    sa.ev_off = d->ev_off; sa.events = d->events; sa.trans = d->trans; sa.key_error = d->key_error;
    sa.n_trans = (uint32_t)d->n_trans; sa.n_keys = (int32_t)s.K; sa.max_seg = lcd::SEG_MAX;
    // segments of about fill x (resident waves / keys) per key
    const double per_key = std::max(1.0, 2.0 * grid / (double)s.K);
    sa.seg_len = (uint32_t)std::max<double>(64.0, (double)d->n_events / (double)s.K / per_key);
    if (c->o->seg_len > 0) sa.seg_len = (uint32_t)c->o->seg_len;
    sa.seg_cnt = c->seg_cnt; sa.seg_end = c->seg_end; sa.seg_out = c->seg_out; sa.seg0_fev = c->seg0_fev;
    sa.work = c->seg_work; sa.rerun = c->seg_rerun; sa.rerun_init = c->seg_rerun_init; sa.ctl = c->seg_ctl;
    sa.err = a.err; sa.valid = a.valid; sa.fail_event = a.fail_event; sa.cause = a.cause;
    sa.rec = a.rec;
    sa.strict = a.strict;
    sa.err_base = a.err_base;
    return sa;
}

static lcd::SpecLaunch spec_launch(const Step &s) {
    Dev *c = s.c;
    const lc_opts &o = *c->o;
    lcd::SpecLaunch l{};
    l.segs = s.p.segs;
    l.ws = s.L->spec_ws; l.rr = s.L->spec_rr; l.parity = s.L->spec_parity;
    // (spec_ck == 0: the defaults; else (ck1 + 1) | (ck2 + 1) << 16)
    l.ck1 = o.spec_ck ? ((uint32_t)o.spec_ck & 0xFFFFu) - 1u : 32u;
    l.ck2 = o.spec_ck ? ((uint32_t)o.spec_ck >> 16) - 1u : 120u;
    // the rerun launch usually finds no key: a few one-wave blocks, so that
    // its dispatch never queues behind the other lane's k_spec blocks; a
    // longer rerun list walks the grid (step_plan.hpp)
    l.rerun_grid = s.p.rerun_grid;
    l.validate_blocks = s.p.spec_vblocks;
    l.events16 = s.p.ev16 ? s.d->events16 : nullptr;
    l.cost_cuts = (o.path_flags & LC_PATH_SPEC_COST) != 0;
    // Issue priority by progress helps a launch that has the device to
    // itself (its laggards run ahead); beside another step's launch, whose
    // fresh blocks would all outrank this one's tail, wave age alone measured
    // better (C2, 200 overlapping steps: 0.1735 against 0.1796 ms per step;
    // one search at a time 0.2130 with it, 0.2568 without)
    // (A/B: make variant VFLAGS=-DLC_SPEC_PRIO_OVERLAP=1 keeps it on there)
#ifndef LC_SPEC_PRIO_OVERLAP
#define LC_SPEC_PRIO_OVERLAP 0
#endif
    l.prio = !(o.path_flags & LC_PATH_SPEC_NOPRIO) && (LC_SPEC_PRIO_OVERLAP || !(s.lu && s.lu->overlap));
    l.vfirst = s.p.spec_vfirst;
    l.fin = s.p.exact ? s.L->spec_fin : nullptr;
    l.stage = !(o.path_flags & LC_PATH_SPEC_NOSTAGE);
    return l;
}

// The register tier's launch -- key segments, speculative segments or the
// lattice; none for a table model -- with the validation the host skipped
// beside it on the second stream where the plan says so, joined before the
// set tiers and the readback.
static int launch_register_tier(Step &s, const lcd::Args &a0, const lcd::Args *dargs) {
    Dev *c = s.c;
    const lc::StepPlan &p = s.p;
    const int64_t K = s.K;
    if (p.side_validate) {
        HIPCHK(hipEventRecord(c->vin, c->stream));
        HIPCHK(hipStreamWaitEvent(c->stream1, c->vin, 0));
        lcd::Args av = s.a;
        av.n_order = (int32_t)K;
        HIPCHK(lcd::launch_validate(av, c->stream1, p.gen_validate));
        HIPCHK(hipEventRecord(c->vdone, c->stream1));
    }
    // (et0 only where its time is read: each recorded event costs the stream
    // a few microseconds between kernels)
    if (p.split) {
        const int grid = c->cu_count * 12;
        HIPCHK(hipMemsetAsync(c->seg_ctl, 0, 4 * sizeof(int32_t), c->stream));
        HIPCHK(lcd::launch_segments(seg_args(s, grid), grid, c->stream));
        if (!p.async) HIPCHK(hipEventRecord(c->et0, c->stream));
    } else if (p.spec) {
        HIPCHK(lcd::launch_spec(a0, dargs, spec_launch(s), s.q));
        s.L->spec_parity ^= 1;
        if (!p.async) HIPCHK(hipEventRecord(c->et0, s.q));
    } else if (K > 0 && !s.d->table) {
        HIPCHK(lcd::launch_t0(a0, dargs, p.g0, p.t0_wide, c->stream, s.ticket_base));
        if (!p.async) HIPCHK(hipEventRecord(c->et0, c->stream));
    } else if (K > 0) {
        HIPCHK(hipEventRecord(c->et0, c->stream));  // a table model: no register lattice
    }
    if (p.side_validate) HIPCHK(hipStreamWaitEvent(c->stream, c->vdone, 0));
    return LC_OK;
}

// Where the next T0-only step's ticket continues from.
static void keep_ticket(const Step &s) {
    s.c->ticket_next = (s.p.split || s.p.spec) ? s.ticket_base : s.ticket_base + (uint32_t)s.K + (uint32_t)s.p.g0;
    s.c->ticket_live = true;
}

// The end of an enqueued step: its ring event, nothing read back.
static int finish_async(const Step &s, lc_stats *st, bool *enqueued) {
    Dev *c = s.c;
    // (the span's end, ea1, is recorded by dev_wait after the last
    // enqueued step: one timing event per step cost the stream a few
    // microseconds between searches)
    if (s.lu && s.lu->dst) {
        // records that went into the lane's block: out to the caller's
        // buffer, behind the step that was given that buffer before (the
        // wait stands after the searches' launches, so it delays neither)
        if (s.lu->after) HIPCHK(hipStreamWaitEvent(s.q, s.lu->after, 0));
        HIPCHK(hipMemcpyAsync(s.lu->dst, s.L->rec, s.lu->n * 8, hipMemcpyDeviceToHost, s.q));
    }
    HIPCHK(hipEventRecord(c->ring[c->async_seq % 4], s.q));
    if (s.lu && s.lu->overlap) {
        ++c->run_n;
        c->lane1_live |= s.lu->lane == 1;
    }
    c->ea1_pending = true;
    ++c->async_seq;
    ++c->n_async;
    keep_ticket(s);
    if (st) {  // times come from lc_wait
        *st = lc_stats{};
        st->t0_path = s.p.t0_path;
        st->ev_word_bytes = s.p.ev_word_bytes;
    }
    if (enqueued) *enqueued = true;
    return LC_OK;
}

// T1 (LDS hash sets) over the keys T0 spilled -- every key of a table model
// -- then T2 over the keys that outgrew T1.
static int run_set_tiers(const Step &s) {
    Dev *c = s.c;
    const Lists l = lists_of(c);
    lcd::Args a1 = s.a;
    a1.order = l.spill0; a1.n_order = 0; a1.n_in = l.n_spill0; a1.ticket = c->counters + 9;
    if (s.d->table) { a1.order = s.d->order; a1.n_order = (int32_t)s.K; a1.n_in = nullptr; }  // every key
    a1.spill = l.spill1; a1.n_spill = l.n_spill1; a1.wide = l.wide; a1.n_wide = l.n_wide;
    int g1 = (int)std::min<int64_t>(s.K, (int64_t)c->cu_count * 7);
    HIPCHK(lcd::launch_t1(a1, g1, c->stream));
    lcd::Args a2 = s.a;
    a2.order = l.spill1; a2.n_order = 0; a2.n_in = l.n_spill1; a2.ticket = c->counters + 10;
    a2.spill = l.spill2; a2.n_spill = l.n_spill2; a2.wide = l.wide; a2.n_wide = l.n_wide;
    HIPCHK(lcd::launch_t2(a2, c->cu_count, c->stream));
    return LC_OK;
}

// The end of a synchronous T0-only step: only the error words come back,
// unless the results go to host memory.
static int read_t0_step(const Step &s) {
    Dev *c = s.c;
    int rc;
    if (s.mode != RES_HOST) {
        HIPCHK(hipEventRecord(c->e1, c->stream));
        HIPCHK(hipMemcpyAsync(c->hctl + 6, c->counters + 4, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        rc = take_error(c);
    } else {
        rc = readback(s);
    }
    std::memset(c->hctl, 0, CTL_BYTES);  // counters not kept on this path
    keep_ticket(s);
    return rc;
}

// T3 (HBM tier): keys beyond T2 (s.n_deep), then keys needing wide configs.
// Each launch's workspace is sized from the counts the one before it left.
static int run_hbm_tier(Step &s) {
    Dev *c = s.c;
    const Lists l = lists_of(c);
    const int32_t *cnt = (const int32_t *)(c->hctl + 4);
    s.t3 = true;
    HIPCHK(hipEventRecord(c->et3a, c->stream));
    lcd::Args a3 = s.a;
    a3.wide = l.wide; a3.n_wide = l.n_wide;
    // Narrow keys: the layered form first (<= 8 states; LC_PATH_LAYERS_OFF
    // turns it off for A/B runs), the config-keyed narrow tier for the
    // keys it hands on (cnt[6]).
    // (the layered form steps ops as register-state masks: not a table model)
    const bool layers = !s.d->table && !(c->o->path_flags & LC_PATH_LAYERS_OFF);
    int32_t *narrow_list = l.spill2, *narrow_n = l.n_spill2;
    int32_t n_narrow = s.n_deep;
    int slots = 0;
    if (s.n_deep > 0 && layers) {
        LCCHK(ensure_lay_ws(c, s.n_deep, &slots));
        a3.order = l.spill2; a3.n_order = 0; a3.n_in = l.n_spill2; a3.ticket = c->counters + 11;
        a3.spill = l.old_narrow; a3.n_spill = c->counters + 6;
        HIPCHK(lcd::launch_t3_layers(a3, c->lws.w, slots, c->stream));
        HIPCHK(hipMemcpyAsync(c->hctl, c->ctl, CTL_BYTES, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        narrow_list = l.old_narrow; narrow_n = c->counters + 6;
        n_narrow = cnt[6];
    }
    if (n_narrow > 0) {
        LCCHK(ensure_ws(c, 0, n_narrow, &slots));
        a3.order = narrow_list; a3.n_order = 0; a3.n_in = narrow_n; a3.ticket = c->counters + 13;
        HIPCHK(lcd::launch_t3_narrow(a3, c->ws[0].w, slots, c->stream));
        HIPCHK(hipMemcpyAsync(c->hctl, c->ctl, CTL_BYTES, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    if (cnt[3] > 0) {
        LCCHK(ensure_ws(c, 1, cnt[3], &slots));
        a3.order = l.wide; a3.n_order = 0; a3.n_in = l.n_wide; a3.ticket = c->counters + 12;
        HIPCHK(lcd::launch_t3_wide(a3, c->ws[1].w, slots, c->stream));
    }
    HIPCHK(hipEventRecord(c->et3b, c->stream));
    return readback(s);
}

// knossos.competition: the keys :linear left :unknown at its budget are
// answered by WGL's search (the analysis that could still finish)
static int run_competition(Step &s) {
    Dev *c = s.c;
    const unsigned long long *acc = c->hctl;
    int32_t *const list = c->lists, *const count = c->counters + 20;  // (run_wgl zeroes [16..19])
    HIPCHK(hipMemsetAsync(count, 0, sizeof(int32_t), c->stream));
    HIPCHK(lcd::launch_collect_budget(s.a.cause, (int32_t)s.K, list, count, c->stream));
    int32_t *h = (int32_t *)(c->hctl + 4) + 20;
    HIPCHK(hipMemcpyAsync(c->hctl, c->ctl, CTL_BYTES, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(h, count, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const int32_t n_b = *h;
    const uint64_t ev0 = acc[1];
    if (n_b <= 0) return LC_OK;
    lc_stats ws{};
    LCCHK(run_wgl(c, s.d, s.a, list, 0, count, n_b, s.analyzer, &ws));
    LCCHK(readback(s));
    HIPCHK(hipEventElapsedTime(&s.msw, c->et3a, c->et3b));
    HIPCHK(hipEventElapsedTime(&s.ms, c->e0, c->e1));
    s.wgl_keys = (uint64_t)n_b;
    s.wgl_steps = acc[1] - ev0;
    s.wgl_spilled = ws.wgl_spilled;
    return LC_OK;
}

static void fill_stats(const Step &s, lc_stats *st) {
    const unsigned long long *acc = s.c->hctl;
    st->kernel_ms = s.ms;
    st->tier0_ms = s.ms0;
    st->tier3_ms = s.ms3;
    st->probes_t3 = s.t3 ? acc[0] - s.probes_pre_t3 : 0;
    st->t3_bytes = s.t3 ? acc[3] : 0;
    st->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - s.t0).count();
    st->probes = acc[0];
    st->events = acc[1];
    st->lds_keys = acc[2];
    st->deep_keys = (uint64_t)(s.n_deep + s.n_widek);  // keys the HBM tier (re)searched
    st->t0_path = s.p.t0_path;
    st->ev_word_bytes = s.p.ev_word_bytes;
    st->wgl_ms = s.msw;
    st->wgl_keys = s.wgl_keys;
    st->wgl_steps = s.wgl_steps;
    st->wgl_spilled = s.wgl_spilled;
}

// Search d on c.  RES_HOST: r's arrays are host memory and receive the
// results; RES_DEV: r's arrays are device memory on c; RES_CTX: results stay
// in c's own device arrays (r unused).  allow_async: a step that is T0 alone
// is only enqueued (*enqueued = true; errors surface at the next wait).
// What runs is plan_step's choice (step_plan.hpp); this is the order it runs in.
// lu: an overlapping step of lc_check_node_async and its lane (plan_lane's
// choice, lane_plan.hpp); any other step runs on lane 0, behind everything
// enqueued on either lane before it.
int lcx::dev_search(Dev *c, const DevBatch *d, const lc_result *r, ResMode mode, bool allow_async, int64_t key0,
                    lc_stats *st, bool *enqueued, int64_t res_off, const LaneUse *lu) {
    lc::Range range("lincheck: search");
    if (enqueued) *enqueued = false;
    const auto t0 = std::chrono::steady_clock::now();
    HIPCHK(hipSetDevice(c->device));
    const int64_t K = d->n_keys;
    if (K > 0x7FFFFFFF) return lc::fail(LC_E_INVALID, "lc_check_device: too many keys");
    const bool overlap = lu && lu->overlap;
    if (!overlap) LCCHK(join_lanes(c));
    LCCHK(ensure_capacity(c, K));
    Step s{c, d, r, mode, K, t0};
    s.lu = lu;
    s.L = &c->lane[overlap ? lu->lane : 0];
    s.q = s.L->stream;
    step_args(s, key0, res_off);
    s.p = lc::plan_step(step_in(s, allow_async));
    const lc::StepPlan &p = s.p;
    if (overlap && !(p.async && p.spec))
        return lc::fail(LC_E_DEVICE, "lc_check_node_async: an overlapping step left the speculative segments");
    if (overlap && lu->lane == 1 && c->lane1_wait_start) {  // lane 0's set-up of this run, once
        HIPCHK(hipStreamWaitEvent(s.q, c->run_start, 0));
        c->lane1_wait_start = false;
    }
    s.a.strict = p.strict ? 1 : 0;
    if (s.analyzer && K > 0 && !p.wgl_only) HIPCHK(hipMemsetAsync(s.analyzer, LC_ALGO_LINEAR, (size_t)K, c->stream));
    if (p.wgl_only) return search_wgl(s, st);
    if (!p.async && c->ea1_pending) {  // the asynchronous steps' span ends before this one
        HIPCHK(hipEventRecord(c->ea1, c->stream));
        c->ea1_pending = false;
    }
    // an enqueued step reports a malformed batch through its own error words
    if (p.async) s.a.err = c->counters + ERR_RING + 2 * (int)(c->async_seq % 4);
    if (p.split) LCCHK(ensure_segments(c, K));
    if (p.spec) LCCHK(ensure_spec_ws(s));
    if (!p.ev16) LCCHK(ensure_ev32(c, d, s.q));
    lcd::Args a0{}, *dargs = nullptr;  // (zeroed padding too: args_slot compares the bytes)
    LCCHK(t0_args(s, &a0));
    LCCHK(args_slot(*s.L, a0, &dargs));
    // timing events only where their times are read (each recorded event
    // costs the stream a few microseconds between kernels): an enqueued step
    // is timed by the span ea0 .. ea1 alone
    if (!p.async) HIPCHK(hipEventRecord(c->e0, c->stream));
    if (p.async && c->n_async == 0) HIPCHK(hipEventRecord(c->ea0, s.q));
    if (overlap && lu->lane == 0 && c->run_n == 0) {
        // a run of overlapping steps begins: lane 1 starts behind what lane 0
        // holds so far, this step's set-up included
        HIPCHK(hipEventRecord(c->run_start, s.q));
        c->lane1_wait_start = true;
    }
    LCCHK(launch_register_tier(s, a0, dargs));
    if (p.async) return finish_async(s, st, enqueued);
    if (K > 0 && !p.t0_step) LCCHK(run_set_tiers(s));
    // One readback for the common case.  The T3 (HBM) tier is launched only
    // when T2 left keys for it (its workspace is sized from those counts),
    // after which the readback is repeated.
    LCCHK(p.t0_step ? read_t0_step(s) : readback(s));
    const int32_t *cnt = (const int32_t *)(c->hctl + 4);
    s.probes_pre_t3 = c->hctl[0];
    s.n_deep = cnt[2];
    s.n_widek = cnt[3];
    if (K > 0 && (s.n_deep > 0 || s.n_widek > 0)) LCCHK(run_hbm_tier(s));
    HIPCHK(hipEventElapsedTime(&s.ms, c->e0, c->e1));
    if (K > 0) HIPCHK(hipEventElapsedTime(&s.ms0, c->e0, c->et0));
    if (s.t3) HIPCHK(hipEventElapsedTime(&s.ms3, c->et3a, c->et3b));
    if (p.competition && K > 0) LCCHK(run_competition(s));
    if (st) fill_stats(s, st);
    return LC_OK;
}

// Wait for everything enqueued on c; *n_async / *span_ms: the asynchronous
// steps since the last wait and their HIP-event span.
int lcx::dev_wait(Dev *c, int *n_async, float *span_ms) {
    lc::Range range("lincheck: wait");
    HIPCHK(hipSetDevice(c->device));
    // lane 0 behind lane 1: the span's end below is the later lane's, and
    // the one synchronisation covers both
    LCCHK(join_lanes(c));
    if (c->ea1_pending) HIPCHK(hipEventRecord(c->ea1, c->stream));
    c->ea1_pending = false;
    HIPCHK(hipMemcpyAsync(c->hctl + 6, c->counters + 4, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    // every step's ring slot read and cleared behind them: one
    // synchronisation for the wait and both error reads
    const int re = take_ring_enqueue(c, 0xFu, c->stream);
    if (re) return re;
    HIPCHK(hipStreamSynchronize(c->stream));
    *n_async = (int)c->n_async;
    *span_ms = 0;
    if (c->n_async) HIPCHK(hipEventElapsedTime(span_ms, c->ea0, c->ea1));
    c->n_async = 0;
    const int rr = ring_taken(c, -1);
    const int rs = take_error(c);
    return rs ? rs : rr;
}

static void merge_stats(lc_stats &t, const lc_stats &s) {
    t.kernel_ms = std::max(t.kernel_ms, s.kernel_ms);
    t.tier0_ms = std::max(t.tier0_ms, s.tier0_ms);
    t.tier3_ms = std::max(t.tier3_ms, s.tier3_ms);
    t.probes += s.probes;
    t.probes_t3 += s.probes_t3;
    t.t3_bytes += s.t3_bytes;
    t.lds_keys += s.lds_keys;
    t.deep_keys += s.deep_keys;
    t.events += s.events;
    t.t0_path = std::max(t.t0_path, s.t0_path);
    t.ev_word_bytes = std::max(t.ev_word_bytes, s.ev_word_bytes);
    t.wgl_ms = std::max(t.wgl_ms, s.wgl_ms);
    t.wgl_keys += s.wgl_keys;
    t.wgl_spilled += s.wgl_spilled;
    t.wgl_steps += s.wgl_steps;
}

// Run fn(g) for every device g of c at once (one driver thread per device
// beyond the first); returns the first nonzero code.
static int each_device(lc_ctx *c, const std::function<int(int)> &fn) {
    if (c->n_dev == 1) return fn(0);
    std::vector<int> rc((size_t)c->n_dev, 0);
    std::vector<std::string> err((size_t)c->n_dev);
    c->drivers->run((unsigned)c->n_dev, [&](unsigned g) {
        rc[g] = fn((int)g);
        if (rc[g]) err[g] = lc_last_error();
    });
    for (int g = 0; g < c->n_dev; ++g)
        if (rc[g]) return lc::fail(rc[g], "%s", err[g].c_str());
    return LC_OK;
}

// Validate b (events too unless T0 will) and, when its event words are not
// page-locked, copy them into the context's pinned staging buffer.  *src:
// where the uploads read the events from (b->events or the staging copy).
int lcx::prepare_batch(lc_ctx *c, const lc_batch *b, Shape *sh, const uint32_t **src) {
    lc::Range range("lincheck: prepare");
    int rc = validate_batch(b);
    if (rc) return rc;
    *sh = batch_shape(b);
    *src = b->events;
    const int64_t K = b->n_keys;
    if (!K) return LC_OK;
    const size_t n_ev = (size_t)b->ev_off[K];
    // Batches above 256 MB of events keep the pageable path (no pinned
    // allocation that large); page-locked caller memory is used as it is.
    // A batch given only as 16-bit words is widened here when its upload
    // needs the 32-bit ones (keys beyond the register tier, or the A/B flag
    // LC_PATH_EV32); a register-tier batch uploads the 16-bit words.
    const bool up16 = b->events16 && sh->t0_only && !(c->o.path_flags & LC_PATH_EV32);
    const bool widen = n_ev > 0 && !b->events && !up16;
    const bool stage = widen || (n_ev > 0 && b->events && n_ev <= (256u << 20) / 4 && !pinned(b->events) &&
                                 !(up16 && pinned(b->events16)));
    if (stage) HIPCHK(grow_pinned(c->hstage, c->hstage_cap, n_ev));
    // The device validates every event of a batch (k_validate beside the
    // first tier; the later tiers do nothing over a refused batch), so the
    // host walks the events only to stage pageable ones -- and to check a
    // table model, whose rows are checked against the key's states here.
    sh->host_checked = b->table != nullptr;
    if (!stage && !sh->host_checked) return LC_OK;  // nothing to copy, the device validates
    if (K >= 256 && !c->pool)
        c->pool = new HostPool(std::max(1u, std::min(16u, std::thread::hardware_concurrency())) - 1);
    int64_t bk = -1;
    if (int why = validate_events(b, &bk, stage ? c->hstage : nullptr, K >= 256 ? c->pool : nullptr, sh->host_checked))
        return events_error(why, bk);
    if (stage) *src = c->hstage;
    return LC_OK;
}

// The part of r that holds the keys from k0 on: one device's share of a
// result a context of several devices fills.
static lc_result slice_result(const lc_result &r, int64_t k0, int max_final) {
    lc_result s = r;
    s.valid = r.valid + k0;
    s.fail_event = r.fail_event + k0;
    s.cause = r.cause + k0;
    if (r.peak_configs) s.peak_configs = r.peak_configs + k0;
    if (r.final_configs) s.final_configs = r.final_configs + (size_t)k0 * max_final * 2;
    if (r.n_final) s.n_final = r.n_final + k0;
    if (r.analyzer) s.analyzer = r.analyzer + k0;
    return s;
}

// ---- C ABI ------------------------------------------------------------------

extern "C" int lc_upload(lc_ctx *c, const lc_batch *b, lc_dev_batch **out) {
    if (!c || !b || !out) return lc::fail(LC_E_INVALID, "lc_upload: null argument");
    std::lock_guard<std::mutex> g(c->mu);
    Shape sh;
    const uint32_t *src = nullptr;
    int rc = prepare_batch(c, b, &sh, &src);
    if (rc) return rc;
    lc_dev_batch *d = new (std::nothrow) lc_dev_batch();
    if (!d) return lc::fail(LC_E_NOMEM, "lc_upload: out of memory");
    d->n_parts = c->n_dev;
    d->n_keys = b->n_keys;
    shard_keys(b, c->n_dev, d->key0);
    for (int p = 0; p < c->n_dev; ++p) {
        d->part[p] = new (std::nothrow) DevBatch();
        if (!d->part[p]) { delete d; return lc::fail(LC_E_NOMEM, "lc_upload: out of memory"); }
        d->part[p]->device = c->dev[p]->device;
    }
    rc = each_device(c, [&](int p) {
        std::vector<uint64_t> off;
        const lc_batch s = c->n_dev > 1 ? sub_batch(b, d->key0[p], d->key0[p + 1], off) : *b;
        const uint32_t *es = src ? src + (b->n_keys ? b->ev_off[d->key0[p]] : 0) : nullptr;
        return upload_into(c->dev[p], &s, d->part[p], sh, sh.host_checked, es);
    });
    if (rc) { delete d; return rc; }
    *out = d;
    return LC_OK;
}

extern "C" void lc_dev_batch_free(lc_dev_batch *d) { delete d; }

extern "C" int lc_check_device(lc_ctx *c, const lc_dev_batch *d, lc_result *r, int flags, lc_stats *st) {
    if (flags & ~(LC_DEV_RESULT | LC_DEV_ASYNC)) return lc::fail(LC_E_INVALID, "lc_check_device: unknown flags 0x%x", flags);
    const bool dev_result = (flags & LC_DEV_RESULT) != 0;
    if (!c || !d || !r || !r->valid || !r->fail_event || !r->cause)
        return lc::fail(LC_E_INVALID, "lc_check_device: null argument");
    if (d->n_parts != c->n_dev) return lc::fail(LC_E_INVALID, "lc_check_device: batch uploaded by another context shape");
    for (int p = 0; p < d->n_parts; ++p)
        if (d->part[p]->device != c->dev[p]->device)
            return lc::fail(LC_E_INVALID, "lc_check_device: batch lives on another device");
    if (dev_result && c->n_dev > 1)
        return lc::fail(LC_E_INVALID, "lc_check_device: LC_DEV_RESULT needs a one-device context");
    std::lock_guard<std::mutex> g(c->mu);
    if (c->n_dev == 1)
        return dev_search(c->dev[0], d->part[0], r, dev_result ? RES_DEV : RES_HOST, (flags & LC_DEV_ASYNC) != 0, 0, st);
    auto t0 = std::chrono::steady_clock::now();
    std::vector<lc_stats> ps((size_t)c->n_dev);
    int rc = each_device(c, [&](int p) {
        const lc_result rp = slice_result(*r, d->key0[p], c->o.max_final);
        return dev_search(c->dev[p], d->part[p], &rp, RES_HOST, false, d->key0[p], &ps[(size_t)p]);
    });
    if (rc) return rc;
    if (st) {
        *st = lc_stats{};
        for (const lc_stats &s : ps) merge_stats(*st, s);
        st->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return LC_OK;
}

extern "C" int lc_wait(lc_ctx *c, lc_stats *st) {
    if (!c) return lc::fail(LC_E_INVALID, "lc_wait: null context");
    lc::Range range("lc_wait");
    std::lock_guard<std::mutex> g(c->mu);
    int n = 0;
    float ms = 0;
    int rc = LC_OK;
    for (int p = 0; p < c->n_dev; ++p) {
        int np = 0;
        float mp = 0;
        int r = dev_wait(c->dev[p], &np, &mp);
        if (r && !rc) rc = r;
        n = std::max(n, np);
        ms = std::max(ms, mp);
    }
    if (rc) return rc;
    if (st) {
        *st = lc_stats{};
        st->kernel_ms = ms;                    // first enqueued step's start .. last one's end
        st->tier0_ms = n ? ms / (float)n : 0;  // per step, gaps between launches included
    }
    return n;
}

extern "C" int lc_wait_step(lc_ctx *c, int back) {
    if (!c) return lc::fail(LC_E_INVALID, "lc_wait_step: null context");
    std::lock_guard<std::mutex> g(c->mu);
    int rc = LC_OK;
    for (int p = 0; p < c->n_dev; ++p) {
        Dev *d = c->dev[p];
        HIPCHK(hipSetDevice(d->device));
        int r;
        if (back < 0 || back >= 4 || (uint64_t)back >= d->async_seq) {
            LCCHK(drain_lanes(d));  // no such step on record: everything
            r = take_ring(d, 0xFu, -1, d->stream);
        } else {
            // Errors of the finished step surface here (include/lincheck.h):
            // its own error words, read and cleared atomically on a stream of
            // their own, so the later steps still running keep theirs (one 4
            // steps later shares the slot: an error it has raised already is
            // reported now too)
            const int q = (int)((d->async_seq - 1 - (uint64_t)back) % 4);
            HIPCHK(hipEventSynchronize(d->ring[q]));
            r = take_ring(d, 1u << q, q, d->estream);
        }
        if (r && !rc) rc = r;
    }
    return rc;
}

extern "C" int lc_check_batch(lc_ctx *c, const lc_batch *b, lc_result *r, lc_stats *st) {
    lc::Range range("lc_check_batch");
    auto t0 = std::chrono::steady_clock::now();
    if (!c || !b || !r || !r->valid || !r->fail_event || !r->cause)
        return lc::fail(LC_E_INVALID, "lc_check_batch: null argument");
    std::lock_guard<std::mutex> g(c->mu);
    Shape sh;
    const uint32_t *src = nullptr;
    int rc = prepare_batch(c, b, &sh, &src);
    if (rc) return rc;
    const auto t_val = std::chrono::steady_clock::now();
    int64_t key0[MAX_DEV + 1];
    shard_keys(b, c->n_dev, key0);
    std::vector<lc_stats> ps((size_t)c->n_dev);
    rc = each_device(c, [&](int p) {
        Dev *d = c->dev[p];
        if (int e = staging_batch(d->staged, "lc_check_batch")) return e;
        std::vector<uint64_t> off;
        const lc_batch s = c->n_dev > 1 ? sub_batch(b, key0[p], key0[p + 1], off) : *b;
        const uint32_t *es = src ? src + (b->n_keys ? b->ev_off[key0[p]] : 0) : nullptr;
        int e = upload_into(d, &s, d->staged, sh, sh.host_checked, es);
        if (e) return e;
        const lc_result rp = slice_result(*r, key0[p], c->o.max_final);
        return dev_search(d, d->staged, &rp, RES_HOST, false, key0[p], &ps[(size_t)p]);
    });
    if (std::getenv("LC_TIMING")) {
        using ms = std::chrono::duration<double, std::milli>;
        std::fprintf(stderr, "lc_check_batch: validate/stage %.3f ms, upload + check %.3f ms\n",
                     ms(t_val - t0).count(), ms(std::chrono::steady_clock::now() - t_val).count());
    }
    if (rc) return rc;
    if (st) {
        *st = lc_stats{};
        for (const lc_stats &s : ps) merge_stats(*st, s);
        st->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return LC_OK;
}

// What dev_search will plan for a node step whose results stay in the
// context (plan_lane decides from it before the search is enqueued).
lc::StepPlan lcx::node_step_plan(Dev *c, const DevBatch *d) {
    const Step s{c, d, nullptr, RES_CTX, d->n_keys, {}};
    return lc::plan_step(step_in(s, true));
}

extern "C" void *lc_host_alloc(size_t bytes) {
    void *p = nullptr;
    if (hipHostMalloc(&p, std::max<size_t>(bytes, 1), hipHostMallocDefault) != hipSuccess) {
        lc::set_error("lc_host_alloc: page-locked allocation failed");
        return nullptr;
    }
    return p;
}

extern "C" void lc_host_free(void *p) {
    if (p) (void)hipHostFree(p);
}

// ---- the set workload (set.clj:46; device_set.hip) ---------------------------

extern "C" int lc_set_check(lc_ctx *c, const lc_set_batch *b, lc_set_result *r) {
    if (!c || !b || !r) return lc::fail(LC_E_INVALID, "lc_set_check: null argument");
    CtxCall x(c);
    LCCHK(x.enter());
    return lcs::set_check(&x.d->setdev, x.d->stream, c->o.path_flags, b, r);
}

extern "C" int lc_set_last_timing(lc_ctx *c, double *out_ms) {
    if (!c || !out_ms) return lc::fail(LC_E_INVALID, "lc_set_last_timing: null argument");
    std::lock_guard<std::mutex> g(c->mu);
    return lcs::set_last_timing(c->dev[0]->setdev, out_ms);
}

// ---- checker/set-full (device_setfull.hip) -----------------------------------

extern "C" int lc_setfull_check(lc_ctx *c, const lc_setfull_batch *b, const lc_setfull_opts *o, lc_setfull_result *r) {
    if (!c || !b || !o || !r) return lc::fail(LC_E_INVALID, "lc_setfull_check: null argument");
    CtxCall x(c);
    LCCHK(x.enter());
    return lcf::setfull_check(&x.d->setfulldev, x.d->stream, b, o, r);
}

extern "C" int lc_setfull_last_timing(lc_ctx *c, double *out8) {
    if (!c || !out8) return lc::fail(LC_E_INVALID, "lc_setfull_last_timing: null argument");
    std::lock_guard<std::mutex> g(c->mu);
    return lcf::setfull_last_timing(c->dev[0]->setfulldev, out8);
}

// ---- checker/counter (include/lincheck_counter.h; kernels: device_counter.hip) ----

namespace {

// Sections of a block, each 16-byte aligned.
struct CtLayout {
    size_t at = 0;
    size_t take(size_t bytes) {
        const size_t o = at;
        at += (bytes + 15) & ~(size_t)15;
        return o;
    }
};

int counter_check(CounterDev &D, hipStream_t stream, const lc_counter_batch *b, uint32_t tile, lc_counter_result *r) {
    const auto wall0 = std::chrono::steady_clock::now();
    const int64_t K = b->n_keys;
    const size_t nk = (size_t)K;
    const uint64_t E = b->ev_off[K], R = b->read_off[K];
    const uint64_t te = lcc::ct_tiles(E, tile), tr = lcc::ct_tiles(R, tile), tmax = std::max(te, tr);
    if (tmax > lcc::CT_MAX_TILES) return lc::fail(LC_E_INVALID, "lc_counter_check: more than 2^31 tiles");
    for (hipEvent_t &e : D.ev)
        if (!e) HIPCHK(hipEventCreate(&e));
    std::vector<uint32_t> first_ev, first_rd;
    try {
        if (E) first_ev = lcc::ct_first_key(b->ev_off, K, E, tile);
        if (R) first_rd = lcc::ct_first_key(b->read_off, K, R, tile);
    } catch (const std::bad_alloc &) {
        return lc::fail(LC_E_NOMEM, "lc_counter_check: out of memory");
    }
    // one metadata block, one copy
    CtLayout L;
    const size_t o_ev_off = L.take((nk + 1) * 8), o_rd_off = L.take((nk + 1) * 8);
    const size_t o_first_ev = L.take(first_ev.size() * 4), o_first_rd = L.take(first_rd.size() * 4);
    HIPCHK(grow_pinned(D.hmeta, D.hmeta_cap, L.at));
    HIPCHK(grow_pinned(D.hout, D.hout_cap, (size_t)2));
    std::memcpy(D.hmeta + o_ev_off, b->ev_off, (nk + 1) * 8);
    std::memcpy(D.hmeta + o_rd_off, b->read_off, (nk + 1) * 8);
    if (E) std::memcpy(D.hmeta + o_first_ev, first_ev.data(), first_ev.size() * 4);
    if (R) std::memcpy(D.hmeta + o_first_rd, first_rd.data(), first_rd.size() * 4);
    CtLayout T;  // the tile records and carries, shared by the two scans
    const size_t o_sa = T.take(tmax * 8), o_sb = T.take(tmax * 8), o_ca = T.take(tmax * 8), o_cb = T.take(tmax * 8);
    const size_t o_hd = T.take(tmax);
    char *meta, *tiles;
    uint8_t *kind;
    int64_t *val, *rval, *lower, *upper;
    unsigned long long *err_off, *err_idx, *out;
    HIPCHK(grow(D.mem[CounterDev::META], meta, L.at));
    HIPCHK(grow(D.mem[CounterDev::KIND], kind, (size_t)E));
    HIPCHK(grow(D.mem[CounterDev::VAL], val, (size_t)E));
    HIPCHK(grow(D.mem[CounterDev::RVAL], rval, (size_t)R));
    HIPCHK(grow(D.mem[CounterDev::LOWER], lower, (size_t)R));
    HIPCHK(grow(D.mem[CounterDev::UPPER], upper, (size_t)R));
    HIPCHK(grow(D.mem[CounterDev::TILES], tiles, T.at));
    HIPCHK(grow(D.mem[CounterDev::ERR_OFF], err_off, nk + 1));
    HIPCHK(grow(D.mem[CounterDev::ERR_IDX], err_idx, (size_t)std::min<uint64_t>(r->err_cap, R)));
    HIPCHK(grow(D.mem[CounterDev::OUT], out, (size_t)2));
    const uint64_t cap = std::min<uint64_t>(r->err_cap, R);  // (no more reads than R can be flagged)

    HIPCHK(hipEventRecord(D.ev[0], stream));
    HIPCHK(hipMemcpyAsync(meta, D.hmeta, L.at, hipMemcpyHostToDevice, stream));
    if (E) {
        HIPCHK(hipMemcpyAsync(kind, b->ev_kind, E, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(val, b->ev_val, E * 8, hipMemcpyHostToDevice, stream));
    }
    if (R) HIPCHK(hipMemcpyAsync(rval, b->read_val, R * 8, hipMemcpyHostToDevice, stream));
    HIPCHK(hipEventRecord(D.ev[1], stream));
    HIPCHK(hipMemsetAsync(out, 0, 16, stream));
    HIPCHK(hipMemsetAsync(err_off, 0, (nk + 1) * 8, stream));
    if (R) {
        HIPCHK(hipMemsetAsync(lower, 0, R * 8, stream));
        HIPCHK(hipMemsetAsync(upper, 0, R * 8, stream));
    }
    lcc::CtTiles ct{(unsigned long long *)(tiles + o_sa), (unsigned long long *)(tiles + o_sb),
                    (unsigned long long *)(tiles + o_ca), (unsigned long long *)(tiles + o_cb), (uint8_t *)(tiles + o_hd)};
    if (E) {
        lcc::CtEvents a{};
        a.s = lcc::CtSeries{(const uint64_t *)(meta + o_ev_off), (const uint32_t *)(meta + o_first_ev), K, E, te};
        a.t = ct;
        a.kind = kind; a.val = val; a.lower = lower; a.upper = upper; a.R = R;
        a.err = (uint32_t *)(out + 1);
        HIPCHK(lcc::counter_launch_events(stream, tile, a));
    }
    if (R) {
        lcc::CtJudge a{};
        a.s = lcc::CtSeries{(const uint64_t *)(meta + o_rd_off), (const uint32_t *)(meta + o_first_rd), K, R, tr};
        a.t = ct;
        a.val = rval; a.lower = lower; a.upper = upper;
        a.err_off = err_off; a.err_idx = err_idx; a.err_cap = cap; a.n_err = out;
        HIPCHK(lcc::counter_launch_judge(stream, tile, a));
    }
    HIPCHK(hipEventRecord(D.ev[2], stream));
    HIPCHK(hipMemcpyAsync(D.hout, out, 16, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(r->err_off, err_off, (nk + 1) * 8, hipMemcpyDeviceToHost, stream));
    if (R) {
        HIPCHK(hipMemcpyAsync(r->lower, lower, R * 8, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipMemcpyAsync(r->upper, upper, R * 8, hipMemcpyDeviceToHost, stream));
    }
    HIPCHK(hipStreamSynchronize(stream));
    if ((uint32_t)D.hout[1]) return lc::fail(LC_E_INVALID, "lc_counter_check: a bad event kind, or a read event that names no read of the batch");
    const uint64_t n_err = D.hout[0];
    r->n_err = n_err;
    for (int64_t k = 0; k < K; ++k) {
        r->n_errors[k] = r->err_off[k + 1] - r->err_off[k];
        r->valid[k] = b->status && b->status[k] != LC_COUNTER_KEY_OK ? LC_UNKNOWN : r->n_errors[k] ? LC_INVALID : LC_VALID;
    }
    if (n_err && n_err <= r->err_cap) HIPCHK(hipMemcpyAsync(r->err_idx, err_idx, n_err * 8, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipEventRecord(D.ev[3], stream));
    HIPCHK(hipStreamSynchronize(stream));
    float f = 0;
    for (int i = 0; i < 3; ++i) {
        HIPCHK(hipEventElapsedTime(&f, D.ev[i], D.ev[i + 1]));
        D.ms[i] = f;
    }
    D.ms[3] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    if (n_err > r->err_cap)
        return lc::fail(LC_E_NOMEM, "lc_counter_check: err_cap %llu, %llu needed", (unsigned long long)r->err_cap,
                        (unsigned long long)n_err);
    return LC_OK;
}

}  // namespace

extern "C" int lc_counter_check(lc_ctx *c, const lc_counter_batch *b, const lc_counter_opts *o, lc_counter_result *r) {
    if (!c || !b || !o || !r) return lc::fail(LC_E_INVALID, "lc_counter_check: null argument");
    lc::Range range("lc_counter_check");
    LCCHK(lcc::counter_validate(b, "lc_counter_check"));
    if (o->flags) return lc::fail(LC_E_INVALID, "lc_counter_check: unknown flags 0x%x", o->flags);
    const uint32_t tile = lcc::ct_tile_of(o->tile);
    if (!tile) return lc::fail(LC_E_INVALID, "lc_counter_check: tile %u (256 or 2048)", o->tile);
    r->n_err = 0;
    if (b->n_keys == 0) return LC_OK;
    const uint64_t R = b->read_off[b->n_keys];
    if (!r->valid || !r->n_errors || !r->err_off || (R && (!r->lower || !r->upper)) || (r->err_cap && !r->err_idx))
        return lc::fail(LC_E_INVALID, "lc_counter_check: null result array");
    CtxCall x(c);
    LCCHK(x.enter());
    if (!x.d->counterdev) x.d->counterdev = new (std::nothrow) CounterDev();
    if (!x.d->counterdev) return lc::fail(LC_E_NOMEM, "lc_counter_check: out of memory");
    return counter_check(*x.d->counterdev, x.d->stream, b, tile, r);
}

extern "C" int lc_counter_last_timing(lc_ctx *c, double *out4) {
    if (!c || !out4) return lc::fail(LC_E_INVALID, "lc_counter_last_timing: null argument");
    std::lock_guard<std::mutex> g(c->mu);
    const CounterDev *d = c->dev[0]->counterdev;
    for (int i = 0; i < 4; ++i) out4[i] = d ? d->ms[i] : 0.0;
    return LC_OK;
}

// ---- checker/total-queue and /unique-ids (include/lincheck_queue.h; kernels: device_queue.hip) ----

namespace {

int queue_check(QueueDev &D, hipStream_t stream, const lc_queue_batch *b, uint64_t slots, lc_queue_result *r) {
    const auto wall0 = std::chrono::steady_clock::now();
    const size_t nk = (size_t)b->n_keys, n = (size_t)b->n_rows;
    for (hipEvent_t &e : D.ev)
        if (!e) HIPCHK(hipEventCreate(&e));
    // the per-key words as one block: counts, lo, hi
    const size_t o_lo = nk * LC_QN_COUNTS * 8, o_hi = o_lo + nk * 8, keyst_bytes = o_hi + nk * 8;
    const uint64_t cap = std::min<uint64_t>(r->ent_cap, 2 * (uint64_t)n);  // (a distinct value makes at most two entries)
    HIPCHK(grow_pinned(D.hkeyst, D.hkeyst_cap, keyst_bytes));
    HIPCHK(grow_pinned(D.hout, D.hout_cap, (size_t)lcq::QO_WORDS));
    lcq::QueueArgs a{};
    uint32_t *row_key;
    uint8_t *row_kind, *status;
    int64_t *row_val;
    char *keyst;
    HIPCHK(grow(D.mem[QueueDev::ROW_KEY], row_key, n));
    HIPCHK(grow(D.mem[QueueDev::ROW_KIND], row_kind, n));
    HIPCHK(grow(D.mem[QueueDev::ROW_VAL], row_val, n));
    HIPCHK(grow(D.mem[QueueDev::STATUS], status, nk));
    HIPCHK(grow(D.mem[QueueDev::TABLE], a.table, (size_t)slots));
    HIPCHK(grow(D.mem[QueueDev::KEYST], keyst, keyst_bytes));
    HIPCHK(grow(D.mem[QueueDev::ENT_KEY], a.ent_key, (size_t)cap));
    HIPCHK(grow(D.mem[QueueDev::ENT_CLASS], a.ent_class, (size_t)cap));
    HIPCHK(grow(D.mem[QueueDev::ENT_VAL], a.ent_val, (size_t)cap));
    HIPCHK(grow(D.mem[QueueDev::ENT_MULT], a.ent_mult, (size_t)cap));
    HIPCHK(grow(D.mem[QueueDev::OUT], a.out, (size_t)lcq::QO_WORDS));
    a.row_key = row_key; a.row_kind = row_kind; a.row_val = row_val; a.status = status;
    a.n_rows = n; a.K = (uint32_t)nk; a.mode = b->mode; a.slots = (uint32_t)slots;
    a.counts = (unsigned long long *)keyst;
    a.lo = (long long *)(keyst + o_lo);
    a.hi = (long long *)(keyst + o_hi);
    a.ent_cap = cap;
    // status is staged in the landing of the per-key words, which the stream fills only after this copy
    if (b->status) std::memcpy(D.hkeyst, b->status, nk);
    else std::memset(D.hkeyst, LC_QUEUE_KEY_OK, nk);

    HIPCHK(hipEventRecord(D.ev[0], stream));
    HIPCHK(hipMemcpyAsync(status, D.hkeyst, nk, hipMemcpyHostToDevice, stream));
    if (n) {
        HIPCHK(hipMemcpyAsync(row_key, b->row_key, n * 4, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(row_kind, b->row_kind, n, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(row_val, b->row_val, n * 8, hipMemcpyHostToDevice, stream));
    }
    HIPCHK(hipEventRecord(D.ev[1], stream));
    HIPCHK(lcq::queue_launch(stream, a));
    HIPCHK(hipEventRecord(D.ev[2], stream));
    HIPCHK(hipMemcpyAsync(D.hout, a.out, lcq::QO_WORDS * 8, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(D.hkeyst, keyst, keyst_bytes, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    if (D.hout[lcq::QO_ERR] & lcq::QE_BAD_ROW)
        return lc::fail(LC_E_INVALID, "lc_queue_check: a row_key that is not below n_keys, or a row_kind the mode has not");
    if (D.hout[lcq::QO_ERR])
        return lc::fail(LC_E_INVALID, "lc_queue_check: a row found no slot in a table of %llu", (unsigned long long)slots);
    std::memcpy(r->counts, D.hkeyst, o_lo);
    lcq::queue_finish(b, r);
    for (size_t k = 0; k < nk; ++k)
        if (r->has_range[k]) {
            std::memcpy(&r->lo[k], D.hkeyst + o_lo + k * 8, 8);
            std::memcpy(&r->hi[k], D.hkeyst + o_hi + k * 8, 8);
        }
    const uint64_t n_ent = D.hout[lcq::QO_N_ENT];
    r->n_ent = n_ent;
    const bool fits = n_ent <= r->ent_cap;
    size_t o_cls = 0, o_val = 0, o_mult = 0;
    if (n_ent && fits) {
        const size_t ne = (size_t)n_ent;  // (n_ent <= 2 n: ne <= cap)
        o_val = (ne * 4 + 15) & ~(size_t)15; o_mult = o_val + ne * 8; o_cls = o_mult + ne * 8;
        HIPCHK(grow_pinned(D.hent, D.hent_cap, o_cls + ne));
        HIPCHK(hipMemcpyAsync(D.hent, a.ent_key, ne * 4, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipMemcpyAsync(D.hent + o_val, a.ent_val, ne * 8, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipMemcpyAsync(D.hent + o_mult, a.ent_mult, ne * 8, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipMemcpyAsync(D.hent + o_cls, a.ent_class, ne, hipMemcpyDeviceToHost, stream));
    }
    HIPCHK(hipEventRecord(D.ev[3], stream));
    HIPCHK(hipStreamSynchronize(stream));
    if (n_ent && fits) {
        try {
            // the device's order is unspecified: the call returns the entries sorted
            lcq::queue_sort_entries(r, n_ent, (const uint32_t *)D.hent, (const uint8_t *)(D.hent + o_cls),
                                    (const int64_t *)(D.hent + o_val), (const unsigned long long *)(D.hent + o_mult));
        } catch (const std::bad_alloc &) {
            return lc::fail(LC_E_NOMEM, "lc_queue_check: out of memory");
        }
    }
    float f = 0;
    for (int i = 0; i < 3; ++i) {
        HIPCHK(hipEventElapsedTime(&f, D.ev[i], D.ev[i + 1]));
        D.ms[i] = f;
    }
    D.ms[3] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    if (!fits)
        return lc::fail(LC_E_NOMEM, "lc_queue_check: ent_cap %llu, %llu needed", (unsigned long long)r->ent_cap,
                        (unsigned long long)n_ent);
    return LC_OK;
}

}  // namespace

extern "C" int lc_queue_check(lc_ctx *c, const lc_queue_batch *b, const lc_queue_opts *o, lc_queue_result *r) {
    if (!c || !b || !o || !r) return lc::fail(LC_E_INVALID, "lc_queue_check: null argument");
    lc::Range range("lc_queue_check");
    LCCHK(lcq::queue_validate(b, r, "lc_queue_check"));
    if (o->flags) return lc::fail(LC_E_INVALID, "lc_queue_check: unknown flags 0x%x", o->flags);
    const uint64_t slots = lcq::qp_slots_of(o->slots, (uint64_t)b->n_rows);
    if (slots == lcq::QP_BAD_SLOTS)
        return lc::fail(LC_E_INVALID, "lc_queue_check: slots %u (a power of two, at least the %lld rows)", o->slots, (long long)b->n_rows);
    if (!lcq::qp_fits(slots))
        return lc::fail(LC_E_NOMEM, "lc_queue_check: a table of %llu slots needs %llu bytes, the cap is %llu", (unsigned long long)slots,
                        (unsigned long long)lcq::qp_bytes(slots), (unsigned long long)lcq::QP_MAX_BYTES);
    r->n_ent = 0;
    if (b->n_keys == 0) {
        if (b->n_rows) return lc::fail(LC_E_INVALID, "lc_queue_check: rows without a key");
        return LC_OK;
    }
    CtxCall x(c);
    LCCHK(x.enter());
    if (!x.d->queuedev) x.d->queuedev = new (std::nothrow) QueueDev();
    if (!x.d->queuedev) return lc::fail(LC_E_NOMEM, "lc_queue_check: out of memory");
    return queue_check(*x.d->queuedev, x.d->stream, b, slots, r);
}

extern "C" int lc_queue_last_timing(lc_ctx *c, double *out4) {
    if (!c || !out4) return lc::fail(LC_E_INVALID, "lc_queue_last_timing: null argument");
    std::lock_guard<std::mutex> g(c->mu);
    const QueueDev *d = c->dev[0]->queuedev;
    for (int i = 0; i < 4; ++i) out4[i] = d ? d->ms[i] : 0.0;
    return LC_OK;
}

// ---- checker/perf (etcdemo.clj:165-167; device_perf.hip) ----------------------

extern "C" int lc_perf_check(lc_ctx *c, const lc_perf_batch *b, const lc_perf_opts *o, lc_perf_result *r) {
    if (!c || !b || !o || !r) return lc::fail(LC_E_INVALID, "lc_perf_check: null argument");
    CtxCall x(c);
    LCCHK(x.enter());
    return lcp::perf_check(&x.d->perfdev, x.d->stream, b, o, r);
}

extern "C" int lc_perf_last_timing(lc_ctx *c, double *out_ms) {
    if (!c || !out_ms) return lc::fail(LC_E_INVALID, "lc_perf_last_timing: null argument");
    std::lock_guard<std::mutex> g(c->mu);
    return lcp::perf_last_timing(c->dev[0]->perfdev, out_ms);
}
