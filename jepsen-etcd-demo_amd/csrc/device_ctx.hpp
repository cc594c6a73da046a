// device_ctx.hpp -- the context as device_api.hip, device_node.hip and device_stream.hip share it: the error
// macros, the allocation helpers, a context's devices, lanes and batches, and the functions of
// device_api.hip that the node steps and the stream call.  Internal: no other file includes it.
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "common.hpp"
#include "device_search.hpp"
#include "device_perf.hpp"
#include "device_set.hpp"
#include "device_setfull.hpp"
#include "device_counter.hpp"
#include "device_queue.hpp"
#include "step_plan.hpp"
#include "lane_plan.hpp"

#define HIPCHK(expr)                                                                       \
    do {                                                                                   \
        hipError_t _e = (expr);                                                            \
        if (_e != hipSuccess)                                                              \
            return lc::fail(LC_E_DEVICE, "%s failed: %s", #expr, hipGetErrorString(_e));  \
    } while (0)

// a step of ours that failed: its code goes up as it is (lc::fail has the message)
#define LCCHK(expr)            \
    do {                       \
        int _rc = (expr);      \
        if (_rc) return _rc;   \
    } while (0)

#define RCCLCHK(expr)                                                                     \
    do {                                                                                   \
        ncclResult_t _r = (expr);                                                          \
        if (_r != ncclSuccess)                                                             \
            return lc::fail(LC_E_DEVICE, "%s failed: %s", #expr, R->error(_r));            \
    } while (0)

namespace lcx {

constexpr int MAX_DEV = LC_MAX_DEVICES;

template <class T>
hipError_t dalloc(T **p, size_t n) {
    *p = nullptr;
    if (n == 0) n = 1;
    return hipMalloc((void **)p, n * sizeof(T));
}

template <class T>
void dfree(T *&p) {
    if (p) (void)hipFree(p);
    p = nullptr;
}

// RCCL, loaded on first use from the directory of the HIP runtime this
// library is bound to (a process may hold two: torch bundles its own), so
// the communicator and our streams belong to one runtime.
struct Rccl {
    void *h = nullptr;
    decltype(&ncclGetUniqueId) get_unique_id = nullptr;
    decltype(&ncclCommInitRank) comm_init_rank = nullptr;
    decltype(&ncclCommDestroy) comm_destroy = nullptr;
    decltype(&ncclAllGather) all_gather = nullptr;
    decltype(&ncclGetErrorString) error_string = nullptr;
    const char *error(ncclResult_t r) const { return error_string ? error_string(r) : "rccl error"; }
};
const Rccl *rccl();

// One device's part of a batch in HBM.
struct DevBatch {
    int device = 0;
    int64_t n_keys = 0;
    uint64_t n_events = 0;
    int64_t n_trans = 0;
    uint32_t init_state = 0;
    uint32_t shared_states = 0;  // 1 + largest state id in a shared table
    bool has_trans_off = false;
    uint64_t *ev_off = nullptr;
    uint32_t *events = nullptr;
    uint32_t *trans = nullptr;
    uint32_t *trans_off = nullptr;
    uint8_t *key_width = nullptr;
    uint16_t *key_states = nullptr;
    uint8_t *key_error = nullptr;
    uint16_t *table = nullptr; // a table model's rows (lc_batch.table), or null
    int64_t n_table = 0;
    int32_t *order = nullptr;  // LPT: keys by event count, descending
    bool t0_only = false;      // every key declared to fit the register lattice
    bool taggable = false;     // keys may be cut into segments (shared table, states 0..5, no op installs nil)
    bool seg_pays = false;     // sampled keys have quiescent points close enough for segments to pay
    bool validated = false;    // the host checked every event (else the device does: T0_STRICT or k_validate<true>)
    int64_t narrow_keys = 0;   // keys with at most 24 window slots (key_width): the WGL walk's LDS cache tier
    // Device storage behind the arrays above, grown on demand: a batch that is
    // re-uploaded (a context's staging batch for lc_check_batch) keeps it, so
    // a host-to-host check allocates nothing once its sizes have been seen.
    struct Mem {
        void *p = nullptr;
        size_t cap = 0;
    } mem[8];
    // pinned host staging of the per-key arrays and the transition table
    // (one copy per upload); `hmeta_done` marks the end of the last copy out
    // of it, so it is not rewritten while that copy may still read it
    char *hmeta = nullptr;
    size_t hmeta_cap = 0;
    hipEvent_t hmeta_done = nullptr;
    uint16_t *events16 = nullptr;    // 16-bit event words (mem[3]), or null: a register-tier batch
                                     // uploaded at 2 bytes per event (lc_batch.events16)
    mutable bool ev32_ready = true;  // `events` holds the 32-bit words (else widened, once, by the
                                     // first step whose kernels read them: all but k_spec)
    // the LPT order of the last upload and the offsets it was computed from
    // (a batch re-uploaded with the same offsets reuses it)
    std::vector<uint64_t> order_off;
    std::vector<int32_t> order_of;
    ~DevBatch() {
        if (hmeta_done) (void)hipEventSynchronize(hmeta_done);
        for (Mem &m : mem)
            if (m.p) (void)hipFree(m.p);
        if (hmeta) (void)hipHostFree(hmeta);
        if (hmeta_done) (void)hipEventDestroy(hmeta_done);
    }
};

// Point p at m's storage, growing it to hold n elements of T.
template <class T>
hipError_t grow(DevBatch::Mem &m, T *&p, size_t n) {
    const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
    if (bytes > m.cap) {
        if (m.p) (void)hipFree(m.p);
        m.p = nullptr;
        m.cap = 0;
        p = nullptr;
        hipError_t e = hipMalloc(&m.p, bytes);
        if (e != hipSuccess) return e;
        m.cap = bytes;
    }
    p = (T *)m.p;
    return hipSuccess;
}

// lc_counter_check's state on a device (device_api.hip; the kernels are
// device_counter.hip's): cached device arrays, pinned staging and timing
// events, grown on demand and kept from one call to the next.
struct CounterDev {
    // meta: both offset arrays and both first-key arrays (one copy); tiles: the
    // tile records and carries; out: the error count and the error word
    enum { META, KIND, VAL, RVAL, LOWER, UPPER, TILES, ERR_OFF, ERR_IDX, OUT, N_MEM };
    DevBatch::Mem mem[N_MEM];
    char *hmeta = nullptr;   // pinned staging of meta
    size_t hmeta_cap = 0;
    unsigned long long *hout = nullptr;  // pinned landing of out (2 words)
    size_t hout_cap = 0;
    hipEvent_t ev[4] = {};
    double ms[4] = {0, 0, 0, 0};
    ~CounterDev() {
        for (DevBatch::Mem &m : mem)
            if (m.p) (void)hipFree(m.p);
        if (hmeta) (void)hipHostFree(hmeta);
        if (hout) (void)hipHostFree(hout);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

// lc_queue_check's state on a device (device_api.hip; the kernels are
// device_queue.hip's): the hash table, the batch's arrays, the per-key words
// and the entries, pinned landings and timing events, grown on demand and kept
// from one call to the next.
struct QueueDev {
    // keyst: counts [K][7], lo [K], hi [K] in one block (one copy back); out: the entry cursor and the error word
    enum { ROW_KEY, ROW_KIND, ROW_VAL, STATUS, TABLE, KEYST, ENT_KEY, ENT_CLASS, ENT_VAL, ENT_MULT, OUT, N_MEM };
    DevBatch::Mem mem[N_MEM];
    char *hkeyst = nullptr;  // pinned landing of keyst, and staging of status before it
    size_t hkeyst_cap = 0;
    char *hent = nullptr;    // pinned landing of the four entry arrays
    size_t hent_cap = 0;
    unsigned long long *hout = nullptr;  // pinned landing of out
    size_t hout_cap = 0;
    hipEvent_t ev[4] = {};
    double ms[4] = {0, 0, 0, 0};
    ~QueueDev() {
        for (DevBatch::Mem &m : mem)
            if (m.p) (void)hipFree(m.p);
        if (hkeyst) (void)hipHostFree(hkeyst);
        if (hent) (void)hipHostFree(hent);
        if (hout) (void)hipHostFree(hout);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

// What a search step reaches through stream order, one copy per search
// lane: consecutive enqueued register-tier steps of lc_check_node_async
// search on the two lanes in turn and overlap (lane_plan.hpp); every other
// step runs on lane 0, after joining lane 1.
struct Lane {
    hipStream_t stream = nullptr;
    // a step's verdicts when its results stay in the context (RES_CTX, RES_HOST)
    int8_t *valid = nullptr;
    int32_t *fail_event = nullptr;
    uint8_t *cause = nullptr;
    // speculative segments: each wave's 9-10-pending workspace, the rerun list
    uint32_t *spec_ws = nullptr;
    size_t spec_ws_words = 0;
    uint32_t *spec_fin = nullptr;  // exact speculative segments: each run's saved set
    size_t spec_fin_words = 0;
    int32_t *spec_rr = nullptr;    // two rerun counts (used in turn), then the rerun list
    int64_t spec_rr_cap = 0;
    int spec_parity = 0;
    // Device copies of T0's Args (read once per key): a ring of 12, so steps
    // alternating between result sets (the N > 1 bench), or pipelined steps
    // between their staging batches and error words (3 x 4 in turn on one
    // lane, 3 x 2 on each of two), each find theirs without a copy; a slot's
    // pinned staging copy is rewritten only after the copy out of it
    // (args_ev) has run.
    static constexpr int ARGS_RING = 12;
    lcd::Args *dargs = nullptr;    // [ARGS_RING]
    lcd::Args *hargs = nullptr;    // [ARGS_RING] pinned
    hipEvent_t args_ev[ARGS_RING] = {};
    bool args_ok[ARGS_RING] = {};
    uint32_t args_next = 0;
    // an overlapping step's records when they cannot go straight into the
    // caller's buffer (a step still in flight was given it too)
    uint64_t *rec = nullptr;
    int64_t rec_cap = 0;
    hipEvent_t done = nullptr;  // lane 1: everything enqueued on it, for lane 0 to join
    void free_all() {
        dfree(valid); dfree(fail_event); dfree(cause);
        dfree(spec_ws); dfree(spec_rr); dfree(spec_fin); dfree(dargs); dfree(rec);
        if (hargs) (void)hipHostFree(hargs);
        hargs = nullptr;
        for (hipEvent_t &e : args_ev) {
            if (e) (void)hipEventDestroy(e);
            e = nullptr;
        }
        if (done) (void)hipEventDestroy(done);
        done = nullptr;
    }
};

// One device of a context: its streams, scratch and result arrays.
struct Dev {
    const lc_opts *o = nullptr;  // the context's options
    int device = 0;
    int cu_count = 256;
    hipStream_t stream = nullptr;   // lane 0's (lane[0].stream): every step but the overlapping ones' second
    hipStream_t stream1 = nullptr;  // lane 1's: every second overlapping search; else the validation of
                                    // host-unchecked batches, beside T0
    Lane lane[lc::LANES];
    bool lane1_live = false;        // lane 1 has work lane 0 has not joined
    bool lane1_wait_start = false;  // lane 1's next search first waits for run_start
    uint64_t run_n = 0;             // overlapping steps since the lanes were last joined
    hipEvent_t run_start = nullptr; // lane 0, ahead of such a run's first search (its set-up done)
    hipStream_t cstream = nullptr;  // lc_check_node's chunked uploads, ahead of the searches
    hipStream_t estream = nullptr;  // lc_wait_step's error reads (behind no upload or step)
    static constexpr int NODE_CHUNKS = 4;
    DevBatch *chunk[NODE_CHUNKS] = {};
    hipEvent_t chunk_ready[NODE_CHUNKS] = {};
    hipEvent_t vin = nullptr, vdone = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr, et0 = nullptr, et3a = nullptr, et3b = nullptr;
    hipEvent_t ea0 = nullptr, ea1 = nullptr;  // span of the LC_DEV_ASYNC steps since lc_wait
    uint32_t n_async = 0;
    bool ea1_pending = false;  // asynchronous steps enqueued since ea1 was last recorded
    hipEvent_t ring[4] = {};  // end of each of the last 4 LC_DEV_ASYNC steps (lc_wait_step)
    uint64_t async_seq = 0;
    // scratch, grown on demand
    int64_t cap_keys = 0;
    int32_t *lists = nullptr;      // 5 x cap_keys: spill0, spill1, spill2, wide, old (T3L -> narrow T3)
    // one 96-byte control block, zeroed and read back in one operation each:
    // acc (4 x u64: probes, events, keys_done, T3L stream bytes) then counters (16 x i32:
    // n_spill0, n_spill1, n_spill2, n_wide, err bits, 1 + bad key, n_old, -,
    // tickets[8..15])
    unsigned long long *ctl = nullptr;
    unsigned long long *acc = nullptr;
    int32_t *counters = nullptr;
    unsigned long long *hctl = nullptr;  // pinned host copy of ctl
    uint32_t *peak = nullptr;
    uint64_t *final_cfg = nullptr;
    uint32_t *n_final = nullptr;
    DevBatch *staged = nullptr;    // lc_check_batch's staging batch (device arrays reused)
    // T0-only steps skip re-zeroing the control block: the ticket continues
    // from where the previous such step left it.
    bool ticket_live = false;
    uint32_t ticket_next = 0;
    // key segments (register-tier steps of a batch of about one key per
    // SIMD): per-key cut points, segment results, work lists
    int64_t seg_keys = 0;
    uint32_t *seg_cnt = nullptr, *seg_end = nullptr, *seg_out = nullptr, *seg_work = nullptr;
    uint32_t *seg_rerun = nullptr, *seg_rerun_init = nullptr;
    int32_t *seg0_fev = nullptr, *seg_ctl = nullptr;
    // node records (lc_check_node): this rank's block and the gathered node
    uint64_t *send = nullptr, *node = nullptr;
    int64_t node_cap = 0, node_n = 0;
    uint64_t *rec_out = nullptr;  // set around a node step's search: finish_key writes the records there
    uint64_t *hnode = nullptr;  // pinned landing area of the node's records (lc_check_node)
    int64_t hnode_cap = 0;
    // lc_check_node_async: three staging batches used in turn, so a step's
    // upload (on cstream) runs while the two steps before it search; pipe_ready
    // = a slot's upload is done; the step that read a slot is done when its
    // ring event (async_seq pipe_seq[s]) is; pipe_lo .. pipe_hi = the
    // caller's record buffer that step was given
    static constexpr int PIPE = lc::LANE_SLOTS;
    DevBatch *pipe[PIPE] = {};
    hipEvent_t pipe_ready[PIPE] = {};
    uint64_t pipe_seq[PIPE] = {};
    bool pipe_busy[PIPE] = {};
    uint64_t pipe_lo[PIPE] = {}, pipe_hi[PIPE] = {};
    uint64_t pipe_next = 0;
    // T3 (HBM tier) workspaces: narrow / wide configs
    struct Ws {
        char *base = nullptr;
        size_t bytes = 0;
        int slots = 0;
        lcd::HbmWs w{};
    } ws[2];
    // layered T3 workspace (device_layers.hip)
    struct LWs {
        char *base = nullptr;
        size_t bytes = 0;
        int slots = 0;
        lcd::LayWs w{};
    } lws;
    // knossos.wgl workspaces (device_wgl.hip): [0] tables sized to share at
    // most a share of the free HBM (WGL_SHARE_MAX), [1] tables the budget
    // fits, for the keys that outgrow [0]; zeroed once (entries are stamped)
    struct WWs {
        char *base = nullptr;
        size_t bytes = 0;
        lcd::WglWs layout{};  // the layout its contents were written under
        int slots = 0;
    } wws[2];
    uint32_t wgl_seq = 0;     // launches so far (the high half of every cache stamp)
    uint8_t *analyzer = nullptr;  // [cap_keys] LC_ALGO_* that answered each key
    lcs::SetDev *setdev = nullptr;  // lc_set_check's cached arrays (device_set.hip), made on first use
    lcp::PerfDev *perfdev = nullptr;  // lc_perf_check's (device_perf.hip), likewise
    lcf::SetFullDev *setfulldev = nullptr;  // lc_setfull_check's (device_setfull.hip), likewise
    CounterDev *counterdev = nullptr;  // lc_counter_check's (device_api.hip), likewise
    QueueDev *queuedev = nullptr;  // lc_queue_check's (device_api.hip), likewise
    // lc_counter_check_history's (device_counter_pack.hip, in libcounter_pack_kernels.so, which also frees it), likewise
    void *cpackdev = nullptr;
    void (*cpackdev_free)(void *) = nullptr;
    // lc_perf_check_history's (device_perf_pack.hip, in libperf_pack_kernels.so, which also frees it), likewise; the batch
    // it builds lies in perfdev's record columns
    void *ppackdev = nullptr;
    void (*ppackdev_free)(void *) = nullptr;
    ~Dev() {
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
        if (stream1) (void)hipStreamSynchronize(stream1);
        lcs::set_dev_free(setdev);
        lcp::perf_dev_free(perfdev);
        lcf::setfull_dev_free(setfulldev);
        delete counterdev;
        delete queuedev;
        if (cpackdev_free) cpackdev_free(cpackdev);
        if (ppackdev_free) ppackdev_free(ppackdev);
        dfree(lists); dfree(ctl);
        if (hctl) (void)hipHostFree(hctl);
        dfree(peak); dfree(final_cfg); dfree(n_final);
        dfree(ws[0].base); dfree(ws[1].base); dfree(lws.base); dfree(send); dfree(node);
        dfree(wws[0].base); dfree(wws[1].base); dfree(analyzer);
        dfree(seg_cnt); dfree(seg_end); dfree(seg_out); dfree(seg_work); dfree(seg_rerun); dfree(seg_rerun_init);
        dfree(seg0_fev); dfree(seg_ctl);
        for (Lane &l : lane) l.free_all();
        if (hnode) (void)hipHostFree(hnode);
        delete staged;
        for (int i = 0; i < PIPE; ++i) {
            delete pipe[i];
            for (hipEvent_t e : {pipe_ready[i]})
                if (e) (void)hipEventDestroy(e);
        }
        for (int i = 0; i < NODE_CHUNKS; ++i) {
            delete chunk[i];
            if (chunk_ready[i]) (void)hipEventDestroy(chunk_ready[i]);
        }
        if (cstream) (void)hipStreamSynchronize(cstream);
        if (cstream) (void)hipStreamDestroy(cstream);
        if (estream) (void)hipStreamSynchronize(estream);
        if (estream) (void)hipStreamDestroy(estream);
        for (hipEvent_t e : {e0, e1, et0, et3a, et3b, ea0, ea1, vin, vdone, run_start})
            if (e) (void)hipEventDestroy(e);
        if (stream1) (void)hipStreamDestroy(stream1);
        for (hipEvent_t &e : ring)
            if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

}  // namespace lcx

struct lc_dev_batch {
    int n_parts = 0;
    int64_t n_keys = 0;
    int64_t key0[lcx::MAX_DEV + 1] = {};  // part g holds keys [key0[g], key0[g + 1])
    lcx::DevBatch *part[lcx::MAX_DEV] = {};
    ~lc_dev_batch() {
        for (lcx::DevBatch *p : part)
            if (p) {
                (void)hipSetDevice(p->device);
                delete p;
            }
    }
};

struct lc_ctx {
    lc_opts o{};
    int n_dev = 0;
    lcx::Dev *dev[lcx::MAX_DEV] = {};
    std::mutex mu;                 // one call at a time (include/lincheck.h)
    lc::HostPool *pool = nullptr;      // validation / staging workers, created on first use
    lc::HostPool *drivers = nullptr;   // one thread per device beyond the first
    uint32_t *hstage = nullptr;    // pinned copy of a batch's event words
    size_t hstage_cap = 0;
    // one process per GPU: RCCL communicator over the node's ranks
    ncclComm_t comm = nullptr;
    int rank = 0, size = 1;
    ~lc_ctx() {
        if (comm) {
            (void)hipSetDevice(dev[0]->device);
            (void)hipStreamSynchronize(dev[0]->stream);
            if (const lcx::Rccl *R = lcx::rccl()) (void)R->comm_destroy(comm);
        }
        for (lcx::Dev *d : dev) delete d;
        delete pool;
        delete drivers;
        if (hstage) (void)hipHostFree(hstage);
    }
};

namespace lcx {

// What the register tier needs to know of a batch before any upload: the
// state count of a shared table and whether every key is declared to fit T0
// (width, states, initial state).  A batch that does is validated by T0
// itself (T0_STRICT), so the host skips its per-event pass.
struct Shape {
    uint32_t shared_states = 0;
    bool t0_only = false;
    bool taggable = false;  // segments (lcd::SegArgs): shared table, states 0..5 from nil, nothing installs nil
    bool seg_pays = false;  // sampled keys: the longest stretch without a quiescent point is short
    bool host_checked = false;  // prepare_batch walked every event (table models: their rows too)
};

enum ResMode { RES_HOST = 0, RES_DEV = 1, RES_CTX = 2 };

// How lc_check_node_async places an enqueued step (lane_plan.hpp): its lane,
// and for records that go through the lane's block (Lane::rec) their download
// -- n records to dst behind the searches' launches, once `after` has passed.
struct LaneUse {
    int lane = 0;
    bool overlap = false;
    uint64_t *dst = nullptr;
    size_t n = 0;
    hipEvent_t after = nullptr;
};

// device_api.hip's, as the node steps and the stream call them (each is described where it is defined).
int join_lanes(Dev *c);
int drain_lanes(Dev *c);
int ensure_capacity(Dev *c, int64_t n_keys);
bool pinned(const void *p);
lc_batch sub_batch(const lc_batch *b, int64_t k0, int64_t k1, std::vector<uint64_t> &off);
void shard_keys(const lc_batch *b, int n, int64_t *key0);
int upload_into(Dev *c, const lc_batch *b, DevBatch *d, const Shape &sh, bool validated,
                const uint32_t *events_src = nullptr, bool sync = true, hipStream_t stream = nullptr);
int prepare_batch(lc_ctx *c, const lc_batch *b, Shape *sh, const uint32_t **src);
int dev_search(Dev *c, const DevBatch *d, const lc_result *r, ResMode mode, bool allow_async, int64_t key0,
               lc_stats *st, bool *enqueued = nullptr, int64_t res_off = 0, const LaneUse *lu = nullptr);
int dev_wait(Dev *c, int *n_async, float *span_ms);
lc::StepPlan node_step_plan(Dev *c, const DevBatch *d);

// A call that works on the context's one device behind everything enqueued
// so far: holds the context's lock from its construction on; enter() makes
// the device current and puts lane 0 behind lane 1.
struct CtxCall {
    std::lock_guard<std::mutex> lock;
    Dev *d;
    explicit CtxCall(lc_ctx *c) : lock(c->mu), d(c->dev[0]) {}
    int enter() {
        HIPCHK(hipSetDevice(d->device));
        return join_lanes(d);
    }
};

// Grow a device buffer to `need` elements, its contents not kept.  c: the
// device whose enqueued steps may still be using the one it replaces (the
// speculative segments' buffers), or null.
template <class T, class N>
int grow_dev(Dev *c, T *&ptr, N &have, N need) {
    if (need <= have) return LC_OK;
    if (c && c->n_async) LCCHK(drain_lanes(c));
    dfree(ptr);
    have = 0;
    HIPCHK(dalloc(&ptr, (size_t)need));
    have = need;
    return LC_OK;
}

// A staging batch of the context, made on first use.
inline int staging_batch(DevBatch *&p, const char *who) {
    if (!p) p = new (std::nothrow) DevBatch();
    return p ? LC_OK : lc::fail(LC_E_NOMEM, "%s: out of memory", who);
}

// grow_dev for a page-locked host buffer.
template <class T, class N>
hipError_t grow_pinned(T *&ptr, N &have, N need) {
    if (need <= have) return hipSuccess;
    if (ptr) (void)hipHostFree(ptr);
    ptr = nullptr;
    have = 0;
    const hipError_t e = hipHostMalloc((void **)&ptr, (size_t)need * sizeof(T), hipHostMallocDefault);
    if (e == hipSuccess) have = need;
    return e;
}

}  // namespace lcx
