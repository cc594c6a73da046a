// device_node.hip -- one process per GPU: node-wide verdict records (C ABI: lc_check_node, _async, _device,
// lc_node_records; include/lincheck.h).  Host code only: a node step is prepare_batch, upload_into and
// dev_search of device_api.hip around the record buffers here, each entry point a sequence of named stages.

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "device_ctx.hpp"

using namespace lcx;

// A node step as its stages see it: the call's arguments, the batch's shape,
// and for an enqueued step its staging slot, lane and record route.
struct NodeStep {
    lc_ctx *x;
    Dev *d;
    const lc_batch *b;
    int64_t block;
    uint64_t *node;
    lc_stats *st;
    Shape sh{};                     // from prepare_batch, with src
    const uint32_t *src = nullptr;  // where the uploads read the events from (prepare_batch)
    bool enq = false;               // the search was only enqueued
    int slot = 0;
    uint64_t *dnode = nullptr;      // `node` as the device sees it, when it is mapped
    lc::LaneIn li{};
    lc::LanePlan lp{};
    LaneUse lu{};
    std::chrono::steady_clock::time_point t0, t_prep, t_up, t_search, t_gather;  // lc_check_node's LC_TIMING line
};

// The rank's record block (and the node's), grown on demand; the search that
// follows writes its records straight into the block (Dev::rec_out), and the
// padding past the shard's n keys is zeroed.
static int node_buffers(lc_ctx *x, Dev *c, int64_t n, int64_t block) {
    if (block > c->node_cap || !c->send) {
        if (c->n_async) LCCHK(drain_lanes(c));  // an enqueued step may still write them
        dfree(c->send);
        dfree(c->node);
        HIPCHK(dalloc(&c->send, (size_t)std::max<int64_t>(block, 1)));
        HIPCHK(dalloc(&c->node, (size_t)std::max<int64_t>(block, 1) * x->size));
        c->node_cap = block;
    }
    uint64_t *blk = x->comm ? c->send : c->node;
    if (block > n) HIPCHK(hipMemsetAsync(blk + n, 0, (size_t)(block - n) * 8, c->stream));
    c->rec_out = blk;
    return LC_OK;
}

// All-gather every rank's block (the records the search wrote) over RCCL on
// c's stream; one rank: the block is the node.
static int gather_node(lc_ctx *x, Dev *c, int64_t block) {
    lc::Range range("lincheck: gather");
    c->rec_out = nullptr;
    if (x->comm) {
        const Rccl *R = rccl();
        RCCLCHK(R->all_gather(c->send, c->node, (size_t)block, ncclUint64, x->comm, c->stream));
    }
    c->node_n = block * x->size;
    return LC_OK;
}

// Stops later searches writing records, on every return of a node step.
struct RecOff {
    Dev *d;
    ~RecOff() { d->rec_out = nullptr; }
};

// A node step's error return: the copies out of the caller's arrays are waited for.
static int drained(Dev *d, int e) {
    (void)hipStreamSynchronize(d->cstream);
    (void)hipStreamSynchronize(d->stream1);
    (void)hipStreamSynchronize(d->stream);
    d->lane1_live = d->lane1_wait_start = false;
    d->run_n = 0;
    return e;
}

// An overlapping step's record block on its lane (grown on demand), the
// padding past the shard's n keys zeroed: the search writes its records
// there, and they are copied out behind it (finish_async).
static int lane_records(Dev *c, Lane &L, int64_t n, int64_t block) {
    LCCHK(grow_dev(c, L.rec, L.rec_cap, std::max<int64_t>(block, 1)));
    if (block > n) HIPCHK(hipMemsetAsync(L.rec + n, 0, (size_t)(block - n) * 8, L.stream));
    c->rec_out = L.rec;
    return LC_OK;
}

static int node_check_args(lc_ctx *c, int64_t n_keys, int64_t block) {
    if (c->n_dev != 1) return lc::fail(LC_E_INVALID, "lc_check_node: needs a one-device context");
    if (block < n_keys) return lc::fail(LC_E_INVALID, "lc_check_node: block %lld < the shard's %lld keys",
                                        (long long)block, (long long)n_keys);
    return LC_OK;
}

// ---- lc_check_node: the synchronous step --------------------------------------

// A large register-tier shard (throughput-bound: many keys per SIMD) is
// uploaded and searched in NODE_CHUNKS key chunks: the copies run on a
// stream of their own, and each chunk's search waits only for its own
// copy, so the host-to-device transfer overlaps the search
// (lc_opts.path_flags LC_PATH_CHUNKS_ON / _OFF pin the choice).
// (Searching page-locked event words in place, over the host link, was
// measured slower: 0.468 against 0.332 ms for C2's search, the link
// sustaining ~31 GB/s of kernel reads; the 16-bit upload won instead.)
static int node_chunks(const NodeStep &s) {
    const lc_opts &o = s.x->o;
    const int64_t K = s.b->n_keys;
    const uint64_t n_ev = K ? s.b->ev_off[K] : 0;
    const bool can_chunk = s.sh.t0_only && !(o.flags & LC_OPT_COUNT_PROBES) && K >= Dev::NODE_CHUNKS;
    bool big = K >= 16 * (int64_t)s.d->cu_count && n_ev >= (8u << 20);
    if (o.path_flags & LC_PATH_CHUNKS_ON) big = true;
    if (o.path_flags & LC_PATH_CHUNKS_OFF) big = false;
    return can_chunk && big ? Dev::NODE_CHUNKS : 1;
}

// The chunked step: every chunk's upload on the copy stream, then their
// searches, each behind its own chunk's copy.
static int node_search_chunked(NodeStep &s, int chunks) {
    Dev *d = s.d;
    const lc_batch *b = s.b;
    LCCHK(ensure_capacity(d, b->n_keys));
    int64_t key0[Dev::NODE_CHUNKS + 1];
    shard_keys(b, chunks, key0);
    for (int i = 0; i < chunks; ++i) {
        if (int rc = staging_batch(d->chunk[i], "lc_check_node")) return drained(d, rc);
        if (!d->chunk_ready[i]) HIPCHK(hipEventCreateWithFlags(&d->chunk_ready[i], hipEventDisableTiming));
        std::vector<uint64_t> off;
        const lc_batch sub = sub_batch(b, key0[i], key0[i + 1], off);
        const uint32_t *es = s.src ? s.src + b->ev_off[key0[i]] : nullptr;
        if (int rc = upload_into(d, &sub, d->chunk[i], s.sh, s.sh.host_checked, es, false, d->cstream))
            return drained(d, rc);
        HIPCHK(hipEventRecord(d->chunk_ready[i], d->cstream));
    }
    s.t_up = std::chrono::steady_clock::now();
    const lc_result none{};
    for (int i = 0; i < chunks; ++i) {
        HIPCHK(hipStreamWaitEvent(d->stream, d->chunk_ready[i], 0));
        bool e = false;
        if (int rc = dev_search(d, d->chunk[i], &none, RES_CTX, true, key0[i], s.st, &e, key0[i])) return drained(d, rc);
        s.enq = i == 0 ? e : (s.enq && e);
    }
    if (!s.enq) return drained(d, lc::fail(LC_E_DEVICE, "lc_check_node: a chunk left the register tier"));
    return LC_OK;
}

// The whole shard in one upload (the context's staging batch) and one search.
static int node_search_whole(NodeStep &s) {
    Dev *d = s.d;
    LCCHK(upload_into(d, s.b, d->staged, s.sh, s.sh.host_checked, s.src, false));
    s.t_up = std::chrono::steady_clock::now();
    const lc_result none{};
    if (int rc = dev_search(d, d->staged, &none, RES_CTX, true, 0, s.st, &s.enq)) return drained(d, rc);
    return LC_OK;
}

// The node's records into the caller's array: they land in pinned memory (a
// copy into the caller's pageable array would be a synchronous staged copy)
// and are copied out after the wait.
static int node_land_records(NodeStep &s) {
    Dev *d = s.d;
    if (int rc = gather_node(s.x, d, s.block)) return drained(d, rc);
    if (grow_pinned(d->hnode, d->hnode_cap, d->node_n) != hipSuccess)
        return drained(d, lc::fail(LC_E_NOMEM, "lc_check_node: pinned record buffer"));
    if (d->node_n && hipMemcpyAsync(d->hnode, d->node, (size_t)d->node_n * 8, hipMemcpyDeviceToHost, d->stream) !=
                         hipSuccess)
        return drained(d, lc::fail(LC_E_DEVICE, "lc_check_node: record download failed"));
    s.t_gather = std::chrono::steady_clock::now();
    if (s.enq) {  // a T0-only step (or chunks): one wait for the search, the exchange and the download
        int n_async = 0;
        float span = 0;
        if (int rc = dev_wait(d, &n_async, &span)) return drained(d, rc);
        if (s.st) s.st->kernel_ms = s.st->tier0_ms = span;
    } else {
        HIPCHK(hipStreamSynchronize(d->stream));
    }
    if (d->node_n) std::memcpy(s.node, d->hnode, (size_t)d->node_n * 8);
    return LC_OK;
}

static void node_timing_line(const NodeStep &s) {
    using ms = std::chrono::duration<double, std::milli>;
    std::fprintf(stderr, "lc_check_node: prepare %.3f, upload %.3f, search enqueue %.3f, gather enqueue %.3f, "
                 "wait %.3f ms (search span %.3f)\n", ms(s.t_prep - s.t0).count(), ms(s.t_up - s.t_prep).count(),
                 ms(s.t_search - s.t_up).count(), ms(s.t_gather - s.t_search).count(),
                 ms(std::chrono::steady_clock::now() - s.t_gather).count(), s.st ? s.st->kernel_ms : 0.f);
}

extern "C" int lc_check_node(lc_ctx *c, const lc_batch *b, int64_t block, uint64_t *node, lc_stats *st) {
    lc::Range range("lc_check_node");
    const auto t0 = std::chrono::steady_clock::now();
    if (!c || !b || !node) return lc::fail(LC_E_INVALID, "lc_check_node: null argument");
    std::lock_guard<std::mutex> g(c->mu);
    LCCHK(node_check_args(c, b->n_keys, block));
    NodeStep s{c, c->dev[0], b, block, node, st};
    s.t0 = t0;
    LCCHK(prepare_batch(c, b, &s.sh, &s.src));
    LCCHK(staging_batch(s.d->staged, "lc_check_node"));
    LCCHK(node_buffers(c, s.d, b->n_keys, block));
    RecOff rec_off{s.d};
    s.t_prep = std::chrono::steady_clock::now();
    const int chunks = node_chunks(s);
    LCCHK(chunks > 1 ? node_search_chunked(s, chunks) : node_search_whole(s));
    s.t_search = std::chrono::steady_clock::now();
    LCCHK(node_land_records(s));
    if (std::getenv("LC_TIMING")) node_timing_line(s);
    if (st) st->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return LC_OK;
}

// ---- lc_check_node_async: the pipelined step ----------------------------------

// May the step be enqueued at all?  Keys and events, no table model, no probe counting, records to
// page-locked memory.  (A large shard is not cut into chunks here: its whole upload overlaps the
// previous step's search instead.)
static bool node_step_can_enqueue(const lc_ctx *c, const lc_batch *b, const uint64_t *node) {
    const int64_t K = b->n_keys;
    const uint64_t n_ev = K ? b->ev_off[K] : 0;
    return K > 0 && n_ev > 0 && !b->table && !(c->o.flags & LC_OPT_COUNT_PROBES) && pinned(node) &&
           !(c->o.path_flags & LC_PATH_NODE_SYNC);
}

// The step's staging slot (made on first use) and its upload, on the copy
// stream.  Where the step runs is plan_lane's choice (lane_plan.hpp); its
// staging slot follows from the sequence number alone.
static int node_step_upload(NodeStep &s) {
    Dev *d = s.d;
    s.li.seq = d->pipe_next;
    const int t = s.slot = lc::plan_lane(s.li).slot;
    LCCHK(staging_batch(d->pipe[t], "lc_check_node_async"));
    // (a device-scope release: the host only learns from it that the upload's device writes are done)
    if (!d->pipe_ready[t] &&
        hipEventCreateWithFlags(&d->pipe_ready[t], hipEventDisableTiming | hipEventReleaseToDevice) != hipSuccess) {
        (void)hipGetLastError();
        HIPCHK(hipEventCreateWithFlags(&d->pipe_ready[t], hipEventDisableTiming));
    }
    // the step that last read this slot (three back) has finished -- at most two other steps stay in
    // flight, one on each lane -- so its buffers may be rewritten or regrown.  Its end is the ring event its
    // search recorded: a marker of its own after every step cost the stream ~5 us between consecutive
    // searches (a system-scope fence each).
    // (A ring slot re-recorded since by a later step only makes this wait for that later step.)
    if (d->pipe_busy[t]) HIPCHK(hipEventSynchronize(d->ring[d->pipe_seq[t] % 4]));
    d->pipe_busy[t] = false;
    if (int rc = upload_into(d, s.b, d->pipe[t], s.sh, s.sh.host_checked, s.src, false, d->cstream)) return drained(d, rc);
    HIPCHK(hipEventRecord(d->pipe_ready[t], d->cstream));
    return LC_OK;
}

// What plan_lane decides from: the step's plan, the caller's buffer, and the
// steps still in flight (those whose ring event has passed are retired here).
static void node_step_lane_in(NodeStep &s) {
    Dev *d = s.d;
    lc::LaneIn &li = s.li;
    li.mapped = hipHostGetDevicePointer((void **)&s.dnode, s.node, 0) == hipSuccess && s.dnode;
    if (!li.mapped) (void)hipGetLastError();
    const lc::StepPlan stp = node_step_plan(d, d->pipe[s.slot]);
    li.run_n = d->run_n;
    li.async = stp.async; li.spec = stp.spec; li.split = stp.split;
    li.waves = s.b->n_keys * stp.segs;
    li.resident_waves = (int64_t)d->cu_count * 4 * LC_SPEC8_WAVES;
    li.comm = s.x->comm != nullptr;
    li.path_flags = s.x->o.path_flags;
    li.lo = (uint64_t)(uintptr_t)s.node;
    li.hi = li.lo + (uint64_t)std::max<int64_t>(s.block, 1) * 8;
    for (int t = 0; t < Dev::PIPE; ++t) {
        if (t == s.slot || !d->pipe_busy[t]) continue;
        if (hipEventQuery(d->ring[d->pipe_seq[t] % 4]) == hipSuccess) {
            d->pipe_busy[t] = false;
            continue;
        }
        (void)hipGetLastError();
        lc::LaneIn::Flight &f = li.flight[li.n_flight++];
        f.seq = d->pipe_seq[t]; f.lo = d->pipe_lo[t]; f.hi = d->pipe_hi[t];
    }
}

// The lane, and how the records reach `node`.  One rank: the search writes them straight into the
// caller's page-locked buffer (device-mapped), so no download follows it -- unless a step still in flight
// was given that buffer too and this step may overlap it: then they go through the lane's block in HBM
// and are copied out behind that step's end, so the buffer ends up with the latest step's records.  With
// a communicator they go through HBM for the all-gather.
static int node_step_route(NodeStep &s) {
    Dev *d = s.d;
    const int64_t K = s.b->n_keys;
    const lc::LanePlan &lp = s.lp = lc::plan_lane(s.li);
    s.lu.lane = lp.lane;
    s.lu.overlap = lp.overlap;
    if (lp.direct) {
        if (s.block > K) std::memset(s.node + K, 0, (size_t)(s.block - K) * 8);
        d->rec_out = s.dnode;
        return LC_OK;
    }
    if (!lp.overlap) return node_buffers(s.x, d, K, s.block);
    LCCHK(lane_records(d, d->lane[lp.lane], K, s.block));
    s.lu.dst = s.node;
    s.lu.n = (size_t)s.block;
    s.lu.after = lp.after >= 0 ? d->ring[lp.after % 4] : nullptr;
    return LC_OK;
}

// The host waits for the upload (the steps before are searching meanwhile) and then enqueues the search:
// no cross-stream wait on the device, whose latency sat between consecutive searches (C2 0.3415 ->
// 0.3365 ms per step).  It also frees the context's staging copy of pageable events.
static int node_step_search(NodeStep &s) {
    HIPCHK(hipEventSynchronize(s.d->pipe_ready[s.slot]));
    const lc_result none{};
    return dev_search(s.d, s.d->pipe[s.slot], &none, RES_CTX, true, 0, s.st, &s.enq, 0, &s.lu);
}

// Records that went through the node's block: the exchange, then out to `node`.
static int node_step_records_out(NodeStep &s) {
    Dev *d = s.d;
    if (s.lp.direct || s.lu.dst) {
        d->node_n = 0;  // the records are in `node` only (lc_node_records has none)
        return LC_OK;
    }
    LCCHK(gather_node(s.x, d, s.block));
    if (d->node_n && hipMemcpyAsync(s.node, d->node, (size_t)d->node_n * 8, hipMemcpyDeviceToHost, d->stream) != hipSuccess)
        return lc::fail(LC_E_DEVICE, "lc_check_node_async: record download failed");
    return LC_OK;
}

// The slot is the step's until its ring event has passed.
static void node_step_book(NodeStep &s) {
    Dev *d = s.d;
    d->pipe_busy[s.slot] = s.enq;
    d->pipe_seq[s.slot] = d->async_seq - 1;
    d->pipe_lo[s.slot] = s.li.lo;
    d->pipe_hi[s.slot] = s.li.hi;
    ++d->pipe_next;
}

// An eligible step, under the context's lock: 1 once it is enqueued.
static int node_step_enqueue(NodeStep &s) {
    LCCHK(node_step_upload(s));
    node_step_lane_in(s);
    if (int rc = node_step_route(s)) return drained(s.d, rc);
    RecOff rec_off{s.d};
    if (int rc = node_step_search(s)) return drained(s.d, rc);
    if (int rc = node_step_records_out(s)) return drained(s.d, rc);
    node_step_book(s);
    if (s.enq) return 1;
    HIPCHK(hipStreamSynchronize(s.d->stream));  // not reached for a register-tier batch
    return LC_OK;
}

// The pipelined form of lc_check_node.  A register-tier step (every key fits
// the register lattice, no probe counting, one upload, records to page-locked
// memory) is only enqueued: its upload goes into the staging slot the step
// three back used (once that step is done) on the copy stream, its search
// follows that upload on one of the two search lanes, and the records land
// in `node` with the search or behind it.  So step i + 2's host-to-device
// copy overlaps the searches of steps i and i + 1, step i + 1's workgroups
// take the slots step i's finished blocks free (lane_plan.hpp), and the host
// enqueues ahead instead of waiting between steps.
// Anything else runs as lc_check_node.
extern "C" int lc_check_node_async(lc_ctx *c, const lc_batch *b, int64_t block, uint64_t *node, lc_stats *st) {
    lc::Range range("lc_check_node_async");
    if (!c || !b || !node) return lc::fail(LC_E_INVALID, "lc_check_node_async: null argument");
    {
        std::lock_guard<std::mutex> g(c->mu);
        LCCHK(node_check_args(c, b->n_keys, block));
        NodeStep s{c, c->dev[0], b, block, node, st};
        HIPCHK(hipSetDevice(s.d->device));
        if (node_step_can_enqueue(c, b, node)) {
            LCCHK(prepare_batch(c, b, &s.sh, &s.src));
            if (s.sh.t0_only) return node_step_enqueue(s);  // every key fits the register tier
        }
    }
    return lc_check_node(c, b, block, node, st);
}

extern "C" int lc_check_node_device(lc_ctx *c, const lc_dev_batch *db, int64_t block, int flags, lc_stats *st) {
    if (!c || !db) return lc::fail(LC_E_INVALID, "lc_check_node_device: null argument");
    if (flags & ~LC_DEV_ASYNC) return lc::fail(LC_E_INVALID, "lc_check_node_device: unknown flags 0x%x", flags);
    std::lock_guard<std::mutex> g(c->mu);
    LCCHK(node_check_args(c, db->n_keys, block));
    if (db->n_parts != 1 || db->part[0]->device != c->dev[0]->device)
        return lc::fail(LC_E_INVALID, "lc_check_node_device: batch lives on another device");
    Dev *d = c->dev[0];
    const lc_result none{};
    bool enq = false;
    LCCHK(node_buffers(c, d, db->n_keys, block));
    RecOff rec_off{d};
    LCCHK(dev_search(d, db->part[0], &none, RES_CTX, (flags & LC_DEV_ASYNC) != 0, 0, st, &enq));
    LCCHK(gather_node(c, d, block));
    if (!enq) HIPCHK(hipStreamSynchronize(d->stream));
    return LC_OK;
}

extern "C" int lc_node_records(lc_ctx *c, uint64_t *node, int64_t n) {
    if (!c || (!node && n)) return lc::fail(LC_E_INVALID, "lc_node_records: null argument");
    CtxCall x(c);
    Dev *d = x.d;
    if (n > d->node_n) return lc::fail(LC_E_INVALID, "lc_node_records: %lld records asked, %lld gathered",
                                       (long long)n, (long long)d->node_n);
    LCCHK(x.enter());
    if (n) HIPCHK(hipMemcpyAsync(node, d->node, (size_t)n * 8, hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    return LC_OK;
}
