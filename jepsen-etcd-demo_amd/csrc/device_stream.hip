// device_stream.hip -- a resident search (lc_stream_*; device_stream_lattice.hip
// k_stream, device_stream_set.hip): the device half of a stream, behind
// device_stream.hpp.  host_stream.cpp owns the stream (its packer, verdicts and
// C entry points); this is the per-key records and the launches of one call.
// Host code only.

#include <cstddef>
#include <cstring>

#include "device_ctx.hpp"
#include "device_stream.hpp"
#include "stream_plan.hpp"

using namespace lcx;

static_assert(sizeof(lcst::Item) == sizeof(lcd::StreamItem) && offsetof(lcst::Item, ns) == offsetof(lcd::StreamItem, ns),
              "lcst::Item is lcd::StreamItem");

struct lcst::StreamDev {
    lc_ctx *ctx = nullptr;
    uint32_t *rec = nullptr;   // STREAM_REC_WORDS per key
    int64_t rec_cap = 0;       // keys
    char *din = nullptr, *hin = nullptr;  // a call's items, transitions, words: device, pinned host
    size_t din_cap = 0, hin_cap = 0;
    uint32_t *dout = nullptr, *hout = nullptr;  // the dead list
    size_t dout_cap = 0, hout_cap = 0;  // words
    hipEvent_t ev[6] = {};     // [4], [5]: after the migrations, after k_stream_set
    float ms[3] = {0, 0, 0};
    // the resident set tier: the set-record pool -- chunk c holds
    // SET_CHUNK0 << c slots of stream_set_slot_bytes() and never moves -- and
    // k_stream_set's workspace, one slot per resident workgroup
    std::vector<uint32_t *> set_chunk;
    std::vector<int32_t> set_free;
    int64_t set_slots = 0, set_used = 0, set_peak = 0;
    char *set_ws = nullptr;
    int set_ws_slots = 0;
    float set_ms[2] = {0, 0};
    // exact mode (LC_STREAM_EXACT): k_stream_exact's launches, and the keys'
    // final configs and their counts beside the records (same capacity)
    bool exact = false;
    uint64_t *fin = nullptr;
    uint32_t *nfin = nullptr;
    hipEvent_t fev[2] = {};
    float final_ms = 0;
};

namespace {
using namespace lcst;

constexpr size_t STREAM_OUT_HEAD = 63;  // dead keys read back with the count, in one copy
constexpr int64_t SET_CHUNK0 = 4;       // slots of the set-record pool's first chunk
constexpr int SET_GRID = 64;            // k_stream_set workgroups (and workspace slots) at most
size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }

// Pool slot -> its record (chunk c starts at slot SET_CHUNK0 * (2^c - 1)).
uint32_t *set_slot_ptr(const StreamDev *s, int64_t slot) {
    if (slot < 0 || slot >= s->set_slots) return nullptr;
    int c = 0;
    int64_t first = 0;
    while (slot >= first + (SET_CHUNK0 << c)) first += SET_CHUNK0 << c++;
    return s->set_chunk[(size_t)c] + (size_t)(slot - first) * lc::STREAM_SET_REC_WORDS;
}

// k_stream_set's workspace for `slots` resident workgroups, hash sets empty.
int set_ws_grow(StreamDev *s, Dev *d, int slots) {
    if (slots <= s->set_ws_slots) return LC_OK;
    const size_t slot_bytes = lcd::stream_set_ws_layout().slot_bytes;
    const int want = std::min(SET_GRID, std::max(slots, 2 * s->set_ws_slots));
    size_t have = (size_t)s->set_ws_slots * slot_bytes;
    s->set_ws_slots = 0;
    LCCHK(grow_dev(nullptr, s->set_ws, have, (size_t)want * slot_bytes));
    HIPCHK(hipMemsetAsync(s->set_ws, 0xFF, (size_t)want * slot_bytes, d->stream));  // EMPTY tables
    s->set_ws_slots = want;
    return LC_OK;
}

int stream_grow(StreamDev *s, Dev *d, int64_t n_keys, size_t in_bytes, size_t out_words) {
    if (n_keys > s->rec_cap) {
        const int64_t cap = std::max<int64_t>({n_keys, 2 * s->rec_cap, 64});
        uint32_t *nr = nullptr;
        HIPCHK(dalloc(&nr, (size_t)cap * lc::STREAM_REC_WORDS));
        const size_t old = (size_t)s->rec_cap * lc::STREAM_REC_WORDS * 4, all = (size_t)cap * lc::STREAM_REC_WORDS * 4;
        hipError_t e = hipSuccess;
        if (old) e = hipMemcpyAsync(nr, s->rec, old, hipMemcpyDeviceToDevice, d->stream);
        if (e == hipSuccess) e = hipMemsetAsync((char *)nr + old, 0, all - old, d->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
        if (e != hipSuccess) {
            dfree(nr);
            return lc::fail(LC_E_DEVICE, "lc_stream: growing the records failed: %s", hipGetErrorString(e));
        }
        if (s->exact) {  // the final-config arrays grow with the records
            const uint32_t mf = (uint32_t)s->ctx->o.max_final;
            const size_t of = (size_t)lc::stream_final_bytes((uint64_t)s->rec_cap, mf);
            const size_t af = (size_t)lc::stream_final_bytes((uint64_t)cap, mf);
            const size_t on = (size_t)lc::stream_nfinal_bytes((uint64_t)s->rec_cap);
            const size_t an = (size_t)lc::stream_nfinal_bytes((uint64_t)cap);
            uint64_t *nf = nullptr;
            uint32_t *nn = nullptr;
            e = dalloc(&nf, af / 8);
            if (e == hipSuccess) e = dalloc(&nn, an / 4);
            if (e == hipSuccess && of) e = hipMemcpyAsync(nf, s->fin, of, hipMemcpyDeviceToDevice, d->stream);
            if (e == hipSuccess && on) e = hipMemcpyAsync(nn, s->nfin, on, hipMemcpyDeviceToDevice, d->stream);
            if (e == hipSuccess) e = hipMemsetAsync((char *)nf + of, 0, af - of, d->stream);
            if (e == hipSuccess) e = hipMemsetAsync((char *)nn + on, 0, an - on, d->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
            if (e != hipSuccess) {
                dfree(nf);
                dfree(nn);
                dfree(nr);
                return lc::fail(LC_E_DEVICE, "lc_stream: growing the final configs failed: %s", hipGetErrorString(e));
            }
            dfree(s->fin);
            dfree(s->nfin);
            s->fin = nf;
            s->nfin = nn;
        }
        dfree(s->rec);
        s->rec = nr;
        s->rec_cap = cap;
    }
    if (in_bytes > s->hin_cap) {  // (the pair grows together: hin is the later of the two)
        const size_t cap = std::max<size_t>(in_bytes * 2, 1 << 16);
        LCCHK(grow_dev(nullptr, s->din, s->din_cap, cap));
        HIPCHK(grow_pinned(s->hin, s->hin_cap, cap));
    }
    if (out_words > s->hout_cap) {
        const size_t cap = std::max<size_t>(out_words * 2, 1024);
        LCCHK(grow_dev(nullptr, s->dout, s->dout_cap, cap));
        HIPCHK(grow_pinned(s->hout, s->hout_cap, cap));
    }
    return LC_OK;
}

// One stream_dev_push call: its arguments and the counts its parts share.
struct Push {
    int64_t n_keys, n_items;
    const Item *items;
    const uint16_t *ev16;
    const uint32_t *trans;
    uint64_t n_ev, n_trans;
    uint32_t init_state;
    const SetWork *set;
    int64_t n_mig, n_set;
    uint64_t n_ev32;
    bool sets;  // the call has work for the set tier
};

// Every index a wave follows, checked before the launch.
int push_check(const StreamDev *s, const Push &p) {
    if (p.n_items > (int64_t)1 << 30 || p.n_ev > 0xFFFFFFFFull || p.n_trans > 0xFFFFFFFFull ||
        p.n_mig > (int64_t)1 << 24 || p.n_set > (int64_t)1 << 24 || p.n_ev32 > 0x3FFFFFFFull)
        return lc::fail(LC_E_INVALID, "lc_stream: too much for one call");
    for (int64_t i = 0; i < p.n_mig; ++i) {
        const SetMig &m = p.set->mig[i];
        if (m.key < 0 || m.key >= p.n_keys || !set_slot_ptr(s, m.slot))
            return lc::fail(LC_E_INVALID, "lc_stream: migration %lld is out of range (internal error)", (long long)i);
    }
    for (int64_t i = 0; i < p.n_set; ++i) {
        const SetItem &it = p.set->items[i];
        if (it.key < 0 || it.key >= p.n_keys || !set_slot_ptr(s, it.slot) || it.ev_b > it.ev_e || it.ev_e > p.n_ev32 ||
            it.tr_b > p.n_trans || it.ntr > p.n_trans - it.tr_b)
            return lc::fail(LC_E_INVALID, "lc_stream: set work item %lld is out of range (internal error)", (long long)i);
    }
    for (int64_t i = 0; i < p.n_items; ++i) {
        const Item &it = p.items[i];
        if (it.key < 0 || it.key >= p.n_keys || it.ev_b > it.ev_e || it.ev_e > p.n_ev || it.tr_b > p.n_trans ||
            it.ntr > p.n_trans - it.tr_b)
            return lc::fail(LC_E_INVALID, "lc_stream: work item %lld is out of range (internal error)", (long long)i);
    }
    return LC_OK;
}

// Where a call's pieces lie in the staging block (din / hin, bytes) and its
// two lists in the result block (dout / hout, words): the set tier's list
// follows k_stream's.
struct PushLayout {
    size_t items = 0, trans, ev, mig, desc, set, ev32, in_bytes, out2, out_words;
    explicit PushLayout(const Push &p) {
        trans = up16((size_t)p.n_items * sizeof(Item));
        ev = trans + up16((size_t)p.n_trans * 4);
        mig = ev + up16((size_t)p.n_ev * 2);
        desc = mig + up16((size_t)p.n_mig * sizeof(lcd::StreamMigItem));
        set = desc + up16((size_t)p.n_mig * 64 * 4);
        ev32 = set + up16((size_t)p.n_set * sizeof(lcd::StreamSetItem));
        in_bytes = ev32 + up16((size_t)p.n_ev32 * 4);
        out2 = 1 + 4 * (size_t)p.n_items;
        out_words = out2 + (p.sets ? 1 + 4 * (size_t)p.n_set : 0);
    }
};

// The call's pieces into the pinned staging block, pool slots as pointers.
void push_fill(const StreamDev *s, const Push &p, const PushLayout &l) {
    if (p.n_items) std::memcpy(s->hin + l.items, p.items, (size_t)p.n_items * sizeof(Item));
    if (p.n_trans) std::memcpy(s->hin + l.trans, p.trans, (size_t)p.n_trans * 4);
    if (p.n_ev) std::memcpy(s->hin + l.ev, p.ev16, (size_t)p.n_ev * 2);
    for (int64_t i = 0; i < p.n_mig; ++i) {
        lcd::StreamMigItem m{set_slot_ptr(s, p.set->mig[i].slot), p.set->mig[i].key, (uint32_t)i * 64u};
        std::memcpy(s->hin + l.mig + (size_t)i * sizeof m, &m, sizeof m);
        std::memcpy(s->hin + l.desc + (size_t)i * 64 * 4, p.set->mig[i].descs, 64 * 4);
    }
    for (int64_t i = 0; i < p.n_set; ++i) {
        const SetItem &it = p.set->items[i];
        lcd::StreamSetItem m{set_slot_ptr(s, it.slot), it.key, it.ev_b, it.ev_e, it.tr_b, it.ntr, 0u};
        std::memcpy(s->hin + l.set + (size_t)i * sizeof m, &m, sizeof m);
    }
    if (p.n_ev32) std::memcpy(s->hin + l.ev32, p.set->ev32, (size_t)p.n_ev32 * 4);
}

// The staging block up, the lists' counts zeroed, the launches, and the first
// `head` words of the result block back: all on lane 0, then the host waits.
int push_enqueue(StreamDev *s, Dev *d, const Push &p, const PushLayout &l, size_t head) {
    lcd::StreamArgs a{};
    a.items = (const lcd::StreamItem *)(s->din + l.items);
    a.trans = (const uint32_t *)(s->din + l.trans);
    a.events16 = (const uint16_t *)(s->din + l.ev);
    a.rec = s->rec;
    a.out = s->dout;
    a.n_items = (int32_t)p.n_items;
    a.init_state = p.init_state;
    lcd::StreamSetArgs sa{};
    sa.mig = (const lcd::StreamMigItem *)(s->din + l.mig);
    sa.descs = (const uint32_t *)(s->din + l.desc);
    sa.rec = s->rec;
    sa.items = (const lcd::StreamSetItem *)(s->din + l.set);
    sa.events32 = (const uint32_t *)(s->din + l.ev32);
    sa.trans = a.trans;
    sa.ws = lcd::stream_set_ws_layout();
    sa.ws.base = s->set_ws;
    sa.out = s->dout + l.out2;
    sa.n_mig = (int32_t)p.n_mig;
    sa.n_items = (int32_t)p.n_set;
    sa.init_state = p.init_state;
    HIPCHK(hipEventRecord(s->ev[0], d->stream));
    HIPCHK(hipMemcpyAsync(s->din, s->hin, l.in_bytes, hipMemcpyHostToDevice, d->stream));
    HIPCHK(hipMemsetAsync(s->dout, 0, 4, d->stream));
    if (p.sets) HIPCHK(hipMemsetAsync(s->dout + l.out2, 0, 4, d->stream));
    HIPCHK(hipEventRecord(s->ev[1], d->stream));
    if (p.n_items && s->exact) {
        lcd::StreamExactArgs xa{};
        xa.items = a.items;
        xa.events16 = a.events16;
        xa.trans = a.trans;
        xa.rec = s->rec;
        xa.out = s->dout;
        xa.final_cfg = s->fin;
        xa.n_final = s->nfin;
        xa.budget = s->ctx->o.max_configs;
        xa.n_items = a.n_items;
        xa.init_state = p.init_state;
        xa.max_final = s->ctx->o.max_final;
        HIPCHK(lcd::launch_stream_exact(xa, (int)std::min<int64_t>(p.n_items, 8192), d->stream));
    } else if (p.n_items) {
        HIPCHK(lcd::launch_stream(a, (int)std::min<int64_t>(p.n_items, 8192), d->stream));
    }
    HIPCHK(hipEventRecord(s->ev[2], d->stream));
    // in this order on the one lane: a key's register words, its migration,
    // its set words -- each launch sees what the one before it stored
    if (p.n_mig) HIPCHK(lcd::launch_stream_migrate(sa, (int)std::min<int64_t>(p.n_mig, 8192), d->stream));
    if (p.sets) HIPCHK(hipEventRecord(s->ev[4], d->stream));
    if (p.n_set && s->exact) {  // the exact set tier: the same items, records and workspace
        lcd::StreamSetExactArgs xs{};
        xs.set = sa;
        xs.rec = s->rec;
        xs.final_cfg = s->fin;
        xs.n_final = s->nfin;
        xs.budget = s->ctx->o.max_configs;
        xs.max_final = s->ctx->o.max_final;
        HIPCHK(lcd::launch_stream_set_exact(xs, (int)std::min<int64_t>(p.n_set, s->set_ws_slots), d->stream));
    } else if (p.n_set) {
        HIPCHK(lcd::launch_stream_set(sa, (int)std::min<int64_t>(p.n_set, s->set_ws_slots), d->stream));
    }
    if (p.sets) HIPCHK(hipEventRecord(s->ev[5], d->stream));
    HIPCHK(hipMemcpyAsync(s->hout, s->dout, head * 4, hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipEventRecord(s->ev[3], d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    return LC_OK;
}

// The two lists as the host has them (the rest of a long dead list fetched
// first), merged ascending by key; and the call's device times.
int push_read_lists(StreamDev *s, Dev *d, const Push &p, const PushLayout &l, size_t head, std::vector<Dead> *dead) {
    const size_t n_dead = s->hout[0];
    if (n_dead > (size_t)p.n_items) return lc::fail(LC_E_DEVICE, "lc_stream: the dead list holds more keys than the launch had");
    if (1 + 4 * n_dead > head) {
        HIPCHK(hipMemcpyAsync(s->hout + head, s->dout + head, (1 + 4 * n_dead - head) * 4, hipMemcpyDeviceToHost, d->stream));
        HIPCHK(hipStreamSynchronize(d->stream));
    }
    const size_t n_left = p.sets ? s->hout[l.out2] : 0;
    if (n_left > (size_t)p.n_set) return lc::fail(LC_E_DEVICE, "lc_stream: the set tier's list holds more keys than the launch had");
    (void)hipEventElapsedTime(&s->ms[0], s->ev[0], s->ev[1]);
    (void)hipEventElapsedTime(&s->ms[1], s->ev[1], s->ev[2]);
    (void)hipEventElapsedTime(&s->ms[2], s->ev[p.sets ? 5 : 2], s->ev[3]);
    if (p.sets) {
        (void)hipEventElapsedTime(&s->set_ms[0], s->ev[2], s->ev[4]);
        (void)hipEventElapsedTime(&s->set_ms[1], s->ev[4], s->ev[5]);
    }
    dead->resize(n_dead + n_left);
    for (size_t i = 0; i < n_dead + n_left; ++i) {
        const uint32_t *o = i < n_dead ? s->hout + 1 + 4 * i : s->hout + l.out2 + 1 + 4 * (i - n_dead);
        (*dead)[i] = Dead{o[0], o[1], o[2], o[3]};
    }
    std::sort(dead->begin(), dead->end(), [](const Dead &x, const Dead &y) { return x.key < y.key; });
    return LC_OK;
}

// Exact mode: what the keys that died at an event left in the stream's arrays
// and in their headers.  Few keys die in a call: three small copies each.
int push_read_finals(StreamDev *s, Dev *d, int64_t n_keys, const std::vector<Dead> &dead, std::vector<Final> *fin) {
    fin->assign(dead.size(), Final{});
    const uint32_t mf = (uint32_t)s->ctx->o.max_final;
    bool any = false;
    for (size_t i = 0; i < dead.size(); ++i) {
        const Dead &x = dead[i];
        if ((x.status != lc::STREAM_INVALID && x.status != lc::STREAM_BUDGET) || (int64_t)x.key >= n_keys) continue;
        Final &f = (*fin)[i];
        HIPCHK(hipMemcpyAsync(f.cfg, s->fin + lc::stream_final_off64(x.key, mf, 0), lc::stream_final_words64(mf) * 8,
                              hipMemcpyDeviceToHost, d->stream));
        HIPCHK(hipMemcpyAsync(&f.n_final, s->nfin + x.key, 4, hipMemcpyDeviceToHost, d->stream));
        HIPCHK(hipMemcpyAsync(&f.peak, s->rec + (size_t)x.key * lc::STREAM_REC_WORDS + lc::STREAM_H_PEAK, 4,
                              hipMemcpyDeviceToHost, d->stream));
        any = true;
    }
    if (any) HIPCHK(hipStreamSynchronize(d->stream));
    for (Final &f : *fin) f.n_final = std::min(f.n_final, mf);
    return LC_OK;
}
}  // namespace

int lcst::stream_dev_open(lc_ctx *c, bool exact, StreamDev **out) {
    if (c->n_dev != 1 || c->comm)
        return lc::fail(LC_E_UNSUPPORTED, "lc_stream_open: a stream needs a context of one device and no communicator");
    if (exact && (c->o.max_final < 0 || c->o.max_final > (int32_t)lc::STREAM_MAX_FINAL))
        return lc::fail(LC_E_UNSUPPORTED, "lc_stream_open: max_final %d is past %u", c->o.max_final, lc::STREAM_MAX_FINAL);
    if (!lc::stream_budget_ok(c->o.max_configs, exact))
        return lc::fail(LC_E_UNSUPPORTED, "lc_stream_open: budget %llu is below %llu, where the register tier's sets are exact",
                        (unsigned long long)c->o.max_configs, (unsigned long long)lc::STREAM_MIN_BUDGET);
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(hipSetDevice(c->dev[0]->device));
    StreamDev *s = new StreamDev;
    s->ctx = c;
    s->exact = exact;
    hipEvent_t *const evs[] = {&s->ev[0], &s->ev[1], &s->ev[2], &s->ev[3], &s->ev[4], &s->ev[5], &s->fev[0], &s->fev[1]};
    for (hipEvent_t *e : evs) {
        hipError_t r = hipEventCreate(e);
        if (r != hipSuccess) {
            for (hipEvent_t &x : s->ev)
                if (x) (void)hipEventDestroy(x);
            for (hipEvent_t &x : s->fev)
                if (x) (void)hipEventDestroy(x);
            delete s;
            return lc::fail(LC_E_DEVICE, "lc_stream_open: hipEventCreate failed: %s", hipGetErrorString(r));
        }
    }
    *out = s;
    return LC_OK;
}

void lcst::stream_dev_close(StreamDev *s) {
    if (!s) return;
    std::lock_guard<std::mutex> g(s->ctx->mu);
    Dev *d = s->ctx->dev[0];
    (void)hipSetDevice(d->device);
    (void)hipStreamSynchronize(d->stream);
    dfree(s->rec);
    dfree(s->fin);
    dfree(s->nfin);
    dfree(s->dout);
    for (uint32_t *&c : s->set_chunk) dfree(c);
    if (s->set_ws) (void)hipFree(s->set_ws);
    if (s->din) (void)hipFree(s->din);
    if (s->hin) (void)hipHostFree(s->hin);
    if (s->hout) (void)hipHostFree(s->hout);
    for (hipEvent_t e : s->ev)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : s->fev)
        if (e) (void)hipEventDestroy(e);
    delete s;
}

int lcst::stream_dev_max_final(const StreamDev *s) { return s->ctx->o.max_final; }
double lcst::stream_dev_final_ms(const StreamDev *s) { return s->final_ms; }

int lcst::stream_dev_peaks(StreamDev *s, int64_t n_keys, uint32_t *out) {
    if (!s->exact) return lc::fail(LC_E_INVALID, "lc_stream: peaks are kept in exact mode only");
    CtxCall x(s->ctx);
    LCCHK(x.enter());
    const int64_t have = std::min(n_keys, s->rec_cap);  // keys past the records have searched nothing yet
    if (have > 0) {
        HIPCHK(hipMemcpy2DAsync(out, 4, s->rec + lc::STREAM_H_PEAK, (size_t)lc::STREAM_REC_WORDS * 4, 4, (size_t)have,
                                hipMemcpyDeviceToHost, x.d->stream));
        HIPCHK(hipStreamSynchronize(x.d->stream));
    }
    for (int64_t i = 0; i < n_keys; ++i) out[i] = i < have && out[i] ? out[i] : 1u;
    return LC_OK;
}

int lcst::stream_dev_finals(StreamDev *s, int64_t n_keys, const int32_t *keys, int64_t n_live, uint32_t init_state,
                            uint64_t *cfg, uint32_t *n_final, const SetLive *set_live, int64_t n_set_live) {
    if (!s->exact) return lc::fail(LC_E_INVALID, "lc_stream: final configs are kept in exact mode only");
    s->final_ms = 0;
    if (n_keys <= 0) return LC_OK;
    for (int64_t i = 0; i < n_live; ++i)
        if (keys[i] < 0 || keys[i] >= n_keys)
            return lc::fail(LC_E_INVALID, "lc_stream: live key %lld is out of range (internal error)", (long long)i);
    for (int64_t i = 0; i < n_set_live; ++i)
        if (set_live[i].key < 0 || set_live[i].key >= n_keys || !set_slot_ptr(s, set_live[i].slot))
            return lc::fail(LC_E_INVALID, "lc_stream: live set-tier key %lld is out of range (internal error)", (long long)i);
    CtxCall x(s->ctx);
    LCCHK(x.enter());
    const size_t set_off = up16((size_t)std::max<int64_t>(n_live, 0) * 4);
    LCCHK(stream_grow(s, x.d, n_keys, set_off + (size_t)std::max<int64_t>(n_set_live, 0) * sizeof(lcd::StreamSetItem), 0));
    const uint32_t mf = (uint32_t)s->ctx->o.max_final;
    if (n_set_live > 0) {  // the set tier's live keys: one workgroup each, before the copies back
        for (int64_t i = 0; i < n_set_live; ++i) {
            lcd::StreamSetItem m{set_slot_ptr(s, set_live[i].slot), set_live[i].key, 0u, 0u, 0u, 0u, 0u};
            std::memcpy(s->hin + set_off + (size_t)i * sizeof m, &m, sizeof m);
        }
        lcd::StreamSetExactArgs xs{};
        xs.set.items = (const lcd::StreamSetItem *)(s->din + set_off);
        xs.set.n_items = (int32_t)std::min<int64_t>(n_set_live, (int64_t)1 << 24);
        xs.rec = s->rec;
        xs.final_cfg = s->fin;
        xs.n_final = s->nfin;
        xs.budget = s->ctx->o.max_configs;
        xs.max_final = (int32_t)mf;
        HIPCHK(hipMemcpyAsync(s->din + set_off, s->hin + set_off, (size_t)n_set_live * sizeof(lcd::StreamSetItem),
                              hipMemcpyHostToDevice, x.d->stream));
        HIPCHK(lcd::launch_stream_set_final(xs, (int)std::min<int64_t>(n_set_live, 8192), x.d->stream));
    }
    if (n_live > 0) {
        std::memcpy(s->hin, keys, (size_t)n_live * 4);
        lcd::StreamExactArgs a{};
        a.keys = (const int32_t *)s->din;
        a.rec = s->rec;
        a.final_cfg = s->fin;
        a.n_final = s->nfin;
        a.n_items = (int32_t)std::min<int64_t>(n_live, (int64_t)1 << 30);
        a.init_state = init_state;
        a.max_final = (int32_t)mf;
        HIPCHK(hipMemcpyAsync(s->din, s->hin, (size_t)n_live * 4, hipMemcpyHostToDevice, x.d->stream));
        HIPCHK(hipEventRecord(s->fev[0], x.d->stream));
        HIPCHK(lcd::launch_stream_final(a, (int)std::min<int64_t>(n_live, 8192), x.d->stream));
        HIPCHK(hipEventRecord(s->fev[1], x.d->stream));
    }
    const size_t bf = (size_t)lc::stream_final_bytes((uint64_t)n_keys, mf), bn = (size_t)lc::stream_nfinal_bytes((uint64_t)n_keys);
    if (bf) HIPCHK(hipMemcpyAsync(cfg, s->fin, bf, hipMemcpyDeviceToHost, x.d->stream));
    HIPCHK(hipMemcpyAsync(n_final, s->nfin, bn, hipMemcpyDeviceToHost, x.d->stream));
    HIPCHK(hipStreamSynchronize(x.d->stream));
    if (n_live > 0) (void)hipEventElapsedTime(&s->final_ms, s->fev[0], s->fev[1]);
    for (int64_t i = 0; i < n_keys; ++i) n_final[i] = std::min(n_final[i], mf);
    return LC_OK;
}

void lcst::stream_dev_timing(const StreamDev *s, double *out3) {
    for (int i = 0; i < 3; ++i) out3[i] = s->ms[i];
}

int lcst::stream_dev_set_alloc(StreamDev *s, int32_t *slot) {
    std::lock_guard<std::mutex> g(s->ctx->mu);
    if (s->set_free.empty()) {
        if (s->set_slots > ((int64_t)1 << 20)) return lc::fail(LC_E_DEVICE, "lc_stream: the set-record pool is full");
        HIPCHK(hipSetDevice(s->ctx->dev[0]->device));
        const int64_t n = SET_CHUNK0 << s->set_chunk.size();
        uint32_t *c = nullptr;
        HIPCHK(dalloc(&c, (size_t)n * lc::STREAM_SET_REC_WORDS));
        s->set_chunk.push_back(c);
        for (int64_t i = n; i-- > 0;) s->set_free.push_back((int32_t)(s->set_slots + i));
        s->set_slots += n;
    }
    *slot = s->set_free.back();
    s->set_free.pop_back();
    s->set_peak = std::max(s->set_peak, ++s->set_used);
    return LC_OK;
}

void lcst::stream_dev_set_free(StreamDev *s, int32_t slot) {
    std::lock_guard<std::mutex> g(s->ctx->mu);
    if (slot < 0 || slot >= s->set_slots) return;
    s->set_free.push_back(slot);
    --s->set_used;
}

void lcst::stream_dev_set_stats(const StreamDev *s, double *out6) {
    out6[0] = s->set_ms[0];
    out6[1] = s->set_ms[1];
    out6[2] = (double)s->set_slots;
    out6[3] = (double)s->set_used;
    out6[4] = (double)s->set_peak;
    out6[5] = (double)lc::stream_set_slot_bytes();
}

int lcst::stream_dev_set_record(StreamDev *s, int32_t slot, int64_t off, uint32_t *out, int64_t words) {
    CtxCall x(s->ctx);
    const uint32_t *p = set_slot_ptr(s, slot);
    if (!p || off < 0 || words < 0 || off + words > (int64_t)lc::STREAM_SET_REC_WORDS)
        return lc::fail(LC_E_INVALID, "lc_stream_set_record: no such record");
    if (!words) return LC_OK;
    LCCHK(x.enter());
    HIPCHK(hipMemcpyAsync(out, p + off, (size_t)words * 4, hipMemcpyDeviceToHost, x.d->stream));
    HIPCHK(hipStreamSynchronize(x.d->stream));
    return LC_OK;
}

int lcst::stream_dev_record(StreamDev *s, int64_t key, uint32_t *out) {
    CtxCall x(s->ctx);
    if (key < 0 || key >= s->rec_cap) return lc::fail(LC_E_INVALID, "lc_stream_record: key %lld has no record", (long long)key);
    LCCHK(x.enter());
    HIPCHK(hipMemcpyAsync(out, s->rec + (size_t)key * lc::STREAM_REC_WORDS, lc::STREAM_REC_WORDS * 4, hipMemcpyDeviceToHost,
                          x.d->stream));
    HIPCHK(hipStreamSynchronize(x.d->stream));
    return LC_OK;
}

int lcst::stream_dev_push(StreamDev *s, int64_t n_keys, const Item *items, int64_t n_items, const uint16_t *ev16,
                          uint64_t n_ev, const uint32_t *trans, uint64_t n_trans, uint32_t init_state,
                          std::vector<Dead> *dead, const SetWork *set, std::vector<Final> *fin) {
    dead->clear();
    if (fin) fin->clear();
    s->ms[0] = s->ms[1] = s->ms[2] = 0;
    s->set_ms[0] = s->set_ms[1] = 0;
    Push p{n_keys, std::max<int64_t>(n_items, 0), items, ev16, trans, n_ev, n_trans, init_state, set};
    p.n_mig = set ? set->n_mig : 0;
    p.n_set = set ? set->n_items : 0;
    p.n_ev32 = set ? set->n_ev32 : 0;
    p.sets = p.n_mig > 0 || p.n_set > 0;
    if (p.n_items <= 0 && !p.sets) return LC_OK;
    LCCHK(push_check(s, p));
    CtxCall x(s->ctx);
    LCCHK(x.enter());
    const PushLayout l(p);
    LCCHK(stream_grow(s, x.d, n_keys, l.in_bytes, l.out_words));
    if (p.n_set) LCCHK(set_ws_grow(s, x.d, (int)std::min<int64_t>(p.n_set, SET_GRID)));
    push_fill(s, p, l);
    const size_t head = p.sets ? l.out_words : std::min<size_t>(l.out_words, 1 + 4 * STREAM_OUT_HEAD);
    LCCHK(push_enqueue(s, x.d, p, l, head));
    LCCHK(push_read_lists(s, x.d, p, l, head, dead));
    if (s->exact && fin) LCCHK(push_read_finals(s, x.d, n_keys, *dead, fin));
    return LC_OK;
}
