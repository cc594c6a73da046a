// host_counter_stream.cpp -- lc_counter_stream_*: the packer of a streaming
// checker/counter, its entry points and the host stream's fold
// (include/lincheck_counter_stream.h has the contract).
// Single-threaded, as host_queue_stream.cpp.  No HIP here.
//
// The packer is serial and incremental: it keeps the open invocation of every
// (key, process) between appends and never the events.  An append is taken in
// two steps, so that a refused one leaves the stream as it was:
//   look     codes, columns, keyedness and the size rules of
//            counter_stream_plan.hpp, from counts of the append's rows alone;
//            with a device the reads array is grown here, the last step that
//            may refuse
//   fold     row by row (host_counter.cpp's pairing).  Per touched key the
//            append's events; an invocation that completes within the append
//            is resolved in place, as the one-shot pack resolves it (a failed
//            pair is dropped, an :ok's value replaces its invocation's).  A
//            completion of an invocation of an EARLIER append becomes a patch
//            (key, r0, delta).  Then the chunk (device_counter_stream.hpp)
//            and the fold of it: the device half, or HostFold below.
// The :unknown bookkeeping is the packer's: per key a permanent flag, the
// count of surviving bad invocations (counted as 0 in the sums) and the
// surviving sum in 128 bits.  Only `upper` is ever revised: `lower` moves at
// :ok :add rows, which change nothing behind them.
//
// A read's slot holds the `lower` stored at its :invoke until its :ok.  Slots
// are reused, but one freed in an append is handed out again only in the next:
// the device judges an append's reads after all of its events.

#include <algorithm>
#include <chrono>
#include <cstring>
#include <numeric>
#include <string>
#include <unordered_map>
#include <vector>

#include "common.hpp"
#include "counter_plan.hpp"
#include "counter_stream_plan.hpp"
#include "device_counter_stream.hpp"

namespace {

using lccs::CsChunk;
using lccs::CS_NO_READS;
typedef unsigned __int128 u128;

constexpr uint8_t GONE = 0xFF;
constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr uint8_t BAD_NIL = 1, BAD_NEG = 2;

const char *const E_SECOND = "a second invocation by a process that has one open";
const char *const E_ORPHAN = "a completion by a process with no open invocation";
const char *const E_OTHER_F = "a completion whose :f is not its invocation's";
const char *const E_READ = "an :ok :read whose value is nil or not an integer";
const char *const E_NIL = "an :add whose value is nil or not an integer";
const char *const E_NEG = "an :add of a negative value";
const char *const E_SUM = "the adds sum past the largest 64-bit integer";

struct Open {
    uint8_t f = 0, bad = 0;
    uint64_t app = 0;     // the append that holds the invocation
    uint32_t ev = 0;      // its event in the key's list, while that append lasts
    uint32_t at = 0;      // an add: r0, the reads resident at its invocation; a read: its slot
    int64_t counted = 0;  // an add: its value as the sums hold it (0 for a bad one)
};

struct Ev {
    uint8_t kind;
    uint32_t aux;
    int64_t val;
};

struct Key {
    std::unordered_map<int64_t, Open> open;
    const char *dead = nullptr;  // a permanent error
    uint64_t n_nil = 0, n_neg = 0;
    u128 sum = 0;
    uint64_t n_reads = 0, n_errors = 0;
    int8_t valid = LC_VALID;
    uint64_t seen_in = 0, touch_in = 0, look_in = 0;  // the appends that last put it on those lists
    std::vector<Ev> cur;
    const char *error() const {
        if (dead) return dead;
        if (n_nil) return E_NIL;
        if (n_neg) return E_NEG;
        if (sum > (u128)INT64_MAX) return E_SUM;
        return nullptr;
    }
};

struct Patch {
    uint32_t key, r0;
    int64_t delta;
};

inline bool out_of_bounds(int64_t lo, int64_t v, int64_t up) { return !(lo <= v && v <= up); }

// The host stream's resident state and its fold of a chunk: what the kernels
// do, in history order on one thread.
struct HostFold {
    std::vector<uint64_t> key_lo, key_up, n_err, slot_lo;
    std::vector<uint32_t> rd_key, rd_rank;
    std::vector<int64_t> rd_lower, rd_val, rd_upper;
    std::vector<uint8_t> rd_flag;

    void append(const CsChunk &c, uint64_t *n_errors) {
        if (key_lo.size() < c.n_keys) {
            key_lo.resize(c.n_keys, 0); key_up.resize(c.n_keys, 0); n_err.resize(c.n_keys, 0);
        }
        if (slot_lo.size() < c.n_slots) slot_lo.resize(c.n_slots, 0);
        const uint64_t R0 = c.reads_before;
        for (uint64_t r = c.n_patch ? c.min_r0 : R0; r < R0; ++r) {
            const uint32_t k = rd_key[r];
            // the last patch with (key, r0) <= (k, r)
            uint64_t lo = 0, hi = c.n_patch;
            while (lo < hi) {
                const uint64_t m = (lo + hi) / 2;
                if (c.p_key[m] < k || (c.p_key[m] == k && c.p_r0[m] <= r)) lo = m + 1;
                else hi = m;
            }
            if (lo == 0 || c.p_key[lo - 1] != k) continue;
            rd_upper[r] = (int64_t)((uint64_t)rd_upper[r] + (uint64_t)c.p_acc[lo - 1]);
            const uint8_t fl = out_of_bounds(rd_lower[r], rd_val[r], rd_upper[r]);
            if (fl != rd_flag[r]) n_err[k] += fl ? 1 : ~0ull;
            rd_flag[r] = fl;
        }
        for (uint64_t p = 0; p < c.n_patch; ++p)
            if (p + 1 == c.n_patch || c.p_key[p + 1] != c.p_key[p]) key_up[c.p_key[p]] += (uint64_t)c.p_acc[p];
        const size_t R1 = (size_t)(R0 + c.n_reads);
        rd_key.resize(R1); rd_rank.resize(R1); rd_lower.resize(R1); rd_val.resize(R1); rd_upper.resize(R1); rd_flag.resize(R1);
        for (uint64_t i = 0; i < c.n_reads; ++i) {
            rd_key[R0 + i] = c.rd_key[i]; rd_rank[R0 + i] = c.rd_rank[i]; rd_val[R0 + i] = c.rd_val[i];
            rd_lower[R0 + i] = 0; rd_upper[R0 + i] = 0; rd_flag[R0 + i] = 0;
        }
        for (uint64_t e = 0; e < c.n_events; ++e) {
            const uint32_t k = c.seg_key[c.ev_seg[e]];
            switch (c.ev_kind[e]) {
                case LC_CE_UP: key_up[k] += (uint64_t)c.ev_val[e]; break;
                case LC_CE_LOW: key_lo[k] += (uint64_t)c.ev_val[e]; break;
                case LC_CE_RINV: slot_lo[c.ev_aux[e]] = key_lo[k]; break;
                default: {
                    const uint64_t r = R0 + (uint64_t)c.ev_val[e];
                    rd_lower[r] = (int64_t)slot_lo[c.ev_aux[e]];
                    rd_upper[r] = (int64_t)key_up[k];
                    rd_flag[r] = out_of_bounds(rd_lower[r], rd_val[r], rd_upper[r]);
                    n_err[k] += rd_flag[r];
                }
            }
        }
        for (uint64_t i = 0; i < c.n_look; ++i) n_errors[i] = n_err[c.look[i]];
    }

    void results(const uint64_t *read_off, uint64_t total, int64_t *lower, int64_t *upper, int64_t *value, uint8_t *flag) const {
        for (size_t r = 0; r < rd_key.size(); ++r) {
            const uint64_t off = read_off[rd_key[r]];
            if (off == CS_NO_READS) continue;
            const uint64_t at = off + rd_rank[r];
            if (at >= total) continue;
            lower[at] = rd_lower[r]; upper[at] = rd_upper[r]; flag[at] = rd_flag[r];
            if (value) value[at] = rd_val[r];
        }
    }
};

}  // namespace

struct lc_counter_stream {
    lc_ctx *ctx = nullptr;
    lccs::CsDev *dev = nullptr;
    HostFold *host = nullptr;
    uint32_t tile = 0;
    uint64_t launch_events = 0;
    int keyed = -1;       // -1: no client row yet
    bool broken = false;  // a device step failed half way
    int64_t rows = 0;
    uint64_t reads = 0, events = 0, cap = 0, appends = 0, n_slots = 0;
    std::vector<int64_t> keys;
    std::unordered_map<int64_t, uint32_t> ids;
    std::vector<Key> key;
    std::vector<uint32_t> free_slots, freed_now;
    std::vector<int64_t> changed;
    // the current append
    std::vector<uint32_t> seen, touched;
    std::vector<Patch> patches;
    lc::pinned_vector<uint8_t> ev_kind;
    lc::pinned_vector<uint32_t> ev_seg, ev_aux, seg_key, rd_key, rd_rank, rd_slot, p_key, p_r0, look;
    lc::pinned_vector<int64_t> ev_val, rd_val, p_acc;
    std::vector<uint64_t> look_err;
    double ms[6] = {0, 0, 0, 0, 0, 0};
};

namespace {

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

uint32_t add_key(lc_counter_stream *s, int64_t k) {
    const uint32_t id = (uint32_t)s->keys.size();
    s->ids.emplace(k, id);
    s->keys.push_back(k);
    s->key.emplace_back();
    return id;
}

int8_t valid_of(const Key &k) {
    if (k.error()) return LC_UNKNOWN;
    return k.n_errors ? LC_INVALID : LC_VALID;
}

// Refusals: nothing of the stream has changed when one fires.
int refuse(const lc_counter_stream *s, const lc_counter_history *h, int *kind, uint64_t *ok_reads) {
    const int64_t n = h->n;
    if (n < 0) return lc::fail(LC_E_INVALID, "lc_counter_stream_append: n < 0");
    if (n > 0 && (!h->type || !h->f || !h->value)) return lc::fail(LC_E_INVALID, "lc_counter_stream_append: null column");
    bool has_key = false;
    uint64_t client = 0, oks = 0;
    for (int64_t r = 0; r < n; ++r) {
        if (h->type[r] > LC_INFO || h->f[r] > LC_CF_OTHER)
            return lc::fail(LC_E_INVALID, "lc_counter_stream_append: row %lld: bad :type / :f code", (long long)r);
        client += h->f[r] != LC_CF_OTHER;
        oks += h->f[r] == LC_CF_READ && h->type[r] == LC_OK_T;
        has_key |= h->key && h->key[r] != LC_NO_KEY;
    }
    *kind = has_key ? 1 : client ? 0 : -1;
    *ok_reads = oks;
    if (*kind >= 0 && s->keyed >= 0 && *kind != s->keyed)
        return lc::fail(LC_E_INVALID, "lc_counter_stream_append: %s rows appended to a stream of %s rows", *kind ? "keyed" : "unkeyed",
                        s->keyed ? "keyed" : "unkeyed");
    if (const int why = lccs::csp_refuses(s->reads, s->events, oks, client))
        return lc::fail(LC_E_UNSUPPORTED, "lc_counter_stream_append: the stream's %s stay below 2^32", why == 1 ? "reads" : "events");
    return LC_OK;
}

uint32_t take_slot(lc_counter_stream *s) {
    if (!s->free_slots.empty()) {
        const uint32_t x = s->free_slots.back();
        s->free_slots.pop_back();
        return x;
    }
    return (uint32_t)s->n_slots++;
}

struct Fold {
    lc_counter_stream *s;
    uint64_t patched = 0;

    uint32_t push(Key &k, uint8_t kind, uint32_t aux, int64_t v) {
        k.cur.push_back(Ev{kind, aux, v});
        return (uint32_t)(k.cur.size() - 1);
    }

    void row(uint32_t ki, uint8_t t, uint8_t f, int64_t proc, int64_t v) {
        Key &k = s->key[ki];
        if (t == LC_INVOKE) {
            if (k.open.count(proc)) { k.dead = E_SECOND; return; }
            Open o;
            o.f = f; o.app = s->appends;
            if (f == LC_CF_ADD) {
                o.bad = v == LC_NIL ? BAD_NIL : v < 0 ? BAD_NEG : 0;
                o.counted = o.bad ? 0 : v;
                o.at = (uint32_t)(s->reads + s->rd_key.size());
                o.ev = push(k, LC_CE_UP, 0, o.counted);
                if (o.bad == BAD_NIL) ++k.n_nil;
                else if (o.bad == BAD_NEG) ++k.n_neg;
                else k.sum += (u128)(uint64_t)v;
            } else {
                o.at = take_slot(s);
                o.ev = push(k, LC_CE_RINV, o.at, 0);
            }
            k.open.emplace(proc, o);
            return;
        }
        auto it = k.open.find(proc);
        if (it == k.open.end()) { k.dead = E_ORPHAN; return; }
        const Open o = it->second;
        if (o.f != f) { k.dead = E_OTHER_F; return; }
        k.open.erase(it);
        const bool mine = o.app == s->appends;
        if (f == LC_CF_READ) {
            s->freed_now.push_back(o.at);
            if (t != LC_OK_T) return;
            if (v == LC_NIL) { k.dead = E_READ; return; }
            push(k, LC_CE_ROK, o.at, (int64_t)s->rd_key.size());
            s->rd_key.push_back(ki); s->rd_rank.push_back((uint32_t)k.n_reads++); s->rd_slot.push_back(o.at); s->rd_val.push_back(v);
            return;
        }
        if (t == LC_INFO) return;  // the invocation stays as it stands
        if (t == LC_OK_T && (v == LC_NIL || v < 0)) { k.dead = v == LC_NIL ? E_NIL : E_NEG; return; }
        // the invocation leaves the sums (:fail) or takes the :ok's value
        const int64_t now = t == LC_OK_T ? v : 0;
        if (o.bad == BAD_NIL) --k.n_nil;
        else if (o.bad == BAD_NEG) --k.n_neg;
        k.sum = k.sum - (u128)(uint64_t)o.counted + (u128)(uint64_t)now;
        if (mine) {
            if (t == LC_OK_T) k.cur[o.ev].val = v;
            else k.cur[o.ev].kind = GONE;
        } else {
            ++patched;
            if (now != o.counted) s->patches.push_back(Patch{ki, o.at, (int64_t)((uint64_t)now - (uint64_t)o.counted)});
        }
        if (t == LC_OK_T) push(k, LC_CE_LOW, 0, v);
    }
};

int append(lc_counter_stream *s, const lc_counter_history *h, lc_counter_stream_update *u) {
    const auto t0 = std::chrono::steady_clock::now();
    if (s->broken) return lc::fail(LC_E_INVALID, "lc_counter_stream_append: an earlier append failed on the device; close the stream");
    int kind = -1;
    uint64_t ok_reads = 0;
    if (int rc = refuse(s, h, &kind, &ok_reads)) return rc;
    const int64_t n = h->n;
    bool grew = false;
    double grow_ms = 0;
    if (s->reads + ok_reads > s->cap) {
        const uint64_t to = lccs::csp_reads_cap(s->cap, s->reads + ok_reads);
        if (to == lccs::CSP_BAD)
            return lc::fail(LC_E_NOMEM, "lc_counter_stream_append: %llu reads beside %llu resident need more than the reads array's cap of %llu bytes",
                            (unsigned long long)ok_reads, (unsigned long long)s->reads, (unsigned long long)lccs::CSP_MAX_BYTES);
        if (s->dev)
            if (int rc = lccs::cs_dev_reserve(s->dev, to, s->reads, &grow_ms)) {
                if (rc != LC_E_NOMEM) s->broken = true;
                return rc;
            }
        s->cap = to;
        grew = true;
    }

    // ---- fold: from here on nothing refuses
    s->broken = true;  // (an exception half way leaves the packer between two states)
    if (s->keyed < 0 && kind == 1) {  // the placeholder LC_NO_KEY, which nothing has touched
        s->keys.clear(); s->ids.clear(); s->key.clear();
    }
    if (s->keyed < 0) s->keyed = kind;
    ++s->appends;
    s->seen.clear(); s->touched.clear(); s->patches.clear(); s->freed_now.clear();
    s->rd_key.clear(); s->rd_rank.clear(); s->rd_slot.clear(); s->rd_val.clear();
    const uint64_t reads_before = s->reads;
    Fold fold{s};
    const bool keyed = s->keyed == 1;
    int64_t last = LC_NO_KEY;
    uint32_t last_i = keyed ? NONE : 0;
    for (int64_t r = 0; r < n; ++r) {
        if (keyed) {
            const int64_t k = h->key ? h->key[r] : LC_NO_KEY;
            if (k != last) {
                last = k;
                if (k == LC_NO_KEY) {
                    last_i = NONE;
                } else {
                    auto it = s->ids.find(k);
                    if (it == s->ids.end()) {
                        if (s->keys.size() >= 0x7FFFFFF0u) return lc::fail(LC_E_INVALID, "lc_counter_stream_append: more than 2^31 keys");
                        last_i = add_key(s, k);
                    } else {
                        last_i = it->second;
                    }
                }
            }
        }
        const uint32_t ki = last_i;
        if (ki == NONE || s->keyed < 0) continue;
        Key &k = s->key[ki];
        if (k.seen_in != s->appends) {
            k.seen_in = s->appends;
            s->seen.push_back(ki);
        }
        if (k.dead || h->f[r] == LC_CF_OTHER) continue;
        const int64_t proc = h->process ? h->process[r] : 0;
        if (proc == LC_NO_PROCESS) continue;
        if (k.touch_in != s->appends) {
            k.touch_in = s->appends;
            s->touched.push_back(ki);
        }
        fold.row(ki, h->type[r], h->f[r], proc, h->value[r]);
    }

    // ---- the chunk
    s->ev_kind.clear(); s->ev_seg.clear(); s->ev_aux.clear(); s->ev_val.clear(); s->seg_key.clear();
    for (uint32_t ki : s->touched) {
        Key &k = s->key[ki];
        if (!k.dead) {
            const uint32_t seg = (uint32_t)s->seg_key.size();
            bool any = false;
            for (const Ev &e : k.cur) {
                if (e.kind == GONE) continue;
                s->ev_kind.push_back(e.kind); s->ev_seg.push_back(seg); s->ev_aux.push_back(e.aux); s->ev_val.push_back(e.val);
                any = true;
            }
            if (any) s->seg_key.push_back(ki);
        }
        k.cur.clear();
    }
    // patches of keys that live, by (key, r0), the deltas accumulated within the key
    s->patches.erase(std::remove_if(s->patches.begin(), s->patches.end(), [&](const Patch &p) { return s->key[p.key].dead != nullptr; }),
                     s->patches.end());
    std::sort(s->patches.begin(), s->patches.end(), [](const Patch &a, const Patch &b) { return a.key != b.key ? a.key < b.key : a.r0 < b.r0; });
    const size_t P = s->patches.size();
    s->p_key.resize(P); s->p_r0.resize(P); s->p_acc.resize(P);
    uint64_t min_r0 = reads_before, acc = 0;
    for (size_t i = 0; i < P; ++i) {
        const Patch &p = s->patches[i];
        acc = i && s->patches[i - 1].key == p.key ? acc + (uint64_t)p.delta : (uint64_t)p.delta;
        s->p_key[i] = p.key; s->p_r0[i] = p.r0; s->p_acc[i] = (int64_t)acc;
        min_r0 = std::min<uint64_t>(min_r0, p.r0);
    }
    // the keys whose n_errors may move: those with patches or reads
    s->look.clear();
    auto look_at = [&](uint32_t ki) {
        Key &k = s->key[ki];
        if (k.dead || k.look_in == s->appends) return;
        k.look_in = s->appends;
        s->look.push_back(ki);
    };
    for (size_t i = 0; i < P; ++i) look_at(s->p_key[i]);
    for (uint32_t ki : s->rd_key) look_at(ki);
    s->look_err.assign(s->look.size(), 0);

    CsChunk c;
    c.n_events = s->ev_kind.size();
    c.ev_kind = s->ev_kind.data(); c.ev_seg = s->ev_seg.data(); c.ev_aux = s->ev_aux.data(); c.ev_val = s->ev_val.data();
    c.n_seg = s->seg_key.size(); c.seg_key = s->seg_key.data();
    c.n_reads = s->rd_key.size();
    c.rd_key = s->rd_key.data(); c.rd_rank = s->rd_rank.data(); c.rd_slot = s->rd_slot.data(); c.rd_val = s->rd_val.data();
    c.n_patch = P; c.min_r0 = min_r0;
    c.p_key = s->p_key.data(); c.p_r0 = s->p_r0.data(); c.p_acc = s->p_acc.data();
    c.n_look = s->look.size(); c.look = s->look.data();
    c.n_keys = s->keys.size(); c.n_slots = s->n_slots; c.reads_before = reads_before;

    s->rows += n;
    s->reads += c.n_reads;
    s->events += c.n_events;
    s->free_slots.insert(s->free_slots.end(), s->freed_now.begin(), s->freed_now.end());
    std::fill(s->ms, s->ms + 6, 0.0);
    s->ms[0] = ms_since(t0);
    s->ms[4] = grow_ms;
    if (s->dev) {
        if (c.n_events || c.n_patch || c.n_reads)
            if (int rc = lccs::cs_dev_append(s->dev, &c, s->look_err.data(), s->ms + 1)) return rc;
    } else {
        const auto t1 = std::chrono::steady_clock::now();
        s->host->append(c, s->look_err.data());
        s->ms[2] = ms_since(t1);
    }
    for (size_t i = 0; i < s->look.size(); ++i) s->key[s->look[i]].n_errors = s->look_err[i];
    s->changed.clear();
    for (uint32_t ki : s->seen) {
        Key &k = s->key[ki];
        const int8_t v = valid_of(k);
        if (v != k.valid) s->changed.push_back((int64_t)ki);
        k.valid = v;
    }
    std::sort(s->changed.begin(), s->changed.end());
    s->broken = false;
    s->ms[5] = ms_since(t0);
    if (u) {
        u->n_keys = (int64_t)s->keys.size();
        u->rows = s->rows;
        u->events = (int64_t)c.n_events;
        u->reads = (int64_t)c.n_reads;
        u->reads_total = (int64_t)s->reads;
        u->patched = (int64_t)fold.patched;
        u->revisited = P ? (int64_t)(reads_before - min_r0) : 0;
        u->grew = grew;
        u->n_changed = (int64_t)s->changed.size();
        u->changed = s->changed.data();
    }
    return LC_OK;
}

void counts(const lc_counter_stream *s, int8_t *valid, uint64_t *n_errors, uint64_t *n_reads) {
    for (size_t k = 0; k < s->key.size(); ++k) {
        const Key &a = s->key[k];
        const bool ok = a.valid != LC_UNKNOWN;
        valid[k] = a.valid;
        n_errors[k] = ok ? a.n_errors : 0;
        n_reads[k] = ok ? a.n_reads : 0;
    }
}

int results(lc_counter_stream *s, lc_counter_result *r, int64_t *value) {
    const size_t K = s->key.size();
    if (!r->valid || !r->n_errors || !r->err_off || (r->err_cap && !r->err_idx))
        return lc::fail(LC_E_INVALID, "lc_counter_stream_results: null result array");
    std::vector<uint64_t> n_reads(K), off(K);
    counts(s, r->valid, r->n_errors, n_reads.data());
    uint64_t R = 0, n_err = 0;
    for (size_t k = 0; k < K; ++k) {
        off[k] = r->valid[k] == LC_UNKNOWN ? CS_NO_READS : R;
        R += n_reads[k];
        r->err_off[k] = n_err;
        n_err += r->n_errors[k];
    }
    r->err_off[K] = n_err;
    r->n_err = n_err;
    if (R && (!r->lower || !r->upper)) return lc::fail(LC_E_INVALID, "lc_counter_stream_results: null result array");
    std::vector<uint8_t> flag((size_t)R, 0);
    if (R) {
        if (s->dev) {
            if (int rc = lccs::cs_dev_results(s->dev, off.data(), K, s->reads, R, r->lower, r->upper, value, flag.data())) return rc;
        } else {
            s->host->results(off.data(), R, r->lower, r->upper, value, flag.data());
        }
    }
    if (n_err > r->err_cap)
        return lc::fail(LC_E_NOMEM, "lc_counter_stream_results: err_cap %llu, %llu needed", (unsigned long long)r->err_cap,
                        (unsigned long long)n_err);
    uint64_t at = 0;
    for (uint64_t i = 0; i < R && at < n_err; ++i)
        if (flag[(size_t)i]) r->err_idx[at++] = i;
    if (at != n_err) return lc::fail(LC_E_DEVICE, "lc_counter_stream_results: %llu flagged reads, %llu counted", (unsigned long long)at,
                                     (unsigned long long)n_err);
    return LC_OK;
}

template <class F>
int guarded(const char *who, F &&f) {
    try {
        return f();
    } catch (const std::bad_alloc &) {
        return lc::fail(LC_E_NOMEM, "%s: out of memory", who);
    } catch (const std::exception &e) {
        return lc::fail(LC_E_NOMEM, "%s: %s", who, e.what());
    }
}

}  // namespace

extern "C" int lc_counter_stream_open(lc_ctx *ctx, const lc_counter_stream_opts *o, lc_counter_stream **out) {
    if (!out) return lc::fail(LC_E_INVALID, "lc_counter_stream_open: null out");
    *out = nullptr;
    if (o && o->flags) return lc::fail(LC_E_INVALID, "lc_counter_stream_open: unknown flags 0x%x", o->flags);
    const uint32_t tile = lcc::ct_tile_of(o ? o->tile : 0);
    if (!tile) return lc::fail(LC_E_INVALID, "lc_counter_stream_open: tile %u (256 or 2,048)", o->tile);
    const uint64_t cap = lccs::csp_first_reads(o ? o->reads : 0);
    if (cap == lccs::CSP_BAD) return lc::fail(LC_E_INVALID, "lc_counter_stream_open: reads %u pass the reads array's byte cap", o->reads);
    return guarded("lc_counter_stream_open", [&]() -> int {
        lc_counter_stream *s = new lc_counter_stream;
        s->ctx = ctx;
        s->tile = tile;
        s->launch_events = lccs::csp_launch_events(o ? o->launch_events : 0, tile);
        s->cap = cap;
        add_key(s, LC_NO_KEY);
        if (ctx) {
            int rc = lccs::cs_dev_open ? lccs::cs_dev_open(ctx, tile, s->launch_events, &s->dev)
                                       : lc::fail(LC_E_UNSUPPORTED, "lc_counter_stream_open: this build has no device half");
            double ms = 0;
            if (!rc) rc = lccs::cs_dev_reserve(s->dev, cap, 0, &ms);
            if (rc) {
                if (s->dev) lccs::cs_dev_close(s->dev);
                delete s;
                return rc;
            }
        } else {
            s->host = new HostFold;
        }
        *out = s;
        return LC_OK;
    });
}

extern "C" void lc_counter_stream_close(lc_counter_stream *s) {
    if (!s) return;
    if (s->dev) lccs::cs_dev_close(s->dev);
    delete s->host;
    delete s;
}

extern "C" int lc_counter_stream_append(lc_counter_stream *s, const lc_counter_history *rows, lc_counter_stream_update *u) {
    lc::Range range("lc_counter_stream_append");
    if (!s || !rows) return lc::fail(LC_E_INVALID, "lc_counter_stream_append: null argument");
    return guarded("lc_counter_stream_append", [&]() -> int { return append(s, rows, u); });
}

extern "C" int lc_counter_stream_counts(lc_counter_stream *s, int8_t *valid, uint64_t *n_errors, uint64_t *n_reads) {
    if (!s || !valid || !n_errors || !n_reads) return lc::fail(LC_E_INVALID, "lc_counter_stream_counts: null argument");
    counts(s, valid, n_errors, n_reads);
    return LC_OK;
}

extern "C" int lc_counter_stream_results(lc_counter_stream *s, lc_counter_result *r, int64_t *value) {
    if (!s || !r) return lc::fail(LC_E_INVALID, "lc_counter_stream_results: null argument");
    if (s->broken) return lc::fail(LC_E_INVALID, "lc_counter_stream_results: an earlier append failed on the device");
    return guarded("lc_counter_stream_results", [&]() -> int { return results(s, r, value); });
}

extern "C" int64_t lc_counter_stream_keys(const lc_counter_stream *s, int64_t *out) {
    if (!s) return lc::fail(LC_E_INVALID, "lc_counter_stream_keys: null stream");
    if (out) std::copy(s->keys.begin(), s->keys.end(), out);
    return (int64_t)s->keys.size();
}

extern "C" const char *lc_counter_stream_key_error(const lc_counter_stream *s, int64_t i) {
    if (!s || i < 0 || (size_t)i >= s->key.size()) return nullptr;
    return s->key[(size_t)i].error();
}

extern "C" int lc_counter_stream_last_timing(const lc_counter_stream *s, double *out6) {
    if (!s || !out6) return lc::fail(LC_E_INVALID, "lc_counter_stream_last_timing: null argument");
    std::copy(s->ms, s->ms + 6, out6);
    return LC_OK;
}

extern "C" int lc_counter_stream_launch_info(int64_t *out6) {
    if (!out6) return lc::fail(LC_E_INVALID, "lc_counter_stream_launch_info: null out");
    out6[0] = lccs::CSP_BLOCK;
    out6[1] = lcc::CT_TILE_DEFAULT;
    out6[2] = lccs::CSP_READ_BYTES;
    out6[3] = (int64_t)lccs::CSP_MAX_BYTES;
    out6[4] = (int64_t)lccs::CSP_DEFAULT_READS;
    out6[5] = (int64_t)lccs::CSP_LAUNCH_EVENTS;
    return LC_OK;
}
