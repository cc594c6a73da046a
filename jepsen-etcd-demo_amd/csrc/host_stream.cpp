// host_stream.cpp -- lc_stream_*: the streaming packer and the stream's
// verdict book-keeping (include/lincheck.h "incremental check"; DESIGN.md
// section 3.11).  The device half -- the per-key records and k_stream's
// launch -- is device_stream.hip's (device_stream.hpp).
//
// The packer restates lc_pack's steps (host_pack.cpp: pairing, complete's
// value fill, without-failures, window slots, interning) for rows that arrive
// in pieces.  An invoke row turns into an event only once its fate is known:
//   completed :ok    value = (or invocation-value completion-value)
//   completed :fail  emits nothing
//   :info            pending forever, its own value
//   superseded       the same process invokes again in the key: pending forever
//   open at finish   pending forever
// so a key's rows from its first invoke without a fate are held back, and what
// lies before them -- the decided prefix -- is emitted.  State ids and
// transition ids are per key and stable for the stream's life (nil = state 0);
// every value an op names is interned when the op is emitted, reads included:
// a read may precede the write that installs its value.
//
// With LC_STREAM_SET_TIER (lc_stream_open_opts) a key that leaves the register
// tier is not held for lc_stream_finish: send_rows sends its words past
// defer_at too -- the first time with a migration item (the key's pool slot and
// its pending ops' descriptors by window slot), later to its set record
// (device_stream_set.hip).  A key the set tier cannot hold falls back to the
// deferral (stream_plan.hpp stream_set_falls_back) and its slot is reused.
//
// With LC_STREAM_EXACT the register tier's launches are k_stream_exact's
// (device_stream_exact.hip): a key may also die at the budget (:unknown, not on
// the invalid list), a dead key brings its peak and the final configs of the
// set before its failing event with it, lc_stream_finish fetches every other
// key's (k_stream_final; deferred keys from the batch path), and
// lc_stream_report renders a key's counterexample from the packer's own words
// and rows (report_core.hpp).
//
// With both flags the set tier's launches are k_stream_set_exact's
// (device_stream_set_exact.hip): the migrated set is Knossos's own, so a key
// in the set tier dies at the budget or invalid at the oracle's event, with
// its peak and final configs, and lc_stream_finish fetches the live set-tier
// keys' too (k_stream_set_final).

#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "common.hpp"
#include "device_stream.hpp"
#include "report_core.hpp"
#include "stream_plan.hpp"

namespace {

enum { FATE_OPEN = 0, FATE_OK = 1, FATE_FAIL = 2, FATE_FOREVER = 3 };

struct SOp {
    int64_t v0, v1;
    uint8_t f, fate;
    int16_t slot;   // window slot once emitted
};

struct Held {
    int64_t row;
    int32_t op;
    bool ok;        // the op's :ok row (else its invoke row)
};

inline bool client_f(uint8_t f, int model) {
    if (model == LC_MODEL_MUTEX) return f == LC_F_ACQUIRE || f == LC_F_RELEASE;
    if (model == LC_MODEL_REGISTER) return f == LC_F_READ || f == LC_F_WRITE;
    return f == LC_F_READ || f == LC_F_WRITE || f == LC_F_CAS;
}

inline uint16_t word16(uint32_t w) {
    return (uint16_t)(((w >> 16) & 0x8000u) | (LC_EV_SLOT(w) << 11) | LC_EV_TRANS(w));
}

// One key of a stream: the packer's state (rows mode) and its verdict.
struct SKey {
    int64_t key = 0;
    // ---- packer
    std::vector<SOp> ops;            // ops some row still refers to (a pool: `free_ops` lists the holes)
    std::vector<int32_t> free_ops;
    std::vector<std::pair<int64_t, int32_t>> procs;  // process -> its open op
    std::vector<Held> held;          // rows held back, from held_head
    size_t held_head = 0;
    uint64_t freemask[2] = {~0ull, ~0ull};
    std::vector<int64_t> vals;       // state id -> value (id 0: nil)
    std::unordered_map<int64_t, uint32_t> val_id;  // used past 16 states
    std::vector<uint32_t> descs;     // transition id -> descriptor
    std::unordered_map<uint32_t, uint32_t> desc_id;  // used past 32 descriptors
    std::vector<uint32_t> ev;        // every emitted word (32-bit form)
    std::vector<int64_t> ev_row;     // ... and its history row
    int width = 0;                   // 1 + the largest slot used
    int64_t defer_at = -1;           // ordinal of the invoke that left the register tier
    int err = 0;
    std::string msg;
    // ---- the search
    uint64_t sent = 0;               // events given to the device
    int8_t valid = LC_VALID;
    uint8_t cause = LC_CAUSE_NONE;
    int32_t fail_event = -1;
    bool dead = false;               // invalid or in error on the device: no more words go there
    bool touched = false;
    // ---- the resident set tier (LC_STREAM_SET_TIER)
    int32_t set_slot = -1;           // its set record in the pool, while it is in the set tier
    bool fell_back = false;          // it left the set tier (or could not enter it): checked at finish
    // ---- exact mode (LC_STREAM_EXACT): the words lc_check_batch writes beside the verdict
    uint32_t peak = 1;               // a dead key's; every key's after finish
    std::vector<uint64_t> finals;    // two words per config: a dead key's, every key's after finish
};

}  // namespace

struct lc_stream {
    lc_ctx *ctx = nullptr;
    lcst::StreamDev *dev = nullptr;
    int model = LC_MODEL_CAS_REGISTER;
    int mode = 0;  // 0 undecided, 1 rows, 2 events
    bool finished = false;
    std::vector<SKey> keys;
    std::unordered_map<int64_t, int32_t> key_index;
    int64_t rows_seen = 0;
    int64_t rows_held = 0, n_deferred = 0;
    uint32_t init_state = 0;  // events mode: the chunks' (all the same)
    bool have_init = false;
    std::vector<int64_t> invalid_now;
    std::vector<int32_t> touched;
    double ms[4] = {0, 0, 0, 0};
    // scratch of one call
    std::vector<lcst::Item> items;
    std::vector<uint16_t> ev16;
    std::vector<uint32_t> trans;
    std::vector<lcst::Dead> dead;
    bool set_tier = false;  // LC_STREAM_SET_TIER, on a stream with a device
    bool exact = false;     // LC_STREAM_EXACT
    std::vector<lcst::Final> fin;  // exact mode: beside `dead`, entry for entry
    double final_ms = 0;    // exact mode: k_stream_final at finish, and the keys it wrote
    int64_t final_keys = 0;
    std::vector<lcst::SetMig> set_mig;
    std::vector<lcst::SetItem> set_items;
    std::vector<uint32_t> ev32;
};

namespace {

int32_t key_of(lc_stream *s, int64_t key) {
    auto it = s->key_index.find(key);
    if (it != s->key_index.end()) return it->second;
    const int32_t i = (int32_t)s->keys.size();
    s->keys.emplace_back();
    SKey &k = s->keys.back();
    k.key = key;
    k.vals.push_back(LC_NIL);
    if (s->model == LC_MODEL_MUTEX) k.vals.push_back(1);  // state 1 = locked (state 0 = unlocked)
    s->key_index.emplace(key, i);
    return i;
}

void key_error(SKey &k, int err, std::string msg) {
    if (k.err) return;
    k.err = err;
    k.msg = std::move(msg);
}

int32_t new_op(SKey &k, const SOp &op) {
    if (!k.free_ops.empty()) {
        const int32_t i = k.free_ops.back();
        k.free_ops.pop_back();
        k.ops[(size_t)i] = op;
        return i;
    }
    k.ops.push_back(op);
    return (int32_t)k.ops.size() - 1;
}

int32_t *proc_find(SKey &k, int64_t p) {
    for (auto &e : k.procs)
        if (e.first == p) return &e.second;
    return nullptr;
}
void proc_erase(SKey &k, int64_t p) {
    for (size_t i = 0; i < k.procs.size(); ++i)
        if (k.procs[i].first == p) {
            k.procs[i] = k.procs.back();
            k.procs.pop_back();
            return;
        }
}

// State id of a value, interned on first use; *grew: a new id was made.
uint32_t state_id(SKey &k, int64_t v) {
    if (v == LC_NIL) return 0;
    if (k.val_id.empty()) {
        for (size_t i = 1; i < k.vals.size(); ++i)
            if (k.vals[i] == v) return (uint32_t)i;
        if (k.vals.size() > 16)
            for (size_t i = 1; i < k.vals.size(); ++i) k.val_id.emplace(k.vals[i], (uint32_t)i);
    } else {
        auto it = k.val_id.find(v);
        if (it != k.val_id.end()) return it->second;
    }
    if (k.vals.size() >= LC_STATE_NONE) return LC_STATE_NONE;
    const uint32_t id = (uint32_t)k.vals.size();
    k.vals.push_back(v);
    if (!k.val_id.empty()) k.val_id.emplace(v, id);
    return id;
}

uint32_t describe(SKey &k, const SOp &op) {
    switch (op.f) {
        case LC_F_ACQUIRE: return LC_DESC(LC_T_CAS, 0, 1);  // unlocked -> locked
        case LC_F_RELEASE: return LC_DESC(LC_T_CAS, 1, 0);  // locked -> unlocked
        case LC_F_READ: return op.v0 == LC_NIL ? LC_DESC(LC_T_READ_ANY, 0, 0) : LC_DESC(LC_T_READ, state_id(k, op.v0), 0);
        case LC_F_WRITE: return LC_DESC(LC_T_WRITE, 0, state_id(k, op.v0));
        default: {
            const uint32_t a = state_id(k, op.v0), b = state_id(k, op.v1);
            return LC_DESC(LC_T_CAS, a, b);
        }
    }
}

uint32_t trans_id(SKey &k, uint32_t d) {
    if (k.desc_id.empty()) {
        for (size_t i = 0; i < k.descs.size(); ++i)
            if (k.descs[i] == d) return (uint32_t)i;
        if (k.descs.size() > 32)
            for (size_t i = 0; i < k.descs.size(); ++i) k.desc_id.emplace(k.descs[i], (uint32_t)i);
    } else {
        auto it = k.desc_id.find(d);
        if (it != k.desc_id.end()) return it->second;
    }
    const uint32_t id = (uint32_t)k.descs.size();
    k.descs.push_back(d);
    if (!k.desc_id.empty()) k.desc_id.emplace(d, id);
    return id;
}

// Emit the key's decided prefix: held rows up to its first invoke without a fate.
void drain(lc_stream *s, SKey &k) {
    while (k.held_head < k.held.size()) {
        const Held h = k.held[k.held_head];
        SOp &op = k.ops[(size_t)h.op];
        if (!h.ok && op.fate == FATE_OPEN) break;
        ++k.held_head;
        --s->rows_held;
        if (!h.ok) {
            if (op.fate == FATE_FAIL) {  // without-failures
                k.free_ops.push_back(h.op);
                continue;
            }
            int slot;
            if (k.freemask[0]) slot = __builtin_ctzll(k.freemask[0]);
            else if (k.freemask[1]) slot = 64 + __builtin_ctzll(k.freemask[1]);
            else slot = 128;
            if (slot < 127) k.freemask[slot >> 6] &= ~(1ull << (slot & 63));
            const int enc = slot < 127 ? slot : 127;  // >= 127 cannot be encoded; the search stops earlier
            op.slot = (int16_t)enc;
            k.width = std::max(k.width, std::min(slot + 1, 255));
            const uint32_t d = describe(k, op);
            const uint32_t t = trans_id(k, d);
            if (k.defer_at < 0 && lc::stream_defers((uint32_t)slot, (uint32_t)k.vals.size())) {
                k.defer_at = (int64_t)k.ev.size();
                if (!s->set_tier) ++s->n_deferred;  // (set tier: counted when the key falls back)
            }
            k.ev.push_back(((uint32_t)enc << 24) | (t & 0xFFFFFFu));
            k.ev_row.push_back(h.row);
            if (op.fate == FATE_FOREVER) k.free_ops.push_back(h.op);  // no row names it again; its slot stays taken
        } else {
            const int slot = op.slot;
            if (slot < 127) k.freemask[slot >> 6] |= 1ull << (slot & 63);
            k.ev.push_back(LC_EV_OK_BIT | ((uint32_t)slot << 24));
            k.ev_row.push_back(h.row);
            k.free_ops.push_back(h.op);
        }
    }
    if (k.held_head == k.held.size()) {
        k.held.clear();
        k.held_head = 0;
    } else if (k.held_head > 64 && k.held_head * 2 > k.held.size()) {
        k.held.erase(k.held.begin(), k.held.begin() + (std::ptrdiff_t)k.held_head);
        k.held_head = 0;
    }
}

void touch(lc_stream *s, int32_t ki) {
    SKey &k = s->keys[(size_t)ki];
    if (!k.touched) {
        k.touched = true;
        s->touched.push_back(ki);
    }
}

// A key that leaves the set tier (dead, in error, fallen back) gives its record back.
void release_set(lc_stream *s, SKey &k) {
    if (k.set_slot < 0) return;
    lcst::stream_dev_set_free(s->dev, k.set_slot);
    k.set_slot = -1;
}

// One row of key ki (A3 pairing, as host_pack.cpp pair_rows).
void take_row(lc_stream *s, int32_t ki, const lc_history &h, int64_t r, int64_t row) {
    SKey &k = s->keys[(size_t)ki];
    if (k.err) return;
    const uint8_t t = h.type[r];
    const int64_t p = h.process[r];
    if (t == LC_INVOKE) {
        if (!client_f(h.f[r], s->model)) {
            static const char *names[] = {"cas-register", "register", "mutex"};
            key_error(k, LC_E_UNSUPPORTED, "row " + std::to_string(row) + ": " + names[s->model] + " cannot step this :f");
            release_set(s, k);
            return;
        }
        const int32_t id = new_op(k, SOp{h.v0[r], h.v1[r], h.f[r], FATE_OPEN, -1});
        if (int32_t *open = proc_find(k, p)) {
            k.ops[(size_t)*open].fate = FATE_FOREVER;  // superseded: complete's assoc! overwrites the pending index
            *open = id;
        } else {
            k.procs.emplace_back(p, id);
        }
        k.held.push_back(Held{row, id, false});
        ++s->rows_held;
    } else if (t == LC_OK_T || t == LC_FAIL) {
        int32_t *open = proc_find(k, p);
        if (!open) {
            key_error(k, LC_E_INVALID,
                      "row " + std::to_string(row) + ": process completed an operation without a prior invocation");
            release_set(s, k);
            return;
        }
        SOp &op = k.ops[(size_t)*open];
        if (t == LC_OK_T) {
            op.fate = FATE_OK;
            // (or (:value invocation) (:value completion))
            if (op.f == LC_F_CAS) {
                if (op.v0 == LC_NIL && op.v1 == LC_NIL) { op.v0 = h.v0[r]; op.v1 = h.v1[r]; }
            } else if (op.v0 == LC_NIL) {
                op.v0 = h.v0[r];
            }
            k.held.push_back(Held{row, *open, true});
            ++s->rows_held;
        } else {
            op.fate = FATE_FAIL;
        }
        proc_erase(k, p);
    } else {  // :info -- crashed: pending forever
        if (int32_t *open = proc_find(k, p)) {
            k.ops[(size_t)*open].fate = FATE_FOREVER;
            proc_erase(k, p);
        }
    }
    drain(s, k);
    touch(s, ki);
}

void fill_update(lc_stream *s, lc_stream_update *u, int64_t events) {
    if (!u) return;
    u->n_keys = (int64_t)s->keys.size();
    u->events = events;
    u->rows_held = s->rows_held;
    u->n_deferred = s->n_deferred;
    u->n_invalid = (int64_t)s->invalid_now.size();
    u->invalid = s->invalid_now.empty() ? nullptr : s->invalid_now.data();
}

void fall_back(lc_stream *s, SKey &k) {
    release_set(s, k);
    if (!k.fell_back) ++s->n_deferred;
    k.fell_back = true;
}

// The launch's dead keys into the verdicts; the first key in error (or -1).
int64_t take_dead(lc_stream *s, uint32_t *why) {
    int64_t bad = -1;
    for (size_t di = 0; di < s->dead.size(); ++di) {
        const lcst::Dead &d = s->dead[di];
        if (d.key >= s->keys.size()) continue;
        SKey &k = s->keys[d.key];
        if (d.status == lc::STREAM_SET_FALLBACK) {  // back to deferral: not dead, checked at finish
            fall_back(s, k);
            continue;
        }
        release_set(s, k);
        k.dead = true;
        if (d.status == lc::STREAM_INVALID) {
            k.valid = LC_INVALID;
            k.cause = LC_CAUSE_NONLIN;
            k.fail_event = (int32_t)d.fail_event;
            s->invalid_now.push_back((int64_t)d.key);
        } else if (d.status == lc::STREAM_BUDGET) {  // exact mode: :unknown, not on the invalid list
            k.valid = LC_UNKNOWN;
            k.cause = LC_CAUSE_BUDGET;
            k.fail_event = (int32_t)d.fail_event;
        } else {
            k.valid = LC_UNKNOWN;
            k.cause = LC_CAUSE_ERROR;
            k.fail_event = -1;
            if (bad < 0) { bad = (int64_t)d.key; *why = d.why; }
        }
        if (s->exact && di < s->fin.size() && (d.status == lc::STREAM_INVALID || d.status == lc::STREAM_BUDGET)) {
            const lcst::Final &f = s->fin[di];
            k.peak = f.peak;
            k.finals.assign(f.cfg, f.cfg + 2 * (size_t)f.n_final);
        }
    }
    return bad;
}

// Rows mode: every touched key's unsent decided words to the device.
int send_rows(lc_stream *s, int64_t *events) {
    *events = 0;
    s->items.clear();
    s->ev16.clear();
    s->trans.clear();
    s->set_mig.clear();
    s->set_items.clear();
    s->ev32.clear();
    std::sort(s->touched.begin(), s->touched.end());
    for (int32_t ki : s->touched) {
        SKey &k = s->keys[(size_t)ki];
        k.touched = false;
        if (k.err || k.dead || !s->dev) continue;
        const uint64_t end = k.defer_at >= 0 ? (uint64_t)k.defer_at : (uint64_t)k.ev.size();
        const uint32_t tr_b = (uint32_t)s->trans.size();
        if (end > k.sent) {
            lcst::Item it;
            it.key = ki;
            it.ev_b = (uint32_t)s->ev16.size();
            for (uint64_t j = k.sent; j < end; ++j) s->ev16.push_back(word16(k.ev[(size_t)j]));
            it.ev_e = (uint32_t)s->ev16.size();
            it.tr_b = tr_b;
            it.ntr = (uint32_t)k.descs.size();
            s->trans.insert(s->trans.end(), k.descs.begin(), k.descs.end());
            it.ns = (uint32_t)k.vals.size();
            s->items.push_back(it);
            *events += (int64_t)(end - k.sent);
            k.sent = end;
        }
        // past the register tier: the key migrates with its first words there,
        // later words go to its set record
        if (!s->set_tier || k.defer_at < 0 || k.fell_back || k.ev.size() <= k.sent) continue;
        bool narrow = !lc::stream_set_falls_back(0, 0, 0, (uint32_t)k.vals.size());
        for (size_t j = (size_t)k.sent; j < k.ev.size() && narrow; ++j)
            narrow = (k.ev[j] & LC_EV_OK_BIT) || !lc::stream_set_falls_back(0, 0, LC_EV_SLOT(k.ev[j]), 0);
        if (!narrow) {
            fall_back(s, k);
            continue;
        }
        if (k.set_slot < 0) {
            int rc = lcst::stream_dev_set_alloc(s->dev, &k.set_slot);
            if (rc) return rc;
            lcst::SetMig m{};
            m.key = ki;
            m.slot = k.set_slot;
            // descriptors of the ops pending at defer_at, by window slot
            int32_t tr_of[64];
            std::fill(tr_of, tr_of + 64, -1);
            for (size_t j = 0; j < (size_t)k.defer_at; ++j) {
                const uint32_t w = k.ev[j], sl = LC_EV_SLOT(w) & 63u;
                tr_of[sl] = (w & LC_EV_OK_BIT) ? -1 : (int32_t)LC_EV_TRANS(w);
            }
            for (int sl = 0; sl < 64; ++sl) m.descs[sl] = tr_of[sl] >= 0 ? k.descs[(size_t)tr_of[sl]] : 0u;
            s->set_mig.push_back(m);
        }
        lcst::SetItem it;
        it.key = ki;
        it.slot = k.set_slot;
        it.ev_b = (uint32_t)s->ev32.size();
        s->ev32.insert(s->ev32.end(), k.ev.begin() + (std::ptrdiff_t)k.sent, k.ev.end());
        it.ev_e = (uint32_t)s->ev32.size();
        if (s->trans.size() == tr_b) s->trans.insert(s->trans.end(), k.descs.begin(), k.descs.end());
        it.tr_b = tr_b;
        it.ntr = (uint32_t)k.descs.size();
        s->set_items.push_back(it);
        *events += (int64_t)(k.ev.size() - k.sent);
        k.sent = k.ev.size();
    }
    s->touched.clear();
    if (!s->dev || (s->items.empty() && s->set_items.empty())) return LC_OK;
    const lcst::SetWork sw{s->set_mig.data(), (int64_t)s->set_mig.size(), s->set_items.data(),
                           (int64_t)s->set_items.size(), s->ev32.data(), s->ev32.size()};
    int rc = lcst::stream_dev_push(s->dev, (int64_t)s->keys.size(), s->items.data(), (int64_t)s->items.size(),
                                   s->ev16.data(), s->ev16.size(), s->trans.data(), s->trans.size(), 0, &s->dead,
                                   s->set_tier ? &sw : nullptr, &s->fin);
    if (rc) return rc;
    uint32_t why = 0;
    const int64_t bad = take_dead(s, &why);
    if (bad >= 0)  // the packer's own words: cannot happen
        return lc::fail(LC_E_DEVICE, "lc_stream: the device refused the packer's words of key index %lld (reasons 0x%x)",
                        (long long)bad, why);
    return LC_OK;
}

int check_mode(lc_stream *s, int mode, const char *fn) {
    if (s->finished) return lc::fail(LC_E_INVALID, "%s: the stream is finished", fn);
    if (s->mode && s->mode != mode)
        return lc::fail(LC_E_INVALID, "%s: the stream is in %s mode (fixed by its first call)", fn,
                        s->mode == 1 ? "rows" : "events");
    return LC_OK;
}

// Exact mode at finish: the live register-tier keys' end sets (k_stream_final),
// the live set-tier keys' (k_stream_set_final) and every searched key's peak,
// into the keys.  Keys that died keep what
// their launch left; deferred keys got theirs from the batch path.
int finish_exact(lc_stream *s) {
    const size_t n = s->keys.size();
    if (!n) return LC_OK;
    std::vector<int32_t> live;
    std::vector<lcst::SetLive> set_live;  // with the set tier: its keys still live (k_stream_set_final)
    for (size_t ki = 0; ki < n; ++ki) {
        const SKey &k = s->keys[ki];
        if (k.err || k.dead) continue;
        if (k.defer_at < 0) live.push_back((int32_t)ki);
        else if (s->set_tier && !k.fell_back && k.set_slot >= 0) set_live.push_back(lcst::SetLive{(int32_t)ki, k.set_slot});
    }
    const size_t mf = (size_t)lcst::stream_dev_max_final(s->dev);
    std::vector<uint64_t> cfg(n * mf * 2 + 1);
    std::vector<uint32_t> n_final(n), peak(n);
    int rc = lcst::stream_dev_finals(s->dev, (int64_t)n, live.data(), (int64_t)live.size(), s->init_state, cfg.data(),
                                     n_final.data(), set_live.data(), (int64_t)set_live.size());
    if (rc) return rc;
    s->final_ms = lcst::stream_dev_final_ms(s->dev);
    s->final_keys = (int64_t)live.size();
    rc = lcst::stream_dev_peaks(s->dev, (int64_t)n, peak.data());
    if (rc) return rc;
    for (const lcst::SetLive &sl : set_live) live.push_back(sl.key);
    for (int32_t ki : live) {
        SKey &k = s->keys[(size_t)ki];
        k.peak = peak[(size_t)ki];
        k.finals.assign(cfg.begin() + (std::ptrdiff_t)((size_t)ki * mf * 2),
                        cfg.begin() + (std::ptrdiff_t)((size_t)ki * mf * 2 + (size_t)n_final[(size_t)ki] * 2));
    }
    return LC_OK;
}

double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

void dev_times(lc_stream *s) {
    double t[3] = {0, 0, 0};
    if (s->dev) lcst::stream_dev_timing(s->dev, t);
    s->ms[1] = t[0]; s->ms[2] = t[1]; s->ms[3] = t[2];
}

}  // namespace

extern "C" int lc_stream_open(lc_ctx *ctx, const lc_pack_opts *opts, lc_stream **out) {
    return lc_stream_open_opts(ctx, opts, nullptr, out);
}

extern "C" int lc_stream_open_opts(lc_ctx *ctx, const lc_pack_opts *opts, const lc_stream_opts *sopts, lc_stream **out) {
    if (!out) return lc::fail(LC_E_INVALID, "lc_stream_open: null out");
    *out = nullptr;
    if (sopts && (sopts->flags & ~(uint32_t)(LC_STREAM_SET_TIER | LC_STREAM_EXACT)))
        return lc::fail(LC_E_INVALID, "lc_stream_open_opts: unknown flags 0x%x", sopts->flags);
    const bool exact = sopts && (sopts->flags & LC_STREAM_EXACT);
    if (exact && (sopts->flags & LC_STREAM_SET_TIER) && !ctx)
        return lc::fail(LC_E_UNSUPPORTED, "lc_stream_open_opts: LC_STREAM_EXACT with LC_STREAM_SET_TIER: a packer-only "
                                          "stream has no set tier to make exact");
    const int model = opts ? opts->model : LC_MODEL_CAS_REGISTER;
    if (model == LC_MODEL_MULTI_REGISTER)
        return lc::fail(LC_E_UNSUPPORTED, "lc_stream_open: multi-register has no register-tier search to resume");
    if (model < 0 || model > LC_MODEL_MUTEX) return lc::fail(LC_E_INVALID, "lc_stream_open: unknown model %d", model);
    lc_stream *s = new lc_stream;
    s->ctx = ctx;
    s->model = model;
    s->exact = exact;
    if (ctx) {
        int rc = lcst::stream_dev_open(ctx, exact, &s->dev);
        if (rc) {
            delete s;
            return rc;
        }
    }
    s->set_tier = s->dev && sopts && (sopts->flags & LC_STREAM_SET_TIER);
    *out = s;
    return LC_OK;
}

extern "C" void lc_stream_close(lc_stream *s) {
    if (!s) return;
    lcst::stream_dev_close(s->dev);
    delete s;
}

extern "C" int lc_stream_append(lc_stream *s, const lc_history *h, lc_stream_update *u) {
    if (!s || !h) return lc::fail(LC_E_INVALID, "lc_stream_append: null argument");
    int rc = check_mode(s, 1, "lc_stream_append");
    if (rc) return rc;
    if (h->n < 0 || (h->n > 0 && (!h->type || !h->f || !h->process || !h->key || !h->v0 || !h->v1)))
        return lc::fail(LC_E_INVALID, "lc_stream_append: null column");
    // refusals first: a refused call leaves the stream as it was
    for (int64_t r = 0; r < h->n; ++r) {
        if (h->type[r] > LC_INFO) return lc::fail(LC_E_INVALID, "lc_stream_append: row %lld: bad :type code %d", (long long)r, h->type[r]);
        if (h->f[r] > LC_F_TXN) return lc::fail(LC_E_INVALID, "lc_stream_append: row %lld: bad :f code %d", (long long)r, h->f[r]);
        if (h->f[r] == LC_F_TXN) return lc::fail(LC_E_UNSUPPORTED, "lc_stream_append: row %lld: a :txn row in a register stream", (long long)r);
        if (h->key[r] == LC_NO_KEY && h->process[r] != LC_NO_PROCESS)
            return lc::fail(LC_E_UNSUPPORTED, "lc_stream_append: row %lld: a client row without a key belongs to every key's "
                                              "sub-history; a stream cannot hold it", (long long)r);
    }
    const double t0 = now_ms();
    s->mode = 1;
    s->invalid_now.clear();
    for (int64_t r = 0; r < h->n; ++r) {
        if (h->key[r] == LC_NO_KEY) continue;  // the nemesis: a no-op in every key
        if (h->process[r] == LC_NO_PROCESS) {
            // a keyed row of no client process: only an :info is a no-op (as in lc_pack)
            if (h->type[r] == LC_INFO) continue;
        }
        take_row(s, key_of(s, h->key[r]), *h, r, s->rows_seen + r);
    }
    s->rows_seen += h->n;
    int64_t events = 0;
    s->ms[0] = now_ms() - t0;
    rc = send_rows(s, &events);
    dev_times(s);
    if (rc) return rc;
    fill_update(s, u, events);
    return LC_OK;
}

extern "C" int lc_stream_finish(lc_stream *s, lc_stream_update *u) {
    if (!s) return lc::fail(LC_E_INVALID, "lc_stream_finish: null argument");
    if (s->finished) return lc::fail(LC_E_INVALID, "lc_stream_finish: the stream is finished");
    s->invalid_now.clear();
    int64_t events = 0;
    if (s->mode == 1) {
        const double t0 = now_ms();
        // ops still open are pending forever: every held row is decided
        for (size_t ki = 0; ki < s->keys.size(); ++ki) {
            SKey &k = s->keys[ki];
            if (k.err || k.held_head == k.held.size()) continue;
            for (size_t j = k.held_head; j < k.held.size(); ++j) {
                SOp &op = k.ops[(size_t)k.held[j].op];
                if (op.fate == FATE_OPEN) op.fate = FATE_FOREVER;
            }
            k.procs.clear();
            drain(s, k);
            touch(s, (int32_t)ki);
        }
        s->ms[0] = now_ms() - t0;
        int rc = send_rows(s, &events);
        dev_times(s);
        if (rc) return rc;
        // deferred keys: once, from their first event, through the batch path
        std::vector<int32_t> dk;
        for (size_t ki = 0; ki < s->keys.size(); ++ki) {
            const SKey &k = s->keys[ki];
            if (k.defer_at >= 0 && !k.err && !k.dead && (!s->set_tier || k.fell_back)) dk.push_back((int32_t)ki);
        }
        if (!dk.empty() && s->ctx) {
            std::vector<uint64_t> ev_off(dk.size() + 1, 0);
            std::vector<uint32_t> events32, trans, trans_off(dk.size());
            std::vector<uint8_t> width(dk.size());
            std::vector<uint16_t> states(dk.size());
            for (size_t i = 0; i < dk.size(); ++i) {
                const SKey &k = s->keys[(size_t)dk[i]];
                events32.insert(events32.end(), k.ev.begin(), k.ev.end());
                ev_off[i + 1] = events32.size();
                trans_off[i] = (uint32_t)trans.size();
                trans.insert(trans.end(), k.descs.begin(), k.descs.end());
                width[i] = (uint8_t)std::min(k.width, 255);
                states[i] = (uint16_t)std::min<size_t>(k.vals.size(), 65535);
            }
            lc_batch b{};
            b.n_keys = (int64_t)dk.size();
            b.ev_off = ev_off.data();
            b.events = events32.data();
            b.trans = trans.data();
            b.n_trans = (int64_t)trans.size();
            b.trans_off = trans_off.data();
            b.key_width = width.data();
            b.key_states = states.data();
            b.init_state = 0;
            std::vector<int8_t> valid(dk.size());
            std::vector<int32_t> fev(dk.size());
            std::vector<uint8_t> cause(dk.size());
            lc_result r{};
            r.valid = valid.data();
            r.fail_event = fev.data();
            r.cause = cause.data();
            // exact mode: the keys' full records, as the one-shot check writes them
            const size_t mf = s->exact ? (size_t)lcst::stream_dev_max_final(s->dev) : 0;
            std::vector<uint32_t> peak, n_final;
            std::vector<uint64_t> cfg;
            if (s->exact) {
                peak.assign(dk.size(), 0);
                n_final.assign(dk.size(), 0);
                cfg.assign(dk.size() * mf * 2 + 1, 0);
                r.peak_configs = peak.data();
                r.n_final = n_final.data();
                r.final_configs = cfg.data();
            }
            rc = lc_check_batch(s->ctx, &b, &r, nullptr);
            if (rc) return rc;
            for (size_t i = 0; i < dk.size(); ++i) {
                SKey &k = s->keys[(size_t)dk[i]];
                k.valid = valid[i];
                k.cause = cause[i];
                k.fail_event = fev[i];
                if (s->exact) {
                    k.peak = peak[i];
                    const size_t nf = std::min<size_t>(n_final[i], mf);
                    k.finals.assign(cfg.begin() + (std::ptrdiff_t)(i * mf * 2), cfg.begin() + (std::ptrdiff_t)(i * mf * 2 + nf * 2));
                }
                if (valid[i] == LC_INVALID) s->invalid_now.push_back(dk[i]);
            }
            std::sort(s->invalid_now.begin(), s->invalid_now.end());
        }
    }
    if (s->exact && s->dev) {
        int rc = finish_exact(s);
        if (rc) return rc;
    }
    s->finished = true;
    fill_update(s, u, events);
    return LC_OK;
}

extern "C" int lc_stream_push(lc_stream *s, const lc_batch *b, const int64_t *key_ids, lc_stream_update *u) {
    if (!s || !b) return lc::fail(LC_E_INVALID, "lc_stream_push: null argument");
    int rc = check_mode(s, 2, "lc_stream_push");
    if (rc) return rc;
    if (!s->dev) return lc::fail(LC_E_INVALID, "lc_stream_push: a packer-only stream has no device");
    if (b->n_keys < 0 || b->n_keys > (int64_t)1 << 30) return lc::fail(LC_E_INVALID, "lc_stream_push: bad n_keys");
    if (b->n_keys > 0 && (!key_ids || !b->ev_off || (!b->events && !b->events16) || !b->key_width || !b->key_states))
        return lc::fail(LC_E_INVALID, "lc_stream_push: key_ids, ev_off, event words, key_width and key_states are required");
    if (b->table) return lc::fail(LC_E_UNSUPPORTED, "lc_stream_push: a table model's chunk");
    if (b->n_trans < 0 || (b->n_trans > 0 && !b->trans)) return lc::fail(LC_E_INVALID, "lc_stream_push: bad transition table");
    if (b->init_state >= lc::STREAM_MAX_STATES || (s->have_init && b->init_state != s->init_state))
        return lc::fail(LC_E_INVALID, "lc_stream_push: init_state %u (a stream has one, below %u)", b->init_state,
                        lc::STREAM_MAX_STATES);
    {
        std::unordered_map<int64_t, char> seen;
        for (int64_t k = 0; k < b->n_keys; ++k) {
            if (b->ev_off[k] > b->ev_off[k + 1] || b->ev_off[k + 1] > 0xFFFFFFFFull)
                return lc::fail(LC_E_INVALID, "lc_stream_push: ev_off is not ascending at key %lld", (long long)k);
            if (b->trans_off && b->trans_off[k] > (uint64_t)b->n_trans)
                return lc::fail(LC_E_INVALID, "lc_stream_push: trans_off of key %lld is past the table", (long long)k);
            if (b->key_width[k] > lc::STREAM_MAX_WIDTH || b->key_states[k] > lc::STREAM_MAX_STATES)
                return lc::fail(LC_E_UNSUPPORTED, "lc_stream_push: key %lld (width %d, %d states) leaves the register tier",
                                (long long)k, b->key_width[k], b->key_states[k]);
            if (!seen.emplace(key_ids[k], 0).second)
                return lc::fail(LC_E_INVALID, "lc_stream_push: key id %lld twice in one chunk", (long long)key_ids[k]);
        }
    }
    const double t0 = now_ms();
    s->mode = 2;
    s->init_state = b->init_state;
    s->have_init = true;
    s->invalid_now.clear();
    s->items.clear();
    s->ev16.clear();
    int64_t events = 0, host_bad = -1;
    for (int64_t k = 0; k < b->n_keys; ++k) {
        const int32_t ki = key_of(s, key_ids[k]);
        SKey &K = s->keys[(size_t)ki];
        const uint64_t eb = b->ev_off[k], ee = b->ev_off[k + 1];
        if (K.dead || eb == ee) continue;
        lcst::Item it;
        it.key = ki;
        it.ev_b = (uint32_t)s->ev16.size();
        bool fits = true;
        for (uint64_t j = eb; j < ee; ++j) {
            if (b->events16) {
                s->ev16.push_back(b->events16[j]);
            } else {
                const uint32_t w = b->events[j];
                fits &= LC_EV_SLOT(w) <= LC_EV16_MAX_SLOT && LC_EV_TRANS(w) <= LC_EV16_MAX_TRANS;
                s->ev16.push_back(word16(w));
            }
        }
        if (!fits) {  // a word no register-tier key has: malformed before the device sees it
            s->ev16.resize(it.ev_b);
            K.dead = true;
            K.valid = LC_UNKNOWN;
            K.cause = LC_CAUSE_ERROR;
            K.fail_event = -1;
            if (host_bad < 0) host_bad = ki;
            continue;
        }
        it.ev_e = (uint32_t)s->ev16.size();
        it.tr_b = b->trans_off ? b->trans_off[k] : 0u;
        it.ntr = (uint32_t)b->n_trans - it.tr_b;
        it.ns = b->key_states[k];
        s->items.push_back(it);
        events += (int64_t)(ee - eb);
        K.sent += ee - eb;
    }
    s->ms[0] = now_ms() - t0;
    rc = lcst::stream_dev_push(s->dev, (int64_t)s->keys.size(), s->items.data(), (int64_t)s->items.size(), s->ev16.data(),
                               s->ev16.size(), b->trans, (uint64_t)b->n_trans, s->init_state, &s->dead, nullptr, &s->fin);
    dev_times(s);
    if (rc) return rc;
    uint32_t why = 0;
    int64_t bad = take_dead(s, &why);
    fill_update(s, u, events);
    if (bad < 0 && host_bad >= 0) { bad = host_bad; why = 4; }
    if (bad >= 0)
        return lc::fail(LC_E_INVALID, "lc_stream_push: key index %lld (id %lld) has malformed event words (reasons 0x%x: 1 slot "
                                      "protocol, 2 transition, 4 fit); the other keys advanced",
                        (long long)bad, (long long)s->keys[(size_t)bad].key, why);
    return LC_OK;
}

extern "C" int lc_stream_results(lc_stream *s, lc_result *r) {
    if (!s || !r) return lc::fail(LC_E_INVALID, "lc_stream_results: null argument");
    if (!s->dev) return lc::fail(LC_E_INVALID, "lc_stream_results: a packer-only stream searches nothing");
    if (!s->keys.empty() && (!r->valid || !r->fail_event || !r->cause))
        return lc::fail(LC_E_INVALID, "lc_stream_results: valid, fail_event and cause are required");
    for (size_t i = 0; i < s->keys.size(); ++i) {
        const SKey &k = s->keys[i];
        if (k.err) {  // check-safe around that one key, whatever was found before
            r->valid[i] = LC_UNKNOWN;
            r->cause[i] = LC_CAUSE_ERROR;
            r->fail_event[i] = -1;
        } else {
            r->valid[i] = k.valid;
            r->cause[i] = k.cause;
            r->fail_event[i] = k.fail_event;
        }
    }
    if (!s->exact) return LC_OK;
    // exact mode: the rest of the record, where the caller asks for it.  A
    // key that died or a finished stream: the words kept with the key; a live
    // key: its running peak from its device record, no configs yet.
    const size_t n = s->keys.size(), mf = (size_t)lcst::stream_dev_max_final(s->dev);
    if (r->peak_configs && n) {
        if (!s->finished) {
            int rc = lcst::stream_dev_peaks(s->dev, (int64_t)n, r->peak_configs);
            if (rc) return rc;
        }
        for (size_t i = 0; i < n; ++i) {
            const SKey &k = s->keys[i];
            if (k.err) r->peak_configs[i] = 0;
            else if (s->finished || k.dead) r->peak_configs[i] = k.peak;
        }
    }
    for (size_t i = 0; i < n; ++i) {
        const SKey &k = s->keys[i];
        const size_t nf = k.err ? 0 : std::min(k.finals.size() / 2, mf);
        if (r->n_final) r->n_final[i] = (uint32_t)nf;
        if (r->final_configs) {
            uint64_t *o = r->final_configs + i * mf * 2;
            std::fill(o, o + mf * 2, 0ull);
            std::copy(k.finals.begin(), k.finals.begin() + (std::ptrdiff_t)(nf * 2), o);
        }
    }
    return LC_OK;
}

namespace {
// A key of a stream as the counterexample's source (report_core.hpp): its own
// words, transitions, state values and event rows.
struct StreamSrc {
    const SKey &k;
    uint64_t n() const { return k.ev.size(); }
    uint32_t word(uint64_t j) const { return k.ev[(size_t)j]; }
    int64_t row(uint64_t j) const { return k.ev_row[(size_t)j]; }
    uint32_t step(uint32_t w, uint32_t st) const {
        const uint32_t t = LC_EV_TRANS(w);
        return t < k.descs.size() ? lcr::desc_step(k.descs[t], st) : LC_STATE_NONE;
    }
    int64_t value(uint32_t st) const { return st && st < k.vals.size() ? k.vals[st] : LC_NIL; }
    // An op in window slot `slot` whose :ok row has arrived but is still held
    // back behind an open invoke: its event is to come, its row is known.
    int64_t late_done_row(uint32_t slot) const {
        for (size_t j = k.held_head; j < k.held.size(); ++j)
            if (k.held[j].ok && k.ops[(size_t)k.held[j].op].slot == (int16_t)slot) return k.held[j].row;
        return -1;
    }
};
}  // namespace

extern "C" int64_t lc_stream_report(const lc_stream *s, int64_t i, int32_t valid, int32_t fail_event,
                                    const uint64_t *final_configs, uint32_t n_final, int32_t max_paths, int64_t *out,
                                    int64_t cap) {
    if (!s || i < 0 || i >= (int64_t)s->keys.size()) return lc::fail(LC_E_INVALID, "lc_stream_report: no such key index");
    if (s->mode == 2)
        return lc::fail(LC_E_UNSUPPORTED, "lc_stream_report: a stream in events mode has no history rows to name");
    const SKey &k = s->keys[(size_t)i];
    if (k.err) return lc::fail(LC_E_INVALID, "lc_stream_report: key %lld could not be prepared: %s", (long long)i, k.msg.c_str());
    return lcr::report(StreamSrc{k}, valid, fail_event, final_configs, n_final, max_paths, false, out, cap);
}

extern "C" int64_t lc_stream_keys(const lc_stream *s, int64_t *out) {
    if (!s) return lc::fail(LC_E_INVALID, "lc_stream_keys: null argument");
    if (out)
        for (size_t i = 0; i < s->keys.size(); ++i) out[i] = s->keys[i].key;
    return (int64_t)s->keys.size();
}

#define STREAM_KEY(fn)                                                                                      \
    if (!s || i < 0 || i >= (int64_t)s->keys.size()) return lc::fail(LC_E_INVALID, fn ": no such key index"); \
    const SKey &k = s->keys[(size_t)i]

extern "C" int lc_stream_key_events(const lc_stream *s, int64_t i, int64_t *out4) {
    STREAM_KEY("lc_stream_key_events");
    if (!out4) return lc::fail(LC_E_INVALID, "lc_stream_key_events: null out");
    out4[0] = (int64_t)k.ev.size();
    out4[1] = (int64_t)(k.held.size() - k.held_head);
    out4[2] = k.defer_at;
    out4[3] = (int64_t)k.sent;
    return LC_OK;
}

extern "C" int64_t lc_stream_event_row(const lc_stream *s, int64_t i, int64_t j) {
    STREAM_KEY("lc_stream_event_row");
    if (j < 0 || j >= (int64_t)k.ev_row.size()) return lc::fail(LC_E_INVALID, "lc_stream_event_row: key %lld has no event %lld", (long long)i, (long long)j);
    return k.ev_row[(size_t)j];
}

extern "C" int64_t lc_stream_key_words(const lc_stream *s, int64_t i, uint32_t *out, int64_t cap) {
    STREAM_KEY("lc_stream_key_words");
    if (out)
        for (int64_t j = 0; j < cap && j < (int64_t)k.ev.size(); ++j) out[j] = k.ev[(size_t)j];
    return (int64_t)k.ev.size();
}

extern "C" int64_t lc_stream_key_trans(const lc_stream *s, int64_t i, uint32_t *out, int64_t cap) {
    STREAM_KEY("lc_stream_key_trans");
    if (out)
        for (int64_t j = 0; j < cap && j < (int64_t)k.descs.size(); ++j) out[j] = k.descs[(size_t)j];
    return (int64_t)k.descs.size();
}

extern "C" int lc_stream_state_value(const lc_stream *s, int64_t i, uint32_t st, int64_t *value, int *is_nil) {
    STREAM_KEY("lc_stream_state_value");
    if (!value || !is_nil || st >= k.vals.size()) return lc::fail(LC_E_INVALID, "lc_stream_state_value: key %lld has no state %u", (long long)i, st);
    *value = k.vals[st];
    *is_nil = st == 0;
    return LC_OK;
}

extern "C" const char *lc_stream_key_error(const lc_stream *s, int64_t i) {
    if (!s || i < 0 || i >= (int64_t)s->keys.size()) return nullptr;
    const SKey &k = s->keys[(size_t)i];
    return k.err ? k.msg.c_str() : nullptr;
}

extern "C" int lc_stream_record(lc_stream *s, int64_t i, uint32_t *out) {
    STREAM_KEY("lc_stream_record");
    (void)k;
    if (!out) return lc::fail(LC_E_INVALID, "lc_stream_record: null out");
    if (!s->dev) return lc::fail(LC_E_INVALID, "lc_stream_record: a packer-only stream has no device");
    return lcst::stream_dev_record(s->dev, i, out);
}

namespace {
int tier_of(const lc_stream *s, const SKey &k) {
    if (k.err || k.dead) return LC_STREAM_TIER_DEAD;
    if (k.defer_at < 0) return LC_STREAM_TIER_REGISTER;
    return s->set_tier && !k.fell_back ? LC_STREAM_TIER_SET : LC_STREAM_TIER_FALLEN_BACK;
}
}  // namespace

extern "C" int lc_stream_key_tier(const lc_stream *s, int64_t i) {
    STREAM_KEY("lc_stream_key_tier");
    return tier_of(s, k);
}

extern "C" int lc_stream_tiers(const lc_stream *s, int64_t *out4) {
    if (!s || !out4) return lc::fail(LC_E_INVALID, "lc_stream_tiers: null argument");
    out4[0] = out4[1] = out4[2] = out4[3] = 0;
    for (const SKey &k : s->keys) ++out4[tier_of(s, k)];
    return LC_OK;
}

extern "C" int64_t lc_stream_set_record(lc_stream *s, int64_t i, uint32_t *out, int64_t cap) {
    STREAM_KEY("lc_stream_set_record");
    if (!s->dev || k.set_slot < 0) return lc::fail(LC_E_INVALID, "lc_stream_set_record: key %lld has no set record", (long long)i);
    uint32_t head[lc::STREAM_SET_OFF_S0];
    int rc = lcst::stream_dev_set_record(s->dev, k.set_slot, 0, head, lc::STREAM_SET_OFF_S0);
    if (rc) return rc;
    const int64_t n_s = std::min<uint32_t>(head[lc::STREAM_SET_H_NS], lc::STREAM_SET_CAP);
    const int64_t all = (int64_t)lc::STREAM_SET_OFF_S0 + 2 * n_s;
    if (out && cap > 0) {
        std::memcpy(out, head, (size_t)std::min<int64_t>(cap, lc::STREAM_SET_OFF_S0) * 4);
        const int64_t more = std::min(cap, all) - (int64_t)lc::STREAM_SET_OFF_S0;
        if (more > 0) {
            rc = lcst::stream_dev_set_record(s->dev, k.set_slot, lc::stream_set_off_s(head[lc::STREAM_SET_H_CUR] & 1u),
                                             out + lc::STREAM_SET_OFF_S0, more);
            if (rc) return rc;
        }
    }
    return all;
}

extern "C" int lc_stream_set_stats(const lc_stream *s, double *out6) {
    if (!s || !out6) return lc::fail(LC_E_INVALID, "lc_stream_set_stats: null argument");
    for (int i = 0; i < 6; ++i) out6[i] = 0;
    if (s->dev) lcst::stream_dev_set_stats(s->dev, out6);
    return LC_OK;
}

extern "C" int lc_stream_exact_stats(const lc_stream *s, double *out2) {
    if (!s || !out2) return lc::fail(LC_E_INVALID, "lc_stream_exact_stats: null argument");
    out2[0] = s->final_ms;
    out2[1] = (double)s->final_keys;
    return LC_OK;
}

extern "C" int lc_stream_last_timing(const lc_stream *s, double *out_ms4) {
    if (!s || !out_ms4) return lc::fail(LC_E_INVALID, "lc_stream_last_timing: null argument");
    for (int i = 0; i < 4; ++i) out_ms4[i] = s->ms[i];
    return LC_OK;
}
