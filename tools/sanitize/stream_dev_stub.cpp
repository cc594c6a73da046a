// The device half of a stream (csrc/device_stream.hpp) for the host-only
// sanitizer build: host_stream.cpp links against these.  A packer-only stream
// (no context) never reaches one that does anything.  A stream opened on
// sanitize_fake_ctx() gets a scripted stand-in for the device, so that the host
// paths that follow a launch run under the sanitizers too: it searches
// nothing, follows every index the host hands it (items, words, migrations,
// live lists -- out-of-range ones are the sanitizer's to report) and lets a
// key die in the set tier at its DIE_AT-th :ok there -- invalid, at the budget
// or fallen back, by key index; every fourth key stays live -- with a Final of
// made-up configs in exact mode.  lc_check_batch answers "valid" for the keys that fell back.
#include <algorithm>
#include <vector>

#include "../../jepsen-etcd-demo_amd/csrc/common.hpp"
#include "../../jepsen-etcd-demo_amd/csrc/device_stream.hpp"
#include "../../jepsen-etcd-demo_amd/csrc/stream_plan.hpp"

static int fake_ctx_storage;
extern "C" lc_ctx *sanitize_fake_ctx() { return reinterpret_cast<lc_ctx *>(&fake_ctx_storage); }

struct lcst::StreamDev {
    bool exact = false;
    std::vector<uint64_t> sent;      // per key: events taken so far
    std::vector<uint32_t> set_oks;   // per key: :ok words taken in the set tier
    std::vector<int32_t> free_slots;
    int32_t slots = 0, used = 0, peak = 0;
};

namespace lcst {
namespace {
constexpr int MAX_FINAL = 10;
constexpr uint32_t DIE_AT = 3;
int none() { return lc::fail(LC_E_DEVICE, "sanitizer build: no device half"); }
void keys_upto(StreamDev *d, int64_t n) {
    if ((int64_t)d->sent.size() < n) {
        d->sent.resize((size_t)n, 0);
        d->set_oks.resize((size_t)n, 0);
    }
}
}  // namespace

int stream_dev_open(lc_ctx *c, bool exact, StreamDev **out) {
    if (c != sanitize_fake_ctx()) return none();
    *out = new StreamDev;
    (*out)->exact = exact;
    return LC_OK;
}
void stream_dev_close(StreamDev *d) { delete d; }
int stream_dev_max_final(const StreamDev *) { return MAX_FINAL; }

int stream_dev_push(StreamDev *d, int64_t n_keys, const Item *items, int64_t n_items, const uint16_t *ev16, uint64_t n_ev,
                    const uint32_t *trans, uint64_t n_trans, uint32_t, std::vector<Dead> *dead, const SetWork *set,
                    std::vector<Final> *fin) {
    dead->clear();
    if (fin) fin->clear();
    if (!d) return none();
    keys_upto(d, n_keys);
    uint64_t touched = 0;  // every word and transition is read, as a launch would
    for (int64_t i = 0; i < n_items; ++i) {
        const Item &it = items[i];
        for (uint32_t j = it.ev_b; j < it.ev_e && j < n_ev; ++j) touched += ev16[j];
        for (uint32_t j = 0; j < it.ntr && it.tr_b + j < n_trans; ++j) touched += trans[it.tr_b + j];
        d->sent[(size_t)it.key] += it.ev_e - it.ev_b;
    }
    for (int64_t i = 0; set && i < set->n_mig; ++i)
        for (int j = 0; j < 64; ++j) touched += set->mig[i].descs[j];
    for (int64_t i = 0; set && i < set->n_items; ++i) {
        const SetItem &it = set->items[i];
        const size_t k = (size_t)it.key;
        uint32_t j = it.ev_b;
        for (; j < it.ev_e && j < set->n_ev32; ++j) {
            touched += set->ev32[j];
            if ((set->ev32[j] & LC_EV_OK_BIT) && ++d->set_oks[k] == DIE_AT && k % 4 != 3) break;
        }
        for (uint32_t t = 0; t < it.ntr && it.tr_b + t < n_trans; ++t) touched += trans[it.tr_b + t];
        if (j < it.ev_e) {
            const uint32_t status = k % 4 == 0 ? lc::STREAM_INVALID : k % 4 == 1 ? lc::STREAM_BUDGET : lc::STREAM_SET_FALLBACK;
            dead->push_back(Dead{(uint32_t)k, status, (uint32_t)(d->sent[k] + (j - it.ev_b)), 0u});
        }
        d->sent[k] += it.ev_e - it.ev_b;
    }
    if (touched == ~0ull) return none();  // (keeps the reads)
    std::sort(dead->begin(), dead->end(), [](const Dead &x, const Dead &y) { return x.key < y.key; });
    if (d->exact && fin) {
        fin->assign(dead->size(), Final{});
        for (size_t i = 0; i < dead->size(); ++i) {
            if ((*dead)[i].status != lc::STREAM_INVALID && (*dead)[i].status != lc::STREAM_BUDGET) continue;
            Final &f = (*fin)[i];
            f.peak = 7;
            f.n_final = 2;
            f.cfg[0] = 1; f.cfg[1] = 0;              // (slot 0 linearized, state nil)
            f.cfg[2] = 3; f.cfg[3] = 0;
        }
    }
    return LC_OK;
}

int stream_dev_peaks(StreamDev *d, int64_t n_keys, uint32_t *out) {
    if (!d) return none();
    for (int64_t i = 0; i < n_keys; ++i) out[i] = 1 + (uint32_t)(i % 5);
    return LC_OK;
}

int stream_dev_finals(StreamDev *d, int64_t n_keys, const int32_t *keys, int64_t n_live, uint32_t, uint64_t *cfg,
                      uint32_t *n_final, const SetLive *set_live, int64_t n_set_live) {
    if (!d) return none();
    std::fill(cfg, cfg + n_keys * MAX_FINAL * 2, 0ull);
    std::fill(n_final, n_final + n_keys, 0u);
    for (int64_t i = 0; i < n_live; ++i) n_final[keys[i]] = 1;  // (the nil state, nothing pending)
    for (int64_t i = 0; i < n_set_live; ++i) {
        const int32_t k = set_live[i].key;
        if (set_live[i].slot < 0 || set_live[i].slot >= d->slots) return lc::fail(LC_E_INVALID, "stub: a live set key without a slot");
        n_final[k] = 2;
        cfg[((size_t)k * MAX_FINAL + 1) * 2] = 1ull << 11;  // (window slot 11 linearized)
    }
    return LC_OK;
}
double stream_dev_final_ms(const StreamDev *) { return 0; }

int stream_dev_set_alloc(StreamDev *d, int32_t *slot) {
    if (!d) return none();
    if (d->free_slots.empty()) d->free_slots.push_back(d->slots++);
    *slot = d->free_slots.back();
    d->free_slots.pop_back();
    d->peak = std::max(d->peak, ++d->used);
    return LC_OK;
}
void stream_dev_set_free(StreamDev *d, int32_t slot) {
    if (!d || slot < 0 || slot >= d->slots) return;
    d->free_slots.push_back(slot);
    --d->used;
}
int stream_dev_set_record(StreamDev *, int32_t, int64_t, uint32_t *, int64_t) { return none(); }
void stream_dev_set_stats(const StreamDev *d, double *out6) {
    if (!d) return;
    out6[2] = d->slots; out6[3] = d->used; out6[4] = d->peak;
}
int stream_dev_record(StreamDev *, int64_t, uint32_t *) { return none(); }
void stream_dev_timing(const StreamDev *, double *) {}
}  // namespace lcst

// lc_stream_finish checks deferred keys through the batch path: only with a
// context.  The fake one: every key valid, one final config, every word read.
extern "C" int lc_check_batch(lc_ctx *c, const lc_batch *b, lc_result *r, lc_stats *) {
    if (c != sanitize_fake_ctx()) return lcst::none();
    uint64_t touched = 0;
    for (int64_t k = 0; k < b->n_keys; ++k) {
        for (uint64_t j = b->ev_off[k]; j < b->ev_off[k + 1]; ++j) touched += b->events[j];
        touched += b->key_width[k] + b->key_states[k] + (b->trans_off[k] < (uint64_t)b->n_trans ? b->trans[b->trans_off[k]] : 0u);
        r->valid[k] = LC_VALID;
        r->cause[k] = LC_CAUSE_NONE;
        r->fail_event[k] = -1;
        if (r->peak_configs) r->peak_configs[k] = 3;
        if (r->n_final) r->n_final[k] = 1;
        if (r->final_configs) {
            uint64_t *o = r->final_configs + (size_t)k * lcst::MAX_FINAL * 2;
            std::fill(o, o + lcst::MAX_FINAL * 2, 0ull);
        }
    }
    return touched == ~0ull ? LC_E_DEVICE : LC_OK;
}
