// host_setfull_stream.cpp -- lc_setfull_stream_*: the packer of a streaming
// set-full and its entry points (include/lincheck_setfull_stream.h has the
// contract).  Single-threaded, as host_stream.cpp.
//
// The packer carries, per key, what of jepsen.checker/set-full's fold is not
// per (read, element): the value-to-id map (ids in order of first appearance,
// an :invoke :add or a value inside an :ok :read), the open read of every
// process, per id the position of its last :invoke :add and whether an :ok
// :add has been seen since, and the error rules (host_setfull.cpp's, in the
// same order).  Each append becomes one CHUNK (lc_setfull_stream_chunk):
//   * per touched id one entry: FRESH with the position of the chunk's LAST
//     :invoke :add of it (an earlier one is discarded by the fold anyway),
//     ACK with the first :ok :add after the current invocation;
//   * the new :ok reads per key in completion order, with their invocation's
//     position and time, and their values as ids.
// The largest multiplicity of an id inside one read is counted here (a stamp
// per id), before the lists are dropped: the device only flags THAT an id was
// held twice.
// Ids live in blocks of 256 (setfull_stream_plan.hpp); a key takes the next
// free block when its ids outgrow the ones it owns.
// No HIP here: the device half is device_setfull_stream.hpp's, and a stream
// opened without a context never reaches it.

#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "common.hpp"
#include "device_setfull_stream.hpp"
#include "setfull_stream_plan.hpp"

namespace {

struct Entry {
    uint32_t id, flags;
    int64_t inv_pos, ack_pos, ack_time;
};

struct OpenRead {
    int64_t pos, time;
};

struct KeyState {
    bool bad = false;
    std::string error;
    std::unordered_map<int64_t, uint32_t> id_of;
    std::vector<int64_t> elems;                    // id -> element
    std::unordered_map<int64_t, OpenRead> open;    // process -> its open :read invocation
    std::vector<int64_t> inv_pos;                  // per id: its last :invoke :add, or LC_SETFULL_NONE
    std::vector<uint8_t> acked;                    // per id: an :ok :add seen since
    std::vector<uint32_t> mult;                    // per id: largest multiplicity in one read
    std::vector<uint64_t> stamp;                   // per id: the read that last held it ...
    std::vector<uint32_t> stamp_n;                 // ... and how often so far
    std::vector<uint32_t> blocks;                  // resident block numbers
    // the current chunk
    uint64_t touched_in = 0;                       // the append that last touched the key (1-based)
    std::vector<uint32_t> entry_of;                // per id: 1 + its entry in `entries`, this chunk
    std::vector<uint64_t> entry_chunk;             // per id: the append entry_of is of
    std::vector<Entry> entries;
    std::vector<int64_t> row_pos, row_time, row_inv_pos, row_inv_time;
    std::vector<uint64_t> row_els;                 // elements per row
    std::vector<uint32_t> read_id;
    void fail(const char *why) {
        if (!bad) error = why;
        bad = true;
    }
    void drop_chunk() {
        entries.clear();
        row_pos.clear(); row_time.clear(); row_inv_pos.clear(); row_inv_time.clear(); row_els.clear(); read_id.clear();
    }
};

struct Chunk {
    std::vector<int64_t> tk_key;
    std::vector<uint32_t> tk_n_ids, blk, en_t, en_id, en_flags, read_id;
    std::vector<uint64_t> tk_row_off, tk_blk_off, el_off;
    std::vector<int64_t> en_inv_pos, en_ack_pos, en_ack_time, row_pos, row_time, row_inv_pos, row_inv_time;
    void clear() {
        tk_key.clear(); tk_n_ids.clear(); blk.clear(); en_t.clear(); en_id.clear(); en_flags.clear(); read_id.clear();
        tk_row_off.assign(1, 0); tk_blk_off.assign(1, 0); el_off.assign(1, 0);
        en_inv_pos.clear(); en_ack_pos.clear(); en_ack_time.clear();
        row_pos.clear(); row_time.clear(); row_inv_pos.clear(); row_inv_time.clear();
    }
};

}  // namespace

struct lc_setfull_stream {
    lc_ctx *ctx = nullptr;
    lcfs::SfsDev *dev = nullptr;
    lc_setfull_opts o{};
    int keyed = -1;        // -1: no client row yet
    bool broken = false;   // a device step failed half way: the records are not what the packer thinks
    int64_t rows = 0;
    uint64_t appends = 0, reads_seen = 0;
    uint64_t n_blocks = 0;
    std::vector<int64_t> keys;
    std::unordered_map<int64_t, int32_t> key_index;
    std::vector<KeyState> ks;
    std::vector<int8_t> valid;
    std::vector<uint64_t> counts;
    std::vector<int64_t> changed;
    Chunk chunk;
    std::vector<int32_t> touched;  // keys of the current append, in order of first touch
    double ms[6] = {0, 0, 0, 0, 0, 0};
    // scratch of results()
    std::vector<uint8_t> t_outcome, t_dup;
    std::vector<int64_t> t_lat, t_known, t_la;
    std::vector<int8_t> t_valid;
    std::vector<uint64_t> t_counts;
};

namespace {

int32_t add_key(lc_setfull_stream *s, int64_t k) {
    const int32_t i = (int32_t)s->keys.size();
    s->keys.push_back(k);
    s->key_index.emplace(k, i);
    s->ks.emplace_back();
    s->valid.push_back(LC_UNKNOWN);
    s->counts.insert(s->counts.end(), 6, 0);
    return i;
}

// The id of v in key a, a new one (and a new block when the key's are full) on first sight.
int intern(lc_setfull_stream *s, KeyState &a, int64_t v, uint32_t *out) {
    auto it = a.id_of.find(v);
    if (it != a.id_of.end()) {
        *out = it->second;
        return LC_OK;
    }
    const uint64_t id = a.elems.size();
    if (id == (uint64_t)a.blocks.size() * lcfs::SFS_BLOCK_IDS) {
        if (s->n_blocks >= lcfs::SFS_MAX_BLOCKS) return lc::fail(LC_E_INVALID, "lc_setfull_stream_append: more than 2^32 element ids");
        a.blocks.push_back((uint32_t)s->n_blocks++);
    }
    a.id_of.emplace(v, (uint32_t)id);
    a.elems.push_back(v);
    a.inv_pos.push_back(LC_SETFULL_NONE);
    a.acked.push_back(0);
    a.mult.push_back(0);
    a.stamp.push_back(0);
    a.stamp_n.push_back(0);
    a.entry_of.push_back(0);
    a.entry_chunk.push_back(0);
    *out = (uint32_t)id;
    return LC_OK;
}

Entry &entry(lc_setfull_stream *s, KeyState &a, uint32_t id) {
    if (a.entry_chunk[id] != s->appends || a.entry_of[id] == 0) {
        a.entry_chunk[id] = s->appends;
        a.entries.push_back({id, 0u, LC_SETFULL_NONE, LC_SETFULL_NONE, 0});
        a.entry_of[id] = (uint32_t)a.entries.size();
    }
    return a.entries[a.entry_of[id] - 1];
}

// Refusals: nothing of the stream has changed when one of them fires.
int refuse(const lc_setfull_stream *s, const lc_setfull_history *h, int *kind) {
    const int64_t n = h->n;
    if (n < 0) return lc::fail(LC_E_INVALID, "lc_setfull_stream_append: n < 0");
    if (n > 0 && (!h->type || !h->f || !h->elem)) return lc::fail(LC_E_INVALID, "lc_setfull_stream_append: null column");
    for (int64_t r = 0; r < n; ++r)
        if (h->type[r] > LC_INFO || h->f[r] > LC_SF_OTHER)
            return lc::fail(LC_E_INVALID, "lc_setfull_stream_append: row %lld: bad :type / :f code", (long long)r);
    if (h->read_off) {
        if (h->read_off[0] < 0) return lc::fail(LC_E_INVALID, "lc_setfull_stream_append: read_off[0] < 0");
        for (int64_t r = 0; r < n; ++r)
            if (h->read_off[r + 1] < h->read_off[r])
                return lc::fail(LC_E_INVALID, "lc_setfull_stream_append: read_off not ascending at row %lld", (long long)r);
        if (h->read_off[n] > 0 && !h->read_elem) return lc::fail(LC_E_INVALID, "lc_setfull_stream_append: read_elem is null");
    }
    bool client = false, has_key = false;
    for (int64_t r = 0; r < n; ++r) {
        client |= h->f[r] != LC_SF_OTHER;
        has_key |= h->key && h->key[r] != LC_NO_KEY;
    }
    *kind = has_key ? 1 : client ? 0 : -1;
    if (*kind >= 0 && s->keyed >= 0 && *kind != s->keyed)
        return lc::fail(LC_E_INVALID, "lc_setfull_stream_append: %s rows appended to a stream of %s rows",
                        *kind ? "keyed" : "unkeyed", s->keyed ? "keyed" : "unkeyed");
    return LC_OK;
}

int pack_rows(lc_setfull_stream *s, const lc_setfull_history *h) {
    const int64_t n = h->n;
    const bool keyed = s->keyed == 1;
    if (s->keyed == 0 && s->keys.empty()) add_key(s, LC_NO_KEY);
    int64_t last = LC_NO_KEY;
    int32_t last_i = -1;
    for (int64_t r = 0; r < n; ++r) {
        const int64_t pos = s->rows + r;
        int32_t ki = 0;
        if (keyed) {
            const int64_t k = h->key ? h->key[r] : LC_NO_KEY;
            if (k != last) {
                last = k;
                if (k == LC_NO_KEY) {
                    last_i = -1;
                } else {
                    auto it = s->key_index.find(k);
                    if (it == s->key_index.end()) {
                        if (s->keys.size() >= 0x7FFFFFF0u) return lc::fail(LC_E_INVALID, "lc_setfull_stream_append: more than 2^31 keys");
                        last_i = add_key(s, k);
                    } else {
                        last_i = it->second;
                    }
                }
            }
            ki = last_i;
            if (ki < 0) continue;
        } else if (s->keyed < 0) {
            continue;  // no client row yet: nothing to fold
        }
        KeyState &a = s->ks[(size_t)ki];
        if (a.bad || h->f[r] == LC_SF_OTHER) continue;
        const int64_t proc = h->process ? h->process[r] : 0;
        if (proc == LC_NO_PROCESS) continue;
        const uint8_t t = h->type[r];
        const int64_t time = h->time ? h->time[r] : 0;
        auto touch = [&]() {
            if (a.touched_in != s->appends) {
                a.touched_in = s->appends;
                s->touched.push_back(ki);
            }
        };
        if (h->f[r] == LC_SF_ADD) {
            if (t != LC_INVOKE && t != LC_OK_T) continue;
            const int64_t v = h->elem[r];
            touch();
            if (v == LC_NIL) { a.fail("a set element is nil or not an integer"); continue; }
            if (t == LC_INVOKE) {
                uint32_t id;
                if (int rc = intern(s, a, v, &id)) return rc;
                a.inv_pos[id] = pos;
                a.acked[id] = 0;
                Entry &e = entry(s, a, id);
                e.flags = LC_SFS_FRESH;
                e.inv_pos = pos;
                e.ack_pos = LC_SETFULL_NONE;
                e.ack_time = 0;
            } else {
                auto it = a.id_of.find(v);
                if (it == a.id_of.end() || a.inv_pos[it->second] == LC_SETFULL_NONE) {
                    a.fail("an :ok :add of an element with no earlier :invoke :add");
                    continue;
                }
                const uint32_t id = it->second;
                if (!a.acked[id]) {
                    a.acked[id] = 1;
                    Entry &e = entry(s, a, id);
                    e.flags |= LC_SFS_ACK;
                    e.ack_pos = pos;
                    e.ack_time = time;
                }
            }
        } else if (t == LC_INVOKE) {
            a.open[proc] = {pos, time};
        } else if (t == LC_FAIL) {
            a.open.erase(proc);
        } else if (t == LC_OK_T) {
            touch();
            auto it = a.open.find(proc);
            if (it == a.open.end()) { a.fail("an :ok :read by a process with no open :read invocation"); continue; }
            const int64_t rb = h->read_off ? h->read_off[r] : 0, re = h->read_off ? h->read_off[r + 1] : 0;
            bool nil = false;
            for (int64_t i = rb; i < re && !nil; ++i) nil = h->read_elem[i] == LC_NIL;
            if (nil) { a.fail("a :read value is no collection, or holds nil or a non-integer"); continue; }
            const uint64_t serial = ++s->reads_seen;
            for (int64_t i = rb; i < re; ++i) {
                uint32_t id;
                if (int rc = intern(s, a, h->read_elem[i], &id)) return rc;
                if (a.stamp[id] == serial) {
                    a.mult[id] = std::max(a.mult[id], ++a.stamp_n[id]);
                } else {
                    a.stamp[id] = serial;
                    a.stamp_n[id] = 1;
                }
                a.read_id.push_back(id);
            }
            a.row_pos.push_back(pos); a.row_time.push_back(time);
            a.row_inv_pos.push_back(it->second.pos); a.row_inv_time.push_back(it->second.time);
            a.row_els.push_back((uint64_t)(re - rb));
        }
    }
    return LC_OK;
}

// The touched keys' chunk parts, one after the other; error keys send nothing.
void build_chunk(lc_setfull_stream *s) {
    Chunk &c = s->chunk;
    c.clear();
    for (int32_t ki : s->touched) {
        KeyState &a = s->ks[(size_t)ki];
        if (a.bad) {
            a.drop_chunk();
            continue;
        }
        const uint32_t t = (uint32_t)c.tk_key.size();
        c.tk_key.push_back(ki);
        c.tk_n_ids.push_back((uint32_t)a.elems.size());
        c.blk.insert(c.blk.end(), a.blocks.begin(), a.blocks.end());
        c.tk_blk_off.push_back(c.blk.size());
        for (const Entry &e : a.entries) {
            c.en_t.push_back(t); c.en_id.push_back(e.id); c.en_flags.push_back(e.flags);
            c.en_inv_pos.push_back(e.inv_pos); c.en_ack_pos.push_back(e.ack_pos); c.en_ack_time.push_back(e.ack_time);
        }
        c.row_pos.insert(c.row_pos.end(), a.row_pos.begin(), a.row_pos.end());
        c.row_time.insert(c.row_time.end(), a.row_time.begin(), a.row_time.end());
        c.row_inv_pos.insert(c.row_inv_pos.end(), a.row_inv_pos.begin(), a.row_inv_pos.end());
        c.row_inv_time.insert(c.row_inv_time.end(), a.row_inv_time.begin(), a.row_inv_time.end());
        for (uint64_t n : a.row_els) c.el_off.push_back(c.el_off.back() + n);
        c.read_id.insert(c.read_id.end(), a.read_id.begin(), a.read_id.end());
        c.tk_row_off.push_back(c.row_pos.size());
        a.drop_chunk();
    }
}

void view_chunk(const Chunk &c, lc_setfull_stream_chunk *o) {
    o->n_touched = (int64_t)c.tk_key.size();
    o->tk_key = c.tk_key.data(); o->tk_n_ids = c.tk_n_ids.data();
    o->tk_row_off = c.tk_row_off.data(); o->tk_blk_off = c.tk_blk_off.data(); o->blk = c.blk.data();
    o->n_entries = (int64_t)c.en_t.size();
    o->en_t = c.en_t.data(); o->en_id = c.en_id.data(); o->en_flags = c.en_flags.data();
    o->en_inv_pos = c.en_inv_pos.data(); o->en_ack_pos = c.en_ack_pos.data(); o->en_ack_time = c.en_ack_time.data();
    o->row_pos = c.row_pos.data(); o->row_time = c.row_time.data();
    o->row_inv_pos = c.row_inv_pos.data(); o->row_inv_time = c.row_inv_time.data();
    o->el_off = c.el_off.data(); o->read_id = c.read_id.data();
}

int64_t total_ids(const lc_setfull_stream *s) {
    int64_t n = 0;
    for (const KeyState &a : s->ks)
        if (!a.bad) n += (int64_t)a.elems.size();
    return n;
}

int append(lc_setfull_stream *s, const lc_setfull_history *h, lc_setfull_stream_update *u) {
    const auto t0 = std::chrono::steady_clock::now();
    if (s->broken) return lc::fail(LC_E_INVALID, "lc_setfull_stream_append: an earlier append failed on the device; close the stream");
    int kind = -1;
    if (int rc = refuse(s, h, &kind)) return rc;
    if (s->keyed < 0) s->keyed = kind;
    ++s->appends;
    s->touched.clear();
    s->changed.clear();
    s->chunk.clear();
    const std::vector<int8_t> before = s->valid;
    int rc = pack_rows(s, h);
    if (rc) {
        s->broken = true;  // (2^31 keys or 2^32 ids: the packer stopped half way)
        return rc;
    }
    s->rows += h->n;
    build_chunk(s);
    for (int32_t ki : s->touched)
        if (s->ks[(size_t)ki].bad) {
            s->valid[(size_t)ki] = LC_UNKNOWN;
            std::fill(s->counts.begin() + 6 * ki, s->counts.begin() + 6 * ki + 6, 0);
        }
    std::fill(s->ms, s->ms + 6, 0.0);
    s->ms[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    const Chunk &c = s->chunk;
    if (s->dev && !c.tk_key.empty()) {
        lc_setfull_stream_chunk v;
        view_chunk(c, &v);
        const size_t T = c.tk_key.size();
        s->t_valid.assign(T, 0);
        s->t_counts.assign(6 * T, 0);
        rc = lcfs::sfs_dev_append(s->dev, &v, s->n_blocks, s->o.linearizable, s->o.max_matrix_bytes, s->t_valid.data(),
                                  s->t_counts.data(), s->ms + 1);
        if (rc) {
            s->broken = true;
            return rc;
        }
        for (size_t t = 0; t < T; ++t) {
            const size_t ki = (size_t)c.tk_key[t];
            s->valid[ki] = s->t_valid[t];
            std::copy(s->t_counts.begin() + 6 * t, s->t_counts.begin() + 6 * t + 6, s->counts.begin() + 6 * ki);
        }
    }
    if (s->dev)
        for (size_t k = 0; k < s->valid.size(); ++k)
            if (k >= before.size() ? s->valid[k] != LC_UNKNOWN : s->valid[k] != before[k]) s->changed.push_back((int64_t)k);
    if (u) {
        u->n_keys = (int64_t)s->keys.size();
        u->rows = s->rows;
        u->reads = (int64_t)c.row_pos.size();
        u->ids = total_ids(s);
        u->n_changed = (int64_t)s->changed.size();
        u->changed = s->changed.data();
    }
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

extern "C" int lc_setfull_stream_open(lc_ctx *ctx, const lc_setfull_opts *o, lc_setfull_stream **out) {
    if (!out) return lc::fail(LC_E_INVALID, "lc_setfull_stream_open: null out");
    *out = nullptr;
    if (o && o->flags) return lc::fail(LC_E_INVALID, "lc_setfull_stream_open: unknown flags 0x%x", o->flags);
    return guarded("lc_setfull_stream_open", [&]() -> int {
        lc_setfull_stream *s = new lc_setfull_stream;
        if (o) s->o = *o;
        s->ctx = ctx;
        s->chunk.clear();
        if (ctx) {
            if (!lcfs::sfs_dev_open) {
                delete s;
                return lc::fail(LC_E_UNSUPPORTED, "lc_setfull_stream_open: this build has no device half");
            }
            if (int rc = lcfs::sfs_dev_open(ctx, &s->dev)) {
                delete s;
                return rc;
            }
        }
        *out = s;
        return LC_OK;
    });
}

extern "C" void lc_setfull_stream_close(lc_setfull_stream *s) {
    if (!s) return;
    if (s->dev) lcfs::sfs_dev_close(s->dev);
    delete s;
}

extern "C" int lc_setfull_stream_append(lc_setfull_stream *s, const lc_setfull_history *rows, lc_setfull_stream_update *u) {
    lc::Range range("lc_setfull_stream_append");
    if (!s || !rows) return lc::fail(LC_E_INVALID, "lc_setfull_stream_append: null argument");
    return guarded("lc_setfull_stream_append", [&]() -> int { return append(s, rows, u); });
}

extern "C" int lc_setfull_stream_counts(lc_setfull_stream *s, int8_t *valid, uint64_t *counts) {
    if (!s || !valid || !counts) return lc::fail(LC_E_INVALID, "lc_setfull_stream_counts: null argument");
    if (!s->dev) return lc::fail(LC_E_UNSUPPORTED, "lc_setfull_stream_counts: a packer-only stream has no results");
    std::copy(s->valid.begin(), s->valid.end(), valid);
    std::copy(s->counts.begin(), s->counts.end(), counts);
    return LC_OK;
}

extern "C" int64_t lc_setfull_stream_ids(const lc_setfull_stream *s, int64_t key, int64_t *elems, int64_t cap) {
    if (!s || key < 0 || (size_t)key >= s->ks.size()) return lc::fail(LC_E_INVALID, "lc_setfull_stream_ids: no such key");
    const KeyState &a = s->ks[(size_t)key];
    if (a.bad) return 0;
    const int64_t n = (int64_t)a.elems.size();
    if (elems) std::copy(a.elems.begin(), a.elems.begin() + std::max<int64_t>(0, std::min(n, cap)), elems);
    return n;
}

extern "C" int lc_setfull_stream_multiplicity(const lc_setfull_stream *s, int64_t key, uint32_t *out, int64_t cap) {
    if (!s || !out || key < 0 || (size_t)key >= s->ks.size()) return lc::fail(LC_E_INVALID, "lc_setfull_stream_multiplicity: no such key");
    const KeyState &a = s->ks[(size_t)key];
    if (a.bad) return LC_OK;
    const int64_t n = (int64_t)a.mult.size();
    std::copy(a.mult.begin(), a.mult.begin() + std::max<int64_t>(0, std::min(n, cap)), out);
    return LC_OK;
}

extern "C" int lc_setfull_stream_results(lc_setfull_stream *s, lc_setfull_result *r) {
    if (!s || !r) return lc::fail(LC_E_INVALID, "lc_setfull_stream_results: null argument");
    if (!s->dev) return lc::fail(LC_E_UNSUPPORTED, "lc_setfull_stream_results: a packer-only stream has no results");
    if (s->broken) return lc::fail(LC_E_INVALID, "lc_setfull_stream_results: an earlier append failed on the device");
    return guarded("lc_setfull_stream_results", [&]() -> int {
        if (r->valid) std::copy(s->valid.begin(), s->valid.end(), r->valid);
        if (r->counts) std::copy(s->counts.begin(), s->counts.end(), r->counts);
        const int64_t n_ids = total_ids(s);
        if (n_ids == 0) return LC_OK;
        if (!r->outcome || !r->latency || !r->known || !r->last_absent || !r->duplicated)
            return lc::fail(LC_E_INVALID, "lc_setfull_stream_results: null per-id result array");
        const size_t slots = (size_t)s->n_blocks * lcfs::SFS_BLOCK_IDS;
        s->t_outcome.resize(slots); s->t_dup.resize(slots);
        s->t_lat.resize(slots); s->t_known.resize(slots); s->t_la.resize(slots);
        if (int rc = lcfs::sfs_dev_results(s->dev, s->n_blocks, s->t_outcome.data(), s->t_lat.data(), s->t_known.data(),
                                           s->t_la.data(), s->t_dup.data()))
            return rc;
        size_t at = 0;
        for (const KeyState &a : s->ks) {
            if (a.bad) continue;
            const size_t n = a.elems.size();
            for (size_t b = 0; b * lcfs::SFS_BLOCK_IDS < n; ++b) {
                const size_t m = std::min<size_t>(lcfs::SFS_BLOCK_IDS, n - b * lcfs::SFS_BLOCK_IDS);
                const size_t from = (size_t)a.blocks[b] * lcfs::SFS_BLOCK_IDS;
                std::copy_n(s->t_outcome.begin() + from, m, r->outcome + at);
                std::copy_n(s->t_dup.begin() + from, m, r->duplicated + at);
                std::copy_n(s->t_lat.begin() + from, m, r->latency + at);
                std::copy_n(s->t_known.begin() + from, m, r->known + at);
                std::copy_n(s->t_la.begin() + from, m, r->last_absent + at);
                at += m;
            }
        }
        return LC_OK;
    });
}

extern "C" int64_t lc_setfull_stream_keys(const lc_setfull_stream *s, int64_t *out) {
    if (!s) return lc::fail(LC_E_INVALID, "lc_setfull_stream_keys: null stream");
    if (out) std::copy(s->keys.begin(), s->keys.end(), out);
    return (int64_t)s->keys.size();
}

extern "C" const char *lc_setfull_stream_key_error(const lc_setfull_stream *s, int64_t i) {
    if (!s || i < 0 || (size_t)i >= s->ks.size() || !s->ks[(size_t)i].bad) return nullptr;
    return s->ks[(size_t)i].error.c_str();
}

extern "C" int lc_setfull_stream_last_chunk(const lc_setfull_stream *s, lc_setfull_stream_chunk *out) {
    if (!s || !out) return lc::fail(LC_E_INVALID, "lc_setfull_stream_last_chunk: null argument");
    view_chunk(s->chunk, out);
    return LC_OK;
}

extern "C" int lc_setfull_stream_last_timing(const lc_setfull_stream *s, double *out_ms) {
    if (!s || !out_ms) return lc::fail(LC_E_INVALID, "lc_setfull_stream_last_timing: null argument");
    std::copy(s->ms, s->ms + 6, out_ms);
    return LC_OK;
}
