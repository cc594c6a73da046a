// lc_report: the Knossos-shaped counterexample of one key, rendered from its
// verdict record and the final configs the device returned (SURVEY.md 8(a)
// A8, 8(f) F-2).  jepsen.checker/linearizable (etcdemo.clj:117-118) reports,
// for an invalid key, the :ok that could not be linearized (:op), the last
// :ok before it (:previous-ok / :last-op), the config set standing before it
// (:configs) and :final-paths -- from each of those configs, every sequence of
// further pending ops the model allows, ending with the failing op, which is
// inconsistent in every state so reached (that is why the set emptied).
// Knossos iterates a hash set here, so only the SET of paths is comparable;
// paths are generated depth-first, shortest first, from the configs in device
// order, up to max_paths distinct ones (jepsen truncates to 10).  Both
// bindings (Python lincheck.checker, the JVM's gpu_checker.clj) decode this
// one rendering.
//
// lc_report_wgl shapes the same key for :algorithm :wgl (knossos.wgl, SURVEY
// 8(f) F-3; parity unpinned -- restated in oracle/wgl_ref.py).  The Wing-Gong
// search with Lowe's cache gets stuck, at its deepest, on the same :ok (the
// first whose prefix cannot be linearized: a property of the history), and
// its frontier there is every (model, linearized pending ops) it reached at
// that return entry: the closure of the config set standing before the :ok
// under the pending ops other than the failing one.  :configs are those
// frontier configs, breadth first from the device's configs (so a subset of
// the frontier when the device truncated them); :op, :previous-ok,
// :last-op and :final-paths are shaped as for :linear.

#include "common.hpp"
#include "packed.hpp"
#include "report_core.hpp"

namespace {

// A key of an lc_packed as the rendering's source (report_core.hpp).
struct PackedSrc {
    const lc_packed *p;
    int64_t key;
    uint64_t eb, ne;            // the key's events: [eb, eb + ne)
    PackedSrc(const lc_packed *pk, int64_t k) : p(pk), key(k) {
        eb = p->ev_off[(size_t)k];
        ne = p->ev_off[(size_t)k + 1] - eb;
    }
    uint64_t n() const { return ne; }
    uint32_t word(uint64_t j) const { return p->word(eb + j); }
    int64_t row(uint64_t j) const { return p->event_row((size_t)key, eb + j); }
    uint32_t step(uint32_t w, uint32_t st) const {
        const uint64_t tb = p->trans_off.empty() ? 0 : p->trans_off[(size_t)key];
        const uint32_t d = p->trans[tb + LC_EV_TRANS(w)];
        if (p->table.empty()) return lcr::desc_step(d, st);
        const uint16_t s2 = p->table[(size_t)d + st];  // a table-model row (lc_batch.table)
        return s2 == LC_TABLE_NONE ? LC_STATE_NONE : s2;
    }
    int64_t late_done_row(uint32_t) const { return -1; }  // every event of the key is in the words
    int64_t value(uint32_t st) const {
        if (p->model == LC_MODEL_MULTI_REGISTER) return st;  // a map: lc_packed_state_map
        if (st == 0) return LC_NIL;
        const uint64_t base = p->state_off.empty() ? 0 : p->state_off[(size_t)key];
        const uint64_t lim = p->state_off.empty() ? p->state_vals.size() : p->state_off[(size_t)key + 1];
        return base + st < lim ? p->state_vals[base + st] : LC_NIL;
    }
};

}  // namespace

static int64_t report(const lc_packed *p, int64_t key, int32_t valid, int32_t fail_event,
                      const uint64_t *final_configs, uint32_t n_final, int32_t max_paths, bool wgl, int64_t *out,
                      int64_t cap) {
    if (!p || key < 0 || key >= (int64_t)p->keys.size() || (n_final && !final_configs) || cap < 0 ||
        (cap && !out))
        return lc::fail(LC_E_INVALID, "lc_report: bad argument");
    if (!p->key_error.empty() && p->key_error[(size_t)key])
        return lc::fail(LC_E_INVALID, "lc_report: key %lld could not be prepared: %s", (long long)key,
                        p->key_msg[(size_t)key].c_str());
    return lcr::report(PackedSrc(p, key), valid, fail_event, final_configs, n_final, max_paths, wgl, out, cap);
}

extern "C" int64_t lc_report(const lc_packed *p, int64_t key, int32_t valid, int32_t fail_event,
                             const uint64_t *final_configs, uint32_t n_final, int32_t max_paths, int64_t *out,
                             int64_t cap) {
    return report(p, key, valid, fail_event, final_configs, n_final, max_paths, false, out, cap);
}

extern "C" int64_t lc_report_wgl(const lc_packed *p, int64_t key, int32_t valid, int32_t fail_event,
                                 const uint64_t *final_configs, uint32_t n_final, int32_t max_paths, int64_t *out,
                                 int64_t cap) {
    return report(p, key, valid, fail_event, final_configs, n_final, max_paths, true, out, cap);
}

extern "C" int lc_packed_keys(const lc_packed *p, int64_t *out) {
    if (!p || (!out && !p->keys.empty())) return lc::fail(LC_E_INVALID, "lc_packed_keys: null argument");
    std::copy(p->keys.begin(), p->keys.end(), out);
    return LC_OK;
}
