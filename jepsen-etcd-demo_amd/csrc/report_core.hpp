// report_core.hpp -- the rendering of one key's Knossos-shaped result, shared
// by lc_report / lc_report_wgl (host_report.cpp: a key of an lc_packed) and
// lc_stream_report (host_stream.cpp: a key of a stream).  The words written
// are described in include/lincheck.h; how they are chosen, in
// host_report.cpp's head comment.  Host code.
#pragma once

#include <algorithm>
#include <set>
#include <vector>

#include "common.hpp"

namespace lcr {

// One interned transition from state st (include/lincheck.h LC_DESC): the
// next state, or LC_STATE_NONE when the model step is inconsistent.
inline uint32_t desc_step(uint32_t d, uint32_t st) {
    const uint32_t t = d & 3u, a = (d >> 2) & 0x7FFFu, b = d >> 17;
    if (t == LC_T_READ_ANY) return st;
    if (t == LC_T_READ) return st == a ? st : LC_STATE_NONE;
    if (t == LC_T_WRITE) return b;
    return st == a ? b : LC_STATE_NONE;
}

// A key as the rendering reads it, over a source Src of its own words:
//   uint64_t n() const               its events
//   uint32_t word(uint64_t j) const  event j, 32-bit form
//   int64_t row(uint64_t j) const    the history row of event j
//   uint32_t step(uint32_t w, uint32_t st) const  the op of invoke word w from
//                                    state st: the next state or LC_STATE_NONE
//   int64_t value(uint32_t st) const the register value of state st
//   int64_t late_done_row(uint32_t slot) const  the completion row of the op
//                                    pending in `slot` at the end of the words,
//                                    where it is known already, else -1
// PackedSrc (host_report.cpp) reads an lc_packed, host_stream.cpp's source a
// stream's per-key words, transitions, state values and event rows.
template <class Src>
struct KeyView {
    const Src &p;
    uint64_t n;                 // the key's events
    // (slot, invoke event (ordinal)) holding it at `upto`, in slot order.
    // Built from a per-slot array in one pass: a std::map updated at every
    // event was most of a C5 counterexample's rendering (~70 us per key).
    std::vector<std::pair<uint32_t, uint64_t>> held;
    int64_t last_ok = -1;       // last :ok event before `upto`

    KeyView(const Src &src, uint64_t upto) : p(src) {
        n = p.n();
        upto = std::min<uint64_t>(upto, n);
        constexpr uint32_t NS = 128;  // LC_EV_SLOT's range
        uint64_t at[NS];
        bool on[NS] = {};
        for (uint64_t j = 0; j < upto; ++j) {
            const uint32_t w = p.word(j);
            const uint32_t s = LC_EV_SLOT(w);
            if (w & LC_EV_OK_BIT) {
                on[s] = false;
                last_ok = (int64_t)j;
            } else {
                on[s] = true;
                at[s] = j;
            }
        }
        for (uint32_t s = 0; s < NS; ++s)
            if (on[s]) held.push_back({s, at[s]});
    }
    const std::pair<uint32_t, uint64_t> *find(uint32_t s) const {
        for (const auto &h : held)
            if (h.first == s) return &h;
        return nullptr;
    }
    int64_t row(uint64_t j) const { return p.row(j); }
    // the row completing invoke event j (its slot's next event, when an :ok)
    int64_t done_row(uint64_t j) const {
        const uint32_t s = LC_EV_SLOT(p.word(j));
        for (uint64_t i = j + 1; i < n; ++i) {
            const uint32_t w = p.word(i);
            if (LC_EV_SLOT(w) == s) return (w & LC_EV_OK_BIT) ? row(i) : -1;
        }
        return p.late_done_row(s);
    }
    // the op of invoke event j from state st: next state or LC_STATE_NONE
    uint32_t step(uint64_t j, uint32_t st) const { return p.step(p.word(j), st); }
    int64_t value(uint32_t st) const { return p.value(st); }
};

template <class Src>
int64_t report(const Src &src, int32_t valid, int32_t fail_event,
                      const uint64_t *final_configs, uint32_t n_final, int32_t max_paths, bool wgl, int64_t *out,
                      int64_t cap) {
    if ((n_final && !final_configs) || cap < 0 || (cap && !out)) return lc::fail(LC_E_INVALID, "lc_report: bad argument");
    const uint64_t n_ev = src.n();
    if (fail_event >= 0 && (uint64_t)fail_event >= n_ev) return lc::fail(LC_E_INVALID, "lc_report: bad fail_event");
    const uint64_t upto = fail_event >= 0 ? (uint64_t)fail_event : n_ev;
    try {
        KeyView<Src> kv(src, upto);
        std::vector<int64_t> o;
        o.push_back(fail_event >= 0 ? kv.row((uint64_t)fail_event) : -1);
        o.push_back(kv.last_ok >= 0 ? kv.row((uint64_t)kv.last_ok) : -1);
        o.push_back(0);  // n_configs
        o.push_back(0);  // n_paths
        // final configs: {state, slot mask} as the device writes them
        std::vector<std::pair<uint32_t, std::pair<uint64_t, uint64_t>>> finals;
        for (uint32_t c = 0; c < n_final; ++c) {
            const uint64_t lo = final_configs[2 * c], hi = final_configs[2 * c + 1];
            finals.push_back({(uint32_t)((hi >> 48) & 0x7FFFu), {lo, hi & ((1ull << 48) - 1)}});
        }
        auto in_mask = [](const std::pair<uint64_t, uint64_t> &m, uint32_t s) {
            return s < 64 ? ((m.first >> s) & 1) != 0 : ((m.second >> (s - 64)) & 1) != 0;
        };
        const uint32_t p_slot = fail_event >= 0 ? LC_EV_SLOT(src.word((uint64_t)fail_event)) : 0xFFFFFFFFu;
        const size_t want = (size_t)std::max(max_paths, 0);
        std::vector<std::pair<uint32_t, std::pair<uint64_t, uint64_t>>> shown(
            finals.begin(), finals.begin() + (ptrdiff_t)std::min(finals.size(), want));
        if (wgl && valid == LC_INVALID && fail_event >= 0) {
            // WGL's frontier at the stuck return entry: breadth first from the
            // device's configs, every legal linearization of a further pending
            // op other than the failing one, each distinct config once
            std::set<std::pair<uint32_t, std::pair<uint64_t, uint64_t>>> seen(finals.begin(), finals.end());
            std::vector<std::pair<uint32_t, std::pair<uint64_t, uint64_t>>> q(finals.begin(), finals.end());
            for (size_t at = 0; at < q.size() && shown.size() < want && seen.size() < (1u << 16); ++at) {
                const auto c = q[at];
                for (auto &h : kv.held) {
                    if (h.first == p_slot || in_mask(c.second, h.first)) continue;
                    const uint32_t s2 = kv.step(h.second, c.first);
                    if (s2 == LC_STATE_NONE) continue;
                    auto m2 = c.second;
                    if (h.first < 64) m2.first |= 1ull << h.first;
                    else m2.second |= 1ull << (h.first - 64);
                    const std::pair<uint32_t, std::pair<uint64_t, uint64_t>> c2{s2, m2};
                    if (!seen.insert(c2).second) continue;
                    q.push_back(c2);
                    if (shown.size() < want) shown.push_back(c2);
                }
            }
        }
        const size_t n_cfg = shown.size();
        for (size_t c = 0; c < n_cfg; ++c) {
            o.push_back(kv.value(shown[c].first));
            for (int lin = 0; lin < 2; ++lin) {
                const size_t at = o.size();
                o.push_back(0);
                for (auto &h : kv.held)
                    if (in_mask(shown[c].second, h.first) == (lin == 1)) {
                        o.push_back(kv.row(h.second));
                        o.push_back(kv.done_row(h.second));
                        ++o[at];
                    }
            }
        }
        o[2] = (int64_t)n_cfg;
        if (valid == LC_INVALID && fail_event >= 0 && max_paths > 0) {
            const auto *ph = kv.find(p_slot);
            if (ph) {
                const uint64_t p_inv = ph->second;
                std::vector<std::pair<uint32_t, uint64_t>> others;  // (slot, invoke event)
                for (auto &h : kv.held)
                    if (h.first != p_slot) others.push_back(h);
                std::set<std::vector<uint64_t>> seen;
                std::vector<std::pair<uint64_t, uint32_t>> steps;  // (invoke event, state after)
                int64_t visits = 0, n_paths = 0;
                const int64_t max_visits = 1 << 16;
                uint32_t st0 = 0;
                auto emit = [&](uint32_t st) {
                    std::vector<uint64_t> id{st0};
                    for (auto &s : steps) id.push_back(s.first);
                    if (!seen.insert(id).second) return;
                    o.push_back(kv.value(st0));
                    o.push_back((int64_t)steps.size());
                    for (auto &s : steps) {
                        o.push_back(kv.row(s.first));
                        o.push_back(kv.done_row(s.first));
                        o.push_back(kv.value(s.second));
                    }
                    o.push_back(kv.value(st));  // the state the failing op cannot be stepped in
                    ++n_paths;
                };
                std::vector<char> used(others.size(), 0);
                auto dfs = [&](auto &&self, uint32_t st) -> void {
                    ++visits;
                    if (n_paths >= max_paths || visits > max_visits) return;
                    if (kv.step(p_inv, st) == LC_STATE_NONE) emit(st);
                    for (size_t q = 0; q < others.size(); ++q) {
                        if (used[q]) continue;
                        const uint32_t s2 = kv.step(others[q].second, st);
                        if (s2 == LC_STATE_NONE) continue;
                        used[q] = 1;
                        steps.push_back({others[q].second, s2});
                        self(self, s2);
                        steps.pop_back();
                        used[q] = 0;
                        if (n_paths >= max_paths || visits > max_visits) return;
                    }
                };
                for (auto &f : finals) {
                    if (n_paths >= max_paths) break;
                    st0 = f.first;
                    for (size_t q = 0; q < others.size(); ++q) used[q] = in_mask(f.second, others[q].first);
                    dfs(dfs, st0);
                }
                o[3] = n_paths;
            }
        }
        if ((int64_t)o.size() <= cap) std::copy(o.begin(), o.end(), out);
        return (int64_t)o.size();
    } catch (const std::bad_alloc &) {
        return lc::fail(LC_E_NOMEM, "lc_report: out of memory");
    }
}

}  // namespace lcr
