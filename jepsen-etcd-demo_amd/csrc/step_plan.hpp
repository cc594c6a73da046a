// Which kernels one search step runs: every rule of dev_search
// (device_api.hip) as a pure function of plain values, so the choice is
// tested as a choice, without a GPU (tests/test_step_plan.py).  No HIP here.
// (device_node.hip asks for a node step's plan ahead of its search through
// node_step_plan, device_ctx.hpp.)
#pragma once

#include <algorithm>
#include <cstdint>

#include "../../include/lincheck.h"

namespace lc {

struct StepIn {
    int64_t K = 0;             // keys of the batch
    uint64_t n_events = 0;     // (no rule reads it yet; the segments' length is sized from it at their launch)
    int cu_count = 256;
    // the batch (DevBatch)
    bool t0_only = false, table = false, taggable = false, seg_pays = false, validated = false, has_events16 = false;
    // the context's options (lc_opts)
    int32_t algorithm = LC_ALGO_LINEAR, flags = 0, path_flags = 0, spec_segs = 0;
    uint64_t max_configs = 1ull << 20;
    // result arrays the caller asked for
    bool want_peak = false, want_final = false, want_n_final = false;
    bool res_host = false;     // the results go to host memory
    bool allow_async = false;  // the caller accepts a step that is only enqueued
    int spec8_waves = 8;       // LC_SPEC8_WAVES (device_search.hpp)
    // the speculative segments' workspaces per key and segment, in words
    // (lcd::spec_ws_words(1, 1), lcd::spec_fin_words(1, 1)), and the most
    // device memory a batch's may take
    uint64_t ws_words = 0, fin_words = 0;
    uint64_t ws_max_bytes = 8ull << 30;
};

struct StepPlan {
    bool wgl_only = false;     // knossos.wgl's own search for every key: nothing below applies
    bool competition = false;  // then WGL for the keys :linear left at its budget
    bool t0_step = false;      // the step is the register tier alone
    bool async = false;        // ... and only enqueued
    bool split = false;        // quiescent-point key segments (k_search_segments)
    bool spec = false;         // speculative key segments (k_spec)
    int segs = 0;              // ... per key
    bool exact = false;        // ... with exact sets (final configs wanted, no peaks)
    bool ev16 = false;         // the register tier reads the 16-bit event words in place
    bool t0_wide = false;      // k_search_lattice's 16-register build
    int g0 = 1;                // its grid
    bool strict = false;       // T0_STRICT: the register tier refuses a key that does not fit
    bool gen_validate = false;   // the general validation kernel (every width)
    bool side_validate = false;  // a validation kernel on the second stream, beside the register tier
    int spec_vblocks = 0;      // k_spec: validation blocks in its own launch
    bool spec_vfirst = false;  // ... ahead of the keys' blocks
    int rerun_grid = 1;        // k_spec_rerun: its one-wave workgroups
    uint32_t t0_path = LC_T0_PATH_NONE;  // lc_stats.t0_path
    uint32_t ev_word_bytes = 0;          // lc_stats.ev_word_bytes
};

// One-wave workgroups of the rerun launch at most: the smallest of 8, 32 and
// 128 at which the launch, beside the other lane's k_spec, takes what it takes
// alone (all three did: 0.0044, 0.0047, 0.0050 ms against 0.0042; C2 the
// same with each; profiles/rerun_thin.json).  A/B: make variant
// VFLAGS=-DLC_SPEC_RERUN_GRID=n.
#ifndef LC_SPEC_RERUN_GRID
#define LC_SPEC_RERUN_GRID 8
#endif
constexpr int SPEC_RERUN_GRID = LC_SPEC_RERUN_GRID;

inline StepPlan plan_step(const StepIn &in) {
    StepPlan p;
    const int64_t K = in.K;
    // T0_STRICT: a register-tier batch the host did not walk (T0 refuses a key
    // that does not fit instead of spilling it); other unwalked batches get
    // the general validation kernel ahead of the set tiers
    p.strict = !in.validated && in.t0_only;
    p.gen_validate = !in.validated && !in.t0_only;
    if (in.algorithm == LC_ALGO_WGL) {
        p.wgl_only = true;
        return p;
    }
    p.competition = in.algorithm == LC_ALGO_COMPETITION;
    // Nothing counted and no key can leave T0: no T1/T2 launches, no counter
    // readback and no control-block memset -- the step is T0 alone (plus the
    // result download when the results go to host memory).
    p.t0_step = K > 0 && in.t0_only && !(in.flags & LC_OPT_COUNT_PROBES);
    // (competition: the WGL step needs the :linear step's causes)
    p.async = p.t0_step && in.allow_async && !p.competition && !in.res_host;
    // Key segments (device_segments.hip): verdicts only, a batch of about one
    // key per SIMD or fewer (where each key's serial chain is exposed), and
    // quiescent points close enough for the cuts to pay (segments_pay: on
    // C2, whose clients think about as long as an op takes, the longest
    // stretch without one is most of a key, so its keys stay whole).
    // lc_opts.path_flags LC_PATH_SPLIT_ON / _OFF pin the choice (A/B and tests).
    const bool fast = !in.want_peak && !in.want_final && in.max_configs >= 16ull * 64 * 32;
    const bool want = (in.path_flags & LC_PATH_SPLIT_ON) ? true : (in.path_flags & LC_PATH_SPLIT_OFF) ? false : in.seg_pays;
    p.split = p.t0_step && fast && in.taggable && want && K <= (int64_t)in.cu_count * 8;
    // Speculative segments (device_spec.hip): the same regime without
    // quiescent points -- every key a workgroup of `segs` waves, about four
    // segment waves per SIMD in all (C2: 1,000 keys x 4).  The kernel's 80
    // VGPRs would allow six, but 6-wave workgroups land unevenly on a CU's
    // four SIMDs (5-7 waves each): C2 0.357 ms at 4 segments per key, 0.406
    // at 6, 0.386 at 8.  lc_opts: LC_PATH_SPEC_OFF turns them off, spec_segs
    // pins the segments per key.
    //
    // Large batches too (C3 shards: 2 segments per key; 12,500 x 2,000 4.44
    // ms against 5.51 unsegmented, the whole C3 key space 33.2 against 38.0).
    // More segments than waves (a key's waves taking its segments from a
    // block-local queue) measured slower: C2 8 segments on 4 waves
    // 0.302 ms, 12 on 4 0.332, against 0.273 for 4 on 4; a C3 shard 4 on 2
    // 4.75 ms, 8 on 2 5.30, against 4.40 for 2 on 2.
    int segs = K > 0 ? (int)std::min<int64_t>(8, (int64_t)in.cu_count * 4 * 4 / std::max<int64_t>(K, 1)) : 0;
    segs = segs >= 8 ? 8 : segs >= 4 ? 4 : K > 0 ? 2 : 0;
    // Final configs wanted and no set sizes (the Jepsen-shaped checkers):
    // the segments with exact sets (Knossos's S, not its closure), each run
    // saving its set at its end or death, the true run's written as the
    // key's final configs (k_spec<.., EX>).
    const bool exact_spec = !in.want_peak && in.want_final && in.want_n_final && in.max_configs >= 16ull * 64 * 32;
    // 8 per key while 8 x keys waves are resident at the 8-wave build's 8
    // per SIMD (device_search.hpp LC_SPEC8_WAVES).  The exact segments too
    // since round 6 (spill-free builds, overlapped verifying runs;
    // tools/ex_segs_ab.py, records equal): C2 0.2843 -> 0.2530 ms, a C5-shaped
    // batch of another seed 0.2822 -> 0.2627, BASELINE's C5 0.2717 -> 0.2755.
    // (Round 5, before both: C5 0.289 -> 0.352 ms with 8.)
    if (in.spec8_waves >= 8 && (fast || exact_spec) && K > 0 && K * 8 <= (int64_t)in.cu_count * 4 * 8) segs = 8;
    if (in.spec_segs) segs = in.spec_segs;
    p.exact = exact_spec && !fast;
    if (p.exact) segs = segs >= 8 ? 8 : segs >= 4 ? 4 : 2;  // the exact builds
    p.segs = segs;
    p.spec = !p.split && p.t0_step && (fast || exact_spec) && segs >= 2 && !(in.path_flags & LC_PATH_SPEC_OFF);
    // The segments' workspaces are per key: a batch whose keys
    // would need more than ws_max_bytes of them takes the unsegmented
    // register tier, whose workspace is per resident wave.
    if (p.spec && (uint64_t)K * (uint64_t)segs * (in.ws_words + (p.exact ? in.fin_words : 0)) * 4 > in.ws_max_bytes)
        p.spec = false;
    // The speculative segments read 16-bit event words in place; every other
    // kernel reads the 32-bit form, widened once per upload.
    p.ev16 = p.spec && in.has_events16;
    p.t0_path = K == 0 || in.table ? LC_T0_PATH_NONE
                : p.split          ? LC_T0_PATH_SEGMENTS
                : p.spec           ? LC_T0_PATH_SPEC
                                   : LC_T0_PATH_LATTICE;
    p.ev_word_bytes = p.t0_path ? (p.ev16 ? 2u : 4u) : 0u;
    // T0 has two builds: 16 lattice registers (n <= 10 pending in VGPRs, 2
    // waves per SIMD) when every key can be resident at once -- each key's
    // events are serial, so there per-key latency is the whole story -- and
    // 4 registers (9-10 pending in LDS, 4 waves per SIMD) for larger batches,
    // where occupancy hides latency across keys.
    p.t0_wide = K <= (int64_t)in.cu_count * 8;
    p.g0 = (int)std::max<int64_t>(1, std::min<int64_t>(K, (int64_t)in.cu_count * (p.t0_wide ? 8 : 16)));
    // the event-by-event validation the host skipped: on the second stream,
    // beside T0 -- but k_spec runs that of a register-tier batch in extra
    // blocks of its own launch (a second stream cost ~40 us of cross-stream
    // waits), first in the grid when the keys take more than one resident round
    p.side_validate = K > 0 && ((p.strict && !p.spec) || p.gen_validate);
    p.spec_vblocks = p.spec && p.strict ? (int)std::min<int64_t>(K, in.cu_count) : 0;
    p.spec_vfirst = p.spec && K * segs > (int64_t)in.cu_count * 16;
    // The rerun launch (k_spec_rerun) is in every step and usually finds no
    // key, so its dispatch is what it costs: a fixed number of one-wave
    // workgroups, whatever the chip's size, that fit beside the other
    // lane's k_spec blocks.  Wave b works in slot b of the step's K * segs
    // k_spec workspaces, and more waves than keys would find nothing to do.
    p.rerun_grid = (int)std::max<int64_t>(1, std::min<int64_t>(SPEC_RERUN_GRID, p.spec ? K : 1));
    return p;
}

}  // namespace lc
