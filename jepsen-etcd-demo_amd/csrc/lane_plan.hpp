// Where an enqueued node step (lc_check_node_async, device_node.hip) runs: its
// search lane, whether it may overlap the step before it, how its records
// reach the caller's buffer, and its staging slot -- as a pure function of
// plain values, tested without a GPU (tests/test_lane_plan.py).  No HIP here.
//
// Consecutive register-tier steps search on two streams in turn, so a step's
// workgroups take the slots the previous step's finished blocks free (its
// slowest block sets a launch's length: DESIGN.md "Two search lanes").
#pragma once

#include <cstdint>

#include "../../include/lincheck.h"

namespace lc {

constexpr int LANES = 2;       // search streams
constexpr int LANE_SLOTS = 3;  // staging batches: two searches and one upload in flight
constexpr int LANE_FLIGHT = LANE_SLOTS - 1;  // steps that may still run when one is enqueued

struct LaneIn {
    uint64_t seq = 0;    // pipelined steps enqueued before this one (the slots' turn)
    uint64_t run_n = 0;  // ... of them, since the lanes were last joined (the lanes' turn)
    // the step's plan (step_plan.hpp)
    bool async = false, spec = false, split = false;
    // its search launch in waves (keys x segments), and the waves the device
    // holds at once (8 per SIMD, the 8-wave k_spec build's)
    int64_t waves = 0, resident_waves = 0;
    bool comm = false;   // the context has a communicator
    int32_t path_flags = 0;
    bool mapped = false;  // the caller's buffer can be written by the device in place
    // the caller's buffer, [lo, hi) in bytes, and those of the steps still in flight
    uint64_t lo = 0, hi = 0;
    int n_flight = 0;
    struct Flight {
        uint64_t seq = 0, lo = 0, hi = 0;
    } flight[LANE_FLIGHT];
};

struct LanePlan {
    int lane = 0;
    bool overlap = false;  // the search does not wait for the steps before it
    // records: written in place by the search (direct), or into the lane's
    // own block and copied out behind the search -- when `after` >= 0, only
    // once step `after` has ended, so a buffer given to several steps ends up
    // holding the latest one's records
    bool direct = false;
    int64_t after = -1;
    int slot = 0;             // staging batch
    int64_t slot_waits = -1;  // the step that used it last (its end is waited for), or none
};

inline LanePlan plan_lane(const LaneIn &in) {
    LanePlan p;
    p.slot = (int)(in.seq % LANE_SLOTS);
    p.slot_waits = in.seq >= (uint64_t)LANE_SLOTS ? (int64_t)(in.seq - LANE_SLOTS) : -1;
    // Two lanes for the speculative segments only: the lattice's ticket
    // continues from step to step, key segments share their work lists, and
    // a communicator's collectives stay on one stream, in one order.  And
    // only for a launch that is resident at once: there the slots its
    // finished blocks free stay empty until its slowest block ends, which is
    // what the next step's blocks fill.  A launch of several rounds refills
    // them itself, and two of those side by side only share the device
    // (measured: BASELINE C3's 100,000 keys 25.7 -> 34.2 ms per step).
    p.overlap = in.async && in.spec && !in.split && !in.comm && !(in.path_flags & LC_PATH_NODE_SERIAL) &&
                in.waves <= in.resident_waves;
    p.lane = p.overlap ? (int)(in.run_n % LANES) : 0;
    const bool may_map = in.mapped && !in.comm && !(in.path_flags & LC_PATH_NODE_STAGED);
    if (!p.overlap) {  // one stream: its order is the records' order
        p.direct = may_map;
        return p;
    }
    for (int i = 0; i < in.n_flight && i < LANE_FLIGHT; ++i) {
        const LaneIn::Flight &f = in.flight[i];
        if (f.lo < in.hi && in.lo < f.hi) p.after = p.after < (int64_t)f.seq ? (int64_t)f.seq : p.after;
    }
    p.direct = may_map && p.after < 0;
    return p;
}

}  // namespace lc
