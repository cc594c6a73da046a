// device_counter.hpp -- checker/counter's kernels (device_counter.hip, built as
// libcounter_kernels.so): what device_api.hip needs to launch them on a
// context's stream.  The step that runs them, lc_counter_check, and its cached
// device arrays (CounterDev, device_ctx.hpp) are device_api.hip's.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/lincheck_counter.h"

namespace lcc {

// One series of a batch on the device (counter_plan.hpp): n items, key k's at
// off[k] .. off[k + 1], tile t's offset entries first[t] .. first[t + 1].
struct CtSeries {
    const uint64_t *off;    // [K + 1]
    const uint32_t *first;  // [tiles + 1]
    int64_t K;
    uint64_t n, tiles;
};

// The tile records and carries of one scan: [tiles] each.
struct CtTiles {
    unsigned long long *sum_a, *sum_b;      // a tile's two sums since its last key head (or its start)
    unsigned long long *carry_a, *carry_b;  // what reaches the tile's first item from the tiles before it
    uint8_t *heads;                         // CT_HEAD_*
};

struct CtEvents {
    CtSeries s;
    CtTiles t;
    const uint8_t *kind;
    const int64_t *val;
    int64_t *lower, *upper;  // [R]
    uint64_t R;
    uint32_t *err;           // set to 1 by a bad kind or read index
};

struct CtJudge {
    CtSeries s;
    CtTiles t;
    const int64_t *val, *lower, *upper;  // [R]
    unsigned long long *err_off;         // [K + 1]
    unsigned long long *err_idx;         // [err_cap]
    uint64_t err_cap;
    unsigned long long *n_err;
};

// k_counter_tile, k_counter_carry, k_counter_apply over the events (s.n > 0);
// tile: 256 or 2,048.
hipError_t counter_launch_events(hipStream_t stream, uint32_t tile, const CtEvents &a);
// k_counter_judge_tile, k_counter_carry, k_counter_judge over the reads (s.n > 0).
hipError_t counter_launch_judge(hipStream_t stream, uint32_t tile, const CtJudge &a);

// host_counter.cpp: the offset arrays and status codes of a batch.
int counter_validate(const lc_counter_batch *b, const char *who);

}  // namespace lcc
