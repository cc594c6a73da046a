// device_queue.hpp -- checker/total-queue's and checker/unique-ids' kernels
// (device_queue.hip, built as libqueue_kernels.so): what device_api.hip needs
// to launch them on a context's stream.  The step that runs them,
// lc_queue_check, and its cached device arrays (QueueDev, device_ctx.hpp) are
// device_api.hip's.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/lincheck_queue.h"

namespace lcq {

// lc_queue_check's out words on the device.
enum { QO_N_ENT = 0, QO_ERR = 1, QO_WORDS = 2 };
// QO_ERR
constexpr unsigned long long QE_BAD_ROW = 1;  // row_key >= n_keys, or a row_kind the mode has not
constexpr unsigned long long QE_FULL = 2;     // a lane visited every slot and found no place

struct QueueArgs {
    // the batch on the device; no kernel writes these
    const uint32_t *row_key;
    const uint8_t *row_kind;
    const int64_t *row_val;
    const uint8_t *status;  // [K]
    uint64_t n_rows;
    uint32_t K, mode;
    // the table: slots x {rep, tally[3]}
    uint4 *table;
    uint32_t slots;  // a power of two >= n_rows
    // per key
    unsigned long long *counts;  // [K][LC_QN_COUNTS]
    long long *lo, *hi;          // [K]
    // the entries, in no order
    uint32_t *ent_key;
    uint8_t *ent_class;
    int64_t *ent_val;
    unsigned long long *ent_mult;
    uint64_t ent_cap;
    unsigned long long *out;  // [QO_WORDS]
};

// k_queue_reset, k_queue_tally, k_queue_classify, in stream order.
hipError_t queue_launch(hipStream_t stream, const QueueArgs &a);

// host_queue.cpp: a batch's shape and a result's arrays.
int queue_validate(const lc_queue_batch *b, const lc_queue_result *r, const char *who);
// host_queue.cpp: valid and has_range from the counts, and the entries sorted
// by (key, class, value) into r (n of them, n <= r->ent_cap).
void queue_finish(const lc_queue_batch *b, lc_queue_result *r);
void queue_sort_entries(lc_queue_result *r, uint64_t n, const uint32_t *key, const uint8_t *cls, const int64_t *val,
                        const unsigned long long *mult);

}  // namespace lcq
