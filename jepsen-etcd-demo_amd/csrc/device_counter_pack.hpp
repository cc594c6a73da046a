// device_counter_pack.hpp -- the device half of lc_counter_check_history
// (device_counter_pack.hip, in lincheck/libcounter_pack_kernels.so) as
// host_counter_pack.cpp calls it, and the result arrays it fills.  No HIP in
// this header: host_counter_pack.cpp is host C++ and is also built stand-alone
// (tests), where these functions are absent -- they are weak, and the entry
// points say LC_E_DEVICE without them.
#pragma once

#include <cstdint>
#include <vector>

#include "common.hpp"
#include "../../include/lincheck_counter_pack.h"

namespace lccp {

// What comes back from the device: per key, per read, and the reads out of bounds.
struct CpOut {
    int64_t n_keys = 0;
    uint64_t E = 0, R = 0, n_err = 0;
    uint64_t generation = 0;  // of the context's device batch this was read from
    std::vector<int64_t> keys;
    std::vector<uint8_t> status;
    std::vector<uint64_t> error;  // [n_keys] cp_word of the key's error, or CP_NO_ERROR
    std::vector<uint64_t> ev_off, read_off, err_off;  // [n_keys + 1]
    lc::pinned_vector<int64_t> lower, upper, read_val;  // [R]
    lc::pinned_vector<uint64_t> err_idx;                // [n_err]
    // lc_counter_checked_batch's
    lc::pinned_vector<uint8_t> ev_kind;
    lc::pinned_vector<int64_t> ev_val;
};

#define LC_CP_WEAK __attribute__((weak))

// Refuses a context of several devices or with a communicator.  h->n >= 1.
LC_CP_WEAK int cp_dev_check(lc_ctx *ctx, const lc_counter_history *h, uint32_t tile, CpOut *out);
// ev_kind and ev_val of the batch out->generation names.
LC_CP_WEAK int cp_dev_batch(lc_ctx *ctx, CpOut *out);
LC_CP_WEAK int cp_dev_timing(lc_ctx *ctx, double *out6);

}  // namespace lccp
