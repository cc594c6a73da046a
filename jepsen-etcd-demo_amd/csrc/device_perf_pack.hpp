// device_perf_pack.hpp -- the device half of lc_perf_check_history
// (device_perf_pack.hip, in lincheck/libperf_pack_kernels.so) as
// host_perf_pack.cpp calls it, and what it fills.  No HIP in this header:
// host_perf_pack.cpp is host C++ and is also built stand-alone (tests), where
// these functions are absent -- they are weak, and the entry points say
// LC_E_DEVICE without them.
#pragma once

#include <cstdint>
#include <vector>

#include "common.hpp"
#include "../../include/lincheck_perf_pack.h"

namespace lcpp {

// What comes back from the device.
struct PpOut {
    // lc_perf_packed_view's counts and bounds
    int64_t n_rec = 0, matched = 0, unmatched = 0, orphans = 0;
    int64_t t_min = 0, t_max = 0, x_min = 0, x_max = 0;
    int32_t n_f = 0;
    int64_t hist_max = 0;      // the largest :time of all rows
    std::vector<int64_t> nem;  // (f, time) of the rows without a process whose f is f_start or f_stop, in history order
    // lc_perf_check's result
    int64_t shape[4] = {0, 0, 0, 0};  // rate_first, rate_n, q_first, q_n
    std::vector<uint64_t> rate, group;
    std::vector<int64_t> quant;
    uint64_t generation = 0;  // of the device's record columns this was computed from
    // lc_perf_checked_records'
    lc::pinned_vector<int64_t> t_comp, t_inv;
    lc::pinned_vector<uint32_t> meta;
};

// host_perf.cpp's interval rule over the compacted nemesis rows: :start opens
// if none is open, the next :stop closes it, one left open ends at hist_max.
void pp_fold_intervals(const std::vector<int64_t> &nem, int32_t f_start, int32_t f_stop, int64_t hist_max, std::vector<int64_t> &out);

#define LC_PP_WEAK __attribute__((weak))

// Refuses a context of several devices or with a communicator.  h->n >= 1 and h->n_f is in range.
LC_PP_WEAK int pp_dev_check(lc_ctx *ctx, const lc_perf_history *h, const lc_perf_opts *o, PpOut *out);
// t_comp, t_inv and meta of the batch out->generation names.
LC_PP_WEAK int pp_dev_records(lc_ctx *ctx, PpOut *out);
LC_PP_WEAK int pp_dev_timing(lc_ctx *ctx, double *out6);

}  // namespace lcpp
