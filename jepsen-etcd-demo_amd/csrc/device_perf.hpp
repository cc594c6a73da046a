// device_perf.hpp -- checker/perf's analysis on the device (device_perf.hip):
// what device_api.hip needs to run lc_perf_check on a context's stream (the
// context keeps a PerfDev per device: device_ctx.hpp).
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/lincheck.h"

namespace lcp {

// A device's perf state: cached device arrays and pinned staging, grown on
// demand and kept from one call to the next.  Owned by the context's Dev.
struct PerfDev;
void perf_dev_free(PerfDev *d);

// lc_perf_check on `stream` of the current device (the caller holds the
// context's lock).  *dev is created on first use.
int perf_check(PerfDev **dev, hipStream_t stream, const lc_perf_batch *b, const lc_perf_opts *o, lc_perf_result *r);
// lc_perf_last_timing.
int perf_last_timing(const PerfDev *d, double *out_ms);

// The same step on a batch that lies in the device's own record columns
// (lc_perf_check_history builds it there: device_perf_pack.hip).
// perf_records_device grows the three columns to n records and hands them out
// to be written on `stream`; perf_check_device then runs perf_check's launches
// on them: sizes carries the counts and bounds, its column pointers are not
// read, nothing is uploaded.  Checks, results and timing slots are perf_check's.
int perf_records_device(PerfDev **dev, uint64_t n, int64_t **t_comp, int64_t **t_inv, uint32_t **meta);
int perf_check_device(PerfDev **dev, hipStream_t stream, const lc_perf_batch *sizes, const lc_perf_opts *o, lc_perf_result *r);
// The columns' generation: it changes whenever a call is about to rewrite them.
uint64_t perf_generation(const PerfDev *d);
// The first n records of the columns to host arrays (synchronises the stream).
int perf_records_download(PerfDev *d, hipStream_t stream, uint64_t n, int64_t *t_comp, int64_t *t_inv, uint32_t *meta);

}  // namespace lcp
