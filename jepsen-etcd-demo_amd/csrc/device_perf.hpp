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

}  // namespace lcp
