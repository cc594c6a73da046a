// device_set.hpp -- the set-workload check on the device (device_set.hip):
// what device_api.hip needs to run lc_set_check on a context's stream (the
// context keeps a SetDev per device: device_ctx.hpp).
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/lincheck.h"

namespace lcs {

// A device's set-check state: cached device arrays and pinned staging, grown
// on demand and kept from one call to the next.  Owned by the context's Dev.
struct SetDev;
void set_dev_free(SetDev *d);

// lc_set_check on `stream` of the current device (the caller holds the
// context's lock).  *dev is created on first use.
int set_check(SetDev **dev, hipStream_t stream, int path_flags, const lc_set_batch *b, lc_set_result *r);
// lc_set_last_timing.
int set_last_timing(const SetDev *d, double *out_ms);

}  // namespace lcs
