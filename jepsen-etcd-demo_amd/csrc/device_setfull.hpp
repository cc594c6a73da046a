// device_setfull.hpp -- checker/set-full on the device (device_setfull.hip):
// what device_api.hip needs to run lc_setfull_check on a context's stream (the
// context keeps a SetFullDev per device: device_ctx.hpp).
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/lincheck.h"

namespace lcf {

// A device's set-full state: cached device arrays, pinned staging and timing
// events, grown on demand and kept from one call to the next.  Owned by the
// context's Dev.
struct SetFullDev;
void setfull_dev_free(SetFullDev *d);

// lc_setfull_check on `stream` of the current device (the caller holds the
// context's lock).  *dev is created on first use.
int setfull_check(SetFullDev **dev, hipStream_t stream, const lc_setfull_batch *b, const lc_setfull_opts *o,
                  lc_setfull_result *r);
// lc_setfull_last_timing.
int setfull_last_timing(const SetFullDev *d, double *out8);

}  // namespace lcf
