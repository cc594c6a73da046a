// device_setfull_stream.hpp -- the device half of a streaming set-full
// (device_setfull_stream.hip, in lincheck/libsetfull_stream_kernels.so) as
// host_setfull_stream.cpp calls it.  No HIP in this header: the packer is
// host C++ and is also built stand-alone (tests), where these functions are
// absent -- they are weak, and a packer-only stream never calls them.
#pragma once

#include "../../include/lincheck_setfull_stream.h"

namespace lcfs {

struct SfsDev;  // the resident records and a stream's staging, timing events

#define LC_SFS_WEAK __attribute__((weak))

// Refuses a context of several devices or with a communicator.
LC_SFS_WEAK int sfs_dev_open(lc_ctx *ctx, SfsDev **out);
LC_SFS_WEAK void sfs_dev_close(SfsDev *d);
// Fold one chunk: n_blocks = blocks in use after it.  valid [n_touched] and
// counts [6 * n_touched] come back per touched key.  ms: upload, mark,
// fold + finish, readback, passes.
LC_SFS_WEAK int sfs_dev_append(SfsDev *d, const lc_setfull_stream_chunk *c, uint64_t n_blocks, int linearizable,
                               uint64_t cap_bytes, int8_t *valid, uint64_t *counts, double *ms5);
// The per-slot result arrays of blocks [0, n_blocks): each [256 * n_blocks].
LC_SFS_WEAK int sfs_dev_results(SfsDev *d, uint64_t n_blocks, uint8_t *outcome, int64_t *latency, int64_t *known,
                                int64_t *last_absent, uint8_t *dup);

}  // namespace lcfs
