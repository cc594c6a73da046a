// device_counter_stream.hpp -- the device half of a streaming checker/counter
// (device_counter_stream.hip, in lincheck/libcounter_stream_kernels.so) as
// host_counter_stream.cpp calls it, and the CHUNK the packer makes of one
// append, which the host stream's fold reads too.  No HIP in this header: the
// packer and the host fold are host C++ and are also built stand-alone (tests),
// where these functions are absent -- they are weak, and a host stream never
// calls them.
//
// THE CHUNK.  Three things, all in the packer's own ids:
//   events   grouped by touched key (a SEGMENT per key, in order of first
//            touch), in history order within the key.  ev_seg names the
//            segment, seg_key[segment] the key.
//              LC_CE_UP   ev_val: the add's value as it is counted
//              LC_CE_LOW  ev_val: the :ok :add's value
//              LC_CE_RINV ev_aux: the slot that takes `lower`
//              LC_CE_ROK  ev_aux: that slot; ev_val: the read, as an index
//                         into this chunk's reads
//   reads    this append's :ok :read rows in arrival order: key, rank within
//            the key, slot, value.  Read i becomes resident read
//            reads_before + i.  A slot is not handed out twice in one append.
//   patches  invocations of earlier appends revised by this one, sorted by
//            (key, r0): r0 the resident reads when the add was invoked, acc
//            what the revisions of this key up to and including this entry add
//            to `upper`.  Read r of the key takes the acc of the last entry
//            with r0 <= r; the key's sum takes the acc of its last entry.
// look names the keys whose n_errors may have changed (those with patches or
// reads); their counts come back in that order.
#pragma once

#include "../../include/lincheck_counter_stream.h"

namespace lccs {

constexpr uint64_t CS_NO_READS = ~0ull;  // read_off of a key that has no reads in results()

struct CsChunk {
    uint64_t n_events = 0;
    const uint8_t *ev_kind = nullptr;
    const uint32_t *ev_seg = nullptr, *ev_aux = nullptr;
    const int64_t *ev_val = nullptr;
    uint64_t n_seg = 0;
    const uint32_t *seg_key = nullptr;
    uint64_t n_reads = 0;
    const uint32_t *rd_key = nullptr, *rd_rank = nullptr, *rd_slot = nullptr;
    const int64_t *rd_val = nullptr;
    uint64_t n_patch = 0, min_r0 = 0;
    const uint32_t *p_key = nullptr, *p_r0 = nullptr;
    const int64_t *p_acc = nullptr;
    uint64_t n_look = 0;
    const uint32_t *look = nullptr;
    uint64_t n_keys = 0, n_slots = 0, reads_before = 0;
};

struct CsDev;  // the resident arrays, a stream's staging, timing events

#define LC_CS_WEAK __attribute__((weak))

// Refuses a context of several devices or with a communicator.
LC_CS_WEAK int cs_dev_open(lc_ctx *ctx, uint32_t tile, uint64_t launch_events, CsDev **out);
LC_CS_WEAK void cs_dev_close(CsDev *d);
// The reads arrays hold `cap` reads (at least the current capacity), the
// `reads` resident ones copied.  A failed allocation is LC_E_NOMEM and leaves
// them as they were.  *ms: the step's device time.
LC_CS_WEAK int cs_dev_reserve(CsDev *d, uint64_t cap, uint64_t reads, double *ms);
// One append's chunk: patch, scan (in pieces), judge, gather.  n_errors
// [n_look] comes back; ms3: upload, kernels, readback.
LC_CS_WEAK int cs_dev_append(CsDev *d, const CsChunk *c, uint64_t *n_errors, double *ms3);
// Every resident read of a key with read_off != CS_NO_READS at read_off[key] +
// rank: lower, upper, value (may be NULL), flag; [total] each.
LC_CS_WEAK int cs_dev_results(CsDev *d, const uint64_t *read_off, uint64_t n_keys, uint64_t reads, uint64_t total, int64_t *lower,
                              int64_t *upper, int64_t *value, uint8_t *flag);

}  // namespace lccs
