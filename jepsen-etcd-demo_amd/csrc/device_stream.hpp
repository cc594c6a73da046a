// device_stream.hpp -- the device half of a stream (lc_stream_*): what
// host_stream.cpp needs from device_api.hip to keep per-key search records
// resident and to advance them.  No HIP types here.
#pragma once

#include <cstdint>
#include <vector>

#include "../../include/lincheck.h"

namespace lcst {

// A stream's device state: the records, staging and result buffers.
struct StreamDev;

// One key's new work in a launch (lcd::StreamItem's layout).
struct Item {
    int32_t key;
    uint32_t ev_b, ev_e;  // its new 16-bit words
    uint32_t tr_b, ntr;   // its transitions
    uint32_t ns;          // state ids it uses
};
// A key that died in a launch.
struct Dead {
    uint32_t key, status, fail_event, why;  // STREAM_INVALID / STREAM_ERROR; LC_BATCH_E_* bits
};

// Refuses (LC_E_UNSUPPORTED) a context with several devices or a
// communicator, or a budget below the FAST walk's exact range.
int stream_dev_open(lc_ctx *c, StreamDev **out);
void stream_dev_close(StreamDev *d);
// Search the items' words (one k_stream launch on the context's lane 0,
// joined behind lane 1) and return the keys that died, ascending by key.
// n_keys: the stream's keys so far (records are grown, zero-filled, to hold them).
int stream_dev_push(StreamDev *d, int64_t n_keys, const Item *items, int64_t n_items, const uint16_t *ev16,
                    uint64_t n_ev, const uint32_t *trans, uint64_t n_trans, uint32_t init_state,
                    std::vector<Dead> *dead);
// Key's record as it is in device memory (STREAM_REC_WORDS words).
int stream_dev_record(StreamDev *d, int64_t key, uint32_t *out);
// Device-event times of the last push, ms: upload, k_stream, readback.
void stream_dev_timing(const StreamDev *d, double *out3);

}  // namespace lcst
