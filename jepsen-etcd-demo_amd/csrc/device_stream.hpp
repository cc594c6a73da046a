// device_stream.hpp -- the device half of a stream (lc_stream_*): what
// host_stream.cpp needs from device_stream.hip to keep per-key search records
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
    uint32_t key, status, fail_event, why;  // STREAM_INVALID / STREAM_ERROR / STREAM_BUDGET; LC_BATCH_E_* bits
};
// Exact mode (LC_STREAM_EXACT): what a key that is invalid or at the budget
// leaves beside its verdict, the words lc_check_batch writes for it.
struct Final {
    uint32_t peak = 1, n_final = 0;
    uint64_t cfg[32] = {};  // n_final configs of two words (max_final <= 16)
};

// The resident set tier's work of a call (LC_STREAM_SET_TIER): keys that
// migrate from their register record into pool slot `slot`, with their pending
// ops' descriptors by window slot, and keys searched from their set record.
struct SetMig {
    int32_t key, slot;
    uint32_t descs[64];
};
struct SetItem {
    int32_t key, slot;
    uint32_t ev_b, ev_e;  // its new 32-bit words
    uint32_t tr_b, ntr;   // its transitions
};
struct SetWork {
    const SetMig *mig;
    int64_t n_mig;
    const SetItem *items;
    int64_t n_items;
    const uint32_t *ev32;
    uint64_t n_ev32;
};

// Refuses (LC_E_UNSUPPORTED) a context with several devices or a
// communicator, or -- unless `exact` -- a budget below the FAST walk's exact
// range.  exact: the launches are k_stream_exact's, with the context's budget,
// and the stream owns final-config arrays beside its records.
int stream_dev_open(lc_ctx *c, bool exact, StreamDev **out);
// The context's lc_opts.max_final: configs per key in exact mode's arrays.
int stream_dev_max_final(const StreamDev *d);
void stream_dev_close(StreamDev *d);
// Search the items' words (one k_stream launch on the context's lane 0,
// joined behind lane 1) and return the keys that died, ascending by key.
// n_keys: the stream's keys so far (records are grown, zero-filled, to hold them).
// set (may be null): after k_stream, on the same lane, the migrations and then
// one k_stream_set launch (exact mode: k_stream_set_exact, whose keys may also
// die at the budget and leave their Final); keys that left the set tier are in
// `dead` too (status STREAM_SET_FALLBACK for those that fell back).
int stream_dev_push(StreamDev *d, int64_t n_keys, const Item *items, int64_t n_items, const uint16_t *ev16,
                    uint64_t n_ev, const uint32_t *trans, uint64_t n_trans, uint32_t init_state,
                    std::vector<Dead> *dead, const SetWork *set = nullptr, std::vector<Final> *fin = nullptr);
// Exact mode.  fin (may be null: a stream without the flag leaves it empty)
// gets one entry per entry of `dead`, filled for STREAM_INVALID / STREAM_BUDGET.
// stream_dev_peaks: every key's running peak from its record's header
// (out[n_keys]; a fresh record counts 1).  stream_dev_finals: one
// k_stream_final launch over the live keys `keys` (their end sets' configs
// into the stream's arrays), then every key's configs and count back:
// cfg[n_keys * max_final * 2], n_final[n_keys].
int stream_dev_peaks(StreamDev *d, int64_t n_keys, uint32_t *out);
// set_live (exact mode with the set tier): the set-tier keys still live, whose
// end sets one k_stream_set_final launch writes before the copies back.
struct SetLive {
    int32_t key, slot;
};
int stream_dev_finals(StreamDev *d, int64_t n_keys, const int32_t *keys, int64_t n_live, uint32_t init_state,
                      uint64_t *cfg, uint32_t *n_final, const SetLive *set_live = nullptr, int64_t n_set_live = 0);
// Device time of the last stream_dev_finals launch, ms.
double stream_dev_final_ms(const StreamDev *d);
// The set-record pool: a slot for a migrating key (the pool is allocated on
// first use and grows geometrically, in chunks that never move), and its return.
int stream_dev_set_alloc(StreamDev *d, int32_t *slot);
void stream_dev_set_free(StreamDev *d, int32_t slot);
// Words off .. off + words of pool slot `slot` as they are in device memory.
int stream_dev_set_record(StreamDev *d, int32_t slot, int64_t off, uint32_t *out, int64_t words);
// [0] migration, [1] k_stream_set device time of the last push, ms; the pool's
// [2] slots allocated, [3] in use, [4] most in use at once, [5] bytes per slot.
void stream_dev_set_stats(const StreamDev *d, double *out6);
// Key's record as it is in device memory (STREAM_REC_WORDS words).
int stream_dev_record(StreamDev *d, int64_t key, uint32_t *out);
// Device-event times of the last push, ms: upload, k_stream, readback.
void stream_dev_timing(const StreamDev *d, double *out3);

}  // namespace lcst
