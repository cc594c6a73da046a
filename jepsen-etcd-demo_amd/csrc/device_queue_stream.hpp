// device_queue_stream.hpp -- the device half of a streaming total-queue /
// unique-ids (device_queue_stream.hip, in lincheck/libqueue_stream_kernels.so)
// as host_queue_stream.cpp calls it.  No HIP in this header: the packer and the
// host fold are host C++ and are also built stand-alone (tests), where these
// functions are absent -- they are weak, and a host stream never calls them.
//
// THE SLOT, 48 bytes, three 16-byte words:
//   {state, key, value (int64)} {tally[3], dirty} {applied[3], -}
// state is QS_EMPTY, QS_SETTLED (key and value are the slot's own), or
// QS_ROW0 + r: the slot was claimed by row r of the piece being tallied, whose
// row_key[r] / row_val[r] are its identity until k_qs_settle copies them in.
// A slot's home is slot_hash(key, value) & (slots - 1) (device_queue.hip's
// mixer: x = value ^ key * 0x9E3779B97F4A7C15, two multiply-xorshift rounds by
// 0xBF58476D1CE4E5B9 and 0x94D049BB133111EB with shifts 30, 27, 31, the two
// halves folded by xor); probing is linear.
#pragma once

#include "../../include/lincheck_queue_stream.h"

namespace lcqs {

constexpr uint32_t QS_EMPTY = 0;    // (a table is born by a memset to 0)
constexpr uint32_t QS_SETTLED = 1;
constexpr uint32_t QS_ROW0 = 2;

// A touched key's words in the readback: the seven counts, then the range as
// two maxima of order-preserving unsigned images, so that every word starts
// at 0: QS_LO holds max(~u), QS_HI max(u), u = value ^ 2^63.
enum { QS_LO = LC_QN_COUNTS, QS_HI = LC_QN_COUNTS + 1, QS_KEY_WORDS = LC_QN_COUNTS + 2 };

struct QsDev;  // the resident table and per-key words, a stream's staging, timing events

// One append's packed rows and the keys they touch.
struct QsChunk {
    uint64_t n_rows = 0;
    const uint32_t *row_key = nullptr;
    const uint8_t *row_kind = nullptr;
    const int64_t *row_val = nullptr;
    uint64_t n_touched = 0;
    const uint32_t *touched = nullptr;  // key ids, in order of first touch
    uint64_t n_keys = 0;                // keys so far, this append's included
};

#define LC_QS_WEAK __attribute__((weak))

// Refuses a context of several devices or with a communicator.  The table
// itself is made by the first qs_dev_grow.
LC_QS_WEAK int qs_dev_open(lc_ctx *ctx, uint32_t mode, QsDev **out);
LC_QS_WEAK void qs_dev_close(QsDev *d);
// A table of `slots` (a power of two above the current one's) with every
// settled slot of the current one rehashed into it (k_qs_rehash); the old one
// is freed behind the kernel.  A failed allocation is LC_E_NOMEM and leaves
// the table as it was.  *ms: the step's device time.
LC_QS_WEAK int qs_dev_grow(QsDev *d, uint64_t slots, double *ms);
// Tally and settle one append's rows (in pieces of QSP_LAUNCH_ROWS), which the
// caller has made room for.  words [n_touched][QS_KEY_WORDS] and *distinct come
// back; ms3: upload, kernels, readback.
LC_QS_WEAK int qs_dev_append(QsDev *d, const QsChunk *c, uint64_t *words, uint64_t *distinct, double *ms3);
// The entries of every settled slot whose key's status is LC_QUEUE_KEY_OK, in
// no order: at most cap of them written, *n_ent all of them counted.
LC_QS_WEAK int qs_dev_entries(QsDev *d, const uint8_t *status, uint64_t n_keys, uint64_t cap, uint32_t *ent_key, uint8_t *ent_class,
                              int64_t *ent_val, uint64_t *ent_mult, uint64_t *n_ent);

}  // namespace lcqs
