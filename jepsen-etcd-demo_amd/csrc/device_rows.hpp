// device_rows.hpp -- the model-independent front end of a device pack
// (device_rows.hip, in lincheck/libcounter_pack_kernels.so): raw history rows
// are grouped by independent key and paired by (key, process) on the device.
// rows_plan.hpp has the sizes.  A checker's own half (device_counter_pack.hip is
// the first) says which rows take part and reads what comes out:
//
//   rows_group   a hash table of the keys and one of the processes, each slot
//                holding the lowest row that names it; a row that is its key's
//                first row numbers the key, by a scan, in order of first
//                appearance.  One stream synchronisation: the number of
//                distinct keys and processes comes back.
//   rows_pair    rows sorted (stable) by key index, which is history order
//                within every key: a row's place there is its POSITION.  A
//                second stable sort, by process index, of the positions puts
//                every (key, process) group side by side in history order, and
//                a position's left and right neighbour there, when of its
//                group, are its predecessor and successor.
//   rows_scan2   an in-place exclusive scan of pairs of 64-bit sums, the
//                grand totals behind the last item.
//
// A batch is KEYED when some row has a key; otherwise it has the one key
// LC_NO_KEY, and every row that takes part is that key's.  Rows that take no
// part, have no process, or in a keyed batch no key, get the key index n_keys
// and sort behind every key.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace lcr {

struct RowsIn {
    uint32_t n;              // 1 .. RP_MAX_ROWS
    const uint8_t *takes;    // [n] 1: the row takes part (device)
    const int64_t *process;  // [n] device, or null: every row is process 0
    const int64_t *key;      // [n] device, or null: no row has a key
};

// Everything below is device memory, owned by the Rows object and valid until its next rows_group.
struct RowsView {
    uint32_t n = 0;
    uint32_t n_keys = 0;      // at least 1
    bool keyed = false;
    const int64_t *keys = nullptr;        // [n_keys] in order of first appearance
    const uint32_t *first_row = nullptr;  // [n_keys]
    const uint32_t *pos_key = nullptr;    // [n] key index of each position, ascending; n_keys: takes no part
    const uint32_t *pos_row = nullptr;    // [n] its history row
    const uint32_t *prev = nullptr;       // [n] position of its predecessor in its (key, process) group, or RP_NONE
    const uint32_t *next = nullptr;       // [n] of its successor, or RP_NONE
    uint32_t *err = nullptr;              // a probe that overran its table sets bit 0
};

struct Rows;

int rows_open(Rows **out);
void rows_close(Rows *r);
int rows_group(Rows *r, hipStream_t stream, const RowsIn &in, uint64_t *n_keys, uint64_t *n_procs);
int rows_pair(Rows *r, hipStream_t stream, RowsView *out);
// a: [n + 1] device; a[n] receives the totals.
int rows_scan2(Rows *r, hipStream_t stream, ulonglong2 *a, uint64_t n);

}  // namespace lcr
