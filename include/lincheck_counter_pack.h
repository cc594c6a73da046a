/* lincheck_counter_pack.h -- checker/counter from raw rows: the history is
 * grouped by key, paired and packed on the device (DESIGN.md section 3.18;
 * ABI 13, additive).
 *
 * A section of include/lincheck_counter.h kept in a file of its own, as
 * lincheck_counter_stream.h is; everything here is exported by the same
 * liblincheck.so.  The rules are lincheck_counter.h's.
 *
 * lc_counter_check_history(h) equals lc_counter_pack(h) followed by
 * lc_counter_check_host, in every field: the keys and their order, status, an
 * error key's text, ev_off, read_off, ev_kind, ev_val, read_val, valid,
 * n_errors, lower, upper, err_off, err_idx.  A bad :type / :f code ends the
 * call with LC_E_INVALID, naming the lowest offending row.
 *
 * One call uploads type, f, process, key and value (index is not read; a NULL
 * process is process 0 everywhere, a NULL key means no row has one), through
 * pinned staging when the caller's arrays are not page-locked.  Everything
 * else runs on the context's first device and stream, and only results come
 * back: there is no host pass over the rows.  The context must have one device
 * and no communicator, and n at most 2^31 - 16: else LC_E_UNSUPPORTED.
 */
#ifndef LINCHECK_COUNTER_PACK_H
#define LINCHECK_COUNTER_PACK_H

#include "lincheck_counter.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lc_counter_checked lc_counter_checked;  /* library-owned: R and the number of errors are not known up front */

int  lc_counter_check_history(lc_ctx *ctx, const lc_counter_history *h, const lc_counter_opts *o, lc_counter_checked **out);
void lc_counter_checked_free(lc_counter_checked *c);
/* Borrowed host arrays, valid until lc_counter_checked_free.  sizes: n_keys,
 * ev_off, read_off and status; ev_kind, ev_val and read_val are NULL (see
 * lc_counter_checked_read_vals and lc_counter_checked_batch).  result: every
 * array; err_cap = n_err. */
int  lc_counter_checked_view(const lc_counter_checked *c, lc_counter_batch *sizes, lc_counter_result *result);
/* The independent key of every key (n_keys entries). */
int  lc_counter_checked_keys(const lc_counter_checked *c, int64_t *out);
/* Why key i is :unknown (NULL when it is checked; borrowed). */
const char *lc_counter_checked_key_error(const lc_counter_checked *c, int64_t i);
/* The row of key i's error (-1 when it is checked). */
int64_t lc_counter_checked_key_error_row(const lc_counter_checked *c, int64_t i);
/* The :ok reads' values (R entries). */
int  lc_counter_checked_read_vals(const lc_counter_checked *c, int64_t *out);
/* Test and debug: the batch the device built, downloaded, in lc_counter_pack's
 * layout (borrowed, valid until lc_counter_checked_free).  The device keeps it
 * until the context's next lc_counter_check_history: c must be that context's
 * latest, else LC_E_INVALID. */
int  lc_counter_checked_batch(lc_ctx *ctx, lc_counter_checked *c, lc_counter_batch *out);
/* Times of the last lc_counter_check_history, ms: [0] upload (staging
 * included), [1] grouping and pairing, [2] the batch's build, [3] the scan
 * kernels, [4] download, [5] the whole call (wall). */
int  lc_counter_history_timing(lc_ctx *ctx, double *out6);
/* Launch constants (no device needed): [0] threads per workgroup, [1] a
 * scan's tile, [2] the largest n. */
int  lc_counter_pack_launch_info(int64_t *out3);
/* Slots of the key table (and of the process table) for n rows; a key's first
 * slot is the 64-bit MurmurHash3 finaliser of the key, masked (csrc/rows_plan.hpp). */
int64_t lc_counter_pack_table_slots(int64_t n);

#ifdef __cplusplus
}
#endif
#endif
