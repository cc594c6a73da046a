/* lincheck_perf_pack.h -- checker/perf from raw rows: the history is paired
 * and packed on the device, and lc_perf_check's kernels run on the batch where
 * it lies (ABI 13, additive).
 *
 * A section of include/lincheck.h's checker/perf kept in a file of its own, as
 * lincheck_counter_pack.h is; everything here is exported by the same
 * liblincheck.so.  The structs and the rules are lincheck.h's.
 *
 * lc_perf_check_history(h, o) equals lc_perf_pack(h) followed by
 * lc_perf_check, in every field: the batch (n, n_matched, the four bounds,
 * n_f, t_comp, t_inv and meta in history order), the four info numbers, the
 * nemesis intervals, and the result (rate_first, rate_n, q_first, q_n, rate,
 * group, quant).  Where that pair fails this call fails with the same code: a
 * bad :type / :f code names the lowest offending row, a matched invocation
 * whose :time is INT64_MIN names the row lc_perf_pack names.
 *
 * One call uploads type, f, process and time (18 bytes a row), through pinned
 * staging when the caller's arrays are not page-locked.  Everything else runs
 * on the context's first device and stream, and only the tables, the counts,
 * the bounds and the nemesis rows come back: there is no host pass over the
 * rows.  The context must have one device and no communicator, and n at most
 * 2^31 - 16: else LC_E_UNSUPPORTED.  A history of no rows touches no device.
 */
#ifndef LINCHECK_PERF_PACK_H
#define LINCHECK_PERF_PACK_H

#include "lincheck.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lc_perf_checked lc_perf_checked;  /* library-owned: the tables' sizes are not known up front */

int  lc_perf_check_history(lc_ctx *ctx, const lc_perf_history *h, const lc_perf_opts *o, lc_perf_checked **out);
void lc_perf_checked_free(lc_perf_checked *c);
/* Borrowed host arrays, valid until lc_perf_checked_free.  sizes: the counts
 * and bounds of lc_perf_packed_view with t_comp, t_inv and meta NULL (see
 * lc_perf_checked_records).  result: the three tables, each cap its size. */
int  lc_perf_checked_view(const lc_perf_checked *c, lc_perf_batch *sizes, lc_perf_result *result);
/* lc_perf_packed_info's numbers: matched, unmatched, orphans, intervals. */
int  lc_perf_checked_info(const lc_perf_checked *c, int64_t *out4);
/* lc_perf_packed_intervals' pairs (2 x intervals entries). */
int  lc_perf_checked_intervals(const lc_perf_checked *c, int64_t *out);
/* The record columns the device built, downloaded on demand, in
 * lc_perf_pack's layout (borrowed, valid until lc_perf_checked_free).  The
 * device keeps them until the context's next lc_perf_check_history or
 * lc_perf_check: c must be that context's latest, else LC_E_INVALID. */
int  lc_perf_checked_records(lc_ctx *ctx, lc_perf_checked *c, lc_perf_batch *out);
/* Times of the last lc_perf_check_history, ms: [0] upload (staging included),
 * [1] grouping and pairing, [2] the batch's build, [3] the perf kernels,
 * [4] download, [5] the whole call (wall). */
int  lc_perf_history_timing(lc_ctx *ctx, double *out6);
/* Launch constants (no device needed): [0] threads per workgroup, [1] a
 * scan's tile, [2] the largest n. */
int  lc_perf_pack_launch_info(int64_t *out3);

#ifdef __cplusplus
}
#endif
#endif
