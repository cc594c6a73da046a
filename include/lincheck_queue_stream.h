/* lincheck_queue_stream.h -- streaming checker/total-queue and checker/unique-ids:
 * a tally that stays resident on the device, verdicts after every append
 * (ABI 13, additive).
 *
 * A section of include/lincheck.h kept in a file of its own:
 * lincheck_queue.h lists exactly the one-shot entry points (its tests pin that
 * list), and everything here is exported by the same liblincheck.so.
 *
 * Both checkers keep a multiset of values per key, so the state after row n
 * depends on rows 0..n only.  Nothing is held back: after ANY append the exact
 * answer for everything appended so far exists.  The multisets live in a
 * concurrent hash table on the device between calls; an append uploads only
 * its own rows, and its cost follows those rows and the keys they touch, not
 * the table.
 *
 * THE CONTRACT.  For any split of a history into appends and either mode,
 * after every append the keys in their order, the per-key valid and seven
 * counts, lo / hi / has_range and the entries sorted by (key, class, value)
 * equal lc_queue_pack + lc_queue_check_host of the concatenation of all rows
 * appended so far.  There is no finish.
 *   valid       is NOT monotone (a value lost now may be dequeued later): an
 *               update names every key whose valid differs from before the
 *               call, in either direction
 *   rules       lincheck_queue.h's, unchanged.  An :info drain makes its key
 *               :unknown with the one-shot path's error from the append that
 *               holds it on: the key's counts read 0, it has no entries, and
 *               none of its rows, of that append or a later one, contributes.
 *               Other keys are unaffected
 *   keyedness   fixed, as lincheck_setfull_stream.h fixes it, by the first
 *               append that holds a row with a key or with a queue or id :f
 *               (anything but LC_QF_OTHER): keyed when some row of it has a
 *               key (its rows without one are ignored, as the one-shot pack
 *               ignores them), else the single key LC_NO_KEY.  Until then the
 *               stream reads as the one-shot check of an empty history does:
 *               one key LC_NO_KEY, valid, all counts 0.  A later append of the
 *               other kind, and an append with a bad :type / :f code, is
 *               refused whole with LC_E_INVALID and leaves the stream as it was
 *   changed     a key first seen in this call counts as valid (what a key
 *               without rows is) before it
 *   size        the packed rows of a stream stay below 2^32 (the 32-bit
 *               tallies cannot wrap): the append that would pass that is
 *               refused whole with LC_E_UNSUPPORTED; one that would pass the
 *               table's byte cap (csrc/queue_stream_plan.hpp) with LC_E_NOMEM.
 *               Either leaves the stream as it was
 * ctx NULL opens a HOST STREAM: the same contract by an incremental fold on
 * one thread, lc_queue_check_host's std::unordered_map kept between appends.
 * A context of several devices or with a communicator is refused with
 * LC_E_UNSUPPORTED, as lc_stream_open does.  One stream is used by one thread
 * at a time; its calls take the context's lock.
 */
#ifndef LINCHECK_QUEUE_STREAM_H
#define LINCHECK_QUEUE_STREAM_H

#include "lincheck_queue.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lc_queue_stream lc_queue_stream; /* library-owned */

typedef struct lc_queue_stream_opts {
    uint32_t slots;  /* the table's first size: a power of two; 0: the default (csrc/queue_stream_plan.hpp) */
    uint32_t flags;  /* must be 0 */
} lc_queue_stream_opts;

typedef struct lc_queue_stream_update {
    int64_t  n_keys;         /* keys so far                                              */
    int64_t  rows;           /* history rows appended so far                             */
    int64_t  packed;         /* packed rows (values that count) of this call             */
    int64_t  distinct;       /* distinct (key, value) resident, every key's              */
    int64_t  slots;          /* the table's slots after this call                        */
    int64_t  grew;           /* 1 when this call grew the table first                    */
    int64_t  n_changed;      /* keys whose valid differs from before this call ...       */
    const int64_t *changed;  /* ... their indices, ascending (borrowed until next call)  */
} lc_queue_stream_update;

/* mode: LC_QM_*.  o may be NULL (the defaults). */
int  lc_queue_stream_open(lc_ctx *ctx, uint32_t mode, const lc_queue_stream_opts *o, lc_queue_stream **out);
/* rows: the next rows of the history.  u may be NULL. */
int  lc_queue_stream_append(lc_queue_stream *s, const lc_queue_history *rows, lc_queue_stream_update *u);
/* Per key so far, as lc_queue_result's arrays of the same names ([n_keys],
 * counts [n_keys][LC_QN_COUNTS]).  Reads nothing from the table. */
int  lc_queue_stream_counts(lc_queue_stream *s, int8_t *valid, uint64_t *counts, int64_t *lo, int64_t *hi, uint8_t *has_range);
/* Everything, entries included, with lc_queue_check's ent_cap / LC_E_NOMEM protocol. */
int  lc_queue_stream_results(lc_queue_stream *s, lc_queue_result *r);
/* Keys in order of first appearance; returns their number (out may be NULL). */
int64_t lc_queue_stream_keys(const lc_queue_stream *s, int64_t *out);
/* Why key i is :unknown (NULL when it is checked; borrowed). */
const char *lc_queue_stream_key_error(const lc_queue_stream *s, int64_t i);
/* The last append, ms: [0] pack (host), [1] upload, [2] tally, settle and
 * gather kernels, [3] readback, [4] the grow step (0 when the table did not
 * grow), [5] the whole call (wall).  A host stream: [0] pack, [2] the fold, [5]. */
int  lc_queue_stream_last_timing(const lc_queue_stream *s, double *out6);
/* Launch constants (no device needed): [0] threads per workgroup, [1] the
 * slots-per-value bound a grow restores, [2] bytes per slot, [3] the table's
 * byte cap, [4] the default first slots, [5] the rows of one launch. */
int  lc_queue_stream_launch_info(int64_t *out6);
void lc_queue_stream_close(lc_queue_stream *s);

#ifdef __cplusplus
}
#endif
#endif
