/* lincheck_counter_stream.h -- streaming checker/counter: the two running sums
 * of every key and every read's bounds stay resident, verdicts after every
 * append (ABI 13, additive).
 *
 * A section of include/lincheck.h kept in a file of its own: lincheck_counter.h
 * lists exactly the one-shot entry points (its test pins that list), and
 * everything here is exported by the same liblincheck.so.
 *
 * THE CONTRACT.  For any split of a history into appends, after EVERY append
 * the following equal lc_counter_pack + lc_counter_check_host of the
 * concatenation of all rows appended so far:
 *   - the keys, in order of first appearance;
 *   - per key valid (LC_UNKNOWN included) and n_errors;
 *   - per read lower and upper, in the batch's order: key-major, and within a
 *     key in the order of its :ok :read rows;
 *   - err_off and err_idx.
 * There is no finish.  The rules are lincheck_counter.h's, unchanged; an open
 * invocation counts "as it stands", exactly as the one-shot pack treats the
 * end of a history.
 *   not final   PAST ANSWERS ARE REVISED.  A :fail removes an :invoke :add
 *               that earlier reads counted in their upper bound; an :ok may
 *               replace its invocation's value.  The upper bound of every read
 *               of that key completed since the invocation changes, and valid
 *               can move in either direction.  An update names every key whose
 *               valid differs from before the call, in any direction among
 *               valid / invalid / unknown; a key first seen in this call
 *               counts as valid before it
 *   unknown     a pairing error, a bad :ok :add value and a bad :ok :read
 *               value are PERMANENT: from that append on the key has no reads
 *               and none of its rows contributes.  A surviving :invoke :add
 *               with a nil, non-integer or negative value makes the key
 *               :unknown only WHILE IT SURVIVES, and a surviving sum past
 *               INT64_MAX only while that lasts: a later :ok with a good
 *               value, or a :fail, brings such a key back with all its reads
 *               and the right bounds.  lc_counter_stream_key_error names one
 *               reason that holds (the one-shot pack names the first in
 *               history order)
 *   keyedness   fixed, as lincheck_queue_stream.h fixes it, by the first
 *               append that holds a client row (a row with a key or with :f
 *               :add / :read): keyed when some row of it has a key (its rows
 *               without one are ignored, as the one-shot pack ignores them),
 *               else the single key LC_NO_KEY.  Until then the stream reads as
 *               the one-shot check of an empty history: one key LC_NO_KEY,
 *               valid, no reads
 *   refusals    leave the stream as it was: LC_E_INVALID for a later append of
 *               the other keyedness and for a bad :type / :f code;
 *               LC_E_UNSUPPORTED for an append that could take the stream's
 *               reads or events to 2^32 (counted before anything is folded:
 *               its :ok :read rows are the reads it can add, its :add / :read
 *               rows the events); LC_E_NOMEM for one whose reads would need a
 *               reads array past the byte cap (csrc/counter_stream_plan.hpp)
 * ctx NULL opens a HOST STREAM: the same contract by an incremental fold on
 * one thread.  A context of several devices or with a communicator is refused
 * with LC_E_UNSUPPORTED, as lc_stream_open does.  One stream is used by one
 * thread at a time; its calls take the context's lock.
 */
#ifndef LINCHECK_COUNTER_STREAM_H
#define LINCHECK_COUNTER_STREAM_H

#include "lincheck_counter.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lc_counter_stream lc_counter_stream; /* library-owned */

typedef struct lc_counter_stream_opts {
    uint32_t tile;           /* events per workgroup: 256 or 2,048, as lc_counter_opts.tile; 0: the default */
    uint32_t reads;          /* the reads array's first capacity; 0: the default (csrc/counter_stream_plan.hpp) */
    uint32_t launch_events;  /* the events of one launch; 0: the default */
    uint32_t flags;          /* must be 0 */
} lc_counter_stream_opts;

typedef struct lc_counter_stream_update {
    int64_t  n_keys;         /* keys so far                                              */
    int64_t  rows;           /* history rows appended so far                             */
    int64_t  events;         /* packed events of this call                               */
    int64_t  reads;          /* reads (:ok :read rows that count) of this call           */
    int64_t  reads_total;    /* reads resident, every key's                              */
    int64_t  patched;        /* invocations of earlier appends that this call revised    */
    int64_t  revisited;      /* resident reads looked at again because of them           */
    int64_t  grew;           /* 1 when this call grew the reads array first              */
    int64_t  n_changed;      /* keys whose valid differs from before this call ...       */
    const int64_t *changed;  /* ... their indices, ascending (borrowed until next call)  */
} lc_counter_stream_update;

/* o may be NULL (the defaults). */
int  lc_counter_stream_open(lc_ctx *ctx, const lc_counter_stream_opts *o, lc_counter_stream **out);
/* rows: the next rows of the history.  u may be NULL. */
int  lc_counter_stream_append(lc_counter_stream *s, const lc_counter_history *rows, lc_counter_stream_update *u);
/* Per key so far ([n_keys] each): valid, n_errors, and the reads it has in
 * results() (0 for an :unknown key).  Reads nothing from the device. */
int  lc_counter_stream_counts(lc_counter_stream *s, int8_t *valid, uint64_t *n_errors, uint64_t *n_reads);
/* Everything, with lc_counter_check's err_cap / LC_E_NOMEM protocol; lower and
 * upper hold the sum of counts()' n_reads.  value may be NULL; else the reads'
 * values in the same order.  May cost the whole history. */
int  lc_counter_stream_results(lc_counter_stream *s, lc_counter_result *r, int64_t *value);
/* Keys in order of first appearance; returns their number (out may be NULL). */
int64_t lc_counter_stream_keys(const lc_counter_stream *s, int64_t *out);
/* Why key i is :unknown (NULL when it is checked; borrowed until the next append). */
const char *lc_counter_stream_key_error(const lc_counter_stream *s, int64_t i);
/* The last append, ms: [0] pack (host), [1] upload, [2] kernels, [3] readback,
 * [4] the grow step (0 when nothing grew), [5] the whole call (wall).  A host
 * stream: [0] pack, [2] the fold, [5]. */
int  lc_counter_stream_last_timing(const lc_counter_stream *s, double *out6);
/* Launch constants (no device needed): [0] threads per workgroup, [1] the
 * default tile, [2] bytes per resident read, [3] the reads array's byte cap,
 * [4] the default first capacity, [5] the default events of one launch. */
int  lc_counter_stream_launch_info(int64_t *out6);
void lc_counter_stream_close(lc_counter_stream *s);

#ifdef __cplusplus
}
#endif
#endif
