/* lincheck_setfull_stream.h -- streaming checker/set-full: per-element verdicts
 * while the set test runs (ABI 13, additive).
 *
 * A section of include/lincheck.h kept in a file of its own: lincheck.h's
 * set-full section lists exactly the one-shot entry points (its tests pin that
 * list), and everything here is exported by the same liblincheck.so.
 *
 * checker/set-full is a causal fold: the state after row n depends on rows
 * 0..n only.  So there is no decided prefix and no held-back row: after ANY
 * append the exact answer for everything appended so far exists.  Per element
 * the carried state is three ops (known, last-present, last-absent), the
 * position of its last :invoke :add and its first :ok :add since; it lives on
 * the device between calls, one record per element id, and an append folds
 * only its own :ok reads into the records.
 *
 * THE CONTRACT.  For any split of a history into appends, after every append
 * the per-key valid and six counts, and per ELEMENT (by value) outcome,
 * latency, known position, last-absent position and the duplicated flag equal
 * lc_setfull_pack + lc_setfull_check of the concatenation of all rows appended
 * so far under the same `linearizable`.  There is no finish.
 *   positions   a row's position is its running row number over all appends
 *   semantics   lincheck.h's set-full fold, unchanged; a row that breaks an
 *               error rule makes its key :unknown with that error from the
 *               append that holds the row on (such a key reports no ids)
 *   reads       an :invoke :read of one append pairs with its :ok :read in a
 *               later one (the packer keeps the open read per process)
 *   keyedness   fixed by the first append that holds a client row (an :add or
 *               :read row): keyed when some row has a key, else the single
 *               key LC_NO_KEY.  A later append of the other kind, and an
 *               append with a bad :type / :f code, is refused whole with
 *               LC_E_INVALID and leaves the stream as it was
 *   ids         per key, stable, in order of first appearance (an :invoke :add
 *               or a value inside an :ok :read).  Not plan_set_key's numbering:
 *               compare with the one-shot path through element values
 * ctx NULL opens a PACKER-ONLY stream: appends build chunks, the accessors
 * work, results do not.  A context of several devices or with a communicator
 * is refused with LC_E_UNSUPPORTED, as lc_stream_open does.  One stream is
 * used by one thread at a time; its calls take the context's lock.
 */
#ifndef LINCHECK_SETFULL_STREAM_H
#define LINCHECK_SETFULL_STREAM_H

#include "lincheck.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lc_setfull_stream lc_setfull_stream; /* library-owned */

typedef struct lc_setfull_stream_update {
    int64_t n_keys;         /* keys so far                                             */
    int64_t rows;           /* rows appended so far (the next row's position)          */
    int64_t reads;          /* :ok reads folded in this call                           */
    int64_t ids;            /* element ids resident, all checked keys                  */
    int64_t n_changed;      /* keys whose valid differs from before this call ...      */
    const int64_t *changed; /* ... their indices, ascending (borrowed until next call) */
} lc_setfull_stream_update;

/* lc_setfull_stream_chunk.en_flags */
#define LC_SFS_FRESH 0x1u /* an :invoke :add in this chunk: the record starts over at en_inv_pos */
#define LC_SFS_ACK   0x2u /* the first :ok :add since the id's current invocation                */

/*
 * What the last append sends to the device (borrowed until the next call).
 * Only keys touched by the append and still checked appear.  Touched key t is
 * key tk_key[t]; it has tk_n_ids[t] ids in blocks of 256, whose resident block
 * numbers are blk[tk_blk_off[t] ..tk_blk_off[t + 1]) (id i's record is slot
 * 256 * blk[tk_blk_off[t] + i / 256] + i % 256); its new :ok reads, in
 * completion order, are rows tk_row_off[t] .. tk_row_off[t + 1]; row r's ids
 * (the key's own numbering) are read_id[el_off[r] .. el_off[r + 1]).
 * Entries: at most one per touched id.
 */
typedef struct lc_setfull_stream_chunk {
    int64_t         n_touched;
    const int64_t  *tk_key;      /* [n_touched] index into the stream's keys */
    const uint32_t *tk_n_ids;    /* [n_touched] */
    const uint64_t *tk_row_off;  /* [n_touched + 1] */
    const uint64_t *tk_blk_off;  /* [n_touched + 1] */
    const uint32_t *blk;
    int64_t         n_entries;
    const uint32_t *en_t;        /* touched key of the entry */
    const uint32_t *en_id;
    const uint32_t *en_flags;    /* LC_SFS_* */
    const int64_t  *en_inv_pos;  /* LC_SFS_FRESH: the LAST :invoke :add of the chunk */
    const int64_t  *en_ack_pos;  /* LC_SFS_ACK */
    const int64_t  *en_ack_time;
    const int64_t  *row_pos;     /* per row, as lc_setfull_batch's */
    const int64_t  *row_time;
    const int64_t  *row_inv_pos;
    const int64_t  *row_inv_time;
    const uint64_t *el_off;      /* [rows + 1] */
    const uint32_t *read_id;
} lc_setfull_stream_chunk;

/* o: linearizable and max_matrix_bytes (0: the default, csrc/setfull_stream_plan.hpp); flags must be 0. */
int  lc_setfull_stream_open(lc_ctx *ctx, const lc_setfull_opts *o, lc_setfull_stream **out);
/* rows: the next rows of the history (index is not read).  u may be NULL. */
int  lc_setfull_stream_append(lc_setfull_stream *s, const lc_setfull_history *rows, lc_setfull_stream_update *u);
/* Per key so far: valid [n_keys] and counts [6 * n_keys], as lc_setfull_result's. */
int  lc_setfull_stream_counts(lc_setfull_stream *s, int8_t *valid, uint64_t *counts);
/* Key `key`'s ids (0 for an error key); with elems, the first min(ids, cap) elements by id. */
int64_t lc_setfull_stream_ids(const lc_setfull_stream *s, int64_t key, int64_t *elems, int64_t cap);
/* Everything: valid and counts per key, the per-id arrays for key 0's ids,
 * then key 1's ..., each in lc_setfull_stream_ids order (update.ids in all). */
int  lc_setfull_stream_results(lc_setfull_stream *s, lc_setfull_result *r);
/* Keys in order of first appearance; returns their number (out may be NULL). */
int64_t lc_setfull_stream_keys(const lc_setfull_stream *s, int64_t *out);
/* Why key i is :unknown (NULL when it is checked; borrowed). */
const char *lc_setfull_stream_key_error(const lc_setfull_stream *s, int64_t i);
/* Key `key`'s largest multiplicity in one read per id, [ids] (0 or 1: never held twice). */
int  lc_setfull_stream_multiplicity(const lc_setfull_stream *s, int64_t key, uint32_t *out, int64_t cap);
/* The last append's chunk. */
int  lc_setfull_stream_last_chunk(const lc_setfull_stream *s, lc_setfull_stream_chunk *out);
/* The last append, ms: [0] pack (host), [1] upload, [2] mark kernels (with the
 * matrices' zeroing), [3] reset, fold and finish kernels, [4] readback, then
 * [5] row passes. */
int  lc_setfull_stream_last_timing(const lc_setfull_stream *s, double *out_ms);
void lc_setfull_stream_close(lc_setfull_stream *s);

#ifdef __cplusplus
}
#endif
#endif
