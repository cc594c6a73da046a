/* lincheck_counter.h -- checker/counter: the bounds of every read of a counter,
 * by a segmented prefix scan on the device (ABI 13,
 * additive).
 *
 * A section of include/lincheck.h kept in a file of its own, as
 * lincheck_setfull_stream.h is; everything here is exported by the same
 * liblincheck.so.
 *
 * THE RULES.  They restate jepsen 0.2.x's checker/counter over
 * knossos.history/complete.  This is the maintainers' reading: parity with
 * Jepsen is unpinned.  A key's history is its rows with
 * :f :add or :f :read and an integer :process; every other row is ignored.
 *   1. pairing  a completion (:ok, :fail, :info) belongs to the open
 *               invocation of its process within the key and closes it.  An
 *               :ok completion's value replaces its invocation's value.  A
 *               :fail removes both rows.  An :info, or no completion, leaves
 *               the invocation as it stands.  A completion without an open
 *               invocation, a second invocation by a process that has one
 *               open, or a completion whose :f is not its invocation's makes
 *               the key :unknown with an error.
 *   2. fold     in history order from lower = upper = 0:
 *                 invoke add v   upper += v
 *                 ok add v       lower += v
 *                 invoke read    remember lower as L
 *                 ok read v      emit the triple [L v upper]
 *   3. errors   the key is :unknown with an error when a surviving add
 *               invocation (after rule 1's replacement) or an :ok add has a
 *               value that is nil, not an integer or negative; when an :ok
 *               read's value is nil or not an integer; when the surviving
 *               add invocations sum past INT64_MAX.
 *   4. result   reads: every triple, in the order of the :ok :read rows;
 *               errors: the triples that are not L <= v <= U, same order;
 *               valid? when errors is empty.
 */
#ifndef LINCHECK_COUNTER_H
#define LINCHECK_COUNTER_H

#include "lincheck.h"

#ifdef __cplusplus
extern "C" {
#endif

/* :f of a counter-workload op map */
#define LC_CF_ADD   0
#define LC_CF_READ  1
#define LC_CF_OTHER 2   /* nemesis rows and anything else: contributes nothing */

/*
 * A raw counter history as struct-of-arrays, one row per op map, in history
 * order.
 *   process  the client's integer :process, or LC_NO_PROCESS (the row is ignored)
 *   key      the k of an independent tuple [k v], or LC_NO_KEY; NULL = no row has one
 *   value    the (unwrapped) integer :value; LC_NIL when it is nil or not an integer
 *   index    the op's :index; may be NULL
 */
typedef struct lc_counter_history {
    int64_t        n;
    const uint8_t *type;     /* LC_INVOKE / LC_OK_T / LC_FAIL / LC_INFO */
    const uint8_t *f;        /* LC_CF_*                                  */
    const int64_t *process;
    const int64_t *key;
    const int64_t *value;
    const int64_t *index;
} lc_counter_history;

/* lc_counter_batch.ev_kind */
#define LC_CE_UP   0  /* a surviving :invoke :add: upper += ev_val            */
#define LC_CE_LOW  1  /* an :ok :add: lower += ev_val                         */
#define LC_CE_RINV 2  /* the :invoke of read ev_val: its lower bound is here  */
#define LC_CE_ROK  3  /* the :ok of read ev_val: its upper bound is here      */
/* lc_counter_batch.status */
#define LC_COUNTER_KEY_OK    0
#define LC_COUNTER_KEY_ERROR 1  /* rules 1 and 3: :unknown with an error; no events, no reads */

/*
 * A packed counter batch: lc_counter_pack's output or caller-built.  Key k's
 * events, in history order and holding only the rows that matter, are
 * ev_off[k] .. ev_off[k + 1]; its :ok reads, in the order of their :ok rows,
 * are reads read_off[k] .. read_off[k + 1] of the batch, and a read event's
 * ev_val is that read's index in the batch (a read event adds nothing to
 * either sum).  Every read has one LC_CE_RINV and, after it, one LC_CE_ROK
 * event in its key.  An add event's ev_val is not negative and a key's
 * LC_CE_UP values sum to at most INT64_MAX (lc_counter_pack makes such a key
 * an error key); a caller-built batch that breaks this gets sums that wrapped.
 * lc_counter_check validates the offsets on the host; the kinds and the read
 * indices are checked where they are used, and a bad one ends the call with
 * LC_E_INVALID.
 */
typedef struct lc_counter_batch {
    int64_t         n_keys;
    const uint64_t *ev_off;    /* [n_keys + 1] */
    const uint8_t  *ev_kind;   /* LC_CE_*      */
    const int64_t  *ev_val;
    const uint64_t *read_off;  /* [n_keys + 1] */
    const int64_t  *read_val;  /* the :ok :read's value */
    const uint8_t  *status;    /* [n_keys] LC_COUNTER_KEY_*, or NULL: all OK */
} lc_counter_batch;

typedef struct lc_counter_packed lc_counter_packed;  /* library-owned */

/* independent/checker's split by key (keys in order of first appearance; one
 * key LC_NO_KEY when no row has one), rows paired by (key, process), rules 1
 * and 3 applied per key. */
int  lc_counter_pack(const lc_counter_history *h, lc_counter_packed **out);
void lc_counter_packed_free(lc_counter_packed *p);
int  lc_counter_packed_view(const lc_counter_packed *p, lc_counter_batch *out);
/* The independent key of every packed key (n_keys entries). */
int  lc_counter_packed_keys(const lc_counter_packed *p, int64_t *out);
/* Why key i is :unknown (NULL when it is checked; borrowed). */
const char *lc_counter_packed_key_error(const lc_counter_packed *p, int64_t i);

typedef struct lc_counter_opts {
    uint32_t tile;   /* events (and reads) per workgroup: 256 or 2,048; 0: the default (csrc/counter_plan.hpp) */
    uint32_t flags;  /* must be 0 */
} lc_counter_opts;

/*
 * Per key: valid (LC_UNKNOWN for an error key) and the number of its reads
 * out of bounds.  Per read of the batch: its lower and upper bound.  err_idx
 * holds the batch indices of the reads that are not lower <= value <= upper,
 * ascending; key k's are err_idx[err_off[k] .. err_off[k + 1]).  Caller-
 * allocated; R = read_off[n_keys].  err_cap is the capacity of err_idx and
 * n_err comes back: when n_err > err_cap the call returns LC_E_NOMEM, names
 * the capacity needed in lc_last_error and sets n_err to it; err_idx then
 * holds nothing to rely on (everything else is written).
 */
typedef struct lc_counter_result {
    int8_t   *valid;     /* [n_keys]     */
    uint64_t *n_errors;  /* [n_keys]     */
    int64_t  *lower;     /* [R]          */
    int64_t  *upper;     /* [R]          */
    uint64_t *err_off;   /* [n_keys + 1] */
    uint64_t *err_idx;   /* [err_cap]    */
    uint64_t  err_cap;
    uint64_t  n_err;
} lc_counter_result;

/* Check every key of the batch in one call on the context's stream (first
 * device of the context): H2D, the scan kernels, D2H. */
int  lc_counter_check(lc_ctx *ctx, const lc_counter_batch *b, const lc_counter_opts *o, lc_counter_result *r);
/* The same fold in plain C++ on one thread, no device. */
int  lc_counter_check_host(const lc_counter_batch *b, lc_counter_result *r);
/* Device-event times of the last lc_counter_check, ms: [0] upload,
 * [1] kernels, [2] download, [3] the whole call (wall). */
int  lc_counter_last_timing(lc_ctx *ctx, double *out4);
/* Launch constants (no device needed): [0] threads per workgroup, [1] the
 * default tile, [2] the smallest tile, [3] tiles per chunk of k_counter_carry. */
int  lc_counter_launch_info(int64_t *out4);

/* history.edn of a counter run: :f :add / :read with an integer or nil
 * :value, optionally inside an independent tuple [k v] (a two-element vector
 * whose first element is an integer); every other :f is LC_CF_OTHER with its
 * value skipped.  A value that is neither an integer nor nil reads as LC_NIL. */
typedef struct lc_counter_hist lc_counter_hist;  /* library-owned */
int  lc_edn_read_counter(const char *path, lc_counter_hist **out);
int  lc_edn_parse_counter(const char *text, int64_t len, lc_counter_hist **out);
int  lc_counter_hist_view(const lc_counter_hist *h, lc_counter_history *out);
void lc_counter_hist_free(lc_counter_hist *h);

#ifdef __cplusplus
}
#endif
#endif
