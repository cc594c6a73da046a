/* lincheck_queue.h -- checker/total-queue and checker/unique-ids: a multiset of
 * values per key, tallied in a concurrent hash table on the device, and every
 * distinct value classified from its counts (ABI 13,
 * additive).
 *
 * A section of include/lincheck.h kept in a file of its own, as
 * lincheck_counter.h is; everything here is exported by the same
 * liblincheck.so.
 *
 * THE RULES.  They restate jepsen 0.2.x's checker/total-queue and
 * checker/unique-ids.  This is the maintainers' reading: parity with Jepsen is
 * unpinned.  Values are integers or nil; nil is LC_NIL, a
 * value like any other that orders below every integer.  A value that is
 * neither is refused by the readers (LC_E_UNSUPPORTED).  Rows are split by
 * independent key: keys in order of first appearance, and one key LC_NO_KEY
 * when no row has one (a row without a key among rows with keys is ignored).
 * No pairing by process is needed.
 *
 * total-queue, per key:
 *   1. drains   a row with :f :drain that is an :invoke or a :fail is dropped;
 *               an :ok drain whose value is a vector of n elements stands for
 *               n :ok :dequeue rows, one per element, in order; an :info
 *               drain makes the key :unknown with the error "Not sure how to
 *               handle a crashed drain operation".
 *   2. tallies  three multisets: attempts, the values of :invoke :enqueue
 *               rows; enqueues, of :ok :enqueue rows; dequeues, of :ok
 *               :dequeue rows, expanded ones included.  Every other row
 *               contributes nothing.
 *   3. classes  for each distinct value with multiplicities a, e, d in those:
 *                 ok          min(d, a)
 *                 unexpected  d when a = 0, else 0
 *                 duplicated  max(d - a, 0) when a > 0, else 0
 *                 lost        max(e - d, 0)
 *                 recovered   max(min(d, a) - e, 0)
 *   4. result   valid? when lost and unexpected are empty (duplicates alone do
 *               not invalidate); attempt-count (the sum of a), acknowledged-
 *               count (of e), ok-, unexpected-, duplicated-, lost- and
 *               recovered-count, each the sum of its class; lost, unexpected,
 *               duplicated, recovered: each class as a sorted list with
 *               repeats, ascending, nil first.
 *
 * unique-ids, per key, over the :f :generate rows:
 *   attempted-count     the number of :invoke rows
 *   acknowledged-count  the number of :ok rows; their values are the acks
 *   duplicated-count    the number of distinct values acknowledged more than once
 *   duplicated          value -> count of the 48 duplicates with the highest
 *                       counts, ties broken towards the larger value,
 *                       presented in ascending value order (the binding's;
 *                       this library returns every duplicate)
 *   range               [min max] of the acks; none without any
 *   valid?              when there is no duplicate
 */
#ifndef LINCHECK_QUEUE_H
#define LINCHECK_QUEUE_H

#include "lincheck.h"

#ifdef __cplusplus
extern "C" {
#endif

/* :f of a queue- or id-workload op map */
#define LC_QF_ENQUEUE  0
#define LC_QF_DEQUEUE  1
#define LC_QF_DRAIN    2
#define LC_QF_GENERATE 3
#define LC_QF_OTHER    4   /* nemesis rows and anything else: contributes nothing */

/* which checker a pack, a batch and a result are for */
#define LC_QM_TOTAL_QUEUE 0
#define LC_QM_UNIQUE_IDS  1

/*
 * A raw history as struct-of-arrays, one row per op map, in history order.
 *   key        the k of an independent tuple [k v], or LC_NO_KEY; NULL = no row has one
 *   value      the (unwrapped) integer :value, LC_NIL for nil; unused on a drain row
 *   drain_off  [n + 1]: row r's drained elements are drain_val[drain_off[r] ..
 *              drain_off[r + 1]) (empty on every row but an :ok :drain);
 *              NULL = no row has any
 */
typedef struct lc_queue_history {
    int64_t         n;
    const uint8_t  *type;       /* LC_INVOKE / LC_OK_T / LC_FAIL / LC_INFO */
    const uint8_t  *f;          /* LC_QF_*                                  */
    const int64_t  *key;
    const int64_t  *value;
    const uint64_t *drain_off;
    const int64_t  *drain_val;
} lc_queue_history;

/* lc_queue_batch.row_kind: the multiset a row's value goes to */
#define LC_QK_ATTEMPT 0  /* :invoke :enqueue                                     */
#define LC_QK_ACK     1  /* :ok :enqueue; unique-ids: :ok :generate (its only kind) */
#define LC_QK_DEQUEUE 2  /* :ok :dequeue, and every element of an :ok :drain      */
/* lc_queue_batch.status */
#define LC_QUEUE_KEY_OK    0
#define LC_QUEUE_KEY_ERROR 1  /* rule 1: :unknown with an error; its rows contribute nothing */

/*
 * A packed batch: lc_queue_pack's output or caller-built.  One row per value
 * that counts, in any order: rows need not be grouped by key.  The call
 * validates row_key < n_keys and row_kind where they are used, and a bad one
 * ends it with LC_E_INVALID.  n_rows is at most 2^29 (the table's byte cap,
 * csrc/queue_plan.hpp).
 */
typedef struct lc_queue_batch {
    int64_t         n_keys;
    int64_t         n_rows;
    uint32_t        mode;       /* LC_QM_*                                        */
    uint32_t        reserved;   /* must be 0                                      */
    const uint32_t *row_key;    /* dense key id                                   */
    const uint8_t  *row_kind;   /* LC_QK_*                                        */
    const int64_t  *row_val;
    const uint8_t  *status;     /* [n_keys] LC_QUEUE_KEY_*, or NULL: all OK       */
    const uint64_t *attempted;  /* [n_keys] unique-ids' :invoke rows, or NULL: 0  */
} lc_queue_batch;

typedef struct lc_queue_packed lc_queue_packed;  /* library-owned */

/* independent/checker's split by key and the drop and expansion rules; nothing
 * per value (interning values is the check itself, and the device's). */
int  lc_queue_pack(const lc_queue_history *h, uint32_t mode, lc_queue_packed **out);
void lc_queue_packed_free(lc_queue_packed *p);
int  lc_queue_packed_view(const lc_queue_packed *p, lc_queue_batch *out);
/* The independent key of every packed key (n_keys entries). */
int  lc_queue_packed_keys(const lc_queue_packed *p, int64_t *out);
/* Why key i is :unknown (NULL when it is checked; borrowed). */
const char *lc_queue_packed_key_error(const lc_queue_packed *p, int64_t i);

typedef struct lc_queue_opts {
    uint32_t slots;  /* the table's slots: a power of two >= n_rows; 0: the default (csrc/queue_plan.hpp) */
    uint32_t flags;  /* must be 0 */
} lc_queue_opts;

/* lc_queue_result.counts[k][..] */
#define LC_QN_ATTEMPT      0  /* unique-ids: attempted-count    */
#define LC_QN_ACKNOWLEDGED 1  /* unique-ids: acknowledged-count */
#define LC_QN_OK           2  /* unique-ids: duplicated-count   */
#define LC_QN_UNEXPECTED   3
#define LC_QN_DUPLICATED   4
#define LC_QN_LOST         5
#define LC_QN_RECOVERED    6
#define LC_QN_COUNTS       7
/* lc_queue_result.ent_class, in the order of the result's lists */
#define LC_QC_LOST       0
#define LC_QC_UNEXPECTED 1
#define LC_QC_DUPLICATED 2  /* unique-ids' only class */
#define LC_QC_RECOVERED  3

/*
 * Per key: valid (LC_UNKNOWN for an error key, whose counts are 0), the seven
 * counts, and for unique-ids the range of the acks: lo / hi are written only
 * where has_range is 1.  An entry is one distinct (key, value) with a non-zero
 * multiplicity in one of the four listed classes (total-queue), or
 * acknowledged more than once (unique-ids: class LC_QC_DUPLICATED, ent_mult
 * its count).  Entries come back sorted by (key, class, value).  Caller-
 * allocated.  ent_cap is the capacity of the four ent_ arrays and n_ent comes
 * back: when n_ent > ent_cap the call returns LC_E_NOMEM, names the capacity
 * needed in lc_last_error and sets n_ent to it; the ent_ arrays then hold
 * nothing to rely on (everything else is written).
 */
typedef struct lc_queue_result {
    int8_t   *valid;      /* [n_keys]                  */
    uint64_t *counts;     /* [n_keys][LC_QN_COUNTS]    */
    int64_t  *lo;         /* [n_keys]                  */
    int64_t  *hi;         /* [n_keys]                  */
    uint8_t  *has_range;  /* [n_keys]                  */
    uint32_t *ent_key;    /* [ent_cap]                 */
    uint8_t  *ent_class;  /* [ent_cap] LC_QC_*         */
    int64_t  *ent_val;    /* [ent_cap]                 */
    uint64_t *ent_mult;   /* [ent_cap]                 */
    uint64_t  ent_cap;
    uint64_t  n_ent;
} lc_queue_result;

/* Check every key of the batch in one call on the context's stream (first
 * device of the context): H2D, reset, tally, classify, D2H, the entries' sort. */
int  lc_queue_check(lc_ctx *ctx, const lc_queue_batch *b, const lc_queue_opts *o, lc_queue_result *r);
/* The same fold in plain C++ on one thread, no device. */
int  lc_queue_check_host(const lc_queue_batch *b, lc_queue_result *r);
/* Device-event times of the last lc_queue_check, ms: [0] upload, [1] kernels,
 * [2] download, [3] the whole call (wall). */
int  lc_queue_last_timing(lc_ctx *ctx, double *out4);
/* Launch constants (no device needed): [0] threads per workgroup, [1] the
 * default slots per row (the reciprocal of the default load factor's bound),
 * [2] bytes per slot, [3] the table's byte cap. */
int  lc_queue_launch_info(int64_t *out4);

/* history.edn of a queue or id-generator run: :f :enqueue / :dequeue / :drain /
 * :generate; every other :f is LC_QF_OTHER with its value skipped.  A value is
 * an integer or nil, optionally inside an independent tuple [k v] (a
 * two-element vector whose first element is an integer).  A drain's value is
 * nil or a vector of integers (nil elements allowed), or [k that]: on a drain
 * row a two-element vector is a tuple when its second element is nil or a
 * vector, and the drained elements otherwise.  Anything else is refused with
 * LC_E_UNSUPPORTED. */
typedef struct lc_queue_hist lc_queue_hist;  /* library-owned */
int  lc_edn_read_queue(const char *path, lc_queue_hist **out);
int  lc_edn_parse_queue(const char *text, int64_t len, lc_queue_hist **out);
int  lc_queue_hist_view(const lc_queue_hist *h, lc_queue_history *out);
void lc_queue_hist_free(lc_queue_hist *h);

#ifdef __cplusplus
}
#endif
#endif
