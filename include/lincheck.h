/*
 * lincheck.h -- C ABI of the MI355X linearizability checker (liblincheck.so).
 *
 * Drop-in for the check phase of the Jepsen etcd demo:
 *
 *   (independent/checker
 *     (checker/compose
 *       {:linear (checker/linearizable {:model (model/cas-register)
 *                                       :algorithm :linear}) ...}))
 *
 * at /root/reference/src/jepsen/etcdemo.clj:115-119.  The reference path is
 * jepsen.independent/checker -> jepsen.checker/linearizable ->
 * knossos.linear/analysis (knossos 0.3.7, jepsen.etcdemo.iml:58), all Clojure.
 * Nothing in the reference is native, so every entry point below replaces a
 * Clojure function; each cites the reference call site it stands behind.
 *
 * Layers:
 *   lc_synth_*   synthetic cas-register histories with the demo's shape
 *                (etcdemo.clj:67-69, :83-105, :120-125).          [test input]
 *   lc_edn_*     Jepsen history.edn reader/writer (store/ layout,
 *                .gitignore:13; SURVEY F-1).                        [ingest]
 *   lc_pack      jepsen.independent/subhistory + knossos.history complete /
 *                without-failures + knossos.model.memo, producing packed
 *                per-key event streams (rows A1-A5).                 [host]
 *   lc_check_*   knossos.linear/analysis on the GPU (rows A6, A7) and the
 *                per-key verdict records jepsen.checker/linearizable and
 *                independent/checker turn into result maps (A8, A9). [device]
 *
 * Conventions: the caller owns every array it passes in or out.  The library
 * copies inputs to the device and never keeps caller pointers after a call
 * returns.  Every function returns 0 on success and a negative LC_E_* code on
 * failure; lc_last_error() (thread-local) describes the last failure.  The
 * library never calls exit() or abort().  One lc_ctx serialises its own calls
 * with an internal mutex; distinct contexts may run concurrently.
 */
#ifndef LINCHECK_H
#define LINCHECK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LC_ABI_VERSION 13

/* ---- error codes --------------------------------------------------------- */
#define LC_OK            0
#define LC_E_INVALID    -1  /* bad argument / malformed history               */
#define LC_E_NOMEM      -2  /* host or device allocation failed               */
#define LC_E_DEVICE     -3  /* HIP runtime error / no usable gfx950 device    */
#define LC_E_PARSE      -4  /* EDN syntax error                               */
#define LC_E_UNSUPPORTED -5 /* op the cas-register model cannot step          */
#define LC_E_IO         -6  /* file could not be read / written               */

/* ---- history vocabulary (etcdemo.clj:67-69, :83-105) --------------------- */
/* :type of an op map */
#define LC_INVOKE 0
#define LC_OK_T   1
#define LC_FAIL   2
#define LC_INFO   3
/* :f of an op map */
#define LC_F_READ  0
#define LC_F_WRITE 1
#define LC_F_CAS   2
#define LC_F_OTHER 3   /* nemesis :start/:stop and anything else */
#define LC_F_ACQUIRE 4 /* (model/mutex) :acquire                  */
#define LC_F_RELEASE 5 /* (model/mutex) :release                  */
#define LC_F_TXN     6 /* (model/multi-register) :txn            */

/* A :txn value is a sequence of micro-ops [f k v] (knossos.model/multi-register):
 * f LC_MOP_READ (v nil reads anything) or LC_MOP_WRITE, k a register id, v
 * an integer or LC_NIL.  lc_history.mop holds them as int64 triples. */
#define LC_MOP_READ  0
#define LC_MOP_WRITE 1
/* Register ids from LC_NAMED_REG_BASE up name non-integer registers (:x ...):
 * lc_edn_read gives the i-th distinct name LC_NAMED_REG_BASE + i
 * (lc_hist_reg_name). */
#define LC_NAMED_REG_BASE ((int64_t)1 << 62)

#define LC_NIL        INT64_MIN  /* a nil value                                */
#define LC_NO_KEY     INT64_MIN  /* :value is not an independent tuple [k v]   */
#define LC_NO_PROCESS INT64_MIN  /* :process is not an integer (:nemesis)      */

/*
 * A raw Jepsen history as struct-of-arrays, one row per op map, in history
 * order.  This is what the Clojure side marshals a `history` vector into
 * (INTEGRATION.md), what lc_edn_read produces and what lc_synth emits.
 *   key   the k of an independent tuple [k v] (jepsen.independent/tuple,
 *         etcdemo.clj:90,120) or LC_NO_KEY;
 *   v0/v1 the unwrapped v: read/write -> v0 (v1 = LC_NIL); cas [old new] ->
 *         v0 = old, v1 = new; LC_NIL for nil;
 *   index the op's :index, or -1 when the map has none.
 */
typedef struct lc_history {
    int64_t        n;
    const uint8_t *type;     /* LC_INVOKE / LC_OK_T / LC_FAIL / LC_INFO */
    const uint8_t *f;        /* LC_F_*                                   */
    const int64_t *process;  /* or LC_NO_PROCESS                         */
    const int64_t *key;      /* or LC_NO_KEY                             */
    const int64_t *v0;
    const int64_t *v1;
    const int64_t *index;    /* may be NULL: rows are then their own index */
    /* :txn values (LC_F_TXN rows; ABI 8).  Row r's micro-ops are the triples
     * mop[3*i .. 3*i+2] for i in [mop_off[r], mop_off[r + 1]); a row with an
     * empty range has a nil :value.  Both may be NULL when no row is a :txn. */
    const int64_t *mop_off;  /* [n + 1] or NULL */
    const int64_t *mop;      /* [3 * mop_off[n]] (f, register, value)       */
} lc_history;

/* ---- packed per-key event streams (rows A3-A5) ---------------------------- */
/*
 * Event word (u32), one per surviving client event of a key sub-history:
 *   bit 31      0 = :invoke, 1 = :ok completion
 *   bits 30..24 slot: the op's position in the key's pending window
 *               (lowest free slot at invoke, freed at :ok; crashed ops keep
 *               theirs forever)
 *   bits 23..0  invoke: transition id (index into trans[] after adding
 *               trans_off[key]); ok: 0
 * Failed ops (:fail) are gone (knossos.history/without-failures); :info
 * completions produce no event (the op stays callable forever).
 */
#define LC_EV_OK_BIT     0x80000000u
#define LC_EV_SLOT(e)    (((e) >> 24) & 0x7Fu)
#define LC_EV_TRANS(e)   ((e) & 0x00FFFFFFu)

/*
 * Transition descriptor (u32) = one interned cas-register op
 * (knossos.model/cas-register step, knossos.model.memo):
 *   bits 1..0   LC_T_READ_ANY (read of nil: legal in every state, no change)
 *               LC_T_READ  (legal iff state == a, no change)
 *               LC_T_WRITE (state := b)
 *               LC_T_CAS   (legal iff state == a, then state := b)
 *   bits 16..2  a (state id; LC_STATE_NONE = a value no op can produce)
 *   bits 31..17 b (state id)
 * State 0 is nil, the register's initial value ((model/cas-register) at
 * etcdemo.clj:117).
 */
#define LC_T_READ_ANY 0u
#define LC_T_READ     1u
#define LC_T_WRITE    2u
#define LC_T_CAS      3u
#define LC_STATE_NONE 0x7FFFu
#define LC_DESC(f, a, b) ((uint32_t)(f) | ((uint32_t)(a) << 2) | ((uint32_t)(b) << 17))

/* Table models ((model/multi-register), whose state is a map of registers):
 * lc_batch.table holds, per key, one row of key_states[key] u16 entries per
 * distinct op -- the next state id from each state, LC_TABLE_NONE when the
 * step is inconsistent -- and the op's descriptor trans[] entry is the offset
 * of its row in table[] (knossos.model.memo's state x transition table).
 * Such a batch needs trans_off and key_states. */
#define LC_TABLE_NONE 0xFFFFu

/* Limits of the packed form.  A key beyond them is reported :unknown with
 * cause LC_CAUSE_WINDOW / LC_CAUSE_STATES (identically in oracle/).  With
 * per-key tables (trans_off and key_states) a key whose key_states exceeds
 * LC_WIDE_MAX_STATES is never stepped, and its descriptors may install
 * LC_STATE_NONE (lc_pack numbers the surplus values so); the other keys of
 * the batch are searched as usual. */
#define LC_NARROW_MAX_SLOTS  56   /* u64 config: 8-bit state | 56 slot bits   */
#define LC_NARROW_MAX_STATES 255
#define LC_WIDE_MAX_SLOTS    112  /* 2 x u64 config                          */
#define LC_WIDE_MAX_STATES   32767

/* A packed batch: caller-visible view of lc_pack output or caller-built. */
typedef struct lc_batch {
    int64_t         n_keys;
    const uint64_t *ev_off;     /* [n_keys + 1] offsets into events          */
    const uint32_t *events;     /* [ev_off[n_keys]]                           */
    const uint32_t *trans;      /* transition descriptors                     */
    int64_t         n_trans;
    const uint32_t *trans_off;  /* [n_keys] per-key base into trans, or NULL  */
    const uint8_t  *key_width;  /* [n_keys] max slots used (1 + max slot), or NULL */
    const uint16_t *key_states; /* [n_keys] state ids used, or NULL           */
    uint32_t        init_state; /* state id of the initial value (0 = nil)    */
    const uint8_t  *key_error;  /* [n_keys] nonzero: the key's sub-history could
                                   not be prepared (lc_pack: knossos.history/
                                   complete's assertion, an op the model cannot
                                   step); the key is :unknown with cause
                                   LC_CAUSE_ERROR and its events are ignored --
                                   jepsen.checker/check-safe around that one key
                                   (etcdemo.clj:115).  NULL = no such key.       */
    const uint16_t *table;      /* [n_table] transition table of a table model
                                   (LC_TABLE_NONE above), or NULL: trans[] are
                                   LC_DESC descriptors (ABI 8)                 */
    int64_t         n_table;
    const uint16_t *events16;   /* [ev_off[n_keys]] or NULL: the same event
                                   words in 16 bits (LC_EV16_* below), given
                                   when every word fits; a register-tier batch
                                   then crosses the host link at 2 bytes per
                                   event and is widened on the device (ABI 8) */
} lc_batch;

/* 16-bit event word: bit 15 :ok, bits 14..11 slot (< 16), bits 10..0
 * transition id (< 2048).  Widened: LC_EV16_WIDE(e). */
#define LC_EV16_MAX_SLOT  15u
#define LC_EV16_MAX_TRANS 2047u
#define LC_EV16_WIDE(e) ((((uint32_t)(e) & 0x8000u) << 16) | ((((uint32_t)(e) >> 11) & 0xFu) << 24) | \
                         ((uint32_t)(e) & 0x7FFu))

/* The Knossos model a batch is checked against (knossos.model, SURVEY.md
 * 8(f) F-4).  The demo uses (model/cas-register) at etcdemo.clj:117; the
 * other two map onto the same transition descriptors:
 *   register     read / write of integer values (no cas)
 *   mutex        two states, unlocked (state 0, the initial one) and locked:
 *                :acquire = cas unlocked -> locked, :release = cas locked ->
 *                unlocked; :value is ignored                            */
#define LC_MODEL_CAS_REGISTER 0
#define LC_MODEL_REGISTER     1
#define LC_MODEL_MUTEX        2
/*   multi-register  knossos.model/multi-register: a map of registers, one
 *                :f :txn whose :value is a sequence of [:read k v] /
 *                [:write k v] micro-ops applied in order (a read of v legal
 *                iff v is nil or register k holds v).  States are the maps
 *                reachable from the initial one (memo), numbered per key; ops
 *                become rows of lc_batch.table.  A key with more than
 *                LC_WIDE_MAX_STATES reachable maps is :unknown (cause
 *                states).  An :ok completion's micro-ops replace the
 *                invocation's (a read learns what it read).             */
#define LC_MODEL_MULTI_REGISTER 3

typedef struct lc_pack_opts {
    int32_t model;     /* LC_MODEL_* (0 = cas-register) */
    int32_t n_init;    /* multi-register: initial registers, pairs        */
    const int64_t *init;  /* [2 * n_init] (register, value); others absent */
    uint32_t flags;    /* LC_PACK_* (ABI 11); 0 = the library's choice     */
} lc_pack_opts;

/* lc_pack_opts.flags: path pins for A/B runs and tests; the packed batch is
 * byte-identical whichever path builds it. */
#define LC_PACK_GENERAL 0x1u  /* always the bucketing path (rows of a key
                                 gathered through a row list), never the
                                 key-major one (each key's rows one run)   */

typedef struct lc_packed lc_packed;  /* library-owned */

/* jepsen.independent/checker's split (history-keys + subhistory, per
 * etcdemo.clj:115) followed by knossos.history/complete + without-failures
 * and model memoisation, for the cas-register model.  Keys appear in order
 * of first appearance.  Non-tuple ops belong to every key's sub-history
 * (jepsen.independent/subhistory keeps them): the nemesis's :info ops are
 * no-ops there, and any other op is paired and stepped in every key.
 *
 * Errors are per key, as independent/checker runs check-safe per key: a key
 * whose sub-history fails complete's assertion (a completion with no
 * outstanding invocation of its process) or holds an op the model cannot
 * step keeps its place with no events and key_error set (lc_batch), and the
 * other keys are packed as usual; lc_packed_key_error names the cause.
 * Only malformed arrays (bad :type / :f codes, missing pointers) fail the
 * whole call. */
int  lc_pack(const lc_history *h, const lc_pack_opts *opts, lc_packed **out);
void lc_packed_free(lc_packed *p);
/* Borrowed view of the packed arrays (valid until lc_packed_free). */
int  lc_packed_view(const lc_packed *p, lc_batch *out);
/* Independent key of packed key i. */
int64_t lc_packed_key(const lc_packed *p, int64_t i);
/* History row (0-based position in the lc_history) of event j of key i. */
int64_t lc_packed_event_row(const lc_packed *p, int64_t i, int64_t j);
/* Which lc_pack path built p (diagnostics, ABI 11): 1 = key-major (every
 * key's rows one run of the history), 0 = bucketing. */
int lc_packed_path(const lc_packed *p);
/* The history row of every event, in event order (ev_off's numbering);
 * out may be NULL to query the count (ABI 11). */
int64_t lc_packed_event_rows(const lc_packed *p, int64_t *out);
/* Number of history rows in key i's sub-history (incl. nemesis rows) and the
 * rows themselves (out may be NULL to query the count). */
int64_t lc_packed_subhistory(const lc_packed *p, int64_t i, int64_t *out_rows);
/* Why key i could not be prepared (NULL when it was; borrowed, valid until
 * lc_packed_free). */
const char *lc_packed_key_error(const lc_packed *p, int64_t i);
/* Register value of state id s of key i (state 0 = nil -> *is_nil = 1). */
int lc_packed_state_value(const lc_packed *p, int64_t i, uint32_t s, int64_t *value, int *is_nil);
/* Every key at once (n_keys entries), in packed order. */
int lc_packed_keys(const lc_packed *p, int64_t *out);
/* multi-register: the map state id s of key i stands for, as (register,
 * value) pairs in register order (a register the map lacks is absent; a
 * present nil is LC_NIL).  Writes at most cap pairs; returns how many the
 * state has. */
int64_t lc_packed_state_map(const lc_packed *p, int64_t i, uint32_t s, int64_t *regs, int64_t *vals, int64_t cap);

/* ---- Knossos-shaped result of one key -------- */
/* jepsen.checker/linearizable's result map (etcdemo.clj:117-118) for packed
 * key i, from its verdict record (valid, fail_event) and the final configs
 * the device returned for it (lc_result.final_configs + i * max_final * 2,
 * n_final[i]).  Ops are named by history rows (positions in the lc_history
 * given to lc_pack); an op is (invoke row, completion row or -1), from which
 * a binding builds the op map knossos.history/complete would (the
 * invocation, taking the completion's :value when it has none).  Model
 * states are register values (LC_NIL for nil; multi-register: state ids, see
 * lc_packed_state_map).  Writes int64 words:
 *   [0] :op row (the :ok that could not be linearized) or -1
 *   [1] :previous-ok row (= :last-op: the last :ok before it) or -1
 *   [2] n_configs (<= max_paths)   [3] n_paths (<= max_paths)
 *   per config: state, n_pending, n_pending x op, n_linearized, n_linearized x op
 *   per path:   start state (the :previous-ok step's model), n_steps,
 *               n_steps x (op, state after it), and the state in which the
 *               failing op is inconsistent (its "can't ..." message)
 * Paths (invalid keys only): from each final config, every sequence of
 * further pending ops the model allows, then the failing op; depth-first,
 * shortest first, in device config order, at most max_paths distinct ones
 * (Knossos iterates a hash set there: only the SET is comparable).  Returns
 * the number of words; nothing is written when that exceeds cap (call again
 * with a larger buffer). */
int64_t lc_report(const lc_packed *p, int64_t i, int32_t valid, int32_t fail_event, const uint64_t *final_configs,
                  uint32_t n_final, int32_t max_paths, int64_t *out, int64_t cap);
/* The same key shaped as knossos.wgl's analysis (:algorithm :wgl,
 * etcdemo.clj:118 slot; ABI 9; parity unpinned, restated in oracle/wgl_ref.py):
 * the same words, with :configs = the Wing-Gong search's frontier at the
 * return entry it is stuck on (the failing :ok) -- every (state, linearized
 * pending ops) reachable from the given final configs by linearizing further
 * pending ops other than the failing one, breadth first, at most max_paths. */
int64_t lc_report_wgl(const lc_packed *p, int64_t i, int32_t valid, int32_t fail_event,
                      const uint64_t *final_configs, uint32_t n_final, int32_t max_paths, int64_t *out, int64_t cap);

/* ---- device checking (rows A6-A9) ------------------------------------------ */
#define LC_ALGO_LINEAR      0  /* :algorithm :linear (etcdemo.clj:118)              */
#define LC_ALGO_WGL         1  /* :algorithm :wgl              */
#define LC_ALGO_COMPETITION 2  /* jepsen.checker/linearizable's default             */
/* LC_ALGO_LINEAR: knossos.linear's config-set search (the tiers T0-T3).
 * LC_ALGO_WGL (ABI 10): knossos.wgl's own search on the device -- the Wing &
 * Gong depth-first walk with Lowe's cache of (linearized set, state) pairs,
 * one wavefront per key; max_configs bounds the cache (more pairs: :unknown,
 * cause budget), so a key the :linear budget gives up on may still be decided
 * (and the other way round).  final_configs of an invalid key are the WGL
 * frontier at the return entry the walk is stuck on (the first max_final the
 * walk reaches), shaped by lc_report_wgl.  Restated in oracle/wgl_ref.py and
 * oracle/wgl_ref.c; parity with Knossos unpinned.
 * LC_ALGO_COMPETITION (knossos.competition races the two and takes the first
 * answer): the :linear search, then WGL for the keys :linear left :unknown at
 * its budget; lc_result.analyzer names the analysis each key's answer came
 * from. */

#define LC_MAX_DEVICES   8    /* devices one context drives (one node)        */
#define LC_COMM_ID_BYTES 128  /* an RCCL unique id (ncclUniqueId)             */

typedef struct lc_opts {
    int32_t  device;        /* HIP device ordinal (n_devices <= 1)              */
    int32_t  algorithm;     /* LC_ALGO_*                                        */
    uint64_t max_configs;   /* search budget B (0 = default 1<<20): a key whose
                               config set or JIT closure exceeds B configs is
                               :unknown (LC_CAUSE_BUDGET); replaces
                               knossos.search's heap-dependent abort (row A7)   */
    int32_t  max_final;     /* configs kept per invalid key (<= 16, default 10,
                               the truncation of jepsen.checker/linearizable)   */
    int32_t  lds_configs;   /* per-wave LDS frontier capacity (0 = default)     */
    int32_t  deep_slots;    /* concurrently searched HBM-tier keys (0 = auto)    */
    int32_t  flags;         /* LC_OPT_*                                          */
    int32_t  debug_mode;    /* 0 (ablation builds only)                          */
    /* One process, several GPUs (independent/checker's pmap over the node's
     * devices): n_devices in 2..LC_MAX_DEVICES checks every
     * batch as contiguous key shards of about equal event counts, one per
     * devices[g] (a device may repeat: shards then share it), all at once.
     * 0 or 1: `device` alone. */
    int32_t  n_devices;
    int32_t  devices[LC_MAX_DEVICES];
    /* One process per GPU (the launcher's ranks): comm_size > 1 makes this
     * context rank comm_rank of an RCCL communicator over comm_size ranks,
     * created here (ncclCommInitRank; it waits for every rank) from comm_id,
     * which rank 0 takes from lc_comm_id and hands to every rank (comm_size
     * 1 with a nonzero comm_id: a one-rank communicator).  lc_check_node
     * all-gathers the verdict records over it. */
    int32_t  comm_rank;
    int32_t  comm_size;
    uint8_t  comm_id[LC_COMM_ID_BYTES];
    /* Search-path choices (ABI 9, in the bytes ABI 8 reserved; all 0 =
     * automatic, the library's own choice per batch).  They pin one choice for
     * A/B measurements and tests, never change a result, and are read at
     * lc_create only: the caller's environment does not steer the kernels. */
    int32_t  path_flags;    /* LC_PATH_*                                         */
    int32_t  spec_segs;     /* speculative segments per key: 2, 3, 4, 6 or 8      */
    int32_t  spec_ck;       /* speculative checkpoints, events past a cut:
                               (ck1 + 1) | (ck2 + 1) << 16 (0: 32 and 120)      */
    int32_t  seg_len;       /* quiescent-point segments: events per segment      */
} lc_opts;

/* lc_opts.path_flags */
#define LC_PATH_SPLIT_ON     0x01  /* quiescent-point key segments where they apply  */
#define LC_PATH_SPLIT_OFF    0x02  /* never (else: when sampled keys say they pay)    */
#define LC_PATH_SPEC_OFF     0x04  /* no speculative key segments                     */
#define LC_PATH_LAYERS_OFF   0x08  /* HBM tier: config-keyed sets only (no T3L)       */
#define LC_PATH_NODE_SYNC    0x10  /* lc_check_node_async runs as lc_check_node        */
#define LC_PATH_NODE_STAGED  0x20  /* one rank: records through HBM, not device-mapped */
#define LC_PATH_CHUNKS_ON    0x40  /* lc_check_node: chunked upload whatever the size  */
#define LC_PATH_CHUNKS_OFF   0x80  /* lc_check_node: one upload whatever the size      */
#define LC_PATH_SPEC_COST    0x100 /* speculative cuts at equal estimated cost
                                      instead of equal event counts                 */
#define LC_PATH_EV32         0x200 /* upload 32-bit event words even when 16-bit ones
                                      are given (lc_batch.events16)                 */
#define LC_PATH_SPEC_NOPRIO  0x400 /* speculative walks: issue priority by wave age
                                      alone, not by progress                        */
#define LC_PATH_WGL_SMALL    0x800 /* WGL: Lowe's caches start in 2^14-entry tables
                                      (keys outgrowing them are searched again with a
                                      table the budget fits)                        */
#define LC_PATH_SPEC_NOSTAGE 0x1000 /* speculative segments: event words read from HBM
                                      by every run, not staged in LDS once per key  */
#define LC_PATH_WGL_EV_HBM   0x2000 /* WGL: every key's events read from HBM, none
                                       staged in LDS (tests of that walk; ABI 11)   */
#define LC_PATH_SET_HBM      0x4000 /* lc_set_check: every key with elements through the
                                       HBM tier, none through the LDS tier (tests of
                                       those kernels; ABI 12)                        */
#define LC_PATH_SET_DIRECT   0x8000 /* lc_set_check, HBM tier: k_set_mark's bits leave by
                                       atomics from the lanes, never through a
                                       workgroup's LDS tile (A/B runs and tests)      */
#define LC_PATH_NODE_SERIAL  0x10000 /* lc_check_node_async: every step's search on one
                                        stream, in turn (else consecutive register-tier
                                        steps search on two streams and overlap; A/B runs
                                        and tests -- the records are the same either way) */
#define LC_PATH_ALL          0x1FFFF

/* lc_opts.flags */
#define LC_OPT_COUNT_PROBES 0x1  /* count successor-config probes (lc_stats.probes,
                                    SURVEY.md 8(d) D-4); off, the register-lattice
                                    tier skips the per-event popcounts          */

/* :valid? per key */
#define LC_VALID    1
#define LC_INVALID  0
#define LC_UNKNOWN -1

/* why a key ended */
#define LC_CAUSE_NONE    0  /* valid                                         */
#define LC_CAUSE_NONLIN  1  /* invalid: config set empty at fail_event       */
#define LC_CAUSE_BUDGET  2  /* unknown: > max_configs configs                 */
#define LC_CAUSE_WINDOW  3  /* unknown: > LC_WIDE_MAX_SLOTS ops pending       */
#define LC_CAUSE_STATES  4  /* unknown: > LC_WIDE_MAX_STATES register values  */
#define LC_CAUSE_ERROR   5  /* unknown: the key's sub-history could not be
                                   prepared (lc_batch.key_error; check-safe)   */

typedef struct lc_result {
    int8_t   *valid;         /* [n_keys] LC_VALID / LC_INVALID / LC_UNKNOWN         */
    int32_t  *fail_event;    /* [n_keys] event ordinal (within the key's stream) of
                                the :ok that could not be linearized, else -1       */
    uint8_t  *cause;         /* [n_keys] LC_CAUSE_*                                  */
    uint32_t *peak_configs;  /* [n_keys] max config-set size seen (may be NULL); a
                                key WGL answered: its cache size at the end       */
    uint64_t *final_configs; /* [n_keys * max_final * 2] (may be NULL): for invalid
                                keys, up to max_final configs of the last non-empty
                                set, as {state, slot mask lo} / {slot mask hi}      */
    uint32_t *n_final;       /* [n_keys] configs written to final_configs (may be NULL) */
    uint8_t  *analyzer;      /* [n_keys] LC_ALGO_LINEAR / LC_ALGO_WGL: the analysis
                                whose answer the key carries (may be NULL; ABI 10) */
} lc_result;

typedef struct lc_stats {
    double   kernel_ms;       /* device time of the search kernels (HIP events) */
    double   total_ms;        /* wall time of the call                          */
    uint64_t probes;          /* successor-config insert attempts (all tiers);
                                 0 unless lc_opts.flags has LC_OPT_COUNT_PROBES */
    uint64_t lds_keys;        /* keys finished in the LDS tier                  */
    uint64_t deep_keys;       /* keys (re)searched in the HBM tier              */
    uint64_t events;          /* events processed (0, like lds_keys, when the
                                 step was T0 alone: no counter readback)     */
    double   tier0_ms;        /* device time of the register-lattice tier alone */
    double   tier3_ms;        /* device time of the HBM tier launches (0 if none) */
    uint64_t probes_t3;       /* the part of `probes` made by the HBM tier      */
    uint64_t t3_bytes;        /* algorithmic HBM bytes of the layered HBM tier:
                                 8 per config-set entry it streams in or out
                                 (ABI 7)                                       */
    uint32_t t0_path;         /* the register tier's kernel this step (ABI 9):
                                 LC_T0_PATH_*                                   */
    uint32_t ev_word_bytes;   /* bytes per event word it read: 2 (lc_batch.events16
                                 read in place) or 4                            */
    double   wgl_ms;          /* device time of the WGL launches (ABI 10)       */
    uint64_t wgl_keys;        /* keys the WGL search answered                   */
    uint64_t wgl_spilled;     /* of those, keys searched again with a table the
                                 budget fits (they outgrew the shared tables)   */
    uint64_t wgl_steps;       /* WGL walk steps (linearizations + backtracks)   */
} lc_stats;

/* lc_stats.t0_path */
#define LC_T0_PATH_NONE      0  /* no register-tier launch (table model, no keys) */
#define LC_T0_PATH_LATTICE   1  /* k_search_lattice: one wave per key            */
#define LC_T0_PATH_SPEC      2  /* k_spec: speculative key segments              */
#define LC_T0_PATH_SEGMENTS  3  /* k_search_segments: quiescent-point segments    */

typedef struct lc_ctx lc_ctx;
typedef struct lc_dev_batch lc_dev_batch;

int         lc_abi_version(void);
const char *lc_last_error(void);
int         lc_device_count(void);
/* Give back the host blocks the library keeps for reuse (page-locked and
 * heap; up to 1 GB each, held after their arrays are freed).  Also done when
 * the last context is destroyed.  Arrays still in use are not touched. */
void        lc_trim(void);

int  lc_create(const lc_opts *opts, lc_ctx **out);
void lc_destroy(lc_ctx *ctx);

/* One call per batch: H2D, search, D2H into caller-owned result arrays.
 * Validation: every array index is checked before a kernel follows it.  The
 * per-event checks (an :ok names a pending slot, transition ids in range,
 * key_width / key_states honest) run on the device, one wave per key beside
 * the register tier (which stays in bounds on any input, and for a batch
 * declared to fit it refuses a key that does not); the set tiers that follow
 * trust the events, so over a refused batch they do nothing, and a malformed
 * key ends the call with LC_E_INVALID naming it.  A table model's batch
 * (lc_batch.table) is checked on the host, rows included.
 * The result arrays of a refused call are unspecified.  Event words in
 * page-locked memory (lc_pack's output on a GPU host) are uploaded directly;
 * others through a pinned staging copy. */
int  lc_check_batch(lc_ctx *ctx, const lc_batch *b, lc_result *r, lc_stats *s);

/* Device-resident batches: upload once, check many times (the bench's step). */
int  lc_upload(lc_ctx *ctx, const lc_batch *b, lc_dev_batch **out);
void lc_dev_batch_free(lc_dev_batch *db);
/* Search an uploaded batch.  flags:
 *   LC_DEV_RESULT  the result arrays in r are DEVICE pointers (e.g. torch
 *                  tensors for an RCCL all-gather) and nothing is copied back;
 *                  without it they are host arrays.
 *   LC_DEV_ASYNC   (with LC_DEV_RESULT) when the step is the register tier
 *                  alone (every key fits it, no probe counting), return once it
 *                  is enqueued on the context's stream: s is zeroed, and results
 *                  are ready after lc_wait.  Other steps run synchronously. */
#define LC_DEV_RESULT 1
#define LC_DEV_ASYNC  2
int  lc_check_device(lc_ctx *ctx, const lc_dev_batch *db, lc_result *r,
                     int flags, lc_stats *s);
/* Wait for every step enqueued on the context, on both of its search
 * streams.  Returns the number of LC_DEV_ASYNC steps since the previous
 * lc_wait (or a negative LC_E_* code); s->kernel_ms = their span (HIP events,
 * first start .. last end on either stream) and s->tier0_ms = span / count
 * (overlapping steps: less than one step's search). */
int  lc_wait(lc_ctx *ctx, lc_stats *s);
/* Wait until the LC_DEV_ASYNC step `back` steps before the latest (0 = the
 * latest, at most 3) has finished, leaving later ones running; steps count in
 * the order they were enqueued, whichever stream searched them.  With no such
 * step on record, wait for everything enqueued on the context.  Returns
 * LC_E_INVALID, naming the key, when a finished step's batch was malformed
 * (an error a later, still running step has raised already may be reported
 * here too); the error is cleared then. */
int  lc_wait_step(lc_ctx *ctx, int back);

/* ---- one process per GPU: node-wide verdict records ------- */
/* A key's verdict record: (valid + 1) | cause << 8 | (fail_event + 1) << 16
 * (8 bytes; 0 = padding).  Each rank checks its shard of the keys and the
 * records of every rank are all-gathered over RCCL (xGMI) -- the one
 * exchange step of the path; the shards share no state. */
#define LC_REC_VALID(r)      ((int)((r) & 0xFFu) - 1)
#define LC_REC_CAUSE(r)      ((int)(((r) >> 8) & 0xFFu))
#define LC_REC_FAIL_EVENT(r) ((int32_t)((int64_t)((r) >> 16) - 1))

/* A fresh RCCL unique id (LC_COMM_ID_BYTES) for lc_opts.comm_id; rank 0
 * calls it and the launcher distributes the bytes. */
int  lc_comm_id(uint8_t *out);
/* This rank's shard, from host SoA: upload, search, pack the shard's
 * records into a block of `block` (>= shard keys; padded with 0), all-gather
 * the blocks of every rank (comm_size of them, rank order), and copy the
 * node's block * comm_size records to `node` (host).  One rank: node = the
 * shard's block. */
int  lc_check_node(lc_ctx *ctx, const lc_batch *shard, int64_t block, uint64_t *node, lc_stats *s);
/* Pipelined lc_check_node.  A step that is the register tier alone
 * (every key fits it, no probe counting, node page-locked: lc_host_alloc)
 * is only enqueued and returns 1: up to three steps are in flight, one
 * uploading and -- without a communicator -- two searching at once on two
 * streams (a step's workgroups take the slots the previous step's finished
 * blocks free; LC_PATH_NODE_SERIAL keeps one search at a time, as a
 * communicator does).  Its records are in `node` once lc_wait (or
 * lc_wait_step over it) returns; errors surface there.  The shard's arrays
 * and `node` must stay untouched until then.  A buffer given to several
 * steps in flight holds, after that wait, the records of the latest step
 * enqueued with it: such a step's records leave through device memory, behind
 * the end of the earlier step.  One rank (no communicator): otherwise the
 * search writes the records straight into `node` (device-mapped); either way
 * lc_node_records has none of them.  Any other step runs as lc_check_node
 * (returns 0). */
int  lc_check_node_async(lc_ctx *ctx, const lc_batch *shard, int64_t block, uint64_t *node, lc_stats *s);
/* Page-locked host memory (for lc_check_node_async's records). */
void *lc_host_alloc(size_t bytes);
void  lc_host_free(void *p);
/* The same from a resident shard (lc_upload), records left in HBM until
 * lc_node_records; flags LC_DEV_ASYNC: a step that is the register tier
 * alone is only enqueued (lc_wait ends the run). */
int  lc_check_node_device(lc_ctx *ctx, const lc_dev_batch *shard, int64_t block, int flags, lc_stats *s);
/* The first n records of the last gather (waits for it). */
int  lc_node_records(lc_ctx *ctx, uint64_t *node, int64_t n);

/* ---- synthetic histories ------------------------------ */
typedef struct lc_synth_opts {
    int64_t  n_keys;
    int64_t  ops_per_key;    /* client invocations per key (gen/limit, :125)     */
    int32_t  concurrency;    /* client threads per key (concurrent-generator 10) */
    int32_t  n_values;       /* values 0..n_values-1 (rand-int 5, :68-69)         */
    double   info_rate;      /* fraction of write/cas that complete :info         */
    double   info_effect_p;  /* probability a crashed op took effect              */
    double   anomaly_rate;   /* fraction of keys given one stale read / lost cas  */
    double   mean_think;     /* mean think time between a thread's ops            */
    double   mean_latency;   /* mean op latency                                   */
    int32_t  interleave;     /* 1: one time-ordered Jepsen history (keys in
                                sequence per thread group, tuples, :index);
                                0: key-major blocks                               */
    double   nemesis_period; /* > 0 and interleave: nemesis :info :start/:stop
                                every period (etcdemo.clj:138-143)                */
    uint64_t seed;
    int64_t  key_base;       /* first key id (shards of a larger key space)       */
} lc_synth_opts;

typedef struct lc_hist lc_hist;      /* library-owned history storage */
int  lc_synth_generate(const lc_synth_opts *o, lc_hist **out);
int  lc_hist_view(const lc_hist *h, lc_history *out);  /* borrowed view */
/* Keys the generator corrupted (anomaly_rate), ascending; out may be NULL to
 * query the count. */
int64_t lc_hist_anomalous_keys(const lc_hist *h, int64_t *out_keys);
void lc_hist_free(lc_hist *h);
/* Named registers of a history read by lc_edn_read: their count, and the
 * i-th name as written in the file (e.g. ":x"), or NULL past the end. */
int64_t     lc_hist_n_reg_names(const lc_hist *h);
const char *lc_hist_reg_name(const lc_hist *h, int64_t i);

/* ---- history.edn (Jepsen store format) ------------------------------------- */
/* Parse a Jepsen history.edn (one op map per line, or one vector of maps)
 * into an owned history.  Supports the op maps this workload produces:
 * :type :f :process :value (nil, ints, [k v] tuples, [old new]) :index :time
 * :error; other keys are skipped.  (model/multi-register) :f :txn values
 * [[:read k v] [:write k v] ...] (also :r / :w), optionally as [key txn]
 * tuples, fill lc_history.mop_off / mop: integer registers keep their ids,
 * other register names get LC_NAMED_REG_BASE + i.  lc_edn_write writes
 * :txn rows back, named registers as :r<i> keywords (lc_edn_write_named: by
 * their names). */
int  lc_edn_read(const char *path, lc_hist **out);
int  lc_edn_parse(const char *text, int64_t len, lc_hist **out);
int  lc_edn_write(const char *path, const lc_history *h);
/* lc_edn_write with named registers written back under their names:
 * reg_names[i] names register LC_NAMED_REG_BASE + i as lc_hist_reg_name gives
 * it (":x"); a name that is not one EDN token is written as :r<i>.  (ABI 9) */
int  lc_edn_write_named(const char *path, const lc_history *h, const char *const *reg_names, int64_t n_reg_names);

/* ---- test.fressian (Jepsen store format, binary) ---------------------------- */
/* Read the history out of a Fressian-encoded Jepsen test map (its :history
 * entry) or a Fressian list of op maps, with the op rules of lc_edn_read.
 * The decoder covers the whole Fressian encoding (caches, struct types,
 * chunked strings, open lists); tagged values of unknown handlers are kept
 * as their fields.  lc_fressian_write emits {:name "lincheck" :history [...]}.
 * Replaces the :history of jepsen.store's test.fressian load (SURVEY.md 8(f)
 * F-1); parity unpinned, no stored run or Fressian library to check against. */
int  lc_fressian_read(const char *path, lc_hist **out);
int  lc_fressian_parse(const uint8_t *buf, int64_t len, lc_hist **out);
int  lc_fressian_write(const char *path, const lc_history *h);

/* ---- the set workload (set.clj:42-49, ABI 12) -------------------------------- */
/* The demo's second workload (etcdemo.clj:128-131, --workload set) is checked
 * with (checker/set) at set.clj:46: every :add that was acknowledged must be
 * in the final :read, and the read may hold only elements that were attempted.
 * Restated from the public Jepsen 0.2.x source of jepsen.checker/set and
 * jepsen.util/integer-interval-set-str (parity unpinned).
 * This path has its own structs and entry points; nothing above changes. */
/* :f of a set-workload op map */
#define LC_SF_ADD   0
#define LC_SF_READ  1
#define LC_SF_OTHER 2   /* nemesis rows and anything else: contributes nothing */

/*
 * A raw set-workload history as struct-of-arrays, one row per op map, in
 * history order.
 *   key        the k of an independent tuple [k v], or LC_NO_KEY; NULL = no row
 *              has one (the demo's single "a-set")
 *   elem       an :add row's element (LC_NIL: nil or not an integer); a :read
 *              row: LC_NIL when its :value is nil, else 0
 *   read_off   row r's read collection is read_elem[read_off[r] .. read_off[r+1])
 *              (empty for rows that are no :read; an element that is nil or
 *              not an integer is LC_NIL); both may be NULL when no row reads
 *   index      the op's :index; may be NULL
 */
typedef struct lc_set_history {
    int64_t        n;
    const uint8_t *type;      /* LC_INVOKE / LC_OK_T / LC_FAIL / LC_INFO */
    const uint8_t *f;         /* LC_SF_*                                  */
    const int64_t *key;
    const int64_t *elem;
    const int64_t *read_off;  /* [n + 1] */
    const int64_t *read_elem;
    const int64_t *index;
} lc_set_history;

/* class byte of an add id */
#define LC_SET_ATTEMPT 1  /* an :invoke :add */
#define LC_SET_ACK     2  /* an :ok :add     */
/* per-key status */
#define LC_SET_KEY_OK         0
#define LC_SET_KEY_NEVER_READ 1  /* no :ok :read, or the last one's value is nil:
                                    {:valid? :unknown :error "Set was never read"} */
#define LC_SET_KEY_ERROR      2  /* a nil or non-integer element (check-safe
                                    around that key): :unknown with an error     */

/*
 * A packed set batch: lc_set_pack's output or caller-built.  Key k's elements
 * are numbered by ids below span[k]:
 *   rank[k] == 0  offset ids: element = min[k] + id
 *   rank[k] == 1  rank ids:   element = vals[vals_off[k] + id], vals ascending
 *                 and distinct, vals_off[k + 1] - vals_off[k] >= span[k]
 * base[k] is the key's offset, in 64-bit words, into each of the three
 * bitmaps (attempted, acknowledged, read) of n_words words: even, ascending,
 * and base[k] + the key's words rounded up to even <= base[k + 1] (n_words for
 * the last key), so no run of set bits bridges two keys.  Keys whose status is
 * not LC_SET_KEY_OK have no rows (add_off / read_off ranges are ignored).
 * lc_set_check validates the offset arrays on the host; every id is checked
 * against span[k] on the device, and a bad one ends the call with
 * LC_E_INVALID naming the key.
 */
typedef struct lc_set_batch {
    int64_t         n_keys;
    const uint64_t *add_off;   /* [n_keys + 1] into add_id / add_cls           */
    const uint32_t *add_id;
    const uint8_t  *add_cls;   /* LC_SET_ATTEMPT / LC_SET_ACK                  */
    const uint64_t *read_off;  /* [n_keys + 1] into read_id (the final read)   */
    const uint32_t *read_id;
    const uint64_t *base;      /* [n_keys] */
    const uint32_t *span;      /* [n_keys] */
    const int64_t  *min;       /* [n_keys] */
    const uint8_t  *rank;      /* [n_keys] */
    const uint64_t *vals_off;  /* [n_keys + 1] */
    const int64_t  *vals;
    const uint8_t  *status;    /* [n_keys] LC_SET_KEY_*, or NULL: all OK       */
    uint64_t        n_words;   /* 64-bit words of one bitmap (even)            */
} lc_set_batch;

typedef struct lc_set_packed lc_set_packed;  /* library-owned */

/* independent/checker's split by key (keys in order of first appearance; one
 * key LC_NO_KEY when no row has one), then per key: the :invoke / :ok :add
 * rows, the last :ok :read, element minimum and maximum, the id form
 * (csrc/set_plan.hpp: plan_set_key) and the arrays above. */
int  lc_set_pack(const lc_set_history *h, lc_set_packed **out);
void lc_set_packed_free(lc_set_packed *p);
int  lc_set_packed_view(const lc_set_packed *p, lc_set_batch *out);
/* The independent key of every packed key (n_keys entries). */
int  lc_set_packed_keys(const lc_set_packed *p, int64_t *out);
/* Why key i is :unknown (NULL when it is not; borrowed). */
const char *lc_set_packed_key_error(const lc_set_packed *p, int64_t i);

/*
 * jepsen.checker/set's result per key, caller-allocated:
 *   counts   6 per key: attempt, acknowledged, ok, lost, recovered, unexpected
 *   runs     the maximal runs of consecutive integers of each key's :ok, :lost,
 *            :unexpected and :recovered sets (in that class order), as (first,
 *            last) element values, ascending; class c of key k owns runs
 *            run_off[4k + c] .. run_off[4k + c + 1)
 * run_cap is the capacity of runs in runs (pairs); n_runs comes back.  When
 * n_runs > run_cap the call returns LC_E_NOMEM, names the capacity needed in
 * lc_last_error, sets n_runs to it and writes no runs.
 */
typedef struct lc_set_result {
    int8_t   *valid;    /* [n_keys] LC_VALID / LC_INVALID / LC_UNKNOWN */
    uint64_t *counts;   /* [6 * n_keys]     */
    uint64_t *run_off;  /* [4 * n_keys + 1] */
    int64_t  *runs;     /* [2 * run_cap]    */
    uint64_t  run_cap;
    uint64_t  n_runs;
} lc_set_result;

/* A run capacity that always suffices: acknowledged adds plus twice the read
 * elements of the keys that are checked. */
int64_t lc_set_batch_max_runs(const lc_set_batch *b);
/* Check every key of the batch in one call on the context's stream (first
 * device of the context): H2D, kernels, D2H. */
int  lc_set_check(lc_ctx *ctx, const lc_set_batch *b, lc_set_result *r);
/* Device-event times of the last lc_set_check, ms: [0] upload, [1] kernels,
 * [2] download of the records, [3] the whole call (wall). */
int  lc_set_last_timing(lc_ctx *ctx, double *out_ms);
/* Launch constants of the set kernels (no device needed), in ids (bits):
 * [0] one lane's chunk of k_set_classify (a 16-byte load), [1] a wave's,
 * [2] a workgroup's, [3] the largest span the LDS tier takes, [4] the span up
 * to which a key keeps offset ids whatever its row count, [5] rows per
 * workgroup of k_set_mark, [6] the ids of its LDS tile. */
int  lc_set_launch_info(int64_t *out7);

/* history.edn of a set-workload run (:f :add with an integer :value, :f :read
 * with nil or a #{...} / [...] / (...) of integers, optionally as [k v]
 * tuples; every other op is LC_SF_OTHER with its value skipped).  A
 * single-threaded read with lc_edn_parse's allocation-free reader. */
typedef struct lc_set_hist lc_set_hist;  /* library-owned */
int  lc_edn_read_set(const char *path, lc_set_hist **out);
int  lc_edn_parse_set(const char *text, int64_t len, lc_set_hist **out);
int  lc_set_hist_view(const lc_set_hist *h, lc_set_history *out);
void lc_set_hist_free(lc_set_hist *h);

/* ---- checker/set-full (per-element set analysis; ABI 13, additive) ------------- */
/* (checker/set-full {:linearizable? ...}) examines EVERY :ok :read, not only
 * the last one, and classifies every element :stable, :lost or :never-read,
 * with stable / lost latencies and the stale elements.  Restated from memory
 * of the public Jepsen 0.2.x source of jepsen.checker/set-full; the rules
 * below are this library's definition (parity
 * unpinned).  Its own structs and entry points; nothing above changes.
 *
 * One key's (unwrapped) ops are folded in history order.  An op's POSITION is
 * its row number in the history; comparisons use positions.  Rows whose
 * :process is not an integer (LC_NO_PROCESS) are skipped.  State: elements
 * (element -> {known, last-present, last-absent}, all nil), reads (process ->
 * its open :read invocation), dups (element -> count).
 *   :invoke :add v   elements[v] = a FRESH record (a second invocation of the
 *                    same element discards what was known)
 *   :ok :add v       known = known or this op; :fail / :info adds change nothing
 *   :invoke :read    reads[p] = op; :fail :read removes reads[p]; :info: nothing
 *   :ok :read V by p (nil = the empty collection) with inv = reads[p]: every x
 *                    occurring c > 1 times in V sets dups[x] = max(dups[x], c)
 *                    (untracked elements too); for EVERY element tracked at
 *                    this moment: in V -> known = known or this op, and
 *                    last-present = inv if last-present is nil or older
 *                    (by position) than inv; else last-absent = inv likewise
 * Errors (that key {:valid? :unknown :error ...}): an :ok :add with no earlier
 * :invoke :add of its element; an :ok :read by a process with no open read; a
 * nil or non-integer element (of an :invoke / :ok :add or inside an :ok :read);
 * an :ok :read value that is neither nil nor a collection.
 * Per element, idx(x) = x's position or -1 for nil:
 *   stable?  last-present and idx(last-absent) < idx(last-present)
 *   lost?    known and last-absent and idx(last-present) < idx(last-absent)
 *            and idx(known) < idx(last-absent);       otherwise never-read
 *   stable-latency = max(0, (last-absent ? last-absent.time + 1 : 0) - known.time) / 10^6
 *   lost-latency   = max(0, (last-present ? last-present.time + 1 : 0) - known.time) / 10^6
 *   (integer nanoseconds in, integer division, milliseconds out)
 * :valid? by the first rule that fires: false if any element is lost; :unknown
 * if none is stable; false if linearizable and any stable element has a
 * stable-latency > 0 (is stale); else true -- and after that false if any
 * element was duplicated in one read. */

/* lc_set_history's columns plus :process and :time. */
typedef struct lc_setfull_history {
    int64_t        n;
    const uint8_t *type;      /* LC_INVOKE / LC_OK_T / LC_FAIL / LC_INFO */
    const uint8_t *f;         /* LC_SF_*                                  */
    const int64_t *key;       /* or NULL                                  */
    const int64_t *elem;
    const int64_t *read_off;  /* [n + 1], or NULL */
    const int64_t *read_elem;
    const int64_t *index;     /* or NULL */
    const int64_t *process;   /* LC_NO_PROCESS: not an integer (the row is skipped) */
    const int64_t *time;      /* :time, ns; NULL: all 0 */
} lc_setfull_history;

#define LC_SETFULL_NONE (-1)  /* no such op (a position) */
/* outcome of an id */
#define LC_SETFULL_UNTRACKED  0  /* an id nobody invoked (a hole of an offset key, or only ever read) */
#define LC_SETFULL_STABLE     1
#define LC_SETFULL_LOST       2
#define LC_SETFULL_NEVER_READ 3

/*
 * A packed set-full batch: lc_setfull_pack's output or caller-built.  Key k's
 * elements are numbered by ids below span[k] exactly as in lc_set_batch
 * (min / rank / vals_off / vals; csrc/set_plan.hpp: plan_set_key).  Every
 * value of any :ok :read has an id too, invoked or not, so that a duplicate of
 * an element nobody added is seen.  Key k's ids are id_off[k] .. id_off[k] +
 * span[k] of the per-id arrays; its :ok reads, IN COMPLETION ORDER (history
 * order, positions ascending), are rows row_off[k] .. row_off[k + 1]; row r's
 * ids are read_id[el_off[r] .. el_off[r + 1]).  Keys whose status is not
 * LC_SET_KEY_OK have no ids and no rows.  lc_setfull_check validates the
 * offsets and the rows' order on the host; every id is checked against
 * span[k] on the device, and a bad one ends the call with LC_E_INVALID naming
 * the key.
 */
typedef struct lc_setfull_batch {
    int64_t         n_keys;
    const uint64_t *id_off;    /* [n_keys + 1]: id_off[k + 1] - id_off[k] >= span[k] */
    const uint32_t *span;      /* [n_keys] */
    const int64_t  *min;       /* [n_keys] */
    const uint8_t  *rank;      /* [n_keys] */
    const uint64_t *vals_off;  /* [n_keys + 1] */
    const int64_t  *vals;
    const uint8_t  *status;    /* [n_keys] LC_SET_KEY_OK / LC_SET_KEY_ERROR, or NULL: all OK */
    /* per id */
    const int64_t  *inv_pos;   /* position of the last :invoke :add, or LC_SETFULL_NONE (untracked) */
    const int64_t  *ack_pos;   /* position of the first :ok :add after it, or LC_SETFULL_NONE */
    const int64_t  *ack_time;  /* that op's :time */
    /* per row (an :ok :read) */
    const uint64_t *row_off;   /* [n_keys + 1] */
    const int64_t  *row_pos;   /* the :ok's position: ascending inside a key */
    const int64_t  *row_time;
    const int64_t  *row_inv_pos;   /* its invocation's position (< row_pos) and :time */
    const int64_t  *row_inv_time;
    const uint64_t *el_off;    /* [rows + 1] into read_id, ascending from 0 */
    const uint32_t *read_id;
} lc_setfull_batch;

typedef struct lc_setfull_packed lc_setfull_packed;  /* library-owned */

/* independent/checker's split by key (keys in order of first appearance; one
 * key LC_NO_KEY when no row has one), reads paired with their invocations by
 * process, elements interned, the error rules applied per key. */
int  lc_setfull_pack(const lc_setfull_history *h, lc_setfull_packed **out);
void lc_setfull_packed_free(lc_setfull_packed *p);
int  lc_setfull_packed_view(const lc_setfull_packed *p, lc_setfull_batch *out);
int  lc_setfull_packed_keys(const lc_setfull_packed *p, int64_t *out);
/* Why key i is :unknown (NULL when it is checked; borrowed). */
const char *lc_setfull_packed_key_error(const lc_setfull_packed *p, int64_t i);

#define LC_SETFULL_MARK_DIRECT 0x1u  /* k_setfull_mark's bits leave by the lanes' own atomics, no LDS tile (A/B) */
typedef struct lc_setfull_opts {
    int32_t  linearizable;      /* {:linearizable? true}: a stale element makes the key invalid */
    uint32_t flags;             /* LC_SETFULL_* path flags (tests, A/B)                         */
    uint64_t max_matrix_bytes;  /* most bytes of presence matrix per pass; 0: the default
                                   (csrc/setfull_plan.hpp)                                      */
} lc_setfull_opts;

/*
 * Per key: valid and six counts -- attempt (tracked ids), stable, lost,
 * never-read, stale, duplicated.  Per id (the batch's id numbering, id_off[k]
 * + id): outcome, the latency in ms (stable-latency of a stable id,
 * lost-latency of a lost one, else -1), the positions of known and
 * last-absent (LC_SETFULL_NONE for nil), and whether some read held it twice.
 * Caller-allocated; n_ids = id_off[n_keys].
 */
typedef struct lc_setfull_result {
    int8_t   *valid;        /* [n_keys] LC_VALID / LC_INVALID / LC_UNKNOWN */
    uint64_t *counts;       /* [6 * n_keys] */
    uint8_t  *outcome;      /* [n_ids] LC_SETFULL_*  */
    int64_t  *latency;      /* [n_ids] */
    int64_t  *known;        /* [n_ids] */
    int64_t  *last_absent;  /* [n_ids] */
    uint8_t  *duplicated;   /* [n_ids] 0 / 1 */
} lc_setfull_result;

/* Check every key of the batch in one call on the context's stream (first
 * device of the context): H2D, per pass mark and scan, finish, D2H. */
int  lc_setfull_check(lc_ctx *ctx, const lc_setfull_batch *b, const lc_setfull_opts *o, lc_setfull_result *r);
/* Device-event times of the last lc_setfull_check, ms: [0] upload, [1] the
 * mark kernels (all passes), [2] the scan and finish kernels, [3] download,
 * [4] the whole call (wall), [5] the matrices' zeroing; then [6] passes and
 * [7] matrix bytes zeroed in all. */
int  lc_setfull_last_timing(lc_ctx *ctx, double *out8);
/* Launch constants (no device needed): [0] ids of one wave of k_setfull_scan,
 * [1] of one workgroup (bands are multiples of it), [2] read elements per
 * workgroup of k_setfull_mark, [3] per lane (16-byte loads of four),
 * [4] the ids of mark's LDS tile, [5] the default max_matrix_bytes. */
int  lc_setfull_launch_info(int64_t *out6);

/* history.edn of a set-workload run as lc_edn_read_set reads it (the same op
 * handler), keeping :process (LC_NO_PROCESS when not an integer) and :time
 * (0 when absent). */
typedef struct lc_setfull_hist lc_setfull_hist;  /* library-owned */
int  lc_edn_read_setfull(const char *path, lc_setfull_hist **out);
int  lc_edn_parse_setfull(const char *text, int64_t len, lc_setfull_hist **out);
int  lc_setfull_hist_view(const lc_setfull_hist *h, lc_setfull_history *out);
void lc_setfull_hist_free(lc_setfull_hist *h);

/* ---- streaming checker/set-full (ABI 13, additive) ------------------------------ */
/* Per-element verdicts while the set test runs: a stream that rows are appended
 * to, whose results after every append are those of the two calls above on
 * everything appended so far.  Its structs and entry points are this header's
 * next section, kept in a file of its own: include/lincheck_setfull_stream.h
 * (DESIGN.md section 3.13), exported by the same library. */

/* ---- checker/perf (etcdemo.clj:165-167, ABI 13) -------------------------------- */
/* The demo's check phase is (checker/compose {:perf (checker/perf) :indep ...}).
 * This path computes what jepsen.checker.perf computes before it draws: the
 * latency of every completed client op, latency quantiles per (:f, window)
 * and completion counts per (:f, :type, window).  Restated from the public
 * Jepsen 0.2.x source of jepsen.checker.perf and jepsen.util/history->latencies
 * (parity unpinned).  Its own structs and entry points;
 * nothing above changes. */
#define LC_PERF_MAX_F 32          /* distinct :f names in one history            */
#define LC_PERF_MAX_Q 8           /* quantiles in one call                       */
#define LC_PERF_NO_INVOKE INT64_MIN  /* t_inv of a completion without an invocation */
#define LC_PERF_META(f_inv, f_comp, type) ((uint32_t)(f_inv) | (uint32_t)(f_comp) << 8 | (uint32_t)(type) << 16)
/* lc_perf_opts.flags: path switches for tests and A/B runs */
#define LC_PERF_SELECT_HBM   0x1  /* every non-empty group through the HBM select */
#define LC_PERF_COUNT_DIRECT 0x2  /* k_perf_count / k_perf_scatter without their LDS
                                     tile: one global atomic per record            */

/*
 * A whole (unsplit) history as struct-of-arrays, one row per op map, in
 * history order.  Times need not be monotone.
 *   f        an id below n_f into a table of :f names the caller owns
 *   process  the client's integer :process, or LC_NO_PROCESS (:nemesis ...)
 *   time     the op's :time, integer nanoseconds
 *   f_start / f_stop  the ids of :start and :stop (nemesis intervals), or -1
 */
typedef struct lc_perf_history {
    int64_t        n;
    const uint8_t *type;     /* LC_INVOKE / LC_OK_T / LC_FAIL / LC_INFO */
    const uint8_t *f;
    const int64_t *process;
    const int64_t *time;
    int32_t        n_f;
    int32_t        f_start;
    int32_t        f_stop;
} lc_perf_history;

/*
 * lc_perf_pack's output, or caller-built: one record per client completion
 * (every client row that is no :invoke), in history order.
 *   meta    LC_PERF_META(f_inv, f_comp, type): the :f of the invocation the row
 *           completes (its own for an orphan), its own :f, its own :type
 *   t_comp  its own :time
 *   t_inv   the invocation's :time, or LC_PERF_NO_INVOKE for an orphan
 * t_min / t_max bound t_comp over all records, x_min / x_max bound t_inv over
 * the matched ones (ignored when there is none).  The device checks every
 * record against them before it addresses a table; a record outside ends the
 * call with LC_E_INVALID.
 */
typedef struct lc_perf_batch {
    int64_t         n;
    const int64_t  *t_comp;
    const int64_t  *t_inv;
    const uint32_t *meta;
    int64_t         n_matched;
    int64_t         t_min, t_max;
    int64_t         x_min, x_max;
    int32_t         n_f;
    int32_t         reserved;
} lc_perf_batch;

typedef struct lc_perf_packed lc_perf_packed;  /* library-owned */

/* Pairing, orphans and nemesis intervals in one O(n) pass over the rows.
 * More than LC_PERF_MAX_F names: LC_E_UNSUPPORTED.  A :type above LC_INFO or
 * an f at or above n_f: LC_E_INVALID. */
int  lc_perf_pack(const lc_perf_history *h, lc_perf_packed **out);
void lc_perf_packed_free(lc_perf_packed *p);
int  lc_perf_packed_view(const lc_perf_packed *p, lc_perf_batch *out);
/* out4: matched pairs, unmatched invocations, orphans, nemesis intervals. */
int  lc_perf_packed_info(const lc_perf_packed *p, int64_t *out4);
/* The nemesis intervals as (t0, t1) pairs: 2 * out4[3] values. */
int  lc_perf_packed_intervals(const lc_perf_packed *p, int64_t *out);

typedef struct lc_perf_opts {
    int64_t  quantile_dt_ns;       /* 30 s */
    int64_t  rate_dt_ns;           /* 10 s */
    int32_t  n_q;                  /* 1 .. LC_PERF_MAX_Q */
    uint32_t flags;                /* LC_PERF_* */
    double   q[LC_PERF_MAX_Q];     /* 0.5 0.95 0.99 1 */
} lc_perf_opts;
void lc_perf_opts_default(lc_perf_opts *o);

/*
 * The series, caller-allocated (lc_perf_shape gives the sizes):
 *   rate    [n_f][3][rate_n] completions of (:f, :ok / :fail / :info, bucket
 *           rate_first + i), by each row's own :f, :type and :time
 *   group   [n_f][q_n] latency points of (:f, bucket q_first + i)
 *   quant   [n_f][q_n][n_q] the latency at index
 *           min(n - 1, (long) floor((double) n * q)) of the group's points in
 *           ascending (invocation time, latency) order; meaningful where the
 *           group count is above 0
 * rate_cap / group_cap / quant_cap are the arrays' capacities in elements.
 */
typedef struct lc_perf_result {
    uint64_t *rate;
    uint64_t *group;
    int64_t  *quant;
    uint64_t  rate_cap, group_cap, quant_cap;
    int64_t   rate_first, rate_n;
    int64_t   q_first, q_n;
} lc_perf_result;

/* out4: rate_first, rate_n, q_first, q_n of a batch under opts (no device
 * needed); a width that is not positive: LC_E_INVALID. */
int  lc_perf_shape(const lc_perf_batch *b, const lc_perf_opts *o, int64_t *out4);
/* One call on the context's stream (first device): H2D, kernels, D2H. */
int  lc_perf_check(lc_ctx *ctx, const lc_perf_batch *b, const lc_perf_opts *o, lc_perf_result *r);
/* Device-event times of the last lc_perf_check, ms: [0] upload, [1] kernels,
 * [2] download, [3] the whole call (wall). */
int  lc_perf_last_timing(lc_ctx *ctx, double *out_ms);
/* Launch constants (no device needed): [0] records per workgroup of the
 * streaming kernels, [1] buckets the LDS histogram tile spans, [2] the largest
 * group the LDS select takes, [3] bits per digit of the HBM select. */
int  lc_perf_launch_info(int64_t *out4);

/* history.edn for perf: :type :f :process :time of every op map, every
 * :value skipped; :f names interned in order of first appearance.  A
 * single-threaded read with lc_edn_parse's allocation-free reader. */
typedef struct lc_perf_hist lc_perf_hist;  /* library-owned */
int  lc_edn_read_perf(const char *path, lc_perf_hist **out);
int  lc_edn_parse_perf(const char *text, int64_t len, lc_perf_hist **out);
int  lc_perf_hist_view(const lc_perf_hist *h, lc_perf_history *out);
/* Name i of the view's n_f names (borrowed; NULL out of range). */
const char *lc_perf_hist_name(const lc_perf_hist *h, int64_t i);
void lc_perf_hist_free(lc_perf_hist *h);

/* ---- incremental check: a resident search fed as the history grows ------------ */
/* A Jepsen run writes its history over minutes or hours.  A stream keeps every
 * key's register-tier search state on the device between calls, so each call
 * searches only what is new and a stale read is reported while the test still
 * runs.  Additive to ABI 13: own structs and entry
 * points, nothing above changes.
 *
 * Rows mode (lc_stream_append): the caller hands over history rows as they are
 * written.  knossos.history/complete makes an invocation's event depend on its
 * completion (a read learns its value from its :ok, a :fail removes the pair,
 * an :info or a later invoke of the same process leaves the op pending
 * forever), so per key the rows from the first invoke whose fate is still open
 * are held back; everything before it -- the key's DECIDED PREFIX -- is turned
 * into event words (the words lc_pack would give) and searched.  After any
 * call a key is invalid exactly when its decided prefix holds the :ok that
 * cannot be linearized; it stays invalid, with that event's ordinal.
 * lc_stream_finish decides every held row (ops still open are pending forever)
 * and after it every key's valid, cause and fail_event equal lc_pack +
 * lc_check_batch on the concatenated rows, whatever the split into calls.
 *   A completion with no open invocation, or an :invoke the model cannot step,
 * makes that key :unknown with LC_CAUSE_ERROR from then on (as lc_pack does
 * for the whole key) -- even if it was reported invalid earlier.  Rows with
 * neither a key nor an integer process (the nemesis) are skipped.  A keyless
 * row of an integer process, an LC_F_TXN row or a bad :type / :f code refuses
 * the whole call and leaves the stream as it was.
 *   The register tier holds 10 pending ops and 32 register states.  A key
 * whose next invoke would pass either is DEFERRED: from that event on its
 * words stay on the host, and lc_stream_finish checks the key once, from its
 * first event, through lc_check_batch with the context's budget.
 *   With LC_STREAM_SET_TIER (lc_stream_open_opts; rows mode only) such a key is
 * not restarted: it MIGRATES to a resident set tier on the device -- its
 * search state written out as a config set of at most 32,768 configs -- and
 * keeps being searched as rows arrive, so it too turns invalid in the call
 * whose decided prefix holds its failing :ok.  A migrated key FALLS BACK to
 * the deferral above when a set or a closure of it would pass 32,768 configs,
 * an invoke takes window slot 56 or above, or the key names more than 255
 * register values.  The guarantee after lc_stream_finish is unchanged: every
 * key's valid, cause and fail_event equal the one-shot check's.
 *
 * Events mode (lc_stream_push): the caller packs chunks itself.  Chunk key k
 * continues stream key key_ids[k] (new ids are new keys, in order of first
 * appearance); its words continue the key's earlier ones -- window slots and
 * state ids carry on across chunks, which is the caller's contract -- while
 * trans / trans_off / key_states / key_width (both required) are the chunk's
 * own.  The device validates the words; a key with malformed ones becomes
 * LC_CAUSE_ERROR and the call returns LC_E_INVALID naming it, the other keys
 * having advanced.  A chunk with a key_width above 10, a key_states above 32 or
 * a table is refused whole (LC_E_UNSUPPORTED).
 *
 * A stream is in one mode, fixed by its first call (mixing: LC_E_INVALID).  It
 * counts no probes and no peaks, and returns no final configs: to render the
 * counterexample of a key found invalid, run the ordinary checker on that
 * key's sub-history -- or open the stream with LC_STREAM_EXACT.
 *
 * Exact mode (LC_STREAM_EXACT in lc_stream_opts.flags; off by default, and
 * without it nothing of the above changes).  The register tier's resident
 * search then keeps Knossos's own config set per key, not a closed superset of
 * it, so for any split of the history into calls:
 *   - any lc_opts.max_configs is accepted.  A register-tier key becomes
 *     LC_UNKNOWN / LC_CAUSE_BUDGET in the call whose searched prefix holds the
 *     first event at which a set or a closure passes the budget; fail_event
 *     names that event, the key is searched no further, and it is NOT on
 *     lc_stream_update.invalid (lc_stream_results and lc_stream_key_tier --
 *     LC_STREAM_TIER_DEAD -- show it);
 *   - lc_stream_results also fills peak_configs, final_configs (max_final x 2
 *     words per key) and n_final where the caller passes them.  A key that died
 *     (invalid, or at the budget) has the set standing before the failing event
 *     and the peak up to it, the words lc_check_batch writes for it; a live key
 *     has its peak so far and n_final 0 until lc_stream_finish;
 *   - after lc_stream_finish every key's valid, cause, fail_event, peak,
 *     n_final and final_configs equal lc_pack + lc_check_batch on the
 *     concatenated rows with the same context -- valid keys' end sets
 *     included.  Deferred keys are checked at finish with peaks and final
 *     configs requested;
 *   - lc_stream_report renders a key's counterexample from the stream itself.
 * LC_STREAM_EXACT with LC_STREAM_SET_TIER: the set that migrates is then
 * Knossos's own, and so is every set of the set tier, so all of the above
 * holds for a key in the set tier too: it turns :unknown / invalid at the
 * oracle's event in the call that reaches it, with its peak and the final
 * configs of the set before that event (the max_final smallest in slot-mask,
 * state-id order), a live set-tier key reports its peak so far, and
 * lc_stream_finish fetches its end set.  A key that falls back (a set past
 * 32,768 configs that is still within the budget, window slot 56, a 256th
 * state) gets its record at finish like any deferred key.  On a packer-only
 * stream (ctx NULL), which has no set tier to make exact, the two flags
 * together are refused (LC_E_UNSUPPORTED).
 * LC_OPT_COUNT_PROBES on the context is ignored by a stream, as without it. */
typedef struct lc_stream lc_stream;  /* library-owned */

typedef struct lc_stream_update {
    int64_t        n_keys;      /* keys of the stream so far                          */
    int64_t        events;      /* event words searched on the device in this call    */
    int64_t        rows_held;   /* rows held back, over all keys (rows mode)           */
    int64_t        n_deferred;  /* keys deferred to lc_stream_finish so far            */
    int64_t        n_invalid;   /* keys that turned invalid in this call ...           */
    const int64_t *invalid;     /* ... their key indices, ascending (borrowed: valid
                                   until the stream's next call)                     */
} lc_stream_update;

#define LC_STREAM_REC_WORDS 1360  /* a key's device record, 32-bit words (csrc/stream_plan.hpp) */

/* Options of a stream beyond the packer's (additive to ABI 13). */
#define LC_STREAM_SET_TIER 1u     /* keys past the register tier resume in the resident set tier */
#define LC_STREAM_EXACT    2u     /* the register tier holds Knossos's exact sets: any budget,
                                     peaks, final configs and counterexamples online (below) */
typedef struct lc_stream_opts {
    uint32_t flags;               /* LC_STREAM_* bits; 0: as lc_stream_open */
} lc_stream_opts;

/* Where a key of a stream is searched (lc_stream_key_tier). */
#define LC_STREAM_TIER_REGISTER    0  /* the register tier's resident record                     */
#define LC_STREAM_TIER_SET         1  /* the resident set tier                                   */
#define LC_STREAM_TIER_FALLEN_BACK 2  /* deferred: lc_stream_finish checks it from its first event
                                         (without LC_STREAM_SET_TIER: every deferred key)        */
#define LC_STREAM_TIER_DEAD        3  /* invalid or in error: nothing more of it is searched     */
#define LC_STREAM_SET_HEAD_WORDS 80   /* header (16) and descriptors (64) of a set record        */

/* ctx NULL: a packer-only stream (rows mode without a device: the accessors
 * below work, lc_stream_results does not).  opts NULL: cas-register.  A
 * context of several devices or with a communicator, or one whose budget is
 * below 16 x 64 x 32 (where the register tier's sets are exact; any budget
 * with LC_STREAM_EXACT), is refused with LC_E_UNSUPPORTED; so is
 * LC_MODEL_MULTI_REGISTER.  The context must
 * outlive the stream. */
int  lc_stream_open(lc_ctx *ctx, const lc_pack_opts *opts, lc_stream **out);
/* The same with stream options (sopts NULL: none).  LC_STREAM_SET_TIER on a
 * packer-only stream and in events mode has no effect (lc_stream_push keeps
 * refusing a key_width above 10); with it n_deferred counts the keys that
 * fell back. */
int  lc_stream_open_opts(lc_ctx *ctx, const lc_pack_opts *opts, const lc_stream_opts *sopts, lc_stream **out);
int  lc_stream_append(lc_stream *s, const lc_history *rows, lc_stream_update *u);
int  lc_stream_push(lc_stream *s, const lc_batch *chunk, const int64_t *key_ids, lc_stream_update *u);
int  lc_stream_finish(lc_stream *s, lc_stream_update *u);
/* valid, fail_event and cause of every key so far, in key-index order (the
 * other arrays of r are not touched).  Before lc_stream_finish a key that is
 * neither invalid nor in error is LC_VALID: nothing searched so far refutes it.
 * An LC_STREAM_EXACT stream also fills r->peak_configs, r->final_configs
 * ([n_keys * max_final * 2], unused words zero) and r->n_final where they are
 * not NULL (see "Exact mode" above); analyzer is never touched. */
int  lc_stream_results(lc_stream *s, lc_result *r);
/* The words lc_report writes, for key i of a stream in rows mode: from the
 * stream's own per-key event words, transitions, state values and event rows,
 * so rows are positions in the concatenation of everything appended.  valid,
 * fail_event, final_configs and n_final are the key's (lc_stream_results of an
 * LC_STREAM_EXACT stream, or any other source of the same record).  Returns
 * the word count and writes them when they fit cap.  Events mode has no rows:
 * LC_E_UNSUPPORTED.  A packer-only stream can be asked too. */
int64_t lc_stream_report(const lc_stream *s, int64_t i, int32_t valid, int32_t fail_event,
                         const uint64_t *final_configs, uint32_t n_final, int32_t max_paths, int64_t *out,
                         int64_t cap);
/* Keys in order of first appearance; returns their count (out may be NULL). */
int64_t lc_stream_keys(const lc_stream *s, int64_t *out);
/* Key i's counts: out4 = events emitted (its decided prefix), rows held back,
 * the event ordinal it was deferred at (-1: it is not), events searched on the
 * device. */
int  lc_stream_key_events(const lc_stream *s, int64_t i, int64_t *out4);
/* History row (counted over every row appended, from 0) of event j of key i. */
int64_t lc_stream_event_row(const lc_stream *s, int64_t i, int64_t j);
/* Rows mode: key i's emitted event words (32-bit form) / its transition
 * descriptors; returns the count and writes at most cap. */
int64_t lc_stream_key_words(const lc_stream *s, int64_t i, uint32_t *out, int64_t cap);
int64_t lc_stream_key_trans(const lc_stream *s, int64_t i, uint32_t *out, int64_t cap);
/* Register value of state id st of key i (state 0 = nil -> *is_nil = 1). */
int  lc_stream_state_value(const lc_stream *s, int64_t i, uint32_t st, int64_t *value, int *is_nil);
/* Why key i is in error (NULL when it is not; borrowed). */
const char *lc_stream_key_error(const lc_stream *s, int64_t i);
/* Diagnostics: key i's device record (LC_STREAM_REC_WORDS words), and the
 * times of the last call, ms: [0] host packing, [1] upload, [2] k_stream,
 * [3] readback (device events). */
int  lc_stream_record(lc_stream *s, int64_t i, uint32_t *out);
int  lc_stream_last_timing(const lc_stream *s, double *out_ms4);
/* Diagnostics of an LC_STREAM_EXACT stream: out2 = device ms of
 * lc_stream_finish's k_stream_final launch, and the live keys it wrote the end
 * sets of (zeros before finish and without the flag). */
int  lc_stream_exact_stats(const lc_stream *s, double *out2);
/* Key i's tier (LC_STREAM_TIER_*; negative: an error code), and the count of
 * keys in each, out4[tier].  deferred_at (lc_stream_key_events) names the
 * event at which a key left the register tier, whatever became of it. */
int  lc_stream_key_tier(const lc_stream *s, int64_t i);
int  lc_stream_tiers(const lc_stream *s, int64_t *out4);
/* Diagnostics of the set tier.  lc_stream_set_record: key i's set record as
 * it is in device memory (csrc/stream_plan.hpp) -- LC_STREAM_SET_HEAD_WORDS
 * words of header and descriptors, then the current set's configs, two words
 * each (low, high; state << 56 | window-slot bits); returns the word count
 * and writes at most cap; LC_E_INVALID for a key that is not in the set tier.
 * lc_stream_set_stats: out6 = device ms of the last call's migrations and of
 * its k_stream_set launch; the set-record pool's slots allocated, in use, most
 * in use at once, and bytes per slot. */
int64_t lc_stream_set_record(lc_stream *s, int64_t i, uint32_t *out, int64_t cap);
int  lc_stream_set_stats(const lc_stream *s, double *out6);
void lc_stream_close(lc_stream *s);

#ifdef __cplusplus
}
#endif
#endif /* LINCHECK_H */
