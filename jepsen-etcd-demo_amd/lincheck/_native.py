"""ctypes binding of liblincheck.so (include/lincheck.h).

The same C ABI a JNA binding on the Clojure side would use.
Loading fails loudly when the library is missing: there is no Python or CPU
fallback for the search.
"""

from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LINCHECK_LIB_OVERRIDE") or os.path.join(HERE, "liblincheck.so")  # override: diagnostics only

# ---- constants (mirror include/lincheck.h) ---------------------------------
LC_ABI_VERSION = 13
LC_MAX_DEVICES = 8
LC_COMM_ID_BYTES = 128
LC_OPT_COUNT_PROBES = 0x1
# lc_opts.path_flags (ABI 9): pinned search-path choices for A/B runs and tests
LC_PATH_SPLIT_ON, LC_PATH_SPLIT_OFF, LC_PATH_SPEC_OFF, LC_PATH_LAYERS_OFF = 0x01, 0x02, 0x04, 0x08
LC_PATH_NODE_SYNC, LC_PATH_NODE_STAGED, LC_PATH_CHUNKS_ON, LC_PATH_CHUNKS_OFF = 0x10, 0x20, 0x40, 0x80
LC_PATH_SPEC_COST, LC_PATH_EV32, LC_PATH_SPEC_NOPRIO, LC_PATH_WGL_SMALL = 0x100, 0x200, 0x400, 0x800
LC_PATH_WGL_EV_HBM = 0x2000  # ABI 11
LC_PATH_SPEC_NOSTAGE = 0x1000
LC_PATH_SET_HBM = 0x4000  # ABI 12: lc_set_check, every key through the HBM tier
LC_PATH_SET_DIRECT = 0x8000  # ABI 12: k_set_mark without its LDS tile
LC_PATH_NODE_SERIAL = 0x10000  # lc_check_node_async: one search at a time (A/B against the two search lanes)
LC_T0_PATH_NONE, LC_T0_PATH_LATTICE, LC_T0_PATH_SPEC, LC_T0_PATH_SEGMENTS = 0, 1, 2, 3
T0_PATH_NAMES = {0: "none", 1: "k_search_lattice", 2: "k_spec", 3: "k_search_segments"}
LC_DEV_RESULT, LC_DEV_ASYNC = 1, 2
LC_INVOKE, LC_OK_T, LC_FAIL, LC_INFO = 0, 1, 2, 3
LC_F_READ, LC_F_WRITE, LC_F_CAS, LC_F_OTHER, LC_F_ACQUIRE, LC_F_RELEASE, LC_F_TXN = 0, 1, 2, 3, 4, 5, 6
LC_MOP_READ, LC_MOP_WRITE = 0, 1
LC_MODEL_CAS_REGISTER, LC_MODEL_REGISTER, LC_MODEL_MUTEX, LC_MODEL_MULTI_REGISTER = 0, 1, 2, 3
LC_TABLE_NONE = 0xFFFF
LC_ALGO_LINEAR, LC_ALGO_WGL, LC_ALGO_COMPETITION = 0, 1, 2
ANALYZERS = {LC_ALGO_LINEAR: "linear", LC_ALGO_WGL: "wgl"}
LC_NIL = -(1 << 63)
LC_NO_KEY = LC_NIL
LC_NO_PROCESS = LC_NIL
LC_EV_OK_BIT = 0x80000000
LC_T_READ_ANY, LC_T_READ, LC_T_WRITE, LC_T_CAS = 0, 1, 2, 3
LC_STATE_NONE = 0x7FFF
LC_NARROW_MAX_SLOTS, LC_WIDE_MAX_SLOTS = 56, 112
LC_WIDE_MAX_STATES = 32767
LC_VALID, LC_INVALID, LC_UNKNOWN = 1, 0, -1
LC_CAUSE_ERROR = 5
CAUSES = {0: "none", 1: "nonlin", 2: "budget", 3: "window", 4: "states", 5: "error"}
ERRORS = {-1: "invalid", -2: "nomem", -3: "device", -4: "parse", -5: "unsupported", -6: "io"}

P = C.POINTER


class LcHistory(C.Structure):
    _fields_ = [("n", C.c_int64), ("type", P(C.c_uint8)), ("f", P(C.c_uint8)),
                ("process", P(C.c_int64)), ("key", P(C.c_int64)),
                ("v0", P(C.c_int64)), ("v1", P(C.c_int64)), ("index", P(C.c_int64)),
                ("mop_off", P(C.c_int64)), ("mop", P(C.c_int64))]


class LcBatch(C.Structure):
    _fields_ = [("n_keys", C.c_int64), ("ev_off", P(C.c_uint64)), ("events", P(C.c_uint32)),
                ("trans", P(C.c_uint32)), ("n_trans", C.c_int64), ("trans_off", P(C.c_uint32)),
                ("key_width", P(C.c_uint8)), ("key_states", P(C.c_uint16)),
                ("init_state", C.c_uint32), ("key_error", P(C.c_uint8)),
                ("table", P(C.c_uint16)), ("n_table", C.c_int64), ("events16", P(C.c_uint16))]


class LcPackOpts(C.Structure):
    _fields_ = [("model", C.c_int32), ("n_init", C.c_int32), ("init", P(C.c_int64)), ("flags", C.c_uint32)]


LC_PACK_GENERAL = 0x1  # lc_pack_opts.flags (ABI 11): always the bucketing path


class LcOpts(C.Structure):
    _fields_ = [("device", C.c_int32), ("algorithm", C.c_int32), ("max_configs", C.c_uint64),
                ("max_final", C.c_int32), ("lds_configs", C.c_int32), ("deep_slots", C.c_int32),
                ("flags", C.c_int32), ("debug_mode", C.c_int32),
                ("n_devices", C.c_int32), ("devices", C.c_int32 * LC_MAX_DEVICES),
                ("comm_rank", C.c_int32), ("comm_size", C.c_int32), ("comm_id", C.c_uint8 * LC_COMM_ID_BYTES),
                ("path_flags", C.c_int32), ("spec_segs", C.c_int32), ("spec_ck", C.c_int32),
                ("seg_len", C.c_int32)]


class LcResult(C.Structure):
    _fields_ = [("valid", P(C.c_int8)), ("fail_event", P(C.c_int32)), ("cause", P(C.c_uint8)),
                ("peak_configs", P(C.c_uint32)), ("final_configs", P(C.c_uint64)),
                ("n_final", P(C.c_uint32)), ("analyzer", P(C.c_uint8))]


class LcStats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("total_ms", C.c_double), ("probes", C.c_uint64),
                ("lds_keys", C.c_uint64), ("deep_keys", C.c_uint64), ("events", C.c_uint64),
                ("tier0_ms", C.c_double), ("tier3_ms", C.c_double),
                ("probes_t3", C.c_uint64), ("t3_bytes", C.c_uint64),
                ("t0_path", C.c_uint32), ("ev_word_bytes", C.c_uint32),
                ("wgl_ms", C.c_double), ("wgl_keys", C.c_uint64), ("wgl_spilled", C.c_uint64),
                ("wgl_steps", C.c_uint64)]


class LcSynthOpts(C.Structure):
    _fields_ = [("n_keys", C.c_int64), ("ops_per_key", C.c_int64), ("concurrency", C.c_int32),
                ("n_values", C.c_int32), ("info_rate", C.c_double), ("info_effect_p", C.c_double),
                ("anomaly_rate", C.c_double), ("mean_think", C.c_double),
                ("mean_latency", C.c_double), ("interleave", C.c_int32),
                ("nemesis_period", C.c_double), ("seed", C.c_uint64), ("key_base", C.c_int64)]


# ---- the set workload (ABI 12) ----------------------------------------------
LC_SF_ADD, LC_SF_READ, LC_SF_OTHER = 0, 1, 2
LC_SET_ATTEMPT, LC_SET_ACK = 1, 2
LC_SET_KEY_OK, LC_SET_KEY_NEVER_READ, LC_SET_KEY_ERROR = 0, 1, 2


class LcSetHistory(C.Structure):
    _fields_ = [("n", C.c_int64), ("type", P(C.c_uint8)), ("f", P(C.c_uint8)), ("key", P(C.c_int64)),
                ("elem", P(C.c_int64)), ("read_off", P(C.c_int64)), ("read_elem", P(C.c_int64)),
                ("index", P(C.c_int64))]


class LcSetBatch(C.Structure):
    _fields_ = [("n_keys", C.c_int64), ("add_off", P(C.c_uint64)), ("add_id", P(C.c_uint32)),
                ("add_cls", P(C.c_uint8)), ("read_off", P(C.c_uint64)), ("read_id", P(C.c_uint32)),
                ("base", P(C.c_uint64)), ("span", P(C.c_uint32)), ("min", P(C.c_int64)), ("rank", P(C.c_uint8)),
                ("vals_off", P(C.c_uint64)), ("vals", P(C.c_int64)), ("status", P(C.c_uint8)),
                ("n_words", C.c_uint64)]


class LcSetResult(C.Structure):
    _fields_ = [("valid", P(C.c_int8)), ("counts", P(C.c_uint64)), ("run_off", P(C.c_uint64)),
                ("runs", P(C.c_int64)), ("run_cap", C.c_uint64), ("n_runs", C.c_uint64)]


# ---- checker/set-full (ABI 13, additive) ----------------------------------------
LC_SETFULL_NONE = -1
LC_SETFULL_UNTRACKED, LC_SETFULL_STABLE, LC_SETFULL_LOST, LC_SETFULL_NEVER_READ = 0, 1, 2, 3
LC_SETFULL_MARK_DIRECT = 0x1  # lc_setfull_opts.flags


class LcSetFullHistory(C.Structure):
    _fields_ = [("n", C.c_int64), ("type", P(C.c_uint8)), ("f", P(C.c_uint8)), ("key", P(C.c_int64)),
                ("elem", P(C.c_int64)), ("read_off", P(C.c_int64)), ("read_elem", P(C.c_int64)),
                ("index", P(C.c_int64)), ("process", P(C.c_int64)), ("time", P(C.c_int64))]


class LcSetFullBatch(C.Structure):
    _fields_ = [("n_keys", C.c_int64), ("id_off", P(C.c_uint64)), ("span", P(C.c_uint32)), ("min", P(C.c_int64)),
                ("rank", P(C.c_uint8)), ("vals_off", P(C.c_uint64)), ("vals", P(C.c_int64)), ("status", P(C.c_uint8)),
                ("inv_pos", P(C.c_int64)), ("ack_pos", P(C.c_int64)), ("ack_time", P(C.c_int64)),
                ("row_off", P(C.c_uint64)), ("row_pos", P(C.c_int64)), ("row_time", P(C.c_int64)),
                ("row_inv_pos", P(C.c_int64)), ("row_inv_time", P(C.c_int64)), ("el_off", P(C.c_uint64)),
                ("read_id", P(C.c_uint32))]


class LcSetFullOpts(C.Structure):
    _fields_ = [("linearizable", C.c_int32), ("flags", C.c_uint32), ("max_matrix_bytes", C.c_uint64)]


class LcSetFullResult(C.Structure):
    _fields_ = [("valid", P(C.c_int8)), ("counts", P(C.c_uint64)), ("outcome", P(C.c_uint8)),
                ("latency", P(C.c_int64)), ("known", P(C.c_int64)), ("last_absent", P(C.c_int64)),
                ("duplicated", P(C.c_uint8))]


# ---- checker/perf (ABI 13) ---------------------------------------------------
LC_PERF_MAX_F, LC_PERF_MAX_Q = 32, 8
LC_PERF_NO_INVOKE = LC_NIL
LC_PERF_SELECT_HBM, LC_PERF_COUNT_DIRECT = 0x1, 0x2  # lc_perf_opts.flags


class LcPerfHistory(C.Structure):
    _fields_ = [("n", C.c_int64), ("type", P(C.c_uint8)), ("f", P(C.c_uint8)), ("process", P(C.c_int64)),
                ("time", P(C.c_int64)), ("n_f", C.c_int32), ("f_start", C.c_int32), ("f_stop", C.c_int32)]


class LcPerfBatch(C.Structure):
    _fields_ = [("n", C.c_int64), ("t_comp", P(C.c_int64)), ("t_inv", P(C.c_int64)), ("meta", P(C.c_uint32)),
                ("n_matched", C.c_int64), ("t_min", C.c_int64), ("t_max", C.c_int64), ("x_min", C.c_int64),
                ("x_max", C.c_int64), ("n_f", C.c_int32), ("reserved", C.c_int32)]


class LcPerfOpts(C.Structure):
    _fields_ = [("quantile_dt_ns", C.c_int64), ("rate_dt_ns", C.c_int64), ("n_q", C.c_int32), ("flags", C.c_uint32),
                ("q", C.c_double * LC_PERF_MAX_Q)]


class LcPerfResult(C.Structure):
    _fields_ = [("rate", P(C.c_uint64)), ("group", P(C.c_uint64)), ("quant", P(C.c_int64)),
                ("rate_cap", C.c_uint64), ("group_cap", C.c_uint64), ("quant_cap", C.c_uint64),
                ("rate_first", C.c_int64), ("rate_n", C.c_int64), ("q_first", C.c_int64), ("q_n", C.c_int64)]


# ---- incremental check (lc_stream_*) -------------------------------------------
LC_STREAM_REC_WORDS = 1360
LC_STREAM_SET_TIER = 1
LC_STREAM_EXACT = 2
LC_STREAM_TIER_REGISTER, LC_STREAM_TIER_SET, LC_STREAM_TIER_FALLEN_BACK, LC_STREAM_TIER_DEAD = 0, 1, 2, 3
LC_STREAM_SET_HEAD_WORDS = 80


class LcStreamOpts(C.Structure):
    _fields_ = [("flags", C.c_uint32)]


class LcStreamUpdate(C.Structure):
    _fields_ = [("n_keys", C.c_int64), ("events", C.c_int64), ("rows_held", C.c_int64), ("n_deferred", C.c_int64),
                ("n_invalid", C.c_int64), ("invalid", P(C.c_int64))]


# Every exported symbol: name -> (restype, argtypes).  tests/test_abi.py checks
# this table against include/lincheck.h.
SIGNATURES = {
    "lc_abi_version": (C.c_int, []),
    "lc_trim": (None, []),
    "lc_last_error": (C.c_char_p, []),
    "lc_device_count": (C.c_int, []),
    "lc_create": (C.c_int, [P(LcOpts), P(C.c_void_p)]),
    "lc_destroy": (None, [C.c_void_p]),
    "lc_check_batch": (C.c_int, [C.c_void_p, P(LcBatch), P(LcResult), P(LcStats)]),
    "lc_upload": (C.c_int, [C.c_void_p, P(LcBatch), P(C.c_void_p)]),
    "lc_dev_batch_free": (None, [C.c_void_p]),
    "lc_check_device": (C.c_int, [C.c_void_p, C.c_void_p, P(LcResult), C.c_int, P(LcStats)]),
    "lc_wait": (C.c_int, [C.c_void_p, P(LcStats)]),
    "lc_wait_step": (C.c_int, [C.c_void_p, C.c_int]),
    "lc_comm_id": (C.c_int, [P(C.c_uint8)]),
    "lc_check_node": (C.c_int, [C.c_void_p, P(LcBatch), C.c_int64, P(C.c_uint64), P(LcStats)]),
    "lc_check_node_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, P(LcStats)]),
    "lc_check_node_async": (C.c_int, [C.c_void_p, P(LcBatch), C.c_int64, P(C.c_uint64), P(LcStats)]),
    "lc_host_alloc": (C.c_void_p, [C.c_size_t]),
    "lc_host_free": (None, [C.c_void_p]),
    "lc_node_records": (C.c_int, [C.c_void_p, P(C.c_uint64), C.c_int64]),
    "lc_pack": (C.c_int, [P(LcHistory), P(LcPackOpts), P(C.c_void_p)]),
    "lc_packed_free": (None, [C.c_void_p]),
    "lc_packed_view": (C.c_int, [C.c_void_p, P(LcBatch)]),
    "lc_packed_key": (C.c_int64, [C.c_void_p, C.c_int64]),
    "lc_packed_event_row": (C.c_int64, [C.c_void_p, C.c_int64, C.c_int64]),
    "lc_packed_path": (C.c_int, [C.c_void_p]),
    "lc_packed_event_rows": (C.c_int64, [C.c_void_p, P(C.c_int64)]),
    "lc_packed_subhistory": (C.c_int64, [C.c_void_p, C.c_int64, P(C.c_int64)]),
    "lc_packed_key_error": (C.c_char_p, [C.c_void_p, C.c_int64]),
    "lc_packed_state_value": (C.c_int, [C.c_void_p, C.c_int64, C.c_uint32, P(C.c_int64), P(C.c_int)]),
    "lc_packed_keys": (C.c_int, [C.c_void_p, P(C.c_int64)]),
    "lc_packed_state_map": (C.c_int64, [C.c_void_p, C.c_int64, C.c_uint32, P(C.c_int64), P(C.c_int64), C.c_int64]),
    "lc_report": (C.c_int64, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, P(C.c_uint64), C.c_uint32, C.c_int32,
                              P(C.c_int64), C.c_int64]),
    "lc_report_wgl": (C.c_int64, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, P(C.c_uint64), C.c_uint32, C.c_int32,
                                  P(C.c_int64), C.c_int64]),
    "lc_synth_generate": (C.c_int, [P(LcSynthOpts), P(C.c_void_p)]),
    "lc_hist_view": (C.c_int, [C.c_void_p, P(LcHistory)]),
    "lc_hist_anomalous_keys": (C.c_int64, [C.c_void_p, P(C.c_int64)]),
    "lc_hist_free": (None, [C.c_void_p]),
    "lc_edn_read": (C.c_int, [C.c_char_p, P(C.c_void_p)]),
    "lc_edn_parse": (C.c_int, [C.c_char_p, C.c_int64, P(C.c_void_p)]),
    "lc_edn_write": (C.c_int, [C.c_char_p, P(LcHistory)]),
    "lc_edn_write_named": (C.c_int, [C.c_char_p, P(LcHistory), P(C.c_char_p), C.c_int64]),
    "lc_hist_n_reg_names": (C.c_int64, [C.c_void_p]),
    "lc_hist_reg_name": (C.c_char_p, [C.c_void_p, C.c_int64]),
    "lc_fressian_read": (C.c_int, [C.c_char_p, P(C.c_void_p)]),
    "lc_fressian_parse": (C.c_int, [C.c_char_p, C.c_int64, P(C.c_void_p)]),
    "lc_fressian_write": (C.c_int, [C.c_char_p, P(LcHistory)]),
    "lc_set_pack": (C.c_int, [P(LcSetHistory), P(C.c_void_p)]),
    "lc_set_packed_free": (None, [C.c_void_p]),
    "lc_set_packed_view": (C.c_int, [C.c_void_p, P(LcSetBatch)]),
    "lc_set_packed_keys": (C.c_int, [C.c_void_p, P(C.c_int64)]),
    "lc_set_packed_key_error": (C.c_char_p, [C.c_void_p, C.c_int64]),
    "lc_set_batch_max_runs": (C.c_int64, [P(LcSetBatch)]),
    "lc_set_check": (C.c_int, [C.c_void_p, P(LcSetBatch), P(LcSetResult)]),
    "lc_set_last_timing": (C.c_int, [C.c_void_p, P(C.c_double)]),
    "lc_set_launch_info": (C.c_int, [P(C.c_int64)]),
    "lc_edn_read_set": (C.c_int, [C.c_char_p, P(C.c_void_p)]),
    "lc_edn_parse_set": (C.c_int, [C.c_char_p, C.c_int64, P(C.c_void_p)]),
    "lc_set_hist_view": (C.c_int, [C.c_void_p, P(LcSetHistory)]),
    "lc_set_hist_free": (None, [C.c_void_p]),
    "lc_setfull_pack": (C.c_int, [P(LcSetFullHistory), P(C.c_void_p)]),
    "lc_setfull_packed_free": (None, [C.c_void_p]),
    "lc_setfull_packed_view": (C.c_int, [C.c_void_p, P(LcSetFullBatch)]),
    "lc_setfull_packed_keys": (C.c_int, [C.c_void_p, P(C.c_int64)]),
    "lc_setfull_packed_key_error": (C.c_char_p, [C.c_void_p, C.c_int64]),
    "lc_setfull_check": (C.c_int, [C.c_void_p, P(LcSetFullBatch), P(LcSetFullOpts), P(LcSetFullResult)]),
    "lc_setfull_last_timing": (C.c_int, [C.c_void_p, P(C.c_double)]),
    "lc_setfull_launch_info": (C.c_int, [P(C.c_int64)]),
    "lc_edn_read_setfull": (C.c_int, [C.c_char_p, P(C.c_void_p)]),
    "lc_edn_parse_setfull": (C.c_int, [C.c_char_p, C.c_int64, P(C.c_void_p)]),
    "lc_setfull_hist_view": (C.c_int, [C.c_void_p, P(LcSetFullHistory)]),
    "lc_setfull_hist_free": (None, [C.c_void_p]),
    "lc_perf_pack": (C.c_int, [P(LcPerfHistory), P(C.c_void_p)]),
    "lc_perf_packed_free": (None, [C.c_void_p]),
    "lc_perf_packed_view": (C.c_int, [C.c_void_p, P(LcPerfBatch)]),
    "lc_perf_packed_info": (C.c_int, [C.c_void_p, P(C.c_int64)]),
    "lc_perf_packed_intervals": (C.c_int, [C.c_void_p, P(C.c_int64)]),
    "lc_perf_opts_default": (None, [P(LcPerfOpts)]),
    "lc_perf_shape": (C.c_int, [P(LcPerfBatch), P(LcPerfOpts), P(C.c_int64)]),
    "lc_perf_check": (C.c_int, [C.c_void_p, P(LcPerfBatch), P(LcPerfOpts), P(LcPerfResult)]),
    "lc_perf_last_timing": (C.c_int, [C.c_void_p, P(C.c_double)]),
    "lc_perf_launch_info": (C.c_int, [P(C.c_int64)]),
    "lc_edn_read_perf": (C.c_int, [C.c_char_p, P(C.c_void_p)]),
    "lc_edn_parse_perf": (C.c_int, [C.c_char_p, C.c_int64, P(C.c_void_p)]),
    "lc_perf_hist_view": (C.c_int, [C.c_void_p, P(LcPerfHistory)]),
    "lc_perf_hist_name": (C.c_char_p, [C.c_void_p, C.c_int64]),
    "lc_perf_hist_free": (None, [C.c_void_p]),
    "lc_stream_open": (C.c_int, [C.c_void_p, P(LcPackOpts), P(C.c_void_p)]),
    "lc_stream_open_opts": (C.c_int, [C.c_void_p, P(LcPackOpts), P(LcStreamOpts), P(C.c_void_p)]),
    "lc_stream_key_tier": (C.c_int, [C.c_void_p, C.c_int64]),
    "lc_stream_tiers": (C.c_int, [C.c_void_p, P(C.c_int64)]),
    "lc_stream_set_record": (C.c_int64, [C.c_void_p, C.c_int64, P(C.c_uint32), C.c_int64]),
    "lc_stream_set_stats": (C.c_int, [C.c_void_p, P(C.c_double)]),
    "lc_stream_append": (C.c_int, [C.c_void_p, P(LcHistory), P(LcStreamUpdate)]),
    "lc_stream_push": (C.c_int, [C.c_void_p, P(LcBatch), P(C.c_int64), P(LcStreamUpdate)]),
    "lc_stream_finish": (C.c_int, [C.c_void_p, P(LcStreamUpdate)]),
    "lc_stream_results": (C.c_int, [C.c_void_p, P(LcResult)]),
    "lc_stream_exact_stats": (C.c_int, [C.c_void_p, P(C.c_double)]),
    "lc_stream_report": (C.c_int64, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, P(C.c_uint64), C.c_uint32, C.c_int32,
                                     P(C.c_int64), C.c_int64]),
    "lc_stream_keys": (C.c_int64, [C.c_void_p, P(C.c_int64)]),
    "lc_stream_key_events": (C.c_int, [C.c_void_p, C.c_int64, P(C.c_int64)]),
    "lc_stream_event_row": (C.c_int64, [C.c_void_p, C.c_int64, C.c_int64]),
    "lc_stream_key_words": (C.c_int64, [C.c_void_p, C.c_int64, P(C.c_uint32), C.c_int64]),
    "lc_stream_key_trans": (C.c_int64, [C.c_void_p, C.c_int64, P(C.c_uint32), C.c_int64]),
    "lc_stream_state_value": (C.c_int, [C.c_void_p, C.c_int64, C.c_uint32, P(C.c_int64), P(C.c_int)]),
    "lc_stream_key_error": (C.c_char_p, [C.c_void_p, C.c_int64]),
    "lc_stream_record": (C.c_int, [C.c_void_p, C.c_int64, P(C.c_uint32)]),
    "lc_stream_last_timing": (C.c_int, [C.c_void_p, P(C.c_double)]),
    "lc_stream_close": (None, [C.c_void_p]),
}


# ---- streaming set-full (include/lincheck_setfull_stream.h; ABI 13, additive) ----
# A header and a table of their own: SIGNATURES mirrors include/lincheck.h name for name.
LC_SFS_FRESH, LC_SFS_ACK = 0x1, 0x2  # lc_setfull_stream_chunk.en_flags


class LcSetFullStreamUpdate(C.Structure):
    _fields_ = [("n_keys", C.c_int64), ("rows", C.c_int64), ("reads", C.c_int64), ("ids", C.c_int64),
                ("n_changed", C.c_int64), ("changed", P(C.c_int64))]


class LcSetFullStreamChunk(C.Structure):
    _fields_ = [("n_touched", C.c_int64), ("tk_key", P(C.c_int64)), ("tk_n_ids", P(C.c_uint32)),
                ("tk_row_off", P(C.c_uint64)), ("tk_blk_off", P(C.c_uint64)), ("blk", P(C.c_uint32)),
                ("n_entries", C.c_int64), ("en_t", P(C.c_uint32)), ("en_id", P(C.c_uint32)), ("en_flags", P(C.c_uint32)),
                ("en_inv_pos", P(C.c_int64)), ("en_ack_pos", P(C.c_int64)), ("en_ack_time", P(C.c_int64)),
                ("row_pos", P(C.c_int64)), ("row_time", P(C.c_int64)), ("row_inv_pos", P(C.c_int64)),
                ("row_inv_time", P(C.c_int64)), ("el_off", P(C.c_uint64)), ("read_id", P(C.c_uint32))]


SETFULL_STREAM_SIGNATURES = {
    "lc_setfull_stream_open": (C.c_int, [C.c_void_p, P(LcSetFullOpts), P(C.c_void_p)]),
    "lc_setfull_stream_append": (C.c_int, [C.c_void_p, P(LcSetFullHistory), P(LcSetFullStreamUpdate)]),
    "lc_setfull_stream_counts": (C.c_int, [C.c_void_p, P(C.c_int8), P(C.c_uint64)]),
    "lc_setfull_stream_ids": (C.c_int64, [C.c_void_p, C.c_int64, P(C.c_int64), C.c_int64]),
    "lc_setfull_stream_results": (C.c_int, [C.c_void_p, P(LcSetFullResult)]),
    "lc_setfull_stream_keys": (C.c_int64, [C.c_void_p, P(C.c_int64)]),
    "lc_setfull_stream_key_error": (C.c_char_p, [C.c_void_p, C.c_int64]),
    "lc_setfull_stream_multiplicity": (C.c_int, [C.c_void_p, C.c_int64, P(C.c_uint32), C.c_int64]),
    "lc_setfull_stream_last_chunk": (C.c_int, [C.c_void_p, P(LcSetFullStreamChunk)]),
    "lc_setfull_stream_last_timing": (C.c_int, [C.c_void_p, P(C.c_double)]),
    "lc_setfull_stream_close": (None, [C.c_void_p]),
}

# ---- checker/counter (include/lincheck_counter.h; ABI 13, additive) ----------------
# A header and a table of their own, as the streaming set-full's.
LC_CF_ADD, LC_CF_READ, LC_CF_OTHER = 0, 1, 2
LC_CE_UP, LC_CE_LOW, LC_CE_RINV, LC_CE_ROK = 0, 1, 2, 3
LC_COUNTER_KEY_OK, LC_COUNTER_KEY_ERROR = 0, 1


class LcCounterHistory(C.Structure):
    _fields_ = [("n", C.c_int64), ("type", P(C.c_uint8)), ("f", P(C.c_uint8)), ("process", P(C.c_int64)),
                ("key", P(C.c_int64)), ("value", P(C.c_int64)), ("index", P(C.c_int64))]


class LcCounterBatch(C.Structure):
    _fields_ = [("n_keys", C.c_int64), ("ev_off", P(C.c_uint64)), ("ev_kind", P(C.c_uint8)), ("ev_val", P(C.c_int64)),
                ("read_off", P(C.c_uint64)), ("read_val", P(C.c_int64)), ("status", P(C.c_uint8))]


class LcCounterOpts(C.Structure):
    _fields_ = [("tile", C.c_uint32), ("flags", C.c_uint32)]


class LcCounterResult(C.Structure):
    _fields_ = [("valid", P(C.c_int8)), ("n_errors", P(C.c_uint64)), ("lower", P(C.c_int64)), ("upper", P(C.c_int64)),
                ("err_off", P(C.c_uint64)), ("err_idx", P(C.c_uint64)), ("err_cap", C.c_uint64), ("n_err", C.c_uint64)]


COUNTER_SIGNATURES = {
    "lc_counter_pack": (C.c_int, [P(LcCounterHistory), P(C.c_void_p)]),
    "lc_counter_packed_free": (None, [C.c_void_p]),
    "lc_counter_packed_view": (C.c_int, [C.c_void_p, P(LcCounterBatch)]),
    "lc_counter_packed_keys": (C.c_int, [C.c_void_p, P(C.c_int64)]),
    "lc_counter_packed_key_error": (C.c_char_p, [C.c_void_p, C.c_int64]),
    "lc_counter_check": (C.c_int, [C.c_void_p, P(LcCounterBatch), P(LcCounterOpts), P(LcCounterResult)]),
    "lc_counter_check_host": (C.c_int, [P(LcCounterBatch), P(LcCounterResult)]),
    "lc_counter_last_timing": (C.c_int, [C.c_void_p, P(C.c_double)]),
    "lc_counter_launch_info": (C.c_int, [P(C.c_int64)]),
    "lc_edn_read_counter": (C.c_int, [C.c_char_p, P(C.c_void_p)]),
    "lc_edn_parse_counter": (C.c_int, [C.c_char_p, C.c_int64, P(C.c_void_p)]),
    "lc_counter_hist_view": (C.c_int, [C.c_void_p, P(LcCounterHistory)]),
    "lc_counter_hist_free": (None, [C.c_void_p]),
}

# ---- checker/counter from raw rows (include/lincheck_counter_pack.h; ABI 13, additive) ----
# A header and a table of their own: COUNTER_SIGNATURES mirrors include/lincheck_counter.h name for name.
COUNTER_PACK_SIGNATURES = {
    "lc_counter_check_history": (C.c_int, [C.c_void_p, P(LcCounterHistory), P(LcCounterOpts), P(C.c_void_p)]),
    "lc_counter_checked_free": (None, [C.c_void_p]),
    "lc_counter_checked_view": (C.c_int, [C.c_void_p, P(LcCounterBatch), P(LcCounterResult)]),
    "lc_counter_checked_keys": (C.c_int, [C.c_void_p, P(C.c_int64)]),
    "lc_counter_checked_key_error": (C.c_char_p, [C.c_void_p, C.c_int64]),
    "lc_counter_checked_key_error_row": (C.c_int64, [C.c_void_p, C.c_int64]),
    "lc_counter_checked_read_vals": (C.c_int, [C.c_void_p, P(C.c_int64)]),
    "lc_counter_checked_batch": (C.c_int, [C.c_void_p, C.c_void_p, P(LcCounterBatch)]),
    "lc_counter_history_timing": (C.c_int, [C.c_void_p, P(C.c_double)]),
    "lc_counter_pack_launch_info": (C.c_int, [P(C.c_int64)]),
    "lc_counter_pack_table_slots": (C.c_int64, [C.c_int64]),
}

# ---- checker/perf from raw rows (include/lincheck_perf_pack.h; ABI 13, additive) ----
# A header and a table of their own: SIGNATURES mirrors include/lincheck.h name for name.
PERF_PACK_SIGNATURES = {
    "lc_perf_check_history": (C.c_int, [C.c_void_p, P(LcPerfHistory), P(LcPerfOpts), P(C.c_void_p)]),
    "lc_perf_checked_free": (None, [C.c_void_p]),
    "lc_perf_checked_view": (C.c_int, [C.c_void_p, P(LcPerfBatch), P(LcPerfResult)]),
    "lc_perf_checked_info": (C.c_int, [C.c_void_p, P(C.c_int64)]),
    "lc_perf_checked_intervals": (C.c_int, [C.c_void_p, P(C.c_int64)]),
    "lc_perf_checked_records": (C.c_int, [C.c_void_p, C.c_void_p, P(LcPerfBatch)]),
    "lc_perf_history_timing": (C.c_int, [C.c_void_p, P(C.c_double)]),
    "lc_perf_pack_launch_info": (C.c_int, [P(C.c_int64)]),
}

# ---- checker/total-queue and /unique-ids (include/lincheck_queue.h; ABI 13, additive) ----
LC_QF_ENQUEUE, LC_QF_DEQUEUE, LC_QF_DRAIN, LC_QF_GENERATE, LC_QF_OTHER = 0, 1, 2, 3, 4
LC_QM_TOTAL_QUEUE, LC_QM_UNIQUE_IDS = 0, 1
LC_QK_ATTEMPT, LC_QK_ACK, LC_QK_DEQUEUE = 0, 1, 2
LC_QUEUE_KEY_OK, LC_QUEUE_KEY_ERROR = 0, 1
LC_QN_ATTEMPT, LC_QN_ACKNOWLEDGED, LC_QN_OK, LC_QN_UNEXPECTED, LC_QN_DUPLICATED, LC_QN_LOST, LC_QN_RECOVERED = range(7)
LC_QN_COUNTS = 7
LC_QC_LOST, LC_QC_UNEXPECTED, LC_QC_DUPLICATED, LC_QC_RECOVERED = 0, 1, 2, 3


class LcQueueHistory(C.Structure):
    _fields_ = [("n", C.c_int64), ("type", P(C.c_uint8)), ("f", P(C.c_uint8)), ("key", P(C.c_int64)),
                ("value", P(C.c_int64)), ("drain_off", P(C.c_uint64)), ("drain_val", P(C.c_int64))]


class LcQueueBatch(C.Structure):
    _fields_ = [("n_keys", C.c_int64), ("n_rows", C.c_int64), ("mode", C.c_uint32), ("reserved", C.c_uint32),
                ("row_key", P(C.c_uint32)), ("row_kind", P(C.c_uint8)), ("row_val", P(C.c_int64)),
                ("status", P(C.c_uint8)), ("attempted", P(C.c_uint64))]


class LcQueueOpts(C.Structure):
    _fields_ = [("slots", C.c_uint32), ("flags", C.c_uint32)]


class LcQueueResult(C.Structure):
    _fields_ = [("valid", P(C.c_int8)), ("counts", P(C.c_uint64)), ("lo", P(C.c_int64)), ("hi", P(C.c_int64)),
                ("has_range", P(C.c_uint8)), ("ent_key", P(C.c_uint32)), ("ent_class", P(C.c_uint8)),
                ("ent_val", P(C.c_int64)), ("ent_mult", P(C.c_uint64)), ("ent_cap", C.c_uint64), ("n_ent", C.c_uint64)]


QUEUE_SIGNATURES = {
    "lc_queue_pack": (C.c_int, [P(LcQueueHistory), C.c_uint32, P(C.c_void_p)]),
    "lc_queue_packed_free": (None, [C.c_void_p]),
    "lc_queue_packed_view": (C.c_int, [C.c_void_p, P(LcQueueBatch)]),
    "lc_queue_packed_keys": (C.c_int, [C.c_void_p, P(C.c_int64)]),
    "lc_queue_packed_key_error": (C.c_char_p, [C.c_void_p, C.c_int64]),
    "lc_queue_check": (C.c_int, [C.c_void_p, P(LcQueueBatch), P(LcQueueOpts), P(LcQueueResult)]),
    "lc_queue_check_host": (C.c_int, [P(LcQueueBatch), P(LcQueueResult)]),
    "lc_queue_last_timing": (C.c_int, [C.c_void_p, P(C.c_double)]),
    "lc_queue_launch_info": (C.c_int, [P(C.c_int64)]),
    "lc_edn_read_queue": (C.c_int, [C.c_char_p, P(C.c_void_p)]),
    "lc_edn_parse_queue": (C.c_int, [C.c_char_p, C.c_int64, P(C.c_void_p)]),
    "lc_queue_hist_view": (C.c_int, [C.c_void_p, P(LcQueueHistory)]),
    "lc_queue_hist_free": (None, [C.c_void_p]),
}

# ---- streaming total-queue and unique-ids (include/lincheck_queue_stream.h; ABI 13, additive) ----
# A header and a table of their own: QUEUE_SIGNATURES mirrors include/lincheck_queue.h name for name.


class LcQueueStreamOpts(C.Structure):
    _fields_ = [("slots", C.c_uint32), ("flags", C.c_uint32)]


class LcQueueStreamUpdate(C.Structure):
    _fields_ = [("n_keys", C.c_int64), ("rows", C.c_int64), ("packed", C.c_int64), ("distinct", C.c_int64),
                ("slots", C.c_int64), ("grew", C.c_int64), ("n_changed", C.c_int64), ("changed", P(C.c_int64))]


QUEUE_STREAM_SIGNATURES = {
    "lc_queue_stream_open": (C.c_int, [C.c_void_p, C.c_uint32, P(LcQueueStreamOpts), P(C.c_void_p)]),
    "lc_queue_stream_append": (C.c_int, [C.c_void_p, P(LcQueueHistory), P(LcQueueStreamUpdate)]),
    "lc_queue_stream_counts": (C.c_int, [C.c_void_p, P(C.c_int8), P(C.c_uint64), P(C.c_int64), P(C.c_int64), P(C.c_uint8)]),
    "lc_queue_stream_results": (C.c_int, [C.c_void_p, P(LcQueueResult)]),
    "lc_queue_stream_keys": (C.c_int64, [C.c_void_p, P(C.c_int64)]),
    "lc_queue_stream_key_error": (C.c_char_p, [C.c_void_p, C.c_int64]),
    "lc_queue_stream_last_timing": (C.c_int, [C.c_void_p, P(C.c_double)]),
    "lc_queue_stream_launch_info": (C.c_int, [P(C.c_int64)]),
    "lc_queue_stream_close": (None, [C.c_void_p]),
}

# ---- streaming checker/counter (include/lincheck_counter_stream.h; ABI 13, additive) ----
# A header and a table of their own: COUNTER_SIGNATURES mirrors include/lincheck_counter.h name for name.


class LcCounterStreamOpts(C.Structure):
    _fields_ = [("tile", C.c_uint32), ("reads", C.c_uint32), ("launch_events", C.c_uint32), ("flags", C.c_uint32)]


class LcCounterStreamUpdate(C.Structure):
    _fields_ = [("n_keys", C.c_int64), ("rows", C.c_int64), ("events", C.c_int64), ("reads", C.c_int64),
                ("reads_total", C.c_int64), ("patched", C.c_int64), ("revisited", C.c_int64), ("grew", C.c_int64),
                ("n_changed", C.c_int64), ("changed", P(C.c_int64))]


COUNTER_STREAM_SIGNATURES = {
    "lc_counter_stream_open": (C.c_int, [C.c_void_p, P(LcCounterStreamOpts), P(C.c_void_p)]),
    "lc_counter_stream_append": (C.c_int, [C.c_void_p, P(LcCounterHistory), P(LcCounterStreamUpdate)]),
    "lc_counter_stream_counts": (C.c_int, [C.c_void_p, P(C.c_int8), P(C.c_uint64), P(C.c_uint64)]),
    "lc_counter_stream_results": (C.c_int, [C.c_void_p, P(LcCounterResult), P(C.c_int64)]),
    "lc_counter_stream_keys": (C.c_int64, [C.c_void_p, P(C.c_int64)]),
    "lc_counter_stream_key_error": (C.c_char_p, [C.c_void_p, C.c_int64]),
    "lc_counter_stream_last_timing": (C.c_int, [C.c_void_p, P(C.c_double)]),
    "lc_counter_stream_launch_info": (C.c_int, [P(C.c_int64)]),
    "lc_counter_stream_close": (None, [C.c_void_p]),
}

_lib: Optional[C.CDLL] = None


class LincheckError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{ERRORS.get(code, code)}: {msg}")
        self.code = code


def lib() -> C.CDLL:
    """Load liblincheck.so (built in-tree by __graft_entry__.build())."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        L = C.CDLL(LIB_PATH)
        tables = (SIGNATURES, SETFULL_STREAM_SIGNATURES, COUNTER_SIGNATURES, QUEUE_SIGNATURES, QUEUE_STREAM_SIGNATURES,
                  COUNTER_STREAM_SIGNATURES, COUNTER_PACK_SIGNATURES, PERF_PACK_SIGNATURES)
        for name, (res, args) in [item for t in tables for item in t.items()]:
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        if L.lc_abi_version() != LC_ABI_VERSION:
            raise ImportError(f"liblincheck ABI {L.lc_abi_version()} != {LC_ABI_VERSION}")
        _lib = L
    return _lib


def check(rc: int) -> int:
    if rc < 0:
        raise LincheckError(rc, lib().lc_last_error().decode(errors="replace"))
    return rc


def ptr(a: np.ndarray, ctype):
    return a.ctypes.data_as(P(ctype))


def carray(p, n: int, dtype) -> np.ndarray:
    """Copy n elements from a ctypes pointer (NULL -> empty)."""
    if not p or n == 0:
        return np.zeros(0, dtype=dtype)
    return np.ctypeslib.as_array(p, shape=(n,)).astype(dtype, copy=True)
