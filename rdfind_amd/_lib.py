"""ctypes binding of the C ABI in ``include/rdfind_hip.h`` (``rdfind_amd/librdfind_hip.so``).

This is the product path: there is no CPU fallback.  If the HIP library is missing or no GPU is
visible, :func:`load` / :class:`Context` raise immediately.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from . import codes

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RDFIND_HIP_LIB") or os.path.join(_HERE, "librdfind_hip.so")  # env: dev variants only

RDF_CLEAN_IMPLIED = 1
RDF_STRATEGY_ALL_AT_ONCE = 2
RDF_SHARD_LOCAL_SLICE = 4
RDF_USE_ASSOCIATION_RULES = 8

# every symbol declared in include/rdfind_hip.h
EXPORTED_SYMBOLS = (
    "rdf_ctx_create", "rdf_ctx_destroy", "rdf_last_error", "rdf_version", "rdf_set_triples",
    "rdf_set_triples_device", "rdf_frequent_conditions", "rdf_build_capture_groups", "rdf_discover_cinds",
    "rdf_run", "rdf_cind_count", "rdf_copy_cinds", "rdf_decode_capture", "rdf_binary_key_count",
    "rdf_copy_binary_keys", "rdf_stage_times", "rdf_kernel_times", "rdf_sync",
    "rdf_copy_cinds_range", "rdf_cind_checksum", "rdf_last_stats", "rdf_shard_begin", "rdf_shard_step",
    "rdf_shard_export", "rdf_shard_import", "rdf_set_dictionary", "rdf_format_size", "rdf_format_cinds",
    "rdf_distinct_triples", "rdf_copy_triples", "rdf_parse_ntriples", "rdf_copy_terms",
    "rdf_set_dictionary_parsed", "rdf_device_bytes", "rdf_copy_cinds_decoded", "rdf_result_sizes",
    "rdf_copy_result_raw", "rdf_association_rules", "rdf_copy_association_rules", "rdf_get_result_layout",
    "rdf_copy_result_compact", "rdf_association_rule_count", "rdf_host_alloc", "rdf_host_free",
    "rdf_discover_cinds_paged", "rdf_next_page", "rdf_shard_parse_begin", "rdf_shard_dictionary_begin", "rdf_num_terms",
    "rdf_dictionary_terms", "rdf_copy_result_refs", "rdf_release_scratch", "rdf_set_handover",
    "rdf_copy_result_refs_async", "rdf_handover_wait", "rdf_set_result_form", "rdf_heavy_chunk_count",
    "rdf_copy_result_heavy", "rdf_parse_begin", "rdf_parse_chunk", "rdf_parse_end", "rdf_copy_term_heap",
    "rdf_rewrite_terms", "rdf_condition_histogram", "rdf_join_histogram", "rdf_copy_histogram", "rdf_count_literals",
    "rdf_cind_stats_begin", "rdf_cind_stats_add", "rdf_cind_stats_end", "rdf_cind_histogram", "rdf_copy_top_refs",
    "rdf_select_cinds", "rdf_selected_count", "rdf_copy_selected_decoded", "rdf_format_selected_size",
    "rdf_format_selected", "rdf_find_terms", "rdf_check_cinds", "rdf_copy_check_rows", "rdf_copy_check_examples",
)
# CIND check (rdf_check_cinds): a term the dictionary lacks, the most examples per candidate
RDF_CHK_ABSENT = 0xFFFFFFFE
RDF_CHK_MAX_EXAMPLES = 16
# result selection (rdf_select_cinds): wildcard value, patterns per side, flags; the code index of a pattern's `codes`
# bits numbers the capture codes in ascending order
RDF_SEL_ANY = 0xFFFFFFFF
RDF_SEL_MAX_PATTERNS = 256
RDF_SEL_COUNT_ONLY = 1
SEL_CODES = (10, 12, 14, 17, 20, 21, 33, 34, 35)
SEL_ALL_CODES = 0x1FF
# rdf_hist_row kinds of the result statistics (rdf_cind_histogram)
RDF_CS_SHAPE, RDF_CS_SUPPORT, RDF_CS_REFS, RDF_CS_INDEGREE = 1, 2, 3, 4
RDF_JH_NO_FIS = 1
RDF_RW_ASCIIFY = 1
RDF_NT_TABS = 1

# the test-only entry points of rdfind_amd/csrc/test_abi.h (not part of the product ABI)
TEST_SYMBOLS = ("rdf_test_scan", "rdf_test_scan_batch", "rdf_test_radix", "rdf_test_radix_passes",
                "rdf_test_radix_segments", "rdf_test_paths", "rdf_test_rewrite_form", "rdf_test_cind_stats_times",
                "rdf_test_fc_trace", "rdf_test_fc_report", "rdf_test_copy_frequent_unary", "rdf_test_unary_lookup",
                "rdf_test_record_tile", "rdf_test_keep_records", "rdf_test_group_build", "rdf_test_shard_report",
                "rdf_test_radix_pairs", "rdf_test_group_kv")
REWRITE_FORMS = {0: None, 1: "lds", 2: "global"}
SCAN_U32_U32, SCAN_U32_U64, SCAN_U64_U64 = range(3)
SCAN_DTYPES = {SCAN_U32_U32: (np.uint32, np.uint32), SCAN_U32_U64: (np.uint32, np.uint64),
               SCAN_U64_U64: (np.uint64, np.uint64)}
RADIX_SORT_BITS, RADIX_SORT_DROP, RADIX_PART_HASHED, RADIX_PART_U32 = range(4)
K1_FORMS = {0: None, 1: "partitioned", 2: "radix", 3: "atomic"}
K2_FORMS = {0: None, 1: "plain", 2: "split", 3: "radix", 4: "atomic"}
K3_FORMS = {0: None, 1: "onepass", 2: "twopass"}
GROUP_FORMS = {0: None, 1: "u64", 2: "kv"}

# rdf_exchange ops (sharded mode, include/rdfind_hip.h)
X_DONE, X_ALLREDUCE_SUM_U32, X_ALLREDUCE_SUM_U64, X_ALLREDUCE_MIN_U64, X_ALLGATHERV_U64, X_ALLTOALLV_U64 = range(6)
MAX_RANKS = 64

# RDF_T_* kernel-family timers (include/rdfind_hip.h)
TIMER_NAMES = ("unary", "binary", "emit", "sort", "support", "groups", "heavymask", "pivot", "light", "esort",
               "hcount", "rules", "hwrite", "class", "cemit")


class FcStats(ctypes.Structure):
    _fields_ = [("min_support", ctypes.c_uint32), ("n_ar_suppressed", ctypes.c_uint32),
                ("n_frequent_unary", ctypes.c_uint64 * 3), ("n_binary_keys", ctypes.c_uint64),
                ("n_frequent_binary", ctypes.c_uint64)]


class ParseStats(ctypes.Structure):
    """rdf_parse_stats: the totals of a chunked parse (rdf_parse_end)."""
    _fields_ = [("n_triples", ctypes.c_uint64), ("n_terms", ctypes.c_uint64), ("n_lines", ctypes.c_uint64),
                ("n_chunks", ctypes.c_uint64), ("heap_bytes", ctypes.c_uint64), ("table_slots", ctypes.c_uint64),
                ("n_table_growths", ctypes.c_uint64), ("ms", ctypes.c_float)]


class RewriteStats(ctypes.Structure):
    """rdf_rewrite_stats (rdf_rewrite_terms)."""
    _fields_ = [("n_terms_before", ctypes.c_uint64), ("n_terms_after", ctypes.c_uint64), ("n_changed", ctypes.c_uint64),
                ("heap_bytes", ctypes.c_uint64), ("ms", ctypes.c_float)]


class GroupStats(ctypes.Structure):
    _fields_ = [("n_records", ctypes.c_uint64), ("n_frequent_records", ctypes.c_uint64),
                ("n_groups", ctypes.c_uint64), ("n_captures", ctypes.c_uint64),
                ("n_unary_captures", ctypes.c_uint64), ("n_heavy_groups", ctypes.c_uint64),
                ("heavy_threshold", ctypes.c_uint64), ("n_sorted_records", ctypes.c_uint64),
                ("n_join_ranges", ctypes.c_uint64), ("n_ranges_kept", ctypes.c_uint64)]


class CindStats(ctypes.Structure):
    _fields_ = [("n_cinds", ctypes.c_uint64), ("n_explicit_raw", ctypes.c_uint64),
                ("n_light_chunks", ctypes.c_uint64), ("n_heavy_chunks", ctypes.c_uint64),
                ("ms_pivot", ctypes.c_float), ("ms_light", ctypes.c_float), ("ms_rules", ctypes.c_float),
                ("ms_heavy", ctypes.c_float), ("n_heavy_candidates", ctypes.c_uint64),
                ("n_class_members", ctypes.c_uint64), ("n_classes", ctypes.c_uint64), ("n_class_cinds", ctypes.c_uint64),
                ("n_light_candidates", ctypes.c_uint64), ("n_light_entries", ctypes.c_uint64)]


class PathReport(ctypes.Structure):
    """rdf_test_path_report (rdfind_amd/csrc/test_abi.h)."""
    _fields_ = [("k1_form", ctypes.c_uint32), ("k2_form", ctypes.c_uint32), ("k3_form", ctypes.c_uint32),
                ("dense_on", ctypes.c_uint32), ("light_stage", ctypes.c_uint32), ("light_hiocc", ctypes.c_uint32),
                ("n_dense", ctypes.c_uint64), ("n_dense_eligible", ctypes.c_uint64),
                ("n_dedup_members", ctypes.c_uint64),
                ("n_light_items", ctypes.c_uint64), ("n_packed_octets", ctypes.c_uint64),
                ("n_mseg_chunks", ctypes.c_uint64), ("n_multi_items", ctypes.c_uint64),
                ("n_light_survivors", ctypes.c_uint64),
                ("light_npx", ctypes.c_uint32), ("packed_npx", ctypes.c_uint32), ("light_ordered", ctypes.c_uint32),
                ("light_side", ctypes.c_uint32), ("light_two_pass", ctypes.c_uint32), ("sig_on", ctypes.c_uint32),
                ("piv2_on", ctypes.c_uint32), ("k3_hist", ctypes.c_uint32),
                ("hclassed", ctypes.c_uint32), ("n_class_chunks", ctypes.c_uint64), ("n_emit_tiles", ctypes.c_uint64),
                ("max_class_list", ctypes.c_uint64), ("n_multi_seg_lists", ctypes.c_uint64),
                ("k3_key_items", ctypes.c_uint64), ("k3_suppressed", ctypes.c_uint64),
                ("group_form", ctypes.c_uint32)]


class FcReport(ctypes.Structure):
    """rdf_test_fc_report_t (rdfind_amd/csrc/test_abi.h)."""
    _fields_ = [("traced", ctypes.c_uint32), ("k1_form", ctypes.c_uint32), ("k1_bits", ctypes.c_uint32),
                ("k2_form", ctypes.c_uint32), ("k2_bits", ctypes.c_uint32), ("k2_sub", ctypes.c_uint32),
                ("k1_buckets", ctypes.c_uint64), ("k1_slices", ctypes.c_uint64), ("k1_multi", ctypes.c_uint64),
                ("k2_buckets", ctypes.c_uint64), ("k2_multi", ctypes.c_uint64), ("k2_spill", ctypes.c_uint64)]


class ShardReport(ctypes.Structure):
    """rdf_test_shard_report_t (rdfind_amd/csrc/test_abi.h)."""
    _fields_ = ([("rank", ctypes.c_uint32), ("nranks", ctypes.c_uint32)]
                + [(k, ctypes.c_uint64) for k in (
                    "holder_survivors", "routed_words", "reports_sent", "verify_sent", "reports_received",
                    "verify_received", "verify_kept", "owner_reports", "owner_kept", "unary_own", "binary_own",
                    "unary_gathered", "n_classes", "n_class_members", "n_class_items", "n_list_entries", "hot_entries",
                    "heavy_base", "heavy_columns")]
                + [("have_max_verify", ctypes.c_uint32), ("max_verify_per_dep", ctypes.c_uint64)])


class ResultLayout(ctypes.Structure):
    _fields_ = [(k, ctypes.c_uint64) for k in ("n_cinds", "n_refs", "n_runs", "n_lists", "n_list_refs", "n_members",
                                                "n_captures")]


# rdf_copy_result_compact parts: name -> (dtype, element count from the layout)
COMPACT_PARTS = (("refs", np.uint32, lambda L: L["n_refs"]), ("runoff", np.uint64, lambda L: L["n_runs"] + 1),
                 ("rundep", np.uint32, lambda L: L["n_runs"]), ("list_refs", np.uint32, lambda L: L["n_list_refs"]),
                 ("list_off", np.uint64, lambda L: L["n_lists"] + 1), ("members", np.uint64, lambda L: L["n_members"]),
                 ("capture_ids", np.uint32, lambda L: L["n_captures"]), ("supports", np.uint32, lambda L: L["n_captures"]))


class Exchange(ctypes.Structure):
    _fields_ = [("op", ctypes.c_int32), ("elem_bytes", ctypes.c_uint32), ("count", ctypes.c_uint64),
                ("send_counts", ctypes.c_uint64 * MAX_RANKS)]


class ExchangeRequest:
    """A collective the sharded library asks its caller to perform (see rdfind_amd/distributed.py)."""

    def __init__(self, op: int, elem_bytes: int, count: int, send_counts=None):
        self.op, self.elem_bytes, self.count = op, elem_bytes, count
        self.send_counts = list(send_counts or [])

    def __repr__(self):
        return f"ExchangeRequest(op={self.op}, count={self.count}, send_counts={self.send_counts})"


# rdf_assoc_rule (include/rdfind_hip.h): condition codes s = 1, p = 2, o = 4, term ids, support
RULE_DTYPE = np.dtype([("antecedent_type", "<u4"), ("consequent_type", "<u4"), ("antecedent", "<u4"),
                       ("consequent", "<u4"), ("support", "<u4")])
CIND_DTYPE = np.dtype([("dep", "<u4"), ("ref", "<u4"), ("support", "<u4")])
# rdf_hist_row (include/rdfind_hip.h): one histogram row, sorted by (kind, value)
HIST_DTYPE = np.dtype([("kind", "<u4"), ("value", "<u4"), ("times", "<u8")])
# rdf_top_ref (include/rdfind_hip.h): a referenced capture (external id) and the CINDs that reference it
TOP_DTYPE = np.dtype([("capture", "<u4"), ("pad", "<u4"), ("cinds", "<u8")])
# rdf_cind_row (include/rdfind_hip.h): the reference's Cind shape with term ids
ROW_DTYPE = np.dtype([("dep_capture_type", "<u4"), ("dep_value1", "<u4"), ("dep_value2", "<u4"),
                      ("ref_capture_type", "<u4"), ("ref_value1", "<u4"), ("ref_value2", "<u4"), ("support", "<u4")])



class CapturePattern(ctypes.Structure):
    """rdf_capture_pattern (include/rdfind_hip.h)."""
    _fields_ = [("codes", ctypes.c_uint32), ("value1", ctypes.c_uint32), ("value2", ctypes.c_uint32)]


class CindQuery(ctypes.Structure):
    """rdf_cind_query (include/rdfind_hip.h)."""
    _fields_ = [("dep", ctypes.POINTER(CapturePattern)), ("n_dep", ctypes.c_uint32),
                ("ref", ctypes.POINTER(CapturePattern)), ("n_ref", ctypes.c_uint32),
                ("min_support", ctypes.c_uint32), ("max_support", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


class CheckStats(ctypes.Structure):
    """rdf_check_stats (include/rdfind_hip.h)."""
    _fields_ = [(n, ctypes.c_uint64) for n in ("n_candidates", "n_captures", "n_conditions", "n_records", "n_values",
                                               "n_holding", "n_violated", "n_empty", "n_work_items")] + \
               [(n, ctypes.c_uint32) for n in ("n_batches", "table_in_lds", "lds_slots", "chunk_values")] + \
               [(n, ctypes.c_float) for n in ("ms_match", "ms_sort", "ms_intersect", "ms_total")]


# rdf_check_row
CHECK_DTYPE = np.dtype([("dep_support", "<u4"), ("ref_support", "<u4"), ("overlap", "<u4"), ("n_examples", "<u4")])

_lib = None


RDF_ERR_OOM = -3  # device memory exhausted (include/rdfind_hip.h)


class RdfError(RuntimeError):
    """A failed library call; ``status`` is its rdf_status (e.g. RDF_ERR_OOM), None for load failures."""

    def __init__(self, msg, status=None):
        super().__init__(msg)
        self.status = status


def load():
    """Load librdfind_hip.so (raises if it is missing: the product has no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RdfError(f"{LIB_PATH} not built; run __graft_entry__.build() (HIP extension missing)")
    lib = ctypes.CDLL(LIB_PATH)
    P, u32, u64, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int32
    sig = {
        "rdf_ctx_create": (i32, [ctypes.c_int, ctypes.POINTER(P)]),
        "rdf_ctx_destroy": (None, [P]),
        "rdf_last_error": (ctypes.c_char_p, [P]),
        "rdf_version": (ctypes.c_char_p, []),
        "rdf_set_triples": (i32, [P, P, P, P, u64, u32]),
        "rdf_set_triples_device": (i32, [P, P, P, P, u64, u32]),
        "rdf_distinct_triples": (i32, [P, ctypes.POINTER(u64), ctypes.POINTER(ctypes.c_float)]),
        "rdf_copy_triples": (i32, [P, P, P, P, u64, ctypes.POINTER(u64)]),
        "rdf_parse_ntriples": (i32, [P, ctypes.c_char_p, u64, u32, ctypes.POINTER(u64), ctypes.POINTER(u32),
                                     ctypes.POINTER(ctypes.c_float)]),
        "rdf_copy_terms": (i32, [P, P, P, u64, ctypes.POINTER(u64)]),
        "rdf_set_dictionary_parsed": (i32, [P]),
        "rdf_parse_begin": (i32, [P, u32, u64]),
        "rdf_parse_chunk": (i32, [P, ctypes.c_char_p, u64, ctypes.POINTER(u64), ctypes.POINTER(u32)]),
        "rdf_parse_end": (i32, [P, ctypes.POINTER(ParseStats)]),
        "rdf_copy_term_heap": (i32, [P, P, u64, ctypes.POINTER(u64)]),
        "rdf_rewrite_terms": (i32, [P, u32, ctypes.c_char_p, P, ctypes.c_char_p, P, u32, ctypes.POINTER(RewriteStats)]),
        "rdf_condition_histogram": (i32, [P, ctypes.POINTER(u64), ctypes.POINTER(ctypes.c_float)]),
        "rdf_join_histogram": (i32, [P, ctypes.c_char_p, u32, ctypes.POINTER(u64), ctypes.POINTER(u64),
                                     ctypes.POINTER(ctypes.c_float)]),
        "rdf_copy_histogram": (i32, [P, P, u64, ctypes.POINTER(u64)]),
        "rdf_count_literals": (i32, [P, ctypes.POINTER(u64), ctypes.POINTER(u64)]),
        "rdf_cind_stats_begin": (i32, [P]),
        "rdf_cind_stats_add": (i32, [P]),
        "rdf_cind_stats_end": (i32, [P, ctypes.POINTER(u64), ctypes.POINTER(ctypes.c_float)]),
        "rdf_cind_histogram": (i32, [P, ctypes.POINTER(u64), ctypes.POINTER(ctypes.c_float)]),
        "rdf_copy_top_refs": (i32, [P, P, u64, ctypes.POINTER(u64)]),
        "rdf_select_cinds": (i32, [P, ctypes.POINTER(CindQuery), ctypes.POINTER(u64), ctypes.POINTER(ctypes.c_float)]),
        "rdf_selected_count": (i32, [P, ctypes.POINTER(u64)]),
        "rdf_copy_selected_decoded": (i32, [P, u64, P, u64, ctypes.POINTER(u64)]),
        "rdf_format_selected_size": (i32, [P, u64, u64, ctypes.POINTER(u64)]),
        "rdf_format_selected": (i32, [P, u64, u64, P, u64, ctypes.POINTER(u64)]),
        "rdf_find_terms": (i32, [P, ctypes.c_char_p, P, u32, P]),
        "rdf_check_cinds": (i32, [P, P, u64, u32, ctypes.POINTER(CheckStats)]),
        "rdf_copy_check_rows": (i32, [P, u64, P, u64, ctypes.POINTER(u64)]),
        "rdf_copy_check_examples": (i32, [P, u64, P, u64, ctypes.POINTER(u64)]),
        "rdf_frequent_conditions": (i32, [P, u32, ctypes.POINTER(FcStats)]),
        "rdf_build_capture_groups": (i32, [P, ctypes.c_char_p, ctypes.POINTER(GroupStats)]),
        "rdf_discover_cinds": (i32, [P, u32, ctypes.POINTER(CindStats)]),
        "rdf_run": (i32, [P, u32, ctypes.c_char_p, u32, ctypes.POINTER(FcStats), ctypes.POINTER(GroupStats),
                          ctypes.POINTER(CindStats)]),
        "rdf_cind_count": (i32, [P, ctypes.POINTER(u64)]),
        "rdf_copy_cinds": (i32, [P, P, u64, ctypes.POINTER(u64)]),
        "rdf_decode_capture": (i32, [P, u32, ctypes.POINTER(u32), ctypes.POINTER(u32), ctypes.POINTER(u32)]),
        "rdf_binary_key_count": (i32, [P, ctypes.POINTER(u64)]),
        "rdf_copy_binary_keys": (i32, [P, P, u64]),
        "rdf_stage_times": (i32, [P, ctypes.POINTER(ctypes.c_float)]),
        "rdf_kernel_times": (i32, [P, ctypes.POINTER(ctypes.c_float), ctypes.c_int]),
        "rdf_sync": (i32, [P]),
        "rdf_device_bytes": (i32, [P, ctypes.POINTER(u64)]),
        "rdf_release_scratch": (i32, [P]),
        "rdf_copy_cinds_range": (i32, [P, u64, P, u64, ctypes.POINTER(u64)]),
        "rdf_cind_checksum": (i32, [P, ctypes.POINTER(u64)]),
        "rdf_copy_cinds_decoded": (i32, [P, u64, P, u64, ctypes.POINTER(u64)]),
        "rdf_result_sizes": (i32, [P, ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.POINTER(u64)]),
        "rdf_copy_result_raw": (i32, [P, P, P, P, P, P]),
        "rdf_get_result_layout": (i32, [P, ctypes.POINTER(ResultLayout)]),
        "rdf_copy_result_compact": (i32, [P, P, P, P, P, P, P, P, P]),
        "rdf_copy_result_refs": (i32, [P, u64, u64, P, ctypes.POINTER(u64)]),
        "rdf_copy_result_refs_async": (i32, [P, u64, u64, P, ctypes.POINTER(u64)]),
        "rdf_handover_wait": (i32, [P]),
        "rdf_set_result_form": (i32, [P, u32]),
        "rdf_heavy_chunk_count": (i32, [P, ctypes.POINTER(u64)]),
        "rdf_copy_result_heavy": (i32, [P, P, P, P]),
        "rdf_set_handover": (i32, [P, P, u64, P, P, u64, P, P, u64]),
        "rdf_set_dictionary": (i32, [P, P, u64, P, u64]),
        "rdf_format_size": (i32, [P, u64, u64, ctypes.POINTER(u64)]),
        "rdf_format_cinds": (i32, [P, u64, u64, P, u64, ctypes.POINTER(u64)]),
        "rdf_last_stats": (i32, [P, ctypes.POINTER(FcStats), ctypes.POINTER(GroupStats), ctypes.POINTER(CindStats)]),
        "rdf_association_rules": (i32, [P, ctypes.POINTER(u64)]),
        "rdf_copy_association_rules": (i32, [P, P, u64, ctypes.POINTER(u64)]),
        "rdf_association_rule_count": (i32, [P, ctypes.POINTER(u64)]),
        "rdf_host_alloc": (P, [u64]),
        "rdf_shard_parse_begin": (i32, [P, u32, u32, ctypes.c_char_p, u64, u32, ctypes.POINTER(u64)]),
        "rdf_shard_dictionary_begin": (i32, [P]),
        "rdf_num_terms": (i32, [P, ctypes.POINTER(u32)]),
        "rdf_dictionary_terms": (i32, [P, P, u64, P, u64, P]),
        "rdf_discover_cinds_paged": (i32, [P, u32, u64, ctypes.POINTER(CindStats)]),
        "rdf_next_page": (i32, [P, ctypes.POINTER(u32), ctypes.POINTER(u64), ctypes.POINTER(u64)]),
        "rdf_host_free": (None, [P]),
        "rdf_shard_begin": (i32, [P, u32, u32, u32, ctypes.c_char_p, u32]),
        "rdf_shard_step": (i32, [P, ctypes.POINTER(Exchange)]),
        "rdf_shard_export": (i32, [P, P]),
        "rdf_shard_import": (i32, [P, P, u64]),
        # test_abi.h
        "rdf_test_scan": (i32, [P, ctypes.c_int, P, u64, u32, u32, ctypes.c_int, ctypes.c_int, P, ctypes.POINTER(u64),
                                ctypes.POINTER(u32)]),
        "rdf_test_scan_batch": (i32, [P, ctypes.c_int, P, u64, u32, P, ctypes.POINTER(u32)]),
        "rdf_test_radix": (i32, [P, ctypes.c_int, P, u64, ctypes.c_int, ctypes.c_int, u64, P, ctypes.POINTER(u64),
                                 ctypes.POINTER(u32)]),
        "rdf_test_radix_passes": (ctypes.c_int, [ctypes.c_int]),
        "rdf_test_radix_segments": (i32, [P, P, u64, P, u64, P, u32, ctypes.c_int, ctypes.c_int, ctypes.c_int32, u32, u32,
                                          P, ctypes.POINTER(u64), ctypes.POINTER(u32)]),
        "rdf_test_paths": (i32, [P, ctypes.POINTER(PathReport)]),
        "rdf_test_rewrite_form": (i32, [P, ctypes.POINTER(u32)]),
        "rdf_test_cind_stats_times": (i32, [P, ctypes.POINTER(ctypes.c_float)]),
        "rdf_test_fc_trace": (i32, [P, ctypes.c_int]),
        "rdf_test_fc_report": (i32, [P, ctypes.POINTER(FcReport)]),
        "rdf_test_shard_report": (i32, [P, ctypes.POINTER(ShardReport)]),
        "rdf_test_copy_frequent_unary": (i32, [P, P, u64, ctypes.POINTER(u64), ctypes.POINTER(u64)]),
        "rdf_test_unary_lookup": (i32, [P, P, u64, P, P, ctypes.POINTER(u32)]),
        "rdf_test_record_tile": (ctypes.c_int, []),
        "rdf_test_keep_records": (i32, [P, P, u64, ctypes.c_int, u64, u32, P, ctypes.POINTER(u64), ctypes.POINTER(u32), P, P,
                                        P, ctypes.POINTER(u32)]),
        "rdf_test_group_build": (i32, [P, P, u64, u32, u64, u32, ctypes.POINTER(u64), P, P, P, ctypes.POINTER(u32)]),
        "rdf_test_radix_pairs": (i32, [P, P, P, u64, ctypes.c_int, ctypes.c_int, P, P, ctypes.POINTER(u32)]),
        "rdf_test_group_kv": (i32, [P, P, u64, ctypes.c_int, u64, u32, u32, P, ctypes.POINTER(u64), ctypes.POINTER(u32), P, P,
                                    ctypes.POINTER(u64), P, P, P, ctypes.POINTER(u32)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name, None) if name in TEST_SYMBOLS else getattr(lib, name)
        if fn is None:  # a dev variant (RDFIND_HIP_LIB) built before the test entry points existed
            continue
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


class PinnedBuffer:
    """Page-locked host memory from the library (rdf_host_alloc), as a numpy array view; freed with the object."""

    def __init__(self, count: int, dtype):
        self.lib = load()
        self.nbytes = max(int(count), 1) * np.dtype(dtype).itemsize
        self.ptr = self.lib.rdf_host_alloc(self.nbytes)
        if not self.ptr:
            raise RdfError(f"rdf_host_alloc({self.nbytes}) failed")
        self.array = np.ctypeslib.as_array((ctypes.c_uint8 * self.nbytes).from_address(self.ptr)).view(dtype)

    def __del__(self):
        if getattr(self, "ptr", None):
            self.lib.rdf_host_free(self.ptr)
            self.ptr = None


def _struct_dict(st):
    out = {}
    for name, _ in st._fields_:
        val = getattr(st, name)
        out[name] = list(val) if isinstance(val, ctypes.Array) else val
    return out


class Context:
    """One GPU context (one per device / rank), mirroring one Flink task instance."""

    def __init__(self, device: int = 0):
        self.lib = load()
        self.ptr = ctypes.c_void_p()
        rc = self.lib.rdf_ctx_create(device, ctypes.byref(self.ptr))
        if rc != 0:
            raise RdfError(f"rdf_ctx_create(device={device}) failed ({rc}): is a GPU visible?")
        self.num_terms = 0
        self.hist_rows = self.join_lines = 0
        self.fc = self.groups = self.cinds = None

    def close(self):
        if self.ptr:
            self.lib.rdf_ctx_destroy(self.ptr)
            self.ptr = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _test_fn(self, name):
        fn = getattr(self.lib, name, None)
        if fn is None:
            raise RdfError(f"{LIB_PATH} has no {name}: built before the test entry points (csrc/test_abi.h); rebuild it")
        return fn

    def _check(self, rc, what):
        if rc != 0:
            msg = self.lib.rdf_last_error(self.ptr)
            raise RdfError(f"{what} failed ({rc}): {msg.decode() if msg else ''}", rc)

    # -- stages ------------------------------------------------------------------------------
    def set_triples(self, s, p, o, num_terms: int):
        s = np.ascontiguousarray(s, dtype=np.uint32)
        p = np.ascontiguousarray(p, dtype=np.uint32)
        o = np.ascontiguousarray(o, dtype=np.uint32)
        if not (s.shape == p.shape == o.shape):
            raise ValueError("s, p, o must have the same length")
        self._check(self.lib.rdf_set_triples(self.ptr, s.ctypes.data, p.ctypes.data, o.ctypes.data, s.shape[0],
                                             num_terms), "rdf_set_triples")
        self.num_terms = num_terms

    def set_triples_device(self, s_ptr: int, p_ptr: int, o_ptr: int, n: int, num_terms: int):
        self._check(self.lib.rdf_set_triples_device(self.ptr, s_ptr, p_ptr, o_ptr, n, num_terms),
                    "rdf_set_triples_device")
        self.num_terms = num_terms

    def distinct_triples(self):
        """--distinct-triples on the resident triples (RDFind.scala:284-287); returns (kept, device ms)."""
        n = ctypes.c_uint64()
        ms = ctypes.c_float()
        self._check(self.lib.rdf_distinct_triples(self.ptr, ctypes.byref(n), ctypes.byref(ms)),
                    "rdf_distinct_triples")
        return int(n.value), float(ms.value)

    def parse_ntriples(self, data: bytes, tabs: bool = False):
        """N-Triples text -> resident dictionary-encoded triples, on the device (rdf_parse_ntriples).
        Returns (n_triples, num_terms, device ms) and keeps ``data`` for :meth:`parsed_terms`."""
        n, v, ms = ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_float()
        self._check(self.lib.rdf_parse_ntriples(self.ptr, data, len(data), RDF_NT_TABS if tabs else 0,
                                                ctypes.byref(n), ctypes.byref(v), ctypes.byref(ms)),
                    "rdf_parse_ntriples")
        self.num_terms = int(v.value)
        self._parsed = data
        return int(n.value), int(v.value), float(ms.value)

    def parse_begin(self, tabs: bool = False, reserve_triples: int = 0):
        """Opens a chunked parse (rdf_parse_begin): the input follows in :meth:`parse_chunk` calls, and the dictionary
        stays on the device between them.  ``reserve_triples`` allocates the triple arrays up front."""
        self._check(self.lib.rdf_parse_begin(self.ptr, RDF_NT_TABS if tabs else 0, reserve_triples), "rdf_parse_begin")
        self._parsed = b""

    def parse_chunk(self, data: bytes):
        """One window of whole lines (rdf_parse_chunk); returns the totals so far, (n_triples, num_terms)."""
        n, v = ctypes.c_uint64(), ctypes.c_uint32()
        self._check(self.lib.rdf_parse_chunk(self.ptr, data, len(data), ctypes.byref(n), ctypes.byref(v)),
                    "rdf_parse_chunk")
        return int(n.value), int(v.value)

    def parse_end(self) -> dict:
        """Closes the chunked parse (rdf_parse_end): its triples become the resident input.  Returns the stats
        (n_triples, n_terms, n_lines, n_chunks, heap_bytes, table_slots, n_table_growths, ms).  The offsets of
        :meth:`parsed_terms` then point into the term heap, which that call fetches (rdf_copy_term_heap)."""
        st = ParseStats()
        self._check(self.lib.rdf_parse_end(self.ptr, ctypes.byref(st)), "rdf_parse_end")
        self.num_terms = int(st.n_terms)
        self._parsed = None  # the term heap, fetched when parsed_terms asks for it
        return {k: (float(st.ms) if k == "ms" else int(getattr(st, k))) for k, _ in ParseStats._fields_}

    def parse_windows(self, windows, tabs: bool = False):
        """A chunked parse of an iterable of ``bytes`` windows (e.g. ``ntriples.iter_windows``); returns
        (n_triples, num_terms, device ms) like :meth:`parse_ntriples`."""
        self.parse_begin(tabs=tabs)
        for w in windows:
            self.parse_chunk(w)
        st = self.parse_end()
        return st["n_triples"], st["n_terms"], st["ms"]

    def parsed_terms(self):
        """The device dictionary of the last parse as (heap bytes, uint64 offsets[V + 1]): term i is
        heap[offsets[i]:offsets[i + 1]] (UTF-8)."""
        v = self.num_terms
        off, ln = np.empty(v, np.uint64), np.empty(v, np.uint32)
        got = ctypes.c_uint64()
        self._check(self.lib.rdf_copy_terms(self.ptr, off.ctypes.data, ln.ctypes.data, v, ctypes.byref(got)),
                    "rdf_copy_terms")
        ln64 = ln.astype(np.int64)
        offsets = np.zeros(v + 1, np.uint64)
        np.cumsum(ln64, out=offsets[1:])
        if self._parsed is None:
            size = ctypes.c_uint64()
            self._check(self.lib.rdf_copy_term_heap(self.ptr, None, 0, ctypes.byref(size)), "rdf_copy_term_heap")
            heap = np.empty(int(size.value), np.uint8)
            self._check(self.lib.rdf_copy_term_heap(self.ptr, heap.ctypes.data, heap.shape[0], ctypes.byref(size)),
                        "rdf_copy_term_heap")
            self._parsed = heap.tobytes()
        src = np.frombuffer(self._parsed, np.uint8)
        pos = np.arange(int(offsets[-1]), dtype=np.int64) + np.repeat(off.astype(np.int64) - offsets[:-1].astype(np.int64),
                                                                       ln64)
        return src[pos].tobytes(), offsets

    def rewrite_terms(self, prefixes=(), asciify: bool = False) -> dict:
        """--asciify-triples and/or --prefixes on the device dictionary of the last parse (rdf_rewrite_terms): every
        distinct term becomes shorten(asciify(term)), equal results share one id, and s / p / o are remapped in HBM.
        ``prefixes`` is [(prefix, url)] as ``ntriples.read_prefixes`` returns it; the keys ``<url`` and the values
        ``prefix:`` are formed here (ShortenUrls.PrefixTrieCreator).  Returns the stats (n_terms_before, n_terms_after,
        n_changed, heap_bytes, ms); :meth:`parsed_terms` fetches the new dictionary afterwards."""
        keys = [("<" + url).encode("utf-8") for _, url in prefixes]
        vals = [(prefix + ":").encode("utf-8") for prefix, _ in prefixes]
        koff, voff = np.zeros(len(keys) + 1, np.uint64), np.zeros(len(keys) + 1, np.uint64)
        np.cumsum([len(k) for k in keys], out=koff[1:])
        np.cumsum([len(v) for v in vals], out=voff[1:])
        st = RewriteStats()
        self._check(self.lib.rdf_rewrite_terms(self.ptr, RDF_RW_ASCIIFY if asciify else 0, b"".join(keys), koff.ctypes.data,
                                               b"".join(vals), voff.ctypes.data, len(keys), ctypes.byref(st)),
                    "rdf_rewrite_terms")
        self.num_terms = int(st.n_terms_after)
        self._parsed = None  # the new term heap, fetched when parsed_terms asks for it
        return {k: (float(st.ms) if k == "ms" else int(getattr(st, k))) for k, _ in RewriteStats._fields_}

    def rewrite_form(self):
        """Which key lookup the last :meth:`rewrite_terms` ran (rdf_test_rewrite_form): "lds", "global" or None."""
        v = ctypes.c_uint32()
        self._check(self._test_fn("rdf_test_rewrite_form")(self.ptr, ctypes.byref(v)), "rdf_test_rewrite_form")
        return REWRITE_FORMS[int(v.value)]

    def set_dictionary_parsed(self):
        """The last parse's dictionary becomes the formatting dictionary, in HBM (rdf_set_dictionary_parsed)."""
        self._check(self.lib.rdf_set_dictionary_parsed(self.ptr), "rdf_set_dictionary_parsed")

    def set_dictionary_heap(self, heap: bytes, offsets):
        """rdf_set_dictionary from a ready heap + offsets (e.g. :meth:`parsed_terms`)."""
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        buf = ctypes.create_string_buffer(heap, max(len(heap), 1))
        self._check(self.lib.rdf_set_dictionary(self.ptr, buf, len(heap), offsets.ctypes.data, offsets.shape[0] - 1),
                    "rdf_set_dictionary")

    def copy_triples(self, n: int):
        """The resident triples as three uint32 arrays (the first n of them)."""
        s, p, o = (np.empty(n, np.uint32) for _ in range(3))
        got = ctypes.c_uint64()
        self._check(self.lib.rdf_copy_triples(self.ptr, s.ctypes.data, p.ctypes.data, o.ctypes.data, n,
                                              ctypes.byref(got)), "rdf_copy_triples")
        return s[:got.value], p[:got.value], o[:got.value]

    # -- dataset statistics ----------------------------------------------------------------------
    def copy_histogram(self, n_rows: int | None = None) -> np.ndarray:
        """The rows of the last histogram call (rdf_copy_histogram), HIST_DTYPE, sorted by (kind, value)."""
        cap = self.hist_rows if n_rows is None else n_rows
        out = np.empty(cap, dtype=HIST_DTYPE)
        got = ctypes.c_uint64()
        self._check(self.lib.rdf_copy_histogram(self.ptr, out.ctypes.data, cap, ctypes.byref(got)), "rdf_copy_histogram")
        return out[: got.value]

    def condition_histogram(self) -> np.ndarray:
        """CountConditions on the resident triples (rdf_condition_histogram): rows (kind, value, times) = ``times``
        distinct conditions of ``kind`` (1 s, 2 p, 4 o, 3 sp, 5 so, 6 po; 0: all six together) occur in exactly
        ``value`` triples.  The device time is left in ``self.hist_ms``."""
        n, ms = ctypes.c_uint64(), ctypes.c_float()
        self._check(self.lib.rdf_condition_histogram(self.ptr, ctypes.byref(n), ctypes.byref(ms)),
                    "rdf_condition_histogram")
        self.hist_rows, self.hist_ms = int(n.value), float(ms.value)
        return self.copy_histogram()

    def join_histogram(self, projection: str = "spo", use_fis: bool = True) -> np.ndarray:
        """--create-join-histogram (rdf_join_histogram): rows (0, k, t) = t join lines of exactly k distinct conditions.
        ``use_fis``: with the frequent conditions of the last :meth:`frequent_conditions` (and the rules of
        :meth:`association_rules` if it ran); otherwise every value passes (RDF_JH_NO_FIS, resident triples only).
        The line count is left in ``self.join_lines``, the device time in ``self.hist_ms``."""
        lines, n, ms = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_float()
        self._check(self.lib.rdf_join_histogram(self.ptr, projection.encode(), 0 if use_fis else RDF_JH_NO_FIS,
                                                ctypes.byref(lines), ctypes.byref(n), ctypes.byref(ms)),
                    "rdf_join_histogram")
        self.join_lines, self.hist_rows, self.hist_ms = int(lines.value), int(n.value), float(ms.value)
        return self.copy_histogram()

    def count_literals(self):
        """CountDistinctValues on the device dictionary of the last parse (rdf_count_literals): (literals, terms);
        terms - literals are the "URLs"."""
        lit, terms = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self.lib.rdf_count_literals(self.ptr, ctypes.byref(lit), ctypes.byref(terms)), "rdf_count_literals")
        return int(lit.value), int(terms.value)

    # -- result statistics -----------------------------------------------------------------------
    def cind_stats_begin(self):
        """rdf_cind_stats_begin: zeroes the accumulators of the result statistics (after a discovery, or a prepared
        paged one)."""
        self._check(self.lib.rdf_cind_stats_begin(self.ptr), "rdf_cind_stats_begin")

    def cind_stats_add(self):
        """rdf_cind_stats_add: adds the current result (the whole result, or the current page) to the statistics."""
        self._check(self.lib.rdf_cind_stats_add(self.ptr), "rdf_cind_stats_add")

    def cind_stats_end(self) -> np.ndarray:
        """rdf_cind_stats_end: the rows (kind, value, times) of the accumulated statistics, HIST_DTYPE sorted by
        (kind, value): kind 1 value = dep_code << 8 | ref_code, times = CINDs; 2 value = support, times = CINDs of
        dependents with it; 3 value = r, times = dependents with r refs; 4 value = d, times = captures referenced by d
        CINDs.  The summed device time of the add calls and this one is left in ``self.hist_ms``."""
        n, ms = ctypes.c_uint64(), ctypes.c_float()
        self._check(self.lib.rdf_cind_stats_end(self.ptr, ctypes.byref(n), ctypes.byref(ms)), "rdf_cind_stats_end")
        self.hist_rows, self.hist_ms = int(n.value), float(ms.value)
        return self.copy_histogram()

    def cind_histogram(self) -> np.ndarray:
        """rdf_cind_histogram: begin + add + end on the current result; rows as :meth:`cind_stats_end`, the device time
        in ``self.hist_ms``.  A pending class part is counted unexpanded and stays pending."""
        n, ms = ctypes.c_uint64(), ctypes.c_float()
        self._check(self.lib.rdf_cind_histogram(self.ptr, ctypes.byref(n), ctypes.byref(ms)), "rdf_cind_histogram")
        self.hist_rows, self.hist_ms = int(n.value), float(ms.value)
        return self.copy_histogram()

    def top_refs(self, k: int) -> np.ndarray:
        """rdf_copy_top_refs: the k most referenced captures of the last statistics as (capture, cinds) rows
        (TOP_DTYPE; external capture ids), descending by cinds, ties by ascending capture id."""
        out = np.zeros(max(int(k), 0), dtype=TOP_DTYPE)
        got = ctypes.c_uint64()
        self._check(self.lib.rdf_copy_top_refs(self.ptr, out.ctypes.data, out.shape[0], ctypes.byref(got)),
                    "rdf_copy_top_refs")
        return out[: got.value][["capture", "cinds"]]

    # -- result selection ---------------------------------------------------------------------
    def find_terms(self, terms) -> np.ndarray:
        """rdf_find_terms: the ids of the given strings in the formatting dictionary (uint32; 0xFFFFFFFF = absent),
        looked up on the device, RDF_SEL_MAX_PATTERNS * 2 per call."""
        enc = [t.encode("utf-8") if isinstance(t, str) else bytes(t) for t in terms]
        ids = np.empty(len(enc), dtype=np.uint32)
        step = 2 * RDF_SEL_MAX_PATTERNS
        for b in range(0, len(enc), step):
            part = enc[b:b + step]
            heap = b"".join(part)
            offsets = np.zeros(len(part) + 1, dtype=np.uint64)
            np.cumsum(np.fromiter((len(e) for e in part), dtype=np.uint64, count=len(part)), out=offsets[1:])
            buf = ctypes.create_string_buffer(heap, max(len(heap), 1))
            self._check(self.lib.rdf_find_terms(self.ptr, buf, offsets.ctypes.data, len(part), ids[b:].ctypes.data),
                        "rdf_find_terms")
        return ids

    @staticmethod
    def _patterns(pats):
        arr = (CapturePattern * max(len(pats), 1))()
        for i, (cd, v1, v2) in enumerate(pats):
            arr[i] = CapturePattern(int(cd), int(v1), int(v2))
        return arr

    def select_cinds(self, dep=(), ref=(), min_support=0, max_support=0xFFFFFFFF, count_only=False) -> int:
        """rdf_select_cinds on the current result (or page): the CINDs whose dependent matches any of `dep`, whose
        referenced capture matches any of `ref` (patterns (codes, value1, value2); an empty side admits every capture)
        and whose support lies in [min_support, max_support].  Returns their number and, unless `count_only`, leaves
        them as a view for selected_decoded / format_selected; the device time is in ``last_select_ms``."""
        dep, ref = list(dep), list(ref)
        da, ra = self._patterns(dep), self._patterns(ref)
        q = CindQuery(da, len(dep), ra, len(ref), min_support, max_support, RDF_SEL_COUNT_ONLY if count_only else 0)
        n, ms = ctypes.c_uint64(), ctypes.c_float()
        self._check(self.lib.rdf_select_cinds(self.ptr, ctypes.byref(q), ctypes.byref(n), ctypes.byref(ms)),
                    "rdf_select_cinds")
        self.last_select_ms = float(ms.value)
        return int(n.value)

    def selected_count(self) -> int:
        n = ctypes.c_uint64()
        self._check(self.lib.rdf_selected_count(self.ptr, ctypes.byref(n)), "rdf_selected_count")
        return int(n.value)

    def selected_decoded(self, offset: int = 0, count: int | None = None) -> np.ndarray:
        """Rows [offset, offset + count) of the selection view, Cind-shaped (ROW_DTYPE), decoded on the device."""
        if count is None:
            count = max(self.selected_count() - offset, 0)
        out = np.empty(count, dtype=ROW_DTYPE)
        copied = ctypes.c_uint64()
        self._check(self.lib.rdf_copy_selected_decoded(self.ptr, offset, out.ctypes.data, count, ctypes.byref(copied)),
                    "rdf_copy_selected_decoded")
        return out[: copied.value]

    def format_selected_array(self, offset=0, count=None) -> np.ndarray:
        """Cind.toString lines of rows [offset, offset + count) of the selection view, as format_array."""
        if count is None:
            count = max(self.selected_count() - offset, 0)
        need = ctypes.c_uint64()
        self._check(self.lib.rdf_format_selected_size(self.ptr, offset, count, ctypes.byref(need)),
                    "rdf_format_selected_size")
        out = np.empty(max(need.value, 1), dtype=np.uint8)
        got = ctypes.c_uint64()
        self._check(self.lib.rdf_format_selected(self.ptr, offset, count, out.ctypes.data, need.value, ctypes.byref(got)),
                    "rdf_format_selected")
        return out[: got.value]

    def format_selected(self, offset=0, count=None) -> bytes:
        """As format_selected_array, as bytes."""
        return self.format_selected_array(offset, count).tobytes()

    # -- CIND check ---------------------------------------------------------------------------
    def check_cinds(self, cands, examples: int = 0):
        """rdf_check_cinds: `cands` is an (M, 6) uint32 array [dep_code, d1, d2, ref_code, r1, r2] (value2 = 0xFFFFFFFF
        for a unary capture, RDF_CHK_ABSENT for a term the dictionary lacks).  Returns the rows (CHECK_DTYPE) and the
        (M, examples) violating term ids, ascending and padded with 0xFFFFFFFF; ``last_check`` holds the stats."""
        cands = np.ascontiguousarray(cands, dtype=np.uint32).reshape(-1, 6)
        m = cands.shape[0]
        st = CheckStats()
        self._check(self.lib.rdf_check_cinds(self.ptr, cands.ctypes.data if m else None, m, int(examples), ctypes.byref(st)),
                    "rdf_check_cinds")
        self.last_check = _struct_dict(st)
        return self.check_rows(0, m), self.check_examples(0, m, int(examples))

    def check_rows(self, offset: int, count: int) -> np.ndarray:
        rows = np.empty(count, dtype=CHECK_DTYPE)
        got = ctypes.c_uint64()
        self._check(self.lib.rdf_copy_check_rows(self.ptr, offset, rows.ctypes.data, count, ctypes.byref(got)),
                    "rdf_copy_check_rows")
        return rows[: got.value]

    def check_examples(self, offset: int, count: int, examples: int) -> np.ndarray:
        ex = np.empty((count, examples), dtype=np.uint32)
        got = ctypes.c_uint64()
        self._check(self.lib.rdf_copy_check_examples(self.ptr, offset, ex.ctypes.data, count, ctypes.byref(got)),
                    "rdf_copy_check_examples")
        return ex[: got.value]

    def cind_stats_times(self):
        """(explicit, class, end) device ms of the last result statistics (rdf_test_cind_stats_times)."""
        arr = (ctypes.c_float * 3)()
        self._check(self._test_fn("rdf_test_cind_stats_times")(self.ptr, arr), "rdf_test_cind_stats_times")
        return list(arr)

    def frequent_conditions(self, min_support: int):
        st = FcStats()
        self._check(self.lib.rdf_frequent_conditions(self.ptr, min_support, ctypes.byref(st)),
                    "rdf_frequent_conditions")
        self.fc = _struct_dict(st)
        return self.fc

    def association_rules(self) -> int:
        """--use-ars after frequent_conditions (rdf_association_rules); returns the number of rules."""
        n = ctypes.c_uint64()
        self._check(self.lib.rdf_association_rules(self.ptr, ctypes.byref(n)), "rdf_association_rules")
        self.n_rules = int(n.value)
        return self.n_rules

    def copy_association_rules(self) -> np.ndarray:
        """The rules of the last rdf_association_rules (or sharded run with use_ars), RULE_DTYPE rows."""
        n = ctypes.c_uint64()
        self._check(self.lib.rdf_association_rule_count(self.ptr, ctypes.byref(n)), "rdf_association_rule_count")
        self.n_rules = int(n.value)
        out = np.empty(self.n_rules, dtype=RULE_DTYPE)
        got = ctypes.c_uint64()
        self._check(self.lib.rdf_copy_association_rules(self.ptr, out.ctypes.data, len(out), ctypes.byref(got)),
                    "rdf_copy_association_rules")
        return out[:got.value]

    def build_capture_groups(self, projection: str = "spo"):
        st = GroupStats()
        self._check(self.lib.rdf_build_capture_groups(self.ptr, projection.encode(), ctypes.byref(st)),
                    "rdf_build_capture_groups")
        self.groups = _struct_dict(st)
        return self.groups

    def discover_cinds(self, clean_implied: bool = True, traversal_strategy: int = 1):
        flags = (RDF_CLEAN_IMPLIED if clean_implied else 0) | (RDF_STRATEGY_ALL_AT_ONCE if traversal_strategy == 0 else 0)
        st = CindStats()
        self._check(self.lib.rdf_discover_cinds(self.ptr, flags, ctypes.byref(st)), "rdf_discover_cinds")
        self.cinds = _struct_dict(st)
        return self.cinds

    def discover_cinds_paged(self, clean_implied: bool = True, traversal_strategy: int = 1, page_bytes: int = 0):
        """rdf_discover_cinds_paged: prepares a paged run (page_bytes of working memory per page, 0 = automatic)."""
        flags = (RDF_CLEAN_IMPLIED if clean_implied else 0) | (RDF_STRATEGY_ALL_AT_ONCE if traversal_strategy == 0 else 0)
        st = CindStats()
        self._check(self.lib.rdf_discover_cinds_paged(self.ptr, flags, page_bytes, ctypes.byref(st)),
                    "rdf_discover_cinds_paged")
        self.cinds = _struct_dict(st)
        return self.cinds

    def next_page(self):
        """rdf_next_page: the next page becomes the current result; returns (first_dep, end_dep), or None when done."""
        done, d0, d1 = ctypes.c_uint32(), ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self.lib.rdf_next_page(self.ptr, ctypes.byref(done), ctypes.byref(d0), ctypes.byref(d1)),
                    "rdf_next_page")
        return None if done.value else (int(d0.value), int(d1.value))

    def pages(self, clean_implied: bool = True, traversal_strategy: int = 1, page_bytes: int = 0):
        """Iterates a paged run: yields (first_dep, end_dep) with each page as the current result."""
        self.discover_cinds_paged(clean_implied, traversal_strategy, page_bytes)
        self._pages = 0
        while True:
            r = self.next_page()
            if r is None:
                return
            self._pages += 1
            yield r

    def run(self, min_support=10, projection="spo", clean_implied=True, traversal_strategy=1, use_ars=False):
        self.frequent_conditions(min_support)
        if use_ars:
            self.association_rules()
        self.build_capture_groups(projection)
        return self.discover_cinds(clean_implied, traversal_strategy)

    def sync(self):
        self._check(self.lib.rdf_sync(self.ptr), "rdf_sync")

    def device_bytes(self) -> int:
        """HBM bytes the context holds (rdf_device_bytes)."""
        v = ctypes.c_uint64()
        self._check(self.lib.rdf_device_bytes(self.ptr, ctypes.byref(v)), "rdf_device_bytes")
        return int(v.value)

    def release_scratch(self):
        """rdf_release_scratch: frees every per-run buffer (triples and dictionary stay); frequent_conditions next."""
        self._check(self.lib.rdf_release_scratch(self.ptr), "rdf_release_scratch")

    def last_stats(self):
        fc, gs, cs = FcStats(), GroupStats(), CindStats()
        self._check(self.lib.rdf_last_stats(self.ptr, ctypes.byref(fc), ctypes.byref(gs), ctypes.byref(cs)),
                    "rdf_last_stats")
        self.fc, self.groups, self.cinds = _struct_dict(fc), _struct_dict(gs), _struct_dict(cs)
        return self.groups, self.cinds

    # -- test-only entry points (rdfind_amd/csrc/test_abi.h) ------------------------------------
    # The primitives run on caller data in buffers fenced by canaries; each method returns the canaries' state with
    # its result (a failed call raises RdfError; its canary state is then in ``self.test_canaries_ok``).
    def test_scan(self, kind: int, values, in_skew=0, out_skew=0, in_place=False, want_total=True):
        """Exclusive scan of ``values`` by the primitive of ``kind``: (out, total or None, canaries_ok)."""
        ti, to = SCAN_DTYPES[kind]
        a = np.ascontiguousarray(values, dtype=ti)
        out = np.empty(a.shape[0], to)
        total, ok = ctypes.c_uint64(), ctypes.c_uint32()
        rc = self._test_fn("rdf_test_scan")(self.ptr, kind, a.ctypes.data, a.shape[0], in_skew, out_skew, int(in_place),
                                    int(want_total), out.ctypes.data, ctypes.byref(total), ctypes.byref(ok))
        self.test_canaries_ok = bool(ok.value)
        self._check(rc, "rdf_test_scan")
        return out, (int(total.value) if want_total else None), bool(ok.value)

    def test_scan_batch(self, rows, skew_mask=0, k=None):
        """exclusive_scan_u32_u64_batch of the rows of a 2-D uint32 array: (out[k, n + 1], canaries_ok).  ``k``
        overrides the row count passed to the primitive (to ask for a count it must refuse)."""
        a = np.ascontiguousarray(rows, dtype=np.uint32)
        assert a.ndim == 2
        k = a.shape[0] if k is None else k
        out = np.empty((max(k, 0), a.shape[1] + 1), np.uint64)
        ok = ctypes.c_uint32()
        rc = self._test_fn("rdf_test_scan_batch")(self.ptr, k, a.ctypes.data, a.shape[1], skew_mask, out.ctypes.data,
                                          ctypes.byref(ok))
        self.test_canaries_ok = bool(ok.value)
        self._check(rc, "rdf_test_scan_batch")
        return out, bool(ok.value)

    def test_radix(self, op: int, keys, lo=0, hi=64, hmask=(1 << 64) - 1):
        """A radix primitive on ``keys`` (uint32 for RADIX_PART_U32, else uint64): (result, canaries_ok); the result
        is the array the primitive's ``keys`` names afterwards (for RADIX_SORT_DROP: the kept keys only)."""
        a = np.ascontiguousarray(keys, dtype=np.uint32 if op == RADIX_PART_U32 else np.uint64)
        out = np.empty_like(a)
        n_out, ok = ctypes.c_uint64(), ctypes.c_uint32()
        rc = self._test_fn("rdf_test_radix")(self.ptr, op, a.ctypes.data, a.shape[0], lo, hi, hmask, out.ctypes.data,
                                     ctypes.byref(n_out), ctypes.byref(ok))
        self.test_canaries_ok = bool(ok.value)
        self._check(rc, "rdf_test_radix")
        return out[: n_out.value], bool(ok.value)

    def test_radix_segments(self, src, counts, bases=None, stride=0, w0=0, bits=64, bump=None):
        """The sort of the keys that lie in segments of ``src`` (rdf_test_radix_segments): segment b is ``counts[b]``
        keys from ``bases[b]`` (``bases`` None: from ``b * stride``).  ``w0``: the first digit's width (0: the sort's
        own).  ``bump`` = (segment, digit, delta) changes one entry of the histogram the first pass is given.  Returns
        (sorted keys, canaries_ok)."""
        a = np.ascontiguousarray(src, dtype=np.uint64)
        cnt = np.ascontiguousarray(counts, dtype=np.uint64)
        base = None if bases is None else np.ascontiguousarray(bases, dtype=np.uint64)
        assert base is None or base.shape == cnt.shape
        out = np.empty(max(int(cnt.sum()), 1), np.uint64)
        bseg, bdig, bdelta = bump if bump else (0, 0, 0)
        n_out, ok = ctypes.c_uint64(), ctypes.c_uint32()
        rc = self._test_fn("rdf_test_radix_segments")(
            self.ptr, a.ctypes.data, a.shape[0], None if base is None else base.ctypes.data, stride, cnt.ctypes.data,
            cnt.shape[0], w0, bits, bdelta, bseg, bdig, out.ctypes.data, ctypes.byref(n_out), ctypes.byref(ok))
        self.test_canaries_ok = bool(ok.value)
        self._check(rc, "rdf_test_radix_segments")
        return out[: n_out.value], bool(ok.value)

    def test_record_tile(self) -> int:
        """Records per tile of the group build's tile kernels (rdf_test_record_tile)."""
        return int(self._test_fn("rdf_test_record_tile")())

    def test_keep_records(self, keys, joinbits: int, ncap: int, ms: int):
        """The support and keep passes over sorted records ``capture << joinbits | join`` (rdf_test_keep_records):
        (support[ncap], dk[Jf], fk[Jf], doff[C + 1], canaries_ok)."""
        a = np.ascontiguousarray(keys, dtype=np.uint64)
        sup = np.empty(ncap, np.uint32)
        dk, fk = np.empty(max(a.shape[0], 1), np.uint64), np.empty(max(a.shape[0], 1), np.uint64)
        doff = np.empty(ncap + 1, np.uint64)
        jf, ncomp, ok = ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_uint32()
        rc = self._test_fn("rdf_test_keep_records")(
            self.ptr, a.ctypes.data, a.shape[0], joinbits, ncap, ms, sup.ctypes.data, ctypes.byref(jf), ctypes.byref(ncomp),
            dk.ctypes.data, fk.ctypes.data, doff.ctypes.data, ctypes.byref(ok))
        self.test_canaries_ok = bool(ok.value)
        self._check(rc, "rdf_test_keep_records")
        return sup, dk[: jf.value], fk[: jf.value], doff[: ncomp.value + 1], bool(ok.value)

    def test_group_build(self, fk, num_values: int, rbase=0, gbase=0):
        """The group passes over records ``join << 32 | capture`` sorted by join (rdf_test_group_build):
        (goff[G + 1], gcap[n], gmap[num_values], canaries_ok); ``rbase`` / ``gbase``: a join range's offsets."""
        a = np.ascontiguousarray(fk, dtype=np.uint64)
        goff = np.empty(a.shape[0] + 1, np.uint64)
        gcap = np.empty(max(a.shape[0], 1), np.uint32)
        gmap = np.empty(num_values, np.uint32)
        g, ok = ctypes.c_uint64(), ctypes.c_uint32()
        rc = self._test_fn("rdf_test_group_build")(
            self.ptr, a.ctypes.data, a.shape[0], num_values, rbase, gbase, ctypes.byref(g), goff.ctypes.data,
            gcap.ctypes.data, gmap.ctypes.data, ctypes.byref(ok))
        self.test_canaries_ok = bool(ok.value)
        self._check(rc, "rdf_test_group_build")
        return goff[: g.value + 1], gcap[: a.shape[0]], gmap, bool(ok.value)

    def test_radix_pairs(self, keys, vals, lo=0, hi=32):
        """The stable pair sort of uint32 keys with uint32 values by key bits [lo, hi) (rdf_test_radix_pairs):
        (sorted keys, their values, canaries_ok); canaries_ok also says that the uploaded keys and values are intact."""
        k = np.ascontiguousarray(keys, dtype=np.uint32)
        v = np.ascontiguousarray(vals, dtype=np.uint32)
        assert k.shape == v.shape
        ko, vo = np.empty_like(k), np.empty_like(v)
        ok = ctypes.c_uint32()
        rc = self._test_fn("rdf_test_radix_pairs")(self.ptr, k.ctypes.data, v.ctypes.data, k.shape[0], lo, hi,
                                                   ko.ctypes.data, vo.ctypes.data, ctypes.byref(ok))
        self.test_canaries_ok = bool(ok.value)
        self._check(rc, "rdf_test_radix_pairs")
        return ko, vo, bool(ok.value)

    def test_group_kv(self, keys, joinbits: int, ncap: int, ms: int, num_values: int) -> dict:
        """The key-value form of the one-pass group build over sorted records ``capture << joinbits | join``
        (rdf_test_group_kv): support[ncap], doff[C + 1], dgrp[Jf], goff[G + 1], gcap[Jf], gmap[num_values], G, Jf and
        canaries_ok, by name."""
        a = np.ascontiguousarray(keys, dtype=np.uint64)
        m = max(a.shape[0], 1)
        sup, doff = np.empty(ncap, np.uint32), np.empty(ncap + 1, np.uint64)
        dgrp, gcap = np.empty(m, np.uint32), np.empty(m, np.uint32)
        goff, gmap = np.empty(m + 1, np.uint64), np.empty(num_values, np.uint32)
        jf, g, ncomp, ok = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_uint32()
        rc = self._test_fn("rdf_test_group_kv")(
            self.ptr, a.ctypes.data, a.shape[0], joinbits, ncap, ms, num_values, sup.ctypes.data, ctypes.byref(jf),
            ctypes.byref(ncomp), doff.ctypes.data, dgrp.ctypes.data, ctypes.byref(g), goff.ctypes.data, gcap.ctypes.data,
            gmap.ctypes.data, ctypes.byref(ok))
        self.test_canaries_ok = bool(ok.value)
        self._check(rc, "rdf_test_group_kv")
        return {"support": sup, "doff": doff[: ncomp.value + 1], "dgrp": dgrp[: jf.value], "goff": goff[: g.value + 1],
                "gcap": gcap[: jf.value], "gmap": gmap, "G": g.value, "Jf": jf.value, "canaries_ok": bool(ok.value)}

    def test_paths(self) -> dict:
        """Which alternative paths the last completed run took (rdf_test_paths): the K1 / K2 / K3 forms by name,
        dense_on, light_stage, light_hiocc, n_dense, n_dense_eligible, n_dedup_members, and what the light launches
        were given, summed over the run's pages, ranges and light passes: n_light_items (k_light work items),
        n_packed_octets (k_light_packed), n_mseg_chunks (k_light_mseg_emit), n_multi_items (items of dependents with
        several chunks), n_light_survivors (pass B's input), light_npx / packed_npx (extra pivots checked), and the
        flags light_ordered, light_side, light_two_pass, sig_on, piv2_on, k3_hist (K3 handed the record sort its first
        digit histogram).  Of the mask classes, as the run left them on the device: hclassed (binary heavy-only
        dependents read the class lists), n_class_chunks (k_class_eval work items), n_emit_tiles (k_class_emit tiles),
        max_class_list (refs of the longest L'(m)) and n_multi_seg_lists (lists longer than one emission segment).  Of K3's
        key items (RDFIND_EMIT_KEYS): k3_key_items (frequent binary keys the last build emitted from) and k3_suppressed
        (records its triples left to them).  group_form: "kv" or "u64", the form of the last one-pass group build
        (RDFIND_GROUP_KV); None after a build in join ranges."""
        r = PathReport()
        self._check(self._test_fn("rdf_test_paths")(self.ptr, ctypes.byref(r)), "rdf_test_paths")
        d = _struct_dict(r)
        d["k1_form"], d["k2_form"], d["k3_form"] = K1_FORMS[r.k1_form], K2_FORMS[r.k2_form], K3_FORMS[r.k3_form]
        d["group_form"] = GROUP_FORMS[r.group_form]
        for name in ("dense_on", "light_stage", "light_hiocc", "light_ordered", "light_side", "light_two_pass", "sig_on",
                     "piv2_on", "k3_hist", "hclassed"):
            d[name] = bool(d[name])
        return d

    def test_shard_report(self) -> dict:
        """What the exchange of the last completed sharded run did on this rank (rdf_test_shard_report): the holder's
        survivors, the words routed (reports and verify words), the reports and verify pairs received, the verify pairs
        kept, the owner's reports and need-complete pairs, the unary and binary pairs, the class counts, the hot table's
        entries, the heavy bit base and columns; max_verify_per_dep (None when the verify offsets are gone) is read
        from the device when this is called."""
        r = ShardReport()
        self._check(self._test_fn("rdf_test_shard_report")(self.ptr, ctypes.byref(r)), "rdf_test_shard_report")
        d = _struct_dict(r)
        if not d.pop("have_max_verify"):
            d["max_verify_per_dep"] = None
        return d

    def test_fc_trace(self, on: bool = True):
        """rdf_test_fc_trace: while on, frequent_conditions reads its slice lists back for :meth:`test_fc_report`."""
        self._check(self._test_fn("rdf_test_fc_trace")(self.ptr, int(on)), "rdf_test_fc_trace")

    def test_fc_report(self) -> dict:
        """The shape of the last frequent_conditions (rdf_test_fc_report): the K1 / K2 forms by name, k1_bits,
        k1_buckets, k2_bits, k2_sub, k2_buckets, k2_spill, and (``traced``: the stage ran under :meth:`test_fc_trace`)
        k1_slices, k1_multi, k2_multi."""
        r = FcReport()
        self._check(self._test_fn("rdf_test_fc_report")(self.ptr, ctypes.byref(r)), "rdf_test_fc_report")
        d = _struct_dict(r)
        d["k1_form"], d["k2_form"], d["traced"] = K1_FORMS[r.k1_form], K2_FORMS[r.k2_form], bool(r.traced)
        return d

    def test_copy_frequent_unary(self):
        """(fval[0, U), [frequent s, p, o]) of the last frequent_conditions (rdf_test_copy_frequent_unary)."""
        U, n3 = ctypes.c_uint64(), (ctypes.c_uint64 * 3)()
        fn = self._test_fn("rdf_test_copy_frequent_unary")
        if fn(self.ptr, None, 0, ctypes.byref(U), n3) != 0 and U.value == 0:  # (cap 0 < U fails after it told U)
            self._check(-1, "rdf_test_copy_frequent_unary")
        out = np.empty(U.value, np.uint32)
        self._check(fn(self.ptr, out.ctypes.data, out.shape[0], ctypes.byref(U), n3), "rdf_test_copy_frequent_unary")
        return out[: U.value], [int(x) for x in n3]

    def test_unary_lookup(self, keys):
        """(rank, bit, canaries_ok) of the unary keys ``pos * V + value`` (rdf_test_unary_lookup): the global rank among
        the frequent conditions (0xffffffff: none) and the key's bit of the frequency bitmap."""
        k = np.ascontiguousarray(keys, dtype=np.uint64)
        rank, bit, ok = np.empty(k.shape[0], np.uint32), np.empty(k.shape[0], np.uint32), ctypes.c_uint32()
        rc = self._test_fn("rdf_test_unary_lookup")(self.ptr, k.ctypes.data, k.shape[0], rank.ctypes.data, bit.ctypes.data,
                                                    ctypes.byref(ok))
        self.test_canaries_ok = bool(ok.value)
        self._check(rc, "rdf_test_unary_lookup")
        return rank, bit, bool(ok.value)

    # -- sharded mode (driven by rdfind_amd.distributed.run_sharded) ---------------------------
    def shard_begin(self, rank: int, nranks: int, min_support: int, projection="spo", clean_implied=True,
                    traversal_strategy=1, local_slice=False, use_ars=False):
        self.n_rules = 0
        """local_slice: the resident triples are this rank's slice of the input (else every rank holds all of
        them and the library takes its row range).  use_ars: association rules from the combined counts."""
        flags = (RDF_CLEAN_IMPLIED if clean_implied else 0) | (RDF_STRATEGY_ALL_AT_ONCE if traversal_strategy == 0 else 0)
        flags |= RDF_SHARD_LOCAL_SLICE if local_slice else 0
        flags |= RDF_USE_ASSOCIATION_RULES if use_ars else 0
        self._nranks = nranks
        self._check(self.lib.rdf_shard_begin(self.ptr, rank, nranks, min_support, projection.encode(), flags),
                    "rdf_shard_begin")

    def shard_parse_begin(self, rank: int, nranks: int, data: bytes, tabs: bool = False) -> int:
        """Sharded ingest of this rank's part of the input (rdf_shard_parse_begin); drive it with
        distributed.run_protocol.  Returns the rank's triples."""
        n = ctypes.c_uint64()
        self._nranks = nranks
        self._parsed = data
        self._check(self.lib.rdf_shard_parse_begin(self.ptr, rank, nranks, data, len(data), RDF_NT_TABS if tabs else 0,
                                                   ctypes.byref(n)), "rdf_shard_parse_begin")
        return int(n.value)

    def shard_dictionary_begin(self):
        """The formatting dictionary by owner lookup after a sharded run (rdf_shard_dictionary_begin)."""
        self._check(self.lib.rdf_shard_dictionary_begin(self.ptr), "rdf_shard_dictionary_begin")

    def num_terms_now(self) -> int:
        v = ctypes.c_uint32()
        self._check(self.lib.rdf_num_terms(self.ptr, ctypes.byref(v)), "rdf_num_terms")
        self.num_terms = int(v.value)
        return self.num_terms

    def dictionary_terms(self, ids) -> list:
        """Terms of the formatting dictionary (rdf_dictionary_terms), as str."""
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        off = np.zeros(ids.shape[0] + 1, np.uint64)
        cap = 1 << 20
        while True:
            out = ctypes.create_string_buffer(cap)
            rc = self.lib.rdf_dictionary_terms(self.ptr, ids.ctypes.data, ids.shape[0], out, cap, off.ctypes.data)
            if rc == 0:
                raw = out.raw
                return [raw[int(off[i]):int(off[i + 1])].decode("utf-8") for i in range(ids.shape[0])]
            if int(off[-1]) <= cap:
                self._check(rc, "rdf_dictionary_terms")
            cap = int(off[-1])

    def shard_step(self) -> ExchangeRequest:
        x = Exchange()
        self._check(self.lib.rdf_shard_step(self.ptr, ctypes.byref(x)), "rdf_shard_step")
        return ExchangeRequest(x.op, x.elem_bytes, x.count, list(x.send_counts)[: self._nranks])

    def shard_export(self, dst_ptr: int):
        self._check(self.lib.rdf_shard_export(self.ptr, dst_ptr), "rdf_shard_export")

    def shard_import(self, src_ptr: int, count: int):
        self._check(self.lib.rdf_shard_import(self.ptr, src_ptr, count), "rdf_shard_import")

    def stage_times(self):
        arr = (ctypes.c_float * 3)()
        self._check(self.lib.rdf_stage_times(self.ptr, arr), "rdf_stage_times")
        return list(arr)

    def kernel_times(self):
        arr = (ctypes.c_float * len(TIMER_NAMES))()
        self._check(self.lib.rdf_kernel_times(self.ptr, arr, len(TIMER_NAMES)), "rdf_kernel_times")
        return dict(zip(TIMER_NAMES, list(arr)))

    # -- results -----------------------------------------------------------------------------
    def cind_count(self) -> int:
        n = ctypes.c_uint64()
        self._check(self.lib.rdf_cind_count(self.ptr, ctypes.byref(n)), "rdf_cind_count")
        return n.value

    def copy_cinds(self) -> np.ndarray:
        n = self.cind_count()
        out = np.empty(n, dtype=CIND_DTYPE)
        copied = ctypes.c_uint64()
        self._check(self.lib.rdf_copy_cinds(self.ptr, out.ctypes.data, n, ctypes.byref(copied)), "rdf_copy_cinds")
        return out[: copied.value]

    def copy_cinds_range(self, offset: int, count: int) -> np.ndarray:
        out = np.empty(count, dtype=CIND_DTYPE)
        copied = ctypes.c_uint64()
        self._check(self.lib.rdf_copy_cinds_range(self.ptr, offset, out.ctypes.data, count, ctypes.byref(copied)),
                    "rdf_copy_cinds_range")
        return out[: copied.value]

    def result_sizes(self):
        """(n_refs, n_runs, n_captures) of the CindSet-shaped result (rdf_result_sizes)."""
        a, b, c = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self.lib.rdf_result_sizes(self.ptr, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)),
                    "rdf_result_sizes")
        return int(a.value), int(b.value), int(c.value)

    def copy_result_raw(self, refs_ptr=None, runoff=None, rundep=None, capture_ids=None, supports=None):
        """rdf_copy_result_raw into caller buffers (raw pointers or numpy arrays; None skips a part)."""
        def ptr(x):
            return None if x is None else (x if isinstance(x, int) else x.ctypes.data)
        self._check(self.lib.rdf_copy_result_raw(self.ptr, ptr(refs_ptr), ptr(runoff), ptr(rundep), ptr(capture_ids),
                                                 ptr(supports)), "rdf_copy_result_raw")

    def result_layout(self) -> dict:
        """Sizes of the compact CindSet-shaped result (rdf_get_result_layout)."""
        L = ResultLayout()
        self._check(self.lib.rdf_get_result_layout(self.ptr, ctypes.byref(L)), "rdf_get_result_layout")
        return _struct_dict(L)

    def copy_result_compact(self, bufs: dict | None = None) -> dict:
        """rdf_copy_result_compact into ``bufs`` (name -> numpy array or raw pointer, e.g. pinned memory sized from
        :meth:`result_layout`), or into fresh numpy arrays; returns the name -> buffer dict."""
        fresh = bufs is None
        if fresh:
            L = self.result_layout()
            bufs = {name: np.empty(max(count(L), 1), dt) for name, dt, count in COMPACT_PARTS}
            bufs["layout"] = L
        ptrs = [bufs[name] if isinstance(bufs[name], int) else bufs[name].ctypes.data for name, _, _ in COMPACT_PARTS]
        self._check(self.lib.rdf_copy_result_compact(self.ptr, *ptrs), "rdf_copy_result_compact")
        if fresh:  # the heavy-bits form's chunks (rdf_set_result_form), when the result has them
            nh = self.heavy_chunk_count()
            bufs["n_heavy_chunks"] = nh
            if nh:
                bufs["heavy_deps"] = np.empty(nh, np.uint32)
                bufs["heavy_pos"] = np.empty(nh, np.uint64)
                bufs["heavy_bits"] = np.empty(nh, np.uint64)
                self.copy_result_heavy(bufs["heavy_deps"], bufs["heavy_pos"], bufs["heavy_bits"])
        return bufs

    def set_handover(self, refs=None, refs_cap: int = 0, runoff=None, rundep=None, runs_cap: int = 0, capture_ids=None,
                     supports=None, capture_cap: int = 0):
        """rdf_set_handover: page-locked buffers (raw pointers or numpy arrays) the next unpaged discoveries fill early;
        rdf_copy_result_compact with the same buffers then copies only the rest.  No arguments: unregister."""
        p = [None if x is None else (x if isinstance(x, int) else x.ctypes.data)
             for x in (refs, runoff, rundep, capture_ids, supports)]
        self._check(self.lib.rdf_set_handover(self.ptr, p[0] or None, refs_cap, p[1] or None, p[2] or None, runs_cap,
                                              p[3] or None, p[4] or None, capture_cap), "rdf_set_handover")

    def copy_result_refs(self, offset: int, count: int, ptr) -> int:
        """rdf_copy_result_refs: refs[offset, offset + count) of the compact result into ``ptr`` (numpy array or raw
        pointer); returns the refs copied."""
        copied = ctypes.c_uint64()
        p = ptr if isinstance(ptr, int) else ptr.ctypes.data
        self._check(self.lib.rdf_copy_result_refs(self.ptr, offset, count, p, ctypes.byref(copied)), "rdf_copy_result_refs")
        return copied.value

    def copy_result_refs_async(self, offset: int, count: int, ptr: int) -> int:
        """rdf_copy_result_refs_async: the same copy queued on the context's copy stream (``ptr``: page-locked, untouched
        until handover_wait); returns the refs queued."""
        copied = ctypes.c_uint64()
        self._check(self.lib.rdf_copy_result_refs_async(self.ptr, offset, count, ptr, ctypes.byref(copied)),
                    "rdf_copy_result_refs_async")
        return copied.value

    def set_result_form(self, heavy_bits: bool) -> None:
        """rdf_set_result_form: RDF_FORM_HEAVY_BITS (the heavy-only refs as survivor words over the class lists) or
        the expanded form, from the next discovery on."""
        self._check(self.lib.rdf_set_result_form(self.ptr, 1 if heavy_bits else 0), "rdf_set_result_form")

    def heavy_chunk_count(self) -> int:
        n = ctypes.c_uint64()
        self._check(self.lib.rdf_heavy_chunk_count(self.ptr, ctypes.byref(n)), "rdf_heavy_chunk_count")
        return int(n.value)

    def copy_result_heavy(self, deps, pos, bits) -> None:
        """rdf_copy_result_heavy into three buffers (numpy arrays or raw pointers) of heavy_chunk_count() elements."""
        ptrs = [b if isinstance(b, int) else b.ctypes.data for b in (deps, pos, bits)]
        self._check(self.lib.rdf_copy_result_heavy(self.ptr, *ptrs), "rdf_copy_result_heavy")

    def handover_wait(self) -> None:
        """rdf_handover_wait: every queued copy has reached the host."""
        self._check(self.lib.rdf_handover_wait(self.ptr), "rdf_handover_wait")

    def copy_cinds_decoded(self, offset: int = 0, count: int | None = None) -> np.ndarray:
        """Cind-shaped rows decoded on the device (rdf_copy_cinds_decoded), ROW_DTYPE."""
        if count is None:
            count = max(self.cind_count() - offset, 0)
        out = np.empty(count, dtype=ROW_DTYPE)
        copied = ctypes.c_uint64()
        self._check(self.lib.rdf_copy_cinds_decoded(self.ptr, offset, out.ctypes.data, count, ctypes.byref(copied)),
                    "rdf_copy_cinds_decoded")
        return out[: copied.value]

    def checksum(self) -> int:
        v = ctypes.c_uint64()
        self._check(self.lib.rdf_cind_checksum(self.ptr, ctypes.byref(v)), "rdf_cind_checksum")
        return v.value

    def binary_keys(self) -> np.ndarray:
        n = ctypes.c_uint64()
        self._check(self.lib.rdf_binary_key_count(self.ptr, ctypes.byref(n)), "rdf_binary_key_count")
        out = np.empty(n.value, dtype=np.uint64)
        if n.value:
            self._check(self.lib.rdf_copy_binary_keys(self.ptr, out.ctypes.data, n.value), "rdf_copy_binary_keys")
        return out

    def set_dictionary(self, terms):
        """Uploads the dictionary (term id -> string) for device-side formatting."""
        enc = [t.encode("utf-8") for t in terms]
        heap = b"".join(enc)
        offsets = np.zeros(len(enc) + 1, dtype=np.uint64)
        if enc:
            np.cumsum(np.fromiter((len(e) for e in enc), dtype=np.uint64, count=len(enc)), out=offsets[1:])
        buf = ctypes.create_string_buffer(heap, max(len(heap), 1))
        self._check(self.lib.rdf_set_dictionary(self.ptr, buf, len(heap), offsets.ctypes.data, len(enc)),
                    "rdf_set_dictionary")

    def format_array(self, offset=0, count=None) -> np.ndarray:
        """Cind.toString lines ("...\n" each) of result rows [offset, offset + count), formatted on the GPU, as a
        uint8 array (no intermediate copies: write it to a file with ``arr.tofile`` / ``f.write(arr)``)."""
        if count is None:
            count = self.cind_count() - offset
        need = ctypes.c_uint64()
        self._check(self.lib.rdf_format_size(self.ptr, offset, count, ctypes.byref(need)), "rdf_format_size")
        out = np.empty(max(need.value, 1), dtype=np.uint8)
        got = ctypes.c_uint64()
        self._check(self.lib.rdf_format_cinds(self.ptr, offset, count, out.ctypes.data, need.value, ctypes.byref(got)),
                    "rdf_format_cinds")
        return out[: got.value]

    def format_cinds(self, offset=0, count=None) -> bytes:
        """As format_array, as bytes."""
        return self.format_array(offset, count).tobytes()

    def decoded_cinds(self):
        """Structured array with (dep_code, dep_v1, dep_v2, ref_code, ref_v1, ref_v2, support);
        v2 = 0xFFFFFFFF for unary captures."""
        rows = self.copy_cinds()
        return decode_rows(rows, self.num_terms, self.binary_keys())


DECODED_DTYPE = np.dtype([("dep_code", "u1"), ("dep_v1", "<u4"), ("dep_v2", "<u4"), ("ref_code", "u1"),
                          ("ref_v1", "<u4"), ("ref_v2", "<u4"), ("support", "<u4")])


def decode_captures(cap: np.ndarray, num_terms: int, bin_keys: np.ndarray):
    """Vectorised capture id -> (code, v1, v2)."""
    V = np.uint64(max(num_terms, 1))
    cap = cap.astype(np.uint64)
    unary = cap < np.uint64(6) * V
    code = np.empty(cap.shape, np.uint8)
    v1 = np.empty(cap.shape, np.uint32)
    v2 = np.full(cap.shape, 0xFFFFFFFF, np.uint32)
    ucodes = np.array(codes.UNARY_CODES, np.uint8)
    code[unary] = ucodes[(cap[unary] // V).astype(np.int64)]
    v1[unary] = (cap[unary] % V).astype(np.uint32)
    if (~unary).any():
        keys = bin_keys[(cap[~unary] - np.uint64(6) * V).astype(np.int64)]
        bcodes = np.array(codes.BINARY_CODES, np.uint8)
        code[~unary] = bcodes[(keys >> np.uint64(62)).astype(np.int64)]
        v1[~unary] = ((keys >> np.uint64(31)) & np.uint64(0x7FFFFFFF)).astype(np.uint32)
        v2[~unary] = (keys & np.uint64(0x7FFFFFFF)).astype(np.uint32)
    return code, v1, v2


def decode_rows(rows: np.ndarray, num_terms: int, bin_keys: np.ndarray) -> np.ndarray:
    out = np.empty(rows.shape[0], dtype=DECODED_DTYPE)
    out["dep_code"], out["dep_v1"], out["dep_v2"] = decode_captures(rows["dep"], num_terms, bin_keys)
    out["ref_code"], out["ref_v1"], out["ref_v2"] = decode_captures(rows["ref"], num_terms, bin_keys)
    out["support"] = rows["support"]
    return out


def decoded_to_set(dec: np.ndarray):
    """Set of (dt, dv1, dv2|None, rt, rv1, rv2|None, support) -- the oracle's comparison form."""
    none = 0xFFFFFFFF
    out = set()
    for r in dec.tolist():
        dt, dv1, dv2, rt, rv1, rv2, sup = r
        out.add((dt, dv1, None if dv2 == none else dv2, rt, rv1, None if rv2 == none else rv2, sup))
    return out
