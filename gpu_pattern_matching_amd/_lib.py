"""ctypes binding of libacmatch.so (the C ABI declared in include/acmatch.h).

The library is the product: there is no Python or CPU fallback.  If the shared
object is missing, ``load()`` raises; if no HIP device is visible, every
device entry point returns ACM_ERR_NODEV and the wrappers raise ``AcmError``.
"""
import ctypes as C
import os

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG, "libacmatch.so")

ACM_OK = 0
ACM_ERR_CAPACITY = -8

_vp = C.c_void_p
_i32p = C.POINTER(C.c_int32)
_u32p = C.POINTER(C.c_uint32)


class ScanBatch(C.Structure):
    """struct acm_scan_batch (include/acmatch.h)."""
    _fields_ = [("d_text", _vp), ("n", C.c_size_t), ("halo", C.c_size_t), ("offset_shift", C.c_long),
                ("init_state", C.c_long), ("d_workspace", _vp), ("workspace_bytes", C.c_size_t),
                ("d_pat_plane", _vp), ("d_off_plane", _vp), ("plane_capacity", C.c_size_t),
                ("stream", _vp), ("wait_before_walk", _vp), ("record_after_walk", _vp), ("report", C.c_int),
                ("profile", C.c_int), ("d_init_plane", _vp), ("init_plane_capacity", C.c_size_t)]


class ShardPlan(C.Structure):
    """struct acm_shard_plan (include/acmatch.h)."""
    _fields_ = [("begin", C.c_size_t), ("end", C.c_size_t), ("halo", C.c_size_t), ("load_begin", C.c_size_t),
                ("load_bytes", C.c_size_t), ("offset_shift", C.c_long)]


REPORT_HEAD, REPORT_STATE = 0, 1
TALLY_ACCUMULATE, TALLY_ALL_PATTERNS = 1, 2
PATTERN_NOCASE = 1
POS_FROM_END = 1
POS_UNBOUNDED = 0x7FFFFFFF
REPL_FILL = 1
REPLACEMENT_MAX_LEN = 65535
EXTRACT_END_INCLUSIVE = 1
EXTRACT_MAX_GLUE = 16
FORMAT_NAME, FORMAT_NUMBER, FORMAT_OFFSET = 2, 4, 8
FORMAT_MAX_NAME = 4096
LINE_SELECTED, LINE_GROUP_HEAD = 1, 2
NORM_PERCENT, NORM_SQUEEZE, NORM_STRIP = 1, 2, 4
NORM_BLOCK = 1024
SEQ_MAX_PARTS = 32
GAP_UNBOUNDED = 0x7FFFFFFF
WILDCARD_MAX_POSITIONS = 4096
APPROX_MAX_K = 15
APPROX_MAX_LEN = 4096
SIG_EXTENDED = 1
SIG_GROUPS = 2
GROUP_MAX_WIDTH = 32
GROUP_MAX_ALTERNATIVES = 256
PATTERN_MAX_GROUPS = 16


class WildGroup(C.Structure):
    """struct acm_wild_group (include/acmatch.h)."""
    _fields_ = [("at", C.c_int32), ("width", C.c_int32), ("count", C.c_int32), ("negated", C.c_int32),
                ("bytes", C.c_char_p)]
RULE_MAX_OPERANDS = 64
RULE_MAX_NESTING = 8


class AcmError(RuntimeError):
    def __init__(self, code, where, detail):
        super().__init__("%s: %s (code %d)" % (where, detail, code))
        self.code = code


# every exported symbol: name -> (restype, argtypes); tests check the .so
# exports exactly these (plus the reference-named layer below)
NATIVE_API = {
    "acm_last_error": (C.c_char_p, []),
    "acm_strerror": (C.c_char_p, [C.c_int]),
    "acm_version": (C.c_char_p, []),
    "acm_device_count": (C.c_int, []),
    "acm_automaton_new": (_vp, []),
    "acm_automaton_state_matches": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_int32), C.c_int]),
    "acm_automaton_free": (None, [_vp]),
    "acm_automaton_add": (C.c_int, [_vp, C.c_char_p, C.c_int, C.c_int]),
    "acm_automaton_load_file": (C.c_int, [_vp, C.c_char_p, C.c_int, C.c_int]),
    "acm_automaton_add_ex": (C.c_int, [_vp, C.c_char_p, C.c_int, C.c_int, C.c_uint]),
    "acm_automaton_load_file_ex": (C.c_int, [_vp, C.c_char_p, C.c_int, C.c_int, C.c_uint]),
    "acm_automaton_pattern_flags": (C.c_int, [_vp, C.c_int]),
    "acm_automaton_mixed_case": (C.c_int, [_vp]),
    "acm_automaton_set_position": (C.c_int, [_vp, C.c_int, C.c_int32, C.c_int32, C.c_uint]),
    "acm_automaton_pattern_position": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                                 C.POINTER(C.c_uint)]),
    "acm_automaton_positioned": (C.c_int, [_vp]),
    "acm_automaton_load_position_file": (C.c_int, [_vp, C.c_char_p]),
    "acm_automaton_set_replacement": (C.c_int, [_vp, C.c_int, C.c_char_p, C.c_int, C.c_uint]),
    "acm_automaton_clear_replacement": (C.c_int, [_vp, C.c_int]),
    "acm_automaton_pattern_replacement": (C.c_int, [_vp, C.c_int, C.POINTER(_vp), C.POINTER(C.c_int),
                                                    C.POINTER(C.c_uint)]),
    "acm_automaton_has_replacements": (C.c_int, [_vp]),
    "acm_automaton_max_replacement_len": (C.c_int, [_vp]),
    "acm_automaton_load_replacement_file": (C.c_int, [_vp, C.c_char_p]),
    "acm_automaton_add_sequence": (C.c_int, [_vp, _i32p, _i32p, _i32p, C.c_int, C.c_int]),
    "acm_automaton_num_sequences": (C.c_int, [_vp]),
    "acm_automaton_sequence": (C.c_int, [_vp, C.c_int, _i32p, _i32p, C.POINTER(_i32p), C.POINTER(_i32p),
                                         C.POINTER(_i32p)]),
    "acm_automaton_pattern_sequence": (C.c_int, [_vp, C.c_int, _i32p, _i32p]),
    "acm_automaton_add_signature": (C.c_int, [_vp, C.c_char_p, C.c_int, C.c_uint]),
    "acm_automaton_load_signature_file": (C.c_int, [_vp, C.c_char_p, C.c_uint]),
    "acm_automaton_add_wildcard": (C.c_int, [_vp, C.c_char_p, C.c_int, C.c_int, C.c_uint]),
    "acm_automaton_pattern_wildcard": (C.c_int, [_vp, C.c_int, _i32p, _i32p, C.POINTER(_vp), C.POINTER(_vp)]),
    "acm_automaton_wildcards": (C.c_int, [_vp]),
    "acm_automaton_wildcard_reach": (C.c_int, [_vp, _i32p, _i32p]),
    "acm_automaton_add_wildcard_groups": (C.c_int, [_vp, C.c_char_p, C.c_int, C.POINTER(WildGroup), C.c_int, C.c_int,
                                                    C.c_uint]),
    "acm_automaton_pattern_groups": (C.c_int, [_vp, C.c_int]),
    "acm_automaton_pattern_group": (C.c_int, [_vp, C.c_int, C.c_int, _i32p, _i32p, _i32p, _i32p, C.POINTER(_vp)]),
    "acm_automaton_groups": (C.c_int, [_vp]),
    "acm_automaton_add_signature_ex": (C.c_int, [_vp, C.c_char_p, C.c_int, C.c_uint, C.c_uint]),
    "acm_automaton_add_approx": (C.c_int, [_vp, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_uint]),
    "acm_automaton_num_approx": (C.c_int, [_vp]),
    "acm_automaton_approx": (C.c_int, [_vp, C.c_int, _i32p, _i32p, _i32p, _i32p, C.POINTER(C.c_uint), C.POINTER(_vp)]),
    "acm_automaton_pattern_approx": (C.c_int, [_vp, C.c_int, _i32p, _i32p, _i32p, _i32p]),
    "acm_automaton_approx_reach": (C.c_int, [_vp, _i32p, _i32p]),
    "acm_automaton_add_edit": (C.c_int, [_vp, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_uint]),
    "acm_automaton_approx_mode": (C.c_int, [_vp, C.c_int]),
    "acm_automaton_load_signature_file_ex": (C.c_int, [_vp, C.c_char_p, C.c_uint, C.c_uint]),
    "acm_automaton_add_rule": (C.c_int, [_vp, _i32p, C.c_int, C.c_char_p, C.c_int]),
    "acm_automaton_num_rules": (C.c_int, [_vp]),
    "acm_automaton_rule": (C.c_int, [_vp, C.c_int, _i32p, _i32p, C.POINTER(_i32p), C.POINTER(C.c_char_p)]),
    "acm_automaton_sequence_rule": (C.c_int, [_vp, C.c_int, _i32p, _i32p]),
    "acm_automaton_add_logical_signature": (C.c_int, [_vp, C.c_char_p, C.c_int, C.c_uint, C.c_uint]),
    "acm_automaton_load_logical_file": (C.c_int, [_vp, C.c_char_p, C.c_uint, C.c_uint]),
    "acm_automaton_set_nocase": (C.c_int, [_vp, C.c_int]),
    "acm_automaton_nocase": (C.c_int, [_vp]),
    "acm_automaton_compile": (C.c_int, [_vp]),
    "acm_automaton_num_patterns": (C.c_int, [_vp]),
    "acm_automaton_max_pattern_len": (C.c_int, [_vp]),
    "acm_automaton_byte_classes": (C.c_int, [_vp, _vp]),
    "acm_compact_selftest": (C.c_int, [_vp, C.c_uint32, _u32p]),
    "acm_sieve_selftest": (C.c_int, [_vp, _u32p]),
    "acm_compact_profile": (C.c_int, [_vp, _vp, C.c_size_t, C.POINTER(C.c_uint64)]),
    "acm_automaton_num_states": (C.c_int, [_vp]),
    "acm_automaton_reference_table_bytes": (C.c_size_t, [_vp]),
    "acm_automaton_export_reference_table": (C.c_int, [_vp, _i32p]),
    "acm_automaton_pattern": (C.c_int, [_vp, C.c_int, _i32p, _i32p, C.POINTER(_vp), _i32p]),
    "acm_automaton_state_output": (C.c_int, [_vp, C.c_int]),
    "acm_automaton_state_fail": (C.c_int, [_vp, C.c_int]),
    "acm_automaton_state_depth": (C.c_int, [_vp, C.c_int]),
    "acm_dfa_upload": (C.c_int, [_vp, C.c_int, C.POINTER(_vp)]),
    "acm_dfa_release": (None, [_vp]),
    "acm_dfa_device_bytes": (C.c_size_t, [_vp]),
    "acm_dfa_hot_rows": (C.c_int, [_vp]),
    "acm_dfa_device": (C.c_int, [_vp]),
    "acm_scan_workspace_bytes": (C.c_size_t, [_vp, C.c_size_t]),
    "acm_scan_async": (C.c_int, [_vp, _vp, C.c_size_t, C.c_long, _vp, C.c_size_t, _vp, _vp,
                                 C.c_size_t, _vp]),
    "acm_scan_shard_async": (C.c_int, [_vp, _vp, C.c_size_t, C.c_size_t, C.c_long, C.c_long, _vp,
                                       C.c_size_t, _vp, _vp, C.c_size_t, _vp]),
    "acm_scan_batch_async": (C.c_int, [_vp, C.POINTER(ScanBatch)]),
    "acm_scan_batches_async": (C.c_int, [_vp, C.POINTER(ScanBatch), C.c_size_t]),
    "acm_scan_set_max_group": (C.c_int, [_vp, C.c_int]),
    "acm_scan_set_chain_bytes": (C.c_int, [_vp, C.c_int]),
    "acm_scan_set_chains_per_lane": (C.c_int, [_vp, C.c_int]),
    "acm_scan_kernel_count": (C.c_int, []),
    "acm_expand_workspace_bytes": (C.c_size_t, [C.c_size_t]),
    "acm_expand_matches_async": (C.c_int, [_vp, _vp, _vp, C.c_size_t, _vp, _vp, C.c_size_t, _vp, C.c_size_t, _vp]),
    "acm_segment_workspace_bytes": (C.c_size_t, [C.c_size_t]),
    "acm_segment_matches_async": (C.c_int, [_vp, _vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_long, C.c_int, _vp, _vp,
                                            _vp, C.c_size_t, _vp, _vp, C.c_size_t, _vp]),
    "acm_word_workspace_bytes": (C.c_size_t, [C.c_size_t]),
    "acm_word_matches_async": (C.c_int, [_vp, _vp, _vp, C.c_size_t, _vp, C.c_long, C.c_long, _vp, C.c_size_t, C.c_int,
                                         _vp, C.c_size_t, _vp, C.c_int, _vp, _vp, C.c_size_t, _vp, _vp, C.c_size_t, _vp]),
    "acm_case_workspace_bytes": (C.c_size_t, [C.c_size_t]),
    "acm_case_matches_async": (C.c_int, [_vp, _vp, _vp, C.c_size_t, _vp, C.c_long, C.c_long, _vp, C.c_size_t, C.c_int,
                                         _vp, _vp, C.c_size_t, _vp, _vp, C.c_size_t, _vp]),
    "acm_position_workspace_bytes": (C.c_size_t, [C.c_size_t]),
    "acm_position_matches_async": (C.c_int, [_vp, _vp, _vp, C.c_size_t, C.c_int, _vp, C.c_size_t, C.c_long, C.c_long,
                                             C.c_long, C.c_int, _vp, _vp, C.c_size_t, _vp, _vp, C.c_size_t, _vp]),
    "acm_wildcard_workspace_bytes": (C.c_size_t, [C.c_size_t]),
    "acm_wildcard_matches_async": (C.c_int, [_vp, _vp, _vp, C.c_size_t, C.c_int, _vp, C.c_long, C.c_long, _vp, C.c_size_t,
                                             _vp, C.c_size_t, C.c_long, C.c_long, C.c_int, _vp, _vp, C.c_size_t, _vp, _vp,
                                             C.c_size_t, _vp]),
    "acm_approx_workspace_bytes": (C.c_size_t, [C.c_size_t]),
    "acm_approx_matches_async": (C.c_int, [_vp, _vp, _vp, C.c_size_t, C.c_int, _vp, C.c_long, C.c_long, _vp, C.c_size_t,
                                           _vp, C.c_size_t, C.c_long, C.c_long, _vp, _vp, _vp, C.c_size_t, _vp, _vp,
                                           C.c_size_t, _vp]),
    "acm_edit_workspace_bytes": (C.c_size_t, [_vp, C.c_size_t]),
    "acm_edit_matches_async": (C.c_int, [_vp, _vp, _vp, C.c_size_t, C.c_int, _vp, C.c_long, C.c_long, _vp, C.c_size_t,
                                         _vp, C.c_size_t, C.c_long, C.c_long, _vp, _vp, _vp, _vp, C.c_size_t, _vp, _vp,
                                         C.c_size_t, _vp]),
    "acm_sequence_workspace_bytes": (C.c_size_t, [_vp, C.c_size_t]),
    "acm_sequence_matches_async": (C.c_int, [_vp, _vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_long, C.c_long, _vp, _vp,
                                             C.c_size_t, _vp, _vp, C.c_size_t, _vp]),
    "acm_rule_workspace_bytes": (C.c_size_t, [_vp, C.c_size_t]),
    "acm_rule_matches_async": (C.c_int, [_vp, _vp, _vp, C.c_size_t, _vp, C.c_size_t, _vp, _vp, _vp, C.c_size_t, _vp, _vp,
                                         C.c_size_t, _vp]),
    "acm_select_workspace_bytes": (C.c_size_t, [C.c_size_t]),
    "acm_select_matches_async": (C.c_int, [_vp, _vp, _vp, C.c_size_t, C.c_long, C.c_uint, _vp, _vp, _vp, C.c_size_t, _vp,
                                           _vp, C.c_size_t, _vp]),
    "acm_rewrite_workspace_bytes": (C.c_size_t, [C.c_size_t, C.c_size_t]),
    "acm_rewrite_async": (C.c_int, [_vp, _vp, C.c_size_t, C.c_long, _vp, _vp, C.c_size_t, _vp, C.c_size_t, _vp, C.c_size_t,
                                    _vp, C.c_size_t, _vp, _vp, _vp, C.c_size_t, _vp]),
    "acm_extract_workspace_bytes": (C.c_size_t, [C.c_size_t, C.c_size_t]),
    "acm_extract_async": (C.c_int, [_vp, C.c_size_t, C.c_long, _vp, _vp, C.c_size_t, C.c_uint, C.c_char_p, C.c_int, C.c_int,
                                    _vp, C.c_size_t, _vp, C.c_size_t, _vp, C.c_size_t, _vp, _vp, _vp, C.c_size_t, _vp]),
    "acm_format_workspace_bytes": (C.c_size_t, [C.c_size_t, C.c_size_t]),
    "acm_format_async": (C.c_int, [_vp, C.c_size_t, C.c_long, _vp, _vp, C.c_size_t, C.c_uint, _vp, _vp, _vp, C.c_long, C.c_long,
                                   C.c_int, C.c_int, _vp, _vp, C.c_size_t, C.c_char_p, C.c_int, C.c_int, _vp, C.c_size_t, _vp,
                                   C.c_size_t, _vp, C.c_size_t, _vp, _vp, _vp, C.c_size_t, _vp]),
    "acm_tally_workspace_bytes": (C.c_size_t, [C.c_size_t, C.c_size_t]),
    "acm_tally_matches_async": (C.c_int, [_vp, _vp, _vp, C.c_size_t, C.c_int, C.c_int, _vp, C.c_size_t, _vp, C.c_size_t,
                                          _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "acm_line_index_workspace_bytes": (C.c_size_t, [C.c_size_t]),
    "acm_line_index_async": (C.c_int, [_vp, C.c_size_t, C.c_long, C.c_int, C.c_int, _vp, _vp, C.c_size_t, _vp, _vp,
                                       C.c_size_t, _vp]),
    "acm_line_number_async": (C.c_int, [_vp, C.c_size_t, _vp, _vp, _vp, C.c_size_t, _vp, _vp]),
    "acm_line_select_workspace_bytes": (C.c_size_t, [C.c_size_t]),
    "acm_line_select_async": (C.c_int, [_vp, C.c_size_t, _vp, C.c_long, C.c_long, _vp, C.c_size_t, C.c_int, _vp, _vp, _vp,
                                        C.c_size_t, _vp, C.c_size_t, _vp]),
    "acm_line_context_workspace_bytes": (C.c_size_t, [C.c_size_t, C.c_size_t]),
    "acm_line_context_async": (C.c_int, [_vp, C.c_size_t, _vp, C.c_long, C.c_long, _vp, C.c_size_t, C.c_int, C.c_int, C.c_int,
                                         _vp, C.c_size_t, _vp, _vp, _vp, _vp, C.c_size_t, _vp, _vp, C.c_size_t, _vp]),
    "acm_line_context_lines_workspace_bytes": (C.c_size_t, [C.c_size_t, C.c_size_t]),
    "acm_line_context_lines_async": (C.c_int, [_vp, C.c_size_t, _vp, C.c_long, C.c_long, _vp, C.c_size_t, C.c_int, C.c_int,
                                               C.c_int, _vp, C.c_size_t, _vp, _vp, _vp, _vp, C.c_size_t, _vp, _vp, C.c_size_t,
                                               _vp]),
    "acm_normalize_workspace_bytes": (C.c_size_t, [C.c_size_t, C.c_size_t]),
    "acm_normalize_async": (C.c_int, [_vp, C.c_size_t, C.c_long, C.c_uint, C.c_char_p, C.c_int, _vp, C.c_size_t, _vp, _vp,
                                      _vp, C.c_size_t, _vp, _vp, _vp, C.c_size_t, _vp]),
    "acm_normalize_remap_async": (C.c_int, [_vp, _vp, C.c_size_t, C.c_long, C.c_uint, _vp, _vp, _vp, _vp, C.c_size_t, _vp,
                                            _vp, _vp, _vp]),
    "acm_scan_set_mode": (C.c_int, [_vp, C.c_int]),
    "acm_scan_set_graphs": (C.c_int, [_vp, C.c_int]),
    "acm_scan_graph_stats": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "acm_scan_sparse_eligible": (C.c_int, [_vp]),
    "acm_scan_lds_resident": (C.c_int, [_vp]),
    "acm_scan_group_capable": (C.c_int, [_vp]),
    "acm_scan_path_taken": (C.c_int, [_vp, _vp, C.c_size_t, _vp]),
    "acm_scan_profile_enable": (C.c_int, [_vp, C.c_int]),
    "acm_scan_profile_read": (C.c_int, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                        C.POINTER(C.c_int)]),
    "acm_exclusive_scan_workspace_bytes": (C.c_size_t, [C.c_size_t]),
    "acm_exclusive_scan_i32": (C.c_int, [_vp, _vp, C.c_size_t, _vp, _vp, C.c_size_t, _vp]),
    "acm_compact_buckets": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, _vp]),
    "acm_bitonic_sort_u32": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint, C.c_uint, C.c_uint, _vp]),
    "acm_bucketize": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp, C.c_size_t, _vp]),
    "acm_pack_chunks": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int, _vp]),
    "acm_remap_offsets": (C.c_int, [_vp, C.c_size_t, _vp, _vp, C.c_int, _vp]),
    "acm_shard_plan_for": (C.c_int, [C.c_size_t, C.c_int, C.c_int, C.c_int, _vp]),
    "acm_gather_planes": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_size_t, _vp, _vp, _vp]),
    "acm_gather_planes_sized": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_size_t, _vp, _vp, _vp, _i32p, _vp]),
    "acm_merge_planes": (C.c_long, [_vp, _vp, C.c_int, C.c_size_t, _vp, _vp, C.c_size_t, _vp]),
    "acm_rt_set_device": (C.c_int, [C.c_int]),
    "acm_rt_malloc": (C.c_int, [C.POINTER(_vp), C.c_size_t]),
    "acm_rt_free": (C.c_int, [_vp]),
    "acm_rt_host_alloc": (C.c_int, [C.POINTER(_vp), C.c_size_t]),
    "acm_rt_host_free": (C.c_int, [_vp]),
    "acm_rt_memcpy_h2d": (C.c_int, [_vp, _vp, C.c_size_t, _vp]),
    "acm_rt_memcpy_d2h": (C.c_int, [_vp, _vp, C.c_size_t, _vp]),
    "acm_rt_memcpy_d2d": (C.c_int, [_vp, _vp, C.c_size_t, _vp]),
    "acm_rt_memset": (C.c_int, [_vp, C.c_int, C.c_size_t, _vp]),
    "acm_rt_stream_create": (C.c_int, [C.POINTER(_vp)]),
    "acm_rt_stream_destroy": (C.c_int, [_vp]),
    "acm_rt_stream_sync": (C.c_int, [_vp]),
    "acm_rt_device_sync": (C.c_int, []),
    "acm_rt_event_create": (C.c_int, [C.POINTER(_vp)]),
    "acm_rt_event_destroy": (C.c_int, [_vp]),
    "acm_rt_event_record": (C.c_int, [_vp, _vp]),
    "acm_rt_event_sync": (C.c_int, [_vp]),
    "acm_rt_event_elapsed_ms": (C.c_int, [_vp, _vp, C.POINTER(C.c_float)]),
    "acm_rt_device_info": (C.c_int, [C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int),
                                     C.POINTER(C.c_size_t), C.POINTER(C.c_int)]),
}

# the reference's names (include/acmatch.h layer 2); signatures are bound in
# compat.py, here only the list the export test checks
REFERENCE_API = [
    "clinitctx",
    "acsm_new", "acsm_add_pattern", "acsm_compile", "acsm_gen_state_table",
    "acsm_get_patterns_table", "acsm_get_max_pattern_size", "acsm_get_states", "acsm_get_size",
    "acsm_cleanup", "acsm_free",
    "databuf_new", "databuf_add_fd", "databuf_add_fp", "databuf_add_chunk", "databuf_reset",
    "databuf_clear", "databuf_copy_host_to_device", "databuf_copy_device_to_host",
    "databuf_process_results", "databuf_free",
    "ocl_aho_match_init", "ocl_aho_match_close", "ocl_aho_match",
    "ocl_prefix_sum_init", "ocl_prefix_sum_close", "ocl_prefix_sum",
    "ocl_compact_array_init", "ocl_compact_array_close", "ocl_compact_array",
    "ocl_bitonic_sort_init", "ocl_bitonic_sort_close", "ocl_bitonic_sort",
]

_lib = None


def load():
    """Load libacmatch.so; raise if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "libacmatch.so is missing (%s). Build it with "
            "`python -m gpu_pattern_matching_amd.build`; there is no fallback path." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in NATIVE_API.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(code, where):
    if code != ACM_OK:
        lib = load()
        detail = lib.acm_last_error().decode() or lib.acm_strerror(code).decode()
        raise AcmError(code, where, detail)
