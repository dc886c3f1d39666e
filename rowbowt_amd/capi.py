"""ctypes binding of rowbowt_amd/librbg.so (the C-ABI of include/rbg.h).

Names mirror the reference's operator API for this path: rbwt::load_rowbowt (rowbowt_io.hpp:176),
rbwt::LoadRbwtFlag (:146-152) and rbwt::RowBowt<> methods find_range / find_range_w_toehold /
locs_at / count / markers_at / find_range_w_markers / resolve_offset (rowbowt.hpp), batched.
The library must be present: a missing or unloadable librbg.so is an error, never a fallback.
"""
import ctypes as C
import enum
import os
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "librbg.so")

U64 = C.c_uint64
VP = C.c_void_p
MAXU = 2**64 - 1
DEVICE_NONE = -1

OPT_BLOCK_THREADS, OPT_RANK_BUCKET_SHIFT, OPT_PHI_BUCKET_SHIFT, OPT_POS_BYTES, OPT_KMER_STEPS, OPT_HBM_BUDGET_MB, OPT_FTAB_K, OPT_PACKED_READS, OPT_DEEP_BUCKET_SHIFT, OPT_DENSE_OVERFLOW, OPT_RANK_LAYOUT = range(1, 12)
OPT_RUN_DEPTHS, OPT_RUN_PHI, OPT_RUN_REC, OPT_RUN_REC_DEPTHS = 14, 16, 17, 18   # (12, 13, 15 were TREE_TOP_KB, SLOT_BYTES, RUN_FMT: retired with ABI 3)
OPT_EXTRACT_CHUNK = 20   # rbg_extract: bases per piece of a split interval (the result does not depend on it)
OPT_JUMP_K = 19          # the jump table (rbg_jump_info): 0 = off, -1 = automatic, 16..64 = symbols per key
OPT_JUMP2_K = 21         # level 2 of the jump table: 0 = off, -1 = automatic, 16..48 = symbols per key after the first table's
ABI_VERSION = 3          # include/rbg.h RBG_ABI_VERSION this binding is written against
MAX_KMER_DEPTH = 8       # RBG_OPT_KMER_STEPS / the depth arrays of Info and LayoutInfo
LAYOUT_AUTO, LAYOUT_SLOTS, LAYOUT_RUNS, LAYOUT_PREFER_SLOTS = 0, 1, 2, 3
SEEDS_W_SAMPLE = 1   # RBG_SEEDS_W_SAMPLE: get_seeds_greedy_w_sample (0: get_seeds_greedy)
(ARR_RUN_HEADS, ARR_RUN_START, ARR_SAMPLES_LAST, ARR_PRED_POS, ARR_PHI_BASE,
 ARR_MARKER_START, ARR_MARKER_END, ARR_MARKER_OFF, ARR_MARKER_VALS) = range(9)


class LoadRbwtFlag(enum.IntFlag):
    """rbwt::LoadRbwtFlag, rowbowt_io.hpp:146-152"""
    NONE = 0
    SA = 1
    MA = 2
    DL = 4
    FT = 8


class RbgError(RuntimeError):
    def __init__(self, code, what):
        self.code = code
        super().__init__(f"{what}: {lib().rbg_strerror(code).decode()} ({code})")


class Info(C.Structure):
    _fields_ = [("n", U64), ("r", U64), ("sigma", C.c_uint32), ("pos_bytes", C.c_uint32), ("device", C.c_int32),
                ("has_tsa", C.c_uint32), ("has_markers", C.c_uint32), ("has_docs", C.c_uint32),
                ("hbm_bytes", U64), ("marker_runs", U64), ("marker_vals", U64),
                ("rank_bucket_shift", C.c_uint32), ("phi_bucket_shift", C.c_uint32), ("slot_bytes", C.c_uint32),
                ("rank_slots", U64), ("rank_slots_overflow", U64), ("phi_slots", U64), ("phi_slots_overflow", U64),
                ("kmer_steps", U64), ("kmer_symbols", U64), ("pair_runs", U64), ("triple_runs", U64), ("quad_runs", U64), ("ftab_k", U64), ("quint_runs", U64),
                ("kmer_steps_requested", U64), ("hbm_free_at_load", U64), ("hbm_budget", U64), ("rank_layout", U64), ("replicas", U64),
                ("depth_runs", U64 * 8)]


class LayoutInfo(C.Structure):
    """rbg_layout_info_t"""
    _fields_ = [("run_fmt", C.c_uint32), ("depths_composed", C.c_uint32), ("depth_mask_asked", C.c_uint32), ("depth_mask_kept", C.c_uint32),
                ("depths_dropped_budget", C.c_uint32), ("rank_directories", C.c_uint32),
                ("phi_directory", C.c_uint32), ("fill_shift", C.c_uint32),
                ("entries", U64 * 8), ("fillers", U64 * 8), ("dir_bytes", U64 * 8),
                ("phi_entries", U64), ("phi_fillers", U64), ("phi_dir_bytes", U64), ("phi_dir_shift", U64), ("phi_slots", U64), ("phi_slot_bytes", U64), ("rec_bytes", U64 * 8), ("rec_overflow", U64 * 8), ("budget_raised", U64)]


class JumpInfo(C.Structure):
    """rbg_jump_info_t"""
    _fields_ = [("k", U64), ("keys", U64), ("bytes", U64), ("buckets", U64), ("build_ms", C.c_double),
                ("k2", U64), ("keys2", U64), ("bytes2", U64), ("buckets2", U64), ("build2_ms", C.c_double)]   # level 2 (rbg_jump_info_sized)


class JumpInfoComplete(C.Structure):
    """rbg_jump_info_t with the field added after level 2; JumpInfo stays the 80-byte prefix it was (rbg_jump_info_sized writes what it is given room for)"""
    _fields_ = JumpInfo._fields_ + [("complete", U64)]   # bit 0 / bit 1: an absent key of level 1 / level 2 ends the read at the probe


class ReportParams(C.Structure):
    """rbg_report_params_t"""
    _fields_ = [(n, U64) for n in ("wsize", "max_range", "min_range", "ftab_k", "read_len", "min_seed_len")] + [("flags", C.c_uint32)]


REPORT_LMEM, REPORT_HEURISTIC, REPORT_BEST_STRAND, REPORT_CLEAR_CONFLICTING, REPORT_CLEAR_IDENTICAL = 1, 2, 4, 8, 16
# rbg_report_seed_t as a numpy record
REPORT_SEED = np.dtype([("range_size", "<u8"), ("query_start", "<u8"), ("query_len", "<u8"), ("mk_begin", "<u8"), ("mk_end", "<u8"),
                        ("strand", "<u4"), ("pad", "<u4")])


# rbg_tally_entry_t as a numpy record
TALLY_ENTRY = np.dtype([("marker", "<u8"), ("n_fwd", "<u8"), ("n_rev", "<u8"), ("len_sum", "<u8")])
TALLY_INFO = ("entries", "capacity", "grows", "records", "elements", "dropped")
# rbg_markers_tally_reads' / rbg_tally_add_reads_dev's flag word; rbg_tally_read_info's four counters
TALLY_PER_READ, TALLY_DROP_SITE_CONFLICTS = 1, 2
TALLY_READ_INFO = ("reads", "elements_seen", "lost", "site_dropped")
DOCS_MAX = 1 << 16        # RBG_DOCS_MAX: documents a device table holds (rbg_docs_prepare)
SAM_MAX_MISMATCH = 8      # RBG_SAM_MAX_MISMATCH: the largest budget of rbg_align_sam_extend / rbg_extend_left_dev
# rbg_extend_t: what the left extension of one item leaves behind
EXTEND = np.dtype([("ext", np.uint32), ("nm", np.uint32), ("score", np.int32), ("steps", np.uint32), ("mis_t", np.uint32, 8), ("mis_ref", np.uint8, 8)])
SAM_SECONDARY = 1         # RBG_SAM_SECONDARY: rbg_align_sam also writes one line per further location, up to max_hits
LOCATE_DOCS_MAX = 1024    # RBG_LOCATE_DOCS_MAX: documents up to which rbg_locate_doc_hits_dev runs (the table in LDS)
DOC_NONE = 0xFFFFFFFF     # RBG_DOC_NONE: the document of a position that has none


def report_params(wsize=19, max_range=1000, min_range=0, ftab_k=0, read_len=101, min_seed_len=0, lmem=False, heuristic=False, best_strand=False,
                  clear_conflicting=False, clear_identical=False):
    """rb_markers' options as an rbg_report_params_t (the defaults are the tool's, rb_markers.cpp:22-40)"""
    flags = ((REPORT_LMEM if lmem else 0) | (REPORT_HEURISTIC if heuristic else 0) | (REPORT_BEST_STRAND if best_strand else 0)
             | (REPORT_CLEAR_CONFLICTING if clear_conflicting else 0) | (REPORT_CLEAR_IDENTICAL if clear_identical else 0))
    return ReportParams(wsize, max_range & MAXU, min_range, ftab_k, read_len, min_seed_len, flags)


# every symbol include/rbg.h declares: (name, restype, argtypes)
_PROTOS = [
    ("rbg_abi_version", C.c_int, []),
    ("rbg_strerror", C.c_char_p, [C.c_int]),
    ("rbg_load", C.c_int, [C.c_char_p, C.c_int, C.c_int, C.POINTER(VP)]),
    ("rbg_build_from_runs", C.c_int, [VP, VP, U64, VP, VP, C.c_int, C.POINTER(VP)]),
    ("rbg_build_from_files", C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(VP)]),
    ("rbg_convert_index", C.c_int, [C.c_char_p, C.c_int, C.c_char_p]),
    ("rbg_convert_raw", C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p]),
    ("rbg_load_cache", C.c_int, [C.c_char_p, C.c_int, C.c_int, C.POINTER(VP)]),
    ("rbg_doc_table", C.c_int, [VP, C.POINTER(U64), C.POINTER(VP), C.POINTER(VP), C.POINTER(U64)]),
    ("rbg_align_text", C.c_int, [VP, VP, VP, VP, U64, U64, C.c_uint32, VP, VP, VP, C.POINTER(VP), C.POINTER(U64)]),
    ("rbg_wait_text", C.c_int, [VP, VP]),
    ("rbg_release_text", C.c_int, [VP, VP]),
    ("rbg_reserve_text", C.c_int, [VP, U64, C.c_int]),
    ("rbg_convert_runs", C.c_int, [VP, VP, U64, VP, VP, C.c_char_p]),
    ("rbg_convert_runs_markers", C.c_int, [VP, VP, U64, VP, VP, VP, VP, U64, VP, VP, C.c_char_p, C.c_char_p]),
    ("rbg_write_ftab", C.c_int, [VP, U64, C.c_char_p]),
    ("rbg_check_ftab", C.c_int, [VP, C.c_char_p, C.POINTER(U64)]),
    ("rbg_set_markers", C.c_int, [VP, VP, VP, U64, VP, VP]),
    ("rbg_set_docs", C.c_int, [VP, C.c_char_p, VP, U64]),
    ("rbg_free", None, [VP]),
    ("rbg_info", C.c_int, [VP, C.POINTER(Info)]),
    ("rbg_info_sized", C.c_int, [VP, C.POINTER(Info), U64]),
    ("rbg_layout_info", C.c_int, [VP, C.POINTER(LayoutInfo), U64]),
    ("rbg_jump_info", C.c_int, [VP, C.POINTER(JumpInfo)]),
    ("rbg_jump_info_sized", C.c_int, [VP, C.POINTER(JumpInfo), U64]),
    ("rbg_get_f", C.c_int, [VP, VP]),
    ("rbg_last_run_sample", C.c_int, [VP, C.POINTER(U64)]),
    ("rbg_host_array", C.c_int, [VP, C.c_int, VP, U64, C.POINTER(U64)]),
    ("rbg_lf", C.c_int, [VP, VP, VP, VP, U64, VP, VP]),
    ("rbg_find_range", C.c_int, [VP, VP, VP, U64, VP, VP]),
    ("rbg_count", C.c_int, [VP, VP, VP, U64, VP]),
    ("rbg_find_range_w_toehold", C.c_int, [VP, VP, VP, U64, VP, VP, VP]),
    ("rbg_find_range_spans", C.c_int, [VP, VP, VP, VP, U64, VP, VP, VP]),
    ("rbg_locs_at", C.c_int, [VP, VP, VP, VP, U64, U64, VP, C.POINTER(VP)]),
    ("rbg_markers_at", C.c_int, [VP, VP, VP, U64, VP, C.POINTER(VP)]),
    ("rbg_find_range_w_markers", C.c_int, [VP, VP, VP, U64, U64, U64, VP, VP, VP, C.POINTER(VP)]),
    ("rbg_get_markers_greedy_seeding", C.c_int, [VP, VP, VP, U64, U64, U64, U64, VP, C.POINTER(VP), C.POINTER(VP)]),
    ("rbg_greedy_longest_seed", C.c_int, [VP, VP, VP, U64, U64, VP, VP, VP, VP, VP]),
    ("rbg_find_locs_greedy_seeding", C.c_int, [VP, VP, VP, U64, U64, U64, VP, C.POINTER(VP)]),
    ("rbg_free_buffer", None, [VP]),
    ("rbg_resolve_offset", C.c_int, [VP, U64, C.POINTER(C.c_char_p), C.POINTER(U64)]),
    ("rbg_find_range_dev", C.c_int, [VP, VP, VP, U64, VP, VP, VP]),
    ("rbg_find_range_w_toehold_dev", C.c_int, [VP, VP, VP, U64, VP, VP, VP, VP]),
    ("rbg_pack_ws_bytes", C.c_size_t, [U64, U64]),
    ("rbg_pack_reads_dev", C.c_int, [VP, VP, VP, U64, U64, VP, C.c_size_t, VP]),
    ("rbg_find_range_packed_dev", C.c_int, [VP, VP, VP, VP, U64, U64, VP, VP, VP]),
    ("rbg_find_range_w_toehold_packed_dev", C.c_int, [VP, VP, VP, VP, U64, U64, VP, VP, VP, VP]),
    ("rbg_locate_plan_tmp_bytes", C.c_size_t, [U64]),
    ("rbg_locate_plan_dev", C.c_int, [VP, VP, VP, U64, U64, VP, VP, C.c_size_t, VP]),
    ("rbg_locate_order_ws_bytes", C.c_size_t, [U64]),
    ("rbg_locate_order_dev", C.c_int, [VP, VP, U64, VP, C.c_size_t, VP]),
    ("rbg_locate_fill_dev", C.c_int, [VP, VP, VP, VP, U64, U64, VP, VP, VP, VP]),
    ("rbg_locate_fill_offset_dev", C.c_int, [VP, VP, VP, VP, U64, U64, VP, VP, VP, VP, VP]),
    ("rbg_greedy_longest_seed_dev", C.c_int, [VP, VP, VP, U64, U64, VP, VP, VP, VP, VP, VP]),
    ("rbg_marker_seeds_plan_dev", C.c_int, [VP, VP, VP, U64, U64, U64, U64, VP, VP, VP, C.c_size_t, VP]),
    ("rbg_marker_seeds_fill_dev", C.c_int, [VP, VP, VP, U64, U64, U64, U64, VP, VP, VP, VP, VP]),
    ("rbg_markers_plan_dev", C.c_int, [VP, VP, VP, U64, VP, VP, C.c_size_t, VP]),
    ("rbg_markers_fill_dev", C.c_int, [VP, VP, VP, U64, VP, VP, VP]),
    ("rbg_marker_seeds_log_bytes", C.c_size_t, [VP, U64, C.c_uint32]),
    ("rbg_marker_seeds_plan_log_dev", C.c_int, [VP, VP, VP, U64, U64, U64, U64, VP, VP, VP, C.c_size_t, VP, C.c_size_t, VP]),
    ("rbg_marker_seeds_fill_log_dev", C.c_int, [VP, VP, VP, U64, U64, U64, U64, VP, VP, VP, VP, VP, C.c_size_t, VP]),
    ("rbg_locate_fill_dev32", C.c_int, [VP, VP, VP, VP, U64, U64, VP, VP, VP, VP]),
    ("rbg_greedy_longest_seed_stats_dev", C.c_int, [VP, VP, VP, U64, U64, VP, VP, VP, VP, VP, VP, VP]),
    ("rbg_marker_seeds_stats_dev", C.c_int, [VP, VP, VP, U64, U64, U64, VP, VP, VP, C.c_size_t, VP, VP, VP, VP]),
    ("rbg_find_range_stats_dev", C.c_int, [VP, VP, VP, U64, VP, VP, VP, VP, VP]),
    ("rbg_locate_fill_stats_dev", C.c_int, [VP, VP, VP, VP, U64, U64, VP, VP, VP, VP, VP]),
    ("rbg_sample_reads_dev", C.c_int, [VP, U64, U64, U64, U64, U64, U64, U64, C.c_uint32, VP, VP, VP, VP]),
    ("rbg_sample_reads_pangenome_dev", C.c_int, [VP, VP, VP, VP, U64, VP, C.c_uint32, U64, U64, U64, U64, U64, U64, U64, C.c_uint32, VP, VP, VP, VP]),
    ("rbg_replicate", C.c_int, [VP, C.c_int, C.POINTER(VP)]),
    ("rbg_replicate_many", C.c_int, [VP, C.POINTER(C.c_int), C.c_int, C.POINTER(VP)]),
    ("rbg_replicate_stats", C.c_int, [VP, C.POINTER(C.c_double)]),
    ("rbg_replica_pointer_check", C.c_int, [VP, VP]),
    ("rbg_comm_cache_clear", C.c_int, []),
    ("rbg_shard_bounds", C.c_int, [U64, C.c_int, C.c_int, C.POINTER(U64), C.POINTER(U64)]),
    ("rbg_find_range_sharded", C.c_int, [VP, C.c_int, VP, VP, U64, VP, VP, VP]),
    ("rbg_counters_allreduce", C.c_int, [VP, VP, VP, VP]),
    ("rbg_counters_allreduce_local", C.c_int, [VP, C.c_int, VP]),
    ("rbg_counters", C.c_int, [VP, VP]),
    ("rbg_counters_reset", C.c_int, [VP]),
    ("rbg_combine_stats", C.c_int, [VP, VP]),
    ("rbg_get_markers_lmems", C.c_int, [VP, VP, VP, U64, U64, U64, U64, VP, C.POINTER(VP), C.POINTER(VP)]),
    ("rbg_marker_lmems_tmp_bytes", C.c_size_t, [U64, U64]),
    ("rbg_marker_lmems_plan_dev", C.c_int, [VP, VP, VP, U64, U64, U64, U64, U64, VP, VP, C.c_size_t, VP]),
    ("rbg_marker_lmems_fill_dev", C.c_int, [VP, VP, VP, U64, U64, U64, U64, U64, VP, VP, VP, VP]),
    ("rbg_get_seeds_greedy", C.c_int, [VP, VP, VP, U64, U64, C.c_uint32, VP, C.POINTER(VP)]),
    ("rbg_greedy_seeds_tmp_bytes", C.c_size_t, [U64]),
    ("rbg_greedy_seeds_plan_dev", C.c_int, [VP, VP, VP, U64, U64, C.c_uint32, VP, VP, C.c_size_t, VP]),
    ("rbg_greedy_seeds_fill_dev", C.c_int, [VP, VP, VP, U64, U64, C.c_uint32, VP, VP, VP, VP, VP, VP, VP]),
    ("rbg_find_range_w_toehold_chkpnts", C.c_int, [VP, VP, VP, U64, U64, VP, C.POINTER(VP)]),
    ("rbg_toehold_chkpnts_tmp_bytes", C.c_size_t, [U64]),
    ("rbg_toehold_chkpnts_slots_dev", C.c_int, [VP, VP, U64, U64, VP, VP, C.c_size_t, VP]),
    ("rbg_find_range_w_toehold_chkpnts_dev", C.c_int, [VP, VP, VP, U64, U64, VP, VP, VP, VP, VP, VP, VP, VP]),
    ("rbg_set_text_markers", C.c_int, [VP, VP, VP, U64, VP, VP]),
    ("rbg_load_text_markers", C.c_int, [VP, C.c_char_p]),
    ("rbg_loc_markers_tmp_bytes", C.c_size_t, [U64]),
    ("rbg_loc_markers_plan_dev", C.c_int, [VP, VP, VP, VP, U64, VP, VP, C.c_size_t, VP]),
    ("rbg_loc_markers_fill_dev", C.c_int, [VP, VP, VP, VP, U64, VP, VP, VP]),
    ("rbg_markers_at_locs", C.c_int, [VP, VP, VP, VP, U64, VP, C.POINTER(VP)]),
    ("rbg_find_loc_markers_greedy_seeding", C.c_int, [VP, VP, VP, U64, U64, U64, VP, C.POINTER(VP), VP, C.POINTER(VP)]),
    ("rbg_read_strands_bytes", C.c_size_t, [U64]),
    ("rbg_read_strands_dev", C.c_int, [VP, VP, VP, U64, U64, VP, VP, VP]),
    ("rbg_marker_seeds_canon_tmp_bytes", C.c_size_t, [U64]),
    ("rbg_marker_seeds_canon_dev", C.c_int, [VP, VP, U64, VP, U64, C.c_uint32, U64, VP, C.c_size_t, VP]),
    ("rbg_report_select_tmp_bytes", C.c_size_t, [U64]),
    ("rbg_report_select_dev", C.c_int, [VP, VP, VP, VP, U64, VP, VP, VP, VP, VP, VP, C.c_size_t, VP]),
    ("rbg_markers_report", C.c_int, [VP, VP, VP, U64, VP, VP, VP, C.POINTER(VP), C.POINTER(VP)]),
    ("rbg_markers_report_text", C.c_int, [VP, VP, VP, U64, VP, VP, VP, VP, VP, C.POINTER(VP), C.POINTER(U64)]),
    ("rbg_tally_create", C.c_int, [VP, U64, C.POINTER(VP)]),
    ("rbg_tally_free", None, [VP]),
    ("rbg_tally_reset", C.c_int, [VP]),
    ("rbg_tally_reserve", C.c_int, [VP, U64]),
    ("rbg_tally_add_tmp_bytes", C.c_size_t, [U64]),
    ("rbg_tally_add_dev", C.c_int, [VP, VP, U64, VP, U64, VP, C.c_size_t, VP]),
    ("rbg_markers_tally", C.c_int, [VP, VP, VP, U64, VP, VP, VP]),
    ("rbg_tally_add_entries", C.c_int, [VP, VP, U64]),
    ("rbg_tally_export", C.c_int, [VP, C.POINTER(U64), C.POINTER(VP)]),
    ("rbg_tally_info", C.c_int, [VP, VP]),
    ("rbg_markers_tally_reads", C.c_int, [VP, VP, VP, U64, VP, VP, C.c_uint32, VP]),
    ("rbg_tally_add_reads_tmp_bytes", C.c_size_t, [U64, U64]),
    ("rbg_tally_add_reads_dev", C.c_int, [VP, VP, U64, VP, U64, VP, U64, C.c_uint32, VP, C.c_size_t, VP]),
    ("rbg_tally_read_info", C.c_int, [VP, VP]),
    ("rbg_docs_prepare", C.c_int, [VP]),
    ("rbg_doc_hits_words", C.c_size_t, [VP]),
    ("rbg_resolve_offsets_dev", C.c_int, [VP, VP, U64, VP, VP, VP]),
    ("rbg_resolve_offsets_dev32", C.c_int, [VP, VP, U64, VP, VP, VP]),
    ("rbg_doc_hits_dev", C.c_int, [VP, VP, VP, U64, VP, VP, VP, VP, VP]),
    ("rbg_doc_hits_dev32", C.c_int, [VP, VP, VP, U64, VP, VP, VP, VP, VP]),
    ("rbg_doc_hits", C.c_int, [VP, VP, VP, U64, U64, VP, VP, VP, VP, VP, VP]),
    ("rbg_locate_doc_hits_dev", C.c_int, [VP, VP, VP, VP, U64, U64, VP, VP, VP, VP, VP, VP, VP]),
    ("rbg_doc_hits_locs", C.c_int, [VP, VP, VP, U64, U64, VP, VP, VP, VP, VP, VP, VP]),
    ("rbg_align_sam", C.c_int, [VP, VP, VP, VP, VP, VP, VP, VP, VP, U64, U64, U64, C.c_uint32, C.POINTER(VP), C.POINTER(U64)]),
    ("rbg_sam_header", C.c_int, [VP, C.c_char_p, C.POINTER(VP), C.POINTER(U64)]),
    ("rbg_align_sam_extend", C.c_int, [VP, VP, VP, VP, VP, VP, VP, VP, VP, U64, U64, U64, C.c_uint32, C.c_uint32, C.POINTER(VP), C.POINTER(U64)]),
    ("rbg_extend_left_dev", C.c_int, [VP, VP, VP, U64, VP, VP, VP, VP, U64, C.c_uint32, VP, VP]),
    ("rbg_fl_prepare", C.c_int, [VP]),
    ("rbg_fl_info", C.c_int, [VP, VP]),
    ("rbg_fl_dev", C.c_int, [VP, VP, U64, VP, VP, VP]),
    ("rbg_extend_right_dev", C.c_int, [VP, VP, VP, U64, VP, VP, VP, VP, VP, U64, C.c_uint32, VP, VP]),
    ("rbg_align_sam_extend_both", C.c_int, [VP, VP, VP, VP, VP, VP, VP, VP, VP, U64, U64, U64, C.c_uint32, C.c_uint32, C.POINTER(VP), C.POINTER(U64)]),
    ("rbg_extract_prepare", C.c_int, [VP]),
    ("rbg_extract_info", C.c_int, [VP, VP]),
    ("rbg_isa_dev", C.c_int, [VP, VP, U64, VP, VP]),
    ("rbg_isa", C.c_int, [VP, VP, U64, VP]),
    ("rbg_extract_dev", C.c_int, [VP, VP, VP, VP, U64, VP, VP, VP]),
    ("rbg_extract", C.c_int, [VP, VP, VP, U64, VP, VP]),
    ("rbg_sa_tmp_bytes", C.c_size_t, [U64, C.c_uint32]),
    ("rbg_suffix_array_dev", C.c_int, [VP, U64, VP, C.c_uint32, VP, C.c_size_t, VP]),
    ("rbg_sa_info", C.c_int, [VP]),
    ("rbg_text_runs_tmp_bytes", C.c_size_t, [U64, C.c_uint32]),
    ("rbg_text_runs_plan_dev", C.c_int, [VP, VP, U64, C.c_uint32, VP, C.c_size_t, C.POINTER(U64), VP]),
    ("rbg_text_runs_fill_dev", C.c_int, [VP, VP, U64, C.c_uint32, VP, C.c_size_t, U64, VP, VP, VP, VP, VP]),
    ("rbg_build_from_text", C.c_int, [VP, U64, C.c_int, C.c_int, C.POINTER(VP)]),
    ("rbg_convert_text", C.c_int, [VP, U64, C.c_char_p, C.c_int, C.c_int, C.c_char_p]),
    ("rbg_marker_runs_tmp_bytes", C.c_size_t, [U64, U64, C.c_uint32, C.c_uint32]),
    ("rbg_marker_runs_plan_dev", C.c_int, [VP, U64, C.c_uint32, VP, VP, VP, U64, C.c_uint32, VP, C.c_size_t, C.POINTER(U64), C.POINTER(U64), VP]),
    ("rbg_marker_runs_fill_dev", C.c_int, [VP, U64, C.c_uint32, VP, VP, VP, U64, C.c_uint32, VP, C.c_size_t, U64, U64, VP, VP, VP, VP, VP]),
    ("rbg_build_from_text_markers", C.c_int, [VP, U64, VP, VP, VP, U64, C.c_uint32, C.c_int, C.c_int, C.POINTER(VP)]),
    ("rbg_convert_text_markers", C.c_int, [VP, U64, VP, VP, VP, U64, C.c_uint32, C.c_char_p, C.c_int, C.c_int, C.c_char_p]),
    ("rbg_set_default_option", C.c_int, [C.c_int, C.c_int64]),
    ("rbg_get_default_option", C.c_int, [C.c_int, C.POINTER(C.c_int64)]),
]
EXPORTS = [p[0] for p in _PROTOS]
_OPTIONAL = {"rbg_jump_info", "rbg_jump_info_sized"}

_lib = None


def _one_hip_runtime():
    """A process must run ONE HIP runtime.  PyTorch's ROCm wheels bundle their own copies of the ROCm libraries: when
    torch is imported AFTER librbg.so has pulled in /opt/rocm's, its device initialisation fails ("No HIP GPUs are
    available"); imported first, its runtime is the one librbg.so binds to as well (same sonames) -- the configuration
    bench.py and the tests run.  So, when PyTorch is installed and not loaded yet, load it first (about a second;
    RBG_NO_TORCH_PRELOAD=1 skips this for processes that never touch torch)."""
    import importlib.util
    import sys
    if "torch" in sys.modules or os.environ.get("RBG_NO_TORCH_PRELOAD") == "1":
        return
    try:
        if importlib.util.find_spec("torch") is not None:
            import torch  # noqa: F401
    except Exception:  # noqa: BLE001  (a broken torch install must not keep the library from loading)
        pass


def lib():
    """Load librbg.so.  Fails loudly if the HIP extension has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(_SO):
            raise ImportError(f"{_SO} is missing: build it with `make -C rowbowt_amd/csrc` "
                              "(or __graft_entry__.build()); there is no CPU fallback")
        _one_hip_runtime()
        L = C.CDLL(_SO)
        L.rbg_abi_version.restype = C.c_int
        L.rbg_abi_version.argtypes = []
        have = L.rbg_abi_version()
        if have != ABI_VERSION:   # (the structs above and the option numbers are this ABI's: never bind another one's symbols blindly)
            raise ImportError(f"{_SO} reports ABI {have}, this binding is written against ABI {ABI_VERSION}: rebuild it with `make -C rowbowt_amd/csrc`")
        for name, res, args in _PROTOS:
            if name in _OPTIONAL and not hasattr(L, name):   # (an addition within ABI 3: bound when the library has it)
                continue
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _check(rc, what):
    if rc != 0:
        raise RbgError(rc, what)


def _p(a):
    return a.ctypes.data_as(VP) if a is not None else None


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def pack_reads(reads):
    """list of bytes -> (uint8 concat, uint64 offsets[N+1]): the batch layout of the C-ABI."""
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    if len(reads):
        off[1:] = np.cumsum([len(r) for r in reads], dtype=np.uint64)
    seqs = np.frombuffer(b"".join(reads), dtype=np.uint8).copy() if len(reads) else np.zeros(0, np.uint8)
    return seqs, off


def convert_index(prefix, flags, out_path):
    _check(lib().rbg_convert_index(os.fsencode(prefix), int(flags), os.fsencode(out_path)), "rbg_convert_index")


def convert_raw(bwt, ssa=None, esa=None, mab=None, docs=None, out_path=None):
    e = lambda x: os.fsencode(x) if x else None
    _check(lib().rbg_convert_raw(e(bwt), e(ssa), e(esa), e(mab), e(docs), e(out_path)), "rbg_convert_raw")


def convert_runs(heads, lens, ssa=None, esa=None, out_path=None, markers=None, docs_text=None):
    """the native cache file from a run-length BWT in memory (rbg_convert_runs[_markers]); markers = (start, end, off, vals)"""
    heads = np.ascontiguousarray(heads, dtype=np.uint8)
    lens = np.ascontiguousarray(lens, dtype=np.uint64)
    ssa = None if ssa is None else np.ascontiguousarray(ssa, dtype=np.uint64)
    esa = None if esa is None else np.ascontiguousarray(esa, dtype=np.uint64)
    mk = [None] * 4 if markers is None else [np.ascontiguousarray(a, dtype=np.uint64) for a in markers]
    _check(lib().rbg_convert_runs_markers(_p(heads), _p(lens), len(heads), _p(ssa) if ssa is not None else None, _p(esa) if esa is not None else None,
                                          _p(mk[0]) if markers is not None else None, _p(mk[1]) if markers is not None else None,
                                          len(mk[0]) if markers is not None else 0, _p(mk[2]) if markers is not None else None,
                                          _p(mk[3]) if markers is not None else None, docs_text.encode() if docs_text else None,
                                          os.fsencode(out_path)), "rbg_convert_runs_markers")


SA_INFO = ("rounds", "sorted", "tmp_bytes", "n", "pos_bytes", "tied_after_first")


def _text_bytes(text):
    return np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else np.ascontiguousarray(text, dtype=np.uint8)


def convert_text(text, out_path, docs_text=None, sa=True, device=0):
    """rbg_convert_text: the native cache file from a text in host memory (bytes or uint8 array whose last byte is its unique smallest)"""
    t = _text_bytes(text)
    _check(lib().rbg_convert_text(_p(t), len(t), docs_text.encode() if docs_text else None, int(LoadRbwtFlag.SA) if sa else 0, device, os.fsencode(out_path)),
           "rbg_convert_text")


def sa_info():
    """rbg_sa_info -> dict of SA_INFO: the last suffix-array build of the process"""
    out = np.zeros(8, np.uint64)
    _check(lib().rbg_sa_info(_p(out)), "rbg_sa_info")
    return {k: int(v) for k, v in zip(SA_INFO, out)}


def _pos_bytes_of(n, pos_bytes):
    return pos_bytes or (8 if n >= 0xFFFFFFF0 else 4)


def suffix_array(text, pos_bytes=0):
    """rbg_suffix_array_dev over torch tensors: text uint8[n] on a device (last byte = its unique smallest) -> the suffix array on that device, int32 where
    n < 2^32 - 16 (the bits are unsigned: .view / & 0xFFFFFFFF above 2^31), else int64; pos_bytes = 8 forces int64.  Waits for the current stream"""
    import torch
    n = int(text.numel())
    pb = _pos_bytes_of(n, pos_bytes)
    assert text.dtype == torch.uint8 and text.is_contiguous()
    with torch.cuda.device(text.device):
        sa = torch.empty(max(n, 1), dtype=torch.int32 if pb == 4 else torch.int64, device=text.device)
        nb = lib().rbg_sa_tmp_bytes(n, pb)
        tmp = torch.empty(nb + 256, dtype=torch.uint8, device=text.device)
        at = (-tmp.data_ptr()) % 256
        rc = lib().rbg_suffix_array_dev(text.data_ptr() if n else None, n, sa.data_ptr(), pb, tmp.data_ptr() + at, nb, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    _check(rc, "rbg_suffix_array_dev")
    return sa[:n]


def text_runs(text, sa):
    """rbg_text_runs_plan_dev + rbg_text_runs_fill_dev over torch tensors (text uint8[n], sa int32[n] or int64[n] on its device) -> numpy dict heads u8[R],
    lens, ssa, esa u64[R], n, r: what synth_pangenome.index_inputs gives.  Only the run arrays leave the device"""
    import torch
    n = int(text.numel())
    pb = sa.element_size()
    assert text.dtype == torch.uint8 and text.is_contiguous() and sa.is_contiguous() and int(sa.numel()) == n and pb in (4, 8)
    L = lib()
    with torch.cuda.device(text.device):
        nb = L.rbg_text_runs_tmp_bytes(n, pb)
        tmp = torch.empty(nb + 256, dtype=torch.uint8, device=text.device)
        at = (-tmp.data_ptr()) % 256
        st = torch.cuda.current_stream().cuda_stream
        R = U64()
        _check(L.rbg_text_runs_plan_dev(text.data_ptr(), sa.data_ptr(), n, pb, tmp.data_ptr() + at, nb, C.byref(R), st), "rbg_text_runs_plan_dev")
        r = int(R.value)
        heads = torch.empty(r, dtype=torch.uint8, device=text.device)
        lens, ssa, esa = (torch.empty(r, dtype=torch.int64, device=text.device) for _ in range(3))
        rc = L.rbg_text_runs_fill_dev(text.data_ptr(), sa.data_ptr(), n, pb, tmp.data_ptr() + at, nb, r, heads.data_ptr(), lens.data_ptr(), ssa.data_ptr(),
                                      esa.data_ptr(), st)
        torch.cuda.synchronize()
    _check(rc, "rbg_text_runs_fill_dev")
    u = lambda t: t.cpu().numpy().view(np.uint64).copy()
    return dict(heads=heads.cpu().numpy().copy(), lens=u(lens), ssa=u(ssa), esa=u(esa), n=n, r=r)


def marker_runs(sa, pos, first, val, w, pos_bytes=0):
    """rbg_marker_runs_plan_dev + rbg_marker_runs_fill_dev over torch tensors: sa int32[n] or int64[n] on its device (capi.suffix_array's), the site records
    pos, first, val int64[S] on the same device, 1 <= w <= 64 -> numpy (run_start, run_end, mk_off, mk_vals), uint64: the arguments of set_markers.
    pos_bytes, when given, must be the width of sa.  Only the marker arrays leave the device"""
    import torch
    n, S = int(sa.numel()), int(pos.numel())
    pb = sa.element_size()
    assert sa.is_contiguous() and pb in (4, 8) and pos_bytes in (0, pb)
    for t in (pos, first, val):
        assert t.dtype == torch.int64 and t.is_contiguous() and int(t.numel()) == S and t.device == sa.device
    L = lib()
    with torch.cuda.device(sa.device):
        nb = L.rbg_marker_runs_tmp_bytes(n, S, w, pb)
        tmp = torch.empty(nb + 256, dtype=torch.uint8, device=sa.device)
        at = (-tmp.data_ptr()) % 256
        st = torch.cuda.current_stream().cuda_stream
        ptrs = [t.data_ptr() if S else None for t in (pos, first, val)]
        nruns, nvals = U64(), U64()
        _check(L.rbg_marker_runs_plan_dev(sa.data_ptr(), n, pb, *ptrs, S, w, tmp.data_ptr() + at, nb, C.byref(nruns), C.byref(nvals), st),
               "rbg_marker_runs_plan_dev")
        r, v = int(nruns.value), int(nvals.value)
        run_start, run_end = (torch.empty(max(r, 1), dtype=torch.int64, device=sa.device) for _ in range(2))
        mk_off = torch.empty(r + 1, dtype=torch.int64, device=sa.device)
        mk_vals = torch.empty(max(v, 1), dtype=torch.int64, device=sa.device)
        rc = L.rbg_marker_runs_fill_dev(sa.data_ptr(), n, pb, *ptrs, S, w, tmp.data_ptr() + at, nb, r, v, run_start.data_ptr(), run_end.data_ptr(),
                                        mk_off.data_ptr(), mk_vals.data_ptr(), st)
        torch.cuda.synchronize()
    _check(rc, "rbg_marker_runs_fill_dev")
    u = lambda t, k: t[:k].cpu().numpy().view(np.uint64).copy()
    return u(run_start, r), u(run_end, r), u(mk_off, r + 1), u(mk_vals, v)


def _site_records(markers):
    """(pos, first, val, w) -> three contiguous uint64 arrays of one length, and w"""
    pos, first, val, w = markers
    a = [np.ascontiguousarray(x, dtype=np.uint64) for x in (pos, first, val)]
    if not (len(a[0]) == len(a[1]) == len(a[2])):
        raise ValueError("pos, first and val differ in length")
    return a, int(w)


def convert_text_markers(text, markers, out_path, docs_text=None, sa=True, device=0):
    """rbg_convert_text_markers: convert_text with the marker array of the site records markers = (pos, first, val, w) stored in the cache file"""
    t = _text_bytes(text)
    a, w = _site_records(markers)
    _check(lib().rbg_convert_text_markers(_p(t), len(t), _p(a[0]), _p(a[1]), _p(a[2]), len(a[0]), w, docs_text.encode() if docs_text else None,
                                          int(LoadRbwtFlag.SA) if sa else 0, device, os.fsencode(out_path)), "rbg_convert_text_markers")


def set_default_option(opt, value):
    _check(lib().rbg_set_default_option(opt, value), "rbg_set_default_option")


def get_default_option(opt):
    v = C.c_int64(0)
    _check(lib().rbg_get_default_option(opt, C.byref(v)), "rbg_get_default_option")
    return int(v.value)


class default_option:
    """with default_option(OPT_X, v): ... -- one knob changed for the loads inside, put back afterwards"""

    def __init__(self, opt, value):
        self.opt, self.value = opt, value

    def __enter__(self):
        self.prev = get_default_option(self.opt)
        set_default_option(self.opt, self.value)
        return self

    def __exit__(self, *exc):
        set_default_option(self.opt, self.prev)
        return False


def _take(ptr, n):
    """a library-malloc'ed uint64 result as a numpy array, without copying (gigabytes of locations); the
    buffer is released (rbg_free_buffer) when the last array viewing it is gone"""
    if n == 0 or not ptr.value:
        lib().rbg_free_buffer(ptr)
        return np.zeros(0, dtype=np.uint64)
    mem = (C.c_char * (n * 8)).from_address(ptr.value)
    weakref.finalize(mem, lib().rbg_free_buffer, VP(ptr.value))
    return np.frombuffer(mem, dtype=np.uint64)   # .base is `mem`: every view keeps it alive


class Tally:
    """rbg_tally: per marker, how many of rb_markers' lines carried it (n_fwd, n_rev, len_sum), accumulated on the index's device across calls.
    Close it before its index; feed it from one thread at a time."""

    def __init__(self, rb, distinct_hint=0):
        self.L = lib()
        self.rb = rb   # (keeps the index alive)
        self.h = VP()
        _check(self.L.rbg_tally_create(rb.h, distinct_hint, C.byref(self.h)), "rbg_tally_create")

    def close(self):
        if self.h:
            self.L.rbg_tally_free(self.h)
            self.h = None

    def __del__(self):
        try:
            if self.rb.h:
                self.close()
        except Exception:
            pass

    def reset(self):
        _check(self.L.rbg_tally_reset(self.h), "rbg_tally_reset")

    def reserve(self, extra):
        _check(self.L.rbg_tally_reserve(self.h, extra), "rbg_tally_reserve")

    def add_entries(self, entries):
        """merge: the export of another tally (TALLY_ENTRY records) added into this one"""
        e = np.ascontiguousarray(entries, dtype=TALLY_ENTRY)
        _check(self.L.rbg_tally_add_entries(self.h, _p(e), len(e)), "rbg_tally_add_entries")

    def export(self):
        """-> TALLY_ENTRY records with n_fwd + n_rev > 0, sorted by (sequence, position, allele)"""
        n, ptr = U64(), VP()
        _check(self.L.rbg_tally_export(self.h, C.byref(n), C.byref(ptr)), "rbg_tally_export")
        return _take(ptr, 4 * n.value).view(TALLY_ENTRY)

    def info(self):
        out = np.zeros(6, np.uint64)
        _check(self.L.rbg_tally_info(self.h, _p(out)), "rbg_tally_info")
        return dict(zip(TALLY_INFO, (int(v) for v in out)))

    def read_info(self):
        """rbg_tally_read_info: what the per-read adds saw -- reads, marker elements, elements that lost to another line of their read, elements the
        site rule dropped (elements_seen = the elements these adds added + lost + site_dropped)"""
        out = np.zeros(4, np.uint64)
        _check(self.L.rbg_tally_read_info(self.h, _p(out)), "rbg_tally_read_info")
        return dict(zip(TALLY_READ_INFO, (int(v) for v in out)))


class RowBowt:
    """rbwt::RowBowt<ri::rle_string_sd> (rowbowt.hpp:23-24), batched over N reads."""

    def __init__(self, handle):
        self.h = handle
        self.L = lib()

    def close(self):
        if self.h:
            self.L.rbg_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @classmethod
    def from_runs(cls, heads, lens, ssa=None, esa=None, device=0):
        heads = np.ascontiguousarray(heads, dtype=np.uint8)
        lens = _u64(lens)
        ssa = _u64(ssa) if ssa is not None else None
        esa = _u64(esa) if esa is not None else None
        h = VP()
        _check(lib().rbg_build_from_runs(_p(heads), _p(lens), len(heads), _p(ssa), _p(esa), device, C.byref(h)),
               "rbg_build_from_runs")
        return cls(h)

    @classmethod
    def from_text(cls, text, sa=True, device=0, markers=None):
        """rbg_build_from_text: the index of a text in host memory (bytes or a uint8 array; its last byte is its unique smallest), built on the device:
        suffix array, runs, samples; sa=False keeps no toehold samples.  markers = (pos, first, val, w), the site records of include/rbg.h: the marker
        array is built from them while the suffix array is on the device and set on the index (rbg_build_from_text_markers)"""
        t = _text_bytes(text)
        h = VP()
        if markers is None:
            _check(lib().rbg_build_from_text(_p(t), len(t), int(LoadRbwtFlag.SA) if sa else 0, device, C.byref(h)), "rbg_build_from_text")
            return cls(h)
        a, w = _site_records(markers)
        _check(lib().rbg_build_from_text_markers(_p(t), len(t), _p(a[0]), _p(a[1]), _p(a[2]), len(a[0]), w, int(LoadRbwtFlag.SA) if sa else 0, device,
                                                 C.byref(h)), "rbg_build_from_text_markers")
        return cls(h)

    @classmethod
    def from_files(cls, bwt, ssa=None, esa=None, device=0):
        """rb_build's raw inputs (rb_build.cpp:83-93): <pre>.bwt, <pre>.ssa, <pre>.esa"""
        h = VP()
        _check(lib().rbg_build_from_files(os.fsencode(bwt), os.fsencode(ssa) if ssa else None,
                                          os.fsencode(esa) if esa else None, device, C.byref(h)), "rbg_build_from_files")
        return cls(h)

    def set_markers(self, run_start, run_end, mk_off, mk_vals):
        a = [_u64(v) for v in (run_start, run_end, mk_off, mk_vals)]
        _check(self.L.rbg_set_markers(self.h, _p(a[0]), _p(a[1]), len(a[0]), _p(a[2]), _p(a[3])), "rbg_set_markers")

    def set_text_markers(self, run_start, run_end, mk_off, mk_vals):
        """the marker table keyed by TEXT position (rb_locs' .midx): runs of text positions in [0, n); replaces the one set before"""
        a = [_u64(v) for v in (run_start, run_end, mk_off, mk_vals)]
        _check(self.L.rbg_set_text_markers(self.h, _p(a[0]), _p(a[1]), len(a[0]), _p(a[2]), _p(a[3])), "rbg_set_text_markers")

    def load_text_markers(self, path):
        _check(self.L.rbg_load_text_markers(self.h, os.fsencode(path)), f"rbg_load_text_markers({path})")

    def set_docs(self, names, starts):
        joined = b"\0".join(n.encode() for n in names) + b"\0"
        s = _u64(starts)
        _check(self.L.rbg_set_docs(self.h, joined, _p(s), len(names)), "rbg_set_docs")

    @classmethod
    def from_cache(cls, path, flags=LoadRbwtFlag.NONE, device=0):
        """native cache file written by convert_index / convert_raw / rb_build (include/rbg.h, next-row f1)"""
        h = VP()
        _check(lib().rbg_load_cache(os.fsencode(path), int(flags), device, C.byref(h)), "rbg_load_cache")
        return cls(h)

    def write_ftab(self, k, path):
        """RowBowt::build_ftab(k) + FTab::serialize (rowbowt.hpp:726-744, ftab.hpp:29-34)"""
        _check(self.L.rbg_write_ftab(self.h, k, os.fsencode(path)), "rbg_write_ftab")

    def check_ftab(self, path):
        """-> k of a .ftab file that is exactly build_ftab(k) of this index (LoadRbwtFlag::FT), else RbgError"""
        k = U64()
        _check(self.L.rbg_check_ftab(self.h, os.fsencode(path), C.byref(k)), "rbg_check_ftab")
        return k.value

    # ---- introspection
    def info(self):
        i = Info()
        _check(self.L.rbg_info(self.h, C.byref(i)), "rbg_info")
        return i

    def jump_info(self):
        """the jump table of this replica (rbg_jump_info_t; all zero when none was built)"""
        i = JumpInfo()
        if hasattr(self.L, "rbg_jump_info_sized"):
            _check(self.L.rbg_jump_info_sized(self.h, C.byref(i), C.sizeof(i)), "rbg_jump_info_sized")
        else:   # (a library of before level 2: its five fields; the rest stay zero)
            _check(self.L.rbg_jump_info(self.h, C.byref(i)), "rbg_jump_info")
        return i

    def jump_complete(self):
        """the levels of this replica's jump table that are complete (rbg_jump_info_t.complete: bit 0 = level 1, bit 1 = level 2; 0 without a table,
        under RBG_JUMP_ABSENT_ENDS=0, or from a library of before the field)"""
        i = JumpInfoComplete()
        if hasattr(self.L, "rbg_jump_info_sized"):
            _check(self.L.rbg_jump_info_sized(self.h, C.cast(C.byref(i), C.POINTER(JumpInfo)), C.sizeof(i)), "rbg_jump_info_sized")
        return int(i.complete)

    def layout_info(self):
        """what the load decided about the run-indexed layout (rbg_layout_info_t; all zero on the slot layout)"""
        i = LayoutInfo()
        _check(self.L.rbg_layout_info(self.h, C.byref(i), C.sizeof(i)), "rbg_layout_info")
        return i

    def get_f(self):
        out = np.zeros(256, dtype=np.uint64)
        _check(self.L.rbg_get_f(self.h, _p(out)), "rbg_get_f")
        return out

    def last_run_sample(self):
        v = U64()
        _check(self.L.rbg_last_run_sample(self.h, C.byref(v)), "rbg_last_run_sample")
        return v.value

    def host_array(self, which):
        cnt = U64()
        _check(self.L.rbg_host_array(self.h, which, None, 0, C.byref(cnt)), "rbg_host_array")
        out = np.zeros(cnt.value, dtype=np.uint64)
        _check(self.L.rbg_host_array(self.h, which, _p(out), cnt.value, C.byref(cnt)), "rbg_host_array")
        return out

    # ---- queries (host buffers)
    def LF(self, lo, hi, sym):
        """RowBowt::LF(range_t, uint8_t), rowbowt.hpp:74-88, for N triples"""
        lo, hi = _u64(lo), _u64(hi)
        sym = np.ascontiguousarray(sym, dtype=np.uint8)
        N = len(lo)
        nlo, nhi = np.zeros(N, np.uint64), np.zeros(N, np.uint64)
        _check(self.L.rbg_lf(self.h, _p(lo), _p(hi), _p(sym), N, _p(nlo), _p(nhi)), "rbg_lf")
        return nlo, nhi

    def find_range(self, seqs, off):
        N = len(off) - 1
        lo, hi = np.zeros(N, np.uint64), np.zeros(N, np.uint64)
        _check(self.L.rbg_find_range(self.h, _p(seqs), _p(off), N, _p(lo), _p(hi)), "rbg_find_range")
        return lo, hi

    def count(self, seqs, off):
        N = len(off) - 1
        cnt = np.zeros(N, np.uint64)
        _check(self.L.rbg_count(self.h, _p(seqs), _p(off), N, _p(cnt)), "rbg_count")
        return cnt

    def find_range_spans(self, buf, begin, length, toehold=False):
        """reads as spans of one host buffer (rbg_find_range_spans)"""
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        begin = _u64(begin)
        length = np.ascontiguousarray(length, dtype=np.uint32)
        N = len(begin)
        lo, hi = np.zeros(N, np.uint64), np.zeros(N, np.uint64)
        k = np.zeros(N, np.uint64) if toehold else None
        _check(self.L.rbg_find_range_spans(self.h, _p(buf), _p(begin), _p(length), N, _p(lo), _p(hi), _p(k)), "rbg_find_range_spans")
        return (lo, hi, k) if toehold else (lo, hi)

    def find_range_w_toehold(self, seqs, off):
        N = len(off) - 1
        lo, hi, k = np.zeros(N, np.uint64), np.zeros(N, np.uint64), np.zeros(N, np.uint64)
        _check(self.L.rbg_find_range_w_toehold(self.h, _p(seqs), _p(off), N, _p(lo), _p(hi), _p(k)),
               "rbg_find_range_w_toehold")
        return lo, hi, k

    def locs_at(self, lo, hi, k, max_hits=MAXU):
        lo, hi, k = _u64(lo), _u64(hi), _u64(k)
        N = len(lo)
        loc_off = np.zeros(N + 1, np.uint64)
        ptr = VP()
        _check(self.L.rbg_locs_at(self.h, _p(lo), _p(hi), _p(k), N, max_hits, _p(loc_off), C.byref(ptr)), "rbg_locs_at")
        return loc_off, _take(ptr, int(loc_off[N]))

    def markers_at(self, lo, hi):
        lo, hi = _u64(lo), _u64(hi)
        N = len(lo)
        mk_off = np.zeros(N + 1, np.uint64)
        ptr = VP()
        _check(self.L.rbg_markers_at(self.h, _p(lo), _p(hi), N, _p(mk_off), C.byref(ptr)), "rbg_markers_at")
        return mk_off, _take(ptr, int(mk_off[N]))

    def find_range_w_markers(self, seqs, off, wsize, max_range=MAXU):
        N = len(off) - 1
        lo, hi, mk_off = np.zeros(N, np.uint64), np.zeros(N, np.uint64), np.zeros(N + 1, np.uint64)
        ptr = VP()
        _check(self.L.rbg_find_range_w_markers(self.h, _p(seqs), _p(off), N, wsize, max_range & MAXU,
                                               _p(lo), _p(hi), _p(mk_off), C.byref(ptr)), "rbg_find_range_w_markers")
        return lo, hi, mk_off, _take(ptr, int(mk_off[N]))

    def get_markers_greedy_seeding(self, seqs, off, wsize, max_range=MAXU, ftab_k=0):
        """RowBowt::get_markers_greedy_seeding (rowbowt.hpp:406-482), ftab_k = k-mer size of the loaded
        ftab or 0: -> seed_off[N+1], seeds[S,6] = (lo, hi, qstart, qend, mk_begin, mk_end), mk"""
        N = len(off) - 1
        seed_off = np.zeros(N + 1, np.uint64)
        ps, pm = VP(), VP()
        _check(self.L.rbg_get_markers_greedy_seeding(self.h, _p(seqs), _p(off), N, wsize, max_range & MAXU, ftab_k, _p(seed_off),
                                                     C.byref(ps), C.byref(pm)), "rbg_get_markers_greedy_seeding")
        S = int(seed_off[N])
        seeds = _take(ps, 6 * S).reshape(S, 6)
        nmk = int(seeds[-1, 5]) if S else 0
        return seed_off, seeds, _take(pm, nmk)

    def get_markers_lmems(self, seqs, off, wsize, max_range=MAXU, ftab_k=0):
        """RowBowt::get_markers_lmems (rowbowt.hpp:341-404): one record per end position m, m-1, ..., 1 of each sequence (the
        non-empty calls of the callback), ftab_k = k-mer size of the ftab or 0: -> seed_off[N+1] (== off), seeds[S,6] =
        (lo, hi, qstart, qend, mk_begin, mk_end), mk"""
        N = len(off) - 1
        seed_off = np.zeros(N + 1, np.uint64)
        ps, pm = VP(), VP()
        _check(self.L.rbg_get_markers_lmems(self.h, _p(seqs), _p(off), N, wsize, max_range & MAXU, ftab_k, _p(seed_off),
                                            C.byref(ps), C.byref(pm)), "rbg_get_markers_lmems")
        S = int(seed_off[N])
        seeds = _take(ps, 6 * S).reshape(S, 6)
        nmk = int(seeds[-1, 5]) if S else 0
        return seed_off, seeds, _take(pm, nmk)

    def _seed_arrays(self, seed_off, ptr):
        S = int(seed_off[-1])
        a = _take(ptr, 5 * S).reshape(5, S)
        return (seed_off,) + tuple(a[t] for t in range(5))

    def get_seeds_greedy(self, seqs, off, min_length, w_sample=True):
        """RowBowt::get_seeds_greedy_w_sample (rowbowt.hpp:222-256) or, w_sample=False, get_seeds_greedy (:191-215): every greedy
        seed of every read, the rightmost first -> (seed_off[N+1], lo, hi, qstart, qend, ssamp), five arrays of seed_off[N]"""
        N = len(off) - 1
        seed_off = np.zeros(N + 1, np.uint64)
        ptr = VP()
        _check(self.L.rbg_get_seeds_greedy(self.h, _p(seqs), _p(off), N, min_length, SEEDS_W_SAMPLE if w_sample else 0, _p(seed_off),
                                           C.byref(ptr)), "rbg_get_seeds_greedy")
        return self._seed_arrays(seed_off, ptr)

    def find_range_w_toehold_chkpnts(self, seqs, off, wsize):
        """RowBowt::find_range_w_toehold_chkpnts (rowbowt.hpp:575-606): a record every wsize steps of each read's backward search
        and the whole read's at the end -> (seed_off[N+1], lo, hi, qstart, qend, ssamp); a read that does not occur has none"""
        N = len(off) - 1
        seed_off = np.zeros(N + 1, np.uint64)
        ptr = VP()
        _check(self.L.rbg_find_range_w_toehold_chkpnts(self.h, _p(seqs), _p(off), N, wsize, _p(seed_off), C.byref(ptr)),
               "rbg_find_range_w_toehold_chkpnts")
        return self._seed_arrays(seed_off, ptr)

    def greedy_longest_seed(self, seqs, off, min_length):
        """get_seeds_greedy_w_sample (rowbowt.hpp:222-256) -> the seed locate_from_longest_seed picks (:669-677)"""
        N = len(off) - 1
        a = [np.zeros(N, np.uint64) for _ in range(5)]
        _check(self.L.rbg_greedy_longest_seed(self.h, _p(seqs), _p(off), N, min_length, *[_p(x) for x in a]),
               "rbg_greedy_longest_seed")
        return a  # lo, hi, qstart, qend, ssamp

    def find_locs_greedy_seeding(self, seqs, off, min_length, max_hits=MAXU):
        """RowBowt::find_locs_greedy_seeding, rowbowt.hpp:633-657"""
        N = len(off) - 1
        loc_off = np.zeros(N + 1, np.uint64)
        ptr = VP()
        _check(self.L.rbg_find_locs_greedy_seeding(self.h, _p(seqs), _p(off), N, min_length, max_hits, _p(loc_off), C.byref(ptr)),
               "rbg_find_locs_greedy_seeding")
        return loc_off, _take(ptr, int(loc_off[N]))

    def markers_at_locs(self, locs, loc_off, off):
        """markers of the text-position table over [l, l + m_i - 1] for every location l of read i: (mk_off[N+1] per read, values)"""
        locs, loc_off, off = _u64(locs), _u64(loc_off), _u64(off)
        N = len(off) - 1
        mk_off = np.zeros(N + 1, np.uint64)
        ptr = VP()
        _check(self.L.rbg_markers_at_locs(self.h, _p(locs), _p(loc_off), _p(off), N, _p(mk_off), C.byref(ptr)), "rbg_markers_at_locs")
        return mk_off, _take(ptr, int(mk_off[N]))

    def find_loc_markers_greedy_seeding(self, seqs, off, min_length, max_hits=MAXU):
        """one read of rb_locs, batched (rb_markers_tsa.cpp:76-88): (loc_off, locs, mk_off, mk)"""
        N = len(off) - 1
        loc_off, mk_off = np.zeros(N + 1, np.uint64), np.zeros(N + 1, np.uint64)
        lp, mp = VP(), VP()
        _check(self.L.rbg_find_loc_markers_greedy_seeding(self.h, _p(seqs), _p(off), N, min_length, max_hits, _p(loc_off), C.byref(lp),
                                                          _p(mk_off), C.byref(mp)), "rbg_find_loc_markers_greedy_seeding")
        return loc_off, _take(lp, int(loc_off[N])), mk_off, _take(mp, int(mk_off[N]))

    def resolve_offset(self, i):
        name, off = C.c_char_p(), U64()
        _check(self.L.rbg_resolve_offset(self.h, i, C.byref(name), C.byref(off)), "rbg_resolve_offset")
        return name.value.decode(), off.value

    def docs_prepare(self):
        """rbg_docs_prepare: the document table and its directory on this handle's device (idempotent; again after every set_docs)"""
        _check(self.L.rbg_docs_prepare(self.h), "rbg_docs_prepare")

    def doc_hits_words(self):
        """W = ceil(ndocs / 64): the u64 words of one read's document set"""
        return int(self.L.rbg_doc_hits_words(self.h))

    def resolve_offsets(self, locs):
        """resolve_offset for an array of text positions, on the device (rbg_resolve_offsets_dev): -> (doc[M] uint32, DOC_NONE where a position has
        no document, offset[M] uint64).  doc indexes rbg_doc_table's names.  The arrays cross to the device and back through torch"""
        import torch
        locs = _u64(locs)
        M = len(locs)
        self.docs_prepare()
        info = self.info()
        with torch.cuda.device(info.device):
            d_locs = torch.from_numpy(locs.view(np.int64)).cuda()
            d_doc = torch.empty(max(M, 1), dtype=torch.int32, device="cuda")
            d_off = torch.empty(max(M, 1), dtype=torch.int64, device="cuda")
            st = torch.cuda.current_stream().cuda_stream
            _check(self.L.rbg_resolve_offsets_dev(self.h, d_locs.data_ptr() if M else None, M, d_doc.data_ptr(), d_off.data_ptr(), st), "rbg_resolve_offsets_dev")
            torch.cuda.synchronize()
            return d_doc[:M].cpu().numpy().view(np.uint32), d_off[:M].cpu().numpy().view(np.uint64)

    def locate_doc_hits(self, d_lo, d_hi, d_k, max_hits=MAXU, order=True, doc_locs=False):
        """rbg_locate_doc_hits_dev on device tensors (int64 [N]: what rbg_find_range_w_toehold_dev wrote): the chains walked and reduced in one kernel, no
        location stored -> (sets[N, W] int64, ndocs[N] int32, nodoc[N] int32, doc_reads[ndocs] int64[, doc_locs[ndocs] int64]) on the same device, the bit
        patterns of rbg_doc_hits' outputs.  order: sort the chains by toehold first (rbg_locate_order_dev).  The table must be prepared (docs_prepare)"""
        import torch
        N = int(d_lo.numel())
        W = self.doc_hits_words()
        nd = self.doc_table(names=False)[0]
        with torch.cuda.device(d_lo.device):
            st = torch.cuda.current_stream().cuda_stream
            ws = None
            if order and N:
                ws_bytes = int(self.L.rbg_locate_order_ws_bytes(N))
                ws = torch.empty(ws_bytes, dtype=torch.uint8, device=d_lo.device)
                _check(self.L.rbg_locate_order_dev(self.h, d_k.data_ptr(), N, ws.data_ptr(), ws_bytes, st), "rbg_locate_order_dev")
            sets = torch.zeros((N, W), dtype=torch.int64, device=d_lo.device)
            ndocs, nodoc = (torch.zeros(N, dtype=torch.int32, device=d_lo.device) for _ in range(2))
            reads = torch.zeros(nd, dtype=torch.int64, device=d_lo.device)
            locs = torch.zeros(nd, dtype=torch.int64, device=d_lo.device) if doc_locs else None
            _check(self.L.rbg_locate_doc_hits_dev(self.h, d_lo.data_ptr(), d_hi.data_ptr(), d_k.data_ptr(), N, max_hits, ws.data_ptr() if ws is not None else None,
                                                  sets.data_ptr(), ndocs.data_ptr(), nodoc.data_ptr(), reads.data_ptr(),
                                                  locs.data_ptr() if doc_locs else None, st), "rbg_locate_doc_hits_dev")
        return (sets, ndocs, nodoc, reads, locs) if doc_locs else (sets, ndocs, nodoc, reads)

    def doc_hits(self, seqs, off, max_hits=MAXU, doc_locs=False):
        """rbg_doc_hits: per read its range and the SET of documents its locations (locs_at with max_hits) fall in, the locations staying on the
        device -> (lo, hi, sets[N, W] uint64 -- bit d % 64 of word d / 64 = document d --, ndocs[N], nodoc[N] uint32, doc_reads[ndocs] uint64 = the
        reads of this batch that hit each document).  doc_locs=True (rbg_doc_hits_locs): one more array, doc_locs[ndocs] uint64 = the locations of this
        batch in each document"""
        seqs, off = np.ascontiguousarray(seqs, dtype=np.uint8), _u64(off)
        N = len(off) - 1
        self.docs_prepare()
        W = self.doc_hits_words()
        nd = self.doc_table(names=False)[0]
        lo, hi = np.zeros(N, np.uint64), np.zeros(N, np.uint64)
        sets = np.zeros((N, W), np.uint64)
        ndocs, nodoc = np.zeros(N, np.uint32), np.zeros(N, np.uint32)
        doc_reads = np.zeros(nd, np.uint64)
        if doc_locs:
            dl = np.zeros(nd, np.uint64)
            _check(self.L.rbg_doc_hits_locs(self.h, _p(seqs), _p(off), N, max_hits, _p(lo), _p(hi), _p(sets), _p(ndocs), _p(nodoc), _p(doc_reads), _p(dl)),
                   "rbg_doc_hits_locs")
            return lo, hi, sets, ndocs, nodoc, doc_reads, dl
        _check(self.L.rbg_doc_hits(self.h, _p(seqs), _p(off), N, max_hits, _p(lo), _p(hi), _p(sets), _p(ndocs), _p(nodoc), _p(doc_reads)), "rbg_doc_hits")
        return lo, hi, sets, ndocs, nodoc, doc_reads

    def doc_table(self, names=True):
        """rbg_doc_table: (ndocs, sorted_starts uint64[ndocs], names (None when not asked for), size)"""
        nd, size, ps, pn = U64(), U64(), VP(), VP()
        _check(self.L.rbg_doc_table(self.h, C.byref(nd), C.byref(ps), C.byref(pn), C.byref(size)), "rbg_doc_table")
        n = int(nd.value)
        starts = np.ctypeslib.as_array(C.cast(ps, C.POINTER(U64)), shape=(n,)).copy()
        got = [C.cast(pn, C.POINTER(C.c_char_p))[j].decode() for j in range(n)] if names else None
        return n, starts, got, int(size.value)

    def align_text(self, lo, hi, k, names, max_hits=MAXU, markers=False):
        """rbg_align_text: the `rb_align -s` text of a batch (bytes), made on the device; names = list of bytes"""
        lo, hi = (np.ascontiguousarray(a, dtype=np.uint64) for a in (lo, hi))
        k = None if k is None else np.ascontiguousarray(k, dtype=np.uint64)   # None: the count-only report
        blob = b"".join(names)
        nlen = np.array([len(x) for x in names], dtype=np.uint32)
        nbeg = np.zeros(len(names), dtype=np.uint64)
        if len(names) > 1:
            nbeg[1:] = np.cumsum(nlen[:-1], dtype=np.uint64)
        buf = C.create_string_buffer(blob, len(blob) + 1)
        text, n = VP(), U64()
        _check(self.L.rbg_align_text(self.h, _p(lo), _p(hi), _p(k) if k is not None else None, len(names), max_hits, 1 if markers else 0, buf, _p(nbeg), _p(nlen), C.byref(text), C.byref(n)), "rbg_align_text")
        try:
            _check(self.L.rbg_wait_text(self.h, text), "rbg_wait_text")
            return C.string_at(text, n.value)
        finally:
            self.L.rbg_release_text(self.h, text)

    def align_sam_extend(self, seqs, quals, names, min_length=20, max_hits=16, secondary=False, max_mismatch=4, right=False):
        """rbg_align_sam_extend: align_sam's lines with every seed extended leftwards through up to max_mismatch mismatches by an LF walk (POS and the left
        clip move, NM / MD / AS follow HI on every mapped line); right=True: rbg_align_sam_extend_both, the right clip extended too by an FL walk with what
        the left walk left of the budget (fl_prepare first)"""
        return self._sam_lines(seqs, quals, names, min_length, max_hits, secondary, max_mismatch, right)

    def fl_prepare(self):
        """rbg_fl_prepare: the FL index (per-base run lists keyed by rank, and their directories) on this handle's device; idempotent, opt-in"""
        _check(self.L.rbg_fl_prepare(self.h), "rbg_fl_prepare")

    def fl_info(self):
        """rbg_fl_info -> dict: prepared, bytes, runs (A C G T), shift (A C G T), dir_entries"""
        out = np.zeros(8, np.uint64)
        _check(self.L.rbg_fl_info(self.h, _p(out)), "rbg_fl_info")
        return dict(prepared=bool(out[0]), bytes=int(out[1]), runs=[int(v) for v in out[2:6]], shift=[(int(out[6]) >> (8 * j)) & 0xFF for j in range(4)],
                    dir_entries=int(out[7]))

    def fl(self, rows):
        """rbg_fl_dev: (sym uint8[M], next uint64[M]) -- the F byte of each row (0: not one of A C G T) and FL(row) (2^64 - 1 then).  Through torch"""
        import torch
        rows = _u64(rows)
        M = len(rows)
        with torch.cuda.device(self.info().device):
            d_rows = torch.from_numpy(rows.view(np.int64)).cuda()
            d_sym = torch.full((max(M, 1),), 0xA5, dtype=torch.uint8, device="cuda")
            d_next = torch.full((max(M, 1),), -6, dtype=torch.int64, device="cuda")
            rc = self.L.rbg_fl_dev(self.h, d_rows.data_ptr() if M else None, M, d_sym.data_ptr(), d_next.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            sym, nxt = d_sym.cpu().numpy()[:M].copy(), d_next.cpu().numpy()[:M].view(np.uint64).copy()
        _check(rc, "rbg_fl_dev")
        return sym, nxt

    def extract_prepare(self):
        """rbg_extract_prepare: the ISA sample (text position -> row, by samples and an FL walk) on this handle's device; runs fl_prepare if needed;
        idempotent, opt-in"""
        _check(self.L.rbg_extract_prepare(self.h), "rbg_extract_prepare")

    def extract_info(self):
        """rbg_extract_info -> dict: prepared, bytes, samples, shift, dir_entries, second_kind, max_gap, build_us"""
        out = np.zeros(8, np.uint64)
        _check(self.L.rbg_extract_info(self.h, _p(out)), "rbg_extract_info")
        keys = ("bytes", "samples", "shift", "dir_entries", "second_kind", "max_gap", "build_us")
        return dict(prepared=bool(out[0]), **{k: int(v) for k, v in zip(keys, out[1:])})

    def isa(self, pos):
        """rbg_isa_dev: uint64[M], the row of the suffix at each text position.  Through torch"""
        import torch
        pos = _u64(pos)
        M = len(pos)
        with torch.cuda.device(self.info().device):
            d_pos = torch.from_numpy(pos.view(np.int64)).cuda()
            d_row = torch.full((max(M, 1),), -6, dtype=torch.int64, device="cuda")
            rc = self.L.rbg_isa_dev(self.h, d_pos.data_ptr() if M else None, M, d_row.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            row = d_row.cpu().numpy()[:M].view(np.uint64).copy()
        _check(rc, "rbg_isa_dev")
        return row

    def extract_dev(self, d_pos, d_len, d_out_off, d_out, d_got):
        """rbg_extract_dev over torch tensors on this handle's device: d_pos int64[M], d_len int32[M], d_out_off int64[M], d_out uint8[...], d_got int32[M];
        item j writes exactly d_len[j] bytes at d_out[d_out_off[j]:] (the bases, then zeros) and d_got[j].  Waits for the current stream"""
        import torch
        M = int(d_pos.numel())
        assert int(d_len.numel()) == M and int(d_out_off.numel()) == M and int(d_got.numel()) >= M
        assert d_pos.element_size() == 8 and d_out_off.element_size() == 8 and d_len.element_size() == 4 and d_got.element_size() == 4 and d_out.element_size() == 1
        with torch.cuda.device(self.info().device):
            ptr = lambda t: t.data_ptr() if M else None
            rc = self.L.rbg_extract_dev(self.h, ptr(d_pos), ptr(d_len), ptr(d_out_off), M, ptr(d_out), ptr(d_got), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
        _check(rc, "rbg_extract_dev")

    def extract(self, pos, length):
        """rbg_extract from host memory: (bytes, got) -- the concatenation of the intervals in item order, interval j at the exclusive sum of the lengths: got[j]
        bases from pos[j] on (up to the first byte that is no base), then zeros.  A single position and length give (bytes, int)"""
        one = np.isscalar(pos)
        pos, length = _u64(np.atleast_1d(pos)), _u64(np.atleast_1d(length))
        if len(pos) != len(length):
            raise ValueError("extract: a length per position")
        out = np.full(max(int(length.sum()), 1), 0xA5, np.uint8)
        got = np.zeros(max(len(pos), 1), np.uint64)
        _check(self.L.rbg_extract(self.h, _p(pos), _p(length), len(pos), _p(out), _p(got)), "rbg_extract")
        text = out[:int(length.sum())].tobytes()
        return (text, int(got[0])) if one else (text, got[:len(pos)].copy())

    def extend_right(self, seqs, off, item_seq, item_b, item_row, item_skip, item_limit, max_mismatch=4):
        """rbg_extend_right_dev: the FL walk alone -- item j takes item_skip[j] FL steps from row item_row[j], then goes right from position item_b[j] of
        sequence item_seq[j] of the packed batch (seqs, off), at most item_limit[j] bases -> a numpy array of EXTEND records.  Through torch"""
        import torch
        seqs, off = np.ascontiguousarray(seqs, dtype=np.uint8), _u64(off)
        N, M = len(off) - 1, len(item_seq)
        pad = (-len(seqs)) % 16 + 16
        with torch.cuda.device(self.info().device):
            dev = lambda a, t: torch.from_numpy(np.ascontiguousarray(a).view(t)).cuda()
            d_seqs = dev(np.concatenate([seqs, np.zeros(pad, np.uint8)]), np.uint8)
            d_off = dev(off, np.int64)
            d_seq, d_b, d_skip = (dev(np.asarray(a, np.uint32), np.int32) for a in (item_seq, item_b, item_skip))
            d_row, d_lim = dev(_u64(item_row), np.int64), dev(_u64(item_limit), np.int64)
            d_out = torch.full((max(M, 1) * EXTEND.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
            ptr = lambda t: t.data_ptr() if M else None
            rc = self.L.rbg_extend_right_dev(self.h, d_seqs.data_ptr(), d_off.data_ptr(), N, ptr(d_seq), ptr(d_b), ptr(d_row), ptr(d_skip), ptr(d_lim), M,
                                             max_mismatch, d_out.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            out = d_out.cpu().numpy()[:M * EXTEND.itemsize].view(EXTEND).copy()
        _check(rc, "rbg_extend_right_dev")
        return out

    def extend_left(self, seqs, off, item_seq, item_a, item_row, item_limit, max_mismatch=4):
        """rbg_extend_left_dev: the LF walk alone -- item j goes left from position item_a[j] of sequence item_seq[j] of the packed batch (seqs, off), whose
        occurrence lies at row item_row[j], at most item_limit[j] bases -> a numpy array of EXTEND records.  The arrays cross to the device and back through
        torch"""
        import torch
        seqs, off = np.ascontiguousarray(seqs, dtype=np.uint8), _u64(off)
        N, M = len(off) - 1, len(item_seq)
        pad = (-len(seqs)) % 16 + 16
        info = self.info()
        with torch.cuda.device(info.device):
            dev = lambda a, t: torch.from_numpy(np.ascontiguousarray(a).view(t)).cuda()
            d_seqs = dev(np.concatenate([seqs, np.zeros(pad, np.uint8)]), np.uint8)
            d_off = dev(off, np.int64)
            d_seq, d_a = dev(np.asarray(item_seq, np.uint32), np.int32), dev(np.asarray(item_a, np.uint32), np.int32)
            d_row, d_lim = dev(_u64(item_row), np.int64), dev(_u64(item_limit), np.int64)
            d_out = torch.full((max(M, 1) * EXTEND.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
            st = torch.cuda.current_stream().cuda_stream
            rc = self.L.rbg_extend_left_dev(self.h, d_seqs.data_ptr(), d_off.data_ptr(), N, d_seq.data_ptr() if M else None, d_a.data_ptr() if M else None,
                                            d_row.data_ptr() if M else None, d_lim.data_ptr() if M else None, M, max_mismatch, d_out.data_ptr(), st)
            torch.cuda.synchronize()
            out = d_out.cpu().numpy()[:M * EXTEND.itemsize].view(EXTEND).copy()
        _check(rc, "rbg_extend_left_dev")
        return out

    def align_sam(self, seqs, quals, names, min_length=20, max_hits=16, secondary=False):
        """rbg_align_sam: the SAM lines of a batch of raw reads (bytes), both strands searched, written on the device.  seqs / names: lists of bytes;
        quals: a list of bytes of the reads' lengths, or None (every QUAL is "*")"""
        return self._sam_lines(seqs, quals, names, min_length, max_hits, secondary, None)

    def _sam_lines(self, seqs, quals, names, min_length, max_hits, secondary, _max_mismatch, _right=False):
        """the spans of a batch, then rbg_align_sam (_max_mismatch None), rbg_align_sam_extend or rbg_align_sam_extend_both (_right), then the text"""
        def spans(items):
            ln = np.array([len(x) for x in items], dtype=np.uint32)
            beg = np.zeros(len(items), dtype=np.uint64)
            if len(items) > 1:
                beg[1:] = np.cumsum(ln[:-1], dtype=np.uint64)
            blob = b"".join(items)
            return C.create_string_buffer(blob, len(blob) + 1), beg, ln
        if quals is not None and [len(q) for q in quals] != [len(s) for s in seqs]:
            raise ValueError("align_sam: a quality string per read, of the read's length")
        if len(names) != len(seqs):
            raise ValueError("align_sam: a name per read")
        sbuf, sbeg, slen = spans(seqs)
        qbuf, qbeg, _ = spans(quals) if quals is not None else (None, None, None)
        nbuf, nbeg, nlen = spans(names)
        text, n = VP(), U64()
        flags = SAM_SECONDARY if secondary else 0
        if _max_mismatch is None:
            _check(self.L.rbg_align_sam(self.h, sbuf, _p(sbeg), _p(slen), qbuf, _p(qbeg), nbuf, _p(nbeg), _p(nlen), len(seqs), min_length, max_hits,
                                        flags, C.byref(text), C.byref(n)), "rbg_align_sam")
        elif _right:
            _check(self.L.rbg_align_sam_extend_both(self.h, sbuf, _p(sbeg), _p(slen), qbuf, _p(qbeg), nbuf, _p(nbeg), _p(nlen), len(seqs), min_length, max_hits,
                                                    flags, _max_mismatch, C.byref(text), C.byref(n)), "rbg_align_sam_extend_both")
        else:
            _check(self.L.rbg_align_sam_extend(self.h, sbuf, _p(sbeg), _p(slen), qbuf, _p(qbeg), nbuf, _p(nbeg), _p(nlen), len(seqs), min_length, max_hits,
                                               flags, _max_mismatch, C.byref(text), C.byref(n)), "rbg_align_sam_extend")
        try:
            _check(self.L.rbg_wait_text(self.h, text), "rbg_wait_text")
            return C.string_at(text, n.value) if n.value else b""
        finally:
            self.L.rbg_release_text(self.h, text)

    def sam_header(self, pg=None):
        """rbg_sam_header: @HD, one @SQ per document in sorted-start order, then `pg` (bytes, appended as given)"""
        text, n = VP(), U64()
        _check(self.L.rbg_sam_header(self.h, pg, C.byref(text), C.byref(n)), "rbg_sam_header")
        try:
            return C.string_at(text, n.value)
        finally:
            self.L.rbg_free_buffer(text)

    def markers_report(self, seqs, off, params, first_fwd=None):
        """rbg_markers_report: what rb_markers prints for a batch of RAW reads, as records -> (seed_off[N+1], records (REPORT_SEED), mk);
        read i prints records[seed_off[i]:seed_off[i+1]], a record's markers are mk[mk_begin:mk_end] (sorted, unique).  params: report_params(...);
        first_fwd: the heuristic worker's coin per read (None: forward first)"""
        N = len(off) - 1
        seed_off = np.zeros(N + 1, np.uint64)
        coin = None if first_fwd is None else np.ascontiguousarray(first_fwd, dtype=np.uint8)
        ps, pm = VP(), VP()
        _check(self.L.rbg_markers_report(self.h, _p(seqs), _p(off), N, _p(coin), C.byref(params), _p(seed_off), C.byref(ps), C.byref(pm)), "rbg_markers_report")
        S = int(seed_off[N])
        recs = _take(ps, 6 * S).view(REPORT_SEED)
        nmk = int(recs["mk_end"][-1]) if S else 0
        return seed_off, recs, _take(pm, nmk)

    def markers_report_text(self, seqs, off, names, params, first_fwd=None):
        """rbg_markers_report_text: rb_markers' stdout for a batch of RAW reads (bytes), written on the device; names = list of bytes"""
        N = len(off) - 1
        coin = None if first_fwd is None else np.ascontiguousarray(first_fwd, dtype=np.uint8)
        blob = b"".join(names)
        nlen = np.array([len(x) for x in names], dtype=np.uint32)
        nbeg = np.zeros(len(names), dtype=np.uint64)
        if len(names) > 1:
            nbeg[1:] = np.cumsum(nlen[:-1], dtype=np.uint64)
        buf = C.create_string_buffer(blob, len(blob) + 1)
        text, n = VP(), U64()
        _check(self.L.rbg_markers_report_text(self.h, _p(seqs), _p(off), N, _p(coin), C.byref(params), buf, _p(nbeg), _p(nlen), C.byref(text), C.byref(n)),
               "rbg_markers_report_text")
        try:
            _check(self.L.rbg_wait_text(self.h, text), "rbg_wait_text")
            return C.string_at(text, n.value) if n.value else b""
        finally:
            self.L.rbg_release_text(self.h, text)

    def markers_tally(self, seqs, off, params, first_fwd, tally, flags=0):
        """rbg_markers_tally: markers_report's inputs; the markers of the lines rb_markers would print are added to `tally` (a Tally of this
        index) on the device, nothing is returned.  flags: TALLY_PER_READ counts a marker once per read (its longest line),
        | TALLY_DROP_SITE_CONFLICTS leaves out the sites of which a read carries two alleles (rbg_markers_tally_reads)"""
        N = len(off) - 1
        coin = None if first_fwd is None else np.ascontiguousarray(first_fwd, dtype=np.uint8)
        if flags:
            _check(self.L.rbg_markers_tally_reads(self.h, _p(seqs), _p(off), N, _p(coin), C.byref(params), flags, tally.h), "rbg_markers_tally_reads")
            return
        _check(self.L.rbg_markers_tally(self.h, _p(seqs), _p(off), N, _p(coin), C.byref(params), tally.h), "rbg_markers_tally")

    def counters(self):
        out = np.zeros(4, np.uint64)
        _check(self.L.rbg_counters(self.h, _p(out)), "rbg_counters")
        return out

    # ---- several GPUs in one process
    def replicate(self, device):
        """a further replica of the device index on `device` (peer copy); free it before this one"""
        h = VP()
        _check(self.L.rbg_replicate(self.h, device, C.byref(h)), "rbg_replicate")
        r = RowBowt(h)
        r._primary = self   # keeps the primary alive
        return r

    def replicate_many(self, devices):
        """replicas on every device of `devices` at once (the peer copies overlap); free them before this one"""
        G = len(devices)
        devs = (C.c_int * G)(*devices)
        hs = (VP * G)()
        _check(self.L.rbg_replicate_many(self.h, devs, G, hs), "rbg_replicate_many")
        out = []
        for g in range(G):
            r = RowBowt(VP(hs[g]))
            r._primary = self
            out.append(r)
        return out

    def replicate_stats(self):
        """a replica's share of the fan-out: {ms of its peer copies, bytes, GB/s, peer access}"""
        out = (C.c_double * 3)()
        _check(self.L.rbg_replicate_stats(self.h, out), "rbg_replicate_stats")
        ms, nbytes, peer = float(out[0]), int(out[1]), int(out[2])
        return {"copy_ms": ms, "bytes": nbytes, "GBps": (nbytes / (ms * 1e-3) / 1e9) if ms > 0 else None,
                "peer_access": {1: "direct", 0: "staged through the host", -1: "same device"}[peer]}

    def replica_pointer_check(self):
        """what the check of the re-pointed copy found when this replica was made (rbg_replica_pointer_check): pointer words recognised and words that
        break the invariant, in DevIndex and in the records of the pointer tables"""
        out = np.zeros(4, np.uint64)
        _check(self.L.rbg_replica_pointer_check(self.h, _p(out)), "rbg_replica_pointer_check")
        return dict(zip(("dev_pointers", "dev_violations", "table_pointers", "table_violations"), (int(v) for v in out)))

    def counters_reset(self):
        _check(self.L.rbg_counters_reset(self.h), "rbg_counters_reset")

    def combine_stats(self):
        """(launches, requests) of the one-read calls that went through the micro-batching queue"""
        out = np.zeros(2, np.uint64)
        _check(self.L.rbg_combine_stats(self.h, _p(out)), "rbg_combine_stats")
        return int(out[0]), int(out[1])


def load_rowbowt(prefix, flag=LoadRbwtFlag.NONE, device=0):
    """rbwt::load_rowbowt(prefix, flag), rowbowt_io.hpp:176-189"""
    h = VP()
    _check(lib().rbg_load(os.fsencode(prefix), int(flag), device, C.byref(h)), f"rbg_load({prefix})")
    return RowBowt(h)


def shard_bounds(n_items, rank, world):
    b, e = U64(), U64()
    _check(lib().rbg_shard_bounds(n_items, rank, world, C.byref(b), C.byref(e)), "rbg_shard_bounds")
    return b.value, e.value


def find_range_sharded(replicas, seqs, off, toehold=False):
    """find_range / find_range_w_toehold with the batch sharded over the replicas (contiguous blocks, concurrently)"""
    N = len(off) - 1
    hs = (VP * len(replicas))(*[r.h for r in replicas])
    lo, hi = np.zeros(N, np.uint64), np.zeros(N, np.uint64)
    k = np.zeros(N, np.uint64) if toehold else None
    _check(lib().rbg_find_range_sharded(hs, len(replicas), _p(seqs), _p(off), N, _p(lo), _p(hi), _p(k)), "rbg_find_range_sharded")
    return (lo, hi, k) if toehold else (lo, hi)


def counters_allreduce_local(replicas):
    """one RCCL all-reduce of the four counters over replicas on distinct devices of this process"""
    hs = (VP * len(replicas))(*[r.h for r in replicas])
    out = np.zeros(4, np.uint64)
    _check(lib().rbg_counters_allreduce_local(hs, len(replicas), _p(out)), "rbg_counters_allreduce_local")
    return out
