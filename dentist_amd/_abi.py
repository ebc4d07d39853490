"""include/dentist_hip.h as ctypes sees it: loading libdentist_hip.so, the error type, struct layouts, record dtypes and the
one table of prototypes.  No compute, no fallback."""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))


def lib_path():
    # DH_DEV_LIB: development builds of the same library (profiling counters compiled in), never a fallback
    return os.environ.get("DH_DEV_LIB") or os.path.join(_HERE, "libdentist_hip.so")


class DhError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libdentist_hip error {code}: {msg}")
        self.code = code


class _Fields(ctypes.Structure):
    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class AlignOpts(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in (
        "k", "hmin", "band_shift", "tspace", "min_len", "pen", "xdrop", "max_err_ppm", "max_cand",
        "max_la", "tcap", "strands", "skip_self", "dmax", "width", "kmer_mod", "algo")]


class AlignStats(_Fields):
    _fields_ = [("hits", ctypes.c_int64), ("cands", ctypes.c_int64), ("alignments", ctypes.c_int64),
                ("wave_cells", ctypes.c_int64), ("las", ctypes.c_int64), ("b_bases", ctypes.c_int64),
                ("ms_index", ctypes.c_float), ("ms_seed", ctypes.c_float), ("ms_wave", ctypes.c_float),
                ("ms_gather", ctypes.c_float), ("ms_total", ctypes.c_float),
                ("wave_launches", ctypes.c_int32), ("overflow_items", ctypes.c_int32), ("big_items", ctypes.c_int64)]


class CumStats(_Fields):
    _fields_ = [("ms_index", ctypes.c_double), ("ms_seed", ctypes.c_double), ("ms_wave", ctypes.c_double),
                ("ms_gather", ctypes.c_double)] + [(n, ctypes.c_int64) for n in (
                    "wave_launches", "wave_cells", "alignments", "las", "aligned_bp", "trace_values", "hits",
                    "b_bases")]


class ProcessOpts(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in (
        "tspace_map", "allowance", "min_anchor", "min_reads", "max_reads", "tspace_pile", "rounds",
        "flank_window", "max_align_err_ppm", "max_ins_err_ppm", "bad_fraction_ppm", "width", "dust", "algo",
        "max_partners", "min_relative_score_ppm")]


class ChainOpts(ctypes.Structure):
    """dh_chain_opts (ChainingOptions of the reference): 32 bytes"""
    _fields_ = [("max_indel", ctypes.c_int32), ("max_chain_gap", ctypes.c_int32), ("min_score", ctypes.c_int32),
                ("pad_", ctypes.c_int32), ("max_relative_overlap", ctypes.c_double), ("min_relative_score", ctypes.c_double)]


class RepeatOpts(ctypes.Structure):
    """dh_repeat_opts"""
    _fields_ = [(n, ctypes.c_int32) for n in ("lower", "upper", "improper_lower", "improper_upper", "allowance", "with_improper")]


class MaskOpts(ctypes.Structure):
    """dh_mask_opts"""
    _fields_ = [(n, ctypes.c_int32) for n in ("min_count", "min_gap", "min_interval", "pad_")]


class ScaffoldOpts(ctypes.Structure):
    _fields_ = [("min_spanning_reads", ctypes.c_int32), ("merge_extensions", ctypes.c_int32),
                ("best_pile_up_margin", ctypes.c_double), ("existing_gap_bonus", ctypes.c_double),
                ("only_joins", ctypes.c_int32), ("pad_", ctypes.c_int32)]


class OutputOpts(ctypes.Structure):
    _fields_ = [("line_width", ctypes.c_int32), ("highlight", ctypes.c_int32), ("join_policy", ctypes.c_int32),
                ("agp_dazzler", ctypes.c_int32), ("agp_skip_read_ids", ctypes.c_int32), ("only", ctypes.c_int32),
                ("agp_version", ctypes.c_char_p), ("tool", ctypes.c_char_p), ("input_assembly", ctypes.c_char_p),
                ("min_extension_length", ctypes.c_int32), ("pad", ctypes.c_int32)]


class OutputFilter(ctypes.Structure):
    _fields_ = [("max_insertion_error_ppm", ctypes.c_int32), ("nskip", ctypes.c_int32), ("skip_gaps2", ctypes.c_void_p)]


# dh_remap_fn
REMAP_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32), ctypes.c_int32,
                            ctypes.POINTER(ctypes.c_int32), ctypes.c_int32, ctypes.POINTER(ctypes.c_void_p),
                            ctypes.POINTER(ctypes.c_int64))

LA_DTYPE = np.dtype([("tlen", "<i4"), ("diffs", "<i4"), ("abpos", "<i4"), ("bbpos", "<i4"),
                     ("aepos", "<i4"), ("bepos", "<i4"), ("flags", "<u4"), ("aread", "<i4"),
                     ("bread", "<i4"), ("pad", "<i4"), ("toff", "<i8")])

# dh_seed_cand (16 bytes): one candidate of the seed stage
SEED_CAND_DTYPE = np.dtype([("score", "<i4"), ("aseq", "<i4"), ("apos", "<i4"), ("bpos", "<i4")])

INSERTION_DTYPE = np.dtype([(n, "<i4") for n in (
    "contig_left", "status", "nreads", "ref_read", "ref_read_id", "crop_left", "crop_right", "left_aepos",
    "right_abpos", "ins_begin", "ins_end", "comp", "cons_len", "left_diffs", "right_diffs", "join")]
    + [("cons_off", "<i8"), ("contig_right", "<i4"), ("pad", "<i4")])

# dh_contig_mapping / dh_gap_summary (dh_check_gaps)
CONTIG_MAPPING_DTYPE = np.dtype([("ref_contig", "<i4"), ("ref_begin", "<i4"), ("ref_end", "<i4"), ("ref_contig_length", "<i4"),
                                 ("query_contig", "<i4"), ("duplicate", "<i4"), ("complement", "<i4"), ("alignment_error", "<f4")])
GAP_SUMMARY_DTYPE = np.dtype([(f, "<i4") for f in (
    "state", "gap_length", "lhs_map", "rhs_map", "align_status", "complement", "true_contig", "true_begin", "true_end",
    "result_begin_contig", "result_begin", "result_end_contig", "result_end", "col_begin", "col_end", "reference_length",
    "query_length", "matches", "dust_ops", "dust_matches", "none_dust_ops", "none_dust_matches")])
GAP_STATES = ("unkown", "broken", "unclosed", "partiallyClosed", "closed", "ignored")
# dh_exact_hit (32 bytes): one exact occurrence of a query (complement 1: of its reverse complement) in a reference record
EXACT_HIT_DTYPE = np.dtype([("query", "<i4"), ("ref", "<i4"), ("begin", "<i8"), ("end", "<i8"), ("complement", "<i4"),
                            ("pad", "<i4")])

REGION_DTYPE = np.dtype([("contig", "<i4"), ("begin", "<i4"), ("end", "<i4")])
REGION_REPORT_DTYPE = np.dtype([("num_spanning_reads", "<i4"), ("weak_bp", "<i4"), ("is_valid", "<i4"),
                                ("ctx_begin", "<i4"), ("ctx_end", "<i4")])

JOIN_DTYPE = np.dtype([("contig0", "<i4"), ("part0", "<i4"), ("contig1", "<i4"), ("part1", "<i4"), ("type", "<i4"),
                       ("count", "<i4"), ("first", "<i8")])
READ_ALIGNMENT_DTYPE = np.dtype([("read", "<i4"), ("la0", "<i4"), ("la1", "<i4"), ("seed0", "u1"), ("seed1", "u1"),
                                 ("n", "u1"), ("pad", "u1")])

# pile-ups.db / insertions.db
SEEDED_DTYPE = np.dtype([("id", "<i8"), ("contig_a_id", "<u4"), ("contig_a_len", "<u4"), ("contig_b_id", "<u4"),
                         ("contig_b_len", "<u4"), ("flags", "u1"), ("seed", "u1"), ("tspace", "<u2"), ("nla", "<i4")])
CHAIN_LA_DTYPE = np.dtype([("a_begin", "<u4"), ("a_end", "<u4"), ("b_begin", "<u4"), ("b_end", "<u4"), ("diffs", "<u4"),
                           ("ntp", "<i4")])
INSERTION_REC_DTYPE = np.dtype([("start_contig", "<i8"), ("end_contig", "<i8"), ("start_part", "u1"), ("end_part", "u1"),
                                ("pad", "u1", (6,)), ("seq_len", "<i8"), ("contig_len", "<i8"), ("noverlaps", "<i4"),
                                ("nread_ids", "<i4")])
assert SEEDED_DTYPE.itemsize == 32 and CHAIN_LA_DTYPE.itemsize == 24 and INSERTION_REC_DTYPE.itemsize == 48

# ---------------------------------------------------------------- the prototypes
# One row per function include/dentist_hip.h declares, grouped and ordered as there: name -> (result, arguments).
# int is cint, int32_t i32, int64_t i64, double f64, void None; a `const char *` that takes bytes or None is cstr; a pointer
# that callers fill through byref() of one ctypes type is P(that type); every other pointer is vp (an address, byref(...) or
# None).  lib() applies the table once; nothing else sets a prototype.
cint, i32, i64, f64 = ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
vp, cstr, P = ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER

_PROTOTYPES = {
    "dh_last_error": (cstr, []),
    "dh_abi_version": (i32, []),
    # ---- context
    "dh_ctx_create": (cint, [i32, vp, P(vp)]),
    "dh_ctx_destroy": (None, [vp]),
    "dh_ctx_sync": (cint, [vp]),
    # ---- alignment options
    "dh_default_align_opts": (None, [P(AlignOpts)]),
    # ---- device-resident sequence DB
    "dh_db_create": (cint, [vp, vp, vp, i32, vp, P(vp)]),
    "dh_db_destroy": (None, [vp]),
    "dh_db_set_mask": (cint, [vp, vp, vp]),
    "dh_db_dust": (cint, [vp]),
    "dh_db_get_mask": (i64, [vp, vp, vp, i64]),
    "dh_db_drop_cache": (cint, [vp]),
    "dh_db_nreads": (i32, [vp]),
    "dh_db_total_bases": (i64, [vp]),
    # ---- local alignments, statistics and counters, dh_align_db
    "dh_la_set_destroy": (None, [vp]),
    "dh_la_set_count": (i64, [vp]),
    "dh_la_set_trace_len": (i64, [vp]),
    "dh_la_set_records": (vp, [vp]),
    "dh_la_set_trace": (vp, [vp]),
    "dh_la_set_tspace": (i32, [vp]),
    "dh_get_align_stats": (cint, [vp, P(AlignStats)]),
    "dh_get_cum_stats": (cint, [vp, P(CumStats), i32]),
    "dh_ctx_release_scratch": (cint, [vp]),
    "dh_get_mjoin_counts": (cint, [vp, vp, i32]),
    "dh_get_join_counts": (cint, [vp, vp, i32]),
    "dh_get_tjoin_counts": (cint, [vp, vp, i32]),
    "dh_get_seed_tier_counts": (cint, [vp, vp, i32]),
    "dh_get_seed_band_counts": (cint, [vp, vp, i32]),
    "dh_join_hit_capacity": (i64, [vp, vp, i32, i32, f64, i64]),
    "dh_align_db": (cint, [vp, vp, vp, P(AlignOpts), i32, P(vp)]),
    "dh_seed_candidates": (cint, [vp, vp, vp, P(AlignOpts), vp, vp, vp]),
    "dh_extend_candidates": (cint, [vp, vp, vp, P(AlignOpts), vp, vp, i32, P(vp), P(vp)]),
    "dh_set_near_best": (None, [i32]),
    "dh_ctx_set_near_best": (cint, [vp, i32]),
    "dh_align_db_block": (cint, [vp, vp, vp, i32, i32, P(AlignOpts), i32, P(vp)]),
    "dh_align_db_transposed": (cint, [vp, vp, vp, vp, i32, vp, vp]),
    "dh_la_set_merge": (cint, [P(vp), i32, P(vp)]),
    # ---- .las files
    "dh_las_write": (cint, [cstr, vp, i64, vp, i32]),
    "dh_las_read": (cint, [cstr, P(vp)]),
    "dh_las_merge": (cint, [P(cstr), i32, cstr]),
    # ---- trace-point arithmetic of the alignment model
    "dh_translate_trace_point": (cint, [vp, vp, i32, i32, i32, P(i32), P(i32)]),
    "dh_common_trace_point": (cint, [vp, i64, vp, i32, i32, i32, i32, vp, i64, P(i32)]),
    # ---- pile-ups, the host commands on the mapping, dh_map_reads
    "dh_default_process_opts": (None, [P(ProcessOpts)]),
    "dh_collect_spanning": (cint, [vp, i64, vp, i32, P(ProcessOpts), P(vp)]),
    "dh_collect_candidates": (cint, [vp, i64, vp, i32, P(ProcessOpts), P(vp)]),
    "dh_pileups_create": (cint, [vp, vp, i32, vp, P(vp)]),
    "dh_pileups_select": (cint, [vp, vp, i64, P(ProcessOpts), P(vp)]),
    "dh_pileups_destroy": (None, [vp]),
    "dh_pileups_count": (i32, [vp]),
    "dh_pileups_get": (i32, [vp, i32, P(i32), P(vp)]),
    "dh_pileups_create_joins": (cint, [vp, vp, i32, vp, P(vp)]),
    "dh_pileups_get_join": (cint, [vp, i32, vp]),
    "dh_db_mask_coverage": (cint, [vp, vp, i64, vp, i32, i32, i32, i32, i32]),
    "dh_max_coverage_reads": (i32, [f64]),
    "dh_max_improper_coverage_reads": (i32, [f64]),
    "dh_propagate_mask": (i64, [vp, i64, vp, i32, vp, vp, i32, vp, i32, vp, vp, i64]),
    "dh_validate_regions": (i64, [vp, i64, vp, i32, vp, i32, i32, i32, i32, i32, vp, vp, i64]),
    "dh_map_reads": (cint, [vp, vp, vp, i32, i32, P(AlignOpts), P(ProcessOpts), vp, vp, i32, vp, P(vp), P(vp)]),
    # ---- the scaffold-graph pile-up builder of `dentist collect`
    "dh_default_scaffold_opts": (None, [vp]),
    "dh_scaffold_pileups": (cint, [vp, i64, vp, i32, vp, i32, vp, i32, P(ScaffoldOpts), P(vp)]),
    "dh_scaffold_pileups_cb": (cint, [vp, i64, vp, i32, vp, i32, vp, i32, P(ScaffoldOpts), i32, i32, REMAP_FN, vp, P(vp), P(vp), P(i32)]),
    "dh_scaffold_pileups_resolved": (cint, [vp, vp, vp, vp, i64, vp, i32, P(ScaffoldOpts), P(AlignOpts), i32, i32, i32, P(vp), P(vp), P(i32)]),
    "dh_scaffold_npiles": (i32, [vp]),
    "dh_scaffold_nentries": (i64, [vp]),
    "dh_scaffold_joins": (vp, [vp]),
    "dh_scaffold_entries": (vp, [vp]),
    "dh_scaffold_destroy": (None, [vp]),
    "dh_remap_skipping_reads": (cint, [vp, vp, vp, vp, i32, vp, i32, vp, i32, P(vp)]),
    "dh_scaffold_spanning": (cint, [vp, vp, i64, P(vp), P(i32)]),
    "dh_scaffold_gap_pileups": (cint, [vp, vp, i64, P(vp), P(i32)]),
    "dh_scaffold_all_pileups": (cint, [vp, vp, i64, i32, P(vp), P(i32)]),
    "dh_collect_filter": (cint, [vp, i64, vp, i32, vp, i32, vp, vp, P(ProcessOpts), vp, vp]),
    "dh_pileups_flat": (i64, [vp, vp, vp, vp]),
    # ---- `dentist process` for a batch of pile-ups
    "dh_process_pileups": (cint, [vp, vp, vp, vp, i64, vp, vp, P(ProcessOpts), P(vp)]),
    "dh_insertions_destroy": (None, [vp]),
    "dh_insertions_count": (i32, [vp]),
    "dh_insertions_records": (vp, [vp]),
    "dh_insertions_bases": (vp, [vp]),
    "dh_insertions_bases_len": (i64, [vp]),
    "dh_insertions_read_ids": (vp, [vp]),
    "dh_insertions_read_ids_off": (vp, [vp]),
    "dh_crop_pileups": (cint, [vp, vp, vp, i32, vp, i64, vp, vp, P(ProcessOpts), P(vp)]),
    "dh_crop_pileups_masked": (cint, [vp, vp, vp, i32, vp, i64, vp, vp, vp, vp, vp, vp]),
    "dh_process_pileups_masked": (cint, [vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp]),
    "dh_process_pileups_set": (cint, [vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "dh_la_set_trace_on_device": (i32, [vp]),
    "dh_cropped_create": (cint, [vp, i32, i32, vp, vp, vp, vp, vp, P(vp)]),
    "dh_cropped_create2": (cint, [vp, i32, i32, vp, vp, vp, vp, vp, vp, P(vp)]),
    "dh_cropped_destroy": (None, [vp]),
    "dh_cropped_npiles": (i32, [vp]),
    "dh_cropped_kind": (vp, [vp]),
    # ---- the host work of one rank between the collectives of the sharded path
    "dh_shard_free": (None, [vp]),
    "dh_shard_pack_candidates": (cint, [vp, vp, i64, i32, P(vp), P(i64)]),
    "dh_shard_plan_create": (cint, [vp, vp, i32, P(ProcessOpts), P(vp)]),
    "dh_shard_read_joins": (cint, [vp, i64, vp, i32, vp, i32, i32, P(vp), P(i64)]),
    "dh_shard_graph_plan_create": (cint, [vp, vp, i32, i32, vp, i32, P(ScaffoldOpts), P(ProcessOpts), P(vp)]),
    "dh_shard_plan_destroy": (None, [vp]),
    "dh_shard_plan_las": (vp, [vp]),
    "dh_shard_plan_nlas": (i64, [vp]),
    "dh_shard_plan_pileups": (vp, [vp]),
    "dh_shard_plan_owner": (vp, [vp]),
    "dh_shard_pack_cropped": (cint, [vp, vp, i32, vp, vp]),
    "dh_shard_unpack_cropped": (cint, [vp, vp, i32, vp, i32, vp, i32, P(vp)]),
    "dh_cropped_records": (vp, [vp]),
    # ---- the multi-GPU entry, the rest of dh_cropped, the process statistics
    "dh_comm_unique_id": (cint, [vp]),
    "dh_comm_create": (cint, [cstr, i32, i32, vp, P(vp)]),
    "dh_comm_create_local": (cint, [i32, vp, vp]),
    "dh_comm_destroy": (None, [vp]),
    "dh_comm_rank": (i32, [vp]),
    "dh_comm_world": (i32, [vp]),
    "dh_comm_all_gather": (cint, [vp, vp, i64, P(vp), vp]),
    "dh_comm_all_to_all": (cint, [vp, vp, vp, P(vp), vp]),
    "dh_shard_run": (cint, [vp, vp, vp, i32, vp, i32, vp, i64, vp, P(ProcessOpts), vp, vp, vp, i32, vp, P(vp), vp]),
    "dh_cropped_nreads": (i32, [vp]),
    "dh_cropped_pile": (vp, [vp]),
    "dh_cropped_entry": (vp, [vp]),
    "dh_cropped_read_id": (vp, [vp]),
    "dh_cropped_offsets": (vp, [vp]),
    "dh_cropped_bases": (vp, [vp]),
    "dh_process_cropped": (cint, [vp, vp, vp, P(ProcessOpts), P(vp)]),
    "dh_get_process_stats": (cint, [vp, vp, vp]),
    "dh_get_process_work": (cint, [vp, vp]),
    # ---- stage-level entry points
    "dh_tile_qv": (cint, [vp, vp, vp, i64, vp, i32, i32, vp, i32]),
    "dh_consensus": (cint, [vp, vp, vp, i64, vp, i32, i32, i32, vp, i64, P(i64)]),
    # ---- base-level alignments from trace points
    "dh_la_edit_paths": (cint, [vp, vp, vp, vp, i64, vp, i32, i64, i64, P(vp)]),
    "dh_la_set_edit_paths": (cint, [vp, vp, vp, vp, i64, i64, P(vp)]),
    "dh_edit_paths_destroy": (None, [vp]),
    "dh_edit_paths_count": (i64, [vp]),
    "dh_edit_paths_op_off": (vp, [vp]),
    "dh_edit_paths_ops": (vp, [vp]),
    "dh_edit_paths_score": (vp, [vp]),
    "dh_edit_paths_tile_off": (vp, [vp]),
    "dh_edit_paths_tile_score": (vp, [vp]),
    "dh_edit_paths_general_tiles": (i64, [vp]),
    "dh_format_cigar": (i64, [vp, i64, i32, vp, i64]),
    "dh_format_alignment": (i64, [vp, vp, vp, i64, i32, vp, i64]),
    # ---- base-level alignment of whole chains
    "dh_la_chain_paths": (cint, [vp, vp, vp, vp, i64, vp, i32, vp, i64, P(vp), vp]),
    "dh_la_set_chain_paths": (cint, [vp, vp, vp, vp, P(vp), vp]),
    "dh_edit_paths_fillers": (i64, [vp]),
    "dh_edit_paths_entry_fillers": (vp, [vp]),
    # ---- exact transposition of local alignments
    "dh_la_transpose": (cint, [vp, vp, vp, vp, i64, vp, i32, i32, P(vp), vp]),
    "dh_la_set_transpose": (cint, [vp, vp, vp, vp, i32, P(vp), vp]),
    # ---- global alignment of arbitrary sequence pairs
    "dh_nw_batch": (cint, [vp, vp, vp, vp, vp, i64, i32, P(vp), vp]),
    # ---- global alignment with affine gap costs
    "dh_nw_affine_batch": (cint, [vp, vp, vp, vp, vp, i64, vp, P(vp), vp]),
    "dh_format_pair": (i64, [cstr, vp, i64, cstr, vp, i64, vp, i64, i32, vp, i64, vp, i64]),
    # ---- exact-match locator
    "dh_exact_locate": (cint, [vp, vp, vp, i64, vp, vp, i64, i32, P(vp)]),
    "dh_exact_hits_destroy": (None, [vp]),
    "dh_exact_hits_count": (i64, [vp]),
    "dh_exact_hits_records": (vp, [vp]),
    # ---- chaining of local alignments
    "dh_default_chain_opts": (None, [P(ChainOpts), i32]),
    "dh_la_chain": (cint, [vp, vp, i64, P(ChainOpts), P(vp)]),
    "dh_la_set_chain": (cint, [vp, vp, P(ChainOpts), P(vp)]),
    "dh_la_chains_destroy": (None, [vp]),
    "dh_la_chains_count": (i64, [vp]),
    "dh_la_chains_records": (i64, [vp]),
    "dh_la_chains_off": (vp, [vp]),
    "dh_la_chains_score": (vp, [vp]),
    "dh_la_chains_src_index": (vp, [vp]),
    "dh_la_chains_flags": (vp, [vp]),
    "dh_la_chains_big_pairs": (i64, [vp]),
    "dh_la_chains_to_set": (cint, [vp, vp, i64, vp, i32, P(vp)]),
    # ---- mask propagation on the device
    "dh_la_propagate_mask": (cint, [vp, vp, i64, vp, i64, i32, vp, vp, i32, vp, i32, P(vp)]),
    "dh_la_set_propagate_mask": (cint, [vp, vp, vp, vp, i32, vp, i32, P(vp)]),
    "dh_mask_result_destroy": (None, [vp]),
    "dh_mask_result_count": (i64, [vp]),
    "dh_mask_result_ptr": (vp, [vp]),
    "dh_mask_result_iv": (vp, [vp]),
    "dh_mask_result_raw": (i64, [vp]),
    "dh_mask_result_hit": (i64, [vp]),
    "dh_mask_result_passes": (i32, [vp]),
    # ---- region validation on the device
    "dh_la_validate_regions": (cint, [vp, vp, i64, vp, i32, vp, i32, i32, i32, i32, i32, P(vp)]),
    "dh_la_set_validate_regions": (cint, [vp, vp, vp, i32, vp, i32, i32, i32, i32, i32, P(vp)]),
    "dh_region_result_destroy": (None, [vp]),
    "dh_region_result_count": (i32, [vp]),
    "dh_region_result_reports": (vp, [vp]),
    "dh_region_result_weak_count": (i64, [vp]),
    "dh_region_result_weak": (vp, [vp]),
    "dh_region_result_span_off": (vp, [vp]),
    "dh_region_result_span_ids": (vp, [vp]),
    "dh_region_result_mask_ptr": (vp, [vp]),
    "dh_region_result_mask_iv": (vp, [vp]),
    "dh_region_result_mask_count": (i64, [vp]),
    "dh_region_result_pairs": (i64, [vp]),
    "dh_region_result_big_regions": (i64, [vp]),
    "dh_region_result_groups": (i64, [vp]),
    # ---- the alignment filters of `dentist collect` on the device
    "dh_la_collect_filter": (cint, [vp, vp, i64, vp, i32, vp, i32, vp, vp, P(ProcessOpts), vp, vp]),
    "dh_la_set_collect_filter": (cint, [vp, vp, vp, i32, vp, i32, vp, vp, P(ProcessOpts), vp, vp]),
    # ---- `dentist mask-repetitive-regions` on the device
    "dh_la_repeat_mask": (cint, [vp, vp, i64, vp, i32, vp, i32, P(RepeatOpts), P(vp)]),
    "dh_la_set_repeat_mask": (cint, [vp, vp, vp, i32, vp, i32, P(RepeatOpts), P(vp)]),
    "dh_repeat_result_destroy": (None, [vp]),
    "dh_repeat_result_mask_ptr": (vp, [vp]),
    "dh_repeat_result_mask_iv": (vp, [vp]),
    "dh_repeat_result_mask_count": (i64, [vp]),
    "dh_repeat_result_all_ptr": (vp, [vp]),
    "dh_repeat_result_all_iv": (vp, [vp]),
    "dh_repeat_result_all_count": (i64, [vp]),
    "dh_repeat_result_improper_ptr": (vp, [vp]),
    "dh_repeat_result_improper_iv": (vp, [vp]),
    "dh_repeat_result_improper_count": (i64, [vp]),
    "dh_repeat_result_units": (i64, [vp]),
    "dh_repeat_result_improper_units": (i64, [vp]),
    "dh_repeat_result_tier_contigs": (i64, [vp, i32]),
    "dh_repeat_result_groups": (i64, [vp]),
    # ---- mask algebra on the device
    "dh_default_mask_opts": (None, [P(MaskOpts)]),
    "dh_mask_combine": (cint, [vp, vp, vp, i32, vp, vp, vp, i32, P(MaskOpts), P(vp)]),
    "dh_la_tandem_mask": (cint, [vp, vp, i64, vp, i32, i32, i32, P(vp)]),
    "dh_mask_set_destroy": (None, [vp]),
    "dh_mask_set_ptr": (vp, [vp]),
    "dh_mask_set_iv": (vp, [vp]),
    "dh_mask_set_count": (i64, [vp]),
    "dh_mask_set_events": (i64, [vp]),
    "dh_mask_set_sort_passes": (i64, [vp]),
    "dh_mask_set_groups": (i64, [vp]),
    # ---- gap analysis of `dentist check-results` on the device
    "dh_check_gaps": (cint, [vp, vp, vp, vp, i32, vp, i32, vp, vp, vp, i32, vp, i32, i32, P(vp)]),
    "dh_gap_report_destroy": (None, [vp]),
    "dh_gap_report_count": (i64, [vp]),
    "dh_gap_report_summaries": (vp, [vp]),
    "dh_gap_report_paths": (vp, [vp]),
    "dh_gap_report_aligned": (i64, [vp]),
    "dh_gap_report_groups": (i64, [vp]),
    # ---- gap-closed assembly writer
    "dh_output_fasta": (cint, [cstr, cstr, vp, vp, i32, vp, P(cstr), vp, vp, i32, vp, i32, i32]),
    "dh_default_output_opts": (None, [P(OutputOpts)]),
    "dh_scaffold_graph_probe": (cint, [i32, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32]),
    "dh_output_assembly": (cint, [cstr, cstr, cstr, vp, vp, i32, vp, vp, vp, vp, i32, vp, vp, vp, i32, vp, P(OutputOpts), P(i32)]),
    "dh_output_db": (cint, [vp, vp, cstr, cstr, cstr, vp, vp, vp, vp, i32, vp, P(OutputOpts), P(OutputFilter), P(i32)]),
    "dh_output_plan": (cint, [vp, i32, vp, vp, vp, vp, i32, i64, P(OutputOpts), P(vp)]),
    "dh_out_plan_destroy": (None, [vp]),
    "dh_out_plan_array": (vp, [vp, i32, P(i64)]),
    "dh_get_output_stats": (cint, [vp, vp]),
    # ---- DAZZ_DB files on disk
    "dh_dazz_create_dam": (cint, [cstr, cstr, i64]),
    "dh_dazz_create_db": (cint, [cstr, cstr, i64]),
    "dh_dazz_split": (cint, [cstr, i32, i32, i64]),
    "dh_dazz_open": (cint, [cstr, P(vp)]),
    "dh_dazz_close": (None, [vp]),
    # ---- sparse packed read loader, the accessors of an open DAZZ_DB, mask tracks
    "dh_dazz_load_reads": (cint, [vp, cstr, vp, i32, P(vp)]),
    "dh_get_load_stats": (cint, [vp, vp, vp]),
    "dh_db_get_bases": (cint, [vp, i32, i32, vp, i64]),
    "dh_db_get_offsets": (cint, [vp, vp]),
    "dh_dazz_nreads": (i32, [vp]),
    "dh_dazz_first_id": (i32, [vp]),
    "dh_dazz_bases": (vp, [vp]),
    "dh_dazz_offsets": (vp, [vp]),
    "dh_dazz_origin": (vp, [vp]),
    "dh_dazz_fpulse": (vp, [vp]),
    "dh_dazz_flags": (vp, [vp]),
    "dh_dazz_header": (cstr, [vp, i32]),
    "dh_dazz_read_mask": (i64, [vp, cstr, cstr, vp, vp, i64]),
    "dh_dazz_write_mask": (cint, [cstr, cstr, i32, vp, vp]),
    # ---- track extras, BED -> mask
    "dh_dazz_read_extra": (i64, [cstr, cstr, cstr, P(i32), P(i32), vp, i64]),
    "dh_dazz_write_extra": (cint, [cstr, cstr, cstr, i32, i32, vp, i64]),
    "dh_bed_to_mask": (cint, [vp, cstr, i64, cstr, i32, P(vp)]),
    "dh_bed_mask_destroy": (None, [vp]),
    "dh_bed_mask_ncontigs": (i32, [vp]),
    "dh_bed_mask_count": (i64, [vp]),
    "dh_bed_mask_ptr": (vp, [vp]),
    "dh_bed_mask_iv": (vp, [vp]),
    "dh_bed_mask_contig_ids": (vp, [vp]),
    "dh_bed_mask_read_off": (vp, [vp]),
    "dh_bed_mask_read_ids": (vp, [vp]),
    # ---- the binary containers between DENTIST's commands
    "dh_pileupdb_write": (cint, [cstr, i32, vp, vp, vp, vp, vp]),
    "dh_pileupdb_read": (cint, [cstr, P(vp)]),
    "dh_insertiondb_write": (cint, [cstr, i32, vp, vp, vp, vp, vp, vp]),
    "dh_insertiondb_read": (cint, [cstr, P(vp)]),
    "dh_insertiondb_merge": (cint, [P(cstr), i32, cstr, P(i64)]),
    "dh_pileups_write_db": (cint, [vp, vp, i64, vp, vp, i32, vp, i32, i32, cstr]),
    "dh_insertions_write_db": (cint, [vp, vp, i32, i32, cstr]),
    "dh_insertions_from_db": (cint, [cstr, vp, i32, P(vp)]),
    "dh_pileups_from_db": (cint, [cstr, i32, i32, vp, i32, P(vp), P(vp), P(vp)]),
    "dh_process_pileups_db": (cint, [vp, vp, cstr, cstr, i32, i32, vp, vp, vp, P(vp)]),
    "dh_process_pileups_db_batches": (cint, [vp, vp, cstr, cstr, vp, i32, vp, vp, vp, i32, i32, vp, vp, vp, vp]),
    "dh_chaindb_destroy": (None, [vp]),
    "dh_chaindb_npiles": (i32, [vp]),
    "dh_chaindb_pile_counts": (vp, [vp]),
    "dh_chaindb_nread_alignments": (i32, [vp]),
    "dh_chaindb_read_alignment_counts": (vp, [vp]),
    "dh_chaindb_nseeded": (i64, [vp]),
    "dh_chaindb_seeded": (vp, [vp]),
    "dh_chaindb_nlas": (i64, [vp]),
    "dh_chaindb_las": (vp, [vp]),
    "dh_chaindb_ntrace": (i64, [vp]),
    "dh_chaindb_trace": (vp, [vp]),
    "dh_chaindb_ninsertions": (i32, [vp]),
    "dh_chaindb_insertions": (vp, [vp]),
    "dh_chaindb_bases": (vp, [vp]),
    "dh_chaindb_read_ids": (vp, [vp]),
    "dh_dazz_write_track": (cint, [cstr, cstr, i32, vp, vp]),
    "dh_dazz_read_track": (i64, [vp, cstr, cstr, vp, vp, i64]),
    "dh_dazz_remove": (cint, [cstr]),
}

# every symbol include/dentist_hip.h declares (tests check the library exports all of them)
SYMBOLS = list(_PROTOTYPES)

_LIB = None


def lib():
    """Load libdentist_hip.so; raises if it has not been built (no fallback)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: build it with `make` or __graft_entry__.build(); "
                           "dentist_amd has no CPU fallback")
    L = ctypes.CDLL(path)
    for name, (res, args) in _PROTOTYPES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    _LIB = L
    return L


def _check(rc):
    if rc != 0:
        raise DhError(rc, lib().dh_last_error().decode(errors="replace"))
