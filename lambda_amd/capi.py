"""ctypes binding of the C ABI in include/lambda_ext.h (liblambda_ext.so).

This is the only way Python code reaches the HIP path: tests, bench.py and the smoke test call the same exported
symbols a C++ maintainer of the reference would link against.  If the shared library is missing
or no gfx950 device is usable, everything here raises -- there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

LIB_PATH = Path(os.environ.get("LX_LIB_PATH") or Path(__file__).resolve().parent / "csrc" / "liblambda_ext.so")  # (override: kernel variants during development)

LX_ALPH = 32
LX_OK = 0
LX_EINVAL = -1
LX_ESTATE = -6
LX_OPT_MAX_QLEN = 1
LX_OPT_QUERY_RUN = 2
LX_OPT_WORKSPACE_BYTES = 3

# every symbol include/lambda_ext.h declares (tests/test_abi.py checks that the library exports all of them)
EXPORTED_SYMBOLS = [
    "lx_abi_version", "lx_build_id", "lx_device_count", "lx_create", "lx_destroy", "lx_last_error", "lx_set_option", "lx_get_option", "lx_host_threads_info", "lx_plan_free_packing_bound", "lx_plan_free_packing_dev", "lx_set_band_centres", "lx_set_band_centres_dev",
    "lx_set_scoring", "lx_builtin_scoring", "lx_score_batch", "lx_score_batch_dev", "lx_align_batch",
    "lx_align_batch_dev", "lx_extend_batch_dev", "lx_prefilter_batch", "lx_synchronize", "lx_last_kernel_ms", "lx_last_kernel_name", "lx_last_trace_kernel_name", "lx_last_phase_ms",
    "lx_iterate_matches", "lx_set_queries", "lx_set_subject_seqs", "lx_iterate_matches_dev", "lx_widen_and_preprocess_dev", "lx_reserve", "lx_sort_words_dev", "lx_trim_result_cache",
    "lx_iterate_result_count", "lx_iterate_result_matches", "lx_iterate_result_ops", "lx_iterate_result_stats",
    "lx_iterate_result_free", "lx_karlin_params", "lx_length_adjustment", "lx_evalue", "lx_bitscore",
    "lx_widen_and_preprocess", "lx_postprocess_records", "lx_postprocess_records_dev", "lx_iterate_matches_dev_top",
    "lx_cull_options_default", "lx_postprocess_records_ex", "lx_postprocess_records_dev_ex", "lx_iterate_matches_dev_top_ex", "lx_compute_lca", "lx_write_records", "lx_convert_ranks",
    "lx_set_subjects", "lx_extend_batch", "lx_extend_batch_rle", "lx_extend_batch_list", "lx_write_records_ex", "lx_check_output_options", "lx_write_footer", "lx_output_options_default", "lx_last_output_error", "lx_expand_ops", "lx_last_extend_stats", "lx_set_frames", "lx_untrue_qry_id", "lx_untrue_subj_id", "lx_translate_six_frames",
    "lx_plan_step", "lx_render_records", "lx_bytes_data", "lx_bytes_size", "lx_bytes_free", "lx_bgzf_bound", "lx_bgzf_compress",
    "lx_write_records_bgzf", "lx_render_bam_dev", "lx_write_bam_dev", "lx_format_number", "lx_render_text_dev", "lx_write_text_dev", "lx_gunzip", "lx_last_gunzip_stats", "lx_gunzip_decline_text", "lx_find_accessions", "lx_taxmap_create", "lx_taxmap_feed", "lx_taxmap_finish",
    "lx_taxmap_destroy", "lx_taxonomy_build", "lx_taxonomy_get", "lx_taxonomy_free",
    "lx_index_build", "lx_index_plan_slices", "lx_index_load", "lx_index_save", "lx_index_attach", "lx_index_get_info", "lx_index_copy_entries", "lx_index_destroy",
    "lx_seed_queries", "lx_seed_result_stats", "lx_seed_result_matches", "lx_seed_result_matches_dev", "lx_seed_result_free",
    "lx_gunzip_stream_open", "lx_gunzip_stream_next", "lx_gunzip_stream_close", "lx_out_open", "lx_out_append", "lx_out_append_ex", "lx_out_close",
    "lx_lca_options_default", "lx_compute_lca_ex", "lx_check_tax_tree", "lx_tax_dev_create", "lx_tax_dev_destroy", "lx_compute_lca_dev",
    "lx_tax_subject_mask", "lx_subject_mask_create_dev", "lx_subject_mask_create", "lx_subject_mask_info", "lx_subject_mask_copy", "lx_subject_mask_destroy", "lx_seed_result_filter",
    "lx_seg_params_default", "lx_seg_tables", "lx_query_mask_create_seg", "lx_query_mask_create", "lx_query_mask_info", "lx_query_mask_copy", "lx_query_mask_destroy",
    "lx_seed_queries_masked", "lx_dust_params_default", "lx_query_mask_create_dust",
]

LX_OPT_MAX_SLEN = 4
LX_OPT_TRACE_BYTES = 5
LX_OPT_BS_MATCH_RULE = 6
LX_OPT_PACKED_HALF = 7
LX_OPT_PASS2_MODE = 8
LX_OPT_BAND = 9
LX_OPT_EXTEND_CHUNK = 10
LX_OPT_MQ_SWEEP = 11
LX_OPT_ITERATE_RECORDS = 13
LX_OPT_HOST_THREADS = 14
LX_OPT_ADAPT_PERMILLE = 12
LX_OPT_GUNZIP_CHUNK = 15
LX_OPT_GUNZIP_PARALLEL_FROM = 16
LX_OPT_BAM_RANGE_BYTES = 17
LX_OPT_INDEX_SLICE_WORDS = 18  # lx_index_build on a handle: 0 = one sort, N >= 1 = in slices of at most N words
LX_OPT_LCA_RANGE_ROWS = 19  # lx_compute_lca_dev: rows per range of whole queries (0 = default, 2^24)
OPT_GUNZIP_WAVE_TEST = 1017  # not part of the ABI (lx_internal.h): chunks per wave, for the tests of lx_gunzip's waves
LX_GUNZIP_NEVER = (1 << 64) - 1  # LX_OPT_GUNZIP_PARALLEL_FROM: no plain member takes the device path


class Karlin(C.Structure):
    _fields_ = [("lambda_", C.c_double), ("K", C.c_double), ("H", C.c_double), ("alpha", C.c_double),
                ("beta", C.c_double)]


class SearchParams(C.Structure):
    _fields_ = [("max_evalue", C.c_double), ("min_bitscore", C.c_int32), ("id_cutoff", C.c_int32),
                ("db_total_length", C.c_uint64), ("query_translated", C.c_int32), ("qry_num_frames", C.c_int32),
                ("sbj_num_frames", C.c_int32), ("bisulfite", C.c_int32), ("q_frame_mode", C.c_int32),
                ("s_frame_mode", C.c_int32), ("karlin", Karlin), ("band", C.c_int32), ("flags", C.c_int32)]


LX_ITERATE_NO_OPS = 1


class IterateStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("hits_duplicate", "failed_bitscore", "failed_evalue", "failed_identity",
                                          "num_ext_score", "num_ext_ali")]


BLAST_MATCH_DTYPE = np.dtype([
    ("qry_id", "<u8"), ("subj_id", "<u8"), ("n_qid", "<u8"), ("n_sid", "<u8"), ("q_start", "<u8"), ("q_end", "<u8"),
    ("s_start", "<u8"), ("s_end", "<u8"), ("score", "<i4"), ("alignment_length", "<i4"), ("num_matches", "<i4"),
    ("num_mismatches", "<i4"), ("num_positives", "<i4"), ("num_gap_opens", "<i4"), ("num_gap_extensions", "<i4"),
    ("identity", "<f4"), ("bit_score", "<f8"), ("e_value", "<f8"), ("ops_off", "<u8"), ("n_ops", "<u4"),
    ("q_frame", "<i2"), ("s_frame", "<i2")])


class RecordStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("qrys_with_hit", "hits_duplicate2", "hits_abundant", "hits_final", "pairs")]


class CullOptions(C.Structure):
    """lx_cull_options: max_hsps and culling_limit between _writeRecord's unique and its cut (0 = off)."""
    _fields_ = [("max_hsps", C.c_uint64), ("culling_limit", C.c_uint64), ("q_lens", C.c_void_p), ("n_q", C.c_uint64), ("q_translated", C.c_int32)]


class CullStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("hits_max_hsps", "hits_culled")]


class GunzipStats(C.Structure):
    """lx_gunzip_stats: where the members of the last lx_gunzip or lx_gunzip_stream_next call were decoded."""
    _fields_ = [(n, C.c_uint64) for n in ("bgzf_members", "plain_parallel", "plain_host", "chunks", "chunks_dropped", "waves", "declined",
                                          "bytes_up", "bytes_down")] + [("last_decline", C.c_int32), ("waits", C.c_int32)]


class TaxTree(C.Structure):
    _fields_ = [("parents", C.c_void_p), ("heights", C.c_void_p), ("n_taxa", C.c_uint64), ("s_tax_off", C.c_void_p),
                ("s_tax_ids", C.c_void_p), ("n_s", C.c_uint64)]


class TaxonFilter(C.Structure):
    _fields_ = [("taxa", C.c_void_p), ("n", C.c_uint64), ("exclude", C.c_int32), ("reserved", C.c_uint32)]


class LcaOptions(C.Structure):
    """lx_lca_options: top_percent 100 = the reference's rule, below it only the records within that share of the query's best bit score."""
    _fields_ = [("top_percent", C.c_double), ("reserved", C.c_uint64)]


class TaxmapResult(C.Structure):
    _fields_ = [("s_tax_off", C.c_void_p), ("s_tax_ids", C.c_void_p), ("n_s", C.c_uint64), ("present", C.c_void_p), ("n_present", C.c_uint64)] + [
        (n, C.c_uint64) for n in ("no_acc", "multi_acc", "no_tax", "multi_tax", "lines", "matched")]


class TaxonomyInfo(C.Structure):
    _fields_ = [("parents", C.c_void_p), ("heights", C.c_void_p), ("names", C.POINTER(C.c_char_p)), ("n_taxa", C.c_uint64),
                ("n_nodes", C.c_uint64), ("max_height", C.c_uint32), ("unnamed", C.c_uint32), ("warnings", C.c_char_p)]


LX_TAXMAP_NCBI, LX_TAXMAP_UNIPROT = 0, 1


class IndexInfo(C.Structure):
    _fields_ = [("n_entries", C.c_uint64), ("n_prefix", C.c_uint64), ("alph", C.c_int32), ("key_len", C.c_int32), ("prefix_len", C.c_int32),
                ("built_on_device", C.c_int32)]


INDEX_ENTRY_DTYPE = np.dtype([("key", "<u8"), ("seq", "<u4"), ("pos", "<u4")])


class SeedParams(C.Structure):
    """lx_seed_params (include/lambda_ext.h); seed_params() fills one from keywords."""
    _fields_ = [("seed_length", C.c_int32), ("seed_offset", C.c_int32), ("max_seed_dist", C.c_int32), ("half_exact", C.c_int32),
                ("adaptive", C.c_int32), ("pre_scoring", C.c_int32), ("pre_scoring_thresh", C.c_double), ("max_matches", C.c_uint64),
                ("q_num_frames", C.c_int32), ("unknown_rank", C.c_int32), ("matrix", C.c_void_p), ("matrix_rev", C.c_void_p),
                ("host_threads", C.c_uint32)]


class SegParams(C.Structure):
    """lx_seg_params: window 4 .. 64, 0 < k1 <= k2 <= log2(window) in bits; the defaults are SEG's."""
    _fields_ = [("window", C.c_int32), ("k1", C.c_double), ("k2", C.c_double)]

    def __init__(self, window: int = 12, k1: float = 2.2, k2: float = 2.5):
        super().__init__(window, k1, k2)


class DustParams(C.Structure):
    """lx_dust_params: window 4 .. 64 letters, level 1 .. 1000 (ten times the score bound); the defaults are dustmasker's and sdust's."""
    _fields_ = [("window", C.c_int32), ("level", C.c_int32)]

    def __init__(self, window: int = 64, level: int = 20):
        super().__init__(window, level)


class SeedStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_matches", "hits_after_seeding", "hits_failed_pre_extend", "reads_declined", "launches_full")]


class SeqNames(C.Structure):
    _fields_ = [("q_ids", C.POINTER(C.c_char_p)), ("q_lens", C.c_void_p), ("s_ids", C.POINTER(C.c_char_p)),
                ("s_lens", C.c_void_p), ("n_q", C.c_uint64), ("n_s", C.c_uint64)]


LX_OUT_BLAST_TAB, LX_OUT_BLAST_TAB_COMMENTS, LX_OUT_SAM, LX_OUT_BAM = 0, 1, 2, 3
LX_BGZF_EOF = 1


class Scoring(C.Structure):
    _fields_ = [("alphabet_size", C.c_int32), ("gap_open", C.c_int32), ("gap_extend", C.c_int32),
                ("reserved", C.c_int32), ("matrix", C.c_int8 * (LX_ALPH * LX_ALPH))]

    def matrix_np(self) -> np.ndarray:
        return np.ctypeslib.as_array(self.matrix).reshape(LX_ALPH, LX_ALPH).copy()


EXT_DTYPE = np.dtype([("q_off", "<u8"), ("s_off", "<u8"), ("q_len", "<u4"), ("s_len", "<u4")])
class SurvivorList(C.Structure):
    """lx_survivor_list (include/lambda_ext.h)."""
    _fields_ = [("count", C.c_uint64), ("index", C.c_void_p), ("hsp", C.c_void_p), ("codes_off", C.c_void_p), ("codes", C.c_void_p),
                ("codes_bytes", C.c_uint64)]


HSP_DTYPE = np.dtype([("score", "<i4"), ("q_begin", "<i4"), ("q_end", "<i4"), ("s_begin", "<i4"), ("s_end", "<i4"),
                      ("n_ops", "<i4"), ("num_matches", "<i4"), ("num_mismatches", "<i4"), ("num_positives", "<i4"),
                      ("num_gap_opens", "<i4"), ("num_gap_extensions", "<i4"), ("ops_shift", "<i4")])
MATCH_DTYPE = np.dtype([("qryId", "<u8"), ("subjId", "<u8"), ("qryStart", "<u8"), ("qryEnd", "<u8"),
                        ("subjStart", "<u8"), ("subjEnd", "<u8")])
SEED_DTYPE = np.dtype([("q_off", "<u8"), ("s_off", "<u8"), ("q_len", "<u4"), ("s_len", "<u4"),
                       ("qry_start", "<u4"), ("qry_end", "<u4"), ("subj_start", "<u4"), ("reserved", "<u4")])

_lib = None


class LambdaExtError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"lambda_ext error {code}: {msg}")
        self.code = code


def load():
    """Loads liblambda_ext.so (raises if it has not been built: the product path must fail loudly)."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise FileNotFoundError(f"{LIB_PATH} not built -- run `python -m lambda_amd.build` (needs hipcc)")
    # PyTorch wheels bundle their own libamdhip64/libhsa-runtime64.  Two HIP runtimes in one process do not work
    # (the second one sees no GPU), so if torch is going to be used in this process it must be loaded first; our
    # library then binds to the runtime that is already resident (same SONAME).  A C++ host links /opt/rocm's.
    try:
        import torch  # noqa: F401
    except Exception:  # torch is plumbing for tests/bench only, never a requirement of the C ABI
        pass
    lib = C.CDLL(str(LIB_PATH))
    vp, i32, u64 = C.c_void_p, C.c_int, C.c_uint64
    lib.lx_abi_version.restype = i32
    lib.lx_build_id.restype = C.c_char_p
    lib.lx_device_count.restype = i32
    lib.lx_create.argtypes = [i32, C.POINTER(vp)]
    lib.lx_destroy.argtypes = [vp]
    lib.lx_destroy.restype = None
    lib.lx_last_error.argtypes = [vp]
    lib.lx_last_error.restype = C.c_char_p
    lib.lx_set_option.argtypes = [vp, i32, u64]
    lib.lx_get_option.argtypes = [vp, i32, C.POINTER(u64)]
    lib.lx_host_threads_info.argtypes = [C.POINTER(C.c_uint32)] * 3
    lib.lx_plan_free_packing_bound.argtypes = [u64, u64, C.c_uint32]
    lib.lx_plan_free_packing_bound.restype = u64
    lib.lx_plan_free_packing_dev.argtypes = [vp, vp, u64, u64, i32, C.c_uint32, C.POINTER(u64), vp, vp, vp, vp]
    lib.lx_set_band_centres.argtypes = [vp, vp, u64]
    lib.lx_set_band_centres_dev.argtypes = [vp, vp]
    lib.lx_set_scoring.argtypes = [vp, i32, C.POINTER(Scoring)]
    lib.lx_builtin_scoring.argtypes = [i32, i32, i32, i32, i32, C.POINTER(Scoring)]
    lib.lx_score_batch.argtypes = [vp, i32, vp, u64, vp, u64, vp, u64, vp]
    lib.lx_score_batch_dev.argtypes = [vp, i32, vp, vp, vp, u64, vp, vp]
    lib.lx_synchronize.argtypes = [vp]
    lib.lx_last_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
    lib.lx_last_kernel_name.argtypes = [vp]
    lib.lx_last_kernel_name.restype = C.c_char_p
    lib.lx_last_trace_kernel_name.argtypes = [vp]
    lib.lx_last_trace_kernel_name.restype = C.c_char_p
    lib.lx_last_phase_ms.argtypes = [vp, i32, C.POINTER(C.c_float), C.POINTER(C.c_int)]
    for name, args in (("lx_align_batch", [vp, i32, vp, u64, vp, u64, vp, u64, vp, vp, vp, vp]),
                       ("lx_align_batch_dev", [vp, i32, vp, vp, vp, u64, vp, vp, vp, vp]),
                       ("lx_prefilter_batch", [vp, i32, vp, u64, vp, u64, vp, u64, C.c_uint32, C.c_int32, C.c_double, vp])):
        if hasattr(lib, name):
            getattr(lib, name).argtypes = args
    lib.lx_extend_batch_dev.argtypes = [vp, i32, vp, vp, vp, u64, vp, C.c_int32, vp, vp, vp, vp, vp, vp]
    lib.lx_karlin_params.argtypes = [i32, i32, i32, i32, i32, C.POINTER(Karlin)]
    lib.lx_length_adjustment.argtypes = [u64, u64, C.POINTER(Karlin)]
    lib.lx_length_adjustment.restype = u64
    lib.lx_evalue.argtypes = [C.c_int32, u64, u64, C.POINTER(Karlin)]
    lib.lx_evalue.restype = C.c_double
    lib.lx_bitscore.argtypes = [C.c_int32, C.POINTER(Karlin)]
    lib.lx_bitscore.restype = C.c_double
    lib.lx_convert_ranks.argtypes = [i32, vp, u64, vp]
    lib.lx_set_subjects.argtypes = [vp, vp, u64]
    lib.lx_extend_batch.argtypes = [vp, i32, vp, u64, vp, u64, vp, u64, vp, i32, vp, vp, vp, C.POINTER(vp), C.POINTER(u64)]
    lib.lx_extend_batch_rle.argtypes = lib.lx_extend_batch.argtypes
    lib.lx_extend_batch_list.argtypes = [vp, i32, vp, u64, vp, u64, vp, u64, vp, i32, vp, C.POINTER(SurvivorList)]
    lib.lx_expand_ops.argtypes = [vp, i32, vp]
    lib.lx_last_extend_stats.argtypes = [vp, vp]
    lib.lx_set_frames.argtypes = [i32, i32, u64, u64, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.lx_set_frames.restype = None
    lib.lx_untrue_qry_id.argtypes = [i32, u64, i32]
    lib.lx_untrue_qry_id.restype = u64
    lib.lx_untrue_subj_id.argtypes = [i32, u64, i32]
    lib.lx_untrue_subj_id.restype = u64
    lib.lx_translate_six_frames.argtypes = [vp, u64, i32, vp, u64, vp, vp]
    lib.lx_widen_and_preprocess.argtypes = [vp, u64, vp, vp]
    lib.lx_widen_and_preprocess.restype = u64
    lib.lx_iterate_matches.argtypes = [vp, i32, vp, u64, vp, vp, u64, vp, vp, u64, vp, vp, u64, vp, u64,
                                       C.POINTER(SearchParams), C.POINTER(vp)]
    lib.lx_set_queries.argtypes = [vp, vp, u64, vp, vp, u64, vp, i32]
    lib.lx_set_subject_seqs.argtypes = [vp, vp, vp, u64]
    lib.lx_iterate_matches_dev.argtypes = [vp, i32, vp, u64, C.POINTER(SearchParams), C.POINTER(vp)]
    lib.lx_trim_result_cache.restype = u64
    lib.lx_trim_result_cache.argtypes = []
    lib.lx_reserve.restype = i32
    lib.lx_reserve.argtypes = [vp, u64, u64, u64, u64]
    lib.lx_widen_and_preprocess_dev.argtypes = [vp, vp, u64, i32, vp, C.POINTER(u64)]
    lib.lx_sort_words_dev.argtypes = [i32, C.POINTER(vp), C.POINTER(vp), u64, u64, vp, C.POINTER(i32)]
    lib.lx_iterate_result_count.argtypes = [vp]
    lib.lx_iterate_result_count.restype = u64
    lib.lx_iterate_result_matches.argtypes = [vp]
    lib.lx_iterate_result_matches.restype = vp
    lib.lx_iterate_result_ops.argtypes = [vp]
    lib.lx_iterate_result_ops.restype = vp
    lib.lx_iterate_result_stats.argtypes = [vp]
    lib.lx_iterate_result_stats.restype = IterateStats
    lib.lx_iterate_result_free.argtypes = [vp]
    lib.lx_iterate_result_free.restype = None
    lib.lx_postprocess_records.argtypes = [vp, u64, u64, C.POINTER(RecordStats)]
    lib.lx_postprocess_records.restype = u64
    lib.lx_postprocess_records_dev.argtypes = [vp, vp, u64, u64, C.POINTER(RecordStats), C.POINTER(u64)]
    lib.lx_iterate_matches_dev_top.argtypes = [vp, i32, vp, u64, C.POINTER(SearchParams), u64, C.POINTER(RecordStats), C.POINTER(vp)]
    if hasattr(lib, "lx_postprocess_records_ex"):  # (not in an older library loaded through LX_LIB_PATH: the yardstick of tools/records_bench.py)
        lib.lx_cull_options_default.argtypes = [C.POINTER(CullOptions)]
        lib.lx_cull_options_default.restype = None
        lib.lx_postprocess_records_ex.argtypes = [vp, u64, u64, C.POINTER(CullOptions), C.POINTER(RecordStats), C.POINTER(CullStats)]
        lib.lx_postprocess_records_ex.restype = C.c_int64
        lib.lx_postprocess_records_dev_ex.argtypes = [vp, vp, u64, u64, C.POINTER(CullOptions), C.POINTER(RecordStats), C.POINTER(CullStats), C.POINTER(u64)]
        lib.lx_iterate_matches_dev_top_ex.argtypes = [vp, i32, vp, u64, C.POINTER(SearchParams), u64, C.POINTER(CullOptions), C.POINTER(RecordStats),
                                                      C.POINTER(CullStats), C.POINTER(vp)]
    lib.lx_write_records.argtypes = [C.c_char_p, i32, i32, C.c_char_p, vp, u64, vp, C.POINTER(SeqNames), vp, vp]
    lib.lx_write_records_ex.argtypes = [C.c_char_p, i32, i32, C.c_char_p, vp, u64, vp, C.POINTER(SeqNames), vp, vp, C.POINTER(OutputOptions)]
    lib.lx_write_footer.argtypes = [C.c_char_p, i32, u64]
    lib.lx_output_options_default.argtypes = [C.POINTER(OutputOptions)]
    lib.lx_output_options_default.restype = None
    lib.lx_last_output_error.restype = C.c_char_p
    lib.lx_compute_lca.argtypes = [vp, u64, C.POINTER(TaxTree), vp, vp, C.POINTER(u64)]
    lib.lx_lca_options_default.argtypes = [C.POINTER(LcaOptions)]
    lib.lx_lca_options_default.restype = None
    lib.lx_compute_lca_ex.argtypes = [vp, u64, C.POINTER(TaxTree), C.POINTER(LcaOptions), vp, vp, C.POINTER(u64)]
    lib.lx_check_tax_tree.argtypes = [C.POINTER(TaxTree)]
    lib.lx_tax_dev_create.argtypes = [vp, C.POINTER(TaxTree), C.POINTER(vp)]
    lib.lx_tax_dev_destroy.argtypes = [vp]
    lib.lx_tax_dev_destroy.restype = None
    lib.lx_compute_lca_dev.argtypes = [vp, vp, vp, u64, C.POINTER(LcaOptions), vp, vp, C.POINTER(u64)]
    lib.lx_tax_subject_mask.argtypes = [C.POINTER(TaxTree), C.POINTER(TaxonFilter), vp, C.POINTER(u64), vp]
    lib.lx_subject_mask_create_dev.argtypes = [vp, vp, C.POINTER(TaxonFilter), C.POINTER(vp)]
    lib.lx_subject_mask_create.argtypes = [vp, vp, u64, C.POINTER(vp)]
    lib.lx_subject_mask_info.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
    lib.lx_subject_mask_copy.argtypes = [vp, vp]
    lib.lx_subject_mask_destroy.argtypes = [vp]
    lib.lx_subject_mask_destroy.restype = None
    lib.lx_seed_result_filter.argtypes = [vp, vp, C.c_int32, C.POINTER(u64), C.POINTER(u64)]
    lib.lx_render_records.argtypes = [i32, i32, C.c_char_p, vp, u64, vp, C.POINTER(SeqNames), vp, vp, C.POINTER(OutputOptions), C.c_int64, C.POINTER(vp)]
    lib.lx_bytes_data.argtypes = [vp]
    lib.lx_bytes_data.restype = vp
    lib.lx_bytes_size.argtypes = [vp]
    lib.lx_bytes_size.restype = u64
    lib.lx_bytes_free.argtypes = [vp]
    lib.lx_bytes_free.restype = None
    lib.lx_bgzf_bound.argtypes = [u64]
    lib.lx_bgzf_bound.restype = u64
    lib.lx_bgzf_compress.argtypes = [vp, vp, u64, vp, u64, C.POINTER(u64), i32]
    lib.lx_gunzip.argtypes = [vp, vp, u64, C.POINTER(vp)]
    lib.lx_last_gunzip_stats.argtypes = [vp, C.POINTER(GunzipStats)]
    lib.lx_gunzip_decline_text.argtypes = [i32]
    lib.lx_gunzip_decline_text.restype = C.c_char_p
    lib.lx_gunzip_stream_open.argtypes = [vp, C.c_char_p, u64, C.POINTER(vp)]
    lib.lx_gunzip_stream_next.argtypes = [vp, C.POINTER(vp)]
    lib.lx_gunzip_stream_close.argtypes = [vp]
    lib.lx_gunzip_stream_close.restype = None
    lib.lx_find_accessions.argtypes = [vp, u64, vp, vp, u64, C.POINTER(u64)]
    lib.lx_taxmap_create.argtypes = [vp, i32, vp, vp, u64, u64, C.c_uint32, C.POINTER(vp)]
    lib.lx_taxmap_feed.argtypes = [vp, vp, u64]
    lib.lx_taxmap_finish.argtypes = [vp, C.POINTER(TaxmapResult)]
    lib.lx_taxmap_destroy.argtypes = [vp]
    lib.lx_taxmap_destroy.restype = None
    lib.lx_taxonomy_build.argtypes = [C.c_char_p, u64, C.c_char_p, u64, vp, u64, C.POINTER(vp)]
    lib.lx_taxonomy_get.argtypes = [vp, C.POINTER(TaxonomyInfo)]
    lib.lx_taxonomy_free.argtypes = [vp]
    lib.lx_taxonomy_free.restype = None
    lib.lx_index_build.argtypes = [vp, vp, vp, vp, u64, i32, C.c_uint32, C.POINTER(vp)]
    lib.lx_index_plan_slices.argtypes = [vp, u64, u64, vp, u64, C.POINTER(u64)]
    lib.lx_index_load.argtypes = [vp, vp, u64, vp, vp, vp, u64, C.POINTER(vp)]
    lib.lx_index_save.argtypes = [vp, C.POINTER(vp)]
    lib.lx_index_attach.argtypes = [vp, vp, C.POINTER(vp)]
    lib.lx_index_get_info.argtypes = [vp, C.POINTER(IndexInfo)]
    lib.lx_index_copy_entries.argtypes = [vp, u64, u64, vp]
    lib.lx_index_destroy.argtypes = [vp]
    lib.lx_index_destroy.restype = None
    lib.lx_seed_queries.argtypes = [vp, vp, vp, vp, vp, vp, vp, u64, vp, u64, C.POINTER(SeedParams), C.POINTER(vp)]
    if hasattr(lib, "lx_seed_queries_masked"):  # (not in an older library loaded through LX_LIB_PATH: the yardstick of tools/query_mask_bench.py)
        lib.lx_seed_queries_masked.argtypes = [vp, vp, vp, vp, vp, vp, vp, u64, vp, u64, vp, C.POINTER(SeedParams), C.POINTER(vp)]
        lib.lx_seg_params_default.argtypes = [C.POINTER(SegParams)]
        lib.lx_seg_params_default.restype = None
        lib.lx_seg_tables.argtypes = [C.POINTER(SegParams), vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        lib.lx_query_mask_create_seg.argtypes = [vp, vp, vp, vp, u64, C.POINTER(SegParams), C.c_uint32, C.POINTER(vp)]
        lib.lx_query_mask_create.argtypes = [vp, vp, vp, vp, u64, C.POINTER(vp)]
        lib.lx_query_mask_info.argtypes = [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
        lib.lx_query_mask_copy.argtypes = [vp, vp]
        lib.lx_query_mask_destroy.argtypes = [vp]
        lib.lx_query_mask_destroy.restype = None
    if hasattr(lib, "lx_query_mask_create_dust"):
        lib.lx_dust_params_default.argtypes = [C.POINTER(DustParams)]
        lib.lx_dust_params_default.restype = None
        lib.lx_query_mask_create_dust.argtypes = [vp, vp, vp, vp, u64, C.POINTER(DustParams), C.c_uint32, C.POINTER(vp)]
    lib.lx_seed_result_stats.argtypes = [vp]
    lib.lx_seed_result_stats.restype = SeedStats
    lib.lx_seed_result_matches.argtypes = [vp]
    lib.lx_seed_result_matches.restype = vp
    lib.lx_seed_result_matches_dev.argtypes = [vp]
    lib.lx_seed_result_matches_dev.restype = vp
    lib.lx_seed_result_free.argtypes = [vp]
    lib.lx_seed_result_free.restype = None
    lib.lx_write_records_bgzf.argtypes = [vp, C.c_char_p, i32, C.c_char_p, vp, u64, vp, C.POINTER(SeqNames), vp, vp, C.POINTER(OutputOptions),
                                          C.c_int64]
    lib.lx_render_bam_dev.argtypes = [vp, i32, C.c_char_p, vp, u64, vp, u64, C.POINTER(SeqNames), vp, vp, C.POINTER(OutputOptions), C.POINTER(vp)]
    lib.lx_write_bam_dev.argtypes = [vp, C.c_char_p, C.c_char_p, vp, u64, vp, u64, C.POINTER(SeqNames), vp, vp, C.POINTER(OutputOptions)]
    lib.lx_format_number.argtypes = [i32, C.c_double, C.c_char_p, u64]
    lib.lx_render_text_dev.argtypes = [vp, i32, i32, C.c_char_p, vp, u64, vp, u64, C.POINTER(SeqNames), vp, vp, C.POINTER(OutputOptions), C.c_int64,
                                       C.POINTER(vp)]
    lib.lx_write_text_dev.argtypes = [vp, C.c_char_p, i32, i32, C.c_char_p, vp, u64, vp, u64, C.POINTER(SeqNames), vp, vp, C.POINTER(OutputOptions),
                                      C.c_int64]
    lib.lx_out_open.argtypes = [vp, C.c_char_p, i32, i32, C.c_char_p, C.POINTER(SeqNames), C.POINTER(OutputOptions), C.POINTER(vp)]
    lib.lx_out_append.argtypes = [vp, i32, vp, u64, vp, u64, C.POINTER(SeqNames), vp, vp, vp, vp, u64]
    if hasattr(lib, "lx_out_append_ex"):  # (not in an older library loaded through LX_LIB_PATH: the yardstick of tools/bam_render_bench.py --parent)
        lib.lx_out_append_ex.restype = i32
        lib.lx_out_append_ex.argtypes = [vp, i32, vp, u64, vp, u64, C.POINTER(SeqNames), vp, vp, vp, vp, vp, u64]
    lib.lx_out_close.argtypes = [vp, C.c_int64]
    _lib = lib
    return lib


def compute_lca(bms: np.ndarray, parents, heights, s_tax_off, s_tax_ids):
    """The LCA step of _writeRecord (src/search_algo.hpp:884-907) over a result list grouped by query: (n_qid, lcaTaxId) arrays."""
    m = np.ascontiguousarray(bms, dtype=BLAST_MATCH_DTYPE)
    par = np.ascontiguousarray(parents, dtype=np.uint32)
    hgt = np.ascontiguousarray(heights, dtype=np.uint32)
    off = np.ascontiguousarray(s_tax_off, dtype=np.uint64)
    ids = np.ascontiguousarray(s_tax_ids, dtype=np.uint32)
    tree = TaxTree(par.ctypes.data, hgt.ctypes.data, len(par), off.ctypes.data, ids.ctypes.data if len(ids) else None, len(off) - 1)
    qid = np.zeros(max(len(m), 1), dtype=np.uint64)
    lca = np.zeros(max(len(m), 1), dtype=np.uint32)
    cnt = C.c_uint64(0)
    rc = load().lx_compute_lca(_ptr(m) if len(m) else None, len(m), C.byref(tree), _ptr(qid), _ptr(lca), C.byref(cnt))
    if rc != 0:
        raise LambdaExtError(rc, "lx_compute_lca: ids outside the taxonomy, or a path that does not lead to the root")
    return qid[: cnt.value].copy(), lca[: cnt.value].copy()


def _tax_tree(parents, heights, s_tax_off, s_tax_ids):
    """An lx_tax_tree over the four arrays (returned too: they must outlive the calls that read the tree)."""
    par = np.ascontiguousarray(parents, dtype=np.uint32)
    hgt = np.ascontiguousarray(heights, dtype=np.uint32)
    off = np.ascontiguousarray(s_tax_off, dtype=np.uint64)
    ids = np.ascontiguousarray(s_tax_ids, dtype=np.uint32)
    tree = TaxTree(par.ctypes.data if len(par) else None, hgt.ctypes.data if len(hgt) else None, len(par), off.ctypes.data,
                   ids.ctypes.data if len(ids) else None, len(off) - 1)
    return tree, (par, hgt, off, ids)


def lca_options(top_percent: float = 100.0) -> LcaOptions:
    o = LcaOptions()
    load().lx_lca_options_default(C.byref(o))
    o.top_percent = top_percent
    return o


def compute_lca_ex(bms: np.ndarray, parents, heights, s_tax_off, s_tax_ids, top_percent: float = 100.0):
    """lx_compute_lca_ex: compute_lca over the records whose bit score lies within top_percent percent of their query's best
    (100 = all of them, the reference's rule): (n_qid, lcaTaxId) arrays."""
    m = np.ascontiguousarray(bms, dtype=BLAST_MATCH_DTYPE)
    tree, keep = _tax_tree(parents, heights, s_tax_off, s_tax_ids)
    qid = np.zeros(max(len(m), 1), dtype=np.uint64)
    lca = np.zeros(max(len(m), 1), dtype=np.uint32)
    cnt = C.c_uint64(0)
    opt = lca_options(top_percent)
    rc = load().lx_compute_lca_ex(_ptr(m) if len(m) else None, len(m), C.byref(tree), C.byref(opt), _ptr(qid), _ptr(lca), C.byref(cnt))
    if rc != 0:
        raise LambdaExtError(rc, "lx_compute_lca_ex: " + (last_output_error() or "ids outside the taxonomy, or a path that does not lead to the root"))
    return qid[: cnt.value].copy(), lca[: cnt.value].copy()


def check_tax_tree(parents, heights, s_tax_off, s_tax_ids):
    """lx_check_tax_tree: raises LambdaExtError with the broken rule unless every climb on the tree ends."""
    tree, keep = _tax_tree(parents, heights, s_tax_off, s_tax_ids)
    rc = load().lx_check_tax_tree(C.byref(tree))
    if rc != LX_OK:
        raise LambdaExtError(rc, last_output_error())


class TaxDev:
    """lx_tax_dev: a taxonomic tree resident on a handle's device (checked by lx_check_tax_tree first).  Close it before its handle."""

    def __init__(self, handle: "Handle", parents, heights, s_tax_off, s_tax_ids):
        self.lib = load()
        self.handle = handle
        tree, keep = _tax_tree(parents, heights, s_tax_off, s_tax_ids)
        t = C.c_void_p()
        handle._check(self.lib.lx_tax_dev_create(handle.h, C.byref(tree), C.byref(t)))
        self.t = t

    def close(self):
        if getattr(self, "t", None):
            self.lib.lx_tax_dev_destroy(self.t)
            self.t = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        self.close()


def taxon_filter(taxa, exclude: bool = False):
    """An lx_taxon_filter over `taxa` (returned with the array that must outlive the calls that read it)."""
    arr = np.ascontiguousarray(taxa, dtype=np.uint32)
    return TaxonFilter(arr.ctypes.data if len(arr) else None, len(arr), int(bool(exclude)), 0), arr


def subject_mask(parents, heights, s_tax_off, s_tax_ids, taxa, exclude: bool = False):
    """lx_tax_subject_mask, the rule on the host: (words as uint64, one bit per subject; n_kept; known, one byte per listed taxon)."""
    tree, keep = _tax_tree(parents, heights, s_tax_off, s_tax_ids)
    f, arr = taxon_filter(taxa, exclude)
    words = np.zeros((int(tree.n_s) + 63) // 64, dtype=np.uint64)
    known = np.zeros(max(len(arr), 1), dtype=np.uint8)
    kept = C.c_uint64(0)
    rc = load().lx_tax_subject_mask(C.byref(tree), C.byref(f), _ptr(words) if len(words) else words.ctypes.data, C.byref(kept), _ptr(known))
    if rc != LX_OK:
        raise LambdaExtError(rc, last_output_error())
    return words, int(kept.value), known[: len(arr)].copy()


def mask_bits(words: np.ndarray, n_s: int) -> np.ndarray:
    """The first n_s bits of mask words as a bool array (bit s of word s // 64)."""
    return np.unpackbits(np.ascontiguousarray(words, dtype="<u8").view(np.uint8), bitorder="little")[:n_s].astype(bool)


class SubjectMask:
    """lx_subject_mask: one bit per subject.  from_words(handle or None, words, n_s) takes given words (with a handle they are also
    uploaded); from_taxa(handle, tax_dev, taxa, exclude) makes them by kernels over a resident tree.  Close it before its handle."""

    def __init__(self, m, handle=None):
        self.lib, self.m, self.handle = load(), m, handle

    @classmethod
    def from_words(cls, handle: "Handle | None", words, n_s: int) -> "SubjectMask":
        lib, w, out = load(), np.ascontiguousarray(words, dtype=np.uint64), C.c_void_p()
        h = handle.h if handle is not None else None
        rc = lib.lx_subject_mask_create(h, w.ctypes.data if len(w) else None, n_s, C.byref(out))
        if rc != LX_OK:
            raise LambdaExtError(rc, last_output_error())
        return cls(out, handle)

    @classmethod
    def from_taxa(cls, handle: "Handle", tax_dev: "TaxDev", taxa, exclude: bool = False) -> "SubjectMask":
        lib, out = load(), C.c_void_p()
        f, arr = taxon_filter(taxa, exclude)
        handle._check(lib.lx_subject_mask_create_dev(handle.h, tax_dev.t if tax_dev is not None else None, C.byref(f), C.byref(out)))
        return cls(out, handle)

    def info(self):
        """(n_s, n_kept)"""
        n_s, kept = C.c_uint64(0), C.c_uint64(0)
        self.lib.lx_subject_mask_info(self.m, C.byref(n_s), C.byref(kept))
        return int(n_s.value), int(kept.value)

    def words(self) -> np.ndarray:
        w = np.zeros((self.info()[0] + 63) // 64, dtype=np.uint64)
        if self.lib.lx_subject_mask_copy(self.m, w.ctypes.data if len(w) else None) != LX_OK:
            raise LambdaExtError(LX_EINVAL, last_output_error())
        return w

    def close(self):
        if getattr(self, "m", None):
            self.lib.lx_subject_mask_destroy(self.m)
            self.m = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    __del__ = close


def seed_result_filter(result: "SeedResult", mask: SubjectMask, sbj_num_frames: int = 1):
    """lx_seed_result_filter: drops the matches whose subject (subjId // sbj_num_frames) has a 0 bit, in place and in order:
    (n_before, n_kept)."""
    before, kept = C.c_uint64(0), C.c_uint64(0)
    rc = load().lx_seed_result_filter(result.r, mask.m if mask is not None else None, sbj_num_frames, C.byref(before), C.byref(kept))
    if rc != LX_OK:
        raise LambdaExtError(rc, last_output_error())
    return int(before.value), int(kept.value)


def postprocess_records(bms: np.ndarray, max_matches: int = 25):
    """_writeRecord's sort / dedupe / top-N (src/search_algo.hpp:820-913) over a result list grouped by query."""
    m = np.ascontiguousarray(bms, dtype=BLAST_MATCH_DTYPE).copy()
    st = RecordStats()
    n = load().lx_postprocess_records(_ptr(m), len(m), max_matches, C.byref(st))
    return m[: int(n)], st


def postprocess_records_dev(handle, bms: np.ndarray, max_matches: int = 25):
    """lx_postprocess_records_dev: postprocess_records with the sort / dedupe / top-N as kernels on `handle`'s device; (rows, stats)."""
    m = np.ascontiguousarray(bms, dtype=BLAST_MATCH_DTYPE).copy()
    st = RecordStats()
    n = C.c_uint64(0)
    handle._check(handle.lib.lx_postprocess_records_dev(handle.h, _ptr(m) if len(m) else None, len(m), max_matches, C.byref(st), C.byref(n)))
    return m[: int(n.value)], st


def cull_options(max_hsps: int = 0, culling_limit: int = 0, q_lens=None, q_translated: bool = False):
    """An lx_cull_options and the uint64 array it points into (keep it alive as long as the options): (CullOptions, array)."""
    lens = None if q_lens is None else np.ascontiguousarray(q_lens, dtype=np.uint64)
    opt = CullOptions()
    load().lx_cull_options_default(C.byref(opt))
    opt.max_hsps, opt.culling_limit, opt.q_translated = max_hsps, culling_limit, 1 if q_translated else 0
    opt.q_lens, opt.n_q = (lens.ctypes.data if lens is not None and len(lens) else None), (0 if lens is None else len(lens))
    return opt, lens


def postprocess_records_ex(bms: np.ndarray, max_matches: int = 25, max_hsps: int = 0, culling_limit: int = 0, q_lens=None, q_translated: bool = False):
    """lx_postprocess_records_ex: postprocess_records with --max-hsps / --culling-limit between the unique and the cut;
    (rows, stats, cull stats).  Raises LambdaExtError with lx_last_output_error()'s text on a refusal."""
    m = np.ascontiguousarray(bms, dtype=BLAST_MATCH_DTYPE).copy()
    opt, _keep = cull_options(max_hsps, culling_limit, q_lens, q_translated)
    st, cs = RecordStats(), CullStats()
    n = load().lx_postprocess_records_ex(_ptr(m) if len(m) else None, len(m), max_matches, C.byref(opt), C.byref(st), C.byref(cs))
    if n < 0:
        raise LambdaExtError(int(n), last_output_error())
    return m[: int(n)], st, cs


def postprocess_records_dev_ex(handle, bms: np.ndarray, max_matches: int = 25, max_hsps: int = 0, culling_limit: int = 0, q_lens=None, q_translated: bool = False):
    """lx_postprocess_records_dev_ex: postprocess_records_ex with the step as kernels on `handle`'s device; (rows, stats, cull stats)."""
    m = np.ascontiguousarray(bms, dtype=BLAST_MATCH_DTYPE).copy()
    opt, _keep = cull_options(max_hsps, culling_limit, q_lens, q_translated)
    st, cs, n = RecordStats(), CullStats(), C.c_uint64(0)
    handle._check(handle.lib.lx_postprocess_records_dev_ex(handle.h, _ptr(m) if len(m) else None, len(m), max_matches, C.byref(opt), C.byref(st), C.byref(cs), C.byref(n)))
    return m[: int(n.value)], st, cs


class OutputOptions(C.Structure):
    """lx_output_options (include/lambda_ext.h): the reference's output options, src/search_options.hpp:224-379."""
    _fields_ = [("columns", C.c_char_p), ("sam_tags", C.c_char_p), ("sam_seq", C.c_int32), ("sam_hard_clip", C.c_int32),
                ("sam_with_ref_header", C.c_int32), ("version_to_output", C.c_int32), ("version", C.c_char_p), ("command_line", C.c_char_p),
                ("db_name", C.c_char_p), ("genetic_code", C.c_int32), ("reserved", C.c_int32), ("tax", C.c_void_p), ("lca_qid", C.c_void_p),
                ("lca_tax", C.c_void_p), ("n_lca", C.c_uint64), ("tax_names", C.c_void_p), ("q_qual", C.c_void_p)]


LX_SAM_SEQ_NEVER, LX_SAM_SEQ_UNIQ, LX_SAM_SEQ_ALWAYS = 0, 1, 2


def output_options(**kw) -> OutputOptions:
    """lx_output_options_default, then the given fields (str values are encoded)."""
    o = OutputOptions()
    load().lx_output_options_default(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v.encode() if isinstance(v, str) else v)
    return o


def last_output_error() -> str:
    return (load().lx_last_output_error() or b"").decode()


def write_footer(path, fmt: int, n_records: int):
    rc = load().lx_write_footer(str(path).encode(), fmt, C.c_uint64(n_records))
    if rc != LX_OK:
        raise LambdaExtError(rc, "lx_write_footer")


def _with_qual(options, q_qual):
    """`options` with q_qual pointing at the bytes (a copy; the defaults for None), and the array that must outlive the call.  q_qual
    None: `options` itself."""
    if q_qual is None:
        return options, None
    o = OutputOptions()
    if options is None:
        load().lx_output_options_default(C.byref(o))
    else:
        C.memmove(C.byref(o), C.byref(options), C.sizeof(o))
    arr = np.frombuffer(q_qual, dtype=np.uint8)
    o.q_qual = arr.ctypes.data if len(arr) else None
    return o, (arr, options)


def _writer_args(bms, ops, q_ids, q_lens, s_ids, s_lens, q_ascii, q_ascii_off, options, q_qual=None):
    """The arguments the writers share (the arrays are returned too: they must outlive the call).  q_qual: the queries' Phred+33
    qualities, parallel to q_ascii (lx_output_options::q_qual)."""
    options, keep_qual = _with_qual(options, q_qual)
    m = np.ascontiguousarray(bms, dtype=BLAST_MATCH_DTYPE)
    qa = (C.c_char_p * len(q_ids))(*[x.encode() for x in q_ids])
    sa = (C.c_char_p * len(s_ids))(*[x.encode() for x in s_ids])
    ql = np.ascontiguousarray(q_lens, dtype=np.uint64)
    sl = np.ascontiguousarray(s_lens, dtype=np.uint64)
    names = SeqNames(qa, ql.ctypes.data, sa, sl.ctypes.data, len(q_ids), len(s_ids))
    o = np.frombuffer(ops + b"\0", dtype=np.uint8)
    qasc = np.frombuffer(q_ascii, dtype=np.uint8) if q_ascii else None
    qoff = np.ascontiguousarray(q_ascii_off, dtype=np.uint64) if q_ascii_off is not None else None
    args = (_ptr(m), len(m), _ptr(o), C.byref(names), _ptr(qasc) if qasc is not None else None, _ptr(qoff) if qoff is not None else None,
            C.byref(options) if options is not None else None)
    return args, (m, qa, sa, ql, sl, names, o, qasc, qoff, options, keep_qual)


def render_records(fmt: int, bms: np.ndarray, ops: bytes, q_ids, q_lens, s_ids, s_lens, program="blastp", write_header=True,
                   q_ascii: bytes | None = None, q_ascii_off=None, options: OutputOptions | None = None, footer_records: int = -1, q_qual: bytes | None = None) -> bytes:
    """lx_render_records: the bytes of a text format (what write_records + write_footer put in a file), or the uncompressed BAM
    stream (LX_OUT_BAM).  footer_records < 0: no footer."""
    args, keep = _writer_args(bms, ops, q_ids, q_lens, s_ids, s_lens, q_ascii, q_ascii_off, options, q_qual)
    lib = load()
    out = C.c_void_p()
    rc = lib.lx_render_records(fmt, 1 if write_header else 0, program.encode(), *args, footer_records, C.byref(out))
    if rc != LX_OK:
        raise LambdaExtError(rc, "lx_render_records: " + last_output_error())
    try:
        return C.string_at(lib.lx_bytes_data(out), lib.lx_bytes_size(out)) if lib.lx_bytes_size(out) else b""
    finally:
        lib.lx_bytes_free(out)


LX_RENDER_HOST, LX_RENDER_DEV = 0, 1


class Out:
    """lx_out_*: an output file written piece by piece; after close() it is byte for byte the file the one-shot writers make from the
    concatenated list.  handle None: a plain text file rendered on the host.  bgzf (always for LX_OUT_BAM): BGZF-compressed on the
    handle's device.  append() takes whole query groups; its query ids, lengths, letters and LCA pairs are those of the piece, the
    records' n_qid count within it."""

    def __init__(self, handle: "Handle | None", path, fmt: int, s_ids, s_lens, program="blastp", bgzf=False,
                 options: OutputOptions | None = None):
        self.lib, self.handle, self.o = load(), handle, C.c_void_p()
        sa = (C.c_char_p * len(s_ids))(*[x.encode() for x in s_ids])
        sl = np.ascontiguousarray(s_lens, dtype=np.uint64)
        self._keep = (sa, sl, options)  # (the library reads the subjects until close)
        subjects = SeqNames(None, None, sa, sl.ctypes.data, 0, len(s_ids))
        self._check(self.lib.lx_out_open(handle.h if handle is not None else None, os.fsencode(path), fmt, 1 if bgzf else 0, program.encode(),
                                         C.byref(subjects), C.byref(options) if options is not None else None, C.byref(self.o)))

    def _check(self, rc):
        if rc != LX_OK:
            raise LambdaExtError(rc, self.lib.lx_last_error(self.handle.h).decode() if self.handle is not None else last_output_error())

    def append(self, where: int, bms: np.ndarray, ops: bytes, q_ids, q_lens, q_ascii: bytes | None = None, q_ascii_off=None,
               lca_qid=None, lca_tax=None, q_qual: bytes | None = None):
        """lx_out_append, or lx_out_append_ex when the piece's qualities are given (q_qual, parallel to q_ascii)."""
        args, keep = _writer_args(bms, ops, q_ids, q_lens, [], [], q_ascii, q_ascii_off, None)
        lq = np.ascontiguousarray(lca_qid, dtype=np.uint64) if lca_qid is not None else None
        lt = np.ascontiguousarray(lca_tax, dtype=np.uint32) if lca_tax is not None else None
        lca = (_ptr(lq) if lq is not None and len(lq) else None, _ptr(lt) if lt is not None and len(lt) else None, len(lq) if lq is not None else 0)
        if q_qual is None:
            self._check(self.lib.lx_out_append(self.o, where, *args[:3], len(ops), *args[3:6], *lca))
        else:
            qq = np.frombuffer(q_qual, dtype=np.uint8)
            self._check(self.lib.lx_out_append_ex(self.o, where, *args[:3], len(ops), *args[3:6], _ptr(qq) if len(qq) else None, *lca))

    def close(self, footer_records: int = -1):
        o, self.o = self.o, C.c_void_p()
        if o:
            self._check(self.lib.lx_out_close(o, footer_records))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


LX_NUM_E1, LX_NUM_F1, LX_NUM_F2, LX_NUM_G_FLOAT = 0, 1, 2, 3


def format_number(kind: int, v: float, cap: int = 32) -> str:
    """lx_format_number: the text printf makes of v ("%.1e", "%.1f", "%.2f", or "%g" of a float widened to double), by the integer
    formatter the device text writers print with.  LambdaExtError(LX_EINVAL) for a short cap, an unknown kind, an F value outside
    |v| < 1e15."""
    buf = C.create_string_buffer(max(cap, 1))
    n = load().lx_format_number(kind, C.c_double(v), buf, cap)
    if n < 0:
        raise LambdaExtError(n, "lx_format_number")
    return buf.raw[:n].decode("ascii")


def bgzf_bound(n: int) -> int:
    return int(load().lx_bgzf_bound(n))


def gunzip(handle: "Handle | None", data: bytes) -> bytes:
    """lx_gunzip: the bytes of a gzip stream of one or more members.  BGZF members are decoded on the handle's device, and so are
    plain members of LX_OPT_GUNZIP_PARALLEL_FROM bytes or more (in chunks, in parallel; Handle.last_gunzip_stats() says what went
    where); every other member on this thread; handle None = every member on the host.  Malformed input raises LambdaExtError(LX_EINVAL) with the
    library's message, which names the member and its byte offset."""
    lib = load()
    buf = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, np.uint8)
    out = C.c_void_p()
    h = handle.h if handle is not None else None
    rc = lib.lx_gunzip(h, _ptr(buf), len(data), C.byref(out))
    if rc != LX_OK:
        raise LambdaExtError(rc, lib.lx_last_error(h).decode() if h is not None else last_output_error())
    try:
        return C.string_at(lib.lx_bytes_data(out), lib.lx_bytes_size(out)) if lib.lx_bytes_size(out) else b""
    finally:
        lib.lx_bytes_free(out)


def gunzip_stream(handle: "Handle | None", path, piece_bytes: int = 0):
    """lx_gunzip_stream_*: yields the pieces of the file's decompressed text (of the file's own bytes when it is not gzip), each of
    at most piece_bytes + 65536 bytes (0 = 64 MiB); concatenated they are gunzip(handle, the file's bytes).  BGZF members are decoded
    in groups on the handle's device (handle None: on this thread), plain members of LX_OPT_GUNZIP_PARALLEL_FROM bytes or more wave by
    wave on it, every other member on this thread with a 32 KiB window.  Handle.last_gunzip_stats() and last_phase_ms(10) after a piece
    are those of the call that made it; once the generator has ended the stats are those of the whole file.  A corrupt stream raises LambdaExtError(LX_EINVAL) from the piece that reaches the damage,
    with gunzip's message."""
    lib = load()
    h = handle.h if handle is not None else None

    def error(rc):
        return LambdaExtError(rc, lib.lx_last_error(h).decode() if h is not None else last_output_error())

    s = C.c_void_p()
    rc = lib.lx_gunzip_stream_open(h, os.fsencode(path) if path is not None else None, piece_bytes, C.byref(s))
    if rc != LX_OK:
        raise error(rc)
    try:
        while True:
            out = C.c_void_p()
            rc = lib.lx_gunzip_stream_next(s, C.byref(out))
            if rc != LX_OK:
                raise error(rc)
            if not out:
                return
            try:
                piece = C.string_at(lib.lx_bytes_data(out), lib.lx_bytes_size(out))
            finally:
                lib.lx_bytes_free(out)
            yield piece
    finally:
        lib.lx_gunzip_stream_close(s)


def find_accessions(text: bytes):
    """lx_find_accessions: every non-overlapping match of the reference's accession regex in `text`, as (start, length) pairs."""
    lib = load()
    buf = np.frombuffer(text, dtype=np.uint8) if len(text) else np.zeros(1, np.uint8)
    cnt = C.c_uint64()
    if lib.lx_find_accessions(_ptr(buf), len(text), None, None, 0, C.byref(cnt)) != LX_OK:
        raise LambdaExtError(LX_EINVAL, "lx_find_accessions")
    beg = np.zeros(max(cnt.value, 1), np.uint64)
    ln = np.zeros(max(cnt.value, 1), np.uint32)
    if lib.lx_find_accessions(_ptr(buf), len(text), _ptr(beg), _ptr(ln), cnt.value, C.byref(cnt)) != LX_OK:
        raise LambdaExtError(LX_EINVAL, "lx_find_accessions")
    return [(int(b), int(l)) for b, l in zip(beg[: cnt.value], ln[: cnt.value])]


class TaxMap:
    """lx_taxmap_*: the accession table of the subject ids joined with an accession-to-taxon map fed in pieces.  handle None = the
    library's host threads (`threads` parts, 0 = its default); chunk_bytes 0 = 256 MiB.  finish() returns a dict: s_tax_off,
    s_tax_ids, present (numpy arrays) and the counts.  Errors raise LambdaExtError with the library's message."""

    def __init__(self, handle: "Handle | None", fmt: int, ids, chunk_bytes: int = 0, threads: int = 0):
        self.lib = load()
        self.hh = handle.h if handle is not None else None
        raw = [x.encode() if isinstance(x, str) else bytes(x) for x in ids]
        off = np.zeros(len(raw) + 1, np.uint64)
        off[1:] = np.cumsum([len(x) for x in raw]) if raw else []
        blob = np.frombuffer(b"".join(raw) or b"\0", dtype=np.uint8)
        tm = C.c_void_p()
        rc = self.lib.lx_taxmap_create(self.hh, fmt, _ptr(blob), _ptr(off), len(raw), chunk_bytes, threads, C.byref(tm))
        self._check(rc)
        self.tm = tm

    def _check(self, rc):
        if rc != LX_OK:
            raise LambdaExtError(rc, self.lib.lx_last_error(self.hh).decode() if self.hh is not None else last_output_error())

    def feed(self, data: bytes):
        buf = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, np.uint8)
        self._check(self.lib.lx_taxmap_feed(self.tm, _ptr(buf), len(data)))

    def finish(self):
        r = TaxmapResult()
        self._check(self.lib.lx_taxmap_finish(self.tm, C.byref(r)))
        off = np.ctypeslib.as_array(C.cast(r.s_tax_off, C.POINTER(C.c_uint64)), (r.n_s + 1,)).copy()
        nids = int(off[-1])
        ids = np.ctypeslib.as_array(C.cast(r.s_tax_ids, C.POINTER(C.c_uint32)), (nids,)).copy() if nids else np.zeros(0, np.uint32)
        present = np.ctypeslib.as_array(C.cast(r.present, C.POINTER(C.c_uint32)), (r.n_present,)).copy()
        out = {"s_tax_off": off, "s_tax_ids": ids, "present": present}
        out.update({n: int(getattr(r, n)) for n in ("no_acc", "multi_acc", "no_tax", "multi_tax", "lines", "matched")})
        return out

    def close(self):
        if getattr(self, "tm", None):
            self.lib.lx_taxmap_destroy(self.tm)
            self.tm = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        self.close()


def _raise(lib, h, rc):
    raise LambdaExtError(rc, lib.lx_last_error(h).decode() if h is not None else last_output_error())


def index_plan_slices(pre, slice_words: int) -> np.ndarray:
    """lx_index_plan_slices: the first bucket of every slice the sliced build (LX_OPT_INDEX_SLICE_WORDS) cuts the prefix table
    `pre` into; no device is touched."""
    lib = load()
    pre = np.ascontiguousarray(pre, dtype=np.uint64)
    n = C.c_uint64()
    rc = lib.lx_index_plan_slices(_ptr(pre) if pre.size else None, pre.size, slice_words, None, 0, C.byref(n))
    if rc != LX_OK:
        _raise(lib, None, rc)
    first = np.zeros(n.value, np.uint64)
    rc = lib.lx_index_plan_slices(_ptr(pre), pre.size, slice_words, _ptr(first), first.size, C.byref(n))
    if rc != LX_OK:
        _raise(lib, None, rc)
    return first


class Index:
    """lx_index: the sorted word table over reduced, frame-expanded subjects (Level 3).  Index.build / Index.load / attach make
    one; handle None = on the host threads, no device; with a handle the table and the reduced subjects stay on its device.
    Destroy (close) an index before its handle."""

    def __init__(self, ix, handle):
        self.lib, self.ix, self.handle = load(), ix, handle

    @staticmethod
    def _seqs(s_red, s_off, s_len):
        red = np.ascontiguousarray(s_red, dtype=np.uint8)
        return (red if red.size else np.zeros(1, np.uint8)), np.ascontiguousarray(s_off, dtype=np.uint64), np.ascontiguousarray(s_len, dtype=np.uint64)

    @classmethod
    def build(cls, handle: "Handle | None", s_red, s_off, s_len, alph: int, host_threads: int = 0):
        lib = load()
        red, off, ln = cls._seqs(s_red, s_off, s_len)
        h, out = (handle.h if handle is not None else None), C.c_void_p()
        rc = lib.lx_index_build(h, _ptr(red), _ptr(off), _ptr(ln), len(off), alph, host_threads, C.byref(out))
        if rc != LX_OK:
            _raise(lib, h, rc)
        return cls(out, handle)

    @classmethod
    def load(cls, handle: "Handle | None", data: bytes, s_red, s_off, s_len):
        lib = load()
        red, off, ln = cls._seqs(s_red, s_off, s_len)
        buf = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, np.uint8)
        h, out = (handle.h if handle is not None else None), C.c_void_p()
        rc = lib.lx_index_load(h, _ptr(buf), len(data), _ptr(red), _ptr(off), _ptr(ln), len(off), C.byref(out))
        if rc != LX_OK:
            _raise(lib, h, rc)
        return cls(out, handle)

    def attach(self, handle: "Handle | None"):
        """lx_index_attach: the same table for another handle (shares the host copy)."""
        h, out = (handle.h if handle is not None else None), C.c_void_p()
        rc = self.lib.lx_index_attach(self.ix, h, C.byref(out))
        if rc != LX_OK:
            _raise(self.lib, h, rc)
        return Index(out, handle)

    def save(self) -> bytes:
        out = C.c_void_p()
        rc = self.lib.lx_index_save(self.ix, C.byref(out))
        if rc != LX_OK:
            _raise(self.lib, None, rc)
        try:
            return C.string_at(self.lib.lx_bytes_data(out), self.lib.lx_bytes_size(out))
        finally:
            self.lib.lx_bytes_free(out)

    def info(self) -> IndexInfo:
        r = IndexInfo()
        if self.lib.lx_index_get_info(self.ix, C.byref(r)) != LX_OK:
            raise LambdaExtError(LX_EINVAL, "lx_index_get_info")
        return r

    def entries(self, first: int = 0, n: int | None = None) -> np.ndarray:
        n = int(self.info().n_entries) - first if n is None else n
        out = np.zeros(max(n, 1), dtype=INDEX_ENTRY_DTYPE)
        if self.lib.lx_index_copy_entries(self.ix, first, n, _ptr(out)) != LX_OK:
            raise LambdaExtError(LX_EINVAL, "lx_index_copy_entries: range outside the table")
        return out[:n]

    def close(self):
        if getattr(self, "ix", None):
            self.lib.lx_index_destroy(self.ix)
            self.ix = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def seed_params(matrix, seed_length=10, seed_offset=5, max_seed_dist=0, half_exact=True, adaptive=True, pre_scoring=2, pre_scoring_thresh=2.0,
                max_matches=256, q_num_frames=1, unknown_rank=25, matrix_rev=None, host_threads=0) -> SeedParams:
    """lx_seed_params; matrix / matrix_rev: LX_ALPH x LX_ALPH int8 arrays (kept alive by the returned object)."""
    p = SeedParams(seed_length, seed_offset, max_seed_dist, int(half_exact), int(adaptive), pre_scoring, pre_scoring_thresh, max_matches,
                   q_num_frames, unknown_rank, None, None, host_threads)
    p._keep = [None if m is None else np.ascontiguousarray(m, dtype=np.int8).reshape(LX_ALPH * LX_ALPH) for m in (matrix, matrix_rev)]
    p.matrix = None if p._keep[0] is None else p._keep[0].ctypes.data
    p.matrix_rev = None if p._keep[1] is None else p._keep[1].ctypes.data
    return p


class _DevList:
    """A device address with torch's data_ptr() spelling: what Handle.iterate_matches_dev* take."""

    def __init__(self, ptr):
        self.ptr = ptr

    def data_ptr(self):
        return self.ptr


class SeedResult:
    """lx_seed_result: stats, matches() (host copy, MATCH_DTYPE), dev() (the list in device memory; None for a host-path result).
    Free (close) results before their handle."""

    def __init__(self, r):
        self.lib, self.r = load(), r

    @property
    def stats(self) -> SeedStats:
        return self.lib.lx_seed_result_stats(self.r)

    def matches(self) -> np.ndarray:
        n = int(self.stats.n_matches)
        p = self.lib.lx_seed_result_matches(self.r)
        if not p:
            raise LambdaExtError(-3, "lx_seed_result_matches")
        return np.frombuffer(C.string_at(p, n * MATCH_DTYPE.itemsize), dtype=MATCH_DTYPE).copy() if n else np.zeros(0, MATCH_DTYPE)

    def dev(self):
        p = self.lib.lx_seed_result_matches_dev(self.r)
        return _DevList(p) if p else None

    def close(self):
        if getattr(self, "r", None):
            self.lib.lx_seed_result_free(self.r)
            self.r = None

    __del__ = close


def seg_tables(params: "SegParams | None" = None):
    """lx_seg_tables: (T, thr1, thr2) of the masking rule -- T[c] = round(c * log2 c * 65536), c = 0 .. 64, as int64."""
    lib, p = load(), params if params is not None else SegParams()
    T, t1, t2 = np.zeros(65, np.int64), C.c_int64(0), C.c_int64(0)
    rc = lib.lx_seg_tables(C.byref(p), _ptr(T), C.byref(t1), C.byref(t2))
    if rc != LX_OK:
        raise LambdaExtError(rc, last_output_error())
    return T, int(t1.value), int(t2.value)


class QueryMask:
    """lx_query_mask: which letters of a query set are masked.  seg(handle or None, q_res, q_off, q_len, params) applies the SEG rule
    (with a handle: by kernels, the mask stays on its device), dust(...) the nucleotide rule in the same way; from_bytes(handle or None, masked, q_off, q_len) takes given 0 / 1
    bytes indexed like q_res.  Close it before its handle."""

    def __init__(self, m, handle, extent):
        self.lib, self.m, self.handle, self.extent = load(), m, handle, extent

    @staticmethod
    def _table(q_off, q_len):
        off, ln = np.ascontiguousarray(q_off, dtype=np.uint64), np.ascontiguousarray(q_len, dtype=np.uint64)
        return off, ln, int((off + ln)[ln > 0].max()) if (ln > 0).any() else 0

    @classmethod
    def seg(cls, handle: "Handle | None", q_res, q_off, q_len, params: "SegParams | None" = None, host_threads: int = 0) -> "QueryMask":
        lib, out, p = load(), C.c_void_p(), params if params is not None else SegParams()
        res = np.ascontiguousarray(q_res, dtype=np.uint8)
        off, ln, extent = cls._table(q_off, q_len)
        h = handle.h if handle is not None else None
        rc = lib.lx_query_mask_create_seg(h, _ptr(res) if res.size else None, _ptr(off) if off.size else None, _ptr(ln) if ln.size else None, len(off),
                                          C.byref(p), host_threads, C.byref(out))
        if rc != LX_OK:
            raise LambdaExtError(rc, last_output_error())
        return cls(out, handle, extent)

    @classmethod
    def dust(cls, handle: "Handle | None", q_res, q_off, q_len, params: "DustParams | None" = None, host_threads: int = 0) -> "QueryMask":
        """the nucleotide rule, symmetric DUST, on alignment ranks A, C, G, T = 0 .. 3 (any other rank is a break)"""
        lib, out, p = load(), C.c_void_p(), params if params is not None else DustParams()
        res = np.ascontiguousarray(q_res, dtype=np.uint8)
        off, ln, extent = cls._table(q_off, q_len)
        h = handle.h if handle is not None else None
        rc = lib.lx_query_mask_create_dust(h, _ptr(res) if res.size else None, _ptr(off) if off.size else None, _ptr(ln) if ln.size else None, len(off),
                                           C.byref(p), host_threads, C.byref(out))
        if rc != LX_OK:
            raise LambdaExtError(rc, last_output_error())
        return cls(out, handle, extent)

    @classmethod
    def from_bytes(cls, handle: "Handle | None", masked, q_off, q_len) -> "QueryMask":
        lib, out = load(), C.c_void_p()
        msk = np.ascontiguousarray(masked, dtype=np.uint8)
        off, ln, extent = cls._table(q_off, q_len)
        if msk.size < extent:
            raise LambdaExtError(LX_EINVAL, "QueryMask.from_bytes: fewer mask bytes than letters")
        h = handle.h if handle is not None else None
        rc = lib.lx_query_mask_create(h, _ptr(msk) if msk.size else None, _ptr(off) if off.size else None, _ptr(ln) if ln.size else None, len(off),
                                      C.byref(out))
        if rc != LX_OK:
            raise LambdaExtError(rc, last_output_error())
        return cls(out, handle, extent)

    def info(self):
        """(letters, masked letters, sequences with a masked letter)"""
        a, b, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self.lib.lx_query_mask_info(self.m, C.byref(a), C.byref(b), C.byref(c))
        return int(a.value), int(b.value), int(c.value)

    def copy(self) -> np.ndarray:
        """0 / 1 per letter, indexed like q_res up to the last sequence's end"""
        out = np.zeros(max(self.extent, 1), np.uint8)
        if self.lib.lx_query_mask_copy(self.m, _ptr(out)) != LX_OK:
            raise LambdaExtError(LX_EINVAL, last_output_error())
        return out[:self.extent]

    def close(self):
        if getattr(self, "m", None):
            self.lib.lx_query_mask_destroy(self.m)
            self.m = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    __del__ = close


def seed_queries(handle: "Handle | None", index: Index, s_res, q_res, q_red, q_off, q_len, params: SeedParams, reads=None,
                 mask: "QueryMask | None" = None) -> SeedResult:
    """lx_seed_queries: search() for the reads whose first frame sequences are listed (None: all).  s_res None with a handle: the
    subjects lx_set_subjects made resident.  mask: lx_seed_queries_masked -- no seed starts on or covers a masked letter."""
    lib = load()
    keep = [None if a is None else np.ascontiguousarray(a, dtype=np.uint8) for a in (s_res, q_res, q_red)]
    keep = [a if a is None or a.size else np.zeros(1, np.uint8) for a in keep]
    off, ln = np.ascontiguousarray(q_off, dtype=np.uint64), np.ascontiguousarray(q_len, dtype=np.uint64)
    rd = None if reads is None else np.ascontiguousarray(reads, dtype=np.uint64)
    h, out = (handle.h if handle is not None else None), C.c_void_p()
    args = (h, index.ix, *[None if a is None else _ptr(a) for a in keep], _ptr(off), _ptr(ln), len(off), None if rd is None else _ptr(rd),
            0 if rd is None else len(rd))
    if mask is None:
        rc = lib.lx_seed_queries(*args, C.byref(params), C.byref(out))
    else:
        rc = lib.lx_seed_queries_masked(*args, mask.m, C.byref(params), C.byref(out))
    if rc != LX_OK:
        _raise(lib, h, rc)
    return SeedResult(out)


def taxonomy_build(nodes: bytes, names: bytes, present):
    """lx_taxonomy_build: the reference's thinned and flattened tree.  A dict: parents, heights (numpy), names (list of str; "" for
    taxa that are not kept), n_nodes, max_height, unnamed, warnings."""
    lib = load()
    pres = np.ascontiguousarray(present, dtype=np.uint32)
    t = C.c_void_p()
    rc = lib.lx_taxonomy_build(nodes, len(nodes), names, len(names), _ptr(pres) if len(pres) else None, len(pres), C.byref(t))
    if rc != LX_OK:
        raise LambdaExtError(rc, last_output_error())
    try:
        info = TaxonomyInfo()
        lib.lx_taxonomy_get(t, C.byref(info))
        n = int(info.n_taxa)
        par = np.ctypeslib.as_array(C.cast(info.parents, C.POINTER(C.c_uint32)), (n,)).copy()
        hgt = np.ctypeslib.as_array(C.cast(info.heights, C.POINTER(C.c_uint32)), (n,)).copy()
        nm = [info.names[i].decode() for i in range(n)]
        return {"parents": par, "heights": hgt, "names": nm, "n_nodes": int(info.n_nodes), "max_height": int(info.max_height),
                "unnamed": int(info.unnamed), "warnings": (info.warnings or b"").decode()}
    finally:
        lib.lx_taxonomy_free(t)


def write_records(path, fmt: int, bms: np.ndarray, ops: bytes, q_ids, q_lens, s_ids, s_lens, program="blastp",
                  write_header=True, q_ascii: bytes | None = None, q_ascii_off=None, options: OutputOptions | None = None, q_qual: bytes | None = None):
    m = np.ascontiguousarray(bms, dtype=BLAST_MATCH_DTYPE)
    qa = (C.c_char_p * len(q_ids))(*[x.encode() for x in q_ids])
    sa = (C.c_char_p * len(s_ids))(*[x.encode() for x in s_ids])
    ql = np.ascontiguousarray(q_lens, dtype=np.uint64)
    sl = np.ascontiguousarray(s_lens, dtype=np.uint64)
    names = SeqNames(qa, ql.ctypes.data, sa, sl.ctypes.data, len(q_ids), len(s_ids))
    o = np.frombuffer(ops + b"\0", dtype=np.uint8)
    qasc = np.frombuffer(q_ascii, dtype=np.uint8) if q_ascii else None
    qoff = np.ascontiguousarray(q_ascii_off, dtype=np.uint64) if q_ascii_off is not None else None
    options, _keep_qual = _with_qual(options, q_qual)
    rc = load().lx_write_records_ex(str(path).encode(), fmt, 1 if write_header else 0, program.encode(), _ptr(m), len(m), _ptr(o),
                                    C.byref(names), _ptr(qasc) if qasc is not None else None, _ptr(qoff) if qoff is not None else None,
                                    C.byref(options) if options is not None else None)
    if rc != LX_OK:
        raise LambdaExtError(rc, "lx_write_records: " + last_output_error())


class StepPlan(C.Structure):
    _fields_ = [("family", C.c_int32), ("group_lanes", C.c_int32), ("strip_cols", C.c_int32), ("panels", C.c_int32),
                ("compact_codes", C.c_int32), ("queries_per_wavefront", C.c_int32), ("may_decline", C.c_int32), ("adapted", C.c_int32),
                ("slot_bytes", C.c_uint64), ("lds_bytes", C.c_uint64), ("score_bound", C.c_uint64), ("name", C.c_char * 160)]


PLAN_NO_SWEEP, PLAN_HALF, PLAN_I16_COMPACT_WIDE, PLAN_I16_PAIRS, PLAN_INT32, PLAN_MQ = range(6)


def plan_step(scoring, max_qlen: int, max_slen: int, query_run: int, n: int, pass2_mode: int = 2, mq_sweep: int = 1, packed_half: int = 1,
              trace_bytes: int = 64 << 30, survivor_share: float = -1.0, adapt_permille: int = 30) -> StepPlan:
    """lx_plan_step: how lx_extend_batch_dev would run such a batch (no device needed)."""
    lib = load()
    lib.lx_plan_step.argtypes = [C.c_void_p] + [C.c_uint64] * 8 + [C.c_double, C.c_uint64, C.c_void_p]
    lib.lx_plan_step.restype = C.c_int
    out = StepPlan()
    rc = lib.lx_plan_step(C.byref(scoring), max_qlen, max_slen, query_run, n, pass2_mode, mq_sweep, packed_half, trace_bytes, survivor_share,
                          adapt_permille, C.byref(out))
    if rc != LX_OK:
        raise LambdaExtError(rc, "lx_plan_step")
    return out


def karlin_params(method: int, match: int = 2, mismatch: int = -3, gap_open: int = -11, gap_extend: int = -1) -> Karlin:
    ka = Karlin()
    rc = load().lx_karlin_params(method, match, mismatch, gap_open, gap_extend, C.byref(ka))
    if rc != LX_OK:
        raise LambdaExtError(rc, "no Karlin-Altschul values for this scoring scheme")
    return ka


def widen_and_preprocess(matches: np.ndarray, qlens: np.ndarray, slens: np.ndarray) -> np.ndarray:
    m = np.ascontiguousarray(matches, dtype=MATCH_DTYPE).copy()
    qlens = np.ascontiguousarray(qlens, dtype=np.uint64)
    slens = np.ascontiguousarray(slens, dtype=np.uint64)
    n = load().lx_widen_and_preprocess(_ptr(m), len(m), _ptr(qlens), _ptr(slens))
    return m[: int(n)]


LX_RANKS_AA27, LX_RANKS_DNA5_BS, LX_RANKS_SIMPLE = 0, 1, 2
LX_FRAMES_NONE, LX_FRAMES_REVCOMP, LX_FRAMES_TRANSLATED, LX_FRAMES_BISULFITE = 0, 1, 2, 3


def set_frames(q_mode: int, s_mode: int, qry_id: int, subj_id: int) -> tuple[int, int]:
    """_setFrames (src/search_algo.hpp:768-814): (qFrameShift, sFrameShift) of a frame-expanded id pair."""
    qf, sf = C.c_int32(), C.c_int32()
    load().lx_set_frames(q_mode, s_mode, qry_id, subj_id, C.byref(qf), C.byref(sf))
    return qf.value, sf.value


def translate_six_frames(dna5: np.ndarray, genetic_code: int = 1) -> list[np.ndarray]:
    """Six-frame translation of BioC++ dna5 ranks into SeqAn AminoAcid ranks, frames +1 +2 +3 -1 -2 -3."""
    src = np.ascontiguousarray(dna5, dtype=np.uint8)
    out = np.zeros(2 * src.size + 8, dtype=np.uint8)
    off, ln = np.zeros(6, dtype=np.uint64), np.zeros(6, dtype=np.uint64)
    rc = load().lx_translate_six_frames(_ptr(src), src.size, genetic_code, _ptr(out), out.size, _ptr(off), _ptr(ln))
    if rc != LX_OK:
        raise LambdaExtError(rc, "lx_translate_six_frames")
    return [out[int(o): int(o) + int(l)].copy() for o, l in zip(off, ln)]



def convert_ranks(kind: int, ranks: np.ndarray) -> np.ndarray:
    """BioC++ ranks -> the ranks the scoring tables use (src/seqan2_to_biocpp.hpp:352-395)."""
    src = np.ascontiguousarray(ranks, dtype=np.uint8)
    out = np.empty_like(src)
    rc = load().lx_convert_ranks(kind, _ptr(src), src.size, _ptr(out))
    if rc != LX_OK:
        raise LambdaExtError(rc, "lx_convert_ranks: unknown kind or rank outside the alphabet")
    return out


def builtin_scoring(method: int, match: int = 2, mismatch: int = -3, gap_open: int = -11, gap_extend: int = -1) -> Scoring:
    sc = Scoring()
    rc = load().lx_builtin_scoring(method, match, mismatch, gap_open, gap_extend, C.byref(sc))
    if rc != LX_OK:
        raise LambdaExtError(rc, "lx_builtin_scoring")
    return sc


def sort_words_dev(key0, key1, val0, val1, n: int, key_bits: int, device: int = 0, stream=None) -> int:
    """lx_sort_words_dev: the library's radix sort of n (key, value) uint64 pairs in device memory.  key0 / val0 hold the input, key1 /
    val1 are scratch of the same size: device pointers (integers, None for NULL) or objects with data_ptr().  key_bits is a bit mask:
    every 8-bit digit it touches is sorted by in full.  Returns sorted_in, the index of the buffer pair that holds the result."""
    def dptr(a):
        return a.data_ptr() if hasattr(a, "data_ptr") else a

    key = (C.c_void_p * 2)(dptr(key0), dptr(key1))
    val = (C.c_void_p * 2)(dptr(val0), dptr(val1))
    where = C.c_int(-1)
    rc = load().lx_sort_words_dev(device, key, val, n, key_bits & 0xFFFFFFFFFFFFFFFF, stream, C.byref(where))
    if rc != LX_OK:
        raise LambdaExtError(rc, "lx_sort_words_dev")
    return int(where.value)


def _sptr(a):
    return None if a is None else _ptr(a)


def _ssize(a) -> int:
    return 0 if a is None else int(a.size)


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


class Handle:
    """One lx_handle: one device, one HIP stream (the analogue of the reference's per-thread LocalDataHolder)."""

    def __init__(self, device: int = 0):
        self.lib = load()
        h = C.c_void_p()
        rc = self.lib.lx_create(device, C.byref(h))
        if rc != LX_OK:
            raise LambdaExtError(rc, self.lib.lx_last_error(None).decode())
        self.h = h
        self.device = device

    def close(self):
        if getattr(self, "h", None):
            self.lib.lx_destroy(self.h)
            self.h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc: int):
        if rc != LX_OK:
            raise LambdaExtError(rc, self.lib.lx_last_error(self.h).decode())

    def set_option(self, opt: int, value: int):
        self._check(self.lib.lx_set_option(self.h, opt, value))

    def set_band(self, band: int, centres=None, d_centres=None):
        """Band mode (LX_OPT_BAND): half width in diagonals (0 = off), optional per-extension centre diagonals for the next
        host-buffer call (numpy int32) / for the *_dev calls (torch int32 tensor on the device)."""
        self.set_option(LX_OPT_BAND, band)
        if centres is None:
            self._check(self.lib.lx_set_band_centres(self.h, None, 0))
        else:
            c = np.ascontiguousarray(centres, dtype=np.int32)
            self._check(self.lib.lx_set_band_centres(self.h, _ptr(c), len(c)))
        self._band_dev = d_centres  # keeps the tensor alive
        self._check(self.lib.lx_set_band_centres_dev(self.h, d_centres.data_ptr() if d_centres is not None else None))

    def get_option(self, opt: int) -> int:
        v = C.c_uint64()
        self._check(self.lib.lx_get_option(self.h, opt, C.byref(v)))
        return int(v.value)

    def set_scoring(self, sc: Scoring, slot: int = 0):
        self._check(self.lib.lx_set_scoring(self.h, slot, C.byref(sc)))

    # ---- host-buffer entry points -------------------------------------------------------------------
    def score_batch(self, q_res: np.ndarray, s_res: np.ndarray, ext: np.ndarray, slot: int = 0) -> np.ndarray:
        q_res = np.ascontiguousarray(q_res, dtype=np.uint8)
        s_res = None if s_res is None else np.ascontiguousarray(s_res, dtype=np.uint8)  # None: resident subjects
        ext = np.ascontiguousarray(ext, dtype=EXT_DTYPE)
        out = np.full(len(ext), -1, dtype=np.int32)
        self._check(self.lib.lx_score_batch(self.h, slot, _ptr(q_res), q_res.size, _sptr(s_res), _ssize(s_res), _ptr(ext),
                                            len(ext), _ptr(out)))
        return out

    def align_batch(self, q_res: np.ndarray, s_res: np.ndarray, ext: np.ndarray, slot: int = 0, known_score=None,
                    raw: bool = False):
        """lx_align_batch; known_score = the pass-1 scores of `ext` if the caller has them (saves the score pre-pass).
        raw=True returns (hsp, ops buffer, ops_off) without building the per-extension bytes objects."""
        q_res = np.ascontiguousarray(q_res, dtype=np.uint8)
        s_res = None if s_res is None else np.ascontiguousarray(s_res, dtype=np.uint8)  # None: resident subjects
        ext = np.ascontiguousarray(ext, dtype=EXT_DTYPE)
        n = len(ext)
        sizes = ext["q_len"].astype(np.uint64) + ext["s_len"].astype(np.uint64)
        ops_off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(sizes, out=ops_off[1:])
        hsp = np.zeros(n, dtype=HSP_DTYPE)
        ops = np.zeros(int(ops_off[-1]) + 1, dtype=np.uint8)
        ks = None if known_score is None else np.ascontiguousarray(known_score, dtype=np.int32)
        self._check(self.lib.lx_align_batch(self.h, slot, _ptr(q_res), q_res.size, _sptr(s_res), _ssize(s_res), _ptr(ext), n,
                                            None if ks is None else _ptr(ks), _ptr(hsp), _ptr(ops), _ptr(ops_off)))
        if raw:
            return hsp, ops, ops_off
        st = ops_off[:n].astype(np.int64) + hsp["ops_shift"].astype(np.int64)
        ops_list = [bytes(ops[int(st[i]):int(st[i]) + int(hsp["n_ops"][i])]) for i in range(n)]
        return hsp, ops_list

    def prefilter_batch(self, q_res, s_res, seeds, seed_length: int, pre_scoring: int, thresh: float, slot: int = 0):
        q_res = np.ascontiguousarray(q_res, dtype=np.uint8)
        s_res = None if s_res is None else np.ascontiguousarray(s_res, dtype=np.uint8)  # None: resident subjects
        seeds = np.ascontiguousarray(seeds, dtype=SEED_DTYPE)
        keep = np.zeros(len(seeds), dtype=np.uint8)
        self._check(self.lib.lx_prefilter_batch(self.h, slot, _ptr(q_res), q_res.size, _sptr(s_res), _ssize(s_res),
                                                _ptr(seeds), len(seeds), seed_length, pre_scoring, thresh, _ptr(keep)))
        return keep

    def extend_batch_rle(self, q_res, s_res, ext, min_score, slot: int = 0):
        """lx_extend_batch_rle: as extend_batch, the ops as run-length codes ((op << 6) | (len - 1), op 0/1/2 = M/D/I)."""
        return self.extend_batch(q_res, s_res, ext, min_score, slot=slot, rle=True)

    @staticmethod
    def expand_ops(codes: np.ndarray, n_ops: int) -> bytes:
        out = np.zeros(max(n_ops, 1), dtype=np.uint8)
        c = np.ascontiguousarray(codes, dtype=np.uint8)
        rc = load().lx_expand_ops(_ptr(c), n_ops, _ptr(out))
        if rc != LX_OK:
            raise LambdaExtError(rc, "lx_expand_ops")
        return bytes(out[:n_ops])

    def extend_batch(self, q_res, s_res, ext, min_score, slot: int = 0, copy_ops: bool = True, rle: bool = False, out=None):
        """lx_extend_batch: both passes on host buffers.  min_score = int cut-off for all, or an int32 array per
        extension.  Returns (scores, hsp, ops_off, ops) -- ops is a copy of the handle-owned buffer (copy_ops=False: a
        view that the next call invalidates)."""
        q_res = np.ascontiguousarray(q_res, dtype=np.uint8)
        s_res = None if s_res is None else np.ascontiguousarray(s_res, dtype=np.uint8)
        ext = np.ascontiguousarray(ext, dtype=EXT_DTYPE)
        n = len(ext)
        per = None if np.isscalar(min_score) else np.ascontiguousarray(min_score, dtype=np.int32)
        # out = (score, hsp, off) arrays of an earlier call to write into (a caller that keeps its buffers pays no page faults)
        score, hsp, off = out if out is not None else (np.zeros(n, dtype=np.int32), np.zeros(n, dtype=HSP_DTYPE), np.zeros(n, dtype=np.uint64))
        p, nb = C.c_void_p(), C.c_uint64()
        fn = self.lib.lx_extend_batch_rle if rle else self.lib.lx_extend_batch
        self._check(fn(self.h, slot, _ptr(q_res), q_res.size, _sptr(s_res), _ssize(s_res), _ptr(ext), n,
                                             None if per is None else _ptr(per), 0 if per is not None else int(min_score),
                                             _ptr(score), _ptr(hsp), _ptr(off), C.byref(p), C.byref(nb)))
        if not nb.value:
            return score, hsp, off, np.zeros(1, np.uint8)
        ops = np.ctypeslib.as_array((C.c_uint8 * int(nb.value)).from_address(p.value))
        return score, hsp, off, ops.copy() if copy_ops else ops

    def extend_batch_list(self, q_res, s_res, ext, min_score, slot: int = 0, copy: bool = True, out_score=None):
        """lx_extend_batch_list: the scores of every extension and the survivors of the filter as a list.  Returns
        (scores, index, hsp, codes_off, codes): `index[k]` is survivor k's position in `ext`; copy=False gives views of the
        handle's buffers that the next extend_batch* call invalidates."""
        q_res = np.ascontiguousarray(q_res, dtype=np.uint8)
        s_res = None if s_res is None else np.ascontiguousarray(s_res, dtype=np.uint8)
        ext = np.ascontiguousarray(ext, dtype=EXT_DTYPE)
        n = len(ext)
        per = None if np.isscalar(min_score) else np.ascontiguousarray(min_score, dtype=np.int32)
        score = out_score if out_score is not None else np.zeros(n, dtype=np.int32)
        sl = SurvivorList()
        self._check(self.lib.lx_extend_batch_list(self.h, slot, _ptr(q_res), q_res.size, _sptr(s_res), _ssize(s_res), _ptr(ext), n,
                                                  None if per is None else _ptr(per), 0 if per is not None else int(min_score),
                                                  _ptr(score), C.byref(sl)))
        k = int(sl.count)
        if not k:
            return score, np.zeros(0, np.uint32), np.zeros(0, HSP_DTYPE), np.zeros(0, np.uint64), np.zeros(1, np.uint8)
        view = lambda ptr, dtype, count: np.frombuffer((C.c_uint8 * (count * np.dtype(dtype).itemsize)).from_address(ptr), dtype=dtype, count=count)
        index, hsp, off = view(sl.index, np.uint32, k), view(sl.hsp, HSP_DTYPE, k), view(sl.codes_off, np.uint64, k)
        codes = view(sl.codes, np.uint8, max(int(sl.codes_bytes), 1))
        if copy:
            index, hsp, off, codes = index.copy(), hsp.copy(), off.copy(), codes.copy()
        return score, index, hsp, off, codes

    def last_extend_stats(self):
        """(extensions, slots, cells, executed cells) of the last extend_batch call."""
        out = np.zeros(4, dtype=np.uint64)
        self._check(self.lib.lx_last_extend_stats(self.h, _ptr(out)))
        return tuple(int(x) for x in out)

    def set_subjects(self, s_res):
        """lx_set_subjects: keep the subject residues on the device; later host-buffer calls may pass s_res=None."""
        if s_res is None:
            self._check(self.lib.lx_set_subjects(self.h, None, 0))
            return
        s_res = np.ascontiguousarray(s_res, dtype=np.uint8)
        self._check(self.lib.lx_set_subjects(self.h, _sptr(s_res), _ssize(s_res)))

    # ---- device-resident entry points (torch tensors on this handle's device) --------------------------
    def score_batch_dev(self, d_q, d_s, d_ext, n: int, d_out, stream=None, slot: int = 0):
        self._check(self.lib.lx_score_batch_dev(self.h, slot, d_q.data_ptr(), d_s.data_ptr(), d_ext.data_ptr(), n,
                                                d_out.data_ptr(), stream))

    def align_batch_dev(self, d_q, d_s, d_ext, n: int, d_hsp, d_ops, d_ops_off, stream=None, slot: int = 0):
        self._check(self.lib.lx_align_batch_dev(self.h, slot, d_q.data_ptr(), d_s.data_ptr(), d_ext.data_ptr(), n,
                                                d_hsp.data_ptr(), d_ops.data_ptr(), d_ops_off.data_ptr(), stream))

    def iterate_matches(self, q_res, q_off, q_len, q_orig_len, s_res, s_off, s_len, matches, params: "SearchParams",
                        slot: int = 0):
        """iterateMatchesFullSimd: returns (blast_matches ndarray, list of ops bytes, IterateStats)."""
        q_res = np.ascontiguousarray(q_res, dtype=np.uint8)
        s_res = None if s_res is None else np.ascontiguousarray(s_res, dtype=np.uint8)  # None: resident subjects
        q_off = np.ascontiguousarray(q_off, dtype=np.uint64)
        q_len = np.ascontiguousarray(q_len, dtype=np.uint64)
        s_off = np.ascontiguousarray(s_off, dtype=np.uint64)
        s_len = np.ascontiguousarray(s_len, dtype=np.uint64)
        q_orig = np.ascontiguousarray(q_orig_len, dtype=np.uint64)
        m = np.ascontiguousarray(matches, dtype=MATCH_DTYPE).copy()
        res = C.c_void_p()
        self._check(self.lib.lx_iterate_matches(self.h, slot, _ptr(q_res), q_res.size, _ptr(q_off), _ptr(q_len), len(q_off),
                                                _ptr(q_orig), _sptr(s_res), _ssize(s_res), _ptr(s_off), _ptr(s_len),
                                                len(s_off), _ptr(m), len(m), C.byref(params), C.byref(res)))
        return self._take_iterate_result(res)

    def set_queries(self, q_res, q_off, q_len, q_orig_len=None, qry_num_frames: int = 1):
        """lx_set_queries: the (frame-expanded) query set becomes resident on the device (for iterate_matches_dev)."""
        q_res = np.ascontiguousarray(q_res, dtype=np.uint8)
        q_off = np.ascontiguousarray(q_off, dtype=np.uint64)
        q_len = np.ascontiguousarray(q_len, dtype=np.uint64)
        q_orig = None if q_orig_len is None else np.ascontiguousarray(q_orig_len, dtype=np.uint64)
        self._check(self.lib.lx_set_queries(self.h, _ptr(q_res), q_res.size, _ptr(q_off), _ptr(q_len), len(q_off),
                                            None if q_orig is None else _ptr(q_orig), qry_num_frames))

    def set_subject_seqs(self, s_off, s_len):
        s_off = np.ascontiguousarray(s_off, dtype=np.uint64)
        s_len = np.ascontiguousarray(s_len, dtype=np.uint64)
        self._check(self.lib.lx_set_subject_seqs(self.h, _ptr(s_off), _ptr(s_len), len(s_off)))

    def reserve(self, n_matches: int, n_windows: int, n_hsps: int, n_columns: int = 0):
        """lx_reserve: what the first iterate_matches_dev call would allocate inside the call, ahead of it."""
        self._check(self.lib.lx_reserve(self.h, n_matches, n_windows, n_hsps, n_columns))

    def iterate_matches_dev(self, d_matches, n: int, params: "SearchParams", slot: int = 0):
        """lx_iterate_matches_dev on a device tensor holding n lx_match records (48 bytes each); results as iterate_matches."""
        res = C.c_void_p()
        self._check(self.lib.lx_iterate_matches_dev(self.h, slot, d_matches.data_ptr() if n else None, n, C.byref(params), C.byref(res)))
        return self._take_iterate_result(res)

    def iterate_matches_dev_top(self, d_matches, n: int, params: "SearchParams", max_matches: int = 25, slot: int = 0):
        """lx_iterate_matches_dev_top: iterate_matches_dev with _writeRecord's sort / dedupe / top-N on the device before the result
        comes down; (records, ops, stats, record stats)."""
        res = C.c_void_p()
        rst = RecordStats()
        self._check(self.lib.lx_iterate_matches_dev_top(self.h, slot, d_matches.data_ptr() if n else None, n, C.byref(params), max_matches, C.byref(rst), C.byref(res)))
        return (*self._take_iterate_result(res), rst)

    def iterate_matches_dev_top_ex(self, d_matches, n: int, params: "SearchParams", max_matches: int = 25, max_hsps: int = 0, culling_limit: int = 0, slot: int = 0):
        """lx_iterate_matches_dev_top_ex: iterate_matches_dev_top with --max-hsps / --culling-limit (the lengths are the resident
        q_orig_len of set_queries); (records, ops, stats, record stats, cull stats)."""
        res = C.c_void_p()
        rst, cst = RecordStats(), CullStats()
        opt, _ = cull_options(max_hsps, culling_limit)
        self._check(self.lib.lx_iterate_matches_dev_top_ex(self.h, slot, d_matches.data_ptr() if n else None, n, C.byref(params), max_matches, C.byref(opt),
                                                           C.byref(rst), C.byref(cst), C.byref(res)))
        return (*self._take_iterate_result(res), rst, cst)

    def plan_free_packing_dev(self, d_ext, n: int, n_qseq: int, strip_cols: int = 19, cuts=None):
        """lx_plan_free_packing_dev: (plan [nwf, 16], wf_pan [nwf], wf_maxs [nwf], report [16]) for n lx_extension records in a device tensor."""
        cuts = np.ascontiguousarray([0, n] if cuts is None else cuts, dtype=np.uint64)
        nranges = len(cuts) - 1
        cap = int(self.lib.lx_plan_free_packing_bound(n, n_qseq, nranges))
        plan, pan, maxs, rep = np.zeros(cap * 16, np.uint32), np.zeros(cap, np.uint32), np.zeros(cap, np.uint32), np.zeros(16, np.uint32)
        self._check(self.lib.lx_plan_free_packing_dev(self.h, d_ext.data_ptr(), n, n_qseq, strip_cols, nranges, cuts.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                      _ptr(plan), _ptr(pan), _ptr(maxs), _ptr(rep)))
        nwf = int(rep[0])
        assert nwf <= cap, (nwf, cap)
        return plan[:nwf * 16].reshape(nwf, 16).copy(), pan[:nwf].copy(), maxs[:nwf].copy(), rep

    def widen_and_preprocess_dev(self, d_matches, n: int, bisulfite: bool = False):
        """lx_widen_and_preprocess_dev: the window list of a device match list (n lx_match records) as a MATCH_DTYPE array."""
        out = np.zeros(max(n, 1), dtype=MATCH_DTYPE)
        cnt = C.c_uint64(0)
        self._check(self.lib.lx_widen_and_preprocess_dev(self.h, d_matches.data_ptr() if n else None, n, 1 if bisulfite else 0, _ptr(out), C.byref(cnt)))
        return out[:cnt.value].copy()

    def _take_iterate_result(self, res):
        try:
            n = int(self.lib.lx_iterate_result_count(res))
            stats = self.lib.lx_iterate_result_stats(res)
            if n == 0:
                return np.zeros(0, dtype=BLAST_MATCH_DTYPE), [], stats
            buf = (C.c_char * (n * BLAST_MATCH_DTYPE.itemsize)).from_address(self.lib.lx_iterate_result_matches(res))
            bms = np.frombuffer(buf, dtype=BLAST_MATCH_DTYPE).copy()
            total = int((bms["ops_off"].astype(np.uint64) + bms["n_ops"].astype(np.uint64)).max())  # (not the last record's: bisulfite runs two passes)
            if not self.lib.lx_iterate_result_ops(res):  # LX_ITERATE_NO_OPS
                return bms, [], stats
            obuf = (C.c_char * max(total, 1)).from_address(self.lib.lx_iterate_result_ops(res))
            allops = bytes(obuf)
            ops = [allops[o:o + k] for o, k in zip(bms["ops_off"].tolist(), bms["n_ops"].tolist())]  # (record scalars one by one cost 0.7 ms per thousand)
            return bms, ops, stats
        finally:
            self.lib.lx_iterate_result_free(res)

    def extend_batch_dev(self, d_q, d_s, d_ext, n: int, min_score: int, d_score, d_hsp, d_ops, d_ops_off, d_count,
                         d_min_score=None, stream=None, slot: int = 0):
        self._check(self.lib.lx_extend_batch_dev(self.h, slot, d_q.data_ptr(), d_s.data_ptr(), d_ext.data_ptr(), n,
                                                 d_min_score.data_ptr() if d_min_score is not None else None, min_score,
                                                 d_score.data_ptr(), d_hsp.data_ptr(), d_ops.data_ptr(),
                                                 d_ops_off.data_ptr(), d_count.data_ptr(), stream))

    def synchronize(self):
        self._check(self.lib.lx_synchronize(self.h))

    def bgzf_compress(self, data: bytes, eof: bool = False) -> bytes:
        """lx_bgzf_compress: BGZF members of `data` made on this handle's device (+ the EOF member if asked)."""
        buf = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, np.uint8)
        out = np.empty(bgzf_bound(len(data)), dtype=np.uint8)
        got = C.c_uint64(0)
        self._check(self.lib.lx_bgzf_compress(self.h, _ptr(buf), len(data), _ptr(out), len(out), C.byref(got), LX_BGZF_EOF if eof else 0))
        return out[: got.value].tobytes()

    def write_records_bgzf(self, path, fmt: int, bms: np.ndarray, ops: bytes, q_ids, q_lens, s_ids, s_lens, program="blastp",
                           q_ascii: bytes | None = None, q_ascii_off=None, options: OutputOptions | None = None, footer_records: int = -1, q_qual: bytes | None = None):
        """lx_write_records_bgzf: header, records and footer (footer_records >= 0) of `fmt`, BGZF-compressed into `path`."""
        args, keep = _writer_args(bms, ops, q_ids, q_lens, s_ids, s_lens, q_ascii, q_ascii_off, options, q_qual)
        self._check(self.lib.lx_write_records_bgzf(self.h, str(path).encode(), fmt, program.encode(), *args, footer_records))

    def render_bam(self, bms: np.ndarray, ops: bytes, q_ids, q_lens, s_ids, s_lens, program="blastp", write_header=True,
                   q_ascii: bytes | None = None, q_ascii_off=None, options: OutputOptions | None = None, q_qual: bytes | None = None) -> bytes:
        """lx_render_bam_dev: render_records(LX_OUT_BAM, ...) with the records made by kernels on this handle's device; the same bytes."""
        args, keep = _writer_args(bms, ops, q_ids, q_lens, s_ids, s_lens, q_ascii, q_ascii_off, options, q_qual)
        out = C.c_void_p()
        rc = self.lib.lx_render_bam_dev(self.h, 1 if write_header else 0, program.encode(), *args[:3], len(ops), *args[3:], C.byref(out))
        self._check(rc)
        try:
            return C.string_at(self.lib.lx_bytes_data(out), self.lib.lx_bytes_size(out)) if self.lib.lx_bytes_size(out) else b""
        finally:
            self.lib.lx_bytes_free(out)

    def write_bam(self, path, bms: np.ndarray, ops: bytes, q_ids, q_lens, s_ids, s_lens, program="blastp",
                  q_ascii: bytes | None = None, q_ascii_off=None, options: OutputOptions | None = None, q_qual: bytes | None = None):
        """lx_write_bam_dev: write_records_bgzf(path, LX_OUT_BAM, ...) with the records rendered and compressed on the device; the same file."""
        args, keep = _writer_args(bms, ops, q_ids, q_lens, s_ids, s_lens, q_ascii, q_ascii_off, options, q_qual)
        self._check(self.lib.lx_write_bam_dev(self.h, str(path).encode(), program.encode(), *args[:3], len(ops), *args[3:]))

    def render_text(self, fmt: int, bms: np.ndarray, ops: bytes, q_ids, q_lens, s_ids, s_lens, program="blastp", write_header=True,
                    q_ascii: bytes | None = None, q_ascii_off=None, options: OutputOptions | None = None, footer_records: int = -1, q_qual: bytes | None = None) -> bytes:
        """lx_render_text_dev: render_records(fmt, ...) for LX_OUT_BLAST_TAB, LX_OUT_BLAST_TAB_COMMENTS and LX_OUT_SAM with the records made
        by kernels on this handle's device; the same bytes."""
        args, keep = _writer_args(bms, ops, q_ids, q_lens, s_ids, s_lens, q_ascii, q_ascii_off, options, q_qual)
        out = C.c_void_p()
        rc = self.lib.lx_render_text_dev(self.h, fmt, 1 if write_header else 0, program.encode(), *args[:3], len(ops), *args[3:], footer_records,
                                         C.byref(out))
        self._check(rc)
        try:
            return C.string_at(self.lib.lx_bytes_data(out), self.lib.lx_bytes_size(out)) if self.lib.lx_bytes_size(out) else b""
        finally:
            self.lib.lx_bytes_free(out)

    def write_text(self, path, fmt: int, bms: np.ndarray, ops: bytes, q_ids, q_lens, s_ids, s_lens, program="blastp", bgzf=False,
                   q_ascii: bytes | None = None, q_ascii_off=None, options: OutputOptions | None = None, footer_records: int = -1, q_qual: bytes | None = None):
        """lx_write_text_dev: the file write_records + write_footer (bgzf False) or write_records_bgzf (bgzf True) write for a text format,
        with the records rendered (and compressed) on the device; the same file."""
        args, keep = _writer_args(bms, ops, q_ids, q_lens, s_ids, s_lens, q_ascii, q_ascii_off, options, q_qual)
        self._check(self.lib.lx_write_text_dev(self.h, str(path).encode(), fmt, 1 if bgzf else 0, program.encode(), *args[:3], len(ops), *args[3:],
                                               footer_records))

    def last_gunzip_stats(self) -> GunzipStats:
        """lx_last_gunzip_stats: the counts of the last gunzip(handle, ...), of the last piece of gunzip_stream(handle, ...), or, once
        that stream has ended, of its whole file;
        .decline_text is the last decline reason in words."""
        st = GunzipStats()
        self._check(self.lib.lx_last_gunzip_stats(self.h, C.byref(st)))
        st.decline_text = self.lib.lx_gunzip_decline_text(st.last_decline).decode()
        return st

    def last_kernel_name(self) -> str:
        return self.lib.lx_last_kernel_name(self.h).decode()

    def last_trace_kernel_name(self) -> str:
        return self.lib.lx_last_trace_kernel_name(self.h).decode()

    def compute_lca_dev(self, tax_dev: "TaxDev", bms: np.ndarray, top_percent: float = 100.0):
        """lx_compute_lca_dev: compute_lca_ex with the fold as kernels on this handle's device, over `tax_dev`'s resident tree."""
        m = np.ascontiguousarray(bms, dtype=BLAST_MATCH_DTYPE)
        qid = np.zeros(max(len(m), 1), dtype=np.uint64)
        lca = np.zeros(max(len(m), 1), dtype=np.uint32)
        cnt = C.c_uint64(0)
        opt = lca_options(top_percent)
        self._check(self.lib.lx_compute_lca_dev(self.h, tax_dev.t if tax_dev is not None else None, _ptr(m) if len(m) else None, len(m),
                                                C.byref(opt), _ptr(qid), _ptr(lca), C.byref(cnt)))
        return qid[: cnt.value].copy(), lca[: cnt.value].copy()

    def last_phase_ms(self, phase: int):
        ms, cnt = C.c_float(), C.c_int()
        self._check(self.lib.lx_last_phase_ms(self.h, phase, C.byref(ms), C.byref(cnt)))
        return float(ms.value), int(cnt.value)

    def last_kernel_ms(self) -> float:
        ms = C.c_float()
        self._check(self.lib.lx_last_kernel_ms(self.h, C.byref(ms)))
        return float(ms.value)
