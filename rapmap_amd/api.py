"""Host-side mirror of the reference's call surface, over the C ABI of libqmap_mi355.so.

The reference exposes three C++ entry points to its callers:
``SACollector::operator()`` (include/SACollector.hpp:108), ``hitsToMappingsSimple``
(include/HitManager.hpp:130-135) and ``mergeLeftRightHits`` (include/RapMapUtils.hpp:1185),
driven per read pair by ``processReadsPairSA`` (src/RapMapSAMapper.cpp:376).  Here the same
three steps run batched on the GPU behind ``QuasiMapper.map_pairs``; the index object mirrors
``RapMapSAIndex`` (include/RapMapSAIndex.hpp:70-82).

There is NO CPU fallback: if the HIP library is missing or no GPU is visible the calls raise.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("QM_LIB_OVERRIDE") or os.path.join(_HERE, "libqmap_mi355.so")   # override: profiling variants only

HIT_DTYPE = np.dtype([
    ("tid", "<u4"), ("pos", "<i4"), ("mate_pos", "<i4"), ("frag_len", "<u4"),
    ("read_len", "<u4"), ("mate_len", "<u4"),
    ("fwd", "u1"), ("mate_is_fwd", "u1"), ("is_paired", "u1"), ("mate_status", "u1"),
    ("aln_score", "<i4"),
])
INTERVAL_DTYPE = np.dtype([("begin", "<i4"), ("end", "<i4"), ("len", "<u4"), ("query_pos", "<u4"),
                           ("query_rc", "u1"), ("list", "u1"), ("pad", "<u2")])
assert HIT_DTYPE.itemsize == 32 and INTERVAL_DTYPE.itemsize == 20

# every symbol include/qmap_mi355.h declares
ABI_SYMBOLS = [
    "qm_last_error", "qm_version", "qm_opts_default", "qm_index_open", "qm_index_close", "qm_index_info_get",
    "qm_index_txp_name", "qm_index_txp_len", "qm_index_arrays", "qm_index_raw", "qm_ctx_create", "qm_ctx_destroy", "qm_ctx_device_bytes",
    "qm_map_pairs", "qm_map_reads", "qm_map_device", "qm_pack_reads", "qm_packed_offset", "qm_packed_bytes", "qm_map_pairs_packed", "qm_map_reads_packed", "qm_fetch_hits", "qm_result_device", "qm_ctx_set_debug",
    "qm_fetch_intervals", "qm_last_kernel_ms", "qm_ctx_stat", "qm_fetch_skipped", "qm_build_index", "qm_build_index_ex",
    "qm_collect_reads", "qm_fetch_found", "qm_hits_to_mappings", "qm_fetch_read_lists", "qm_merge_lists", "qm_fetch_too_many",
    "qm_map_pairs_stages", "qm_map_pairs_stages_ex", "qm_map_pairs_stages_packed", "qm_stage_bytes", "qm_fetch_stages", "qm_pinned_alloc", "qm_pinned_free", "qm_ctx_create_ex", "qm_fetch_hits_pinned", "qm_xxh64",
    "qm_stream_open", "qm_stream_open_ex", "qm_stream_reserve", "qm_stream_next", "qm_stream_close", "qm_stream_last_error", "qm_stream_stats", "qm_stream_stats_ex",
    "qm_reader_open", "qm_reader_next", "qm_reader_close", "qm_io_last_error", "qm_sam_header", "qm_sam_records",
    "qm_eqc_create", "qm_eqc_destroy", "qm_eqc_clear", "qm_eqc_add", "qm_eqc_add_labels", "qm_eqc_size", "qm_eqc_fetch", "qm_eqc_stat",
    "qm_stream_eqc_finish", "qm_stream_eqc_fetch",
    "qm_quant_create", "qm_quant_set_start", "qm_quant_set_method", "qm_quant_exp_digamma", "qm_quant_run", "qm_quant_fetch", "qm_quant_stat", "qm_quant_destroy",
    "qm_quant_fetch_classes", "qm_boot_create", "qm_boot_resample", "qm_boot_set_counts", "qm_boot_fetch_counts", "qm_boot_run", "qm_boot_fetch",
    "qm_boot_stat", "qm_boot_destroy",
    "qm_fld_create", "qm_fld_destroy", "qm_fld_clear", "qm_fld_add", "qm_fld_add_hits", "qm_fld_add_counts", "qm_fld_fetch", "qm_fld_stat",
    "qm_fld_eff_lens_from_counts", "qm_fld_eff_lens", "qm_stream_fld_fetch",
    "qm_gcb_create", "qm_gcb_destroy", "qm_gcb_clear", "qm_gcb_add", "qm_gcb_add_hits", "qm_gcb_add_counts", "qm_gcb_fetch", "qm_gcb_stat",
    "qm_gcb_expect", "qm_gcb_eff_lens_from_counts", "qm_gcb_window_gc", "qm_stream_gcb_fetch",
    "qm_sqb_create", "qm_sqb_destroy", "qm_sqb_clear", "qm_sqb_add", "qm_sqb_add_hits", "qm_sqb_add_counts", "qm_sqb_fetch", "qm_sqb_stat",
    "qm_sqb_expect", "qm_sqb_eff_lens", "qm_sqb_context", "qm_sqb_weights", "qm_sqb_ratios", "qm_stream_sqb_fetch",
    "qm_psb_create", "qm_psb_destroy", "qm_psb_clear", "qm_psb_add", "qm_psb_add_hits", "qm_psb_add_counts", "qm_psb_fetch", "qm_psb_stat",
    "qm_psb_expect", "qm_psb_eff_lens", "qm_psb_position", "qm_psb_ratios", "qm_stream_psb_fetch",
    "qm_lib_create", "qm_lib_destroy", "qm_lib_clear", "qm_lib_add", "qm_lib_add_hits", "qm_lib_compact_hits", "qm_lib_add_counts", "qm_lib_fetch",
    "qm_lib_stat", "qm_eqc_add_lib", "qm_lib_type_mask", "qm_lib_infer", "qm_stream_lib_fetch",
    "qm_sam_write", "qm_sam_writer_open", "qm_sam_writer_open_ex", "qm_sam_writer_header", "qm_sam_writer_put", "qm_sam_writer_close", "qm_buf_free",
]

# the `which` of QuasiMapper.stat (qm_ctx_stat) and of EqClasses.stat (qm_eqc_stat): the two enums of include/qmap_mi355.h, which says what each counts
(QM_STAT_RELAUNCHES, QM_STAT_LIST_WORDS, QM_STAT_SLOW_READS, QM_STAT_LEAN_READS, QM_STAT_LEAN_DEFERRED, QM_STAT_SKIPPED_READS,
 QM_STAT_SEL_QUESTIONS, QM_STAT_KSW2_ALIGNMENTS, QM_STAT_STRIP_ALIGNMENTS, QM_STAT_PAIR_KERNEL_PAIRS, QM_STAT_PAIRS_MERGED,
 QM_STAT_DEFER_DIRTY, QM_STAT_DEFER_HOMOPOLYMER, QM_STAT_DEFER_WIDE, QM_STAT_DEFER_BOTH_STRANDS, QM_STAT_N_PASS_READS) = range(16)
QM_EQC_STAT_GROWTHS, QM_EQC_STAT_COLLISION_PROBES, QM_EQC_STAT_LONG_UNITS, QM_EQC_STAT_ROUNDS, QM_EQC_STAT_LAST_FOLD_US = range(5)


class QmError(RuntimeError):
    pass


class QmOpts(C.Structure):
    """MappingOpts (src/RapMapSAMapper.cpp:114-152), hot-path fields only."""
    _fields_ = [("sensitive", C.c_int32), ("strict_check", C.c_int32), ("max_num_hits", C.c_int32),
                ("no_orphans", C.c_int32), ("no_dovetail", C.c_int32), ("fuzzy", C.c_int32),
                ("max_interval", C.c_int32), ("sel_aln", C.c_int32), ("quasi_cov", C.c_double),
                ("hard_filter", C.c_int32), ("match_score", C.c_int32), ("mismatch_penalty", C.c_int32), ("gap_open", C.c_int32),
                ("gap_extend", C.c_int32), ("dp_bandwidth", C.c_int32), ("max_mmp_extension", C.c_int32), ("aln_policy", C.c_int32),
                ("min_score_fraction", C.c_double), ("consensus_slack", C.c_double)]


class QmCounters(C.Structure):
    """HitCounters (include/RapMapUtils.hpp:208-216)."""
    _fields_ = [("pe_hits", C.c_uint64), ("se_hits", C.c_uint64), ("tot_hits", C.c_uint64),
                ("num_reads", C.c_uint64), ("too_many_hits", C.c_uint64), ("mapped", C.c_uint64)]

    def as_dict(self):
        return {"peHits": self.pe_hits, "seHits": self.se_hits, "totHits": self.tot_hits,
                "numReads": self.num_reads, "tooManyHits": self.too_many_hits, "mappedUnits": self.mapped}


class QmHitRaw(C.Structure):
    _fields_ = [("b", C.c_uint8 * 32)]


class QmStreamBatch(C.Structure):
    """qm_stream_batch (include/qmap_mi355.h): pointers into the stream's pinned buffers"""
    _fields_ = [("n_units", C.c_int64),
                ("seq1", C.c_void_p), ("off1", C.c_void_p), ("names1", C.c_void_p), ("name_off1", C.c_void_p),
                ("seq2", C.c_void_p), ("off2", C.c_void_p), ("names2", C.c_void_p), ("name_off2", C.c_void_p),
                ("hit_offsets", C.c_void_p), ("hits", C.c_void_p), ("n_hits", C.c_int64),
                ("counters", QmCounters), ("gpu_ms", C.c_double), ("device", C.c_int32), ("pad", C.c_int32)]


class QmStageView(C.Structure):
    _fields_ = [("n_units", C.c_int64), ("n_reads", C.c_int64), ("iv_off", C.c_void_p), ("iv", C.c_void_p), ("found", C.c_void_p),
                ("list_off", C.c_void_p), ("words", C.c_void_p), ("hit_off", C.c_void_p), ("hits", C.c_void_p), ("too_many", C.c_void_p)]


class QmIndexInfo(C.Structure):
    _fields_ = [("k", C.c_int32), ("big_sa", C.c_int32), ("perfect_hash", C.c_int32), ("pad", C.c_int32),
                ("text_len", C.c_int64), ("n_txps", C.c_int64), ("n_keys", C.c_int64)]


_lib = None


def lib():
    """Load libqmap_mi355.so; fails loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise QmError("HIP library %s is missing - run `python -c 'import __graft_entry__ as g; g.build()'` "
                      "(there is no CPU fallback)" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    L.qm_last_error.restype = C.c_char_p
    L.qm_version.restype = C.c_char_p
    L.qm_index_open.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
    L.qm_index_close.argtypes = [C.c_void_p]
    L.qm_index_info_get.argtypes = [C.c_void_p, C.POINTER(QmIndexInfo)]
    L.qm_index_txp_name.restype = C.c_char_p
    L.qm_index_txp_name.argtypes = [C.c_void_p, C.c_int64]
    L.qm_index_txp_len.restype = C.c_int64
    L.qm_index_txp_len.argtypes = [C.c_void_p, C.c_int64]
    L.qm_index_arrays.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_void_p),
                                  C.POINTER(C.c_int64)]
    L.qm_ctx_create.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
    L.qm_ctx_create_ex.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.POINTER(C.c_void_p)]
    L.qm_ctx_destroy.argtypes = [C.c_void_p]
    L.qm_ctx_device_bytes.restype = C.c_int64
    L.qm_ctx_device_bytes.argtypes = [C.c_void_p]
    L.qm_map_pairs.argtypes = [C.c_void_p, C.POINTER(QmOpts), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.POINTER(C.c_int64), C.POINTER(QmCounters)]
    L.qm_map_reads.argtypes = [C.c_void_p, C.POINTER(QmOpts), C.c_int64, C.c_void_p, C.c_void_p,
                               C.POINTER(C.c_int64), C.POINTER(QmCounters)]
    L.qm_map_device.argtypes = [C.c_void_p, C.POINTER(QmOpts), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.POINTER(QmCounters)]
    L.qm_fetch_hits.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.qm_result_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.qm_ctx_set_debug.argtypes = [C.c_void_p, C.c_int]
    L.qm_fetch_intervals.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    L.qm_last_kernel_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.qm_ctx_stat.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64)]
    L.qm_fetch_skipped.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    L.qm_collect_reads.argtypes = [C.c_void_p, C.POINTER(QmOpts), C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
    L.qm_fetch_found.argtypes = [C.c_void_p, C.c_void_p]
    L.qm_hits_to_mappings.argtypes = [C.c_void_p, C.POINTER(QmOpts), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
    L.qm_fetch_read_lists.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    L.qm_merge_lists.argtypes = [C.c_void_p, C.POINTER(QmOpts), C.c_int64] + [C.c_void_p] * 8 + [C.POINTER(C.c_int64), C.POINTER(QmCounters)]
    L.qm_fetch_too_many.argtypes = [C.c_void_p, C.c_void_p]
    L.qm_map_pairs_stages.argtypes = L.qm_map_pairs.argtypes
    L.qm_pack_reads.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    L.qm_map_pairs_packed.argtypes = [C.c_void_p, C.POINTER(QmOpts), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(QmCounters)]
    L.qm_map_reads_packed.argtypes = [C.c_void_p, C.POINTER(QmOpts), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                      C.POINTER(C.c_int64), C.POINTER(QmCounters)]
    L.qm_stage_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    L.qm_fetch_stages.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(QmStageView)]
    L.qm_pinned_alloc.argtypes = [C.c_int64]; L.qm_pinned_alloc.restype = C.c_void_p
    L.qm_pinned_free.argtypes = [C.c_void_p]; L.qm_pinned_free.restype = None
    L.qm_stream_open.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.POINTER(QmOpts), C.c_char_p, C.c_char_p, C.c_int64, C.c_int32,
                                 C.POINTER(C.c_void_p)]
    L.qm_stream_open_ex.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.c_uint32, C.POINTER(QmOpts), C.c_char_p, C.c_char_p,
                                    C.c_int64, C.c_int32, C.c_uint32, C.POINTER(C.c_void_p)]
    L.qm_stream_reserve.argtypes = [C.c_int64]
    L.qm_stream_stats.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    L.qm_stream_stats_ex.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int32]
    L.qm_stream_next.argtypes = [C.c_void_p, C.POINTER(QmStreamBatch)]
    L.qm_stream_close.argtypes = [C.c_void_p]
    L.qm_stream_last_error.restype = C.c_char_p
    L.qm_fetch_hits_pinned.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.qm_build_index.argtypes = [C.c_char_p, C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    L.qm_build_index_ex.argtypes = [C.c_char_p, C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_char_p]
    L.qm_opts_default.argtypes = [C.POINTER(QmOpts)]
    L.qm_io_last_error.restype = C.c_char_p
    L.qm_reader_open.argtypes = [C.c_char_p, C.c_char_p, C.c_int32, C.POINTER(C.c_void_p)]
    L.qm_reader_next.argtypes = [C.c_void_p, C.c_int64, C.POINTER(C.c_int64)] + [C.POINTER(C.c_void_p)] * 8
    L.qm_reader_close.argtypes = [C.c_void_p]
    L.qm_sam_header.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    L.qm_sam_records.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 10 + [C.c_int32, C.c_int32,
                                 C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    L.qm_sam_write.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 10 + [C.c_int32, C.c_int32, C.c_int,
                               C.POINTER(C.c_int64)]
    L.qm_sam_writer_open.argtypes = [C.c_void_p, C.c_int, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    L.qm_sam_writer_open_ex.argtypes = [C.c_void_p, C.c_int, C.c_int32, C.c_int32, C.c_uint32, C.POINTER(C.c_void_p)]
    L.qm_sam_writer_header.argtypes = [C.c_void_p]
    L.qm_sam_writer_put.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 10
    L.qm_sam_writer_close.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    L.qm_buf_free.argtypes = [C.c_void_p]
    L.qm_eqc_create.argtypes = [C.c_void_p, C.c_int64, C.c_uint32, C.POINTER(C.c_void_p)]
    L.qm_eqc_destroy.argtypes = [C.c_void_p]
    L.qm_eqc_clear.argtypes = [C.c_void_p]
    L.qm_eqc_add.argtypes = [C.c_void_p, C.c_void_p]
    L.qm_eqc_add_labels.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.qm_eqc_size.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_uint64)]
    L.qm_eqc_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.qm_eqc_stat.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64)]
    L.qm_stream_eqc_finish.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.qm_stream_eqc_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.qm_quant_create.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_void_p)]
    L.qm_quant_set_start.argtypes = [C.c_void_p, C.c_void_p]
    L.qm_quant_set_method.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.qm_quant_exp_digamma.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
    L.qm_quant_run.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_double, C.POINTER(C.c_int32), C.POINTER(C.c_double)]
    L.qm_quant_fetch.argtypes = [C.c_void_p, C.c_void_p]
    L.qm_quant_stat.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64)]
    L.qm_quant_destroy.argtypes = [C.c_void_p]
    L.qm_quant_fetch_classes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.qm_boot_create.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
    L.qm_boot_resample.argtypes = [C.c_void_p, C.c_uint64, C.c_int64]
    L.qm_boot_set_counts.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    L.qm_boot_fetch_counts.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    L.qm_boot_run.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_void_p, C.c_void_p]
    L.qm_boot_fetch.argtypes = [C.c_void_p, C.c_void_p]
    L.qm_boot_stat.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64)]
    L.qm_boot_destroy.argtypes = [C.c_void_p]
    L.qm_fld_create.argtypes = [C.c_void_p, C.c_int32, C.c_uint32, C.POINTER(C.c_void_p)]
    L.qm_fld_destroy.argtypes = [C.c_void_p]
    L.qm_fld_clear.argtypes = [C.c_void_p]
    L.qm_fld_add.argtypes = [C.c_void_p, C.c_void_p]
    L.qm_fld_add_hits.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.qm_fld_add_counts.argtypes = [C.c_void_p, C.c_void_p]
    L.qm_fld_fetch.argtypes = [C.c_void_p, C.c_void_p]
    L.qm_fld_stat.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64)]
    L.qm_fld_eff_lens_from_counts.argtypes = [C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.qm_fld_eff_lens.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.qm_stream_fld_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.qm_gcb_create.argtypes = [C.c_void_p, C.c_int32, C.c_uint32, C.POINTER(C.c_void_p)]
    L.qm_gcb_destroy.argtypes = [C.c_void_p]
    L.qm_gcb_clear.argtypes = [C.c_void_p]
    L.qm_gcb_add.argtypes = [C.c_void_p, C.c_void_p]
    L.qm_gcb_add_hits.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.qm_gcb_add_counts.argtypes = [C.c_void_p, C.c_void_p]
    L.qm_gcb_fetch.argtypes = [C.c_void_p, C.c_void_p]
    L.qm_gcb_stat.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64)]
    L.qm_gcb_expect.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    L.qm_gcb_eff_lens_from_counts.argtypes = [C.c_int32, C.c_void_p, C.c_int64] + [C.c_void_p] * 7
    L.qm_gcb_window_gc.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.qm_stream_gcb_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.qm_sqb_create.argtypes = [C.c_void_p, C.c_int32, C.c_uint32, C.POINTER(C.c_void_p)]
    L.qm_sqb_destroy.argtypes = [C.c_void_p]
    L.qm_sqb_clear.argtypes = [C.c_void_p]
    L.qm_sqb_add.argtypes = [C.c_void_p, C.c_void_p]
    L.qm_sqb_add_hits.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.qm_sqb_add_counts.argtypes = [C.c_void_p, C.c_void_p]
    L.qm_sqb_fetch.argtypes = [C.c_void_p, C.c_void_p]
    L.qm_sqb_stat.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64)]
    L.qm_sqb_expect.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.qm_sqb_eff_lens.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.qm_sqb_context.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.qm_sqb_weights.argtypes = [C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]
    L.qm_sqb_ratios.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.qm_stream_sqb_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.qm_psb_create.argtypes = [C.c_void_p, C.c_int32, C.c_uint32, C.POINTER(C.c_void_p)]
    L.qm_psb_destroy.argtypes = [C.c_void_p]
    L.qm_psb_clear.argtypes = [C.c_void_p]
    L.qm_psb_add.argtypes = [C.c_void_p, C.c_void_p]
    L.qm_psb_add_hits.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.qm_psb_add_counts.argtypes = [C.c_void_p, C.c_void_p]
    L.qm_psb_fetch.argtypes = [C.c_void_p, C.c_void_p]
    L.qm_psb_stat.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64)]
    L.qm_psb_expect.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.qm_psb_eff_lens.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.qm_psb_position.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.qm_psb_ratios.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.qm_stream_psb_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.qm_lib_create.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
    L.qm_lib_destroy.argtypes = [C.c_void_p]
    L.qm_lib_clear.argtypes = [C.c_void_p]
    L.qm_lib_add.argtypes = [C.c_void_p, C.c_void_p]
    L.qm_lib_add_hits.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.qm_lib_compact_hits.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.qm_lib_add_counts.argtypes = [C.c_void_p, C.c_void_p]
    L.qm_lib_fetch.argtypes = [C.c_void_p, C.c_void_p]
    L.qm_lib_stat.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64)]
    L.qm_eqc_add_lib.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.qm_lib_type_mask.argtypes = [C.c_char_p, C.POINTER(C.c_uint32)]
    L.qm_lib_infer.argtypes = [C.c_void_p, C.c_char_p]
    L.qm_stream_lib_fetch.argtypes = [C.c_void_p, C.c_void_p]
    _lib = L
    return L


def lib_():
    """lib(), for a method whose own parameter is called lib"""
    return lib()


def _check(rc):
    if rc != 0:
        raise QmError("qmap_mi355 error %d: %s" % (rc, lib().qm_last_error().decode(errors="replace")))


def default_opts(**kw):
    """`rapmap quasimap` defaults (src/RapMapSAMapper.cpp:992-1023,1113-1114)."""
    o = QmOpts()
    _check(lib().qm_opts_default(C.byref(o)))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise AttributeError(k)
        setattr(o, k, v)
    return o


def build_index(fasta, out_dir, k=31, no_clip_poly_a=False, keep_duplicates=False, threads=None, perfect_hash=False, header_sep=None):
    """`rapmap quasiindex -t FASTA -i OUT -k K [-p] [-s SEP]` (src/RapMapSAIndexer.cpp:821-927); int64 ("BigSA") form for a text beyond 2^31 - 2 characters."""
    threads = threads or min(32, os.cpu_count() or 1)
    rc = lib().qm_build_index_ex(os.fsencode(fasta), os.fsencode(out_dir), k, int(no_clip_poly_a), int(keep_duplicates), threads,
                                 int(perfect_hash), header_sep.encode() if header_sep is not None else None)
    if rc != 0:
        lib().qm_indexer_last_error.restype = C.c_char_p
        raise QmError("qm_build_index failed (%d): %s" % (rc, lib().qm_indexer_last_error().decode()))


def pack_reads(reads):
    """list of bytes/str -> (uint8 concat, int64 offsets[n+1])"""
    bs = [r.encode() if isinstance(r, str) else bytes(r) for r in reads]
    off = np.zeros(len(bs) + 1, dtype=np.int64)
    if bs:
        np.cumsum([len(b) for b in bs], out=off[1:])
    seq = np.frombuffer(b"".join(bs), dtype=np.uint8).copy() if bs else np.zeros(0, np.uint8)
    return seq, off


class QuasiIndex:
    """RapMapSAIndex<int32_t | int64_t, RegHashT | PerfectHashT>: load() == qm_index_open (src/RapMapSAIndex.cpp:97-176)."""

    def __init__(self, index_dir):
        self._h = C.c_void_p()
        _check(lib().qm_index_open(os.fsencode(index_dir), C.byref(self._h)))
        info = QmIndexInfo()
        _check(lib().qm_index_info_get(self._h, C.byref(info)))
        self.k, self.text_len, self.n_txps, self.n_keys = info.k, info.text_len, info.n_txps, info.n_keys
        self.perfect_hash = bool(info.perfect_hash)
        self.big_sa = bool(info.big_sa)     # int64 on disk (RapMapSAIndex<int64_t, ...>), unsigned 32-bit offsets on the device
        self._names = None
        self._lens = None

    @property
    def txp_names(self):
        if self._names is None:
            self._names = [lib().qm_index_txp_name(self._h, i).decode() for i in range(self.n_txps)]
        return self._names

    @property
    def txp_lens(self):
        if self._lens is None:
            self._lens = np.array([lib().qm_index_txp_len(self._h, i) for i in range(self.n_txps)], dtype=np.int64)
        return self._lens

    def arrays(self):
        """(text uint8[n], txpOffsets int64[T]) -- copies of rmi.seq / rmi.txpOffsets"""
        tp, tl, op, nt = C.c_void_p(), C.c_int64(), C.c_void_p(), C.c_int64()
        _check(lib().qm_index_arrays(self._h, C.byref(tp), C.byref(tl), C.byref(op), C.byref(nt)))
        text = np.ctypeslib.as_array(C.cast(tp, C.POINTER(C.c_uint8)), shape=(tl.value,)).copy()
        raw = np.ctypeslib.as_array(C.cast(op, C.POINTER(C.c_uint8)), shape=(nt.value * 4,)).copy()
        return text, raw.view("<u4").astype(np.int64)      # unsigned: a BigSA index has offsets beyond 2^31

    def raw(self, which):
        """zero-copy view of one of the library's own arrays of the open index (qm_index_raw): "sa" uint32[nSA], "hash" records
        {key u8, lb u4, ub u4} in file order (empty for a -p index), "complete_lens" uint32[T]; valid until close()"""
        code, dt = {"sa": (0, np.dtype("<u4")), "hash": (1, np.dtype([("key", "<u8"), ("lb", "<u4"), ("ub", "<u4")])), "complete_lens": (2, np.dtype("<u4"))}[which]
        p, n = C.c_void_p(), C.c_int64()
        _check(lib().qm_index_raw(self._h, code, C.byref(p), C.byref(n)))
        return _view(p, n.value, dt)

    def close(self):
        if self._h:
            lib().qm_index_close(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MapResult:
    __slots__ = ("hit_offsets", "hits", "counters", "n_hits", "map_kernel_ms", "total_ms")


class QuasiMapper:
    """One GPU context: the index replicated in HBM + work buffers.  `map_pairs` performs, for every
    pair, SACollector() x2 -> hitsToMappingsSimple() x2 -> mergeLeftRightHits() on one wavefront."""

    def __init__(self, index: QuasiIndex, device=0, debug=False, reuse_results=False, ph_compact=False, pair_kernel=True, wide_reads=False):
        """reuse_results: hit arrays of successive calls share one buffer (views valid until the next call) instead of
        a fresh allocation per batch, whose pages would have to be faulted in again every time -- for streaming callers
        that are done with a batch before they map the next (the CLI)"""
        self._reuse = bool(reuse_results)
        self._buf_hits = None
        self._buf_offs = None
        self.index = index
        self._h = C.c_void_p()
        # ph_compact: a -p index keeps the BooPHF / FrugalBooMap structure on the device instead of the expanded bucket table
        # pair_kernel=False: QM_CTX_NO_PAIR_KERNEL (paired reads of up to 128 characters take qm_lean_kernel alone); wide_reads: QM_CTX_WIDE_READS
        _check(lib().qm_ctx_create_ex(index._h, device, (1 if ph_compact else 0) | (0 if pair_kernel else 2) | (4 if wide_reads else 0), C.byref(self._h)))
        if debug:
            _check(lib().qm_ctx_set_debug(self._h, 1))
        self.device = device

    @property
    def device_bytes(self):
        return lib().qm_ctx_device_bytes(self._h)

    def _finish(self, n, n_hits, ctr, fetch=True):
        r = MapResult()
        r.n_hits = n_hits.value
        r.counters = ctr.as_dict()
        a, b = C.c_double(), C.c_double()
        _check(lib().qm_last_kernel_ms(self._h, C.byref(a), C.byref(b)))
        r.map_kernel_ms, r.total_ms = a.value, b.value
        if fetch and self._reuse:
            nh = max(r.n_hits, 0)
            if self._buf_hits is None or self._buf_hits.size < nh:
                self._buf_hits = np.empty(nh + nh // 4 + 1024, dtype=HIT_DTYPE)
            if self._buf_offs is None or self._buf_offs.size < n + 1:
                self._buf_offs = np.empty(n + 1 + n // 4, dtype=np.int64)
            r.hit_offsets = self._buf_offs[: n + 1]
            r.hits = self._buf_hits[:nh]
            _check(lib().qm_fetch_hits(self._h, r.hit_offsets.ctypes.data, r.hits.ctypes.data if r.n_hits else None))
        elif fetch:
            r.hit_offsets = np.zeros(n + 1, dtype=np.int64)
            r.hits = np.zeros(max(r.n_hits, 0), dtype=HIT_DTYPE)
            _check(lib().qm_fetch_hits(self._h, r.hit_offsets.ctypes.data, r.hits.ctypes.data if r.n_hits else None))
        else:
            r.hit_offsets = r.hits = None
        return r

    def map_pairs(self, seq1, off1, seq2, off2, opts=None):
        opts = opts or default_opts()
        seq1 = np.ascontiguousarray(seq1, dtype=np.uint8); off1 = np.ascontiguousarray(off1, dtype=np.int64)
        seq2 = np.ascontiguousarray(seq2, dtype=np.uint8); off2 = np.ascontiguousarray(off2, dtype=np.int64)
        n = len(off1) - 1
        if len(off2) - 1 != n:
            raise ValueError("left/right read counts differ")
        nh, ctr = C.c_int64(0), QmCounters()
        # numpy gives a non-null pointer even for empty arrays
        _check(lib().qm_map_pairs(self._h, C.byref(opts), n, seq1.ctypes.data or 1, off1.ctypes.data,
                                  seq2.ctypes.data or 1, off2.ctypes.data, C.byref(nh), C.byref(ctr)))
        return self._finish(n, nh, ctr)

    def map_reads(self, seq, off, opts=None):
        opts = opts or default_opts()
        seq = np.ascontiguousarray(seq, dtype=np.uint8); off = np.ascontiguousarray(off, dtype=np.int64)
        n = len(off) - 1
        nh, ctr = C.c_int64(0), QmCounters()
        _check(lib().qm_map_reads(self._h, C.byref(opts), n, seq.ctypes.data or 1, off.ctypes.data, C.byref(nh), C.byref(ctr)))
        return self._finish(n, nh, ctr)

    def map_device(self, n, d_seq1, d_off1, d_seq2, d_off2, max_read_len, opts=None, fetch=False):
        """Inputs are raw device pointers (ints) of arrays already resident in this GPU's HBM."""
        opts = opts or default_opts()
        nh, ctr = C.c_int64(0), QmCounters()
        _check(lib().qm_map_device(self._h, C.byref(opts), n, d_seq1, d_off1, d_seq2, d_off2, max_read_len,
                                   C.byref(nh), C.byref(ctr)))
        return self._finish(n, nh, ctr, fetch=fetch)

    def skipped(self):
        """qm_fetch_skipped: the reads of the last call that were skipped, not mapped -> (total, reads int64[], codes int32[]);
        code 1: longer than QM_MAX_LONG_READ_LEN characters, 2: interval lists beyond the scratch (max_interval above its default)"""
        tot = C.c_int64()
        _check(lib().qm_fetch_skipped(self._h, None, None, 0, C.byref(tot)))
        n = min(tot.value, 4096)
        reads = np.zeros(n, dtype=np.int64); codes = np.zeros(n, dtype=np.int32)
        if n:
            _check(lib().qm_fetch_skipped(self._h, reads.ctypes.data, codes.ctypes.data, n, C.byref(tot)))
        return tot.value, reads, codes

    def stat(self, which):
        """qm_ctx_stat; which is one of this module's QM_STAT_*: RELAUNCHES stage-A relaunches of the last call, LIST_WORDS list buffer capacity
        (words), SLOW_READS reads on the -s slow path, LEAN_READS reads the lean stage-A kernel was launched over (-1: the general kernel ran),
        LEAN_DEFERRED reads it left to the general kernel, SKIPPED_READS reads that were skipped (qm_fetch_skipped), SEL_QUESTIONS / KSW2_ALIGNMENTS /
        STRIP_ALIGNMENTS (-s) alignment questions beyond PERFECT chains / ksw2 alignments run for them / alignments the strip DP answered,
        PAIR_KERNEL_PAIRS pairs the pair kernel was launched over (-1: not used), PAIRS_MERGED pairs it merged itself, DEFER_DIRTY / DEFER_HOMOPOLYMER /
        DEFER_WIDE / DEFER_BOTH_STRANDS why the reads of LEAN_DEFERRED were left: a character that is not A C G T / a window of k equal bases / an
        interval or a list beyond the kernel's lanes / hits on the other strand as well, N_PASS_READS reads with N's that the N-aware second pass of
        stage A mapped (not part of LEAN_DEFERRED or DEFER_DIRTY)"""
        v = C.c_int64()
        _check(lib().qm_ctx_stat(self._h, int(which), C.byref(v)))
        return v.value

    # ---- the reference's three entry points as calls of their own (include/qmap_mi355.h) ----
    def collect_reads(self, seq, off, opts=None):
        """SACollector::operator() for every read: (found uint8[n], int_offsets int64[n+1], intervals)"""
        opts = opts or default_opts()
        seq = np.ascontiguousarray(seq, dtype=np.uint8); off = np.ascontiguousarray(off, dtype=np.int64)
        n = len(off) - 1
        ni = C.c_int64(0)
        _check(lib().qm_collect_reads(self._h, C.byref(opts), n, seq.ctypes.data or 1, off.ctypes.data, C.byref(ni)))
        found = np.zeros(n + 1, dtype=np.uint8)
        _check(lib().qm_fetch_found(self._h, found.ctypes.data))
        offs, ints = self.intervals(n)
        return found[:n], offs, ints

    def hits_to_mappings(self, read_len, int_offsets, ints, opts=None):
        """hitsToMappingsSimple for every read from its SA-interval hits: (list_offsets int64[n+1], words uint64[])"""
        opts = opts or default_opts()
        read_len = np.ascontiguousarray(read_len, dtype=np.int32); int_offsets = np.ascontiguousarray(int_offsets, dtype=np.int64)
        ints = np.ascontiguousarray(ints, dtype=INTERVAL_DTYPE)
        n = len(read_len)
        nw = C.c_int64(0)
        _check(lib().qm_hits_to_mappings(self._h, C.byref(opts), n, read_len.ctypes.data or 1, int_offsets.ctypes.data,
                                         ints.ctypes.data if ints.size else None, C.byref(nw)))
        return self.read_lists(n)

    def read_lists(self, nreads):
        lo = np.zeros(nreads + 1, dtype=np.int64)
        _check(lib().qm_fetch_read_lists(self._h, lo.ctypes.data, None, 0))
        w = np.zeros(int(lo[-1]) + 1, dtype=np.uint64)
        _check(lib().qm_fetch_read_lists(self._h, lo.ctypes.data, w.ctypes.data, int(lo[-1])))
        return lo, w[: int(lo[-1])]

    def merge_lists(self, lo_l, w_l, lo_r, w_r, found_l, found_r, len_l, len_r, opts=None):
        """mergeLeftRightHits[Fuzzy] for every pair: MapResult (hits, counters) + .too_many uint8[n]"""
        opts = opts or default_opts()
        a = [np.ascontiguousarray(lo_l, dtype=np.int64), np.ascontiguousarray(w_l, dtype=np.uint64), np.ascontiguousarray(lo_r, dtype=np.int64),
             np.ascontiguousarray(w_r, dtype=np.uint64), np.ascontiguousarray(found_l, dtype=np.uint8), np.ascontiguousarray(found_r, dtype=np.uint8),
             np.ascontiguousarray(len_l, dtype=np.int32), np.ascontiguousarray(len_r, dtype=np.int32)]
        n = len(a[0]) - 1
        nh, ctr = C.c_int64(0), QmCounters()
        _check(lib().qm_merge_lists(self._h, C.byref(opts), n, *[x.ctypes.data if x.size else None for x in a], C.byref(nh), C.byref(ctr)))
        r = self._finish(n, nh, ctr)
        tm = np.zeros(n + 1, dtype=np.uint8)
        _check(lib().qm_fetch_too_many(self._h, tm.ctypes.data))
        r_too = tm[:n]
        return r, r_too

    def map_pairs_packed(self, seq1, off1, seq2, off2, opts=None):
        """map_pairs with the reads sent 2-bit packed (qm_pack_reads on the host, qm_map_pairs_packed): same result"""
        opts = opts or default_opts()
        a = [pack_2bit(seq1, off1), pack_2bit(seq2, off2)]
        n = len(a[0][1]) - 1
        nh, ctr = C.c_int64(0), QmCounters()
        _check(lib().qm_map_pairs_packed(self._h, C.byref(opts), n, a[0][0].ctypes.data, a[0][1].ctypes.data, a[0][2].ctypes.data, len(a[0][2]),
                                         a[1][0].ctypes.data, a[1][1].ctypes.data, a[1][2].ctypes.data, len(a[1][2]), C.byref(nh), C.byref(ctr)))
        return self._finish(n, nh, ctr)

    def map_pairs_prepacked(self, pk1, off1, exc1, pk2, off2, exc2, opts=None, fetch=True):
        """qm_map_pairs_packed on reads that are packed already (pack_2bit / pinned_copy): what a caller that keeps its batches 2-bit packed pays per call"""
        opts = opts or default_opts()
        n = len(off1) - 1
        nh, ctr = C.c_int64(0), QmCounters()
        _check(lib().qm_map_pairs_packed(self._h, C.byref(opts), n, pk1.ctypes.data, off1.ctypes.data, exc1.ctypes.data if len(exc1) else None, len(exc1),
                                         pk2.ctypes.data, off2.ctypes.data, exc2.ctypes.data if len(exc2) else None, len(exc2), C.byref(nh), C.byref(ctr)))
        return self._finish(n, nh, ctr, fetch=fetch)

    def map_reads_packed(self, seq, off, opts=None):
        opts = opts or default_opts()
        pk, off, exc = pack_2bit(seq, off)
        n = len(off) - 1
        nh, ctr = C.c_int64(0), QmCounters()
        _check(lib().qm_map_reads_packed(self._h, C.byref(opts), n, pk.ctypes.data, off.ctypes.data, exc.ctypes.data, len(exc), C.byref(nh), C.byref(ctr)))
        return self._finish(n, nh, ctr)

    def map_pairs_stages(self, seq1, off1, seq2, off2, opts=None, no_intervals=False, packed=False):
        """the three stages fused, every stage's output kept: MapResult of the merge (no caller-level bookkeeping).
        no_intervals: QM_STAGES_NO_INTERVALS (the stage view's interval arrays stay empty); packed: the reads go up 2-bit packed"""
        opts = opts or default_opts()
        seq1 = np.ascontiguousarray(seq1, dtype=np.uint8); off1 = np.ascontiguousarray(off1, dtype=np.int64)
        seq2 = np.ascontiguousarray(seq2, dtype=np.uint8); off2 = np.ascontiguousarray(off2, dtype=np.int64)
        n = len(off1) - 1
        nh, ctr = C.c_int64(0), QmCounters()
        fl = 1 if no_intervals else 0
        if packed:
            a = [pack_2bit(seq1, off1), pack_2bit(seq2, off2)]
            _check(lib().qm_map_pairs_stages_packed(self._h, C.byref(opts), C.c_int64(n), C.c_void_p(a[0][0].ctypes.data), C.c_void_p(a[0][1].ctypes.data),
                                                    C.c_void_p(a[0][2].ctypes.data if len(a[0][2]) else None), C.c_int64(len(a[0][2])),
                                                    C.c_void_p(a[1][0].ctypes.data), C.c_void_p(a[1][1].ctypes.data),
                                                    C.c_void_p(a[1][2].ctypes.data if len(a[1][2]) else None), C.c_int64(len(a[1][2])), C.c_uint32(fl), C.byref(nh), C.byref(ctr)))
        elif fl:
            _check(lib().qm_map_pairs_stages_ex(self._h, C.byref(opts), C.c_int64(n), C.c_void_p(seq1.ctypes.data or 1), C.c_void_p(off1.ctypes.data),
                                                C.c_void_p(seq2.ctypes.data or 1), C.c_void_p(off2.ctypes.data), C.c_uint32(fl), C.byref(nh), C.byref(ctr)))
        else:
            _check(lib().qm_map_pairs_stages(self._h, C.byref(opts), n, seq1.ctypes.data or 1, off1.ctypes.data,
                                             seq2.ctypes.data or 1, off2.ctypes.data, C.byref(nh), C.byref(ctr)))
        return self._finish(n, nh, ctr)

    def fetch_stages(self, pinned=True):
        """qm_fetch_stages after map_pairs_stages: every stage's output in one download, compacted on the device.  Returns a dict of
        numpy views into an arena this mapper keeps (valid until the next fetch_stages): iv_off / iv / found per READ (2u left,
        2u + 1 right), list_off / words per read, hit_off / hits / too_many per pair."""
        need = C.c_int64(0)
        _check(lib().qm_stage_bytes(self._h, C.byref(need)))
        if getattr(self, "_arena_cap", 0) < need.value:
            if getattr(self, "_arena", None) and self._arena_pinned:
                lib().qm_pinned_free(self._arena)
            self._arena_cap = need.value + need.value // 2 + 4096
            self._arena_pinned = bool(pinned)
            if pinned:
                self._arena = lib().qm_pinned_alloc(self._arena_cap)
                if not self._arena:
                    raise QmError("out of page-locked host memory")
            else:
                self._arena_np = np.zeros(self._arena_cap, dtype=np.uint8)
                self._arena = self._arena_np.ctypes.data
        v = QmStageView()
        _check(lib().qm_fetch_stages(self._h, C.c_void_p(self._arena), self._arena_cap, C.byref(v)))
        nr, n = v.n_reads, v.n_units
        out = {"n_units": n, "n_reads": nr}
        out["iv_off"] = _view(v.iv_off, nr + 1, np.int64); out["iv"] = _view(v.iv, int(out["iv_off"][-1]), INTERVAL_DTYPE)
        out["found"] = _view(v.found, nr, np.uint8)
        out["list_off"] = _view(v.list_off, nr + 1, np.int64); out["words"] = _view(v.words, int(out["list_off"][-1]), np.uint64)
        out["hit_off"] = _view(v.hit_off, n + 1, np.int64); out["hits"] = _view(v.hits, int(out["hit_off"][-1]), HIT_DTYPE)
        out["too_many"] = _view(v.too_many, n, np.uint8)
        return out

    def intervals(self, n):
        """fwdSAInts / rcSAInts kept by the last call (fused calls: needs debug=True)."""
        offs = np.zeros(n + 1, dtype=np.int64)
        _check(lib().qm_fetch_intervals(self._h, offs.ctypes.data, None, 0))
        ints = np.zeros(int(offs[-1]), dtype=INTERVAL_DTYPE)
        if ints.size:
            _check(lib().qm_fetch_intervals(self._h, offs.ctypes.data, ints.ctypes.data, ints.size))
        return offs, ints

    def close(self):
        if self._h:
            if getattr(self, "_arena", None) and getattr(self, "_arena_pinned", False):
                lib().qm_pinned_free(self._arena)
            self._arena = None; self._arena_cap = 0
            lib().qm_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def write_eq_classes(path, txp_names, label_offsets, tids, counts):
    """Salmon's eq_classes.txt: the number of transcripts, the number of classes, one transcript name per line, then per class
    (in the order given: EqClasses.fetch's canonical one) `k<TAB>t1<TAB>...<TAB>tk<TAB>count`"""
    label_offsets = np.asarray(label_offsets, dtype=np.int64); tids = np.asarray(tids, dtype=np.uint32); counts = np.asarray(counts, dtype=np.uint64)
    nc = len(label_offsets) - 1
    with open(path, "w") as f:
        f.write("%d\n%d\n" % (len(txp_names), nc))
        for nm in txp_names:
            f.write(nm + "\n")
        out = []
        for i in range(nc):
            a, b = int(label_offsets[i]), int(label_offsets[i + 1])
            out.append("\t".join([str(b - a)] + [str(int(t)) for t in tids[a:b]] + [str(int(counts[i]))]))
            if len(out) >= 65536:
                f.write("\n".join(out) + "\n"); out = []
        if out:
            f.write("\n".join(out) + "\n")


def read_eq_classes(path):
    """the inverse of write_eq_classes: (txp_names, label_offsets int64[nc + 1], tids uint32[], counts uint64[nc])"""
    with open(path) as f:
        nt = int(f.readline()); nc = int(f.readline())
        names = [f.readline().rstrip("\n") for _ in range(nt)]
        off = np.zeros(nc + 1, dtype=np.int64); tids = []; counts = np.zeros(nc, dtype=np.uint64)
        for i in range(nc):
            w = f.readline().split("\t")
            k = int(w[0])
            if len(w) != k + 2:
                raise ValueError("%s: class %d has %d fields, %d expected" % (path, i, len(w), k + 2))
            tids.extend(int(x) for x in w[1:1 + k]); counts[i] = int(w[1 + k]); off[i + 1] = off[i] + k
    return names, off, np.array(tids, dtype=np.uint32), counts


def _host_hits(hit_offsets, hits):
    """(n, hit_offsets int64[n + 1], hits HIT_DTYPE[]) of host arrays in CSR form, checked"""
    hit_offsets = np.ascontiguousarray(hit_offsets, dtype=np.int64)
    hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE) if hits is not None else np.zeros(0, dtype=HIT_DTYPE)
    n = len(hit_offsets) - 1
    if n < 0:
        raise ValueError("hit_offsets needs n + 1 entries")
    if n and int(hit_offsets[-1]) > hits.size:
        raise ValueError("hit_offsets point beyond hits")
    return n, hit_offsets, hits


class _Object:
    """what the estimation classes share: the ABI handle self._h; close() through the class's destroy function (DESTROY), whose
    answer is looked at only where CLOSE_RAISES; __del__; and stat(), a dictionary of STATS from the class's stat function (STAT)"""

    DESTROY = STAT = None
    STATS = ()
    CLOSE_RAISES = False

    def _stat(self, which):
        v = C.c_int64()
        _check(getattr(lib(), self.STAT)(self._h, int(which), C.byref(v)))
        return v.value

    def stat(self):
        return {k: self._stat(i) for i, k in enumerate(self.STATS)}

    def close(self):
        if self._h:
            rc = getattr(lib(), self.DESTROY)(self._h)
            if self.CLOSE_RAISES:
                _check(rc)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class EqClasses(_Object):
    """qm_eqc_*: a label -> count table in the device memory of a mapper's GPU.  A unit's label is the ascending list of the
    distinct transcripts of its hit list; add(mapper) folds the mapper's last result where it lies (no hit crosses PCIe),
    add_labels folds lists held on the host (the merge primitive: another table's fetch() with its counts as weights).
    expected: classes to size the table for (it grows by itself); hash_bits: keep only that many bits of the 64-bit key (tests)."""

    GROWTHS, COLLISION_PROBES, LONG_UNITS, ROUNDS, LAST_FOLD_US = 0, 1, 2, 3, 4
    DESTROY, STAT = "qm_eqc_destroy", "qm_eqc_stat"

    def __init__(self, mapper, expected=1 << 16, hash_bits=0):
        self._h = C.c_void_p()
        if not 0 <= int(hash_bits) <= 63:
            raise ValueError("hash_bits must be 0 .. 63")
        _check(lib().qm_eqc_create(mapper._h, int(expected), int(hash_bits) << 8, C.byref(self._h)))
        self.device = mapper.device

    def add(self, mapper, lib=None):
        """fold the result of the mapper's last map call; lib (a LibFormat): only the hits its library type keeps are folded, and the
        batch is tallied into it (qm_eqc_add_lib)"""
        if lib is None:
            _check(lib_().qm_eqc_add(self._h, mapper._h))
        else:
            _check(lib_().qm_eqc_add_lib(self._h, mapper._h, lib._h))

    def add_labels(self, offsets, tids, weights=None):
        offsets = np.ascontiguousarray(offsets, dtype=np.int64); tids = np.ascontiguousarray(tids, dtype=np.uint32)
        n = len(offsets) - 1
        if n < 0:
            raise ValueError("offsets needs n + 1 entries")
        if n and int(offsets[-1]) > tids.size:
            raise ValueError("offsets point beyond tids")
        if weights is not None:
            weights = np.ascontiguousarray(weights, dtype=np.uint64)
            if weights.size != n:
                raise ValueError("one weight per list")
        _check(lib().qm_eqc_add_labels(self._h, n, offsets.ctypes.data, tids.ctypes.data if tids.size else None,
                                       weights.ctypes.data if weights is not None and n else None))

    def _size(self):
        nc, nt, tot = C.c_int64(), C.c_int64(), C.c_uint64()
        _check(lib().qm_eqc_size(self._h, C.byref(nc), C.byref(nt), C.byref(tot)))
        return nc.value, nt.value, tot.value

    @property
    def n_classes(self):
        return self._size()[0]

    @property
    def total(self):
        """sum of all counts: the units (weights) folded so far that had a hit"""
        return self._size()[2]

    def fetch(self):
        """(label_offsets int64[n_classes + 1], tids uint32[], counts uint64[n_classes]), labels ascending (lexicographic)"""
        nc, nt, _ = self._size()
        off = np.zeros(nc + 1, dtype=np.int64); tids = np.zeros(nt + 1, dtype=np.uint32); cnt = np.zeros(nc + 1, dtype=np.uint64)
        _check(lib().qm_eqc_fetch(self._h, off.ctypes.data, tids.ctypes.data, cnt.ctypes.data))
        return off, tids[:nt], cnt[:nc]

    def stat(self, which):
        """qm_eqc_stat; which is one of this module's QM_EQC_STAT_*: GROWTHS, COLLISION_PROBES, LONG_UNITS, ROUNDS, LAST_FOLD_US (the last fold by
        HIP events on its stream)"""
        return self._stat(which)

    def clear(self):
        _check(lib().qm_eqc_clear(self._h))

    def write(self, path, txp_names):
        off, tids, cnt = self.fetch()
        write_eq_classes(path, txp_names, off, tids, cnt)

    def quantify(self, n_txps, eff_lens=None, method="em", prior=1e-2, per_transcript=False, **run_kw):
        """the one-call form of Quant: alpha float64[n_txps] after a run from the uniform start (method, prior, per_transcript:
        Quant.set_method's; run_kw: Quant.run's)"""
        q = Quant(self, n_txps, eff_lens)
        try:
            if method != "em":
                q.set_method(method, prior, per_transcript)
            q.run(**run_kw)
            return q.fetch()
        finally:
            q.close()


class Quant(_Object):
    """qm_quant_*: abundance estimation on the device, the EM over a snapshot of an EqClasses table (later folds into the table do
    not alter it).  One iteration, all in float64: w = alpha / eff; d_c = sum of w over the class's label; r_c = n_c / d_c;
    alpha'_t = w_t * sum of r_c over the classes that contain t.  eff_lens: n_txps positive numbers (None: 1.0 each).  The start is
    total / M for the M transcripts that occur in a label and 0 for the others, unless set_start gives another one.  set_method
    chooses the variational Bayes EM instead, which differs in w alone."""

    STATS = ("classes", "entries", "present", "longest_label", "longest_list", "queued_labels", "queued_txps", "last_run_us", "build_us")
    DESTROY, STAT, CLOSE_RAISES = "qm_quant_destroy", "qm_quant_stat", True

    def stat(self):
        """qm_quant_stat: a dictionary of STATS (last_run_us, build_us: the last run / the structure build by HIP events on its stream)"""
        return super().stat()

    def close(self):
        """qm_quant_destroy; raises while a Bootstrap of this object lives (nothing is destroyed then)"""
        super().close()
    DEFAULTS = dict(max_iter=10000, check_every=10, rel_tol=1e-2, min_alpha=1e-8)     # Salmon's offline EM

    def __init__(self, eq_classes, n_txps, eff_lens=None):
        self._h = C.c_void_p()
        self.n_txps = int(n_txps)
        if eff_lens is not None:
            eff_lens = np.ascontiguousarray(eff_lens, dtype=np.float64)
            if eff_lens.size != self.n_txps:
                raise ValueError("one effective length per transcript")
        _check(lib().qm_quant_create(eq_classes._h, self.n_txps, eff_lens.ctypes.data if eff_lens is not None and eff_lens.size else None,
                                     C.byref(self._h)))
        self.device = eq_classes.device
        self._eff = eff_lens                                          # (what a per-nucleotide prior is built from)

    METHODS = {"em": 0, "vbem": 1}                                    # QM_QUANT_METHOD_*

    def set_method(self, method="em", prior=1e-2, per_transcript=False):
        """qm_quant_set_method: "em", or "vbem": the variational Bayes EM, whose weight is w = exp(digamma(alpha + p)) / eff with the
        prior p_t = prior * eff_t (per nucleotide, the default) or p_t = prior (per_transcript=True); prior may also be an array of
        n_txps numbers, taken as p itself, or None (0.0 each).  Holds for every later run and for Bootstraps made later; alpha stays
        as it is, and keeps meaning the expected fragments without the prior.  Raises while a Bootstrap of this object lives."""
        if method not in self.METHODS:
            raise ValueError("method is 'em' or 'vbem'")
        p = None
        if method == "vbem" and prior is not None:
            if np.ndim(prior) == 0:
                p = np.full(self.n_txps, float(prior), dtype=np.float64)
                if not per_transcript and self._eff is not None:
                    p = float(prior) * self._eff
            else:
                p = np.ascontiguousarray(prior, dtype=np.float64)
                if p.size != self.n_txps:
                    raise ValueError("one prior per transcript")
        _check(lib().qm_quant_set_method(self._h, self.METHODS[method], p.ctypes.data if p is not None and p.size else None))

    def set_start(self, alpha0=None):
        """alpha0: n_txps non-negative numbers; None: the uniform default"""
        if alpha0 is not None:
            alpha0 = np.ascontiguousarray(alpha0, dtype=np.float64)
            if alpha0.size != self.n_txps:
                raise ValueError("one start value per transcript")
        _check(lib().qm_quant_set_start(self._h, alpha0.ctypes.data if alpha0 is not None and alpha0.size else None))

    def run(self, max_iter=DEFAULTS["max_iter"], check_every=DEFAULTS["check_every"], rel_tol=DEFAULTS["rel_tol"], min_alpha=DEFAULTS["min_alpha"]):
        """up to max_iter iterations from the current alpha -> (iterations, last_rel_change); the relative change is looked at every
        check_every-th iteration only (rel_tol=0: never, exactly max_iter iterations, last_rel_change -1)"""
        it, rel = C.c_int32(), C.c_double()
        _check(lib().qm_quant_run(self._h, int(max_iter), int(check_every), float(rel_tol), float(min_alpha), C.byref(it), C.byref(rel)))
        return it.value, rel.value

    def fetch(self):
        """the current alpha: float64[n_txps]"""
        a = np.zeros(self.n_txps, dtype=np.float64)
        _check(lib().qm_quant_fetch(self._h, a.ctypes.data if a.size else None))
        return a

    def classes(self):
        """qm_quant_fetch_classes: the snapshot's class side in the snapshot's own order, which is what a bootstrap draw is defined
        against (NOT the sorted order of EqClasses.fetch): (label_offsets int64[classes + 1], tids uint32[], counts uint64[classes])"""
        st = self.stat()
        nc, ne = st["classes"], st["entries"]
        off = np.zeros(nc + 1, dtype=np.int64); tids = np.zeros(ne + 1, dtype=np.uint32); cnt = np.zeros(nc + 1, dtype=np.uint64)
        _check(lib().qm_quant_fetch_classes(self._h, off.ctypes.data, tids.ctypes.data, cnt.ctypes.data))
        return off, tids[:ne], cnt[:nc]

    def bootstrap(self, n_reps, seed=0, **run_kw):
        """the one-call form of Bootstrap: float64[n_reps, n_txps], replicate numbers 0 .. n_reps - 1 under `seed` (run_kw: Bootstrap.run's)"""
        b = Bootstrap(self, n_reps)
        try:
            b.resample(seed=seed)
            b.run(**run_kw)
            return b.fetch()
        finally:
            b.close()


def exp_digamma(x, device=0):
    """qm_quant_exp_digamma: E(x) = exp(digamma(x)), 0 below 1e-10, as the variational method computes it on the device -> float64
    array of x's shape"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.zeros(x.shape, dtype=np.float64)
    _check(lib().qm_quant_exp_digamma(int(device), x.ctypes.data if x.size else None, x.size, out.ctypes.data if x.size else None))
    return out


class Bootstrap(_Object):
    """qm_boot_*: bootstrap replicates of a Quant's estimate on the device (Salmon's --numBootstraps).  A replicate resamples the
    snapshot's class counts -- N draws, a multinomial over the classes -- and runs Quant's method (the EM, or what set_method chose
    before this object was made) on them; n_reps replicates are iterated
    at once and each stops by itself.  Slot i holds replicate number first_rep + i; a replicate's counts depend on (snapshot, seed,
    replicate number) alone and its alpha on those and run's arguments, not on n_reps or its slot.  Borrows the Quant's graph and
    stream: close this before the Quant."""

    STATS = ("replicates", "draws", "last_resample_us", "last_run_us", "launches", "queued_labels", "queued_txps")
    DESTROY, STAT = "qm_boot_destroy", "qm_boot_stat"

    def stat(self):
        """qm_boot_stat: a dictionary of STATS (last_resample_us, last_run_us: by HIP events on the stream)"""
        return super().stat()

    def __init__(self, quant, n_reps):
        self._h = C.c_void_p()
        self.n_reps = int(n_reps); self.n_txps = quant.n_txps
        self._quant = quant                                           # (kept alive: the ABI object borrows it)
        _check(lib().qm_boot_create(quant._h, self.n_reps, C.byref(self._h)))
        self.n_classes = quant.stat()["classes"]

    def resample(self, seed=0, first_rep=0):
        """every slot anew: the counts of replicate numbers first_rep .. first_rep + n_reps - 1 under `seed`, the uniform start"""
        _check(lib().qm_boot_resample(self._h, int(seed) & (2 ** 64 - 1), int(first_rep)))

    def set_counts(self, rep, counts):
        """one slot's counts as given, in the order of Quant.classes(); the slot starts anew"""
        counts = np.ascontiguousarray(counts, dtype=np.uint64)
        if counts.size != self.n_classes:
            raise ValueError("one count per class")
        _check(lib().qm_boot_set_counts(self._h, int(rep), counts.ctypes.data if counts.size else None))

    def counts(self, rep):
        """one slot's counts: uint64[classes], in the order of Quant.classes()"""
        c = np.zeros(self.n_classes, dtype=np.uint64)
        _check(lib().qm_boot_fetch_counts(self._h, int(rep), c.ctypes.data if c.size else None))
        return c

    def run(self, max_iter=Quant.DEFAULTS["max_iter"], check_every=Quant.DEFAULTS["check_every"], rel_tol=Quant.DEFAULTS["rel_tol"],
            min_alpha=Quant.DEFAULTS["min_alpha"]):
        """Quant.run per replicate -> (iterations int32[n_reps] of this call, last relative change float64[n_reps]); a replicate that
        stopped is frozen, a later run goes on with the others"""
        it = np.zeros(self.n_reps, dtype=np.int32); rel = np.zeros(self.n_reps, dtype=np.float64)
        _check(lib().qm_boot_run(self._h, int(max_iter), int(check_every), float(rel_tol), float(min_alpha), it.ctypes.data, rel.ctypes.data))
        return it, rel

    def fetch(self):
        """the current alphas: float64[n_reps, n_txps]"""
        a = np.zeros((self.n_reps, self.n_txps), dtype=np.float64)
        _check(lib().qm_boot_fetch(self._h, a.ctypes.data if a.size else None))
        return a

    def close(self):
        if self._h:
            super().close()
            self._quant = None


def write_bootstraps(path, alphas):
    """Salmon's bootstraps.gz: gzip of B x n_txps little-endian float64, row-major, transcripts in quant.sf order"""
    import gzip
    a = np.ascontiguousarray(alphas, dtype="<f8")
    if a.ndim != 2:
        raise ValueError("alphas: [replicates, transcripts]")
    with gzip.open(path, "wb") as f:
        f.write(a.tobytes())


def read_bootstraps(path, n_txps):
    """the inverse of write_bootstraps: float64[B, n_txps]"""
    import gzip
    with gzip.open(path, "rb") as f:
        raw = f.read()
    if n_txps <= 0 or len(raw) % (8 * n_txps):
        raise ValueError("%s: %d bytes are no whole number of rows of %d float64" % (path, len(raw), n_txps))
    return np.frombuffer(raw, dtype="<f8").astype(np.float64).reshape(-1, n_txps)


QUANT_HEADER = "Name\tLength\tEffectiveLength\tTPM\tNumReads"


def write_quant(path, names, lens, eff_lens, alpha):
    """Salmon's quant.sf: Name, Length, EffectiveLength, TPM, NumReads, tab-separated under that header.  TPM is (alpha / eff) over
    its sum, times 1e6.  Floats are written with repr: read_quant gives NumReads back bit for bit."""
    alpha = np.asarray(alpha, dtype=np.float64); eff = np.asarray(eff_lens, dtype=np.float64)
    if not (len(names) == len(lens) == eff.size == alpha.size):
        raise ValueError("names, lens, eff_lens and alpha differ in length")
    rate = alpha / eff
    tot = float(rate.sum())
    tpm = rate / tot * 1e6 if tot > 0 else np.zeros_like(rate)
    with open(path, "w") as f:
        f.write(QUANT_HEADER + "\n")
        for i, nm in enumerate(names):
            f.write("%s\t%d\t%s\t%s\t%s\n" % (nm, int(lens[i]), repr(float(eff[i])), repr(float(tpm[i])), repr(float(alpha[i]))))


def read_quant(path):
    """the inverse of write_quant: (names, lens int64[], eff_lens float64[], tpm float64[], num_reads float64[])"""
    names, cols = [], ([], [], [], [])
    with open(path) as f:
        if f.readline().rstrip("\n") != QUANT_HEADER:
            raise ValueError("%s: not a quant file (header)" % path)
        for ln, line in enumerate(f, 2):
            w = line.rstrip("\n").split("\t")
            if len(w) != 5:
                raise ValueError("%s:%d: %d fields, 5 expected" % (path, ln, len(w)))
            names.append(w[0]); cols[0].append(int(w[1]))
            for j in (1, 2, 3):
                cols[j].append(float(w[j + 1]))
    return names, np.array(cols[0], dtype=np.int64), np.array(cols[1], dtype=np.float64), np.array(cols[2], dtype=np.float64), np.array(cols[3], dtype=np.float64)


FLD_DEFAULT_MAX_LEN = 1000                                            # QM_FLD_DEFAULT_MAX_LEN
FLD_STATS = ("units", "used", "unmapped", "multi", "not_paired", "same_strand", "out_of_range")


def _fld_lens(lens):
    a = np.asarray(lens)
    if a.size and (a.min() < 0 or a.max() > 0xffffffff):
        raise ValueError("transcript lengths must fit 32 unsigned bits")
    return np.ascontiguousarray(a, dtype=np.uint32)


def eff_lens_from_counts(counts, lens):
    """qm_fld_eff_lens_from_counts, a pure host function: effective lengths float64[len(lens)] from a fragment-length histogram
    counts uint64[max_len + 1] -- e = L + 1 - (mean of the fragment lengths up to min(L, max_len)), e = L where there are none"""
    counts = np.ascontiguousarray(counts, dtype=np.uint64); lens = _fld_lens(lens)
    eff = np.zeros(lens.size, dtype=np.float64)
    _check(lib().qm_fld_eff_lens_from_counts(int(counts.size) - 1, counts.ctypes.data if counts.size else None, int(lens.size),
                                             lens.ctypes.data if lens.size else None, eff.ctypes.data if lens.size else None))
    return eff


def frag_len_mean(counts):
    """Q / P over all bins of a histogram: the mean fragment length, nan when it is empty"""
    c = [int(x) for x in np.asarray(counts, dtype=np.uint64)]
    p = sum(c[1:]); q = sum(l * c[l] for l in range(1, len(c)))
    return q / p if p else float("nan")


def write_flen_dist(path, counts):
    """one line of max_len + 1 tab-separated values count[l] / used, %.17g (every value 0 when nothing was used)"""
    c = np.asarray(counts, dtype=np.uint64)
    used = int(c.sum())
    with open(path, "w") as f:
        f.write("\t".join("%.17g" % (int(x) / used if used else 0.0) for x in c) + "\n")


def read_flen_dist(path):
    """the inverse of write_flen_dist: float64[max_len + 1]"""
    with open(path) as f:
        return np.array([float(x) for x in f.readline().rstrip("\n").split("\t")], dtype=np.float64)


class FragLenDist(_Object):
    """qm_fld_*: a histogram fragment length -> fragments in the device memory of a mapper's GPU.  add(mapper) folds the mapper's
    last result where it lies; add_hits folds arrays held on the host through the same kernel; add_counts adds another histogram's
    counts (the merge primitive, and the way to a prior).  Only a unit with exactly one hit that is properly paired, on opposite
    strands and of 1 .. max_len bases counts; stat() tells where the others went.  max_blocks: at most that many workgroups per
    fold (0: as many as are resident)."""

    STATS = FLD_STATS + ("max_len", "folds", "last_fold_us")
    DESTROY, STAT = "qm_fld_destroy", "qm_fld_stat"

    def stat(self):
        """qm_fld_stat: a dictionary of STATS (the six categories add up to units; last_fold_us: the last fold's kernel by HIP events)"""
        return super().stat()

    def __init__(self, mapper, max_len=FLD_DEFAULT_MAX_LEN, max_blocks=0):
        self._h = C.c_void_p()
        if not 0 <= int(max_blocks) <= 0xffff:
            raise ValueError("max_blocks must be 0 .. 65535")
        _check(lib().qm_fld_create(mapper._h, int(max_len), int(max_blocks), C.byref(self._h)))
        self.device = mapper.device
        self.max_len = int(max_len)

    def add(self, mapper):
        """fold the result of the mapper's last map call"""
        _check(lib().qm_fld_add(self._h, mapper._h))

    def add_hits(self, hit_offsets, hits):
        n, hit_offsets, hits = _host_hits(hit_offsets, hits)
        _check(lib().qm_fld_add_hits(self._h, n, hit_offsets.ctypes.data, hits.ctypes.data if hits.size else None))

    def add_counts(self, counts):
        counts = np.ascontiguousarray(counts, dtype=np.uint64)
        if counts.size != self.max_len + 1:
            raise ValueError("max_len + 1 counts")
        _check(lib().qm_fld_add_counts(self._h, counts.ctypes.data))

    def counts(self):
        """uint64[max_len + 1]; bin 0 is never used"""
        c = np.zeros(self.max_len + 1, dtype=np.uint64)
        _check(lib().qm_fld_fetch(self._h, c.ctypes.data))
        return c

    def eff_lens(self, lens):
        """qm_fld_eff_lens: effective lengths float64[len(lens)] from the histogram as it stands"""
        lens = _fld_lens(lens)
        eff = np.zeros(lens.size, dtype=np.float64)
        _check(lib().qm_fld_eff_lens(self._h, int(lens.size), lens.ctypes.data if lens.size else None, eff.ctypes.data if lens.size else None))
        return eff

    def mean(self):
        return frag_len_mean(self.counts())

    def clear(self):
        _check(lib().qm_fld_clear(self._h))


GCB_BINS = 25                                                         # QM_GCB_BINS
GCB_STATS = ("units", "used", "unmapped", "multi", "not_paired", "same_strand", "out_of_range", "overhang")


def gc_eff_lens_from_counts(counts, lens, H, alpha, obs):
    """qm_gcb_eff_lens_from_counts, a pure host function: (eff float64[T], exp float64[25], ratio float64[25]) from the
    fragment-length histogram counts uint64[max_len + 1], the expected matrix H uint64[T][25], a first estimate alpha float64[T]
    and the observed histogram obs uint64[25] -- the arithmetic of include/qmap_mi355.h, nothing fused"""
    counts = np.ascontiguousarray(counts, dtype=np.uint64); lens = _fld_lens(lens)
    H = np.ascontiguousarray(H, dtype=np.uint64); alpha = np.ascontiguousarray(alpha, dtype=np.float64); obs = np.ascontiguousarray(obs, dtype=np.uint64)
    if H.size != lens.size * GCB_BINS or alpha.size != lens.size or obs.size != GCB_BINS:
        raise ValueError("H must be [len(lens)][%d], alpha [len(lens)], obs [%d]" % (GCB_BINS, GCB_BINS))
    eff = np.zeros(lens.size, dtype=np.float64); ex = np.zeros(GCB_BINS, dtype=np.float64); ratio = np.zeros(GCB_BINS, dtype=np.float64)
    some = lens.size > 0
    _check(lib().qm_gcb_eff_lens_from_counts(int(counts.size) - 1, counts.ctypes.data if counts.size else None, int(lens.size),
                                             lens.ctypes.data if some else None, H.ctypes.data if some else None, alpha.ctypes.data if some else None,
                                             obs.ctypes.data, eff.ctypes.data if some else None, ex.ctypes.data, ratio.ctypes.data))
    return eff, ex, ratio


class GCBias(_Object):
    """qm_gcb_*: the fragment GC bias model in the device memory of a mapper's GPU.  add(mapper) sweeps the mapper's last result where
    it lies, add_hits sweeps arrays held on the host through the same kernel, add_counts adds another object's observed counts (the
    merge primitive): a unit with exactly one hit that is properly paired, on opposite strands, of 1 .. max_len bases and lying on
    its transcript counts in the bin of its window's GC fraction; stat() tells where the others went.  expect(counts) is the same
    count over every window of every transcript, weighted by a fragment-length histogram; window_gc probes the rank structure.
    max_blocks: at most that many workgroups per launch (0: as many as are resident)."""

    STATS = GCB_STATS + ("max_len", "folds", "last_fold_us", "last_expect_us", "rank_build_us")
    DESTROY, STAT = "qm_gcb_destroy", "qm_gcb_stat"

    def stat(self):
        """qm_gcb_stat: a dictionary of STATS (the seven categories add up to units; the times by HIP events)"""
        return super().stat()

    def __init__(self, mapper, max_len=FLD_DEFAULT_MAX_LEN, max_blocks=0):
        self._h = C.c_void_p()
        if not 0 <= int(max_blocks) <= 0xffff:
            raise ValueError("max_blocks must be 0 .. 65535")
        _check(lib().qm_gcb_create(mapper._h, int(max_len), int(max_blocks), C.byref(self._h)))
        self.device = mapper.device
        self.max_len = int(max_len)

    def add(self, mapper):
        """sweep the result of the mapper's last map call"""
        _check(lib().qm_gcb_add(self._h, mapper._h))

    def add_hits(self, hit_offsets, hits):
        n, hit_offsets, hits = _host_hits(hit_offsets, hits)
        _check(lib().qm_gcb_add_hits(self._h, n, hit_offsets.ctypes.data, hits.ctypes.data if hits.size else None))

    def add_counts(self, obs):
        obs = np.ascontiguousarray(obs, dtype=np.uint64)
        if obs.size != GCB_BINS:
            raise ValueError("%d counts" % GCB_BINS)
        _check(lib().qm_gcb_add_counts(self._h, obs.ctypes.data))

    def counts(self):
        """the observed histogram, uint64[25]"""
        c = np.zeros(GCB_BINS, dtype=np.uint64)
        _check(lib().qm_gcb_fetch(self._h, c.ctypes.data))
        return c

    def expect(self, counts, n_txps):
        """qm_gcb_expect: the expected matrix uint64[n_txps][25] of a fragment-length histogram counts uint64[max_len + 1]"""
        counts = np.ascontiguousarray(counts, dtype=np.uint64)
        if counts.size != self.max_len + 1:
            raise ValueError("max_len + 1 counts")
        H = np.zeros((int(n_txps), GCB_BINS), dtype=np.uint64)
        _check(lib().qm_gcb_expect(self._h, counts.ctypes.data, int(n_txps), H.ctypes.data if H.size else None))
        return H

    def window_gc(self, tids, starts, lens):
        """qm_gcb_window_gc: int32[n], the G / C characters of transcript tids[i] in [starts[i], starts[i] + lens[i]); -1 where the
        window is empty or does not lie on the transcript"""
        tids = np.ascontiguousarray(tids, dtype=np.uint32); starts = np.ascontiguousarray(starts, dtype=np.int32); lens = np.ascontiguousarray(lens, dtype=np.int32)
        if not tids.size == starts.size == lens.size:
            raise ValueError("tids, starts and lens must be of one length")
        out = np.zeros(tids.size, dtype=np.int32)
        if tids.size:
            _check(lib().qm_gcb_window_gc(self._h, int(tids.size), tids.ctypes.data, starts.ctypes.data, lens.ctypes.data, out.ctypes.data))
        return out

    def clear(self):
        _check(lib().qm_gcb_clear(self._h))


def write_gc_bias(path, obs, exp, ratio):
    """FILE.gcBias.txt: a header line, then per bin `bin<TAB>obs<TAB>exp<TAB>ratio` -- obs an integer, exp and ratio %.17g (every double
    comes back bit for bit)"""
    with open(path, "w") as f:
        f.write("bin\tobs\texp\tratio\n")
        for b in range(GCB_BINS):
            f.write("%d\t%d\t%.17g\t%.17g\n" % (b, int(obs[b]), float(exp[b]), float(ratio[b])))


def read_gc_bias(path):
    """the inverse of write_gc_bias: (obs uint64[25], exp float64[25], ratio float64[25])"""
    obs = np.zeros(GCB_BINS, dtype=np.uint64); ex = np.zeros(GCB_BINS, dtype=np.float64); ratio = np.zeros(GCB_BINS, dtype=np.float64)
    with open(path) as f:
        if f.readline().rstrip("\n").split("\t") != ["bin", "obs", "exp", "ratio"]:
            raise ValueError("%s: not a gcBias file" % path)
        for b in range(GCB_BINS):
            w = f.readline().rstrip("\n").split("\t")
            if len(w) != 4 or int(w[0]) != b:
                raise ValueError("%s: line %d" % (path, b + 2))
            obs[b] = int(w[1]); ex[b] = float(w[2]); ratio[b] = float(w[3])
    return obs, ex, ratio


SQB_BINS = 1152                                                       # QM_SQB_BINS: [2 ends][9 positions][64 words]
SQB_SHAPE = (2, 9, 64)
SQB_STATS = ("units", "used", "unmapped", "multi", "not_paired", "same_strand", "out_of_range", "overhang", "ambiguous")


def seq_bias_weights(alpha, lens, counts):
    """qm_sqb_weights, a pure host function: (q uint64[T], k) -- the integer weights q_t = floor(rho_t * 2^k) of the expected counts from
    a first estimate alpha float64[T], the transcript lengths and the fragment-length histogram counts uint64[max_len + 1]"""
    counts = np.ascontiguousarray(counts, dtype=np.uint64); lens = _fld_lens(lens); alpha = np.ascontiguousarray(alpha, dtype=np.float64)
    if alpha.size != lens.size:
        raise ValueError("alpha must be [len(lens)]")
    q = np.zeros(lens.size, dtype=np.uint64); k = C.c_int32(0)
    some = lens.size > 0
    _check(lib().qm_sqb_weights(int(counts.size) - 1, counts.ctypes.data if counts.size else None, int(lens.size), lens.ctypes.data if some else None,
                                alpha.ctypes.data if some else None, q.ctypes.data if some else None, C.byref(k)))
    return q, int(k.value)


def seq_bias_ratios(obs, exp):
    """qm_sqb_ratios, a pure host function: R float64[2][9][64] from the observed and the expected counts, uint64[2][9][64] each"""
    obs = np.ascontiguousarray(obs, dtype=np.uint64).ravel(); exp = np.ascontiguousarray(exp, dtype=np.uint64).ravel()
    if obs.size != SQB_BINS or exp.size != SQB_BINS:
        raise ValueError("%d counts each" % SQB_BINS)
    R = np.zeros(SQB_BINS, dtype=np.float64)
    _check(lib().qm_sqb_ratios(obs.ctypes.data, exp.ctypes.data, R.ctypes.data))
    return R.reshape(SQB_SHAPE)


class SeqBias(_Object):
    """qm_sqb_*: the sequence-specific bias model in the device memory of a mapper's GPU.  add(mapper) sweeps the mapper's last result
    where it lies, add_hits sweeps arrays held on the host through the same kernel, add_counts adds another object's observed counts:
    a unit with exactly one hit that is properly paired, on opposite strands, of 1 .. max_len bases, whose two nine-character end
    contexts lie on its transcript and hold A, C, G, T only, counts once in each of its 18 words; stat() tells where the others went.
    expect(counts, n_txps, q) is the same count over every place of every transcript a fragment could start or end at, weighted;
    eff_lens(counts, n_txps, R) the effective lengths under a table of ratios; context probes single contexts.
    max_blocks: at most that many workgroups per launch (0: as many as are resident)."""

    STATS = SQB_STATS + ("max_len", "folds", "last_fold_us", "last_expect_us", "last_efflen_us")
    DESTROY, STAT = "qm_sqb_destroy", "qm_sqb_stat"

    def __init__(self, mapper, max_len=FLD_DEFAULT_MAX_LEN, max_blocks=0):
        self._h = C.c_void_p()
        if not 0 <= int(max_blocks) <= 0xffff:
            raise ValueError("max_blocks must be 0 .. 65535")
        _check(lib().qm_sqb_create(mapper._h, int(max_len), int(max_blocks), C.byref(self._h)))
        self.device = mapper.device
        self.max_len = int(max_len)

    def add(self, mapper):
        """sweep the result of the mapper's last map call"""
        _check(lib().qm_sqb_add(self._h, mapper._h))

    def add_hits(self, hit_offsets, hits):
        n, hit_offsets, hits = _host_hits(hit_offsets, hits)
        _check(lib().qm_sqb_add_hits(self._h, n, hit_offsets.ctypes.data, hits.ctypes.data if hits.size else None))

    def add_counts(self, obs):
        obs = np.ascontiguousarray(obs, dtype=np.uint64).ravel()
        if obs.size != SQB_BINS:
            raise ValueError("%d counts" % SQB_BINS)
        _check(lib().qm_sqb_add_counts(self._h, obs.ctypes.data))

    def counts(self):
        """the observed counts, uint64[2][9][64]"""
        c = np.zeros(SQB_BINS, dtype=np.uint64)
        _check(lib().qm_sqb_fetch(self._h, c.ctypes.data))
        return c.reshape(SQB_SHAPE)

    def expect(self, counts, n_txps, q):
        """qm_sqb_expect: the expected counts uint64[2][9][64] of a fragment-length histogram counts uint64[max_len + 1] and weights q uint64[n_txps]"""
        counts = np.ascontiguousarray(counts, dtype=np.uint64); q = np.ascontiguousarray(q, dtype=np.uint64)
        if counts.size != self.max_len + 1 or q.size != int(n_txps):
            raise ValueError("max_len + 1 counts and n_txps weights")
        ex = np.zeros(SQB_BINS, dtype=np.uint64)
        _check(lib().qm_sqb_expect(self._h, counts.ctypes.data, int(n_txps), q.ctypes.data if q.size else None, ex.ctypes.data))
        return ex.reshape(SQB_SHAPE)

    def eff_lens(self, counts, n_txps, R):
        """qm_sqb_eff_lens: the effective lengths float64[n_txps] under the ratios R float64[2][9][64]"""
        counts = np.ascontiguousarray(counts, dtype=np.uint64); R = np.ascontiguousarray(R, dtype=np.float64).ravel()
        if counts.size != self.max_len + 1 or R.size != SQB_BINS:
            raise ValueError("max_len + 1 counts and %d ratios" % SQB_BINS)
        eff = np.zeros(int(n_txps), dtype=np.float64)
        _check(lib().qm_sqb_eff_lens(self._h, counts.ctypes.data, int(n_txps), R.ctypes.data, eff.ctypes.data if eff.size else None))
        return eff

    def context(self, tids, positions, ends):
        """qm_sqb_context: int32[n][9], the nine words of the context of end ends[i] (0: 5', 1: 3') at positions[i] of transcript tids[i];
        a row of -1 where the context does not lie on the transcript or holds a character that is not A, C, G, T"""
        tids = np.ascontiguousarray(tids, dtype=np.uint32); positions = np.ascontiguousarray(positions, dtype=np.int32); ends = np.ascontiguousarray(ends, dtype=np.int32)
        if not tids.size == positions.size == ends.size:
            raise ValueError("tids, positions and ends must be of one length")
        out = np.zeros((tids.size, 9), dtype=np.int32)
        if tids.size:
            _check(lib().qm_sqb_context(self._h, int(tids.size), tids.ctypes.data, positions.ctypes.data, ends.ctypes.data, out.ctypes.data))
        return out

    def clear(self):
        _check(lib().qm_sqb_clear(self._h))


def write_seq_bias(path, obs, exp, ratio):
    """FILE.seqBias.txt: a header line, then per entry `end<TAB>position<TAB>word<TAB>obs<TAB>exp<TAB>ratio` -- obs and exp integers, ratio
    %.17g (every double comes back bit for bit)"""
    obs = np.asarray(obs).reshape(SQB_SHAPE); exp = np.asarray(exp).reshape(SQB_SHAPE); ratio = np.asarray(ratio).reshape(SQB_SHAPE)
    with open(path, "w") as f:
        f.write("end\tposition\tword\tobs\texp\tratio\n")
        for e in range(2):
            for j in range(9):
                for w in range(64):
                    f.write("%d\t%d\t%d\t%d\t%d\t%.17g\n" % (e, j, w, int(obs[e, j, w]), int(exp[e, j, w]), float(ratio[e, j, w])))


def read_seq_bias(path):
    """the inverse of write_seq_bias: (obs uint64[2][9][64], exp uint64[2][9][64], ratio float64[2][9][64])"""
    obs = np.zeros(SQB_SHAPE, dtype=np.uint64); ex = np.zeros(SQB_SHAPE, dtype=np.uint64); ratio = np.zeros(SQB_SHAPE, dtype=np.float64)
    with open(path) as f:
        if f.readline().rstrip("\n").split("\t") != ["end", "position", "word", "obs", "exp", "ratio"]:
            raise ValueError("%s: not a seqBias file" % path)
        for i in range(SQB_BINS):
            w = f.readline().rstrip("\n").split("\t")
            e, j, k = i // 576, (i // 64) % 9, i % 64
            if len(w) != 6 or (int(w[0]), int(w[1]), int(w[2])) != (e, j, k):
                raise ValueError("%s: line %d" % (path, i + 2))
            obs[e, j, k] = int(w[3]); ex[e, j, k] = int(w[4]); ratio[e, j, k] = float(w[5])
    return obs, ex, ratio


PSB_BINS = 200                                                        # QM_PSB_BINS: [2 ends][5 length classes][20 bins]
PSB_SHAPE = (2, 5, 20)
PSB_STATS = ("units", "used", "unmapped", "multi", "not_paired", "same_strand", "out_of_range", "overhang")


def pos_bias_ratios(obs, exp):
    """qm_psb_ratios, a pure host function: R float64[2][5][20] from the observed and the expected counts, uint64[2][5][20] each"""
    obs = np.ascontiguousarray(obs, dtype=np.uint64).ravel(); exp = np.ascontiguousarray(exp, dtype=np.uint64).ravel()
    if obs.size != PSB_BINS or exp.size != PSB_BINS:
        raise ValueError("%d counts each" % PSB_BINS)
    R = np.zeros(PSB_BINS, dtype=np.float64)
    _check(lib().qm_psb_ratios(obs.ctypes.data, exp.ctypes.data, R.ctypes.data))
    return R.reshape(PSB_SHAPE)


class PosBias(_Object):
    """qm_psb_*: the positional bias model in the device memory of a mapper's GPU.  add(mapper) sweeps the mapper's last result where it
    lies, add_hits sweeps arrays held on the host through the same kernel, add_counts adds another object's observed counts: a unit
    with exactly one hit that is properly paired, on opposite strands, of 1 .. max_len bases and on its transcript counts once in the
    bin of its start and once in the bin of its last position, in the class of its transcript's length; stat() tells where the others
    went.  expect(counts, n_txps, q) is the same count over every place of every transcript a fragment could start or end at,
    weighted (q: seq_bias_weights); eff_lens(counts, n_txps, R) the effective lengths under a table of ratios; position probes single
    positions.  max_blocks: at most that many workgroups per launch (0: as many as are resident)."""

    STATS = PSB_STATS + ("max_len", "folds", "last_fold_us", "last_expect_us", "last_efflen_us")
    DESTROY, STAT = "qm_psb_destroy", "qm_psb_stat"

    def __init__(self, mapper, max_len=FLD_DEFAULT_MAX_LEN, max_blocks=0):
        self._h = C.c_void_p()
        if not 0 <= int(max_blocks) <= 0xffff:
            raise ValueError("max_blocks must be 0 .. 65535")
        _check(lib().qm_psb_create(mapper._h, int(max_len), int(max_blocks), C.byref(self._h)))
        self.device = mapper.device
        self.max_len = int(max_len)

    def add(self, mapper):
        """sweep the result of the mapper's last map call"""
        _check(lib().qm_psb_add(self._h, mapper._h))

    def add_hits(self, hit_offsets, hits):
        n, hit_offsets, hits = _host_hits(hit_offsets, hits)
        _check(lib().qm_psb_add_hits(self._h, n, hit_offsets.ctypes.data, hits.ctypes.data if hits.size else None))

    def add_counts(self, obs):
        obs = np.ascontiguousarray(obs, dtype=np.uint64).ravel()
        if obs.size != PSB_BINS:
            raise ValueError("%d counts" % PSB_BINS)
        _check(lib().qm_psb_add_counts(self._h, obs.ctypes.data))

    def counts(self):
        """the observed counts, uint64[2][5][20]"""
        c = np.zeros(PSB_BINS, dtype=np.uint64)
        _check(lib().qm_psb_fetch(self._h, c.ctypes.data))
        return c.reshape(PSB_SHAPE)

    def expect(self, counts, n_txps, q):
        """qm_psb_expect: the expected counts uint64[2][5][20] of a fragment-length histogram counts uint64[max_len + 1] and weights q uint64[n_txps]"""
        counts = np.ascontiguousarray(counts, dtype=np.uint64); q = np.ascontiguousarray(q, dtype=np.uint64)
        if counts.size != self.max_len + 1 or q.size != int(n_txps):
            raise ValueError("max_len + 1 counts and n_txps weights")
        ex = np.zeros(PSB_BINS, dtype=np.uint64)
        _check(lib().qm_psb_expect(self._h, counts.ctypes.data, int(n_txps), q.ctypes.data if q.size else None, ex.ctypes.data))
        return ex.reshape(PSB_SHAPE)

    def eff_lens(self, counts, n_txps, R):
        """qm_psb_eff_lens: the effective lengths float64[n_txps] under the ratios R float64[2][5][20]"""
        counts = np.ascontiguousarray(counts, dtype=np.uint64); R = np.ascontiguousarray(R, dtype=np.float64).ravel()
        if counts.size != self.max_len + 1 or R.size != PSB_BINS:
            raise ValueError("max_len + 1 counts and %d ratios" % PSB_BINS)
        eff = np.zeros(int(n_txps), dtype=np.float64)
        _check(lib().qm_psb_eff_lens(self._h, counts.ctypes.data, int(n_txps), R.ctypes.data, eff.ctypes.data if eff.size else None))
        return eff

    def position(self, tids, positions):
        """qm_psb_position: int32[n][2], the class of transcript tids[i] and the bin of positions[i] on it; a row of -1 where there is no
        such transcript or the position does not lie on it"""
        tids = np.ascontiguousarray(tids, dtype=np.uint32); positions = np.ascontiguousarray(positions, dtype=np.int32)
        if tids.size != positions.size:
            raise ValueError("tids and positions must be of one length")
        out = np.zeros((tids.size, 2), dtype=np.int32)
        if tids.size:
            _check(lib().qm_psb_position(self._h, int(tids.size), tids.ctypes.data, positions.ctypes.data, out.ctypes.data))
        return out

    def clear(self):
        _check(lib().qm_psb_clear(self._h))


def write_pos_bias(path, obs, exp, ratio):
    """FILE.posBias.txt: a header line, then per entry `end<TAB>class<TAB>bin<TAB>obs<TAB>exp<TAB>ratio` -- obs and exp integers, ratio
    %.17g (every double comes back bit for bit)"""
    obs = np.asarray(obs).reshape(PSB_SHAPE); exp = np.asarray(exp).reshape(PSB_SHAPE); ratio = np.asarray(ratio).reshape(PSB_SHAPE)
    with open(path, "w") as f:
        f.write("end\tclass\tbin\tobs\texp\tratio\n")
        for e in range(2):
            for c in range(5):
                for b in range(20):
                    f.write("%d\t%d\t%d\t%d\t%d\t%.17g\n" % (e, c, b, int(obs[e, c, b]), int(exp[e, c, b]), float(ratio[e, c, b])))


def read_pos_bias(path):
    """the inverse of write_pos_bias: (obs uint64[2][5][20], exp uint64[2][5][20], ratio float64[2][5][20])"""
    obs = np.zeros(PSB_SHAPE, dtype=np.uint64); ex = np.zeros(PSB_SHAPE, dtype=np.uint64); ratio = np.zeros(PSB_SHAPE, dtype=np.float64)
    with open(path) as f:
        if f.readline().rstrip("\n").split("\t") != ["end", "class", "bin", "obs", "exp", "ratio"]:
            raise ValueError("%s: not a posBias file" % path)
        for i in range(PSB_BINS):
            w = f.readline().rstrip("\n").split("\t")
            e, c, b = i // 100, (i // 20) % 5, i % 20
            if len(w) != 6 or (int(w[0]), int(w[1]), int(w[2])) != (e, c, b):
                raise ValueError("%s: line %d" % (path, i + 2))
            obs[e, c, b] = int(w[3]); ex[e, c, b] = int(w[4]); ratio[e, c, b] = float(w[5])
    return obs, ex, ratio


LIB_TYPES = ("IU", "ISF", "ISR", "OU", "OSF", "OSR", "MU", "MSF", "MSR", "U", "SF", "SR", "A")
LIB_CODES = ("ISF", "ISR", "OSF", "OSR", "MSF", "MSR", "LF", "LR", "RF", "RR", "SF", "SR")    # a hit's code: words 0 .. 11 of a tally
LIB_TOTALS = ("units", "unmapped_units", "kept_units", "dropped_units", "hits", "kept_hits")  # words 24 .. 29; word 30: other_hits
LIB_ALL_CODES = 0xfff


def lib_type_mask(name):
    """qm_lib_type_mask, a pure host function: the 12-bit mask over the codes of a library type name (LIB_TYPES)"""
    m = C.c_uint32()
    _check(lib().qm_lib_type_mask(str(name).encode(), C.byref(m)))
    return m.value


def _lib_counts(counts):
    c = np.ascontiguousarray(counts, dtype=np.uint64)
    if c.size != 32:
        raise ValueError("a tally has 32 words")
    return c


def infer_lib_type(counts):
    """qm_lib_infer, a pure host function: the type the single-hit units of a tally (words 12 .. 23) point to -- the orientation with
    the most of them, stranded when more than 70 % agree -- or "" without any"""
    c = _lib_counts(counts)
    out = C.create_string_buffer(4)
    _check(lib().qm_lib_infer(c.ctypes.data, out))
    return out.value.decode()


def lib_format_counts(counts, lib_type):
    """the dictionary write_lib_format_counts writes"""
    c = [int(x) for x in _lib_counts(counts)]
    inferred = infer_lib_type(counts)
    kept, dropped = c[26], c[27]
    d = {"expected_format": inferred if lib_type == "A" else str(lib_type), "inferred_format": inferred,
         "compatible_fragment_ratio": kept / (kept + dropped) if kept + dropped else 0.0}
    d.update(zip(LIB_TOTALS, c[24:30]))
    d["other_hits"] = c[30]
    d["hits_by_code"] = dict(zip(LIB_CODES, c[:12]))
    d["single_hit_units_by_code"] = dict(zip(LIB_CODES, c[12:24]))
    return d


def write_lib_format_counts(path, counts, lib_type):
    """FILE.lib_format_counts.json: the twelve hit counts and the twelve single-hit counts by code name, the totals, expected_format
    (the given type; under A the inferred one), inferred_format and compatible_fragment_ratio = kept / (kept + dropped) units"""
    import json
    with open(path, "w") as f:
        json.dump(lib_format_counts(counts, lib_type), f, indent=2)
        f.write("\n")


def read_lib_format_counts(path):
    """the inverse of write_lib_format_counts: (counts uint64[32], the dictionary)"""
    import json
    with open(path) as f:
        d = json.load(f)
    c = np.zeros(32, dtype=np.uint64)
    c[:12] = [d["hits_by_code"][k] for k in LIB_CODES]; c[12:24] = [d["single_hit_units_by_code"][k] for k in LIB_CODES]
    c[24:30] = [d[k] for k in LIB_TOTALS]; c[30] = d["other_hits"]
    return c, d


class LibFormat(_Object):
    """qm_lib_*: the tallies of a library type in the device memory of a mapper's GPU.  Every hit record has an orientation code
    (LIB_CODES; include/qmap_mi355.h has the table); lib_type names the codes that are compatible (LIB_TYPES, or a 12-bit mask; "A":
    all of them, nothing is dropped).  add(mapper) tallies the mapper's last result where it lies, add_hits arrays held on the host
    through the same sweep, compact_hits also brings the filtered lists back, add_counts adds another tally (the merge primitive);
    EqClasses.add(mapper, lib=...) folds the compatible hits only.  max_blocks: at most that many workgroups per sweep (0: as many
    as are resident)."""

    STATS = ("sweeps", "last_sweep_us", "mask")
    DESTROY, STAT = "qm_lib_destroy", "qm_lib_stat"

    def stat(self):
        """qm_lib_stat: a dictionary of STATS (last_sweep_us: the last sweep by HIP events)"""
        return super().stat()

    def __init__(self, mapper, lib_type="A", max_blocks=0):
        self._h = C.c_void_p()
        if not 0 <= int(max_blocks) <= 0xffff:
            raise ValueError("max_blocks must be 0 .. 65535")
        self.mask = lib_type_mask(lib_type) if isinstance(lib_type, str) else int(lib_type)
        self.lib_type = lib_type
        _check(lib().qm_lib_create(mapper._h, self.mask & 0xffffffff, int(max_blocks), C.byref(self._h)))
        self.device = mapper.device

    def add(self, mapper):
        """tally the result of the mapper's last map call"""
        _check(lib().qm_lib_add(self._h, mapper._h))

    def add_hits(self, hit_offsets, hits):
        n, hit_offsets, hits = _host_hits(hit_offsets, hits)
        _check(lib().qm_lib_add_hits(self._h, n, hit_offsets.ctypes.data, hits.ctypes.data if hits.size else None))

    def compact_hits(self, hit_offsets, hits):
        """add_hits, and the filtered lists: (new_offsets int64[n + 1], tids uint32[]) -- every unit's kept hits, in their order"""
        n, hit_offsets, hits = _host_hits(hit_offsets, hits)
        new_off = np.zeros(n + 1, dtype=np.int64); tids = np.zeros((int(hit_offsets[-1] - hit_offsets[0]) if n else 0) + 1, dtype=np.uint32)
        _check(lib().qm_lib_compact_hits(self._h, n, hit_offsets.ctypes.data, hits.ctypes.data if hits.size else None, new_off.ctypes.data, tids.ctypes.data))
        return new_off, tids[:int(new_off[-1])].copy()

    def add_counts(self, counts):
        c = _lib_counts(counts)
        _check(lib().qm_lib_add_counts(self._h, c.ctypes.data))

    def counts(self):
        """uint64[32]: hits by code, single-hit units by code, then units, unmapped, kept, dropped, hits, kept hits, other hits, 0"""
        c = np.zeros(32, dtype=np.uint64)
        _check(lib().qm_lib_fetch(self._h, c.ctypes.data))
        return c

    def clear(self):
        _check(lib().qm_lib_clear(self._h))


PACK_EXC_DTYPE = np.dtype([("pos", "<u4"), ("ch", "<u4")])


def pinned_copy(a):
    """a copy of the array in page-locked host memory (qm_pinned_alloc; kept for the life of the process): DMA source of the host-buffer calls"""
    a = np.ascontiguousarray(a)
    p = lib().qm_pinned_alloc(max(64, a.nbytes))
    if not p:
        raise QmError("qm_pinned_alloc(%d) failed" % a.nbytes)
    v = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(max(64, a.nbytes),))[: a.nbytes].view(a.dtype).reshape(a.shape)
    v[...] = a
    return v


def pack_2bit(seq, off):
    """qm_pack_reads: (packed uint8[], off int64[n+1], exceptions {pos, ch}[]) of a batch of reads -- four characters to a byte,
    read i from byte (off[i] >> 2) + i on, everything that is not upper-case A C G T as an exception"""
    seq = np.ascontiguousarray(seq, dtype=np.uint8); off = np.ascontiguousarray(off, dtype=np.int64)
    n = len(off) - 1
    pk = np.zeros((int(off[-1]) >> 2) + n + 8, dtype=np.uint8)
    cap = int(off[-1]) + 16
    exc = np.zeros(cap, dtype=PACK_EXC_DTYPE)
    ne = C.c_int64(0)
    rc = lib().qm_pack_reads(seq.ctypes.data or 1, off.ctypes.data, n, pk.ctypes.data, exc.ctypes.data, cap, C.byref(ne))
    if rc != 0:
        raise QmError(lib().qm_io_last_error().decode())
    return pk, off, exc[: ne.value].copy()


def unpack_2bit(pk, off, exc):
    """the inverse, in numpy (tests): the characters the device's unpack kernels write"""
    off = np.asarray(off, dtype=np.int64); n = len(off) - 1
    out = np.zeros(int(off[-1]), dtype=np.uint8)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    for i in range(n):
        o, e = int(off[i]), int(off[i + 1])
        b = pk[(o >> 2) + i:(o >> 2) + i + (e - o + 3) // 4]
        codes = ((b[:, None] >> (2 * np.arange(4))[None, :]) & 3).reshape(-1)[: e - o]
        out[o:e] = lut[codes]
    out[exc["pos"]] = exc["ch"].astype(np.uint8)
    return out


class _Mem:
    """array-interface carrier: np.asarray(_Mem(...)) is a zero-copy view of foreign memory in a few microseconds
    (np.ctypeslib.as_array builds a new ctypes array type per shape: ~1 ms per view, which at 2^18-pair batches was a third
    of the stream's wall time)"""
    __slots__ = ("__array_interface__",)

    def __init__(self, addr, count, dt):
        self.__array_interface__ = {"data": (addr, False), "shape": (count,), "typestr": dt.str, "version": 3}
        if dt.fields:
            self.__array_interface__["descr"] = dt.descr


def _view(p, count, dt):
    """zero-copy numpy view of `count` elements of dtype dt at the address held by a ctypes pointer / integer"""
    addr = p.value if hasattr(p, "value") else p
    if count == 0 or not addr:
        return np.zeros(0, dtype=dt)
    return np.asarray(_Mem(int(addr), int(count), np.dtype(dt)))


class ReadBatch:
    """one chunk handed out by FastxReader: packed sequences/names (numpy views, valid until the next chunk)"""
    pass


class FastxReader:
    """FASTA/FASTQ(.gz) ingest through the library's native reader (qm_reader_*): the packed batches that
    QuasiMapper.map_pairs / map_reads take.  path2=None for single-end input."""

    def __init__(self, path1, path2=None, threads=None):
        self._h = C.c_void_p()
        rc = lib().qm_reader_open(path1.encode(), path2.encode() if path2 else None,
                                  int(threads or min(16, os.cpu_count() or 1)), C.byref(self._h))
        if rc != 0:
            raise QmError(lib().qm_io_last_error().decode())
        self.paired = path2 is not None

    def chunks(self, max_units):
        L = lib()
        n = C.c_int64()
        ptr = [C.c_void_p() for _ in range(8)]
        while True:
            rc = L.qm_reader_next(self._h, int(max_units), C.byref(n), *[C.byref(x) for x in ptr])
            if rc != 0:
                raise QmError(L.qm_io_last_error().decode())
            if n.value == 0:
                return
            b = ReadBatch(); b.n = n.value

            arr = _view
            b.off1 = arr(ptr[1], b.n + 1, np.int64); b.seq1 = arr(ptr[0], int(b.off1[-1]), np.uint8)
            b.name_off1 = arr(ptr[3], b.n + 1, np.int64); b.names1 = arr(ptr[2], int(b.name_off1[-1]), np.uint8)
            if self.paired:
                b.off2 = arr(ptr[5], b.n + 1, np.int64); b.seq2 = arr(ptr[4], int(b.off2[-1]), np.uint8)
                b.name_off2 = arr(ptr[7], b.n + 1, np.int64); b.names2 = arr(ptr[6], int(b.name_off2[-1]), np.uint8)
            yield b

    def close(self):
        if self._h:
            lib().qm_reader_close(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def reserve_stream_memory(nbytes=512 << 20):
    """qm_stream_reserve: pin the process-wide pool the streams' slots come out of, in the background (returns at once).  Call it
    early -- before the index is uploaded -- so that pinning (5.5 GB/s) runs under other work."""
    _check(lib().qm_stream_reserve(int(nbytes)))


class MappedStream:
    """FASTA/FASTQ files -> mapped batches through the library's pipelined stream (qm_stream_*): ingest workers packing batches
    into pinned slots, two device contexts per device, results in pinned memory.  `device` may be one id or a list of ids
    (consecutive batches go to different devices; batches still come back in input order).  Iterating yields ReadBatch
    objects that also carry hit_offsets / hits / counters / device; every array is a zero-copy view that stays valid until
    the next batch is taken.  names=False: read names are not kept (hits-only callers).  eq_classes=True: every batch is folded
    into equivalence classes on its device (eq_classes() after the last batch); with hits=False on top the hits stay on the
    device -- hit_offsets / hits of a batch are None, n_hits and counters as ever.  frag_len_dist=True: every batch is folded into a
    fragment-length histogram on its device as well (frag_len_dist() after the last batch).  gc_bias=True: every batch is swept into
    the observed counts of the fragment GC bias model as well (gc_bias() after the last batch).  seq_bias=True: ... and into the observed
    counts of the sequence-specific bias model (seq_bias() after the last batch).  pos_bias=True: ... and into those of the positional
    bias model (pos_bias() after the last batch).  lib_type (a name of LIB_TYPES or a
    12-bit mask): every batch is tallied by orientation code on its device (lib_counts() after the last batch), and with
    eq_classes=True the classes hold only the hits that type keeps."""

    def __init__(self, index: QuasiIndex, path1, path2=None, opts=None, device=0, batch_units=1 << 20, threads=None, ph_compact=False,
                 names=True, eq_classes=False, hits=True, frag_len_dist=False, lib_type=None, gc_bias=False, seq_bias=False, pos_bias=False):
        self._h = C.c_void_p()
        self.paired = path2 is not None
        self.names = bool(names)
        self.with_hits = bool(hits)
        self._eqc = bool(eq_classes)
        if not hits and not eq_classes:
            raise ValueError("hits=False needs eq_classes=True")
        opts = opts or default_opts()
        devs = [int(d) for d in device] if isinstance(device, (list, tuple)) else [int(device)]
        self.devices = devs
        darr = (C.c_int32 * len(devs))(*devs)
        rc = lib().qm_stream_open_ex(index._h, darr, len(devs), 1 if ph_compact else 0, C.byref(opts), os.fsencode(path1),
                                     os.fsencode(path2) if path2 else None, int(batch_units),
                                     int(threads or min(32, os.cpu_count() or 1)),
                                     (0 if names else 1) | (2 if eq_classes else 0) | (0 if hits else 4) | (8 if frag_len_dist else 0) | (32 if gc_bias else 0) | (64 if seq_bias else 0) | (128 if pos_bias else 0) |
                                     (0 if lib_type is None else 16 | (lib_type_mask(lib_type) if isinstance(lib_type, str) else int(lib_type)) << 16), C.byref(self._h))
        if rc != 0:
            raise QmError("qm_stream_open failed (%d): %s" % (rc, lib().qm_stream_last_error().decode(errors="replace")))
        self._index = index

    def _call(self, name, *args):
        """lib().<name>(the stream, args...); QmError with qm_stream_last_error when it fails"""
        rc = getattr(lib(), name)(self._h, *args)
        if rc != 0:
            raise QmError("%s failed (%d): %s" % (name, rc, lib().qm_stream_last_error().decode(errors="replace")))

    def __iter__(self):
        sb = QmStreamBatch()

        arr = _view
        while True:
            self._call("qm_stream_next", C.byref(sb))
            if sb.n_units == 0:
                return
            b = ReadBatch(); b.n = n = sb.n_units
            b.off1 = arr(sb.off1, n + 1, np.int64); b.seq1 = arr(sb.seq1, int(b.off1[-1]), np.uint8)
            if self.names:
                b.name_off1 = arr(sb.name_off1, n + 1, np.int64); b.names1 = arr(sb.names1, int(b.name_off1[-1]), np.uint8)
            if self.paired:
                b.off2 = arr(sb.off2, n + 1, np.int64); b.seq2 = arr(sb.seq2, int(b.off2[-1]), np.uint8)
                if self.names:
                    b.name_off2 = arr(sb.name_off2, n + 1, np.int64); b.names2 = arr(sb.names2, int(b.name_off2[-1]), np.uint8)
            b.device = sb.device
            b.n_hits = sb.n_hits
            if self.with_hits:
                b.hit_offsets = arr(sb.hit_offsets, n + 1, np.int64)
                b.hits = arr(sb.hits, sb.n_hits, HIT_DTYPE) if sb.n_hits else np.zeros(0, dtype=HIT_DTYPE)
            else:
                b.hit_offsets = b.hits = None
            b.counters = sb.counters.as_dict()
            b.gpu_ms = sb.gpu_ms
            yield b

    def eq_classes(self):
        """after the last batch: the classes of the whole input, merged over the stream's contexts and devices --
        (label_offsets, tids, counts) as EqClasses.fetch gives them"""
        nc, nt = C.c_int64(), C.c_int64()
        self._call("qm_stream_eqc_finish", C.byref(nc), C.byref(nt))
        off = np.zeros(nc.value + 1, dtype=np.int64); tids = np.zeros(nt.value + 1, dtype=np.uint32); cnt = np.zeros(nc.value + 1, dtype=np.uint64)
        self._call("qm_stream_eqc_fetch", off.ctypes.data, tids.ctypes.data, cnt.ctypes.data)
        return off, tids[:nt.value], cnt[:nc.value]

    def frag_len_dist(self):
        """after the last batch of a stream opened with frag_len_dist=True: (counts uint64[1001], stats) summed over the stream's
        contexts and devices -- stats: a dictionary of units and the six categories (FLD_STATS)"""
        c = np.zeros(FLD_DEFAULT_MAX_LEN + 1, dtype=np.uint64); st = np.zeros(7, dtype=np.int64)
        self._call("qm_stream_fld_fetch", c.ctypes.data, st.ctypes.data)
        return c, dict(zip(FLD_STATS, (int(x) for x in st)))

    def gc_bias(self):
        """after the last batch of a stream opened with gc_bias=True: (obs uint64[25], stats) summed over the stream's contexts and
        devices -- stats: a dictionary of units and the seven categories (GCB_STATS)"""
        c = np.zeros(GCB_BINS, dtype=np.uint64); st = np.zeros(8, dtype=np.int64)
        self._call("qm_stream_gcb_fetch", c.ctypes.data, st.ctypes.data)
        return c, dict(zip(GCB_STATS, (int(x) for x in st)))

    def seq_bias(self):
        """after the last batch of a stream opened with seq_bias=True: (obs uint64[2][9][64], stats) summed over the stream's contexts and
        devices -- stats: a dictionary of units and the eight categories (SQB_STATS)"""
        c = np.zeros(SQB_BINS, dtype=np.uint64); st = np.zeros(9, dtype=np.int64)
        self._call("qm_stream_sqb_fetch", c.ctypes.data, st.ctypes.data)
        return c.reshape(SQB_SHAPE), dict(zip(SQB_STATS, (int(x) for x in st)))

    def pos_bias(self):
        """after the last batch of a stream opened with pos_bias=True: (obs uint64[2][5][20], stats) summed over the stream's contexts and
        devices -- stats: a dictionary of units and the seven categories (PSB_STATS)"""
        c = np.zeros(PSB_BINS, dtype=np.uint64); st = np.zeros(8, dtype=np.int64)
        self._call("qm_stream_psb_fetch", c.ctypes.data, st.ctypes.data)
        return c.reshape(PSB_SHAPE), dict(zip(PSB_STATS, (int(x) for x in st)))

    def lib_counts(self):
        """after the last batch of a stream opened with lib_type: the tallies uint64[32] (LibFormat.counts) summed over the stream's
        contexts and devices"""
        c = np.zeros(32, dtype=np.uint64)
        self._call("qm_stream_lib_fetch", c.ctypes.data)
        return c

    def stats(self):
        """seconds: read_s = open to the last batch packed (wall), map_s / fetch_s = upload + kernels / download summed over the
        contexts, parse_cpu_s / copy_cpu_s = the ingest workers' task time summed over the workers"""
        a = (C.c_double * 19)()
        _check(lib().qm_stream_stats_ex(self._h, a, 19))
        return dict(zip(("read_s", "map_s", "fetch_s", "caller_wait_s", "open_s", "alloc_s", "first_batch_s", "parse_cpu_s", "copy_cpu_s",
                         "inflate_s", "bytes_parsed", "last_mapped_s", "packed_batches", "fold_s", "fold_contexts", "fld_fold_s", "gcb_sweep_s", "sqb_sweep_s", "psb_sweep_s"), [float(x) for x in a]))

    def close(self):
        if self._h:
            lib().qm_stream_close(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _take_buf(p, n):
    try:
        return C.string_at(p, n.value)
    finally:
        lib().qm_buf_free(p)


def sam_header_text(index: "QuasiIndex") -> bytes:
    p = C.c_void_p(); n = C.c_int64()
    _check(lib().qm_sam_header(index._h, C.byref(p), C.byref(n)))
    return _take_buf(p, n)


def _sam_batch_args(batch, hit_offsets, hits):
    ho = np.ascontiguousarray(hit_offsets, dtype=np.int64)
    hh = np.ascontiguousarray(hits)
    paired = getattr(batch, "seq2", None) is not None
    keep = [np.ascontiguousarray(x) for x in (batch.names1, batch.name_off1, batch.seq1, batch.off1)]
    if paired:
        keep += [np.ascontiguousarray(x) for x in (batch.names2, batch.name_off2, batch.seq2, batch.off2)]
    args = [C.c_void_p(a.ctypes.data) for a in keep] + ([C.c_void_p(0)] * 4 if not paired else [])
    if not keep[2].size:                       # a zero-length sequence array still needs a non-null pointer
        args[2] = C.c_void_p(ho.ctypes.data)
    args += [C.c_void_p(ho.ctypes.data), C.c_void_p(hh.ctypes.data if hh.size else ho.ctypes.data)]
    return args, (keep, ho, hh)


class SamWriter:
    """qm_sam_writer_*: SAM records of a run onto one file descriptor; put() formats a batch and returns while the writer's
    own thread writes the previous one."""

    def __init__(self, index: "QuasiIndex", fd, max_num_hits=200, threads=None, gzip=False, level=1):
        """gzip=True: `-x` -- every part of a batch becomes a gzip member compressed by its own worker (a valid .gz stream)"""
        self._h = C.c_void_p()
        self._index = index
        flags = (1 | (int(level) & 15) << 8) if gzip else 0
        rc = lib().qm_sam_writer_open_ex(index._h, int(fd), int(max_num_hits), int(threads or min(16, os.cpu_count() or 1)), flags, C.byref(self._h))
        if rc != 0:
            raise QmError(lib().qm_io_last_error().decode())

    def header(self):
        """the SAM header, through the writer's queue (compressed like the records when gzip=True)"""
        rc = lib().qm_sam_writer_header(self._h)
        if rc != 0:
            raise QmError(lib().qm_io_last_error().decode())

    def put(self, batch, hit_offsets, hits):
        args, keep = _sam_batch_args(batch, hit_offsets, hits)
        rc = lib().qm_sam_writer_put(self._h, int(batch.n), *args)
        if rc != 0:
            raise QmError(lib().qm_io_last_error().decode())

    def close(self):
        """drains the writer; returns the bytes written"""
        if not self._h:
            return 0
        nb = C.c_int64()
        rc = lib().qm_sam_writer_close(self._h, C.byref(nb))
        self._h = C.c_void_p()
        if rc != 0:
            raise QmError(lib().qm_io_last_error().decode())
        return nb.value


def sam_records_text(index: "QuasiIndex", batch, hit_offsets, hits, max_num_hits=200, threads=None, fd=None):
    """SAM records of one mapped ReadBatch (paired when the batch has mates), formatted by the library.
    fd=None: returns the text; otherwise writes it to that file descriptor and returns the byte count."""
    def vp(a):
        return C.c_void_p(np.ascontiguousarray(a).ctypes.data) if a is not None and len(a) else C.c_void_p(0)
    ho = np.ascontiguousarray(hit_offsets, dtype=np.int64)
    hh = np.ascontiguousarray(hits)
    paired = getattr(batch, "seq2", None) is not None
    keep = [np.ascontiguousarray(x) for x in (batch.names1, batch.name_off1, batch.seq1, batch.off1)]
    if paired:
        keep += [np.ascontiguousarray(x) for x in (batch.names2, batch.name_off2, batch.seq2, batch.off2)]
    args = [C.c_void_p(a.ctypes.data) for a in keep] + ([C.c_void_p(0)] * 4 if not paired else [])
    # a zero-length sequence array still needs a non-null pointer
    if not keep[2].size:
        args[2] = C.c_void_p(ho.ctypes.data)
    nthr = int(threads or min(16, os.cpu_count() or 1))
    if fd is not None:
        nb = C.c_int64()
        rc = lib().qm_sam_write(index._h, int(batch.n), *args, C.c_void_p(ho.ctypes.data),
                                C.c_void_p(hh.ctypes.data if hh.size else ho.ctypes.data), int(max_num_hits), nthr, int(fd),
                                C.byref(nb))
        if rc != 0:
            raise QmError(lib().qm_io_last_error().decode())
        return nb.value
    p = C.c_void_p(); n = C.c_int64()
    rc = lib().qm_sam_records(index._h, int(batch.n), *args, C.c_void_p(ho.ctypes.data),
                              C.c_void_p(hh.ctypes.data if hh.size else ho.ctypes.data), int(max_num_hits),
                              int(threads or min(16, os.cpu_count() or 1)), C.byref(p), C.byref(n))
    if rc != 0:
        raise QmError(lib().qm_io_last_error().decode())
    return _take_buf(p, n)
