"""rapmap_amd -- MI355X-native drop-in for the `rapmap quasimap` hot path (RapMap v0.6.0).

Only what the path needs: csrc/ (HIP kernels + the C ABI of include/qmap_mi355.h), api.py (host mirror
of the reference's call surface), synth.py (synthetic transcriptome / reads)."""
from .api import (QuasiIndex, QuasiMapper, QmError, QmOpts, default_opts, build_index, pack_reads,  # noqa: F401
                  FastxReader, ReadBatch, MappedStream, reserve_stream_memory, SamWriter, sam_header_text, sam_records_text,
                  HIT_DTYPE, INTERVAL_DTYPE, LIB_PATH, ABI_SYMBOLS, EqClasses, write_eq_classes, read_eq_classes,
                  Quant, exp_digamma, write_quant, read_quant, Bootstrap, write_bootstraps, read_bootstraps,
                  FragLenDist, GCBias, gc_eff_lens_from_counts, write_gc_bias, read_gc_bias, GCB_BINS, GCB_STATS,
                  SeqBias, seq_bias_weights, seq_bias_ratios, write_seq_bias, read_seq_bias, SQB_BINS, SQB_STATS,
                  PosBias, pos_bias_ratios, write_pos_bias, read_pos_bias, PSB_BINS, PSB_STATS,
                  eff_lens_from_counts, frag_len_mean, write_flen_dist, read_flen_dist, FLD_DEFAULT_MAX_LEN, FLD_STATS,
                  LibFormat, lib_type_mask, infer_lib_type, lib_format_counts, write_lib_format_counts, read_lib_format_counts,
                  LIB_TYPES, LIB_CODES, LIB_TOTALS, LIB_ALL_CODES)
from . import api

# QM_STAT_* and QM_EQC_STAT_*: what QuasiMapper.stat and EqClasses.stat are asked for
globals().update({name: value for name, value in vars(api).items() if name.startswith(("QM_STAT_", "QM_EQC_STAT_"))})
