"""ctypes binding of the gfx950 codec library (include/pgnano_hip.h).

The product path has no CPU fallback: if ``_build/libpgnano_hip.so`` is missing or cannot be
loaded, every entry point raises :class:`NativeLibraryError`.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_build", "libpgnano_hip.so")
# diagnostic build with per-phase shader-clock timers (tools/phase_profile.py)
PROF_LIB_PATH = os.path.join(_HERE, "_build", "libpgnano_hip_prof.so")

PGN_OK = 0
PGN_ERR_DST_TOO_SMALL = 1
PGN_ERR_NOT_ZSTD = 2
PGN_ERR_ZSTD_DECOMPRESS = 3
PGN_ERR_REMAINING = 4
PGN_ERR_ZSTD_COMPRESS = 5
PGN_ERR_CORRUPT = 6
PGN_ERR_UNSUPPORTED = 9
PGN_ERR_INVALID_ARG = 10
PGN_ERR_HIP = 11
PGN_ERR_NO_DEVICE = 12
PGN_ERR_IO = 13

PGN_POD5_CODEC_VBZ = 100  # include/pgnano_pod5.h
PGN_MAX_CHUNK_SAMPLES = 16777216
# pgn_variant: the reference's compile-time COMPRESSOR_* variants (pgnano.cpp:70-92)
VARIANTS = {"C5": 0, "C4": 1, "C1": 2, "C2": 3, "C3": 4, "VBZ0": 5}
PGN_STATS_PER_CHUNK = 10
# pgn_out_type: the element type of pgn_decompress_batch_device_pa's output
PGN_OUT_INT16, PGN_OUT_F32, PGN_OUT_F16 = 0, 1, 2

# pgn_norm_mode and the two structs of the per-read normalisation calls
PGN_NORM_QUANTILE, PGN_NORM_MEDMAD = 0, 1
NORM_MODES = {"quantile": PGN_NORM_QUANTILE, "medmad": PGN_NORM_MEDMAD}


class NormParams(C.Structure):
    """pgn_norm_params"""
    _fields_ = [("mode", C.c_int32), ("pad", C.c_int32), ("p_lo", C.c_double), ("p_hi", C.c_double),
                ("centre_mult", C.c_float), ("spread_mult", C.c_float), ("spread_floor", C.c_float), ("pad2", C.c_float)]


class ReadStats(C.Structure):
    """pgn_read_stats"""
    _fields_ = [("n", C.c_uint64), ("status", C.c_int32), ("q_lo", C.c_int16), ("q_hi", C.c_int16), ("m2", C.c_int32),
                ("mad4", C.c_uint32), ("centre", C.c_float), ("spread", C.c_float)]


PGN_SELECT_MAX_PARTS = 4096


class SelectSplit(C.Structure):
    """pgn_select_split"""
    _fields_ = [("split_min_samples", C.c_uint32), ("part_samples", C.c_uint32), ("max_split_reads", C.c_uint32),
                ("pad", C.c_uint32)]


class TrimParams(C.Structure):
    """pgn_trim_params"""
    _fields_ = [("max_samples", C.c_uint32), ("window", C.c_uint32), ("min_elements", C.c_uint32),
                ("min_trim", C.c_uint32), ("mad_mult", C.c_float), ("threshold_mads", C.c_float)]


class SegmentParams(C.Structure):
    """pgn_segment_params"""
    _fields_ = [("length", C.c_uint32), ("overlap", C.c_uint32)]


class ReadSegments(C.Structure):
    """pgn_read_segments"""
    _fields_ = [("first_segment", C.c_uint64), ("nsegments", C.c_uint32), ("trim", C.c_uint32), ("status", C.c_int32),
                ("head_m2", C.c_int32), ("head_mad4", C.c_uint32), ("threshold", C.c_float)]


class Segment(C.Structure):
    """pgn_segment"""
    _fields_ = [("read", C.c_uint32), ("start", C.c_uint32), ("valid", C.c_uint32), ("pad", C.c_uint32)]


class StitchParams(C.Structure):
    """pgn_stitch_params"""
    _fields_ = [("length", C.c_uint32), ("overlap", C.c_uint32), ("frame_samples", C.c_uint32), ("pad", C.c_uint32)]


class StitchSegment(C.Structure):
    """pgn_stitch_segment"""
    _fields_ = [("dst_frame", C.c_uint64), ("first", C.c_uint32), ("count", C.c_uint32)]


PGN_CTC_TILE_FRAMES = 1024


class CtcParams(C.Structure):
    """pgn_ctc_params"""
    _fields_ = [("classes", C.c_uint32), ("blank", C.c_uint32), ("score_type", C.c_uint32), ("pad", C.c_uint32),
                ("alphabet", C.c_uint8 * 64)]


PGN_CRF_DEFAULT_SCRATCH = 1 << 30  # the cap pgn_ctx_set_crf_scratch(ctx, 0) restores
PGN_CRF_MAX_FRAMES = 1 << 24


class CrfParams(C.Structure):
    """pgn_crf_params"""
    _fields_ = [("state_len", C.c_uint32), ("transitions", C.c_uint32), ("score_type", C.c_uint32),
                ("stay_score", C.c_float)]


PGN_QUAL_MAX = 93  # '!' + 93 is '~'


class QualParams(C.Structure):
    """pgn_qual_params"""
    _fields_ = [("q_min", C.c_uint32), ("nthresholds", C.c_uint32), ("thr", C.c_uint32 * PGN_QUAL_MAX)]


PGN_READ_QUAL_TILE_BASES = 4096
PGN_FASTQ_TILE_BYTES = 16384
PGN_FASTQ_MAX_TAGS = 8
PGN_FASTQ_REVERSE = 1


class ReadQualParams(C.Structure):
    """pgn_read_qual_params"""
    _fields_ = [("mean", QualParams), ("skip_bases", C.c_uint32), ("min_mean_q", C.c_uint32),
                ("err", C.c_uint32 * (PGN_QUAL_MAX + 1))]


class FastqParams(C.Structure):
    """pgn_fastq_params"""
    _fields_ = [("flags", C.c_uint32), ("ntags", C.c_uint32), ("tag_name", (C.c_uint8 * 2) * PGN_FASTQ_MAX_TAGS),
                ("d_tag", C.c_void_p * PGN_FASTQ_MAX_TAGS)]


PGN_BAM_MAX_TAGS = 8
PGN_BAM_REVERSE, PGN_BAM_MOVES, PGN_BAM_BGZF = 1, 2, 4
PGN_BGZF_BLOCK_BYTES = 65280


class BamParams(C.Structure):
    """pgn_bam_params"""
    _fields_ = [("flags", C.c_uint32), ("ntags", C.c_uint32), ("tag_name", (C.c_uint8 * 2) * PGN_BAM_MAX_TAGS),
                ("d_tag", C.c_void_p * PGN_BAM_MAX_TAGS), ("stride", C.c_uint32), ("pad", C.c_uint32)]


# typed record tags: pgn_tag_column, pgn_record_tags
PGN_TAG_U32, PGN_TAG_I32, PGN_TAG_F32, PGN_TAG_DICT, PGN_TAG_STR = 0, 1, 2, 3, 4
PGN_REC_MAX_TAGS = 16
PGN_TAG_MAX_STRING = 255


class TagColumn(C.Structure):
    """pgn_tag_column"""
    _fields_ = [("name", C.c_uint8 * 2), ("type", C.c_uint8), ("pad", C.c_uint8), ("nstrings", C.c_uint32),
                ("d_values", C.c_void_p), ("d_str_off", C.c_void_p), ("d_strings", C.c_void_p),
                ("str_capacity", C.c_uint64)]


class RecordTags(C.Structure):
    """pgn_record_tags"""
    _fields_ = [("ncols", C.c_uint32), ("pad", C.c_uint32), ("col", TagColumn * PGN_REC_MAX_TAGS)]


PGN_DEMUX_NONE = 0xFFFFFFFF          # no distance, no position, no barcode
PGN_PATTERN_NO_CLASS = 0xFFFFFFFF    # the class of an adapter or primer
PGN_DEMUX_MAX_WINDOW = 1024
PGN_DEMUX_MAX_PATTERNS = 4096
PGN_DEMUX_MAX_PATTERN_BYTES = 128


# pgn_load_kind and pgn_pod5_load_args (include/pgnano_pod5file.h)
PGN_LOAD_ADC, PGN_LOAD_PA, PGN_LOAD_NORM = 0, 1, 2
LOAD_KINDS = {"adc": PGN_LOAD_ADC, "pa": PGN_LOAD_PA, "norm": PGN_LOAD_NORM}


class LoadArgs(C.Structure):
    """pgn_pod5_load_args"""
    _fields_ = [("kind", C.c_int32), ("out_type", C.c_int32), ("pgnano_variant", C.c_int32), ("pad", C.c_int32),
                ("norm", C.POINTER(NormParams)), ("d_out", C.c_void_p), ("out_capacity", C.c_uint64),
                ("read_out_offsets", C.c_void_p), ("d_adc", C.c_void_p), ("d_stats", C.c_void_p),
                ("d_read_status", C.c_void_p), ("read_offsets_out", C.c_void_p), ("read_counts_out", C.c_void_p)]


# every symbol include/pgnano_hip.h declares: (name, restype, argtypes)
_VP, _SZ, _U64P, _U32P, _I32P = C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p
SIGNATURES = [
    ("pgn_status_string", C.c_char_p, [C.c_int]),
    ("pgn_last_error", C.c_char_p, []),
    ("pgn_ctx_create", C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    ("pgn_ctx_destroy", C.c_int, [_VP]),
    ("pgn_ctx_stream", C.c_void_p, [_VP]),
    ("pgn_compressed_signal_max_size", C.c_size_t, [C.c_size_t]),
    ("pgn_compress_signal", C.c_int, [_VP, _VP, _SZ, _VP, _SZ, C.POINTER(C.c_size_t)]),
    ("pgn_decompress_signal", C.c_int, [_VP, _VP, _SZ, _VP, _SZ]),
    ("pgn_pinanoraw_compress_signal", C.c_int, [_VP, _SZ, _VP, C.POINTER(C.c_size_t)]),
    ("pgn_pod5_vbz_compress_signal", C.c_int, [_VP, _SZ, _VP, C.POINTER(C.c_size_t)]),
    ("pgn_pod5_vbz_decompress_signal", C.c_int, [_VP, _SZ, _SZ, _VP]),
    ("pgn_compress_batch_device", C.c_int,
     [_VP, _SZ, _VP, _U64P, _U32P, _VP, _U64P, _U64P, _U64P, _I32P, _U64P, _VP]),
    ("pgn_decompress_batch_device", C.c_int, [_VP, _SZ, _VP, _U64P, _U64P, _VP, _U64P, _U32P, _I32P, _VP]),
    ("pgn_compress_batch_device_bounded", C.c_int,
     [_VP, C.c_uint32, _SZ, _VP, _U64P, _U32P, _VP, _U64P, _U64P, _U64P, _I32P, _U64P, _VP]),
    ("pgn_decompress_batch_device_bounded", C.c_int,
     [_VP, C.c_uint32, _SZ, _VP, _U64P, _U64P, _VP, _U64P, _U32P, _I32P, _VP]),
    ("pgn_vbz_compressed_signal_max_size", C.c_size_t, [C.c_size_t]),
    ("pgn_vbz_compress_signal", C.c_int, [_VP, _VP, _SZ, _VP, _SZ, C.POINTER(C.c_size_t)]),
    ("pgn_vbz_decompress_signal", C.c_int, [_VP, _VP, _SZ, _VP, _SZ]),
    ("pgn_vbz_compress_batch_device", C.c_int,
     [_VP, _SZ, _VP, _U64P, _U32P, _VP, _U64P, _U64P, _U64P, _I32P, _U64P, _VP]),
    ("pgn_vbz_decompress_batch_device", C.c_int, [_VP, _SZ, _VP, _U64P, _U64P, _VP, _U64P, _U32P, _I32P, _VP]),
    ("pgn_variant_compress_signal", C.c_int, [_VP, C.c_int, _VP, _SZ, _VP, _SZ, C.POINTER(C.c_size_t)]),
    ("pgn_variant_decompress_signal", C.c_int, [_VP, C.c_int, _VP, _SZ, _VP, _SZ]),
    ("pgn_variant_compress_batch_device", C.c_int,
     [_VP, C.c_int, _SZ, _VP, _U64P, _U32P, _VP, _U64P, _U64P, _U64P, _I32P, _U64P, _VP]),
    ("pgn_variant_decompress_batch_device", C.c_int,
     [_VP, C.c_int, _SZ, _VP, _U64P, _U64P, _VP, _U64P, _U32P, _I32P, _VP]),
    ("pgn_decompress_batch_device_pa", C.c_int,
     [_VP, C.c_int, C.c_uint32, _SZ, _VP, _U64P, _U64P, _VP, C.c_int, _U64P, _U32P, _VP, _VP, _I32P, _VP]),
    ("pgn_read_stats_device", C.c_int, [_VP, _SZ, _VP, _U64P, _U64P, _VP, _VP, _VP]),
    ("pgn_decompress_reads_device_norm", C.c_int,
     [_VP, C.c_int, C.c_uint32, _SZ, _SZ, _U64P, _VP, _U64P, _U64P, _U32P, _VP, C.c_int, _U64P, _VP, _VP, _VP, _I32P,
      _VP]),
    ("pgn_ctx_set_select_split", C.c_int, [_VP, C.POINTER(SelectSplit)]),
    ("pgn_ctx_get_select_split", C.c_int, [_VP, C.POINTER(SelectSplit)]),
    ("pgn_select_split_counts", C.c_int, [_VP, C.POINTER(C.c_uint64 * 5)]),
    ("pgn_decompress_reads_device_pa", C.c_int,
     [_VP, C.c_int, C.c_uint32, _SZ, _SZ, _U64P, _VP, _U64P, _U64P, _U32P, _VP, C.c_int, _U64P, _VP, _VP, _I32P, _I32P,
      _VP]),
    ("pgn_reads_status_device", C.c_int, [_VP, _SZ, _U64P, _I32P, _I32P, _VP]),
    ("pgn_segment_reads_device", C.c_int,
     [_VP, _SZ, _VP, _U64P, _U64P, _I32P, C.POINTER(TrimParams), C.POINTER(NormParams), C.POINTER(SegmentParams), _VP,
      C.c_int, C.c_uint64, _VP, _VP, _VP, _U64P, _VP]),
    ("pgn_stitch_plan_device", C.c_int, [_VP, _SZ, _VP, _VP, C.c_uint64, C.POINTER(StitchParams), _VP, _U64P, _VP]),
    ("pgn_stitch_rows_device", C.c_int,
     [_VP, C.POINTER(StitchParams), _VP, C.c_uint64, C.c_uint64, _VP, C.c_uint64, C.c_uint64, C.c_uint32, _VP,
      C.c_uint64, C.c_uint64, _VP]),
    ("pgn_ctc_decode_device", C.c_int,
     [_VP, C.POINTER(CtcParams), _SZ, _U64P, _VP, C.c_uint64, C.c_uint64, C.c_uint64, _VP, C.c_uint64, _U64P, _I32P,
      _U32P, _VP, _VP, _VP]),
    ("pgn_collapse_codes_device", C.c_int,
     [_VP, C.POINTER(C.c_uint8 * 128), _SZ, _U64P, _VP, C.c_uint64, C.c_uint64, _VP, C.c_uint64, _U64P, _I32P, _U32P,
      _VP]),
    ("pgn_ctx_set_crf_scratch", C.c_int, [_VP, C.c_uint64]),
    ("pgn_crf_viterbi_rows_device", C.c_int,
     [_VP, C.POINTER(CrfParams), C.c_uint64, C.c_uint32, _VP, C.c_uint64, C.c_uint64, _VP, C.c_uint64, _VP, _VP]),
    ("pgn_crf_posterior_rows_device", C.c_int,
     [_VP, C.POINTER(CrfParams), C.c_uint64, C.c_uint32, _VP, C.c_uint64, C.c_uint64, _VP, C.c_uint64, _VP]),
    ("pgn_base_qual_device", C.c_int,
     [_VP, C.POINTER(QualParams), _SZ, _U64P, _VP, _VP, C.c_uint64, C.c_uint64, _U64P, _U32P, _I32P, _VP, C.c_uint64,
      _VP]),
    ("pgn_read_qual_device", C.c_int,
     [_VP, C.POINTER(ReadQualParams), _SZ, _U64P, _I32P, _VP, C.c_uint64, _U32P, _U64P, _VP, _VP]),
    ("pgn_fastq_records_device", C.c_int,
     [_VP, C.POINTER(FastqParams), _SZ, _VP, _U64P, _I32P, _VP, _VP, _VP, C.c_uint64, _VP, C.c_uint64, _U64P, _I32P,
      _VP]),
    ("pgn_bam_records_device", C.c_int,
     [_VP, C.POINTER(BamParams), _SZ, _VP, _U64P, _I32P, _VP, _VP, _VP, C.c_uint64, _U64P, _VP, C.c_uint64, C.c_uint64,
      _VP, C.c_uint64, _U64P, _I32P, _U64P, _VP]),
    ("pgn_bam_records_tagged_device", C.c_int,
     [_VP, C.POINTER(BamParams), C.POINTER(RecordTags), _SZ, _VP, _U64P, _I32P, _VP, _VP, _VP, C.c_uint64, _U64P, _VP,
      C.c_uint64, C.c_uint64, _VP, C.c_uint64, _U64P, _I32P, _U64P, _VP]),
    ("pgn_fastq_records_tagged_device", C.c_int,
     [_VP, C.POINTER(FastqParams), C.POINTER(RecordTags), _SZ, _VP, _U64P, _I32P, _VP, _VP, _VP, C.c_uint64, _VP,
      C.c_uint64, _U64P, _I32P, _VP]),
    ("pgn_bgzf_deflate_device", C.c_int,
     [_VP, C.c_uint32, _VP, C.c_uint64, _U64P, _VP, C.c_uint64, _U64P, _U64P, _VP]),
    ("pgn_find_patterns_device", C.c_int,
     [_VP, _SZ, _VP, _U64P, _I32P, C.c_uint64, C.c_uint32, C.c_uint32, _VP, C.c_uint64, _U32P, _VP, _U32P, _U32P, _U32P,
      _U32P, _VP]),
    ("pgn_classify_reads_device", C.c_int,
     [_VP, _SZ, _U64P, _I32P, C.c_uint64, C.c_uint32, _VP, _U32P, _U32P, C.c_uint32, C.c_uint32, _U32P, _U32P, _U32P,
      _U32P, _U32P, _U32P, _U32P, _U32P, _VP]),
    ("pgn_trim_reads_device", C.c_int,
     [_VP, _SZ, _VP, _VP, _U64P, _I32P, C.c_uint64, _U32P, _U32P, _U32P, _U64P, _VP, C.c_uint64, C.c_uint64, _VP, _VP,
      _U32P, C.c_uint64, _U64P, _I32P, _VP, C.c_uint64, _U64P, _U32P, _VP]),
    ("pgn_synth_reads_device", C.c_int,
     [_VP, _SZ, C.c_uint64, C.c_uint64, C.c_uint64, _VP, _U64P, _U32P, C.c_uint32, C.c_int32, C.c_int32, C.c_int32,
      _VP]),
    ("pgn_debug_phase_cycles", C.c_int, [_VP, _VP, C.c_int]),
    ("pgn_debug_decode_units", C.c_int, [_VP, _VP, C.c_size_t]),
    ("pgn_ctx_kernels", C.c_char_p, [_VP, C.c_int]),
    ("pgn_ctx_last_encode_ms", C.c_float, [_VP]),
    ("pgn_ctx_last_decode_ms", C.c_float, [_VP]),
    # include/pgnano_pod5.h
    ("pgn_pod5_batch_create", C.c_int, [_VP, C.c_int, C.c_uint32, C.POINTER(C.c_void_p)]),
    ("pgn_pod5_batch_destroy", C.c_int, [_VP]),
    ("pgn_pod5_compress_reads", C.c_int, [_VP, C.c_uint32, _VP, _VP, C.POINTER(C.c_size_t), C.POINTER(C.c_void_p),
                                          C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    ("pgn_pod5_decompress_rows", C.c_int, [_VP, C.c_uint32, _VP, _VP, _VP, _VP, _VP]),
    ("pgn_pod5_last_error", C.c_char_p, []),
    # include/pgnano_pod5file.h
    ("pgn_pod5_file_error", C.c_char_p, []),
    ("pgn_pod5_file_open", C.c_int, [C.c_char_p, C.POINTER(C.c_void_p)]),
    ("pgn_pod5_file_close", C.c_int, [_VP]),
    ("pgn_pod5_file_identifier", C.c_char_p, [_VP]),
    ("pgn_pod5_file_software", C.c_char_p, [_VP]),
    ("pgn_pod5_file_pod5_version", C.c_char_p, [_VP]),
    ("pgn_pod5_file_embedded_count", C.c_int, [_VP]),
    ("pgn_pod5_file_embedded", C.c_int, [_VP, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                         C.POINTER(C.c_int)]),
    ("pgn_pod5_signal_info", C.c_int, [_VP, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_int),
                                       C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("pgn_pod5_signal_read", C.c_int, [_VP, _VP, _VP, _VP, _VP]),
    ("pgn_pod5_write_file", C.c_int, [C.c_char_p, _VP, C.c_int, C.c_uint64, _VP, _VP, _VP, _VP, C.c_uint32,
                                      C.c_char_p, _VP]),
    ("pgn_pod5_write_file_reserved", C.c_int, [C.c_char_p, _VP, C.c_int, C.c_uint64, _VP, _VP, _VP, C.c_uint32,
                                               C.c_char_p, _VP, C.c_int, _VP]),
    ("pgn_pod5_signal_batch_row_counts", C.c_int, [_VP, _VP]),
    ("pgn_pod5_write_file_keep_going", C.c_int, [C.c_char_p, _VP, C.c_int, C.c_uint64, _VP, _VP, _VP, _VP, _VP,
                                                 C.c_uint32, _VP, _VP]),
    ("pgn_pod5_transcode_file_ex", C.c_int, [_VP, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_uint32, C.c_uint32,
                                             _VP, _VP]),
    ("pgn_pod5_transcode_file", C.c_int, [_VP, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_uint32, _VP]),
    ("pgn_pod5_signal_batch_rows", C.c_int, [_VP, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("pgn_pod5_signal_read_batches", C.c_int, [_VP, _VP, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                               C.POINTER(C.c_uint64), _VP, _VP, _VP, _VP]),
    ("pgn_pod5_transcode_part", C.c_int, [_VP, _VP, _VP, C.c_uint32, C.c_int, C.c_int, C.POINTER(C.c_void_p), _VP]),
    ("pgn_pod5_part_get", C.c_int, [_VP, C.POINTER(C.c_uint64), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    ("pgn_pod5_part_free", C.c_int, [_VP]),
    ("pgn_pod5_reads_info", C.c_int, [_VP, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    ("pgn_pod5_reads_read", C.c_int, [_VP] * 11),
    ("pgn_pod5_load_row_lists_device", C.c_int, [_VP, _VP, _SZ, _U64P, _U64P, _VP, _VP, C.POINTER(LoadArgs), _VP]),
    ("pgn_pod5_load_reads_device", C.c_int, [_VP, _VP, _U64P, _SZ, C.POINTER(LoadArgs), _VP]),
]


class NativeLibraryError(RuntimeError):
    pass


_lib = None
_lock = threading.Lock()


def load(path: str | None = None) -> C.CDLL:
    """Load (once) and return the codec library; raise if it is not built."""
    global _lib
    with _lock:
        if _lib is not None and path is None:
            return _lib
        # PGN_LIB: an alternative build of the same library (A/B measurements of kernel variants)
        p = path or os.environ.get("PGN_LIB") or (PROF_LIB_PATH if os.environ.get("PGN_PHASE_PROFILE") == "1" else LIB_PATH)
        # One HIP runtime per process: PyTorch ships its own libamdhip64 (soname libamdhip64.so.7,
        # but its libraries NEED the unversioned name), so load torch first and let this library
        # bind to the runtime torch already mapped; loading ours first would map a second runtime.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        if not os.path.exists(p):
            raise NativeLibraryError(
                f"{p} is missing: build it with `make -C rawnanoporesignalcompression_amd` "
                "(or __graft_entry__.build()); there is no CPU fallback")
        lib = C.CDLL(p)
        for name, res, args in SIGNATURES:
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if path is None:
            _lib = lib
        return lib
