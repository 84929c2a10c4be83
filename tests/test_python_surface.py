"""The package's Python surface, held to a table printed from the commit before the binding was reorganised
(host models to host.py, one launch scope, shared argument helpers): every name of ``__all__``, the signature of
every public function, of every public method and ``__init__`` the package's classes define, and each class's
public attribute names.  The table is the output of ``python tests/test_python_surface.py`` run at that commit
(`surface()` below, the function the test compares with); it is regenerated only when a change means to alter
the surface, never to follow one.
"""
import inspect
import os
import pprint
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "rawnanoporesignalcompression_amd"


def surface():
    """(``__all__``, {callable: signature}, {class: public attribute names}) of the package as imported."""
    import rawnanoporesignalcompression_amd as pkg

    sigs, attrs = {}, {}
    for name in pkg.__all__:
        obj = getattr(pkg, name)
        if inspect.isclass(obj):
            own = [k for k in obj.__mro__ if k.__module__.startswith(PKG)]
            attrs[name] = sorted({n for k in own for n in vars(k) if not n.startswith("_")})
            if any("__init__" in vars(k) for k in own):
                sigs[f"{name}.__init__"] = str(inspect.signature(obj.__init__))
            for a in attrs[name]:
                m = inspect.getattr_static(obj, a)
                m = m.__func__ if isinstance(m, (staticmethod, classmethod)) else m
                if inspect.isfunction(m):
                    sigs[f"{name}.{a}"] = str(inspect.signature(m))
        elif callable(obj):
            sigs[name] = str(inspect.signature(obj))
    return list(pkg.__all__), sigs, attrs


def test_all_is_the_same_list():
    assert surface()[0] == ALL
    assert len(ALL) == 45


def test_every_signature_is_the_same():
    sigs = surface()[1]
    assert sorted(sigs) == sorted(SIGNATURES), set(sigs) ^ set(SIGNATURES)
    assert len(SIGNATURES) == 109
    changed = {k: (sigs[k], SIGNATURES[k]) for k in SIGNATURES if sigs[k] != SIGNATURES[k]}
    assert not changed, changed


def test_every_class_has_the_same_public_attributes():
    assert surface()[2] == ATTRIBUTES


def test_names_tests_import_from_codec_stay_there():
    from rawnanoporesignalcompression_amd.codec import (_alphabet_bytes, compressed_signal_max_size,  # noqa: F401
                                                        vbz_compress_signal_capi, vbz_decompress_signal_capi)


def test_host_module_needs_no_torch():
    """In a fresh process: importing the host models (and with them the package) leaves torch unloaded."""
    code = (f"import sys; sys.path.insert(0, {ROOT!r}); import {PKG}.host; "
            "assert 'torch' not in sys.modules, 'torch was imported'")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- the table (see the module docstring) --------------------------------------------------------------------------
ALL = ['LoadedReads', 'Pod5File', 'Pod5FileError', 'ReadsTable', 'CrfCodes', 'DecodedReads', 'EncodedBatch',
 'NativeLibraryError', 'PGN_MAX_CHUNK_SAMPLES', 'PGNanoCodec', 'PGNanoError', 'Pod5SignalBatch', 'ReadSegments',
 'ReadStats', 'SegmentTable', 'SegmentedReads', 'StitchPlan', 'StitchTable', 'VBZCodec', 'calibrate_signal',
 'collapse_codes_signal', 'compress_signal', 'compressed_signal_max_size', 'crf_params', 'crf_viterbi_signal',
 'ctc_decode_signal', 'ctc_params', 'decompress_signal', 'default_codec', 'load_native', 'norm_params',
 'normalise_signal', 'pinanoraw_compress_signal', 'segment_bound', 'segment_params', 'segment_signal', 'select_parts',
 'stitch_bound', 'stitch_params', 'stitch_plan_signal', 'trim_params', 'trim_signal', 'vbz_compress_signal_capi',
 'vbz_compressed_signal_max_size', 'vbz_decompress_signal_capi']

SIGNATURES = {'LoadedReads.__init__': '(self, out: "\'object\'", offsets: \'np.ndarray\', counts: \'np.ndarray\', status: '
                         '"\'object\'", stats: "\'object\'", adc: "\'object\'" = None) -> None',
 'Pod5File.__init__': "(self, path: 'str')",
 'Pod5File.batch_row_counts': "(self) -> 'np.ndarray'",
 'Pod5File.batch_rows': "(self, batch: 'int') -> 'tuple[int, int]'",
 'Pod5File.close': "(self) -> 'None'",
 'Pod5File.load_reads': "(self, codec, reads=None, output: 'str' = 'pa', dtype=None, out=None, out_offsets=None, "
                        "stream: 'int | None' = None, row_lists=None, calibration=None, adc=None, **norm_params) -> "
                        "'LoadedReads'",
 'Pod5File.load_segments': '(self, codec, reads=None, *, length, overlap, trim=None, dtype=None, **norm_params)',
 'Pod5File.read_batches': "(self, batch_ids) -> 'SignalTable'",
 'Pod5File.reads': "(self) -> 'ReadsTable'",
 'Pod5File.row_columns': "(self) -> 'tuple[np.ndarray, np.ndarray]'",
 'Pod5File.signal_table': "(self) -> 'SignalTable'",
 'Pod5FileError.__init__': "(self, status: 'int', what: 'str')",
 'ReadsTable.__init__': "(self, read_id: 'np.ndarray', row_first: 'np.ndarray', rows: 'np.ndarray', num_samples: "
                        "'np.ndarray', signal_samples: 'np.ndarray', calibration_offset: 'np.ndarray', "
                        "calibration_scale: 'np.ndarray', read_number: 'np.ndarray', channel: 'np.ndarray', well: "
                        "'np.ndarray', batches: 'int' = 0) -> None",
 'ReadsTable.index_of': "(self, read_ids) -> 'np.ndarray'",
 'CrfCodes.__init__': '(self, codes: "\'object\'", row_score: "\'object\'", params: "\'object\'") -> None',
 'DecodedReads.__init__': '(self, seq: "\'object\'", read_bases: "\'object\'", status: "\'object\'", base_frame: '
                          '"\'object\'", base_score: "\'object\'", codes: "\'object\'", params: "\'object\'") -> '
                          'None',
 'DecodedReads.sequences': '(self)',
 'EncodedBatch.__init__': '(self, blobs: "\'object\'", offsets: "\'object\'", caps: "\'object\'", sizes: '
                          '"\'object\'", status: "\'object\'", stats: "\'object | None\'") -> None',
 'PGNanoCodec.__init__': "(self, device: 'int' = 0, variant: 'str' = 'C5')",
 'PGNanoCodec.close': "(self) -> 'None'",
 'PGNanoCodec.collapse_codes': "(self, codes, read_frames, alphabet, *, frame_base: 'int' = 0, capacity=None, "
                               "base_frame: 'bool' = True, stream: 'int | None' = None) -> 'DecodedReads'",
 'PGNanoCodec.compress_batch': "(self, samples, sample_offsets, sample_counts, with_stats: 'bool' = False, out=None, "
                               "out_offsets=None, out_caps=None, stream: 'int | None' = None, max_chunk_samples: "
                               "'int | None' = None) -> 'EncodedBatch'",
 'PGNanoCodec.compress_signal': "(self, samples, read_data=None, is_last_batch: 'bool' = False) -> 'bytes'",
 'PGNanoCodec.crf_viterbi': "(self, rows, state_len, *, transitions=None, stay_score=0.0, time_major: 'bool' = "
                            "False, codes=None, row_score: 'bool' = True, stream: 'int | None' = None) -> 'CrfCodes'",
 'PGNanoCodec.ctc_decode': "(self, frames, read_frames, *, alphabet='NACGT', blank=0, frame_base: 'int' = 0, "
                           "capacity=None, base_frame: 'bool' = True, base_score: 'bool' = True, codes: 'bool' = "
                           "False, stream: 'int | None' = None) -> 'DecodedReads'",
 'PGNanoCodec.decompress_batch': '(self, blobs, blob_offsets, blob_sizes, sample_counts, out=None, out_offsets=None, '
                                 "stream: 'int | None' = None, max_chunk_samples: 'int | None' = None)",
 'PGNanoCodec.decompress_batch_pa': '(self, blobs, blob_offsets, blob_sizes, sample_counts, cal_offset, cal_scale, '
                                    "dtype=None, out=None, out_offsets=None, stream: 'int | None' = None, "
                                    "max_chunk_samples: 'int | None' = None)",
 'PGNanoCodec.decompress_reads_norm': '(self, blobs, blob_offsets, blob_sizes, sample_counts, read_first_chunk, *, '
                                      "mode='quantile', p=(0.2, 0.9), centre_mult=0.51, spread_mult=0.53, "
                                      'spread_floor=1.0, dtype=None, out=None, read_out_offsets=None, adc=None, '
                                      "max_chunk_samples: 'int' = 0, stream: 'int | None' = None)",
 'PGNanoCodec.decompress_reads_pa': '(self, blobs, blob_offsets, blob_sizes, sample_counts, read_first_chunk, '
                                    'cal_offset=None, cal_scale=None, *, dtype=None, out=None, '
                                    "read_out_offsets=None, max_chunk_samples: 'int' = 0, stream: 'int | None' = "
                                    'None)',
 'PGNanoCodec.decompress_signal': "(self, compressed, destination=None, state=None, sample_count: 'int | None' = "
                                  'None)',
 'PGNanoCodec.kernels': "(self, direction: 'int') -> 'str'",
 'PGNanoCodec.last_decode_ms': "(self) -> 'float'",
 'PGNanoCodec.last_encode_ms': "(self) -> 'float'",
 'PGNanoCodec.max_size': "(sample_count: 'int') -> 'int'",
 'PGNanoCodec.read_stats': "(self, samples, read_offsets, read_counts, stream: 'int | None' = None, **params) -> "
                           "'ReadStats'",
 'PGNanoCodec.reads_status': "(self, read_first_chunk, chunk_status, stream: 'int | None' = None)",
 'PGNanoCodec.segment_reads': '(self, samples, read_offsets, read_counts, *, length, overlap, trim=None, dtype=None, '
                              "read_status=None, capacity=None, out=None, stream: 'int | None' = None, **norm) -> "
                              "'SegmentedReads'",
 'PGNanoCodec.select_split_counts': "(self) -> 'dict'",
 'PGNanoCodec.set_crf_scratch': "(self, nbytes: 'int' = 0) -> 'None'",
 'PGNanoCodec.set_select_split': "(self, split_min_samples=None, part_samples=None, max_split_reads=None) -> 'None'",
 'PGNanoCodec.stitch': "(self, plan: 'StitchPlan', rows, first_segment: 'int' = 0, out=None, frame_base: 'int' = 0, "
                       "time_major: 'bool' = False, stream: 'int | None' = None)",
 'PGNanoCodec.stitch_plan': "(self, segmented: 'SegmentedReads', length, overlap, frame_samples, capacity=None, "
                            "stream: 'int | None' = None) -> 'StitchPlan'",
 'PGNanoCodec.synth_reads': "(self, nreads: 'int', samples_per_read, seed: 'int' = 42, first_read: 'int' = 0, "
                            "read_stride: 'int' = 1, p_switch_q16: 'int' = 6554, level_mean: 'int' = 500, level_sd: "
                            "'int' = 60, noise_sd: 'int' = 12, out=None)",
 'PGNanoError.__init__': "(self, status: 'int', detail: 'str' = '')",
 'Pod5SignalBatch.__init__': "(self, codec: 'PGNanoCodec', chunk_size: 'int' = 0)",
 'Pod5SignalBatch.close': "(self) -> 'None'",
 'Pod5SignalBatch.compress_reads': "(self, reads, copy: 'bool' = True)",
 'Pod5SignalBatch.decompress_rows': '(self, offsets, data, samples, out=None)',
 'ReadSegments.__init__': '(self, raw)',
 'ReadSegments.numpy': '(self)',
 'ReadStats.__init__': '(self, raw)',
 'ReadStats.numpy': '(self)',
 'SegmentTable.__init__': '(self, raw)',
 'SegmentTable.numpy': '(self)',
 'SegmentedReads.__init__': '(self, out: "\'object\'", segments: \'SegmentTable\', reads: \'ReadSegments\', stats: '
                            '\'ReadStats\', total: "\'object\'") -> None',
 'StitchPlan.__init__': '(self, segments: \'StitchTable\', read_frames: "\'object\'", params: "\'object\'") -> None',
 'StitchTable.__init__': '(self, raw)',
 'StitchTable.numpy': '(self)',
 'VBZCodec.__init__': "(self, device: 'int' = 0)",
 'VBZCodec.close': "(self) -> 'None'",
 'VBZCodec.collapse_codes': "(self, codes, read_frames, alphabet, *, frame_base: 'int' = 0, capacity=None, "
                            "base_frame: 'bool' = True, stream: 'int | None' = None) -> 'DecodedReads'",
 'VBZCodec.compress_batch': "(self, samples, sample_offsets, sample_counts, with_stats: 'bool' = False, out=None, "
                            "out_offsets=None, out_caps=None, stream: 'int | None' = None, max_chunk_samples: 'int | "
                            "None' = None) -> 'EncodedBatch'",
 'VBZCodec.compress_signal': "(self, samples, read_data=None, is_last_batch: 'bool' = False) -> 'bytes'",
 'VBZCodec.crf_viterbi': "(self, rows, state_len, *, transitions=None, stay_score=0.0, time_major: 'bool' = False, "
                         "codes=None, row_score: 'bool' = True, stream: 'int | None' = None) -> 'CrfCodes'",
 'VBZCodec.ctc_decode': "(self, frames, read_frames, *, alphabet='NACGT', blank=0, frame_base: 'int' = 0, "
                        "capacity=None, base_frame: 'bool' = True, base_score: 'bool' = True, codes: 'bool' = False, "
                        "stream: 'int | None' = None) -> 'DecodedReads'",
 'VBZCodec.decompress_batch': '(self, blobs, blob_offsets, blob_sizes, sample_counts, out=None, out_offsets=None, '
                              "stream: 'int | None' = None, max_chunk_samples: 'int | None' = None)",
 'VBZCodec.decompress_batch_pa': '(self, blobs, blob_offsets, blob_sizes, sample_counts, cal_offset, cal_scale, '
                                 "dtype=None, out=None, out_offsets=None, stream: 'int | None' = None, "
                                 "max_chunk_samples: 'int | None' = None)",
 'VBZCodec.decompress_reads_norm': '(self, blobs, blob_offsets, blob_sizes, sample_counts, read_first_chunk, *, '
                                   "mode='quantile', p=(0.2, 0.9), centre_mult=0.51, spread_mult=0.53, "
                                   'spread_floor=1.0, dtype=None, out=None, read_out_offsets=None, adc=None, '
                                   "max_chunk_samples: 'int' = 0, stream: 'int | None' = None)",
 'VBZCodec.decompress_reads_pa': '(self, blobs, blob_offsets, blob_sizes, sample_counts, read_first_chunk, '
                                 'cal_offset=None, cal_scale=None, *, dtype=None, out=None, read_out_offsets=None, '
                                 "max_chunk_samples: 'int' = 0, stream: 'int | None' = None)",
 'VBZCodec.decompress_signal': "(self, compressed, destination=None, state=None, sample_count: 'int | None' = None)",
 'VBZCodec.kernels': "(self, direction: 'int') -> 'str'",
 'VBZCodec.last_decode_ms': "(self) -> 'float'",
 'VBZCodec.last_encode_ms': "(self) -> 'float'",
 'VBZCodec.max_size': "(sample_count: 'int') -> 'int'",
 'VBZCodec.read_stats': "(self, samples, read_offsets, read_counts, stream: 'int | None' = None, **params) -> "
                        "'ReadStats'",
 'VBZCodec.reads_status': "(self, read_first_chunk, chunk_status, stream: 'int | None' = None)",
 'VBZCodec.segment_reads': '(self, samples, read_offsets, read_counts, *, length, overlap, trim=None, dtype=None, '
                           "read_status=None, capacity=None, out=None, stream: 'int | None' = None, **norm) -> "
                           "'SegmentedReads'",
 'VBZCodec.select_split_counts': "(self) -> 'dict'",
 'VBZCodec.set_crf_scratch': "(self, nbytes: 'int' = 0) -> 'None'",
 'VBZCodec.set_select_split': "(self, split_min_samples=None, part_samples=None, max_split_reads=None) -> 'None'",
 'VBZCodec.stitch': "(self, plan: 'StitchPlan', rows, first_segment: 'int' = 0, out=None, frame_base: 'int' = 0, "
                    "time_major: 'bool' = False, stream: 'int | None' = None)",
 'VBZCodec.stitch_plan': "(self, segmented: 'SegmentedReads', length, overlap, frame_samples, capacity=None, stream: "
                         "'int | None' = None) -> 'StitchPlan'",
 'VBZCodec.synth_reads': "(self, nreads: 'int', samples_per_read, seed: 'int' = 42, first_read: 'int' = 0, "
                         "read_stride: 'int' = 1, p_switch_q16: 'int' = 6554, level_mean: 'int' = 500, level_sd: "
                         "'int' = 60, noise_sd: 'int' = 12, out=None)",
 'calibrate_signal': "(adc, offset, scale, dtype=<class 'numpy.float32'>)",
 'collapse_codes_signal': '(codes, alphabet)',
 'compress_signal': "(samples, pool=None, read_data=None, is_last_batch: 'bool' = False) -> 'bytes'",
 'compressed_signal_max_size': "(sample_count: 'int') -> 'int'",
 'crf_params': "(state_len, transitions=5, dtype=<class 'numpy.float16'>, stay_score=0.0)",
 'crf_viterbi_signal': '(scores, state_len, transitions=5, stay_score=0.0)',
 'ctc_decode_signal': "(scores, alphabet='NACGT', blank=0)",
 'ctc_params': "(classes, blank=0, alphabet='NACGT', dtype=<class 'numpy.float16'>)",
 'decompress_signal': "(compressed, pool=None, destination=None, state=None, sample_count: 'int | None' = None)",
 'default_codec': "() -> 'PGNanoCodec'",
 'load_native': "(path: 'str | None' = None) -> 'C.CDLL'",
 'norm_params': "(mode='quantile', p=(0.2, 0.9), centre_mult=0.51, spread_mult=0.53, spread_floor=1.0)",
 'normalise_signal': "(adc, centre, spread, dtype=<class 'numpy.float32'>)",
 'pinanoraw_compress_signal': "(signal, buffer_size: 'int | None' = None) -> 'bytes'",
 'segment_bound': "(counts, length, overlap) -> 'int'",
 'segment_params': '(length, overlap)',
 'segment_signal': "(adc, length, overlap, trim=None, dtype=<class 'numpy.float16'>, **norm)",
 'select_parts': "(n: 'int', split_min_samples: 'int', part_samples: 'int')",
 'stitch_bound': "(counts, length, overlap, frame_samples) -> 'int'",
 'stitch_params': '(length, overlap, frame_samples)',
 'stitch_plan_signal': '(m_or_segments, length, overlap, frame_samples)',
 'trim_params': '(max_samples=8000, window=40, min_elements=3, min_trim=10, mad_mult=1.4826, threshold_mads=2.4)',
 'trim_signal': "(adc, **trim) -> 'int'",
 'vbz_compress_signal_capi': "(signal, buffer_size: 'int | None' = None) -> 'bytes'",
 'vbz_compressed_signal_max_size': "(sample_count: 'int') -> 'int'",
 'vbz_decompress_signal_capi': "(compressed, sample_count: 'int')"}

ATTRIBUTES = {'LoadedReads': ['adc'],
 'Pod5File': ['batch_row_counts', 'batch_rows', 'close', 'load_reads', 'load_segments', 'read_batches', 'reads',
              'row_columns', 'signal_table'],
 'Pod5FileError': [],
 'ReadsTable': ['batches', 'index_of'],
 'CrfCodes': [],
 'DecodedReads': ['sequences'],
 'EncodedBatch': [],
 'NativeLibraryError': [],
 'PGNanoCodec': ['close', 'collapse_codes', 'compress_batch', 'compress_signal', 'crf_viterbi', 'ctc_decode',
                 'decompress_batch', 'decompress_batch_pa', 'decompress_reads_norm', 'decompress_reads_pa',
                 'decompress_signal', 'kernels', 'last_decode_ms', 'last_encode_ms', 'max_size', 'read_stats',
                 'reads_status', 'segment_reads', 'select_split', 'select_split_counts', 'set_crf_scratch',
                 'set_select_split', 'stitch', 'stitch_plan', 'stream', 'synth_reads'],
 'PGNanoError': [],
 'Pod5SignalBatch': ['close', 'compress_reads', 'decompress_rows'],
 'ReadSegments': ['DTYPE', 'numpy'],
 'ReadStats': ['DTYPE', 'numpy'],
 'SegmentTable': ['DTYPE', 'numpy'],
 'SegmentedReads': [],
 'StitchPlan': [],
 'StitchTable': ['DTYPE', 'numpy'],
 'VBZCodec': ['close', 'collapse_codes', 'compress_batch', 'compress_signal', 'crf_viterbi', 'ctc_decode',
              'decompress_batch', 'decompress_batch_pa', 'decompress_reads_norm', 'decompress_reads_pa',
              'decompress_signal', 'kernels', 'last_decode_ms', 'last_encode_ms', 'max_size', 'read_stats',
              'reads_status', 'segment_reads', 'select_split', 'select_split_counts', 'set_crf_scratch',
              'set_select_split', 'stitch', 'stitch_plan', 'stream', 'synth_reads']}


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    names, sigs, attrs = surface()
    print("ALL =", pprint.pformat(names, width=118, compact=True))
    print("\nSIGNATURES =", pprint.pformat(sigs, width=118, sort_dicts=False))
    print("\nATTRIBUTES =", pprint.pformat(attrs, width=118, compact=True, sort_dicts=False))
