// pgn_internal.h -- in-library entry points shared by pgn_kernels.hip and pgn_pod5.hip (not part of
// the C ABI).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/pgnano_hip.h"

// The batched device calls of pgnano_hip.h for a pgnano variant (pgn_variant) or the VBZ codec
// (PGN_POD5_CODEC_VBZ), with the caller's bound on d_sample_counts (max_samples, 0 = unknown): a
// bound at or below the batched passes' chunk size skips the large-chunk scan and its host wait.
__attribute__((visibility("hidden"))) int pgn_compress_batch_bounded(
    pgn_ctx* ctx, int codec, uint32_t max_samples, size_t nchunks, const int16_t* d_samples,
    const uint64_t* d_sample_offsets, const uint32_t* d_sample_counts, uint8_t* d_out, const uint64_t* d_out_offsets,
    const uint64_t* d_out_caps, uint64_t* d_out_sizes, int32_t* d_status, uint64_t* d_stats, void* stream);
__attribute__((visibility("hidden"))) int pgn_decompress_batch_bounded(
    pgn_ctx* ctx, int codec, uint32_t max_samples, size_t nchunks, const uint8_t* d_in, const uint64_t* d_in_offsets,
    const uint64_t* d_in_sizes, int16_t* d_samples, const uint64_t* d_sample_offsets, const uint32_t* d_sample_counts,
    int32_t* d_status, void* stream);

// ---- the POD5 loader (pgn_pod5.hip) -------------------------------------------------------------
#include "../../include/pgnano_pod5file.h"

// Where signal rows rows[0..n) of f sit in the file image: data[i] .. + bytes[i] (the compressed blob,
// or 2 x samples little-endian bytes when the table is uncompressed) and samples[i].  Consecutive rows
// of one record batch are adjacent.  PGN_ERR_INVALID_ARG for a row at or beyond the table's rows.
__attribute__((visibility("hidden"))) int pgn_pod5_signal_row_spans(const pgn_pod5_file* f, size_t n,
                                                                    const uint64_t* rows, const uint8_t** data,
                                                                    uint64_t* bytes, uint32_t* samples);

// One object another translation unit keeps on the context (the loader's staging): destroy(p) runs in
// pgn_ctx_destroy after the context's streams have drained.
__attribute__((visibility("hidden"))) void* pgn_ctx_ext_get(pgn_ctx* ctx);
__attribute__((visibility("hidden"))) void pgn_ctx_ext_set(pgn_ctx* ctx, void* p, void (*destroy)(void*));
__attribute__((visibility("hidden"))) int pgn_ctx_device(pgn_ctx* ctx);

// pgn_decompress_reads_device_norm's parameter checks, for a caller that must refuse before it uploads.
__attribute__((visibility("hidden"))) bool pgn_norm_params_valid(const pgn_norm_params* params);

// The statistics and the elementwise pass of pgn_decompress_reads_device_norm over reads whose samples
// are already in d_adc (the loader's uncompressed tables): per chunk d_chunk_out (elements),
// d_sample_counts and d_chunk_read; per read d_read_out_offsets and d_read_n.
__attribute__((visibility("hidden"))) int pgn_norm_decoded_reads(
    pgn_ctx* ctx, size_t nreads, size_t nchunks, const int16_t* d_adc, void* d_out, int out_type,
    const uint64_t* d_read_out_offsets, const uint64_t* d_read_n, const uint64_t* d_chunk_out,
    const uint32_t* d_sample_counts, const uint32_t* d_chunk_read, const pgn_norm_params* params,
    pgn_read_stats* d_stats, void* stream);
