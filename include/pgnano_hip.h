/*
 * pgnano_hip.h -- C ABI of the MI355X (gfx950) pgnano "C5" signal codec.
 *
 * Drop-in boundary for the reference's per-chunk plugin surface (tomas-gr/RawNanoporeSignalCompression):
 *   pgnano::compress_signal   pod5/c++/pod5_format/pgnano/pgnano.h:19-23, pgnano.cpp:59-96
 *   pgnano::decompress_signal pod5/c++/pod5_format/pgnano/pgnano.h:13-17, pgnano.cpp:98-126
 * and of the pod5 C-API entry points built on it (pod5/c++/pod5_format/c_api.h:676-712,
 * c_api.cpp:1177-1273).  The compressed bytes are identical to the reference's default
 * COMPRESSOR_C5 variant (pgnano/svb16/C5.hpp:282-683) with libzstd 1.4.8/1.4.9 level 1.
 *
 * Plain pointers and sizes only.  Functions taking `d_` pointers expect device (HBM) memory and are
 * asynchronous on the given HIP stream (`stream` is a hipStream_t, NULL = the context's stream);
 * the others take host memory and are synchronous.  Every function returns a pgn_status.
 */
#ifndef PGNANO_HIP_H
#define PGNANO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum pgn_status {
    PGN_OK = 0,
    PGN_ERR_DST_TOO_SMALL = 1,    /* "Not enough space in destination buffer"       C5.hpp:420-427 */
    PGN_ERR_NOT_ZSTD = 2,         /* "Input data not compressed by zstd"            C5.hpp:495-502 */
    PGN_ERR_ZSTD_DECOMPRESS = 3,  /* "Input data failed to decompress using zstd"   C5.hpp:593-600 */
    PGN_ERR_REMAINING = 4,        /* "Remaining data at end of signal buffer"       C5.hpp:675-677 */
    PGN_ERR_ZSTD_COMPRESS = 5,    /* "Failed to compress ..."                        C5.hpp:340-342 */
    PGN_ERR_CORRUPT = 6,          /* input on which the reference reads out of bounds (UB there) */
    PGN_ERR_ALLOC = 8,            /* decode: the frames' content sizes sum to more than 2^40 bytes, taken as the
                                     reference's allocation of that intermediate failing (C5.hpp:575-583); also
                                     a chunk whose frames could really expand to more than 1 GiB (the claims pass's
                                     intermediate limit, see the decode notes below) */
    PGN_ERR_UNSUPPORTED = 9,      /* chunk above PGN_MAX_CHUNK_SAMPLES */
    PGN_ERR_INVALID_ARG = 10,
    PGN_ERR_HIP = 11,             /* HIP runtime failure (message in pgn_last_error) */
    PGN_ERR_NO_DEVICE = 12,
    PGN_ERR_IO = 13               /* file open/read/write failure (pgnano_pod5file.h) */
} pgn_status;

/* Largest chunk the GPU path encodes and decodes (16 Mi samples; the reference takes any size: its
 * ZSTD_compress and svb16 calls are unbounded, signal_compression.cpp:57-66, C5.hpp:337-413).  Every
 * stream is one zstd frame in 128 KiB blocks as libzstd 1.4.x writes it at level 1: single-segment
 * up to 512 KiB, a window-descriptor frame (windowLog 19, matches within the window) above.  The
 * reference writer's default chunk is 102,400 samples (pod5/c++/pod5_format/file_writer.h:22); the
 * chunk size is a writer option (c_api.h:526-539).
 * Chunks up to 262,144 samples run in the batched passes; larger ones in a second pass of the same
 * call whose per-chunk buffers are spaced for the largest of them (see the batch calls below).
 * Decode: a chunk's decoded frames share an intermediate buffer of 2.25 bytes per sample + 1,024 of
 * the call's largest chunk (262,144 samples when the call gives no bound): every blob whose frames
 * decode to what its merge consumes fits it.  Frames whose content sizes claim more are decoded as the
 * reference decodes them -- each into exactly its claim, in an intermediate of the claims' sum -- by a
 * second pass of the same call (a claim the frame's blocks cannot produce is "failed to decompress",
 * as ZSTD_decompress reports it, without decoding); so a chunk's status does not depend on the other
 * chunks of its call. */
#define PGN_MAX_CHUNK_SAMPLES 16777216u

/* Per-chunk statistics, the reference's global byte counters (src/c++/copy.cpp:64-85, updated at
 * C5.hpp:318-324,467-471): raw stream sizes then frame sizes, order keys, S, M, Llow, Lhigh. */
#define PGN_STATS_PER_CHUNK 10

typedef struct pgn_ctx pgn_ctx;

/* Message of a status code (the reference's arrow::Status text where one exists). */
const char *pgn_status_string(int status);
/* Detail of the last PGN_ERR_HIP on this thread. */
const char *pgn_last_error(void);

/* Context bound to one HIP device (one process per GPU): scratch memory and a stream. */
int pgn_ctx_create(int device, pgn_ctx **out);
int pgn_ctx_destroy(pgn_ctx *ctx);
/* The context's HIP stream (hipStream_t). */
void *pgn_ctx_stream(pgn_ctx *ctx);

/* pgnano::Compressor::compressed_signal_max_size (pgnano/compressor.h:39-45):
 * max(2n + 26, 1024) -- the destination size pgnano::compress_signal allocates. */
size_t pgn_compressed_signal_max_size(size_t sample_count);

/* pgnano::compress_signal (pgnano.cpp:59-96) -> compress_signal_N01 (C5.hpp:282-474), host memory.
 * dst_capacity plays the role of the destination span; *out_size gets the blob size (or, on
 * PGN_ERR_DST_TOO_SMALL, the required size the reference prints at C5.hpp:423-424). */
int pgn_compress_signal(pgn_ctx *ctx, const int16_t *samples, size_t sample_count, uint8_t *dst,
                        size_t dst_capacity, size_t *out_size);

/* pgnano::decompress_signal (pgnano.cpp:98-126) -> decompress_signal_N01 (C5.hpp:477-683), host
 * memory; sample_count is the destination span size (the POD5 `samples` column). */
int pgn_decompress_signal(pgn_ctx *ctx, const uint8_t *compressed, size_t compressed_size, int16_t *dst,
                          size_t sample_count);

/* pod5_pinanoraw_compress_signal (c_api.h:696-700, c_api.cpp:1217-1253) on a default context of
 * device 0: *compressed_signal_size is the buffer size on input, the blob size on output. */
int pgn_pinanoraw_compress_signal(const int16_t *signal, size_t signal_size, char *compressed_signal_out,
                                  size_t *compressed_signal_size);

/* pod5_vbz_compress_signal / pod5_vbz_decompress_signal (c_api.h:685-711, c_api.cpp:1183-1214,
 * 1255-1273) with the same argument shapes, on the default context of device 0: the VBZ codec of
 * the reference's --VBZ path.  Compress: *compressed_signal_size is the buffer size on input and
 * the blob size on output (a blob larger than the buffer is PGN_ERR_DST_TOO_SMALL, the reference's
 * "Compressed signal size (..) is greater than provided buffer size").  Decompress: sample_count
 * samples into signal_out. */
int pgn_pod5_vbz_compress_signal(const int16_t *signal, size_t signal_size, char *compressed_signal_out,
                                 size_t *compressed_signal_size);
int pgn_pod5_vbz_decompress_signal(const char *compressed_signal, size_t compressed_signal_size,
                                   size_t sample_count, short *signal_out);

/* Batched, device-resident encode of `nchunks` independent chunks (each <= PGN_MAX_CHUNK_SAMPLES):
 * chunk i = d_samples[d_sample_offsets[i] .. + d_sample_counts[i]) -> d_out[d_out_offsets[i] ..),
 * capacity d_out_caps[i]; d_out_sizes[i] and d_status[i] receive the result.  d_stats (optional)
 * receives PGN_STATS_PER_CHUNK uint64 per chunk.
 * The batch calls are asynchronous on `stream` except for one host wait: the chunks above 262,144
 * samples (and, when decoding, the chunks whose frames claim more than the batched pass's
 * intermediates) are listed by a small kernel that runs after the work queued before the call (while
 * the batched pass runs) and the host reads their count before queueing their pass.  The wait ends
 * when the earlier work and that kernel have finished, not the call's own kernels.  The _bounded
 * variants below skip it. */
int pgn_compress_batch_device(pgn_ctx *ctx, size_t nchunks, const int16_t *d_samples,
                              const uint64_t *d_sample_offsets, const uint32_t *d_sample_counts, uint8_t *d_out,
                              const uint64_t *d_out_offsets, const uint64_t *d_out_caps, uint64_t *d_out_sizes,
                              int32_t *d_status, uint64_t *d_stats, void *stream);

/* Batched, device-resident decode: blob i = d_in[d_in_offsets[i] .. + d_in_sizes[i]) ->
 * d_samples[d_sample_offsets[i] .. + d_sample_counts[i]). */
int pgn_decompress_batch_device(pgn_ctx *ctx, size_t nchunks, const uint8_t *d_in, const uint64_t *d_in_offsets,
                                const uint64_t *d_in_sizes, int16_t *d_samples, const uint64_t *d_sample_offsets,
                                const uint32_t *d_sample_counts, int32_t *d_status, void *stream);

/* The batch calls with the caller's bound on the chunk sizes (max_chunk_samples >= every
 * d_sample_counts[i], e.g. the writer's chunk size, file_writer.h:22): with a bound at or below
 * 262,144 samples no scan runs and the call never waits on the host; the decode intermediates are
 * spaced for the bound.  A chunk above the bound may get PGN_ERR_UNSUPPORTED.  Decode: a chunk whose
 * frames claim more than 2.25 x the bound + 1,024 bytes and could really produce it gets
 * PGN_ERR_UNSUPPORTED here (listing it needs the host wait; the unbounded call decodes it as the
 * reference does). */
int pgn_compress_batch_device_bounded(pgn_ctx *ctx, uint32_t max_chunk_samples, size_t nchunks,
                                      const int16_t *d_samples, const uint64_t *d_sample_offsets,
                                      const uint32_t *d_sample_counts, uint8_t *d_out, const uint64_t *d_out_offsets,
                                      const uint64_t *d_out_caps, uint64_t *d_out_sizes, int32_t *d_status,
                                      uint64_t *d_stats, void *stream);
int pgn_decompress_batch_device_bounded(pgn_ctx *ctx, uint32_t max_chunk_samples, size_t nchunks, const uint8_t *d_in,
                                        const uint64_t *d_in_offsets, const uint64_t *d_in_sizes, int16_t *d_samples,
                                        const uint64_t *d_sample_offsets, const uint32_t *d_sample_counts,
                                        int32_t *d_status, void *stream);

/* ---- VBZ: the pod5 baseline codec (svb16 + zstd level 1), same context, same conventions ------
 * pod5::compressed_signal_max_size (signal_compression.cpp:14-19):
 * ZSTD_compressBound(svb16_max_encoded_length(n)) = ZSTD_compressBound(ceil(n/8) + 2n). */
size_t pgn_vbz_compressed_signal_max_size(size_t sample_count);

/* pod5::compress_signal(samples, pool, destination) (signal_compression.cpp:21-50): the compressed
 * size in *out_size; a frame larger than dst_capacity is PGN_ERR_ZSTD_COMPRESS ("Failed to compress
 * data"). */
int pgn_vbz_compress_signal(pgn_ctx *ctx, const int16_t *samples, size_t sample_count, uint8_t *dst,
                            size_t dst_capacity, size_t *out_size);

/* pod5::decompress_signal(compressed, pool, destination) (signal_compression.cpp:96-141). */
int pgn_vbz_decompress_signal(pgn_ctx *ctx, const uint8_t *compressed, size_t compressed_size, int16_t *dst,
                              size_t sample_count);

/* Batched device-resident VBZ encode / decode; arguments as pgn_compress_batch_device /
 * pgn_decompress_batch_device (d_stats: svb16 bytes at [0], frame bytes at [5], others 0). */
int pgn_vbz_compress_batch_device(pgn_ctx *ctx, size_t nchunks, const int16_t *d_samples,
                                  const uint64_t *d_sample_offsets, const uint32_t *d_sample_counts, uint8_t *d_out,
                                  const uint64_t *d_out_offsets, const uint64_t *d_out_caps, uint64_t *d_out_sizes,
                                  int32_t *d_status, uint64_t *d_stats, void *stream);
int pgn_vbz_decompress_batch_device(pgn_ctx *ctx, size_t nchunks, const uint8_t *d_in, const uint64_t *d_in_offsets,
                                    const uint64_t *d_in_sizes, int16_t *d_samples, const uint64_t *d_sample_offsets,
                                    const uint32_t *d_sample_counts, int32_t *d_status, void *stream);

/* ---- The other compile-time pgnano variants as a runtime choice ------------------------------
 * The reference builds one binary per `#define COMPRESSOR_*` (pgnano.cpp:1, 70-92, 105-125;
 * utils/compile_all.sh); blobs carry no variant tag, so reader and writer must agree on it.  Same
 * conventions as the C5 entry points (destination capacity max(2n+26, 1024) from
 * pgn_compressed_signal_max_size; C5 through these calls equals the C5 functions above).
 *   C4   compress_signal_N02    (pgnano/svb16/C4.hpp:274-679)    5 frames, C5 layout on raw values
 *   C1   compress_signal_KD     (C1.hpp:202-382)                 2 frames: svb16 keys, svb16 data
 *   C2   compress_signal_lh     (C2.hpp:195-463)                 3 frames: keys, low bytes, high bytes
 *   C3   compress_signal_ll_lh  (C3.hpp:212-503)                 4 frames: keys, small low, big low, big high
 *   VBZ0 compress_signal_VBZ1   (VBZ_0.hpp:316-423)              1 frame: 2-bit keys + nibble stream
 * VBZ0 compresses straight into the destination ("Failed to compress data" = PGN_ERR_ZSTD_COMPRESS
 * when the frame does not fit); C1/C2/C3 copy into it unchecked in the reference, here a
 * too-small destination is PGN_ERR_DST_TOO_SMALL with the required size, as for C5/C4. */
typedef enum pgn_variant {
    PGN_VARIANT_C5 = 0,
    PGN_VARIANT_C4 = 1,
    PGN_VARIANT_C1 = 2,
    PGN_VARIANT_C2 = 3,
    PGN_VARIANT_C3 = 4,
    PGN_VARIANT_VBZ0 = 5
} pgn_variant;

int pgn_variant_compress_signal(pgn_ctx *ctx, int variant, const int16_t *samples, size_t sample_count, uint8_t *dst,
                                size_t dst_capacity, size_t *out_size);
int pgn_variant_decompress_signal(pgn_ctx *ctx, int variant, const uint8_t *compressed, size_t compressed_size,
                                  int16_t *dst, size_t sample_count);
/* d_stats: raw stream sizes at [0..frames), frame sizes at [5..5+frames), in frame order */
int pgn_variant_compress_batch_device(pgn_ctx *ctx, int variant, size_t nchunks, const int16_t *d_samples,
                                      const uint64_t *d_sample_offsets, const uint32_t *d_sample_counts,
                                      uint8_t *d_out, const uint64_t *d_out_offsets, const uint64_t *d_out_caps,
                                      uint64_t *d_out_sizes, int32_t *d_status, uint64_t *d_stats, void *stream);
int pgn_variant_decompress_batch_device(pgn_ctx *ctx, int variant, size_t nchunks, const uint8_t *d_in,
                                        const uint64_t *d_in_offsets, const uint64_t *d_in_sizes, int16_t *d_samples,
                                        const uint64_t *d_sample_offsets, const uint32_t *d_sample_counts,
                                        int32_t *d_status, void *stream);

/* ---- Calibrated output of the batched device decode ------------------------------------------
 * A GPU basecaller consumes the calibrated signal pA = (adc + offset) * scale (the reference's Python
 * reader, pod5/python/pod5/src/pod5/reader.py:356-368), not ADC counts.  This call decodes as the
 * batch calls above do and writes that value from the merge's own stores, instead of a second pass over
 * the decoded int16 tensor.  One entry point for every codec and both bound modes:
 *   codec              a pgn_variant value, or PGN_POD5_CODEC_VBZ (100, pgnano_pod5.h) for VBZ
 *   max_chunk_samples  0: no bound -- the unbounded calls above, their one host wait included (not a
 *                      bound of 1).  Non-zero: the caller's bound on every d_sample_counts[i], as the
 *                      _bounded calls take it; every codec is served (none gives PGN_ERR_INVALID_ARG
 *                      for its bound), and only the staged C5 / VBZ passes space their intermediates
 *                      for it
 *   d_out, out_type    the output and its element type (pgn_out_type); d_out_offsets[i] is in elements
 *                      of that type
 *   d_cal_offset[i], d_cal_scale[i]   per chunk: the chunks of one read carry that read's calibration
 *                      (the caller expands read -> chunk).  Required for PGN_OUT_F32 / PGN_OUT_F16,
 *                      ignored (may be NULL) for PGN_OUT_INT16
 * The value, exactly:
 *   PGN_OUT_F32   s = (float)adc (exact); a = s + offset in IEEE binary32, round to nearest even;
 *                 out = a * scale likewise.  Two roundings, no wider intermediate, no FMA -- numpy's
 *                 (x.astype(float32) + float32(offset)) * float32(scale), bit for bit
 *   PGN_OUT_F16   that binary32 value converted once to binary16, round to nearest even; overflow
 *                 gives +-inf (numpy's astype(float16))
 *   PGN_OUT_INT16 exactly what the int16 call of the codec writes
 * Non-finite calibration values pass through the arithmetic; nothing is validated.
 * d_status[i] is what the int16 call gives for the same blob, corrupted blobs included.  The output of
 * a chunk whose status is not PGN_OK is unspecified, but nothing is written outside
 * [d_out_offsets[i], + d_sample_counts[i]) of any chunk.
 * A NULL ctx, an unknown codec or out_type, or a missing calibration array is PGN_ERR_INVALID_ARG
 * before any GPU call.
 * Not covered: the host-memory per-chunk calls and pgn_pod5_decompress_rows (link-bound; calibrating
 * on the host is one line there), bfloat16.  The calibration of a POD5 file's reads comes from
 * pgn_pod5_reads_read (pgnano_pod5file.h).  Per-read normalisation is the next section. */
typedef enum pgn_out_type { PGN_OUT_INT16 = 0, PGN_OUT_F32 = 1, PGN_OUT_F16 = 2 } pgn_out_type;

int pgn_decompress_batch_device_pa(pgn_ctx *ctx, int codec, uint32_t max_chunk_samples, size_t nchunks,
                                   const uint8_t *d_in, const uint64_t *d_in_offsets, const uint64_t *d_in_sizes,
                                   void *d_out, int out_type, const uint64_t *d_out_offsets,
                                   const uint32_t *d_sample_counts, const float *d_cal_offset,
                                   const float *d_cal_scale, int32_t *d_status, void *stream);

/* ---- Per-read normalised output (quantile, med/MAD) -------------------------------------------
 * A basecaller front end normalises each read by its own robust statistics: (x - centre) / spread,
 * usually stored as binary16.  The statistics need the whole read and a read spans several chunks, so
 * these calls work on reads.  Everything is exact: the order statistics are integers, the float steps
 * are listed operation by operation.
 * For a read with samples x[0..n) (its chunks concatenated in order) and s = sort(x) ascending:
 *   rank statistic   q(p) = s[k], k = floor(p * (double)(n - 1)): one binary64 multiply, then floor
 *                    (this formula, not numpy.quantile's virtual index)
 *   median, doubled  m2 = s[(n-1)/2] + s[n/2];  med = 0.5f * (float)m2 (exact)
 *   MAD, quadrupled  d_i = |2 x_i - m2|, t = sort(d), mad4 = t[(n-1)/2] + t[n/2];  MAD = 0.25f * (float)mad4
 *                    (numpy's median(x) and median(abs(x - median(x))) in float64)
 *   PGN_NORM_QUANTILE  a = q(p_lo), b = q(p_hi);  centre = centre_mult * (float)(a + b);
 *                      spread = spread_mult * (float)(b - a)   (p_lo, p_hi, centre_mult, spread_mult used)
 *   PGN_NORM_MEDMAD    centre = med;  spread = spread_mult * MAD   (spread_mult used; p and centre_mult
 *                      are still validated)
 *   both               spread = spread_floor where spread < spread_floor
 *   output             inv = 1.0f / spread (one IEEE division);  out32 = ((float)adc + (-centre)) * inv --
 *                      the pA formula above with offset = -centre and scale = inv (two roundings, no FMA);
 *                      PGN_OUT_F16 is that value converted once, round to nearest even
 * The multipliers are the caller's (usual: p 0.2 / 0.9 with 0.51 / 0.53, or 1.4826 for the MAD); the C ABI
 * has no defaults.  Statistics are taken on ADC counts; for a positive calibration scale the normalised
 * value equals the one taken on pA, and centre / spread are returned so a caller can map them to pA.
 * n == 0: nothing is written; every stats field is 0 except spread = 1.  n >= 2^32: the read's status is
 * PGN_ERR_UNSUPPORTED (n is reported, the other fields as for n == 0).  Fields the mode does not use are 0.
 * Both calls return PGN_ERR_INVALID_ARG before any GPU call, checking in this order: a NULL ctx or
 * params; an unknown mode (and, for the decode, codec or out_type, PGN_OUT_INT16 included); p outside
 * [0, 1], NaN or p_lo > p_hi; a non-finite multiplier; spread_floor not > 0; then missing arrays. */
typedef enum pgn_norm_mode { PGN_NORM_QUANTILE = 0, PGN_NORM_MEDMAD = 1 } pgn_norm_mode;
typedef struct pgn_norm_params {
    int32_t mode;  /* pgn_norm_mode */
    int32_t pad;
    double p_lo, p_hi;
    float centre_mult, spread_mult, spread_floor, pad2;
} pgn_norm_params;
typedef struct pgn_read_stats {
    uint64_t n;
    int32_t status;
    int16_t q_lo, q_hi;
    int32_t m2;
    uint32_t mad4;
    float centre, spread;
} pgn_read_stats;

/* Statistics of reads already decoded on the device: read r = d_samples[d_read_offsets[r] .. +
 * d_read_counts[r]) (elements; a read may start on any 2-byte boundary) -> d_stats[r]. */
int pgn_read_stats_device(pgn_ctx *ctx, size_t nreads, const int16_t *d_samples, const uint64_t *d_read_offsets,
                          const uint64_t *d_read_counts, const pgn_norm_params *params, pgn_read_stats *d_stats,
                          void *stream);

/* Decode the chunks of nreads reads and write each read normalised and contiguous.
 *   codec, max_chunk_samples   as for pgn_decompress_batch_device_pa (0 = no bound)
 *   d_read_first_chunk         nreads + 1 entries: read r owns chunks [first[r], first[r+1]) of the
 *                              nchunks chunks, which are in read order (first[nreads] == nchunks)
 *   d_out, out_type            PGN_OUT_F32 or PGN_OUT_F16; read r occupies [d_read_out_offsets[r], + n_r)
 *                              elements, chunk c of it starting after the read's earlier chunks
 *   d_adc                      optional: receives the raw samples at the same element offsets.  Without it
 *                              PGN_OUT_F16 decodes into d_out and converts in place; PGN_OUT_F32 needs it
 *                              (PGN_ERR_INVALID_ARG: the host cannot size a workspace without a wait)
 *   d_stats                    optional: nreads entries
 * Sequence: a small kernel expands reads to chunks (into context scratch, never read by the host), the
 * int16 decode runs unchanged, then the statistics kernels, then one elementwise pass.  Asynchronous on
 * `stream`, with no host wait beyond the unbounded decode's own.  d_chunk_status[c] is what the int16
 * call gives; a read's status is its first chunk status that is not PGN_OK, in chunk order, and the
 * output and stats of such a read are unspecified.  Nothing is written outside
 * [d_read_out_offsets[r], + n_r) of any read.
 * Not covered: adapter trimming (that is pgn_segment_reads_device, "Trimmed, normalised model segments"
 * below), bfloat16, the host-memory per-chunk calls.  The read -> chunk map of a POD5 file comes from
 * pgn_pod5_reads_read, and pgn_pod5_load_reads_device (pgnano_pod5file.h) makes this call from a file. */
int pgn_decompress_reads_device_norm(pgn_ctx *ctx, int codec, uint32_t max_chunk_samples, size_t nreads,
                                     size_t nchunks, const uint64_t *d_read_first_chunk, const uint8_t *d_in,
                                     const uint64_t *d_in_offsets, const uint64_t *d_in_sizes,
                                     const uint32_t *d_sample_counts, void *d_out, int out_type,
                                     const uint64_t *d_read_out_offsets, int16_t *d_adc,
                                     const pgn_norm_params *params, pgn_read_stats *d_stats,
                                     int32_t *d_chunk_status, void *stream);

/* ---- Long reads: one selection shared by several workgroups ---------------------------------------
 * The statistics above are an exact selection over a read's samples.  A read of up to split_min_samples
 * is selected by one workgroup (one wave up to 512 samples); a longer one, below 2^32 samples, is selected
 * in parts = min(ceil(n / part_samples), PGN_SELECT_MAX_PARTS) parts, part j covering samples
 * [floor(j * n / parts), floor((j + 1) * n / parts)): workgroups histogram the parts, the histograms are
 * summed per read with integer adds, and the rank walk runs once on the sum.  Every field of
 * pgn_read_stats, and everything computed from it, is bit for bit what one workgroup gives.
 * Such a read holds one of max_split_reads slots (a little over 5 KB of context scratch each) for the
 * call; the slots go to the qualifying reads in read order, and a read that finds none is selected by one
 * workgroup as before.  The plan lives on the device: the calls keep their arguments, their checks and
 * their freedom from host waits (context scratch grows with nreads and with max_split_reads, as the
 * segment call's does).  The setting belongs to the context and is read at each call of
 * pgn_read_stats_device, pgn_decompress_reads_device_norm, pgn_segment_reads_device and the POD5 loads
 * built on them.  max_split_reads == 0 switches it off: the launches are then those of one workgroup per
 * read alone.
 * Defaults after pgn_ctx_create: split_min_samples 196608, part_samples 32768, max_split_reads 1024.
 * pgn_ctx_set_select_split returns PGN_ERR_INVALID_ARG for a NULL argument, part_samples outside
 * [1024, 2^24], split_min_samples < part_samples (so a split read has at least two parts) or
 * max_split_reads > 65536.
 * pgn_select_split_counts (a diagnostic) waits for the context's last call and reports its most recent
 * selection (in pgn_segment_reads_device: the one over the trimmed reads): out[0] reads of one wave,
 * out[1] reads of one workgroup (those of out[4] included), out[2] split reads, out[3] their parts,
 * out[4] reads above split_min_samples that found no slot.  All zero when that selection ran with the
 * split off, or before any. */
#define PGN_SELECT_MAX_PARTS 4096
typedef struct pgn_select_split {
    uint32_t split_min_samples, part_samples, max_split_reads, pad;
} pgn_select_split;
int pgn_ctx_set_select_split(pgn_ctx *ctx, const pgn_select_split *s);
int pgn_ctx_get_select_split(pgn_ctx *ctx, pgn_select_split *s);
int pgn_select_split_counts(pgn_ctx *ctx, uint64_t out[5]);

/* ---- Per-read calibrated output ------------------------------------------------------------------
 * pgn_decompress_batch_device_pa for whole reads: the chunks are in read order, d_read_first_chunk and
 * d_read_out_offsets as in the norm call above, and the calibration is per read (d_read_cal_offset[r],
 * d_read_cal_scale[r]; ignored, may be NULL, for PGN_OUT_INT16 -- the device form of
 * pod5_get_read_complete_signal, c_api.h:489-502).  A small kernel expands reads to chunks (output
 * offset, offset and scale per chunk, into context scratch the host never reads), then the decode of
 * pgn_decompress_batch_device_pa runs unchanged: the values are that call's, bit for bit.
 * d_chunk_status[c] is what the int16 call gives.  d_read_status (optional, nreads entries) receives
 * each read's first chunk status that is not PGN_OK, in chunk order; a read without chunks gets PGN_OK.
 * PGN_ERR_INVALID_ARG before any GPU call, in the norm call's order: a NULL ctx; an unknown codec or
 * out_type; then (for nreads > 0: with no reads the arrays have no entries and may be NULL) missing
 * arrays.  No host wait beyond the unbounded decode's own. */
int pgn_decompress_reads_device_pa(pgn_ctx *ctx, int codec, uint32_t max_chunk_samples, size_t nreads, size_t nchunks,
                                   const uint64_t *d_read_first_chunk, const uint8_t *d_in,
                                   const uint64_t *d_in_offsets, const uint64_t *d_in_sizes,
                                   const uint32_t *d_sample_counts, void *d_out, int out_type,
                                   const uint64_t *d_read_out_offsets, const float *d_read_cal_offset,
                                   const float *d_read_cal_scale, int32_t *d_read_status, int32_t *d_chunk_status,
                                   void *stream);

/* The same per-read statuses for the callers of pgn_decompress_reads_device_norm (or of any batch
 * decode whose chunks are in read order): d_read_status[r] = the first of
 * d_chunk_status[first[r] .. first[r + 1]) that is not PGN_OK, else PGN_OK.  Asynchronous on `stream`,
 * ordered after the context's earlier calls. */
int pgn_reads_status_device(pgn_ctx *ctx, size_t nreads, const uint64_t *d_read_first_chunk,
                            const int32_t *d_chunk_status, int32_t *d_read_status, void *stream);

/* ---- Trimmed, normalised model segments -------------------------------------------------------------
 * The last two steps before a basecaller's model: cut the adapter head off each read, normalise what is
 * left by its own statistics, and lay it out as rows of a [segments, L] tensor of fixed-length, overlapping
 * pieces.  One call takes decoded int16 reads on the device and leaves that tensor and its index there.
 * Every output is exact; the definitions below are the contract.  (The trim is the windowed-threshold head
 * trim that basecaller front ends use; no such source was at hand to compare with, so this text defines it.)
 * A read is x[0..n), int16.
 *
 * Trim (pgn_trim_params; usual values max_samples 8000, window 40, min_elements 3, min_trim 10, mad_mult
 * 1.4826, threshold_mads 2.4 -- the C ABI has no defaults):
 *   max_samples == 0   trim = 0: trimming is off and no head statistics are taken
 *   H = min(n, max_samples).  H < min_trim + window: no complete window, trim = min(min_trim, n)
 *   otherwise          m2 and mad4 are those of the head x[0..H), as the per-read normalisation section
 *                      defines them (the same selection computes them), and in binary32, one rounding per
 *                      operation and no FMA:
 *                        centre_h = 0.5f * (float)m2
 *                        spread_h = mad_mult * (0.25f * (float)mad4)        (no floor)
 *                        thr      = centre_h + threshold_mads * spread_h
 *                      A sample is "above" when (float)x[i] > thr.
 *                      W = (H - min_trim) / window windows; window w covers [s, e), s = min_trim + w * window,
 *                      e = s + window.  Scan w = 0 .. W-1 with seen = false:
 *                        if seen, or the window has more than min_elements samples above: seen = true, and
 *                          if x[e-1] is above, go on to the next window;
 *                          otherwise stop: trim = e if e < H, else min_trim
 *                        (a window before the first such peak never stops the scan)
 *                      If the scan ends without stopping, trim = min_trim.
 * Normalisation: pgn_norm_params and the statistics as in the per-read section, taken over y = x[trim..n),
 * m = n - trim samples.  The value is that section's ((float)adc + (-centre)) * (1.0f / spread); PGN_OUT_F16
 * is that value converted once.
 * Segments (pgn_segment_params: length L, overlap V, 0 <= V < L, 1 <= L <= 2^24; stride S = L - V):
 *   m == 0   no segment
 *   m <= L   one segment, start 0, valid = m
 *   m > L    k = ceil((m - L) / S) + 1 segments; segment j starts at min(j * S, m - L) with valid = L, so
 *            the last one ends at the read's end
 * A segment's row is y[start .. start + valid) normalised; elements [valid, L) are +0.0 (all bits zero).
 * Segments are numbered in read order, then start order.  segments(m) does not decrease as m grows, so the
 * count taken from the untrimmed n is an upper bound the host can compute without a wait.
 *
 * pgn_read_segments (one per read): its segments are [first_segment, + nsegments); head_m2, head_mad4 and
 * threshold are 0 where no head statistics were taken.  pgn_segment (one per segment): `start` is the sample
 * index in the untrimmed read (it includes trim).
 * A read's status is d_read_status_in[r] if that array is given and the entry is not PGN_OK; otherwise what
 * the statistics give (n >= 2^32: PGN_ERR_UNSUPPORTED; such a read is not trimmed).
 * A read whose status is not PGN_OK produces no segments; one with a bad input status is not trimmed, and
 * its d_stats entry is unspecified.
 * A segment whose index is at or above segment_capacity is not written, neither its row nor its table
 * entry; every read that has one gets PGN_ERR_DST_TOO_SMALL (its first_segment and nsegments are still
 * what they would be), and *d_total is the number needed.  Nothing is written outside rows
 * [0, min(total, segment_capacity)) of d_out.  With segment_capacity == 0, d_out and d_segments may be NULL.
 * d_stats (optional) receives the statistics of the trimmed reads, d_total (optional) the segment count.
 * Asynchronous on `stream`, no host wait; the work arrays live in context scratch that grows with nreads.
 * PGN_ERR_INVALID_ARG before any GPU call, checking in this order: a NULL ctx or a NULL params struct; the
 * norm parameters as in the per-read section; window < 1 with max_samples > 0, a non-finite mad_mult or
 * threshold_mads; L or V outside the ranges above; out_type not PGN_OUT_F32 or PGN_OUT_F16; then, for
 * nreads > 0, a missing array, or nreads >= 2^32.
 * Not covered: a decode-fused entry point (the norm call is decode, then statistics, then a pass, so this
 * call after an int16 decode costs the same); bfloat16; a maximum-trim fraction or a rejection of
 * over-trimmed reads; front padding. */
typedef struct pgn_trim_params {
    uint32_t max_samples, window, min_elements, min_trim;
    float mad_mult, threshold_mads;
} pgn_trim_params;
typedef struct pgn_segment_params {
    uint32_t length, overlap;
} pgn_segment_params;
typedef struct pgn_read_segments {
    uint64_t first_segment;
    uint32_t nsegments, trim;
    int32_t status;
    int32_t head_m2;
    uint32_t head_mad4;
    float threshold;
} pgn_read_segments;
typedef struct pgn_segment {
    uint32_t read, start, valid, pad;
} pgn_segment;

int pgn_segment_reads_device(pgn_ctx *ctx, size_t nreads, const int16_t *d_samples, const uint64_t *d_read_offsets,
                             const uint64_t *d_read_counts, const int32_t *d_read_status_in,
                             const pgn_trim_params *trim, const pgn_norm_params *norm,
                             const pgn_segment_params *segment, void *d_out, int out_type, uint64_t segment_capacity,
                             pgn_segment *d_segments, pgn_read_segments *d_reads, pgn_read_stats *d_stats,
                             uint64_t *d_total, void *stream);

/* ---- Model output back to reads -----------------------------------------------------------------------
 * The inverse of the cut above, for what a model makes of the rows: a model of stride s turns a row of L
 * samples into T = L / s frames of some fixed number of bytes; neighbouring rows of a read overlap, so their
 * frames are doubled there.  The plan call decides, from the index the segment call left, which frames of
 * every row are kept and where they go; the rows call copies the kept frames of one model batch into a dense
 * per-read layout.  Every output is exact: an index computation and a byte copy.  No outside source defines
 * the rule, so this text does.
 *
 * Parameters (pgn_stitch_params: length L, overlap V, frame_samples s): 1 <= s, L % s == 0, s <= L - V,
 * L <= 2^24; T = L / s.  L and V must be the ones the segments were cut with; nothing can check that.
 *
 * A read is taken when its pgn_read_segments.status is PGN_OK, it has k = nsegments >= 1 segments and all of
 * them lie below segment_capacity.  For its segments j = 0..k-1 let a_j = start_j - start_0 and valid_j be
 * those of the segment table.  Cut points, in samples of the trimmed read:
 *   c_j     = a_{j+1} + floor((a_j + L - a_{j+1}) / 2)   for j < k-1  (the middle of the overlap)
 *   c_{k-1} = a_{k-1} + valid_{k-1}                       (the read's end)
 *   c_{-1}  = 0
 * Segment j owns the samples [c_{j-1}, c_j).  Frame f of segment j is kept iff its first sample a_j + f * s
 * lies in what its segment owns:
 *   first_j = ceil((c_{j-1} - a_j) / s)
 *   end_j   = min(T, ceil((c_j - a_j) / s))
 *   count_j = max(0, end_j - first_j)
 * The read's frames are the kept frames of its segments in segment order, frames_r = sum count_j; reads
 * follow each other in read order, and d_read_frames (nreads + 1 entries) is the exclusive scan of frames_r.
 * pgn_stitch_segment (one per table row): frames [first, first + count) of the row are kept, and `dst_frame`
 * is the index of the first of them in that layout, d_read_frames[read] + sum of count_i over i < j.
 * A read that is not taken (another status, PGN_ERR_DST_TOO_SMALL included, whose later segments were never
 * written; no segments; or a segment at or above segment_capacity) yields no frames: its plan entries below
 * the capacity have first = 0, count = 0 and dst_frame = d_read_frames[read].  Table entries at or above
 * segment_capacity are never read; plan entries [0, min(total, segment_capacity)) are written, total being
 * the segment count of the pgn_read_segments array.
 * What follows from the rule: the kept frames' first samples rise strictly and lie in [0, m) for a trimmed
 * read of m samples; |frames_r - ceil(m / s)| <= k - 1; frames_r <= ceil(n / s) + segments(n) for every
 * untrimmed length n >= m, which is the bound a host can take without a wait.  Where 2s divides V, s divides
 * L - V and the read ends on the segment grid, h = V / (2s) frames are dropped on each side of every joint
 * (segment 0 keeps [0, T - h), the last [h, T), the inner ones [h, T - h)) and frames_r = ceil(m / s).
 *
 * pgn_stitch_plan_device: asynchronous on `stream`, no host wait; its scratch lives on the context and grows
 * with segment_capacity.  With segment_capacity == 0, d_segments and d_plan may be NULL.
 *
 * pgn_stitch_rows_device copies the kept frames of table rows [first_segment, + nsegments), one model batch
 * whose output lies at d_rows: frame f of table row g is the frame_bytes contiguous bytes at
 *   d_rows + (g - first_segment) * row_stride_bytes + f * frame_stride_bytes
 * (an [N, T, C] output has row stride T * C and frame stride C elements, a [T, N, C] output C and N * C), and
 * goes to
 *   d_out + (dst_frame + (f - first) - out_frame_base) * frame_bytes.
 * A frame whose destination index dst_frame + (f - first) - out_frame_base lies outside
 * [0, out_capacity_frames) is not written, and nothing but the kept frames' bytes is written.  d_plan is the
 * whole plan (it is indexed by g).  A frame at or above T is never read, whatever the plan says.  Any
 * alignment of d_rows, d_out and the strides is allowed; 16-byte moves are used where the destination
 * allows.  d_rows and d_out must not overlap.  Asynchronous on `stream`, no host wait, no scratch.
 *
 * PGN_ERR_INVALID_ARG before any GPU call, checking in this order: a NULL ctx or params; the parameter
 * constraints above; then for the plan call a NULL d_read_frames and, with nreads > 0, a NULL d_reads, a NULL
 * d_segments or d_plan with segment_capacity > 0, nreads >= 2^32, or segment_capacity >= 2^40 (with
 * nreads == 0 only d_read_frames[0] = 0 is written); for the rows call frame_bytes == 0, frame_stride_bytes < frame_bytes unless T == 1, then, with
 * nsegments > 0, a NULL d_plan, d_rows or d_out.
 * Not covered: decoding itself; stitching of decoded sequences or move tables; models whose T != L / s
 * (padding or valid convolutions); stitching in place. */
typedef struct pgn_stitch_params {
    uint32_t length, overlap, frame_samples;
    uint32_t pad;
} pgn_stitch_params;
typedef struct pgn_stitch_segment {
    uint64_t dst_frame;
    uint32_t first, count;
} pgn_stitch_segment;

int pgn_stitch_plan_device(pgn_ctx *ctx, size_t nreads, const pgn_read_segments *d_reads,
                           const pgn_segment *d_segments, uint64_t segment_capacity,
                           const pgn_stitch_params *params, pgn_stitch_segment *d_plan, uint64_t *d_read_frames,
                           void *stream);
int pgn_stitch_rows_device(pgn_ctx *ctx, const pgn_stitch_params *params, const pgn_stitch_segment *d_plan,
                           uint64_t first_segment, uint64_t nsegments, const void *d_rows,
                           uint64_t row_stride_bytes, uint64_t frame_stride_bytes, uint32_t frame_bytes,
                           void *d_out, uint64_t out_frame_base, uint64_t out_capacity_frames, void *stream);

/* ---- Stitched frames to bases -------------------------------------------------------------------------
 * The best-path (greedy) CTC decode of the frames the rows call laid end to end: per read its base sequence
 * and per base its frame and score; and, as a call of its own, the second half of it, which turns one code
 * byte per frame into bases.  Every output is a selection, so the tolerance is zero.  No outside source defines
 * the rule, so this text does.
 *
 * Frames are those of the dense per-read layout: frame i has C = classes scores of one type (PGN_OUT_F32 or
 * PGN_OUT_F16), d_read_frames (nreads + 1 entries) is the plan's exclusive scan, read r has the frames i in
 * [read_frames[r], read_frames[r+1]), and t = i - read_frames[r].
 *   Label     l_i = argmax_c scores_i[c] as numpy.argmax computes it: IEEE comparison (-0 == +0), the lowest
 *             index wins a tie, a NaN beats every number and the first NaN wins.  float16 scores are compared
 *             as their exact float32 values.
 *   Emission  frame i emits a base iff l_i != blank and (t == 0 or l_i != l_{i-1}).  The first frame of a read
 *             looks at no predecessor, even if the previous read ended on the same label.
 *   Code      code_i = l_i | 0x80 if the frame emits, else l_i: one byte per frame, which is why C <= 64.
 *   Bases     read r's bases are alphabet[l_i] of its emitting frames in frame order, bases_r of them.
 *             d_read_bases (nreads + 1) is the exclusive scan of bases_r over the reads in read order.  Base j
 *             of read r has the global index g = read_bases[r] + j; with i its emitting frame
 *               seq[g] = alphabet[l_i], base_frame[g] = t, base_score[g] = (float)scores_i[l_i]
 *             (the float16-to-float32 widening is exact).
 * Taken reads and the window.  The call sees frames [frame_base, frame_base + frame_capacity); frame i lies at
 * d_frames + (i - frame_base) * frame_stride_bytes.  A read is taken iff
 *   frame_base <= read_frames[r] <= read_frames[r+1] <= frame_base + frame_capacity.
 * A read that is not taken gives bases_r = 0 and status PGN_ERR_INVALID_ARG, and none of its frames is read;
 * read_frames is device data, so this per-read check is also what keeps every access inside the buffers.  A
 * caller may therefore decode the reads that are complete inside one stitched batch buffer.
 * Capacity.  A base with g >= base_capacity is not written to seq, base_frame or base_score.  A taken read with
 * bases_r > 0 and read_bases[r+1] > base_capacity gets PGN_ERR_DST_TOO_SMALL, every other taken read PGN_OK.
 * read_bases always holds the full counts, so read_bases[nreads] is the capacity that would have sufficed;
 * bases_r <= frames_r, so the frame count is the bound a host can take without a wait.
 * Codes.  d_codes[i - frame_base] is written for every frame of a taken read when the caller passes the
 * array (without it the codes live in context scratch).  Nothing else in any output is written.  If read_frames
 * does not ascend, the reads with read_frames[r] > read_frames[r+1] are not taken; the rest is unspecified,
 * except that no access leaves the window or the buffers.
 *
 * pgn_collapse_codes_device is the second half applied to the caller's codes, whatever made them: a frame
 * emits iff bit 7 of its code is set, and its base is alphabet[code & 0x7f] (128 entries).  Two emitting frames
 * in a row with the same class give two bases.  Taken reads, capacity, statuses and read_bases follow the rule
 * above; base_frame[g] = t.
 *
 * Both calls are asynchronous on `stream` with no host wait; their scratch lives on the context (16 bytes per
 * PGN_CTC_TILE_FRAMES frames of frame_capacity, and frame_capacity bytes for a decode without d_codes).
 * PGN_CTC_TILE_FRAMES is the number of frames one workgroup handles.
 *
 * PGN_ERR_INVALID_ARG before any GPU call, checking in this order: a NULL ctx, or NULL params (decode) or
 * alphabet (collapse); classes outside 2..64, blank >= classes, score_type not PGN_OUT_F32 or PGN_OUT_F16, or
 * pad != 0; frame_stride_bytes < C * the element size, or d_frames or frame_stride_bytes not a multiple of the
 * element size; nreads >= 2^32 or frame_capacity >= 2^40; a NULL d_read_bases; with nreads > 0 a NULL
 * d_read_frames or d_read_status; with frame_capacity > 0 a NULL d_frames (d_codes in the collapse call); with
 * base_capacity > 0 a NULL d_seq.  With nreads == 0 only d_read_bases[0] = 0 is written.
 * Not covered: transducer decoding and beam search; quality strings for this path (pgn_base_qual_device makes
 * them of posterior marginals, which a best-path CTC decode does not have); bfloat16 scores. */
#define PGN_CTC_TILE_FRAMES 1024
typedef struct pgn_ctc_params {
    uint32_t classes;       /* C, 2..64 */
    uint32_t blank;         /* < C */
    uint32_t score_type;    /* PGN_OUT_F32 or PGN_OUT_F16 */
    uint32_t pad;
    uint8_t  alphabet[64];  /* byte written for class c; the blank's entry is not used */
} pgn_ctc_params;

int pgn_ctc_decode_device(pgn_ctx *ctx, const pgn_ctc_params *params, size_t nreads,
                          const uint64_t *d_read_frames, const void *d_frames, uint64_t frame_stride_bytes,
                          uint64_t frame_base, uint64_t frame_capacity,
                          uint8_t *d_seq, uint64_t base_capacity, uint64_t *d_read_bases, int32_t *d_read_status,
                          uint32_t *d_base_frame /* may be NULL */, float *d_base_score /* may be NULL */,
                          uint8_t *d_codes /* may be NULL: context scratch is used */, void *stream);

int pgn_collapse_codes_device(pgn_ctx *ctx, const uint8_t alphabet[128], size_t nreads,
                              const uint64_t *d_read_frames, const uint8_t *d_codes, uint64_t frame_base,
                              uint64_t frame_capacity,
                              uint8_t *d_seq, uint64_t base_capacity, uint64_t *d_read_bases, int32_t *d_read_status,
                              uint32_t *d_base_frame /* may be NULL */, void *stream);

/* ---- Model rows to per-frame codes (CRF) ---------------------------------------------------------------
 * The best-path (Viterbi) decode of a CRF model's output, row by row as the model wrote it and before any
 * stitching: one code byte per frame, exactly the byte pgn_collapse_codes_device reads, so that
 *   segment -> model -> this call -> pgn_stitch_rows_device (frame_bytes = 1) -> pgn_collapse_codes_device
 * is a route to bases.  Every output is a selection among float32 sums formed in a fixed order, so the
 * tolerance is zero.  No outside source defines the rule, so this text does.
 *
 * Parameters (pgn_crf_params, 16 bytes): k = state_len in 1..5, so S = 4^k states; transitions is 5 or 4 and
 * C = transitions * S; score_type is PGN_OUT_F16 or PGN_OUT_F32, and float16 is used as its exact float32
 * value.  A state is a k-mer in base 4; its last digit s & 3 is the newest base.  The predecessor of s by
 * option b in 0..3 is
 *   p(s, b) = (b * S + s) >> 2      (drop s's newest base and put b on top).
 * Scores of frame t are x_t[0..C).  With transitions == 5, x_t[5s] is "stay in s" and x_t[5s + 1 + b] is
 * "move into s from p(s, b)".  With transitions == 4 the move score is x_t[4s + b] and every stay scores the
 * constant stay_score (models with a fixed blank score).  With transitions == 5, stay_score must be +0.0f
 * (bits zero): its role is that of a pad.
 *
 * Forward, all arithmetic in float32, one rounding per add:
 *   a_0[s] = 0.
 *   For t = 0..T-1 and every s:
 *     best = a_t[s] + stay, j = 0.
 *     For b = 0, 1, 2, 3 in that order: cand = a_t[p(s, b)] + move(t, s, b);
 *       if (cand > best) { best = cand; j = 1 + b; }
 *     a_{t+1}[s] = best, bp_t[s] = j.
 * The comparison is that C expression and nothing else.  A tie keeps the earlier option.  A NaN candidate
 * never replaces, and a NaN best is never replaced.
 * End: e = 0, m = a_T[0].  For s = 1..S-1: if (a_T[s] > m) { m = a_T[s]; e = s; }.  row_score = m, s_T = e.
 * Traceback, for t = T-1 .. 0:
 *   j = bp_t[s_{t+1}].
 *   code_t = (s_{t+1} & 3) | (j ? 0x80 : 0).
 *   s_t = j ? p(s_{t+1}, j - 1) : s_{t+1}.
 * code_t is the byte the collapse call reads: bit 7 is the move, the class below it is the base, and the
 * alphabet is "ACGT".  The first state's older bases are never emitted.  A joint between two rows may double or
 * lose a base there, as with any chunked decode; stitching cuts in the middle of the overlap for that reason.
 *
 * pgn_crf_viterbi_rows_device: frame t of row g is the C contiguous elements at
 *   d_rows + g * row_stride_bytes + t * frame_stride_bytes
 * (the convention of pgn_stitch_rows_device: it serves [N, T, C] and [T, N, C]), and row g's codes go to
 * d_codes + g * codes_row_stride + t.  The call is asynchronous on `stream` with no host wait.  Nothing but the
 * T code bytes per row and d_row_score[g] is written.  Any element-aligned pointer and strides are allowed;
 * 16-byte loads are used where the address allows them, and no byte outside the frames is read.
 *
 * Scratch is the backpointers; they live on the context:
 *   bytes per row = 4 * S * ceil(T / 8) + 16
 * (4 bits per state and frame, a dword per state and 8 frames, then the row's end state).
 * pgn_ctx_set_crf_scratch(ctx, bytes) sets a cap on it; the default is PGN_CRF_DEFAULT_SCRATCH (1 GiB) and 0
 * restores it.  The rows of one call are handled in successive groups of floor(cap / bytes per row) rows; the
 * groups are further launches on the same stream, with no host wait.  A single row that does not fit the cap is
 * PGN_ERR_INVALID_ARG.
 *
 * PGN_ERR_INVALID_ARG before any GPU call, checking in this order: a NULL ctx or params; state_len outside
 * 1..5, transitions not 4 or 5, score_type not PGN_OUT_F32 or PGN_OUT_F16, or stay_score bits non-zero with
 * transitions == 5; T == 0 or T > 2^24; frame_stride_bytes < C * the element size unless T == 1, or d_rows or
 * either stride not a multiple of the element size; codes_row_stride < T unless nrows <= 1; nrows >= 2^32; a
 * row that exceeds the scratch cap; with nrows > 0 a NULL d_rows or d_codes.  nrows == 0 returns PGN_OK and
 * touches nothing.  pgn_ctx_set_crf_scratch refuses a NULL ctx.
 * Not covered: beam search, posteriors and forward-backward; quality strings; bfloat16 scores; a decode that
 * stops at a short row's valid samples (padding frames are decoded, and the stitch drops them); alphabets
 * other than 4 bases.  That is this call's list: posteriors by forward-backward and the quality strings made of
 * them are calls of their own, "Posteriors and qualities (CRF)" below. */
#define PGN_CRF_DEFAULT_SCRATCH 1073741824ull
typedef struct pgn_crf_params {
    uint32_t state_len;     /* k, 1..5: S = 4^k states */
    uint32_t transitions;   /* 5 (stay + 4 moves per state) or 4 (moves only, stays score stay_score) */
    uint32_t score_type;    /* PGN_OUT_F32 or PGN_OUT_F16 */
    float    stay_score;    /* transitions == 4: the score of every stay; else +0.0f */
} pgn_crf_params;

int pgn_ctx_set_crf_scratch(pgn_ctx *ctx, uint64_t bytes);
int pgn_crf_viterbi_rows_device(pgn_ctx *ctx, const pgn_crf_params *params, uint64_t nrows, uint32_t T,
                                const void *d_rows, uint64_t row_stride_bytes, uint64_t frame_stride_bytes,
                                uint8_t *d_codes, uint64_t codes_row_stride, float *d_row_score /* may be NULL */,
                                void *stream);

/* ---- Posteriors and qualities (CRF) ---------------------------------------------------------------------
 * The posterior marginals of a CRF model's rows by a log-sum-exp forward-backward pass over the rows
 * pgn_crf_viterbi_rows_device reads, and, once both are stitched, one phred character per called base:
 *   segment -> model -> pgn_crf_viterbi_rows_device and pgn_crf_posterior_rows_device
 *     -> pgn_stitch_rows_device of the codes (frame_bytes = 1) and of the probabilities (frame_bytes = 16)
 *     -> pgn_collapse_codes_device -> pgn_base_qual_device
 * is a route to FASTQ records.  No outside source defines the rules, so this text does.
 *
 * pgn_crf_posterior_rows_device.  Parameters, states, p(s, b), stay and move(t, s, b) are those of "Model rows to
 * per-frame codes (CRF)".  With
 *   c(u, n) = ((u << 2) | n) & (S - 1)   and   top(u) = u >> (2k - 2)
 * (the state after u by a move that appends base n, and the base that move drops):
 *   Forward   a_0[s] = 0.
 *             a_{t+1}[s] = log( exp(a_t[s] + stay(t, s)) + sum_b exp(a_t[p(s, b)] + move(t, s, b)) ).
 *   Backward  b_T[s] = 0.
 *             b_t[u] = log( exp(stay(t, u) + b_{t+1}[u]) + sum_n exp(move(t, c(u, n), top(u)) + b_{t+1}[c(u, n)]) ).
 *   Marginal of the state after frame t
 *             g_t[s] = exp(a_{t+1}[s] + b_{t+1}[s]) / sum_s' exp(a_{t+1}[s'] + b_{t+1}[s']).
 *   Output    post[t][b] = sum over s with (s & 3) == b of g_t[s]:
 * the probability that the newest base of the state after frame t is b.  That state is the one whose newest base
 * the Viterbi call writes into code_t, so post[t][code_t & 3] is the called base's marginal.
 * Arithmetic is float32 with a renormalisation per frame: both recursions and the marginal do not change when a
 * constant is added to a whole vector, so each step subtracts element 0 of the vector it reads, and the stored
 * a_t and b_t stay near zero whatever T is (states differ by at most k moves' worth of score).  Every log-sum-exp
 * takes its largest term out first.  Unlike the other model calls this one has a tolerance: crf_posteriors_signal
 * (the package's numpy model) in float64 is the reference and its float32 form the yardstick; the device is held to
 * 4 times the float32 form's own error, measured as max |p - p64| / max(p64, 1e-6) with a floor of 2^-20.  The
 * domain is finite scores: for a row that holds a NaN or an infinity the values are unspecified, but no access
 * leaves the buffers and the call ends.
 *
 * Frame t of row g is read as in pgn_crf_viterbi_rows_device (both [N, T, C] and [T, N, C], float16 or float32,
 * any element-aligned pointer), and its four float32 values go to
 *   d_post + g * post_row_stride + 4 * t        (post_row_stride in floats).
 * Nothing else is written.  The call is asynchronous on `stream` with no host wait.
 *
 * Scratch is the forward vectors, one float32 per state and frame:
 *   bytes per row = 4 * S * T
 * on the context and under the cap of pgn_ctx_set_crf_scratch, which both calls share (as they share the memory).
 * Rows are handled in successive groups of floor(cap / bytes per row) on the same stream, with no host wait; a
 * single row above the cap is PGN_ERR_INVALID_ARG.  At k = 5 and T = 2,000 a row takes 8,192,000 bytes and the
 * default cap holds 131 rows, fewer than the device has compute units: raise the cap for such batches.
 *
 * PGN_ERR_INVALID_ARG before any GPU call, checking in the Viterbi call's order: a NULL ctx or params; the
 * parameter conditions; T == 0 or T > 2^24; frame_stride_bytes < C * the element size unless T == 1, or d_rows or
 * either stride not a multiple of the element size; post_row_stride < 4 * T unless nrows <= 1, or d_post not a
 * multiple of 4; nrows >= 2^32; a row that exceeds the scratch cap; with nrows > 0 a NULL d_rows or d_post.
 * nrows == 0 returns PGN_OK and touches nothing.
 *
 * pgn_base_qual_device.  Exact: integer sums and comparisons.  The window (frame_base, frame_capacity) and the
 * taken reads are those of pgn_collapse_codes_device, whose outputs for the same window the call reads:
 * d_read_bases, d_base_frame, d_read_status.  d_codes[i - frame_base] is frame i's code and
 * d_post + 4 * (i - frame_base) its four probabilities, as the rows call lays 16-byte frames.  A read gets output
 * iff it is taken, its status is PGN_OK and read_bases[r+1] <= base_capacity (and it has fewer than 2^32 frames,
 * which base_frame could not describe); for every other read nothing is read or written.
 * Base g of read r: t0 = base_frame[g]; t1 = base_frame[g+1] if g + 1 < read_bases[r+1], else the read's frame
 * count; n = t1 - t0.  With c = code_{t0} & 3, for every frame t in [t0, t1):
 *   err_t = (post[t][(c+1)&3] + post[t][(c+2)&3]) + post[t][(c+3)&3]       in float32, in that order
 *   u_t   = (uint64)trunc(clamp(err_t, 0, 1) * 2^32), clamped to 2^32 - 1; a NaN counts as 2^32 - 1.
 *   U = sum of u_t (uint64; it cannot wrap), and
 *   qual[g] = 33 + q_min + #{ j < nthresholds : U <= (uint64)thr[j] * n }.
 * The sum has no order, so any split of a long block gives the same byte.  Frames before a read's first base belong
 * to no base.  Parameters (pgn_qual_params): q_min + nthresholds <= 93 and thr non-increasing, else
 * PGN_ERR_INVALID_ARG.  thr[j] is the mean error, in units of 2^-32, at or below which a base earns q_min + j + 1:
 * the package's qual_thresholds builds floor(2^32 * 10^(-((q_min + j + 0.5) - q_shift) / (10 * q_scale))), the
 * points where q_shift + q_scale * (-10 log10 err) rounds up.
 * PGN_ERR_INVALID_ARG before any GPU call, in this order: a NULL ctx or params; the parameter conditions;
 * nreads >= 2^32 or frame_capacity >= 2^40; d_post not a multiple of 4; with nreads > 0 a NULL d_read_frames,
 * d_read_bases or d_read_status; with frame_capacity > 0 a NULL d_codes or d_post; with base_capacity > 0 a NULL
 * d_base_frame or d_qual.  nreads == 0 returns PGN_OK and touches nothing.  Asynchronous, no host wait, no scratch.
 *
 * Not covered: beam search; a row's log partition function; per-read mean quality; bfloat16; alphabets other than
 * 4 bases; qualities for the CTC path; a checkpointed backward pass (a third read of the scores for a sixteenth of
 * the scratch). */
typedef struct pgn_qual_params {
    uint32_t q_min;         /* the quality of a base no threshold admits */
    uint32_t nthresholds;   /* q_min + nthresholds <= 93 */
    uint32_t thr[93];       /* non-increasing over the first nthresholds; the rest is not read */
} pgn_qual_params;

int pgn_crf_posterior_rows_device(pgn_ctx *ctx, const pgn_crf_params *params, uint64_t nrows, uint32_t T,
                                  const void *d_rows, uint64_t row_stride_bytes, uint64_t frame_stride_bytes,
                                  float *d_post, uint64_t post_row_stride, void *stream);

int pgn_base_qual_device(pgn_ctx *ctx, const pgn_qual_params *params, size_t nreads, const uint64_t *d_read_frames,
                         const uint8_t *d_codes, const float *d_post, uint64_t frame_base, uint64_t frame_capacity,
                         const uint64_t *d_read_bases, const uint32_t *d_base_frame, const int32_t *d_read_status,
                         uint8_t *d_qual, uint64_t base_capacity, void *stream);

/* ---- FASTQ records ------------------------------------------------------------------------------------------
 * The last two steps of the route above:
 *   ... -> pgn_collapse_codes_device -> pgn_base_qual_device -> pgn_read_qual_device -> pgn_fastq_records_device
 * A read's mean quality with a pass flag, and the kept reads as FASTQ text in one device buffer with per-read
 * offsets, so that the result goes to a file with one download and one write().  Both rules are integer and byte
 * rules: the tolerance is zero.  No outside source defines the rule, so this text does.
 *
 * pgn_read_qual_device.  d_read_bases (nreads + 1, non-decreasing) and d_read_status are what
 * pgn_collapse_codes_device left, d_qual what pgn_base_qual_device wrote, base_capacity the size of d_qual.
 * A read "has input" iff its status is PGN_OK, read_bases[r] <= read_bases[r+1] <= base_capacity and
 *   m = read_bases[r+1] - read_bases[r] > 0.
 * For a read with input:
 *   s = skip_bases if m > skip_bases else 0, and n = m - s
 * (the leading bases of a read are the adapter's neighbours, and basecallers leave them out of the mean);
 *   U = sum over g in [s, m) of err[min(max(qual[read_bases[r] + g], 33), 126) - 33]      (uint64; n < 2^32, so
 *       it cannot wrap)
 *   mean_q[r] = q_min + #{ j < nthresholds : U <= (uint64)thr[j] * n }
 *   pass[r] = mean_q[r] >= min_mean_q                                                      (1 or 0)
 * and err_sum[r] = U.  For every other read mean_q = 0, err_sum = 0 and pass = 0.  All three arrays are written for
 * every read, so they are defined after the call; d_err_sum may be NULL.  d_mean_q is uint32 so that it can be a tag
 * column of the record call.  Parameters (pgn_read_qual_params): `mean` holds q_min, nthresholds and thr with the
 * conditions of pgn_base_qual_device; err[q] is the error of phred character 33 + q in units of 2^-32: the
 * package's err_table builds err[q] = min(2^32 - 1, rint(2^32 * 10^(-q/10))), and qual_thresholds builds thr.  The
 * comparison is the one pgn_base_qual_device uses; the mean is of error probabilities, not of qualities.
 * The work is flat over the bases in tiles of PGN_READ_QUAL_TILE_BASES, tile k being bases [k * tile, (k+1) * tile)
 * of d_qual; the sum is of integers, so its split over tiles changes nothing.  If d_read_bases decreases anywhere
 * the three outputs are unspecified, but no access leaves the buffers and the call ends.
 * PGN_ERR_INVALID_ARG before any GPU call, in this order: a NULL ctx or params; the `mean` conditions;
 * nreads >= 2^32; with nreads > 0 a NULL d_read_bases, d_read_status, d_mean_q or d_pass; with base_capacity > 0 a
 * NULL d_qual.  nreads == 0 returns PGN_OK and touches nothing.  Asynchronous on `stream`, no host wait; the
 * scratch, when d_err_sum is NULL, is 8 bytes per read on the context.
 *
 * pgn_fastq_records_device.  A read is kept iff its status is PGN_OK, read_bases[r] <= read_bases[r+1] <=
 * base_capacity, m > 0, and d_keep is NULL or d_keep[r] != 0.  d_keep is `pass` of the call above or anything of
 * the caller's: the complement of a mask writes the fail file with a second call.
 * Record of a kept read, byte for byte:
 *   '@' uuid { '\t' name0 name1 ':' 'i' ':' dec(tag_k[r]) } '\n' SEQ '\n' '+' '\n' QUAL '\n'
 * uuid: the 36 characters of d_read_ids[16 r ..], the 16 bytes in order as lowercase hex with '-' after bytes 4, 6,
 * 8 and 10 (Python's str(uuid.UUID(bytes=...))).  Tags: ntags <= PGN_FASTQ_MAX_TAGS columns k = 0 .. ntags - 1 in
 * order, each a two-byte name ([A-Za-z][A-Za-z0-9]) and a device array of nreads uint32, the value written in
 * decimal without leading zeros.  SEQ / QUAL: the read's m bytes of d_seq / d_qual; with PGN_FASTQ_REVERSE in flags
 * both are written in reverse order (direct RNA reads are sequenced 3' to 5'; the alphabet is
 * pgn_collapse_codes_device's business).
 *   length of a kept read's record = 42 + 2m + sum_k (6 + digits(tag_k[r])); a read that is not kept has length 0.
 * d_rec_off (nreads + 1, uint64) is the exclusive scan of the lengths.  It always holds the full counts, so
 * rec_off[nreads] is the capacity that would have sufficed.  A kept read with rec_off[r+1] > byte_capacity gets
 * rec_status PGN_ERR_DST_TOO_SMALL and no byte of it is written: there are no partial records.  A kept read that
 * is written gets PGN_OK, its record at d_out + rec_off[r].  A read that is not kept gets its own status if that is
 * non-zero, else PGN_OK.  Nothing outside the written records is touched, and no byte outside the kept reads'
 * [read_bases[r], read_bases[r+1]) ranges of d_seq and d_qual, their ids and their tag entries is read.
 *   fastq_bound(nreads, nbases, ntags) = nreads * (42 + 16 * ntags) + 2 * nbases
 * gives the host a capacity without a wait.  d_out may have any alignment.  The writer is flat over the output
 * bytes: a workgroup owns the PGN_FASTQ_TILE_BYTES bytes between two addresses that are multiples of that constant
 * apart, counted from d_out rounded down to 16, so with d_out a multiple of 16 the seams lie at the output offsets
 * k * PGN_FASTQ_TILE_BYTES.
 * PGN_ERR_INVALID_ARG before any GPU call, in this order: a NULL ctx or params; unknown flag bits; ntags >
 * PGN_FASTQ_MAX_TAGS or a bad name among the first ntags; nreads >= 2^32; with nreads > 0 a NULL d_read_ids,
 * d_read_bases, d_read_status, d_rec_status, or a NULL d_tag[k] for k < ntags; a NULL d_rec_off; with
 * base_capacity > 0 a NULL d_seq or d_qual; with byte_capacity > 0 a NULL d_out.  nreads == 0 writes
 * rec_off[0] = 0 only.  Asynchronous on `stream`, no host wait; the scratch is 8 bytes per 1,024 reads.
 *
 * Not covered: SAM/uBAM output, and the move-table tag; a float qs:f: tag; compression of the text; pass and fail
 * files from one call; records for the CTC path's bases without qualities; signed or 64-bit tag values; splitting
 * of reads.  The text leaves compressed through pgn_bgzf_deflate_device ("BGZF deflate" below). */
#define PGN_READ_QUAL_TILE_BASES 4096u
#define PGN_FASTQ_TILE_BYTES 16384u
#define PGN_FASTQ_MAX_TAGS 8u
#define PGN_FASTQ_REVERSE 1u

typedef struct pgn_read_qual_params {
    pgn_qual_params mean;   /* q_min, nthresholds, thr: as for pgn_base_qual_device */
    uint32_t skip_bases;    /* leading bases left out of the mean of a read longer than this */
    uint32_t min_mean_q;    /* pass = mean_q >= min_mean_q */
    uint32_t err[94];       /* the error of phred character 33 + q in units of 2^-32 */
} pgn_read_qual_params;

typedef struct pgn_fastq_params {
    uint32_t flags;                 /* PGN_FASTQ_REVERSE or 0 */
    uint32_t ntags;                 /* <= PGN_FASTQ_MAX_TAGS */
    uint8_t  tag_name[8][2];        /* [A-Za-z][A-Za-z0-9] for the first ntags; the rest is not read */
    const uint32_t *d_tag[8];       /* nreads values each for the first ntags; the rest is not read */
} pgn_fastq_params;

int pgn_read_qual_device(pgn_ctx *ctx, const pgn_read_qual_params *params, size_t nreads,
                         const uint64_t *d_read_bases, const int32_t *d_read_status, const uint8_t *d_qual,
                         uint64_t base_capacity, uint32_t *d_mean_q, uint64_t *d_err_sum /* may be NULL */,
                         uint8_t *d_pass, void *stream);

int pgn_fastq_records_device(pgn_ctx *ctx, const pgn_fastq_params *params, size_t nreads, const uint8_t *d_read_ids,
                             const uint64_t *d_read_bases, const int32_t *d_read_status,
                             const uint8_t *d_keep /* may be NULL */, const uint8_t *d_seq, const uint8_t *d_qual,
                             uint64_t base_capacity, uint8_t *d_out, uint64_t byte_capacity, uint64_t *d_rec_off,
                             int32_t *d_rec_status, void *stream);

/* ---- BAM records --------------------------------------------------------------------------------------------
 * The other end of the same route: the kept reads as unaligned BAM records with the move table, laid out raw or
 * in BGZF blocks, so that the file is header + one download per batch + the end marker.
 *   ... -> pgn_base_qual_device -> pgn_read_qual_device -> pgn_bam_records_device
 * The rule is the SAM/BAM specification's (SAMv1 section 4.2 for the record, 4.1 for BGZF); no outside program
 * defines the bytes here, so this text does.  Integers and bytes alone: the tolerance is zero.
 *
 * pgn_bam_records_device.  The inputs are those of pgn_fastq_records_device, and for the move table d_read_frames
 * (nreads + 1), d_codes, frame_base and frame_capacity with the window meaning they have in pgn_base_qual_device:
 * d_codes[i - frame_base] is frame i's code.  A read is kept iff its status is PGN_OK, read_bases[r] <=
 * read_bases[r+1] <= base_capacity, m > 0, and d_keep is NULL or d_keep[r] != 0.  With PGN_BAM_MOVES a read that
 * would be kept must also have its frames [read_frames[r], read_frames[r+1]) inside [frame_base, frame_base +
 * frame_capacity), and F = read_frames[r+1] - read_frames[r] < 2^31 of them; a read that fails either is not kept
 * and gets PGN_ERR_INVALID_ARG.
 * Record of a kept read, little-endian, byte for byte:
 *   block_size u32 = the record's length minus 4
 *   refID i32 = -1, pos i32 = -1, l_read_name u8 = 37, mapq u8 = 0, bin u16 = 4680, n_cigar_op u16 = 0,
 *   flag u16 = 4, l_seq u32 = m, next_refID i32 = -1, next_pos i32 = -1, tlen i32 = 0
 *   read_name: the 36 uuid characters of the FASTQ rule, then NUL.  No CIGAR.
 *   seq: (m + 1) / 2 bytes, base 2i in the high nibble and base 2i+1 in the low nibble, the low nibble of the
 *     last byte of an odd read 0; a nibble is the position of the upper-cased character in "=ACMGRSVTWYHKDBN",
 *     and 15 for any other byte.
 *   qual: m bytes, min(max(q, 33), 126) - 33; with d_qual == NULL every byte is 0xFF.
 *   tags: for each column k < ntags, name0 name1 'I' and the uint32 (7 bytes); with PGN_BAM_MOVES, last,
 *     'm' 'v' 'B' 'c', u32 count 1 + F, stride as int8, then F bytes (codes[read_frames[r] - frame_base + f] >> 7) & 1.
 * PGN_BAM_REVERSE reverses the order of bases and of qualities before packing.  The move table stays in signal
 * order: it is not reversed.
 *   block_size of a kept read = 69 + (m + 1) / 2 + m + 7 * ntags + (moves ? 9 + F : 0),
 *   length of its record = block_size + 4, at least 75; a read that is not kept has length 0.
 * The length depends on m, F and ntags alone.  d_rec_off (nreads + 1, uint64) is the exclusive scan of the lengths
 * and always holds the full counts.  A kept read whose record ends above the stream capacity gets
 * PGN_ERR_DST_TOO_SMALL and no byte: there are no partial records.  The offsets are non-decreasing, so the written
 * records are a prefix of the stream; W, the largest rec_off[r+1] within the capacity, is d_written[0].  A kept read
 * that is written gets PGN_OK; a read that is not kept its own status, or PGN_ERR_INVALID_ARG as above.
 * Two layouts:
 *   Raw (without PGN_BAM_BGZF): stream byte o is d_out[o], the stream capacity is byte_capacity, d_written[1] = W.
 *   PGN_BAM_BGZF: the stream is cut every PGN_BGZF_BLOCK_BYTES = 65,280 bytes (htslib's 0xff00).  Stream byte o is
 *     d_out[(o / 65280) * 65311 + 23 + o % 65280].  Block k < ceil(W / 65280) with payload length n gets the header
 *       1f 8b 08 04 00 00 00 00 00 ff 06 00 42 43 02 00, BSIZE = n + 30 as u16,
 *     the stored-deflate prefix 01, n as u16, ~n as u16, and behind the payload CRC32(payload) (the zlib polynomial,
 *     reflected 0xEDB88320) and n, both u32.  The stream capacity is the largest S with S + 31 * ceil(S / 65280) <=
 *     byte_capacity; d_written[1] = W + 31 * ceil(W / 65280).  W == 0 writes no block; the last block is short.
 *     The records of one call form a self-contained run of blocks, so batches concatenate behind a BGZF block
 *     with the BAM header and in front of the 28-byte end marker, which the caller writes.
 * Nothing at or beyond d_out + d_written[1] is touched, and nothing in front of d_out; d_out may have any alignment.
 *   bam_bound(nreads, nbases, ntags, nframes) = nreads * (74 + 7 * ntags) + nbases + nbases / 2 [+ 9 * nreads + nframes]
 *   bgzf_bound(nbytes) = nbytes + 31 * ceil(nbytes / 65280)
 * give the host a capacity without a wait.  The writer is flat over the stream, a workgroup per 65,280 stream bytes
 * in either layout; with PGN_BAM_BGZF it checksums the block it holds in LDS before it stores it.
 * PGN_ERR_INVALID_ARG before any GPU call, in this order: a NULL ctx or params; unknown flag bits; ntags >
 * PGN_BAM_MAX_TAGS or a bad name among the first ntags ([A-Za-z][A-Za-z0-9]); with PGN_BAM_MOVES a stride outside
 * 1..127; nreads >= 2^32; with nreads > 0 a NULL d_read_ids, d_read_bases, d_read_status, d_rec_status, a NULL
 * d_tag[k] for k < ntags, or with PGN_BAM_MOVES a NULL d_read_frames; a NULL d_rec_off or d_written; with
 * base_capacity > 0 a NULL d_seq; with PGN_BAM_MOVES and frame_capacity > 0 a NULL d_codes; with byte_capacity > 0
 * a NULL d_out.  d_qual may be NULL; d_codes and d_read_frames may be NULL without PGN_BAM_MOVES.  nreads == 0
 * writes rec_off[0] = 0 and d_written = {0, 0} only.  Asynchronous on `stream`, no host wait; the scratch is 8 bytes
 * per 1,024 reads.
 *
 * Not covered: deflate compression (every block holds a stored deflate block, as `samtools view -u` writes);
 * aligned records and reference headers; qs:f and other non-uint32 tags; a reversed move table; SAM text; BGZF
 * framing of other buffers.  Both are pgn_bgzf_deflate_device's ("BGZF deflate" below), which reads the raw layout. */
#define PGN_BAM_MAX_TAGS 8u
#define PGN_BAM_REVERSE 1u
#define PGN_BAM_MOVES 2u
#define PGN_BAM_BGZF 4u
#define PGN_BGZF_BLOCK_BYTES 65280u

typedef struct pgn_bam_params {
    uint32_t flags;                 /* PGN_BAM_REVERSE | PGN_BAM_MOVES | PGN_BAM_BGZF */
    uint32_t ntags;                 /* <= PGN_BAM_MAX_TAGS */
    uint8_t  tag_name[8][2];        /* [A-Za-z][A-Za-z0-9] for the first ntags; the rest is not read */
    const uint32_t *d_tag[8];       /* nreads values each for the first ntags; the rest is not read */
    uint32_t stride;                /* 1..127 with PGN_BAM_MOVES: the model's stride, the move table's first entry */
    uint32_t pad;
} pgn_bam_params;

int pgn_bam_records_device(pgn_ctx *ctx, const pgn_bam_params *params, size_t nreads, const uint8_t *d_read_ids,
                           const uint64_t *d_read_bases, const int32_t *d_read_status,
                           const uint8_t *d_keep /* may be NULL */, const uint8_t *d_seq,
                           const uint8_t *d_qual /* may be NULL */, uint64_t base_capacity,
                           const uint64_t *d_read_frames, const uint8_t *d_codes, uint64_t frame_base,
                           uint64_t frame_capacity, uint8_t *d_out, uint64_t byte_capacity, uint64_t *d_rec_off,
                           int32_t *d_rec_status, uint64_t *d_written, void *stream);

/* ---- BGZF deflate -------------------------------------------------------------------------------------------
 * Any device byte stream in BGZF blocks that each hold one Huffman-only dynamic deflate block, or a stored block
 * where that is not smaller, packed end to end: the raw records of pgn_bam_records_device (without PGN_BAM_BGZF),
 * the text of pgn_fastq_records_device, anything else.
 *   ... -> pgn_bam_records_device (raw) | pgn_fastq_records_device -> pgn_bgzf_deflate_device
 * The container is SAMv1 section 4.1's and the bit stream RFC 1951's; which of the many valid streams is written no
 * outside program defines, so this text does.  Integers and bits alone: the tolerance is zero.
 *
 * The stream.  Its length is W = min(*d_nbytes, src_capacity), and W = src_capacity with d_nbytes == NULL.  It is cut
 * every PGN_BGZF_BLOCK_BYTES = 65,280 bytes: block k < nblocks = ceil(W / 65280) has a payload p of n bytes, 1 <= n <=
 * 65280.
 * The file bytes of block k: the 16 header bytes of "BAM records", BSIZE as u16 = the block's total length minus 1,
 * the deflate bytes, CRC32(p) as u32, n as u32.
 * The deflate bytes are the dynamic block below if its byte length is < n + 5, else the stored block 01 n ~n p (n and
 * ~n as u16).  A tie stores.
 * The dynamic block.  Bits fill each byte from bit 0 upwards.
 *   Counts: cnt[s] for s < 256 is the number of payload bytes equal to s; cnt[256] = 1, the end-of-block symbol.
 *   ll = lengths(cnt, 15) over the 257 symbols.
 *   Header bits, in this order: BFINAL = 1 in 1 bit; BTYPE = 2 in 2 bits; HLIT = 0 in 5 bits (257 codes); HDIST = 1 in
 *   5 bits (two distance codes, both of length 1 and never used, as zlib writes them, so every inflater reads it);
 *   HCLEN - 4 in 4 bits.
 *   The length sequence has 259 entries: ll[0..256], 1, 1.  It is cut into maximal runs of equal values over the whole
 *   sequence (a run may join ll[256] and the two trailing ones).
 *   A run of r zeros: while r >= 11, symbol 18 with t = min(r, 138), extra value t - 11 in 7 bits, r -= t; then if
 *   r >= 3, symbol 17 with r - 3 in 3 bits; otherwise r literal zeros.
 *   A run of r values v > 0: v once, r -= 1; while r >= 3, symbol 16 with t = min(r, 6), extra value t - 3 in 2 bits,
 *   r -= t; then r literal v.
 *   cl = lengths(histogram of those symbols, 7) over the 19 code-length symbols.
 *   HCLEN is the position of the last non-zero cl in the order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, plus
 *   one, and at least 4; that many lengths follow, 3 bits each.  Then the symbols, each followed by its extra bits.
 *   Then the n literals' codes and the code of symbol 256.
 *   Codes are canonical (RFC 1951 section 3.2.2) and written from their most significant bit; extra bits from their
 *   least significant bit.  The last byte is padded with zeros.
 * lengths(cnt, L).  The used symbols (cnt > 0), sorted by (cnt, symbol) ascending, are the leaf queue; internal nodes
 * queue in creation order.  Each step takes the two smallest weights from the fronts of the two queues, the leaf where
 * its weight is <= the internal node's; the new node's weight is their sum.  A symbol's length is its leaf's depth.
 * One used symbol alone gets length 1.  If the largest length exceeds L, the limiter:
 *   1. every length above L becomes L; 2. K = sum 2^(L - len);
 *   3. while K > 2^L: among the used symbols with len < L take the longest length, then the smallest count, then the
 *      largest symbol, and give it one more bit;
 *   4. D = 2^L - K; 5. while D > 0: among the used symbols with len > 1 and 2^(L - len) <= D take the largest count,
 *      then the smallest symbol, subtract that 2^(L - len) from D and take one bit from the symbol.
 * Layout and capacity.  d_blk_off[0 .. ntiles], ntiles = ceil(src_capacity / 65280), is the exclusive scan of the
 * blocks' file lengths and always holds the full counts; entries above nblocks repeat the total.  Block k is written
 * iff blk_off[k + 1] <= byte_capacity, so the written blocks are a prefix; call their number kw.  d_written[0] =
 * min(W, 65280 * kw) is the stream bytes consumed, d_written[1] = blk_off[kw].  There are no partial blocks.  Nothing
 * at or beyond d_out + d_written[1] is touched, and nothing in front of d_out; d_src and d_out may have any alignment.
 * bgzf_bound(src_capacity) always suffices, because a block is never longer than its stored form.  W == 0 writes no
 * block.  The blocks of one call are a self-contained run, so batches concatenate in front of the 28-byte end marker.
 * Three kernels: a workgroup per block counts, checksums and builds both codes (the plan); the scan of the lengths;
 * a workgroup per block writes the bits into an image in LDS and stores it (the pack).  No match search.
 * PGN_ERR_INVALID_ARG before any GPU call, in this order: a NULL ctx; flags != 0; with src_capacity > 0 a NULL d_src; a
 * NULL d_blk_off or d_written; with byte_capacity > 0 a NULL d_out; src_capacity >= 2^48.  src_capacity == 0 writes
 * blk_off[0] = 0 and d_written = {0, 0} only.  Asynchronous on `stream`, no host wait; the scratch is 1,568 bytes per
 * block of src_capacity (the header's bits, the 257 codes and the CRC between the plan and the pack).
 *
 * Not covered: a match search, so the output is Huffman only; several deflate blocks per BGZF block; fixed-Huffman
 * blocks; a .gzi or .bai index from blk_off; fusing into the record writers; decompression. */
int pgn_bgzf_deflate_device(pgn_ctx *ctx, uint32_t flags /* 0 */, const uint8_t *d_src, uint64_t src_capacity,
                            const uint64_t *d_nbytes /* may be NULL */, uint8_t *d_out, uint64_t byte_capacity,
                            uint64_t *d_blk_off, uint64_t *d_written, void *stream);

/* ---- Adapters and barcodes ----------------------------------------------------------------------------------
 * The step between "bases" and "records": where the adapter, primer and barcode sequences lie at the two ends of
 * each read, which barcode the read carries, and the read cut to what lies between, with its qualities and its
 * move table.
 *   ... -> pgn_collapse_codes_device -> pgn_find_patterns_device -> pgn_classify_reads_device
 *       -> pgn_trim_reads_device -> pgn_base_qual_device ... pgn_bam_records_device | pgn_fastq_records_device
 * No outside program defines the rule, so this text does.  Integers and bytes alone: the tolerance is zero.
 * Throughout, a read is taken iff its status is PGN_OK, read_bases[r] <= read_bases[r+1] <= base_capacity and
 * m = read_bases[r+1] - read_bases[r] > 0.  PGN_DEMUX_NONE = 0xFFFFFFFF stands for "no value".
 *
 * pgn_find_patterns_device.  The reads are those pgn_collapse_codes_device or pgn_ctc_decode_device leave (d_seq,
 * d_read_bases with nreads + 1 entries, d_read_status, base_capacity).  The P = npatterns patterns are device
 * arrays: d_pat holds their bytes end to end in pat_capacity bytes, pattern p is d_pat[pat_off[p] .. pat_off[p+1])
 * (d_pat_off has P + 1 entries), d_pat_side[p] is 0 for the head and 1 for the tail, d_max_dist[p] the largest
 * distance that is a hit.  A pattern is searched iff its side is 0 or 1, pat_off[p] < pat_off[p+1] <= pat_capacity
 * and its length L = pat_off[p+1] - pat_off[p] <= 128; the arrays are device data, so this check is also what keeps
 * every access inside d_pat.
 *   Text      of a taken read for a head pattern: its first n = min(m, window) bases, w0 = 0; for a tail pattern its
 *             last n bases, w0 = m - n.
 *   Match     pattern byte x matches text byte y iff x == 'N' or x == y.  Bytes are compared as they are: no case
 *             folding, and IUPAC codes other than 'N' are plain bytes ('N' in the text matches 'N' in the pattern
 *             alone).
 *   Distance  unit costs, the pattern global and the text local: D[0][j] = 0, D[i][0] = i,
 *               D[i][j] = min(D[i-1][j-1] + !match(p_i, t_j), D[i-1][j] + 1, D[i][j-1] + 1),
 *             dist = min over j in 0..n of D[L][j], end = w0 + the lowest j that attains it.  So dist <= L, and a
 *             pattern that matches nowhere gives dist = L and end = w0.
 *   Start     is computed iff dist <= max_dist[p] (a hit): with the reversed pattern and the text t[0:j] reversed,
 *             R[0][q] = q, R[i][0] = i and the same recurrence, q* is the lowest q with R[L][q] == dist (it exists),
 *             and start = end - q*: the shortest span that ends at end, which is the largest start.  Without a hit
 *             start = PGN_DEMUX_NONE.
 * d_dist, d_start and d_end are uint32 [nreads, P], a row per read; positions count bases from the read's start
 * (modulo 2^32).  A read that is not taken, and a pattern that is not searched, get PGN_DEMUX_NONE in all three.
 * Nothing else is written, and no byte of d_seq outside the taken reads' windows is read.  A workgroup takes one
 * (read, side) with the window in LDS and a lane per pattern (Myers' bit-vector recurrence, the column in two
 * 64-bit words); the scratch is 12 bytes per pattern, a per-side index built once per call.
 * PGN_ERR_INVALID_ARG before any GPU call, in this order: a NULL ctx; window outside 1..PGN_DEMUX_MAX_WINDOW or
 * npatterns outside 1..PGN_DEMUX_MAX_PATTERNS; nreads >= 2^32; a NULL d_pat_off, d_pat_side or d_max_dist; with
 * pat_capacity > 0 a NULL d_pat; with nreads > 0 a NULL d_read_bases, d_read_status, d_dist, d_start or d_end; with
 * base_capacity > 0 a NULL d_seq.  nreads == 0 returns PGN_OK and touches nothing.
 *
 * pgn_classify_reads_device.  d_dist, d_start, d_end as the search left them; d_pat_class[p] is a class below
 * nclasses, or PGN_PATTERN_NO_CLASS for an adapter or primer; any other value is a pattern that never hits.
 *   A pattern hits a taken read iff its side is 0 or 1 and dist <= max_dist[p] (PGN_DEMUX_NONE is no distance).
 *   d_c is the lowest dist among the hits of class c, absent without one.  best is the class with the lowest d_c,
 *   ties to the lowest c; second is the lowest d_c among the other classes.
 *   barcode[r] = best iff best exists and (second is absent or d_second - d_best >= min_sep), else PGN_DEMUX_NONE.
 *   The trimming hits are the hits whose class is PGN_PATTERN_NO_CLASS or equals barcode[r].  lo is the largest end
 *   among the trimming head hits, 0 without one; hi is the smallest start among the trimming tail hits, m without
 *   one.  If lo >= hi the read stays whole: lo = 0, hi = m.
 * Outputs, uint32 per read: d_barcode, d_best_dist, d_second_dist (PGN_DEMUX_NONE where absent), d_lo, d_hi.  A read
 * that is not taken gets PGN_DEMUX_NONE, PGN_DEMUX_NONE, PGN_DEMUX_NONE, 0, 0.  A thread per read; no scratch.
 * Per-barcode files need nothing more: keep = (barcode == c) is the d_keep of the record writers, and barcode fits
 * their uint32 tag columns.
 * PGN_ERR_INVALID_ARG before any GPU call, in this order: a NULL ctx; npatterns outside 1..PGN_DEMUX_MAX_PATTERNS;
 * nreads >= 2^32; a NULL d_pat_side, d_max_dist or d_pat_class; with nreads > 0 a NULL d_read_bases, d_read_status,
 * d_dist, d_start, d_end, d_barcode, d_best_dist, d_second_dist, d_lo or d_hi.  nreads == 0 touches nothing.
 *
 * pgn_trim_reads_device.  Bases [lo, hi) of every read, with its qualities (d_qual may be NULL) and, when
 * d_read_frames is not NULL ("with moves"), its move table: d_base_frame as pgn_collapse_codes_device leaves it, and
 * d_read_frames, d_codes, frame_base and frame_capacity with the meaning they have in pgn_bam_records_device.
 *   A read is sliced iff it is taken and lo <= hi <= m; with moves its frames [read_frames[r], read_frames[r+1])
 *   must also lie inside [frame_base, frame_base + frame_capacity), F of them, and with
 *     f_lo = base_frame[lo] if lo < hi, else 0;  f_hi = base_frame[hi] if lo < hi < m, F if lo < hi == m, else 0
 *   (base_frame counted from the read's first base) it must hold that f_lo <= f_hi <= F, so no access leaves the
 *   buffers whatever base_frame holds.  A read that fails has length 0 and keeps its status if that is not PGN_OK,
 *   else gets PGN_ERR_INVALID_ARG.
 *   d_new_read_bases (nreads + 1) is the exclusive scan of hi - lo; new base j of read r is old base lo + j, for seq
 *   and qual.  With moves d_new_read_frames is the scan of f_hi - f_lo, the new codes are the old frames [f_lo,
 *   f_hi) of the read, new base_frame = old - f_lo, and d_trim_frames[r] = f_lo (0 for a read that is not sliced):
 *   times the stride, the samples to add to the read's ts.  The first kept base then emits at frame 0, and the kept
 *   codes hold hi - lo emitting frames when base_frame is that of the codes.
 *   Both scans always hold the full counts.  A base at or above new_base_capacity and a frame at or above
 *   new_frame_capacity is not written, and a sliced read with bases or frames there gets PGN_ERR_DST_TOO_SMALL; every
 *   other sliced read PGN_OK (the rule of pgn_ctc_decode_device).  Nothing else is written.
 * The lengths, the scan of 1,024-read totals and the offsets as in the record writers; a flat copy over the output
 * serves seq, qual and codes, a 4-byte form base_frame.  The scratch is 16 bytes per 1,024 reads.
 * PGN_ERR_INVALID_ARG before any GPU call, in this order: a NULL ctx; nreads >= 2^32; a NULL d_new_read_bases; with
 * moves a NULL d_new_read_frames; with nreads > 0 a NULL d_read_bases, d_read_status, d_lo, d_hi or d_new_status,
 * and with moves a NULL d_trim_frames; with base_capacity > 0 a NULL d_seq, and with moves a NULL d_base_frame; with
 * moves and frame_capacity > 0 a NULL d_codes; with new_base_capacity > 0 a NULL d_new_seq, with d_qual a NULL
 * d_new_qual, with moves a NULL d_new_base_frame; with moves and new_frame_capacity > 0 a NULL d_new_codes.  With
 * nreads == 0 only new_read_bases[0] = 0 and, with moves, new_read_frames[0] = 0 are written.
 *
 * All three calls are asynchronous on `stream` with no host wait.
 * Not covered: a BC:Z string tag (barcode goes into a uint32 tag column); two-stage flank-then-barcode scoring and
 * a both-ends requirement; adapters in the middle of a read and read splitting; affine gaps or scores other than
 * unit costs; IUPAC classes beyond 'N'; patterns above 128 bytes or windows above 1,024; trimming inside the record
 * writers; reversed (direct RNA) coordinates, for which the caller swaps the sides; kit definitions: the caller
 * supplies the sequences. */
#define PGN_DEMUX_NONE 0xFFFFFFFFu
#define PGN_PATTERN_NO_CLASS 0xFFFFFFFFu
#define PGN_DEMUX_MAX_WINDOW 1024u
#define PGN_DEMUX_MAX_PATTERNS 4096u
#define PGN_DEMUX_MAX_PATTERN_BYTES 128u

int pgn_find_patterns_device(pgn_ctx *ctx, size_t nreads, const uint8_t *d_seq, const uint64_t *d_read_bases,
                             const int32_t *d_read_status, uint64_t base_capacity, uint32_t window, uint32_t npatterns,
                             const uint8_t *d_pat, uint64_t pat_capacity, const uint32_t *d_pat_off,
                             const uint8_t *d_pat_side, const uint32_t *d_max_dist, uint32_t *d_dist, uint32_t *d_start,
                             uint32_t *d_end, void *stream);

int pgn_classify_reads_device(pgn_ctx *ctx, size_t nreads, const uint64_t *d_read_bases, const int32_t *d_read_status,
                              uint64_t base_capacity, uint32_t npatterns, const uint8_t *d_pat_side,
                              const uint32_t *d_max_dist, const uint32_t *d_pat_class, uint32_t nclasses,
                              uint32_t min_sep, const uint32_t *d_dist, const uint32_t *d_start, const uint32_t *d_end,
                              uint32_t *d_barcode, uint32_t *d_best_dist, uint32_t *d_second_dist, uint32_t *d_lo,
                              uint32_t *d_hi, void *stream);

int pgn_trim_reads_device(pgn_ctx *ctx, size_t nreads, const uint8_t *d_seq, const uint8_t *d_qual /* may be NULL */,
                          const uint64_t *d_read_bases, const int32_t *d_read_status, uint64_t base_capacity,
                          const uint32_t *d_lo, const uint32_t *d_hi,
                          const uint32_t *d_base_frame,
                          const uint64_t *d_read_frames /* NULL: no moves, and no frame argument is looked at */,
                          const uint8_t *d_codes, uint64_t frame_base,
                          uint64_t frame_capacity, uint8_t *d_new_seq, uint8_t *d_new_qual, uint32_t *d_new_base_frame,
                          uint64_t new_base_capacity, uint64_t *d_new_read_bases, int32_t *d_new_status,
                          uint8_t *d_new_codes, uint64_t new_frame_capacity, uint64_t *d_new_read_frames,
                          uint32_t *d_trim_frames, void *stream);

/* ---- Typed record tags --------------------------------------------------------------------------------------
 * The two record writers again, with tag columns that have a type: unsigned, signed and float 32-bit values, a
 * string per read from a dictionary, and a string per read from a pool.
 *   ... pgn_read_stats_device, pgn_read_qual_device, pgn_classify_reads_device
 *       -> pgn_bam_records_tagged_device | pgn_fastq_records_tagged_device -> pgn_bgzf_deflate_device
 * The BAM bytes are those of SAMv1 section 4.2.4, the text that of SAMv1 section 1.5; no outside program defines
 * the bytes here, so this text does.  Integers and bytes alone: the tolerance is zero.
 *
 * pgn_bam_records_tagged_device and pgn_fastq_records_tagged_device take every argument of pgn_bam_records_device
 * and pgn_fastq_records_device in the same order, with `tags` behind `params`.  params->ntags must be 0: the columns
 * are those of `tags` alone.  The flags, the stride, the kept-read rule, the layouts (raw and PGN_BAM_BGZF), rec_off,
 * rec_status, d_written, "no partial records" and "nothing outside the written records is touched" keep the meaning
 * they have in the old calls.
 * Per kept read r the columns k = 0 .. ncols - 1 are written in order where the old calls write theirs; in BAM
 * mv:B:c stays last.  A column has a two-byte name ([A-Za-z][A-Za-z0-9]) and a type:
 *   PGN_TAG_U32   v = ((const uint32_t *)d_values)[r].  BAM: name0 name1 'I' and the 4 bytes, 7 bytes.
 *                 FASTQ: '\t' name0 name1 ':' 'i' ':' dec(v), 6 + digits(v) bytes.
 *   PGN_TAG_I32   v = ((const int32_t *)d_values)[r].  BAM: name0 name1 'i' and the 4 bytes, 7 bytes.
 *                 FASTQ: the same text with '-' in front of dec(|v|) for v < 0; -2^31 prints as -2147483648.
 *   PGN_TAG_F32   BAM: name0 name1 'f' and the 4 bytes of d_values exactly as stored, 7 bytes: a NaN's payload and
 *                 -0 are not touched.  FASTQ: a column of this type refuses the whole call (below); a float's
 *                 text has no rule here.
 *   PGN_TAG_DICT  idx = ((const uint32_t *)d_values)[r].  idx >= nstrings: the column is absent for this read, 0
 *                 bytes in either format, so PGN_DEMUX_NONE leaves an unclassified read untagged and nstrings == 0
 *                 leaves every read untagged.  Otherwise the span is [d_str_off[idx], d_str_off[idx + 1]).
 *   PGN_TAG_STR   The span is [d_str_off[r], d_str_off[r + 1]).  The column is always present; an empty span writes
 *                 an empty value.
 * A span [a, b) is valid iff a <= b <= str_capacity, b - a <= PGN_TAG_MAX_STRING = 255 and every byte
 * d_strings[a .. b) is in 0x20 .. 0x7E.  A read that would be kept but has an invalid span in any column is not
 * kept and gets PGN_ERR_INVALID_ARG, as a read whose frames leave the window does.  A dictionary entry that no kept
 * read references is never looked at.  No access leaves the buffers, whatever the offsets hold.
 * A string value (DICT, STR) of len bytes:
 *   BAM: name0 name1 'Z' the bytes NUL, 4 + len bytes.  FASTQ: '\t' name0 name1 ':' 'Z' ':' the bytes, 6 + len bytes.
 *   block_size of a kept read = 69 + (m + 1) / 2 + m + sum_k bytes_k(r) + (moves ? 9 + F : 0)
 *   length of a kept read's FASTQ record = 42 + 2m + sum_k text_k(r)
 * with bytes_k(r) and text_k(r) the lengths above.
 *   bam_bound_tagged(nreads, nbases, columns, nframes) = nreads * 74 + nbases + nbases / 2 + sum_k bam_k
 *                                                         [+ 9 * nreads + nframes]
 *   fastq_bound_tagged(nreads, nbases, columns) = nreads * 42 + 2 * nbases + sum_k fastq_k
 * give the host a capacity without a wait, from the column types, each DICT column's longest entry L and each STR
 * column's pool size: bam_k = 7 * nreads (U32, I32, F32), (4 + L) * nreads (DICT), str_capacity + 4 * nreads (STR);
 * fastq_k = 16 * nreads (U32), 17 * nreads (I32), (6 + L) * nreads (DICT), str_capacity + 6 * nreads (STR).  A
 * STR column's term holds for non-decreasing d_str_off; spans that overlap can need more, which rec_off[nreads]
 * tells as always.
 * With U32 columns only, every output (the bytes, rec_off, rec_status, d_written) is identical to the old call's
 * with the same columns.
 * The length kernels add the columns' bytes, a thread per read, and validate each span they use; the scan and the
 * offsets are the old calls'; the writers stay flat over the stream, a workgroup per 65,280 stream bytes in BAM and
 * per PGN_FASTQ_TILE_BYTES in FASTQ, and walk a record's columns where the old ones walk theirs.  The length of a
 * record's tag area is recomputed in the writer from rec_off (and read_frames), not carried: the scratch is 0
 * bytes per read and 8 bytes per 1,024 reads, as in the old calls.
 * PGN_ERR_INVALID_ARG before any GPU call, in this order: a NULL ctx, params or tags; unknown flag bits;
 * params->ntags != 0; ncols > PGN_REC_MAX_TAGS, or a bad name or an unknown type among the first ncols; in FASTQ a
 * PGN_TAG_F32 column; with PGN_BAM_MOVES a stride outside 1..127; nreads >= 2^32; a str_capacity >= 2^32; with
 * nreads > 0 a NULL d_values (types 0 to 3) or a NULL d_str_off (STR, or DICT with nstrings > 0); with
 * str_capacity > 0 a NULL d_strings; then the old call's remaining conditions in the old call's order (from "with
 * nreads > 0 a NULL d_read_ids" on, without its d_tag clause).  nreads == 0 writes rec_off[0] = 0 (and d_written =
 * {0, 0} in BAM) only.  Asynchronous on `stream`, no host wait.
 *
 * Not covered: other BAM types (A, c C s S, H, B arrays other than mv); 64-bit values; float text in FASTQ; strings
 * above 255 bytes; uniqueness of names; a float mean quality computed on the device; @RG header lines, which stay
 * the caller's header_text; SAM text. */
#define PGN_TAG_U32  0u   /* BAM 'I'; text  XX:i:dec                                   */
#define PGN_TAG_I32  1u   /* BAM 'i'; text  XX:i:[-]dec                                */
#define PGN_TAG_F32  2u   /* BAM 'f', the four bytes as stored; refused in FASTQ       */
#define PGN_TAG_DICT 3u   /* 'Z': string d_values[r] of a table of nstrings strings    */
#define PGN_TAG_STR  4u   /* 'Z': string r of a pool with nreads + 1 offsets           */
#define PGN_REC_MAX_TAGS 16u
#define PGN_TAG_MAX_STRING 255u

typedef struct pgn_tag_column {
    uint8_t  name[2];            /* [A-Za-z][A-Za-z0-9] */
    uint8_t  type, pad;
    uint32_t nstrings;           /* DICT: entries of the table */
    const void     *d_values;    /* U32/I32/F32: nreads 4-byte values; DICT: nreads uint32 indices; STR: not read */
    const uint32_t *d_str_off;   /* DICT: nstrings + 1; STR: nreads + 1 */
    const uint8_t  *d_strings;
    uint64_t str_capacity;       /* bytes of d_strings, < 2^32 */
} pgn_tag_column;
typedef struct pgn_record_tags { uint32_t ncols, pad; pgn_tag_column col[16]; } pgn_record_tags;

int pgn_bam_records_tagged_device(pgn_ctx *ctx, const pgn_bam_params *params, const pgn_record_tags *tags,
                                  size_t nreads, const uint8_t *d_read_ids, const uint64_t *d_read_bases,
                                  const int32_t *d_read_status, const uint8_t *d_keep /* may be NULL */,
                                  const uint8_t *d_seq, const uint8_t *d_qual /* may be NULL */,
                                  uint64_t base_capacity, const uint64_t *d_read_frames, const uint8_t *d_codes,
                                  uint64_t frame_base, uint64_t frame_capacity, uint8_t *d_out,
                                  uint64_t byte_capacity, uint64_t *d_rec_off, int32_t *d_rec_status,
                                  uint64_t *d_written, void *stream);

int pgn_fastq_records_tagged_device(pgn_ctx *ctx, const pgn_fastq_params *params, const pgn_record_tags *tags,
                                    size_t nreads, const uint8_t *d_read_ids, const uint64_t *d_read_bases,
                                    const int32_t *d_read_status, const uint8_t *d_keep /* may be NULL */,
                                    const uint8_t *d_seq, const uint8_t *d_qual, uint64_t base_capacity,
                                    uint8_t *d_out, uint64_t byte_capacity, uint64_t *d_rec_off,
                                    int32_t *d_rec_status, void *stream);

/* Device generator of the synthetic nanopore-like reads used by bench.py (integer-only, identical
 * to the checker's pgno_synth_read): global read first_read + r * read_stride ->
 * d_samples[d_sample_offsets[r] .. + d_sample_counts[r]). */
int pgn_synth_reads_device(pgn_ctx *ctx, size_t nreads, uint64_t seed, uint64_t first_read, uint64_t read_stride,
                           int16_t *d_samples,
                           const uint64_t *d_sample_offsets, const uint32_t *d_sample_counts,
                           uint32_t p_switch_q16, int32_t level_mean, int32_t level_sd, int32_t noise_sd, void *stream);

/* Diagnostics: accumulated shader-clock cycles per kernel phase (out[0..15] encode, out[16..31]
 * decode; all zero unless the context was created with PGN_PHASE_PROFILE=1 in the environment). */
int pgn_debug_phase_cycles(pgn_ctx *ctx, uint64_t *out, int n);
/* Diagnostics: per-stream decode records of the first n chunks of the last decode pass
 * (5 per chunk, 24 bytes each: u64 frame offset, u32 frame bytes, u32 content size,
 * u32 intermediate offset, i32 decoded bytes or a negative error). */
int pgn_debug_decode_units(pgn_ctx *ctx, void *out, size_t nchunks);

/* Kernels of the C5 batch path on ctx, direction 0 = encode, 1 = decode: the fused per-chunk kernel
 * or the staged three-kernel pipeline (PGN_ENC_PIPELINE / PGN_DEC_PIPELINE = fused | staged). */
const char *pgn_ctx_kernels(pgn_ctx *ctx, int direction);

/* Kernel time (ms, HIP events on the launch stream) of the last batch encode / decode call on ctx. */
float pgn_ctx_last_encode_ms(pgn_ctx *ctx);
float pgn_ctx_last_decode_ms(pgn_ctx *ctx);

#ifdef __cplusplus
}
#endif

#endif /* PGNANO_HIP_H */
