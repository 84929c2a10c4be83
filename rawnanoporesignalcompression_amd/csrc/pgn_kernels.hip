// pgn_kernels.hip -- gfx950 kernels and the C ABI (include/pgnano_hip.h) of the C5 codec.
//
// Layout (DESIGN.md "Data layout in HBM"): one 64-lane workgroup per resident slot; each slot owns a
// fixed scratch window in HBM (its five streams, hash table, literal/sequence staging) and walks the
// chunks blockIdx.x, blockIdx.x + gridDim.x, ...  Chunks are independent (the delta restarts at 0
// and every zstd frame is self-contained, C5.hpp:302-309), so there is no inter-workgroup traffic.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <condition_variable>
#include <mutex>
#include <vector>

#include "../../include/pgnano_hip.h"
#include "../../include/pgnano_pod5.h"
#include "pgn_c5.h"
#include "pgn_internal.h"
#include "pgn_segment.h"
#include "pgn_stitch.h"
#include "pgn_ctc.h"
#include "pgn_crf.h"
#include "pgn_crf_post.h"
#include "pgn_qual.h"
#include "pgn_fastq.h"
#include "pgn_bam.h"
#include "pgn_deflate.h"
#include "pgn_demux.h"
#include "pgn_tags.h"
#include "pgn_select.h"
#include "pgn_vbz.h"
#include "pgn_variants.h"
#include "pgn_zdec.h"
#include "pgn_zenc.h"

namespace pgn {

// Chunks up to kPassSamples take the batched passes, whose per-chunk buffers are spaced for that
// many samples; larger ones (up to PGN_MAX_CHUNK_SAMPLES) take the large-chunk pass, whose slot
// buffers are spaced for the largest chunk of the call (launch_large_*).
constexpr uint32_t kPassSamples = 262144;
static_assert(PGN_MAX_CHUNK_SAMPLES >= kPassSamples, "chunk limits");
// literals and sequences live per zstd block (<= 128 KiB); a frame's blocks reuse them
constexpr uint32_t kMaxEncSeq = (uint32_t)z1::kMaxSrc / 4 + 2;  // every match covers >= 4 bytes
// every stream of the largest chunk fits one encoder frame (its svb16 buffer, ~2.13 n, the largest)
static_assert((size_t)PGN_MAX_CHUNK_SAMPLES * 9 / 4 + 64 <= kMaxFrameBytes, "frame index field");
constexpr int kStreams = 5;
// Codecs of a batch call: the pgnano C5 variant (5 zstd frames per chunk) and the pod5 VBZ codec
// (one zstd frame per chunk).  Both share the per-chunk buffers and the zstd kernels.
enum Codec : int { kCodecC5 = 0, kCodecVbz = 1, kCodecC4 = 2, kCodecC1 = 3, kCodecC2 = 4, kCodecC3 = 5, kCodecVbz0 = 6 };

__host__ __device__ constexpr size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Capacity of C5 stream s of a chunk of at most capN samples: keys n/4, S n/2, M/Ll/Lh n.  The
// stream area of a chunk (3.75 capN) also holds its VBZ / C1 svb16 buffer (<= 2.13 n) and the other
// variants' streams.
__host__ __device__ constexpr uint32_t stream_cap(int s, uint32_t capN = kPassSamples)
{
    return s == 0 ? capN / 4 + 1 : (s == 1 ? capN / 2 + 1 : capN);
}
__host__ __device__ constexpr size_t stream_pad(int s, uint32_t capN = kPassSamples)
{
    return align_up((size_t)stream_cap(s, capN) + 64, 256);
}
// byte offset of stream s inside a chunk's stream area
__host__ __device__ constexpr size_t stream_off(int s, uint32_t capN = kPassSamples)
{
    size_t o = 0;
    for (int t = 0; t < s; t++) o += stream_pad(t, capN);
    return o;
}
__host__ __device__ constexpr size_t chunk_stream_bytes(uint32_t capN) { return stream_off(kStreams, capN); }
constexpr size_t kChunkStreamBytes = chunk_stream_bytes(kPassSamples);
// ZSTD_COMPRESSBOUND (the frame of a stream never exceeds it)
__host__ __device__ constexpr size_t frame_bound(size_t n)
{
    return n + (n >> 8) + (n < (128u << 10) ? (((128u << 10) - n) >> 11) : 0);
}
__host__ __device__ constexpr size_t frame_pad(int s) { return align_up(frame_bound(stream_cap(s)) + 64, 256); }
__host__ __device__ constexpr size_t frame_off(int s)
{
    size_t o = 0;
    for (int t = 0; t < s; t++) o += frame_pad(t);
    return o;
}
constexpr size_t kChunkFrameBytes = frame_off(kStreams);

// ---------------------------------------------------------------------------------------------
// Scratch of one resident zstd-encode workgroup ("slot")
// ---------------------------------------------------------------------------------------------
struct EncLayout {
    size_t ht, lit, seqs, codes, seqSection, seqWork, huf, bytes;
};
__host__ __device__ inline EncLayout enc_layout()
{
    EncLayout l{};
    size_t o = 0;
    auto take = [&](size_t n) { size_t r = o; o = align_up(o + n + 64, 256); return r; };
    l.ht = take((size_t)4 << 15);
    l.lit = take(z1::kMaxSrc);
    l.seqs = take(sizeof(z1::Seq) * kMaxEncSeq);
    l.codes = take(3 * (size_t)kMaxEncSeq);
    l.seqSection = take(16 + 10 * (size_t)kMaxEncSeq + 1024);
    l.seqWork = take(sizeof(z1::SeqWork));
    l.huf = take(2 * 256 * 4);
    l.bytes = o;
    return l;
}

struct DecLayout {
    size_t lit, tables, htab, bytes;
};
__host__ __device__ inline DecLayout dec_layout()
{
    DecLayout l{};
    size_t o = 0;
    auto take = [&](size_t n) { size_t r = o; o = align_up(o + n + 64, 256); return r; };
    l.lit = take(z1::kMaxSrc);
    l.tables = take(4 * ((size_t)kSeqTab + 4));
    l.htab = take(2u << z1::kHufTableLogMax);
    l.bytes = o;
    return l;
}
// A chunk's intermediate (the decoded frames back to back) holds 2.25 capN + 1,024 bytes: the most
// any blob of a chunk of n <= capN samples holds when its frames decode to what its merge consumes --
// C5 / C4: n/4 key bytes + 2 bytes per sample at most (a class-3 sample), every one of its S / M /
// class-3 bytes standing for one sample; C1 / C2 / C3: n/8 + 2 n; VBZ0 n/4 + 2 n; VBZ's svb16 buffer
// n/8 + 2 n + 16 padding bytes -- plus slack for trailing bytes ("Remaining data").  Frames claiming
// more go through over_claim_status (the reference's own outcome for them, decided without decoding).
__host__ __device__ constexpr size_t inter_cap(uint32_t capN) { return (size_t)capN * 9 / 4 + 1024; }
// svb16::decode_input_buffer_padding_byte_count() on x86-64 (svb16/decode.hpp:16-23): the VBZ
// intermediate is the frame content plus 16 bytes, and ZSTD_decompress may fill them.
constexpr size_t kVbzPadding = 16;
constexpr uint64_t kAllocLimit = (uint64_t)1 << 40;  // a decode intermediate above this is an allocation failure (PGN_ERR_ALLOC)
__host__ __device__ constexpr size_t chunk_inter_bytes(uint32_t capN) { return align_up(inter_cap(capN) + 64, 256); }
// per-chunk decode buffers of the passes in flight (intermediates, records, Huffman jobs), all
// buffers together
constexpr size_t kDecBufferBudget = (size_t)32 << 30;
constexpr int kMaxDecBufs = 4;  // decode pass buffers in rotation (pgn_ctx::decBufs)

// Work-unit order of the per-stream kernels: the large streams first (M, S, keys, Llow, Lhigh), so
// the dynamic queue ends with short units.
__device__ __forceinline__ int unit_stream(uint32_t k) { return (int)((0x43012u >> (4 * k)) & 0xFu); }

// ---------------------------------------------------------------------------------------------
// Encode: split -> per-stream zstd -> assemble, over a sub-batch of G chunks (chunk g = base + g)
// ---------------------------------------------------------------------------------------------
struct EncArgs {
    size_t nchunks;
    const int16_t* samples;
    const uint64_t* sampleOffsets;
    const uint32_t* sampleCounts;
    uint8_t* out;
    const uint64_t* outOffsets;
    const uint64_t* outCaps;
    uint64_t* outSizes;
    int32_t* status;
    uint64_t* stats;
    uint8_t* streams;    // G * kChunkStreamBytes
    uint8_t* frames;     // G * kChunkFrameBytes
    uint32_t* sizes;     // [G][5] raw stream sizes; sizes[g*5] = ~0u marks an unsupported chunk
    uint32_t* fsizes;    // [G][5] frame sizes
    uint8_t* slotScratch;
    size_t slotBytes;
    uint32_t* epochs;
    uint32_t* queue;     // work counter of this sub-batch
    uint64_t* prof;
    size_t base, G;
    uint32_t nu;         // zstd work units per chunk: 5 (C5) or 1 (VBZ)
    // fused kernels: slot buffers spaced for capN samples; chunk u of the queue is list[u] (the
    // large-chunk pass) or u
    uint32_t capN;
    const uint32_t* list;
    uint64_t* lookback;  // small batches: the range split's published words (kSplitRanges x 2 per chunk)
    uint64_t epoch;      // this call's tag in those words (bits 48..63)
};

__global__ __launch_bounds__(64) void enc_split_kernel(EncArgs a)
{
    static __shared__ SplitLds W;
    const size_t g = blockIdx.x;
    const size_t c = a.base + g;
    if (g >= a.G || c >= a.nchunks) return;
    PhaseProf P;
    P.init(a.prof);
    const uint32_t n = a.sampleCounts[c];
    uint32_t* sz = a.sizes + g * kStreams;
    if (n > kPassSamples) {  // the large-chunk pass takes it (or reports it unsupported)
        if (lane_id() == 0) {
            sz[0] = ~0u;
            a.status[c] = PGN_ERR_UNSUPPORTED;
            a.outSizes[c] = 0;
        }
        return;
    }
    uint8_t* base = a.streams + g * kChunkStreamBytes;
    C5Streams st{base + stream_off(0), base + stream_off(1), base + stream_off(2), base + stream_off(3), base + stream_off(4)};
    uint32_t sizes[5];
    c5_split_wave(a.samples + a.sampleOffsets[c], n, st, sizes, W);
    if (lane_id() == 0)
        for (int s = 0; s < kStreams; s++) sz[s] = sizes[s];
    P.mark(0);
    P.flush();
}

// Decoupled look-back between the single-wave range workgroups of one chunk (small batches): a
// range publishes a tagged 64-bit word (this call's epoch in bits 48..63) and later ranges wait for
// the words of the ranges before them; a workgroup only waits on lower-numbered ones, which the
// dispatcher started first.
__device__ __forceinline__ void lb_publish(uint64_t* w, uint64_t epoch, uint64_t payload)
{
    __hip_atomic_store(w, (epoch << 48) | payload, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}
// lane v < nv waits for word v * 3 + k of the chunk's look-back array; returns its payload (0 for v >= nv)
__device__ __forceinline__ uint64_t lb_wait(uint64_t* lb, int k, uint32_t nv, uint64_t epoch)
{
    const uint32_t v = (uint32_t)lane_id();
    uint64_t x = 0;
    if (v < nv) {
        while (true) {
            x = __hip_atomic_load(lb + 3 * v + k, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
            if ((x >> 48) == epoch) break;
            __builtin_amdgcn_s_sleep(1);
        }
    }
    return x & 0xFFFFFFFFFFFFull;
}
// Small batches, many CUs per chunk: the split over kSplitRanges single-wave range workgroups.
// Each publishes its class counts, sums those of the ranges before it (its places in the S / M /
// class-3 streams), splits its range and publishes the nibbles the S bytes it shares need; the last
// range writes those bytes and the stream sizes.  Same bytes as enc_split_kernel.
constexpr int kSplitRanges = 32;
__global__ __launch_bounds__(64) void enc_split_lb_kernel(EncArgs a)
{
    const size_t g = blockIdx.x / kSplitRanges;
    const uint32_t r = blockIdx.x % kSplitRanges;
    const size_t c = a.base + g;
    if (g >= a.G || c >= a.nchunks) return;
    __shared__ SplitLds W;
    const uint32_t lane = (uint32_t)lane_id();
    const uint32_t n = a.sampleCounts[c];
    uint32_t* sz = a.sizes + g * kStreams;
    if (n > kPassSamples) {  // the large-chunk pass takes it
        if (r == 0 && lane == 0) {
            sz[0] = ~0u;
            a.status[c] = PGN_ERR_UNSUPPORTED;
            a.outSizes[c] = 0;
        }
        return;
    }
    uint64_t* lb = a.lookback + g * (3 * kSplitRanges);
    const uint64_t ep = a.epoch;
    const int16_t* x = a.samples + a.sampleOffsets[c];
    uint8_t* base = a.streams + g * kChunkStreamBytes;
    const C5Streams st{base + stream_off(0), base + stream_off(1), base + stream_off(2), base + stream_off(3),
                       base + stream_off(4)};
    const uint32_t steps = (n + kSplitStep - 1) / kSplitStep;
    const uint32_t s0 = steps * r / kSplitRanges, s1 = steps * (r + 1) / kSplitRanges;
    const uint32_t t0 = s0 * kSplitStep, t1 = s1 * kSplitStep < n ? s1 * kSplitStep : n;
    uint32_t cS = 0, cM = 0, cL = 0;
    if (t0 < t1) c5_split_counts(x, n, t0, t1, cS, cM, cL);
    if (lane == 0) lb_publish(lb + 3 * r, ep, (uint64_t)cS | ((uint64_t)cM << 16) | ((uint64_t)cL << 32));
    const uint64_t pc = lb_wait(lb, 0, r, ep);
    const uint32_t pS = (uint32_t)wave_sum64(pc & 0xFFFFu), pM = (uint32_t)wave_sum64((pc >> 16) & 0xFFFFu),
                   pL = (uint32_t)wave_sum64(pc >> 32);
    uint32_t firstNib = 0xFFu, lastNib = 0xFFu;
    if (t0 < t1) c5_split_range(x, n, t0, t1, st, pS, pM, pL, W, firstNib, lastNib);
    if (lane == 0) lb_publish(lb + 3 * r + 1, ep, (uint64_t)(firstNib & 0xFFu) | ((uint64_t)(lastNib & 0xFFu) << 8));
    if (r != kSplitRanges - 1) return;
    // the last range: every range's counts and nibbles -> the shared S bytes, a trailing half byte, sizes
    const uint64_t cnt = lb_wait(lb, 0, kSplitRanges, ep);
    const uint64_t nb = lb_wait(lb, 1, kSplitRanges, ep);
    const uint32_t tS = (uint32_t)wave_sum64(cnt & 0xFFFFu), tM = (uint32_t)wave_sum64((cnt >> 16) & 0xFFFFu),
                   tL = (uint32_t)wave_sum64(cnt >> 32);
    const uint32_t mS = (uint32_t)(cnt & 0xFFFFu);  // lane v: range v's S count
    const uint32_t fN = (uint32_t)(nb & 0xFFu), lN = (uint32_t)((nb >> 8) & 0xFFu);
    uint32_t at = 0, lastOwner = ~0u;
    for (uint32_t v = 0; v < (uint32_t)kSplitRanges; v++) {  // wave-uniform walk over the ranges
        const uint32_t cv = readlane_u32(mS, (int)v);
        if (cv == 0) continue;
        if ((at & 1u) && lastOwner != ~0u && lane == 0)
            gst<uint8_t>(st.S + (at >> 1), (uint8_t)(readlane_u32(lN, (int)lastOwner) | (readlane_u32(fN, (int)v) << 4)));
        at += cv;
        lastOwner = v;
    }
    if ((at & 1u) && lastOwner != ~0u && lane == 0) gst<uint8_t>(st.S + (at >> 1), (uint8_t)readlane_u32(lN, (int)lastOwner));
    if (lane == 0) {
        sz[0] = (n + 3) / 4;
        sz[1] = (tS + 1) / 2;
        sz[2] = tM;
        sz[3] = tL;
        sz[4] = tL;
    }
}

constexpr size_t kSplitWgMaxChunks = 64;  // batches up to this many chunks take the small-batch kernels

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4))) void enc_zstd_kernel(EncArgs a)
{
    const int lane = lane_id();
    const EncLayout lay = enc_layout();
    uint8_t* sbase = a.slotScratch + (size_t)blockIdx.x * a.slotBytes;
    EncScratch S;
    S.ht = (uint32_t*)(sbase + lay.ht);
    S.seqs = (z1::Seq*)(sbase + lay.seqs);
    S.codes = sbase + lay.codes;
    S.lit = sbase + lay.lit;
    S.seqSection = sbase + lay.seqSection;
    S.seqWork = (z1::SeqWork*)(sbase + lay.seqWork);
    S.maxSeq = kMaxEncSeq;
    S.huf = (uint32_t*)(sbase + lay.huf);
    S.coop = nullptr;
    uint32_t epoch = a.epochs[blockIdx.x];  // table state: epoch tag | written extent << 8 (ht_next_epoch)
    PhaseProf P;
    P.init(a.prof, a.prof);  // (the encode's search attribution: PhaseProf::ext)
    const size_t G = a.G, units = (size_t)a.nu * G;
    while (true) {
        uint32_t u = 0;
        if (lane == 0) u = atomicAdd(a.queue, 1u);
        u = __builtin_amdgcn_readfirstlane(u);
        if (u >= units) break;
        const int s = a.nu == 1 ? 0 : unit_stream((uint32_t)(u / G));
        const size_t g = u % G;
        if (a.base + g >= a.nchunks) continue;
        const uint32_t n = a.sizes[g * kStreams + s];
        if (a.sizes[g * kStreams] == ~0u) continue;  // unsupported chunk
        ht_next_epoch(S.ht, epoch, n);
        // VBZ: the svb16 buffer starts at the offset its split recorded in sizes[1]
        const uint8_t* src = a.streams + g * kChunkStreamBytes + (a.nu == 1 ? a.sizes[g * kStreams + 1] : stream_off(s));
        uint8_t* dst = a.frames + g * kChunkFrameBytes + frame_off(s);
        const size_t fsz = zstd1_compress_wave(dst, src, n, S, epoch & 0xFFu, P);
        if (lane == 0) a.fsizes[g * kStreams + s] = (uint32_t)fsz;
        wave_sync();
    }
    if (lane == 0) a.epochs[blockIdx.x] = epoch;
    P.flush();
}

// The small-batch C5 encode places its frames itself (no enc_assemble_kernel): frame s publishes
// its size in look-back word 3 s + 2 of its chunk, waits for the sizes of frames 0 .. s-1, and
// copies itself behind their length prefixes (C5.hpp:429-462).  enc_zstd_coop_kernel numbers its
// workgroups u = s * G + g (blob order, coop_unit_stream), so every frame it waits for belongs to a
// lower-numbered workgroup, which the dispatcher started first: forward progress does not depend on
// all of a call's workgroups being resident at once (another context or process may hold CUs)
// when it fits the capacity.  Frame 4 then knows the total and writes the status, the size and the
// stats as enc_assemble_kernel does.  On DST_TOO_SMALL the bytes that fit may have been written
// (as in the fused kernel, which writes its frames straight into the blob).
__device__ __noinline__ void enc_place_frame(const EncArgs& a, size_t g, int s, const uint8_t* fr, uint32_t f)
{
    const size_t c = a.base + g;
    const int lane = lane_id();
    uint64_t* lb = a.lookback + g * (3 * kSplitRanges);
    const uint64_t ep = a.epoch;
    if (lane == 0) lb_publish(lb + 3 * s + 2, ep, f);
    const uint64_t fv = lb_wait(lb, 2, (uint32_t)s, ep);  // lane v < s: frame v's size
    const uint64_t off = wave_sum64(fv) + 8ull * (uint64_t)s;
    const uint32_t pre = s < kStreams - 1 ? 8u : 0u;
    const uint64_t cap = a.outCaps[c];
    uint8_t* out = a.out + a.outOffsets[c];
    if (off + pre + f <= cap) {
        if (pre && lane == 0) {
            const uint64_t v = f;
            __builtin_memcpy(out + off, &v, 8);
        }
        wave_copy(out + off + pre, fr, f);
    }
    if (s != kStreams - 1) return;
    const uint64_t total = off + f;
    const uint32_t* sz = a.sizes + g * kStreams;
    if (lane == 0) {
        a.status[c] = total <= cap ? PGN_OK : PGN_ERR_DST_TOO_SMALL;
        a.outSizes[c] = total;
    }
    if (a.stats && lane < kStreams) {
        a.stats[c * PGN_STATS_PER_CHUNK + lane] = sz[lane];
        a.stats[c * PGN_STATS_PER_CHUNK + 5 + lane] = lane == kStreams - 1 ? f : (uint32_t)fv;
    }
}

// Stream of unit u in the cooperative kernels: blob order (keys, S, M, Llow, Lhigh).  Not the large-
// first order of the persistent kernels: every workgroup of a cooperative launch starts at once, and
// enc_place_frame's waits must point at lower-numbered workgroups.
__device__ __forceinline__ int coop_unit_stream(uint32_t k) { return (int)k; }

// Small batches (the per-chunk calls): one workgroup of kCoopEncWaves waves per stream.  Wave 0
// compresses the stream; the histograms and the bit packing of its four-segment literals sections
// are shared with the other waves, one segment each (pgn_zenc.h CoopEncCmd).  A lone chunk's encode
// is bound by its largest stream's frame.
__global__ __launch_bounds__(64 * kCoopEncWaves) void enc_zstd_coop_kernel(EncArgs a)
{
    const int lane = lane_id();
    const uint32_t wid = (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t G = a.G;
    const uint32_t u = blockIdx.x;
    if ((size_t)u >= (size_t)a.nu * G) return;
    const int s = a.nu == 1 ? 0 : coop_unit_stream((uint32_t)(u / G));
    const size_t g = u % G;
    if (a.base + g >= a.nchunks) return;
    if (a.sizes[g * kStreams] == ~0u) return;  // unsupported chunk (the same for every wave)
    __shared__ uint32_t winAll[(kCoopEncWaves - 1) * kWinWords];
    __shared__ CoopEncCmd cmdLds;
    lds_enc_cmd* cmd = (lds_enc_cmd*)&cmdLds;
    if (wid != 0) {
        coop_enc_helper_wave(wid, cmd, (lds_u32*)&winAll[(wid - 1) * kWinWords]);
        return;
    }
    const EncLayout lay = enc_layout();
    uint8_t* sbase = a.slotScratch + (size_t)u * a.slotBytes;
    EncScratch S;
    S.ht = (uint32_t*)(sbase + lay.ht);
    S.seqs = (z1::Seq*)(sbase + lay.seqs);
    S.codes = sbase + lay.codes;
    S.lit = sbase + lay.lit;
    S.seqSection = sbase + lay.seqSection;
    S.seqWork = (z1::SeqWork*)(sbase + lay.seqWork);
    S.maxSeq = kMaxEncSeq;
    S.huf = (uint32_t*)(sbase + lay.huf);
    S.coop = cmd;
    uint32_t epoch = a.epochs[u];  // table state of slot u (ht_next_epoch)
    PhaseProf P;
    P.init(a.prof, a.prof);  // (the encode's search attribution: PhaseProf::ext)
    const uint32_t n = a.sizes[g * kStreams + s];
    ht_next_epoch(S.ht, epoch, n);
    const uint8_t* src = a.streams + g * kChunkStreamBytes + (a.nu == 1 ? a.sizes[g * kStreams + 1] : stream_off(s));
    uint8_t* dst = a.frames + g * kChunkFrameBytes + frame_off(s);
    const size_t fsz = zstd1_compress_wave<true>(dst, src, n, S, epoch & 0xFFu, P);
    if (lane == 0) {
        a.fsizes[g * kStreams + s] = (uint32_t)fsz;
        a.epochs[u] = epoch;
    }
    coop_enc_finish(cmd);
    if (a.lookback) enc_place_frame(a, g, s, dst, (uint32_t)fsz);  // C5 (the look-back split ran)
    P.flush();
}

__global__ __launch_bounds__(64) void enc_assemble_kernel(EncArgs a)
{
    const size_t g = blockIdx.x;
    const size_t c = a.base + g;
    if (g >= a.G || c >= a.nchunks) return;
    const int lane = lane_id();
    const uint32_t* sz = a.sizes + g * kStreams;
    if (sz[0] == ~0u) return;
    PhaseProf P;
    P.init(a.prof);
    const uint32_t* fs = a.fsizes + g * kStreams;
    uint64_t total = 0;
    for (int s = 0; s < kStreams; s++) total += (s < 4 ? 8 : 0) + fs[s];
    const uint64_t cap = a.outCaps[c];
    const bool ok = total <= cap;  // C5.hpp:420-427 "Not enough space in destination buffer"
    if (ok) {
        uint8_t* dst = a.out + a.outOffsets[c];
        const uint8_t* fr = a.frames + g * kChunkFrameBytes;
        uint64_t off = 0;
        for (int s = 0; s < kStreams; s++) {
            if (s < 4) {
                if (lane == 0) {
                    const uint64_t v = fs[s];
                    __builtin_memcpy(dst + off, &v, 8);
                }
                off += 8;
            }
            wave_copy(dst + off, fr + frame_off(s), fs[s]);
            off += fs[s];
        }
    }
    if (lane == 0) {
        a.status[c] = ok ? PGN_OK : PGN_ERR_DST_TOO_SMALL;
        a.outSizes[c] = total;
        if (a.stats) {
            for (int s = 0; s < kStreams; s++) {
                a.stats[c * PGN_STATS_PER_CHUNK + s] = sz[s];
                a.stats[c * PGN_STATS_PER_CHUNK + 5 + s] = fs[s];
            }
        }
    }
    P.mark(10);
    P.flush();
}

// ---------------------------------------------------------------------------------------------
// Decode: parse -> per-stream zstd decode -> merge
// ---------------------------------------------------------------------------------------------
struct DecUnit {
    uint64_t src;       // frame offset in the input batch
    uint32_t len;       // frame bytes
    uint32_t cs;        // frame content size (= decoded bytes expected)
    uint32_t interOff;  // offset of this stream in the chunk's intermediate
    int32_t dres;       // decoded bytes, < 0 on failure
};

struct DecArgs {
    size_t nchunks;
    const uint8_t* in;
    const uint64_t* inOffsets;
    const uint64_t* inSizes;
    int16_t* samples;
    const uint64_t* sampleOffsets;
    const uint32_t* sampleCounts;
    int32_t* status;
    DecUnit* units;      // [G][5]
    uint8_t* inter;      // G * interStride
    size_t interStride;  // bytes between chunks' intermediates: chunk_inter_bytes(capN)
    uint8_t* slotScratch;
    size_t slotBytes;
    uint32_t* queue;
    uint64_t* prof;
    size_t base, G;
    uint32_t nu;         // zstd work units per chunk: 5 (C5) or 1 (VBZ)
    uint32_t capN;       // fused kernels: as EncArgs
    const uint32_t* list;
    uint64_t* lookback;  // small batches: the range merge's published counts / sums / results (kMergeRanges x 3 per chunk)
    uint64_t epoch;      // this call's tag in those words (bits 48..63)
    uint32_t coopParse;  // dec_zstd_coop_kernel parses the chunks itself (no dec_parse_kernel launch)
    uint8_t* jobs;       // [G][5] HufJob records (pgn_hufjob.h): dec_zstd_kernel defers, dec_huf_kernel decodes; null = in place
    uint32_t hufPrio;    // dec_huf_kernel waves at raised priority (the last deferred pass: the decode's drain)
    uint64_t interBytes; // dec_chunk_kernel's claims pass: the slot intermediate's bytes (0: inter_cap(capN))
    // calibrated output (pgn_decompress_batch_device_pa): the output as bytes, its element type
    // (pgn_out_type; sampleOffsets are in elements of it) and the per-chunk calibration.
    // PGN_OUT_INT16 (0): the kernels write `samples`
    uint8_t* outBytes;
    int32_t outType;
    const float* calOffset;
    const float* calScale;
};

// chunk c's destination and calibration for the output element T (wave-uniform)
template <class T>
__device__ __forceinline__ T* out_chunk(const DecArgs& a, size_t c)
{
    if constexpr (kIsAdc<T>) return a.samples + a.sampleOffsets[c];
    else return reinterpret_cast<T*>(a.outBytes) + a.sampleOffsets[c];
}
template <class T>
__device__ __forceinline__ Cal cal_chunk(const DecArgs& a, size_t c)
{
    if constexpr (kIsAdc<T>) return Cal{0.f, 0.f};
    else return Cal{uni(a.calOffset[c]), uni(a.calScale[c])};
}

// The status of a chunk whose frames claim more content (ZSTD_getFrameContentSize) than the
// decoder's intermediate holds.  The reference allocates the sum of the claims (a size_t sum,
// C5.hpp:575-583) and decompresses each frame into exactly its claim (C5.hpp:588-667): a sum above
// 2^40 bytes is taken as that allocation failing (PGN_ERR_ALLOC, as the oracle), a frame whose blocks
// cannot produce its claim fails in ZSTD_decompress ("failed to decompress", PGN_ERR_ZSTD_DECOMPRESS,
// z1::frame_content_bound); only frames that could really expand that far are PGN_ERR_UNSUPPORTED.
__device__ inline int over_claim_status(const uint8_t* in, const DecUnit* u, const uint64_t* cs, int nf)
{
    uint64_t tot = 0;  // each claim capped just above the limit: five claims near 2^64 cannot wrap below it
    for (int s = 0; s < nf; s++) tot += cs[s] <= kAllocLimit ? cs[s] : kAllocLimit + 1;
    if (tot > kAllocLimit) return PGN_ERR_ALLOC;
    for (int s = 0; s < nf; s++) {
        const int64_t b = z1::frame_content_bound(in + u[s].src, (size_t)u[s].len);
        if (b < 0 || (uint64_t)b < cs[s]) return PGN_ERR_ZSTD_DECOMPRESS;
    }
    return PGN_ERR_UNSUPPORTED;
}

// The claims pass (launch_claims_decode) decodes the chunks over_claim_status leaves UNSUPPORTED, as
// the reference does: every frame into exactly its claim, in an intermediate of the claims' sum.  A
// chunk whose sum exceeds kClaimPassMax gets PGN_ERR_ALLOC (that intermediate does not fit the
// device's budget, the reference's allocation failing) -- only a blob built to expand (its blocks'
// bound is at most 32,768 times its length) reaches it.
constexpr uint64_t kClaimPassMax = (uint64_t)1 << 30;

// A blob of nf frames behind nf - 1 eight-byte length prefixes (C5.hpp:530-586; the variants'
// decompress_signal_* the same with fewer frames): false when it does not parse that far (the
// decoders' PGN_ERR_CORRUPT / PGN_ERR_NOT_ZSTD); else the claims' sum and largest claim, and
// *expand = the claims sum to at most 2^40 and every frame's blocks could produce its claim
// (z1::frame_content_bound) -- the chunks over_claim_status calls UNSUPPORTED when they exceed a
// decoder's buffer.
__host__ __device__ inline bool blob_claims(const uint8_t* src, uint64_t len, int nf, uint64_t* sum, uint64_t* maxClaim,
                                            bool* expand)
{
    uint64_t pos = 0, tot = 0, mx = 0, fo[kStreams], fl[kStreams], cs[kStreams];
    for (int s = 0; s < nf; s++) {
        uint64_t l;
        if (s < nf - 1) {
            if (pos > len || len - pos < 8) return false;
            memcpy(&l, src + pos, 8);
            pos += 8;
            if (l > len - pos) return false;
        } else {
            l = len - pos;
        }
        bool ok = false;
        cs[s] = z1::frame_content_size(src + pos, (size_t)l, &ok);
        if (!ok) return false;
        fo[s] = pos;
        fl[s] = l;
        tot += cs[s] <= kAllocLimit ? cs[s] : kAllocLimit + 1;  // capped: five claims cannot wrap
        mx = cs[s] > mx ? cs[s] : mx;
        pos += l;
    }
    bool ex = tot <= kAllocLimit;
    for (int s = 0; ex && s < nf; s++) {
        const int64_t b = z1::frame_content_bound(src + fo[s], (size_t)fl[s]);
        ex = b >= 0 && (uint64_t)b >= cs[s];
    }
    *sum = tot;
    *maxClaim = mx;
    *expand = ex;
    return true;
}
// a chunk of n samples the claims pass must decode: its frames claim more than any decoder buffer
// spaced for n samples holds (inter_cap(n) less the VBZ padding, or one frame above n bytes: the C5
// per-stream bound) and could really produce it
__host__ __device__ inline bool claims_pass_chunk(const uint8_t* src, uint64_t len, int nf, uint32_t n, uint64_t* sum)
{
    uint64_t mx = 0;
    bool ex = false;
    if (!blob_claims(src, len, nf, sum, &mx, &ex) || !ex) return false;
    return *sum + kVbzPadding > inter_cap(n) || mx > n;
}

// Unhinted batch decodes: the chunks for the claims pass, listed on the scan stream beside the
// batched pass (hdr[4] count, hdr[5] the largest claims' sum in KiB, capped at 2^32 - 1).
__global__ void claim_scan_kernel(const uint8_t* in, const uint64_t* inOffsets, const uint64_t* inSizes,
                                  const uint32_t* counts, size_t n, int nf, uint32_t* list, uint32_t* hdr)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        uint64_t sum = 0;
        if (!claims_pass_chunk(in + inOffsets[i], inSizes[i], nf, counts[i], &sum)) continue;
        list[atomicAdd(hdr + 4, 1u)] = (uint32_t)i;
        const uint64_t kib = (sum + 1023) >> 10;
        atomicMax(hdr + 5, kib < 0xFFFFFFFFull ? (uint32_t)kib : 0xFFFFFFFFu);
    }
}

// one thread per chunk: the four length prefixes and the five frame headers (C5.hpp:530-586).
// Frames claiming more content than the intermediate holds (inter_cap(capN) = 2.25 capN + 1,024
// bytes, capN >= every chunk of the call), or one frame more than kPassSamples bytes, get
// over_claim_status.
__device__ inline int c5_parse_chunk(const uint8_t* in, uint64_t src0, uint64_t len, DecUnit* u, size_t interCap)
{
    const uint8_t* src = in + src0;
    uint64_t pos = 0;
    uint64_t cs[5];
    for (int s = 0; s < kStreams; s++) {
        uint64_t fl;
        if (s < 4) {
            if (pos > len || len - pos < 8) return PGN_ERR_CORRUPT;
            fl = ld64u(src + pos);
            pos += 8;
            if (fl > len - pos) return PGN_ERR_CORRUPT;
        } else {
            fl = len - pos;  // last frame length is implicit (C5.hpp:560)
        }
        bool ok = false;
        cs[s] = z1::frame_content_size(src + pos, (size_t)fl, &ok);
        if (!ok) return PGN_ERR_NOT_ZSTD;
        u[s].src = src0 + pos;
        u[s].len = (uint32_t)fl;
        pos += fl;
    }
    uint64_t off = 0;
    for (int s = 0; s < kStreams; s++) {
        if (cs[s] > kPassSamples || cs[s] > interCap - off) return over_claim_status(in, u, cs, kStreams);
        u[s].cs = (uint32_t)cs[s];
        u[s].interOff = (uint32_t)off;
        off += cs[s];
    }
    return PGN_OK;
}

__global__ __launch_bounds__(64) void dec_parse_kernel(DecArgs a)
{
    const size_t g = (size_t)blockIdx.x * 64 + lane_id();
    const size_t c = a.base + g;
    if (g >= a.G || c >= a.nchunks) return;
    // a chunk above kPassSamples is left to the large-chunk pass
    a.status[c] = a.sampleCounts[c] > kPassSamples ? PGN_ERR_UNSUPPORTED
                                                   : c5_parse_chunk(a.in, a.inOffsets[c], a.inSizes[c], a.units + g * kStreams,
                                                                    inter_cap(a.capN));
}

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5))) void dec_zstd_kernel(DecArgs a)
{
    const int lane = lane_id();
    const DecLayout lay = dec_layout();
    uint8_t* sbase = a.slotScratch + (size_t)blockIdx.x * a.slotBytes;
    DecScratch S;
    S.lit = sbase + lay.lit;
    S.tables = (uint32_t*)(sbase + lay.tables);
    S.htab = (uint16_t*)(sbase + lay.htab);
    S.coopCmd = nullptr;
    S.coopStg = nullptr;
    PhaseProf P;
    P.init(a.prof);
    const size_t G = a.G, units = (size_t)a.nu * G;
    uint32_t tk = 0;
    if (lane == 0) tk = atomicAdd(a.queue, 1u);
    while (true) {
        const uint32_t u = __builtin_amdgcn_readfirstlane(tk);
        if (u >= units) break;
        if (lane == 0) tk = atomicAdd(a.queue, 1u);
        const int s = a.nu == 1 ? 0 : unit_stream((uint32_t)(u / G));
        const size_t g = u % G;
        const size_t c = a.base + g;
        S.job = a.jobs ? a.jobs + (g * kStreams + (size_t)s) * kJobBytes : nullptr;
        if (S.job && lane == 0) gst<uint32_t>(&((HufJob*)S.job)->flag, 0u);  // every unit of the pass: fresh
        if (c >= a.nchunks || a.status[c] != PGN_OK) continue;
        DecUnit& d = a.units[g * kStreams + s];
        // destination capacity: the frame content size (C5.hpp:588-667 sizes each stream's slot
        // exactly); VBZ's intermediate carries svb16's 16 padding bytes (signal_compression.cpp:112-118)
        const size_t cap = a.nu == 1 ? (size_t)d.cs + kVbzPadding : (size_t)d.cs;
        uint8_t* const dst = a.inter + g * a.interStride + d.interOff;
        // (the record's fields are read again for the call: kept live across the fast path they
        // pushed this kernel from 37 to 186 spilled VGPRs)
        P.mark(3);
        long r = dec_frame_fast(a.in + d.src, d.len, dst, cap, S.job, S.htab, P, sDec.hb);
        P.mark(2);  // (phase 2: the fast path, or its fall-through)
        if (r < 0) r = zstd_decompress_wave(a.in + d.src, d.len, dst, cap, S, P);
        if (lane == 0) d.dres = (int32_t)r;
        wave_sync();
    }
    P.flush();
}

// ---------------------------------------------------------------------------------------------
// Deferred four-stream Huffman sections (pgn_hufjob.h): one lane per stream, kHufFrames frames per
// wave (lane 4f + k: stream k of frame f).  The wave takes the frames of one stream type (M, keys,
// ...) of kHufFrames consecutive chunks, so its lanes' streams have nearly the same length.  The
// compact tables go to LDS; a lane keeps a 64-bit left-aligned bit container: a symbol is a peek of
// the top bits, the compact-table read, a 64-bit shift by the code length (the entry's low byte) and
// the symbol byte packed four to a word; every second symbol the container takes the next dword when
// it holds 32 bits or fewer (a code is at most 11 bits, so two symbols always fit).
//
// Memory pattern (what the loop is built around; measured: tools/gpu_k2diag.sh).
// * On gfx9 one counter (vmcnt) covers loads and stores and retires in order, so waiting for a load
//   also waits for every store issued before it.  The loop issues the same memory operations every
//   iteration, unconditionally (nothing is branched around): two 16-byte loads per 16-symbol
//   iteration, consumed at the start of the next one.
// * Input: the stream is read backwards in 16-byte blocks (block b at gtop - 16 b); dword j of block
//   b sits at ring position 4 b + 3 - j of the lane's 16-dword LDS ring ([slot][lane],
//   conflict-free), so block b is ring group b & 3.  An iteration consumes at most 176 bits (six
//   dwords), so loading blocks bc + 2 and bc + 3 (bc: the block of the next dword) one iteration
//   ahead always covers the next iteration and overwrites only consumed groups.
// * Output: whole 128-byte lines.  A lane first decodes the symbols before its destination's first
//   16-byte boundary (the head, at most 15), so each iteration's four words are an aligned block.
//   Blocks written one per iteration left 64 partial lines per wave open in L2; evicted
//   half-written, they cost more than the decode (2.84 -> 1.63 ms per 20,000 chunks with the stores
//   sent to one line).  So every lane starts 7 - m0 iterations late, m0 being its blocks before its
//   first 128-byte boundary, and after a 7-iteration prologue (those blocks stored one by one) all
//   lanes' lines end on the same iterations: the main loop runs trips of 8 iterations and stores
//   each lane's line as 8 consecutive 16-byte stores at the trip's end.
// * Lanes outside their stream's iterations are frozen: their peek reads a 16-entry zero table (code
//   length 0), their stores go to a junk line, their loads stay inside their stream.  The trips in
//   which no lane changes state run a body without the selects that freezing needs.
// The head and tail bytes are byte stores.  After its symbols a stream must end exactly at its first
// bit (the strict rule of huf_decode4_wave), else the frame's result is kDecErrHufStream.
// ---------------------------------------------------------------------------------------------
constexpr int kHufFrames = 16;
#ifndef PGN_K2_PF
#define PGN_K2_PF 1
#endif
constexpr uint32_t kPf = PGN_K2_PF;             // iterations between a block load and its staging
constexpr uint32_t kRing = 16 * kPf;            // dwords per lane (4 kPf blocks)
constexpr uint32_t kRingBlocks = kRing / 4;
constexpr uint32_t kTabStride = kJobTabUse;     // LDS table entries per frame
constexpr uint32_t kZeroTab = 16;               // frozen lanes' table entries
constexpr size_t kHufJunkBytes = 64 * 128;      // frozen lanes' store target: a line per lane, shared by all waves
static_assert((2 * kTabStride) % 16 == 0, "frame tables stay 16-byte aligned");

__device__ __forceinline__ uint64_t shl64(uint64_t c, uint32_t e)  // c << (e & 63), one v_lshlrev_b64
{
    return c << (e & 63u);
}
__device__ __forceinline__ uint32_t cnd(bool c, uint32_t a, uint32_t b)  // c ? a : b, one v_cndmask
{
    uint32_t r;
    asm volatile("v_cndmask_b32 %0, %2, %1, %3" : "=v"(r) : "v"(a), "v"(b), "s"((uint64_t)ballot(c)));
    return r;
}
__device__ __forceinline__ uint32_t pick4(bool q1, bool q2, uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    return cnd(q2, cnd(q1, d, c), cnd(q1, b, a));
}
__device__ __forceinline__ uint32_t sel4(const uint4& v, uint32_t i)
{
    return i == 0 ? v.x : (i == 1 ? v.y : (i == 2 ? v.z : v.w));
}

__global__ __launch_bounds__(64) void dec_huf_kernel(DecArgs a)
{
    __shared__ __attribute__((aligned(16))) uint16_t tabs[kHufFrames * kTabStride + kZeroTab];
    __shared__ uint32_t ring[kRing * 64];
    const uint32_t lane = (uint32_t)lane_id();
    const size_t G = a.G;
    const uint32_t ngrp = (uint32_t)((G + kHufFrames - 1) / kHufFrames);
    const uint32_t kq = blockIdx.x / ngrp;  // queue position: the large streams' groups first
    if (kq >= a.nu) return;
    const int s = unit_stream(kq);
    const size_t g0 = (size_t)(blockIdx.x % ngrp) * kHufFrames;
    const uint32_t f = lane >> 2, q = lane & 3;
    const size_t g = g0 + f;
    const bool inb = g < G && a.base + g < a.nchunks;
    const HufJob* J = (const HufJob*)(a.jobs + (inb ? (g * kStreams + (size_t)s) * kJobBytes : 0));
    const uint32_t flag = inb ? gld<uint32_t>(&J->flag) : 0u;
    const uint64_t fm = ballot(flag != 0);
    if (fm == 0) return;
    if (a.hufPrio) __builtin_amdgcn_s_setprio(3);  // ahead of the merges sharing the CU (the drain)
    // phase profile build: dec_huf's own region of the profile buffer (kHufProfOff, DecArgs.prof = +kPhases)
    PhaseProf Pp;
    Pp.init(a.prof ? a.prof + (kHufProfOff - kPhases) : nullptr);
    Pp.count(0);
    Pp.count(2, (uint64_t)__builtin_popcountll(fm));
    // the pending frames' compact tables (kTabStride entries each, 16 bytes per lane; all loads in
    // flight at once)
    {
        const uint32_t lt = lane < kTabStride / 8 ? lane : kTabStride / 8 - 1;
        uint4 tv[kHufFrames];
#pragma unroll
        for (int ff = 0; ff < kHufFrames; ff++) {
            const size_t gf = (fm >> (4 * ff)) & 1u ? g0 + (size_t)ff : g0;
            tv[ff] = gld<uint4>(a.jobs + (gf * kStreams + (size_t)s) * kJobBytes + sizeof(HufJob) + 16 * lt);
        }
#pragma unroll
        for (int ff = 0; ff < kHufFrames; ff++)
            if (lane < kTabStride / 8) *(uint4*)&tabs[ff * kTabStride + 8 * lane] = tv[ff];
        if (lane < kZeroTab / 2) ((uint32_t*)&tabs[kHufFrames * kTabStride])[lane] = 0u;
    }
    uint8_t* const junk = a.jobs + G * kStreams * kJobBytes + 128 * lane;
    Pp.mark(0);  // the job flags and the compact tables in LDS
    // this lane's stream
    uint64_t hp = 0, dstp = 0;
    uint4 len = make_uint4(0, 0, 0, 0), prm = make_uint4(0, 11, 0, 0);
    uint32_t C2 = 0;
    if (flag) {
        hp = gld<uint64_t>(&J->hp);
        dstp = gld<uint64_t>(&J->dst);
        len = gld<uint4>(&J->len[0]);
        prm = gld<uint4>(&J->rs);
        C2 = gld<uint32_t>(&J->C2);
    }
    const uint32_t rs = prm.x, tl = prm.y, d1 = prm.z & 0xFFu, d2 = prm.z >> 8, C1 = prm.w;
    const uint32_t so = (q > 0 ? len.x : 0u) + (q > 1 ? len.y : 0u) + (q > 2 ? len.z : 0u);
    const uint32_t sl = sel4(len, q);
    const uint32_t seg = (rs + 3) / 4;
    uint32_t nsym = flag ? (q == 3 ? rs - 3 * seg : seg) : 0u;
    const uint8_t* src = (const uint8_t*)hp + 6 + so;
    uint8_t* sdst = (uint8_t*)dstp + (size_t)seg * q;
    const uint32_t lastB = (flag && sl) ? (uint32_t)gb(src + sl - 1) : 0u;
    bool bad = flag && lastB == 0;
    const bool live = flag && !bad;
    if (!live) nsym = 0;
    const uint32_t sh1 = 32 - tl, shA = sh1 + d1, shB = sh1 + d2;
    // ---- bit reader.  Lanes without a stream read their junk line (readable, never decoded).
    const uint64_t e = live ? (uint64_t)src + sl - 1 : (uint64_t)junk;
    const uint64_t amin = live ? ((uint64_t)src & ~(uint64_t)15) : (uint64_t)junk;  // blocks holding stream bytes
    const uint64_t gtop = e & ~(uint64_t)15;
    const uint32_t bmax = (uint32_t)((gtop - amin) >> 4);
#if PGN_K2_DIAG == 2  // diagnostic (wrong output): every block load reads the stream's top block
    auto blk = [&](uint32_t b) { return gld<uint4>((const void*)(gtop - 16ull * (b < bmax ? b : bmax) * 0)); };
#else
    auto blk = [&](uint32_t b) { return gld<uint4>((const void*)(gtop - 16ull * (b < bmax ? b : bmax))); };
#endif
    auto stage = [&](uint32_t b, const uint4& v) {  // block b -> ring group b % kRingBlocks (highest address first)
        uint32_t* r = ring + lane + 256u * (b & (kRingBlocks - 1u));
        r[0] = v.w;
        r[64] = v.z;
        r[128] = v.y;
        r[192] = v.x;
    };
    const uint32_t hb = lastB ? z1::highbit32(lastB) : 0u;
    const uint32_t i0 = (uint32_t)(e >> 2) & 3u;
    const uint32_t v0 = live ? (uint32_t)(e & 3u) * 8u + hb : 0u;  // valid bits of the top dword
    const uint32_t totalBits = sl ? (sl - 1) * 8u + hb : 0u;
    const uint32_t ins0 = 4 - i0;  // ring position of the dword below the top one
    // insb: the ring position of the next dword times 256 (its slot's byte offset in the ring, before
    // the wrap), so a refill advances it and forms the LDS address with one instruction each
    uint32_t insb = ins0 << 8, avail = v0;
    const uint32_t laneOff = 4u * lane;
    auto ring_at = [&](uint32_t ib) -> uint32_t {  // ring[64 * ((ib >> 8) & (kRing - 1)) + lane]
        return *(const uint32_t*)((const uint8_t*)ring + ((ib & ((kRing - 1) << 8)) | laneOff));
    };
    uint64_t C;
    uint32_t nd;
    // blocks in flight: slot 0 was loaded kPf iterations ago (staged next), slot kPf - 1 last
    uint4 La[kPf], Lb[kPf];
    uint32_t lb[kPf];  // block of La (Lb: lb + 1)
    auto issue = [&](uint32_t slot) {
        lb[slot] = (insb >> 10) + 2 * kPf;
        La[slot] = blk(lb[slot]);
        Lb[slot] = blk(lb[slot] + 1);
    };
    {
        uint4 b0v[2 * kPf + 2];
#pragma unroll
        for (uint32_t k = 0; k < 2 * kPf + 2; k++) b0v[k] = blk(k);
#pragma unroll
        for (uint32_t k = 0; k < kPf; k++) {  // the loop's pattern: two loads, then one store
            issue(k);
            gst<uint4>(junk, make_uint4(0, 0, 0, 0));
        }
#pragma unroll
        for (uint32_t k = 0; k < 2 * kPf + 2; k++) stage(k, b0v[k]);
        const uint4 b0 = b0v[0];
        const uint32_t dw0 = sel4(b0, i0);
        C = v0 ? ((uint64_t)dw0 << (64 - v0)) : 0ull;
        // first refill (avail <= 31), and a second one when the container still holds only 32
        // bits: every pair of symbols starts with at least 33
        nd = ring_at(insb);
        C |= shl64((uint64_t)nd, 32u - avail);
        avail += 32;
        insb += 256;
        nd = ring_at(insb);
        if (avail <= 32) {
            C |= (uint64_t)nd;
            avail += 32;
            insb += 256;
            nd = ring_at(insb);
        }
    }
    // refill check: the dword goes into Cadd, which the next symbol ORs into the container only
    // after its table read has been issued (its peek is valid without it: a pair of symbols starts
    // with at least 33 bits and takes at most 22), so the refill is off the symbols' latency chain
    uint64_t Cadd = 0;
    auto refill = [&]() {
        const uint32_t m01 = avail <= 32 ? 1u : 0u;
        const uint32_t x = m01 ? nd : 0u;
        Cadd = shl64((uint64_t)x, 32u - avail);
        avail += m01 << 5;  // one v_lshl_add each
        insb += m01 << 8;
        nd = ring_at(insb);
    };
    // table byte addresses: entry min(p, (p >> d1) + C1, (p >> d2) + C2) of the lane's compact table
    // (pgn_hufjob.h), p = peek >> (32 - tl); tb / tc1 / tc2 carry the table base (the zero table when
    // frozen: then every candidate is the zero table's base plus a peek shift, the smallest at most 15)
    const uint32_t tbLive = f * kTabStride, tbZero = kHufFrames * kTabStride;
    uint32_t tb = tbLive, tc1 = C1 + tbLive, tc2 = C2 + tbLive, s1 = sh1;
    auto symbol = [&](bool merge) -> uint32_t {
        const uint32_t hi = (uint32_t)(C >> 32);
        const uint32_t a0 = ((hi >> s1) + tb) << 1, a1 = ((hi >> shA) + tc1) << 1, a2 = ((hi >> shB) + tc2) << 1;
        const uint32_t am = a0 < a1 ? a0 : a1;
#if PGN_K2_DIAG == 3  // diagnostic (wrong output): the table read replaced by arithmetic on the peek
        const uint32_t ent = ((am < a2 ? am : a2) & 0xFF00u) | (4u + (hi >> 30));
#else
        const uint32_t ent = *(const uint16_t*)((const uint8_t*)tabs + (am < a2 ? am : a2));
#endif
        C = shl64(merge ? (C | Cadd) : C, ent);
        avail -= ent & 0xFFu;
        return ent;
    };
    auto word4 = [&]() -> uint32_t {  // four symbols (refill checks after the second and fourth)
        const uint32_t e0 = symbol(true);
        const uint32_t e1 = symbol(false);
        refill();
        const uint32_t e2 = symbol(true);
        const uint32_t e3 = symbol(false);
        refill();
        // byte 1 of each entry: the symbol
        return __builtin_amdgcn_perm(e1, e0, 0x0C0C0501u) | __builtin_amdgcn_perm(e3, e2, 0x05010C0Cu);
    };
    auto freeze = [&](bool fz) {  // frozen: code length 0 from the zero table (peek < 16)
        tb = fz ? tbZero : tbLive;
        tc1 = fz ? tbZero : C1 + tbLive;
        tc2 = fz ? tbZero : C2 + tbLive;
        s1 = fz ? 28u : sh1;
    };
    // ---- output geometry.  The lane's first h symbols (the head: the bytes before its first 16-byte
    // boundary A0) are decoded before the iterations and stored as bytes, so super-group m (symbols
    // h + 16 m .. h + 16 m + 15) is exactly the aligned block A0 + 16 m and an iteration's four words
    // are stored as they are.  m0 blocks precede the lane's first 128-byte boundary; the lane's
    // super-group li runs in global iteration li + 7 - m0, so block m0 + 8 t + k comes out of global
    // iteration 7 + 8 t + k.
    const uint32_t h = (16u - ((uint32_t)(uintptr_t)sdst & 15u)) & 15u;  // head bytes before the first block
    const uint32_t hh = h < nsym ? h : nsym;  // (a stream shorter than its head: no iterations)
    uint8_t* A0 = sdst + h;
    const uint32_t m0 = ((128u - ((uint32_t)(uintptr_t)A0 & 127u)) & 127u) >> 4;
    const int sft = 7 - (int)m0;
    const int sg = (int)((nsym - hh) / 16);  // super-groups of 16 symbols after the head: whole blocks
    auto active = [&](int gi) { const int li = gi - sft; return li >= 0 && li < sg; };
    auto advance = [&]() {  // stage the blocks loaded an iteration ago, load the next two
        stage(lb[0], La[0]);
        stage(lb[0] + 1, Lb[0]);
#pragma unroll
        for (uint32_t k = 0; k + 1 < kPf; k++) {
            lb[k] = lb[k + 1];
            La[k] = La[k + 1];
            Lb[k] = Lb[k + 1];
        }
        issue(kPf - 1);
    };
    // the head: an iteration of its own for the ring (at most 15 symbols, 165 bits), in pairs like
    // every other symbol (a pair starts with at least 33 bits); a symbol the lane does not have is
    // frozen (code length 0, nothing consumed)
    {
        advance();
        const uint32_t hmax = wave_max(hh);
        for (uint32_t j = 0; j < hmax; j += 2) {
            freeze(j >= hh);
            const uint32_t e0 = symbol(true);
            freeze(j + 1 >= hh);
            const uint32_t e1 = symbol(false);
            refill();
            if (j < hh) gst<uint8_t>(sdst + j, (uint8_t)(e0 >> 8));
            if (j + 1 < hh) gst<uint8_t>(sdst + j + 1, (uint8_t)(e1 >> 8));
        }
        gst<uint4>(junk, make_uint4(0, 0, 0, 0));  // (the loop's pattern again: two loads, then one store)
    }
    // one global iteration: 16 symbols, the lane's block li = gi - sft when it is active (zeros when
    // not).  all: every lane is either active for the whole trip or never (no selects on active)
    auto iteration = [&](int gi, bool all) -> uint4 {
        advance();
        uint32_t W[4];
#pragma unroll
        for (int k = 0; k < 4; k++) W[k] = word4();
        if (!all) freeze(!active(gi + 1));
        return make_uint4(W[0], W[1], W[2], W[3]);
    };
    freeze(!active(0));
    // prologue: global iterations 0 .. 6, the blocks before each lane's first line one by one
    // (unrolled: the in-flight slots rotate by renaming, not by copies that would wait for the loads)
#pragma unroll
    for (int gi = 0; gi < 7; gi++) {
        const uint4 D = iteration(gi, false);
        const int m = gi - sft;
#if PGN_K2_DIAG == 1  // diagnostic (wrong output): every store to the junk line
        uint8_t* ad = junk;
#else
        uint8_t* ad = (m >= 0 && m < sg) ? A0 + 16 * m : junk;
#endif
        gst<uint4>(ad, D);
    }
    // the trip loop's pattern: loads, then eight stores (so its first wait is on the loads only)
#pragma unroll
    for (int k = 1; k < 8; k++) gst<uint4>(junk + 16 * k, make_uint4(0, 0, 0, 0));
    // trips of 8 iterations: one whole line per lane.  A lane without iterations (sg == 0: no job, a
    // bad or a short stream) keeps the zero table and its junk line throughout; the first tripsAll
    // trips have every other lane active in all eight iterations
    const int lines = sg > (int)m0 ? (sg - (int)m0 + 7) / 8 : 0;
    const int trips = (int)wave_max((uint32_t)lines);
    const int tripsAll = trips - (int)wave_max((uint32_t)(sg > 0 ? trips - (sg - (int)m0) / 8 : 0));
    uint8_t* line = sg > 0 ? A0 + 16 * m0 : junk;  // the trip's line
    const uint32_t lineStep = sg > 0 ? 128u : 0u;
    Pp.mark(1);  // stream setup, first loads, the head, the 7-iteration prologue
    Pp.count(1, (uint64_t)trips);
    Pp.count(3, (uint64_t)wave_sum(nsym));
    for (int t = 0; t < tripsAll; t++) {
        uint4 Dk[8];
#pragma unroll
        for (int k = 0; k < 8; k++) Dk[k] = iteration(0, true);
#pragma unroll
        for (int k = 0; k < 8; k++) {
#if PGN_K2_DIAG == 1
            uint8_t* ad = junk + 16 * k;
#else
            uint8_t* ad = line + 16 * k;
#endif
            gst<uint4>(ad, Dk[k]);
        }
        line += lineStep;
    }
    freeze(!active(7 + 8 * tripsAll));
    for (int t = tripsAll; t < trips; t++) {
        uint4 Dk[8];
#pragma unroll
        for (int k = 0; k < 8; k++) Dk[k] = iteration(7 + 8 * t + k, false);
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int m = (int)m0 + 8 * t + k;
#if PGN_K2_DIAG == 1
            uint8_t* ad = junk + 16 * k;
#else
            uint8_t* ad = m < sg ? line + 16 * k : junk + 16 * k;
#endif
            gst<uint4>(ad, Dk[k]);
        }
        line += lineStep;
    }
    Pp.mark(2);  // the trips of 8 iterations
#pragma unroll
    for (uint32_t k = 0; k < kPf; k++) {
        stage(lb[k], La[k]);
        stage(lb[k] + 1, Lb[k]);
    }
    freeze(false);
    C |= Cadd;
    Cadd = 0;
    // the remaining symbols one by one (fewer than 16: the ring holds them)
    for (uint32_t i = hh + 16 * (uint32_t)sg; i < nsym; i++) {
        const uint32_t ent = symbol(true);
        refill();
        gst<uint8_t>(sdst + i, (uint8_t)(ent >> 8));
    }
    // exact end: the stream's bits consumed to its first bit
    if (live) bad = (v0 + 32u * ((insb >> 8) - ins0) - avail) != totalBits;
    const uint64_t bm = ballot(bad);
    if (q == 0 && flag && ((bm >> (4 * f)) & 0xFull)) gst<int32_t>(&a.units[g * kStreams + (size_t)s].dres, (int32_t)z1::kDecErrHufStream);
    Pp.mark(3);  // drain, head / tail bytes, the last symbols, the end check
    Pp.flush();
}

// The same jobs, latency first (the last deferred pass of a call: nothing overlaps its sections
// once the frame decode has ended -- the decode's drain).  A workgroup of four waves per job, one wave
// per stream with all 64 lanes (huf_decode1of4_wave64, the cooperative decoder: speculative windows,
// a sync, an exact second pass), so a stream's ~16,000 symbols take a few 64-lane rounds instead of
// one lane's serial chain; about 2.5 times the instructions of dec_huf_kernel, on a chip that is
// otherwise waiting.  The compact table is expanded back into the full 2^tl-entry table in LDS.  Same
// symbols and the same strict end rule; a failing stream marks its frame kDecErrHufStream.
__global__ __launch_bounds__(64 * kCoopWaves) void dec_huf_wide_kernel(DecArgs a)
{
    const uint32_t u = blockIdx.x;
    const size_t G = a.G;
    if ((size_t)u >= (size_t)a.nu * G) return;
    const int s = unit_stream((uint32_t)(u / G));  // large streams first
    const size_t g = u % G;
    if (a.base + g >= a.nchunks) return;
    const HufJob* J = (const HufJob*)(a.jobs + (g * kStreams + (size_t)s) * kJobBytes);
    if (gld<uint32_t>(&J->flag) == 0) return;  // the same for every wave of the group
    __shared__ uint32_t stgAll[kCoopWaves * kCoopStgWords];
    __shared__ uint32_t bad;
    const uint32_t tid = threadIdx.x;
    const int wid = (int)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint64_t hp = gld<uint64_t>(&J->hp), dstp = gld<uint64_t>(&J->dst);
    const uint4 len = gld<uint4>(&J->len[0]);
    const uint4 prm = gld<uint4>(&J->rs);
    const uint32_t C2 = gld<uint32_t>(&J->C2);
    const uint32_t rs = prm.x, tl = prm.y, d1 = prm.z & 0xFFu, d2 = prm.z >> 8, C1 = prm.w;
    // the full table from the compact one: entry min(p, (p >> d1) + C1, (p >> d2) + C2), swapped back
    // to symbol | nbBits << 8
    const uint16_t* ct = (const uint16_t*)(a.jobs + (g * kStreams + (size_t)s) * kJobBytes + sizeof(HufJob));
    for (uint32_t p = tid; p < (1u << tl); p += 64 * kCoopWaves) {
        const uint32_t i1 = (p >> d1) + C1, i2 = (p >> d2) + C2;
        uint32_t i = p < i1 ? p : i1;
        i = i < i2 ? i : i2;
        const uint32_t c = gld<uint16_t>(ct + i);
        sDec.tab[p] = (uint16_t)((c >> 8) | ((c & 0xFFu) << 8));
    }
    if (tid == 0) bad = 0;
    __syncthreads();
    PhaseProf P;
    P.init(nullptr);
    const size_t remain = 6 + (size_t)len.x + len.y + len.z + len.w;
    const bool ok = huf_decode1of4_wave64(tl, (const uint8_t*)hp, remain, (uint8_t*)dstp, rs, len.x | (len.y << 16), len.z,
                                          wid, (lds_u32*)&stgAll[wid * kCoopStgWords + 2 * 64], P);
    if (!ok && lane_id() == 0) atomicOr(&bad, 1u);
    __syncthreads();
    if (tid == 0 && bad) gst<int32_t>(&a.units[g * kStreams + (size_t)s].dres, (int32_t)z1::kDecErrHufStream);
}

// Small batches (the per-chunk calls): one workgroup of kCoopWaves waves per work unit.  Wave 0
// decodes the frame; the four Huffman streams of each literals section are decoded by the four
// waves at once, 64 lanes per stream (pgn_zdec.h CoopCmd).  A lone 100,000-sample chunk's decode
// is bound by its largest frame's Huffman rounds, which this cuts about fourfold.
constexpr size_t kCoopMaxChunks = 64;  // batches up to this many chunks use it
__global__ __launch_bounds__(64 * kCoopWaves) void dec_zstd_coop_kernel(DecArgs a)
{
    const int lane = lane_id();
    const int wid = (int)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t G = a.G;
    const uint32_t u = blockIdx.x;
    if ((size_t)u >= (size_t)a.nu * G) return;
    const int s = a.nu == 1 ? 0 : unit_stream((uint32_t)(u / G));
    const size_t g = u % G;
    const size_t c = a.base + g;
    if (c >= a.nchunks) return;
    __shared__ int32_t parseRc;
    __shared__ DecUnit myUnit;
    if (a.coopParse) {  // the chunk's prefixes and frame headers (dec_parse_kernel's work), here
        if (threadIdx.x == 0) {
            DecUnit uu[kStreams];
            const int rc = a.sampleCounts[c] > kPassSamples ? PGN_ERR_UNSUPPORTED
                                                            : c5_parse_chunk(a.in, a.inOffsets[c], a.inSizes[c], uu,
                                                                             inter_cap(a.capN));
            parseRc = rc;
            if (rc == PGN_OK) myUnit = uu[s];
            if (s == 0) {  // the chunk's first frame publishes its status and frame records for the merge
                a.status[c] = rc;
                if (rc == PGN_OK) {
                    for (int k = 0; k < kStreams; k++) {
                        DecUnit& w = a.units[g * kStreams + k];
                        w.src = uu[k].src;
                        w.len = uu[k].len;
                        w.cs = uu[k].cs;
                        w.interOff = uu[k].interOff;
                    }
                }
            }
        }
        __syncthreads();
        if (parseRc != PGN_OK) return;  // the same for every wave of the group
    } else {
        if (a.status[c] != PGN_OK) return;
        if (threadIdx.x == 0) myUnit = a.units[g * kStreams + s];
        __syncthreads();
    }
    PhaseProf P;
    P.init(a.prof);
    __shared__ uint32_t stgAll[kCoopWaves * kCoopStgWords];
    __shared__ CoopCmd cmdLds;
    lds_cmd* cmd = (lds_cmd*)&cmdLds;
    lds_u32* stg = (lds_u32*)&stgAll[wid * kCoopStgWords + 2 * 64];
    if (wid != 0) {
        coop_helper_wave(wid, cmd, stg, P);
        P.flush();
        return;
    }
    const DecLayout lay = dec_layout();
    uint8_t* sbase = a.slotScratch + (size_t)u * a.slotBytes;
    DecScratch S;
    S.lit = sbase + lay.lit;
    S.tables = (uint32_t*)(sbase + lay.tables);
    S.htab = (uint16_t*)(sbase + lay.htab);
    S.coopCmd = cmd;
    S.coopStg = stg;
    S.job = nullptr;
    const uint64_t dsrc = myUnit.src;
    const uint32_t dlen = myUnit.len, dcs = myUnit.cs, doff = myUnit.interOff;
    const size_t cap = a.nu == 1 ? (size_t)dcs + kVbzPadding : (size_t)dcs;
    const long r = zstd_decompress_wave<true>(a.in + dsrc, dlen, a.inter + g * a.interStride + doff, cap, S, P);
    if (lane == 0) a.units[g * kStreams + s].dres = (int32_t)r;
    coop_finish(cmd);
    P.flush();
}

// The staged C5 merge, one wave per chunk, for the output element T (the sample sink, pgn_c5.h):
// dec_merge_kernel writes the int16 samples, dec_merge_pa_kernel<float / _Float16> the calibrated ones.
template <class T>
__device__ __forceinline__ void dec_merge_body(const DecArgs& a, MergeLds& W)
{
    const size_t g = blockIdx.x;
    const size_t c = a.base + g;
    if (g >= a.G || c >= a.nchunks) return;
    if (a.status[c] != PGN_OK) return;
    PhaseProf P;
    P.init(a.prof);
#if PGN_MERGE_DIAG == 1  // diagnostic: chunk g merges chunk g % 32's intermediate (L2-resident reads, same work on equal-size chunks)
    const size_t gi = g % 32;
#else
    const size_t gi = g;
#endif
    const DecUnit* d = a.units + gi * kStreams;
    uint64_t total = 0;
    int st = PGN_OK;
    for (int s = 0; s < kStreams; s++) {
        if (d[s].dres < 0) st = PGN_ERR_ZSTD_DECOMPRESS;
        total += d[s].cs;
    }
    if (st == PGN_OK) {
        uint64_t consumed = 0;
        const int bad = c5_merge_wave(a.inter + gi * a.interStride, total, (uint64_t)d[1].dres, (uint64_t)d[2].dres,
                                      (uint64_t)d[3].dres, out_chunk<T>(a, c), a.sampleCounts[c], &consumed, W,
                                      cal_chunk<T>(a, c));
        if (bad) st = PGN_ERR_CORRUPT;
        else if (consumed != total) st = PGN_ERR_REMAINING;
    }
    if (lane_id() == 0) a.status[c] = st;
    P.mark(6);
    P.flush();
}

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(6))) void dec_merge_kernel(DecArgs a)
{
    static __shared__ MergeLds W;
    dec_merge_body<int16_t>(a, W);
}
template <class T>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(6))) void dec_merge_pa_kernel(DecArgs a)
{
    static __shared__ MergeLds W;
    dec_merge_body<T>(a, W);
}

constexpr size_t kMergeWgMaxChunks = 64;  // batches up to this many chunks take the small-batch kernels

// Small batches, many CUs per chunk: the chunk's steps in kMergeRanges ranges, one single-wave
// workgroup each, so a lone chunk's merge runs on kMergeRanges CUs instead of one.  The ranges find
// their places without another launch: each publishes its class counts, then (after summing those of
// the ranges before it) the delta sum of its stream bytes, then its result, as tagged 64-bit words
// (this call's epoch in bits 48..63) that later ranges wait for -- decoupled look-back; a workgroup
// only waits on lower-numbered ones, which the dispatcher started first.  The last range sets the
// status once every range is done.  Same bytes and statuses as dec_merge_kernel.
constexpr int kMergeRanges = 32;
template <class T>
__device__ __forceinline__ void dec_merge_lb_body(const DecArgs& a, MergeLds& W)
{
    const size_t g = blockIdx.x / kMergeRanges;
    const uint32_t r = blockIdx.x % kMergeRanges;
    const size_t c = a.base + g;
    if (g >= a.G || c >= a.nchunks) return;
    if (a.status[c] != PGN_OK) return;
    const uint32_t lane = (uint32_t)lane_id();
#if PGN_MERGE_DIAG == 1  // diagnostic: chunk g merges chunk g % 32's intermediate (L2-resident reads, same work on equal-size chunks)
    const size_t gi = g % 32;
#else
    const size_t gi = g;
#endif
    const DecUnit* d = a.units + gi * kStreams;
    uint64_t total = 0;
    int st = PGN_OK;
    for (int s = 0; s < kStreams; s++) {
        if (d[s].dres < 0) st = PGN_ERR_ZSTD_DECOMPRESS;
        total += d[s].cs;
    }
    if (st != PGN_OK) {  // the same for every range of the chunk
        if (r == 0 && lane == 0) a.status[c] = st;
        return;
    }
    uint64_t* lb = a.lookback + g * (3 * kMergeRanges);
    const uint64_t ep = a.epoch;
    const uint32_t n = a.sampleCounts[c];
    const uint8_t* in = a.inter + g * a.interStride;
    T* out = out_chunk<T>(a, c);
    const uint64_t dS = (uint64_t)d[1].dres, dM = (uint64_t)d[2].dres, dLl = (uint64_t)d[3].dres;
    const uint64_t kl = ((uint64_t)n + 3) / 4;
    const uint64_t ps = kl, pm = kl + dS, pl = kl + dS + dM, ph = kl + dS + dM + dLl;
    const uint32_t steps = (n + kSplitStep - 1) / kSplitStep;
    const uint32_t s0 = (uint32_t)((uint64_t)steps * r / kMergeRanges), s1 = (uint32_t)((uint64_t)steps * (r + 1) / kMergeRanges);
    const uint32_t t0 = s0 * kSplitStep, t1 = s1 * kSplitStep < n ? s1 * kSplitStep : n;
    // 1. own class counts (16 bits each: a range has at most 16 steps below PGN pass sizes)
    uint32_t cS = 0, cM = 0, cL = 0;
    if (kl <= total) c5_class_counts(in, n, t0, t1, cS, cM, cL);
    if (lane == 0) lb_publish(lb + 3 * r, ep, (uint64_t)cS | ((uint64_t)cM << 16) | ((uint64_t)cL << 32));
    // 2. the counts before me -> my stream spans -> my delta sum
    const uint64_t pc = lb_wait(lb, 0, r, ep);
    const uint64_t sN0 = wave_sum64(pc & 0xFFFFu), mN0 = wave_sum64((pc >> 16) & 0xFFFFu), lN0 = wave_sum64(pc >> 32);
    const uint64_t sN1 = sN0 + cS, mN1 = mN0 + cM, lN1 = lN0 + cL;
    const bool inside = kl <= total && ps + ((sN1 + 1) >> 1) <= total && pm + mN1 <= total && pl + lN1 <= total &&
                        ph + lN1 <= total;
    uint32_t sum = 0;
    if (inside) sum = c5_range_delta_sum(in, ps, pm, pl, ph, sN0, sN1, mN0, mN1, lN0, lN1);
    if (lane == 0) lb_publish(lb + 3 * r + 1, ep, (uint64_t)sum | ((uint64_t)(inside ? 0u : 1u) << 32));
    // 3. the running sum at my start: the sums before me; merge unless a range so far is outside
    const uint64_t ps_ = lb_wait(lb, 1, r, ep);
    const uint32_t carryIn = (uint32_t)wave_sum64(ps_ & 0xFFFFu);
    const bool outsideBefore = wave_sum64((ps_ >> 32) & 1u) != 0;
    int bad = (!inside || outsideBefore) ? 1 : 0;
    if (!bad) {
        uint32_t carry = carryIn;
        uint64_t lEnd = 0;
        bad = c5_merge_range<false>(in, total, dS, dM, dLl, out, n, t0, t1, sN0, mN0, lN0, carry, &lEnd, W, cal_chunk<T>(a, c));
    }
    if (lane == 0) lb_publish(lb + 3 * r + 2, ep, (uint64_t)(bad ? 1u : 0u));
    // 4. the last range: every range done -> status
    if (r == kMergeRanges - 1) {
        const uint64_t dn = lb_wait(lb, 2, kMergeRanges, ep);
        const bool badAny = wave_sum64(dn & 1u) != 0;
        const uint64_t lTot = lN1;  // the class-3 count through the last range
        if (lane == 0) {
            __threadfence();
            a.status[c] = badAny ? PGN_ERR_CORRUPT : ((ph + lTot != total) ? PGN_ERR_REMAINING : PGN_OK);
        }
    }
}

__global__ __launch_bounds__(64) void dec_merge_lb_kernel(DecArgs a)
{
    __shared__ MergeLds W;
    dec_merge_lb_body<int16_t>(a, W);
}
template <class T>
__global__ __launch_bounds__(64) void dec_merge_lb_pa_kernel(DecArgs a)
{
    __shared__ MergeLds W;
    dec_merge_lb_body<T>(a, W);
}


// ---------------------------------------------------------------------------------------------
// VBZ (pod5::compress_signal / decompress_signal, signal_compression.cpp:37-141): split -> one
// zstd frame per chunk -> copy into place; parse -> zstd decode -> svb16 merge.  The per-chunk
// buffers are the C5 ones (a chunk's stream area holds its svb16 buffer, <= 2.125 n bytes).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void vbz_split_kernel(EncArgs a)
{
    static __shared__ VbzSplitLds W;
    const size_t g = blockIdx.x;
    const size_t c = a.base + g;
    if (g >= a.G || c >= a.nchunks) return;
    PhaseProf P;
    P.init(a.prof);
    const uint32_t n = a.sampleCounts[c];
    uint32_t* sz = a.sizes + g * kStreams;
    if (n > kPassSamples) {  // the large-chunk pass takes it
        if (lane_id() == 0) {
            sz[0] = ~0u;
            a.status[c] = PGN_ERR_UNSUPPORTED;
            a.outSizes[c] = 0;
        }
        return;
    }
    // place the buffer so that its data part (after the ceil(n/8) key bytes) is 16-byte aligned
    const uint32_t pad = (16u - (svb_key_length(n) & 15u)) & 15u;
    const uint32_t m = vbz_split_wave(a.samples + a.sampleOffsets[c], n, a.streams + g * kChunkStreamBytes + pad, W);
    if (lane_id() == 0) {
        sz[0] = m;
        sz[1] = pad;
    }
    P.mark(0);
    P.flush();
}

__global__ __launch_bounds__(64) void vbz_assemble_kernel(EncArgs a)
{
    const size_t g = blockIdx.x;
    const size_t c = a.base + g;
    if (g >= a.G || c >= a.nchunks) return;
    const int lane = lane_id();
    const uint32_t* sz = a.sizes + g * kStreams;
    if (sz[0] == ~0u) return;
    const uint32_t fs = a.fsizes[g * kStreams];
    // ZSTD_compress into the caller's span fails when the frame does not fit
    // (signal_compression.cpp:57-62 "Failed to compress data")
    const bool ok = fs <= a.outCaps[c];
    if (ok) wave_copy(a.out + a.outOffsets[c], a.frames + g * kChunkFrameBytes, fs);
    if (lane == 0) {
        a.status[c] = ok ? PGN_OK : PGN_ERR_ZSTD_COMPRESS;
        a.outSizes[c] = ok ? fs : 0;
        if (a.stats) {
            for (int s = 0; s < PGN_STATS_PER_CHUNK; s++) a.stats[c * PGN_STATS_PER_CHUNK + s] = 0;
            a.stats[c * PGN_STATS_PER_CHUNK] = sz[0];
            a.stats[c * PGN_STATS_PER_CHUNK + 5] = fs;
        }
    }
}

// one thread per chunk: ZSTD_getFrameContentSize (signal_compression.cpp:100-109)
__global__ __launch_bounds__(64) void vbz_parse_kernel(DecArgs a)
{
    const size_t g = (size_t)blockIdx.x * 64 + lane_id();
    const size_t c = a.base + g;
    if (g >= a.G || c >= a.nchunks) return;
    DecUnit* u = a.units + g * kStreams;
    bool ok = false;
    const uint64_t src0 = a.inOffsets[c], len = a.inSizes[c];
    const uint64_t cs = z1::frame_content_size(a.in + src0, (size_t)len, &ok);
    int st = PGN_OK;
    if (a.sampleCounts[c] > kPassSamples) st = PGN_ERR_UNSUPPORTED;  // the large-chunk pass takes it
    else if (!ok) st = PGN_ERR_NOT_ZSTD;
    else if (len > 0xFFFFFFFFull) st = PGN_ERR_UNSUPPORTED;
    else if (cs + kVbzPadding > inter_cap(a.capN)) {
        u->src = src0;
        u->len = (uint32_t)len;
        st = over_claim_status(a.in, u, &cs, 1);
    } else {
        u->src = src0;
        u->len = (uint32_t)len;
        u->cs = (uint32_t)cs;
        u->interOff = 0;
        u->dres = 0;
    }
    a.status[c] = st;
}

template <class T>
__device__ __forceinline__ void vbz_merge_body(const DecArgs& a, VbzMergeLds& W)
{
    const size_t g = blockIdx.x;
    const size_t c = a.base + g;
    if (g >= a.G || c >= a.nchunks) return;
    if (a.status[c] != PGN_OK) return;
    PhaseProf P;
    P.init(a.prof);
    const DecUnit* d = a.units + g * kStreams;
    int st = PGN_OK;
    if (d->dres < 0) {
        st = PGN_ERR_ZSTD_DECOMPRESS;
    } else {
        // svb16::decode over the padded intermediate, then "consumed + padding == size"
        // (signal_compression.cpp:124-131): bytes past the content but inside the padding are the
        // "Remaining data" error, beyond it the reference reads out of bounds
        uint64_t consumed = 0;
        const uint32_t n = a.sampleCounts[c];
        const uint64_t total = (uint64_t)d->cs + kVbzPadding;
        if (svb_key_length(n) > d->cs) {  // keys alone run into the padding (or past it)
            st = svb_key_length(n) <= total ? PGN_ERR_REMAINING : PGN_ERR_CORRUPT;
        } else {
            const int bad = vbz_merge_wave(a.inter + g * a.interStride, total, out_chunk<T>(a, c), n, &consumed, W,
                                           cal_chunk<T>(a, c));
            if (bad) st = PGN_ERR_CORRUPT;
            else if (consumed != d->cs) st = PGN_ERR_REMAINING;
        }
    }
    if (lane_id() == 0) a.status[c] = st;
    P.mark(6);
    P.flush();
}

__global__ __launch_bounds__(64) void vbz_merge_kernel(DecArgs a)
{
    static __shared__ VbzMergeLds W;
    vbz_merge_body<int16_t>(a, W);
}
template <class T>
__global__ __launch_bounds__(64) void vbz_merge_pa_kernel(DecArgs a)
{
    static __shared__ VbzMergeLds W;
    vbz_merge_body<T>(a, W);
}

// ---------------------------------------------------------------------------------------------
// Fused per-chunk pipeline.  One persistent wave takes whole chunks from a queue:
//   encode: split into its slot's stream area -> the chunk's zstd frames written straight into its
//           blob behind their length prefixes -> size, status, stats;
//   decode: prefixes and frame headers -> the frames decoded into its slot's intermediate -> merge
//           into the samples, consumed-bytes check.
// Waves in different stages share each CU (VALU-bound split/merge beside latency-bound entropy
// coding), a chunk's streams are re-read by the wave that just wrote them, and frames are never
// staged and copied.  The split/merge LDS overlays the zstd stage's (stages of one wave never
// overlap in time).  Every codec runs here; C5 and VBZ also have the staged pipeline above.
// ---------------------------------------------------------------------------------------------
static_assert(sizeof(SplitLds) <= sizeof(EncLds) && sizeof(VbzSplitLds) <= sizeof(EncLds) &&
                  sizeof(Vbz0SplitLds) <= sizeof(EncLds),
              "split LDS overlay");
static_assert(sizeof(MergeLds) <= sizeof(DecLds) && sizeof(VbzMergeLds) <= sizeof(DecLds) &&
                  sizeof(Vbz0MergeLds) <= sizeof(DecLds),
              "merge LDS overlay");

// Frames per chunk: C5/C4 5, C3 4, C2 3, C1 2, VBZ/VBZ0 1 (pgnano/svb16/C*.hpp, VBZ_0.hpp)
__host__ __device__ constexpr int codec_frames(int codec)
{
    return codec == kCodecC5 || codec == kCodecC4 ? 5 : (codec == kCodecC3 ? 4 : (codec == kCodecC2 ? 3 : (codec == kCodecC1 ? 2 : 1)));
}

// slot scratch of the fused kernels for chunks of up to capN samples: the zstd scratch, then the
// chunk's streams (encode: + one frame for a stream that may not fit the destination; any one
// stream's frame, a VBZ / C1 svb16 buffer of up to ~2.13 capN the largest) or its intermediate
// (decode)
__host__ __device__ inline size_t slot_frame_bytes(uint32_t capN) { return align_up(frame_bound((size_t)capN * 9 / 4 + 64) + 64, 256); }
__host__ __device__ inline size_t enc_slot_bytes(uint32_t capN = kPassSamples)
{
    return enc_layout().bytes + chunk_stream_bytes(capN) + slot_frame_bytes(capN);
}
__host__ __device__ inline size_t dec_slot_bytes(uint32_t capN = kPassSamples) { return dec_layout().bytes + chunk_inter_bytes(capN); }

// The split and merge stages as non-inlined calls with wave-uniform arguments: each gets its own
// register allocation instead of sharing the kernel's with the state kept across the zstd calls
// (inlined, both spilled to scratch inside their step loops).
struct SplitOut {
    uint32_t s[kStreams];
};
template <bool C4>
__device__ __noinline__ SplitOut c5_split_chunk(const int16_t* x, uint32_t n, uint8_t* streams, uint32_t capN)
{
    x = uni(x);
    n = uni(n);
    streams = uni(streams);
    capN = uni(capN);
    C5Streams st{streams + stream_off(0, capN), streams + stream_off(1, capN), streams + stream_off(2, capN),
                 streams + stream_off(3, capN), streams + stream_off(4, capN)};
    SplitOut o;
    c5_split_wave<C4>(x, n, st, o.s, *reinterpret_cast<SplitLds*>(&sEnc));
    return o;
}
template <bool C3>
__device__ __noinline__ SplitOut c23_split_chunk(const int16_t* x, uint32_t n, uint8_t* streams, uint32_t capN)
{
    x = uni(x);
    n = uni(n);
    streams = uni(streams);
    capN = uni(capN);
    SplitOut o;
    c23_split_wave<C3>(x, n, streams + stream_off(0, capN), streams + stream_off(2, capN), streams + stream_off(3, capN),
                       streams + stream_off(4, capN), o.s);
    return o;
}
__device__ __noinline__ uint32_t vbz_split_chunk(const int16_t* x, uint32_t n, uint8_t* out)
{
    return vbz_split_wave(uni(x), uni(n), uni(out), *reinterpret_cast<VbzSplitLds*>(&sEnc));
}
__device__ __noinline__ uint32_t vbz0_split_chunk(const int16_t* x, uint32_t n, uint8_t* out)
{
    return vbz0_split_wave(uni(x), uni(n), uni(out), *reinterpret_cast<Vbz0SplitLds*>(&sEnc));
}
struct MergeOut {
    int bad;
    uint64_t consumed;
};
// T: the output element of the sample sink; its calibration arrives with the other arguments (none
// for the int16 samples: an empty argument)
template <class T>
struct CalArg {
    float off, scale;
    __device__ __forceinline__ Cal get() const { return Cal{uni(off), uni(scale)}; }
};
template <>
struct CalArg<int16_t> {
    __device__ __forceinline__ Cal get() const { return Cal{0.f, 0.f}; }
};
template <bool C4, class T>
__device__ __noinline__ MergeOut c5_merge_chunk(const uint8_t* in, uint64_t total, uint64_t dS, uint64_t dM, uint64_t dLl,
                                                T* out, uint32_t n, CalArg<T> ca)
{
    MergeOut o{0, 0};
    o.bad = c5_merge_wave<C4>(uni(in), uni(total), uni(dS), uni(dM), uni(dLl), uni(out), uni(n), &o.consumed,
                              *reinterpret_cast<MergeLds*>(&sDec), ca.get());
    return o;
}
template <bool C3, class T>
__device__ __noinline__ MergeOut c23_merge_chunk(const uint8_t* in, uint64_t total, uint64_t dA, uint64_t dB, T* out,
                                                 uint32_t n, CalArg<T> ca)
{
    MergeOut o{0, 0};
    o.bad = c23_merge_wave<C3>(uni(in), uni(total), uni(dA), uni(dB), uni(out), uni(n), &o.consumed, ca.get());
    return o;
}
template <class T>
__device__ __noinline__ MergeOut vbz_merge_chunk(const uint8_t* in, uint64_t total, T* out, uint32_t n, CalArg<T> ca)
{
    MergeOut o{0, 0};
    o.bad = vbz_merge_wave(uni(in), uni(total), uni(out), uni(n), &o.consumed, *reinterpret_cast<VbzMergeLds*>(&sDec),
                           ca.get());
    return o;
}
template <class T>
__device__ __noinline__ MergeOut vbz0_merge_chunk(const uint8_t* in, uint64_t total, T* out, uint32_t n, CalArg<T> ca)
{
    MergeOut o{0, 0};
    o.bad = vbz0_merge_wave(uni(in), uni(total), uni(out), uni(n), &o.consumed, *reinterpret_cast<Vbz0MergeLds*>(&sDec),
                            ca.get());
    return o;
}

__device__ __forceinline__ void enc_fail_chunk(const EncArgs& a, size_t c, int st)
{
    if (lane_id() == 0) {
        a.status[c] = st;
        a.outSizes[c] = 0;
    }
}

template <int Codec>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5))) void enc_chunk_kernel(EncArgs a)
{
    constexpr int nf = codec_frames(Codec);
    // VBZ and VBZ0 compress straight into the destination span: a frame that does not fit fails
    // (signal_compression.cpp:57-62, VBZ_0.hpp:345-350); the multi-frame variants check the total
    // (C5.hpp:412-427) and report the required size
    constexpr bool oneFrame = nf == 1;
    const int lane = lane_id();
    const EncLayout lay = enc_layout();
    uint8_t* sbase = a.slotScratch + (size_t)blockIdx.x * a.slotBytes;
    EncScratch S;
    S.ht = (uint32_t*)(sbase + lay.ht);
    S.seqs = (z1::Seq*)(sbase + lay.seqs);
    S.codes = sbase + lay.codes;
    S.lit = sbase + lay.lit;
    S.seqSection = sbase + lay.seqSection;
    S.seqWork = (z1::SeqWork*)(sbase + lay.seqWork);
    S.maxSeq = kMaxEncSeq;
    S.huf = (uint32_t*)(sbase + lay.huf);
    S.coop = nullptr;
    const uint32_t capN = a.capN;
    uint8_t* streams = sbase + lay.bytes;
    uint8_t* fbuf = streams + chunk_stream_bytes(capN);
    uint32_t epoch = a.epochs[blockIdx.x];  // table state: epoch tag | written extent << 8 (ht_next_epoch)
    PhaseProf P;
    P.init(a.prof, a.prof);  // (the encode's search attribution: PhaseProf::ext)
    while (true) {
        uint32_t u = 0;
        if (lane == 0) u = atomicAdd(a.queue, 1u);
        u = __builtin_amdgcn_readfirstlane(u);
        if (u >= a.nchunks) break;
        const size_t c = a.list ? a.list[u] : u;
        const uint32_t n = a.sampleCounts[c];
        if (n > capN) {  // the large-chunk pass takes it (or reports it unsupported)
            enc_fail_chunk(a, c, PGN_ERR_UNSUPPORTED);
            continue;
        }
        const int16_t* x = a.samples + a.sampleOffsets[c];
        uint32_t sz[kStreams] = {0, 0, 0, 0, 0};
        const uint8_t* src[kStreams] = {streams, streams, streams, streams, streams};
        if (Codec == kCodecVbz || Codec == kCodecC1) {
            // svb16 keys | data, the data part 16-byte aligned (as in vbz_split_kernel)
            const uint32_t pad = (16u - (svb_key_length(n) & 15u)) & 15u;
            const uint32_t m = vbz_split_chunk(x, n, streams + pad);
            src[0] = streams + pad;
            if (Codec == kCodecVbz) {
                sz[0] = m;
            } else {  // C1: the keys frame and the data frame (C1.hpp:229-266)
                sz[0] = n ? svb_key_length(n) : 0u;
                sz[1] = m - sz[0];
                src[1] = src[0] + sz[0];
            }
        } else if (Codec == kCodecVbz0) {
            sz[0] = vbz0_split_chunk(x, n, streams);
        } else if (Codec == kCodecC2 || Codec == kCodecC3) {
            const SplitOut so = c23_split_chunk<Codec == kCodecC3>(x, n, streams, capN);
#pragma unroll
            for (int s = 0; s < kStreams; s++) sz[s] = so.s[s];
            src[0] = streams + stream_off(0, capN);
            src[1] = streams + stream_off(2, capN);
            src[2] = streams + stream_off(Codec == kCodecC3 ? 3 : 4, capN);
            src[3] = streams + stream_off(4, capN);
        } else {
            const SplitOut so = c5_split_chunk<Codec == kCodecC4>(x, n, streams, capN);
#pragma unroll
            for (int s = 0; s < kStreams; s++) {
                sz[s] = so.s[s];
                src[s] = streams + stream_off(s, capN);
            }
        }
#pragma unroll
        for (int s = 0; s < kStreams; s++) sz[s] = uni(sz[s]);
        bool big = false;  // a stream above the encoder's largest frame (not reached below the chunk limit)
#pragma unroll
        for (int s = 0; s < nf; s++) big |= sz[s] > kMaxFrameBytes;
        if (big) {
            enc_fail_chunk(a, c, PGN_ERR_UNSUPPORTED);
            continue;
        }
        P.mark(0);
        P.count(9, (n + 1023) / 1024);
        wave_sync();
        uint8_t* dst = a.out + a.outOffsets[c];
        const uint64_t cap = a.outCaps[c];
        uint64_t off = 0;
        bool ok = true;
        uint32_t fs[kStreams] = {0, 0, 0, 0, 0};
#pragma unroll
        for (int s = 0; s < nf; s++) {
            if (s < nf - 1) off += 8;  // length prefixes of all frames but the last (C5.hpp:429-462)
            ht_next_epoch(S.ht, epoch, sz[s]);
            // straight into the blob when the frame bound fits the capacity; otherwise through the
            // slot's frame buffer (the reference compresses into its own buffers, then checks)
            const bool direct = ok && off + frame_bound(sz[s]) <= cap;
            const size_t f = uni(zstd1_compress_wave(direct ? dst + off : fbuf, src[s], sz[s], S, epoch & 0xFFu, P));
            wave_sync();
            if (!direct && ok) {
                if (off + f <= cap) wave_copy(dst + off, fbuf, f);
                else ok = false;
                wave_sync();
            }
            if (s < nf - 1 && ok && lane == 0) {
                const uint64_t v = f;
                __builtin_memcpy(dst + off - 8, &v, 8);
            }
            fs[s] = (uint32_t)f;
            off += f;
        }
        P.mark(10);
        if (lane == 0) {
            if (oneFrame) {
                a.status[c] = ok ? PGN_OK : PGN_ERR_ZSTD_COMPRESS;
                a.outSizes[c] = ok ? off : 0;
            } else {
                a.status[c] = ok ? PGN_OK : PGN_ERR_DST_TOO_SMALL;
                a.outSizes[c] = off;  // the reference's "Required size" on failure
            }
            if (a.stats) {
                for (int s = 0; s < kStreams; s++) {
                    a.stats[c * PGN_STATS_PER_CHUNK + s] = s < nf ? sz[s] : 0;
                    a.stats[c * PGN_STATS_PER_CHUNK + 5 + s] = s < nf ? fs[s] : 0;
                }
            }
        }
        wave_sync();
    }
    if (lane == 0) a.epochs[blockIdx.x] = epoch;
    P.flush();
}

// nf frames behind nf-1 length prefixes (the decompress_signal_* front half, C5.hpp:477-586):
// frame records with content sizes and intermediate offsets; the frames together must fit the
// slot's intermediate.
template <int NF>
__device__ inline int parse_frames(const uint8_t* in, uint64_t src0, uint64_t len, DecUnit* u, uint64_t* total,
                                   size_t interCap)
{
    const uint8_t* src = in + src0;
    uint64_t pos = 0, cs[kStreams];
    for (int s = 0; s < NF; s++) {
        uint64_t fl;
        if (s < NF - 1) {
            if (pos > len || len - pos < 8) return PGN_ERR_CORRUPT;
            fl = ld64u(src + pos);
            pos += 8;
            if (fl > len - pos) return PGN_ERR_CORRUPT;
        } else {
            fl = len - pos;  // the last frame's length is implicit
        }
        bool ok = false;
        cs[s] = z1::frame_content_size(src + pos, (size_t)fl, &ok);
        if (!ok) return PGN_ERR_NOT_ZSTD;
        if (fl > 0xFFFFFFFFull) return PGN_ERR_UNSUPPORTED;
        u[s].src = src0 + pos;
        u[s].len = (uint32_t)fl;
        pos += fl;
    }
    uint64_t off = 0;
    for (int s = 0; s < NF; s++) {
        if (cs[s] > interCap - kVbzPadding - off) return over_claim_status(in, u, cs, NF);
        u[s].cs = (uint32_t)cs[s];
        u[s].interOff = (uint32_t)off;
        off += cs[s];
    }
    *total = off;
    return PGN_OK;
}

// the merge of one chunk's decoded frames (d, in the intermediate `inter`) by codec
template <int Codec, class T>
__device__ __forceinline__ MergeOut merge_chunk(const uint8_t* inter, uint64_t total, const DecUnit* d, T* out, uint32_t n,
                                                CalArg<T> ca)
{
    MergeOut mo{0, 0};
    if (Codec == kCodecVbz) {
        // svb16::decode over content + 16 padding bytes, then "consumed + padding == size"
        // (signal_compression.cpp:100-131): keys running into the padding are "Remaining data"
        const uint64_t padded = total + kVbzPadding;
        if (svb_key_length(n) > total) {
            mo.bad = svb_key_length(n) <= padded ? 2 : 1;
        } else {
            mo = vbz_merge_chunk(inter, padded, out, n, ca);
        }
    } else if (Codec == kCodecC1) {
        mo = vbz_merge_chunk(inter, total, out, n, ca);
    } else if (Codec == kCodecVbz0) {
        mo = vbz0_merge_chunk(inter, total, out, n, ca);
    } else if (Codec == kCodecC2 || Codec == kCodecC3) {
        mo = c23_merge_chunk<Codec == kCodecC3>(inter, total, (uint64_t)d[1].dres,
                                                Codec == kCodecC3 ? (uint64_t)d[2].dres : 0ull, out, n, ca);
    } else {
        mo = c5_merge_chunk<Codec == kCodecC4>(inter, total, (uint64_t)d[1].dres, (uint64_t)d[2].dres,
                                               (uint64_t)d[3].dres, out, n, ca);
    }
    return mo;
}

template <int Codec>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4))) void dec_chunk_kernel(DecArgs a)
{
    constexpr int nf = codec_frames(Codec);
    const int lane = lane_id();
    const DecLayout lay = dec_layout();
    uint8_t* sbase = a.slotScratch + (size_t)blockIdx.x * a.slotBytes;
    DecScratch S;
    S.lit = sbase + lay.lit;
    S.tables = (uint32_t*)(sbase + lay.tables);
    S.htab = (uint16_t*)(sbase + lay.htab);
    S.coopCmd = nullptr;
    S.coopStg = nullptr;
    S.job = nullptr;
    uint8_t* inter = sbase + lay.bytes;
    const uint32_t capN = a.capN;
    PhaseProf P;
    P.init(a.prof);
    while (true) {
        uint32_t u = 0;
        if (lane == 0) u = atomicAdd(a.queue, 1u);
        u = __builtin_amdgcn_readfirstlane(u);
        if (u >= a.nchunks) break;
        const size_t c = a.list ? a.list[u] : u;
        const uint32_t n = a.sampleCounts[c];
        DecUnit d[kStreams];
        uint64_t total = 0;
        // the claims pass (a.interBytes): any sample count, the frames in an intermediate sized from
        // the listed chunks' claims; a chunk claiming more than it is the claims pass's ALLOC
        const bool claims = a.interBytes != 0;
        int st = (n > capN && !claims) ? PGN_ERR_UNSUPPORTED  // the large-chunk pass takes it
                                       : __builtin_amdgcn_readfirstlane(parse_frames<nf>(
                                             a.in, a.inOffsets[c], a.inSizes[c], d, &total,
                                             claims ? (size_t)a.interBytes : inter_cap(capN)));
        if (claims && st == PGN_ERR_UNSUPPORTED) st = PGN_ERR_ALLOC;
        if (Codec == kCodecC5 && st == PGN_OK && !claims) {  // C5: the staged path's per-stream bound
            uint64_t cs64[kStreams];
            bool over = false;
#pragma unroll
            for (int s = 0; s < nf; s++) {
                cs64[s] = d[s].cs;
                over = over || d[s].cs > capN;
            }
            if (over) st = __builtin_amdgcn_readfirstlane(over_claim_status(a.in, d, cs64, nf));
        }
        if (st == PGN_OK) {
#pragma unroll
            for (int s = 0; s < nf; s++) {  // in blob order (C5.hpp:588-667)
                if (st == PGN_OK) {
                    // VBZ's intermediate carries svb16's 16 padding bytes (signal_compression.cpp:112-118);
                    // the pgnano variants decompress into exactly the content size
                    const size_t cap = Codec == kCodecVbz ? (size_t)d[s].cs + kVbzPadding : (size_t)d[s].cs;
                    const long r = zstd_decompress_wave(a.in + d[s].src, d[s].len, inter + d[s].interOff, cap, S, P);
                    wave_sync();
                    if (r < 0) st = PGN_ERR_ZSTD_DECOMPRESS;
                    d[s].dres = (int32_t)r;
                }
            }
        }
        if (st == PGN_OK) {
            MergeOut mo{0, 0};
            uint64_t want = total;  // the pgnano svb16 decoders need no padding: consume everything
            // the merge for the call's output element: a wave-uniform branch between non-inlined calls
            if (a.outType == PGN_OUT_F32)
                mo = merge_chunk<Codec>(inter, total, d, out_chunk<float>(a, c), n, CalArg<float>{a.calOffset[c], a.calScale[c]});
            else if (a.outType == PGN_OUT_F16)
                mo = merge_chunk<Codec>(inter, total, d, out_chunk<_Float16>(a, c), n,
                                        CalArg<_Float16>{a.calOffset[c], a.calScale[c]});
            else mo = merge_chunk<Codec>(inter, total, d, out_chunk<int16_t>(a, c), n, CalArg<int16_t>{});
            if (mo.bad == 2) st = PGN_ERR_REMAINING;
            else if (mo.bad) st = PGN_ERR_CORRUPT;
            else if (mo.consumed != want) st = PGN_ERR_REMAINING;
        }
        P.mark(6);
        if (lane == 0) a.status[c] = st;
        wave_sync();
    }
    P.flush();
}

// ---------------------------------------------------------------------------------------------
// Synthetic reads (the checker's pgno_synth_read, oracle/pgn_oracle.c), 64 samples per thread
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t mix64(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ uint64_t synth_draw(uint64_t rb, uint64_t i, unsigned c)
{
    return mix64(rb + (8ull * i + c + 1ull) * 0x9E3779B97F4A7C15ull);
}
__device__ __forceinline__ int32_t gauss12(uint64_t a, uint64_t b, uint64_t c)
{
    int32_t s = 0;
#pragma unroll
    for (int k = 0; k < 4; k++)
        s += (int32_t)((a >> (16 * k)) & 0xFFFF) + (int32_t)((b >> (16 * k)) & 0xFFFF) + (int32_t)((c >> (16 * k)) & 0xFFFF);
    return s - 393216;
}

struct SynthArgs {
    size_t nreads;
    uint64_t seed, firstRead, readStride;
    int16_t* samples;
    const uint64_t* offsets;
    const uint32_t* counts;
    uint32_t pq;
    int32_t mean, lsd, nsd;
};

__global__ void synth_kernel(SynthArgs a, uint64_t totalTasks, const uint64_t* taskStart)
{
    // task = (read, 64-sample block); taskStart[r] = first task of read r (prefix sum)
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < totalTasks; t += (uint64_t)gridDim.x * blockDim.x) {
        // binary search the read of task t
        size_t lo = 0, hi = a.nreads;
        while (hi - lo > 1) {
            size_t mid = (lo + hi) / 2;
            if (taskStart[mid] <= t) lo = mid; else hi = mid;
        }
        const size_t r = lo;
        const uint32_t n = a.counts[r];
        const uint32_t i0 = (uint32_t)(t - taskStart[r]) * 64u;
        const uint64_t rid = a.firstRead + r * a.readStride;
        const uint64_t rb = mix64((a.seed << 32) ^ (rid * 0x9E3779B97F4A7C15ull) ^ 0x5851F42D4C957F2Dull);
        // level in force at i0: last switch point <= i0
        uint32_t j = i0;
        while (j > 0 && (uint32_t)(synth_draw(rb, j, 3) >> 48) >= a.pq) j--;
        int32_t level = a.mean + (int32_t)(((int64_t)gauss12(synth_draw(rb, j, 4), synth_draw(rb, j, 5), synth_draw(rb, j, 6)) * a.lsd) >> 16);
        int16_t* out = a.samples + a.offsets[r];
        const uint32_t iend = (i0 + 64 < n) ? i0 + 64 : n;
        for (uint32_t i = i0; i < iend; i++) {
            if (i > i0 && (uint32_t)(synth_draw(rb, i, 3) >> 48) < a.pq)
                level = a.mean + (int32_t)(((int64_t)gauss12(synth_draw(rb, i, 4), synth_draw(rb, i, 5), synth_draw(rb, i, 6)) * a.lsd) >> 16);
            int32_t g = gauss12(synth_draw(rb, i, 0), synth_draw(rb, i, 1), synth_draw(rb, i, 2));
            int32_t v = level + (int32_t)(((int64_t)g * a.nsd) >> 16);
            v = v < -32768 ? -32768 : (v > 32767 ? 32767 : v);
            out[i] = (int16_t)v;
        }
    }
}

__global__ void synth_tasks_kernel(const uint32_t* counts, size_t nreads, uint64_t* taskCount)
{
    for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r < nreads; r += (size_t)gridDim.x * blockDim.x)
        taskCount[r] = (counts[r] + 63u) / 64u;
}

// The chunks above kPassSamples of a batch (their indices, in any order), their count and the
// largest sample count among them, and the largest of all: hdr = {count, max large, -, max all},
// zeroed by the caller.
__global__ void large_scan_kernel(const uint32_t* counts, size_t n, uint32_t* list, uint32_t* hdr)
{
    uint32_t mx = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const uint32_t v = counts[i];
        mx = v > mx ? v : mx;
        if (v > kPassSamples) {
            list[atomicAdd(hdr, 1u)] = (uint32_t)i;
            atomicMax(hdr + 1, v);
        }
    }
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0 && mx) atomicMax(hdr + 3, mx);
}

}  // namespace pgn

// =============================================================================================
// Host side: contexts, scratch, launches (C ABI)
// =============================================================================================
using namespace pgn;

// ---- concurrent per-chunk host calls ------------------------------------------------------------
// The reference's readers call the plugin surface from several threads at once (the pod5 async
// signal loader's workers, async_signal_loader.cpp:174-208 -> signal_table_reader.cpp:135-139).  Calls
// on one context that arrive while another is on the device are combined into one small batch
// (flat combining): each call reserves room in the open arena (pinned host memory with a device
// mirror), copies its input there itself, and the first caller that finds the device free runs the
// whole arena as one batch -- one upload, the small-batch kernels for up to kPcMaxReqs chunks, one
// wait -- while later callers fill the other arena.  Each caller copies its own result out.
constexpr int kPcMaxReqs = 64;                    // the small-batch kernels' batch limit
constexpr size_t kPcHdr = 16384;                  // per-request arrays (<= 136 B per request)
constexpr size_t kPcInCap = (size_t)32 << 20;     // input bytes of one arena
constexpr size_t kPcOutCap = (size_t)32 << 20;    // output bytes of one arena
struct PcReq {
    int dir;             // 0 encode, 1 decode
    int codec;
    const void* in;      // samples (encode) or blob (decode), caller's host memory
    size_t inBytes;
    uint32_t n;          // samples
    void* dst;           // encode: blob destination; decode: samples
    size_t cap;          // encode: the destination's capacity
    size_t outBytes;     // room reserved for the result
    size_t inOff, outOff;
    int rc;
    uint64_t outSize;    // encode: blob size (or the required size on PGN_ERR_DST_TOO_SMALL)
    bool done;
};
struct PcArena {
    uint8_t* h = nullptr;     // pinned: [arrays | inputs | outputs]
    uint8_t* hDev = nullptr;  // the device's address of h (the kernels write results there)
    uint8_t* d = nullptr;     // device mirror of [arrays | inputs]
    size_t inUsed = 0, outUsed = 0;
    PcReq* reqs[kPcMaxReqs] = {};
    int nreq = 0, unstaged = 0, readers = 0;
    int state = 0;            // 0 idle / open, 1 on the device, 2 results being copied out
};

// A grow-only device allocation of a context: the pointer and its capacity in bytes.  It can only be
// constructed into its owner's list, which is what pgn_ctx_destroy frees; reserve() is what grows it.
struct DevMem {
    void* p = nullptr;
    size_t cap = 0;
    explicit DevMem(std::vector<DevMem*>& owner) { owner.push_back(this); }
    DevMem(const DevMem&) = delete;
    DevMem& operator=(const DevMem&) = delete;
};
template <class T>
struct DevBuf : DevMem {
    using DevMem::DevMem;
    operator T*() const { return static_cast<T*>(p); }
};

struct pgn_ctx {
    std::vector<DevMem*> bufs;  // every DevBuf below (declared first: they register as they are constructed)
    int device = 0;
    hipStream_t stream = nullptr;
    int numCUs = 0;
    size_t encSlotsMax = 0, decSlotsMax = 0;
    // pipeline per direction: the fused per-chunk kernel, or the three-kernel sub-batch pipeline
    // ("staged"); PGN_ENC_PIPELINE / PGN_DEC_PIPELINE = fused | staged override the measured defaults
    bool encStaged = false, decStaged = true;
    // small batches (the per-chunk plugin calls: one chunk) encode on the staged pipeline, whose five
    // stream waves run in parallel: 0.48 ms per 100,000-sample chunk against 0.75 ms for one fused
    // wave; at or below this many chunks (PGN_ENC_STAGED_BELOW; default the CU count) unless
    // PGN_ENC_PIPELINE forces a pipeline
    bool encForced = false;
    size_t encStagedBelow = 0;
    size_t encFusedSlotsMax = 0, decFusedSlotsMax = 0;
    size_t subBatch = 8192;  // chunks per pipeline pass (PGN_SUBBATCH, staged pipeline)
    // C5 decode batches of at least deferMin chunks defer their four-stream Huffman sections to
    // dec_huf_kernel (pgn_hufjob.h), in passes of up to deferG chunks: a lane-per-stream decoder
    // needs thousands of frames in flight (PGN_DEFER_MIN_CHUNKS / PGN_DEFER_G tune both; the output
    // is the same either way)
    size_t deferMin = 12288, deferG = 12500;
    // the last pass of a deferred call decodes its Huffman sections in place (dec_zstd_kernel's 16-
    // lanes-per-stream decoder): this many chunks (PGN_DEFER_TAIL_PLAIN; 0 = every pass deferred).
    // A deferred pass ends with one lane's ~16,000-symbol chain per M stream, which nothing overlaps
    // once the frame decode of the last pass is done (the decode's drain)
    size_t deferTailPlain = 0;
    bool hufPrioLast = false;  // PGN_HUF_PRIO_LAST=1: the last deferred pass's dec_huf waves at raised priority
    size_t hufWideLast = 0;    // PGN_HUF_WIDE_LAST: the last this many deferred passes decode their sections with dec_huf_wide_kernel
    bool lastDeferred = false;  // the last staged C5 decode deferred its Huffman sections (pgn_ctx_kernels)
    // encode: per-slot scratch of the zstd kernel, per-chunk streams/frames of one sub-batch
    DevBuf<uint8_t> encScratch{bufs};
    DevBuf<uint32_t> epochs{bufs};
    DevBuf<uint8_t> encChunks{bufs};  // per buffer: G * (kChunkStreamBytes + kChunkFrameBytes) + sizes + fsizes
    // decode
    DevBuf<uint8_t> decScratch{bufs};
    DevBuf<uint8_t> decChunks{bufs};  // per buffer: G * interStride + units (+ Huffman jobs)
    DecUnit* lastUnits = nullptr;  // decode records of the last pass (diagnostics)
    size_t lastG = 0;              // ... for this many chunks
    DevBuf<uint32_t> queues{bufs};  // a ring of work counters, zeroed when it wraps (one per sub-batch pass)
    size_t qNext = 0;              // next unused counter of the ring
    uint32_t* qCur = nullptr;      // the current call's counters
    DevBuf<uint64_t> lookback{bufs};  // dec_merge_lb_kernel's published words (kMergeWgMaxChunks chunks)
    uint64_t lbEpoch = 0;          // the tag of the last call that used them
    // host-call staging: a device buffer and its pinned host mirror (same layout), so a per-chunk
    // call is one upload, the launches and one download
    DevBuf<uint8_t> stage{bufs};
    uint8_t* hstage = nullptr;     // as large as stage (null: to be allocated)
    uint8_t* hstageDev = nullptr;  // the device's address of hstage (kernels write the call's outputs there)
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    // two-stream pipeline over sub-batches (launch_encode / launch_decode): the side stream runs the
    // split (encode) or the merge (decode) of one sub-batch while the caller's stream runs the zstd
    // kernel of the neighbouring one; two per-chunk buffers alternate between sub-batches
    hipStream_t side = nullptr;
    hipEvent_t evFork = nullptr, evJoin = nullptr, evStage[2] = {nullptr, nullptr}, evFree[2] = {nullptr, nullptr};
    // deferred-Huffman decode passes: the merges on a third stream, so the merge of pass p (VALU-bound)
    // can share the CUs with the Huffman sections of pass p + 1 (latency-bound)
    hipStream_t mergeS = nullptr;
    // decode passes: buffers in rotation (PGN_DEC_BUFS, 2..kMaxDecBufs) with their stage / sections /
    // free events, and the streams the deferred sections alternate over (PGN_HUF_STREAMS: 1 or 2 with
    // the merges on mergeS; 3 = sections and merge of pass p both on side stream p % 3 of side, side2,
    // mergeS).  Measured (tools/gpu_env_sweep.sh, 100,000 chunks): 2 buffers / 1 stream / passes of
    // 20,000: decode 23.1 ms; 4 / 2 / 12,500: 22.7 ms; 4 / 3 / 12,500: 22.3-22.6 ms against 22.8-23.1
    // in interleaved A/B (profiles/r05_decode_pipeline_sweep.log)
    size_t decBufs = 4, hufStreams = 3;
    hipStream_t side2 = nullptr;
    hipEvent_t evDStage[kMaxDecBufs] = {}, evDHuf[kMaxDecBufs] = {}, evDFree[kMaxDecBufs] = {};
    DevBuf<uint64_t> prof{bufs};  // kProfWords: phase cycles and counters (encode, decode, dec_huf) when PGN_PHASE_PROFILE=1
    bool encTimed = false, decTimed = false;
    // Stream ordering of the context's shared state (work counters, slot scratch, per-chunk buffers):
    // every launch sequence records evLast on its stream at the end, and the next one, on whatever
    // stream, waits for it before touching that state (CallScope).  Calls on one context therefore run
    // in call order on the device even when callers pass different streams.
    hipEvent_t evLast = nullptr;
    bool haveLast = false;
    // Large-chunk pass (chunks above kPassSamples, launch_large): the chunk list, its header
    // {count, largest} on the device and in pinned memory, read on a stream of its own while the
    // batched pass runs; slot scratch spaced for the largest chunk, and its own table epochs and
    // work counter.
    DevBuf<uint32_t> largeList{bufs};
    DevBuf<uint32_t> claimList{bufs};  // the claims pass's chunks (claim_scan_kernel, or from the host)
    DevBuf<uint32_t> largeHdr{bufs};   // [0..1] header, [2] the large pass's work counter, [3] largest chunk,
                                       // [4..5] the claims pass's count and largest sum (KiB)
    uint32_t* largeHdrHost = nullptr;
    hipStream_t scanStream = nullptr;
    hipEvent_t evScanFork = nullptr, evScan = nullptr;
    // the encode and the decode of the large pass keep separate slot scratch: the encoder's hash
    // tables persist across calls (epoch tags), so a decode must never write over them
    DevBuf<uint8_t> largeScratch{bufs};
    DevBuf<uint32_t> largeEpochs{bufs};
    DevBuf<uint8_t> largeDecScratch{bufs};
    // pgn_decompress_reads_device_norm: the reads expanded to chunks (per chunk: output offset and
    // read; per read: n and, when the caller passes no d_stats, the statistics)
    DevBuf<uint64_t> normChunkOut{bufs};
    DevBuf<uint32_t> normChunkRead{bufs};
    DevBuf<uint64_t> normReadN{bufs};
    DevBuf<pgn_read_stats> normStats{bufs};
    // pgn_decompress_reads_device_pa: the reads' calibration expanded to chunks (the chunks' output
    // offsets share normChunkOut)
    DevBuf<float> paChunkOffset{bufs};
    DevBuf<float> paChunkScale{bufs};
    // pgn_segment_reads_device: per read the head count, the trimmed offset and count, the head's and the
    // trimmed read's statistics; then the segment total (one block, carved up by ensure_segment)
    DevBuf<uint8_t> segWork{bufs};
    // pgn_stitch_plan_device: the frame totals of the count kernel's workgroups, then their sum
    DevBuf<uint64_t> stitchSums{bufs};
    // pgn_ctc_decode_device / pgn_collapse_codes_device: the tiles' base counts, the reads at the tile edges
    // and the spans' sums with the total, in one block; the code bytes of a decode whose caller passes no array
    DevBuf<uint64_t> ctcSums{bufs};
    DevBuf<uint8_t> ctcCodes{bufs};
    // pgn_crf_viterbi_rows_device: the backpointers of one group of rows (crf::row_scratch_bytes each), at most
    // crfCap bytes (pgn_ctx_set_crf_scratch); PGN_CRF_TRACEBACK=split moves the traceback into a kernel of its own,
    // =none leaves it out (measurements only: no codes are written).  pgn_crf_posterior_rows_device keeps its forward
    // vectors (crf::post_row_scratch_bytes per row) in the same memory under the same cap: a call sequence of the
    // context follows the one before it, so the two never hold it at once.
    DevBuf<uint32_t> crfBp{bufs};
    // pgn_read_qual_device: the reads' error sums when the caller passes no array.  pgn_fastq_records_device: the
    // totals of the length kernel's workgroups, their sum and the end of the written records; pgn_bam_records_device:
    // the same totals and their sum.  PGN_BAM_CRC=split moves the BGZF checksum into a kernel of its own
    // (measurements only: the bytes are the same)
    DevBuf<uint64_t> fqWork{bufs};
    // pgn_bgzf_deflate_device: a deflate::BlockPlan per 65,280 stream bytes, written by the plan kernel of every call.
    // PGN_BGZF_KERNELS=plan | scan ends the call behind that kernel (measurements only: no block is written)
    DevBuf<deflate::BlockPlan> bgzfPlans{bufs};
    // pgn_find_patterns_device: the per-side index of the patterns (the head, tail and not-searched lists and their
    // counts), built by the first kernel of every call.  pgn_trim_reads_device keeps its workgroups' totals in fqWork
    DevBuf<uint32_t> demuxIndex{bufs};
    // PGN_DEMUX_FIND=plain keeps the index in pattern order and both words of the column in every wave
    // (measurements only: the outputs are the same)
    bool demuxByLength = true;
    int bgzfKernels = 3;
    bool bamCrcSplit = false;
    uint64_t crfCap = crf::kDefaultScratch;
    int crfTrace = 0;  // 0 in the row's workgroup, 1 split, 2 none
    // the selection of long reads in parts (pgn_select.h, pgn_ctx_set_select_split): the head, the slots'
    // first work items and the slots in one block sized by max_split_reads; the per-read counts the one-workgroup kernel reads.
    // Defaults measured by tools/select_split_timing.py (profiles/select_split_timing.log)
    pgn_select_split split = {196608u, 32768u, 1024u, 0u};
    DevBuf<uint8_t> splitWork{bufs};
    DevBuf<uint64_t> splitWholeCounts{bufs};
    bool splitCounted = false;  // the last selection ran the plan kernel (pgn_select_split_counts)
    // an object of another translation unit (the POD5 loader's staging, pgn_internal.h)
    void* ext = nullptr;
    void (*extDestroy)(void*) = nullptr;
    std::mutex mu;
    // combined per-chunk host calls (PcArena): pcOpen = the arena new calls join (-1: none idle)
    std::mutex pcMu;
    std::condition_variable pcCv;
    PcArena pcA[2];
    int pcOpen = 0;
    bool pcBusy = false;
    int pcReady = 0;  // 0 not yet allocated, 1 ready, -1 allocation failed (calls run one by one)
};

static thread_local char g_err[512];

static int hip_fail(hipError_t e, const char* what)
{
    snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
    return PGN_ERR_HIP;
}
#define HIPCHK(x)                                   \
    do {                                            \
        hipError_t e_ = (x);                        \
        if (e_ != hipSuccess) return hip_fail(e_, #x); \
    } while (0)

extern "C" {

const char* pgn_status_string(int s)
{
    switch (s) {
    case PGN_OK: return "OK";
    case PGN_ERR_DST_TOO_SMALL: return "Not enough space in destination buffer";
    case PGN_ERR_NOT_ZSTD: return "Input data not compressed by zstd";
    case PGN_ERR_ZSTD_DECOMPRESS: return "Input data failed to decompress using zstd";
    case PGN_ERR_REMAINING: return "Remaining data at end of signal buffer";
    case PGN_ERR_ZSTD_COMPRESS: return "Failed to compress data";
    case PGN_ERR_CORRUPT: return "Corrupt compressed signal (stream read past its end)";
    case PGN_ERR_ALLOC: return "Out of memory: the frames' content sizes sum to more than 2^40 bytes";
    case PGN_ERR_UNSUPPORTED: return "Chunk larger than PGN_MAX_CHUNK_SAMPLES, or frames expanding beyond the decoder's buffer";
    case PGN_ERR_INVALID_ARG: return "Invalid argument";
    case PGN_ERR_HIP: return "HIP runtime error";
    case PGN_ERR_NO_DEVICE: return "No HIP device";
    case PGN_ERR_IO: return "File I/O failure";
    default: return "Unknown status";
    }
}

const char* pgn_last_error(void) { return g_err; }

size_t pgn_compressed_signal_max_size(size_t n)
{
    size_t s = n * 2 + 10 + 16;
    return s > 1024 ? s : 1024;
}

// An empty buffer's first allocation (the fixed-size ones; the others grow through reserve()).
static hipError_t dev_alloc(DevMem& b, size_t bytes)
{
    const hipError_t e = hipMalloc(&b.p, bytes);
    if (e == hipSuccess) b.cap = bytes;
    return e;
}

// The settings, streams, events and fixed-size buffers of a new context (c->device is set and current).
// On an error pgn_ctx_create destroys what exists by then.
static int ctx_init(pgn_ctx* c)
{
    const int device = c->device;
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    c->numCUs = prop.multiProcessorCount;
    int encPerCU = 0, decPerCU = 0;
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&encPerCU, enc_zstd_kernel, 64, 0));
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&decPerCU, dec_zstd_kernel, 64, 0));
    int fe = 0, fd = 0;
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&fe, enc_chunk_kernel<kCodecC5>, 64, 0));
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&fd, dec_chunk_kernel<kCodecC5>, 64, 0));
    if (fe < 1) fe = 1;
    if (fd < 1) fd = 1;
    if (const char* v = getenv("PGN_ENC_WG_PER_CU")) { const int x = atoi(v); if (x > 0 && x < fe) fe = x; }
    if (const char* v = getenv("PGN_DEC_WG_PER_CU")) { const int x = atoi(v); if (x > 0 && x < fd) fd = x; }
    c->encFusedSlotsMax = (size_t)c->numCUs * (size_t)(fe > 32 ? 32 : fe);
    c->decFusedSlotsMax = (size_t)c->numCUs * (size_t)(fd > 32 ? 32 : fd);
    if (encPerCU < 1) encPerCU = 1;
    if (decPerCU < 1) decPerCU = 1;
    // resident zstd workgroups per CU (tuning knobs PGN_ENC_WG_PER_CU / PGN_DEC_WG_PER_CU: fewer
    // leave room for the side stream's split / merge kernels)
    if (const char* v = getenv("PGN_ENC_WG_PER_CU")) { const int x = atoi(v); if (x > 0 && x < encPerCU) encPerCU = x; }
    if (const char* v = getenv("PGN_DEC_WG_PER_CU")) { const int x = atoi(v); if (x > 0 && x < decPerCU) decPerCU = x; }
    c->encSlotsMax = (size_t)c->numCUs * (size_t)(encPerCU > 32 ? 32 : encPerCU);
    c->decSlotsMax = (size_t)c->numCUs * (size_t)(decPerCU > 32 ? 32 : decPerCU);
    c->encStagedBelow = (size_t)c->numCUs;
    if (const char* v = getenv("PGN_ENC_STAGED_BELOW")) c->encStagedBelow = (size_t)atol(v);
    if (const char* pp = getenv("PGN_ENC_PIPELINE")) {
        c->encStaged = strcmp(pp, "staged") == 0;
        c->encForced = true;
    }
    if (const char* pp = getenv("PGN_DEC_PIPELINE")) c->decStaged = strcmp(pp, "staged") == 0;
    if (const char* sb = getenv("PGN_SUBBATCH")) {
        long v = atol(sb);
        if (v > 0) c->subBatch = (size_t)v;
    }
    if (const char* v = getenv("PGN_DEFER_MIN_CHUNKS")) { const long x = atol(v); if (x > 0) c->deferMin = (size_t)x; }
    if (const char* v = getenv("PGN_DEFER_G")) { const long x = atol(v); if (x > 0) c->deferG = (size_t)x; }
    if (const char* v = getenv("PGN_HUF_WIDE_LAST")) { const long x = atol(v); if (x >= 0) c->hufWideLast = (size_t)x; }
    if (const char* v = getenv("PGN_HUF_PRIO_LAST")) c->hufPrioLast = v[0] == '1';
    if (const char* v = getenv("PGN_CRF_TRACEBACK")) c->crfTrace = strcmp(v, "split") == 0 ? 1 : strcmp(v, "none") == 0 ? 2 : 0;
    if (const char* v = getenv("PGN_BAM_CRC")) c->bamCrcSplit = strcmp(v, "split") == 0;
    if (const char* v = getenv("PGN_DEMUX_FIND")) c->demuxByLength = strcmp(v, "plain") != 0;
    if (const char* v = getenv("PGN_BGZF_KERNELS")) c->bgzfKernels = strcmp(v, "plan") == 0 ? 1 : strcmp(v, "scan") == 0 ? 2 : 3;
    if (const char* v = getenv("PGN_DEFER_TAIL_PLAIN")) { const long x = atol(v); if (x >= 0) c->deferTailPlain = (size_t)x; }
    HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    const char* pe = getenv("PGN_PHASE_PROFILE");
    if (pe && pe[0] == '1') {
        // [encode phases][decode phases][encode counters][decode counters]
        HIPCHK(dev_alloc(c->prof, kProfWords * sizeof(uint64_t)));
        HIPCHK(hipMemset(c->prof, 0, kProfWords * sizeof(uint64_t)));
        HIPCHK(hipDeviceSynchronize());
    }
    for (int i = 0; i < 4; i++) HIPCHK(hipEventCreate(&c->ev[i]));
    HIPCHK(hipEventCreateWithFlags(&c->evLast, hipEventDisableTiming));
    HIPCHK(hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&c->mergeS, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&c->side2, hipStreamNonBlocking));
    for (int i = 0; i < kMaxDecBufs; i++) {
        HIPCHK(hipEventCreateWithFlags(&c->evDStage[i], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&c->evDHuf[i], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&c->evDFree[i], hipEventDisableTiming));
    }
    if (const char* v = getenv("PGN_DEC_BUFS")) {
        const long x = atol(v);
        if (x >= 2 && x <= kMaxDecBufs) c->decBufs = (size_t)x;
    }
    if (const char* v = getenv("PGN_HUF_STREAMS")) {
        const long x = atol(v);
        c->hufStreams = x >= 1 && x <= 3 ? (size_t)x : c->hufStreams;
    }
    HIPCHK(hipStreamCreateWithFlags(&c->scanStream, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&c->evScanFork, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->evScan, hipEventDisableTiming));
    HIPCHK(dev_alloc(c->largeHdr, 8 * sizeof(uint32_t)));
    HIPCHK(hipHostMalloc((void**)&c->largeHdrHost, 8 * sizeof(uint32_t), hipHostMallocDefault));
    HIPCHK(hipEventCreateWithFlags(&c->evFork, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->evJoin, hipEventDisableTiming));
    for (int i = 0; i < 2; i++) {
        HIPCHK(hipEventCreateWithFlags(&c->evStage[i], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&c->evFree[i], hipEventDisableTiming));
    }
    // the predefined sequence FSE tables of the decoder (one wave, once per context)
    hipLaunchKernelGGL(seq_default_tables_kernel, dim3(1), dim3(64), 0, c->stream);
    HIPCHK(hipGetLastError());
    // and the encoder's
    hipLaunchKernelGGL(seq_default_ctables_kernel, dim3(1), dim3(64), 0, c->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    return PGN_OK;
}

int pgn_ctx_create(int device, pgn_ctx** out)
{
    if (!out) return PGN_ERR_INVALID_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return PGN_ERR_NO_DEVICE;
    if (device < 0 || device >= ndev) return PGN_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(device));
    pgn_ctx* c = new pgn_ctx();
    c->device = device;
    const int rc = ctx_init(c);
    if (rc != PGN_OK) {  // whatever step failed: nothing of the context is left, *out is untouched
        (void)pgn_ctx_destroy(c);
        return rc;
    }
    *out = c;
    return PGN_OK;
}

// Also the teardown of a context whose creation failed part-way: every member may still be null.
int pgn_ctx_destroy(pgn_ctx* c)
{
    if (!c) return PGN_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->haveLast) (void)hipEventSynchronize(c->evLast);
    if (c->ext && c->extDestroy) c->extDestroy(c->ext);
    if (c->scanStream) (void)hipStreamSynchronize(c->scanStream);
    for (DevMem* b : c->bufs) (void)hipFree(b->p);
    if (c->hstage) (void)hipHostFree(c->hstage);
    for (PcArena& A : c->pcA) {
        if (A.h) (void)hipHostFree(A.h);
        (void)hipFree(A.d);
    }
    if (c->largeHdrHost) (void)hipHostFree(c->largeHdrHost);
    for (hipEvent_t e : {c->evScanFork, c->evScan})
        if (e) (void)hipEventDestroy(e);
    if (c->scanStream) (void)hipStreamDestroy(c->scanStream);
    for (int i = 0; i < 4; i++) if (c->ev[i]) (void)hipEventDestroy(c->ev[i]);
    if (c->side) (void)hipStreamSynchronize(c->side);
    if (c->mergeS) (void)hipStreamSynchronize(c->mergeS);
    if (c->side2) (void)hipStreamSynchronize(c->side2);
    for (int i = 0; i < kMaxDecBufs; i++)
        for (hipEvent_t e : {c->evDStage[i], c->evDHuf[i], c->evDFree[i]})
            if (e) (void)hipEventDestroy(e);
    if (c->evLast) (void)hipEventSynchronize(c->evLast);
    for (hipEvent_t e : {c->evFork, c->evJoin, c->evStage[0], c->evStage[1], c->evFree[0], c->evFree[1], c->evLast})
        if (e) (void)hipEventDestroy(e);
    if (c->side) (void)hipStreamDestroy(c->side);
    if (c->mergeS) (void)hipStreamDestroy(c->mergeS);
    if (c->side2) (void)hipStreamDestroy(c->side2);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return PGN_OK;
}

void* pgn_ctx_stream(pgn_ctx* c) { return c ? (void*)c->stream : nullptr; }

// The last launch sequence on any stream (evLast) has finished with the context's buffers.
static void wait_last_host(pgn_ctx* c)
{
    if (c->haveLast) (void)hipEventSynchronize(c->evLast);
    (void)hipStreamSynchronize(c->stream);
}

// The one place a context's scratch grows.  `group` lists buffers that are sized together with the bytes
// each must hold: when any of them is too small, all are freed and allocated again at exactly the bytes
// asked for (no geometric growth).  Before anything is freed the host waits for the last launch sequence,
// and, by `flags`, for the whole device, for the scan stream or for `also`, the caller's stream.  kZeroFill
// clears the new memory on the context's stream and waits for that (the stream is non-blocking, so a
// launch on any other stream would not).  A buffer that could not be allocated is left empty.
enum : unsigned { kSyncDevice = 1, kSyncScan = 2, kZeroFill = 4 };
struct Want {
    DevMem& buf;
    size_t bytes;
};
static int reserve(pgn_ctx* c, std::initializer_list<Want> group, unsigned flags = 0, hipStream_t also = nullptr)
{
    bool fits = true;
    for (const Want& w : group) fits = fits && w.bytes <= w.buf.cap;
    if (fits) return PGN_OK;
    wait_last_host(c);
    if (flags & kSyncDevice) (void)hipDeviceSynchronize();
    if (flags & kSyncScan) (void)hipStreamSynchronize(c->scanStream);
    if (also) (void)hipStreamSynchronize(also);
    for (const Want& w : group) {
        (void)hipFree(w.buf.p);
        w.buf.p = nullptr;
        w.buf.cap = 0;
    }
    for (const Want& w : group) HIPCHK(dev_alloc(w.buf, w.bytes));
    if (flags & kZeroFill) {
        for (const Want& w : group) HIPCHK(hipMemsetAsync(w.buf.p, 0, w.bytes, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return PGN_OK;
}

// One call's launch sequence on a context: it takes the context's lock (unless the caller holds it: the
// per-chunk host calls, and a decode inside a read call), makes the device current, picks the stream and
// orders it behind the previous sequence (evLast, whatever stream that ran on).  However the scope is
// left, by an error too, it records evLast behind what the call queued, so the next call on another
// stream never overtakes kernels that still use the context's scratch.
struct CallScope {
    enum Lock { kLock, kLocked };
    pgn_ctx* const c;
    std::unique_lock<std::mutex> lock;
    hipStream_t s = nullptr;
    int rc = PGN_OK;  // not PGN_OK: the scope did not open, and the call returns this
    CallScope(pgn_ctx* ctx, void* stream, Lock l = kLock) : c(ctx)
    {
        if (l == kLock) lock = std::unique_lock<std::mutex>(c->mu);
        rc = open(stream);
    }
    ~CallScope()
    {
        if (rc == PGN_OK && hipEventRecord(c->evLast, s) == hipSuccess) c->haveLast = true;
    }
    CallScope(const CallScope&) = delete;
    CallScope& operator=(const CallScope&) = delete;

private:
    int open(void* stream)
    {
        HIPCHK(hipSetDevice(c->device));
        s = stream ? (hipStream_t)stream : c->stream;
        if (c->haveLast) HIPCHK(hipStreamWaitEvent(s, c->evLast, 0));
        return PGN_OK;
    }
};

static int ensure_enc(pgn_ctx* c, size_t slots, size_t G)
{
    // tag 0 never matches: a zeroed table is an empty table for every epoch >= 1
    int rc = reserve(c, {{c->encScratch, enc_slot_bytes() * slots}, {c->epochs, 4 * slots}}, kZeroFill);
    if (rc) return rc;
    // G = chunk capacity over all buffers
    return reserve(c, {{c->encChunks, G * (kChunkStreamBytes + kChunkFrameBytes + 2 * 4 * kStreams)}}, kSyncDevice);
}

static int ensure_dec(pgn_ctx* c, size_t slots, size_t bytes)
{
    int rc = reserve(c, {{c->decScratch, dec_slot_bytes() * slots}});
    if (rc) return rc;
    return reserve(c, {{c->decChunks, bytes}}, kSyncDevice);  // the per-chunk buffers of all passes in flight
}

// The look-back words of the small-batch range split / merge and this call's tag.  Launch sequences
// on a context are ordered (evLast), so one array serves every call; it is cleared when the 16-bit
// tags wrap.
static int take_lookback(pgn_ctx* c, hipStream_t s, uint64_t*& words, uint64_t& epoch)
{
    const size_t bytes = sizeof(uint64_t) * 3 * 32 * 64;  // 3 words x 32 ranges x 64 chunks
    if (!c->lookback) {
        HIPCHK(dev_alloc(c->lookback, bytes));
        HIPCHK(hipMemsetAsync(c->lookback, 0, bytes, s));
    }
    if (++c->lbEpoch > 0xFFFFu) {
        HIPCHK(hipMemsetAsync(c->lookback, 0, bytes, s));
        c->lbEpoch = 1;
    }
    words = c->lookback;
    epoch = c->lbEpoch;
    return PGN_OK;
}

// n fresh zeroed work counters for this call (c->qCur).  The counters come from a ring that is zeroed
// only when it wraps: a per-call memset was a fill kernel plus a launch gap in front of every
// per-chunk call.  Launch sequences on a context are ordered (evLast), so the wrap's memset runs
// after every earlier user of the ring.
static int ensure_queues(pgn_ctx* c, size_t n, hipStream_t s)
{
    constexpr size_t kRing = 1 << 14;
    const size_t had = c->queues.cap;
    const int rc = reserve(c, {{c->queues, 4 * (n < kRing ? kRing : n)}}, 0, s);
    if (rc) return rc;
    if (c->queues.cap != had || c->qNext + n > c->queues.cap / 4) {  // a new ring, or the ring wraps
        HIPCHK(hipMemsetAsync(c->queues, 0, c->queues.cap, s));
        c->qNext = 0;
    }
    c->qCur = c->queues + c->qNext;
    c->qNext += n;
    return PGN_OK;
}

// A decode call's destination: the int16 samples (what an int16_t* converts to), or the calibrated
// output of pgn_decompress_batch_device_pa (element type and per-chunk calibration).
struct DecOut {
    void* p;
    int type;
    const float *calOffset, *calScale;
    DecOut(int16_t* samples) : p(samples), type(PGN_OUT_INT16), calOffset(nullptr), calScale(nullptr) {}
    DecOut(void* out, int t, const float* off, const float* scale) : p(out), type(t), calOffset(off), calScale(scale) {}
};

// The caller's device arrays of an encode / a decode call, one entry per chunk, as the C entry points
// receive them.  Everything below the entry points passes them on as one.
struct EncIO {
    const int16_t* samples;
    const uint64_t* sampleOffsets;
    const uint32_t* sampleCounts;
    uint8_t* out;
    const uint64_t* outOffsets;
    const uint64_t* outCaps;
    uint64_t* outSizes;
    int32_t* status;
    uint64_t* stats;
};
struct DecIO {
    const uint8_t* in;
    const uint64_t* inOffsets;
    const uint64_t* inSizes;
    DecOut out;
    const uint64_t* sampleOffsets;
    const uint32_t* sampleCounts;
    int32_t* status;
};

// The launch arguments every encode / decode path starts from: what comes from the caller and what is the
// same for the whole context (taken after the path's ensure_*, which may move the context's buffers).  A
// path then sets only what it differs in: slot scratch, queue, capN, the list, the passes' geometry.
static EncArgs enc_args(const pgn_ctx* c, const EncIO& io, size_t nchunks)
{
    EncArgs a{};
    a.nchunks = nchunks;
    a.samples = io.samples;
    a.sampleOffsets = io.sampleOffsets;
    a.sampleCounts = io.sampleCounts;
    a.out = io.out;
    a.outOffsets = io.outOffsets;
    a.outCaps = io.outCaps;
    a.outSizes = io.outSizes;
    a.status = io.status;
    a.stats = io.stats;
    a.epochs = c->epochs;
    a.prof = c->prof;
    return a;
}
static DecArgs dec_args(const pgn_ctx* c, const DecIO& io, size_t nchunks)
{
    DecArgs a{};
    a.nchunks = nchunks;
    a.in = io.in;
    a.inOffsets = io.inOffsets;
    a.inSizes = io.inSizes;
    a.samples = (int16_t*)io.out.p;
    a.outBytes = (uint8_t*)io.out.p;
    a.outType = io.out.type;
    a.calOffset = io.out.calOffset;
    a.calScale = io.out.calScale;
    a.sampleOffsets = io.sampleOffsets;
    a.sampleCounts = io.sampleCounts;
    a.status = io.status;
    a.prof = c->prof ? c->prof + kPhases : nullptr;
    return a;
}

static int launch_enc_chunks(int codec, const EncArgs& a, size_t slots, hipStream_t s);
static int launch_dec_chunks(int codec, const DecArgs& a, size_t slots, hipStream_t s);

static int launch_encode_fused(pgn_ctx* c, int codec, size_t nchunks, const EncIO& io, hipStream_t s)
{
    const size_t slots = nchunks < c->encFusedSlotsMax ? nchunks : c->encFusedSlotsMax;
    int rc = ensure_enc(c, slots, 0);
    if (rc) return rc;
    HIPCHK(hipEventRecord(c->ev[0], s));
    rc = ensure_queues(c, 1, s);
    if (rc) return rc;
    EncArgs a = enc_args(c, io, nchunks);
    a.slotScratch = c->encScratch;
    a.slotBytes = enc_slot_bytes();
    a.queue = c->qCur;
    a.capN = kPassSamples;
    return launch_enc_chunks(codec, a, slots, s);
}

static int launch_enc_chunks(int codec, const EncArgs& a, size_t slots, hipStream_t s)
{
    switch (codec) {
    case kCodecC5: hipLaunchKernelGGL(enc_chunk_kernel<kCodecC5>, dim3((unsigned)slots), dim3(64), 0, s, a); break;
    case kCodecVbz: hipLaunchKernelGGL(enc_chunk_kernel<kCodecVbz>, dim3((unsigned)slots), dim3(64), 0, s, a); break;
    case kCodecC4: hipLaunchKernelGGL(enc_chunk_kernel<kCodecC4>, dim3((unsigned)slots), dim3(64), 0, s, a); break;
    case kCodecC1: hipLaunchKernelGGL(enc_chunk_kernel<kCodecC1>, dim3((unsigned)slots), dim3(64), 0, s, a); break;
    case kCodecC2: hipLaunchKernelGGL(enc_chunk_kernel<kCodecC2>, dim3((unsigned)slots), dim3(64), 0, s, a); break;
    case kCodecC3: hipLaunchKernelGGL(enc_chunk_kernel<kCodecC3>, dim3((unsigned)slots), dim3(64), 0, s, a); break;
    case kCodecVbz0: hipLaunchKernelGGL(enc_chunk_kernel<kCodecVbz0>, dim3((unsigned)slots), dim3(64), 0, s, a); break;
    default: return PGN_ERR_INVALID_ARG;
    }
    HIPCHK(hipGetLastError());
    return PGN_OK;
}

static int launch_decode_fused(pgn_ctx* c, int codec, size_t nchunks, const DecIO& io, hipStream_t s)
{
    const size_t slots = nchunks < c->decFusedSlotsMax ? nchunks : c->decFusedSlotsMax;
    int rc = ensure_dec(c, slots, 0);
    if (rc) return rc;
    HIPCHK(hipEventRecord(c->ev[2], s));
    rc = ensure_queues(c, 1, s);
    if (rc) return rc;
    DecArgs a = dec_args(c, io, nchunks);
    a.slotScratch = c->decScratch;
    a.slotBytes = dec_slot_bytes();
    a.queue = c->qCur;
    a.capN = kPassSamples;
    c->lastUnits = nullptr;
    return launch_dec_chunks(codec, a, slots, s);
}

static int launch_dec_chunks(int codec, const DecArgs& a, size_t slots, hipStream_t s)
{
    switch (codec) {
    case kCodecC5: hipLaunchKernelGGL(dec_chunk_kernel<kCodecC5>, dim3((unsigned)slots), dim3(64), 0, s, a); break;
    case kCodecVbz: hipLaunchKernelGGL(dec_chunk_kernel<kCodecVbz>, dim3((unsigned)slots), dim3(64), 0, s, a); break;
    case kCodecC4: hipLaunchKernelGGL(dec_chunk_kernel<kCodecC4>, dim3((unsigned)slots), dim3(64), 0, s, a); break;
    case kCodecC1: hipLaunchKernelGGL(dec_chunk_kernel<kCodecC1>, dim3((unsigned)slots), dim3(64), 0, s, a); break;
    case kCodecC2: hipLaunchKernelGGL(dec_chunk_kernel<kCodecC2>, dim3((unsigned)slots), dim3(64), 0, s, a); break;
    case kCodecC3: hipLaunchKernelGGL(dec_chunk_kernel<kCodecC3>, dim3((unsigned)slots), dim3(64), 0, s, a); break;
    case kCodecVbz0: hipLaunchKernelGGL(dec_chunk_kernel<kCodecVbz0>, dim3((unsigned)slots), dim3(64), 0, s, a); break;
    default: return PGN_ERR_INVALID_ARG;
    }
    HIPCHK(hipGetLastError());
    return PGN_OK;
}

static int launch_encode_impl(pgn_ctx* c, int codec, size_t nchunks, const EncIO& io, hipStream_t s)
{
    const bool staged = c->encStaged || (!c->encForced && nchunks <= c->encStagedBelow);
    if (!staged || (codec != kCodecC5 && codec != kCodecVbz))  // the other variants are fused only
        return launch_encode_fused(c, codec, nchunks, io, s);
    const size_t G = nchunks < c->subBatch ? nchunks : c->subBatch;
    const size_t passes = (nchunks + G - 1) / G;
    const uint32_t nu = codec == kCodecVbz ? 1u : (uint32_t)kStreams;
    const size_t slots = nu * G < c->encSlotsMax ? nu * G : c->encSlotsMax;
    const size_t nbuf = passes > 1 ? 2 : 1;
    int rc = ensure_enc(c, slots, nbuf * G);
    if (rc) return rc;
    HIPCHK(hipEventRecord(c->ev[0], s));
    rc = ensure_queues(c, passes, s);
    if (rc) return rc;
    // the split of pass p + 1 runs on the side stream beside pass p's zstd kernel; a single pass
    // stays on the caller's stream (no fork, no cross-stream events)
    const hipStream_t sideS = passes > 1 ? c->side : s;
    if (passes > 1) {
        HIPCHK(hipEventRecord(c->evFork, s));
        HIPCHK(hipStreamWaitEvent(c->side, c->evFork, 0));
    }
    const size_t bufBytes = G * (kChunkStreamBytes + kChunkFrameBytes + 2 * 4 * kStreams);
    EncArgs a = enc_args(c, io, nchunks);
    a.slotScratch = c->encScratch;
    a.slotBytes = enc_slot_bytes();
    a.G = G;
    a.nu = nu;
    a.capN = kPassSamples;
    if (passes == 1 && G <= kSplitWgMaxChunks && codec != kCodecVbz) {  // the look-back range split (one epoch per pass)
        rc = take_lookback(c, s, a.lookback, a.epoch);
        if (rc) return rc;
    }
    // pass p: split on the side stream into buffer p % 2; zstd + assemble on the caller's stream.
    // The split of pass p+1 overlaps the zstd kernel of pass p; a buffer is split into again only
    // after the assemble kernel of the pass before last has read it.
    for (size_t p = 0; p < passes; p++) {
        const int b = (int)(p & 1);
        uint8_t* buf = c->encChunks + (size_t)b * bufBytes;
        a.streams = buf;
        a.frames = buf + G * kChunkStreamBytes;
        a.sizes = (uint32_t*)(a.frames + G * kChunkFrameBytes);
        a.fsizes = a.sizes + G * kStreams;
        a.base = p * G;
        a.queue = c->qCur + p;
        if (p >= 2) HIPCHK(hipStreamWaitEvent(c->side, c->evFree[b], 0));
        if (codec == kCodecVbz) hipLaunchKernelGGL(vbz_split_kernel, dim3((unsigned)G), dim3(64), 0, sideS, a);
        else if (a.lookback)  // few chunks: kSplitRanges single-wave workgroups per chunk
            hipLaunchKernelGGL(enc_split_lb_kernel, dim3((unsigned)(G * kSplitRanges)), dim3(64), 0, sideS, a);
        else hipLaunchKernelGGL(enc_split_kernel, dim3((unsigned)G), dim3(64), 0, sideS, a);
        if (passes > 1) {
            HIPCHK(hipEventRecord(c->evStage[b], c->side));
            HIPCHK(hipStreamWaitEvent(s, c->evStage[b], 0));
        }
        const bool coop = G <= kSplitWgMaxChunks && (size_t)nu * G <= slots;
        if (coop)  // few chunks: a workgroup per stream (C5: the frames place themselves, enc_place_frame)
            hipLaunchKernelGGL(enc_zstd_coop_kernel, dim3((unsigned)(nu * G)), dim3(64 * kCoopEncWaves), 0, s, a);
        else hipLaunchKernelGGL(enc_zstd_kernel, dim3((unsigned)slots), dim3(64), 0, s, a);
        if (codec == kCodecVbz) hipLaunchKernelGGL(vbz_assemble_kernel, dim3((unsigned)G), dim3(64), 0, s, a);
        else if (!(coop && a.lookback)) hipLaunchKernelGGL(enc_assemble_kernel, dim3((unsigned)G), dim3(64), 0, s, a);
        if (passes > 1) HIPCHK(hipEventRecord(c->evFree[b], s));
    }
    HIPCHK(hipGetLastError());
    return PGN_OK;
}

// The staged passes' merge for the call's output element (a.outType).
#define PGN_LAUNCH_MERGE_PA(T)                                                                                           \
    do {                                                                                                                 \
        if (codec == kCodecVbz) hipLaunchKernelGGL(vbz_merge_pa_kernel<T>, dim3((unsigned)G), dim3(64), 0, ms, a);       \
        else if (a.lookback)                                                                                             \
            hipLaunchKernelGGL(dec_merge_lb_pa_kernel<T>, dim3((unsigned)(G * kMergeRanges)), dim3(64), 0, ms, a);       \
        else hipLaunchKernelGGL(dec_merge_pa_kernel<T>, dim3((unsigned)G), dim3(64), 0, ms, a);                          \
    } while (0)
static void launch_merge(int codec, const DecArgs& a, size_t G, hipStream_t ms)
{
    if (a.outType == PGN_OUT_F32) PGN_LAUNCH_MERGE_PA(float);
    else if (a.outType == PGN_OUT_F16) PGN_LAUNCH_MERGE_PA(_Float16);
    else if (codec == kCodecVbz) hipLaunchKernelGGL(vbz_merge_kernel, dim3((unsigned)G), dim3(64), 0, ms, a);
    else if (a.lookback)  // few chunks: kMergeRanges single-wave workgroups per chunk
        hipLaunchKernelGGL(dec_merge_lb_kernel, dim3((unsigned)(G * kMergeRanges)), dim3(64), 0, ms, a);
    else hipLaunchKernelGGL(dec_merge_kernel, dim3((unsigned)G), dim3(64), 0, ms, a);
}

// capCall: every chunk of the call has at most this many samples (a multiple of 4096, at most
// kPassSamples); the per-chunk intermediates are spaced for it.
static int launch_decode_impl(pgn_ctx* c, int codec, size_t nchunks, const DecIO& io, hipStream_t s, uint32_t capCall)
{
    if (!c->decStaged || (codec != kCodecC5 && codec != kCodecVbz)) return launch_decode_fused(c, codec, nchunks, io, s);
    // large C5 batches: deferred Huffman sections (dec_huf_kernel), passes of up to deferG chunks
    // balanced over the batch; otherwise passes of subBatch chunks
    bool defer = codec == kCodecC5 && nchunks >= c->deferMin;
    const size_t stride = chunk_inter_bytes(capCall);
    size_t G = nchunks < c->subBatch ? nchunks : c->subBatch;  // chunks per pass (the buffers' capacity)
    // the passes: chunks [pBase[p], pBase[p] + pCnt[p]); pPlain[p]: a deferred call's in-place tail
    std::vector<size_t> pBase, pCnt;
    std::vector<char> pPlain;
    if (defer) {  // up to deferG chunks per pass, and decBufs passes' buffers within kDecBufferBudget
        // (the budget's bound is at least subBatch chunks; PGN_DEFER_G below that is the tests' way to
        // run several passes on small batches)
        size_t gmax = kDecBufferBudget / (c->decBufs * (stride + kStreams * (sizeof(DecUnit) + kJobBytes)));
        gmax = gmax < c->subBatch ? c->subBatch : gmax;
        gmax = gmax < c->deferG ? gmax : c->deferG;
        // the passes of up to gmax chunks balanced over the batch, less an optional in-place tail pass
        // (PGN_DEFER_TAIL_PLAIN)
        size_t tail = c->deferTailPlain;
        if (!(tail > 0 && tail <= gmax && nchunks >= 2 * tail)) tail = 0;
        const size_t mid = nchunks - tail;
        const size_t np = (mid + gmax - 1) / gmax;
        const size_t Gd = (mid + np - 1) / np;
        for (size_t b = 0; b < mid; b += Gd) {
            pBase.push_back(b);
            pCnt.push_back(mid - b < Gd ? mid - b : Gd);
            pPlain.push_back(0);
        }
        if (tail) {
            pBase.push_back(nchunks - tail);
            pCnt.push_back(tail);
            pPlain.push_back(1);
        }
        G = 0;
        for (size_t k : pCnt) G = k > G ? k : G;
    } else {
        for (size_t b = 0; b < nchunks; b += G) {
            pBase.push_back(b);
            pCnt.push_back(G);  // the kernels stop at nchunks
            pPlain.push_back(1);
        }
    }
    const size_t passes = pBase.size();
    size_t nDefPasses = 0;  // deferred passes (an in-place tail pass comes last)
    for (size_t p = 0; p < passes; p++) nDefPasses += defer && !pPlain[p] ? 1 : 0;
    const uint32_t nu = codec == kCodecVbz ? 1u : (uint32_t)kStreams;
    const size_t slots = nu * G < c->decSlotsMax ? nu * G : c->decSlotsMax;
    // few chunks: a workgroup per frame (not for the passes of a larger deferred call)
    const bool coop = G <= kCoopMaxChunks && (size_t)nu * G <= slots && !(defer && nchunks > kCoopMaxChunks);
    defer = defer && !coop;  // the cooperative kernel decodes its sections itself
    c->lastDeferred = defer;
    // buffers in rotation: a pass parses into buffer p % nbuf once the merge of pass p - nbuf has read it
    const size_t nbuf = passes > 1 ? (passes < c->decBufs ? passes : c->decBufs) : 1;
    const size_t unitBytes = align_up(G * kStreams * sizeof(DecUnit), 256);
    const size_t bufBytes = G * stride + unitBytes + (defer ? G * kStreams * kJobBytes + kHufJunkBytes : 0);
    int rc = ensure_dec(c, slots, nbuf * bufBytes);
    if (rc) return rc;
    HIPCHK(hipEventRecord(c->ev[2], s));
    rc = ensure_queues(c, passes, s);
    if (rc) return rc;
    // the merge of pass p runs on the side stream beside pass p + 1's zstd kernel; a single pass
    // stays on the caller's stream
#ifdef PGN_SERIAL_DECODE  // diagnostic builds: every decode kernel on the caller's stream (isolated kernel times)
    const hipStream_t sideS = s;
    const bool multi = false;
#else
    const hipStream_t sideS = passes > 1 ? c->side : s;
    const bool multi = passes > 1;
#endif
    // deferred sections over several passes: the sections of pass p on hufS[p % hufStreams], the merges
    // on a third stream behind them
    // 3: the sections and the merge of pass p both on side stream p % 3 (no separate merge stream)
    const hipStream_t hufS[3] = {c->side, c->side2, c->mergeS};
    const size_t hufStreams = c->hufStreams;
    if (passes > 1) {
        HIPCHK(hipEventRecord(c->evFork, s));
        HIPCHK(hipStreamWaitEvent(c->side, c->evFork, 0));
    }
    DecArgs a = dec_args(c, io, nchunks);
    a.slotScratch = c->decScratch;
    a.slotBytes = dec_slot_bytes();
    a.G = G;
    a.nu = nu;
    a.capN = capCall;
    a.interStride = stride;
    if (passes == 1 && G <= kMergeWgMaxChunks && codec != kCodecVbz) {  // the look-back range merge (one epoch per pass)
        const int lrc = take_lookback(c, s, a.lookback, a.epoch);
        if (lrc) return lrc;
    }
    // pass p: parse + zstd on the caller's stream into buffer p % nbuf, the deferred Huffman sections
    // and the merge on the side streams.  Those of pass p overlap the zstd kernel of pass p+1.
    for (size_t p = 0; p < passes; p++) {
        const int b = (int)(p % nbuf);
        uint8_t* buf = c->decChunks + (size_t)b * bufBytes;
        const bool deferP = defer && !pPlain[p];
        a.base = pBase[p];
        a.G = pCnt[p];
        a.inter = buf;
        a.units = (DecUnit*)(buf + G * stride);
        a.jobs = deferP ? buf + G * stride + unitBytes : nullptr;
        // the last deferred pass's sections: nothing after them overlaps their chains
        a.hufPrio = (deferP && c->hufPrioLast && (p + 1 == passes || (p + 2 == passes && pPlain[passes - 1]))) ? 1u : 0u;
        c->lastUnits = a.units;
        c->lastG = a.G;
        a.queue = c->qCur + p;
        if (p >= nbuf) HIPCHK(hipStreamWaitEvent(s, c->evDFree[b], 0));
        a.coopParse = (coop && codec != kCodecVbz) ? 1u : 0u;
        if (codec == kCodecVbz) hipLaunchKernelGGL(vbz_parse_kernel, dim3((unsigned)((G + 63) / 64)), dim3(64), 0, s, a);
        else if (!a.coopParse) hipLaunchKernelGGL(dec_parse_kernel, dim3((unsigned)((G + 63) / 64)), dim3(64), 0, s, a);
        if (coop)
            hipLaunchKernelGGL(dec_zstd_coop_kernel, dim3((unsigned)(nu * G)), dim3(64 * kCoopWaves), 0, s, a);
        else hipLaunchKernelGGL(dec_zstd_kernel, dim3((unsigned)slots), dim3(64), 0, s, a);
        // the stream of this pass's sections (deferred) or merge (otherwise)
        const hipStream_t hs = multi ? (defer ? hufS[p % hufStreams] : c->side) : sideS;
        if (multi && hs != s) {
            HIPCHK(hipEventRecord(c->evDStage[b], s));
            HIPCHK(hipStreamWaitEvent(hs, c->evDStage[b], 0));
        }
        // the deferred sections (kHufFrames frames of one stream type per wave), ahead of the pass's
        // merge: they overlap the next pass's frame decode
        // the last hufWideLast deferred passes: the latency-first decoder (dec_huf_wide_kernel)
        const bool wide = deferP && p + c->hufWideLast >= nDefPasses;
        if (deferP && wide)
            hipLaunchKernelGGL(dec_huf_wide_kernel, dim3((unsigned)(nu * a.G)), dim3(64 * kCoopWaves), 0, hs, a);
        else if (deferP)
            hipLaunchKernelGGL(dec_huf_kernel, dim3((unsigned)(nu * ((a.G + kHufFrames - 1) / kHufFrames))), dim3(64), 0, hs, a);
        // with deferred sections over several passes the merge goes to the third stream behind its
        // pass's sections (so it overlaps the next pass's sections); the buffer is free after it
        hipStream_t ms = hs;
        if (defer && multi && hufStreams < 3 && hs != s) {
            HIPCHK(hipEventRecord(c->evDHuf[b], hs));
            HIPCHK(hipStreamWaitEvent(c->mergeS, c->evDHuf[b], 0));
            ms = c->mergeS;
        }
        launch_merge(codec, a, G, ms);
        if (passes > 1) HIPCHK(hipEventRecord(c->evDFree[b], ms));
    }
    HIPCHK(hipGetLastError());
    if (multi && defer && hufStreams == 3) {  // every buffer's last merge (each follows its pass's sections)
        for (size_t b = 0; b < nbuf; b++) HIPCHK(hipStreamWaitEvent(s, c->evDFree[b], 0));
    } else if (multi) {  // the last merge follows every other launch of the call on the side streams
        HIPCHK(hipEventRecord(c->evJoin, defer ? c->mergeS : c->side));
        HIPCHK(hipStreamWaitEvent(s, c->evJoin, 0));
    }
    return PGN_OK;
}

// ---- the large-chunk pass --------------------------------------------------------------------
// A call whose chunks may exceed kPassSamples (maxHint = the caller's bound on the sample counts,
// 0 = unknown) lists them on the scan stream, after the work queued before the call, while the
// batched pass runs (which leaves them UNSUPPORTED); the host reads the list's header and, when it
// is not empty, runs the fused kernel over the listed chunks with slot buffers spaced for the
// largest of them.  Chunks above PGN_MAX_CHUNK_SAMPLES stay UNSUPPORTED.
static bool need_scan(uint32_t maxHint) { return maxHint == 0 || maxHint > kPassSamples; }

// the large pass's and the claims pass's lists, for n chunks (at least 4,096 entries each)
static int ensure_lists(pgn_ctx* c, size_t n)
{
    const size_t bytes = 4 * (n < 4096 ? 4096 : n);
    return reserve(c, {{c->largeList, bytes}, {c->claimList, bytes}}, kSyncScan);
}

// dec: a decode call's arrays, whose scan also lists the chunks of the claims pass (claim_scan_kernel;
// nf: the codec's frames per chunk)
static int start_scan(pgn_ctx* c, size_t nchunks, const uint32_t* d_counts, hipStream_t s, const DecIO* dec = nullptr,
                      int nf = 0)
{
    const int rc = ensure_lists(c, nchunks);
    if (rc) return rc;
    HIPCHK(hipEventRecord(c->evScanFork, s));
    HIPCHK(hipStreamWaitEvent(c->scanStream, c->evScanFork, 0));
    HIPCHK(hipMemsetAsync(c->largeHdr, 0, 8 * sizeof(uint32_t), c->scanStream));
    unsigned grid = (unsigned)((nchunks + 255) / 256);
    grid = grid > 1024 ? 1024 : grid;
    hipLaunchKernelGGL(large_scan_kernel, dim3(grid), dim3(256), 0, c->scanStream, d_counts, nchunks, c->largeList,
                       c->largeHdr);
    if (dec)
        hipLaunchKernelGGL(claim_scan_kernel, dim3(grid), dim3(256), 0, c->scanStream, dec->in, dec->inOffsets,
                           dec->inSizes, d_counts, nchunks, nf, c->claimList, c->largeHdr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c->largeHdrHost, c->largeHdr, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->scanStream));
    HIPCHK(hipEventRecord(c->evScan, c->scanStream));
    return PGN_OK;
}

// slot buffers of the large pass: spaced for the largest listed chunk (64 Ki-sample steps, so that
// similar calls reuse them), as many slots as fit kLargeScratchBudget (at least one)
constexpr size_t kLargeScratchBudget = (size_t)8 << 30;
static uint32_t large_cap(uint32_t maxN)
{
    const uint64_t r = ((uint64_t)maxN + 65535u) & ~(uint64_t)65535u;
    return r > PGN_MAX_CHUNK_SAMPLES ? PGN_MAX_CHUNK_SAMPLES : (uint32_t)r;
}
static int ensure_large_enc(pgn_ctx* c, size_t bytes, size_t epochSlots)
{
    // fresh tables: tag 0 never matches (as in ensure_enc)
    return reserve(c, {{c->largeScratch, bytes}, {c->largeEpochs, 4 * epochSlots}}, kZeroFill);
}
static int ensure_large_dec(pgn_ctx* c, size_t bytes) { return reserve(c, {{c->largeDecScratch, bytes}}); }
static size_t large_slots(pgn_ctx* c, uint32_t count, size_t slotBytes, size_t fusedMax)
{
    size_t slots = count < fusedMax ? count : fusedMax;
    if (slots * slotBytes > kLargeScratchBudget) slots = kLargeScratchBudget / slotBytes;
    return slots ? slots : 1;
}

static int finish_scan(pgn_ctx* c, uint32_t& count, uint32_t& maxN, uint32_t* maxAll = nullptr)
{
    HIPCHK(hipEventSynchronize(c->evScan));
    count = c->largeHdrHost[0];
    maxN = c->largeHdrHost[1];
    if (maxAll) *maxAll = c->largeHdrHost[3];
    return PGN_OK;
}
// the batched decode's per-chunk sample bound: a multiple of 4096 covering every chunk of the call
static uint32_t call_cap(uint32_t maxN)
{
    const uint32_t r = (maxN + 4095u) & ~4095u;
    return r < 4096u ? 4096u : (r > kPassSamples ? kPassSamples : r);
}

static int launch_large_encode(pgn_ctx* c, int codec, uint32_t count, uint32_t maxN, const EncIO& io, hipStream_t s)
{
    const uint32_t capN = large_cap(maxN);
    const size_t sb = enc_slot_bytes(capN);
    const size_t slots = large_slots(c, count, sb, c->encFusedSlotsMax);
    int rc = ensure_large_enc(c, sb * slots, slots);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(c->largeHdr + 2, 0, sizeof(uint32_t), s));
    EncArgs a = enc_args(c, io, count);
    a.slotScratch = c->largeScratch;
    a.slotBytes = sb;
    a.epochs = c->largeEpochs;  // the large pass's own tables
    a.queue = c->largeHdr + 2;
    a.capN = capN;
    a.list = c->largeList;
    return launch_enc_chunks(codec, a, slots, s);
}

static int launch_large_decode(pgn_ctx* c, int codec, uint32_t count, uint32_t maxN, const DecIO& io, hipStream_t s)
{
    const uint32_t capN = large_cap(maxN);
    const size_t sb = dec_slot_bytes(capN);
    const size_t slots = large_slots(c, count, sb, c->decFusedSlotsMax);
    int rc = ensure_large_dec(c, sb * slots);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(c->largeHdr + 2, 0, sizeof(uint32_t), s));
    DecArgs a = dec_args(c, io, count);
    a.slotScratch = c->largeDecScratch;
    a.slotBytes = sb;
    a.queue = c->largeHdr + 2;
    a.capN = capN;
    a.list = c->largeList;
    return launch_dec_chunks(codec, a, slots, s);
}

// The claims pass: the listed chunks (list: device, count entries) decoded as the reference decodes
// them -- every frame into exactly its content-size claim, in an intermediate of the claims' sum
// (maxSum: the largest listed sum; above kClaimPassMax the chunk is PGN_ERR_ALLOC) -- then merged;
// their statuses and samples replace the batched pass's.  The fused kernel, slot scratch of the
// large pass (ordered after it on the stream).
static int launch_claims_decode(pgn_ctx* c, int codec, uint32_t count, uint64_t maxSum, const uint32_t* list,
                                const DecIO& io, hipStream_t s)
{
    const uint64_t cap = (maxSum < kClaimPassMax ? maxSum : kClaimPassMax) + kVbzPadding;
    const size_t sb = dec_layout().bytes + align_up(cap + 64, 256);
    const size_t slots = large_slots(c, count, sb, c->decFusedSlotsMax);
    int rc = ensure_large_dec(c, sb * slots);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(c->largeHdr + 2, 0, sizeof(uint32_t), s));
    DecArgs a = dec_args(c, io, count);
    a.slotScratch = c->largeDecScratch;
    a.slotBytes = sb;
    a.queue = c->largeHdr + 2;
    a.capN = PGN_MAX_CHUNK_SAMPLES;
    a.list = list;
    a.interBytes = cap;
    return launch_dec_chunks(codec, a, slots, s);
}

// The claims pass for chunks of a host-memory call (the blobs are in host memory too): the chunks
// among [0, n) whose status came back PGN_ERR_UNSUPPORTED are listed on the host from their own bytes
// (the device arrays describe the same chunks); then the pass runs and the call waits for it.
static int claims_from_host(pgn_ctx* c, int codec, size_t n, const int32_t* status, const uint32_t* counts,
                            const uint8_t* const* blobs, const uint64_t* blobLens, const DecIO& io, hipStream_t s)
{
    uint32_t idx[kPcMaxReqs];
    uint32_t k = 0;
    uint64_t maxSum = 0;
    const int nf = codec_frames(codec);
    for (size_t i = 0; i < n && k < (uint32_t)kPcMaxReqs; i++) {
        uint64_t sum = 0;
        if (status[i] != PGN_ERR_UNSUPPORTED || counts[i] > PGN_MAX_CHUNK_SAMPLES) continue;
        if (!claims_pass_chunk(blobs[i], blobLens[i], nf, counts[i], &sum)) continue;
        idx[k++] = (uint32_t)i;
        maxSum = sum > maxSum ? sum : maxSum;
    }
    if (k == 0) return PGN_OK;
    int rc = ensure_lists(c, kPcMaxReqs);  // allocates them when no scan has yet
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(c->claimList, idx, 4 * k, hipMemcpyHostToDevice, s));
    rc = launch_claims_decode(c, codec, k, maxSum, c->claimList, io, s);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(s));
    return PGN_OK;
}

// The encode / decode launch sequence of one call (a CallScope; `lock`: whether the caller already holds
// the context's lock).  ev[0..1] / ev[2..3] bracket the call's kernels.
static int launch_encode(pgn_ctx* c, int codec, size_t nchunks, const EncIO& io, void* stream, uint32_t maxHint,
                         CallScope::Lock lock)
{
    CallScope sc(c, stream, lock);
    if (sc.rc) return sc.rc;
    const hipStream_t s = sc.s;
    const bool scan = need_scan(maxHint);
    int rc = scan ? start_scan(c, nchunks, io.sampleCounts, s) : PGN_OK;
    if (rc == PGN_OK) rc = launch_encode_impl(c, codec, nchunks, io, s);
    uint32_t count = 0, maxN = 0;
    if (rc == PGN_OK && scan) rc = finish_scan(c, count, maxN);
    if (rc == PGN_OK && count) rc = launch_large_encode(c, codec, count, maxN, io, s);
    if (rc == PGN_OK) {
        HIPCHK(hipEventRecord(c->ev[1], s));
        c->encTimed = true;
    }
    return rc;
}

static int launch_decode(pgn_ctx* c, int codec, size_t nchunks, const DecIO& io, void* stream, uint32_t maxHint,
                         CallScope::Lock lock)
{
    CallScope sc(c, stream, lock);
    if (sc.rc) return sc.rc;
    const hipStream_t s = sc.s;
    const bool scan = need_scan(maxHint);
    // The intermediates are spaced for the call's largest chunk when the caller bounds it, else for
    // kPassSamples (the scan then runs beside the batched pass, and the launch stays asynchronous).
    uint32_t capCall = (!scan && maxHint) ? call_cap(maxHint) : kPassSamples;
    uint32_t count = 0, maxN = 0;
    int rc = scan ? start_scan(c, nchunks, io.sampleCounts, s, &io, codec_frames(codec)) : PGN_OK;
    // small calls (the per-chunk ones) keep the full capacity: a frame is then decoded up to its own
    // content size, as the reference does, and the chunk ends with its statuses (e.g. "Remaining
    // data" for samples fewer than the frames hold) rather than PGN_ERR_UNSUPPORTED
    if (nchunks <= kCoopMaxChunks) capCall = kPassSamples;
    if (rc == PGN_OK) rc = launch_decode_impl(c, codec, nchunks, io, s, capCall);
    if (rc == PGN_OK && scan) rc = finish_scan(c, count, maxN);
    if (rc == PGN_OK && count) rc = launch_large_decode(c, codec, count, maxN, io, s);
    // the chunks whose frames claim more than the passes' intermediates hold (listed by the scan)
    if (rc == PGN_OK && scan && c->largeHdrHost[4])
        rc = launch_claims_decode(c, codec, c->largeHdrHost[4], (uint64_t)c->largeHdrHost[5] << 10, c->claimList, io, s);
    if (rc == PGN_OK) {
        HIPCHK(hipEventRecord(c->ev[3], s));
        c->decTimed = true;
    }
    return rc;
}

static int compress_batch(int codec, pgn_ctx* c, size_t nchunks, const EncIO& io, void* stream, uint32_t maxHint = 0)
{
    if (!c || !io.samples || !io.sampleOffsets || !io.sampleCounts || !io.out || !io.outOffsets || !io.outCaps ||
        !io.outSizes || !io.status)
        return PGN_ERR_INVALID_ARG;
    if (nchunks == 0) return PGN_OK;
    return launch_encode(c, codec, nchunks, io, stream, maxHint, CallScope::kLock);
}

static int decompress_batch(int codec, pgn_ctx* c, size_t nchunks, const DecIO& io, void* stream, uint32_t maxHint = 0)
{
    if (!c || !io.in || !io.inOffsets || !io.inSizes || !io.out.p || !io.sampleOffsets || !io.sampleCounts || !io.status)
        return PGN_ERR_INVALID_ARG;
    if (nchunks == 0) return PGN_OK;
    return launch_decode(c, codec, nchunks, io, stream, maxHint, CallScope::kLock);
}

int pgn_compress_batch_device(pgn_ctx* c, size_t nchunks, const int16_t* d_samples, const uint64_t* d_sample_offsets,
                              const uint32_t* d_sample_counts, uint8_t* d_out, const uint64_t* d_out_offsets,
                              const uint64_t* d_out_caps, uint64_t* d_out_sizes, int32_t* d_status, uint64_t* d_stats,
                              void* stream)
{
    const EncIO io{d_samples, d_sample_offsets, d_sample_counts, d_out, d_out_offsets, d_out_caps, d_out_sizes, d_status, d_stats};
    return compress_batch(kCodecC5, c, nchunks, io, stream);
}

int pgn_compress_batch_device_bounded(pgn_ctx* c, uint32_t max_chunk_samples, size_t nchunks, const int16_t* d_samples,
                                      const uint64_t* d_sample_offsets, const uint32_t* d_sample_counts, uint8_t* d_out,
                                      const uint64_t* d_out_offsets, const uint64_t* d_out_caps, uint64_t* d_out_sizes,
                                      int32_t* d_status, uint64_t* d_stats, void* stream)
{
    const EncIO io{d_samples, d_sample_offsets, d_sample_counts, d_out, d_out_offsets, d_out_caps, d_out_sizes, d_status, d_stats};
    return compress_batch(kCodecC5, c, nchunks, io, stream, max_chunk_samples ? max_chunk_samples : 1u);
}

int pgn_decompress_batch_device_bounded(pgn_ctx* c, uint32_t max_chunk_samples, size_t nchunks, const uint8_t* d_in,
                                        const uint64_t* d_in_offsets, const uint64_t* d_in_sizes, int16_t* d_samples,
                                        const uint64_t* d_sample_offsets, const uint32_t* d_sample_counts,
                                        int32_t* d_status, void* stream)
{
    const DecIO io{d_in, d_in_offsets, d_in_sizes, d_samples, d_sample_offsets, d_sample_counts, d_status};
    return decompress_batch(kCodecC5, c, nchunks, io, stream, max_chunk_samples ? max_chunk_samples : 1u);
}

int pgn_decompress_batch_device(pgn_ctx* c, size_t nchunks, const uint8_t* d_in, const uint64_t* d_in_offsets,
                                const uint64_t* d_in_sizes, int16_t* d_samples, const uint64_t* d_sample_offsets,
                                const uint32_t* d_sample_counts, int32_t* d_status, void* stream)
{
    const DecIO io{d_in, d_in_offsets, d_in_sizes, d_samples, d_sample_offsets, d_sample_counts, d_status};
    return decompress_batch(kCodecC5, c, nchunks, io, stream);
}

int pgn_vbz_compress_batch_device(pgn_ctx* c, size_t nchunks, const int16_t* d_samples, const uint64_t* d_sample_offsets,
                                  const uint32_t* d_sample_counts, uint8_t* d_out, const uint64_t* d_out_offsets,
                                  const uint64_t* d_out_caps, uint64_t* d_out_sizes, int32_t* d_status,
                                  uint64_t* d_stats, void* stream)
{
    const EncIO io{d_samples, d_sample_offsets, d_sample_counts, d_out, d_out_offsets, d_out_caps, d_out_sizes, d_status, d_stats};
    return compress_batch(kCodecVbz, c, nchunks, io, stream);
}

int pgn_vbz_decompress_batch_device(pgn_ctx* c, size_t nchunks, const uint8_t* d_in, const uint64_t* d_in_offsets,
                                    const uint64_t* d_in_sizes, int16_t* d_samples, const uint64_t* d_sample_offsets,
                                    const uint32_t* d_sample_counts, int32_t* d_status, void* stream)
{
    const DecIO io{d_in, d_in_offsets, d_in_sizes, d_samples, d_sample_offsets, d_sample_counts, d_status};
    return decompress_batch(kCodecVbz, c, nchunks, io, stream);
}

// the pgnano variants by pgn_variant id -> internal codec
static int variant_codec(int variant)
{
    switch (variant) {
    case PGN_VARIANT_C5: return kCodecC5;
    case PGN_VARIANT_C4: return kCodecC4;
    case PGN_VARIANT_C1: return kCodecC1;
    case PGN_VARIANT_C2: return kCodecC2;
    case PGN_VARIANT_C3: return kCodecC3;
    case PGN_VARIANT_VBZ0: return kCodecVbz0;
    default: return -1;
    }
}

int pgn_variant_compress_batch_device(pgn_ctx* c, int variant, size_t nchunks, const int16_t* d_samples,
                                      const uint64_t* d_sample_offsets, const uint32_t* d_sample_counts, uint8_t* d_out,
                                      const uint64_t* d_out_offsets, const uint64_t* d_out_caps, uint64_t* d_out_sizes,
                                      int32_t* d_status, uint64_t* d_stats, void* stream)
{
    const int codec = variant_codec(variant);
    if (codec < 0) return PGN_ERR_INVALID_ARG;
    const EncIO io{d_samples, d_sample_offsets, d_sample_counts, d_out, d_out_offsets, d_out_caps, d_out_sizes, d_status, d_stats};
    return compress_batch(codec, c, nchunks, io, stream);
}

int pgn_variant_decompress_batch_device(pgn_ctx* c, int variant, size_t nchunks, const uint8_t* d_in,
                                        const uint64_t* d_in_offsets, const uint64_t* d_in_sizes, int16_t* d_samples,
                                        const uint64_t* d_sample_offsets, const uint32_t* d_sample_counts,
                                        int32_t* d_status, void* stream)
{
    const int codec = variant_codec(variant);
    if (codec < 0) return PGN_ERR_INVALID_ARG;
    const DecIO io{d_in, d_in_offsets, d_in_sizes, d_samples, d_sample_offsets, d_sample_counts, d_status};
    return decompress_batch(codec, c, nchunks, io, stream);
}

}  // extern "C"

static int bounded_codec(int codec)
{
    return codec == PGN_POD5_CODEC_VBZ ? (int)kCodecVbz : variant_codec(codec);
}

extern "C" int pgn_decompress_batch_device_pa(pgn_ctx* c, int codec, uint32_t max_chunk_samples, size_t nchunks,
                                              const uint8_t* d_in, const uint64_t* d_in_offsets, const uint64_t* d_in_sizes,
                                              void* d_out, int out_type, const uint64_t* d_out_offsets,
                                              const uint32_t* d_sample_counts, const float* d_cal_offset,
                                              const float* d_cal_scale, int32_t* d_status, void* stream)
{
    const int k = bounded_codec(codec);
    if (!c || k < 0) return PGN_ERR_INVALID_ARG;
    if (out_type != PGN_OUT_INT16 && out_type != PGN_OUT_F32 && out_type != PGN_OUT_F16) return PGN_ERR_INVALID_ARG;
    if (out_type != PGN_OUT_INT16 && (!d_cal_offset || !d_cal_scale)) return PGN_ERR_INVALID_ARG;
    // max_chunk_samples == 0: no bound (the unbounded calls, with their host wait), not a bound of 1
    const DecOut out(d_out, out_type, out_type == PGN_OUT_INT16 ? nullptr : d_cal_offset,
                     out_type == PGN_OUT_INT16 ? nullptr : d_cal_scale);
    const DecIO io{d_in, d_in_offsets, d_in_sizes, out, d_out_offsets, d_sample_counts, d_status};
    return decompress_batch(k, c, nchunks, io, stream, max_chunk_samples);
}

// ---- per-read statistics and normalised output (pgn_select.h) -----------------------------------
static int ensure_norm(pgn_ctx* c, size_t nreads, size_t nchunks)
{
    int rc = reserve(c, {{c->normChunkOut, nchunks * sizeof(uint64_t)}, {c->normChunkRead, nchunks * sizeof(uint32_t)}});
    if (rc) return rc;
    return reserve(c, {{c->normReadN, nreads * sizeof(uint64_t)}, {c->normStats, nreads * sizeof(pgn_read_stats)}});
}

// scratch of the split selection: [SplitHead][itemFirst: slots + 1][slots], and per read the counts of
// the one-workgroup kernel, followed by the classify blocks' totals (one per 512 reads)
static int ensure_split(pgn_ctx* c, size_t nreads, sel::SplitArgs& sa)
{
    const size_t slots = c->split.max_split_reads;
    const size_t firstBytes = ((slots + 1) * sizeof(uint32_t) + 63) & ~(size_t)63;
    int rc = reserve(c, {{c->splitWork, 64 + firstBytes + slots * sizeof(sel::SplitSlot)}});
    if (rc) return rc;
    const size_t nblocks = (nreads + sel::kPlanThreads - 1) / sel::kPlanThreads;
    rc = reserve(c, {{c->splitWholeCounts, nreads * sizeof(uint64_t) + nblocks * sizeof(sel::SplitBlock)}});
    if (rc) return rc;
    static_assert(sizeof(sel::SplitHead) <= 64, "the head's room");
    sa.head = static_cast<sel::SplitHead*>(c->splitWork.p);
    sa.itemFirst = reinterpret_cast<uint32_t*>(c->splitWork + 64);
    sa.slots = reinterpret_cast<sel::SplitSlot*>(c->splitWork + 64 + firstBytes);
    sa.wholeCounts = c->splitWholeCounts;
    sa.blocks = reinterpret_cast<sel::SplitBlock*>(c->splitWholeCounts + nreads);
    return PGN_OK;
}

// The statistics kernels: reads above sel::kShortMax samples one workgroup each, the others one wave
// each; with the split on, the classification and the plan first, and after them the kernels that select
// the reads holding a slot in parts.  countBound: what the host knows no read's count exceeds; where that
// rules a split out, the launches are those without it.
static int launch_read_stats(pgn_ctx* c, sel::StatsArgs a, hipStream_t s, uint64_t countBound = ~0ull)
{
    const size_t cus = (size_t)(c->numCUs > 0 ? c->numCUs : 1);
    const bool split = c->split.max_split_reads > 0 && countBound > c->split.split_min_samples;
    sel::SplitArgs sa{};
    c->splitCounted = false;
    if (split) {
        const int rc = ensure_split(c, a.nreads, sa);
        if (rc != PGN_OK) return rc;
        sa.splitMin = c->split.split_min_samples;
        sa.partSamples = c->split.part_samples;
        sa.maxSlots = c->split.max_split_reads;
        sa.a = a;
        const size_t nblocks = (a.nreads + sel::kPlanThreads - 1) / sel::kPlanThreads;
        hipLaunchKernelGGL(sel::split_classify_kernel, dim3((unsigned)nblocks), dim3(sel::kPlanThreads), 0, s, sa);
        hipLaunchKernelGGL(sel::split_plan_kernel, dim3(1), dim3(sel::kPlanThreads), 0, s, sa);
        HIPCHK(hipGetLastError());
        c->splitCounted = true;
    }
    // the one-workgroup kernel is the same code either way: with the split on it reads the plan's counts,
    // in which a read that holds a slot has none
    sel::StatsArgs whole = a;
    if (split) whole.counts = sa.wholeCounts;
    const size_t longGrid = std::min<size_t>(a.nreads, cus * 4);
    hipLaunchKernelGGL(sel::read_stats_kernel, dim3((unsigned)longGrid), dim3(sel::kSelThreads), 0, s, whole);
    HIPCHK(hipGetLastError());
    const size_t shortGrid = std::min<size_t>((a.nreads + 3) / 4, cus * 8);
    hipLaunchKernelGGL(sel::read_stats_short_kernel, dim3((unsigned)shortGrid), dim3(sel::kSelThreads), 0, s, a);
    HIPCHK(hipGetLastError());
    if (split) {
        // fixed grids (the host knows neither the slots in use nor their parts): the parts kernels hold
        // 32 KB of LDS per workgroup, the slot kernels are one wave per slot
        const dim3 partsGrid((unsigned)(cus * 4)), threads(sel::kSelThreads);
        const dim3 slotGrid((unsigned)std::min<size_t>(sa.maxSlots, cus * 8)), wave(sel::kSlotThreads);
        hipLaunchKernelGGL((sel::split_parts_kernel<false, false>), partsGrid, threads, 0, s, sa);
        hipLaunchKernelGGL(sel::split_place_kernel, slotGrid, wave, 0, s, sa, 0u);
        hipLaunchKernelGGL((sel::split_parts_kernel<false, true>), partsGrid, threads, 0, s, sa);
        hipLaunchKernelGGL(sel::split_finish_kernel<false>, slotGrid, wave, 0, s, sa);
        HIPCHK(hipGetLastError());
        if (a.prm.mode == PGN_NORM_MEDMAD) {
            hipLaunchKernelGGL((sel::split_parts_kernel<true, false>), partsGrid, threads, 0, s, sa);
            hipLaunchKernelGGL(sel::split_place_kernel, slotGrid, wave, 0, s, sa, 1u);
            hipLaunchKernelGGL((sel::split_parts_kernel<true, true>), partsGrid, threads, 0, s, sa);
            hipLaunchKernelGGL(sel::split_finish_kernel<true>, slotGrid, wave, 0, s, sa);
            HIPCHK(hipGetLastError());
        }
    }
    return PGN_OK;
}

extern "C" int pgn_ctx_set_select_split(pgn_ctx* c, const pgn_select_split* v)
{
    if (!c || !sel::split_valid(v)) return PGN_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    c->split = *v;
    c->split.pad = 0;
    return PGN_OK;
}

extern "C" int pgn_ctx_get_select_split(pgn_ctx* c, pgn_select_split* v)
{
    if (!c || !v) return PGN_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    *v = c->split;
    return PGN_OK;
}

extern "C" int pgn_select_split_counts(pgn_ctx* c, uint64_t out[5])
{
    if (!c || !out) return PGN_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(hipSetDevice(c->device));
    wait_last_host(c);
    for (int i = 0; i < 5; i++) out[i] = 0;
    if (c->splitCounted)
        HIPCHK(hipMemcpy(out, c->splitWork + offsetof(sel::SplitHead, counts), 5 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return PGN_OK;
}

extern "C" int pgn_read_stats_device(pgn_ctx* c, size_t nreads, const int16_t* d_samples, const uint64_t* d_read_offsets,
                                     const uint64_t* d_read_counts, const pgn_norm_params* params,
                                     pgn_read_stats* d_stats, void* stream)
{
    if (!c || !sel::params_valid(params)) return PGN_ERR_INVALID_ARG;
    if (!d_samples || !d_read_offsets || !d_read_counts || !d_stats) return PGN_ERR_INVALID_ARG;
    if (nreads == 0) return PGN_OK;
    CallScope sc(c, stream);
    if (sc.rc) return sc.rc;
    const sel::StatsArgs a{d_samples, d_read_offsets, d_read_counts, nreads, *params, d_stats, nullptr, nullptr};
    return launch_read_stats(c, a, sc.s);
}

extern "C" int pgn_decompress_reads_device_norm(pgn_ctx* c, int codec, uint32_t max_chunk_samples, size_t nreads,
                                                size_t nchunks, const uint64_t* d_read_first_chunk, const uint8_t* d_in,
                                                const uint64_t* d_in_offsets, const uint64_t* d_in_sizes,
                                                const uint32_t* d_sample_counts, void* d_out, int out_type,
                                                const uint64_t* d_read_out_offsets, int16_t* d_adc,
                                                const pgn_norm_params* params, pgn_read_stats* d_stats,
                                                int32_t* d_chunk_status, void* stream)
{
    if (!c || !params) return PGN_ERR_INVALID_ARG;
    const int k = bounded_codec(codec);
    if ((params->mode != PGN_NORM_QUANTILE && params->mode != PGN_NORM_MEDMAD) || k < 0 ||
        (out_type != PGN_OUT_F32 && out_type != PGN_OUT_F16))
        return PGN_ERR_INVALID_ARG;
    if (!sel::params_valid(params)) return PGN_ERR_INVALID_ARG;
    if (!d_read_first_chunk || !d_out || !d_read_out_offsets) return PGN_ERR_INVALID_ARG;
    if (nchunks && (!d_in || !d_in_offsets || !d_in_sizes || !d_sample_counts || !d_chunk_status)) return PGN_ERR_INVALID_ARG;
    if (out_type == PGN_OUT_F32 && !d_adc) return PGN_ERR_INVALID_ARG;  // no workspace the host could size
    if (nreads == 0) return PGN_OK;
    if (nreads > 0xFFFFFFFFull) return PGN_ERR_INVALID_ARG;  // the chunks' read index is 32-bit
    CallScope sc(c, stream);
    if (sc.rc) return sc.rc;
    const hipStream_t s = sc.s;
    int rc = ensure_norm(c, nreads, nchunks);
    if (rc != PGN_OK) return rc;
    hipLaunchKernelGGL(sel::expand_reads_kernel, dim3((unsigned)((nreads + 255) / 256)), dim3(256), 0, s, (uint64_t)nreads,
                       d_read_first_chunk, d_read_out_offsets, d_sample_counts, c->normChunkOut, c->normChunkRead,
                       c->normReadN);
    HIPCHK(hipGetLastError());
    // the int16 decode, as the batch calls run it: into d_adc, or into the binary16 output itself
    int16_t* adc = d_adc ? d_adc : (int16_t*)d_out;
    if (nchunks) {
        const DecIO io{d_in, d_in_offsets, d_in_sizes, adc, c->normChunkOut, d_sample_counts, d_chunk_status};
        rc = launch_decode(c, k, nchunks, io, s, max_chunk_samples, CallScope::kLocked);
    }
    if (rc != PGN_OK) return rc;
    pgn_read_stats* stats = d_stats ? d_stats : c->normStats;
    const sel::StatsArgs a{adc, d_read_out_offsets, c->normReadN, nreads, *params, stats, nchunks ? d_chunk_status : nullptr,
                           d_read_first_chunk};
    rc = launch_read_stats(c, a, s);
    if (rc == PGN_OK && nchunks) {
        const sel::NormArgs na{adc, d_out, c->normChunkOut, d_sample_counts, c->normChunkRead, stats, nchunks};
        const dim3 grid((unsigned)std::min<size_t>(nchunks, 1u << 20), sel::kNormSplit);
        if (out_type == PGN_OUT_F32)
            hipLaunchKernelGGL(sel::norm_convert_kernel<float>, grid, dim3(256), 0, s, na);
        else
            hipLaunchKernelGGL(sel::norm_convert_kernel<_Float16>, grid, dim3(256), 0, s, na);
        HIPCHK(hipGetLastError());
    }
    return rc;
}

// ---- whole reads, calibrated (pgn_decompress_reads_device_pa) -----------------------------------
static int ensure_reads_pa(pgn_ctx* c, size_t nchunks)
{
    int rc = ensure_norm(c, 0, nchunks);  // normChunkOut (and the norm call's other per-chunk array)
    if (rc != PGN_OK) return rc;
    return reserve(c, {{c->paChunkOffset, nchunks * sizeof(float)}, {c->paChunkScale, nchunks * sizeof(float)}});
}

static int launch_reads_status(size_t nreads, const uint64_t* d_first, const int32_t* d_chunk_status, int32_t* d_read_status,
                               hipStream_t s)
{
    hipLaunchKernelGGL(sel::reads_status_kernel, dim3((unsigned)((nreads + 255) / 256)), dim3(256), 0, s, (uint64_t)nreads,
                       d_first, d_chunk_status, d_read_status);
    HIPCHK(hipGetLastError());
    return PGN_OK;
}

extern "C" int pgn_decompress_reads_device_pa(pgn_ctx* c, int codec, uint32_t max_chunk_samples, size_t nreads,
                                              size_t nchunks, const uint64_t* d_read_first_chunk, const uint8_t* d_in,
                                              const uint64_t* d_in_offsets, const uint64_t* d_in_sizes,
                                              const uint32_t* d_sample_counts, void* d_out, int out_type,
                                              const uint64_t* d_read_out_offsets, const float* d_read_cal_offset,
                                              const float* d_read_cal_scale, int32_t* d_read_status,
                                              int32_t* d_chunk_status, void* stream)
{
    if (!c) return PGN_ERR_INVALID_ARG;
    const int k = bounded_codec(codec);
    if (k < 0 || (out_type != PGN_OUT_INT16 && out_type != PGN_OUT_F32 && out_type != PGN_OUT_F16)) return PGN_ERR_INVALID_ARG;
    if (nreads == 0) return PGN_OK;  // arrays of no entries may be NULL
    if (!d_read_first_chunk || !d_out || !d_read_out_offsets) return PGN_ERR_INVALID_ARG;
    if (nchunks && (!d_in || !d_in_offsets || !d_in_sizes || !d_sample_counts || !d_chunk_status)) return PGN_ERR_INVALID_ARG;
    const bool cal = out_type != PGN_OUT_INT16;
    if (cal && (!d_read_cal_offset || !d_read_cal_scale)) return PGN_ERR_INVALID_ARG;
    CallScope sc(c, stream);
    if (sc.rc) return sc.rc;
    const hipStream_t s = sc.s;
    int rc = PGN_OK;
    if (nchunks) {
        rc = ensure_reads_pa(c, nchunks);
        if (rc != PGN_OK) return rc;
        hipLaunchKernelGGL(sel::expand_reads_pa_kernel, dim3((unsigned)((nreads + 255) / 256)), dim3(256), 0, s,
                           (uint64_t)nreads, d_read_first_chunk, d_read_out_offsets, d_sample_counts,
                           cal ? d_read_cal_offset : nullptr, cal ? d_read_cal_scale : nullptr, c->normChunkOut,
                           c->paChunkOffset, c->paChunkScale);
        HIPCHK(hipGetLastError());
        // the decode of pgn_decompress_batch_device_pa, with the expanded arrays
        const DecOut out(d_out, out_type, cal ? c->paChunkOffset : nullptr, cal ? c->paChunkScale : nullptr);
        const DecIO io{d_in, d_in_offsets, d_in_sizes, out, c->normChunkOut, d_sample_counts, d_chunk_status};
        rc = launch_decode(c, k, nchunks, io, s, max_chunk_samples, CallScope::kLocked);
        if (rc != PGN_OK) return rc;
    }
    if (d_read_status) rc = launch_reads_status(nreads, d_read_first_chunk, d_chunk_status, d_read_status, s);
    return rc;
}

extern "C" int pgn_reads_status_device(pgn_ctx* c, size_t nreads, const uint64_t* d_read_first_chunk,
                                       const int32_t* d_chunk_status, int32_t* d_read_status, void* stream)
{
    if (!c || !d_read_first_chunk || !d_read_status) return PGN_ERR_INVALID_ARG;
    if (nreads == 0) return PGN_OK;
    CallScope sc(c, stream);
    if (sc.rc) return sc.rc;
    return launch_reads_status(nreads, d_read_first_chunk, d_chunk_status, d_read_status, sc.s);
}

// ---- trimmed, normalised model segments (pgn_segment.h) -----------------------------------------
struct SegWork {
    uint64_t* headN;
    uint64_t* trimOffsets;
    uint64_t* trimCounts;
    pgn_read_stats* headStats;
    pgn_read_stats* stats;
    uint64_t* total;
};

static int ensure_segment(pgn_ctx* c, size_t nreads, SegWork& w)
{
    const int rc = reserve(c, {{c->segWork, nreads * (3 * sizeof(uint64_t) + 2 * sizeof(pgn_read_stats)) + sizeof(uint64_t)}});
    if (rc) return rc;
    const size_t R = nreads;
    w.headN = static_cast<uint64_t*>(c->segWork.p);
    w.trimOffsets = w.headN + R;
    w.trimCounts = w.trimOffsets + R;
    w.headStats = reinterpret_cast<pgn_read_stats*>(w.trimCounts + R);
    w.stats = w.headStats + R;
    w.total = reinterpret_cast<uint64_t*>(w.stats + R);
    return PGN_OK;
}

extern "C" int pgn_segment_reads_device(pgn_ctx* c, size_t nreads, const int16_t* d_samples, const uint64_t* d_read_offsets,
                                        const uint64_t* d_read_counts, const int32_t* d_read_status_in,
                                        const pgn_trim_params* trim, const pgn_norm_params* norm,
                                        const pgn_segment_params* segment, void* d_out, int out_type,
                                        uint64_t segment_capacity, pgn_segment* d_segments, pgn_read_segments* d_reads,
                                        pgn_read_stats* d_stats, uint64_t* d_total, void* stream)
{
    if (!c || !trim || !norm || !segment) return PGN_ERR_INVALID_ARG;
    if (!sel::params_valid(norm) || !seg::trim_params_valid(trim) || !seg::segment_params_valid(segment))
        return PGN_ERR_INVALID_ARG;
    if (out_type != PGN_OUT_F32 && out_type != PGN_OUT_F16) return PGN_ERR_INVALID_ARG;
    if (nreads) {
        if (!d_samples || !d_read_offsets || !d_read_counts || !d_reads) return PGN_ERR_INVALID_ARG;
        if (segment_capacity && (!d_out || !d_segments)) return PGN_ERR_INVALID_ARG;
        if (nreads > 0xFFFFFFFFull) return PGN_ERR_INVALID_ARG;  // a segment's read index is 32-bit
    }
    if (nreads == 0 && !d_total) return PGN_OK;
    CallScope sc(c, stream);
    if (sc.rc) return sc.rc;
    const hipStream_t s = sc.s;
    if (nreads == 0) {
        HIPCHK(hipMemsetAsync(d_total, 0, sizeof(uint64_t), s));
        return PGN_OK;
    }
    SegWork w;
    int rc = ensure_segment(c, nreads, w);
    if (rc != PGN_OK) return rc;
    const size_t cus = (size_t)(c->numCUs > 0 ? c->numCUs : 1);
    const unsigned perRead = (unsigned)((nreads + 255) / 256);
    const unsigned waveGrid = (unsigned)std::min<size_t>((nreads + 3) / 4, cus * 64);
    const bool trimOn = trim->max_samples > 0;
    const uint64_t* offsets = d_read_offsets;
    const uint64_t* counts = d_read_counts;
    if (trimOn) {
        const seg::TrimArgs ta{d_samples, d_read_offsets, d_read_counts, d_read_status_in, nreads, *trim, w.headN,
                               w.headStats, d_reads, w.trimOffsets, w.trimCounts};
        hipLaunchKernelGGL(seg::trim_heads_kernel, dim3(perRead), dim3(256), 0, s, ta);
        HIPCHK(hipGetLastError());
        // med/MAD of the heads: only m2 and mad4 are used, so the float parameters are placeholders
        const pgn_norm_params headPrm{PGN_NORM_MEDMAD, 0, 0.0, 1.0, 1.0f, 1.0f, 1.0f, 0.0f};
        const sel::StatsArgs ha{d_samples, d_read_offsets, w.headN, nreads, headPrm, w.headStats, nullptr, nullptr};
        rc = launch_read_stats(c, ha, s, trim->max_samples);  // a head has at most max_samples
        if (rc != PGN_OK) return rc;
        hipLaunchKernelGGL(seg::trim_kernel, dim3(waveGrid), dim3(256), 0, s, ta);
        HIPCHK(hipGetLastError());
        offsets = w.trimOffsets;
        counts = w.trimCounts;
    }
    pgn_read_stats* stats = d_stats ? d_stats : w.stats;
    const sel::StatsArgs sa{d_samples, offsets, counts, nreads, *norm, stats, nullptr, nullptr};
    rc = launch_read_stats(c, sa, s);
    if (rc != PGN_OK) return rc;
    const uint32_t L = segment->length, S = segment->length - segment->overlap;
    const seg::PlanArgs pa{nreads, d_read_status_in, stats, d_reads, w.total, d_total, segment_capacity, L, S, trimOn ? 0u : 1u};
    hipLaunchKernelGGL(seg::segment_scan_kernel, dim3(1), dim3(seg::kScanThreads), 0, s, pa);
    HIPCHK(hipGetLastError());
    if (segment_capacity) {
        const seg::TableArgs tb{nreads, d_reads, stats, d_segments, segment_capacity, L, S};
        hipLaunchKernelGGL(seg::segment_table_kernel, dim3(waveGrid), dim3(256), 0, s, tb);
        HIPCHK(hipGetLastError());
        // a row is shared by the smallest power of two of threads that covers its 16-byte units, up to the
        // workgroup; longer rows are split over up to kWriteSplit workgroups of four or more passes each
        const uint32_t unit = out_type == PGN_OUT_F32 ? seg::kUnit<float> : seg::kUnit<_Float16>;
        const uint32_t units = (L + unit - 1) / unit;
        uint32_t log2Tpr = 0;
        while (log2Tpr < 8 && (1u << log2Tpr) < units) log2Tpr++;
        const uint32_t rowsPerBlock = seg::kWriteThreads >> log2Tpr;
        const uint32_t split = std::min<uint32_t>(seg::kWriteSplit, std::max<uint32_t>(1, units / (4 * seg::kWriteThreads)));
        const uint64_t blocks = (segment_capacity + rowsPerBlock - 1) / rowsPerBlock;
        const dim3 grid((unsigned)std::min<uint64_t>(blocks, 1u << 20), split);
        const seg::WriteArgs wa{d_samples, d_read_offsets, stats, d_segments, w.total, d_out, segment_capacity, L, log2Tpr};
        if (out_type == PGN_OUT_F32)
            hipLaunchKernelGGL(seg::segment_write_kernel<float>, grid, dim3(seg::kWriteThreads), 0, s, wa);
        else
            hipLaunchKernelGGL(seg::segment_write_kernel<_Float16>, grid, dim3(seg::kWriteThreads), 0, s, wa);
        HIPCHK(hipGetLastError());
    }
    return PGN_OK;
}

// ---- model output back to reads (pgn_stitch.h) ----------------------------------------------------
static int ensure_stitch(pgn_ctx* c, size_t nblocks)
{
    return reserve(c, {{c->stitchSums, (nblocks + 1) * sizeof(uint64_t)}});
}

extern "C" int pgn_stitch_plan_device(pgn_ctx* c, size_t nreads, const pgn_read_segments* d_reads,
                                      const pgn_segment* d_segments, uint64_t segment_capacity,
                                      const pgn_stitch_params* params, pgn_stitch_segment* d_plan,
                                      uint64_t* d_read_frames, void* stream)
{
    if (!c || !params) return PGN_ERR_INVALID_ARG;
    if (!stitch::params_valid(params)) return PGN_ERR_INVALID_ARG;
    if (!d_read_frames) return PGN_ERR_INVALID_ARG;
    if (nreads) {
        if (!d_reads) return PGN_ERR_INVALID_ARG;
        if (segment_capacity && (!d_segments || !d_plan)) return PGN_ERR_INVALID_ARG;
        if (nreads > 0xFFFFFFFFull) return PGN_ERR_INVALID_ARG;  // a segment's read index is 32-bit
        if (segment_capacity >> 40) return PGN_ERR_INVALID_ARG;  // the count kernel's grid
    }
    CallScope sc(c, stream);
    if (sc.rc) return sc.rc;
    const hipStream_t s = sc.s;
    if (nreads == 0) {
        HIPCHK(hipMemsetAsync(d_read_frames, 0, sizeof(uint64_t), s));
        return PGN_OK;
    }
    const uint64_t nblocks = std::max<uint64_t>(1, (segment_capacity + stitch::kPlanThreads - 1) / stitch::kPlanThreads);
    const int rc = ensure_stitch(c, (size_t)nblocks);
    if (rc != PGN_OK) return rc;
    const stitch::PlanArgs pa{nreads, d_reads, d_segments, segment_capacity, params->length, params->frame_samples,
                              params->length / params->frame_samples, d_plan, c->stitchSums, nblocks, d_read_frames};
    hipLaunchKernelGGL(stitch::stitch_count_kernel, dim3((unsigned)nblocks), dim3(stitch::kPlanThreads), 0, s, pa);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(stitch::stitch_scan_kernel, dim3(1), dim3(stitch::kPlanThreads), 0, s, pa);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(stitch::stitch_offset_kernel, dim3((unsigned)nblocks), dim3(stitch::kPlanThreads), 0, s, pa);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(stitch::stitch_read_frames_kernel, dim3((unsigned)(nreads / 256 + 1)), dim3(256), 0, s, pa);
    HIPCHK(hipGetLastError());
    return PGN_OK;
}

extern "C" int pgn_stitch_rows_device(pgn_ctx* c, const pgn_stitch_params* params, const pgn_stitch_segment* d_plan,
                                      uint64_t first_segment, uint64_t nsegments, const void* d_rows,
                                      uint64_t row_stride_bytes, uint64_t frame_stride_bytes, uint32_t frame_bytes,
                                      void* d_out, uint64_t out_frame_base, uint64_t out_capacity_frames, void* stream)
{
    if (!c || !params) return PGN_ERR_INVALID_ARG;
    if (!stitch::params_valid(params)) return PGN_ERR_INVALID_ARG;
    const uint32_t T = params->length / params->frame_samples;
    if (frame_bytes == 0) return PGN_ERR_INVALID_ARG;
    if (frame_stride_bytes < frame_bytes && T != 1) return PGN_ERR_INVALID_ARG;
    if (nsegments == 0) return PGN_OK;
    if (!d_plan || !d_rows || !d_out) return PGN_ERR_INVALID_ARG;
    if (out_capacity_frames == 0) return PGN_OK;
    CallScope sc(c, stream);
    if (sc.rc) return sc.rc;
    const hipStream_t s = sc.s;
    // a piece (a dense row's kept frames, or one frame of a strided row) is shared by the smallest power of
    // two of threads that covers its 16-byte units -- its bytes, up to 32, where the destination is not known
    // to fall on 16-byte boundaries -- up to the workgroup
    const bool dense = frame_stride_bytes == frame_bytes || T == 1;
    const bool alignedDst = ((uintptr_t)d_out & 15u) == 0 && frame_bytes % 16 == 0;
    const uint64_t pieceBytes = dense ? (uint64_t)T * frame_bytes : frame_bytes;
    uint64_t units = (pieceBytes + 15) / 16;
    if (!alignedDst) units = std::max<uint64_t>(units, std::min<uint64_t>(pieceBytes, 32));
    uint32_t log2Tpr = 0;
    while (log2Tpr < 8 && (1ull << log2Tpr) < units) log2Tpr++;
    const uint32_t slots = stitch::kRowsThreads >> log2Tpr;
    const uint64_t blocks = dense ? (nsegments + slots - 1) / slots : nsegments;
    const uint64_t perPart = 4ull * (dense ? stitch::kRowsThreads : slots);
    const uint32_t split = (uint32_t)std::min<uint64_t>(stitch::kRowsSplit, std::max<uint64_t>(1, (dense ? units : T) / perPart));
    const dim3 grid((unsigned)std::min<uint64_t>(blocks, 1u << 20), split);
    const stitch::RowsArgs ra{d_plan + first_segment, nsegments, static_cast<const uint8_t*>(d_rows), row_stride_bytes,
                              frame_stride_bytes, frame_bytes, T, static_cast<uint8_t*>(d_out), out_frame_base,
                              out_capacity_frames, log2Tpr, dense ? 1u : 0u};
    hipLaunchKernelGGL(stitch::stitch_rows_kernel, grid, dim3(stitch::kRowsThreads), 0, s, ra);
    HIPCHK(hipGetLastError());
    return PGN_OK;
}

// ---- stitched frames to bases (pgn_ctc.h) -----------------------------------------------------------
static int ensure_ctc(pgn_ctx* c, size_t ntiles, size_t codeBytes)
{
    // the tiles' sums, the edges' reads, the spans' sums and the total
    int rc = reserve(c, {{c->ctcSums, ((ntiles + 1) * 2 + ntiles / ctc::kScanSpan + 2) * sizeof(uint64_t)}});
    if (rc) return rc;
    return reserve(c, {{c->ctcCodes, codeBytes}});
}

// what the two calls share once their arguments are checked: the label pass (decode) or the count of the
// caller's codes (collapse), the scan, the write pass and the statuses
static int ctc_run(pgn_ctx* c, ctc::Args& a, bool decode, bool ownCodes, void* stream)
{
    CallScope sc(c, stream);
    if (sc.rc) return sc.rc;
    const hipStream_t s = sc.s;
    if (a.nreads == 0) {
        HIPCHK(hipMemsetAsync(a.readBases, 0, sizeof(uint64_t), s));
        return PGN_OK;
    }
    if (a.capacity > UINT64_MAX - a.frameBase) a.capacity = UINT64_MAX - a.frameBase;  // no frame index wraps
    a.ntiles = std::max<uint64_t>(1, (a.capacity + ctc::kTile - 1) / ctc::kTile);
    const int rc = ensure_ctc(c, (size_t)a.ntiles, ownCodes ? (size_t)a.capacity : 0);
    if (rc != PGN_OK) return rc;
    a.tileSums = c->ctcSums;
    a.bounds = reinterpret_cast<uint32_t*>(c->ctcSums + a.ntiles + 1);
    a.spanSums = c->ctcSums + 2 * (a.ntiles + 1);
    a.nspans = (a.ntiles + ctc::kScanSpan - 1) / ctc::kScanSpan;
    if (ownCodes) a.codes = c->ctcCodes;
    const dim3 grid((unsigned)a.ntiles), block(ctc::kThreads);
    const size_t stageBytes = a.staged ? (size_t)ctc::kTile * a.classes * a.elem + 16 : 0;
    hipLaunchKernelGGL(ctc::ctc_bounds_kernel, dim3((unsigned)(a.ntiles / 256 + 1)), dim3(256), 0, s, a);
    HIPCHK(hipGetLastError());
    if (decode)
        hipLaunchKernelGGL(ctc::ctc_label_kernel, grid, block, stageBytes, s, a);
    else
        hipLaunchKernelGGL(ctc::ctc_count_kernel, grid, block, 0, s, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(ctc::ctc_scan_kernel, dim3((unsigned)a.nspans), dim3(ctc::kScanThreads), 0, s, a);
    HIPCHK(hipGetLastError());
    stitch::PlanArgs top{};  // the scan of the spans' totals is the stitch plan's
    top.blockSums = a.spanSums;
    top.nblocks = a.nspans;
    hipLaunchKernelGGL(stitch::stitch_scan_kernel, dim3(1), dim3(stitch::kPlanThreads), 0, s, top);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(ctc::ctc_write_kernel, grid, block, 0, s, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(ctc::ctc_status_kernel, dim3((unsigned)(a.nreads / 256 + 1)), dim3(256), 0, s, a);
    HIPCHK(hipGetLastError());
    return PGN_OK;
}

extern "C" int pgn_ctc_decode_device(pgn_ctx* c, const pgn_ctc_params* params, size_t nreads,
                                     const uint64_t* d_read_frames, const void* d_frames, uint64_t frame_stride_bytes,
                                     uint64_t frame_base, uint64_t frame_capacity, uint8_t* d_seq, uint64_t base_capacity,
                                     uint64_t* d_read_bases, int32_t* d_read_status, uint32_t* d_base_frame,
                                     float* d_base_score, uint8_t* d_codes, void* stream)
{
    if (!c || !params) return PGN_ERR_INVALID_ARG;
    if (!ctc::params_valid(params)) return PGN_ERR_INVALID_ARG;
    const uint32_t elem = ctc::elem_bytes(params->score_type);
    const uint64_t frameBytes = (uint64_t)params->classes * elem;
    if (frame_stride_bytes < frameBytes || frame_stride_bytes % elem || (uintptr_t)d_frames % elem) return PGN_ERR_INVALID_ARG;
    if ((uint64_t)nreads >> 32 || frame_capacity >> 40) return PGN_ERR_INVALID_ARG;
    if (!d_read_bases) return PGN_ERR_INVALID_ARG;
    if (nreads && (!d_read_frames || !d_read_status)) return PGN_ERR_INVALID_ARG;
    if (frame_capacity && !d_frames) return PGN_ERR_INVALID_ARG;
    if (base_capacity && !d_seq) return PGN_ERR_INVALID_ARG;
    ctc::Args a{};
    a.nreads = nreads;
    a.readFrames = d_read_frames;
    a.frames = static_cast<const uint8_t*>(d_frames);
    a.frameStride = frame_stride_bytes;
    a.classes = params->classes;
    a.blank = params->blank;
    a.elem = elem;
    a.staged = frame_stride_bytes == frameBytes && frameBytes <= ctc::kStageFrameBytes;
    a.frameBase = frame_base;
    a.capacity = frame_capacity;
    a.codes = d_codes;
    a.seq = d_seq;
    a.baseCapacity = base_capacity;
    a.readBases = d_read_bases;
    a.status = d_read_status;
    a.baseFrame = d_base_frame;
    a.baseScore = d_base_score;
    memcpy(a.alphabet, params->alphabet, sizeof params->alphabet);
    return ctc_run(c, a, true, d_codes == nullptr, stream);
}

extern "C" int pgn_collapse_codes_device(pgn_ctx* c, const uint8_t alphabet[128], size_t nreads,
                                         const uint64_t* d_read_frames, const uint8_t* d_codes, uint64_t frame_base,
                                         uint64_t frame_capacity, uint8_t* d_seq, uint64_t base_capacity,
                                         uint64_t* d_read_bases, int32_t* d_read_status, uint32_t* d_base_frame,
                                         void* stream)
{
    if (!c || !alphabet) return PGN_ERR_INVALID_ARG;
    if ((uint64_t)nreads >> 32 || frame_capacity >> 40) return PGN_ERR_INVALID_ARG;
    if (!d_read_bases) return PGN_ERR_INVALID_ARG;
    if (nreads && (!d_read_frames || !d_read_status)) return PGN_ERR_INVALID_ARG;
    if (frame_capacity && !d_codes) return PGN_ERR_INVALID_ARG;
    if (base_capacity && !d_seq) return PGN_ERR_INVALID_ARG;
    ctc::Args a{};
    a.nreads = nreads;
    a.readFrames = d_read_frames;
    a.frameBase = frame_base;
    a.capacity = frame_capacity;
    a.codes = const_cast<uint8_t*>(d_codes);  // the count and the write pass only read them
    a.seq = d_seq;
    a.baseCapacity = base_capacity;
    a.readBases = d_read_bases;
    a.status = d_read_status;
    a.baseFrame = d_base_frame;
    memcpy(a.alphabet, alphabet, sizeof a.alphabet);
    return ctc_run(c, a, false, false, stream);
}

// ---- model rows to per-frame codes (pgn_crf.h) --------------------------------------------------------
extern "C" int pgn_ctx_set_crf_scratch(pgn_ctx* c, uint64_t bytes)
{
    if (!c) return PGN_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    c->crfCap = bytes ? bytes : crf::kDefaultScratch;
    return PGN_OK;
}

template <uint32_t K, typename E, uint32_t TR>
static void crf_launch_one(const crf::Args& a, hipStream_t s)
{
    hipLaunchKernelGGL((crf::crf_forward_kernel<K, E, TR>), dim3((unsigned)a.nrows), dim3(crf::Shape<K, E, TR>::kThreads), 0,
                       s, a);
}
template <uint32_t K>
static void crf_launch_k(const crf::Args& a, bool f32, uint32_t tr, hipStream_t s)
{
    if (f32)
        tr == 5 ? crf_launch_one<K, float, 5>(a, s) : crf_launch_one<K, float, 4>(a, s);
    else
        tr == 5 ? crf_launch_one<K, _Float16, 5>(a, s) : crf_launch_one<K, _Float16, 4>(a, s);
}

extern "C" int pgn_crf_viterbi_rows_device(pgn_ctx* c, const pgn_crf_params* params, uint64_t nrows, uint32_t T,
                                           const void* d_rows, uint64_t row_stride_bytes, uint64_t frame_stride_bytes,
                                           uint8_t* d_codes, uint64_t codes_row_stride, float* d_row_score, void* stream)
{
    if (!c || !params) return PGN_ERR_INVALID_ARG;
    if (!crf::params_valid(params)) return PGN_ERR_INVALID_ARG;
    if (T == 0 || T > crf::kMaxT) return PGN_ERR_INVALID_ARG;
    const uint32_t elem = ctc::elem_bytes(params->score_type), S = crf::states(params->state_len);
    const uint64_t frameBytes = (uint64_t)params->transitions * S * elem;
    if (frame_stride_bytes < frameBytes && T != 1) return PGN_ERR_INVALID_ARG;
    if ((uintptr_t)d_rows % elem || row_stride_bytes % elem || frame_stride_bytes % elem) return PGN_ERR_INVALID_ARG;
    if (codes_row_stride < T && nrows > 1) return PGN_ERR_INVALID_ARG;
    if (nrows >> 32) return PGN_ERR_INVALID_ARG;
    // a missing array is refused behind the scratch cap, with the same status: only the cap needs the context
    if (nrows && (!d_rows || !d_codes)) return PGN_ERR_INVALID_ARG;
    const uint64_t rowBytes = crf::row_scratch_bytes(S, T);
    uint64_t cap;
    {
        std::lock_guard<std::mutex> g(c->mu);
        cap = c->crfCap;
    }
    if (rowBytes > cap) return PGN_ERR_INVALID_ARG;
    if (nrows == 0) return PGN_OK;
    CallScope sc(c, stream);
    if (sc.rc) return sc.rc;
    const hipStream_t s = sc.s;
    const uint64_t groupRows = std::min<uint64_t>(cap / rowBytes, 1u << 30);
    const int rc = reserve(c, {{c->crfBp, (size_t)(std::min(nrows, groupRows) * rowBytes)}});
    if (rc != PGN_OK) return rc;
    crf::Args a{};
    a.rowStride = row_stride_bytes;
    a.frameStride = frame_stride_bytes;
    a.T = T;
    a.split = c->crfTrace ? 1u : 0u;
    a.stay = params->stay_score;
    a.codesStride = codes_row_stride;
    a.bp = c->crfBp;
    a.rowWords = rowBytes / 4;
    // the groups follow each other on the stream, so each finds the scratch free
    for (uint64_t g0 = 0; g0 < nrows; g0 += groupRows) {
        a.nrows = std::min(groupRows, nrows - g0);
        a.rows = static_cast<const uint8_t*>(d_rows) + g0 * row_stride_bytes;
        a.codes = d_codes + g0 * codes_row_stride;
        a.rowScore = d_row_score ? d_row_score + g0 : nullptr;
        const bool f32 = params->score_type == PGN_OUT_F32;
        switch (params->state_len) {
        case 1: crf_launch_k<1>(a, f32, params->transitions, s); break;
        case 2: crf_launch_k<2>(a, f32, params->transitions, s); break;
        case 3: crf_launch_k<3>(a, f32, params->transitions, s); break;
        case 4: crf_launch_k<4>(a, f32, params->transitions, s); break;
        default: crf_launch_k<5>(a, f32, params->transitions, s); break;
        }
        HIPCHK(hipGetLastError());
        if (c->crfTrace == 1) {
            hipLaunchKernelGGL(crf::crf_traceback_kernel, dim3((unsigned)((a.nrows + 63) / 64)), dim3(64), 0, s, a, S);
            HIPCHK(hipGetLastError());
        }
    }
    return PGN_OK;
}

// ---- posteriors of model rows (pgn_crf_post.h) and qualities of bases (pgn_qual.h) -----------------------
template <uint32_t K, typename E, uint32_t TR>
static void crf_post_launch_one(const crf::PostArgs& a, uint64_t nrows, hipStream_t s)
{
    hipLaunchKernelGGL((crf::crf_posterior_kernel<K, E, TR>), dim3((unsigned)nrows), dim3(crf::Shape<K, E, TR>::kThreads), 0,
                       s, a);
}
template <uint32_t K>
static void crf_post_launch_k(const crf::PostArgs& a, uint64_t nrows, bool f32, uint32_t tr, hipStream_t s)
{
    if (f32)
        tr == 5 ? crf_post_launch_one<K, float, 5>(a, nrows, s) : crf_post_launch_one<K, float, 4>(a, nrows, s);
    else
        tr == 5 ? crf_post_launch_one<K, _Float16, 5>(a, nrows, s) : crf_post_launch_one<K, _Float16, 4>(a, nrows, s);
}

extern "C" int pgn_crf_posterior_rows_device(pgn_ctx* c, const pgn_crf_params* params, uint64_t nrows, uint32_t T,
                                             const void* d_rows, uint64_t row_stride_bytes, uint64_t frame_stride_bytes,
                                             float* d_post, uint64_t post_row_stride, void* stream)
{
    if (!c || !params) return PGN_ERR_INVALID_ARG;
    if (!crf::params_valid(params)) return PGN_ERR_INVALID_ARG;
    if (T == 0 || T > crf::kMaxT) return PGN_ERR_INVALID_ARG;
    const uint32_t elem = ctc::elem_bytes(params->score_type), S = crf::states(params->state_len);
    const uint64_t frameBytes = (uint64_t)params->transitions * S * elem;
    if (frame_stride_bytes < frameBytes && T != 1) return PGN_ERR_INVALID_ARG;
    if ((uintptr_t)d_rows % elem || row_stride_bytes % elem || frame_stride_bytes % elem) return PGN_ERR_INVALID_ARG;
    if (post_row_stride < 4ull * T && nrows > 1) return PGN_ERR_INVALID_ARG;
    if ((uintptr_t)d_post % 4) return PGN_ERR_INVALID_ARG;
    if (nrows >> 32) return PGN_ERR_INVALID_ARG;
    if (nrows && (!d_rows || !d_post)) return PGN_ERR_INVALID_ARG;
    const uint64_t rowBytes = crf::post_row_scratch_bytes(S, T);
    uint64_t cap;
    {
        std::lock_guard<std::mutex> g(c->mu);
        cap = c->crfCap;
    }
    if (rowBytes > cap) return PGN_ERR_INVALID_ARG;
    if (nrows == 0) return PGN_OK;
    CallScope sc(c, stream);
    if (sc.rc) return sc.rc;
    const hipStream_t s = sc.s;
    const uint64_t groupRows = std::min<uint64_t>(cap / rowBytes, 1u << 30);
    const int rc = reserve(c, {{c->crfBp, (size_t)(std::min(nrows, groupRows) * rowBytes)}});
    if (rc != PGN_OK) return rc;
    crf::PostArgs a{};
    a.rowStride = row_stride_bytes;
    a.frameStride = frame_stride_bytes;
    a.T = T;
    a.stay = params->stay_score;
    a.postStride = post_row_stride;
    a.fwd = static_cast<float*>(c->crfBp.p);
    a.rowWords = rowBytes / 4;
    // the groups follow each other on the stream, so each finds the scratch free
    for (uint64_t g0 = 0; g0 < nrows; g0 += groupRows) {
        const uint64_t n = std::min(groupRows, nrows - g0);
        a.rows = static_cast<const uint8_t*>(d_rows) + g0 * row_stride_bytes;
        a.post = d_post + g0 * post_row_stride;
        const bool f32 = params->score_type == PGN_OUT_F32;
        switch (params->state_len) {
        case 1: crf_post_launch_k<1>(a, n, f32, params->transitions, s); break;
        case 2: crf_post_launch_k<2>(a, n, f32, params->transitions, s); break;
        case 3: crf_post_launch_k<3>(a, n, f32, params->transitions, s); break;
        case 4: crf_post_launch_k<4>(a, n, f32, params->transitions, s); break;
        default: crf_post_launch_k<5>(a, n, f32, params->transitions, s); break;
        }
        HIPCHK(hipGetLastError());
    }
    return PGN_OK;
}

extern "C" int pgn_base_qual_device(pgn_ctx* c, const pgn_qual_params* params, size_t nreads, const uint64_t* d_read_frames,
                                    const uint8_t* d_codes, const float* d_post, uint64_t frame_base,
                                    uint64_t frame_capacity, const uint64_t* d_read_bases, const uint32_t* d_base_frame,
                                    const int32_t* d_read_status, uint8_t* d_qual, uint64_t base_capacity, void* stream)
{
    if (!c || !params) return PGN_ERR_INVALID_ARG;
    if (!qual::params_valid(params)) return PGN_ERR_INVALID_ARG;
    if ((uint64_t)nreads >> 32 || frame_capacity >> 40) return PGN_ERR_INVALID_ARG;
    if ((uintptr_t)d_post % 4) return PGN_ERR_INVALID_ARG;
    if (nreads && (!d_read_frames || !d_read_bases || !d_read_status)) return PGN_ERR_INVALID_ARG;
    if (frame_capacity && (!d_codes || !d_post)) return PGN_ERR_INVALID_ARG;
    if (base_capacity && (!d_base_frame || !d_qual)) return PGN_ERR_INVALID_ARG;
    if (nreads == 0) return PGN_OK;
    CallScope sc(c, stream);
    if (sc.rc) return sc.rc;
    qual::Args a{};
    a.nreads = nreads;
    a.readFrames = d_read_frames;
    a.codes = d_codes;
    a.post = d_post;
    a.frameBase = frame_base;
    a.capacity = std::min(frame_capacity, UINT64_MAX - frame_base);  // no frame index wraps
    a.readBases = d_read_bases;
    a.baseFrame = d_base_frame;
    a.status = d_read_status;
    a.qual = d_qual;
    a.baseCapacity = base_capacity;
    a.prm = *params;
    hipLaunchKernelGGL(qual::base_qual_kernel, dim3((unsigned)std::min<uint64_t>(nreads, 1u << 20)), dim3(qual::kThreads), 0,
                       sc.s, a);
    HIPCHK(hipGetLastError());
    return PGN_OK;
}

// ---- mean quality and FASTQ records (pgn_fastq.h) ----------------------------------------------------------
extern "C" int pgn_read_qual_device(pgn_ctx* c, const pgn_read_qual_params* params, size_t nreads,
                                    const uint64_t* d_read_bases, const int32_t* d_read_status, const uint8_t* d_qual,
                                    uint64_t base_capacity, uint32_t* d_mean_q, uint64_t* d_err_sum, uint8_t* d_pass,
                                    void* stream)
{
    if (!c || !params) return PGN_ERR_INVALID_ARG;
    if (!qual::params_valid(&params->mean)) return PGN_ERR_INVALID_ARG;
    if ((uint64_t)nreads >> 32) return PGN_ERR_INVALID_ARG;
    if (nreads && (!d_read_bases || !d_read_status || !d_mean_q || !d_pass)) return PGN_ERR_INVALID_ARG;
    if (base_capacity && !d_qual) return PGN_ERR_INVALID_ARG;
    if (nreads == 0) return PGN_OK;
    CallScope sc(c, stream);
    if (sc.rc) return sc.rc;
    const hipStream_t s = sc.s;
    if (!d_err_sum) {
        const int rc = reserve(c, {{c->fqWork, nreads * sizeof(uint64_t)}});
        if (rc != PGN_OK) return rc;
    }
    fastq::QualArgs a{};
    a.nreads = nreads;
    a.readBases = d_read_bases;
    a.status = d_read_status;
    a.qual = d_qual;
    a.baseCapacity = base_capacity;
    a.acc = d_err_sum ? d_err_sum : static_cast<uint64_t*>(c->fqWork);
    a.meanQ = d_mean_q;
    a.errSum = d_err_sum;
    a.pass = d_pass;
    a.prm = *params;
    HIPCHK(hipMemsetAsync(a.acc, 0, nreads * sizeof(uint64_t), s));
    const uint64_t ntiles = (base_capacity + fastq::kQualTile - 1) / fastq::kQualTile;
    for (a.tileBase = 0; a.tileBase < ntiles; a.tileBase += 1u << 30) {  // a grid holds fewer than 2^31 tiles
        const uint64_t n = std::min<uint64_t>(ntiles - a.tileBase, 1u << 30);
        hipLaunchKernelGGL(fastq::read_qual_sum_kernel, dim3((unsigned)n), dim3(fastq::kThreads), 0, s, a);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(fastq::read_qual_finish_kernel, dim3((unsigned)(nreads / 256 + 1)), dim3(256), 0, s, a);
    HIPCHK(hipGetLastError());
    return PGN_OK;
}

// Both FASTQ record calls: `tags` is NULL for pgn_fastq_records_device, whose columns are the params' own, and the
// typed columns of pgn_fastq_records_tagged_device (pgn_tags.h) otherwise.
static int fastq_records_call(pgn_ctx* c, const pgn_fastq_params* params, const pgn_record_tags* tags, bool tagged,
                              size_t nreads, const uint8_t* d_read_ids, const uint64_t* d_read_bases,
                              const int32_t* d_read_status, const uint8_t* d_keep, const uint8_t* d_seq,
                              const uint8_t* d_qual, uint64_t base_capacity, uint8_t* d_out, uint64_t byte_capacity,
                              uint64_t* d_rec_off, int32_t* d_rec_status, void* stream)
{
    if (!c || !params || (tagged && !tags)) return PGN_ERR_INVALID_ARG;
    if (tagged) {
        if (params->flags & ~(uint32_t)PGN_FASTQ_REVERSE) return PGN_ERR_INVALID_ARG;
        if (params->ntags != 0) return PGN_ERR_INVALID_ARG;
        if (!tags::columns_valid(tags, true)) return PGN_ERR_INVALID_ARG;
    }
    if (!fastq::params_valid(params)) return PGN_ERR_INVALID_ARG;
    if ((uint64_t)nreads >> 32) return PGN_ERR_INVALID_ARG;
    if (tagged && !tags::pointers_valid(tags, nreads)) return PGN_ERR_INVALID_ARG;
    if (nreads) {
        if (!d_read_ids || !d_read_bases || !d_read_status || !d_rec_status) return PGN_ERR_INVALID_ARG;
        for (uint32_t k = 0; k < params->ntags; k++)
            if (!params->d_tag[k]) return PGN_ERR_INVALID_ARG;
    }
    if (!d_rec_off) return PGN_ERR_INVALID_ARG;
    if (base_capacity && (!d_seq || !d_qual)) return PGN_ERR_INVALID_ARG;
    if (byte_capacity && !d_out) return PGN_ERR_INVALID_ARG;
    CallScope sc(c, stream);
    if (sc.rc) return sc.rc;
    const hipStream_t s = sc.s;
    if (nreads == 0) {
        HIPCHK(hipMemsetAsync(d_rec_off, 0, sizeof(uint64_t), s));
        return PGN_OK;
    }
    fastq::RecArgs a{};
    a.nreads = nreads;
    a.ids = d_read_ids;
    a.readBases = d_read_bases;
    a.status = d_read_status;
    a.keep = d_keep;
    a.seq = d_seq;
    a.qual = d_qual;
    a.baseCapacity = base_capacity;
    a.out = d_out;
    a.byteCapacity = byte_capacity;
    a.recOff = d_rec_off;
    a.recStatus = d_rec_status;
    a.nblocks = (nreads + fastq::kScanThreads - 1) / fastq::kScanThreads;
    a.mis = (uint32_t)((uintptr_t)d_out & 15u);
    a.ntiles = byte_capacity ? (byte_capacity + a.mis + fastq::kTile - 1) / fastq::kTile : 0;
    a.prm = *params;
    const int rc = reserve(c, {{c->fqWork, (size_t)(a.nblocks + 2) * sizeof(uint64_t)}});
    if (rc != PGN_OK) return rc;
    a.blockSums = c->fqWork;
    tags::Cols cols{};
    if (tagged) {
        cols.t = *tags;
        hipLaunchKernelGGL(tags::fastq_len_tagged_kernel, dim3((unsigned)a.nblocks), dim3(fastq::kScanThreads), 0, s, a, cols);
    } else {
        hipLaunchKernelGGL(fastq::fastq_len_kernel, dim3((unsigned)a.nblocks), dim3(fastq::kScanThreads), 0, s, a);
    }
    HIPCHK(hipGetLastError());
    stitch::PlanArgs top{};  // the scan of the workgroups' totals is the stitch plan's
    top.blockSums = a.blockSums;
    top.nblocks = a.nblocks;
    hipLaunchKernelGGL(stitch::stitch_scan_kernel, dim3(1), dim3(stitch::kPlanThreads), 0, s, top);
    HIPCHK(hipGetLastError());
    {
        // a typed read without a record keeps the status its length kernel wrote: the offset kernel copies
        // status[r] to rec_status[r] for such a read, so it is given rec_status as the statuses
        fastq::RecArgs o = a;
        if (tagged) o.status = d_rec_status;
        hipLaunchKernelGGL(fastq::fastq_offset_kernel, dim3((unsigned)a.nblocks), dim3(fastq::kScanThreads), 0, s, o);
    }
    HIPCHK(hipGetLastError());
    if (a.ntiles) {
        // tiles behind the written records end at once, so a capacity far above the text costs little
        const unsigned grid = (unsigned)std::min<uint64_t>(a.ntiles, 1u << 24);
        if (tagged)
            hipLaunchKernelGGL(tags::fastq_write_tagged_kernel, dim3(grid), dim3(fastq::kThreads), 0, s, a, cols);
        else
            hipLaunchKernelGGL(fastq::fastq_write_kernel, dim3(grid), dim3(fastq::kThreads), 0, s, a);
        HIPCHK(hipGetLastError());
    }
    return PGN_OK;
}

extern "C" int pgn_fastq_records_device(pgn_ctx* c, const pgn_fastq_params* params, size_t nreads,
                                        const uint8_t* d_read_ids, const uint64_t* d_read_bases,
                                        const int32_t* d_read_status, const uint8_t* d_keep, const uint8_t* d_seq,
                                        const uint8_t* d_qual, uint64_t base_capacity, uint8_t* d_out,
                                        uint64_t byte_capacity, uint64_t* d_rec_off, int32_t* d_rec_status, void* stream)
{
    return fastq_records_call(c, params, nullptr, false, nreads, d_read_ids, d_read_bases, d_read_status, d_keep, d_seq,
                              d_qual, base_capacity, d_out, byte_capacity, d_rec_off, d_rec_status, stream);
}

extern "C" int pgn_fastq_records_tagged_device(pgn_ctx* c, const pgn_fastq_params* params, const pgn_record_tags* tags,
                                               size_t nreads, const uint8_t* d_read_ids, const uint64_t* d_read_bases,
                                               const int32_t* d_read_status, const uint8_t* d_keep, const uint8_t* d_seq,
                                               const uint8_t* d_qual, uint64_t base_capacity, uint8_t* d_out,
                                               uint64_t byte_capacity, uint64_t* d_rec_off, int32_t* d_rec_status,
                                               void* stream)
{
    return fastq_records_call(c, params, tags, true, nreads, d_read_ids, d_read_bases, d_read_status, d_keep, d_seq,
                              d_qual, base_capacity, d_out, byte_capacity, d_rec_off, d_rec_status, stream);
}

// ---- BAM records (pgn_bam.h) ----------------------------------------------------------------------------------
// Both BAM record calls, as fastq_records_call
static int bam_records_call(pgn_ctx* c, const pgn_bam_params* params, const pgn_record_tags* tags, bool tagged,
                            size_t nreads, const uint8_t* d_read_ids, const uint64_t* d_read_bases,
                            const int32_t* d_read_status, const uint8_t* d_keep, const uint8_t* d_seq, const uint8_t* d_qual,
                            uint64_t base_capacity, const uint64_t* d_read_frames, const uint8_t* d_codes,
                            uint64_t frame_base, uint64_t frame_capacity, uint8_t* d_out, uint64_t byte_capacity,
                            uint64_t* d_rec_off, int32_t* d_rec_status, uint64_t* d_written, void* stream)
{
    if (!c || !params || (tagged && !tags)) return PGN_ERR_INVALID_ARG;
    if (tagged) {
        if (params->flags & ~(uint32_t)(PGN_BAM_REVERSE | PGN_BAM_MOVES | PGN_BAM_BGZF)) return PGN_ERR_INVALID_ARG;
        if (params->ntags != 0) return PGN_ERR_INVALID_ARG;
        if (!tags::columns_valid(tags, false)) return PGN_ERR_INVALID_ARG;
    }
    if (!bam::params_valid(params)) return PGN_ERR_INVALID_ARG;
    if ((uint64_t)nreads >> 32) return PGN_ERR_INVALID_ARG;
    if (tagged && !tags::pointers_valid(tags, nreads)) return PGN_ERR_INVALID_ARG;
    const bool moves = (params->flags & PGN_BAM_MOVES) != 0, bgzf = (params->flags & PGN_BAM_BGZF) != 0;
    if (nreads) {
        if (!d_read_ids || !d_read_bases || !d_read_status || !d_rec_status) return PGN_ERR_INVALID_ARG;
        for (uint32_t k = 0; k < params->ntags; k++)
            if (!params->d_tag[k]) return PGN_ERR_INVALID_ARG;
        if (moves && !d_read_frames) return PGN_ERR_INVALID_ARG;
    }
    if (!d_rec_off || !d_written) return PGN_ERR_INVALID_ARG;
    if (base_capacity && !d_seq) return PGN_ERR_INVALID_ARG;
    if (moves && frame_capacity && !d_codes) return PGN_ERR_INVALID_ARG;
    if (byte_capacity && !d_out) return PGN_ERR_INVALID_ARG;
    CallScope sc(c, stream);
    if (sc.rc) return sc.rc;
    const hipStream_t s = sc.s;
    if (nreads == 0) {
        HIPCHK(hipMemsetAsync(d_rec_off, 0, sizeof(uint64_t), s));
        HIPCHK(hipMemsetAsync(d_written, 0, 2 * sizeof(uint64_t), s));
        return PGN_OK;
    }
    bam::Args a{};
    a.nreads = nreads;
    a.ids = d_read_ids;
    a.readBases = d_read_bases;
    a.status = d_read_status;
    a.keep = d_keep;
    a.seq = d_seq;
    a.qual = d_qual;
    a.baseCapacity = base_capacity;
    a.readFrames = d_read_frames;
    a.codes = d_codes;
    a.frameBase = frame_base;
    a.frameCapacity = frame_capacity;
    a.out = d_out;
    a.streamCapacity = bgzf ? bam::bgzf_stream_capacity(byte_capacity) : byte_capacity;
    a.recOff = d_rec_off;
    a.recStatus = d_rec_status;
    a.written = d_written;
    a.nblocks = (nreads + bam::kScanThreads - 1) / bam::kScanThreads;
    a.ntiles = (a.streamCapacity + bam::kBlock - 1) / bam::kBlock;
    a.crcSplit = bgzf && c->bamCrcSplit;
    a.prm = *params;
    const int rc = reserve(c, {{c->fqWork, (size_t)(a.nblocks + 1) * sizeof(uint64_t)}});
    if (rc != PGN_OK) return rc;
    a.blockSums = c->fqWork;
    tags::Cols cols{};
    if (tagged) {
        cols.t = *tags;
        hipLaunchKernelGGL(tags::bam_len_tagged_kernel, dim3((unsigned)a.nblocks), dim3(bam::kScanThreads), 0, s, a, cols);
    } else {
        hipLaunchKernelGGL(bam::bam_len_kernel, dim3((unsigned)a.nblocks), dim3(bam::kScanThreads), 0, s, a);
    }
    HIPCHK(hipGetLastError());
    stitch::PlanArgs top{};  // the scan of the workgroups' totals is the stitch plan's
    top.blockSums = a.blockSums;
    top.nblocks = a.nblocks;
    hipLaunchKernelGGL(stitch::stitch_scan_kernel, dim3(1), dim3(stitch::kPlanThreads), 0, s, top);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(bam::bam_offset_kernel, dim3((unsigned)a.nblocks), dim3(bam::kScanThreads), 0, s, a);
    HIPCHK(hipGetLastError());
    if (a.ntiles) {
        // tiles behind the written records end at once, so a capacity far above the stream costs little
        const unsigned grid = (unsigned)std::min<uint64_t>(a.ntiles, 1u << 24);
        if (tagged)
            hipLaunchKernelGGL(tags::bam_write_tagged_kernel, dim3(grid), dim3(bam::kThreads), 0, s, a, cols);
        else
            hipLaunchKernelGGL(bam::bam_write_kernel, dim3(grid), dim3(bam::kThreads), 0, s, a);
        HIPCHK(hipGetLastError());
        if (a.crcSplit) {
            hipLaunchKernelGGL(bam::bgzf_crc_kernel, dim3(grid), dim3(bam::kThreads), 0, s, a);
            HIPCHK(hipGetLastError());
        }
    }
    return PGN_OK;
}

extern "C" int pgn_bam_records_device(pgn_ctx* c, const pgn_bam_params* params, size_t nreads, const uint8_t* d_read_ids,
                                      const uint64_t* d_read_bases, const int32_t* d_read_status, const uint8_t* d_keep,
                                      const uint8_t* d_seq, const uint8_t* d_qual, uint64_t base_capacity,
                                      const uint64_t* d_read_frames, const uint8_t* d_codes, uint64_t frame_base,
                                      uint64_t frame_capacity, uint8_t* d_out, uint64_t byte_capacity,
                                      uint64_t* d_rec_off, int32_t* d_rec_status, uint64_t* d_written, void* stream)
{
    return bam_records_call(c, params, nullptr, false, nreads, d_read_ids, d_read_bases, d_read_status, d_keep, d_seq,
                            d_qual, base_capacity, d_read_frames, d_codes, frame_base, frame_capacity, d_out, byte_capacity,
                            d_rec_off, d_rec_status, d_written, stream);
}

extern "C" int pgn_bam_records_tagged_device(pgn_ctx* c, const pgn_bam_params* params, const pgn_record_tags* tags,
                                             size_t nreads, const uint8_t* d_read_ids, const uint64_t* d_read_bases,
                                             const int32_t* d_read_status, const uint8_t* d_keep, const uint8_t* d_seq,
                                             const uint8_t* d_qual, uint64_t base_capacity, const uint64_t* d_read_frames,
                                             const uint8_t* d_codes, uint64_t frame_base, uint64_t frame_capacity,
                                             uint8_t* d_out, uint64_t byte_capacity, uint64_t* d_rec_off,
                                             int32_t* d_rec_status, uint64_t* d_written, void* stream)
{
    return bam_records_call(c, params, tags, true, nreads, d_read_ids, d_read_bases, d_read_status, d_keep, d_seq, d_qual,
                            base_capacity, d_read_frames, d_codes, frame_base, frame_capacity, d_out, byte_capacity,
                            d_rec_off, d_rec_status, d_written, stream);
}

// ---- BGZF deflate (pgn_deflate.h) -----------------------------------------------------------------------------
extern "C" int pgn_bgzf_deflate_device(pgn_ctx* c, uint32_t flags, const uint8_t* d_src, uint64_t src_capacity,
                                       const uint64_t* d_nbytes, uint8_t* d_out, uint64_t byte_capacity,
                                       uint64_t* d_blk_off, uint64_t* d_written, void* stream)
{
    if (!c) return PGN_ERR_INVALID_ARG;
    if (flags) return PGN_ERR_INVALID_ARG;
    if (src_capacity && !d_src) return PGN_ERR_INVALID_ARG;
    if (!d_blk_off || !d_written) return PGN_ERR_INVALID_ARG;
    if (byte_capacity && !d_out) return PGN_ERR_INVALID_ARG;
    if (src_capacity >> 48) return PGN_ERR_INVALID_ARG;
    CallScope sc(c, stream);
    if (sc.rc) return sc.rc;
    const hipStream_t s = sc.s;
    if (src_capacity == 0) {
        HIPCHK(hipMemsetAsync(d_blk_off, 0, sizeof(uint64_t), s));
        HIPCHK(hipMemsetAsync(d_written, 0, 2 * sizeof(uint64_t), s));
        return PGN_OK;
    }
    deflate::Args a{};
    a.src = d_src;
    a.srcCapacity = src_capacity;
    a.nbytes = d_nbytes;
    a.out = d_out;
    a.byteCapacity = byte_capacity;
    a.blkOff = d_blk_off;
    a.written = d_written;
    a.ntiles = (src_capacity + deflate::kBlock - 1) / deflate::kBlock;
    const int rc = reserve(c, {{c->bgzfPlans, (size_t)a.ntiles * sizeof(deflate::BlockPlan)}});
    if (rc != PGN_OK) return rc;
    a.plans = c->bgzfPlans;
    // tiles behind the stream's end finish at once, so a capacity far above *d_nbytes costs little
    const unsigned grid = (unsigned)std::min<uint64_t>(a.ntiles, 1u << 24);
    hipLaunchKernelGGL(deflate::deflate_plan_kernel, dim3(grid), dim3(deflate::kThreads), 0, s, a);
    HIPCHK(hipGetLastError());
    if (c->bgzfKernels < 2) return PGN_OK;
    stitch::PlanArgs top{};  // the scan of the blocks' lengths is the stitch plan's
    top.blockSums = d_blk_off;
    top.nblocks = a.ntiles;
    hipLaunchKernelGGL(stitch::stitch_scan_kernel, dim3(1), dim3(stitch::kPlanThreads), 0, s, top);
    HIPCHK(hipGetLastError());
    if (c->bgzfKernels < 3) return PGN_OK;
    hipLaunchKernelGGL(deflate::deflate_pack_kernel, dim3(grid), dim3(deflate::kThreads), 0, s, a);
    HIPCHK(hipGetLastError());
    return PGN_OK;
}

// ---- adapters and barcodes (pgn_demux.h) -------------------------------------------------------------------------
extern "C" int pgn_find_patterns_device(pgn_ctx* c, size_t nreads, const uint8_t* d_seq, const uint64_t* d_read_bases,
                                        const int32_t* d_read_status, uint64_t base_capacity, uint32_t window,
                                        uint32_t npatterns, const uint8_t* d_pat, uint64_t pat_capacity,
                                        const uint32_t* d_pat_off, const uint8_t* d_pat_side, const uint32_t* d_max_dist,
                                        uint32_t* d_dist, uint32_t* d_start, uint32_t* d_end, void* stream)
{
    if (!c) return PGN_ERR_INVALID_ARG;
    if (window < 1 || window > demux::kMaxWindow || npatterns < 1 || npatterns > demux::kMaxPatterns) return PGN_ERR_INVALID_ARG;
    if ((uint64_t)nreads >> 32) return PGN_ERR_INVALID_ARG;
    if (!d_pat_off || !d_pat_side || !d_max_dist) return PGN_ERR_INVALID_ARG;
    if (pat_capacity && !d_pat) return PGN_ERR_INVALID_ARG;
    if (nreads && (!d_read_bases || !d_read_status || !d_dist || !d_start || !d_end)) return PGN_ERR_INVALID_ARG;
    if (base_capacity && !d_seq) return PGN_ERR_INVALID_ARG;
    if (nreads == 0) return PGN_OK;
    CallScope sc(c, stream);
    if (sc.rc) return sc.rc;
    const hipStream_t s = sc.s;
    const int rc = reserve(c, {{c->demuxIndex, (size_t)(3 * npatterns + 3) * sizeof(uint32_t)}});
    if (rc != PGN_OK) return rc;
    demux::FindArgs a{};
    a.nreads = nreads;
    a.seq = d_seq;
    a.readBases = d_read_bases;
    a.status = d_read_status;
    a.baseCapacity = base_capacity;
    a.window = window;
    a.npat = npatterns;
    a.pat = d_pat;
    a.patCapacity = pat_capacity;
    a.patOff = d_pat_off;
    a.patSide = d_pat_side;
    a.maxDist = d_max_dist;
    a.dist = d_dist;
    a.start = d_start;
    a.end = d_end;
    a.index = c->demuxIndex;
    a.byLength = c->demuxByLength ? 1u : 0u;
    hipLaunchKernelGGL(demux::pattern_index_kernel, dim3(1), dim3(demux::kIndexThreads), 0, s, a);
    HIPCHK(hipGetLastError());
    const unsigned grid = (unsigned)std::min<uint64_t>(2 * (uint64_t)nreads, 1u << 22);
    hipLaunchKernelGGL(demux::find_patterns_kernel, dim3(grid), dim3(demux::kFindThreads), 0, s, a);
    HIPCHK(hipGetLastError());
    return PGN_OK;
}

extern "C" int pgn_classify_reads_device(pgn_ctx* c, size_t nreads, const uint64_t* d_read_bases,
                                         const int32_t* d_read_status, uint64_t base_capacity, uint32_t npatterns,
                                         const uint8_t* d_pat_side, const uint32_t* d_max_dist, const uint32_t* d_pat_class,
                                         uint32_t nclasses, uint32_t min_sep, const uint32_t* d_dist,
                                         const uint32_t* d_start, const uint32_t* d_end, uint32_t* d_barcode,
                                         uint32_t* d_best_dist, uint32_t* d_second_dist, uint32_t* d_lo, uint32_t* d_hi,
                                         void* stream)
{
    if (!c) return PGN_ERR_INVALID_ARG;
    if (npatterns < 1 || npatterns > demux::kMaxPatterns) return PGN_ERR_INVALID_ARG;
    if ((uint64_t)nreads >> 32) return PGN_ERR_INVALID_ARG;
    if (!d_pat_side || !d_max_dist || !d_pat_class) return PGN_ERR_INVALID_ARG;
    if (nreads && (!d_read_bases || !d_read_status || !d_dist || !d_start || !d_end || !d_barcode || !d_best_dist ||
                   !d_second_dist || !d_lo || !d_hi))
        return PGN_ERR_INVALID_ARG;
    if (nreads == 0) return PGN_OK;
    CallScope sc(c, stream);
    if (sc.rc) return sc.rc;
    demux::ClassArgs a{};
    a.nreads = nreads;
    a.readBases = d_read_bases;
    a.status = d_read_status;
    a.baseCapacity = base_capacity;
    a.npat = npatterns;
    a.nclasses = nclasses;
    a.minSep = min_sep;
    a.patSide = d_pat_side;
    a.maxDist = d_max_dist;
    a.patClass = d_pat_class;
    a.dist = d_dist;
    a.start = d_start;
    a.end = d_end;
    a.barcode = d_barcode;
    a.bestDist = d_best_dist;
    a.secondDist = d_second_dist;
    a.lo = d_lo;
    a.hi = d_hi;
    const unsigned grid = (unsigned)((nreads + demux::kFlatThreads - 1) / demux::kFlatThreads);
    hipLaunchKernelGGL(demux::classify_reads_kernel, dim3(grid), dim3(demux::kFlatThreads), 0, sc.s, a);
    HIPCHK(hipGetLastError());
    return PGN_OK;
}

extern "C" int pgn_trim_reads_device(pgn_ctx* c, size_t nreads, const uint8_t* d_seq, const uint8_t* d_qual,
                                     const uint64_t* d_read_bases, const int32_t* d_read_status, uint64_t base_capacity,
                                     const uint32_t* d_lo, const uint32_t* d_hi, const uint32_t* d_base_frame,
                                     const uint64_t* d_read_frames, const uint8_t* d_codes, uint64_t frame_base,
                                     uint64_t frame_capacity, uint8_t* d_new_seq, uint8_t* d_new_qual,
                                     uint32_t* d_new_base_frame, uint64_t new_base_capacity, uint64_t* d_new_read_bases,
                                     int32_t* d_new_status, uint8_t* d_new_codes, uint64_t new_frame_capacity,
                                     uint64_t* d_new_read_frames, uint32_t* d_trim_frames, void* stream)
{
    if (!c) return PGN_ERR_INVALID_ARG;
    if ((uint64_t)nreads >> 32) return PGN_ERR_INVALID_ARG;
    const bool moves = d_read_frames != nullptr;
    if (!d_new_read_bases) return PGN_ERR_INVALID_ARG;
    if (moves && !d_new_read_frames) return PGN_ERR_INVALID_ARG;
    if (nreads) {
        if (!d_read_bases || !d_read_status || !d_lo || !d_hi || !d_new_status) return PGN_ERR_INVALID_ARG;
        if (moves && !d_trim_frames) return PGN_ERR_INVALID_ARG;
    }
    if (base_capacity && (!d_seq || (moves && !d_base_frame))) return PGN_ERR_INVALID_ARG;
    if (moves && frame_capacity && !d_codes) return PGN_ERR_INVALID_ARG;
    if (new_base_capacity && (!d_new_seq || (d_qual && !d_new_qual) || (moves && !d_new_base_frame))) return PGN_ERR_INVALID_ARG;
    if (moves && new_frame_capacity && !d_new_codes) return PGN_ERR_INVALID_ARG;
    CallScope sc(c, stream);
    if (sc.rc) return sc.rc;
    const hipStream_t s = sc.s;
    if (nreads == 0) {
        HIPCHK(hipMemsetAsync(d_new_read_bases, 0, sizeof(uint64_t), s));
        if (moves) HIPCHK(hipMemsetAsync(d_new_read_frames, 0, sizeof(uint64_t), s));
        return PGN_OK;
    }
    demux::TrimArgs a{};
    a.nreads = nreads;
    a.seq = d_seq;
    a.qual = d_qual;
    a.readBases = d_read_bases;
    a.status = d_read_status;
    a.baseCapacity = base_capacity;
    a.lo = d_lo;
    a.hi = d_hi;
    a.baseFrame = d_base_frame;
    a.readFrames = d_read_frames;
    a.codes = d_codes;
    a.frameBase = frame_base;
    a.frameCapacity = frame_capacity;
    a.newSeq = d_new_seq;
    a.newQual = d_new_qual;
    a.newBaseFrame = d_new_base_frame;
    a.newBaseCapacity = new_base_capacity;
    a.newReadBases = d_new_read_bases;
    a.newStatus = d_new_status;
    a.newCodes = d_new_codes;
    a.newFrameCapacity = new_frame_capacity;
    a.newReadFrames = d_new_read_frames;
    a.trimFrames = d_trim_frames;
    a.nblocks = (nreads + demux::kScanThreads - 1) / demux::kScanThreads;
    const int rc = reserve(c, {{c->fqWork, (size_t)(2 * (a.nblocks + 1)) * sizeof(uint64_t)}});
    if (rc != PGN_OK) return rc;
    a.blockSums = c->fqWork;
    hipLaunchKernelGGL(demux::trim_len_kernel, dim3((unsigned)a.nblocks), dim3(demux::kScanThreads), 0, s, a);
    HIPCHK(hipGetLastError());
    for (int k = 0; k < (moves ? 2 : 1); k++) {
        stitch::PlanArgs top{};  // the scan of the workgroups' totals is the stitch plan's
        top.blockSums = a.blockSums + k * (a.nblocks + 1);
        top.nblocks = a.nblocks;
        hipLaunchKernelGGL(stitch::stitch_scan_kernel, dim3(1), dim3(stitch::kPlanThreads), 0, s, top);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(demux::trim_offset_kernel, dim3((unsigned)a.nblocks), dim3(demux::kScanThreads), 0, s, a);
    HIPCHK(hipGetLastError());
    // units and values behind the slices' end finish at once, so a capacity far above the kept bases costs little
    auto flat_grid = [](uint64_t items) {
        return (unsigned)std::min<uint64_t>((items + demux::kFlatThreads - 1) / demux::kFlatThreads, 1u << 22);
    };
    demux::CopyArgs cp{};
    cp.nreads = nreads;
    cp.newOff = d_new_read_bases;
    cp.oldOff = d_read_bases;
    cp.shift = d_lo;
    cp.capacity = new_base_capacity;
    if (new_base_capacity) {
        const unsigned grid = flat_grid(new_base_capacity / 16 + 2);
        cp.src = d_seq;
        cp.dst = d_new_seq;
        hipLaunchKernelGGL(demux::trim_copy_kernel, dim3(grid), dim3(demux::kFlatThreads), 0, s, cp);
        HIPCHK(hipGetLastError());
        if (d_qual) {
            cp.src = d_qual;
            cp.dst = d_new_qual;
            hipLaunchKernelGGL(demux::trim_copy_kernel, dim3(grid), dim3(demux::kFlatThreads), 0, s, cp);
            HIPCHK(hipGetLastError());
        }
        if (moves) {
            cp.src = d_base_frame;
            cp.dst = d_new_base_frame;
            cp.sub = d_trim_frames;
            hipLaunchKernelGGL(demux::trim_base_frame_kernel, dim3(flat_grid(new_base_capacity)), dim3(demux::kFlatThreads), 0,
                               s, cp);
            HIPCHK(hipGetLastError());
        }
    }
    if (moves && new_frame_capacity) {
        cp.newOff = d_new_read_frames;
        cp.oldOff = d_read_frames;
        cp.oldBase = frame_base;
        cp.shift = d_trim_frames;
        cp.sub = nullptr;
        cp.src = d_codes;
        cp.dst = d_new_codes;
        cp.capacity = new_frame_capacity;
        hipLaunchKernelGGL(demux::trim_copy_kernel, dim3(flat_grid(new_frame_capacity / 16 + 2)), dim3(demux::kFlatThreads), 0,
                           s, cp);
        HIPCHK(hipGetLastError());
    }
    return PGN_OK;
}

// ---- in-library entry points of the POD5 loader (pgn_internal.h) --------------------------------
void* pgn_ctx_ext_get(pgn_ctx* c) { return c ? c->ext : nullptr; }
void pgn_ctx_ext_set(pgn_ctx* c, void* p, void (*destroy)(void*))
{
    c->ext = p;
    c->extDestroy = destroy;
}
int pgn_ctx_device(pgn_ctx* c) { return c->device; }
bool pgn_norm_params_valid(const pgn_norm_params* params) { return sel::params_valid(params); }

int pgn_norm_decoded_reads(pgn_ctx* c, size_t nreads, size_t nchunks, const int16_t* d_adc, void* d_out, int out_type,
                           const uint64_t* d_read_out_offsets, const uint64_t* d_read_n, const uint64_t* d_chunk_out,
                           const uint32_t* d_sample_counts, const uint32_t* d_chunk_read, const pgn_norm_params* params,
                           pgn_read_stats* d_stats, void* stream)
{
    if (!c || !sel::params_valid(params) || (out_type != PGN_OUT_F32 && out_type != PGN_OUT_F16)) return PGN_ERR_INVALID_ARG;
    if (nreads == 0) return PGN_OK;
    CallScope sc(c, stream);
    if (sc.rc) return sc.rc;
    const hipStream_t s = sc.s;
    int rc = ensure_norm(c, nreads, 0);
    if (rc != PGN_OK) return rc;
    pgn_read_stats* stats = d_stats ? d_stats : c->normStats;
    const sel::StatsArgs a{d_adc, d_read_out_offsets, d_read_n, nreads, *params, stats, nullptr, nullptr};
    rc = launch_read_stats(c, a, s);
    if (rc == PGN_OK && nchunks) {
        const sel::NormArgs na{d_adc, d_out, d_chunk_out, d_sample_counts, d_chunk_read, stats, nchunks};
        const dim3 grid((unsigned)std::min<size_t>(nchunks, 1u << 20), sel::kNormSplit);
        if (out_type == PGN_OUT_F32)
            hipLaunchKernelGGL(sel::norm_convert_kernel<float>, grid, dim3(256), 0, s, na);
        else
            hipLaunchKernelGGL(sel::norm_convert_kernel<_Float16>, grid, dim3(256), 0, s, na);
        HIPCHK(hipGetLastError());
    }
    return rc;
}

int pgn_compress_batch_bounded(pgn_ctx* c, int codec, uint32_t max_samples, size_t nchunks, const int16_t* d_samples,
                               const uint64_t* d_sample_offsets, const uint32_t* d_sample_counts, uint8_t* d_out,
                               const uint64_t* d_out_offsets, const uint64_t* d_out_caps, uint64_t* d_out_sizes,
                               int32_t* d_status, uint64_t* d_stats, void* stream)
{
    const int k = bounded_codec(codec);
    if (k < 0) return PGN_ERR_INVALID_ARG;
    const EncIO io{d_samples, d_sample_offsets, d_sample_counts, d_out, d_out_offsets, d_out_caps, d_out_sizes, d_status, d_stats};
    return compress_batch(k, c, nchunks, io, stream, max_samples);
}

int pgn_decompress_batch_bounded(pgn_ctx* c, int codec, uint32_t max_samples, size_t nchunks, const uint8_t* d_in,
                                 const uint64_t* d_in_offsets, const uint64_t* d_in_sizes, int16_t* d_samples,
                                 const uint64_t* d_sample_offsets, const uint32_t* d_sample_counts, int32_t* d_status,
                                 void* stream)
{
    const int k = bounded_codec(codec);
    if (k < 0) return PGN_ERR_INVALID_ARG;
    const DecIO io{d_in, d_in_offsets, d_in_sizes, d_samples, d_sample_offsets, d_sample_counts, d_status};
    return decompress_batch(k, c, nchunks, io, stream, max_samples);
}

extern "C" {

#ifdef PGN_DEBUG_HUF
// diagnostic build only: the Huffman decoder's record buffer (count, then records of 8 words)
int pgn_debug_huf_dump(uint32_t* out, size_t nwords)
{
    uint32_t cnt = 0;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpyFromSymbol(&cnt, HIP_SYMBOL(gHufDbgN), 4));
    out[0] = cnt;
    size_t m = cnt < (1u << 18) ? cnt : (1u << 18);
    if (m > nwords - 1) m = nwords - 1;
    HIPCHK(hipMemcpyFromSymbol(out + 1, HIP_SYMBOL(gHufDbg), 4 * m));
    return PGN_OK;
}
#endif

int pgn_debug_phase_cycles(pgn_ctx* c, uint64_t* out, int n)
{
    if (!c || !out || n < 2 * kPhases) return PGN_ERR_INVALID_ARG;
    const int m = n < kProfWords ? n : kProfWords;
    if (!c->prof) {
        memset(out, 0, sizeof(uint64_t) * m);
        return PGN_OK;
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, c->prof, sizeof(uint64_t) * m, hipMemcpyDeviceToHost));
    return PGN_OK;
}

// Diagnostics: the per-stream decode records {frame offset, length, content size, offset, result}
// of the first n chunks of the last decode pass (24 bytes each, 5 per chunk).
int pgn_debug_decode_units(pgn_ctx* c, void* out, size_t nchunks)
{
    if (!c || !out) return PGN_ERR_INVALID_ARG;
    if (!c->lastUnits || nchunks > c->lastG) return PGN_ERR_INVALID_ARG;
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, c->lastUnits, nchunks * kStreams * sizeof(DecUnit), hipMemcpyDeviceToHost));
    return PGN_OK;
}

const char* pgn_ctx_kernels(pgn_ctx* c, int direction)
{
    if (!c) return "";
    if (direction == 0)
        return c->encStaged ? "enc_split_kernel + enc_zstd_kernel + enc_assemble_kernel" : "enc_chunk_kernel<C5>";
    if (!c->decStaged) return "dec_chunk_kernel<C5>";
    return c->lastDeferred ? "dec_parse_kernel + dec_zstd_kernel + dec_huf_kernel + dec_merge_kernel"
                           : "dec_parse_kernel + dec_zstd_kernel + dec_merge_kernel";
}

float pgn_ctx_last_encode_ms(pgn_ctx* c)
{
    if (!c || !c->encTimed) return -1.f;
    float ms = -1.f;
    if (hipEventSynchronize(c->ev[1]) != hipSuccess) return -1.f;
    if (hipEventElapsedTime(&ms, c->ev[0], c->ev[1]) != hipSuccess) return -1.f;
    return ms;
}
float pgn_ctx_last_decode_ms(pgn_ctx* c)
{
    if (!c || !c->decTimed) return -1.f;
    float ms = -1.f;
    if (hipEventSynchronize(c->ev[3]) != hipSuccess) return -1.f;
    if (hipEventElapsedTime(&ms, c->ev[2], c->ev[3]) != hipSuccess) return -1.f;
    return ms;
}

int pgn_synth_reads_device(pgn_ctx* c, size_t nreads, uint64_t seed, uint64_t first_read, uint64_t read_stride,
                           int16_t* d_samples,
                           const uint64_t* d_offsets, const uint32_t* d_counts, uint32_t pq, int32_t mean, int32_t lsd,
                           int32_t nsd, void* stream)
{
    if (!c || !d_samples || !d_offsets || !d_counts) return PGN_ERR_INVALID_ARG;
    if (nreads == 0) return PGN_OK;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    // task prefix sums (host-side scan over a device copy of the counts: simple and off the timed path)
    uint32_t* hc = (uint32_t*)malloc(4 * nreads);
    uint64_t* hs = (uint64_t*)malloc(8 * (nreads + 1));
    if (!hc || !hs) { free(hc); free(hs); return PGN_ERR_INVALID_ARG; }
    HIPCHK(hipMemcpyAsync(hc, d_counts, 4 * nreads, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    hs[0] = 0;
    for (size_t r = 0; r < nreads; r++) hs[r + 1] = hs[r] + (hc[r] + 63u) / 64u;
    uint64_t* dts = nullptr;
    HIPCHK(hipMallocAsync((void**)&dts, 8 * (nreads + 1), s));
    HIPCHK(hipMemcpyAsync(dts, hs, 8 * (nreads + 1), hipMemcpyHostToDevice, s));
    SynthArgs a{nreads, seed, first_read, read_stride ? read_stride : 1, d_samples, d_offsets, d_counts, pq, mean, lsd, nsd};
    uint64_t tasks = hs[nreads];
    unsigned grid = (unsigned)((tasks + 255) / 256);
    if (grid > 65536) grid = 65536;
    if (grid == 0) grid = 1;
    hipLaunchKernelGGL(synth_kernel, dim3(grid), dim3(256), 0, s, a, tasks, (const uint64_t*)dts);
    HIPCHK(hipGetLastError());
    HIPCHK(hipFreeAsync(dts, s));
    HIPCHK(hipStreamSynchronize(s));
    free(hc);
    free(hs);
    return PGN_OK;
}

// ---- host-memory per-chunk entry points (the plugin surface) --------------------------------
static int ensure_stage(pgn_ctx* c, size_t bytes)
{
    if (c->hstage && bytes <= c->stage.cap) return PGN_OK;
    const size_t b = align_up(bytes > c->stage.cap ? bytes : c->stage.cap, 1 << 20);
    const int rc = reserve(c, {{c->stage, b}});  // after its wait nothing uses the pinned mirror either
    if (rc) return rc;
    if (c->hstage) (void)hipHostFree(c->hstage);
    c->hstage = nullptr;
    uint8_t* h = nullptr;
    HIPCHK(hipHostMalloc((void**)&h, b, hipHostMallocDefault));
    const hipError_t e = hipHostGetDevicePointer((void**)&c->hstageDev, h, 0);
    if (e != hipSuccess) {
        (void)hipHostFree(h);
        return hip_fail(e, "hipHostGetDevicePointer");
    }
    c->hstage = h;
    return PGN_OK;
}

struct StageHdr {
    uint64_t off0, cnt0pad, outOff, outCap, outSize, inOff, inSize;
    uint32_t count;
    int32_t status;
    uint64_t stats[PGN_STATS_PER_CHUNK];
};

// One chunk from host memory: header and samples staged in the pinned mirror and uploaded in one
// copy; the kernels write the blob, its size, status and stats straight into the pinned mirror
// (no copies back: the call's tail is the kernels and one wait); the blob leaves it by memcpy.
static int compress_signal_one(int codec, pgn_ctx* c, const int16_t* samples, size_t n, uint8_t* dst, size_t cap,
                               size_t* out_size)
{
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(hipSetDevice(c->device));
    const size_t hdrB = 256, inB = align_up(2 * n + 16, 256);
    int rc = ensure_stage(c, hdrB + inB + cap + 64);
    if (rc) return rc;
    uint8_t* dh = c->stage;
    uint8_t* din = c->stage + hdrB;
    uint8_t* hout = c->hstageDev + hdrB + inB;  // the blob, written by the kernels into host memory
    StageHdr* hh = (StageHdr*)c->hstage;
    StageHdr* hd = (StageHdr*)c->hstageDev;     // the same header, the outputs written by the kernels
    *hh = StageHdr{};
    hh->outCap = cap;
    hh->count = (uint32_t)n;
    if (n) memcpy(c->hstage + hdrB, samples, 2 * n);
    HIPCHK(hipMemcpyAsync(dh, c->hstage, hdrB + 2 * n, hipMemcpyHostToDevice, c->stream));
    StageHdr* d = (StageHdr*)dh;
    const EncIO io{(const int16_t*)din, &d->off0, &d->count, hout, &d->outOff, &d->outCap, &hd->outSize, &hd->status, hd->stats};
    rc = launch_encode(c, codec, 1, io, c->stream, n ? (uint32_t)n : 1u, CallScope::kLocked);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    *out_size = (size_t)hh->outSize;
    if (hh->status != PGN_OK) return hh->status;
    memcpy(dst, c->hstage + hdrB + inB, (size_t)hh->outSize);
    return PGN_OK;
}

static int decompress_signal_one(int codec, pgn_ctx* c, const uint8_t* src, size_t len, int16_t* dst, size_t n)
{
    const size_t hdrB = 256, inB = align_up(len + 16, 256);
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(hipSetDevice(c->device));
    int rc = ensure_stage(c, hdrB + inB + 2 * n + 64);
    if (rc) return rc;
    uint8_t* dh = c->stage;
    uint8_t* din = c->stage + hdrB;
    int16_t* hout = (int16_t*)(c->hstageDev + hdrB + inB);  // the samples, written by the kernels into host memory
    StageHdr* hh = (StageHdr*)c->hstage;
    StageHdr* hd = (StageHdr*)c->hstageDev;
    *hh = StageHdr{};
    hh->inSize = len;
    hh->count = (uint32_t)n;
    if (len) memcpy(c->hstage + hdrB, src, len);
    HIPCHK(hipMemcpyAsync(dh, c->hstage, hdrB + len, hipMemcpyHostToDevice, c->stream));
    StageHdr* d = (StageHdr*)dh;
    const DecIO io{din, &d->inOff, &d->inSize, hout, &d->off0, &d->count, &hd->status};
    rc = launch_decode(c, codec, 1, io, c->stream, n ? (uint32_t)n : 1u, CallScope::kLocked);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    if (hh->status == PGN_ERR_UNSUPPORTED) {  // frames claiming more than the intermediate: the claims pass
        const uint8_t* bl = c->hstage + hdrB;
        const uint64_t ln = len;
        rc = claims_from_host(c, codec, 1, &hh->status, &hh->count, &bl, &ln, io, c->stream);
        if (rc) return rc;
    }
    if (hh->status != PGN_OK) return hh->status;
    if (n) memcpy(dst, c->hstage + hdrB + inB, 2 * n);
    return PGN_OK;
}

// An arena's per-request arrays (kPcHdr bytes at its start; index = the request's place in the
// batch order): the kernels read the device mirror's copy and write the results into pinned memory.
struct PcHdr {
    uint64_t off0[kPcMaxReqs];     // sample offset (elements): encode from the inputs, decode from the outputs
    uint32_t cnt[kPcMaxReqs];
    uint64_t outOff[kPcMaxReqs];   // encode: blob offset in the outputs
    uint64_t outCap[kPcMaxReqs];
    uint64_t inOff[kPcMaxReqs];    // decode: blob offset in the inputs
    uint64_t inSize[kPcMaxReqs];
    uint64_t outSize[kPcMaxReqs];  // results
    int32_t status[kPcMaxReqs];
    uint64_t stats[kPcMaxReqs * PGN_STATS_PER_CHUNK];
};
static_assert(sizeof(PcHdr) <= kPcHdr, "per-request arrays");

static int pc_init(pgn_ctx* c)
{
    HIPCHK(hipSetDevice(c->device));
    for (PcArena& A : c->pcA) {
        HIPCHK(hipHostMalloc((void**)&A.h, kPcHdr + kPcInCap + kPcOutCap, hipHostMallocDefault));
        HIPCHK(hipHostGetDevicePointer((void**)&A.hDev, A.h, 0));
        HIPCHK(hipMalloc(&A.d, kPcHdr + kPcInCap));
    }
    return PGN_OK;
}

// One arena's requests as one batch per (direction, codec) group, each group a batched launch over
// the arena's arrays; one upload, one wait.  Called by the leader without pcMu.
static void pc_run(pgn_ctx* c, PcArena& A)
{
    const int k = A.nreq;
    PcReq* ord[kPcMaxReqs];
    for (int i = 0; i < k; i++) ord[i] = A.reqs[i];
    std::stable_sort(ord, ord + k, [](const PcReq* x, const PcReq* y) {
        return x->dir * 16 + x->codec < y->dir * 16 + y->codec;
    });
    PcHdr* hh = (PcHdr*)A.h;
    for (int i = 0; i < k; i++) {
        const PcReq& r = *ord[i];
        hh->cnt[i] = r.n;
        hh->status[i] = -1;
        hh->outSize[i] = 0;
        if (r.dir == 0) {
            hh->off0[i] = r.inOff / 2;
            hh->outOff[i] = r.outOff;
            hh->outCap[i] = r.cap;
        } else {
            hh->off0[i] = r.outOff / 2;
            hh->inOff[i] = r.inOff;
            hh->inSize[i] = r.inBytes;
        }
    }
    const PcHdr* dh = (const PcHdr*)A.d;  // the device mirror of the arrays
    PcHdr* ho = (PcHdr*)A.hDev;           // results straight into pinned memory
    uint8_t* const inD = A.d + kPcHdr;
    uint8_t* const outH = A.hDev + kPcHdr + kPcInCap;
    // the arrays of the group of requests that starts at request i0
    const auto encIO = [&](int i0) {
        return EncIO{(const int16_t*)inD, dh->off0 + i0, dh->cnt + i0, outH, dh->outOff + i0, dh->outCap + i0,
                     ho->outSize + i0, ho->status + i0, ho->stats + (size_t)i0 * PGN_STATS_PER_CHUNK};
    };
    const auto decIO = [&](int i0) {
        return DecIO{inD, dh->inOff + i0, dh->inSize + i0, (int16_t*)outH, dh->off0 + i0, dh->cnt + i0, ho->status + i0};
    };
    int rc = PGN_OK;
    {
        std::lock_guard<std::mutex> g(c->mu);
        if (hipSetDevice(c->device) != hipSuccess ||
            hipMemcpyAsync(A.d, A.h, kPcHdr + A.inUsed, hipMemcpyHostToDevice, c->stream) != hipSuccess)
            rc = PGN_ERR_HIP;
        for (int i0 = 0; rc == PGN_OK && i0 < k;) {
            int i1 = i0;
            uint32_t maxN = 1;
            while (i1 < k && ord[i1]->dir == ord[i0]->dir && ord[i1]->codec == ord[i0]->codec) {
                maxN = ord[i1]->n > maxN ? ord[i1]->n : maxN;
                i1++;
            }
            const size_t m = (size_t)(i1 - i0);
            if (ord[i0]->dir == 0) rc = launch_encode(c, ord[i0]->codec, m, encIO(i0), c->stream, maxN, CallScope::kLocked);
            else rc = launch_decode(c, ord[i0]->codec, m, decIO(i0), c->stream, maxN, CallScope::kLocked);
            i0 = i1;
        }
        if (hipStreamSynchronize(c->stream) != hipSuccess && rc == PGN_OK) rc = PGN_ERR_HIP;
        // decode chunks whose frames claim more than the batch's intermediates: the claims pass
        for (int i0 = 0; rc == PGN_OK && i0 < k;) {
            int i1 = i0;
            while (i1 < k && ord[i1]->dir == ord[i0]->dir && ord[i1]->codec == ord[i0]->codec) i1++;
            if (ord[i0]->dir == 1) {
                const uint8_t* bl[kPcMaxReqs];
                uint64_t ln[kPcMaxReqs];
                for (int i = i0; i < i1; i++) {
                    bl[i - i0] = A.h + kPcHdr + ord[i]->inOff;
                    ln[i - i0] = ord[i]->inBytes;
                }
                rc = claims_from_host(c, ord[i0]->codec, (size_t)(i1 - i0), hh->status + i0, hh->cnt + i0, bl, ln, decIO(i0),
                                      c->stream);
            }
            i0 = i1;
        }
    }
    for (int i = 0; i < k; i++) {
        PcReq& r = *ord[i];
        r.rc = rc != PGN_OK ? rc : hh->status[i];
        r.outSize = hh->outSize[i];
    }
}

enum { kPcExclusive = 1000 };  // the call runs on its own (too large for an arena, or no arenas)

// A per-chunk host call through the arenas (see PcArena).  Returns the call's status, or
// kPcExclusive when it should run by itself.
static int pc_call(pgn_ctx* c, PcReq& r)
{
    const size_t inB = align_up(r.inBytes + 16, 256), outB = align_up(r.outBytes + 64, 256);
    if (inB > kPcInCap || outB > kPcOutCap) return kPcExclusive;
    std::unique_lock<std::mutex> lk(c->pcMu);
    if (c->pcReady == 0) c->pcReady = pc_init(c) == PGN_OK ? 1 : -1;
    if (c->pcReady < 0) return kPcExclusive;
    PcArena* A = nullptr;
    while (true) {  // join the open arena when it has room
        if (c->pcOpen >= 0) {
            PcArena& O = c->pcA[c->pcOpen];
            if (O.nreq < kPcMaxReqs && O.inUsed + inB <= kPcInCap && O.outUsed + outB <= kPcOutCap) {
                A = &O;
                break;
            }
        }
        c->pcCv.wait(lk);
    }
    const int ai = (int)(A - c->pcA);
    r.inOff = A->inUsed;
    r.outOff = A->outUsed;
    A->inUsed += inB;
    A->outUsed += outB;
    A->reqs[A->nreq++] = &r;
    A->unstaged++;
    r.done = false;
    lk.unlock();
    if (r.inBytes) memcpy(A->h + kPcHdr + r.inOff, r.in, r.inBytes);
    lk.lock();
    if (--A->unstaged == 0) c->pcCv.notify_all();
    while (!r.done) {
        if (!c->pcBusy && A->state == 0) {  // lead: run this arena (it holds this call)
            c->pcBusy = true;
            A->state = 1;
            PcArena& B = c->pcA[1 - ai];
            c->pcOpen = (B.state == 0 && B.nreq == 0) ? 1 - ai : -1;  // new calls fill the other arena
            c->pcCv.notify_all();
            while (A->unstaged) c->pcCv.wait(lk);
            lk.unlock();
            pc_run(c, *A);
            lk.lock();
            A->state = 2;
            A->readers = A->nreq;
            for (int i = 0; i < A->nreq; i++) A->reqs[i]->done = true;
            c->pcBusy = false;
            c->pcCv.notify_all();
        } else {
            c->pcCv.wait(lk);
        }
    }
    lk.unlock();
    const uint8_t* res = A->h + kPcHdr + kPcInCap + r.outOff;
    if (r.rc == PGN_OK) {
        if (r.dir == 0) memcpy(r.dst, res, (size_t)r.outSize);
        else if (r.n) memcpy(r.dst, res, 2 * (size_t)r.n);
    }
    lk.lock();
    if (--A->readers == 0) {  // the arena is idle again
        A->state = 0;
        A->nreq = 0;
        A->inUsed = A->outUsed = 0;
        if (c->pcOpen < 0) c->pcOpen = ai;
        c->pcCv.notify_all();
    }
    return r.rc;
}

// The blob bytes an encode call can need: its five frames (each at most ZSTD_COMPRESSBOUND of its
// stream, the streams together at most 3.75 n bytes; VBZ: one frame of ~2.13 n) and their prefixes.
static size_t pc_enc_out_bytes(size_t n, size_t cap)
{
    const size_t b = 4 * n + 4096;
    return cap < b ? cap : b;
}

static int compress_signal(int codec, pgn_ctx* c, const int16_t* samples, size_t n, uint8_t* dst, size_t cap,
                           size_t* out_size)
{
    if (!c || (!samples && n) || !dst || !out_size) return PGN_ERR_INVALID_ARG;
    if (n > PGN_MAX_CHUNK_SAMPLES) return PGN_ERR_UNSUPPORTED;
    PcReq r{};
    r.dir = 0;
    r.codec = codec;
    r.in = samples;
    r.inBytes = 2 * n;
    r.n = (uint32_t)n;
    r.dst = dst;
    r.cap = cap;
    r.outBytes = pc_enc_out_bytes(n, cap);
    const int rc = pc_call(c, r);
    if (rc == kPcExclusive) return compress_signal_one(codec, c, samples, n, dst, cap, out_size);
    *out_size = (size_t)r.outSize;
    return rc;
}

static int decompress_signal(int codec, pgn_ctx* c, const uint8_t* src, size_t len, int16_t* dst, size_t n)
{
    if (!c || (!src && len) || (!dst && n)) return PGN_ERR_INVALID_ARG;
    if (n > PGN_MAX_CHUNK_SAMPLES) return PGN_ERR_UNSUPPORTED;
    PcReq r{};
    r.dir = 1;
    r.codec = codec;
    r.in = src;
    r.inBytes = len;
    r.n = (uint32_t)n;
    r.dst = dst;
    r.outBytes = 2 * n;
    const int rc = pc_call(c, r);
    if (rc == kPcExclusive) return decompress_signal_one(codec, c, src, len, dst, n);
    return rc;
}

int pgn_compress_signal(pgn_ctx* c, const int16_t* samples, size_t n, uint8_t* dst, size_t cap, size_t* out_size)
{
    return compress_signal(kCodecC5, c, samples, n, dst, cap, out_size);
}

int pgn_decompress_signal(pgn_ctx* c, const uint8_t* src, size_t len, int16_t* dst, size_t n)
{
    return decompress_signal(kCodecC5, c, src, len, dst, n);
}

size_t pgn_vbz_compressed_signal_max_size(size_t n)
{
    return z1::compress_bound((size_t)svb_key_length((uint32_t)n) + 2 * n);
}

int pgn_vbz_compress_signal(pgn_ctx* c, const int16_t* samples, size_t n, uint8_t* dst, size_t cap, size_t* out_size)
{
    return compress_signal(kCodecVbz, c, samples, n, dst, cap, out_size);
}

int pgn_vbz_decompress_signal(pgn_ctx* c, const uint8_t* src, size_t len, int16_t* dst, size_t n)
{
    return decompress_signal(kCodecVbz, c, src, len, dst, n);
}

int pgn_variant_compress_signal(pgn_ctx* c, int variant, const int16_t* samples, size_t n, uint8_t* dst, size_t cap,
                                size_t* out_size)
{
    const int codec = variant_codec(variant);
    if (codec < 0) return PGN_ERR_INVALID_ARG;
    return compress_signal(codec, c, samples, n, dst, cap, out_size);
}

int pgn_variant_decompress_signal(pgn_ctx* c, int variant, const uint8_t* src, size_t len, int16_t* dst, size_t n)
{
    const int codec = variant_codec(variant);
    if (codec < 0) return PGN_ERR_INVALID_ARG;
    return decompress_signal(codec, c, src, len, dst, n);
}

static pgn_ctx* g_default = nullptr;
static std::mutex g_default_mu;

static int default_ctx(pgn_ctx** c)
{
    std::lock_guard<std::mutex> g(g_default_mu);
    if (!g_default) {
        const int rc = pgn_ctx_create(0, &g_default);
        if (rc) return rc;
    }
    *c = g_default;
    return PGN_OK;
}

// The pod5 C-API wrappers (c_api.cpp:1183-1253): compress into a buffer of the codec's maximum size,
// then check the caller's buffer ("Compressed signal size (..) is greater than provided buffer size").
static int capi_compress(int codec, const int16_t* signal, size_t signal_size, char* out, size_t* inout_size)
{
    if (!signal || !out || !inout_size) return PGN_ERR_INVALID_ARG;
    pgn_ctx* c = nullptr;
    int rc = default_ctx(&c);
    if (rc) return rc;
    // pgnano::compress_signal allocates compressed_signal_max_size(n) (pgnano.cpp:66-68), pod5's
    // VBZ compress_signal pod5::compressed_signal_max_size(n) (signal_compression.cpp:21-35) ...
    const size_t cap = codec == kCodecVbz ? pgn_vbz_compressed_signal_max_size(signal_size)
                                          : pgn_compressed_signal_max_size(signal_size);
    uint8_t* tmp = (uint8_t*)malloc(cap);
    if (!tmp) return PGN_ERR_INVALID_ARG;
    size_t sz = 0;
    rc = compress_signal(codec, c, signal, signal_size, tmp, cap, &sz);
    if (rc == PGN_OK) {
        // ... then c_api.cpp:1240-1250 checks the caller's buffer
        if (sz > *inout_size) {
            rc = PGN_ERR_DST_TOO_SMALL;
        } else {
            memcpy(out, tmp, sz);
            *inout_size = sz;
        }
    }
    free(tmp);
    return rc;
}

int pgn_pinanoraw_compress_signal(const int16_t* signal, size_t signal_size, char* out, size_t* inout_size)
{
    return capi_compress(kCodecC5, signal, signal_size, out, inout_size);
}

int pgn_pod5_vbz_compress_signal(const int16_t* signal, size_t signal_size, char* out, size_t* inout_size)
{
    return capi_compress(kCodecVbz, signal, signal_size, out, inout_size);
}

int pgn_pod5_vbz_decompress_signal(const char* compressed, size_t compressed_size, size_t sample_count, short* out)
{
    if (!compressed || !out) return PGN_ERR_INVALID_ARG;  // check_not_null / check_output_pointer_not_null
    pgn_ctx* c = nullptr;
    const int rc = default_ctx(&c);
    if (rc) return rc;
    return decompress_signal(kCodecVbz, c, (const uint8_t*)compressed, compressed_size, (int16_t*)out, sample_count);
}

}  // extern "C"
