// pgn_bam.h -- the kept reads as unaligned BAM records with the move table, raw or in BGZF blocks of stored deflate
// (include/pgnano_hip.h "BAM records", the rule of pgn_bam_records_device).  Byte copies, shifts, a nibble table and
// a CRC-32: the tolerance is zero.
//
// The lengths and the scan have the FASTQ call's shape (a thread per read, stitch::block_scan inside 1,024 reads,
// stitch_scan_kernel over the workgroups' totals, the offsets); the 64-way search, the uuid's characters and the
// quality clamp are pgn_fastq.h's.  The writer is flat over the stream and never gives a workgroup to a read: a
// workgroup owns kBlock = 65,280 stream bytes, one BGZF block's payload, which it builds as an image in LDS laid
// out at the destination's alignment (image byte i belongs at the payload's address rounded down to 16, plus i):
//   A. a thread per record puts the fixed fields, the name, the tags and the mv header, byte by byte,
//   B. a thread per 16-byte unit of the image fills SEQ, QUAL and the moves: a unit wholly inside one of them is
//      two 16-byte loads and a 2-to-1 nibble gather, or one load and a clamp, or one load and a shift, and one
//      16-byte LDS store; any other unit goes byte by byte (a record is at least 75 bytes, so it meets at most two).
//      Every unit goes through the image in either layout: storing B's whole units straight from registers where
//      no checksum needs them was measured and is no faster (profiles/bam_timing.log),
//   C. with PGN_BAM_BGZF the CRC-32 of the image's payload, then the image leaves as aligned 16-byte stores (byte
//      by byte only in front of the payload's first and behind its last 16-byte address) with the block's 23 bytes
//      in front and 8 behind.
// The CRC: lane t of the 1,024 checksums the kSlice = 68 bytes that end 68 * (1023 - t) bytes in front of the
// payload's end (17 dwords: a stride that is odd in banks, so ds_read_b32 meets no conflict), by four tables of 256
// from LDS, then multiplies by x^(8 * 68 * (1023 - t)) mod P, a constant per lane, carry-less in 32 steps; the
// products' exclusive-or is the block's CRC (zlib's crc32_combine, whose conditioning cancels).  Slices are counted
// from the end so that only one of them is short, whatever the payload's length.
// bgzf_crc_kernel is the other placement, kept for the measurement (PGN_BAM_CRC=split): the writer stores the
// payloads and this kernel reads each back into an image, checksums it the same way and writes the 31 bytes.
#ifndef PGN_BAM_H
#define PGN_BAM_H

#include "pgn_fastq.h"

namespace pgn {
namespace bam {

constexpr uint32_t kThreads = 1024;
constexpr uint32_t kBlock = PGN_BGZF_BLOCK_BYTES;  // stream bytes of one workgroup of the writer
constexpr uint32_t kHead = 23, kTail = 8;          // a BGZF block's bytes in front of and behind its payload
constexpr uint32_t kFile = kBlock + kHead + kTail; // 65,311
constexpr uint32_t kImage = kBlock + 32;           // the payload behind up to 15 bytes, and a dword to read beyond
constexpr uint32_t kUnits = (kBlock + 15 + 15) / 16;
constexpr uint32_t kRounds = (kUnits + kThreads - 1) / kThreads;
constexpr uint32_t kMaxTags = PGN_BAM_MAX_TAGS;
constexpr uint32_t kFront = 73;                    // block_size, the fixed fields and the name
constexpr uint32_t kNameAt = 36;
constexpr uint32_t kTagBytes = 7, kMvHead = 9;
constexpr uint32_t kSlice = 68;                    // bytes one lane checksums
constexpr uint32_t kScanThreads = stitch::kPlanThreads;
constexpr uint32_t kPoly = 0xEDB88320u;
static_assert(kSlice % 4 == 0 && (kSlice / 4) % 2 == 1, "an odd number of dwords per lane");
static_assert(kSlice * kThreads >= kBlock, "the lanes' slices cover a block");
static_assert(sizeof(pgn_bam_params) == sizeof(pgn_fastq_params) + 8, "the tag columns are the FASTQ struct's");

// PGN_ERR_INVALID_ARG conditions of the parameters, in the header's order
inline bool params_valid(const pgn_bam_params* P)
{
    if (!P) return false;
    if (P->flags & ~(uint32_t)(PGN_BAM_REVERSE | PGN_BAM_MOVES | PGN_BAM_BGZF)) return false;
    pgn_fastq_params f{};
    f.ntags = P->ntags;
    memcpy(f.tag_name, P->tag_name, sizeof(f.tag_name));
    if (!fastq::params_valid(&f)) return false;
    if ((P->flags & PGN_BAM_MOVES) && (P->stride < 1 || P->stride > 127)) return false;
    return true;
}

// the largest S with S + 31 * ceil(S / kBlock) <= byte_capacity
inline uint64_t bgzf_stream_capacity(uint64_t byte_capacity)
{
    const uint64_t q = byte_capacity / kFile, rem = byte_capacity % kFile;
    return q * kBlock + (rem > kHead + kTail ? rem - (kHead + kTail) : 0);
}

// a * b mod P in the reflected representation (bit 31 is x^0)
PGN_HD constexpr uint32_t mulmod(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int i = 0; i < 32; i++) {
        p ^= (a & 0x80000000u) ? b : 0u;
        a <<= 1;
        b = (b >> 1) ^ ((b & 1u) ? kPoly : 0u);
    }
    return p;
}

struct CrcConst {
    uint32_t t[4][256];        // slicing by four
    uint32_t shift[kThreads];  // x^(8 * kSlice * j) mod P
};

constexpr CrcConst make_crc_const()
{
    CrcConst c{};
    for (uint32_t i = 0; i < 256; i++) {
        uint32_t v = i;
        for (int k = 0; k < 8; k++) v = (v >> 1) ^ ((v & 1u) ? kPoly : 0u);
        c.t[0][i] = v;
    }
    for (uint32_t k = 1; k < 4; k++)
        for (uint32_t i = 0; i < 256; i++) c.t[k][i] = (c.t[k - 1][i] >> 8) ^ c.t[0][c.t[k - 1][i] & 0xFFu];
    uint32_t x = 0x80000000u;  // x^0
    for (uint32_t i = 0; i < 8 * kSlice; i++) x = (x >> 1) ^ ((x & 1u) ? kPoly : 0u);
    c.shift[0] = 0x80000000u;
    for (uint32_t j = 1; j < kThreads; j++) c.shift[j] = mulmod(c.shift[j - 1], x);
    return c;
}

#ifndef PGN_SELECT_HOST_ONLY
using Vec16 = ctc::Vec16;

__device__ const CrcConst kCrc = make_crc_const();

struct Args {
    uint64_t nreads;             // >= 1
    const uint8_t* ids;          // 16 per read
    const uint64_t* readBases;   // nreads + 1
    const int32_t* status;
    const uint8_t* keep;         // may be null
    const uint8_t* seq;
    const uint8_t* qual;         // may be null: 0xFF
    uint64_t baseCapacity;
    const uint64_t* readFrames;  // nreads + 1, with moves
    const uint8_t* codes;
    uint64_t frameBase, frameCapacity;
    uint8_t* out;
    uint64_t streamCapacity;     // byte_capacity, or what it holds in BGZF blocks
    uint64_t* recOff;            // nreads + 1: the lengths between the count and the offset kernel, then the scan
    int32_t* recStatus;
    uint64_t* written;           // W and the file bytes
    uint64_t* blockSums;         // context scratch: one per workgroup of the count kernel and their total
    uint64_t nblocks;
    uint64_t ntiles;             // of the writer
    uint32_t crcSplit;           // the CRC and the blocks' 31 bytes are bgzf_crc_kernel's
    pgn_bam_params prm;
};

// length of read r's record, 0 for a read that is not kept, whose status goes to st
__device__ __forceinline__ uint64_t record_length(const Args& a, uint64_t r, int32_t& st)
{
    const uint64_t b0 = a.readBases[r], b1 = a.readBases[r + 1];
    st = a.status[r];
    if (st != PGN_OK || b1 <= b0 || b1 > a.baseCapacity) return 0;
    if (a.keep && !a.keep[r]) return 0;
    const uint64_t m = b1 - b0;
    uint64_t len = kFront + (m + 1) / 2 + m + kTagBytes * a.prm.ntags;
    if (a.prm.flags & PGN_BAM_MOVES) {
        const uint64_t f0 = a.readFrames[r], f1 = a.readFrames[r + 1];
        if (f0 < a.frameBase || f1 < f0 || f1 - a.frameBase > a.frameCapacity || (f1 - f0) >> 31) {
            st = PGN_ERR_INVALID_ARG;
            return 0;
        }
        len += kMvHead + (f1 - f0);
    }
    return len;
}

__global__ __launch_bounds__(kScanThreads) void bam_len_kernel(Args a)
{
    __shared__ uint64_t waveSum[kScanThreads / 64];
    const uint64_t r = (uint64_t)blockIdx.x * kScanThreads + threadIdx.x;
    uint64_t len = 0;
    if (r < a.nreads) {
        int32_t st;
        len = record_length(a, r, st);
        a.recOff[r] = len;
        a.recStatus[r] = st;  // of a read without a record; the offset kernel writes the others'
    }
    uint64_t before;
    const uint64_t all = stitch::block_scan(len, waveSum, before);
    if (threadIdx.x == 0) a.blockSums[blockIdx.x] = all;
}

// rec_off of every read and rec_status of every record behind the scan of the workgroups' totals, and W: the
// largest rec_off value that the stream capacity admits, which exactly one thread finds
__global__ __launch_bounds__(kScanThreads) void bam_offset_kernel(Args a)
{
    __shared__ uint64_t waveSum[kScanThreads / 64];
    const uint64_t r = (uint64_t)blockIdx.x * kScanThreads + threadIdx.x;
    const uint64_t len = r < a.nreads ? a.recOff[r] : 0;
    uint64_t before;
    stitch::block_scan(len, waveSum, before);
    if (r >= a.nreads) return;
    const uint64_t off = a.blockSums[blockIdx.x] + before, end = off + len, S = a.streamCapacity;
    a.recOff[r] = off;
    if (len) a.recStatus[r] = end > S ? PGN_ERR_DST_TOO_SMALL : PGN_OK;
    uint64_t W = ~0ull;
    if (len && off <= S && end > S) W = off;
    if (r + 1 == a.nreads) {
        a.recOff[a.nreads] = end;
        if (end <= S) W = end;
    }
    if (W != ~0ull) {
        a.written[0] = W;
        a.written[1] = (a.prm.flags & PGN_BAM_BGZF) ? W + (kHead + kTail) * ((W + kBlock - 1) / kBlock) : W;
    }
}

// The CRC-32 of the n payload bytes at image + mis, by the whole workgroup of kThreads; T is kCrc.t in LDS and red
// sixteen words.  Every thread returns it.  n <= kBlock.
__device__ __forceinline__ uint32_t block_crc(const uint8_t* image, uint32_t mis, uint32_t n, const uint32_t (*T)[256],
                                              uint32_t* red)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t behind = kThreads - 1 - tid;  // whole slices behind this one
    const int32_t end = (int32_t)n - (int32_t)(kSlice * behind), beg = end - (int32_t)kSlice;
    uint32_t c = 0;
    if (end > 0) {
        c = 0xFFFFFFFFu;
        if (beg >= 0) {
            const uint32_t s = mis + (uint32_t)beg;
            const uint32_t* w = reinterpret_cast<const uint32_t*>(image) + (s >> 2);
            uint32_t lo = w[0];
#pragma unroll
            for (uint32_t j = 0; j < kSlice / 4; j++) {
                const uint32_t hi = w[j + 1];
                c ^= __builtin_amdgcn_alignbyte(hi, lo, s & 3u);
                c = T[3][c & 0xFFu] ^ T[2][(c >> 8) & 0xFFu] ^ T[1][(c >> 16) & 0xFFu] ^ T[0][c >> 24];
                lo = hi;
            }
        } else {
            for (int32_t i = 0; i < end; i++) c = T[0][(c ^ image[mis + i]) & 0xFFu] ^ (c >> 8);
        }
        c = mulmod(~c, kCrc.shift[behind]);
    }
#pragma unroll
    for (uint32_t off = 32; off; off >>= 1) c ^= __shfl_xor(c, off);
    if (lane == 0) red[tid >> 6] = c;
    __syncthreads();
    c = 0;
#pragma unroll
    for (uint32_t k = 0; k < kThreads / 64; k++) c ^= red[k];
    return c;
}

// the 23 bytes in front of and the 8 behind a block's payload of n bytes at dst, by threads 0..22 and 32..39
__device__ __forceinline__ void block_frame(uint8_t* dst, uint32_t n, uint32_t crc)
{
    const uint32_t tid = threadIdx.x;
    if (tid < kHead) {
        const uint64_t h0 = 0x0000000004088B1Full;  // 1f 8b 08 04 00 00 00 00
        const uint64_t h1 = 0x000243420006FF00ull;  // 00 ff 06 00 42 43 02 00
        const uint32_t bsize = n + 30, nn = ~n & 0xFFFFu;
        uint32_t b;
        if (tid < 8)
            b = (uint32_t)(h0 >> (8 * tid));
        else if (tid < 16)
            b = (uint32_t)(h1 >> (8 * (tid - 8)));
        else if (tid < 18)
            b = bsize >> (8 * (tid - 16));
        else if (tid == 18)
            b = 1;
        else if (tid < 21)
            b = n >> (8 * (tid - 19));
        else
            b = nn >> (8 * (tid - 21));
        dst[(int32_t)tid - (int32_t)kHead] = (uint8_t)b;
    } else if (tid >= 32 && tid < 32 + kTail) {
        const uint32_t k = tid - 32;
        dst[n + k] = (uint8_t)((k < 4 ? crc : n) >> (8 * (k & 3u)));
    }
}

// nibble of a base character: its place in "=ACMGRSVTWYHKDBN" whatever its case, 15 for any other byte
__device__ __forceinline__ uint32_t base_nibble(uint32_t ch)
{
    const char code[17] = "=ACMGRSVTWYHKDBN";
    const uint32_t up = ch >= 'a' && ch <= 'z' ? ch - 32u : ch;
    uint32_t nib = 15;
#pragma unroll
    for (uint32_t k = 0; k < 16; k++)
        if (up == (uint32_t)code[k]) nib = k;
    return nib;
}

__device__ __forceinline__ uint32_t qual_byte(uint32_t q) { return fastq::err_index(q); }

// What the writer knows of the record that holds a stream byte
struct Rec {
    uint64_t off, end;  // its stream bytes [off, end)
    uint64_t b0, m;     // its bases
    uint64_t sl;        // packed SEQ bytes
    uint64_t c0;        // index in codes of its first frame
    uint64_t mv0;       // offset in the record of its first move; the record's length without moves
};

__device__ __forceinline__ Rec load_rec(const Args& a, uint64_t r)
{
    Rec R;
    R.off = a.recOff[r];
    R.end = a.recOff[r + 1];
    R.b0 = a.readBases[r];
    R.m = a.readBases[r + 1] - R.b0;
    R.sl = (R.m + 1) / 2;
    R.mv0 = kFront + R.sl + R.m + kTagBytes * a.prm.ntags;
    R.c0 = 0;
    if (a.prm.flags & PGN_BAM_MOVES) {
        R.mv0 += kMvHead;
        R.c0 = a.readFrames[r] - a.frameBase;
    }
    return R;
}

// the last r in [lo, hi] with rec_off[r] <= o
__device__ __forceinline__ uint64_t record_of(const uint64_t* recOff, uint64_t lo, uint64_t hi, uint64_t o)
{
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (recOff[mid] <= o)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(kThreads) void bam_write_kernel(Args a)
{
    __shared__ __attribute__((aligned(16))) uint8_t image[kImage];
    __shared__ uint32_t crcT[4][256];
    __shared__ uint8_t nib[256];
    __shared__ uint32_t red[kThreads / 64];
    __shared__ uint64_t edge[2];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const bool reverse = (a.prm.flags & PGN_BAM_REVERSE) != 0, moves = (a.prm.flags & PGN_BAM_MOVES) != 0;
    const bool bgzf = (a.prm.flags & PGN_BAM_BGZF) != 0;
    const uint64_t W = a.written[0];
    if (tid < 256) nib[tid] = (uint8_t)base_nibble(tid);
    (&crcT[0][0])[tid] = (&kCrc.t[0][0])[tid];
    static_assert(kThreads == 4 * 256, "a table entry per thread");
    for (uint64_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        const uint64_t olo = t * kBlock;
        if (olo >= W) return;  // the whole workgroup: this tile and all behind it hold no record
        const uint32_t n = (uint32_t)(W - olo < kBlock ? W - olo : kBlock);
        const uint64_t ohi = olo + n;
        uint8_t* const dst = bgzf ? a.out + t * kFile + kHead : a.out + olo;  // of the tile's first stream byte
        const uint32_t mis = (uint32_t)((uintptr_t)dst & 15u);
        // its first and last record: the last r with rec_off[r] <= olo, which holds that byte, and the same for ohi - 1
        if (wave == 0) {
            const uint64_t r = fastq::wave_first_above(a.recOff, a.nreads + 1, olo);
            if (lane == 0) edge[0] = r - 1;
        } else if (wave == 1) {
            const uint64_t r = fastq::wave_first_above(a.recOff, a.nreads + 1, ohi - 1);
            if (lane == 0) edge[1] = r - 1;
        }
        __syncthreads();
        const uint64_t rFirst = edge[0], rLast = edge[1];

        // A. fixed fields, names, tags and mv headers, a thread per record
        for (uint64_t r = rFirst + tid; r <= rLast; r += kThreads) {
            const Rec R = load_rec(a, r);
            if (R.end == R.off) continue;
            auto put = [&](uint64_t o, uint32_t b) {
                if (o >= olo && o < ohi) image[mis + (uint32_t)(o - olo)] = (uint8_t)b;
            };
            auto put32 = [&](uint64_t o, uint32_t v) {
#pragma unroll
                for (uint32_t k = 0; k < 4; k++) put(o + k, v >> (8 * k));
            };
            if (R.off + kFront > olo && R.off < ohi) {
                put32(R.off, (uint32_t)(R.end - R.off - 4));
                put32(R.off + 4, 0xFFFFFFFFu);    // refID
                put32(R.off + 8, 0xFFFFFFFFu);    // pos
                put32(R.off + 12, 0x12480025u);   // l_read_name 37, mapq 0, bin 4680
                put32(R.off + 16, 0x00040000u);   // n_cigar_op 0, flag 4
                put32(R.off + 20, (uint32_t)R.m); // l_seq
                put32(R.off + 24, 0xFFFFFFFFu);   // next_refID
                put32(R.off + 28, 0xFFFFFFFFu);   // next_pos
                put32(R.off + 32, 0u);            // tlen
                const uint8_t* id = a.ids + 16 * r;
                for (uint32_t q = 0; q < fastq::kUuidChars; q++) put(R.off + kNameAt + q, fastq::uuid_char(id, q));
                put(R.off + kNameAt + fastq::kUuidChars, 0);
            }
            const uint64_t tagAt = R.off + kFront + R.sl + R.m;
            if (tagAt + kTagBytes * kMaxTags + kMvHead > olo && tagAt < ohi) {
#pragma unroll
                for (uint32_t k = 0; k < kMaxTags; k++) {
                    if (k < a.prm.ntags) {
                        const uint64_t o = tagAt + kTagBytes * k;
                        put(o, a.prm.tag_name[k][0]);
                        put(o + 1, a.prm.tag_name[k][1]);
                        put(o + 2, 'I');
                        put32(o + 3, a.prm.d_tag[k][r]);
                    }
                }
                if (moves) {
                    const uint64_t o = R.off + R.mv0 - kMvHead;
                    put32(o, 0x6342766Du);  // 'm' 'v' 'B' 'c'
                    put32(o + 4, (uint32_t)(1 + (R.end - R.off - R.mv0)));
                    put(o + 8, a.prm.stride);
                }
            }
        }

        // B. SEQ, QUAL and the moves, a thread per 16-byte unit of the image
#pragma unroll 1
        for (uint32_t j = 0; j < kRounds; j++) {
            const uint32_t u = j * kThreads + tid;
            const uint32_t ia = 16u * u > mis ? 16u * u : mis, ib = 16u * u + 16u < mis + n ? 16u * u + 16u : mis + n;
            if (u >= kUnits || ia >= ib) continue;
            const uint64_t oa = olo + (ia - mis), ob = olo + (ib - mis);  // stream bytes [oa, ob)
            uint64_t r = record_of(a.recOff, rFirst, rLast, oa);
            Rec R = load_rec(a, r);
            if (ib - ia == 16 && ob <= R.end) {
                const uint64_t p = oa - R.off;
                Vec16 v;
                bool done = false;
                if (p >= kFront && p + 16 <= kFront + R.sl && 2 * (p - kFront) + 32 <= R.m) {
                    const uint64_t g = 2 * (p - kFront);  // the unit's first base
                    const uint8_t* src = a.seq + R.b0 + (reverse ? R.m - 32 - g : g);
                    Vec16 s0 = stitch::load16(src), s1 = stitch::load16(src + 16);
                    if (reverse) {
                        const Vec16 x = fastq::reversed(s1);
                        s1 = fastq::reversed(s0);
                        s0 = x;
                    }
#pragma unroll
                    for (uint32_t k = 0; k < 4; k++) {
                        const uint32_t w0 = k < 2 ? s0[2 * k] : s1[2 * k - 4], w1 = k < 2 ? s0[2 * k + 1] : s1[2 * k - 3];
                        const uint32_t o0 = nib[w0 & 0xFFu] << 4 | nib[(w0 >> 8) & 0xFFu];
                        const uint32_t o1 = nib[(w0 >> 16) & 0xFFu] << 4 | nib[w0 >> 24];
                        const uint32_t o2 = nib[w1 & 0xFFu] << 4 | nib[(w1 >> 8) & 0xFFu];
                        const uint32_t o3 = nib[(w1 >> 16) & 0xFFu] << 4 | nib[w1 >> 24];
                        v[k] = o0 | o1 << 8 | o2 << 16 | o3 << 24;
                    }
                    done = true;
                } else if (p >= kFront + R.sl && p + 16 <= kFront + R.sl + R.m) {
                    if (a.qual) {
                        const uint64_t g = p - kFront - R.sl;
                        const Vec16 s = stitch::load16(a.qual + R.b0 + (reverse ? R.m - 16 - g : g));
                        const Vec16 q = reverse ? fastq::reversed(s) : s;
#pragma unroll
                        for (uint32_t k = 0; k < 4; k++)
                            v[k] = qual_byte(q[k] & 0xFFu) | qual_byte((q[k] >> 8) & 0xFFu) << 8 |
                                   qual_byte((q[k] >> 16) & 0xFFu) << 16 | qual_byte(q[k] >> 24) << 24;
                    } else {
                        v = Vec16{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
                    }
                    done = true;
                } else if (moves && p >= R.mv0) {
                    const Vec16 s = stitch::load16(a.codes + R.c0 + (p - R.mv0));
#pragma unroll
                    for (uint32_t k = 0; k < 4; k++) v[k] = (s[k] >> 7) & 0x01010101u;
                    done = true;
                }
                if (done) {
                    *reinterpret_cast<Vec16*>(image + 16u * u) = v;
                    continue;
                }
            }
            for (uint64_t o = oa; o < ob; o++) {
                if (o >= R.end) {  // the next record with bytes: a run of reads without a record may lie between
                    r = record_of(a.recOff, r + 1, rLast, o);
                    R = load_rec(a, r);
                }
                uint64_t q = o - R.off;
                if (q < kFront) continue;
                q -= kFront;
                uint32_t b;
                if (q < R.sl) {
                    const uint64_t g = 2 * q;
                    b = nib[a.seq[R.b0 + (reverse ? R.m - 1 - g : g)]] << 4;
                    if (g + 1 < R.m) b |= nib[a.seq[R.b0 + (reverse ? R.m - 2 - g : g + 1)]];
                } else if (q < R.sl + R.m) {
                    const uint64_t g = q - R.sl;
                    b = a.qual ? qual_byte(a.qual[R.b0 + (reverse ? R.m - 1 - g : g)]) : 0xFFu;
                } else if (moves && q + kFront >= R.mv0) {
                    b = (a.codes[R.c0 + (q + kFront - R.mv0)] >> 7) & 1u;
                } else {
                    continue;  // tags and the mv header
                }
                image[mis + (uint32_t)(o - olo)] = (uint8_t)b;
            }
        }
        __syncthreads();

        // C. the checksum, the image's units and the block's frame to the output
        if (bgzf && !a.crcSplit) {
            const uint32_t crc = block_crc(image, mis, n, crcT, red);
            block_frame(dst, n, crc);
        }
        uint8_t* const dstA = dst - mis;
#pragma unroll 1
        for (uint32_t j = 0; j < kRounds; j++) {
            const uint32_t u = j * kThreads + tid;
            const uint32_t ia = 16u * u > mis ? 16u * u : mis, ib = 16u * u + 16u < mis + n ? 16u * u + 16u : mis + n;
            if (u >= kUnits || ia >= ib) continue;
            if (ib - ia == 16)
                *reinterpret_cast<Vec16*>(dstA + 16u * u) = *reinterpret_cast<const Vec16*>(image + 16u * u);
            else
                for (uint32_t i = ia; i < ib; i++) dstA[i] = image[i];
        }
        __syncthreads();  // the next tile writes the image, the edges and red
    }
}

// The other placement of the CRC: a workgroup reads a stored payload back, checksums it and writes the 31 bytes.
__global__ __launch_bounds__(kThreads) void bgzf_crc_kernel(Args a)
{
    __shared__ __attribute__((aligned(16))) uint8_t image[kImage];
    __shared__ uint32_t crcT[4][256];
    __shared__ uint32_t red[kThreads / 64];
    const uint32_t tid = threadIdx.x;
    const uint64_t W = a.written[0];
    (&crcT[0][0])[tid] = (&kCrc.t[0][0])[tid];
    for (uint64_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        const uint64_t olo = t * kBlock;
        if (olo >= W) return;
        const uint32_t n = (uint32_t)(W - olo < kBlock ? W - olo : kBlock);
        uint8_t* const dst = a.out + t * kFile + kHead;
        const uint32_t mis = (uint32_t)((uintptr_t)dst & 15u);
        const uint8_t* const dstA = dst - mis;
#pragma unroll 1
        for (uint32_t j = 0; j < kRounds; j++) {
            const uint32_t u = j * kThreads + tid;
            const uint32_t ia = 16u * u > mis ? 16u * u : mis, ib = 16u * u + 16u < mis + n ? 16u * u + 16u : mis + n;
            if (u >= kUnits || ia >= ib) continue;
            if (ib - ia == 16)
                *reinterpret_cast<Vec16*>(image + 16u * u) = *reinterpret_cast<const Vec16*>(dstA + 16u * u);
            else
                for (uint32_t i = ia; i < ib; i++) image[i] = dstA[i];
        }
        __syncthreads();
        const uint32_t crc = block_crc(image, mis, n, crcT, red);
        block_frame(dst, n, crc);
        __syncthreads();
    }
}
#endif  // PGN_SELECT_HOST_ONLY

}  // namespace bam
}  // namespace pgn

#endif  // PGN_BAM_H
