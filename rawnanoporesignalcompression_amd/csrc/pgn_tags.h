// pgn_tags.h -- typed tag columns of the two record writers (include/pgnano_hip.h "Typed record tags", the rule of
// pgn_bam_records_tagged_device and pgn_fastq_records_tagged_device): uint32, int32 and float values, a string per
// read from a dictionary or from a pool.  Byte copies, comparisons and a decimal: the tolerance is zero.
//
// The calls are the old ones with another source of tag bytes.  The length kernels here take the old record length
// with no tags and add the columns' bytes, a thread per read; a thread validates each span its read uses (offsets
// first, so that no byte outside the pool is read, then at most 255 bytes), and a read with an invalid span has no
// record and PGN_ERR_INVALID_ARG.  The scans and the offset kernels are the old ones.  The writers are the old
// writers with one step changed: step A's thread per record walks the columns and puts their bytes behind the tile
// guard it already has.  The tag area's length is not carried: it is what the record's length in rec_off leaves, so
// the calls need no scratch per read.  A span that the length kernel accepted is read again by the writer; the
// buffers do not change between the two, so the writer meets no invalid span.
#ifndef PGN_TAGS_H
#define PGN_TAGS_H

#include "pgn_bam.h"

namespace pgn {
namespace tags {

constexpr uint32_t kMaxCols = PGN_REC_MAX_TAGS;
constexpr uint32_t kMaxString = PGN_TAG_MAX_STRING;
static_assert(sizeof(pgn_tag_column) == 40 && sizeof(pgn_record_tags) == 8 + 16 * 40, "the header's layout");

// PGN_ERR_INVALID_ARG conditions of the columns, in the header's order: the count, the names and the types, then
// with `fastq` a float column
inline bool columns_valid(const pgn_record_tags* T, bool fastq)
{
    if (T->ncols > kMaxCols) return false;
    for (uint32_t k = 0; k < T->ncols; k++) {
        const uint8_t a = T->col[k].name[0], b = T->col[k].name[1];
        const bool alpha0 = (a >= 'A' && a <= 'Z') || (a >= 'a' && a <= 'z');
        const bool alnum1 = (b >= 'A' && b <= 'Z') || (b >= 'a' && b <= 'z') || (b >= '0' && b <= '9');
        if (!alpha0 || !alnum1 || T->col[k].type > PGN_TAG_STR) return false;
    }
    if (fastq)
        for (uint32_t k = 0; k < T->ncols; k++)
            if (T->col[k].type == PGN_TAG_F32) return false;
    return true;
}

// ... and of their pointers, behind nreads >= 2^32
inline bool pointers_valid(const pgn_record_tags* T, size_t nreads)
{
    for (uint32_t k = 0; k < T->ncols; k++)
        if (T->col[k].str_capacity >> 32) return false;
    if (nreads)
        for (uint32_t k = 0; k < T->ncols; k++) {
            const pgn_tag_column& c = T->col[k];
            if (c.type <= PGN_TAG_DICT && !c.d_values) return false;
            if ((c.type == PGN_TAG_STR || (c.type == PGN_TAG_DICT && c.nstrings > 0)) && !c.d_str_off) return false;
        }
    for (uint32_t k = 0; k < T->ncols; k++)
        if (T->col[k].str_capacity && !T->col[k].d_strings) return false;
    return true;
}

#ifndef PGN_SELECT_HOST_ONLY
// The span of a string column for read r: false iff its offsets are invalid.  present: the column has a value.
__device__ __forceinline__ bool span_of(const pgn_tag_column& c, uint64_t r, uint32_t& at, uint32_t& n, bool& present)
{
    uint64_t i = r;
    present = true;
    at = n = 0;
    if (c.type == PGN_TAG_DICT) {
        i = static_cast<const uint32_t*>(c.d_values)[r];
        if (i >= c.nstrings) {
            present = false;
            return true;
        }
    }
    const uint32_t a = c.d_str_off[i], b = c.d_str_off[i + 1];
    if (a > b || b > c.str_capacity || b - a > kMaxString) return false;
    at = a;
    n = b - a;
    return true;
}

struct Cols {
    pgn_record_tags t;

    // The bytes that read r's columns add to its record, in BAM or as text; false iff a span is invalid.
    __device__ __forceinline__ bool length(uint64_t r, bool bam, uint64_t& len) const
    {
        len = 0;
        bool ok = true;
        for (uint32_t k = 0; k < t.ncols; k++) {
            const pgn_tag_column& c = t.col[k];
            if (c.type <= PGN_TAG_F32) {
                if (bam) {
                    len += 7;
                } else {
                    const uint32_t v = static_cast<const uint32_t*>(c.d_values)[r];
                    const bool neg = c.type == PGN_TAG_I32 && (v >> 31);
                    len += 6u + neg + fastq::digits10(neg ? 0u - v : v);
                }
                continue;
            }
            uint32_t at, n;
            bool present;
            if (!span_of(c, r, at, n, present)) {
                ok = false;
                continue;
            }
            if (!present) continue;
            for (uint32_t i = 0; i < n; i++) {
                const uint32_t ch = c.d_strings[at + i];
                ok = ok && ch >= 0x20u && ch <= 0x7Eu;
            }
            len += (bam ? 4u : 6u) + n;
        }
        return ok;
    }

    // Read r's columns as BAM tags from stream byte o on, through the writer's guarded put(o, byte).
    template <class Put>
    __device__ __forceinline__ void put_bam(uint64_t r, uint64_t o, Put& put) const
    {
        for (uint32_t k = 0; k < t.ncols; k++) {
            const pgn_tag_column& c = t.col[k];
            if (c.type <= PGN_TAG_F32) {
                const uint32_t v = static_cast<const uint32_t*>(c.d_values)[r];
                put(o, c.name[0]);
                put(o + 1, c.name[1]);
                put(o + 2, c.type == PGN_TAG_U32 ? 'I' : c.type == PGN_TAG_I32 ? 'i' : 'f');
#pragma unroll
                for (uint32_t j = 0; j < 4; j++) put(o + 3 + j, v >> (8 * j));
                o += 7;
                continue;
            }
            uint32_t at, n;
            bool present;
            if (!span_of(c, r, at, n, present) || !present) continue;
            put(o, c.name[0]);
            put(o + 1, c.name[1]);
            put(o + 2, 'Z');
            for (uint32_t i = 0; i < n; i++) put(o + 3 + i, c.d_strings[at + i]);
            put(o + 3 + n, 0);
            o += 4u + n;
        }
    }

    // ... and as text behind the uuid; returns the position behind them.
    template <class Put>
    __device__ __forceinline__ uint64_t put_fastq(uint64_t r, uint64_t o, Put& put) const
    {
        for (uint32_t k = 0; k < t.ncols; k++) {
            const pgn_tag_column& c = t.col[k];
            uint32_t at = 0, n = 0, v = 0;
            bool present = true, neg = false;
            if (c.type <= PGN_TAG_F32) {
                v = static_cast<const uint32_t*>(c.d_values)[r];
                neg = c.type == PGN_TAG_I32 && (v >> 31);
                v = neg ? 0u - v : v;
            } else if (!span_of(c, r, at, n, present) || !present) {
                continue;
            }
            put(o, '\t');
            put(o + 1, c.name[0]);
            put(o + 2, c.name[1]);
            put(o + 3, ':');
            put(o + 4, c.type <= PGN_TAG_F32 ? 'i' : 'Z');
            put(o + 5, ':');
            o += 6;
            if (c.type <= PGN_TAG_F32) {
                if (neg) put(o++, '-');
                const uint32_t nd = fastq::digits10(v);
                for (uint32_t d = nd; d-- > 0;) {
                    put(o + d, (uint8_t)('0' + v % 10u));
                    v /= 10u;
                }
                o += nd;
            } else {
                for (uint32_t i = 0; i < n; i++) put(o + i, c.d_strings[at + i]);
                o += n;
            }
        }
        return o;
    }
};

__global__ __launch_bounds__(bam::kScanThreads) void bam_len_tagged_kernel(bam::Args a, Cols cols)
{
    __shared__ uint64_t waveSum[bam::kScanThreads / 64];
    const uint64_t r = (uint64_t)blockIdx.x * bam::kScanThreads + threadIdx.x;
    uint64_t len = 0;
    if (r < a.nreads) {
        int32_t st;
        len = bam::record_length(a, r, st);  // with no tags: the call refuses params->ntags != 0
        if (len) {
            uint64_t add;
            if (cols.length(r, true, add)) {
                len += add;
            } else {
                len = 0;
                st = PGN_ERR_INVALID_ARG;
            }
        }
        a.recOff[r] = len;
        a.recStatus[r] = st;
    }
    uint64_t before;
    const uint64_t all = stitch::block_scan(len, waveSum, before);
    if (threadIdx.x == 0) a.blockSums[blockIdx.x] = all;
}

// What the writer knows of a record: bam::load_rec with the tag area's length taken from the record's own
__device__ __forceinline__ bam::Rec typed_rec(const bam::Args& a, uint64_t r)
{
    bam::Rec R;
    R.off = a.recOff[r];
    R.end = a.recOff[r + 1];
    R.b0 = a.readBases[r];
    R.m = a.readBases[r + 1] - R.b0;
    R.sl = (R.m + 1) / 2;
    R.mv0 = R.end - R.off;
    R.c0 = 0;
    if (a.prm.flags & PGN_BAM_MOVES) {
        const uint64_t f0 = a.readFrames[r];
        R.mv0 -= a.readFrames[r + 1] - f0;
        R.c0 = f0 - a.frameBase;
    }
    return R;
}

// bam::bam_write_kernel with two differences: a record's tag area and its first move lie where its length says
// (typed_rec), and step A writes the columns through Cols::put_bam.  It is a copy and not a shared body because the
// old kernel has to compile to the code it had: as a wrapper of a shared body, by value or by reference, it came out
// with another schedule and register count (profiles/tagged_resource_usage.txt).  The identity tests hold the two
// together: with U32 columns both write the same bytes on every case.
__global__ __launch_bounds__(bam::kThreads) void bam_write_tagged_kernel(bam::Args a, Cols cols)
{
    using namespace bam;
    __shared__ __attribute__((aligned(16))) uint8_t image[bam::kImage];
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
            const Rec R = typed_rec(a, r);
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
            if (R.off + R.mv0 > olo && tagAt < ohi) {  // mv0 is the record's length without moves
                cols.put_bam(r, tagAt, put);
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
            Rec R = typed_rec(a, r);
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
                    R = typed_rec(a, r);
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

__global__ __launch_bounds__(fastq::kScanThreads) void fastq_len_tagged_kernel(fastq::RecArgs a, Cols cols)
{
    __shared__ uint64_t waveSum[fastq::kScanThreads / 64];
    const uint64_t r = (uint64_t)blockIdx.x * fastq::kScanThreads + threadIdx.x;
    uint64_t len = 0;
    if (r < a.nreads) {
        int32_t st = a.status[r];
        len = fastq::record_length(a, r);
        if (len) {
            uint64_t add;
            if (cols.length(r, false, add)) {
                len += add;
            } else {
                len = 0;
                st = PGN_ERR_INVALID_ARG;
            }
        }
        a.recOff[r] = len;
        a.recStatus[r] = st;  // of a read without a record; the offset kernel writes the others'
    }
    uint64_t before;
    const uint64_t all = stitch::block_scan(len, waveSum, before);
    if (threadIdx.x == 0) a.blockSums[blockIdx.x] = all;
}

// fastq::fastq_write_kernel with the header's columns written through Cols::put_fastq; a copy for the reason above.
__global__ __launch_bounds__(fastq::kThreads) void fastq_write_tagged_kernel(fastq::RecArgs a, Cols cols)
{
    using namespace fastq;
    __shared__ __attribute__((aligned(16))) uint8_t stage[kTile];
    __shared__ uint64_t edge[2];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const bool reverse = (a.prm.flags & PGN_FASTQ_REVERSE) != 0;
    // Positions are counted from out rounded down to 16: x = output offset + mis, so that x % 16 is the address's.
    const uint64_t mis = a.mis;
    uint8_t* const outA = a.out - mis;
    const uint64_t xEnd = mis + a.blockSums[a.nblocks + 1];  // behind the last written record
    for (uint64_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        const uint64_t x0 = t * kTile;
        const uint64_t xlo = x0 > mis ? x0 : mis, xhi = x0 + kTile < xEnd ? x0 + kTile : xEnd;
        if (xlo >= xhi) return;  // the whole workgroup: this tile and all behind it hold no record
        const uint64_t olo = xlo - mis, ohi = xhi - mis;  // the tile's output offsets
        // its first and last record: the last r with rec_off[r] <= olo, which holds that byte, and the same for ohi - 1
        if (wave == 0) {
            const uint64_t r = wave_first_above(a.recOff, a.nreads + 1, olo);
            if (lane == 0) edge[0] = r - 1;
        } else if (wave == 1) {
            const uint64_t r = wave_first_above(a.recOff, a.nreads + 1, ohi - 1);
            if (lane == 0) edge[1] = r - 1;
        }
        __syncthreads();
        const uint64_t rFirst = edge[0], rLast = edge[1];

        // A. headers and constant bytes, a thread per record
        for (uint64_t r = rFirst + tid; r <= rLast; r += kThreads) {
            const uint64_t off = a.recOff[r], len = a.recOff[r + 1] - off;
            if (!len) continue;
            const uint64_t m = a.readBases[r + 1] - a.readBases[r];
            const uint64_t H = len - 2 * m - 4;  // '@' to the header's newline
            auto put = [&](uint64_t o, uint8_t ch) {
                if (o >= olo && o < ohi) stage[o - olo + (xlo - x0)] = ch;
            };
            put(off + H + m, '\n');
            put(off + H + m + 1, '+');
            put(off + H + m + 2, '\n');
            put(off + len - 1, '\n');
            if (off + H <= olo || off >= ohi) continue;  // the header lies outside the tile
            put(off, '@');
            const uint8_t* id = a.ids + 16 * r;
            for (uint32_t q = 0; q < kUuidChars; q++) put(off + 1 + q, uuid_char(id, q));
            put(cols.put_fastq(r, off + 1 + kUuidChars, put), '\n');
        }

        // B. SEQ and QUAL, a thread per 16-byte unit
        uint32_t direct = 0;  // units stored from registers
#pragma unroll
        for (uint32_t j = 0; j < kUnits; j++) {
            const uint32_t u = j * kThreads + tid;
            const uint64_t ux = x0 + 16ull * u;
            const uint64_t ua = ux > xlo ? ux : xlo, ub = ux + 16 < xhi ? ux + 16 : xhi;  // in x
            if (ua >= ub) continue;
            const uint64_t oa = ua - mis, ob = ub - mis;  // output offsets [oa, ob)
            // the record of the unit's first byte: the last in [rFirst, rLast] with rec_off <= oa
            uint64_t lo = rFirst, hi = rLast;
            while (lo < hi) {
                const uint64_t mid = lo + (hi - lo + 1) / 2;
                if (a.recOff[mid] <= oa)
                    lo = mid;
                else
                    hi = mid - 1;
            }
            uint64_t r = lo, off = a.recOff[r], end = a.recOff[r + 1];
            uint64_t b0 = a.readBases[r], m = a.readBases[r + 1] - b0, H = end - off - 2 * m - 4;
            if (ob - oa == 16 && ob <= end) {
                const uint64_t p = oa - off;
                const bool inSeq = p >= H && p + 16 <= H + m, inQual = p >= H + m + 3 && p + 16 <= H + 2 * m + 3;
                if (inSeq || inQual) {
                    const uint64_t i = inSeq ? p - H : p - H - m - 3;
                    const uint8_t* src = (inSeq ? a.seq : a.qual) + b0 + (reverse ? m - 16 - i : i);
                    Vec16 v;
                    __builtin_memcpy(&v, src, 16);  // at the source's own alignment
                    *reinterpret_cast<Vec16*>(outA + ux) = reverse ? reversed(v) : v;
                    direct |= 1u << j;
                    continue;
                }
            }
            for (uint64_t o = oa; o < ob; o++) {
                if (o >= end) {
                    // the next record with bytes: a run of reads without a record may lie between
                    lo = r + 1, hi = rLast;
                    while (lo < hi) {
                        const uint64_t mid = lo + (hi - lo + 1) / 2;
                        if (a.recOff[mid] <= o)
                            lo = mid;
                        else
                            hi = mid - 1;
                    }
                    r = lo, off = a.recOff[r], end = a.recOff[r + 1];
                    b0 = a.readBases[r], m = a.readBases[r + 1] - b0, H = end - off - 2 * m - 4;
                }
                uint64_t q = o - off;
                if (q < H) continue;  // header
                q -= H;
                const uint8_t* base = a.seq;
                if (q >= m) {
                    if (q < m + 3) continue;  // newline, plus, newline
                    q -= m + 3;
                    if (q >= m) continue;     // the final newline
                    base = a.qual;
                }
                stage[o - olo + (xlo - x0)] = base[b0 + (reverse ? m - 1 - q : q)];
            }
        }
        __syncthreads();

        // C. the image's units to the output
#pragma unroll
        for (uint32_t j = 0; j < kUnits; j++) {
            const uint32_t u = j * kThreads + tid;
            const uint64_t ux = x0 + 16ull * u;
            const uint64_t ua = ux > xlo ? ux : xlo, ub = ux + 16 < xhi ? ux + 16 : xhi;
            if (ua >= ub || (direct >> j & 1u)) continue;
            if (ub - ua == 16)
                *reinterpret_cast<Vec16*>(outA + ux) = *reinterpret_cast<const Vec16*>(stage + 16u * u);
            else
                for (uint64_t x = ua; x < ub; x++) outA[x] = stage[x - x0];
        }
        __syncthreads();  // the next tile writes the image and the edges
    }
}
#endif  // PGN_SELECT_HOST_ONLY

}  // namespace tags
}  // namespace pgn

#endif  // PGN_TAGS_H
