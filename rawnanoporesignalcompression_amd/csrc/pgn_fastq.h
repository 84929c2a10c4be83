// pgn_fastq.h -- per-read mean quality with a pass flag, and the kept reads as FASTQ text (include/pgnano_hip.h
// "FASTQ records", the rules of pgn_read_qual_device and pgn_fastq_records_device).  Integer sums, comparisons and
// byte copies alone: the tolerance is zero.
//
// Read lengths are heavy-tailed, so neither call gives a read to a workgroup; every dependency is a kernel boundary.
//   pgn_read_qual_device: flat over the bases, a tile of PGN_READ_QUAL_TILE_BASES per workgroup, sixteen bases per
//     thread.  Two waves find the reads that cross the tile, each with a 64-way search in read_bases (a round reads
//     64 entries at once: three rounds for 10^5 reads, where ctc_bounds_kernel's binary search takes seventeen
//     dependent loads).  A thread whose bases lie in one read sums them from one 16-byte load; a wave whose lanes all
//     did so for the same read adds one value to the read's uint64 accumulator, every other lane adds its own, read
//     by read.  Integer sums have no order, so the result is exact.  A thread per read then applies the thresholds.
//   pgn_fastq_records_device: a thread per read for the lengths, the exclusive scan in the three steps of the
//     stitch plan (block_scan inside 1,024 reads, stitch_scan_kernel over the workgroups' totals, the offsets), and
//     the writer, flat over the output bytes: a workgroup owns PGN_FASTQ_TILE_BYTES between two 16-byte addresses,
//     finds its first and last record with two 64-way searches in rec_off, and
//       A. a thread per record formats the header and the four constant bytes into the tile's LDS image,
//       B. a thread per 16-byte unit copies SEQ and QUAL: a unit wholly inside one of them is one 16-byte load at
//          the source's own alignment and one aligned 16-byte store, straight from registers; any other unit puts
//          its SEQ and QUAL bytes into the image one by one,
//       C. the units of B's second kind leave the image as aligned 16-byte stores, byte by byte only in front of
//          the first and behind the last 16-byte address of the whole output.
//     A record is at least 44 bytes long, so a unit meets at most two records.
#ifndef PGN_FASTQ_H
#define PGN_FASTQ_H

#include "pgn_qual.h"

namespace pgn {
namespace fastq {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kQualTile = PGN_READ_QUAL_TILE_BASES;  // bases of one workgroup of the sum
constexpr uint32_t kQualPerThread = kQualTile / kThreads;
constexpr uint32_t kTile = PGN_FASTQ_TILE_BYTES;          // output bytes of one workgroup of the writer
constexpr uint32_t kUnits = kTile / 16 / kThreads;        // 16-byte units of one thread
constexpr uint32_t kMaxTags = PGN_FASTQ_MAX_TAGS;
constexpr uint32_t kErrs = 94;                            // phred characters '!' .. '~'
constexpr uint32_t kFixedBytes = 42;                      // '@', 36 of the uuid, four newlines and the '+'
constexpr uint32_t kUuidChars = 36;
constexpr uint32_t kScanThreads = stitch::kPlanThreads;   // block_scan is written for this many threads
static_assert(kQualPerThread == 16, "a 16-byte load per thread");
static_assert(kTile % (16 * kThreads) == 0, "whole units, whole rounds");

// PGN_ERR_INVALID_ARG conditions of the record call's parameters, in the header's order
inline bool params_valid(const pgn_fastq_params* P)
{
    if (!P) return false;
    if (P->flags & ~(uint32_t)PGN_FASTQ_REVERSE) return false;
    if (P->ntags > kMaxTags) return false;
    for (uint32_t k = 0; k < P->ntags; k++) {
        const uint8_t a = P->tag_name[k][0], b = P->tag_name[k][1];
        const bool alpha0 = (a >= 'A' && a <= 'Z') || (a >= 'a' && a <= 'z');
        const bool alnum1 = (b >= 'A' && b <= 'Z') || (b >= 'a' && b <= 'z') || (b >= '0' && b <= '9');
        if (!alpha0 || !alnum1) return false;
    }
    return true;
}

// decimal digits of v, by comparisons against the powers of ten
PGN_HD uint32_t digits10(uint32_t v)
{
    return 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) +
           (v >= 10000000u) + (v >= 100000000u) + (v >= 1000000000u);
}

// index into err of one quality byte
PGN_HD uint32_t err_index(uint32_t q) { return (q < 33u ? 33u : q > 126u ? 126u : q) - 33u; }

// character q in [0, 36) of the uuid of the 16 bytes at id
PGN_HD uint8_t uuid_char(const uint8_t* id, uint32_t q)
{
    if (q == 8 || q == 13 || q == 18 || q == 23) return '-';
    const uint32_t h = q - (q > 8) - (q > 13) - (q > 18) - (q > 23);  // the hex digit's index
    const uint32_t nib = (id[h >> 1] >> ((h & 1u) ? 0 : 4)) & 15u;
    return (uint8_t)(nib < 10 ? '0' + nib : 'a' + (nib - 10));
}

#ifndef PGN_SELECT_HOST_ONLY
using Vec16 = ctc::Vec16;

// The first i in [0, n) with a[i] > v, or n, for a non-decreasing a.  The whole wave calls it: a round reads 64
// entries spread over what is left, which shrinks to below a 64th.  It ends on any data, inside [0, n].
__device__ __forceinline__ uint64_t wave_first_above(const uint64_t* a, uint64_t n, uint64_t v)
{
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t step = (hi - lo + 63) / 64;
        const uint64_t idx = lo + lane * step;
        const bool below = idx < hi && a[idx] <= v;
        const uint32_t c = (uint32_t)__popcll(__ballot(below));
        if (c == 0) break;  // a[lo] is above v
        const uint64_t top = lo + c * step;
        hi = top < hi ? top : hi;
        lo = lo + (c - 1) * step + 1;
    }
    return lo;
}

// =============================================================================================
// Mean quality
// =============================================================================================
struct QualArgs {
    uint64_t nreads;            // >= 1
    const uint64_t* readBases;  // nreads + 1
    const int32_t* status;
    const uint8_t* qual;
    uint64_t baseCapacity;
    uint64_t tileBase;          // the tile of the launch's first workgroup
    uint64_t* acc;              // one per read, zeroed: d_err_sum or context scratch
    uint32_t* meanQ;
    uint64_t* errSum;           // may be null
    uint8_t* pass;
    pgn_read_qual_params prm;
};

// A read's bases [b0, b0 + m) and the first one that counts; false iff the read has no input.
__device__ __forceinline__ bool read_input(const QualArgs& a, uint64_t r, uint64_t& b0, uint64_t& m, uint64_t& skip)
{
    b0 = a.readBases[r];
    const uint64_t b1 = a.readBases[r + 1];
    m = skip = 0;
    if (a.status[r] != PGN_OK || b1 <= b0 || b1 > a.baseCapacity) return false;
    m = b1 - b0;
    skip = m > a.prm.skip_bases ? a.prm.skip_bases : 0;
    return true;
}

__global__ __launch_bounds__(kThreads) void read_qual_sum_kernel(QualArgs a)
{
    __shared__ uint32_t errT[kErrs];
    __shared__ uint64_t edge[2];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t A = (a.tileBase + blockIdx.x) * kQualTile;  // below baseCapacity by the grid's size
    const uint64_t B = a.baseCapacity - A < kQualTile ? a.baseCapacity : A + kQualTile;
    if (tid < kErrs) errT[tid] = a.prm.err[tid];
    // the reads that cross the tile: from the first that ends above A to the one before the first that starts at B
    if (wave == 0) {
        const uint64_t r = wave_first_above(a.readBases + 1, a.nreads, A);
        if (lane == 0) edge[0] = r;
    } else if (wave == 1) {
        const uint64_t r = wave_first_above(a.readBases, a.nreads, B - 1);
        if (lane == 0) edge[1] = r;
    }
    __syncthreads();
    const uint64_t rLo = edge[0], rHi = edge[1];
    if (rLo >= rHi) return;  // the whole workgroup

    const uint64_t g0 = A + (uint64_t)tid * kQualPerThread;
    const uint64_t g1 = g0 + kQualPerThread < B ? g0 + kQualPerThread : B;
    // the read of the thread's first base: the first in [rLo, rHi) that ends above it
    uint64_t r = rLo;
    if (g0 < g1) {
        uint64_t lo = rLo, hi = rHi;
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (a.readBases[mid + 1] <= g0)
                lo = mid + 1;
            else
                hi = mid;
        }
        r = lo;
    }
    bool whole = false;  // all sixteen bases count for read r
    uint64_t sum = 0;
    if (g0 < g1 && r < rHi) {
        uint64_t b0, m, skip;
        whole = read_input(a, r, b0, m, skip) && g0 >= b0 + skip && g0 + kQualPerThread <= b0 + m;
    }
    if (whole) {
        const uint8_t* p = a.qual + g0;
        if (((uintptr_t)p & 15u) == 0) {
            const Vec16 v = *reinterpret_cast<const Vec16*>(p);
#pragma unroll
            for (uint32_t i = 0; i < 16; i++) sum += errT[err_index((v[i >> 2] >> (8 * (i & 3u))) & 0xFFu)];
        } else {
#pragma unroll
            for (uint32_t i = 0; i < 16; i++) sum += errT[err_index(p[i])];
        }
    }
    // a wave inside one read adds once
    const uint64_t r0 = __shfl(r, 0);
    if (__all(whole && r == r0)) {
#pragma unroll
        for (uint32_t off = 32; off; off >>= 1) sum += __shfl_xor(sum, off);
        if (lane == 0) atomicAdd(reinterpret_cast<unsigned long long*>(a.acc + r0), (unsigned long long)sum);
        return;
    }
    if (whole) {
        atomicAdd(reinterpret_cast<unsigned long long*>(a.acc + r), (unsigned long long)sum);
        return;
    }
    // read by read over the thread's bases
    uint64_t g = g0;
    while (g < g1 && r < rHi) {
        uint64_t b0, m, skip;
        const bool input = read_input(a, r, b0, m, skip);
        const uint64_t b1 = a.readBases[r + 1];
        if (b1 <= g) {
            r++;
            continue;
        }
        const uint64_t end = b1 < g1 ? b1 : g1;
        if (input) {
            uint64_t from = b0 + skip;
            from = from > g ? from : g;
            sum = 0;
            for (uint64_t i = from; i < end; i++) sum += errT[err_index(a.qual[i])];
            if (from < end) atomicAdd(reinterpret_cast<unsigned long long*>(a.acc + r), (unsigned long long)sum);
        }
        g = end;  // a read that starts above g leaves the bases between to no read
        r++;
    }
}

// mean_q, err_sum and pass of every read, a thread per read
__global__ void read_qual_finish_kernel(QualArgs a)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.nreads) return;
    uint64_t b0, m, skip, U = 0;
    uint32_t q = 0, pass = 0;
    if (read_input(a, r, b0, m, skip)) {
        U = a.acc[r];
        const uint64_t n = m - skip;
        q = a.prm.mean.q_min;
        for (uint32_t k = 0; k < a.prm.mean.nthresholds; k++) q += U <= (uint64_t)a.prm.mean.thr[k] * n ? 1u : 0u;
        pass = q >= a.prm.min_mean_q ? 1u : 0u;
    }
    a.meanQ[r] = q;
    if (a.errSum) a.errSum[r] = U;
    a.pass[r] = (uint8_t)pass;
}

// =============================================================================================
// Records
// =============================================================================================
struct RecArgs {
    uint64_t nreads;            // >= 1
    const uint8_t* ids;         // 16 per read
    const uint64_t* readBases;  // nreads + 1
    const int32_t* status;
    const uint8_t* keep;        // may be null
    const uint8_t* seq;
    const uint8_t* qual;
    uint64_t baseCapacity;
    uint8_t* out;
    uint64_t byteCapacity;
    uint64_t* recOff;           // nreads + 1: the lengths between the count and the offset kernel, then the scan
    int32_t* recStatus;
    uint64_t* blockSums;        // context scratch: one per workgroup of the count kernel, their total, and the end of
    uint64_t nblocks;           // the written records at blockSums[nblocks + 1]
    uint64_t ntiles;            // of the writer
    uint32_t mis;               // out modulo 16
    pgn_fastq_params prm;
};

// length of read r's record, 0 for a read that is not kept
__device__ __forceinline__ uint64_t record_length(const RecArgs& a, uint64_t r)
{
    const uint64_t b0 = a.readBases[r], b1 = a.readBases[r + 1];
    if (a.status[r] != PGN_OK || b1 <= b0 || b1 > a.baseCapacity) return 0;
    if (a.keep && !a.keep[r]) return 0;
    uint64_t len = kFixedBytes + 2 * (b1 - b0);
#pragma unroll
    for (uint32_t k = 0; k < kMaxTags; k++)
        if (k < a.prm.ntags) len += 6u + digits10(a.prm.d_tag[k][r]);
    return len;
}

__global__ __launch_bounds__(kScanThreads) void fastq_len_kernel(RecArgs a)
{
    __shared__ uint64_t waveSum[kScanThreads / 64];
    const uint64_t r = (uint64_t)blockIdx.x * kScanThreads + threadIdx.x;
    uint64_t len = 0;
    if (r < a.nreads) {
        len = record_length(a, r);
        a.recOff[r] = len;
    }
    uint64_t before;
    const uint64_t all = stitch::block_scan(len, waveSum, before);
    if (threadIdx.x == 0) a.blockSums[blockIdx.x] = all;
}

// rec_off and rec_status of every read behind the scan of the workgroups' totals, and the end of the written
// records: the largest rec_off value that byte_capacity admits, which exactly one thread finds
__global__ __launch_bounds__(kScanThreads) void fastq_offset_kernel(RecArgs a)
{
    __shared__ uint64_t waveSum[kScanThreads / 64];
    const uint64_t r = (uint64_t)blockIdx.x * kScanThreads + threadIdx.x;
    const uint64_t len = r < a.nreads ? a.recOff[r] : 0;
    uint64_t before;
    stitch::block_scan(len, waveSum, before);
    if (r >= a.nreads) return;
    const uint64_t off = a.blockSums[blockIdx.x] + before, end = off + len;
    a.recOff[r] = off;
    int32_t st = PGN_OK;
    if (len)
        st = end > a.byteCapacity ? PGN_ERR_DST_TOO_SMALL : PGN_OK;
    else
        st = a.status[r];
    a.recStatus[r] = st;
    if (len && off <= a.byteCapacity && end > a.byteCapacity) a.blockSums[a.nblocks + 1] = off;
    if (r + 1 == a.nreads) {
        a.recOff[a.nreads] = end;
        if (end <= a.byteCapacity) a.blockSums[a.nblocks + 1] = end;
    }
}

// the sixteen bytes of v in reverse order
__device__ __forceinline__ Vec16 reversed(const Vec16 v)
{
    Vec16 o;
    o[0] = __builtin_bswap32(v[3]);
    o[1] = __builtin_bswap32(v[2]);
    o[2] = __builtin_bswap32(v[1]);
    o[3] = __builtin_bswap32(v[0]);
    return o;
}

__global__ __launch_bounds__(kThreads) void fastq_write_kernel(RecArgs a)
{
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
            uint64_t o = off + 1 + kUuidChars;
#pragma unroll
            for (uint32_t k = 0; k < kMaxTags; k++) {
                if (k < a.prm.ntags) {
                    uint32_t v = a.prm.d_tag[k][r];
                    const uint32_t nd = digits10(v);
                    put(o, '\t');
                    put(o + 1, a.prm.tag_name[k][0]);
                    put(o + 2, a.prm.tag_name[k][1]);
                    put(o + 3, ':');
                    put(o + 4, 'i');
                    put(o + 5, ':');
                    for (uint32_t d = nd; d-- > 0;) {
                        put(o + 6 + d, (uint8_t)('0' + v % 10u));
                        v /= 10u;
                    }
                    o += 6u + nd;
                }
            }
            put(o, '\n');
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

}  // namespace fastq
}  // namespace pgn

#endif  // PGN_FASTQ_H
