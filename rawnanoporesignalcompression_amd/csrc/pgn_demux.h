// pgn_demux.h -- adapter, primer and barcode sequences at the two ends of called reads (include/pgnano_hip.h
// "Adapters and barcodes"): where each pattern fits best in a read's head or tail window (the search), the read's
// barcode and the bases to keep (the class), and the ragged slice of everything a read carries (the trim).
// Integers and bits alone: the tolerance is zero.
//
// The search.  The text byte of a DP column is the same for every pattern searched in one read's window, so a
// workgroup of kFindThreads takes one (read, side), puts the window's n <= 1,024 bytes in LDS and gives each lane one
// pattern of that side, looping while the side has more patterns than the workgroup has lanes.  The patterns of a side
// come from a per-side index that pattern_index_kernel builds once per call (a third list holds the patterns that
// are not searched; the workgroup of side 0 fills their outputs).
// A lane runs Myers' bit-vector recurrence (Myers 1999, in Hyyro's block form) with the pattern's column of up to
// 128 rows in two 64-bit words: the vertical deltas Pv, Mv of each word stay in registers, the horizontal delta that
// leaves word 0 at row 64 enters word 1, and the score follows the horizontal delta at row L, bit (L - 1) & 63 of
// word (L - 1) / 64.  Rows above L in the last word compute values nobody reads: a row depends on lower rows only.
// The match masks of 'A', 'C', 'G' and 'T' are in registers (bits of pattern bytes 'N' are set in all four); the
// text byte is the same in every lane, so it is read once per wave (readfirstlane) and the choice among the masks is
// a scalar branch.  Any other text byte builds its mask from the pattern's bytes, which is slow and rare.
// The index lists a side's patterns of at most 64 bytes first, and a wave whose lanes all hold such patterns leaves
// the second word out (byLength; measured 0.13 ms of 10.48, profiles/demux_timing.log; the other form stays for
// the measurement and writes the same outputs).
// start is computed for hits only, and hits are few (most barcodes do not match a given read): the same recurrence
// over the reversed pattern and the text read backwards from `end`, with +1 as the horizontal delta that enters
// row 1 (R[0][q] = q), until the score first equals dist.  There the lanes of a wave no longer share a text byte,
// so the mask is chosen per lane.
//
// The class is a thread per read over its P hits, twice: the best and the second class in one pass with two
// (distance, class) slots, then the trimming hits.
// The trim has the record writers' shape: a thread per read for the lengths, stitch::block_scan inside 1,024 reads,
// stitch_scan_kernel over the workgroups' totals, the offsets; then one flat copy kernel over the output's 16-byte
// units serves seq, qual and codes (a unit inside one read is one 16-byte load of any alignment and one aligned
// store, any other goes byte by byte), and a 4-byte form with the subtraction serves base_frame.  No workgroup is
// given to a read.
#ifndef PGN_DEMUX_H
#define PGN_DEMUX_H

#include "pgn_stitch.h"

namespace pgn {
namespace demux {

constexpr uint32_t kNone = PGN_DEMUX_NONE;
constexpr uint32_t kMaxWindow = PGN_DEMUX_MAX_WINDOW;
constexpr uint32_t kMaxPatterns = PGN_DEMUX_MAX_PATTERNS;
constexpr uint32_t kMaxPatternBytes = PGN_DEMUX_MAX_PATTERN_BYTES;
static_assert(kMaxPatternBytes == 128, "a pattern's column is two 64-bit words");

#if defined(__HIP_DEVICE_COMPILE__)
#define PGN_DEMUX_UNIFORM(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#else
#define PGN_DEMUX_UNIFORM(x) (x)
#endif

// ---- the bit-vector column (host and device: the host build is what a CPU test of the recurrence runs) ---------
struct Eq {
    uint64_t w0, w1;  // bit i of w0: pattern byte i matches the text byte; w1: bytes 64..127
};

struct Column {
    uint64_t pv0, mv0, pv1, mv1;  // D[i][j] - D[i-1][j] is +1 (pv) or -1 (mv), rows 1..64 and 65..128
};

struct PatMasks {
    Eq a, c, g, t;
};

struct Hit {
    uint32_t dist, start, end;
};

PGN_HD Column column_start() { return Column{~0ull, 0ull, ~0ull, 0ull}; }  // D[i][0] = i

// The column of the next text byte from the one before it.  hin is D[0][j] - D[0][j-1], 0 or 1.  Returns
// D[L][j] - D[L][j-1].  kTwo false: L <= 64, and word 1 is neither read nor written.
template <bool kTwo>
PGN_HD int32_t column_step(Column& c, const Eq eq, const uint64_t hin, const uint32_t L)
{
    uint64_t xv = eq.w0 | c.mv0;
    uint64_t xh = (((eq.w0 & c.pv0) + c.pv0) ^ c.pv0) | eq.w0;
    uint64_t ph = c.mv0 | ~(xh | c.pv0);
    uint64_t mh = c.pv0 & xh;
    const uint64_t ph0 = ph, mh0 = mh;
    const uint64_t up = ph >> 63, um = mh >> 63;  // the horizontal delta below row 65
    ph = (ph << 1) | hin;
    mh <<= 1;
    c.pv0 = mh | ~(xv | ph);
    c.mv0 = ph & xv;
    const uint32_t sh = (L - 1u) & 63u;
    if (!kTwo) return (int32_t)((ph0 >> sh) & 1u) - (int32_t)((mh0 >> sh) & 1u);

    xv = eq.w1 | c.mv1;
    const uint64_t e1 = eq.w1 | um;
    xh = (((e1 & c.pv1) + c.pv1) ^ c.pv1) | e1;
    ph = c.mv1 | ~(xh | c.pv1);
    mh = c.pv1 & xh;
    const uint64_t lp = L > 64u ? ph : ph0, lm = L > 64u ? mh : mh0;
    const int32_t d = (int32_t)((lp >> sh) & 1u) - (int32_t)((lm >> sh) & 1u);
    ph = (ph << 1) | up;
    mh = (mh << 1) | um;
    c.pv1 = mh | ~(xv | ph);
    c.mv1 = ph & xv;
    return d;
}

// pattern byte i of the pass: from the far end when the pattern is reversed
PGN_HD uint32_t pat_byte(const uint8_t* pat, uint32_t L, bool rev, uint32_t i) { return pat[rev ? L - 1u - i : i]; }

// the mask of text byte y from the pattern's bytes: x matches y iff x == 'N' or x == y
PGN_HD Eq byte_mask(const uint8_t* pat, uint32_t L, bool rev, uint32_t y)
{
    Eq e{0ull, 0ull};
    for (uint32_t i = 0; i < L; i++) {
        const uint32_t x = pat_byte(pat, L, rev, i);
        const uint64_t bit = (x == 'N' || x == y) ? 1ull : 0ull;
        if (i < 64u)
            e.w0 |= bit << i;
        else
            e.w1 |= bit << (i - 64u);
    }
    return e;
}

PGN_HD PatMasks pat_masks(const uint8_t* pat, uint32_t L, bool rev)
{
    PatMasks M{{0ull, 0ull}, {0ull, 0ull}, {0ull, 0ull}, {0ull, 0ull}};
    for (uint32_t i = 0; i < L; i++) {
        const uint32_t x = pat_byte(pat, L, rev, i);
        const uint64_t n = x == 'N' ? 1ull : 0ull;
        const uint64_t ba = (x == 'A' ? 1ull : 0ull) | n, bc = (x == 'C' ? 1ull : 0ull) | n;
        const uint64_t bg = (x == 'G' ? 1ull : 0ull) | n, bt = (x == 'T' ? 1ull : 0ull) | n;
        if (i < 64u) {
            M.a.w0 |= ba << i;
            M.c.w0 |= bc << i;
            M.g.w0 |= bg << i;
            M.t.w0 |= bt << i;
        } else {
            M.a.w1 |= ba << (i - 64u);
            M.c.w1 |= bc << (i - 64u);
            M.g.w1 |= bg << (i - 64u);
            M.t.w1 |= bt << (i - 64u);
        }
    }
    return M;
}

// kUniform: every active lane of the wave passes the same y
template <bool kUniform>
PGN_HD Eq text_mask(const PatMasks& M, const uint8_t* pat, uint32_t L, bool rev, uint32_t y)
{
    if (kUniform) y = PGN_DEMUX_UNIFORM(y);
    if (y == 'A') return M.a;
    if (y == 'C') return M.c;
    if (y == 'G') return M.g;
    if (y == 'T') return M.t;
    return byte_mask(pat, L, rev, y);
}

// One pattern of L in 1..128 bytes in the n <= 1,024 text bytes at `text` (the window, which starts w0 bases into the
// read): the rule of pgn_find_patterns_device.  On the device every active lane of a wave passes the same text.
// kTwo false: L <= 64 in this lane (on the device: in every active lane of the wave).
template <bool kTwo>
PGN_HD Hit search_words(const uint8_t* text, uint32_t n, uint32_t w0, const uint8_t* pat, uint32_t L, uint32_t maxDist)
{
    PatMasks M = pat_masks(pat, L, false);
    Column c = column_start();
    uint32_t score = L, best = L, bestJ = 0;
    for (uint32_t j = 0; j < n; j++) {
        const Eq e = text_mask<true>(M, pat, L, false, text[j]);
        score += (uint32_t)column_step<kTwo>(c, e, 0ull, L);
        if (score < best) {
            best = score;
            bestJ = j + 1u;
        }
    }
    Hit h{best, kNone, w0 + bestJ};
    if (best <= maxDist) {
        uint32_t q = 0;
        if (best != L) {  // R[L][0] = L: a hit at distance L starts where it ends
            M = pat_masks(pat, L, true);
            c = column_start();
            score = L;
            for (q = 1; q < bestJ; q++) {
                const Eq e = text_mask<false>(M, pat, L, true, text[bestJ - q]);
                score += (uint32_t)column_step<kTwo>(c, e, 1ull, L);
                if (score == best) break;
            }
            // q == bestJ without a break: the span is the whole text in front of `end` (a span exists, so it is)
        }
        h.start = h.end - q;
    }
    return h;
}

// two: some lane of the wave has L > 64 (any value that is true where L > 64 gives the same result)
PGN_HD Hit search(const uint8_t* text, uint32_t n, uint32_t w0, const uint8_t* pat, uint32_t L, uint32_t maxDist, bool two)
{
    return two ? search_words<true>(text, n, w0, pat, L, maxDist) : search_words<false>(text, n, w0, pat, L, maxDist);
}

#ifndef PGN_SELECT_HOST_ONLY
using Vec16 = stitch::Vec16;

constexpr uint32_t kFindThreads = 128;   // lanes, and so patterns, per pass of one (read, side)
constexpr uint32_t kIndexThreads = stitch::kPlanThreads;
constexpr uint32_t kScanThreads = stitch::kPlanThreads;
constexpr uint32_t kFlatThreads = 256;   // of the class, copy and base_frame kernels

// ---- the search ----------------------------------------------------------------------------------------------
struct FindArgs {
    uint64_t nreads;  // >= 1
    const uint8_t* seq;
    const uint64_t* readBases;  // nreads + 1
    const int32_t* status;
    uint64_t baseCapacity;
    uint32_t window, npat;
    const uint8_t* pat;
    uint64_t patCapacity;
    const uint32_t* patOff;  // npat + 1
    const uint8_t* patSide;
    const uint32_t* maxDist;
    uint32_t *dist, *start, *end;  // [nreads, npat]
    uint32_t* index;  // context scratch: the head, tail and not-searched lists, npat entries each, then their counts
    uint32_t byLength;  // the lists' order and the one-word waves (PGN_DEMUX_FIND, pgn_kernels.hip)
};

// taken: status 0, read_bases[r] <= read_bases[r+1] <= base_capacity and m > 0
__device__ __forceinline__ bool read_taken(const uint64_t* readBases, const int32_t* status, uint64_t baseCapacity, uint64_t r,
                                           uint64_t& b0, uint64_t& m)
{
    b0 = readBases[r];
    const uint64_t b1 = readBases[r + 1];
    m = b1 > b0 ? b1 - b0 : 0;
    return status[r] == PGN_OK && b1 > b0 && b1 <= baseCapacity;
}

// 0 head, 1 tail, 2 not searched: a side above 1, a length outside 1..128 or bytes beyond the pattern buffer
__device__ __forceinline__ uint32_t pattern_list(const FindArgs& a, uint32_t p)
{
    const uint32_t o0 = a.patOff[p], o1 = a.patOff[p + 1], side = a.patSide[p];
    if (side > 1u || o1 <= o0 || o1 - o0 > kMaxPatternBytes || o1 > a.patCapacity) return 2u;
    return side;
}

// The three lists by one workgroup, each in pattern order; with byLength a side's patterns of at most 64 bytes come
// first, so that whole waves of the search hold such patterns alone and leave the column's second word out.
__global__ __launch_bounds__(kIndexThreads) void pattern_index_kernel(FindArgs a)
{
    __shared__ uint64_t waveSum[kIndexThreads / 64];
    const uint32_t P = a.npat;
    uint32_t count[5] = {0, 0, 0, 0, 0};  // head short, head long, tail short, tail long, not searched
    uint32_t base[5] = {0, 0, 0, 0, 0};
    for (uint32_t pass = 0; pass < 2; pass++) {
        for (uint32_t first = 0; first < P; first += kIndexThreads) {
            const uint32_t p = first + threadIdx.x;
            uint32_t list = 5u;
            if (p < P) {
                const uint32_t side = pattern_list(a, p);
                const bool isLong = a.byLength && side < 2u && a.patOff[p + 1] - a.patOff[p] > 64u;
                list = side == 2u ? 4u : 2u * side + (isLong ? 1u : 0u);
            }
#pragma unroll
            for (uint32_t l = 0; l < 5; l++) {
                uint64_t before;
                const uint64_t all = stitch::block_scan(list == l ? 1u : 0u, waveSum, before);
                if (pass == 0)
                    count[l] += (uint32_t)all;
                else {
                    if (list == l) a.index[base[l] + (uint32_t)before] = p;
                    base[l] += (uint32_t)all;
                }
            }
        }
        base[0] = 0, base[1] = count[0];
        base[2] = P, base[3] = P + count[2];
        base[4] = 2 * P;
    }
    if (threadIdx.x == 0) {
        a.index[3 * P + 0] = count[0] + count[1];
        a.index[3 * P + 1] = count[2] + count[3];
        a.index[3 * P + 2] = count[4];
    }
}

__global__ __launch_bounds__(kFindThreads) void find_patterns_kernel(FindArgs a)
{
    __shared__ uint8_t text[kMaxWindow];
    const uint32_t tid = threadIdx.x, P = a.npat;
    const uint32_t nSide[2] = {a.index[3 * P], a.index[3 * P + 1]}, nSkip = a.index[3 * P + 2];
    for (uint64_t w = blockIdx.x; w < 2 * a.nreads; w += gridDim.x) {
        const uint64_t r = w >> 1;
        const uint32_t side = (uint32_t)(w & 1u);
        uint32_t* const dist = a.dist + r * P;
        uint32_t* const start = a.start + r * P;
        uint32_t* const end = a.end + r * P;
        uint64_t b0, m;
        if (!read_taken(a.readBases, a.status, a.baseCapacity, r, b0, m)) {
            if (side == 0)
                for (uint32_t p = tid; p < P; p += kFindThreads) dist[p] = start[p] = end[p] = kNone;
            continue;
        }
        if (side == 0)
            for (uint32_t k = tid; k < nSkip; k += kFindThreads) {
                const uint32_t p = a.index[2 * P + k];
                dist[p] = start[p] = end[p] = kNone;
            }
        const uint32_t count = nSide[side];
        if (count == 0) continue;  // the whole workgroup
        const uint32_t n = (uint32_t)(m < a.window ? m : a.window);
        const uint64_t w0 = side ? m - n : 0;
        for (uint32_t j = tid; j < n; j += kFindThreads) text[j] = a.seq[b0 + w0 + j];
        __syncthreads();
        for (uint32_t k = tid; k < count; k += kFindThreads) {
            const uint32_t p = a.index[side * P + k];
            const uint32_t o0 = a.patOff[p];
            const uint32_t L = a.patOff[p + 1] - o0;
            const bool two = !a.byLength || __any(L > 64u);  // the same in every lane of the wave
            const Hit h = search(text, n, (uint32_t)w0, a.pat + o0, L, a.maxDist[p], two);
            dist[p] = h.dist;
            start[p] = h.start;
            end[p] = h.end;
        }
        __syncthreads();  // the next (read, side) writes the window
    }
}

// ---- the class -----------------------------------------------------------------------------------------------
struct ClassArgs {
    uint64_t nreads;
    const uint64_t* readBases;
    const int32_t* status;
    uint64_t baseCapacity;
    uint32_t npat, nclasses, minSep;
    const uint8_t* patSide;
    const uint32_t *maxDist, *patClass;
    const uint32_t *dist, *start, *end;
    uint32_t *barcode, *bestDist, *secondDist, *lo, *hi;
};

__global__ __launch_bounds__(kFlatThreads) void classify_reads_kernel(ClassArgs a)
{
    const uint64_t r = (uint64_t)blockIdx.x * kFlatThreads + threadIdx.x;
    if (r >= a.nreads) return;
    uint64_t b0, m;
    if (!read_taken(a.readBases, a.status, a.baseCapacity, r, b0, m)) {
        a.barcode[r] = a.bestDist[r] = a.secondDist[r] = kNone;
        a.lo[r] = a.hi[r] = 0;
        return;
    }
    const uint32_t P = a.npat;
    const uint32_t* const dist = a.dist + r * P;
    // a hit: a side of 0 or 1, a class below nclasses or none, and a distance (not 0xFFFFFFFF) within max_dist
    auto hit = [&](uint32_t p, uint32_t& cls) {
        cls = a.patClass[p];
        if (cls != kNone && cls >= a.nclasses) return false;
        if (a.patSide[p] > 1u) return false;
        const uint32_t d = dist[p];
        return d != kNone && d <= a.maxDist[p];
    };
    // (d1, c1): the lowest (d_c, c) so far; (d2, c2): the lowest among the other classes
    uint32_t d1 = kNone, c1 = kNone, d2 = kNone, c2 = kNone;
    for (uint32_t p = 0; p < P; p++) {
        uint32_t cls;
        if (!hit(p, cls) || cls == kNone) continue;
        const uint32_t d = dist[p];
        if (cls == c1) {
            d1 = d < d1 ? d : d1;
        } else if (cls == c2) {
            d2 = d < d2 ? d : d2;
            if (d2 < d1 || (d2 == d1 && c2 < c1)) {
                const uint32_t td = d1, tc = c1;
                d1 = d2, c1 = c2;
                d2 = td, c2 = tc;
            }
        } else if (d < d1 || (d == d1 && cls < c1)) {
            d2 = d1, c2 = c1;
            d1 = d, c1 = cls;
        } else if (d < d2 || (d == d2 && cls < c2)) {
            d2 = d, c2 = cls;
        }
    }
    const uint32_t barcode = (c1 != kNone && (c2 == kNone || d2 - d1 >= a.minSep)) ? c1 : kNone;
    const uint32_t m32 = (uint32_t)m;
    uint32_t lo = 0, hi = m32;
    bool tail = false;
    for (uint32_t p = 0; p < P; p++) {
        uint32_t cls;
        if (!hit(p, cls) || (cls != kNone && cls != barcode)) continue;  // a losing class does not trim
        if (a.patSide[p] == 0) {
            const uint32_t e = a.end[r * P + p];
            lo = e > lo ? e : lo;
        } else {
            const uint32_t s = a.start[r * P + p];
            hi = (!tail || s < hi) ? s : hi;
            tail = true;
        }
    }
    if (lo >= hi) lo = 0, hi = m32;
    a.barcode[r] = barcode;
    a.bestDist[r] = d1;
    a.secondDist[r] = d2;
    a.lo[r] = lo;
    a.hi[r] = hi;
}

// ---- the trim ------------------------------------------------------------------------------------------------
struct TrimArgs {
    uint64_t nreads;  // >= 1
    const uint8_t *seq, *qual;  // qual may be null
    const uint64_t* readBases;
    const int32_t* status;
    uint64_t baseCapacity;
    const uint32_t *lo, *hi;
    const uint32_t* baseFrame;
    const uint64_t* readFrames;  // null: no moves, and none of the frame arrays is touched
    const uint8_t* codes;
    uint64_t frameBase, frameCapacity;
    uint8_t *newSeq, *newQual;
    uint32_t* newBaseFrame;
    uint64_t newBaseCapacity;
    uint64_t* newReadBases;      // the lengths between the length and the offset kernel, then the scan
    int32_t* newStatus;
    uint8_t* newCodes;
    uint64_t newFrameCapacity;
    uint64_t* newReadFrames;     // as newReadBases
    uint32_t* trimFrames;
    uint64_t* blockSums;         // context scratch: nblocks + 1 for the bases, then nblocks + 1 for the frames
    uint64_t nblocks;
};

__global__ __launch_bounds__(kScanThreads) void trim_len_kernel(TrimArgs a)
{
    __shared__ uint64_t waveSum[kScanThreads / 64];
    const uint64_t r = (uint64_t)blockIdx.x * kScanThreads + threadIdx.x;
    const bool moves = a.readFrames != nullptr;
    uint64_t len = 0, flen = 0;
    if (r < a.nreads) {
        uint64_t b0, m;
        const bool taken = read_taken(a.readBases, a.status, a.baseCapacity, r, b0, m);
        const uint64_t lo = a.lo[r], hi = a.hi[r];
        bool ok = taken && lo <= hi && hi <= m;
        uint64_t flo = 0, fhi = 0;
        if (ok && moves) {
            const uint64_t f0 = a.readFrames[r], f1 = a.readFrames[r + 1];
            ok = f0 >= a.frameBase && f1 >= f0 && f1 - a.frameBase <= a.frameCapacity;
            if (ok) {
                const uint64_t F = f1 - f0;
                if (lo < hi) {
                    flo = a.baseFrame[b0 + lo];
                    fhi = hi < m ? (uint64_t)a.baseFrame[b0 + hi] : F;
                }
                ok = flo <= fhi && fhi <= F;
            }
        }
        int32_t st = a.status[r];
        if (ok) {
            len = hi - lo;
            flen = fhi - flo;
            st = PGN_OK;
        } else if (st == PGN_OK) {
            st = PGN_ERR_INVALID_ARG;
            flo = 0;
        } else {
            flo = 0;
        }
        a.newReadBases[r] = len;
        a.newStatus[r] = st;  // PGN_OK marks a sliced read for the offset kernel, which also looks at the capacities
        if (moves) {
            a.newReadFrames[r] = flen;
            a.trimFrames[r] = (uint32_t)flo;
        }
    }
    uint64_t before;
    uint64_t all = stitch::block_scan(len, waveSum, before);
    if (threadIdx.x == 0) a.blockSums[blockIdx.x] = all;
    if (moves) {
        all = stitch::block_scan(flen, waveSum, before);
        if (threadIdx.x == 0) a.blockSums[a.nblocks + 1 + blockIdx.x] = all;
    }
}

__global__ __launch_bounds__(kScanThreads) void trim_offset_kernel(TrimArgs a)
{
    __shared__ uint64_t waveSum[kScanThreads / 64];
    const uint64_t r = (uint64_t)blockIdx.x * kScanThreads + threadIdx.x;
    const bool moves = a.readFrames != nullptr, mine = r < a.nreads;
    const uint64_t len = mine ? a.newReadBases[r] : 0, flen = mine && moves ? a.newReadFrames[r] : 0;
    uint64_t before, fbefore = 0;
    stitch::block_scan(len, waveSum, before);
    if (moves) stitch::block_scan(flen, waveSum, fbefore);
    if (!mine) return;
    const uint64_t off = a.blockSums[blockIdx.x] + before;
    bool cut = len && off + len > a.newBaseCapacity;
    a.newReadBases[r] = off;
    if (r + 1 == a.nreads) a.newReadBases[a.nreads] = off + len;
    if (moves) {
        const uint64_t foff = a.blockSums[a.nblocks + 1 + blockIdx.x] + fbefore;
        cut = cut || (flen && foff + flen > a.newFrameCapacity);
        a.newReadFrames[r] = foff;
        if (r + 1 == a.nreads) a.newReadFrames[a.nreads] = foff + flen;
    }
    if (cut) a.newStatus[r] = PGN_ERR_DST_TOO_SMALL;  // only a sliced read has a length
}

// The ragged copy of one array: new element g of read r is old element oldOff[r] - oldBase + shift[r] + (g - newOff[r])
struct CopyArgs {
    uint64_t nreads;
    const uint64_t* newOff;  // nreads + 1, the scan
    const uint64_t* oldOff;
    uint64_t oldBase;
    const uint32_t* shift;   // lo for the bases, trim_frames for the codes
    const uint32_t* sub;     // base_frame: trim_frames, taken off every value
    const void* src;
    void* dst;
    uint64_t capacity;       // elements of dst
};

// the last r in [0, nreads) with off[r] <= g, for g < off[nreads]: the read that holds g
__device__ __forceinline__ uint64_t read_of(const uint64_t* off, uint64_t nreads, uint64_t g)
{
    uint64_t lo = 0, hi = nreads - 1;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (off[mid] <= g)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// bytes: a thread per 16-byte unit of dst, counted from dst's address rounded down to 16
__global__ __launch_bounds__(kFlatThreads) void trim_copy_kernel(CopyArgs a)
{
    const uint8_t* const src = static_cast<const uint8_t*>(a.src);
    uint8_t* const dst = static_cast<uint8_t*>(a.dst);
    const uint64_t all = a.newOff[a.nreads], total = all < a.capacity ? all : a.capacity;
    const uint64_t mis = (uint64_t)((uintptr_t)dst & 15u);
    const uint64_t units = (total + mis + 15) / 16;
    for (uint64_t u = (uint64_t)blockIdx.x * kFlatThreads + threadIdx.x; u < units; u += (uint64_t)gridDim.x * kFlatThreads) {
        const uint64_t ga = 16 * u > mis ? 16 * u - mis : 0, gb = 16 * u + 16 - mis < total ? 16 * u + 16 - mis : total;
        if (ga >= gb) continue;
        uint64_t r = read_of(a.newOff, a.nreads, ga);
        uint64_t from = a.oldOff[r] - a.oldBase + a.shift[r], at = a.newOff[r], next = a.newOff[r + 1];
        if (gb - ga == 16 && gb <= next) {
            *reinterpret_cast<Vec16*>(dst + ga) = stitch::load16(src + from + (ga - at));
            continue;
        }
        for (uint64_t g = ga; g < gb; g++) {
            while (g >= next) {  // g < newOff[nreads], so r + 1 < nreads here
                r++;
                at = next;
                next = a.newOff[r + 1];
                from = a.oldOff[r] - a.oldBase + a.shift[r];
            }
            dst[g] = src[from + (g - at)];
        }
    }
}

// base_frame: a thread per value, the read's first kept frame taken off
__global__ __launch_bounds__(kFlatThreads) void trim_base_frame_kernel(CopyArgs a)
{
    const uint32_t* const src = static_cast<const uint32_t*>(a.src);
    uint32_t* const dst = static_cast<uint32_t*>(a.dst);
    const uint64_t all = a.newOff[a.nreads], total = all < a.capacity ? all : a.capacity;
    for (uint64_t g = (uint64_t)blockIdx.x * kFlatThreads + threadIdx.x; g < total; g += (uint64_t)gridDim.x * kFlatThreads) {
        const uint64_t r = read_of(a.newOff, a.nreads, g);
        dst[g] = src[a.oldOff[r] - a.oldBase + a.shift[r] + (g - a.newOff[r])] - a.sub[r];
    }
}
#endif  // PGN_SELECT_HOST_ONLY

}  // namespace demux
}  // namespace pgn

#endif  // PGN_DEMUX_H
