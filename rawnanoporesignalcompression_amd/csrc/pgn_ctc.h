// pgn_ctc.h -- best-path CTC decode of the stitched frames and the collapse of per-frame codes into bases
// (include/pgnano_hip.h "Stitched frames to bases").
//
// The work is flat over the frames of the window, a tile of PGN_CTC_TILE_FRAMES frames per workgroup of 256
// threads, never a workgroup per read; every dependency between workgroups is a kernel boundary:
//   the reads at the tile edges (a thread per edge: binary searches in read_frames)
//   -> label pass: per frame its read (a binary search in read_frames between the tile's first and last read),
//               the argmax of its scores, the code byte; per tile the number of emitting frames
//   -> the exclusive scan of the tile counts (8,192 per workgroup, then one workgroup over their totals)
//   -> write pass over the code bytes: ballot and popcount prefix inside a wave, the wave counts inside the
//      tile; seq, base_frame, base_score, and read_bases[r] of the reads whose start lies in the tile
//   -> the statuses (a thread per read) and read_bases[nreads].
// The collapse call counts the emitting codes per tile instead of the label pass; the rest is the same.
// The tile that holds read_frames[r], clamped into the window, owns read r's entry of read_bases: reads are
// found by their start, not by their frames, so a run of empty reads is owned like any other read.
#ifndef PGN_CTC_H
#define PGN_CTC_H

#include "pgn_stitch.h"

namespace pgn {
namespace ctc {

constexpr uint32_t kTile = PGN_CTC_TILE_FRAMES;  // frames of one workgroup
// Its threads, four frames each: with a thread per frame a CU holds two tiles, too few bytes in flight for
// 10-byte frames (33 ms against 20 for the decode at 2 x 10^9 frames).
constexpr uint32_t kThreads = 256;
constexpr uint32_t kPerThread = kTile / kThreads;
constexpr uint32_t kStageFrameBytes = 32;        // contiguous frames up to this size are staged through LDS
constexpr uint32_t kScanThreads = stitch::kPlanThreads;  // block_scan is written for this many threads
constexpr uint32_t kScanPerThread = 8;           // tile counts one thread of the scan takes
constexpr uint32_t kScanSpan = kScanThreads * kScanPerThread;  // and one workgroup of it
static_assert(kTile % kThreads == 0 && kThreads % 64 == 0, "whole waves, whole rounds");

PGN_HD uint32_t elem_bytes(uint32_t scoreType) { return scoreType == PGN_OUT_F32 ? 4u : 2u; }

// PGN_ERR_INVALID_ARG conditions of the parameters, in the header's order
inline bool params_valid(const pgn_ctc_params* P)
{
    if (!P) return false;
    if (P->classes < 2 || P->classes > 64 || P->blank >= P->classes) return false;
    return (P->score_type == PGN_OUT_F32 || P->score_type == PGN_OUT_F16) && P->pad == 0;
}

// One score as its exact float32 value.
template <typename Ptr>
PGN_HD float score_at(Ptr p, uint32_t c, uint32_t elem)
{
    if (elem == 4) return reinterpret_cast<const float*>(p)[c];  // elements lie at multiples of their size
    return (float) reinterpret_cast<const _Float16*>(p)[c];
}

// numpy's argmax of one frame: IEEE comparison (so -0 == +0), the lowest index wins a tie, a NaN beats every
// number and the first NaN wins.
template <typename Ptr>
PGN_HD uint32_t argmax_frame(Ptr p, uint32_t C, uint32_t elem)
{
    uint32_t best = 0;
    float bv = score_at(p, 0, elem);
    for (uint32_t c = 1; c < C; c++) {
        const float v = score_at(p, c, elem);
        if (bv == bv && (v > bv || v != v)) {
            bv = v;
            best = c;
        }
    }
    return best;
}

#ifndef PGN_SELECT_HOST_ONLY
struct Args {
    uint64_t nreads;             // >= 1
    const uint64_t* readFrames;  // nreads + 1
    const uint8_t* frames;       // frame i at frames + (i - frameBase) * frameStride (decode only)
    uint64_t frameStride;
    uint32_t classes, blank, elem, staged;
    uint64_t frameBase, capacity;  // the window; frameBase + capacity does not wrap
    uint64_t ntiles;               // >= 1
    uint8_t* codes;                // one byte per frame of the window
    uint64_t* tileSums;            // context scratch: one per tile
    uint64_t* spanSums;            // context scratch: one per kScanSpan tiles, then the total
    uint64_t nspans;
    uint32_t* bounds;              // context scratch, two per tile edge k = 0..ntiles, at frame e_k = frameBase +
                                   // min(k * kTile, capacity): the first read that starts at or above e_k, and above e_k
    uint8_t* seq;
    uint64_t baseCapacity;
    uint64_t* readBases;
    int32_t* status;
    uint32_t* baseFrame;  // may be null
    float* baseScore;     // may be null
    uint8_t alphabet[128];
};

// the first r in [0, nreads) with read_frames[r] >= v, or nreads; ends on any data
__device__ __forceinline__ uint64_t first_start_at_or_above(const Args& a, uint64_t v)
{
    uint64_t lo = 0, hi = a.nreads;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (a.readFrames[mid] < v)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// A tile: frames [A, A + nf) of the window, and the reads rLo <= rHi < nreads between which every frame of
// it finds its read.
struct Tile {
    uint64_t A;
    uint32_t nf;
    uint64_t rLo, rHi;
};
__device__ __forceinline__ Tile tile_of(const Args& a)
{
    Tile t;
    const uint64_t off = (uint64_t)blockIdx.x * kTile;
    t.A = a.frameBase + off;
    const uint64_t left = a.capacity > off ? a.capacity - off : 0;
    t.nf = left < kTile ? (uint32_t)left : kTile;
    t.rLo = t.rHi = 0;
    if (t.nf) {
        const uint64_t lo = a.bounds[2 * (uint64_t)blockIdx.x + 1], hi = a.bounds[2 * (uint64_t)blockIdx.x + 2];
        t.rLo = lo ? lo - 1 : 0;
        t.rHi = hi ? hi - 1 : 0;
        if (t.rHi < t.rLo) t.rHi = t.rLo;
    }
    return t;
}

// The reads at the tile edges, a thread per edge: every tile then finds its first and last read, and the reads
// whose start it owns, with two loads instead of three binary searches of dependent loads.
__global__ void ctc_bounds_kernel(Args a)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k > a.ntiles) return;
    const uint64_t off = k * kTile < a.capacity ? k * kTile : a.capacity;
    const uint64_t v = a.frameBase + off;
    a.bounds[2 * k] = (uint32_t)first_start_at_or_above(a, v);
    a.bounds[2 * k + 1] = v + 1 ? (uint32_t)first_start_at_or_above(a, v + 1) : (uint32_t)a.nreads;
}

// whether read [s, e) is taken: wholly inside the window
__device__ __forceinline__ bool read_taken(const Args& a, uint64_t s, uint64_t e)
{
    return s >= a.frameBase && s <= e && e - a.frameBase <= a.capacity;
}

// The read of frame i: the last r in [rLo, rHi] with read_frames[r] <= i.  True iff i is a frame of it and the
// read is taken; then r and its first frame are returned.
__device__ __forceinline__ bool frame_read(const Args& a, const Tile& t, uint64_t i, uint64_t& r, uint64_t& start)
{
    uint64_t lo = t.rLo, hi = t.rHi;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (a.readFrames[mid] <= i)
            lo = mid;
        else
            hi = mid - 1;
    }
    const uint64_t s = a.readFrames[lo], e = a.readFrames[lo + 1];
    r = lo;
    start = s;
    return s <= i && i < e && read_taken(a, s, e);
}

// The tile's frames are shared by kThreads threads in kPerThread rounds: frame j = k * kThreads + threadIdx.x
// in round k, so a wave's 64 frames of a round are neighbours and (round, wave) pairs follow in frame order.
// The number of set flags in the tile and, in before[k], in the frames below this thread's frame of round k.
__device__ __forceinline__ uint32_t tile_count(const bool (&flag)[kPerThread], uint32_t* waveCnt, uint32_t (&before)[kPerThread])
{
    constexpr uint32_t kWaves = kThreads / 64;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t mask[kPerThread];
#pragma unroll
    for (uint32_t k = 0; k < kPerThread; k++) {
        mask[k] = __ballot(flag[k]);
        if (lane == 0) waveCnt[k * kWaves + wave] = (uint32_t)__popcll(mask[k]);
    }
    __syncthreads();
    uint32_t all = 0;
#pragma unroll
    for (uint32_t k = 0; k < kPerThread; k++) {
#pragma unroll
        for (uint32_t w = 0; w < kWaves; w++) {
            if (w == wave) before[k] = all + (uint32_t)__popcll(mask[k] & ((1ull << lane) - 1));
            all += waveCnt[k * kWaves + w];
        }
    }
    __syncthreads();  // the next call writes waveCnt
    return all;
}

using Vec16 = uint32_t __attribute__((ext_vector_type(4)));

// The label pass.  Frames that are contiguous and at most kStageFrameBytes long come through LDS (dynamic,
// kTile frames + 16 bytes): the bytes of the tile's taken frames in 16-byte loads at 16-byte addresses, what
// lies in front of the first and behind the last such address element by element, so that no byte outside
// those frames is read.  Larger or strided frames are read by their own lane.
__global__ __launch_bounds__(kThreads) void ctc_label_kernel(Args a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t stage[];
    __shared__ uint8_t labels[kTile];
    __shared__ uint32_t waveCnt[kTile / 64];
    __shared__ uint32_t span[2];  // the tile's first taken frame and the one behind its last

    const Tile t = tile_of(a);
    const uint32_t tid = threadIdx.x;
    const uint32_t fbz = a.classes * a.elem;
    bool mine[kPerThread];
    uint64_t start[kPerThread];
    if (tid < 2) span[tid] = tid ? 0u : kTile;
#pragma unroll
    for (uint32_t k = 0; k < kPerThread; k++) {
        const uint32_t j = k * kThreads + tid;
        uint64_t r;
        start[k] = 0;
        mine[k] = j < t.nf && frame_read(a, t, t.A + j, r, start[k]);
    }

    uint32_t label[kPerThread];
    if (a.staged) {
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < kPerThread; k++) {
            const uint64_t mask = __ballot(mine[k]);
            const uint32_t j0 = (k * kThreads + tid) & ~63u;
            if ((tid & 63u) == 0 && mask) {
                atomicMin(&span[0], j0 + (uint32_t)__builtin_ctzll(mask));
                atomicMax(&span[1], j0 + 64u - (uint32_t)__builtin_clzll(mask));
            }
        }
        __syncthreads();
        const uint32_t lo = span[0], hi = span[1];
        uint32_t mis = 0;
        if (lo < hi) {
            const uint8_t* g0 = a.frames + (t.A - a.frameBase + lo) * (uint64_t)fbz;
            const uint32_t bytes = (hi - lo) * fbz;
            mis = (uint32_t)((uintptr_t)g0 & 15u);
            const uint32_t toBoundary = (16u - mis) & 15u;
            const uint32_t head = toBoundary < bytes ? toBoundary : bytes;
            const uint32_t nvec = (bytes - head) >> 4, tailAt = head + (nvec << 4);
            const uint32_t ends = (head + (bytes - tailAt)) / a.elem;  // elements in front and behind: < 16
            if (tid < ends) {
                const uint32_t e = tid * a.elem, off = e < head ? e : tailAt + (e - head);
                for (uint32_t b = 0; b < a.elem; b++) stage[mis + off + b] = g0[off + b];
            }
            const Vec16* src = reinterpret_cast<const Vec16*>(g0 + head);
            Vec16* dst = reinterpret_cast<Vec16*>(stage + mis + head);
            for (uint32_t v = tid; v < nvec; v += kThreads) dst[v] = src[v];
        }
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < kPerThread; k++) {
            const uint32_t j = k * kThreads + tid;
            label[k] = mine[k] ? argmax_frame(stage + mis + (j - lo) * fbz, a.classes, a.elem) : 0xFFu;
        }
    } else {
#pragma unroll
        for (uint32_t k = 0; k < kPerThread; k++) {
            const uint64_t i = t.A + k * kThreads + tid;
            label[k] = mine[k] ? argmax_frame(a.frames + (i - a.frameBase) * a.frameStride, a.classes, a.elem) : 0xFFu;
        }
    }
#pragma unroll
    for (uint32_t k = 0; k < kPerThread; k++) labels[k * kThreads + tid] = (uint8_t)label[k];
    __syncthreads();

    bool emit[kPerThread];
#pragma unroll
    for (uint32_t k = 0; k < kPerThread; k++) {
        const uint32_t j = k * kThreads + tid;
        const uint64_t i = t.A + j;
        emit[k] = false;
        if (mine[k]) {
            emit[k] = label[k] != a.blank;
            if (emit[k] && i != start[k]) {
                // the predecessor is a frame of the same read: taken, so inside the window; the tile's first
                // frame finds it in the tile before and computes its label again
                const uint32_t prev = j ? labels[j - 1]
                                        : argmax_frame(a.frames + (i - 1 - a.frameBase) * a.frameStride, a.classes, a.elem);
                emit[k] = label[k] != prev;
            }
            a.codes[i - a.frameBase] = (uint8_t)(label[k] | (emit[k] ? 0x80u : 0u));
        }
    }
    uint32_t before[kPerThread];
    const uint32_t all = tile_count(emit, waveCnt, before);
    if (tid == 0) a.tileSums[blockIdx.x] = all;
}

// The collapse call's count: the emitting codes of every tile's taken frames.
__global__ __launch_bounds__(kThreads) void ctc_count_kernel(Args a)
{
    __shared__ uint32_t waveCnt[kTile / 64];
    const Tile t = tile_of(a);
    bool emit[kPerThread];
#pragma unroll
    for (uint32_t k = 0; k < kPerThread; k++) {
        const uint32_t j = k * kThreads + threadIdx.x;
        const uint64_t i = t.A + j;
        uint64_t r, start;
        emit[k] = j < t.nf && frame_read(a, t, i, r, start) && (a.codes[i - a.frameBase] & 0x80u);
    }
    uint32_t before[kPerThread];
    const uint32_t all = tile_count(emit, waveCnt, before);
    if (threadIdx.x == 0) a.tileSums[blockIdx.x] = all;
}

// The exclusive scan of the tile counts in place, kScanSpan of them per workgroup (kScanPerThread per thread);
// each workgroup's total goes to spanSums, whose own exclusive scan (stitch_scan_kernel, one workgroup) follows:
// a tile's offset is its scanned count plus its span's.
__global__ __launch_bounds__(kScanThreads) void ctc_scan_kernel(Args a)
{
    __shared__ uint64_t waveSum[kScanThreads / 64];
    const uint64_t b0 = (uint64_t)blockIdx.x * kScanSpan + (uint64_t)threadIdx.x * kScanPerThread;
    uint64_t v[kScanPerThread], sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < kScanPerThread; k++) {
        v[k] = b0 + k < a.ntiles ? a.tileSums[b0 + k] : 0;
        sum += v[k];
    }
    uint64_t run;
    const uint64_t all = stitch::block_scan(sum, waveSum, run);
#pragma unroll
    for (uint32_t k = 0; k < kScanPerThread; k++) {
        if (b0 + k < a.ntiles) a.tileSums[b0 + k] = run;
        run += v[k];
    }
    if (threadIdx.x == 0) a.spanSums[blockIdx.x] = all;
}

// The write pass: the bases of the tile's emitting frames, and read_bases[r] of the reads whose start,
// clamped into the window, lies in the tile (the last tile also owns a start at the window's end).
__global__ __launch_bounds__(kThreads) void ctc_write_kernel(Args a)
{
    __shared__ uint32_t waveCnt[kTile / 64];
    __shared__ uint32_t pre[kTile + 1];  // emitting frames of the tile below local frame j; pre[nf] is all of them

    const Tile t = tile_of(a);
    const uint32_t tid = threadIdx.x;
    bool emit[kPerThread];
    uint32_t code[kPerThread];
    uint64_t start[kPerThread];
#pragma unroll
    for (uint32_t k = 0; k < kPerThread; k++) {
        const uint32_t j = k * kThreads + tid;
        const uint64_t i = t.A + j;
        uint64_t r;
        start[k] = 0;
        const bool mine = j < t.nf && frame_read(a, t, i, r, start[k]);
        code[k] = mine ? a.codes[i - a.frameBase] : 0u;
        emit[k] = (code[k] & 0x80u) != 0;
    }
    uint32_t before[kPerThread];
    const uint32_t all = tile_count(emit, waveCnt, before);
    const uint64_t tileOff = a.tileSums[blockIdx.x] + a.spanSums[blockIdx.x / kScanSpan];
    if (tid == 0) pre[kTile] = all;
#pragma unroll
    for (uint32_t k = 0; k < kPerThread; k++) {
        const uint32_t j = k * kThreads + tid;
        const uint64_t i = t.A + j;
        pre[j] = before[k];
        const uint64_t gi = tileOff + before[k];
        if (emit[k] && gi < a.baseCapacity) {
            const uint32_t cls = code[k] & 0x7Fu;
            a.seq[gi] = a.alphabet[cls];
            if (a.baseFrame) a.baseFrame[gi] = (uint32_t)(i - start[k]);
            if (a.baseScore) a.baseScore[gi] = score_at(a.frames + (i - a.frameBase) * a.frameStride, cls, a.elem);
        }
    }
    __syncthreads();

    const bool firstTile = blockIdx.x == 0, lastTile = blockIdx.x + 1 == a.ntiles;
    const uint64_t B = t.A + t.nf;
    const uint64_t rA = firstTile ? 0 : a.bounds[2 * (uint64_t)blockIdx.x];
    const uint64_t rB = lastTile ? a.nreads : a.bounds[2 * (uint64_t)blockIdx.x + 2];
    for (uint64_t q = rA + tid; q < rB; q += kThreads) {
        const uint64_t s = a.readFrames[q];
        const uint64_t x = s < t.A ? t.A : s > B ? B : s;
        a.readBases[q] = tileOff + pre[(uint32_t)(x - t.A)];
    }
}

// status of every read, and read_bases[nreads]
__global__ void ctc_status_kernel(Args a)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > a.nreads) return;
    const uint64_t total = a.spanSums[a.nspans];
    if (r == a.nreads) {
        a.readBases[r] = total;
        return;
    }
    const uint64_t b0 = a.readBases[r], b1 = r + 1 < a.nreads ? a.readBases[r + 1] : total;
    int32_t st = PGN_ERR_INVALID_ARG;
    if (read_taken(a, a.readFrames[r], a.readFrames[r + 1])) st = b1 > b0 && b1 > a.baseCapacity ? PGN_ERR_DST_TOO_SMALL : PGN_OK;
    a.status[r] = st;
}
#endif  // PGN_SELECT_HOST_ONLY

}  // namespace ctc
}  // namespace pgn

#endif  // PGN_CTC_H
