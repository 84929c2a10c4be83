// pgn_stitch.h -- per-segment model output back into whole reads (include/pgnano_hip.h "Model output back
// to reads"): which frames of every row are kept and where they go (the plan), and the ragged copy of one
// model batch's kept frames into the dense per-read layout (the rows call).
//
// The plan for a batch, all of it on the device:
//   the kept frames [first, first + count) of every table row (grid over rows, 1,024 per workgroup) and each
//   workgroup's frame total -> the exclusive scan of those totals (one workgroup, pgn_segment.h's
//   count-and-scan) -> dst_frame = the exclusive scan of count over the rows, per workgroup -> read_frames.
// Reads are in read order and a read's segments in start order, so the scan over all rows is at once the
// prefix over a read's segments and the scan over the reads: no loop runs over one read's segments.
#ifndef PGN_STITCH_H
#define PGN_STITCH_H

#include "pgn_segment.h"

namespace pgn {
namespace stitch {

// PGN_ERR_INVALID_ARG conditions of the parameters, in the header's order
inline bool params_valid(const pgn_stitch_params* P)
{
    if (!P) return false;
    if (P->frame_samples < 1 || P->length < 1 || P->length > seg::kMaxLength) return false;
    if (P->length % P->frame_samples) return false;
    return P->overlap <= P->length && P->frame_samples <= P->length - P->overlap;
}

// ceil(x / s)
PGN_HD uint64_t ceil_div(uint64_t x, uint32_t s) { return (x + s - 1) / s; }

// The kept frames of segment j of a taken read: a, aPrev, aNext are the starts of segments j, j - 1, j + 1
// (any common origin; aPrev is not looked at for the first segment, aNext not for the last).  A table that
// breaks aPrev <= a <= aNext <= a + L gives some count, never first + count > T.
PGN_HD void kept_frames(uint64_t aPrev, uint64_t a, uint64_t aNext, uint32_t valid, bool isFirst, bool isLast,
                        uint32_t L, uint32_t s, uint32_t T, uint32_t& first, uint32_t& count)
{
    const uint64_t lo = isFirst ? 0 : (aPrev + L - a) / 2;                      // c_{j-1} - a_j
    const uint64_t hi = isLast ? valid : (aNext - a) + (a + L - aNext) / 2;     // c_j - a_j
    const uint64_t f = ceil_div(lo, s), e = ceil_div(hi, s);
    const uint64_t end = e < T ? e : T;
    first = (uint32_t)(f < T ? f : T);
    count = end > f ? (uint32_t)(end - f) : 0u;
}

#ifndef PGN_SELECT_HOST_ONLY
// =============================================================================================
// The plan
// =============================================================================================
constexpr uint32_t kPlanThreads = 1024;  // rows per workgroup of the count and the offset kernels

struct PlanArgs {
    uint64_t nreads;
    const pgn_read_segments* reads;
    const pgn_segment* segments;
    uint64_t capacity;
    uint32_t length, frameSamples, T;
    pgn_stitch_segment* plan;
    uint64_t* blockSums;   // context scratch: one per workgroup, then their total
    uint64_t nblocks;
    uint64_t* readFrames;  // nreads + 1
};

// rows the table holds: min(total, capacity)
__device__ __forceinline__ uint64_t table_rows(const PlanArgs& a)
{
    const pgn_read_segments& last = a.reads[a.nreads - 1];
    const uint64_t total = last.first_segment + last.nsegments;
    return total < a.capacity ? total : a.capacity;
}

// the sum of v over the workgroup's threads and, in `before`, over the threads below this one
__device__ __forceinline__ uint64_t block_scan(uint64_t v, uint64_t* waveSum, uint64_t& before)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t incl = v;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint64_t up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
    }
    if (lane == 63) waveSum[wave] = incl;
    __syncthreads();
    uint64_t lower = 0, all = 0;
#pragma unroll
    for (uint32_t i = 0; i < kPlanThreads / 64; i++) {
        const uint64_t w = waveSum[i];
        lower += i < wave ? w : 0;
        all += w;
    }
    __syncthreads();  // the next call writes waveSum
    before = lower + incl - v;
    return all;
}

// first and count of every row, and the workgroup's frame total.  A row's read is taken from the table; an
// entry that names no read, or not a segment of its read, keeps no frames.
__global__ __launch_bounds__(kPlanThreads) void stitch_count_kernel(PlanArgs a)
{
    __shared__ uint64_t waveSum[kPlanThreads / 64];
    const uint64_t nrows = table_rows(a);
    const uint64_t g = (uint64_t)blockIdx.x * kPlanThreads + threadIdx.x;
    uint32_t first = 0, count = 0;
    if (g < nrows) {
        const pgn_segment sg = a.segments[g];
        if (sg.read < a.nreads) {
            const pgn_read_segments rs = a.reads[sg.read];
            const uint64_t k = rs.nsegments, j = g - rs.first_segment;
            if (rs.status == PGN_OK && g >= rs.first_segment && j < k && rs.first_segment + k <= a.capacity) {
                const bool isFirst = j == 0, isLast = j == k - 1;
                const uint64_t aPrev = isFirst ? 0 : a.segments[g - 1].start;
                const uint64_t aNext = isLast ? 0 : a.segments[g + 1].start;
                kept_frames(aPrev, sg.start, aNext, sg.valid, isFirst, isLast, a.length, a.frameSamples, a.T, first, count);
            }
        }
        a.plan[g].first = first;
        a.plan[g].count = count;
    }
    uint64_t before;
    const uint64_t all = block_scan(count, waveSum, before);
    if (threadIdx.x == 0) a.blockSums[blockIdx.x] = all;
}

// The exclusive scan of the workgroups' totals in place, by one workgroup, 1,024 per step with the running
// total carried from step to step; the grand total goes behind them.
__global__ __launch_bounds__(kPlanThreads) void stitch_scan_kernel(PlanArgs a)
{
    __shared__ uint64_t waveSum[kPlanThreads / 64];
    uint64_t carry = 0;
    for (uint64_t base = 0; base < a.nblocks; base += kPlanThreads) {
        const uint64_t b = base + threadIdx.x;
        const uint64_t v = b < a.nblocks ? a.blockSums[b] : 0;
        uint64_t before;
        const uint64_t all = block_scan(v, waveSum, before);
        if (b < a.nblocks) a.blockSums[b] = carry + before;
        carry += all;
    }
    if (threadIdx.x == 0) a.blockSums[a.nblocks] = carry;
}

// dst_frame of every row: the workgroup's offset plus the scan of count inside it
__global__ __launch_bounds__(kPlanThreads) void stitch_offset_kernel(PlanArgs a)
{
    __shared__ uint64_t waveSum[kPlanThreads / 64];
    const uint64_t nrows = table_rows(a);
    const uint64_t g = (uint64_t)blockIdx.x * kPlanThreads + threadIdx.x;
    const uint64_t count = g < nrows ? a.plan[g].count : 0;
    uint64_t before;
    block_scan(count, waveSum, before);
    if (g < nrows) a.plan[g].dst_frame = a.blockSums[blockIdx.x] + before;
}

// read_frames[r] = dst_frame of the read's first row (a read without rows below the capacity starts where
// the rows end: the frame total); read_frames[nreads] = the frame total
__global__ void stitch_read_frames_kernel(PlanArgs a)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > a.nreads) return;
    const uint64_t nrows = table_rows(a);
    const uint64_t total = a.blockSums[a.nblocks];
    uint64_t v = total;
    if (r < a.nreads) {
        const uint64_t first = a.reads[r].first_segment;
        if (first < nrows) v = a.plan[first].dst_frame;
    }
    a.readFrames[r] = v;
}

// =============================================================================================
// The rows
// =============================================================================================
struct RowsArgs {
    const pgn_stitch_segment* plan;  // already moved to the batch's first row
    uint64_t nsegments;
    const uint8_t* rows;
    uint64_t rowStride, frameStride;
    uint32_t frameBytes, T;
    uint8_t* out;
    uint64_t frameBase, capacity;
    uint32_t log2Tpr;  // a piece is shared by 1 << log2Tpr threads of the 256
    uint32_t dense;    // frame_stride == frame_bytes: a row's kept frames are one piece, else each frame is one
};

constexpr uint32_t kRowsThreads = 256;
constexpr uint32_t kRowsSplit = 8;  // at most this many workgroups share one row (blockIdx.y)

using Vec16 = uint32_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ Vec16 load16(const uint8_t* p)  // any alignment
{
    Vec16 v;
    __builtin_memcpy(&v, p, 16);
    return v;
}

// `len` bytes from src to dst by the `tpr` threads of which this is number `tir`, as part `part` of `parts`
// (workgroups along blockIdx.y): the bytes in front of the destination's first 16-byte boundary and behind its
// last one go byte by byte (part 0), what lies between in whole 16-byte stores, four loads in flight per thread.
__device__ __forceinline__ void copy_piece(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, uint64_t len,
                                           uint32_t tir, uint32_t tpr, uint32_t part, uint32_t parts)
{
    const uint64_t toBoundary = (16u - (uint32_t)((uintptr_t)dst & 15u)) & 15u;
    const uint64_t head = toBoundary < len ? toBoundary : len;
    const uint64_t nvec = (len - head) >> 4;
    const uint64_t tailAt = head + (nvec << 4);
    const uint32_t ends = (uint32_t)(head + (len - tailAt));  // < 32
    if (part == 0)
        for (uint32_t i = tir; i < ends; i += tpr) {
            const uint64_t off = i < head ? i : tailAt + (i - head);
            dst[off] = src[off];
        }
    const uint8_t* __restrict__ s = src + head;
    Vec16* __restrict__ d = reinterpret_cast<Vec16*>(dst + head);
    const uint64_t step = (uint64_t)parts * tpr;
    for (uint64_t k = (uint64_t)part * tpr + tir; k < nvec; k += 4 * step) {
        const uint64_t k1 = k + step, k2 = k + 2 * step, k3 = k + 3 * step;
        Vec16 v0 = load16(s + (k << 4)), v1 = {}, v2 = {}, v3 = {};
        if (k1 < nvec) v1 = load16(s + (k1 << 4));
        if (k2 < nvec) v2 = load16(s + (k2 << 4));
        if (k3 < nvec) v3 = load16(s + (k3 << 4));
        d[k] = v0;
        if (k1 < nvec) d[k1] = v1;
        if (k2 < nvec) d[k2] = v2;
        if (k3 < nvec) d[k3] = v3;
    }
}

// The kept frames of rows [0, nsegments) of one batch.  Dense rows: a workgroup takes 256 >> log2Tpr rows at
// a time, one piece each, and blockIdx.y shares a long piece's 16-byte units.  Strided rows: a workgroup
// takes one row at a time and its 256 >> log2Tpr thread groups, with blockIdx.y, share the row's frames.
__global__ __launch_bounds__(kRowsThreads) void stitch_rows_kernel(RowsArgs a)
{
    const uint32_t tpr = 1u << a.log2Tpr, slots = kRowsThreads >> a.log2Tpr;
    const uint32_t slot = threadIdx.x >> a.log2Tpr, tir = threadIdx.x & (tpr - 1);
    const uint32_t rpb = a.dense ? slots : 1u;
    for (uint64_t row = (uint64_t)blockIdx.x * rpb + (a.dense ? slot : 0u); row < a.nsegments;
         row += (uint64_t)gridDim.x * rpb) {
        const pgn_stitch_segment e = a.plan[row];
        // kept frames [lo, hi) of the row, cut to the frames the row has and to those whose destination
        // index d(f) = dst_frame + (f - first) - frameBase lies in [0, capacity)
        uint64_t lo = e.first, hi = (uint64_t)e.first + e.count;
        if (hi > a.T) hi = a.T;
        if (lo >= hi) continue;
        if (e.dst_frame < a.frameBase) {
            const uint64_t skip = a.frameBase - e.dst_frame;
            if (skip >= hi - lo) continue;
            lo += skip;
        }
        const uint64_t d0 = e.dst_frame + (lo - e.first) - a.frameBase;  // >= 0
        if (d0 >= a.capacity) continue;
        if (hi - lo > a.capacity - d0) hi = lo + (a.capacity - d0);
        const uint8_t* src = a.rows + row * a.rowStride;
        uint8_t* dst = a.out + d0 * a.frameBytes;
        if (a.dense) {
            copy_piece(src + lo * a.frameBytes, dst, (hi - lo) * a.frameBytes, tir, tpr, blockIdx.y, gridDim.y);
        } else {
            for (uint64_t f = lo + (uint64_t)blockIdx.y * slots + slot; f < hi; f += (uint64_t)gridDim.y * slots)
                copy_piece(src + f * a.frameStride, dst + (f - lo) * a.frameBytes, a.frameBytes, tir, tpr, 0, 1);
        }
    }
}
#endif  // PGN_SELECT_HOST_ONLY

}  // namespace stitch
}  // namespace pgn

#endif  // PGN_STITCH_H
