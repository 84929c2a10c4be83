// pgn_segment.h -- head trimming and the cut of normalised reads into fixed-length, overlapping model
// segments (include/pgnano_hip.h "Trimmed, normalised model segments").
//
// The order of work for a batch of decoded int16 reads, all of it on the device:
//   head counts -> med/MAD of every head (pgn_select.h's selection) -> trim scan (one wave per read)
//   -> statistics of the trimmed reads (the same selection, the caller's parameters)
//   -> segment counts and their exclusive scan over the reads (one workgroup)
//   -> the segment table (one wave per read) -> the rows (grid over segments).
// The trim rule, the threshold, the segment count and start and the parameter checks are host/device
// code: libpgn_model.so (model_capi.hip) runs them on the CPU, the kernels below on the device.
#ifndef PGN_SEGMENT_H
#define PGN_SEGMENT_H

#include "pgn_select.h"

namespace pgn {
namespace seg {

constexpr uint32_t kMaxLength = 1u << 24;

// PGN_ERR_INVALID_ARG conditions of the parameters, in the header's order
inline bool trim_params_valid(const pgn_trim_params* T)
{
    if (!T) return false;
    if (T->max_samples > 0 && T->window < 1) return false;
    return isfinite(T->mad_mult) && isfinite(T->threshold_mads);
}
inline bool segment_params_valid(const pgn_segment_params* S)
{
    return S && S->length >= 1 && S->length <= kMaxLength && S->overlap < S->length;
}

// ---- trim ------------------------------------------------------------------------------------------
// The head whose med/MAD the scan needs: min(n, max_samples) samples, or 0 where no window is scanned
// (trimming off, no complete window, or a read the statistics reject).
PGN_HD uint32_t trim_head(const pgn_trim_params& T, uint64_t n)
{
    if (T.max_samples == 0 || (n >> 32)) return 0;
    const uint32_t H = n < T.max_samples ? (uint32_t)n : T.max_samples;
    return (uint64_t)H < (uint64_t)T.min_trim + T.window ? 0 : H;
}
// The trim of a read whose trim_head is 0.
PGN_HD uint32_t trim_unscanned(const pgn_trim_params& T, uint64_t n)
{
    if (T.max_samples == 0 || (n >> 32)) return 0;
    return n < T.min_trim ? (uint32_t)n : T.min_trim;
}

// thr = centre_h + threshold_mads * spread_h, every operation one binary32 rounding: the product is
// kept out of the add's reach so that no compiler contracts the two into an FMA.
PGN_HD float trim_threshold(const pgn_trim_params& T, int32_t m2, uint32_t mad4)
{
    const float spread = T.mad_mult * (0.25f * (float)mad4);
#ifdef __HIP_DEVICE_COMPILE__
    float centre = 0.5f * (float)m2, prod = T.threshold_mads * spread;
    asm("" : "+v"(centre), "+v"(prod));  // (the halving is exact, so fusing it would not change a bit either)
#else
    const float centre = 0.5f * (float)m2;
    volatile float prod = T.threshold_mads * spread;
#endif
    return centre + prod;
}
PGN_HD bool above(int16_t x, float thr) { return (float)x > thr; }

// Window w of the head covers [min_trim + w * window, + window).
PGN_HD uint32_t trim_windows(const pgn_trim_params& T, uint32_t H) { return (H - T.min_trim) / T.window; }
// The trim when the scan stops at window w.
PGN_HD uint32_t trim_at(const pgn_trim_params& T, uint32_t H, uint32_t w)
{
    const uint64_t e = (uint64_t)T.min_trim + ((uint64_t)w + 1) * T.window;  // <= H
    return e < H ? (uint32_t)e : T.min_trim;
}

// The scan as the header writes it, window by window (the host's form; trim_scan_wave is the device's).
inline uint32_t trim_scan(const int16_t* x, uint32_t H, const pgn_trim_params& T, float thr)
{
    const uint32_t W = trim_windows(T, H);
    bool seen = false;
    for (uint32_t w = 0; w < W; w++) {
        const int16_t* p = x + T.min_trim + (uint64_t)w * T.window;
        if (!seen) {
            uint32_t cnt = 0;
            for (uint32_t t = 0; t < T.window; t++) cnt += above(p[t], thr) ? 1u : 0u;
            seen = cnt > T.min_elements;
        }
        if (seen && !above(p[T.window - 1], thr)) return trim_at(T, H, w);
    }
    return T.min_trim;
}

// trim, and the head statistics behind it (0 where none were taken), of one read on the host
struct TrimResult {
    uint32_t trim;
    int32_t m2;
    uint32_t mad4;
    float thr;
};
inline TrimResult host_trim(const int16_t* x, uint64_t n, const pgn_trim_params& T)
{
    TrimResult r{0, 0, 0, 0.0f};
    const uint32_t H = trim_head(T, n);
    if (!H) {
        r.trim = trim_unscanned(T, n);
        return r;
    }
    const pgn_norm_params P{PGN_NORM_MEDMAD, 0, 0.0, 1.0, 1.0f, 1.0f, 1.0f, 0.0f};
    pgn_read_stats s;
    sel::host_read_stats(x, H, P, s);
    r.m2 = s.m2;
    r.mad4 = s.mad4;
    r.thr = trim_threshold(T, s.m2, s.mad4);
    r.trim = trim_scan(x, H, T, r.thr);
    return r;
}

// ---- segments --------------------------------------------------------------------------------------
// m samples -> segments of length L, stride S = L - overlap: the last one ends at the read's end.
PGN_HD uint64_t segment_count(uint64_t m, uint32_t L, uint32_t S)
{
    if (m == 0) return 0;
    if (m <= L) return 1;
    return (m - L + S - 1) / S + 1;
}
// segment j of them starts at this sample of the trimmed read
PGN_HD uint64_t segment_start(uint64_t m, uint32_t L, uint32_t S, uint64_t j)
{
    if (m <= L) return 0;
    const uint64_t a = j * S, last = m - L;
    return a < last ? a : last;
}
PGN_HD uint32_t segment_valid(uint64_t m, uint32_t L) { return m < L ? (uint32_t)m : L; }

#ifndef PGN_SELECT_HOST_ONLY
// =============================================================================================
// Kernels
// =============================================================================================
struct TrimArgs {
    const int16_t* samples;
    const uint64_t* offsets;        // per read, in elements
    const uint64_t* counts;
    const int32_t* statusIn;        // optional
    uint64_t nreads;
    pgn_trim_params prm;
    uint64_t* headN;                // out (prep): the head the selection takes, 0 for none
    const pgn_read_stats* headStats;  // in (trim): med/MAD of those heads
    pgn_read_segments* reads;       // out (trim): trim, head_m2, head_mad4, threshold
    uint64_t* trimOffsets;          // out (trim): the trimmed reads
    uint64_t* trimCounts;
};

__device__ inline bool status_bad(const int32_t* statusIn, uint64_t r) { return statusIn && statusIn[r] != PGN_OK; }

__global__ void trim_heads_kernel(TrimArgs a)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.nreads) return;
    a.headN[r] = status_bad(a.statusIn, r) ? 0 : trim_head(a.prm, a.counts[r]);
}

// The scan by one wave, 64 windows at a time: lane l counts window g + l and looks at its last sample;
// two ballots give the first window with a peak and, from there on, the first whose last sample is not
// above.  Every lane returns the trim.
__device__ __forceinline__ uint32_t trim_scan_wave(const int16_t* __restrict__ x, uint32_t H, const pgn_trim_params& T,
                                                   float thr, uint32_t lane)
{
    const uint32_t W = trim_windows(T, H);
    bool seen = false;
    for (uint64_t g = 0; g < W; g += 64) {
        const uint64_t w = g + lane;
        const bool valid = w < W;
        uint32_t cnt = 0;
        bool last = false;
        if (valid) {
            const int16_t* p = x + T.min_trim + w * T.window;
#pragma unroll 8
            for (uint32_t t = 0; t < T.window; t++) cnt += above(p[t], thr) ? 1u : 0u;
            last = above(p[T.window - 1], thr);
        }
        uint64_t stop = __ballot(valid && !last);
        if (!seen) {
            const uint64_t peak = __ballot(valid && cnt > T.min_elements);
            if (!peak) continue;
            seen = true;
            stop &= ~0ull << __builtin_ctzll(peak);
        }
        if (stop) return trim_at(T, H, (uint32_t)(g + (uint64_t)__builtin_ctzll(stop)));
    }
    return T.min_trim;
}

// One wave per read.  A read whose input status is not PGN_OK is left untrimmed.
__global__ __launch_bounds__(256) void trim_kernel(TrimArgs a)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint64_t r = (uint64_t)blockIdx.x * 4 + wave; r < a.nreads; r += (uint64_t)gridDim.x * 4) {
        const uint64_t n = a.counts[r];
        const bool bad = status_bad(a.statusIn, r);
        const uint32_t H = bad ? 0 : trim_head(a.prm, n);
        int32_t m2 = 0;
        uint32_t mad4 = 0, trim = 0;
        float thr = 0.0f;
        if (H) {
            m2 = a.headStats[r].m2;
            mad4 = a.headStats[r].mad4;
            thr = trim_threshold(a.prm, m2, mad4);
            trim = trim_scan_wave(a.samples + a.offsets[r], H, a.prm, thr, lane);
        } else if (!bad) {
            trim = trim_unscanned(a.prm, n);
        }
        if (lane == 0) {
            pgn_read_segments& o = a.reads[r];
            o.trim = trim;
            o.head_m2 = m2;
            o.head_mad4 = mad4;
            o.threshold = thr;
            a.trimOffsets[r] = a.offsets[r] + trim;
            a.trimCounts[r] = n - trim;
        }
    }
}

struct PlanArgs {
    uint64_t nreads;
    const int32_t* statusIn;      // optional
    const pgn_read_stats* stats;  // of the trimmed reads: n and status
    pgn_read_segments* reads;
    uint64_t* total;              // context scratch (the later kernels read it)
    uint64_t* totalOut;           // optional: the caller's
    uint64_t capacity;
    uint32_t length, stride;
    uint32_t trimOff;             // no trim kernel ran: this one clears the trim fields
};

constexpr uint32_t kScanThreads = 1024;

// Segment counts and their exclusive scan over all reads by one workgroup: 1,024 reads per step (wave
// scans by shuffles, the 16 wave totals through LDS), the running total carried from step to step.  The
// next step's loads are issued before this step's barriers.
__global__ __launch_bounds__(kScanThreads) void segment_scan_kernel(PlanArgs a)
{
    __shared__ uint64_t waveSum[kScanThreads / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    auto load = [&](uint64_t r, int32_t& status, uint64_t& m) {
        status = PGN_OK;
        m = 0;
        if (r < a.nreads) {
            status = status_bad(a.statusIn, r) ? a.statusIn[r] : a.stats[r].status;
            m = a.stats[r].n;
        }
    };
    uint64_t carry = 0, m, mNext;
    int32_t status, statusNext;
    load(tid, status, m);
    for (uint64_t base = 0; base < a.nreads; base += kScanThreads) {
        const uint64_t r = base + tid;
        load(r + kScanThreads, statusNext, mNext);
        const uint64_t nseg = status == PGN_OK ? segment_count(m, a.length, a.stride) : 0;
        uint64_t incl = nseg;
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint64_t up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        if (lane == 63) waveSum[wave] = incl;
        __syncthreads();
        uint64_t before = 0, all = 0;
#pragma unroll
        for (uint32_t i = 0; i < kScanThreads / 64; i++) {
            const uint64_t v = waveSum[i];
            before += i < wave ? v : 0;
            all += v;
        }
        if (r < a.nreads) {
            pgn_read_segments& o = a.reads[r];
            const uint64_t first = carry + before + incl - nseg;
            o.first_segment = first;
            o.nsegments = (uint32_t)nseg;
            o.status = nseg && first + nseg > a.capacity ? PGN_ERR_DST_TOO_SMALL : status;  // nseg: status is PGN_OK
            if (a.trimOff) {
                o.trim = 0;
                o.head_m2 = 0;
                o.head_mad4 = 0;
                o.threshold = 0.0f;
            }
        }
        carry += all;
        status = statusNext;
        m = mNext;
        __syncthreads();  // the next step writes waveSum
    }
    if (tid == 0) {
        *a.total = carry;
        if (a.totalOut) *a.totalOut = carry;
    }
}

struct TableArgs {
    uint64_t nreads;
    const pgn_read_segments* reads;
    const pgn_read_stats* stats;
    pgn_segment* segments;
    uint64_t capacity;
    uint32_t length, stride;
};

// One wave per read writes the read's table entries, those below the capacity.
__global__ __launch_bounds__(256) void segment_table_kernel(TableArgs a)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint64_t r = (uint64_t)blockIdx.x * 4 + wave; r < a.nreads; r += (uint64_t)gridDim.x * 4) {
        const pgn_read_segments rs = a.reads[r];
        if (rs.nsegments == 0 || rs.first_segment >= a.capacity) continue;
        const uint64_t m = a.stats[r].n;
        const uint64_t room = a.capacity - rs.first_segment;
        const uint64_t k = rs.nsegments < room ? rs.nsegments : room;
        const uint32_t valid = segment_valid(m, a.length);
        for (uint64_t j = lane; j < k; j += 64) {
            pgn_segment sg;
            sg.read = (uint32_t)r;
            sg.start = rs.trim + (uint32_t)segment_start(m, a.length, a.stride, j);
            sg.valid = valid;
            sg.pad = 0;
            a.segments[rs.first_segment + j] = sg;
        }
    }
}

struct WriteArgs {
    const int16_t* samples;
    const uint64_t* offsets;       // per read (untrimmed), in elements
    const pgn_read_stats* stats;   // of the trimmed reads: centre and spread
    const pgn_segment* segments;
    const uint64_t* total;
    void* out;
    uint64_t capacity;
    uint32_t length;
    uint32_t log2Tpr;              // a row is shared by 1 << log2Tpr threads of the 256
};

constexpr uint32_t kWriteThreads = 256;
constexpr uint32_t kWriteSplit = 8;  // at most this many workgroups share one row (blockIdx.y)

// elements of one 16-byte store: a thread's unit of work
template <class T>
constexpr uint32_t kUnit = 16 / sizeof(T);
// the 16 bytes of one store as a single value
template <class W>
using StoreVec = W __attribute__((ext_vector_type(4)));

// Rows [0, min(total, capacity)) of the output.  A thread takes the kUnit consecutive elements of one
// 16-byte store at a time (8 binary16 or 4 float32, so a wave's stores are contiguous): one load of their
// samples (any 2-byte boundary), the values, and the 16-byte store where the row starts on a 16-byte
// boundary.  The unit that holds the end of the valid samples or of the row goes element by element; the
// padding is +0.0.
template <class T>
__global__ __launch_bounds__(kWriteThreads) void segment_write_kernel(WriteArgs a)
{
    constexpr uint32_t E = kUnit<T>;
    const uint64_t total = *a.total;
    const uint64_t nrows = total < a.capacity ? total : a.capacity;
    const uint32_t tpr = 1u << a.log2Tpr, rpb = kWriteThreads >> a.log2Tpr;
    const uint32_t sub = threadIdx.x >> a.log2Tpr, tir = threadIdx.x & (tpr - 1);
    const uint32_t units = (a.length + E - 1) / E;
    for (uint64_t row = (uint64_t)blockIdx.x * rpb + sub; row < nrows; row += (uint64_t)gridDim.x * rpb) {
        const pgn_segment sg = a.segments[row];
        const pgn_read_stats* st = a.stats + sg.read;
        const float negc = -st->centre, inv = 1.0f / st->spread;
        const int16_t* __restrict__ src = a.samples + a.offsets[sg.read] + sg.start;
        T* __restrict__ dst = reinterpret_cast<T*>(a.out) + row * a.length;
        const bool aligned = ((uintptr_t)dst & 15u) == 0;
        for (uint32_t k = blockIdx.y * tpr + tir; k < units; k += gridDim.y * tpr) {
            const uint32_t e0 = k * E;
            const uint32_t nv = sg.valid > e0 ? (sg.valid - e0 < E ? sg.valid - e0 : E) : 0u;  // samples
            const uint32_t ne = a.length - e0 < E ? a.length - e0 : E;                          // elements
            uint32_t x[E];
            if (nv == E) {
                uint32_t w[E / 2];
                __builtin_memcpy(w, src + e0, 2 * E);
#pragma unroll
                for (uint32_t j = 0; j < E / 2; j++) {
                    x[2 * j] = w[j] & 0xFFFFu;
                    x[2 * j + 1] = w[j] >> 16;
                }
            } else {
#pragma unroll
                for (uint32_t j = 0; j < E; j++) x[j] = j < nv ? (uint32_t)(uint16_t)src[e0 + j] : 0u;
            }
            float f[E];
#pragma unroll
            for (uint32_t j = 0; j < E; j++) f[j] = j < nv ? sel::norm_value(x[j], negc, inv) : 0.0f;
            T* o = dst + e0;
            if constexpr (sizeof(T) == 4) {
                if (aligned && ne == E) {
                    // one vector value, not float4's four members: as four member stores the last one is
                    // merged with the other branch's and a 12-byte store is left here
                    const StoreVec<float> v = {f[0], f[1], f[2], f[3]};
                    *reinterpret_cast<StoreVec<float>*>(o) = v;
                } else {
#pragma unroll
                    for (uint32_t j = 0; j < E; j++)
                        if (j < ne) o[j] = f[j];
                }
            } else {
                uint32_t h[E];
#pragma unroll
                for (uint32_t j = 0; j < E; j++) h[j] = j < nv ? sel::norm_f16_bits(f[j]) : 0u;
                if (aligned && ne == E) {
                    const StoreVec<uint32_t> v = {h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16),
                                                  h[6] | (h[7] << 16)};
                    *reinterpret_cast<StoreVec<uint32_t>*>(o) = v;
                } else {
                    uint16_t* o16 = reinterpret_cast<uint16_t*>(o);
#pragma unroll
                    for (uint32_t j = 0; j < E; j++)
                        if (j < ne) o16[j] = (uint16_t)h[j];
                }
            }
        }
    }
}
#endif  // PGN_SELECT_HOST_ONLY

}  // namespace seg
}  // namespace pgn

#endif  // PGN_SEGMENT_H
