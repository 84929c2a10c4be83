// pgn_select.h -- per-read robust statistics (exact order statistics of int16 samples) and the
// normalised output built on them (include/pgnano_hip.h "Per-read normalised output").
//
// Exact radix selection.  A sample becomes an unsigned key whose order is the order wanted:
//   plain   key = x ^ 0x8000 (offset binary, 16 bits)           -- quantiles and the median
//   MAD     key = |2x - m2|  (17 bits, m2 = twice the median)   -- the median absolute deviation
// Pass 1 counts the keys' top 10 bits (1,024 coarse bins: 64 plain values or 128 MAD values wide),
// the rank walk places every requested rank in a coarse bin with a residual rank, pass 2 counts the
// low bits of the keys that fall in the chosen bins (one fine histogram per rank; ranks that share a
// coarse bin share it) and a second walk gives the value.  Counts are 32-bit: a read has < 2^32 samples.
//
// The part between the passes -- histogram + ranks -> coarse bin and residual rank -> value -- and
// the integer -> float step are host/device code: libpgn_model.so (model_capi.hip) runs them on the
// CPU over serially built histograms, the kernels below over LDS histograms.
#ifndef PGN_SELECT_H
#define PGN_SELECT_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/pgnano_hip.h"

#ifndef PGN_HD
#define PGN_HD __host__ __device__ inline
#endif

namespace pgn {
namespace sel {

constexpr uint32_t kCoarseBins = 1024;  // top 10 bits of a key
constexpr uint32_t kGroupBins = 4;      // the walk's first level sums this many coarse bins
constexpr uint32_t kGroups = kCoarseBins / kGroupBins;
constexpr uint32_t kPlainShift = 6, kMadShift = 7;  // key bits below the coarse bin
constexpr uint32_t kMaxFineBins = 1u << kMadShift;

PGN_HD uint32_t key_plain(int16_t x) { return (uint32_t)(uint16_t)x ^ 0x8000u; }
PGN_HD int32_t unkey_plain(uint32_t k) { return (int32_t)(int16_t)(uint16_t)(k ^ 0x8000u); }
PGN_HD uint32_t key_mad(int16_t x, int32_t m2)
{
    const int32_t d = 2 * (int32_t)x - m2;  // |d| <= 131070
    return (uint32_t)(d < 0 ? -d : d);
}

// k = floor(p * (double)(n - 1)): one binary64 multiply, then floor (n >= 1, 0 <= p <= 1)
PGN_HD uint32_t rank_of(double p, uint64_t n) { return (uint32_t)floor(p * (double)(n - 1)); }

struct Place {
    uint32_t bin, resid;  // the bin holding the rank, and the rank among that bin's keys
};

// One walk over hist[0, nbins) for every rank at once (each k[i] below the histogram's total, in any
// order): out[i].bin is the first bin whose running total passes k[i].  N is a compile-time count so
// that the per-rank state stays in registers on the device.
template <int N>
PGN_HD void walk_ranks(const uint32_t* hist, uint32_t nbins, const uint32_t (&k)[N], Place (&out)[N])
{
    bool done[N];
    for (int i = 0; i < N; i++) {  // a rank at or above the total would end in the last bin
        done[i] = false;
        out[i].bin = nbins - 1;
        out[i].resid = 0;
    }
    uint32_t cum = 0;
    for (uint32_t b = 0; b < nbins; b++) {
        const uint32_t h = hist[b];
        bool all = true;
        for (int i = 0; i < N; i++) {
            if (!done[i] && k[i] - cum < h) {  // cum <= k[i] while rank i is not placed
                out[i].bin = b;
                out[i].resid = k[i] - cum;
                done[i] = true;
            }
            all = all && done[i];
        }
        if (all) break;
        cum += h;
    }
}

// The coarse walk in two levels: groups[g] = sum of coarse[4g .. 4g + 3]; the ranks are placed in a
// group first (256 steps) and then among that group's four bins.
template <int N>
PGN_HD void locate(const uint32_t* groups, const uint32_t* coarse, const uint32_t (&k)[N], Place (&out)[N])
{
    Place g[N];
    walk_ranks<N>(groups, kGroups, k, g);
    for (int i = 0; i < N; i++) {
        const uint32_t k1[1] = {g[i].resid};
        Place p1[1];
        walk_ranks<1>(coarse + g[i].bin * kGroupBins, kGroupBins, k1, p1);
        out[i].bin = g[i].bin * kGroupBins + p1[0].bin;
        out[i].resid = p1[0].resid;
    }
}

// The key of a rank from its coarse place and the fine histogram of that coarse bin.
PGN_HD uint32_t refine(const Place& coarse, const uint32_t* fine, uint32_t shift)
{
    const uint32_t k[1] = {coarse.resid};
    Place f[1];
    walk_ranks<1>(fine, 1u << shift, k, f);
    return (coarse.bin << shift) | f[0].bin;
}

PGN_HD void stats_clear(pgn_read_stats& s, uint64_t n, int32_t status)
{
    s.n = n;
    s.status = status;
    s.q_lo = s.q_hi = 0;
    s.m2 = 0;
    s.mad4 = 0;
    s.centre = 0.0f;
    s.spread = 1.0f;
}

// integers -> centre and spread, one binary32 rounding per operation
PGN_HD void finish_quantile(const pgn_norm_params& P, int32_t a, int32_t b, pgn_read_stats& s)
{
    s.q_lo = (int16_t)a;
    s.q_hi = (int16_t)b;
    s.centre = P.centre_mult * (float)(a + b);
    float spread = P.spread_mult * (float)(b - a);
    if (spread < P.spread_floor) spread = P.spread_floor;
    s.spread = spread;
}
PGN_HD void finish_medmad(const pgn_norm_params& P, int32_t m2, uint32_t mad4, pgn_read_stats& s)
{
    s.m2 = m2;
    s.mad4 = mad4;
    s.centre = 0.5f * (float)m2;
    float spread = P.spread_mult * (0.25f * (float)mad4);
    if (spread < P.spread_floor) spread = P.spread_floor;
    s.spread = spread;
}

// PGN_ERR_INVALID_ARG conditions of the parameters, in the header's order
inline bool params_valid(const pgn_norm_params* P)
{
    if (!P) return false;
    if (P->mode != PGN_NORM_QUANTILE && P->mode != PGN_NORM_MEDMAD) return false;
    if (!(P->p_lo >= 0.0 && P->p_lo <= 1.0 && P->p_hi >= 0.0 && P->p_hi <= 1.0) || P->p_lo > P->p_hi) return false;
    if (!isfinite(P->centre_mult) || !isfinite(P->spread_mult)) return false;
    return P->spread_floor > 0.0f;
}

// ---- one read shared by several workgroups: the plan (include/pgnano_hip.h pgn_select_split) -----
// The parts a read of n samples is selected in: 1 (not split) up to split_min_samples and from 2^32 on,
// else ceil(n / part_samples) capped at PGN_SELECT_MAX_PARTS.  split_min_samples >= part_samples, so a
// split read has at least two parts.
PGN_HD uint32_t split_parts(uint64_t n, uint32_t splitMin, uint32_t partSamples)
{
    if (n <= splitMin || (n >> 32)) return 1;
    const uint64_t p = (n + partSamples - 1) / partSamples;
    return p < PGN_SELECT_MAX_PARTS ? (uint32_t)p : (uint32_t)PGN_SELECT_MAX_PARTS;
}
// Part j of `parts` covers [part_begin(j), part_begin(j + 1)): the parts tile [0, n) and, with
// parts <= n, none is empty (n < 2^32 and j <= 4096, so the product fits 64 bits).
PGN_HD uint64_t part_begin(uint64_t n, uint32_t parts, uint32_t j) { return (uint64_t)j * n / parts; }

// PGN_ERR_INVALID_ARG conditions of pgn_ctx_set_select_split
inline bool split_valid(const pgn_select_split* s)
{
    if (!s) return false;
    if (s->part_samples < 1024u || s->part_samples > (1u << 24)) return false;
    return s->split_min_samples >= s->part_samples && s->max_split_reads <= 65536u;
}

// ---- the selection on the host, over serially built histograms (libpgn_model.so) ---------------
template <bool MAD>
inline void host_select2(const int16_t* x, uint64_t n, int32_t m2, uint32_t kLo, uint32_t kHi, uint32_t& vLo, uint32_t& vHi)
{
    constexpr uint32_t shift = MAD ? kMadShift : kPlainShift;
    uint32_t coarse[kCoarseBins], groups[kGroups], fine[2][kMaxFineBins];
    for (uint32_t& c : coarse) c = 0;
    for (uint32_t& g : groups) g = 0;
    for (uint64_t i = 0; i < n; i++) coarse[(MAD ? key_mad(x[i], m2) : key_plain(x[i])) >> shift]++;
    for (uint32_t b = 0; b < kCoarseBins; b++) groups[b / kGroupBins] += coarse[b];
    const uint32_t k[2] = {kLo, kHi};
    Place pl[2];
    locate<2>(groups, coarse, k, pl);
    for (auto& f : fine)
        for (uint32_t& c : f) c = 0;
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t key = MAD ? key_mad(x[i], m2) : key_plain(x[i]);
        const uint32_t b = key >> shift, f = key & ((1u << shift) - 1);
        if (b == pl[0].bin) fine[0][f]++;
        else if (b == pl[1].bin) fine[1][f]++;
    }
    vLo = refine(pl[0], fine[0], shift);
    vHi = refine(pl[1], fine[pl[1].bin == pl[0].bin ? 0 : 1], shift);
}

inline void host_read_stats(const int16_t* x, uint64_t n, const pgn_norm_params& P, pgn_read_stats& s)
{
    stats_clear(s, n, PGN_OK);
    if (n == 0) return;
    if (n >> 32) {
        s.status = PGN_ERR_UNSUPPORTED;
        return;
    }
    uint32_t lo, hi;
    if (P.mode == PGN_NORM_QUANTILE) {
        host_select2<false>(x, n, 0, rank_of(P.p_lo, n), rank_of(P.p_hi, n), lo, hi);
        finish_quantile(P, unkey_plain(lo), unkey_plain(hi), s);
    } else {
        const uint32_t kLo = (uint32_t)((n - 1) / 2), kHi = (uint32_t)(n / 2);
        host_select2<false>(x, n, 0, kLo, kHi, lo, hi);
        const int32_t m2 = unkey_plain(lo) + unkey_plain(hi);
        host_select2<true>(x, n, m2, kLo, kHi, lo, hi);
        finish_medmad(P, m2, lo + hi, s);
    }
}

#ifndef PGN_SELECT_HOST_ONLY
// =============================================================================================
// Kernels
// =============================================================================================
constexpr uint32_t kSelThreads = 256;  // the long-read kernel's workgroup (four waves)
constexpr uint32_t kCopies = 8;        // sub-histograms: a lane counts in copy (lane & 7)
constexpr uint32_t kShortMax = 512;    // reads up to this long: one wave each, keys in registers
constexpr uint32_t kShortPerLane = kShortMax / 64;

struct StatsArgs {
    const int16_t* samples;
    const uint64_t* offsets;      // per read, in elements
    const uint64_t* counts;       // per read
    uint64_t nreads;
    pgn_norm_params prm;
    pgn_read_stats* stats;
    const int32_t* chunkStatus;   // optional: the decode's statuses and the reads' chunk ranges
    const uint64_t* firstChunk;
};

// a read's status: its first chunk status that is not PGN_OK, in chunk order
__device__ inline int32_t read_status(const StatsArgs& a, uint64_t r)
{
    if (!a.chunkStatus) return PGN_OK;
    for (uint64_t c = a.firstChunk[r]; c < a.firstChunk[r + 1]; c++)
        if (a.chunkStatus[c] != PGN_OK) return a.chunkStatus[c];
    return PGN_OK;
}

template <bool MAD>
__device__ __forceinline__ uint32_t key_of(uint32_t x16, int32_t m2)
{
    return MAD ? key_mad((int16_t)(uint16_t)x16, m2) : ((x16 & 0xFFFFu) ^ 0x8000u);
}

// Every key of p[0, n) through f, once, by the 256 threads of the workgroup.  A read starts on a
// 2-byte boundary: up to 7 samples before the first 16-byte boundary and up to 7 after the last
// whole vector go one per thread, the rest as 16-byte loads.
template <bool MAD, class F>
__device__ __forceinline__ void scan_keys(const int16_t* __restrict__ p, uint32_t n, int32_t m2, F f)
{
    const uint32_t tid = threadIdx.x;
    uint32_t head = (uint32_t)((16u - (uint32_t)((uintptr_t)p & 15u)) & 15u) >> 1;
    if (head > n) head = n;
    const uint32_t nvec = (n - head) >> 3;
    if (tid < head) f(key_of<MAD>((uint16_t)p[tid], m2));
    const uint4* __restrict__ q = reinterpret_cast<const uint4*>(p + head);
#pragma unroll 2
    for (uint32_t i = tid; i < nvec; i += kSelThreads) {
        const uint4 v = q[i];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            f(key_of<MAD>(w[j] & 0xFFFFu, m2));
            f(key_of<MAD>(w[j] >> 16, m2));
        }
    }
    const uint64_t t = (uint64_t)head + ((uint64_t)nvec << 3) + tid;
    if (t < n) f(key_of<MAD>((uint16_t)p[t], m2));
}

struct SelLds {
    alignas(16) uint32_t hist[kCoarseBins * kCopies];  // pass 1: [bin][copy]; pass 2: two fine histograms [fine][copy]
    uint32_t coarse[kCoarseBins];
    uint32_t groups[kGroups];
    uint32_t fine[2 * kMaxFineBins];
    Place place[2];
    uint32_t val[2];
};

// The keys of ranks kLo <= kHi of the read, by the whole workgroup (every thread returns both).
template <bool MAD>
__device__ void select2(const int16_t* __restrict__ p, uint32_t n, int32_t m2, uint32_t kLo, uint32_t kHi, SelLds& L,
                        uint32_t& vLo, uint32_t& vHi)
{
    constexpr uint32_t shift = MAD ? kMadShift : kPlainShift, fineBins = 1u << shift;
    const uint32_t tid = threadIdx.x, copy = tid & (kCopies - 1);
    uint4* h4 = reinterpret_cast<uint4*>(L.hist);
    for (uint32_t i = tid; i < kCoarseBins * kCopies / 4; i += kSelThreads) h4[i] = make_uint4(0, 0, 0, 0);
    __syncthreads();
    scan_keys<MAD>(p, n, m2, [&](uint32_t key) { atomicAdd(&L.hist[(key >> shift) * kCopies + copy], 1u); });
    __syncthreads();
    {  // thread t sums the copies of coarse bins 4t .. 4t + 3 (128 contiguous bytes) and their group
        uint32_t g = 0;
#pragma unroll
        for (uint32_t j = 0; j < kGroupBins; j++) {
            const uint4 a = h4[(tid * kGroupBins + j) * 2], b = h4[(tid * kGroupBins + j) * 2 + 1];
            const uint32_t s = a.x + a.y + a.z + a.w + b.x + b.y + b.z + b.w;
            L.coarse[tid * kGroupBins + j] = s;
            g += s;
        }
        L.groups[tid] = g;
    }
    __syncthreads();
    if (tid == 0) {
        const uint32_t k[2] = {kLo, kHi};
        Place pl[2];
        locate<2>(L.groups, L.coarse, k, pl);
        L.place[0] = pl[0];
        L.place[1] = pl[1];
    }
    for (uint32_t i = tid; i < 2 * fineBins * kCopies / 4; i += kSelThreads) h4[i] = make_uint4(0, 0, 0, 0);
    __syncthreads();
    const uint32_t bLo = L.place[0].bin, bHi = L.place[1].bin;
    scan_keys<MAD>(p, n, m2, [&](uint32_t key) {
        const uint32_t b = key >> shift, f = key & (fineBins - 1);
        if (b == bLo) atomicAdd(&L.hist[f * kCopies + copy], 1u);
        else if (b == bHi) atomicAdd(&L.hist[(fineBins + f) * kCopies + copy], 1u);
    });
    __syncthreads();
    if (tid < 2 * fineBins) {
        const uint4 a = h4[tid * 2], b = h4[tid * 2 + 1];
        L.fine[tid] = a.x + a.y + a.z + a.w + b.x + b.y + b.z + b.w;
    }
    __syncthreads();
    if (tid < 2) {
        const Place pl = L.place[tid];
        L.val[tid] = refine(pl, L.fine + ((tid == 1 && bHi != bLo) ? fineBins : 0), shift);
    }
    __syncthreads();
    vLo = L.val[0];
    vHi = L.val[1];
    __syncthreads();  // the next selection clears what this one read
}

// Reads above kShortMax samples: one workgroup per read, reads blockIdx.x, + gridDim.x, ...
__global__ __launch_bounds__(kSelThreads) void read_stats_kernel(StatsArgs a)
{
    __shared__ SelLds L;
    for (uint64_t r = blockIdx.x; r < a.nreads; r += gridDim.x) {
        const uint64_t n64 = a.counts[r];
        if (n64 <= kShortMax) continue;  // read_stats_short_kernel's
        pgn_read_stats s;
        stats_clear(s, n64, PGN_OK);
        if (n64 >> 32) {
            s.status = PGN_ERR_UNSUPPORTED;
        } else {
            const uint32_t n = (uint32_t)n64;
            const int16_t* p = a.samples + a.offsets[r];
            uint32_t lo, hi;
            if (a.prm.mode == PGN_NORM_QUANTILE) {
                select2<false>(p, n, 0, rank_of(a.prm.p_lo, n), rank_of(a.prm.p_hi, n), L, lo, hi);
                finish_quantile(a.prm, unkey_plain(lo), unkey_plain(hi), s);
            } else {
                const uint32_t kLo = (n - 1) / 2, kHi = n / 2;
                select2<false>(p, n, 0, kLo, kHi, L, lo, hi);
                const int32_t m2 = unkey_plain(lo) + unkey_plain(hi);
                select2<true>(p, n, m2, kLo, kHi, L, lo, hi);
                finish_medmad(a.prm, m2, lo + hi, s);
            }
        }
        if (threadIdx.x == 0) {
            if (s.status == PGN_OK) s.status = read_status(a, r);
            a.stats[r] = s;
        }
    }
}

// The key of rank k among the wave's keys (8 per lane, absent ones 0xFFFFFFFF), bit by bit from the
// top: the largest v with fewer than k + 1 keys below it.  Counts are ballots, so every lane agrees.
__device__ __forceinline__ uint32_t wave_select(const uint32_t (&key)[kShortPerLane], uint32_t k, int bits)
{
    uint32_t ans = 0;
    for (int b = bits - 1; b >= 0; b--) {
        const uint32_t trial = ans | (1u << b);
        uint32_t c = 0;
#pragma unroll
        for (uint32_t j = 0; j < kShortPerLane; j++) c += (uint32_t)__popcll(__ballot(key[j] < trial));
        if (c <= k) ans = trial;
    }
    return ans;
}

// Reads up to kShortMax samples (n = 0 included): one wave per read, no LDS, no barrier.
__global__ __launch_bounds__(kSelThreads) void read_stats_short_kernel(StatsArgs a)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    constexpr uint32_t kWaves = kSelThreads / 64;
    for (uint64_t r = (uint64_t)blockIdx.x * kWaves + wave; r < a.nreads; r += (uint64_t)gridDim.x * kWaves) {
        const uint64_t n64 = a.counts[r];
        if (n64 > kShortMax) continue;
        const uint32_t n = (uint32_t)n64;
        pgn_read_stats s;
        stats_clear(s, n64, PGN_OK);
        if (n) {
            const int16_t* p = a.samples + a.offsets[r];
            uint32_t x[kShortPerLane], key[kShortPerLane];
#pragma unroll
            for (uint32_t j = 0; j < kShortPerLane; j++) {
                const uint32_t i = j * 64 + lane;
                x[j] = i < n ? (uint32_t)(uint16_t)p[i] : 0u;
                key[j] = i < n ? key_of<false>(x[j], 0) : 0xFFFFFFFFu;
            }
            if (a.prm.mode == PGN_NORM_QUANTILE) {
                const uint32_t lo = wave_select(key, rank_of(a.prm.p_lo, n), 16);
                const uint32_t hi = wave_select(key, rank_of(a.prm.p_hi, n), 16);
                finish_quantile(a.prm, unkey_plain(lo), unkey_plain(hi), s);
            } else {
                const uint32_t kLo = (n - 1) / 2, kHi = n / 2;
                const int32_t m2 = unkey_plain(wave_select(key, kLo, 16)) + unkey_plain(wave_select(key, kHi, 16));
#pragma unroll
                for (uint32_t j = 0; j < kShortPerLane; j++)
                    key[j] = j * 64 + lane < n ? key_of<true>(x[j], m2) : 0xFFFFFFFFu;
                finish_medmad(a.prm, m2, wave_select(key, kLo, 17) + wave_select(key, kHi, 17), s);
            }
        }
        if (lane == 0) {
            s.status = read_status(a, r);
            a.stats[r] = s;
        }
    }
}

// ---- one read shared by several workgroups ------------------------------------------------------------
// A read above split_min_samples takes a slot (while there are slots) and is selected in parts: every
// part's histogram is added to the slot's with integer atomics, and the rank walk and the refinement run
// once per slot on the sums.  The order on the stream is classify -> plan -> (the kernels above) ->
// coarse parts -> place -> fine parts -> finish (med/MAD: the last four again with MAD keys); every
// dependency is a kernel boundary, and no workgroup waits for another inside a kernel.
struct SplitSlot {
    alignas(16) uint32_t coarse[kCoarseBins];  // the parts' coarse histograms, summed
    uint32_t fine[2 * kMaxFineBins];           // the two fine histograms, the second at 1 << shift
    Place place[2];
    uint64_t read;
    int32_t m2;
    uint32_t pad;
};
static_assert(sizeof(SplitSlot) % 16 == 0 && offsetof(SplitSlot, fine) == sizeof(uint32_t) * kCoarseBins, "slot layout");
constexpr uint32_t kSlotHistVecs = (kCoarseBins + 2 * kMaxFineBins) / 4;  // the histograms as 16-byte words

struct SplitHead {
    uint32_t nslots, nitems;  // slots handed out, and their parts: the work items of the parts kernels
    uint64_t counts[5];       // pgn_select_split_counts
};

struct SplitBlock {         // what the plan needs of 512 consecutive reads
    uint32_t qual, nshort;  // reads above split_min_samples and below 2^32; reads of at most kShortMax samples
    uint64_t parts;         // the parts of the former
};

struct SplitArgs {
    StatsArgs a;
    uint32_t splitMin, partSamples, maxSlots, pad;
    uint64_t* wholeCounts;  // out (plan): per read, its count as read_stats_kernel is to see it -- 0 (a read
                            // it skips) where the read holds a slot
    SplitBlock* blocks;     // out (classify): one per 512 reads
    SplitHead* head;
    uint32_t* itemFirst;    // maxSlots + 1: the first work item of every slot, then their count
    SplitSlot* slots;
};

// the reads of one classify block and the plan's workgroup: 512 threads leave the plan 256 registers a
// thread, which it needs to stay out of scratch
constexpr uint32_t kPlanThreads = 512;

// Classification, across the device: one block per 512 consecutive reads writes the block's totals
// and copies the reads' counts for the one-workgroup kernel (the plan zeroes those of the reads it
// gives slots).
__global__ __launch_bounds__(kPlanThreads) void split_classify_kernel(SplitArgs s)
{
    __shared__ unsigned long long tot[3];
    const uint32_t tid = threadIdx.x;
    if (tid < 3) tot[tid] = 0;
    __syncthreads();
    const uint64_t r = (uint64_t)blockIdx.x * kPlanThreads + tid;
    const bool valid = r < s.a.nreads;
    const uint64_t n = valid ? s.a.counts[r] : 0;
    if (valid) s.wholeCounts[r] = n;
    const uint32_t parts = split_parts(n, s.splitMin, s.partSamples);
    const uint64_t qual = __ballot(parts > 1), small = __ballot(valid && n <= kShortMax);
    if ((tid & 63u) == 0) {
        if (qual) atomicAdd(&tot[0], (unsigned long long)__popcll(qual));
        if (small) atomicAdd(&tot[1], (unsigned long long)__popcll(small));
    }
    if (parts > 1) atomicAdd(&tot[2], (unsigned long long)parts);
    __syncthreads();
    if (tid == 0) {
        SplitBlock b;
        b.qual = (uint32_t)tot[0];
        b.nshort = (uint32_t)tot[1];
        b.parts = tot[2];
        s.blocks[blockIdx.x] = b;
    }
}

// Exclusive scan of (q, p) over the plan's workgroup (shuffles inside a wave, the 16 wave totals through
// LDS), with the totals.
__device__ __forceinline__ void plan_scan(uint32_t q, uint64_t p, uint32_t* waveQual, uint64_t* waveParts, uint64_t& exQ,
                                          uint64_t& exP, uint64_t& allQ, uint64_t& allP)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inclQ = q;
    uint64_t inclP = p;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t upQ = __shfl_up(inclQ, d);
        const uint64_t upP = __shfl_up(inclP, d);
        if (lane >= d) {
            inclQ += upQ;
            inclP += upP;
        }
    }
    if (lane == 63) {
        waveQual[wave] = inclQ;
        waveParts[wave] = inclP;
    }
    __syncthreads();
    uint64_t beforeQ = 0, beforeP = 0;
    allQ = allP = 0;
#pragma unroll
    for (uint32_t i = 0; i < kPlanThreads / 64; i++) {
        const uint64_t wq = waveQual[i], wp = waveParts[i];
        beforeQ += i < wave ? wq : 0;
        beforeP += i < wave ? wp : 0;
        allQ += wq;
        allP += wp;
    }
    exQ = beforeQ + inclQ - q;
    exP = beforeP + inclP - p;
    __syncthreads();  // the next scan writes the wave totals
}

// The plan, by one workgroup (pgn_segment.h's count-and-scan, over the classify blocks' totals, 512
// blocks per step): the slots go out in read order and the work items (slot, part) are numbered; only a
// block that holds a read above split_min_samples is looked at read by read.  Then the counters, and the
// histograms of the slots used are cleared.
__global__ __launch_bounds__(kPlanThreads) void split_plan_kernel(SplitArgs s)
{
    __shared__ uint64_t waveParts[kPlanThreads / 64];
    __shared__ uint32_t waveQual[kPlanThreads / 64];
    __shared__ uint32_t blkQual[kPlanThreads];
    __shared__ uint64_t blkSlot[kPlanThreads], blkItem[kPlanThreads];  // a block's first slot and work item
    __shared__ unsigned long long cnt[2];
    const uint32_t tid = threadIdx.x;
    if (tid < 2) cnt[tid] = 0;
    const uint64_t nblocks = (s.a.nreads + kPlanThreads - 1) / kPlanThreads;
    uint64_t carryQ = 0, carryP = 0;  // qualifying reads and their parts so far
    uint64_t nShort = 0;
    uint32_t nParts = 0;
    for (uint64_t bbase = 0; bbase < nblocks; bbase += kPlanThreads) {
        SplitBlock info{0, 0, 0};
        if (bbase + tid < nblocks) info = s.blocks[bbase + tid];
        uint64_t exQ, exP, allQ, allP;
        plan_scan(info.qual, info.parts, waveQual, waveParts, exQ, exP, allQ, allP);
        blkQual[tid] = info.qual;
        blkSlot[tid] = carryQ + exQ;
        blkItem[tid] = carryP + exP;
        nShort += info.nshort;
        __syncthreads();
        const uint32_t nb = nblocks - bbase < kPlanThreads ? (uint32_t)(nblocks - bbase) : kPlanThreads;
        for (uint32_t i = 0; i < nb; i++) {
            // the reads that qualify before a read all hold slots while slot < maxSlots, so their parts
            // are the work items before that read's; the read with slot == maxSlots marks their end
            if (blkQual[i] == 0 || blkSlot[i] > s.maxSlots) continue;
            const uint64_t r = (bbase + i) * kPlanThreads + tid;
            const uint64_t n = r < s.a.nreads ? s.a.counts[r] : 0;
            const uint32_t parts = split_parts(n, s.splitMin, s.partSamples);
            const uint32_t q = parts > 1 ? 1u : 0u;
            uint64_t inQ, inP, blockQ, blockP;
            plan_scan(q, q ? parts : 0u, waveQual, waveParts, inQ, inP, blockQ, blockP);
            const uint64_t slot = blkSlot[i] + inQ, item = blkItem[i] + inP;
            if (q && slot < s.maxSlots) {
                s.wholeCounts[r] = 0;
                s.itemFirst[slot] = (uint32_t)item;
                s.slots[slot].read = r;
                nParts += parts;
            } else if (q && slot == s.maxSlots) {
                s.itemFirst[slot] = (uint32_t)item;
            }
        }
        carryQ += allQ;
        carryP += allP;
        __syncthreads();  // the next step writes the blocks' arrays
    }
    atomicAdd(&cnt[0], (unsigned long long)nShort);
    atomicAdd(&cnt[1], (unsigned long long)nParts);
    __syncthreads();
    const uint32_t nslots = carryQ < s.maxSlots ? (uint32_t)carryQ : s.maxSlots;
    if (tid == 0) {
        if (carryQ <= s.maxSlots) s.itemFirst[carryQ] = (uint32_t)carryP;
        s.head->nslots = nslots;
        s.head->nitems = (uint32_t)cnt[1];
        s.head->counts[0] = cnt[0];
        s.head->counts[1] = s.a.nreads - cnt[0] - nslots;
        s.head->counts[2] = nslots;
        s.head->counts[3] = cnt[1];
        s.head->counts[4] = carryQ - nslots;
    }
    for (uint64_t i = tid; i < (uint64_t)nslots * kSlotHistVecs; i += kPlanThreads)
        reinterpret_cast<uint4*>(s.slots + i / kSlotHistVecs)[i % kSlotHistVecs] = make_uint4(0, 0, 0, 0);
}

// The histogram of one part of a split read, added to its slot's: pass 1 (FINE false) counts the keys'
// coarse bins, pass 2 the low bits of the keys in the two placed bins, as select2 does for a whole read.
// A fixed grid loops over the work items; item -> slot by bisection of itemFirst.
template <bool MAD, bool FINE>
__global__ __launch_bounds__(kSelThreads) void split_parts_kernel(SplitArgs s)
{
    constexpr uint32_t shift = MAD ? kMadShift : kPlainShift, fineBins = 1u << shift;
    constexpr uint32_t bins = FINE ? 2 * fineBins : kCoarseBins;
    __shared__ alignas(16) uint32_t hist[bins * kCopies];  // [bin][copy]
    const uint32_t tid = threadIdx.x, copy = tid & (kCopies - 1);
    const uint32_t nitems = s.head->nitems, nslots = s.head->nslots;
    uint4* h4 = reinterpret_cast<uint4*>(hist);
    for (uint32_t item = blockIdx.x; item < nitems; item += gridDim.x) {
        uint32_t lo = 0, hi = nslots;  // itemFirst[lo] <= item < itemFirst[hi]
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (s.itemFirst[mid] <= item) lo = mid;
            else hi = mid;
        }
        SplitSlot& S = s.slots[lo];
        const uint32_t first = s.itemFirst[lo], parts = s.itemFirst[lo + 1] - first, j = item - first;
        const uint64_t r = S.read, n = s.a.counts[r];
        const uint64_t b0 = part_begin(n, parts, j), b1 = part_begin(n, parts, j + 1);
        const int16_t* p = s.a.samples + s.a.offsets[r] + b0;
        const int32_t m2 = MAD ? S.m2 : 0;
        for (uint32_t i = tid; i < bins * kCopies / 4; i += kSelThreads) h4[i] = make_uint4(0, 0, 0, 0);
        __syncthreads();
        if constexpr (FINE) {
            const uint32_t bLo = S.place[0].bin, bHi = S.place[1].bin;
            scan_keys<MAD>(p, (uint32_t)(b1 - b0), m2, [&](uint32_t key) {
                const uint32_t b = key >> shift, f = key & (fineBins - 1);
                if (b == bLo) atomicAdd(&hist[f * kCopies + copy], 1u);
                else if (b == bHi) atomicAdd(&hist[(fineBins + f) * kCopies + copy], 1u);
            });
        } else {
            scan_keys<MAD>(p, (uint32_t)(b1 - b0), m2,
                           [&](uint32_t key) { atomicAdd(&hist[(key >> shift) * kCopies + copy], 1u); });
        }
        __syncthreads();
        uint32_t* dst = FINE ? S.fine : S.coarse;
        for (uint32_t b = tid; b < bins; b += kSelThreads) {
            const uint4 u = h4[b * 2], v = h4[b * 2 + 1];
            const uint32_t sum = u.x + u.y + u.z + u.w + v.x + v.y + v.z + v.w;
            if (sum) atomicAdd(&dst[b], sum);
        }
        __syncthreads();  // the next item clears what this one read
    }
}

constexpr uint32_t kSlotThreads = 64;  // the place and finish kernels: one wave per slot

// The ranks of a slot's read in its summed coarse histogram: what thread 0 of select2 does.  `mad`: the
// second selection of med/MAD (the same ranks, MAD keys).
__global__ __launch_bounds__(kSlotThreads) void split_place_kernel(SplitArgs s, uint32_t mad)
{
    __shared__ alignas(16) uint32_t coarse[kCoarseBins];
    __shared__ uint32_t groups[kGroups];
    const uint32_t lane = threadIdx.x, nslots = s.head->nslots;
    for (uint32_t slot = blockIdx.x; slot < nslots; slot += gridDim.x) {
        SplitSlot& S = s.slots[slot];
        const uint32_t n = (uint32_t)s.a.counts[S.read];
        const uint4* c4 = reinterpret_cast<const uint4*>(S.coarse);
#pragma unroll
        for (uint32_t j = 0; j < kGroups / kSlotThreads; j++) {  // a 16-byte word is one group
            const uint4 v = c4[j * kSlotThreads + lane];
            reinterpret_cast<uint4*>(coarse)[j * kSlotThreads + lane] = v;
            groups[j * kSlotThreads + lane] = v.x + v.y + v.z + v.w;
        }
        __syncthreads();
        if (lane == 0) {
            const bool quantile = !mad && s.a.prm.mode == PGN_NORM_QUANTILE;
            const uint32_t k[2] = {quantile ? rank_of(s.a.prm.p_lo, n) : (n - 1) / 2,
                                   quantile ? rank_of(s.a.prm.p_hi, n) : n / 2};
            Place pl[2];
            locate<2>(groups, coarse, k, pl);
            S.place[0] = pl[0];
            S.place[1] = pl[1];
        }
        __syncthreads();  // the next slot overwrites the histogram
    }
}

// The two values from a slot's fine histograms, then the read's statistics -- or, after the median's
// selection of med/MAD, m2 and histograms cleared for the selection with MAD keys.
template <bool MAD>
__global__ __launch_bounds__(kSlotThreads) void split_finish_kernel(SplitArgs s)
{
    constexpr uint32_t shift = MAD ? kMadShift : kPlainShift, fineBins = 1u << shift;
    __shared__ alignas(16) uint32_t fine[2 * kMaxFineBins];
    __shared__ uint32_t val[2];
    const uint32_t lane = threadIdx.x, nslots = s.head->nslots;
    for (uint32_t slot = blockIdx.x; slot < nslots; slot += gridDim.x) {
        SplitSlot& S = s.slots[slot];
        reinterpret_cast<uint4*>(fine)[lane] = reinterpret_cast<const uint4*>(S.fine)[lane];
        __syncthreads();
        if (lane < 2) {
            const Place pl = S.place[lane];
            val[lane] = refine(pl, fine + ((lane == 1 && S.place[1].bin != S.place[0].bin) ? fineBins : 0), shift);
        }
        __syncthreads();
        const uint32_t lo = val[0], hi = val[1];
        if (!MAD && s.a.prm.mode == PGN_NORM_MEDMAD) {
            if (lane == 0) S.m2 = unkey_plain(lo) + unkey_plain(hi);
            for (uint32_t i = lane; i < kSlotHistVecs; i += kSlotThreads)
                reinterpret_cast<uint4*>(&S)[i] = make_uint4(0, 0, 0, 0);
        } else if (lane == 0) {
            const uint64_t r = S.read;
            pgn_read_stats st;
            stats_clear(st, s.a.counts[r], read_status(s.a, r));
            if (MAD) finish_medmad(s.a.prm, S.m2, lo + hi, st);
            else finish_quantile(s.a.prm, unkey_plain(lo), unkey_plain(hi), st);
            s.a.stats[r] = st;
        }
        __syncthreads();  // the next slot overwrites fine and val
    }
}

// ---- reads -> chunks ------------------------------------------------------------------------------
// Chunk c of read r lands at readOut[r] + the read's earlier chunk counts; the read's n is their sum.
__global__ void expand_reads_kernel(uint64_t nreads, const uint64_t* __restrict__ firstChunk,
                                    const uint64_t* __restrict__ readOut, const uint32_t* __restrict__ counts,
                                    uint64_t* __restrict__ chunkOut, uint32_t* __restrict__ chunkRead,
                                    uint64_t* __restrict__ readN)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nreads) return;
    uint64_t acc = 0;
    const uint64_t base = readOut[r];
    for (uint64_t c = firstChunk[r]; c < firstChunk[r + 1]; c++) {
        chunkOut[c] = base + acc;
        chunkRead[c] = (uint32_t)r;
        acc += counts[c];
    }
    readN[r] = acc;
}

// The same for the calibrated decode (pgn_decompress_reads_device_pa): a chunk carries its read's
// calibration.  calOffset / calScale are NULL together (int16 output: nothing to expand).
__global__ void expand_reads_pa_kernel(uint64_t nreads, const uint64_t* __restrict__ firstChunk,
                                       const uint64_t* __restrict__ readOut, const uint32_t* __restrict__ counts,
                                       const float* __restrict__ calOffset, const float* __restrict__ calScale,
                                       uint64_t* __restrict__ chunkOut, float* __restrict__ chunkOffset,
                                       float* __restrict__ chunkScale)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nreads) return;
    uint64_t acc = 0;
    const uint64_t base = readOut[r];
    const float off = calOffset ? calOffset[r] : 0.0f, scale = calScale ? calScale[r] : 0.0f;
    for (uint64_t c = firstChunk[r]; c < firstChunk[r + 1]; c++) {
        chunkOut[c] = base + acc;
        if (calOffset) {
            chunkOffset[c] = off;
            chunkScale[c] = scale;
        }
        acc += counts[c];
    }
}

// A read's status: its first chunk status that is not PGN_OK, in chunk order (PGN_OK without chunks).
__global__ void reads_status_kernel(uint64_t nreads, const uint64_t* __restrict__ firstChunk,
                                    const int32_t* __restrict__ chunkStatus, int32_t* __restrict__ readStatus)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nreads) return;
    int32_t s = PGN_OK;
    for (uint64_t c = firstChunk[r]; c < firstChunk[r + 1]; c++)
        if (chunkStatus[c] != PGN_OK) {
            s = chunkStatus[c];
            break;
        }
    readStatus[r] = s;
}

// ---- the elementwise pass: out = ((float)adc + (-centre)) * inv -----------------------------------
// binary32 -> binary16 bits, round to nearest even, of the rounded binary32 product: the empty asm keeps
// the compiler from fusing multiply and conversion into one rounding (v_fma_mixlo_f16, see pgn_c5.h).
__device__ __forceinline__ uint32_t norm_f16_bits(float f)
{
    asm("" : "+v"(f));
    return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)f);
}
__device__ __forceinline__ float norm_value(uint32_t x16, float negc, float inv)
{
    return ((float)(int32_t)(int16_t)(uint16_t)x16 + negc) * inv;
}

struct NormArgs {
    const int16_t* adc;          // the decoded samples (may be the output itself for binary16)
    void* out;
    const uint64_t* chunkOut;    // per chunk, in elements (both arrays)
    const uint32_t* counts;
    const uint32_t* chunkRead;
    const pgn_read_stats* stats;
    uint64_t nchunks;
};

constexpr uint32_t kNormSplit = 8;  // workgroups that share one chunk (blockIdx.y)

// One chunk per blockIdx.x step, its 16-byte vectors dealt to kNormSplit workgroups.  A thread reads
// its eight samples before it writes them, and no other thread touches them: binary16 in place is safe.
template <class T>
__global__ __launch_bounds__(256) void norm_convert_kernel(NormArgs a)
{
    for (uint64_t c = blockIdx.x; c < a.nchunks; c += gridDim.x) {
        const uint32_t n = a.counts[c];
        if (!n) continue;
        const pgn_read_stats* st = a.stats + a.chunkRead[c];
        const float negc = -st->centre, inv = 1.0f / st->spread;
        const int16_t* in = a.adc + a.chunkOut[c];
        T* out = reinterpret_cast<T*>(a.out) + a.chunkOut[c];
        auto one = [&](uint32_t i) {
            const float v = norm_value((uint16_t)in[i], negc, inv);
            if constexpr (sizeof(T) == 4) out[i] = v;
            else reinterpret_cast<uint16_t*>(out)[i] = (uint16_t)norm_f16_bits(v);
        };
        uint32_t head = (uint32_t)((16u - (uint32_t)((uintptr_t)in & 15u)) & 15u) >> 1;
        if (head > n) head = n;
        const uint32_t nvec = (n - head) >> 3;
        const bool aligned = ((uintptr_t)(out + head) & 15u) == 0;
        if (blockIdx.y == 0) {
            if (threadIdx.x < head) one(threadIdx.x);
            const uint32_t t = head + (nvec << 3) + threadIdx.x;
            if (t < n) one(t);
        }
        const uint4* q = reinterpret_cast<const uint4*>(in + head);
        for (uint32_t i = blockIdx.y * 256 + threadIdx.x; i < nvec; i += kNormSplit * 256) {
            const uint4 v = q[i];
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            float f[8];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                f[2 * j] = norm_value(w[j] & 0xFFFFu, negc, inv);
                f[2 * j + 1] = norm_value(w[j] >> 16, negc, inv);
            }
            T* o = out + head + (size_t)i * 8;
            if constexpr (sizeof(T) == 4) {
                if (aligned) {
                    reinterpret_cast<float4*>(o)[0] = make_float4(f[0], f[1], f[2], f[3]);
                    reinterpret_cast<float4*>(o)[1] = make_float4(f[4], f[5], f[6], f[7]);
                } else {
#pragma unroll
                    for (int j = 0; j < 8; j++) o[j] = f[j];
                }
            } else {
                uint32_t h[4];
#pragma unroll
                for (int j = 0; j < 4; j++) h[j] = norm_f16_bits(f[2 * j]) | (norm_f16_bits(f[2 * j + 1]) << 16);
                if (aligned) {
                    *reinterpret_cast<uint4*>(o) = make_uint4(h[0], h[1], h[2], h[3]);
                } else {
                    uint16_t* o16 = reinterpret_cast<uint16_t*>(o);
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        o16[2 * j] = (uint16_t)h[j];
                        o16[2 * j + 1] = (uint16_t)(h[j] >> 16);
                    }
                }
            }
        }
    }
}
#endif  // PGN_SELECT_HOST_ONLY

}  // namespace sel
}  // namespace pgn

#endif  // PGN_SELECT_H
