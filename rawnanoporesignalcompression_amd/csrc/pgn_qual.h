// pgn_qual.h -- stitched base probabilities to one phred character per base (include/pgnano_hip.h "Posteriors
// and qualities (CRF)", the rule of pgn_base_qual_device).  Integer sums and comparisons alone: the tolerance is zero.
//
// A workgroup per read (further reads in a stride of the grid), a wave per 64 of its bases, a base per lane.  A
// lane sums its own block of frames up to kLongBlock of them.  A longer block (a stalled read's) is summed by the
// whole wave, lane after lane over neighbouring frames, and handed back to its lane: the sum is of integers, so the
// split changes nothing.  The thresholds travel in the kernel's arguments.
#ifndef PGN_QUAL_H
#define PGN_QUAL_H

#include "pgn_ctc.h"

namespace pgn {
namespace qual {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kLongBlock = 64;  // frames of one base above which the wave shares the sum
constexpr uint32_t kMaxQ = 93;       // '!' + 93 is '~', the last phred character

// PGN_ERR_INVALID_ARG conditions of the parameters
inline bool params_valid(const pgn_qual_params* P)
{
    if (!P) return false;
    if (P->q_min > kMaxQ || P->nthresholds > kMaxQ - P->q_min) return false;
    for (uint32_t j = 1; j < P->nthresholds; j++)
        if (P->thr[j] > P->thr[j - 1]) return false;
    return true;
}

// err_t of one frame as u_t: the error probability in units of 2^-32, the called base being c
PGN_HD uint64_t frame_error(const float* p, uint32_t c)
{
    const float err = (p[(c + 1) & 3] + p[(c + 2) & 3]) + p[(c + 3) & 3];
    if (err != err || err >= 1.0f) return 0xFFFFFFFFull;
    if (!(err > 0.0f)) return 0;
    return (uint64_t)(err * 4294967296.0f);  // exact scaling, truncation; below 2^32
}

#ifndef PGN_SELECT_HOST_ONLY
struct Args {
    uint64_t nreads;
    const uint64_t* readFrames;  // nreads + 1
    const uint8_t* codes;        // frame i at codes[i - frameBase]
    const float* post;           // and at post + 4 * (i - frameBase)
    uint64_t frameBase, capacity;  // the window; frameBase + capacity does not wrap
    const uint64_t* readBases;   // nreads + 1
    const uint32_t* baseFrame;
    const int32_t* status;
    uint8_t* qual;
    uint64_t baseCapacity;
    pgn_qual_params prm;
};

__global__ __launch_bounds__(kThreads) void base_qual_kernel(Args a)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    constexpr uint32_t kWaves = kThreads / 64;
    for (uint64_t r = blockIdx.x; r < a.nreads; r += gridDim.x) {
        const uint64_t f0 = a.readFrames[r], f1 = a.readFrames[r + 1];
        if (f0 < a.frameBase || f1 < f0 || f1 > a.frameBase + a.capacity) continue;  // not taken
        const uint64_t F = f1 - f0;
        if (F >> 32) continue;  // base_frame does not describe it
        if (a.status[r] != PGN_OK) continue;
        const uint64_t b0 = a.readBases[r], b1 = a.readBases[r + 1];
        if (b1 < b0 || b1 > a.baseCapacity) continue;
        const uint64_t nb = b1 - b0;
        const uint8_t* codes = a.codes + (f0 - a.frameBase);
        const float* post = a.post + 4 * (f0 - a.frameBase);
        for (uint64_t first = 64ull * wave; first < nb; first += 64ull * kWaves) {
            const uint64_t j = first + lane;
            const bool has = j < nb;
            // the block of frames [t0, t0 + n) inside the read, whatever base_frame holds
            uint64_t t0 = 0, n = 0;
            uint32_t c = 0;
            if (has) {
                t0 = a.baseFrame[b0 + j];
                uint64_t t1 = j + 1 < nb ? a.baseFrame[b0 + j + 1] : F;
                t0 = t0 < F ? t0 : F;
                t1 = t1 < F ? t1 : F;
                n = t1 > t0 ? t1 - t0 : 0;
                if (n) c = codes[t0] & 3u;
            }
            uint64_t U = 0;
            if (n <= kLongBlock)
                for (uint64_t t = t0; t < t0 + n; t++) U += frame_error(post + 4 * t, c);
            unsigned long long longs = __ballot(n > kLongBlock);
            while (longs) {
                const int src = __ffsll(longs) - 1;
                longs &= longs - 1;
                const uint64_t T0 = __shfl(t0, src), N = __shfl(n, src);
                const uint32_t C = __shfl(c, src);
                uint64_t sum = 0;
                for (uint64_t q = lane; q < N; q += 64) sum += frame_error(post + 4 * (T0 + q), C);
#pragma unroll
                for (uint32_t off = 32; off; off >>= 1) sum += __shfl_xor(sum, off);
                if ((int)lane == src) U = sum;
            }
            if (has) {
                uint32_t q = a.prm.q_min;
                for (uint32_t k = 0; k < a.prm.nthresholds; k++) q += U <= (uint64_t)a.prm.thr[k] * n ? 1u : 0u;
                a.qual[b0 + j] = (uint8_t)(33u + q);
            }
        }
    }
}
#endif  // PGN_SELECT_HOST_ONLY

}  // namespace qual
}  // namespace pgn

#endif  // PGN_QUAL_H
