// pgn_crf_post.h -- posterior marginals (forward-backward) of a CRF model's rows: four float32 per frame, the
// probability of each newest base (include/pgnano_hip.h "Posteriors and qualities (CRF)").
//
// One row per workgroup and one state per lane, as in pgn_crf.h, whose shapes and staged 16-byte loads with frames
// in flight this kernel uses.  Both recursions are float32 log-sum-exps of five candidates, kept near zero by
// subtracting element 0 of the vector they read (one more broadcast read of LDS, no barrier).
//   forward   the Viterbi kernel's data flow: a wave stages its own slice of a frame and takes its lanes' 5 or 4
//             scores from it behind a wave fence; a_t lies twice in LDS, one barrier per frame.  a_{t+1}[s] goes to
//             the row's scratch, scratch[t * S + s], a coalesced dword store per frame that only lane s reads back.
//   backward  a lane's four successors c(u, 0..3) are four neighbouring states of another wave's slice, so the
//             frame's scores stand in one buffer for the whole workgroup, behind a barrier; the second barrier of
//             the frame lets the next one overwrite them.  b_{t+1}[c(u, 0..3)] is one 16-byte read.  The scratch
//             value of frame t travels with the frame's scores in the ring of loads in flight.
//   marginal  w_t[s] = a_{t+1}[s] + b_{t+1}[s] of kPostBatch frames waits in LDS; then a wave takes a frame: the
//             maximum over the states, exp(w - max) summed per lane (a lane's states share lane & 3), over the
//             lanes of equal lane & 3, and over the four classes.  It costs no barrier of its own.
// No index depends on a score, so a row of NaNs or infinities reads and writes what any row does.
#ifndef PGN_CRF_POST_H
#define PGN_CRF_POST_H

#include "pgn_crf.h"

namespace pgn {
namespace crf {

// the forward vectors of one row: a float per state and frame
PGN_HD uint64_t post_row_scratch_bytes(uint32_t S, uint32_t T) { return 4ull * S * T; }

#ifndef PGN_SELECT_HOST_ONLY
struct PostArgs {
    const uint8_t* rows;  // frame t of row g at rows + g * rowStride + t * frameStride
    uint64_t rowStride, frameStride;
    uint32_t T;
    float stay;
    float* post;          // row g's at post + g * postStride, four floats per frame
    uint64_t postStride;
    float* fwd;           // context scratch: rowWords floats per row
    uint64_t rowWords;
};

constexpr uint32_t kPostBatch = 8;  // frames whose marginals are reduced together

// exp of a value at or below zero and log of a sum in [1, 5], by the hardware's exp2 and log2.  The product with
// log2(e) costs an exponent |x| * 2^-24 of absolute error, so a term's relative error grows with its smallness,
// and its share of the sum shrinks faster: measured against the float64 model, this form is no further from it than
// the library's functions (profiles/crf_post_accuracy.log), and the call is a fifth to a quarter faster
// (profiles/crf_post_timing.log).
__device__ __forceinline__ float exp_le0(float x) { return __expf(x); }

// log(sum of exp) of five values, the largest taken out first
__device__ __forceinline__ float lse5(float v0, float v1, float v2, float v3, float v4)
{
    const float m = fmaxf(fmaxf(fmaxf(v0, v1), fmaxf(v2, v3)), v4);
    const float sum = (exp_le0(v0 - m) + exp_le0(v1 - m)) + (exp_le0(v2 - m) + exp_le0(v3 - m)) + exp_le0(v4 - m);
    return m + __logf(sum);
}

template <uint32_t K, typename E, uint32_t TR>
__global__ __launch_bounds__(threads_of(K)) void crf_posterior_kernel(PostArgs a)
{
    using Sh = Shape<K, E, TR>;
    constexpr uint32_t S = Sh::S, kElem = Sh::kElem, kWaveBytes = Sh::kWaveBytes, R = Sh::kRounds;
    constexpr uint32_t kDepth = Sh::kDepth, kWaves = Sh::kWaves, B = kPostBatch;
    constexpr uint32_t kFrameBytes = S * TR * kElem;
    static_assert(kWaves == 1 || kWaveBytes % 16 == 0, "every wave's slice of a frame has the frame's misalignment");
    // the frame as it lies in memory, from its misalignment on: byte j of the frame at stage[mis + j]
    __shared__ __attribute__((aligned(16))) uint8_t stage[kFrameBytes + 32];
    __shared__ __attribute__((aligned(16))) float vec[2][S];  // a_t, then b_t
    __shared__ float wbuf[B][S];

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t row = blockIdx.x;
    const uint32_t T = a.T;
    const uint8_t* rowBase = a.rows + row * a.rowStride + (uint64_t)wave * kWaveBytes;
    float* fwdRow = a.fwd + row * a.rowWords;
    float* postRow = a.post + row * a.postStride;
    uint8_t* myStage = stage + wave * kWaveBytes;
    const bool active = S >= 64 || tid < S;
    const uint32_t s = tid;

    struct Ring {
        Pre<R> p;
        float fwd;  // backward: a_{t+1}[s] of the frame t in p
    };
    // pgn_crf.h's load and put: every lane issues every load, whatever the alignment
    auto load = [&](Pre<R>& p, uint32_t t) {
        const uint8_t* g = rowBase + (uint64_t)t * a.frameStride;
        const Span sp = span_of<kWaveBytes, kElem>(g);
#pragma unroll
        for (uint32_t r = 0; r < R; r++) {
            const uint32_t v = r * 64 + lane < sp.nvec ? r * 64 + lane : sp.nvec - 1;
            p.v[r] = *reinterpret_cast<const Vec16*>(g + sp.head + 16 * v);
        }
        const uint32_t o = lane * kElem;
        const uint32_t off = lane < sp.nedge ? (o < sp.head ? o : sp.tailAt + (o - sp.head)) : 0u;
        if (kElem == 4)
            p.e = *reinterpret_cast<const uint32_t*>(g + off);
        else
            p.e = *reinterpret_cast<const uint16_t*>(g + off);
    };
    auto put = [&](const Pre<R>& p, uint32_t t) -> uint32_t {
        const uint8_t* g = rowBase + (uint64_t)t * a.frameStride;
        const Span sp = span_of<kWaveBytes, kElem>(g);
#pragma unroll
        for (uint32_t r = 0; r < R; r++) {
            const uint32_t v = r * 64 + lane;
            if (v < sp.nvec) *reinterpret_cast<Vec16*>(myStage + sp.mis + sp.head + 16 * v) = p.v[r];
        }
        if (lane < sp.nedge) {
            const uint32_t o = lane * kElem, off = o < sp.head ? o : sp.tailAt + (o - sp.head);
            if (kElem == 4)
                *reinterpret_cast<uint32_t*>(myStage + sp.mis + off) = p.e;
            else
                *reinterpret_cast<uint16_t*>(myStage + sp.mis + off) = (uint16_t)p.e;
        }
        return sp.mis;
    };
    auto group_sync = [&]() {
        if (S > 64)
            __syncthreads();
        else
            wave_sync();
    };

    // ---- forward: frame t, whose scores are in p; then p takes the scores of frame `next` ----
    float own = 0.0f;
    auto forward = [&](Ring& r, uint32_t t, uint32_t next) {
        const uint32_t mis = put(r.p, t);
        load(r.p, next);
        wave_sync();
        if (active) {
            const E* x = reinterpret_cast<const E*>(myStage + mis + lane * (TR * kElem));
            const float* A = vec[t & 1];
            const float zero = A[0];
            const float v = lse5((own - zero) + (TR == 5 ? (float)x[0] : a.stay),
                                 (A[pred(S, s, 0)] - zero) + (float)x[TR - 4 + 0],
                                 (A[pred(S, s, 1)] - zero) + (float)x[TR - 4 + 1],
                                 (A[pred(S, s, 2)] - zero) + (float)x[TR - 4 + 2],
                                 (A[pred(S, s, 3)] - zero) + (float)x[TR - 4 + 3]);
            vec[(t & 1) ^ 1][s] = v;
            own = v;
            fwdRow[(uint64_t)t * S + s] = v;
        }
        group_sync();
    };

    Ring ring[kDepth];
#pragma unroll
    for (uint32_t j = 0; j < kDepth; j++) load(ring[j].p, j < T ? j : T - 1);
    if (active) vec[0][s] = 0.0f;
    group_sync();
    uint32_t i0 = 0;
    for (; i0 + kDepth <= T; i0 += kDepth) {
#pragma unroll
        for (uint32_t j = 0; j < kDepth; j++) {
            const uint32_t next = i0 + j + kDepth;
            forward(ring[j], i0 + j, next < T ? next : T - 1);
        }
    }
#pragma unroll
    for (uint32_t j = 0; j + 1 < kDepth; j++)
        if (i0 + j < T) forward(ring[j], i0 + j, T - 1);

    // ---- backward: step i handles frame t = T - 1 - i ----
    // the marginals of the frames in wbuf[0 .. n): step i - (n - 1) + j put frame T - 1 - (i - (n - 1) + j) there
    auto marginals = [&](uint32_t i, uint32_t n) {
        for (uint32_t j = wave; j < n; j += kWaves) {
            const uint32_t t = T - 1 - (i - (n - 1) + j);
            constexpr uint32_t Q = S < 64 ? 1 : S / 64;
            float w[Q > 4 ? 1 : Q];
            float m = -INFINITY;
            if constexpr (Q <= 4) {
#pragma unroll
                for (uint32_t q = 0; q < Q; q++) {
                    w[q] = lane + 64 * q < S ? wbuf[j][lane + 64 * q] : -INFINITY;
                    m = fmaxf(m, w[q]);
                }
            } else {
                for (uint32_t q = 0; q < Q; q++) m = fmaxf(m, wbuf[j][lane + 64 * q]);
            }
#pragma unroll
            for (uint32_t off = 32; off; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
            float e = 0.0f;
            if constexpr (Q <= 4) {
#pragma unroll
                for (uint32_t q = 0; q < Q; q++) e += lane + 64 * q < S ? exp_le0(w[q] - m) : 0.0f;
            } else {
                for (uint32_t q = 0; q < Q; q++) e += exp_le0(wbuf[j][lane + 64 * q] - m);
            }
#pragma unroll
            for (uint32_t off = 32; off >= 4; off >>= 1) e += __shfl_xor(e, off);
            float total = e + __shfl_xor(e, 1);
            total += __shfl_xor(total, 2);
            if (lane < 4) postRow[4ull * t + lane] = e / total;
        }
    };

    constexpr uint32_t kTopShift = 2 * K - 2;
    const uint32_t succ = (s << 2) & (S - 1), top = s >> kTopShift;
    auto backward = [&](Ring& r, uint32_t i, uint32_t next) {
        const uint32_t t = T - 1 - i;
        const uint32_t mis = put(r.p, t);
        const float aNext = r.fwd;
        load(r.p, next);
        if (active) {
            r.fwd = fwdRow[(uint64_t)next * S + s];
            wbuf[i % B][s] = aNext + own;
        }
        group_sync();  // the frame's scores and this step's w are the workgroup's
        if (active) {
            const E* x = reinterpret_cast<const E*>(stage + mis);
            const float* Bv = vec[i & 1];
            const float zero = Bv[0];
            const float4 nb = *reinterpret_cast<const float4*>(Bv + succ);
            const float v = lse5((own - zero) + (TR == 5 ? (float)x[s * TR] : a.stay),
                                 (nb.x - zero) + (float)x[(succ + 0) * TR + TR - 4 + top],
                                 (nb.y - zero) + (float)x[(succ + 1) * TR + TR - 4 + top],
                                 (nb.z - zero) + (float)x[(succ + 2) * TR + TR - 4 + top],
                                 (nb.w - zero) + (float)x[(succ + 3) * TR + TR - 4 + top]);
            vec[(i & 1) ^ 1][s] = v;
            own = v;
        }
        if (i % B == B - 1 || t == 0) marginals(i, i % B + 1);
        group_sync();  // the next step overwrites the scores and, behind its own barrier, reads this b_t
    };

    // the forward pass ended on a barrier: vec and the stage are free
#pragma unroll
    for (uint32_t j = 0; j < kDepth; j++) {
        const uint32_t t = j < T ? T - 1 - j : 0;
        load(ring[j].p, t);
        ring[j].fwd = active ? fwdRow[(uint64_t)t * S + s] : 0.0f;
    }
    if (active) vec[0][s] = 0.0f;
    own = 0.0f;
    group_sync();
    i0 = 0;
    for (; i0 + kDepth <= T; i0 += kDepth) {
#pragma unroll
        for (uint32_t j = 0; j < kDepth; j++) {
            const uint32_t next = i0 + j + kDepth;
            backward(ring[j], i0 + j, next < T ? T - 1 - next : 0);
        }
    }
#pragma unroll
    for (uint32_t j = 0; j + 1 < kDepth; j++)
        if (i0 + j < T) backward(ring[j], i0 + j, 0);
}
#endif  // PGN_SELECT_HOST_ONLY

}  // namespace crf
}  // namespace pgn

#endif  // PGN_CRF_POST_H
