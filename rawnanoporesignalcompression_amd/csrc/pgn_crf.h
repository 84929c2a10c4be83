// pgn_crf.h -- best-path (Viterbi) decode of a CRF model's rows into one code byte per frame
// (include/pgnano_hip.h "Model rows to per-frame codes (CRF)").
//
// One row per workgroup and one state per lane: S / 64 waves (one wave, part of it idle, below 64 states).
//   forward   a_t lies twice in LDS; a frame reads the four predecessors (four neighbouring lanes read the same
//             four words: a broadcast), adds, compares and writes the other copy; one barrier per frame, a wave
//             fence where the row is one wave.  A wave's scores of a frame are 64 * transitions contiguous
//             elements: they come in 16-byte global loads (the elements in front of the first and behind the
//             last 16-byte address one by one), depth_of(k) frames ahead in registers, and pass through a buffer in
//             LDS that only this wave uses, from which every lane takes its 5 or 4.  A lane collects its
//             backpointers of 8 frames, 4 bits each, in one dword: bp[(t / 8) * S + s], a coalesced store per
//             8 frames.
//   end       wave 0 reduces a_T with the index carried (the lowest index wins a tie).
//   traceback by default in the same workgroup: the backpointers of kTraceGroups * 8 frames are copied to LDS
//             by all threads (the copy of the chunk before is in flight meanwhile), thread 0 walks them and
//             leaves the codes in LDS, all threads store them in dwords where the address allows.  With
//             PGN_CRF_TRACEBACK=split the forward kernel leaves the end state behind the row's backpointers and
//             crf_traceback_kernel walks a row per lane in global memory (the measured alternative); =none leaves
//             the traceback out, which is how tools/crf_timing.py times the forward pass alone.
#ifndef PGN_CRF_H
#define PGN_CRF_H

#include "pgn_ctc.h"

namespace pgn {
namespace crf {

// Frames whose scores are in flight ahead of the one being computed.  Measured at T = 2,000 and 10.5 GB of
// float16 scores (profiles/crf_timing.log), depth 1 / 2 / 4 / 8: k = 3 3.74 / 3.58 / 3.21 / 3.26 ms, k = 4
// 3.46 / 3.33 / 3.35 / 3.41 ms, k = 5 3.25 / 3.15 / 3.70 / 3.68 ms.  -DPGN_CRF_DEPTH=n builds the library with n
// frames at every state length, which is how those were taken.
constexpr uint32_t depth_of(uint32_t stateLen)
{
#ifdef PGN_CRF_DEPTH
    return PGN_CRF_DEPTH;
#else
    return stateLen >= 5 ? 2u : 4u;
#endif
}
constexpr uint64_t kDefaultScratch = PGN_CRF_DEFAULT_SCRATCH;
constexpr uint32_t kMaxT = 1u << 24;
constexpr uint32_t kRowTailBytes = 16;  // the end state, and the next row stays 16-byte aligned

PGN_HD uint32_t states(uint32_t stateLen) { return 1u << (2 * stateLen); }
// the predecessor of s by option b: drop s's newest base and put b on top
PGN_HD uint32_t pred(uint32_t S, uint32_t s, uint32_t b) { return (b * S + s) >> 2; }
// backpointers of one row: a dword per state and 8 frames, then the end state
PGN_HD uint64_t row_scratch_bytes(uint32_t S, uint32_t T) { return 4ull * S * ((T + 7) / 8) + kRowTailBytes; }

// PGN_ERR_INVALID_ARG conditions of the parameters
inline bool params_valid(const pgn_crf_params* P)
{
    if (!P) return false;
    if (P->state_len < 1 || P->state_len > 5) return false;
    if (P->transitions != 4 && P->transitions != 5) return false;
    if (P->score_type != PGN_OUT_F32 && P->score_type != PGN_OUT_F16) return false;
    uint32_t bits;
    memcpy(&bits, &P->stay_score, sizeof bits);
    return P->transitions == 4 || bits == 0;
}

#ifndef PGN_SELECT_HOST_ONLY
struct Args {
    const uint8_t* rows;  // frame t of row g at rows + g * rowStride + t * frameStride
    uint64_t rowStride, frameStride;
    uint64_t nrows;       // of this launch
    uint32_t T, split;    // split: the traceback is crf_traceback_kernel's
    float stay;
    uint8_t* codes;       // row g's at codes + g * codesStride
    uint64_t codesStride;
    float* rowScore;      // may be null
    uint32_t* bp;         // context scratch: rowWords dwords per row
    uint64_t rowWords;
};

using Vec16 = ctc::Vec16;

// every lane has written what the wave's other lanes read next
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// threads of a row's workgroup: a lane per state, whole waves
constexpr uint32_t threads_of(uint32_t stateLen) { return stateLen < 3 ? 64u : 1u << (2 * stateLen); }

template <uint32_t K, typename E, uint32_t TR>
struct Shape {
    static constexpr uint32_t S = 1u << (2 * K);
    static constexpr uint32_t kThreads = threads_of(K);
    static constexpr uint32_t kWaves = kThreads / 64;
    static constexpr uint32_t kWaveStates = S < 64 ? S : 64;
    static constexpr uint32_t kElem = sizeof(E);
    static constexpr uint32_t kDepth = depth_of(K);
    static_assert(kDepth >= 1 && kDepth <= 8, "the prefetch ring lives in registers");
    static constexpr uint32_t kWaveBytes = kWaveStates * TR * kElem;  // a wave's scores of one frame
    static constexpr uint32_t kRounds = (kWaveBytes / 16 + 63) / 64;  // 16-byte loads per lane and frame
    static constexpr uint32_t kStageStride = (kWaveBytes + 16 + 15) & ~15u;
    // the traceback's chunk: this many groups of 8 frames, at most 4,096 dwords
    static constexpr uint32_t kTraceGroups = 4096 / S < 16 ? 4096 / S : 16;
    static constexpr uint32_t kTraceWords = kTraceGroups * S;
    static constexpr uint32_t kTracePerThread = (kTraceWords + kThreads - 1) / kThreads;
    static_assert(kWaveBytes / 16 >= 2 && kRounds <= 2, "loads per lane");
};

// A wave's scores of one frame on their way from global memory to its buffer in LDS.
template <uint32_t R>
struct Pre {
    Vec16 v[R];
    uint32_t e;  // one of the elements in front of the first or behind the last 16-byte address
};

// Where the 16-byte addresses of n bytes at g begin and end: [0, head) and [tailAt, n) go element by element.
struct Span {
    uint32_t mis, head, nvec, tailAt, nedge;
};
template <uint32_t kBytes, uint32_t kElem>
__device__ __forceinline__ Span span_of(const uint8_t* g)
{
    Span s;
    s.mis = (uint32_t)((uintptr_t)g & 15u);
    const uint32_t toBoundary = (16u - s.mis) & 15u;
    s.head = toBoundary < kBytes ? toBoundary : kBytes;
    s.nvec = (kBytes - s.head) >> 4;
    s.tailAt = s.head + (s.nvec << 4);
    s.nedge = (s.head + (kBytes - s.tailAt)) / kElem;  // below 16
    return s;
}

// The forward pass of one row, its end state and, unless a.split, its traceback.
template <uint32_t K, typename E, uint32_t TR>
__global__ __launch_bounds__(threads_of(K)) void crf_forward_kernel(Args a)
{
    using Sh = Shape<K, E, TR>;
    constexpr uint32_t S = Sh::S, kThreads = Sh::kThreads, kElem = Sh::kElem, kWaveBytes = Sh::kWaveBytes, R = Sh::kRounds;
    constexpr uint32_t kDepth = Sh::kDepth;
    __shared__ __attribute__((aligned(16))) uint8_t stage[Sh::kWaves][Sh::kStageStride];
    __shared__ float alpha[2][S];
    __shared__ uint32_t trace[Sh::kTraceWords];
    __shared__ __attribute__((aligned(4))) uint8_t cbuf[Sh::kTraceGroups * 8];
    __shared__ uint32_t endState;

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t row = blockIdx.x;
    const uint32_t T = a.T;
    const uint8_t* rowBase = a.rows + row * a.rowStride + (uint64_t)wave * kWaveBytes;
    uint32_t* bpRow = a.bp + row * a.rowWords;
    uint8_t* myStage = stage[wave];
    const bool active = S >= 64 || tid < S;  // a row below 64 states leaves lanes idle
    const uint32_t s = tid;

    // Every lane issues every load, whatever the alignment: a lane without a piece of its own repeats the last
    // 16-byte piece, or the frame's first element.  Behind a branch the loads would be waited for with
    // vmcnt(0) at every use, and the frames in flight behind them with them.
    auto load = [&](Pre<R>& p, uint32_t t) {
        const uint8_t* g = rowBase + (uint64_t)t * a.frameStride;
        const Span sp = span_of<kWaveBytes, kElem>(g);  // nvec >= 1: a wave's bytes are at least 32
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
    // the buffer keeps the frame's misalignment, so the 16-byte pieces land on 16-byte addresses of LDS
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

    float own = 0.0f;
    uint32_t word = 0;
    // frame t, whose scores are in p; then p takes the scores of frame `next`
    auto step = [&](Pre<R>& p, uint32_t t, uint32_t next) {
        const uint32_t mis = put(p, t);
        load(p, next);
        wave_sync();
        if (active) {
            const E* x = reinterpret_cast<const E*>(myStage + mis + lane * (TR * kElem));
            const float* A = alpha[t & 1];
            float best = own + (TR == 5 ? (float)x[0] : a.stay);
            uint32_t opt = 0;
#pragma unroll
            for (uint32_t b = 0; b < 4; b++) {
                const float cand = A[pred(S, s, b)] + (float)x[TR - 4 + b];
                if (cand > best) {
                    best = cand;
                    opt = 1 + b;
                }
            }
            alpha[(t & 1) ^ 1][s] = best;
            own = best;
            word |= opt << (4 * (t & 7));
            if ((t & 7) == 7 || t + 1 == T) {
                bpRow[(uint64_t)(t >> 3) * S + s] = word;
                word = 0;
            }
        }
        // the next frame reads what this one wrote, and writes the buffers this one read
        if (S > 64)
            __syncthreads();
        else
            wave_sync();
    };

    Pre<R> ring[kDepth];
#pragma unroll
    for (uint32_t j = 0; j < kDepth; j++) load(ring[j], j < T ? j : T - 1);
    if (active) alpha[0][s] = 0.0f;
    if (S > 64)
        __syncthreads();
    else
        wave_sync();

    // whole rounds of the ring without a branch around a load; a frame behind the row's end is its last again
    uint32_t t0 = 0;
    for (; t0 + kDepth <= T; t0 += kDepth) {
#pragma unroll
        for (uint32_t j = 0; j < kDepth; j++) {
            const uint32_t next = t0 + j + kDepth;
            step(ring[j], t0 + j, next < T ? next : T - 1);
        }
    }
#pragma unroll
    for (uint32_t j = 0; j + 1 < kDepth; j++)
        if (t0 + j < T) step(ring[j], t0 + j, T - 1);
    __syncthreads();  // the backpointers are in memory for the whole workgroup

    // the end: m = a_T[0], then every a_T[s] > m in index order.  A NaN at s > 0 never replaces, so it counts as
    // absent; a NaN at 0 is never replaced.
    if (wave == 0) {
        const float* A = alpha[T & 1];
        float m = -INFINITY;
        uint32_t e = 0xFFFFFFFFu;
        for (uint32_t q = lane; q < S; q += 64) {
            const float v = A[q];
            if (e == 0xFFFFFFFFu) {
                e = q;
                if (v == v) m = v;
            } else if (v > m) {
                m = v;
                e = q;
            }
        }
#pragma unroll
        for (uint32_t off = 32; off; off >>= 1) {
            const float m2 = __shfl_xor(m, off);
            const uint32_t e2 = __shfl_xor(e, off);
            if (m2 > m || (m2 == m && e2 < e)) {
                m = m2;
                e = e2;
            }
        }
        const float a0 = A[0];
        if (a0 != a0) {
            m = a0;
            e = 0;
        }
        if (lane == 0) {
            endState = e;
            if (a.rowScore) a.rowScore[row] = m;
            if (a.split) bpRow[a.rowWords - kRowTailBytes / 4] = e;
        }
    }
    if (a.split) return;
    __syncthreads();

    // the traceback, a chunk of kTraceGroups * 8 frames at a time from the row's end
    constexpr uint32_t G = Sh::kTraceGroups, W = Sh::kTracePerThread;
    const uint32_t ngroups = (T + 7) / 8, nchunks = (ngroups + G - 1) / G;
    uint32_t pre[W];
    auto fetch = [&](uint32_t c) {
        const uint32_t left = ngroups - c * G, n = (left < G ? left : G) * S;
        const uint32_t* src = bpRow + (uint64_t)c * G * S;
#pragma unroll
        for (uint32_t i = 0; i < W; i++) {
            const uint32_t idx = i * kThreads + tid;
            if (idx < n) pre[i] = src[idx];
        }
    };
    fetch(nchunks - 1);
    uint32_t cur = endState;
    uint8_t* codesRow = a.codes + row * a.codesStride;
    for (uint32_t c = nchunks; c-- > 0;) {
#pragma unroll
        for (uint32_t i = 0; i < W; i++) {
            const uint32_t idx = i * kThreads + tid;
            if (idx < Sh::kTraceWords) trace[idx] = pre[i];
        }
        if (c) fetch(c - 1);
        __syncthreads();
        const uint32_t f0 = c * G * 8, f1 = T - f0 < G * 8 ? T : f0 + G * 8;
        if (tid == 0) {
            for (uint32_t t = f1; t-- > f0;) {
                const uint32_t w = trace[((t >> 3) - c * G) * S + cur];
                const uint32_t opt = (w >> (4 * (t & 7))) & 7u;
                cbuf[t - f0] = (uint8_t)((cur & 3u) | (opt ? 0x80u : 0u));
                if (opt) cur = pred(S, cur, opt - 1);
            }
        }
        __syncthreads();
        // the chunk's codes: dwords between the first and the last 4-byte address, bytes around them
        uint8_t* dst = codesRow + f0;
        const uint32_t n = f1 - f0;
        const uint32_t toBoundary = (4u - (uint32_t)((uintptr_t)dst & 3u)) & 3u;
        const uint32_t head = toBoundary < n ? toBoundary : n;
        const uint32_t body = (n - head) >> 2, tailAt = head + (body << 2);
        for (uint32_t i = tid; i < body; i += kThreads) {
            const uint8_t* q = cbuf + head + 4 * i;
            reinterpret_cast<uint32_t*>(dst + head)[i] = q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24;
        }
        if (tid < head) dst[tid] = cbuf[tid];
        if (tid < n - tailAt) dst[tailAt + tid] = cbuf[tailAt + tid];
        // the next chunk's codes are written behind its first barrier, its backpointers only by thread 0's peers
        // that have passed the second one
    }
}

// The traceback of a row per lane from the backpointers in global memory (PGN_CRF_TRACEBACK=split).
__global__ __launch_bounds__(64) void crf_traceback_kernel(Args a, uint32_t S)
{
    const uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= a.nrows) return;
    const uint32_t* bpRow = a.bp + row * a.rowWords;
    uint8_t* codesRow = a.codes + row * a.codesStride;
    uint32_t cur = bpRow[a.rowWords - kRowTailBytes / 4];
    for (uint32_t t = a.T; t-- > 0;) {
        const uint32_t w = bpRow[(uint64_t)(t >> 3) * S + cur];
        const uint32_t opt = (w >> (4 * (t & 7))) & 7u;
        codesRow[t] = (uint8_t)((cur & 3u) | (opt ? 0x80u : 0u));
        if (opt) cur = pred(S, cur, opt - 1);
    }
}
#endif  // PGN_SELECT_HOST_ONLY

}  // namespace crf
}  // namespace pgn

#endif  // PGN_CRF_H
