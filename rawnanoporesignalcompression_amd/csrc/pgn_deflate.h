// pgn_deflate.h -- any device byte stream as BGZF blocks that each hold one Huffman-only dynamic deflate block, or a
// stored block where that is not smaller, packed end to end (include/pgnano_hip.h "BGZF deflate", the rule of
// pgn_bgzf_deflate_device).  Integers and bits alone: the tolerance is zero.
//
// A block's length follows from its histogram: sum cnt * len plus the header's bits.  So the call is three kernels:
//   plan  a workgroup per 65,280 stream bytes loads the payload into an LDS image (pgn_bam.h's layout, at the source's
//         alignment), counts the bytes in four histograms that the lanes share out, checksums the image (bam::block_crc), builds the
//         literal code and the code-length code, writes the header's bits, and leaves the block's file length in
//         blk_off[k] and the header bits, the 257 codes and the CRC in the context's scratch (BlockPlan),
//   scan  stitch::stitch_scan_kernel over blk_off in place,
//   pack  a workgroup per block that the capacity admits: thread t takes payload bytes [64 t, 64 t + 64), the
//         workgroup scans the runs' bit counts, and every thread ORs its bits into an output image in LDS laid out at
//         the destination's alignment; the image leaves as aligned 16-byte stores with byte-wise edges, and the
//         block's 18 bytes in front and 8 behind go byte by byte.  A stored block takes the same way out.
// The code construction is the rule's, step for step: a rank sort of the used symbols by (count, symbol) by the
// workgroup, the two-queue merge by one thread (at most 256 steps), a leaf's depth by its own thread, the limiter
// by one wave with the lengths in registers and a wave-wide maximum per step.
#ifndef PGN_DEFLATE_H
#define PGN_DEFLATE_H

#include "pgn_bam.h"

namespace pgn {
namespace deflate {

constexpr uint32_t kThreads = bam::kThreads;
constexpr uint32_t kWaves = kThreads / 64;
constexpr uint32_t kBlock = bam::kBlock;
constexpr uint32_t kFrame = 26;                 // a BGZF block's bytes around its deflate bytes: 18 in front, 8 behind
constexpr uint32_t kFront = 18;
constexpr uint32_t kStored = 5;                 // 01 n ~n
constexpr uint32_t kSyms = 257, kClSyms = 19, kSeq = 259;
constexpr uint32_t kLitLimit = 15, kClLimit = 7;
constexpr uint32_t kHdrBytes = 512;             // 17 + 19 * 3 + 259 * (7 + 7) bits at the most
constexpr uint32_t kUnits = (kBlock + kStored + 15 + 15) / 16;
constexpr uint32_t kRounds = (kUnits + kThreads - 1) / kThreads;
constexpr uint32_t kImage = 16 * kUnits + 16;   // and a dword to read beyond
constexpr uint32_t kHistCopies = 4;             // of the plan kernel's histogram, by the lane: see deflate_plan_kernel
constexpr uint32_t kRun = 64;                   // payload bytes of one thread of the pack kernel
static_assert(kRun * kThreads >= kBlock, "the threads' runs cover a block");
static_assert(17 + 3 * kClSyms + 14 * kSeq <= 8 * kHdrBytes, "the header's bits fit");

// What the plan kernel leaves for the pack kernel, per block
struct BlockPlan {
    uint32_t crc, hdrBits, pad[2];
    uint32_t code[260];       // per symbol: the code's bits in stream order, and its length << 16
    uint8_t hdr[kHdrBytes];   // the bits in front of the first literal, the last byte padded with zeros
};
static_assert(sizeof(BlockPlan) == 1568, "include/pgnano_hip.h states the scratch per block");

#ifndef PGN_SELECT_HOST_ONLY
using Vec16 = ctc::Vec16;

struct Args {
    const uint8_t* src;
    uint64_t srcCapacity;     // >= 1
    const uint64_t* nbytes;   // may be null
    uint8_t* out;
    uint64_t byteCapacity;
    uint64_t* blkOff;         // ntiles + 1: the blocks' lengths between the plan and the scan, then the scan
    uint64_t* written;
    BlockPlan* plans;         // context scratch, one per tile
    uint64_t ntiles;
};

__device__ __forceinline__ uint64_t stream_bytes(const Args& a)
{
    const uint64_t w = a.nbytes ? *a.nbytes : a.srcCapacity;
    return w < a.srcCapacity ? w : a.srcCapacity;
}

// LDS of the code construction
struct Build {
    uint32_t w[2 * kSyms];        // the leaves in queue order, then the internal nodes in creation order
    uint16_t parent[2 * kSyms];
    uint16_t order[kSyms];        // the leaves' symbols
};

// The limiter of the rule, by wave 0 alone: lane l holds symbols l, l + 64, ...
__device__ __forceinline__ void limit_lengths(const uint32_t* cnt, uint32_t nsym, uint32_t L, uint8_t* len)
{
    constexpr uint32_t kPer = (kSyms + 63) / 64;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t c[kPer], l[kPer];
    uint32_t K = 0;
#pragma unroll
    for (uint32_t j = 0; j < kPer; j++) {
        const uint32_t s = lane + 64 * j;
        c[j] = s < nsym ? cnt[s] : 0;
        l[j] = c[j] ? (len[s] > L ? L : len[s]) : 0;
        if (c[j]) K += 1u << (L - l[j]);
    }
#pragma unroll
    for (uint32_t off = 32; off; off >>= 1) K += __shfl_xor(K, off);
    auto wave_max = [](uint32_t v) {
#pragma unroll
        for (uint32_t off = 32; off; off >>= 1) {
            const uint32_t o = __shfl_xor(v, off);
            v = o > v ? o : v;
        }
        return v;
    };
    // one more bit for the longest code below L, then the smallest count, then the largest symbol
    while (K > (1u << L)) {
        uint32_t key = 0;
#pragma unroll
        for (uint32_t j = 0; j < kPer; j++)
            if (c[j] && l[j] < L) {
                const uint32_t k = l[j] << 26 | (0x1FFFFu - c[j]) << 9 | (lane + 64 * j);
                key = k > key ? k : key;
            }
        key = wave_max(key);
        if (!key) break;
        const uint32_t s = key & 511u;
#pragma unroll
        for (uint32_t j = 0; j < kPer; j++)
            if (lane + 64 * j == s) l[j]++;
        K -= 1u << (L - (key >> 26) - 1);
    }
    // one bit less where the rest allows it: the largest count, then the smallest symbol
    uint32_t D = (1u << L) - K;
    while (D > 0) {
        uint32_t key = 0;
#pragma unroll
        for (uint32_t j = 0; j < kPer; j++)
            if (c[j] && l[j] > 1 && (1u << (L - l[j])) <= D) {
                const uint32_t k = c[j] << 13 | (511u - (lane + 64 * j)) << 4 | l[j];
                key = k > key ? k : key;
            }
        key = wave_max(key);
        if (!key) break;
        const uint32_t s = 511u - ((key >> 4) & 511u);
#pragma unroll
        for (uint32_t j = 0; j < kPer; j++)
            if (lane + 64 * j == s) l[j]--;
        D -= 1u << (L - (key & 15u));
    }
#pragma unroll
    for (uint32_t j = 0; j < kPer; j++)
        if (lane + 64 * j < nsym) len[lane + 64 * j] = (uint8_t)l[j];
}

// lengths(cnt, L) of the rule over nsym <= kSyms symbols (counts below 2^17), by the whole workgroup; cnt is
// ready and len is complete when it returns
__device__ __forceinline__ void build_lengths(const uint32_t* cnt, uint32_t nsym, uint32_t L, uint8_t* len, Build& b)
{
    const uint32_t tid = threadIdx.x;
    const uint32_t c = tid < nsym ? cnt[tid] : 0;
    if (tid < nsym) len[tid] = 0;
    if (c) {
        uint32_t rank = 0;
        for (uint32_t t = 0; t < nsym; t++) {
            const uint32_t ct = cnt[t];
            rank += (ct && (ct < c || (ct == c && t < tid))) ? 1u : 0u;
        }
        b.order[rank] = (uint16_t)tid;
        b.w[rank] = c;
    }
    const uint32_t m = (uint32_t)__syncthreads_count(c != 0);
    if (tid == 0 && m > 1) {
        // the queues' front weights stay in registers (~0 for an empty queue), so a pick waits for one LDS load
        uint32_t li = 0, ii = m, wl = b.w[0], wi = ~0u;
        for (uint32_t next = m; next < 2 * m - 1; next++) {
            uint32_t sum = 0;
            for (uint32_t k = 0; k < 2; k++) {
                if (wl <= wi) {
                    b.parent[li++] = (uint16_t)next;
                    sum += wl;
                    wl = li < m ? b.w[li] : ~0u;
                } else {
                    b.parent[ii++] = (uint16_t)next;
                    sum += wi;
                    wi = ii < next ? b.w[ii] : ~0u;
                }
            }
            b.w[next] = sum;
            if (ii == next) wi = sum;
        }
    }
    __syncthreads();
    uint32_t d = 0;
    if (tid < m) {  // a leaf's depth is its hops to the root, the last node
        d = 1;
        if (m > 1)
            for (uint32_t i = b.parent[tid]; i != 2 * m - 2; i = b.parent[i]) d++;
        len[b.order[tid]] = (uint8_t)d;
    }
    const int over = __syncthreads_or(d > L);
    if (over) {
        if (tid < 64) limit_lengths(cnt, nsym, L, len);
        __syncthreads();
    }
}

// the code of symbol s by RFC 1951 section 3.2.2, its bits reversed into stream order, and the length << 16
__device__ __forceinline__ uint32_t canonical_entry(const uint8_t* len, uint32_t nsym, uint32_t s)
{
    const uint32_t l = len[s];
    if (!l) return 0;
    uint32_t code = 0;
    for (uint32_t t = 0; t < nsym; t++) {
        const uint32_t lt = len[t];
        if (lt && lt < l) code += 1u << (l - lt);
        if (lt == l && t < s) code++;
    }
    return (__brev(code) >> (32 - l)) | l << 16;
}

// bits into bytes of LDS, from bit 0 of each byte upwards, by one thread
struct BitWriter {
    uint8_t* p;
    uint64_t acc = 0;
    uint32_t nb = 0, total = 0;
    __device__ __forceinline__ void put(uint32_t v, uint32_t bits)
    {
        acc |= (uint64_t)v << nb;
        nb += bits;
        total += bits;
        while (nb >= 8) {
            *p++ = (uint8_t)acc;
            acc >>= 8;
            nb -= 8;
        }
    }
    __device__ __forceinline__ void finish()
    {
        if (nb) *p++ = (uint8_t)acc;
    }
};

// The length sequence ll[0..256], 1, 1 in code-length symbols by the rule's runs: sym[i] = symbol | extra << 8, and
// the symbols' counts.  One thread.
__device__ __forceinline__ uint32_t length_symbols(const uint8_t* len, uint16_t* sym, uint32_t* clCnt)
{
    uint32_t ns = 0;
    auto emit = [&](uint32_t s, uint32_t extra) {
        sym[ns++] = (uint16_t)(s | extra << 8);
        clCnt[s]++;
    };
    auto at_seq = [&](uint32_t i) -> uint32_t { return i < kSyms ? len[i] : 1u; };
    for (uint32_t at = 0; at < kSeq;) {
        const uint32_t v = at_seq(at);
        uint32_t r = 1;
        while (at + r < kSeq && at_seq(at + r) == v) r++;
        at += r;
        if (v == 0) {
            while (r >= 11) {
                const uint32_t t = r < 138 ? r : 138;
                emit(18, t - 11);
                r -= t;
            }
            if (r >= 3) {
                emit(17, r - 3);
                r = 0;
            }
            for (; r; r--) emit(0, 0);
        } else {
            emit(v, 0);
            r--;
            while (r >= 3) {
                const uint32_t t = r < 6 ? r : 6;
                emit(16, t - 3);
                r -= t;
            }
            for (; r; r--) emit(v, 0);
        }
    }
    return ns;
}

// LDS: 80,000 bytes or so, and eight waves per SIMD (64 VGPRs), so that a CU holds two workgroups: one's serial steps (the
// merge, the runs, the header) run beside the other's parallel ones
__global__ __launch_bounds__(kThreads, 8) void deflate_plan_kernel(Args a)
{
    __shared__ __attribute__((aligned(16))) uint8_t image[kImage];
    __shared__ uint32_t crcT[4][256];
    __shared__ uint32_t hist[256 * kHistCopies];  // value v of lane l counts in hist[v * kHistCopies + l % kHistCopies]
    __shared__ uint32_t red[kWaves];
    __shared__ uint64_t waveSum[kWaves];
    __shared__ uint32_t cnt[kSyms + 3], clCnt[kClSyms + 1], clCode[kClSyms + 1];
    __shared__ uint8_t len[kSyms + 3], clLen[kClSyms + 1];
    __shared__ uint16_t clSym[kSeq + 1];
    __shared__ uint8_t hdr[kHdrBytes];
    __shared__ uint32_t shared[2];  // the code-length symbols' number, the header's bits
    __shared__ Build bld;
    const uint32_t tid = threadIdx.x;
    const uint64_t W = stream_bytes(a);
    (&crcT[0][0])[tid] = (&bam::kCrc.t[0][0])[tid];
    static_assert(kThreads == 4 * 256, "a table entry per thread");
    for (uint64_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        const uint64_t olo = t * kBlock;
        if (olo >= W) {  // the whole workgroup: no block
            if (tid == 0) a.blkOff[t] = 0;
            continue;
        }
        const uint32_t n = (uint32_t)(W - olo < kBlock ? W - olo : kBlock);
        const uint8_t* const src = a.src + olo;
        const uint32_t mis = (uint32_t)((uintptr_t)src & 15u);
        const uint8_t* const srcA = src - mis;
#pragma unroll
        for (uint32_t j = 0; j < kHistCopies * 256 / kThreads; j++) hist[j * kThreads + tid] = 0;
        if (tid < kHdrBytes) hdr[tid] = 0;
        if (tid < kClSyms) clCnt[tid] = 0;
#pragma unroll 1
        for (uint32_t j = 0; j < kRounds; j++) {
            const uint32_t u = j * kThreads + tid;
            const uint32_t ia = 16u * u > mis ? 16u * u : mis, ib = 16u * u + 16u < mis + n ? 16u * u + 16u : mis + n;
            if (u >= kUnits || ia >= ib) continue;
            if (ib - ia == 16)
                *reinterpret_cast<Vec16*>(image + 16u * u) = *reinterpret_cast<const Vec16*>(srcA + 16u * u);
            else
                for (uint32_t i = ia; i < ib; i++) image[i] = srcA[i];
        }
        __syncthreads();
        for (uint32_t i = tid; i < n; i += kThreads)
            atomicAdd(&hist[image[mis + i] * kHistCopies + (tid & (kHistCopies - 1))], 1u);
        const uint32_t crc = bam::block_crc(image, mis, n, crcT, red);  // with a barrier behind the histogram
        if (tid < 256) {
            uint32_t c = 0;
#pragma unroll
            for (uint32_t k = 0; k < kHistCopies; k++) c += hist[tid * kHistCopies + k];
            cnt[tid] = c;
        } else if (tid == 256) {
            cnt[256] = 1;
        }
        __syncthreads();
        build_lengths(cnt, kSyms, kLitLimit, len, bld);
        if (tid == 0) shared[0] = length_symbols(len, clSym, clCnt);
        __syncthreads();
        build_lengths(clCnt, kClSyms, kClLimit, clLen, bld);
        if (tid < kClSyms) clCode[tid] = canonical_entry(clLen, kClSyms, tid);
        __syncthreads();
        BlockPlan& plan = a.plans[t];
        uint64_t bits = 0;
        if (tid == 0) {
            const uint8_t order[kClSyms] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
            uint32_t hclen = 4;
            for (uint32_t i = 4; i < kClSyms; i++)
                if (clLen[order[i]]) hclen = i + 1;
            BitWriter bw{hdr};
            bw.put(1, 1);
            bw.put(2, 2);
            bw.put(0, 5);
            bw.put(1, 5);
            bw.put(hclen - 4, 4);
            for (uint32_t i = 0; i < hclen; i++) bw.put(clLen[order[i]], 3);
            const uint32_t ns = shared[0];
            for (uint32_t i = 0; i < ns; i++) {
                const uint32_t s = clSym[i] & 0xFFu, extra = clSym[i] >> 8;
                bw.put(clCode[s] & 0xFFFFu, clCode[s] >> 16);
                if (s >= 16) bw.put(extra, s == 16 ? 2 : s == 17 ? 3 : 7);
            }
            bw.finish();
            shared[1] = bw.total;
        } else if (tid >= 512 && tid < 512 + kSyms) {  // the literals' codes, by other waves than thread 0's
            const uint32_t s = tid - 512;
            const uint32_t e = canonical_entry(len, kSyms, s);
            plan.code[s] = e;
            bits = (uint64_t)cnt[s] * (e >> 16);
        }
        uint64_t before;
        bits = stitch::block_scan(bits, waveSum, before);  // with a barrier behind the header
        const uint32_t hdrBits = shared[1];
        const uint32_t dyn = (uint32_t)((hdrBits + bits + 7) / 8);
        if (tid == 0) {
            a.blkOff[t] = kFrame + (dyn < n + kStored ? dyn : n + kStored);
            plan.crc = crc;
            plan.hdrBits = hdrBits;
        }
        if (tid < kHdrBytes) plan.hdr[tid] = hdr[tid];
        __syncthreads();  // the next tile writes the image and the tables
    }
}

// the 18 bytes in front of a block of `size` file bytes at dst and the 8 behind, by threads 0..17 and 32..39
__device__ __forceinline__ void block_frame(uint8_t* dst, uint32_t size, uint32_t n, uint32_t crc)
{
    const uint32_t tid = threadIdx.x;
    if (tid < kFront) {
        const uint64_t h0 = 0x0000000004088B1Full;  // 1f 8b 08 04 00 00 00 00
        const uint64_t h1 = 0x000243420006FF00ull;  // 00 ff 06 00 42 43 02 00
        uint32_t b;
        if (tid < 8)
            b = (uint32_t)(h0 >> (8 * tid));
        else if (tid < 16)
            b = (uint32_t)(h1 >> (8 * (tid - 8)));
        else
            b = (size - 1) >> (8 * (tid - 16));
        dst[tid] = (uint8_t)b;
    } else if (tid >= 32 && tid < 40) {
        const uint32_t k = tid - 32;
        dst[size - 8 + k] = (uint8_t)((k < 4 ? crc : n) >> (8 * (k & 3u)));
    }
}

__global__ __launch_bounds__(kThreads) void deflate_pack_kernel(Args a)
{
    __shared__ __attribute__((aligned(16))) uint8_t image[kImage];
    __shared__ uint32_t tab[260];
    __shared__ uint64_t waveSum[kWaves];
    const uint32_t tid = threadIdx.x;
    const uint64_t W = stream_bytes(a);
    uint32_t* const words = reinterpret_cast<uint32_t*>(image);
    for (uint64_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        const uint64_t off = a.blkOff[t], end = a.blkOff[t + 1];
        const bool fits = end <= a.byteCapacity;
        if (tid == 0) {
            // the written blocks are a prefix: exactly one tile is its last, or the first does not fit
            const bool nextFits = t + 1 < a.ntiles && a.blkOff[t + 2] <= a.byteCapacity;
            if (fits && !nextFits) {
                const uint64_t used = (t + 1) * kBlock;
                a.written[0] = W < used ? W : used;
                a.written[1] = end;
            } else if (t == 0 && !fits) {
                a.written[0] = 0;
                a.written[1] = 0;
            }
        }
        const uint64_t olo = t * kBlock;
        if (olo >= W || !fits) continue;  // the whole workgroup
        const uint32_t n = (uint32_t)(W - olo < kBlock ? W - olo : kBlock);
        const uint32_t size = (uint32_t)(end - off), dlen = size - kFrame;  // the deflate bytes
        const bool stored = dlen == n + kStored;
        const BlockPlan& plan = a.plans[t];
        const uint8_t* const src = a.src + olo;
        uint8_t* const dst = a.out + off;
        uint8_t* const body = dst + kFront;
        const uint32_t mis = (uint32_t)((uintptr_t)body & 15u);
        if (stored) {
            if (tid < kStored) {
                const uint32_t nn = ~n & 0xFFFFu;
                image[mis + tid] = (uint8_t)(tid == 0 ? 1u : tid < 3 ? n >> (8 * (tid - 1)) : nn >> (8 * (tid - 3)));
            }
            const uint32_t p0 = mis + kStored;  // the payload's place in the image
#pragma unroll 1
            for (uint32_t j = 0; j < kRounds; j++) {
                const uint32_t u = j * kThreads + tid;
                const uint32_t ia = 16u * u > p0 ? 16u * u : p0, ib = 16u * u + 16u < p0 + n ? 16u * u + 16u : p0 + n;
                if (u >= kUnits || ia >= ib) continue;
                if (ib - ia == 16)
                    *reinterpret_cast<Vec16*>(image + 16u * u) = stitch::load16(src + (16u * u - p0));
                else
                    for (uint32_t i = ia; i < ib; i++) image[i] = src[i - p0];
            }
        } else {
#pragma unroll 1
            for (uint32_t j = 0; j < kRounds; j++) {
                const uint32_t u = j * kThreads + tid;
                if (u < kUnits) *reinterpret_cast<Vec16*>(image + 16u * u) = Vec16{0u, 0u, 0u, 0u};
            }
            if (tid < 260) tab[tid] = tid < kSyms ? plan.code[tid] : 0u;
            __syncthreads();
            const uint32_t hdrBits = plan.hdrBits;
            if (tid < (hdrBits + 7) / 8) {
                const uint32_t at = mis + tid;
                atomicOr(&words[at >> 2], (uint32_t)plan.hdr[tid] << (8 * (at & 3u)));
            }
            // this thread's run: the bits it needs, their place by the scan, then the bits
            const uint32_t r0 = kRun * tid, r1 = r0 + kRun < n ? r0 + kRun : n;
            const bool whole = r0 + kRun <= n;
            uint32_t v[kRun / 4];
            uint64_t mine = 0;
            if (whole) {
#pragma unroll
                for (uint32_t k = 0; k < kRun / 16; k++) {
                    const Vec16 x = stitch::load16(src + r0 + 16 * k);
#pragma unroll
                    for (uint32_t q = 0; q < 4; q++) v[4 * k + q] = x[q];
                }
#pragma unroll
                for (uint32_t i = 0; i < kRun; i++) mine += tab[(v[i / 4] >> (8 * (i & 3u))) & 0xFFu] >> 16;
            } else {
                for (uint32_t i = r0; i < r1; i++) mine += tab[src[i]] >> 16;
            }
            uint64_t before;
            const uint64_t all = stitch::block_scan(mine, waveSum, before);
            const uint64_t at = 8ull * mis + hdrBits + before;
            uint32_t* w = words + (at >> 5);
            uint64_t acc = 0;
            uint32_t nb = (uint32_t)at & 31u;
            auto put = [&](uint32_t e) {
                acc |= (uint64_t)(e & 0xFFFFu) << nb;
                nb += e >> 16;
                if (nb >= 32) {
                    atomicOr(w++, (uint32_t)acc);
                    acc >>= 32;
                    nb -= 32;
                }
            };
            if (whole) {
#pragma unroll
                for (uint32_t i = 0; i < kRun; i++) put(tab[(v[i / 4] >> (8 * (i & 3u))) & 0xFFu]);
            } else {
                for (uint32_t i = r0; i < r1; i++) put(tab[src[i]]);
            }
            if (nb) atomicOr(w, (uint32_t)acc);
            if (tid == 0) {  // the end of the block
                const uint64_t e = 8ull * mis + hdrBits + all;
                const uint64_t bitsE = (uint64_t)(tab[256] & 0xFFFFu) << (e & 31u);
                atomicOr(&words[e >> 5], (uint32_t)bitsE);
                if (bitsE >> 32) atomicOr(&words[(e >> 5) + 1], (uint32_t)(bitsE >> 32));
            }
        }
        __syncthreads();
        block_frame(dst, size, n, plan.crc);
        uint8_t* const bodyA = body - mis;
#pragma unroll 1
        for (uint32_t j = 0; j < kRounds; j++) {
            const uint32_t u = j * kThreads + tid;
            const uint32_t ia = 16u * u > mis ? 16u * u : mis, ib = 16u * u + 16u < mis + dlen ? 16u * u + 16u : mis + dlen;
            if (u >= kUnits || ia >= ib) continue;
            if (ib - ia == 16)
                *reinterpret_cast<Vec16*>(bodyA + 16u * u) = *reinterpret_cast<const Vec16*>(image + 16u * u);
            else
                for (uint32_t i = ia; i < ib; i++) bodyA[i] = image[i];
        }
        __syncthreads();  // the next tile writes the image
    }
}
#endif  // PGN_SELECT_HOST_ONLY

}  // namespace deflate
}  // namespace pgn

#endif  // PGN_DEFLATE_H
