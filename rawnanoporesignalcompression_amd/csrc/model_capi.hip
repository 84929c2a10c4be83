// model_capi.hip -- TEST-ONLY host build of the shared zstd level-1 encoder/decoder code
// (zstd1_model.h / zstd1_dec.h), so the test-suite can fuzz the exact code the GPU kernels run
// against libzstd at host speed.  Never loaded by the product path.
#include <stdlib.h>
#include <string.h>

#define PGN_SELECT_HOST_ONLY
#include "pgn_segment.h"
#include "pgn_select.h"
#include "zstd1_dec.h"
#include "zstd1_model.h"

using namespace pgn::z1;

extern "C" {

// ZSTD_compress(dst, cap, src, n, 1) equivalent; returns size or 0 on error/unsupported.
size_t z1m_compress(const uint8_t* src, size_t n, uint8_t* dst, size_t cap)
{
    if (n > 0xFFFFFFF0ull || cap < compress_bound(n)) return 0;
    uint32_t* ht = (uint32_t*)calloc((size_t)1 << 15, 4);
    size_t ns = kMaxSrc / 4 + 2;
    Seq* seqs = (Seq*)malloc(ns * sizeof(Seq));
    uint8_t* codes = (uint8_t*)malloc(3 * ns);
    uint8_t* litbuf = (uint8_t*)malloc(kMaxSrc + 1);
    CompressWork* w = (CompressWork*)malloc(sizeof(CompressWork));
    size_t r = compress_serial(dst, src, n, ht, seqs, codes, codes + ns, codes + 2 * ns, litbuf, *w);
    free(w); free(litbuf); free(codes); free(seqs); free(ht);
    return r;
}

// Sequences found by the level-1 match finder (for debugging parity): returns nbSeq.
size_t z1m_sequences(const uint8_t* src, size_t n, uint32_t* out3, size_t maxSeq)
{
    if (n < 7 || n > kMaxSrc) return 0;
    uint32_t* ht = (uint32_t*)calloc((size_t)1 << 15, 4);
    Seq* seqs = (Seq*)malloc((n / 4 + 2) * sizeof(Seq));
    size_t lastLL = 0;
    uint32_t rep[3] = {1, 4, 8};
    size_t nb = fast_search_serial(src, 0, n, level1_params(n), ht, rep, seqs, &lastLL);
    for (size_t i = 0; i < nb && i < maxSeq; i++) {
        out3[3 * i] = seqs[i].litLength; out3[3 * i + 1] = seqs[i].offset; out3[3 * i + 2] = seqs[i].mlBase;
    }
    free(seqs); free(ht);
    return nb;
}

// The encoder's no-match certificate (pgn_zenc.h no_match_certificate), serially: 1 when the
// level-1 search of the single-block frame src[0, n) provably finds no match.
static uint32_t cert_fmix32(uint32_t x)
{
    x ^= x >> 16;
    x *= 0x85EBCA6Bu;
    x ^= x >> 13;
    x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return x;
}
int z1m_no_match_certificate(const uint8_t* src, size_t n)
{
    if (n < 7 || n > kMaxSrc) return 0;
    const Params p = level1_params(n);
    const long ilimit = (long)n - 8;
    const uint32_t words = 8192 / 8, maxKeys = 2048;  // pgn_zenc.h kCertWords, kCertKeys
    uint64_t* filt = (uint64_t*)calloc(words, 8);
    int ok = 1;
    uint32_t e = 257, k = 0;
    for (;; k++) {
        if (k % 64 == 0 && 2 * (k + 64) > maxKeys) { ok = 0; break; }
        const long pk = (long)e - 256;
        e += e >> 7;
        if (!(pk + 1 < ilimit)) break;
        const uint64_t v8 = rd64(src + pk);
        if (rd32(src + pk + 1) == (uint32_t)(v8 >> 16)) { ok = 0; break; }  // repcode (offset 1) at ip0 + 2
        const uint32_t keys[2] = {(uint32_t)v8 ^ (hash_word(v8, p.hashLog, p.mls) * 0x9E3779B1u),
                                  (uint32_t)(v8 >> 8) ^ (hash_word(v8 >> 8, p.hashLog, p.mls) * 0x9E3779B1u)};
        for (int j = 0; j < 2 && ok; j++) {  // blocked Bloom filter: six bits of one 64-bit word
            const uint32_t a = cert_fmix32(keys[j]), b = cert_fmix32(keys[j] ^ 0x5BD1E995u);
            const uint64_t m = (1ull << (a & 63u)) | (1ull << ((a >> 6) & 63u)) | (1ull << ((a >> 12) & 63u)) |
                               (1ull << ((a >> 18) & 63u)) | (1ull << ((a >> 24) & 63u)) | (1ull << (b & 63u));
            uint64_t* w = filt + ((b >> 6) & (words - 1));
            if ((*w & m) == m) ok = 0;
            *w |= m;
        }
        if (!ok) break;
    }
    free(filt);
    return ok;
}

long z1m_decompress(const uint8_t* src, size_t n, uint8_t* dst, size_t cap)
{
    DecWork* w = (DecWork*)malloc(sizeof(DecWork));
    long r = decompress_frames(src, n, dst, cap, *w);
    free(w);
    return r;
}

// HUF_buildCTable's code lengths for a histogram (maxNbBits 11): decode-table size studies.
unsigned z1m_huf_lengths(const uint32_t* count, unsigned maxSymbolValue, uint8_t* nbBits)
{
    HufNode* nodes = (HufNode*)calloc(1024, sizeof(HufNode));
    huf_sort_serial(nodes + 1, count, maxSymbolValue);
    uint16_t val[256];
    const unsigned r = huf_build_from_sorted(nodes, maxSymbolValue, 11, nbBits, val);
    free(nodes);
    return r;
}

long long z1m_content_size(const uint8_t* src, size_t n)
{
    bool ok = false;
    uint64_t v = frame_content_size(src, n, &ok);
    return ok ? (long long)v : -1;
}

// The read statistics (pgn_select.h) over serially built histograms: the rank walk, the keys and the
// integer -> float step the kernels run.  Returns 0, or -1 for parameters the C ABI rejects.
int pgnm_read_stats(const int16_t* x, uint64_t n, const pgn_norm_params* prm, pgn_read_stats* out)
{
    if (!pgn::sel::params_valid(prm) || !out) return -1;
    pgn::sel::host_read_stats(x, n, *prm, *out);
    return 0;
}

// The two-level coarse walk alone: coarse[1024] and nranks (1 or 2) ranks -> bin and residual rank.
int pgnm_locate(const uint32_t* coarse, const uint32_t* k, int nranks, uint32_t* bin, uint32_t* resid)
{
    using namespace pgn::sel;
    uint32_t groups[kGroups] = {};
    for (uint32_t b = 0; b < kCoarseBins; b++) groups[b / kGroupBins] += coarse[b];
    if (nranks == 1) {
        const uint32_t k1[1] = {k[0]};
        Place p[1];
        locate<1>(groups, coarse, k1, p);
        bin[0] = p[0].bin; resid[0] = p[0].resid;
    } else if (nranks == 2) {
        const uint32_t k2[2] = {k[0], k[1]};
        Place p[2];
        locate<2>(groups, coarse, k2, p);
        for (int i = 0; i < 2; i++) { bin[i] = p[i].bin; resid[i] = p[i].resid; }
    } else {
        return -1;
    }
    return 0;
}

// The plan of a long read's selection (pgn_select.h split_parts / part_begin): *parts of them, and the
// first min(*parts + 1, max) part boundaries (begin[j] is where part j starts; begin[*parts] == n).
// Returns 0, or -1 for settings pgn_ctx_set_select_split rejects.
int pgnm_select_parts(uint64_t n, uint32_t split_min_samples, uint32_t part_samples, uint32_t* parts, uint64_t max,
                      uint64_t* begin)
{
    const pgn_select_split s{split_min_samples, part_samples, 0, 0};
    if (!pgn::sel::split_valid(&s) || !parts) return -1;
    *parts = pgn::sel::split_parts(n, split_min_samples, part_samples);
    for (uint64_t j = 0; j <= *parts && j < max; j++) begin[j] = pgn::sel::part_begin(n, *parts, (uint32_t)j);
    return 0;
}

// The head trim (pgn_segment.h) of one read: the selection above over the head, the threshold and the
// window scan as the header writes it.  Returns 0, or -1 for parameters the C ABI rejects.
int pgnm_trim(const int16_t* x, uint64_t n, const pgn_trim_params* prm, uint32_t* trim, int32_t* head_m2,
              uint32_t* head_mad4, float* threshold)
{
    if (!pgn::seg::trim_params_valid(prm) || !trim) return -1;
    const pgn::seg::TrimResult r = pgn::seg::host_trim(x, n, *prm);
    *trim = r.trim;
    if (head_m2) *head_m2 = r.m2;
    if (head_mad4) *head_mad4 = r.mad4;
    if (threshold) *threshold = r.thr;
    return 0;
}

// The segments of a trimmed read of m samples: *nseg of them, and the first min(*nseg, max) starts and
// valid counts.  Returns 0, or -1 for parameters the C ABI rejects.
int pgnm_segment_plan(uint64_t m, const pgn_segment_params* prm, uint64_t* nseg, uint64_t max, uint64_t* start,
                      uint32_t* valid)
{
    using namespace pgn::seg;
    if (!segment_params_valid(prm) || !nseg) return -1;
    const uint32_t L = prm->length, S = prm->length - prm->overlap;
    *nseg = segment_count(m, L, S);
    for (uint64_t j = 0; j < *nseg && j < max; j++) {
        start[j] = segment_start(m, L, S, j);
        valid[j] = segment_valid(m, L);
    }
    return 0;
}

}  // extern "C"
