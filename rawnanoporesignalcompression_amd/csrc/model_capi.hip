// model_capi.hip -- TEST-ONLY host build of the shared zstd level-1 encoder/decoder code
// (zstd1_model.h / zstd1_dec.h), so the test-suite can fuzz the exact code the GPU kernels run
// against libzstd at host speed.  Never loaded by the product path.
#include <stdlib.h>
#include <string.h>

#define PGN_SELECT_HOST_ONLY
#include "pgn_segment.h"
#include "pgn_select.h"
#include "pgn_stitch.h"
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

// Search profile of a single-block frame (n <= 128 KiB): fast_search_serial restated with the
// bookkeeping that says which of the wave search's paths (pgn_zenc.h fast_search_wave) a sequence
// takes there.  Visits are numbered from the last match (k) and grouped in 64s, as the wave's rounds
// are.  One row of kProfileCols words per sequence:
//   0 position of the match (after the backward extension)      1 k (0 for a post-match repcode)
//   2 kind: 0 repcode at ip0 + 2, 1 table candidate, 2 candidate written by an earlier visit of the
//     same group of 64, 3 post-match repcode                     3 backward extension
//   4 match length    5 1 when the match ran to the stream's end
//   6 lookups of the group, at or before the hit, whose table candidate (not one of the group's own
//     writes) had the entry's fingerprint (pgn_zenc.h ht_fp at ht_idx_bits(n)) but other 4 bytes
//   7 litLength   8 offset value   9 matchLength - 3   (z1m_sequences' triple)
// Returns the number of sequences; writes the first max_rows rows.
static const size_t kProfileCols = 10;
size_t z1m_search_profile(const uint8_t* src, size_t n, uint32_t* rows, size_t max_rows)
{
    if (n < 7 || n > kMaxSrc) return 0;
    const Params p = level1_params(n);
    const unsigned hlog = p.hashLog, mls = p.mls;
    const uint32_t idxBits = (n + 2 < (1u << 17)) ? 17u : 20u;
    auto fp = [&](uint32_t bytes) { return (bytes * 0x9E3779B1u) >> (32u - (27u - idxBits)); };
    uint32_t* ht = (uint32_t*)calloc((size_t)1 << 15, 4);
    uint32_t* wr = (uint32_t*)calloc((size_t)1 << 15, 4);  // who wrote the entry: (segment << 5 | group) + 1, 0 after a match
    size_t nbSeq = 0;
    auto row = [&](long pos, uint32_t k, uint32_t kind, uint32_t back, size_t ml, bool toEnd, uint32_t nfalse, long ll,
                   uint32_t offset) {
        if (nbSeq < max_rows) {
            uint32_t* r = rows + kProfileCols * nbSeq;
            r[0] = (uint32_t)pos; r[1] = k; r[2] = kind; r[3] = back; r[4] = (uint32_t)ml; r[5] = toEnd ? 1u : 0u;
            r[6] = nfalse; r[7] = (uint32_t)ll; r[8] = offset; r[9] = (uint32_t)(ml - 3);
        }
        nbSeq++;
    };
    long ip0 = 1, ip1 = 2, anchor = 0;
    const long iend = (long)n, ilimit = (long)n - 8;
    const uint32_t lowIdx = 1;
    uint32_t offset_1 = 1, offset_2 = 0;  // offset_2 (4) lies beyond the first position: invalidated
    uint32_t segment = 0, k = 0, nfalse = 0;
    while (ip1 < ilimit) {
        const long ip2 = ip0 + 2;
        if (k % 64 == 0) nfalse = 0;
        const uint32_t me = ((segment << 5) | (k / 64)) + 1;  // k / 64 < 21: a block's chain has under 1344 visits
        const uint32_t h0 = hash_at(src + ip0, hlog, mls), h1 = hash_at(src + ip1, hlog, mls);
        const uint32_t val0 = rd32(src + ip0), val1 = rd32(src + ip1);
        const uint32_t cur0 = (uint32_t)ip0 + 1, cur1 = (uint32_t)ip1 + 1;
        const uint32_t mi0 = ht[h0], mi1 = ht[h1];
        const bool own0 = wr[h0] == me, own1 = wr[h1] == me;
        ht[h0] = cur0; wr[h0] = me;
        ht[h1] = cur1; wr[h1] = me;
        long match0;
        size_t mLength;
        uint32_t offcode, kind, back = 0;
        if ((offset_1 > 0) && (rd32(src + ip2 - offset_1) == rd32(src + ip2))) {
            mLength = (src[ip2 - 1] == src[ip2 - (long)offset_1 - 1]) ? 1 : 0;
            ip0 = ip2 - (long)mLength;
            match0 = ip0 - (long)offset_1;
            mLength += 4;
            offcode = 0;
            kind = 0;
        } else {
            const bool eq0 = (mi0 > lowIdx) && rd32(src + mi0 - 1) == val0;
            const bool eq1 = (mi1 > lowIdx) && rd32(src + mi1 - 1) == val1;
            if ((mi0 > lowIdx) && !eq0 && !own0 && fp(rd32(src + mi0 - 1)) == fp(val0)) nfalse++;
            if (!eq0 && (mi1 > lowIdx) && !eq1 && !own1 && fp(rd32(src + mi1 - 1)) == fp(val1)) nfalse++;
            if (eq0) {
                match0 = (long)mi0 - 1;
                kind = own0 ? 2 : 1;
            } else if (eq1) {
                ip0 = ip1;
                match0 = (long)mi1 - 1;
                kind = own1 ? 2 : 1;
            } else {
                const long step = ((ip0 - anchor) >> 7) + 2;
                ip0 += step;
                ip1 += step;
                k++;
                continue;
            }
            offset_2 = offset_1;
            offset_1 = (uint32_t)(ip0 - match0);
            offcode = offset_1 + 2;
            mLength = 4;
            while ((ip0 > anchor) && (match0 > 0) && (src[ip0 - 1] == src[match0 - 1])) {
                ip0--;
                match0--;
                mLength++;
                back++;
            }
        }
        mLength += match_count(src, (size_t)ip0 + mLength, (size_t)match0 + mLength, (size_t)iend);
        row(ip0, k, kind, back, mLength, ip0 + (long)mLength == iend, nfalse, ip0 - anchor, offcode + 1);
        ip0 += (long)mLength;
        anchor = ip0;
        if (ip0 <= ilimit) {
            const uint32_t ha = hash_at(src + cur0 + 1, hlog, mls), hb = hash_at(src + ip0 - 2, hlog, mls);
            ht[ha] = cur0 + 2; wr[ha] = 0;
            ht[hb] = (uint32_t)(ip0 - 2) + 1; wr[hb] = 0;
            if (offset_2 > 0) {
                while ((ip0 <= ilimit) && (rd32(src + ip0) == rd32(src + ip0 - offset_2))) {
                    const size_t rLength = match_count(src, (size_t)ip0 + 4, (size_t)ip0 + 4 - offset_2, (size_t)iend) + 4;
                    const uint32_t t = offset_2; offset_2 = offset_1; offset_1 = t;
                    const uint32_t hr = hash_at(src + ip0, hlog, mls);
                    ht[hr] = (uint32_t)ip0 + 1; wr[hr] = 0;
                    row(ip0, 0, 3, 0, rLength, ip0 + (long)rLength == iend, 0, 0, 1);
                    ip0 += (long)rLength;
                    anchor = ip0;
                }
            }
        }
        ip1 = ip0 + 1;
        segment++;
        k = 0;
    }
    free(wr); free(ht);
    return nbSeq;
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

// The level-1 search of the single-block frame src[0, n), n <= 128 KiB, from an empty table.
// mode 0: fast_search_serial.  mode 1: the encoder's dispatch -- small_search_serial (zstd1_model.h)
// for n <= kSmallSearchBytes, and the general search otherwise or when the small search's log
// overflows.  Writes the first maxSeq (litLength, offset, mlBase) triples and
//   info[0] 1 when the small search produced the result   info[1] 1 when its log overflowed
//   info[2] nbSeq   info[3] last literal run   info[4], info[5] repeat offsets on exit
//   info[6..14] the small search's rounds, log entries, keys flagged by the filter, flagged keys
//               the log refuted, log scans, and SmallSearchInfo's refutedAbsent, shadowed, fpThenHit, repFirst
// Returns nbSeq, or (size_t)-1 for a size out of range.
size_t z1m_small_search(const uint8_t* src, size_t n, int mode, uint32_t* out3, size_t maxSeq, uint32_t* info)
{
    if (n < 7 || n > kMaxSrc) return (size_t)-1;
    const Params p = level1_params(n);
    Seq* seqs = (Seq*)malloc((n / 4 + 2) * sizeof(Seq));
    size_t lastLL = 0, nb = (size_t)-1;
    uint32_t rep[3] = {1, 4, 8};
    for (int i = 0; i < 15; i++) info[i] = 0;
    if (mode == 1 && n <= kSmallSearchBytes) {
        SmallSearchWork* w = (SmallSearchWork*)malloc(sizeof(SmallSearchWork));
        SmallSearchInfo si;
        nb = small_search_serial(src, n, p, rep, seqs, &lastLL, *w, &si);
        free(w);
        info[0] = nb != (size_t)-1;
        info[1] = nb == (size_t)-1;
        info[6] = si.rounds; info[7] = si.logEntries; info[8] = si.flagged; info[9] = si.falsePositives; info[10] = si.scans;
        info[11] = si.refutedAbsent; info[12] = si.shadowed; info[13] = si.fpThenHit; info[14] = si.repFirst;
    }
    if (nb == (size_t)-1) {
        uint32_t* ht = (uint32_t*)calloc((size_t)1 << 15, 4);
        rep[0] = 1; rep[1] = 4;
        nb = fast_search_serial(src, 0, n, p, ht, rep, seqs, &lastLL);
        free(ht);
    }
    info[2] = (uint32_t)nb; info[3] = (uint32_t)lastLL; info[4] = rep[0]; info[5] = rep[1];
    for (size_t i = 0; i < nb && i < maxSeq; i++) {
        out3[3 * i] = seqs[i].litLength; out3[3 * i + 1] = seqs[i].offset; out3[3 * i + 2] = seqs[i].mlBase;
    }
    free(seqs);
    return nb;
}
unsigned z1m_small_search_bytes(void) { return kSmallSearchBytes; }
unsigned z1m_small_search_log_cap(void) { return kSmallLogCap; }

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

// The kept frames (pgn_stitch.h) of a taken read's k segments, given their table starts and valid counts:
// the function the plan kernel runs per row.  Returns 0, or -1 for parameters the C ABI rejects.
int pgnm_stitch_frames(const pgn_stitch_params* prm, uint64_t k, const uint32_t* start, const uint32_t* valid,
                       uint32_t* first, uint32_t* count)
{
    using namespace pgn::stitch;
    if (!params_valid(prm)) return -1;
    const uint32_t L = prm->length, s = prm->frame_samples, T = L / s;
    for (uint64_t j = 0; j < k; j++)
        kept_frames(j ? start[j - 1] : 0, start[j], j + 1 < k ? start[j + 1] : 0, valid[j], j == 0, j + 1 == k, L, s, T,
                    first[j], count[j]);
    return 0;
}

}  // extern "C"
