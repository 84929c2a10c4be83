// zstd1_model.h -- serial composition of zstd1_common.h into a full `ZSTD_compress(.., 1)` for one
// source (a single-segment frame up to 512 KiB, a window-descriptor frame above).
//
// Host and device: the GPU kernels run the serial parts of these on one lane; the host build
// (libpgn_model.so, test-only) lets the test-suite fuzz the exact same code against libzstd.
//
// Parts of this file restate algorithms of Zstandard (libzstd 1.4.x), Copyright (c) 2016-present,
// Facebook, Inc., used under its BSD licence: see THIRD_PARTY_NOTICES.md at the repository root.
#pragma once
#include "zstd1_common.h"

namespace pgn {
namespace z1 {

// ---------------------------------------------------------------------------------------------
// ZSTD_compressBlock_fast (libzstd 1.4.x, two positions per step, kSearchStrength 8, stepSize 2) over
// the block [start, end) of a frame: window base = src - 1 (table entries hold indices = offset + 1,
// and persist across the blocks of a frame; the caller zeroes the table once per frame).  A source
// within the window (single segment, n <= 2^windowLog) has prefixStartIndex 1; above it, the block's
// candidates must lie within 2^windowLog of the block's end (ZSTD_getLowestPrefixIndex).  rep[0..1] are the confirmed
// repeat offsets on entry and the block's candidates on exit (ZSTD_compressBlock_fast_generic's
// offsetSaved rule); at the first position of the frame, offset_2 (4) > maxRep (1) is invalidated.
// Appends sequences (literal runs are implied: src[anchor .. anchor + litLength)); returns nbSeq,
// *lastLL = trailing literal run of the block.
// ---------------------------------------------------------------------------------------------
PGN_HD size_t match_count(const uint8_t* src, size_t a, size_t b, size_t end)
{
    size_t n = 0;
    while (a + n < end && src[a + n] == src[b + n]) n++;
    return n;
}

PGN_HD size_t fast_search_serial(const uint8_t* src, size_t start, size_t end, const Params& p, uint32_t* ht,
                                 uint32_t rep[3], Seq* seqs, size_t* lastLL)
{
    const unsigned hlog = p.hashLog, mls = p.mls;
    size_t nbSeq = 0;
    long ip0 = (long)start + (start == 0 ? 1 : 0), anchor = (long)start;
    long ip1 = ip0 + 1;
    const long iend = (long)end, ilimit = (long)end - 8;
    // ZSTD_getLowestPrefixIndex: candidates must lie within the window of the block's end
    const uint32_t lowIdx = window_low_index(end, p.windowLog);
    const long prefixStart = (long)lowIdx - 1;  // its position
    uint32_t offset_1 = rep[0], offset_2 = rep[1], offsetSaved = 0;
    {
        // current - windowLow at the first position
        const uint32_t maxRep = (uint32_t)ip0 + 1u - window_low_index((size_t)ip0, p.windowLog);
        if (offset_2 > maxRep) { offsetSaved = offset_2; offset_2 = 0; }
        if (offset_1 > maxRep) { offsetSaved = offset_1; offset_1 = 0; }
    }
    while (ip1 < ilimit) {
        long ip2 = ip0 + 2;
        uint32_t h0 = hash_at(src + ip0, hlog, mls);
        uint32_t h1 = hash_at(src + ip1, hlog, mls);
        uint32_t val0 = rd32(src + ip0), val1 = rd32(src + ip1);
        uint32_t cur0 = (uint32_t)ip0 + 1, cur1 = (uint32_t)ip1 + 1;
        uint32_t mi0 = ht[h0], mi1 = ht[h1];
        ht[h0] = cur0;
        ht[h1] = cur1;
        long match0;
        size_t mLength;
        uint32_t offcode;
        if ((offset_1 > 0) && (rd32(src + ip2 - offset_1) == rd32(src + ip2))) {
            mLength = (src[ip2 - 1] == src[ip2 - (long)offset_1 - 1]) ? 1 : 0;
            ip0 = ip2 - (long)mLength;
            match0 = ip0 - (long)offset_1;
            mLength += 4;
            offcode = 0;
        } else {
            bool found = false;
            if ((mi0 > lowIdx) && rd32(src + mi0 - 1) == val0) {
                match0 = (long)mi0 - 1;
                found = true;
            } else if ((mi1 > lowIdx) && rd32(src + mi1 - 1) == val1) {
                ip0 = ip1;
                match0 = (long)mi1 - 1;
                found = true;
            }
            if (!found) {
                long step = ((ip0 - anchor) >> 7) + 2;
                ip0 += step;
                ip1 += step;
                continue;
            }
            offset_2 = offset_1;
            offset_1 = (uint32_t)(ip0 - match0);
            offcode = offset_1 + 2;
            mLength = 4;
            while ((ip0 > anchor) && (match0 > prefixStart) && (src[ip0 - 1] == src[match0 - 1])) {
                ip0--;
                match0--;
                mLength++;
            }
        }
        mLength += match_count(src, (size_t)ip0 + mLength, (size_t)match0 + mLength, (size_t)iend);
        seqs[nbSeq].litLength = (uint32_t)(ip0 - anchor);
        seqs[nbSeq].offset = offcode + 1;
        seqs[nbSeq].mlBase = (uint32_t)(mLength - 3);
        nbSeq++;
        ip0 += (long)mLength;
        anchor = ip0;
        if (ip0 <= ilimit) {
            ht[hash_at(src + cur0 + 1, hlog, mls)] = cur0 + 2;
            ht[hash_at(src + ip0 - 2, hlog, mls)] = (uint32_t)(ip0 - 2) + 1;
            if (offset_2 > 0) {
                while ((ip0 <= ilimit) && (rd32(src + ip0) == rd32(src + ip0 - offset_2))) {
                    size_t rLength = match_count(src, (size_t)ip0 + 4, (size_t)ip0 + 4 - offset_2, (size_t)iend) + 4;
                    uint32_t t = offset_2; offset_2 = offset_1; offset_1 = t;
                    ht[hash_at(src + ip0, hlog, mls)] = (uint32_t)ip0 + 1;
                    ip0 += (long)rLength;
                    seqs[nbSeq].litLength = 0;
                    seqs[nbSeq].offset = 1;
                    seqs[nbSeq].mlBase = (uint32_t)(rLength - 3);
                    nbSeq++;
                    anchor = ip0;
                }
            }
        }
        ip1 = ip0 + 1;
    }
    rep[0] = offset_1 ? offset_1 : offsetSaved;
    rep[1] = offset_2 ? offset_2 : offsetSaved;
    *lastLL = (size_t)(iend - anchor);
    return nbSeq;
}

// ---------------------------------------------------------------------------------------------
// The same search for a small single-block frame (start 0, n <= kSmallSearchBytes) without a hash
// table: the model of an on-chip search, in the wave search's rounds of 64 speculated visits
// (pgn_zenc.h fast_search_wave).
//   * Committed table writes are appended, in the serial loop's order, to a log of (hash, index);
//     "the table's entry for hash h" is the latest log entry with hash h.
//   * A visit asks the log only when a blocked Bloom filter over the keys (hash, first 4 bytes) of
//     earlier rounds says that an equal key may have been written.  A key the filter calls absent
//     cannot match: the table's entry for its hash, whatever it is, then holds other 4 bytes.  The
//     filter is tested before the round's own keys go in (all 64 visits', also those speculated
//     past the round's hit: they only add false positives; the log takes committed writes only).
//   * Inside a round, a visit sees the writes of the visits before it exactly (their hashes and
//     bytes are at hand), as the wave search does.
//   * Only the round's first hit is resolved: a flagged key whose latest log entry does not match 4
//     bytes is dropped and the next hit taken.
//   * A round whose first visit's repcode holds is decided at once: that visit's two writes are
//     committed, nothing else is hashed, asked or speculated.
// Returns nbSeq, or (size_t)-1 when the log overflows (the caller then runs the general search from
// the start: the bytes never differ).
// ---------------------------------------------------------------------------------------------
constexpr uint32_t kSmallSearchBytes = 2048;
constexpr uint32_t kSmallLogCap = 688;      // log entries: hash << 16 | index (position + 1); what the codec LDS leaves
constexpr uint32_t kSmallBloomWords = 128;  // 64-bit filter words
struct SmallSearchWork {
    uint32_t log[kSmallLogCap];
    uint64_t bloom[kSmallBloomWords];
};
struct SmallSearchInfo {
    uint32_t rounds, logEntries, flagged, falsePositives, scans;
    uint32_t refutedAbsent;  // flagged keys whose hash the log does not hold (a visit speculated past a hit left the key)
    uint32_t shadowed;       // flagged keys refuted by a later entry of their hash, an older entry holding their 4 bytes
    uint32_t fpThenHit;      // rounds that dropped a flagged key and then found their match
    uint32_t repFirst;       // rounds decided by the repcode of their first visit
};
PGN_HD uint32_t small_fmix32(uint32_t x)
{
    x ^= x >> 16;
    x *= 0x85EBCA6Bu;
    x ^= x >> 13;
    x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return x;
}
// the filter word and the four bits of the key (hash h, 4 bytes v): one mix, 31 of its bits (a block
// holds a few hundred keys in 128 words, so four bits of a word keep false positives near 1 in 10^4)
PGN_HD uint64_t small_bloom_bits(uint32_t h, uint32_t v, uint32_t* word)
{
    const uint32_t a = small_fmix32(v ^ (h * 0x9E3779B1u));
    *word = (a >> 24) & (kSmallBloomWords - 1u);
    return (1ull << (a & 63u)) | (1ull << ((a >> 6) & 63u)) | (1ull << ((a >> 12) & 63u)) | (1ull << ((a >> 18) & 63u));
}
PGN_HD size_t small_search_serial(const uint8_t* src, size_t n, const Params& p, uint32_t rep[3], Seq* seqs, size_t* lastLL,
                                  SmallSearchWork& W, SmallSearchInfo* info)
{
    const unsigned hlog = p.hashLog, mls = p.mls;
    const long iend = (long)n, ilimit = (long)n - 8;
    const uint32_t lowIdx = 1;  // a frame within its window
    size_t nbSeq = 0;
    long anchor = 0;
    uint32_t off1 = rep[0], off2 = rep[1], offSaved = 0;
    if (off2 > 1) { offSaved = off2; off2 = 0; }  // maxRep at the frame's first position is 1
    if (off1 > 1) { offSaved = off1; off1 = 0; }
    uint32_t logN = 0;
    for (uint32_t i = 0; i < kSmallBloomWords; i++) W.bloom[i] = 0;
    SmallSearchInfo I = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    bool overflow = false;
    auto bloom_add = [&](uint32_t h, uint32_t v) {
        uint32_t w;
        const uint64_t m = small_bloom_bits(h, v, &w);
        W.bloom[w] |= m;
    };
    auto bloom_has = [&](uint32_t h, uint32_t v) {
        uint32_t w;
        const uint64_t m = small_bloom_bits(h, v, &w);
        return (W.bloom[w] & m) == m;
    };
    auto log_add = [&](uint32_t h, uint32_t idx) {
        if (logN >= kSmallLogCap) { overflow = true; return; }
        W.log[logN++] = (h << 16) | idx;
    };
    auto log_latest = [&](uint32_t h) -> uint32_t {  // the index, 0 if the hash was never written
        for (uint32_t i = logN; i > 0; i--)
            if ((W.log[i - 1] >> 16) == h) return W.log[i - 1] & 0xFFFFu;
        return 0;
    };
    uint32_t e0 = 257;  // the round's first visit: e = ip0 - anchor + 256 (257: the frame's first position is 1)
    long ip0 = 1;
    while (ip0 + 1 < ilimit && !overflow) {
        I.rounds++;
        long pk[64];
        uint32_t h0[64], h1[64], v0[64], v1[64], m0[64], m1[64];
        bool valid[64], repk[64], c0[64], c1[64], fw0[64], fw1[64];
        uint32_t e = e0;
        int nValid = 0;
        for (int k = 0; k < 64; k++) {
            pk[k] = (long)e - 256 + anchor;
            e += e >> 7;
            valid[k] = pk[k] + 1 < ilimit;
            repk[k] = c0[k] = c1[k] = fw0[k] = fw1[k] = false;
            m0[k] = m1[k] = 0;
            if (!valid[k]) continue;
            nValid = k + 1;
            const uint64_t v8 = rd64(src + pk[k]);
            h0[k] = hash_word(v8, hlog, mls);
            h1[k] = hash_word(v8 >> 8, hlog, mls);
            v0[k] = (uint32_t)v8;
            v1[k] = (uint32_t)(v8 >> 8);
            repk[k] = off1 > 0 && rd32(src + pk[k] + 2 - (long)off1) == (uint32_t)(v8 >> 16);
            // the repcode of the round's first visit decides the round before anything is asked of the
            // table: only that visit's two writes are committed, and nothing is speculated
            if (k == 0 && repk[0]) {
                I.repFirst++;
                break;
            }
            // the latest write of an earlier visit of this round to my slots (ip1's after ip0's)
            uint32_t d0 = 0, d1 = 0;
            for (int j = k - 1; j >= 0 && !fw0[k]; j--) {
                if (h1[j] == h0[k]) { m0[k] = (uint32_t)pk[j] + 2; d0 = v1[j]; fw0[k] = true; }
                else if (h0[j] == h0[k]) { m0[k] = (uint32_t)pk[j] + 1; d0 = v0[j]; fw0[k] = true; }
            }
            for (int j = k - 1; j >= 0 && !fw1[k]; j--) {
                if (h1[j] == h1[k]) { m1[k] = (uint32_t)pk[j] + 2; d1 = v1[j]; fw1[k] = true; }
                else if (h0[j] == h1[k]) { m1[k] = (uint32_t)pk[j] + 1; d1 = v0[j]; fw1[k] = true; }
            }
            // (visits run to pk + 1 < ilimit in order, so every valid visit has its predecessors valid)
            c0[k] = fw0[k] ? (m0[k] > lowIdx && d0 == v0[k]) : bloom_has(h0[k], v0[k]);
            c1[k] = fw1[k] ? (m1[k] > lowIdx && d1 == v1[k]) : bloom_has(h1[k], v1[k]);
            if (!fw0[k] && c0[k]) I.flagged++;
            if (!fw1[k] && c1[k]) I.flagged++;
        }
        for (int k = 0; k < nValid; k++) {  // the round's keys, speculated ones included
            bloom_add(h0[k], v0[k]);
            bloom_add(h1[k], v1[k]);
        }
        // the first hit, a flagged key resolved against the log
        int f = 64;
        uint32_t fwdKnown = 0;
        bool dropped = false;
        for (int k = 0; k < nValid && f == 64; k++) {
            while (repk[k] || c0[k] || c1[k]) {
                if (repk[k]) { f = k; break; }
                const bool isC0 = c0[k];
                if (isC0 ? fw0[k] : fw1[k]) { f = k; break; }
                I.scans++;
                const uint32_t mf = log_latest(isC0 ? h0[k] : h1[k]);
                const size_t nm = mf > lowIdx ? match_count(src, (size_t)pk[k] + (isC0 ? 0 : 1), mf - 1, (size_t)iend) : 0;
                if (nm >= 4) {
                    (isC0 ? m0[k] : m1[k]) = mf;
                    fwdKnown = (uint32_t)nm;
                    f = k;
                    break;
                }
                I.falsePositives++;
                dropped = true;
                if (mf == 0) I.refutedAbsent++;
                else {
                    const uint32_t hq = isC0 ? h0[k] : h1[k], vq = isC0 ? v0[k] : v1[k];
                    bool older = false;
                    for (uint32_t i = 0; i < logN; i++)
                        if ((W.log[i] >> 16) == hq && rd32(src + (W.log[i] & 0xFFFFu) - 1) == vq) older = true;
                    if (older) I.shadowed++;
                }
                if (isC0) c0[k] = false;
                else c1[k] = false;
            }
        }
        if (dropped && f < 64) I.fpThenHit++;
        const int lastCommit = f < 64 ? f : nValid - 1;
        for (int k = 0; k <= lastCommit; k++) {
            log_add(h0[k], (uint32_t)pk[k] + 1);
            log_add(h1[k], (uint32_t)pk[k] + 2);
        }
        if (overflow) break;
        if (f == 64) {
            if (nValid < 64) break;
            ip0 = (long)e - 256 + anchor;
            e0 = e;
            continue;
        }
        // the match at visit f, as the serial loop processes it
        const long ipf = pk[f];
        const uint32_t cur0 = (uint32_t)ipf + 1;
        long ipm, match0;
        size_t mLength;
        uint32_t offcode;
        if (repk[f]) {
            const long ip2 = ipf + 2;
            mLength = (src[ip2 - 1] == src[ip2 - (long)off1 - 1]) ? 1 : 0;
            ipm = ip2 - (long)mLength;
            match0 = ipm - (long)off1;
            mLength += 4;
            offcode = 0;
        } else {
            if (c0[f]) { ipm = ipf; match0 = (long)m0[f] - 1; }
            else { ipm = ipf + 1; match0 = (long)m1[f] - 1; }
            off2 = off1;
            off1 = (uint32_t)(ipm - match0);
            offcode = off1 + 2;
            mLength = 4;
            while (ipm > anchor && match0 > 0 && src[ipm - 1] == src[match0 - 1]) {
                ipm--;
                match0--;
                mLength++;
            }
        }
        // (the forward part starts 4 bytes past the candidate, whatever the backward extension)
        mLength += fwdKnown ? fwdKnown - 4 : match_count(src, (size_t)ipm + mLength, (size_t)match0 + mLength, (size_t)iend);
        seqs[nbSeq].litLength = (uint32_t)(ipm - anchor);
        seqs[nbSeq].offset = offcode + 1;
        seqs[nbSeq].mlBase = (uint32_t)(mLength - 3);
        nbSeq++;
        ip0 = ipm + (long)mLength;
        anchor = ip0;
        e0 = 256;
        if (ip0 <= ilimit) {
            auto insert = [&](long pos) {
                const uint64_t w = rd64(src + pos);
                const uint32_t h = hash_word(w, hlog, mls);
                log_add(h, (uint32_t)pos + 1);
                bloom_add(h, (uint32_t)w);
            };
            insert((long)cur0 + 1);
            insert(ip0 - 2);
            if (off2 > 0) {
                while (ip0 <= ilimit && rd32(src + ip0) == rd32(src + ip0 - (long)off2)) {
                    const size_t rLength = match_count(src, (size_t)ip0 + 4, (size_t)ip0 + 4 - off2, (size_t)iend) + 4;
                    const uint32_t t = off2;
                    off2 = off1;
                    off1 = t;
                    insert(ip0);
                    ip0 += (long)rLength;
                    seqs[nbSeq].litLength = 0;
                    seqs[nbSeq].offset = 1;
                    seqs[nbSeq].mlBase = (uint32_t)(rLength - 3);
                    nbSeq++;
                    anchor = ip0;
                }
            }
        }
    }
    I.logEntries = logN;
    if (info) *info = I;
    if (overflow) return (size_t)-1;
    rep[0] = off1 ? off1 : offSaved;
    rep[1] = off2 ? off2 : offSaved;
    *lastLL = (size_t)(iend - anchor);
    return nbSeq;
}

// ---------------------------------------------------------------------------------------------
// Literals section (ZSTD_compressLiterals -> HUF_compress{1,4}X_repeat).  `prev` is the Huffman
// table state the frame carries from its last compressed block (HUF_repeat_none on the first
// block; HUF_repeat_check once a table was built -- level 1 never reaches HUF_repeat_valid);
// `next` receives this block's state (confirmed by the caller only if the block is emitted
// compressed).  `work` must hold a LitWork.  Returns the section size written at dst.
// ---------------------------------------------------------------------------------------------
struct HufState {
    uint8_t nbBits[256];  // 0 for symbols the table does not hold
    uint16_t val[256];
    bool check;           // HUF_repeat_check: the table may be reused
};

struct LitWork {
    uint32_t count[256];
    HufNode nodes[2 * 256 + 1];
    uint8_t nbBits[256];
    uint16_t val[256];
    FseCTable fct;
    uint8_t scratch[64];
};

PGN_HD size_t write_raw_literals(uint8_t* dst, const uint8_t* lit, size_t n)
{
    size_t fl = write_rawrle_lit_header(dst, n, kSetBasic);
    for (size_t i = 0; i < n; i++) dst[fl + i] = lit[i];
    return fl + n;
}

// Huffman-encode `n` symbols (1X stream) into dst; returns bytes (end mark included).
PGN_HD size_t huf_encode_1x(uint8_t* dst, const uint8_t* src, size_t n, const uint8_t* nbBits, const uint16_t* val)
{
    BitW bw;
    bw_init(bw, dst);
    for (size_t i = n; i-- > 0;) bw_add(bw, val[src[i]], nbBits[src[i]]);
    return bw_close(bw, dst);
}

// HUF_compress{1,4}X_usingCTable: the streams (and the 4X jump table) at dst; returns their size
PGN_HD size_t huf_encode_streams(uint8_t* dst, const uint8_t* lit, size_t n, bool singleStream, const uint8_t* nbBits,
                                 const uint16_t* val)
{
    if (singleStream) return huf_encode_1x(dst, lit, n, nbBits, val);
    const size_t seg = (n + 3) / 4;
    uint8_t* jt = dst;
    uint8_t* sp = jt + 6;
    for (int k = 0; k < 4; k++) {
        size_t a = seg * (size_t)k, b = (k == 3) ? n : seg * (size_t)(k + 1);
        size_t c = huf_encode_1x(sp, lit + a, b - a, nbBits, val);
        if (k < 3) wr16(jt + 2 * k, (uint32_t)c);
        sp += c;
    }
    return (size_t)(sp - dst);
}

// HUF_estimateCompressedSize
PGN_HD size_t huf_estimate(const uint8_t* nbBits, const uint32_t* count, unsigned maxSym)
{
    size_t bits = 0;
    for (unsigned s = 0; s <= maxSym; s++) bits += (size_t)nbBits[s] * count[s];
    return bits >> 3;
}

PGN_HD size_t compress_literals(uint8_t* dst, const uint8_t* lit, size_t n, LitWork& w, const HufState& prev,
                                HufState& next)
{
    next = prev;  // "Prepare nextEntropy assuming reusing the existing table"
    if (n <= 63) return write_raw_literals(dst, lit, n);
    const size_t minGain = (n >> 6) + 2;
    const size_t lhSize = huf_lit_header_size(n);
    const bool singleStream = n < 256;
    const bool preferRepeat = n <= 1024;  // strategy < ZSTD_lazy
    // HIST_count_wksp
    for (int s = 0; s < 256; s++) w.count[s] = 0;
    for (size_t i = 0; i < n; i++) w.count[lit[i]]++;
    unsigned maxSym = 255;
    while (w.count[maxSym] == 0) maxSym--;
    uint32_t largest = 0;
    for (unsigned s = 0; s <= maxSym; s++) if (w.count[s] > largest) largest = w.count[s];
    if (largest == n) {  // single symbol: RLE literals block
        size_t fl = write_rawrle_lit_header(dst, n, kSetRle);
        dst[fl] = lit[0];
        return fl + 1;
    }
    if (largest <= (n >> 7) + 4) return write_raw_literals(dst, lit, n);
    // HUF_validateCTable: the previous table must code every symbol present
    bool repeat = prev.check;
    if (repeat)
        for (unsigned s = 0; s <= maxSym; s++) repeat = repeat && !(w.count[s] != 0 && prev.nbBits[s] == 0);
    uint8_t* op = dst + lhSize;
    bool useOld = repeat && preferRepeat;
    size_t hSize = 0;
    if (!useOld) {
        unsigned huffLog = huf_optimal_table_log(kHufTableLogDefault, n, maxSym);
        for (int i = 0; i < 2 * 256 + 1; i++) { w.nodes[i].count = 0; w.nodes[i].parent = 0; w.nodes[i].byte = 0; w.nodes[i].nbBits = 0; }
        huf_sort_serial(w.nodes + 1, w.count, maxSym);
        huffLog = huf_build_from_sorted(w.nodes, maxSym, huffLog, w.nbBits, w.val);
        for (unsigned s = maxSym + 1; s < 256; s++) { w.nbBits[s] = 0; w.val[s] = 0; }
        hSize = huf_write_ctable(op, w.nbBits, maxSym, huffLog, w.fct, w.scratch);
        if (hSize == 0) return write_raw_literals(dst, lit, n);  // HUF_writeCTable error -> raw
        if (repeat) {  // is the previous table still the better one?
            const size_t oldSize = huf_estimate(prev.nbBits, w.count, maxSym);
            const size_t newSize = huf_estimate(w.nbBits, w.count, maxSym);
            if (oldSize <= hSize + newSize || hSize + 12 >= n) useOld = true;
        }
        if (!useOld && hSize + 12 >= n) return write_raw_literals(dst, lit, n);
    }
    size_t total;
    if (useOld) {  // HUF_compressCTable_internal with the previous table: no description
        const size_t c = huf_encode_streams(op, lit, n, singleStream, prev.nbBits, prev.val);
        if (c >= n - 1 || c >= n - minGain) return write_raw_literals(dst, lit, n);
        write_huf_lit_header(dst, lhSize, n, c, singleStream, kSetRepeat);
        return lhSize + c;
    }
    const size_t c = huf_encode_streams(op + hSize, lit, n, singleStream, w.nbBits, w.val);
    total = hSize + c;
    if (total >= n - 1) return write_raw_literals(dst, lit, n);        // HUF_compressCTable_internal
    if (total >= n - minGain) return write_raw_literals(dst, lit, n);  // ZSTD_compressLiterals
    write_huf_lit_header(dst, lhSize, n, total, singleStream);
    for (int s = 0; s < 256; s++) { next.nbBits[s] = w.nbBits[s]; next.val[s] = w.val[s]; }
    next.check = true;  // a newly built table: HUF_repeat_check
    return lhSize + total;
}

// ---------------------------------------------------------------------------------------------
// Sequences section (ZSTD_compressSequences_internal, repeat mode none).  Returns bytes written,
// or (size_t)-1 for "emit a raw block" (the <= 1.3.4 decoder workaround).
// ---------------------------------------------------------------------------------------------
struct SeqWork {
    FseCTable ll, of, ml;
    uint8_t tableSymbol[512];
    uint32_t count[kMaxML + 1];
    int16_t norm[kMaxML + 1];
};

PGN_HD size_t build_seq_table(uint8_t* op, FseCTable& ct, unsigned type, uint32_t* count, unsigned max,
                              unsigned lastCode, size_t nbSeq, unsigned fseLog, unsigned defaultNormLog,
                              unsigned defaultMax, int kind, SeqWork& w)
{
    if (type == kSetRle) {
        fse_build_ctable_rle(ct, max);
        op[0] = (uint8_t)lastCode;  // codeTable[0]; all codes are equal
        return 1;
    }
    if (type == kSetBasic) {
        for (unsigned s = 0; s <= defaultMax; s++)
            w.norm[s] = kind == 0 ? ll_default_norm(s) : (kind == 1 ? of_default_norm(s) : ml_default_norm(s));
        fse_build_ctable(ct, w.norm, defaultMax, defaultNormLog, w.tableSymbol);
        return 0;
    }
    // compressed
    size_t nbSeq_1 = nbSeq;
    unsigned tableLog = fse_optimal_table_log(fseLog, nbSeq, max, 2);
    if (count[lastCode] > 1) { count[lastCode]--; nbSeq_1--; }
    if (!fse_normalize(w.norm, tableLog, count, nbSeq_1, max, nbSeq_1 >= 2048)) return (size_t)-2;
    size_t nc = fse_write_ncount(op, w.norm, max, tableLog);
    if (nc == 0) return (size_t)-2;
    fse_build_ctable(ct, w.norm, max, tableLog, w.tableSymbol);
    return nc;
}

// codes: ll/of/ml code per sequence (filled here)
PGN_HD size_t compress_sequences(uint8_t* dst, const Seq* seqs, size_t nbSeq, uint8_t* llC, uint8_t* ofC,
                                 uint8_t* mlC, SeqWork& w)
{
    uint8_t* op = dst;
    if (nbSeq < 128) {
        *op++ = (uint8_t)nbSeq;
    } else if (nbSeq < 0x7F00) {
        op[0] = (uint8_t)((nbSeq >> 8) + 0x80);
        op[1] = (uint8_t)nbSeq;
        op += 2;
    } else {
        op[0] = 0xFF;
        wr16(op + 1, (uint32_t)(nbSeq - 0x7F00));
        op += 3;
    }
    if (nbSeq == 0) return (size_t)(op - dst);
    uint8_t* seqHead = op++;
    for (size_t i = 0; i < nbSeq; i++) {
        llC[i] = (uint8_t)ll_code(seqs[i].litLength);
        ofC[i] = (uint8_t)highbit32(seqs[i].offset);
        mlC[i] = (uint8_t)ml_code(seqs[i].mlBase);
    }
    uint8_t* lastNCount = nullptr;
    unsigned types[3];
    FseCTable* cts[3] = {&w.ll, &w.of, &w.ml};
    const uint8_t* codes[3] = {llC, ofC, mlC};
    const unsigned maxes[3] = {kMaxLL, kMaxOff, kMaxML};
    const unsigned fseLogs[3] = {kLLFSELog, kOffFSELog, kMLFSELog};
    const unsigned normLogs[3] = {kLLDefaultNormLog, kOFDefaultNormLog, kMLDefaultNormLog};
    const unsigned defMax[3] = {kMaxLL, kDefaultMaxOff, kMaxML};
    for (int k = 0; k < 3; k++) {
        // HIST_countFast_wksp
        for (unsigned s = 0; s <= kMaxML; s++) w.count[s] = 0;
        for (size_t i = 0; i < nbSeq; i++) w.count[codes[k][i]]++;
        unsigned max = maxes[k];
        while (max > 0 && w.count[max] == 0) max--;
        uint32_t mostFrequent = 0;
        for (unsigned s = 0; s <= max; s++) if (w.count[s] > mostFrequent) mostFrequent = w.count[s];
        bool defaultAllowed = (k == 1) ? (max <= kDefaultMaxOff) : true;
        types[k] = select_encoding_type(mostFrequent, nbSeq, normLogs[k], defaultAllowed);
        size_t sz = build_seq_table(op, *cts[k], types[k], w.count, max, codes[k][nbSeq - 1], nbSeq, fseLogs[k],
                                    normLogs[k], defMax[k], k, w);
        if (sz == (size_t)-2) return (size_t)-2;
        if (types[k] == kSetCompressed) lastNCount = op;
        op += sz;
    }
    *seqHead = (uint8_t)((types[0] << 6) + (types[1] << 4) + (types[2] << 2));
    // ZSTD_encodeSequences (no long offsets: windowLog <= 17)
    BitW bw;
    bw_init(bw, op);
    FseState sLL, sOF, sML;
    const size_t last = nbSeq - 1;
    fse_init_state2(sML, w.ml, mlC[last]);
    fse_init_state2(sOF, w.of, ofC[last]);
    fse_init_state2(sLL, w.ll, llC[last]);
    bw_add(bw, seqs[last].litLength, ll_bits(llC[last]));
    bw_add(bw, seqs[last].mlBase, ml_bits(mlC[last]));
    bw_add(bw, seqs[last].offset, ofC[last]);
    for (size_t n = nbSeq - 1; n-- > 0;) {
        fse_encode(bw, sOF, w.of, ofC[n]);
        fse_encode(bw, sML, w.ml, mlC[n]);
        fse_encode(bw, sLL, w.ll, llC[n]);
        bw_add(bw, seqs[n].litLength, ll_bits(llC[n]));
        bw_add(bw, seqs[n].mlBase, ml_bits(mlC[n]));
        bw_add(bw, seqs[n].offset, ofC[n]);
    }
    fse_flush(bw, sML, w.ml);
    fse_flush(bw, sOF, w.of);
    fse_flush(bw, sLL, w.ll);
    size_t streamSize = bw_close(bw, op);
    op += streamSize;
    if (lastNCount && (op - lastNCount) < 4) return (size_t)-1;
    return (size_t)(op - dst);
}

// ---------------------------------------------------------------------------------------------
// Blocks + frame (ZSTD_compress_frameChunk / ZSTD_compressBlock_internal, libzstd 1.4.8/1.4.9).
// ---------------------------------------------------------------------------------------------
PGN_HD size_t write_empty_frame(uint8_t* dst)
{
    size_t h = write_frame_header(dst, 0, 10);
    wr24(dst + h, 1u + (kBtRaw << 1));
    return h + 3;
}
PGN_HD size_t write_raw_block_frame(uint8_t* dst, const uint8_t* src, size_t n)
{
    size_t h = write_frame_header(dst, n, 10);
    wr24(dst + h, (uint32_t)(1u + (kBtRaw << 1) + (n << 3)));
    for (size_t i = 0; i < n; i++) dst[h + 3 + i] = src[i];
    return h + 3 + n;
}

struct CompressWork {
    LitWork lit;
    SeqWork seq;
    HufState huf[2];  // confirmed (previous compressed block) and candidate (this block)
};

// ZSTD_isRLE
PGN_HD bool block_is_rle(const uint8_t* p, size_t n)
{
    for (size_t i = 1; i < n; i++)
        if (p[i] != p[0]) return false;
    return true;
}

// One block [start, start + bs) of a frame: its header and body at dst; returns bytes written.
// `rep` / `huf` are the frame's confirmed state, updated when the block is emitted compressed
// (ZSTD_confirmRepcodesAndEntropyTables).  Sequence FSE tables never repeat at level 1 (the
// repeat mode stays "check", never "valid"), so they carry no state.
PGN_HD size_t compress_block(uint8_t* dst, const uint8_t* src, size_t start, size_t bs, bool last, bool first,
                             const Params& p, uint32_t* ht, uint32_t rep[3], Seq* seqs, uint8_t* llC, uint8_t* ofC,
                             uint8_t* mlC, uint8_t* litbuf, CompressWork& w)
{
    const uint8_t* blk = src + start;
    size_t cSize = 0;  // 0: raw block, 1: RLE block, else compressed body size
    if (bs >= 7) {     // MIN_CBLOCK_SIZE + ZSTD_blockHeaderSize + 1: below it no compression is tried
        uint32_t nrep[3] = {rep[0], rep[1], rep[2]};
        size_t lastLL = 0;
        const size_t nbSeq = fast_search_serial(src, start, start + bs, p, ht, nrep, seqs, &lastLL);
        const uint8_t* lit = blk;
        size_t nLit = bs;
        if (nbSeq > 0) {
            size_t pos = start, o = 0;
            for (size_t i = 0; i < nbSeq; i++) {
                for (uint32_t k = 0; k < seqs[i].litLength; k++) litbuf[o++] = src[pos + k];
                pos += seqs[i].litLength + seqs[i].mlBase + 3;
            }
            for (size_t k = 0; k < lastLL; k++) litbuf[o++] = src[pos + k];
            lit = litbuf;
            nLit = o;
        }
        uint8_t* body = dst + 3;
        const size_t litSize = compress_literals(body, lit, nLit, w.lit, w.huf[0], w.huf[1]);
        const size_t seqSize = compress_sequences(body + litSize, seqs, nbSeq, llC, ofC, mlC, w.seq);
        const size_t maxCSize = bs - ((bs >> 6) + 2);
        if (seqSize != (size_t)-1 && seqSize != (size_t)-2 && litSize + seqSize < maxCSize) cSize = litSize + seqSize;
        // a later block of one repeated byte is an RLE block (never the first: decoders <= 1.4.3)
        if (!first && cSize < 25 && block_is_rle(blk, bs)) cSize = 1;
        if (cSize > 1) {  // ZSTD_confirmRepcodesAndEntropyTables
            rep[0] = nrep[0];
            rep[1] = nrep[1];
            rep[2] = nrep[2];
            w.huf[0] = w.huf[1];
        }
    }
    if (cSize == 0) {
        wr24(dst, (uint32_t)((last ? 1u : 0u) + (kBtRaw << 1) + (bs << 3)));
        for (size_t i = 0; i < bs; i++) dst[3 + i] = blk[i];
        return 3 + bs;
    }
    if (cSize == 1) {
        wr24(dst, (uint32_t)((last ? 1u : 0u) + (kBtRle << 1) + (bs << 3)));
        dst[3] = blk[0];
        return 4;
    }
    wr24(dst, (uint32_t)((last ? 1u : 0u) + (kBtCompressed << 1) + (cSize << 3)));
    return 3 + cSize;
}

// Full serial ZSTD_compress(dst, bound, src, n, 1) (blocks of 128 KiB; a window-descriptor frame
// above 2^windowLog = 512 KiB).
// `ht`: 2^15 entries; `seqs`, `llC/ofC/mlC`: kMaxSrc/4 + 2 entries; `litbuf`: kMaxSrc bytes
// (per block); dst capacity >= compress_bound(n).
PGN_HD size_t compress_serial(uint8_t* dst, const uint8_t* src, size_t n, uint32_t* ht, Seq* seqs, uint8_t* llC,
                              uint8_t* ofC, uint8_t* mlC, uint8_t* litbuf, CompressWork& w)
{
    if (n == 0) return write_empty_frame(dst);
    if (n < 7) return write_raw_block_frame(dst, src, n);
    const Params p = level1_params(n);
    for (size_t i = 0; i < ((size_t)1 << p.hashLog); i++) ht[i] = 0;
    uint32_t rep[3] = {1, 4, 8};
    w.huf[0].check = false;
    for (int s = 0; s < 256; s++) { w.huf[0].nbBits[s] = 0; w.huf[0].val[s] = 0; }
    size_t o = write_frame_header(dst, n, p.windowLog);
    for (size_t start = 0; start < n; start += kMaxSrc) {
        const size_t bs = (n - start < kMaxSrc) ? n - start : kMaxSrc;
        o += compress_block(dst + o, src, start, bs, start + bs == n, start == 0, p, ht, rep, seqs, llC, ofC, mlC, litbuf, w);
    }
    return o;
}

}  // namespace z1
}  // namespace pgn
