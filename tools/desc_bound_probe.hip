// desc_bound_probe.hip -- host-only study tool (not part of the product or the tests): for one literal
// stream, the exact size HUF_writeCTable returns against the bracket that the weight histogram and the
// normalised counts give before the weight-FSE chains run (pgn_zenc.h huf_write_ctable_wave, rawFrom).
// Build and run from the repository root (after the oracle is built):
//   hipcc --offload-arch=gfx950 -O2 -fPIC -std=c++17 -Irawnanoporesignalcompression_amd/csrc -Iinclude \
//       -shared -o _ab/libdesc_bound_probe.so tools/desc_bound_probe.hip
//   python tools/desc_bound_probe.py 200
#include <stdlib.h>
#include <string.h>
#define PGN_SELECT_HOST_ONLY
#include "pgn_select.h"
#include "zstd1_dec.h"
#include "zstd1_model.h"
using namespace pgn::z1;

extern "C" int probe(const uint8_t* lit, size_t n, long* out)
{
    // out: 0 path (0 short/raw early, 1 full), 1 n, 2 maxSym, 3 largest, 4 cs, 5 minGain, 6 hSize (returned by write_ctable),
    // 7 hLow (fse form, without +1), 8 hHigh, 9 nh, 10 tableLog, 11 final raw? 12 wtSize
    memset(out, 0, 16 * sizeof(long));
    out[1] = (long)n;
    if (n <= 63) return 0;
    LitWork* w = (LitWork*)calloc(1, sizeof(LitWork));
    for (size_t i = 0; i < n; i++) w->count[lit[i]]++;
    unsigned maxSym = 255;
    while (!w->count[maxSym]) maxSym--;
    uint32_t largest = 0;
    for (unsigned s = 0; s <= maxSym; s++) if (w->count[s] > largest) largest = w->count[s];
    out[2] = maxSym; out[3] = largest;
    const size_t minGain = (n >> 6) + 2;
    out[5] = (long)minGain;
    if (largest == n || largest <= (n >> 7) + 4) { free(w); return 0; }
    unsigned huffLog = huf_optimal_table_log(kHufTableLogDefault, n, maxSym);
    huf_sort_serial(w->nodes + 1, w->count, maxSym);
    huffLog = huf_build_from_sorted(w->nodes, maxSym, huffLog, w->nbBits, w->val);
    // stream sizes
    const bool single = n < 256;
    size_t cs = single ? 0 : 6;
    const size_t seg = (n + 3) / 4;
    for (int k = 0; k < (single ? 1 : 4); k++) {
        size_t a = single ? 0 : seg * k, b = single ? n : (k == 3 ? n : seg * (k + 1));
        size_t bits = 0;
        for (size_t i = a; i < b; i++) bits += w->nbBits[lit[i]];
        cs += (bits + 8) >> 3;
    }
    out[4] = (long)cs;
    out[0] = 1;
    uint8_t hdr[300];
    size_t hSize = huf_write_ctable(hdr, w->nbBits, maxSym, huffLog, w->fct, w->scratch);
    out[6] = (long)hSize;
    // bracket
    uint8_t wt[256];
    uint32_t cnt[13] = {0};
    const unsigned wtSize = maxSym;
    for (unsigned s = 0; s < wtSize; s++) { wt[s] = w->nbBits[s] ? (uint8_t)(huffLog + 1 - w->nbBits[s]) : 0; cnt[wt[s]]++; }
    out[12] = wtSize;
    out[7] = out[8] = -1;
    if (wtSize > 2) {
        unsigned maxW = 12;
        while (!cnt[maxW]) maxW--;
        uint32_t maxCount = 0;
        for (unsigned v = 0; v <= maxW; v++) if (cnt[v] > maxCount) maxCount = cnt[v];
        if (maxCount != wtSize && maxCount > 1) {
            unsigned tl = fse_optimal_table_log(6, wtSize, maxW, 2);
            int16_t norm[13];
            if (fse_normalize(norm, tl, cnt, wtSize, maxW, false)) {
                uint8_t tmp[64];
                size_t nh = fse_write_ncount(tmp, norm, maxW, tl);
                out[9] = (long)nh; out[10] = tl;
                if (nh) {
                    uint32_t c2[13];
                    for (int v = 0; v < 13; v++) c2[v] = cnt[v];
                    c2[wt[wtSize - 1]]--; c2[wt[wtSize - 2]]--;
                    uint32_t lo = 0, hi = 0;
                    for (unsigned v = 0; v <= maxW; v++) {
                        if (!c2[v]) continue;
                        const int nv = norm[v];
                        uint32_t mx, mn;
                        if (nv == 1 || nv == -1) mx = mn = tl;
                        else { mx = tl - highbit32((uint32_t)(nv - 1)); mn = mx - 1; if (!(nv & (nv - 1))) mx = mn; }
                        lo += c2[v] * mn; hi += c2[v] * mx;
                    }
                    out[7] = (long)(nh + ((lo + 2 * tl + 1 + 7) >> 3));
                    out[8] = (long)(nh + ((hi + 2 * tl + 1 + 7) >> 3));
                }
            }
        }
    }
    bool raw = hSize == 0 || hSize + 12 >= n || hSize + cs >= n - minGain;
    out[11] = raw;
    free(w);
    return 1;
}
