"""A zstd frame writer for tests: content bytes plus a recipe become a frame, with a record of what
was emitted.  Written from the format (RFC 8878) and from this project's decoder (zstd1_dec.h): it
writes what a decoder must accept, not what an encoder would choose -- 12-bit Huffman tables, RLE and
repeat sequence tables, non-minimal headers, zero-bit sequences, oversized raw blocks, skippable
frames -- and frames with one named defect.  Pure Python/numpy; tests only.

    frame, rec = build_frame(content, {"blocks": [{"type": "comp", "size": 5000, "lit": {...}, ...}], ...})
    b = Builder(seed); b.comp(seqs=[(ll, ml, off), ...], tail=7); frame, rec, content = b.finish()

Recipe keys (all optional):
  frame:  fcs (0/1/2/4/8 bytes, None = smallest), single (bool), window (descriptor byte), dict_flag
          (0..3, value 0), checksum ("ok" / "bad" / None), fcs_value (a lie), blocks [...]
  block:  type raw / rle / comp, size (content bytes it covers), last (forced flag), and for comp:
    lit:  mode raw / rle / huf / treeless, hform (header bytes: 1,2,3 raw/rle; 3,4,5 huf), streams 1/4,
          L (table log), min_len (shortest code, 1 or 2), desc direct / fse, extra_syms (table symbols
          beyond the content's), defects: stream_delta (+1/-1 symbols in stream 0), jump_past,
          weights (raw weight list written instead of the table's)
    seq:  ll / of / ml table modes predef / rle / fse / repeat, logs (LL, OF, ML accuracy), low (use
          "less than one" counts), form (nbSeq bytes 1/2/3), defects: extra_bits, rle_symbol
          (seq.rep: "prefer" repeat codes where one fits, or "ban" them: a real offset code even for rep0)
    parse: offsets (allowed), min_ml, max_ml, ll0 (force ll == 0 neighbours by splitting matches), every
          (literals between matches), or seqs: an explicit [(ll, ml, offset[, repeat code 1..3])] list.
"""
from __future__ import annotations

import bisect
import struct

import numpy as np

MAGIC = 0xFD2FB528
SKIP_MAGIC = 0x184D2A50

LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
LL_BASE = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384,
                             32768, 65536]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195,
                                16387, 32771, 65539]
LL_DEF = ([4, 3] + [2] * 11 + [1] * 3 + [2] * 9 + [3, 2] + [1] * 5 + [-1] * 4, 6)
OF_DEF = ([1] * 6 + [2] * 3 + [1] * 15 + [-1] * 5, 5)
ML_DEF = ([1, 4, 3] + [2] * 6 + [1] * 37 + [-1] * 7, 6)
MAX_LOG = {"ll": 9, "of": 8, "ml": 9}
MAX_SYM = {"ll": 35, "of": 31, "ml": 52}
DEFAULTS = {"ll": LL_DEF, "of": OF_DEF, "ml": ML_DEF}
assert len(LL_BITS) == len(LL_BASE) == len(LL_DEF[0]) == 36 and len(ML_BITS) == len(ML_BASE) == len(ML_DEF[0]) == 53
assert all(sum(abs(c) for c in n) == 1 << lg for n, lg in DEFAULTS.values())


def ll_code(v):
    return bisect.bisect_right(LL_BASE, v) - 1


def ml_code(v):
    return bisect.bisect_right(ML_BASE, v) - 1


# ------------------------------------------------------------------------------------------------
# bits
# ------------------------------------------------------------------------------------------------
class BitW:
    """Little-endian bit accumulator; whole bytes leave the big integer every 1024 bits."""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def add(self, v, nb):
        assert 0 <= v < (1 << nb) or nb == 0 and v == 0, (v, nb)
        self.acc |= v << self.n
        self.n += nb
        if self.n >= 1024:
            k = self.n >> 3
            self.out += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k
            self.n -= 8 * k

    def close(self, mark=True):
        """mark: the end bit of a backward stream (the decoder starts below the highest set bit)."""
        if mark:
            self.add(1, 1)
        self.out += self.acc.to_bytes((self.n + 7) >> 3, "little")
        self.acc = self.n = 0
        return bytes(self.out)


def xxh64(data: bytes, seed: int = 0) -> int:
    M = (1 << 64) - 1
    P1, P2, P3, P4, P5 = (11400714785074694791, 14029467366897019727, 1609587929392839161, 9650029242287828579,
                          2870177450012600261)

    def rotl(x, r):
        return ((x << r) | (x >> (64 - r))) & M

    def rnd(acc, inp):
        return (rotl((acc + inp * P2) & M, 31) * P1) & M

    n, p = len(data), 0
    if n >= 32:
        v = [(seed + P1 + P2) & M, (seed + P2) & M, seed, (seed - P1) & M]
        while p + 32 <= n:
            w = struct.unpack_from("<4Q", data, p)
            v = [rnd(v[i], w[i]) for i in range(4)]
            p += 32
        h = (rotl(v[0], 1) + rotl(v[1], 7) + rotl(v[2], 12) + rotl(v[3], 18)) & M
        for x in v:
            h = ((h ^ rnd(0, x)) * P1 + P4) & M
    else:
        h = (seed + P5) & M
    h = (h + n) & M
    while p + 8 <= n:
        h = (rotl(h ^ rnd(0, struct.unpack_from("<Q", data, p)[0]), 27) * P1 + P4) & M
        p += 8
    if p + 4 <= n:
        h = (rotl(h ^ (struct.unpack_from("<I", data, p)[0] * P1) & M, 23) * P2 + P3) & M
        p += 4
    while p < n:
        h = (rotl(h ^ (data[p] * P5) & M, 11) * P1) & M
        p += 1
    h ^= h >> 33
    h = (h * P2) & M
    h ^= h >> 29
    h = (h * P3) & M
    return h ^ (h >> 32)


# ------------------------------------------------------------------------------------------------
# FSE
# ------------------------------------------------------------------------------------------------
class FseTable:
    """The decode table of normalised counts (the decoder's own construction), indexed for encoding:
    to leave the decoder in state T after symbol s, the state before is the one entry of s whose
    range [newState, newState + 2^nbBits) holds T, and the bits are T - newState."""

    def __init__(self, norm, log, rle_symbol=None):
        self.norm, self.log = (list(norm) if norm is not None else None), log
        if rle_symbol is not None:
            self.log = 0
            self.sym, self.nb, self.new = [rle_symbol], [0], [0]
        else:
            size = 1 << log
            assert sum(abs(c) for c in norm) == size, (norm, log)
            sym, high, nxt = [0] * size, size - 1, {}
            for s, c in enumerate(norm):
                if c == -1:
                    sym[high] = s
                    high -= 1
                    nxt[s] = 1
                elif c > 0:
                    nxt[s] = c
            step, pos = (size >> 1) + (size >> 3) + 3, 0
            for s, c in enumerate(norm):
                for _ in range(max(c, 0)):
                    sym[pos] = s
                    pos = (pos + step) & (size - 1)
                    while pos > high:
                        pos = (pos + step) & (size - 1)
            assert pos == 0
            self.sym, self.nb, self.new = sym, [0] * size, [0] * size
            for u in range(size):
                x = nxt[sym[u]]
                nxt[sym[u]] += 1
                self.nb[u] = log - (x.bit_length() - 1)
                self.new[u] = (x << self.nb[u]) - size
        self.by_sym = {}
        for u in sorted(range(len(self.sym)), key=lambda u: self.new[u]):
            st, us = self.by_sym.setdefault(self.sym[u], ([], []))
            st.append(self.new[u])
            us.append(u)

    def has(self, s):
        return s in self.by_sym

    def first(self, s, want_bits=False):
        """A free starting state for s (with the most update bits when want_bits)."""
        us = self.by_sym[s][1]
        return max(us, key=lambda u: self.nb[u]) if want_bits else us[0]

    def step(self, s, target):
        """(state before, bits, nbBits) so that decoding s there and reading the bits gives target."""
        st, us = self.by_sym[s]
        u = us[bisect.bisect_right(st, target) - 1]
        return u, target - self.new[u], self.nb[u]


def write_ncount(norm, log) -> bytes:
    """The count description FSE_readNCount parses (zero-run flags and "less than one" included)."""
    w = BitW()
    w.add(log - 5, 4)
    remaining, threshold, nb = (1 << log) + 1, 1 << log, log + 1
    s, prev0 = 0, False
    while remaining > 1:
        if prev0:
            start = s
            while norm[s] == 0:
                s += 1
            while s >= start + 24:
                start += 24
                w.add(0xFFFF, 16)
            while s >= start + 3:
                start += 3
                w.add(3, 2)
            w.add(s - start, 2)
        c = norm[s]
        s += 1
        mx = (2 * threshold - 1) - remaining
        remaining -= abs(c)
        c += 1
        if c >= threshold:
            c += mx
        w.add(c, nb - 1 if c < mx else nb)
        prev0 = c == 1
        while remaining < threshold:
            nb -= 1
            threshold >>= 1
    assert remaining == 1
    return w.close(mark=False)


def normalize(hist: dict, log: int, max_sym: int, low: bool = False):
    """Normalised counts summing to 2^log over the symbols of hist (each >= 1 slot); low: symbols that
    would round to one slot are written as "less than one" (-1).  A lone symbol gets a -1 partner, as a
    one-symbol distribution has no description."""
    hist = dict(hist)
    if len(hist) == 1:
        s = next(iter(hist))
        hist[s + 1 if s < max_sym else s - 1] = 0
    size, total = 1 << log, max(sum(hist.values()), 1)
    assert len(hist) <= size
    norm = [0] * (max(hist) + 1)
    for s, c in hist.items():
        v = max(1, c * size // total)
        norm[s] = -1 if v == 1 and (low or c == 0) else v
    diff = size - sum(abs(c) for c in norm)
    while diff:
        s = max(range(len(norm)), key=lambda k: norm[k])
        d = diff if diff > 0 else -min(-diff, norm[s] - 1)
        assert d, "cannot normalise"
        norm[s] += d
        diff -= d
    return norm


# ------------------------------------------------------------------------------------------------
# Huffman
# ------------------------------------------------------------------------------------------------
def comb_lengths(k: int, L: int, min_len: int = 1):
    """k code lengths, Kraft-complete, longest L, shortest min_len: a comb 1,2,..,L,L (or 2,2,2,3,..,L,L)
    whose longest splittable leaf is split until there are k."""
    if min_len == 1:
        ls = list(range(1, L + 1)) + [L]
    else:
        assert min_len == 2 and L >= 2
        ls = [2, 2, 2, 2] if L == 2 else [2, 2, 2] + list(range(3, L + 1)) + [L]
    assert len(ls) <= k <= (1 << L), (k, L, len(ls))
    while len(ls) < k:
        keep = 1 if min_len == 1 else 3  # leaves of the shortest length that stay
        cand = [i for i in range(keep, len(ls)) if ls[i] < L]
        if not cand:
            cand = [i for i in range(len(ls)) if ls[i] < L]
        i = max(cand, key=lambda j: ls[j])
        ls[i] += 1
        ls.append(ls[i])
    ls.sort()
    assert sum(1 << (L - l) for l in ls) == 1 << L
    return ls


class HufTable:
    def __init__(self, weights):
        """weights[s] for s in 0..maxSym (0 = absent), Kraft-complete."""
        self.weights = list(weights)
        tot = sum((1 << w) >> 1 for w in weights)
        self.log = tot.bit_length() - 1
        assert tot == 1 << self.log, "incomplete code"
        self.max_weight = max(weights)
        self.code, nxt = {}, 0
        for w in range(1, self.log + 1):  # the decoder's fill: ascending weight, then symbol
            for s, ws in enumerate(weights):
                if ws == w:
                    self.code[s] = (nxt >> (w - 1), self.log + 1 - w)
                    nxt += 1 << (w - 1)

    @staticmethod
    def for_content(lits: bytes, L: int, min_len: int = 1, extra_syms: int = 0, span: int | None = None,
                    cover: int = 0):
        """A table of log L holding every symbol of lits: frequent symbols get short codes; symbols the
        content lacks are added (from the low end of [0, span)) when the comb needs more leaves."""
        cnt = np.bincount(np.frombuffer(lits, np.uint8), minlength=256)
        present = sorted({int(s) for s in np.nonzero(cnt)[0]} | set(range(cover)))  # cover: for later treeless blocks
        need = max(len(present) + extra_syms, L + 1 if min_len == 1 else (4 if L == 2 else L + 2), 2)
        pool = [s for s in range(span if span else 256) if s not in present]
        syms = present + pool[:max(0, need - len(present))]
        assert len(syms) == need, "alphabet too small for this table log"
        ls = comb_lengths(len(syms), L, min_len)
        syms.sort(key=lambda s: (-int(cnt[s]), s))
        weights = [0] * (max(syms) + 1)
        for s, l in zip(syms, ls):
            weights[s] = L + 1 - l
        return HufTable(weights)

    def describe(self, form: str, weights=None):
        """The table description; weights: a raw list to write instead (defect frames).  The last
        symbol's weight is implied and not written."""
        ws = list(self.weights[:-1]) if weights is None else list(weights)
        if form == "direct":
            assert 1 <= len(ws) <= 128
            b = bytearray([127 + len(ws)])
            for i in range(0, len(ws), 2):
                b.append(ws[i] << 4 | (ws[i + 1] if i + 1 < len(ws) else 0))
            return bytes(b)
        assert form == "fse" and len(ws) >= 2
        hist = {}
        for x in ws:
            hist[x] = hist.get(x, 0) + 1
        log = 6 if len(hist) > 8 or len(ws) > 40 else 5
        norm = normalize(hist, log, 12)
        t = FseTable(norm, log)
        # two interleaved states; the last two weights are the states the stream ends in, and the
        # update after the last-but-one must run past the stream's start (the decoder's stop)
        n = len(ws)
        cur = [None, None]
        cur[(n - 1) & 1] = t.first(ws[n - 1])
        cur[(n - 2) & 1] = t.first(ws[n - 2], want_bits=True)
        assert t.nb[cur[(n - 2) & 1]] > 0
        w = BitW()
        for i in range(n - 3, -1, -1):
            u, bits, nb = t.step(ws[i], cur[i & 1])
            w.add(bits, nb)
            cur[i & 1] = u
        w.add(cur[1], log)
        w.add(cur[0], log)
        body = write_ncount(norm, log) + w.close()
        assert len(body) < 128, "weights do not fit an FSE description"
        return bytes([len(body)]) + body

    def encode(self, syms: bytes) -> bytes:
        w = BitW()
        code = self.code
        for s in reversed(syms):
            c, nb = code[s]
            w.add(c, nb)
        return w.close()


# ------------------------------------------------------------------------------------------------
# literals and sequences sections
# ------------------------------------------------------------------------------------------------
def _lit_header_plain(kind, size, hform):
    if hform is None:
        hform = 1 if size < 32 else (2 if size < 4096 else 3)
    if hform == 1:
        assert size < 32
        return bytes([kind | size << 3])
    if hform == 2:
        assert size < 4096
        return (kind | 1 << 2 | size << 4).to_bytes(2, "little")
    assert hform == 3 and size < (1 << 20)
    return (kind | 3 << 2 | size << 4).to_bytes(3, "little")


def encode_literals(lits: bytes, r: dict, state: dict, rec: dict) -> bytes:
    mode = r.get("mode", "raw")
    rec["lit_mode"], rec["lit_size"] = mode, len(lits)
    if mode in ("raw", "rle"):
        h = _lit_header_plain(0 if mode == "raw" else 1, len(lits), r.get("hform"))
        rec["lit_hform"] = len(h)
        if mode == "raw":
            return h + lits
        assert len(set(lits)) <= 1
        return h + bytes([lits[0] if lits else r.get("byte", 0)])
    streams = r.get("streams", 4)
    if mode == "huf":
        t = r.get("table") or HufTable.for_content(lits, r["L"], r.get("min_len", 1), r.get("extra_syms", 0),
                                                   r.get("span"), r.get("cover", 0))
        desc = t.describe(r.get("desc", "direct"), r.get("weights"))
        state["huf"] = t
        rec.update(huf_log=t.log, huf_max_weight=t.max_weight, huf_desc=r.get("desc", "direct"),
                   huf_nweights=len(t.weights) - 1, huf_desc_len=len(desc))
    else:
        assert mode == "treeless"
        t, desc = r.get("table") or state.get("huf"), b""
        assert t is not None or r.get("no_table"), "treeless literals need an earlier table"
        if t is None:  # defect: no previous table -- any bytes will do for the streams
            t = HufTable([1, 1])
            lits = bytes(len(lits))
        rec.update(huf_log=t.log, huf_max_weight=t.max_weight)
    n = len(lits)
    if streams == 1:
        k = n + r.get("stream_delta", 0)
        body = t.encode((lits + lits[-1:])[:k])
        rec["huf_stream_syms"] = [n]
    else:
        seg = (n + 3) // 4
        if r.get("overhang"):  # sizes 1, 2, 5: three full streams already pass the end, the fourth is empty
            assert 3 * seg > n
            parts = [lits[0:seg], lits[seg:2 * seg], (lits[2 * seg:] + lits[:seg])[:seg], b""]
        else:
            assert 3 * seg <= n, "four streams cannot hold this size"
            parts = [lits[0:seg], lits[seg:2 * seg], lits[2 * seg:3 * seg], lits[3 * seg:]]
        if r.get("stream_delta"):
            parts[0] = (parts[0] + parts[0][-1:])[:seg + r["stream_delta"]]
        enc = [t.encode(p) for p in parts]
        jt = [len(e) for e in enc[:3]]
        if r.get("jump_past"):
            jt[2] += len(enc[3]) + 7
        assert max(jt) < 65536
        body = struct.pack("<3H", *jt) + b"".join(enc)
        rec["huf_stream_syms"] = [len(p) for p in parts]
        rec["huf_jump_off"] = len(desc)
    comp = rec["huf_comp"] = len(desc) + len(body)
    hform = r.get("hform")
    if hform is None:
        hform = 3 if n < 1024 and comp < 1024 else (4 if n < 16384 and comp < 16384 else 5)
    wbits = {3: 10, 4: 14, 5: 18}[hform]
    assert n < (1 << wbits) and comp < (1 << wbits), (n, comp, hform)
    assert streams == 4 or hform == 3 or r.get("_measure"), "one stream has only the 3-byte header"
    sf = (0 if streams == 1 else 1) if hform == 3 else hform - 2
    kind = 2 if mode == "huf" else 3
    h = (kind | sf << 2 | n << 4 | comp << (4 + wbits)).to_bytes(hform, "little")
    rec.update(lit_hform=hform, huf_streams=streams, huf_desc_off=hform)
    return h + desc + body


def ofv_apply(rep, ofv, ll):
    """The decoder's repeat-offset rule: (offset, new history) of offset value ofv after ll literals."""
    r0, r1, r2 = rep
    if ofv > 3:
        return ofv - 3, [ofv - 3, r0, r1]
    idx = ofv - 1 + (1 if ll == 0 else 0)
    if idx == 0:
        return r0, [r0, r1, r2]
    off = (r0 - 1 if idx == 3 else (r1 if idx == 1 else r2)) or 1
    return off, ([off, r0, r2] if idx == 1 else [off, r0, r1])


def choose_ofv(rep, off, ll, policy):
    """Offset value for a real offset: policy "prefer" repeat codes when one fits, "ban" them (a real
    offset code even for rep0), or a forced value 1..3 (asserted to give off)."""
    if policy in (1, 2, 3):
        assert ofv_apply(rep, policy, ll)[0] == off, (rep, off, ll, policy)
        return policy
    if policy == "prefer":
        for v in (1, 2, 3):
            if ofv_apply(rep, v, ll)[0] == off:
                return v
    return off + 3


def encode_sequences(seqs, r: dict, state: dict, rec: dict) -> bytes:
    """seqs: [(ll, ml, offset)] or [(ll, ml, offset, policy)]; state carries rep history and tables."""
    n = len(seqs)
    form = r.get("form")
    if form is None:
        form = 1 if n < 128 else (2 if n < 0x7F00 else 3)
    if form == 1:
        assert n < 128
        out = bytearray([n])
    elif form == 2:
        assert n < 0x7F00
        out = bytearray([128 + (n >> 8), n & 255])
    else:
        assert 0x7F00 <= n <= 0x7F00 + 0xFFFF
        out = bytearray([255]) + (n - 0x7F00).to_bytes(2, "little")
    rec.update(nbseq=n, nbseq_form=form)
    if n == 0:
        return bytes(out)
    rep = state["rep"]
    codes, extra, ofvs = [], [], []
    for q in seqs:
        ll, ml, off = q[:3]
        ofv = choose_ofv(rep, off, ll, q[3] if len(q) > 3 else r.get("rep", "prefer"))
        got, rep = ofv_apply(rep, ofv, ll)
        assert got == off
        lc, mc, oc = ll_code(ll), ml_code(ml), ofv.bit_length() - 1
        codes.append((lc, oc, mc))
        extra.append((ll - LL_BASE[lc], ofv - (1 << oc), ml - ML_BASE[mc]))
        ofvs.append(ofv)
    state["rep"] = rep
    rec.update(ofvs=ofvs if n <= 4096 else None, ll0_rep=[v for v, q in zip(ofvs, seqs) if v <= 3 and q[0] == 0],
               llpos_rep=[v for v, q in zip(ofvs, seqs) if v <= 3 and q[0] > 0],
               max_codes=tuple(max(c[k] for c in codes) for k in range(3)))
    tabs, modes, descs = {}, {}, b""
    for k, name in enumerate(("ll", "of", "ml")):
        mode = r.get(name, "predef")
        hist = {}
        for c in codes:
            hist[c[k]] = hist.get(c[k], 0) + 1
        if mode == "try_rle":  # random recipes: the mode when the block allows it
            mode = "rle" if len(hist) == 1 else "fse"
        elif mode == "try_repeat":
            prev = state["tabs"].get(name)
            mode = "repeat" if prev is not None and all(prev.has(s) for s in hist) else "fse"
        if mode == "predef":
            t = FseTable(*DEFAULTS[name])
        elif mode == "rle":
            sym = r.get("rle_symbol", {}).get(name)
            assert len(hist) == 1 or sym is not None, f"{name}: RLE mode needs one code, has {sorted(hist)}"
            t = FseTable(None, 0, rle_symbol=next(iter(hist)))
            descs += bytes([next(iter(hist)) if sym is None else sym])
        elif mode == "fse":
            log = r.get("logs", {}).get(name, 6)
            while (1 << log) < len(hist) + 1:
                log += 1
            assert log <= MAX_LOG[name]
            for s in r.get("ghosts", {}).get(name, []):  # unused symbols with a "less than one" count
                hist.setdefault(s, 0)
            norm = normalize(hist, log, MAX_SYM[name], r.get("low", False))
            t = FseTable(norm, log)
            d = write_ncount(norm, log)
            descs += d
            rec.setdefault("fse_desc", {})[name] = dict(log=log, low=norm.count(-1), zero_runs=_zero_runs(norm),
                                                        bytes=len(d))
        else:
            assert mode == "repeat"
            t = state["tabs"].get(name)
            assert t is not None or r.get("no_table"), f"{name}: repeat mode needs an earlier table"
            if t is None:
                t = FseTable(*DEFAULTS[name])
        assert all(t.has(s) for s in hist), f"{name}: table lacks a code of {sorted(hist)}"
        tabs[name], modes[name] = t, mode
    state["tabs"] = tabs
    rec["seq_modes"] = (modes["ll"], modes["of"], modes["ml"])
    out.append({"predef": 0, "rle": 1, "fse": 2, "repeat": 3}[modes["ll"]] << 6 |
               {"predef": 0, "rle": 1, "fse": 2, "repeat": 3}[modes["of"]] << 4 |
               {"predef": 0, "rle": 1, "fse": 2, "repeat": 3}[modes["ml"]] << 2)
    out += descs
    tl, to, tm = tabs["ll"], tabs["of"], tabs["ml"]
    w = BitW()
    lc, oc, mc = codes[-1]
    sl, so, sm = tl.first(lc), to.first(oc), tm.first(mc)
    # libzstd 1.4.x updates the states after the last sequence as well: these bits may be left over
    rec["end_slack"] = tl.nb[sl] + to.nb[so] + tm.nb[sm]
    xb = r.get("extra_bits", 0)  # bits the decoder never needs, below the last sequence's
    if xb:
        w.add(0, rec["end_slack"] + xb if r.get("extra_over_slack") else xb)
    for i in range(n - 1, -1, -1):
        lc, oc, mc = codes[i]
        if i != n - 1:  # the update after sequence i, read LL, ML, OF: written OF, ML, LL
            so, b, nb = to.step(oc, so)
            w.add(b, nb)
            sm, b, nb = tm.step(mc, sm)
            w.add(b, nb)
            sl, b, nb = tl.step(lc, sl)
            w.add(b, nb)
        el, eo, em = extra[i]  # read OF, ML, LL: written LL, ML, OF
        w.add(el, LL_BITS[lc])
        w.add(em, ML_BITS[mc])
        w.add(eo, oc)
    w.add(sm, tm.log)
    w.add(so, to.log)
    w.add(sl, tl.log)
    bs = w.close()[r.get("cut_bytes", 0):]  # defect: the stream's first bytes (its last bits) missing
    rec["seq_bits_len"] = len(bs)
    return bytes(out) + bs


def _zero_runs(norm):
    runs, k = [], 0
    for c in norm:
        if c == 0:
            k += 1
        elif k:
            runs.append(k)
            k = 0
    return runs


# ------------------------------------------------------------------------------------------------
# content -> sequences
# ------------------------------------------------------------------------------------------------
def parse(content: bytes, start: int, end: int, p: dict):
    """Greedy parse of content[start:end) into [(ll, ml, offset)] + trailing literal count.  Matches
    may reach back to the frame start (content[0]).  p: offsets (allowed, in order of preference;
    default 1..8 and powers of two), min_ml, max_ml, ll0 (split every match so that its second half
    follows with ll == 0), every (take a match only each `every` bytes, leaving literals)."""
    a = np.frombuffer(content, np.uint8)
    offsets = p.get("offsets") or [1, 2, 3, 4, 5, 6, 7, 8, 16, 32, 64, 128, 256, 1024]
    min_ml, max_ml = max(3, p.get("min_ml", 3)), min(p.get("max_ml", 131074), 131074)
    runs = {}
    for o in offsets:
        if o >= end:
            continue
        eq = np.zeros(end + 1, np.int64)
        eq[o:end] = a[o:end] == a[0:end - o]
        # run[i] = number of consecutive equal positions from i
        z = np.nonzero(eq == 0)[0]
        nxt = z[np.searchsorted(z, np.arange(end + 1))]
        runs[o] = nxt - np.arange(end + 1)
    seqs, i, lit0 = [], start, start
    gap = p.get("every", 0)
    while i < end:
        best = None
        if i - lit0 >= gap or not seqs:
            for o, run in runs.items():
                if o <= i and run[i] >= min_ml:
                    best = (o, int(min(run[i], max_ml, end - i)))
                    break
        if best is None or best[1] < min_ml:
            i += 1
            continue
        o, ml = best
        if p.get("ll0") and ml >= 2 * min_ml:
            h = ml // 2
            seqs.append((i - lit0, h, o))
            seqs.append((0, ml - h, o))
        else:
            seqs.append((i - lit0, ml, o))
        i += ml
        lit0 = i
    return seqs, end - lit0


# ------------------------------------------------------------------------------------------------
# blocks and frames
# ------------------------------------------------------------------------------------------------
def new_state():
    return {"rep": [1, 4, 8], "huf": None, "tabs": {}}


def encode_block(content: bytes, pos: int, b: dict, state: dict, last: bool):
    """One block covering content[pos, pos + size): (bytes with the 3-byte header, record)."""
    size, typ = b["size"], b.get("type", "raw")
    rec = {"type": typ, "size": size, "pos": pos}
    chunk = content[pos:pos + size]
    if typ == "raw":
        body, bsize = chunk, size
    elif typ == "rle":
        assert len(set(chunk)) <= 1
        body, bsize = bytes([chunk[0] if chunk else b.get("byte", 0)]), size
    elif typ == "reserved":
        body, bsize = chunk, size
    else:
        if "seqs" in b:
            seqs = list(b["seqs"])
            tail = size - sum(q[0] + q[1] for q in seqs)
        else:
            seqs, tail = parse(content, pos, pos + size, b.get("parse", {})) if b.get("parse") is not None else ([], size)
        assert tail >= 0
        lits = block_literals(content, pos, size, seqs)
        rec["seqs"] = seqs if len(seqs) <= 4096 else None
        lit_r = dict(b.get("lit", {}))
        lit_extra = lit_r.pop("phantom", 0)  # defect: a literal length past the literals (drop bytes)
        lsec = encode_literals(bytes(lits[:len(lits) - lit_extra]), lit_r, state, rec)
        body = lsec + encode_sequences(seqs, b.get("seq", {}), state, rec)
        bsize = len(body)
        rec["lit_off"] = 3
        rec["seq_off"] = 3 + len(lsec)
    if "pad_to" in b:  # a compressed block of an exact size cannot be padded: the recipe sizes it
        assert len(body) == b["pad_to"], (len(body), b["pad_to"])
    lastf = b.get("last", last)
    code = {"raw": 0, "rle": 1, "comp": 2, "reserved": 3}[typ]
    assert bsize < (1 << 21)
    rec.update(bsize=bsize, last=bool(lastf))
    return (int(lastf) | code << 1 | bsize << 3).to_bytes(3, "little") + body, rec


def skippable(n: int, nibble: int = 0, fill: int = 0xA5, truncate: int = 0) -> bytes:
    f = struct.pack("<II", SKIP_MAGIC | nibble, n) + bytes([fill]) * n
    return f[:len(f) - truncate]


def build_frame(content: bytes, recipe: dict):
    """One frame for content: (bytes, record).  record: header fields, blocks [...], and byte offsets
    of each block inside the frame (rec['blocks'][i]['off'])."""
    content = bytes(content)
    blocks = recipe.get("blocks")
    if blocks is None:
        blocks = [{"type": "raw", "size": len(content)}]
    single = recipe.get("single", True)
    fcs = recipe.get("fcs", None)
    n = recipe.get("fcs_value", len(content))
    if fcs is None:
        fcs = (1 if n < 256 and single else (2 if 256 <= n < 65536 + 256 else (4 if n < (1 << 32) else 8)))
    assert fcs in (0, 1, 2, 4, 8)
    assert not (fcs == 0 and single), "no content size needs a window descriptor"
    assert not (fcs == 1 and not single), "the 1-byte size exists only in single-segment frames"
    flag = {0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[fcs]
    dflag = recipe.get("dict_flag", 0)
    chk = recipe.get("checksum")
    out = bytearray(struct.pack("<I", MAGIC))
    out.append(flag << 6 | int(single) << 5 | (4 if chk else 0) | dflag)
    if not single:
        out.append(recipe.get("window", 0x00))  # 1 KiB unless told otherwise
    out += bytes([0, 1, 2, 4][dflag])
    if fcs == 2:
        assert 256 <= n < 65536 + 256
        out += struct.pack("<H", n - 256)
    elif fcs:
        out += n.to_bytes(fcs, "little")
    rec = {"fcs_bytes": fcs, "single": single, "dict_flag": dflag, "checksum": chk, "header_len": len(out),
           "blocks": []}
    state, pos = new_state(), 0
    for i, b in enumerate(blocks):
        data, br = encode_block(content, pos, b, state, i == len(blocks) - 1)
        br["off"] = len(out)
        out += data
        rec["blocks"].append(br)
        pos += b["size"]
    assert pos == len(content) or recipe.get("partial"), (pos, len(content))
    if chk:
        h = xxh64(content) & 0xFFFFFFFF
        out += struct.pack("<I", h if chk == "ok" else h ^ 0x00010000)
    return bytes(out), rec


class Builder:
    """Content grown from operations: literals come from a seeded generator, matches copy what is
    already there, so a block's sequence list is exactly what was asked for."""

    def __init__(self, seed: int = 0, alphabet: int = 200):
        self.rng = np.random.default_rng(seed)
        self.alphabet = alphabet
        self.content = bytearray()
        self.blocks = []
        self.rep = [1, 4, 8]

    def _lits(self, n, const=None):
        if const is not None:
            return bytes([const]) * n
        # skewed, so that Huffman tables of any log have something to shorten
        v = np.minimum(self.rng.geometric(0.08, n) - 1, self.alphabet - 1)
        return v.astype(np.uint8).tobytes()

    def raw(self, n, **kw):
        self.content += self._lits(n)
        self.blocks.append(dict(type="raw", size=n, **kw))
        return self

    def rle(self, n, byte=7, **kw):
        self.content += bytes([byte]) * n
        self.blocks.append(dict(type="rle", size=n, byte=byte, **kw))
        return self

    def comp(self, seqs=(), tail=0, lit=None, seq=None, const=None, before_start=False, **kw):
        """seqs: (ll, ml, offset[, policy]); offsets count back from the current end (frame start = 0).
        offset None with a policy 1..3: whatever that repeat code means at this point.  before_start:
        an offset beyond the frame start is let through (a defect frame; the bytes are zeros)."""
        start, out = len(self.content), []
        for q in seqs:
            ll, ml, off = q[:3]
            pol = q[3] if len(q) > 3 else (seq or {}).get("rep", "prefer")
            self.content += self._lits(ll, const)
            if off is None:
                off = ofv_apply(self.rep, pol, ll)[0]
            self.rep = ofv_apply(self.rep, choose_ofv(self.rep, off, ll, pol), ll)[1]
            assert 0 < off <= len(self.content) or before_start, (off, len(self.content))
            if off > len(self.content):
                self.content += bytes(ml)
            else:
                fast_copy(self.content, ml, off)
            out.append((ll, ml, off, pol))
        self.content += self._lits(tail, const)
        self.blocks.append(dict(type="comp", size=len(self.content) - start, seqs=out, lit=lit or {},
                                seq=seq or {}, **kw))
        return self

    def finish(self, **frame):
        f, rec = build_frame(bytes(self.content), dict(frame, blocks=self.blocks))
        return f, rec, bytes(self.content)


def fast_copy(content: bytearray, ml: int, off: int):
    """content += ml bytes copied from off back (overlap repeats), without a Python loop per byte."""
    src = bytes(content[-off:])
    reps = ml // off + 1
    content += (src * reps)[:ml]


def block_literals(content: bytes, pos: int, size: int, seqs) -> bytes:
    lits, p = bytearray(), pos
    for q in seqs:
        lits += content[p:p + q[0]]
        p += q[0] + q[1]
    return bytes(lits + content[p:pos + size])


def random_recipe(rng, content: bytes) -> dict:
    """A valid recipe for content: random block cuts and types, parses, literal modes, Huffman table
    logs and description forms, sequence table modes and logs, header forms and frame header fields.
    Every choice is made among what the content can carry (a table log needs enough leaves, a direct
    description symbols up to 128, RLE one value), so every recipe builds and must decode."""
    n = len(content)
    blocks, pos = [], 0
    huf, tabs = None, set()
    while pos < n or not blocks:
        size = min(n - pos, int(rng.choice([rng.integers(0, 40), rng.integers(0, 3000), rng.integers(0, 20001)])))
        chunk = content[pos:pos + size]
        kind = str(rng.choice(["raw", "rle", "comp", "comp", "comp"]))
        if kind == "rle" and len(set(chunk)) > 1:
            kind = "comp"
        b = {"type": kind, "size": size}
        if kind == "comp":
            p = {"min_ml": int(rng.choice([3, 4, 8])), "max_ml": int(rng.choice([5, 70, 131074])),
                 "ll0": bool(rng.random() < 0.3), "every": int(rng.choice([0, 0, 5, 40]))}
            seqs, _ = parse(content, pos, pos + size, p) if rng.random() < 0.8 else ([], size)
            b["seqs"] = seqs
            lits = block_literals(content, pos, size, seqs)
            nl, nsym = len(lits), len(set(lits))
            choices = ["raw"] + (["rle"] if nsym <= 1 else []) + (["huf", "huf"] if nl >= 1 else [])
            if huf is not None and nl >= 1 and all(s in huf.code for s in set(lits)):
                choices.append("treeless")
            lit = {"mode": str(rng.choice(choices))}
            if lit["mode"] in ("raw", "rle"):
                lit["hform"] = int(rng.integers(1 if nl < 32 else (2 if nl < 4096 else 3), 4))
            else:
                streams = int(rng.choice([1, 4]))
                if 3 * ((nl + 3) // 4) > nl or nl < 4:
                    streams = 1
                if lit["mode"] == "huf":
                    L = int(rng.integers(max(1, (max(nsym, 2) - 1).bit_length()), 13))
                    desc = str(rng.choice(["direct", "fse"]))
                    t = None
                    for form, span in ((desc, 129), ("fse", 256), ("direct", 129), ("fse", 129)):
                        try:
                            t = HufTable.for_content(lits, L, 2 if L == 12 else int(rng.choice([1, 1, 2])) if L >= 3 else 1,
                                                     span=span)
                            t.describe(form)
                            lit.update(table=t, desc=form)
                            break
                        except AssertionError:
                            t = None
                    if t is None:
                        lit = {"mode": "raw"}
                else:
                    lit["table"] = huf
                if lit["mode"] != "raw":
                    # measure, then pick a stream count and a header form that hold the sizes
                    m = {}
                    if streams == 1:
                        encode_literals(lits, dict(lit, streams=1, hform=5, _measure=True), new_state(), m)
                        if nl >= 1024 or m["huf_comp"] >= 1024:
                            streams = 4
                    if streams == 4 and 3 * ((nl + 3) // 4) > nl:
                        lit = {"mode": "raw"}
                    else:
                        if streams == 4:
                            encode_literals(lits, dict(lit, streams=4, hform=5), new_state(), m)
                        comp = m["huf_comp"]
                        lit["streams"] = streams
                        lo = 3 if nl < 1024 and comp < 1024 else (4 if nl < 16384 and comp < 16384 else 5)
                        lit["hform"] = 3 if streams == 1 else int(rng.integers(lo, 6))
            b["lit"] = lit
            if lit["mode"] == "huf":
                huf = lit["table"]
            if seqs:
                sq = {"rep": str(rng.choice(["prefer", "ban"])), "low": bool(rng.random() < 0.5),
                      "logs": {"ll": int(rng.integers(5, 10)), "of": int(rng.integers(5, 9)), "ml": int(rng.integers(5, 10))}}
                for name in ("ll", "of", "ml"):
                    sq[name] = str(rng.choice(["predef", "fse", "fse", "try_rle", "try_repeat"]))
                ns = len(seqs)
                lo = 1 if ns < 128 else (2 if ns < 0x7F00 else 3)
                sq["form"] = 3 if lo == 3 else int(rng.integers(lo, 3))
                b["seq"] = sq
        blocks.append(b)
        pos += size
    single = bool(rng.random() < 0.6)
    ok = [f for f in (0, 1, 2, 4, 8) if not (f == 1 and (n >= 256 or not single)) and not (f == 2 and not 256 <= n < 65792)
          and not (f == 0 and single)]
    return {"blocks": blocks, "single": single, "fcs": int(rng.choice(ok)), "dict_flag": int(rng.integers(0, 4)),
            "checksum": "ok" if rng.random() < 0.4 else None, "window": int(rng.integers(0, 60))}




# ------------------------------------------------------------------------------------------------
# The named cases: every frame the GPU tests decode, checked against libzstd on the CPU first.
# ------------------------------------------------------------------------------------------------
class Case:
    """stream: one or more frames as a stream holds them; content: what a valid stream decodes to;
    valid: libzstd must give exactly content (else: an error, the case's one defect); has(recs): the
    emitted records carry the feature the case is named for; group: the test that reports it."""

    def __init__(self, name, stream, content, recs, has, valid=True, group="misc"):
        self.name, self.stream, self.content, self.recs = name, bytes(stream), bytes(content), recs
        self.has, self.valid, self.group = has, valid, group

    def __repr__(self):
        return self.name


def _b0(recs):
    return recs[0]["blocks"]


def zero_bit_seqs(n):
    """n sequences of no literals and a 3-byte match through repeat code 1: with ll == 0 that is the
    second history slot, so the offsets alternate (4, 1, 4, ...); LL, OF and ML codes are all 0."""
    rep, out = [1, 4, 8], []
    for _ in range(n):
        off, rep = ofv_apply(rep, 1, 0)
        out.append((0, 3, off, 1))
    return out


def _lit_content(rng, n, L, step=3):
    """n literals over at most min(2^L, 40) symbols, spaced `step` apart (gaps give zero weights)."""
    a = min(1 << L, 40)
    v = np.minimum(rng.geometric(0.15, n) - 1, a - 1)
    v[:a] = np.arange(a)[:n]  # every symbol present: the table's leaf count is known
    return (v * step).astype(np.uint8).tobytes()


_CASES = None


def catalogue():
    global _CASES
    if _CASES is None:
        _CASES = _make_cases()
    return _CASES


def _make_cases():
    C = []
    rng = np.random.default_rng(20240611)

    def add(name, frame_rec_content, has, **kw):
        f, rec, content = frame_rec_content
        C.append(Case(name, f, content, [rec], has, **kw))

    def one(content, block, **frame):
        f, rec = build_frame(content, dict(frame, blocks=[dict(block, size=len(content))]))
        return f, rec, content

    # ---- Huffman table logs
    for L in (1, 2, 5, 6, 11, 12):
        for streams in (1, 4):
            for desc in ("direct", "fse"):
                c = _lit_content(rng, 700, L)
                lit = dict(mode="huf", L=L, streams=streams, desc=desc, span=129, min_len=2 if L == 12 else 1)
                add(f"huf_log{L}_{streams}s_{desc}", one(c, dict(type="comp", lit=lit)),
                    lambda r, L=L, s=streams, d=desc: _b0(r)[0]["huf_log"] == L and _b0(r)[0]["huf_streams"] == s and
                    _b0(r)[0]["huf_desc"] == d and _b0(r)[0]["huf_max_weight"] <= 11, group="huf_logs")
    c = bytes(rng.integers(0, 129, 3000, dtype=np.uint8)) + bytes(range(129))
    add("huf_direct_128_weights", one(c, dict(type="comp", lit=dict(mode="huf", L=9, desc="direct", span=129))),
        lambda r: _b0(r)[0]["huf_nweights"] == 128 and _b0(r)[0]["huf_desc"] == "direct", group="huf_logs")
    for L in (11, 12):  # the table outlives a sequence block and a raw block: parked in HBM
        b = Builder(L, alphabet=60)
        hl = dict(mode="huf", L=L, min_len=2 if L == 12 else 1, desc="fse", cover=60)
        b.comp([(300, 20, 7), (100, 9, 50)], tail=200, lit=hl).raw(100)
        b.comp([(250, 12, 3), (0, 5, 400)], tail=77, lit=dict(mode="treeless"))
        b.comp([], tail=333, lit=dict(mode="treeless", streams=1))
        add(f"huf_log{L}_parked_treeless", b.finish(),
            lambda r, L=L: _b0(r)[0]["huf_log"] == L and _b0(r)[0]["nbseq"] > 0 and _b0(r)[2]["lit_mode"] == "treeless"
            and _b0(r)[2]["huf_log"] == L and _b0(r)[3]["lit_mode"] == "treeless", group="huf_logs")
    for order in ((12, 11, 12), (11, 12, 11)):
        b = Builder(sum(order), alphabet=60)
        for L in order:
            b.comp([(300, 20, 7)], tail=300, lit=dict(mode="huf", L=L, min_len=2 if L == 12 else 1, cover=60))
        b.comp([(200, 5, 9)], tail=100, lit=dict(mode="treeless"))
        add("huf_logs_" + "_".join(map(str, order)) + "_treeless", b.finish(),
            lambda r, o=order: [x["huf_log"] for x in _b0(r)] == list(o) + [o[-1]], group="huf_logs")

    # ---- four-stream literals: every size in every header form that holds it
    sizes = [4, 6, 7, 8, 9, 255, 256, 1021, 1023, 1024, 16383, 16384]  # 5 cannot split: 3 * ceil(5/4) > 5
    for hform in (3, 4, 5):
        blocks, content = [], bytearray()
        for n in sizes:
            if n >= (1 << {3: 10, 4: 14, 5: 18}[hform]):
                continue
            c = _lit_content(rng, n, 2 if n < 10 else 6)
            content += c
            blocks.append(dict(type="comp", size=n, lit=dict(mode="huf", L=2 if n < 10 else 6, streams=4, hform=hform,
                                                             span=129)))
        f, rec = build_frame(bytes(content), dict(blocks=blocks))
        add(f"huf4_sizes_hform{hform}", (f, rec, bytes(content)),
            lambda r, h=hform: all(x["lit_hform"] == h and x["huf_streams"] == 4 for x in _b0(r)) and
            any(x["huf_stream_syms"][3] < x["huf_stream_syms"][0] for x in _b0(r)) and
            {x["lit_size"] for x in _b0(r)} >= {4, 9, 255, 256, 1023}, group="huf4_sizes")

    # ---- header window (256 bytes): a raw block in front puts the next block's header at each offset
    # (its length 180 to 265), so the block header, the literals header (3 further), the end of the table
    # description and the jump table (6 + description further) each land on every offset from 230 to 262
    for P in range(190, 276):
        for desc in ("direct", "fse"):
            b = Builder(P, alphabet=40)
            # frame header 4 + 1 + 2 (2-byte size: the content is >= 256 bytes), raw block header 3
            b.raw(P - 7 - 3)
            b.comp([(120, 30, 11)], tail=150, lit=dict(mode="huf", L=7, desc=desc, span=129))
            fr = b.finish(fcs=2)
            add(f"hdrwin_block_at_{P}_{desc}", fr,
                lambda r, P=P: _b0(r)[1]["off"] == P and _b0(r)[1]["huf_streams"] == 4, group="hdrwin")
    for n in (230, 247, 248, 249, 255, 256, 262):  # a skippable frame in front: the frame header moves
        b = Builder(n, alphabet=40).comp([(120, 30, 11)], tail=150, lit=dict(mode="huf", L=7, span=129))
        f, rec, c = b.finish()
        C.append(Case(f"hdrwin_skippable_{n}", skippable(n - 8) + f, c, [rec], lambda r: True, group="hdrwin"))

    # ---- match copies
    mls = [3, 4, 5, 63, 64, 65, 70, 130]
    for off in (1, 2, 3, 7, 31, 63, 64, 65, 127, 128):
        ms = sorted(set(mls + [m for m in (off - 1, off, off + 1) if m >= 3]))
        seqs = [(max(off, 3), ms[0], off)] + [(2, m, off) for m in ms[1:]]
        assert len(seqs) <= 64 and sum(q[0] + q[1] for q in seqs) + 5 <= 4096
        has = lambda r, off=off, k=0: all(q[2] == off for q in _b0(r)[k]["seqs"]) and \
            {q[1] for q in _b0(r)[k]["seqs"]} >= {3, 4, 5, 63, 64, 65, max(off, 3)}
        add(f"match_off{off}_lds", Builder(off).comp(seqs, tail=5, seq=dict(rep="ban")).finish(), has, group="match")
        add(f"match_off{off}_global", Builder(off).comp(seqs + [(1, 3000, off), (0, 1500, off)], tail=5,
                                                         seq=dict(rep="ban")).finish(), has, group="match")
        add(f"match_off{off}_loop", Builder(off).comp(seqs * (65 // len(seqs) + 1), tail=5, seq=dict(rep="ban", of="fse")).finish(),
            lambda r, off=off: _b0(r)[0]["nbseq"] >= 65 and all(q[2] == off for q in _b0(r)[0]["seqs"]), group="match")
        first = [(0, ms[-1], off)] + [(2, m, off) for m in ms]  # the first match reaches back into the block before
        add(f"match_off{off}_after_raw", Builder(off).raw(off + 2).comp(first, tail=5, seq=dict(rep="ban")).finish(),
            lambda r, has=has: has(r, k=1) and _b0(r)[0]["type"] == "raw", group="match")
        add(f"match_off{off}_after_rle", Builder(off).rle(off + 2).comp(first, tail=5, seq=dict(rep="ban")).finish(),
            lambda r, has=has: has(r, k=1) and _b0(r)[0]["type"] == "rle", group="match")
        add(f"match_off{off}_after_comp", Builder(off).comp([(off + 3, 9, 2)], tail=1).comp(
            first, tail=5, seq=dict(rep="ban")).finish(),
            lambda r, has=has: has(r, k=1) and _b0(r)[0]["type"] == "comp", group="match")

    # ---- repeat offsets: each code with ll == 0 and ll > 0, chained so that the three slots rotate
    chain = [(20, 4, 5), (3, 4, 9), (2, 4, 13)]
    for rnd_ in range(3):
        for v in (1, 2, 3):
            for ll in (0, 2):
                chain.append((ll, 4 + rnd_, None, v))
    b = Builder(77).comp(chain, tail=3)
    add("rep_all_codes_chained", b.finish(),
        lambda r: {(v, 0) for v in _b0(r)[0]["ll0_rep"]} | {(v, 1) for v in _b0(r)[0]["llpos_rep"]} ==
        {(v, z) for v in (1, 2, 3) for z in (0, 1)} and len({q[2] for q in _b0(r)[0]["seqs"]}) >= 6, group="rep")
    b = Builder(78).comp([(10, 4, 1), (0, 5, None, 3), (0, 5, None, 3), (2, 4, None, 1)], tail=3)
    add("rep0_minus_1_is_0", b.finish(), lambda r: _b0(r)[0]["seqs"][1][2] == 1 and _b0(r)[0]["ofvs"][1:3] == [3, 3],
        group="rep")
    b = Builder(79).comp([(20, 4, 5), (3, 4, 9), (2, 4, 13)], tail=3).raw(40).comp([(0, 4, None, 1), (2, 4, None, 2)])
    b.rle(30).comp([(1, 4, None, 3), (0, 6, None, 2)], tail=2).comp([], tail=25).comp([(0, 7, None, 3), (4, 4, None, 1)])
    add("rep_history_across_blocks", b.finish(),
        lambda r: [x["type"] for x in _b0(r)] == ["comp", "raw", "comp", "rle", "comp", "comp", "comp"] and
        _b0(r)[5]["nbseq"] == 0 and all(v <= 3 for k in (2, 4, 6) for v in _b0(r)[k]["ofvs"]), group="rep")

    # ---- sequence tables
    def mixed(seed, n, maxoff=60000):
        """A raw block of history, then n sequences with long codes: wide offsets, literal and match lengths."""
        b = Builder(seed)
        b.raw(maxoff + 8)
        r = np.random.default_rng(seed)
        return b, [(int(r.choice([0, 1, 3, 17, 40])), int(r.choice([3, 4, 20, 36, 70])),
                    int(r.integers(1, maxoff))) for _ in range(n)]
    b, seqs = mixed(5, 400)
    sq = dict(ll="fse", of="fse", ml="fse", logs=dict(ll=9, of=8, ml=9), low=True, rep="ban",
              ghosts=dict(ll=[30, 35], of=[25, 31], ml=[48, 52]))
    add("seq_fse_logs_9_8_9_low_and_zero_runs", b.comp(seqs, tail=9, seq=sq).finish(),
        lambda r: all(_b0(r)[1]["fse_desc"][k]["log"] == lg and _b0(r)[1]["fse_desc"][k]["low"] > 0 and
                      _b0(r)[1]["fse_desc"][k]["zero_runs"] for k, lg in (("ll", 9), ("of", 8), ("ml", 9))), group="seqtab")
    same = [(2, 5, 9 + (i % 4)) for i in range(90)]  # one LL, one ML and one OF code
    for rl in (("ll",), ("of", "ml"), ("ll", "of", "ml")):
        sq = dict(rep="ban", **{k: "rle" for k in rl})
        add("seq_rle_" + "_".join(rl), Builder(len(rl)).comp([(16, 3, 2)], tail=0).comp(same, tail=4, seq=sq).finish(),
            lambda r, rl=rl: [m == "rle" for m in _b0(r)[1]["seq_modes"]] == [k in rl for k in ("ll", "of", "ml")],
            group="seqtab")
    for prev in ("predef", "rle", "fse"):
        sq = dict(rep="ban", ll=prev, of=prev, ml=prev)
        b = Builder(ord(prev[0])).comp([(16, 3, 2)], tail=0).comp(same, tail=4, seq=sq).raw(10)
        b.comp(same[:40], tail=2, seq=dict(rep="ban", ll="repeat", of="repeat", ml="repeat"))
        add(f"seq_repeat_after_{prev}", b.finish(),
            lambda r, p=prev: _b0(r)[1]["seq_modes"] == (p,) * 3 and _b0(r)[3]["seq_modes"] == ("repeat",) * 3,
            group="seqtab")
    for n, form in ((127, 1), (127, 2), (128, 2), (0x7EFF, 2), (0x7F00, 3)):
        b = Builder(n).rle(16, 9).comp(zero_bit_seqs(n), tail=2, const=9, lit=dict(mode="rle"),
                                       seq=dict(ll="rle", of="rle", ml="rle", form=form))
        add(f"seq_nbseq_{n}_form{form}", b.finish(),
            lambda r, n=n, f=form: _b0(r)[1]["nbseq"] == n and _b0(r)[1]["nbseq_form"] == f, group="seqtab")
    b = Builder(35).comp([(131071, 3, 1), (0, 131074, 1)], const=3, lit=dict(mode="rle"),
                         seq=dict(ll="fse", of="predef", ml="fse", rep="ban"))
    add("seq_ll35_ml52_all_extra_bits", b.finish(), lambda r: _b0(r)[0]["max_codes"] == (35, 2, 52), group="big")
    b = Builder(18).raw(262144).comp([(0, 8, 262142)], tail=1, seq=dict(rep="ban", of="rle"))
    add("seq_offset_code_18_in_256k", b.finish(), lambda r: _b0(r)[1]["max_codes"][1] == 18, group="big")
    b, seqs = mixed(6, 3200)
    add("seq_bitstream_over_three_windows", b.comp(seqs, tail=9, seq=dict(rep="ban", ll="fse", of="fse", ml="fse")).finish(),
        lambda r: _b0(r)[1]["seq_bits_len"] > 3 * 2048, group="seqtab")

    # ---- more sequences in a block than 128 KiB / 3
    for n in (43700, 98047):
        b = Builder(n).rle(16, 9).comp(zero_bit_seqs(n), tail=1, const=9, lit=dict(mode="rle"),
                                       seq=dict(ll="rle", of="rle", ml="rle"))
        add(f"seq_count_{n}", b.finish(), lambda r, n=n: _b0(r)[1]["nbseq"] == n and n > 43692, group="seqcount")

    # ---- frame level
    c300 = _lit_content(rng, 300, 5)
    c200 = c300[:200]
    blk = dict(type="comp", lit=dict(mode="huf", L=5, span=129))
    for fcs, single, c in ((1, True, c200), (2, True, c300), (2, False, c300), (4, True, c300), (4, False, c200),
                           (8, True, c300), (8, False, c200), (0, False, c300)):
        add(f"frame_fcs{fcs}_{'single' if single else 'window'}", one(c, blk, fcs=fcs, single=single),
            lambda r, f=fcs, s=single: r[0]["fcs_bytes"] == f and r[0]["single"] == s, group="frame")
    for d in (1, 2, 3):
        add(f"frame_dict_flag{d}_id0", one(c300, blk, dict_flag=d), lambda r, d=d: r[0]["dict_flag"] == d, group="frame")
    add("frame_checksum_ok", one(c300, blk, checksum="ok"), lambda r: r[0]["checksum"] == "ok", group="frame")
    f, rec, _ = one(c300, blk)
    e, erec = build_frame(b"", dict(blocks=[dict(type="raw", size=0)]))
    for name, stream in (("skippable_before", skippable(40) + f), ("skippable_after", f + skippable(0, nibble=7)),
                         ("skippable_between", f + skippable(300, nibble=15) + e),
                         ("two", f + e), ("three", f + e + e)):
        C.append(Case(f"frames_{name}", stream, c300, [rec, erec], lambda r: True, group="frame"))
    f1, rec1, _ = one(c300[:120], blk)
    f2, rec2, _ = one(c300[120:], blk)
    C.append(Case("frames_two_with_content_each", f1 + f2, c300, [rec1, rec2], lambda r: True, group="frame"))
    for n in (200000, 300000):
        add(f"block_raw_{n}", Builder(n).raw(n).finish(), lambda r, n=n: _b0(r)[0]["bsize"] == n, group="big")
        add(f"block_rle_{n}", Builder(n).rle(n).finish(), lambda r, n=n: _b0(r)[0]["size"] == n and _b0(r)[0]["bsize"] == n,
            group="big")
    b = Builder(1024).raw(6000).comp([(3, 40, 5000)], tail=2, seq=dict(rep="ban"))
    add("offset_beyond_1k_window", b.finish(single=False, window=0, fcs=2),
        lambda r: not r[0]["single"] and _b0(r)[1]["seqs"][0][2] == 5000, group="frame")
    c = bytes(rng.integers(0, 256, 131067, dtype=np.uint8))
    add("block_comp_131071_bytes", one(c, dict(type="comp", lit=dict(mode="raw", hform=3))),
        lambda r: _b0(r)[0]["bsize"] == 131071, group="big")

    # ---- frames with one defect
    def bad(name, frc, has=lambda r: True, group="defect"):
        f, rec, content = frc
        C.append(Case(name, f, content, [rec], has, valid=False, group=group))
    c = _lit_content(rng, 700, 12)
    for desc in ("direct", "fse"):
        bad(f"bad_weight_12_{desc}", one(c, dict(type="comp", lit=dict(mode="huf", L=12, min_len=1, desc=desc, span=129))),
            lambda r: _b0(r)[0]["huf_max_weight"] == 12 and _b0(r)[0]["huf_log"] == 12, group="weight12")
    c = bytes(rng.integers(0, 256, 131068, dtype=np.uint8))
    bad("bad_block_comp_131072_bytes", one(c, dict(type="comp", lit=dict(mode="raw", hform=3))),
        lambda r: _b0(r)[0]["bsize"] == 131072, group="block128k")
    c = _lit_content(rng, 400, 4)
    t = HufTable.for_content(c, 4, span=129)
    bad("bad_table_log_13", one(c, dict(type="comp", lit=dict(mode="huf", table=t, weights=[11, 11, 11, 11]))))
    bad("bad_weight_sum_not_power_of_two", one(c, dict(type="comp", lit=dict(mode="huf", table=t, weights=[3, 1]))))
    for st in (1, 4):
        for d in (-1, 1):
            bad(f"bad_huf_stream_{'early' if d < 0 else 'late'}_{st}s",
                one(c, dict(type="comp", lit=dict(mode="huf", L=4, span=129, streams=st, stream_delta=d))))
    bad("bad_jump_table_past_section", one(c, dict(type="comp", lit=dict(mode="huf", L=4, span=129, jump_past=True))))
    bad("bad_repeat_mode_without_table", Builder(1).comp([(9, 4, 2)], tail=3, seq=dict(ll="repeat", no_table=True)).finish())
    bad("bad_treeless_without_table", one(c, dict(type="comp", lit=dict(mode="treeless", no_table=True))))
    for k, s in (("ll", 36), ("of", 32), ("ml", 53)):
        bad(f"bad_rle_symbol_{k}_{s}", Builder(s).comp([(16, 3, 2)]).comp(same, tail=4, seq=dict(
            rep="ban", **{k: "rle"}, rle_symbol={k: s})).finish())
    bad("bad_offset_before_frame_block1", Builder(2).comp([(9, 4, 10)], tail=3, seq=dict(rep="ban"), before_start=True).finish())
    bad("bad_offset_before_frame_block2", Builder(3).raw(50).comp([(9, 4, 60)], tail=3, seq=dict(rep="ban"),
                                                                   before_start=True).finish())
    bad("bad_literal_length_past_literals", Builder(4).comp([(9, 4, 2), (6, 5, 3)], lit=dict(mode="raw", phantom=1)).finish())
    for name, sq in (("predef", {}), ("fse", dict(ll="fse", of="fse", ml="fse", logs=dict(ll=9, of=8, ml=9)))):
        # bits left over: as many as the state update after the last sequence reads are accepted, one more is not
        sb = [(9, 4, 2), (6, 5, 3), (1, 40, 17), (18, 3, 1)]
        for k in (1, 0):
            f = Builder(5).comp(sb, tail=2, seq=dict(sq, extra_bits=k, extra_over_slack=True, rep="ban")).finish()
            slack = f[1]["blocks"][0]["end_slack"]
            if k == 0:
                f = Builder(5).comp(sb, tail=2, seq=dict(sq, extra_bits=slack, rep="ban")).finish()
                add(f"seq_bits_left_over_within_last_update_{name}", f, lambda r: _b0(r)[0]["end_slack"] > 0, group="leftover")
            else:
                bad(f"bad_sequence_bits_left_over_{name}", f)
    c5 = bytes([0, 3, 3, 0, 3])
    bad("known_divergence_huf4_size_5_overhang", one(c5, dict(type="comp", lit=dict(mode="huf", L=1, streams=4, overhang=True,
                                                                                  span=129))),
        lambda r: _b0(r)[0]["huf_stream_syms"] == [2, 2, 2, 0], group="overhang")
    b, sq_ = mixed(7, 50)
    bad("known_divergence_sequence_stream_cut", b.comp(sq_, tail=3, seq=dict(rep="ban", ll="fse", of="fse", ml="fse",
                                                                            cut_bytes=1)).finish(), group="cut")
    bad("bad_content_size", one(c300, blk, fcs_value=301))
    bad("bad_block_type_3", one(c300, dict(type="reserved")))
    f, rec, _ = one(c300, blk)
    C.append(Case("bad_truncated_skippable", f + skippable(20, truncate=5), c300, [rec], lambda r: True, valid=False,
                  group="defect"))
    bad("bad_empty_compressed_block_2_bytes", Builder(6).raw(20).comp([], tail=0, lit=dict(mode="raw")).finish(),
        lambda r: _b0(r)[1]["bsize"] == 2)
    bad("known_divergence_wrong_checksum", one(c300, blk, checksum="bad"), lambda r: r[0]["checksum"] == "bad",
        group="checksum")
    names = [x.name for x in C]
    assert len(set(names)) == len(names)
    return C
