"""Byte streams built for the speculation hazards of the GPU match search (csrc/pgn_zenc.h
fast_search_wave), and the host profile (csrc/model_capi.hip z1m_search_profile) that says which of
its paths a stream's sequences take.  Every stream is carried as the M stream of a C5 chunk
(test_gpu_enc_tables.m_signal), so the chunk's M frame is ZSTD_compress(stream, 1).  Seeds are fixed:
the set is the same on every machine.  Shared by test_search_profile.py (CPU: what the cases reach)
and test_gpu_search.py (GPU: byte equality with the oracle)."""
import ctypes as C
import functools

import numpy as np

import _oracle as O
from test_gpu_enc_tables import frame_info, m_signal, search

N_DIRECTED = 20000
SINGLE_SIZES = (1000, 4096, 16384, 16385, 65536, 131069)
WIDE_SIZES = (131070, 131072)  # still one block, but the 20-bit index with a 7-bit fingerprint
MULTI_SIZES = (131073, 200000, 262144, 262145, 540000)
PAIR_SIZES = (1048573, 1048574)  # index 20 -> 21 bits

# profile columns (model_capi.hip z1m_search_profile)
POS, K, KIND, BACK, MLEN, TO_END, NFALSE, LL, OFFSET, MLBASE = range(10)
REP_IP2, TABLE, SAME_ROUND, POST_REP = range(4)

END_LENGTHS = tuple(range(4, 13)) + tuple(range(250, 263)) + tuple(range(506, 519))
# A match is found at a visited position, and the search visits ip0 <= n - 10 and ip1 <= n - 9
# (ip1 < ilimit = n - 8); the repcode tests (ip0 + 2, and ip0 <= ilimit after a match) start at
# n - 8 at the latest.  So no match that ends at the stream's end is shorter than 8 bytes: the
# lengths 4 .. 7 exist only before the end.
END_LENGTHS_AT_END = tuple(l for l in END_LENGTHS if l >= 8)
BACKS = (63, 64, 65, 127, 128, 129)
LANES = (0, 62, 63)
FALSE_EQUAL = (3,)  # leading bytes a false same-slot, same-fingerprint candidate shares with the position


def gap_before_end(length):
    """The directed distance (1 .. 9) between the end of the match of this length and the stream's end.
    A match of 4 .. 12 bytes that ends g bytes before the end holds a visited position (<= n - 9) with 4
    bytes of it ahead only if length >= 9 - g: those lengths take g = 13 - length, the others cycle."""
    return 13 - length if length <= 12 else 1 + length % 9


# ---- the host model ---------------------------------------------------------------------------------
def _arr(stream):
    return np.ascontiguousarray(np.frombuffer(bytes(stream), np.uint8))


def profile(stream) -> np.ndarray:
    """One row per sequence of the single-block stream (columns above)."""
    M = O.model()
    M.z1m_search_profile.restype = C.c_size_t
    M.z1m_search_profile.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    a = _arr(stream)
    assert 7 <= a.size <= 131072
    rows = np.zeros((a.size // 4 + 2, 10), np.uint32)
    nb = M.z1m_search_profile(a.ctypes.data, a.size, rows.ctypes.data, rows.shape[0])
    assert nb <= rows.shape[0]
    return rows[:nb].astype(np.int64)


def certified(stream) -> bool:
    """The encoder's no-match certificate holds: the GPU does not run the search on this stream."""
    M = O.model()
    M.z1m_no_match_certificate.restype = C.c_int
    M.z1m_no_match_certificate.argtypes = [C.c_void_p, C.c_size_t]
    a = _arr(stream)
    return bool(M.z1m_no_match_certificate(a.ctypes.data, a.size))


def model_compress(stream) -> bytes:
    M = O.model()
    a = _arr(stream)
    cap = a.size + a.size // 128 + 1024
    out = np.zeros(cap, np.uint8)
    r = M.z1m_compress(a.ctypes.data, a.size, out.ctypes.data, cap)
    assert r > 0
    return out[:r].tobytes()


# ---- generators -------------------------------------------------------------------------------------
def noise(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8)


def noise64(rng, n):
    """Noise over 64 symbols: its literals gain under Huffman, so a block with only a few short matches is
    still written compressed (a block that gains too little is written raw, whatever the search found)."""
    return rng.integers(0, 64, n, dtype=np.uint8)


def late_copy(rng, n):
    """Noise with copies of 300 .. 3,000 bytes from far back, 500 .. 6,000 literals apart (the far
    anchor makes the visits sparse, so a copy is hit deep inside and extended backwards); shorter in
    proportion below 20,000 bytes."""
    a = noise(rng, n)
    f = min(1.0, n / 20000)
    p = int(3000 * f)
    while p + int(4000 * f) < n:
        ln = int(rng.integers(int(300 * f), int(3000 * f)))
        s = int(rng.integers(0, p - ln)) if p - ln > 0 else 0
        a[p:p + ln] = a[s:s + ln]
        p += ln + int(rng.integers(int(500 * f), int(6000 * f)))
    return a.tobytes()


def short_period(rng, n):
    """Noise with stretches of period 1 .. 120: candidates written by the round's own visits, and
    overlapping copies for the decoder."""
    a = noise(rng, n)
    p = 200
    while p + 700 < n:
        per = int(rng.integers(1, 121))
        ln = int(rng.integers(per + 8, 600))
        a[p:p + ln] = np.resize(a[p - per:p], ln)
        p += ln + int(rng.integers(20, 400))
    return a.tobytes()


def word_soup(rng, n, words=None):
    """Picks from 600 .. 3,000 random words of 5 .. 11 bytes: occupied slots that hold other bytes, false
    fingerprints and retries."""
    words = int(rng.integers(600, 3001)) if words is None else words
    lens = rng.integers(5, 12, words)
    starts = np.concatenate([[0], np.cumsum(lens)])
    pool = noise(rng, int(starts[-1]))
    picks = rng.integers(0, words, n // 5 + 1)
    return np.concatenate([pool[starts[w]:starts[w + 1]] for w in picks])[:n].tobytes()


def small_alphabet(rng, n):
    """2 .. 4 symbols: a hit almost every visit, and filter slots shared by many lanes."""
    return rng.integers(0, int(rng.integers(2, 5)), n, dtype=np.uint8).tobytes()


def runs(rng, n):
    """Copies that alternate between two offsets with 0 .. 3 literals between them: repcode chains (the
    repcode at ip0 + 2, the post-match repcode), offset swaps and sequences without literals."""
    a = noise(rng, n)
    p = 300
    while p + 400 < n:
        d = [int(rng.integers(8, 250)), int(rng.integers(8, 250))]
        for j in range(int(rng.integers(2, 12))):
            ln = int(rng.integers(5, 40))
            if p + ln + 4 >= n:
                break
            o = d[j & 1] if rng.integers(0, 4) else d[0]
            a[p:p + ln] = a[p - o:p - o + ln] if o >= ln else np.resize(a[p - o:p], ln)
            p += ln + int(rng.integers(0, 4))
        p += int(rng.integers(10, 300))
    return a.tobytes()


def uniform(rng, n):
    return noise(rng, n).tobytes()


# the sizes each generator runs at: every single-block size and both index layouts where the search
# has most to get wrong, fewer of the large ones elsewhere (the whole set stays under 8 MB)
GRID = {"late_copy": SINGLE_SIZES + WIDE_SIZES[1:], "short_period": SINGLE_SIZES[:-1] + WIDE_SIZES[1:],
        "word_soup": SINGLE_SIZES[:-1] + WIDE_SIZES, "small_alphabet": SINGLE_SIZES[:-2] + WIDE_SIZES[1:],
        "runs": SINGLE_SIZES[:-2] + WIDE_SIZES[1:], "uniform": SINGLE_SIZES[:-1]}
GENERATORS = {"late_copy": late_copy, "short_period": short_period, "word_soup": word_soup,
              "small_alphabet": small_alphabet, "runs": runs, "uniform": uniform}


# ---- directed cases ---------------------------------------------------------------------------------
def _differ(a, i, j):
    """Make a[i] != a[j] (by changing a[i])."""
    if a[i] == a[j]:
        a[i] ^= 0x55


def end_match(rng, length, gap):
    """A 20,000-byte stream whose last match has `length` bytes and ends `gap` bytes before the end
    (0: at the end).  A helper copy ends shortly before each of the match's source and the match, so
    the visits around both are dense (two positions per step of 2)."""
    n = N_DIRECTED
    a = noise(rng, n)
    a[300:340] = a[100:140]                # helper: the anchor moves to 340
    src = 344 + int(rng.integers(0, 8))    # the match's source, every position of its head visited
    e = n - gap
    s = e - length
    h = s - int(rng.integers(6, 30))       # the second helper ends here
    a[h - 400:h] = a[900:1300]             # long enough for the sparse visits this far from the anchor
    # shorter than the hashed bytes (mls 6 here), or from the last position a repcode is tried at (n - 8,
    # one past the last visit): only a repcode finds it -- the helper's offset
    if length < 6 or (gap == 0 and length == 8):
        src = s - (h - 400 - 900)
        _differ(a, h, 1300)
    a[s:e] = a[src:src + length]
    _differ(a, s - 1, src - 1)
    if gap:
        _differ(a, e, src + length)
    return a.tobytes()


def compressed_block(stream) -> bool:
    """The oracle writes the stream's (first) block compressed: only then do the sequences reach the frame
    (a block that gains too little is written raw, whatever the search found)."""
    return frame_info(O.zstd_compress1(stream))["block"] == 2


def _last_is(stream, length, gap):
    r = profile(stream)
    return compressed_block(stream) and len(r) and r[-1][MLEN] == length and r[-1][POS] == len(stream) - gap - length and \
        r[-1][TO_END] == (gap == 0)


def back_extension(rng, back):
    """A 600-byte copy far from the last match (sparse visits: it is hit deep inside); noise is put back
    over its head so that it starts exactly `back` bytes before the hit."""
    n = N_DIRECTED
    a = noise(rng, n)
    orig = a.copy()
    p = int(rng.integers(9000, 15000))
    q = int(rng.integers(100, 5000))
    a[p:p + 600] = a[q:q + 600]
    rows = profile(a.tobytes())
    hit = [r for r in rows if r[KIND] in (TABLE, SAME_ROUND) and p <= r[POS] + r[BACK] < p + 600]
    if not hit:
        return a.tobytes()
    h = int(hit[0][POS] + hit[0][BACK])  # where the search finds the copy
    if h - back < p:
        return a.tobytes()
    a[p:h - back] = orig[p:h - back]
    _differ(a, h - back - 1, h - back - 1 - (p - q))
    return a.tobytes()


def anchor_stop(rng):
    """Two copies back to back; the second one's source starts with the five bytes that end the first,
    so the second match, hit a little after the first one's end, extends backwards until the anchor
    stops it (the bytes before the anchor are equal too)."""
    n = N_DIRECTED
    a = noise(rng, n)
    s1, s2, e = 500, 1500, 6000 + int(rng.integers(0, 2000))
    a[s2:s2 + 5] = a[s1 + 295:s1 + 300]
    a[e - 300:e] = a[s1:s1 + 300]
    a[e - 5:e + 200] = a[s2:s2 + 205]
    _differ(a, s1 + 300, s2 + 5)
    return a.tobytes()


def anchor_stopped_rows(stream):
    a = np.frombuffer(stream, np.uint8)
    return [r for r in profile(stream)
            if r[KIND] in (TABLE, SAME_ROUND) and r[BACK] > 0 and r[LL] == 0 and r[POS] - (r[OFFSET] - 3) > 0
            and a[r[POS] - 1] == a[r[POS] - (r[OFFSET] - 3) - 1]]


def _le(b):
    """Little-endian value of the bytes b[..., i] (uint64)."""
    return sum(b[..., i].astype(np.uint64) << np.uint64(8 * i) for i in range(b.shape[-1]))


def hash6_13(v):
    """ZSTD_hash6Ptr at hashLog 13 (the parameters of a 20,000-byte frame) of 6 little-endian bytes."""
    return ((v << np.uint64(16)) * np.uint64(227718039650203)) >> np.uint64(64 - 13)


def entry_fp(v, n):
    """The table entry's fingerprint of the low 4 little-endian bytes in a frame of n <= 131,072 bytes: 10
    bits beside the 17-bit index, 7 beside the 20-bit one (pgn_zenc.h ht_fp, ht_idx_bits)."""
    bits = 10 if n + 2 < (1 << 17) else 7
    return (((v & np.uint64(0xFFFFFFFF)) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - bits)


# The fingerprint is the top of a 32-bit product, and the 4th byte moves the product's top 8 bits
# one-to-one: two words that differ in the 4th byte alone never share a 10-bit fingerprint.  A false
# candidate with exactly 3 equal leading bytes exists only under the 7-bit fingerprint, so that case is a
# 131,070-byte stream (with fewer equal bytes 20,000 would do).
FALSE_SIZE = {0: N_DIRECTED, 1: N_DIRECTED, 2: N_DIRECTED, 3: WIDE_SIZES[0]}


FALSE_A, FALSE_B = 349, 452  # where false_prefix plants its pair


def false_prefix(rng, equal):
    """A false table candidate that shares exactly `equal` (< 4) leading bytes with the position: a pair of
    6-byte strings with one hash (the slot), one fingerprint of their first 4 bytes and those leading bytes
    in common, found by bucketing 2^16 random strings.  The first lies in the dense visits after one helper
    match, the second in those after another (a new chain: a table candidate, not a same-round writer),
    and a real match follows in the second one's round.  The search must count the candidate's bytes and
    drop it: accepted with 3 equal bytes it would be a match of 3."""
    n = FALSE_SIZE[equal]
    a = noise64(rng, n)
    a[300:340] = a[100:140]   # helper: anchor 340, every position up to 468 visited
    a[400:440] = a[150:190]   # helper: anchor 440, a new chain
    b = np.zeros((1 << 16, 6), np.uint8)
    b[:] = noise(rng, 6)
    b[:, equal:] = rng.integers(0, 256, (1 << 16, 6 - equal), dtype=np.uint8)  # the common prefix stays
    w = _le(b)
    key = (hash6_13(w) << np.uint64(10)) | entry_fp(w, n)
    order = np.argsort(key, kind="stable")
    k = key[order]
    pairs = np.flatnonzero((k[1:] == k[:-1]) & (b[order[1:], equal] != b[order[:-1], equal]))
    if not pairs.size:
        return a.tobytes()
    i = int(pairs[int(rng.integers(0, pairs.size))])
    a[FALSE_A:FALSE_A + 6] = b[order[i]]
    a[FALSE_B:FALSE_B + 6] = b[order[i + 1]]
    a[470:482] = a[120:132]   # the round's real match
    _differ(a, 469, 119)
    return a.tobytes()


def false_prefix_rows(stream, equal):
    """The rows of the round in which the planted candidate is dropped, if the stream is what
    false_prefix means it to be: [] otherwise."""
    a = np.frombuffer(stream, np.uint8)
    A, B = a[FALSE_A:FALSE_A + 6], a[FALSE_B:FALSE_B + 6]
    if not ((A[:equal] == B[:equal]).all() and A[equal] != B[equal]):
        return []
    wa, wb = _le(A[None, :]), _le(B[None, :])
    if hash6_13(wa)[0] != hash6_13(wb)[0] or entry_fp(wa, a.size)[0] != entry_fp(wb, a.size)[0]:
        return []
    r = profile(stream)
    # the second helper's match ends at 440 and the next sequence, in its first round, saw one false candidate
    ends = r[:, POS] + r[:, MLEN]
    return [x for j, x in enumerate(r) if j and ends[j - 1] == 440 and x[KIND] == TABLE and x[K] < 64
            and FALSE_B < x[POS] + x[BACK] and x[NFALSE] == 1]


def visit_positions(anchor, first):
    """Positions of the visits after a match (or from the frame's start: first) while nothing is found."""
    e = 257 if first else 256
    out = []
    while len(out) < 400:
        out.append(anchor + e - 256)
        e += e >> 7
    return out


def _lz_copy(a, dst, src, ln):
    """a[dst:dst + ln] = what an LZ copy from src gives (the source may run into the destination)."""
    a[dst:dst + ln] = np.resize(a[src:min(dst, src + ln)], ln)


def lane_hits(rng, lane):
    """Matches whose first hit is visit k of its chain, k % 64 == lane, over several rounds (k = lane,
    lane + 64, ...; lane 0 from k = 64): the target lies at visit k's position (or one past it: the
    second candidate), its source at an earlier visit's -- of an earlier round (a table candidate) or,
    for the lanes 62 and 63, of the same round."""
    n = N_DIRECTED
    a = noise64(rng, n)
    anchor, first = 0, True
    for i, m in enumerate((1, 2, 3, 4, 1, 2) if lane == 0 else (0, 1, 2, 3, 0, 1)):
        k = lane + 64 * m
        pos = visit_positions(anchor, first)
        j = int(rng.integers(64 * m, k - 2)) if lane and (m == 0 or i % 2) else int(rng.integers(2, 64 * m))
        second = int(rng.integers(0, 2))
        tp, sp = pos[k] + second, pos[j] + second
        ln = int(rng.integers(20, 60))
        if tp + ln + 600 > n:
            break
        _lz_copy(a, tp, sp, ln)
        _differ(a, tp - 1, sp - 1)
        _differ(a, tp + ln, sp + ln)
        anchor, first = tp + ln, False
    return a.tobytes()


def _lane_count(stream, lane):
    return sum(1 for r in profile(stream) if r[KIND] != POST_REP and r[K] % 64 == lane and (lane or r[K] >= 64))


# ---- the set ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def profiled_cases():
    """name -> stream: the single-block cases, each with a profile."""
    c = {}
    seed = 7000
    for g, make in GENERATORS.items():
        for n in GRID[g]:
            seed += 1
            c[f"{g}/{n}"] = make(np.random.default_rng(seed), n)
    # uniform streams on which the certificate fails (a false positive of its filter, or 4 equal bytes
    # under one hash that the search then rejects or takes): the exact search runs on noise
    found = 0
    for s in range(4000):
        u = uniform(np.random.default_rng(8000 + s), 5000 + s % 7)
        if not certified(u):
            c[f"uniform/uncertified{found}_{len(u)}"] = u
            found += 1
            if found == 10:
                break
    assert found == 10
    for length in END_LENGTHS:
        if length in END_LENGTHS_AT_END:
            c[f"end/{length}_at_end"] = search(lambda r, l=length: end_match(r, l, 0), lambda s, l=length: _last_is(s, l, 0))
        g = gap_before_end(length)
        c[f"end/{length}_gap{g}"] = search(lambda r, l=length, g=g: end_match(r, l, g),
                                           lambda s, l=length, g=g: _last_is(s, l, g))
    for b in BACKS:
        c[f"back/{b}"] = search(lambda r, b=b: back_extension(r, b),
                                lambda s, b=b: (lambda p: len(p) and (p[:, BACK] == b).any())(profile(s)))
    c["back/anchor_stop"] = search(anchor_stop, lambda s: len(anchor_stopped_rows(s)) > 0)
    for eq in FALSE_EQUAL:
        c[f"false{eq}/pair"] = search(lambda r, eq=eq: false_prefix(r, eq), lambda s, eq=eq: len(false_prefix_rows(s, eq)) > 0)
    for lane in LANES:
        c[f"lane/{lane}"] = search(lambda r, lane=lane: lane_hits(r, lane), lambda s, lane=lane: _lane_count(s, lane) >= 3)
    return c


@functools.lru_cache(maxsize=None)
def large_cases():
    """name -> stream: multi-block and large frames (byte equality only, no profile)."""
    c = {}
    seed = 9000
    for g in ("word_soup", "late_copy"):
        for n in MULTI_SIZES:
            seed += 1
            c[f"{g}/{n}"] = GENERATORS[g](np.random.default_rng(seed), n)
    pair = word_soup(np.random.default_rng(9100), PAIR_SIZES[1])
    c[f"word_soup/{PAIR_SIZES[0]}"] = pair[:PAIR_SIZES[0]]
    c[f"word_soup/{PAIR_SIZES[1]}"] = pair
    return c


def cases():
    return {**profiled_cases(), **large_cases()}


def directed(name):
    return name.split("/")[0] in ("end", "back", "lane", "false3")


@functools.lru_cache(maxsize=None)
def reference():
    """name -> (signal, the oracle's blob, its stream sizes); computed once."""
    ref = {}
    for name, s in cases().items():
        x = m_signal(s)
        rc, blob, st = O.c5_compress(x)
        assert rc == 0, (name, rc)
        ref[name] = (x, blob, st)
    return ref


def m_frame_of(blob, st):
    """The M frame inside the oracle's blob: [u64 cK][K][u64 cS][S][u64 cM][M]..."""
    k = 8 + int(st[5]) + 8 + int(st[6]) + 8
    return blob[k:k + int(st[7])]
