"""Byte streams for the on-chip search of small single-block frames (csrc/pgn_zenc.h small_search_wave,
host model csrc/zstd1_model.h small_search_serial through model_capi.hip z1m_small_search): the
generators of _search_cases.py at the lengths around a round, a table and the bound, the Lhigh streams
of bench reads, and streams built for the search's own hazards.  Every byte is at most 253, so each
stream can be carried as the Lhigh stream of a C5 chunk (lhigh_signal).  Seeds are fixed.  Shared by
test_small_search_model.py (CPU: model against the serial search) and test_gpu_small_search.py (GPU:
byte equality with the oracle)."""
import ctypes as C
import functools

import numpy as np

import _oracle as O
import _search_cases as S

INFO = ("small", "overflow", "nbseq", "last_ll", "rep0", "rep1", "rounds", "log_entries", "flagged", "refuted", "scans",
        "refuted_absent", "shadowed", "fp_then_hit", "rep_first")


@functools.lru_cache(maxsize=None)
def _model():
    M = O.model()
    M.z1m_small_search.restype = C.c_size_t
    M.z1m_small_search.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    M.z1m_small_search_bytes.restype = C.c_uint
    M.z1m_small_search_log_cap.restype = C.c_uint
    return M


def search(make, want, tries=400):
    """First stream of make(rng) over a fixed seed sequence for which want(stream) holds."""
    for seed in range(tries):
        s = make(np.random.default_rng(1000 + seed))
        if want(s):
            return s
    raise AssertionError("no seed gives the case")


def small_bytes() -> int:
    """kSmallSearchBytes: the largest block the small search takes."""
    return int(_model().z1m_small_search_bytes())


def log_cap() -> int:
    return int(_model().z1m_small_search_log_cap())


def run(stream, mode):
    """(sequences [nbSeq, 3], info dict) of the stream's search: mode 0 fast_search_serial, mode 1 the
    encoder's dispatch (the small search, or the general one beyond the bound and after an overflow)."""
    a = np.ascontiguousarray(np.frombuffer(bytes(stream), np.uint8))
    out = np.zeros((a.size // 4 + 2, 3), np.uint32)
    info = np.zeros(len(INFO), np.uint32)
    nb = _model().z1m_small_search(a.ctypes.data, a.size, mode, out.ctypes.data, out.shape[0], info.ctypes.data)
    assert nb <= out.shape[0]
    return out[:nb].copy(), dict(zip(INFO, (int(v) for v in info)))


def fold(stream) -> bytes:
    """Bytes 254 and 255 moved down (an Lhigh byte is at most 254, and 254 limits the low byte)."""
    a = np.frombuffer(bytes(stream), np.uint8).copy()
    a[a >= 254] -= 128
    return a.tobytes()


def lhigh_signal(stream: bytes, seed: int) -> np.ndarray:
    """The int16 signal whose every sample is of class 3 with `stream` as the Lhigh stream and random
    low bytes: v = 273 + (high << 8 | low) is the zig-zag of the sample's delta.  The low bytes are
    random over 64 values, not 256: with an incompressible Lhigh stream beside an incompressible Llow
    stream the chunk outgrows the plugin's output bound (2 n + 26) and the oracle refuses it; Llow stays
    a noise stream."""
    hi = np.frombuffer(stream, np.uint8).astype(np.int64)
    assert hi.max(initial=0) <= 253
    lo = np.random.default_rng(seed).integers(0, 64, hi.size)
    v = 273 + (hi << 8) + lo
    d = np.where(v & 1, -((v + 1) >> 1), v >> 1)  # inverse zig-zag
    return (np.cumsum(d) & 0xFFFF).astype(np.uint16).view(np.int16)


def lengths():
    K = small_bytes()
    return (8, 9, 16, 63, 64, 65, 255, 256, 257, 1151, K - 1, K)


GENERATORS = dict(S.GENERATORS, noise=lambda rng, n: S.noise(rng, n).tobytes())
N_BENCH_READS = 50
N_RUNS = 1151     # the size of a bench read's Lhigh stream, about
N_DIRECTED = 700  # built streams: noise around the planted matches, whose writes must still fit the log


# ---- directed streams -------------------------------------------------------------------------------
def lane_hits(rng, lane):
    """_search_cases.lane_hits in a small block: first hits at visit k of a chain, k % 64 == lane, with
    the source at an earlier visit of an earlier round or (lanes 62, 63) of the same."""
    n = N_DIRECTED
    a = S.noise64(rng, n)
    anchor, first = 0, True
    for i, m in enumerate((1, 1, 1, 1, 1) if lane == 0 else (0, 1, 0, 1, 0)):
        k = lane + 64 * m
        pos = S.visit_positions(anchor, first)
        j = int(rng.integers(64 * m, k - 2)) if lane and (m == 0 or i % 2) else int(rng.integers(2, max(3, 64 * m)))
        second = int(rng.integers(0, 2))
        tp, sp = pos[k] + second, pos[j] + second
        ln = int(rng.integers(12, 30))
        if tp + ln + 40 > n:
            break
        S._lz_copy(a, tp, sp, ln)
        S._differ(a, tp - 1, sp - 1)
        S._differ(a, tp + ln, sp + ln)
        anchor, first = tp + ln, False
    return a.tobytes()


def _hash5(words, hlog):
    """ZSTD_hash5Ptr of little-endian words (uint64) at this hash log."""
    return ((words << np.uint64(24)) * np.uint64(889523592379)) >> np.uint64(64 - hlog)


SHADOW_A, SHADOW_B, SHADOW_C = 349, 380, 452


def shadowed(rng):
    """Two 5-byte strings A, B of one hash and different first 4 bytes: A in one round, B later in it (the
    hash's latest entry), and after a helper match, in a new round, A's 5 bytes again with another 6th
    byte.  An equal key is in the filter and in the log, but the table's entry is B's: no match there."""
    n = N_DIRECTED
    a = S.noise64(rng, n)
    a[300:340] = a[100:140]  # helper: anchor 340, every position up to 468 visited
    a[400:440] = a[150:190]  # helper: a new round from 440
    b = rng.integers(0, 64, (1 << 15, 5), dtype=np.uint8)
    h = _hash5(S._le(b), 12)  # the hash log of a frame of 1,025 .. 2,048 bytes
    order = np.argsort(h, kind="stable")
    hs = h[order]
    pairs = np.flatnonzero((hs[1:] == hs[:-1]) & (b[order[1:], :4] != b[order[:-1], :4]).any(axis=1))
    if not pairs.size:
        return a.tobytes()
    i = int(pairs[int(rng.integers(0, pairs.size))])
    A, B = b[order[i]], b[order[i + 1]]
    a[SHADOW_A:SHADOW_A + 5] = A
    a[SHADOW_B:SHADOW_B + 5] = B
    a[SHADOW_C:SHADOW_C + 5] = A
    S._differ(a, SHADOW_C + 5, SHADOW_A + 5)
    S._differ(a, SHADOW_C - 1, SHADOW_A - 1)
    return a.tobytes()


def no_match_at_shadow(stream) -> bool:
    return not any(SHADOW_C - 4 <= r[S.POS] + r[S.BACK] <= SHADOW_C + 4 for r in S.profile(stream))


def anchor_stop(rng):
    """_search_cases.anchor_stop in a small block: a second match, hit a little after the first one's
    end, extends backwards until the anchor stops it."""
    n = N_DIRECTED
    a = S.noise64(rng, n)
    s1, s2, e = 150, 320, 480 + int(rng.integers(0, 80))
    a[s2:s2 + 5] = a[s1 + 95:s1 + 100]
    a[e - 100:e] = a[s1:s1 + 100]
    a[e - 5:e + 100] = a[s2:s2 + 105]
    S._differ(a, s1 + 100, s2 + 5)
    return a.tobytes()


END_GAPS = tuple(range(9))  # the match ends at the block's last byte, and 1 .. 8 bytes before it


def end_match(rng, gap):
    """A 20-byte match that ends `gap` bytes before the block's end; a helper match ends shortly before
    it, so the visits there are dense."""
    n = N_DIRECTED
    a = S.noise64(rng, n)
    e = n - gap
    s = e - 20
    h = s - int(rng.integers(6, 20))
    a[h - 60:h] = a[200:260]
    S._differ(a, h, 260)
    src = 30 + int(rng.integers(0, 60))  # the dense first visits: every position written
    a[s:e] = a[src:src + 20]
    S._differ(a, s - 1, src - 1)
    if gap:
        S._differ(a, e, src + 20)
    return a.tobytes()


def ends_at(stream, gap) -> bool:
    r = S.profile(stream)
    return len(r) > 0 and r[-1][S.POS] + r[-1][S.MLEN] == len(stream) - gap and r[-1][S.TO_END] == (gap == 0) and \
        r[-1][S.MLEN] >= 20


def _info(stream):
    return run(stream, 1)[1]


@functools.lru_cache(maxsize=None)
def directed_cases():
    """name -> stream; each is searched for with a fixed seed sequence until the model's own bookkeeping
    (or the serial search's profile) says that the stream does what its name says."""
    c = {}
    for lane in S.LANES:
        c[f"lane/{lane}"] = search(lambda r, lane=lane: lane_hits(r, lane), lambda s, lane=lane: S._lane_count(s, lane) >= 2)
    # a key that a visit speculated past a hit left in the filter and no committed write backs, met
    # before the round's true match
    c["filter/false_positive_then_match"] = search(
        lambda r: fold(S.runs(r, N_RUNS)),
        lambda s: (lambda i: i["small"] and i["refuted_absent"] >= 1 and i["fp_then_hit"] >= 1)(_info(s)))
    c["filter/shadowed"] = search(shadowed, lambda s: _info(s)["shadowed"] >= 1 and no_match_at_shadow(s))
    c["repcode/after_match"] = search(
        lambda r: fold(S.runs(r, N_RUNS)),
        lambda s: _info(s)["small"] and (S.profile(s)[:, S.KIND] == S.POST_REP).sum() >= 3)
    c["back/anchor_stop"] = search(anchor_stop, lambda s: len(S.anchor_stopped_rows(s)) > 0)
    for g in END_GAPS:
        c[f"end/gap{g}"] = search(lambda r, g=g: end_match(r, g), lambda s, g=g: ends_at(s, g))
    return c


# ---- streams at the bound ---------------------------------------------------------------------------
# A noise-like block that fails the certificate writes more than the log holds from about 1.2 KB on (the
# generators above at 1,151 bytes and more: OVERFLOWING), and a noise block that passes it never reaches
# the exact search on the GPU.  What reaches the search's last positions in use is a stream of long
# runs, as C5's Lhigh is: these are built at kSmallSearchBytes - 1 and kSmallSearchBytes.
def long_runs(rng, n):
    """About 98 % zero bytes with single small values between them, and a few repeated short words."""
    a = np.zeros(n, np.uint8)
    k = max(2, n // 50)
    a[rng.integers(0, n, k)] = rng.integers(1, 4, k)
    for _ in range(n // 400):
        p, q = int(rng.integers(20, n - 20)), int(rng.integers(20, n - 20))
        a[p:p + 6] = rng.integers(1, 8, 6)
        a[q:q + 6] = a[p:p + 6]
    return a.tobytes()


def end_match_at_bound(rng, n, gap):
    """A block of n bytes: noise first (the dense first visits write every position), long runs, and a
    noise tail that holds a 20-byte match from the head ending `gap` bytes before the block's end."""
    a = np.frombuffer(long_runs(rng, n), np.uint8).copy()
    a[:130] = S.noise64(rng, 130)
    a[n - 150:] = S.noise64(rng, 150)
    e = n - gap
    s = e - 20
    src = 30 + int(rng.integers(0, 60))
    a[s:e] = a[src:src + 20]
    S._differ(a, s - 1, src - 1)
    if gap:
        S._differ(a, e, src + 20)
    return a.tobytes()


def bound_sizes():
    return (small_bytes() - 1, small_bytes())


@functools.lru_cache(maxsize=None)
def bound_cases():
    """name -> stream, each of kSmallSearchBytes - 1 or kSmallSearchBytes bytes, uncertified, and searched
    to its end on the small path."""
    c = {}
    for n in bound_sizes():
        for j in range(3):
            c[f"bound_runs/{n}_{j}"] = long_runs(np.random.default_rng(7300 + 3 * n + j), n)
        for g in END_GAPS:
            c[f"bound_end/{n}_gap{g}"] = search(lambda r, n=n, g=g: end_match_at_bound(r, n, g),
                                                lambda s, g=g: _info(s)["small"] and ends_at(s, g))
    return c


# the generated cases whose committed writes outrun the log (the model says so; listed, not tolerated)
OVERFLOWING = ("late_copy/1151", "late_copy/2047", "late_copy/2048", "short_period/2047", "short_period/2048",
               "word_soup/1151", "word_soup/2047", "word_soup/2048", "small_alphabet/1151", "small_alphabet/2047",
               "small_alphabet/2048", "runs/2047", "runs/2048")


@functools.lru_cache(maxsize=None)
def overflow_case():
    """A block whose committed writes outrun the log: few symbols, a match at almost every visit."""
    K = small_bytes()
    return search(lambda r: S.small_alphabet(r, K), lambda s: _info(s)["overflow"] == 1)


@functools.lru_cache(maxsize=None)
def beyond_case():
    """One byte more than the small search takes: the general search."""
    return fold(S.runs(np.random.default_rng(6100), small_bytes() + 1))


@functools.lru_cache(maxsize=None)
def bench_lhigh():
    """The Lhigh streams of the first bench reads (seed 42, 100,000 samples): about 98 % zero bytes."""
    return {f"bench_lhigh/{r}": O.c5_streams(O.synth_read(r, 100_000))[4] for r in range(N_BENCH_READS)}


@functools.lru_cache(maxsize=None)
def generated_cases():
    c = {}
    seed = 6000
    for g, make in GENERATORS.items():
        for n in lengths():
            seed += 1
            c[f"{g}/{n}"] = fold(make(np.random.default_rng(seed), n))
            assert len(c[f"{g}/{n}"]) == n
    return c


@functools.lru_cache(maxsize=None)
def cases():
    """name -> stream: everything; "overflow/...", "beyond/..." and the generated cases named in OVERFLOWING
    are those that do not end on the small path."""
    return {**generated_cases(), **bench_lhigh(), **directed_cases(), **bound_cases(), "overflow/small_alphabet": overflow_case(),
            "beyond/runs": beyond_case()}


@functools.lru_cache(maxsize=None)
def reference():
    """name -> (signal, the oracle's blob); computed once."""
    ref = {}
    for k, (name, s) in enumerate(cases().items()):
        x = lhigh_signal(s, 100 + k)
        assert O.c5_streams(x)[4] == s, name
        rc, blob, st = O.c5_compress(x)
        assert rc == 0, (name, rc)
        ref[name] = (x, blob)
    return ref
