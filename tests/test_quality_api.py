"""Posteriors and qualities (pgn_crf_posterior_rows_device, pgn_base_qual_device): the C ABI surface, the refusals
and the two numpy models, without a GPU.

The float64 model of the posteriors is held to a brute-force sum over all paths of tiny rows, which uses nothing of
the recursions: every path is a start state and a stay or one of four moves per frame, its weight is the exponential
of its scores' sum, and post[t][b] is the weight of the paths whose state after frame t ends in base b over the
weight of all.  The float32 model is held to the float64 one; the quality rule to blocks built for its threshold's
edges.
"""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POST, QUAL = "pgn_crf_posterior_rows_device", "pgn_base_qual_device"
NAN, INF = float("nan"), float("inf")


def _header(comments=False):
    src = open(os.path.join(ROOT, "include", "pgnano_hip.h")).read()
    return src if comments else re.sub(r"/\*.*?\*/", "", src, flags=re.S)


# ---- surface -------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_bound():
    import rawnanoporesignalcompression_amd as pkg
    from rawnanoporesignalcompression_amd import _native, host, quality

    lib = _native.load()
    sigs = {s[0]: s for s in _native.SIGNATURES}
    for name, nargs in ((POST, 10), (QUAL, 14)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", _header())
        assert hasattr(lib, name)
        assert sigs[name][1] is C.c_int and len(sigs[name][2]) == nargs
    for name in ("crf_posteriors", "base_qual", "crf_posteriors_signal", "base_qual_signal", "qual_thresholds"):
        assert name in quality.__all__ and callable(getattr(quality, name))
        assert name not in pkg.__all__                      # the package's own surface stays as it is
    for name in ("crf_posteriors_signal", "base_qual_signal", "qual_thresholds"):
        assert getattr(quality, name) is getattr(host, name)
    for attr in ("crf_posteriors", "base_qual"):
        assert not hasattr(pkg.PGNanoCodec, attr)


def test_struct_layout():
    from rawnanoporesignalcompression_amd import _native

    m = re.search(r"typedef struct pgn_qual_params \{([^}]*)\}", _header())
    assert m and re.findall(r"(\w+)\s+(\w+)(?:\[(\d+)\])?;", m.group(1)) == [("uint32_t", "q_min", ""),
                                                                          ("uint32_t", "nthresholds", ""),
                                                                          ("uint32_t", "thr", "93")]
    S = _native.QualParams
    assert C.sizeof(S) == 4 * 95
    assert [(f, getattr(S, f).offset) for f, _ in S._fields_] == [("q_min", 0), ("nthresholds", 4), ("thr", 8)]


def test_the_header_carries_the_rules():
    src = re.sub(r"\s*\n \*\s*", " ", _header(comments=True))
    for text in ("Posteriors and qualities (CRF)",
                 "c(u, n) = ((u << 2) | n) & (S - 1)", "top(u) = u >> (2k - 2)",
                 "a_{t+1}[s] = log( exp(a_t[s] + stay(t, s)) + sum_b exp(a_t[p(s, b)] + move(t, s, b)) ).",
                 "b_t[u] = log( exp(stay(t, u) + b_{t+1}[u]) + sum_n exp(move(t, c(u, n), top(u)) + b_{t+1}[c(u, n)]) ).",
                 "g_t[s] = exp(a_{t+1}[s] + b_{t+1}[s]) / sum_s' exp(a_{t+1}[s'] + b_{t+1}[s']).",
                 "post[t][b] = sum over s with (s & 3) == b of g_t[s]",
                 "bytes per row = 4 * S * T",
                 "the default cap holds 131 rows",
                 "err_t = (post[t][(c+1)&3] + post[t][(c+2)&3]) + post[t][(c+3)&3]",
                 "qual[g] = 33 + q_min + #{ j < nthresholds : U <= (uint64)thr[j] * n }.",
                 "Not covered: beam search; a row's log partition function; per-read mean quality; bfloat16; alphabets "
                 "other than 4 bases; qualities for the CTC path"):
        assert text in src, text
    for path in ("README.md", "DESIGN.md"):
        text = re.sub(r"\s+", " ", open(os.path.join(ROOT, path)).read())
        assert "Qualities" in text and "crf_posteriors" in text and "base_qual" in text and "131 rows" in text, path


# ---- the refusals, made before any GPU call ----------------------------------------------------------------------
def _crf(state_len=1, transitions=5, score_type=2, stay_score=0.0):
    from rawnanoporesignalcompression_amd import _native

    return _native.CrfParams(state_len, transitions, score_type, stay_score)


BAD_CRF = [(0, 5, 2, 0.0), (6, 5, 2, 0.0), (3, 3, 2, 0.0), (3, 6, 2, 0.0), (3, 5, 0, 0.0), (3, 5, 3, 0.0),
           (3, 5, 2, 1.0), (3, 5, 2, -0.0), (3, 5, 1, 0.5)]


def test_posterior_call_refusals_and_their_order():
    """The Viterbi call's refusals in its order, with dummy pointers: nothing is dereferenced and no device is
    touched.  The scratch cap reads the context, so it and the PGN_OK of nrows == 0 behind it are shown on the
    device (tests/test_gpu_crf_post.py)."""
    from rawnanoporesignalcompression_amd import _native

    fn = getattr(_native.load(), POST)
    bad = _native.PGN_ERR_INVALID_ARG
    dummy = C.c_void_p(0x1000)

    # k = 1, 5 transitions, float16: C = 20, a frame is 40 bytes
    def call(ctx=dummy, p=_crf(), nrows=2, T=8, rows=dummy, rstride=320, fstride=40, post=dummy, pstride=32):
        return fn(ctx, C.byref(p) if p is not None else None, nrows, T, rows, rstride, fstride, post, pstride, None)

    empty = dict(nrows=0, rows=None, post=None)
    assert call(ctx=None) == bad
    assert call(p=None) == bad
    assert call(ctx=None, **empty) == bad
    for prm in BAD_CRF:
        assert call(p=_crf(*prm)) == bad, prm
        assert call(p=_crf(*prm), **empty) == bad, prm
    assert call(T=0) == bad
    assert call(T=(1 << 24) + 1, pstride=1 << 27) == bad
    assert call(T=0, **empty) == bad
    assert call(fstride=38) == bad
    assert call(fstride=41) == bad
    assert call(rstride=321) == bad
    assert call(rows=C.c_void_p(0x1001)) == bad
    assert call(p=_crf(score_type=1), fstride=76, rstride=640) == bad
    assert call(p=_crf(score_type=1), fstride=80, rstride=640, rows=C.c_void_p(0x1002)) == bad
    assert call(p=_crf(transitions=4, stay_score=0.5), fstride=30, rstride=320) == bad
    assert call(fstride=38, **empty) == bad
    assert call(fstride=0, T=2, pstride=8) == bad
    assert call(pstride=31) == bad                             # below 4 * T with two rows
    assert call(pstride=31, nrows=1 << 32) == bad
    assert call(post=C.c_void_p(0x1002)) == bad                # d_post is 4-byte aligned
    assert call(**dict(empty, post=C.c_void_p(0x1002))) == bad
    assert call(nrows=1 << 32) == bad
    assert call(rows=None) == bad
    assert call(post=None) == bad
    assert call(nrows=1, post=None, pstride=0) == bad
    assert call(ctx=None, p=_crf(*BAD_CRF[0]), T=0, fstride=1, pstride=0, nrows=1 << 32, rows=None, post=None) == bad


def _qual(q_min=1, thr=(300, 200, 200, 5)):
    from rawnanoporesignalcompression_amd import _native

    p = _native.QualParams(q_min, len(thr))
    p.thr[:len(thr)] = list(thr)
    return p


def test_qual_call_refusals():
    from rawnanoporesignalcompression_amd import _native

    fn = getattr(_native.load(), QUAL)
    bad = _native.PGN_ERR_INVALID_ARG
    dummy = C.c_void_p(0x1000)

    def call(ctx=dummy, p=_qual(), nreads=2, rf=dummy, codes=dummy, post=dummy, fbase=0, fcap=10, rb=dummy, bf=dummy,
             st=dummy, qual=dummy, bcap=10):
        return fn(ctx, C.byref(p) if p is not None else None, nreads, rf, codes, post, fbase, fcap, rb, bf, st, qual, bcap,
                  None)

    assert call(ctx=None) == bad
    assert call(p=None) == bad
    assert call(p=_qual(94, ())) == bad                        # q_min + nthresholds <= 93
    assert call(p=_qual(90, (4, 3, 2, 1))) == bad
    assert call(p=_qual(1, (5, 6))) == bad                     # non-increasing
    assert call(p=_qual(1, (9, 9, 8, 9))) == bad
    over = _qual(0, ())
    over.nthresholds = 94
    assert call(p=over) == bad
    assert call(nreads=1 << 32) == bad
    assert call(fcap=1 << 40) == bad
    assert call(post=C.c_void_p(0x1002)) == bad
    for name in ("rf", "rb", "st", "codes", "post", "bf", "qual"):
        assert call(**{name: None}) == bad, name
    # nothing to do: PGN_OK without a look at the context or at any array
    assert call(nreads=0, rf=None, rb=None, st=None) == 0
    assert call(p=_qual(0, tuple(range(93, 0, -1))), nreads=0) == 0
    assert call(p=_qual(93, ()), nreads=0) == 0
    assert call(ctx=None, nreads=0) == bad
    # an empty window and no room for bases need no arrays, but the reads' three do not go away
    assert call(fcap=0, codes=None, post=None, bcap=0, bf=None, qual=None, nreads=0) == 0
    assert call(fcap=0, codes=None, post=None, bcap=0, bf=None, qual=None, rf=None) == bad


# ---- the posteriors ---------------------------------------------------------------------------------------------
def brute_force(x, k, tr, stay):
    """post [T, 4] of one row by the sum over all paths, in float64."""
    T, S = len(x), 4 ** k
    x = np.asarray(x, np.float64)
    weight = np.zeros((T, 4))
    for s0 in range(S):
        for choices in itertools.product(range(5), repeat=T):   # 0 stays, 1 + n appends base n
            s, total, ends = s0, 0.0, []
            for t, ch in enumerate(choices):
                if ch == 0:
                    total += x[t, 5 * s] if tr == 5 else stay
                else:
                    b, s = s >> (2 * k - 2), ((s << 2) | (ch - 1)) & (S - 1)   # the move drops b: p(s', b) = s
                    total += x[t, tr * s + tr - 4 + b]
                ends.append(s & 3)
            w = np.exp(total)
            for t, e in enumerate(ends):
                weight[t, e] += w
    return weight / weight.sum(1, keepdims=True)


@pytest.mark.parametrize("k,T,tr", [(1, 4, 5), (1, 4, 4), (2, 2, 5), (2, 2, 4)])
def test_float64_model_against_all_paths(k, T, tr):
    from rawnanoporesignalcompression_amd.quality import crf_posteriors_signal

    rng = np.random.default_rng(10 * k + tr)
    stay = 0.0 if tr == 5 else -0.5
    for dtype in (np.float32, np.float16):
        x = (rng.standard_normal((T, tr * 4 ** k)) * 2).astype(dtype)
        got = crf_posteriors_signal(x, k, tr, stay)
        assert got.dtype == np.float64 and got.shape == (T, 4)
        assert np.abs(got - brute_force(x, k, tr, stay)).max() <= 1e-12


def test_p_and_the_score_layout_by_a_planted_path():
    """k = 2: a path planted at +8 through known states; the marginal of each frame's newest base is nearly one."""
    from rawnanoporesignalcompression_amd.quality import crf_posteriors_signal

    rng = np.random.default_rng(3)
    k, S, T = 2, 16, 12
    for tr in (5, 4):
        x = -(rng.random((T, tr * S)) * 0.99 + 0.01)
        s, newest = 6, []
        for t in range(T):
            if t % 3 == 0 and tr == 5:
                x[t, 5 * s] = 8
            else:
                b, s = s >> 2, ((s << 2) & 15) | int(rng.integers(0, 4))
                x[t, tr * s + tr - 4 + b] = 8
            newest.append(s & 3)
        post = crf_posteriors_signal(x.astype(np.float32), k, tr, 0.0)
        assert (post[np.arange(T), newest] > 1 - 1e-2).all(), tr


def test_rows_sum_to_one_and_float32_follows_float64():
    from rawnanoporesignalcompression_amd.quality import crf_posteriors_signal

    rng = np.random.default_rng(8)
    for k, tr, T in ((1, 5, 300), (2, 4, 50), (3, 5, 300), (4, 5, 20)):
        x = (rng.standard_normal((T, tr * 4 ** k)) * 3).astype(np.float16)
        stay = 0.0 if tr == 5 else 0.25
        p64 = crf_posteriors_signal(x, k, tr, stay)
        p32 = crf_posteriors_signal(x, k, tr, stay, dtype=np.float32)
        assert p32.dtype == np.float32 and p32.shape == p64.shape == (T, 4)
        assert np.abs(p64.sum(1) - 1).max() <= 1e-12 and (p64 >= 0).all()
        assert np.abs(p32.sum(1, dtype=np.float64) - 1).max() <= 1e-6
        # the renormalised float32 pass: a few units of float32's precision relative to the probability, at any T
        assert (np.abs(p32 - p64) / np.maximum(p64, 1e-6)).max() <= 5e-5, (k, T)
    for args in ((np.zeros(20, np.float16), 1), (np.zeros((2, 21), np.float16), 1), (np.zeros((0, 20), np.float16), 1),
                 (np.zeros((2, 20), np.float16), 2)):
        with pytest.raises(ValueError):
            crf_posteriors_signal(*args)
    with pytest.raises(ValueError):
        crf_posteriors_signal(np.zeros((2, 20), np.float16), 1, dtype=np.float16)


# ---- the qualities ----------------------------------------------------------------------------------------------
def test_thresholds():
    from rawnanoporesignalcompression_amd.quality import qual_params, qual_thresholds

    thr = qual_thresholds()
    assert thr.dtype == np.uint32 and len(thr) == 49
    assert int(thr[0]) == 3040603991 and int(thr[-1]) == 48190
    assert (np.diff(thr.astype(np.int64)) < 0).all()
    # thr[j] is where q = -10 log10(err) rounds up to q_min + j + 1
    for j in (0, 10, 48):
        q = -10 * np.log10((int(thr[j]) + np.array([0.0, 1.0])) / 2.0 ** 32)
        assert q[0] >= 1 + j + 0.5 > q[1]
    scaled = qual_thresholds(q_scale=0.9, q_shift=-0.2, q_min=2, q_max=40)
    assert len(scaled) == 38 and (np.diff(scaled.astype(np.int64)) <= 0).all()
    assert int(qual_thresholds(q_shift=60.0)[0]) == 0xFFFFFFFF           # clamped to uint32
    p = qual_params()
    assert (p.q_min, p.nthresholds) == (1, 49) and list(p.thr[:49]) == thr.tolist()
    p = qual_params([7, 7, 3], q_min=0)
    assert (p.q_min, p.nthresholds, list(p.thr[:3])) == (0, 3, [7, 7, 3])
    for args in (([3, 4], 1), ([1] * 93, 1), ([[1]], 1), ([-1], 1), ([1 << 32], 1)):
        with pytest.raises(ValueError):
            qual_params(*args)
    with pytest.raises(ValueError):
        qual_thresholds(q_min=3, q_max=2)


def frames_with_sum(total, n, c):
    """[n, 4] float32 whose error integers for the called base c sum to exactly `total`: every frame carries
    total // n, the first total % n of them one more, as err = v / 2^32 with v below 2^24 (exact in float32)."""
    assert total // n + 1 < 1 << 24
    post = np.zeros((n, 4), np.float32)
    v = np.full(n, total // n, np.int64)
    v[:total % n] += 1
    post[:, (c + 2) & 3] = (v.astype(np.float64) / 2.0 ** 32).astype(np.float32)
    post[:, c] = 1.0
    return post


def test_rule_at_the_threshold_edges():
    """Blocks whose U is exactly thr[j] * n, one below and one above, for one frame and for many."""
    from rawnanoporesignalcompression_amd.quality import base_qual_signal

    thr = np.array([5_000_000, 70_000, 70_000, 900, 0], np.uint32)
    for n in (1, 3, 64, 65, 700):
        for j, step in ((0, 1), (1, 2), (3, 1)):      # the doubled threshold counts twice
            blocks = [(int(thr[j]) * n + d, n) for d in (0, -1, 1)]
            codes = np.zeros(0, np.uint8)
            post = np.zeros((0, 4), np.float32)
            at = []
            for g, (total, m) in enumerate(blocks):
                c = g % 4
                at.append(len(codes))
                codes = np.concatenate([codes, np.full(m, c | 0x80, np.uint8)[:1], np.full(m - 1, (c + 1) & 3, np.uint8)])
                post = np.concatenate([post, frames_with_sum(total, m, c)])
            q = base_qual_signal(codes, post, at, len(codes), thr, 2)
            below = 33 + 2 + j + step                   # thresholds 0..j admit (and j's double, if any)
            assert q.tolist() == [below, below, below - step], (n, j, q)


def test_rule_specials():
    from rawnanoporesignalcompression_amd.quality import base_qual_signal, qual_thresholds

    thr = qual_thresholds()
    post = np.array([[0.25, 0.25, 0.25, 0.25],       # err 0.75 for any base: below q 1.5, so q_min
                     [1.0, 0.0, 0.0, 0.0],           # err 0: every threshold admits
                     [NAN, 0.0, 0.0, 0.0],           # called base NaN: not part of the sum
                     [0.5, NAN, 0.0, 0.0],           # a NaN error counts as 2^32 - 1
                     [1.0, -0.5, 0.25, 0.0],         # a negative sum clamps to 0
                     [0.0, 2.0, 2.0, 2.0],           # above one clamps to 2^32 - 1
                     [0.0, INF, -INF, 0.0],          # inf - inf is NaN
                     [0.9, 1e-3, 0.0, 0.0]], np.float32)
    codes = np.full(len(post), 0x80, np.uint8)
    q = base_qual_signal(codes, post, np.arange(len(post)), len(post), thr, 1)
    assert q.tolist() == [34, 83, 83, 34, 83, 34, 34, 33 + 30]
    # frames before the first base belong to no base, and the block's base is the code of its first frame
    codes = np.array([1, 1, 0x82, 3, 3, 0x82], np.uint8)
    post = np.zeros((6, 4), np.float32)
    post[:, 2] = 1
    post[:2] = 0.25
    post[3, 3], post[3, 2] = 0.5, 0.5                # the frame's own label is 3, the block's base is 2
    q = base_qual_signal(codes, post, [2, 5], 6, thr, 1)
    assert q.tolist() == [33 + 8, 83]                # mean error 0.5 / 3: q = 7.78 rounds to 8
    assert base_qual_signal(np.zeros(4, np.uint8), np.zeros((4, 4), np.float32), [], 4, thr, 1).tolist() == []
