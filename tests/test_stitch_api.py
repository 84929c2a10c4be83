"""Model output back to reads (pgn_stitch_plan_device / pgn_stitch_rows_device): the C ABI surface, the
refusals and the rule itself, without a GPU.

The rule (include/pgnano_hip.h), for a taken read of k segments with starts a_j (from the first one's) and a
model of stride s, T = L / s frames per row:
  cut points  c_j = a_{j+1} + floor((a_j + L - a_{j+1}) / 2) for j < k-1, c_{k-1} = a_{k-1} + valid_{k-1}, c_{-1} = 0
  kept        frame f of segment j iff c_{j-1} <= a_j + f*s < c_j:
              first_j = ceil((c_{j-1} - a_j) / s), end_j = min(T, ceil((c_j - a_j) / s)), count_j = max(0, end_j - first_j)
ref_plan below is that text with Python integers, one segment at a time; stitch_plan_signal (the package's
numpy form, which the GPU tests compare the device with) must agree with it everywhere.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _oracle as O
from test_segment_api import ref_segments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN, ROWS = "pgn_stitch_plan_device", "pgn_stitch_rows_device"
BAD_PARAMS = [(8, 0, 0), (0, 0, 1), (8, 0, 3), (8, 5, 4), (8, 8, 1), (8, 9, 1), ((1 << 24) + 4, 0, 4)]  # (L, V, s)
OK_PARAMS = [(8, 0, 8), (8, 4, 4), (40, 8, 4), (40, 7, 4), (48, 12, 6), (1 << 24, 0, 1), (8, 7, 1)]


def ceil_div(a, b):
    return -(-a // b)


def ref_plan(segs, L, s):
    """[(first, count)] of a read's segments [(start, valid)], by the header's text."""
    T = L // s
    k = len(segs)
    a = [st - segs[0][0] for st, _ in segs]
    out = []
    for j in range(k):
        c_prev = 0 if j == 0 else a[j] + (a[j - 1] + L - a[j]) // 2
        c = a[j] + segs[j][1] if j == k - 1 else a[j + 1] + (a[j] + L - a[j + 1]) // 2
        first = ceil_div(c_prev - a[j], s)
        end = min(T, ceil_div(c - a[j], s))
        out.append((first, max(0, end - first)))
    return out


def sweep(seed, n):
    """Random (m, L, V, s) within the constraints, short and long reads alike."""
    rng = np.random.default_rng(seed)
    for _ in range(n):
        s = int(rng.integers(1, 13))
        T = int(rng.integers(1, 41))
        L = s * T
        V = int(rng.integers(0, L - s + 1))
        m = int(rng.integers(0, 7 * L + 1)) if rng.integers(0, 4) else int(rng.integers(0, 40 * L + 1))
        yield m, L, V, s


# ---- surface -------------------------------------------------------------------------------------
def _header():
    src = open(os.path.join(ROOT, "include", "pgnano_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_symbols_declared_exported_and_bound():
    from rawnanoporesignalcompression_amd import _native

    lib = _native.load()
    sigs = {s[0]: s for s in _native.SIGNATURES}
    for name, nargs in ((PLAN, 9), (ROWS, 13)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", _header())
        assert hasattr(lib, name)
        assert sigs[name][1] is C.c_int and len(sigs[name][2]) == nargs


def test_the_header_carries_the_rule():
    src = open(os.path.join(ROOT, "include", "pgnano_hip.h")).read()
    for text in ("c_j     = a_{j+1} + floor((a_j + L - a_{j+1}) / 2)", "first_j = ceil((c_{j-1} - a_j) / s)",
                 "end_j   = min(T, ceil((c_j - a_j) / s))", "count_j = max(0, end_j - first_j)"):
        assert text in src, text


def test_struct_layouts():
    from rawnanoporesignalcompression_amd import StitchTable, _native

    code = _header()
    for name in ("pgn_stitch_params", "pgn_stitch_segment"):
        assert re.search(r"typedef struct " + name + r" \{", code)
    N = _native
    assert [C.sizeof(S) for S in (N.StitchParams, N.StitchSegment)] == [16, 16]
    offsets = lambda S: [(f, getattr(S, f).offset) for f, _ in S._fields_]
    assert offsets(N.StitchParams) == [("length", 0), ("overlap", 4), ("frame_samples", 8), ("pad", 12)]
    assert offsets(N.StitchSegment) == [("dst_frame", 0), ("first", 8), ("count", 12)]
    D = StitchTable.DTYPE
    assert D.itemsize == 16
    assert [D.fields[f][1] for f, _ in N.StitchSegment._fields_] == [0, 8, 12]


def test_plan_call_refusals():
    """Every refusal is PGN_ERR_INVALID_ARG with dummy pointers: nothing is dereferenced and no device is
    touched (this runs without one)."""
    from rawnanoporesignalcompression_amd import _native

    fn = getattr(_native.load(), PLAN)
    bad = _native.PGN_ERR_INVALID_ARG
    dummy = C.c_void_p(0x1000)
    ok = _native.StitchParams(40, 8, 4, 0)

    def call(ctx=dummy, nreads=1, reads=dummy, segments=dummy, capacity=5, p=ok, plan=dummy, frames=dummy):
        return fn(ctx, nreads, reads, segments, capacity, C.byref(p) if p is not None else None, plan, frames, None)

    assert call(ctx=None) == bad
    assert call(p=None) == bad
    for L, V, s in BAD_PARAMS:
        assert call(p=_native.StitchParams(L, V, s, 0)) == bad, (L, V, s)
    assert call(frames=None) == bad
    assert call(frames=None, nreads=0) == bad
    for missing in ("reads", "segments", "plan"):
        assert call(**{missing: None}) == bad, missing
    assert call(reads=None, capacity=0, segments=None, plan=None) == bad  # d_reads is needed at any capacity
    assert call(nreads=1 << 32) == bad
    assert call(capacity=1 << 40) == bad


def test_rows_call_refusals_and_their_order():
    """The refusals, and what the order of the checks lets through: with no segments the call returns PGN_OK
    after the parameter and frame checks and before it looks at an array; with segments and no room in the
    output it returns PGN_OK after the array check.  A dummy context is never dereferenced on these paths."""
    from rawnanoporesignalcompression_amd import _native

    fn = getattr(_native.load(), ROWS)
    bad, fine = _native.PGN_ERR_INVALID_ARG, _native.PGN_OK
    dummy = C.c_void_p(0x1000)
    ok = _native.StitchParams(40, 8, 4, 0)

    def call(ctx=dummy, p=ok, plan=dummy, nseg=3, rows=dummy, row_stride=160, frame_stride=16, frame_bytes=16,
             out=dummy, cap=0):
        return fn(ctx, C.byref(p) if p is not None else None, plan, 0, nseg, rows, row_stride, frame_stride, frame_bytes,
                  out, 0, cap, None)

    assert call(ctx=None) == bad
    assert call(p=None) == bad
    for L, V, s in BAD_PARAMS:
        assert call(p=_native.StitchParams(L, V, s, 0)) == bad, (L, V, s)
    for L, V, s in OK_PARAMS:
        assert call(p=_native.StitchParams(L, V, s, 0), frame_stride=1 << 20) == fine, (L, V, s)
    assert call(frame_bytes=0) == bad
    assert call(frame_bytes=0, nseg=0) == bad          # the frame checks come before the empty batch
    assert call(frame_stride=15) == bad
    assert call(frame_stride=15, nseg=0) == bad
    one = _native.StitchParams(8, 0, 8, 0)             # T == 1: the frame stride is never used
    assert call(p=one, frame_stride=0) == fine
    for missing in ("plan", "rows", "out"):
        assert call(**{missing: None}) == bad, missing
        assert call(**{missing: None}, nseg=0) == fine, missing   # an empty batch needs no array
    assert call(ctx=None, nseg=0) == bad
    assert call() == fine and call(nseg=0) == fine


def test_python_parameter_helpers():
    from rawnanoporesignalcompression_amd import stitch_bound, stitch_params, stitch_plan_signal

    for L, V, s in BAD_PARAMS + [(8, -1, 1)]:
        with pytest.raises(ValueError):
            stitch_params(L, V, s)
        with pytest.raises(ValueError):
            stitch_plan_signal(100, L, V, s)
    for L, V, s in OK_PARAMS:
        p = stitch_params(L, V, s)
        assert (p.length, p.overlap, p.frame_samples, p.pad) == (L, V, s, 0)
    assert stitch_plan_signal(0, 40, 8, 4).shape == (0, 2)
    assert stitch_plan_signal([], 40, 8, 4).shape == (0, 2)
    assert stitch_bound([], 40, 8, 4) == 0
    assert stitch_bound([0, 1, 40, 41], 40, 8, 4) == (0 + 1 + 10 + 11) + (0 + 1 + 1 + 2)


# ---- the rule --------------------------------------------------------------------------------------
def test_numpy_rule_is_the_headers_text():
    """stitch_plan_signal against ref_plan, from a length and from table rows whose starts include a trim."""
    from rawnanoporesignalcompression_amd import stitch_plan_signal

    for i, (m, L, V, s) in enumerate(sweep(11, 4000)):
        segs = ref_segments(m, L, V)
        want = ref_plan(segs, L, s) if segs else []
        got = stitch_plan_signal(m, L, V, s)
        assert got.dtype == np.int64 and got.tolist() == [list(w) for w in want], (m, L, V, s)
        if segs and i % 4 == 0:
            moved = np.array([(st + 77, v) for st, v in segs], np.uint32)  # the table's own type
            assert np.array_equal(stitch_plan_signal(moved, L, V, s), got), (m, L, V, s)


@pytest.mark.skipif(not os.path.exists(O.MODEL_SO), reason="libpgn_model.so not built")
def test_host_build_of_the_kernels_rule():
    """kept_frames, the function the plan kernel runs per table row, in its host build (libpgn_model.so)
    against the numpy rule, from uint32 table columns whose starts include a trim."""
    from rawnanoporesignalcompression_amd import _native, stitch_plan_signal

    lib = O.model()
    lib.pgnm_stitch_frames.restype = C.c_int
    lib.pgnm_stitch_frames.argtypes = [C.c_void_p, C.c_uint64] + [C.c_void_p] * 4
    for m, L, V, s in sweep(13, 3000):
        segs = ref_segments(m, L, V)
        k = len(segs)
        start = np.array([st + 123 for st, _ in segs], np.uint32)
        valid = np.array([v for _, v in segs], np.uint32)
        first, count = np.full(k, 99, np.uint32), np.full(k, 99, np.uint32)
        prm = _native.StitchParams(L, V, s, 0)
        assert lib.pgnm_stitch_frames(C.byref(prm), k, start.ctypes.data, valid.ctypes.data, first.ctypes.data,
                                      count.ctypes.data) == 0
        assert np.array_equal(np.stack([first, count], 1).astype(np.int64), stitch_plan_signal(m, L, V, s)), (m, L, V, s)
    for L, V, s in BAD_PARAMS:
        assert lib.pgnm_stitch_frames(C.byref(_native.StitchParams(L, V, s, 0)), 0, None, None, None, None) == -1


def test_rule_properties():
    """Over a seeded random sweep: the kept frames' first samples rise strictly and lie in [0, m); the frame
    count is within k - 1 of ceil(m / s); it is bounded by ceil(n / s) + segments(n) for untrimmed lengths
    n >= m, which is what stitch_bound adds up."""
    from rawnanoporesignalcompression_amd import stitch_bound, stitch_plan_signal

    rng = np.random.default_rng(5)
    multi = 0
    for m, L, V, s in sweep(12, 8000):
        segs = ref_segments(m, L, V)
        plan = stitch_plan_signal(m, L, V, s)
        k = len(segs)
        assert plan.shape == (k, 2)
        T = L // s
        assert (plan[:, 0] >= 0).all() and (plan[:, 0] + plan[:, 1] <= T).all()
        frames = int(plan[:, 1].sum())
        if k == 0:
            assert frames == 0
            continue
        multi += k > 2
        pos = np.concatenate([segs[j][0] + s * np.arange(f, f + c) for j, (f, c) in enumerate(plan.tolist())])
        assert pos.size == frames and (np.diff(pos) > 0).all(), (m, L, V, s)
        assert pos[0] >= 0 and pos[-1] < m, (m, L, V, s)
        assert abs(frames - ceil_div(m, s)) <= k - 1, (m, L, V, s, frames)
        for n in (m, m + int(rng.integers(0, 3 * L))):
            assert frames <= ceil_div(n, s) + len(ref_segments(n, L, V)), (m, n, L, V, s)
            assert frames <= stitch_bound([n], L, V, s)
    assert multi > 2000


def test_without_the_stride_constraint_coverage_breaks():
    """Why s <= L - V is required: with s > L - V a segment can own less than one frame, and the kept frames
    of such a read no longer come within k - 1 of ceil(m / s)."""
    L, V, s = 8, 7, 4  # S = 1 < s
    segs = ref_segments(40, L, V)
    frames = sum(c for _, c in ref_plan(segs, L, s))
    assert len(segs) == 33 and frames <= ceil_div(40, s) + len(segs)
    assert any(c == 0 for _, c in ref_plan(segs, L, s))


@pytest.mark.parametrize("L,V,s", [(8, 0, 8), (8, 4, 2), (40, 8, 4), (48, 12, 6), (10000, 500, 5), (64, 0, 1)])
def test_regular_case_closed_form(L, V, s):
    """2s | V, s | L - V and a read that ends on the segment grid: h = V / (2s) frames go on each side of
    every joint and frames_r = ceil(m / s).  A read of at most L samples keeps [0, ceil(m / s))."""
    from rawnanoporesignalcompression_amd import stitch_plan_signal

    S, T, h = L - V, L // s, V // (2 * s)
    assert V % (2 * s) == 0 and S % s == 0
    for k in (2, 3, 7):
        m = L + (k - 1) * S
        plan = stitch_plan_signal(m, L, V, s).tolist()
        want = [[0 if j == 0 else h, T - (0 if j == 0 else h) - (0 if j == k - 1 else h)] for j in range(k)]
        assert plan == want, (k, plan)
        assert sum(c for _, c in plan) == ceil_div(m, s)
    for m in (1, s, L - 1, L):
        assert stitch_plan_signal(m, L, V, s).tolist() == [[0, ceil_div(m, s)]]


def test_bound_covers_trimmed_reads():
    """stitch_bound of the untrimmed lengths against the rule's total for every trim of them."""
    from rawnanoporesignalcompression_amd import stitch_bound, stitch_plan_signal

    rng = np.random.default_rng(9)
    for L, V, s in ((8, 4, 4), (40, 7, 4), (48, 12, 6)):
        counts = rng.integers(0, 12 * L, 300)
        trims = np.minimum(rng.integers(0, 3 * L, 300), counts)
        total = sum(int(stitch_plan_signal(int(n - t), L, V, s)[:, 1].sum()) for n, t in zip(counts, trims))
        assert total <= stitch_bound(counts, L, V, s)
        assert stitch_bound(counts, L, V, s) == sum(ceil_div(int(n), s) + len(ref_segments(int(n), L, V)) for n in counts)
