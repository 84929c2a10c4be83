"""Model rows to per-frame codes on the GPU (PGNanoCodec.crf_viterbi over pgn_crf_viterbi_rows_device), bit for
bit against crf_viterbi_signal row by row (the numpy rule, which tests/test_crf_api.py holds to the header's
text): every output is a selection among float32 sums formed in a fixed order, so the tolerance is zero.

Most tests call the C ABI with buffers of their own: the codes and the row scores lie between canary bytes, and
the whole buffers are compared, so a write that the rule does not name shows.  Shapes are the smallest at which
each hazard exists: T spans the backpointers' period of 8 frames, the prefetch depth and the traceback's chunks,
k every template instance (part of a wave, one wave, 4 and 16 waves).
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CANARY = 0xA5
SCORE_CANARY = -12345.5
PAD = 64
FRAMES = (1, 2, 3, 7, 8, 9, 37, 300)
NAN, INF = float("nan"), float("inf")
BAD = 10


def make_scores(rng, kind, shape, dtype):
    """ties: small integers; generic: float32 values whose sums round differently from row to row; special: the
    small integers with +-inf, NaN and the two zeros mixed in at about 10 %."""
    if kind == "ties":
        return rng.integers(-2, 3, shape).astype(dtype)
    if kind == "generic":
        return (rng.standard_normal(shape) * 3).astype(np.float32).astype(dtype)
    values = np.array([INF, -INF, NAN, -0.0, 0.0], np.float32)
    x = rng.integers(-2, 3, shape).astype(np.float32)
    return np.where(rng.random(shape) < 0.10, values[rng.integers(0, len(values), shape)], x).astype(dtype)


def reference(host, k, tr, stay):
    """(codes [N, T], row_score [N]) of host [N, T, C], row by row."""
    from rawnanoporesignalcompression_amd import crf_viterbi_signal

    got = [crf_viterbi_signal(row, k, tr, stay) for row in host]
    return np.stack([g[0] for g in got]), np.array([g[1] for g in got], np.float32)


def place(host, layout):
    """host [N, T, C] on the device as (view, time_major)."""
    import torch

    N, T, C_ = host.shape
    t = torch.from_numpy(np.ascontiguousarray(host)).to("cuda:0")
    if layout == "NTC":
        return t, False
    if layout == "TNC":
        return t.permute(1, 0, 2).contiguous(), True
    if layout == "rowpad":      # rows 3 elements further apart than T * C
        buf = torch.zeros(N * (T * C_ + 3), dtype=t.dtype, device="cuda:0")
        view = buf.as_strided((N, T, C_), (T * C_ + 3, C_, 1))
    elif layout == "framepad":  # frames one element further apart than C
        buf = torch.zeros(N * T * (C_ + 1), dtype=t.dtype, device="cuda:0")
        view = buf.as_strided((N, T, C_), (T * (C_ + 1), C_ + 1, 1))
    else:
        assert layout == "offset"   # from one element behind an allocation's start: no wide load is aligned
        buf = torch.zeros(N * T * C_ + 1, dtype=t.dtype, device="cuda:0")
        view = buf[1:].view(N, T, C_)
    view.copy_(t)
    return view, False


def run(codec, view, k, tr, stay, time_major=False, cstride=None, score=True, expect=0):
    """The call through the C ABI into canary-filled buffers; (codes [N, T], row_score [N] or None) on the host,
    after checking that nothing else in either buffer changed."""
    import torch

    from rawnanoporesignalcompression_amd import crf_params

    nd, td = (1, 0) if time_major else (0, 1)
    N, T = int(view.shape[nd]), int(view.shape[td])
    item = view.element_size()
    prm = crf_params(k, tr, np.float16 if view.dtype == torch.float16 else np.float32, stay)
    cstride = T if cstride is None else cstride
    cbuf = torch.full((PAD + N * cstride + PAD,), CANARY, dtype=torch.uint8, device="cuda:0")
    sbuf = torch.full((PAD + N + PAD,), SCORE_CANARY, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    rc = codec._lib.pgn_crf_viterbi_rows_device(
        codec._h, C.byref(prm), N, T, view.data_ptr(), int(view.stride(nd)) * item, int(view.stride(td)) * item,
        cbuf.data_ptr() + PAD, cstride, sbuf.data_ptr() + 4 * PAD if score else None, None)
    torch.cuda.synchronize()
    assert rc == expect
    c, s = cbuf.cpu().numpy(), sbuf.cpu().numpy()
    assert (c[:PAD] == CANARY).all() and (c[PAD + N * cstride:] == CANARY).all(), "codes: canary"
    body = c[PAD:PAD + N * cstride].reshape(N, cstride)
    assert (body[:, T:] == CANARY).all(), "codes: the bytes between rows"
    assert (s[:PAD] == SCORE_CANARY).all() and (s[PAD + N:] == SCORE_CANARY).all(), "row_score: canary"
    if expect:
        assert (body == CANARY).all() and (s == SCORE_CANARY).all(), "a refused call wrote"
        return None, None
    if not score:
        assert (s == SCORE_CANARY).all()
    return body[:, :T].copy(), s[PAD:PAD + N].copy() if score else None


def same(got, want, what):
    codes, score = got
    wcodes, wscore = want
    if not np.array_equal(codes, wcodes):
        bad = np.argwhere(codes != wcodes)
        raise AssertionError(f"{what}: {len(bad)} of {codes.size} codes differ, first at row {bad[0][0]} frame "
                             f"{bad[0][1]}: got {codes[tuple(bad[0])]:#x}, want {wcodes[tuple(bad[0])]:#x}")
    if score is not None:
        assert np.array_equal(score.view(np.uint32), wscore.view(np.uint32)), (what, score, wscore)


CONFIGS = [(k, tr, dt) for k in (1, 2, 3, 4, 5) for tr in (5, 4) for dt in (np.float16, np.float32)]


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: f"k{c[0]}-tr{c[1]}-{np.dtype(c[2]).name}")
def test_every_instance_every_length(codec, cfg):
    """Three rows of every T in FRAMES, for every state length, both layouts of the transitions (4 with a
    non-zero stay_score) and both types; the three kinds of values take turns."""
    k, tr, dtype = cfg
    stay = 0.0 if tr == 5 else -0.75
    rng = np.random.default_rng(100 * k + 10 * tr + np.dtype(dtype).itemsize)
    kinds = ("ties", "generic", "special")
    for i, T in enumerate(FRAMES):
        for kind in (kinds[i % 3], kinds[(i + 1) % 3]) if k < 5 else (kinds[i % 3],):
            host = make_scores(rng, kind, (3, T, tr * 4 ** k), dtype)
            view, tm = place(host, "NTC")
            same(run(codec, view, k, tr, stay), reference(host, k, tr, stay), f"{cfg} T={T} {kind}")


@pytest.mark.parametrize("kind", ["ties", "generic", "special"])
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_many_rows_and_one(codec, k, kind):
    """130 rows (more workgroups than one round of a small grid, more rows than a wave has lanes) and one row."""
    rng = np.random.default_rng(7 * k + len(kind))
    dtype = np.float16 if k % 2 else np.float32
    for N, T in ((130, 9 if k == 4 else 37), (1, 37)):
        host = make_scores(rng, kind, (N, T, 5 * 4 ** k), dtype)
        same(run(codec, place(host, "NTC")[0], k, 5, 0.0), reference(host, k, 5, 0.0), f"k={k} N={N} {kind}")


def test_largest_instance(codec):
    """k = 5: sixteen waves per row, five rows of 300 frames (15 MB of float16 scores), generic values."""
    rng = np.random.default_rng(55)
    host = make_scores(rng, "generic", (5, 300, 5120), np.float16)
    same(run(codec, place(host, "NTC")[0], 5, 5, 0.0), reference(host, 5, 5, 0.0), "k=5")


@pytest.mark.parametrize("layout", ["NTC", "TNC", "rowpad", "framepad", "offset"])
@pytest.mark.parametrize("k,dtype", [(1, np.float16), (1, np.float32), (3, np.float16), (3, np.float32), (4, np.float16)])
def test_layouts(codec, k, dtype, layout):
    """[N, T, C], [T, N, C], a row stride above T * C, a frame stride above C and a view that starts one element
    into its buffer (k = 1 rows of float16 are 40 bytes apart and misalign by themselves), through the C ABI and
    through the method; the codes go to rows 5 bytes further apart than T."""
    import torch

    rng = np.random.default_rng(k + len(layout))
    N, T = 3, 37
    for tr, stay in ((5, 0.0), (4, 0.5)):
        host = make_scores(rng, "special" if tr == 5 else "ties", (N, T, tr * 4 ** k), dtype)
        want = reference(host, k, tr, stay)
        view, tm = place(host, layout)
        same(run(codec, view, k, tr, stay, time_major=tm, cstride=T + 5), want, f"k={k} {layout} tr={tr}")
        res = codec.crf_viterbi(view, k, stay_score=stay, time_major=tm)
        assert res.params.transitions == tr and res.codes.shape == (N, T) and res.codes.dtype == torch.uint8
        same((res.codes.cpu().numpy(), res.row_score.cpu().numpy()), want, f"method k={k} {layout} tr={tr}")
        out = torch.full((N, T + 3), CANARY, dtype=torch.uint8, device="cuda:0")
        res = codec.crf_viterbi(view, k, transitions=tr, stay_score=stay, time_major=tm, codes=out[:, :T], row_score=False)
        assert res.row_score is None and res.codes.data_ptr() == out.data_ptr()
        assert np.array_equal(out.cpu().numpy()[:, :T], want[0]) and (out.cpu().numpy()[:, T:] == CANARY).all()


def test_without_row_score_and_without_rows(codec):
    from rawnanoporesignalcompression_amd import crf_params

    rng = np.random.default_rng(5)
    host = make_scores(rng, "ties", (3, 9, 320), np.float16)
    view, _ = place(host, "NTC")
    codes, score = run(codec, view, 3, 5, 0.0, score=False)
    assert score is None
    same((codes, None), reference(host, 3, 5, 0.0), "no row_score")
    prm = crf_params(3)
    fn = codec._lib.pgn_crf_viterbi_rows_device
    assert fn(codec._h, C.byref(prm), 0, 9, None, 0, 640, None, 0, None, None) == 0   # nrows == 0 touches nothing
    assert fn(codec._h, C.byref(prm), 1, 9, None, 5760, 640, C.c_void_p(view.data_ptr()), 9, None, None) == BAD


def test_scratch_groups_and_the_cap(codec):
    """A cap that holds two rows: five rows are decoded in three groups, with the default's output.  A cap below
    one row is refused, and nothing is written."""
    from rawnanoporesignalcompression_amd import PGNanoError

    rng = np.random.default_rng(9)
    k, T = 2, 37
    row_bytes = 4 * 16 * ((T + 7) // 8) + 16
    host = make_scores(rng, "generic", (5, T, 80), np.float32)
    view, _ = place(host, "NTC")
    want = reference(host, k, 5, 0.0)
    whole = run(codec, view, k, 5, 0.0)
    same(whole, want, "default cap")
    try:
        codec.set_crf_scratch(2 * row_bytes + row_bytes // 2)
        same(run(codec, view, k, 5, 0.0), want, "groups of two rows")
        codec.set_crf_scratch(row_bytes)
        same(run(codec, view, k, 5, 0.0), want, "groups of one row")
        codec.set_crf_scratch(row_bytes - 1)
        run(codec, view, k, 5, 0.0, expect=BAD)
        with pytest.raises(PGNanoError):
            codec.crf_viterbi(view, k)
        codec.set_crf_scratch(0)
        same(run(codec, view, k, 5, 0.0), want, "the default restored")
    finally:
        codec.set_crf_scratch(0)


def test_method_argument_validation(codec):
    import torch

    x = torch.zeros((2, 4, 20), dtype=torch.float16, device="cuda:0")
    for bad in (lambda: codec.crf_viterbi(x[0], 1), lambda: codec.crf_viterbi(x, 2), lambda: codec.crf_viterbi(x, 0),
                lambda: codec.crf_viterbi(x, 1, transitions=4), lambda: codec.crf_viterbi(x.double(), 1),
                lambda: codec.crf_viterbi(x, 1, stay_score=1.0), lambda: codec.crf_viterbi(x.cpu(), 1),
                lambda: codec.crf_viterbi(x[:, :, ::2], 1, transitions=5),
                lambda: codec.crf_viterbi(x, 1, codes=torch.zeros((2, 5), dtype=torch.uint8, device="cuda:0")),
                lambda: codec.crf_viterbi(x, 1, codes=torch.zeros((2, 4), dtype=torch.int8, device="cuda:0")),
                lambda: codec.set_crf_scratch(-1)):
        with pytest.raises(ValueError):
            bad()
    empty = codec.crf_viterbi(x[:0], 1)
    assert empty.codes.shape == (0, 4) and empty.row_score.shape == (0,)


# ---- the chain: rows -> codes -> stitched codes -> bases ----------------------------------------------
def planted_rows(rng, R, T, k, tr):
    """[R, T, C] float16 scores, every row with a path of its own planted: its transitions score +4 (with 4
    transitions its stays are the constant 0), everything else lies in [-1, -0.01]."""
    S = 4 ** k
    x = -(rng.random((R, T, tr * S)) * 0.99 + 0.01)
    for r in range(R):
        s = int(rng.integers(0, S))
        for t in range(T):
            if rng.random() < 0.5:
                if tr == 5:
                    x[r, t, 5 * s] = 4
            else:
                b, s = s >> (2 * (k - 1)), ((s << 2) & (S - 1)) | int(rng.integers(0, 4))
                x[r, t, tr * s + tr - 4 + b] = 4
    return x.astype(np.float16)


def segment_starts(m, L, V):
    if m == 0:
        return []
    if m <= L:
        return [(0, m)]
    stride = L - V
    return [(min(j * stride, m - L), L) for j in range(-(-(m - L) // stride) + 1)]


def test_the_chain_to_bases(codec):
    """A host-built segment table of ragged reads (one of a single short padded row, one with a status, one
    without samples), planted-path scores per row at k = 3, crf_viterbi in two model batches, the stitch of the
    code bytes and collapse_codes -- against the same chain in numpy."""
    import torch

    from rawnanoporesignalcompression_amd import (ReadSegments, SegmentedReads, SegmentTable, collapse_codes_signal,
                                                  stitch_plan_signal)

    L, V, s, k = 40, 8, 4, 3
    T = L // s
    lengths, trims = [100, 333, 25, 57, 0, 40, 131], [0, 3, 5, 0, 0, 2, 7]
    bad_read = 3
    segs, reads = [], np.zeros(len(lengths), ReadSegments.DTYPE)
    for r, (m, trim) in enumerate(zip(lengths, trims)):
        mine = segment_starts(m, L, V)
        reads[r] = (len(segs), len(mine), trim, 6 if r == bad_read else 0, 0, 0, 0.0)
        segs += [(r, trim + a, valid, 0) for a, valid in mine]
    table = np.array(segs, SegmentTable.DTYPE)
    R = len(table)
    as_raw = lambda a: torch.from_numpy(a.view(np.uint8).reshape(len(a), -1).copy()).to("cuda:0")
    segmented = SegmentedReads(None, SegmentTable(as_raw(table)), ReadSegments(as_raw(reads)), None, None)
    plan = codec.stitch_plan(segmented, L, V, s)

    rng = np.random.default_rng(77)
    host = planted_rows(rng, R, T, k, 5)
    rows = torch.from_numpy(host).to("cuda:0")
    total = int(plan.read_frames[-1].item())
    frames = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda:0")
    split = R // 2 + 1
    for first, n in ((0, split), (split, R - split)):
        batch = codec.crf_viterbi(rows[first:first + n], k)
        codec.stitch(plan, batch.codes, first, out=frames)
    got = codec.collapse_codes(frames, plan.read_frames, "ACGT")

    codes = np.stack([reference(host[g:g + 1], k, 5, 0.0)[0][0] for g in range(R)])
    want_seq, want_bases, want_frames = [], [0], []
    for r in range(len(lengths)):
        first, n = int(reads["first_segment"][r]), int(reads["nsegments"][r])
        mine = np.zeros(0, np.uint8)
        if reads["status"][r] == 0 and n:
            fc = stitch_plan_signal(np.stack([table["start"][first:first + n], table["valid"][first:first + n]], 1), L, V, s)
            mine = np.concatenate([codes[first + j, a:a + c] for j, (a, c) in enumerate(fc)])
        want_frames.append(mine)
        seq, _ = collapse_codes_signal(mine, "ACGT")
        want_seq.append(seq)
        want_bases.append(want_bases[-1] + len(seq))
    assert np.array_equal(frames.cpu().numpy(), np.concatenate(want_frames))
    assert np.array_equal(got.read_bases.cpu().numpy(), np.array(want_bases, np.int64))
    assert got.seq.cpu().numpy()[:want_bases[-1]].tobytes() == np.concatenate(want_seq).tobytes()
    assert (got.status.cpu().numpy() == 0).all()
    assert want_bases[bad_read] == want_bases[bad_read + 1] and len(want_frames[2]) == 7 and want_bases[-1] > 50
    assert set(np.concatenate(want_seq).tobytes()) <= set(b"ACGT")
