"""Stitched probabilities to phred strings on the GPU (pgn_base_qual_device), bit for bit against base_qual_signal
read by read: the rule is integer sums and comparisons, so the tolerance is zero.

Every input is built on the host -- the frames' codes and probabilities, read_frames, and what
pgn_collapse_codes_device would leave for them (read_bases, base_frame, statuses; collapse_codes_signal gives
them) -- so that each rule can be set against the others: a read outside the window or with a status still has
bases in read_bases, and must get nothing.  The qualities lie between canary bytes and the whole buffer is
compared: the bytes of a read that gets no output keep the canary.
"""
import ctypes as C

import numpy as np
import pytest

from test_quality_api import frames_with_sum

pytestmark = pytest.mark.gpu

CANARY = 0xA5
PAD = 64
NAN, INF = float("nan"), float("inf")


def random_read(rng, F, p_emit, first=0):
    """(codes, post) of F frames: a frame emits with probability p_emit from frame `first` on; the probabilities
    are a softmax of normal scores times 4, so the errors span the thresholds."""
    codes = rng.integers(0, 4, F).astype(np.uint8)
    emit = rng.random(F) < p_emit
    emit[:first] = False
    codes[emit] |= 0x80
    z = rng.standard_normal((F, 4)) * 4
    e = np.exp(z - z.max(1, keepdims=True))
    return codes, (e / e.sum(1, keepdims=True)).astype(np.float32)


def check(codec, reads, thr, q_min, *, status=None, window=None, capacity=None, offset_post=False):
    """reads: [(codes, post)].  Runs the call through the C ABI and compares the whole quality buffer with the
    rule; returns the strings of the reads that get output (None for the others)."""
    import torch

    from rawnanoporesignalcompression_amd import collapse_codes_signal
    from rawnanoporesignalcompression_amd.quality import base_qual_signal, qual_params

    n = len(reads)
    frames = np.array([0] + [len(c) for c, _ in reads], np.int64).cumsum()
    at = [collapse_codes_signal(c, "ACGT")[1] for c, _ in reads]
    bases = np.array([0] + [len(a) for a in at], np.int64).cumsum()
    status = np.zeros(n, np.int32) if status is None else np.asarray(status, np.int32)
    lo, hi = (0, int(frames[-1])) if window is None else window
    capacity = int(bases[-1]) if capacity is None else capacity
    codes = np.concatenate([c for c, _ in reads] + [np.zeros(0, np.uint8)])
    post = np.concatenate([p for _, p in reads] + [np.zeros((0, 4), np.float32)]).astype(np.float32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    d_codes = dev(codes[lo:hi])
    d_post = dev(np.concatenate([np.zeros(1, np.float32), post[lo:hi].reshape(-1)]))   # 4-byte aligned, no more
    post_ptr = d_post.data_ptr() + 4
    if not offset_post:
        d_post = dev(post[lo:hi].reshape(-1))
        post_ptr = d_post.data_ptr()
    d_frames, d_bases, d_status = dev(frames), dev(bases), dev(status)
    d_at = dev(np.concatenate(at + [np.zeros(1, np.uint32)]).astype(np.uint32))
    qbuf = torch.full((PAD + int(bases[-1]) + PAD,), CANARY, dtype=torch.uint8, device="cuda:0")
    prm = qual_params(thr, q_min)
    torch.cuda.synchronize()
    rc = codec._lib.pgn_base_qual_device(
        codec._h, C.byref(prm), n, d_frames.data_ptr(), d_codes.data_ptr() if hi > lo else None,
        post_ptr if hi > lo else None, lo, hi - lo, d_bases.data_ptr(), d_at.data_ptr(), d_status.data_ptr(),
        qbuf.data_ptr() + PAD if capacity else None, capacity, None)
    torch.cuda.synchronize()
    assert rc == 0
    want = np.full(len(qbuf), CANARY, np.uint8)
    strings = []
    for r, (c, p) in enumerate(reads):
        ok = lo <= frames[r] and frames[r + 1] <= hi and status[r] == 0 and bases[r + 1] <= capacity
        q = base_qual_signal(c, p, at[r], len(c), thr, q_min) if ok else None
        strings.append(q)
        if ok:
            want[PAD + bases[r]:PAD + bases[r + 1]] = q
    got = qbuf.cpu().numpy()
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    return strings


def test_the_rules_among_reads(codec):
    """Blocks of one frame; a block of 5,000 frames between short ones; two emitting frames in a row; a read without
    bases; frames before the first base; a read without frames; and ordinary reads of many bases (more than one wave's
    64, more than the workgroup's 256)."""
    from rawnanoporesignalcompression_amd.quality import qual_thresholds

    rng = np.random.default_rng(1)
    every = random_read(rng, 70, 1.1)                      # every frame emits: blocks of one frame
    stalled = random_read(rng, 5400, 0.0)
    stalled[0][[3, 4, 5, 5005, 5006, 5399]] |= 0x80        # two in a row, then 5,000 frames, then a last block of one
    silent = random_read(rng, 40, 0.0)
    late = random_read(rng, 300, 0.3, first=37)
    none = (np.zeros(0, np.uint8), np.zeros((0, 4), np.float32))
    reads = [every, stalled, silent, late, none, random_read(rng, 3000, 0.35), random_read(rng, 900, 0.05)]
    thr = qual_thresholds()
    strings = check(codec, reads, thr, 1)
    assert len(strings[0]) == 70 and len(strings[1]) == 6 and len(strings[2]) == 0 and len(strings[5]) > 600
    assert len({int(q) for s in strings for q in s}) > 20  # the qualities spread over the scale
    check(codec, reads, thr, 1, offset_post=True)          # probabilities at a 4-byte address
    check(codec, reads, qual_thresholds(0.9, -0.3, 2, 60), 2)
    check(codec, reads, np.zeros(0, np.uint32), 7)         # no thresholds: q_min everywhere


def test_reads_that_get_nothing(codec):
    """A read with a status, a read outside the window at either end and the reads cut by the capacity keep the
    canary although read_bases and base_frame describe their bases; the others are as before."""
    from rawnanoporesignalcompression_amd.quality import qual_thresholds

    rng = np.random.default_rng(2)
    reads = [random_read(rng, F, 0.4) for F in (50, 120, 64, 200, 90)]
    thr = qual_thresholds()
    all_of_them = check(codec, reads, thr, 1)
    got = check(codec, reads, thr, 1, status=[0, 6, 0, 0, 1])
    assert got[1] is None and got[4] is None and all(np.array_equal(got[r], all_of_them[r]) for r in (0, 2, 3))
    frames = np.cumsum([0] + [len(c) for c, _ in reads])
    got = check(codec, reads, thr, 1, window=(int(frames[1]), int(frames[4])))
    assert got[0] is None and got[4] is None and all(np.array_equal(got[r], all_of_them[r]) for r in (1, 2, 3))
    got = check(codec, reads, thr, 1, window=(int(frames[1]) + 1, int(frames[4]) - 1))
    assert [g is None for g in got] == [True, True, False, True, True]
    nbases = np.cumsum([len(s) for s in all_of_them])
    got = check(codec, reads, thr, 1, capacity=int(nbases[2]))
    assert [g is None for g in got] == [False, False, False, True, True]
    got = check(codec, reads, thr, 1, capacity=int(nbases[2]) - 1)
    assert [g is None for g in got] == [False, False, True, True, True]
    assert all(g is None for g in check(codec, reads, thr, 1, capacity=0))
    assert all(g is None for g in check(codec, reads, thr, 1, window=(7, 7)))


def test_special_probabilities(codec):
    """NaN (in the called base's place it does not count, elsewhere it is 2^32 - 1), infinities, negative values and
    sums above one, in blocks of one frame and inside a block of 100."""
    from rawnanoporesignalcompression_amd.quality import qual_thresholds

    rows = np.array([[0.25, 0.25, 0.25, 0.25], [1.0, 0.0, 0.0, 0.0], [NAN, 0.0, 0.0, 0.0], [0.5, NAN, 0.0, 0.0],
                     [1.0, -0.5, 0.25, 0.0], [0.0, 2.0, 2.0, 2.0], [0.0, INF, -INF, 0.0], [0.9, 1e-3, 0.0, 0.0],
                     [1.0, -0.0, 0.0, -1e-30], [0.0, 1.0, 0.0, 0.0], [0.0, INF, 0.0, 0.0], [0.0, 0.5, 0.5, 2.0 ** -25]],
                    np.float32)
    thr = qual_thresholds()
    for c in range(4):
        post = np.roll(rows, c, axis=1)
        singles = check(codec, [(np.full(len(rows), 0x80 | c, np.uint8), post)], thr, 1)[0]
        assert singles[:8].tolist() == [34, 83, 83, 34, 83, 34, 34, 63]
    rng = np.random.default_rng(3)
    codes, post = random_read(rng, 400, 0.0)
    codes[[0, 100, 200, 300]] |= 0x80
    post[[5, 150, 151, 250, 399]] = rows[[3, 4, 5, 6, 2]]
    check(codec, [(codes, post)], thr, 1)


def test_threshold_edges(codec):
    """U exactly at thr[j] * n, one below and one above, for blocks of 1, 3, 64, 65 (the wave takes over), 700 and
    5,000 frames: the sum of a long block split among lanes is the same integer."""
    thr = np.array([5_000_000, 70_000, 70_000, 900, 0], np.uint32)
    for n in (1, 3, 64, 65, 700, 5000):
        codes, post, expect = [], [], []
        for j, count in ((0, 1), (1, 3), (3, 4)):
            for d, admitted in ((0, count), (-1, count), (1, count - (2 if j == 1 else 1))):
                c = len(expect) % 4
                codes.append(np.concatenate([[c | 0x80], np.full(n - 1, (c + 1) & 3)]).astype(np.uint8))
                post.append(frames_with_sum(int(thr[j]) * n + d, n, c))
                expect.append(33 + 2 + admitted)
        got = check(codec, [(np.concatenate(codes), np.concatenate(post))], thr, 2)[0]
        assert got.tolist() == expect, (n, got.tolist(), expect)


def test_the_function(codec):
    """quality.base_qual on what collapse_codes left, with a frame_base, a capacity that cuts and an `out`."""
    import torch

    from rawnanoporesignalcompression_amd import quality

    rng = np.random.default_rng(4)
    reads = [random_read(rng, F, 0.4) for F in (80, 33, 500)]
    base = 1000
    frames = torch.tensor(np.cumsum([0] + [len(c) for c, _ in reads]) + base, dtype=torch.int64, device="cuda:0")
    codes = torch.from_numpy(np.concatenate([c for c, _ in reads])).to("cuda:0")
    post = torch.from_numpy(np.concatenate([p for _, p in reads])).to("cuda:0")
    want = [quality.base_qual_signal(c, p, np.flatnonzero(c & 0x80), len(c), quality.qual_thresholds(), 1) for c, p in reads]
    dec = codec.collapse_codes(codes, frames, "ACGT", frame_base=base)
    q = quality.base_qual(codec, dec, codes, post, frames, frame_base=base)
    assert q.dtype == torch.uint8 and q.shape == dec.seq.shape
    total = sum(len(w) for w in want)
    assert np.array_equal(q.cpu().numpy()[:total], np.concatenate(want))
    cut = len(want[0]) + len(want[1])
    dec = codec.collapse_codes(codes, frames, "ACGT", frame_base=base, capacity=cut)
    out = torch.full((cut,), CANARY, dtype=torch.uint8, device="cuda:0")
    q = quality.base_qual(codec, dec, codes, post, frames, [9, 4], q_min=0, frame_base=base, out=out)
    assert q.data_ptr() == out.data_ptr()
    assert np.array_equal(out.cpu().numpy(), np.concatenate([quality.base_qual_signal(c, p, np.flatnonzero(c & 0x80), len(c),
                                                                                      [9, 4], 0) for c, p in reads[:2]]))
    for bad in (lambda: quality.base_qual(codec, dec, codes, post[:-1], frames),
                lambda: quality.base_qual(codec, dec, codes, post.double(), frames),
                lambda: quality.base_qual(codec, dec, codes, post, frames[:-1]),
                lambda: quality.base_qual(codec, dec, codes, post, frames, [1, 2]),
                lambda: quality.base_qual(codec, dec, codes, post, frames, out=out[:-1]),
                lambda: quality.base_qual(codec, codec.collapse_codes(codes, frames, "ACGT", frame_base=base, base_frame=False),
                                          codes, post, frames)):
        with pytest.raises(ValueError):
            bad()
