"""Adapters and barcodes on the GPU (pgn_find_patterns_device, pgn_classify_reads_device, pgn_trim_reads_device
through demux.find_patterns, demux.classify and demux.trim_reads), bit for bit against the host models on every case
of tests/_demux_cases.py, the 0xFFFFFFFF fills included.  The C calls are also made directly with every output a
view into a sentinel-filled buffer, at odd alignments too: the guard bytes around every output, and every element
the rule does not write, keep the sentinel.  The refusals come in the header's order on a real context.
"""
import ctypes as C

import numpy as np
import pytest

import _demux_cases as K

pytestmark = pytest.mark.gpu

SENTINEL, FRONT, BACK = 0xA5, 64, 96


@pytest.fixture(scope="module")
def find_cases():
    return K.find_cases()


@pytest.fixture(scope="module")
def class_cases():
    return K.class_cases()


@pytest.fixture(scope="module")
def trim_cases():
    return K.trim_cases()


def up(a):
    import torch

    a = np.ascontiguousarray(a)
    signed = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype)
    return torch.from_numpy(a.view(signed) if signed else a).to("cuda:0")


class Guarded:
    """``count`` elements of ``dtype`` inside a sentinel-filled byte buffer, ``shift`` bytes off 16-byte alignment."""

    def __init__(self, count, dtype, shift=0):
        import torch

        self.dtype, self.count = np.dtype(dtype), count
        self.at = FRONT + shift
        self.buf = torch.full((self.at + count * self.dtype.itemsize + BACK,), SENTINEL, dtype=torch.uint8, device="cuda:0")
        assert self.buf.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.at if self.count else 0

    def check(self, want, what):
        """The first ``len(want)`` elements equal ``want``; everything else is the sentinel."""
        got = self.buf.cpu().numpy()
        nbytes = len(want) * self.dtype.itemsize
        mine = got[self.at:self.at + nbytes].view(self.dtype)
        if not np.array_equal(mine, np.asarray(want).astype(self.dtype)):
            bad = np.flatnonzero(mine != np.asarray(want).astype(self.dtype))
            raise AssertionError(f"{what}: {len(bad)} of {len(want)} differ, the first at {bad[:8].tolist()}: "
                                 f"{mine[bad[:8]].tolist()} for {np.asarray(want)[bad[:8]].tolist()}")
        assert (got[:self.at] == SENTINEL).all() and (got[self.at + nbytes:] == SENTINEL).all(), f"{what}: a guard byte changed"


def decoded_of(c, base_frame=None):
    from rawnanoporesignalcompression_amd import DecodedReads

    return DecodedReads(up(c.seq[:c.base_capacity]), up(c.read_bases), up(c.status), None if base_frame is None else up(base_frame[:c.base_capacity]),
                        None, None, None)


def pattern_set(c, classes=None):
    from rawnanoporesignalcompression_amd import demux

    pat, off, side, md = c.arrays()
    cls = np.full(len(side), K.NO_CLASS, np.uint32) if classes is None else classes
    return demux.PatternSet.from_arrays(pat, off, side, md, cls).to(0)


# ---- the search ----------------------------------------------------------------------------------------------
def run_find(codec, c, shift=0):
    import torch

    from rawnanoporesignalcompression_amd import demux

    decoded, pats = decoded_of(c), pattern_set(c)
    n, P = len(c.status), len(c.patterns)
    want = c.expected()
    hits = demux.find_patterns(codec, decoded, pats, window=c.window)
    for name, w in zip(("dist", "start", "end"), want):
        got = getattr(hits, name)
        assert got.dtype == torch.int32 and tuple(got.shape) == (n, P)
        assert np.array_equal(got.cpu().numpy().view(np.uint32), w), (c.name, name)
    outs = [Guarded(n * P, np.uint32, shift) for _ in range(3)]
    with codec._launch(None) as ls:
        rc = codec._lib.pgn_find_patterns_device(
            codec._h, n, decoded.seq.data_ptr(), decoded.read_bases.data_ptr(), decoded.status.data_ptr(), c.base_capacity,
            c.window, P, pats.d_pat.data_ptr(), int(pats.d_pat.numel()), pats.d_pat_off.data_ptr(), pats.d_side.data_ptr(),
            pats.d_max_dist.data_ptr(), outs[0].ptr, outs[1].ptr, outs[2].ptr, ls.cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    for name, o, w in zip(("dist", "start", "end"), outs, want):
        o.check(w.reshape(-1), f"{c.name} {name}")
    return hits


@pytest.mark.parametrize("name", [c.name for c in K.find_cases()])
def test_find_patterns(codec, find_cases, name):
    c = {c.name: c for c in find_cases}[name]
    run_find(codec, c, shift=4 * (len(name) % 4))


def test_find_patterns_reads_no_pattern_byte_beyond_its_buffer(codec, find_cases):
    """Offsets that point beyond the pattern bytes, descend or repeat: those patterns are not searched, the others are."""
    import torch

    from rawnanoporesignalcompression_amd import demux

    c = {c.name: c for c in find_cases}["tie-ends"]
    decoded = decoded_of(c)
    pat = np.frombuffer(b"ACGAGGACG", np.uint8)
    off = np.array([0, 3, 3, 6, 4, 9, 4000, 4003], np.uint32)      # 3 bytes, 0, 3, descending, 5, beyond, beyond
    pats = demux.PatternSet.from_arrays(pat, off, [0] * 7, [1] * 7, [K.NO_CLASS] * 7).to(0)
    hits = demux.find_patterns(codec, decoded, pats, window=c.window)
    torch.cuda.synchronize()
    want = K.host.find_patterns_signal(c.seq, c.read_bases, c.status, [b"ACG", b"", b"AGG", b"", b"GGACG", b"", b""], [0] * 7,
                                       [1] * 7, c.window)
    for name, w in zip(("dist", "start", "end"), want):
        assert np.array_equal(getattr(hits, name).cpu().numpy().view(np.uint32), w), name
    assert (want[0][:, [1, 3, 5, 6]] == K.NONE).all() and (want[0][:, [0, 2, 4]] != K.NONE).all()


def test_find_patterns_on_a_callers_stream_and_repeated(codec, find_cases):
    import torch

    from rawnanoporesignalcompression_amd import demux

    by = {c.name: c for c in find_cases}
    s = torch.cuda.Stream()
    for name in ("P257-tail", "L1", "long-read", "P257-tail"):
        c = by[name]
        hits = demux.find_patterns(codec, decoded_of(c), pattern_set(c), window=c.window, stream=s.cuda_stream)
        torch.cuda.synchronize()
        assert np.array_equal(hits.dist.cpu().numpy().view(np.uint32), c.expected()[0]), name
        assert np.array_equal(hits.start.cpu().numpy().view(np.uint32), c.expected()[1]), name


def test_find_patterns_in_its_other_form(find_cases):
    """PGN_DEMUX_FIND=plain (the index in pattern order, both words of the column in every wave) gives the same
    outputs: the form kept for the measurement, on a context of its own."""
    import os

    import torch

    from rawnanoporesignalcompression_amd import PGNanoCodec, demux

    os.environ["PGN_DEMUX_FIND"] = "plain"
    try:
        plain = PGNanoCodec(0)
    finally:
        del os.environ["PGN_DEMUX_FIND"]
    try:
        for c in find_cases:
            if c.tags & {"seam", "mixed", "P257", "P65", "n", "bad", "fuzz", "N"}:
                hits = demux.find_patterns(plain, decoded_of(c), pattern_set(c), window=c.window)
                torch.cuda.synchronize()
                for name, w in zip(("dist", "start", "end"), c.expected()):
                    assert np.array_equal(getattr(hits, name).cpu().numpy().view(np.uint32), w), (c.name, name)
    finally:
        plain.close()


# ---- the class -----------------------------------------------------------------------------------------------
NAMES5 = ("barcode", "best_dist", "second_dist", "lo", "hi")


def run_classify(codec, c, shift=0):
    import torch

    from rawnanoporesignalcompression_amd import DecodedReads, demux

    n, P = c.dist.shape
    total = int(c.read_bases[-1])
    decoded = DecodedReads(torch.zeros(c.base_capacity, dtype=torch.uint8, device="cuda:0"), up(c.read_bases), up(c.status),
                           None, None, None, None)
    assert c.base_capacity <= total
    pats = demux.PatternSet.from_arrays(np.zeros(P, np.uint8), np.arange(P + 1), c.sides, c.max_dist, c.classes).to(0)
    hits = demux.PatternHits(up(c.dist), up(c.start), up(c.end))
    want = c.expected()
    got = demux.classify(codec, decoded, hits, pats, c.nclasses, c.min_sep)
    for name, w in zip(NAMES5, want):
        assert np.array_equal(getattr(got, name).cpu().numpy().view(np.uint32), w), (c.name, name)
    outs = [Guarded(n, np.uint32, shift) for _ in range(5)]
    with codec._launch(None) as ls:
        rc = codec._lib.pgn_classify_reads_device(
            codec._h, n, decoded.read_bases.data_ptr(), decoded.status.data_ptr(), c.base_capacity, P, pats.d_side.data_ptr(),
            pats.d_max_dist.data_ptr(), pats.d_pclass.data_ptr(), c.nclasses, c.min_sep, hits.dist.data_ptr(),
            hits.start.data_ptr(), hits.end.data_ptr(), *(o.ptr for o in outs), ls.cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    for name, o, w in zip(NAMES5, outs, want):
        o.check(w, f"{c.name} {name}")


@pytest.mark.parametrize("name", [c.name for c in K.class_cases()])
def test_classify(codec, class_cases, name):
    run_classify(codec, {c.name: c for c in class_cases}[name], shift=4)


def test_classify_the_hits_of_the_search(codec, find_cases):
    """The two calls in a row on the search cases with classes laid over their patterns."""
    from rawnanoporesignalcompression_amd import demux

    for name in ("fuzz0", "fuzz1", "fuzz2", "text-lengths", "P257-tail", "not-taken", "bad-patterns"):
        c = {c.name: c for c in find_cases}[name]
        P = len(c.patterns)
        classes = np.array([K.NO_CLASS if p % 4 == 3 else p % 3 for p in range(P)], np.uint32)
        decoded, pats = decoded_of(c), pattern_set(c, classes)
        hits = demux.find_patterns(codec, decoded, pats, window=c.window)
        got = demux.classify(codec, decoded, hits, pats, 3, 1)
        d, s, e = c.expected()
        want = K.host.classify_signal(d, s, e, c.read_bases, c.status, c.sides, c.max_dist, classes, 3, 1, c.base_capacity)
        for field, w in zip(NAMES5, want):
            assert np.array_equal(getattr(got, field).cpu().numpy().view(np.uint32), w), (name, field)


# ---- the slice -----------------------------------------------------------------------------------------------
def run_trim(codec, c, shift=0):
    import torch

    from rawnanoporesignalcompression_amd import demux

    n = len(c.status)
    want = c.expected()
    decoded = decoded_of(c, c.base_frame)
    qual = None if c.qual is None else up(c.qual[:c.base_capacity])
    lo, hi = up(c.lo), up(c.hi)
    moves = None
    if c.moves:
        moves = (up(c.codes), up(c.read_frames), 5, c.frame_base)
    nframes = len(c.codes) if c.moves else 0
    bcap = c.base_capacity if c.new_base_capacity is None else c.new_base_capacity
    fcap = nframes if c.new_frame_capacity is None else c.new_frame_capacity
    t = demux.trim_reads(codec, decoded, lo, hi, qual=qual, moves=moves, capacity=c.new_base_capacity,
                         frame_capacity=c.new_frame_capacity)
    assert int(t.decoded.seq.numel()) == bcap and t.decoded.params is decoded.params and t.decoded.base_score is None
    host = lambda x: x.cpu().numpy()
    nb = len(want["seq"])
    assert np.array_equal(host(t.decoded.read_bases).view(np.uint64), want["read_bases"]), c.name
    assert np.array_equal(host(t.decoded.status), want["status"]), c.name
    assert np.array_equal(host(t.decoded.seq)[:nb], want["seq"]), c.name
    assert (t.qual is None) == (c.qual is None)
    if c.qual is not None:
        assert np.array_equal(host(t.qual)[:nb], want["qual"]), c.name
    if c.moves:
        nf = len(want["codes"])
        assert t.decoded.codes is t.codes and int(t.codes.numel()) == fcap
        assert np.array_equal(host(t.read_frames).view(np.uint64), want["read_frames"]), c.name
        assert np.array_equal(host(t.trim_frames).view(np.uint32), want["trim_frames"]), c.name
        assert np.array_equal(host(t.codes)[:nf], want["codes"]), c.name
        assert np.array_equal(host(t.decoded.base_frame).view(np.uint32)[:nb], want["base_frame"]), c.name
    else:
        assert t.codes is None and t.read_frames is None and t.trim_frames is None and t.decoded.base_frame is None

    # the C call into guarded views: the bytes, the base_frame values and the codes off 16-byte alignment
    g = dict(seq=Guarded(bcap, np.uint8, shift), qual=Guarded(bcap if c.qual is not None else 0, np.uint8, shift + 1),
             bf=Guarded(bcap if c.moves else 0, np.uint32, 4), rb=Guarded(n + 1, np.uint64, 8), st=Guarded(n, np.int32, 4),
             codes=Guarded(fcap if c.moves else 0, np.uint8, shift + 2), rf=Guarded(n + 1 if c.moves else 0, np.uint64, 8),
             cut=Guarded(n if c.moves else 0, np.uint32, 4))
    p = lambda x: x.data_ptr() if x is not None and x.numel() else 0
    with codec._launch(None) as ls:
        rc = codec._lib.pgn_trim_reads_device(
            codec._h, n, p(decoded.seq), p(qual), decoded.read_bases.data_ptr(), p(decoded.status), c.base_capacity, p(lo), p(hi),
            p(decoded.base_frame) if c.moves else 0, moves[1].data_ptr() if c.moves else 0, p(moves[0]) if c.moves else 0,
            c.frame_base, nframes, g["seq"].ptr, g["qual"].ptr, g["bf"].ptr, bcap, g["rb"].ptr, g["st"].ptr, g["codes"].ptr,
            fcap, g["rf"].ptr, g["cut"].ptr, ls.cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    g["seq"].check(want["seq"], f"{c.name} seq")
    g["rb"].check(want["read_bases"], f"{c.name} read_bases")
    g["st"].check(want["status"], f"{c.name} status")
    g["qual"].check(want["qual"] if c.qual is not None else [], f"{c.name} qual")
    if c.moves:
        g["bf"].check(want["base_frame"], f"{c.name} base_frame")
        g["codes"].check(want["codes"], f"{c.name} codes")
        g["rf"].check(want["read_frames"], f"{c.name} read_frames")
        g["cut"].check(want["trim_frames"], f"{c.name} trim_frames")
    return t


@pytest.mark.parametrize("name", [c.name for c in K.trim_cases()])
def test_trim_reads(codec, trim_cases, name):
    run_trim(codec, {c.name: c for c in trim_cases}[name], shift=len(name) % 13)


def test_trim_reads_every_alignment_of_the_outputs(codec, trim_cases):
    c = {c.name: c for c in trim_cases}["inside"]
    for shift in range(13):
        run_trim(codec, c, shift=shift)


# ---- refusals ------------------------------------------------------------------------------------------------
def test_python_refusals(codec, find_cases, trim_cases):
    import torch

    from rawnanoporesignalcompression_amd import demux

    c = {c.name: c for c in find_cases}["tie-ends"]
    decoded, pats = decoded_of(c), pattern_set(c)
    host_set = demux.PatternSet([b"ACG"], [0], 1)
    for kw in (dict(window=0), dict(window=1025), dict(patterns=host_set), dict(patterns=None)):
        args = dict(patterns=pats, window=8)
        args.update(kw)
        with pytest.raises(ValueError):
            demux.find_patterns(codec, decoded, **args)
    hits = demux.find_patterns(codec, decoded, pats, window=8)
    with pytest.raises(ValueError):
        demux.classify(codec, decoded, demux.PatternHits(hits.dist[:1], hits.start, hits.end), pats, 2)
    with pytest.raises(ValueError):
        demux.classify(codec, decoded, demux.PatternHits(hits.dist.float(), hits.start, hits.end), pats, 2)
    with pytest.raises(ValueError):
        demux.classify(codec, decoded, hits, pats, -1)
    t = {c.name: c for c in trim_cases}["inside"]
    d = decoded_of(t, t.base_frame)
    lo, hi, codes, rf = up(t.lo), up(t.hi), up(t.codes), up(t.read_frames)
    for kw in (dict(lo=lo[:-1]), dict(hi=hi.cpu()), dict(qual=up(t.qual)[:-1]), dict(moves=(codes, rf)), dict(moves=(codes, rf, 0)),
               dict(moves=(codes, rf[:-1], 5)), dict(moves=(codes.float(), rf, 5)), dict(capacity=-1)):
        args = dict(lo=lo, hi=hi)
        args.update(kw)
        with pytest.raises(ValueError):
            demux.trim_reads(codec, d, args.pop("lo"), args.pop("hi"), **args)
    with pytest.raises(ValueError):                                 # moves need base_frame
        demux.trim_reads(codec, decoded_of(t), lo, hi, moves=(codes, rf, 5))


def test_the_refusals_come_in_the_headers_order(codec):
    """On a real context: a later fault never hides an earlier one, and a refused call leaves the context usable."""
    import torch

    from rawnanoporesignalcompression_amd import _native

    lib, h, bad = codec._lib, codec._h, _native.PGN_ERR_INVALID_ARG
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    d = buf.data_ptr()

    def find(n=2, seq=d, rb=d, st=d, cap=16, window=8, P=2, pat=d, pcap=8, off=d, side=d, md=d, dist=d + 512, start=d + 640,
             end=d + 768):
        return lib.pgn_find_patterns_device(h, n, seq, rb, st, cap, window, P, pat, pcap, off, side, md, dist, start, end, None)

    for kw in (dict(window=0), dict(window=1025), dict(P=0), dict(P=4097), dict(n=1 << 32), dict(off=0), dict(side=0), dict(md=0),
               dict(pat=0), dict(rb=0), dict(st=0), dict(dist=0), dict(start=0), dict(end=0), dict(seq=0)):
        assert find(**kw) == bad, kw
    assert find() == 0                                             # zeros: two empty reads, nothing searched
    torch.cuda.synchronize()
    assert (buf[512:528] == 0xFF).all() and not buf[528:640].any() and (buf[768:784] == 0xFF).all() and not buf[:512].any()

    def classify(n=2, rb=d, st=d, P=2, side=d, md=d, cls=d, dist=d, bc=d + 1024, hi=d + 1280):
        return lib.pgn_classify_reads_device(h, n, rb, st, 16, P, side, md, cls, 1, 1, dist, d, d, bc, d + 1088, d + 1152, d + 1216,
                                             hi, None)

    for kw in (dict(P=0), dict(P=4097), dict(n=1 << 32), dict(side=0), dict(md=0), dict(cls=0), dict(rb=0), dict(st=0), dict(dist=0),
               dict(bc=0), dict(hi=0)):
        assert classify(**kw) == bad, kw
    assert classify() == 0
    torch.cuda.synchronize()
    assert (buf[1024:1032] == 0xFF).all() and not buf[1280:1288].any()    # two reads that are not taken

    def trim(n=2, seq=d, qual=0, rb=d, st=d, cap=16, lo=d, hi=d, bf=0, rf=0, codes=0, ncap=16, nseq=d + 1536, nrb=d + 2048,
             nst=d + 3072):
        return lib.pgn_trim_reads_device(h, n, seq, qual, rb, st, cap, lo, hi, bf, rf, codes, 0, 0, nseq, 0, 0, ncap, nrb, nst, 0, 0,
                                         0, 0, None)

    for kw in (dict(n=1 << 32), dict(nrb=0), dict(rb=0), dict(lo=0), dict(nst=0), dict(seq=0), dict(nseq=0)):
        assert trim(**kw) == bad, kw
    assert trim() == 0
    torch.cuda.synchronize()
    assert not buf[2048:2048 + 24].any()                          # the scan of three zeros
