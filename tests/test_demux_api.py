"""Adapters and barcodes (pgn_find_patterns_device, pgn_classify_reads_device, pgn_trim_reads_device): the C ABI
surface, the refusals, the rule's text, the Python module and the three host models, without a GPU.

The search model is held to the brute-force checker of tests/_demux_cases.py on every case and to the rule's
invariants; the class model to results written by hand; the slice to the move table's own arithmetic.  Mutants of
the rule, in the manner of tests/test_bgzf_deflate_api.py, show that the case list tells each of them from the
rule: a mutant that no case catches fails the test.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _demux_cases as K
from rawnanoporesignalcompression_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FNS = ("pgn_find_patterns_device", "pgn_classify_reads_device", "pgn_trim_reads_device")
NONE = K.NONE


def _header(comments=False):
    src = open(os.path.join(ROOT, "include", "pgnano_hip.h")).read()
    return src if comments else re.sub(r"/\*.*?\*/", "", src, flags=re.S)


@pytest.fixture(scope="module")
def find_cases():
    return K.find_cases()


@pytest.fixture(scope="module")
def class_cases():
    return K.class_cases()


@pytest.fixture(scope="module")
def trim_cases():
    return K.trim_cases()


# ---- surface -------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_bound():
    import rawnanoporesignalcompression_amd as pkg
    from rawnanoporesignalcompression_amd import _native, demux

    lib = _native.load()
    sigs = {s[0]: s for s in _native.SIGNATURES}
    for fn, nargs in zip(FNS, (17, 20, 25)):
        assert re.search(r"\bint\s+" + fn + r"\s*\(", _header())
        assert hasattr(lib, fn)
        assert sigs[fn][1] is C.c_int and len(sigs[fn][2]) == nargs
    for name in ("PatternSet", "barcode_patterns", "adapter_patterns", "revcomp", "find_patterns", "classify", "trim_reads",
                 "PatternHits", "ReadClasses", "TrimmedReads", "find_patterns_signal", "classify_signal", "trim_reads_signal"):
        assert name in demux.__all__ and hasattr(demux, name)
        assert name not in pkg.__all__                      # the package's own surface stays as it is
    for name in ("find_patterns_signal", "classify_signal", "trim_reads_signal"):
        assert getattr(demux, name) is getattr(host, name)
    for name in ("find_patterns", "classify", "trim_reads"):
        assert not hasattr(pkg.PGNanoCodec, name)
    assert _native.PGN_PATTERN_NO_CLASS == _native.PGN_DEMUX_NONE == 0xFFFFFFFF
    for name, value in (("PGN_DEMUX_NONE", "0xFFFFFFFFu"), ("PGN_PATTERN_NO_CLASS", "0xFFFFFFFFu"), ("PGN_DEMUX_MAX_WINDOW", "1024u"),
                        ("PGN_DEMUX_MAX_PATTERNS", "4096u"), ("PGN_DEMUX_MAX_PATTERN_BYTES", "128u")):
        assert re.search(r"#define\s+" + name + r"\s+" + value + r"\b", _header()), name
    src = open(os.path.join(ROOT, "rawnanoporesignalcompression_amd", "csrc", "pgn_kernels.hip")).read()
    assert '#include "pgn_demux.h"' in src


def test_call_refusals_and_their_order():
    """Each refusal with every later argument bad as well would say nothing of the order, so each call below has one
    fault and, where the header's order matters, a second, later one that must not be reached first: all return
    PGN_ERR_INVALID_ARG before the context is looked at (the context here is not one)."""
    from rawnanoporesignalcompression_amd import _native

    lib = _native.load()
    bad = _native.PGN_ERR_INVALID_ARG
    d = C.c_void_p(0x1000)

    def find(ctx=d, n=3, seq=d, rb=d, st=d, cap=100, window=150, P=4, pat=d, pcap=40, off=d, side=d, md=d, dist=d, start=d, end=d):
        return lib.pgn_find_patterns_device(ctx, n, seq, rb, st, cap, window, P, pat, pcap, off, side, md, dist, start, end, None)

    assert find(ctx=None) == bad
    for window in (0, 1025, 1 << 31):
        assert find(window=window) == bad
    for P in (0, 4097):
        assert find(P=P) == bad
    assert find(n=1 << 32) == bad
    for name in ("off", "side", "md", "pat", "rb", "st", "dist", "start", "end", "seq"):
        assert find(**{name: None}) == bad, name
    assert find(pat=None, pcap=0, n=0) == _native.PGN_OK          # no bytes, no reads: nothing is touched
    assert find(n=0, seq=None, cap=0, rb=None, st=None, dist=None, start=None, end=None) == _native.PGN_OK
    assert find(n=0, off=None) == bad                               # ... but the patterns are still asked for
    assert find(n=0, window=0) == bad

    def classify(ctx=d, n=3, rb=d, st=d, cap=100, P=4, side=d, md=d, cls=d, ncls=2, sep=1, dist=d, start=d, end=d, bc=d,
                 best=d, second=d, lo=d, hi=d):
        return lib.pgn_classify_reads_device(ctx, n, rb, st, cap, P, side, md, cls, ncls, sep, dist, start, end, bc, best,
                                             second, lo, hi, None)

    assert classify(ctx=None) == bad
    for P in (0, 4097):
        assert classify(P=P) == bad
    assert classify(n=1 << 32) == bad
    for name in ("side", "md", "cls", "rb", "st", "dist", "start", "end", "bc", "best", "second", "lo", "hi"):
        assert classify(**{name: None}) == bad, name
    assert classify(n=0, rb=None, st=None, dist=None, start=None, end=None, bc=None, best=None, second=None, lo=None,
                    hi=None) == _native.PGN_OK
    assert classify(n=0, cls=None) == bad

    def trim(ctx=d, n=3, seq=d, qual=d, rb=d, st=d, cap=100, lo=d, hi=d, bf=d, rf=d, codes=d, fbase=0, fcap=200, nseq=d, nqual=d,
             nbf=d, ncap=100, nrb=d, nst=d, ncodes=d, nfcap=200, nrf=d, cut=d):
        return lib.pgn_trim_reads_device(ctx, n, seq, qual, rb, st, cap, lo, hi, bf, rf, codes, fbase, fcap, nseq, nqual, nbf,
                                         ncap, nrb, nst, ncodes, nfcap, nrf, cut, None)

    assert trim(ctx=None) == bad
    assert trim(n=1 << 32) == bad
    for name in ("nrb", "nrf", "rb", "st", "lo", "hi", "nst", "cut", "seq", "bf", "codes", "nseq", "nqual", "nbf", "ncodes"):
        assert trim(**{name: None}) == bad, name
    # without moves (no read_frames) the frame arguments are not looked at, so a fault behind them is still found
    assert trim(rf=None, bf=None, codes=None, nrf=None, cut=None, nbf=None, ncodes=None, nseq=None) == bad
    assert trim(rf=None, bf=None, codes=None, nrf=None, cut=None, nbf=None, ncodes=None, nrb=None) == bad


def test_the_header_carries_the_rule():
    text = re.sub(r"\s+\*\s+", " ", _header(comments=True))
    at = text.index("---- Adapters and barcodes")
    text = text[at:text.index("#define PGN_DEMUX_NONE", at)]
    for phrase in ("pgn_find_patterns_device", "pgn_classify_reads_device", "pgn_trim_reads_device",
                   "x == 'N' or x == y", "D[0][j] = 0", "D[i][0] = i", "the lowest j that attains it", "R[0][q] = q",
                   "start = end - q*", "the largest start", "dist = L and end = w0", "no case folding", "ties to the lowest c",
                   "d_second - d_best >= min_sep", "If lo >= hi the read stays whole", "f_lo <= f_hi <= F",
                   "PGN_ERR_DST_TOO_SMALL", "PGN_ERR_INVALID_ARG before any GPU call, in this order", "Not covered",
                   "BC:Z", "read splitting", "affine gaps", "IUPAC", "direct RNA", "kit definitions", "no host wait"):
        assert phrase in text, phrase
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "Adapters and barcodes" in readme and readme.index("BGZF deflate") < readme.index("Adapters and barcodes")


# ---- the Python module ---------------------------------------------------------------------------------------
def test_revcomp_and_the_pattern_builders():
    from rawnanoporesignalcompression_amd import demux

    assert demux.revcomp("ACGTN") == b"NACGT"
    assert demux.revcomp(b"AAGGCT") == b"AGCCTT"
    assert demux.revcomp("acgU") == b"Acgt"
    assert demux.revcomp(b"") == b""
    s = demux.barcode_patterns("GGT", ["AAAC", "CCCA"], "TTG", max_dist=3)
    assert s.patterns == [b"GGTAAACTTG", b"CAAGTTTACC", b"GGTCCCATTG", b"CAATGGGACC"]
    assert s.side.tolist() == [0, 1, 0, 1] and s.pclass.tolist() == [0, 0, 1, 1] and s.max_dist.tolist() == [3] * 4
    assert s.pat.tobytes() == b"".join(s.patterns) and s.pat_off.tolist() == [0, 10, 20, 30, 40]
    head = demux.barcode_patterns("GGT", ["AAAC", "CCCA"], "TTG", max_dist=[2, 5], tail=False)
    assert head.patterns == [b"GGTAAACTTG", b"GGTCCCATTG"] and head.side.tolist() == [0, 0] and head.max_dist.tolist() == [2, 5]
    a = demux.adapter_patterns(head=["ACGTAC"], tail=[b"TTTT", "GG"], max_dist=1)
    assert a.patterns == [b"ACGTAC", b"TTTT", b"GG"] and a.side.tolist() == [0, 1, 1]
    assert a.pclass.tolist() == [demux.PATTERN_NO_CLASS] * 3
    both = s + a
    assert len(both) == 7 and both.patterns == s.patterns + a.patterns
    assert both.pat_off.tolist() == [0, 10, 20, 30, 40, 46, 50, 52] and both.pclass.tolist()[3:5] == [1, demux.PATTERN_NO_CLASS]
    assert both.pat_off.dtype == np.uint32 and both.side.dtype == np.uint8 and both.device is None


def test_pattern_set_refusals():
    from rawnanoporesignalcompression_amd import demux

    for args in (([b""], [0], 1), ([b"A" * 129], [0], 1), ([b"ACG"], [2], 1), ([b"ACG"], [0, 1], 1), ([], [], 1),
                 ([b"A"] * 4097, 0, 1), ([b"ACG"], [0], -1), ([b"ACG"], [0], 1, [1 << 32])):
        with pytest.raises(ValueError):
            demux.PatternSet(*args)
    assert len(demux.PatternSet([b"A" * 128, "N"], [0, 1], 128)) == 2
    raw = demux.PatternSet.from_arrays(np.zeros(200, np.uint8), [0, 0, 129, 132], [0, 1, 7], [1, 1, 1], [0, 0, 0])
    assert [len(p) for p in raw.patterns] == [0, 129, 3]        # nothing refused: the device does not search them
    with pytest.raises(ValueError):
        demux.PatternSet.from_arrays(np.zeros(8, np.uint8), [0, 4], [0, 1], [1, 1], [0, 0])


def test_python_model_refusals():
    with pytest.raises(ValueError):
        host.find_patterns_signal(b"ACGT", [0, 4], [0], [b"AC"], [0], [1], window=0)
    with pytest.raises(ValueError):
        host.find_patterns_signal(b"ACGT", [0, 4], [0], [b"AC"], [0], [1], window=1025)
    with pytest.raises(ValueError):
        host.find_patterns_signal(b"ACGT", [0, 4], [0], [], [], [])
    with pytest.raises(ValueError):
        host.find_patterns_signal(b"ACGT", [0, 4], [0], [b"AC"], [0, 1], [1])
    with pytest.raises(ValueError):
        host.find_patterns_signal(b"ACGT", [0, 4], [0, 0], [b"AC"], [0], [1])
    z = np.zeros((1, 1), np.uint32)
    with pytest.raises(ValueError):
        host.classify_signal(z, z, np.zeros((1, 2), np.uint32), [0, 4], [0], [0], [1], [0], 1)
    with pytest.raises(ValueError):
        host.trim_reads_signal(b"ACGT", [0, 4], [0], [0, 0], [4])
    with pytest.raises(ValueError):
        host.trim_reads_signal(b"ACGT", [0, 4], [0], [0], [4], moves=(np.zeros(8, np.uint8), [0, 8], 5))


# ---- the search ----------------------------------------------------------------------------------------------
def test_the_search_model_equals_the_brute_force_checker(find_cases):
    for c in find_cases:
        want, got = K.brute_find(c), c.expected()
        for name, a, b in zip(("dist", "start", "end"), want, got):
            assert b.dtype == np.uint32 and b.shape == (len(c.status), len(c.patterns))
            assert np.array_equal(a, b), (c.name, name, a.tolist(), b.tolist())


def test_the_search_models_invariants(find_cases):
    hits = 0
    for c in find_cases:
        dist, start, end = c.expected()
        for r in range(len(c.status)):
            b0, b1 = int(c.read_bases[r]), int(c.read_bases[r + 1])
            taken = c.status[r] == 0 and b0 < b1 <= c.base_capacity
            for p, pat in enumerate(c.patterns):
                d, s, e = int(dist[r, p]), int(start[r, p]), int(end[r, p])
                if not taken or c.sides[p] not in (0, 1) or not 1 <= len(pat) <= 128:
                    assert (d, s, e) == (NONE, NONE, NONE)
                    continue
                m = b1 - b0
                n = min(m, c.window)
                w0 = m - n if c.sides[p] else 0
                assert d <= len(pat) and w0 <= e <= w0 + n
                assert (s != NONE) == (d <= c.max_dist[p])
                if d == len(pat):
                    assert e == w0
                if s != NONE:
                    hits += 1
                    assert w0 <= s <= e
                    assert K.lev_ends(pat, c.seq[b0 + s:b0 + e].tobytes())[-1] == d
    assert hits > 100


def test_the_case_list_covers_the_issue(find_cases, class_cases, trim_cases):
    tags = set().union(*(c.tags for c in find_cases))
    assert {"seam", "P1", "n", "w0", "align", "tie-end", "tie-start", "dist-L", "edge", "max-dist", "N", "odd", "case", "P65",
            "one-side", "P257", "mixed", "bad", "taken", "nreads0", "fuzz"} <= tags
    lengths = {len(p) for c in find_cases for p in c.patterns}
    assert {1, 2, 63, 64, 65, 127, 128} <= lengths
    by = {c.name: c for c in find_cases}
    assert len(by) == len(find_cases)
    seam_ops = {(len(c.patterns[0]), c.name.split("-")[2]) for c in find_cases if "seam" in c.tags}
    for L in (65, 66):
        assert {(L, op + str(k)) for op in ("sub", "ins", "del") for k in (62, 63, 64)} <= seam_ops
    assert any(L == 128 for L, _ in seam_ops) and any(L == 127 for L, _ in seam_ops)
    assert {c.sides[0] for c in find_cases if "seam" in c.tags} == {0, 1}     # the anchored pass crosses the boundary too
    # both sides of a hit: max_dist == dist and dist - 1
    d, s, _ = by["max-dist"].expected()
    assert d[0].tolist() == [2, 2, 2, 2] and [v != NONE for v in s[0].tolist()] == [True, False, True, False]
    # the long read's tail window starts at 4,850
    d, s, e = by["long-read"].expected()
    assert (d[0, 0], s[0, 0], e[0, 0]) == (0, 40, 64) and (d[0, 1], s[0, 1], e[0, 1]) == (1, 4964, 4988) and s[0, 2] == NONE
    # ties: the lowest end and the largest start
    d, s, e = by["tie-ends"].expected()
    assert (d[0, 0], s[0, 0], e[0, 0]) == (0, 0, 3) and (d[0, 1], s[0, 1], e[0, 1]) == (0, 0, 3)
    d, s, e = by["tie-starts"].expected()
    assert (d[0, 0], s[0, 0], e[0, 0]) == (0, 0, 3) and (d[1, 2], s[1, 2], e[1, 2]) == (1, 2, 4)
    d, s, e = by["no-match"].expected()
    assert (d[0, 0], s[0, 0], e[0, 0]) == (3, 0, 0) and (d[0, 1], s[0, 1], e[0, 1]) == (3, 2, 2) and (d[0, 2], s[0, 2], e[0, 2]) == (3, NONE, 2)
    d, s, e = by["window-ends"].expected()
    assert (d[0, 0], s[0, 0], e[0, 0]) == (0, 0, 9) and (d[0, 1], s[0, 1], e[0, 1]) == (0, 39, 48)
    d, s, e = by["lower-case"].expected()
    assert d[0, 0] == 4 and d[0, 1] == 4 and d[0, 2] == 0 and d[0, 3] == 2 and d[1, 0] == 0
    d, s, e = by["odd-bytes"].expected()
    assert d[0].tolist()[:3] == [0, 1, 0] and d[2].tolist()[5] == 2       # 'N' in the text matches 'N' alone
    d, _, _ = by["bad-patterns"].expected()
    assert d[0].tolist() == [0, NONE, NONE, NONE, NONE, 0]
    d, _, _ = by["not-taken"].expected()
    assert [row[0] != NONE for row in d.tolist()] == [True, False, False, True, False]
    assert by["empty"].expected()[0].shape == (0, 1)
    assert {c.name for c in class_cases} >= {"rules", "rules-sep0"} and len(trim_cases) >= 10


# ---- the class -----------------------------------------------------------------------------------------------
def test_the_class_model_on_rows_written_by_hand(class_cases):
    by = {c.name: c for c in class_cases}
    out = by["rules"].expected()
    for o in out:
        assert o.dtype == np.uint32 and o.shape == (len(K.CLASS_ROWS),)
    for r, (name, _, _, want) in enumerate(K.CLASS_ROWS):
        assert tuple(int(o[r]) for o in out) == want, name
    out = by["rules-sep0"].expected()                              # min_sep 0: every best class is the barcode
    rows = {row[0]: r for r, row in enumerate(K.CLASS_ROWS)}
    assert tuple(int(o[rows["tie-lowest-class"]]) for o in out) == (1, 1, 1, 30, 100)
    assert tuple(int(o[rows["tie-lowest-class-sep0"]]) for o in out) == (1, 1, 1, 30, 100)
    assert tuple(int(o[rows["sep-one-short"]]) for o in out) == (0, 1, 2, 22, 100)


def test_the_class_models_invariants(class_cases):
    for c in class_cases:
        barcode, best, second, lo, hi = (o.astype(np.int64) for o in c.expected())
        m = np.diff(c.read_bases)
        taken = (c.status == 0) & (m > 0) & (c.read_bases[1:] <= c.base_capacity)
        assert (barcode[~taken] == NONE).all() and (lo[~taken] == 0).all() and (hi[~taken] == 0).all()
        assert (lo[taken] < hi[taken]).all()
        assert ((barcode == NONE) | (barcode < c.nclasses)).all()
        assert (best <= second).all() and ((best != NONE) | (barcode == NONE)).all()
        named = barcode != NONE
        assert ((second[named] == NONE) | (second[named] - best[named] >= c.min_sep)).all()


# ---- the slice -----------------------------------------------------------------------------------------------
def test_the_slice_model_on_every_case(trim_cases):
    for c in trim_cases:
        out = c.expected()
        n = len(c.status)
        nrb = out["read_bases"].astype(np.int64)
        m = np.diff(c.read_bases)
        lo, hi = c.lo.astype(np.int64), c.hi.astype(np.int64)
        sliced = out["status"] <= 1
        sliced &= (c.status == 0)
        assert np.array_equal(np.diff(nrb), np.where(sliced, hi - lo, 0)), c.name
        assert (out["status"][(c.status != 0)] == c.status[c.status != 0]).all()
        assert (out["status"][(c.status == 0) & ((lo > hi) | (hi > m))] == 10).all()
        cap = c.new_base_capacity
        full = c.expected(cut=False)
        assert np.array_equal(out["read_bases"], full["read_bases"]), c.name          # the scans hold the full counts
        assert np.array_equal(out["seq"], full["seq"][:cap]) and len(out["seq"]) == min(int(nrb[-1]), len(full["seq"]) if cap is None else cap)
        for r in range(n):
            if sliced[r]:
                a = int(c.read_bases[r])
                assert np.array_equal(full["seq"][nrb[r]:nrb[r + 1]], c.seq[a + lo[r]:a + hi[r]])
                if c.qual is not None:
                    assert np.array_equal(full["qual"][nrb[r]:nrb[r + 1]], c.qual[a + lo[r]:a + hi[r]])
        if not c.moves:
            assert out["codes"] is None and out["read_frames"] is None and out["trim_frames"] is None and out["base_frame"] is None
            continue
        assert np.array_equal(out["read_frames"], full["read_frames"]) and np.array_equal(out["trim_frames"], full["trim_frames"])
        nrf = full["read_frames"].astype(np.int64)
        spoiled = c.name == "spoiled"
        for r in range(n):
            codes = full["codes"][nrf[r]:nrf[r + 1]]
            if not sliced[r]:
                assert len(codes) == 0 and out["trim_frames"][r] == 0
            elif not spoiled:
                # the kept frames emit exactly the kept bases, the first of them at frame 0, at the new base_frame
                at = np.flatnonzero(codes >> 7)
                assert len(at) == hi[r] - lo[r], (c.name, r)
                assert np.array_equal(at, full["base_frame"][nrb[r]:nrb[r + 1]]), (c.name, r)
                if len(at):
                    assert at[0] == 0
                    f0 = int(c.read_frames[r]) - c.frame_base + int(out["trim_frames"][r])
                    assert np.array_equal(codes, c.codes[f0:f0 + len(codes)])
    by = {c.name: c for c in trim_cases}
    assert by["spoiled"].expected()["status"].tolist() == [10, 0, 10, 0, 0, 10, 0, 10]
    assert by["edges"].expected()["status"].tolist() == [0, 0, 0, 0, 0, 0, 10, 10]
    assert by["frame-window"].expected()["status"].tolist() == [10, 0, 0, 0, 0, 0, 0, 10]
    assert by["not-taken"].expected()["status"].tolist() == [0, 6, 0, 1, 0, 0, 0, 10]
    assert by["base-capacity"].expected()["status"].tolist() == [0, 0, 1, 1, 1, 1, 1, 1]
    assert by["frame-capacity"].expected()["status"].tolist() == [0, 0, 0, 1, 1, 1, 1, 1]
    assert by["edges"].expected()["trim_frames"][0] == 0 and by["edges"].expected()["trim_frames"][2] > 0


# ---- mutants of the rule --------------------------------------------------------------------------------------
def _mutant_window(pat, text, m):
    """``(dist, j, q)`` of one pattern in one window by the rule's two tables, written out cell by cell, or by the
    rule with one change ``m``."""
    def match(x, y):
        if m == "N-not-wildcard":
            return x == y
        if m == "text-N-matches":
            return x == 78 or y == 78 or x == y
        return x == 78 or x == y

    def last_row(p, t, anchored):
        row = list(range(len(t) + 1)) if anchored else [0] * (len(t) + 1)
        for i, x in enumerate(p, 1):
            cur = [i]
            for j, y in enumerate(t, 1):
                cur.append(min(row[j - 1] + (not match(x, y)), row[j] + 1, cur[j - 1] + 1))
            row = cur
        return row

    last = last_row(pat, text, False)
    dist = min(last)
    ends = [j for j, v in enumerate(last) if v == dist]
    j = ends[-1] if m == "highest-end" else ends[0]
    back = last_row(pat[::-1], text[:j][::-1], True)
    qs = [q for q, v in enumerate(back) if v == dist]
    return dist, j, (qs[-1] if m == "smallest-start" else qs[0])


def _mutant_find(c, m):
    n, P = len(c.status), len(c.patterns)
    out = np.full((3, n, P), NONE, np.uint32)
    for r in range(n):
        b0, b1 = int(c.read_bases[r]), int(c.read_bases[r + 1])
        if c.status[r] != 0 or not b0 < b1 <= c.base_capacity:
            continue
        size = b1 - b0
        k = min(size, c.window)
        for p, pat in enumerate(c.patterns):
            if c.sides[p] not in (0, 1) or not 1 <= len(pat) <= 128:
                continue
            w0 = size - k if c.sides[p] else 0
            if m == "tail-off-by-one" and c.sides[p] and w0 > 0:
                w0 -= 1
            dist, j, q = _mutant_window(pat, c.seq[b0 + w0:b0 + w0 + k].tobytes(), m)
            out[0, r, p], out[2, r, p] = dist, w0 + j
            if dist <= c.max_dist[p]:
                out[1, r, p] = w0 + j - q
    return tuple(out)


def _mutant_classify(c, m):
    n, P = c.dist.shape
    out = np.full((5, n), NONE, np.uint32)
    out[3:] = 0
    for r in range(n):
        size = int(c.read_bases[r + 1] - c.read_bases[r])
        if c.status[r] != 0 or size <= 0 or c.read_bases[r + 1] > c.base_capacity:
            continue
        hits = [p for p in range(P) if c.sides[p] <= 1 and (c.classes[p] == K.NO_CLASS or c.classes[p] < c.nclasses)
                and c.dist[r, p] != NONE and c.dist[r, p] <= c.max_dist[p]]
        d = {}
        for p in hits:
            if c.classes[p] != K.NO_CLASS:
                d[int(c.classes[p])] = min(d.get(int(c.classes[p]), NONE), int(c.dist[r, p]))
        order = sorted((v, k) for k, v in d.items())
        barcode = NONE
        if order:
            out[1, r] = order[0][0]
            gap = order[1][0] - order[0][0] if len(order) > 1 else None
            if gap is not None:
                out[2, r] = order[1][0]
            if gap is None or (gap > c.min_sep if m == "sep-greater" else gap >= c.min_sep):
                barcode = order[0][1]
        out[0, r] = barcode
        trims = [p for p in hits if m == "loser-trims" or c.classes[p] == K.NO_CLASS or c.classes[p] == barcode]
        lo = max([int(c.end[r, p]) for p in trims if c.sides[p] == 0], default=0)
        hi = min([int(c.start[r, p]) for p in trims if c.sides[p] == 1], default=size)
        out[3, r], out[4, r] = (0, size) if lo >= hi else (lo, hi)
    return tuple(out)


def _mutant_frames(c, m):
    """``(read_frames, trim_frames)`` of a slice with moves by the rule, or with f_hi taken from the last kept base."""
    n = len(c.status)
    nrf, cut = np.zeros(n + 1, np.uint64), np.zeros(n, np.uint32)
    for r in range(n):
        b0, size = int(c.read_bases[r]), int(c.read_bases[r + 1] - c.read_bases[r])
        lo, hi = int(c.lo[r]), int(c.hi[r])
        f0, f1 = int(c.read_frames[r]), int(c.read_frames[r + 1])
        nrf[r + 1] = nrf[r]
        if c.status[r] != 0 or size <= 0 or b0 + size > c.base_capacity or not lo <= hi <= size:
            continue
        if not c.frame_base <= f0 <= f1 <= c.frame_base + len(c.codes):
            continue
        f_lo = f_hi = 0
        if lo < hi:
            f_lo = int(c.base_frame[b0 + lo])
            if m == "f_hi-from-last-base":
                f_hi = int(c.base_frame[b0 + hi - 1]) + 1
            else:
                f_hi = int(c.base_frame[b0 + hi]) if hi < size else f1 - f0
        if f_lo <= f_hi <= f1 - f0:
            nrf[r + 1] += np.uint64(f_hi - f_lo)
            cut[r] = f_lo
    return nrf, cut


FIND_MUTANTS = ("highest-end", "smallest-start", "N-not-wildcard", "text-N-matches", "tail-off-by-one")
CLASS_MUTANTS = ("sep-greater", "loser-trims")
TRIM_MUTANTS = ("f_hi-from-last-base",)


def test_mutants_of_the_rule_fail_on_the_cases(find_cases, class_cases, trim_cases):
    """The rule written out a second time equals the model on every case, and each mutant of it differs from the
    model on at least one: the case list tells every mutant from the rule."""
    same = lambda a, b: all(np.array_equal(x, y) for x, y in zip(a, b))
    seen = {}
    for c in find_cases:
        assert same(_mutant_find(c, None), c.expected()), c.name
        for m in FIND_MUTANTS:
            if not same(_mutant_find(c, m), c.expected()):
                seen.setdefault(m, []).append(c.name)
    for c in class_cases:
        assert same(_mutant_classify(c, None), c.expected()), c.name
        for m in CLASS_MUTANTS:
            if not same(_mutant_classify(c, m), c.expected()):
                seen.setdefault(m, []).append(c.name)
    for c in trim_cases:
        if not c.moves:
            continue
        want = c.expected()
        assert same(_mutant_frames(c, None), (want["read_frames"], want["trim_frames"])), c.name
        for m in TRIM_MUTANTS:
            if not same(_mutant_frames(c, m), (want["read_frames"], want["trim_frames"])):
                seen.setdefault(m, []).append(c.name)
    for m in FIND_MUTANTS + CLASS_MUTANTS + TRIM_MUTANTS:
        assert seen.get(m), f"no case tells the mutant {m} from the rule"
    # the explicit tie cases catch their mutants, not the fuzz alone
    assert "tie-ends" in seen["highest-end"] and "tie-starts" in seen["smallest-start"]
    assert "lower-case" in seen["N-not-wildcard"] and "odd-bytes" in seen["text-N-matches"]
    assert "window-ends" in seen["tail-off-by-one"] and "rules" in seen["sep-greater"] and "rules" in seen["loser-trims"]
