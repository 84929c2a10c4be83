"""Stitched frames to bases (pgn_ctc_decode_device / pgn_collapse_codes_device): the C ABI surface, the
refusals in their order and the rule itself, without a GPU.

The rule (include/pgnano_hip.h), for one read's frames i = 0..F-1 of C scores each:
  label     l_i = argmax of scores_i as numpy computes it: IEEE comparison (-0 == +0), the lowest index wins a
            tie, a NaN beats every number and the first NaN wins
  emission  frame i emits iff l_i != blank and (i == 0 or l_i != l_{i-1})
  code      l_i | 0x80 if the frame emits, else l_i
  bases     alphabet[l_i], i and (float32)scores_i[l_i] of the emitting frames in frame order
ref_decode below is that text with Python loops, one frame and one class at a time; ctc_decode_signal (the
package's numpy form, which the GPU tests compare the device with) must agree with it everywhere.
"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECODE, COLLAPSE = "pgn_ctc_decode_device", "pgn_collapse_codes_device"
NAN, INF = float("nan"), float("inf")


def ref_argmax(row):
    """The label of one frame: Python floats hold float16 and float32 values exactly."""
    best, bv = 0, float(row[0])
    for c in range(1, len(row)):
        v = float(row[c])
        if math.isnan(bv):
            break                       # the first NaN wins
        if math.isnan(v) or v > bv:     # a NaN beats every number; a tie (and -0 against +0) keeps the lower index
            best, bv = c, v
    return best


def ref_collapse(codes, alphabet):
    seq, at = [], []
    for i, code in enumerate(codes):
        if code & 0x80:
            seq.append(alphabet[code & 0x7F])
            at.append(i)
    return bytes(seq), at


def ref_decode(scores, alphabet, blank):
    """(seq bytes, [frame], [score], [code]) of one read by the header's text."""
    codes, prev = [], None
    for i in range(len(scores)):
        l = ref_argmax(scores[i])
        emit = l != blank and (i == 0 or l != prev)
        codes.append(l | 0x80 if emit else l)
        prev = l
    seq, at = ref_collapse(codes, alphabet)
    return seq, at, [np.float32(scores[i][codes[i] & 0x7F]) for i in at], codes


def check_signal(scores, alphabet, blank):
    from rawnanoporesignalcompression_amd import ctc_decode_signal

    seq, at, score, codes = ctc_decode_signal(scores, alphabet, blank)
    wseq, wat, wscore, wcodes = ref_decode(scores, alphabet.encode() if isinstance(alphabet, str) else alphabet, blank)
    assert (seq.dtype, at.dtype, score.dtype, codes.dtype) == (np.uint8, np.uint32, np.float32, np.uint8)
    assert codes.tolist() == wcodes
    assert seq.tobytes() == wseq and at.tolist() == wat
    assert np.array_equal(score.view(np.uint32), np.array(wscore, np.float32).view(np.uint32))
    return seq.tobytes(), at.tolist()


# ---- surface -------------------------------------------------------------------------------------
def _header():
    src = open(os.path.join(ROOT, "include", "pgnano_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_symbols_declared_exported_and_bound():
    from rawnanoporesignalcompression_amd import _native

    lib = _native.load()
    sigs = {s[0]: s for s in _native.SIGNATURES}
    for name, nargs in ((DECODE, 16), (COLLAPSE, 13)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", _header())
        assert hasattr(lib, name)
        assert sigs[name][1] is C.c_int and len(sigs[name][2]) == nargs
    m = re.search(r"#define\s+PGN_CTC_TILE_FRAMES\s+(\d+)", _header())
    assert m and int(m.group(1)) == _native.PGN_CTC_TILE_FRAMES and _native.PGN_CTC_TILE_FRAMES % 64 == 0


def test_the_header_carries_the_rule():
    src = open(os.path.join(ROOT, "include", "pgnano_hip.h")).read()
    for text in ("frame i emits a base iff l_i != blank and (t == 0 or l_i != l_{i-1})",
                 "code_i = l_i | 0x80 if the frame emits, else l_i",
                 "seq[g] = alphabet[l_i], base_frame[g] = t, base_score[g] = (float)scores_i[l_i]",
                 "frame_base <= read_frames[r] <= read_frames[r+1] <= frame_base + frame_capacity",
                 "the lowest", "a NaN beats every number and the first NaN wins",
                 "Not covered: decoding itself"):   # the stitch section keeps its text
        assert text in src, text


def test_struct_layout():
    from rawnanoporesignalcompression_amd import _native

    assert re.search(r"typedef struct pgn_ctc_params \{", _header())
    S = _native.CtcParams
    assert C.sizeof(S) == 80
    assert [(f, getattr(S, f).offset) for f, _ in S._fields_] == [("classes", 0), ("blank", 4), ("score_type", 8),
                                                                  ("pad", 12), ("alphabet", 16)]


BAD_PARAMS = [(1, 0, 2, 0), (0, 0, 2, 0), (65, 0, 2, 0), (5, 5, 2, 0), (5, 64, 2, 0), (5, 0, 0, 0), (5, 0, 3, 0),
              (5, 0, 2, 1)]  # (classes, blank, score_type, pad)


def _params(classes=5, blank=0, score_type=2, pad=0):
    from rawnanoporesignalcompression_amd import _native

    return _native.CtcParams(classes, blank, score_type, pad, (C.c_uint8 * 64)(*b"NACGT"))


def test_decode_call_refusals_and_their_order():
    """Every refusal is PGN_ERR_INVALID_ARG with dummy pointers: nothing is dereferenced and no device is touched
    (this runs without one).  The order is shown by calls that break two rules at once and are refused whether
    or not the later rule's condition (nreads > 0, frame_capacity > 0, base_capacity > 0) holds."""
    from rawnanoporesignalcompression_amd import _native

    fn = getattr(_native.load(), DECODE)
    bad = _native.PGN_ERR_INVALID_ARG
    dummy = C.c_void_p(0x1000)

    def call(ctx=dummy, p=_params(), nreads=1, rf=dummy, frames=dummy, stride=10, base=0, fcap=8, seq=dummy, bcap=8,
             rb=dummy, st=dummy, bf=None, bs=None, codes=None):
        return fn(ctx, C.byref(p) if p is not None else None, nreads, rf, frames, stride, base, fcap, seq, bcap, rb, st,
                  bf, bs, codes, None)

    assert call(ctx=None) == bad                                    # 1
    assert call(p=None) == bad
    for prm in BAD_PARAMS:                                          # 2
        assert call(p=_params(*prm)) == bad, prm
        assert call(p=_params(*prm), nreads=0, fcap=0, bcap=0, rf=None, st=None, frames=None, seq=None) == bad, prm
    assert call(stride=8) == bad                                    # 3: below C * 2
    assert call(stride=11) == bad                                   #    no multiple of the element size
    assert call(frames=C.c_void_p(0x1001)) == bad
    assert call(p=_params(score_type=1), stride=18) == bad          #    float32: below C * 4
    assert call(p=_params(score_type=1), stride=22) == bad
    assert call(p=_params(score_type=1), stride=20, frames=C.c_void_p(0x1002)) == bad
    assert call(stride=8, nreads=0, fcap=0, bcap=0) == bad          #    ... before anything about the arrays
    assert call(nreads=1 << 32) == bad                              # 4
    assert call(fcap=1 << 40) == bad
    assert call(rb=None) == bad                                     # 5
    assert call(rb=None, nreads=0) == bad
    assert call(rf=None) == bad                                     # 6
    assert call(st=None) == bad
    assert call(frames=None) == bad                                 # 7
    assert call(seq=None) == bad                                    # 8
    # what the order lets through up to the first GPU call is shown by the NULL context alone being refused
    # first: every later rule broken as well
    assert call(ctx=None, p=_params(*BAD_PARAMS[0]), stride=1, nreads=1 << 32, rb=None, rf=None, frames=None, seq=None) == bad


def test_collapse_call_refusals():
    from rawnanoporesignalcompression_amd import _native

    fn = getattr(_native.load(), COLLAPSE)
    bad = _native.PGN_ERR_INVALID_ARG
    dummy = C.c_void_p(0x1000)
    table = (C.c_uint8 * 128)(*b"NACGT")

    def call(ctx=dummy, alphabet=table, nreads=1, rf=dummy, codes=dummy, base=0, fcap=8, seq=dummy, bcap=8, rb=dummy,
             st=dummy, bf=None):
        return fn(ctx, C.byref(alphabet) if alphabet is not None else None, nreads, rf, codes, base, fcap, seq, bcap, rb,
                  st, bf, None)

    assert call(ctx=None) == bad
    assert call(alphabet=None) == bad
    assert call(nreads=1 << 32) == bad
    assert call(fcap=1 << 40) == bad
    assert call(rb=None) == bad
    assert call(rb=None, nreads=0) == bad
    assert call(rf=None) == bad
    assert call(st=None) == bad
    assert call(codes=None) == bad
    assert call(seq=None) == bad


def test_python_parameter_helper():
    from rawnanoporesignalcompression_amd import _native, ctc_decode_signal, ctc_params

    p = ctc_params(5)
    assert (p.classes, p.blank, p.score_type, p.pad, bytes(p.alphabet)[:5]) == (5, 0, _native.PGN_OUT_F16, 0, b"NACGT")
    p = ctc_params(3, 2, b"xy-", np.float32)
    assert (p.classes, p.blank, p.score_type, bytes(p.alphabet)[:3]) == (3, 2, _native.PGN_OUT_F32, b"xy-")
    for args in ((1, 0, "N"), (65, 0, "N" * 65), (5, 5), (5, -1), (5, 0, "NACG"), (5, 0, "NACGT", np.float64)):
        with pytest.raises(ValueError):
            ctc_params(*args)
    with pytest.raises(ValueError):
        ctc_decode_signal(np.zeros(5, np.float16))
    empty = ctc_decode_signal(np.zeros((0, 5), np.float16))
    assert [a.size for a in empty] == [0, 0, 0, 0]


# ---- the rule --------------------------------------------------------------------------------------
def one_hot(labels, C_=5, dtype=np.float16):
    x = np.zeros((len(labels), C_), dtype)
    x[np.arange(len(labels)), labels] = 1
    return x


def test_hand_worked_examples():
    """Spelled out: classes N A C G T, blank 0."""
    # A A - A C C - -  T : the repeat split by a blank gives two A, the run of C one
    assert check_signal(one_hot([1, 1, 0, 1, 2, 2, 0, 0, 4]), "NACGT", 0) == (b"AACT", [0, 3, 4, 8])
    # all blank; no blank at all (every change of label is a base)
    assert check_signal(one_hot([0, 0, 0, 0]), "NACGT", 0) == (b"", [])
    assert check_signal(one_hot([1, 2, 2, 3, 1, 1, 4]), "NACGT", 0) == (b"ACGAT", [0, 1, 3, 4, 6])
    # another blank position: class 4 emits nothing, class 0 does
    assert check_signal(one_hot([0, 0, 4, 0, 3]), "NACGT", 4) == (b"NNG", [0, 3, 4])
    # ties: the lowest index wins -- all equal is class 0 (blank); A and G equal is A
    x = np.array([[2, 2, 2, 2, 2], [0, 3, 1, 3, 0], [0, 1, 1, 3, 3]], np.float16)
    assert check_signal(x, "NACGT", 0) == (b"AG", [1, 2])
    # -0 == +0: a tie that class 0 wins, and +0 does not beat -0 later
    x = np.array([[-0.0, 0.0, -1, -1, -1], [-1, -0.0, 0.0, -1, -1]], np.float32)
    assert check_signal(x, "NACGT", 0) == (b"A", [1])
    # NaN beats every number, +inf included; the first NaN wins
    x = np.array([[INF, 1, NAN, NAN, 0], [NAN, INF, 0, 0, NAN], [0, 0, 0, 0, NAN], [-INF, -INF, -INF, 5, -INF],
                  [-INF, -INF, -INF, -INF, -INF], [0, INF, INF, 0, 0]], np.float16)
    assert check_signal(x, "NACGT", 0) == (b"CTGA", [0, 2, 3, 5])


def test_numpy_rule_is_the_headers_text():
    """ctc_decode_signal against ref_decode on random scores from a small set of values (ties are common) with
    NaN, the two zeros and the infinities mixed in, for both types, several C and every blank position."""
    values = np.array([-2, -1, -0.0, 0.0, 1, 2, 3, INF, -INF, NAN], np.float32)
    rng = np.random.default_rng(3)
    for C_ in (2, 3, 5, 41, 64):
        for dtype in (np.float16, np.float32):
            for blank in sorted({0, 1, C_ // 2, C_ - 1}):
                for F in (1, 2, 37, 300):
                    special = rng.random((F, C_)) < 0.15
                    x = np.where(special, values[rng.integers(0, len(values), (F, C_))],
                                 values[rng.integers(0, 7, (F, C_))]).astype(dtype)
                    path = np.repeat(rng.integers(0, C_, F), rng.integers(1, 4, F))[:F]
                    x[np.arange(F), path] += (rng.random(F) < 0.7) * dtype(2)
                    alphabet = bytes(rng.integers(33, 127, C_).astype(np.uint8))
                    check_signal(x, alphabet, blank)


def test_collapse_codes_signal():
    from rawnanoporesignalcompression_amd import collapse_codes_signal

    # two emitting frames of one class in a row give two bases; class bits up to 127
    alphabet = bytes(range(128, 256))
    codes = [0x81, 0x81, 0x01, 0x80 | 127, 0x7F, 0x80, 0x80 | 64, 0x80 | 64]
    seq, at = collapse_codes_signal(codes, alphabet)
    assert seq.tolist() == [129, 129, 255, 128, 192, 192] and at.tolist() == [0, 1, 3, 5, 6, 7]
    assert at.dtype == np.uint32 and seq.dtype == np.uint8
    rng = np.random.default_rng(4)
    for n in (0, 1, 500):
        codes = rng.integers(0, 256, n).astype(np.uint8)
        seq, at = collapse_codes_signal(codes, alphabet)
        wseq, wat = ref_collapse(codes.tolist(), alphabet)
        assert seq.tobytes() == wseq and at.tolist() == wat
    short, _ = collapse_codes_signal([0x81, 0x85], "NACGT")  # entries the alphabet does not name are 0
    assert short.tolist() == [65, 0]
    with pytest.raises(ValueError):
        collapse_codes_signal([1], bytes(129))
