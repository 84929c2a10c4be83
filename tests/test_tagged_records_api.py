"""Typed record tags (pgn_bam_records_tagged_device, pgn_fastq_records_tagged_device): the C ABI surface, the
refusals and their order, the rule's text, the host models and the Python wrappers, without a GPU.

The models are held to a parser written from SAMv1 section 4.2.4 (tests/_tag_cases.py) and, for FASTQ, to a split of
the header line: every tag of every case is read back and compared with what the case's columns say, independent of
the model.  The cases of the GPU tests are built here too, so the conditions their builders assert are checked on
the CPU.
"""
import ctypes as C
import gzip
import os
import re
import struct

import numpy as np
import pytest

import _tag_cases as K
from rawnanoporesignalcompression_amd import host
from rawnanoporesignalcompression_amd.host import TAG_DICT, TAG_F32, TAG_I32, TAG_STR, TAG_U32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAM_FN, FASTQ_FN = "pgn_bam_records_tagged_device", "pgn_fastq_records_tagged_device"


def _header(comments=False):
    src = open(os.path.join(ROOT, "include", "pgnano_hip.h")).read()
    return src if comments else re.sub(r"/\*.*?\*/", "", src, flags=re.S)


@pytest.fixture(scope="module")
def cases():
    return K.tag_cases()


# ---- surface -------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_bound():
    import rawnanoporesignalcompression_amd as pkg
    from rawnanoporesignalcompression_amd import _native, bam, demux, fastq, tags

    lib = _native.load()
    sigs = {s[0]: s for s in _native.SIGNATURES}
    old = {"pgn_bam_records_device": BAM_FN, "pgn_fastq_records_device": FASTQ_FN}
    for was, fn in old.items():
        assert re.search(r"\bint\s+" + fn + r"\s*\(", _header())
        assert hasattr(lib, fn)
        # every argument of the old call in the same order, with the tags behind the params
        assert sigs[fn][1] is C.c_int and sigs[fn][2][:2] == sigs[was][2][:2] and sigs[fn][2][3:] == sigs[was][2][2:]
        assert sigs[fn][2][2] is C.POINTER(_native.RecordTags)
    assert C.sizeof(_native.TagColumn) == 40 and C.sizeof(_native.RecordTags) == 8 + 16 * 40
    for name, value in (("PGN_TAG_U32", 0), ("PGN_TAG_I32", 1), ("PGN_TAG_F32", 2), ("PGN_TAG_DICT", 3), ("PGN_TAG_STR", 4),
                        ("PGN_REC_MAX_TAGS", 16), ("PGN_TAG_MAX_STRING", 255)):
        assert re.search(r"#define\s+" + name + r"\s+" + str(value) + r"u\b", _header()), name
        assert getattr(_native, name) == value
    for name in ("u32", "i32", "f32", "zdict", "zstr", "tag_bytes_signal", "bam_records_tagged_signal",
                 "fastq_records_tagged_signal", "bam_bound_tagged", "fastq_bound_tagged"):
        assert name in tags.__all__ and callable(getattr(tags, name))
        assert name not in pkg.__all__                      # the package's own surface stays as it is
    for name in ("tag_bytes_signal", "bam_records_tagged_signal", "fastq_records_tagged_signal", "bam_bound_tagged",
                 "fastq_bound_tagged"):
        assert getattr(tags, name) is getattr(host, name)
    assert "barcode_tag" in demux.__all__ and callable(demux.barcode_tag)
    assert "tags" not in pkg.__all__ and not hasattr(pkg.PGNanoCodec, "bam_records_tagged")
    assert callable(bam.bam_records) and callable(fastq.fastq_records)
    src = open(os.path.join(ROOT, "rawnanoporesignalcompression_amd", "csrc", "pgn_kernels.hip")).read()
    assert '#include "pgn_tags.h"' in src


# ---- refusals ------------------------------------------------------------------------------------------------
def _columns(*cols):
    """pgn_record_tags of ``(name, type, nstrings, d_values, d_str_off, d_strings, str_capacity)`` rows."""
    from rawnanoporesignalcompression_amd import _native

    t = _native.RecordTags(len(cols), 0)
    for k, (name, typ, nstrings, values, off, strings, cap) in enumerate(cols[:16]):
        c = t.col[k]
        c.name[:] = list(name.encode("latin-1"))
        c.type, c.nstrings, c.d_values, c.d_str_off, c.d_strings, c.str_capacity = typ, nstrings, values, off, strings, cap
    return t


P = 0x1000                                                   # a pointer no refusal looks behind


def _u32(name="ch"):
    return (name, TAG_U32, 0, P, None, None, 0)


def test_bam_call_refusals_and_their_order():
    from rawnanoporesignalcompression_amd import _native

    fn = getattr(_native.load(), BAM_FN)
    bad = _native.PGN_ERR_INVALID_ARG
    dummy = C.c_void_p(P)

    def call(ctx=dummy, flags=0, ntags=0, stride=5, tags=None, no_tags=False, nreads=3, ids=dummy, rb=dummy, st=dummy,
             seq=dummy, cap=100, rf=dummy, codes=dummy, fcap=10, out=dummy, bcap=100, off=dummy, rst=dummy, wr=dummy,
             params=True):
        prm = _native.BamParams(flags, ntags)
        prm.stride = stride
        cols = _columns(_u32()) if tags is None else tags
        return fn(ctx, C.byref(prm) if params else None, None if no_tags else C.byref(cols), nreads, ids, rb, st, None, seq,
                  None, cap, rf, codes, 0, fcap, out, bcap, off, rst, wr, None)

    # every refusal alone
    assert call(ctx=None) == bad and call(params=False) == bad and call(no_tags=True) == bad
    for flags in (8, 16, 1 << 31):
        assert call(flags=flags) == bad, flags
    assert call(ntags=1) == bad and call(ntags=8) == bad
    many = _columns(*[_u32()] * 16)
    many.ncols = 17
    assert call(tags=many) == bad
    for name in ("1a", "a_", "\x00\x00", "a ", "é0"):
        assert call(tags=_columns(_u32(name))) == bad, name
    for typ in (5, 6, 255):
        assert call(tags=_columns(("ch", typ, 0, P, P, P, 0))) == bad, typ
    for stride in (0, 128, 1 << 20):
        assert call(flags=_native.PGN_BAM_MOVES, stride=stride) == bad, stride
    assert call(nreads=1 << 32) == bad
    assert call(tags=_columns(("pi", TAG_STR, 0, None, P, P, 1 << 32))) == bad
    for typ in (TAG_U32, TAG_I32, TAG_F32, TAG_DICT):
        assert call(tags=_columns(("ch", typ, 0, None, None, None, 0))) == bad, typ
    assert call(tags=_columns(("pi", TAG_STR, 0, None, None, P, 4))) == bad
    assert call(tags=_columns(("BC", TAG_DICT, 2, P, None, P, 4))) == bad
    assert call(tags=_columns(("pi", TAG_STR, 0, None, P, None, 4))) == bad
    for kw in (dict(ids=None), dict(rb=None), dict(st=None), dict(rst=None), dict(flags=_native.PGN_BAM_MOVES, rf=None),
               dict(off=None), dict(wr=None), dict(seq=None), dict(flags=_native.PGN_BAM_MOVES, codes=None), dict(out=None)):
        assert call(**kw) == bad, kw
    # Every refusal gives the same code, so the order shows only in what an earlier one keeps the call from looking
    # at: with a NULL ctx nothing else, and behind unknown flag bits or ntags != 0 columns that hold anything.  An
    # F32 column is no fault here.
    assert call(ctx=None, flags=8, ntags=1, tags=many, nreads=1 << 32, ids=None) == bad
    assert call(tags=_columns(("qs", TAG_F32, 0, P, None, None, 0)), ids=None) == bad
    junk = _columns(("\xff\xff", 99, 0, None, None, None, 1 << 40))
    junk.ncols = 0xFFFFFFFF
    assert call(flags=8, tags=junk) == bad and call(ntags=1, tags=junk) == bad


def test_fastq_call_refusals_and_their_order():
    from rawnanoporesignalcompression_amd import _native

    fn = getattr(_native.load(), FASTQ_FN)
    bad = _native.PGN_ERR_INVALID_ARG
    dummy = C.c_void_p(P)

    def call(ctx=dummy, flags=0, ntags=0, tags=None, no_tags=False, nreads=3, ids=dummy, rb=dummy, st=dummy, seq=dummy,
             qual=dummy, cap=100, out=dummy, bcap=100, off=dummy, rst=dummy, params=True):
        prm = _native.FastqParams(flags, ntags)
        cols = _columns(_u32()) if tags is None else tags
        return fn(ctx, C.byref(prm) if params else None, None if no_tags else C.byref(cols), nreads, ids, rb, st, None, seq,
                  qual, cap, out, bcap, off, rst, None)

    assert call(ctx=None) == bad and call(params=False) == bad and call(no_tags=True) == bad
    for flags in (2, 4, 1 << 31):
        assert call(flags=flags) == bad, flags
    assert call(ntags=1) == bad
    many = _columns(*[_u32()] * 16)
    many.ncols = 17
    assert call(tags=many) == bad
    assert call(tags=_columns(_u32("9a"))) == bad and call(tags=_columns(("ch", 5, 0, P, P, P, 0))) == bad
    # a float column refuses the whole call, wherever it stands and whatever else is right
    assert call(tags=_columns(("qs", TAG_F32, 0, P, None, None, 0))) == bad
    assert call(tags=_columns(_u32(), ("ts", TAG_I32, 0, P, None, None, 0), ("qs", TAG_F32, 0, P, None, None, 0))) == bad
    assert call(nreads=1 << 32) == bad
    assert call(tags=_columns(("pi", TAG_STR, 0, None, P, P, 1 << 32))) == bad
    assert call(tags=_columns(("ts", TAG_I32, 0, None, None, None, 0))) == bad
    assert call(tags=_columns(("pi", TAG_STR, 0, None, None, P, 4))) == bad
    assert call(tags=_columns(("BC", TAG_DICT, 0, P, None, None, 4))) == bad          # str_capacity > 0, no d_strings
    for kw in (dict(ids=None), dict(rb=None), dict(st=None), dict(rst=None), dict(off=None), dict(seq=None), dict(qual=None),
               dict(out=None)):
        assert call(**kw) == bad, kw
    assert call(ctx=None, flags=2, ntags=1, tags=many, nreads=1 << 32, ids=None) == bad


def test_the_header_carries_the_rule():
    src = re.sub(r"\s*\n \*\s*", " ", _header(comments=True))
    for text in ("---- Typed record tags", "params->ntags must be 0", "in BAM mv:B:c stays last",
                 "BAM: name0 name1 'I' and the 4 bytes, 7 bytes.", "FASTQ: '\\t' name0 name1 ':' 'i' ':' dec(v)",
                 "with '-' in front of dec(|v|) for v < 0; -2^31 prints as -2147483648",
                 "exactly as stored, 7 bytes: a NaN's payload and -0 are not touched",
                 "a float's text has no rule here",
                 "idx >= nstrings: the column is absent for this read, 0 bytes in either format",
                 "nstrings == 0 leaves every read untagged", "Otherwise the span is [d_str_off[idx], d_str_off[idx + 1])",
                 "The span is [d_str_off[r], d_str_off[r + 1]).  The column is always present; an empty span writes an empty value.",
                 "A span [a, b) is valid iff a <= b <= str_capacity, b - a <= PGN_TAG_MAX_STRING = 255 and every byte "
                 "d_strings[a .. b) is in 0x20 .. 0x7E.",
                 "is not kept and gets PGN_ERR_INVALID_ARG, as a read whose frames leave the window does",
                 "No access leaves the buffers, whatever the offsets hold.",
                 "BAM: name0 name1 'Z' the bytes NUL, 4 + len bytes.", "':' 'Z' ':' the bytes, 6 + len bytes.",
                 "block_size of a kept read = 69 + (m + 1) / 2 + m + sum_k bytes_k(r) + (moves ? 9 + F : 0)",
                 "length of a kept read's FASTQ record = 42 + 2m + sum_k text_k(r)",
                 "bam_bound_tagged(nreads, nbases, columns, nframes)", "fastq_bound_tagged(nreads, nbases, columns)",
                 "With U32 columns only, every output (the bytes, rec_off, rec_status, d_written) is identical to the old call's",
                 "the scratch is 0 bytes per read and 8 bytes per 1,024 reads",
                 "in this order: a NULL ctx, params or tags; unknown flag bits; params->ntags != 0; ncols > PGN_REC_MAX_TAGS, "
                 "or a bad name or an unknown type among the first ncols; in FASTQ a PGN_TAG_F32 column; with PGN_BAM_MOVES a "
                 "stride outside 1..127; nreads >= 2^32; a str_capacity >= 2^32;",
                 "nreads == 0 writes rec_off[0] = 0 (and d_written = {0, 0} in BAM) only.",
                 "Not covered: other BAM types (A, c C s S, H, B arrays other than mv); 64-bit values; float text in FASTQ; "
                 "strings above 255 bytes; uniqueness of names; a float mean quality computed on the device; @RG header "
                 "lines, which stay the caller's header_text; SAM text.",
                 # the sections whose gap this closes keep their sentences
                 "a float qs:f: tag;", "signed or 64-bit tag values;", "qs:f and other non-uint32 tags;",
                 "Not covered: a BC:Z string tag (barcode goes into a uint32 tag column);"):
        assert text in src, text
    assert src.index("---- Adapters and barcodes") < src.index("---- Typed record tags")
    for path in ("README.md", "DESIGN.md", os.path.join("tools", "README.md")):
        text = re.sub(r"\s+", " ", open(os.path.join(ROOT, path)).read())
        assert "yped tags" in text and "tagged_records_timing" in text, path


# ---- the models against a parser -------------------------------------------------------------------------------
def test_every_bam_tag_reads_back(cases):
    for c in cases:
        for layout in [l for l in c.layouts if l != "fastq"]:
            data, stream, off, st, written = c.expected(layout)
            b = c.base
            assert off.dtype == np.uint64 and written.dtype == np.uint64 and len(off) == len(b.status) + 1
            if layout == "bgzf":
                assert (gzip.decompress(data) if data else b"") == stream, c.name
            recs = K.parse_records(stream)
            keeps = np.flatnonzero(K.kept(c, layout) & (st == 0))
            assert len(recs) == len(keeps), c.name
            assert set(c.bad) == set(np.flatnonzero((st == K.BAD) & (np.asarray(b.status) != K.BAD)).tolist()), c.name
            for rec, r in zip(recs, keeps):
                tags = rec["tags"]
                if b.codes is not None:
                    tag, typ, (sub, arr) = tags[-1]
                    F = int(b.read_frames[r + 1] - b.read_frames[r])
                    assert (tag, typ, sub) == ("mv", "B", "c") and len(arr) == 1 + F and arr[0] == b.stride, (c.name, r)
                    tags = tags[:-1]
                want = K.expected_tags(c, r, layout)
                got = [(t, y, v[1] if y == "f" else v) for t, y, v in tags]
                assert got == want, (c.name, layout, int(r))
                # the length rule
                m = int(b.read_bases[r + 1] - b.read_bases[r])
                size = 4 + 69 + (m + 1) // 2 + m + sum(7 if y in "Iif" else 4 + len(v) for _, y, v in want)
                size += 0 if b.codes is None else 9 + int(b.read_frames[r + 1] - b.read_frames[r])
                assert int(off[r + 1] - off[r]) == size, (c.name, int(r))


def test_every_fastq_tag_reads_back(cases):
    for c in cases:
        if "fastq" not in c.layouts:
            continue
        text, _, off, st, _ = c.expected("fastq")
        lines = text.split(b"\n")
        keeps = np.flatnonzero(K.kept(c, "fastq") & (st == 0))
        assert len(lines) == 4 * len(keeps) + 1 and lines[-1] == b"", c.name
        assert set(c.bad) == set(np.flatnonzero((st == K.BAD) & (np.asarray(c.base.status) != K.BAD)).tolist()), c.name
        for k, r in enumerate(keeps):
            uuid, tags = K.parse_fastq_header(lines[4 * k])
            assert len(uuid) == 36 and tags == K.expected_tags(c, r, "fastq"), (c.name, int(r))
            m = int(c.base.read_bases[r + 1] - c.base.read_bases[r])
            assert int(off[r + 1] - off[r]) == 42 + 2 * m + sum(6 + len(v) for _, _, v in tags), (c.name, int(r))


def test_identity_with_the_old_models(cases):
    """With U32 columns only the tagged models are the old ones, on the reads of every case."""
    for c in cases:
        b = c.base
        n = len(b.status)
        plain = [("qs", np.arange(n, dtype=np.uint32) * 1_000_003), ("ch", np.full(n, 0xFFFFFFFF, np.uint32))]
        typed = [(name, K.U(v)) for name, v in plain]
        for bgzf in (False, True):
            cap = 3000 if c.stream_capacity is not None else None
            old = host.bam_records_signal(b.ids, b.seq, b.qual, b.read_bases, b.status, plain, b.keep, b.reverse, b.moves,
                                          len(b.seq), cap, bgzf)
            new = host.bam_records_tagged_signal(b.ids, b.seq, b.qual, b.read_bases, b.status, typed, b.keep, b.reverse,
                                                 b.moves, len(b.seq), cap, bgzf)
            assert old[0] == new[0] and all(np.array_equal(x, y) for x, y in zip(old[1:], new[1:])), c.name
        if b.qual is not None:
            old = host.fastq_records_signal(b.ids, b.seq, b.qual, b.read_bases, b.status, plain, b.keep, b.reverse, len(b.seq))
            new = host.fastq_records_tagged_signal(b.ids, b.seq, b.qual, b.read_bases, b.status, typed, b.keep, b.reverse,
                                                   len(b.seq))
            assert old[0] == new[0] and all(np.array_equal(x, y) for x, y in zip(old[1:], new[1:])), c.name
        assert host.bam_bound_tagged(n, len(b.seq), typed, 7) == host.bam_bound(n, len(b.seq), 2, 7)
        assert host.fastq_bound_tagged(n, len(b.seq), typed) == host.fastq_bound(n, len(b.seq), 2)


def test_the_bounds_suffice(cases):
    for c in cases:
        if not c.monotonic:
            continue
        for layout in c.layouts:
            free = K.Case(c.name, c.base, c.cols, c.layouts, c.bad, None)
            _, _, off, st, _ = free.expected(layout)
            assert int(off[-1]) <= free.bound(layout), (c.name, layout)
            assert not ((st == K.SMALL) & (np.asarray(c.base.status) != K.SMALL)).any(), (c.name, layout)


# ---- mutants ---------------------------------------------------------------------------------------------------
MUTANTS = ("nul-omitted", "i-for-u32", "idx-nstrings-accepted", "0x7f-accepted", "cap-256", "columns-reordered",
           "minus-dropped", "absent-writes-name", "f32-normalised")


def _mutant_bytes(name, col, r, text, m):
    """tag_bytes_signal again, with the one thing changed that ``m`` names (None: nothing)."""
    name = name.encode()
    v, off, pool = col.host()
    t = col.type
    if t in (TAG_U32, TAG_I32, TAG_F32):
        bits = int(v[r])
        if not text:
            if t == TAG_F32 and m == "f32-normalised":
                bits = struct.unpack("<I", struct.pack("<f", struct.unpack("<f", struct.pack("<I", bits))[0] + 0.0))[0]
            code = b"i" if (t == TAG_U32 and m == "i-for-u32") else b"Iif"[t:t + 1]
            return name + code + struct.pack("<I", bits)
        val = bits - (1 << 32) if t == TAG_I32 and bits >> 31 else bits
        return b"\t" + name + b":i:" + str(abs(val) if m == "minus-dropped" else val).encode()
    absent = (b"\t" + name + b":Z:" if text else name + b"Z\0") if m == "absent-writes-name" else b""
    i = r
    if t == TAG_DICT:
        i = int(v[r])
        if i > col.nstrings if m == "idx-nstrings-accepted" else i >= col.nstrings:
            return absent
        if i == col.nstrings:
            a = b = int(off[i]) if off is not None else 0      # the entry behind the table: an empty one
        else:
            a, b = int(off[i]), int(off[i + 1])
    else:
        a, b = int(off[i]), int(off[i + 1])
    if not (a <= b <= col.str_capacity and b - a <= (256 if m == "cap-256" else 255)):
        return None
    s = pool[a:b].tobytes() if pool is not None else b""
    if any(ch < 0x20 or ch > (0x7F if m == "0x7f-accepted" else 0x7E) for ch in s):
        return None
    if text:
        return b"\t" + name + b":Z:" + s
    return name + b"Z" + s + (b"" if m == "nul-omitted" else b"\0")


def _mutant_run(c, layout, m):
    b = c.base
    cols = c.columns(layout)
    if m == "columns-reordered":
        cols = cols[::-1]

    def row(r):
        parts = [_mutant_bytes(name, col, r, layout == "fastq", m) for name, col in cols]
        return None if any(p is None for p in parts) else b"".join(parts)

    if layout == "fastq":
        return host._fastq_records(b.ids, b.seq, b.qual, b.read_bases, b.status, b.keep, b.reverse, len(b.seq),
                                   c.capacity(layout), row)
    return host._bam_records(b.ids, b.seq, b.qual, b.read_bases, b.status, b.keep, b.reverse, b.moves, len(b.seq),
                             c.capacity(layout), False, row)


def test_mutants_of_the_rule_fail_on_the_cases(cases):
    """Nine copies of the rule with one thing changed each: the unchanged copy writes the model's bytes on every
    case, and every mutant writes other bytes (or other offsets or statuses) on at least one."""
    small = [c for c in cases if not c.name.startswith("tag-seams") and not c.name.startswith("tag-align+")]
    seen = {m: [] for m in MUTANTS}
    for c in small:
        for layout in [l for l in c.layouts if l != "bgzf"]:
            want = c.expected(layout)
            same = _mutant_run(c, layout, None)
            assert same[0] == want[1] and np.array_equal(same[1], want[2]) and np.array_equal(same[2], want[3]), (c.name, layout)
            for m in MUTANTS:
                got = _mutant_run(c, layout, m)
                if got[0] != same[0] or not np.array_equal(got[1], same[1]) or not np.array_equal(got[2], same[2]):
                    seen[m].append(f"{c.name}/{layout}")
    for m in MUTANTS:
        print(f"  {m:24s} differs on {len(seen[m]):2d}: {' '.join(seen[m][:6])}")
        assert seen[m], f"no case tells the mutant {m} from the rule"
    # each of these has a case built for it
    assert any(s.startswith("tag-dictionary/") for s in seen["idx-nstrings-accepted"])
    assert any(s.startswith("tag-strings/") for s in seen["0x7f-accepted"]) and any(s.startswith("tag-strings/") for s in seen["cap-256"])
    assert any(s == "tag-values/fastq" for s in seen["minus-dropped"]) and any(s == "tag-values/raw" for s in seen["f32-normalised"])


def test_the_case_list_covers_the_issue(cases):
    by = {c.name: c for c in cases}
    for name in ("tag-seams", "tag-seams-fastq", "tag-strings", "tag-empty-pools", "tag-dictionary", "tag-values", "tag-cols0",
                 "tag-cols16", "tag-gaps", "tag-reverse", "tag-reverse-nomoves", "tag-noqual", "tag-capacity-raw",
                 "tag-capacity-fastq", "tag-empty"):
        assert name in by, name
    assert {c.base.out_offset for c in cases if c.name.startswith("tag-align+")} == set(range(16))
    assert by["tag-seams"].layouts == ("raw", "bgzf") and by["tag-seams-fastq"].layouts == ("fastq",)
    assert len(by["tag-cols16"].cols) == 16 and by["tag-cols0"].cols == []
    assert by["tag-reverse"].base.reverse and by["tag-reverse"].base.codes is not None
    assert by["tag-reverse-nomoves"].base.reverse and by["tag-reverse-nomoves"].base.codes is None
    assert by["tag-noqual"].base.qual is None and len(by["tag-empty"].base.status) == 0
    lens = {int(b) - int(a) for _, col in by["tag-strings"].cols if col.type == TAG_STR
            for a, b in zip(col.host()[1][:4], col.host()[1][1:5])}
    assert lens == {0, 1, 255, 256}
    assert len(K.runs()) == sum(len(c.layouts) for c in cases)


# ---- the Python surface ------------------------------------------------------------------------------------------
def test_wrappers_and_their_refusals():
    import torch

    from rawnanoporesignalcompression_amd import tags

    n = 4
    ints, floats = torch.arange(n, dtype=torch.int32), torch.arange(n, dtype=torch.float32)
    assert tags.u32(ints).type == TAG_U32 and tags.i32(ints).type == TAG_I32 and tags.f32(floats).type == TAG_F32
    for make, t in ((tags.u32, floats), (tags.i32, floats), (tags.f32, ints), (tags.u32, ints.long()), (tags.f32, floats.double()),
                    (tags.i32, ints.short())):
        with pytest.raises(ValueError):
            make(t)
    with pytest.raises(ValueError):
        tags.zdict(floats, ["a"])
    for bad in (["x" * 256], [b"a\x7f"], [b"\x1fa"], [b"a\0b"]):
        with pytest.raises(ValueError):
            tags.zdict(ints, bad)
        with pytest.raises(ValueError):
            tags.zstr(bad)
    with pytest.raises(ValueError):
        tags.StringTable.from_arrays(torch.zeros(3, dtype=torch.int32), np.zeros(3, np.uint8))   # one of each
    with pytest.raises(ValueError):
        tags.StringTable.from_arrays(torch.zeros(3, dtype=torch.int64), torch.zeros(3, dtype=torch.uint8))
    z = tags.zdict(ints, ["bc01", "bc02", ""])
    assert z.type == TAG_DICT and len(z.table) == 3 and z.table.nbytes == 8 and z.column.nstrings == 3
    s = tags.zstr([b"a", b"", b"ccc", b"dd"])
    assert s.type == TAG_STR and s.values is None and s.table.off.tolist() == [0, 1, 1, 4, 6]
    s2 = tags.zstr(np.array([0, 1, 1, 4, 6]), np.frombuffer(b"acccdd", np.uint8))
    assert s2.table.data.tobytes() == b"acccdd" and s2.column.str_capacity == 6
    # which call a dict goes to: plain integer tensors alone stay with the old one
    assert not tags.has_typed(None) and not tags.has_typed({}) and not tags.has_typed({"qs": ints, "ch": ints})
    assert tags.has_typed({"qs": ints, "ts": tags.i32(ints)}) and tags.has_typed({"BC": z})
    # the wrappers are what the host models take
    ids = np.arange(16 * n, dtype=np.uint8).reshape(n, 16)
    seq, rb = np.frombuffer(b"ACGTACGTAC", np.uint8), np.array([0, 3, 5, 6, 10])
    out = host.fastq_records_tagged_signal(ids, seq, seq, rb, np.zeros(n, np.int32), {"ts": tags.i32(-ints), "BC": z, "pi": s})
    assert out[0].split(b"\n")[4].endswith(b"\tts:i:-1\tBC:Z:bc02\tpi:Z:")
    with pytest.raises(ValueError):
        host.fastq_records_tagged_signal(ids, seq, seq, rb, np.zeros(n, np.int32), {"qs": tags.f32(floats)})
    with pytest.raises(ValueError):
        host.bam_records_tagged_signal(ids, seq, seq, rb, np.zeros(n, np.int32), {f"t{chr(97 + k)}": ints.numpy() for k in range(17)})
    with pytest.raises(ValueError):
        host.tag_bytes_signal("qs", tags.f32(floats).column, 0, text=True)


def test_record_calls_check_typed_columns_before_any_launch():
    """native_columns, what bam_records and fastq_records build the C struct with: its refusals need no device."""
    import torch

    from rawnanoporesignalcompression_amd import tags

    class Codec:
        device = 0

    n = 3
    ints = torch.arange(n, dtype=torch.int32)
    with pytest.raises(ValueError, match="no f32 column"):
        tags.native_columns(Codec, {"qs": tags.f32(ints.float())}, n, text=True)
    with pytest.raises(ValueError, match="at most 16"):
        tags.native_columns(Codec, {f"t{k:x}": tags.u32(ints) for k in range(17)}, n, text=False)
    with pytest.raises(ValueError, match="float column is tags.f32"):
        tags.native_columns(Codec, {"qs": ints.float(), "ts": tags.i32(ints)}, n, text=False)
    with pytest.raises(ValueError, match="name"):
        tags.native_columns(Codec, {"1s": tags.i32(ints)}, n, text=False)
    with pytest.raises(ValueError, match="cuda:0"):
        tags.native_columns(Codec, {"ts": tags.i32(ints)}, n, text=False)             # a host tensor
    with pytest.raises(ValueError, match="on the device"):
        tags.native_columns(Codec, {"pi": tags.zstr([b"a", b"b", b"c"])}, n, text=False)


def test_barcode_tag_refuses_a_table_with_unclassified():
    import torch

    from rawnanoporesignalcompression_amd import demux, tags

    with pytest.raises(ValueError):
        demux.barcode_tag(torch.zeros(3, dtype=torch.int32), tags.StringTable(["a"]), unclassified="none")
    with pytest.raises(ValueError):
        demux.barcode_tag(torch.zeros(3, dtype=torch.int32), ["bad\x7fname"])
