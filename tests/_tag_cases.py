"""Cases for the typed record tags (include/pgnano_hip.h "Typed record tags"), built once for the CPU tests
(tests/test_tagged_records_api.py) and the GPU tests (tests/test_gpu_tagged_records.py), and the parser both hold the
BAM bytes to: written here from SAMv1 section 4.2.4 with ``struct``, independent of the host model.

The list is built for where the kernels can go wrong, not for the workload: a tile seam on every byte of a tag area
in turn (BAM raw, BAM in BGZF blocks, FASTQ), every way a string span can be invalid, the dictionary's edges, the
values whose bytes or text are easy to get wrong, 0 and 16 columns, and the layouts of the old calls' cases with typed
columns in them.  Every builder asserts here, on the CPU, the condition its case exists for, and states by hand which
reads a column refuses (``bad``), so a case list that drifts fails without a GPU.
"""
import functools
import struct
from dataclasses import dataclass

import numpy as np

import _bam_cases as B
from rawnanoporesignalcompression_amd import _native
from rawnanoporesignalcompression_amd.host import (TAG_DICT, TAG_F32, TAG_I32, TAG_STR, TAG_U32, TagColumn,
                                                   bam_bound_tagged, bam_records_tagged_signal, bgzf_blocks_signal,
                                                   bgzf_bound, fastq_bound_tagged, fastq_records_tagged_signal)

BLOCK = _native.PGN_BGZF_BLOCK_BYTES
TILE = _native.PGN_FASTQ_TILE_BYTES
BAD = _native.PGN_ERR_INVALID_ARG
SMALL = _native.PGN_ERR_DST_TOO_SMALL
NONE = 0xFFFFFFFF
LAYOUTS = ("raw", "bgzf", "fastq")


# ---- the parser ----------------------------------------------------------------------------------------------------
_FIXED = {"A": "<c", "c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I", "f": "<f"}


def parse_tags(rec, p):
    """The optional fields of a BAM record from byte ``p`` to its end, by SAMv1 section 4.2.4: ``[(tag, type,
    value)]``; a float comes with its four bytes, ``(value, bytes)``; a ``B`` array as ``(subtype, numpy array)``."""
    out = []
    while p < len(rec):
        assert p + 3 <= len(rec), "a tag and its type"
        tag, typ = rec[p:p + 2].decode("ascii"), chr(rec[p + 2])
        assert tag[0].isalpha() and tag[1].isalnum(), tag
        p += 3
        if typ in _FIXED:
            size = struct.calcsize(_FIXED[typ])
            assert p + size <= len(rec)
            v = struct.unpack_from(_FIXED[typ], rec, p)[0]
            out.append((tag, typ, (v, bytes(rec[p:p + 4])) if typ == "f" else v))
            p += size
        elif typ in "ZH":
            end = rec.index(b"\0", p)                       # a ValueError where the NUL is missing
            out.append((tag, typ, bytes(rec[p:end])))
            p = end + 1
        elif typ == "B":
            sub, count = chr(rec[p]), struct.unpack_from("<I", rec, p + 1)[0]
            dt = np.dtype({"c": "i1", "C": "u1", "s": "<i2", "S": "<u2", "i": "<i4", "I": "<u4", "f": "<f4"}[sub])
            assert p + 5 + count * dt.itemsize <= len(rec)
            out.append((tag, typ, (sub, np.frombuffer(rec, dt, count, p + 5))))
            p += 5 + count * dt.itemsize
        else:
            raise AssertionError(f"unknown tag type {typ!r}")
    assert p == len(rec)
    return out


def parse_records(stream):
    """The records of a stream of BAM records (SAMv1 section 4.2): ``[dict(name, l_seq, qual, tags)]``."""
    out, at = [], 0
    while at < len(stream):
        (block_size,) = struct.unpack_from("<I", stream, at)
        rec = stream[at + 4:at + 4 + block_size]
        assert len(rec) == block_size, "a whole record"
        _, _, l_name, _, _, n_cigar, flag, l_seq, _, _, _ = struct.unpack_from("<iiBBHHHIiii", rec, 0)
        assert flag == 4 and n_cigar == 0
        p = 32 + l_name + (l_seq + 1) // 2 + l_seq
        out.append(dict(name=bytes(rec[32:32 + l_name]), l_seq=l_seq, tags=parse_tags(rec, p)))
        at += 4 + block_size
    assert at == len(stream)
    return out


def parse_fastq_header(line):
    """``(uuid, [(tag, type, value text)])`` of a FASTQ header line: a split by tabs, then by the first two colons."""
    parts = line.split(b"\t")
    assert parts[0][:1] == b"@"
    return parts[0][1:], [tuple(p.split(b":", 2)) for p in parts[1:]]


# ---- columns -------------------------------------------------------------------------------------------------------
def U(v):
    return TagColumn(TAG_U32, np.asarray(v, np.uint64).astype(np.uint32))


def I(v):
    return TagColumn(TAG_I32, (np.asarray(v, np.int64) & 0xFFFFFFFF).astype(np.uint32))


def F(bits):
    return TagColumn(TAG_F32, np.asarray(bits, np.uint64).astype(np.uint32))


def pool_of(strings):
    off = np.zeros(len(strings) + 1, np.uint32)
    off[1:] = np.cumsum([len(s) for s in strings])
    return off, np.frombuffer(b"".join(strings), np.uint8).copy()


def D(index, strings, nstrings=None):
    """A dictionary column of the strings as they are (nothing is checked: the rule decides per read)."""
    off, pool = pool_of(strings)
    return TagColumn(TAG_DICT, (np.asarray(index, np.int64) & 0xFFFFFFFF).astype(np.uint32), off, pool,
                     len(strings) if nstrings is None else nstrings)


def S(strings):
    off, pool = pool_of(strings)
    return TagColumn(TAG_STR, None, off, pool)


@dataclass
class Case:
    name: str
    base: B.Case                                   # the reads: ids, seq, qual, offsets, statuses, keep, moves
    cols: list                                     # [(name, TagColumn)]
    layouts: tuple = LAYOUTS
    bad: tuple = ()                                # reads that a column refuses (status 10), stated by hand
    stream_capacity: int = None                    # BAM stream bytes / FASTQ bytes; None: the tagged bound
    monotonic: bool = True                         # every STR column's offsets are non-decreasing (the bound holds)

    def columns(self, layout):
        """A FASTQ call takes no float column: the case's columns without them."""
        return [(n, c) for n, c in self.cols if not (layout == "fastq" and c.type == TAG_F32)]

    def bound(self, layout):
        b, cols = self.base, [c for _, c in self.columns(layout)]
        if layout == "fastq":
            return fastq_bound_tagged(len(b.status), len(b.seq), cols)
        return bam_bound_tagged(len(b.status), len(b.seq), cols, None if b.codes is None else len(b.codes))

    def capacity(self, layout):
        """Bytes of ``out``."""
        s = self.bound(layout) if self.stream_capacity is None else self.stream_capacity
        return bgzf_bound(s) if layout == "bgzf" else s

    def expected(self, layout):
        """BAM: ``(file bytes, stream, rec_off, status, written)``; FASTQ: ``(text, text, rec_off, status, None)``."""
        return _expected(self, layout)


@functools.lru_cache(maxsize=None)
def _expected(c, layout):
    b = c.base
    if layout == "fastq":
        text, off, st = fastq_records_tagged_signal(b.ids, b.seq, b.qual, b.read_bases, b.status, c.columns(layout), b.keep,
                                                    b.reverse, len(b.seq), c.capacity(layout))
        return text, text, off, st, None
    bgzf = layout == "bgzf"
    stream, off, st, written = bam_records_tagged_signal(b.ids, b.seq, b.qual, b.read_bases, b.status, c.columns(layout),
                                                         b.keep, b.reverse, b.moves, len(b.seq), c.capacity(layout), bgzf)
    data = bgzf_blocks_signal(stream) if bgzf else stream
    assert len(stream) == int(written[0]) and len(data) == int(written[1]) <= c.capacity(layout)
    return data, stream, off, st, written


Case.__hash__ = lambda self: id(self)              # cases are built once and never change
Case.__eq__ = lambda self, other: self is other


def expected_tags(c, r, layout):
    """Read ``r``'s tags as the parser must find them, from the columns themselves and not from the model:
    ``[(tag, type, value)]`` in BAM, ``[(tag, type, text)]`` in FASTQ, without ``mv``."""
    out = []
    for name, col in c.columns(layout):
        v, off, pool = col.host()
        if col.type in (TAG_U32, TAG_I32):
            bits = int(v[r])
            val = bits - (1 << 32) if col.type == TAG_I32 and bits >> 31 else bits
            out.append((name, "i", str(val).encode()) if layout == "fastq" else (name, "Ii"[col.type], val))
        elif col.type == TAG_F32:
            raw = struct.pack("<I", int(v[r]))
            out.append((name, "f", raw))
        else:
            i = r if col.type == TAG_STR else int(v[r])
            if col.type == TAG_DICT and i >= col.nstrings:
                continue
            s = pool[int(off[i]):int(off[i + 1])].tobytes()
            out.append((name, "Z", s))
    if layout == "fastq":
        return [(n.encode(), t.encode(), s) for n, t, s in out]
    return out


def kept(c, layout):
    """The reads with a record (whatever the capacity)."""
    _, _, off, _, _ = c.expected(layout)
    return np.diff(off.astype(np.int64)) > 0


# ---- a seam on every byte of a tag area -------------------------------------------------------------------------------
SEAM_Z = b"bc005"
SEAM_AREA = 7 + 7 + (4 + len(SEAM_Z)) + 9          # ts:i, qs:f, BC:Z with its NUL, the mv header


def bam_seams():
    """A read longer than a tile, then pairs of a filler read and a short read: pair k's filler has the frames that
    put byte k of the short read's tag area (an I32, an F32, a Z of 5 bytes with its NUL, the mv header) directly
    behind tile seam k + 2."""
    tagb = 7 + 7 + 4 + len(SEAM_Z)
    lengths, frames, at = [50], [100_000], B.record_length(50, 0, 100_000) + tagb
    assert BLOCK < at < 2 * BLOCK
    want = []
    for k in range(SEAM_AREA):
        ms = 20 + (k & 1)
        rel = B.FRONT + (ms + 1) // 2 + ms                  # the short record's tag area
        filler = B.record_length(30, 0, 0) + tagb
        nf = (k + 2) * BLOCK - at - filler - rel - k
        assert nf > 20_000
        lengths += [30, ms]
        frames += [nf, 10]
        want.append((len(lengths) - 1, rel + k, (k + 2) * BLOCK))
        at += filler + nf + rel + tagb + 9 + 10
    n = len(lengths)
    base = B.make("tag-seams", lengths, 71, frames=frames)
    rng = np.random.default_rng(72)
    cols = [("ts", I(rng.integers(-2**31, 2**31, n))), ("qs", F(rng.integers(0, 2**32, n))), ("BC", D([0] * n, [SEAM_Z]))]
    c = Case("tag-seams", base, cols, layouts=("raw", "bgzf"))
    _, stream, off, st, _ = c.expected("raw")
    assert not st.any() and int(off[1]) > BLOCK, "the first read passes a whole tile"
    for r, byte, seam in want:
        assert int(off[r]) + byte == seam, (r, byte)
    k = want[23][0]                                         # the seam lies on the mv header's first byte here
    rec = stream[int(off[k]):int(off[k + 1])]
    assert rec[want[23][1]:want[23][1] + 4] == b"mvBc"
    assert stream[want[22][2] - 5:want[22][2] + 1] == SEAM_Z + b"\0", "... and one pair earlier on the string's NUL"
    return c


def fastq_seams():
    """The same at the FASTQ writer's seams (every PGN_FASTQ_TILE_BYTES, ``out`` a multiple of 16): byte k of the
    short read's tag text behind seam k + 2.  A filler's bases move the text by two bytes, its ``pi`` string by one."""
    text = len(b"\tts:i:-12\tch:i:7\tBC:Z:bc005")
    area = text + len(b"\tpi:Z:xyz")
    lengths, pi, at = [10_000], [b"first"], 42 + 20_000 + text + 6 + 5
    assert TILE < at < 2 * TILE
    want = []
    for k in range(area):
        ms = 10
        gap = (k + 2) * TILE - at - (42 + text + 6) - 37 - k     # the filler's 2 m + len(pi)
        assert gap > 12_000
        lengths += [gap // 2, ms]
        pi += [b"p" * (gap & 1), b"xyz"]
        want.append((len(lengths) - 1, 37 + k, (k + 2) * TILE))
        at += (42 + text + 6) + gap + (42 + 2 * ms + area)
    n = len(lengths)
    base = B.make("tag-seams-fastq", lengths, 73, frames=None)
    cols = [("ts", I([-12] * n)), ("ch", U([7] * n)), ("BC", D([0] * n, [SEAM_Z])), ("pi", S(pi))]
    c = Case("tag-seams-fastq", base, cols, layouts=("fastq",))
    _, data, off, st, _ = c.expected("fastq")
    assert not st.any() and int(off[1]) > TILE
    for r, byte, seam in want:
        assert int(off[r]) + byte == seam, (r, byte)
    assert data[want[0][2]:want[0][2] + 9] == b"\tts:i:-12" and data[want[-1][2]:want[-1][2] + 2] == b"z\n"
    return c


# ---- strings ----------------------------------------------------------------------------------------------------------
def strings():
    """A pool string per read: lengths 0, 1, 255 and 256; the bytes 0x1F, 0x7F and 0x00 first, last and inside; a
    decreasing offset; a span that ends one past the pool.  Only the reads named in ``bad`` lose their record."""
    good = bytes(range(0x20, 0x7F))
    items = [b"", b"~", (good * 3)[:255], (good * 3)[:256]]
    for ch in (0x1F, 0x7F, 0x00):
        items += [bytes([ch]) + b"abcd", b"abcd" + bytes([ch]), b"ab" + bytes([ch]) + b"cd"]
    items += [b" spaces and ~ are fine ", b"before-the-step-back", b"behind", b"the-last-one"]
    off, pool = pool_of(items)
    n = len(items)
    back = items.index(b"before-the-step-back")
    off[back + 1] -= 30                                     # read `back` runs backwards; the next one is longer by as much
    off[n] = len(pool) + 1                                  # the last read ends one past str_capacity
    col = TagColumn(TAG_STR, None, off, pool)
    base = B.make("tag-strings", [7 + r for r in range(n)], 74)
    c = Case("tag-strings", base, [("rn", U(np.arange(n))), ("pi", col), ("ts", I(-np.arange(n)))],
             bad=(3,) + tuple(range(4, 13)) + (back, n - 1), stream_capacity=2 * sum(len(s) for s in items) + 400 * n,
             monotonic=False)
    assert int(off[back + 1]) < int(off[back]) and int(off[back + 2]) - int(off[back + 1]) == 30 + len(b"behind")
    for layout in LAYOUTS:
        _, _, _, st, _ = c.expected(layout)
        assert np.flatnonzero(st).tolist() == sorted(c.bad) and set(st[list(c.bad)]) == {BAD}, layout
    return c


def empty_pools():
    """``str_capacity == 0``: every span is empty, a STR column writes empty values and a dictionary of empty
    entries too."""
    n = 5
    base = B.make("tag-empty-pools", [3, 9, 1, 30, 2], 75)
    c = Case("tag-empty-pools", base, [("pi", S([b""] * n)), ("BC", D([0, 1, 2, NONE, 0], [b"", b""])), ("ch", U(range(n)))])
    assert all(col.str_capacity == 0 for _, col in c.cols[:2])
    recs = parse_records(c.expected("raw")[1])
    assert [t[:3] for t in recs[0]["tags"][:2]] == [("pi", "Z", b""), ("BC", "Z", b"")] and recs[2]["tags"][1][0] == "ch"
    return c


# ---- the dictionary -----------------------------------------------------------------------------------------------------
def dictionary():
    """Indices nstrings - 1, nstrings and 0xFFFFFFFF; a column with no strings at all; a bad entry that only a read
    without a record references, and one (too long, and one with a 0x7F) that kept reads reference: only they fail.
    Columns behind an absent one move up."""
    names = [b"barcode01", b"bad\x7fentry", b"barcode03", b"x" * 256, b"unreferenced\x01", b"last"]
    idx = [0, 5, 6, NONE, 1, 2, 3, 4, 5, 0x80000000]
    n = len(idx)
    keep = np.ones(n, np.uint8)
    keep[7] = 0                                             # the read that references entry 4
    base = B.make("tag-dictionary", [11, 4, 8, 15, 16, 17, 2, 9, 33, 5], 76, keep=keep)
    cols = [("BC", D(idx, names)), ("RG", TagColumn(TAG_DICT, np.zeros(n, np.uint32), None, None, 0)),
            ("ch", U(np.arange(n) + 100)), ("b2", D([NONE, 0] * (n // 2), [b"second"]))]
    c = Case("tag-dictionary", base, cols, bad=(4, 6))
    for layout in LAYOUTS:
        _, _, _, st, _ = c.expected(layout)
        assert np.flatnonzero(st).tolist() == [4, 6] and not kept(c, layout)[7]
    recs = parse_records(c.expected("raw")[1])
    assert [t[0] for t in recs[0]["tags"]] == ["BC", "ch", "mv"] and [t[0] for t in recs[1]["tags"]] == ["BC", "ch", "b2", "mv"]
    assert [t[0] for t in recs[2]["tags"]] == ["ch", "mv"] and recs[1]["tags"][0][2] == b"last"
    return c


# ---- values ---------------------------------------------------------------------------------------------------------------
FLOAT_BITS = [0x7FC12345, 0xFFC00001, 0x80000000, 0x00000000, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF, 0x3FC00000]
INT_VALUES = [0, -1, -2**31, 2**31 - 1, 9, -10, 1_000_000_000, -999_999_999, 10]
UINT_VALUES = [2**32 - 1, 0, 2**31, 2**31 - 1, 9, 10, 99, 100, 4_000_000_000]


def values():
    """Floats whose bytes must pass untouched (NaNs with payloads, -0, infinities, denormals), the signed values
    whose text has a sign or the most digits, and the largest unsigned value."""
    n = len(FLOAT_BITS)
    base = B.make("tag-values", [5 + 3 * r for r in range(n)], 77)
    c = Case("tag-values", base, [("qs", F(FLOAT_BITS)), ("ts", I(INT_VALUES)), ("ch", U(UINT_VALUES)), ("sm", F(FLOAT_BITS[::-1]))])
    text = c.expected("fastq")[0].split(b"\n")
    assert text[8].endswith(b"\tts:i:-2147483648\tch:i:2147483648") and text[0].endswith(b"\tts:i:0\tch:i:4294967295")
    tags = parse_records(c.expected("raw")[1])[0]["tags"]
    assert tags[0][2][1] == bytes.fromhex("4523c17f") and np.isnan(tags[0][2][0])
    return c


# ---- column counts ------------------------------------------------------------------------------------------------------
def column_counts():
    n = 7
    lengths = [1, 2, 40, 3, 17, 64, 9]
    rng = np.random.default_rng(78)
    zero = Case("tag-cols0", B.make("tag-cols0", lengths, 79), [])
    names = ["qs", "ch", "rn", "ts", "ns", "sm", "sd", "du", "BC", "pi", "Z9", "a0", "mx", "RG", "st", "f5"]
    kinds = "fuuiifffdsuidsfu"
    cols = []
    for name, kind in zip(names, kinds):
        if kind == "f":
            cols.append((name, F(rng.integers(0, 2**32, n))))
        elif kind == "u":
            cols.append((name, U(rng.integers(0, 2**32, n))))
        elif kind == "i":
            cols.append((name, I(rng.integers(-2**31, 2**31, n))))
        elif kind == "d":
            cols.append((name, D(rng.integers(0, 4, n), [b"one", b"", b"three of them"])))   # index 3: absent
        else:
            cols.append((name, S([bytes(rng.integers(0x20, 0x7F, int(k)).astype(np.uint8)) for k in rng.integers(0, 40, n)])))
    full = Case("tag-cols16", B.make("tag-cols16", lengths, 80), cols)
    nomoves = Case("tag-cols16-nomoves", B.make("tag-cols16-nomoves", lengths, 81, frames=None, reverse=True), cols)
    assert len(cols) == _native.PGN_REC_MAX_TAGS and {c.type for _, c in cols} == {0, 1, 2, 3, 4}
    return [zero, full, nomoves]


# ---- layouts ------------------------------------------------------------------------------------------------------------
def _mixed(n, seed):
    rng = np.random.default_rng(seed)
    return [("qs", F(rng.integers(0, 2**32, n))), ("BC", D(rng.integers(0, 3, n), [b"bc01", b"barcode-two"])),
            ("ts", I(rng.integers(-5000, 5000, n))), ("pi", S([b"parent-%d" % r * (r % 3) for r in range(n)])),
            ("ch", U(rng.integers(0, 3000, n)))]


def layouts():
    """The old calls' layouts with typed columns in them: reads without a record between kept ones, ``reverse`` with
    and without moves, no qualities, all 16 alignments of ``out``, a capacity that cuts inside a tag area, no reads."""
    out = []
    lengths = [4, 0, 6, 9, 1, 1, 200, 2, 3, 0, 8, 5, 7, 0, 0, 30, 12]
    n = len(lengths)
    status, keep = np.zeros(n, np.int32), np.ones(n, np.uint8)
    status[0], keep[2], status[7], keep[8], status[10], keep[12] = 6, 0, BAD, 0, 1, 0
    gaps = Case("tag-gaps", B.make("tag-gaps", lengths, 82, status=status, keep=keep, cut=5), _mixed(n, 83))
    k = kept(gaps, "raw")
    assert not k[:3].any() and k[3] and not k[7:10].any() and not k[12:15].any() and not k[16] and k[15]
    out.append(gaps)
    small = [1, 2, 3, 15, 16, 17, 31, 32, 33, 64, 65, 5, 8]
    n = len(small)
    out.append(Case("tag-reverse", B.make("tag-reverse", small, 84, reverse=True), _mixed(n, 85)))
    out.append(Case("tag-reverse-nomoves", B.make("tag-reverse-nomoves", small, 86, reverse=True, frames=None), _mixed(n, 87)))
    out.append(Case("tag-noqual", B.make("tag-noqual", small, 88, qual=False), _mixed(n, 89), layouts=("raw", "bgzf")))
    for o in range(16):
        out.append(Case(f"tag-align+{o}", B.make(f"tag-align+{o}", small, 90, out_offset=o), _mixed(n, 91),
                        layouts=("raw", "fastq") if o % 5 else LAYOUTS))
    # a capacity that ends inside record 6's tag area, in either format
    full = Case("tag-full", B.make("tag-full", small, 92), _mixed(n, 93))
    for layout in ("raw", "fastq"):
        _, _, off, _, _ = full.expected(layout)
        m = small[6]
        area = int(off[6]) + (B.FRONT + (m + 1) // 2 + m + 9 if layout == "raw" else 37 + 12)
        c = Case(f"tag-capacity-{layout}", B.make(f"tag-capacity-{layout}", small, 92), _mixed(n, 93),
                 layouts=("raw", "bgzf") if layout == "raw" else ("fastq",), stream_capacity=area)
        for lay in c.layouts:
            data, _, off2, st, wr = c.expected(lay)
            assert np.array_equal(off2, off) and (st[:6] == 0).all() and (st[6:] == SMALL).all(), lay
            assert int(off[6]) < area < int(off[7]) and (wr is None or int(wr[0]) == int(off[6]))
        out.append(c)
    out.append(Case("tag-empty", B.make("tag-empty", [], 94), _mixed(0, 95)))
    return out


@functools.lru_cache(maxsize=None)
def tag_cases():
    """Every case of the tagged record calls, built once a process; nothing changes a case."""
    cases = [bam_seams(), fastq_seams(), strings(), empty_pools(), dictionary(), values()] + column_counts() + layouts()
    names = [c.name for c in cases]
    assert len(set(names)) == len(names), names
    return cases


def runs():
    """``(case name, layout)`` of every run."""
    return [(c.name, layout) for c in tag_cases() for layout in c.layouts]
