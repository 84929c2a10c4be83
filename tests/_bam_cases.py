"""Cases for the BAM record call (include/pgnano_hip.h "BAM records"), built once for the CPU tests
(tests/test_bam_api.py) and the GPU tests (tests/test_gpu_bam.py), and the parser both hold the bytes to: written
here from the SAM specification with ``struct``, independent of the host model.

Every builder asserts here, on the CPU, the condition its case exists for (a BGZF seam inside a given field, a
stream of exactly a block's length, a capacity one byte short of a record's end), from the host model's own
outputs: a case list that drifts fails without a GPU.
"""
import functools
import struct
from dataclasses import dataclass, field

import numpy as np

from rawnanoporesignalcompression_amd import _native
from rawnanoporesignalcompression_amd.host import (bam_bound, bam_records_signal, bgzf_blocks_signal, bgzf_bound,
                                                   bgzf_stream_capacity)

B = _native.PGN_BGZF_BLOCK_BYTES
FILE = B + 31
BAD = _native.PGN_ERR_INVALID_ARG
SMALL = _native.PGN_ERR_DST_TOO_SMALL
FRONT = 73                               # block_size, the fixed fields and the name
W_CASES = (0, 1, B - 1, B, B + 1, 2 * B)
LAYOUTS = ("raw", "bgzf")


# ---- the parser ----------------------------------------------------------------------------------------------------
def parse_records(stream):
    """The records of a stream of BAM records as dicts, by the SAM specification (SAMv1 section 4.2)."""
    out, at = [], 0
    while at < len(stream):
        (block_size,) = struct.unpack_from("<I", stream, at)
        rec = stream[at + 4:at + 4 + block_size]
        assert len(rec) == block_size, "a whole record"
        ref, pos, l_name, mapq, bin_, n_cigar, flag, l_seq, nref, npos, tlen = struct.unpack_from("<iiBBHHHIiii", rec, 0)
        p = 32
        name = rec[p:p + l_name]
        p += l_name + 4 * n_cigar
        packed = rec[p:p + (l_seq + 1) // 2]
        p += (l_seq + 1) // 2
        seq = "".join("=ACMGRSVTWYHKDBN"[b >> 4] + "=ACMGRSVTWYHKDBN"[b & 15] for b in packed)
        pad = seq[l_seq:]
        qual = rec[p:p + l_seq]
        p += l_seq
        tags, moves, stride = [], None, None
        while p < len(rec):
            tag, typ = rec[p:p + 2].decode(), chr(rec[p + 2])
            p += 3
            if typ == "I":
                tags.append((tag, struct.unpack_from("<I", rec, p)[0]))
                p += 4
            elif typ == "B":
                sub, count = chr(rec[p]), struct.unpack_from("<I", rec, p + 1)[0]
                assert tag == "mv" and sub == "c" and count >= 1
                arr = np.frombuffer(rec, np.int8, count, p + 5)
                stride, moves = int(arr[0]), arr[1:].astype(np.uint8)
                p += 5 + count
            else:
                raise AssertionError(f"unexpected tag type {typ}")
        assert p == len(rec)
        out.append(dict(at=at, size=4 + block_size, ref=ref, pos=pos, mapq=mapq, bin=bin_, n_cigar=n_cigar, flag=flag,
                        next_ref=nref, next_pos=npos, tlen=tlen, name=name, seq=seq[:l_seq], pad=pad, qual=bytes(qual),
                        tags=tags, moves=moves, stride=stride))
        at += 4 + block_size
    assert at == len(stream)
    return out


def parse_bgzf(data):
    """The blocks of a BGZF stream as ``(offset, BSIZE + 1, payload, crc, isize)``, by SAMv1 section 4.1."""
    out, at = [], 0
    while at < len(data):
        head = data[at:at + 18]
        assert head[:16] == bytes.fromhex("1f8b08040000000000ff060042430200"), at
        size = struct.unpack_from("<H", head, 16)[0] + 1
        body = data[at + 18:at + size - 8]
        crc, isize = struct.unpack_from("<II", data, at + size - 8)
        out.append((at, size, body, crc, isize))
        at += size
    assert at == len(data)
    return out


def stored_payload(body):
    """The bytes of a deflate stream that is one final stored block."""
    n, nn = struct.unpack_from("<HH", body, 1)
    assert body[0] == 1 and n ^ nn == 0xFFFF and len(body) == 5 + n
    return body[5:]


# ---- cases ---------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    ids: np.ndarray
    seq: np.ndarray          # base_capacity bytes
    qual: np.ndarray         # or None
    read_bases: np.ndarray   # int64, reads + 1: may run beyond the capacity
    status: np.ndarray       # int32
    tags: list = field(default_factory=list)   # [(name, uint32 values)]
    keep: np.ndarray = None
    reverse: bool = False
    codes: np.ndarray = None                   # None: no move table
    read_frames: np.ndarray = None             # int64, reads + 1
    stride: int = 5
    frame_base: int = 0
    stream_capacity: int = None                # None: bam_bound
    out_offset: int = 0                        # bytes between a 16-byte address and out

    @property
    def moves(self):
        return None if self.codes is None else (self.codes, self.read_frames, self.stride, self.frame_base)

    def capacity(self, layout):
        """Bytes of ``out``."""
        s = self.stream_capacity
        if s is None:
            s = bam_bound(len(self.status), len(self.seq), len(self.tags), None if self.codes is None else len(self.codes))
        return bgzf_bound(s) if layout == "bgzf" else s

    def expected(self, layout):
        """``(file bytes, stream, rec_off, status, written)``."""
        bgzf = layout == "bgzf"
        stream, off, st, written = bam_records_signal(
            self.ids, self.seq, self.qual, self.read_bases, self.status, self.tags, self.keep, self.reverse, self.moves,
            len(self.seq), self.capacity(layout), bgzf)
        data = bgzf_blocks_signal(stream) if bgzf else stream
        assert len(stream) == int(written[0]) and len(data) == int(written[1]) <= self.capacity(layout)
        return data, stream, off, st, written


def make(name, lengths, seed, *, frames="auto", status=None, keep=None, tags=(), reverse=False, cut=0, qual=True,
         stream_capacity=None, out_offset=0, frame_base=0, stride=5, seq_bytes=None, qual_bytes=None):
    """A case of reads of the given base counts; frames: per-read frame counts, "auto" (2 m + 3) or None (no move
    table); the last `cut` bases lie beyond the capacity."""
    rng = np.random.default_rng(seed)
    n = len(lengths)
    rb = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    cap = int(rb[-1]) - cut
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, cap)] if seq_bytes is None else np.asarray(seq_bytes, np.uint8)
    q = rng.integers(33, 127, cap).astype(np.uint8) if qual_bytes is None else np.asarray(qual_bytes, np.uint8)
    assert len(seq) == cap and len(q) == cap
    ids = rng.integers(0, 256, (n, 16)).astype(np.uint8)
    status = np.zeros(n, np.int32) if status is None else np.asarray(status, np.int32)
    keep = None if keep is None else np.asarray(keep, np.uint8)
    tags = [(k, np.asarray(v, np.uint32)) for k, v in tags]
    codes = rf = None
    if frames is not None:
        F = [2 * m + 3 for m in lengths] if isinstance(frames, str) else list(frames)
        rf = (np.concatenate([[0], np.cumsum(F)]) + frame_base).astype(np.int64)
        codes = rng.integers(0, 256, int(rf[-1]) - frame_base).astype(np.uint8)
    return Case(name, ids, seq, q if qual else None, rb, status, tags, keep, reverse, codes, rf, stride, frame_base,
                stream_capacity, out_offset)


def kept_mask(c):
    """The reads with a record (whatever the capacity)."""
    _, off, _, _ = bam_records_signal(c.ids, c.seq, c.qual, c.read_bases, c.status, c.tags, c.keep, c.reverse, c.moves,
                                      len(c.seq))
    return np.diff(off.astype(np.int64)) > 0


def record_length(m, ntags, F=None):
    return FRONT + (m + 1) // 2 + m + 7 * ntags + (0 if F is None else 9 + F)


# ---- small reads: the nibble phase, a last half byte, every alignment of record and source ---------------------------
def small_reads(out_offset=0, reverse=False, qual=True, stream_capacity=None, name="small", frames="auto"):
    rng = np.random.default_rng(5)
    lengths = [0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65] + rng.integers(1, 90, 100).tolist()
    n = len(lengths)
    c = make(f"{name}+{out_offset}", lengths, 6, tags=[("qs", rng.integers(0, 60, n)), ("ch", rng.integers(0, 3000, n))],
             reverse=reverse, out_offset=out_offset, qual=qual, stream_capacity=stream_capacity, frames=frames)
    _, _, off, _, _ = c.expected("raw")
    k = kept_mask(c)
    assert not k[0] and k[1:].all()
    assert set((off[:-1][k] % 16).tolist()) == set(range(16)), "record starts at every residue of 16"
    assert {0, 1} == set((np.diff(c.read_bases)[k] % 2).tolist())
    return c


# ---- a BGZF seam inside each field -----------------------------------------------------------------------------------
SEAM_M, SEAM_F, SEAM_TAG = 21, 50, 0x01020304
_SL = (SEAM_M + 1) // 2
SEAM_BYTES = {"block_size": 2, "name": 36 + 10, "seq": FRONT + 4, "seq_last": FRONT + _SL - 1, "qual": FRONT + _SL + 7,
              "tag_value": FRONT + _SL + SEAM_M + 3 + 2, "mv_count": FRONT + _SL + SEAM_M + 7 + 4 + 2,
              "mv_stride": FRONT + _SL + SEAM_M + 7 + 8, "moves": FRONT + _SL + SEAM_M + 7 + 9 + 20}


def seam_case(which, reverse=False):
    """Two filler reads in front place byte `which` of the third read's record directly behind the first seam."""
    P = SEAM_BYTES[which]
    m0, m1 = 2001, 40
    fixed = record_length(m0, 1, 0) + record_length(m1, 1, 0)
    F0 = (B - P - fixed) // 2
    F1 = B - P - fixed - F0
    c = make(f"seam-{which}" + ("-reverse" if reverse else ""), [m0, m1, SEAM_M, 3, 40, 1], 11,
             frames=[F0, F1, SEAM_F, 9, 100, 4], tags=[("rn", [7, 77, SEAM_TAG, 1, 2, 3])], reverse=reverse)
    _, stream, off, st, _ = c.expected("raw")
    assert int(off[2]) + P == B and int(off[3]) > B, which
    rec = stream[int(off[2]):int(off[3])]
    assert len(rec) == record_length(SEAM_M, 1, SEAM_F)
    got = parse_records(rec)[0]
    assert got["tags"] == [("rn", SEAM_TAG)] and len(got["moves"]) == SEAM_F
    if which == "tag_value":
        assert rec[P - 2:P + 2] == struct.pack("<I", SEAM_TAG)
    if which == "mv_count":
        assert rec[P - 2:P + 2] == struct.pack("<I", 1 + SEAM_F)
    if which == "mv_stride":
        assert rec[P] == c.stride and rec[P - 8:P - 4] == b"mvBc"
    if which == "moves":
        assert rec[P] == (c.codes[int(c.read_frames[2]) + 20] >> 7)
    return c


# ---- exact stream lengths ------------------------------------------------------------------------------------------
def exact_stream(W):
    """Reads whose records fill exactly W stream bytes (W a positive member of W_CASES that records can reach)."""
    m = [1500, 30, 7]
    fixed = sum(record_length(x, 0, 0) for x in m)
    rest = W - fixed
    F = [rest // 2, rest - rest // 2 - 11, 11]
    c = make(f"exact-{W}", m, 12, frames=F)
    _, stream, off, _, written = c.expected("bgzf")
    assert len(stream) == W == int(written[0]) and int(written[1]) == W + 31 * (-(-W // B))
    return c


# ---- one long read over several blocks -------------------------------------------------------------------------------
def long_read(reverse=False):
    c = make("long" + ("-reverse" if reverse else ""), [40, 150_000, 5, 1, 70], 21, frames=[90, 400_000, 12, 2, 150],
             tags=[("qs", [1, 2, 3, 4, 5])], reverse=reverse)
    _, _, off, _, _ = c.expected("raw")
    assert (int(off[2]) - 1) // B - int(off[1]) // B >= 9, "one record over ten blocks"
    return c


def many_one_base(n=2200):
    c = make("many", [1] * n, 22, frames=None)
    _, _, off, _, _ = c.expected("raw")
    assert B // int(off[1]) > 800 and int(off[-1]) > 2 * B, "nearly as many records in a block as the workgroup has threads"
    return c


# ---- bytes ----------------------------------------------------------------------------------------------------------
def byte_values():
    """Every byte value in seq at either nibble, lower case, and the quality bytes at the clamp's edges."""
    seq = np.concatenate([np.arange(256), np.arange(256)[::-1], [ord("a")], np.frombuffer(b"acgtnACGTN=mrswyhkdbv", np.uint8)])
    lengths = [256, 257, len(seq) - 513]
    qual = np.resize(np.array([0, 32, 33, 126, 127, 255, 34, 125], np.uint8), len(seq))
    c = make("bytes", lengths, 23, seq_bytes=seq.astype(np.uint8), qual_bytes=qual, frames="auto")
    _, stream, _, _, _ = c.expected("raw")
    recs = parse_records(stream)
    assert recs[2]["seq"] == "ACGTNACGTN=MRSWYHKDBV" and recs[1]["seq"][-1] == "A" and recs[0]["seq"][ord("c")] == "C" and recs[0]["seq"][0] == "N"
    assert set(recs[0]["qual"][:6]) == {0, 93} and recs[0]["qual"][2:4] == bytes([0, 93])
    return c


# ---- reads without a record ----------------------------------------------------------------------------------------
def without_record():
    """Statuses, keep == 0, empty reads, reads beyond the base capacity and reads outside the frame window, singly
    and in runs, at the call's start and end."""
    rng = np.random.default_rng(31)
    lengths = [4, 0, 6, 9, 1, 1, 700, 2, 3, 0, 8, 5, 7, 0, 0, 30, 12, 6, 6, 6, 9, 9, 9]
    n = len(lengths)
    status, keep = np.zeros(n, np.int32), np.ones(n, np.uint8)
    status[0], keep[2] = 6, 0
    status[7], keep[8], status[10] = BAD, 0, 1
    keep[12] = 0
    status[17], keep[18] = 3, 0
    cut = 9 + 9 + 4
    c = make("without", lengths, 32, status=status, keep=keep, cut=cut, tags=[("ch", rng.integers(0, 9, n))], frame_base=1000)
    c.codes = c.codes[:int(c.read_frames[16]) - 1000 - 1]   # read 15 ends one frame beyond the window
    _, _, off, st, _ = c.expected("raw")
    k = kept_mask(c)
    assert not k[:3].any() and not k[-3:].any() and k[3] and k[11] and not k[15] and st[15] == BAD
    assert (st[16:20] == [BAD, 3, 0, BAD]).all(), "reads behind the window's end are refused where they would be kept"
    assert st[0] == 6 and st[7] == BAD and st[10] == 1 and st[1] == 0 and st[-1] == 0 and st[2] == 0
    return c


def outside_window():
    """frame_base above the first reads' frames, and a read whose frames run backwards."""
    c = make("window", [5, 6, 7, 8, 9, 10], 33, frames=[10, 12, 14, 16, 18, 20])
    rf = c.read_frames.copy()
    base = int(rf[2])
    c.frame_base, c.codes = base, c.codes[base:]
    rf[5] = rf[4] - 1                                   # read 4 runs backwards; read 5 is longer by as much
    c.read_frames = rf
    _, stream, off, st, _ = c.expected("raw")
    assert st.tolist() == [BAD, BAD, 0, 0, BAD, 0] and len(parse_records(stream)) == 3
    return c


def no_kept_read():
    c = make("none", [3, 0, 5, 2, 0, 0, 7, 1, 1], 34, status=[6, 0, 0, 1, 0, 0, BAD, 0, 0], keep=[1, 1, 0, 1, 1, 1, 1, 0, 0])
    data, stream, off, st, written = c.expected("bgzf")
    assert data == b"" and not off.any() and not written.any()
    return c


# ---- tags ----------------------------------------------------------------------------------------------------------
def tag_cases():
    values = [0, 9, 255, 256, 65535, 65536, 0x7FFFFFFF, 0x80000000, 4294967295, 12345]
    n = len(values)
    rng = np.random.default_rng(41)
    lengths = rng.integers(1, 40, n).tolist()
    names = ["qs", "ch", "rn", "tr", "ns", "Z9", "a0", "mx"]
    cols = [(names[k], np.roll(np.array(values, np.uint64), k).astype(np.uint32)) for k in range(8)]
    cases = [make("tags0", lengths, 42), make("tags8", lengths, 44, tags=cols), make("tags8-nomoves", lengths, 45, tags=cols, frames=None)]
    _, stream, _, _, _ = cases[1].expected("raw")
    assert parse_records(stream)[0]["tags"] == [(names[k], int(cols[k][1][0])) for k in range(8)]
    return cases


# ---- capacities ----------------------------------------------------------------------------------------------------
def capacity_cases():
    """A stream capacity exactly at, one byte short of and one byte past a record's end, in the middle and at the
    stream's end, and 0."""
    full = small_reads()
    _, _, off, _, _ = full.expected("raw")
    k = np.flatnonzero(kept_mask(full))
    mid = int(k[len(k) // 2])
    out = []
    for label, cap, written in (("at", int(off[mid + 1]), len(k) // 2 + 1), ("short", int(off[mid + 1]) - 1, len(k) // 2),
                                ("past", int(off[mid + 1]) + 1, len(k) // 2 + 1), ("total", int(off[-1]), len(k)),
                                ("total-short", int(off[-1]) - 1, len(k) - 1), ("zero", 0, 0)):
        c = small_reads(stream_capacity=cap, name=f"capacity-{label}")
        for layout in LAYOUTS:
            _, stream, off2, st, wr = c.expected(layout)
            assert np.array_equal(off2, off) and int((st[k] == 0).sum()) == written, (label, layout)
            assert int((st == SMALL).sum()) == len(k) - written and int(wr[0]) == (int(off[k[written - 1] + 1]) if written else 0)
        out.append(c)
    return out


def seam_capacity_cases():
    """A capacity at and one byte short of the end of a record that a seam cuts: two blocks, or one short one."""
    out = []
    for label, delta in (("seam-at", 0), ("seam-short", -1)):
        c = seam_case("moves")
        _, _, off, _, _ = c.expected("raw")
        c.name, c.stream_capacity = f"capacity-{label}", int(off[3]) + delta
        for layout in LAYOUTS:
            data, stream, _, st, wr = c.expected(layout)
            assert int(wr[0]) == (int(off[3]) if delta == 0 else int(off[2])) and (int(wr[0]) > B) == (delta == 0)
            assert (st[2:] == ([0] + [SMALL] * 3 if delta == 0 else [SMALL] * 4)).all()
        out.append(c)
    return out


def block_capacity():
    """A BGZF buffer whose last block may hold 1 byte, 0 bytes and no header: the stream capacity follows."""
    for cap, S in ((FILE + 32, B + 1), (FILE + 31, B), (FILE + 5, B), (FILE, B), (FILE - 1, B - 1), (31, 0), (32, 1)):
        assert bgzf_stream_capacity(cap) == S, cap
    c = exact_stream(B + 1)
    c.name = "block-capacity"
    return c


def empty_call():
    return make("empty", [], 61)


@functools.lru_cache(maxsize=None)
def record_cases():
    """Every case of the record call, built once a process; nothing changes a case."""
    cases = [small_reads()] + [seam_case(w) for w in SEAM_BYTES] + [seam_case("seq", reverse=True)]
    cases += [exact_stream(W) for W in W_CASES if W > 1] + [long_read(), many_one_base(), byte_values(), without_record(),
                                                            outside_window(), no_kept_read()]
    cases += tag_cases() + [long_read(reverse=True), small_reads(reverse=True, name="small-reverse"),
                            small_reads(qual=False, name="small-noqual"), small_reads(frames=None, name="small-nomoves"),
                            small_reads(qual=False, reverse=True, frames=None, name="small-ctc")]
    cases += [small_reads(out_offset=o) for o in (1, 15)] + capacity_cases() + seam_capacity_cases()
    cases += [block_capacity(), empty_call()]
    names = [c.name for c in cases]
    assert len(set(names)) == len(names), names
    return cases
