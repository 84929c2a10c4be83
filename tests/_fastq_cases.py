"""Cases for the FASTQ record call and the mean-quality call (include/pgnano_hip.h "FASTQ records"), built once for
the CPU tests (tests/test_fastq_api.py) and the GPU tests (tests/test_gpu_fastq.py, tests/test_gpu_read_qual.py).

Every builder asserts here, on the CPU, the condition its case exists for (a record byte directly behind a tile
boundary, every residue of the offsets modulo 16, an error sum that equals a threshold times the count), from the
host models' own outputs: a case list that drifts fails without a GPU.
"""
import functools
from dataclasses import dataclass, field

import numpy as np

from rawnanoporesignalcompression_amd import _native
from rawnanoporesignalcompression_amd.host import err_table, fastq_bound, fastq_records_signal, read_qual_signal

T = _native.PGN_FASTQ_TILE_BYTES
QT = _native.PGN_READ_QUAL_TILE_BASES
BAD = _native.PGN_ERR_INVALID_ARG
TAG_VALUES = [0, 9, 10, 99, 100, 999, 1000, 9999, 10000, 99999, 100000, 999999, 1000000, 9999999, 10000000, 99999999,
              100000000, 999999999, 1000000000, 4294967295]


@dataclass
class Case:
    name: str
    ids: np.ndarray
    seq: np.ndarray          # base_capacity bytes
    qual: np.ndarray
    read_bases: np.ndarray   # int64, reads + 1: may run beyond the capacity
    status: np.ndarray       # int32
    tags: list = field(default_factory=list)   # [(name, uint32 values)]
    keep: np.ndarray = None
    reverse: bool = False
    byte_capacity: int = None                  # None: fastq_bound
    out_offset: int = 0                        # bytes between a 16-byte address and out

    @property
    def capacity(self):
        n = len(self.status)
        return fastq_bound(n, len(self.seq), len(self.tags)) if self.byte_capacity is None else self.byte_capacity

    def expected(self):
        return fastq_records_signal(self.ids, self.seq, self.qual, self.read_bases, self.status, self.tags, self.keep,
                                    self.reverse, len(self.seq), self.capacity)


def make(name, lengths, seed, *, status=None, keep=None, tags=(), reverse=False, cut=0, byte_capacity=None, out_offset=0):
    """A case of reads of the given base counts; the last `cut` bases lie beyond the capacity."""
    rng = np.random.default_rng(seed)
    n = len(lengths)
    rb = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    cap = int(rb[-1]) - cut
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, cap)]
    qual = rng.integers(33, 127, cap).astype(np.uint8)
    ids = rng.integers(0, 256, (n, 16)).astype(np.uint8)
    status = np.zeros(n, np.int32) if status is None else np.asarray(status, np.int32)
    keep = None if keep is None else np.asarray(keep, np.uint8)
    tags = [(k, np.asarray(v, np.uint32)) for k, v in tags]
    return Case(name, ids, seq, qual, rb, status, tags, keep, reverse, byte_capacity, out_offset)


def kept_mask(c):
    n = len(c.status)
    m = np.diff(c.read_bases)
    ok = (c.status == 0) & (m > 0) & (c.read_bases[1:] <= len(c.seq))
    return ok & (np.ones(n, bool) if c.keep is None else c.keep != 0)


# ---- small reads ---------------------------------------------------------------------------------------------------
def small_reads(out_offset=0, reverse=False, byte_capacity=None, name="small"):
    rng = np.random.default_rng(5)
    lengths = [0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65] + rng.integers(1, 90, 100).tolist()
    n = len(lengths)
    c = make(f"{name}+{out_offset}", lengths, 6, tags=[("qs", rng.integers(0, 60, n)), ("ch", rng.integers(0, 3000, n))],
             reverse=reverse, out_offset=out_offset, byte_capacity=byte_capacity)
    _, off, _ = c.expected()
    k = kept_mask(c)
    assert set((off[:-1][k] % 16).tolist()) == set(range(16)), "record starts at every residue of 16"
    assert set((c.read_bases[:-1][k] % 16).tolist()) == set(range(16)), "sources at every residue of 16"
    return c


# ---- tile seams ----------------------------------------------------------------------------------------------------
SEAM_M, SEAM_TAG = 20, 12345           # the record behind the filler: 20 bases, one tag of 5 digits
_H = 1 + 36 + 6 + 5 + 1                # its header with the newline
SEAM_BYTES = {"at": 0, "uuid": 5, "hyphen": 9, "tab": 37, "digits": 45, "header_newline": _H - 1, "seq_first": _H,
              "seq_last": _H + SEAM_M - 1, "plus": _H + SEAM_M + 1, "qual_first": _H + SEAM_M + 3,
              "qual_last": _H + 2 * SEAM_M + 2, "final_newline": _H + 2 * SEAM_M + 3}


def seam_case(which, reverse=False):
    """A filler read in front places byte `which` of the second read's record directly behind a tile boundary."""
    P = SEAM_BYTES[which]
    d0 = 1 if (42 + 6 + 1 + P) % 2 == 0 else 2            # the filler's tag digits make the rest even
    mf = (T - 42 - 6 - d0 - P) // 2
    c = make(f"seam-{which}", [mf, SEAM_M, 3, 40, 1], 11, tags=[("rn", [7 if d0 == 1 else 77, SEAM_TAG, 1, 2, 3])],
             reverse=reverse)
    text, off, st = c.expected()
    at = int(off[1]) + P
    assert at % T == 0 and at > 0, which
    rec = text[int(off[1]):int(off[2])]
    assert len(rec) == _H + 2 * SEAM_M + 4
    want = {"at": b"@", "hyphen": b"-", "tab": b"\t", "digits": b"3", "header_newline": b"\n", "plus": b"+",
            "final_newline": b"\n"}.get(which)
    if want:
        assert rec[P:P + 1] == want, which
    src = {"seq_first": (c.seq, 0), "seq_last": (c.seq, SEAM_M - 1), "qual_first": (c.qual, 0),
           "qual_last": (c.qual, SEAM_M - 1)}.get(which)
    if src:
        b0 = int(c.read_bases[1])
        assert rec[P] == src[0][b0 + (SEAM_M - 1 - src[1] if reverse else src[1])], which
    if which == "uuid":
        assert chr(rec[P]) in "0123456789abcdef"
    return c


# ---- long and many -------------------------------------------------------------------------------------------------
def long_record(reverse=False):
    m = 3 * T // 2 + 7
    c = make("long" + ("-reverse" if reverse else ""), [m, 5, 1, 70], 21, tags=[("qs", [1, 2, 3, 4])], reverse=reverse)
    _, off, _ = c.expected()
    assert (int(off[1]) - 1) // T - int(off[0]) // T >= 3, "one record over more than three tiles"
    return c


def many_one_base(n=1000):
    c = make("thousand", [1] * n, 22)
    _, off, _ = c.expected()
    assert T // int(off[1]) > 256, "more records in a tile than a workgroup has threads"
    assert int(off[-1]) > 2 * T
    return c


# ---- reads without a record ----------------------------------------------------------------------------------------
def without_record():
    """Each kind alone and in runs, at the call's start and end, and a run with a tile boundary on either side."""
    rng = np.random.default_rng(31)
    first = (T - 67 - 51 - 51 - 49) // 2           # ends the fourth kept record exactly at the first tile boundary
    lengths = [4, 0, 6, 9, 1, 1, first, 2, 3, 0, 8, 5, 7, 0, 0, 30, 12, 6, 6, 6, 9, 9, 9]
    n = len(lengths)
    status = np.zeros(n, np.int32)
    keep = np.ones(n, np.uint8)
    status[0], keep[2] = 6, 0                      # the start: a status, an empty read, keep == 0
    status[7], keep[8], status[10] = BAD, 0, 1     # a run behind the boundary: status, keep, empty, status
    keep[12] = 0                                   # singly
    status[17], keep[18] = 3, 0
    cut = 9 + 9 + 4                                # the last two reads and a part of the one before lie beyond
    c = make("without", lengths, 32, status=status, keep=keep, cut=cut, tags=[("ch", rng.integers(0, 9, n))])
    text, off, st = c.expected()
    k = kept_mask(c)
    assert not k[:3].any() and not k[-3:].any() and k[3] and k[-4]
    assert int(off[7]) == T and not k[7:11].any() and k[11], "a run directly behind a tile boundary"
    assert st[0] == 6 and st[7] == BAD and st[10] == 1 and st[17] == 3 and st[1] == 0 and st[-1] == 0
    return c


def run_across_boundary():
    """A run of reads without a record inside a record pair that a tile boundary cuts."""
    mf = (T - 49 - 31) // 2                        # the record behind the run starts 31 bytes in front of the boundary
    n = 40
    lengths = [mf] + [2] * 30 + [25, 3] + [4] * 7
    keep = np.ones(n, np.uint8)
    keep[1:31] = 0
    c = make("run-across", lengths, 33, keep=keep, tags=[("rn", np.arange(n))])
    _, off, _ = c.expected()
    assert int(off[31]) == int(off[1]) < T < int(off[32]), "the boundary lies inside the record behind the run"
    return c


def no_kept_read():
    n = 9
    c = make("none", [3, 0, 5, 2, 0, 0, 7, 1, 1], 34, status=[6, 0, 0, 1, 0, 0, BAD, 0, 0], keep=[1, 1, 0, 1, 1, 1, 1, 0, 0])
    text, off, st = c.expected()
    assert text == b"" and not off.any() and not kept_mask(c).any()
    return c


# ---- tags ----------------------------------------------------------------------------------------------------------
def tag_cases():
    n = len(TAG_VALUES)
    rng = np.random.default_rng(41)
    lengths = rng.integers(1, 40, n).tolist()
    names = ["qs", "ch", "rn", "tr", "ns", "Z9", "a0", "mx"]
    cols = [(names[k], np.roll(np.array(TAG_VALUES, np.uint64), k).astype(np.uint32)) for k in range(8)]
    cases = [make("tags0", lengths, 42), make("tags1", lengths, 43, tags=cols[:1]), make("tags8", lengths, 44, tags=cols)]
    text, off, _ = cases[2].expected()
    assert b"\tqs:i:4294967295\tch:i:1000000000\t" in text and b"\tqs:i:0\t" in text
    return cases


# ---- reverse -------------------------------------------------------------------------------------------------------
def reverse_cases():
    c = make("reverse", [1, 2, 7, 8, 33, 16, 100], 51, tags=[("qs", [5] * 7)], reverse=True)
    text, off, _ = c.expected()
    assert text[int(off[2]):int(off[3])].split(b"\n")[1] == c.seq[3:10][::-1].tobytes()
    return [c, long_record(reverse=True), small_reads(reverse=True, name="small-reverse")]


# ---- byte capacity -------------------------------------------------------------------------------------------------
def capacity_cases():
    """(case, records written) for a capacity equal to the total, one below, inside an earlier SEQ, and 0."""
    full = small_reads()
    _, off, _ = full.expected()
    total, n = int(off[-1]), len(full.status)
    k = np.flatnonzero(kept_mask(full))
    m = np.diff(full.read_bases)
    at = next(i for i in range(len(k) // 2, len(k)) if m[k[i]] >= 2)
    mid = int(k[at])
    header = int(off[mid + 1] - off[mid]) - 2 * int(m[mid]) - 4
    inside = int(off[mid]) + header + int(m[mid]) // 2          # in the SEQ of a record in the middle
    assert int(off[mid]) + header <= inside < int(off[mid]) + header + int(m[mid])
    out = []
    for cap, written in ((total, len(k)), (total - 1, len(k) - 1), (inside, at), (0, 0)):
        c = small_reads(byte_capacity=cap, name=f"capacity{cap}")
        text, off2, st = c.expected()
        assert np.array_equal(off2, off) and int((st[k] == 0).sum()) == written
        assert int((st == _native.PGN_ERR_DST_TOO_SMALL).sum()) == len(k) - written
        out.append(c)
    return out


def empty_call():
    return make("empty", [], 61)


@functools.lru_cache(maxsize=None)
def record_cases():
    """Every case of the record call, built once a process; nothing changes a case."""
    cases = [small_reads()] + [seam_case(w) for w in SEAM_BYTES] + [long_record(), many_one_base(), without_record(),
                                                                    run_across_boundary(), no_kept_read()]
    cases += tag_cases() + reverse_cases() + [small_reads(out_offset=o) for o in (1, 3, 8, 15)] + capacity_cases()
    cases.append(empty_call())
    names = [c.name for c in cases]
    assert len(set(names)) == len(names), names
    return cases


# =====================================================================================================================
# Mean quality
# =====================================================================================================================
@dataclass
class QualCase:
    name: str
    qual: np.ndarray
    read_bases: np.ndarray
    status: np.ndarray
    thresholds: np.ndarray = None     # None: qual_thresholds
    q_min: int = 1
    skip_bases: int = 60
    min_mean_q: int = 0

    def expected(self):
        from rawnanoporesignalcompression_amd.host import qual_thresholds

        thr = qual_thresholds(q_min=self.q_min, q_max=max(self.q_min, 50)) if self.thresholds is None else self.thresholds
        return read_qual_signal(self.qual, self.read_bases, self.status, thr, q_min=self.q_min,
                                skip_bases=self.skip_bases, min_mean_q=self.min_mean_q, base_capacity=len(self.qual))


def _qual_case(name, reads, **kw):
    """reads: one uint8 array of quality bytes per read."""
    rb = np.concatenate([[0], np.cumsum([len(q) for q in reads])]).astype(np.int64)
    status = np.asarray(kw.pop("status", np.zeros(len(reads))), np.int32)
    cut = kw.pop("cut", 0)
    qual = np.concatenate([np.asarray(q, np.uint8) for q in reads] + [np.zeros(0, np.uint8)])
    return QualCase(name, qual[:len(qual) - cut], rb, status, **kw)


def table_thresholds(q_min=1, q_max=60):
    """Thresholds taken from the error table itself: a read of one quality Q throughout has U == thr[Q - q_min - 1] * n."""
    return err_table()[q_min + 1:q_max + 1]


@functools.lru_cache(maxsize=None)
def qual_cases():
    """Every case of the mean-quality call, built once a process."""
    rng = np.random.default_rng(71)
    rand = lambda m: rng.integers(33, 84, m).astype(np.uint8)
    cases = []
    cases.append(_qual_case("skip", [rand(59), rand(60), rand(61), rand(1), rand(200)]))
    cases.append(_qual_case("skip0", [rand(59), rand(60), rand(61), rand(1)], skip_bases=0))
    # the comparison's edge
    thr, q_min = table_thresholds(), 1
    err = [int(v) for v in err_table()]
    reads, want = [], []
    for Q, n in ((20, 1), (20, 7), (35, 64), (2, 5), (59, 1000), (60, 9)):
        base = np.full(n, 33 + Q, np.uint8)
        better, worse = base.copy(), base.copy()
        better[n // 2], worse[n // 2] = 33 + Q + 1, 33 + Q - 1
        reads += [base, better, worse]
        assert err[Q] * n == int(thr[Q - q_min - 1]) * n, "U equals the threshold times the count"
        want += [Q, Q + 1 if n == 1 else Q, Q - 1]        # one better base does not reach the next threshold
    edge = _qual_case("edge", reads, thresholds=thr, q_min=q_min, skip_bases=0)
    assert edge.expected()[0].tolist() == want
    cases.append(edge)
    cases.append(_qual_case("bytes", [np.array([0, 32, 33, 126, 127, 255], np.uint8), np.array([0], np.uint8),
                                      np.array([255, 127], np.uint8), np.array([126] * 70, np.uint8)], skip_bases=2))
    # a read of several tiles among one-base reads; boundaries at a tile's first and last base
    lengths = [1] * 9 + [QT - 9, 3 * QT + 5, 1, 1, QT - 8, 1, 2 * QT - 1, 1, 300]
    tiles = _qual_case("tiles", [rand(m) for m in lengths])
    assert QT in tiles.read_bases and (5 * QT - 1) in tiles.read_bases and (7 * QT - 1) in tiles.read_bases
    assert any(b % QT == 0 for b in tiles.read_bases[1:-1]) and any(b % QT == QT - 1 for b in tiles.read_bases[1:-1])
    cases.append(tiles)
    # min_mean_q at, below and above a read's mean
    uniform = [np.full(80, 33 + Q, np.uint8) for Q in (19, 20, 21)]
    gate = _qual_case("gate", uniform, thresholds=thr, q_min=q_min, min_mean_q=20)
    assert gate.expected()[0].tolist() == [19, 20, 21] and gate.expected()[2].tolist() == [0, 1, 1]
    cases.append(gate)
    # reads with a status, and reads the capacity cuts
    cases.append(_qual_case("status-cut", [rand(100), rand(5), rand(0), rand(4200), rand(70), rand(90), rand(10)],
                            status=[0, 6, 0, BAD, 0, 0, 0], cut=95))
    mq, U, ps = cases[-1].expected()
    assert mq[0] > 0 and mq[4] > 0 and not mq[[1, 2, 3, 5, 6]].any() and not U[[1, 2, 3, 5, 6]].any()
    return cases
