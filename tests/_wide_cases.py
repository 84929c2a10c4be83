"""The arithmetic of the wide-stream tests (tests/test_gpu_wide_streams.py): streams whose byte offsets pass 2^32
through pgn_bgzf_deflate_device, pgn_bam_records_device and pgn_fastq_records_device.

Each input is periodic, so the output is: one period is held to the host model, every other period to the first on
the device.  Here are the periods, the repetition counts, ``blk_off`` and ``rec_off`` as closed forms, and the
indices of the blocks and records that contain byte 2^32.  tests/test_wide_cases.py asserts the conditions the
designs rest on without a GPU: a design that drifts fails there.
"""
import functools
from dataclasses import dataclass

import numpy as np

import _bam_cases
from rawnanoporesignalcompression_amd import _native
from rawnanoporesignalcompression_amd.host import (bam_records_signal, bgzf_blocks_signal, bgzf_bound,
                                                   bgzf_deflate_signal, fastq_records_signal)

B = _native.PGN_BGZF_BLOCK_BYTES
FILE = B + 31                                     # a BGZF block with a stored deflate block of B bytes
T = _native.PGN_FASTQ_TILE_BYTES
SMALL = _native.PGN_ERR_DST_TOO_SMALL
WIDE = 1 << 32
GIB = 1 << 30
MEMORY_CAP = 12 * GIB                             # a test's peak device memory
MEMORY_NEEDED = 16 * GIB                          # free device memory below which a test may skip
CHUNK_BYTES = 256 << 20                           # of one comparison: the largest temporary, far below 1 GiB
DOWNLOAD_CAP = 64 << 20
PLAN_BYTES = 1568                                 # the deflate call's scratch per block (include/pgnano_hip.h)


def row_chunks(rows, row_bytes):
    """``(first, end)`` row ranges of at most CHUNK_BYTES bytes each."""
    step = max(1, CHUNK_BYTES // row_bytes)
    return [(a, min(a + step, rows)) for a in range(0, rows, step)]


# ---- deflate ---------------------------------------------------------------------------------------------------------
TAIL = 777
OUT_OFFSET = 5                                    # bytes between a 16-byte address and out


@dataclass
class Deflate:
    period: bytes          # three blocks of B bytes: dynamic at about 0.5, stored, dynamic at 0.95 or more
    tail: bytes            # TAIL bytes behind the last period
    first: bytes           # the file bytes of one period
    tail_file: bytes       # the file bytes of the tail block
    sizes: tuple           # the three blocks' file lengths
    reps: int

    @property
    def S(self):
        return sum(self.sizes)

    @property
    def src_bytes(self):
        return self.reps * 3 * B + TAIL

    @property
    def ntiles(self):
        return 3 * self.reps + 1

    @property
    def total(self):
        return self.reps * self.S + len(self.tail_file)

    def blk_off(self):
        """The scan of all blocks' file lengths, ntiles + 1 entries: ``(k // 3) * S`` plus the lengths of the
        period's blocks in front of block ``k % 3``, then the total."""
        k = np.arange(3 * self.reps + 1, dtype=np.uint64)
        pre = np.array([0, self.sizes[0], self.sizes[0] + self.sizes[1]], np.uint64)
        return np.concatenate([k // np.uint64(3) * np.uint64(self.S) + pre[(k % np.uint64(3)).astype(np.int64)],
                               np.array([self.total], np.uint64)])

    def block_file(self, k):
        """The file bytes of block k < 3 * reps."""
        pre = [0, self.sizes[0], self.sizes[0] + self.sizes[1], self.S]
        return self.first[pre[k % 3]:pre[k % 3 + 1]]

    def block_payload(self, k, n=B):
        return self.period[(k % 3) * B:(k % 3) * B + n]

    def first_block_past(self, value):
        """The first j with blk_off[j] > value."""
        return int(np.searchsorted(self.blk_off(), np.uint64(value), "right"))

    def block_of_file_byte(self, at):
        return self.first_block_past(at) - 1

    def cut(self, nbytes):
        """``(blk_off, written, last block's index, its payload bytes, its file bytes)`` of the call that reads
        ``nbytes < reps * 3 * B`` stream bytes of the same source: entries above the last block repeat the total."""
        assert nbytes < self.reps * 3 * B
        nb = -(-nbytes // B)
        n = nbytes - (nb - 1) * B
        last = bgzf_deflate_signal(self.block_payload(nb - 1, n))[0]
        off = self.blk_off()
        total = int(off[nb - 1]) + len(last)
        off[nb:] = total
        return off, np.array([nbytes, total], np.uint64), nb - 1, n, last

    def memory(self):
        """Device bytes of the test: the source, the sentinel-filled output, the call's scratch and offsets, and a
        comparison's temporaries."""
        return self.src_bytes + (64 + OUT_OFFSET + self.total + 80) + self.ntiles * (PLAN_BYTES + 8) + 3 * CHUNK_BYTES


@functools.lru_cache(maxsize=None)
def deflate():
    for seed in range(100, 200):
        rng = np.random.default_rng(seed)
        half = (rng.integers(0, 16, B) * 17).astype(np.uint8)                    # 16 values: 4 bits a byte
        flat = rng.integers(0, 256, B).astype(np.uint8)                          # stored
        p = np.where(np.arange(256) % 2 == 0, 2.0, 1.0)
        mild = rng.choice(256, B, p=p / p.sum()).astype(np.uint8)                # 7.9 bits a byte
        period = np.concatenate([half, flat, mild]).tobytes()
        first, off, _ = bgzf_deflate_signal(period)
        sizes = tuple(np.diff(off.astype(np.int64)).tolist())
        if sum(sizes) % 2 == 0:
            continue                                                             # re-seed: S must be odd
        S = sum(sizes)
        reps = -(-(WIDE + 3 * S) // S)
        tail = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, TAIL)].tobytes()
        return Deflate(period, tail, first, bgzf_deflate_signal(tail)[0], sizes, reps)
    raise AssertionError("no seed gives a period of odd file length")


# the call that reads 2^32 + B + 1 bytes ends with a block of (2^32 + 1) % B = 257 bytes; the one a block later, by
# 256 bytes fewer, ends with a block of one byte
NBYTES_PAST = WIDE + B + 1
NBYTES_ONE = (WIDE // B + 2) * B + 1


# ---- records: identical reads ------------------------------------------------------------------------------------------
TAG = ("qs", 12)


@dataclass
class Reads:
    m: int                 # bases of a read
    F: int                 # frames of a read, or None
    n: int                 # reads
    R: int                 # a record's bytes
    one: dict              # a read's id, bases, qualities and frame codes

    def arrays(self, n):
        """The host model's arguments for the first n reads."""
        o = self.one
        rb = np.arange(n + 1, dtype=np.int64) * self.m
        args = dict(read_ids=np.tile(o["id"], (n, 1)), seq=np.tile(o["seq"], n), qual=np.tile(o["qual"], n), read_bases=rb,
                    status=np.zeros(n, np.int32), tags=[(TAG[0], np.full(n, TAG[1], np.uint32))])
        if self.F is not None:
            args["moves"] = (np.tile(o["codes"], n), np.arange(n + 1, dtype=np.int64) * self.F, 5)
        return args

    @property
    def stream_bytes(self):
        return self.n * self.R

    def input_bytes(self):
        return self.n * (2 * self.m + (self.F or 0) + 16 + 4 + 4 + 8 + 8 + 8) + 64


def _one_read(m, F, seed):
    rng = np.random.default_rng(seed)
    return dict(id=rng.integers(0, 256, 16).astype(np.uint8), seq=np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, m)],
                qual=rng.integers(33, 127, m).astype(np.uint8), codes=None if F is None else rng.integers(0, 256, F).astype(np.uint8))


BAM_R = 7680                                      # 512 * 15: 17 records fill two blocks of 65,280, no whole number one
BAM_PAIR = 2 * B // BAM_R


def _bam(m, seed):
    F = BAM_R - _bam_cases.record_length(m, 1, 0)
    pairs = -(-(WIDE + 3 * B) // (2 * B))
    return Reads(m, F, BAM_PAIR * pairs, _bam_cases.record_length(m, 1, F), _one_read(m, F, seed))


@functools.lru_cache(maxsize=None)
def bam_frames():
    """Short reads with long move tables: the frame offsets pass 2^31 (the raw layout's shape)."""
    return _bam(1001, 201)


@functools.lru_cache(maxsize=None)
def bam_bases():
    """Long reads with short move tables: read_bases pass 2^31 (the BGZF layout's shape)."""
    return _bam(4001, 202)


def bam_model(r, n, bgzf=False, byte_capacity=None):
    """``(stream, rec_off, status, written)`` of the first n reads."""
    return bam_records_signal(**r.arrays(n), bgzf=bgzf, byte_capacity=byte_capacity)


def bam_file(r, n):
    """``(file bytes, written)`` of the first n reads in the BGZF layout."""
    stream, _, _, written = bam_model(r, n, bgzf=True)
    return bgzf_blocks_signal(stream), written


def bam_cut(r):
    """A capacity inside the first record that begins past 2^32: ``(capacity, that record's index)``."""
    first = -(-WIDE // r.R)
    return first * r.R + r.R // 2, first


@functools.lru_cache(maxsize=None)
def fastq():
    m = 1001
    one = _one_read(m, None, 203)
    r = Reads(m, None, 1, 0, one)
    text, off, _ = fastq_records_signal(**r.arrays(1))
    R = len(text)
    return Reads(m, None, -(-(WIDE + 3 * T) // R), R, one)


def fastq_model(r, n, reverse=False, byte_capacity=None):
    """``(text, rec_off, status)`` of the first n reads."""
    return fastq_records_signal(**r.arrays(n), reverse=reverse, byte_capacity=byte_capacity)


def fastq_cut(r):
    """A capacity one byte short of the end of the record that contains byte 2^32: ``(capacity, its index)``."""
    at = WIDE // r.R
    return (at + 1) * r.R - 1, at


def records_memory(r, out_bytes):
    return r.input_bytes() + 64 + out_bytes + 80 + 3 * CHUNK_BYTES
