"""The row writer (segment_write_kernel) at the row lengths where its launch changes: odd rows at every 2-byte
and 4-byte alignment, a partial last 16-byte unit, more than 256 units (a thread's second pass over a row),
and rows shared by 2 and by 8 workgroups, the workload's own L = 10,000 among them.  Untrimmed, quantile
normalisation, both dtypes, every row bit for bit against ref_batch (tests/test_segment_api.py), the zero
padding as +0.0 bits; rows at or above total and a margin in front of the output keep their sentinel.

The launch's arithmetic is restated here from pgn_segment_reads_device: a thread stores 16-byte units (8
binary16 or 4 float32), a row has units = ceil(L / unit) of them and is shared by the smallest power of two
of threads that covers them, at most the workgroup's 256, so more than 256 units mean a second pass; the row
is split over min(8, max(1, units / 1024)) workgroups.  Each plan asserts what it is here to reach, so a
change of those thresholds shows as a test that no longer reaches its target.
"""
import numpy as np
import pytest

import _oracle as O
from test_gpu_segments import BITS, NP_OF, SENTINEL, dev, tdtype
from test_norm_api import QUANTILE
from test_segment_api import ref_batch

pytestmark = pytest.mark.gpu

UNIT = {"float16": 8, "float32": 4}
THREADS, MAX_SPLIT = 256, 8
MARGIN = 64  # elements in front of the output (a multiple of 16 bytes in both dtypes)

# (L, V, dtypes, what the plan reaches)
PLANS = [
    (1, 0, ("float16", "float32"), "odd"), (3, 1, ("float16", "float32"), "odd"), (7, 2, ("float16", "float32"), "odd"),
    (9, 0, ("float16", "float32"), "odd"), (13, 5, ("float16", "float32"), "odd"),
    (12, 4, ("float16", "float32"), "partial_unit"),
    (2052, 100, ("float16",), "second_pass"), (1028, 100, ("float32",), "second_pass"),
    (10000, 500, ("float16", "float32"), "workload"),
    (10001, 500, ("float16", "float32"), "odd_long"),
    (16384, 0, ("float16",), "split2_edge"), (8192, 0, ("float32",), "split2_edge"),
    (65536, 1000, ("float16", "float32"), "split8"),
]
CASES = [(L, V, dt, what) for L, V, dts, what in PLANS for dt in dts]


def launch(L, dtype):
    """(units, threads per row, passes, split) as pgn_segment_reads_device derives them."""
    units = -(-L // UNIT[dtype])
    tpr = 1
    while tpr < THREADS and tpr < units:
        tpr *= 2
    split = min(MAX_SPLIT, max(1, units // (4 * THREADS)))
    return units, tpr, -(-units // (tpr * split)), split


def plan_lengths(L, V):
    """L-9 .. L+1 (the end of the valid samples at every position of a unit; L+1: two rows that overlap in all
    but one sample), 2L+3, five rows, and an empty read."""
    S = L - V
    near = sorted({max(n, 0) for n in range(L - 9, L + 2)})
    return near + [2 * L + 3, L + 4 * S - (1 if S > 1 else 0), 0]


_BATCH = {}


def batch(L, V):
    """reads, flat, offsets, counts and the float32 reference of one plan (shared by both dtypes)."""
    if (L, V) not in _BATCH:
        reads = [O.synth_read(6000 + j, n) for j, n in enumerate(plan_lengths(L, V))]
        counts = np.array([r.size for r in reads], np.int64)
        offsets = 1 + np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
        flat = np.concatenate([np.array([12345], np.int16)] + reads)
        assert (offsets % 2 == 1).any() and (offsets % 2 == 0).any()
        want = ref_batch(reads, L, V, None, QUANTILE)
        _BATCH.clear()  # one plan at a time: the long plans' references are a few MB each
        _BATCH[(L, V)] = (flat, offsets, counts, want)
    return _BATCH[(L, V)]


def run_and_check(codec, L, V, dtype, lead):
    import torch

    flat, offsets, counts, want = batch(L, V)
    total = want["total"]
    cap = total + 2
    buf = torch.empty(lead + cap * L + 8, dtype=tdtype(dtype), device="cuda:0")
    buf.view(torch.int32 if dtype == "float32" else torch.int16).fill_(SENTINEL[dtype])
    out = buf[lead:lead + cap * L].view(cap, L)
    res = codec.segment_reads(dev(flat), dev(offsets), counts, length=L, overlap=V, trim=False, dtype=tdtype(dtype),
                              out=out, **QUANTILE)
    assert int(res.total.item()) == total
    segs = res.segments.numpy()[:total]
    assert np.array_equal(np.stack([segs["read"], segs["start"], segs["valid"]], 1).astype(np.int64), want["segments"])
    host = buf.cpu().numpy().view(BITS[dtype])
    with np.errstate(over="ignore"):
        rows = want["rows32"].astype(NP_OF[dtype]).view(BITS[dtype])
    got = host[lead:lead + total * L].reshape(total, L)
    diff = np.argwhere(got != rows)
    assert not len(diff), (f"L {L} V {V} {dtype} lead {lead}: {len(diff)} of {rows.size} values differ, first at row "
                           f"{diff[0][0]} column {diff[0][1]}: got {got[tuple(diff[0])]:#x}, want {rows[tuple(diff[0])]:#x}")
    # the padding is +0.0 (all bits zero): the rows of the reads shorter than L
    short = [int(r["first_segment"]) for r, n in zip(want["reads"], counts) if 0 < n < L]
    for row, n in zip(short, [int(n) for n in counts if 0 < n < L]):
        assert (got[row, n:] == 0).all() and (rows[row, n:] == 0).all()
    assert (host[:lead] == SENTINEL[dtype]).all(), "elements in front of the output were written"
    assert (host[lead + total * L:] == SENTINEL[dtype]).all(), "rows at or above total were written"
    return want


@pytest.mark.parametrize("L,V,dtype,what", CASES, ids=[f"{L}-{V}-{dt}" for L, V, dt, _ in CASES])
def test_writer_shapes(codec, L, V, dtype, what):
    units, tpr, passes, split = launch(L, dtype)
    if what == "odd":
        assert L % 2 == 1 and units <= 4
    elif what == "partial_unit":
        assert (L % UNIT[dtype] == 0) == (dtype == "float32") and units == (3 if dtype == "float32" else 2)
    elif what == "second_pass":
        assert units > THREADS and units == 257 and split == 1 and passes == 2
    elif what == "workload":
        assert units > THREADS and (units // 1024 >= 2 and split == 2 if dtype == "float32" else split == 1)
    elif what == "odd_long":
        assert L % 2 == 1 and L % UNIT[dtype] and units > THREADS
    elif what == "split2_edge":
        assert units == 2048 and units // 1024 >= 2 and split == 2 and launch(L - UNIT[dtype], dtype)[3] == 1
    elif what == "split8":
        assert units // 1024 >= 8 and split == MAX_SPLIT
    want = run_and_check(codec, L, V, dtype, MARGIN)
    lengths = plan_lengths(L, V)
    assert 0 in lengths and L + 1 in lengths and max(r["nsegments"] for r in want["reads"]) >= 5
    if L >= 10:  # the end of the valid samples at every position of a unit
        assert {n % UNIT[dtype] for n in lengths if 0 < n < L} == set(range(UNIT[dtype]))


@pytest.mark.parametrize("dtype", ["float16", "float32"])
def test_writer_shapes_unaligned_output(codec, dtype):
    """The workload's rows into a view one element into its buffer: no row starts on a 16-byte boundary."""
    run_and_check(codec, 10000, 500, dtype, 1)
