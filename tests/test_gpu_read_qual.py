"""Per-read mean quality on the GPU (pgn_read_qual_device through fastq.read_qual), bit for bit against
read_qual_signal on the cases of tests/_fastq_cases.py: mean_q, err_sum and passed of every read, for reads around
skip_bases, error sums that equal a threshold times the count and their neighbours, the quality bytes outside
'!'..'~', a read of several tiles among one-base reads with boundaries at a tile's first and last base, min_mean_q
at, below and above a read's mean, reads with a status and reads the capacity cuts.
"""
import ctypes as C

import numpy as np
import pytest

import _fastq_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return {c.name: (c, c.expected()) for c in K.qual_cases()}


def device_arrays(c):
    import torch

    from rawnanoporesignalcompression_amd import DecodedReads

    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    qual = up(c.qual)
    return DecodedReads(torch.empty_like(qual), up(c.read_bases), up(c.status), None, None, None, None), qual


def compare(rq, want, name):
    mq, U, ps = want
    assert np.array_equal(rq.mean_q.cpu().numpy().view(np.uint32), mq), name
    assert np.array_equal(rq.err_sum.cpu().numpy().view(np.uint64), U), name
    assert np.array_equal(rq.passed.cpu().numpy(), ps), name


@pytest.mark.parametrize("name", [c.name for c in K.qual_cases()])
def test_read_qual(codec, cases, name):
    from rawnanoporesignalcompression_amd import fastq

    c, want = cases[name]
    decoded, qual = device_arrays(c)
    rq = fastq.read_qual(codec, decoded, qual, c.thresholds, q_min=c.q_min, skip_bases=c.skip_bases,
                         min_mean_q=c.min_mean_q)
    compare(rq, want, name)


def test_the_case_list_covers_the_issue():
    assert [c.name for c in K.qual_cases()] == ["skip", "skip0", "edge", "bytes", "tiles", "gate", "status-cut"]


def test_unaligned_qual_and_a_callers_stream(codec, cases):
    """qual as a view 5 bytes into a buffer takes the byte loads; the same numbers on a caller's stream."""
    import torch

    from rawnanoporesignalcompression_amd import DecodedReads, fastq

    c, want = cases["tiles"]
    decoded, qual = device_arrays(c)
    buf = torch.empty(int(qual.numel()) + 5, dtype=torch.uint8, device="cuda:0")
    view = buf[5:]
    view.copy_(qual)
    assert view.data_ptr() % 16 == 5 and view.is_contiguous()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    rq = fastq.read_qual(codec, DecodedReads(view, decoded.read_bases, decoded.status, None, None, None, None), view,
                         stream=s.cuda_stream)
    compare(rq, want, "tiles, unaligned")


def test_without_err_sum_and_empty_call(codec, cases):
    """The C call with a NULL d_err_sum sums in the context's scratch; nreads == 0 touches nothing."""
    import torch

    from rawnanoporesignalcompression_amd.host import read_qual_params

    c, (mq, U, ps) = cases["status-cut"]
    decoded, qual = device_arrays(c)
    n = len(c.status)
    prm = read_qual_params(None, c.q_min, c.skip_bases, c.min_mean_q)
    mean_q = torch.full((n + 1,), -7, dtype=torch.int32, device="cuda:0")
    passed = torch.full((n + 1,), 9, dtype=torch.uint8, device="cuda:0")
    fn = codec._lib.pgn_read_qual_device
    torch.cuda.synchronize()                                  # the fills above run on torch's stream
    for _ in range(2):                                        # the scratch is zeroed by every call
        assert fn(codec._h, C.byref(prm), n, decoded.read_bases.data_ptr(), decoded.status.data_ptr(), qual.data_ptr(),
                  len(c.qual), mean_q.data_ptr(), None, passed.data_ptr(), None) == 0
        torch.cuda.synchronize()
        assert np.array_equal(mean_q.cpu().numpy()[:n].view(np.uint32), mq) and int(mean_q[n]) == -7
        assert np.array_equal(passed.cpu().numpy()[:n], ps) and int(passed[n]) == 9
    assert fn(codec._h, C.byref(prm), 0, None, None, qual.data_ptr(), len(c.qual), None, None, None, None) == 0
    torch.cuda.synchronize()
    assert int(mean_q[0]) == int(mq[0])
