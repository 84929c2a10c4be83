"""The chain to an unaligned BAM file on the GPU, at the shape of tests/test_gpu_quality_chain.py (the segment table,
planted rows at k = 3 and two model batches of tests/test_gpu_crf.py::test_the_chain_to_bases), one run per path:
the CRF path with qualities and moves (crf_viterbi -> stitch -> collapse_codes -> base_qual -> read_qual ->
bam_records) and the CTC path without qualities.  Two batches go through write_bam; the file passes
``gzip.decompress``, and the parser of tests/_bam_cases.py gives back the reads' bases in order, each with a move
table that sums to its length.
"""
import gzip
import uuid

import numpy as np
import pytest

import _bam_cases as K
from test_gpu_crf import CANARY, planted_rows, segment_starts

pytestmark = pytest.mark.gpu

L, V, S_, KLEN = 40, 8, 4, 3
LENGTHS, TRIMS = [100, 333, 25, 57, 0, 40, 131], [0, 3, 5, 0, 0, 2, 7]
BAD_READ, EMPTY_READ = 3, 4


def segmented_reads(codec):
    import torch

    from rawnanoporesignalcompression_amd import ReadSegments, SegmentedReads, SegmentTable

    segs, reads = [], np.zeros(len(LENGTHS), ReadSegments.DTYPE)
    for r, (m, trim) in enumerate(zip(LENGTHS, TRIMS)):
        mine = segment_starts(m, L, V)
        reads[r] = (len(segs), len(mine), trim, 6 if r == BAD_READ else 0, 0, 0, 0.0)
        segs += [(r, trim + a, valid, 0) for a, valid in mine]
    table = np.array(segs, SegmentTable.DTYPE)
    as_raw = lambda a: torch.from_numpy(a.view(np.uint8).reshape(len(a), -1).copy()).to("cuda:0")
    segmented = SegmentedReads(None, SegmentTable(as_raw(table)), ReadSegments(as_raw(reads)), None, None)
    return codec.stitch_plan(segmented, L, V, S_), len(table)


def check_file(raw, header_text, batches):
    """batches: [(ids, seq, read_bases, kept reads, codes, read_frames, qual or None)] in file order."""
    from rawnanoporesignalcompression_amd import bam

    assert raw.endswith(bam.BGZF_EOF)
    plain = gzip.decompress(raw)
    head = bam.bam_header(header_text)
    assert plain.startswith(head)
    recs = K.parse_records(plain[len(head):])
    want = [(b, r) for b in batches for r in b[3]]
    assert len(recs) == len(want)
    for rec, (b, r) in zip(recs, want):
        ids, seq, rb, _, codes, rf, qual = b
        assert rec["name"] == str(uuid.UUID(bytes=ids[r].tobytes())).encode() + b"\0"
        assert rec["seq"] == seq[rb[r]:rb[r + 1]].tobytes().decode() and set(rec["seq"]) <= set("ACGT")
        assert rec["flag"] == 4 and rec["stride"] == S_
        assert np.array_equal(rec["moves"], codes[rf[r]:rf[r + 1]] >> 7) and int(rec["moves"].sum()) == len(rec["seq"])
        if qual is None:
            assert rec["qual"] == b"\xff" * len(rec["seq"])
        else:
            assert rec["qual"] == bytes(int(q) - 33 for q in qual[rb[r]:rb[r + 1]])
    return recs


def test_the_crf_chain_to_a_bam_file(codec, tmp_path):
    import torch

    from rawnanoporesignalcompression_amd import bam, fastq, quality

    plan, R = segmented_reads(codec)
    T = L // S_
    rng = np.random.default_rng(77)
    rows = torch.from_numpy(planted_rows(rng, R, T, KLEN, 5)).to("cuda:0")
    total = int(plan.read_frames[-1].item())
    frames = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda:0")
    probs = torch.full((total, 4), -1.0, dtype=torch.float32, device="cuda:0")
    split = R // 2 + 1
    for first, n in ((0, split), (split, R - split)):
        batch = codec.crf_viterbi(rows[first:first + n], KLEN)
        post = quality.crf_posteriors(codec, rows[first:first + n], KLEN)
        codec.stitch(plan, batch.codes, first, out=frames)
        codec.stitch(plan, post, first, out=probs)
    bases = codec.collapse_codes(frames, plan.read_frames, "ACGT")
    qual = quality.base_qual(codec, bases, frames, probs, plan.read_frames)
    nreads = len(LENGTHS)
    ids = rng.integers(0, 256, (nreads, 16)).astype(np.uint8)
    dids = torch.from_numpy(ids).to("cuda:0")
    rq = fastq.read_qual(codec, bases, qual, skip_bases=10, min_mean_q=2)
    moves = (frames, plan.read_frames, S_)
    passed = bam.bam_records(codec, bases, qual, dids, {"qs": rq.mean_q}, keep=rq.passed, moves=moves)
    failed = bam.bam_records(codec, bases, qual, dids, {"qs": rq.mean_q}, keep=1 - rq.passed, moves=moves)
    path = tmp_path / "crf.bam"
    bam.write_bam(str(path), [passed, failed], header_text="@HD\tVN:1.6\tSO:unknown\n@CO\tcrf\n")

    seq, q = bases.seq.cpu().numpy(), qual.cpu().numpy()
    rb, status, ok = bases.read_bases.cpu().numpy(), bases.status.cpu().numpy(), rq.passed.cpu().numpy()
    codes, rf = frames.cpu().numpy(), plan.read_frames.cpu().numpy()
    has = [r for r in range(nreads) if status[r] == 0 and rb[r + 1] > rb[r]]
    kept, rest = [r for r in has if ok[r]], [r for r in has if not ok[r]]
    assert BAD_READ not in has and EMPTY_READ not in has and len(kept) >= 4
    recs = check_file(path.read_bytes(), "@HD\tVN:1.6\tSO:unknown\n@CO\tcrf\n",
                      [(ids, seq, rb, kept, codes, rf, q), (ids, seq, rb, rest, codes, rf, q)])
    mean_q = rq.mean_q.cpu().numpy()
    assert [rec["tags"] for rec in recs] == [[("qs", int(mean_q[r]))] for r in kept + rest]
    for rec_batch, mask in ((passed, ok), (failed, 1 - ok)):
        want = bam.bam_records_signal(ids, seq, q, rb, status, {"qs": mean_q.view(np.uint32)}, keep=mask,
                                      moves=(codes, rf, S_), bgzf=True, byte_capacity=int(rec_batch.data.numel()))
        assert rec_batch.tobytes() == bam.bgzf_blocks_signal(want[0])
        assert np.array_equal(rec_batch.status.cpu().numpy(), want[2])


def test_the_ctc_chain_to_a_bam_file(codec, tmp_path):
    import torch

    from rawnanoporesignalcompression_amd import bam

    plan, R = segmented_reads(codec)
    T = L // S_
    rng = np.random.default_rng(78)
    scores = torch.from_numpy(rng.standard_normal((R, T, 5)).astype(np.float16)).to("cuda:0")
    total = int(plan.read_frames[-1].item())
    frames = torch.zeros((total, 5), dtype=torch.float16, device="cuda:0")
    split = R // 2 + 1
    for first, n in ((0, split), (split, R - split)):
        codec.stitch(plan, scores[first:first + n], first, out=frames)
    bases = codec.ctc_decode(frames, plan.read_frames, codes=True)
    nreads = len(LENGTHS)
    ids = rng.integers(0, 256, (nreads, 16)).astype(np.uint8)
    dids = torch.from_numpy(ids).to("cuda:0")
    half = torch.tensor([1, 0, 1, 1, 1, 0, 1], dtype=torch.uint8, device="cuda:0")
    moves = (bases.codes, plan.read_frames, S_)
    first_half = bam.bam_records(codec, bases, None, dids, keep=half, moves=moves)
    second_half = bam.bam_records(codec, bases, None, dids, keep=1 - half, moves=moves)
    buf_path = tmp_path / "ctc.bam"
    with open(buf_path, "wb") as f:
        bam.write_bam(f, [first_half, second_half])

    seq, rb, status = bases.seq.cpu().numpy(), bases.read_bases.cpu().numpy(), bases.status.cpu().numpy()
    codes, rf, mask = bases.codes.cpu().numpy(), plan.read_frames.cpu().numpy(), half.cpu().numpy()
    has = [r for r in range(nreads) if status[r] == 0 and rb[r + 1] > rb[r]]
    assert BAD_READ not in has and EMPTY_READ not in has and len(has) == 5
    a, b = [r for r in has if mask[r]], [r for r in has if not mask[r]]
    check_file(buf_path.read_bytes(), None, [(ids, seq, rb, a, codes, rf, None), (ids, seq, rb, b, codes, rf, None)])
