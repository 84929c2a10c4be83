"""The chain to FASTQ on the GPU: rows -> crf_viterbi and crf_posteriors -> the stitch of the code bytes and the
stitch of the 16-byte probability frames -> collapse_codes -> base_qual, in the shape of
tests/test_gpu_crf.py::test_the_chain_to_bases (its segment table, its planted rows at k = 3, two model batches).

The quality string is bit for bit base_qual_signal of the device's own stitched probabilities.  Against the string
made from the float64 model's probabilities it may differ only where the float64 mean error of a base lies within
a relative 1e-4 of a threshold, and there by one: the device's probabilities carry float32's error, a few 1e-6
relative, which moves a base across a threshold only if it stood next to it.
"""
import numpy as np
import pytest

from test_gpu_crf import CANARY, planted_rows, reference, segment_starts

pytestmark = pytest.mark.gpu


def test_the_chain_to_qualities(codec):
    import torch

    from rawnanoporesignalcompression_amd import (ReadSegments, SegmentedReads, SegmentTable, collapse_codes_signal,
                                                  quality, stitch_plan_signal)

    L, V, s, k = 40, 8, 4, 3
    T = L // s
    lengths, trims = [100, 333, 25, 57, 0, 40, 131], [0, 3, 5, 0, 0, 2, 7]
    bad_read = 3
    segs, reads = [], np.zeros(len(lengths), ReadSegments.DTYPE)
    for r, (m, trim) in enumerate(zip(lengths, trims)):
        mine = segment_starts(m, L, V)
        reads[r] = (len(segs), len(mine), trim, 6 if r == bad_read else 0, 0, 0, 0.0)
        segs += [(r, trim + a, valid, 0) for a, valid in mine]
    table = np.array(segs, SegmentTable.DTYPE)
    R = len(table)
    as_raw = lambda a: torch.from_numpy(a.view(np.uint8).reshape(len(a), -1).copy()).to("cuda:0")
    segmented = SegmentedReads(None, SegmentTable(as_raw(table)), ReadSegments(as_raw(reads)), None, None)
    plan = codec.stitch_plan(segmented, L, V, s)

    rng = np.random.default_rng(77)
    host = planted_rows(rng, R, T, k, 5)
    rows = torch.from_numpy(host).to("cuda:0")
    total = int(plan.read_frames[-1].item())
    frames = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda:0")
    probs = torch.full((total, 4), -1.0, dtype=torch.float32, device="cuda:0")
    split = R // 2 + 1
    for first, n in ((0, split), (split, R - split)):
        batch = codec.crf_viterbi(rows[first:first + n], k)
        post = quality.crf_posteriors(codec, rows[first:first + n], k)
        codec.stitch(plan, batch.codes, first, out=frames)
        codec.stitch(plan, post, first, out=probs)
    bases = codec.collapse_codes(frames, plan.read_frames, "ACGT")
    thr = quality.qual_thresholds()
    qual = quality.base_qual(codec, bases, frames, probs, plan.read_frames)

    # the same chain on the host: the codes bit for bit, the probabilities of the float64 model
    codes = np.stack([reference(host[g:g + 1], k, 5, 0.0)[0][0] for g in range(R)])
    p64 = np.stack([quality.crf_posteriors_signal(host[g], k) for g in range(R)])
    got_frames, got_probs = frames.cpu().numpy(), probs.cpu().numpy()
    got_qual, read_frames = qual.cpu().numpy(), plan.read_frames.cpu().numpy()
    read_bases = bases.read_bases.cpu().numpy()
    assert (got_probs >= 0).all() and np.abs(got_probs.sum(1) - 1).max() <= 1e-5   # every frame of the plan was written
    near = differ = nbases = 0
    for r in range(len(lengths)):
        first, n = int(reads["first_segment"][r]), int(reads["nsegments"][r])
        mine, mine64 = np.zeros(0, np.uint8), np.zeros((0, 4))
        if reads["status"][r] == 0 and n:
            fc = stitch_plan_signal(np.stack([table["start"][first:first + n], table["valid"][first:first + n]], 1), L, V, s)
            mine = np.concatenate([codes[first + j, a:a + c] for j, (a, c) in enumerate(fc)])
            mine64 = np.concatenate([p64[first + j, a:a + c] for j, (a, c) in enumerate(fc)])
        f0, f1 = int(read_frames[r]), int(read_frames[r + 1])
        assert f1 - f0 == len(mine) and np.array_equal(got_frames[f0:f1], mine)
        _, at = collapse_codes_signal(mine, "ACGT")
        b0, b1 = int(read_bases[r]), int(read_bases[r + 1])
        assert b1 - b0 == len(at)
        # bit for bit the rule applied to the device's own stitched probabilities
        want = quality.base_qual_signal(mine, got_probs[f0:f1], at, len(mine), thr, 1)
        assert np.array_equal(got_qual[b0:b1], want), r
        # and the float64 model's string, except next to a threshold
        ends = np.append(at[1:], len(mine)).astype(np.int64)
        for g, (t0, t1) in enumerate(zip(at.astype(np.int64), ends)):
            c = int(mine[t0]) & 3
            err = mine64[t0:t1, (c + 1) & 3] + mine64[t0:t1, (c + 2) & 3] + mine64[t0:t1, (c + 3) & 3]
            mean = float(np.trunc(np.clip(err, 0, 1) * 2.0 ** 32).sum()) / (t1 - t0)
            q64 = 33 + 1 + int((mean <= thr.astype(np.float64)).sum())
            close = bool((np.abs(mean - thr.astype(np.float64)) <= 1e-4 * thr).any())
            nbases += 1
            near += close
            if got_qual[b0 + g] != q64:
                differ += 1
                assert close and abs(int(got_qual[b0 + g]) - q64) == 1, (r, g, int(got_qual[b0 + g]), q64, mean)
    print(f"chain: {nbases} bases, {near} within 1e-4 of a threshold, {differ} differ from the float64 string")
    assert nbases > 50 and read_bases[bad_read] == read_bases[bad_read + 1]
    assert len(set(got_qual[:nbases].tolist())) > 2
    assert (bases.status.cpu().numpy() == 0).all()
