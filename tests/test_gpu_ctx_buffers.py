"""The context's scratch buffers under growth (csrc/pgn_kernels.hip: reserve, CallScope).  Each test has a
fresh context, so every buffer starts empty, grows from call to call while the previous call may still be on
the device, and is then reused by a smaller call.  All inputs are valid data; the results are held to the
CPU oracle and to the NumPy references of the stages' own API tests, bit for bit.

No test here makes a call that is refused after its launch sequence has opened: every refusal of the C ABI
is an argument check that returns before the context is touched, and the only later ones are failed
allocations, which a test must not provoke.
"""
import numpy as np
import pytest

import _oracle as O
from test_ctc_api import ref_decode
from test_decode_pa_api import ref_pa
from test_gpu_segments import check as check_segments
from test_norm_api import MEDMAD, QUANTILE, assert_stats_equal, ref_norm, ref_stats
from test_segment_api import USUAL, ref_batch
from test_stitch_api import ref_plan

pytestmark = pytest.mark.gpu

BATCHES = [1, 16, 300, 16]  # chunks per call: 300 is above the 64-chunk cooperative limit


def dev(a):
    import torch

    return torch.from_numpy(np.array(a, order="C")).to(torch.device("cuda", 0))


def starts(counts):
    return np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)


@pytest.mark.parametrize("vbz", [False, True], ids=["C5", "VBZ"])
def test_growth_with_work_in_flight(vbz):
    """Encode and decode batches of 1, 16, 300 and 16 chunks of 1 to 6,000 samples through the C ABI, the calls
    alternating between two streams with no host synchronisation: each call needs more slots, per-chunk
    buffers and counters than the one before, whose kernels may still run on the other stream, and the last
    call runs in the buffers the largest left.  A decode reads the blobs and sizes its encode wrote on the
    other stream, so only the context orders them."""
    import torch

    from rawnanoporesignalcompression_amd import PGNanoCodec, VBZCodec

    codec = VBZCodec(0) if vbz else PGNanoCodec(0)
    try:
        lib, h = codec._lib, codec._h
        enc_fn = lib.pgn_vbz_compress_batch_device if vbz else lib.pgn_compress_batch_device
        dec_fn = lib.pgn_vbz_decompress_batch_device if vbz else lib.pgn_decompress_batch_device
        max_size = lib.pgn_vbz_compressed_signal_max_size if vbz else lib.pgn_compressed_signal_max_size
        rng = np.random.default_rng(17)
        calls = []
        for b, k in enumerate(BATCHES):
            counts = rng.integers(1, 6001, k)
            counts[0], counts[-1] = (1, 6000) if k > 1 else (4097, 4097)
            reads = [O.synth_read(1000 * b + r, int(n)) for r, n in enumerate(counts)]
            caps = np.array([int(max_size(int(n))) for n in counts], np.int64)
            t = dict(reads=reads, samples=dev(np.concatenate(reads)), offs=dev(starts(counts)),
                     cnt=dev(counts.astype(np.int32)), caps=dev(caps), bo=dev(starts(caps)),
                     blobs=torch.zeros(int(caps.sum()), dtype=torch.uint8, device="cuda:0"),
                     sizes=torch.zeros(k, dtype=torch.int64, device="cuda:0"),
                     est=torch.full((k,), -1, dtype=torch.int32, device="cuda:0"),
                     dec=torch.zeros(int(counts.sum()), dtype=torch.int16, device="cuda:0"),
                     dst=torch.full((k,), -1, dtype=torch.int32, device="cuda:0"))
            calls.append(t)
        torch.cuda.synchronize()
        sa, sb = torch.cuda.Stream("cuda:0"), torch.cuda.Stream("cuda:0")
        for b, t in enumerate(calls):
            k = len(t["reads"])
            s_enc, s_dec = (sa, sb) if b % 2 == 0 else (sb, sa)
            assert enc_fn(h, k, t["samples"].data_ptr(), t["offs"].data_ptr(), t["cnt"].data_ptr(), t["blobs"].data_ptr(),
                          t["bo"].data_ptr(), t["caps"].data_ptr(), t["sizes"].data_ptr(), t["est"].data_ptr(), None,
                          s_enc.cuda_stream) == 0
            assert dec_fn(h, k, t["blobs"].data_ptr(), t["bo"].data_ptr(), t["sizes"].data_ptr(), t["dec"].data_ptr(),
                          t["offs"].data_ptr(), t["cnt"].data_ptr(), t["dst"].data_ptr(), s_dec.cuda_stream) == 0
        torch.cuda.synchronize()
        for b, t in enumerate(calls):
            assert (t["est"] == 0).all() and (t["dst"] == 0).all(), b
            assert np.array_equal(t["dec"].cpu().numpy(), np.concatenate(t["reads"])), b
            blobs, bo, bs = t["blobs"].cpu().numpy(), t["bo"].cpu().numpy(), t["sizes"].cpu().numpy()
            for r, x in enumerate(t["reads"]):
                want = O.vbz_compress(x) if vbz else O.c5_compress(x)[1]
                assert blobs[bo[r]:bo[r] + bs[r]].tobytes() == want, (b, r)
    finally:
        codec.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint16)


def run_read_stages(codec, nreads, seed):
    """Every read stage once on `nreads` reads of 1,500 to 4,500 samples, each result against its reference."""
    import torch

    rng = np.random.default_rng(seed)
    reads = [O.synth_read(seed + r, int(n)) for r, n in enumerate(rng.integers(1500, 4501, nreads))]
    n = np.array([x.size for x in reads], np.int64)
    flat, offs = dev(np.concatenate(reads)), starts(n)
    what = f"{nreads} reads"

    st = codec.read_stats(flat, dev(offs), dev(n), **QUANTILE).numpy()
    for r, x in enumerate(reads):
        assert_stats_equal(st[r], ref_stats(x, **QUANTILE), f"read_stats, {what}: read {r}")

    # the reads as chunks of up to 1,024 samples, encoded by the context itself
    chunks = [[min(1024, x.size - a) for a in range(0, x.size, 1024)] for x in reads]
    counts = np.array([c for cs in chunks for c in cs], np.int32)
    first = np.concatenate([[0], np.cumsum([len(cs) for cs in chunks])]).astype(np.int64)
    enc = codec.compress_batch(flat, dev(starts(counts)), dev(counts))
    out, ro, nst, cst = codec.decompress_reads_norm(enc.blobs, enc.offsets, enc.sizes, dev(counts), dev(first),
                                                    dtype=torch.float32, **MEDMAD)
    got, ro, nst = out.cpu().numpy(), ro.cpu().numpy(), nst.numpy()
    assert (enc.status.cpu().numpy() == 0).all() and (cst.cpu().numpy() == 0).all(), what
    for r, x in enumerate(reads):
        w = ref_stats(x, **MEDMAD)
        assert_stats_equal(nst[r], w, f"reads_norm, {what}: read {r}")
        assert np.array_equal(bits(got[ro[r]:ro[r] + x.size]), bits(ref_norm(x, w["centre"], w["spread"]))), (what, r)

    cal_off = rng.integers(-20, 20, nreads).astype(np.float32)
    cal_scale = (0.1 + rng.random(nreads)).astype(np.float32)
    out, ro, rst, cst = codec.decompress_reads_pa(enc.blobs, enc.offsets, enc.sizes, dev(counts), dev(first), dev(cal_off),
                                                  dev(cal_scale), dtype=torch.float32)
    got, ro = out.cpu().numpy(), ro.cpu().numpy()
    assert (rst.cpu().numpy() == 0).all() and (cst.cpu().numpy() == 0).all(), what
    for r, x in enumerate(reads):
        assert np.array_equal(bits(got[ro[r]:ro[r] + x.size]), bits(ref_pa(x, cal_off[r], cal_scale[r]))), (what, r)

    L, V, s = 64, 16, 8
    seg = codec.segment_reads(flat, dev(offs), dev(n), length=L, overlap=V, trim=True, dtype=torch.float32, **MEDMAD)
    want = ref_batch(reads, L, V, USUAL, MEDMAD)
    check_segments(seg, want, "float32", int(seg.out.shape[0]), f"segment_reads, {what}")

    # the plan of every row by the header's rule, and the frames the rows call must copy
    plan = codec.stitch_plan(seg, L, V, s)
    T, total = L // s, want["total"]
    rows = torch.from_numpy(rng.integers(-3, 4, (total, T, 5)).astype(np.float16)).to("cuda:0")
    host_rows, table = rows.cpu().numpy(), plan.segments.numpy()[:total]
    frames, read_frames = [np.zeros((0, 5), np.float16)], [0]
    for rec in want["reads"]:
        a, k = rec["first_segment"], rec["nsegments"]
        pos = read_frames[-1]
        for j, (f, c) in enumerate(ref_plan([(int(st_), int(v)) for _, st_, v in want["segments"][a:a + k]], L, s) if k else []):
            g = table[a + j]
            assert (int(g["first"]), int(g["count"]), int(g["dst_frame"])) == (f, c, pos), (what, a + j)
            frames.append(host_rows[a + j, f:f + c])
            pos += c
        read_frames.append(pos)
    assert plan.read_frames.cpu().tolist() == read_frames, what
    stitched = codec.stitch(plan, rows)
    scores = np.concatenate(frames)
    assert np.array_equal(bits(stitched.cpu().numpy()), bits(scores)), what

    dec = codec.ctc_decode(stitched, plan.read_frames, alphabet="NACGT", blank=0, codes=True)
    seqs, rb = dec.sequences(), dec.read_bases.cpu().numpy()
    at, sc, cd = dec.base_frame.cpu().numpy(), dec.base_score.cpu().numpy(), dec.codes.cpu().numpy()
    assert (dec.status.cpu().numpy() == 0).all(), what
    for r in range(nreads):
        a, b = read_frames[r], read_frames[r + 1]
        wseq, wat, wsc, wcd = ref_decode(scores[a:b], b"NACGT", 0)
        assert seqs[r] == wseq and at[rb[r]:rb[r + 1]].tolist() == wat and cd[a:b].tolist() == wcd, (what, r)
        assert np.array_equal(bits(sc[rb[r]:rb[r + 1]]), bits(np.array(wsc, np.float32))), (what, r)


def test_read_stages_regrow():
    """read_stats, decompress_reads_norm, decompress_reads_pa, segment_reads, stitch_plan + stitch and ctc_decode
    on one context with 2 reads and then with 40: the second round regrows every per-read, per-chunk, per-row
    and per-tile block the first one allocated, behind the first round's kernels."""
    from rawnanoporesignalcompression_amd import PGNanoCodec

    codec = PGNanoCodec(0)
    try:
        run_read_stages(codec, 2, 7000)
        run_read_stages(codec, 40, 8000)
    finally:
        codec.close()
