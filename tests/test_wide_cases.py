"""The designs of the wide-stream tests (tests/_wide_cases.py, run by tests/test_gpu_wide_streams.py), without a GPU:
what makes a stream pass 2^32 where the tests say it does, the closed forms against the host models on short
prefixes, and the memory each test takes.
"""
import zlib

import numpy as np

import _bam_cases
import _wide_cases as Wd
from rawnanoporesignalcompression_amd.host import bgzf_deflate_signal

B, WIDE = Wd.B, Wd.WIDE


def test_deflate_period_and_counts():
    d = Wd.deflate()
    assert len(d.period) == 3 * B and len(d.tail) == Wd.TAIL
    blocks = _bam_cases.parse_bgzf(d.first)
    assert [size for _, size, _, _, _ in blocks] == list(d.sizes) and len(d.first) == d.S
    ratios = [(size - 26) / B for size in d.sizes]
    print(f"deflate: S = {d.S}, reps = {d.reps}, source {d.src_bytes} bytes, file {d.total} bytes, ratios "
          + " ".join(f"{r:.3f}" for r in ratios))
    assert 0.45 < ratios[0] < 0.55 and blocks[0][2][0] & 7 == 5, "dynamic at about 0.5"
    assert d.sizes[1] == Wd.FILE and blocks[1][2][0] == 1, "stored"
    assert 0.95 <= ratios[2] < 1 and blocks[2][2][0] & 7 == 5, "dynamic at 0.95 or more"
    assert d.S % 2 == 1, "an odd period: the blocks walk through every alignment"
    off = d.blk_off()
    assert {int(v) % 16 for v in off[:3 * 16 + 3]} == set(range(16))
    assert {(Wd.OUT_OFFSET + int(v)) % 16 for v in off[0:3 * 16:3]} == set(range(16)), "each kind of block at every alignment"
    assert d.reps * d.S >= WIDE + 3 * d.S and (d.reps - 1) * d.S < WIDE + 3 * d.S
    assert d.reps * 3 * B > WIDE and d.S < 3 * B, "the source passes 2^32 before the file does"
    assert d.memory() <= Wd.MEMORY_CAP and off.nbytes <= Wd.DOWNLOAD_CAP
    assert all(b - a <= Wd.CHUNK_BYTES // d.S for a, b in Wd.row_chunks(d.reps, d.S))


def test_deflate_closed_forms_follow_the_model():
    d = Wd.deflate()
    off = d.blk_off()
    assert off.dtype == np.uint64 and len(off) == d.ntiles + 1 and int(off[-1]) == d.total and int(off[-2]) == d.reps * d.S
    assert (np.diff(off.astype(np.int64)) > 26).all()
    # two periods and the tail through the model
    data, moff, written = bgzf_deflate_signal(d.period * 2 + d.tail)
    assert data == d.first * 2 + d.tail_file
    assert np.array_equal(moff[:7], off[:7]) and int(moff[7]) - int(moff[6]) == len(d.tail_file)
    for k in (0, 1, 2, 3, 7, 3 * d.reps - 1):
        blk = d.block_file(k)
        assert len(blk) == int(off[k + 1] - off[k])
        (_, _, body, crc, isize), = _bam_cases.parse_bgzf(blk)
        assert zlib.decompressobj(-15).decompress(body) == d.block_payload(k) and crc == zlib.crc32(d.block_payload(k)) and isize == B
    # the blocks the GPU test downloads
    j = d.block_of_file_byte(WIDE)
    assert int(off[j]) <= WIDE < int(off[j + 1]) and j < 3 * d.reps
    k = WIDE // B
    assert k * B <= WIDE < (k + 1) * B and k < j, "the source's block at 2^32 lies in front of the file's"
    assert int(off[k + 1]) < WIDE
    # the capacity call: the first offset past 2^32
    j = d.first_block_past(WIDE)
    assert int(off[j]) > WIDE >= int(off[j - 1]) and 3 * d.reps - j >= 6, "whole blocks stay unwritten behind the capacity"


def test_deflate_cut_calls():
    d = Wd.deflate()
    assert (WIDE + 1) % B == 257 and Wd.NBYTES_PAST % B == 257, "2^32 + 65,280 + 1 bytes end with a block of 257 bytes"
    assert Wd.NBYTES_ONE % B == 1 and WIDE < Wd.NBYTES_ONE < Wd.NBYTES_PAST + B
    for nbytes, n in ((Wd.NBYTES_PAST, 257), (Wd.NBYTES_ONE, 1)):
        off, written, last, got_n, blk = d.cut(nbytes)
        assert got_n == n and last == nbytes // B and last * B + n == nbytes > WIDE
        assert int(written[0]) == nbytes and int(written[1]) == int(off[last + 1]) == int(off[last]) + len(blk)
        assert (off[last + 1:] == off[last + 1]).all() and len(off) == d.ntiles + 1 and d.ntiles - last > 3
        assert np.array_equal(off[:last + 1], d.blk_off()[:last + 1])
        (_, size, body, crc, isize), = _bam_cases.parse_bgzf(blk)
        assert isize == n and zlib.decompressobj(-15).decompress(body) == d.block_payload(last, n)
    # on a short prefix the same closed form is the model's
    short = 4 * B + 257
    data, moff, written = bgzf_deflate_signal((d.period * 2)[:short])
    assert int(written[0]) == short and len(data) == int(moff[-1]) == int(d.blk_off()[4]) + len(bgzf_deflate_signal(d.block_payload(4, 257))[0])


def test_bam_reads():
    for r, what in ((Wd.bam_frames(), "frames"), (Wd.bam_bases(), "bases")):
        assert r.R == Wd.BAM_R == _bam_cases.record_length(r.m, 1, r.F) and r.F > 0
        assert r.R % 512 == 0 and (2 * B) % r.R == 0 and B % r.R != 0 and Wd.BAM_PAIR == 17
        assert r.n % Wd.BAM_PAIR == 0 and r.stream_bytes >= WIDE + 3 * B and r.stream_bytes - 2 * B < WIDE + 3 * B
        assert r.m % 2 == 1, "a last half byte of packed bases in every record"
        passes = {"frames": r.n * r.F, "bases": r.n * r.m}[what]
        assert passes > 1 << 31, what
        assert max(r.n * r.m, r.n * r.F) < WIDE, "no input buffer passes 2^32: one that did, with the output, would not fit the cap"
        out = max(r.stream_bytes, Wd.bgzf_bound(r.stream_bytes))
        print(f"bam {what}: m = {r.m}, F = {r.F}, {r.n} reads, stream {r.stream_bytes}, memory {Wd.records_memory(r, out) / Wd.GIB:.2f} GiB")
        assert Wd.records_memory(r, out) <= Wd.MEMORY_CAP
        stream, off, st, written = Wd.bam_model(r, 2 * Wd.BAM_PAIR)
        assert len(stream) == 4 * B and np.array_equal(off, np.arange(2 * Wd.BAM_PAIR + 1, dtype=np.uint64) * np.uint64(r.R))
        assert stream[:2 * B] == stream[2 * B:] and stream[:r.R] == stream[r.R:2 * r.R] and not st.any()
        rec = _bam_cases.parse_records(stream[:r.R])[0]
        assert len(rec["seq"]) == r.m and len(rec["moves"]) == r.F and rec["tags"] == [Wd.TAG]
        data, written = Wd.bam_file(r, Wd.BAM_PAIR)
        assert len(data) == 2 * Wd.FILE == int(written[1]) and int(written[0]) == 2 * B
        cap, first = Wd.bam_cut(r)
        assert (first - 1) * r.R < WIDE < first * r.R < cap < (first + 1) * r.R <= r.stream_bytes - r.R
    # the cut on a short prefix through the model
    r = Wd.bam_frames()
    _, off, st, written = Wd.bam_model(r, 6, byte_capacity=3 * r.R + r.R // 2)
    assert st.tolist() == [0, 0, 0, Wd.SMALL, Wd.SMALL, Wd.SMALL] and written.tolist() == [3 * r.R, 3 * r.R] and int(off[-1]) == 6 * r.R


def test_fastq_reads():
    r = Wd.fastq()
    assert r.R == 42 + 8 + 2 * r.m and r.stream_bytes >= WIDE + 3 * Wd.T > r.stream_bytes - r.R
    assert r.R % 16 != 0 and r.R % 2 == 0 and r.m % 16 != 0, "records and their sources at changing alignments"
    assert Wd.records_memory(r, r.stream_bytes) <= Wd.MEMORY_CAP and (r.n + 1) * 8 <= Wd.DOWNLOAD_CAP
    assert r.n * 2 * r.m < WIDE, "the input side stays below 2^32: with the output it would not fit the cap"
    print(f"fastq: m = {r.m}, {r.n} reads, text {r.stream_bytes}, memory {Wd.records_memory(r, r.stream_bytes) / Wd.GIB:.2f} GiB")
    for reverse in (False, True):
        text, off, st = Wd.fastq_model(r, 3, reverse)
        assert len(text) == 3 * r.R and text[:r.R] == text[r.R:2 * r.R] and off.tolist() == [0, r.R, 2 * r.R, 3 * r.R]
        assert text.startswith(b"@") and b"\tqs:i:12\n" in text[:60] and not st.any()
    assert Wd.fastq_model(r, 1, True)[0] != Wd.fastq_model(r, 1)[0]
    cap, at = Wd.fastq_cut(r)
    assert at * r.R <= WIDE < (at + 1) * r.R == cap + 1 and at < r.n - 3
    _, off, st = Wd.fastq_model(r, 5, byte_capacity=3 * r.R - 1)
    assert st.tolist() == [0, 0, Wd.SMALL, Wd.SMALL, Wd.SMALL] and int(off[-1]) == 5 * r.R


def test_row_chunks():
    for rows, row in ((1, 10), (1000, 130622), (26815, 160177), (5, Wd.CHUNK_BYTES)):
        ch = Wd.row_chunks(rows, row)
        assert ch[0][0] == 0 and ch[-1][1] == rows and all(a[1] == b[0] for a, b in zip(ch, ch[1:]))
        assert all((b - a) * row <= max(Wd.CHUNK_BYTES, row) for a, b in ch)
