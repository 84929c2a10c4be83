"""Streams whose byte offsets pass 2^32 through the three calls that end every route: pgn_bgzf_deflate_device,
pgn_bam_records_device and pgn_fastq_records_device (the header states limits of 2^32 reads and 2^40 frames, so
such streams are in contract).  An offset kept in 32 bits anywhere (a tile index times a tile's bytes, a scan's
carry, a capacity comparison) writes a period of these streams over an earlier one or leaves it unwritten.

Each input is periodic and built on the device, so the output is periodic: one period is held to the host model, bit
for bit, every other period to the first on the device through a ``[periods, bytes]`` view, in chunks of 256 MiB.
``blk_off`` and ``rec_off`` are held to closed forms, and the blocks and records that contain byte 2^32 come down and
are parsed on the host.  tests/_wide_cases.py holds the arithmetic and tests/test_wide_cases.py its conditions.

The output side passes 2^32.  The writers' input side does not: bases, qualities and frame codes each stay below
2^32 bytes, since an input buffer above 4 GiB beside an output above 4 GiB and the other inputs would not fit the
12 GiB a test here may take.  ``read_bases`` passes 2^31 in the BGZF test's shape and the frame offsets in the raw
test's; the deflate call's source passes 2^32 itself.
"""
import zlib

import numpy as np
import pytest

import _bam_cases
import _wide_cases as Wd

pytestmark = pytest.mark.gpu

SENTINEL, FRONT, BACK = 0xA5, 64, 80
B, WIDE = Wd.B, Wd.WIDE
DEV = "cuda:0"


class Scope:
    """The body of one test: skipped only where the device has too little free memory, and its peak held to the
    cap (less 256 MiB for the calls' own scratch, which the allocator here does not see)."""

    def __enter__(self):
        import torch

        torch.cuda.empty_cache()
        free, _ = torch.cuda.mem_get_info()
        if free < Wd.MEMORY_NEEDED:
            pytest.skip(f"{free >> 30} GiB of device memory free, 16 GiB needed")
        torch.cuda.reset_peak_memory_stats()
        return self

    def __exit__(self, *exc):
        import torch

        peak = torch.cuda.max_memory_allocated()
        if exc[0] is None:
            print(f"peak device memory {peak / Wd.GIB:.2f} GiB")
            assert peak <= Wd.MEMORY_CAP - (256 << 20), f"peak device memory {peak}"
        return False


def scoped(body, *args):
    """The body in a frame of its own, so that its buffers are gone when the cache is emptied, whatever happened."""
    import gc

    import torch

    try:
        body(*args)
    finally:
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def up(a):
    import torch

    return torch.from_numpy(np.array(a)).to(DEV)            # a copy: the models' bytes are read-only


def down(t):
    assert t.numel() * t.element_size() <= Wd.DOWNLOAD_CAP
    return t.cpu().numpy()


def repeated(one, n):
    """``one`` n times end to end, on the device."""
    import torch

    out = torch.empty(n * len(one), dtype=torch.uint8, device=DEV)
    out.view(n, len(one)).copy_(up(one).unsqueeze(0).expand(n, len(one)))
    return out


def rows_equal_first(flat, rows, row_bytes):
    """Whether every row of the ``[rows, row_bytes]`` view of ``flat`` equals the first: one answer, on the device."""
    import torch

    view = flat[:rows * row_bytes].view(rows, row_bytes)
    ok = torch.ones((), dtype=torch.bool, device=DEV)
    for a, b in Wd.row_chunks(rows, row_bytes):
        ok &= (view[a:b] == view[0]).all()
    return bool(ok.item())


def all_sentinel(t):
    import torch

    ok = torch.ones((), dtype=torch.bool, device=DEV)
    step = Wd.CHUNK_BYTES
    for a in range(0, int(t.numel()), step):
        ok &= (t[a:a + step] == SENTINEL).all()
    return bool(ok.item())


def sentinel_buffer(out_offset, nbytes):
    import torch

    buf = torch.full((FRONT + out_offset + nbytes + BACK,), SENTINEL, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    return buf, FRONT + out_offset


def offsets(n, step):
    import torch

    return torch.arange(n + 1, dtype=torch.int64, device=DEV) * step


# ---- deflate ---------------------------------------------------------------------------------------------------------
def check_block(blk, payload):
    """One BGZF block from the device against its payload: inflated by zlib, with CRC and ISIZE."""
    (_, size, body, crc, isize), = _bam_cases.parse_bgzf(blk)
    z = zlib.decompressobj(-15)
    assert z.decompress(body) == payload and z.eof and not z.unused_data
    assert crc == zlib.crc32(payload) and isize == len(payload) and size == len(blk)


def deflate_past_4_gib(codec):
    import torch

    from rawnanoporesignalcompression_amd import bgzf

    d = Wd.deflate()
    off = d.blk_off()
    with Scope():
        src = torch.empty(d.src_bytes, dtype=torch.uint8, device=DEV)
        src[:d.reps * 3 * B].view(d.reps, 3 * B).copy_(up(np.frombuffer(d.period, np.uint8)).unsqueeze(0).expand(d.reps, 3 * B))
        src[d.reps * 3 * B:].copy_(up(np.frombuffer(d.tail, np.uint8)))
        buf, at = sentinel_buffer(Wd.OUT_OFFSET, d.total)
        assert (buf.data_ptr() + at) % 16 == Wd.OUT_OFFSET

        # call 1: everything
        out = buf[at:at + d.total]
        got = bgzf.bgzf_deflate(codec, src, None, out=out)
        torch.cuda.synchronize()
        assert int(got.blk_off.numel()) == d.ntiles + 1
        assert np.array_equal(down(got.blk_off).view(np.uint64), off)
        assert down(got.written).view(np.uint64).tolist() == [d.src_bytes, d.total]
        assert down(out[:d.S]).tobytes() == d.first, "the first period is the model's"
        assert down(out[d.reps * d.S:]).tobytes() == d.tail_file, "the tail block is the model's"
        assert rows_equal_first(out, d.reps, d.S), "every period equals the first"
        assert all_sentinel(buf[:at]) and all_sentinel(buf[at + d.total:])
        j = d.block_of_file_byte(WIDE)                      # the file's block at byte 2^32, and the source's
        k = WIDE // B
        for i in (j, k):
            blk = down(out[int(off[i]):int(off[i + 1])]).tobytes()
            assert blk == d.block_file(i)
            payload = down(src[i * B:(i + 1) * B]).tobytes()
            assert payload == d.block_payload(i)
            check_block(blk, payload)
        assert rows_equal_first(src, d.reps, 3 * B), "the source is untouched"

        # call 2: a capacity that ends at the first block boundary past 2^32
        j = d.first_block_past(WIDE)
        cap = int(off[j])
        buf.fill_(SENTINEL)
        got = bgzf.bgzf_deflate(codec, src, None, out=buf[at:at + cap])
        torch.cuda.synchronize()
        assert down(got.written).view(np.uint64).tolist() == [j * B, cap]
        assert np.array_equal(down(got.blk_off).view(np.uint64), off)
        assert all_sentinel(buf[at + cap:]) and all_sentinel(buf[:at]), "nothing behind the capacity"
        assert down(buf[at + int(off[j - 1]):at + cap]).tobytes() == d.block_file(j - 1), "the last block that fits"
        whole = j // 3
        assert rows_equal_first(buf[at:], whole, d.S) and down(buf[at:at + d.S]).tobytes() == d.first

        # calls 3 and 4: the stream's length from the device, past 2^32, with the whole source as the capacity
        for nbytes, n in ((Wd.NBYTES_PAST, (WIDE + 1) % B), (Wd.NBYTES_ONE, 1)):
            want_off, want_written, last, last_n, last_file = d.cut(nbytes)
            assert last_n == n
            buf.fill_(SENTINEL)
            count = torch.tensor([nbytes], dtype=torch.int64, device=DEV)
            got = bgzf.bgzf_deflate(codec, src, count, out=out)
            torch.cuda.synchronize()
            assert down(got.written).view(np.uint64).tolist() == want_written.tolist()
            have = down(got.blk_off).view(np.uint64)
            assert np.array_equal(have, want_off) and (have[last + 1:] == want_written[1]).all(), "entries above repeat the total"
            end = int(want_written[1])
            blk = down(out[int(want_off[last]):end]).tobytes()
            assert blk == last_file
            check_block(blk, d.block_payload(last, n))
            assert down(out[int(want_off[last - 1]):int(want_off[last])]).tobytes() == d.block_file(last - 1)
            assert all_sentinel(buf[at + end:]) and all_sentinel(buf[:at])
            assert rows_equal_first(out, last // 3, d.S)


# ---- the record writers ----------------------------------------------------------------------------------------------
def device_reads(r):
    """The reads of ``r`` on the device: the same id, bases, qualities, tag value and move table in every read."""
    import torch

    from rawnanoporesignalcompression_amd import DecodedReads

    o = r.one
    qual = repeated(o["qual"], r.n)
    decoded = DecodedReads(repeated(o["seq"], r.n), offsets(r.n, r.m), torch.zeros(r.n, dtype=torch.int32, device=DEV), None, None, None, None)
    ids = repeated(o["id"], r.n).view(r.n, 16)
    tags = {Wd.TAG[0]: torch.full((r.n,), Wd.TAG[1], dtype=torch.int32, device=DEV)}
    moves = None
    if r.F is not None:
        moves = (repeated(o["codes"], r.n), offsets(r.n, r.F), 5)
    return decoded, qual, ids, tags, moves


def check_cut(rec, buf, at, r, first_out, written=None):
    """A call whose capacity ended inside record ``first_out``: the records in front are written, it and every one
    behind have status 1, rec_off is the whole scan, and nothing lies behind the last written record."""
    import torch

    st = rec.status
    assert bool((st[:first_out] == 0).all().item()) and bool((st[first_out:] == Wd.SMALL).all().item())
    assert st[first_out - 1:first_out + 1].cpu().tolist() == [0, Wd.SMALL]
    assert torch.equal(rec.rec_off, offsets(r.n, r.R))
    if written is not None:
        assert rec.written.cpu().tolist() == written
    assert all_sentinel(buf[at + first_out * r.R:]) and all_sentinel(buf[:at])
    assert rows_equal_first(buf[at:], first_out, r.R)


def bam_raw_past_4_gib(codec):
    """The raw layout, with the frame offsets past 2^31: every record, rec_off, written, and a capacity that cuts
    inside the first record that begins past 2^32."""
    import torch

    from rawnanoporesignalcompression_amd import bam

    r = Wd.bam_frames()
    stream, _, _, _ = Wd.bam_model(r, 1)
    with Scope():
        decoded, qual, ids, tags, moves = device_reads(r)
        assert int(moves[1][-1].item()) > 1 << 31
        buf, at = sentinel_buffer(3, r.stream_bytes)
        out = buf[at:at + r.stream_bytes]
        rec = bam.bam_records(codec, decoded, qual, ids, tags, moves=moves, bgzf=False, out=out)
        torch.cuda.synchronize()
        assert torch.equal(rec.rec_off, offsets(r.n, r.R)) and not bool(rec.status.any().item())
        assert rec.written.cpu().tolist() == [r.stream_bytes, r.stream_bytes]
        first = down(out[:r.R]).tobytes()
        assert first == stream, "the first record is the model's"
        got = _bam_cases.parse_records(first)[0]
        assert len(got["seq"]) == r.m and len(got["moves"]) == r.F and got["tags"] == [Wd.TAG] and got["stride"] == 5
        assert rows_equal_first(out, r.n, r.R), "every record equals the first"
        assert all_sentinel(buf[:at]) and all_sentinel(buf[at + r.stream_bytes:])
        at_wide = WIDE // r.R                               # the record that contains byte 2^32
        assert down(out[at_wide * r.R:(at_wide + 1) * r.R]).tobytes() == stream

        cap, first_out = Wd.bam_cut(r)
        buf.fill_(SENTINEL)
        rec = bam.bam_records(codec, decoded, qual, ids, tags, moves=moves, bgzf=False, out=buf[at:at + cap])
        torch.cuda.synchronize()
        check_cut(rec, buf, at, r, first_out, [first_out * r.R, first_out * r.R])


def bam_bgzf_past_4_gib(codec):
    """The BGZF layout, with read_bases past 2^31: 17 records fill two blocks, so the file repeats every 130,622
    bytes; the block that contains file byte 2^32 comes down."""
    import torch

    from rawnanoporesignalcompression_amd import bam

    r = Wd.bam_bases()
    pair, _ = Wd.bam_file(r, Wd.BAM_PAIR)
    pairs = r.n // Wd.BAM_PAIR
    total = Wd.bgzf_bound(r.stream_bytes)
    assert total == pairs * 2 * Wd.FILE == pairs * len(pair)
    with Scope():
        decoded, qual, ids, tags, moves = device_reads(r)
        assert int(decoded.read_bases[-1].item()) > 1 << 31
        buf, at = sentinel_buffer(9, total)
        out = buf[at:at + total]
        rec = bam.bam_records(codec, decoded, qual, ids, tags, moves=moves, bgzf=True, out=out)
        torch.cuda.synchronize()
        assert torch.equal(rec.rec_off, offsets(r.n, r.R)) and not bool(rec.status.any().item())
        assert rec.written.cpu().tolist() == [r.stream_bytes, total]
        assert down(out[:len(pair)]).tobytes() == pair, "the first pair of blocks is the model's"
        assert rows_equal_first(out, pairs, len(pair)), "every pair equals the first"
        assert all_sentinel(buf[:at]) and all_sentinel(buf[at + total:])
        b = WIDE // Wd.FILE                                 # the block that contains file byte 2^32
        blk = down(out[b * Wd.FILE:(b + 1) * Wd.FILE]).tobytes()
        (_, size, body, crc, isize), = _bam_cases.parse_bgzf(blk)
        payload = _bam_cases.stored_payload(body)
        stream, _, _, _ = Wd.bam_model(r, Wd.BAM_PAIR)
        assert payload == stream[(b % 2) * B:(b % 2 + 1) * B] and crc == zlib.crc32(payload) and isize == B and size == Wd.FILE


def fastq_past_4_gib(codec, reverse):
    """The text, forward and with PGN_FASTQ_REVERSE: every record, rec_off, and a capacity one byte short of the end
    of the record that contains byte 2^32."""
    import torch

    from rawnanoporesignalcompression_amd import fastq

    r = Wd.fastq()
    text, _, _ = Wd.fastq_model(r, 1, reverse)
    with Scope():
        decoded, qual, ids, tags, _ = device_reads(r)
        buf, at = sentinel_buffer(11, r.stream_bytes)
        out = buf[at:at + r.stream_bytes]
        rec = fastq.fastq_records(codec, decoded, qual, ids, tags, reverse=reverse, out=out)
        torch.cuda.synchronize()
        assert torch.equal(rec.rec_off, offsets(r.n, r.R)) and not bool(rec.status.any().item())
        assert int(rec.rec_off[-1].item()) == r.stream_bytes >= WIDE + 3 * Wd.T
        assert down(out[:r.R]).tobytes() == text, "the first record is the model's"
        assert rows_equal_first(out, r.n, r.R), "every record equals the first"
        assert all_sentinel(buf[:at]) and all_sentinel(buf[at + r.stream_bytes:])

        cap, first_out = Wd.fastq_cut(r)
        buf.fill_(SENTINEL)
        rec = fastq.fastq_records(codec, decoded, qual, ids, tags, reverse=reverse, out=buf[at:at + cap])
        torch.cuda.synchronize()
        check_cut(rec, buf, at, r, first_out)
        assert down(buf[at + (first_out - 1) * r.R:at + first_out * r.R]).tobytes() == text


# ---- the tests: each body runs in its own frame and leaves no buffer behind -----------------------------------------
@pytest.fixture(autouse=True)
def _nothing_left_cached():
    yield
    import torch

    torch.cuda.empty_cache()


def test_deflate_past_4_gib(codec):
    scoped(deflate_past_4_gib, codec)


def test_bam_raw_past_4_gib(codec):
    scoped(bam_raw_past_4_gib, codec)


def test_bam_bgzf_past_4_gib(codec):
    scoped(bam_bgzf_past_4_gib, codec)


@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reverse"])
def test_fastq_past_4_gib(codec, reverse):
    scoped(fastq_past_4_gib, codec, reverse)
