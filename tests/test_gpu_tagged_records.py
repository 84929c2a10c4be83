"""Typed record tags on the GPU (pgn_bam_records_tagged_device and pgn_fastq_records_tagged_device, through
bam.bam_records and fastq.fastq_records with the wrappers of the tags module), bit for bit against
bam_records_tagged_signal and fastq_records_tagged_signal on the cases of tests/_tag_cases.py: a tile seam on every
byte of a tag area in the raw layout, in BGZF blocks and in FASTQ text, invalid string spans of every kind, the
dictionary's edges, float and integer values, 0 and 16 columns, reads without a record, reversed strings, missing
qualities, every alignment of the output, a capacity that cuts inside a tag area and the empty call.  Every byte that
no written record or block owns keeps its sentinel, in front of and behind ``out`` too.
"""
import ctypes as C
import gzip
import zlib

import numpy as np
import pytest

import _bam_cases
import _tag_cases as K
from rawnanoporesignalcompression_amd.host import TAG_F32, TAG_I32, TAG_STR, TAG_U32

pytestmark = pytest.mark.gpu

SENTINEL, FRONT, BACK = 0xA5, 64, 80
DEV = "cuda:0"


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in K.tag_cases()}


def up(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def device_reads(c):
    from rawnanoporesignalcompression_amd import DecodedReads

    b = c.base
    decoded = DecodedReads(up(b.seq), up(b.read_bases), up(b.status), None, None, None, None)
    keep = None if b.keep is None else up(b.keep)
    qual = None if b.qual is None else up(b.qual)
    moves = None if b.codes is None else (up(b.codes), up(b.read_frames), b.stride, b.frame_base)
    return decoded, qual, up(b.ids.reshape(-1, 16)), keep, moves


def device_tags(c, layout):
    """The case's columns as the Python surface takes them: a wrapper per typed column over the arrays as they are
    (no table is checked: the device decides per read), and a U32 column as a plain tensor where another column makes
    the call the tagged one."""
    from rawnanoporesignalcompression_amd import tags

    cols = c.columns(layout)
    typed = any(col.type != TAG_U32 for _, col in cols)
    out = {}
    for name, col in cols:
        v, off, pool = col.host()
        if col.type == TAG_U32:
            out[name] = up(v.view(np.int32)) if typed else tags.u32(up(v.view(np.int32)))
        elif col.type == TAG_I32:
            out[name] = tags.i32(up(v.view(np.int32)))
        elif col.type == TAG_F32:
            out[name] = tags.f32(up(v.view(np.float32)))
        else:
            table = None
            if off is not None:
                table = tags.StringTable.from_arrays(up(off.view(np.int32)), up(pool))
                assert table.nbytes == col.str_capacity
            out[name] = tags.Tag(col.type, None if col.type == TAG_STR else up(v.view(np.int32)), table)
    return out


def call_without_columns(codec, c, layout, out):
    """The tagged entry points with ``ncols == 0``, which no dict of wrappers reaches: the C calls themselves."""
    import torch

    from rawnanoporesignalcompression_amd import _native, bam, fastq

    decoded, qual, ids, keep, moves = device_reads(c)
    b = c.base
    n, cap, nbytes = len(b.status), len(b.seq), int(out.numel())
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else 0
    rec_off = torch.empty(n + 1, dtype=torch.int64, device=DEV)
    status = torch.empty(n, dtype=torch.int32, device=DEV)
    written = torch.empty(2, dtype=torch.int64, device=DEV)
    cols = _native.RecordTags(0, 0)
    with codec._launch(None) as ls:
        if layout == "fastq":
            prm = _native.FastqParams(_native.PGN_FASTQ_REVERSE if b.reverse else 0, 0)
            rc = codec._lib.pgn_fastq_records_tagged_device(
                codec._h, C.byref(prm), C.byref(cols), n, ptr(ids), ptr(decoded.read_bases), ptr(decoded.status), ptr(keep),
                ptr(decoded.seq), ptr(qual), cap, ptr(out), nbytes, ptr(rec_off), ptr(status), ls.cuda_stream)
            assert rc == 0
            return fastq.FastqRecords(out, rec_off, status)
        flags = (_native.PGN_BAM_REVERSE if b.reverse else 0) | (_native.PGN_BAM_BGZF if layout == "bgzf" else 0)
        prm = _native.BamParams(flags | (_native.PGN_BAM_MOVES if moves else 0), 0)
        prm.stride = b.stride
        rc = codec._lib.pgn_bam_records_tagged_device(
            codec._h, C.byref(prm), C.byref(cols), n, ptr(ids), ptr(decoded.read_bases), ptr(decoded.status), ptr(keep),
            ptr(decoded.seq), ptr(qual), cap, ptr(moves[1]) if moves else 0, ptr(moves[0]) if moves else 0, b.frame_base,
            len(b.codes) if moves else 0, ptr(out), nbytes, ptr(rec_off), ptr(status), ptr(written), ls.cuda_stream)
        assert rc == 0
        return bam.BamRecords(out, rec_off, status, written)


def run(codec, c, layout, stream=None):
    """One call into a view of a sentinel-filled buffer; everything compared."""
    import torch

    from rawnanoporesignalcompression_amd import bam, fastq

    b = c.base
    cap = c.capacity(layout)
    buf = torch.full((FRONT + b.out_offset + cap + BACK,), SENTINEL, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    out = buf[FRONT + b.out_offset:FRONT + b.out_offset + cap]
    if not c.columns(layout):
        rec = call_without_columns(codec, c, layout, out)
    else:
        decoded, qual, ids, keep, moves = device_reads(c)
        tags = device_tags(c, layout)
        if layout == "fastq":
            rec = fastq.fastq_records(codec, decoded, qual, ids, tags, keep=keep, reverse=b.reverse, out=out, stream=stream)
        else:
            rec = bam.bam_records(codec, decoded, qual, ids, tags, keep=keep, reverse=b.reverse, moves=moves,
                                  bgzf=layout == "bgzf", out=out, stream=stream)
    torch.cuda.synchronize()
    data, stream_bytes, off, st, written = c.expected(layout)
    assert rec.data.data_ptr() == out.data_ptr()
    assert np.array_equal(rec.rec_off.cpu().numpy().view(np.uint64), off), (c.name, layout)
    assert np.array_equal(rec.status.cpu().numpy(), st), (c.name, layout)
    if written is not None:
        assert np.array_equal(rec.written.cpu().numpy().view(np.uint64), written), (c.name, layout)
    got = buf.cpu().numpy()
    at = FRONT + b.out_offset
    if got[at:at + len(data)].tobytes() != data:
        bad = np.flatnonzero(got[at:at + len(data)] != np.frombuffer(data, np.uint8))
        raise AssertionError(f"{c.name} {layout}: {len(bad)} bytes differ, the first at {bad[:8].tolist()}")
    # the guard bytes, and with them every byte of a record that was not written
    assert (got[:at] == SENTINEL).all() and (got[at + len(data):] == SENTINEL).all(), (c.name, layout)
    if layout == "bgzf":
        for k, (pos, size, body, crc, isize) in enumerate(_bam_cases.parse_bgzf(rec.tobytes())):
            payload = _bam_cases.stored_payload(body)
            assert pos == k * _bam_cases.FILE and crc == zlib.crc32(payload) and isize == len(payload), (c.name, k)
    return rec


@pytest.mark.parametrize("name,layout", K.runs())
def test_records(codec, cases, name, layout):
    run(codec, cases[name], layout)


def test_the_seam_cases_cross_their_tiles(codec, cases):
    """What the seam cases are for, said once more on the device's output: both BGZF blocks of a seam checksum, and
    the tags on either side of every seam read back."""
    rec = run(codec, cases["tag-seams"], "bgzf")
    plain = gzip.decompress(rec.tobytes())
    recs = K.parse_records(plain)
    assert len(recs) == len(cases["tag-seams"].base.status) and len(plain) > (K.SEAM_AREA + 1) * K.BLOCK
    assert all([t[0] for t in r["tags"]] == ["ts", "qs", "BC", "mv"] and r["tags"][2][2] == K.SEAM_Z for r in recs)


def test_identity_with_the_old_calls(codec, cases):
    """With U32 columns only, every output of the tagged calls is that of the old calls with the same columns."""
    import torch

    from rawnanoporesignalcompression_amd import bam, fastq, tags

    for name in ("tag-seams", "tag-gaps", "tag-reverse-nomoves", "tag-align+7", "tag-empty"):
        c = cases[name]
        decoded, qual, ids, keep, moves = device_reads(c)
        n = len(c.base.status)
        plain = {"qs": up((np.arange(n, dtype=np.uint32) * 1_000_003).view(np.int32)), "ch": up(np.full(n, -1, np.int32))}
        typed = {k: tags.u32(v) for k, v in plain.items()}
        for bgzf in (False, True):
            old = bam.bam_records(codec, decoded, qual, ids, plain, keep=keep, reverse=c.base.reverse, moves=moves, bgzf=bgzf)
            new = bam.bam_records(codec, decoded, qual, ids, typed, keep=keep, reverse=c.base.reverse, moves=moves, bgzf=bgzf)
            assert old.tobytes() == new.tobytes() and int(old.data.numel()) == int(new.data.numel()), (name, bgzf)
            assert all(torch.equal(getattr(old, f), getattr(new, f)) for f in ("rec_off", "status", "written")), (name, bgzf)
            assert int(old.written[0]) > 0 or n == 0
        if qual is not None:
            old = fastq.fastq_records(codec, decoded, qual, ids, plain, keep=keep, reverse=c.base.reverse)
            new = fastq.fastq_records(codec, decoded, qual, ids, typed, keep=keep, reverse=c.base.reverse)
            assert old.tobytes() == new.tobytes() and torch.equal(old.rec_off, new.rec_off) and torch.equal(old.status, new.status)


def test_records_to_deflated_blocks_with_a_barcode_tag(codec, cases):
    """bam_records(bgzf=False) -> bgzf_deflate -> gzip -> the parser, with demux.barcode_tag's column: classified
    reads carry BC:Z with their barcode's name, unclassified ones none, or the name given for them."""
    import torch

    from rawnanoporesignalcompression_amd import bam, bgzf, demux, tags

    c = cases["tag-reverse"]
    decoded, qual, ids, keep, moves = device_reads(c)
    n = len(c.base.status)
    names = ["kit-barcode%02d" % k for k in range(1, 4)]
    barcode = np.array([(r % 5) if r % 5 < 3 else -1 for r in range(n)], np.int32)
    ts = np.arange(n, dtype=np.int32) * -1000
    for unclassified in (None, "unclassified"):
        col = demux.barcode_tag(up(barcode), names, unclassified=unclassified)
        rec = bam.bam_records(codec, decoded, qual, ids, {"ts": tags.i32(up(ts)), "BC": col, "ch": up(np.arange(n, dtype=np.int32))},
                              reverse=True, moves=moves, bgzf=False)
        blocks = bgzf.bgzf_deflate(codec, rec.data, rec.written[:1])
        assert torch.equal(rec.status, torch.zeros_like(rec.status))
        recs = K.parse_records(gzip.decompress(blocks.tobytes()))
        assert len(recs) == n
        for r, got in enumerate(recs):
            want = [("ts", "i", int(ts[r]))]
            if barcode[r] >= 0 or unclassified:
                want.append(("BC", "Z", (names[barcode[r]] if barcode[r] >= 0 else unclassified).encode()))
            want.append(("ch", "I", r))
            assert got["tags"][:-1] == want and got["tags"][-1][0] == "mv", r


def test_which_symbol_a_dict_reaches(codec, cases):
    """A dict of plain integer tensors still goes to the old C calls; one wrapper among them to the tagged ones; a
    plain float tensor and an f32 column in FASTQ are ValueErrors, as are 9 plain and 17 typed columns."""
    import torch

    from rawnanoporesignalcompression_amd import bam, fastq, tags

    class Recorder:
        def __init__(self, lib):
            self.lib, self.names = lib, []

        def __getattr__(self, name):
            self.names.append(name)
            return getattr(self.lib, name)

    c = cases["tag-reverse"]
    decoded, qual, ids, keep, moves = device_reads(c)
    col = up(np.arange(len(c.base.status), dtype=np.int32))
    lib = codec._lib
    codec._lib = rec = Recorder(lib)
    try:
        bam.bam_records(codec, decoded, qual, ids, {"qs": col, "ch": col})
        fastq.fastq_records(codec, decoded, qual, ids, {"qs": col})
        bam.bam_records(codec, decoded, qual, ids, {"qs": col, "ts": tags.i32(col)})
        fastq.fastq_records(codec, decoded, qual, ids, {"qs": tags.u32(col)})
    finally:
        codec._lib = lib
    torch.cuda.synchronize()
    assert [n for n in rec.names if "records" in n] == ["pgn_bam_records_device", "pgn_fastq_records_device",
                                                        "pgn_bam_records_tagged_device", "pgn_fastq_records_tagged_device"]
    for call, t in ((bam.bam_records, {"qs": col.float()}), (fastq.fastq_records, {"qs": col.float()}),
                    (fastq.fastq_records, {"qs": tags.f32(col.float())}), (bam.bam_records, {f"t{k}": col for k in range(9)}),
                    (bam.bam_records, {f"t{chr(97 + k)}": tags.u32(col) for k in range(17)}),
                    (bam.bam_records, {"pi": tags.zstr([b"host"] * len(c.base.status))}),
                    (bam.bam_records, {"pi": tags.zstr([b"short"]).to(DEV)}), (bam.bam_records, {"ts": tags.i32(col[:-1])})):
        with pytest.raises(ValueError):
            call(codec, decoded, qual, ids, t)
    # sixteen typed columns are fine, and the default buffers hold them
    many = {f"t{chr(97 + k)}": tags.u32(col) if k % 2 else tags.i32(col) for k in range(16)}
    rec = bam.bam_records(codec, decoded, qual, ids, many, moves=moves)
    assert torch.equal(rec.status, torch.zeros_like(rec.status)) and len(K.parse_records(gzip.decompress(rec.tobytes()))[0]["tags"]) == 17
