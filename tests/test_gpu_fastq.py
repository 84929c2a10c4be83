"""FASTQ records on the GPU (pgn_fastq_records_device through fastq.fastq_records), bit for bit against
fastq_records_signal on the cases of tests/_fastq_cases.py: small reads at every alignment of record and source, a
tile boundary in front of every kind of record byte, one record over several tiles and a thousand in three, reads
without a record, the tag counts and values, reversed strings, every alignment of the output and every kind of byte
capacity.  Every byte that no written record owns keeps its sentinel, in front of and behind ``out`` too.
"""
import numpy as np
import pytest

import _fastq_cases as K

pytestmark = pytest.mark.gpu

SENTINEL, FRONT, BACK = 0xA5, 64, 80


@pytest.fixture(scope="module")
def cases():
    return {c.name: (c, c.expected()) for c in K.record_cases()}


def device_arrays(c):
    import torch

    from rawnanoporesignalcompression_amd import DecodedReads

    dev = "cuda:0"
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    decoded = DecodedReads(up(c.seq), up(c.read_bases), up(c.status), None, None, None, None)
    tags = {name: up(v.view(np.int32)) for name, v in c.tags}
    keep = None if c.keep is None else up(c.keep)
    return decoded, up(c.qual), up(c.ids.reshape(-1, 16)), tags, keep


def run(codec, c, want, stream=None):
    """One call into a view of a sentinel-filled buffer; everything compared."""
    import torch

    from rawnanoporesignalcompression_amd import fastq

    decoded, qual, ids, tags, keep = device_arrays(c)
    cap = c.capacity
    buf = torch.full((FRONT + c.out_offset + cap + BACK,), SENTINEL, dtype=torch.uint8, device="cuda:0")
    assert buf.data_ptr() % 16 == 0
    out = buf[FRONT + c.out_offset:FRONT + c.out_offset + cap]
    rec = fastq.fastq_records(codec, decoded, qual, ids, tags, keep=keep, reverse=c.reverse, out=out, stream=stream)
    torch.cuda.synchronize()
    text, off, st = want
    assert rec.data.data_ptr() == out.data_ptr()
    assert np.array_equal(rec.rec_off.cpu().numpy().view(np.uint64), off), c.name
    assert np.array_equal(rec.status.cpu().numpy(), st), c.name
    got = buf.cpu().numpy()
    at = FRONT + c.out_offset
    assert got[at:at + len(text)].tobytes() == text, c.name
    assert (got[:at] == SENTINEL).all() and (got[at + len(text):] == SENTINEL).all(), c.name
    if int(off[-1]) <= cap:
        assert rec.tobytes() == text
    return rec


@pytest.mark.parametrize("name", [c.name for c in K.record_cases()])
def test_records(codec, cases, name):
    c, want = cases[name]
    run(codec, c, want)


def test_the_case_list_covers_the_issue():
    got = [c.name for c in K.record_cases()]
    for prefix, count in (("small+", 4 + 1), ("seam-", len(K.SEAM_BYTES)), ("long", 2), ("thousand", 1), ("without", 1),
                          ("run-across", 1), ("none", 1), ("tags", 3), ("reverse", 1), ("small-reverse", 1),
                          ("capacity", 4), ("empty", 1)):
        assert len([n for n in got if n.startswith(prefix)]) == count, prefix


def test_no_kept_read_leaves_out_untouched(codec, cases):
    c, want = cases["none"]
    rec = run(codec, c, want)
    assert not rec.rec_off.cpu().numpy().any() and want[0] == b""


def test_default_out_and_tobytes(codec, cases):
    """Without ``out`` the call sizes it by fastq_bound; tobytes() is the text."""
    import torch

    from rawnanoporesignalcompression_amd import fastq

    c, (text, off, st) = cases["tags8"]
    decoded, qual, ids, tags, keep = device_arrays(c)
    rec = fastq.fastq_records(codec, decoded, qual, ids, tags)
    assert int(rec.data.numel()) == fastq.fastq_bound(len(c.status), len(c.seq), 8)
    assert rec.tobytes() == text and torch.equal(rec.status, torch.zeros_like(rec.status))


def test_repeated_calls_and_a_callers_stream(codec, cases):
    """Two calls in succession with different shapes on one codec, then one on a caller's stream."""
    import torch

    for name in ("thousand", "seam-plus", "long"):
        run(codec, *cases[name])
    s = torch.cuda.Stream()
    run(codec, *cases["without"], stream=s.cuda_stream)
    run(codec, *cases["small+3"], stream=s.cuda_stream)
    run(codec, *cases["thousand"])


def test_read_tags_of_a_reads_table(codec):
    """The ids, channels and read numbers of a selection, as the record call takes them."""
    import types
    import uuid

    from rawnanoporesignalcompression_amd import fastq

    rng = np.random.default_rng(9)
    table = types.SimpleNamespace(read_id=rng.integers(0, 256, (6, 16)).astype(np.uint8),
                                  channel=np.array([1, 512, 3000, 7, 65535, 9], np.uint16),
                                  read_number=np.array([0, 5, 4294967295, 77, 8, 123456], np.uint32))
    pick = [4, 2, 0]
    ids, ch, rn = fastq.read_tags(table, pick, codec.device)
    assert ids.is_cuda and tuple(ids.shape) == (3, 16) and ch.dtype == rn.dtype
    c = K.make("picked", [3, 2, 4], 10)
    decoded, qual, _, _, _ = device_arrays(c)
    text = fastq.fastq_records(codec, decoded, qual, ids, {"ch": ch, "rn": rn}).tobytes()
    heads = text.split(b"\n")[0:12:4]
    assert heads == [f"@{uuid.UUID(bytes=table.read_id[r].tobytes())}\tch:i:{int(table.channel[r])}"
                     f"\trn:i:{int(table.read_number[r])}".encode() for r in pick]
    every = fastq.read_tags(table, None, codec.device)
    assert tuple(every[0].shape) == (6, 16) and every[1].cpu().numpy().view(np.uint32).tolist() == table.channel.tolist()


def test_python_refusals(codec, cases):
    import torch

    from rawnanoporesignalcompression_amd import fastq

    c, _ = cases["tags1"]
    decoded, qual, ids, tags, keep = device_arrays(c)
    n = len(c.status)
    bad_tags = [{"q": tags["qs"]}, {"1s": tags["qs"]}, {"qs": tags["qs"][:-1]}, {"qs": tags["qs"].float()},
                {"qs": tags["qs"].cpu()}, {f"t{k}": tags["qs"] for k in range(9)}]
    for t in bad_tags:
        with pytest.raises(ValueError):
            fastq.fastq_records(codec, decoded, qual, ids, t)
    for kw in (dict(read_ids=ids[:-1]), dict(read_ids=ids.cpu()), dict(qual=qual[:-1]), dict(keep=torch.ones(n + 1, dtype=torch.uint8, device="cuda:0")),
               dict(out=torch.empty(10, dtype=torch.int8, device="cuda:0")), dict(out=torch.empty(10, dtype=torch.uint8))):
        args = dict(qual=qual, read_ids=ids)
        args.update({k: v for k, v in kw.items() if k in args})
        rest = {k: v for k, v in kw.items() if k not in args}
        with pytest.raises(ValueError):
            fastq.fastq_records(codec, decoded, args["qual"], args["read_ids"], tags, **rest)
