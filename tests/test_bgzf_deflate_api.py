"""BGZF deflate (pgn_bgzf_deflate_device): the C ABI surface, the refusals, the rule's text and the host model,
without a GPU.

The model is held to zlib: every block's body inflates to its payload with nothing left over, the file to the
stream, and the CRC field to ``zlib.crc32``; the code lengths to the Kraft sum and to the unrestricted construction
where that fits; the size to zlib's own Huffman-only output.  The cases of the GPU tests are built here too, so the
conditions their builders assert are checked on the CPU.
"""
import ctypes as C
import gzip
import io
import os
import re
import zlib

import numpy as np
import pytest

import _bam_cases
import _bgzf_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FN = "pgn_bgzf_deflate_device"


def _header(comments=False):
    src = open(os.path.join(ROOT, "include", "pgnano_hip.h")).read()
    return src if comments else re.sub(r"/\*.*?\*/", "", src, flags=re.S)


@pytest.fixture(scope="module")
def cases():
    return K.deflate_cases()


# ---- surface -------------------------------------------------------------------------------------------------
def test_symbol_declared_exported_and_bound():
    import rawnanoporesignalcompression_amd as pkg
    from rawnanoporesignalcompression_amd import _native, bam, bgzf, host

    lib = _native.load()
    sigs = {s[0]: s for s in _native.SIGNATURES}
    assert re.search(r"\bint\s+" + FN + r"\s*\(", _header())
    assert hasattr(lib, FN)
    assert sigs[FN][1] is C.c_int and len(sigs[FN][2]) == 10
    for name in ("bgzf_deflate", "write_gz", "BgzfBlocks", "deflate_lengths_signal", "deflate_block_signal",
                 "bgzf_deflate_signal", "bgzf_bound", "BGZF_EOF"):
        assert name in bgzf.__all__ and hasattr(bgzf, name)
        assert name not in pkg.__all__                      # the package's own surface stays as it is
    for name in ("deflate_lengths_signal", "deflate_block_signal", "bgzf_deflate_signal", "bgzf_bound", "BGZF_EOF"):
        assert getattr(bgzf, name) is getattr(host, name)
    assert not hasattr(pkg.PGNanoCodec, "bgzf_deflate")
    assert bgzf.BGZF_EOF is bam.BGZF_EOF
    src = open(os.path.join(ROOT, "rawnanoporesignalcompression_amd", "csrc", "pgn_kernels.hip")).read()
    assert '#include "pgn_deflate.h"' in src


def test_call_refusals_and_their_order():
    from rawnanoporesignalcompression_amd import _native

    fn = getattr(_native.load(), FN)
    bad = _native.PGN_ERR_INVALID_ARG
    dummy = C.c_void_p(0x1000)

    def call(ctx=dummy, flags=0, src=dummy, scap=100, nbytes=None, out=dummy, cap=200, off=dummy, wr=dummy):
        return fn(ctx, flags, src, scap, nbytes, out, cap, off, wr, None)

    assert call(ctx=None) == bad
    for flags in (1, 4, 1 << 31):
        assert call(flags=flags) == bad, flags
    assert call(src=None) == bad
    assert call(off=None) == bad
    assert call(wr=None) == bad
    assert call(off=None, scap=0, src=None) == bad          # ... with nothing to read, too
    assert call(wr=None, scap=0, src=None) == bad
    assert call(out=None) == bad
    for scap in (1 << 48, 1 << 63):
        assert call(scap=scap) == bad, scap
    assert call(ctx=None, flags=1, src=None, off=None, out=None, scap=1 << 48) == bad


def test_the_header_carries_the_rule():
    src = re.sub(r"\s*\n \*\s*", " ", _header(comments=True))
    for text in ("---- BGZF deflate", "W = min(*d_nbytes, src_capacity)", "BSIZE as u16 = the block's total length minus 1",
                 "the dynamic block below if its byte length is < n + 5, else the stored block 01 n ~n p",
                 "A tie stores.", "cnt[256] = 1, the end-of-block symbol", "ll = lengths(cnt, 15) over the 257 symbols",
                 "BFINAL = 1 in 1 bit; BTYPE = 2 in 2 bits; HLIT = 0 in 5 bits (257 codes); HDIST = 1 in 5 bits",
                 "The length sequence has 259 entries: ll[0..256], 1, 1.",
                 "symbol 18 with t = min(r, 138), extra value t - 11 in 7 bits", "symbol 17 with r - 3 in 3 bits",
                 "symbol 16 with t = min(r, 6), extra value t - 3 in 2 bits",
                 "cl = lengths(histogram of those symbols, 7) over the 19 code-length symbols",
                 "16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15", "sorted by (cnt, symbol) ascending, are the leaf queue",
                 "the leaf where its weight is <= the internal node's", "One used symbol alone gets length 1.",
                 "take the longest length, then the smallest count, then the largest symbol",
                 "take the largest count, then the smallest symbol",
                 "Block k is written iff blk_off[k + 1] <= byte_capacity", "d_written[0] = min(W, 65280 * kw)",
                 "There are no partial blocks.", "entries above nblocks repeat the total",
                 "the scratch is 1,568 bytes per block",
                 "Not covered: a match search, so the output is Huffman only; several deflate blocks per BGZF block; "
                 "fixed-Huffman blocks; a .gzi or .bai index from blk_off; fusing into the record writers; decompression.",
                 # the sections whose gap this closes keep their sentences and point here
                 "Not covered: deflate compression (every block holds a stored deflate block, as `samtools view -u` writes);",
                 "framing of other buffers.  Both are pgn_bgzf_deflate_device's (\"BGZF deflate\" below)",
                 "compression of the text;", "The text leaves compressed through pgn_bgzf_deflate_device (\"BGZF deflate\" below)."):
        assert text in src, text
    assert src.index("---- BAM records") < src.index("---- BGZF deflate")
    for path in ("README.md", "DESIGN.md", os.path.join("tools", "README.md")):
        text = re.sub(r"\s+", " ", open(os.path.join(ROOT, path)).read())
        assert "BGZF deflate" in text and "bgzf_deflate" in text, path


# ---- the model against zlib ----------------------------------------------------------------------------------------
def test_every_case_inflates_and_is_laid_out(cases):
    for c in cases:
        data, off, written = c.expected()
        stream = c.data[:c.W]
        assert off.dtype == np.uint64 and written.dtype == np.uint64 and len(off) == c.ntiles + 1
        consumed = int(written[0])
        assert (gzip.decompress(data) if data else b"") == stream[:consumed], c.name
        blocks = _bam_cases.parse_bgzf(data)
        assert consumed == min(c.W, K.B * len(blocks)) and (consumed == c.W or consumed % K.B == 0)
        for k, (at, size, body, crc, isize) in enumerate(blocks):
            p = stream[k * K.B:(k + 1) * K.B]
            assert at == int(off[k]) and at + size == int(off[k + 1]) <= c.capacity, (c.name, k)
            z = zlib.decompressobj(-15)
            assert z.decompress(body) == p and z.eof and not z.unused_data and not z.unconsumed_tail, (c.name, k)
            assert crc == zlib.crc32(p) and isize == len(p), (c.name, k)
            assert len(body) <= len(p) + 5 and (body[0] & 7) in (1, 5)    # final, and stored or dynamic
            assert (body[0] & 7 == 1) == (len(body) == len(p) + 5), "a block is stored iff it is as long as the stored form"
        nblocks = -(-c.W // K.B)
        assert (off[nblocks:] == off[nblocks]).all() and (np.diff(off.astype(np.int64))[:nblocks] > 26).all()
        # the written blocks are the longest prefix that the capacity holds
        assert len(blocks) == nblocks or int(off[len(blocks) + 1]) > c.capacity, c.name
        from rawnanoporesignalcompression_amd.host import bgzf_bound
        assert int(off[-1]) <= bgzf_bound(c.W)


def test_python_model_refusals():
    from rawnanoporesignalcompression_amd.host import deflate_block_signal

    for p in (b"", bytes(K.B + 1)):
        with pytest.raises(ValueError):
            deflate_block_signal(p)


def _unrestricted(cnt):
    """Code lengths by a textbook Huffman construction with the rule's tie order, written apart from the model."""
    import heapq

    heap = [(c, 0, s, (s,)) for s, c in enumerate(cnt) if c]      # leaves before internal nodes, then by age
    depth = {s: 0 for _, _, s, _ in heap}
    if len(heap) == 1:
        return {heap[0][2]: 1}
    heapq.heapify(heap)
    age = 0
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for s in a[3] + b[3]:
            depth[s] += 1
        age += 1
        heapq.heappush(heap, (a[0] + b[0], 1, age, a[3] + b[3]))
    return depth


def test_lengths_on_direct_histograms():
    from rawnanoporesignalcompression_amd.host import deflate_lengths_signal

    rng = np.random.default_rng(81)
    fib = [1, 2]
    while len(fib) < 30:
        fib.append(fib[-1] + fib[-2] + 1)
    hists = [[5], [0, 0, 7], [1, 1], [3, 0, 3, 3], [1] * 257, [1] * 19, fib[:20] + [1], fib[:12], list(range(1, 258)),
             [1, 1, 2, 4, 8, 16, 32, 64, 128, 256, 512], [0] * 10]
    for _ in range(300):
        k = int(rng.integers(1, 258))
        h = (rng.pareto(0.5, k) * 3).astype(np.int64) % 60000
        hists.append(h.tolist())
    deep = {15: 0, 7: 0}
    for h in hists:
        for limit, width in ((15, 257), (7, 19)):
            cnt = h[:width]
            got = deflate_lengths_signal(cnt, limit)
            used = [v for v in got if v]
            assert len(got) == len(cnt) and [v > 0 for v in got] == [c > 0 for c in cnt]
            assert max(got, default=0) <= limit
            if len(used) >= 2:
                assert sum(1 << (limit - v) for v in used) == 1 << limit, "the Kraft sum is exactly 1"
            elif used:
                assert used == [1]
            free = _unrestricted(cnt)
            if max(free.values(), default=0) <= limit:
                assert {s: v for s, v in enumerate(got) if v} == free
            else:
                deep[limit] += 1
                # the limiter only moves bits: never below the unrestricted cost
                assert sum(c * v for c, v in zip(cnt, got)) >= sum(cnt[s] * v for s, v in free.items())
    assert deep[15] >= 1 and deep[7] >= 10, deep


def test_size_against_zlib_huffman_only(cases):
    """A guard on the length rule: within 2 % of zlib's own Huffman-only streams, block by block (the margin is for
    other zlib versions' block cuts).  With zlib 1.2.11 the ratios are 1.0191 on the long read, whose fields zlib meets
    with a new deflate block every 32,768 literals, and 1.0003 on the deep histogram."""
    by_name = {c.name: c for c in cases}
    for name in ("bam", "deep-histogram"):
        c = by_name[name]
        data, off, _ = c.expected()
        ours = sum(size - 26 for _, size, _, _, _ in _bam_cases.parse_bgzf(data))
        theirs = 0
        for at in range(0, len(c.data), K.B):
            z = zlib.compressobj(9, zlib.DEFLATED, -15, 9, zlib.Z_HUFFMAN_ONLY)
            theirs += len(z.compress(c.data[at:at + K.B]) + z.flush())
        print(f"{name}: {ours} deflate bytes, zlib Z_HUFFMAN_ONLY {theirs}, ratio {ours / theirs:.4f}")
        assert ours <= 1.02 * theirs, (name, ours, theirs)


def test_write_gz_and_write_bam(tmp_path, cases):
    from rawnanoporesignalcompression_amd import bam, bgzf

    by_name = {c.name: c for c in cases}
    text, stream = by_name["fastq"], by_name["bam"]
    path = tmp_path / "reads.fastq.gz"
    n = bgzf.write_gz(str(path), [text.expected()[0], by_name["w-0"].expected()[0], by_name["tiny-2"].expected()[0]])
    raw = path.read_bytes()
    assert n == len(raw) and raw.endswith(bgzf.BGZF_EOF)
    assert gzip.decompress(raw) == text.data + by_name["tiny-2"].data
    buf = io.BytesIO()
    assert bgzf.write_gz(buf, []) == 28 and buf.getvalue() == bgzf.BGZF_EOF
    buf = io.BytesIO()
    bam.write_bam(buf, [stream.expected()[0]])
    plain = gzip.decompress(buf.getvalue())
    assert plain == bam.bam_header() + stream.data
    assert len(_bam_cases.parse_records(plain[len(bam.bam_header()):])) == 5
    assert len(buf.getvalue()) < 0.45 * len(plain)


def test_the_case_list_covers_the_issue(cases):
    got = [c.name for c in cases]
    for prefix, count in (("bam", 1), ("fastq", 1), ("zeros", 1), ("tiny-", 2), ("uniform", 1), ("every-value", 1),
                          ("two-values", 1), ("equal-lengths", 1), ("deep-histogram", 1), ("limited-header", 1),
                          ("break-even", 3), ("w-", 7), ("align-", 8), ("capacity-", 7), ("nbytes-", 4)):
        assert len([n for n in got if n.startswith(prefix)]) == count, prefix
    assert sorted(len(c.data) for c in cases if c.name.startswith("w-")) == sorted(K.W_CASES)
    assert {(c.src_offset, c.out_offset) for c in cases} == {(s, o) for s in K.OFFSETS for o in K.OFFSETS}
    assert {c.nbytes is None for c in cases} == {True, False}
