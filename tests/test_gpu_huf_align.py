"""dec_huf_kernel's output geometry against the oracle, at zero tolerance (samples and statuses).

A lane of the deferred Huffman decoder (one lane per stream, 16 frames per wave) first decodes the
h = (16 - (dst & 15)) & 15 symbols in front of its destination's first 16-byte boundary, then whole
aligned blocks, starting 7 - m0 iterations late (m0: blocks before its first 128-byte line), in trips
of eight iterations with a body of their own while every lane with blocks is inside its stream.  The
M stream of a C5 chunk starts at keys bytes + S bytes of the chunk's intermediate and lane q of its
section at (rs + 3) / 4 * q further, so a chunk here is built from its streams: the sample count, the
class-1 count and the M size choose every h and m0; the M frame is libzstd's, or written by hand
(literals only, four streams) for sections no encoder writes.  Small batches take the deferred path
through PGN_DEFER_MIN_CHUNKS=1, as in test_gpu_hufjob.py.  The output tensor carries sentinel samples
between the chunks' spans.  (The decoder's junk line lies in the context's own scratch, which the
binding does not expose: its neighbours are the job records and tables of the same pass, so a write
beside it shows as a wrong sample or status of that pass.)
"""
import os
import struct

import numpy as np
import pytest

import _oracle as O
import _zframes as Z

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5B
GAP = 8


@pytest.fixture(scope="module")
def dcodec():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rawnanoporesignalcompression_amd import PGNanoCodec

    keys = ("PGN_DEFER_MIN_CHUNKS", "PGN_DEFER_G", "PGN_DEFER_TAIL_PLAIN", "PGN_HUF_WIDE_LAST")
    old = {k: os.environ.get(k) for k in keys}
    os.environ["PGN_DEFER_MIN_CHUNKS"] = "1"
    os.environ["PGN_DEFER_G"] = "96"
    os.environ["PGN_DEFER_TAIL_PLAIN"] = "0"
    os.environ["PGN_HUF_WIDE_LAST"] = "0"
    try:
        c = PGNanoCodec(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    yield c
    c.close()


# ---- chunks from their streams ------------------------------------------------------------------------
def _keys(classes):
    c = np.asarray(classes, np.uint8)
    c = np.concatenate([c, np.zeros((-c.size) % 4, np.uint8)]).reshape(-1, 4)
    return (c[:, 0] | (c[:, 1] << 2) | (c[:, 2] << 4) | (c[:, 3] << 6)).astype(np.uint8).tobytes()


def _skewed(rng, n, alphabet=40):
    return np.minimum(rng.geometric(0.12, n) - 1, alphabet - 1).astype(np.uint8).tobytes()


def huf4_frame(parts, table, n=None):
    """A single-segment frame of one compressed block without sequences whose literals are four Huffman
    streams holding `parts` (4-byte literals header, direct weights); n: the regenerated size it claims."""
    n = sum(len(p) for p in parts) if n is None else n
    desc = table.describe("direct")
    enc = [table.encode(p) for p in parts]
    body = struct.pack("<3H", *(len(e) for e in enc[:3])) + b"".join(enc)
    comp = len(desc) + len(body)
    assert n < (1 << 14) and comp < (1 << 14)
    lsec = (2 | 2 << 2 | n << 4 | comp << 18).to_bytes(4, "little") + desc + body
    block = lsec + b"\x00"
    hdr = struct.pack("<I", Z.MAGIC)
    hdr += bytes([0x20, n]) if n < 256 else bytes([0x60]) + struct.pack("<H", n - 256)
    return hdr + (1 | 2 << 1 | len(block) << 3).to_bytes(3, "little") + block


def quarters(m):
    seg = (len(m) + 3) // 4
    assert 3 * seg <= len(m)
    return [m[0:seg], m[seg:2 * seg], m[2 * seg:3 * seg], m[3 * seg:]]


class Chunk:
    """n samples: n1 of class 1, then len(m) of class 2, the rest of class 0; mframe: the M stream's frame"""

    def __init__(self, rng, n1, m, mframe=None, pad=5):
        self.n = n1 + len(m) + pad
        cls = [1] * n1 + [2] * len(m) + [0] * pad
        s = rng.integers(0, 256, (n1 + 1) // 2, dtype=np.uint8)
        if n1 & 1:
            s[-1] &= 15
        self.mstart = (self.n + 3) // 4 + s.size  # where M starts in the chunk's intermediate
        self.rs = len(m)
        frames = [O.zstd_compress1(_keys(cls)), O.zstd_compress1(s.tobytes()),
                  mframe if mframe is not None else O.zstd_compress1(m), O.zstd_compress1(b""), O.zstd_compress1(b"")]
        self.blob = O.c5_assemble(frames)

    def lanes(self):
        """(h, m0) of the four lanes, for an intermediate that starts on a line"""
        seg = (self.rs + 3) // 4
        out = []
        for q in range(4):
            d = self.mstart + seg * q
            h = -d % 16
            out.append((h, (-(d + h) % 128) // 16))
        return out


def _m_frame(rng, m, L=6):
    t = Z.HufTable.for_content(m, L, span=129)
    return huf4_frame(quarters(m), t)


def check(codec, chunks):
    import torch

    assert len(chunks) > 64  # (smaller batches take the cooperative decoder, not the deferred pass)
    dev = torch.device("cuda", 0)
    blobs = [c.blob for c in chunks]
    lens = np.array([c.n for c in chunks], np.int64)
    sizes = np.array([len(b) for b in blobs], np.int64)
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    flat = np.frombuffer(b"".join(blobs), np.uint8).copy()
    so = np.cumsum(np.concatenate([[GAP], lens[:-1] + GAP])).astype(np.int64)
    total = int(so[-1] + lens[-1] + GAP)
    out = torch.full((total,), SENTINEL, dtype=torch.int16, device=dev)
    res, _, st = codec.decompress_batch(torch.from_numpy(flat).to(dev), torch.from_numpy(offs).to(dev),
                                        torch.from_numpy(sizes).to(dev), torch.from_numpy(lens.astype(np.int32)).to(dev),
                                        out=out, out_offsets=torch.from_numpy(so).to(dev))
    torch.cuda.synchronize()
    assert "dec_huf_kernel" in codec.kernels(1)
    o, st = res.cpu().numpy(), st.cpu().numpy()
    statuses = []
    for i, c in enumerate(chunks):
        rc, ref = O.c5_decompress(c.blob, c.n)
        if rc == 0 and not O.c5_frames_strictly_valid(c.blob):
            rc = 3  # libzstd's double-symbol decoder accepts one trailing codeword; this decoder does not
        assert st[i] == rc, (i, rc, st[i])
        statuses.append(rc)
        if rc == 0:
            assert np.array_equal(o[so[i]:so[i] + c.n], ref), (i, c.lanes())
    # the gaps between the spans (a failed chunk's span is not compared: its content is unspecified)
    gaps = np.ones(total, bool)
    for i, c in enumerate(chunks):
        gaps[so[i]:so[i] + c.n] = False
    assert (o[gaps] == np.int16(SENTINEL)).all(), np.flatnonzero(gaps & (o != np.int16(SENTINEL)))[:8]
    return statuses


# ---- every alignment ------------------------------------------------------------------------------------
def _sweep(rng):
    """256 chunks, M sections of 256 .. 400 literals (the smallest an encoder writes with four streams);
    consecutive chunks differ in both residues, so the lanes of a wave start late by different amounts"""
    out = []
    for i in range(256):
        n1 = 2 * ((37 * i) % 128) + (i // 128)
        rs = 256 + (i * 29) % 145
        m = _skewed(rng, rs)
        out.append(Chunk(rng, n1, m, None if i % 2 else _m_frame(rng, m), pad=5 + i % 4))
    return out


def test_every_head_length_and_line_offset_on_every_lane(dcodec):
    rng = np.random.default_rng(5)
    chunks = _sweep(rng)
    for q in range(4):
        assert {c.lanes()[q][0] for c in chunks} == set(range(16)), q
        assert {c.lanes()[q][1] for c in chunks} == set(range(8)), q
    for w in range(0, 256, 16):  # mixed inside a wave's 16 chunks
        assert len({c.lanes()[0] for c in chunks[w:w + 16]}) >= 8
    assert any(c.rs % 4 for c in chunks)  # a shorter fourth stream
    assert check(dcodec, chunks) == [0] * 256


def test_symbols_after_the_head(dcodec):
    """lane 0's stream holds exactly h + k symbols for k = 0, 15, 16, 17, 32 (hand-made sections: an
    encoder's smallest lanes hold 64), and sections below 64 literals, where a stream is shorter than h"""
    rng = np.random.default_rng(6)
    chunks = []
    for k in (0, 15, 16, 17, 32):
        for h in (1, 6, 15):
            seg = h + k
            for n1 in range(0, 64, 2):  # n1 for which M starts at -h mod 16
                m = _skewed(rng, 4 * seg, 20)
                c = Chunk(rng, n1, m, _m_frame(rng, m, L=5))
                if c.lanes()[0][0] == h:
                    chunks.append(c)
                    break
            else:
                raise AssertionError((k, h))
    for i in range(96):  # regenerated sizes 8 .. 63, every alignment
        m = _skewed(rng, 8 + (i * 7) % 56, 12)
        chunks.append(Chunk(rng, 2 * (i % 16) + 32 * (i % 3) + 2 * (i // 48), m, _m_frame(rng, m, L=4)))
    assert any(min(len(p) for p in quarters(b"x" * c.rs)) < max(h for h, _ in c.lanes()) for c in chunks[15:])
    m = _skewed(rng, 297)  # the fourth stream three symbols shorter
    chunks.append(Chunk(rng, 10, m, _m_frame(rng, m)))
    assert check(dcodec, chunks) == [0] * len(chunks)


# ---- code lengths and the end of a stream ----------------------------------------------------------------
def test_longest_and_shortest_codes_and_the_end_bit(dcodec):
    rng = np.random.default_rng(7)
    chunks = []
    # 11-bit codes throughout: only the table's longest leaves occur
    t11 = Z.HufTable.for_content(_skewed(rng, 3000, 40), 11, span=129)
    deep = [s for s, (_, nb) in t11.code.items() if nb == 11]
    assert len(deep) >= 2
    # 1-bit codes throughout
    t1 = Z.HufTable([1, 1])
    for j in range(24):
        m = bytes(rng.choice(deep, 3000 + 16 * j + j).astype(np.uint8))
        chunks.append(Chunk(rng, 2 * j + 6 * (j % 5), m, huf4_frame(quarters(m), t11)))
    for j in range(24):
        m = bytes(rng.integers(0, 2, 3000 + 17 * j, dtype=np.uint8))
        chunks.append(Chunk(rng, 2 * j + 6 * (j % 5), m, huf4_frame(quarters(m), t1)))
    # the last stream one bit short / one bit long (1-bit codes: a symbol is a bit)
    for j in range(24):
        m = bytes(rng.integers(0, 2, 1200 + 4 * j, dtype=np.uint8))
        p = quarters(m)
        p[3] = p[3][:-1] if j % 2 else p[3] + b"\x01"
        chunks.append(Chunk(rng, 2 * j, m, huf4_frame(p, t1, n=len(m))))
    st = check(dcodec, chunks)
    assert st[:48] == [0] * 48
    assert all(s != 0 for s in st[48:]), st[48:]


# ---- both trip bodies -------------------------------------------------------------------------------------
def _long(rng, count, rs_of):
    out = []
    for i in range(count):
        m = _skewed(rng, rs_of(i))
        out.append(Chunk(rng, 2 * ((11 * i) % 64), m, _m_frame(rng, m)))
    return out


def test_equal_lengths_in_a_wave(dcodec):
    assert check(dcodec, _long(np.random.default_rng(8), 80, lambda i: 6000)) == [0] * 80


def test_one_frame_a_quarter_of_the_others(dcodec):
    assert check(dcodec, _long(np.random.default_rng(9), 80, lambda i: 1500 if i in (5, 20, 70) else 6000)) == [0] * 80


def test_fewer_chunks_than_a_wave_holds(dcodec):
    """a pass of 7 chunks (the second of 96 + 7: batches of up to 64 chunks take the cooperative decoder
    instead), so 36 lanes of its waves hold no job"""
    assert check(dcodec, _long(np.random.default_rng(10), 103, lambda i: 2500 + 100 * (i % 7))) == [0] * 103
