"""The full-step loops of the C5 split and of the Huffman bit packing issue a fixed sequence of
memory operations per step.  Split: every lane stores one S and one M block (the lanes past the
completed blocks store the window's open block at the stream's end, inside the slot's scratch), the
sample prefetch of the last full step is clamped, and the loop is primed with stores that its first
step repeats.  Bit packing: two 16-byte stores per lane, the lanes past the last complete 16 bytes
repeat them, up to 15 complete bytes wait for the next step.  None of that may change a byte: blobs
equal the CPU oracle's, samples equal the input, and nothing outside a blob or a chunk's samples is
written.  The merge is exercised at the same shapes (its code is the decode half of every check).

Shapes: chunk lengths around the 16-sample lane and the 1,024-sample step (no full step, one, the
last full step before a ragged one, several); 4,096-sample chunks built to drive each stream window
to its extremes; chunks whose M stream drives the bit packing.  Every batch holds more than 64
chunks, so the staged kernels (enc_chunk_kernel, dec_merge_kernel) run; one test takes the
small-batch range merge.

The bit packing's full steps.  A full step needs a literals segment of 1,024 bytes or more, that is a
four-stream Huffman section of 4,096 literals or more after the match search has taken its share.
The two 4,096-byte M streams the issue names (two symbols; mostly 11-bit codes) do not get there: the
search consumes a two-symbol stream (91 literals are left) and leaves 2,033 of the other, so both take
only the ragged step's dword stores.  They stay, as the issue sets them, and three 63,000-byte M
streams are added whose frames are checked on the CPU (test_bit_packing_cases_reach_full_steps):
  * huf_high_step: 16 common symbols and, ending at the second segment's end, 3,000 bytes of the other
    240: that segment's first full step is all long codes, more than 64 quads, so the second store's
    own quads (64 .. 87) are written;
  * huf_low_step: four equally likely symbols, the smallest alphabet whose literals still fill
    segments of 1,024 (about 2 bits per symbol, 16 quads a step).  The minimum of 8 quads (1-bit
    codes) cannot be reached through compress_batch: a two-symbol stream's literals never fill a
    segment (770 of 63,000 bytes, 1,055 with three symbols);
  * synth_read data runs in between (about 52 quads).
"""
import numpy as np
import pytest

import _oracle as O
from test_gpu_decode_pa import BITS, SENTINEL, Batch, assert_bits, decode, dev, encode, tdtype

pytestmark = pytest.mark.gpu

STEP = 1024
LENGTHS = [1, 15, 16, 17, 1023, 1024, 1025, 2047, 2048, 2049, 3 * STEP + 17, 5 * STEP]
# more full steps: exactly four, four and a ragged one, eight with a ragged one, six and the longest
# ragged one; forty, whose literals segments take several full bit-packing steps each
MORE_LENGTHS = [4 * STEP, 4 * STEP + 1, 8 * STEP + 5, 6 * STEP + 1023, 40 * STEP + 77]
BLOB_SENTINEL = 0xA5
SAMPLE_SENTINEL = 0x5EAD


def _from_deltas(d):
    """int16 samples whose 16-bit deltas (from 0) are d."""
    return np.cumsum(np.asarray(d, np.int64)).astype(np.uint16).view(np.int16)


def _from_m_bytes(b):
    """Samples that are all class 2 with the M stream b (C5 stores zig-zag(delta) - 17 there)."""
    v = np.frombuffer(bytes(b), np.uint8).astype(np.int64) + 17
    return _from_deltas(np.where(v & 1, -((v + 1) >> 1), v >> 1))


def hand_built():
    """name -> samples: 4,096 (four full steps) for the windows' extremes, others as noted."""
    n = 4 * STEP
    alt = np.where(np.arange(n) % 2 == 0, 1, -1)
    c = {}
    c["zeros"] = np.zeros(n, np.int16)  # no S / M / L block in any step
    c["class1"] = _from_deltas(alt)     # 1,024 nibbles a step: 32 S blocks
    # step 0 leaves 15 M bytes; steps 1..3 are all class 2: fill 15 + 1,024, 64 blocks, 15 carried
    d = 50 * alt
    d[15:STEP] = 0
    c["class2_carry15"] = _from_deltas(d)
    c["class2"] = _from_deltas(50 * alt)
    c["class3"] = _from_deltas(1000 * alt)  # L and H 64 blocks a step; the 10-bit count field wraps
    d = np.zeros(n, np.int64)
    d[STEP + 333] = 50  # step 0 all zero, step 1 one class-2 sample (no block, one carried byte), then zeros
    c["one_class2"] = _from_deltas(d)
    c["alternating"] = _from_deltas(np.tile([0, 1, 50, 1000, 0, -1, -50, -1000], n // 8))
    rng = np.random.default_rng(20261020)
    # Huffman extremes as M streams: two symbols (1-bit codes); one common symbol and 255 rare ones
    c["huf_two_symbols"] = _from_m_bytes(rng.integers(0, 2, n, dtype=np.uint8) * 0x5B + 0x11)
    skew = np.where(rng.random(n) < 0.7, 0, rng.integers(1, 256, n)).astype(np.uint8)
    c["huf_11_bits"] = _from_m_bytes(skew)
    # a few class-3 samples in a short chunk: Llow / Lhigh of 7 .. 63 bytes without a match become raw
    # blocks, and Lhigh's frame ends the blob (the frame writer's "no sequences" byte lay past it)
    d = np.zeros(600, np.int64)
    d[40:600:56] = [300, -700, 1100, -1500, 1900, -2300, 2700, -3100, 3500, -3900]
    c["few_class3"] = _from_deltas(d)
    c.update(bit_packing_cases())
    return c


HUF_N = 63_000        # M bytes of the bit-packing cases: one zstd block, four segments of 15,750
HUF_RARE = (29_000, 32_000)  # the long-code stretch; segment 1 is [15,750, 31,500)


def bit_packing_cases():
    """name -> samples whose M stream (63,000 bytes) gives full bit-packing steps at an extreme."""
    rng = np.random.default_rng(7)
    common = rng.choice(256, 16, replace=False)
    rare = np.setdiff1d(np.arange(256), common)
    m = common[rng.integers(0, 16, HUF_N)].astype(np.uint8)
    m[HUF_RARE[0]:HUF_RARE[1]] = rare[rng.integers(0, rare.size, HUF_RARE[1] - HUF_RARE[0])]
    low = np.random.default_rng(1).integers(0, 4, HUF_N).astype(np.uint8)  # (which bytes are matched depends on the values)
    return {"huf_high_step": _from_m_bytes(m), "huf_low_step": _from_m_bytes(low)}


def literals_section(frame):
    """Of a frame of one compressed block: (streams, regenerated size, compressed size, the four
    streams' sizes) of its Huffman literals section (RFC 8878 3.1.1.3.1)."""
    assert frame[:4] == bytes.fromhex("28b52ffd")
    fhd = frame[4]
    single, fcs = (fhd >> 5) & 1, fhd >> 6
    assert fhd & 3 == 0, "no dictionary id"
    p = 5 + (0 if single else 1) + (single if fcs == 0 else (2, 4, 8)[fcs - 1])
    bh = int.from_bytes(frame[p:p + 3], "little")
    assert (bh >> 1) & 3 == 2 and bh & 1, "one compressed block, the last"
    p += 3
    assert frame[p] & 3 == 2, "a Huffman literals section with its table"
    sf = (frame[p] >> 2) & 3
    nb, bits = {0: (3, 10), 1: (3, 10), 2: (4, 14), 3: (5, 18)}[sf]
    v = int.from_bytes(frame[p:p + nb], "little") >> 4
    regen, comp = v & ((1 << bits) - 1), v >> bits
    if sf == 0:
        return 1, regen, comp, None
    # table description, then the jump table of the first three streams' sizes
    q = p + nb
    hb = frame[q]
    q += 1 + (hb if hb < 128 else (hb - 127 + 1) // 2)
    s3 = [int.from_bytes(frame[q + 2 * k:q + 2 * k + 2], "little") for k in range(3)]
    return 4, regen, comp, s3 + [p + nb + comp - (q + 6) - sum(s3)]


class Cases:
    """The chunks, their oracle blobs and oracle decodes, computed once."""

    def __init__(self, variant):
        self.variant = variant
        built = hand_built()
        self.names = [f"n{n}" for n in LENGTHS + MORE_LENGTHS] + list(built)
        chunks = [O.synth_read(700 + r, n) for r, n in enumerate(LENGTHS + MORE_LENGTHS)] + list(built.values())
        while len(chunks) < 70:  # above the small-batch threshold of 64 chunks
            self.names.append(f"fill{len(chunks)}")
            chunks.append(O.synth_read(800 + len(chunks), 300 + 7 * len(chunks)))
        self.b = Batch(chunks)
        self.blobs = []
        for name, x in zip(self.names, chunks):
            rc, blob, _ = O.c5_compress(x) if variant == "C5" else O.variant_compress(variant, x)
            assert rc == 0, f"{variant} {name}: the oracle does not support this input (status {rc})"
            rc, back = O.c5_decompress(blob, x.size) if variant == "C5" else O.variant_decompress(variant, blob, x.size)[:2]
            assert rc == 0 and np.array_equal(back, x), f"{variant} {name}: oracle round trip"
            self.blobs.append(blob)


_cases = {}


def cases(variant):
    if variant not in _cases:
        _cases[variant] = Cases(variant)
    return _cases[variant]


@pytest.fixture(scope="module")
def codecs():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rawnanoporesignalcompression_amd import PGNanoCodec

    made = {}

    def get(name):
        if name not in made:
            made[name] = PGNanoCodec(0, variant=name)
        return made[name]

    yield get
    for c in made.values():
        c.close()


def test_hand_built_inputs_reach_their_extremes():
    """The stream sizes the oracle reports are the ones the cases are built for (sizes[0..4]: the raw
    keys / S / M / Llow / Lhigh bytes)."""
    built = hand_built()
    raw = {k: [len(s) for s in O.c5_streams(x)] for k, x in built.items()}
    n = 4 * STEP
    assert raw["zeros"] == [n // 4, 0, 0, 0, 0]
    assert raw["class1"] == [n // 4, n // 2, 0, 0, 0]
    assert raw["class2"] == [n // 4, 0, n, 0, 0]
    assert raw["class2_carry15"] == [n // 4, 0, 15 + 3 * STEP, 0, 0]
    assert raw["class3"] == [n // 4, 0, 0, n, n]
    assert raw["one_class2"] == [n // 4, 0, 1, 0, 0]
    assert raw["alternating"] == [n // 4, n // 8, n // 4, n // 4, n // 4]
    assert raw["huf_two_symbols"][2] == n and raw["huf_11_bits"][2] == n
    m = np.frombuffer(O.c5_streams(built["huf_two_symbols"])[2], np.uint8)
    assert np.unique(m).size == 2
    m = np.frombuffer(O.c5_streams(built["huf_11_bits"])[2], np.uint8)
    assert np.unique(m).size > 200 and (m == 0).mean() > 0.6
    assert raw["few_class3"] == [150, 0, 0, 10, 10]


def test_bit_packing_cases_reach_full_steps():
    """What zstd makes of the bit-packing cases, from the oracle's M frames (CPU only): four-stream
    Huffman sections whose segments hold several full steps, the long-code stretch filling a whole
    step with more than 64 quads, the low case near 2 bits per symbol; and the issue's two 4,096-byte
    cases, which leave no full step."""
    built = hand_built()
    frame = {k: O.zstd_compress1(O.c5_streams(built[k])[2]) for k in built if k.startswith("huf_")}
    assert literals_section(frame["huf_two_symbols"])[:2] == (1, 91)
    streams, regen, _, _ = literals_section(frame["huf_11_bits"])
    assert streams == 4 and regen < 4 * STEP  # segments below 1,024: the ragged step only
    # high: no byte is matched, so literal i is M byte i and the segments are [15,750 k, 15,750 (k + 1))
    streams, regen, comp, sizes = literals_section(frame["huf_high_step"])
    assert (streams, regen) == (4, HUF_N)
    seg = (regen + 3) // 4
    assert HUF_RARE[0] <= 2 * seg - STEP and 2 * seg <= HUF_RARE[1]  # segment 1's first step (its last 1,024 bytes)
    # bits per long code from the segments' sizes: segment 0 is all common symbols, segment 1 has
    # 2 seg - HUF_RARE[0] long codes and common ones before them
    n_rare = 2 * seg - HUF_RARE[0]
    per_common = 8 * sizes[0] / seg
    per_rare = (8 * sizes[1] - per_common * (seg - n_rare)) / n_rare
    print(f"huf_high_step: {per_common:.2f} bits per common symbol, {per_rare:.2f} per rare one, "
          f"{STEP * per_rare / 128:.1f} quads in the all-rare step")
    assert STEP * per_rare / 128 > 80  # of at most 88; the second store's own quads start at 64
    # low: segments of 1,024 or more, about 2 bits per symbol
    streams, regen, comp, sizes = literals_section(frame["huf_low_step"])
    assert streams == 4 and regen >= 4 * STEP
    print(f"huf_low_step: {regen} literals, {8 * sum(sizes) / regen:.2f} bits per symbol")
    assert 8 * sum(sizes) / regen < 2.2


@pytest.mark.parametrize("variant", ["C5", "C4"])
def test_blobs_equal_the_oracle_and_stay_inside(codecs, variant):
    """Blobs at odd byte offsets in a buffer filled with a sentinel: sizes and bytes are the oracle's and
    every byte outside a blob keeps the sentinel (no store of the bit packing past a blob's size, none
    of the split's open-block or priming stores in caller memory)."""
    import torch

    from rawnanoporesignalcompression_amd.codec import compressed_signal_max_size

    cs = cases(variant)
    b = cs.b
    caps = np.array([compressed_signal_max_size(int(n)) for n in b.counts], np.int64)
    starts, pos = [], 13
    for i, cap in enumerate(caps.tolist()):
        starts.append(pos)
        pos += cap + 5 + (i % 7)
    total = pos + 64
    out = torch.full((total,), BLOB_SENTINEL, dtype=torch.uint8, device="cuda:0")
    enc = codecs(variant).compress_batch(dev(b.flat), dev(b.offsets), dev(b.counts), out=out,
                                         out_offsets=dev(np.array(starts, np.int64)), out_caps=dev(caps))
    st, sizes, got = enc.status.cpu().numpy(), enc.sizes.cpu().numpy(), out.cpu().numpy()
    assert (st == 0).all(), st
    inside = np.zeros(total, bool)
    for i, (s, blob) in enumerate(zip(starts, cs.blobs)):
        assert sizes[i] == len(blob), f"{cs.names[i]}: size {sizes[i]}, oracle {len(blob)}"
        assert got[s:s + len(blob)].tobytes() == blob, f"{cs.names[i]}: blob differs from the oracle's"
        inside[s:s + len(blob)] = True
    assert (got[~inside] == BLOB_SENTINEL).all(), np.flatnonzero(~inside & (got != BLOB_SENTINEL))[:8]


def _placed(counts, shift):
    """Chunk starts congruent to `shift` samples modulo 8 (16 bytes of int16), 8+ samples apart."""
    starts, pos = [], 8
    for n in counts:
        s = pos + (shift - pos) % 8
        starts.append(s)
        pos = s + n + 8
    return starts, pos + 64


@pytest.mark.parametrize("shift", [0, 1, 3, 8])
@pytest.mark.parametrize("variant", ["C5", "C4"])
def test_samples_equal_and_stay_inside(codecs, variant, shift):
    """The oracle's blobs decoded to destinations at 0, 1, 3 and 8 samples modulo 8 (16-byte aligned:
    non-temporal stores; otherwise plain ones) in a buffer filled with a sentinel: samples equal,
    every element outside a chunk untouched."""
    import torch

    cs = cases(variant)
    b = cs.b
    starts, total = _placed(b.counts.tolist(), shift)
    out = torch.full((total,), SAMPLE_SENTINEL, dtype=torch.int16, device="cuda:0")
    sizes = np.array([len(x) for x in cs.blobs], np.int64)
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    flat = dev(np.frombuffer(b"".join(cs.blobs), np.uint8))
    got, _, st = codecs(variant).decompress_batch(flat, dev(offs), dev(sizes), dev(b.counts), out=out,
                                                  out_offsets=dev(np.array(starts, np.int64)))
    got, st = got.cpu().numpy(), st.cpu().numpy()
    assert (st == 0).all(), st
    inside = np.zeros(total, bool)
    for i, (s, n) in enumerate(zip(starts, b.counts.tolist())):
        assert np.array_equal(got[s:s + n], b.chunks[i]), f"{cs.names[i]} at {s}"
        inside[s:s + n] = True
    assert (got[~inside] == SAMPLE_SENTINEL).all(), np.flatnonzero(~inside & (got != SAMPLE_SENTINEL))[:8]


@pytest.mark.parametrize("dtype", ["float32", "float16"])
@pytest.mark.parametrize("shift", [0, 1])
def test_float_outputs(codecs, dtype, shift):
    """The calibrated outputs share the merge loop (float32: four plain stores per lane; float16: the
    int16 output's two): the 1,025- and 2,049-sample chunks and the longer ones, at element offsets 0
    and 1 modulo 8, bit for bit against the reference computation, sentinel outside."""
    import torch

    cs = cases("C5")
    b = cs.b
    for n in (1025, 2049, 4 * STEP, 8 * STEP + 5):
        assert f"n{n}" in cs.names
    starts, total = _placed(b.counts.tolist(), shift)
    out = torch.empty(total, dtype=tdtype(dtype), device="cuda:0")
    sent = SENTINEL[dtype]
    out.view(torch.int32 if dtype == "float32" else torch.int16).fill_(sent)
    codec = codecs("C5")
    got, _, st = decode(codec, encode(codec, b), b, dtype, out=out, out_offsets=dev(np.array(starts, np.int64)))
    assert (st == 0).all(), st
    inside = np.zeros(total, bool)
    for i, (s, n) in enumerate(zip(starts, b.counts.tolist())):
        assert_bits(got[s:s + n], b.chunk_ref(i, dtype), dtype, f"{cs.names[i]} at {s}")
        inside[s:s + n] = True
    bits = got.view(BITS[dtype])
    assert (bits[~inside] == sent).all(), np.flatnonzero(bits[~inside] != sent)[:8]


@pytest.mark.parametrize("shift", [0, 3])
def test_small_batch_ranges_of_eight_steps(codecs, shift):
    """Three chunks take the cooperative encode and the range merge, where the waves of a workgroup
    (encode) or single-wave workgroups (merge) share a chunk: 262,144 samples give every merge range
    eight full steps and every literals segment several full bit-packing steps."""
    import torch

    xs = [O.synth_read(901, 262_144), O.synth_read(902, 5 * STEP), O.synth_read(903, 1)]
    b = Batch(xs)
    starts, total = _placed(b.counts.tolist(), shift)
    out = torch.full((total,), SAMPLE_SENTINEL, dtype=torch.int16, device="cuda:0")
    codec = codecs("C5")
    enc = encode(codec, b)
    blobs, bo, bs = enc.blobs.cpu().numpy(), enc.offsets.cpu().numpy(), enc.sizes.cpu().numpy()
    for i, x in enumerate(xs):
        assert blobs[bo[i]:bo[i] + bs[i]].tobytes() == O.c5_compress(x)[1], f"chunk {i}: blob differs from the oracle's"
    got, _, st = codec.decompress_batch(enc.blobs, enc.offsets, enc.sizes, dev(b.counts), out=out,
                                        out_offsets=dev(np.array(starts, np.int64)))
    got, st = got.cpu().numpy(), st.cpu().numpy()
    assert (st == 0).all(), st
    inside = np.zeros(total, bool)
    for i, (s, n) in enumerate(zip(starts, b.counts.tolist())):
        assert np.array_equal(got[s:s + n], xs[i]), f"chunk {i} at {s}"
        inside[s:s + n] = True
    assert (got[~inside] == SAMPLE_SENTINEL).all()
