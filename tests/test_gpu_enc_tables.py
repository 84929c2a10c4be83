"""The encoder's entropy-table stage against the oracle, byte for byte: the Huffman table description
(weight FSE chains, its raw and rejected forms, sections that land just on either side of "compressed")
and the sequences section (one batch of up to 64 sequences, more, and the extra-bits codes).

Every case is a byte stream of at most 4,096 bytes carried as the M stream of a C5 chunk: a signal whose
deltas all fall in class 2 (zig-zag value = byte + 17), so the chunk's M frame is
ZSTD_compress(stream, 1) and the other frames are trivial.  All chunks go through the batched encode
(one wave per chunk) and again in batches of 64 (the cooperative workgroup encode); the blobs must
equal the oracle's c5_compress, whose M frame must equal zstd_compress1 of the stream.  What a case is
meant to reach is checked on the oracle's frame (and on the host model's sequences), not on the GPU's.
Needs an MI355X."""
import ctypes as C
import functools

import numpy as np
import pytest

import _oracle as O

pytestmark = pytest.mark.gpu

MAXN = 4096


# ---- streams as chunks ---------------------------------------------------------------------------
def m_signal(stream: bytes) -> np.ndarray:
    """The int16 signal whose C5 M stream is `stream`."""
    v = np.frombuffer(stream, np.uint8).astype(np.int64) + 17
    d = np.where(v & 1, -((v + 1) >> 1), v >> 1)  # inverse zig-zag
    return (np.cumsum(d) & 0xFFFF).astype(np.uint16).view(np.int16)


# ---- the oracle's frame, as far as the cases need it -----------------------------------------------
def frame_info(frame: bytes) -> dict:
    """First block of a single-segment frame: block type, literals type / sizes, the Huffman
    description's header byte, the number of sequences."""
    assert frame[:4] == b"\x28\xb5\x2f\xfd"
    fhd = frame[4]
    assert fhd & 0x20 and not fhd & 3, "single segment, no dictionary"
    p = 5 + (1, 2, 4, 8)[fhd >> 6]
    bh = int.from_bytes(frame[p:p + 3], "little")
    p += 3
    info = {"block": (bh >> 1) & 3, "last": bh & 1}
    if info["block"] != 2:
        return info
    b0 = frame[p]
    lt, sf = b0 & 3, (b0 >> 2) & 3
    if lt < 2:
        hl = (1, 2, 1, 3)[sf]
        regen = int.from_bytes(frame[p:p + hl], "little") >> (3 if hl == 1 else 4)
        csize = regen if lt == 0 else 1
    else:
        hl = (3, 3, 4, 5)[sf]
        v = int.from_bytes(frame[p:p + hl], "little") >> 4
        bits = (10, 10, 14, 18)[sf]
        regen, csize = v & ((1 << bits) - 1), v >> bits
        info["streams"] = 1 if sf == 0 else 4
        info["hbyte"] = frame[p + hl]
    info.update(lit=lt, regen=regen, csize=csize)
    q = p + hl + csize
    nb = frame[q]
    if nb >= 128:
        nb = ((nb - 128) << 8) + frame[q + 1] if nb < 255 else frame[q + 1] + (frame[q + 2] << 8) + 0x7F00
    info["nbseq"] = nb
    if 0 < nb < 128:  # the LL, OF, ML table modes: 0 predefined, 1 RLE, 2 compressed
        info["modes"] = tuple((frame[q + 1] >> sh) & 3 for sh in (6, 4, 2))
    return info


def m_frame(stream: bytes) -> bytes:
    return O.zstd_compress1(stream)


def model_sequences(stream: bytes):
    """(litLength, offset value, matchLength - 3) of the level-1 search, from the host model."""
    M = O.model()
    a = np.frombuffer(stream, np.uint8).copy()
    out = np.zeros(3 * (len(stream) // 4 + 2), np.uint32)
    M.z1m_sequences.restype = C.c_size_t
    M.z1m_sequences.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    nb = M.z1m_sequences(a.ctypes.data, a.size, out.ctypes.data, out.size // 3)
    return out[: 3 * nb].reshape(-1, 3)


# ---- generators ------------------------------------------------------------------------------------
def skewed(rng, n, syms, ratio):
    """n bytes over `syms`, probabilities falling by `ratio` per symbol, every symbol present."""
    syms = np.asarray(syms)
    p = ratio ** np.arange(syms.size)
    out = syms[rng.choice(syms.size, n, p=p / p.sum())]
    where = rng.permutation(n)[: syms.size]
    out[where] = syms
    return out.astype(np.uint8).tobytes()


def dyadic(rng, lengths, scale):
    """Symbol i exactly scale * 2^(maxlen - lengths[i]) times, shuffled: Huffman lengths = `lengths`
    (a complete code), weights in the order given."""
    mx = max(lengths)
    s = np.concatenate([np.full(scale << (mx - l), i, np.uint8) for i, l in enumerate(lengths)])
    assert s.size <= MAXN
    return rng.permutation(s).tobytes()


def with_repeats(rng, n, k, mlen=8, base_syms=256, ratio=0.995, dmin=None, dmax=64):
    """Near-random bytes with k planted copies of earlier bytes (mlen bytes from dmin .. dmax - 1 back),
    evenly spaced."""
    s = bytearray(skewed(rng, n, np.arange(base_syms), ratio))
    gap = (n - 80) // max(k, 1)
    assert gap >= mlen + 6
    for j in range(k):
        p = 72 + j * gap
        d = int(rng.integers(dmin or mlen, dmax))
        s[p:p + mlen] = s[p - d:p - d + mlen]
    return bytes(s)


def search(make, want, tries=400):
    """First stream of make(seed) for which want(stream) holds."""
    for seed in range(tries):
        s = make(np.random.default_rng(1000 + seed))
        if want(s):
            return s
    raise AssertionError("no seed gives the case")


def lit_kind(stream: bytes) -> str:
    """How the oracle codes the literals of the stream's (single) block."""
    i = frame_info(m_frame(stream))
    if i["block"] != 2:
        return ("raw", "rle")[i["block"]]
    return ("raw", "rle", "huf", "repeat")[i["lit"]]


def boundary_pair(rng, n, nsym):
    """Two streams one byte apart (and three further off) where the oracle's literals go from raw to
    Huffman: the section misses its gain by the narrowest margin on one side and makes it on the other.  Bytes
    of an incompressible stream are replaced by symbol 0 one at a time; bisection keeps a raw stream
    below a compressed one until they are neighbours."""
    order = rng.permutation(n)
    for top in (nsym, 256):  # the alphabet asked for, unless its uniform stream already compresses
        base = np.frombuffer(skewed(rng, n, np.arange(top), 1.0), np.uint8)

        def at(t):
            s = base.copy()
            s[order[:t]] = 0
            return s.tobytes()

        if lit_kind(at(0)) == "raw":
            break
    lo = 0
    hi = next(t for t in range(n // 32, n, n // 32) if lit_kind(at(t)) == "huf")
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if lit_kind(at(mid)) == "huf":
            hi = mid
        else:
            lo = mid
    return at(lo), at(hi), [at(max(lo - back, 0)) for back in (30, 100, 300)]


@functools.lru_cache(maxsize=None)
def cases():
    """name -> stream, in groups (the name's prefix)."""
    rng = np.random.default_rng(20240)
    c = {}
    # -- by weight count: the alphabet 0 .. N-1 (N symbols, N - 1 weights) and 0 .. N (N weights)
    for N in (2, 3, 4, 127, 128, 129, 255, 256):
        for syms in (N, N + 1):
            if syms > 256:
                continue
            ratio = 0.5 if syms <= 5 else (0.95 if syms <= 130 else 0.97)
            c[f"weights/{N}_alphabet{syms}"] = skewed(rng, MAXN if syms > 5 else 600, np.arange(syms), ratio)
    # -- by chain length: emissions = weights - 2, odd and even, short and across the 64-lane groups
    for wts in (3, 4, 5, 40, 41, 65, 66, 67, 130, 131, 193, 194, 195, 254, 255):
        c[f"chain/{wts}_weights"] = skewed(rng, MAXN, np.arange(wts + 1), 0.96 if wts > 100 else 0.9)
    # -- raw 4-bit weights: every weight value once or twice, so FSE cannot gain
    c["rawweights/distinct"] = dyadic(rng, [1, 2, 3, 4, 5, 6, 7, 8, 9, 9], 4)
    c["rawweights/distinct_short"] = dyadic(rng, [1, 2, 3, 4, 4], 40)
    # -- one weight value only (hSize == 1): equal lengths
    for k in (2, 3, 4, 5, 6):
        c[f"oneweight/{1 << k}_symbols"] = dyadic(rng, [k] * (1 << k), MAXN >> k >> 1)
    # -- the FSE form tried and rejected (hSize >= maxSym / 2): weight values in pairs
    c["rejected/pairs16"] = dyadic(rng, [2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 8, 8], 8)
    c["rejected/pairs10"] = dyadic(rng, [2, 2, 3, 3, 4, 4, 5, 5, 5, 5], 60)
    c["rejected/pairs12"] = dyadic(rng, [1, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 7, 7], 16)
    # -- sections just raw and just compressed
    for j, (n, nsym) in enumerate([(300, 120), (700, 200), (1150, 222), (1150, 216), (1200, 256), (2000, 256),
                                   (4096, 256), (4096, 129), (900, 128), (640, 100), (1500, 240), (3000, 255)]):
        a, b, further = boundary_pair(rng, n, nsym)
        c[f"boundary/{j}_n{n}_raw"] = a
        c[f"boundary/{j}_n{n}_huf"] = b
        for k, s in enumerate(further):  # raw by a wider margin: the description's bounds can decide it early
            c[f"boundary/{j}_n{n}_further{k}_raw"] = s
    # hSize + 12 >= n: a wide sparse alphabet in a stream a little over the 63-byte minimum (the section is
    # raw on this side only: with the streams' >= 9 bytes the gain check fails wherever this one does)
    for j, n in enumerate((64, 66, 70, 76, 84, 96, 120)):
        syms = np.sort(rng.permutation(256)[: n - 8])
        s = np.concatenate([syms, np.full(8, syms[0])])
        c[f"tiny/{j}_n{n}"] = rng.permutation(s).astype(np.uint8).tobytes()
    # -- sequences: exact counts around the one-batch limit
    for k in (1, 2, 63, 64, 65, 127):
        n = 600 if k <= 2 else MAXN
        c[f"seq/{k}"] = search(lambda r, n=n, k=k: with_repeats(r, n, k, mlen=40 if k <= 2 else 8), lambda s, k=k: frame_info(m_frame(s)).get("nbseq") == k)
        c[f"seq/{k}_huf_literals"] = search(lambda r, n=n, k=k: with_repeats(r, n, k, base_syms=64, ratio=0.93),
                                            lambda s, k=k: frame_info(m_frame(s)).get("nbseq") == k)
    # 36 .. 64 sequences take the one-batch path only when every offset has the same code (an RLE table: with
    # more codes the offsets' table is compressed and the general path runs, as in seq/63 and seq/64 above)
    for k in (36, 63, 64):
        c[f"seq/{k}_one_offset_code"] = search(
            lambda r, k=k: with_repeats(r, MAXN, k, dmin=29, dmax=61),
            lambda s, k=k: (lambda i: i.get("nbseq") == k and i["modes"][1] == 1)(frame_info(m_frame(s))))
    # -- long lengths: literal runs >= 64 and matches >= 131 (the extra-bits codes)
    def long_lengths(r, n_copies, ml):
        s = bytearray(skewed(r, MAXN, np.arange(256), 0.995))
        p = ml + 400
        for _ in range(n_copies):
            m = int(r.integers(ml, ml + 300))
            d = int(r.integers(m, p + 1))
            s[p:p + m] = s[p - d:p - d + m]
            p += m + int(r.integers(64, 500))
            if p + ml + 300 > MAXN:
                break
        return bytes(s)

    for j, (copies, ml) in enumerate([(1, 131), (3, 131), (6, 140), (2, 1000)]):
        c[f"long/{j}"] = search(lambda r, copies=copies, ml=ml: long_lengths(r, copies, ml), lambda s: True)
    return c


@functools.lru_cache(maxsize=None)
def reference():
    """name -> (signal, the oracle's blob, frame_info of the M frame); computed once."""
    ref = {}
    for name, s in cases().items():
        assert 0 < len(s) <= MAXN, name
        x = m_signal(s)
        assert O.c5_streams(x)[2] == s, name
        rc, blob, st = O.c5_compress(x)
        assert rc == 0, name
        fr = m_frame(s)
        assert int(st[7]) == len(fr), name
        k = 8 + int(st[5]) + 8 + int(st[6]) + 8
        assert blob[k:k + len(fr)] == fr, name
        ref[name] = (x, blob, frame_info(fr))
    return ref


@pytest.fixture(scope="module")
def encoded(codec):
    """name -> the GPU's blob from one batch of all chunks, and -> its blob from batches of 64."""
    import torch

    ref = reference()
    names = list(ref)
    xs = [ref[n][0] for n in names]
    lens = np.array([x.size for x in xs], np.int32)
    dev = torch.device("cuda", 0)
    samples = torch.from_numpy(np.concatenate(xs)).to(dev)
    counts = torch.from_numpy(lens).to(dev)
    offs = torch.from_numpy(np.concatenate([[0], np.cumsum(lens.astype(np.int64))[:-1]])).to(dev)
    assert len(names) > 64

    def run(a, b):
        e = codec.compress_batch(samples, offs[a:b], counts[a:b])
        torch.cuda.synchronize()
        assert (e.status.cpu().numpy() == 0).all()
        eb, eo, es = e.blobs.cpu().numpy(), e.offsets.cpu().numpy(), e.sizes.cpu().numpy()
        return [eb[eo[i]:eo[i] + es[i]].tobytes() for i in range(b - a)]

    whole = dict(zip(names, run(0, len(names))))
    small = {}
    for a in range(0, len(names), 64):
        b = min(a + 64, len(names))
        small.update(zip(names[a:b], run(a, b)))
    return whole, small


def group(prefix):
    return [n for n in cases() if n.startswith(prefix + "/")]


def check(encoded, names):
    whole, small = encoded
    ref = reference()
    assert names
    for n in names:
        assert whole[n] == ref[n][1], f"{n}: one wave per chunk"
        assert small[n] == ref[n][1], f"{n}: cooperative encode"


def test_weight_counts(encoded):
    """Alphabets of exactly 2, 3, 4, 127, 128, 129, 255 and 256 symbols, and of as many weights."""
    names = group("weights")
    ref = reference()
    for n in names:
        if int(n.split("alphabet")[1]) >= 100:
            assert ref[n][2].get("lit") == 2 and ref[n][2]["hbyte"] < 128, n  # Huffman, FSE description
    check(encoded, names)


def test_chain_lengths(encoded):
    """Odd and even counts of weight-FSE emissions, from 1 to 253."""
    names = group("chain")
    ref = reference()
    for n in names:
        assert ref[n][2].get("lit") == 2, n
        if int(n.split("/")[1].split("_")[0]) >= 65:
            assert ref[n][2]["hbyte"] < 128, n  # the FSE form
    check(encoded, names)


def test_raw_weights(encoded):
    names = group("rawweights")
    ref = reference()
    for n in names:
        assert ref[n][2].get("lit") == 2 and ref[n][2]["hbyte"] >= 128, n
    check(encoded, names)


def test_one_weight_value(encoded):
    """All weights equal: HUF_compressWeights returns 1, the description is the raw form."""
    names = group("oneweight")
    ref = reference()
    for n in names:
        assert ref[n][2].get("lit") == 2 and ref[n][2]["hbyte"] >= 128, n
    check(encoded, names)


def test_fse_form_rejected(encoded):
    """Repeated weight values, so the FSE form is tried, over so few symbols that it is rejected."""
    names = group("rejected")
    ref = reference()
    for n in names:
        assert ref[n][2].get("lit") == 2 and ref[n][2]["hbyte"] >= 128, n
    check(encoded, names)


def test_sections_just_raw_and_just_compressed(encoded):
    """Around hSize + cStreams == n - minGain: twelve seeded bisections, the neighbours on either side and
    three raw streams further off (where the description's bounds decide before its chains run)."""
    names = group("boundary")
    ref = reference()
    for n in names:
        i = ref[n][2]
        if n.endswith("_raw"):
            assert i["block"] == 0 or i["lit"] == 0, n
        else:
            assert i["block"] == 2 and i["lit"] == 2, n
    assert len(names) == 60
    check(encoded, names)


def test_tiny_sections(encoded):
    """Around hSize + 12 == n: wide sparse alphabets in 64 .. 120 bytes.  Only the raw side exists: the
    streams take at least 9 bytes, so hSize + cStreams >= n - minGain fails wherever hSize + 12 >= n does."""
    names = group("tiny")
    ref = reference()
    for n in names:
        assert ref[n][2]["block"] == 0 or ref[n][2]["lit"] == 0, n
    check(encoded, names)


def test_sequence_counts(encoded):
    """Exactly 1, 2, 63, 64, 65 and 127 sequences, over raw and over Huffman literals."""
    names = group("seq")
    ref = reference()
    for n in names:
        assert ref[n][2]["block"] == 2 and ref[n][2]["nbseq"] == int(n.split("/")[1].split("_")[0]), n
    assert any(ref[n][2]["lit"] == 2 for n in names) and any(ref[n][2]["lit"] == 0 for n in names)
    for n in names:  # which path the section takes: one batch unless a table is compressed or it has > 64
        k, modes = ref[n][2]["nbseq"], ref[n][2]["modes"]
        if k < 36 or n.endswith("_one_offset_code"):
            assert 2 not in modes, (n, modes)
        elif k <= 64:
            assert modes[1] == 2, (n, modes)
    check(encoded, names)


def test_long_lengths(encoded):
    """Literal lengths >= 64 and match lengths >= 131: the codes with the most extra bits."""
    names = group("long")
    for n in names:
        sq = model_sequences(cases()[n])
        assert sq.size and (sq[:, 0] >= 64).any() and (sq[:, 2] + 3 >= 131).any(), n
        assert reference()[n][2]["nbseq"] == len(sq), n
    check(encoded, names)
