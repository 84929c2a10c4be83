"""The test frame writer (_zframes.py) against libzstd, and the host build of the decoder
(zstd1_dec.h, the code the GPU kernels share) against libzstd, on frames no encoder writes.

Every named case the GPU tests decode (tests/_zframes.py catalogue) and a seeded sweep of random recipes
go through ZSTD_decompress (the oracle's pgno_zstd_decompress, whatever libzstd the oracle loaded, asked
when the test runs) and through z1m_decompress: a valid recipe must give exactly the content, a recipe
with one stated defect an error, the host model must agree in acceptance and in bytes, and the emitted
record must hold the feature the case is named for.  The differences kept on purpose
have tests of their own that pin both sides.
"""
import os

import numpy as np
import pytest

import _oracle as O
import _zframes as Z

pytestmark = pytest.mark.skipif(not os.path.exists(O.MODEL_SO), reason="libpgn_model.so not built")

GROUPS = ["huf_logs", "huf4_sizes", "hdrwin", "match", "rep", "seqtab", "seqcount", "frame", "big", "leftover",
          "defect", "weight12", "block128k"]
KNOWN = ["checksum", "overhang", "cut"]  # known divergences: their own tests below


def libzstd(stream: bytes, cap: int):
    """(accepted, bytes) from ZSTD_decompress into cap bytes."""
    a = np.frombuffer(stream, np.uint8)
    out = np.zeros(cap + 64, np.uint8)
    r = O.oracle().pgno_zstd_decompress(a.ctypes.data, a.size, out.ctypes.data, cap)
    return (True, out[:r].tobytes()) if r < (1 << 63) else (False, b"")


def model(stream: bytes, cap: int):
    a = np.frombuffer(stream, np.uint8)
    out = np.zeros(cap + 64, np.uint8)
    r = O.model().z1m_decompress(a.ctypes.data, a.size, out.ctypes.data, cap)
    return (True, out[:r].tobytes()) if r >= 0 else (False, b"")


def check(stream, content, valid, name):
    cap = len(content) + 32
    zok, zb = libzstd(stream, cap)
    mok, mb = model(stream, cap)
    if valid:
        assert zok and zb == content, f"{name}: libzstd refuses or alters a frame the recipe calls valid"
    else:
        assert not zok, f"{name}: libzstd accepts a frame whose recipe states a defect"
    assert mok == zok, f"{name}: libzstd {'accepts' if zok else 'rejects'}, the host model does not"
    assert mb == zb, f"{name}: bytes differ between libzstd and the host model"


def test_catalogue_groups_are_all_tested():
    assert {c.group for c in Z.catalogue()} == set(GROUPS) | set(KNOWN)


@pytest.mark.parametrize("group", GROUPS)
def test_named_cases_libzstd_and_model_agree(group):
    cases = [c for c in Z.catalogue() if c.group == group]
    assert cases
    for c in cases:
        check(c.stream, c.content, c.valid, c.name)
        assert c.has(c.recs), f"{c.name}: the record lacks the feature the case is named for"


def _known(group):
    (c,) = [c for c in Z.catalogue() if c.group == group]
    assert c.has(c.recs)
    return c, libzstd(c.stream, len(c.content) + 32), model(c.stream, len(c.content) + 32)


def test_known_divergence_wrong_checksum_is_accepted():
    """libzstd verifies the XXH64 trailer; this decoder skips it (the reference never writes one, and
    verifying needs a hash of the whole output).  The same frame with the right trailer is in the
    catalogue, so the writer's XXH64 is libzstd's."""
    c, z, m = _known("checksum")
    assert not z[0]
    assert m == (True, c.content)


def test_known_divergence_four_streams_of_size_5_are_rejected():
    """Four Huffman streams cannot split 1, 2 or 5 bytes (three streams of ceil(n/4) symbols pass the end).
    libzstd 1.4.x decodes such a section when its fourth stream is empty, writing one byte past the
    literals; libzstd 1.5 and this decoder call it corrupt."""
    c, z, m = _known("overhang")
    assert not m[0]
    if O.oracle().pgno_zstd_version() < 10500:
        assert z == (True, c.content)
    else:
        assert not z[0]


def test_known_divergence_cut_sequence_stream_is_rejected():
    """A sequence bitstream that ends before its sequences do: libzstd 1.4.x reads on through what its
    64-bit container holds and returns bytes; libzstd 1.5 and this decoder call it corrupt."""
    c, z, m = _known("cut")
    assert not m[0]
    if O.oracle().pgno_zstd_version() < 10500:
        assert z[0] and z[1] != c.content
    else:
        assert not z[0]


def test_xxh64_vectors():
    assert Z.xxh64(b"") == 0xEF46DB3751D8E999
    assert Z.xxh64(b"a") == 0xD24EC4F1A98C6E5B
    assert Z.xxh64(b"abc") == 0x44BC2CF5AD770999


def _content(rng, n):
    kind = int(rng.integers(0, 6))
    if kind == 0:
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    if kind == 1:
        k = int(rng.integers(1, 200))
        return rng.choice(k, n, p=rng.dirichlet(np.ones(k) * float(rng.choice([0.05, 0.3, 1, 5])))).astype(np.uint8).tobytes()
    if kind == 2:
        vals = rng.integers(0, 256, n // 10 + 2, dtype=np.uint8)
        return np.repeat(vals, rng.geometric(float(rng.choice([0.01, 0.1, 0.5])), n // 10 + 2))[:n].tobytes()
    if kind == 3:
        return bytes([int(rng.integers(0, 256))]) * n
    if kind == 4:
        p = rng.integers(0, 60, int(rng.integers(1, 130)), dtype=np.uint8).tobytes()
        return (p * (n // len(p) + 1))[:n]
    b = bytearray(rng.integers(0, int(rng.integers(2, 257)), n, dtype=np.uint8).tobytes())
    for _ in range(int(rng.integers(0, 60))):
        if n < 20:
            break
        L = int(rng.integers(4, min(n, 3000)))
        s, d = int(rng.integers(0, n - L + 1)), int(rng.integers(0, n - L + 1))
        b[d:d + L] = b[s:s + L]
    return bytes(b)


_SWEEP = []


def _sweep():
    """300 random recipes (seed 1), content of at most 20,000 bytes; about 4 s on one CPU core."""
    if not _SWEEP:
        rng = np.random.default_rng(1)
        for i in range(300):
            n = int(rng.choice([rng.integers(0, 300), rng.integers(0, 20001)]))
            content = _content(rng, n)
            n = len(content)
            recipe = Z.random_recipe(rng, content)
            frame, rec = Z.build_frame(content, recipe)
            _SWEEP.append((frame, content, rec))
    return _SWEEP


def test_random_recipes_libzstd_and_model_agree():
    for i, (frame, content, rec) in enumerate(_sweep()):
        check(frame, content, True, f"sweep frame {i}")


def test_records_cover_the_format():
    """What the named cases and the sweep emitted, from their records: each part of the format the
    writer exists for was written at least once (and, by the tests above, decoded by libzstd)."""
    frames = [r for c in Z.catalogue() if c.valid for r in c.recs] + [rec for _, _, rec in _sweep()]
    blocks = [b for f in frames for b in f["blocks"]]
    comp = [b for b in blocks if b["type"] == "comp"]
    assert {f["fcs_bytes"] for f in frames} == {0, 1, 2, 4, 8}
    assert {(f["single"], f["dict_flag"]) for f in frames} >= {(s, d) for s in (True, False) for d in range(4)}
    assert any(f["checksum"] == "ok" for f in frames)
    assert {b["type"] for b in blocks} == {"raw", "rle", "comp"}
    assert any(b["last"] for b in blocks if b["type"] == "raw") and any(b["last"] for b in blocks if b["type"] == "rle")
    assert any(b["bsize"] > 131072 for b in blocks if b["type"] == "raw")
    assert any(b["size"] > 131072 for b in blocks if b["type"] == "rle")
    assert {(b["lit_mode"], b["lit_hform"]) for b in comp} >= {("raw", 1), ("raw", 2), ("raw", 3), ("rle", 1), ("rle", 2),
                                                               ("rle", 3), ("huf", 3), ("huf", 4), ("huf", 5),
                                                               ("treeless", 3), ("treeless", 4)}
    huf = [b for b in comp if b["lit_mode"] == "huf"]
    assert {b["huf_log"] for b in huf} == set(range(1, 13))
    assert {(b["huf_log"], b["huf_streams"], b["huf_desc"]) for b in huf} >= {
        (L, s, d) for L in (1, 2, 5, 6, 11, 12) for s in (1, 4) for d in ("direct", "fse")}
    assert all(b["huf_max_weight"] <= 11 for b in huf)
    assert any(b["huf_nweights"] == 128 and b["huf_desc"] == "direct" for b in huf)
    seqb = [b for b in comp if b["nbseq"]]
    for k in range(3):
        assert {b["seq_modes"][k] for b in seqb} == {"predef", "rle", "fse", "repeat"}
    assert {b["nbseq_form"] for b in comp} == {1, 2, 3}
    assert any(b["nbseq_form"] == 2 and b["nbseq"] < 128 for b in comp)
    assert max(b["max_codes"][0] for b in seqb) == 35 and max(b["max_codes"][2] for b in seqb) == 52
    assert max(b["max_codes"][1] for b in seqb) >= 18
    assert {(v, 0) for b in seqb for v in b["ll0_rep"]} | {(v, 1) for b in seqb for v in b["llpos_rep"]} == {
        (v, z) for v in (1, 2, 3) for z in (0, 1)}
    descs = [d for b in seqb for d in b.get("fse_desc", {}).items()]
    for name, lg in (("ll", 9), ("of", 8), ("ml", 9)):
        assert any(k == name and d["log"] == lg and d["low"] and d["zero_runs"] for k, d in descs)
    assert any(max(d["zero_runs"], default=0) >= 3 for _, d in descs)
    assert max(b["nbseq"] for b in comp) == 98047
    # the 256-byte header window: block header, literals header and jump table (= the description's end)
    # at every offset around its end, and a raw block of every length from 230 to 262 in front
    win = [f["blocks"] for c in Z.catalogue() if c.group == "hdrwin" for f in c.recs if len(f["blocks"]) == 2]
    want = set(range(230, 263))
    assert {b[1]["off"] for b in win} >= want and {b[1]["off"] + 3 for b in win} >= want
    assert {b[1]["off"] + 3 + b[1]["huf_desc_off"] + b[1]["huf_jump_off"] for b in win if b[1]["off"] + 8 <= 256} >= want
    assert {b[0]["bsize"] for b in win} >= want
    assert any(b["seq_bits_len"] > 3 * 2048 for b in seqb)
