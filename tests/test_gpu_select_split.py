"""Long reads selected in parts by several workgroups (include/pgnano_hip.h, "Long reads";
PGNanoCodec.set_select_split) on the GPU.  Every pgn_read_stats field is compared bit for bit with the host
reference of tests/test_norm_api.py and with the same call with the split off, and the counters of
pgn_select_split_counts say how many reads were split into how many parts, so no test passes with the
split silently not taken.  Unless stated the settings are the smallest the setter allows (split above 1,024
samples, parts of 1,024), so a read of 1,025 samples already has two parts.
"""
import numpy as np
import pytest

import _oracle as O
from test_norm_api import MEDMAD, QUANTILE, assert_stats_equal, ref_norm, ref_stats
from test_segment_api import USUAL, ref_batch

pytestmark = pytest.mark.gpu

SMALL = dict(split_min_samples=1024, part_samples=1024, max_split_reads=1024)
DEFAULTS = (196608, 32768, 1024)  # include/pgnano_hip.h
PARAMS = {"quantile": QUANTILE, "extremes": dict(QUANTILE, p=(0.0, 1.0)), "p_equal": dict(QUANTILE, p=(0.5, 0.5)),
          "medmad": MEDMAD}
MIXED = [0, 1, 512, 513, 1024, 1025, 2047, 2048, 2049, 5000, 70_001, 300_007]


def dev(a):
    import torch

    return torch.from_numpy(np.array(a, order="C")).to(torch.device("cuda", 0))


@pytest.fixture(scope="module")
def codec():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rawnanoporesignalcompression_amd import PGNanoCodec

    c = PGNanoCodec(0)
    yield c
    c.close()


def pack(reads):
    """Back to back behind one leading sample: flat, offsets, counts."""
    counts = np.array([r.size for r in reads], np.int64)
    offsets = 1 + np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    return np.concatenate([np.array([12345], np.int16)] + list(reads)), offsets, counts


def expected_counts(counts, split_min=1024, part=1024, slots=1024):
    """What the plan does with reads of these lengths, from the contract."""
    want = dict(short=0, whole=0, split=0, parts=0, no_slot=0)
    for n in counts:
        n = int(n)
        if n > split_min and want["split"] < slots:
            want["split"] += 1
            want["parts"] += min(-(-n // part), 4096)
        elif n > split_min:
            want["no_slot"] += 1
            want["whole"] += 1
        else:
            want["short" if n <= 512 else "whole"] += 1
    return want


def stats_both_ways(codec, reads, prm, settings=SMALL, what=""):
    """read_stats with the split on (the counters are returned) and off: both equal the host reference, and
    each other byte for byte."""
    flat, offsets, counts = pack(reads)
    d = dev(flat), dev(offsets), dev(counts)
    codec.set_select_split(**settings)
    on = codec.read_stats(*d, **prm).numpy()
    got = codec.select_split_counts()
    codec.set_select_split(max_split_reads=0)
    off = codec.read_stats(*d, **prm).numpy()
    assert codec.select_split_counts() == dict(short=0, whole=0, split=0, parts=0, no_slot=0)
    codec.set_select_split(**settings)
    assert on.tobytes() == off.tobytes(), f"{what}: split and one-workgroup statistics differ"
    for r, x in enumerate(reads):
        assert_stats_equal(on[r], ref_stats(x, **prm), f"{what}: read {r} (n {x.size})")
    return got


def test_settings_round_trip(codec):
    from rawnanoporesignalcompression_amd import PGNanoError

    codec.set_select_split(split_min_samples=5000, part_samples=2048, max_split_reads=7)
    assert codec.select_split == (5000, 2048, 7)
    codec.set_select_split(max_split_reads=0)
    assert codec.select_split == (5000, 2048, 0)
    for bad in (dict(part_samples=1023), dict(part_samples=(1 << 24) + 1, split_min_samples=1 << 25),
                dict(split_min_samples=2047), dict(max_split_reads=65537)):
        with pytest.raises(PGNanoError):
            codec.set_select_split(**bad)
    assert codec.select_split == (5000, 2048, 0)
    codec.set_select_split(**SMALL)
    assert codec.select_split == (1024, 1024, 1024)


@pytest.mark.parametrize("key", list(PARAMS))
def test_mixed_lengths_in_one_call(codec, key):
    from rawnanoporesignalcompression_amd import select_parts

    reads = [O.synth_read(300 + j, n) for j, n in enumerate(MIXED)]
    _, offsets, counts = pack(reads)
    assert (offsets % 2 == 1).any() and (offsets % 2 == 0).any()
    starts = np.concatenate([o + select_parts(n, 1024, 1024)[:-1].astype(np.int64) for o, n in zip(offsets, counts) if n > 1024])
    assert set((starts % 8).tolist()) == set(range(8))
    got = stats_both_ways(codec, reads, PARAMS[key], what=key)
    assert got == dict(short=3, whole=2, split=7, parts=2 + 2 + 2 + 3 + 5 + 69 + 293, no_slot=0)
    assert got == expected_counts(counts)


def stress_reads():
    rng = np.random.default_rng(2027)
    n = 70_001
    halves = np.concatenate([rng.integers(380, 420, n // 2), rng.integers(3380, 3420, n - n // 2)]).astype(np.int16)
    # an odd m2 needs the two middle values of an even count to differ by an odd number: 70,002 samples,
    # half of them at most 400 and half at least 401 (an odd count gives m2 = 2 * median, always even)
    odd_m2 = np.concatenate([rng.integers(300, 401, 35_001), rng.integers(401, 500, 35_001)]).astype(np.int16)
    odd_m2[0], odd_m2[35_001] = 400, 401
    reads = {
        "constant": np.full(n, 431, np.int16),
        "two_values": np.where(rng.integers(0, 2, n) == 1, 32767, -32768).astype(np.int16),
        "ramp": np.linspace(-32768, 32767, n).round().astype(np.int16),
        "gaussian": np.clip(rng.normal(400, 50, n).round(), -32768, 32767).astype(np.int16),
        "halves": halves,
        "odd_m2": rng.permutation(odd_m2),
    }
    assert ref_stats(reads["odd_m2"], **MEDMAD)["m2"] % 2 == 1
    return reads


@pytest.mark.parametrize("key", list(PARAMS))
def test_data_that_stresses_the_bins(codec, key):
    reads = stress_reads()
    got = stats_both_ways(codec, list(reads.values()), PARAMS[key], what=key)
    assert got == dict(short=0, whole=0, split=6, parts=6 * 69, no_slot=0)  # 70,001 and 70,002: 69 parts each


@pytest.mark.parametrize("key", ["quantile", "medmad"])
def test_the_cap(codec, key):
    """One read of 4,096 * 1,024 + 12,345 samples: 4,096 parts of 1,027 or 1,028 samples."""
    n = 4096 * 1024 + 12_345
    x = O.synth_read(77, n)
    got = stats_both_ways(codec, [x], PARAMS[key], what=f"cap {key}")
    assert got == dict(short=0, whole=0, split=1, parts=4096, no_slot=0)


def test_slot_exhaustion(codec):
    reads = [O.synth_read(500 + j, 5000) for j in range(5)]
    for key in ("quantile", "medmad"):
        got = stats_both_ways(codec, reads, PARAMS[key], settings=dict(SMALL, max_split_reads=2), what=f"two slots {key}")
        assert got == dict(short=0, whole=3, split=2, parts=10, no_slot=3)
    codec.set_select_split(**SMALL)


def test_many_reads_cross_the_plan_steps(codec):
    """20,000 reads: the reads are classified in blocks of 512 and the plan numbers slots and work items
    across the blocks, so the running counts cross threads, waves and blocks; the 150 slots run out in the
    middle of a block.  Every 97th read is long enough to split, one in three of the others takes the
    one-workgroup kernel."""
    rng = np.random.default_rng(97)
    lengths = np.where(np.arange(20_000) % 3 == 0, 600, rng.integers(0, 9, 20_000))
    lengths[::97] = rng.integers(1025, 3000, lengths[::97].size)
    reads = [rng.integers(300, 700, int(n)).astype(np.int16) for n in lengths]
    flat, offsets, counts = pack(reads)
    d = dev(flat), dev(offsets), dev(counts)
    for key in ("quantile", "medmad"):
        codec.set_select_split(**dict(SMALL, max_split_reads=150))
        on = codec.read_stats(*d, **PARAMS[key]).numpy()
        got = codec.select_split_counts()
        codec.set_select_split(max_split_reads=0)
        off = codec.read_stats(*d, **PARAMS[key]).numpy()
        codec.set_select_split(**SMALL)
        want = expected_counts(counts, slots=150)
        assert got == want and want["split"] == 150 and want["no_slot"] == 207 - 150 and want["short"] > 10_000
        assert on.tobytes() == off.tobytes(), key
        for r in range(0, 20_000, 97):
            assert_stats_equal(on[r], ref_stats(reads[r], **PARAMS[key]), f"{key}: read {r} (n {reads[r].size})")
        for r in (1, 3, 8191, 8192, 8193, 16_383, 16_384, 19_998, 19_999):
            assert_stats_equal(on[r], ref_stats(reads[r], **PARAMS[key]), f"{key}: read {r} (n {reads[r].size})")


def test_more_reads_than_one_plan_step(codec):
    """300,000 reads: the plan scans the totals of blocks of 512 reads, 512 blocks (262,144 reads) per step,
    so the last reads belong to a second step.  Nearly all reads are one sample long; six are long enough
    to split, on both sides of the step boundary, and with four slots the last two find none."""
    rng = np.random.default_rng(5)
    lengths = np.ones(300_000, np.int64)
    long_reads = [7, 100_000, 262_143, 262_144, 280_000, 299_999]
    lengths[long_reads] = [1500, 2049, 1025, 3000, 1100, 2500]
    offsets = 1 + np.concatenate([[0], np.cumsum(lengths)[:-1]])
    flat = rng.integers(300, 700, int(lengths.sum()) + 1).astype(np.int16)
    d = dev(flat), dev(offsets), dev(lengths)
    for slots in (1024, 4):
        codec.set_select_split(**dict(SMALL, max_split_reads=slots))
        on = codec.read_stats(*d, **MEDMAD).numpy()
        got = codec.select_split_counts()
        codec.set_select_split(max_split_reads=0)
        off = codec.read_stats(*d, **MEDMAD).numpy()
        codec.set_select_split(**SMALL)
        assert got == expected_counts(lengths, slots=slots) and got["split"] == min(slots, 6) and got["short"] == 299_994
        assert on.tobytes() == off.tobytes(), slots
        for r in long_reads + [0, 262_142, 299_998]:
            x = flat[offsets[r]:offsets[r] + lengths[r]]
            assert_stats_equal(on[r], ref_stats(x, **MEDMAD), f"slots {slots}: read {r} (n {x.size})")


def test_defaults(codec):
    """A fresh context (the module's own has had its settings changed)."""
    from rawnanoporesignalcompression_amd import PGNanoCodec

    fresh = PGNanoCodec(0)
    try:
        assert fresh.select_split == DEFAULTS
        split_min, part, slots = DEFAULTS
        reads = [O.synth_read(41, split_min + 1), O.synth_read(42, split_min), O.synth_read(43, 100)]
        for key in ("quantile", "medmad"):
            got = stats_both_ways(fresh, reads, PARAMS[key],
                                  settings=dict(split_min_samples=split_min, part_samples=part, max_split_reads=slots),
                                  what=f"defaults {key}")
            assert got == dict(short=1, whole=1, split=1, parts=-(-(split_min + 1) // part), no_slot=0)
    finally:
        fresh.close()


# ---- through the callers -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float16", "float32"])
def test_decompress_reads_norm_splits(codec, dtype):
    """Reads of several chunks, one of them with a truncated blob (tests/test_gpu_norm.py's corruption): the
    read carries the chunk's status, every other read is exact; float16 converts in place, float32 has adc."""
    import torch

    tdt = {"float16": torch.float16, "float32": torch.float32}[dtype]
    npdt, bits = {"float16": (np.float16, np.uint16), "float32": (np.float32, np.uint32)}[dtype]
    sizes = [[3000, 2000], [5000, 1234, 4000], [777], [], [2500, 2500], [40_000, 30_001]]
    reads = [O.synth_read(950 + r, sum(cs)) for r, cs in enumerate(sizes)]
    counts = np.array([c for cs in sizes for c in cs], np.int32)
    first = np.concatenate([[0], np.cumsum([len(cs) for cs in sizes])]).astype(np.int64)
    blobs = []
    for r, cs in enumerate(sizes):
        at = 0
        for c in cs:
            rc, blob = O.c5_compress(reads[r][at:at + c])[:2]
            assert rc == 0
            blobs.append(blob)
            at += c
    bad_chunk, bad_read = 3, 1  # the 1,234-sample chunk of read 1
    blobs[bad_chunk] = blobs[bad_chunk][:len(blobs[bad_chunk]) - 9]
    bsizes = np.array([len(x) for x in blobs], np.int64)
    boffs = np.concatenate([[0], np.cumsum(bsizes)[:-1]]).astype(np.int64)
    d_blobs = dev(np.frombuffer(b"".join(blobs), np.uint8).copy())
    _, _, want_st = codec.decompress_batch(d_blobs, dev(boffs), dev(bsizes), dev(counts))
    want_st = want_st.cpu().numpy()
    assert want_st[bad_chunk] != 0 and (np.delete(want_st, bad_chunk) == 0).all()
    total = sum(x.size for x in reads)
    results = {}
    for slots in (1024, 0):
        codec.set_select_split(**dict(SMALL, max_split_reads=slots))
        adc = torch.full((total,), -9999, dtype=torch.int16, device="cuda:0") if dtype == "float32" else None
        out, ro, st, cst = codec.decompress_reads_norm(d_blobs, dev(boffs), dev(bsizes), dev(counts), dev(first),
                                                       dtype=tdt, adc=adc, **QUANTILE)
        results[slots] = (out.cpu().numpy(), ro.cpu().numpy(), st.numpy(), cst.cpu().numpy(), codec.select_split_counts())
    codec.set_select_split(**SMALL)
    out, ro, st, cst, got = results[1024]
    assert got == dict(short=1, whole=1, split=4, parts=5 + 10 + 5 + 69, no_slot=0)
    assert results[0][4]["split"] == 0
    assert np.array_equal(cst, want_st)
    for r, x in enumerate(reads):
        if r == bad_read:
            assert int(st[r]["status"]) == int(want_st[bad_chunk]) and int(st[r]["n"]) == x.size
            continue
        w = ref_stats(x, **QUANTILE)
        assert_stats_equal(st[r], w, f"read {r}")
        assert st[r].tobytes() == results[0][2][r].tobytes()
        seg = out[ro[r]:ro[r] + x.size]
        assert np.array_equal(seg.view(bits), ref_norm(x, w["centre"], w["spread"], npdt).view(bits)), f"read {r}"
        assert np.array_equal(seg.view(bits), results[0][0][ro[r]:ro[r] + x.size].view(bits))


@pytest.mark.parametrize("mode", ["quantile", "medmad"])
def test_segment_reads_splits(codec, mode):
    """The usual trim on reads of 20,000 to 120,000 samples: the heads (8,000 samples) and the trimmed reads,
    which start at offset + trim on any boundary, are both selected in parts."""
    import torch

    from rawnanoporesignalcompression_amd import segment_signal

    prm = PARAMS[mode]
    lengths = [20_000, 33_333, 64_001, 90_010, 120_000]
    reads = [O.synth_read(900 + j, n) for j, n in enumerate(lengths)]
    flat, offsets, counts = pack(reads)
    L, V = 4000, 500
    want = ref_batch(reads, L, V, USUAL, prm)
    trims = [int(r["trim"]) for r in want["reads"]]
    assert len({(o + t) % 8 for o, t in zip(offsets, trims)}) >= 3 and any(t > 10 for t in trims)
    cap = want["total"] + 2
    results = {}
    for slots in (1024, 0):
        codec.set_select_split(**dict(SMALL, max_split_reads=slots))
        res = codec.segment_reads(dev(flat), dev(offsets), counts, length=L, overlap=V, trim=True, dtype=torch.float16,
                                  capacity=cap, **prm)
        results[slots] = (int(res.total.item()), res.reads.numpy(), res.segments.numpy(), res.stats.numpy(),
                          res.out.cpu().numpy()[:want["total"]], codec.select_split_counts())
    codec.set_select_split(**SMALL)
    total, got_reads, segs, stats, out, got = results[1024]
    assert got == expected_counts([n - t for n, t in zip(lengths, trims)]) and got["split"] == 5
    assert results[0][5]["split"] == 0
    assert total == want["total"] == results[0][0]
    for r, w in enumerate(want["reads"]):
        for k in ("first_segment", "nsegments", "trim", "status", "head_m2", "head_mad4"):
            assert int(got_reads[r][k]) == int(w[k]), f"read {r} {k}"
        assert_stats_equal(stats[r], want["stats"][r], f"read {r}")
    assert np.array_equal(np.stack([segs["read"], segs["start"], segs["valid"]], 1).astype(np.int64)[:total], want["segments"])
    rows = np.concatenate([segment_signal(x, L, V, trim=True, dtype=np.float16, **prm) for x in reads])
    assert rows.shape == (total, L)
    assert np.array_equal(out.view(np.uint16), rows.view(np.uint16))
    for a, b in zip(results[1024][1:5], results[0][1:5]):  # the split off: the same bytes everywhere
        assert a.tobytes() == b.tobytes()
