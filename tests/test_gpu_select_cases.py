"""The reads of tests/_select_cases.py through the selection kernels (csrc/pgn_select.h) on the GPU: every case
through read_stats with the split on and off, bit for bit against ref_stats (np.sort) and the builder's intended
statistics, with the split counters saying that every read took the route it was built for; calls in succession
on one context; the convert pass with destinations whose 16-byte phases differ (its element-wise stores); and
float16 outputs below the normal range, above it and on ties.  Everything is integer-exact or a listed sequence
of IEEE operations: the tolerance is zero.  tests/test_select_cases.py checks the cases themselves.
"""
import numpy as np
import pytest

import _select_cases as S
from test_gpu_norm import BITS, NP_OF, SENTINEL, assert_bits, dev, tdtype
from test_gpu_select_split import SMALL, expected_counts
from test_norm_api import QUANTILE, assert_stats_equal, ref_norm, ref_stats

pytestmark = pytest.mark.gpu

ZERO = dict(short=0, whole=0, split=0, parts=0, no_slot=0)


@pytest.fixture(scope="module")
def codec():
    """A context of this module's own: the tests change its split settings, and put them back."""
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rawnanoporesignalcompression_amd import PGNanoCodec

    c = PGNanoCodec(0)
    before = c.select_split
    c.set_select_split(**SMALL)
    yield c
    c.set_select_split(*before)
    assert c.select_split == before
    c.close()


def stats_on_and_off(codec, reads, prm, what):
    """read_stats of the packed reads with the split on and off: (on, off, counters of the call with it on).  The
    flat buffer starts on a 16-byte boundary, so a case's phase is its address modulo 16 bytes."""
    flat, offsets, counts = S.pack(reads)
    d = dev(flat), dev(offsets), dev(counts)
    assert d[0].data_ptr() % 16 == 0
    codec.set_select_split(**SMALL)
    on = codec.read_stats(*d, **prm).numpy()
    got = codec.select_split_counts()
    codec.set_select_split(max_split_reads=0)
    off = codec.read_stats(*d, **prm).numpy()
    assert codec.select_split_counts() == ZERO
    codec.set_select_split(**SMALL)
    assert got == expected_counts(counts), what
    assert on.tobytes() == off.tobytes(), f"{what}: split and one-workgroup statistics differ"
    return on, got


GROUPS = S.groups()


@pytest.mark.parametrize("g", range(len(GROUPS)), ids=[f"{p['mode']}_{p['p'][0]:.4g}_{p['p'][1]:.4g}" for p, _ in GROUPS])
def test_every_case_on_its_route(codec, g):
    """One call per parameter set holds the set's cases of all three routes; the counters equal what the lengths
    imply and what the cases were built for."""
    prm, cases = GROUPS[g]
    on, got = stats_on_and_off(codec, cases, prm, f"{prm['mode']} {prm['p']}")
    routes = [c.route for c in cases]
    assert (got["short"], got["whole"], got["split"]) == tuple(routes.count(r) for r in S.ROUTES) and got["no_slot"] == 0
    assert got["parts"] == sum(len(S.parts_of(c.x.size)) - 1 for c in cases if c.route == "split")
    for r, c in enumerate(cases):
        assert_stats_equal(on[r], ref_stats(c.x, **c.prm), c.name)
        for k, v in c.want.items():
            assert int(on[r][k]) == v, (c.name, k, int(on[r][k]), v)


def test_every_route_in_the_catalogue():
    """No parameter set is left out and the catalogue's reads reach all three kernels."""
    assert sum(len(cs) for _, cs in GROUPS) == len(S.catalogue())
    assert {c.route for c in S.catalogue()} == set(S.ROUTES)


# ---- family 7: calls in succession -----------------------------------------------------------------------------
def test_calls_in_succession(codec):
    """med/MAD with 3 split reads, quantiles with 1 split read of other data, med/MAD with 5, on one context with
    the split on throughout: the slots and their histograms are used again from call to call."""
    codec.set_select_split(**SMALL)
    results = []
    for prm, rs in S.succession():
        flat, offsets, counts = S.pack([x for x, _ in rs])
        st = codec.read_stats(dev(flat), dev(offsets), dev(counts), **prm).numpy()
        got = codec.select_split_counts()
        assert got == expected_counts(counts) and got["split"] == sum(x.size > 1024 for x, _ in rs)
        results.append(st)
        for r, (x, want) in enumerate(rs):
            assert_stats_equal(st[r], ref_stats(x, **prm), f"{prm['mode']} read {r} (n {x.size})")
            for k, v in want.items():
                assert int(st[r][k]) == v
    assert [int((st["n"] > 1024).sum()) for st in results] == [3, 1, 5]
    # and the same calls with the split off
    codec.set_select_split(max_split_reads=0)
    for (prm, rs), on in zip(S.succession(), results):
        flat, offsets, counts = S.pack([x for x, _ in rs])
        off = codec.read_stats(dev(flat), dev(offsets), dev(counts), **prm).numpy()
        assert codec.select_split_counts() == ZERO and on.tobytes() == off.tobytes()
    codec.set_select_split(**SMALL)


def test_a_workgroup_takes_several_reads(codec):
    """1,200 reads of 513 to 600 samples in one call: more than the one-workgroup kernel's grid (four workgroups per
    compute unit), so a workgroup selects a second read in the LDS the first one filled -- and that read's placed
    bins are the bins the read before filled most."""
    import torch

    reads = S.chain_reads()
    assert 4 * torch.cuda.get_device_properties(0).multi_processor_count < len(reads)
    on, got = stats_on_and_off(codec, [x for x, _ in reads], QUANTILE, "chain")
    assert got == dict(ZERO, whole=len(reads))
    for r, (x, want) in enumerate(reads):
        assert_stats_equal(on[r], ref_stats(x, **QUANTILE), f"chain read {r} (n {x.size})")
        assert (int(on[r]["q_lo"]), int(on[r]["q_hi"])) == (want["q_lo"], want["q_hi"])


# ---- the convert pass off its aligned path ---------------------------------------------------------------------
class ConvertBatch:
    def __init__(self, codec):
        self.reads, self.chunks, self.starts, self.total = S.convert_reads()
        self.counts = np.array([c for cs in self.chunks for c in cs], np.int32)
        self.first = np.concatenate([[0], np.cumsum([len(cs) for cs in self.chunks])]).astype(np.int64)
        flat = np.concatenate(self.reads)
        chunk_off = np.concatenate([[0], np.cumsum(self.counts.astype(np.int64))[:-1]]).astype(np.int64)
        self.enc = codec.compress_batch(dev(flat), dev(chunk_off), dev(self.counts))
        assert (self.enc.status.cpu().numpy() == 0).all()
        self.stats = [ref_stats(x, **QUANTILE) for x in self.reads]
        self.ref = {dt: [ref_norm(x, s["centre"], s["spread"], NP_OF[dt]) for x, s in zip(self.reads, self.stats)]
                    for dt in ("float32", "float16")}


@pytest.fixture(scope="module")
def convert_batch(codec):
    return ConvertBatch(codec)


CONVERT = [(dt, a, b) for dt, views in S.CONVERT_VIEWS.items() for a, b in views]


@pytest.mark.parametrize("dtype,out_start,adc_start", CONVERT,
                         ids=[f"{dt}_out{a}_" + ("in_place" if b is None else f"adc{b}") for dt, a, b in CONVERT])
def test_convert_with_destinations_out_of_phase(codec, convert_batch, dtype, out_start, adc_start):
    """out starts out_start elements into its allocation and adc adc_start elements into its own, at different
    16-byte phases, with gaps between the reads: the whole of both allocations is compared -- the reads' spans
    with ref_norm and the samples, every other element with the sentinel it held."""
    import torch

    b = convert_batch
    margin = 8
    sent = SENTINEL[dtype]
    out_buf = torch.empty(out_start + b.total + margin, dtype=tdtype(dtype), device="cuda:0")
    out_buf.view(torch.int32 if dtype == "float32" else torch.int16).fill_(sent)
    out = out_buf[out_start:]
    adc_buf = adc = None
    if adc_start is not None:
        adc_buf = torch.full((adc_start + b.total + margin,), -9999, dtype=torch.int16, device="cuda:0")
        adc = adc_buf[adc_start:]
        assert adc_buf.data_ptr() % 16 == 0 and adc.data_ptr() % 16 == S.byte_phase("float16", adc_start)
        assert adc.data_ptr() % 16 != out.data_ptr() % 16
    assert out_buf.data_ptr() % 16 == 0 and out.data_ptr() % 16 == S.byte_phase(dtype, out_start)
    got, ro, st, cst = codec.decompress_reads_norm(b.enc.blobs, b.enc.offsets, b.enc.sizes, dev(b.counts), dev(b.first),
                                                   dtype=tdtype(dtype), out=out, adc=adc, read_out_offsets=dev(b.starts),
                                                   **QUANTILE)
    assert got.data_ptr() == out.data_ptr() and (cst.cpu().numpy() == 0).all()
    assert np.array_equal(ro.cpu().numpy(), b.starts)
    s = st.numpy()
    want = np.full(out_buf.numel(), sent, BITS[dtype])
    want_adc = np.full(adc_buf.numel(), -9999, np.int16) if adc_buf is not None else None
    for r, x in enumerate(b.reads):
        assert_stats_equal(s[r], b.stats[r], f"read {r}")
        at = int(b.starts[r])
        want[out_start + at:out_start + at + x.size] = b.ref[dtype][r].view(BITS[dtype])
        if want_adc is not None:
            want_adc[adc_start + at:adc_start + at + x.size] = x
    assert_bits(out_buf.cpu().numpy(), want.view(NP_OF[dtype]), dtype, f"{dtype} out +{out_start} adc +{adc_start}")
    if want_adc is not None:
        assert np.array_equal(adc_buf.cpu().numpy(), want_adc)


# ---- float16 outside the normal range ----------------------------------------------------------------------------
class RangeBatch:
    def __init__(self, codec):
        self.x = S.all_values_read()
        self.counts = np.array([30000, 35536], np.int32)
        self.first = np.array([0, 2], np.int64)
        self.enc = codec.compress_batch(dev(self.x), dev(np.array([0, 30000], np.int64)), dev(self.counts),
                                        out_caps=dev(self.counts.astype(np.int64) * 4 + 4096))
        assert (self.enc.status.cpu().numpy() == 0).all()


@pytest.fixture(scope="module")
def range_batch(codec):
    return RangeBatch(codec)


@pytest.mark.parametrize("dtype", ["float32", "float16"])
@pytest.mark.parametrize("key", list(S.F16_RANGE))
def test_float16_range(codec, range_batch, key, dtype):
    """All 65,536 int16 values under the usual parameters, a spread that makes every output a binary16 subnormal,
    and the floor as spread, under which half the outputs overflow to infinities and thousands lie on ties."""
    b, prm = range_batch, S.F16_RANGE[key]
    out, ro, st, cst = codec.decompress_reads_norm(b.enc.blobs, b.enc.offsets, b.enc.sizes, dev(b.counts), dev(b.first),
                                                   dtype=tdtype(dtype), **prm)
    assert (cst.cpu().numpy() == 0).all()
    w = ref_stats(b.x, **prm)
    assert_stats_equal(st.numpy()[0], w, key)
    with np.errstate(over="ignore"):  # binary16 overflow is +-inf, as in the kernel
        want = ref_norm(b.x, w["centre"], w["spread"], NP_OF[dtype])
    assert_bits(out.cpu().numpy()[:b.x.size], want, dtype, f"{key} {dtype}")
