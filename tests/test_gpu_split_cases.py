"""Every split route on the signals of tests/_split_cases.py, byte for byte against the oracle.

tests/test_split_cases.py holds the catalogue on the CPU (claims, restatement, reference, faults, capacity).
Here every case goes through every route that reaches a split kernel, and every blob must be the oracle's:

  C5, default context   compress_signal (one chunk: the 32-range split); compress_batch in batches of at most 64
                        (the range split) and of 65 to the CU count (enc_split_kernel, one wave per chunk); the
                        chunk above 262,144 samples alone and inside a batch (the large-chunk pass)
  C5, forced contexts   PGN_ENC_PIPELINE=staged: batches of 65 or more; PGN_ENC_PIPELINE=fused: small and large
                        batches and single chunks (c5_split_wave inside enc_chunk_kernel)
  VBZ                   compress_signal, batches, and the same two forced contexts (vbz_split_kernel, fused)
  C4, C1, C2, C3, VBZ0  compress_signal and batches (fused only)

Batches.  Every case is followed in memory, and in the batch, by a short chunk that starts far from the case's
last sample, so a ragged step that read on behind its chunk would see a large delta; a one-sample gap in
front of every other case puts the chunk starts on odd and even sample offsets.  The blobs go into a caller's
buffer with out_offsets / out_caps, the reference's capacities apart by guard bytes that must survive.  C5
batches ask for the stream counters, which must be the oracle's.  Every blob is also decoded on the GPU and
compared with the samples.

A blob that differs is decoded frame by frame with libzstd on the host: the failure names the case, the route,
the stream, the first differing byte and the sample, step and range that byte belongs to, or says that the
streams are equal and only the zstd frames differ.
"""
import os

import numpy as np
import pytest

import _oracle as O
import _split_cases as S

pytestmark = pytest.mark.gpu

VARIANTS = ["C4", "C1", "C2", "C3", "VBZ0"]
GUARD = 64
SENTINEL = 0xA5
STAGED = "enc_split_kernel + enc_zstd_kernel + enc_assemble_kernel"
FUSED = "enc_chunk_kernel<C5>"
STREAM_NAMES = {5: ["keys", "S", "M", "Llow", "Lhigh"], 4: ["keys", "A", "B", "H"], 3: ["keys", "A", "H"],
                2: ["keys", "data"], 1: ["frame"]}


class Item:
    """one chunk of a batch: a case, or the far chunk behind one"""

    def __init__(self, name, x, gap=0):
        self.name, self.x, self.n, self.gap = name, np.ascontiguousarray(x, np.int16), int(np.asarray(x).size), gap


def far_chunk(c):
    """a short chunk whose first sample is 0x4000 and a little more away from the case's last one (the same
    chunk wherever the case stands in a batch)"""
    last = int(c.x[-1]) if c.n else 0
    z = S.coded(S._mixed(17, c.n % 7))
    z[0] = 0
    x = (S.signal(z).astype(np.int64) + last + 0x4000 + 257 * (c.n % 61)) & 0xFFFF
    return Item(c.name + "+far", x.astype(np.uint16).view(np.int16))


def with_far(cases):
    out = []
    for i, c in enumerate(cases):
        out += [Item(c.name, c.x, gap=i & 1), far_chunk(c)]
    return out


_EXPECT = {}


def expect(codec, it):
    """(blob, stream counters) of the oracle, computed once per module"""
    key = (codec, it.name)
    if key not in _EXPECT:
        if codec == "VBZ":
            _EXPECT[key] = (O.vbz_compress(it.x), None)
        else:
            rc, blob, st = O.c5_compress(it.x) if codec == "C5" else O.variant_compress(codec, it.x)
            assert rc == 0, (codec, it.name, rc)
            _EXPECT[key] = (blob, st.astype(np.int64))
    return _EXPECT[key]


def nframes(codec):
    return 1 if codec == "VBZ" else O.VARIANT_FRAMES[codec]


def diagnose(codec, it, got, want):
    """what differs between two blobs of one chunk"""
    nf = nframes(codec)
    gs, ws = O.blob_streams(got, nf, it.n), O.blob_streams(want, nf, it.n)
    if gs is None:
        return f"sizes {len(got)} / {len(want)}, the frame lengths run past the blob"
    for s, (g, w) in enumerate(zip(gs, ws)):
        name = STREAM_NAMES[nf][s]
        if g is None:
            return f"stream {name}: libzstd does not decode the frame"
        if g != w:
            m = min(len(g), len(w))
            at = next((i for i in range(m) if g[i] != w[i]), m)
            where = S.locate(it.x, codec, s, at)
            place = "" if where is None else f", sample {where[0]}, step {where[1]}, range {where[2]}"
            gb = f"{g[at]:#04x}" if at < len(g) else "none"
            wb = f"{w[at]:#04x}" if at < len(w) else "none"
            return f"stream {name}: {len(g)} / {len(w)} bytes, first differing byte {at} ({gb} / {wb}){place}"
    return "the streams are equal and the zstd frames differ (a zstd difference, not the split's)"


def report(route, codec, wrong):
    assert not wrong, f"{route}, {codec}: {len(wrong)} chunks differ: " + "; ".join(wrong[:8])


def check_single(c, codec, cases, route):
    wrong = []
    for case in cases:
        it = Item(case.name, case.x)
        want, _ = expect(codec, it)
        got = c.compress_signal(it.x)
        if got != want:
            wrong.append(f"{it.name}: {diagnose(codec, it, got, want)}")
        back = c.decompress_signal(got, sample_count=it.n)
        if not np.array_equal(back, it.x):
            wrong.append(f"{it.name}: the GPU's decode of its blob differs from the samples")
    report(route, codec, wrong)


def run_batch(c, codec, items, route, stats=False):
    """one compress_batch call into a guarded buffer; every blob, counter and guard byte checked, the blobs decoded"""
    import torch

    dev = torch.device("cuda", 0)
    starts, parts, pos = [], [], 0
    for it in items:
        if it.gap:
            parts.append(np.full(it.gap, 12345, np.int16))
            pos += it.gap
        starts.append(pos)
        parts.append(it.x)
        pos += it.n
    parts.append(np.full(64, -23456, np.int16))  # what lies behind the last chunk
    flat = np.concatenate(parts)
    counts = np.array([it.n for it in items], np.int32)
    caps = c._default_caps(torch.from_numpy(counts)).numpy().astype(np.int64)
    offs = GUARD + np.concatenate([[0], np.cumsum(caps + GUARD)[:-1]]).astype(np.int64)
    total = int(offs[-1] + caps[-1] + GUARD)
    out = torch.full((total,), SENTINEL, dtype=torch.uint8, device=dev)
    samples = torch.from_numpy(flat).to(dev)
    so = torch.from_numpy(np.array(starts, np.int64)).to(dev)
    cn = torch.from_numpy(counts).to(dev)
    enc = c.compress_batch(samples, so, cn, with_stats=stats, out=out, out_offsets=torch.from_numpy(offs).to(dev),
                           out_caps=torch.from_numpy(caps).to(dev))
    torch.cuda.synchronize()
    st = enc.status.cpu().numpy()
    sizes = enc.sizes.cpu().numpy()
    o = out.cpu().numpy()
    assert enc.blobs.data_ptr() == out.data_ptr()
    counters = enc.stats.cpu().numpy() if stats else None
    wrong = []
    guard = np.ones(total, bool)
    for i, it in enumerate(items):
        guard[offs[i]:offs[i] + caps[i]] = False
        want, wst = expect(codec, it)
        if st[i] != 0:
            wrong.append(f"{it.name}: status {st[i]}")
            continue
        got = o[offs[i]:offs[i] + sizes[i]].tobytes()
        if got != want:
            wrong.append(f"{it.name}: {diagnose(codec, it, got, want)}")
        if stats and not np.array_equal(counters[i], wst):
            wrong.append(f"{it.name}: stream counters {counters[i].tolist()}, oracle {wst.tolist()}")
    report(route, codec, wrong)
    assert (o[guard] == SENTINEL).all(), f"{route}, {codec}: bytes written between the capacities"
    # the GPU's own decode of what it wrote
    dec, dso, dst = c.decompress_batch(enc.blobs, enc.offsets, enc.sizes, cn)
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == 0).all(), route
    d, dso = dec.cpu().numpy(), dso.cpu().numpy()
    for i, it in enumerate(items):
        assert np.array_equal(d[dso[i]:dso[i] + it.n], it.x), f"{route}, {codec}: {it.name} decodes to other samples"


def small_batches(c, codec, cases, route, stats=False):
    """batches of at most 64 chunks: 32 cases and the far chunk behind each"""
    for i in range(0, len(cases), 32):
        items = with_far(cases[i:i + 32])
        assert len(items) <= 64
        run_batch(c, codec, items, route, stats)


def large_batches(c, codec, cases, route, stats=False, per=68, limit=None):
    """batches of 65 or more chunks (and at most `limit`): `per` cases and their far chunks; a short rest joins
    the batch before it"""
    cuts = list(range(0, len(cases), per))
    if len(cases) - cuts[-1] < 33 and len(cuts) > 1:
        cuts.pop()
    for k, a in enumerate(cuts):
        part = cases[a:cuts[k + 1]] if k + 1 < len(cuts) else cases[a:]
        items = with_far(part)
        if len(items) < 65:  # a family smaller than a batch: plain chunks up to 65
            items += [Item(f"plain_{j}", O.synth_read(7100 + j, 200 + 61 * j)) for j in range(65 - len(items))]
        assert len(items) >= 65 and (limit is None or len(items) <= limit)
        run_batch(c, codec, items, route, stats)


def forced(cls, pipeline, want):
    """a context created under PGN_ENC_PIPELINE=pipeline"""
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    old = os.environ.get("PGN_ENC_PIPELINE")
    os.environ["PGN_ENC_PIPELINE"] = pipeline
    try:
        c = cls(0)
    finally:
        if old is None:
            os.environ.pop("PGN_ENC_PIPELINE", None)
        else:
            os.environ["PGN_ENC_PIPELINE"] = old
    assert c.kernels(0) == want
    return c


@pytest.fixture(scope="module")
def staged():
    from rawnanoporesignalcompression_amd import PGNanoCodec

    c = forced(PGNanoCodec, "staged", STAGED)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fused():
    from rawnanoporesignalcompression_amd import PGNanoCodec

    c = forced(PGNanoCodec, "fused", FUSED)
    yield c
    c.close()


@pytest.fixture(scope="module")
def vbz():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rawnanoporesignalcompression_amd import VBZCodec

    c = VBZCodec(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def vbz_staged():
    from rawnanoporesignalcompression_amd import VBZCodec

    c = forced(VBZCodec, "staged", STAGED)
    yield c
    c.close()


@pytest.fixture(scope="module")
def vbz_fused():
    from rawnanoporesignalcompression_amd import VBZCodec

    c = forced(VBZCodec, "fused", FUSED)
    yield c
    c.close()


@pytest.fixture(scope="module")
def variants():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rawnanoporesignalcompression_amd import PGNanoCodec

    cs = {v: PGNanoCodec(0, variant=v) for v in VARIANTS}
    yield cs
    for c in cs.values():
        c.close()


def fam(family):
    bl = S.cases(family=family)
    assert bl
    return bl


def cu_count():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- C5, default context -------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", S.FAMILIES)
def test_c5_compress_signal_range_split(codec, family):
    """one chunk per call: 32 ranges; the chunk above 262,144 samples alone takes the large-chunk pass"""
    assert codec.kernels(0) == FUSED  # the default: staged below the CU count, fused from there
    check_single(codec, "C5", fam(family), "C5 compress_signal")


@pytest.mark.parametrize("family", S.FAMILIES)
def test_c5_batch_range_split(codec, family):
    small_batches(codec, "C5", fam(family), "C5 batch of at most 64 (range split)", stats=True)


@pytest.mark.parametrize("family", S.FAMILIES)
def test_c5_batch_wave_per_chunk(codec, family):
    """65 chunks to the CU count: the staged pipeline's enc_split_kernel, one wave per chunk"""
    large_batches(codec, "C5", fam(family), "C5 batch of 65 or more (enc_split_kernel)", stats=True, limit=cu_count())


def test_c5_large_chunk_alone_and_in_batches(codec):
    big = [c for c in S.cases(family="capacity") if c.n > S.PASS_SAMPLES]
    assert len(big) == 1
    run_batch(codec, "C5", [Item(big[0].name, big[0].x)], "C5 large chunk alone in a batch", stats=True)
    rest = S.cases(family="ragged")
    run_batch(codec, "C5", with_far(rest[:20] + big + rest[20:30]), "C5 large chunk in a small batch", stats=True)
    run_batch(codec, "C5", with_far(rest[:20] + big + rest[20:]), "C5 large chunk in a batch of 65 or more", stats=True)


def test_c5_range_split_twice_on_one_context(codec):
    """The look-back words carry the call's epoch: a second small batch, of other chunks in the same slots, must
    not read the first one's counts and nibbles."""
    a, b = S.cases(family="ranges", max_n=70000), S.cases(family="carries")
    k = min(len(a), len(b), 32)
    for _ in range(2):
        run_batch(codec, "C5", with_far(a[:k]), "C5 small batch, first catalogue")
        run_batch(codec, "C5", with_far(b[:k]), "C5 small batch, second catalogue in the same slots")
        run_batch(codec, "C5", with_far(b[k - 1::-1]), "C5 small batch, second catalogue reversed")


# ---- C5, forced contexts -------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", S.FAMILIES)
def test_c5_staged_context_wave_per_chunk(staged, family):
    assert staged.kernels(0) == STAGED
    large_batches(staged, "C5", fam(family), "C5 staged context, batch of 65 or more", stats=True)


def test_c5_staged_context_above_the_cu_count(staged):
    """one batch of every case up to 70,000 samples: more chunks than CUs, still the staged split"""
    items = with_far(S.cases(max_n=70000))
    assert len(items) > cu_count()
    run_batch(staged, "C5", items, "C5 staged context, whole catalogue in one batch", stats=True)


@pytest.mark.parametrize("family", S.FAMILIES)
def test_c5_fused_context(fused, family):
    """c5_split_wave inside enc_chunk_kernel, at every batch size"""
    assert fused.kernels(0) == FUSED
    bl = fam(family)
    small_batches(fused, "C5", bl, "C5 fused context, batch of at most 64", stats=True)
    large_batches(fused, "C5", bl, "C5 fused context, batch of 65 or more", stats=True)
    check_single(fused, "C5", bl[::5], "C5 fused context, compress_signal")


# ---- VBZ -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", S.FAMILIES)
def test_vbz_compress_signal(vbz, family):
    check_single(vbz, "VBZ", fam(family), "VBZ compress_signal")


@pytest.mark.parametrize("family", S.FAMILIES)
def test_vbz_batches(vbz, family):
    bl = fam(family)
    small_batches(vbz, "VBZ", bl, "VBZ batch of at most 64 (vbz_split_kernel)")
    large_batches(vbz, "VBZ", bl, "VBZ batch of 65 or more (vbz_split_kernel)", limit=cu_count())


@pytest.mark.parametrize("family", S.FAMILIES)
def test_vbz_staged_context(vbz_staged, family):
    assert vbz_staged.kernels(0) == STAGED
    large_batches(vbz_staged, "VBZ", fam(family), "VBZ staged context, batch of 65 or more")


@pytest.mark.parametrize("family", S.FAMILIES)
def test_vbz_fused_context(vbz_fused, family):
    assert vbz_fused.kernels(0) == FUSED
    bl = fam(family)
    small_batches(vbz_fused, "VBZ", bl, "VBZ fused context, batch of at most 64")
    large_batches(vbz_fused, "VBZ", bl, "VBZ fused context, batch of 65 or more")
    check_single(vbz_fused, "VBZ", bl[::5], "VBZ fused context, compress_signal")


# ---- C4, C1, C2, C3, VBZ0 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", S.FAMILIES)
@pytest.mark.parametrize("variant", VARIANTS)
def test_variant_compress_signal(variants, variant, family):
    check_single(variants[variant], variant, fam(family), f"{variant} compress_signal")


@pytest.mark.parametrize("family", S.FAMILIES)
@pytest.mark.parametrize("variant", VARIANTS)
def test_variant_batches(variants, variant, family):
    bl = fam(family)
    small_batches(variants[variant], variant, bl, f"{variant} batch of at most 64")
    large_batches(variants[variant], variant, bl, f"{variant} batch of 65 or more")
