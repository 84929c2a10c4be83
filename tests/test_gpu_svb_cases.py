"""Every merge route on the stream sets of tests/_svb_cases.py: keys with set tail codes, frames cut
elsewhere, streams that read on into the next one, streams too long and too short, the VBZ padding
edges.  tests/test_svb_cases.py holds the catalogue to the oracle and the reference on the CPU; here the
status must be the oracle's for every chunk, crafted or padding, on every route, and the samples the
oracle's wherever its status is 0.

Routes.  C5: decompress_signal; batches of at most 64 (the 32-range look-back merge) and of 65 or more
(one wave per chunk), each also through the bounded call, where no claims pass follows and the staged
merge's result is final; the fused kernel through the 263,173-sample cases in a mixed batch and, for the
whole catalogue, through a context created with PGN_DEC_PIPELINE=fused; the claims == True cases in an
unbounded batch (the claims pass).  C4, C1, C2, C3, VBZ0: decompress_signal and mixed batches.  VBZ:
decompress_signal, batches of at most 64 and of 65 or more, unbounded (every VBZ chunk that decodes is
a claims chunk, so the fused kernel has the last word there) and bounded (the staged VBZ merge has it),
and the 263,173-sample cases.  decompress_batch_pa in float32 and float16 for all seven codecs.

Every batch decodes into a tensor with a sentinel pattern before the first and after the last chunk;
both must be intact afterwards, status-6 chunks or not.
"""
import os

import numpy as np
import pytest

import _oracle as O
import _svb_cases as S
from test_gpu_zframes import compare, decode_single, padding, vbz  # noqa: F401  (vbz: the VBZCodec fixture)

pytestmark = pytest.mark.gpu

VARIANTS = ["C4", "C1", "C2", "C3", "VBZ0"]
C5_FAMILIES = [f for f in S.FAMILIES if "C5" in S.APPLIES[f]]
VBZ_FAMILIES = [f for f in S.FAMILIES if "VBZ" in S.APPLIES[f]]
PA_FAMILIES = ("exact", "tail", "recut", "borrow", "empty")
GUARD = 4096
PASS_SAMPLES = 262144


class Plain:
    def __init__(self, name, codec, x):
        self.name, self.n = name, x.size
        self.blob = O.variant_compress(codec, x)[1]
        self.rc, self.want = O.variant_decompress(codec, self.blob, x.size)
        assert self.rc == 0


_PLAIN = {}


def plain(codec, count):
    """Ordinary oracle blobs to share workgroups and passes with the crafted ones."""
    if codec in ("C5", "VBZ"):
        return padding(codec == "VBZ", count)
    if codec not in _PLAIN:
        _PLAIN[codec] = [Plain(f"plain_{i}", codec, O.synth_read(7000 + i, 300 + 79 * i)) for i in range(72)]
    return _PLAIN[codec][:count]


def mixed(bl, codec, at_least):
    """bl interleaved with plain blobs, then plain ones up to at_least chunks"""
    pad = plain(codec, 72)
    part = [x for pair in zip(bl, pad * (len(bl) // 72 + 1)) for x in pair]
    return part + pad[: max(at_least - len(part), 8)]


def run_batch(c, bl, bound=None, dtype=None, cal=None):
    """Decode bl in one call into a guarded tensor: (per-chunk outputs, statuses)."""
    import torch

    dev = torch.device("cuda", 0)
    sizes = np.array([len(b.blob) for b in bl], np.int64)
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    flat = np.frombuffer(b"".join(b.blob for b in bl), np.uint8).copy()
    counts = np.array([b.n for b in bl], np.int32)
    so = GUARD + np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
    tdt = dtype or torch.int16
    sentinel = 23130 if tdt == torch.int16 else 1234.0
    out = torch.full((int(so[-1]) + GUARD,), sentinel, dtype=tdt, device=dev)
    args = (torch.from_numpy(flat).to(dev), torch.from_numpy(offs).to(dev), torch.from_numpy(sizes).to(dev),
            torch.from_numpy(counts).to(dev))
    kw = dict(out=out, out_offsets=torch.from_numpy(so[:-1].copy()).to(dev))
    if dtype is None and bound is None:
        _, _, st = c.decompress_batch(*args, **kw)
    else:
        co, cs = (None, None) if cal is None else (torch.from_numpy(cal[0]).to(dev), torch.from_numpy(cal[1]).to(dev))
        _, _, st = c.decompress_batch_pa(*args, co, cs, dtype=tdt, max_chunk_samples=bound, **kw)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    want = np.asarray(sentinel, o.dtype)
    assert (o[:GUARD] == want).all(), "samples written before the first chunk"
    assert (o[int(so[-1]):] == want).all(), "samples written after the last chunk"
    return [o[so[i]:so[i + 1]] for i in range(len(bl))], st.cpu().numpy()


def in_batches(c, bl, codec, route, size=40, **kw):
    """bl in batches of at most 64 chunks: `size` crafted ones and plain ones to 64"""
    for i in range(0, len(bl), size):
        part = bl[i:i + size]
        part = part + plain(codec, 64 - len(part))
        assert len(part) <= 64
        compare(part, *run_batch(c, part, **kw), route)


def check_single(c, bl, route):
    res = [decode_single(c, b) for b in bl]
    compare(bl, [r[0] for r in res], [r[1] for r in res], route)


def fam(codec, family, max_n=None):
    bl = S.cases(codec=codec, family=family, max_n=max_n)
    assert bl
    return bl


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


@pytest.fixture(scope="module")
def fused():
    """A context whose C5 decode is the fused per-chunk kernel at every size."""
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rawnanoporesignalcompression_amd import PGNanoCodec

    keys = ("PGN_DEC_PIPELINE",)
    old = {k: os.environ.get(k) for k in keys}
    os.environ["PGN_DEC_PIPELINE"] = "fused"
    try:
        c = PGNanoCodec(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    assert c.kernels(1) == "dec_chunk_kernel<C5>"
    yield c
    c.close()


# ---- C5 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", C5_FAMILIES)
def test_c5_decompress_signal(codec, family):
    check_single(codec, fam("C5", family), "C5 decompress_signal")


@pytest.mark.parametrize("bound", [None, PASS_SAMPLES])
@pytest.mark.parametrize("family", C5_FAMILIES)
def test_c5_batch_lookback_ranges(codec, family, bound):
    """At most 64 chunks: 32 single-wave ranges per chunk, whose class counts, delta sums and merges must
    mask the tail codes and bound their reads alike."""
    bl = fam("C5", family, PASS_SAMPLES if bound else None)
    in_batches(codec, bl, "C5", f"C5 batch of at most 64, bound {bound}", bound=bound)
    assert "dec_merge_kernel" in codec.kernels(1)  # the staged pipeline (the look-back kernel is its small-batch merge)


@pytest.mark.parametrize("bound", [None, PASS_SAMPLES])
@pytest.mark.parametrize("family", C5_FAMILIES)
def test_c5_batch_wave_per_chunk(codec, family, bound):
    part = mixed(fam("C5", family, PASS_SAMPLES if bound else None), "C5", 70)
    assert len(part) >= 65
    compare(part, *run_batch(codec, part, bound=bound), f"C5 batch of 65 or more, bound {bound}")


def test_c5_fused_kernel_large_chunks_in_a_mixed_batch(codec):
    big = [c for c in S.cases(codec="C5") if c.n > PASS_SAMPLES]
    assert len(big) >= 2 and {c.family for c in big} == {"exact", "borrow"}
    part = mixed(big + fam("C5", "corrupt")[:6] + fam("C5", "remaining")[:6], "C5", 70)
    compare(part, *run_batch(codec, part), "C5 large chunks in a mixed batch")
    part = big + plain("C5", 10)
    compare(part, *run_batch(codec, part), "C5 large chunks in a small batch")


@pytest.mark.parametrize("family", C5_FAMILIES)
def test_c5_fused_context(fused, family):
    bl = fam("C5", family)
    part = mixed(bl, "C5", 70)
    compare(part, *run_batch(fused, part), "C5 fused context, batch of 65 or more")
    in_batches(fused, bl[:40], "C5", "C5 fused context, batch of at most 64")
    check_single(fused, bl[::7], "C5 fused context, decompress_signal")


def test_c5_claims_pass(codec):
    bl = [c for c in S.cases(codec="C5") if c.claims]
    assert len(bl) >= 10 and {0, 4} <= {c.rc for c in bl}
    part = mixed(bl, "C5", 70)
    compare(part, *run_batch(codec, part), "C5 claims pass, batch of 65 or more")
    in_batches(codec, bl, "C5", "C5 claims pass, batch of at most 64")


# ---- C4, C1, C2, C3, VBZ0 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_variant_decompress_signal(variants, variant):
    check_single(variants[variant], S.cases(codec=variant), f"{variant} decompress_signal")


@pytest.mark.parametrize("bound", [None, PASS_SAMPLES])
@pytest.mark.parametrize("variant", VARIANTS)
def test_variant_mixed_batch(variants, variant, bound):
    """Every family in one batch of 70 or more; the bounded call (through decompress_batch_pa's int16
    output) has no claims pass."""
    import torch

    bl = S.cases(codec=variant, max_n=PASS_SAMPLES if bound else None)
    assert {c.family for c in bl} == {f for f in S.FAMILIES if variant in S.APPLIES[f]}
    part = mixed(bl, variant, 70)
    assert len(part) >= 70
    kw = dict(bound=bound, dtype=torch.int16) if bound else {}
    compare(part, *run_batch(variants[variant], part, **kw), f"{variant} mixed batch, bound {bound}")
    in_batches(variants[variant], bl[::5], variant, f"{variant} batch of at most 64, bound {bound}", **kw)


# ---- VBZ --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", VBZ_FAMILIES)
def test_vbz_decompress_signal(vbz, family):  # noqa: F811
    check_single(vbz, fam("VBZ", family), "VBZ decompress_signal")


@pytest.mark.parametrize("bound", [None, PASS_SAMPLES])
@pytest.mark.parametrize("family", VBZ_FAMILIES)
def test_vbz_batches(vbz, family, bound):  # noqa: F811
    import torch

    bl = fam("VBZ", family, PASS_SAMPLES if bound else None)
    kw = dict(bound=bound, dtype=torch.int16) if bound else {}
    in_batches(vbz, bl, "VBZ", f"VBZ batch of at most 64, bound {bound}", **kw)
    part = mixed(bl, "VBZ", 70)
    assert len(part) >= 65
    compare(part, *run_batch(vbz, part, **kw), f"VBZ batch of 65 or more, bound {bound}")


def test_vbz_large_chunks(vbz):  # noqa: F811
    big = [c for c in S.cases(codec="VBZ") if c.n > PASS_SAMPLES]
    assert big
    check_single(vbz, big, "VBZ decompress_signal, large chunk")
    part = mixed(big, "VBZ", 70)
    compare(part, *run_batch(vbz, part), "VBZ large chunks in a mixed batch")


# ---- calibrated output ------------------------------------------------------------------------------------
def _pa_check(c, part, dtype, route):
    import torch

    k = np.arange(len(part))
    off = (-300.0 + 7.0 * k).astype(np.float32)
    scale = (0.1 + 0.001 * k).astype(np.float32)
    got, st = run_batch(c, part, dtype=dtype, cal=(off, scale))
    npdt, bits = (np.float32, np.uint32) if dtype == torch.float32 else (np.float16, np.uint16)
    wrong = []
    for i, (b, g, s) in enumerate(zip(part, got, st)):
        if int(s) != b.rc:
            wrong.append(f"{b.name}: status {int(s)}, oracle {b.rc}")
        elif b.rc == 0:
            want = (b.want.astype(np.float32) + np.float32(off[i])) * np.float32(scale[i])
            if dtype == torch.float16:
                want = want.astype(np.float16)
            assert want.dtype == npdt and g.dtype == npdt
            if not np.array_equal(g.view(bits), want.view(bits)):
                wrong.append(f"{b.name}: values differ")
    assert not wrong, f"{route}: " + "; ".join(wrong[:12]) + (f" (+{len(wrong) - 12} more)" if len(wrong) > 12 else "")


@pytest.mark.parametrize("dtype", ["float32", "float16"])
@pytest.mark.parametrize("name", S.CODECS)
def test_calibrated_output(codec, variants, vbz, name, dtype):  # noqa: F811
    """(want.astype(float32) + float32(off)) * float32(scale) bit for bit, float16 that value rounded
    once; another offset and scale for every chunk."""
    import torch

    c = codec if name == "C5" else (vbz if name == "VBZ" else variants[name])
    dt = getattr(torch, dtype)
    bl = [b for b in S.cases(codec=name) if b.family in PA_FAMILIES]
    assert {b.family for b in bl} == {f for f in PA_FAMILIES if name in S.APPLIES[f]}
    _pa_check(c, mixed(bl, name, 70), dt, f"{name} {dtype}, batch of 65 or more")
    if name == "C5":  # the look-back merge's sinks
        for i in range(0, len(bl), 50):
            _pa_check(c, bl[i:i + 50] + plain(name, 14), dt, f"{name} {dtype}, batch of at most 64")


# ---- containment ------------------------------------------------------------------------------------------
def test_status_6_chunks_write_inside_their_own_samples(codec, variants, vbz):  # noqa: F811
    """Batches of nothing but status-6 chunks between two status-0 ones: the sentinels around the output
    stay (run_batch asserts it) and the neighbours keep their samples."""
    for name in S.CODECS:
        c = codec if name == "C5" else (vbz if name == "VBZ" else variants[name])
        bad = [b for b in S.cases(codec=name) if b.rc == 6]
        assert len(bad) >= 4, name
        ok = plain(name, 2)
        for part in ([ok[0]] + bad[:60] + [ok[1]], [ok[0]] + bad + bad + bad + [ok[1]]):
            compare(part, *run_batch(c, part), f"{name} status-6 batch of {len(part)}")
