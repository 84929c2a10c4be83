"""The GPU match search (csrc/pgn_zenc.h fast_search_wave) on streams built for its speculation
hazards: candidates written by the round's own visits, false fingerprints and the retry after one, a
false candidate that shares 3 of its 4 bytes with the position, first hits in the last lanes of a round,
backward extensions of 63 .. 129 bytes and up to the anchor, matches
that end at and just before the stream's end, repcode chains, both entry layouts and multi-block
frames.  tests/_search_cases.py builds the set and tests/test_search_profile.py checks on the host what
it reaches; here every chunk's blob must equal the oracle's (libzstd level 1) byte for byte -- a wrong
bound in the search still gives a valid frame, so no round trip would notice -- by three routes (one
batch of all chunks: one wave per chunk; batches of at most 64: the cooperative encode; compress_signal
per chunk), and again on a context with one encode slot per CU, whose tables hold stale entries of other
epochs and of the other entry layout.  Every GPU blob is decoded on the GPU too.  Needs an MI355X."""
import numpy as np
import pytest

import _search_cases as S
from test_gpu_hash_epochs import few_slots  # noqa: F401  (a context with one encode slot per CU)

pytestmark = pytest.mark.gpu

GROUPS = ("late_copy", "short_period", "word_soup", "small_alphabet", "runs", "uniform", "end", "back", "lane", "false3", "large")
FRAMES = ("keys", "S", "M", "Llow", "Lhigh")


def group(g):
    if g == "large":
        return list(S.large_cases())
    return [n for n in S.profiled_cases() if n.startswith(g + "/")]


def test_groups_cover_the_set():
    names = [n for g in GROUPS for n in group(g)]
    assert sorted(names) == sorted(S.cases()) and len(set(names)) == len(names)


def where(ref: bytes, i: int) -> str:
    """The frame of the blob [u64 cK][K][u64 cS][S][u64 cM][M][u64 cLl][Ll][Lh] that holds byte i."""
    p = 0
    for k, f in enumerate(FRAMES):
        if k < 4:
            if i < p + 8:
                return f"size field of the {f} frame"
            size = int.from_bytes(ref[p:p + 8], "little")
            p += 8
        else:
            size = len(ref) - p
        if i < p + size:
            return f"{f} frame, byte {i - p} of {size}"
        p += size
    return "past the oracle's blob"


def same(name, route, got: bytes, ref: bytes):
    if got == ref:
        return
    a, b = np.frombuffer(got, np.uint8), np.frombuffer(ref, np.uint8)
    m = min(a.size, b.size)
    d = np.flatnonzero(a[:m] != b[:m])
    i = int(d[0]) if d.size else m
    pytest.fail(f"{name} ({route}): {len(got)} bytes, the oracle {len(ref)}; first difference at byte {i} "
                f"({where(ref, i)}): {got[i:i + 8].hex()} != {ref[i:i + 8].hex()}", pytrace=False)


def encode_batch(c, names, route, chunk=None):
    """Encodes the chunks `names` in batches of `chunk` (all at once by default), compares every blob
    with the oracle's and decodes the GPU's blobs on the GPU."""
    import torch

    ref = S.reference()
    dev = torch.device("cuda", 0)
    assert names
    chunk = chunk or len(names)
    for a in range(0, len(names), chunk):
        part = names[a:a + chunk]
        xs = [ref[n][0] for n in part]
        lens = np.array([x.size for x in xs], np.int64)
        samples = torch.from_numpy(np.concatenate(xs)).to(dev)
        counts = torch.from_numpy(lens.astype(np.int32)).to(dev)
        offs = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)[:-1]])).to(dev)
        e = c.compress_batch(samples, offs, counts)
        out, oo, dst = c.decompress_batch(e.blobs, e.offsets, e.sizes, counts)
        torch.cuda.synchronize()
        est, eb, eo, es = e.status.cpu().numpy(), e.blobs.cpu().numpy(), e.offsets.cpu().numpy(), e.sizes.cpu().numpy()
        for i, n in enumerate(part):
            assert est[i] == 0, f"{n} ({route}): encode status {est[i]}"
            same(n, route, eb[eo[i]:eo[i] + es[i]].tobytes(), ref[n][1])
        dst, oo = dst.cpu().numpy(), oo.cpu().numpy()
        if not ((dst == 0).all() and torch.equal(out[: samples.numel()], samples)):
            out = out.cpu().numpy()
            for i, n in enumerate(part):
                assert dst[i] == 0, f"{n} ({route}): decode status {dst[i]}"
                assert np.array_equal(out[oo[i]:oo[i] + lens[i]], xs[i]), f"{n} ({route}): decoded samples differ"


def test_one_batch_of_all_chunks(codec):
    """More chunks than encode slots' worth of cooperation: one wave per chunk."""
    names = list(S.cases())
    assert len(names) > 64
    encode_batch(codec, names, "one batch of all chunks")


@pytest.mark.parametrize("g", GROUPS)
def test_batches_of_at_most_64(codec, g):
    """Few chunks per launch: the cooperative encode."""
    encode_batch(codec, group(g), "batch of <= 64", 64)


@pytest.mark.parametrize("g", GROUPS)
def test_compress_signal_per_chunk(codec, g):
    """Every directed case, and the case of each generator at each size."""
    ref = S.reference()
    names = [n for n in group(g) if not n.startswith("uniform/uncertified")]
    assert names
    for n in names:
        x = ref[n][0]
        blob = codec.compress_signal(x)
        same(n, "compress_signal", blob, ref[n][1])
        assert np.array_equal(codec.decompress_signal(blob, sample_count=x.size), x), f"{n} (compress_signal): decode"


def test_few_slots_in_order(few_slots):
    encode_batch(few_slots, list(S.cases()), "one slot per CU, in order")


def test_few_slots_shuffled(few_slots):
    """Over the tables the launches before left behind: every lookup also meets entries of other
    epochs and of the other entry layout."""
    names = list(S.cases())
    order = np.random.default_rng(77).permutation(len(names))
    encode_batch(few_slots, [names[i] for i in order], "one slot per CU, shuffled")
