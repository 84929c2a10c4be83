"""The on-chip search of small single-block frames (csrc/pgn_zenc.h small_search_wave) on the GPU:
every stream of tests/_small_search_cases.py -- the generators at the lengths around a round and the
bound, bench reads' Lhigh streams, the built hazards, streams of long runs and matches at the block's end
at 2,047 and 2,048 bytes (the exact search run to the bound: a noise-like block of that size either passes
the certificate or overflows the log), the streams that overflow the search's log and the one a byte too
large for it -- is the Lhigh stream of a chunk whose samples are all of class 3.  Each
chunk's blob must equal the oracle's (libzstd level 1) byte for byte, by the three routes of
test_gpu_search.py (one batch of all chunks: one wave per chunk; batches of at most 64: the cooperative
encode; compress_signal per chunk), and on a context with one encode slot per CU, where the general
search of the overflowing and the larger chunks follows small searches that never touched the slot's
hash table: its epoch tags must still be right.  Every GPU blob is decoded on the GPU too.  What the
streams reach is checked on the host (test_small_search_model.py).  Needs an MI355X."""
import numpy as np
import pytest

import _small_search_cases as SS
from test_gpu_hash_epochs import few_slots  # noqa: F401  (a context with one encode slot per CU)
from test_gpu_search import same

pytestmark = pytest.mark.gpu


def encode_batch(c, names, route, chunk=None):
    """Encodes the chunks `names` in batches of `chunk` (all at once by default), compares every blob
    with the oracle's and decodes the GPU's blobs on the GPU."""
    import torch

    ref = SS.reference()
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
        dst, oo, out = dst.cpu().numpy(), oo.cpu().numpy(), out.cpu().numpy()
        for i, n in enumerate(part):
            assert dst[i] == 0, f"{n} ({route}): decode status {dst[i]}"
            assert np.array_equal(out[oo[i]:oo[i] + lens[i]], xs[i]), f"{n} ({route}): decoded samples differ"


def test_one_batch_of_all_chunks(codec):
    names = list(SS.cases())
    assert len(names) > 64 and "overflow/small_alphabet" in names and "beyond/runs" in names
    encode_batch(codec, names, "one batch of all chunks")


def test_batches_of_at_most_64(codec):
    """Few chunks per launch: the cooperative encode, whose wave 0 runs the search."""
    encode_batch(codec, list(SS.cases()), "batch of <= 64", 64)


def test_compress_signal_per_chunk(codec):
    ref = SS.reference()
    for n, (x, blob) in ref.items():
        got = codec.compress_signal(x)
        same(n, "compress_signal", got, blob)
        assert np.array_equal(codec.decompress_signal(got, sample_count=x.size), x), f"{n} (compress_signal): decode"


def test_few_slots_general_after_small(few_slots):
    """One encode slot per CU, the chunks in an order that puts the overflowing and the larger chunks
    (general search, hash table) between runs of small searches (no table), three times over: a slot's
    table meets the entries of its earlier epochs."""
    names = list(SS.cases())
    order = np.random.default_rng(78).permutation(len(names))
    mixed = [names[i] for i in order]
    general = ["overflow/small_alphabet", "beyond/runs"] + [n for n in SS.generated_cases() if n.endswith("/2048")]
    seq = []
    for k in range(3):
        seq += mixed[k::3] + general
    encode_batch(few_slots, seq, "one slot per CU, general after small")
