"""Cases for the BGZF deflate call (include/pgnano_hip.h "BGZF deflate"), built once for the CPU tests
(tests/test_bgzf_deflate_api.py) and the GPU tests (tests/test_gpu_bgzf_deflate.py).

Every builder asserts here, on the CPU, the condition its case exists for (a code that needs the limiter, a run of
lengths coded with a given symbol, a payload on a given side of the stored/dynamic break-even, a capacity one byte
short of a block's end), from the host model's own outputs: a case list that drifts fails without a GPU.
"""
import functools
from dataclasses import dataclass

import numpy as np

import _bam_cases
import _fastq_cases
from rawnanoporesignalcompression_amd import _native
from rawnanoporesignalcompression_amd.host import (_deflate_dynamic, _length_symbols, bgzf_bound, bgzf_deflate_signal,
                                                   deflate_block_signal, deflate_lengths_signal)

B = _native.PGN_BGZF_BLOCK_BYTES
W_CASES = (0, 1, B - 1, B, B + 1, 2 * B, 3 * B + 777)
OFFSETS = (0, 1, 15)


@dataclass
class Case:
    name: str
    data: bytes               # the source buffer: src_capacity bytes
    nbytes: int = None        # the value behind d_nbytes; None: a NULL pointer
    byte_capacity: int = None  # None: bgzf_bound(src_capacity)
    src_offset: int = 0       # bytes between a 16-byte address and the source
    out_offset: int = 0       # bytes between a 16-byte address and out

    @property
    def W(self):
        return len(self.data) if self.nbytes is None else min(self.nbytes, len(self.data))

    @property
    def capacity(self):
        return bgzf_bound(len(self.data)) if self.byte_capacity is None else self.byte_capacity

    @property
    def ntiles(self):
        return -(-len(self.data) // B)

    def expected(self):
        """``(file bytes, blk_off of ntiles + 1 entries, written)``."""
        data, off, written = _model(self.data[:self.W], self.capacity)
        full = np.full(self.ntiles + 1, off[-1], np.uint64)
        full[:len(off)] = off
        assert len(data) == int(written[1]) <= self.capacity
        return data, full, written


@functools.lru_cache(maxsize=None)
def _model(stream, capacity):
    return bgzf_deflate_signal(stream, capacity)


def counts_of(p):
    return np.bincount(np.frombuffer(p, np.uint8), minlength=256).tolist() + [1]


def is_stored(p):
    body = deflate_block_signal(p)
    stored = len(body) == len(p) + 5 and body[0] == 1
    assert stored == (len(_deflate_dynamic(p)) >= len(p) + 5)
    return stored


def payload_of(cnt, seed):
    """A shuffled payload with the byte counts ``cnt``."""
    p = np.repeat(np.arange(len(cnt)), cnt).astype(np.uint8)
    np.random.default_rng(seed).shuffle(p)
    return p.tobytes()


# ---- payloads ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bam_stream():
    """The raw records of _bam_cases.long_read(): packed bases, qualities and a move table over ten blocks."""
    stream = _bam_cases.long_read().expected("raw")[1]
    assert len(stream) > 9 * B and not any(is_stored(stream[k:k + B]) for k in range(0, len(stream), B))
    return stream


@functools.lru_cache(maxsize=None)
def fastq_text():
    c = _fastq_cases.make("text", [3000] * 30 + [17, 1, 250], 71, tags=[("qs", list(range(33))), ("ch", list(range(100, 133)))])
    text = c.expected()[0]
    assert 2 * B < len(text) < 4 * B and text[:1] == b"@" and not is_stored(text[:B])
    return text


def zeros():
    p = bytes(B + 100)
    ll = deflate_lengths_signal(counts_of(p[:B]), 15)
    assert ll[0] == 1 and ll[256] == 1 and sum(ll) == 2, "two symbols of length 1"
    return Case("zeros", p)


def tiny(n):
    p = bytes(range(65, 65 + n))
    assert is_stored(p)
    return Case(f"tiny-{n}", p)


def uniform():
    p = np.random.default_rng(72).integers(0, 256, B + 3000).astype(np.uint8).tobytes()
    assert is_stored(p[:B]) and is_stored(p[B:])
    return Case("uniform", p)


def every_value():
    """All 256 values, skewed, so that the dynamic block wins with no zero length to run over."""
    cnt = [10 + (7919 * s) % 101 + (2800 if s % 16 == 0 else 0) for s in range(256)]
    p = payload_of(cnt, 73)
    ll = deflate_lengths_signal(counts_of(p), 15)
    assert len(p) <= B and all(ll) and not is_stored(p)
    return Case("every-value", p)


def two_values():
    """Only 0 and 255: the 254 zero lengths between them are coded 18(138) 18(116)."""
    p = (np.random.default_rng(74).integers(0, 2, B) * 255).astype(np.uint8).tobytes()
    syms = _length_symbols(deflate_lengths_signal(counts_of(p), 15))
    assert [s for s in syms if s[0] == 18] == [(18, 138 - 11, 7), (18, 116 - 11, 7)] and not is_stored(p)
    return Case("two-values", p)


def equal_lengths():
    """64 equiprobable values in groups of 1, 8, 9 and 46 neighbours: runs of equal non-zero lengths through symbol
    16, with leftovers of 1 and 2 literal lengths."""
    values = [0] + list(range(2, 10)) + list(range(11, 20)) + list(range(21, 67))
    assert len(values) == 64
    cnt = [0] * 256
    for v in values:
        cnt[v] = B // 64
    p = payload_of(cnt, 75)
    ll = deflate_lengths_signal(counts_of(p), 15)
    assert len(p) == B and len(set(ll[2:10])) == 1 and len(set(ll[11:20])) == 1 and ll[2] > 0
    syms = _length_symbols(ll)
    v = ll[2]
    flat = [s[:2] for s in syms]
    at = flat.index((v, 0), 1)                              # behind value 0's own length and a zero
    assert flat[at:at + 3] == [(v, 0), (16, 3), (v, 0)], "a run of 8: the length, 16 for six, one literal"
    assert flat[at + 4:at + 8] == [(v, 0), (16, 3), (v, 0), (v, 0)], "a run of 9: the length, 16 for six, two literals"
    return Case("equal-lengths", p)


def deep_histogram():
    """Counts 1, 2, 4, 7, 12, ... (c_k = c_{k-1} + c_{k-2} + 1): an unrestricted depth of 20 within a block."""
    c = [1, 2]
    while len(c) < 20:
        c.append(c[-1] + c[-2] + 1)
    p = payload_of(c, 76)
    cnt = counts_of(p)
    assert len(p) == 46345 and max(deflate_lengths_signal(cnt, 64)) == 20
    ll = deflate_lengths_signal(cnt, 15)
    assert max(ll) == 15 and sum(2.0 ** -v for v in ll if v) == 1.0 and not is_stored(p)
    return Case("deep-histogram", p)


def limited_header():
    """A payload whose code-length symbols need the limit of 7, by a seeded search over skewed histograms."""
    rng = np.random.default_rng(77)
    for _ in range(200):
        k = int(rng.integers(40, 257))
        cnt = np.zeros(256, np.int64)
        cnt[rng.choice(256, k, replace=False)] = 1 + (rng.pareto(0.6, k) * 2).astype(np.int64) % 4000
        cnt = (cnt * min(1.0, B / cnt.sum())).astype(np.int64)
        if not cnt.sum():
            continue
        p = payload_of(cnt.tolist(), 78)
        clcnt = [0] * 19
        for s, _, _ in _length_symbols(deflate_lengths_signal(counts_of(p), 15)):
            clcnt[s] += 1
        if max(deflate_lengths_signal(clcnt, 64)) > 7:
            cl = deflate_lengths_signal(clcnt, 7)
            assert max(cl) == 7 and sum(2.0 ** -v for v in cl if v) == 1.0
            return Case("limited-header", p)
    raise AssertionError("no histogram found whose code-length code is deeper than 7")


def break_even():
    """Payloads whose dynamic block is one byte shorter than the stored block, exactly as long (the tie stores) and
    one byte longer, by a seeded search."""
    rng = np.random.default_rng(79)
    found = {}
    for _ in range(4000):
        n = int(rng.integers(20, 400))
        p = rng.integers(0, int(rng.integers(2, 257)), n).astype(np.uint8).tobytes()
        d = len(_deflate_dynamic(p)) - (n + 5)
        if d in (-1, 0, 1) and d not in found:
            found[d] = p
        if len(found) == 3:
            break
    assert sorted(found) == [-1, 0, 1], sorted(found)
    assert not is_stored(found[-1]) and is_stored(found[0]) and is_stored(found[1])
    return [Case(f"break-even{d:+d}", found[d]) for d in (-1, 0, 1)]


# ---- stream lengths, alignments, capacities, d_nbytes ---------------------------------------------------------------
def mixed(W):
    """W bytes that change kind at the blocks' seams: records, random bytes, text, records."""
    parts = [bam_stream()[:B], uniform().data[:B], fastq_text()[:B], bam_stream()[B:2 * B]]
    return b"".join(parts)[:W]


def stream_lengths():
    out = [Case(f"w-{W}", mixed(W)) for W in W_CASES]
    data, off, written = out[-1].expected()
    assert np.diff(off.astype(np.int64)).tolist()[1] == B + 31 and len(set(np.diff(off.astype(np.int64)).tolist())) == 4
    return out


def alignments():
    return [Case(f"align-{s}-{o}", mixed(B + 100), src_offset=s, out_offset=o) for s in OFFSETS for o in OFFSETS if s or o]


def capacity_cases():
    """A capacity at a block's end, one byte short of it and one byte past it, in the middle and at the stream's end,
    and 0."""
    p = mixed(3 * B + 777)
    _, off, _ = Case("all", p).expected()
    off = off.astype(np.int64).tolist()
    out = []
    for label, cap, kw in (("at", off[2], 2), ("short", off[2] - 1, 1), ("past", off[2] + 1, 2), ("total", off[4], 4),
                           ("total-short", off[4] - 1, 3), ("first-short", off[1] - 1, 0), ("zero", 0, 0)):
        c = Case(f"capacity-{label}", p, byte_capacity=cap, out_offset=1 if label == "short" else 0)
        data, off2, written = c.expected()
        assert off2.tolist() == off and written.tolist() == [min(len(p), kw * B), off[kw]] and len(data) == off[kw], label
        out.append(c)
    return out


def nbytes_cases():
    p = mixed(2 * B + 50)
    out = [Case("nbytes-below", p, nbytes=B + 7), Case("nbytes-above", p, nbytes=len(p) + 1000), Case("nbytes-zero", p, nbytes=0),
           Case("nbytes-equal", p, nbytes=len(p))]
    data, off, written = out[0].expected()
    assert written.tolist()[0] == B + 7 and len(off) == 4 and off[2] == off[3] == len(data), "entries above nblocks repeat the total"
    assert out[1].expected()[0] == out[3].expected()[0] == Case("n", p).expected()[0]
    assert out[2].expected()[0] == b"" and not out[2].expected()[1].any()
    return out


@functools.lru_cache(maxsize=None)
def deflate_cases():
    """Every case of the deflate call, built once a process; nothing changes a case."""
    cases = [Case("bam", bam_stream()), Case("fastq", fastq_text()), zeros(), tiny(1), tiny(2), uniform(), every_value(),
             two_values(), equal_lengths(), deep_histogram(), limited_header()] + break_even()
    cases += stream_lengths() + alignments() + capacity_cases() + nbytes_cases()
    names = [c.name for c in cases]
    assert len(set(names)) == len(names), names
    return cases
