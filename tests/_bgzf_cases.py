"""Cases for the BGZF deflate call (include/pgnano_hip.h "BGZF deflate"), built once for the CPU tests
(tests/test_bgzf_deflate_api.py) and the GPU tests (tests/test_gpu_bgzf_deflate.py): deflate_cases(), the call's
surface (lengths, alignments, capacities, ``nbytes``, one block of each kind), and hazard_cases(), single blocks built
for what the kernels can get wrong without a file of records ever showing it: the limiter's two tie orders at both
limits, the merge's ties, every run length at which the code-length symbols change, HCLEN, and the pack kernel's
longest and shortest runs of bits, its whole/byte-wise split and every alignment.

Every builder asserts here, on the CPU, the condition its case exists for (a code that needs the limiter, a run of
lengths coded with a given symbol, a payload on a given side of the stored/dynamic break-even, a capacity one byte
short of a block's end), from the host model's own outputs: a case list that drifts fails without a GPU.
"""
import functools
import time
from dataclasses import dataclass, field

import numpy as np

import _bam_cases
import _fastq_cases
from rawnanoporesignalcompression_amd import _native
from rawnanoporesignalcompression_amd.host import (_CL_ORDER, _deflate_dynamic, _length_symbols, bgzf_bound,
                                                   bgzf_deflate_signal, deflate_block_signal, deflate_lengths_signal)

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


# ---- hazard cases: what the model computes for a block, and traces of its two serial loops ---------------------------
@dataclass
class Plan:
    ll: list            # the literal code's lengths, 257
    syms: list          # the code-length symbols of ll, 1, 1
    clcnt: list         # their histogram, 19
    cl: list            # the code-length code's lengths
    hclen: int
    hdr_bits: int       # the bits in front of the first literal
    lit_bits: int       # the literals' bits, without the end of block


@functools.lru_cache(maxsize=None)
def plan_of(p):
    """The model's codes for the payload ``p``, and its bit counts (held to the model's own byte length)."""
    cnt = counts_of(p)
    ll = deflate_lengths_signal(cnt, 15)
    syms = _length_symbols(ll)
    clcnt = [0] * 19
    for s, _, _ in syms:
        clcnt[s] += 1
    cl = deflate_lengths_signal(clcnt, 7)
    hclen = max(4, max(i + 1 for i, s in enumerate(_CL_ORDER) if cl[s]))
    hdr_bits = 17 + 3 * hclen + sum(cl[s] + ebits for s, _, ebits in syms)
    lit_bits = sum(c * v for c, v in zip(cnt[:256], ll))
    assert (hdr_bits + lit_bits + ll[256] + 7) // 8 == len(_deflate_dynamic(p))
    return Plan(ll, syms, clcnt, cl, hclen, hdr_bits, lit_bits)


def kraft_is_one(lens, limit):
    return sum(1 << (limit - v) for v in lens if v) == 1 << limit


@dataclass
class LimiterTrace:
    needed: bool                                  # the unlimited code is deeper than the limit
    depth: int = 0                                # of the unlimited code
    p1_steps: int = 0
    p1_ties: list = field(default_factory=list)   # per step with one: the candidates that share the winning (length, count)
    p1_deep: int = 0                              # steps that picked a length below L - 1
    p2_steps: int = 0
    p2_ties: list = field(default_factory=list)   # per step with one: the candidates that share the winning count

    @property
    def ties(self):
        return self.p1_ties + self.p2_ties


def trace_limiter(cnt, L):
    """The rule's two limiter loops run again on the unlimited lengths, step by step, with what each step met; the
    result is held to ``deflate_lengths_signal(cnt, L)``."""
    cnt = [int(c) for c in cnt]
    free = deflate_lengths_signal(cnt, 64)
    t = LimiterTrace(max(free, default=0) > L, max(free, default=0))
    if not t.needed:
        assert deflate_lengths_signal(cnt, L) == free
        return t
    used = [s for s, c in enumerate(cnt) if c]
    out = [min(v, L) for v in free]
    K = sum(1 << (L - out[s]) for s in used)
    while K > 1 << L:
        cand = [s for s in used if out[s] < L]
        top = max((out[s], -cnt[s]) for s in cand)
        tied = [s for s in cand if (out[s], -cnt[s]) == top]
        s = tied[-1]                                        # the largest symbol
        t.p1_steps += 1
        t.p1_deep += out[s] < L - 1
        if len(tied) > 1:
            t.p1_ties.append(tied)
        K -= 1 << (L - out[s] - 1)
        out[s] += 1
    D = (1 << L) - K
    while D > 0:
        cand = [s for s in used if out[s] > 1 and 1 << (L - out[s]) <= D]
        top = max(cnt[s] for s in cand)
        tied = [s for s in cand if cnt[s] == top]
        s = tied[0]                                         # the smallest symbol
        t.p2_steps += 1
        if len(tied) > 1:
            t.p2_ties.append(tied)
        D -= 1 << (L - out[s])
        out[s] -= 1
    assert out == deflate_lengths_signal(cnt, L), "the trace follows the model"
    return t


def trace_merge(cnt):
    """The two-queue merge again: per step, for either pick, whether a leaf and an internal node of equal weight stood
    at the queues' fronts (the rule takes the leaf).  The depths are held to the model's unlimited lengths."""
    cnt = [int(c) for c in cnt]
    leaves = sorted((c, s) for s, c in enumerate(cnt) if c > 0)
    m = len(leaves)
    assert m > 1
    w = [c for c, _ in leaves] + [0] * (m - 1)
    parent = [0] * (2 * m - 1)
    li, ii, steps = 0, m, []
    for nxt in range(m, 2 * m - 1):
        pair, ties = [], []
        for _ in range(2):
            ties.append(li < m and ii < nxt and w[li] == w[ii])
            if li < m and (ii >= nxt or w[li] <= w[ii]):
                pair.append(li)
                li += 1
            else:
                pair.append(ii)
                ii += 1
        w[nxt] = w[pair[0]] + w[pair[1]]
        parent[pair[0]] = parent[pair[1]] = nxt
        steps.append(tuple(ties))
    depth = [0] * (2 * m - 1)
    for i in range(2 * m - 3, -1, -1):
        depth[i] = depth[parent[i]] + 1
    free = deflate_lengths_signal(cnt, 64)
    assert all(free[s] == depth[i] for i, (_, s) in enumerate(leaves)), "the trace follows the model"
    return steps


def has_run(syms, expected, group):
    """Whether the symbols hold ``expected`` as one whole run: bounded on both sides by symbols outside ``group``."""
    k = len(expected)
    for i in range(len(syms) - k + 1):
        if syms[i:i + k] == expected and (i == 0 or syms[i - 1][0] not in group) and \
                (i + k == len(syms) or syms[i + k][0] not in group):
            return True
    return False


def run_lengths(seq):
    out = []
    for v in seq:
        if out and out[-1][0] == v:
            out[-1][1] += 1
        else:
            out.append([v, 1])
    return [tuple(x) for x in out]


# ---- hazard cases: the limiter families ------------------------------------------------------------------------------
LIMIT_QUOTA = {15: {"needed": 8, "p1-tie": 4, "p1-deep": 4, "p2": 4, "p2-tie": 3, "tie-across-groups": 1, "tie-with-eob": 1},
               7: {"needed": 8, "p1-tie": 2, "p1-deep": 3, "p2": 3, "p2-tie": 2}}


def geometric_histogram(seed):
    """Counts ``base ** e`` with random exponents at random byte values, scaled down to a block with no used count
    below 1: many equal small counts under a ladder of large ones."""
    rng = np.random.default_rng(seed)
    base = (1.3, 1.5, 1.7, 2.0)[seed % 4]
    k = int(rng.integers(8, 257))
    top = np.log(B) / np.log(base)
    e = rng.integers(0, int(top * rng.uniform(0.6, 1.5)) + 2, k)
    c = base ** e.astype(np.float64)
    c = np.maximum(1, np.floor(c * min(1.0, B / c.sum()))).astype(np.int64)
    while c.sum() > B:
        c[int(np.argmax(c))] -= min(int(c.sum() - B), int(c.max()) - 1)
    cnt = np.zeros(256, np.int64)
    cnt[rng.choice(256, k, replace=False)] = c
    return cnt.tolist() + [1]


def laddered_histogram(seed):
    """A ladder of small counts (c_k = c_{k-1} + c_{k-2} or one more) under groups of equal counts that each about
    double the weight below them: a deep literal code whose lengths' own histogram is skewed."""
    rng = np.random.default_rng(seed)
    c = [1, 2]
    for _ in range(int(rng.integers(8, 15)) - 2):
        c.append(c[-1] + c[-2] + int(rng.integers(0, 2)))
    left = 256 - len(c)
    while left > 0:
        n = min(left, int(2 ** rng.integers(0, 8)))
        per = max(1, int(sum(c) * rng.uniform(0.5, 1.5) / n))
        if sum(c) + n * per > B:
            break
        c += [per] * n
        left -= n
    cnt = np.zeros(256, np.int64)
    cnt[rng.permutation(256)[:len(c)]] = c
    return cnt.tolist() + [1]


def limiter_labels(cnt):
    """``{15: labels, 7: labels}`` of a literal histogram: what either limiter meets for it, from the traces."""
    out = {}
    ll = deflate_lengths_signal(cnt, 15)
    clcnt = [0] * 19
    for s, _, _ in _length_symbols(ll):
        clcnt[s] += 1
    for L, h in ((15, cnt), (7, clcnt)):
        t = trace_limiter(h, L)
        lab = set()
        if t.needed:
            lab.add("needed")
            lab |= {"p1-tie"} if t.p1_ties else set()
            lab |= {"p1-deep"} if t.p1_deep else set()
            lab |= {"p2"} if t.p2_steps else set()
            lab |= {"p2-tie"} if t.p2_ties else set()
            if L == 15:
                # two of the tied symbols lie in different groups of 64: not only in different lanes of the wave but in
                # different registers of them
                lab |= {"tie-across-groups"} if any(max(x) - min(x) >= 64 for x in t.ties) else set()
                lab |= {"tie-with-eob"} if any(256 in x and any(s < 256 and h[s] == 1 for s in x) for x in t.ties) else set()
            assert kraft_is_one(deflate_lengths_signal(h, L), L)
        out[L] = lab
    out["depth"] = max(deflate_lengths_signal(cnt, 64))
    return out


def limiter_cases():
    """Seeded search: the histograms that still add to a quota of LIMIT_QUOTA, until every quota is met."""
    have = {L: {k: 0 for k in q} for L, q in LIMIT_QUOTA.items()}
    cases, labels = [], {}

    def take(name, cnt, lab):
        p = payload_of(cnt[:256], 90 + len(cases))
        assert counts_of(p) == cnt and len(p) <= B
        cases.append(Case(name, p))
        labels[name] = {f"L{L}:{k}" for L in (15, 7) for k in lab[L]}
        for L in (15, 7):
            for k in lab[L]:
                have[L][k] += 1

    def open_quota(lab):
        return any(have[L][k] < LIMIT_QUOTA[L][k] for L in (15, 7) for k in lab[L])

    for seed in range(2000):                                # both limiters in one block, which uses the Build LDS again
        cnt = laddered_histogram(seed)
        lab = limiter_labels(cnt)
        if lab["depth"] >= 18 and "needed" in lab[7]:
            take(f"limit-both-{seed}", cnt, lab)
            labels[cases[-1].name].add("both-limiters")
            break
    else:
        raise AssertionError("no histogram found that is 18 deep and needs the limit of 7 too")
    for seed in range(4000):
        if not any(have[L][k] < n for L, q in LIMIT_QUOTA.items() for k, n in q.items()):
            break
        cnt = geometric_histogram(seed)
        lab = limiter_labels(cnt)
        if open_quota(lab):
            take(f"limit-{seed}", cnt, lab)
    for L, q in LIMIT_QUOTA.items():
        for k, n in q.items():
            assert have[L][k] >= n, (L, k, have[L][k], n)
    return cases, labels


# ---- hazard cases: the merge's ties ----------------------------------------------------------------------------------
def merge_tie_cases():
    """A leaf and an internal node of equal weight at the queues' fronts: for one pick (leaves 1, 1, 1, 2: the pair
    of ones weighs 2 when the third one is taken and the leaf 2 comes up beside it; the other choice gives other
    depths), and for both picks of one step (leaves 1, 1, 1, 1, 2, 2, 4: two pairs of ones wait when the two twos
    are taken)."""
    out = []
    for name, small, both in (("merge-tie", {10: 1, 11: 1, 20: 2}, False),
                              ("merge-tie-both", {10: 1, 11: 1, 12: 1, 20: 2, 30: 2, 40: 4}, True)):
        cnt = [0] * 256
        for s, c in small.items():
            cnt[s] = c
        cnt[50], cnt[60], cnt[200] = 700, 1900, 5000
        p = payload_of(cnt, 85)
        steps = trace_merge(counts_of(p))
        assert any(a or b for a, b in steps) and any(a and b for a, b in steps) == both, (name, steps)
        out.append(Case(name, p))
    return out


# ---- hazard cases: runs of lengths, HCLEN ----------------------------------------------------------------------------
ZERO_RUNS = {3: [(17, 0, 3)], 10: [(17, 7, 3)], 11: [(18, 0, 7)], 138: [(18, 127, 7)], 139: [(18, 127, 7), (0, 0, 0)],
             148: [(18, 127, 7), (17, 7, 3)], 149: [(18, 127, 7), (18, 0, 7)]}


def zero_run_case(runs):
    """Unused byte values in runs of exactly the given lengths between used ones."""
    cnt, at = [0] * 256, 0
    for k in range(256):
        cnt[at] = 40 + 37 * (k % 11) ** 2 + (9000 if k % 29 == 0 else 0)
        at += 1 + (runs[k] if k < len(runs) else 0)
        if at >= 256:
            break
    scale = min(1.0, 0.9 * B / sum(cnt))
    cnt = [max(1, int(c * scale)) if c else 0 for c in cnt]
    p = payload_of(cnt, 86)
    pl = plan_of(p)
    rl = run_lengths(pl.ll + [1, 1])
    for r in runs:
        assert (0, r) in rl and has_run(pl.syms, ZERO_RUNS[r], (0, 17, 18)), (r, rl)
    return Case("zero-runs-" + "-".join(map(str, runs)), p)


def nonzero_run_case():
    """Equal non-zero lengths in runs of exactly 4, 7, 10 and 11, each between unused values, by a seeded search over
    the groups' counts: v 16(3); v 16(6); v 16(6) 16(3); v 16(6) 16(4).  (The rule's ``t = min(r, 6)`` is greedy: a
    literal length behind two 16s needs a rest of 1 or 2, as the run of 9 of equal_lengths() has behind one.)"""
    rng = np.random.default_rng(87)
    want = {4: [(16, 0, 2)], 7: [(16, 3, 2)], 10: [(16, 3, 2), (16, 0, 2)], 11: [(16, 3, 2), (16, 1, 2)]}
    for _ in range(3000):
        cnt, at = [0] * 256, 2
        cnt[0] = int(rng.integers(1, 30000))
        for r in (4, 7, 10, 11):
            cnt[at:at + r] = [int(2 ** rng.integers(3, 10))] * r
            at += r + 1
        p = payload_of(cnt, 88)
        ll = deflate_lengths_signal(counts_of(p), 15)
        rl = run_lengths(ll + [1, 1])
        if all(any(v and n == r for v, n in rl) for r in want):
            syms = _length_symbols(ll)
            for r, tail in want.items():
                v = next(v for v, n in rl if v and n == r)
                exp = [(v, 0, 0)] + [(v, 0, 0) if x is None else x for x in tail]
                assert has_run(syms, exp, (v, 16)), (r, exp)
            return Case("nonzero-runs", p)
    raise AssertionError("no counts found with equal lengths in runs of 4, 7, 10 and 11")


def ones_into_distances():
    """Only the value 255: ll[255] = ll[256] = 1 run on into the two appended distance lengths, a run of four ones
    coded 1 16(3).  (Three literal symbols cannot all have length 1, so ll[254] is 0: four is the longest such run.)"""
    p = bytes([255]) * 3001
    pl = plan_of(p)
    assert pl.ll[254:] == [0, 1, 1] and pl.syms[-2:] == [(1, 0, 0), (16, 0, 2)] and not is_stored(p)
    assert pl.syms[:-2] == [(18, 127, 7), (18, 117 - 11, 7)]
    return Case("ones-into-distances", p)


def hclen_cases(limiters):
    """HCLEN 19 where the literal code has a length of 15 (symbol 15 is the last of the order), and the smallest
    value the search over every other hazard case and a few plain payloads finds: 18.  That is the floor: the two
    distance lengths are ones, a run of ones begins with the literal symbol 1, and symbol 1 is the order's 18th."""
    deep = next(c for c in limiters if 15 in plan_of(c.data).ll)
    assert plan_of(deep.data).hclen == 19 and plan_of(deep.data).cl[15] > 0
    pool = [bytes(200), bytes(range(4)) * 500, b"ACGT\n" * 3000 + b"N", fastq_text()[:5000]] + [c.data for c in limiters]
    low = min(pool, key=lambda p: plan_of(p).hclen)
    assert plan_of(low).hclen == 18 == min(plan_of(p).hclen for p in pool) and not is_stored(low)
    return [Case("hclen-19", deep.data), Case("hclen-18", low)]


# ---- hazard cases: the pack kernel -----------------------------------------------------------------------------------
def _ladder_counts():
    """127 values once and the end of block: a subtree 7 deep under a ladder of eight leaves that each weigh what lies
    below them: lengths 1 to 8, and 15 for the 128 rare symbols, without the limiter."""
    cnt = [0] * 256
    cnt[1:128] = [1] * 127
    for k in range(8):
        cnt[130 + 10 * k] = 128 << k
    ll = deflate_lengths_signal(cnt + [1], 15)
    assert ll[1:128] == [15] * 127 and ll[256] == 15 and [ll[130 + 10 * k] for k in range(8)] == list(range(8, 0, -1))
    assert max(deflate_lengths_signal(cnt + [1], 64)) == 15
    return cnt, ll


def pack_extreme_runs():
    """Unshuffled: the pack kernel's thread 0 packs 64 codes of 15 bits (960 bits, 30 flushes of its accumulator),
    thread 1 packs 64 codes of 1 bit (two flushes at the most)."""
    cnt, ll = _ladder_counts()
    p = np.repeat(np.arange(256), cnt).astype(np.uint8)
    rare, most = p[p < 128], p[p == 200]
    rest = p[(p >= 128) & (p != 200)]
    p = np.concatenate([rare[:64], most[:64], rare[64:], rest, most[64:]]).tobytes()
    assert counts_of(p) == cnt + [1]
    bits = np.asarray(plan_of(p).ll)[np.frombuffer(p, np.uint8)]
    per_run = bits[:len(p) // 64 * 64].reshape(-1, 64)
    assert (per_run[0] == 15).all() and (per_run[1] == 1).all() and (per_run == 1).all(1).sum() > 100
    return Case("pack-15-bits-and-1-bit", p)


def pack_eob_across_words():
    """The end-of-block code has 15 bits and lies across a 32-bit word of the pack kernel's output image: the image
    starts at the 16-byte address in front of the deflate bytes, 18 bytes behind ``out``."""
    cnt, ll = _ladder_counts()
    p = payload_of(cnt, 89)
    pl = plan_of(p)
    assert pl.ll[256] == 15
    for out_offset in range(16):
        e = 8 * ((out_offset + 18) % 16) + pl.hdr_bits + pl.lit_bits
        if e % 32 + 15 > 32:
            return Case(f"pack-eob-across-words-out{out_offset}", p, out_offset=out_offset)
    raise AssertionError("no out_offset puts the end of block across two words")


PACK_LENGTHS = (63, 64, 65, 127, 128, 129, 65215, 65216, 65217, 65279)


def pack_lengths():
    """Lengths around the pack kernel's last whole run of 64 bytes, with three values, so each block is dynamic."""
    rng = np.random.default_rng(91)
    out = []
    for n in PACK_LENGTHS:
        p = np.array([7, 100, 255], np.uint8)[rng.choice(3, n, p=(0.6, 0.3, 0.1))].tobytes()
        assert len(set(p)) == 3 and not is_stored(p)
        out.append(Case(f"pack-n-{n}", p))
    return out


def pack_alignments():
    """One compressible payload at every alignment of the output, and at every alignment of the source."""
    p = fastq_text()[:40003]
    assert not is_stored(p) and len(_deflate_dynamic(p)) < 0.7 * len(p)
    return [Case(f"pack-out-{o}", p, out_offset=o) for o in range(16)] + \
           [Case(f"pack-src-{s}-out-7", p, src_offset=s, out_offset=7) for s in range(1, 16)]


@functools.lru_cache(maxsize=None)
def _hazards():
    t0 = time.perf_counter()
    limiters, labels = limiter_cases()
    cases = limiters + merge_tie_cases()
    cases += [zero_run_case([3, 10, 11, 138]), zero_run_case([139]), zero_run_case([148]), zero_run_case([149]),
              nonzero_run_case(), ones_into_distances()] + hclen_cases(limiters)
    cases += [pack_extreme_runs(), pack_eob_across_words()] + pack_lengths() + pack_alignments()
    names = [c.name for c in cases]
    assert len(set(names)) == len(names), names
    for p in {c.data for c in cases}:                       # every case: one dynamic block, both codes complete
        pl = plan_of(p)
        assert 0 < len(p) <= B and not is_stored(p)
        assert kraft_is_one(pl.ll, 15) and kraft_is_one(pl.cl, 7), "the Kraft sum is exactly 1"
    assert all(c.nbytes is None and c.byte_capacity is None for c in cases)
    return cases, labels, time.perf_counter() - t0


def hazard_cases():
    """The single-block cases built for the code construction's and the pack kernel's hazards, built once a process."""
    return _hazards()[0]


def hazard_labels():
    """Per limiter case, the conditions of LIMIT_QUOTA that its traces show, as ``L15:p1-tie`` and so on."""
    return _hazards()[1]


def hazard_build_seconds():
    return _hazards()[2]
