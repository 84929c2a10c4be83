"""BGZF deflate (pgn_bgzf_deflate_device): the C ABI surface, the refusals, the rule's text and the host model,
without a GPU.

The model is held to zlib: every block's body inflates to its payload with nothing left over, the file to the
stream, and the CRC field to ``zlib.crc32``; the code lengths to the Kraft sum and to the unrestricted construction
where that fits; the size to zlib's own Huffman-only output.  The cases of the GPU tests are built here too, so the
conditions their builders assert are checked on the CPU.
"""
import ctypes as C
import gzip
import io
import os
import re
import zlib

import numpy as np
import pytest

import _bam_cases
import _bgzf_cases as K
from rawnanoporesignalcompression_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FN = "pgn_bgzf_deflate_device"


def _header(comments=False):
    src = open(os.path.join(ROOT, "include", "pgnano_hip.h")).read()
    return src if comments else re.sub(r"/\*.*?\*/", "", src, flags=re.S)


@pytest.fixture(scope="module")
def cases():
    return K.deflate_cases()


@pytest.fixture(scope="module")
def hazards():
    return K.hazard_cases()


# ---- surface -------------------------------------------------------------------------------------------------
def test_symbol_declared_exported_and_bound():
    import rawnanoporesignalcompression_amd as pkg
    from rawnanoporesignalcompression_amd import _native, bam, bgzf, host

    lib = _native.load()
    sigs = {s[0]: s for s in _native.SIGNATURES}
    assert re.search(r"\bint\s+" + FN + r"\s*\(", _header())
    assert hasattr(lib, FN)
    assert sigs[FN][1] is C.c_int and len(sigs[FN][2]) == 10
    for name in ("bgzf_deflate", "write_gz", "BgzfBlocks", "deflate_lengths_signal", "deflate_block_signal",
                 "bgzf_deflate_signal", "bgzf_bound", "BGZF_EOF"):
        assert name in bgzf.__all__ and hasattr(bgzf, name)
        assert name not in pkg.__all__                      # the package's own surface stays as it is
    for name in ("deflate_lengths_signal", "deflate_block_signal", "bgzf_deflate_signal", "bgzf_bound", "BGZF_EOF"):
        assert getattr(bgzf, name) is getattr(host, name)
    assert not hasattr(pkg.PGNanoCodec, "bgzf_deflate")
    assert bgzf.BGZF_EOF is bam.BGZF_EOF
    src = open(os.path.join(ROOT, "rawnanoporesignalcompression_amd", "csrc", "pgn_kernels.hip")).read()
    assert '#include "pgn_deflate.h"' in src


def test_call_refusals_and_their_order():
    from rawnanoporesignalcompression_amd import _native

    fn = getattr(_native.load(), FN)
    bad = _native.PGN_ERR_INVALID_ARG
    dummy = C.c_void_p(0x1000)

    def call(ctx=dummy, flags=0, src=dummy, scap=100, nbytes=None, out=dummy, cap=200, off=dummy, wr=dummy):
        return fn(ctx, flags, src, scap, nbytes, out, cap, off, wr, None)

    assert call(ctx=None) == bad
    for flags in (1, 4, 1 << 31):
        assert call(flags=flags) == bad, flags
    assert call(src=None) == bad
    assert call(off=None) == bad
    assert call(wr=None) == bad
    assert call(off=None, scap=0, src=None) == bad          # ... with nothing to read, too
    assert call(wr=None, scap=0, src=None) == bad
    assert call(out=None) == bad
    for scap in (1 << 48, 1 << 63):
        assert call(scap=scap) == bad, scap
    assert call(ctx=None, flags=1, src=None, off=None, out=None, scap=1 << 48) == bad


def test_the_header_carries_the_rule():
    src = re.sub(r"\s*\n \*\s*", " ", _header(comments=True))
    for text in ("---- BGZF deflate", "W = min(*d_nbytes, src_capacity)", "BSIZE as u16 = the block's total length minus 1",
                 "the dynamic block below if its byte length is < n + 5, else the stored block 01 n ~n p",
                 "A tie stores.", "cnt[256] = 1, the end-of-block symbol", "ll = lengths(cnt, 15) over the 257 symbols",
                 "BFINAL = 1 in 1 bit; BTYPE = 2 in 2 bits; HLIT = 0 in 5 bits (257 codes); HDIST = 1 in 5 bits",
                 "The length sequence has 259 entries: ll[0..256], 1, 1.",
                 "symbol 18 with t = min(r, 138), extra value t - 11 in 7 bits", "symbol 17 with r - 3 in 3 bits",
                 "symbol 16 with t = min(r, 6), extra value t - 3 in 2 bits",
                 "cl = lengths(histogram of those symbols, 7) over the 19 code-length symbols",
                 "16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15", "sorted by (cnt, symbol) ascending, are the leaf queue",
                 "the leaf where its weight is <= the internal node's", "One used symbol alone gets length 1.",
                 "take the longest length, then the smallest count, then the largest symbol",
                 "take the largest count, then the smallest symbol",
                 "Block k is written iff blk_off[k + 1] <= byte_capacity", "d_written[0] = min(W, 65280 * kw)",
                 "There are no partial blocks.", "entries above nblocks repeat the total",
                 "the scratch is 1,568 bytes per block",
                 "Not covered: a match search, so the output is Huffman only; several deflate blocks per BGZF block; "
                 "fixed-Huffman blocks; a .gzi or .bai index from blk_off; fusing into the record writers; decompression.",
                 # the sections whose gap this closes keep their sentences and point here
                 "Not covered: deflate compression (every block holds a stored deflate block, as `samtools view -u` writes);",
                 "framing of other buffers.  Both are pgn_bgzf_deflate_device's (\"BGZF deflate\" below)",
                 "compression of the text;", "The text leaves compressed through pgn_bgzf_deflate_device (\"BGZF deflate\" below)."):
        assert text in src, text
    assert src.index("---- BAM records") < src.index("---- BGZF deflate")
    for path in ("README.md", "DESIGN.md", os.path.join("tools", "README.md")):
        text = re.sub(r"\s+", " ", open(os.path.join(ROOT, path)).read())
        assert "BGZF deflate" in text and "bgzf_deflate" in text, path


# ---- the model against zlib ----------------------------------------------------------------------------------------
def _inflates_and_is_laid_out(cases):
    for c in cases:
        data, off, written = c.expected()
        stream = c.data[:c.W]
        assert off.dtype == np.uint64 and written.dtype == np.uint64 and len(off) == c.ntiles + 1
        consumed = int(written[0])
        assert (gzip.decompress(data) if data else b"") == stream[:consumed], c.name
        blocks = _bam_cases.parse_bgzf(data)
        assert consumed == min(c.W, K.B * len(blocks)) and (consumed == c.W or consumed % K.B == 0)
        for k, (at, size, body, crc, isize) in enumerate(blocks):
            p = stream[k * K.B:(k + 1) * K.B]
            assert at == int(off[k]) and at + size == int(off[k + 1]) <= c.capacity, (c.name, k)
            z = zlib.decompressobj(-15)
            assert z.decompress(body) == p and z.eof and not z.unused_data and not z.unconsumed_tail, (c.name, k)
            assert crc == zlib.crc32(p) and isize == len(p), (c.name, k)
            assert len(body) <= len(p) + 5 and (body[0] & 7) in (1, 5)    # final, and stored or dynamic
            assert (body[0] & 7 == 1) == (len(body) == len(p) + 5), "a block is stored iff it is as long as the stored form"
        nblocks = -(-c.W // K.B)
        assert (off[nblocks:] == off[nblocks]).all() and (np.diff(off.astype(np.int64))[:nblocks] > 26).all()
        # the written blocks are the longest prefix that the capacity holds
        assert len(blocks) == nblocks or int(off[len(blocks) + 1]) > c.capacity, c.name
        from rawnanoporesignalcompression_amd.host import bgzf_bound
        assert int(off[-1]) <= bgzf_bound(c.W)


def test_every_case_inflates_and_is_laid_out(cases):
    _inflates_and_is_laid_out(cases)


def test_every_hazard_case_inflates_and_is_laid_out(hazards):
    _inflates_and_is_laid_out(hazards)
    assert all(len(_bam_cases.parse_bgzf(c.expected()[0])) == 1 for c in hazards), "single blocks"


def test_python_model_refusals():
    from rawnanoporesignalcompression_amd.host import deflate_block_signal

    for p in (b"", bytes(K.B + 1)):
        with pytest.raises(ValueError):
            deflate_block_signal(p)


def _unrestricted(cnt):
    """Code lengths by a textbook Huffman construction with the rule's tie order, written apart from the model."""
    import heapq

    heap = [(c, 0, s, (s,)) for s, c in enumerate(cnt) if c]      # leaves before internal nodes, then by age
    depth = {s: 0 for _, _, s, _ in heap}
    if len(heap) == 1:
        return {heap[0][2]: 1}
    heapq.heapify(heap)
    age = 0
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for s in a[3] + b[3]:
            depth[s] += 1
        age += 1
        heapq.heappush(heap, (a[0] + b[0], 1, age, a[3] + b[3]))
    return depth


def test_lengths_on_direct_histograms():
    from rawnanoporesignalcompression_amd.host import deflate_lengths_signal

    rng = np.random.default_rng(81)
    fib = [1, 2]
    while len(fib) < 30:
        fib.append(fib[-1] + fib[-2] + 1)
    hists = [[5], [0, 0, 7], [1, 1], [3, 0, 3, 3], [1] * 257, [1] * 19, fib[:20] + [1], fib[:12], list(range(1, 258)),
             [1, 1, 2, 4, 8, 16, 32, 64, 128, 256, 512], [0] * 10]
    for _ in range(300):
        k = int(rng.integers(1, 258))
        h = (rng.pareto(0.5, k) * 3).astype(np.int64) % 60000
        hists.append(h.tolist())
    deep = {15: 0, 7: 0}
    for h in hists:
        for limit, width in ((15, 257), (7, 19)):
            cnt = h[:width]
            got = deflate_lengths_signal(cnt, limit)
            used = [v for v in got if v]
            assert len(got) == len(cnt) and [v > 0 for v in got] == [c > 0 for c in cnt]
            assert max(got, default=0) <= limit
            if len(used) >= 2:
                assert sum(1 << (limit - v) for v in used) == 1 << limit, "the Kraft sum is exactly 1"
            elif used:
                assert used == [1]
            free = _unrestricted(cnt)
            if max(free.values(), default=0) <= limit:
                assert {s: v for s, v in enumerate(got) if v} == free
            else:
                deep[limit] += 1
                # the limiter only moves bits: never below the unrestricted cost
                assert sum(c * v for c, v in zip(cnt, got)) >= sum(cnt[s] * v for s, v in free.items())
    assert deep[15] >= 1 and deep[7] >= 10, deep


def test_size_against_zlib_huffman_only(cases):
    """A guard on the length rule: within 2 % of zlib's own Huffman-only streams, block by block (the margin is for
    other zlib versions' block cuts).  With zlib 1.2.11 the ratios are 1.0191 on the long read, whose fields zlib meets
    with a new deflate block every 32,768 literals, and 1.0003 on the deep histogram."""
    by_name = {c.name: c for c in cases}
    for name in ("bam", "deep-histogram"):
        c = by_name[name]
        data, off, _ = c.expected()
        ours = sum(size - 26 for _, size, _, _, _ in _bam_cases.parse_bgzf(data))
        theirs = 0
        for at in range(0, len(c.data), K.B):
            z = zlib.compressobj(9, zlib.DEFLATED, -15, 9, zlib.Z_HUFFMAN_ONLY)
            theirs += len(z.compress(c.data[at:at + K.B]) + z.flush())
        print(f"{name}: {ours} deflate bytes, zlib Z_HUFFMAN_ONLY {theirs}, ratio {ours / theirs:.4f}")
        assert ours <= 1.02 * theirs, (name, ours, theirs)


def test_hazard_sizes_against_zlib_huffman_only(hazards):
    """The same guard on every hazard payload: zlib limits its lengths by another rule and may code a small payload
    with the fixed code, so a rule that loses bits to either limiter or to its runs would show here."""
    worst = 0.0
    for p in sorted({c.data for c in hazards}, key=len):
        ours = len(K.deflate_block_signal(p))
        z = zlib.compressobj(9, zlib.DEFLATED, -15, 9, zlib.Z_HUFFMAN_ONLY)
        theirs = len(z.compress(p) + z.flush())
        worst = max(worst, ours / theirs)
        assert ours <= 1.02 * theirs, (len(p), ours, theirs)
    print(f"hazard payloads: the worst ratio to zlib Z_HUFFMAN_ONLY is {worst:.4f}")


# ---- the hazard list: what it meets, and that it can fail ------------------------------------------------------------
def test_the_hazard_list_meets_every_condition(hazards):
    """The table of the conditions the limiter families exist for, counted from the traces, and the build time."""
    labels = K.hazard_labels()
    rows = [(f"L{L}:{k}", n) for L, q in K.LIMIT_QUOTA.items() for k, n in q.items()] + [("both-limiters", 1)]
    print(f"hazard_cases(): {len(hazards)} cases built in {K.hazard_build_seconds():.2f} s")
    for label, need in rows:
        have = sorted(name for name, v in labels.items() if label in v)
        print(f"  {label:24s} needs {need}, has {len(have):2d}: {' '.join(have)}")
        assert len(have) >= need, label
    by_name = {c.name: c for c in hazards}
    both = by_name[next(n for n, v in labels.items() if "both-limiters" in v)]
    t = K.trace_limiter(K.counts_of(both.data), 15)
    assert t.depth >= 18 and K.trace_limiter(K.plan_of(both.data).clcnt, 7).needed
    # a tie across groups: two tied symbols at least 64 apart; a tie with the end of block: 256 among byte values of count 1
    assert any(max(x) - min(x) >= 64 for c in hazards if c.name.startswith("limit-")
               for x in K.trace_limiter(K.counts_of(c.data), 15).ties)
    eob = by_name[next(n for n, v in labels.items() if "L15:tie-with-eob" in v)]
    cnt = K.counts_of(eob.data)
    assert any(256 in x and len(x) > 1 and all(cnt[s] == 1 for s in x) for x in K.trace_limiter(cnt, 15).ties)
    # the lists of the other families
    names = [c.name for c in hazards]
    for prefix, count in (("merge-tie", 2), ("zero-runs-", 4), ("nonzero-runs", 1), ("ones-into-distances", 1), ("hclen-", 2),
                          ("pack-15-bits-and-1-bit", 1), ("pack-eob-across-words", 1), ("pack-n-", len(K.PACK_LENGTHS)),
                          ("pack-out-", 16), ("pack-src-", 15)):
        assert len([n for n in names if n.startswith(prefix)]) == count, prefix
    assert sorted(len(c.data) for c in hazards if c.name.startswith("pack-n-")) == sorted(K.PACK_LENGTHS)
    assert {c.out_offset for c in hazards if c.name.startswith("pack-out-")} == set(range(16))
    assert {(c.src_offset, c.out_offset) for c in hazards if c.name.startswith("pack-src-")} == {(s, 7) for s in range(1, 16)}
    assert {r for c in hazards if c.name.startswith("zero-runs-") for r in map(int, c.name.split("-")[2:])} == set(K.ZERO_RUNS)
    assert K.hazard_build_seconds() < 10, "the seeded searches stay short"


MUTANTS = ("p1-tie-largest-count", "p1-tie-smallest-symbol", "p2-tie-largest-symbol", "p2-smallest-count", "p2-skipped",
           "merge-prefers-internal", "rank-ties-reversed", "cap-18-at-137", "cap-16-at-5", "17-from-4", "hclen-untrimmed")
TIE_MUTANTS = MUTANTS[:3]


def _mutant_lengths(cnt, L, m):
    """deflate_lengths_signal again, with the one thing changed that ``m`` names (None: nothing)."""
    cnt = [int(c) for c in cnt]
    out = [0] * len(cnt)
    leaves = sorted(((c, s) for s, c in enumerate(cnt) if c > 0), key=lambda x: (x[0], -x[1] if m == "rank-ties-reversed" else x[1]))
    n = len(leaves)
    if n == 0:
        return out
    if n == 1:
        out[leaves[0][1]] = 1
        return out
    w = [c for c, _ in leaves] + [0] * (n - 1)
    parent = [0] * (2 * n - 1)
    li, ii = 0, n
    for nxt in range(n, 2 * n - 1):
        pair = []
        for _ in range(2):
            if li < n and (ii >= nxt or (w[li] < w[ii] if m == "merge-prefers-internal" else w[li] <= w[ii])):
                pair.append(li)
                li += 1
            else:
                pair.append(ii)
                ii += 1
        w[nxt] = w[pair[0]] + w[pair[1]]
        parent[pair[0]] = parent[pair[1]] = nxt
    depth = [0] * (2 * n - 1)
    for i in range(2 * n - 3, -1, -1):
        depth[i] = depth[parent[i]] + 1
    for i, (_, s) in enumerate(leaves):
        out[s] = depth[i]
    if max(out) <= L:
        return out
    used = [s for _, s in leaves]
    for s in used:
        out[s] = min(out[s], L)
    k1 = {"p1-tie-largest-count": lambda s: (out[s], cnt[s], s), "p1-tie-smallest-symbol": lambda s: (out[s], -cnt[s], -s)}
    k2 = {"p2-tie-largest-symbol": lambda s: (cnt[s], s), "p2-smallest-count": lambda s: (-cnt[s], -s)}
    Kr = sum(1 << (L - out[s]) for s in used)
    while Kr > 1 << L:
        s = max((s for s in used if out[s] < L), key=k1.get(m, lambda s: (out[s], -cnt[s], s)))
        Kr -= 1 << (L - out[s] - 1)
        out[s] += 1
    D = 0 if m == "p2-skipped" else (1 << L) - Kr
    while D > 0:
        s = max((s for s in used if out[s] > 1 and 1 << (L - out[s]) <= D), key=k2.get(m, lambda s: (cnt[s], -s)))
        D -= 1 << (L - out[s])
        out[s] -= 1
    return out


def _mutant_symbols(ll, m):
    """_length_symbols again, with the run rule that ``m`` names changed."""
    cap18, cap16, min17 = (137 if m == "cap-18-at-137" else 138), (5 if m == "cap-16-at-5" else 6), (4 if m == "17-from-4" else 3)
    seq = list(ll) + [1, 1]
    syms, at = [], 0
    while at < len(seq):
        v, r = seq[at], 1
        while at + r < len(seq) and seq[at + r] == v:
            r += 1
        at += r
        if v == 0:
            while r >= 11:
                t = min(r, cap18)
                syms.append((18, t - 11, 7))
                r -= t
            if r >= min17:
                syms.append((17, r - 3, 3))
            else:
                syms += [(0, 0, 0)] * r
        else:
            syms.append((v, 0, 0))
            r -= 1
            while r >= 3:
                t = min(r, cap16)
                syms.append((16, t - 3, 2))
                r -= t
            syms += [(v, 0, 0)] * r
    return syms


def _mutant_plan(p, m):
    ll = _mutant_lengths(K.counts_of(p), 15, m)
    syms = _mutant_symbols(ll, m)
    clcnt = [0] * 19
    for s, _, _ in syms:
        clcnt[s] += 1
    cl = _mutant_lengths(clcnt, 7, m)
    hclen = 19 if m == "hclen-untrimmed" else max(4, max(i + 1 for i, s in enumerate(host._CL_ORDER) if cl[s]))
    return ll, syms, cl, hclen


def _mutant_block(plan, p):
    """The dynamic block of a plan: the bits of _deflate_dynamic, written apart from it."""
    ll, syms, cl, hclen = plan
    fields = [(1, 1), (2, 2), (0, 5), (1, 5), (hclen - 4, 4)] + [(cl[s], 3) for s in host._CL_ORDER[:hclen]]
    clcode = host._canonical_codes(cl)

    def msb_first(code, bits):
        return int(format(code, f"0{bits}b")[::-1], 2) if bits else 0

    for s, extra, ebits in syms:
        fields += [(msb_first(clcode[s], cl[s]), cl[s]), (extra, ebits)]
    code = host._canonical_codes(ll)
    rev = np.array([msb_first(code[s], ll[s]) for s in range(257)], np.int64)
    lens = np.asarray(ll, np.int64)
    lit = np.concatenate([np.frombuffer(p, np.uint8).astype(np.int64), [256]])
    head = [(v >> i) & 1 for v, n in fields for i in range(n)]
    at = len(head) + np.concatenate([[0], np.cumsum(lens[lit])])
    bits = np.zeros(int(at[-1]), np.uint8)
    bits[:len(head)] = head
    for k in range(15):
        has = lens[lit] > k
        bits[at[:-1][has] + k] = (rev[lit][has] >> k) & 1
    return np.packbits(bits, bitorder="little").tobytes()


def _blocks_of(cases):
    """The distinct payloads of the cases' blocks."""
    return {c.name + (f"[{k // K.B}]" if c.W > K.B else ""): c.data[k:min(k + K.B, c.W)]
            for c in cases for k in range(0, c.W, K.B)}


def test_mutants_of_the_rule_fail_on_the_hazard_cases(cases, hazards):
    """Eleven copies of the rule with one thing changed each: every one writes, for at least one hazard case, a block
    that differs from the model's and still is a deflate block of the payload.  zlib inflates ten of them; it
    refuses a literal code that is not complete, so the block without the give-back loop is held to its lengths: no
    longer than 15, the Kraft sum at most 1.  The cases of deflate_cases() meet no tie at the limit of 15 and one at
    the limit of 7 (limited-header, in phase 1, between equal counts that only the symbol order separates): of the
    three tie mutants they tell that one from the rule, there, and no other."""
    seen = {}
    payloads = {}
    for c in hazards:
        payloads.setdefault(c.data, c.name)
    for p, name in payloads.items():
        same = _mutant_plan(p, None)
        assert same == (lambda pl: (pl.ll, pl.syms, pl.cl, pl.hclen))(K.plan_of(p)), name
        model = host._deflate_dynamic(p)
        assert _mutant_block(same, p) == model, name
        for m in MUTANTS:
            plan = _mutant_plan(p, m)
            if plan == same:
                continue
            block = _mutant_block(plan, p)
            assert block != model, (m, name)
            if m == "p2-skipped":
                assert max(plan[0]) <= 15 and sum(1 << (15 - v) for v in plan[0] if v) <= 1 << 15
                assert sum(1 << (7 - v) for v in plan[2] if v) <= 1 << 7
            else:
                z = zlib.decompressobj(-15)
                assert z.decompress(block) == p and z.eof and not z.unused_data, (m, name)
            seen.setdefault(m, []).append(name)
    for m in MUTANTS:
        print(f"  {m:24s} fails on {len(seen.get(m, ())):2d}: {' '.join(seen.get(m, ()))}")
        assert seen.get(m), f"no hazard case tells the mutant {m} from the rule"
    old = _blocks_of(cases)
    for m in TIE_MUTANTS:
        told = [name for name, p in old.items() if p and _mutant_plan(p, m) != _mutant_plan(p, None)]
        print(f"  deflate_cases() alone: {m} fails on {told}")
        # at the limit of 15 nothing; at 7, limited-header meets one phase-1 tie, which only the symbol order decides
        assert not [name for name, p in old.items() if p and _mutant_lengths(K.counts_of(p), 15, m) != K.plan_of(p).ll], m
        assert told == (["limited-header"] if m == "p1-tie-smallest-symbol" else []), (m, told)


def test_write_gz_and_write_bam(tmp_path, cases):
    from rawnanoporesignalcompression_amd import bam, bgzf

    by_name = {c.name: c for c in cases}
    text, stream = by_name["fastq"], by_name["bam"]
    path = tmp_path / "reads.fastq.gz"
    n = bgzf.write_gz(str(path), [text.expected()[0], by_name["w-0"].expected()[0], by_name["tiny-2"].expected()[0]])
    raw = path.read_bytes()
    assert n == len(raw) and raw.endswith(bgzf.BGZF_EOF)
    assert gzip.decompress(raw) == text.data + by_name["tiny-2"].data
    buf = io.BytesIO()
    assert bgzf.write_gz(buf, []) == 28 and buf.getvalue() == bgzf.BGZF_EOF
    buf = io.BytesIO()
    bam.write_bam(buf, [stream.expected()[0]])
    plain = gzip.decompress(buf.getvalue())
    assert plain == bam.bam_header() + stream.data
    assert len(_bam_cases.parse_records(plain[len(bam.bam_header()):])) == 5
    assert len(buf.getvalue()) < 0.45 * len(plain)


def test_the_case_list_covers_the_issue(cases):
    got = [c.name for c in cases]
    for prefix, count in (("bam", 1), ("fastq", 1), ("zeros", 1), ("tiny-", 2), ("uniform", 1), ("every-value", 1),
                          ("two-values", 1), ("equal-lengths", 1), ("deep-histogram", 1), ("limited-header", 1),
                          ("break-even", 3), ("w-", 7), ("align-", 8), ("capacity-", 7), ("nbytes-", 4)):
        assert len([n for n in got if n.startswith(prefix)]) == count, prefix
    assert sorted(len(c.data) for c in cases if c.name.startswith("w-")) == sorted(K.W_CASES)
    assert {(c.src_offset, c.out_offset) for c in cases} == {(s, o) for s in K.OFFSETS for o in K.OFFSETS}
    assert {c.nbytes is None for c in cases} == {True, False}
