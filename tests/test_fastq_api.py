"""FASTQ records (pgn_read_qual_device, pgn_fastq_records_device): the C ABI surface, the refusals and the two host
models, without a GPU.

The record model is held to a three-line formatter made of ``uuid.UUID``, f-strings and slices, the mean-quality
model to a loop over Python integers, and the error table to its closed form in ``decimal``; the cases of the GPU
tests (tests/_fastq_cases.py) are built here too, so the conditions their builders assert are checked on the CPU.
"""
import ctypes as C
import decimal
import os
import re
import uuid

import numpy as np
import pytest

import _fastq_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RQ, REC = "pgn_read_qual_device", "pgn_fastq_records_device"


def _header(comments=False):
    src = open(os.path.join(ROOT, "include", "pgnano_hip.h")).read()
    return src if comments else re.sub(r"/\*.*?\*/", "", src, flags=re.S)


# ---- surface -------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_bound():
    import rawnanoporesignalcompression_amd as pkg
    from rawnanoporesignalcompression_amd import _native, fastq, host

    lib = _native.load()
    sigs = {s[0]: s for s in _native.SIGNATURES}
    for name, nargs in ((RQ, 11), (REC, 15)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", _header())
        assert hasattr(lib, name)
        assert sigs[name][1] is C.c_int and len(sigs[name][2]) == nargs
    for name in ("read_qual", "fastq_records", "read_tags", "read_qual_signal", "fastq_records_signal", "err_table",
                 "fastq_bound"):
        assert name in fastq.__all__ and callable(getattr(fastq, name))
        assert name not in pkg.__all__                      # the package's own surface stays as it is
    for name in ("read_qual_signal", "fastq_records_signal", "err_table", "fastq_bound"):
        assert getattr(fastq, name) is getattr(host, name)
    for attr in ("read_qual", "fastq_records"):
        assert not hasattr(pkg.PGNanoCodec, attr)
    for name, value in (("PGN_READ_QUAL_TILE_BASES", 4096), ("PGN_FASTQ_TILE_BYTES", 16384), ("PGN_FASTQ_MAX_TAGS", 8),
                        ("PGN_FASTQ_REVERSE", 1)):
        assert re.search(rf"#define {name} {value}u\b", _header()) and getattr(_native, name) == value


def test_struct_layouts():
    from rawnanoporesignalcompression_amd import _native

    fields = lambda body: re.findall(r"(\w[\w ]*?)\s*\*?(\w+)((?:\[\d+\])*);", body)
    m = re.search(r"typedef struct pgn_read_qual_params \{([^}]*)\}", _header())
    assert m and fields(m.group(1)) == [("pgn_qual_params", "mean", ""), ("uint32_t", "skip_bases", ""),
                                        ("uint32_t", "min_mean_q", ""), ("uint32_t", "err", "[94]")]
    S = _native.ReadQualParams
    assert C.sizeof(S) == 4 * 95 + 8 + 4 * 94
    assert [(f, getattr(S, f).offset) for f, _ in S._fields_] == [("mean", 0), ("skip_bases", 380), ("min_mean_q", 384),
                                                                  ("err", 388)]
    m = re.search(r"typedef struct pgn_fastq_params \{([^}]*)\}", _header())
    assert m and fields(m.group(1)) == [("uint32_t", "flags", ""), ("uint32_t", "ntags", ""),
                                        ("uint8_t", "tag_name", "[8][2]"), ("const uint32_t", "d_tag", "[8]")]
    S = _native.FastqParams
    assert C.sizeof(S) == 24 + 8 * C.sizeof(C.c_void_p)
    assert [(f, getattr(S, f).offset) for f, _ in S._fields_] == [("flags", 0), ("ntags", 4), ("tag_name", 8), ("d_tag", 24)]


def test_the_header_carries_the_rules():
    src = re.sub(r"\s*\n \*\s*", " ", _header(comments=True))
    for text in ("FASTQ records", "No outside source defines the rule, so this text does.",
                 "m = read_bases[r+1] - read_bases[r] > 0.",
                 "s = skip_bases if m > skip_bases else 0, and n = m - s",
                 "U = sum over g in [s, m) of err[min(max(qual[read_bases[r] + g], 33), 126) - 33]",
                 "mean_q[r] = q_min + #{ j < nthresholds : U <= (uint64)thr[j] * n }",
                 "pass[r] = mean_q[r] >= min_mean_q",
                 "err[q] = min(2^32 - 1, rint(2^32 * 10^(-q/10)))",
                 "'@' uuid { '\\t' name0 name1 ':' 'i' ':' dec(tag_k[r]) } '\\n' SEQ '\\n' '+' '\\n' QUAL '\\n'",
                 "length of a kept read's record = 42 + 2m + sum_k (6 + digits(tag_k[r]))",
                 "fastq_bound(nreads, nbases, ntags) = nreads * (42 + 16 * ntags) + 2 * nbases",
                 "there are no partial records", "nreads == 0 writes rec_off[0] = 0 only.",
                 "Not covered: SAM/uBAM output, and the move-table tag; a float qs:f: tag; compression of the text; "
                 "pass and fail files from one call; records for the CTC path's bases without qualities; signed or "
                 "64-bit tag values; splitting of reads."):
        assert text in src, text
    assert src.index("Posteriors and qualities (CRF)") < src.index("---- FASTQ records")
    for path in ("README.md", "DESIGN.md"):
        text = re.sub(r"\s+", " ", open(os.path.join(ROOT, path)).read())
        assert "FASTQ records" in text and "read_qual" in text and "fastq_records" in text, path


# ---- the refusals, made before any GPU call ----------------------------------------------------------------------
def _rq(q_min=1, thr=(300, 200, 200, 5), skip=60, min_q=0):
    from rawnanoporesignalcompression_amd import _native

    p = _native.ReadQualParams()
    p.mean.q_min, p.mean.nthresholds, p.skip_bases, p.min_mean_q = q_min, len(thr), skip, min_q
    p.mean.thr[:len(thr)] = list(thr)
    return p


def test_read_qual_call_refusals_and_their_order():
    from rawnanoporesignalcompression_amd import _native

    fn = getattr(_native.load(), RQ)
    bad = _native.PGN_ERR_INVALID_ARG
    dummy = C.c_void_p(0x1000)

    def call(ctx=dummy, p=_rq(), nreads=2, rb=dummy, st=dummy, qual=dummy, bcap=10, mq=dummy, es=dummy, ps=dummy):
        return fn(ctx, C.byref(p) if p is not None else None, nreads, rb, st, qual, bcap, mq, es, ps, None)

    assert call(ctx=None) == bad
    assert call(p=None) == bad
    assert call(p=_rq(94, ())) == bad                          # q_min + nthresholds <= 93
    assert call(p=_rq(90, (4, 3, 2, 1))) == bad
    assert call(p=_rq(1, (5, 6))) == bad                       # non-increasing
    assert call(p=_rq(1, (5, 6)), nreads=0) == bad             # ... whatever else holds
    assert call(nreads=1 << 32) == bad
    assert call(nreads=1 << 32, rb=None, qual=None) == bad
    for name in ("rb", "st", "mq", "ps", "qual"):
        assert call(**{name: None}) == bad, name
    assert call(ctx=None, p=_rq(94, ()), nreads=1 << 32, rb=None, qual=None) == bad
    # nothing to do: PGN_OK without a look at the context or at any array; err_sum may always be missing
    assert call(nreads=0, rb=None, st=None, mq=None, es=None, ps=None) == 0
    assert call(nreads=0, rb=None, st=None, mq=None, ps=None, qual=None, bcap=0) == 0
    assert call(nreads=0, qual=None) == bad                    # base_capacity > 0 wants d_qual
    assert call(ctx=None, nreads=0) == bad


def _fq(flags=0, names=(b"qs", b"ch"), tags=None):
    from rawnanoporesignalcompression_amd import _native

    p = _native.FastqParams(flags, len(names))
    for k, name in enumerate(names[:8]):
        p.tag_name[k][:] = list(name)
        p.d_tag[k] = 0x2000 if tags is None else tags[k]
    return p


def test_record_call_refusals_and_their_order():
    from rawnanoporesignalcompression_amd import _native

    fn = getattr(_native.load(), REC)
    bad = _native.PGN_ERR_INVALID_ARG
    dummy = C.c_void_p(0x1000)

    def call(ctx=dummy, p=_fq(), nreads=2, ids=dummy, rb=dummy, st=dummy, keep=None, seq=dummy, qual=dummy, bcap=10,
             out=dummy, cap=100, off=dummy, rst=dummy):
        return fn(ctx, C.byref(p) if p is not None else None, nreads, ids, rb, st, keep, seq, qual, bcap, out, cap, off,
                  rst, None)

    assert call(ctx=None) == bad
    assert call(p=None) == bad
    assert call(p=_fq(flags=2)) == bad
    assert call(p=_fq(flags=1 << 31)) == bad
    over = _fq()
    over.ntags = 9
    assert call(p=over) == bad
    for name in (b"1s", b"q-", b" s", b"q ", b"\x00\x00", b"_a", b"a_", b"q\xe9"):
        assert call(p=_fq(names=(b"qs", name))) == bad, name
    assert call(p=_fq(names=(b"qs", b"1s")), nreads=0) == bad       # ... whatever else holds
    assert call(nreads=1 << 32) == bad
    for name in ("ids", "rb", "st", "rst"):
        assert call(**{name: None}) == bad, name
    assert call(p=_fq(tags=[0x2000, 0])) == bad                     # a NULL column among the first ntags
    assert call(off=None) == bad
    assert call(off=None, nreads=0) == bad
    assert call(seq=None) == bad
    assert call(qual=None) == bad
    assert call(out=None) == bad
    assert call(ctx=None, p=_fq(flags=2), nreads=1 << 32, ids=None, off=None, seq=None, out=None) == bad
    # empty capacities need no arrays, but d_rec_off does not go away
    assert call(bcap=0, seq=None, qual=None, cap=0, out=None, off=None) == bad


# ---- the models ----------------------------------------------------------------------------------------------------
def three_line_formatter(c):
    """Every kept read's record by uuid.UUID, an f-string and slices."""
    out, off = [], [0]
    kept = K.kept_mask(c)
    for r in range(len(c.status)):
        if kept[r]:
            a, b = int(c.read_bases[r]), int(c.read_bases[r + 1])
            tags = "".join(f"\t{name}:i:{int(v[r])}" for name, v in c.tags)
            s, q = c.seq[a:b].tobytes().decode("latin1"), c.qual[a:b].tobytes().decode("latin1")
            s, q = (s[::-1], q[::-1]) if c.reverse else (s, q)
            out.append(f"@{uuid.UUID(bytes=c.ids[r].tobytes())}{tags}\n{s}\n+\n{q}\n".encode("latin1"))
        off.append(off[-1] + (len(out[-1]) if kept[r] else 0))
    return out, off, kept


@pytest.fixture(scope="module")
def cases():
    return K.record_cases()


def test_record_model_against_the_formatter(cases):
    from rawnanoporesignalcompression_amd import _native
    from rawnanoporesignalcompression_amd.host import fastq_bound

    rng = np.random.default_rng(1)
    extra = [K.make(f"random{i}", rng.integers(0, 50, int(rng.integers(1, 30))).tolist(), 100 + i, reverse=bool(i & 1))
             for i in range(6)]
    for i, c in enumerate(extra):
        n = len(c.status)
        c.tags = [(name, rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)) for name in ("qs", "B7", "zz")[:i % 4]]
        c.status = np.where(rng.random(n) < 0.2, 6, 0).astype(np.int32)
        c.keep = (rng.random(n) < 0.7).astype(np.uint8) if i % 3 else None
    for c in list(cases) + extra:
        recs, off, kept = three_line_formatter(c)
        text, rec_off, st = c.expected()
        assert rec_off.dtype == np.uint64 and rec_off.tolist() == off, c.name
        assert fastq_bound(len(c.status), len(c.seq), len(c.tags)) >= off[-1], c.name
        fits = np.array([off[r + 1] <= c.capacity for r in range(len(kept))], bool)
        assert text == b"".join(rec for rec, r in zip(recs, np.flatnonzero(kept)) if fits[r]), c.name
        want = np.where(kept, np.where(fits, 0, _native.PGN_ERR_DST_TOO_SMALL), c.status)
        assert st.dtype == np.int32 and np.array_equal(st, want), c.name


def test_record_model_refuses_bad_arguments():
    from rawnanoporesignalcompression_amd.host import fastq_records_signal

    ids, seq, rb, st = np.zeros((2, 16), np.uint8), np.full(5, 65, np.uint8), [0, 2, 5], [0, 0]
    for tags in ({"q": [1, 2]}, {"1s": [1, 2]}, {"qs": [1]}, {"qs": [1, -1]}, {"qs": [1, 1 << 32]},
                 {f"t{k}": [1, 2] for k in range(9)}):
        with pytest.raises(ValueError):
            fastq_records_signal(ids, seq, seq, rb, st, tags)
    with pytest.raises(ValueError):
        fastq_records_signal(ids[:1], seq, seq, rb, st)
    with pytest.raises(ValueError):
        fastq_records_signal(ids, seq, seq, rb, [0])


def test_read_qual_model_against_an_integer_loop():
    from rawnanoporesignalcompression_amd.host import err_table, qual_thresholds

    table = [int(v) for v in err_table()]
    for c in K.qual_cases():
        thr = qual_thresholds(q_min=c.q_min, q_max=max(c.q_min, 50)) if c.thresholds is None else c.thresholds
        mq, U, ps = c.expected()
        assert (mq.dtype, U.dtype, ps.dtype) == (np.uint32, np.uint64, np.uint8)
        for r in range(len(c.status)):
            a, b = int(c.read_bases[r]), int(c.read_bases[r + 1])
            want = (0, 0, 0)
            if c.status[r] == 0 and b > a and b <= len(c.qual):
                s = c.skip_bases if b - a > c.skip_bases else 0
                total = 0
                for g in range(a + s, b):
                    total += table[min(max(int(c.qual[g]), 33), 126) - 33]
                q = c.q_min
                for t in thr.tolist():
                    q += 1 if total <= t * (b - a - s) else 0
                want = (q, total, 1 if q >= c.min_mean_q else 0)
            assert (int(mq[r]), int(U[r]), int(ps[r])) == want, (c.name, r)


def test_err_table_against_its_closed_form():
    from rawnanoporesignalcompression_amd.host import err_table, read_qual_params

    err = err_table()
    step = np.diff(err.astype(np.int64))
    assert err.dtype == np.uint32 and err.shape == (94,) and (step <= 0).all() and (step[:80] < 0).all()
    decimal.getcontext().prec = 60
    for q in (0, 1, 10, 40, 93):
        exact = decimal.Decimal(2) ** 32 * decimal.Decimal(10) ** (decimal.Decimal(-q) / 10)
        want = min(2 ** 32 - 1, int(exact.to_integral_value(rounding=decimal.ROUND_HALF_EVEN)))
        assert int(err[q]) == want, q
    assert int(err[0]) == 2 ** 32 - 1 and int(err[10]) == 429496730 and int(err[40]) == 429497
    p = read_qual_params(None, 1, 60, 9)
    assert (p.mean.q_min, p.mean.nthresholds, p.skip_bases, p.min_mean_q) == (1, 49, 60, 9) and list(p.err) == err.tolist()
    for kw in (dict(err=err[:93]), dict(skip_bases=-1), dict(min_mean_q=1 << 32), dict(err=-err.astype(np.int64))):
        with pytest.raises(ValueError):
            read_qual_params(**kw)


def test_fastq_bound():
    from rawnanoporesignalcompression_amd.host import fastq_bound

    assert fastq_bound(0, 0, 0) == 0 and fastq_bound(3, 10, 2) == 3 * 74 + 20
    c = K.tag_cases()[2]
    _, off, _ = c.expected()
    assert int(off[-1]) <= fastq_bound(len(c.status), len(c.seq), 8)
    # the bound is met by a read whose tags all have ten digits
    one = K.make("ten", [4], 1, tags=[(f"t{k}", [4294967295]) for k in range(8)])
    assert int(one.expected()[1][-1]) == fastq_bound(1, 4, 8)
