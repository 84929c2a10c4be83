"""Per-read normalisation (pgn_read_stats_device, pgn_decompress_reads_device_norm): the definitions,
the C ABI surface and the host build of the rank walk, without a GPU.

The contract (include/pgnano_hip.h), for a read x[0..n) and s = sort(x):
  q(p)   = s[floor(p * (double)(n - 1))]                       -- not numpy.quantile's virtual index
  m2     = s[(n-1)/2] + s[n/2]                                  -- twice the median
  mad4   = t[(n-1)/2] + t[n/2],  t = sort(|2 x - m2|)           -- four times the MAD
  quantile: centre = centre_mult * float32(a + b), spread = spread_mult * float32(b - a)
  medmad:   centre = 0.5f * float32(m2),           spread = spread_mult * (0.25f * float32(mad4))
  spread = spread_floor where spread < spread_floor
  out32 = (float32(adc) + (-centre)) * (1.0f / spread);  out16 = float16(out32)
ref_rank / ref_medmad / ref_stats / ref_norm below are these formulas with np.sort and explicit
np.float32 casts; the GPU tests import them.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _oracle as O
from test_decode_pa_api import ref_pa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS_CALL, NORM_CALL = "pgn_read_stats_device", "pgn_decompress_reads_device_norm"

# the parameters the value tests use (both modes)
QUANTILE = dict(mode="quantile", p=(0.2, 0.9), centre_mult=0.51, spread_mult=0.53, spread_floor=1.0)
MEDMAD = dict(mode="medmad", p=(0.2, 0.9), centre_mult=0.51, spread_mult=1.4826, spread_floor=1.0)
INT_FIELDS = ("n", "status", "q_lo", "q_hi", "m2", "mad4")


def ref_rank(x, p):
    """q(p) = sort(x)[floor(p * (double)(n - 1))]: one binary64 multiply, then floor."""
    s = np.sort(np.asarray(x, np.int16))
    k = int(np.floor(np.float64(p) * np.float64(s.size - 1)))
    return int(s[k])


def ref_medmad(x):
    """(m2, mad4): twice the median and four times the median absolute deviation, as integers."""
    v = np.asarray(x, np.int16).astype(np.int64)
    n = v.size
    s = np.sort(v)
    m2 = int(s[(n - 1) // 2] + s[n // 2])
    t = np.sort(np.abs(2 * v - m2))
    return m2, int(t[(n - 1) // 2] + t[n // 2])


def ref_stats(x, mode="quantile", p=(0.2, 0.9), centre_mult=0.51, spread_mult=0.53, spread_floor=1.0):
    """pgn_read_stats of one read as a dict (centre and spread are np.float32)."""
    x = np.asarray(x, np.int16)
    st = dict(n=int(x.size), status=0, q_lo=0, q_hi=0, m2=0, mad4=0, centre=np.float32(0), spread=np.float32(1))
    if x.size == 0:
        return st
    if mode == "quantile":
        a, b = ref_rank(x, p[0]), ref_rank(x, p[1])
        st.update(q_lo=a, q_hi=b, centre=np.float32(centre_mult) * np.float32(a + b),
                  spread=np.float32(spread_mult) * np.float32(b - a))
    else:
        m2, mad4 = ref_medmad(x)
        st.update(m2=m2, mad4=mad4, centre=np.float32(0.5) * np.float32(m2),
                  spread=np.float32(spread_mult) * (np.float32(0.25) * np.float32(mad4)))
    if st["spread"] < np.float32(spread_floor):
        st["spread"] = np.float32(spread_floor)
    assert st["centre"].dtype == np.float32 and st["spread"].dtype == np.float32
    return st


def ref_norm(x, centre, spread, dtype=np.float32):
    """The normalised read: the pA formula with offset = -centre and scale = 1.0f / spread."""
    inv = np.float32(1.0) / np.float32(spread)
    return ref_pa(np.asarray(x, np.int16), -np.float32(centre), inv, dtype)


def f32_bits(v):
    return int(np.array([v], np.float32).view(np.uint32)[0])


def assert_stats_equal(got, want, what=""):
    """got: one record of ReadStats.DTYPE (or a dict); every integer field and the float bits."""
    for k in INT_FIELDS:
        assert int(got[k]) == int(want[k]), f"{what}: {k} = {int(got[k])}, want {int(want[k])}"
    for k in ("centre", "spread"):
        assert f32_bits(got[k]) == f32_bits(want[k]), f"{what}: {k} = {got[k]!r}, want {want[k]!r}"


# ---- data patterns shared with the GPU tests -----------------------------------------------------
def narrow_band(rng, n):
    """Three distinct high bytes: what a 256-bin histogram of the high byte would pile into 3 bins."""
    return rng.integers(0x01C0, 0x03FF, n).astype(np.int16)


def constant(rng, n):
    return np.full(n, int(rng.integers(-32768, 32768)), np.int16)


def two_valued(rng, n):
    return np.where(rng.integers(0, 2, n) == 1, 32767, -32768).astype(np.int16)


def permuted_sweep(rng, n):
    """n distinct values of the full int16 sweep, in random order (the whole sweep when n = 65,536)."""
    return (rng.permutation(65536)[:n].astype(np.int32) - 32768).astype(np.int16)


PATTERNS = [narrow_band, constant, two_valued, permuted_sweep]


# ---- surface -------------------------------------------------------------------------------------
def _header():
    src = open(os.path.join(ROOT, "include", "pgnano_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_symbols_declared_exported_and_bound():
    from rawnanoporesignalcompression_amd import _native

    code = _header()
    lib = _native.load()
    sigs = {s[0]: s for s in _native.SIGNATURES}
    for name, nargs in ((STATS_CALL, 8), (NORM_CALL, 18)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", code)
        assert hasattr(lib, name)
        assert sigs[name][1] is C.c_int and len(sigs[name][2]) == nargs
    m = re.search(r"typedef enum pgn_norm_mode \{([^}]*)\}", code)
    assert m and [t.strip() for t in m.group(1).split(",")] == ["PGN_NORM_QUANTILE = 0", "PGN_NORM_MEDMAD = 1"]
    assert (_native.PGN_NORM_QUANTILE, _native.PGN_NORM_MEDMAD) == (0, 1)


def test_struct_layouts():
    from rawnanoporesignalcompression_amd import ReadStats, _native

    code = _header()
    for name in ("pgn_norm_params", "pgn_read_stats"):
        assert re.search(r"typedef struct " + name + r" \{", code)
    P, S = _native.NormParams, _native.ReadStats
    assert C.sizeof(P) == 40 and C.sizeof(S) == 32
    assert [(f, getattr(P, f).offset) for f, _ in P._fields_] == [
        ("mode", 0), ("pad", 4), ("p_lo", 8), ("p_hi", 16), ("centre_mult", 24), ("spread_mult", 28),
        ("spread_floor", 32), ("pad2", 36)]
    assert [(f, getattr(S, f).offset) for f, _ in S._fields_] == [
        ("n", 0), ("status", 8), ("q_lo", 12), ("q_hi", 14), ("m2", 16), ("mad4", 20), ("centre", 24), ("spread", 28)]
    assert ReadStats.DTYPE.itemsize == 32
    assert [ReadStats.DTYPE.fields[f][1] for f, _ in S._fields_] == [getattr(S, f).offset for f, _ in S._fields_]


def _params(**kw):
    from rawnanoporesignalcompression_amd import _native

    v = dict(mode=0, p_lo=0.2, p_hi=0.9, centre_mult=0.51, spread_mult=0.53, spread_floor=1.0)
    v.update(kw)
    return _native.NormParams(v["mode"], 0, v["p_lo"], v["p_hi"], v["centre_mult"], v["spread_mult"], v["spread_floor"], 0.0)


BAD_PARAMS = [dict(mode=2), dict(mode=-1), dict(p_lo=-0.1), dict(p_hi=1.5), dict(p_lo=float("nan")),
              dict(p_hi=float("nan")), dict(p_lo=0.9, p_hi=0.2), dict(centre_mult=float("inf")),
              dict(spread_mult=float("nan")), dict(spread_mult=float("-inf")), dict(spread_floor=0.0),
              dict(spread_floor=-1.0), dict(spread_floor=float("nan")), dict(mode=1, spread_floor=0.0),
              dict(mode=1, p_lo=2.0)]


def test_invalid_arguments_before_any_gpu_call():
    """Every invalid-argument case returns PGN_ERR_INVALID_ARG with a NULL or a dummy context: nothing
    is dereferenced and no device is touched (this runs without one)."""
    from rawnanoporesignalcompression_amd import _native

    lib = _native.load()
    stats, norm = getattr(lib, STATS_CALL), getattr(lib, NORM_CALL)
    bad = _native.PGN_ERR_INVALID_ARG
    dummy = C.c_void_p(0x1000)  # never dereferenced: validation comes first
    c5, f16, f32 = _native.VARIANTS["C5"], _native.PGN_OUT_F16, _native.PGN_OUT_F32
    ok = _params()

    def call_norm(ctx, prm, codec=c5, out_type=f16, adc=None, arrays=None):
        p = C.byref(prm) if prm is not None else None
        return norm(ctx, codec, 0, 1, 0, arrays, None, None, None, None, arrays, out_type, arrays, adc, p, None, None, None)

    assert call_norm(None, ok) == bad
    assert call_norm(dummy, None) == bad
    assert stats(None, 1, None, None, None, C.byref(ok), None, None) == bad
    assert stats(dummy, 1, None, None, None, None, None, None) == bad
    for kw in BAD_PARAMS:
        prm = _params(**kw)
        assert call_norm(dummy, prm, arrays=dummy) == bad, kw
        assert stats(dummy, 1, dummy, dummy, dummy, C.byref(prm), dummy, None) == bad, kw
    for codec in (77, -1, 6):
        assert call_norm(dummy, ok, codec=codec, arrays=dummy) == bad
    for out_type in (_native.PGN_OUT_INT16, 3, 7, -1):
        assert call_norm(dummy, ok, out_type=out_type, arrays=dummy) == bad
    # float32 needs the raw samples' buffer; missing arrays
    assert call_norm(dummy, ok, out_type=f32, arrays=dummy) == bad
    assert call_norm(dummy, ok, arrays=None) == bad
    assert stats(dummy, 1, None, dummy, dummy, C.byref(ok), dummy, None) == bad


def test_python_rejects_unknown_mode():
    from rawnanoporesignalcompression_amd import norm_params

    with pytest.raises(ValueError):
        norm_params(mode="mean")
    p = norm_params(**MEDMAD)
    assert p.mode == 1 and p.p_lo == 0.2 and abs(p.spread_mult - 1.4826) < 1e-6


# ---- definitions -----------------------------------------------------------------------------------
def test_ref_medmad_is_numpys_median_and_mad():
    """500 random reads of 1..300 samples, odd and even n, heavy ties: m2 / 2 and mad4 / 4 are
    np.median(x) and np.median(np.abs(x - np.median(x))) in float64, exactly."""
    rng = np.random.default_rng(7)
    odd = even = 0
    for i in range(500):
        n = int(rng.integers(1, 301))
        span = int(rng.choice([1, 2, 3, 10, 1000, 65536]))
        lo = int(rng.integers(-32768, 32768 - span + 1))
        x = rng.integers(lo, lo + span, n).astype(np.int16)
        m2, mad4 = ref_medmad(x)
        xf = x.astype(np.float64)
        assert m2 / 2 == np.median(xf)
        assert mad4 / 4 == np.median(np.abs(xf - np.median(xf)))
        odd += n & 1
        even += 1 - (n & 1)
    assert odd > 100 and even > 100


def test_rank_formula_is_not_numpy_quantile():
    """The rank is floor(p * (n - 1)) with the product rounded to binary64 first: on a ramp x[i] = i the
    statistic is that index itself, for every n and every p the tests use."""
    for p in (0.0, 0.2, 0.5, 0.9, 1.0):
        for n in range(1, 400):
            x = np.arange(n, dtype=np.int16)
            assert ref_rank(x, p) == int(np.floor(np.float64(p) * np.float64(n - 1)))
    assert ref_rank(np.arange(101, dtype=np.int16), 0.9) == 90
    assert ref_rank(np.arange(11, dtype=np.int16), 0.9) == 9


def test_normalise_signal_is_ref_norm():
    from rawnanoporesignalcompression_amd import normalise_signal

    x = np.arange(-32768, 32768).astype(np.int16)
    st = ref_stats(np.array([431, 572], np.int16), **dict(QUANTILE, p=(0.0, 1.0)))
    for dt, bits in ((np.float32, np.uint32), (np.float16, np.uint16)):
        assert np.array_equal(normalise_signal(x, st["centre"], st["spread"], dt).view(bits),
                              ref_norm(x, st["centre"], st["spread"], dt).view(bits))


def _typical_stats():
    """centre and spread of the tests' synthetic reads (level 500, sd 60) under both parameter sets."""
    x = O.synth_read(100, 20_000)
    return [ref_stats(x, **QUANTILE), ref_stats(x, **MEDMAD)]


def test_parameters_make_rounding_matter():
    """Over all 65,536 int16 values with the tests' parameters, each wrong arithmetic changes many
    results, so it cannot pass a bit comparison: a float64 intermediate, a true division by spread
    instead of the multiplication by inv, and a truncating float16 conversion.  The med/MAD centre is a
    multiple of 0.5, so its add is exact for every int16 and a wider intermediate cannot differ there:
    that count is asserted for the quantile parameters, whose centre is no such number."""
    x = np.arange(-32768, 32768).astype(np.int16)
    for mode, st in zip(("quantile", "medmad"), _typical_stats()):
        c, s = st["centre"], st["spread"]
        ref32 = ref_norm(x, c, s)
        inv = np.float32(1.0) / s
        wide = ((x.astype(np.float64) - np.float64(c)) * np.float64(inv)).astype(np.float32)
        n_wide = int((wide.view(np.int32) != ref32.view(np.int32)).sum())
        div = (x.astype(np.float32) + (-c)) / s
        assert div.dtype == np.float32
        n_div = int((div.view(np.int32) != ref32.view(np.int32)).sum())
        ref16 = ref32.astype(np.float16)
        trunc = (ref32.view(np.uint32) & np.uint32(0xFFFFE000)).view(np.float32).astype(np.float16)
        n_trunc = int((trunc.view(np.uint16) != ref16.view(np.uint16)).sum())
        print(f"centre {c!r} spread {s!r}: float64 intermediate {n_wide}, division {n_div}, truncation {n_trunc}")
        assert n_div > 5_000 and n_trunc > 20_000, (n_div, n_trunc)
        if mode == "quantile":
            assert n_wide > 5_000, n_wide
        else:
            assert float(c) * 2 == round(float(c) * 2) and n_wide == 0


# ---- the host build of the rank walk (libpgn_model.so) -----------------------------------------------
needs_model = pytest.mark.skipif(not os.path.exists(O.MODEL_SO), reason="libpgn_model.so not built")


def _model():
    L = O.model()
    L.pgnm_read_stats.restype = C.c_int
    L.pgnm_read_stats.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    L.pgnm_locate.restype = C.c_int
    L.pgnm_locate.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    return L


def model_stats(x, **params):
    from rawnanoporesignalcompression_amd import ReadStats, norm_params

    x = np.ascontiguousarray(x, np.int16)
    out = np.zeros(1, ReadStats.DTYPE)
    prm = norm_params(**params)
    assert _model().pgnm_read_stats(x.ctypes.data if x.size else None, x.size, C.byref(prm), out.ctypes.data) == 0
    return out[0]


@needs_model
def test_coarse_walk_against_cumulative_sums():
    L = _model()
    rng = np.random.default_rng(11)
    for trial in range(300):
        h = np.zeros(1024, np.uint32)
        nz = rng.choice(1024, int(rng.integers(1, 40)), replace=False)
        h[nz] = rng.integers(1, 5000, nz.size)
        total = int(h.sum())
        cum = np.cumsum(h.astype(np.int64))
        for ks in ([0], [total - 1], sorted(rng.integers(0, total, 2).tolist()), [int(rng.integers(0, total))] * 2):
            k = np.array(ks, np.uint32)
            b, r = np.zeros(2, np.uint32), np.zeros(2, np.uint32)
            assert L.pgnm_locate(h.ctypes.data, k.ctypes.data, k.size, b.ctypes.data, r.ctypes.data) == 0
            for i, kk in enumerate(ks):
                want = int(np.searchsorted(cum, kk, side="right"))
                assert int(b[i]) == want and int(r[i]) == kk - (int(cum[want - 1]) if want else 0), (trial, ks)


@needs_model
def test_host_rank_walk_against_the_references():
    """2,000 reads of 1..5,000 samples over the four data patterns; ranks from {0, 0.2, 0.5, 0.9, 1}
    (p_lo == p_hi included) and the median / MAD: every field of the host build equals the reference."""
    rng = np.random.default_rng(2026)
    ps = [0.0, 0.2, 0.5, 0.9, 1.0]
    pairs = [(a, b) for a in ps for b in ps if a <= b]
    for i in range(2000):
        n = int(rng.integers(1, 5001))
        x = PATTERNS[i % 4](rng, n)
        q = dict(QUANTILE, p=pairs[(i // 4) % len(pairs)])
        assert_stats_equal(model_stats(x, **q), ref_stats(x, **q), f"read {i} n {n} {q['p']}")
        assert_stats_equal(model_stats(x, **MEDMAD), ref_stats(x, **MEDMAD), f"read {i} n {n} medmad")


@needs_model
def test_host_rank_walk_edge_reads():
    rng = np.random.default_rng(5)
    reads = [np.zeros(0, np.int16), np.array([-32768], np.int16), np.array([32767, -32768], np.int16),
             permuted_sweep(rng, 65536), O.synth_read(3, 70_001), np.full(9, 500, np.int16)]
    for i, x in enumerate(reads):
        for prm in (QUANTILE, MEDMAD, dict(QUANTILE, p=(0.5, 0.5)), dict(QUANTILE, p=(0.0, 1.0))):
            assert_stats_equal(model_stats(x, **prm), ref_stats(x, **prm), f"edge read {i} {prm['mode']} {prm['p']}")
    flat = model_stats(np.full(9, 500, np.int16), **QUANTILE)
    assert float(flat["spread"]) == 1.0  # the floor
