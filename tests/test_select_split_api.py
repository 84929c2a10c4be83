"""The plan of a long read's selection in parts (include/pgnano_hip.h, "Long reads"), without a GPU: the
host build of the plan function (pgnm_select_parts of libpgn_model.so, the code the device plan kernel
runs), its Python restatement, the setter's checks and the exported symbols.

The contract: a read of n samples is split when split_min_samples < n < 2^32, into
parts = min(ceil(n / part_samples), 4096) parts, part j covering [floor(j n / parts), floor((j + 1) n / parts)).
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_PARTS = 4096
NEW_SYMBOLS = ("pgn_ctx_set_select_split", "pgn_ctx_get_select_split", "pgn_select_split_counts")
# (split_min_samples, part_samples): the smallest the setter allows, unequal ones, the defaults, the largest part
SETTINGS = [(1024, 1024), (5000, 1024), (131072, 32768), (1 << 24, 1 << 24), (100_000, 3000)]


def _model():
    L = O.model()
    L.pgnm_select_parts.restype = C.c_int
    L.pgnm_select_parts.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]
    return L


def model_parts(n, split_min, part):
    """The C function's boundaries: parts + 1 values."""
    cnt = C.c_uint32(0)
    assert _model().pgnm_select_parts(n, split_min, part, C.byref(cnt), 0, None) == 0
    b = np.zeros(cnt.value + 1, np.uint64)
    assert _model().pgnm_select_parts(n, split_min, part, C.byref(cnt), b.size, b.ctypes.data) == 0
    assert cnt.value + 1 == b.size
    return b


def numpy_parts(n, split_min, part):
    """The contract restated: Python integers for the products (j * n passes 2^53), numpy for the rest."""
    parts = 1
    if split_min < n < 2 ** 32:
        parts = min((n + part - 1) // part, MAX_PARTS)
    j = np.arange(parts + 1, dtype=object)
    return np.array(j * n // parts, dtype=np.uint64)


def lengths(split_min, part):
    ns = {0, 1, split_min - 1, split_min, split_min + 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 5, MAX_PARTS * part,
          MAX_PARTS * part + 1, MAX_PARTS * part + 12_345}
    for m in (1, 2, 3, 7, 100, MAX_PARTS - 1, MAX_PARTS):
        ns |= {m * part - 1, m * part, m * part + 1}
    return sorted(n for n in ns if n >= 0)


@pytest.mark.parametrize("split_min,part", SETTINGS)
def test_plan_function_against_numpy(split_min, part):
    for n in lengths(split_min, part):
        got, want = model_parts(n, split_min, part), numpy_parts(n, split_min, part)
        assert np.array_equal(got, want), (n, split_min, part)
        parts = got.size - 1
        if n <= split_min or n >= 2 ** 32:
            assert parts == 1, n
        else:
            assert parts == min(-(-n // part), MAX_PARTS) and parts >= 2, n
        # the parts tile [0, n) and none is empty (a read of no samples has one empty part)
        assert int(got[0]) == 0 and int(got[-1]) == n
        if n:
            assert (np.diff(got.astype(object)) > 0).all(), n
        if 1 < parts < MAX_PARTS:
            assert int(np.diff(got.astype(object)).max()) <= part, n


def test_the_cap():
    got = model_parts(MAX_PARTS * 1024 + 12_345, 1024, 1024)
    assert got.size - 1 == MAX_PARTS
    assert set(np.diff(got.astype(np.int64)).tolist()) == {1027, 1028}
    assert model_parts(MAX_PARTS * 1024 + 1, 1024, 1024).size - 1 == MAX_PARTS
    assert model_parts(MAX_PARTS * 1024, 1024, 1024).size - 1 == MAX_PARTS
    assert model_parts((MAX_PARTS - 1) * 1024 + 1, 1024, 1024).size - 1 == MAX_PARTS
    assert model_parts((MAX_PARTS - 1) * 1024, 1024, 1024).size - 1 == MAX_PARTS - 1


@pytest.mark.parametrize("split_min,part", SETTINGS)
def test_python_select_parts_equals_the_c_function(split_min, part):
    from rawnanoporesignalcompression_amd import select_parts

    for n in lengths(split_min, part):
        got = select_parts(n, split_min, part)
        assert got.dtype == np.uint64 and np.array_equal(got, model_parts(n, split_min, part)), (n, split_min, part)


BAD_SETTINGS = [(1024, 1023), (1 << 25, (1 << 24) + 1), (1023, 1024), (32767, 32768), (0, 0)]


def test_rejected_settings():
    """part_samples outside [1024, 2^24] and split_min_samples < part_samples: the plan function, the Python
    restatement and the context's setter (argument checks come before the context is touched)."""
    from rawnanoporesignalcompression_amd import _native, select_parts

    lib = _native.load()
    bad, dummy = _native.PGN_ERR_INVALID_ARG, C.c_void_p(0x1000)
    cnt = C.c_uint32(0)
    for split_min, part in BAD_SETTINGS:
        assert _model().pgnm_select_parts(10_000, split_min, part, C.byref(cnt), 0, None) == -1
        with pytest.raises(ValueError):
            select_parts(10_000, split_min, part)
        assert lib.pgn_ctx_set_select_split(dummy, C.byref(_native.SelectSplit(split_min, part, 4, 0))) == bad
    assert _model().pgnm_select_parts(10_000, 1024, 1024, None, 0, None) == -1
    assert lib.pgn_ctx_set_select_split(dummy, C.byref(_native.SelectSplit(4096, 1024, 65537, 0))) == bad
    assert lib.pgn_ctx_set_select_split(dummy, None) == bad
    ok = _native.SelectSplit(4096, 1024, 65536, 0)
    assert lib.pgn_ctx_set_select_split(None, C.byref(ok)) == bad
    assert lib.pgn_ctx_get_select_split(None, C.byref(ok)) == bad
    assert lib.pgn_ctx_get_select_split(dummy, None) == bad
    out = (C.c_uint64 * 5)()
    assert lib.pgn_select_split_counts(None, C.byref(out)) == bad
    assert lib.pgn_select_split_counts(dummy, None) == bad


def test_symbols_declared_exported_and_bound():
    import rawnanoporesignalcompression_amd as pkg
    from rawnanoporesignalcompression_amd import _native

    src = open(os.path.join(ROOT, "include", "pgnano_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = C.CDLL(_native.LIB_PATH)
    sigs = {s[0]: s for s in _native.SIGNATURES}
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert hasattr(lib, name), name
        assert sigs[name][1] is C.c_int and len(sigs[name][2]) == 2
    assert hasattr(C.CDLL(O.MODEL_SO), "pgnm_select_parts")
    assert re.search(r"#define\s+PGN_SELECT_MAX_PARTS\s+4096\b", code) and _native.PGN_SELECT_MAX_PARTS == MAX_PARTS
    m = re.search(r"typedef struct pgn_select_split \{([^}]*)\}", code)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == "uint32_t split_min_samples, part_samples, max_split_reads, pad;"
    S = _native.SelectSplit
    assert C.sizeof(S) == 16 and [f for f, _ in S._fields_] == ["split_min_samples", "part_samples", "max_split_reads", "pad"]
    assert "select_parts" in pkg.__all__
    for attr in ("select_split", "set_select_split", "select_split_counts"):
        assert hasattr(pkg.PGNanoCodec, attr), attr


def test_not_covered_lists_no_longer_name_the_split():
    for path in ("README.md", "DESIGN.md", os.path.join("include", "pgnano_hip.h")):
        text = re.sub(r"\s+", " ", open(os.path.join(ROOT, path)).read())
        for m in re.finditer(r"Not covered:[^.]*\.", text):
            assert "several workgroups" not in m.group(0), (path, m.group(0))
