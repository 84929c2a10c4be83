"""pgn_decompress_batch_device_pa (calibrated float output of the batched decode): the C ABI surface
and the definition of the value, without a GPU.

The value is numpy's ``(x.astype(float32) + float32(offset)) * float32(scale)`` -- the arithmetic of
the reference reader's ``Read.calibrate_signal_array`` (pod5/python/pod5/src/pod5/reader.py:356-368:
``offset = np.float32(...)``, ``scale = np.float32(...)``, ``(signal_array_adc + offset) * scale``) --
and, for float16, that value through ``astype(float16)``.
"""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "pgn_decompress_batch_device_pa"


def ref_pa(x, off, scale, dtype=np.float32):
    """The reference for every value test of the calibrated decode (explicit casts)."""
    ref32 = (np.asarray(x).astype(np.float32) + np.float32(off)) * np.float32(scale)
    return ref32 if dtype == np.float32 else ref32.astype(np.float16)


def reader_calibrate(signal_array_adc, offset, scale):
    """Read.calibrate_signal_array's body, as the reference's reader.py writes it."""
    offset = np.float32(offset)
    scale = np.float32(scale)
    return (signal_array_adc + offset) * scale


def test_symbol_declared_exported_and_bound():
    from rawnanoporesignalcompression_amd import _native

    src = open(os.path.join(ROOT, "include", "pgnano_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", code)
    m = re.search(r"typedef enum pgn_out_type \{([^}]*)\}", code)
    assert m and [t.strip() for t in m.group(1).split(",")] == ["PGN_OUT_INT16 = 0", "PGN_OUT_F32 = 1", "PGN_OUT_F16 = 2"]
    lib = _native.load()
    assert hasattr(lib, NAME)
    sig = {s[0]: s for s in _native.SIGNATURES}[NAME]
    assert sig[1] is C.c_int and len(sig[2]) == 15
    assert (_native.PGN_OUT_INT16, _native.PGN_OUT_F32, _native.PGN_OUT_F16) == (0, 1, 2)


def test_invalid_arguments_before_any_gpu_call():
    """A NULL context is PGN_ERR_INVALID_ARG (no device is touched: this runs without one)."""
    from rawnanoporesignalcompression_amd import _native

    lib = _native.load()
    fn = getattr(lib, NAME)
    for out_type in (_native.PGN_OUT_INT16, _native.PGN_OUT_F32, _native.PGN_OUT_F16, 7):
        rc = fn(None, _native.VARIANTS["C5"], 0, 1, None, None, None, None, out_type, None, None, None, None, None, None)
        assert rc == _native.PGN_ERR_INVALID_ARG
    assert fn(None, _native.PGN_POD5_CODEC_VBZ, 0, 0, None, None, None, None, 1, None, None, None, None, None,
              None) == _native.PGN_ERR_INVALID_ARG


def test_reference_helper_is_the_readers_formula():
    """ref_pa (and the package's calibrate_signal) give the bits calibrate_signal_array gives, with
    calibration values for which the roundings matter."""
    from rawnanoporesignalcompression_amd import calibrate_signal

    x = np.array([-32768, -1234, -1, 0, 1, 7, 255, 256, 4097, 32767], np.int16)
    off, scale = -243.37, 0.18310547
    want = reader_calibrate(x, off, scale)
    assert want.dtype == np.float32
    got = ref_pa(x, off, scale)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32))
    assert np.array_equal(calibrate_signal(x, off, scale).view(np.int32), want.view(np.int32))
    h = ref_pa(x, off, scale, np.float16)
    assert h.dtype == np.float16 and np.array_equal(h.view(np.uint16), want.astype(np.float16).view(np.uint16))
    assert np.array_equal(calibrate_signal(x, off, scale, np.float16).view(np.uint16), h.view(np.uint16))


def test_calibration_values_make_rounding_matter():
    """Over all 65,536 int16 values with the tests' calibration: a float64 intermediate changes many
    float32 results and a truncating float16 conversion changes many float16 results, so wrong
    arithmetic in a kernel cannot pass the bit comparison."""
    x = np.arange(-32768, 32768).astype(np.int16)
    off, scale = -243.37, 0.18310547
    ref32 = ref_pa(x, off, scale)
    wide = ((x.astype(np.float64) + np.float64(np.float32(off))) * np.float64(np.float32(scale))).astype(np.float32)
    assert int((wide.view(np.int32) != ref32.view(np.int32)).sum()) > 10_000
    ref16 = ref32.astype(np.float16)
    # round toward zero: drop the 13 low mantissa bits of the float32 before an (exact) conversion
    trunc = (ref32.view(np.uint32) & np.uint32(0xFFFFE000)).view(np.float32).astype(np.float16)
    assert int((trunc.view(np.uint16) != ref16.view(np.uint16)).sum()) > 20_000
