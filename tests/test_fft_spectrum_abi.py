"""omr_fft_spectrum_raw without a GPU: the symbol with the header's signature (header, ctypes table, built library,
ffi.rs), every argument error -- omr_get_fft_image's, returned before any device work with omr_last_error() set and
nothing written -- -217 for a valid call where there is no device, and the Python front door."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest

from oics import _lib, fft
from oics._lib import OmrImage, OmrImageOwned

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

NAME = "omr_fft_spectrum_raw"
ARGS = ["constomr_image*", "float*", "float*", "float*", "omr_image_owned*", "omr_image_owned*"]


def _err():
    return _lib.lib().omr_last_error().decode()


def test_symbol_exists_with_the_headers_signature():
    import gen_shim_ffi as g
    decls = {name: (ret, [t.replace(" ", "") for t, _ in params]) for name, ret, params in g.parse_header()}
    assert decls[NAME] == ("int", ARGS)
    assert hasattr(C.CDLL(_lib.LIB_PATH), NAME), "libomrdeskew.so does not export %s" % NAME
    res, argtypes = _lib.SYMBOLS[NAME]
    assert res is C.c_int and argtypes == [C.POINTER(OmrImage), _lib.f32p, _lib.f32p, _lib.f32p, C.POINTER(OmrImageOwned),
                                           C.POINTER(OmrImageOwned)]
    ffi = open(os.path.join(ROOT, "shim", "oics", "src", "ffi.rs")).read()
    m = re.search(r"pub fn %s\((.*?)\) -> c_int;" % NAME, ffi)
    assert m and [a.split(":")[1].strip() for a in m.group(1).split(",")] == [
        "*const OmrImage", "*mut f32", "*mut f32", "*mut f32", "*mut OmrImageOwned", "*mut OmrImageOwned"]
    # documented as what it is, next to omr_get_fft_image
    header = open(os.path.join(ROOT, "include", "omrdeskew.h")).read()
    doc = header[header.index("int omr_get_fft_image("):header.index("int %s(" % NAME)]
    assert "Inspection hook" in doc and "UNSHIFTED" in doc


def _call(rows=6, cols=10, channels=1, step=10, data=True, outputs=True):
    a = np.full((12, 30), 200, np.uint8)
    im = OmrImage(a.ctypes.data if data else None, rows, cols, channels, step)
    half = 16
    row, mag, ext = np.full(2 * half * 12, 7.0, np.float32), np.full(half * 12, 7.0, np.float32), np.full(2, 7.0, np.float32)
    m, lg = OmrImageOwned(), OmrImageOwned()
    if outputs:
        code = _lib.lib().omr_fft_spectrum_raw(C.byref(im), row.ctypes.data_as(_lib.f32p), mag.ctypes.data_as(_lib.f32p),
                                               ext.ctypes.data_as(_lib.f32p), C.byref(m), C.byref(lg))
    else:
        code = _lib.lib().omr_fft_spectrum_raw(C.byref(im), None, None, None, None, None)
    # a refused call writes nothing
    assert (row == 7.0).all() and (mag == 7.0).all() and (ext == 7.0).all() and not m.data and not lg.data
    return code


def test_argument_errors_before_any_device_work():
    assert _lib.lib().omr_fft_spectrum_raw(None, None, None, None, None, None) == -5 and "null image" in _err()
    assert _call(data=False) == -5 and "null image" in _err()
    assert _call(step=9) == -5 and "step_bytes too small" in _err()
    for bad in (dict(rows=0), dict(cols=0), dict(rows=-1), dict(cols=32767, step=40000), dict(rows=32767)):
        assert _call(**bad) == -215, bad
    for cn in (0, 2, 5):
        assert _call(channels=cn, step=60) == -215 and "1, 3 or 4 channels" in _err(), cn
    for cn in (3, 4):
        assert _call(channels=cn, cols=7, step=30) == -215 and "8-bit single-channel image" in _err(), cn
    assert _call(outputs=False) == -5 and "null output" in _err()


def test_no_gpu_is_minus_217_and_nothing_is_written():
    """the valid call is the only one that reaches the device: checked where there is none"""
    if _lib.lib().omr_device_count() == 0:
        assert _call() == -217
        with pytest.raises(_lib.OmrError) as e:
            fft.spectrum_raw(np.zeros((6, 10), np.uint8))
        assert e.value.code == -217


def test_python_front_door():
    assert list(inspect.signature(fft.spectrum_raw).parameters) == ["gray_tm"]
    with pytest.raises(_lib.OmrError) as e:
        fft.spectrum_raw(np.zeros((6, 5, 3), np.uint8))
    assert e.value.code == -215
