"""omr_fft_angles_batch_device / omr_get_angles_with_fft_batch / omr_fourier_transform_batch_device without a GPU: the
symbols with the header's signatures (header, ctypes table, built library, ffi.rs), every argument error -- each
returned before any device work (the pointers handed in are not device pointers, and on a machine without a GPU a call
that reached the device would be -217) with omr_last_error() set -- and the Python and Rust front doors."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest

from oics import _lib, fft, omr
from oics._lib import OmrImage, OmrImageOwned

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

WANT = {
    "omr_fft_angles_batch_device": ("int", ["constuint8_t*", "int32_t", "int64_t", "int32_t", "int32_t", "int64_t", "double",
                                            "double", "double", "double", "double*", "int32_t*", "uint8_t*", "int64_t",
                                            "int64_t", "void*"]),
    "omr_get_angles_with_fft_batch": ("int", ["constomr_image*", "int32_t", "double", "double", "double", "double", "double*",
                                              "omr_image_owned*"]),
    "omr_fourier_transform_batch_device": ("int", ["constuint8_t*", "int32_t", "int64_t", "int32_t", "int32_t", "int32_t",
                                                   "int64_t", "double", "double", "double", "double", "double*", "int32_t*",
                                                   "int32_t*", "void*"]),
}


def _err():
    return _lib.lib().omr_last_error().decode()


def test_symbols_exist_with_the_headers_signatures():
    import gen_shim_ffi as g
    decls = {name: (ret, [t.replace(" ", "") for t, _ in params]) for name, ret, params in g.parse_header()}
    L = C.CDLL(_lib.LIB_PATH)
    ffi = open(os.path.join(ROOT, "shim", "oics", "src", "ffi.rs")).read()
    for name, (ret, args) in WANT.items():
        assert name in decls, name
        assert decls[name][0].strip() == ret
        assert decls[name][1] == args, (name, decls[name][1])
        assert hasattr(L, name), "libomrdeskew.so does not export %s" % name
        res, argtypes = _lib.SYMBOLS[name]
        assert res is C.c_int and len(argtypes) == len(args)
        m = re.search(r"pub fn %s\((.*?)\)" % name, ffi)
        assert m and len(m.group(1).split(",")) == len(args), name
    # the host arrays travel as typed pointers, the device addresses as void *
    dev = _lib.SYMBOLS["omr_fft_angles_batch_device"][1]
    assert dev[10] is _lib.f64p and dev[11] is _lib.i32p and dev[0] is C.c_void_p and dev[12] is C.c_void_p
    four = _lib.SYMBOLS["omr_fourier_transform_batch_device"][1]
    assert four[11] is _lib.f64p and four[12] is _lib.i32p and four[13] is _lib.i32p and four[0] is C.c_void_p
    host = _lib.SYMBOLS["omr_get_angles_with_fft_batch"][1]
    assert host[0] == C.POINTER(OmrImage) and host[-1] == C.POINTER(OmrImageOwned) and host[-2] is _lib.f64p


def _dev(scans=0x1000, n=2, stride=96, rows=8, cols=10, step=12, angles=True, n_lines=True, lined=0x9000, lstride=256,
         lstep=32):
    ang, nl = np.full(4, 7.0), np.full(4, -9, np.int32)
    code = _lib.lib().omr_fft_angles_batch_device(C.c_void_p(scans), n, stride, rows, cols, step, 50.0, 150.0, 10.0, 2.0,
                                                  ang.ctypes.data_as(_lib.f64p) if angles else None,
                                                  nl.ctypes.data_as(_lib.i32p) if n_lines else None,
                                                  C.c_void_p(lined) if lined else None, lstride, lstep, None)
    assert (ang == 7.0).all() and (nl == -9).all()  # a refused call writes nothing
    return code


def test_fft_device_form_argument_errors_before_any_device_work():
    """none of these addresses is a device pointer: each call must answer without touching a device"""
    assert _dev(scans=0) == -5 and "null pointer" in _err()
    assert _dev(angles=False) == -5 and "null pointer" in _err()
    assert _dev(n=0) == -5 and "empty batch" in _err()
    assert _dev(n=-3) == -5 and "empty batch" in _err()
    for bad in (dict(rows=0), dict(cols=0), dict(rows=-1), dict(cols=-4)):
        assert _dev(**bad) == -215 and "empty image" in _err(), bad
    for bad in (dict(rows=32767), dict(cols=32767, step=40000, lstep=120000, lstride=1 << 20)):
        assert _dev(**bad) == -215 and "SHRT_MAX" in _err(), bad
    assert _dev(step=9) == -5 and "step_bytes too small" in _err()
    assert _dev(stride=-1) == -5 and "negative scan stride" in _err()
    assert _dev(lstep=29) == -5 and "step too small" in _err()
    assert _dev(lstride=255) == -5 and "picture stride smaller than a picture" in _err()
    assert _dev(lined=0x1000) == -5 and "in place" in _err()
    # the valid calls are the only ones that reach the device: made only where there is none (on a GPU they would
    # transform the invented addresses).  Without pictures the picture's pitch and stride are not looked at
    if _lib.lib().omr_device_count() == 0:
        assert {_dev(lined=0, lstep=0, lstride=0), _dev(), _dev(n_lines=False), _dev(stride=0)} == {-217}


def _four(scans=0x1000, n=2, stride=400, rows=8, cols=10, cn=3, step=32, angles=True, status=True, n_lines=True):
    ang, st, nl = np.full(4, 7.0), np.full(4, -9, np.int32), np.full(4, -9, np.int32)
    code = _lib.lib().omr_fourier_transform_batch_device(C.c_void_p(scans), n, stride, rows, cols, cn, step, 50.0, 150.0, 10.0,
                                                         2.0, ang.ctypes.data_as(_lib.f64p) if angles else None,
                                                         st.ctypes.data_as(_lib.i32p) if status else None,
                                                         nl.ctypes.data_as(_lib.i32p) if n_lines else None, None)
    assert (ang == 7.0).all() and (st == -9).all() and (nl == -9).all()
    return code


def test_fourier_device_form_argument_errors_before_any_device_work():
    assert _four(scans=0) == -5 and "null pointer" in _err()
    assert _four(angles=False) == -5 and "null pointer" in _err()
    assert _four(n=0) == -5 and "empty batch" in _err()
    assert _four(n=-1) == -5 and "empty batch" in _err()
    for bad in (dict(rows=0), dict(cols=0), dict(rows=-2)):
        assert _four(**bad) == -215 and "empty image" in _err(), bad
    for bad in (dict(rows=32767), dict(cols=32767, step=200000)):
        assert _four(**bad) == -215 and "SHRT_MAX" in _err(), bad
    for cn in (0, 2, 5, -1):
        assert _four(cn=cn, step=64) == -215 and "1, 3 or 4 channels" in _err(), cn
    assert _four(cn=1) == -215 and "RGB2GRAY) needs 3 or 4 channels" in _err()  # the per-call form's code and message
    assert _four(step=29) == -5 and "step_bytes too small" in _err()
    assert _four(cn=4, step=39) == -5 and "step_bytes too small" in _err()
    assert _four(stride=-1) == -5 and "negative scan stride" in _err()
    if _lib.lib().omr_device_count() == 0:
        assert {_four(), _four(cn=4, step=40), _four(status=False), _four(n_lines=False), _four(stride=0)} == {-217}


def _host(n=3, grays=True, angles=True, lined=True, bad=None):
    a = np.full((12, 30), 255, np.uint8)
    ims = (OmrImage * 3)(OmrImage(a.ctypes.data, 12, 10, 1, 30), OmrImage(a.ctypes.data, 6, 30, 1, 30),
                         OmrImage(a.ctypes.data, 12, 10, 1, 30))
    if bad:
        for k, v in bad.items():
            setattr(ims[1], k, v)
    ang = np.full(3, 7.0)
    pics = (OmrImageOwned * 3)()
    code = _lib.lib().omr_get_angles_with_fft_batch(ims if grays else None, n, 50.0, 150.0, 10.0, 2.0,
                                                    ang.ctypes.data_as(_lib.f64p) if angles else None, pics if lined else None)
    assert (ang == 7.0).all()  # no call below may leave a partial result
    assert not any(p.data for p in pics)
    return code


def test_host_form_argument_errors_before_any_device_work():
    assert _host(grays=False) == -5 and "bad batch arguments" in _err()
    assert _host(angles=False) == -5
    assert _host(n=0) == -5 and _host(n=-2) == -5
    # an invalid image in the middle fails the whole call, with omr_get_angle_with_fft's code and message
    assert _host(bad={"data": None}) == -5 and "null image" in _err()
    assert _host(bad={"step_bytes": 29}) == -5 and "step_bytes too small" in _err()
    assert _host(bad={"rows": 0}) == -215 and _host(bad={"cols": 32767}) == -215
    for cn in (0, 2, 5):
        assert _host(bad={"channels": cn}) == -215 and "1, 3 or 4 channels" in _err(), cn
    for cn in (3, 4):
        assert _host(bad={"channels": cn, "cols": 7}) == -215 and "8-bit single-channel image" in _err(), cn
    if _lib.lib().omr_device_count() == 0:
        assert _host() == -217 and _host(lined=False) == -217 and _host(n=1) == -217


def test_python_front_doors():
    sig = inspect.signature(fft.get_angles_with_fft)
    assert list(sig.parameters) == ["grays", "canny_threshold_1", "canny_threshold_2", "min_line_length", "max_line_gap",
                                    "want_pictures"]
    assert sig.parameters["want_pictures"].default is False
    assert list(inspect.signature(fft.fft_angles_batch_device).parameters) == [
        "d_scans", "n", "scan_stride_bytes", "rows", "cols", "step_bytes", "canny_threshold_1", "canny_threshold_2",
        "min_line_length", "max_line_gap", "d_lined", "lined_stride_bytes", "lined_step", "stream"]
    assert list(inspect.signature(omr.fourier_transform_batch_device).parameters) == [
        "d_scans_ptr", "n", "scan_stride", "rows", "cols", "channels", "step", "canny_threshold_weak",
        "canny_threshold_strong", "fourier_min_line_length", "fourier_max_line_gap", "stream"]
    a = np.zeros((6, 5, 3), np.uint8)
    for pics in (False, True):
        with pytest.raises(_lib.OmrError) as e:
            fft.get_angles_with_fft([np.zeros((6, 5), np.uint8), a], 50.0, 150.0, 10.0, 2.0, want_pictures=pics)
        assert e.value.code == -215
        with pytest.raises(_lib.OmrError) as e:
            fft.get_angles_with_fft([], 50.0, 150.0, 10.0, 2.0, want_pictures=pics)
        assert e.value.code == -5
    with pytest.raises(_lib.OmrError) as e:
        fft.fft_angles_batch_device(0x1000, 2, -1, 8, 10, 10, 50.0, 150.0, 10.0, 2.0)
    assert e.value.code == -5 and "negative scan stride" in e.value.message
    with pytest.raises(_lib.OmrError) as e:
        omr.fourier_transform_batch_device(0x1000, 2, 400, 8, 10, 1, 10, 50.0, 150.0, 10.0, 2.0)
    assert e.value.code == -215


def test_shim_has_the_batch_forms():
    src = open(os.path.join(ROOT, "shim", "oics", "src", "fft.rs")).read()
    m = re.search(r"pub fn get_angles_with_fft\((.*?)\)\s*->\s*opencv::Result<Vec<f64>>(.*?)\n\}\n", src, re.S)
    assert m, "fft::get_angles_with_fft"
    params = " ".join(m.group(1).split())
    assert "&[&TransformableMatrix]" in params and params.count("f64") == 4
    assert "ffi::omr_get_angles_with_fft_batch(" in m.group(2) and "null_mut()" in m.group(2)
    m = re.search(r"pub fn get_angles_with_fft_with_pictures\((.*?)\)\s*->\s*opencv::Result<Vec<\(f64, Mat\)>>(.*?)\n\}\n",
                  src, re.S)
    assert m, "fft::get_angles_with_fft_with_pictures"
    assert "ffi::omr_get_angles_with_fft_batch(" in m.group(2) and "into_mat" in m.group(2)
