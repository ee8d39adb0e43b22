"""omr_hough_angles_batch_device / omr_get_angles_with_hough_batch / omr_hough_vote_select_device without a GPU: the
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

from oics import _lib, hough
from oics._lib import OmrImage, OmrImageOwned

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

WANT = {
    "omr_hough_angles_batch_device": ("int", ["constuint8_t*", "int32_t", "int64_t", "int32_t", "int32_t", "int32_t", "int64_t",
                                              "double", "double", "double*", "int32_t*", "int32_t*", "uint8_t*", "int64_t",
                                              "int64_t", "void*"]),
    "omr_get_angles_with_hough_batch": ("int", ["constomr_image*", "int32_t", "double", "double", "double*", "int32_t*",
                                                "omr_image_owned*"]),
    "omr_hough_vote_select_device": ("int", ["constfloat*", "constint32_t*", "int32_t", "int32_t*", "void*"]),
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
    dev = _lib.SYMBOLS["omr_hough_angles_batch_device"][1]
    assert dev[9] is _lib.f64p and dev[10] is _lib.i32p and dev[11] is _lib.i32p and dev[0] is C.c_void_p and dev[12] is C.c_void_p
    host = _lib.SYMBOLS["omr_get_angles_with_hough_batch"][1]
    assert host[0] == C.POINTER(OmrImage) and host[-1] == C.POINTER(OmrImageOwned)


def _dev(scans=0x1000, n=2, stride=96, rows=8, cols=10, cn=1, step=12, angles=True, rc=True, n_lines=True, lined=0x9000,
         lstride=256, lstep=32):
    ang, r, nl = np.full(4, 7.0), np.full(4, -9, np.int32), np.full(4, -9, np.int32)
    code = _lib.lib().omr_hough_angles_batch_device(C.c_void_p(scans), n, stride, rows, cols, cn, step, 10.0, 2.0,
                                                    ang.ctypes.data_as(_lib.f64p) if angles else None,
                                                    r.ctypes.data_as(_lib.i32p) if rc else None,
                                                    nl.ctypes.data_as(_lib.i32p) if n_lines else None,
                                                    C.c_void_p(lined) if lined else None, lstride, lstep, None)
    assert (ang == 7.0).all() and (r == -9).all() and (nl == -9).all()  # a refused call writes nothing
    return code


def test_device_form_argument_errors_before_any_device_work():
    """none of these addresses is a device pointer: each call must answer without touching a device"""
    assert _dev(scans=0) == -5 and "null pointer" in _err()
    assert _dev(angles=False) == -5 and "null pointer" in _err()
    assert _dev(rc=False) == -5 and "null pointer" in _err()
    assert _dev(n=0) == -5 and "empty batch" in _err()
    assert _dev(n=-3) == -5 and "empty batch" in _err()
    for bad in (dict(rows=0), dict(cols=0), dict(rows=-1), dict(cols=-4)):
        assert _dev(**bad) == -215 and "empty image" in _err(), bad
    for bad in (dict(rows=32767), dict(cols=32767, step=40000, lstep=120000, lstride=1 << 20)):
        assert _dev(**bad) == -215 and "SHRT_MAX" in _err(), bad
    for cn in (0, 2, 5, -1):
        assert _dev(cn=cn, step=64) == -215 and "1, 3 or 4 channels" in _err(), cn
    assert _dev(step=9) == -5 and "step_bytes too small" in _err()
    assert _dev(cn=3, step=29) == -5 and "step_bytes too small" in _err()
    assert _dev(cn=4, step=39) == -5 and "step_bytes too small" in _err()
    assert _dev(stride=-1) == -5 and "negative scan stride" in _err()
    assert _dev(lstep=29) == -5 and "step too small" in _err()
    assert _dev(lstride=255) == -5 and "picture stride smaller than a picture" in _err()
    assert _dev(lined=0x1000) == -5 and "in place" in _err()
    # the valid calls are the only ones that reach the device: made only where there is none (on a GPU they would run
    # Canny on the invented addresses).  Without pictures the picture's pitch and stride are not looked at
    if _lib.lib().omr_device_count() == 0:
        assert {_dev(lined=0, lstep=0, lstride=0), _dev(), _dev(n_lines=False), _dev(cn=3, step=30), _dev(cn=4, step=40),
                _dev(stride=0)} == {-217}


def _host(n=3, grays=True, angles=True, rc=True, lined=True, bad=None):
    a = np.full((12, 10, 3), 255, np.uint8)
    ims = (OmrImage * 3)(OmrImage(a.ctypes.data, 12, 10, 3, 30), OmrImage(a.ctypes.data, 6, 30, 1, 30),
                         OmrImage(a.ctypes.data, 12, 10, 3, 30))
    if bad:
        for k, v in bad.items():
            setattr(ims[1], k, v)
    ang, r = np.full(3, 7.0), np.full(3, -9, np.int32)
    pics = (OmrImageOwned * 3)()
    code = _lib.lib().omr_get_angles_with_hough_batch(ims if grays else None, n, 10.0, 2.0,
                                                      ang.ctypes.data_as(_lib.f64p) if angles else None,
                                                      r.ctypes.data_as(_lib.i32p) if rc else None, pics if lined else None)
    assert (ang == 7.0).all() and (r == -9).all()  # no call below may leave a partial result
    assert not any(p.data for p in pics)
    return code


def test_host_form_argument_errors_before_any_device_work():
    assert _host(grays=False) == -5 and "bad batch arguments" in _err()
    assert _host(angles=False) == -5 and _host(rc=False) == -5
    assert _host(n=0) == -5 and _host(n=-2) == -5
    # an invalid image in the middle fails the whole call, with omr_get_angle_with_hough's code and message
    assert _host(bad={"data": None}) == -5 and "null image" in _err()
    assert _host(bad={"step_bytes": 29}) == -5 and "step_bytes too small" in _err()
    assert _host(bad={"rows": 0}) == -215 and _host(bad={"cols": 32767}) == -215
    for cn in (0, 2, 5):
        assert _host(bad={"channels": cn}) == -215 and "1, 3 or 4 channels" in _err(), cn
    if _lib.lib().omr_device_count() == 0:
        assert _host() == -217 and _host(lined=False) == -217 and _host(bad={"channels": 4, "cols": 7}) == -217


def test_vote_hook_argument_errors():
    L = _lib.lib()
    p = C.c_void_p(0x1000)
    assert L.omr_hough_vote_select_device(None, p, 1, p, None) == -5 and "null pointer" in _err()
    assert L.omr_hough_vote_select_device(p, None, 1, p, None) == -5
    assert L.omr_hough_vote_select_device(p, p, 1, None, None) == -5
    assert L.omr_hough_vote_select_device(p, p, 0, p, None) == -5 and "empty batch" in _err()
    if L.omr_device_count() == 0:
        assert L.omr_hough_vote_select_device(p, p, 1, p, None) == -217


def test_python_front_doors():
    sig = inspect.signature(hough.get_angles_with_hough)
    assert list(sig.parameters) == ["grays", "min_line_length", "max_line_gap", "want_pictures"]
    assert sig.parameters["want_pictures"].default is False
    assert list(inspect.signature(hough.hough_angles_batch_device).parameters) == [
        "d_scans", "n", "scan_stride_bytes", "rows", "cols", "channels", "step_bytes", "min_line_length", "max_line_gap",
        "d_lined", "lined_stride_bytes", "lined_step", "stream"]
    a = np.zeros((6, 5, 2), np.uint8)
    for pics in (False, True):
        with pytest.raises(_lib.OmrError) as e:
            hough.get_angles_with_hough([np.zeros((6, 5), np.uint8), a], 10.0, 2.0, want_pictures=pics)
        assert e.value.code == -215
        with pytest.raises(_lib.OmrError) as e:
            hough.get_angles_with_hough([], 10.0, 2.0, want_pictures=pics)
        assert e.value.code == -5
    with pytest.raises(_lib.OmrError) as e:
        hough.hough_angles_batch_device(0x1000, 2, -1, 8, 10, 1, 10, 10.0, 2.0)
    assert e.value.code == -5 and "negative scan stride" in e.value.message


def test_shim_has_the_batch_forms():
    src = open(os.path.join(ROOT, "shim", "oics", "src", "hough.rs")).read()
    m = re.search(r"pub fn get_angles_with_hough\((.*?)\)\s*->\s*Vec<opencv::Result<f64>>(.*?)\n\}\n", src, re.S)
    assert m, "hough::get_angles_with_hough"
    params = " ".join(m.group(1).split())
    assert "&[&TransformableMatrix]" in params and params.count("f64") == 2
    assert "ffi::omr_get_angles_with_hough_batch(" in m.group(2) and "null_mut()" in m.group(2)
    m = re.search(r"pub fn get_angles_with_hough_with_pictures\((.*?)\)\s*->\s*Vec<opencv::Result<\(f64, Mat\)>>(.*?)\n\}\n",
                  src, re.S)
    assert m, "hough::get_angles_with_hough_with_pictures"
    assert "ffi::omr_get_angles_with_hough_batch(" in m.group(2) and "into_mat(" in m.group(2)
