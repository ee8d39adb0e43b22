"""omr_lined_picture / _device / _batch_device and the two *_ex detectors without a GPU: the symbols in the header, the
ctypes table and the built library, every argument error -- each returned before any device work (a device call on a
machine without a GPU would be -217) -- and the Python and Rust front doors."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from oics import _lib, fft, hough
from oics._lib import OmrImage, OmrImageOwned, i32p, u8p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("omr_lined_picture", "omr_lined_picture_device", "omr_lined_picture_batch_device", "omr_get_angle_with_hough_ex",
         "omr_get_angle_with_fft_ex")
BGR = (C.c_uint8 * 3)(186, 88, 255)


def test_symbols_in_header_table_and_library():
    header = open(os.path.join(ROOT, "include", "omrdeskew.h")).read()
    L = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.SYMBOLS
        assert hasattr(L, name), "libomrdeskew.so does not export %s" % name


def test_header_matches_ctypes():
    """argument for argument: the header's C types against the ctypes table"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_shim_ffi
    kinds = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}
    parsed = {name: params for name, ret, params in gen_shim_ffi.parse_header()}
    for name in NAMES:
        res, args = _lib.SYMBOLS[name]
        assert res is C.c_int and len(args) == len(parsed[name]), name
        for (ctype, pname), a in zip(parsed[name], args):
            t = " ".join(ctype.replace("const", "").split())
            if t.endswith("*"):
                base = t[:-1].strip()
                want = {"omr_image": (C.POINTER(OmrImage),), "omr_image_owned": (C.POINTER(OmrImageOwned),),
                        "double": (_lib.f64p,), "void": (C.c_void_p,),
                        "int32_t": (i32p, C.c_void_p), "uint8_t": (u8p, C.c_void_p)}[base]  # device pointers travel as void *
                assert a in want, (name, pname, ctype, a)
            else:
                assert a is kinds[t], (name, pname, ctype, a)


def _host(img=True, rows=8, cols=10, cn=1, step=None, data=True, lines=((1, 1, 5, 5),), n_lines=None, bgr=True, out=True):
    a = np.zeros((8, 10 * max(cn, 1)), np.uint8)
    im = OmrImage(a.ctypes.data if data else None, rows, cols, cn, a.strides[0] if step is None else step)
    l = np.asarray(lines, np.int32).reshape(-1, 4) if lines is not None else None
    o = OmrImageOwned()
    return _lib.lib().omr_lined_picture(C.byref(im) if img else None, l.ctypes.data_as(i32p) if l is not None else None,
                                        (len(l) if l is not None else 0) if n_lines is None else n_lines,
                                        BGR if bgr else None, C.byref(o) if out else None)


def _dev(edges=0x1000, estep=12, rows=8, cols=10, lines=0x5000, n_lines=2, bgr=True, out=0x9000, ostep=32):
    return _lib.lib().omr_lined_picture_device(C.c_void_p(edges), estep, rows, cols, C.c_void_p(lines), n_lines,
                                               BGR if bgr else None, C.c_void_p(out), ostep, None)


def _batch(edges=0x1000, n=2, estride=96, estep=12, rows=8, cols=10, lines=0x5000, off=(0, 2, 5), bgr=True, out=0x9000,
           ostride=256, ostep=32):
    o = np.asarray(off, np.int32) if off is not None else None
    return _lib.lib().omr_lined_picture_batch_device(C.c_void_p(edges), n, estride, estep, rows, cols, C.c_void_p(lines),
                                                     o.ctypes.data_as(i32p) if o is not None else None,
                                                     BGR if bgr else None, C.c_void_p(out), ostride, ostep, None)


def test_argument_errors_before_any_device_work():
    """none of these pointers is a device pointer: each call must return its code without touching a device"""
    for call in (_dev, _batch):
        assert call(edges=0) == -5 and call(out=0) == -5 and call(bgr=False) == -5      # null pointers
        assert call(lines=0) == -5                                                      # segments without a list
        assert call(estep=9) == -5 and call(ostep=29) == -5                             # a step below cols / 3 * cols
        assert call(out=0x1000) == -5                                                   # in place
        for bad in (dict(rows=0), dict(cols=0), dict(rows=-1), dict(cols=-4), dict(rows=32767), dict(cols=32767)):
            assert call(**bad) == -215, bad
    assert _dev(n_lines=-1) == -5
    assert _batch(n=0) == -5 and _batch(n=-3) == -5
    assert _batch(off=None) == -5
    assert _batch(off=(0, 3, 2)) == -5 and _batch(off=(2, 1, 1)) == -5                  # line_offsets must not decrease
    assert _batch(off=(-1, 0, 2)) == -5
    assert _batch(ostride=255) == -5 and _batch(estride=-1) == -5
    assert _host(img=False) == -5 and _host(data=False) == -5 and _host(out=False) == -5 and _host(bgr=False) == -5
    assert _host(n_lines=-1) == -5
    assert _host(lines=None, n_lines=1) == -5
    assert _host(step=9) == -5
    assert _host(rows=0) == -215 and _host(cols=0) == -215 and _host(rows=32767) == -215
    for cn in (0, 2, 3, 4, 5):
        assert _host(cn=cn) == -215, cn                                                 # the channel rule cn_one
    # an end point outside the 10 x 8 picture, each coordinate, each side
    for bad in ((10, 1, 5, 5), (1, 8, 5, 5), (1, 1, 10, 5), (1, 1, 5, 8), (-1, 1, 5, 5), (1, -1, 5, 5), (1, 1, -1, 5),
                (1, 1, 5, -1)):
        assert _host(lines=((0, 0, 9, 7), bad)) == -5, bad
        assert b"segment 1" in _lib.lib().omr_last_error()


def test_ex_detectors_refuse_what_the_detectors_refuse():
    a = np.zeros((8, 10), np.uint8)
    im = OmrImage(a.ctypes.data, 8, 10, 1, 10)
    ang, o = C.c_double(), OmrImageOwned()
    L = _lib.lib()
    assert L.omr_get_angle_with_hough_ex(None, 0.0, 0.0, C.byref(ang), C.byref(o)) == -5
    assert L.omr_get_angle_with_hough_ex(C.byref(im), 0.0, 0.0, None, C.byref(o)) == -5
    assert L.omr_get_angle_with_fft_ex(None, 50.0, 150.0, 0.0, 0.0, C.byref(ang), C.byref(o)) == -5
    assert L.omr_get_angle_with_fft_ex(C.byref(im), 50.0, 150.0, 0.0, 0.0, None, C.byref(o)) == -5
    im3 = OmrImage(a.ctypes.data, 8, 3, 3, 10)
    assert L.omr_get_angle_with_fft_ex(C.byref(im3), 50.0, 150.0, 0.0, 0.0, C.byref(ang), C.byref(o)) == -215
    assert not o.data


def test_a_valid_call_without_a_gpu_is_a_gpu_error():
    if _lib.lib().omr_device_count() > 0:
        pytest.skip("a GPU is present")
    assert _host() == -217 and _host(lines=None) == -217                               # n_lines == 0 is legal
    assert _dev() == -217 and _dev(n_lines=0, lines=0) == -217
    assert _batch() == -217 and _batch(off=(0, 0, 0), lines=0) == -217 and _batch(off=(3, 3, 5)) == -217
    with pytest.raises(_lib.OmrError) as e:
        hough.lined_picture(np.zeros((4, 4), np.uint8), [(0, 0, 3, 3)])
    assert e.value.code == -217


def test_python_front_door():
    for mod in (hough, fft):
        assert list(inspect.signature(mod.lined_picture).parameters) == ["edges", "lines", "color"]
        assert callable(mod.lined_picture_batch_device)
    assert inspect.signature(hough.lined_picture).parameters["color"].default == (186, 88, 255)
    assert list(inspect.signature(hough.lined_picture_batch_device).parameters) == [
        "d_edges", "n", "edge_stride_bytes", "edge_step", "rows", "cols", "d_lines", "line_offsets", "d_out",
        "out_stride_bytes", "out_step", "color", "stream"]
    assert inspect.signature(hough.get_angle_with_hough).parameters["want_picture"].default is False
    assert inspect.signature(fft.get_angle_with_fft).parameters["want_picture"].default is False
    with pytest.raises(_lib.OmrError) as e:
        hough.lined_picture(np.zeros((4, 4), np.uint8), [(0, 0, 4, 3)])
    assert e.value.code == -5
    with pytest.raises(_lib.OmrError) as e:
        fft.lined_picture_batch_device(0x1000, 1, 0, 4, 4, 4, 0x5000, [2, 1], 0x9000, 48, 12)
    assert e.value.code == -5
    with pytest.raises(ValueError):
        hough.lined_picture_batch_device(0x1000, 2, 16, 4, 4, 4, 0x5000, [0, 1], 0x9000, 48, 12)


def test_shim_detectors_write_the_library_picture():
    for f, ex in (("hough.rs", "omr_get_angle_with_hough_ex"), ("fft.rs", "omr_get_angle_with_fft_ex")):
        src = open(os.path.join(ROOT, "shim", "oics", "src", f)).read()
        m = re.search(r"pub fn get_angle_with_\w+\(.*?\n\}\n", src, re.S)
        assert m, f
        body = m.group(0)
        assert re.search(r"ffi::%s\(&v, .*?&mut angle, &mut lined\)" % ex, body, re.S), f
        assert "into_mat(lined)" in body and "imwrite" in body, f
        assert "omr_canny" not in body and "get_fft_image" not in body, f               # nothing runs a second time
    ffi = open(os.path.join(ROOT, "shim", "oics", "src", "ffi.rs")).read()
    for name in NAMES:
        assert re.search(r"pub fn %s\(" % name, ffi), name
