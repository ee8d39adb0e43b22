"""omr_structuring_element / omr_morph / omr_morph_device / omr_morph_batch_device without a GPU: the library's
structuring elements against the numpy restatement (tests/morph_ref.py), every argument error -- each returned before
any device work (a device call on a machine without a GPU would be -217) -- and the Python and Rust front doors."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import morph_ref as mr
from oics import _lib, transfer
from oics._lib import OmrImage, OmrImageOwned

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants():
    assert (_lib.OMR_MORPH_RECT, _lib.OMR_MORPH_CROSS, _lib.OMR_MORPH_ELLIPSE) == (0, 1, 2) == (mr.RECT, mr.CROSS, mr.ELLIPSE)
    assert (_lib.OMR_MORPH_ERODE, _lib.OMR_MORPH_DILATE) == (0, 1) == (mr.ERODE, mr.DILATE)
    assert (transfer.MORPH_RECT, transfer.MORPH_CROSS, transfer.MORPH_ELLIPSE) == (0, 1, 2)
    for name in ("omr_structuring_element", "omr_morph", "omr_morph_device", "omr_morph_batch_device"):
        assert name in _lib.SYMBOLS


@pytest.mark.parametrize("shape", [mr.RECT, mr.CROSS, mr.ELLIPSE])
def test_structuring_element_equals_the_restatement(shape):
    for kw in range(1, 34):
        for kh in range(1, 34):
            for anchor in {(-1, -1), (0, 0), (kw - 1, kh - 1), (kw // 3, kh - 1 - kh // 3), (-1, 0), (kw - 1, -1)}:
                got = transfer.get_structuring_element(shape, (kw, kh), anchor)
                assert got.shape == (kh, kw)
                assert (got == mr.get_structuring_element(shape, (kw, kh), anchor)).all(), (shape, kw, kh, anchor)


def test_structuring_element_errors():
    out = np.zeros(64, np.uint8)
    p = out.ctypes.data_as(_lib.u8p)
    f = _lib.lib().omr_structuring_element
    assert f(0, 3, 3, -1, -1, p) == 0
    assert f(0, 3, 3, -1, -1, None) == -5
    for kw, kh in ((0, 3), (3, 0), (-1, 3), (3, -2)):
        assert f(0, kw, kh, -1, -1, p) == -215
    for ax, ay in ((3, 1), (1, 3), (-2, 1), (1, -2), (5, 5)):
        assert f(1, 3, 3, ax, ay, p) == -215
    for shape in (-1, 3, 100):
        assert f(shape, 3, 3, -1, -1, p) == -215
    assert b"shape" in _lib.lib().omr_last_error()


def _dev(src=0x1000, sstep=30, rows=8, cols=10, cn=3, op=0, shape=2, kw=3, kh=3, ax=-1, ay=-1, it=1, dst=0x9000, dstep=30):
    return _lib.lib().omr_morph_device(C.c_void_p(src), sstep, rows, cols, cn, op, shape, kw, kh, ax, ay, it,
                                       C.c_void_p(dst), dstep, None)


def _batch(src=0x1000, n=2, sstride=240, sstep=30, rows=8, cols=10, cn=3, op=0, shape=2, kw=3, kh=3, ax=-1, ay=-1, it=1,
           dst=0x9000, dstride=240, dstep=30):
    return _lib.lib().omr_morph_batch_device(C.c_void_p(src), n, sstride, sstep, rows, cols, cn, op, shape, kw, kh, ax, ay,
                                             it, C.c_void_p(dst), dstride, dstep, None)


def _host(img=True, out=True, **kw):
    a = np.zeros((8, 10, kw.pop("cn", 3)), np.uint8)
    im = OmrImage(a.ctypes.data, kw.pop("rows", 8), kw.pop("cols", 10), a.shape[2], kw.pop("step", a.strides[0]))
    o = OmrImageOwned()
    d = dict(op=0, shape=2, kw=3, kh=3, ax=-1, ay=-1, it=1)
    d.update(kw)
    return _lib.lib().omr_morph(C.byref(im) if img else None, d["op"], d["shape"], d["kw"], d["kh"], d["ax"], d["ay"],
                                d["it"], C.byref(o) if out else None)


ELEMENT_ERRORS = [dict(kw=0), dict(kh=0), dict(kw=-3), dict(ax=3), dict(ay=3), dict(ax=-2), dict(ay=-7), dict(shape=3),
                  dict(shape=-1)]


def test_argument_errors_before_any_device_work():
    """none of these pointers is a device pointer: each call must return its code without touching a device"""
    for call in (_dev, _batch):
        assert call(src=0) == -5 and call(dst=0) == -5
        assert call(src=0x1000, dst=0x1000) == -5                      # in place, as omr_erode3_device
        assert call(it=-1) == -5
        assert call(op=2) == -5 and call(op=-1) == -5
        assert call(sstep=29) == -5 and call(dstep=29) == -5
        for bad in (dict(rows=0), dict(cols=0), dict(rows=-1), dict(rows=32767), dict(cols=32767), dict(cn=0), dict(cn=5)):
            assert call(**bad) == -215, bad
        for bad in ELEMENT_ERRORS:
            assert call(**bad) == -215, bad
    assert _batch(n=0) == -5 and _batch(n=-3) == -5
    assert _batch(sstride=239) == -5 and _batch(dstride=100) == -5
    assert _host(img=False) == -5 and _host(out=False) == -5
    assert _host(it=-1) == -5 and _host(op=7) == -5
    assert _host(step=29) == -5
    assert _host(rows=0) == -215 and _host(cols=0) == -215
    for bad in ELEMENT_ERRORS:
        assert _host(**bad) == -215, bad


def test_python_methods_have_the_reference_parameter_order():
    for name in ("erode", "dilate"):
        sig = inspect.signature(getattr(transfer.TransformableMatrix, name))
        assert list(sig.parameters) == ["self", "kernel_shape", "kernel_size", "anchor", "iterations"]
    sig = inspect.signature(transfer.get_structuring_element)
    assert list(sig.parameters) == ["shape", "size", "anchor"] and sig.parameters["anchor"].default == (-1, -1)


def test_shim_erode_and_dilate_call_the_library():
    src = open(os.path.join(ROOT, "shim", "oics", "src", "transfer.rs")).read()
    for name, op in (("dilate", 1), ("erode", 0)):
        m = re.search(r"pub fn %s\(&self.*?\n    \}\n" % name, src, re.S)
        assert m, name
        body = m.group(0)
        assert "ffi::omr_morph(" in body and re.search(r"omr_morph\(&view\(&self\.matrix\)\?, %d," % op, body)
        assert "imgproc::erode" not in body and "imgproc::dilate" not in body
    code = "\n".join(l for l in src.splitlines() if not l.lstrip().startswith("//"))
    assert "imgproc::" not in code
