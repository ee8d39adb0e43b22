"""omr_projection_pictures / _device / _batch_device without a GPU: the three symbols in the header, the ctypes table
and the built library, every argument error -- each returned before any device work (a device call on a machine
without a GPU would be -217) -- and the Python and Rust front doors."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from oics import _lib, transfer
from oics._lib import OmrImage, OmrImageOwned

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("omr_projection_pictures", "omr_projection_pictures_device", "omr_projection_pictures_batch_device")


def test_symbols_in_header_table_and_library():
    header = open(os.path.join(ROOT, "include", "omrdeskew.h")).read()
    L = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.SYMBOLS
        assert hasattr(L, name), "libomrdeskew.so does not export %s" % name


def _host(img=True, h=True, v=True, rows=8, cols=10, cn=1, step=None, data=True):
    a = np.zeros((8, 10 * max(cn, 1)), np.uint8)
    im = OmrImage(a.ctypes.data if data else None, rows, cols, cn, a.strides[0] if step is None else step)
    oh, ov = OmrImageOwned(), OmrImageOwned()
    return _lib.lib().omr_projection_pictures(C.byref(im) if img else None, C.byref(oh) if h else None,
                                              C.byref(ov) if v else None)


def _dev(src=0x1000, sstep=12, rows=8, cols=10, h=0x9000, hstep=12, v=0x20000, vstep=12):
    return _lib.lib().omr_projection_pictures_device(C.c_void_p(src), sstep, rows, cols, C.c_void_p(h), hstep,
                                                     C.c_void_p(v), vstep, None)


def _batch(src=0x1000, n=2, sstride=96, sstep=12, rows=8, cols=10, h=0x9000, hstride=96, hstep=12, v=0x20000, vstride=96,
           vstep=12):
    return _lib.lib().omr_projection_pictures_batch_device(C.c_void_p(src), n, sstride, sstep, rows, cols, C.c_void_p(h),
                                                           hstride, hstep, C.c_void_p(v), vstride, vstep, None)


def test_argument_errors_before_any_device_work():
    """none of these pointers is a device pointer: each call must return its code without touching a device"""
    for call in (_dev, _batch):
        assert call(src=0) == -5                                        # null pointer
        assert call(h=0, v=0) == -5                                     # both outputs null
        assert call(sstep=9) == -5 and call(hstep=9) == -5 and call(vstep=9) == -5   # a step below cols
        assert call(h=0x1000) == -5 and call(v=0x1000) == -5            # d_src == d_dst
        for bad in (dict(rows=0), dict(cols=0), dict(rows=-1), dict(cols=-4), dict(rows=32767), dict(cols=32767)):
            assert call(**bad) == -215, bad                             # check_image_shape
    assert _batch(n=0) == -5 and _batch(n=-3) == -5
    assert _batch(hstride=95) == -5 and _batch(vstride=95) == -5        # a destination stride below rows * step
    assert _batch(sstride=-1) == -5                                     # a negative source stride
    assert _host(img=False) == -5 and _host(data=False) == -5
    assert _host(h=False, v=False) == -5
    assert _host(step=9) == -5
    assert _host(rows=0) == -215 and _host(cols=0) == -215 and _host(rows=32767) == -215
    for cn in (0, 2, 3, 4, 5):
        assert _host(cn=cn) == -215, cn                                 # the channel rule cn_one


def test_a_valid_call_without_a_gpu_is_a_gpu_error():
    if _lib.lib().omr_device_count() > 0:
        pytest.skip("a GPU is present")
    assert _host() == -217 and _host(h=False) == -217 and _host(v=False) == -217
    assert _dev() == -217 and _dev(h=0) == -217 and _dev(v=0) == -217
    assert _batch() == -217 and _batch(sstride=0) == -217              # any source stride >= 0 is valid
    with pytest.raises(_lib.OmrError) as e:
        transfer.transfer_thresh_binary_to_horizontal_projection(np.zeros((4, 4), np.uint8))
    assert e.value.code == -217


def test_python_front_door():
    for name in ("transfer_thresh_binary_to_horizontal_projection", "transfer_thresh_binary_to_vertical_projection"):
        assert list(inspect.signature(getattr(transfer, name)).parameters) == ["src"]
    assert list(inspect.signature(transfer.projection_pictures).parameters)[0] == "src"
    sig = inspect.signature(transfer.projection_pictures_batch_device)
    assert list(sig.parameters) == ["d_src", "n", "src_stride_bytes", "src_step", "rows", "cols", "d_horizontal",
                                    "h_stride_bytes", "h_step", "d_vertical", "v_stride_bytes", "v_step", "stream"]
    with pytest.raises(_lib.OmrError) as e:
        transfer.projection_pictures(np.zeros((4, 4), np.uint8), horizontal=False, vertical=False)
    assert e.value.code == -5
    with pytest.raises(_lib.OmrError) as e:
        transfer.projection_pictures_batch_device(0x1000, 0, 0, 4, 4, 4, 0x9000, 16, 4, 0, 0, 0)
    assert e.value.code == -5


def test_shim_pictures_call_the_library():
    src = open(os.path.join(ROOT, "shim", "oics", "src", "transfer.rs")).read()
    for name, args in (("horizontal", r"&mut out, std::ptr::null_mut\(\)"), ("vertical", r"std::ptr::null_mut\(\), &mut out")):
        m = re.search(r"pub fn transfer_thresh_binary_to_%s_projection\(src: &TransformableMatrix\) -> "
                      r"Result<TransformableMatrix, opencv::Error> \{.*?\n\}\n" % name, src, re.S)
        assert m, name
        body = m.group(0)
        assert re.search(r"ffi::omr_projection_pictures\(&view\(&src\.matrix\)\?, %s\)" % args, body), name
        assert "at_2d_mut" not in body and "at_row_mut" not in body and "for " not in body, name
    ffi = open(os.path.join(ROOT, "shim", "oics", "src", "ffi.rs")).read()
    for name in NAMES:
        assert re.search(r"pub fn %s\(" % name, ffi), name
