"""omr_projection_batch_deskew_canvas / omr_projection_batch_deskew_device / omr_deskew_with_projections_batch without a
GPU: the three symbols with the header's signatures (header, ctypes table, built library, ffi.rs), every argument
error that needs no context -- each returned before any device work (the pointers handed in are host pointers, and on a
machine without a GPU a call that reached the device would be -217) with the outputs untouched -- and the Python and
Rust front doors.  A context exists only where there is a device: the canvas query against omr_rotate_size over the
candidate angles and the refusals that look at the context (n outside 1..max_scans, a slot one byte too small, interp
2) are check_context_refusals below, which tests/test_gpu_projection_deskew.py runs on real contexts."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest

from oics import _lib, projection
from oics._lib import OmrImage, OmrImageOwned

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

WANT = {
    "omr_projection_batch_deskew_canvas": ("int", ["omr_projection_batch*", "int32_t*", "int32_t*"]),
    "omr_projection_batch_deskew_device": ("int", ["omr_projection_batch*", "constuint8_t*", "int64_t", "int64_t", "int32_t",
                                                   "int32_t", "constuint8_t*", "uint8_t*", "int64_t", "int64_t", "int32_t*",
                                                   "double*", "int32_t*"]),
    "omr_deskew_with_projections_batch": ("int", ["constomr_image*", "int32_t", "uint16_t", "double", "double", "int32_t",
                                                  "constuint8_t*", "double*", "int32_t*", "omr_image_owned*"]),
}
WHITE = (C.c_uint8 * 4)(255, 255, 255, 0)
HOST = np.zeros(64, np.uint8)  # a host buffer: nothing below may touch it


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
    dev = _lib.SYMBOLS["omr_projection_batch_deskew_device"][1]
    assert dev[6] is _lib.u8p and dev[10] is _lib.i32p and dev[11] is _lib.f64p and dev[12] is _lib.i32p
    assert dev[1] is C.c_void_p and dev[7] is C.c_void_p  # the device addresses travel as void *
    host = _lib.SYMBOLS["omr_deskew_with_projections_batch"][1]
    assert host[0] == C.POINTER(OmrImage) and host[-1] == C.POINTER(OmrImageOwned)


def _deskew(handle, scans=True, stride=0, step=64, n=1, interp=1, border=True, out=True, out_stride=1 << 20, out_step=4096,
            size=True, angle=True):
    """one call with host pointers; the outputs must come back as they went in"""
    p = C.c_void_p(HOST.ctypes.data)
    ang, idx, sz = np.full(4, 7.0), np.full(4, -9, np.int32), np.full(8, -9, np.int32)
    rc = _lib.lib().omr_projection_batch_deskew_device(handle, p if scans else None, stride, step, n, interp,
                                                       WHITE if border else None, p if out else None, out_stride, out_step,
                                                       sz.ctypes.data_as(_lib.i32p) if size else None,
                                                       ang.ctypes.data_as(_lib.f64p) if angle else None,
                                                       idx.ctypes.data_as(_lib.i32p))
    assert (ang == 7.0).all() and (idx == -9).all() and (sz == -9).all()  # a refused call writes nothing
    assert not HOST.any()
    return rc


def test_a_null_context_is_refused_before_any_device_work():
    L = _lib.lib()
    r, c = C.c_int32(-3), C.c_int32(-3)
    assert L.omr_projection_batch_deskew_canvas(None, C.byref(r), C.byref(c)) == -5
    assert (r.value, c.value) == (-3, -3)
    assert _deskew(None) == -5 and _deskew(None, interp=2) == -5


def test_create_keeps_its_channel_rules():
    h = C.c_void_p()
    L = _lib.lib()
    assert L.omr_projection_batch_create(100, 80, 4, 45, 0.2, 0.2, 0, 4, C.byref(h)) == -213 and not h.value
    assert L.omr_projection_batch_create(100, 80, 2, 45, 0.2, 0.2, 0, 4, C.byref(h)) == -215 and not h.value


def test_the_valid_create_is_the_only_call_that_reaches_the_device():
    """a context needs a device: the canvas against omr_rotate_size and the refusals that look at the context are made in
    tests/test_gpu_projection_deskew.py, with check_context_refusals below"""
    L = _lib.lib()
    h = C.c_void_p()
    rc = L.omr_projection_batch_create(320, 400, 3, 45, 0.5, 1.0, 0, 3, C.byref(h))
    if L.omr_device_count() == 0:
        assert rc == -217 and not h.value
    else:
        assert rc == 0 and h.value
        L.omr_projection_batch_destroy(h)


def expected_canvas(rows, cols, max_angle, step):
    """omr_rotate_size (CONTAIN) maximised over the candidate angles (idx - N) * step; columns rounded up to 4"""
    N, A = projection.candidate_count(max_angle, step)
    R = Cc = 0
    r, c = C.c_int32(), C.c_int32()
    for i in range(A):
        assert _lib.lib().omr_rotate_size(rows, cols, (i - N) * step, 1, C.byref(r), C.byref(c)) == 0
        R, Cc = max(R, r.value), max(Cc, c.value)
    return R, (Cc + 3) & ~3


def check_context_refusals(h, rows, cols, cn, max_angle, step):
    """the canvas query of context h (max_scans 3) against omr_rotate_size, and every refusal that looks at the context:
    each with host pointers, so none may reach the device"""
    L = _lib.lib()
    r, c = C.c_int32(), C.c_int32()
    assert L.omr_projection_batch_deskew_canvas(h, C.byref(r), C.byref(c)) == 0
    R, Cc = expected_canvas(rows, cols, max_angle, step)
    assert (r.value, c.value) == (R, Cc)  # the FULL shape's canvas, whatever the working shape
    assert c.value % 4 == 0
    assert L.omr_projection_batch_deskew_canvas(h, None, C.byref(c)) == -5
    assert L.omr_projection_batch_deskew_canvas(h, C.byref(r), None) == -5
    ok = dict(step=cols * cn, out_step=Cc * cn, out_stride=R * Cc * cn)
    assert _deskew(h, scans=False, **ok) == -5 and _deskew(h, border=False, **ok) == -5
    assert _deskew(h, out=False, **ok) == -5 and _deskew(h, size=False, **ok) == -5 and _deskew(h, angle=False, **ok) == -5
    assert _deskew(h, n=0, **ok) == -5 and _deskew(h, n=-1, **ok) == -5 and _deskew(h, n=4, **ok) == -5
    assert _deskew(h, **dict(ok, step=cols * cn - 1)) == -5
    assert _deskew(h, stride=-1, **ok) == -5
    assert _deskew(h, **dict(ok, out_step=Cc * cn - 1)) == -5  # a slot too small by one byte, across ...
    assert _deskew(h, **dict(ok, out_stride=R * Cc * cn - 1)) == -5  # ... and down
    assert _deskew(h, **dict(ok, out_step=1 << 62)) == -5  # rows x pitch leaves 64 bits: still too small a stride
    for interp in (2, 3, 4, -1):
        assert _deskew(h, interp=interp, **ok) == -213, interp
        assert "interpolation flag" in L.omr_last_error().decode()


def _host(n=3, srcs=True, angles=True, rotated=True, border=True, interp=1, max_angle=45, step=0.2, scale=0.5, bad=None):
    a = np.full((12, 10, 3), 255, np.uint8)
    ims = (OmrImage * 3)(OmrImage(a.ctypes.data, 12, 10, 3, 30), OmrImage(a.ctypes.data, 6, 10, 3, 30),
                         OmrImage(a.ctypes.data, 12, 10, 3, 30))
    if bad:
        for k, v in bad.items():
            setattr(ims[1], k, v)
    ang, idx = np.full(3, 7.0), np.full(3, -9, np.int32)
    pics = (OmrImageOwned * 3)()
    rc = _lib.lib().omr_deskew_with_projections_batch(ims if srcs else None, n, max_angle, step, scale, interp,
                                                      WHITE if border else None, ang.ctypes.data_as(_lib.f64p) if angles else None,
                                                      idx.ctypes.data_as(_lib.i32p), pics if rotated else None)
    assert (ang == 7.0).all() and (idx == -9).all()  # no call below may leave a partial result
    assert not any(p.data for p in pics)
    return rc


def test_host_form_argument_errors_before_any_device_work():
    assert _host(srcs=False) == -5 and _host(angles=False) == -5 and _host(rotated=False) == -5 and _host(border=False) == -5
    assert _host(n=0) == -5 and _host(n=-2) == -5
    assert _host(max_angle=0) == -5
    for interp in (2, 4, -1):
        assert _host(interp=interp) == -213, interp
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert _host(scale=bad) == -5, bad
    # an invalid image in the middle fails the whole call, with omr_get_angle_with_projections' code
    assert _host(bad={"data": None}) == -5
    assert _host(bad={"step_bytes": 29}) == -5
    assert _host(bad={"rows": 0}) == -215 and _host(bad={"cols": 32767}) == -215
    assert _host(bad={"channels": 2}) == -215 and _host(bad={"channels": 5}) == -215
    assert _host(bad={"rows": 1}) == -215  # 1 * 0.5 truncates to 0
    if _lib.lib().omr_device_count() == 0:
        assert _host() == -217 and _host(bad={"channels": 4, "step_bytes": 40}) == -217


def test_python_front_doors():
    sig = inspect.signature(projection.get_angles_and_deskew)
    assert list(sig.parameters) == ["srcs", "max_angle", "step", "resize_scale", "interp", "border", "want_idx"]
    assert sig.parameters["interp"].default == 1 and sig.parameters["border"].default == (255, 255, 255)
    assert list(inspect.signature(projection.ProjectionBatch.deskew_device).parameters)[1:] == [
        "d_scans", "scan_stride", "step_bytes", "n", "interp", "border", "d_out", "out_stride", "out_step"]
    assert callable(projection.ProjectionBatch.deskew_canvas)
    a = np.zeros((6, 5, 2), np.uint8)
    with pytest.raises(_lib.OmrError) as e:
        projection.get_angles_and_deskew([a, a], 45, 0.2, 0.5)
    assert e.value.code == -215
    with pytest.raises(_lib.OmrError) as e:
        projection.get_angles_and_deskew([], 45, 0.2, 0.5)
    assert e.value.code == -5
    with pytest.raises(_lib.OmrError) as e:
        projection.get_angles_and_deskew([np.zeros((6, 5, 3), np.uint8)], 45, 0.2, 0.5, interp=2)
    assert e.value.code == -213


def test_shim_has_deskew_with_projections():
    src = open(os.path.join(ROOT, "shim", "oics", "src", "projection.rs")).read()
    m = re.search(r"pub fn deskew_with_projections\((.*?)\)\s*->\s*opencv::Result<Vec<\(f64, Mat\)>>(.*?)\n\}\n", src, re.S)
    assert m, "projection::deskew_with_projections"
    params = " ".join(m.group(1).split())
    assert "&[&TransformableMatrix]" in params and "u16" in params and params.count("f64") == 2 and "Scalar" in params
    assert "ffi::omr_deskew_with_projections_batch(" in m.group(2) and "into_mat" in m.group(2)
