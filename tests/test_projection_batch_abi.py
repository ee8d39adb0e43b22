"""omr_projection_batch_* / omr_get_angles_with_projections_batch without a GPU: the seven symbols with the header's
signatures (header, ctypes table, ffi.rs), omr_projection_batch_working_size against the shape of oracle.scale_self
and resize()'s dispatch over a grid of shapes and scales, every argument error -- each returned before any device
work (the pointers handed in are host pointers, and on a machine without a GPU a call that reached the device would be
-217) -- and the Python and Rust front doors."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest

from oics import _lib, projection
from oics._lib import OmrImage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

NONE, AREA_INT, AREA_GENERAL, LINEAR = 0, 1, 2, 3
WANT = {
    "omr_projection_batch_working_size": ("int", ["int32_t", "int32_t", "double", "int32_t*", "int32_t*", "int32_t*"]),
    "omr_projection_batch_create": ("int", ["int32_t", "int32_t", "int32_t", "uint16_t", "double", "double", "int32_t", "int32_t",
                                            "omr_projection_batch**"]),
    "omr_projection_batch_destroy": ("void", ["omr_projection_batch*"]),
    "omr_projection_batch_info": ("int", ["omr_projection_batch*", "int32_t*", "int32_t*", "int32_t*", "int32_t*"]),
    "omr_projection_batch_front_device": ("int", ["omr_projection_batch*", "constuint8_t*", "int64_t", "int64_t", "int32_t",
                                                  "uint8_t*", "int64_t", "int64_t"]),
    "omr_projection_batch_run_device": ("int", ["omr_projection_batch*", "constuint8_t*", "int64_t", "int64_t", "int32_t",
                                                "double*", "int32_t*", "double*", "double*"]),
    "omr_get_angles_with_projections_batch": ("int", ["constomr_image*", "int32_t", "uint16_t", "double", "double", "double*",
                                                      "int32_t*"]),
}


def test_symbols_exist_with_the_headers_signatures():
    import gen_shim_ffi as g
    decls = {name: (ret, [t.replace(" ", "") for t, _ in params]) for name, ret, params in g.parse_header()}
    L = _lib.lib()
    ffi = open(os.path.join(ROOT, "shim", "oics", "src", "ffi.rs")).read()
    for name, (ret, args) in WANT.items():
        assert name in decls, name
        assert decls[name][0].strip() == ret
        assert decls[name][1] == args, (name, decls[name][1])
        assert hasattr(L, name)  # exported by the built library
        res, argtypes = _lib.SYMBOLS[name]
        assert (res is C.c_int) == (ret == "int") and len(argtypes) == len(args)
        m = re.search(r"pub fn %s\((.*?)\)" % name, ffi)
        assert m and len(m.group(1).split(",")) == len(args), name
    header = open(os.path.join(ROOT, "include", "omrdeskew.h")).read()
    for k, v in (("NONE", NONE), ("AREA_INT", AREA_INT), ("AREA_GENERAL", AREA_GENERAL), ("LINEAR", LINEAR)):
        assert re.search(r"#define OMR_PROJECTION_FRONT_%s %d\b" % (k, v), header), k
        assert getattr(_lib, "OMR_PROJECTION_FRONT_" + k) == v


def _ws(rows, cols, scale):
    r, c, m = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    rc = _lib.lib().omr_projection_batch_working_size(rows, cols, scale, C.byref(r), C.byref(c), C.byref(m))
    return rc, r.value, c.value, m.value


def _dispatch(rows, cols, dr, dc, scale):
    """OpenCV 4.6.0 resize() for scale_self's flags (INTER_LINEAR above 1, INTER_AREA otherwise)"""
    if scale == 1.0 or (dr, dc) == (rows, cols):
        return NONE
    if scale > 1.0:
        return LINEAR
    sx, sy = 1.0 / (dc / cols), 1.0 / (dr / rows)
    eps = sys.float_info.epsilon
    fast = abs(sx - round(sx)) < eps and abs(sy - round(sy)) < eps
    return AREA_INT if fast else AREA_GENERAL


GRID = [(r, c, s)
        for (r, c) in [(3508, 2480), (1150, 1240), (452, 640), (64, 128), (453, 641), (101, 77), (7, 2000), (2, 2), (1, 9)]
        for s in (0.2, 0.5, 0.37, 0.25, 0.999, 1.0, 1.5, 2.0, 3.7)]


def test_working_size_is_scale_selfs_shape_and_resizes_dispatch(oracle):
    seen = set()
    for rows, cols, scale in GRID:
        rc, wr, wc, mode = _ws(rows, cols, scale)
        if int(rows * scale) < 1 or int(cols * scale) < 1:
            assert rc == -215, (rows, cols, scale)  # a 1-pixel axis below 1: resize to an empty size
            continue
        assert rc == 0, (rows, cols, scale)
        exp = oracle.scale_self(np.zeros((rows, cols, 3), np.uint8), scale).shape
        assert (wr, wc) == exp[:2], (rows, cols, scale)
        assert mode == _dispatch(rows, cols, wr, wc, scale), (rows, cols, scale)
        assert projection.projection_batch_working_size(rows, cols, scale) == (wr, wc, mode)
        seen.add(mode)
    assert seen == {NONE, AREA_INT, AREA_GENERAL, LINEAR}
    # the issue's named rows
    assert _ws(3508, 2480, 0.2) == (0, 701, 496, AREA_GENERAL)  # 3508 / 701 is not an integer
    assert _ws(1150, 1240, 0.2) == (0, 230, 248, AREA_INT)
    assert _ws(452, 640, 0.5) == (0, 226, 320, AREA_INT)
    assert _ws(453, 641, 0.5) == (0, 226, 320, AREA_GENERAL)
    assert _ws(453, 641, 1.0) == (0, 453, 641, NONE)
    assert _ws(453, 641, 1.5) == (0, 679, 961, LINEAR)
    assert _ws(1, 9, 0.5)[0] == -215 and _ws(9, 1, 0.9)[0] == -215


def _resize_rule(srows, scols, drows, dcols, linear):
    """OpenCV 4.6.0 resize.cpp, the order of its tests kept: (path, kx, ky) for INTER_LINEAR or INTER_AREA"""
    if (drows, dcols) == (srows, scols):
        return "COPY", 0, 0
    sx, sy = 1.0 / (dcols / scols), 1.0 / (drows / srows)
    kx, ky = round(sx), round(sy)  # both round half to even, as lrint
    eps = sys.float_info.epsilon
    fast = abs(sx - kx) < eps and abs(sy - ky) < eps
    if linear and fast and kx == 2 and ky == 2:
        linear = False  # an exact 2x shrink is INTER_AREA
    if linear or not (sx >= 1 and sy >= 1):
        return "LINEAR", 0, 0
    return ("AREA_INT", kx, ky) if fast else ("AREA_GENERAL", 0, 0)


@pytest.mark.parametrize("rows,cols,scale,path,k", [
    (453, 641, 1.0, "COPY", 0),        # identity: no scale_self at all
    (3, 4, 1.2, "COPY", 0),            # 3.6 x 4.8 truncates to the same 3 x 4
    (452, 640, 0.5, "AREA_INT", 2),    # integer 2x shrink
    (40, 50, 0.3, "AREA_GENERAL", 0),  # 12 x 15: 3.33.. on both axes
    (40, 50, 1.5, "LINEAR", 0),
    (6, 10, 0.499, "AREA_GENERAL", 0),  # 2 x 4: exactly 3 down, 2.5 across -- one integer axis is not enough
])
def test_every_branch_of_the_resize_dispatch(rows, cols, scale, path, k):
    """one case per branch of the rule that resize_ptr, the correct batch and the projection batch share"""
    dr, dc = (rows, cols) if scale == 1.0 else (int(rows * scale), int(cols * scale))  # transfer.rs:70-71 `as i32`
    got = _resize_rule(rows, cols, dr, dc, linear=scale > 1.0)
    assert got == (path, k, k)  # the case is the branch its comment says
    mode = {"COPY": NONE, "AREA_INT": AREA_INT, "AREA_GENERAL": AREA_GENERAL, "LINEAR": LINEAR}[path]
    assert _ws(rows, cols, scale) == (0, dr, dc, mode)


def test_integer_area_factors_divide_the_source_exactly():
    """The integer INTER_AREA kernels carry no partial-block arithmetic and launch_resize refuses d * k != s.  That is
    sound only if resize()'s test for integer factors, |1 / (d / s) - lrint(.)| < DBL_EPSILON, passes for exact
    multiples alone at every size an entry point admits (check_image_shape: <= 32766).  Every source size up to
    2048, the A4 sides and the largest size, against every d below it (the test is per axis, so squares cover it)."""
    fast = 0
    for s in list(range(1, 2049)) + [2480, 3508, 32766]:
        for d in range(1, s):
            path, kx, ky = _resize_rule(s, s, d, d, linear=False)
            if path == "AREA_INT":
                assert kx == ky == s // d and d * kx == s, (s, d, kx)
                fast += 1
    assert fast > 2048  # integer factors were met
    assert _resize_rule(49, 49, 1, 1, linear=False)[0] == "AREA_GENERAL"  # the converse is false, as in OpenCV


def test_working_size_argument_errors():
    L = _lib.lib()
    r, c, m = C.c_int32(), C.c_int32(), C.c_int32()
    assert L.omr_projection_batch_working_size(10, 10, 0.5, None, C.byref(c), C.byref(m)) == -5
    assert L.omr_projection_batch_working_size(10, 10, 0.5, C.byref(r), None, C.byref(m)) == -5
    assert L.omr_projection_batch_working_size(10, 10, 0.5, C.byref(r), C.byref(c), None) == -5
    for bad in (0.0, -0.5, float("nan"), float("inf"), -float("inf")):
        assert _ws(10, 10, bad)[0] == -5, bad
    assert _ws(0, 10, 0.5)[0] == -215 and _ws(10, 0, 0.5)[0] == -215 and _ws(32767, 10, 0.5)[0] == -215
    assert _ws(30000, 30000, 1.5)[0] == -215  # the working image would leave the 16-bit coordinate range


def _create(rows=100, cols=80, cn=3, max_angle=45, step=0.2, scale=0.2, device=0, max_scans=4, out=True):
    h = C.c_void_p()
    rc = _lib.lib().omr_projection_batch_create(rows, cols, cn, max_angle, step, scale, device, max_scans,
                                                C.byref(h) if out else None)
    if rc == 0:
        _lib.lib().omr_projection_batch_destroy(h)
    return rc


def test_create_argument_errors_before_any_device_work():
    assert _create(out=False) == -5
    assert _create(cn=4) == -213
    assert _create(cn=2) == -215 and _create(cn=0) == -215 and _create(cn=5) == -215
    assert _create(rows=0) == -215 and _create(cols=32767) == -215
    assert _create(rows=4, scale=0.2) == -215  # 4 * 0.2 truncates to 0
    assert _create(max_angle=0) == -5 and _create(step=100.0) == -5  # empty candidate range
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert _create(scale=bad) == -5, bad
    assert _create(max_scans=0) == -5 and _create(max_scans=65536) == -5
    assert _create(device=-1) == -5
    if _lib.lib().omr_device_count() == 0:
        assert _create() == -217  # the valid call is the only one that reaches the device


HOST = np.zeros(64, np.uint8)  # a host buffer: nothing below may touch it


def test_run_and_front_refuse_a_null_context_before_any_device_work():
    L = _lib.lib()
    ang, idx = np.zeros(2), np.zeros(2, np.int32)
    p = C.c_void_p(HOST.ctypes.data)
    assert L.omr_projection_batch_run_device(None, p, 0, 64, 1, ang.ctypes.data_as(_lib.f64p), idx.ctypes.data_as(_lib.i32p),
                                             None, None) == -5
    assert L.omr_projection_batch_front_device(None, p, 0, 64, 1, p, 64, 64) == -5
    assert L.omr_projection_batch_info(None, None, None, None, None) == -5
    L.omr_projection_batch_destroy(None)  # a no-op


def _host(n=3, srcs=True, angles=True, max_angle=45, step=0.2, scale=0.5, bad=None):
    a = np.full((12, 10, 3), 255, np.uint8)
    ims = (OmrImage * 3)(OmrImage(a.ctypes.data, 12, 10, 3, 30), OmrImage(a.ctypes.data, 6, 10, 3, 30),
                         OmrImage(a.ctypes.data, 12, 10, 3, 30))
    if bad:
        for k, v in bad.items():
            setattr(ims[1], k, v)
    ang = np.full(3, 7.0)
    idx = np.full(3, -9, np.int32)
    rc = _lib.lib().omr_get_angles_with_projections_batch(ims if srcs else None, n, max_angle, step, scale,
                                                          ang.ctypes.data_as(_lib.f64p) if angles else None,
                                                          idx.ctypes.data_as(_lib.i32p))
    assert (ang == 7.0).all() and (idx == -9).all()  # no call below may leave a partial result
    return rc


def test_host_form_argument_errors_before_any_device_work():
    assert _host(srcs=False) == -5 and _host(angles=False) == -5
    assert _host(n=0) == -5 and _host(n=-2) == -5
    assert _host(max_angle=0) == -5
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert _host(scale=bad) == -5, bad
    # an invalid image in the middle fails the whole call, with omr_get_angle_with_projections' code
    assert _host(bad={"data": None}) == -5
    assert _host(bad={"step_bytes": 29}) == -5
    assert _host(bad={"rows": 0}) == -215 and _host(bad={"cols": 32767}) == -215
    assert _host(bad={"channels": 2}) == -215 and _host(bad={"channels": 5}) == -215 and _host(bad={"channels": 0}) == -215
    assert _host(bad={"rows": 1}) == -215  # 1 * 0.5 truncates to 0
    if _lib.lib().omr_device_count() == 0:
        assert _host() == -217 and _host(bad={"channels": 4, "step_bytes": 40}) == -217


def test_python_front_doors():
    sig = inspect.signature(projection.get_angles_with_projections)
    assert list(sig.parameters)[:4] == ["srcs", "max_angle", "step", "resize_scale"]
    assert list(inspect.signature(projection.ProjectionBatch.__init__).parameters)[1:8] == [
        "rows", "cols", "channels", "max_angle", "step", "resize_scale", "max_scans"]
    for name in ("info", "front_device", "run_device", "close"):
        assert callable(getattr(projection.ProjectionBatch, name))
    a = np.zeros((6, 5, 2), np.uint8)
    with pytest.raises(_lib.OmrError) as e:
        projection.get_angles_with_projections([a, a], 45, 0.2, 0.5)
    assert e.value.code == -215
    with pytest.raises(_lib.OmrError) as e:
        projection.get_angles_with_projections([], 45, 0.2, 0.5)
    assert e.value.code == -5
    with pytest.raises(_lib.OmrError) as e:
        projection.ProjectionBatch(10, 10, 4, 45, 0.2, 0.5, 2)
    assert e.value.code == -213


def test_shim_has_get_angles_with_projections():
    src = open(os.path.join(ROOT, "shim", "oics", "src", "projection.rs")).read()
    m = re.search(r"pub fn get_angles_with_projections\((.*?)\)\s*->\s*Vec<f64>(.*?)\n\}\n", src, re.S)
    assert m, "projection::get_angles_with_projections"
    params = " ".join(m.group(1).split())
    assert "&[&TransformableMatrix]" in params and "u16" in params and params.count("f64") == 2
    assert "ffi::omr_get_angles_with_projections_batch(" in m.group(2)
