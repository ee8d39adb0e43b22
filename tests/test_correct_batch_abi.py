"""CPU-side checks of the correct_default batch (omr_correct_batch_* / omr_correct_default_batch): declared in
include/omrdeskew.h with the agreed parameter lists, exported by the library, bound by the ctypes table; the canvas
bound against omr_rotate_size; argument errors reported without a GPU."""
import ctypes as C
import os
import re
import sys

import numpy as np

import oics
from oics import _lib, omr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_shim_ffi  # noqa: E402

DECLS = {
    "omr_correct_batch_create": ("int", [
        ("int32_t", "rows"), ("int32_t", "cols"), ("int32_t", "channels"), ("uint16_t", "projection_max_angle"),
        ("double", "projection_angle_step"), ("int32_t", "projection_max_width"), ("int32_t", "projection_max_height"),
        ("double", "hough_min_line_length"), ("double", "hough_max_line_gap"), ("int32_t", "device"),
        ("int32_t", "max_scans"), ("omr_correct_batch * *", "out")]),
    "omr_correct_batch_destroy": ("void", [("omr_correct_batch *", "cb")]),
    "omr_correct_batch_canvas": ("int", [("int32_t", "rows"), ("int32_t", "cols"), ("int32_t *", "max_rows"),
                                         ("int32_t *", "max_cols")]),
    "omr_correct_batch_run_device": ("int", [
        ("omr_correct_batch *", "cb"), ("const uint8_t *", "d_scans"), ("int64_t", "scan_stride_bytes"),
        ("int64_t", "step_bytes"), ("int32_t", "n"), ("double *", "rotate_angle"), ("int32_t *", "need_check"),
        ("int32_t *", "scan_rc"), ("uint8_t *", "d_out"), ("int64_t", "out_stride_bytes"), ("int64_t", "out_step_bytes"),
        ("int32_t *", "out_size")]),
    "omr_correct_batch_info": ("int", [
        ("omr_correct_batch *", "cb"), ("int32_t *", "proj_rows"), ("int32_t *", "proj_cols"), ("int32_t *", "front_mode"),
        ("int32_t *", "kx"), ("int32_t *", "ky")]),
    "omr_correct_batch_front_device": ("int", [
        ("omr_correct_batch *", "cb"), ("const uint8_t *", "d_scans"), ("int64_t", "scan_stride_bytes"),
        ("int64_t", "step_bytes"), ("int32_t", "n"), ("uint8_t *", "d_small"), ("int64_t", "small_stride_bytes"),
        ("int64_t", "small_step_bytes")]),
    "omr_correct_default_batch": ("int", [
        ("const omr_image *", "srcs"), ("int32_t", "n"), ("uint16_t", "projection_max_angle"),
        ("double", "projection_angle_step"), ("int32_t", "projection_max_width"), ("int32_t", "projection_max_height"),
        ("double", "hough_min_line_length"), ("double", "hough_max_line_gap"), ("double *", "rotate_angle"),
        ("int32_t *", "need_check"), ("int32_t *", "scan_rc"), ("omr_image_owned *", "rotated")]),
}
PARAMS = (45, 0.2, 248, 230, 150.0, 50.0)


def _norm(params):
    return [(" ".join(t.replace("*", " * ").split()), n) for t, n in params]


def test_header_declares_the_correct_batch_entry_points():
    d = {name: (ret, params) for name, ret, params in gen_shim_ffi.parse_header()}
    for name, (ret, args) in DECLS.items():
        assert name in d, name
        assert d[name][0] == ret, (name, d[name][0])
        assert _norm(d[name][1]) == _norm(args), (name, d[name][1])


def test_library_exports_and_ctypes_binds_them():
    L = C.CDLL(_lib.LIB_PATH)
    for name, (_, args) in DECLS.items():
        assert hasattr(L, name), name
        assert name in _lib.SYMBOLS, name
        assert len(_lib.SYMBOLS[name][1]) == len(args), name


def _grid_max(rows, cols):
    L = oics.lib()
    r, c = C.c_int32(), C.c_int32()
    R = Cc = 0
    for k in range(-8999, 9001):  # (-90, 90] in 0.01 degree steps
        assert L.omr_rotate_size(rows, cols, k * 0.01, 1, C.byref(r), C.byref(c)) == 0
        R, Cc = max(R, r.value), max(Cc, c.value)
    return R, Cc


def test_canvas_bounds_every_contain_size():
    for rows, cols in ((1150, 1240), (1754, 1240), (300, 400), (64, 1000), (1, 1), (37, 53)):
        R, Cc = omr.correct_batch_canvas(rows, cols)
        gr, gc = _grid_max(rows, cols)
        assert R >= gr and Cc >= gc, (rows, cols, R, Cc, gr, gc)
        assert R <= gr + 1, (rows, cols, R, gr)
        assert Cc % 4 == 0 and Cc <= ((gc + 1 + 3) & ~3), (rows, cols, Cc, gc)


def test_canvas_bad_arguments():
    L = oics.lib()
    r, c = C.c_int32(), C.c_int32()
    assert L.omr_correct_batch_canvas(0, 10, C.byref(r), C.byref(c)) == -5
    assert L.omr_correct_batch_canvas(10, -1, C.byref(r), C.byref(c)) == -5
    assert L.omr_correct_batch_canvas(10, 10, None, C.byref(c)) == -5


def _create(rows=1150, cols=1240, cn=3, max_scans=16, max_angle=45, device=0, out=True):
    L = oics.lib()
    h = C.c_void_p()
    _, st, mw, mh, ml, mg = PARAMS
    rc = L.omr_correct_batch_create(rows, cols, cn, max_angle, st, mw, mh, ml, mg, device, max_scans, C.byref(h) if out else None)
    if rc == 0:
        L.omr_correct_batch_destroy(h)
    return rc


def test_create_rejects_bad_arguments_without_a_gpu():
    assert _create(out=False) == -5
    assert _create(max_scans=0) == -5
    assert _create(max_scans=-3) == -5
    assert _create(device=-1) == -5
    assert _create(max_angle=0) == -5  # empty candidate range
    assert _create(rows=0) == -215
    assert _create(cn=2) == -215   # as omr_correct_default: RGB2GRAY needs 3 or 4 channels
    assert _create(cn=4) == -213   # 4-channel batches are out of scope
    assert _create(cn=5) == -215


def test_run_device_rejects_a_null_context():
    L = oics.lib()
    n = 2
    ang = (C.c_double * n)()
    chk = (C.c_int32 * n)()
    rc = (C.c_int32 * n)()
    assert L.omr_correct_batch_run_device(None, C.c_void_p(256), 1150 * 1240 * 3, 1240 * 3, n, ang, chk, rc, None, 0, 0,
                                          None) == -5
    assert len(L.omr_last_error()) > 0


def test_inspection_entry_points_reject_a_null_context():
    L = oics.lib()
    v = [C.c_int32(7) for _ in range(5)]
    assert L.omr_correct_batch_info(None, *[C.byref(x) for x in v]) == -5
    assert [x.value for x in v] == [7] * 5
    assert L.omr_correct_batch_info(None, None, None, None, None, None) == -5
    assert L.omr_correct_batch_front_device(None, C.c_void_p(256), 1150 * 1240 * 3, 1240 * 3, 2, C.c_void_p(512), 230 * 248,
                                            248) == -5
    assert len(L.omr_last_error()) > 0


def test_front_mode_names_match_the_header():
    text = open(os.path.join(ROOT, "include", "omrdeskew.h")).read()
    for name in ("AREA_FUSED", "AREA_INT", "AREA_GENERAL", "LINEAR"):
        m = re.search(r"#define OMR_CORRECT_FRONT_%s (\d+)" % name, text)
        assert m and int(m.group(1)) == getattr(omr, "FRONT_" + name), name


def test_host_batch_rejects_bad_arguments_without_a_gpu():
    L = oics.lib()
    img = np.zeros((40, 30, 3), np.uint8)
    ims = (_lib.OmrImage * 2)(_lib.OmrImage(img.ctypes.data, 40, 30, 3, 90), _lib.OmrImage(img.ctypes.data, 40, 30, 3, 90))
    ang = (C.c_double * 2)()
    chk = (C.c_int32 * 2)()
    src = (C.c_int32 * 2)()
    ma, st, mw, mh, ml, mg = PARAMS

    def call(arr, n, a=ang, c=chk, s=src):
        return L.omr_correct_default_batch(arr, n, ma, st, mw, mh, ml, mg, a, c, s, None)

    assert call(None, 2) == -5
    assert call(ims, 0) == -5
    assert call(ims, -1) == -5
    assert call(ims, 2, a=None) == -5
    assert call(ims, 2, s=None) == -5
    bad = (_lib.OmrImage * 2)(ims[0], _lib.OmrImage(img.ctypes.data, 40, 30, 3, 89))  # step too small
    assert call(bad, 2) == -5
    nul = (_lib.OmrImage * 2)(ims[0], _lib.OmrImage(None, 40, 30, 3, 90))
    assert call(nul, 2) == -5
    two = (_lib.OmrImage * 2)(ims[0], _lib.OmrImage(img.ctypes.data, 40, 30, 2, 90))
    assert call(two, 2) == -215
    four = (_lib.OmrImage * 2)(ims[0], _lib.OmrImage(img.ctypes.data, 30, 30, 4, 120))
    assert call(four, 2) == -213
