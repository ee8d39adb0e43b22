"""omr_rotate_batch_canvas / omr_rotate_batch_device_ex / omr_rotate_batch_ex without a GPU: the three symbols with the
header's signatures, the canvas function against omr_rotate_size image by image, and every argument error -- each
returned before any device work (none of the pointers handed in is a device pointer, and on a machine without a GPU a
call that reached the device would be -217) -- plus the Python and Rust front doors."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from oics import _lib, transfer
from oics._lib import OmrImage, OmrImageOwned

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

ANGLES = [0.0, 0.05, -0.05, 10.0, -10.0, 45.0, -45.0, 90.0, 180.0]
NAMES = ("omr_rotate_batch_canvas", "omr_rotate_batch_device_ex", "omr_rotate_batch_ex")


def test_symbols_exist_with_the_headers_signatures():
    import gen_shim_ffi as g
    decls = {name: (ret, [t.replace(" ", "") for t, _ in params]) for name, ret, params in g.parse_header()}
    want = {
        "omr_rotate_batch_canvas": ["int32_t", "int32_t", "constdouble*", "int32_t", "int32_t", "int32_t*", "int32_t*",
                                    "int32_t*"],
        "omr_rotate_batch_device_ex": ["constuint8_t*", "int32_t", "int64_t", "int64_t", "int32_t", "int32_t", "int32_t",
                                       "constdouble*", "double", "int32_t", "int32_t", "constuint8_t*", "int32_t",
                                       "uint8_t*", "int64_t", "int64_t", "int32_t", "int32_t", "int32_t*", "void*"],
        "omr_rotate_batch_ex": ["constomr_image*", "int32_t", "constdouble*", "double", "int32_t", "int32_t",
                                "constuint8_t*", "int32_t", "omr_image_owned*"],
    }
    L = _lib.lib()
    for name in NAMES:
        assert name in decls, name
        assert decls[name][0].strip() == "int"
        assert decls[name][1] == want[name], (name, decls[name][1])
        assert hasattr(L, name)  # exported by the built library
        res, args = _lib.SYMBOLS[name]
        assert res is C.c_int and len(args) == len(want[name])


def _canvas(rows, cols, angles, clip, sizes=True):
    a = np.asarray(angles, np.float64)
    mr, mc = C.c_int32(-1), C.c_int32(-1)
    out = np.full(2 * len(a), -1, np.int32)
    rc = _lib.lib().omr_rotate_batch_canvas(rows, cols, a.ctypes.data_as(_lib.f64p), len(a), clip, C.byref(mr), C.byref(mc),
                                            out.ctypes.data_as(_lib.i32p) if sizes else None)
    return rc, mr.value, mc.value, out.reshape(-1, 2)


@pytest.mark.parametrize("clip", [0, 1])
@pytest.mark.parametrize("rows,cols", [(453, 311), (452, 312), (3508, 2480), (1, 1), (7, 2000)])
def test_canvas_is_rotate_size_per_image_and_the_independent_maxima(rows, cols, clip):
    rc, mr, mc, sizes = _canvas(rows, cols, ANGLES, clip)
    assert rc == 0
    exp = []
    for ang in ANGLES:
        dr, dc = C.c_int32(), C.c_int32()
        assert _lib.lib().omr_rotate_size(rows, cols, ang, clip, C.byref(dr), C.byref(dc)) == 0
        exp.append((dr.value, dc.value))
    assert sizes.tolist() == [list(e) for e in exp]
    assert mr == max(e[0] for e in exp) and mc == max(e[1] for e in exp)
    if clip == 0:
        assert (mr, mc) == (rows, cols)
    elif rows != cols:
        # the maxima are taken independently: of an upright and a lying canvas neither is the slot
        rc, r2, c2, s2 = _canvas(rows, cols, [0.0, 90.0], clip)
        assert rc == 0 and (r2, c2) == (s2[:, 0].max(), s2[:, 1].max()) and [r2, c2] not in s2.tolist()
    assert _canvas(rows, cols, ANGLES, clip, sizes=False)[:3] == (0, mr, mc)
    # the Python mirror
    pr, pc, ps = transfer.rotate_batch_canvas(rows, cols, ANGLES, clip)
    assert (pr, pc) == (mr, mc) and (ps == sizes).all()


def test_canvas_argument_errors():
    L = _lib.lib()
    a = np.array([1.0, 2.0])
    ap = a.ctypes.data_as(_lib.f64p)
    mr, mc = C.c_int32(), C.c_int32()
    assert L.omr_rotate_batch_canvas(10, 10, ap, 2, 1, C.byref(mr), C.byref(mc), None) == 0
    assert L.omr_rotate_batch_canvas(10, 10, None, 2, 1, C.byref(mr), C.byref(mc), None) == -5
    assert L.omr_rotate_batch_canvas(10, 10, ap, 0, 1, C.byref(mr), C.byref(mc), None) == -5
    assert L.omr_rotate_batch_canvas(10, 10, ap, -1, 1, C.byref(mr), C.byref(mc), None) == -5
    assert L.omr_rotate_batch_canvas(10, 10, ap, 2, 1, None, C.byref(mc), None) == -5
    assert L.omr_rotate_batch_canvas(10, 10, ap, 2, 1, C.byref(mr), None, None) == -5
    assert L.omr_rotate_batch_canvas(0, 10, ap, 2, 1, C.byref(mr), C.byref(mc), None) == -5
    assert L.omr_rotate_batch_canvas(10, 10, ap, 2, 2, C.byref(mr), C.byref(mc), None) == -5
    for bad in (np.nan, np.inf, -np.inf):
        assert _canvas(10, 10, [1.0, bad], 1)[0] == -5


SRC, DST = 1 << 20, 1 << 24  # never allocated, far enough apart for every call below


def _dev(src=SRC, n=3, sstride=None, sstep=None, rows=20, cols=30, cn=3, angles=(10.0, 0.0, -7.5), scale=1.0, flags=1,
         border_mode=0, border=True, clip=1, dst=DST, dstride=None, dstep=None, slot_rows=None, slot_cols=None, sizes=True):
    ang = None if angles is None else np.asarray(angles, np.float64)
    mr, mc = 0, 0
    if ang is not None and n > 0 and rows > 0 and cols > 0 and np.isfinite(ang).all() and clip in (0, 1):
        rc, mr, mc, _ = _canvas(rows, cols, ang, clip)
        if rc:  # a shape the library refuses: any slot will do
            mr, mc = rows, cols
    sr = mr if slot_rows is None else slot_rows
    sc = mc if slot_cols is None else slot_cols
    sstep = cols * cn if sstep is None else sstep
    dstep = sc * cn if dstep is None else dstep
    b = (C.c_uint8 * 4)(1, 2, 3, 4)
    out = np.zeros(2 * max(n, 1), np.int32)
    return _lib.lib().omr_rotate_batch_device_ex(
        C.c_void_p(src) if src else None, n, rows * sstep if sstride is None else sstride, sstep, rows, cols, cn,
        None if ang is None else ang.ctypes.data_as(_lib.f64p), scale, flags, border_mode,
        C.cast(b, _lib.u8p) if border else None, clip, C.c_void_p(dst) if dst else None,
        sr * dstep if dstride is None else dstride, dstep, sr, sc, out.ctypes.data_as(_lib.i32p) if sizes else None, None)


def _host(n=2, srcs=True, dsts=True, angles=(5.0, -3.0), border=True, **kw):
    a = np.zeros((12, 9, 3), np.uint8)
    ims = (OmrImage * 2)(OmrImage(a.ctypes.data, kw.pop("rows", 12), 9, kw.pop("cn", 3), kw.pop("step", 27)),
                         OmrImage(a.ctypes.data, 6, 9, 3, 27))
    outs = (OmrImageOwned * 2)()
    ang = None if angles is None else np.asarray(angles, np.float64)
    b = (C.c_uint8 * 4)(1, 2, 3, 4)
    return _lib.lib().omr_rotate_batch_ex(ims if srcs else None, n, None if ang is None else ang.ctypes.data_as(_lib.f64p),
                                          kw.pop("scale", 1.0), kw.pop("flags", 1), kw.pop("border_mode", 0),
                                          C.cast(b, _lib.u8p) if border else None, kw.pop("clip", 1), outs if dsts else None)


def test_argument_errors_before_any_device_work():
    # omr_rotate_device_ex's codes
    for call in (_dev, _host):
        for f in (5, 6, 7, 5 | 16, 7 | 8):
            assert call(flags=f) == -213, f
        for f in (32, 64, 1 | 128, -1, 1 << 20, 2 | 32):
            assert call(flags=f) == -5, f
        for bm in (-1, 6, 16, 16 | 1):
            assert call(border_mode=bm) == -5, bm
        assert call(border=False) == -5
        assert call(clip=2) == -5
        # the batch's own
        assert call(n=0) == -5 and call(n=-4) == -5
        assert call(angles=None) == -5
        for bad in (np.nan, np.inf, -np.inf):
            assert call(angles=(1.0, bad, 2.0)[:3 if call is _dev else 2]) == -5, bad
    assert _dev(src=0) == -5 and _dev(dst=0) == -5
    assert _dev(sstep=3 * 30 - 1) == -5
    assert _dev(cn=0) == -215 and _dev(cn=5) == -215 and _dev(rows=0) == -215 and _dev(cols=32767) == -215
    # a slot smaller than omr_rotate_batch_canvas's answer, in either direction
    rc, mr, mc, _ = _canvas(20, 30, (10.0, 0.0, -7.5), 1)
    assert _dev(slot_rows=mr - 1) == -5 and _dev(slot_cols=mc - 1) == -5
    assert _dev(clip=0, slot_rows=19) == -5 and _dev(clip=0, slot_cols=29) == -5
    # dst_step < channels * slot_cols, dst_stride_bytes < slot_rows * dst_step
    assert _dev(dstep=3 * mc - 1) == -5
    assert _dev(slot_cols=mc + 4, dstep=3 * (mc + 4) - 1) == -5
    assert _dev(dstride=mr * 3 * mc - 1) == -5
    assert _dev(dstride=0) == -5
    assert _dev(sstride=-1) == -5
    # overlapping ranges: the same block, the destination inside the sources, the sources inside the last slot
    assert _dev(dst=SRC) == -5
    assert _dev(dst=SRC + 2 * 20 * 90 + 19 * 90 + 89) == -5
    assert _dev(src=DST + 2 * mr * 3 * mc + (mr - 1) * 3 * mc + 3 * mc - 1) == -5
    assert _host(srcs=False) == -5 and _host(dsts=False) == -5
    assert _host(step=26) == -5
    assert _host(rows=0) == -215 and _host(cn=5) == -215


def test_valid_calls_reach_the_device():
    """the calls the errors above are variations of are themselves accepted: without a device they end in -217, the
    code of a call that got past its argument checks.  With a device they would touch addresses nobody allocated, so
    there the GPU suite makes the valid calls (tests/test_gpu_rotate_batch.py) and this one has nothing to add."""
    if _lib.lib().omr_device_count() > 0:
        return
    assert _dev() == -217
    assert _dev(sizes=False, sstride=0, slot_cols=64, dstep=200, dstride=1 << 16) == -217
    assert _host() == -217


def test_python_mirrors_refuse_what_the_library_refuses():
    a = np.zeros((6, 5), np.uint8)
    for f in (5, 6, 7):
        with pytest.raises(_lib.OmrError) as e:
            transfer.rotate_batch_ex([a, a], [3.0, 4.0], 1.0, f, transfer.BORDER_REPLICATE)
        assert e.value.code == -213
    with pytest.raises(_lib.OmrError) as e:
        transfer.rotate_batch_ex([a], [float("nan")], 1.0, 1)
    assert e.value.code == -5
    with pytest.raises(_lib.OmrError) as e:
        transfer.rotate_batch_ex([], [], 1.0, 1)
    assert e.value.code == -5
    with pytest.raises(ValueError):
        transfer.rotate_batch_ex([a, a], [1.0], 1.0, 1)
    with pytest.raises(_lib.OmrError) as e:
        transfer.rotate_batch_device_ex(SRC, 2, 30, 5, 6, 5, 1, [1.0, 2.0], 1.0, 1, 9, (0, 0, 0, 0), 0, DST, 30, 5, 6, 5)
    assert e.value.code == -5


def test_shim_binds_the_exports_and_has_rotate_mats():
    ffi = open(os.path.join(ROOT, "shim", "oics", "src", "ffi.rs")).read()
    for name in NAMES:
        assert re.search(r"pub fn %s\(" % name, ffi), name
    src = open(os.path.join(ROOT, "shim", "oics", "src", "transfer.rs")).read()
    m = re.search(r"pub fn rotate_mats\((.*?)\)\s*->\s*Result<Vec<TransformableMatrix>, opencv::Error>(.*?)\n\}\n", src, re.S)
    assert m, "transfer::rotate_mats"
    assert "&[TransformableMatrix]" in m.group(1) and "&[f64]" in m.group(1)
    assert "ffi::omr_rotate_batch_ex(" in m.group(2)
