"""The Hough and FFT deskew flows and the batch gray conversion without a GPU: every argument rule of
omr_rgb_to_gray_batch_device, omr_hough_deskew_batch_device / omr_fft_deskew_batch_device, omr_deskew_with_hough_batch /
omr_deskew_with_fft_batch and their _streams forms is answered before any device work (the device pointers handed in are
invented: a call that reached a device would fault on them, and on a machine without one it answers -217) and leaves the
caller's arrays as they were; the forms with NULL outputs are accepted; omr_detector_deskew_canvas holds every canvas
omr_rotate_size gives over a fine grid of angles, and no more than it must."""
import ctypes as C
import io
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import png_ref as P  # noqa: E402
import oics  # noqa: E402
from oics import _lib, fft, hough, transfer  # noqa: E402
from oics._lib import OmrImage, OmrImageOwned  # noqa: E402

L = oics.lib()
NO_GPU = L.omr_device_count() < 1
i64p = C.POINTER(C.c_int64)
HOUGH = (40.0, 5.0)
FFT = (30.0, 90.0, 40.0, 5.0)
DETECTORS = [("hough", HOUGH), ("fft", FFT)]


def _err():
    return L.omr_last_error().decode()


# ---- the batch gray conversion ---------------------------------------------------------------------------------------
def _gray(src=0x10000, n=2, sstride=400, sstep=36, rows=8, cols=10, cn=3, dst=0x90000, dstride=128, dstep=12):
    return L.omr_rgb_to_gray_batch_device(C.c_void_p(src) if src else None, n, sstride, sstep, rows, cols, cn,
                                          C.c_void_p(dst) if dst else None, dstride, dstep, None)


def test_gray_batch_argument_rules_come_before_any_device_work():
    assert _gray(src=0) == -5 and _gray(dst=0) == -5 and "null" in _err()
    assert _gray(n=0) == -5 and _gray(n=-2) == -5
    for bad in (dict(rows=0), dict(cols=0), dict(rows=-1), dict(cols=-3)):
        assert _gray(**bad) == -215 and "empty image" in _err(), bad
    assert _gray(rows=32767, sstride=1 << 30, dstride=1 << 30) == -215
    for cn in (0, 1, 2, 5, -1):
        assert _gray(cn=cn, sstep=64, sstride=1024) == -215 and "3 or 4 channels" in _err(), cn
    assert _gray(sstep=29) == -5 and _gray(cn=4, sstep=39) == -5 and "step too small" in _err()
    assert _gray(dstep=9) == -5 and "step too small" in _err()
    assert _gray(sstride=8 * 36 - 1) == -5 and "stride" in _err()
    assert _gray(dstride=8 * 12 - 1) == -5 and "stride" in _err()
    assert _gray(sstride=-400) == -5 and _gray(sstride=0) == -5
    # overlapping ranges: the same buffer, the destination inside the source, the source's last byte
    assert _gray(dst=0x10000) == -5 and "overlap" in _err()
    assert _gray(dst=0x10000 + 500) == -5
    last = 0x10000 + 400 + 7 * 36 + 30 - 1
    assert _gray(dst=last) == -5 and _gray(src=0x90000 + 128 + 7 * 12 + 10 - 1) == -5
    if NO_GPU:  # the accepted calls are the only ones that get as far as asking for a device
        assert {_gray(), _gray(cn=4, sstep=40), _gray(dst=last + 1), _gray(sstep=31, sstride=8 * 31, dstep=10, dstride=80)} == {-217}
    with pytest.raises(_lib.OmrError) as e:
        transfer.rgb_to_gray_batch(0x10000, 2, 400, 36, 8, 10, 2, 0x90000, 128, 12)
    assert e.value.code == -215


# ---- the device flows ------------------------------------------------------------------------------------------------
def _dev(which, scans=0x100000, n=2, stride=4096, rows=30, cols=40, cn=3, step=120, flags=1, border_mode=0, border=True, clip=1,
         out=0x900000, ostride=None, ostep=None, size=True, angles=True, rc=True, n_lines=True):
    mr, mc = C.c_int32(), C.c_int32()
    slot = (50, 50) if L.omr_detector_deskew_canvas(rows, cols, clip, C.byref(mr), C.byref(mc)) else (mr.value, mc.value)
    ostep = slot[1] * max(cn, 1) if ostep is None else ostep
    ostride = slot[0] * ostep if ostride is None else ostride
    ang, codes, nl, sz = np.full(4, 7.0), np.full(4, -9, np.int32), np.full(4, -9, np.int32), np.full(8, -9, np.int32)
    bv = (C.c_uint8 * 4)(255, 255, 255, 0)
    fn = L.omr_hough_deskew_batch_device if which == "hough" else L.omr_fft_deskew_batch_device
    code = fn(C.c_void_p(scans) if scans else None, n, stride, rows, cols, cn, step, *(HOUGH if which == "hough" else FFT), flags,
              border_mode, bv if border else None, clip, C.c_void_p(out) if out else None, ostride, ostep,
              sz.ctypes.data_as(_lib.i32p) if size else None, ang.ctypes.data_as(_lib.f64p) if angles else None,
              codes.ctypes.data_as(_lib.i32p) if rc else None, nl.ctypes.data_as(_lib.i32p) if n_lines else None, None)
    assert (ang == 7.0).all() and (codes == -9).all() and (nl == -9).all() and (sz == -9).all()  # a refused call writes nothing
    return code


@pytest.mark.parametrize("which", ["hough", "fft"])
def test_device_flow_argument_rules_come_before_any_device_work(which):
    for null in ("scans", "out"):
        assert _dev(which, **{null: 0}) == -5 and "null pointer" in _err(), null
    for null in ("border", "size", "angles"):
        assert _dev(which, **{null: False}) == -5 and "null pointer" in _err(), null
    assert _dev(which, n=0) == -5 and _dev(which, n=-1) == -5 and "empty batch" in _err()
    for bad in (dict(rows=0), dict(cols=0), dict(rows=-2)):
        assert _dev(which, **bad) == -215 and "empty image" in _err(), bad
    assert _dev(which, rows=32767) == -215
    assert _dev(which, cn=4, step=160) == -213
    for cn in (0, 2, 5):
        assert _dev(which, cn=cn, step=400) == -215, cn
    assert _dev(which, step=119) == -5 and "step_bytes too small" in _err()
    assert _dev(which, cn=1, step=39) == -5
    assert _dev(which, stride=-1) == -5 and "negative scan stride" in _err()
    # the rotate's own rules: flags, border mode, clip
    assert _dev(which, flags=32) == -5 and _dev(which, flags=5) == -213 and _dev(which, flags=7) == -213
    assert _dev(which, border_mode=6) == -5 and _dev(which, border_mode=-1) == -5
    assert _dev(which, clip=2) == -5 and "clip" in _err()
    # every slot holds the worst-case canvas: 51 x 51 for a 30 x 40 image (a 3-4-5 triangle: the diagonal is 50 exactly)
    assert _dev(which, ostep=51 * 3 - 1) == -5 and "omr_detector_deskew_canvas" in _err()
    assert _dev(which, ostride=51 * 153 - 1) == -5
    assert _dev(which, clip=0, ostep=119) == -5 and _dev(which, clip=0, ostride=30 * 120 - 1) == -5
    assert _dev(which, out=0x100000) == -5 and "overlap" in _err()
    assert _dev(which, out=0x100000 + 4096 + 29 * 120 + 119) == -5
    # a shape whose worst-case canvas leaves the image limit
    assert _dev(which, rows=30000, cols=30000, step=90000, stride=1 << 40) == -215
    # rc is the Hough detector's per-scan code; the FFT detector has none to give
    if which == "hough":
        assert _dev(which, rc=False) == -5 and "null pointer" in _err()
    if NO_GPU:
        accepted = {_dev(which), _dev(which, n_lines=False), _dev(which, cn=1, step=40), _dev(which, clip=0), _dev(which, stride=0),
                    _dev(which, flags=0, border_mode=1), _dev(which, out=0x100000 + 4096 + 29 * 120 + 120)}
        if which == "fft":
            accepted.add(_dev(which, rc=False))
        assert accepted == {-217}


# ---- host images -----------------------------------------------------------------------------------------------------
def _host(which, n=3, srcs=True, border=True, angles=True, rc=True, rotated=True, flags=1, border_mode=0, clip=1, bad=None):
    a = np.full((12, 10, 3), 255, np.uint8)
    ims = (OmrImage * 3)(OmrImage(a.ctypes.data, 12, 10, 3, 30), OmrImage(a.ctypes.data, 6, 30, 1, 30), OmrImage(a.ctypes.data, 12, 10, 3, 30))
    for k, v in (bad or {}).items():
        setattr(ims[1], k, v)
    ang, codes = np.full(3, 7.0), np.full(3, -9, np.int32)
    outs = (OmrImageOwned * 3)()
    bv = (C.c_uint8 * 4)(255, 255, 255, 0)
    fn = L.omr_deskew_with_hough_batch if which == "hough" else L.omr_deskew_with_fft_batch
    code = fn(ims if srcs else None, n, *(HOUGH if which == "hough" else FFT), flags, border_mode, bv if border else None, clip,
              ang.ctypes.data_as(_lib.f64p) if angles else None, codes.ctypes.data_as(_lib.i32p) if rc else None,
              outs if rotated else None)
    assert (ang == 7.0).all() and (codes == -9).all() and not any(o.data for o in outs)  # no call below may leave a partial result
    return code


@pytest.mark.parametrize("which", ["hough", "fft"])
def test_host_form_argument_rules_come_before_any_device_work(which):
    for null in ("srcs", "border", "angles", "rotated"):
        assert _host(which, **{null: False}) == -5 and "bad batch arguments" in _err(), null
    assert _host(which, n=0) == -5 and _host(which, n=-2) == -5
    assert _host(which, flags=64) == -5 and _host(which, flags=6) == -213 and _host(which, border_mode=9) == -5 and _host(which, clip=-1) == -5
    # an invalid image in the middle fails the whole call
    assert _host(which, bad={"data": None}) == -5 and "null image" in _err()
    assert _host(which, bad={"step_bytes": 29}) == -5 and "step_bytes too small" in _err()
    assert _host(which, bad={"rows": 0}) == -215 and _host(which, bad={"cols": 32767}) == -215
    assert _host(which, bad={"channels": 4, "cols": 7}) == -213
    for cn in (0, 2, 5):
        assert _host(which, bad={"channels": cn, "cols": 5}) == -215, cn
    if which == "hough":
        assert _host(which, rc=False) == -5
    if NO_GPU:
        assert {_host(which), _host(which, clip=0), _host(which, border_mode=5, flags=2)} == {-217}
        if which == "fft":
            assert _host(which, rc=False) == -217


# ---- file contents ---------------------------------------------------------------------------------------------------
def _jpeg(rows=16, cols=24, **kw):
    from PIL import Image
    img = np.random.default_rng(3).integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    b = io.BytesIO()
    Image.fromarray(img).save(b, format="JPEG", quality=90, **kw)
    return b.getvalue()


def _png(rows=16, cols=24, color_type=2, **kw):
    img = np.random.default_rng(4).integers(0, 256, (rows, cols, 3) if color_type == 2 else (rows, cols), dtype=np.uint8)
    zs = P.deflate(P.filter_rows(P.pack_rows(img, color_type, 8), 3 if color_type == 2 else 1, 0))
    return P.assemble(rows, cols, color_type, 8, zs, **kw)


def _streams(which, streams, *, n=None, channels=3, flags=1, border_mode=0, border=True, clip=1, fmt=0, level=100, null=(),
             null_stream=None, negative=None):
    """the raw call -> (rc, angles, scan_rc, stream pointers, lengths), the outputs pre-filled with marks"""
    bufs = [np.frombuffer(bytes(s), np.uint8) if len(s) else np.zeros(1, np.uint8) for s in streams]
    m = len(bufs)
    sp = (C.c_void_p * max(m, 1))(*[b.ctypes.data for b in bufs])
    if null_stream is not None:
        sp[null_stream] = None
    ln = np.array([len(s) for s in streams] + [0], np.int64)
    if negative is not None:
        ln[negative] = -1
    ang, src = np.full(max(m, 1), 7.5), np.full(max(m, 1), 77, np.int32)
    ptrs = (_lib.u8p * max(m, 1))()
    lens = np.full(max(m, 1), 123, np.int64)
    bv = (C.c_uint8 * 4)(255, 255, 255, 0)
    fn = L.omr_deskew_with_hough_batch_streams if which == "hough" else L.omr_deskew_with_fft_batch_streams
    rc = fn(None if "streams" in null else sp, None if "len" in null else ln.ctypes.data_as(i64p), m if n is None else n, channels,
            *(HOUGH if which == "hough" else FFT), flags, border_mode, bv if border else None, clip, fmt, level,
            None if "angles" in null else ang.ctypes.data_as(_lib.f64p), None if "scan_rc" in null else src.ctypes.data_as(_lib.i32p),
            None if "out" in null else ptrs, None if "out_len" in null else lens.ctypes.data_as(i64p))
    return rc, ang, src, ptrs, lens


def _untouched(r):
    _, ang, src, ptrs, lens = r
    return (ang == 7.5).all() and (src == 77).all() and not any(ptrs) and (lens == 123).all()


@pytest.mark.parametrize("which", ["hough", "fft"])
@pytest.mark.parametrize("fmt", [0, 1])
def test_streams_form_refusals_of_the_call_come_before_any_device_work(which, fmt):
    good = [_jpeg(), _png()]
    refusals = [
        (dict(null=("streams",)), -5), (dict(null=("len",)), -5), (dict(null=("angles",)), -5), (dict(null=("scan_rc",)), -5),
        (dict(null_stream=1), -5), (dict(n=0), -5), (dict(n=-3), -5), (dict(negative=0), -5),
        (dict(null=("out",)), -5), (dict(null=("out_len",)), -5),   # exactly one of the two
        (dict(border=False), -5),                                   # outputs wanted, no border
        (dict(channels=2), -5), (dict(channels=4), -5), (dict(channels=0), -5),
        (dict(flags=128), -5), (dict(flags=5), -213), (dict(border_mode=7), -5), (dict(clip=3), -5),
    ]
    for kw, code in refusals:
        r = _streams(which, good, fmt=fmt, **kw)
        assert r[0] == code, (kw, r[0], _err())
        assert _untouched(r), kw
    for bad_fmt in (2, -1):
        r = _streams(which, good, fmt=bad_fmt)
        assert r[0] == -5 and "format" in _err() and _untouched(r)
    # a shape whose worst-case canvas the encoder's 32-bit offsets cannot take: refused for the whole call from the headers
    if fmt == 1:
        huge = P.assemble(20000, 20000, 2, 8, P.deflate(bytes(64)))  # slot 28285 x 28285 x 3: IDAT above 2^31 - 1 bytes
    else:
        import struct
        j = _jpeg()
        at = j.index(b"\xff\xc0")
        huge = j[:at + 5] + struct.pack(">HH", 9000, 9000) + j[at + 9:]  # slot 12728 x 12728 x 3: 3.8 million blocks
    r = _streams(which, [good[0], huge], fmt=fmt)
    assert r[0] == -215 and _untouched(r), (r[0], _err())
    if NO_GPU:  # the angles-only form has no canvas: the same batch gets as far as asking for a device, as does a good one
        r = _streams(which, [good[0], huge], fmt=fmt, null=("out", "out_len"), border=False)
        assert r[0] == -217 and _untouched(r)
        r = _streams(which, good, fmt=fmt)
        assert r[0] == -217 and _untouched(r)


@pytest.mark.parametrize("which", ["hough", "fft"])
def test_a_batch_of_refused_streams_returns_their_codes_and_no_stream(which):
    streams = [_jpeg(progressive=True), _png(interlace=1), _jpeg()[:20], b"\x00\x01\x02\x03"]
    want = []
    for s in streams:
        b = np.frombuffer(s, np.uint8)
        info = L.omr_png_info if s[:8] == P.SIGNATURE else L.omr_jpeg_info
        want.append(info(b.ctypes.data, b.size, None, None, None, None))
    assert want == [-213, -213, -5, -5]  # what the existing decoder tests pin
    rc, ang, src, ptrs, lens = _streams(which, streams)
    assert rc == 0 and list(src[:4]) == want and (ang[:4] == 0.0).all() and not any(ptrs) and (lens[:4] == 0).all()
    rc, ang, src, ptrs, lens = _streams(which, streams, null=("out", "out_len"), border=False)   # the angles alone
    assert rc == 0 and list(src[:4]) == want and (ang[:4] == 0.0).all()
    # gray from an RGB PNG is refused for that sheet alone
    rc, ang, src, ptrs, lens = _streams(which, [_png(), _png()], channels=1)
    assert rc == 0 and list(src[:2]) == [-213, -213] and not any(ptrs)


# ---- the canvas ------------------------------------------------------------------------------------------------------
def _rotate_size(rows, cols, angle, clip):
    r, c = C.c_int32(), C.c_int32()
    assert L.omr_rotate_size(rows, cols, float(angle), clip, C.byref(r), C.byref(c)) == 0
    return r.value, c.value


@pytest.mark.parametrize("rows,cols", [(150, 199), (120, 90), (1, 1), (1, 700), (3508, 2480), (30, 40), (300, 400), (5, 12)])
def test_canvas_is_rotate_sizes_maximum_over_the_angles(rows, cols):
    """omr_rotate_size over 0.01-degree steps of the whole circle, and at the two angles where a side peaks.  The slot must
    hold every canvas.  It is the least such slot, ceil(diagonal), whenever the grid reaches that size -- which a 0.01-degree
    grid does unless the diagonal lies within 4e-9 of a whole number from above (the peak is flat: cos(0.005 deg) = 1 - 3.8e-9);
    where the diagonal IS a whole number (3-4-5 shapes) rounding can lift a computed side above it and the slot is one more."""
    mr, mc = transfer.detector_deskew_canvas(rows, cols)
    peak = math.degrees(math.atan2(rows, cols))
    angles = np.concatenate([np.arange(0, 36000) * 0.01, [peak, 90.0 - peak, -peak, peak - 90.0, 180.0 - peak]])
    sizes = np.array([_rotate_size(rows, cols, a, 1) for a in angles])
    top_r, top_c = int(sizes[:, 0].max()), int(sizes[:, 1].max())
    assert mr >= top_r and mc >= top_c
    diag = math.hypot(rows, cols)
    if diag == int(diag):
        assert mr == mc == int(diag) + 1 and top_r >= int(diag) and top_c >= int(diag)
    else:
        assert mr == mc == math.ceil(diag) == top_r == top_c
    assert transfer.detector_deskew_canvas(rows, cols, 0) == (rows, cols)  # DEFAULT keeps the size


def test_canvas_argument_rules():
    r, c = C.c_int32(-9), C.c_int32(-9)
    assert L.omr_detector_deskew_canvas(10, 10, 1, None, C.byref(c)) == -5 and L.omr_detector_deskew_canvas(10, 10, 1, C.byref(r), None) == -5
    assert L.omr_detector_deskew_canvas(0, 10, 1, C.byref(r), C.byref(c)) == -215
    assert L.omr_detector_deskew_canvas(10, 32767, 0, C.byref(r), C.byref(c)) == -215
    assert L.omr_detector_deskew_canvas(10, 10, 2, C.byref(r), C.byref(c)) == -5
    assert L.omr_detector_deskew_canvas(23170, 23170, 1, C.byref(r), C.byref(c)) == -215   # diagonal 32767.3
    assert (r.value, c.value) == (-9, -9)
    assert L.omr_detector_deskew_canvas(23169, 23169, 1, C.byref(r), C.byref(c)) == 0 and r.value == c.value == 32766


def test_python_and_rust_front_doors():
    import inspect
    assert list(inspect.signature(hough.deskew).parameters)[:3] == ["srcs", "min_line_length", "max_line_gap"]
    assert list(inspect.signature(fft.deskew_streams).parameters)[:5] == ["streams", "canny_threshold_1", "canny_threshold_2",
                                                                          "min_line_length", "max_line_gap"]
    for mod, args in ((hough, HOUGH), (fft, FFT)):
        with pytest.raises(_lib.OmrError) as e:
            mod.deskew([np.zeros((6, 5), np.uint8), np.zeros((6, 5, 2), np.uint8)], *args)
        assert e.value.code == -215
        ang, rc, out = mod.deskew_streams([_jpeg(progressive=True), b"\x00\x01"], *args)
        assert list(rc) == [-213, -5] and out == [None, None] and (ang == 0.0).all()
        ang, rc, out = mod.deskew_streams([_jpeg(progressive=True)], *args, png=True, want_out=False)
        assert list(rc) == [-213] and out is None
    root = os.path.dirname(HERE)
    for name, fns in (("transfer.rs", {"rgb_images_to_gray": "omr_rgb_to_gray_batch_device"}),
                      ("hough.rs", {"deskew_with_hough": "omr_deskew_with_hough_batch", "deskew_files_with_hough": "omr_deskew_with_hough_batch_streams"}),
                      ("fft.rs", {"deskew_with_fft": "omr_deskew_with_fft_batch", "deskew_files_with_fft": "omr_deskew_with_fft_batch_streams"})):
        rs = open(os.path.join(root, "shim", "oics", "src", name)).read()
        for fn, symbol in fns.items():
            body = rs.split("fn %s(" % fn)[1].split("\n}\n")[0]
            assert "ffi::%s(" % symbol in body and "imgcodecs" not in body, fn
