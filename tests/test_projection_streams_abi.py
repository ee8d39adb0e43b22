"""CPU-side checks of omr_deskew_with_projections_batch_streams and its PNG twin: every refusal of the whole call comes
before any device work and leaves the outputs untouched; a batch of refused streams alone returns 0 with the decoders' own
codes and asks for no device; channels = 1 refuses an RGB PNG for that sheet alone."""
import ctypes as C
import io
import os
import struct
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import png_ref as P  # noqa: E402
import oics  # noqa: E402
from oics import _lib, projection  # noqa: E402

NO_GPU = oics.lib().omr_device_count() < 1
SYMBOLS = ("omr_deskew_with_projections_batch_streams", "omr_deskew_with_projections_batch_streams_png")
i64p = C.POINTER(C.c_int64)


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


def _with_size(jpg, rows, cols):
    """the same stream with another size in its SOF0 segment"""
    at = jpg.index(b"\xff\xc0")
    return jpg[:at + 5] + struct.pack(">HH", rows, cols) + jpg[at + 9:]


def _call(symbol, streams, *, n=None, channels=3, max_angle=10, step=0.5, scale=0.5, interp=1, border=True, level=100,
          null=(), null_stream=None, negative=None):
    """the raw call; -> (rc, angles, best_idx, scan_rc, stream pointers, lengths), the outputs pre-filled with marks"""
    bufs = [np.frombuffer(bytes(s), np.uint8) if len(s) else np.zeros(1, np.uint8) for s in streams]
    m = len(bufs)
    sp = (C.c_void_p * max(m, 1))(*[b.ctypes.data for b in bufs])
    if null_stream is not None:
        sp[null_stream] = None
    ln = np.array([len(s) for s in streams] + [0], np.int64)
    if negative is not None:
        ln[negative] = -1
    ang, idx, src = np.full(max(m, 1), 7.5), np.full(max(m, 1), -9, np.int32), np.full(max(m, 1), 77, np.int32)
    ptrs = (_lib.u8p * max(m, 1))()
    lens = np.full(max(m, 1), 123, np.int64)
    bv = (C.c_uint8 * 4)(255, 255, 255, 0)
    rc = getattr(oics.lib(), symbol)(
        None if "streams" in null else sp, None if "len" in null else ln.ctypes.data_as(i64p), m if n is None else n, channels,
        max_angle, step, scale, interp, bv if border else None, level,
        None if "angles" in null else ang.ctypes.data_as(_lib.f64p), None if "best_idx" in null else idx.ctypes.data_as(_lib.i32p),
        None if "scan_rc" in null else src.ctypes.data_as(_lib.i32p), None if "out" in null else ptrs,
        None if "out_len" in null else lens.ctypes.data_as(i64p))
    return rc, ang, idx, src, ptrs, lens


def _untouched(r):
    _, ang, idx, src, ptrs, lens = r
    return (ang == 7.5).all() and (idx == -9).all() and (src == 77).all() and not any(ptrs) and (lens == 123).all()


@pytest.mark.parametrize("symbol", SYMBOLS)
def test_every_refusal_of_the_call_comes_before_any_device_work(symbol):
    good = [_jpeg(), _png()]
    refusals = [
        (dict(null=("streams",)), -5), (dict(null=("len",)), -5), (dict(null=("angles",)), -5), (dict(null=("scan_rc",)), -5),
        (dict(null_stream=1), -5), (dict(n=0), -5), (dict(n=-3), -5), (dict(negative=0), -5),
        (dict(null=("out",)), -5), (dict(null=("out_len",)), -5),   # exactly one of the two
        (dict(border=False), -5),                                   # outputs wanted, no border
        (dict(channels=2), -5), (dict(channels=4), -5), (dict(channels=0), -5),
        (dict(max_angle=0, step=0.5), -5), (dict(step=10.5), -5),   # an empty candidate range
        (dict(scale=0.0), -5), (dict(scale=-0.5), -5), (dict(scale=float("nan")), -5), (dict(scale=float("inf")), -5),
        (dict(interp=2), -213), (dict(interp=4), -213), (dict(interp=-1), -213),
    ]
    for kw, code in refusals:
        r = _call(symbol, good, **kw)
        assert r[0] == code, (kw, r[0], oics.lib().omr_last_error().decode())
        assert _untouched(r), kw
    # a shape whose deskew canvas the encoder's 32-bit offsets cannot take: refused for the whole call from the headers alone
    if symbol.endswith("_png"):
        huge = P.assemble(20000, 20000, 2, 8, P.deflate(bytes(64)))    # canvas 28285 x 28288 x 3: IDAT above 2^31 - 1 bytes
    else:
        huge = _with_size(_jpeg(), 9000, 9000)                          # canvas 12728 x 12728 x 3: 3.8 million blocks
    r = _call(symbol, [good[0], huge], max_angle=45, step=1.0)
    assert r[0] == -215 and _untouched(r), (r[0], oics.lib().omr_last_error().decode())
    # the angles-only form has no canvas: the same batch gets as far as asking for a device
    if NO_GPU:
        r = _call(symbol, [good[0], huge], max_angle=45, step=1.0, null=("out", "out_len"))
        assert r[0] == -217 and _untouched(r)
        r = _call(symbol, good)
        assert r[0] == -217 and _untouched(r)


@pytest.mark.parametrize("symbol", SYMBOLS)
def test_a_batch_of_refused_streams_returns_their_codes_and_no_stream(symbol):
    progressive = _jpeg(progressive=True)
    adam7 = _png(interlace=1)
    truncated = _jpeg()[:20]
    garbage = b"\x00\x01\x02\x03"
    streams = [progressive, adam7, truncated, garbage]
    want = []
    for s in streams:
        b = np.frombuffer(s, np.uint8)
        info = oics.lib().omr_png_info if s[:8] == P.SIGNATURE else oics.lib().omr_jpeg_info
        want.append(info(b.ctypes.data, b.size, None, None, None, None))
    assert want == [-213, -213, -5, -5]
    rc, ang, idx, src, ptrs, lens = _call(symbol, streams)
    assert rc == 0 and list(src[:4]) == want
    assert (ang[:4] == 0.0).all() and (idx[:4] == -1).all() and not any(ptrs) and (lens[:4] == 0).all()
    # the angles-only form, and without best_idx
    rc, ang, idx, src, ptrs, lens = _call(symbol, streams, null=("out", "out_len", "best_idx"), border=False)
    assert rc == 0 and list(src[:4]) == want and (ang[:4] == 0.0).all() and (idx == -9).all()


def test_gray_from_an_rgb_png_is_refused_for_that_sheet_alone():
    rgb, gray = _png(), _png(color_type=0)
    rc, ang, idx, src, ptrs, lens = _call(SYMBOLS[0], [rgb, rgb], channels=1)
    assert rc == 0 and list(src[:2]) == [-213, -213] and not any(ptrs)
    # a sheet whose working size truncates to 0 has the per-call function's code, from its header alone
    rc, ang, idx, src, ptrs, lens = _call(SYMBOLS[0], [rgb, _png(rows=1, cols=24, color_type=0)], channels=1, scale=0.5)
    assert rc == 0 and list(src[:2]) == [-213, -215] and not any(ptrs)
    if NO_GPU:   # a gray PNG beside it is accepted: the call goes on to ask for a device
        r = _call(SYMBOLS[0], [rgb, gray], channels=1)
        assert r[0] == -217 and _untouched(r)


def test_python_front_doors():
    streams = [_jpeg(progressive=True), b"\x00\x01\x02\x03"]
    ang, rc, out = projection.deskew_streams(streams, 10, 0.5, 0.5)
    assert list(rc) == [-213, -5] and out == [None, None] and (ang == 0.0).all()
    ang, idx, rc, out = projection.deskew_streams(streams, 10, 0.5, 0.5, png=True, want_idx=True)
    assert list(rc) == [-213, -5] and list(idx) == [-1, -1] and out == [None, None]
    ang, rc = projection.get_angles_from_streams(streams, 10, 0.5, 0.5, channels=1)
    assert list(rc) == [-213, -5] and (ang == 0.0).all()
    rs = open(os.path.join(ROOT, "shim", "oics", "src", "projection.rs")).read()
    for name, symbol in (("deskew_files_with_projections", SYMBOLS[0]), ("deskew_files_with_projections_png", SYMBOLS[1])):
        body = rs.split("pub fn %s(" % name)[1].split("\n}\n")[0]
        assert "ffi::%s(" % symbol in body and "imgcodecs" not in body
