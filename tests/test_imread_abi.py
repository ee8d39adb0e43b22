"""CPU-side checks of the imread layer's boundary (omr_imread_info, omr_imread_batch_device, omr_imread,
omr_orient_batch_device, omr_orient): declared in the header, the ctypes table and ffi.rs alike and exported;
omr_imread_info on every EXIF orientation in both byte orders; what is still refused; omr_jpeg_info's contract unchanged;
every argument error of the device entry points, which are all answered before any device work (the device pointers
these calls pass point nowhere)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "fuzz"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuzz_jpeg_decode as fz  # noqa: E402
import orient_ref as O  # noqa: E402
import png_ref as P  # noqa: E402
import oics  # noqa: E402
from oics import _lib, imread, jpeg  # noqa: E402

IGNORE = 128
NEW = {
    "omr_orient_batch_device": ["const uint8_t *", "int64_t", "int64_t", "int32_t", "int32_t", "uint8_t *", "int64_t", "int64_t",
                                "int32_t", "int32_t", "int32_t", "const int32_t *", "const int32_t *", "int32_t", "int32_t *"],
    "omr_orient": ["const omr_image *", "int32_t", "omr_image_owned *"],
    "omr_imread_info": ["const uint8_t *", "int64_t", "int32_t", "int32_t *", "int32_t *", "int32_t *", "int32_t *", "int32_t *"],
    "omr_imread_batch_device": ["const uint8_t * const *", "const int64_t *", "int32_t", "int32_t", "int32_t", "uint8_t *",
                                "int64_t", "int64_t", "int32_t", "int32_t", "int32_t *", "int32_t *"],
    "omr_imread": ["const uint8_t *", "int64_t", "int32_t", "int32_t", "omr_image_owned *"],
}
FAKE = C.c_void_p(0x10000)    # a device address no call below may touch
FAKE2 = C.c_void_p(0x4000000)


def _rgb(rows=37, cols=53, seed=3):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, (rows, cols, 3), dtype=np.uint8)


def _jpeg(**kw):
    return fz.make_stream(_rgb(), 90, **(kw or dict(subsampling=2)))


def _info(s, flags=0):
    b = np.frombuffer(bytes(s), np.uint8) if len(s) else np.zeros(1, np.uint8)
    out = [C.c_int32(-7) for _ in range(5)]
    rc = oics.lib().omr_imread_info(b.ctypes.data, len(s), flags, *[C.byref(v) for v in out])
    return rc, tuple(v.value for v in out)


def test_symbols_agree_everywhere():
    import gen_shim_ffi as g
    decls = {name: (ret, [t for t, _ in params]) for name, ret, params in g.parse_header()}
    L = C.CDLL(_lib.LIB_PATH)
    ffi = open(os.path.join(ROOT, "shim", "oics", "src", "ffi.rs")).read()
    assert g.render(g.parse_header()) == ffi, "ffi.rs is stale: run python tools/gen_shim_ffi.py"
    for name, args in NEW.items():
        assert decls[name] == ("int", args), (name, decls.get(name))
        assert hasattr(L, name)
        res, at = _lib.SYMBOLS[name]
        assert res is C.c_int and len(at) == len(args), name
        assert re.search(r"pub fn %s\(" % name, ffi), name
    header = open(os.path.join(ROOT, "include", "omrdeskew.h")).read()
    assert re.search(r"#define OMR_IMREAD_IGNORE_ORIENTATION 128\b", header) and _lib.OMR_IMREAD_IGNORE_ORIENTATION == 128
    assert "pub const OMR_IMREAD_IGNORE_ORIENTATION: i32 = 128;" in ffi
    # the value the shim's ImReadFlags::IgnoreOrientation stands for (imgcodecs::IMREAD_IGNORE_ORIENTATION)
    shim = open(os.path.join(ROOT, "shim", "oics", "src", "transfer.rs")).read()
    assert "ffi::omr_imread(" in shim and "ffi::omr_orient(" in shim


@pytest.mark.parametrize("little_endian", [True, False])
@pytest.mark.parametrize("code", O.CODES)
def test_info_reports_the_turned_size_and_the_code(code, little_endian):
    s = O.tag_jpeg(_jpeg(), code, little_endian)
    rc, (rows, cols, comps, orient, kind) = _info(s)
    assert rc == 0 and (rows, cols) == O.turned_shape(37, 53, code), (rc, rows, cols)
    assert (comps, orient, kind) == (3, code, _lib.OMR_IMREAD_KIND_JPEG)
    rc, (rows, cols, comps, orient, kind) = _info(s, IGNORE)
    assert rc == 0 and (rows, cols, comps, orient, kind) == (37, 53, 3, code, 0)
    assert imread.info(s) == O.turned_shape(37, 53, code) + (3, code, 0)


def test_info_without_exif_gray_and_png():
    assert _info(_jpeg()) == (0, (37, 53, 3, 1, 0))
    assert _info(_jpeg(gray=True)) == (0, (37, 53, 1, 1, 0))
    png = P.write(_rgb(), 2, 8)
    assert _info(png) == (0, (37, 53, 3, 1, _lib.OMR_IMREAD_KIND_PNG))
    assert _info(P.write(_rgb()[..., 0].copy(), 0, 8)) == (0, (37, 53, 1, 1, 1))
    assert _info(O.tag_png(png, 1)) == (0, (37, 53, 3, 1, 1))
    # the last APP1 segment that carries an orientation decides, as in the decoder's parser
    twice = O.tag_jpeg(O.tag_jpeg(_jpeg(), 6), 3)
    assert _info(twice) == (0, (53, 37, 3, 6, 0))


def test_what_is_still_refused():
    for code in (0, 9, 0xFFFF):
        for le in (True, False):
            s = O.tag_jpeg(_jpeg(), code, le)
            rc, (rows, cols, _, orient, _) = _info(s)
            assert rc == -213 and (rows, cols, orient) == (37, 53, code), (code, rc)
            assert "outside 1..8" in oics.lib().omr_last_error().decode()
            assert _info(s, IGNORE)[0] == 0      # decoded as stored: the value is never looked at
    png6 = O.tag_png(P.write(_rgb(), 2, 8), 6)
    for flags in (0, IGNORE):
        rc, (rows, cols, _, orient, kind) = _info(png6, flags)
        assert rc == -213 and (rows, cols, orient, kind) == (37, 53, 6, 1)
    assert _info(fz.make_stream(_rgb(), 90, progressive=True))[0] == -213
    assert _info(b"")[0] == -5 and _info(b"\x00" * 40)[0] == -5
    assert _info(_jpeg(), 1)[0] == -5 and _info(_jpeg(), 129)[0] == -5    # flags other than 0 / 128


def test_the_decoders_own_entry_points_keep_their_refusal():
    s = O.tag_jpeg(_jpeg(), 6)
    b = np.frombuffer(s, np.uint8)
    out = [C.c_int32(-7) for _ in range(4)]
    assert oics.lib().omr_jpeg_info(b.ctypes.data, b.size, *[C.byref(v) for v in out]) == -213
    assert (out[0].value, out[1].value) == (37, 53)
    with pytest.raises(_lib.OmrError) as e:
        jpeg.info(s)
    assert e.value.code == -213 and "imread would turn the image" in e.value.message
    with pytest.raises(_lib.OmrError) as e:
        jpeg.decode(s)                      # refused on the host, before any device work
    assert e.value.code == -213
    # ... per stream in the batch form, where a call all of whose streams are refused does no device work
    ptrs = (C.c_void_p * 1)(b.ctypes.data)
    lens = np.array([b.size], np.int64)
    size, rc = np.zeros(2, np.int32), np.zeros(1, np.int32)
    i32p = C.POINTER(C.c_int32)
    assert oics.lib().omr_jpeg_decode_batch_device(ptrs, lens.ctypes.data_as(C.POINTER(C.c_int64)), 1, 3, FAKE, 37 * 159, 159,
                                                   37, 53, size.ctypes.data_as(i32p), rc.ctypes.data_as(i32p)) == 0
    assert rc[0] == -213 and list(size) == [0, 0]


def _batch(streams, channels=3, flags=0, d_out=FAKE, stride=53 * 159, step=159, rows=53, cols=53, n=None, null=None):
    bufs = [np.frombuffer(bytes(s), np.uint8) for s in streams]
    k = len(bufs)
    ptrs = (C.c_void_p * max(k, 1))(*[b.ctypes.data for b in bufs])
    lens = np.array([b.size for b in bufs] + [0], np.int64)
    size, rc = np.full((max(k, 1), 2), -7, np.int32), np.full(max(k, 1), -7, np.int32)
    i32p = C.POINTER(C.c_int32)
    args = [ptrs, lens.ctypes.data_as(C.POINTER(C.c_int64)), k if n is None else n, channels, flags, d_out, stride, step, rows,
            cols, size.ctypes.data_as(i32p), rc.ctypes.data_as(i32p)]
    if null is not None:
        args[null] = None
    return oics.lib().omr_imread_batch_device(*args), size, rc


def test_imread_batch_argument_errors_before_any_device_work():
    good = O.tag_jpeg(_jpeg(), 6)
    assert _batch([good], n=-1)[0] == -5
    for null in (0, 1, 5, 10, 11):
        assert _batch([good], null=null)[0] == -5, null
    assert _batch([good], channels=2)[0] == -5 and _batch([good], channels=4)[0] == -5
    assert _batch([good], flags=1)[0] == -5
    assert _batch([good], rows=0)[0] == -5 and _batch([good], cols=0)[0] == -5
    assert _batch([good], step=158)[0] == -5
    assert _batch([good], stride=53 * 159 - 1)[0] == -5
    assert _batch([], n=0)[0] == 0
    # every stream refused -- a code-6 stream in a slot of its stored shape, a progressive one, a PNG with eXIf 6, a code
    # outside 1..8: per-stream codes, the call answers 0 and does no device work
    streams = [good, fz.make_stream(_rgb(), 90, progressive=True), O.tag_png(P.write(_rgb(), 2, 8), 6), O.tag_jpeg(_jpeg(), 9)]
    r, size, rc = _batch(streams, stride=37 * 159, rows=37, cols=53)
    assert r == 0 and list(rc) == [-5, -213, -213, -213] and (size == 0).all()
    # ... and with the flag the turned size no longer matters: a slot too small for the stored shape refuses it
    r, size, rc = _batch([good], flags=IGNORE, stride=53 * 111, step=111, rows=53, cols=37)
    assert r == 0 and list(rc) == [-5]


def test_imread_argument_errors_before_any_device_work():
    L = oics.lib()
    s = np.frombuffer(O.tag_jpeg(_jpeg(), 6), np.uint8)
    out = _lib.OmrImageOwned()
    assert L.omr_imread(None, 0, 3, 0, C.byref(out)) == -5
    assert L.omr_imread(s.ctypes.data, s.size, 3, 0, None) == -5
    assert L.omr_imread(s.ctypes.data, s.size, 2, 0, C.byref(out)) == -5
    assert L.omr_imread(s.ctypes.data, s.size, 3, 64, C.byref(out)) == -5
    assert L.omr_imread(s.ctypes.data, -1, 3, 0, C.byref(out)) == -5
    bad = np.frombuffer(O.tag_jpeg(_jpeg(), 9), np.uint8)
    assert L.omr_imread(bad.ctypes.data, bad.size, 3, 0, C.byref(out)) == -213
    gray_from_rgb = np.frombuffer(P.write(_rgb(), 2, 8), np.uint8)
    assert L.omr_imread(gray_from_rgb.ctypes.data, gray_from_rgb.size, 1, 0, C.byref(out)) == -213
    assert not out.data


def _orient(src=FAKE, sstride=70 * 140, sstep=140, rows=70, cols=131, dst=FAKE2, dstride=131 * 80, dstep=80, drows=131, dcols=70,
            channels=1, sizes=None, codes=(6,), n=None, out=True):
    o = np.array(codes, np.int32)
    k = o.size if n is None else n
    i32p = C.POINTER(C.c_int32)
    sz = None if sizes is None else np.ascontiguousarray(sizes, np.int32)
    res = np.full((max(o.size, 1), 2), -7, np.int32)
    rc = oics.lib().omr_orient_batch_device(src, sstride, sstep, rows, cols, dst, dstride, dstep, drows, dcols, channels,
                                            None if sz is None else sz.ctypes.data_as(i32p),
                                            o.ctypes.data_as(i32p) if o.size else None, k, res.ctypes.data_as(i32p) if out else None)
    return rc, res


def test_orient_batch_argument_errors_before_any_device_work():
    assert _orient(n=-1)[0] == -5
    assert _orient(src=None)[0] == -5 and _orient(dst=None)[0] == -5 and _orient(out=False)[0] == -5
    assert _orient(codes=(), n=1)[0] == -5                                   # null orient
    assert _orient(channels=2)[0] == -5 and _orient(channels=4)[0] == -5
    assert _orient(rows=0)[0] == -5 and _orient(dcols=0)[0] == -5
    assert _orient(sstep=130)[0] == -5 and _orient(dstep=69)[0] == -5
    assert _orient(sstride=70 * 140 - 1)[0] == -5 and _orient(dstride=131 * 80 - 1)[0] == -5
    for code in (0, 9, -1):
        assert _orient(codes=(code,))[0] == -5, code
    assert _orient(sizes=[[71, 5]])[0] == -5 and _orient(sizes=[[5, 132]])[0] == -5 and _orient(sizes=[[-1, 5]])[0] == -5
    assert _orient(sizes=[[0, 5]])[0] == -5
    # a turned image that does not fit the destination slot: 70 x 131 turned by 6 is 131 x 70
    assert _orient(drows=130, dstride=130 * 80)[0] == -5
    assert _orient(codes=(3,))[0] == -5                                      # unturned, 70 x 131 does not fit 131 x 70
    rc, res = _orient(codes=(3,), sizes=[[70, 70]], n=0)
    assert rc == 0 and (res == -7).all()
    # overlap: the destination begins inside the source's range, or the other way round
    inside = C.c_void_p(FAKE.value + 9000)
    assert _orient(dst=inside)[0] == -5 and _orient(src=inside, dst=FAKE)[0] == -5
    assert "overlap" in oics.lib().omr_last_error().decode()
    assert _orient(src=FAKE, dst=FAKE)[0] == -5
    # a batch of 0 x 0 entries alone: sizes are reported, nothing is launched
    rc, res = _orient(codes=(6, 1), sizes=[[0, 0], [0, 0]])
    assert rc == 0 and (res == 0).all()


def test_orient_argument_errors():
    from oics import transfer
    img = _rgb(5, 7)
    for code in (0, 9):
        with pytest.raises(_lib.OmrError) as e:
            transfer.orient(img, code)
        assert e.value.code == -5
    with pytest.raises(_lib.OmrError) as e:
        transfer.orient(np.zeros((5, 7, 4), np.uint8), 6)
    assert e.value.code == -5
    out = _lib.OmrImageOwned()
    assert oics.lib().omr_orient(None, 6, C.byref(out)) == -5
